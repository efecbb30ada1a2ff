// resp_out_check.cpp -- jylis_amd/csrc/jy_resp_out.hpp as plain C++, run
// sequentially.  A stand-alone program, never loaded into Python;
// tests/test_resp_exec_cpu.py builds it with the address and undefined-
// behaviour sanitizers and expects "ok".
//
// It assembles a small heartbeat the way k_resp_out.hip does -- ranges through
// row_range / host_range, an exclusive sum, first_cmd_of per connection, a byte
// copy -- and compares with replies joined per connection the obvious way.
// Every array is a heap vector of exactly its size, so the address sanitizer
// sees a rule that reads past one.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../jylis_amd/csrc/jy_resp_out.hpp"

using namespace jyrout;

static int failures = 0;
#define CHECK(cond)                                         \
  do {                                                      \
    if (!(cond)) {                                          \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
      failures++;                                           \
    }                                                       \
  } while (0)

struct Cmd {
  u32 conn, kind, phase;
  std::string reply;  // what the command answers (a write: +OK)
};

// nconn connections, the commands in stream order -> checks the assembly
static void assemble(u64 nconn, const std::vector<Cmd>& cmds) {
  const u64 ncmd = cmds.size();
  // rows: the keyed commands, stably sorted by (phase, kind); groups of equal (phase, kind)
  std::vector<u32> row_cmd;
  for (u64 k = 0; k < ncmd; k++)
    if (cmds[k].kind != JY_CMD_HOST) row_cmd.push_back((u32)k);
  for (u64 i = 1; i < row_cmd.size(); i++)  // insertion sort: stable
    for (u64 j = i; j > 0; j--) {
      const Cmd &a = cmds[row_cmd[j - 1]], &b = cmds[row_cmd[j]];
      if (a.phase < b.phase || (a.phase == b.phase && a.kind <= b.kind)) break;
      std::swap(row_cmd[j - 1], row_cmd[j]);
    }
  const u64 R = row_cmd.size();
  std::vector<u64> goffs;
  std::vector<u32> gkind;
  for (u64 r = 0; r < R; r++) {
    const Cmd& c = cmds[row_cmd[r]];
    if (r == 0 || cmds[row_cmd[r - 1]].phase != c.phase || cmds[row_cmd[r - 1]].kind != c.kind) {
      goffs.push_back(r);
      gkind.push_back(c.kind);
    }
  }
  const u64 G = gkind.size();
  goffs.push_back(R);
  // the pool: each read group's replies, then +OK, then the host answers
  std::vector<uint8_t> pool;
  std::vector<u64> ro(R + G + 1, ~0ull), gbase(G + 1, 0);
  for (u64 g = 0; g < G; g++) {
    if (!kind_reads(gkind[g])) continue;
    while (pool.size() % 8) pool.push_back(0xEE);
    gbase[g] = pool.size();
    u64 o = 0;
    for (u64 r = goffs[g]; r < goffs[g + 1]; r++) {
      ro[r + g] = o;
      const std::string& s = cmds[row_cmd[r]].reply;
      pool.insert(pool.end(), s.begin(), s.end());
      o += s.size();
    }
    ro[goffs[g + 1] + g] = o;
  }
  while (pool.size() % 8) pool.push_back(0xEE);
  const u64 ok_off = pool.size();
  pool.insert(pool.end(), kOk, kOk + kOkLen);
  while (pool.size() % 8) pool.push_back(0xEE);
  const u64 hbase = pool.size();
  std::vector<u32> hcmd;
  std::vector<u64> hoffs(1, 0);
  for (u64 k = 0; k < ncmd; k++)
    if (cmds[k].kind == JY_CMD_HOST) {
      hcmd.push_back((u32)k);
      pool.insert(pool.end(), cmds[k].reply.begin(), cmds[k].reply.end());
      hoffs.push_back(hoffs.back() + cmds[k].reply.size());
    }
  // 1: ranges
  std::vector<u64> coff(ncmd, ~0ull), clen(ncmd + 1, 0);
  for (u64 r = 0; r < R; r++) {
    const u64 g = group_of(goffs.data(), G, r);
    CHECK(goffs[g] <= r && r < goffs[g + 1]);
    const Range x = row_range(gkind[g], ok_off, gbase[g], ro.data(), r, g);
    coff[row_cmd[r]] = x.off;
    clen[row_cmd[r]] = x.len;
  }
  for (u64 h = 0; h < hcmd.size(); h++) {
    const Range x = host_range(hbase, hoffs.data(), h);
    coff[hcmd[h]] = x.off;
    clen[hcmd[h]] = x.len;
  }
  // 2: offsets
  std::vector<u64> out_offs(ncmd + 1, 0);
  for (u64 k = 0; k < ncmd; k++) out_offs[k + 1] = out_offs[k] + clen[k];
  // 3: connections
  std::vector<u32> cmd_conn(ncmd);
  for (u64 k = 0; k < ncmd; k++) cmd_conn[k] = cmds[k].conn;
  std::vector<u64> conn_offs(nconn + 1);
  for (u64 c = 0; c <= nconn; c++) conn_offs[c] = out_offs[first_cmd_of(cmd_conn.data(), ncmd, c)];
  // 4: bytes
  std::vector<uint8_t> out(out_offs[ncmd]);
  for (u64 k = 0; k < ncmd; k++) {
    CHECK(coff[k] + clen[k] <= pool.size());
    if (clen[k]) std::memcpy(out.data() + out_offs[k], pool.data() + coff[k], clen[k]);
  }
  // the obvious way
  std::vector<std::string> want(nconn);
  for (const Cmd& c : cmds) want[c.conn] += c.kind != JY_CMD_HOST && !kind_reads(c.kind) ? "+OK\r\n" : c.reply;
  CHECK(conn_offs[0] == 0 && conn_offs[nconn] == out.size());
  for (u64 c = 0; c < nconn; c++) {
    CHECK(conn_offs[c] <= conn_offs[c + 1]);
    CHECK(std::string(out.begin() + conn_offs[c], out.begin() + conn_offs[c + 1]) == want[c]);
  }
}

int main() {
  CHECK(kind_reads(JY_CMD_GCOUNT_GET) && kind_reads(JY_CMD_PNCOUNT_GET) && kind_reads(JY_CMD_TREG_GET) &&
        kind_reads(JY_CMD_TLOG_READ));
  CHECK(!kind_reads(JY_CMD_HOST) && !kind_reads(JY_CMD_GCOUNT_INC) && !kind_reads(JY_CMD_PNCOUNT_INC) &&
        !kind_reads(JY_CMD_PNCOUNT_DEC) && !kind_reads(JY_CMD_TREG_SET) && !kind_reads(JY_CMD_TLOG_WRITE));
  {  // first_cmd_of: empty connections first, last, adjacent in the middle, all
    const std::vector<u32> cc = {1, 1, 4, 4, 4, 5};
    const u64 want[] = {0, 0, 2, 2, 2, 5, 6, 6, 6};
    for (u64 c = 0; c < 9; c++) CHECK(first_cmd_of(cc.data(), cc.size(), c) == want[c]);
    const std::vector<u32> none;
    for (u64 c = 0; c < 4; c++) CHECK(first_cmd_of(none.data(), 0, c) == 0);
  }
  {  // group_of at every boundary
    const std::vector<u64> go = {0, 1, 4, 9};
    const u64 want[] = {0, 1, 1, 1, 2, 2, 2, 2, 2};
    for (u64 r = 0; r < 9; r++) CHECK(group_of(go.data(), 3, r) == want[r]);
  }
  // GET a, SET a, GET a beside SET b, GET b: rows are not in command order
  assemble(2, {{0, JY_CMD_TREG_GET, 0, "$-1\r\n"},
               {0, JY_CMD_TREG_SET, 1, ""},
               {0, JY_CMD_TREG_GET, 2, "*2\r\n$1\r\nv\r\n:7\r\n"},
               {1, JY_CMD_TREG_SET, 0, ""},
               {1, JY_CMD_TREG_GET, 1, "*2\r\n$1\r\nw\r\n:8\r\n"}});
  // host commands (one answering nothing) among keyed ones, empty connections everywhere
  assemble(7, {{1, JY_CMD_GCOUNT_INC, 0, ""},
               {1, JY_CMD_HOST, 1, "+help text\r\n"},
               {1, JY_CMD_GCOUNT_GET, 2, ":18446744073709551615\r\n"},
               {4, JY_CMD_HOST, 0, ""},
               {4, JY_CMD_TLOG_READ, 1, "*0\r\n"},
               {4, JY_CMD_TLOG_READ, 1, ":3\r\n"},
               {5, JY_CMD_PNCOUNT_GET, 0, ":-1\r\n"}});
  assemble(3, {});
  assemble(0, {});
  // only writes: every reply the shared range
  {
    std::vector<Cmd> w;
    for (u32 i = 0; i < 40; i++) w.push_back(Cmd{i / 3, (u32)JY_CMD_TLOG_WRITE, 0, ""});
    assemble(14, w);
  }
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
