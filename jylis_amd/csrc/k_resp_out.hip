// k_resp_out.hip -- RESP execute: the receive buffers of a heartbeat's
// connections decoded, applied and answered in one call, the replies assembled
// per connection on the device (jy_resp_exec, jy_resp_replies;
// include/jylis_gpu.h "RESP execute").  The rules -- which pool range a command
// takes, where a connection's replies start -- are jy_resp_out.hpp's.
//
// The host side is the loop jylis_amd/resp_in.py (exec_resp) is: decode with
// the decoder's own core (jy_rin_plan / jy_rin_emit) into device arrays, walk
// the small group table in phase order, one keyed call per group with the
// group's slices of those arrays, the JY_CMD_HOST commands of each phase handed
// to the caller after the phase's groups.  What differs is where the replies go.
// Every reply is a byte range of ONE device pool:
//   read groups   the jy_*_get_resp cores write their reply bytes into the pool
//                 (JyRespDst: room is asked for once a group's total is known)
//                 and their offsets into one shared array
//   writes        +OK\r\n, in the pool once
//   HOST answers  collected on the host while the phases run, uploaded once
// and the assembly is four steps, none of which loops over a connection's
// commands, a group's rows or a reply's length:
//   1 ranges   k_rout_rows, a lane per row: the row's range (row_range) scattered
//              to command order through row_cmd; k_rout_host, a lane per HOST
//              command, the same for the uploaded answers
//   2 offsets  jy_scan_u64 over the lengths: out_offs[commands + 1]
//   3 conns    k_rout_conn, a lane per connection: out_offs at the first command
//              of that connection or a later one (first_cmd_of, a bisection)
//   4 bytes    k_wire_gather with ReqSrc over the pool -- a command's reply is "the
//              bytes of a buffer from off[i] on", exactly a decoded key -- so the
//              byte-balanced gather moves them and there is no copy kernel here
// jy_resp_exec_opts with JY_RESP_UJSON_GET adds one read kind: a JY_CMD_UJSON_GET
// group is one jy_ujson_get_resp_core call with the group's key and value (path)
// slices, into the pool like the others.  The queries that call leaves to the
// host (on_host = 1, an empty range) join their phase's HOST commands by command
// index and are answered through the callback; k_rout_host, launched after
// k_rout_rows, writes their ranges over the rows' empty ones.  Their flags, and
// for device input their words, come to the host only when the render's own
// count says a group left something.
// With JY_RESP_UJSON_WRITE a JY_CMD_UJSON_WRITE group (INS / RM / CLR) is one
// jy_ujson_write_keys_dev call with the group's op, key and value (leaf) slices;
// its rows take the shared +OK like every other write row.
// All stores are ordinary vector stores; there is no atomic.
//
// Roofline: launch- and latency-bound at a heartbeat's size.  Per reply byte one
// byte read from the pool and one written; per command 16 B of range written,
// 8 + 8 read back by the scan and the gather.  Times: DESIGN.md, "RESP execute".

#include <algorithm>
#include <cstring>
#include <vector>

#include "jy_resp_out.hpp"
#include "jy_wire.hpp"

struct jy_resp_sink {
  std::vector<uint8_t>* bytes;
};

namespace {

// the device tables of one assembly, uploaded in one piece behind the answers
struct Plan {
  const u64* goffs;      // [G + 1] rows of group g
  const u64* gbase;      // [G] where a read group's reply bytes start in the pool
  const uint8_t* gkind;  // [G]
  const u64* hoffs;      // [H + 1] the HOST answers, back to back from hbase
  const u32* hcmd;       // [H] the command each answers
  u64 G, H, ok_off, hbase;
};

// ---- 1: ranges ----
__global__ __launch_bounds__(kThreads) void k_rout_rows(Plan P, const u64* __restrict__ ro,
                                                        const u32* __restrict__ row_cmd, u64 R, u64 ncmd,
                                                        u64* __restrict__ coff, u64* __restrict__ clen) {
  const u64 r = gid();
  if (r >= R) return;
  const u64 g = jyrout::group_of(P.goffs, P.G, r);
  const jyrout::Range x = jyrout::row_range(P.gkind[g], P.ok_off, P.gbase[g], ro, r, g);
  const u64 k = row_cmd[r];
  if (k >= ncmd) return;  // never: the decoder's rows name its commands
  coff[k] = x.off;
  clen[k] = x.len;
}

// lane H closes the lengths for the scan
__global__ __launch_bounds__(kThreads) void k_rout_host(Plan P, u64 ncmd, u64* __restrict__ coff,
                                                        u64* __restrict__ clen) {
  const u64 h = gid();
  if (h > P.H) return;
  if (h == P.H) {
    clen[ncmd] = 0;
    return;
  }
  const jyrout::Range x = jyrout::host_range(P.hbase, P.hoffs, h);
  const u64 k = P.hcmd[h];
  if (k >= ncmd) return;
  coff[k] = x.off;
  clen[k] = x.len;
}

// ---- 3: connection offsets (lane nconn: the total) ----
__global__ __launch_bounds__(kThreads) void k_rout_conn(const u32* __restrict__ cmd_conn, u64 ncmd,
                                                        const u64* __restrict__ out_offs, u64 nconn,
                                                        u64* __restrict__ conn_offs) {
  const u64 c = gid();
  if (c > nconn) return;
  conn_offs[c] = out_offs[jyrout::first_cmd_of(cmd_conn, ncmd, c)];
}

inline u64 up8(u64 x) { return (x + 7) & ~7ull; }

// the pool of one call: freed with it
struct Pool : JyRespDst {
  explicit Pool(jy_engine* e) { eng = e; }
  ~Pool() { jy_dev_free(eng, p); }
};

template <class T>
int32_t keep(jy_engine* eng, T** out, u64 count, const char* what) {
  void* p = nullptr;
  JY_TRY(jy_dev_alloc(eng, &p, count * sizeof(T) + 16, what));
  *out = static_cast<T*>(p);
  return JY_OK;
}

}  // namespace

// room for `bytes` more at an 8-byte offset of the pool; a pool that has to
// grow is copied in stream order, so offsets into it stay good and pointers do not
int32_t jy_resp_dst_reserve(JyRespDst* d, u64 bytes, uint8_t** at) {
  jy_engine* eng = d->eng;
  const u64 start = up8(d->used), need = start + bytes + 8;
  if (need > d->cap) {
    const u64 ncap = std::max<u64>(std::max<u64>(need, 2 * d->cap), 4096);
    void* np = nullptr;
    JY_TRY(jy_dev_alloc(eng, &np, ncap + 16, "reply pool"));
    if (d->used) JY_HIP(eng, hipMemcpyAsync(np, d->p, d->used, hipMemcpyDeviceToDevice, eng->stream));
    jy_dev_free(eng, d->p);
    d->p = static_cast<uint8_t*>(np);
    d->cap = ncap;
  }
  d->at = start;
  d->used = start + bytes;
  *at = d->p + start;
  return JY_OK;
}

void jy_resp_kept_free(jy_engine* eng) {
  jy_engine::RespKept& K = eng->resp_kept;
  jy_dev_free(eng, K.bytes);
  jy_dev_free(eng, K.offs);
  jy_dev_free(eng, K.used);
  jy_dev_free(eng, K.err);
  K = jy_engine::RespKept{};
}

static int32_t resp_exec_body(jy_engine* eng, uint64_t nconn, const uint8_t* req_bytes, int32_t req_mem,
                              const uint64_t* conn_offs, uint64_t identity, jy_resp_host_fn on_host, void* ctx,
                              uint32_t flags, uint64_t* sizes_out, uint64_t* uj_sizes);

extern "C" {

int32_t jy_resp_sink_write(jy_resp_sink* sink, const uint8_t* bytes, uint64_t n) {
  if (!sink || (n && !bytes)) return JY_EINVAL;
  sink->bytes->insert(sink->bytes->end(), bytes, bytes + n);
  return JY_OK;
}

int32_t jy_resp_exec(jy_engine* eng, uint64_t nconn, const uint8_t* req_bytes, int32_t req_mem,
                     const uint64_t* conn_offs, uint64_t identity, jy_resp_host_fn on_host, void* ctx,
                     uint64_t* sizes_out) {
  return resp_exec_body(eng, nconn, req_bytes, req_mem, conn_offs, identity, on_host, ctx, 0, sizes_out, nullptr);
}

int32_t jy_resp_exec_opts(jy_engine* eng, uint64_t nconn, const uint8_t* req_bytes, int32_t req_mem,
                          const uint64_t* conn_offs, uint64_t identity, jy_resp_host_fn on_host, void* ctx,
                          uint32_t flags, uint64_t* sizes_out) {
  sizes_out[6] = sizes_out[7] = 0;
  return resp_exec_body(eng, nconn, req_bytes, req_mem, conn_offs, identity, on_host, ctx, flags, sizes_out,
                        sizes_out + 6);
}

}  // extern "C"

// sizes_out[6] as jy_resp_exec's; uj_sizes (jy_resp_exec_opts) = {UJSON GETs rendered on the device, left to on_host}
static int32_t resp_exec_body(jy_engine* eng, uint64_t nconn, const uint8_t* req_bytes, int32_t req_mem,
                              const uint64_t* conn_offs, uint64_t identity, jy_resp_host_fn on_host, void* ctx,
                              uint32_t flags, uint64_t* sizes_out, uint64_t* uj_sizes) {
  JY_HIP(eng, hipSetDevice(eng->device));
  for (int q = 0; q < 6; q++) sizes_out[q] = 0;
  jy_resp_kept_free(eng);  // a failed call retains nothing
  jy_engine::RespKept N;   // what this call will retain
  struct Undo {            // ... unless it fails on the way
    jy_engine* eng;
    jy_engine::RespKept* n;
    ~Undo() {
      if (!n) return;
      jy_dev_free(eng, n->bytes);
      jy_dev_free(eng, n->offs);
      jy_dev_free(eng, n->used);
      jy_dev_free(eng, n->err);
    }
  } undo{eng, &N};
  const auto retain = [&]() {
    N.valid = true;
    eng->resp_kept = N;
    undo.n = nullptr;
    return JY_OK;
  };
  N.nconn = nconn;
  if (req_mem != JY_HOST && req_mem != JY_DEVICE) return eng->fail(JY_EINVAL, "req_mem must be JY_HOST or JY_DEVICE");
  if (nconn >= 0xFFFFFFFFull) return eng->fail(JY_ERANGE, "more than 2^32 - 1 connections in one call");
  JY_TRY(keep(eng, &N.offs, nconn + 1, "connection reply offsets"));
  JY_TRY(keep(eng, &N.used, nconn, "connection bytes used"));
  JY_TRY(keep(eng, &N.err, nconn, "connection verdicts"));
  JY_HIP(eng, hipMemsetAsync(N.offs, 0, (nconn + 1) * 8, eng->stream));
  if (nconn == 0) return retain();
  if (!conn_offs) return eng->fail(JY_EINVAL, "conn_offs is null");

  // ---- decode: the decoder's core, its outputs in device memory ----
  JyRinPlan* plan;
  u64 dsz[6];
  JY_TRY(jy_rin_plan(eng, nconn, req_bytes, req_mem, conn_offs, &plan, dsz, flags));
  struct Drop {
    JyRinPlan* p;
    ~Drop() { jy_rin_free(p); }
  } drop{plan};
  const u64 ncmd = dsz[0], W = dsz[1], R = dsz[2], kbytes = dsz[3], vbytes = dsz[4], G = dsz[5], H = ncmd - R;
  sizes_out[0] = ncmd;
  sizes_out[2] = H;
  if (H && !on_host) return eng->fail(JY_EINVAL, "the batch has JY_CMD_HOST commands and on_host is null");
  Tmp tmp(eng);
  JyRinOut D{};
  D.conn_used = N.used;
  D.conn_err = N.err;
  JY_TRY(tmp.get(&D.cmd_conn, ncmd));
  JY_TRY(tmp.get(&D.cmd_kind, ncmd));
  JY_TRY(tmp.get(&D.cmd_phase, ncmd));
  JY_TRY(tmp.get(&D.cmd_word_offs, ncmd + 1));
  JY_TRY(tmp.get(&D.word_off, W));
  JY_TRY(tmp.get(&D.word_len, W));
  JY_TRY(tmp.get(&D.row_cmd, R));
  JY_TRY(tmp.get(&D.key_bytes, kbytes));
  JY_TRY(tmp.get(&D.key_offs, R + 1));
  JY_TRY(tmp.get(&D.val_bytes, vbytes));
  JY_TRY(tmp.get(&D.val_offs, R + 1));
  JY_TRY(tmp.get(&D.num, R));
  JY_TRY(tmp.get(&D.op, R));
  std::vector<u32> gphase(G + 1);
  std::vector<uint8_t> gkind(G + 1);
  std::vector<u64> goffs(G + 1, 0);
  D.group_phase = gphase.data();
  D.group_class = gkind.data();
  D.group_offs = goffs.data();
  // the command table comes to the host only for a batch that has HOST commands to answer
  std::vector<uint8_t> ckind;
  std::vector<u32> cphase;
  std::vector<u64> cwo, woff, wlen;
  if (H) {
    ckind.resize(ncmd);
    cphase.resize(ncmd);
    cwo.resize(ncmd + 1);
    woff.resize(W + 1);
    wlen.resize(W + 1);
    D.h_cmd_kind = ckind.data();
    D.h_cmd_phase = cphase.data();
    D.h_cmd_word_offs = cwo.data();
    D.h_word_off = woff.data();
    D.h_word_len = wlen.data();
  }
  JY_TRY(jy_rin_emit(eng, plan, D, JY_DEVICE));
  if (ncmd == 0) return retain();  // every range empty: the offsets are zero already

  // ---- the HOST commands in the order they are answered, and their words ----
  std::vector<u32> hcmd;
  hcmd.reserve(H);
  for (u64 k = 0; k < ncmd && H; k++)
    if (ckind[k] == JY_CMD_HOST) hcmd.push_back((u32)k);
  if (hcmd.size() != H) return eng->fail(JY_EINVAL, "resp exec: the command table is inconsistent");
  std::stable_sort(hcmd.begin(), hcmd.end(), [&](u32 a, u32 b) { return cphase[a] < cphase[b]; });
  u64 total_req = conn_offs[nconn];
  // device input: the words of `cmds`, one copy down -> bytes, and per word, in the
  // order of cmds, where it starts in them
  const auto words_down = [&](const std::vector<u32>& cmds, std::vector<uint8_t>& bytes,
                              std::vector<u64>& at_out) -> int32_t {
    std::vector<u64> src, at(1, 0);
    for (u32 k : cmds)
      for (u64 w = cwo[k]; w < cwo[k + 1]; w++) {
        if (w >= W || woff[w] > total_req || wlen[w] > total_req - woff[w])
          return eng->fail(JY_EINVAL, "resp exec: a word lies outside the request bytes");
        src.push_back(woff[w]);
        at.push_back(at.back() + wlen[w]);
      }
    const u64 nw = src.size(), nb = at.back();
    at_out = at;
    bytes.resize(nb + 1);
    if (nw && nb) {
      const void *dsrc, *dat;
      uint8_t* dw;
      JY_TRY(jy_stage_begin(eng));
      JY_TRY(jy_stage(eng, 2, src.data(), nw * 8, JY_HOST, &dsrc));
      JY_TRY(jy_stage(eng, 3, at.data(), (nw + 1) * 8, JY_HOST, &dat));
      JY_TRY(jy_stage_end(eng));
      JY_TRY(tmp.get(&dw, nb));
      JY_TRY(gather(eng, ReqSrc{req_bytes, static_cast<const u64*>(dsrc)}, static_cast<const u64*>(dat), nw, nb, dw));
      JY_HIP(eng, hipMemcpyAsync(bytes.data(), dw, nb, hipMemcpyDeviceToHost, eng->stream));
      JY_HIP(eng, hipStreamSynchronize(eng->stream));
    }
    return JY_OK;
  };
  std::vector<uint8_t> hwords;  // device input: the HOST commands' words
  std::vector<u64> hw_at;       // ... in hcmd order
  if (H && req_mem == JY_DEVICE) JY_TRY(words_down(hcmd, hwords, hw_at));
  // JY_RESP_UJSON_GET: the queries a render left to the host, answered with their phase's HOST commands
  const bool uj = flags & JY_RESP_UJSON_GET;
  bool have_words = H != 0;  // the commands' words are on the host (cwo, woff, wlen)
  uint8_t* oh_dev = nullptr;
  if (uj) JY_TRY(tmp.get(&oh_dev, R));
  std::vector<u32> left;         // this phase's, by command
  std::vector<uint8_t> lwords;   // device input: their words
  std::vector<u64> lw_at;
  std::vector<u32> acmd;         // every command answered through on_host, in the order answered
  acmd.reserve(H);
  u64 uj_dev = 0, uj_host = 0;

  // ---- the phases: keyed groups first, then the phase's HOST commands ----
  uint32_t col = 0;
  JY_TRY(jy_replica_col(eng, identity, &col));
  Pool pool(eng);
  u64* ro;  // the read groups' reply offsets: group g's at ro + goffs[g] + g
  JY_TRY(tmp.get(&ro, R + G + 1));
  std::vector<u64> gbase(G + 1, 0);
  std::vector<uint8_t> answers;
  std::vector<u64> hoffs(1, 0);
  jy_resp_sink sink{&answers};
  std::vector<const uint8_t*> wp;
  std::vector<u64> wl;
  u64 g = 0, h = 0, hw = 0, calls = 0, phases = 0;
  while (g < G || h < H) {
    const u32 phase = std::min<u32>(g < G ? gphase[g] : ~0u, h < H ? cphase[hcmd[h]] : ~0u);
    phases = (u64)phase + 1;
    for (; g < G && gphase[g] == phase; g++) {
      const u64 a = goffs[g], n = goffs[g + 1] - a;
      if (goffs[g + 1] > R || n == 0 || n > R) return eng->fail(JY_EINVAL, "resp exec: the group table is inconsistent");
      const uint8_t* kb = D.key_bytes;
      const u64 *ko = D.key_offs + a, *vo = D.val_offs + a, *num = D.num + a;
      pool.reply_offs = ro + a + g;
      u64 sz[3];
      int32_t rc;
      switch (gkind[g]) {
        case JY_CMD_GCOUNT_INC: rc = jy_counter_write_keys(eng, JY_GCOUNT, 0, col, n, kb, ko, num, JY_DEVICE); break;
        case JY_CMD_PNCOUNT_INC: rc = jy_counter_write_keys(eng, JY_PNCOUNT, 0, col, n, kb, ko, num, JY_DEVICE); break;
        case JY_CMD_PNCOUNT_DEC: rc = jy_counter_write_keys(eng, JY_PNCOUNT, 1, col, n, kb, ko, num, JY_DEVICE); break;
        case JY_CMD_TREG_SET: rc = jy_treg_set_keys(eng, n, kb, ko, num, D.val_bytes, vo, JY_DEVICE); break;
        case JY_CMD_TLOG_WRITE:
          rc = jy_tlog_write_keys(eng, n, D.op + a, kb, ko, num, num, D.val_bytes, vo, JY_DEVICE);
          break;
        case JY_CMD_GCOUNT_GET:
          rc = jy_counter_get_resp_core(eng, JY_GCOUNT, n, kb, ko, JY_DEVICE, 0, nullptr, nullptr, sz, JY_DEVICE, &pool);
          break;
        case JY_CMD_PNCOUNT_GET:
          rc = jy_counter_get_resp_core(eng, JY_PNCOUNT, n, kb, ko, JY_DEVICE, 0, nullptr, nullptr, sz, JY_DEVICE, &pool);
          break;
        case JY_CMD_TREG_GET:
          rc = jy_treg_get_resp_core(eng, n, kb, ko, JY_DEVICE, 0, nullptr, nullptr, sz, JY_DEVICE, &pool);
          break;
        case JY_CMD_TLOG_READ:
          rc = jy_tlog_get_resp_core(eng, n, kb, ko, JY_DEVICE, D.op + a, num, JY_DEVICE, 0, nullptr, nullptr, sz,
                                     JY_DEVICE, &pool);
          break;
        case JY_CMD_UJSON_GET: {
          if (!uj) {
            rc = eng->fail(JY_EINVAL, "resp exec: a group of an unknown kind");
            break;
          }
          // one render for the group: keys and paths are its slices of the decoded columns
          u64 usz[6];
          rc = jy_ujson_get_resp_core(eng, n, nullptr, kb, ko, JY_DEVICE, D.val_bytes, vo, 0, nullptr, nullptr,
                                      oh_dev + a, usz, JY_DEVICE, &pool);
          if (rc != JY_OK) break;
          const u64 nleft = usz[4];
          if (nleft > n) return eng->fail(JY_EINVAL, "resp exec: the render's counts are inconsistent");
          if (nleft) {
            if (!on_host)
              return eng->fail(JY_EINVAL, "a UJSON GET is left to the host (a key to escape, a leaf too deep) and "
                                          "on_host is null");
            // which ones, and (once) where every command's words are
            std::vector<uint8_t> oh(n);
            std::vector<u32> rc_cmd(n);
            JY_HIP(eng, hipMemcpyAsync(oh.data(), oh_dev + a, n, hipMemcpyDeviceToHost, eng->stream));
            JY_HIP(eng, hipMemcpyAsync(rc_cmd.data(), D.row_cmd + a, n * 4, hipMemcpyDeviceToHost, eng->stream));
            if (!have_words) {
              cwo.resize(ncmd + 1);
              woff.resize(W + 1);
              wlen.resize(W + 1);
              JY_HIP(eng, hipMemcpyAsync(cwo.data(), D.cmd_word_offs, (ncmd + 1) * 8, hipMemcpyDeviceToHost, eng->stream));
              JY_HIP(eng, hipMemcpyAsync(woff.data(), D.word_off, W * 8, hipMemcpyDeviceToHost, eng->stream));
              JY_HIP(eng, hipMemcpyAsync(wlen.data(), D.word_len, W * 8, hipMemcpyDeviceToHost, eng->stream));
            }
            JY_HIP(eng, hipStreamSynchronize(eng->stream));
            have_words = true;
            for (u64 i = 0; i < n; i++)
              if (oh[i]) {
                if (rc_cmd[i] >= ncmd || (!left.empty() && rc_cmd[i] <= left.back()))
                  return eng->fail(JY_EINVAL, "resp exec: the row table is inconsistent");
                left.push_back(rc_cmd[i]);  // rows keep stream order inside a group: ascending
              }
            if (left.size() != nleft) return eng->fail(JY_EINVAL, "resp exec: the render's counts are inconsistent");
            if (req_mem == JY_DEVICE) JY_TRY(words_down(left, lwords, lw_at));  // those commands' words only
          }
          uj_dev += n - nleft;
          uj_host += nleft;
          break;
        }
        case JY_CMD_UJSON_WRITE:
          // one keyed write for the group: ops, keys and leaves are its slices of the decoded columns
          rc = (flags & JY_RESP_UJSON_WRITE)
                   ? jy_ujson_write_keys_dev(eng, n, D.op + a, kb, ko, D.val_bytes, vo, col, false)
                   : eng->fail(JY_EINVAL, "resp exec: a group of an unknown kind");
          break;
        default: rc = eng->fail(JY_EINVAL, "resp exec: a group of an unknown kind");
      }
      if (rc != JY_OK) return rc;
      if (uj_sizes) uj_sizes[0] = uj_dev, uj_sizes[1] = uj_host;
      if (jyrout::kind_reads(gkind[g])) gbase[g] = pool.at;
      calls++;
      sizes_out[3] = g + 1;
      sizes_out[4] = calls;
    }
    // the phase's HOST commands and the UJSON GETs its render left, merged by command index
    for (u64 li = 0, lw = 0; (h < H && cphase[hcmd[h]] == phase) || li < left.size();) {
      const bool mine = li < left.size() && !(h < H && cphase[hcmd[h]] == phase && hcmd[h] < left[li]);
      const u32 k = mine ? left[li++] : hcmd[h++];
      const u64 w0 = cwo[k], nw = cwo[k + 1] - w0;
      wp.assign(nw + 1, nullptr);
      wl.assign(nw + 1, 0);
      for (u64 j = 0; j < nw; j++) {
        if (req_mem == JY_DEVICE) {
          const std::vector<uint8_t>& wb = mine ? lwords : hwords;
          const std::vector<u64>& at = mine ? lw_at : hw_at;
          u64& q = mine ? lw : hw;
          wp[j] = wb.data() + at[q];
          wl[j] = at[q + 1] - at[q];
          q++;
        } else {
          if (w0 + j >= W || woff[w0 + j] > total_req || wlen[w0 + j] > total_req - woff[w0 + j])
            return eng->fail(JY_EINVAL, "resp exec: a word lies outside the request bytes");
          wp[j] = req_bytes + woff[w0 + j];
          wl[j] = wlen[w0 + j];
        }
      }
      if (on_host(ctx, k, nw, wp.data(), wl.data(), &sink) != 0)
        return eng->fail(JY_EINVAL, "resp exec: on_host failed for command " + std::to_string(k));
      hoffs.push_back(answers.size());
      acmd.push_back(k);
    }
    left.clear();
  }
  sizes_out[5] = phases;
  const u64 HA = acmd.size();  // H and the UJSON GETs left to the host

  // ---- one upload: +OK, the answers, the assembly's tables ----
  const u64 o_ans = 8, o_hoffs = up8(o_ans + answers.size()), o_goffs = o_hoffs + (HA + 1) * 8,
            o_gbase = o_goffs + (G + 1) * 8, o_hcmd = o_gbase + (G + 1) * 8, o_gkind = up8(o_hcmd + HA * 4),
            blob_n = up8(o_gkind + G + 1);
  std::vector<uint8_t> blob(blob_n, 0);
  std::memcpy(blob.data(), jyrout::kOk, jyrout::kOkLen);
  if (!answers.empty()) std::memcpy(blob.data() + o_ans, answers.data(), answers.size());
  std::memcpy(blob.data() + o_hoffs, hoffs.data(), (HA + 1) * 8);
  std::memcpy(blob.data() + o_goffs, goffs.data(), (G + 1) * 8);
  std::memcpy(blob.data() + o_gbase, gbase.data(), (G + 1) * 8);
  if (HA) std::memcpy(blob.data() + o_hcmd, acmd.data(), HA * 4);
  std::memcpy(blob.data() + o_gkind, gkind.data(), G + 1);
  uint8_t* dblob;
  JY_TRY(jy_resp_dst_reserve(&pool, blob_n, &dblob));
  JY_HIP(eng, hipMemcpyAsync(dblob, blob.data(), blob_n, hipMemcpyHostToDevice, eng->stream));
  Plan P;
  P.goffs = reinterpret_cast<const u64*>(dblob + o_goffs);
  P.gbase = reinterpret_cast<const u64*>(dblob + o_gbase);
  P.gkind = dblob + o_gkind;
  P.hoffs = reinterpret_cast<const u64*>(dblob + o_hoffs);
  P.hcmd = reinterpret_cast<const u32*>(dblob + o_hcmd);
  P.G = G;
  P.H = HA;
  P.ok_off = pool.at;
  P.hbase = pool.at + o_ans;

  // ---- the assembly ----
  u64 *coff, *clen, *out_offs;
  JY_TRY(tmp.get(&coff, ncmd + 1));
  JY_TRY(tmp.get(&clen, ncmd + 1));
  JY_TRY(tmp.get(&out_offs, ncmd + 1));
  if (R) LAUNCH(k_rout_rows, R, P, (const u64*)ro, (const u32*)D.row_cmd, R, ncmd, coff, clen);
  LAUNCH(k_rout_host, HA + 1, P, ncmd, coff, clen);
  JY_TRY(jy_scan_u64(eng, clen, out_offs, ncmd));
  LAUNCH(k_rout_conn, nconn + 1, (const u32*)D.cmd_conn, ncmd, (const u64*)out_offs, nconn, N.offs);
  u64 total = 0;
  JY_TRY(totals(eng, {out_offs + ncmd}, &total));  // the final total (the blob is uploaded by now)
  if (total > pool.used * (ncmd + 1)) return eng->fail(JY_EINVAL, "resp exec: the reply total is inconsistent");
  JY_TRY(keep(eng, &N.bytes, total, "connection replies"));
  JY_TRY(gather(eng, ReqSrc{pool.p, coff}, out_offs, ncmd, total, N.bytes));
  N.total = total;
  sizes_out[1] = total;
  return retain();
}

extern "C" {

int32_t jy_resp_replies(jy_engine* eng, uint64_t nconn, uint64_t cap_bytes, uint8_t* reply_bytes,
                        uint64_t* conn_reply_offs, uint64_t* conn_used, uint8_t* conn_err, uint64_t* sizes_out,
                        int32_t mem) {
  JY_HIP(eng, hipSetDevice(eng->device));
  const jy_engine::RespKept& K = eng->resp_kept;
  sizes_out[0] = K.valid ? K.total : 0;
  sizes_out[1] = K.valid ? K.nconn : 0;
  JY_TRY(mem_check(eng, mem));
  if (!K.valid) return eng->fail(JY_EINVAL, "no jy_resp_exec result is retained");
  if (nconn != K.nconn) return eng->fail(JY_EINVAL, "nconn differs from the retained jy_resp_exec call's");
  if (cap_bytes < K.total) return JY_OK;  // sizes only
  if (!conn_reply_offs || (nconn && (!conn_used || !conn_err)) || (K.total && !reply_bytes))
    return eng->fail(JY_EINVAL, "an output array is null");
  JY_TRY(emit(eng, mem, reply_bytes, K.bytes, K.total));
  JY_TRY(emit(eng, mem, conn_reply_offs, K.offs, (nconn + 1) * 8));
  JY_TRY(emit(eng, mem, conn_used, K.used, nconn * 8));
  JY_TRY(emit(eng, mem, conn_err, K.err, nconn));
  return host_sync(eng, mem);
}

}  // extern "C"
