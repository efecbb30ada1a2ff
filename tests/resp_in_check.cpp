// resp_in_check.cpp -- jylis_amd/csrc/jy_resp_in.hpp as plain C++, run
// sequentially.  A stand-alone program, never loaded into Python.
//
//   resp_in_check                 checks the token, number and classification
//                                 rules against expectations written out here
//                                 and prints "ok" (tests/test_resp_in_cpu.py
//                                 builds it with the address and undefined-
//                                 behaviour sanitizers)
//   resp_in_check FILE ROUNDS     FILE = u64 nconn, u64 conn_offs[nconn + 1],
//                                 the request bytes.  Frames and classifies
//                                 every connection ROUNDS times on this one
//                                 core and prints, per round, a JSON line with
//                                 the milliseconds and the command, row and
//                                 closed-connection counts: the sequential
//                                 floor tools/resp_decode_time.py compares with
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../jylis_amd/csrc/jy_resp_in.hpp"

using namespace jyrin;

static int failures = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);             \
      failures++;                                                       \
    }                                                                   \
  } while (0)

// the token at the start of s, judged in a buffer of exactly s.size() bytes
// (a heap copy: the address sanitizer sees any read past `avail`)
static Token tok(const std::string& s) {
  std::vector<uint8_t> b(s.begin(), s.end());
  return token_at(b.data(), b.size());
}

static bool u64_of(const std::string& s, u64* v) {
  std::vector<uint8_t> b(s.begin(), s.end());
  return parse_u64(b.data(), b.size(), v);
}
static bool i64_of(const std::string& s, int64_t* v) {
  std::vector<uint8_t> b(s.begin(), s.end());
  return parse_i64(b.data(), b.size(), v);
}

static Class cls(const std::vector<std::string>& words) {
  std::vector<std::vector<uint8_t>> keep;
  for (auto& w : words) keep.emplace_back(w.begin(), w.end());
  Word w[kWordsRead];
  for (u32 j = 0; j < kWordsRead; j++)
    w[j] = j < keep.size() ? Word{keep[j].data(), keep[j].size()} : Word{nullptr, 0};
  return classify(words.size(), w);
}

static void check_tokens() {
  // 1 and 20 digits, leading zeros, the u64 edges
  Token t = tok("*3\r\n");
  CHECK(t.status == kComplete && t.type == kHeader && t.val == 3 && t.end == 4);
  t = tok("*00000000000000000003\r\n");
  CHECK(t.status == kComplete && t.val == 3 && t.end == 23);
  t = tok("*18446744073709551615\r\n");
  CHECK(t.status == kComplete && t.val == ~0ull);
  CHECK(tok("*18446744073709551616\r\n").status == kMalformed);
  CHECK(tok("*99999999999999999999\r\n").status == kMalformed);
  CHECK(tok("*000000000000000000001\r\n").status == kMalformed);  // a 21st digit
  CHECK(tok("*000000000000000000001").status == kMalformed);
  t = tok("$5\r\nhello\r\n");
  CHECK(t.status == kComplete && t.type == kBulk && t.val == 5 && t.body == 4 && t.end == 11);
  t = tok("$0\r\n\r\n");
  CHECK(t.status == kComplete && t.val == 0 && t.body == 4 && t.end == 6);
  t = tok("$7\r\n\r\n*1\r\n$\r\n");  // binary-safe: framing bytes inside the value
  CHECK(t.status == kComplete && t.val == 7 && t.end == 13);
  // a length no buffer holds is incomplete, never followed
  t = tok("$18446744073709551615\r\nabc");
  CHECK(t.status == kIncomplete && t.type == kBulk);
  // definite violations
  CHECK(tok("$-1\r\n").status == kMalformed);
  CHECK(tok("*-1\r\n").status == kMalformed);
  CHECK(tok("*+1\r\n").status == kMalformed);
  CHECK(tok("* 1\r\n").status == kMalformed);
  CHECK(tok("*\r\n").status == kMalformed);
  CHECK(tok("*1\n").status == kMalformed);
  CHECK(tok("*1\rX").status == kMalformed);
  CHECK(tok("$3\r\nabcX\n").status == kMalformed);
  CHECK(tok("$3\r\nabc\rX").status == kMalformed);
  CHECK(tok("$3\r\nabcX").status == kMalformed);  // the byte is there and is no \r
  CHECK(tok("GET k\r\n").status == kMalformed && tok("GET k\r\n").type == kNoType);  // inline command
  CHECK(tok("+OK\r\n").status == kMalformed);
  CHECK(tok(":1\r\n").status == kMalformed);
  CHECK(tok("").status == kIncomplete && tok("").type == kNoType);
  // every proper prefix of a well-formed token is incomplete, the token itself complete
  for (const std::string& whole : {std::string("*12\r\n"), std::string("$12\r\nhello\r\nworld\r\n"),
                                  std::string("$0\r\n\r\n"), std::string("*18446744073709551615\r\n")}) {
    for (size_t n = 0; n < whole.size(); n++) {
      const Token p = tok(whole.substr(0, n));
      CHECK(p.status == kIncomplete);
      if (n > 0) CHECK(p.type == (whole[0] == '*' ? kHeader : kBulk));
    }
    CHECK(tok(whole).status == kComplete && tok(whole).end == whole.size());
    // bytes after the token do not change it
    CHECK(tok(whole + "*1\r\n").status == kComplete && tok(whole + "*1\r\n").end == whole.size());
  }
  // every single wrong byte in the framing of a token is malformed or, for a
  // digit changed into another digit, another well-formed reading
  const std::string good = "$3\r\nabc\r\n";
  for (size_t i : {size_t(0), size_t(2), size_t(3), size_t(7), size_t(8)}) {
    std::string bad = good;
    bad[i] = 'x';
    CHECK(tok(bad).status == kMalformed);
  }
}

static void check_numbers() {
  u64 v = 1;
  int64_t x = 1;
  CHECK(u64_of("0", &v) && v == 0);
  CHECK(u64_of("7", &v) && v == 7);
  CHECK(u64_of("00000000000000000042", &v) && v == 42);  // 20 digits
  CHECK(!u64_of("000000000000000000042", &v));           // 21
  CHECK(u64_of("18446744073709551615", &v) && v == ~0ull);
  CHECK(!u64_of("18446744073709551616", &v));
  CHECK(!u64_of("", &v) && !u64_of("+1", &v) && !u64_of("-1", &v) && !u64_of("1 ", &v) && !u64_of("1a", &v));
  CHECK(i64_of("0", &x) && x == 0);
  CHECK(i64_of("+5", &x) && x == 5);
  CHECK(i64_of("-5", &x) && x == -5);
  CHECK(i64_of("-0", &x) && x == 0);
  CHECK(i64_of("9223372036854775807", &x) && x == INT64_MAX);
  CHECK(i64_of("+9223372036854775807", &x) && x == INT64_MAX);
  CHECK(!i64_of("9223372036854775808", &x));
  CHECK(i64_of("-9223372036854775808", &x) && x == INT64_MIN);
  CHECK(!i64_of("-9223372036854775809", &x));
  CHECK(!i64_of("", &x) && !i64_of("-", &x) && !i64_of("+", &x) && !i64_of("--1", &x) && !i64_of("+-1", &x));
  CHECK(!i64_of("18446744073709551616", &x));
}

static void check_classes() {
  Class c = cls({"GCOUNT", "INC", "k", "18446744073709551615"});
  CHECK(c.kind == JY_CMD_GCOUNT_INC && c.num == ~0ull && c.key == 2 && c.val == -1 && c.op == 0);
  CHECK(cls({"GCOUNT", "GET", "k"}).kind == JY_CMD_GCOUNT_GET);
  CHECK(cls({"GCOUNT", "GET", "k", "extra", "words", "ignored"}).kind == JY_CMD_GCOUNT_GET);
  CHECK(cls({"GCOUNT", "DEC", "k", "1"}).kind == JY_CMD_HOST);
  CHECK(cls({"GCOUNT", "INC", "k", "-1"}).kind == JY_CMD_HOST);
  CHECK(cls({"GCOUNT", "INC", "k"}).kind == JY_CMD_HOST);
  c = cls({"PNCOUNT", "INC", "k", "-3"});
  CHECK(c.kind == JY_CMD_PNCOUNT_INC && c.num == (u64)(int64_t)-3);
  c = cls({"PNCOUNT", "DEC", "k", "+3"});
  CHECK(c.kind == JY_CMD_PNCOUNT_DEC && c.num == 3);
  CHECK(cls({"PNCOUNT", "DEC", "k", "9223372036854775808"}).kind == JY_CMD_HOST);
  CHECK(cls({"PNCOUNT", "GET", "k"}).kind == JY_CMD_PNCOUNT_GET);
  c = cls({"TREG", "SET", "k", "value", "12"});
  CHECK(c.kind == JY_CMD_TREG_SET && c.num == 12 && c.key == 2 && c.val == 3);
  CHECK(cls({"TREG", "SET", "k", "value"}).kind == JY_CMD_HOST);
  CHECK(cls({"TREG", "SET", "k", "value", "x"}).kind == JY_CMD_HOST);
  CHECK(cls({"TREG", "GET", "k"}).kind == JY_CMD_TREG_GET);
  CHECK(cls({"TREG", "GET"}).kind == JY_CMD_HOST);
  CHECK(cls({"TREG", "get", "k"}).kind == JY_CMD_HOST && cls({"treg", "GET", "k"}).kind == JY_CMD_HOST);
  c = cls({"TLOG", "INS", "k", "v", "5"});
  CHECK(c.kind == JY_CMD_TLOG_WRITE && c.op == JY_TLOG_INS && c.num == 5 && c.val == 3);
  c = cls({"TLOG", "TRIMAT", "k", "9"});
  CHECK(c.kind == JY_CMD_TLOG_WRITE && c.op == JY_TLOG_TRIMAT && c.num == 9 && c.val == -1);
  c = cls({"TLOG", "TRIM", "k", "2"});
  CHECK(c.kind == JY_CMD_TLOG_WRITE && c.op == JY_TLOG_TRIM && c.num == 2);
  c = cls({"TLOG", "CLR", "k"});
  CHECK(c.kind == JY_CMD_TLOG_WRITE && c.op == JY_TLOG_CLR);
  CHECK(cls({"TLOG", "TRIM", "k"}).kind == JY_CMD_HOST && cls({"TLOG", "TRIM", "k", "x"}).kind == JY_CMD_HOST);
  CHECK(cls({"TLOG", "INS", "k", "v"}).kind == JY_CMD_HOST);
  c = cls({"TLOG", "GET", "k"});
  CHECK(c.kind == JY_CMD_TLOG_READ && c.op == JY_TLOG_RD_GET && c.num == ~0ull);
  c = cls({"TLOG", "GET", "k", "3"});
  CHECK(c.kind == JY_CMD_TLOG_READ && c.num == 3);
  c = cls({"TLOG", "GET", "k", "many"});  // an unparsable count reads as "all"
  CHECK(c.kind == JY_CMD_TLOG_READ && c.num == ~0ull);
  c = cls({"TLOG", "SIZE", "k"});
  CHECK(c.kind == JY_CMD_TLOG_READ && c.op == JY_TLOG_RD_SIZE && c.num == 0);
  c = cls({"TLOG", "CUTOFF", "k"});
  CHECK(c.kind == JY_CMD_TLOG_READ && c.op == JY_TLOG_RD_CUTOFF);
  CHECK(cls({"UJSON", "GET", "k"}).kind == JY_CMD_HOST);
  CHECK(cls({"SYSTEM", "GETLOG"}).kind == JY_CMD_HOST);
  CHECK(cls({"NOPE", "GET", "k"}).kind == JY_CMD_HOST);
  CHECK(cls({}).kind == JY_CMD_HOST && cls({"TREG"}).kind == JY_CMD_HOST);
  // the 16 MiB rule: only the lengths are looked at
  uint8_t one = 'k';
  Word w[kWordsRead] = {{(const uint8_t*)"TREG", 4}, {(const uint8_t*)"GET", 3}, {&one, kMaxKeyedLen + 1},
                        {nullptr, 0}, {nullptr, 0}};
  CHECK(classify(3, w).kind == JY_CMD_HOST);
  w[2].len = 1;
  CHECK(classify(3, w).kind == JY_CMD_TREG_GET);
  Word s[kWordsRead] = {{(const uint8_t*)"TREG", 4}, {(const uint8_t*)"SET", 3}, {&one, 1},
                        {&one, kMaxKeyedLen + 1}, {(const uint8_t*)"1", 1}};
  CHECK(classify(5, s).kind == JY_CMD_HOST);
  s[3].len = 1;
  CHECK(classify(5, s).kind == JY_CMD_TREG_SET);
}

// ---- the sequential decoder: one connection after the other, one token after the other ----
struct Seq {
  u64 ncmd = 0, rows = 0, closed = 0, used = 0, sum = 0;
};
static void decode_conn(const uint8_t* buf, u64 start, u64 end, Seq& out) {
  u64 pos = start;
  for (;;) {
    if (pos >= end) break;
    const Token h = token_at(buf + pos, end - pos);
    if (h.type != kHeader || h.status == kMalformed) {
      out.closed++;
      break;
    }
    if (h.status != kComplete) break;
    u64 p = pos + h.end, j = 0;
    Word w[kWordsRead] = {};
    bool whole = true;
    for (; j < h.val; j++) {
      if (p >= end) {
        whole = false;
        break;
      }
      const Token b = token_at(buf + p, end - p);
      if (b.type != kBulk || b.status == kMalformed) {
        out.closed++;
        whole = false;
        break;
      }
      if (b.status != kComplete) {
        whole = false;
        break;
      }
      if (j < kWordsRead) w[j] = Word{buf + p + b.body, b.val};
      p += b.end;
    }
    if (!whole) break;
    const Class c = classify(h.val, w);
    out.ncmd++;
    if (c.kind != JY_CMD_HOST) {
      out.rows++;
      out.sum += c.num + c.kind + w[c.key].len + (c.val >= 0 ? w[c.val].len : 0);
    }
    pos = p;
  }
  out.used += pos - start;
}

static int run_file(const char* path, int rounds) {
  std::FILE* f = std::fopen(path, "rb");
  if (!f) return 2;
  u64 nconn = 0;
  if (std::fread(&nconn, 8, 1, f) != 1) return 2;
  std::vector<u64> offs(nconn + 1);
  if (std::fread(offs.data(), 8, nconn + 1, f) != nconn + 1) return 2;
  std::vector<uint8_t> buf(offs[nconn] + 1);
  if (offs[nconn] && std::fread(buf.data(), 1, offs[nconn], f) != offs[nconn]) return 2;
  std::fclose(f);
  for (int r = 0; r < rounds; r++) {
    Seq s;
    const auto t0 = std::chrono::steady_clock::now();
    for (u64 c = 0; c < nconn; c++) decode_conn(buf.data(), offs[c], offs[c + 1], s);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    std::printf("{\"ms\": %.4f, \"commands\": %llu, \"rows\": %llu, \"closed\": %llu, \"used\": %llu, \"sum\": %llu}\n",
                ms, (unsigned long long)s.ncmd, (unsigned long long)s.rows, (unsigned long long)s.closed,
                (unsigned long long)s.used, (unsigned long long)s.sum);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 3) return run_file(argv[1], std::atoi(argv[2]));
  check_tokens();
  check_numbers();
  check_classes();
  // the sequential decoder against a buffer worked out by hand
  const std::string a = "*3\r\n$4\r\nTREG\r\n$3\r\nGET\r\n$1\r\nk\r\n";          // 31 bytes
  const std::string b = "*2\r\n$6\r\nSYSTEM\r\n$6\r\nGETLOG\r\n";                // a HOST command
  const std::string buf = a + b + a.substr(0, 17) + a + "X";
  std::vector<uint8_t> heap(buf.begin(), buf.end());
  Seq s;
  decode_conn(heap.data(), 0, a.size() + b.size() + 17, s);  // two commands and an incomplete third
  CHECK(s.ncmd == 2 && s.rows == 1 && s.closed == 0 && s.used == a.size() + b.size());
  Seq e;
  decode_conn(heap.data(), a.size() + b.size() + 17, heap.size(), e);  // one command, then a violation
  CHECK(e.ncmd == 1 && e.rows == 1 && e.closed == 1 && e.used == a.size());
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
