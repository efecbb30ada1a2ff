// resp_check.cpp -- jylis_amd/csrc/jy_resp.hpp as plain C++ against snprintf
// (tests/test_get_resp_cpu.py builds this with the address and
// undefined-behaviour sanitizers and runs it as a program).
//
// For every value: the digit count, every digit, and every generated piece
// (each query head, the entry head, the entry tail) -- its length, each byte,
// and the 8-byte read at every offset, whose bytes past the piece's end must
// be 0.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../jylis_amd/csrc/jy_resp.hpp"

using jyresp::Gen;
typedef uint64_t u64;

static int fails = 0;

static void fail(const char* what, const std::string& want, u64 at) {
  if (fails++ < 20) std::printf("FAIL %s: want \"%s\" at %" PRIu64 "\n", what, want.c_str(), at);
}

static std::string fmt_u(const char* f, u64 v) {
  char buf[64];
  std::snprintf(buf, sizeof buf, f, v);
  return buf;
}

static void check_piece(const char* what, const Gen& g, const std::string& want) {
  if (jyresp::gen_len(g) != want.size()) return fail(what, want, jyresp::gen_len(g));
  const Gen back = jyresp::gen_unpack(jyresp::gen_pack(g), g.v);
  if (back.prefix != g.prefix || back.plen != g.plen || back.v != g.v) fail("pack", want, 0);
  for (size_t b = 0; b < want.size(); b++) {
    if (jyresp::gen_byte(g, (uint32_t)b) != (uint8_t)want[b]) fail(what, want, b);
    const u64 w = jyresp::gen8(g, (uint32_t)b);
    for (size_t j = 0; j < 8; j++) {
      const uint8_t have = (uint8_t)(w >> (8 * j));
      const uint8_t expect = b + j < want.size() ? (uint8_t)want[b + j] : 0;
      if (have != expect) fail(what, want, b * 8 + j);
    }
  }
}

static void check_unsigned(u64 v) {
  const std::string dec = fmt_u("%" PRIu64, v);
  if (jyresp::ndigits(v) != dec.size()) fail("ndigits", dec, jyresp::ndigits(v));
  for (size_t d = 0; d < dec.size(); d++)
    if (jyresp::digit(v, (uint32_t)d) != (uint32_t)(dec[d] - '0')) fail("digit", dec, d);
  check_piece("qhead_array", jyresp::qhead_array(v), "*" + dec + "\r\n");
  check_piece("qhead_uint", jyresp::qhead_uint(v), ":" + dec + "\r\n");
  check_piece("entry_head", jyresp::entry_head(v), "*2\r\n$" + dec + "\r\n");
  check_piece("entry_tail", jyresp::entry_tail(v), "\r\n:" + dec + "\r\n");
}

static void check_signed(int64_t x) {
  char buf[64];
  std::snprintf(buf, sizeof buf, ":%" PRId64 "\r\n", x);
  check_piece("qhead_int", jyresp::qhead_int(x), buf);
}

int main() {
  std::vector<u64> vals = {0, INT64_MAX, 1ull << 63, UINT64_MAX};
  u64 p = 1;
  for (int k = 1; k <= 19; k++) {
    p *= 10;  // 10^k
    vals.push_back(p - 1);
    vals.push_back(p);
  }
  for (u64 len : {0ull, 9ull, 10ull, 99ull, 100ull, 16777215ull}) vals.push_back(len);
  for (u64 v : vals) check_unsigned(v);

  std::vector<int64_t> sv = {0, -1, INT64_MIN, INT64_MAX};
  int64_t q = 1;
  for (int k = 1; k <= 18; k++) {
    q *= 10;  // 10^k <= 10^18 < 2^63
    sv.push_back(-q);
    sv.push_back(q);
    sv.push_back(-(q - 1));
  }
  for (u64 v : vals)
    if (v <= (u64)INT64_MAX) sv.push_back((int64_t)v);
  for (int64_t x : sv) check_signed(x);

  check_piece("qhead_nil", jyresp::qhead_nil(), "$-1\r\n");
  if (jyresp::gen_len(jyresp::gen_none()) != 0) fail("gen_none", "", jyresp::gen_len(jyresp::gen_none()));

  if (fails) {
    std::printf("%d failures\n", fails);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
