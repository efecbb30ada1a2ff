// uj_render_check.cpp -- jylis_amd/csrc/jy_uj_render.hpp as plain C++, run
// sequentially: the leaf compare, the segment common prefix, the mask
// composition and the text a leaf owns, against the renders
// ujson_doc.render_stored_order wrote for the same leaf sets.  Built with
// -fsanitize=address,undefined (tests/test_ujson_render_cpu.py); every leaf is
// its own exact-size heap block, so a read past a leaf's end is an error.
//
// argv[1]: a case file, little-endian u32 words and raw bytes:
//   ncases, then per case: nleaves, per leaf (len, bytes), then (len, text)
// A leaf set may hold duplicates and is in no order.  Prints "ok <ncases>".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../jylis_amd/csrc/jy_leaf.hpp"
#include "../jylis_amd/csrc/jy_uj_render.hpp"

using jyuj::u32;
using jyuj::u64;

struct Leaf {
  uint8_t* p;
  u64 len;
  JyLeafBytes ld() const { return JyLeafBytes{p}; }
};

static int fail(const char* what, size_t at) {
  std::printf("FAIL %s (case %zu)\n", what, at);
  return 1;
}

struct TextOut {
  const Leaf* leaf;
  std::string* s;
  void inl(jyuj::Punct p) {
    for (u32 b = 0; b < p.len; b++) s->push_back((char)(p.bytes >> (8 * b)));
  }
  void ptr(u64 at, u64 len) { s->append(reinterpret_cast<const char*>(leaf->p) + at, len); }
  void close(bool br, u32 nb) {
    // through close8, from every offset a granule may start at
    const u32 len = jyuj::close_len(br, nb);
    std::string whole;
    for (u32 from = 0; from < len; from += 8) {
      const u64 w = jyuj::close8(br, nb, from);
      for (u32 b = 0; b < 8 && from + b < len; b++) whole.push_back((char)(w >> (8 * b)));
    }
    for (u32 from = 1; from < len; from++)
      if ((char)(jyuj::close8(br, nb, from) & 0xFF) != whole[from]) std::abort();
    s->append(whole);
  }
};

// the sequential form of what k_uj_render.hip does in parallel; false: a leaf the device leaves to the host
static bool render(std::vector<Leaf> v, std::string* text) {
  text->clear();
  std::stable_sort(v.begin(), v.end(),
                   [](const Leaf& a, const Leaf& b) { return jyuj::leaf_cmp(a.ld(), a.len, b.ld(), b.len) < 0; });
  std::vector<Leaf> u;
  for (const Leaf& x : v)
    if (u.empty() || jyuj::leaf_cmp(u.back().ld(), u.back().len, x.ld(), x.len) != 0) u.push_back(x);
  const size_t k = u.size();
  std::vector<u32> depth(k), cp(k);
  for (size_t j = 0; j < k; j++) {
    const jyuj::Shape s = jyuj::leaf_shape(u[j].ld(), u[j].len);
    if (s.bad) return false;
    depth[j] = s.depth;
    cp[j] = j ? jyuj::common_segments(u[j - 1].ld(), u[j - 1].len, u[j].ld(), u[j].len, jyuj::kRenderDepth + 1) : 0;
  }
  std::vector<u32> state(k);
  u64 run = jyuj::kMaskId;
  for (size_t j = k; j-- > 0;) {
    const bool last = j + 1 == k;
    run = jyuj::mask_compose(run, jyuj::mask_elem(depth[j], last, last ? 0 : cp[j + 1]));
    state[j] = jyuj::mask_state(run);
  }
  for (size_t j = 0; j < k; j++) {
    jyuj::Place p;
    p.first = j == 0;
    p.last = j + 1 == k;
    p.cp = cp[j];
    p.depth = depth[j];
    p.cs = p.last ? 0 : cp[j + 1];
    p.dnext = p.last ? 0 : depth[j + 1];
    p.state = state[j];
    TextOut out{&u[j], text};
    jyuj::leaf_text(u[j].ld(), u[j].len, p, out);
  }
  return true;
}

static Leaf make_leaf(const std::string& b) {
  Leaf l{static_cast<uint8_t*>(std::malloc(b.size() ? b.size() : 1)), b.size()};
  std::memcpy(l.p, b.data(), b.size());
  return l;
}
static std::string seg(const std::string& k) {
  const u32 n = (u32)k.size();
  std::string s{(char)n, (char)(n >> 8), (char)(n >> 16), (char)(n >> 24)};
  return s + k;
}

// what no case file reaches: the composition's laws and the limits
static int self_checks() {
  // associative, not commutative, kMaskId neutral on both sides
  u64 x = 88172645463325252ull;
  auto next = [&] {
    x ^= x << 13, x ^= x >> 7, x ^= x << 17;
    return ((x % 33) << 32) | ((x >> 8) & 0xFFFFFFFFull);
  };
  bool differs = false;
  for (int i = 0; i < 20000; i++) {
    const u64 a = next(), b = next(), c = next();
    if (jyuj::mask_compose(jyuj::mask_compose(a, b), c) != jyuj::mask_compose(a, jyuj::mask_compose(b, c)))
      return fail("mask_compose is not associative", i);
    if (jyuj::mask_compose(jyuj::kMaskId, a) != a || jyuj::mask_compose(a, jyuj::kMaskId) != a)
      return fail("kMaskId is not neutral", i);
    differs = differs || jyuj::mask_compose(a, b) != jyuj::mask_compose(b, a);
  }
  if (!differs) return fail("mask_compose looks commutative", 0);
  // depth kRenderDepth renders, one more does not; the key bytes left to the host
  for (u32 d : {jyuj::kRenderDepth - 1, jyuj::kRenderDepth, jyuj::kRenderDepth + 1}) {
    std::string b;
    for (u32 i = 0; i < d; i++) b += seg("k");
    Leaf l = make_leaf(b + "\xff\xff\xff\xff" + "1");
    const jyuj::Shape s = jyuj::leaf_shape(l.ld(), l.len);
    std::free(l.p);
    if ((s.bad != 0) != (d > jyuj::kRenderDepth)) return fail("depth limit", d);
    if (!s.bad && (s.depth != d || s.vstart != l.len - 1)) return fail("depth or value start", d);
  }
  for (int c = 0; c < 256; c++) {
    Leaf l = make_leaf(seg(std::string("ab") + (char)c + "cdefghij") + "\xff\xff\xff\xff" + "\"\\\x01\"");
    const jyuj::Shape s = jyuj::leaf_shape(l.ld(), l.len);
    std::free(l.p);
    if ((s.bad != 0) != (c < 0x20 || c == '"' || c == '\\')) return fail("key byte", (size_t)c);
  }
  // malformed encodings stay inside their bytes and are left to the host
  for (const std::string& b : {std::string(""), std::string("\x01\x00\x00"), seg("abc").substr(0, 6),
                               seg("abc"), seg("abc") + "\xff\xff\xff"}) {
    Leaf l = make_leaf(b);
    const bool bad = jyuj::leaf_shape(l.ld(), l.len).bad;
    std::free(l.p);
    if (!bad) return fail("a malformed leaf was accepted", b.size());
  }
  return 0;
}

int main(int argc, char** argv) {
  if (self_checks()) return 1;
  if (argc < 2) {
    std::printf("ok 0\n");
    return 0;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return fail("cannot open the case file", 0);
  std::vector<uint8_t> raw;
  uint8_t buf[65536];
  for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) raw.insert(raw.end(), buf, buf + n);
  std::fclose(f);
  size_t at = 0;
  auto word = [&]() -> u32 {
    if (at + 4 > raw.size()) std::abort();
    u32 w;
    std::memcpy(&w, raw.data() + at, 4);
    at += 4;
    return w;
  };
  auto bytes = [&](u32 n) {
    if (at + n > raw.size()) std::abort();
    std::string s(reinterpret_cast<const char*>(raw.data()) + at, n);
    at += n;
    return s;
  };
  const u32 ncases = word();
  for (u32 c = 0; c < ncases; c++) {
    std::vector<Leaf> v;
    const u32 nl = word();
    for (u32 i = 0; i < nl; i++) v.push_back(make_leaf(bytes(word())));
    const std::string want = bytes(word());
    std::string got;
    const bool ok = render(v, &got);
    for (Leaf& l : v) std::free(l.p);
    if (!ok) return fail("a leaf was left to the host", c);
    if (got != want) {
      std::printf("got  %s\nwant %s\n", got.c_str(), want.c_str());
      return fail("the text differs", c);
    }
  }
  if (at != raw.size()) return fail("trailing bytes in the case file", ncases);
  std::printf("ok %u\n", ncases);
  return 0;
}
