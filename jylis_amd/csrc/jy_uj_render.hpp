// jy_uj_render.hpp -- the rules of a UJSON render in stored order, shared by
// the device (k_uj_render.hip) and the host (tests/uj_render_check.cpp runs
// them sequentially as plain C++ under the sanitizers).  __host__ __device__
// functions only, no HIP calls.
//
// A query's leaves are the distinct encodings relative to its path,
//     len|segment ... FF FF FF FF value         (jy_leaf.hpp)
// ordered by unsigned byte compare of the whole encoding, a proper prefix
// first.  Under one node that puts the children first, in the byte order of
// their encoded segment (the four length bytes as stored, then the key), and
// the node's own values after them in the byte order of their text: the
// terminator sorts above every segment length below 2^24.  All leaves under a
// node are contiguous.
//
// The text of a node: `{"k":<child>,...}` if it has children, then each of its
// values verbatim; one item renders bare, several as `[item,item,...]`.
// jylis_amd/ujson_doc.py states the same rule as render_stored_order.
//
// Per ordered leaf j of depth d (its segments), with cp = the segments it
// shares with its predecessor and cs = those it shares with its successor
// inside the query, the text it OWNS is
//     ,            unless it is the query's first
//     "key":       for every level it opens (segments cp + 1 .. d; a first
//                  leaf: 1 .. d), each node it opens through a child led by
//                  `{`, and by `[` before that if the node is a set
//     [            if its own node opens here and holds a second value
//     value
//     ]            if its own node ends here and held another item
//     }            for every level that ends with it, and one more if its
//                  successor is a value of the node at level cs
// Everything is local to (predecessor, leaf, successor) but one fact: whether
// a node a leaf opens through a child has values of its own, which lie at the
// END of the node's range.  That is the state of a right-to-left composition
// over the leaves (mask_elem / mask_compose): bit t of a leaf's state says the
// node at level t of its path has own values at or to the right of it.
//
// Leaves deeper than kRenderDepth and keys that would need escaping are not
// rendered on the device (leaf_shape reports them; the query goes to the host).
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define JY_UJR_HD __host__ __device__ inline
#else
#define JY_UJR_HD inline
#endif

namespace jyuj {

typedef uint64_t u64;
typedef uint32_t u32;

constexpr u32 kRenderDepth = 31;  // bit t of a u32 ancestor mask, t <= 31
constexpr u32 kTerm = 0xFFFFFFFFu;

// A leaf's bytes are read through ld(i, m): bytes i .. i + m - 1 (m <= 8,
// inside the leaf) as a little-endian word, zero above them (the device reads
// aligned words, jy_ld8u; the host a byte at a time, JyLeafBytes of jy_leaf.hpp).

JY_UJR_HD u64 bswap(u64 x) { return __builtin_bswap64(x); }

// unsigned byte compare of two whole encodings, a proper prefix first: < 0, 0, > 0
template <class LdA, class LdB>
JY_UJR_HD int leaf_cmp(LdA a, u64 alen, LdB b, u64 blen) {
  const u64 n = alen < blen ? alen : blen;
  for (u64 i = 0; i < n; i += 8) {
    const u64 m = n - i < 8 ? n - i : 8;
    const u64 wa = a(i, m), wb = b(i, m);
    if (wa != wb) return bswap(wa) < bswap(wb) ? -1 : 1;  // the first differing byte decides
  }
  return alen < blen ? -1 : alen > blen ? 1 : 0;
}

// a key byte the device does not render: it would need escaping between quotes
JY_UJR_HD bool key_byte_bad(u32 c) { return c < 0x20u || c == 0x22u || c == 0x5Cu; }

struct Shape {
  u32 depth;   // segments before the terminator (counted up to kRenderDepth + 1)
  u32 bad;     // not rendered here: too deep, a key byte to escape, or no well-formed encoding
  u64 vstart;  // where the value text starts (bad == 0)
};
// walks the segments of a (relative) leaf of `len` checked bytes
template <class Ld>
JY_UJR_HD Shape leaf_shape(Ld ld, u64 len) {
  Shape s{0, 0, 0};
  u64 at = 0;
  for (;;) {
    if (len - at < 4) return Shape{s.depth, 1, 0};
    const u32 w = (u32)ld(at, 4);
    at += 4;
    if (w == kTerm) {
      s.vstart = at;
      return s;
    }
    if (w > len - at || s.depth == kRenderDepth) return Shape{s.depth + 1, 1, 0};
    for (u64 i = 0; i < w; i += 8) {
      const u64 m = w - i < 8 ? w - i : 8;
      const u64 x = ld(at + i, m);
      for (u64 b = 0; b < m; b++)
        if (key_byte_bad((u32)(x >> (8 * b)) & 0xFFu)) s.bad = 1;
    }
    at += w;
    s.depth++;
  }
}

// the leading segments two well-formed leaves share (at most `cap`)
template <class LdA, class LdB>
JY_UJR_HD u32 common_segments(LdA a, u64 alen, LdB b, u64 blen, u32 cap) {
  const u64 n = alen < blen ? alen : blen;
  u64 at = 0;
  u32 c = 0;
  while (c < cap && n - at >= 4) {
    const u32 wa = (u32)a(at, 4), wb = (u32)b(at, 4);
    if (wa != wb || wa == kTerm || wa > n - at - 4) return c;
    at += 4;
    for (u64 i = 0; i < wa; i += 8) {
      const u64 m = wa - i < 8 ? wa - i : 8;
      if (a(at + i, m) != b(at + i, m)) return c;
    }
    at += wa;
    c++;
  }
  return c;
}

// ---- the ancestor mask: (keep, set) pairs composed right to left ----
// A word is keep << 32 | set: the low `keep` (0 .. 32) bits of the state to its
// right survive, then `set` is added.  A leaf keeps the levels it shares with
// its successor (cs + 1 of them: the root is level 0) and sets its own depth;
// the last leaf of a query keeps nothing, which is the reset at a query's end.
constexpr u64 kMaskId = 32ull << 32;  // keeps everything, sets nothing
JY_UJR_HD u32 low_bits(u32 k) { return k >= 32 ? 0xFFFFFFFFu : (1u << k) - 1u; }
JY_UJR_HD u64 mask_elem(u32 depth, bool last, u32 cs) {
  const u32 d = depth > kRenderDepth ? kRenderDepth : depth;
  return ((u64)(last ? 0u : cs + 1u) << 32) | (1ull << d);
}
// `right` is everything to the right of `left`, already composed: NOT commutative
JY_UJR_HD u64 mask_compose(u64 right, u64 left) {
  const u32 kr = (u32)(right >> 32), kl = (u32)(left >> 32);
  const u32 set = ((u32)right & low_bits(kl)) | (u32)left;
  return ((u64)(kr < kl ? kr : kl) << 32) | set;
}
JY_UJR_HD u32 mask_state(u64 word) { return (u32)word; }

// ---- generated punctuation ----
struct Punct {
  u64 bytes;  // byte b in bits [8b, 8b + 8)
  u32 len;    // 0 .. 5
};
JY_UJR_HD Punct punct_add(Punct p, u32 c) { return Punct{p.bytes | ((u64)c << (8 * p.len)), p.len + 1}; }
// before a key: `":` closing the key before it, then `,` (a further child of a
// node already open) or `{` (a node opened here, led by `[` if it is a set), then `"`
JY_UJR_HD Punct key_glue(bool after_key, bool comma, bool bracket) {
  Punct p{0, 0};
  if (after_key) p = punct_add(punct_add(p, '"'), ':');
  if (comma) p = punct_add(p, ',');
  else {
    if (bracket) p = punct_add(p, '[');
    p = punct_add(p, '{');
  }
  return punct_add(p, '"');
}
// before a value: `":` closing the last key, `,` (a further value of an open node), `[`
JY_UJR_HD Punct value_glue(bool after_key, bool comma, bool bracket) {
  Punct p{0, 0};
  if (after_key) p = punct_add(punct_add(p, '"'), ':');
  if (comma) p = punct_add(p, ',');
  if (bracket) p = punct_add(p, '[');
  return p;
}
// after a value: `]` (bracket) then nb <= kRenderDepth + 1 times `}`
JY_UJR_HD u32 close_len(bool bracket, u32 nb) { return (bracket ? 1u : 0u) + nb; }
// its bytes [from, from + 8), from < close_len; bytes past its end read as 0
JY_UJR_HD u64 close8(bool bracket, u32 nb, u32 from) {
  const u32 len = close_len(bracket, nb);
  u64 w = 0;
  for (u32 b = 0; b < 8 && from + b < len; b++)
    w |= (u64)(bracket && from + b == 0 ? ']' : '}') << (8 * b);
  return w;
}

// ---- the text one leaf owns ----
struct Place {  // leaf j among its neighbours inside the query
  bool first, last;
  u32 cp;      // segments shared with the predecessor (first: 0)
  u32 depth;   // its own (<= kRenderDepth)
  u32 cs;      // segments shared with the successor (last: unused)
  u32 dnext;   // the successor's depth (last: unused)
  u32 state;   // mask_state of the composition from the query's end down to this leaf
};
// calls, in text order, out.inl(Punct), out.ptr(offset in the leaf, length) for
// the key and value bytes, and out.close(bracket, nb).  The leaf is well formed
// (leaf_shape said so) and `len` long.
template <class Ld, class Out>
JY_UJR_HD void leaf_text(Ld ld, u64 len, const Place& p, Out& out) {
  const u32 d = p.depth;
  const u32 kfirst = p.first ? 1u : p.cp + 1u;  // the first segment (1-based) whose key this leaf writes
  u64 at = 0;
  bool after_key = false;
  for (u32 k = 1; k <= d; k++) {
    const u32 w = (u32)ld(at, 4);
    at += 4;
    if (k >= kfirst) {
      // k == kfirst of a later leaf: a further child of the node at level cp, open already;
      // else the node at level k - 1 opens here through this child
      const bool comma = !p.first && k == kfirst;
      out.inl(key_glue(after_key, comma, !comma && ((p.state >> (k - 1)) & 1u)));
      out.ptr(at, (u64)w);
      after_key = true;
    }
    at += w;
  }
  at += 4;  // the terminator
  const bool opens = p.first || d > p.cp;  // its own node opens with this value
  const bool second = !p.last && p.cs == d && p.dnext == d;
  out.inl(value_glue(after_key, !opens, opens && second));
  out.ptr(at, len - at);
  // its node ends here if the successor shares fewer than d segments (a value's
  // successor never lies deeper under the same node: children come first)
  const bool ends = p.last || p.cs < d;
  const bool bracket = ends && !p.first && p.cp == d;
  const u32 lo = p.last ? 0u : p.cs + 1u;  // levels lo .. d - 1 end with this leaf
  u32 nb = d > lo ? d - lo : 0u;
  if (!p.last && d > p.cs && p.dnext == p.cs) nb++;  // the successor is a value of the node at level cs
  out.close(bracket, nb);
}

}  // namespace jyuj
