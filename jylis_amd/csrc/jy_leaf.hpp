// jy_leaf.hpp -- what the UJSON leaf store's host and device sides share
// (k_leaf.hip, tools/leaf_host_check.cpp): the handle hash, the length guard
// and the probe step.  Compiles as plain C++ and as HIP.
//
// A UJSON element travels as an opaque u64 HANDLE; the leaf behind it is a
// (path, value) pair in its canonical encoding:
//     each path segment as a 4-byte little-endian length plus its bytes,
//     then FF FF FF FF, then the value text
// and   handle = FNV-1a 64 over that encoding, a result of 0 replaced by 1
// (jylis_amd/ujson_doc.py: _fnv1a64(_encode(path, value)) or 1; 0 is "no
// element").  Every replica derives the same handle for the same leaf, so the
// state digests, which hash the handles, do not depend on who stored a leaf.
//
// The store is APPEND-ONLY between collections: a put never removes a leaf.
// jy_ujson_leaves_collect (k_leaf.hip) drops the leaves no document refers to
// any more: a mark pass over the live elements of the state and the pending
// deltas, then a rebuild of table and arena.  Handles are hashes of the leaves
// and do not change when the bytes move.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define JY_LEAF_HD __host__ __device__ inline
#else
#define JY_LEAF_HD inline
#endif

constexpr uint64_t kLeafLenBits = 24;  // an lr is offset << 24 | length (JY_LR_LEN_BITS)
constexpr uint64_t kLeafMaxLen = (1ull << kLeafLenBits) - 1;
constexpr uint64_t kLeafMinLen = 4;  // the terminator alone: empty path, empty value

// the length of item [a, b) of an offsets array, computed ONCE before any loop
// over its bytes; false (a malformed item, skipped): b < a, shorter than the
// terminator, or longer than an lr can name
JY_LEAF_HD bool jy_leaf_len(uint64_t a, uint64_t b, uint64_t* len) {
  *len = 0;
  if (b < a) return false;
  const uint64_t n = b - a;
  if (n < kLeafMinLen || n > kLeafMaxLen) return false;
  *len = n;
  return true;
}

constexpr uint64_t kLeafFnvBasis = 0xCBF29CE484222325ull;
constexpr uint64_t kLeafFnvPrime = 0x100000001B3ull;

// FNV-1a over the low m <= 8 bytes of the little-endian word w
JY_LEAF_HD uint64_t jy_leaf_fold(uint64_t h, uint64_t w, uint64_t m) {
  for (uint64_t b = 0; b < m; b++) {
    h ^= (w >> (8 * b)) & 0xFFu;
    h *= kLeafFnvPrime;
  }
  return h;
}

// the handle of a leaf of `len` bytes; ld(i, m) = its bytes i .. i + m - 1
// (m <= 8) as a little-endian word, zero filled
template <class Ld>
JY_LEAF_HD uint64_t jy_leaf_hash_ld(Ld ld, uint64_t len) {
  uint64_t h = kLeafFnvBasis;
  for (uint64_t i = 0; i < len; i += 8) {
    const uint64_t m = len - i < 8 ? len - i : 8;
    h = jy_leaf_fold(h, ld(i, m), m);
  }
  return h ? h : 1;
}

struct JyLeafBytes {  // a byte at a time: any alignment, any memory
  const uint8_t* p;
  JY_LEAF_HD uint64_t operator()(uint64_t i, uint64_t m) const {
    uint64_t w = 0;
    for (uint64_t b = 0; b < m; b++) w |= (uint64_t)p[i + b] << (8 * b);
    return w;
  }
};
JY_LEAF_HD uint64_t jy_leaf_hash(const uint8_t* p, uint64_t len) { return jy_leaf_hash_ld(JyLeafBytes{p}, len); }

// The table: open addressing, linear probing, a power of two of entries kept
// at least twice the leaves.  FNV-1a's high bits are weak for short inputs, so
// the position is the top bits of the splitmix64 finaliser of the handle.
JY_LEAF_HD uint64_t jy_leaf_start(uint64_t h, uint32_t shift) {
  h ^= h >> 30;
  h *= 0xBF58476D1CE4E5B9ull;
  h ^= h >> 27;
  h *= 0x94D049BB133111EBull;
  h ^= h >> 31;
  return h >> shift;
}
JY_LEAF_HD uint64_t jy_leaf_next(uint64_t p, uint64_t mask) { return (p + 1) & mask; }
