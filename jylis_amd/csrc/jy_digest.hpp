// jy_digest.hpp -- the canonical state digest, for the device and the host.
//
// The digest of a set of keys is the WRAPPING 64-bit SUM of per-key digests,
// so it depends on neither key order nor slot order, and the digest of a node
// is the sum of its shards'.  A key is hashed by its string and a replica by
// its ID (never by slot or column).  Inside a key a TLOG is a list (an
// entry's rank in newest-first order is part of its hash); UJSON elements,
// version-vector entries and cloud dots, and a counter's cells, are sets
// (summed).  Counter cells and vv entries equal to 0 contribute nothing.
//
// This is the definition the test oracle's "canonical state digests" use,
// restated here bit for bit (tests/test_state_digest_*.py tie the two).
//
// BUCKETS.  Peers compare digests per key-hash bucket; both sides must use
// this formula.  With kh = dbytes(key) and B buckets, B a power of two,
// 1 <= B <= 2^20:
//     bucket(kh, B) = 0                                  if B == 1
//                   = dmix(kh ^ 0x7A00) >> (64 - log2 B)  otherwise
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define JY_DG __host__ __device__ __forceinline__
#else
#define JY_DG inline
#endif

namespace jydigest {

typedef uint64_t u64;

constexpr u64 kFnvBasis = 0xCBF29CE484222325ull, kFnvPrime = 0x100000001B3ull;
constexpr u64 kTagLog = 0x7100, kTagEnt = 0x7200, kTagDoc = 0x7300, kTagEl = 0x7400, kTagVV = 0x7500,
              kTagCl = 0x7600, kTagReg = 0x7700, kTagCnt = 0x7800, kTagCell = 0x7900, kTagBucket = 0x7A00;
constexpr uint32_t kMaxBucketsLog2 = 20;

JY_DG u64 dmix(u64 x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
JY_DG u64 dcomb(u64 a, u64 b) { return dmix(a ^ dmix(b)); }
// the last step of dbytes: h = FNV-1a 64 over the n bytes (unsigned)
JY_DG u64 dbytes_end(u64 h, u64 n) { return dcomb(h, n); }
JY_DG u64 dbytes(const uint8_t* p, u64 n) {
  u64 h = kFnvBasis;
  for (u64 i = 0; i < n; i++) {
    h ^= p[i];
    h *= kFnvPrime;
  }
  return dbytes_end(h, n);
}
JY_DG u64 d_reg(u64 kh, u64 ts, u64 vh) { return dcomb(kh, dcomb(kTagReg, dcomb(ts, vh))); }
JY_DG u64 d_log(u64 kh, u64 cutoff) { return dcomb(kh, dcomb(kTagLog, cutoff)); }
JY_DG u64 d_ent(u64 kh, u64 rank, u64 ts, u64 vh) { return dcomb(kh, dcomb(kTagEnt ^ (rank << 16), dcomb(ts, vh))); }
JY_DG u64 d_doc(u64 kh) { return dcomb(kh, kTagDoc); }
JY_DG u64 d_el(u64 kh, u64 id, u64 seq, u64 elem) { return dcomb(kh, dcomb(kTagEl, dcomb(id, dcomb(seq, elem)))); }
JY_DG u64 d_vv(u64 kh, u64 id, u64 n) { return dcomb(kh, dcomb(kTagVV, dcomb(id, n))); }
JY_DG u64 d_cl(u64 kh, u64 id, u64 seq) { return dcomb(kh, dcomb(kTagCl, dcomb(id, seq))); }
JY_DG u64 d_cnt(u64 kh) { return dcomb(kh, kTagCnt); }
JY_DG u64 d_cell(u64 kh, u64 sign, u64 id, u64 v) { return dcomb(kh, dcomb(kTagCell ^ (sign << 16), dcomb(id, v))); }

// lg = log2 B
JY_DG uint32_t bucket(u64 kh, uint32_t lg) { return lg == 0 ? 0u : (uint32_t)(dmix(kh ^ kTagBucket) >> (64 - lg)); }

}  // namespace jydigest
