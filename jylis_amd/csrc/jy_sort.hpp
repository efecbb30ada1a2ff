// jy_sort.hpp -- the engine's device sort (gfx950): a stable least-significant-
// digit radix sort of u64 keys over a chosen bit range, 8 bits a pass, in the
// spirit of jy_dscan.hpp (no library behind it).
//
// A pass is three steps:
//   k_sort_hist     each workgroup counts the digits of its kBlockKeys
//                   consecutive keys (LDS atomics: the counts do not depend on
//                   their order) into hist[digit][workgroup]
//   jydscan::scan   exclusive sum over hist in that order: where each
//                   workgroup's keys of each digit start in the output
//   k_sort_scatter  each workgroup walks its keys again, 256 at a time in input
//                   order; a key's rank among the equal digits of its wave
//                   comes from ballots (no atomics), the waves' counts are
//                   summed in wave order, and the running per-digit base moves
//                   on after every 256 keys
// Keys with equal digits therefore leave a pass in the order they entered it:
// the sort is exact and deterministic, and bits outside [lo, hi) keep their
// input order -- callers put an index in the low bits and sort only the
// significant high bits (k_put.hip: slot << 32 | command index).  A last pass
// with fewer than 8 bits left below hi takes a narrower digit (the pass's
// mask), so bits at and above hi never order anything either.
#pragma once

#include "jy_dscan.hpp"
#include "jy_internal.hpp"

namespace jysort {

constexpr int kThreads = 256;
constexpr int kSub = 4;  // 256-key steps per workgroup
constexpr u64 kBlockKeys = (u64)kThreads * kSub;
constexpr u32 kDigits = 256;

inline u64 blocks_of(u64 n) { return n == 0 ? 1 : (n + kBlockKeys - 1) / kBlockKeys; }
// u64 words of histogram a sort of n keys needs
inline u64 hist_words(u64 n) { return blocks_of(n) * kDigits + 1; }

static __global__ __launch_bounds__(kThreads) void k_sort_hist(const u64* __restrict__ in, u64 n, u32 shift, u32 mask,
                                                        u64* __restrict__ hist, u32 nblk) {
  __shared__ u32 h[kDigits];
  h[threadIdx.x] = 0;
  __syncthreads();
  const u64 i0 = (u64)blockIdx.x * kBlockKeys;
#pragma unroll
  for (int q = 0; q < kSub; q++) {
    const u64 i = i0 + (u64)q * kThreads + threadIdx.x;
    if (i < n) atomicAdd(&h[(u32)(in[i] >> shift) & mask], 1u);
  }
  __syncthreads();
  hist[(u64)threadIdx.x * nblk + blockIdx.x] = h[threadIdx.x];
}

static __global__ __launch_bounds__(kThreads) void k_sort_scatter(const u64* __restrict__ in, u64* __restrict__ out, u64 n,
                                                           u32 shift, u32 mask, const u64* __restrict__ hist,
                                                           u32 nblk) {
  __shared__ u64 base[kDigits];
  __shared__ u32 wcnt[kThreads / 64][kDigits];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  base[threadIdx.x] = hist[(u64)threadIdx.x * nblk + blockIdx.x];
  const u64 i0 = (u64)blockIdx.x * kBlockKeys;
  for (int q = 0; q < kSub; q++) {
#pragma unroll
    for (int v = 0; v < kThreads / 64; v++) wcnt[v][threadIdx.x] = 0;
    __syncthreads();
    const u64 i = i0 + (u64)q * kThreads + threadIdx.x;
    const bool valid = i < n;
    const u64 key = valid ? in[i] : 0;
    const u32 d = (u32)(key >> shift) & mask;
    // the lanes of this wave holding the same digit
    u64 same = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; b++) {
      const bool bit = (d >> b) & 1;
      const u64 m = __ballot(valid && bit);
      same &= bit ? m : ~m;
    }
    const u32 rank = (u32)__popcll(same & ((1ull << lane) - 1));
    if (valid && rank == 0) wcnt[w][d] = (u32)__popcll(same);
    __syncthreads();
    if (valid) {
      u64 pos = base[d] + rank;
      for (int v = 0; v < w; v++) pos += wcnt[v][d];
      out[pos] = key;
    }
    __syncthreads();
    u32 add = 0;
#pragma unroll
    for (int v = 0; v < kThreads / 64; v++) add += wcnt[v][threadIdx.x];
    base[threadIdx.x] += add;
    __syncthreads();
  }
}

// sort the n keys of `a` by their bits [lo, hi), stably; `b` is a second
// buffer of n keys and `hist` one of hist_words(n) words.  *out = whichever of
// a / b holds the result (a when no pass was needed).  Only enqueues.
inline int32_t sort_bits(jy_engine* eng, u64* a, u64* b, u64* hist, u64 n, u32 lo, u32 hi, u64** out) {
  *out = a;
  if (n < 2) return JY_OK;
  const u32 nblk = (u32)blocks_of(n);
  for (u32 shift = lo; shift < hi; shift += 8) {
    // the pass's digit: 8 bits, fewer in a last pass that would reach past hi
    const u32 mask = (1u << (hi - shift < 8 ? hi - shift : 8)) - 1;
    hipLaunchKernelGGL(k_sort_hist, dim3(nblk), dim3(kThreads), 0, eng->stream, (const u64*)a, n, shift, mask, hist,
                       nblk);
    JY_HIP(eng, hipGetLastError());
    JY_TRY((jydscan::scan<jydscan::OpSum, false>(eng, (u64)nblk * kDigits, jydscan::LdArr<u64>{hist},
                                                  jydscan::StArr<u64>{hist})));
    hipLaunchKernelGGL(k_sort_scatter, dim3(nblk), dim3(kThreads), 0, eng->stream, (const u64*)a, b, n, shift, mask,
                       (const u64*)hist, nblk);
    JY_HIP(eng, hipGetLastError());
    u64* t = a;
    a = b;
    b = t;
    *out = a;
  }
  return JY_OK;
}

// bits needed to tell values 0 .. count - 1 apart
inline u32 bits_for(u64 count) {
  u32 b = 0;
  while (b < 64 && (count > (1ull << b))) b++;
  return b;
}

}  // namespace jysort
