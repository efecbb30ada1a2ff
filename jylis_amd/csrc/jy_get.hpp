// jy_get.hpp -- what the keyed reads share: the column form (k_get.hip,
// jy_*_get_keys) and the reply form (k_resp.hip, jy_*_get_resp) look keys up,
// mask missing ones and size and gather TLOG entries with the same kernels.
// The design notes are in k_get.hip's header.
#pragma once

#include <vector>

#include "jy_scan.hpp"
#include "jy_wire.hpp"

namespace {

// found[i] = the key is interned; fix[i] = a slot that exists (slot 0 for a
// missing key: masked afterwards); *nfound += the found queries
__global__ __launch_bounds__(kThreads) void k_get_found(const u32* __restrict__ slots, u64 n,
                                                        uint8_t* __restrict__ found, u32* __restrict__ fix,
                                                        unsigned long long* nfound) {
  const u64 i = gid();
  const bool in = i < n;
  bool f = false;
  if (in) {
    const u32 s = slots[i];
    f = s != JY_NO_SLOT;
    found[i] = f ? 1 : 0;
    if (fix) fix[i] = f ? s : 0u;
  }
  jy_wave_count(f, nfound);
}

// a[i] = b[i] = c[i] = 0 where found[i] == 0 (b, c may be null)
__global__ __launch_bounds__(kThreads) void k_get_mask(const uint8_t* __restrict__ found, u64 n, u64* __restrict__ a,
                                                       u64* __restrict__ b, u64* __restrict__ c) {
  const u64 i = gid();
  if (i >= n || found[i]) return;
  a[i] = 0;
  if (b) b[i] = 0;
  if (c) c[i] = 0;
}

// TLOG sizing, a lane per query; lane n closes `take` for the scan
__global__ __launch_bounds__(kThreads) void k_get_tlog_size(const TMeta* __restrict__ meta,
                                                            const u32* __restrict__ slots,
                                                            const u64* __restrict__ count, u64 n,
                                                            uint8_t* __restrict__ found, u64* __restrict__ size,
                                                            u64* __restrict__ cutoff, u64* __restrict__ take,
                                                            unsigned long long* nfound) {
  const u64 i = gid();
  bool f = false;
  if (i < n) {
    const u32 s = slots[i];
    f = s != JY_NO_SLOT;
    u64 len = 0, cut = 0;
    if (f) {
      const TMeta m = meta[s];
      len = m.len;
      cut = m.cut;
    }
    const u64 c = count ? count[i] : ~0ull;
    found[i] = f ? 1 : 0;
    size[i] = len;
    cutoff[i] = cut;
    take[i] = len < c ? len : c;
  } else if (i == n) {
    take[n] = 0;
  }
  jy_wave_count(f, nfound);
}

// TLOG entries, a lane per output entry t < total = eoff[n]: newest first, on
// equal timestamps the greater value first (the pool is ascending (ts, value))
__global__ __launch_bounds__(kThreads) void k_get_tlog_entries(const TMeta* __restrict__ meta,
                                                               const TRec* __restrict__ pool,
                                                               const u32* __restrict__ slots,
                                                               const u64* __restrict__ eoff, u64 n, u64 total,
                                                               u64* __restrict__ ots, u64* __restrict__ opre,
                                                               u64* __restrict__ olr) {
  __shared__ u64 sh[2];
  const u64 t0 = (u64)blockIdx.x * kThreads;
  if (t0 >= total) return;
  const u64 t1 = t0 + kThreads < total ? t0 + kThreads : total;
  if (threadIdx.x < 128) {
    const u64 k = jyscan::wave_last_le(eoff, n, threadIdx.x < 64 ? t0 : t1 - 1);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = k;
  }
  __syncthreads();
  const u64 t = t0 + threadIdx.x;
  if (t >= t1) return;
  u64 lo = sh[0], hi = sh[1];
  while (lo < hi) {
    const u64 mid = (lo + hi + 1) >> 1;
    if (eoff[mid] <= t) lo = mid;
    else hi = mid - 1;
  }
  // eoff[lo] <= t < eoff[lo + 1]: query lo takes an entry, so it was found
  const TMeta m = meta[slots[lo]];
  const u64 j = t - eoff[lo];  // < take <= m.len
  const TRec x = pool[tm_base(m) + m.len - 1 - j];
  ots[t] = x.ts;
  opre[t] = x.pre;
  olr[t] = x.lr;
}

inline int32_t keys_check(jy_engine* eng, u64 n, const uint8_t* kb, const u64* ko, int32_t keys_mem) {
  if (keys_mem != JY_HOST && keys_mem != JY_DEVICE)
    return eng->fail(JY_EINVAL, "keys_mem must be JY_HOST or JY_DEVICE");
  if (!ko) return eng->fail(JY_EINVAL, "key_offs is null");
  if (keys_mem == JY_HOST) {
    for (u64 i = 0; i < n; i++)
      if (ko[i + 1] < ko[i]) return eng->fail(JY_EINVAL, "key_offs is not ascending");
    if (ko[n] > ko[0] && !kb) return eng->fail(JY_EINVAL, "key_bytes is null");
  }
  return JY_OK;
}

// the queries' slots as a device array (JY_NO_SLOT: no such key).  Host keys go
// through the host cache first, as jy_keys_lookup does.
inline int32_t query_slots(jy_engine* eng, Tmp& tmp, int32_t type, u64 n, const uint8_t* kb, const u64* ko,
                           int32_t keys_mem, const u32** slots) {
  if (keys_mem == JY_DEVICE) {
    u32* ds;
    JY_TRY(tmp.get(&ds, n));
    JY_TRY(jy_keys_lookup_mem(eng, type, n, kb, ko, ds, JY_DEVICE));
    *slots = ds;
    return JY_OK;
  }
  std::vector<u32> hs(n);
  JY_TRY(jy_keys_lookup_mem(eng, type, n, kb, ko, hs.data(), JY_HOST));
  const void* ds;
  JY_TRY(jy_stage_begin(eng));
  JY_TRY(jy_stage(eng, 0, hs.data(), n * 4, JY_HOST, &ds));
  JY_TRY(jy_stage_end(eng));
  *slots = static_cast<const u32*>(ds);
  return JY_OK;
}

}  // namespace
