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
// through the host cache first, as jy_keys_lookup does.  A type without a key
// has no directory to search: every query is missing.
inline int32_t query_slots(jy_engine* eng, Tmp& tmp, int32_t type, u64 n, const uint8_t* kb, const u64* ko,
                           int32_t keys_mem, const u32** slots) {
  if (keys_mem == JY_DEVICE || eng->nkeys[type] == 0) {
    u32* ds;
    JY_TRY(tmp.get(&ds, n));
    if (eng->nkeys[type] == 0) JY_HIP(eng, hipMemsetAsync(ds, 0xFF, n * 4, eng->stream));  // JY_NO_SLOT throughout
    else JY_TRY(jy_keys_lookup_mem(eng, type, n, kb, ko, ds, JY_DEVICE));
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

// ---- the read cores: one per type, under the column form and the reply form ----
// A core takes n > 0 queries whose key columns the caller has checked
// (keys_check) and leaves the answer in temporaries of `tmp`; what a form makes
// of it -- columns in the caller's memory, or reply bytes -- is the form's tail.
//
// JY_NO_SLOT: MASKED, not compacted.  No kernel here or below indexes state
// with JY_NO_SLOT: k_get_tlog_size reads a TMeta only for a found query, and a
// missing query takes no entries, so k_get_tlog_entries never sees its slot.
// The existing readers (treg_records, k_sum) take a slot per item, so they are
// given k_get_found's `fix` array, in which a missing query names slot 0, and
// k_get_mask then zeroes what was read for it.  Slot 0 exists whenever the type
// has a key at all; for a type without one (and maybe without a slab) no reader
// runs and the records are zero-filled, which is what k_get_mask would leave:
// every query is missing.  Compacting the found queries instead would cost a
// scan, a scatter back into query order and a second offsets array for the
// values; a masked lane costs one wasted register read.

// n zeroed words
inline int32_t zero_words(jy_engine* eng, Tmp& tmp, u64 n, u64** out) {
  JY_TRY(tmp.get(out, n));
  JY_HIP(eng, hipMemsetAsync(*out, 0, n * 8, eng->stream));
  return JY_OK;
}

// what TREG and the counters start with: the lookup, then k_get_found
struct Found {
  uint8_t* found = nullptr;  // per query
  u32* fix = nullptr;        // per query: a slot that exists
  u64* nfound = nullptr;     // one device word: the found queries
};
inline int32_t found_slots(jy_engine* eng, Tmp& tmp, int32_t type, u64 n, const uint8_t* kb, const u64* ko,
                           int32_t keys_mem, Found& F) {
  const u32* slots;
  JY_TRY(query_slots(eng, tmp, type, n, kb, ko, keys_mem, &slots));
  JY_TRY(tmp.get(&F.found, n));
  JY_TRY(tmp.get(&F.fix, n));
  JY_TRY(zero_words(eng, tmp, 1, &F.nfound));
  LAUNCH(k_get_found, n, slots, n, F.found, F.fix, reinterpret_cast<unsigned long long*>(F.nfound));
  return JY_OK;
}

// TREG: R = the registers, zero for a missing key.  The caller reads F.nfound
// back with its own totals and calls jy_treg_overflow_check AFTER that wait,
// when every launch before it has finished: a duplicate-list overflow fails the
// read, as jy_treg_read.
inline int32_t treg_read(jy_engine* eng, Tmp& tmp, u64 n, const uint8_t* kb, const u64* ko, int32_t keys_mem, Found& F,
                         TregRecs& R) {
  JY_TRY(found_slots(eng, tmp, JY_TREG, n, kb, ko, keys_mem, F));
  if (eng->nkeys[JY_TREG] == 0) {
    JY_TRY(zero_words(eng, tmp, n, &R.ts));
    JY_TRY(zero_words(eng, tmp, n, &R.pre));
    return zero_words(eng, tmp, n, &R.lr);
  }
  JY_TRY(treg_records(eng, tmp, false, F.fix, n, R));  // duplicates folded first
  LAUNCH(k_get_mask, n, F.found, n, R.ts, R.pre, R.lr);
  return JY_OK;
}

// counters: val = the sums, zero for a missing key
inline int32_t counter_read(jy_engine* eng, Tmp& tmp, int32_t type, u64 n, const uint8_t* kb, const u64* ko,
                            int32_t keys_mem, Found& F, u64** val) {
  JY_TRY(found_slots(eng, tmp, type, n, kb, ko, keys_mem, F));
  if (eng->nkeys[type] == 0) return zero_words(eng, tmp, n, val);
  JY_TRY(tmp.get(val, n));
  JY_TRY(jy_counter_sum(eng, type == JY_GCOUNT ? 0 : 1, n, F.fix, *val));  // k_sum: the slab covers every interned slot
  LAUNCH(k_get_mask, n, F.found, n, *val, static_cast<u64*>(nullptr), static_cast<u64*>(nullptr));
  return JY_OK;
}

// TLOG: sizing with a lane per query, entries with a lane per output entry.
// `count_col` leaves the device count column (null: no limit) in *dcount.  It
// is the caller's, because the forms differ there, and it runs between the
// lookup and the sizing because both stage through the engine's scratch slots:
// a column staged before the lookup of host keys would be overwritten by it.
struct TlogRead {
  uint8_t* found = nullptr;                          // per query
  u64 *size = nullptr, *cutoff = nullptr;            // per query
  u64* eoff = nullptr;                               // per query; eoff[n] = m
  u64 m = 0, nfound = 0;                             // on the host: the entries, the found queries
  u64 *ts = nullptr, *pre = nullptr, *lr = nullptr;  // per entry, newest first per query
};
template <class CountCol>
inline int32_t tlog_read(jy_engine* eng, Tmp& tmp, u64 n, const uint8_t* kb, const u64* ko, int32_t keys_mem,
                         CountCol&& count_col, TlogRead& G) {
  if (eng->nkeys[JY_TLOG]) JY_TRY(jy_tlog_settle(eng));  // as every TLOG state read
  const TlogState& t = eng->tlog;
  const u32* slots;
  JY_TRY(query_slots(eng, tmp, JY_TLOG, n, kb, ko, keys_mem, &slots));
  const u64* dcount = nullptr;
  JY_TRY(count_col(&dcount));
  u64 *take, *nf;
  JY_TRY(tmp.get(&G.found, n));
  JY_TRY(tmp.get(&G.size, n));
  JY_TRY(tmp.get(&G.cutoff, n));
  JY_TRY(tmp.get(&take, n + 1));
  JY_TRY(tmp.get(&G.eoff, n + 1));
  JY_TRY(zero_words(eng, tmp, 1, &nf));
  LAUNCH(k_get_tlog_size, n + 1, t.meta, slots, dcount, n, G.found, G.size, G.cutoff, take,
         reinterpret_cast<unsigned long long*>(nf));
  JY_TRY(jy_scan_u64(eng, take, G.eoff, n));
  u64 tot[2];
  JY_TRY(totals(eng, {G.eoff + n, nf}, tot));  // the first wait
  G.m = tot[0];
  G.nfound = tot[1];
  JY_TRY(tmp.get(&G.ts, G.m));
  JY_TRY(tmp.get(&G.pre, G.m));
  JY_TRY(tmp.get(&G.lr, G.m));
  if (G.m) LAUNCH(k_get_tlog_entries, G.m, t.meta, t.pool, slots, G.eoff, n, G.m, G.ts, G.pre, G.lr);
  return JY_OK;
}

// where the replies go once their total is known: the caller's arrays if they
// hold it (false: sizes only), or room asked of `dst`
inline int32_t resp_room(JyRespDst* dst, u64 total, u64 cap_bytes, uint8_t** reply_bytes, u64** reply_offs,
                         int32_t* mem, bool* fits) {
  *fits = true;
  if (!dst) {
    *fits = cap_bytes >= total;
    return JY_OK;
  }
  JY_TRY(jy_resp_dst_reserve(dst, total, reply_bytes));
  *reply_offs = dst->reply_offs;
  *mem = JY_DEVICE;
  return JY_OK;
}

}  // namespace
