// k_get.hip -- keyed batch reads: GET by key string for every non-UJSON type
// (jy_treg_get_keys, jy_tlog_get_keys, jy_counter_get_keys).
//
// Boundary: RepoTREG.get (repo_treg.pony:54-63), RepoTLOG.get / size / cutoff
// (repo_tlog.pony:69-96), RepoGCOUNT / RepoPNCOUNT.get (repo_gcount.pony:53-55,
// repo_pncount.pony:55-57).  A query is n key strings as the RESP layer has
// them; the answer comes back in reply form -- found flags, timestamps, value
// bytes packed back to back -- gathered on the device in one call.  The slot
// forms (jy_treg_read, jy_tlog_read_sizes + jy_tlog_read + one jy_arena_read
// per long value) stay for the snapshot and flush readers.
//
//   lookup            jy_keys_lookup_mem: the device slot of every query, or
//                     JY_NO_SLOT
//   k_get_found       found[i], and the slot a reader may index state with
//   TLOG  k_get_tlog_size     a lane per QUERY: slot -> TMeta -> size, cutoff,
//                             take = min(len, count); jy_scan_u64 over take
//                             gives ent_offs (total read back: first wait)
//         k_get_tlog_entries  a lane per OUTPUT ENTRY (below)
//   TREG  treg_records (jy_wire.hpp: the fold, then the gather) + k_get_mask
//   counters  jy_counter_sum (k_sum) + k_get_mask
//   values    value_offsets + emit_values (jy_wire.hpp, k_wire_gather<ValSrc>,
//             balanced by output bytes) over the gathered handles, unchanged
//
// JY_NO_SLOT: MASKED, not compacted.  No kernel here or below indexes state
// with JY_NO_SLOT: k_get_tlog_size reads a TMeta only for a found query, and a
// missing query takes no entries, so k_get_tlog_entries never sees its slot.
// The existing readers (treg_records, k_sum) take a slot per item, so they are
// given k_get_found's `fix` array, in which a missing query names slot 0 --
// which exists whenever the type has a key at all (a type without keys answers
// on the host) -- and k_get_mask then zeroes what was read for it.  Compacting
// the found queries instead would cost a scan, a scatter back into query order
// and a second offsets array for the values; a masked lane costs one wasted
// register read.
//
// The entry gather is one lane per output entry, not one per key (k_tlog_gather,
// k_tlog.hip): a query naming one log of 10^5 entries beside 255 short ones
// would run 10^5 dependent iterations on one lane while its wave idles.  Lane t
// finds its query q as the last one with ent_offs[q] <= t (two wave_last_le
// searches per tile and a short bisect, as k_uj_path_match) and reads
// pool[base + len - 1 - (t - ent_offs[q])]: consecutive lanes of a log read
// consecutive 32-byte records, descending, and their stores to ts and to the
// (pre, lr) temporaries are coalesced.  Nothing loops over a log's length, and
// entries past `take` are never read: GET key 10 on a long log moves 10 records.
//
// Roofline: latency-bound at reply sizes (a few launches and two total
// read-backs); per returned entry one 32-byte record read, 24 bytes of
// temporaries written, and the value's bytes once.  Times against the reads it
// replaces: DESIGN.md, "Keyed reads".
//
// The kernels and the query helpers are in jy_get.hpp: the reply form
// (k_resp.hip) runs the same ones.

#include <algorithm>
#include <cstring>
#include <vector>

#include "jy_get.hpp"

namespace {

// n zero bytes / words where `mem` says
int32_t zeros(jy_engine* eng, int32_t mem, void* dst, u64 bytes) {
  if (bytes == 0) return JY_OK;
  if (!dst) return eng->fail(JY_EINVAL, "an output array is null");
  if (mem == JY_DEVICE) JY_HIP(eng, hipMemsetAsync(dst, 0, bytes, eng->stream));
  else std::memset(dst, 0, bytes);
  return JY_OK;
}

}  // namespace

extern "C" {

int32_t jy_treg_get_keys(jy_engine* eng, uint64_t n, const uint8_t* key_bytes, const uint64_t* key_offs,
                         int32_t keys_mem, uint64_t cap_val_bytes, uint8_t* found, uint64_t* ts, uint8_t* val_bytes,
                         uint64_t* val_offs, uint64_t* sizes_out, int32_t mem) {
  JY_HIP(eng, hipSetDevice(eng->device));
  sizes_out[0] = sizes_out[1] = 0;
  JY_TRY(mem_check(eng, mem));
  if (n == 0) return empty_batch(eng, mem, {val_offs});
  JY_TRY(keys_check(eng, n, key_bytes, key_offs, keys_mem));
  if (!found || !ts || !val_offs) return eng->fail(JY_EINVAL, "found, ts or val_offs is null");
  if (eng->nkeys[JY_TREG] == 0) {  // no key exists: every query is missing
    JY_TRY(zeros(eng, mem, found, n));
    JY_TRY(zeros(eng, mem, ts, n * 8));
    JY_TRY(zeros(eng, mem, val_offs, (n + 1) * 8));
    return host_sync(eng, mem);
  }
  Tmp tmp(eng);
  const u32* slots;
  JY_TRY(query_slots(eng, tmp, JY_TREG, n, key_bytes, key_offs, keys_mem, &slots));
  uint8_t* df;
  u32* fix;
  u64 *nf, *voff;
  JY_TRY(tmp.get(&df, n));
  JY_TRY(tmp.get(&fix, n));
  JY_TRY(tmp.get(&nf, 1));
  JY_HIP(eng, hipMemsetAsync(nf, 0, 8, eng->stream));
  LAUNCH(k_get_found, n, slots, n, df, fix, reinterpret_cast<unsigned long long*>(nf));
  TregRecs R;
  JY_TRY(treg_records(eng, tmp, false, fix, n, R));  // duplicates folded first
  LAUNCH(k_get_mask, n, df, n, R.ts, R.pre, R.lr);
  JY_TRY(value_offsets(eng, tmp, R.lr, n, &voff));
  u64 tot[2];
  JY_TRY(totals(eng, {voff + n, nf}, tot));
  // every launch before this read has finished: a duplicate-list overflow fails the read, as jy_treg_read
  JY_TRY(jy_treg_overflow_check(eng));
  sizes_out[0] = tot[0];
  sizes_out[1] = tot[1];
  if (cap_val_bytes < tot[0]) return JY_OK;  // sizes only
  if (tot[0] && !val_bytes) return eng->fail(JY_EINVAL, "val_bytes is null");
  JY_TRY(emit(eng, mem, found, df, n));
  JY_TRY(emit(eng, mem, ts, R.ts, n * 8));
  JY_TRY(emit_values(eng, tmp, JY_TREG, R.pre, R.lr, voff, n, tot[0], val_bytes, val_offs, mem));
  return host_sync(eng, mem);
}

int32_t jy_tlog_get_keys(jy_engine* eng, uint64_t n, const uint8_t* key_bytes, const uint64_t* key_offs,
                         int32_t keys_mem, const uint64_t* count, uint64_t cap_ent, uint64_t cap_val_bytes,
                         uint8_t* found, uint64_t* size, uint64_t* cutoff, uint64_t* ent_offs, uint64_t* ts,
                         uint8_t* val_bytes, uint64_t* val_offs, uint64_t* sizes_out, int32_t mem) {
  JY_HIP(eng, hipSetDevice(eng->device));
  sizes_out[0] = sizes_out[1] = sizes_out[2] = 0;
  JY_TRY(mem_check(eng, mem));
  if (n == 0) return empty_batch(eng, mem, {ent_offs, val_offs});
  JY_TRY(keys_check(eng, n, key_bytes, key_offs, keys_mem));
  if (!found || !size || !cutoff || !ent_offs || !val_offs)
    return eng->fail(JY_EINVAL, "found, size, cutoff, ent_offs or val_offs is null");
  if (eng->nkeys[JY_TLOG] == 0) {  // no key exists: every query is missing
    JY_TRY(zeros(eng, mem, found, n));
    JY_TRY(zeros(eng, mem, size, n * 8));
    JY_TRY(zeros(eng, mem, cutoff, n * 8));
    JY_TRY(zeros(eng, mem, ent_offs, (n + 1) * 8));
    JY_TRY(zeros(eng, mem, val_offs, 8));
    return host_sync(eng, mem);
  }
  JY_TRY(jy_tlog_settle(eng));  // as every TLOG state read
  const TlogState& t = eng->tlog;
  Tmp tmp(eng);
  const u32* slots;
  JY_TRY(query_slots(eng, tmp, JY_TLOG, n, key_bytes, key_offs, keys_mem, &slots));
  const void* dcount = nullptr;
  if (count) {
    JY_TRY(jy_stage_begin(eng));
    JY_TRY(jy_stage(eng, 1, count, n * 8, JY_HOST, &dcount));
    JY_TRY(jy_stage_end(eng));
  }
  // ---- sizing: a lane per query ----
  uint8_t* df;
  u64 *dsize, *dcut, *take, *eoff, *nf;
  JY_TRY(tmp.get(&df, n));
  JY_TRY(tmp.get(&dsize, n));
  JY_TRY(tmp.get(&dcut, n));
  JY_TRY(tmp.get(&take, n + 1));
  JY_TRY(tmp.get(&eoff, n + 1));
  JY_TRY(tmp.get(&nf, 1));
  JY_HIP(eng, hipMemsetAsync(nf, 0, 8, eng->stream));
  LAUNCH(k_get_tlog_size, n + 1, t.meta, slots, static_cast<const u64*>(dcount), n, df, dsize, dcut, take,
         reinterpret_cast<unsigned long long*>(nf));
  JY_TRY(jy_scan_u64(eng, take, eoff, n));
  u64 tot[2];
  JY_TRY(totals(eng, {eoff + n, nf}, tot));  // the first wait
  const u64 m = tot[0];
  // ---- entries: a lane per output entry (the value bytes are a size of the
  // answer: the handles are read before the capacity check) ----
  u64 *dts, *dpre, *dlr, *voff, vbytes = 0;
  JY_TRY(tmp.get(&dts, m));
  JY_TRY(tmp.get(&dpre, m));
  JY_TRY(tmp.get(&dlr, m));
  if (m) LAUNCH(k_get_tlog_entries, m, t.meta, t.pool, slots, eoff, n, m, dts, dpre, dlr);
  JY_TRY(value_offsets(eng, tmp, dlr, m, &voff));
  if (m) JY_TRY(totals(eng, {voff + m}, &vbytes));  // the second and last wait
  sizes_out[0] = m;
  sizes_out[1] = vbytes;
  sizes_out[2] = tot[1];
  if (cap_ent < m || cap_val_bytes < vbytes) return JY_OK;  // sizes only
  if (m && !ts) return eng->fail(JY_EINVAL, "ts is null");
  if (vbytes && !val_bytes) return eng->fail(JY_EINVAL, "val_bytes is null");
  JY_TRY(emit(eng, mem, found, df, n));
  JY_TRY(emit(eng, mem, size, dsize, n * 8));
  JY_TRY(emit(eng, mem, cutoff, dcut, n * 8));
  JY_TRY(emit(eng, mem, ent_offs, eoff, (n + 1) * 8));
  JY_TRY(emit(eng, mem, ts, dts, m * 8));
  JY_TRY(emit_values(eng, tmp, JY_TLOG, dpre, dlr, voff, m, vbytes, val_bytes, val_offs, mem));
  return host_sync(eng, mem);
}

int32_t jy_counter_get_keys(jy_engine* eng, int32_t type, uint64_t n, const uint8_t* key_bytes,
                            const uint64_t* key_offs, int32_t keys_mem, uint8_t* found, uint64_t* out, int32_t mem) {
  JY_HIP(eng, hipSetDevice(eng->device));
  if (type != JY_GCOUNT && type != JY_PNCOUNT) return eng->fail(JY_ETYPE, "not a counter type");
  JY_TRY(mem_check(eng, mem));
  if (n == 0) return JY_OK;
  JY_TRY(keys_check(eng, n, key_bytes, key_offs, keys_mem));
  if (!found || !out) return eng->fail(JY_EINVAL, "found or out is null");
  const int which = type == JY_GCOUNT ? 0 : 1;
  if (eng->nkeys[type] == 0) {  // no key exists (and maybe no slab yet): every query is missing
    JY_TRY(zeros(eng, mem, found, n));
    JY_TRY(zeros(eng, mem, out, n * 8));
    return host_sync(eng, mem);
  }
  Tmp tmp(eng);
  const u32* slots;
  JY_TRY(query_slots(eng, tmp, type, n, key_bytes, key_offs, keys_mem, &slots));
  uint8_t* df;
  u32* fix;
  u64 *nf, *dout;
  JY_TRY(tmp.get(&df, n));
  JY_TRY(tmp.get(&fix, n));
  JY_TRY(tmp.get(&nf, 1));
  JY_TRY(tmp.get(&dout, n));
  JY_HIP(eng, hipMemsetAsync(nf, 0, 8, eng->stream));
  LAUNCH(k_get_found, n, slots, n, df, fix, reinterpret_cast<unsigned long long*>(nf));
  JY_TRY(jy_counter_sum(eng, which, n, fix, dout));  // k_sum: the slab covers every interned slot
  LAUNCH(k_get_mask, n, df, n, dout, static_cast<u64*>(nullptr), static_cast<u64*>(nullptr));
  JY_TRY(emit(eng, mem, found, df, n));
  JY_TRY(emit(eng, mem, out, dout, n * 8));
  return host_sync(eng, mem);
}

}  // extern "C"
