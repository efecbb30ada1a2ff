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
// JY_NO_SLOT is MASKED, not compacted: no kernel here or below indexes state
// with it.  The statement and its reasons stand beside the read cores, in
// jy_get.hpp.
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
// The kernels and the read cores (lookup, found flags, masking, TLOG sizing and
// entries) are in jy_get.hpp: the reply form (k_resp.hip) sits on the same
// ones.  A call here is its argument checks, the core, and the column tail.

#include <algorithm>
#include <cstring>
#include <vector>

#include "jy_get.hpp"

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
  Tmp tmp(eng);
  Found F;
  TregRecs R;
  JY_TRY(treg_read(eng, tmp, n, key_bytes, key_offs, keys_mem, F, R));
  u64* voff;
  JY_TRY(value_offsets(eng, tmp, R.lr, n, &voff));
  u64 tot[2];
  JY_TRY(totals(eng, {voff + n, F.nfound}, tot));
  JY_TRY(jy_treg_overflow_check(eng));  // after the wait: see treg_read
  sizes_out[0] = tot[0];
  sizes_out[1] = tot[1];
  if (cap_val_bytes < tot[0]) return JY_OK;  // sizes only
  if (tot[0] && !val_bytes) return eng->fail(JY_EINVAL, "val_bytes is null");
  JY_TRY(emit(eng, mem, found, F.found, n));
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
  Tmp tmp(eng);
  const auto count_col = [&](const u64** dcount) -> int32_t {  // the host column, staged
    if (!count) return JY_OK;
    const void* d;
    JY_TRY(jy_stage_begin(eng));
    JY_TRY(jy_stage(eng, 1, count, n * 8, JY_HOST, &d));
    *dcount = static_cast<const u64*>(d);
    return jy_stage_end(eng);
  };
  TlogRead G;
  JY_TRY(tlog_read(eng, tmp, n, key_bytes, key_offs, keys_mem, count_col, G));
  // the value bytes are a size of the answer: the handles were read before the capacity check
  const u64 m = G.m;
  u64 *voff, vbytes = 0;
  JY_TRY(value_offsets(eng, tmp, G.lr, m, &voff));
  if (m) JY_TRY(totals(eng, {voff + m}, &vbytes));  // the second and last wait
  sizes_out[0] = m;
  sizes_out[1] = vbytes;
  sizes_out[2] = G.nfound;
  if (cap_ent < m || cap_val_bytes < vbytes) return JY_OK;  // sizes only
  if (m && !ts) return eng->fail(JY_EINVAL, "ts is null");
  if (vbytes && !val_bytes) return eng->fail(JY_EINVAL, "val_bytes is null");
  JY_TRY(emit(eng, mem, found, G.found, n));
  JY_TRY(emit(eng, mem, size, G.size, n * 8));
  JY_TRY(emit(eng, mem, cutoff, G.cutoff, n * 8));
  JY_TRY(emit(eng, mem, ent_offs, G.eoff, (n + 1) * 8));
  JY_TRY(emit(eng, mem, ts, G.ts, m * 8));
  JY_TRY(emit_values(eng, tmp, JY_TLOG, G.pre, G.lr, voff, m, vbytes, val_bytes, val_offs, mem));
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
  Tmp tmp(eng);
  Found F;
  u64* dout;
  JY_TRY(counter_read(eng, tmp, type, n, key_bytes, key_offs, keys_mem, F, &dout));
  JY_TRY(emit(eng, mem, found, F.found, n));
  JY_TRY(emit(eng, mem, out, dout, n * 8));
  return host_sync(eng, mem);
}

}  // extern "C"
