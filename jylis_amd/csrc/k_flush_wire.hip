// k_flush_wire.hip -- flush_deltas() (repo_manager.pony:9, repo_gcount.pony:
// 18-23 and every repo_*.pony): the pending set (PendingSet) and every flush.
// Two output formats:
//   slot form (jy_*_flush): slots and arena handles, what jy_*_converge takes
//   wire form (jy_*_flush_wire): key strings and value bytes, the arrays
//     jy_node_*_converge takes, built on the device from the key directory
//     (KeyDir) and the value arenas
//
// Every flush is: read the pending count (TLOG settles its merges first),
// select the pending slots (ascending), read their deltas from the PENDING
// store with the type's record reader (jy_wire.hpp; nothing is cleared yet),
// and only when every output capacity is large enough copy the records out
// and run the type's one CLEAR.  The wire forms hand the slots to the type's
// wire formatter (jy_wire.hpp) -- the one the state snapshots run over the
// state -- and clear when it reports that everything was written; the slot
// forms emit the reader's records as they are.  A short capacity returns
// JY_ERANGE from the slot-form counter and TREG flushes, JY_OK with the sizes
// from every other one.  Only the counters' cell producer lives here: the
// pending mask and [g][k] values under one column.  Temporaries come from the
// engine's stream-ordered pool (Tmp): no flush uses a scratch slot.

#include "jy_dscan.hpp"
#include "jy_wire.hpp"

namespace {

// counters (jy_cnt_pending_peek's mask and [g][k] totals): cells per key
// from the mask (bit g = sign g written) ...
__global__ __launch_bounds__(kThreads) void k_wire_cnt_ncell(const u32* __restrict__ mask, u32 smask, u64 k,
                                                             u64* __restrict__ ncell) {
  const u64 j = gid();
  if (j > k) return;
  ncell[j] = j < k ? (u64)__popc(mask[j] & smask) : 0;
}
// ... and the cells the mask names, P before N
__global__ __launch_bounds__(kThreads) void k_wire_cnt_cells(const u32* __restrict__ mask,
                                                             const u64* __restrict__ vals, u32 nsigns, u16 col, u64 k,
                                                             const u64* __restrict__ coff, uint8_t* __restrict__ sign,
                                                             u16* __restrict__ ocol, u64* __restrict__ val) {
  const u64 j = gid();
  if (j >= k) return;
  const u32 f = mask[j];
  u64 o = coff[j];
  for (u32 g = 0; g < nsigns; g++)
    if ((f >> g) & 1u) {
      sign[o] = (uint8_t)g;
      ocol[o] = col;
      val[o] = vals[(u64)g * k + j];
      o++;
    }
}

// the k pending slots of a set (a temporary), and for the wire form their
// key lengths / offsets
int32_t pending_slots(jy_engine* eng, Tmp& tmp, int32_t type, const PendingSet& P, u64 k, u32** slots) {
  JY_TRY(tmp.get(slots, k));
  return jy_pending_slots(eng, type, P, k, *slots);
}
int32_t pending_keys(jy_engine* eng, Tmp& tmp, int32_t type, const PendingSet& P, u64 k, Keys& K) {
  JY_TRY(pending_slots(eng, tmp, type, P, k, &K.slots));
  return key_offsets(eng, tmp, type, k, K);
}

constexpr const char* kShort = "flush output capacity is smaller than the pending delta count";

struct PendingPred {
  const u32* flag;
  __device__ bool operator()(u64 s) const { return flag[s] != 0; }
};

}  // namespace

// ---- the pending set ----
int32_t jy_pending_grow(jy_engine* eng, PendingSet& p, u64 kcap, const char* what) {
  if (!p.count) {
    void* c = nullptr;
    JY_TRY(jy_dev_alloc(eng, &c, 16, what));
    JY_HIP(eng, hipMemsetAsync(c, 0, 16, eng->stream));
    p.count = static_cast<u64*>(c);
  }
  if (p.cap >= kcap && p.flag) return JY_OK;
  void* f = p.flag;
  JY_TRY(jy_realloc(eng, &f, p.cap * 4, kcap * 4, true));
  p.flag = static_cast<u32*>(f);
  p.cap = kcap;
  return JY_OK;
}

int32_t jy_pending_count(jy_engine* eng, const PendingSet& p, u64* k) {
  *k = 0;
  if (!p.count) return JY_OK;  // never written
  return totals(eng, {p.count}, k);
}

int32_t jy_pending_slots(jy_engine* eng, int32_t type, const PendingSet& p, u64 k, u32* slots) {
  if (k == 0) return JY_OK;
  return jydscan::select(eng, std::min<u64>(eng->nkeys[type], p.cap), PendingPred{p.flag}, slots,
                         reinterpret_cast<u32*>(p.count + 1));  // (the select's count: k again)
}

int32_t jy_pending_reset(jy_engine* eng, PendingSet& p) {
  JY_HIP(eng, hipMemsetAsync(p.count, 0, 8, eng->stream));
  return JY_OK;
}

extern "C" {

// ---- counters ----
int32_t jy_counter_flush(jy_engine* eng, int32_t type, uint64_t cap, uint32_t* slot_out, uint64_t* vals_out,
                         uint32_t* mask_out, uint64_t* n_out, int32_t mem) {
  JY_HIP(eng, hipSetDevice(eng->device));
  if (type != JY_GCOUNT && type != JY_PNCOUNT) return eng->fail(JY_ETYPE, "not a counter type");
  const int w = type == JY_GCOUNT ? 0 : 1;
  const u64 nsigns = w + 1;
  u64 k = 0;
  JY_TRY(jy_pending_count(eng, eng->cnt[w].pend, &k));
  *n_out = k;
  if (k > cap) return eng->fail(JY_ERANGE, kShort);
  if (k == 0) return JY_OK;
  Tmp tmp(eng);
  const u64 pitch = mem == JY_HOST ? k : cap;  // of the device array the peek writes
  u32 *ds, *dm;
  u64* dv;
  JY_TRY(tmp.out(&ds, slot_out, k, mem));
  JY_TRY(tmp.out(&dm, mask_out, k, mem));
  JY_TRY(tmp.out(&dv, vals_out, nsigns * pitch, mem));
  JY_TRY(jy_pending_slots(eng, type, eng->cnt[w].pend, k, ds));
  JY_TRY(jy_cnt_pending_peek(eng, w, ds, k, pitch, dv, dm));
  JY_TRY(emit(eng, mem, slot_out, ds, k * 4));
  JY_TRY(emit(eng, mem, mask_out, dm, k * 4));
  for (u64 g = 0; g < nsigns; g++) JY_TRY(emit(eng, mem, vals_out + g * cap, dv + g * pitch, k * 8));
  JY_TRY(jy_cnt_pending_clear(eng, w, ds, k));
  if (mem == JY_HOST) JY_HIP(eng, hipStreamSynchronize(eng->stream));
  return JY_OK;
}

int32_t jy_counter_flush_wire(jy_engine* eng, int32_t type, uint32_t col, uint64_t cap_keys, uint64_t cap_key_bytes,
                              uint64_t cap_cells, uint8_t* key_bytes, uint64_t* key_offs, uint64_t* cell_offs,
                              uint8_t* sign, uint16_t* col_out, uint64_t* val, uint64_t* sizes_out, int32_t mem) {
  JY_HIP(eng, hipSetDevice(eng->device));
  if (type != JY_GCOUNT && type != JY_PNCOUNT) return eng->fail(JY_ETYPE, "not a counter type");
  JY_TRY(mem_check(eng, mem));
  const int w = type == JY_GCOUNT ? 0 : 1;
  const u32 nsigns = w + 1;
  CounterState& c = eng->cnt[w];
  sizes_out[0] = sizes_out[1] = sizes_out[2] = 0;
  u64 k = 0;
  JY_TRY(jy_pending_count(eng, c.pend, &k));
  if (k == 0) return empty_batch(eng, mem, {key_offs, cell_offs});
  if (col > 0xFFFF || col >= eng->rep_id.size()) return eng->fail(JY_ERANGE, "column names no registered replica");
  if (c.dcol >= 0 && (u32)c.dcol != col)
    return eng->fail(JY_EINVAL, "pending deltas were written under another replica column");
  Tmp tmp(eng);
  Keys K;
  JY_TRY(pending_keys(eng, tmp, type, c.pend, k, K));
  u32* mask;
  u64 *vals, *ncell, *coff;
  JY_TRY(tmp.get(&mask, k));
  JY_TRY(tmp.get(&vals, nsigns * k));
  JY_TRY(tmp.get(&ncell, k + 1));
  JY_TRY(tmp.get(&coff, k + 1));
  JY_TRY(jy_cnt_pending_peek(eng, w, K.slots, k, k, vals, mask));
  LAUNCH(k_wire_cnt_ncell, k + 1, mask, (1u << nsigns) - 1, k, ncell);
  JY_TRY(jy_scan_u64(eng, ncell, coff, k));
  bool written;
  JY_TRY(counter_format(eng, tmp, type, K, k, coff, {cap_keys, cap_key_bytes, cap_cells},
                        CounterWire{key_bytes, key_offs, cell_offs, sign, col_out, val}, sizes_out, mem, &written,
                        [&](u64, uint8_t* ds, u16* dc, u64* dv) -> int32_t {
                          LAUNCH(k_wire_cnt_cells, k, mask, vals, nsigns, (u16)col, k, coff, ds, dc, dv);
                          return JY_OK;
                        }));
  if (!written) return JY_OK;
  JY_TRY(jy_cnt_pending_clear(eng, w, K.slots, k));
  return host_sync(eng, mem);
}

// ---- TREG ----
int32_t jy_treg_flush(jy_engine* eng, uint64_t cap, uint32_t* slot_out, uint64_t* ts_out, uint64_t* pre_out,
                      uint64_t* lr_out, uint64_t* n_out, int32_t mem) {
  JY_HIP(eng, hipSetDevice(eng->device));
  u64 k = 0;
  JY_TRY(jy_pending_count(eng, eng->treg.pend, &k));
  *n_out = k;
  if (k > cap) return eng->fail(JY_ERANGE, kShort);
  if (k == 0) return JY_OK;
  Tmp tmp(eng);
  u32* ds;
  TregRecs R;
  JY_TRY(tmp.out(&ds, slot_out, k, mem));
  JY_TRY(jy_pending_slots(eng, JY_TREG, eng->treg.pend, k, ds));
  JY_TRY(treg_records(eng, tmp, true, ds, k, R, mem, ts_out, pre_out, lr_out));
  JY_TRY(emit(eng, mem, slot_out, ds, k * 4));
  JY_TRY(emit(eng, mem, ts_out, R.ts, k * 8));
  JY_TRY(emit(eng, mem, pre_out, R.pre, k * 8));
  JY_TRY(emit(eng, mem, lr_out, R.lr, k * 8));
  JY_TRY(jy_treg_pending_clear(eng, ds, k));
  return host_sync(eng, mem);
}

int32_t jy_treg_flush_wire(jy_engine* eng, uint64_t cap_keys, uint64_t cap_key_bytes, uint64_t cap_val_bytes,
                           uint8_t* key_bytes, uint64_t* key_offs, uint64_t* ts, uint8_t* val_bytes,
                           uint64_t* val_offs, uint64_t* sizes_out, int32_t mem) {
  JY_HIP(eng, hipSetDevice(eng->device));
  JY_TRY(mem_check(eng, mem));
  sizes_out[0] = sizes_out[1] = sizes_out[2] = 0;
  u64 k = 0;
  JY_TRY(jy_pending_count(eng, eng->treg.pend, &k));
  if (k == 0) return empty_batch(eng, mem, {key_offs, val_offs});
  Tmp tmp(eng);
  Keys K;
  bool written;
  JY_TRY(pending_keys(eng, tmp, JY_TREG, eng->treg.pend, k, K));
  JY_TRY(treg_format(eng, tmp, K, k, true, {cap_keys, cap_key_bytes, cap_val_bytes},
                     TregWire{key_bytes, key_offs, ts, val_bytes, val_offs}, sizes_out, mem, &written));
  if (!written) return JY_OK;
  JY_TRY(jy_treg_pending_clear(eng, K.slots, k));
  return host_sync(eng, mem);
}

// ---- TLOG ----
int32_t jy_tlog_flush(jy_engine* eng, uint64_t cap_keys, uint64_t cap_ent, uint32_t* slot_out, uint64_t* cutoff_out,
                      uint64_t* offs_out, uint64_t* ts_out, uint64_t* pre_out, uint64_t* lr_out, uint64_t* nkeys_out,
                      uint64_t* nent_out, int32_t mem) {
  JY_HIP(eng, hipSetDevice(eng->device));
  *nkeys_out = *nent_out = 0;
  JY_TRY(jy_tlog_settle(eng));
  u64 k = 0;
  JY_TRY(jy_pending_count(eng, eng->tl_pend, &k));
  *nkeys_out = k;
  if (k == 0) return JY_OK;
  Tmp tmp(eng);
  u32* slots;
  TlogRecs R;
  JY_TRY(pending_slots(eng, tmp, JY_TLOG, eng->tl_pend, k, &slots));
  JY_TRY(tlog_sizing(eng, tmp, eng->tlog_d, slots, k, R));
  JY_TRY(totals(eng, {R.eoff + k}, &R.m));
  const u64 m = *nent_out = R.m;
  if (cap_keys < k || cap_ent < m) return JY_OK;  // sizes only
  JY_TRY(tlog_entries(eng, tmp, eng->tlog_d, slots, k, R, mem, ts_out, pre_out, lr_out));
  JY_TRY(emit(eng, mem, slot_out, slots, k * 4));
  JY_TRY(emit(eng, mem, cutoff_out, R.cuts, k * 8));
  JY_TRY(emit(eng, mem, offs_out, R.eoff, (k + 1) * 8));
  JY_TRY(emit(eng, mem, ts_out, R.ts, m * 8));
  JY_TRY(emit(eng, mem, pre_out, R.pre, m * 8));
  JY_TRY(emit(eng, mem, lr_out, R.lr, m * 8));
  JY_TRY(jy_tlog_pending_clear(eng, slots, k));
  JY_HIP(eng, hipStreamSynchronize(eng->stream));
  return JY_OK;
}

int32_t jy_tlog_flush_wire(jy_engine* eng, uint64_t cap_keys, uint64_t cap_key_bytes, uint64_t cap_ent,
                           uint64_t cap_val_bytes, uint8_t* key_bytes, uint64_t* key_offs, uint64_t* cutoff,
                           uint64_t* ent_offs, uint64_t* ts, uint8_t* val_bytes, uint64_t* val_offs,
                           uint64_t* sizes_out, int32_t mem) {
  JY_HIP(eng, hipSetDevice(eng->device));
  JY_TRY(mem_check(eng, mem));
  for (int q = 0; q < 4; q++) sizes_out[q] = 0;
  JY_TRY(jy_tlog_settle(eng));
  u64 k = 0;
  JY_TRY(jy_pending_count(eng, eng->tl_pend, &k));
  if (k == 0) return empty_batch(eng, mem, {key_offs, ent_offs, val_offs});
  Tmp tmp(eng);
  Keys K;
  bool written;
  JY_TRY(pending_keys(eng, tmp, JY_TLOG, eng->tl_pend, k, K));
  JY_TRY(tlog_format(eng, tmp, K, k, eng->tlog_d, {cap_keys, cap_key_bytes, cap_ent, cap_val_bytes},
                     TlogWire{key_bytes, key_offs, cutoff, ent_offs, ts, val_bytes, val_offs}, sizes_out, mem,
                     &written));
  if (!written) return JY_OK;
  JY_TRY(jy_tlog_pending_clear(eng, K.slots, k));
  return host_sync(eng, mem);
}

// ---- UJSON ----
int32_t jy_ujson_flush(jy_engine* eng, uint64_t cap_docs, uint64_t cap_el, uint64_t cap_cl, uint32_t* slot_out,
                       uint64_t* eoff_out, uint64_t* dots_out, uint64_t* elems_out, uint64_t* vv_out,
                       uint64_t* coff_out, uint64_t* cloud_out, uint64_t* ndocs_out, uint64_t* nel_out,
                       uint64_t* ncl_out, int32_t mem) {
  JY_HIP(eng, hipSetDevice(eng->device));
  *ndocs_out = *nel_out = *ncl_out = 0;
  u64 k = 0;
  JY_TRY(jy_pending_count(eng, eng->uj_pend, &k));
  *ndocs_out = k;
  if (k == 0) return JY_OK;
  const UjsonState& d = eng->ujson_d;
  Tmp tmp(eng);
  u32* slots;
  UjsonRecs D;
  JY_TRY(pending_slots(eng, tmp, JY_UJSON, eng->uj_pend, k, &slots));
  JY_TRY(ujson_sizing(eng, tmp, d, slots, k, D));
  u64 tot[2];
  JY_TRY(totals(eng, {D.eo + k, D.co + k}, tot));
  const u64 me = *nel_out = D.me = tot[0], mc = *ncl_out = D.mc = tot[1];
  if (cap_docs < k || cap_el < me || cap_cl < mc) return JY_OK;  // sizes only
  JY_TRY(ujson_entries(eng, tmp, d, slots, k, D, mem, dots_out, elems_out, vv_out, cloud_out));  // vv: dense [k][R]
  JY_TRY(emit(eng, mem, slot_out, slots, k * 4));
  JY_TRY(emit(eng, mem, eoff_out, D.eo, (k + 1) * 8));
  JY_TRY(emit(eng, mem, coff_out, D.co, (k + 1) * 8));
  JY_TRY(emit(eng, mem, dots_out, D.dots, me * 8));
  JY_TRY(emit(eng, mem, elems_out, D.elems, me * 8));
  JY_TRY(emit(eng, mem, vv_out, D.dense, k * d.R * 8));
  JY_TRY(emit(eng, mem, cloud_out, D.cloud, mc * 8));
  JY_TRY(jy_ujson_pending_clear(eng, slots, k));
  JY_HIP(eng, hipStreamSynchronize(eng->stream));
  return JY_OK;
}

int32_t jy_ujson_flush_wire(jy_engine* eng, uint64_t cap_docs, uint64_t cap_key_bytes, uint64_t cap_el,
                            uint64_t cap_vv, uint64_t cap_cloud, uint8_t* key_bytes, uint64_t* key_offs,
                            uint64_t* el_offs, uint64_t* dots, uint64_t* elems, uint64_t* vv_offs, uint64_t* vv,
                            uint64_t* cloud_offs, uint64_t* cloud, uint64_t* sizes_out, int32_t mem) {
  JY_HIP(eng, hipSetDevice(eng->device));
  JY_TRY(mem_check(eng, mem));
  for (int q = 0; q < 5; q++) sizes_out[q] = 0;
  u64 k = 0;
  JY_TRY(jy_pending_count(eng, eng->uj_pend, &k));
  if (k == 0) return empty_batch(eng, mem, {key_offs, el_offs, vv_offs, cloud_offs});
  Tmp tmp(eng);
  Keys K;
  bool written;
  JY_TRY(pending_keys(eng, tmp, JY_UJSON, eng->uj_pend, k, K));
  JY_TRY(ujson_format(eng, tmp, K, k, eng->ujson_d, {cap_docs, cap_key_bytes, cap_el, cap_vv, cap_cloud},
                      UjsonWire{key_bytes, key_offs, el_offs, dots, elems, vv_offs, vv, cloud_offs, cloud},
                      sizes_out, mem, &written));
  if (!written) return JY_OK;
  JY_TRY(jy_ujson_pending_clear(eng, K.slots, k));
  return host_sync(eng, mem);
}

}  // extern "C"
