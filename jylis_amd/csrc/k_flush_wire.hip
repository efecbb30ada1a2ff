// k_flush_wire.hip -- flush_deltas() (repo_manager.pony:9, repo_gcount.pony:
// 18-23 and every repo_*.pony): the pending set (PendingSet) and every flush.
// One core per type, two output formats:
//   slot form (jy_*_flush): slots and arena handles, what jy_*_converge takes
//   wire form (jy_*_flush_wire): key strings and value bytes, the arrays
//     jy_node_*_converge takes, built on the device from the key directory
//     (KeyDir) and the value arenas
//
// Every flush runs the same steps: read the pending count (TLOG settles its
// merges first), select the pending slots (ascending), PEEK their deltas
// with the type's own peek (nothing is cleared yet), scan the lengths into
// offsets, read the totals back once, and only when every output capacity
// is large enough format the records, copy them out (emit) and run the
// type's one CLEAR.  The forms differ in the formatting alone, and in what a
// short capacity returns (the slot-form counter and TREG flushes: JY_ERANGE;
// every other one: JY_OK with the sizes).  Temporaries come from the
// engine's stream-ordered pool (Tmp): no flush uses a scratch slot.
//
// The string gather, the temporaries and the totals / emit helpers are
// shared with the state snapshots: jy_wire.hpp.

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

// TLOG, both forms: the k pending logs' cutoffs and entry offsets (eoff[k] = all entries)
int32_t tlog_sizes(jy_engine* eng, Tmp& tmp, const u32* slots, u64 k, u64** cuts, u64** eoff) {
  u64* lens;
  JY_TRY(tmp.get(&lens, k + 1));
  JY_TRY(tmp.get(cuts, k));
  JY_TRY(tmp.get(eoff, k + 1));
  JY_HIP(eng, hipMemsetAsync(lens + k, 0, 8, eng->stream));
  JY_TRY(jy_tlog_pending_sizes(eng, k, slots, lens, *cuts));
  return jy_scan_u64(eng, lens, *eoff, k);
}

// UJSON, both forms: the k pending docs' element and cloud offsets
int32_t ujson_sizes(jy_engine* eng, Tmp& tmp, const u32* slots, u64 k, u64** eo, u64** co) {
  u64 *se, *sc;
  JY_TRY(tmp.get(&se, k + 1));
  JY_TRY(tmp.get(&sc, k + 1));
  JY_TRY(tmp.get(eo, k + 1));
  JY_TRY(tmp.get(co, k + 1));
  JY_HIP(eng, hipMemsetAsync(se + k, 0, 8, eng->stream));
  JY_HIP(eng, hipMemsetAsync(sc + k, 0, 8, eng->stream));
  JY_TRY(jy_ujson_sizes_of(eng, eng->ujson_d, k, slots, se, sc));
  JY_TRY(jy_scan_u64(eng, se, *eo, k));
  return jy_scan_u64(eng, sc, *co, k);
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
  u64 tot[2];
  JY_TRY(totals(eng, {K.koff + k, coff + k}, tot));
  const u64 kbytes = tot[0], ncells = tot[1];
  sizes_out[0] = k;
  sizes_out[1] = kbytes;
  sizes_out[2] = ncells;
  if (cap_keys < k || cap_key_bytes < kbytes || cap_cells < ncells) return JY_OK;  // sizes only
  JY_TRY(emit_keys(eng, tmp, type, K, k, kbytes, key_bytes, key_offs, mem));
  uint8_t* ds;
  u16* dc;
  u64* dv;
  JY_TRY(tmp.out(&ds, sign, ncells, mem));
  JY_TRY(tmp.out(&dc, col_out, ncells, mem));
  JY_TRY(tmp.out(&dv, val, ncells, mem));
  LAUNCH(k_wire_cnt_cells, k, mask, vals, nsigns, (u16)col, k, coff, ds, dc, dv);
  JY_TRY(emit(eng, mem, sign, ds, ncells));
  JY_TRY(emit(eng, mem, col_out, dc, ncells * 2));
  JY_TRY(emit(eng, mem, val, dv, ncells * 8));
  JY_TRY(emit(eng, mem, cell_offs, coff, (k + 1) * 8));
  JY_TRY(jy_cnt_pending_clear(eng, w, K.slots, k));
  if (mem == JY_HOST) JY_HIP(eng, hipStreamSynchronize(eng->stream));
  return JY_OK;
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
  u64 *dt, *dp, *dl;
  JY_TRY(tmp.out(&ds, slot_out, k, mem));
  JY_TRY(tmp.out(&dt, ts_out, k, mem));
  JY_TRY(tmp.out(&dp, pre_out, k, mem));
  JY_TRY(tmp.out(&dl, lr_out, k, mem));
  JY_TRY(jy_pending_slots(eng, JY_TREG, eng->treg.pend, k, ds));
  JY_TRY(jy_treg_pending_peek(eng, ds, k, dt, dp, dl));
  JY_TRY(emit(eng, mem, slot_out, ds, k * 4));
  JY_TRY(emit(eng, mem, ts_out, dt, k * 8));
  JY_TRY(emit(eng, mem, pre_out, dp, k * 8));
  JY_TRY(emit(eng, mem, lr_out, dl, k * 8));
  JY_TRY(jy_treg_pending_clear(eng, ds, k));
  if (mem == JY_HOST) JY_HIP(eng, hipStreamSynchronize(eng->stream));
  return JY_OK;
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
  JY_TRY(pending_keys(eng, tmp, JY_TREG, eng->treg.pend, k, K));
  u64 *dts, *pre, *lr, *voff;
  JY_TRY(tmp.get(&dts, k));
  JY_TRY(tmp.get(&pre, k));
  JY_TRY(tmp.get(&lr, k));
  JY_TRY(jy_treg_pending_peek(eng, K.slots, k, dts, pre, lr));
  JY_TRY(value_offsets(eng, tmp, lr, k, &voff));
  u64 tot[2];
  JY_TRY(totals(eng, {K.koff + k, voff + k}, tot));
  const u64 kbytes = tot[0], vbytes = tot[1];
  sizes_out[0] = k;
  sizes_out[1] = kbytes;
  sizes_out[2] = vbytes;
  if (cap_keys < k || cap_key_bytes < kbytes || cap_val_bytes < vbytes) return JY_OK;  // sizes only
  JY_TRY(emit_keys(eng, tmp, JY_TREG, K, k, kbytes, key_bytes, key_offs, mem));
  JY_TRY(emit(eng, mem, ts, dts, k * 8));
  JY_TRY(emit_values(eng, tmp, JY_TREG, pre, lr, voff, k, vbytes, val_bytes, val_offs, mem));
  JY_TRY(jy_treg_pending_clear(eng, K.slots, k));
  if (mem == JY_HOST) JY_HIP(eng, hipStreamSynchronize(eng->stream));
  return JY_OK;
}

// ---- TLOG ----
int32_t jy_tlog_flush(jy_engine* eng, uint64_t cap_keys, uint64_t cap_ent, uint32_t* slot_out, uint64_t* cutoff_out,
                      uint64_t* offs_out, uint64_t* ts_out, uint64_t* pre_out, uint64_t* lr_out, uint64_t* nkeys_out,
                      uint64_t* nent_out, int32_t mem) {
  JY_HIP(eng, hipSetDevice(eng->device));
  *nkeys_out = *nent_out = 0;
  JY_TRY(jy_tlog_settle(eng));
  u64 k = 0, m = 0;
  JY_TRY(jy_pending_count(eng, eng->tl_pend, &k));
  *nkeys_out = k;
  if (k == 0) return JY_OK;
  Tmp tmp(eng);
  u32* slots;
  u64 *cuts, *eoff;
  JY_TRY(pending_slots(eng, tmp, JY_TLOG, eng->tl_pend, k, &slots));
  JY_TRY(tlog_sizes(eng, tmp, slots, k, &cuts, &eoff));
  JY_TRY(totals(eng, {eoff + k}, &m));
  *nent_out = m;
  if (cap_keys < k || cap_ent < m) return JY_OK;  // sizes only
  u64 *dt, *dp, *dl;
  JY_TRY(tmp.out(&dt, ts_out, m, mem));
  JY_TRY(tmp.out(&dp, pre_out, m, mem));
  JY_TRY(tmp.out(&dl, lr_out, m, mem));
  if (m) JY_TRY(jy_tlog_pending_gather(eng, k, slots, eoff, dt, dp, dl));
  JY_TRY(emit(eng, mem, slot_out, slots, k * 4));
  JY_TRY(emit(eng, mem, cutoff_out, cuts, k * 8));
  JY_TRY(emit(eng, mem, offs_out, eoff, (k + 1) * 8));
  JY_TRY(emit(eng, mem, ts_out, dt, m * 8));
  JY_TRY(emit(eng, mem, pre_out, dp, m * 8));
  JY_TRY(emit(eng, mem, lr_out, dl, m * 8));
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
  JY_TRY(pending_keys(eng, tmp, JY_TLOG, eng->tl_pend, k, K));
  u64 *cuts, *eoff;
  JY_TRY(tlog_sizes(eng, tmp, K.slots, k, &cuts, &eoff));
  u64 tot[2];
  JY_TRY(totals(eng, {K.koff + k, eoff + k}, tot));
  const u64 kbytes = tot[0], m = tot[1];
  // (the value bytes are a size of the batch: the entries are read before the capacity check)
  u64 *dts, *pre, *lr, *voff;
  JY_TRY(tmp.get(&dts, m));
  JY_TRY(tmp.get(&pre, m));
  JY_TRY(tmp.get(&lr, m));
  if (m) JY_TRY(jy_tlog_pending_gather(eng, k, K.slots, eoff, dts, pre, lr));
  JY_TRY(value_offsets(eng, tmp, lr, m, &voff));
  u64 vbytes = 0;
  JY_TRY(totals(eng, {voff + m}, &vbytes));
  sizes_out[0] = k;
  sizes_out[1] = kbytes;
  sizes_out[2] = m;
  sizes_out[3] = vbytes;
  if (cap_keys < k || cap_key_bytes < kbytes || cap_ent < m || cap_val_bytes < vbytes) return JY_OK;  // sizes only
  JY_TRY(emit_keys(eng, tmp, JY_TLOG, K, k, kbytes, key_bytes, key_offs, mem));
  JY_TRY(emit(eng, mem, cutoff, cuts, k * 8));
  JY_TRY(emit(eng, mem, ent_offs, eoff, (k + 1) * 8));
  JY_TRY(emit(eng, mem, ts, dts, m * 8));
  JY_TRY(emit_values(eng, tmp, JY_TLOG, pre, lr, voff, m, vbytes, val_bytes, val_offs, mem));
  JY_TRY(jy_tlog_pending_clear(eng, K.slots, k));
  if (mem == JY_HOST) JY_HIP(eng, hipStreamSynchronize(eng->stream));
  return JY_OK;
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
  UjsonState& d = eng->ujson_d;
  Tmp tmp(eng);
  u32* slots;
  u64 *eo, *co;
  JY_TRY(pending_slots(eng, tmp, JY_UJSON, eng->uj_pend, k, &slots));
  JY_TRY(ujson_sizes(eng, tmp, slots, k, &eo, &co));
  u64 tot[2];
  JY_TRY(totals(eng, {eo + k, co + k}, tot));
  const u64 me = tot[0], mc = tot[1];
  *nel_out = me;
  *ncl_out = mc;
  if (cap_docs < k || cap_el < me || cap_cl < mc) return JY_OK;  // sizes only
  u64 *dd, *de, *dv, *dc;
  JY_TRY(tmp.out(&dd, dots_out, me, mem));
  JY_TRY(tmp.out(&de, elems_out, me, mem));
  JY_TRY(tmp.out(&dv, vv_out, k * d.R, mem));  // dense [k][R]
  JY_TRY(tmp.out(&dc, cloud_out, mc, mem));
  JY_TRY(jy_ujson_gather_of(eng, d, k, slots, eo, co, me, mc, dd, de, dv, dc));
  JY_TRY(emit(eng, mem, slot_out, slots, k * 4));
  JY_TRY(emit(eng, mem, eoff_out, eo, (k + 1) * 8));
  JY_TRY(emit(eng, mem, coff_out, co, (k + 1) * 8));
  JY_TRY(emit(eng, mem, dots_out, dd, me * 8));
  JY_TRY(emit(eng, mem, elems_out, de, me * 8));
  JY_TRY(emit(eng, mem, vv_out, dv, k * d.R * 8));
  JY_TRY(emit(eng, mem, cloud_out, dc, mc * 8));
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
  UjsonState& d = eng->ujson_d;
  const u32 R = d.R;
  Tmp tmp(eng);
  Keys K;
  JY_TRY(pending_keys(eng, tmp, JY_UJSON, eng->uj_pend, k, K));
  u64 *eo, *co, *sv, *vo;
  JY_TRY(ujson_sizes(eng, tmp, K.slots, k, &eo, &co));
  JY_TRY(tmp.get(&sv, k + 1));
  JY_TRY(tmp.get(&vo, k + 1));
  LAUNCH(k_wire_vv_count, k + 1, d.vv, R, K.slots, k, sv);
  JY_TRY(jy_scan_u64(eng, sv, vo, k));
  u64 tot[4];
  JY_TRY(totals(eng, {K.koff + k, eo + k, vo + k, co + k}, tot));
  const u64 kbytes = tot[0], me = tot[1], mv = tot[2], mc = tot[3];
  sizes_out[0] = k;
  sizes_out[1] = kbytes;
  sizes_out[2] = me;
  sizes_out[3] = mv;
  sizes_out[4] = mc;
  if (cap_docs < k || cap_key_bytes < kbytes || cap_el < me || cap_vv < mv || cap_cloud < mc) return JY_OK;
  JY_TRY(emit_keys(eng, tmp, JY_UJSON, K, k, kbytes, key_bytes, key_offs, mem));
  u64 *dd, *de, *dv, *dc, *dense;
  JY_TRY(tmp.out(&dd, dots, me, mem));
  JY_TRY(tmp.out(&de, elems, me, mem));
  JY_TRY(tmp.out(&dv, vv, mv, mem));
  JY_TRY(tmp.out(&dc, cloud, mc, mem));
  JY_TRY(tmp.get(&dense, k * R));
  // element and cloud CSRs come out in converge order (dots ascending per doc)
  JY_TRY(jy_ujson_gather_of(eng, d, k, K.slots, eo, co, me, mc, dd, de, dense, dc));
  if (mv) LAUNCH(k_wire_vv_pack, k, dense, R, k, vo, dv);
  JY_TRY(emit(eng, mem, dots, dd, me * 8));
  JY_TRY(emit(eng, mem, elems, de, me * 8));
  JY_TRY(emit(eng, mem, vv, dv, mv * 8));
  JY_TRY(emit(eng, mem, cloud, dc, mc * 8));
  JY_TRY(emit(eng, mem, el_offs, eo, (k + 1) * 8));
  JY_TRY(emit(eng, mem, vv_offs, vo, (k + 1) * 8));
  JY_TRY(emit(eng, mem, cloud_offs, co, (k + 1) * 8));
  JY_TRY(jy_ujson_pending_clear(eng, K.slots, k));
  if (mem == JY_HOST) JY_HIP(eng, hipStreamSynchronize(eng->stream));
  return JY_OK;
}

}  // extern "C"

