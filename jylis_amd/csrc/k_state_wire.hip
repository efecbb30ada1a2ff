// k_state_wire.hip -- the STATE of a slot range as a ready-to-converge batch
// (jy_*_state_wire): record i is the state of slot slot0 + i, as exactly the
// arrays the same type's jy_node_*_converge and jy_*_flush_wire use.  What a
// host needs to bring a late peer up to date (anti-entropy), to persist a
// store (repo_manager.pony:100,107 "TODO: disk persistence?") and to reshard.
//
// Every call runs the flush's steps without its pending set and without a
// clear: the slot list is slot0 + i (k_wire_iota fills it once, so every
// reader that takes a device slot array is reused unchanged), the type's
// state reader gives sizes, a scan turns them into offsets, the totals are
// read back once, and only when every capacity is large enough the records
// are formatted and copied out (jy_wire.hpp).  Nothing is written to the
// engine's state, pending sets, arenas or key directory.
//
// TREG, TLOG and UJSON compose jy_treg_gather, jy_tlog_sizes / _gather and
// jy_ujson_sizes / _gather with the shared string gather.  Counters have no
// reader that yields cells; theirs is the one new hot kernel:
//
// Counter slab [sign][col][kcap] -> per-key CSR of (sign, col, val), the
// non-zero cells, P before N, columns ascending.  Row r = sign * ncols + col.
//   k_state_cnt_count   a lane per slot walks the rows; consecutive lanes
//                       read consecutive slots of one row (coalesced, 8 B per
//                       lane).  Writes the slot's cell count and, while the
//                       rows fit kMaskRows bits, its non-zero row mask.
//   jy_scan_u64         counts -> cell_offs
//   writer, two forms (A/B in DESIGN.md, "State snapshot in wire form"):
//   k_state_cnt_tile    a workgroup takes kTileSlots slots.  It stages their
//                       masks and its slice of cell_offs in LDS, loads only
//                       the cells the masks name (half-wave-wide row segments),
//                       places each at cell_offs[slot] + rank(mask, row) in an
//                       LDS image of the tile's output, and then stores that
//                       image with lanes on consecutive output cells.
//   k_state_cnt_lane    a lane per slot writes its own run of cells.  Valid
//                       for any row count: the fallback above kMaskRows rows
//                       (counter_columns grows at run time, up to 65,535).
// The slab is read once by a call that only sizes and at most twice by one
// that writes (count, then the cells the masks name; every row again by the
// fallback without masks).

#include <cstdlib>
#include <cstring>

#include "jy_wire.hpp"

namespace {

constexpr u32 kMaskRows = 128;   // rows (nsigns * ncols) a per-slot mask holds: two u64
constexpr u32 kTileSlots = 32;   // slots per workgroup of the tile writer (32 KB of staged values)
constexpr u32 kRowGroups = kThreads / kTileSlots;

__device__ __forceinline__ bool mask_bit(u64 m0, u64 m1, u32 r) { return ((r < 64 ? m0 >> r : m1 >> (r - 64)) & 1) != 0; }
// set bits of the mask below row r
__device__ __forceinline__ u32 mask_rank(u64 m0, u64 m1, u32 r) {
  if (r < 64) return (u32)__popcll(m0 & ((1ull << r) - 1));
  return (u32)__popcll(m0) + (u32)__popcll(m1 & ((1ull << (r - 64)) - 1));
}

// ncell[j] = non-zero cells of slot slot0 + j (ncell[n] = 0 for the scan);
// kMask: mask[2j], mask[2j + 1] = bit r set iff row r's cell is non-zero
// kList (the slot-list dumps): record j is the state of slot list[j] instead of slot0 + j
template <bool kMask, bool kList = false>
__global__ __launch_bounds__(kThreads) void k_state_cnt_count(Slab S, u64 slot0, const u32* __restrict__ list, u64 n,
                                                              u64* __restrict__ ncell, u64* __restrict__ mask) {
  const u64 j = gid();
  if (j > n) return;
  if (j == n) {
    ncell[n] = 0;
    return;
  }
  const u64 s = kList ? list[j] : slot0 + j;
  u64 c = 0, m0 = 0, m1 = 0;
#pragma unroll 4
  for (u32 r = 0; r < S.rows; r++) {
    const u64 nz = S.row(r)[s] != 0;
    c += nz;
    if (kMask) {
      if (r < 64) m0 |= nz << r; else m1 |= nz << (r - 64);
    }
  }
  ncell[j] = c;
  if (kMask) {
    mask[2 * j] = m0;
    mask[2 * j + 1] = m1;
  }
}

// the lane-per-slot writer: slot j's cells go to coff[j] ..., in row order
template <bool kMask, bool kList = false>
__global__ __launch_bounds__(kThreads) void k_state_cnt_lane(Slab S, u64 slot0, const u32* __restrict__ list, u64 n,
                                                             const u64* __restrict__ coff,
                                                             const u64* __restrict__ mask,
                                                             uint8_t* __restrict__ sign, u16* __restrict__ col,
                                                             u64* __restrict__ val) {
  const u64 j = gid();
  if (j >= n) return;
  const u64 s = kList ? list[j] : slot0 + j;
  u64 m0 = 0, m1 = 0;
  if (kMask) {
    m0 = mask[2 * j];
    m1 = mask[2 * j + 1];
  }
  u64 o = coff[j];
#pragma unroll 4
  for (u32 r = 0; r < S.rows; r++) {
    if (kMask && !mask_bit(m0, m1, r)) continue;
    const u64 v = S.row(r)[s];
    if (v) {
      const u32 sg = r >= S.ncols ? 1u : 0u;
      sign[o] = (uint8_t)sg;
      col[o] = (u16)(r - sg * S.ncols);
      val[o] = v;
      o++;
    }
  }
}

// the tile writer (S.rows <= kMaskRows): stores by output position.  For a
// slot list only the STORES stay coalesced: the loads' half-wave row segments
// are consecutive slots only where the list is (a sparse list reads a cell
// per 64-B sector, as the lane writer does)
template <bool kList = false>
__global__ __launch_bounds__(kThreads) void k_state_cnt_tile(Slab S, u64 slot0, const u32* __restrict__ list, u64 n,
                                                             const u64* __restrict__ coff,
                                                             const u64* __restrict__ mask,
                                                             uint8_t* __restrict__ sign, u16* __restrict__ col,
                                                             u64* __restrict__ val) {
  __shared__ u64 sv[kTileSlots * kMaskRows];      // the tile's output values, in output order
  __shared__ uint8_t sr[kTileSlots * kMaskRows];  // ... and each one's row
  __shared__ u64 sm[2 * kTileSlots];
  __shared__ u64 so[kTileSlots + 1];
  const u64 t0 = (u64)blockIdx.x * kTileSlots;
  if (t0 >= n) return;
  const u32 nt = (u32)std::min<u64>(kTileSlots, n - t0);
  for (u32 q = threadIdx.x; q <= nt; q += kThreads) so[q] = coff[t0 + q];
  for (u32 q = threadIdx.x; q < 2 * nt; q += kThreads) sm[q] = mask[2 * t0 + q];
  __syncthreads();
  const u32 ls = threadIdx.x % kTileSlots, rg = threadIdx.x / kTileSlots;
  if (ls < nt) {
    const u64 m0 = sm[2 * ls], m1 = sm[2 * ls + 1];
    const u32 base = (u32)(so[ls] - so[0]);  // < nt * rows: every slot before it holds at most `rows` cells
    const u64 s = kList ? list[t0 + ls] : slot0 + t0 + ls;
#pragma unroll 4
    for (u32 r = rg; r < S.rows; r += kRowGroups) {
      if (!mask_bit(m0, m1, r)) continue;
      const u32 at = base + mask_rank(m0, m1, r);
      sv[at] = S.row(r)[s];
      sr[at] = (uint8_t)r;
    }
  }
  __syncthreads();
  const u64 o0 = so[0];
  const u32 total = (u32)(so[nt] - o0);
  for (u32 q = threadIdx.x; q < total; q += kThreads) {
    const u32 r = sr[q];
    const u32 sg = r >= S.ncols ? 1u : 0u;
    sign[o0 + q] = (uint8_t)sg;
    col[o0 + q] = (u16)(r - sg * S.ncols);
    val[o0 + q] = sv[q];
  }
}

// [slot0, slot0 + nslots) must lie inside the type's interned keys
int32_t range_check(jy_engine* eng, int32_t type, u64 slot0, u64 nslots) {
  const u64 nk = eng->nkeys[type];
  if (slot0 > nk || nslots > nk - slot0) return eng->fail(JY_ERANGE, "slot range reaches past the interned keys");
  return JY_OK;
}

// the range's slot list and its key lengths / offsets
int32_t range_keys(jy_engine* eng, Tmp& tmp, int32_t type, u64 slot0, u64 n, Keys& K) {
  JY_TRY(tmp.get(&K.slots, n));
  LAUNCH(k_wire_iota, n, (u32)slot0, n, K.slots);
  return key_offsets(eng, tmp, type, n, K);
}

// err |= 1: list[j] <= list[j - 1] (not strictly ascending), |= 2: list[j] >= nk
__global__ __launch_bounds__(kThreads) void k_wire_list_check(const u32* __restrict__ list, u64 n, u64 nk,
                                                              u32* __restrict__ err) {
  const u64 j = gid();
  if (j >= n) return;
  const u32 s = list[j];
  const u32 e = (j > 0 && s <= list[j - 1] ? 1u : 0u) | (s >= nk ? 2u : 0u);
  if (e) atomicOr(err, e);
}

// range_keys' sibling for a caller's slot list (n > 0): a copy of the list,
// checked ON THE DEVICE to be strictly ascending and inside the interned keys
// before any reader indexes state with it.  The error word is read back
// before the key lengths are (they are indexed by the list), so a list call
// waits for the stream once more than a range call.
int32_t list_keys(jy_engine* eng, Tmp& tmp, int32_t type, u64 n, const u32* list, int32_t list_mem, Keys& K) {
  u32* err;
  JY_TRY(tmp.get(&K.slots, n));
  JY_TRY(tmp.get(&err, 2));
  JY_HIP(eng, hipMemsetAsync(err, 0, 8, eng->stream));
  JY_HIP(eng, hipMemcpyAsync(K.slots, list, n * 4, list_mem == JY_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice,
                             eng->stream));
  LAUNCH(k_wire_list_check, n, K.slots, n, eng->nkeys[type], err);
  u64 e = 0;
  JY_TRY(totals(eng, {reinterpret_cast<const u64*>(err)}, &e));
  if (e & 2) return eng->fail(JY_ERANGE, "slot list names a slot past the interned keys");
  if (e & 1) return eng->fail(JY_EINVAL, "slot list is not strictly ascending");
  return key_offsets(eng, tmp, type, n, K);
}

// the slots of one dump: the range [slot0, slot0 + n), or the n slots of `list`
struct Sel {
  bool is_list;
  u64 slot0, n;
  const u32* list;  // is_list: the n slots (may be null only when n == 0)
  int32_t list_mem;
  static Sel range(u64 slot0, u64 n) { return Sel{false, slot0, n, nullptr, JY_HOST}; }
  static Sel slots(u64 n, const u32* list, int32_t mem) { return Sel{true, 0, n, list, mem}; }
};
int32_t sel_keys(jy_engine* eng, Tmp& tmp, int32_t type, const Sel& sel, Keys& K) {
  if (sel.is_list) return list_keys(eng, tmp, type, sel.n, sel.list, sel.list_mem, K);
  return range_keys(eng, tmp, type, sel.slot0, sel.n, K);
}
int32_t sel_check(jy_engine* eng, int32_t type, const Sel& sel) {
  if (!sel.is_list) return range_check(eng, type, sel.slot0, sel.n);
  if (sel.list_mem != JY_HOST && sel.list_mem != JY_DEVICE)
    return eng->fail(JY_EINVAL, "slots_mem must be JY_HOST or JY_DEVICE");
  if (sel.n > 0 && !sel.list) return eng->fail(JY_EINVAL, "slot list is null");
  return JY_OK;
}

// JY_STATE_CELLS=lane in the environment: the lane-per-slot writer at every
// width (the A/B of tools/state_wire_time.py); read at each call
bool force_lane_writer() {
  const char* v = std::getenv("JY_STATE_CELLS");
  return v && std::strcmp(v, "lane") == 0;
}


int32_t counter_wire(jy_engine* eng, int32_t type, const Sel& sel, uint64_t cap_key_bytes,
                              uint64_t cap_cells, uint8_t* key_bytes, uint64_t* key_offs, uint64_t* cell_offs,
                              uint8_t* sign, uint16_t* col, uint64_t* val, uint64_t* sizes_out, int32_t mem) {
  JY_HIP(eng, hipSetDevice(eng->device));
  if (type != JY_GCOUNT && type != JY_PNCOUNT) return eng->fail(JY_ETYPE, "not a counter type");
  JY_TRY(mem_check(eng, mem));
  sizes_out[0] = sizes_out[1] = sizes_out[2] = 0;
  JY_TRY(sel_check(eng, type, sel));
  const u64 n = sel.n;
  if (n == 0) return empty_batch(eng, mem, {key_offs, cell_offs});
  const int w = type == JY_GCOUNT ? 0 : 1;
  const CounterState& c = eng->cnt[w];
  // columns past the slab's capacity were never written: all zero, no cells
  const u32 ncols = std::min<u32>((u32)eng->rep_id.size(), c.ccap);
  const Slab S{c.slab, c.kcap, (u64)c.ccap * c.kcap, ncols, (u32)(w + 1) * ncols};
  const bool masked = S.rows <= kMaskRows;
  Tmp tmp(eng);
  Keys K;
  JY_TRY(sel_keys(eng, tmp, type, sel, K));
  u64 *ncell, *coff, *mask = nullptr;
  JY_TRY(tmp.get(&ncell, n + 1));
  JY_TRY(tmp.get(&coff, n + 1));
  const u64 slot0 = sel.slot0;
  const u32* list = sel.is_list ? K.slots : nullptr;  // (the checked device copy)
  if (masked) JY_TRY(tmp.get(&mask, 2 * n));
  if (list) {
    if (masked) LAUNCH((k_state_cnt_count<true, true>), n + 1, S, slot0, list, n, ncell, mask);
    else LAUNCH((k_state_cnt_count<false, true>), n + 1, S, slot0, list, n, ncell, mask);
  } else {
    if (masked) LAUNCH(k_state_cnt_count<true>, n + 1, S, slot0, list, n, ncell, mask);
    else LAUNCH(k_state_cnt_count<false>, n + 1, S, slot0, list, n, ncell, mask);
  }
  JY_TRY(jy_scan_u64(eng, ncell, coff, n));
  u64 tot[2];
  JY_TRY(totals(eng, {K.koff + n, coff + n}, tot));
  const u64 kbytes = tot[0], ncells = tot[1];
  sizes_out[0] = n;
  sizes_out[1] = kbytes;
  sizes_out[2] = ncells;
  if (cap_key_bytes < kbytes || cap_cells < ncells) return JY_OK;  // sizes only
  JY_TRY(emit_keys(eng, tmp, type, K, n, kbytes, key_bytes, key_offs, mem));
  uint8_t* ds;
  u16* dc;
  u64* dv;
  JY_TRY(tmp.out(&ds, sign, ncells, mem));
  JY_TRY(tmp.out(&dc, col, ncells, mem));
  JY_TRY(tmp.out(&dv, val, ncells, mem));
  if (ncells) {
    const u64 tiles = (n + kTileSlots - 1) / kTileSlots;
    if (!masked) {
      if (list) LAUNCH((k_state_cnt_lane<false, true>), n, S, slot0, list, n, coff, mask, ds, dc, dv);
      else LAUNCH(k_state_cnt_lane<false>, n, S, slot0, list, n, coff, mask, ds, dc, dv);
    } else if (force_lane_writer()) {
      if (list) LAUNCH((k_state_cnt_lane<true, true>), n, S, slot0, list, n, coff, mask, ds, dc, dv);
      else LAUNCH(k_state_cnt_lane<true>, n, S, slot0, list, n, coff, mask, ds, dc, dv);
    } else if (list) {
      hipLaunchKernelGGL(k_state_cnt_tile<true>, dim3((u32)tiles), dim3(kThreads), 0, eng->stream, S, slot0, list, n,
                         coff, mask, ds, dc, dv);
      JY_HIP(eng, hipGetLastError());
    } else {
      hipLaunchKernelGGL(k_state_cnt_tile<false>, dim3((u32)tiles), dim3(kThreads), 0, eng->stream, S, slot0, list, n,
                         coff, mask, ds, dc, dv);
      JY_HIP(eng, hipGetLastError());
    }
  }
  JY_TRY(emit(eng, mem, sign, ds, ncells));
  JY_TRY(emit(eng, mem, col, dc, ncells * 2));
  JY_TRY(emit(eng, mem, val, dv, ncells * 8));
  JY_TRY(emit(eng, mem, cell_offs, coff, (n + 1) * 8));
  if (mem == JY_HOST) JY_HIP(eng, hipStreamSynchronize(eng->stream));
  return JY_OK;
}

int32_t treg_wire(jy_engine* eng, const Sel& sel, uint64_t cap_key_bytes,
                           uint64_t cap_val_bytes, uint8_t* key_bytes, uint64_t* key_offs, uint64_t* ts,
                           uint8_t* val_bytes, uint64_t* val_offs, uint64_t* sizes_out, int32_t mem) {
  JY_HIP(eng, hipSetDevice(eng->device));
  JY_TRY(mem_check(eng, mem));
  sizes_out[0] = sizes_out[1] = sizes_out[2] = 0;
  JY_TRY(sel_check(eng, JY_TREG, sel));
  const u64 n = sel.n;
  if (n == 0) return empty_batch(eng, mem, {key_offs, val_offs});
  Tmp tmp(eng);
  Keys K;
  JY_TRY(sel_keys(eng, tmp, JY_TREG, sel, K));
  u64 *dts, *pre, *lr, *voff;
  JY_TRY(tmp.get(&dts, n));
  JY_TRY(tmp.get(&pre, n));
  JY_TRY(tmp.get(&lr, n));
  JY_TRY(jy_treg_gather(eng, n, K.slots, dts, pre, lr));
  JY_TRY(value_offsets(eng, tmp, lr, n, &voff));
  u64 tot[2];
  JY_TRY(totals(eng, {K.koff + n, voff + n}, tot));
  // every launch before this read has finished: a duplicate-list overflow fails it, as jy_treg_read
  JY_TRY(jy_treg_overflow_check(eng));
  const u64 kbytes = tot[0], vbytes = tot[1];
  sizes_out[0] = n;
  sizes_out[1] = kbytes;
  sizes_out[2] = vbytes;
  if (cap_key_bytes < kbytes || cap_val_bytes < vbytes) return JY_OK;  // sizes only
  JY_TRY(emit_keys(eng, tmp, JY_TREG, K, n, kbytes, key_bytes, key_offs, mem));
  JY_TRY(emit(eng, mem, ts, dts, n * 8));
  JY_TRY(emit_values(eng, tmp, JY_TREG, pre, lr, voff, n, vbytes, val_bytes, val_offs, mem));
  if (mem == JY_HOST) JY_HIP(eng, hipStreamSynchronize(eng->stream));
  return JY_OK;
}

int32_t tlog_wire(jy_engine* eng, const Sel& sel, uint64_t cap_key_bytes, uint64_t cap_ent,
                           uint64_t cap_val_bytes, uint8_t* key_bytes, uint64_t* key_offs, uint64_t* cutoff,
                           uint64_t* ent_offs, uint64_t* ts, uint8_t* val_bytes, uint64_t* val_offs,
                           uint64_t* sizes_out, int32_t mem) {
  JY_HIP(eng, hipSetDevice(eng->device));
  JY_TRY(mem_check(eng, mem));
  for (int q = 0; q < 4; q++) sizes_out[q] = 0;
  JY_TRY(sel_check(eng, JY_TLOG, sel));
  const u64 n = sel.n;
  if (n == 0) return empty_batch(eng, mem, {key_offs, ent_offs, val_offs});
  JY_TRY(jy_tlog_settle(eng));
  Tmp tmp(eng);
  Keys K;
  JY_TRY(sel_keys(eng, tmp, JY_TLOG, sel, K));
  u64 *lens, *cuts, *eoff;
  JY_TRY(tmp.get(&lens, n + 1));
  JY_TRY(tmp.get(&cuts, n));
  JY_TRY(tmp.get(&eoff, n + 1));
  JY_HIP(eng, hipMemsetAsync(lens + n, 0, 8, eng->stream));
  JY_TRY(jy_tlog_sizes(eng, n, K.slots, lens, cuts));
  JY_TRY(jy_scan_u64(eng, lens, eoff, n));
  u64 tot[2];
  JY_TRY(totals(eng, {K.koff + n, eoff + n}, tot));
  const u64 kbytes = tot[0], m = tot[1];
  // (the value bytes are a size of the batch: the entries are read before the capacity check)
  u64 *dts, *pre, *lr, *voff;
  JY_TRY(tmp.get(&dts, m));
  JY_TRY(tmp.get(&pre, m));
  JY_TRY(tmp.get(&lr, m));
  if (m) JY_TRY(jy_tlog_gather(eng, n, K.slots, eoff, dts, pre, lr));
  JY_TRY(value_offsets(eng, tmp, lr, m, &voff));
  u64 vbytes = 0;
  JY_TRY(totals(eng, {voff + m}, &vbytes));
  sizes_out[0] = n;
  sizes_out[1] = kbytes;
  sizes_out[2] = m;
  sizes_out[3] = vbytes;
  if (cap_key_bytes < kbytes || cap_ent < m || cap_val_bytes < vbytes) return JY_OK;  // sizes only
  JY_TRY(emit_keys(eng, tmp, JY_TLOG, K, n, kbytes, key_bytes, key_offs, mem));
  JY_TRY(emit(eng, mem, cutoff, cuts, n * 8));
  JY_TRY(emit(eng, mem, ent_offs, eoff, (n + 1) * 8));
  JY_TRY(emit(eng, mem, ts, dts, m * 8));
  JY_TRY(emit_values(eng, tmp, JY_TLOG, pre, lr, voff, m, vbytes, val_bytes, val_offs, mem));
  if (mem == JY_HOST) JY_HIP(eng, hipStreamSynchronize(eng->stream));
  return JY_OK;
}

int32_t ujson_wire(jy_engine* eng, const Sel& sel, uint64_t cap_key_bytes, uint64_t cap_el,
                            uint64_t cap_vv, uint64_t cap_cloud, uint8_t* key_bytes, uint64_t* key_offs,
                            uint64_t* el_offs, uint64_t* dots, uint64_t* elems, uint64_t* vv_offs, uint64_t* vv,
                            uint64_t* cloud_offs, uint64_t* cloud, uint64_t* sizes_out, int32_t mem) {
  JY_HIP(eng, hipSetDevice(eng->device));
  JY_TRY(mem_check(eng, mem));
  for (int q = 0; q < 5; q++) sizes_out[q] = 0;
  JY_TRY(sel_check(eng, JY_UJSON, sel));
  const u64 n = sel.n;
  if (n == 0) return empty_batch(eng, mem, {key_offs, el_offs, vv_offs, cloud_offs});
  const UjsonState& d = eng->ujson;
  const u32 R = d.R;
  Tmp tmp(eng);
  Keys K;
  JY_TRY(sel_keys(eng, tmp, JY_UJSON, sel, K));
  u64 *se, *sc, *sv, *eo, *co, *vo;
  JY_TRY(tmp.get(&se, n + 1));
  JY_TRY(tmp.get(&sc, n + 1));
  JY_TRY(tmp.get(&sv, n + 1));
  JY_TRY(tmp.get(&eo, n + 1));
  JY_TRY(tmp.get(&co, n + 1));
  JY_TRY(tmp.get(&vo, n + 1));
  JY_HIP(eng, hipMemsetAsync(se + n, 0, 8, eng->stream));
  JY_HIP(eng, hipMemsetAsync(sc + n, 0, 8, eng->stream));
  JY_TRY(jy_ujson_sizes(eng, n, K.slots, se, sc));
  LAUNCH(k_wire_vv_count, n + 1, d.vv, R, K.slots, n, sv);
  JY_TRY(jy_scan_u64(eng, se, eo, n));
  JY_TRY(jy_scan_u64(eng, sc, co, n));
  JY_TRY(jy_scan_u64(eng, sv, vo, n));
  u64 tot[4];
  JY_TRY(totals(eng, {K.koff + n, eo + n, vo + n, co + n}, tot));
  const u64 kbytes = tot[0], me = tot[1], mv = tot[2], mc = tot[3];
  sizes_out[0] = n;
  sizes_out[1] = kbytes;
  sizes_out[2] = me;
  sizes_out[3] = mv;
  sizes_out[4] = mc;
  if (cap_key_bytes < kbytes || cap_el < me || cap_vv < mv || cap_cloud < mc) return JY_OK;  // sizes only
  JY_TRY(emit_keys(eng, tmp, JY_UJSON, K, n, kbytes, key_bytes, key_offs, mem));
  u64 *dd, *de, *dv, *dc, *dense;
  JY_TRY(tmp.out(&dd, dots, me, mem));
  JY_TRY(tmp.out(&de, elems, me, mem));
  JY_TRY(tmp.out(&dv, vv, mv, mem));
  JY_TRY(tmp.out(&dc, cloud, mc, mem));
  JY_TRY(tmp.get(&dense, n * R));
  // element and cloud CSRs come out in converge order (dots ascending per doc),
  // for documents in the per-column layout too (jy_ujson_gather)
  JY_TRY(jy_ujson_gather(eng, n, K.slots, eo, co, me, mc, dd, de, dense, dc));
  if (mv) LAUNCH(k_wire_vv_pack, n, dense, R, n, vo, dv);
  JY_TRY(emit(eng, mem, dots, dd, me * 8));
  JY_TRY(emit(eng, mem, elems, de, me * 8));
  JY_TRY(emit(eng, mem, vv, dv, mv * 8));
  JY_TRY(emit(eng, mem, cloud, dc, mc * 8));
  JY_TRY(emit(eng, mem, el_offs, eo, (n + 1) * 8));
  JY_TRY(emit(eng, mem, vv_offs, vo, (n + 1) * 8));
  JY_TRY(emit(eng, mem, cloud_offs, co, (n + 1) * 8));
  if (mem == JY_HOST) JY_HIP(eng, hipStreamSynchronize(eng->stream));
  return JY_OK;
}

}  // namespace

extern "C" {

uint32_t jy_counter_state_mask_rows(void) { return kMaskRows; }

int32_t jy_counter_state_wire(jy_engine* eng, int32_t type, uint64_t slot0, uint64_t nslots, uint64_t cap_key_bytes,
                              uint64_t cap_cells, uint8_t* key_bytes, uint64_t* key_offs, uint64_t* cell_offs,
                              uint8_t* sign, uint16_t* col, uint64_t* val, uint64_t* sizes_out, int32_t mem) {
  return counter_wire(eng, type, Sel::range(slot0, nslots), cap_key_bytes, cap_cells, key_bytes, key_offs,
                      cell_offs, sign, col, val, sizes_out, mem);
}
int32_t jy_treg_state_wire(jy_engine* eng, uint64_t slot0, uint64_t nslots, uint64_t cap_key_bytes,
                           uint64_t cap_val_bytes, uint8_t* key_bytes, uint64_t* key_offs, uint64_t* ts,
                           uint8_t* val_bytes, uint64_t* val_offs, uint64_t* sizes_out, int32_t mem) {
  return treg_wire(eng, Sel::range(slot0, nslots), cap_key_bytes, cap_val_bytes, key_bytes, key_offs, ts,
                   val_bytes, val_offs, sizes_out, mem);
}
int32_t jy_tlog_state_wire(jy_engine* eng, uint64_t slot0, uint64_t nslots, uint64_t cap_key_bytes, uint64_t cap_ent,
                           uint64_t cap_val_bytes, uint8_t* key_bytes, uint64_t* key_offs, uint64_t* cutoff,
                           uint64_t* ent_offs, uint64_t* ts, uint8_t* val_bytes, uint64_t* val_offs,
                           uint64_t* sizes_out, int32_t mem) {
  return tlog_wire(eng, Sel::range(slot0, nslots), cap_key_bytes, cap_ent, cap_val_bytes, key_bytes,
                   key_offs, cutoff, ent_offs, ts, val_bytes, val_offs, sizes_out, mem);
}
int32_t jy_ujson_state_wire(jy_engine* eng, uint64_t slot0, uint64_t nslots, uint64_t cap_key_bytes, uint64_t cap_el,
                            uint64_t cap_vv, uint64_t cap_cloud, uint8_t* key_bytes, uint64_t* key_offs,
                            uint64_t* el_offs, uint64_t* dots, uint64_t* elems, uint64_t* vv_offs, uint64_t* vv,
                            uint64_t* cloud_offs, uint64_t* cloud, uint64_t* sizes_out, int32_t mem) {
  return ujson_wire(eng, Sel::range(slot0, nslots), cap_key_bytes, cap_el, cap_vv, cap_cloud, key_bytes,
                    key_offs, el_offs, dots, elems, vv_offs, vv, cloud_offs, cloud, sizes_out, mem);
}

// ---- the slot-list forms: record i is the state of slots[i] ----
int32_t jy_counter_state_wire_slots(jy_engine* eng, int32_t type, uint64_t n, const uint32_t* slots,
                                    int32_t slots_mem, uint64_t cap_key_bytes, uint64_t cap_cells,
                                    uint8_t* key_bytes, uint64_t* key_offs, uint64_t* cell_offs, uint8_t* sign,
                                    uint16_t* col, uint64_t* val, uint64_t* sizes_out, int32_t mem) {
  return counter_wire(eng, type, Sel::slots(n, slots, slots_mem), cap_key_bytes, cap_cells, key_bytes,
                      key_offs, cell_offs, sign, col, val, sizes_out, mem);
}
int32_t jy_treg_state_wire_slots(jy_engine* eng, uint64_t n, const uint32_t* slots, int32_t slots_mem,
                                 uint64_t cap_key_bytes, uint64_t cap_val_bytes, uint8_t* key_bytes,
                                 uint64_t* key_offs, uint64_t* ts, uint8_t* val_bytes, uint64_t* val_offs,
                                 uint64_t* sizes_out, int32_t mem) {
  return treg_wire(eng, Sel::slots(n, slots, slots_mem), cap_key_bytes, cap_val_bytes, key_bytes,
                   key_offs, ts, val_bytes, val_offs, sizes_out, mem);
}
int32_t jy_tlog_state_wire_slots(jy_engine* eng, uint64_t n, const uint32_t* slots, int32_t slots_mem,
                                 uint64_t cap_key_bytes, uint64_t cap_ent, uint64_t cap_val_bytes,
                                 uint8_t* key_bytes, uint64_t* key_offs, uint64_t* cutoff, uint64_t* ent_offs,
                                 uint64_t* ts, uint8_t* val_bytes, uint64_t* val_offs, uint64_t* sizes_out,
                                 int32_t mem) {
  return tlog_wire(eng, Sel::slots(n, slots, slots_mem), cap_key_bytes, cap_ent, cap_val_bytes,
                   key_bytes, key_offs, cutoff, ent_offs, ts, val_bytes, val_offs, sizes_out, mem);
}
int32_t jy_ujson_state_wire_slots(jy_engine* eng, uint64_t n, const uint32_t* slots, int32_t slots_mem,
                                  uint64_t cap_key_bytes, uint64_t cap_el, uint64_t cap_vv, uint64_t cap_cloud,
                                  uint8_t* key_bytes, uint64_t* key_offs, uint64_t* el_offs, uint64_t* dots,
                                  uint64_t* elems, uint64_t* vv_offs, uint64_t* vv, uint64_t* cloud_offs,
                                  uint64_t* cloud, uint64_t* sizes_out, int32_t mem) {
  return ujson_wire(eng, Sel::slots(n, slots, slots_mem), cap_key_bytes, cap_el, cap_vv, cap_cloud,
                    key_bytes, key_offs, el_offs, dots, elems, vv_offs, vv, cloud_offs, cloud, sizes_out, mem);
}

}  // extern "C"
