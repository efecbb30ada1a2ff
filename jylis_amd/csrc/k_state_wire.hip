// k_state_wire.hip -- the STATE of a slot range as a ready-to-converge batch
// (jy_*_state_wire): record i is the state of slot slot0 + i, as exactly the
// arrays the same type's jy_node_*_converge and jy_*_flush_wire use.  What a
// host needs to bring a late peer up to date (anti-entropy), to persist a
// store (repo_manager.pony:100,107 "TODO: disk persistence?") and to reshard.
//
// Every call is: check the selection (Sel: a range, or a slot list checked on
// the device), turn it into a device slot array with its key offsets
// (sel_keys), and hand that to the type's wire formatter over the STATE store
// (jy_wire.hpp) -- the formatter the wire-form flushes run over the pending
// store, so the sizes-only return, the order of the arrays and what an empty
// batch zeroes are written once.  What belongs to the state stays here or in
// the state's readers: tlog_state settles before it reads, jy_treg_gather
// folds pending duplicates, and the TREG formatter checks the duplicate-list
// overflow after its read-back when it reads the state.  Nothing is written
// to the engine's state, pending sets, arenas or key directory.
//
// Counters have no reader that yields cells; their cell producer is the one
// hot kernel of this file (counter_state picks the instantiation, the shared
// counter_format sizes, emits and orders the arrays):
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

// JY_STATE_CELLS=lane in the environment: the lane-per-slot writer at every
// width (the A/B of tools/state_wire_time.py); read at each call
bool force_lane_writer() {
  const char* v = std::getenv("JY_STATE_CELLS");
  return v && std::strcmp(v, "lane") == 0;
}


int32_t counter_state(jy_engine* eng, int32_t type, const Sel& sel, uint64_t cap_key_bytes, uint64_t cap_cells,
                      const CounterWire& o, uint64_t* sizes_out, int32_t mem) {
  JY_HIP(eng, hipSetDevice(eng->device));
  if (type != JY_GCOUNT && type != JY_PNCOUNT) return eng->fail(JY_ETYPE, "not a counter type");
  JY_TRY(mem_check(eng, mem));
  sizes_out[0] = sizes_out[1] = sizes_out[2] = 0;
  JY_TRY(sel_check(eng, type, sel));
  const u64 n = sel.n;
  if (n == 0) return empty_batch(eng, mem, {o.key_offs, o.cell_offs});
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
  // the kernels' instantiations: with or without masks, over the range or the list
  const auto count = list ? (masked ? k_state_cnt_count<true, true> : k_state_cnt_count<false, true>)
                          : (masked ? k_state_cnt_count<true, false> : k_state_cnt_count<false, false>);
  const auto lane = list ? (masked ? k_state_cnt_lane<true, true> : k_state_cnt_lane<false, true>)
                         : (masked ? k_state_cnt_lane<true, false> : k_state_cnt_lane<false, false>);
  const auto tile = list ? k_state_cnt_tile<true> : k_state_cnt_tile<false>;
  LAUNCH(count, n + 1, S, slot0, list, n, ncell, mask);
  JY_TRY(jy_scan_u64(eng, ncell, coff, n));
  bool written;
  JY_TRY(counter_format(eng, tmp, type, K, n, coff, {kNoCap, cap_key_bytes, cap_cells}, o, sizes_out, mem, &written,
                        [&](u64 ncells, uint8_t* ds, u16* dc, u64* dv) -> int32_t {
                          if (ncells == 0) return JY_OK;
                          if (!masked || force_lane_writer()) {
                            LAUNCH(lane, n, S, slot0, list, n, coff, mask, ds, dc, dv);
                          } else {
                            const u64 tiles = (n + kTileSlots - 1) / kTileSlots;
                            hipLaunchKernelGGL(tile, dim3((u32)tiles), dim3(kThreads), 0, eng->stream, S, slot0, list,
                                               n, coff, mask, ds, dc, dv);
                            JY_HIP(eng, hipGetLastError());
                          }
                          return JY_OK;
                        }));
  return written ? host_sync(eng, mem) : JY_OK;
}

int32_t treg_state(jy_engine* eng, const Sel& sel, uint64_t cap_key_bytes, uint64_t cap_val_bytes, const TregWire& o,
                   uint64_t* sizes_out, int32_t mem) {
  JY_HIP(eng, hipSetDevice(eng->device));
  JY_TRY(mem_check(eng, mem));
  sizes_out[0] = sizes_out[1] = sizes_out[2] = 0;
  JY_TRY(sel_check(eng, JY_TREG, sel));
  if (sel.n == 0) return empty_batch(eng, mem, {o.key_offs, o.val_offs});
  Tmp tmp(eng);
  Keys K;
  bool written;
  JY_TRY(sel_keys(eng, tmp, JY_TREG, sel, K));
  JY_TRY(treg_format(eng, tmp, K, sel.n, false, {kNoCap, cap_key_bytes, cap_val_bytes}, o, sizes_out, mem, &written));
  return written ? host_sync(eng, mem) : JY_OK;
}

int32_t tlog_state(jy_engine* eng, const Sel& sel, uint64_t cap_key_bytes, uint64_t cap_ent, uint64_t cap_val_bytes,
                   const TlogWire& o, uint64_t* sizes_out, int32_t mem) {
  JY_HIP(eng, hipSetDevice(eng->device));
  JY_TRY(mem_check(eng, mem));
  for (int q = 0; q < 4; q++) sizes_out[q] = 0;
  JY_TRY(sel_check(eng, JY_TLOG, sel));
  if (sel.n == 0) return empty_batch(eng, mem, {o.key_offs, o.ent_offs, o.val_offs});
  JY_TRY(jy_tlog_settle(eng));
  Tmp tmp(eng);
  Keys K;
  bool written;
  JY_TRY(sel_keys(eng, tmp, JY_TLOG, sel, K));
  JY_TRY(tlog_format(eng, tmp, K, sel.n, eng->tlog, {kNoCap, cap_key_bytes, cap_ent, cap_val_bytes}, o, sizes_out,
                     mem, &written));
  return written ? host_sync(eng, mem) : JY_OK;
}

int32_t ujson_state(jy_engine* eng, const Sel& sel, uint64_t cap_key_bytes, uint64_t cap_el, uint64_t cap_vv,
                    uint64_t cap_cloud, const UjsonWire& o, uint64_t* sizes_out, int32_t mem) {
  JY_HIP(eng, hipSetDevice(eng->device));
  JY_TRY(mem_check(eng, mem));
  for (int q = 0; q < 5; q++) sizes_out[q] = 0;
  JY_TRY(sel_check(eng, JY_UJSON, sel));
  if (sel.n == 0) return empty_batch(eng, mem, {o.key_offs, o.el_offs, o.vv_offs, o.cloud_offs});
  Tmp tmp(eng);
  Keys K;
  bool written;
  JY_TRY(sel_keys(eng, tmp, JY_UJSON, sel, K));
  JY_TRY(ujson_format(eng, tmp, K, sel.n, eng->ujson, {kNoCap, cap_key_bytes, cap_el, cap_vv, cap_cloud}, o,
                      sizes_out, mem, &written));
  return written ? host_sync(eng, mem) : JY_OK;
}

}  // namespace

extern "C" {

uint32_t jy_counter_state_mask_rows(void) { return kMaskRows; }

int32_t jy_counter_state_wire(jy_engine* eng, int32_t type, uint64_t slot0, uint64_t nslots, uint64_t cap_key_bytes,
                              uint64_t cap_cells, uint8_t* key_bytes, uint64_t* key_offs, uint64_t* cell_offs,
                              uint8_t* sign, uint16_t* col, uint64_t* val, uint64_t* sizes_out, int32_t mem) {
  return counter_state(eng, type, Sel::range(slot0, nslots), cap_key_bytes, cap_cells,
                       CounterWire{key_bytes, key_offs, cell_offs, sign, col, val}, sizes_out, mem);
}
int32_t jy_treg_state_wire(jy_engine* eng, uint64_t slot0, uint64_t nslots, uint64_t cap_key_bytes,
                           uint64_t cap_val_bytes, uint8_t* key_bytes, uint64_t* key_offs, uint64_t* ts,
                           uint8_t* val_bytes, uint64_t* val_offs, uint64_t* sizes_out, int32_t mem) {
  return treg_state(eng, Sel::range(slot0, nslots), cap_key_bytes, cap_val_bytes,
                    TregWire{key_bytes, key_offs, ts, val_bytes, val_offs}, sizes_out, mem);
}
int32_t jy_tlog_state_wire(jy_engine* eng, uint64_t slot0, uint64_t nslots, uint64_t cap_key_bytes, uint64_t cap_ent,
                           uint64_t cap_val_bytes, uint8_t* key_bytes, uint64_t* key_offs, uint64_t* cutoff,
                           uint64_t* ent_offs, uint64_t* ts, uint8_t* val_bytes, uint64_t* val_offs,
                           uint64_t* sizes_out, int32_t mem) {
  return tlog_state(eng, Sel::range(slot0, nslots), cap_key_bytes, cap_ent, cap_val_bytes,
                    TlogWire{key_bytes, key_offs, cutoff, ent_offs, ts, val_bytes, val_offs}, sizes_out, mem);
}
int32_t jy_ujson_state_wire(jy_engine* eng, uint64_t slot0, uint64_t nslots, uint64_t cap_key_bytes, uint64_t cap_el,
                            uint64_t cap_vv, uint64_t cap_cloud, uint8_t* key_bytes, uint64_t* key_offs,
                            uint64_t* el_offs, uint64_t* dots, uint64_t* elems, uint64_t* vv_offs, uint64_t* vv,
                            uint64_t* cloud_offs, uint64_t* cloud, uint64_t* sizes_out, int32_t mem) {
  return ujson_state(eng, Sel::range(slot0, nslots), cap_key_bytes, cap_el, cap_vv, cap_cloud,
                     UjsonWire{key_bytes, key_offs, el_offs, dots, elems, vv_offs, vv, cloud_offs, cloud}, sizes_out,
                     mem);
}

// ---- the slot-list forms: record i is the state of slots[i] ----
int32_t jy_counter_state_wire_slots(jy_engine* eng, int32_t type, uint64_t n, const uint32_t* slots,
                                    int32_t slots_mem, uint64_t cap_key_bytes, uint64_t cap_cells,
                                    uint8_t* key_bytes, uint64_t* key_offs, uint64_t* cell_offs, uint8_t* sign,
                                    uint16_t* col, uint64_t* val, uint64_t* sizes_out, int32_t mem) {
  return counter_state(eng, type, Sel::slots(n, slots, slots_mem), cap_key_bytes, cap_cells,
                       CounterWire{key_bytes, key_offs, cell_offs, sign, col, val}, sizes_out, mem);
}
int32_t jy_treg_state_wire_slots(jy_engine* eng, uint64_t n, const uint32_t* slots, int32_t slots_mem,
                                 uint64_t cap_key_bytes, uint64_t cap_val_bytes, uint8_t* key_bytes,
                                 uint64_t* key_offs, uint64_t* ts, uint8_t* val_bytes, uint64_t* val_offs,
                                 uint64_t* sizes_out, int32_t mem) {
  return treg_state(eng, Sel::slots(n, slots, slots_mem), cap_key_bytes, cap_val_bytes,
                    TregWire{key_bytes, key_offs, ts, val_bytes, val_offs}, sizes_out, mem);
}
int32_t jy_tlog_state_wire_slots(jy_engine* eng, uint64_t n, const uint32_t* slots, int32_t slots_mem,
                                 uint64_t cap_key_bytes, uint64_t cap_ent, uint64_t cap_val_bytes,
                                 uint8_t* key_bytes, uint64_t* key_offs, uint64_t* cutoff, uint64_t* ent_offs,
                                 uint64_t* ts, uint8_t* val_bytes, uint64_t* val_offs, uint64_t* sizes_out,
                                 int32_t mem) {
  return tlog_state(eng, Sel::slots(n, slots, slots_mem), cap_key_bytes, cap_ent, cap_val_bytes,
                    TlogWire{key_bytes, key_offs, cutoff, ent_offs, ts, val_bytes, val_offs}, sizes_out, mem);
}
int32_t jy_ujson_state_wire_slots(jy_engine* eng, uint64_t n, const uint32_t* slots, int32_t slots_mem,
                                  uint64_t cap_key_bytes, uint64_t cap_el, uint64_t cap_vv, uint64_t cap_cloud,
                                  uint8_t* key_bytes, uint64_t* key_offs, uint64_t* el_offs, uint64_t* dots,
                                  uint64_t* elems, uint64_t* vv_offs, uint64_t* vv, uint64_t* cloud_offs,
                                  uint64_t* cloud, uint64_t* sizes_out, int32_t mem) {
  return ujson_state(eng, Sel::slots(n, slots, slots_mem), cap_key_bytes, cap_el, cap_vv, cap_cloud,
                     UjsonWire{key_bytes, key_offs, el_offs, dots, elems, vv_offs, vv, cloud_offs, cloud}, sizes_out,
                     mem);
}

}  // extern "C"
