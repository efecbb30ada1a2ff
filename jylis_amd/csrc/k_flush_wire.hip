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
// The string gather (k_wire_gather) is balanced by OUTPUT BYTES: a lane owns
// one aligned 8-byte granule of the packed output, finds the item its first
// byte belongs to by a search in the offsets (the workgroup's slice of them
// staged in LDS), and assembles the granule from the source words of the one
// or more items that meet in it.  Stores are whole aligned words, coalesced
// over the wave; only the output's first and last granule fall back to byte
// stores.  A 2^24-byte value therefore spreads over 2^21 lanes instead of
// one, and the cost does not depend on how the bytes split into items.
// Sources are read with aligned 8-byte loads (jy_ld8u): arena values start
// on 8-byte granules, directory keys at any byte.

#include <algorithm>
#include <vector>

#include "jy_dscan.hpp"
#include "jy_internal.hpp"

namespace {

constexpr int kThreads = 256;
constexpr u64 kGranule = 8;                       // output bytes per lane
constexpr u64 kTileBytes = kThreads * kGranule;   // per workgroup
constexpr u32 kStage = 1024;                      // offsets staged in LDS per workgroup (8 KB)

__device__ __forceinline__ u64 gid() { return (u64)blockIdx.x * kThreads + threadIdx.x; }
u32 blocks_for(u64 n) { return (u32)std::max<u64>(1, (n + kThreads - 1) / kThreads); }

#define LAUNCH(k, n, ...)                                                                      \
  do {                                                                                         \
    hipLaunchKernelGGL(k, dim3(blocks_for(n)), dim3(kThreads), 0, eng->stream, __VA_ARGS__); \
    JY_HIP(eng, hipGetLastError());                                                            \
  } while (0)

// where an item's bytes are: at p, or (p == nullptr) in `inl`, byte b in bits
// [8b, 8b + 8) -- a value of up to 8 bytes lives in its handle's prefix
struct Piece {
  const uint8_t* p;
  u64 inl;
};
struct KeySrc {  // item i = the key string of slot slots[i]
  const uint8_t* bytes;
  const u64* kref;
  const u32* slots;
  __device__ __forceinline__ Piece operator()(u64 i) const {
    return Piece{bytes + (kref[slots[i]] >> JY_LR_LEN_BITS), 0};
  }
};
struct ValSrc {  // item i = the value of handle (pre[i], lr[i])
  const uint8_t* arena;
  const u64* pre;
  const u64* lr;
  __device__ __forceinline__ Piece operator()(u64 i) const {
    const u64 l = lr[i];
    if ((l & JY_LR_LEN_MASK) <= 8) return Piece{nullptr, __builtin_bswap64(pre[i])};
    return Piece{arena + (l >> JY_LR_LEN_BITS), 0};
  }
};

// the item holding output byte x < offs[n]: the largest i with offs[i] <= x
// (empty items share their successor's offset and are never the answer)
template <class At>
__device__ __forceinline__ u64 item_of(At at, u64 lo, u64 hi, u64 x) {
  while (hi - lo > 1) {
    const u64 mid = lo + (hi - lo) / 2;
    if (at(mid) <= x) lo = mid; else hi = mid;
  }
  return lo;
}

// dst[offs[i] .. offs[i + 1]) = item i's bytes, for n items, offs[n] = total > 0.
// `mis` = dst & 7: granule g is the aligned word at dst - mis + 8 g.
template <class Src>
__global__ __launch_bounds__(kThreads) void k_wire_gather(Src src, const u64* __restrict__ offs, u64 n, u64 total,
                                                          uint8_t* __restrict__ dst, u32 mis) {
  __shared__ u64 so[kStage];
  __shared__ u64 ends[2];
  const u64 g0 = (u64)blockIdx.x * kThreads;
  // the tile's output bytes [tb0, tb1) (not empty: the grid covers total + mis bytes)
  const u64 tb0 = g0 * kGranule > mis ? g0 * kGranule - mis : 0;
  const u64 tb1 = std::min<u64>((g0 + kThreads) * kGranule - mis, total);
  const auto glob = [&](u64 j) { return offs[j]; };
  if (threadIdx.x < 2) ends[threadIdx.x] = item_of(glob, 0, n, threadIdx.x == 0 ? tb0 : tb1 - 1);
  __syncthreads();
  const u64 ilo = ends[0], ihi = ends[1];
  const u64 cnt = ihi - ilo + 2;  // offsets ilo .. ihi + 1
  const bool staged = cnt <= kStage;
  if (staged)
    for (u64 q = threadIdx.x; q < cnt; q += kThreads) so[q] = offs[ilo + q];
  __syncthreads();
  const auto at = [&](u64 j) { return staged ? so[j - ilo] : offs[j]; };

  const u64 g = g0 + threadIdx.x;
  const u64 b0 = g * kGranule > mis ? g * kGranule - mis : 0;
  const u64 b1 = std::min<u64>((g + 1) * kGranule - mis, total);
  if (b0 >= b1) return;
  u64 i = item_of(at, ilo, ihi + 1, b0);
  u64 iend = at(i + 1);
  u64 w = 0;
  for (u64 pos = b0; pos < b1;) {
    while (iend <= pos) iend = at(++i + 1);  // empty items in between (offs[n] = total > pos ends it)
    const u64 take = std::min(iend, b1) - pos;
    const u64 from = pos - at(i);
    const Piece pc = src(i);
    u64 v;
    if (pc.p) {
      v = jy_ld8u(pc.p + from, take);
    } else {
      v = pc.inl >> (8 * from);
      if (take < 8) v &= (1ull << (8 * take)) - 1;
    }
    w |= v << (8 * (pos + mis - g * kGranule));
    pos += take;
  }
  uint8_t* word = dst - mis + g * kGranule;
  if (b1 - b0 == kGranule) {
    *reinterpret_cast<u64*>(word) = w;
  } else {  // the output's first / last granule
    for (u64 q = b0; q < b1; q++) dst[q] = (uint8_t)(w >> (8 * (q + mis - g * kGranule)));
  }
}

template <class Src>
int32_t gather(jy_engine* eng, Src src, const u64* offs, u64 n, u64 total, uint8_t* dst) {
  if (n == 0 || total == 0) return JY_OK;
  const u32 mis = (u32)(reinterpret_cast<uintptr_t>(dst) & (kGranule - 1));
  const u64 tiles = (total + mis + kTileBytes - 1) / kTileBytes;
  hipLaunchKernelGGL((k_wire_gather<Src>), dim3((u32)tiles), dim3(kThreads), 0, eng->stream, src, offs, n, total, dst,
                     mis);
  JY_HIP(eng, hipGetLastError());
  return JY_OK;
}

// ---- the wire form's formatting of the types' peeks ----
__global__ __launch_bounds__(kThreads) void k_wire_klen(const u64* __restrict__ kref, const u32* __restrict__ slots,
                                                        u64 k, u64* __restrict__ klen) {
  const u64 j = gid();
  if (j > k) return;
  klen[j] = j < k ? kref[slots[j]] & JY_LR_LEN_MASK : 0;
}

__global__ __launch_bounds__(kThreads) void k_wire_vlen(const u64* __restrict__ lr, u64 m, u64* __restrict__ vlen) {
  const u64 j = gid();
  if (j > m) return;
  vlen[j] = j < m ? lr[j] & JY_LR_LEN_MASK : 0;
}

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

// UJSON: non-zero entries of each pending doc's dense version vector
__global__ __launch_bounds__(kThreads) void k_wire_vv_count(const u64* __restrict__ dvv, u32 R,
                                                            const u32* __restrict__ slots, u64 k,
                                                            u64* __restrict__ nvv) {
  const u64 j = gid();
  if (j > k) return;
  u64 c = 0;
  if (j < k)
    for (u32 q = 0; q < R; q++) c += dvv[(u64)slots[j] * R + q] != 0;
  nvv[j] = c;
}
// dense [k][R] -> packed col << 48 | n, zero entries dropped, columns ascending
__global__ __launch_bounds__(kThreads) void k_wire_vv_pack(const u64* __restrict__ dense, u32 R, u64 k,
                                                           const u64* __restrict__ voff, u64* __restrict__ vv) {
  const u64 j = gid();
  if (j >= k) return;
  u64 o = voff[j];
  for (u32 q = 0; q < R; q++) {
    const u64 x = dense[j * R + q];
    if (x) vv[o++] = ((u64)q << JY_DOT_SEQ_BITS) | x;
  }
}
// ---- host side ----
// temporaries of one call, from the engine's stream-ordered pool (freed in
// stream order: the kernels queued before the free still see them)
struct Tmp {
  jy_engine* eng;
  std::vector<void*> held;
  explicit Tmp(jy_engine* e) : eng(e) {}
  ~Tmp() {
    for (void* p : held) jy_dev_free(eng, p);
  }
  template <class T>
  int32_t get(T** out, u64 count) {
    void* p = nullptr;
    JY_TRY(jy_dev_alloc(eng, &p, count * sizeof(T) + 16, "wire flush temporary"));
    held.push_back(p);
    *out = static_cast<T*>(p);
    return JY_OK;
  }
  // where a kernel writes an output array of the caller's: the array itself
  // (device memory), or a temporary for emit (host memory)
  template <class T>
  int32_t out(T** dev, T* user, u64 count, int32_t mem) {
    if (mem == JY_HOST) return get(dev, count);
    *dev = user;
    return JY_OK;
  }
};

// up to four device words -> the host (one wait)
int32_t totals(jy_engine* eng, std::initializer_list<const u64*> words, u64* out) {
  int q = 0;
  for (const u64* w : words)
    JY_HIP(eng, hipMemcpyAsync(eng->pin_total + q++, w, 8, hipMemcpyDeviceToHost, eng->stream));
  JY_HIP(eng, hipStreamSynchronize(eng->stream));
  for (int i = 0; i < q; i++) out[i] = eng->pin_total[i];
  return JY_OK;
}

// a finished temporary -> the caller's array (device: in stream order);
// nothing to do for an array written in place (Tmp::out)
int32_t emit(jy_engine* eng, int32_t mem, void* dst, const void* src, u64 bytes) {
  if (bytes == 0 || dst == src) return JY_OK;
  if (mem != JY_HOST) {
    JY_HIP(eng, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, eng->stream));
  } else if (bytes >= (1ull << 20)) {
    JY_TRY(jy_readback(eng, dst, src, bytes));  // pinned landing area + parallel host copy
  } else {
    JY_HIP(eng, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, eng->stream));
  }
  return JY_OK;
}

int32_t mem_check(jy_engine* eng, int32_t mem) {
  if (mem != JY_HOST && mem != JY_DEVICE) return eng->fail(JY_EINVAL, "mem must be JY_HOST or JY_DEVICE");
  return JY_OK;
}

// nothing pending: the batch is empty, so every offsets array the caller
// passed holds its one element, 0 (written on the engine stream for JY_DEVICE)
int32_t empty_batch(jy_engine* eng, int32_t mem, std::initializer_list<u64*> offs) {
  for (u64* o : offs) {
    if (!o) continue;
    if (mem == JY_DEVICE) JY_HIP(eng, hipMemsetAsync(o, 0, 8, eng->stream));
    else *o = 0;
  }
  return JY_OK;
}

// the k pending slots of a set (a temporary), and for the wire form their
// key lengths / offsets
int32_t pending_slots(jy_engine* eng, Tmp& tmp, int32_t type, const PendingSet& P, u64 k, u32** slots) {
  JY_TRY(tmp.get(slots, k));
  return jy_pending_slots(eng, type, P, k, *slots);
}
struct Keys {
  u32* slots = nullptr;
  u64* klen = nullptr;
  u64* koff = nullptr;
};
int32_t pending_keys(jy_engine* eng, Tmp& tmp, int32_t type, const PendingSet& P, u64 k, Keys& K) {
  JY_TRY(pending_slots(eng, tmp, type, P, k, &K.slots));
  JY_TRY(tmp.get(&K.klen, k + 1));
  JY_TRY(tmp.get(&K.koff, k + 1));
  LAUNCH(k_wire_klen, k + 1, eng->kdir[type].kref, K.slots, k, K.klen);
  return jy_scan_u64(eng, K.klen, K.koff, k);
}

// key strings -> key_bytes
int32_t emit_keys(jy_engine* eng, Tmp& tmp, int32_t type, const Keys& K, u64 k, u64 kbytes, uint8_t* key_bytes,
                  u64* key_offs, int32_t mem) {
  uint8_t* kb;
  JY_TRY(tmp.out(&kb, key_bytes, kbytes, mem));
  const KeyDir& D = eng->kdir[type];
  JY_TRY(gather(eng, KeySrc{D.bytes, D.kref, K.slots}, K.koff, k, kbytes, kb));
  JY_TRY(emit(eng, mem, key_bytes, kb, kbytes));
  return emit(eng, mem, key_offs, K.koff, (k + 1) * 8);
}

// the value bytes of m handles: their offsets (voff[m] = the total, read by the caller) ...
int32_t value_offsets(jy_engine* eng, Tmp& tmp, const u64* lr, u64 m, u64** voff) {
  u64* vlen;
  JY_TRY(tmp.get(&vlen, m + 1));
  JY_TRY(tmp.get(voff, m + 1));
  LAUNCH(k_wire_vlen, m + 1, lr, m, vlen);
  return jy_scan_u64(eng, vlen, *voff, m);
}
// ... and the bytes -> val_bytes
int32_t emit_values(jy_engine* eng, Tmp& tmp, int32_t type, const u64* pre, const u64* lr, const u64* voff, u64 m,
                    u64 vbytes, uint8_t* val_bytes, u64* val_offs, int32_t mem) {
  uint8_t* vb;
  JY_TRY(tmp.out(&vb, val_bytes, vbytes, mem));
  JY_TRY(gather(eng, ValSrc{eng->arena[type].p, pre, lr}, voff, m, vbytes, vb));
  JY_TRY(emit(eng, mem, val_bytes, vb, vbytes));
  return emit(eng, mem, val_offs, voff, (m + 1) * 8);
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

