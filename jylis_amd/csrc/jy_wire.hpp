// jy_wire.hpp -- the core every wire-form call shares.  Engine contents become
// the arrays jy_node_*_converge takes in three layers, each written once:
//
//   slot selection   Sel / sel_check / sel_slots / sel_keys: a range or a
//                    checked slot list as a device slot array (a flush selects
//                    its pending set instead: jy_pending_slots)
//   record readers   treg_records, tlog_sizing + tlog_entries, ujson_sizing +
//                    ujson_entries: the records of a slot array read from a
//                    STORE -- the state, or the pending deltas
//   wire formatters  treg_format, tlog_format, ujson_format, counter_format:
//                    a reader's records plus key strings and value bytes as the
//                    wire arrays; sizes first, "sizes only" when a capacity is
//                    short, the order of the emits
//
// Who calls what:
//   jy_*_flush_wire         (k_flush_wire.hip)   pending slots -> formatter over the pending store -> clear
//   jy_*_state_wire[_slots] (k_state_wire.hip)   sel_keys -> formatter over the state
//   jy_*_flush, slot form   (k_flush_wire.hip)   pending slots -> reader over the pending store -> clear
//   jy_*_state_digest       (k_state_digest.hip) sel_slots -> reader over the state -> digest kernels
// Below them: the byte-balanced string gather and the host-side helpers of one
// call (temporaries, totals, emit).
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
#pragma once

#include <algorithm>
#include <initializer_list>
#include <type_traits>
#include <vector>

#include "jy_internal.hpp"

namespace {

constexpr int kThreads = 256;
constexpr u64 kGranule = 8;                       // output bytes per lane
constexpr u64 kTileBytes = kThreads * kGranule;   // per workgroup
constexpr u32 kStage = 1024;                      // offsets staged in LDS per workgroup (8 KB)

__device__ __forceinline__ u64 gid() { return (u64)blockIdx.x * kThreads + threadIdx.x; }
inline u32 blocks_for(u64 n) { return (u32)std::max<u64>(1, (n + kThreads - 1) / kThreads); }

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
struct LeafSrc {  // item i = the stored leaf lr[i] names (k_leaf.hip); an lr of 0 is an empty item, never asked for
  const uint8_t* arena;
  const u64* lr;
  __device__ __forceinline__ Piece operator()(u64 i) const { return Piece{arena + (lr[i] >> JY_LR_LEN_BITS), 0}; }
};
struct LeafTailSrc {  // item i = the stored leaf lr[i] from its byte skip[i] on: a leaf relative to a path (k_uj_path.hip)
  const uint8_t* arena;
  const u64* lr;
  const u32* skip;  // < the leaf's length; the tail starts at any byte (jy_ld8u)
  __device__ __forceinline__ Piece operator()(u64 i) const {
    return Piece{arena + (lr[i] >> JY_LR_LEN_BITS) + skip[i], 0};
  }
};
struct ReqSrc {  // item i = the bytes of a request buffer from off[i] on: a decoded command's key or value (k_resp_in.hip)
  const uint8_t* req;
  const u64* off;  // the range starts at any byte (jy_ld8u)
  __device__ __forceinline__ Piece operator()(u64 i) const { return Piece{req + off[i], 0}; }
};

// A source may instead GENERATE its items: it has gen(i, from, take), the
// `take` <= 8 bytes of item i from its byte `from` on as a little-endian word,
// zero above them (RespSrc, k_resp.hip: decimal numbers and framing beside
// pointer and inline values).  The gather asks it for exactly the bytes of the
// granule it is assembling.
template <class Src, class = void>
struct src_generates : std::false_type {};
template <class Src>
struct src_generates<Src, std::void_t<decltype(&Src::gen)>> : std::true_type {};

template <class Src>
__device__ __forceinline__ u64 item_bytes(const Src& src, u64 i, u64 from, u64 take) {
  if constexpr (src_generates<Src>::value) {
    return src.gen(i, from, take);
  } else {
    const Piece pc = src(i);
    if (pc.p) return jy_ld8u(pc.p + from, take);
    u64 v = pc.inl >> (8 * from);
    if (take < 8) v &= (1ull << (8 * take)) - 1;
    return v;
  }
}

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
    const u64 v = item_bytes(src, i, from, take);
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

// ---- the wire form's formatting kernels both callers use ----
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

// the slot list of a range: slots[j] = slot0 + j
[[maybe_unused]] __global__ __launch_bounds__(kThreads) void k_wire_iota(u32 slot0, u64 n, u32* __restrict__ slots) {
  const u64 j = gid();
  if (j < n) slots[j] = slot0 + (u32)j;
}

// UJSON: non-zero entries of each doc's dense version vector
[[maybe_unused]] __global__ __launch_bounds__(kThreads) void k_wire_vv_count(const u64* __restrict__ dvv, u32 R,
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
[[maybe_unused]] __global__ __launch_bounds__(kThreads) void k_wire_vv_pack(const u64* __restrict__ dense, u32 R, u64 k,
                                                           const u64* __restrict__ voff, u64* __restrict__ vv) {
  const u64 j = gid();
  if (j >= k) return;
  u64 o = voff[j];
  for (u32 q = 0; q < R; q++) {
    const u64 x = dense[j * R + q];
    if (x) vv[o++] = ((u64)q << JY_DOT_SEQ_BITS) | x;
  }
}

// a counter slab [sign][col][kcap] as the state readers walk it (k_state_wire.hip,
// k_state_digest.hip): row r = sign * ncols + col, a row's slots contiguous
struct Slab {
  const u64* p;    // the slab's first cell
  u64 pitch;       // cells per column row (kcap)
  u64 sign_pitch;  // cells per sign (ccap * kcap)
  u32 ncols;       // columns read: registered and allocated
  u32 rows;        // nsigns * ncols
  __device__ __forceinline__ const u64* row(u32 r) const {
    const u32 sg = r >= ncols ? 1u : 0u;  // nsigns <= 2
    return p + sg * sign_pitch + (u64)(r - sg * ncols) * pitch;
  }
};

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
    JY_TRY(jy_dev_alloc(eng, &p, count * sizeof(T) + 16, "wire temporary"));
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
inline int32_t totals(jy_engine* eng, std::initializer_list<const u64*> words, u64* out) {
  int q = 0;
  for (const u64* w : words)
    JY_HIP(eng, hipMemcpyAsync(eng->pin_total + q++, w, 8, hipMemcpyDeviceToHost, eng->stream));
  JY_HIP(eng, hipStreamSynchronize(eng->stream));
  for (int i = 0; i < q; i++) out[i] = eng->pin_total[i];
  return JY_OK;
}

// a finished temporary -> the caller's array (device: in stream order);
// nothing to do for an array written in place (Tmp::out)
inline int32_t emit(jy_engine* eng, int32_t mem, void* dst, const void* src, u64 bytes) {
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

inline int32_t mem_check(jy_engine* eng, int32_t mem) {
  if (mem != JY_HOST && mem != JY_DEVICE) return eng->fail(JY_EINVAL, "mem must be JY_HOST or JY_DEVICE");
  return JY_OK;
}

// a JY_HOST call ends with its outputs complete; a JY_DEVICE call without a wait
inline int32_t host_sync(jy_engine* eng, int32_t mem) {
  if (mem == JY_HOST) JY_HIP(eng, hipStreamSynchronize(eng->stream));
  return JY_OK;
}

// an empty batch: every offsets array the caller passed holds its one
// element, 0 (written on the engine stream for JY_DEVICE)
inline int32_t empty_batch(jy_engine* eng, int32_t mem, std::initializer_list<u64*> offs) {
  for (u64* o : offs) {
    if (!o) continue;
    if (mem == JY_DEVICE) JY_HIP(eng, hipMemsetAsync(o, 0, 8, eng->stream));
    else *o = 0;
  }
  return JY_OK;
}

// the key strings of k slots (a device array): their lengths / offsets
// (koff[k] = the total, read by the caller) ...
struct Keys {
  u32* slots = nullptr;
  u64* klen = nullptr;
  u64* koff = nullptr;
};
inline int32_t key_offsets(jy_engine* eng, Tmp& tmp, int32_t type, u64 k, Keys& K) {
  JY_TRY(tmp.get(&K.klen, k + 1));
  JY_TRY(tmp.get(&K.koff, k + 1));
  LAUNCH(k_wire_klen, k + 1, eng->kdir[type].kref, K.slots, k, K.klen);
  return jy_scan_u64(eng, K.klen, K.koff, k);
}

// ... and the strings -> key_bytes
inline int32_t emit_keys(jy_engine* eng, Tmp& tmp, int32_t type, const Keys& K, u64 k, u64 kbytes,
                         uint8_t* key_bytes, u64* key_offs, int32_t mem) {
  uint8_t* kb;
  JY_TRY(tmp.out(&kb, key_bytes, kbytes, mem));
  const KeyDir& D = eng->kdir[type];
  JY_TRY(gather(eng, KeySrc{D.bytes, D.kref, K.slots}, K.koff, k, kbytes, kb));
  JY_TRY(emit(eng, mem, key_bytes, kb, kbytes));
  return emit(eng, mem, key_offs, K.koff, (k + 1) * 8);
}

// the value bytes of m handles: their offsets (voff[m] = the total, read by the caller) ...
inline int32_t value_offsets(jy_engine* eng, Tmp& tmp, const u64* lr, u64 m, u64** voff) {
  u64* vlen;
  JY_TRY(tmp.get(&vlen, m + 1));
  JY_TRY(tmp.get(voff, m + 1));
  LAUNCH(k_wire_vlen, m + 1, lr, m, vlen);
  return jy_scan_u64(eng, vlen, *voff, m);
}
// ... and the bytes -> val_bytes
inline int32_t emit_values(jy_engine* eng, Tmp& tmp, int32_t type, const u64* pre, const u64* lr, const u64* voff,
                           u64 m, u64 vbytes, uint8_t* val_bytes, u64* val_offs, int32_t mem) {
  uint8_t* vb;
  JY_TRY(tmp.out(&vb, val_bytes, vbytes, mem));
  JY_TRY(gather(eng, ValSrc{eng->arena[type].p, pre, lr}, voff, m, vbytes, vb));
  JY_TRY(emit(eng, mem, val_bytes, vb, vbytes));
  return emit(eng, mem, val_offs, voff, (m + 1) * 8);
}

// ---- slot selection: which slots a call reads ----
// [slot0, slot0 + nslots) must lie inside the type's interned keys
inline int32_t range_check(jy_engine* eng, int32_t type, u64 slot0, u64 nslots) {
  const u64 nk = eng->nkeys[type];
  if (slot0 > nk || nslots > nk - slot0) return eng->fail(JY_ERANGE, "slot range reaches past the interned keys");
  return JY_OK;
}

// err |= 1: list[j] <= list[j - 1] (not strictly ascending), |= 2: list[j] >= nk
[[maybe_unused]] __global__ __launch_bounds__(kThreads) void k_wire_list_check(const u32* __restrict__ list, u64 n,
                                                                               u64 nk, u32* __restrict__ err) {
  const u64 j = gid();
  if (j >= n) return;
  const u32 s = list[j];
  const u32 e = (j > 0 && s <= list[j - 1] ? 1u : 0u) | (s >= nk ? 2u : 0u);
  if (e) atomicOr(err, e);
}

// the slots of one state read: the range [slot0, slot0 + n), or the n slots of
// `list`.  (A flush's selection is its pending set: jy_pending_slots.)
struct Sel {
  bool is_list;
  u64 slot0, n;
  const u32* list;  // is_list: the n slots (may be null only when n == 0)
  int32_t list_mem;
  static Sel range(u64 slot0, u64 n) { return Sel{false, slot0, n, nullptr, JY_HOST}; }
  static Sel slots(u64 n, const u32* list, int32_t mem) { return Sel{true, 0, n, list, mem}; }
};
inline int32_t sel_check(jy_engine* eng, int32_t type, const Sel& sel) {
  if (!sel.is_list) return range_check(eng, type, sel.slot0, sel.n);
  if (sel.list_mem != JY_HOST && sel.list_mem != JY_DEVICE)
    return eng->fail(JY_EINVAL, "slots_mem must be JY_HOST or JY_DEVICE");
  if (sel.n > 0 && !sel.list) return eng->fail(JY_EINVAL, "slot list is null");
  return JY_OK;
}
// the selection (n > 0, checked by sel_check) as a device slot array, so every
// reader that takes one is reused unchanged.  A range is slot0 + j.  A list is
// copied and checked ON THE DEVICE to be strictly ascending and inside the
// interned keys before any reader indexes state with it; the error word is
// read back here, so a list call waits for the stream once more than a range
// call.
inline int32_t sel_slots(jy_engine* eng, Tmp& tmp, int32_t type, const Sel& sel, u32** slots) {
  const u64 n = sel.n;
  JY_TRY(tmp.get(slots, n));
  if (!sel.is_list) {
    LAUNCH(k_wire_iota, n, (u32)sel.slot0, n, *slots);
    return JY_OK;
  }
  u32* err;
  JY_TRY(tmp.get(&err, 2));
  JY_HIP(eng, hipMemsetAsync(err, 0, 8, eng->stream));
  JY_HIP(eng, hipMemcpyAsync(*slots, sel.list, n * 4,
                             sel.list_mem == JY_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, eng->stream));
  LAUNCH(k_wire_list_check, n, *slots, n, eng->nkeys[type], err);
  u64 e = 0;
  JY_TRY(totals(eng, {reinterpret_cast<const u64*>(err)}, &e));
  if (e & 2) return eng->fail(JY_ERANGE, "slot list names a slot past the interned keys");
  if (e & 1) return eng->fail(JY_EINVAL, "slot list is not strictly ascending");
  return JY_OK;
}
// ... with its key lengths / offsets
inline int32_t sel_keys(jy_engine* eng, Tmp& tmp, int32_t type, const Sel& sel, Keys& K) {
  JY_TRY(sel_slots(eng, tmp, type, sel, &K.slots));
  return key_offsets(eng, tmp, type, sel.n, K);
}

// ---- records on the device: one reader per type, over either store ----
// A reader takes a device slot array and the store to read: the state, or the
// pending deltas of the write path (read, never cleared).  TLOG and UJSON split
// into a sizing half (per-key offsets, their totals still on the device) and an
// entry half, between which the caller reads the totals back (one wait, shared
// with whatever else it needs) and sets the struct's counts.  An entry half
// writes to the caller's own device arrays where it is given them (mem ==
// JY_DEVICE, as Tmp::out), else to temporaries.  What belongs to the STATE
// store stays with the state's entry points: jy_tlog_settle before a TLOG read
// (the TLOG flushes settle too), the fold inside jy_treg_gather, and
// jy_treg_overflow_check after the read-back.

struct TregRecs {
  u64 *ts = nullptr, *pre = nullptr, *lr = nullptr;  // per key
};
// pending: the delta registers (dts, dval); else the state's, duplicates folded first
inline int32_t treg_records(jy_engine* eng, Tmp& tmp, bool pending, const u32* slots, u64 n, TregRecs& R,
                            int32_t mem = JY_HOST, u64* ts = nullptr, u64* pre = nullptr, u64* lr = nullptr) {
  JY_TRY(tmp.out(&R.ts, ts, n, mem));
  JY_TRY(tmp.out(&R.pre, pre, n, mem));
  JY_TRY(tmp.out(&R.lr, lr, n, mem));
  const TregState& t = eng->treg;
  if (pending) return jy_treg_gather_of(eng, t.dts, t.dval, n, slots, R.ts, R.pre, R.lr);
  return jy_treg_gather(eng, n, slots, R.ts, R.pre, R.lr);
}

struct TlogRecs {
  u64 *cuts = nullptr, *eoff = nullptr;              // per key; eoff[n] = all entries
  u64 m = 0;                                         // eoff[n] on the host: set by the caller
  u64 *ts = nullptr, *pre = nullptr, *lr = nullptr;  // per entry, newest first per key
};
inline int32_t tlog_sizing(jy_engine* eng, Tmp& tmp, const TlogState& t, const u32* slots, u64 n, TlogRecs& R) {
  u64* lens;
  JY_TRY(tmp.get(&lens, n + 1));
  JY_TRY(tmp.get(&R.cuts, n));
  JY_TRY(tmp.get(&R.eoff, n + 1));
  JY_HIP(eng, hipMemsetAsync(lens + n, 0, 8, eng->stream));
  JY_TRY(jy_tlog_sizes_of(eng, t, n, slots, lens, R.cuts));
  return jy_scan_u64(eng, lens, R.eoff, n);
}
inline int32_t tlog_entries(jy_engine* eng, Tmp& tmp, const TlogState& t, const u32* slots, u64 n, TlogRecs& R,
                            int32_t mem = JY_HOST, u64* ts = nullptr, u64* pre = nullptr, u64* lr = nullptr) {
  JY_TRY(tmp.out(&R.ts, ts, R.m, mem));
  JY_TRY(tmp.out(&R.pre, pre, R.m, mem));
  JY_TRY(tmp.out(&R.lr, lr, R.m, mem));
  if (R.m) JY_TRY(jy_tlog_gather_of(eng, t, n, slots, R.eoff, R.ts, R.pre, R.lr));
  return JY_OK;
}

struct UjsonRecs {
  u64 *eo = nullptr, *co = nullptr;  // per doc: element and cloud offsets (eo[n], co[n] = the totals)
  u64 me = 0, mc = 0;                // the totals on the host: set by the caller
  // elements and cloud in converge order (dots ascending per doc, for documents
  // in the per-column layout too), and the dense version vectors [n][R]
  u64 *dots = nullptr, *elems = nullptr, *dense = nullptr, *cloud = nullptr;
};
inline int32_t ujson_sizing(jy_engine* eng, Tmp& tmp, const UjsonState& u, const u32* slots, u64 n, UjsonRecs& D) {
  u64 *se, *sc;
  JY_TRY(tmp.get(&se, n + 1));
  JY_TRY(tmp.get(&sc, n + 1));
  JY_TRY(tmp.get(&D.eo, n + 1));
  JY_TRY(tmp.get(&D.co, n + 1));
  JY_HIP(eng, hipMemsetAsync(se + n, 0, 8, eng->stream));
  JY_HIP(eng, hipMemsetAsync(sc + n, 0, 8, eng->stream));
  JY_TRY(jy_ujson_sizes_of(eng, u, n, slots, se, sc));
  JY_TRY(jy_scan_u64(eng, se, D.eo, n));
  return jy_scan_u64(eng, sc, D.co, n);
}
// (a null `dense` with the others given: the dense vectors alone go to a temporary)
inline int32_t ujson_entries(jy_engine* eng, Tmp& tmp, const UjsonState& u, const u32* slots, u64 n, UjsonRecs& D,
                             int32_t mem = JY_HOST, u64* dots = nullptr, u64* elems = nullptr, u64* dense = nullptr,
                             u64* cloud = nullptr) {
  JY_TRY(tmp.out(&D.dots, dots, D.me, mem));
  JY_TRY(tmp.out(&D.elems, elems, D.me, mem));
  JY_TRY(tmp.out(&D.dense, dense, n * u.R, dense ? mem : JY_HOST));
  JY_TRY(tmp.out(&D.cloud, cloud, D.mc, mem));
  return jy_ujson_gather_of(eng, u, n, slots, D.eo, D.co, D.me, D.mc, D.dots, D.elems, D.dense, D.cloud);
}

// ---- one wire formatter per type ----
// The records of K's n > 0 slots (K from sel_keys or a pending set, ascending)
// read from `store`, as the arrays jy_node_*_converge takes: sizes_out = what
// the batch needs, in the order of `caps`.  The arrays `o` are written, and
// *written set, only when no capacity is short (else JY_OK: sizes only, nothing
// written).  caps[0] bounds the per-key arrays: kNoCap from the snapshots, whose
// per-key arrays hold n by contract.  The caller ends the call: a flush's
// clear, the stream wait of a JY_HOST call.
constexpr u64 kNoCap = ~0ull;

template <int N>
inline bool report_sizes(const u64 (&sizes)[N], const u64 (&caps)[N], u64* sizes_out) {
  bool fits = true;
  for (int q = 0; q < N; q++) {
    sizes_out[q] = sizes[q];
    fits = fits && caps[q] >= sizes[q];
  }
  return fits;
}

struct TregWire {
  uint8_t* key_bytes;
  u64 *key_offs, *ts;
  uint8_t* val_bytes;
  u64* val_offs;
};
inline int32_t treg_format(jy_engine* eng, Tmp& tmp, const Keys& K, u64 n, bool pending, const u64 (&caps)[3],
                           const TregWire& o, u64* sizes_out, int32_t mem, bool* written) {
  *written = false;
  TregRecs R;
  u64* voff;
  JY_TRY(treg_records(eng, tmp, pending, K.slots, n, R));
  JY_TRY(value_offsets(eng, tmp, R.lr, n, &voff));
  u64 tot[2];
  JY_TRY(totals(eng, {K.koff + n, voff + n}, tot));
  // every launch before this read has finished: a duplicate-list overflow fails a state read, as jy_treg_read
  if (!pending) JY_TRY(jy_treg_overflow_check(eng));
  const u64 kbytes = tot[0], vbytes = tot[1];
  if (!report_sizes({n, kbytes, vbytes}, caps, sizes_out)) return JY_OK;  // sizes only
  JY_TRY(emit_keys(eng, tmp, JY_TREG, K, n, kbytes, o.key_bytes, o.key_offs, mem));
  JY_TRY(emit(eng, mem, o.ts, R.ts, n * 8));
  JY_TRY(emit_values(eng, tmp, JY_TREG, R.pre, R.lr, voff, n, vbytes, o.val_bytes, o.val_offs, mem));
  *written = true;
  return JY_OK;
}

struct TlogWire {
  uint8_t* key_bytes;
  u64 *key_offs, *cutoff, *ent_offs, *ts;
  uint8_t* val_bytes;
  u64* val_offs;
};
inline int32_t tlog_format(jy_engine* eng, Tmp& tmp, const Keys& K, u64 n, const TlogState& t, const u64 (&caps)[4],
                           const TlogWire& o, u64* sizes_out, int32_t mem, bool* written) {
  *written = false;
  TlogRecs R;
  JY_TRY(tlog_sizing(eng, tmp, t, K.slots, n, R));
  u64 tot[2];
  JY_TRY(totals(eng, {K.koff + n, R.eoff + n}, tot));
  const u64 kbytes = tot[0], m = R.m = tot[1];
  // (the value bytes are a size of the batch: the entries are read before the capacity check)
  u64 *voff, vbytes = 0;
  JY_TRY(tlog_entries(eng, tmp, t, K.slots, n, R));
  JY_TRY(value_offsets(eng, tmp, R.lr, m, &voff));
  JY_TRY(totals(eng, {voff + m}, &vbytes));
  if (!report_sizes({n, kbytes, m, vbytes}, caps, sizes_out)) return JY_OK;  // sizes only
  JY_TRY(emit_keys(eng, tmp, JY_TLOG, K, n, kbytes, o.key_bytes, o.key_offs, mem));
  JY_TRY(emit(eng, mem, o.cutoff, R.cuts, n * 8));
  JY_TRY(emit(eng, mem, o.ent_offs, R.eoff, (n + 1) * 8));
  JY_TRY(emit(eng, mem, o.ts, R.ts, m * 8));
  JY_TRY(emit_values(eng, tmp, JY_TLOG, R.pre, R.lr, voff, m, vbytes, o.val_bytes, o.val_offs, mem));
  *written = true;
  return JY_OK;
}

struct UjsonWire {
  uint8_t* key_bytes;
  u64 *key_offs, *el_offs, *dots, *elems, *vv_offs, *vv, *cloud_offs, *cloud;
};
inline int32_t ujson_format(jy_engine* eng, Tmp& tmp, const Keys& K, u64 n, const UjsonState& u, const u64 (&caps)[5],
                            const UjsonWire& o, u64* sizes_out, int32_t mem, bool* written) {
  *written = false;
  const u32 R = u.R;
  UjsonRecs D;
  u64 *sv, *vo, *dv;
  JY_TRY(ujson_sizing(eng, tmp, u, K.slots, n, D));
  // the wire form's version vectors are packed: count, scan, and (below) pack the dense ones
  JY_TRY(tmp.get(&sv, n + 1));
  JY_TRY(tmp.get(&vo, n + 1));
  LAUNCH(k_wire_vv_count, n + 1, u.vv, R, K.slots, n, sv);
  JY_TRY(jy_scan_u64(eng, sv, vo, n));
  u64 tot[4];
  JY_TRY(totals(eng, {K.koff + n, D.eo + n, vo + n, D.co + n}, tot));
  const u64 kbytes = tot[0], me = D.me = tot[1], mv = tot[2], mc = D.mc = tot[3];
  if (!report_sizes({n, kbytes, me, mv, mc}, caps, sizes_out)) return JY_OK;  // sizes only
  JY_TRY(emit_keys(eng, tmp, JY_UJSON, K, n, kbytes, o.key_bytes, o.key_offs, mem));
  JY_TRY(tmp.out(&dv, o.vv, mv, mem));
  JY_TRY(ujson_entries(eng, tmp, u, K.slots, n, D, mem, o.dots, o.elems, nullptr, o.cloud));
  if (mv) LAUNCH(k_wire_vv_pack, n, D.dense, R, n, vo, dv);
  JY_TRY(emit(eng, mem, o.dots, D.dots, me * 8));
  JY_TRY(emit(eng, mem, o.elems, D.elems, me * 8));
  JY_TRY(emit(eng, mem, o.vv, dv, mv * 8));
  JY_TRY(emit(eng, mem, o.cloud, D.cloud, mc * 8));
  JY_TRY(emit(eng, mem, o.el_offs, D.eo, (n + 1) * 8));
  JY_TRY(emit(eng, mem, o.vv_offs, vo, (n + 1) * 8));
  JY_TRY(emit(eng, mem, o.cloud_offs, D.co, (n + 1) * 8));
  *written = true;
  return JY_OK;
}

// Counters: the two cell producers differ (a flush reads its pending mask and
// [g][k] values under one column, a snapshot the slab through masks and
// tiles); both hand over the per-key cell offsets coff (coff[n] = all cells)
// and write(sign, col, val): the launch that fills the three cell arrays.
struct CounterWire {
  uint8_t* key_bytes;
  u64 *key_offs, *cell_offs;
  uint8_t* sign;
  u16* col;
  u64* val;
};
template <class Write>
inline int32_t counter_format(jy_engine* eng, Tmp& tmp, int32_t type, const Keys& K, u64 n, const u64* coff,
                              const u64 (&caps)[3], const CounterWire& o, u64* sizes_out, int32_t mem, bool* written,
                              Write write) {
  *written = false;
  u64 tot[2];
  JY_TRY(totals(eng, {K.koff + n, coff + n}, tot));
  const u64 kbytes = tot[0], ncells = tot[1];
  if (!report_sizes({n, kbytes, ncells}, caps, sizes_out)) return JY_OK;  // sizes only
  JY_TRY(emit_keys(eng, tmp, type, K, n, kbytes, o.key_bytes, o.key_offs, mem));
  uint8_t* ds;
  u16* dc;
  u64* dv;
  JY_TRY(tmp.out(&ds, o.sign, ncells, mem));
  JY_TRY(tmp.out(&dc, o.col, ncells, mem));
  JY_TRY(tmp.out(&dv, o.val, ncells, mem));
  JY_TRY(write(ncells, ds, dc, dv));
  JY_TRY(emit(eng, mem, o.sign, ds, ncells));
  JY_TRY(emit(eng, mem, o.col, dc, ncells * 2));
  JY_TRY(emit(eng, mem, o.val, dv, ncells * 8));
  JY_TRY(emit(eng, mem, o.cell_offs, coff, (n + 1) * 8));
  *written = true;
  return JY_OK;
}

}  // namespace
