// jy_wire.hpp -- what the wire-form calls share: the byte-balanced string
// gather and the host-side helpers of one call (temporaries, totals, emit).
// Used by the flushes of pending deltas (k_flush_wire.hip) and by the state
// snapshots (k_state_wire.hip); both produce the arrays jy_node_*_converge
// takes.
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

}  // namespace
