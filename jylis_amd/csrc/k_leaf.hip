// k_leaf.hip -- the UJSON leaf store: element handle -> leaf bytes, in HBM.
//
// Replaces the host dictionary behind UJSON element handles (`LeafTable` of
// jylis_amd/ujson_doc.py, `_leaves` of pony/jylis_gpu/repo_ujson_gpu.pony).
// The reference's UJSON delta carries real paths and values
// (repo_ujson.pony:65-66); with the store next to the documents, any UJSON
// wire batch can be accompanied by the bytes of its leaves
// (jy_ujson_leaves_get on its `elems`), so a receiver can answer GET.
//
// HBM layout (LeafStore), content-addressed, append-only between collections
// (jy_leaf.hpp):
//   tkey[tcap]   open addressing, linear probing, tcap a power of two kept
//                >= 2x the leaves: the u64 handle of an entry, 0 = empty
//   tref[tcap]   the entry's leaf, offset << 24 | length (the lr form);
//                bit 63 set = not stored: ~0, or kPend | i while input item i
//                of a put in flight owns the entry
//   bytes[bcap]  the leaf arena; a leaf starts on an 8-byte granule and owns
//                its length rounded up to 8, so jy_ld8u and k_wire_gather read
//                it unchanged
//   ctr[]        [0] leaves, [1] arena bytes used, [2] collisions
//
// put, three launches, a lane per leaf, no lane ever waits for another:
//   k_leaf_claim    length guard, hash, probe.  An empty entry is claimed by a
//                   CAS of the handle; every item that reaches its handle's
//                   entry while the entry is not stored offers its input index
//                   with an atomicMin, so the FIRST input item of a handle
//                   owns it however the CASes landed.  Handles out.
//   k_leaf_store    an owner takes arena room (one atomicAdd) and copies its
//                   bytes; every other item compares its bytes with the stored
//                   leaf (an entry of an earlier call) or with its owner's
//                   INPUT bytes (already in HBM): different bytes under one
//                   handle are a collision -- handle 0, counted, first stays.
//   k_leaf_publish  owners write their lr into tref.  An owner whose leaf did
//                   not fit the arena (device offsets that lied about their
//                   total) hands the entry back as not stored; it and its
//                   followers get handle 0 and are counted in jy_skipped.
// The host makes room BEFORE the launches, as jy_keys_reserve does for the
// key directory: it keeps upper bounds of the leaves and bytes (+= a put's
// worst case) and only when those reach the capacity reads the exact counters
// back, rehashes into a larger table and reallocates the arena.
//
// get: k_leaf_lookup gives the lr of every handle (0: unknown or handle 0),
// jy_scan_u64 turns the lengths into offsets, and the bytes are gathered by
// k_wire_gather with LeafSrc (jy_wire.hpp), balanced by output bytes.
//
// collect (jy_ujson_leaves_collect): the leaves no document refers to any more
// are dropped and table and arena rebuilt.  A handle is the hash of its leaf,
// so it survives the move of the bytes: no element pool, pending delta or
// digest is rewritten.
//   k_leaf_mark_docs  flattened over the live elements of a document store
//                     (the state, then the pending deltas), a lane per element:
//                     its document by the tile search of k_uj_path_match over
//                     the scanned sizes, its handle through uj_elem_at (either
//                     layout; only meta-described segments, never a dead run),
//                     the table walked as k_leaf_lookup does; AFTER the walk a
//                     plain 1 into the entry's flag (idempotent: no atomic).
//                     The grid is sized by the host's live_e bound and strides,
//                     so the host does not wait for the element total.
//   k_leaf_mark_keep  the same for the caller's `keep` handles
//   k_leaf_plan       per entry the kept length rounded up to 8; jy_scan_u64
//                     over the flags and over those lengths, in table order;
//                     k_leaf_totals gathers the six result words, the ONE
//                     read-back the host waits for (it sizes the new buffers)
//   k_leaf_move       a kept entry's handle and old lr to its scanned position,
//                     and the handle with its new lr into the fresh table (CAS
//                     on an empty entry, as k_leaf_rehash)
//   k_wire_gather     LeafSrc over the compacted old lrs, balanced by output
//                     bytes: a 70,000-byte leaf spreads over lanes, as in get
// The new buffers are allocated before anything is freed; the old ones are
// freed in stream order.
//
// Every table walk is bounded by the table size.  Roofline: latency/HBM -- a
// put reads its input once per pass that needs it (hash, copy or compare),
// one probe chain, and writes new leaves once; a get reads one probe chain
// per handle and moves each leaf's bytes once.  Times per call at 2^20 leaves
// of 24 bytes: DESIGN.md, "UJSON leaf store"; nothing here was tuned to a profile.

#include <algorithm>
#include <cstring>

#include "jy_leaf.hpp"
#include "jy_scan.hpp"
#include "jy_wire.hpp"

namespace {

constexpr u64 kPend = 1ull << 63;
constexpr u64 kIdx = 0xFFFFFFFFull;
constexpr u64 kNotStored = ~0ull;
constexpr u64 kNone = ~0ull;  // pos: the item is skipped; own: nothing to publish
constexpr u64 kMinTable = 1024;
constexpr u64 kMinArena = 1 << 16;

struct Leaves {
  u64* tkey;
  u64* tref;
  u64 mask;
  u32 shift;  // 64 - log2(tcap)
  uint8_t* bytes;
  u64 bcap;
  u64* ctr;
};

struct LdWords {  // aligned 8-byte loads, never past the words that hold the bytes asked for
  const uint8_t* p;
  __device__ __forceinline__ u64 operator()(u64 i, u64 m) const { return jy_ld8u(p + i, m); }
};

// n bytes at a equal n bytes at b.  NOT inlined: a comparison loop inlined into
// a probe loop lost the match on this compiler ("the key-probe miscompile")
__device__ __attribute__((noinline)) bool leaf_equal(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                     u64 n) {
  for (u64 i = 0; i < n; i += 8)
    if (jy_ld8u(a + i, n - i) != jy_ld8u(b + i, n - i)) return false;
  return true;
}

// item i of a put is element at(i) of the offsets: itself, or the idx[i]-th for
// a caller that puts a selection of a batch's leaves (jy_ujson_write_keys: the INS ones)
struct LeafIn {
  const u64* lo;
  const u32* idx;  // or null
  __device__ __forceinline__ u64 at(u64 i) const { return idx ? idx[i] : i; }
};

__global__ __launch_bounds__(kThreads) void k_leaf_claim(Leaves L, const uint8_t* __restrict__ lb, LeafIn in, u64 n,
                                                         u64* __restrict__ hout, u64* __restrict__ pos,
                                                         unsigned long long* skipped) {
  const u64 i = gid();
  if (i >= n) return;
  const u64 q = in.at(i), a = in.lo[q];
  u64 len;
  if (jy_leaf_len(a, in.lo[q + 1], &len)) {
    const u64 h = jy_leaf_hash_ld(LdWords{lb + a}, len);
    u64 p = jy_leaf_start(h, L.shift);
    // outputs written and the lane done AT the match (the shape of k_key_claim)
    for (u64 walk = 0; walk <= L.mask; walk++) {
      u64 k = L.tkey[p];
      if (k == 0) {
        const u64 prev = atomicCAS(reinterpret_cast<unsigned long long*>(&L.tkey[p]), 0ull, h);
        k = prev == 0 ? h : prev;
      }
      if (k == h) {
        if (L.tref[p] >> 63) atomicMin(reinterpret_cast<unsigned long long*>(&L.tref[p]), kPend | i);
        hout[i] = h;
        pos[i] = p;
        return;
      }
      p = jy_leaf_next(p, L.mask);
    }
    // (the walk met a full table: the host's bound was wrong; the item is skipped)
  }
  hout[i] = 0;
  pos[i] = kNone;
  atomicAdd(skipped, 1ull);  // malformed items are rare: no wave aggregation
}

__global__ __launch_bounds__(kThreads) void k_leaf_store(Leaves L, const uint8_t* __restrict__ lb, LeafIn in, u64 n,
                                                         u64* __restrict__ hout, const u64* __restrict__ pos,
                                                         u64* __restrict__ own, u64* __restrict__ nref) {
  const u64 i = gid();
  bool clash = false;
  if (i < n && pos[i] != kNone) {
    const u64 q = in.at(i), a = in.lo[q], len = in.lo[q + 1] - a;  // (guarded by the claim)
    const u64 r = L.tref[pos[i]];
    u64 o = kNone;
    if (!(r >> 63)) {  // stored by an earlier call
      clash = (r & JY_LR_LEN_MASK) != len || !leaf_equal(L.bytes + (r >> JY_LR_LEN_BITS), lb + a, len);
    } else if ((r & kIdx) == i) {  // this item owns the entry
      const u64 room = (len + 7) & ~7ull;
      const u64 at = atomicAdd(reinterpret_cast<unsigned long long*>(L.ctr + 1), room);
      o = i;
      if (at + room > L.bcap) {
        atomicAdd(reinterpret_cast<unsigned long long*>(L.ctr + 1), 0ull - room);
        nref[i] = kNotStored;
      } else {
        u64* dst = reinterpret_cast<u64*>(L.bytes + at);
        for (u64 q = 0; q < len; q += 8) dst[q >> 3] = jy_ld8u(lb + a + q, len - q);
        nref[i] = (at << JY_LR_LEN_BITS) | len;
      }
    } else {  // an earlier item of this call owns it: its input bytes are the leaf
      const u64 j = r & kIdx;
      const u64 qj = in.at(j), aj = in.lo[qj];
      clash = in.lo[qj + 1] - aj != len || !leaf_equal(lb + aj, lb + a, len);
      if (!clash) o = j;
    }
    own[i] = o;
    if (clash) hout[i] = 0;
  }
  jy_wave_count(clash, reinterpret_cast<unsigned long long*>(L.ctr + 2));
}

__global__ __launch_bounds__(kThreads) void k_leaf_publish(Leaves L, u64 n, u64* __restrict__ hout,
                                                           const u64* __restrict__ pos, const u64* __restrict__ own,
                                                           const u64* __restrict__ nref, unsigned long long* skipped) {
  const u64 i = gid();
  bool added = false, lost = false;
  if (i < n && pos[i] != kNone && own[i] != kNone) {
    const u64 r = nref[own[i]];
    if (own[i] == i) {
      L.tref[pos[i]] = r;
      added = r != kNotStored;
    }
    if (r == kNotStored) {
      hout[i] = 0;
      lost = true;
    }
  }
  jy_wave_count(added, reinterpret_cast<unsigned long long*>(L.ctr));
  jy_wave_count(lost, skipped);
}

// the stored entries of the old table into the new one (distinct handles: a
// CAS on an empty entry always finds one within the table)
__global__ __launch_bounds__(kThreads) void k_leaf_rehash(const u64* __restrict__ okey, const u64* __restrict__ oref,
                                                          u64 ocap, Leaves L) {
  const u64 s = gid();
  if (s >= ocap) return;
  const u64 h = okey[s], r = oref[s];
  if (h == 0 || (r >> 63)) return;
  u64 p = jy_leaf_start(h, L.shift);
  for (u64 walk = 0; walk <= L.mask; walk++) {
    if (atomicCAS(reinterpret_cast<unsigned long long*>(&L.tkey[p]), 0ull, h) == 0) {
      L.tref[p] = r;
      return;
    }
    p = jy_leaf_next(p, L.mask);
  }
}

// lr[j] = the stored leaf of handles[j], 0 if there is none (handle 0 included);
// len[j] its length (len[n] = 0 for the scan)
__global__ __launch_bounds__(kThreads) void k_leaf_lookup(Leaves L, const u64* __restrict__ handles, u64 n,
                                                          u64* __restrict__ lr, u64* __restrict__ len,
                                                          unsigned long long* missing) {
  const u64 j = gid();
  if (j > n) return;
  if (j == n) {
    len[n] = 0;
    return;
  }
  const u64 h = handles[j];
  if (h != 0 && L.tkey) {
    u64 p = jy_leaf_start(h, L.shift);
    for (u64 walk = 0; walk <= L.mask; walk++) {
      const u64 k = L.tkey[p];
      if (k == 0) break;
      if (k == h) {
        const u64 r = L.tref[p];
        if (r >> 63) break;  // claimed, never stored
        lr[j] = r;
        len[j] = r & JY_LR_LEN_MASK;
        return;
      }
      p = jy_leaf_next(p, L.mask);
    }
  }
  lr[j] = 0;
  len[j] = 0;
  atomicAdd(missing, 1ull);
}

// ---- collect ----
struct MarkDocs {  // a document store, either layout (the state or the pending deltas)
  const UMeta* meta;
  const URec* epool;
  const LCol* lcol;
  const URec* lpe;
  u32 R;
};

// the entry that stores handle h, kNone if there is none (h == 0, unknown, or
// claimed and never stored).  The walk of k_leaf_lookup; no inner loop in it.
__device__ __forceinline__ u64 leaf_entry_of(const Leaves& L, u64 h) {
  if (h == 0) return kNone;
  u64 p = jy_leaf_start(h, L.shift);
  for (u64 walk = 0; walk <= L.mask; walk++) {
    const u64 k = L.tkey[p];
    if (k == 0) return kNone;
    if (k == h) return (L.tref[p] >> 63) ? kNone : p;
    p = jy_leaf_next(p, L.mask);
  }
  return kNone;
}

// flag[entry] = 1 for the handle of every live element of documents 0 .. n - 1
// (eo[n + 1]: their scanned element counts).  Tiles of kThreads elements, the
// grid striding over them; `missing` counts elements without a stored leaf.
__global__ __launch_bounds__(kThreads) void k_leaf_mark_docs(MarkDocs D, const u64* __restrict__ eo, u64 n, Leaves L,
                                                             u64* __restrict__ flag, unsigned long long* missing) {
  __shared__ u64 sh[2];
  const u64 total = eo[n];
  for (u64 t0 = (u64)blockIdx.x * kThreads; t0 < total; t0 += (u64)gridDim.x * kThreads) {
    const u64 t1 = t0 + kThreads < total ? t0 + kThreads : total;
    if (threadIdx.x < 128) {
      const u64 k = jyscan::wave_last_le(eo, n, threadIdx.x < 64 ? t0 : t1 - 1);
      if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = k;
    }
    __syncthreads();
    const u64 t = t0 + threadIdx.x;
    const bool in = t < t1;
    bool miss = false;
    if (in) {
      u64 lo = sh[0], hi = sh[1];
      while (lo < hi) {
        const u64 m = (lo + hi + 1) >> 1;
        if (eo[m] <= t) lo = m;
        else hi = m - 1;
      }
      const UMeta m = D.meta[lo];
      const u64 h = uj_elem_at(m, D.epool, D.lcol, D.lpe, D.R, t - eo[lo]).elem;
      const u64 p = leaf_entry_of(L, h);
      if (p != kNone) flag[p] = 1;
      else miss = true;
    }
    jy_wave_count(miss, missing);
    __syncthreads();  // sh is written again by the next tile
  }
}

// the same for the caller's handles; handle 0 is ignored
__global__ __launch_bounds__(kThreads) void k_leaf_mark_keep(const u64* __restrict__ keep, u64 n, Leaves L,
                                                             u64* __restrict__ flag, unsigned long long* missing) {
  const u64 j = gid();
  bool miss = false;
  if (j < n) {
    const u64 h = keep[j];
    const u64 p = leaf_entry_of(L, h);
    if (p != kNone) flag[p] = 1;
    else miss = h != 0;
  }
  jy_wave_count(miss, missing);
}

// room[s] = the arena room a kept entry owns (its length rounded up to 8), 0
// for the others; entry tcap closes both scans
__global__ __launch_bounds__(kThreads) void k_leaf_plan(const u64* __restrict__ tref, u64 tcap, u64* __restrict__ flag,
                                                        u64* __restrict__ room) {
  const u64 s = gid();
  if (s > tcap) return;
  if (s == tcap) {
    flag[s] = 0;
    room[s] = 0;
    return;
  }
  room[s] = flag[s] ? ((tref[s] & JY_LR_LEN_MASK) + 7) & ~7ull : 0;
}

// out6 on the device: {kept, bytes kept, dropped, bytes dropped, elements
// without a leaf, keep handles without a leaf}
__global__ void k_leaf_totals(const u64* __restrict__ fo, const u64* __restrict__ bo, u64 tcap,
                              const u64* __restrict__ ctr, const u64* __restrict__ miss, u64* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const u64 k = fo[tcap], b = bo[tcap];
  out[0] = k;
  out[1] = b;
  out[2] = ctr[0] - k;
  out[3] = ctr[1] - b;
  out[4] = miss[0];
  out[5] = miss[1];
}

// a kept entry: its handle with its new lr into the fresh table N (distinct
// handles: a CAS on an empty entry always finds one), its old lr and new offset
// to position fo[s] for the gather; lane ocap closes the offsets
__global__ __launch_bounds__(kThreads) void k_leaf_move(const u64* __restrict__ okey, const u64* __restrict__ oref,
                                                        u64 ocap, const u64* __restrict__ flag,
                                                        const u64* __restrict__ fo, const u64* __restrict__ bo,
                                                        Leaves N, u64* __restrict__ olr, u64* __restrict__ noff) {
  const u64 s = gid();
  if (s > ocap) return;
  if (s == ocap) {
    noff[fo[ocap]] = bo[ocap];
    return;
  }
  if (!flag[s]) return;
  const u64 h = okey[s], r = oref[s], at = bo[s];
  olr[fo[s]] = r;
  noff[fo[s]] = at;
  const u64 nr = (at << JY_LR_LEN_BITS) | (r & JY_LR_LEN_MASK);
  u64 p = jy_leaf_start(h, N.shift);
  for (u64 walk = 0; walk <= N.mask; walk++) {
    if (atomicCAS(reinterpret_cast<unsigned long long*>(&N.tkey[p]), 0ull, h) == 0) {
      N.tref[p] = nr;
      return;
    }
    p = jy_leaf_next(p, N.mask);
  }
}

Leaves view(const LeafStore& S) {
  return Leaves{S.tkey, S.tref, S.tcap ? S.tcap - 1 : 0, 64 - S.lg, S.bytes, S.bcap, S.ctr};
}

// a table for `need` leaves: rehashed into a larger one when it is too small
u64 table_for(u64 need, u32* lg_out) {  // the entries of a table for `need` leaves
  u64 want = kMinTable;
  u32 lg = 10;
  while (want < 2 * need) {
    want <<= 1;
    lg++;
  }
  *lg_out = lg;
  return want;
}

int32_t grow_table(jy_engine* eng, LeafStore& S, u64 need) {
  u32 lg;
  const u64 want = table_for(need, &lg);
  if (S.tkey && want <= S.tcap) return JY_OK;
  u64 *nk = nullptr, *nr = nullptr;
  JY_TRY(jy_dev_alloc(eng, reinterpret_cast<void**>(&nk), want * 8, "leaf table"));
  JY_TRY(jy_dev_alloc(eng, reinterpret_cast<void**>(&nr), want * 8, "leaf table"));
  JY_HIP(eng, hipMemsetAsync(nk, 0, want * 8, eng->stream));
  JY_HIP(eng, hipMemsetAsync(nr, 0xFF, want * 8, eng->stream));
  u64 *ok = S.tkey, *orf = S.tref;
  const u64 ocap = S.tcap;
  S.tkey = nk;
  S.tref = nr;
  S.tcap = want;
  S.lg = lg;
  if (ok && ocap) LAUNCH(k_leaf_rehash, ocap, ok, orf, ocap, view(S));
  jy_dev_free(eng, ok);
  jy_dev_free(eng, orf);
  return JY_OK;
}

int32_t grow_arena(jy_engine* eng, LeafStore& S, u64 need) {
  if (S.bytes && need <= S.bcap) return JY_OK;
  const u64 nc = (std::max<u64>(std::max<u64>(need, S.bcap * 2), kMinArena) + 7) & ~7ull;
  if (nc >> (64 - JY_LR_LEN_BITS)) return eng->fail(JY_ERANGE, "leaf arena beyond what an lr can address");
  void* a = S.bytes;
  JY_TRY(jy_realloc(eng, &a, S.bcap, nc, false));
  S.bytes = static_cast<uint8_t*>(a);
  S.bcap = nc;
  return JY_OK;
}

int32_t counters(jy_engine* eng, LeafStore& S) {
  if (S.ctr) return JY_OK;
  JY_TRY(jy_dev_alloc(eng, reinterpret_cast<void**>(&S.ctr), 64, "leaf counters"));
  JY_HIP(eng, hipMemsetAsync(S.ctr, 0, 64, eng->stream));
  return JY_OK;
}

// the exact counters -> the host's bounds (waits for the stream)
int32_t exact(jy_engine* eng, LeafStore& S, u64* out3) {
  u64 t[3] = {0, 0, 0};
  if (S.ctr) JY_TRY(totals(eng, {S.ctr, S.ctr + 1, S.ctr + 2}, t));
  S.n_bound = t[0];
  S.b_bound = t[1];
  if (out3) std::memcpy(out3, t, sizeof t);
  return JY_OK;
}

// room for add_n more leaves and add_b more arena bytes, by the bounds; the
// exact counters are read only when the bounds say there is none
int32_t room(jy_engine* eng, LeafStore& S, u64 add_n, u64 add_b) {
  JY_TRY(counters(eng, S));
  const bool have = S.tkey && S.bytes;
  if (have && 2 * (S.n_bound + add_n) <= S.tcap && S.b_bound + add_b <= S.bcap) return JY_OK;
  if (have) JY_TRY(exact(eng, S, nullptr));
  JY_TRY(grow_table(eng, S, S.n_bound + add_n));
  return grow_arena(eng, S, S.b_bound + add_b);
}

// collect's mark of one document store: the live elements of its documents
// 0 .. n - 1 (meta-described segments only) -> the flags of their entries.
// Nothing is read back: the grid covers the host's bound of the live elements
// and strides over any excess.
constexpr u64 kMarkLanes = 1ull << 24;
int32_t mark_store(jy_engine* eng, Tmp& tmp, const UjsonState& u, u64 n, const Leaves& L, u64* flag, u64* miss) {
  if (n == 0 || !u.meta) return JY_OK;
  u32* slots;
  u64 *se, *sc, *eo;
  JY_TRY(tmp.get(&slots, n));
  JY_TRY(tmp.get(&se, n + 1));
  JY_TRY(tmp.get(&sc, n));
  JY_TRY(tmp.get(&eo, n + 1));
  LAUNCH(k_wire_iota, n, 0u, n, slots);
  JY_HIP(eng, hipMemsetAsync(se + n, 0, 8, eng->stream));
  JY_TRY(jy_ujson_sizes_of(eng, u, n, slots, se, sc));
  JY_TRY(jy_scan_u64(eng, se, eo, n));
  const u64 lanes = std::min<u64>(std::max<u64>(u.live_e, kThreads), kMarkLanes);
  LAUNCH(k_leaf_mark_docs, lanes, MarkDocs{u.meta, u.epool, u.lcol, u.lpe, u.R}, eo, n, L, flag,
         reinterpret_cast<unsigned long long*>(miss));
  return JY_OK;
}

// collect's new buffers: freed again unless the swap took them
struct NewStore {
  jy_engine* eng;
  u64 *tkey = nullptr, *tref = nullptr;
  uint8_t* bytes = nullptr;
  explicit NewStore(jy_engine* e) : eng(e) {}
  ~NewStore() {
    jy_dev_free(eng, tkey);
    jy_dev_free(eng, tref);
    jy_dev_free(eng, bytes);
  }
};

}  // namespace

// the put's core: n < 2^32 - 1 items in DEVICE memory (item i = element idx[i] of
// the offsets, or i with idx null), `span` an upper bound of their bytes; the
// handles go to dh (device).  Makes room first (which may wait), then only enqueues.
int32_t jy_leaves_put_core(jy_engine* eng, u64 n, const uint8_t* db, const u64* dof, const u32* idx, u64 span,
                           u64* dh) {
  LeafStore& S = eng->leaf;
  // a leaf owns its length rounded up to 8 (device offsets that are not
  // ascending inside can name more than this: k_leaf_store checks the arena)
  const u64 worst = span + 8 * n;
  JY_TRY(room(eng, S, n, worst));
  Tmp tmp(eng);
  u64 *pos, *own, *nref;
  JY_TRY(tmp.get(&pos, n));
  JY_TRY(tmp.get(&own, n));
  JY_TRY(tmp.get(&nref, n));
  const Leaves L = view(S);
  const LeafIn in{dof, idx};
  unsigned long long* skipped = reinterpret_cast<unsigned long long*>(eng->skipped_dev);
  LAUNCH(k_leaf_claim, n, L, db, in, n, dh, pos, skipped);
  LAUNCH(k_leaf_store, n, L, db, in, n, dh, pos, own, nref);
  LAUNCH(k_leaf_publish, n, L, n, dh, pos, own, nref, skipped);
  S.n_bound += n;
  S.b_bound += worst;
  return JY_OK;
}

void jy_leaf_free(jy_engine* eng, LeafStore& S) {
  for (void* p : {static_cast<void*>(S.tkey), static_cast<void*>(S.tref), static_cast<void*>(S.bytes),
                  static_cast<void*>(S.ctr)})
    jy_dev_free(eng, p);
  S = LeafStore{};
}

extern "C" {

int32_t jy_ujson_leaves_reserve(jy_engine* eng, uint64_t nleaves, uint64_t nbytes) {
  JY_HIP(eng, hipSetDevice(eng->device));
  LeafStore& S = eng->leaf;
  JY_TRY(counters(eng, S));
  JY_TRY(grow_table(eng, S, nleaves));
  return grow_arena(eng, S, nbytes);
}

int32_t jy_ujson_leaves_usage(jy_engine* eng, uint64_t* out4) {
  JY_HIP(eng, hipSetDevice(eng->device));
  LeafStore& S = eng->leaf;
  u64 t[3];
  JY_TRY(exact(eng, S, t));
  out4[0] = t[0];
  out4[1] = t[1];
  out4[2] = S.bcap;
  out4[3] = t[2];
  return JY_OK;
}

int32_t jy_ujson_leaves_put(jy_engine* eng, uint64_t n, const uint8_t* leaf_bytes, const uint64_t* leaf_offs,
                            uint64_t* handles_out, int32_t mem) {
  JY_HIP(eng, hipSetDevice(eng->device));
  JY_TRY(mem_check(eng, mem));
  if (n == 0) return JY_OK;
  if (n >= kIdx) return eng->fail(JY_ERANGE, "too many leaves in one call");
  if (!leaf_offs || !handles_out) return eng->fail(JY_EINVAL, "leaf_offs and handles_out must not be null");
  // the extent of the input bytes; host offsets are validated before anything is launched
  u64 first = 0, end = 0;
  if (mem == JY_HOST) {
    for (u64 i = 0; i < n; i++)
      if (leaf_offs[i + 1] < leaf_offs[i]) return eng->fail(JY_EINVAL, "leaf_offs is not ascending");
    first = leaf_offs[0];
    end = leaf_offs[n];
  } else {
    u64 fe[2];
    JY_TRY(totals(eng, {leaf_offs, leaf_offs + n}, fe));
    first = fe[0];
    end = fe[1];
    if (end < first) return eng->fail(JY_EINVAL, "leaf_offs is not ascending");
  }
  if (end > first && !leaf_bytes) return eng->fail(JY_EINVAL, "leaf_bytes is null");
  Tmp tmp(eng);
  const uint8_t* db = leaf_bytes;
  const u64* dof = leaf_offs;
  if (mem == JY_HOST) {
    uint8_t* b;
    u64* o;
    JY_TRY(tmp.get(&b, end));
    JY_TRY(tmp.get(&o, n + 1));
    if (end) JY_HIP(eng, hipMemcpyAsync(b, leaf_bytes, end, hipMemcpyHostToDevice, eng->stream));
    JY_HIP(eng, hipMemcpyAsync(o, leaf_offs, (n + 1) * 8, hipMemcpyHostToDevice, eng->stream));
    db = b;
    dof = o;
  }
  u64* dh;
  JY_TRY(tmp.out(&dh, handles_out, n, mem));
  JY_TRY(jy_leaves_put_core(eng, n, db, dof, nullptr, end - first, dh));
  JY_TRY(emit(eng, mem, handles_out, dh, n * 8));
  if (mem == JY_HOST) JY_HIP(eng, hipStreamSynchronize(eng->stream));
  return JY_OK;
}

int32_t jy_ujson_leaves_get(jy_engine* eng, uint64_t n, const uint64_t* handles, int32_t handles_mem,
                            uint64_t cap_bytes, uint8_t* leaf_bytes, uint64_t* leaf_offs, uint64_t* sizes_out,
                            int32_t mem) {
  JY_HIP(eng, hipSetDevice(eng->device));
  JY_TRY(mem_check(eng, mem));
  sizes_out[0] = sizes_out[1] = 0;
  if (handles_mem != JY_HOST && handles_mem != JY_DEVICE)
    return eng->fail(JY_EINVAL, "handles_mem must be JY_HOST or JY_DEVICE");
  if (n == 0) return empty_batch(eng, mem, {leaf_offs});
  if (!handles) return eng->fail(JY_EINVAL, "handles is null");
  const LeafStore& S = eng->leaf;
  Tmp tmp(eng);
  const u64* dh = handles;
  if (handles_mem == JY_HOST) {
    u64* h;
    JY_TRY(tmp.get(&h, n));
    JY_HIP(eng, hipMemcpyAsync(h, handles, n * 8, hipMemcpyHostToDevice, eng->stream));
    dh = h;
  }
  u64 *lr, *len, *off, *miss;
  JY_TRY(tmp.get(&lr, n));
  JY_TRY(tmp.get(&len, n + 1));
  JY_TRY(tmp.get(&off, n + 1));
  JY_TRY(tmp.get(&miss, 1));
  JY_HIP(eng, hipMemsetAsync(miss, 0, 8, eng->stream));
  LAUNCH(k_leaf_lookup, n + 1, view(S), dh, n, lr, len, reinterpret_cast<unsigned long long*>(miss));
  JY_TRY(jy_scan_u64(eng, len, off, n));
  u64 tot[2];
  JY_TRY(totals(eng, {off + n, miss}, tot));
  sizes_out[0] = tot[0];
  sizes_out[1] = tot[1];
  if (cap_bytes < tot[0]) return JY_OK;  // sizes only
  uint8_t* ob;
  JY_TRY(tmp.out(&ob, leaf_bytes, tot[0], mem));
  JY_TRY(gather(eng, LeafSrc{S.bytes, lr}, off, n, tot[0], ob));
  JY_TRY(emit(eng, mem, leaf_bytes, ob, tot[0]));
  JY_TRY(emit(eng, mem, leaf_offs, off, (n + 1) * 8));
  if (mem == JY_HOST) JY_HIP(eng, hipStreamSynchronize(eng->stream));
  return JY_OK;
}

int32_t jy_ujson_leaves_collect(jy_engine* eng, uint64_t n_keep, const uint64_t* keep, int32_t keep_mem,
                                uint32_t flags, uint64_t* out6) {
  JY_HIP(eng, hipSetDevice(eng->device));
  for (int q = 0; q < 6; q++) out6[q] = 0;
  if (flags & ~JY_LEAVES_SHRINK) return eng->fail(JY_EINVAL, "unknown leaves collect flags");
  if (keep_mem != JY_HOST && keep_mem != JY_DEVICE)
    return eng->fail(JY_EINVAL, "keep_mem must be JY_HOST or JY_DEVICE");
  if (n_keep && !keep) return eng->fail(JY_EINVAL, "keep is null");
  LeafStore& S = eng->leaf;
  if (!S.tkey || !S.bytes || !S.ctr) return JY_OK;  // never used: nothing to collect
  const u64 ocap = S.tcap;
  const Leaves L = view(S);
  Tmp tmp(eng);

  // ---- mark: the state, the pending deltas, the caller's handles ----
  u64 *flag, *rm, *fo, *bo, *miss, *res;
  JY_TRY(tmp.get(&flag, ocap + 1));
  JY_TRY(tmp.get(&rm, ocap + 1));
  JY_TRY(tmp.get(&fo, ocap + 1));
  JY_TRY(tmp.get(&bo, ocap + 1));
  JY_TRY(tmp.get(&miss, 2));
  JY_TRY(tmp.get(&res, 6));
  JY_HIP(eng, hipMemsetAsync(flag, 0, (ocap + 1) * 8, eng->stream));
  JY_HIP(eng, hipMemsetAsync(miss, 0, 16, eng->stream));
  const u64 nk = eng->nkeys[JY_UJSON];
  JY_TRY(mark_store(eng, tmp, eng->ujson, std::min<u64>(nk, eng->ujson.kcap), L, flag, miss));
  JY_TRY(mark_store(eng, tmp, eng->ujson_d, std::min<u64>(nk, eng->ujson_d.kcap), L, flag, miss));
  if (n_keep) {
    const u64* dk = keep;
    if (keep_mem == JY_HOST) {  // (the caller's array outlives the call's wait)
      u64* k;
      JY_TRY(tmp.get(&k, n_keep));
      JY_HIP(eng, hipMemcpyAsync(k, keep, n_keep * 8, hipMemcpyHostToDevice, eng->stream));
      dk = k;
    }
    LAUNCH(k_leaf_mark_keep, n_keep, dk, n_keep, L, flag, reinterpret_cast<unsigned long long*>(miss + 1));
  }

  // ---- plan: the kept entries and their arena room, in table order ----
  LAUNCH(k_leaf_plan, ocap + 1, S.tref, ocap, flag, rm);
  JY_TRY(jy_scan_u64(eng, flag, fo, ocap));
  JY_TRY(jy_scan_u64(eng, rm, bo, ocap));
  hipLaunchKernelGGL(k_leaf_totals, dim3(1), dim3(64), 0, eng->stream, fo, bo, ocap, S.ctr, miss, res);
  JY_HIP(eng, hipGetLastError());
  u64 t[6];
  JY_HIP(eng, hipMemcpyAsync(t, res, sizeof t, hipMemcpyDeviceToHost, eng->stream));
  JY_HIP(eng, hipStreamSynchronize(eng->stream));  // the one wait before the move: it sizes the new buffers
  const u64 kept = t[0], kbytes = t[1];

  // ---- the new table and arena, allocated before anything is freed ----
  u64 ncap = ocap, nbcap = S.bcap;
  u32 nlg = S.lg;
  if (flags & JY_LEAVES_SHRINK) {
    u32 lg;
    const u64 want = table_for(2 * kept, &lg);
    if (want < ocap) ncap = want, nlg = lg;
    nbcap = std::min<u64>(S.bcap, std::max<u64>(kMinArena, 2 * kbytes));  // (both multiples of 8)
  }
  NewStore N(eng);
  JY_TRY(jy_dev_alloc(eng, reinterpret_cast<void**>(&N.tkey), ncap * 8, "leaf table"));
  JY_TRY(jy_dev_alloc(eng, reinterpret_cast<void**>(&N.tref), ncap * 8, "leaf table"));
  JY_TRY(jy_dev_alloc(eng, reinterpret_cast<void**>(&N.bytes), nbcap, "leaf arena"));
  u64 *olr, *noff;
  JY_TRY(tmp.get(&olr, kept));
  JY_TRY(tmp.get(&noff, kept + 1));
  JY_HIP(eng, hipMemsetAsync(N.tkey, 0, ncap * 8, eng->stream));
  JY_HIP(eng, hipMemsetAsync(N.tref, 0xFF, ncap * 8, eng->stream));

  // ---- move ----
  const Leaves NL{N.tkey, N.tref, ncap - 1, 64 - nlg, N.bytes, nbcap, S.ctr};
  LAUNCH(k_leaf_move, ocap + 1, S.tkey, S.tref, ocap, flag, fo, bo, NL, olr, noff);
  JY_TRY(gather(eng, LeafSrc{S.bytes, olr}, noff, kept, kbytes, N.bytes));
  JY_HIP(eng, hipMemcpyAsync(S.ctr, res, 16, hipMemcpyDeviceToDevice, eng->stream));  // leaves, bytes used; collisions stay

  // ---- swap: the old buffers are freed in stream order, behind the move ----
  jy_dev_free(eng, S.tkey);
  jy_dev_free(eng, S.tref);
  jy_dev_free(eng, S.bytes);
  S.tkey = N.tkey;
  S.tref = N.tref;
  S.bytes = N.bytes;
  N.tkey = N.tref = nullptr;
  N.bytes = nullptr;
  S.tcap = ncap;
  S.lg = nlg;
  S.bcap = nbcap;
  S.n_bound = kept;
  S.b_bound = kbytes;
  JY_HIP(eng, hipStreamSynchronize(eng->stream));
  std::memcpy(out6, t, sizeof t);
  return JY_OK;
}

}  // extern "C"
