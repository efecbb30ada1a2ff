// k_uj_path.hip -- UJSON path reads: the elements of a document whose leaf lies
// at or under a path, selected in HBM (jy_ujson_path_read).
//
// RepoUJSON is a path-addressed store (repo_ujson.pony:68-110): GET renders the
// leaves under a path, path-scoped CLR and SET remove them.  With documents
// (k_ujson.hip) and leaves (k_leaf.hip) both on the device, which elements a
// path selects is decided here and only the matches travel.  The leaf encoding
// (jy_leaf.hpp) makes it a byte comparison: a path encoded like a leaf's path,
// without the terminator, is a byte prefix of the leaf's encoding iff its
// segments are a prefix of the leaf's path -- the length words keep the segment
// boundaries aligned, and no segment length is the terminator FF FF FF FF.
//
// The query (slots, paths) is host memory and checked in full before anything
// is launched, so no device loop runs over an unchecked length.  Then:
//   sizes            jy_ujson_sizes_of + jy_scan_u64: eo[n + 1], the examined
//                    elements of every query (a JY_NO_SLOT query: none); the
//                    total is read back (first wait)
//   k_uj_path_match  flattened over the examined elements, a lane per element:
//                    its query by two wave_last_le searches per tile and a
//                    short bisect (as k_uj_gather_items: a document of 10^5
//                    elements spreads over many tiles); the handle through
//                    uj_elem_at (jy_internal.hpp, factored out of
//                    k_uj_gather_items<true>: regular pool or per-column long
//                    layout); the leaf table walked as k_leaf_lookup does;
//                    AFTER the walk the path against the leaf's leading bytes,
//                    8 at a time (path_prefix, noinline).  Writes the handle,
//                    the keep flag, the kept byte length and the lr.
//   scans            jy_scan_u64 over the flags and over the kept lengths
//                    and the read-back of their totals (second and last wait:
//                    "sizes only" when a capacity is short)
//   k_uj_path_offs   el_offs[i] = the flag scan at query i's first element
//   k_uj_path_compact  matched handles, their lr and skip (the path's length),
//                    and leaf_offs, each to its scanned position
//   k_wire_gather    LeafTailSrc (jy_wire.hpp: LeafSrc plus a per-item skip),
//                    balanced by output bytes: the relative leaves
//
// The path bytes are NOT staged in LDS: every lane of a tile inside one query
// reads the same one to three path words, which a wave loads as one broadcast
// line from L2; the lane's own dependent chain (handle, probe, leaf line) is
// what it waits for.  The staged form was not built, so there is no A/B.
//
// Roofline: latency-bound.  Per examined element one 16-byte element record,
// one probe chain (two dependent 8-byte loads at load factor <= 1/2) and one
// line of leaf bytes; per match its bytes once more, in the gather.  Times
// against the reads it replaces: DESIGN.md, "UJSON path reads"; nothing here
// was tuned to a profile.

#include <algorithm>
#include <cstring>

#include "jy_leaf.hpp"
#include "jy_scan.hpp"
#include "jy_wire.hpp"

namespace {

struct PathDocs {  // the state's documents, either layout
  const UMeta* meta;
  const URec* epool;
  const LCol* lcol;
  const URec* lpe;
  u32 R;
};
struct PathQueries {
  const u32* slots;  // [n] (a JY_NO_SLOT query names any slot: it has no elements)
  const u64* eo;     // [n + 1] examined-element offsets
  const uint8_t* pb;  // the paths, packed
  const u64* po;      // [n + 1]
  u64 n;
};
struct PathLeaves {  // the leaf store (k_leaf.hip)
  const u64* tkey;
  const u64* tref;
  u64 mask;
  u32 shift;
  const uint8_t* bytes;
};

// the n path bytes at p equal the first n bytes of the leaf at q (which holds
// at least n + 4).  NOT inlined and called after the probe loop has ended
// ("the key-probe miscompile"; leaf_equal of k_leaf.hip)
__device__ __attribute__((noinline)) bool path_prefix(const uint8_t* __restrict__ p, const uint8_t* __restrict__ q,
                                                      u64 n) {
  for (u64 i = 0; i < n; i += 8)
    if (jy_ld8u(p + i, n - i) != jy_ld8u(q + i, n - i)) return false;
  return true;
}

// slots with JY_NO_SLOT replaced by slot 0 (fix != null), or the sizes of such
// queries set to 0 (se != null)
__global__ __launch_bounds__(kThreads) void k_uj_path_holes(const u32* __restrict__ slots, u64 n,
                                                            u32* __restrict__ fix, u64* __restrict__ se) {
  const u64 i = gid();
  if (i >= n) return;
  const u32 s = slots[i];
  if (fix) fix[i] = s == JY_NO_SLOT ? 0u : s;
  if (se && s == JY_NO_SLOT) se[i] = 0;
}

__global__ __launch_bounds__(kThreads) void k_uj_path_match(PathDocs D, PathQueries Q, PathLeaves L, u64 total,
                                                            u64* __restrict__ he, u64* __restrict__ flag,
                                                            u64* __restrict__ klen, u64* __restrict__ lrs,
                                                            unsigned long long* missing) {
  __shared__ u64 sh[2];
  const u64 t0 = (u64)blockIdx.x * kThreads;
  if (t0 >= total) return;
  const u64 t1 = t0 + kThreads < total ? t0 + kThreads : total;
  if (threadIdx.x < 128) {
    const u64 k = jyscan::wave_last_le(Q.eo, Q.n, threadIdx.x < 64 ? t0 : t1 - 1);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = k;
  }
  __syncthreads();
  const u64 t = t0 + threadIdx.x;
  const bool in = t < t1;
  u64 lr = 0;
  if (in) {
    u64 lo = sh[0], hi = sh[1];
    while (lo < hi) {
      const u64 m = (lo + hi + 1) >> 1;
      if (Q.eo[m] <= t) lo = m;
      else hi = m - 1;
    }
    const UMeta m = D.meta[Q.slots[lo]];
    const u64 h = uj_elem_at(m, D.epool, D.lcol, D.lpe, D.R, t - Q.eo[lo]).elem;
    if (h != 0 && L.tkey) {
      u64 p = jy_leaf_start(h, L.shift);
      for (u64 walk = 0; walk <= L.mask; walk++) {
        const u64 k = L.tkey[p];
        if (k == 0) break;
        if (k == h) {
          const u64 r = L.tref[p];
          if (!(r >> 63)) lr = r;  // (else claimed, never stored)
          break;
        }
        p = jy_leaf_next(p, L.mask);
      }
    }
    // the walk has ended: the prefix compare, never past the leaf
    const u64 a = Q.po[lo], plen = Q.po[lo + 1] - a, len = lr & JY_LR_LEN_MASK;
    const bool keep =
        lr != 0 && plen + kLeafMinLen <= len && path_prefix(Q.pb + a, L.bytes + (lr >> JY_LR_LEN_BITS), plen);
    he[t] = h;
    flag[t] = keep ? 1 : 0;
    klen[t] = keep ? len - plen : 0;
    lrs[t] = lr;
  }
  jy_wave_count(in && lr == 0, missing);
}

// el_offs[i] = matched elements before query i's first examined element
__global__ __launch_bounds__(kThreads) void k_uj_path_offs(const u64* __restrict__ eo, const u64* __restrict__ fo,
                                                           u64 n, u64* __restrict__ el_offs) {
  const u64 i = gid();
  if (i <= n) el_offs[i] = fo[eo[i]];
}

// the matches to their scanned positions; lane `total` closes leaf_offs
__global__ __launch_bounds__(kThreads) void k_uj_path_compact(u64 total, const u64* __restrict__ flag,
                                                              const u64* __restrict__ fo, const u64* __restrict__ lo,
                                                              const u64* __restrict__ he, const u64* __restrict__ klen,
                                                              const u64* __restrict__ lrs, u64* __restrict__ elems,
                                                              u64* __restrict__ klr, u32* __restrict__ skip,
                                                              u64* __restrict__ leaf_offs) {
  const u64 t = gid();
  if (t > total) return;
  if (t == total) {
    if (leaf_offs) leaf_offs[fo[total]] = lo[total];
    return;
  }
  if (!flag[t]) return;
  const u64 p = fo[t];
  elems[p] = he[t];
  if (leaf_offs) {
    const u64 r = lrs[t];
    klr[p] = r;
    skip[p] = (u32)((r & JY_LR_LEN_MASK) - klen[t]);
    leaf_offs[p] = lo[t];
  }
}

// the host's check of one path: whole len|bytes segments, every len <= 2^24 - 1
int32_t path_check(jy_engine* eng, const uint8_t* b, u64 a, u64 e) {
  while (a < e) {
    if (e - a < 4) return eng->fail(JY_EINVAL, "a path ends inside a segment's length word");
    const u64 len = (u64)b[a] | (u64)b[a + 1] << 8 | (u64)b[a + 2] << 16 | (u64)b[a + 3] << 24;
    if (len > kLeafMaxLen) return eng->fail(JY_ERANGE, "a path segment longer than 2^24 - 1 bytes");
    if (len > e - a - 4) return eng->fail(JY_EINVAL, "a path's last segment is cut short");
    a += 4 + len;
  }
  return JY_OK;
}

// no element examined: every query's result is empty
int32_t nothing_matched(jy_engine* eng, int32_t mem, u64 n, u64* el_offs, u64* leaf_offs) {
  if (!el_offs) return empty_batch(eng, mem, {leaf_offs});  // (a sizing call without arrays)
  if (mem == JY_DEVICE) JY_HIP(eng, hipMemsetAsync(el_offs, 0, (n + 1) * 8, eng->stream));
  else std::memset(el_offs, 0, (n + 1) * 8);
  return empty_batch(eng, mem, {leaf_offs});
}

}  // namespace

extern "C" {

int32_t jy_ujson_path_read(jy_engine* eng, uint64_t n, const uint32_t* slots, const uint8_t* path_bytes,
                           const uint64_t* path_offs, uint32_t flags, uint64_t cap_el, uint64_t cap_bytes,
                           uint64_t* el_offs, uint64_t* elems, uint8_t* leaf_bytes, uint64_t* leaf_offs,
                           uint64_t* sizes_out, int32_t mem) {
  JY_HIP(eng, hipSetDevice(eng->device));
  for (int q = 0; q < 4; q++) sizes_out[q] = 0;
  JY_TRY(mem_check(eng, mem));
  if (flags & ~JY_PATH_LEAVES) return eng->fail(JY_EINVAL, "unknown path read flags");
  const bool leaves = flags & JY_PATH_LEAVES;
  if (!leaves) leaf_bytes = nullptr, leaf_offs = nullptr;
  if (n == 0) return empty_batch(eng, mem, {el_offs, leaf_offs});
  if (!slots || !path_offs) return eng->fail(JY_EINVAL, "slots and path_offs must not be null");
  // ---- the whole query is checked here, before any launch ----
  for (u64 i = 0; i < n; i++)
    if (path_offs[i + 1] < path_offs[i]) return eng->fail(JY_EINVAL, "path_offs is not ascending");
  const u64 first = path_offs[0], pbytes = path_offs[n] - first;
  if (pbytes && !path_bytes) return eng->fail(JY_EINVAL, "path_bytes is null");
  for (u64 i = 0; i < n; i++) JY_TRY(path_check(eng, path_bytes, path_offs[i], path_offs[i + 1]));
  const u64 nk = eng->nkeys[JY_UJSON];
  u64 holes = 0;
  for (u64 i = 0; i < n; i++) {
    if (slots[i] == JY_NO_SLOT) holes++;
    else if (slots[i] >= nk) return eng->fail(JY_ERANGE, "a path read names a slot past the interned keys");
  }
  if (holes == n) return nothing_matched(eng, mem, n, el_offs, leaf_offs);  // (no key may exist at all)

  const UjsonState& u = eng->ujson;
  const LeafStore& S = eng->leaf;
  Tmp tmp(eng);
  // the query -> the device (the caller's arrays outlive the call's first wait)
  u32* ds;
  uint8_t* pb;
  u64 *po, *se, *sc, *eo;
  JY_TRY(tmp.get(&ds, n));
  JY_TRY(tmp.get(&pb, pbytes));
  JY_TRY(tmp.get(&po, n + 1));
  JY_HIP(eng, hipMemcpyAsync(ds, slots, n * 4, hipMemcpyHostToDevice, eng->stream));
  if (pbytes) JY_HIP(eng, hipMemcpyAsync(pb, path_bytes + first, pbytes, hipMemcpyHostToDevice, eng->stream));
  JY_HIP(eng, hipMemcpyAsync(po, path_offs, (n + 1) * 8, hipMemcpyHostToDevice, eng->stream));
  const u32* dslots = ds;
  if (holes) {
    u32* fix;
    JY_TRY(tmp.get(&fix, n));
    LAUNCH(k_uj_path_holes, n, ds, n, fix, static_cast<u64*>(nullptr));
    dslots = fix;
  }
  // ---- the examined elements of every query ----
  JY_TRY(tmp.get(&se, n + 1));
  JY_TRY(tmp.get(&sc, n));
  JY_TRY(tmp.get(&eo, n + 1));
  JY_HIP(eng, hipMemsetAsync(se + n, 0, 8, eng->stream));
  JY_TRY(jy_ujson_sizes_of(eng, u, n, dslots, se, sc));
  if (holes) LAUNCH(k_uj_path_holes, n, ds, n, static_cast<u32*>(nullptr), se);
  JY_TRY(jy_scan_u64(eng, se, eo, n));
  u64 me = 0;
  JY_TRY(totals(eng, {eo + n}, &me));  // the first wait
  sizes_out[2] = me;
  if (me == 0) return nothing_matched(eng, mem, n, el_offs, leaf_offs);

  // ---- match, scan ----
  u64 *he, *flag, *klen, *lrs, *fo, *lo = nullptr, *miss;
  JY_TRY(tmp.get(&he, me));
  JY_TRY(tmp.get(&flag, me + 1));
  JY_TRY(tmp.get(&klen, me + 1));
  JY_TRY(tmp.get(&lrs, me));
  JY_TRY(tmp.get(&fo, me + 1));
  JY_TRY(tmp.get(&miss, 1));
  JY_HIP(eng, hipMemsetAsync(flag + me, 0, 8, eng->stream));
  JY_HIP(eng, hipMemsetAsync(klen + me, 0, 8, eng->stream));
  JY_HIP(eng, hipMemsetAsync(miss, 0, 8, eng->stream));
  const PathDocs D{u.meta, u.epool, u.lcol, u.lpe, u.R};
  // (po holds the caller's offsets: the packed copy starts at `first`)
  const PathQueries Q{dslots, eo, pb - first, po, n};
  const PathLeaves L{S.tkey, S.tref, S.tcap ? S.tcap - 1 : 0, 64 - S.lg, S.bytes};
  LAUNCH(k_uj_path_match, me, D, Q, L, me, he, flag, klen, lrs, reinterpret_cast<unsigned long long*>(miss));
  JY_TRY(jy_scan_u64(eng, flag, fo, me));
  if (leaves) {
    JY_TRY(tmp.get(&lo, me + 1));
    JY_TRY(jy_scan_u64(eng, klen, lo, me));
  }
  u64 tot[3];
  JY_TRY(totals(eng, {fo + me, leaves ? lo + me : miss, miss}, tot));  // the second and last wait
  const u64 m = tot[0], bytes = leaves ? tot[1] : 0;
  sizes_out[0] = m;
  sizes_out[1] = bytes;
  sizes_out[3] = tot[2];
  if (cap_el < m || cap_bytes < bytes) return JY_OK;  // sizes only
  if (!el_offs || !elems) return eng->fail(JY_EINVAL, "el_offs or elems is null");
  if (leaves && (!leaf_offs || (bytes && !leaf_bytes))) return eng->fail(JY_EINVAL, "leaf_bytes or leaf_offs is null");

  // ---- compact, gather ----
  u64 *dq, *de, *dlo = nullptr, *klr = nullptr;
  u32* skip = nullptr;
  uint8_t* ob = nullptr;
  JY_TRY(tmp.out(&dq, el_offs, n + 1, mem));
  JY_TRY(tmp.out(&de, elems, m, mem));
  if (leaves) {
    JY_TRY(tmp.out(&dlo, leaf_offs, m + 1, mem));
    JY_TRY(tmp.get(&klr, m));
    JY_TRY(tmp.get(&skip, m));
    JY_TRY(tmp.out(&ob, leaf_bytes, bytes, mem));
  }
  LAUNCH(k_uj_path_offs, n + 1, eo, fo, n, dq);
  LAUNCH(k_uj_path_compact, me + 1, me, flag, fo, lo, he, klen, lrs, de, klr, skip, dlo);
  if (leaves) JY_TRY(gather(eng, LeafTailSrc{S.bytes, klr, skip}, dlo, m, bytes, ob));
  JY_TRY(emit(eng, mem, el_offs, dq, (n + 1) * 8));
  JY_TRY(emit(eng, mem, elems, de, m * 8));
  if (leaves) {
    JY_TRY(emit(eng, mem, leaf_bytes, ob, bytes));
    JY_TRY(emit(eng, mem, leaf_offs, dlo, (m + 1) * 8));
  }
  return host_sync(eng, mem);
}

}  // extern "C"
