// jy_uj_path.hpp -- the core of a UJSON path read, shared by the two calls that
// select leaves by path: jy_ujson_path_read (k_uj_path.hip), which hands the
// matches to the caller, and jy_ujson_get_resp (k_uj_render.hip), which sorts
// and renders them where they are.  The design notes are in k_uj_path.hip's
// header; as jy_get.hpp, this is kernels and host helpers in the anonymous
// namespace of each translation unit that includes it.
//
// The core takes the queries' slots as a DEVICE array (JY_NO_SLOT: no such
// key) and the checked paths in device memory, and leaves its result in
// device temporaries: the CSR over the queries and, per matched element, the
// handle, the leaf reference and its skip (the path's length).  No leaf byte
// is gathered: a reader takes them where LeafTailSrc does.
//   path_query_check  the host's check of every path, before any launch
//   path_select       sizes, match and scans; the totals on the host (two waits)
//   path_compact      the matches to their scanned positions, into arrays the
//                     caller names (its own outputs, or temporaries)
#pragma once

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
inline int32_t path_check(jy_engine* eng, const uint8_t* b, u64 a, u64 e) {
  while (a < e) {
    if (e - a < 4) return eng->fail(JY_EINVAL, "a path ends inside a segment's length word");
    const u64 len = (u64)b[a] | (u64)b[a + 1] << 8 | (u64)b[a + 2] << 16 | (u64)b[a + 3] << 24;
    if (len > kLeafMaxLen) return eng->fail(JY_ERANGE, "a path segment longer than 2^24 - 1 bytes");
    if (len > e - a - 4) return eng->fail(JY_EINVAL, "a path's last segment is cut short");
    a += 4 + len;
  }
  return JY_OK;
}

// the whole of a query's paths (host memory, n > 0), before any launch
inline int32_t path_query_check(jy_engine* eng, u64 n, const uint8_t* path_bytes, const u64* path_offs) {
  for (u64 i = 0; i < n; i++)
    if (path_offs[i + 1] < path_offs[i]) return eng->fail(JY_EINVAL, "path_offs is not ascending");
  if (path_offs[n] - path_offs[0] && !path_bytes) return eng->fail(JY_EINVAL, "path_bytes is null");
  for (u64 i = 0; i < n; i++) JY_TRY(path_check(eng, path_bytes, path_offs[i], path_offs[i + 1]));
  return JY_OK;
}

// the checked paths -> the device (the caller's arrays outlive the call's first
// wait).  *pb is based so that po's offsets, the caller's, index it.
inline int32_t path_stage(jy_engine* eng, Tmp& tmp, u64 n, const uint8_t* path_bytes, const u64* path_offs,
                          const uint8_t** pb, const u64** po) {
  const u64 first = path_offs[0], pbytes = path_offs[n] - first;
  uint8_t* db;
  u64* dp;
  JY_TRY(tmp.get(&db, pbytes));
  JY_TRY(tmp.get(&dp, n + 1));
  if (pbytes) JY_HIP(eng, hipMemcpyAsync(db, path_bytes + first, pbytes, hipMemcpyHostToDevice, eng->stream));
  JY_HIP(eng, hipMemcpyAsync(dp, path_offs, (n + 1) * 8, hipMemcpyHostToDevice, eng->stream));
  *pb = db - first;
  *po = dp;
  return JY_OK;
}

// what path_select leaves on the device (temporaries of the caller's Tmp) and,
// of its totals, on the host
struct PathSel {
  u64 n = 0;
  u64 me = 0;       // examined elements
  u64 m = 0;        // matched elements
  u64 bytes = 0;    // their relative leaf bytes (with_bytes)
  u64 missing = 0;  // examined elements whose handle is not in the leaf store
  u64 *eo = nullptr;                                  // [n + 1] over the examined elements
  u64 *he = nullptr, *flag = nullptr, *klen = nullptr, *lrs = nullptr;  // per examined element
  u64 *fo = nullptr, *lo = nullptr;                   // [me + 1] the scans of flag and klen
};

// sizes, match, scans.  `ds`: the n > 0 device slots; `holes`: some may be
// JY_NO_SLOT (at least one is not, and the type has keys).  me == 0 on return:
// no element was examined and nothing else was made.
inline int32_t path_select(jy_engine* eng, Tmp& tmp, u64 n, const u32* ds, bool holes, const uint8_t* pb,
                           const u64* po, bool with_bytes, PathSel& S) {
  const UjsonState& u = eng->ujson;
  const LeafStore& St = eng->leaf;
  S.n = n;
  const u32* dslots = ds;
  if (holes) {
    u32* fix;
    JY_TRY(tmp.get(&fix, n));
    LAUNCH(k_uj_path_holes, n, ds, n, fix, static_cast<u64*>(nullptr));
    dslots = fix;
  }
  // ---- the examined elements of every query ----
  u64 *se, *sc;
  JY_TRY(tmp.get(&se, n + 1));
  JY_TRY(tmp.get(&sc, n));
  JY_TRY(tmp.get(&S.eo, n + 1));
  JY_HIP(eng, hipMemsetAsync(se + n, 0, 8, eng->stream));
  JY_TRY(jy_ujson_sizes_of(eng, u, n, dslots, se, sc));
  if (holes) LAUNCH(k_uj_path_holes, n, ds, n, static_cast<u32*>(nullptr), se);
  JY_TRY(jy_scan_u64(eng, se, S.eo, n));
  JY_TRY(totals(eng, {S.eo + n}, &S.me));  // the first wait
  const u64 me = S.me;
  if (me == 0) return JY_OK;

  // ---- match, scan ----
  u64* miss;
  JY_TRY(tmp.get(&S.he, me));
  JY_TRY(tmp.get(&S.flag, me + 1));
  JY_TRY(tmp.get(&S.klen, me + 1));
  JY_TRY(tmp.get(&S.lrs, me));
  JY_TRY(tmp.get(&S.fo, me + 1));
  JY_TRY(tmp.get(&miss, 1));
  JY_HIP(eng, hipMemsetAsync(S.flag + me, 0, 8, eng->stream));
  JY_HIP(eng, hipMemsetAsync(S.klen + me, 0, 8, eng->stream));
  JY_HIP(eng, hipMemsetAsync(miss, 0, 8, eng->stream));
  const PathDocs D{u.meta, u.epool, u.lcol, u.lpe, u.R};
  const PathQueries Q{dslots, S.eo, pb, po, n};
  const PathLeaves L{St.tkey, St.tref, St.tcap ? St.tcap - 1 : 0, 64 - St.lg, St.bytes};
  LAUNCH(k_uj_path_match, me, D, Q, L, me, S.he, S.flag, S.klen, S.lrs, reinterpret_cast<unsigned long long*>(miss));
  JY_TRY(jy_scan_u64(eng, S.flag, S.fo, me));
  if (with_bytes) {
    JY_TRY(tmp.get(&S.lo, me + 1));
    JY_TRY(jy_scan_u64(eng, S.klen, S.lo, me));
  }
  u64 tot[3];
  JY_TRY(totals(eng, {S.fo + me, with_bytes ? S.lo + me : miss, miss}, tot));  // the second and last wait
  S.m = tot[0];
  S.bytes = with_bytes ? tot[1] : 0;
  S.missing = tot[2];
  return JY_OK;
}

// the matches of a select with me > 0, compacted: el_offs[n + 1], elems[m] and,
// for a select with_bytes, klr[m], skip[m], leaf_offs[m + 1] (else null)
inline int32_t path_compact(jy_engine* eng, const PathSel& S, u64* el_offs, u64* elems, u64* klr, u32* skip,
                            u64* leaf_offs) {
  LAUNCH(k_uj_path_offs, S.n + 1, S.eo, S.fo, S.n, el_offs);
  LAUNCH(k_uj_path_compact, S.me + 1, S.me, S.flag, S.fo, S.lo, S.he, S.klen, S.lrs, elems, klr, skip, leaf_offs);
  return JY_OK;
}

}  // namespace
