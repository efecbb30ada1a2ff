// k_state_digest.hip -- the canonical digest of a slot range's STATE, split
// into key-hash buckets (jy_*_state_digest), and the slots of named buckets
// (jy_state_bucket_slots).  With the slot-list dumps (jy_*_state_wire_slots,
// k_state_wire.hip) this is anti-entropy without shipping everything: compare
// bucket digests with a peer, select the slots of the buckets that differ,
// dump only those as a converge batch.
//
// The digest of a range IS the digest of its jy_*_state_wire dump
// (jy_digest.hpp): every slot of the range is a key, bottom state included.
// out[B][4] = per bucket {digest, keys, items, bytes-or-cloud}, overwritten.
//
//   k_digest_keyhash   a lane per slot: FNV-1a over the key's bytes (serial, a
//                      word per load through kref, bytes unsigned), kh and the
//                      bucket into temporaries of the call.  Nothing is cached
//                      in the engine: the call is read-only.
//   k_digest_cnt       a lane per slot walks the slab's rows in place:
//                      consecutive lanes read consecutive slots of one row
//                      (the access shape of k_state_cnt_count).
//   k_digest_treg      a lane per slot reads ts and the 16-B handle in place;
//                      values of up to 8 bytes are hashed from the handle's
//                      prefix, longer ones from the arena.
//   TLOG, UJSON        the record readers of the wire forms over the state
//                      (jy_wire.hpp: sel_slots, tlog_sizing / _entries,
//                      ujson_sizing / _entries) fill temporaries; then a lane
//                      per ITEM (entry, element, dense vv word, cloud dot), its
//                      key from an id fill (jy_seg_ids), and a lane per key for
//                      the key's own term.  A 300-entry log is 300 lanes.
//
// Accumulation (Acc): integer adds commute, so any order is exact.  Up to
// kWaveBuckets buckets every bucket's four words are summed over the wave
// first (one atomic per wave, bucket and word).  Up to kLdsBuckets buckets a
// workgroup accumulates in LDS and flushes its non-zero words with global
// 64-bit atomic adds; above that lanes add to global memory directly (buckets
// >> lanes: little contention).  Measured ("State digest and bucket
// repair"; tools/state_digest_time.py switches the forms with JY_DIGEST_ACC):
// at B = 1 the LDS stage is 1.7x to 12x faster than wave-reduced global
// atomics.  Rows for 4,096 buckets (128 KB: one workgroup a CU) win for TREG
// but lose 2.4x for the counters, whose slab 256 workgroups cannot stream, so
// the stage ends at 1,024 buckets, where B = 4096 runs the direct form.

#include <cstdlib>
#include <cstring>

#include "jy_digest.hpp"
#include "jy_dscan.hpp"
#include "jy_wire.hpp"

namespace {

using namespace jydigest;

constexpr u32 kWaveBuckets = 4;     // up to here: wave sums per bucket
constexpr u32 kLdsBuckets = 1024;   // up to here: per-workgroup rows in LDS (32 KB; the A/B above)
constexpr u32 kMaxBlocks = 2048;    // grid-stride: a workgroup's LDS rows are flushed once
constexpr u32 kLdsPlain = 64 << 10; // dynamic LDS a kernel may use without raising its limit
constexpr u32 kBigLdsBlocks = 256;  // workgroups of a launch whose rows exceed kLdsPlain (one a CU)

struct Acc {
  u64* out;   // [B][4], zero before the first kernel of the call
  u32 B;
  bool lds;
};

extern __shared__ u64 acc_rows[];

__device__ __forceinline__ void acc_init(const Acc& A) {
  if (A.lds) {
    for (u32 q = threadIdx.x; q < A.B * 4; q += kThreads) acc_rows[q] = 0;
    __syncthreads();
  }
}
__device__ __forceinline__ u64 wave_sum(u64 x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}
// every thread of the workgroup calls this together (valid = it has a term)
__device__ __forceinline__ void acc_add(const Acc& A, bool valid, u32 b, u64 d, u64 keys, u64 items, u64 w3) {
  u64* dst = A.lds ? acc_rows : A.out;
  const u64 v[4] = {d, keys, items, w3};
  if (A.B <= kWaveBuckets) {
    for (u32 bb = 0; bb < A.B; bb++) {
      const bool mine = valid && b == bb;
      if (__ballot(mine) == 0) continue;  // wave-uniform
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const u64 x = wave_sum(mine ? v[q] : 0);
        if (__lane_id() == 0 && x) atomicAdd(reinterpret_cast<unsigned long long*>(dst + bb * 4 + q), (unsigned long long)x);
      }
    }
  } else if (valid) {
#pragma unroll
    for (int q = 0; q < 4; q++)
      if (v[q]) atomicAdd(reinterpret_cast<unsigned long long*>(dst + (u64)b * 4 + q), (unsigned long long)v[q]);
  }
}
__device__ __forceinline__ void acc_flush(const Acc& A) {
  if (!A.lds) return;
  __syncthreads();
  for (u32 q = threadIdx.x; q < A.B * 4; q += kThreads) {
    const u64 x = acc_rows[q];
    if (x) atomicAdd(reinterpret_cast<unsigned long long*>(A.out + q), (unsigned long long)x);
  }
}

// one lane's term of the digest
struct Term {
  u32 b = 0;  // bucket
  u64 d = 0, keys = 0, items = 0, w3 = 0;
};
// a kernel's body over n items: f(j, term) for every item, grid-stride with a
// trip count uniform over the workgroup (acc_add shuffles)
template <class F>
__device__ __forceinline__ void digest_loop(const Acc& A, u64 n, F f) {
  acc_init(A);
  for (u64 base = (u64)blockIdx.x * kThreads; base < n; base += (u64)gridDim.x * kThreads) {
    const u64 j = base + threadIdx.x;
    const bool valid = j < n;
    Term t;
    if (valid) f(j, t);
    acc_add(A, valid, t.b, t.d, t.keys, t.items, t.w3);
  }
  acc_flush(A);
}

// FNV-1a steps over the low m bytes of w (byte 0 first)
__device__ __forceinline__ u64 fnv_word(u64 h, u64 w, u32 m) {
  for (u32 q = 0; q < m; q++) {
    h ^= (w >> (8 * q)) & 0xFFu;
    h *= kFnvPrime;
  }
  return h;
}
// dbytes over memory at any alignment, a word per load (jy_ld8u)
__device__ __forceinline__ u64 dbytes_mem(const uint8_t* p, u64 len) {
  u64 h = kFnvBasis;
  for (u64 i = 0; i < len; i += 8) {
    const u32 m = (u32)(len - i < 8 ? len - i : 8);
    h = fnv_word(h, jy_ld8u(p + i, m), m);
  }
  return dbytes_end(h, len);
}
// dbytes of a value handle: up to 8 bytes live in pre (big-endian, zero-padded)
__device__ __forceinline__ u64 dbytes_value(u64 pre, u64 lr, const uint8_t* __restrict__ arena) {
  const u64 len = lr & JY_LR_LEN_MASK;
  if (len <= 8) return dbytes_end(fnv_word(kFnvBasis, __builtin_bswap64(pre), (u32)len), len);
  return dbytes_mem(arena + (lr >> JY_LR_LEN_BITS), len);
}

// kh[j], bk[j] of slot slot0 + j
__global__ __launch_bounds__(kThreads) void k_digest_keyhash(const uint8_t* __restrict__ bytes,
                                                             const u64* __restrict__ kref, u64 slot0, u64 n, u32 lg,
                                                             u64* __restrict__ kh, u32* __restrict__ bk) {
  const u64 j = gid();
  if (j >= n) return;
  const u64 kr = kref[slot0 + j];
  const u64 h = dbytes_mem(bytes + (kr >> JY_LR_LEN_BITS), kr & JY_LR_LEN_MASK);
  kh[j] = h;
  bk[j] = bucket(h, lg);
}

__global__ __launch_bounds__(kThreads) void k_digest_cnt(Slab S, const u64* __restrict__ ids, u64 slot0, u64 n,
                                                         const u64* __restrict__ kh, const u32* __restrict__ bk,
                                                         Acc A) {
  digest_loop(A, n, [&](u64 j, Term& t) {
    const u64 s = slot0 + j, h = kh[j];
    t.b = bk[j];
    t.d = d_cnt(h);
    t.keys = 1;
#pragma unroll 4
    for (u32 r = 0; r < S.rows; r++) {
      const u64 v = S.row(r)[s];
      if (v) {
        const u32 sg = r >= S.ncols ? 1u : 0u;
        t.d += d_cell(h, sg, ids[r - sg * S.ncols], v);
        t.items++;
        t.w3 += v;
      }
    }
  });
}

__global__ __launch_bounds__(kThreads) void k_digest_treg(const u64* __restrict__ ts, const TVal* __restrict__ val,
                                                          const uint8_t* __restrict__ arena, u64 slot0, u64 n,
                                                          const u64* __restrict__ kh, const u32* __restrict__ bk,
                                                          Acc A) {
  digest_loop(A, n, [&](u64 j, Term& t) {
    const u64 s = slot0 + j;
    const TVal v = val[s];
    t.b = bk[j];
    t.d = d_reg(kh[j], ts[s], dbytes_value(v.pre, v.lr, arena));
    t.keys = t.items = 1;
    t.w3 = v.lr & JY_LR_LEN_MASK;
  });
}

// the key's own term of a TLOG (d_log of its cutoff) or a UJSON document (cut == nullptr)
__global__ __launch_bounds__(kThreads) void k_digest_keyterm(const u64* __restrict__ cut, u64 n,
                                                             const u64* __restrict__ kh, const u32* __restrict__ bk,
                                                             Acc A) {
  digest_loop(A, n, [&](u64 j, Term& t) {
    t.b = bk[j];
    t.d = cut ? d_log(kh[j], cut[j]) : d_doc(kh[j]);
    t.keys = 1;
  });
}

// TLOG entries, newest first per key (the gather's order): rank = position in the key's run
__global__ __launch_bounds__(kThreads) void k_digest_ent(const u32* __restrict__ seg, const u64* __restrict__ eoff,
                                                         const u64* __restrict__ ts, const u64* __restrict__ pre,
                                                         const u64* __restrict__ lr,
                                                         const uint8_t* __restrict__ arena, u64 m,
                                                         const u64* __restrict__ kh, const u32* __restrict__ bk,
                                                         Acc A) {
  digest_loop(A, m, [&](u64 j, Term& t) {
    const u32 i = seg[j];
    const u64 l = lr[j];
    t.b = bk[i];
    t.d = d_ent(kh[i], j - eoff[i], ts[j], dbytes_value(pre[j], l, arena));
    t.items = 1;
    t.w3 = l & JY_LR_LEN_MASK;
  });
}

// UJSON elements (elems != nullptr) or cloud dots, packed col << 48 | seq
__global__ __launch_bounds__(kThreads) void k_digest_dots(const u32* __restrict__ seg, const u64* __restrict__ dots,
                                                          const u64* __restrict__ elems,
                                                          const u64* __restrict__ ids, u32 nids, u64 m,
                                                          const u64* __restrict__ kh, const u32* __restrict__ bk,
                                                          Acc A) {
  digest_loop(A, m, [&](u64 j, Term& t) {
    const u32 i = seg[j];
    const u64 dot = dots[j], c = dot >> JY_DOT_SEQ_BITS, seq = dot & JY_DOT_SEQ_MASK;
    const u64 id = c < nids ? ids[c] : 0;  // (every stored column is registered)
    t.b = bk[i];
    if (elems) {
      t.d = d_el(kh[i], id, seq, elems[j]);
      t.items = 1;
    } else {
      t.d = d_cl(kh[i], id, seq);
      t.w3 = 1;
    }
  });
}

// the dense version vectors [n][R]: a lane per word, zero entries contribute nothing
__global__ __launch_bounds__(kThreads) void k_digest_vv(const u64* __restrict__ dense, u32 R,
                                                        const u64* __restrict__ ids, u32 nids, u64 n,
                                                        const u64* __restrict__ kh, const u32* __restrict__ bk,
                                                        Acc A) {
  const u64 m = n * R;
  digest_loop(A, m, [&](u64 j, Term& t) {
    const u64 i = j / R, c = j - i * R, x = dense[j];
    t.b = bk[i];
    if (x && c < nids) t.d = d_vv(kh[i], ids[c], x);
  });
}

__global__ __launch_bounds__(kThreads) void k_bucket_add(u32* __restrict__ slots, u64 n, u32 slot0) {
  const u64 j = gid();
  if (j < n) slots[j] += slot0;
}

struct BucketPred {
  const u32* bk;
  const u64* bits;
  __device__ __forceinline__ bool operator()(u64 i) const {
    const u32 b = bk[i];
    return ((bits[b >> 6] >> (b & 63)) & 1) != 0;
  }
};

// buckets up to which a workgroup accumulates in LDS.  JY_DIGEST_ACC in the
// environment (read at each call; the A/B of tools/state_digest_time.py):
// "global" = never, "lds1k" = up to 1,024 rows (32 KB, the default), "lds4k" =
// up to 4,096 rows (128 KB, one workgroup a CU: the arm that lost)
u32 lds_rows() {
  const char* v = std::getenv("JY_DIGEST_ACC");
  if (v && std::strcmp(v, "global") == 0) return 0;
  if (v && std::strcmp(v, "lds1k") == 0) return 1024;
  if (v && std::strcmp(v, "lds4k") == 0) return 4096;
  return kLdsBuckets;
}

int32_t buckets_check(jy_engine* eng, u32 B, u32* lg) {
  if (B == 0 || (B & (B - 1)) != 0 || B > (1u << kMaxBucketsLog2))
    return eng->fail(JY_EINVAL, "nbuckets must be a power of two between 1 and 2^20");
  *lg = (u32)__builtin_ctz(B);
  return JY_OK;
}

// one digest call: the output rows (zeroed), the key hashes and buckets of the range
struct Call {
  jy_engine* eng;
  Tmp tmp;
  Acc A{};
  u64* user = nullptr;
  int32_t mem = JY_HOST;
  u64* kh = nullptr;
  u32* bk = nullptr;
  explicit Call(jy_engine* e) : eng(e), tmp(e) {}

  // JY_OK with *empty set: nslots == 0, out is all zero already
  int32_t begin(int32_t type, u64 slot0, u64 n, u32 B, u64* out, int32_t m, bool* empty) {
    u32 lg;
    mem = m;
    user = out;
    JY_TRY(mem_check(eng, mem));
    JY_TRY(buckets_check(eng, B, &lg));
    JY_TRY(range_check(eng, type, slot0, n));
    *empty = n == 0;
    if (n == 0) {
      if (mem == JY_DEVICE) JY_HIP(eng, hipMemsetAsync(out, 0, (u64)B * 32, eng->stream));
      else std::memset(out, 0, (u64)B * 32);
      return JY_OK;
    }
    A.B = B;
    A.lds = B <= lds_rows();
    JY_TRY(tmp.out(&A.out, out, (u64)B * 4, mem));
    JY_HIP(eng, hipMemsetAsync(A.out, 0, (u64)B * 32, eng->stream));
    JY_TRY(tmp.get(&kh, n));
    JY_TRY(tmp.get(&bk, n));
    const KeyDir& D = eng->kdir[type];
    LAUNCH(k_digest_keyhash, n, D.bytes, D.kref, slot0, n, lg, kh, bk);
    return JY_OK;
  }
  int32_t end() {
    JY_TRY(emit(eng, mem, user, A.out, (u64)A.B * 32));
    if (mem == JY_HOST) JY_HIP(eng, hipStreamSynchronize(eng->stream));
    return JY_OK;
  }
  // the replica id of every column, uploaded for this call (pinned staging:
  // the host table may grow while the copy is in flight)
  int32_t ids(const u64** dev, u32* n) {
    *n = (u32)eng->rep_id.size();
    u64* d;
    JY_TRY(tmp.get(&d, std::max<u32>(*n, 1)));
    if (*n) {
      JY_TRY(jy_stage_begin(eng));
      const void* staged = nullptr;
      JY_TRY(jy_stage(eng, 0, eng->rep_id.data(), (u64)*n * 8, JY_HOST, &staged));
      JY_HIP(eng, hipMemcpyAsync(d, staged, (u64)*n * 8, hipMemcpyDeviceToDevice, eng->stream));
      JY_TRY(jy_stage_end(eng));
    }
    *dev = d;
    return JY_OK;
  }
};

// launch a digest kernel over n items
#define DIGEST(call, k, n, ...)                                                                          \
  do {                                                                                                   \
    if ((n) > 0) {                                                                                       \
      const u32 lds_ = (call).A.lds ? (call).A.B * 32 : 0;                                              \
      /* above 64 KB of rows one workgroup fits a CU: one each, and the kernel's limit raised */       \
      if (lds_ > kLdsPlain)                                                                              \
        JY_HIP(eng, hipFuncSetAttribute(reinterpret_cast<const void*>(k),                               \
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_));        \
      const u32 nb_ = std::min<u32>(blocks_for(n), lds_ > kLdsPlain ? kBigLdsBlocks : kMaxBlocks);      \
      hipLaunchKernelGGL(k, dim3(nb_), dim3(kThreads), lds_, eng->stream, \
                         __VA_ARGS__, (call).A);                                                         \
      JY_HIP(eng, hipGetLastError());                                                                    \
    }                                                                                                    \
  } while (0)

}  // namespace

extern "C" {

int32_t jy_counter_state_digest(jy_engine* eng, int32_t type, uint64_t slot0, uint64_t nslots, uint32_t nbuckets,
                                uint64_t* out, int32_t mem) {
  JY_HIP(eng, hipSetDevice(eng->device));
  if (type != JY_GCOUNT && type != JY_PNCOUNT) return eng->fail(JY_ETYPE, "not a counter type");
  Call c(eng);
  bool empty;
  JY_TRY(c.begin(type, slot0, nslots, nbuckets, out, mem, &empty));
  if (empty) return JY_OK;
  const int w = type == JY_GCOUNT ? 0 : 1;
  const CounterState& cs = eng->cnt[w];
  // columns past the slab's capacity were never written: all zero, no cells
  const u32 ncols = std::min<u32>((u32)eng->rep_id.size(), cs.ccap);
  const Slab S{cs.slab, cs.kcap, (u64)cs.ccap * cs.kcap, ncols, (u32)(w + 1) * ncols};
  const u64* ids;
  u32 nids;
  JY_TRY(c.ids(&ids, &nids));
  DIGEST(c, k_digest_cnt, nslots, S, ids, slot0, nslots, c.kh, c.bk);
  return c.end();
}

int32_t jy_treg_state_digest(jy_engine* eng, uint64_t slot0, uint64_t nslots, uint32_t nbuckets, uint64_t* out,
                             int32_t mem) {
  JY_HIP(eng, hipSetDevice(eng->device));
  Call c(eng);
  bool empty;
  JY_TRY(c.begin(JY_TREG, slot0, nslots, nbuckets, out, mem, &empty));
  if (empty) return JY_OK;
  // entries of slots named twice in one launch wait in a list: fold them in
  // first, as every TREG state read does (jy_treg_gather)
  JY_TRY(jy_treg_fold(eng));
  const TregState& t = eng->treg;
  DIGEST(c, k_digest_treg, nslots, t.ts, t.val, eng->arena[JY_TREG].p, slot0, nslots, c.kh, c.bk);
  JY_TRY(c.end());
  return jy_treg_overflow_check(eng);
}

int32_t jy_tlog_state_digest(jy_engine* eng, uint64_t slot0, uint64_t nslots, uint32_t nbuckets, uint64_t* out,
                             int32_t mem) {
  JY_HIP(eng, hipSetDevice(eng->device));
  Call c(eng);
  bool empty;
  JY_TRY(c.begin(JY_TLOG, slot0, nslots, nbuckets, out, mem, &empty));
  if (empty) return JY_OK;
  JY_TRY(jy_tlog_settle(eng));
  const u64 n = nslots;
  Tmp& tmp = c.tmp;
  u32* slots;
  TlogRecs R;
  JY_TRY(sel_slots(eng, tmp, JY_TLOG, Sel::range(slot0, n), &slots));
  JY_TRY(tlog_sizing(eng, tmp, eng->tlog, slots, n, R));
  JY_TRY(totals(eng, {R.eoff + n}, &R.m));
  const u64 m = R.m;
  DIGEST(c, k_digest_keyterm, n, (const u64*)R.cuts, n, c.kh, c.bk);
  if (m) {
    u32* seg;
    JY_TRY(tmp.get(&seg, m));
    JY_TRY(tlog_entries(eng, tmp, eng->tlog, slots, n, R));
    JY_TRY(jy_seg_ids(eng, R.eoff, n, m, seg));
    DIGEST(c, k_digest_ent, m, seg, R.eoff, R.ts, R.pre, R.lr, eng->arena[JY_TLOG].p, m, c.kh, c.bk);
  }
  return c.end();
}

int32_t jy_ujson_state_digest(jy_engine* eng, uint64_t slot0, uint64_t nslots, uint32_t nbuckets, uint64_t* out,
                              int32_t mem) {
  JY_HIP(eng, hipSetDevice(eng->device));
  Call c(eng);
  bool empty;
  JY_TRY(c.begin(JY_UJSON, slot0, nslots, nbuckets, out, mem, &empty));
  if (empty) return JY_OK;
  const u64 n = nslots;
  const UjsonState& u = eng->ujson;
  Tmp& tmp = c.tmp;
  u32* slots;
  UjsonRecs D;
  JY_TRY(sel_slots(eng, tmp, JY_UJSON, Sel::range(slot0, n), &slots));
  JY_TRY(ujson_sizing(eng, tmp, u, slots, n, D));
  u64 tot[2];
  JY_TRY(totals(eng, {D.eo + n, D.co + n}, tot));
  const u64 me = D.me = tot[0], mc = D.mc = tot[1];
  JY_TRY(ujson_entries(eng, tmp, u, slots, n, D));
  const u64* ids;
  u32 nids;
  JY_TRY(c.ids(&ids, &nids));
  const u64* none = nullptr;
  DIGEST(c, k_digest_keyterm, n, none, n, c.kh, c.bk);
  DIGEST(c, k_digest_vv, n * u.R, (const u64*)D.dense, u.R, ids, nids, n, c.kh, c.bk);
  if (me || mc) {
    u32* seg;
    JY_TRY(tmp.get(&seg, std::max(me, mc)));
    if (me) {
      JY_TRY(jy_seg_ids(eng, D.eo, n, me, seg));
      DIGEST(c, k_digest_dots, me, seg, (const u64*)D.dots, (const u64*)D.elems, ids, nids, me, c.kh, c.bk);
    }
    if (mc) {
      JY_TRY(jy_seg_ids(eng, D.co, n, mc, seg));
      DIGEST(c, k_digest_dots, mc, seg, (const u64*)D.cloud, none, ids, nids, mc, c.kh, c.bk);
    }
  }
  return c.end();
}

int32_t jy_state_bucket_slots(jy_engine* eng, int32_t type, uint64_t slot0, uint64_t nslots, uint32_t nbuckets,
                              const uint64_t* bucket_bits, uint64_t cap, uint32_t* slots_out, uint64_t* n_out,
                              int32_t mem) {
  JY_HIP(eng, hipSetDevice(eng->device));
  *n_out = 0;
  if (type < 0 || type >= JY_NTYPES) return eng->fail(JY_ETYPE, "unknown CRDT type");
  u32 lg;
  JY_TRY(mem_check(eng, mem));
  JY_TRY(buckets_check(eng, nbuckets, &lg));
  JY_TRY(range_check(eng, type, slot0, nslots));
  const u64 n = nslots;
  if (n == 0) return JY_OK;
  Tmp tmp(eng);
  u64 *kh, *bits, *cnt;
  u32 *bk, *sel;
  const u64 words = ((u64)nbuckets + 63) / 64;
  JY_TRY(tmp.get(&kh, n));
  JY_TRY(tmp.get(&bk, n));
  JY_TRY(tmp.get(&sel, n));
  JY_TRY(tmp.get(&bits, words));
  JY_TRY(tmp.get(&cnt, 1));
  JY_TRY(jy_stage_begin(eng));
  const void* staged = nullptr;
  JY_TRY(jy_stage(eng, 0, bucket_bits, words * 8, JY_HOST, &staged));
  JY_HIP(eng, hipMemcpyAsync(bits, staged, words * 8, hipMemcpyDeviceToDevice, eng->stream));
  JY_TRY(jy_stage_end(eng));
  JY_HIP(eng, hipMemsetAsync(cnt, 0, 8, eng->stream));
  const KeyDir& D = eng->kdir[type];
  LAUNCH(k_digest_keyhash, n, D.bytes, D.kref, slot0, n, lg, kh, bk);
  // flag, scan, select in one pass (jy_dscan.hpp): positions in the range, ascending
  JY_TRY(jydscan::select(eng, n, BucketPred{bk, bits}, sel, reinterpret_cast<u32*>(cnt)));
  u64 k = 0;
  JY_TRY(totals(eng, {cnt}, &k));
  *n_out = k;
  if (cap < k || k == 0) return JY_OK;  // the count only
  LAUNCH(k_bucket_add, k, sel, k, (u32)slot0);
  JY_TRY(emit(eng, mem, slots_out, sel, k * 4));
  if (mem == JY_HOST) JY_HIP(eng, hipStreamSynchronize(eng->stream));
  return JY_OK;
}

}  // extern "C"
