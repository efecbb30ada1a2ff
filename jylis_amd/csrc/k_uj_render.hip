// k_uj_render.hip -- UJSON GET as RESP reply bytes, rendered on the GPU
// (jy_ujson_get_resp).
//
// The other types answer a keyed GET on the device (k_resp.hip); a UJSON GET
// selected its leaves there (k_uj_path.hip) and then copied every one to the
// host to be decoded, put into a tree and printed.  Here the text is written
// where the leaves are.  The rules -- the order, the text a leaf owns, the
// ancestor mask -- are jy_uj_render.hpp, which the host runs too.
//
//   path core        jy_uj_path.hpp: slots from the key strings (query_slots),
//                    sizes, match, scans, compact.  Leaves the CSR over the
//                    queries and per match (leaf reference, skip): no leaf byte
//                    is gathered, every later step reads a leaf where
//                    LeafTailSrc would.
//   order            a merge sort of the match indices by (query, relative
//                    leaf bytes): ceil(log2 m) launches of k_uj_merge, in each
//                    of which a lane finds its rank in the sibling run by a
//                    bisection (lower bound from the left run, upper bound from
//                    the right: stable).  A lane makes at most log2 m leaf
//                    compares a round and never walks a document's leaves; a
//                    compare runs over lengths the leaf store checked at put.
//                    jy_sort.hpp's radix sort was not used: in rounds over a
//                    few leaf bytes it needs (bytes of the longest tie) / 3
//                    rounds of 5+ passes each, and keys of 256 bytes are in
//                    the tests.
//   de-duplicate     k_uj_heads_of flags a leaf that differs from its
//                    predecessor, one scan, k_uj_uniq compacts
//   structure        k_uj_shape: per distinct leaf its depth, the segments it
//                    shares with its predecessor, and whether the device
//                    renders it (else on_host[query] = 1).  Then the ancestor
//                    mask, an inclusive right-to-left composition.  jy_dscan.hpp
//                    is NOT used for it: its wave_incl applies op(later,
//                    earlier) and k_scan_part reduces lanes' strided items by
//                    xor shuffles, so it assumes a commutative operator, and
//                    mask_compose is not one.  k_uj_mask_* below is the same
//                    reduce-then-scan with every combine in order.
//   pieces           k_uj_count runs leaf_text to count a leaf's pieces and
//                    text bytes; two scans place them; k_uj_pieces runs it
//                    again to write (length, reference) per piece, k_uj_qpieces
//                    the `$<len>\r\n` head and `\r\n` tail of every query
//   write            ONE scan over the piece lengths (piece offsets, and
//                    reply_offs at the heads), then k_wire_gather with
//                    RenderSrc: key and value bytes are pointer pieces into the
//                    leaf arena, punctuation is inline in the reference, the
//                    closers and the head are generated (jy_resp.hpp's gen8)
//
// Waits: the path core's two, the piece count, the reply total.
//
// Roofline: latency-bound, as the keyed reads.  Per matched leaf: 8 + 4 + 4
// bytes of (reference, skip, query) written once and read by every sort round
// through a 4-byte index; per distinct leaf its bytes read four times (shape,
// count, pieces, gather) and 2 keys + 3 pieces of 16 bytes written; per reply
// byte one byte written once.  Times: DESIGN.md, "UJSON replies".

#include <algorithm>
#include <cstring>

#include "jy_get.hpp"
#include "jy_resp.hpp"
#include "jy_uj_path.hpp"
#include "jy_uj_render.hpp"

namespace {

using jyuj::kRenderDepth;
static_assert(kRenderDepth == JY_UJSON_RENDER_DEPTH, "the header states the depth the rules render");

struct DevLeaf {  // a leaf's bytes from any byte address (jy_ld8u)
  const uint8_t* p;
  __device__ __forceinline__ u64 operator()(u64 i, u64 m) const { return jy_ld8u(p + i, m); }
};

struct Matches {  // the path core's result, compacted
  const uint8_t* arena;
  const u64* klr;   // per match: the stored leaf
  const u32* skip;  // ... and where its relative encoding starts
  const u32* qid;   // ... and its query
  __device__ __forceinline__ DevLeaf leaf(u64 t) const { return DevLeaf{arena + (klr[t] >> JY_LR_LEN_BITS) + skip[t]}; }
  __device__ __forceinline__ u64 len(u64 t) const { return (klr[t] & JY_LR_LEN_MASK) - skip[t]; }
  // (query, relative leaf bytes), a proper prefix first
  __device__ __forceinline__ int cmp(u64 a, u64 b) const {
    const u32 qa = qid[a], qb = qid[b];
    if (qa != qb) return qa < qb ? -1 : 1;
    return jyuj::leaf_cmp(leaf(a), len(a), leaf(b), len(b));
  }
};

// qid[t] = the query of match t < m: el_offs[q] <= t < el_offs[q + 1]
__global__ __launch_bounds__(kThreads) void k_uj_qid(const u64* __restrict__ el_offs, u64 n, u64 m,
                                                     u32* __restrict__ qid) {
  __shared__ u64 ends[2];
  const u64 t0 = (u64)blockIdx.x * kThreads;
  if (t0 >= m) return;
  const u64 t1 = std::min<u64>(t0 + kThreads, m);
  const auto at = [&](u64 j) { return el_offs[j]; };
  if (threadIdx.x < 2) ends[threadIdx.x] = item_of(at, 0, n, threadIdx.x == 0 ? t0 : t1 - 1);
  __syncthreads();
  const u64 t = t0 + threadIdx.x;
  if (t < t1) qid[t] = (u32)item_of(at, ends[0], ends[1] + 1, t);
}

// one round of the merge sort: runs of w sorted indices in src (null: the
// identity) merge pairwise into dst
__global__ __launch_bounds__(kThreads) void k_uj_merge(Matches M, u64 m, u64 w, const u32* __restrict__ src,
                                                       u32* __restrict__ dst) {
  const u64 i = gid();
  if (i >= m) return;
  const auto at = [&](u64 j) { return src ? (u64)src[j] : j; };
  const u64 base = i / (2 * w) * (2 * w);
  const u64 mid = std::min(base + w, m), end = std::min(base + 2 * w, m);
  const u64 x = at(i);
  const bool left = i < mid;
  // the elements of the sibling run that sort before x: strictly less for a
  // left element, less or equal for a right one
  u64 lo = left ? mid : base, hi = left ? end : mid;
  while (lo < hi) {
    const u64 c = lo + (hi - lo) / 2;
    const int r = M.cmp(at(c), x);
    if (left ? r < 0 : r <= 0) lo = c + 1;
    else hi = c;
  }
  dst[left ? i + (lo - mid) : (i - mid) + lo] = (u32)x;
}

// head[i] = sorted match i starts a distinct leaf of its query; lane m closes the scan's input
__global__ __launch_bounds__(kThreads) void k_uj_heads_of(Matches M, u64 m, const u32* __restrict__ perm,
                                                          u64* __restrict__ head) {
  const u64 i = gid();
  if (i > m) return;
  head[i] = i == m ? 0 : i == 0 ? 1 : M.cmp(perm[i - 1], perm[i]) != 0 ? 1 : 0;
}

// the distinct leaves, in order: a reference each, and the CSR over the queries
struct Uniq {
  u64* lr;
  u32* skip;
  u32* q;
};
__global__ __launch_bounds__(kThreads) void k_uj_uniq(Matches M, u64 m, const u32* __restrict__ perm,
                                                      const u64* __restrict__ head, const u64* __restrict__ ho,
                                                      Uniq U) {
  const u64 i = gid();
  if (i >= m || !head[i]) return;
  const u64 j = ho[i], t = perm[i];
  U.lr[j] = M.klr[t];
  U.skip[j] = M.skip[t];
  U.q[j] = M.qid[t];
}
// uo[q] = distinct leaves before query q's (a query keeps its positions through the sort)
__global__ __launch_bounds__(kThreads) void k_uj_uoffs(const u64* __restrict__ el_offs, const u64* __restrict__ ho,
                                                       u64 n, u64* __restrict__ uo) {
  const u64 q = gid();
  if (q <= n) uo[q] = ho[el_offs[q]];
}

struct Leaves {  // the distinct leaves
  const uint8_t* arena;
  const u64* lr;
  const u32* skip;
  const u32* q;
  const u64* count;  // -> how many there are (on the device)
  __device__ __forceinline__ u64 off(u64 j) const { return (lr[j] >> JY_LR_LEN_BITS) + skip[j]; }
  __device__ __forceinline__ DevLeaf leaf(u64 j) const { return DevLeaf{arena + off(j)}; }
  __device__ __forceinline__ u64 len(u64 j) const { return (lr[j] & JY_LR_LEN_MASK) - skip[j]; }
};

// shape word: depth | cp << 8 | first << 16 | bad << 17
constexpr u32 kShFirst = 1u << 16, kShBad = 1u << 17;
__global__ __launch_bounds__(kThreads) void k_uj_shape(Leaves L, u32* __restrict__ shape,
                                                       uint8_t* __restrict__ on_host) {
  const u64 j = gid();
  if (j >= *L.count) return;
  const jyuj::Shape s = jyuj::leaf_shape(L.leaf(j), L.len(j));
  const bool first = j == 0 || L.q[j - 1] != L.q[j];
  u32 cp = 0;
  if (!first) cp = jyuj::common_segments(L.leaf(j - 1), L.len(j - 1), L.leaf(j), L.len(j), kRenderDepth + 1);
  shape[j] = s.depth | (cp << 8) | (first ? kShFirst : 0u) | (s.bad ? kShBad : 0u);
  if (s.bad) on_host[L.q[j]] = 1;
}

// ---- the ancestor mask: an ordered inclusive scan from the right ----
// Scan position s is leaf u - 1 - s.  A workgroup takes kMaskTile consecutive
// positions, a lane kMaskPer consecutive ones; every combine is
// mask_compose(what lies to the right, what lies to the left).
constexpr int kMaskPer = 4;
constexpr u64 kMaskTile = (u64)kThreads * kMaskPer;

struct MaskIn {
  const u32* shape;
  u64 u;
  // the (keep, set) pair of scan position s < u
  __device__ __forceinline__ u64 operator()(u64 s) const {
    const u64 j = u - 1 - s;
    const u32 sh = shape[j];
    const bool last = j + 1 == u || (shape[j + 1] & kShFirst);
    // the reset at a query's end: the last leaf keeps nothing
    return jyuj::mask_elem(sh & 0xFFu, last, last ? 0u : (shape[j + 1] >> 8) & 0xFFu);
  }
};

__device__ __forceinline__ u64 mask_wave_incl(u64 x) {
  const int lane = __lane_id();
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u64 y = __shfl_up(x, o);  // the lanes before: to the right
    if (lane >= o) x = jyuj::mask_compose(y, x);
  }
  return x;
}
// exclusive over the workgroup, in thread order; every thread gets the total
__device__ __forceinline__ u64 mask_block_excl(u64 x, u64* lds, u64& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const u64 inc = mask_wave_incl(x);
  if (lane == 63) lds[w] = inc;
  __syncthreads();
  u64 off = jyuj::kMaskId, tot = jyuj::kMaskId;
#pragma unroll
  for (int i = 0; i < kThreads / 64; i++) {
    const u64 v = lds[i];
    if (i < w) off = jyuj::mask_compose(off, v);
    tot = jyuj::mask_compose(tot, v);
  }
  __syncthreads();
  total = tot;
  const u64 ex = __shfl_up(inc, 1);
  return lane == 0 ? off : jyuj::mask_compose(off, ex);
}

__global__ __launch_bounds__(kThreads) void k_uj_mask_part(const u32* __restrict__ shape, const u64* __restrict__ count,
                                                           u64* __restrict__ part) {
  __shared__ u64 lds[kThreads / 64];
  const MaskIn in{shape, *count};
  const u64 s0 = (u64)blockIdx.x * kMaskTile + (u64)threadIdx.x * kMaskPer;
  u64 x = jyuj::kMaskId;
#pragma unroll
  for (int k = 0; k < kMaskPer; k++)
    if (s0 + k < in.u) x = jyuj::mask_compose(x, in(s0 + k));
  u64 tot;
  mask_block_excl(x, lds, tot);
  if (threadIdx.x == 0) part[blockIdx.x] = tot;
}
// one workgroup: the nb tile totals -> what lies to the right of each tile
__global__ __launch_bounds__(kThreads) void k_uj_mask_mid(u64 nb, u64* __restrict__ part) {
  __shared__ u64 lds[kThreads / 64];
  u64 carry = jyuj::kMaskId;
  for (u64 b0 = 0; b0 < nb; b0 += kThreads) {
    const u64 b = b0 + threadIdx.x;
    u64 tot;
    const u64 ex = mask_block_excl(b < nb ? part[b] : jyuj::kMaskId, lds, tot);
    if (b < nb) part[b] = jyuj::mask_compose(carry, ex);
    carry = jyuj::mask_compose(carry, tot);
  }
}
__global__ __launch_bounds__(kThreads) void k_uj_mask_down(const u32* __restrict__ shape, const u64* __restrict__ count,
                                                           const u64* __restrict__ part, u32* __restrict__ state) {
  __shared__ u64 lds[kThreads / 64];
  const MaskIn in{shape, *count};
  const u64 s0 = (u64)blockIdx.x * kMaskTile + (u64)threadIdx.x * kMaskPer;
  u64 e[kMaskPer], x = jyuj::kMaskId;
#pragma unroll
  for (int k = 0; k < kMaskPer; k++) {
    e[k] = s0 + k < in.u ? in(s0 + k) : jyuj::kMaskId;
    x = jyuj::mask_compose(x, e[k]);
  }
  u64 tot;
  u64 run = jyuj::mask_compose(part[blockIdx.x], mask_block_excl(x, lds, tot));
#pragma unroll
  for (int k = 0; k < kMaskPer; k++) {
    run = jyuj::mask_compose(run, e[k]);
    if (s0 + k < in.u) state[in.u - 1 - (s0 + k)] = jyuj::mask_state(run);
  }
}

// ---- pieces ----
__device__ __forceinline__ jyuj::Place place_of(const u32* __restrict__ shape, const u32* __restrict__ state, u64 j,
                                                u64 u) {
  const u32 sh = shape[j];
  jyuj::Place p;
  p.first = sh & kShFirst;
  p.cp = (sh >> 8) & 0xFFu;
  p.depth = sh & 0xFFu;
  p.last = j + 1 == u || (shape[j + 1] & kShFirst);
  p.cs = p.last ? 0u : (shape[j + 1] >> 8) & 0xFFu;
  p.dnext = p.last ? 0u : shape[j + 1] & 0xFFu;
  p.state = state[j];
  return p;
}

constexpr u64 kRefShift = 62;
constexpr u64 kRefPayload = (1ull << kRefShift) - 1;
enum : u64 { kInl = 0, kPtr = 1, kClose = 2, kHead = 3 };
__host__ __device__ constexpr u64 ref_of(u64 kind, u64 payload) { return (kind << kRefShift) | payload; }
__device__ __forceinline__ jyresp::Gen head_gen(u64 text) { return jyresp::Gen{0x24ull, 1, text}; }  // $<len>\r\n

struct CountOut {  // a leaf's pieces and text bytes
  u64 pieces = 0, bytes = 0;
  __device__ __forceinline__ void inl(jyuj::Punct p) { pieces++, bytes += p.len; }
  __device__ __forceinline__ void ptr(u64, u64 len) { pieces++, bytes += len; }
  __device__ __forceinline__ void close(bool br, u32 nb) { pieces++, bytes += jyuj::close_len(br, nb); }
};
struct WriteOut {  // (length, reference) of each piece, from piece k on
  u64* plen;
  u64* pref;
  u64 k;
  u64 leaf_off;  // the leaf's first byte in the arena
  __device__ __forceinline__ void put(u64 len, u64 ref) {
    plen[k] = len;
    pref[k++] = ref;
  }
  __device__ __forceinline__ void inl(jyuj::Punct p) { put(p.len, ref_of(kInl, p.bytes)); }
  __device__ __forceinline__ void ptr(u64 at, u64 len) { put(len, ref_of(kPtr, leaf_off + at)); }
  __device__ __forceinline__ void close(bool br, u32 nb) {
    put(jyuj::close_len(br, nb), ref_of(kClose, (br ? 256u : 0u) | nb));
  }
};

// per distinct leaf its pieces and text bytes (0 for a query left to the host);
// lanes u .. m close both scans' inputs
__global__ __launch_bounds__(kThreads) void k_uj_count(Leaves L, u64 m, const u32* __restrict__ shape,
                                                       const u32* __restrict__ state,
                                                       const uint8_t* __restrict__ on_host, u64* __restrict__ cnt,
                                                       u64* __restrict__ tlen, unsigned long long* rendered) {
  const u64 j = gid(), u = *L.count;
  bool r = false;
  if (j <= m) {
    CountOut out;
    if (j < u && !on_host[L.q[j]]) {
      jyuj::leaf_text(L.leaf(j), L.len(j), place_of(shape, state, j, u), out);
      r = true;
    }
    cnt[j] = out.pieces;
    tlen[j] = out.bytes;
  }
  jy_wave_count(r, rendered);
}

// Query q's pieces are 2 q + coff[uo[q]] (its head) .. 2 q + 1 + coff[uo[q + 1]]
// (its tail), its leaves' in between.
__global__ __launch_bounds__(kThreads) void k_uj_pieces(Leaves L, const u32* __restrict__ shape,
                                                        const u32* __restrict__ state,
                                                        const uint8_t* __restrict__ on_host,
                                                        const u64* __restrict__ coff, u64* __restrict__ plen,
                                                        u64* __restrict__ pref) {
  const u64 j = gid(), u = *L.count;
  if (j >= u) return;
  const u32 q = L.q[j];
  if (on_host[q]) return;
  WriteOut out{plen, pref, 2 * (u64)q + 1 + coff[j], L.off(j)};
  jyuj::leaf_text(L.leaf(j), L.len(j), place_of(shape, state, j, u), out);
}
// head and tail of query q < n (both empty for a query left to the host), where
// its reply starts among the pieces, and (lane n) the end of the lengths
__global__ __launch_bounds__(kThreads) void k_uj_qpieces(const u64* __restrict__ uo, const u64* __restrict__ coff,
                                                         const u64* __restrict__ toff,
                                                         const uint8_t* __restrict__ on_host, u64 n,
                                                         u64* __restrict__ plen, u64* __restrict__ pref,
                                                         u64* __restrict__ hidx, unsigned long long* nhost) {
  const u64 q = gid();
  bool host = false;
  if (q <= n) {
    const u64 h = 2 * q + coff[uo[q]];
    hidx[q] = h;
    if (q == n) {
      plen[h] = 0;
    } else {
      host = on_host[q] != 0;
      const u64 t = 2 * q + 1 + coff[uo[q + 1]];
      const u64 text = toff[uo[q + 1]] - toff[uo[q]];
      plen[h] = host ? 0 : jyresp::gen_len(head_gen(text));
      pref[h] = ref_of(kHead, text);
      plen[t] = host ? 0 : 2;
      pref[t] = ref_of(kInl, 0x0A0Dull);
    }
  }
  jy_wave_count(host, nhost);
}
__global__ __launch_bounds__(kThreads) void k_uj_roffs(const u64* __restrict__ poff, const u64* __restrict__ hidx,
                                                       u64 n, u64* __restrict__ roffs) {
  const u64 q = gid();
  if (q <= n) roffs[q] = poff[hidx[q]];
}

// piece i of the reply stream (k_wire_gather's generating form, as RespSrc)
struct RenderSrc {
  const u64* ref;  // per piece: kind << 62 | inline bytes, arena offset, closers or text length
  const uint8_t* arena;
  __device__ __forceinline__ u64 gen(u64 i, u64 from, u64 take) const {
    const u64 r = ref[i];
    const u64 kind = r >> kRefShift, x = r & kRefPayload;
    if (kind == kPtr) return jy_ld8u(arena + x + from, take);
    u64 v = kind == kInl     ? x >> (8 * from)
            : kind == kClose ? jyuj::close8((x >> 8) & 1u, (u32)(x & 0xFFu), (u32)from)
                             : jyresp::gen8(head_gen(x), (u32)from);
    if (take < 8) v &= (1ull << (8 * take)) - 1;
    return v;
  }
};

}  // namespace

// The render's core (jy_internal.hpp): n > 0 queries by device slots (`slots`,
// JY_NO_SLOT: no such key) or, slots == nullptr, by key strings the caller has
// checked (keys_check), at paths in DEVICE memory: path i = d_path_bytes[
// d_path_offs[i] .. d_path_offs[i + 1]), d_path_offs == nullptr: every path
// empty.  reply_bytes, reply_offs and on_host are left in the memory the caller
// names: its own arrays in `mem` under the two-phase rule, or, with `dst`, room
// asked of it once the total is known, the offsets at dst->reply_offs and
// on_host a device array.
// NO PATH IS CHECKED ON THE DEVICE.  The path core never parses a path and never
// reads past one: k_uj_path_match compares the plen bytes between two offsets
// with the head of a stored leaf, after the one test that the leaf is at least
// that long (plen + kLeafMinLen <= len).  What a path must be is a whole
// sequence of len|bytes segments, so that what is left of a matched leaf starts
// at a segment: the render reads it as segments from there.  Paths a caller
// wrote are therefore checked in full on the host before this core is called
// (jy_ujson_get_resp, path_query_check).  The only other paths are the
// decoder's (k_resp_in.hip, JY_RESP_UJSON_GET), which are well-formed by
// construction: k_rin_vpiece_words writes every segment as the four bytes of
// a word's length and then exactly that word, of words whose lengths passed
// path_word_ok, at offsets that are the scan of those same 4 + len.
int32_t jy_ujson_get_resp_core(jy_engine* eng, uint64_t n, const uint32_t* slots, const uint8_t* key_bytes,
                               const uint64_t* key_offs, int32_t keys_mem, const uint8_t* d_path_bytes,
                               const uint64_t* d_path_offs, uint64_t cap_bytes, uint8_t* reply_bytes,
                               uint64_t* reply_offs, uint8_t* on_host, uint64_t* sizes_out, int32_t mem,
                               JyRespDst* dst) {
  JY_HIP(eng, hipSetDevice(eng->device));
  for (int q = 0; q < 6; q++) sizes_out[q] = 0;
  if (dst) mem = JY_DEVICE, reply_offs = dst->reply_offs;
  if (!reply_offs || !on_host) return eng->fail(JY_EINVAL, "reply_offs or on_host is null");
  if (n >= (1ull << 31)) return eng->fail(JY_ERANGE, "more than 2^31 - 1 queries");

  Tmp tmp(eng);
  if (!slots) JY_TRY(query_slots(eng, tmp, JY_UJSON, n, key_bytes, key_offs, keys_mem, &slots));
  uint8_t *df, *oh;
  u64* cnts;  // found keys, rendered leaves, queries left to the host
  JY_TRY(tmp.get(&df, n));
  JY_TRY(tmp.get(&oh, n));
  JY_TRY(tmp.get(&cnts, 3));
  JY_HIP(eng, hipMemsetAsync(oh, 0, n, eng->stream));
  JY_HIP(eng, hipMemsetAsync(cnts, 0, 24, eng->stream));
  unsigned long long* ucnts = reinterpret_cast<unsigned long long*>(cnts);
  LAUNCH(k_get_found, n, slots, n, df, static_cast<u32*>(nullptr), ucnts);

  // ---- the path core: which leaves each query renders ----
  PathSel S;
  if (eng->nkeys[JY_UJSON]) {
    const uint8_t* pb = d_path_bytes;
    const u64* po = d_path_offs;
    if (!po) {  // every path is empty
      u64* z;
      JY_TRY(tmp.get(&z, n + 1));
      JY_HIP(eng, hipMemsetAsync(z, 0, (n + 1) * 8, eng->stream));
      po = z;
    }
    JY_TRY(path_select(eng, tmp, n, slots, true, pb, po, true, S));
  }
  const u64 m = S.me ? S.m : 0;
  sizes_out[3] = S.me;
  sizes_out[5] = S.missing;
  if (m >= (1ull << 32)) return eng->fail(JY_ERANGE, "more than 2^32 - 1 leaves selected");

  // the distinct leaves in order, their CSR uo[n + 1], and the scans of their
  // pieces (coff) and text bytes (toff); with no match all of it is zeros
  u64 *uo, *coff, *toff, *ucount;
  u32 *shape = nullptr, *state = nullptr;
  Leaves L{eng->leaf.bytes, nullptr, nullptr, nullptr, nullptr};
  JY_TRY(tmp.get(&uo, n + 1));
  JY_TRY(tmp.get(&coff, m + 1));
  JY_TRY(tmp.get(&toff, m + 1));
  if (m == 0) {
    JY_TRY(tmp.get(&ucount, 1));
    JY_HIP(eng, hipMemsetAsync(uo, 0, (n + 1) * 8, eng->stream));
    JY_HIP(eng, hipMemsetAsync(coff, 0, 8, eng->stream));
    JY_HIP(eng, hipMemsetAsync(toff, 0, 8, eng->stream));
    JY_HIP(eng, hipMemsetAsync(ucount, 0, 8, eng->stream));
    L.count = ucount;
  } else {
    u64 *dq, *de, *klr, *dlo, *head, *ho, *cnt, *tlen;
    u32 *skip, *qid, *pa, *pb2;
    JY_TRY(tmp.get(&dq, n + 1));
    JY_TRY(tmp.get(&de, m));
    JY_TRY(tmp.get(&klr, m));
    JY_TRY(tmp.get(&skip, m));
    JY_TRY(tmp.get(&dlo, m + 1));
    JY_TRY(path_compact(eng, S, dq, de, klr, skip, dlo));
    JY_TRY(tmp.get(&qid, m));
    LAUNCH(k_uj_qid, m, dq, n, m, qid);
    const Matches M{eng->leaf.bytes, klr, skip, qid};
    // ---- order ----
    JY_TRY(tmp.get(&pa, m));
    JY_TRY(tmp.get(&pb2, m));
    const u32* perm = nullptr;
    for (u64 w = 1; w < m || !perm; w *= 2) {  // (m == 1: one round, the identity written out)
      u32* dst = perm == pa ? pb2 : pa;
      LAUNCH(k_uj_merge, m, M, m, w, perm, dst);
      perm = dst;
    }
    // ---- de-duplicate ----
    Uniq U;
    JY_TRY(tmp.get(&head, m + 1));
    JY_TRY(tmp.get(&ho, m + 1));
    JY_TRY(tmp.get(&U.lr, m));
    JY_TRY(tmp.get(&U.skip, m));
    JY_TRY(tmp.get(&U.q, m));
    LAUNCH(k_uj_heads_of, m + 1, M, m, perm, head);
    JY_TRY(jy_scan_u64(eng, head, ho, m));
    LAUNCH(k_uj_uniq, m, M, m, perm, head, ho, U);
    LAUNCH(k_uj_uoffs, n + 1, dq, ho, n, uo);
    L = Leaves{eng->leaf.bytes, U.lr, U.skip, U.q, ho + m};
    // ---- structure ----
    JY_TRY(tmp.get(&shape, m));
    JY_TRY(tmp.get(&state, m));
    LAUNCH(k_uj_shape, m, L, shape, oh);
    const u64 nb = (m + kMaskTile - 1) / kMaskTile;
    u64* part;
    JY_TRY(tmp.get(&part, nb));
    hipLaunchKernelGGL(k_uj_mask_part, dim3((u32)nb), dim3(kThreads), 0, eng->stream, (const u32*)shape, L.count, part);
    hipLaunchKernelGGL(k_uj_mask_mid, dim3(1), dim3(kThreads), 0, eng->stream, nb, part);
    hipLaunchKernelGGL(k_uj_mask_down, dim3((u32)nb), dim3(kThreads), 0, eng->stream, (const u32*)shape, L.count,
                       (const u64*)part, state);
    JY_HIP(eng, hipGetLastError());
    // ---- pieces: counted ----
    JY_TRY(tmp.get(&cnt, m + 1));
    JY_TRY(tmp.get(&tlen, m + 1));
    LAUNCH(k_uj_count, m + 1, L, m, shape, state, oh, cnt, tlen, ucnts + 1);
    JY_TRY(jy_scan_u64(eng, cnt, coff, m));
    JY_TRY(jy_scan_u64(eng, tlen, toff, m));
  }
  u64 tot[3];
  JY_TRY(totals(eng, {coff + m, cnts, cnts + 1}, tot));  // the third wait: the leaves' pieces
  const u64 P = 2 * n + tot[0];
  sizes_out[1] = tot[1];
  sizes_out[2] = tot[2];

  // ---- pieces: written, and the one scan over their lengths ----
  u64 *plen, *pref, *poff, *hidx;
  JY_TRY(tmp.get(&plen, P + 1));
  JY_TRY(tmp.get(&pref, P + 1));
  JY_TRY(tmp.get(&poff, P + 1));
  JY_TRY(tmp.get(&hidx, n + 1));
  if (m) LAUNCH(k_uj_pieces, m, L, shape, state, oh, coff, plen, pref);
  LAUNCH(k_uj_qpieces, n + 1, uo, coff, toff, oh, n, plen, pref, hidx, ucnts + 2);
  JY_TRY(jy_scan_u64(eng, plen, poff, P));
  u64 fin[2];
  JY_TRY(totals(eng, {poff + P, cnts + 2}, fin));  // the last wait: the reply bytes
  const u64 total = fin[0];
  sizes_out[0] = total;
  sizes_out[4] = fin[1];
  bool fits;
  JY_TRY(resp_room(dst, total, cap_bytes, &reply_bytes, &reply_offs, &mem, &fits));
  if (!fits) return JY_OK;  // sizes only
  if (total && !reply_bytes) return eng->fail(JY_EINVAL, "reply_bytes is null");

  // ---- write ----
  uint8_t* rb;
  u64* ro;
  JY_TRY(tmp.out(&rb, reply_bytes, total, mem));
  JY_TRY(tmp.out(&ro, reply_offs, n + 1, mem));
  JY_TRY(gather(eng, RenderSrc{pref, eng->leaf.bytes}, poff, P, total, rb));
  LAUNCH(k_uj_roffs, n + 1, poff, hidx, n, ro);
  JY_TRY(emit(eng, mem, reply_bytes, rb, total));
  JY_TRY(emit(eng, mem, reply_offs, ro, (n + 1) * 8));
  JY_TRY(emit(eng, mem, on_host, oh, n));
  return host_sync(eng, mem);
}

extern "C" {

// the core plus what a caller's own paths need: the host's check, and their staging.
// The null and 2^31 checks (and the zeroing of sizes_out) are the core's too, ON
// PURPOSE: here they keep the call's error order -- keys, paths, outputs, count --
// and nothing is staged for a call that fails; the core keeps them for its other caller.
int32_t jy_ujson_get_resp(jy_engine* eng, uint64_t n, const uint8_t* key_bytes, const uint64_t* key_offs,
                          int32_t keys_mem, const uint8_t* path_bytes, const uint64_t* path_offs, uint64_t cap_bytes,
                          uint8_t* reply_bytes, uint64_t* reply_offs, uint8_t* on_host, uint64_t* sizes_out,
                          int32_t mem) {
  JY_HIP(eng, hipSetDevice(eng->device));
  for (int q = 0; q < 6; q++) sizes_out[q] = 0;
  JY_TRY(mem_check(eng, mem));
  if (n == 0) return empty_batch(eng, mem, {reply_offs});
  JY_TRY(keys_check(eng, n, key_bytes, key_offs, keys_mem));
  // ---- the paths are checked in full here, before any launch ----
  if (path_offs) JY_TRY(path_query_check(eng, n, path_bytes, path_offs));
  if (!reply_offs || !on_host) return eng->fail(JY_EINVAL, "reply_offs or on_host is null");
  if (n >= (1ull << 31)) return eng->fail(JY_ERANGE, "more than 2^31 - 1 queries");
  Tmp stage(eng);  // outlives the core's launches (freed in stream order)
  const uint8_t* pb = nullptr;
  const u64* po = nullptr;
  if (path_offs && eng->nkeys[JY_UJSON]) JY_TRY(path_stage(eng, stage, n, path_bytes, path_offs, &pb, &po));
  return jy_ujson_get_resp_core(eng, n, nullptr, key_bytes, key_offs, keys_mem, pb, po, cap_bytes, reply_bytes,
                                reply_offs, on_host, sizes_out, mem, nullptr);
}

}  // extern "C"
