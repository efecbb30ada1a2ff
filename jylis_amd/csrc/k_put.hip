// k_put.hip -- keyed batch writes: INC / DEC, TREG SET and the TLOG commands
// by key string, in host or device memory (include/jylis_gpu.h "keyed
// writes").
//
// Boundary: RepoGCOUNT.inc (repo_gcount.pony:57-60), RepoPNCOUNT.inc / dec
// (repo_pncount.pony:59-67), RepoTREG.set (repo_treg.pony:65-68), RepoTLOG.ins
// / trimat / trim / clr (repo_tlog.pony:85-111), each with its _data_for
// (create on miss).  One call takes a batch of commands as the RESP layer has
// them -- key strings and value bytes -- interns the keys on the device, packs
// the values on the device and applies the batch in command order; no slot
// and no value handle crosses to the host.
//
// Three pieces live here:
//   value packing   jy_values_pack's (pre, lr) handles computed on the device:
//                   lengths -> padded lengths of the long values -> one scan
//                   -> a lane per value writes pre / lr -> the long values'
//                   bytes copied with the output balanced by 8-byte granules
//                   (a 1 MiB value spreads over 131072 lanes; jy_wire.hpp's
//                   gather does the same for reads).  Long values start on
//                   8-byte granules, so an output granule belongs to exactly
//                   one value.
//   checks          host arrays are checked on the host; device arrays by one
//                   kernel whose verdict is read back before any kernel that
//                   loops over a length is launched (jy_put_check.hpp, shared
//                   with k_uj_put.hip, as is the staging of a ragged column)
//   TLOG in order   a batch that repeats keys goes through the device round
//                   split (jy_drounds.hpp, shared with k_uj_put.hip): grouped
//                   by key, each key's run cut into UNITS -- up to 64
//                   consecutive INS, or one TRIMAT / TRIM / CLR -- and the
//                   j-th unit of every key applied in round j: one delta per
//                   key per round, the rounds in stream order.  What stays
//                   here is a round: an INS unit is one multi-entry
//                   delta: a wave orders its entries newest first, drops
//                   exact duplicates and judges each against the state by
//                   the rules of jy_tlog_rules.hpp, as k_tlog_wprep judges
//                   one INS (INS never moves the cutoff, duplicates collapse
//                   in the join).
#include <algorithm>
#include <cstring>
#include <vector>

#include "jy_drounds.hpp"
#include "jy_internal.hpp"
#include "jy_put_check.hpp"
#include "jy_tlog_rules.hpp"
#include "jy_wire.hpp"

namespace {

constexpr u32 kUnitMax = 64;  // INS commands in one unit: one wave orders them

inline u64 round_up8(u64 x) { return (x + 7) & ~7ull; }

// ---- value packing -------------------------------------------------------------
// plen[i] = arena bytes value i takes (0 for values of up to 8 bytes); plen[n] = 0
__global__ __launch_bounds__(kThreads) void k_put_vlen(const u64* __restrict__ offs, u64 n, u64* __restrict__ plen) {
  const u64 i = gid();
  if (i > n) return;
  u64 v = 0;
  if (i < n) {
    const u64 len = offs[i + 1] - offs[i];
    if (len > 8 && len <= JY_MAX_VALUE_LEN) v = (len + 7) & ~7ull;
  }
  plen[i] = v;
}

// a lane per value: pre = first 8 bytes big-endian, zero padded; lr = len, or
// (base + poff[i]) << 24 | len for a value in the arena
__global__ __launch_bounds__(kThreads) void k_put_handles(const uint8_t* __restrict__ bytes,
                                                          const u64* __restrict__ offs, u64 n,
                                                          const u64* __restrict__ poff, u64 base,
                                                          u64* __restrict__ pre, u64* __restrict__ lr) {
  const u64 i = gid();
  if (i >= n) return;
  const u64 o = offs[i], len = offs[i + 1] - o;
  pre[i] = __builtin_bswap64(jy_ld8u(bytes + o, len < 8 ? len : 8));
  lr[i] = len > 8 ? ((base + poff[i]) << JY_LR_LEN_BITS) | len : len;
}

// dst[poff[i] .. poff[i] + len_i) = value i's bytes, zero padded to its 8-byte
// granules, for the values with poff[i + 1] > poff[i]; total = poff[n] > 0.
// A lane owns one output granule; dst is 8-byte aligned.
__global__ __launch_bounds__(kThreads) void k_put_copy(const uint8_t* __restrict__ bytes, const u64* __restrict__ offs,
                                                       const u64* __restrict__ poff, u64 n, u64 total,
                                                       uint8_t* __restrict__ dst) {
  __shared__ u64 so[kStage];
  __shared__ u64 ends[2];
  const u64 g0 = (u64)blockIdx.x * kThreads;
  const u64 tb0 = g0 * kGranule;
  const u64 tb1 = std::min<u64>((g0 + kThreads) * kGranule, total);
  const auto glob = [&](u64 j) { return poff[j]; };
  if (threadIdx.x < 2) ends[threadIdx.x] = item_of(glob, 0, n, threadIdx.x == 0 ? tb0 : tb1 - 1);
  __syncthreads();
  const u64 ilo = ends[0], ihi = ends[1];
  const u64 cnt = ihi - ilo + 2;  // offsets ilo .. ihi + 1
  const bool staged = cnt <= kStage;
  if (staged)
    for (u64 q = threadIdx.x; q < cnt; q += kThreads) so[q] = poff[ilo + q];
  __syncthreads();
  const auto at = [&](u64 j) { return staged ? so[j - ilo] : poff[j]; };
  const u64 b0 = (g0 + threadIdx.x) * kGranule;
  if (b0 >= total) return;
  const u64 i = item_of(at, ilo, ihi + 1, b0);
  const u64 from = b0 - at(i), o = offs[i], len = offs[i + 1] - o;
  const u64 take = from < len ? std::min<u64>(len - from, kGranule) : 0;
  *reinterpret_cast<u64*>(dst + b0) = jy_ld8u(bytes + o + from, take);
}

// ---- TLOG: one round of units (jy_drounds.hpp cuts the batch into them) -------
struct PCmd {
  const uint8_t* op;
  const u64* ts;
  const u64* arg;
  const u64* pre;
  const u64* lr;
};
constexpr uint8_t kDropped = 0xFF;

// One wave per unit of this round (units ul[0 .. m)).  An INS unit: lane l
// holds the unit's l-th command; `newer` = the lanes whose entry is newer (ts,
// then value), `dup` = an equal entry sits on a lower lane.  Kept entries are
// judged against the state (jy_tlog_rules.hpp, as k_tlog_wprep judges one
// INS); their ranks among the kept (state delta) and among the changed
// (pending delta) are stashed per sorted position for k_put_wpack.  Any other
// unit is one command, judged by lane 0.  Every unit marks its key pending.
__global__ __launch_bounds__(kThreads) void k_put_wprep(PCmd W, const u64* __restrict__ ul, u64 m,
                                                        const u64* __restrict__ ustart, const u64* __restrict__ skey,
                                                        const TMeta* __restrict__ meta, const TRec* __restrict__ pool,
                                                        const uint8_t* __restrict__ arena, u32* __restrict__ rslot,
                                                        u64* __restrict__ scut, u64* __restrict__ scnt,
                                                        u64* __restrict__ dcut, u64* __restrict__ dcnt,
                                                        uint8_t* __restrict__ spos, uint8_t* __restrict__ dpos,
                                                        u32* __restrict__ pend, u64* __restrict__ pcount) {
  const u64 w = gid() >> 6;
  const int lane = threadIdx.x & 63;
  if (w >= m) return;  // whole waves leave together
  const u32 u = (u32)ul[w];
  const u64 a = ustart[u], cnt = ustart[u + 1] - a;
  const u64 k0 = skey[a];
  const u32 s = (u32)(k0 >> 32);
  const TMeta mt = meta[s];
  const uint8_t op = W.op[(u32)k0];
  u64 raise = 0, ns = 0, nd = 0;
  bool changed = false;
  if (op == JY_TLOG_INS) {
    const bool valid = (u64)lane < cnt;
    Ent x{0, 0, 0};  // (an idle lane's entry has no arena bytes)
    if (valid) {
      const u32 i = (u32)skey[a + lane];
      x = Ent{W.ts[i], W.pre[i], W.lr[i]};
    }
    u64 newer = 0;
    bool dup = false;
    for (u32 j = 0; j < (u32)cnt; j++) {
      const Ent y{__shfl(x.t, (int)j), __shfl(x.p, (int)j), __shfl(x.l, (int)j)};
      int c = y.t != x.t ? (y.t > x.t ? 1 : -1) : 0;
      if (c == 0 && valid) c = jy_value_cmp(y.p, y.l, x.p, x.l, arena);
      if (c > 0) newer |= 1ull << j;
      if (c == 0 && j < (u32)lane) dup = true;
    }
    const bool keep = valid && !dup;
    const bool chg = keep && tlog_ins_changes(mt, pool, arena, x);
    const u64 keepm = __ballot(keep), chgm = __ballot(chg);
    if (valid) {
      spos[a + lane] = keep ? (uint8_t)__popcll(newer & keepm) : kDropped;
      dpos[a + lane] = chg ? (uint8_t)__popcll(newer & chgm) : kDropped;
    }
    ns = (u64)__popcll(keepm);
    nd = (u64)__popcll(chgm);
  } else if (lane == 0) {
    const u32 i = (u32)k0;
    raise = tlog_cut_raise(op, W.ts[i], W.arg[i], mt, pool, &changed);
    spos[a] = kDropped;
    dpos[a] = kDropped;
  }
  if (lane == 0) {
    rslot[w] = s;
    scut[w] = raise;
    scnt[w] = ns;
    dcut[w] = changed ? raise : 0;
    dcnt[w] = nd;
    if (atomicExch(pend + s, 1u) == 0) atomicAdd(reinterpret_cast<unsigned long long*>(pcount), 1ull);
  }
}

// the units' entries into the two deltas' CSRs, newest first
__global__ __launch_bounds__(kThreads) void k_put_wpack(PCmd W, const u64* __restrict__ ul, u64 m,
                                                        const u64* __restrict__ ustart, const u64* __restrict__ skey,
                                                        const uint8_t* __restrict__ spos,
                                                        const uint8_t* __restrict__ dpos, const u64* __restrict__ soff,
                                                        const u64* __restrict__ doff, u64* __restrict__ sts,
                                                        u64* __restrict__ spre, u64* __restrict__ slr,
                                                        u64* __restrict__ dts, u64* __restrict__ dpre,
                                                        u64* __restrict__ dlr) {
  const u64 w = gid() >> 6;
  const u64 lane = threadIdx.x & 63;
  if (w >= m) return;
  const u32 u = (u32)ul[w];
  const u64 a = ustart[u], cnt = ustart[u + 1] - a;
  if (lane >= cnt) return;
  const uint8_t sp = spos[a + lane], dp = dpos[a + lane];
  if (sp == kDropped) return;
  const u32 i = (u32)skey[a + lane];
  const u64 t = W.ts[i], p = W.pre[i], l = W.lr[i];
  const u64 so = soff[w] + sp;
  sts[so] = t;
  spre[so] = p;
  slr[so] = l;
  if (dp != kDropped) {
    const u64 o = doff[w] + dp;
    dts[o] = t;
    dpre[o] = p;
    dlr[o] = l;
  }
}

}  // namespace

// ---- value packing: device arrays in, device handles out ----------------------
// `add` = the arena bytes the long values take with their padding (the host
// knows it for host input; device input: ~0, read back with the verdict in
// the call's one wait).  `verdict` (device, or null) is k_put_check's word.
static int32_t pack_dev(jy_engine* eng, Tmp& tmp, int32_t type, u64 n, const uint8_t* bytes, const u64* offs, u64 add,
                        const u32* verdict, u64* pre, u64* lr) {
  if (type != JY_TREG && type != JY_TLOG) return eng->fail(JY_EINVAL, "only TREG and TLOG hold an arena");
  if (n == 0) return JY_OK;
  u64 *plen, *poff;
  JY_TRY(tmp.get(&plen, 2 * (n + 1)));
  poff = plen + n + 1;
  LAUNCH(k_put_vlen, n + 1, offs, n, plen);
  JY_TRY(jy_scan_u64(eng, plen, poff, n));
  if (add == ~0ull) {
    u64* pin = eng->pin_total;
    pin[0] = 0;
    if (verdict) JY_HIP(eng, hipMemcpyAsync(pin, verdict, 4, hipMemcpyDeviceToHost, eng->stream));
    JY_HIP(eng, hipMemcpyAsync(pin + 1, poff + n, 8, hipMemcpyDeviceToHost, eng->stream));
    JY_HIP(eng, hipMemcpyAsync(pin + 2, offs + n, 8, hipMemcpyDeviceToHost, eng->stream));
    JY_HIP(eng, hipStreamSynchronize(eng->stream));
    JY_TRY(verdict_rc(eng, (u32)pin[0]));
    add = pin[1];
    if (add > round_up8(pin[2]) + 8 * n) return eng->fail(JY_EINVAL, "value offsets do not bound their bytes");
  }
  Arena& a = eng->arena[type];
  const u64 base = round_up8(a.len);
  if (add == 0) {
    LAUNCH(k_put_handles, n, bytes, offs, n, poff, base, pre, lr);
    return JY_OK;
  }
  if ((base + add) >> (64 - JY_LR_LEN_BITS)) return eng->fail(JY_ERANGE, "arena offset overflow");
  JY_TRY(jy_arena_ensure(eng, type, add));  // before the launches: the arena does not move under them
  if (base > a.len) JY_HIP(eng, hipMemsetAsync(a.p + a.len, 0, base - a.len, eng->stream));
  LAUNCH(k_put_handles, n, bytes, offs, n, poff, base, pre, lr);
  const u64 tiles = (add + kTileBytes - 1) / kTileBytes;
  hipLaunchKernelGGL(k_put_copy, dim3((u32)tiles), dim3(kThreads), 0, eng->stream, bytes, offs, (const u64*)poff, n,
                     add, a.p + base);
  JY_HIP(eng, hipGetLastError());
  a.len = base + add;
  return JY_OK;
}

// host offsets: ascending, every length within `max_len`; *add_out (optional)
// = the arena bytes of the long values
static int32_t offs_check_host(jy_engine* eng, u64 n, const u64* offs, u64 max_len, const char* what, u64* add_out) {
  u64 add = 0;
  for (u64 i = 0; i < n; i++) {
    if (offs[i + 1] < offs[i]) return eng->fail(JY_EINVAL, std::string(what) + " offsets do not ascend");
    const u64 len = offs[i + 1] - offs[i];
    if (len > max_len) return eng->fail(JY_ERANGE, std::string(what) + " longer than 16 MiB");
    if (len > 8) add += round_up8(len);
  }
  if (add_out) *add_out = add;
  return JY_OK;
}

// ---- TLOG: a device batch in command order, whatever repeats ------------------
int32_t jy_tlog_write_ordered(jy_engine* eng, u64 n, const uint8_t* op, const u32* slot, const u64* ts, const u64* arg,
                              const u64* pre, const u64* lr) {
  if (n == 0) return JY_OK;
  if (n >= 0xFFFFFFFFull) return eng->fail(JY_ERANGE, "more than 2^32 - 1 commands in one call");
  eng->tlw_calls++;
  if (n == 1) {
    eng->tlw_rounds_last = 1;
    eng->tlw_rounds_total++;
    return jy_tlog_write_batch(eng, n, op, slot, ts, arg, pre, lr);
  }
  Tmp tmp(eng);
  // the grouping (jy_drounds.hpp): up to kUnitMax consecutive INS of a key are one unit
  JyDRounds D;
  const u32 sbits = jysort::bits_for(eng->nkeys[JY_TLOG]);
  JY_TRY(jy_drounds<kUnitMax>(eng, tmp, n, slot, nullptr, op, JY_TLOG_INS, sbits, &D));
  const u64 R = D.R, *skey = D.skey, *ustart = D.ustart, *ul = D.ul;
  const std::vector<u64>& ro = D.ro;
  eng->tlw_rounds_last = R;
  eng->tlw_rounds_total += R;
  if (R == 1 && D.U == n)  // no key repeats: the batch as it is, one command per key
    return jy_tlog_write_batch(eng, n, op, slot, ts, arg, pre, lr);
  const u64 m0 = ro[1];  // the first round is the largest
  const u64 e0 = std::min<u64>(n, kUnitMax * m0);
  u64* d;
  JY_TRY(tmp.get(&d, 6 * (m0 + 1) + 6 * e0 + (m0 + 1) / 2 + n / 4 + 16));
  u64 *scut = d, *scnt = scut + m0 + 1, *dcut = scnt + m0 + 1, *dcnt = dcut + m0 + 1, *soff = dcnt + m0 + 1,
      *doff = soff + m0 + 1, *sts = doff + m0 + 1, *spre = sts + e0, *slr = spre + e0, *dts = slr + e0, *dpre = dts + e0,
      *dlr = dpre + e0;
  u32* rslot = reinterpret_cast<u32*>(dlr + e0);
  uint8_t* spos = reinterpret_cast<uint8_t*>(rslot + m0 + 2);
  uint8_t* dpos = spos + n;
  const PCmd W{op, ts, arg, pre, lr};
  JY_TRY(jy_tlog_pending_grow(eng));
  for (u64 j = 0; j < R; j++) {
    const u64 m = ro[j + 1] - ro[j];
    if (m == 0 || m > m0) return eng->fail(JY_EINVAL, "tlog write: a round's units are out of range");
    const u64 ecap = std::min<u64>(n, kUnitMax * m);
    // every unit is judged against the state as the rounds before left it
    JY_TRY(jy_tlog_settle(eng));
    TlogState& t = eng->tlog;
    JY_HIP(eng, hipMemsetAsync(scnt + m, 0, 8, eng->stream));
    JY_HIP(eng, hipMemsetAsync(dcnt + m, 0, 8, eng->stream));
    LAUNCH(k_put_wprep, m * 64, W, ul + ro[j], m, ustart, skey, t.meta, t.pool,
           eng->arena[JY_TLOG].p, rslot, scut, scnt, dcut, dcnt, spos, dpos, eng->tl_pend.flag, eng->tl_pend.count);
    JY_TRY(jy_scan_u64(eng, scnt, soff, m));
    JY_TRY(jy_scan_u64(eng, dcnt, doff, m));
    LAUNCH(k_put_wpack, m * 64, W, ul + ro[j], m, ustart, skey,
           (const uint8_t*)spos, (const uint8_t*)dpos, (const u64*)soff, (const u64*)doff, sts, spre, slr, dts, dpre,
           dlr);
    JY_TRY(jy_tlog_merge_into(eng, t, m, rslot, scut, soff, ecap, sts, spre, slr));
    JY_TRY(jy_tlog_merge_into(eng, eng->tlog_d, m, rslot, dcut, doff, ecap, dts, dpre, dlr));
  }
  // the temporaries are freed in stream order, after the last round's merges;
  // a spilled merge keeps its own copy of its deltas
  return JY_OK;
}

// ---- the keyed calls -----------------------------------------------------------
// The keys of a call are staged (host: stage_ragged leaves the call's own
// column pointers naming the device copies) or used in place (device) and
// interned on the device with create-on-miss; the slots stay in a temporary.
extern "C" {

int32_t jy_values_pack_mem(jy_engine* eng, int32_t type, uint64_t n, const uint8_t* bytes, const uint64_t* offs,
                           int32_t mem, uint64_t* pre_out, uint64_t* lr_out, int32_t out_mem) {
  JY_HIP(eng, hipSetDevice(eng->device));
  if (type != JY_TREG && type != JY_TLOG) return eng->fail(JY_EINVAL, "only TREG and TLOG hold an arena");
  if ((mem != JY_HOST && mem != JY_DEVICE) || (out_mem != JY_HOST && out_mem != JY_DEVICE))
    return eng->fail(JY_EINVAL, "mem must be JY_HOST or JY_DEVICE");
  if (n == 0) return JY_OK;
  if (n >= 0xFFFFFFFFull) return eng->fail(JY_ERANGE, "more than 2^32 - 1 values in one call");
  Tmp tmp(eng);
  u64 add = ~0ull;
  u32* verdict = nullptr;
  if (mem == JY_HOST) {
    JY_TRY(offs_check_host(eng, n, offs, JY_MAX_VALUE_LEN, "value", &add));
    JY_TRY(jy_stage_begin(eng));
    JY_TRY(stage_ragged(eng, 6, 7, bytes, offs, n, &bytes, &offs));
    JY_TRY(jy_stage_end(eng));
  } else {
    JY_TRY(check_dev(eng, tmp, n, nullptr, offs, nullptr, 0, &verdict));
  }
  u64 *dpre, *dlr;
  JY_TRY(tmp.out(&dpre, pre_out, n, out_mem));
  JY_TRY(tmp.out(&dlr, lr_out, n, out_mem));
  JY_TRY(pack_dev(eng, tmp, type, n, bytes, offs, add, verdict, dpre, dlr));
  if (out_mem == JY_HOST) {
    JY_HIP(eng, hipMemcpyAsync(pre_out, dpre, n * 8, hipMemcpyDeviceToHost, eng->stream));
    JY_HIP(eng, hipMemcpyAsync(lr_out, dlr, n * 8, hipMemcpyDeviceToHost, eng->stream));
    JY_HIP(eng, hipStreamSynchronize(eng->stream));
  }
  return JY_OK;
}

int32_t jy_counter_write_keys(jy_engine* eng, int32_t type, int32_t sign, uint32_t col, uint64_t n,
                              const uint8_t* key_bytes, const uint64_t* key_offs, const uint64_t* val, int32_t mem) {
  JY_HIP(eng, hipSetDevice(eng->device));
  if (type != JY_GCOUNT && type != JY_PNCOUNT) return eng->fail(JY_ETYPE, "not a counter type");
  const int w = type == JY_GCOUNT ? 0 : 1;
  if (sign < 0 || sign > w) return eng->fail(JY_EINVAL, "sign must be 0 (INC) or, for PNCOUNT, 1 (DEC)");
  if (col >= eng->rep_id.size()) return eng->fail(JY_ERANGE, "column names no registered replica");
  if (mem != JY_HOST && mem != JY_DEVICE) return eng->fail(JY_EINVAL, "mem must be JY_HOST or JY_DEVICE");
  if (n == 0) return JY_OK;
  if (n >= 0xFFFFFFFFull) return eng->fail(JY_ERANGE, "more than 2^32 - 1 commands in one call");
  Tmp tmp(eng);
  const void* dv = val;
  if (mem == JY_HOST) {
    JY_TRY(offs_check_host(eng, n, key_offs, kKeyLenMax, "key", nullptr));
    JY_TRY(jy_stage_begin(eng));
    JY_TRY(stage_ragged(eng, 0, 1, key_bytes, key_offs, n, &key_bytes, &key_offs));
    JY_TRY(jy_stage(eng, 5, val, n * 8, JY_HOST, &dv));
    JY_TRY(jy_stage_end(eng));
  } else {
    u32* verdict;
    JY_TRY(check_dev(eng, tmp, n, key_offs, nullptr, nullptr, 0, &verdict));
    JY_TRY(verdict_wait(eng, verdict));
  }
  u32* slots;
  JY_TRY(tmp.get(&slots, n + 2));
  JY_TRY(jy_keys_intern_dev(eng, type, n, key_bytes, key_offs, slots, nullptr, nullptr));
  JY_TRY(jy_counter_grow(eng, w, (u32)eng->rep_id.size(), eng->nkeys[type]));
  return jy_cnt_write(eng, w, sign, (u16)col, n, slots, static_cast<const u64*>(dv));
}

int32_t jy_treg_set_keys(jy_engine* eng, uint64_t n, const uint8_t* key_bytes, const uint64_t* key_offs,
                         const uint64_t* ts, const uint8_t* val_bytes, const uint64_t* val_offs, int32_t mem) {
  JY_HIP(eng, hipSetDevice(eng->device));
  if (mem != JY_HOST && mem != JY_DEVICE) return eng->fail(JY_EINVAL, "mem must be JY_HOST or JY_DEVICE");
  if (n == 0) return JY_OK;
  if (n >= 0xFFFFFFFFull) return eng->fail(JY_ERANGE, "more than 2^32 - 1 entries in one call");
  if (!key_offs || !ts || !val_offs) return eng->fail(JY_EINVAL, "SET needs keys, ts and values");
  Tmp tmp(eng);
  u64 add = ~0ull;
  u32* verdict = nullptr;
  const void* dt = ts;
  if (mem == JY_HOST) {
    JY_TRY(offs_check_host(eng, n, key_offs, kKeyLenMax, "key", nullptr));
    JY_TRY(offs_check_host(eng, n, val_offs, JY_MAX_VALUE_LEN, "value", &add));
    JY_TRY(jy_stage_begin(eng));
    JY_TRY(stage_ragged(eng, 0, 1, key_bytes, key_offs, n, &key_bytes, &key_offs));
    JY_TRY(jy_stage(eng, 4, ts, n * 8, JY_HOST, &dt));
    JY_TRY(stage_ragged(eng, 6, 7, val_bytes, val_offs, n, &val_bytes, &val_offs));
    JY_TRY(jy_stage_end(eng));
  } else {
    JY_TRY(check_dev(eng, tmp, n, key_offs, val_offs, nullptr, 0, &verdict));
  }
  // the values first: with device input their one wait brings the verdict
  // back before the directory walks a key
  u64* h;
  JY_TRY(tmp.get(&h, 2 * n));
  JY_TRY(pack_dev(eng, tmp, JY_TREG, n, val_bytes, val_offs, add, verdict, h, h + n));
  u32* slots;
  JY_TRY(tmp.get(&slots, n + 2));
  JY_TRY(jy_keys_intern_dev(eng, JY_TREG, n, key_bytes, key_offs, slots, nullptr, nullptr));
  return jy_treg_set_batch(eng, n, slots, static_cast<const u64*>(dt), h, h + n);
}

int32_t jy_tlog_write_keys(jy_engine* eng, uint64_t n, const uint8_t* op, const uint8_t* key_bytes,
                           const uint64_t* key_offs, const uint64_t* ts, const uint64_t* arg,
                           const uint8_t* val_bytes, const uint64_t* val_offs, int32_t mem) {
  JY_HIP(eng, hipSetDevice(eng->device));
  if (mem != JY_HOST && mem != JY_DEVICE) return eng->fail(JY_EINVAL, "mem must be JY_HOST or JY_DEVICE");
  if (n == 0) return JY_OK;
  if (n >= 0xFFFFFFFFull) return eng->fail(JY_ERANGE, "more than 2^32 - 1 commands in one call");
  if (!op || !key_offs) return eng->fail(JY_EINVAL, "a write batch needs ops and keys");
  Tmp tmp(eng);
  u64 add = ~0ull;
  u32* verdict = nullptr;
  const void *dop = op, *dt = ts, *da = arg;
  if (mem == JY_HOST) {
    JY_TRY(offs_check_host(eng, n, key_offs, kKeyLenMax, "key", nullptr));
    for (u64 i = 0; i < n; i++) {
      if (op[i] > JY_TLOG_CLR) return eng->fail(JY_EINVAL, "unknown TLOG write op");
      if (op[i] == JY_TLOG_INS && (!ts || !val_offs)) return eng->fail(JY_EINVAL, "INS needs ts and a value");
      if ((op[i] == JY_TLOG_TRIMAT && !ts) || (op[i] == JY_TLOG_TRIM && !arg))
        return eng->fail(JY_EINVAL, "TRIMAT needs ts, TRIM needs arg");
    }
    if (val_offs) JY_TRY(offs_check_host(eng, n, val_offs, JY_MAX_VALUE_LEN, "value", &add));
    JY_TRY(jy_stage_begin(eng));
    JY_TRY(stage_ragged(eng, 0, 1, key_bytes, key_offs, n, &key_bytes, &key_offs));
    JY_TRY(jy_stage(eng, 3, op, n, JY_HOST, &dop));
    if (ts) JY_TRY(jy_stage(eng, 4, ts, n * 8, JY_HOST, &dt));
    if (arg) JY_TRY(jy_stage(eng, 5, arg, n * 8, JY_HOST, &da));
    if (val_offs) JY_TRY(stage_ragged(eng, 6, 7, val_bytes, val_offs, n, &val_bytes, &val_offs));
    JY_TRY(jy_stage_end(eng));
  } else {
    if (!ts || !arg || !val_offs) return eng->fail(JY_EINVAL, "a device batch passes every column");
    JY_TRY(check_dev(eng, tmp, n, key_offs, val_offs, op, JY_TLOG_CLR, &verdict));
  }
  // columns a host batch left out read as zeros
  u64* h;
  JY_TRY(tmp.get(&h, 3 * n));
  if (!dt || !da || !val_offs) JY_HIP(eng, hipMemsetAsync(h, 0, 3 * n * 8, eng->stream));
  u64 *hpre = h, *hlr = h + n, *zero = h + 2 * n;
  if (val_offs) JY_TRY(pack_dev(eng, tmp, JY_TLOG, n, val_bytes, val_offs, add, verdict, hpre, hlr));
  if (!dt) dt = zero;
  if (!da) da = zero;
  u32* slots;
  JY_TRY(tmp.get(&slots, n + 2));
  JY_TRY(jy_keys_intern_dev(eng, JY_TLOG, n, key_bytes, key_offs, slots, nullptr, nullptr));
  return jy_tlog_write_ordered(eng, n, static_cast<const uint8_t*>(dop), slots, static_cast<const u64*>(dt),
                               static_cast<const u64*>(da), hpre, hlr);
}

int32_t jy_tlog_write_rounds(jy_engine* eng, uint64_t* out3) {
  out3[0] = eng->tlw_calls;
  out3[1] = eng->tlw_rounds_last;
  out3[2] = eng->tlw_rounds_total;
  return JY_OK;
}

}  // extern "C"
