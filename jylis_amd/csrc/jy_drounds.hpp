// jy_drounds.hpp -- the device round split of a batch that may repeat slots:
// the device counterpart of JyRounds (jy_rounds.hpp), for the keyed writes
// whose commands never leave the device (k_put.hip: TLOG, k_uj_put.hip: UJSON).
//
// The commands are grouped by slot (jy_sort.hpp: slot << 32 | command, only the
// slot bits sorted, so a slot's commands keep their call order), each slot's
// run is cut into UNITS -- up to kUnit consecutive commands of the one op
// that merges, or one command of any other op -- and the j-th unit of every
// slot goes to round j.  A round holds each slot at most once, in slot order;
// round r + 1 is never larger than round r.  With kUnit = 1 a unit is a
// command and its round is the number of earlier commands of its slot, which
// is JyRounds' rule.
//
// One host wait brings back the round count, the unit count and the first
// kRoundsInline round offsets; a batch with more rounds pays a second copy.
// Ordinary vector stores; the atomics: the rounds' counts and the round count.
#pragma once

#include "jy_sort.hpp"
#include "jy_wire.hpp"

namespace {

constexpr u64 kRoundsInline = 4096;  // rounds whose offsets come back with the round count in one copy

struct JyDRounds {
  u64 R = 0, U = 0;     // rounds, units
  std::vector<u64> ro;  // round r is ul[ro[r] .. ro[r + 1]); ro[R] = U
  // device arrays, the caller's Tmp holds them:
  const u64* skey = nullptr;    // the commands sorted by slot: slot << 32 | command
  const u64* ustart = nullptr;  // unit u is skey[ustart[u] .. ustart[u + 1]); units count in slot order
  const u64* ul = nullptr;      // the units in round order, slot order inside a round: (u32)ul[j] = u
};

static __global__ __launch_bounds__(kThreads) void k_dr_keys(const u32* __restrict__ slot, const u32* __restrict__ idx,
                                                             u64 n, u64* __restrict__ key) {
  const u64 j = gid();
  if (j >= n) return;
  const u32 i = idx ? idx[j] : (u32)j;
  key[j] = (u64)slot[i] << 32 | i;
}

// over the sorted commands: where a stretch starts -- a slot's first command
// and, with `op`, a command that is not `merge` or follows one that is not --
// as position + 1, else 0
static __global__ __launch_bounds__(kThreads) void k_dr_stretch(const u64* __restrict__ skey,
                                                                const uint8_t* __restrict__ op, uint8_t merge, u64 n,
                                                                u64* __restrict__ sst) {
  const u64 p = gid();
  if (p >= n) return;
  const u64 k = skey[p];
  bool start = p == 0;
  if (!start) {
    const u64 q = skey[p - 1];
    start = (q >> 32) != (k >> 32) || (op && (op[(u32)k] != merge || op[(u32)q] != merge));
  }
  sst[p] = start ? p + 1 : 0;
}

template <u32 kUnit>
struct LdUnitFlag {  // 1 where a unit starts: every kUnit commands of a stretch
  const u64* sst;    // inclusive max scan of k_dr_stretch's marks
  __device__ __forceinline__ u64 operator()(u64 p) const { return (p + 1 - sst[p]) % kUnit == 0; }
};
struct LdHeadUnit {  // a slot's first command carries its unit id, the others 0
  const u64* skey;
  const u64* uid;
  __device__ __forceinline__ u64 operator()(u64 p) const {
    return (p == 0 || (skey[p - 1] >> 32) != (skey[p] >> 32)) ? uid[p] : 0;
  }
};

// per unit u (0-based, in slot order): its first sorted position and its round
// (its ordinal within its slot); the units of each round counted, the largest
// round + 1 kept in info[0], the units in info[1]; ustart[units] = n.  kUnit
// 1 (uid, huid null): unit p is command p, its round its place in its stretch.
template <u32 kUnit>
__global__ __launch_bounds__(kThreads) void k_dr_units(const u64* __restrict__ sst, const u64* __restrict__ uid,
                                                       const u64* __restrict__ huid, u64 n, u64* __restrict__ ustart,
                                                       u64* __restrict__ ukey, u64* __restrict__ rcnt,
                                                       unsigned long long* __restrict__ info) {
  constexpr bool one = kUnit == 1;
  const u64 p = gid();
  if (p >= n) return;
  const u64 at = p + 1 - sst[p];  // < n
  if (at % kUnit == 0) {
    const u64 u = one ? p : uid[p] - 1, round = one ? at : uid[p] - huid[p];
    ustart[u] = p;
    ukey[u] = round << 32 | u;
    atomicAdd(reinterpret_cast<unsigned long long*>(rcnt + round), 1ull);
    atomicMax(info, (unsigned long long)(round + 1));
  }
  if (p == n - 1) {
    const u64 units = one ? n : uid[p];
    ustart[units] = n;
    info[1] = units;
  }
}

// Split the n commands idx[0 .. n) (idx null: 0 .. n - 1; 1 <= n < 2^32 - 1)
// by their slots, slot[i] < 2^sbits.  Consecutive commands of a slot whose
// op[i] == merge share a unit of up to kUnit; with kUnit == 1 `op` is not
// read and neither the unit-id nor the head-unit scan is launched.
template <u32 kUnit>
int32_t jy_drounds(jy_engine* eng, Tmp& tmp, u64 n, const u32* slot, const u32* idx, const uint8_t* op, uint8_t merge,
                   u32 sbits, JyDRounds* out) {
  constexpr bool one = kUnit == 1;
  // one allocation; info sits between the counts and their offsets: one memset, one copy
  const u64 w = n + 2, hw = jysort::hist_words(n);
  u64* g;
  JY_TRY(tmp.get(&g, (one ? 7 : 9) * w + hw + 2));
  u64 *ka = g, *kb = ka + w, *sst = kb + w, *ustart = sst + w, *ukey = ustart + w, *rcnt = ukey + w, *info = rcnt + w,
      *roff = info + 2, *hist = roff + w, *uid = one ? nullptr : hist + hw, *huid = one ? nullptr : uid + w;
  LAUNCH(k_dr_keys, n, slot, idx, n, ka);
  u64* skey;
  JY_TRY(jysort::sort_bits(eng, ka, kb, hist, n, 32, 32 + sbits, &skey));
  u64* spare = skey == ka ? kb : ka;
  LAUNCH(k_dr_stretch, n, (const u64*)skey, one ? nullptr : op, merge, n, sst);
  JY_TRY((jydscan::scan<jydscan::OpMax, true>(eng, n, jydscan::LdArr<u64>{sst}, jydscan::StArr<u64>{sst})));
  if constexpr (!one) {
    JY_TRY((jydscan::scan<jydscan::OpSum, true>(eng, n, LdUnitFlag<kUnit>{sst}, jydscan::StArr<u64>{uid})));
    JY_TRY((jydscan::scan<jydscan::OpMax, true>(eng, n, LdHeadUnit{skey, uid}, jydscan::StArr<u64>{huid})));
  }
  JY_HIP(eng, hipMemsetAsync(rcnt, 0, (w + 2) * 8, eng->stream));
  LAUNCH(k_dr_units<kUnit>, n, (const u64*)sst, (const u64*)uid, (const u64*)huid, n, ustart, ukey, rcnt,
         reinterpret_cast<unsigned long long*>(info));
  JY_TRY(jy_scan_u64(eng, rcnt, roff, n));
  // the round count, the unit count and the first rounds' offsets: one wait
  const u64 nin = std::min<u64>(n, kRoundsInline) + 1;
  std::vector<u64> h(2 + nin);
  JY_HIP(eng, hipMemcpyAsync(h.data(), info, (2 + nin) * 8, hipMemcpyDeviceToHost, eng->stream));
  JY_HIP(eng, hipStreamSynchronize(eng->stream));
  const u64 R = out->R = h[0], U = out->U = h[1];
  if (R == 0 || R > n || U == 0 || U > n) return eng->fail(JY_EINVAL, "keyed write: the grouping is inconsistent");
  std::vector<u64>& ro = out->ro;
  ro.assign(h.begin() + 2, h.begin() + 2 + std::min(nin, R + 1));
  if (R + 1 > nin) {
    ro.resize(R + 1);
    JY_HIP(eng, hipMemcpyAsync(ro.data() + nin, roff + nin, (R + 1 - nin) * 8, hipMemcpyDeviceToHost, eng->stream));
    JY_HIP(eng, hipStreamSynchronize(eng->stream));
  }
  if (ro[0] != 0 || ro[R] != U) return eng->fail(JY_EINVAL, "keyed write: the rounds do not cover the units");
  // the units in round order (stable: slot order inside a round; one round: no pass)
  u64* ul;
  JY_TRY(jysort::sort_bits(eng, ukey, spare, hist, U, 32, 32 + jysort::bits_for(R), &ul));
  out->skey = skey;
  out->ustart = ustart;
  out->ul = ul;
  return JY_OK;
}

}  // namespace
