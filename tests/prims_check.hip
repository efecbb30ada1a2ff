// prims_check.hip -- test-only entry points over the engine's device scan,
// select and sort primitives (jy_dscan.hpp, jy_sort.hpp, jy_scan.hpp) and the
// device round split built on them (jy_drounds.hpp), so that
// tests/test_prims_gpu.py can drive each one alone at the sizes its own
// constants decide.  The headers are included unchanged: what runs here is
// what the engine's callers run.  Built by `make -C jylis_amd primcheck` into
// tests/libjy_primcheck.so (links against libjylis_gpu.so for jy_scratch and
// jy_dscan_ctx); nothing here is part of include/jylis_gpu.h.
//
// Every entry point takes a live engine and device pointers, enqueues on the
// engine's stream, waits for that stream and returns the engine's status.
#include "../jylis_amd/csrc/jy_drounds.hpp"
#include "../jylis_amd/csrc/jy_dscan.hpp"
#include "../jylis_amd/csrc/jy_internal.hpp"
#include "../jylis_amd/csrc/jy_sort.hpp"

namespace {

int32_t finish(jy_engine* eng, int32_t rc) {
  JY_HIP(eng, hipStreamSynchronize(eng->stream));
  return rc;
}

template <class T, class Op>
int32_t scan_op(jy_engine* eng, int incl, u64 n, const T* in, T* out) {
  const jydscan::LdArr<T> ld{in};
  const jydscan::StArr<T> st{out};
  return incl ? jydscan::scan<Op, true>(eng, n, ld, st) : jydscan::scan<Op, false>(eng, n, ld, st);
}
template <class T>
int32_t scan_any(jy_engine* eng, int op, int incl, u64 n, const T* in, T* out) {
  if (op == 0) return finish(eng, scan_op<T, jydscan::OpSum>(eng, incl, n, in, out));
  if (op == 1) return finish(eng, scan_op<T, jydscan::OpMax>(eng, incl, n, in, out));
  return eng->fail(JY_EINVAL, "jyt_scan: op is 0 (sum) or 1 (max)");
}

struct FlagPred {
  const uint8_t* f;
  __device__ __forceinline__ bool operator()(u64 i) const { return f[i] != 0; }
};

// one wave per query (four to a workgroup, the way the engine's kernels call
// it with every wave of the workgroup)
__global__ __launch_bounds__(256) void k_last_le(const u64* __restrict__ offs, u64 n, u64 nq,
                                                 const u64* __restrict__ x, u64* __restrict__ out) {
  const u64 q = (u64)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= nq) return;  // wave-uniform
  const u64 k = jyscan::wave_last_le(offs, n, x[q]);
  if ((threadIdx.x & 63) == 0) out[q] = k;
}

template <int kT>
__global__ __launch_bounds__(kT) void k_block_excl(const u64* __restrict__ in, u64* __restrict__ prefix,
                                                   u64* __restrict__ total) {
  __shared__ u64 red[kT / 64];
  const u64 i = (u64)blockIdx.x * kT + threadIdx.x;
  u64 tot;
  const u64 pre = jyscan::block_excl<kT, u64>(in[i], red, tot);
  prefix[i] = pre;
  if (threadIdx.x == 0) total[blockIdx.x] = tot;
}

// a ticketed scan, one tile per workgroup (tools/mb_scan.hip's shape with the
// tile of jy_dscan.hpp): exclusive sums of u32 items; the sum stays < 2^40
constexpr int kLbThreads = 256;
constexpr int kLbPer = 8;
constexpr u64 kLbTile = (u64)kLbThreads * kLbPer;
__global__ __launch_bounds__(kLbThreads) void k_lookback_scan(const u32* __restrict__ in, u64* __restrict__ out, u64 n,
                                                              u32* tick, u64* status, u32 epoch) {
  __shared__ u64 red[kLbThreads / 64];
  __shared__ u64 pre;
  __shared__ u32 tk;
  const u32 t = jyscan::ticket(tick, &tk);
  if (t == gridDim.x - 1 && threadIdx.x == 0) *tick = 0;  // every other ticket is drawn by now (k_select)
  const u64 i0 = (u64)t * kLbTile + (u64)threadIdx.x * kLbPer;
  u64 v[kLbPer], s = 0;
#pragma unroll
  for (int u = 0; u < kLbPer; u++) {
    v[u] = s;
    s += i0 + u < n ? in[i0 + u] : 0;
  }
  u64 tot;
  const u64 off = jyscan::block_excl<kLbThreads, u64>(s, red, tot);
  const u64 p = jyscan::lookback(status, t, epoch, tot, &pre);
#pragma unroll
  for (int u = 0; u < kLbPer; u++)
    if (i0 + u < n) out[i0 + u] = p + off + v[u];
}

}  // namespace

extern "C" {

int32_t jyt_scan_u64(jy_engine* eng, int32_t op, int32_t incl, u64 n, const u64* in, u64* out) {
  return scan_any<u64>(eng, op, incl, n, in, out);
}
int32_t jyt_scan_u32(jy_engine* eng, int32_t op, int32_t incl, u64 n, const u32* in, u32* out) {
  return scan_any<u32>(eng, op, incl, n, in, out);
}

// the exclusive sum over the rows * W + 1 items of a row-major [rows][W]
// matrix taken column after column, in place; a[rows * W] = the grand total
int32_t jyt_scan_colmajor(jy_engine* eng, u64 rows, u64 W, u64* a) {
  return finish(eng, jydscan::scan<jydscan::OpSum, false>(eng, rows * W + 1, jydscan::LdColMajor{a, rows, W},
                                                           jydscan::StColMajor{a, rows, W}));
}

int32_t jyt_select_flags(jy_engine* eng, u64 n, const uint8_t* flags, u32* out, u32* count) {
  return finish(eng, jydscan::select(eng, n, FlagPred{flags}, out, count));
}

// *which = 0: the sorted keys are in a, 1: in b
int32_t jyt_sort_bits(jy_engine* eng, u64 n, u64* a, u64* b, u64* hist, u32 lo, u32 hi, int32_t* which) {
  u64* res = nullptr;
  const int32_t rc = jysort::sort_bits(eng, a, b, hist, n, lo, hi, &res);
  *which = res == a ? 0 : res == b ? 1 : -1;
  return finish(eng, rc);
}
u64 jyt_sort_hist_words(u64 n) { return jysort::hist_words(n); }
u32 jyt_sort_bits_for(u64 count) { return jysort::bits_for(count); }

// out[q] = the last k in [0, n] with offs[k] <= x[q] (offs[0..n] non-decreasing, offs[0] <= x[q])
int32_t jyt_last_le(jy_engine* eng, u64 n, const u64* offs, u64 nq, const u64* x, u64* out) {
  if (nq == 0) return finish(eng, JY_OK);
  hipLaunchKernelGGL(k_last_le, dim3((u32)((nq + 3) / 4)), dim3(256), 0, eng->stream, offs, n, nq, x, out);
  JY_HIP(eng, hipGetLastError());
  return finish(eng, JY_OK);
}

// nblocks workgroups of `threads` (256 or 1024) items each: every item's
// exclusive prefix within its workgroup, and each workgroup's total
int32_t jyt_block_excl(jy_engine* eng, u32 threads, u32 nblocks, const u64* in, u64* prefix, u64* total) {
  if (nblocks == 0) return finish(eng, JY_OK);
  if (threads == 256)
    hipLaunchKernelGGL(k_block_excl<256>, dim3(nblocks), dim3(256), 0, eng->stream, in, prefix, total);
  else if (threads == 1024)
    hipLaunchKernelGGL(k_block_excl<1024>, dim3(nblocks), dim3(1024), 0, eng->stream, in, prefix, total);
  else
    return eng->fail(JY_EINVAL, "jyt_block_excl: 256 or 1024 threads");
  JY_HIP(eng, hipGetLastError());
  return finish(eng, JY_OK);
}

// out[i] = in[0] + ... + in[i - 1], by tickets and the look-back of jy_scan.hpp
int32_t jyt_lookback_scan(jy_engine* eng, u64 n, const u32* in, u64* out) {
  const u64 tiles = n == 0 ? 1 : (n + kLbTile - 1) / kLbTile;
  u64* status;
  u32 *tick, epoch;
  JY_TRY(jy_dscan_ctx(eng, tiles, &status, &tick, &epoch));
  hipLaunchKernelGGL(k_lookback_scan, dim3((u32)tiles), dim3(kLbThreads), 0, eng->stream, in, out, n, tick, status,
                     epoch);
  JY_HIP(eng, hipGetLastError());
  return finish(eng, JY_OK);
}

// the device round split (jy_drounds.hpp) of n commands in device memory.
// Host outputs: ru = {R, U}; ro[0 .. R] the round offsets (room for n + 1);
// per unit j in round order its slot uslot[j] and its commands
// cmd[uoff[j] .. uoff[j + 1]) (room for n, n + 1 and n).
int32_t jyt_drounds(jy_engine* eng, u64 n, const u32* slot, const u32* idx, const uint8_t* op, u32 merge, u32 unit_max,
                    u32 sbits, u64* ru, u64* ro, u32* uslot, u64* uoff, u32* cmd) {
  Tmp tmp(eng);
  JyDRounds D;
  if (unit_max != 1 && unit_max != 64) return eng->fail(JY_EINVAL, "jyt_drounds: units of 1 or 64, as the engine's");
  JY_TRY(finish(eng, unit_max == 1 ? jy_drounds<1>(eng, tmp, n, slot, idx, op, (uint8_t)merge, sbits, &D)
                                   : jy_drounds<64>(eng, tmp, n, slot, idx, op, (uint8_t)merge, sbits, &D)));
  std::vector<u64> skey(n), ustart(D.U + 1), ul(D.U);
  JY_HIP(eng, hipMemcpy(skey.data(), D.skey, n * 8, hipMemcpyDeviceToHost));
  JY_HIP(eng, hipMemcpy(ustart.data(), D.ustart, (D.U + 1) * 8, hipMemcpyDeviceToHost));
  JY_HIP(eng, hipMemcpy(ul.data(), D.ul, D.U * 8, hipMemcpyDeviceToHost));
  ru[0] = D.R;
  ru[1] = D.U;
  std::copy(D.ro.begin(), D.ro.end(), ro);
  uoff[0] = 0;
  for (u64 j = 0, c = 0; j < D.U; j++) {
    const u32 u = (u32)ul[j];
    if (u >= D.U || ustart[u] >= ustart[u + 1] || ustart[u + 1] > n || c + (ustart[u + 1] - ustart[u]) > n)
      return eng->fail(JY_EINVAL, "jyt_drounds: a unit is out of range");
    uslot[j] = (u32)(skey[ustart[u]] >> 32);
    for (u64 p = ustart[u]; p < ustart[u + 1]; p++) cmd[c++] = (u32)skey[p];
    uoff[j + 1] = c;
  }
  return JY_OK;
}

// the epoch the next scan context counts on from
void jyt_dscan_epoch_set(jy_engine* eng, u32 v) { eng->dscan_epoch = v; }
u32 jyt_dscan_epoch_get(jy_engine* eng) { return eng->dscan_epoch; }

}  // extern "C"
