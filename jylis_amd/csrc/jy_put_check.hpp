// jy_put_check.hpp -- what every keyed write does to its input before a kernel
// loops over a length (k_put.hip, k_uj_put.hip): the check of a command table
// in device memory, its verdict as the call's return, and the staging of a
// ragged host column.  A key, a TREG / TLOG value and a UJSON leaf share one
// length limit, 2^24 - 1 bytes (the length field of an lr handle).
#pragma once

#include "jy_wire.hpp"

namespace {

constexpr u64 kKeyLenMax = JY_LR_LEN_MASK;
static_assert(kKeyLenMax == JY_MAX_VALUE_LEN, "keys and values share one length limit");

// verdict bits: 1 = offsets not ascending, 2 = a length over the limit,
// 4 = an unknown op.  One ragged column's bits for the item [a, b):
__host__ __device__ inline u32 put_offs_bits(u64 a, u64 b) { return b < a ? 1u : b - a > kKeyLenMax ? 2u : 0u; }

// any of koffs / voffs / op may be null
static __global__ __launch_bounds__(kThreads) void k_put_check(u64 n, const u64* __restrict__ koffs,
                                                               const u64* __restrict__ voffs,
                                                               const uint8_t* __restrict__ op, u32 op_max,
                                                               u32* __restrict__ verdict) {
  const u64 i = gid();
  if (i >= n) return;
  u32 bad = 0;
  if (koffs) bad |= put_offs_bits(koffs[i], koffs[i + 1]);
  if (voffs) bad |= put_offs_bits(voffs[i], voffs[i + 1]);
  if (op && op[i] > op_max) bad |= 4;
  if (bad) atomicOr(verdict, bad);
}

// a verdict word as the call's return: JY_EINVAL ranks over JY_ERANGE
inline int32_t verdict_rc(jy_engine* eng, u32 v) {
  if (v & 5) return eng->fail(JY_EINVAL, v & 4 ? "unknown write op" : "offsets do not ascend");
  if (v & 2) return eng->fail(JY_ERANGE, "a key, a value or a leaf is longer than 2^24 - 1 bytes");
  return JY_OK;
}

// the check kernel with a verdict word of its own, and the wait of a call
// that has nothing else to read back with it
inline int32_t check_dev(jy_engine* eng, Tmp& tmp, u64 n, const u64* koffs, const u64* voffs, const uint8_t* op,
                         u32 op_max, u32** verdict) {
  JY_TRY(tmp.get(verdict, 2));
  JY_HIP(eng, hipMemsetAsync(*verdict, 0, 8, eng->stream));
  LAUNCH(k_put_check, n, n, koffs, voffs, op, op_max, *verdict);
  return JY_OK;
}
inline int32_t verdict_wait(jy_engine* eng, const u32* verdict) {
  u64* pin = eng->pin_total;
  pin[0] = 0;
  JY_HIP(eng, hipMemcpyAsync(pin, verdict, 4, hipMemcpyDeviceToHost, eng->stream));
  JY_HIP(eng, hipStreamSynchronize(eng->stream));
  return verdict_rc(eng, (u32)pin[0]);
}

// a ragged host column (bytes, offs[0 .. n]) staged in slots `ib` and `io`;
// *db counts from `bytes`, as the offsets do (only offs[0] .. offs[n] travel)
inline int32_t stage_ragged(jy_engine* eng, int ib, int io, const uint8_t* bytes, const u64* offs, u64 n,
                            const uint8_t** db, const u64** dofs) {
  const void *b, *o;
  JY_TRY(jy_stage(eng, ib, bytes + offs[0], offs[n] - offs[0], JY_HOST, &b));
  JY_TRY(jy_stage(eng, io, offs, (n + 1) * 8, JY_HOST, &o));
  *db = static_cast<const uint8_t*>(b) - offs[0];
  *dofs = static_cast<const u64*>(o);
  return JY_OK;
}

}  // namespace
