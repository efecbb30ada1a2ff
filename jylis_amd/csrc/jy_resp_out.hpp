// jy_resp_out.hpp -- the rules of assembling a heartbeat's REPLIES, stated once
// for the host and the device: which byte range of the reply pool a command
// takes, and where a connection's replies start.
//
// __host__ __device__ functions only, no HIP calls, in the manner of
// jy_resp.hpp and jy_resp_in.hpp: the reply assembly (k_resp_out.hip) runs them
// a lane per row, per host command and per connection, and
// tests/resp_out_check.cpp includes this file as plain C++ and runs them
// sequentially.
//
// THE POOL is one byte buffer.  Every command's reply is a range (offset,
// length) of it:
//   a read row    its group's reply bytes were written at the group's base by a
//                 jy_*_get_resp core, reply i of the group at reply_offs[i] ..
//                 reply_offs[i + 1] from there.  The offsets of all read groups
//                 share one array: group g's n + 1 offsets start at element
//                 group_offs[g] + g (every earlier group spends one closing
//                 element), so row r of group g reads elements r + g and
//                 r + g + 1.
//   a write row   the five bytes +OK\r\n, which the pool holds once
//   a HOST command  the answer the host gave, uploaded with all the others
// THE OUTPUT is the commands' ranges back to back in command order, which is
// connection-major: connection c's replies start at the output offset of the
// first command whose connection is c or later.  A connection without a
// complete command so gets an empty range wherever it lies, and the entry
// past the last connection is the total.
// The only loops are the two bisections.
#pragma once

#include <cstdint>

#include "../../include/jylis_gpu.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define JY_ROUT_HD __host__ __device__ __forceinline__
#else
#define JY_ROUT_HD inline
#endif

namespace jyrout {

typedef uint64_t u64;
typedef uint32_t u32;

constexpr u64 kOkLen = 5;  // +OK\r\n
constexpr uint8_t kOk[kOkLen] = {'+', 'O', 'K', '\r', '\n'};

struct Range {
  u64 off, len;
};

// the kinds whose keyed call is a jy_*_get_resp: their rows take reply bytes
JY_ROUT_HD bool kind_reads(u32 kind) {
  return kind == JY_CMD_GCOUNT_GET || kind == JY_CMD_PNCOUNT_GET || kind == JY_CMD_TREG_GET ||
         kind == JY_CMD_TLOG_READ || kind == JY_CMD_UJSON_GET;
}

// the group row r < group_offs[G] lies in: the largest g with group_offs[g] <= r
JY_ROUT_HD u64 group_of(const u64* group_offs, u64 G, u64 r) {
  u64 lo = 0, hi = G;
  while (hi - lo > 1) {
    const u64 mid = lo + (hi - lo) / 2;
    if (group_offs[mid] <= r) lo = mid; else hi = mid;
  }
  return lo;
}

// the pool range of row r, a row of group g of kind `kind`: base = where the
// group's reply bytes start in the pool, ro = the shared offsets array
JY_ROUT_HD Range row_range(u32 kind, u64 ok_off, u64 base, const u64* ro, u64 r, u64 g) {
  if (!kind_reads(kind)) return Range{ok_off, kOkLen};
  const u64 a = ro[r + g], b = ro[r + g + 1];
  return Range{base + a, b - a};
}

// the pool range of host command h: answers back to back from `base`, hoffs[H + 1]
JY_ROUT_HD Range host_range(u64 base, const u64* hoffs, u64 h) {
  return Range{base + hoffs[h], hoffs[h + 1] - hoffs[h]};
}

// the first command k <= ncmd with cmd_conn[k] >= c (ncmd: none), cmd_conn ascending
JY_ROUT_HD u64 first_cmd_of(const u32* cmd_conn, u64 ncmd, u64 c) {
  u64 lo = 0, hi = ncmd;  // the answer lies in [lo, hi]
  while (lo < hi) {
    const u64 mid = lo + (hi - lo) / 2;
    if (cmd_conn[mid] >= c) hi = mid; else lo = mid + 1;
  }
  return lo;
}

}  // namespace jyrout
