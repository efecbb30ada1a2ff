// jy_tlog_rules.hpp -- the TLOG write rules, stated once for the two kernels
// that judge commands: k_tlog_wprep (k_tlog.hip, a lane per command) and
// k_put_wprep (k_put.hip, a wave per unit of a key's commands).
//
// Write path: RepoTLOG.ins / trimat / trim / clr (repo_tlog.pony:85-111).
// Each command becomes a delta log for the state -- entries, and a cutoff --
// judged against the state as it is:
//   INS     the entry (ts, value); changes the state iff ts >= cutoff and the
//           entry is new (TLog.write)
//   TRIMAT  cutoff ts; changes iff ts > cutoff (raise_cutoff)
//   TRIM n  cutoff = ts of the n-th newest entry (n == 0: CLR; past the end:
//           nothing, as the reference's try swallows the bounds error)
//   CLR     cutoff = newest ts + 1 (U64 wraps), nothing on an empty log
// and, where the state changed, the same delta goes to the key's pending
// delta log (d.write / d.raise_cutoff(l.cutoff) of the reference).  Every
// command marks its key pending (_delta_for runs either way).
#pragma once

#include "jy_internal.hpp"

struct Ent {
  u64 t, p, l;
};

// sign of (pool[m] - x) in age order; value handles are read only on a tie
__device__ __forceinline__ int cmp_at(const TRec* __restrict__ pool, u64 m, const Ent& x,
                                      const uint8_t* __restrict__ arena) {
  const u64 t = pool[m].ts;
  if (t != x.t) return t > x.t ? 1 : -1;
  return jy_value_cmp(pool[m].pre, pool[m].lr, x.p, x.l, arena);
}

// INS: does the entry x change the log m?
__device__ __forceinline__ bool tlog_ins_changes(const TMeta& m, const TRec* __restrict__ pool,
                                                 const uint8_t* __restrict__ arena, const Ent& x) {
  if (x.t < m.cut) return false;
  // present? the log is ascending (ts, value) from base
  u64 lo = tm_base(m), hi = tm_base(m) + m.len;
  while (lo < hi) {
    const u64 mid = (lo + hi) >> 1;
    if (cmp_at(pool, mid, x, arena) < 0) lo = mid + 1;
    else hi = mid;
  }
  return !(lo < tm_base(m) + m.len && cmp_at(pool, lo, x, arena) == 0);
}

// TRIMAT / TRIM / CLR: the cutoff the command raises on the log m, and
// whether that changes the state.  TRIMAT hands its ts to the join whatever
// the state's cutoff; TRIM and CLR raise nothing unless the state changes.
// `ts` and `arg` are the command's cells, read only by the op that uses them.
__device__ __forceinline__ u64 tlog_cut_raise(uint8_t op, const u64& ts, const u64& arg, const TMeta& m,
                                              const TRec* __restrict__ pool, bool* changed) {
  u64 raise = 0;
  *changed = false;
  if (op == JY_TLOG_TRIMAT) {
    raise = ts;
    *changed = raise > m.cut;
  } else {
    const u64 cnt = op == JY_TLOG_CLR ? 0 : arg;
    if (cnt == 0) {
      if (m.len) {
        raise = m.newest + 1;
        *changed = raise > m.cut;
      }
    } else if (cnt - 1 < m.len) {
      raise = pool[tm_base(m) + m.len - cnt].ts;
      *changed = raise > m.cut;
    }
    if (!*changed) raise = 0;
  }
  return raise;
}
