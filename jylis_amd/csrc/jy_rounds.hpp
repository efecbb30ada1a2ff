// jy_rounds.hpp -- the host round split of a batch that may repeat slots, and
// the column gather that goes with it (abi_logs.hip: the host-array forms of
// the TLOG and UJSON converge and write calls).  Plain C++: no HIP include, so
// a host-only program can test it.
//
// A merge takes one delta per key (the sender's `_deltas` Map guarantees it
// between nodes).  A host call that repeats a slot is therefore applied in
// ROUNDS: item i goes to round r when r earlier items of the call have its
// slot.  Every round holds each slot at most once, a slot's items keep their
// order across the rounds, and round r + 1 is never larger than round r.
#pragma once

#include <cstdint>
#include <unordered_map>
#include <vector>

// a span of item indices; p == nullptr stands for 0 .. n - 1 as they are
struct JyIdx {
  const uint64_t* p;
  uint64_t n;
  uint64_t size() const { return n; }
  uint64_t operator[](uint64_t k) const { return p ? p[k] : k; }
};

struct JyRounds {
  uint32_t count = 1;
  // the items round by round, in input order inside a round: round r is
  // idx[start[r] .. start[r + 1]).  Both stay empty when no slot repeats (the
  // one round is then the batch as it is).
  std::vector<uint64_t> idx, start;

  // O(n) work and memory.  The map is sized to the call, not to the interned
  // keys: the host mirror makes many one-key calls.
  JyRounds(uint64_t n, const uint32_t* slot) : n_(n) {
    if (n <= 1) return;
    std::vector<uint32_t> occ;  // occurrence number of each item, made at the first repeat
    {
      std::unordered_map<uint32_t, uint32_t> seen;
      seen.reserve(n);
      for (uint64_t i = 0; i < n; i++) {
        const uint32_t o = seen[slot[i]]++;
        if (o == 0) continue;
        if (occ.empty()) occ.assign(n, 0);
        occ[i] = o;
        if (o + 1 > count) count = o + 1;
      }
    }
    if (count == 1) return;
    start.assign((uint64_t)count + 1, 0);
    for (uint64_t i = 0; i < n; i++) start[occ[i] + 1]++;
    for (uint32_t r = 0; r < count; r++) start[r + 1] += start[r];
    idx.resize(n);
    std::vector<uint64_t> fill(start.begin(), start.end() - 1);
    for (uint64_t i = 0; i < n; i++) idx[fill[occ[i]]++] = i;
  }

  JyIdx round(uint32_t r) const {
    if (count == 1) return JyIdx{nullptr, n_};
    return JyIdx{idx.data() + start[r], start[r + 1] - start[r]};
  }

 private:
  uint64_t n_;
};

// the rows `ix` of a column, or zeros where the column is null
template <class T>
std::vector<T> jy_rows(const T* col, JyIdx ix) {
  std::vector<T> out(ix.size());
  if (col)
    for (uint64_t k = 0; k < ix.size(); k++) out[k] = col[ix[k]];
  return out;
}
