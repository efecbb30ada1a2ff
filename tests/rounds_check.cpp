// rounds_check.cpp -- jy_rounds.hpp on its own, as a host program
// (tests/test_rounds_cpu.py builds it with the address and undefined-behaviour
// sanitizers and runs it).  Prints "ok" and returns 0, or names the first
// check that failed.
#include <cstdio>
#include <vector>

#include "../jylis_amd/csrc/jy_rounds.hpp"

static int failed = 0;
#define CHECK(cond)                                            \
  do {                                                         \
    if (!(cond)) {                                             \
      std::printf("line %d: %s\n", __LINE__, #cond);           \
      failed = 1;                                              \
    }                                                          \
  } while (0)

static std::vector<uint64_t> items(JyIdx ix) {
  std::vector<uint64_t> v;
  for (uint64_t k = 0; k < ix.size(); k++) v.push_back(ix[k]);
  return v;
}

int main() {
  using V = std::vector<uint64_t>;
  {  // nothing, and one item: one round, no slot is read for n = 0
    const JyRounds none(0, nullptr);
    CHECK(none.count == 1 && none.idx.empty() && none.start.empty() && none.round(0).size() == 0);
    const uint32_t s = 9;
    const JyRounds one(1, &s);
    CHECK(one.count == 1 && one.idx.empty() && one.start.empty());
    CHECK(items(one.round(0)) == V{0});
  }
  {  // distinct slots: one round, the batch as it is, no index array
    const uint32_t s[8] = {5, 0, 7, 0xFFFFFFFEu, 3, 1, 2, 4};
    const JyRounds r(8, s);
    CHECK(r.count == 1 && r.idx.empty() && r.start.empty());
    CHECK(r.round(0).p == nullptr);
    CHECK((items(r.round(0)) == V{0, 1, 2, 3, 4, 5, 6, 7}));
  }
  {  // [a,b,a,c,a,b,a]: later rounds are strict subsets, input order kept
    const uint32_t a = 40, b = 2, c = 11;
    const uint32_t s[7] = {a, b, a, c, a, b, a};
    const JyRounds r(7, s);
    CHECK(r.count == 4 && r.idx.size() == 7 && r.start.size() == 5);
    CHECK((items(r.round(0)) == V{0, 1, 3}));
    CHECK((items(r.round(1)) == V{2, 5}));
    CHECK((items(r.round(2)) == V{4}));
    CHECK((items(r.round(3)) == V{6}));
    // the gather: rows of a column, zeros for a null column
    const uint64_t col[7] = {10, 11, 12, 13, 14, 15, 16};
    CHECK((jy_rows(col, r.round(1)) == V{12, 15}));
    CHECK((jy_rows<uint64_t>(nullptr, r.round(0)) == V{0, 0, 0}));
    const uint8_t op[7] = {1, 2, 3, 4, 5, 6, 7};
    CHECK((jy_rows(op, r.round(0)) == std::vector<uint8_t>{1, 2, 4}));
    CHECK((jy_rows(s, r.round(1)) == std::vector<uint32_t>{a, b}));
  }
  {  // the gather over the batch as it is
    const uint32_t s[3] = {1, 2, 3};
    const uint64_t col[3] = {7, 8, 9};
    const JyRounds r(3, s);
    CHECK((jy_rows(col, r.round(0)) == V{7, 8, 9}));
    CHECK((jy_rows<uint64_t>(nullptr, r.round(0)) == V{0, 0, 0}));
  }
  {  // one slot 1,000 times: 1,000 rounds of one item, 1,000 indices in all
    const std::vector<uint32_t> s(1000, 77);
    const JyRounds r(s.size(), s.data());
    CHECK(r.count == 1000 && r.idx.size() == 1000 && r.start.size() == 1001);
    bool each = true;
    for (uint32_t k = 0; k < r.count; k++) each = each && r.round(k).size() == 1 && r.round(k)[0] == k;
    CHECK(each);
  }
  {  // the first repeat comes late: the items before it are round 0 too
    const uint32_t s[5] = {1, 2, 3, 4, 2};
    const JyRounds r(5, s);
    CHECK(r.count == 2);
    CHECK((items(r.round(0)) == V{0, 1, 2, 3}));
    CHECK((items(r.round(1)) == V{4}));
  }
  if (!failed) std::printf("ok\n");
  return failed;
}
