// leaf_host_check -- the host side of jylis_amd/csrc/jy_leaf.hpp, checked
// without a GPU: the handle hash against a table of (encoding, handle) pairs
// and the length guard on the malformed shapes.
//
//   c++ -std=c++17 -O1 -o leaf_host_check tools/leaf_host_check.cpp
//   leaf_host_check TABLE     TABLE: one "<encoding in hex> <handle in hex>" per line
//
// Prints "ok <pairs>" and exits 0, or names every mismatch and exits 1.
// (tests/test_ujson_leaves_cpu.py writes the table from jylis_amd.ujson_doc.)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../jylis_amd/csrc/jy_leaf.hpp"

static int bad = 0;

struct Words {  // bytes i .. i + m - 1 as a little-endian word (a little-endian host)
  const uint8_t* p;
  uint64_t operator()(uint64_t i, uint64_t m) const {
    uint64_t w = 0;
    std::memcpy(&w, p + i, m);
    return w;
  }
};

static void expect(bool ok, const char* what) {
  if (ok) return;
  std::printf("FAILED: %s\n", what);
  bad++;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s TABLE\n", argv[0]);
    return 2;
  }
  std::ifstream in(argv[1]);
  if (!in) {
    std::fprintf(stderr, "cannot read %s\n", argv[1]);
    return 2;
  }
  std::string hex, want;
  unsigned long pairs = 0;
  while (in >> hex >> want) {
    if (hex.size() % 2) {
      std::printf("FAILED: odd hex string on line %lu\n", pairs + 1);
      return 1;
    }
    std::vector<uint8_t> b(hex.size() / 2);
    for (size_t i = 0; i < b.size(); i++) b[i] = (uint8_t)std::stoul(hex.substr(2 * i, 2), nullptr, 16);
    const uint64_t h = jy_leaf_hash(b.data(), b.size());
    const uint64_t w = std::stoull(want, nullptr, 16);
    if (h != w) {
      std::printf("FAILED: pair %lu (%zu bytes): hash %016llx, table %016llx\n", pairs, b.size(),
                  (unsigned long long)h, (unsigned long long)w);
      bad++;
    }
    // word loads, as the kernels hash (jy_leaf_hash_ld), give the same handle
    if (jy_leaf_hash_ld(Words{b.data()}, b.size()) != h) {
      std::printf("FAILED: pair %lu: the word-at-a-time hash differs from the byte-at-a-time one\n", pairs);
      bad++;
    }
    uint64_t len = 0;
    if (!jy_leaf_len(0, b.size(), &len) || len != b.size()) {
      std::printf("FAILED: pair %lu: a %zu-byte leaf fails the length guard\n", pairs, b.size());
      bad++;
    }
    pairs++;
  }
  uint64_t len = 77;
  expect(!jy_leaf_len(10, 9, &len) && len == 0, "a decreasing offset pair is malformed, length 0");
  expect(!jy_leaf_len(1ull << 40, 5, &len) && len == 0, "a far decreasing pair does not wrap into a length");
  expect(!jy_leaf_len(8, 11, &len) && len == 0, "a length of 3 is malformed");
  expect(jy_leaf_len(8, 12, &len) && len == 4, "a length of 4 is the shortest leaf");
  expect(!jy_leaf_len(0, 1ull << 24, &len) && len == 0, "a length of 2^24 is malformed");
  expect(jy_leaf_len(5, 5 + (1ull << 24) - 1, &len) && len == (1ull << 24) - 1, "a length of 2^24 - 1 is the longest leaf");
  expect(jy_leaf_fold(kLeafFnvBasis, 0, 0) == kLeafFnvBasis, "folding no bytes leaves the hash");
  for (uint32_t lg = 10; lg <= 40; lg += 10) {
    const uint64_t mask = (1ull << lg) - 1;
    expect(jy_leaf_start(~0ull, 64 - lg) <= mask && jy_leaf_start(1, 64 - lg) <= mask, "a start position lies in the table");
    expect(jy_leaf_next(mask, mask) == 0 && jy_leaf_next(0, mask) == 1, "the probe step wraps at the table's end");
  }
  if (bad) return 1;
  std::printf("ok %lu\n", pairs);
  return 0;
}
