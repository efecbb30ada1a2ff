// resp_ujson_check.cpp -- jylis_amd/csrc/jy_resp_in.hpp's classify_opts and
// classify_all as plain C++, run sequentially over cases a file names.  A
// stand-alone program, never loaded into Python (tests/test_resp_ujson_cpu.py
// builds it with the address and undefined-behaviour sanitizers and compares
// what it prints with tests/resp_ujson_cases.py's reference).
//
//   resp_ujson_check FILE    FILE holds one case a line:
//                              flags nwords len[0] .. len[nwords - 1] nhead hex[0] .. hex[nhead - 1]
//                            the length of EVERY word, and the bytes of the first
//                            nhead <= kWordsRead words as hex ("-": empty).  A word
//                            without bytes has a null pointer: only its length may
//                            be looked at.  Prints, per case,
//                              kind op num key val same
//                            same = classify_opts(.., 0) equals classify field by field.
#include <cinttypes>
#include <cstdio>
#include <string>
#include <vector>

#include "../jylis_amd/csrc/jy_resp_in.hpp"

using namespace jyrin;

static bool same(const Class& a, const Class& b) {
  return a.kind == b.kind && a.op == b.op && a.num == b.num && a.key == b.key && a.val == b.val;
}

int main(int argc, char** argv) {
  static_assert(JY_CMD_UJSON_GET == 10 && JY_CMD_NKINDS == 11 && JY_RESP_UJSON_GET == 1, "the header's values");
  static_assert(kPathWord0 == 3 && kWordsRead == 5, "the cases put a segment at word 3 and at word 7");
  if (argc < 2) return 2;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  unsigned flags;
  unsigned long long nwords;
  while (std::fscanf(f, "%u %llu", &flags, &nwords) == 2) {
    std::vector<u64> lens(nwords);
    for (auto& x : lens) {
      unsigned long long v;
      if (std::fscanf(f, "%llu", &v) != 1) return 2;
      x = v;
    }
    unsigned nhead;
    if (std::fscanf(f, "%u", &nhead) != 1 || nhead > kWordsRead) return 2;
    std::vector<std::vector<uint8_t>> keep(nhead);  // heap copies: the address sanitizer sees a read past a word
    for (auto& b : keep) {
      char hex[4096];
      if (std::fscanf(f, "%4095s", hex) != 1) return 2;
      const std::string h = hex;
      if (h == "-") continue;
      for (size_t i = 0; i + 1 < h.size(); i += 2) b.push_back((uint8_t)std::stoul(h.substr(i, 2), nullptr, 16));
    }
    Word w[kWordsRead];
    for (u32 j = 0; j < kWordsRead; j++) {
      const u64 len = j < nwords ? lens[j] : 0;
      // a head word's bytes must be all there; any other word is a length alone
      const bool has = j < nhead && keep[j].size() == len;
      w[j] = Word{has && len ? keep[j].data() : nullptr, len};
    }
    const Class c = classify_all(nwords, w, lens.data(), flags);
    const bool eq = same(classify_opts(nwords, w, 0), classify(nwords, w));
    std::printf("%u %u %" PRIu64 " %d %d %d\n", c.kind, c.op, c.num, c.key, c.val, eq ? 1 : 0);
  }
  std::fclose(f);
  return 0;
}
