// ujson_put_check.cpp -- jylis_amd/csrc/jy_resp_in.hpp's ujson_value_plain,
// classify_opts and classify_all as plain C++, run sequentially over cases a
// file names.  A stand-alone program, never loaded into Python
// (tests/test_ujson_put_cpu.py builds it with the address and undefined-
// behaviour sanitizers and compares what it prints with
// tests/ujson_put_cases.py's reference).
//
//   ujson_put_check FILE    FILE holds one case a line:
//                             flags nwords len[0] .. len[nwords - 1] hex[0] .. hex[nwords - 1]
//                           the length of EVERY word and its bytes as hex: "-" an
//                           empty word, "?" a word that is a length alone (a null
//                           pointer: only its length may be looked at).  Prints,
//                           per case, three classes as `kind op num key val` --
//                           classify_all under the case's flags, under flags 0
//                           and under JY_RESP_UJSON_GET alone -- then whether
//                           classify_opts(.., 0) equals classify, and
//                           ujson_value_plain of the last word (-1: no bytes).
#include <cinttypes>
#include <cstdio>
#include <string>
#include <vector>

#include "../jylis_amd/csrc/jy_resp_in.hpp"

using namespace jyrin;

static bool same(const Class& a, const Class& b) {
  return a.kind == b.kind && a.op == b.op && a.num == b.num && a.key == b.key && a.val == b.val;
}

static void print(const Class& c) { std::printf("%u %u %" PRIu64 " %d %d ", c.kind, c.op, c.num, c.key, c.val); }

int main(int argc, char** argv) {
  static_assert(JY_CMD_UJSON_WRITE == 11 && JY_CMD_NKINDS == 11 && JY_CMD_NKINDS_ALL == 12, "the header's kinds");
  static_assert(JY_RESP_UJSON_GET == 1 && JY_RESP_UJSON_WRITE == 2, "the header's flags");
  static_assert(JY_UJSON_INS == 0 && JY_UJSON_RM == 1 && JY_UJSON_CLR == 2, "the ops a row carries");
  static_assert(kUjValueMax == 255 && kPathWord0 == 3 && kWordsRead == 5, "the cases put the value at words 3, 4, 5 and 9");
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
    // heap copies of exactly the word's bytes: the address sanitizer sees a read past a word
    std::vector<std::vector<uint8_t>> keep(nwords);
    std::vector<bool> has(nwords);
    for (u64 j = 0; j < nwords; j++) {
      char hex[4096];
      if (std::fscanf(f, "%4095s", hex) != 1) return 2;
      const std::string h = hex;
      has[j] = h != "?";
      if (h == "-" || h == "?") continue;
      for (size_t i = 0; i + 1 < h.size(); i += 2) keep[j].push_back((uint8_t)std::stoul(h.substr(i, 2), nullptr, 16));
      if (keep[j].size() != lens[j]) return 2;
    }
    const auto word = [&](u64 j) {
      return Word{j < nwords && has[j] && lens[j] ? keep[j].data() : nullptr, j < nwords ? lens[j] : 0};
    };
    Word w[kWordsRead];
    for (u32 j = 0; j < kWordsRead; j++) w[j] = word(j);
    const Word last = nwords ? word(nwords - 1) : Word{nullptr, 0};
    const bool last_has = nwords && has[nwords - 1];
    print(classify_all(nwords, w, lens.data(), flags, last_has ? &last : nullptr));
    print(classify_all(nwords, w, lens.data(), 0, last_has ? &last : nullptr));
    print(classify_all(nwords, w, lens.data(), JY_RESP_UJSON_GET));
    std::printf("%d %d\n", (int)same(classify_opts(nwords, w, 0), classify(nwords, w)),
                last_has ? (int)ujson_value_plain(last.p, last.len) : -1);
  }
  std::fclose(f);
  return 0;
}
