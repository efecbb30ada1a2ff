// jy_resp_in.hpp -- the rules of a RESP REQUEST, stated once for the host and
// the device: what a token is, how a decimal parses, and which keyed call a
// command's words belong to.
//
// __host__ __device__ functions only, no HIP calls, in the manner of
// jy_resp.hpp: the request decoder (k_resp_in.hip) runs them a lane per byte,
// per token and per command, and tests/resp_in_check.cpp includes this file as
// plain C++ and runs them sequentially.
//
// TOKENS.  A request is an array of bulk strings,
//     *<n>\r\n   then n times   $<len>\r\n<len bytes>\r\n
// and nothing else: an inline command is malformed.  <n> and <len> are 1 to 20
// decimal digits without sign or blanks, leading zeros accepted, a value over
// 2^64 - 1 malformed ($-1 and *-1 therefore too).  token_at judges the token
// that starts at p, of which `avail` bytes belong to the connection:
//   complete     end = its length; a bulk string's bytes start at `body`
//   incomplete   the connection's bytes end before the token can be decided
//                or finished
//   malformed    a definite violation in the bytes that are present: another
//                first byte, a non-digit, a 21st digit, a missing \r\n where
//                the byte is there
// `type` is set from the first byte whenever that byte is '*' or '$', also for
// an incomplete token: a '$' where a header must stand is a violation before
// the string is complete.
// The only loop is over one number's at most 20 digits; a bulk string's
// length is compared with `avail`, never walked, and never added to anything
// before that comparison.
#pragma once

#include <cstdint>

#include "../../include/jylis_gpu.h"

#if defined(__HIPCC__)
#define JY_RIN_HD __host__ __device__ __forceinline__
#else
#define JY_RIN_HD inline
#endif

namespace jyrin {

typedef uint64_t u64;
typedef uint32_t u32;

enum : u32 { kComplete = 0, kIncomplete = 1, kMalformed = 2 };
enum : u32 { kHeader = 0, kBulk = 1, kNoType = 2 };

// the longest key or value a keyed call takes (2^24 - 1 bytes)
constexpr u64 kMaxKeyedLen = (1ull << 24) - 1;

struct Token {
  u32 status;  // kComplete / kIncomplete / kMalformed
  u32 type;    // kHeader / kBulk, kNoType when the first byte is neither
  u64 val;     // a complete token's <n> or <len>
  u64 body;    // a complete bulk string: where its bytes start
  u64 end;     // a complete token's length
};

JY_RIN_HD Token token_at(const uint8_t* p, u64 avail) {
  Token t{kIncomplete, kNoType, 0, 0, 0};
  if (avail == 0) return t;
  const uint8_t c0 = p[0];
  if (c0 != '*' && c0 != '$') {
    t.status = kMalformed;
    return t;
  }
  t.type = c0 == '*' ? kHeader : kBulk;
  u64 v = 0, i = 1;
  u32 nd = 0;
  for (;; i++) {  // at most 20 digits and the \r
    if (i >= avail) return t;
    const uint8_t c = p[i];
    if (c >= '0' && c <= '9') {
      const u64 d = (u64)(c - '0');
      if (++nd > 20 || v > (~0ull - d) / 10) {
        t.status = kMalformed;
        return t;
      }
      v = v * 10 + d;
      continue;
    }
    if (c != '\r' || nd == 0) {
      t.status = kMalformed;
      return t;
    }
    break;
  }
  if (i + 1 >= avail) return t;
  if (p[i + 1] != '\n') {
    t.status = kMalformed;
    return t;
  }
  const u64 body = i + 2;  // <= avail
  t.val = v;
  if (t.type == kHeader) {
    t.status = kComplete;
    t.end = body;
    return t;
  }
  const u64 rem = avail - body;
  if (v >= rem) return t;  // the bytes, or the \r after them, are not there yet
  if (p[body + v] != '\r') {
    t.status = kMalformed;
    return t;
  }
  if (v + 1 >= rem) return t;
  if (p[body + v + 1] != '\n') {
    t.status = kMalformed;
    return t;
  }
  t.status = kComplete;
  t.body = body;
  t.end = body + v + 2;
  return t;
}

// NUMBERS.  Pony String.u64()? / i64()? as host_repo.hip restates them: the
// whole string is decimal digits, 1 to 20 of them, no overflow; i64 takes one
// leading '+' or '-', and its magnitude must fit.
JY_RIN_HD bool parse_u64(const uint8_t* p, u64 len, u64* out) {
  if (len == 0 || len > 20) return false;
  u64 v = 0;
  for (u64 i = 0; i < len; i++) {
    const uint8_t c = p[i];
    if (c < '0' || c > '9') return false;
    const u64 d = (u64)(c - '0');
    if (v > (~0ull - d) / 10) return false;
    v = v * 10 + d;
  }
  *out = v;
  return true;
}
JY_RIN_HD bool parse_i64(const uint8_t* p, u64 len, int64_t* out) {
  if (len == 0) return false;
  const bool neg = p[0] == '-', sign = neg || p[0] == '+';
  u64 m;
  if (!parse_u64(p + (sign ? 1 : 0), len - (sign ? 1 : 0), &m)) return false;
  if (neg ? m > (1ull << 63) : m > (u64)INT64_MAX) return false;
  *out = neg ? (int64_t)(0 - m) : (int64_t)m;
  return true;
}

// CLASSIFICATION.  A command's words -> the keyed call it feeds
// (include/jylis_gpu.h JY_CMD_*), by exact, case-sensitive names as
// jyh_db_apply and the Repo*::apply bodies compare them; words beyond those a
// command reads are ignored, as Cmd ignores them.  Everything a keyed call
// does not exist for is JY_CMD_HOST: another type or op, a missing word, a
// number that does not parse (TLOG GET's count alone reads as "all" then,
// repo_tlog.pony:49-50), no word at all, a key or value over kMaxKeyedLen.
struct Word {
  const uint8_t* p;
  u64 len;
};
constexpr u32 kWordsRead = 5;  // type, op, key and up to two arguments

struct Class {
  u32 kind;  // JY_CMD_*
  u32 op;    // JY_TLOG_* / JY_TLOG_RD_*, 0 elsewhere
  u64 num;   // ts, amount bits, trim count or GET count (~0: all)
  int key;   // the key's word index
  int val;   // the value's word index, -1: the class has none
};

template <int N>
JY_RIN_HD bool word_is(const Word& w, const char (&name)[N]) {
  if (w.len != (u64)(N - 1)) return false;
  for (int i = 0; i < N - 1; i++)
    if (w.p[i] != (uint8_t)name[i]) return false;
  return true;
}

// UJSON GET's path (JY_RESP_UJSON_GET): one word is one segment, and a segment
// over kMaxKeyedLen is the render's JY_ERANGE.  The rule over ONE word, because
// a path has any number of them: classify_opts applies it to the words it
// reads, path_words_ok to the rest one after the other (the host), the decoder
// a lane per word (k_rin_pathchk).
JY_RIN_HD bool path_word_ok(u64 len) { return len <= kMaxKeyedLen; }
constexpr u32 kPathWord0 = 3;  // UJSON GET key segment...: the path starts at word 3

// UJSON INS / RM's value (JY_RESP_UJSON_WRITE).  A stored leaf holds the
// CANONICAL text of its JSON primitive (ujson_doc.canonical_value); the device
// does not canonicalise, it copies.  So a value word is taken only if it already
// is its canonical text, and exactly one of
//   true, false, null
//   an integer  -?(0|[1-9][0-9]{0,17})  other than -0: at most 18 digits
//   a string    "  then bytes 0x20 .. 0x7E other than " and \  then  "
// of at most kUjValueMax bytes.  Everything else -- floats, exponents, blanks,
// escapes, non-ASCII, 19 digits, longer values -- leaves the command with the
// host, which canonicalises or rejects it.  The rule over ONE word; its only
// loop is over that word's at most kUjValueMax bytes.
constexpr u64 kUjValueMax = 255;
JY_RIN_HD bool ujson_value_plain(const uint8_t* p, u64 len) {
  if (len == 0 || len > kUjValueMax) return false;
  const Word w{p, len};
  const uint8_t c0 = p[0];
  if (c0 == '"') {
    if (len < 2 || p[len - 1] != '"') return false;
    for (u64 i = 1; i + 1 < len; i++) {
      const uint8_t c = p[i];
      if (c < 0x20 || c > 0x7E || c == '"' || c == '\\') return false;
    }
    return true;
  }
  if (c0 == 't' || c0 == 'f' || c0 == 'n') return word_is(w, "true") || word_is(w, "false") || word_is(w, "null");
  const u64 d0 = c0 == '-' ? 1 : 0, nd = len - d0;
  if (nd == 0 || nd > 18) return false;
  if (p[d0] == '0') return nd == 1 && d0 == 0;  // 0; never -0 or a leading zero
  for (u64 i = d0; i < len; i++)
    if (p[i] < '0' || p[i] > '9') return false;
  return true;
}

// w[0 .. min(nwords, kWordsRead)); flags = JY_RESP_*.  JY_CMD_UJSON_GET and
// JY_CMD_UJSON_WRITE here judge the words read only: the command is of that
// kind iff the words from kWordsRead on pass their rules too (classify_all).
// UJSON INS / RM key [segment...] value: words 3 .. nwords - 2 are segments, the
// LAST word is the value, wherever it lies; UJSON CLR key has exactly 3 words
// (a CLR with a path stays with the host, as SET does).
JY_RIN_HD Class classify_opts(u64 nwords, const Word* w, u32 flags) {
  Class host{JY_CMD_HOST, 0, 0, -1, -1};
  if (nwords < 3) return host;  // every keyed command has a type, an op and a key
  if (w[2].len > kMaxKeyedLen) return host;
  Class c{JY_CMD_HOST, 0, 0, 2, -1};
  if ((flags & (JY_RESP_UJSON_GET | JY_RESP_UJSON_WRITE)) && word_is(w[0], "UJSON")) {
    if ((flags & JY_RESP_UJSON_GET) && word_is(w[1], "GET")) {
      for (u32 j = kPathWord0; j < kWordsRead && j < nwords; j++)
        if (!path_word_ok(w[j].len)) return host;
      c.kind = JY_CMD_UJSON_GET;  // its value is built from the words kPathWord0 .. nwords - 1, not one word
      return c;
    }
    if (!(flags & JY_RESP_UJSON_WRITE)) return host;
    if (word_is(w[1], "CLR")) {
      if (nwords != 3) return host;
      c.kind = JY_CMD_UJSON_WRITE;
      c.op = JY_UJSON_CLR;
      return c;
    }
    const bool ins = word_is(w[1], "INS");
    if (!(ins || word_is(w[1], "RM")) || nwords < 4) return host;
    for (u32 j = kPathWord0; j < kWordsRead && j + 1 < nwords; j++)
      if (!path_word_ok(w[j].len)) return host;
    if (nwords <= kWordsRead && !ujson_value_plain(w[nwords - 1].p, w[nwords - 1].len)) return host;
    c.kind = JY_CMD_UJSON_WRITE;  // its value is the leaf encoding, built from the words kPathWord0 .. nwords - 1
    c.op = ins ? JY_UJSON_INS : JY_UJSON_RM;
    return c;
  }
  const bool g = word_is(w[0], "GCOUNT"), pn = word_is(w[0], "PNCOUNT");
  if (g || pn) {
    if (word_is(w[1], "GET")) {
      c.kind = g ? JY_CMD_GCOUNT_GET : JY_CMD_PNCOUNT_GET;
      return c;
    }
    const bool inc = word_is(w[1], "INC"), dec = pn && word_is(w[1], "DEC");
    if (!(inc || dec) || nwords < 4) return host;
    if (g) {
      if (!parse_u64(w[3].p, w[3].len, &c.num)) return host;
      c.kind = JY_CMD_GCOUNT_INC;
    } else {
      int64_t x;
      if (!parse_i64(w[3].p, w[3].len, &x)) return host;
      c.num = (u64)x;
      c.kind = inc ? JY_CMD_PNCOUNT_INC : JY_CMD_PNCOUNT_DEC;
    }
    return c;
  }
  if (word_is(w[0], "TREG")) {
    if (word_is(w[1], "GET")) {
      c.kind = JY_CMD_TREG_GET;
      return c;
    }
    if (!word_is(w[1], "SET") || nwords < 5) return host;
    if (w[3].len > kMaxKeyedLen || !parse_u64(w[4].p, w[4].len, &c.num)) return host;
    c.kind = JY_CMD_TREG_SET;
    c.val = 3;
    return c;
  }
  if (word_is(w[0], "TLOG")) {
    if (word_is(w[1], "GET")) {
      c.kind = JY_CMD_TLOG_READ;
      c.op = JY_TLOG_RD_GET;
      c.num = ~0ull;
      if (nwords >= 4 && !parse_u64(w[3].p, w[3].len, &c.num)) c.num = ~0ull;
      return c;
    }
    if (word_is(w[1], "SIZE") || word_is(w[1], "CUTOFF")) {
      c.kind = JY_CMD_TLOG_READ;
      c.op = word_is(w[1], "SIZE") ? JY_TLOG_RD_SIZE : JY_TLOG_RD_CUTOFF;
      return c;
    }
    if (word_is(w[1], "INS")) {
      if (nwords < 5 || w[3].len > kMaxKeyedLen || !parse_u64(w[4].p, w[4].len, &c.num)) return host;
      c.kind = JY_CMD_TLOG_WRITE;
      c.op = JY_TLOG_INS;
      c.val = 3;
      return c;
    }
    if (word_is(w[1], "TRIMAT") || word_is(w[1], "TRIM")) {
      if (nwords < 4 || !parse_u64(w[3].p, w[3].len, &c.num)) return host;
      c.kind = JY_CMD_TLOG_WRITE;
      c.op = word_is(w[1], "TRIM") ? JY_TLOG_TRIM : JY_TLOG_TRIMAT;
      return c;
    }
    if (word_is(w[1], "CLR")) {
      c.kind = JY_CMD_TLOG_WRITE;
      c.op = JY_TLOG_CLR;
      return c;
    }
  }
  return host;
}

JY_RIN_HD Class classify(u64 nwords, const Word* w) { return classify_opts(nwords, w, 0); }

// the whole rule, sequentially: w[0 .. min(nwords, kWordsRead)) as above and
// lens[0 .. nwords) the length of every word; `last` = the command's last word
// with its bytes, looked at only for a JY_CMD_UJSON_WRITE of more than
// kWordsRead words (its value lies beyond the words read).  A leaf encoding --
// per segment 4 + its bytes, the terminator's 4, the value -- over kMaxKeyedLen,
// the leaf store's limit, leaves the command with the host.
JY_RIN_HD Class classify_all(u64 nwords, const Word* w, const u64* lens, u32 flags, const Word* last = nullptr) {
  const Class host{JY_CMD_HOST, 0, 0, -1, -1};
  Class c = classify_opts(nwords, w, flags);
  if (c.kind == JY_CMD_UJSON_GET)
    for (u64 j = kWordsRead; j < nwords; j++)
      if (!path_word_ok(lens[j])) return host;
  if (c.kind == JY_CMD_UJSON_WRITE && c.op != JY_UJSON_CLR) {
    for (u64 j = kWordsRead; j + 1 < nwords; j++)
      if (!path_word_ok(lens[j])) return host;
    if (nwords > kWordsRead && (!last || last->len != lens[nwords - 1] || !ujson_value_plain(last->p, last->len)))
      return host;
    u64 leaf = 0;  // (every term is at most 2^24 + 3: no overflow below 2^39 words)
    for (u64 j = kPathWord0; j < nwords; j++) leaf += 4 + lens[j];
    if (leaf > kMaxKeyedLen) return host;
  }
  return c;
}

}  // namespace jyrin
