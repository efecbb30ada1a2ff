// k_resp_in.hip -- RESP requests on the GPU: the bytes clients send, decoded into
// the column batches the keyed calls take (jy_resp_decode; include/jylis_gpu.h
// "RESP requests").  The rules -- tokens, numbers, classes -- are
// jy_resp_in.hpp's; this file is the parallel form of following them.
//
// A bulk string is binary-safe, so where a command starts is defined only by
// following lengths from the start of its connection's buffer: a chain.  One
// connection may pipeline tens of thousands of commands, so a lane per
// connection would put the whole batch behind that one chain.  Instead:
//   1 next     a lane per BYTE judges the token that would start there
//              (token_at, bounded by the connection's end) and writes its
//              successor next[i]: the token's end, or i itself when the token
//              is not complete or ends the connection -- a chain stops there.
//              Only a byte that is '*' or '$' parses anything.
//   2 reach    pointer doubling: reach[start of each connection] = 1, then a
//              fixed number of rounds of  reach[jump[i]] |= reach[i],
//              jump'[i] = jump[jump[i]]  (jump double-buffered; reach only
//              grows, so it is updated in place).  After round r the tokens
//              0 .. 2^r - 1 of every chain are marked; the host derives the
//              rounds from the longest connection (a complete token is at
//              least 4 bytes), so nothing is read back.
//   3 tokens   select compacts the reachable positions: the tokens, in
//              stream order.  A lane per token judges it again (type, value,
//              end) and finds its connection.
//   4 frames   an inclusive max-scan gives every token its latest header.  A
//              string more than n past its header, a header not exactly n + 1
//              past the one before, a string where a connection starts: each
//              is a violation; every token that is not complete closes its
//              connection too.  Each connection keeps its FIRST such token
//              (a min), and whether it is a violation or only the end of the
//              bytes so far.  A header with all its n strings before that
//              point is a command; select compacts the commands.
//   5 commands a lane per command reads at most kWordsRead words, classifies
//              and parses (classify).  Two scans give the phase: the kind
//              changes summed, minus the sum at the connection's first command
//              (a max-scan carries that command's index).  The commands of a
//              keyed kind are the rows: select, then jysort::sort_bits on
//              (phase << 8 | kind) above the command index -- stable, so rows
//              keep stream order inside a group.  Keys and values are gathered
//              by k_wire_gather with ReqSrc, whose item is a byte range of
//              req_bytes (jy_wire.hpp): no copy kernel of its own.
//   5' paths   only under JY_RESP_UJSON_GET (jy_resp_decode_opts; flags 0 runs
//              none of it): `UJSON GET key segment...` is a kind of its own
//              whose value column is the path, 4-byte length + bytes per
//              segment.  A path has any number of words, so every step is a
//              lane per path WORD (token), never a lane over a command's words:
//              k_rin_pathchk applies the segment rule to the words beyond
//              kWordsRead, k_rin_pathw + one scan over the tokens give every
//              word's place and (k_rin_pathlen, a difference of two scan
//              elements) every row's value length, which the existing value
//              scan places.  The value column is then gathered from PIECES
//              (k_rin_rowpieces, k_rin_vpiece_rows / _words) by k_wire_gather
//              with the generating source PathSrc: the length bytes generated,
//              the segment a pointer piece; other rows are one pointer piece.
//   5" leaves  only under JY_RESP_UJSON_WRITE: `UJSON INS / RM key segment...
//              value` and `UJSON CLR key` are a kind whose value column is the
//              LEAF encoding: the segments as above, the terminator FF FF FF FF
//              (a generated piece like a length) and the value word (a pointer
//              piece).  The same kernels, a lane per word; the one thing a word
//              cannot be judged by its length for is the value, the command's
//              LAST word: k_rin_ujval, a lane per command, reads it through the
//              token table and applies ujson_value_plain (at most 255 bytes).
// No lane, wave or workgroup loops over a connection's command or token count
// or over a key's or value's length; the loops are token_at's and parse_u64's
// 20 digits, the kWordsRead words of a command and the bisections.  Device
// input is never trusted: a length only ever enters a comparison with the bytes
// its connection has left, so every successor lies inside its connection and
// every later index derives from positions the select produced.
// All stores are ordinary vector stores; the two atomics are the min of step 4
// (taken only by a token that closes its connection) and a wave-reduced max.
//
// Roofline: latency- and launch-bound at a heartbeat's size; per request byte
// 1 B read + 9 B written by step 1 and 13 B moved by each doubling round, so a
// long pipelined connection pays rounds x bytes -- DESIGN.md, "RESP requests".

#include <algorithm>
#include <cstring>
#include <vector>

#include "jy_dscan.hpp"
#include "jy_resp_in.hpp"
#include "jy_sort.hpp"
#include "jy_wire.hpp"

namespace {

constexpr u64 kNoBad = ~0ull;
constexpr u32 kKindBits = 8;
constexpr u32 kPhaseBitsMax = 24;

// the connection byte x lies in: the largest c in [lo, hi) with offs[c] <= x
// (empty connections share their successor's offset and are never the answer)
__device__ __forceinline__ u64 conn_of(const u64* __restrict__ offs, u64 lo, u64 hi, u64 x) {
  return item_of([&](u64 j) { return offs[j]; }, lo, hi, x);
}

// ---- 1: successors ----
__global__ __launch_bounds__(kThreads) void k_rin_next(const uint8_t* __restrict__ req, const u64* __restrict__ offs,
                                                       u64 nconn, u64 total, u32* __restrict__ next,
                                                       uint8_t* __restrict__ reach) {
  __shared__ u64 ends[2];
  const u64 first = offs[0];
  const u64 i0 = (u64)blockIdx.x * kThreads, i1 = std::min<u64>(i0 + kThreads, total);
  if (threadIdx.x < 2) ends[threadIdx.x] = conn_of(offs, 0, nconn, std::max<u64>(threadIdx.x == 0 ? i0 : i1 - 1, first));
  __syncthreads();
  const u64 i = i0 + threadIdx.x;
  if (i >= i1) return;
  u32 nx = (u32)i;
  uint8_t r = 0;
  if (i >= first) {
    const u64 c = conn_of(offs, ends[0], ends[1] + 1, i);
    const u64 end = offs[c + 1];
    r = i == offs[c];
    const uint8_t b = req[i];
    if (b == '*' || b == '$') {
      const jyrin::Token t = jyrin::token_at(req + i, end - i);
      if (t.status == jyrin::kComplete && t.end < end - i) nx = (u32)(i + t.end);
    }
  }
  next[i] = nx;
  reach[i] = r;
}

// ---- 2: one doubling round ----
__global__ __launch_bounds__(kThreads) void k_rin_jump(const u32* __restrict__ jin, u32* __restrict__ jout, u64 total,
                                                       uint8_t* reach) {
  const u64 i = gid();
  if (i >= total) return;
  const u32 j = jin[i];  // <= total - 1: a successor lies inside its connection
  jout[i] = jin[j];
  if (j != (u32)i && reach[i]) reach[j] = 1;
}

struct PredReach {
  const uint8_t* reach;
  __device__ __forceinline__ bool operator()(u64 i) const { return reach[i] != 0; }
};

// ---- 3: tokens ----
// info = type | status << 2 (jy_resp_in.hpp's codes)
struct Toks {
  uint8_t* info;
  u64* val;   // <n> / <len>
  u32* end;   // where a complete token ends in req_bytes
  u32* body;  // where a complete string's bytes start
  u32* conn;
  u64* hdr;   // before the scan: t + 1 for a header token, else 0; after: the latest header at or before t, + 1
};
__device__ __forceinline__ u32 tok_type(uint8_t info) { return info & 3u; }

__global__ __launch_bounds__(kThreads) void k_rin_tok(const uint8_t* __restrict__ req, const u64* __restrict__ offs,
                                                      u64 nconn, const u32* __restrict__ pos, u64 T, Toks K,
                                                      unsigned long long* __restrict__ firstbad) {
  const u64 t = gid();
  if (t >= T) return;
  const u64 p = pos[t];
  const u64 c = conn_of(offs, 0, nconn, p);
  const jyrin::Token k = jyrin::token_at(req + p, offs[c + 1] - p);
  K.info[t] = (uint8_t)(k.type | (k.status << 2));
  K.val[t] = k.val;
  K.end[t] = (u32)(p + k.end);
  K.body[t] = (u32)(p + k.body);
  K.conn[t] = (u32)c;
  K.hdr[t] = k.type == jyrin::kHeader ? t + 1 : 0;
  if (k.status != jyrin::kComplete)
    atomicMin(firstbad + c, (unsigned long long)(t << 1 | (k.status == jyrin::kIncomplete ? 1u : 0u)));
}

// ---- 4: frames ----
// firstbad[c] = the connection's first closing token << 1 | (it only ends the bytes so far);
// lasttok[c] = its last token + 1 (0: it has none)
__global__ __launch_bounds__(kThreads) void k_rin_frames(Toks K, u64 T, unsigned long long* __restrict__ firstbad,
                                                         u64* __restrict__ lasttok) {
  const u64 t = gid();
  if (t >= T) return;
  const u32 c = K.conn[t];
  if (t + 1 == T || K.conn[t + 1] != c) lasttok[c] = t + 1;
  const u32 type = tok_type(K.info[t]);
  if (type == jyrin::kNoType) return;  // malformed: k_rin_tok closed the connection here
  bool bad;
  if (t == 0 || K.conn[t - 1] != c) {
    bad = type != jyrin::kHeader;  // a connection starts at a command boundary
  } else {
    const u64 h = K.hdr[t - 1];  // the latest header before t, + 1
    if (h == 0 || K.conn[h - 1] != c) return;  // the connection's first token was no header: closed there
    const u64 n = K.val[h - 1], past = t - (h - 1);  // t is the past-th token after its header
    bad = type == jyrin::kHeader ? past <= n : past > n;
  }
  if (bad) atomicMin(firstbad + c, (unsigned long long)(t << 1));
}

// a header with its n strings before its connection's closing point
struct PredCmd {
  const uint8_t* info;
  const u64* val;
  const u32* conn;
  const u64* firstbad;
  const u64* lasttok;
  __device__ __forceinline__ bool operator()(u64 t) const {
    if (info[t] != (uint8_t)(jyrin::kHeader | (jyrin::kComplete << 2))) return false;
    const u32 c = conn[t];
    const u64 fb = firstbad[c];
    const u64 lim = fb == kNoBad ? lasttok[c] : std::min<u64>(fb >> 1, lasttok[c]);
    return t < lim && val[t] < lim - t;
  }
};

__global__ __launch_bounds__(kThreads) void k_rin_conn_err(const u64* __restrict__ firstbad, u64 nconn,
                                                           uint8_t* __restrict__ err) {
  const u64 c = gid();
  if (c >= nconn) return;
  const u64 fb = firstbad[c];
  err[c] = fb != kNoBad && !(fb & 1);
}

// ---- 5: commands ----
struct Cmds {
  u32* conn;
  uint8_t* kind;
  u32* phase;
  u64* nwords;  // [ncmd + 1], the last 0: scanned into cmd_word_offs
  u64* num;
  uint8_t* op;
  u64 *koff, *klen, *voff, *vlen;  // the key's and the value's range of req_bytes
  u64* first;                      // k + 1 for a connection's first command, else 0; scanned (max)
  u64* chg;                        // 1 where the kind differs from the command before in the connection; scanned (sum)
};

__global__ __launch_bounds__(kThreads) void k_rin_cmd(const uint8_t* __restrict__ req, const u64* __restrict__ offs,
                                                      Toks K, const u32* __restrict__ cmdtok, u64 ncmd, Cmds C,
                                                      u32* __restrict__ tokcmd, u64* __restrict__ conn_used,
                                                      u32 flags) {
  const u64 k = gid();
  if (k > ncmd) return;
  if (k == ncmd) {
    C.nwords[k] = 0;
    return;
  }
  const u64 h = cmdtok[k];
  const u64 n = K.val[h];  // < T: PredCmd
  const u32 c = K.conn[h];
  jyrin::Word w[jyrin::kWordsRead];
  const u32 nw = (u32)std::min<u64>(n, jyrin::kWordsRead);
  for (u32 j = 0; j < jyrin::kWordsRead; j++) {
    const u64 t = h + 1 + (j < nw ? j : 0);
    w[j] = j < nw ? jyrin::Word{req + K.body[t], K.val[t]} : jyrin::Word{req, 0};
  }
  const jyrin::Class cl = jyrin::classify_opts(n, w, flags);
  C.conn[k] = c;
  C.kind[k] = (uint8_t)cl.kind;
  C.nwords[k] = n;
  C.num[k] = cl.num;
  C.op[k] = (uint8_t)cl.op;
  const bool keyed = cl.kind != JY_CMD_HOST;
  C.koff[k] = keyed ? K.body[h + 1 + cl.key] : 0;
  C.klen[k] = keyed ? K.val[h + 1 + cl.key] : 0;
  C.voff[k] = keyed && cl.val >= 0 ? K.body[h + 1 + cl.val] : 0;
  C.vlen[k] = keyed && cl.val >= 0 ? K.val[h + 1 + cl.val] : 0;
  C.first[k] = (k == 0 || K.conn[cmdtok[k - 1]] != c) ? k + 1 : 0;
  tokcmd[h] = (u32)k;
  // the connection's last command: its end is what the connection used
  if (k + 1 == ncmd || K.conn[cmdtok[k + 1]] != c) conn_used[c] = (u64)K.end[h + n] - offs[c];
}

__global__ __launch_bounds__(kThreads) void k_rin_chg(Cmds C, u64 ncmd) {
  const u64 k = gid();
  if (k >= ncmd) return;
  C.chg[k] = C.first[k] == 0 && C.kind[k] != C.kind[k - 1];
}

// phase = the kind changes up to k minus those up to its connection's first command; info[0] = the largest
__global__ __launch_bounds__(kThreads) void k_rin_phase(Cmds C, u64 ncmd, unsigned long long* __restrict__ info) {
  const u64 k = gid();
  u64 ph = 0;
  if (k < ncmd) {
    ph = C.chg[k] - C.chg[C.first[k] - 1];
    C.phase[k] = (u32)ph;
  }
  ph = jydscan::wave_reduce<jydscan::OpMax>(ph);
  if ((threadIdx.x & 63) == 0 && ph) atomicMax(info, (unsigned long long)ph);
}

// word j of command k is token cmdtok[k] + 1 + j: a lane per token
__global__ __launch_bounds__(kThreads) void k_rin_words(Toks K, u64 T, PredCmd is_cmd, const u32* __restrict__ tokcmd,
                                                        const u64* __restrict__ cwoff, u64* __restrict__ word_off,
                                                        u64* __restrict__ word_len) {
  const u64 t = gid();
  if (t >= T) return;
  if (K.info[t] != (uint8_t)(jyrin::kBulk | (jyrin::kComplete << 2))) return;
  const u64 h1 = K.hdr[t];
  if (h1 == 0 || !is_cmd(h1 - 1)) return;
  const u64 j = t - h1;  // t's ordinal among its header's strings
  if (j >= K.val[h1 - 1]) return;
  const u64 w = cwoff[tokcmd[h1 - 1]] + j;
  word_off[w] = K.body[t];
  word_len[w] = K.val[t];
}

// ---- UJSON GET's path (JY_RESP_UJSON_GET): a lane per path WORD ----
// A path has any number of words, so nothing here runs per command over its
// words: the segment rule, the bytes a word adds to its row's value and the two
// pieces it becomes are each a lane per token, and a command's share of a scan
// over the tokens is a difference of two of its elements.
struct PathWord {
  bool is;     // token t is word j >= kPathWord0 of a command (of any kind)
  u64 k, h, j;  // the command, its header token, the word's ordinal
};
__device__ __forceinline__ PathWord path_word(const Toks& K, const PredCmd& is_cmd, const u32* __restrict__ tokcmd,
                                              u64 t) {
  PathWord w{false, 0, 0, 0};
  if (K.info[t] != (uint8_t)(jyrin::kBulk | (jyrin::kComplete << 2))) return w;
  const u64 h1 = K.hdr[t];
  if (h1 == 0 || !is_cmd(h1 - 1)) return w;
  w.j = t - h1;
  if (w.j >= K.val[h1 - 1] || w.j < jyrin::kPathWord0) return w;
  w.is = true;
  w.h = h1 - 1;
  w.k = tokcmd[h1 - 1];
  return w;
}

// the segment rule beyond the words k_rin_cmd read: one word that breaks it
// sends its command to the host (every such lane stores the same byte)
__global__ __launch_bounds__(kThreads) void k_rin_pathchk(Toks K, u64 T, PredCmd is_cmd,
                                                          const u32* __restrict__ tokcmd, uint8_t* kind) {
  const u64 t = gid();
  if (t >= T) return;
  const PathWord w = path_word(K, is_cmd, tokcmd, t);
  if (!w.is || w.j < jyrin::kWordsRead || jyrin::path_word_ok(K.val[t])) return;
  const uint8_t kd = kind[w.k];
  // (a UJSON write's last word is its value, not a segment: k_rin_ujval's)
  if (kd == JY_CMD_UJSON_GET || (kd == JY_CMD_UJSON_WRITE && w.j + 1 < K.val[w.h])) kind[w.k] = JY_CMD_HOST;
}

// JY_RESP_UJSON_WRITE: the value of an INS / RM is the command's LAST word, which
// may lie beyond the words k_rin_cmd read.  One lane per command reads it through
// the token table and applies the value rule (its loop: kUjValueMax bytes).
__global__ __launch_bounds__(kThreads) void k_rin_ujval(const uint8_t* __restrict__ req, Toks K,
                                                        const u32* __restrict__ cmdtok, u64 ncmd, Cmds C) {
  const u64 k = gid();
  if (k >= ncmd || C.kind[k] != JY_CMD_UJSON_WRITE || C.op[k] == JY_UJSON_CLR) return;
  const u64 n = C.nwords[k];
  if (n <= jyrin::kWordsRead) return;  // classify_opts judged it
  const u64 t = (u64)cmdtok[k] + n;    // < T: PredCmd
  if (!jyrin::ujson_value_plain(req + K.body[t], K.val[t])) C.kind[k] = JY_CMD_HOST;
}

// pw[t] = the bytes token t adds to its row's value: 4 + len for a path word of a UJSON GET or write (lane T closes the scan's input)
__global__ __launch_bounds__(kThreads) void k_rin_pathw(Toks K, u64 T, PredCmd is_cmd, const u32* __restrict__ tokcmd,
                                                        const uint8_t* __restrict__ kind, u64* __restrict__ pw) {
  const u64 t = gid();
  if (t > T) return;
  u64 x = 0;
  if (t < T) {
    const PathWord w = path_word(K, is_cmd, tokcmd, t);
    // a UJSON write's words are its segments and, last, its value behind the terminator's four bytes
    if (w.is && (kind[w.k] == JY_CMD_UJSON_GET || kind[w.k] == JY_CMD_UJSON_WRITE)) x = 4 + K.val[t];
  }
  pw[t] = x;
}

// a UJSON GET's or write's value length: its words' share of the scan (tokens h + 1 .. h + n; h + n < T)
__global__ __launch_bounds__(kThreads) void k_rin_pathlen(const u32* __restrict__ cmdtok, u64 ncmd, Cmds C,
                                                          const u64* __restrict__ pws) {
  const u64 k = gid();
  if (k >= ncmd || (C.kind[k] != JY_CMD_UJSON_GET && C.kind[k] != JY_CMD_UJSON_WRITE)) return;
  const u64 h = cmdtok[k];
  const u64 len = pws[h + 1 + C.nwords[k]] - pws[h + 1];
  C.vlen[k] = len;
  // a leaf the store cannot hold is the host's to reject
  if (C.kind[k] == JY_CMD_UJSON_WRITE && len > jyrin::kMaxKeyedLen) C.kind[k] = JY_CMD_HOST;
}

// the kinds whose value is built from the words kPathWord0 .. nwords - 1
__device__ __forceinline__ bool uj_built(uint8_t kind) { return kind == JY_CMD_UJSON_GET || kind == JY_CMD_UJSON_WRITE; }

// The value column under the flag is gathered from PIECES: a row of another
// kind is one pointer piece (its value word), a UJSON GET row two pieces per
// segment -- the four length bytes, generated, and the segment, a pointer.
// npc[r] = row r's pieces (lane R: 0), rowof[command] = its row.
__global__ __launch_bounds__(kThreads) void k_rin_rowpieces(Cmds C, const u64* __restrict__ skey, u64 R,
                                                            u64* __restrict__ npc, u32* __restrict__ rowof) {
  const u64 r = gid();
  if (r > R) return;
  if (r == R) {
    npc[r] = 0;
    return;
  }
  const u32 k = (u32)skey[r];
  // (a UJSON write: two per segment and the terminator with the value word; a CLR has 3 words, so none)
  npc[r] = uj_built(C.kind[k]) ? 2 * (C.nwords[k] - jyrin::kPathWord0) : 1;
  rowof[k] = (u32)r;
}

constexpr u64 kPieceLen = 1ull << 63;  // pref: this bit | the length to write; else an offset into req_bytes
struct PathSrc {  // piece i of the value column (k_wire_gather's generating form)
  const uint8_t* req;
  const u64* pref;
  __device__ __forceinline__ u64 gen(u64 i, u64 from, u64 take) const {
    const u64 r = pref[i];
    if (!(r & kPieceLen)) return jy_ld8u(req + r + from, take);
    u64 v = (r & 0xFFFFFFFFull) >> (8 * from);  // little-endian: byte 0 is the lowest
    if (take < 8) v &= (1ull << (8 * take)) - 1;
    return v;
  }
};

// the one piece of every row that is no UJSON GET; lane R closes the piece offsets
__global__ __launch_bounds__(kThreads) void k_rin_vpiece_rows(Cmds C, const u32* __restrict__ wcmd,
                                                              const u64* __restrict__ wvoff, u64 R,
                                                              const u64* __restrict__ voffs,
                                                              const u64* __restrict__ pbase, u64* __restrict__ poff,
                                                              u64* __restrict__ pref) {
  const u64 r = gid();
  if (r > R) return;
  const u64 p = pbase[r];
  if (r == R) {
    poff[p] = voffs[R];
    return;
  }
  if (uj_built(C.kind[wcmd[r]])) return;
  poff[p] = voffs[r];
  pref[p] = wvoff[r];
}
// the two pieces of every path word: where they go is the row's value offset
// plus the word's place in the scan, both of which exist already
__global__ __launch_bounds__(kThreads) void k_rin_vpiece_words(Toks K, u64 T, PredCmd is_cmd,
                                                               const u32* __restrict__ tokcmd,
                                                               const uint8_t* __restrict__ kind,
                                                               const u32* __restrict__ rowof,
                                                               const u64* __restrict__ pws,
                                                               const u64* __restrict__ voffs,
                                                               const u64* __restrict__ pbase, u64 P,
                                                               u64* __restrict__ poff, u64* __restrict__ pref) {
  const u64 t = gid();
  if (t >= T) return;
  const PathWord w = path_word(K, is_cmd, tokcmd, t);
  if (!w.is || !uj_built(kind[w.k])) return;
  const u32 r = rowof[w.k];
  const u64 p = pbase[r] + 2 * (w.j - jyrin::kPathWord0);
  if (p + 1 >= P) return;  // never: pbase is the scan of these very counts
  const u64 o = voffs[r] + (pws[t] - pws[w.h + 1]);
  // the value word of a UJSON write follows the terminator FF FF FF FF, a generated piece like a length
  const bool value = kind[w.k] == JY_CMD_UJSON_WRITE && w.j + 1 == K.val[w.h];
  poff[p] = o;
  pref[p] = kPieceLen | (value ? 0xFFFFFFFFull : K.val[t]);
  poff[p + 1] = o + 4;
  pref[p + 1] = K.body[t];
}

struct PredRow {
  const uint8_t* kind;
  __device__ __forceinline__ bool operator()(u64 k) const { return kind[k] != JY_CMD_HOST; }
};

// sort keys: (phase << 8 | kind) << 32 | command
__global__ __launch_bounds__(kThreads) void k_rin_rowkey(Cmds C, const u32* __restrict__ rowsel, u64 R,
                                                         u64* __restrict__ key) {
  const u64 r = gid();
  if (r >= R) return;
  const u32 k = rowsel[r];
  key[r] = ((u64)C.phase[k] << kKindBits | C.kind[k]) << 32 | k;
}

struct Rows {
  u32* cmd;
  u64* num;
  uint8_t* op;
  u64 *klen, *vlen;  // [R + 1], the last 0
  u64 *koff, *voff;  // ranges of req_bytes (ReqSrc)
};
__global__ __launch_bounds__(kThreads) void k_rin_rows(Cmds C, const u64* __restrict__ skey, u64 R, Rows W) {
  const u64 r = gid();
  if (r > R) return;
  if (r == R) {
    W.klen[r] = W.vlen[r] = 0;
    return;
  }
  const u32 k = (u32)skey[r];
  W.cmd[r] = k;
  W.num[r] = C.num[k];
  W.op[r] = C.op[k];
  W.klen[r] = C.klen[k];
  W.vlen[r] = C.vlen[k];
  W.koff[r] = C.koff[k];
  W.voff[r] = C.voff[k];
}

struct PredGroup {  // a row whose (phase, kind) differs from the row before
  const u64* skey;
  __device__ __forceinline__ bool operator()(u64 r) const { return r == 0 || (skey[r] >> 32) != (skey[r - 1] >> 32); }
};
__global__ __launch_bounds__(kThreads) void k_rin_groups(const u64* __restrict__ skey, const u32* __restrict__ gstart,
                                                         u64 G, u64 R, u32* __restrict__ gphase,
                                                         uint8_t* __restrict__ gclass, u64* __restrict__ goffs) {
  const u64 g = gid();
  if (g > G) return;
  if (g == G) {
    goffs[g] = R;
    return;
  }
  const u32 r = gstart[g];
  gphase[g] = (u32)(skey[r] >> (32 + kKindBits));
  gclass[g] = (uint8_t)(skey[r] >> 32);
  goffs[g] = r;
}

// device word(s) -> the host, with one wait (u32 counts of select land in the low half of a cleared word)
int32_t read_counts(jy_engine* eng, std::initializer_list<std::pair<const void*, u64>> words, u64* out) {
  int q = 0;
  for (auto& w : words) {
    eng->pin_total[q] = 0;
    JY_HIP(eng, hipMemcpyAsync(eng->pin_total + q++, w.first, w.second, hipMemcpyDeviceToHost, eng->stream));
  }
  JY_HIP(eng, hipStreamSynchronize(eng->stream));
  for (int i = 0; i < q; i++) out[i] = eng->pin_total[i];
  return JY_OK;
}

// an empty decode: no command anywhere (conn_used / conn_err are the caller's to fill)
int32_t no_commands(jy_engine* eng, int32_t mem, u64* cmd_word_offs, u64* key_offs, u64* val_offs, u64* group_offs) {
  JY_TRY(empty_batch(eng, mem, {cmd_word_offs, key_offs, val_offs}));
  if (group_offs) *group_offs = 0;
  return host_sync(eng, mem);
}

// how far a decode's input went
enum : int { kRinNoBytes = 0, kRinNoCmd = 1, kRinFull = 2 };

}  // namespace

// The decoder's core, in two halves (jy_internal.hpp): what the decode knows
// after its four waits -- the sizes, and the device tables the outputs are
// written from -- and the writing of those outputs.  jy_resp_decode is the two
// with the capacity check between them; jy_resp_exec (k_resp_out.hip) sizes its
// own device arrays from the plan instead.
struct JyRinPlan {
  Tmp tmp;
  int stage = kRinNoBytes;
  u64 nconn = 0, total = 0, T = 0, ncmd = 0, W = 0, R = 0, G = 0, kbytes = 0, vbytes = 0;
  const uint8_t* req = nullptr;
  u64* d_used = nullptr;
  uint8_t* d_err = nullptr;
  Toks K{};
  Cmds C{};
  Rows X{};
  PredCmd is_cmd{};
  u64 *cwoff = nullptr, *skey = nullptr, *koffs = nullptr, *voffs_r = nullptr;
  u32 *tokcmd = nullptr, *gstart = nullptr;
  // JY_RESP_UJSON_GET: the scan of the path words' bytes over the tokens, the
  // rows' piece offsets (NP pieces in all) and each command's row
  u32 flags = 0;
  u64 NP = 0;
  u64 *pws = nullptr, *pbase = nullptr;
  u32* rowof = nullptr;
  explicit JyRinPlan(jy_engine* e) : tmp(e) {}
};

void jy_rin_free(JyRinPlan* p) { delete p; }

// steps 1 .. 5 up to the last wait: nconn > 0, conn_offs checked here.  sizes_out[6] as jy_resp_decode's.
int32_t jy_rin_plan(jy_engine* eng, uint64_t nconn, const uint8_t* req_bytes, int32_t req_mem,
                    const uint64_t* conn_offs, JyRinPlan** plan_out, uint64_t* sizes_out, uint32_t flags) {
  *plan_out = nullptr;
  if (flags & ~(uint32_t)(JY_RESP_UJSON_GET | JY_RESP_UJSON_WRITE))
    return eng->fail(JY_EINVAL, "an unknown JY_RESP_* flag");
  const bool uj = flags != 0;  // either flag builds value columns from pieces
  for (int q = 0; q < 6; q++) sizes_out[q] = 0;
  if (req_mem != JY_HOST && req_mem != JY_DEVICE) return eng->fail(JY_EINVAL, "req_mem must be JY_HOST or JY_DEVICE");
  if (nconn >= 0xFFFFFFFFull) return eng->fail(JY_ERANGE, "more than 2^32 - 1 connections in one call");
  if (nconn == 0 || !conn_offs) return eng->fail(JY_EINVAL, "conn_offs or caps is null");
  u64 longest = 0;
  for (u64 c = 0; c < nconn; c++) {
    if (conn_offs[c + 1] < conn_offs[c]) return eng->fail(JY_EINVAL, "conn_offs do not ascend");
    longest = std::max<u64>(longest, conn_offs[c + 1] - conn_offs[c]);
  }
  const u64 total = conn_offs[nconn];
  if (total > 0xFFFFFFFEull) return eng->fail(JY_ERANGE, "more than 2^32 - 2 request bytes in one call");
  if (total && !req_bytes) return eng->fail(JY_EINVAL, "req_bytes is null");

  JyRinPlan* P = new JyRinPlan(eng);
  struct Drop {
    JyRinPlan* p;
    ~Drop() { delete p; }
  } drop{P};
  const auto done = [&]() {
    drop.p = nullptr;
    *plan_out = P;
    return JY_OK;
  };
  Tmp& tmp = P->tmp;
  P->nconn = nconn;
  P->total = total;
  P->flags = flags;
  u64*& d_used = P->d_used;
  uint8_t*& d_err = P->d_err;
  JY_TRY(tmp.get(&d_used, nconn));
  JY_TRY(tmp.get(&d_err, nconn));
  JY_HIP(eng, hipMemsetAsync(d_used, 0, nconn * 8, eng->stream));
  JY_HIP(eng, hipMemsetAsync(d_err, 0, nconn, eng->stream));
  if (conn_offs[0] == total) return done();  // no byte at all
  const void *vreq, *voffs;
  JY_TRY(jy_stage_begin(eng));
  JY_TRY(jy_stage(eng, 0, req_bytes, total, req_mem, &vreq));
  JY_TRY(jy_stage(eng, 1, conn_offs, (nconn + 1) * 8, JY_HOST, &voffs));
  JY_TRY(jy_stage_end(eng));
  const uint8_t* req = P->req = static_cast<const uint8_t*>(vreq);
  const u64* offs = static_cast<const u64*>(voffs);

  // ---- 1, 2: successors and the reachable positions ----
  u32 *ja, *jb;
  uint8_t* reach;
  JY_TRY(tmp.get(&ja, total));
  JY_TRY(tmp.get(&jb, total));
  JY_TRY(tmp.get(&reach, total));
  LAUNCH(k_rin_next, total, req, offs, nconn, total, ja, reach);
  // a chain of a connection of `longest` bytes has at most longest / 4 + 1 tokens
  const u64 max_tokens = longest / 4 + 1;
  for (u64 marked = 1; marked < max_tokens; marked *= 2) {
    LAUNCH(k_rin_jump, total, (const u32*)ja, jb, total, reach);
    std::swap(ja, jb);
  }

  // ---- 3: tokens ----
  u32* tokpos = jb;  // the spare jump buffer: as many words as positions
  u64* cnt;
  JY_TRY(tmp.get(&cnt, 8));
  JY_HIP(eng, hipMemsetAsync(cnt, 0, 64, eng->stream));
  JY_TRY(jydscan::select(eng, total, PredReach{reach}, tokpos, reinterpret_cast<u32*>(cnt)));
  u64 T = 0;
  JY_TRY(read_counts(eng, {{cnt, 4}}, &T));  // the first wait
  if (T == 0 || T > total) return eng->fail(JY_EINVAL, "resp decode: the token count is inconsistent");
  P->T = T;
  Toks& K = P->K;
  JY_TRY(tmp.get(&K.info, T));
  JY_TRY(tmp.get(&K.val, T));
  JY_TRY(tmp.get(&K.end, T));
  JY_TRY(tmp.get(&K.body, T));
  JY_TRY(tmp.get(&K.conn, T));
  JY_TRY(tmp.get(&K.hdr, T));
  u64 *firstbad, *lasttok;
  JY_TRY(tmp.get(&firstbad, nconn));
  JY_TRY(tmp.get(&lasttok, nconn));
  JY_HIP(eng, hipMemsetAsync(firstbad, 0xFF, nconn * 8, eng->stream));
  JY_HIP(eng, hipMemsetAsync(lasttok, 0, nconn * 8, eng->stream));
  LAUNCH(k_rin_tok, T, req, offs, nconn, (const u32*)tokpos, T, K, reinterpret_cast<unsigned long long*>(firstbad));

  // ---- 4: frames ----
  JY_TRY((jydscan::scan<jydscan::OpMax, true>(eng, T, jydscan::LdArr<u64>{K.hdr}, jydscan::StArr<u64>{K.hdr})));
  LAUNCH(k_rin_frames, T, K, T, reinterpret_cast<unsigned long long*>(firstbad), lasttok);
  LAUNCH(k_rin_conn_err, nconn, (const u64*)firstbad, nconn, d_err);
  const PredCmd is_cmd = P->is_cmd = PredCmd{K.info, K.val, K.conn, firstbad, lasttok};
  u32*& tokcmd = P->tokcmd;
  u32* cmdtok;
  JY_TRY(tmp.get(&cmdtok, T));
  JY_TRY(tmp.get(&tokcmd, T));
  JY_TRY(jydscan::select(eng, T, is_cmd, cmdtok, reinterpret_cast<u32*>(cnt + 1)));
  u64 ncmd = 0;
  JY_TRY(read_counts(eng, {{cnt + 1, 4}}, &ncmd));  // the second wait
  if (ncmd > T) return eng->fail(JY_EINVAL, "resp decode: the command count is inconsistent");
  sizes_out[0] = P->ncmd = ncmd;
  P->stage = kRinNoCmd;
  if (ncmd == 0) return done();

  // ---- 5: commands ----
  Cmds& C = P->C;
  u64*& cwoff = P->cwoff;
  JY_TRY(tmp.get(&C.conn, ncmd));
  JY_TRY(tmp.get(&C.kind, ncmd));
  JY_TRY(tmp.get(&C.phase, ncmd));
  JY_TRY(tmp.get(&C.nwords, ncmd + 1));
  JY_TRY(tmp.get(&C.num, ncmd));
  JY_TRY(tmp.get(&C.op, ncmd));
  JY_TRY(tmp.get(&C.koff, ncmd));
  JY_TRY(tmp.get(&C.klen, ncmd));
  JY_TRY(tmp.get(&C.voff, ncmd));
  JY_TRY(tmp.get(&C.vlen, ncmd));
  JY_TRY(tmp.get(&C.first, ncmd));
  JY_TRY(tmp.get(&C.chg, ncmd));
  JY_TRY(tmp.get(&cwoff, ncmd + 1));
  LAUNCH(k_rin_cmd, ncmd + 1, req, offs, K, (const u32*)cmdtok, ncmd, C, tokcmd, d_used, flags);
  if (uj) {  // the words k_rin_cmd did not read, and the paths' lengths: before the kinds are compared
    u64* pw;
    JY_TRY(tmp.get(&pw, T + 1));
    JY_TRY(tmp.get(&P->pws, T + 1));
    LAUNCH(k_rin_pathchk, T, K, T, is_cmd, (const u32*)tokcmd, C.kind);
    if (flags & JY_RESP_UJSON_WRITE) LAUNCH(k_rin_ujval, ncmd, req, K, (const u32*)cmdtok, ncmd, C);
    LAUNCH(k_rin_pathw, T + 1, K, T, is_cmd, (const u32*)tokcmd, (const uint8_t*)C.kind, pw);
    JY_TRY(jy_scan_u64(eng, pw, P->pws, T));
    LAUNCH(k_rin_pathlen, ncmd, (const u32*)cmdtok, ncmd, C, (const u64*)P->pws);
  }
  JY_TRY(jy_scan_u64(eng, C.nwords, cwoff, ncmd));
  LAUNCH(k_rin_chg, ncmd, C, ncmd);
  JY_TRY((jydscan::scan<jydscan::OpSum, true>(eng, ncmd, jydscan::LdArr<u64>{C.chg}, jydscan::StArr<u64>{C.chg})));
  JY_TRY((jydscan::scan<jydscan::OpMax, true>(eng, ncmd, jydscan::LdArr<u64>{C.first}, jydscan::StArr<u64>{C.first})));
  LAUNCH(k_rin_phase, ncmd, C, ncmd, reinterpret_cast<unsigned long long*>(cnt + 2));
  u32* rowsel;
  JY_TRY(tmp.get(&rowsel, ncmd));
  JY_TRY(jydscan::select(eng, ncmd, PredRow{C.kind}, rowsel, reinterpret_cast<u32*>(cnt + 3)));
  u64 got[3];
  JY_TRY(read_counts(eng, {{cwoff + ncmd, 8}, {cnt + 2, 8}, {cnt + 3, 4}}, got));  // the third wait
  const u64 W = got[0], max_phase = got[1], R = got[2];
  if (W > T || R > ncmd || max_phase >= ncmd) return eng->fail(JY_EINVAL, "resp decode: the command table is inconsistent");
  const u32 pbits = jysort::bits_for(max_phase + 1);
  if (pbits > kPhaseBitsMax) return eng->fail(JY_ERANGE, "more than 2^24 phases in one call");
  sizes_out[1] = P->W = W;
  sizes_out[2] = P->R = R;

  // the rows in (phase, kind) order, their key and value offsets, the groups
  u64 *&skey = P->skey, *&koffs = P->koffs, *&voffs_r = P->voffs_r;
  Rows& X = P->X;
  u32*& gstart = P->gstart;
  u64 G = 0, kbytes = 0, vbytes = 0;
  if (R) {
    u64 *ka, *kb, *hist;
    JY_TRY(tmp.get(&ka, R));
    JY_TRY(tmp.get(&kb, R));
    JY_TRY(tmp.get(&hist, jysort::hist_words(R)));
    LAUNCH(k_rin_rowkey, R, C, (const u32*)rowsel, R, ka);
    JY_TRY(jysort::sort_bits(eng, ka, kb, hist, R, 32, 32 + kKindBits + pbits, &skey));
    JY_TRY(tmp.get(&X.cmd, R));
    JY_TRY(tmp.get(&X.num, R));
    JY_TRY(tmp.get(&X.op, R));
    JY_TRY(tmp.get(&X.klen, R + 1));
    JY_TRY(tmp.get(&X.vlen, R + 1));
    JY_TRY(tmp.get(&X.koff, R));
    JY_TRY(tmp.get(&X.voff, R));
    JY_TRY(tmp.get(&koffs, R + 1));
    JY_TRY(tmp.get(&voffs_r, R + 1));
    JY_TRY(tmp.get(&gstart, R));
    LAUNCH(k_rin_rows, R + 1, C, (const u64*)skey, R, X);
    JY_TRY(jy_scan_u64(eng, X.klen, koffs, R));
    JY_TRY(jy_scan_u64(eng, X.vlen, voffs_r, R));
    JY_TRY(jydscan::select(eng, R, PredGroup{skey}, gstart, reinterpret_cast<u32*>(cnt + 4)));
    u64* npc = nullptr;
    if (uj) {
      JY_TRY(tmp.get(&npc, R + 1));
      JY_TRY(tmp.get(&P->pbase, R + 1));
      JY_TRY(tmp.get(&P->rowof, ncmd));
      LAUNCH(k_rin_rowpieces, R + 1, C, (const u64*)skey, R, npc, P->rowof);
      JY_TRY(jy_scan_u64(eng, npc, P->pbase, R));
    }
    u64 g3[4] = {0, 0, 0, 0};
    if (uj)  // the fourth and last wait
      JY_TRY(read_counts(eng, {{cnt + 4, 4}, {koffs + R, 8}, {voffs_r + R, 8}, {P->pbase + R, 8}}, g3));
    else
      JY_TRY(read_counts(eng, {{cnt + 4, 4}, {koffs + R, 8}, {voffs_r + R, 8}}, g3));
    G = g3[0], kbytes = g3[1], vbytes = g3[2];
    P->NP = g3[3];
    if (G == 0 || G > R || kbytes > total || vbytes > total || P->NP > R + 2 * T)
      return eng->fail(JY_EINVAL, "resp decode: the row table is inconsistent");
  }
  sizes_out[3] = P->kbytes = kbytes;
  sizes_out[4] = P->vbytes = vbytes;
  sizes_out[5] = P->G = G;
  P->stage = kRinFull;
  return done();
}

// the plan's tables -> the arrays of `o`, in `mem` (the group table: host memory);
// every capacity is known to fit.  Ends as jy_resp_decode does.
int32_t jy_rin_emit(jy_engine* eng, JyRinPlan* P, const JyRinOut& o, int32_t mem) {
  Tmp& tmp = P->tmp;
  const u64 nconn = P->nconn, T = P->T, ncmd = P->ncmd, W = P->W, R = P->R, G = P->G, kbytes = P->kbytes,
            vbytes = P->vbytes;
  JY_TRY(emit(eng, mem, o.conn_used, P->d_used, nconn * 8));
  JY_TRY(emit(eng, mem, o.conn_err, P->d_err, nconn));
  if (P->stage != kRinFull) return no_commands(eng, mem, o.cmd_word_offs, o.key_offs, o.val_offs, o.group_offs);
  if (!o.cmd_conn || !o.cmd_kind || !o.cmd_phase || !o.cmd_word_offs || (W && (!o.word_off || !o.word_len)))
    return eng->fail(JY_EINVAL, "a command array is null");
  if (!o.key_offs || !o.val_offs || !o.group_offs ||
      (R && (!o.row_cmd || !o.num || !o.op || !o.group_phase || !o.group_class)) || (kbytes && !o.key_bytes) ||
      (vbytes && !o.val_bytes))
    return eng->fail(JY_EINVAL, "a row or group array is null");
  const Toks& K = P->K;
  const Cmds& C = P->C;
  const Rows& X = P->X;
  const uint8_t* req = P->req;
  u64 *cwoff = P->cwoff, *koffs = P->koffs, *voffs_r = P->voffs_r;

  // ---- outputs ----
  JY_TRY(emit(eng, mem, o.cmd_conn, C.conn, ncmd * 4));
  JY_TRY(emit(eng, mem, o.cmd_kind, C.kind, ncmd));
  JY_TRY(emit(eng, mem, o.cmd_phase, C.phase, ncmd * 4));
  JY_TRY(emit(eng, mem, o.cmd_word_offs, cwoff, (ncmd + 1) * 8));
  u64 *wo = nullptr, *wl = nullptr;
  if (W) {
    JY_TRY(tmp.out(&wo, o.word_off, W, mem));
    JY_TRY(tmp.out(&wl, o.word_len, W, mem));
    LAUNCH(k_rin_words, T, K, T, P->is_cmd, (const u32*)P->tokcmd, (const u64*)cwoff, wo, wl);
    JY_TRY(emit(eng, mem, o.word_off, wo, W * 8));
    JY_TRY(emit(eng, mem, o.word_len, wl, W * 8));
  }
  // a caller that answers the JY_CMD_HOST commands itself (jy_resp_exec) takes the command table on the host too
  if (o.h_cmd_kind) {
    JY_HIP(eng, hipMemcpyAsync(o.h_cmd_kind, C.kind, ncmd, hipMemcpyDeviceToHost, eng->stream));
    JY_HIP(eng, hipMemcpyAsync(o.h_cmd_phase, C.phase, ncmd * 4, hipMemcpyDeviceToHost, eng->stream));
    JY_HIP(eng, hipMemcpyAsync(o.h_cmd_word_offs, cwoff, (ncmd + 1) * 8, hipMemcpyDeviceToHost, eng->stream));
    if (W) {
      JY_HIP(eng, hipMemcpyAsync(o.h_word_off, wo, W * 8, hipMemcpyDeviceToHost, eng->stream));
      JY_HIP(eng, hipMemcpyAsync(o.h_word_len, wl, W * 8, hipMemcpyDeviceToHost, eng->stream));
    }
  }
  if (R == 0) {
    JY_TRY(empty_batch(eng, mem, {o.key_offs, o.val_offs}));
    *o.group_offs = 0;
    return host_sync(eng, o.h_cmd_kind ? JY_HOST : mem);
  }
  JY_TRY(emit(eng, mem, o.row_cmd, X.cmd, R * 4));
  JY_TRY(emit(eng, mem, o.num, X.num, R * 8));
  JY_TRY(emit(eng, mem, o.op, X.op, R));
  uint8_t *dkb, *dvb;
  JY_TRY(tmp.out(&dkb, o.key_bytes, kbytes, mem));
  JY_TRY(tmp.out(&dvb, o.val_bytes, vbytes, mem));
  JY_TRY(gather(eng, ReqSrc{req, X.koff}, koffs, R, kbytes, dkb));
  if (!P->flags) {
    JY_TRY(gather(eng, ReqSrc{req, X.voff}, voffs_r, R, vbytes, dvb));
  } else if (vbytes) {  // the same bytes from pieces: a value word, or a path's lengths and segments
    const u64 NP = P->NP;
    u64 *poff, *pref;
    JY_TRY(tmp.get(&poff, NP + 1));
    JY_TRY(tmp.get(&pref, NP + 1));
    LAUNCH(k_rin_vpiece_rows, R + 1, C, (const u32*)X.cmd, (const u64*)X.voff, R, (const u64*)voffs_r, (const u64*)P->pbase, poff, pref);
    LAUNCH(k_rin_vpiece_words, T, K, T, P->is_cmd, (const u32*)P->tokcmd, (const uint8_t*)C.kind,
           (const u32*)P->rowof, (const u64*)P->pws, (const u64*)voffs_r, (const u64*)P->pbase, NP, poff, pref);
    JY_TRY(gather(eng, PathSrc{req, pref}, poff, NP, vbytes, dvb));
  }
  JY_TRY(emit(eng, mem, o.key_bytes, dkb, kbytes));
  JY_TRY(emit(eng, mem, o.val_bytes, dvb, vbytes));
  JY_TRY(emit(eng, mem, o.key_offs, koffs, (R + 1) * 8));
  JY_TRY(emit(eng, mem, o.val_offs, voffs_r, (R + 1) * 8));
  // the group table is the host's plan of keyed calls: always host memory
  u32* gph;
  uint8_t* gcl;
  u64* gof;
  JY_TRY(tmp.get(&gph, G));
  JY_TRY(tmp.get(&gcl, G));
  JY_TRY(tmp.get(&gof, G + 1));
  LAUNCH(k_rin_groups, G + 1, (const u64*)P->skey, (const u32*)P->gstart, G, R, gph, gcl, gof);
  JY_HIP(eng, hipMemcpyAsync(o.group_phase, gph, G * 4, hipMemcpyDeviceToHost, eng->stream));
  JY_HIP(eng, hipMemcpyAsync(o.group_class, gcl, G, hipMemcpyDeviceToHost, eng->stream));
  JY_HIP(eng, hipMemcpyAsync(o.group_offs, gof, (G + 1) * 8, hipMemcpyDeviceToHost, eng->stream));
  JY_HIP(eng, hipStreamSynchronize(eng->stream));
  return JY_OK;
}

extern "C" int32_t jy_resp_decode_opts(jy_engine* eng, uint64_t nconn, const uint8_t* req_bytes, int32_t req_mem,
                                       const uint64_t* conn_offs, const uint64_t* caps, uint64_t* conn_used,
                                       uint8_t* conn_err, uint32_t* cmd_conn, uint8_t* cmd_kind, uint32_t* cmd_phase,
                                       uint64_t* cmd_word_offs, uint64_t* word_off, uint64_t* word_len,
                                       uint32_t* row_cmd, uint8_t* key_bytes, uint64_t* key_offs, uint8_t* val_bytes,
                                       uint64_t* val_offs, uint64_t* num, uint8_t* op, uint32_t* group_phase,
                                       uint8_t* group_class, uint64_t* group_offs, uint64_t* sizes_out, int32_t mem,
                                       uint32_t flags) {
  JY_HIP(eng, hipSetDevice(eng->device));
  for (int q = 0; q < 6; q++) sizes_out[q] = 0;
  JY_TRY(mem_check(eng, mem));
  if (req_mem != JY_HOST && req_mem != JY_DEVICE) return eng->fail(JY_EINVAL, "req_mem must be JY_HOST or JY_DEVICE");
  if (nconn >= 0xFFFFFFFFull) return eng->fail(JY_ERANGE, "more than 2^32 - 1 connections in one call");
  if (nconn == 0) return no_commands(eng, mem, cmd_word_offs, key_offs, val_offs, group_offs);
  if (!conn_offs || !caps) return eng->fail(JY_EINVAL, "conn_offs or caps is null");
  if (!conn_used || !conn_err) return eng->fail(JY_EINVAL, "conn_used or conn_err is null");
  JyRinPlan* P;
  JY_TRY(jy_rin_plan(eng, nconn, req_bytes, req_mem, conn_offs, &P, sizes_out, flags));
  struct Drop {
    JyRinPlan* p;
    ~Drop() { delete p; }
  } drop{P};
  for (int q = 0; q < 6; q++)
    if (caps[q] < sizes_out[q]) return JY_OK;  // sizes only
  return jy_rin_emit(eng, P, JyRinOut{conn_used, conn_err, cmd_conn, cmd_kind, cmd_phase, cmd_word_offs, word_off,
                                      word_len, row_cmd, key_bytes, key_offs, val_bytes, val_offs, num, op,
                                      group_phase, group_class, group_offs},
                     mem);
}

extern "C" int32_t jy_resp_decode(jy_engine* eng, uint64_t nconn, const uint8_t* req_bytes, int32_t req_mem,
                                  const uint64_t* conn_offs, const uint64_t* caps, uint64_t* conn_used,
                                  uint8_t* conn_err, uint32_t* cmd_conn, uint8_t* cmd_kind, uint32_t* cmd_phase,
                                  uint64_t* cmd_word_offs, uint64_t* word_off, uint64_t* word_len, uint32_t* row_cmd,
                                  uint8_t* key_bytes, uint64_t* key_offs, uint8_t* val_bytes, uint64_t* val_offs,
                                  uint64_t* num, uint8_t* op, uint32_t* group_phase, uint8_t* group_class,
                                  uint64_t* group_offs, uint64_t* sizes_out, int32_t mem) {
  return jy_resp_decode_opts(eng, nconn, req_bytes, req_mem, conn_offs, caps, conn_used, conn_err, cmd_conn, cmd_kind,
                             cmd_phase, cmd_word_offs, word_off, word_len, row_cmd, key_bytes, key_offs, val_bytes,
                             val_offs, num, op, group_phase, group_class, group_offs, sizes_out, mem, 0);
}
