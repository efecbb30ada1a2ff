// k_uj_put.hip -- keyed UJSON writes: INS / RM / CLR by key string, in host or
// device memory (jy_ujson_write_keys; include/jylis_gpu.h "UJSON INS / RM / CLR
// by KEY STRING").
//
// Boundary: RepoUJSON.ins / rm / clr (repo_ujson.pony:85-110) with _data_for
// (INS creates on a miss) and the no-op of RM / CLR on a missing key
// (repo_ujson.pony:86,108).  One call takes a batch of commands as the RESP
// layer has them -- op, key string, the leaf in the leaf store's encoding --
// and applies it in command order; no slot and no handle crosses to the host.
//   checks   host arrays on the host; device arrays by k_ujp_check, whose
//            verdict comes back (with the counts below) before any kernel that
//            loops over a length is launched
//   keys     the INS commands are selected (jydscan::select), their keys
//            gathered into a column of their own (k_wire_gather, ReqSrc: a
//            256-byte key does not sit on one lane) and interned with create on
//            miss; then EVERY key is looked up.  A batch of INS alone interns
//            its key column as it is.
//   handles  the INS leaves go through the leaf store's put core with the
//            selection as its item list; k_ujp_elem hashes an RM leaf
//            (jy_leaf.hpp: a remove never grows the store) and gives CLR 0;
//            k_ujp_ins scatters the put's handles and counts the zeros
//   order    k_ujp_claim stamps each command's document with the call's number
//            (one atomicExch): a second command of a document sees the stamp,
//            so a batch without repeats is known as such without a sort and is
//            ONE jy_ujson_write_batch.  Otherwise the applied commands are
//            sorted by slot (jy_sort.hpp: slot << 32 | command, the slot bits
//            only), a command's round is its distance from its document's first
//            (a max-scan), a second sort by round lines the rounds up, and each
//            round is one jy_ujson_write_batch over its slice of the gathered
//            columns.  A unit is one command: runs of INS are not merged.
// The loops: k_ujp_elem's over one RM leaf's bytes (an RM leaf is a client's
// path and value; the decoder bounds it by 2^24 - 1), the hash being sequential
// by definition (FNV-1a); everything else is a lane per command.
// All stores are ordinary vector stores; the atomics are the stamp, the wave-
// aggregated counts and the per-round counts.
//
// Roofline: launch- and latency-bound at a heartbeat's size -- a call is three
// waits of its own plus the directory's and one per round (jy_ujson_write_batch
// sizes its delta from the state).  Times: DESIGN.md, "UJSON writes by key".
#include <algorithm>
#include <cstring>
#include <vector>

#include "jy_dscan.hpp"
#include "jy_leaf.hpp"
#include "jy_sort.hpp"
#include "jy_wire.hpp"

namespace {

constexpr u64 kKeyLenMax = JY_LR_LEN_MASK;
constexpr u64 kRoundsInline = 4096;  // round offsets that come back with the round count

// verdict bits: 1 = offsets not ascending, 2 = a length over its limit, 4 = an unknown op
__global__ __launch_bounds__(kThreads) void k_ujp_check(u64 n, const u64* __restrict__ ko, const u64* __restrict__ lo,
                                                        const uint8_t* __restrict__ op, u32* __restrict__ verdict) {
  const u64 i = gid();
  if (i >= n) return;
  u32 bad = 0;
  const u64 ka = ko[i], kb = ko[i + 1], la = lo[i], lb = lo[i + 1];
  if (kb < ka || lb < la) bad |= 1;
  if ((kb >= ka && kb - ka > kKeyLenMax) || (lb >= la && lb - la > kLeafMaxLen)) bad |= 2;
  if (op[i] > JY_UJSON_CLR) bad |= 4;
  if (bad) atomicOr(verdict, bad);
}

int32_t verdict_rc(jy_engine* eng, u32 v) {
  if (v & 5) return eng->fail(JY_EINVAL, v & 4 ? "unknown UJSON write op" : "offsets do not ascend");
  if (v & 2) return eng->fail(JY_ERANGE, "a key or a leaf is longer than 2^24 - 1 bytes");
  return JY_OK;
}

struct PredIns {
  const uint8_t* op;
  __device__ __forceinline__ bool operator()(u64 i) const { return op[i] == JY_UJSON_INS; }
};

// ikl[i] = the key bytes command i adds to the INS commands' key column (lane n: 0)
__global__ __launch_bounds__(kThreads) void k_ujp_inslen(const uint8_t* __restrict__ op, const u64* __restrict__ ko,
                                                         u64 n, u64* __restrict__ ikl) {
  const u64 i = gid();
  if (i > n) return;
  u64 v = 0;
  if (i < n && op[i] == JY_UJSON_INS) {
    const u64 a = ko[i], b = ko[i + 1];
    if (b >= a && b - a <= kKeyLenMax) v = b - a;  // (else the verdict fails the call)
  }
  ikl[i] = v;
}

// the q-th INS command (idx[q], *cnt of them): where its key starts in the
// batch's key bytes and in the compacted column; res = {INS commands, their
// key bytes, the leaf bytes' first and last offset}
__global__ __launch_bounds__(kThreads) void k_ujp_inskeys(const u32* __restrict__ idx, const u32* __restrict__ cnt,
                                                          const u64* __restrict__ ko, const u64* __restrict__ iks,
                                                          const u64* __restrict__ lo, u64 n, u64* __restrict__ isrc,
                                                          u64* __restrict__ iko, u64* __restrict__ res) {
  const u64 q = gid();
  if (q > n) return;
  const u64 c = std::min<u64>(*cnt, n);
  if (q < c) {
    const u32 i = idx[q];  // < n: the select's
    isrc[q] = ko[i];
    iko[q] = iks[i];
  }
  if (q == c) iko[c] = iks[n];
  if (q == 0) {
    res[0] = c;
    res[1] = iks[n];
    res[2] = lo[0];
    res[3] = lo[n];
  }
}

struct LdWords {  // aligned 8-byte loads, never past the words that hold the bytes asked for
  const uint8_t* p;
  __device__ __forceinline__ u64 operator()(u64 i, u64 m) const { return jy_ld8u(p + i, m); }
};

// elem[i] of a command that puts nothing: an RM's leaf hashed (0 for a leaf no
// put would take: it matches no element), 0 for CLR; INS: k_ujp_ins
__global__ __launch_bounds__(kThreads) void k_ujp_elem(const uint8_t* __restrict__ op, const uint8_t* __restrict__ lb,
                                                       const u64* __restrict__ lo, u64 n, u64* __restrict__ elem) {
  const u64 i = gid();
  if (i >= n) return;
  u64 h = 0, len;
  if (op[i] == JY_UJSON_RM && jy_leaf_len(lo[i], lo[i + 1], &len)) h = jy_leaf_hash_ld(LdWords{lb + lo[i]}, len);
  elem[i] = h;
}

// the put's handles to their commands; info[0] += the INS whose put gave handle 0
__global__ __launch_bounds__(kThreads) void k_ujp_ins(const u32* __restrict__ idx, const u64* __restrict__ dh, u64 nins,
                                                      u64 n, u64* __restrict__ elem, u64* __restrict__ info) {
  const u64 q = gid();
  bool bad = false;
  if (q < nins) {
    const u64 h = dh[q];
    const u32 i = idx[q];
    if (i < n) elem[i] = h;
    bad = h == 0;
  }
  jy_wave_count(bad, reinterpret_cast<unsigned long long*>(info));
}

// every command stamps its document: info[1] += the commands without one (a
// missing key), info[2] = 1 once a document is named twice
__global__ __launch_bounds__(kThreads) void k_ujp_claim(const u32* __restrict__ slots, u64 n, u64 nkeys, u32 epoch,
                                                        u32* __restrict__ claim, u64* __restrict__ info) {
  const u64 i = gid();
  bool miss = false;
  if (i < n) {
    const u32 s = slots[i];
    miss = s >= nkeys;  // JY_NO_SLOT (nothing else: the directory's slots)
    if (!miss && atomicExch(claim + s, epoch) == epoch) info[2] = 1;
  }
  jy_wave_count(miss, reinterpret_cast<unsigned long long*>(info + 1));
}

struct PredLive {
  const u32* slots;
  u64 nkeys;
  __device__ __forceinline__ bool operator()(u64 i) const { return slots[i] < nkeys; }
};

__global__ __launch_bounds__(kThreads) void k_ujp_keys(const u32* __restrict__ slots, const u32* __restrict__ live,
                                                       u64 m, u64* __restrict__ key) {
  const u64 j = gid();
  if (j < m) key[j] = (u64)slots[live[j]] << 32 | live[j];
}

// over the commands sorted by slot: p + 1 where a document's run starts, else 0
__global__ __launch_bounds__(kThreads) void k_ujp_runs(const u64* __restrict__ skey, u64 m, u64* __restrict__ sst) {
  const u64 p = gid();
  if (p >= m) return;
  sst[p] = (p == 0 || (skey[p - 1] >> 32) != (skey[p] >> 32)) ? p + 1 : 0;
}

// a command's round = its place in its document's run (sst: the max-scan of
// the marks); the rounds' sizes counted, info[3] = the rounds
__global__ __launch_bounds__(kThreads) void k_ujp_rounds(const u64* __restrict__ skey, const u64* __restrict__ sst,
                                                         u64 m, u64* __restrict__ rkey, u64* __restrict__ rcnt,
                                                         u64* __restrict__ info) {
  const u64 p = gid();
  if (p >= m) return;
  const u64 round = p + 1 - sst[p];  // < m
  rkey[p] = round << 32 | (u32)skey[p];
  atomicAdd(reinterpret_cast<unsigned long long*>(rcnt + round), 1ull);
  atomicMax(reinterpret_cast<unsigned long long*>(info + 3), (unsigned long long)(round + 1));
}

// the columns of the commands `ord` names (u32 indices, or the low halves of sorted keys), in that order
__global__ __launch_bounds__(kThreads) void k_ujp_pick(const u32* __restrict__ ord32, const u64* __restrict__ ord64,
                                                       u64 m, u64 n, const uint8_t* __restrict__ op,
                                                       const u32* __restrict__ slots, const u64* __restrict__ elem,
                                                       uint8_t* __restrict__ gop, u32* __restrict__ gslot,
                                                       u64* __restrict__ gelem) {
  const u64 j = gid();
  if (j >= m) return;
  const u32 i = ord32 ? ord32[j] : (u32)ord64[j];
  if (i >= n) return;  // never: the select's and the sort's indices
  gop[j] = op[i];
  gslot[j] = slots[i];
  gelem[j] = elem[i];
}

int32_t claim_grow(jy_engine* eng, u64 nk) {
  DevArray& c = eng->ujw_claim;
  if (c.bytes < nk * 4) {  // grows rarely: the whole array (re)set to epoch 0 once
    const u64 nb = std::max<u64>(std::max<u64>(nk * 4, c.bytes * 2), 4096);
    jy_dev_free(eng, c.p);
    c.p = nullptr;
    c.bytes = 0;
    JY_TRY(jy_dev_alloc(eng, &c.p, nb, "ujson write claims"));
    c.bytes = nb;
    JY_HIP(eng, hipMemsetAsync(c.p, 0, nb, eng->stream));
  }
  if (++eng->ujw_epoch == 0) {  // wrapped: no old stamp may match a new call
    JY_HIP(eng, hipMemsetAsync(c.p, 0, c.bytes, eng->stream));
    eng->ujw_epoch = 1;
  }
  return JY_OK;
}

}  // namespace

int32_t jy_ujson_write_keys_dev(jy_engine* eng, u64 n, const uint8_t* op, const uint8_t* kb, const u64* ko,
                                const uint8_t* lb, const u64* lo, u32 col, bool checked) {
  if (n == 0) return JY_OK;
  if (n >= 0xFFFFFFFFull) return eng->fail(JY_ERANGE, "more than 2^32 - 1 commands in one call");
  if (col >= eng->ujson.R) return eng->fail(JY_ERANGE, "ujson write: replica column outside the version vector");
  Tmp tmp(eng);

  // ---- checks, and the INS commands with their keys: the first wait ----
  u64 *res, *info, *ikl, *iks, *isrc, *iko;
  u32* idx;
  JY_TRY(tmp.get(&res, 8));  // [0 .. 3] k_ujp_inskeys', [4] the verdict, [5] the select's count
  JY_TRY(tmp.get(&info, 4));
  JY_TRY(tmp.get(&ikl, n + 1));
  JY_TRY(tmp.get(&iks, n + 1));
  JY_TRY(tmp.get(&isrc, n + 1));
  JY_TRY(tmp.get(&iko, n + 1));
  JY_TRY(tmp.get(&idx, n));
  JY_HIP(eng, hipMemsetAsync(res, 0, 64, eng->stream));
  JY_HIP(eng, hipMemsetAsync(info, 0, 32, eng->stream));
  if (!checked) LAUNCH(k_ujp_check, n, n, ko, lo, op, reinterpret_cast<u32*>(res + 4));
  LAUNCH(k_ujp_inslen, n + 1, op, ko, n, ikl);
  JY_TRY(jy_scan_u64(eng, ikl, iks, n));
  JY_TRY(jydscan::select(eng, n, PredIns{op}, idx, reinterpret_cast<u32*>(res + 5)));
  LAUNCH(k_ujp_inskeys, n + 1, (const u32*)idx, reinterpret_cast<const u32*>(res + 5), ko, (const u64*)iks, lo, n, isrc,
         iko, res);
  u64 h[5];
  JY_HIP(eng, hipMemcpyAsync(h, res, sizeof h, hipMemcpyDeviceToHost, eng->stream));
  JY_HIP(eng, hipStreamSynchronize(eng->stream));
  JY_TRY(verdict_rc(eng, (u32)h[4]));
  const u64 nins = h[0], ikbytes = h[1], lfirst = h[2], lend = h[3];
  if (nins > n || lend < lfirst || ikbytes > nins * kKeyLenMax)
    return eng->fail(JY_EINVAL, "ujson write: the command table is inconsistent");

  // ---- keys: intern the INS commands', then look every key up ----
  u32* slots;
  JY_TRY(tmp.get(&slots, n + 2));
  if (nins == n) {
    JY_TRY(jy_keys_intern_dev(eng, JY_UJSON, n, kb, ko, slots, nullptr, nullptr));
  } else {
    if (nins) {
      uint8_t* ikb;
      u32* islots;
      JY_TRY(tmp.get(&ikb, ikbytes));
      JY_TRY(tmp.get(&islots, nins + 2));
      JY_TRY(gather(eng, ReqSrc{kb, isrc}, iko, nins, ikbytes, ikb));
      JY_TRY(jy_keys_intern_dev(eng, JY_UJSON, nins, ikb, iko, islots, nullptr, nullptr));
    }
    u64 created = 0;
    JY_TRY(jy_keydir_run(eng, JY_UJSON, n, kb, ko, slots, false, &created));
  }
  const u64 nk = eng->nkeys[JY_UJSON];

  // ---- handles: INS leaves put, RM leaves hashed ----
  u64* elem;
  JY_TRY(tmp.get(&elem, n));
  LAUNCH(k_ujp_elem, n, op, lb, lo, n, elem);
  if (nins) {
    u64* dh;
    JY_TRY(tmp.get(&dh, nins));
    JY_TRY(jy_leaves_put_core(eng, nins, lb, lo, idx, lend - lfirst, dh));
    LAUNCH(k_ujp_ins, nins, (const u32*)idx, (const u64*)dh, nins, n, elem, info);
  }

  // ---- which documents, and whether one is named twice: the second wait ----
  JY_TRY(claim_grow(eng, std::max<u64>(nk, 1)));
  LAUNCH(k_ujp_claim, n, (const u32*)slots, n, nk, eng->ujw_epoch, static_cast<u32*>(eng->ujw_claim.p), info);
  u64 g[3];
  JY_HIP(eng, hipMemcpyAsync(g, info, sizeof g, hipMemcpyDeviceToHost, eng->stream));
  JY_HIP(eng, hipStreamSynchronize(eng->stream));
  const u64 bad = g[0], miss = g[1];
  const bool repeats = g[2] != 0;
  if (bad)
    return eng->fail(JY_EINVAL, "ujson write: the leaf store refused " + std::to_string(bad) +
                                    " INS leaf(s) (malformed, or a 64-bit handle collision); no document changed");
  if (miss > n) return eng->fail(JY_EINVAL, "ujson write: the command table is inconsistent");
  const u64 m = n - miss;
  u64 rounds = 0;
  if (m == 0) {
    // every command an RM / CLR of a missing key
  } else if (miss == 0 && !repeats) {
    rounds = 1;
    JY_TRY(jy_ujson_write_batch(eng, n, op, slots, elem, col));
  } else {
    u32* live;
    u64* cnt;
    JY_TRY(tmp.get(&live, n));
    JY_TRY(tmp.get(&cnt, 1));
    JY_TRY(jydscan::select(eng, n, PredLive{slots, nk}, live, reinterpret_cast<u32*>(cnt)));
    uint8_t* gop;
    u32* gslot;
    u64* gelem;
    JY_TRY(tmp.get(&gop, m));
    JY_TRY(tmp.get(&gslot, m));
    JY_TRY(tmp.get(&gelem, m));
    std::vector<u64> ro{0, m};
    if (!repeats) {
      rounds = 1;
      LAUNCH(k_ujp_pick, m, (const u32*)live, (const u64*)nullptr, m, n, op, (const u32*)slots, (const u64*)elem, gop,
             gslot, gelem);
    } else {
      const u64 hw = jysort::hist_words(m);
      u64* w;
      JY_TRY(tmp.get(&w, 6 * (m + 2) + hw));
      u64 *ka = w, *kc = ka + m + 2, *sst = kc + m + 2, *rkey = sst + m + 2, *rcnt = rkey + m + 2, *roff = rcnt + m + 2,
          *hist = roff + m + 2;
      LAUNCH(k_ujp_keys, m, (const u32*)slots, (const u32*)live, m, ka);
      u64* skey;
      JY_TRY(jysort::sort_bits(eng, ka, kc, hist, m, 32, 32 + jysort::bits_for(nk), &skey));
      u64* spare = skey == ka ? kc : ka;
      LAUNCH(k_ujp_runs, m, (const u64*)skey, m, sst);
      JY_TRY((jydscan::scan<jydscan::OpMax, true>(eng, m, jydscan::LdArr<u64>{sst}, jydscan::StArr<u64>{sst})));
      JY_HIP(eng, hipMemsetAsync(rcnt, 0, (m + 2) * 8, eng->stream));
      LAUNCH(k_ujp_rounds, m, (const u64*)skey, (const u64*)sst, m, rkey, rcnt, info);
      JY_TRY(jy_scan_u64(eng, rcnt, roff, m));
      // the round count and the first rounds' offsets: the third wait
      const u64 nin = std::min<u64>(m, kRoundsInline) + 1;
      std::vector<u64> hro(nin + 1);
      JY_HIP(eng, hipMemcpyAsync(hro.data(), info + 3, 8, hipMemcpyDeviceToHost, eng->stream));
      JY_HIP(eng, hipMemcpyAsync(hro.data() + 1, roff, nin * 8, hipMemcpyDeviceToHost, eng->stream));
      JY_HIP(eng, hipStreamSynchronize(eng->stream));
      rounds = hro[0];
      if (rounds == 0 || rounds > m) return eng->fail(JY_EINVAL, "ujson write: the grouping is inconsistent");
      ro.assign(hro.begin() + 1, hro.end());
      if (rounds + 1 > nin) {
        ro.resize(rounds + 1);
        JY_HIP(eng, hipMemcpyAsync(ro.data() + nin, roff + nin, (rounds + 1 - nin) * 8, hipMemcpyDeviceToHost,
                                   eng->stream));
        JY_HIP(eng, hipStreamSynchronize(eng->stream));
      }
      if (ro[0] != 0 || ro[rounds] != m) return eng->fail(JY_EINVAL, "ujson write: the rounds do not cover the commands");
      // the commands in round order (stable: document order inside a round)
      u64* ul;
      JY_TRY(jysort::sort_bits(eng, rkey, spare, hist, m, 32, 32 + jysort::bits_for(rounds), &ul));
      LAUNCH(k_ujp_pick, m, (const u32*)nullptr, (const u64*)ul, m, n, op, (const u32*)slots, (const u64*)elem, gop,
             gslot, gelem);
    }
    for (u64 j = 0; j < rounds; j++) {
      const u64 a = ro[j], mj = ro[j + 1] - a;
      if (ro[j + 1] > m || mj == 0 || mj > m) return eng->fail(JY_EINVAL, "ujson write: a round is out of range");
      // every round is judged against the documents as the rounds before left them
      JY_TRY(jy_ujson_write_batch(eng, mj, gop + a, gslot + a, gelem + a, col));
    }
  }
  u64* I = eng->ujw_info;
  I[0]++;
  I[1] = rounds;
  I[2] += rounds;
  I[3] = m;
  I[4] = miss;
  I[5] = nins;
  return JY_OK;
}

extern "C" {

int32_t jy_ujson_write_keys(jy_engine* eng, uint64_t n, const uint8_t* op, const uint8_t* key_bytes,
                            const uint64_t* key_offs, const uint8_t* leaf_bytes, const uint64_t* leaf_offs,
                            uint64_t identity, int32_t mem) {
  JY_HIP(eng, hipSetDevice(eng->device));
  JY_TRY(mem_check(eng, mem));
  if (n == 0) return JY_OK;
  if (n >= 0xFFFFFFFFull) return eng->fail(JY_ERANGE, "more than 2^32 - 1 commands in one call");
  if (!op || !key_offs || !leaf_offs) return eng->fail(JY_EINVAL, "a write batch needs ops, keys and leaves");
  if (mem == JY_HOST) {
    u32 v = 0;
    for (u64 i = 0; i < n; i++) {
      const u64 ka = key_offs[i], kb = key_offs[i + 1], la = leaf_offs[i], lb = leaf_offs[i + 1];
      if (kb < ka || lb < la) v |= 1;
      else if (kb - ka > kKeyLenMax || lb - la > kLeafMaxLen) v |= 2;
      if (op[i] > JY_UJSON_CLR) v |= 4;
    }
    JY_TRY(verdict_rc(eng, v));
    if ((key_offs[n] > key_offs[0] && !key_bytes) || (leaf_offs[n] > leaf_offs[0] && !leaf_bytes))
      return eng->fail(JY_EINVAL, "key_bytes or leaf_bytes is null");
  }
  uint32_t col = 0;
  JY_TRY(jy_replica_col(eng, identity, &col));
  if (mem == JY_DEVICE) return jy_ujson_write_keys_dev(eng, n, op, key_bytes, key_offs, leaf_bytes, leaf_offs, col, false);
  // only offs[0] .. offs[n] travel; the device pointers count from the arrays' starts, as the offsets do
  const void *dop, *dkb, *dko, *dlb, *dlo;
  JY_TRY(jy_stage_begin(eng));
  JY_TRY(jy_stage(eng, 0, key_bytes + key_offs[0], key_offs[n] - key_offs[0], JY_HOST, &dkb));
  JY_TRY(jy_stage(eng, 1, key_offs, (n + 1) * 8, JY_HOST, &dko));
  JY_TRY(jy_stage(eng, 3, op, n, JY_HOST, &dop));
  JY_TRY(jy_stage(eng, 6, leaf_bytes + leaf_offs[0], leaf_offs[n] - leaf_offs[0], JY_HOST, &dlb));
  JY_TRY(jy_stage(eng, 7, leaf_offs, (n + 1) * 8, JY_HOST, &dlo));
  JY_TRY(jy_stage_end(eng));
  return jy_ujson_write_keys_dev(eng, n, static_cast<const uint8_t*>(dop),
                                 static_cast<const uint8_t*>(dkb) - key_offs[0], static_cast<const u64*>(dko),
                                 static_cast<const uint8_t*>(dlb) - leaf_offs[0], static_cast<const u64*>(dlo), col,
                                 true);
}

int32_t jy_ujson_write_keys_info(jy_engine* eng, uint64_t* out6) {
  for (int q = 0; q < 6; q++) out6[q] = eng->ujw_info[q];
  return JY_OK;
}

}  // extern "C"
