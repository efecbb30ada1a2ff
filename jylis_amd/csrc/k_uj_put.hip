// k_uj_put.hip -- keyed UJSON writes: INS / RM / CLR by key string, in host or
// device memory (jy_ujson_write_keys; include/jylis_gpu.h "UJSON INS / RM / CLR
// by KEY STRING").
//
// Boundary: RepoUJSON.ins / rm / clr (repo_ujson.pony:85-110) with _data_for
// (INS creates on a miss) and the no-op of RM / CLR on a missing key
// (repo_ujson.pony:86,108).  One call takes a batch of commands as the RESP
// layer has them -- op, key string, the leaf in the leaf store's encoding --
// and applies it in command order; no slot and no handle crosses to the host.
//   checks   host arrays on the host; device arrays by k_put_check
//            (jy_put_check.hpp, shared with k_put.hip), whose verdict comes
//            back (with the counts below) before any kernel that loops over a
//            length is launched
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
//            ONE jy_ujson_write_batch.  Otherwise the applied commands go
//            through the device round split (jy_drounds.hpp, shared with
//            k_put.hip) with a unit of one command -- runs of INS are not
//            merged -- and each round is one jy_ujson_write_batch over its
//            slice of the columns k_ujp_pick gathers in round order.
// The loops: k_ujp_elem's over one RM leaf's bytes (an RM leaf is a client's
// path and value; the decoder bounds it by 2^24 - 1), the hash being sequential
// by definition (FNV-1a); everything else is a lane per command.
// All stores are ordinary vector stores; the atomics are the stamp and the
// wave-aggregated counts (and the split's own).
//
// Roofline: launch- and latency-bound at a heartbeat's size -- a call is three
// waits of its own plus the directory's and one per round (jy_ujson_write_batch
// sizes its delta from the state).  Times: DESIGN.md, "UJSON writes by key".
#include <algorithm>
#include <cstring>
#include <vector>

#include "jy_drounds.hpp"
#include "jy_leaf.hpp"
#include "jy_put_check.hpp"
#include "jy_wire.hpp"

namespace {

static_assert(kLeafMaxLen == kKeyLenMax, "a leaf is checked against the keys' limit (jy_put_check.hpp)");

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

// the columns of m commands in the order asked for: the commands live[0 .. m)
// as they are (ul null), or in the round order of a split of them (JyDRounds
// with units of one command: unit u is the command skey[u] names)
__global__ __launch_bounds__(kThreads) void k_ujp_pick(const u32* __restrict__ live, const u64* __restrict__ ul,
                                                       const u64* __restrict__ skey, u64 m, u64 n,
                                                       const uint8_t* __restrict__ op, const u32* __restrict__ slots,
                                                       const u64* __restrict__ elem, uint8_t* __restrict__ gop,
                                                       u32* __restrict__ gslot, u64* __restrict__ gelem) {
  const u64 j = gid();
  if (j >= m) return;
  const u32 u = ul ? (u32)ul[j] : 0;
  if (u >= m) return;  // never: the split's unit ids
  const u32 i = ul ? (u32)skey[u] : live[j];
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
  if (!checked) LAUNCH(k_put_check, n, n, ko, lo, op, (u32)JY_UJSON_CLR, reinterpret_cast<u32*>(res + 4));
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
    JyDRounds D;
    D.ro = {0, m};
    if (!repeats) {
      rounds = 1;
      LAUNCH(k_ujp_pick, m, (const u32*)live, (const u64*)nullptr, (const u64*)nullptr, m, n, op, (const u32*)slots,
             (const u64*)elem, gop, gslot, gelem);
    } else {
      // the live commands split into rounds (jy_drounds.hpp; a unit is one command): the third wait
      JY_TRY(jy_drounds<1>(eng, tmp, m, slots, live, nullptr, 0, jysort::bits_for(nk), &D));
      rounds = D.R;
      LAUNCH(k_ujp_pick, m, (const u32*)nullptr, D.ul, D.skey, m, n, op, (const u32*)slots, (const u64*)elem, gop,
             gslot, gelem);
    }
    const std::vector<u64>& ro = D.ro;
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
    u32 v = 0;  // every item's faults, as the kernel ORs them
    for (u64 i = 0; i < n; i++)
      v |= put_offs_bits(key_offs[i], key_offs[i + 1]) | put_offs_bits(leaf_offs[i], leaf_offs[i + 1]) |
           (op[i] > JY_UJSON_CLR ? 4u : 0u);
    JY_TRY(verdict_rc(eng, v));
    if ((key_offs[n] > key_offs[0] && !key_bytes) || (leaf_offs[n] > leaf_offs[0] && !leaf_bytes))
      return eng->fail(JY_EINVAL, "key_bytes or leaf_bytes is null");
  }
  uint32_t col = 0;
  JY_TRY(jy_replica_col(eng, identity, &col));
  if (mem == JY_DEVICE) return jy_ujson_write_keys_dev(eng, n, op, key_bytes, key_offs, leaf_bytes, leaf_offs, col, false);
  const void* dop;
  JY_TRY(jy_stage_begin(eng));
  JY_TRY(stage_ragged(eng, 0, 1, key_bytes, key_offs, n, &key_bytes, &key_offs));
  JY_TRY(jy_stage(eng, 3, op, n, JY_HOST, &dop));
  JY_TRY(stage_ragged(eng, 6, 7, leaf_bytes, leaf_offs, n, &leaf_bytes, &leaf_offs));
  JY_TRY(jy_stage_end(eng));
  return jy_ujson_write_keys_dev(eng, n, static_cast<const uint8_t*>(dop), key_bytes, key_offs, leaf_bytes, leaf_offs,
                                 col, true);
}

int32_t jy_ujson_write_keys_info(jy_engine* eng, uint64_t* out6) {
  for (int q = 0; q < 6; q++) out6[q] = eng->ujw_info[q];
  return JY_OK;
}

}  // extern "C"
