/* jylis_gpu.h -- C ABI of the MI355X CRDT delta-convergence engine.
 *
 * Drop-in point: RepoManagerCore.converge_deltas (jylis/repo_manager.pony:92-93)
 * loops `_repo.converge(k, d)` over one decoded MsgPushDeltas batch
 * (jylis/msg.pony:20-24).  A GPU-backed Repo* marshals that whole
 * Array[(String, Any box)] into structure-of-arrays once and makes ONE call
 * here per batch (see INTEGRATION.md for the Pony FFI declarations).
 *
 * Conventions
 *   - every entry returns int32 status: 0 ok, < 0 error (detail in
 *     jy_last_error).  Pony FFI has no exceptions; the reference swallows
 *     converge failures (`try ... end`, repo_gcount.pony:51), so malformed
 *     entries are skipped and counted, never fatal (jy_skipped()).
 *   - pointers are borrowed for the duration of the call only.  `mem` says
 *     where they live: JY_HOST (copied through pinned staging) or JY_DEVICE
 *     (HBM-resident; read asynchronously on the engine stream, keep them
 *     alive until jy_sync).
 *   - one engine = one GPU = one key shard.  An engine handle is not
 *     thread-safe: the caller serialises calls (one RepoManager actor per
 *     type, repo_manager.pony:18).  No thread-local HIP state is assumed.
 *   - keys are interned to dense per-type slots (u32); replica identities
 *     (u64 Address.hash64, jylis/address.pony:29-33) to dense columns (u16).
 *   - within ONE converge call every slot appears at most once (a batch
 *     comes from the sender's `_deltas` Map, repo_gcount.pony:14,19-23).
 *     Host-pointer calls enforce this by splitting into rounds; device
 *     batches must honour it (routed batches are converged per source).
 */
#ifndef JYLIS_GPU_H
#define JYLIS_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JY_OK 0
#define JY_EINVAL (-1)
#define JY_ENOMEM (-2)
#define JY_EHIP (-3)
#define JY_ERANGE (-4)
#define JY_ETYPE (-5)

#define JY_NO_SLOT 0xFFFFFFFFu

/* CRDT types: the RepoManager names of database.pony:18-22 */
enum { JY_GCOUNT = 0, JY_PNCOUNT = 1, JY_TREG = 2, JY_TLOG = 3, JY_UJSON = 4, JY_NTYPES = 5 };
enum { JY_HOST = 0, JY_DEVICE = 1 };

typedef struct jy_engine jy_engine;

/* jy_config.flags: test switches that force a kernel form the engine would
 * otherwise pick by state size (the parity tests reach every form) */
#define JY_CFG_TREG_WHOLE_LINES 1u /* k_treg_lww<true>: every handle line rewritten */
#define JY_CFG_TREG_DUP_TEST 2u    /* a fixed 64-record TREG duplicate list the host never folds
                                      ahead of time: a test overflows it and expects JY_ERANGE */

typedef struct jy_config {
  int32_t device;            /* HIP device ordinal                                   */
  uint32_t counter_columns;  /* initial replica-column capacity of GCOUNT/PNCOUNT    */
  uint32_t ujson_columns;    /* version-vector width of UJSON contexts (fixed)       */
  uint32_t flags;            /* JY_CFG_* switches; 0 in production                   */
  uint64_t key_capacity[JY_NTYPES];   /* initial slots per type (grows by doubling)  */
  uint64_t entry_capacity[JY_NTYPES]; /* initial TLOG entries / UJSON dots            */
  uint64_t arena_capacity[JY_NTYPES]; /* initial string arena bytes (TREG, TLOG)      */
} jy_config;

/* ---- engine lifecycle (replaces RepoXXX.create(identity), repo_manager.pony:6) ---- */
void jy_config_default(jy_config* cfg);
int32_t jy_engine_create(const jy_config* cfg, jy_engine** out);
void jy_engine_destroy(jy_engine* eng);
const char* jy_last_error(const jy_engine* eng);
uint64_t jy_skipped(const jy_engine* eng);      /* malformed entries skipped so far  */
int32_t jy_set_stream(jy_engine* eng, void* hip_stream); /* NULL: engine-owned stream */
void* jy_get_stream(jy_engine* eng);
int32_t jy_sync(jy_engine* eng);
/* measurement (not on the reference's surface; bench.py and rocprof
 * cross-checks): while enabled, every merge call brackets its device work
 * (first to last launch, host staging excluded) with HIP events on the
 * engine stream.  jy_timing_read waits for them, writes up to `cap`
 * per-call durations in ms, returns the count in *n_out and clears them. */
int32_t jy_timing_enable(jy_engine* eng, int32_t on);
int32_t jy_timing_read(jy_engine* eng, uint64_t cap, double* ms_out, uint64_t* n_out);

/* ---- replica dictionary: u64 identity <-> dense column ---- */
int32_t jy_replica_col(jy_engine* eng, uint64_t replica_id, uint32_t* col_out);
int32_t jy_replica_id(const jy_engine* eng, uint32_t col, uint64_t* id_out);
uint32_t jy_replica_count(const jy_engine* eng);

/* ---- key interning: `_data_for(key)` (repo_gcount.pony:36-41) creates on miss,
 *      `_data(key)?` (repo_gcount.pony:53-55) only looks up (JY_NO_SLOT) ---- */
int32_t jy_keys_intern(jy_engine* eng, int32_t type, uint64_t n, const uint8_t* key_bytes,
                       const uint64_t* key_offs, uint32_t* slots_out);
int32_t jy_keys_lookup(const jy_engine* eng, int32_t type, uint64_t n, const uint8_t* key_bytes,
                       const uint64_t* key_offs, uint32_t* slots_out);
/* The key directory lives in HBM (hash table + key bytes, k_keys.hip); the
 * host-pointer calls above consult a host cache first and send the misses to
 * it.  The _mem forms take key_bytes / key_offs / slots_out in HBM when
 * mem = JY_DEVICE (bulk interning with no host round trip per key).  Slots
 * are dense, per type, handed out in order of first occurrence. */
int32_t jy_keys_intern_mem(jy_engine* eng, int32_t type, uint64_t n, const uint8_t* key_bytes,
                           const uint64_t* key_offs, uint32_t* slots_out, int32_t mem);
int32_t jy_keys_lookup_mem(jy_engine* eng, int32_t type, uint64_t n, const uint8_t* key_bytes,
                           const uint64_t* key_offs, uint32_t* slots_out, int32_t mem);
uint64_t jy_keys_count(const jy_engine* eng, int32_t type);
/* the key strings of slots [slot0, slot0 + n) (host out): offs_out u64[n + 1];
 * bytes_out is written when cap_bytes >= offs_out[n] (else sizes only).
 * Keys interned on the device (jy_keys_intern_mem, jy_keys_intern_lens) get
 * their names back this way.  Blocks. */
int32_t jy_keys_export(jy_engine* eng, int32_t type, uint64_t slot0, uint64_t n, uint64_t* offs_out,
                       uint8_t* bytes_out, uint64_t cap_bytes);
/* The directory as it lies in HBM (host out), for audits: info_out u64[4] =
 * {table entries (a power of two; 0 before the first key), their log2, keys,
 * key bytes}; table_out u64[table entries], each tag32 << 32 | slot or ~0 for
 * an empty one (the position is the top bits of a key's 64-bit hash, the tag
 * its low 32 bits); kref_out u64[keys] = byte offset << 24 | length; khash_out
 * u64[keys]; kw_out u64[keys][2] = the key's bytes 0..7 and 8..15, little
 * endian, zero filled.  With cap_entries or cap_slots short, or an output
 * missing, info_out alone is written (sizes only).  Read-only, no launch.
 * Blocks. */
int32_t jy_keys_table_read(jy_engine* eng, int32_t type, uint64_t* info_out, uint64_t* table_out,
                           uint64_t cap_entries, uint64_t* kref_out, uint64_t* khash_out, uint64_t* kw_out,
                           uint64_t cap_slots);
int32_t jy_keys_reserve(jy_engine* eng, int32_t type, uint64_t key_capacity);
/* owner shard of a key when keys are hash-sharded over `nshards` engines */
uint32_t jy_key_owner(const uint8_t* key, uint64_t len, uint32_t nshards);

/* ---- string arena of TREG / TLOG values (value bytes beyond the 8-byte prefix) ----
 * A value is held as (prefix u64 = first 8 bytes big-endian, zero padded;
 * lr u64 = arena_offset << 24 | length).  Values of <= 8 bytes never touch
 * the arena.  jy_values_pack appends long values (each on an 8-byte
 * boundary) and fills pre/lr. */
int32_t jy_values_pack(jy_engine* eng, int32_t type, uint64_t n, const uint8_t* bytes,
                       const uint64_t* offs, uint64_t* pre_out, uint64_t* lr_out);
/* The same handles for the same bytes, computed on the device (k_put.hip):
 * bytes / offs[n + 1] live in `mem`, pre_out / lr_out in `out_mem` (JY_HOST or
 * JY_DEVICE each).  pre = the first 8 bytes big-endian, zero padded; lr = len
 * for a value of up to 8 bytes, else arena_offset << 24 | len; long values
 * start on 8-byte granules, in call order, from the rounded-up arena end.
 * With host input the host sizes the arena and the call only enqueues (a
 * JY_HOST out_mem blocks for its copy); with device input one check kernel
 * judges the offsets and the call waits once for its verdict and offs[n].
 * Offsets that do not ascend are JY_EINVAL, a value over 16 MiB JY_ERANGE;
 * either way nothing is packed. */
int32_t jy_values_pack_mem(jy_engine* eng, int32_t type, uint64_t n, const uint8_t* bytes,
                           const uint64_t* offs, int32_t mem, uint64_t* pre_out, uint64_t* lr_out,
                           int32_t out_mem);

/* arena bytes in use / reserved (host counters, no GPU work) */
int32_t jy_arena_usage(jy_engine* eng, int32_t type, uint64_t* len_out, uint64_t* cap_out);
/* Reclaim the arena (TREG, TLOG): copy the values every live register, log
 * entry and pending delta still references back to back into a fresh arena
 * and rewrite their handles; *live_out = the bytes kept.  Handles packed by
 * jy_values_pack but not yet merged become INVALID: call between converge /
 * write calls (the reference frees a replaced value, repo_treg.pony:51-52).
 * Blocks. */
int32_t jy_arena_collect(jy_engine* eng, int32_t type, uint64_t* live_out);

/* ---- GCOUNT: GCounter.converge (repo_gcount.pony:50-51) / value (:53-55) ----
 * COO form: n cells (slot, col, value): s[slot][col] = max(s, value). */
int32_t jy_gcount_converge(jy_engine* eng, uint64_t n, const uint32_t* slot, const uint16_t* col,
                           const uint64_t* val, int32_t mem);
/* Column-block form: ncols peer columns over the slot run [slot0, slot0+nslots);
 * vals is [ncols][nslots] (one flushed peer batch per column, in slot order). */
int32_t jy_gcount_converge_block(jy_engine* eng, uint32_t ncols, const uint16_t* cols_host,
                                 uint32_t slot0, uint32_t nslots, const uint64_t* vals, int32_t mem);
int32_t jy_gcount_get(jy_engine* eng, uint64_t n, const uint32_t* slots, uint64_t* out, int32_t mem);

/* ---- GCOUNT / PNCOUNT: one decoded peer batch WITH its key strings ----
 * RepoManagerCore.converge_deltas (repo_manager.pony:92-93) of a counter
 * batch including each key's _data_for (repo_gcount.pony:36-41,
 * repo_pncount.pony:38-43: create on miss) in ONE call: the nkeys key strings
 * (key_bytes / key_offs, as jy_keys_intern) are interned on the device and
 * the ncells cells merged with their device slots -- no slot crosses to the
 * host (jy_keys_intern + jy_gcount_converge move every slot down and up).
 * Cell i belongs to key cell_key[i] (NULL: cell i is key i, ncells == nkeys)
 * and, for PNCOUNT, to sign[i] (0 = P, 1 = N; NULL: all P); GCOUNT takes
 * sign NULL.  s[slot][col] = max(s, val).  mem applies to every array (with
 * JY_DEVICE the key bytes / offsets are in HBM too). */
int32_t jy_counter_converge_keys(jy_engine* eng, int32_t type, uint64_t nkeys, const uint8_t* key_bytes,
                                 const uint64_t* key_offs, uint64_t ncells, const uint32_t* cell_key,
                                 const uint8_t* sign, const uint16_t* col, const uint64_t* val, int32_t mem);

/* ---- PNCOUNT: two GCounters (repo_pncount.pony:52-57); GET = (sum P - sum N) as i64 ---- */
int32_t jy_pncount_converge(jy_engine* eng, uint64_t np, const uint32_t* pslot, const uint16_t* pcol,
                            const uint64_t* pval, uint64_t nn, const uint32_t* nslot,
                            const uint16_t* ncol, const uint64_t* nval, int32_t mem);
/* vals_p / vals_n are each [ncols][nslots] */
int32_t jy_pncount_converge_block(jy_engine* eng, uint32_t ncols, const uint16_t* cols_host,
                                  uint32_t slot0, uint32_t nslots, const uint64_t* vals_p,
                                  const uint64_t* vals_n, int32_t mem);
int32_t jy_pncount_get(jy_engine* eng, uint64_t n, const uint32_t* slots, int64_t* out, int32_t mem);

/* counter state dump for parity checks: out is [nsigns][ncols][nslots] over
 * columns [0, ncols) and slots [slot0, slot0+nslots) (host memory) */
int32_t jy_counter_export(jy_engine* eng, int32_t type, uint32_t ncols, uint32_t slot0,
                          uint32_t nslots, uint64_t* out);

/* ---- counter write path: the local writes that produce deltas ----
 * jy_counter_write: n writes of THIS replica, whose column is `col`
 * (= jy_replica_col(identity)): GCOUNT INC (sign 0, RepoGCOUNT.inc
 * repo_gcount.pony:57-60), PNCOUNT INC (sign 0) / DEC (sign 1)
 * (RepoPNCOUNT.inc/dec repo_pncount.pony:59-67; the i64 argument bit-cast to
 * u64).  s[slot][col] += v (wrapping); each key's pending delta records its
 * post-write total (GCounter.increment).  Keys may repeat within a batch. */
int32_t jy_counter_write(jy_engine* eng, int32_t type, int32_t sign, uint32_t col, uint64_t n,
                         const uint32_t* slot, const uint64_t* val, int32_t mem);

/* ---- keyed writes: a batch of commands by KEY STRING (k_put.hip) ----
 * The write calls of the three keyed value types with their _data_for (create
 * on miss) in ONE call each: the n key strings (key_bytes / key_offs[n + 1],
 * as jy_keys_intern) are interned on the device, the values (val_bytes /
 * val_offs[n + 1]) packed on the device (jy_values_pack_mem), and the batch
 * applied with the device slots and handles -- no slot and no value handle
 * crosses to the host.  `mem` (JY_HOST / JY_DEVICE) applies to every array of
 * the call.  The state and the pending deltas end up exactly as if the
 * commands had gone one at a time, in call order, through jy_keys_intern +
 * jy_values_pack + the slot form of the call; keys may repeat any number of
 * times, in either memory.
 * Host arrays are checked in full before anything is launched; device arrays
 * by one check kernel whose verdict is read back before any kernel that loops
 * over a key or value length runs.  Offsets that do not ascend, an unknown op
 * or a missing column are JY_EINVAL, a key or value over 16 MiB JY_ERANGE;
 * nothing is applied.
 *   jy_counter_write_keys  jy_counter_write by key
 *   jy_treg_set_keys       jy_treg_set by key, value bytes instead of handles
 *   jy_tlog_write_keys     jy_tlog_write by key: op[i] as there; ts / arg /
 *                          val_bytes / val_offs may be null in a host batch
 *                          that has no command reading them (a device batch
 *                          passes every column) */
int32_t jy_counter_write_keys(jy_engine* eng, int32_t type, int32_t sign, uint32_t col, uint64_t n,
                              const uint8_t* key_bytes, const uint64_t* key_offs, const uint64_t* val,
                              int32_t mem);
int32_t jy_treg_set_keys(jy_engine* eng, uint64_t n, const uint8_t* key_bytes, const uint64_t* key_offs,
                         const uint64_t* ts, const uint8_t* val_bytes, const uint64_t* val_offs,
                         int32_t mem);
int32_t jy_tlog_write_keys(jy_engine* eng, uint64_t n, const uint8_t* op, const uint8_t* key_bytes,
                           const uint64_t* key_offs, const uint64_t* ts, const uint64_t* arg,
                           const uint8_t* val_bytes, const uint64_t* val_offs, int32_t mem);
/* telemetry of the TLOG write path's grouping: [0] write calls that grouped
 * their commands by key (device batches, keyed batches), [1] the rounds the
 * last of them ran, [2] the rounds of all of them.  A batch with no repeated
 * key runs one round; n INS to one key run ceil(n / 64). */
int32_t jy_tlog_write_rounds(jy_engine* eng, uint64_t* out3);
/* deltas_size() (repo_gcount.pony:16): keys with a pending delta.  Blocks. */
int32_t jy_counter_deltas_size(jy_engine* eng, int32_t type, uint64_t* n_out);
/* flush_deltas() (repo_gcount.pony:18-23): every pending key, ascending slot:
 * slot_out[i]; vals_out[sign * cap + i] = the recorded total (0 where that
 * sign was not written); mask_out[i] bit s set iff sign s was written.  Clears
 * the pending set.  *n_out = the count; JY_ERANGE (nothing cleared, *n_out =
 * the count needed) if cap is smaller.  Blocks. */
int32_t jy_counter_flush(jy_engine* eng, int32_t type, uint64_t cap, uint32_t* slot_out,
                         uint64_t* vals_out, uint32_t* mask_out, uint64_t* n_out, int32_t mem);

/* ---- TREG: TRegString.converge (repo_treg.pony:51-52), LWW by (ts, value) ----
 * An entry of a device batch whose slot is JY_NO_SLOT is skipped (a key not
 * interned): not merged, never a duplicate, not counted in jy_skipped.  A host
 * batch's slots are checked before anything is merged: every one must be
 * interned, JY_NO_SLOT included (JY_ERANGE otherwise). */
int32_t jy_treg_converge(jy_engine* eng, uint64_t n, const uint32_t* slot, const uint64_t* ts,
                         const uint64_t* pre, const uint64_t* lr, int32_t mem);
/* The same join for a BLOCK batch: entry i is the delta of slot slot0 + i
 * (a full-state delta, or a shard's batch regrouped in slot order), so no
 * slot stream is read and no slot can repeat.  [slot0, slot0 + n) must be
 * interned (JY_ERANGE otherwise). */
int32_t jy_treg_converge_block(jy_engine* eng, uint32_t slot0, uint64_t n, const uint64_t* ts,
                               const uint64_t* pre, const uint64_t* lr, int32_t mem);
/* read (ts, pre, lr) for n slots (host out) and fetch arena bytes */
int32_t jy_treg_read(jy_engine* eng, uint64_t n, const uint32_t* slots, uint64_t* ts_out,
                     uint64_t* pre_out, uint64_t* lr_out);
int32_t jy_arena_read(jy_engine* eng, int32_t type, uint64_t offset, uint64_t len, uint8_t* dst);

/* ---- TREG write path: RepoTREG.set (repo_treg.pony:65-68) ----
 * n local SETs (slot, ts, value handle from jy_values_pack): a SET that wins
 * against the state (LWW as converge) changes it and is LWW-merged into the
 * key's pending delta; the key's delta exists even when the SET loses
 * (_delta_for is evaluated either way).  Batches may repeat keys (applied in
 * order), in host or device memory. */
int32_t jy_treg_set(jy_engine* eng, uint64_t n, const uint32_t* slot, const uint64_t* ts,
                    const uint64_t* pre, const uint64_t* lr, int32_t mem);
int32_t jy_treg_deltas_size(jy_engine* eng, uint64_t* n_out);  /* deltas_size(); blocks */
/* flush_deltas() (repo_treg.pony:18-22): every pending key, ascending slot,
 * with its delta register (ts, pre, lr; a losing-only key reads ("", 0)), then
 * clears them.  JY_ERANGE (nothing cleared, *n_out = needed) if cap is short. */
int32_t jy_treg_flush(jy_engine* eng, uint64_t cap, uint32_t* slot_out, uint64_t* ts_out,
                      uint64_t* pre_out, uint64_t* lr_out, uint64_t* n_out, int32_t mem);
/* the first-occurrence claim of the TREG merges, read-only and off every merge
 * path (tests and diagnostics; waits for the engine's stream, folds nothing,
 * changes nothing).  out holds 8 words: [0] records in the pending duplicate
 * list as the device counts them (not clamped to the capacity), [1] the
 * list's capacity in records, [2] the host's upper bound of [0], [3] words of
 * one claim bitmap (32 slots each) -- zeros where a buffer does not exist yet;
 * then this build's geometry: [4] entries per lane of a keyed or block
 * launch, [5] records per lane of a routed launch, [6] parallel fold rounds
 * before the one-wave tail, [7] entries per workgroup of a keyed or block
 * launch.  With the list empty before it, one keyed merge launch leaves
 * [0] = its entries that were not the first of their slot, exactly.  A null
 * engine writes the build's words alone. */
int32_t jy_treg_claim_info(jy_engine* eng, uint64_t* out8);

/* ---- TLOG: TLog[String].converge (repo_tlog.pony:66-67) ----
 * nkeys delta logs, CSR: entries of key i are [ent_offs[i], ent_offs[i+1]),
 * canonical (later ts first, then greater value; unique; ts >= cutoff[i]).
 * Non-canonical segments are skipped (counted in jy_skipped). */
int32_t jy_tlog_converge(jy_engine* eng, uint64_t nkeys, const uint32_t* slot, const uint64_t* cutoff,
                         const uint64_t* ent_offs, uint64_t nent, const uint64_t* ts,
                         const uint64_t* pre, const uint64_t* lr, int32_t mem);
/* ---- TLOG write path: RepoTLOG.ins / trimat / trim / clr (repo_tlog.pony:85-111) ----
 * n commands applied in order: op[i] is JY_TLOG_INS (value handle pre/lr from
 * jy_values_pack at ts[i]), JY_TLOG_TRIMAT (ts[i]), JY_TLOG_TRIM (arg[i] =
 * count) or JY_TLOG_CLR.  Each changes the state as TLog.write / raise_cutoff
 * / trim / clear do, and where it changed the state the same change goes into
 * the key's pending delta log; every command marks its key pending.  Batches
 * may repeat keys (applied in order), in host or device memory: a device
 * batch is grouped by key on the device and applied in rounds (k_put.hip),
 * one round when no key repeats.  Unused columns of a host batch may be
 * null. */
#define JY_TLOG_INS 0
#define JY_TLOG_TRIMAT 1
#define JY_TLOG_TRIM 2
#define JY_TLOG_CLR 3
int32_t jy_tlog_write(jy_engine* eng, uint64_t n, const uint8_t* op, const uint32_t* slot, const uint64_t* ts,
                      const uint64_t* arg, const uint64_t* pre, const uint64_t* lr, int32_t mem);
int32_t jy_tlog_deltas_size(jy_engine* eng, uint64_t* n_out);  /* deltas_size(); blocks */
/* flush_deltas() (repo_tlog.pony:21-25): every pending key, ascending slot,
 * with its delta log (cutoff, entries newest first as a CSR); then clears
 * them.  With cap_keys / cap_ent too small nothing is written or cleared and
 * *nkeys_out / *nent_out report the sizes needed (JY_OK). */
int32_t jy_tlog_flush(jy_engine* eng, uint64_t cap_keys, uint64_t cap_ent, uint32_t* slot_out,
                      uint64_t* cutoff_out, uint64_t* ent_offs_out, uint64_t* ts_out, uint64_t* pre_out,
                      uint64_t* lr_out, uint64_t* nkeys_out, uint64_t* nent_out, int32_t mem);
/* Threading: a TLOG converge only enqueues.  Where a merge's rebuilt logs do
 * not fit the entry pool, the device leaves those keys as they were and keeps
 * their deltas; they are re-merged after a pool compaction by the next call
 * that finds the merge finished, or by any call that reads TLOG state (reads,
 * write commands, flush, jy_arena_collect, jy_sync), which waits for it.  A
 * call that fails midway may have applied part of its batch; retrying it is
 * safe (the join is idempotent). */
/* telemetry of the state store (not on the reference's surface): [0] merges
 * issued, [1] merges whose rebuilt logs were spilled and re-merged, [2] pool
 * compactions, [3] pool capacity in entries */
int32_t jy_tlog_stats(jy_engine* eng, uint64_t* out4);
/* where the state store keeps n logs (host slots), read-only and off the
 * merge path (tests and diagnostics; waits for the merges in flight like every
 * TLOG read).  out holds 6 n + 2 words, one column of n per field: pool index
 * of the oldest live entry (base), free entries just below it (front), live
 * entries (len), entries reserved from base (cap), cutoff, newest timestamp;
 * then the pool capacity in entries and the pool's bump pointer. */
int32_t jy_tlog_layout(jy_engine* eng, uint64_t n, const uint32_t* slots, uint64_t* out);
/* two-phase read: sizes (n entries per slot + cutoffs), then entries */
int32_t jy_tlog_read_sizes(jy_engine* eng, uint64_t n, const uint32_t* slots, uint64_t* len_out,
                           uint64_t* cutoff_out);
int32_t jy_tlog_read(jy_engine* eng, uint64_t n, const uint32_t* slots, const uint64_t* out_offs,
                     uint64_t* ts_out, uint64_t* pre_out, uint64_t* lr_out);

/* ---- UJSON: UJSON.converge (repo_ujson.pony:65-66), dot-kernel join ----
 * dots are packed (col << 48 | seq), seq in [1, 2^48).  Per doc i:
 *   elements [el_offs[i], el_offs[i+1]) of (dots, elems), dots ascending;
 *   context  version vector [vv_offs[i], vv_offs[i+1]) of packed (col << 48 | n)
 *            meaning "every seq <= n of col seen", plus
 *            cloud [cloud_offs[i], cloud_offs[i+1]) of packed dots, ascending. */
int32_t jy_ujson_converge(jy_engine* eng, uint64_t ndocs, const uint32_t* slot, const uint64_t* el_offs,
                          uint64_t nel, const uint64_t* dots, const uint64_t* elems,
                          const uint64_t* vv_offs, uint64_t nvv, const uint64_t* vv,
                          const uint64_t* cloud_offs, uint64_t ncloud, const uint64_t* cloud,
                          int32_t mem);
/* two-phase read: per slot element / cloud counts, then contents; vv_out is
 * [n][ujson_columns] dense */
int32_t jy_ujson_read_sizes(jy_engine* eng, uint64_t n, const uint32_t* slots, uint64_t* nel_out,
                            uint64_t* ncloud_out);
int32_t jy_ujson_read(jy_engine* eng, uint64_t n, const uint32_t* slots, const uint64_t* el_offs,
                      uint64_t* dots_out, uint64_t* elems_out, uint64_t* vv_out,
                      const uint64_t* cloud_offs, uint64_t* cloud_out);

/* ---- UJSON write path: RepoUJSON.ins / rm / clr (repo_ujson.pony:74-110) ----
 * Elements are opaque handles of (path, value) leaves (the leaf store below).
 * Path-scoped CLR and SET are RM / INS of the handles at or under the path;
 * which handles those are is selected on the device, by jy_ujson_path_read
 * (below), and only they travel to the host.  n commands applied
 * in order: JY_UJSON_INS elem[i] under a fresh dot of replica column col
 * (seq = the doc's vv[col] + 1); JY_UJSON_RM removes every element equal to
 * elem[i] (observed remove); JY_UJSON_CLR removes every element of the doc.
 * Each command's delta is converged into the state and into the doc's pending
 * delta; every command marks its doc pending (issue RM / CLR only for docs
 * that exist: repo_ujson.pony:86,108 create nothing).  Host batches may repeat
 * docs (applied in order); a device batch holds one command per doc. */
#define JY_UJSON_INS 0
#define JY_UJSON_RM 1
#define JY_UJSON_CLR 2
int32_t jy_ujson_write(jy_engine* eng, uint64_t n, const uint8_t* op, const uint32_t* slot, const uint64_t* elem,
                       uint32_t col, int32_t mem);
int32_t jy_ujson_deltas_size(jy_engine* eng, uint64_t* n_out);  /* deltas_size(); blocks */
/* flush_deltas() (repo_ujson.pony:22-26): every pending doc, ascending slot,
 * with its delta document (elements CSR, dense vv [ndocs][ujson_columns],
 * cloud CSR), then clears them.  Caps too small: sizes only (JY_OK). */
int32_t jy_ujson_flush(jy_engine* eng, uint64_t cap_docs, uint64_t cap_el, uint64_t cap_cloud, uint32_t* slot_out,
                       uint64_t* el_offs_out, uint64_t* dots_out, uint64_t* elems_out, uint64_t* vv_out,
                       uint64_t* cloud_offs_out, uint64_t* cloud_out, uint64_t* ndocs_out, uint64_t* nel_out,
                       uint64_t* ncloud_out, int32_t mem);

/* ---- wire-form flush: flush_deltas() as a ready-to-converge batch ----
 * `fun ref flush_deltas(): Array[(String, Any box)]` (repo_manager.pony:9,
 * repo_gcount.pony:18-23 and every repo_*.pony) returns KEY STRINGS and
 * deltas; the jy_*_flush calls above return slots and arena handles and leave
 * naming and value reads to the caller.  These calls flush the same pending
 * set -- every pending key, ascending slot, the same content -- as exactly
 * the arrays the same type's jy_node_*_converge takes, in its argument order:
 * key_bytes / key_offs[n + 1], then
 *   counters: cell_offs[n + 1], sign, col, val  (a key's cells P before N)
 *   TREG:     ts[n], val_bytes, val_offs[n + 1] (a key whose SETs all lost:
 *             ts 0 and an empty value, as jy_treg_flush)
 *   TLOG:     cutoff[n], ent_offs[n + 1], ts[nent], val_bytes, val_offs[nent + 1]
 *             (entries newest first; a cutoff-only delta has an empty range)
 *   UJSON:    el_offs[n + 1], dots, elems, vv_offs[n + 1], vv (packed
 *             col << 48 | n, zero entries dropped, columns ascending),
 *             cloud_offs[n + 1], cloud
 * Key and value bytes are packed back to back; offsets start at 0.  The
 * strings come from the device key directory and the value arenas: keys
 * interned on the device (jy_keys_intern_mem, jy_keys_intern_lens, a node
 * converge) are named without any jy_keys_export, and no jy_arena_read is
 * needed.
 * Two-phase: every output array has a capacity argument, in elements (bytes
 * for the byte arrays; an offsets array needs one element more than its
 * capacity names).  sizes_out receives the sizes needed, in the order of the
 * capacity arguments.  If any capacity is too small NOTHING is written and
 * nothing is cleared (JY_OK, sizes only: pass zeros and null pointers to
 * size); if all fit the outputs are written and the pending set is cleared
 * (jy_*_deltas_size is 0, the slot-form flush returns nothing).  With
 * nothing pending the batch is empty: sizes_out is all 0 and every non-null
 * offsets array receives its single element, 0.
 * `mem` applies to every output array (sizes_out is host memory).  With
 * JY_DEVICE the call only enqueues on the engine stream, apart from the
 * small read-backs of the pending count and the totals: the outputs are
 * complete after jy_sync.  With JY_HOST it blocks.
 * Columns: UJSON dots and vv entries carry THIS engine's columns; counter
 * cells carry the caller's `col` (the writing replica's column, as passed to
 * jy_counter_write).  Mapping column -> replica id -> the receiver's column
 * stays with the caller (jy_replica_id), as it does on the converge side.
 * LEAVES: a UJSON wire batch (a flush, a state or a slot-list dump) may carry
 * leaf_bytes / leaf_offs[nel + 1], parallel to `elems`: item i is the encoded
 * leaf of elems[i], one item per element, NOT de-duplicated (like TLOG's
 * val_bytes / val_offs).  They are a function of `elems` alone, so no wire
 * call's signature changes: "with leaves" is the wire call followed by
 * jy_ujson_leaves_get on its elems (below), on the device end to end with
 * JY_DEVICE output. */
int32_t jy_counter_flush_wire(jy_engine* eng, int32_t type, uint32_t col, uint64_t cap_keys,
                              uint64_t cap_key_bytes, uint64_t cap_cells, uint8_t* key_bytes, uint64_t* key_offs,
                              uint64_t* cell_offs, uint8_t* sign, uint16_t* col_out, uint64_t* val,
                              uint64_t* sizes_out /* [3] */, int32_t mem);
int32_t jy_treg_flush_wire(jy_engine* eng, uint64_t cap_keys, uint64_t cap_key_bytes, uint64_t cap_val_bytes,
                           uint8_t* key_bytes, uint64_t* key_offs, uint64_t* ts, uint8_t* val_bytes,
                           uint64_t* val_offs, uint64_t* sizes_out /* [3] */, int32_t mem);
int32_t jy_tlog_flush_wire(jy_engine* eng, uint64_t cap_keys, uint64_t cap_key_bytes, uint64_t cap_ent,
                           uint64_t cap_val_bytes, uint8_t* key_bytes, uint64_t* key_offs, uint64_t* cutoff,
                           uint64_t* ent_offs, uint64_t* ts, uint8_t* val_bytes, uint64_t* val_offs,
                           uint64_t* sizes_out /* [4] */, int32_t mem);
int32_t jy_ujson_flush_wire(jy_engine* eng, uint64_t cap_docs, uint64_t cap_key_bytes, uint64_t cap_el,
                            uint64_t cap_vv, uint64_t cap_cloud, uint8_t* key_bytes, uint64_t* key_offs,
                            uint64_t* el_offs, uint64_t* dots, uint64_t* elems, uint64_t* vv_offs, uint64_t* vv,
                            uint64_t* cloud_offs, uint64_t* cloud, uint64_t* sizes_out /* [5] */, int32_t mem);

/* ---- state snapshot in wire form: any slot range as a converge batch ----
 * The wire-form flushes above turn PENDING DELTAS into a ready-to-converge
 * batch; these calls do the same for STATE.  The reference only ever sends
 * deltas to the peers connected at flush time (repo_manager.pony:86-90,
 * cluster.pony:205-213) and keeps nothing on disk (repo_manager.pony:100,107
 * "TODO: disk persistence?"): a batch of state is what brings a late peer up
 * to date, what a host writes out to persist a store, and what is re-fed
 * through jy_node_*_converge to reshard.
 * One record per slot: record i is the state of slot slot0 + i, for EVERY
 * slot of [slot0, slot0 + nslots), in slot order.  The range must lie inside
 * jy_keys_count(type); otherwise JY_ERANGE, nothing is written and sizes_out
 * is all 0.  Arrays indexed per key hold exactly nslots elements (nslots + 1
 * for offsets): the caller knows that size, so it has no capacity argument;
 * sizes_out[0] = nslots all the same, for symmetry with the flush.
 * A slot in bottom state still produces a record: its key string and an
 * empty payload -- a counter whose cells are all 0 has no cells, TREG is
 * (ts 0, ""), TLOG an empty entry range and its cutoff, UJSON empty ranges.
 * Converging the record interns the key on the receiver (_data_for), so a
 * snapshot converged in order re-creates the key directory in slot order.
 * The arrays and their order are those of the same type's
 * jy_node_*_converge and jy_*_flush_wire (the block above): strings packed
 * back to back, offsets starting at 0; TLOG entries newest first and
 * canonical; UJSON dots ascending per document, the version vector packed
 * col << 48 | n with zero entries dropped, the cloud ascending -- for a
 * document in the per-column in-place layout the same canonical order
 * jy_ujson_read gives.
 * Counters: a key's cells are its NON-ZERO state cells over every registered
 * column [0, jy_replica_count) (zero equals absent under max and sum), all P
 * cells before all N cells, columns ascending within a sign.  `col` is THIS
 * engine's column: mapping column -> replica id -> the receiver's column
 * stays with the caller (jy_replica_id), as for the flush.
 * Two-phase like the flush: sizes_out receives nslots and then the sizes
 * needed, in the order of the capacity arguments.  If any capacity is too
 * small NOTHING is written (JY_OK, sizes only: pass zeros and null pointers
 * to size a range); if all fit every output is written.  nslots == 0 is an
 * empty batch: sizes_out is all 0 and every non-null offsets array receives
 * its single element, 0.
 * Read-only: no state, pending set, arena or key directory changes;
 * jy_*_deltas_size is the same afterwards and a later jy_*_flush_wire
 * returns what it would have returned without the call.  The TLOG call
 * settles outstanding merges first (as every TLOG state read does).
 * `mem` applies to every output array (sizes_out is host memory).  With
 * JY_DEVICE the call only enqueues on the engine stream, apart from the
 * read-back of the totals: the outputs are complete after jy_sync.  With
 * JY_HOST it blocks.
 * Under a node these calls read state that converges change: they are made
 * under jy_node_lock_type(node, type), NOT under JY_NODE_NOFENCE. */
int32_t jy_counter_state_wire(jy_engine* eng, int32_t type, uint64_t slot0, uint64_t nslots,
                              uint64_t cap_key_bytes, uint64_t cap_cells, uint8_t* key_bytes, uint64_t* key_offs,
                              uint64_t* cell_offs, uint8_t* sign, uint16_t* col, uint64_t* val,
                              uint64_t* sizes_out /* [3] */, int32_t mem);
int32_t jy_treg_state_wire(jy_engine* eng, uint64_t slot0, uint64_t nslots, uint64_t cap_key_bytes,
                           uint64_t cap_val_bytes, uint8_t* key_bytes, uint64_t* key_offs, uint64_t* ts,
                           uint8_t* val_bytes, uint64_t* val_offs, uint64_t* sizes_out /* [3] */, int32_t mem);
int32_t jy_tlog_state_wire(jy_engine* eng, uint64_t slot0, uint64_t nslots, uint64_t cap_key_bytes,
                           uint64_t cap_ent, uint64_t cap_val_bytes, uint8_t* key_bytes, uint64_t* key_offs,
                           uint64_t* cutoff, uint64_t* ent_offs, uint64_t* ts, uint8_t* val_bytes,
                           uint64_t* val_offs, uint64_t* sizes_out /* [4] */, int32_t mem);
int32_t jy_ujson_state_wire(jy_engine* eng, uint64_t slot0, uint64_t nslots, uint64_t cap_key_bytes,
                            uint64_t cap_el, uint64_t cap_vv, uint64_t cap_cloud, uint8_t* key_bytes,
                            uint64_t* key_offs, uint64_t* el_offs, uint64_t* dots, uint64_t* elems,
                            uint64_t* vv_offs, uint64_t* vv, uint64_t* cloud_offs, uint64_t* cloud,
                            uint64_t* sizes_out /* [5] */, int32_t mem);
/* ---- Slot-list snapshots (jy_*_state_wire_slots) ----
 * The same batch for a LIST of slots: record i is the state of slots[i].
 * Arguments, outputs, the two-phase convention and the read-only contract are
 * those of the type's jy_*_state_wire, with (slot0, nslots) replaced by
 * (n, slots, slots_mem); slots_mem (JY_HOST / JY_DEVICE) says where the list
 * lives, independently of `mem`.  The list must be STRICTLY ASCENDING and
 * every slot below jy_keys_count(type); this is checked on the device before
 * anything is read through the list: a list that is not ascending (a repeated
 * slot included) returns JY_EINVAL, a slot out of range JY_ERANGE, and
 * neither writes anything but zeros to sizes_out.  The list call waits for
 * the stream once more than the range call (the check's error word).  The
 * lists come from jy_state_bucket_slots below.  Locking under a node: as
 * jy_*_state_wire (jy_node_lock_type, not JY_NODE_NOFENCE). */
int32_t jy_counter_state_wire_slots(jy_engine* eng, int32_t type, uint64_t n, const uint32_t* slots,
                                    int32_t slots_mem, uint64_t cap_key_bytes, uint64_t cap_cells,
                                    uint8_t* key_bytes, uint64_t* key_offs, uint64_t* cell_offs, uint8_t* sign,
                                    uint16_t* col, uint64_t* val, uint64_t* sizes_out /* [3] */, int32_t mem);
int32_t jy_treg_state_wire_slots(jy_engine* eng, uint64_t n, const uint32_t* slots, int32_t slots_mem,
                                 uint64_t cap_key_bytes, uint64_t cap_val_bytes, uint8_t* key_bytes,
                                 uint64_t* key_offs, uint64_t* ts, uint8_t* val_bytes, uint64_t* val_offs,
                                 uint64_t* sizes_out /* [3] */, int32_t mem);
int32_t jy_tlog_state_wire_slots(jy_engine* eng, uint64_t n, const uint32_t* slots, int32_t slots_mem,
                                 uint64_t cap_key_bytes, uint64_t cap_ent, uint64_t cap_val_bytes,
                                 uint8_t* key_bytes, uint64_t* key_offs, uint64_t* cutoff, uint64_t* ent_offs,
                                 uint64_t* ts, uint8_t* val_bytes, uint64_t* val_offs,
                                 uint64_t* sizes_out /* [4] */, int32_t mem);
int32_t jy_ujson_state_wire_slots(jy_engine* eng, uint64_t n, const uint32_t* slots, int32_t slots_mem,
                                  uint64_t cap_key_bytes, uint64_t cap_el, uint64_t cap_vv, uint64_t cap_cloud,
                                  uint8_t* key_bytes, uint64_t* key_offs, uint64_t* el_offs, uint64_t* dots,
                                  uint64_t* elems, uint64_t* vv_offs, uint64_t* vv, uint64_t* cloud_offs,
                                  uint64_t* cloud, uint64_t* sizes_out /* [5] */, int32_t mem);

/* ---- UJSON leaf store (jy_ujson_leaves_*): the leaves behind the handles ----
 * A UJSON element is an opaque u64 handle; the (path, value) leaf behind it
 * lives in a content-addressed store in HBM, one per engine: an
 * open-addressing table keyed by the handle and a byte arena (leaves on 8-byte
 * granules, referenced as offset << 24 | length like arena values).  A leaf is
 * stored in its canonical ENCODING: each path segment as a 4-byte
 * little-endian length plus its bytes, then FF FF FF FF, then the value text.
 * HANDLE FORMULA: handle = FNV-1a 64 over the encoding, a result of 0
 * replaced by 1 (0 is "no element").  Every replica derives the same handle
 * for the same leaf; the state digests hash handles and stay valid.
 * The store is APPEND-ONLY between collections: a put never removes a leaf;
 * jy_ujson_leaves_collect (below) drops the leaves no document refers to.
 * jy_ujson_leaves_put: n leaves packed back to back (leaf_bytes,
 * leaf_offs[n + 1]).  A lane per leaf hashes it on the device, stores it if
 * its handle is absent and writes the handle to handles_out[i].  A handle
 * already present has its stored bytes compared with the new ones: equal,
 * nothing is stored; different (a 64-bit collision), the first leaf stays,
 * handles_out[i] = 0 and the collision counter goes up (still JY_OK).  A leaf
 * repeated within one call is stored once and every copy gets the same
 * handle.  Malformed items -- offs[i + 1] < offs[i], a length below 4 (no
 * terminator) or above 2^24 - 1 -- are skipped, counted in jy_skipped and get
 * handle 0, never fatal.  JY_HOST offsets are checked on the host before
 * anything is launched: an array that is not ascending returns JY_EINVAL and
 * stores nothing.  With JY_DEVICE the call only enqueues, apart from the
 * read-back of leaf_offs[0] and leaf_offs[n] that sizes the arena; handles_out
 * is complete after jy_sync.  With JY_HOST it blocks.
 * jy_ujson_leaves_get: item i = the encoded leaf of handles[i] (handles_mem
 * says where `handles` lives, `mem` where leaf_bytes / leaf_offs[n + 1] do).
 * Two-phase like the wire calls: sizes_out = {bytes needed, handles not in
 * the store}; if cap_bytes is too small NOTHING is written (JY_OK).  An
 * unknown handle, and handle 0, give an EMPTY item (unambiguous: a stored
 * leaf has at least 4 bytes).  n == 0 writes the single offset 0.  Read-only.
 * jy_ujson_leaves_reserve: a table for nleaves leaves and an arena of nbytes
 * bytes in all (a leaf takes its length rounded up to 8), so that puts within
 * them neither rehash nor reallocate.
 * jy_ujson_leaves_usage: out4 = {leaves, arena bytes used, arena capacity,
 * collisions} (synchronising).
 * jy_ujson_leaves_collect: drops every leaf whose handle is not LIVE and
 * rebuilds the table and the arena around the rest.  A handle is live if it is
 * (a) the elem of an element of a document of the state, slots 0 ..
 * nkeys[JY_UJSON], in either layout; (b) the same in the pending-delta store
 * (a local INS that a peer's delta already removed from the state is still
 * flushed later, and its flush must find the leaf); or (c) one of the n_keep
 * handles in `keep` (keep_mem says where the array lives) -- the KEEP RULE: a
 * caller that has put leaves and not yet written their elements passes their
 * handles here.  Handle 0 in `keep` is ignored.  Dead runs of the element
 * pools are not walked.  Handles do not change: they are hashes of the leaves,
 * so no element, pending delta or digest is touched.  The LOST-HANDLE RULE: a
 * handle that was put but neither written into a document nor passed in
 * `keep` loses its leaf; putting the same leaf again restores it under the
 * same handle.  out6 = {leaves kept, arena bytes kept, leaves dropped, arena
 * bytes dropped, live elements examined whose handle has no stored leaf,
 * keep handles with no stored leaf}; the last two are reports, not errors
 * (handles may be opaque).  Without JY_LEAVES_SHRINK table and arena keep
 * their capacities, so a jy_ujson_leaves_reserve still holds; with it the
 * table becomes the one a put would make for 2 x kept leaves and the arena
 * max(64 KiB, 2 x kept bytes), neither larger than before.  The new buffers
 * are allocated before the old ones are freed: JY_ENOMEM leaves the store as
 * it was.  The call is synchronising; it reads the state behind whatever
 * converges are in flight on the engine stream, as jy_ujson_path_read does.
 * Unknown flags and a keep_mem that is neither JY_HOST nor JY_DEVICE are
 * JY_EINVAL; a store that was never used gives JY_OK and six zeros.  The LOCK
 * RULE: under a node the call is made under jy_node_lock_type(node, JY_UJSON),
 * which waits for the queued UJSON jobs whose leaves were already put.
 * Under a node these calls touch a store that the UJSON worker's engine calls
 * share a stream and a memory pool with: they are made under
 * jy_node_lock_type(node, JY_UJSON), NEVER under JY_NODE_NOFENCE. */
int32_t jy_ujson_leaves_put(jy_engine* eng, uint64_t n, const uint8_t* leaf_bytes, const uint64_t* leaf_offs,
                            uint64_t* handles_out, int32_t mem);
int32_t jy_ujson_leaves_get(jy_engine* eng, uint64_t n, const uint64_t* handles, int32_t handles_mem,
                            uint64_t cap_bytes, uint8_t* leaf_bytes, uint64_t* leaf_offs,
                            uint64_t* sizes_out /* [2] */, int32_t mem);
int32_t jy_ujson_leaves_reserve(jy_engine* eng, uint64_t nleaves, uint64_t nbytes);
int32_t jy_ujson_leaves_usage(jy_engine* eng, uint64_t* out4);
#define JY_LEAVES_SHRINK 1u /* also shrink the table and the arena to 2 x what is kept */
int32_t jy_ujson_leaves_collect(jy_engine* eng, uint64_t n_keep, const uint64_t* keep, int32_t keep_mem,
                                uint32_t flags, uint64_t* out6);

/* ---- UJSON path reads (jy_ujson_path_read): the leaves at or under a path ----
 * RepoUJSON is a path-addressed store (repo_ujson.pony:68-110): GET renders
 * the leaves at or under a path, path-scoped CLR and SET remove them.  Query
 * i asks for the live elements of document slots[i] whose leaf lies at or
 * under path i = path_bytes[path_offs[i] .. path_offs[i + 1]): the path's
 * segments in the leaf encoding (4-byte little-endian length plus bytes each),
 * WITHOUT the FF FF FF FF terminator.  Such a path is a byte prefix of a
 * leaf's encoding iff its segments are a prefix of the leaf's path (the equal
 * length words keep the segment boundaries aligned; no segment length is
 * 0xFFFFFFFF), so membership is one prefix compare per element, on the
 * device, and only the matches travel.  An empty path selects the whole
 * document; slots[i] == JY_NO_SLOT is a key that does not exist (an empty
 * result); the same slot may appear in several queries.
 * The QUERY (slots, path_bytes, path_offs) is host memory and checked in full
 * before anything is launched: path_offs must ascend and every path must
 * parse into whole segments (else JY_EINVAL), every segment length must be
 * <= 2^24 - 1 and every slot JY_NO_SLOT or < jy_keys_count(JY_UJSON) (else
 * JY_ERANGE); flags other than JY_PATH_LEAVES are JY_EINVAL.  A refused call
 * writes nothing but zeros to sizes_out.
 * OUTPUTS live where `mem` says.  el_offs[n + 1] is a CSR over the queries;
 * elems holds the matched handles, one entry per live element (dot), in the
 * document's converge order (dots ascending, for documents in the per-column
 * layout too): a leaf inserted concurrently under two dots appears twice.
 * With JY_PATH_LEAVES item j of leaf_bytes / leaf_offs[matched + 1] is matched
 * element j's encoding with the query's path prefix removed, i.e. the
 * encoding of (relative path, value), at least 4 bytes.  Without the flag no
 * byte is gathered, leaf_bytes / leaf_offs may be null and sizes_out[1] = 0.
 * Two-phase like jy_ujson_leaves_get: sizes_out = {matched elements, leaf
 * bytes, elements examined, examined elements whose handle is not in the leaf
 * store}; if cap_el or cap_bytes is too small NOTHING is written (JY_OK).  An
 * element whose handle is not in the store cannot be matched: it is left out
 * and counted in sizes_out[3].  n == 0 writes the single offset 0 to each
 * non-null offsets array.  Read-only.  JY_HOST blocks; with JY_DEVICE the
 * call waits for its two total read-backs only and the outputs are complete
 * after jy_sync.
 * Under a node: under jy_node_lock_type(node, JY_UJSON), NEVER under
 * JY_NODE_NOFENCE, as the leaf store calls above. */
#define JY_PATH_LEAVES 1u /* also return the matched leaves' bytes */
int32_t jy_ujson_path_read(jy_engine* eng, uint64_t n, const uint32_t* slots, const uint8_t* path_bytes,
                           const uint64_t* path_offs /* [n + 1] */, uint32_t flags, uint64_t cap_el,
                           uint64_t cap_bytes, uint64_t* el_offs /* [n + 1] */, uint64_t* elems /* [cap_el] */,
                           uint8_t* leaf_bytes /* [cap_bytes] */, uint64_t* leaf_offs /* [cap_el + 1] */,
                           uint64_t* sizes_out /* [4] */, int32_t mem);

/* ---- keyed reads (jy_*_get_keys): GET by key string, answers in reply form ----
 * The read path of every non-UJSON type for a batch of keys AS THE RESP LAYER
 * HAS THEM: RepoTREG.get (repo_treg.pony:54-63), RepoTLOG.get / size / cutoff
 * (repo_tlog.pony:69-96), RepoGCOUNT / RepoPNCOUNT.get (repo_gcount.pony:53-55,
 * repo_pncount.pony:55-57).  The slot reads above (jy_treg_read, jy_tlog_read,
 * jy_gcount_get) leave the lookup, JY_NO_SLOT and one jy_arena_read per long
 * value to the caller; these calls take key strings and return found flags,
 * timestamps and the value bytes packed back to back, gathered on the device.
 * All three are READ-ONLY: no state, pending set, arena or key directory
 * changes (a key that is not interned is not created).
 * QUERY: n key strings, key_bytes / key_offs[n + 1] (as jy_keys_lookup);
 * keys_mem (JY_HOST / JY_DEVICE) says where they live, independently of `mem`.
 * A key may repeat in one query: each occurrence is answered.  A key that was
 * never interned is a normal answer (found = 0 and the type's bottom), not an
 * error.  JY_HOST key offsets are checked on the host, before anything is
 * launched: offsets that do not ascend return JY_EINVAL and write nothing.
 * OUTPUTS live where `mem` says (sizes_out is host memory).  n == 0 writes the
 * single offset 0 to each offsets array and returns JY_OK.  Two-phase like
 * jy_ujson_path_read: sizes_out is always filled; if a capacity is too small
 * NOTHING else is written (JY_OK, sizes only: pass zero capacities to size).
 * JY_HOST blocks; with JY_DEVICE the call waits only for the read-backs of its
 * totals and the outputs are complete after jy_sync.
 * Under a node these calls read state that converges change: they are made
 * under jy_node_lock_type(node, type), NEVER under JY_NODE_NOFENCE.
 *
 * jy_treg_get_keys: found[i] = 1 iff key i is interned; ts[i] and value i
 * (val_bytes[val_offs[i] .. val_offs[i + 1])) are its register.  A missing key
 * gives found 0, ts 0 and an empty value; a key converged to ("", 0) gives
 * found 1, ts 0 and an empty value (GET answers nil only for the former).
 * Pending duplicates are folded before the read and a duplicate-list overflow
 * fails the call after its read-back (JY_ERANGE), as for jy_treg_read.
 * sizes_out = {value bytes, keys found}.
 *
 * jy_tlog_get_keys: count is HOST memory, u64[n], or NULL for "every entry";
 * UINT64_MAX means the same (Pony's -1 default).  Query i returns its
 * take = min(size[i], count[i]) newest entries, newest first, on equal
 * timestamps the greater value first (the order of jy_tlog_read), as entries
 * [ent_offs[i], ent_offs[i + 1]) of ts / val_bytes / val_offs[entries + 1].
 * size[i] is the log's full length whatever the count and cutoff[i] its
 * cutoff: count[i] == 0 serves SIZE and CUTOFF without touching an entry, and
 * entries past `take` are never read.  A missing key gives found 0, size 0,
 * cutoff 0 and no entries; a key that exists with an empty log (after CLR)
 * gives found 1, size 0 and its cutoff.  Outstanding merges are settled first,
 * as for every TLOG state read.  sizes_out = {entries, value bytes, keys
 * found}; capacities cap_ent (ts; val_offs holds cap_ent + 1) and
 * cap_val_bytes.
 *
 * jy_counter_get_keys: type JY_GCOUNT or JY_PNCOUNT (else JY_ETYPE).  out[i] =
 * the key's value, 0 for a missing key; for PNCOUNT (sum P - sum N) as bits
 * (an int64).  No capacity: both outputs hold n elements. */
int32_t jy_treg_get_keys(jy_engine* eng, uint64_t n, const uint8_t* key_bytes, const uint64_t* key_offs,
                         int32_t keys_mem, uint64_t cap_val_bytes, uint8_t* found /* [n] */, uint64_t* ts /* [n] */,
                         uint8_t* val_bytes, uint64_t* val_offs /* [n + 1] */, uint64_t* sizes_out /* [2] */,
                         int32_t mem);
int32_t jy_tlog_get_keys(jy_engine* eng, uint64_t n, const uint8_t* key_bytes, const uint64_t* key_offs,
                         int32_t keys_mem, const uint64_t* count /* host [n] or NULL */, uint64_t cap_ent,
                         uint64_t cap_val_bytes, uint8_t* found /* [n] */, uint64_t* size /* [n] */,
                         uint64_t* cutoff /* [n] */, uint64_t* ent_offs /* [n + 1] */, uint64_t* ts /* [cap_ent] */,
                         uint8_t* val_bytes, uint64_t* val_offs /* [cap_ent + 1] */, uint64_t* sizes_out /* [3] */,
                         int32_t mem);
int32_t jy_counter_get_keys(jy_engine* eng, int32_t type, uint64_t n, const uint8_t* key_bytes,
                            const uint64_t* key_offs, int32_t keys_mem, uint8_t* found /* [n] */,
                            uint64_t* out /* [n] */, int32_t mem);

/* ---- RESP replies (jy_*_get_resp): the keyed GETs answered as reply bytes ----
 * The keyed reads above answer in columns; these answer in the bytes a client
 * reads, written on the device exactly as jemc/pony-resp's Respond writes them
 * (restated in csrc/host_repo.hip), so no caller formats a reply on the host.
 * All numbers are decimal, without leading zeros and without '+'.
 *   TREG GET k             key interned: *2\r\n$<len>\r\n<value>\r\n:<ts>\r\n
 *                          never interned: $-1\r\n  (a register converged to
 *                          ("", 0) is interned: *2\r\n$0\r\n\r\n:0\r\n)
 *   TLOG GET k [count]     *<take>\r\n, then per entry
 *                          *2\r\n$<len>\r\n<value>\r\n:<ts>\r\n ; never interned
 *                          or emptied by CLR: *0\r\n
 *   TLOG SIZE k            :<size>\r\n           never interned: :0\r\n
 *   TLOG CUTOFF k          :<cutoff>\r\n         never interned: :0\r\n
 *   GCOUNT GET k           :<u64>\r\n            never interned: :0\r\n
 *   PNCOUNT GET k          :<i64>\r\n ('-' for negatives), never interned: :0\r\n
 * QUERY and CONTRACT as for the keyed reads: READ-ONLY (no state, pending set,
 * arena or key directory changes); n key strings in key_bytes / key_offs[n + 1],
 * in the memory keys_mem names, independently of `mem`; a key may repeat, each
 * occurrence is answered; JY_HOST key offsets that do not ascend return
 * JY_EINVAL and write nothing.
 * OUTPUT: reply i is reply_bytes[reply_offs[i] .. reply_offs[i + 1]), the
 * replies lie back to back in query order; both arrays live where `mem` says
 * (sizes_out is host memory), and reply_bytes may start at any byte address.
 * Two-phase: sizes_out is always filled; if cap_bytes is smaller than the reply
 * bytes NOTHING else is written (JY_OK, sizes only: pass 0 to size).  n == 0
 * writes the single offset 0.  JY_HOST blocks; with JY_DEVICE the call waits
 * only for the read-backs of its totals and the outputs are complete after
 * jy_sync.
 * Under a node these calls read state that converges change: they are made
 * under jy_node_lock_type(node, type), NEVER under JY_NODE_NOFENCE.
 *
 * jy_treg_get_resp: pending duplicates are folded before the read and a
 * duplicate-list overflow fails the call after its read-back (JY_ERANGE), as
 * for jy_treg_get_keys.  sizes_out = {reply bytes, keys found}.
 *
 * jy_tlog_get_resp: what is HOST memory, u8[n] of JY_TLOG_RD_*, or NULL for GET
 * throughout; any other value returns JY_EINVAL before anything is launched
 * and writes nothing.  count is HOST memory, u64[n], or NULL for "every
 * entry"; UINT64_MAX means the same.  A GET returns its take = min(size,
 * count) newest entries, newest first, on equal timestamps the greater value
 * first, exactly the entries jy_tlog_get_keys returns.  SIZE and CUTOFF ignore
 * count and touch no entry.  Outstanding merges are settled first, as for every
 * TLOG state read.  sizes_out = {reply bytes, entries, keys found}.
 *
 * jy_counter_get_resp: type JY_GCOUNT or JY_PNCOUNT (else JY_ETYPE).
 * sizes_out = {reply bytes, keys found}. */
enum { JY_TLOG_RD_GET = 0, JY_TLOG_RD_SIZE = 1, JY_TLOG_RD_CUTOFF = 2 };
int32_t jy_treg_get_resp(jy_engine* eng, uint64_t n, const uint8_t* key_bytes, const uint64_t* key_offs,
                         int32_t keys_mem, uint64_t cap_bytes, uint8_t* reply_bytes /* [cap_bytes] */,
                         uint64_t* reply_offs /* [n + 1] */, uint64_t* sizes_out /* [2] */, int32_t mem);
int32_t jy_tlog_get_resp(jy_engine* eng, uint64_t n, const uint8_t* key_bytes, const uint64_t* key_offs,
                         int32_t keys_mem, const uint8_t* what /* host [n] or NULL */,
                         const uint64_t* count /* host [n] or NULL */, uint64_t cap_bytes,
                         uint8_t* reply_bytes /* [cap_bytes] */, uint64_t* reply_offs /* [n + 1] */,
                         uint64_t* sizes_out /* [3] */, int32_t mem);
int32_t jy_counter_get_resp(jy_engine* eng, int32_t type, uint64_t n, const uint8_t* key_bytes,
                            const uint64_t* key_offs, int32_t keys_mem, uint64_t cap_bytes,
                            uint8_t* reply_bytes /* [cap_bytes] */, uint64_t* reply_offs /* [n + 1] */,
                            uint64_t* sizes_out /* [2] */, int32_t mem);

/* ---- UJSON replies (jy_ujson_get_resp): GET key [path...] rendered on the device ----
 * The UJSON member of the family above (k_uj_render.hip): query i is the key
 * string i and path i, and reply i is the bytes a client reads for
 * `UJSON GET key path...`,
 *     $<len>\r\n<text>\r\n
 * A key never interned, a document without a leaf at or under the path and an
 * empty document all give $0\r\n\r\n (repo_ujson.pony:68-72).
 * THE TEXT.  The reference leaves the order of set members and map keys open
 * (Pony Map iteration); this call fixes one, the STORED ORDER, stated once in
 * csrc/jy_uj_render.hpp and, on the host, as ujson_doc.render_stored_order:
 *   - a query's leaves are the distinct encodings relative to its path that
 *     jy_ujson_path_read returns with JY_PATH_LEAVES (len|segment ... FF FF FF
 *     FF value); a leaf held under two dots counts once;
 *   - they are ordered by unsigned byte compare of the whole encoding, a proper
 *     prefix first: under a node its children come first, by the bytes of their
 *     encoded segment (the four length bytes as stored, then the key), then the
 *     node's own values by the bytes of their text;
 *   - a node's items are {"k":<child>,...} if it has children, then each value's
 *     stored text verbatim; one item renders bare, several as [item,item,...];
 *     keys go between quotes verbatim.
 * QUERY: n key strings as for the calls above (key_bytes / key_offs[n + 1] in
 * keys_mem).  The n paths are HOST memory in the jy_ujson_path_read encoding,
 * path i = path_bytes[path_offs[i] .. path_offs[i + 1]); path_offs == NULL means
 * every path is empty.  The paths are checked in full before anything is
 * launched, with the path read's rules and codes (JY_EINVAL: offsets that do
 * not ascend, a path that ends inside a length word or whose last segment is
 * cut short; JY_ERANGE: a segment longer than 2^24 - 1 bytes); nothing is
 * written then.
 * LEFT TO THE HOST: a query with a leaf more than JY_UJSON_RENDER_DEPTH
 * segments below its path, or with a key segment holding a byte below 0x20,
 * '"' or '\' (the device escapes nothing), is not rendered: on_host[i] = 1,
 * its reply range is empty, and the caller renders it (0x20, 0x7F and bytes
 * above are rendered).  on_host[i] = 0 for every other query.
 * OUTPUT: reply_bytes / reply_offs[n + 1] as above, on_host u8[n] in the same
 * memory.  sizes_out[6] (host) = {reply bytes, keys found, distinct leaves
 * rendered, elements examined, queries left to the host, examined elements
 * whose handle is not in the leaf store (not rendered)}.  Two-phase, n == 0,
 * JY_HOST / JY_DEVICE, read-only, any reply_bytes address and the node lock
 * (jy_node_lock_type(node, JY_UJSON)) exactly as for the calls above. */
enum { JY_UJSON_RENDER_DEPTH = 31 };
int32_t jy_ujson_get_resp(jy_engine* eng, uint64_t n, const uint8_t* key_bytes, const uint64_t* key_offs,
                          int32_t keys_mem, const uint8_t* path_bytes /* host */,
                          const uint64_t* path_offs /* host [n + 1] or NULL */, uint64_t cap_bytes,
                          uint8_t* reply_bytes /* [cap_bytes] */, uint64_t* reply_offs /* [n + 1] */,
                          uint8_t* on_host /* [n] */, uint64_t* sizes_out /* [6] */, int32_t mem);

/* ---- UJSON INS / RM / CLR by KEY STRING (jy_ujson_write_keys, k_uj_put.hip) ----
 * RepoUJSON.ins / rm / clr (repo_ujson.pony:85-110) for a batch of n commands as
 * the RESP layer has them -- op[i] (JY_UJSON_INS / _RM / _CLR), the key string
 * (key_bytes / key_offs[n + 1]) and the LEAF in the leaf store's encoding
 * (leaf_bytes / leaf_offs[n + 1] as jy_ujson_leaves_put takes them; empty for a
 * CLR) -- applied in command order to the column of replica `identity`
 * (registered if new), however often a key repeats.  No slot and no element
 * handle crosses to the host.  `mem` (JY_HOST / JY_DEVICE) applies to every array.
 *   keys     the keys of the INS commands are interned (created on a miss, as
 *            _data_for does); those of RM / CLR are looked up, and a miss is a
 *            no-op that creates nothing (repo_ujson.pony:86,108).  The interning
 *            comes first: an RM that precedes, in the same batch, the INS that
 *            creates its key runs on the empty document -- the same state and
 *            the same pending set as skipping it.
 *   leaves   an INS leaf is put into the leaf store from device memory; an RM
 *            leaf is only hashed (a remove never grows the store); an INS whose
 *            put gives handle 0 (a malformed leaf, a 64-bit collision) fails the
 *            call with JY_EINVAL before any document changes.
 *   order    the commands are grouped by document; the j-th command of every
 *            document runs in round j, each round one write of one command per
 *            document.  A batch without a repeated document is one round.
 * Host arrays are checked in full before anything is launched; device arrays by
 * one check kernel whose verdict is read back first.  An unknown op or offsets
 * that do not ascend are JY_EINVAL, a key or a leaf over 2^24 - 1 bytes
 * JY_ERANGE; nothing is applied, interned or put then.
 * Keys, segments and values are bytes here (binary-safe); the text-only
 * restriction of the host path belongs to UJSONDocs.apply.
 * LOCKING as for jy_ujson_get_resp: the caller holds the lock it puts leaves
 * under; on a node, jy_node_lock_type(node, JY_UJSON).
 * jy_ujson_write_keys_info (read-only): out6 = {[0] calls that applied their
 * batch, [1] the rounds of the last of them, [2] the rounds of all of them, [3]
 * the commands the last call applied, [4] the RM / CLR commands it skipped for a
 * missing key, [5] the INS leaves it handed to the leaf store}. */
int32_t jy_ujson_write_keys(jy_engine* eng, uint64_t n, const uint8_t* op, const uint8_t* key_bytes,
                            const uint64_t* key_offs, const uint8_t* leaf_bytes, const uint64_t* leaf_offs,
                            uint64_t identity, int32_t mem);
int32_t jy_ujson_write_keys_info(jy_engine* eng, uint64_t* out6);

/* ---- RESP requests (jy_resp_decode): client bytes decoded into keyed batches ----
 * The request side of the path above: the bytes clients SENT, framed, split
 * into words, classified and parsed on the device (k_resp_in.hip), and
 * returned as the column batches the keyed calls take -- jy_counter_write_keys,
 * jy_treg_set_keys, jy_tlog_write_keys and the jy_*_get_resp calls -- so no
 * caller frames a command or parses a decimal on the host.  READ-ONLY: the
 * engine's state does not change; the caller makes the keyed calls.
 * The rules (tokens, numbers, classes) are csrc/jy_resp_in.hpp's: only the
 * array-of-bulk-strings form `*<n>\r\n` + n x `$<len>\r\n<bytes>\r\n`, <n> and
 * <len> 1 to 20 decimal digits; bulk strings are binary-safe.
 * INPUT: req_bytes holds the receive buffers of nconn connections back to
 * back, in req_mem (JY_HOST / JY_DEVICE), at any byte address; connection c is
 * req_bytes[conn_offs[c] .. conn_offs[c + 1]).  conn_offs is HOST memory (it is
 * the call's plan) and ascending, else JY_EINVAL; conn_offs[nconn] above
 * 2^32 - 2 is JY_ERANGE.  Each connection's range starts at a command boundary
 * and may end anywhere.  Device input is checked before any length in it is
 * trusted: no length a client sent moves a read outside its connection.
 * OUTPUT, two-phase like the keyed reads: sizes_out (host) = {commands, words,
 * rows, key bytes, value bytes, groups} is always filled; caps[6] (host) are
 * the capacities in the same order, and if any is short NOTHING else is
 * written (JY_OK, sizes only: pass zeros to size).  The arrays live where `mem`
 * says, except the group table, which is host memory.  JY_HOST blocks; with
 * JY_DEVICE the call waits only for the read-backs of its totals and the
 * device arrays are complete after jy_sync (the group table on return).
 *   per connection   conn_used[c]: the bytes that formed complete, well-formed
 *                    commands (the caller keeps the tail); conn_err[c] = 1 iff
 *                    what starts at conn_used[c] holds a definite violation
 *                    (the connection is to be closed).  Commands before that
 *                    point stand, nothing after it is decoded.
 *   per command      in stream order (connection-major): cmd_conn, cmd_kind
 *                    (JY_CMD_*), cmd_phase, and its words: word cmd_word_offs[k]
 *                    + j is req_bytes[word_off[w] .. + word_len[w]), so a host
 *                    answering a JY_CMD_HOST command does not frame again.
 *   rows             the commands of every kind but JY_CMD_HOST, stably sorted
 *                    by (phase, kind): row_cmd[r] = the command; its key and
 *                    value gathered into key_bytes / key_offs[rows + 1] and
 *                    val_bytes / val_offs[rows + 1] (an empty value for a kind
 *                    without one); num[r] = ts, amount (PNCOUNT: the i64's
 *                    bits), TRIM count or GET count (UINT64_MAX: all; an
 *                    unparsable GET count reads as all); op[r] = JY_TLOG_* for
 *                    JY_CMD_TLOG_WRITE, JY_TLOG_RD_* for JY_CMD_TLOG_READ, else 0.
 *   groups (host)    group g is the rows group_offs[g] .. group_offs[g + 1] of
 *                    phase group_phase[g] and kind group_class[g], ascending by
 *                    (phase, kind).  key_bytes with key_offs + group_offs[g] IS
 *                    the key_bytes / key_offs[n + 1] argument of the group's
 *                    keyed call, in the same memory, and so for the values,
 *                    num (ts / arg / val / count) and op (op / what).
 * PHASES: a command's phase is the number of kind changes before it in its own
 * connection (JY_CMD_HOST is a kind).  Commands of different connections have
 * no mutual order and those of one connection are of one kind per phase, so
 * the groups run in ascending phase, one keyed call each (and the host's
 * answers to the JY_CMD_HOST commands of that phase), apply every connection's
 * commands in its own order; rows keep stream order inside a group.  More than
 * 2^24 phases in one call is JY_ERANGE.
 * JY_CMD_HOST: UJSON and SYSTEM commands, an unknown type or op, a missing
 * word, a number that does not parse, a command of no words, a key or value
 * longer than 2^24 - 1 bytes (which a keyed call would reject for the batch).
 *
 * jy_resp_decode_opts is jy_resp_decode with `flags`; flags 0 IS jy_resp_decode.
 * JY_RESP_UJSON_GET makes `UJSON GET key [segment...]` a keyed kind of its own,
 * JY_CMD_UJSON_GET, which appears ONLY under this flag (every other UJSON
 * command, and every UJSON command without the flag, stays JY_CMD_HOST): word 0
 * is exactly UJSON, word 1 exactly GET, at least 3 words, the key (word 2) and
 * every path segment (words 3 .. nwords - 1, however many) at most 2^24 - 1
 * bytes -- the render's JY_ERANGE limit, so a command that breaks it goes to
 * the host instead of failing its batch.  The row's key is word 2; its VALUE is
 * the path in the jy_ujson_path_read encoding, built on the device: per segment
 * the 4-byte little-endian length, then the bytes, no terminator, empty for a
 * GET of the whole document.  sizes_out[4] (value bytes) includes the paths;
 * num and op are 0.  The kind counts for the phases like any other: UJSON SET
 * (JY_CMD_HOST) followed by UJSON GET on one connection is a phase change.
 * val_bytes with val_offs + group_offs[g] of such a group are well-formed paths
 * by construction and are what jy_resp_exec_opts hands to the render.
 *
 * JY_RESP_UJSON_WRITE, independent of JY_RESP_UJSON_GET (flags without it run
 * none of its code), makes three UJSON writes a keyed kind, JY_CMD_UJSON_WRITE,
 * which appears ONLY under this flag; word 0 is exactly UJSON:
 *   INS key [segment...] value, RM key [segment...] value   at least 4 words, the
 *     key and every segment (words 3 .. nwords - 2) at most 2^24 - 1 bytes, the
 *     LAST word a PLAIN value, the whole leaf encoding at most 2^24 - 1 bytes
 *     (the leaf store's limit): op = JY_UJSON_INS / JY_UJSON_RM
 *   CLR key   exactly 3 words: op = JY_UJSON_CLR, an empty value
 * UJSON SET, a CLR with a path and anything that breaks these rules stay
 * JY_CMD_HOST.  PLAIN VALUE (csrc/jy_resp_in.hpp ujson_value_plain): a stored
 * leaf holds the canonical text of its JSON primitive and the device does not
 * canonicalise, so the value word must already BE that text: at most 255 bytes
 * and exactly true, false or null; an integer -?(0|[1-9][0-9]{0,17}) other than
 * -0; or a string of bytes 0x20 .. 0x7E without '"' and '\' between two '"'.
 * Floats, exponents, blanks, escapes, non-ASCII bytes, 19 digits and longer
 * values go to the host, which canonicalises or rejects them as before.
 * The row's key is word 2; its VALUE is the leaf in the leaf store's encoding
 * (jy_ujson_leaves_put), built on the device: per segment the 4-byte
 * little-endian length and the bytes, then FF FF FF FF, then the value word's
 * bytes.  num is 0.  Keys and segments are binary-safe here, as for the GET; the
 * text-only restriction belongs to the host's UJSONDocs.apply.  The kind counts
 * for the phases like any other: UJSON INS | UJSON SET | UJSON GET on one
 * connection is three phases.
 * JY_CMD_NKINDS counts the kinds 0 .. 10; JY_CMD_NKINDS_ALL those and
 * JY_CMD_UJSON_WRITE. */
enum { JY_RESP_UJSON_GET = 1, JY_RESP_UJSON_WRITE = 2 };
enum {
  JY_CMD_HOST = 0,
  JY_CMD_GCOUNT_INC = 1,  /* GCOUNT INC k v        jy_counter_write_keys(JY_GCOUNT, sign 0) */
  JY_CMD_GCOUNT_GET = 2,  /* GCOUNT GET k          jy_counter_get_resp(JY_GCOUNT) */
  JY_CMD_PNCOUNT_INC = 3, /* PNCOUNT INC k v       jy_counter_write_keys(JY_PNCOUNT, sign 0) */
  JY_CMD_PNCOUNT_DEC = 4, /* PNCOUNT DEC k v       jy_counter_write_keys(JY_PNCOUNT, sign 1) */
  JY_CMD_PNCOUNT_GET = 5, /* PNCOUNT GET k         jy_counter_get_resp(JY_PNCOUNT) */
  JY_CMD_TREG_SET = 6,    /* TREG SET k value ts   jy_treg_set_keys */
  JY_CMD_TREG_GET = 7,    /* TREG GET k            jy_treg_get_resp */
  JY_CMD_TLOG_WRITE = 8,  /* TLOG INS / TRIMAT / TRIM / CLR      jy_tlog_write_keys */
  JY_CMD_TLOG_READ = 9,   /* TLOG GET [count] / SIZE / CUTOFF    jy_tlog_get_resp */
  JY_CMD_UJSON_GET = 10,  /* UJSON GET k [segment...]            jy_ujson_get_resp; ONLY under JY_RESP_UJSON_GET */
  JY_CMD_NKINDS = 11
};
enum {
  JY_CMD_UJSON_WRITE = 11, /* UJSON INS / RM k [segment...] value, CLR k   jy_ujson_write_keys; ONLY under JY_RESP_UJSON_WRITE */
  JY_CMD_NKINDS_ALL = 12
};
int32_t jy_resp_decode(jy_engine* eng, uint64_t nconn, const uint8_t* req_bytes, int32_t req_mem,
                       const uint64_t* conn_offs /* host [nconn + 1] */, const uint64_t* caps /* host [6] */,
                       uint64_t* conn_used /* [nconn] */, uint8_t* conn_err /* [nconn] */,
                       uint32_t* cmd_conn, uint8_t* cmd_kind, uint32_t* cmd_phase /* [caps[0]] */,
                       uint64_t* cmd_word_offs /* [caps[0] + 1] */, uint64_t* word_off,
                       uint64_t* word_len /* [caps[1]] */, uint32_t* row_cmd /* [caps[2]] */, uint8_t* key_bytes,
                       uint64_t* key_offs /* [caps[2] + 1] */, uint8_t* val_bytes,
                       uint64_t* val_offs /* [caps[2] + 1] */, uint64_t* num, uint8_t* op /* [caps[2]] */,
                       uint32_t* group_phase, uint8_t* group_class /* host [caps[5]] */,
                       uint64_t* group_offs /* host [caps[5] + 1] */, uint64_t* sizes_out /* [6] */, int32_t mem);
int32_t jy_resp_decode_opts(jy_engine* eng, uint64_t nconn, const uint8_t* req_bytes, int32_t req_mem,
                            const uint64_t* conn_offs /* host [nconn + 1] */, const uint64_t* caps /* host [6] */,
                            uint64_t* conn_used, uint8_t* conn_err, uint32_t* cmd_conn, uint8_t* cmd_kind,
                            uint32_t* cmd_phase, uint64_t* cmd_word_offs, uint64_t* word_off, uint64_t* word_len,
                            uint32_t* row_cmd, uint8_t* key_bytes, uint64_t* key_offs, uint8_t* val_bytes,
                            uint64_t* val_offs, uint64_t* num, uint8_t* op, uint32_t* group_phase,
                            uint8_t* group_class, uint64_t* group_offs, uint64_t* sizes_out /* [6] */, int32_t mem,
                            uint32_t flags /* JY_RESP_* */);

/* ---- RESP execute (jy_resp_exec, jy_resp_replies): request bytes to reply bytes ----
 * The two paths above joined in one call (k_resp_out.hip): the receive buffers
 * of a heartbeat's connections are decoded, their commands applied and answered,
 * and ONE reply byte stream per connection is assembled on the device.  No
 * caller walks the group table, frames +OK or re-orders replies by connection.
 * jy_resp_exec CHANGES STATE, so it cannot be "called once to size, again to
 * write" as the reads are: its result stays in engine-owned device memory until
 * the next jy_resp_exec or jy_engine_destroy, and jy_resp_replies copies it out.
 *
 * jy_resp_exec.  INPUT exactly jy_resp_decode's: req_bytes / req_mem / conn_offs
 * (host) under the same rules, with the same error codes.  The decoder's own
 * core decodes into engine-owned device memory; the groups run in ascending
 * phase, one keyed call per group by the JY_CMD_* table above (the counter
 * writes to the column of `identity`, registered if new), each with the group's
 * slices of the decoded columns in device memory: no decoded key byte, value
 * byte, num or op element crosses to the host.  In each phase the keyed groups
 * run first, then that phase's JY_CMD_HOST commands are answered through
 * on_host, in command order:
 *   on_host(ctx, cmd, nwords, words, lens, sink)   cmd = the command's index in
 *     stream order; words[j] / lens[j] = its words as HOST pointers, valid
 *     during the callback only -- into req_bytes for JY_HOST input, into one
 *     copy of the HOST commands' words for JY_DEVICE input.  It answers with
 *     jy_resp_sink_write(sink, bytes, n), any number of times (the pieces are
 *     appended; no call at all is an answer of zero bytes) and returns 0; the
 *     answers are uploaded once per call.  It may call the engine (the calls of a
 *     host-side UJSON repo), but not jy_resp_exec or jy_resp_replies.
 * sizes_out (host) = {commands, reply bytes, JY_CMD_HOST commands, groups,
 * keyed calls made, phases}.
 * FAILURES.  JY_CMD_HOST commands with on_host NULL: JY_EINVAL before anything
 * is applied.  A keyed call that fails, or an on_host that returns non-zero
 * (JY_EINVAL, jy_last_error says which command), stops the call with that code:
 * the groups already run STAND, exactly as after the same keyed calls made by
 * hand, sizes_out[3] = the groups completed, and NO replies are retained (nor
 * are those of an earlier call: jy_resp_replies returns JY_EINVAL).
 *
 * jy_resp_replies.  READ-ONLY: copies the retained result out in one piece.
 * Connection c's replies are reply_bytes[conn_reply_offs[c] ..
 * conn_reply_offs[c + 1]): the replies of its complete commands in command
 * order, back to back, connections in input order; a connection without a
 * complete command has an empty range.  conn_used / conn_err are the decoder's.
 * The four arrays live where `mem` says; reply_bytes may start at any byte
 * address.  sizes_out (host) = {reply bytes, connections} is always filled; if
 * cap_bytes is short NOTHING else is written (JY_OK, sizes only) and the call
 * can be repeated.  JY_EINVAL if nothing is retained or nconn differs from the
 * retained call's.  JY_HOST blocks; JY_DEVICE outputs are complete after jy_sync.
 *
 * jy_resp_exec_opts is jy_resp_exec with `flags` (JY_RESP_*) and eight sizes;
 * flags 0 IS jy_resp_exec (sizes_out[6], [7] = 0).  Under JY_RESP_UJSON_GET the
 * decode is jy_resp_decode_opts', and a JY_CMD_UJSON_GET group makes ONE render
 * call (the core of jy_ujson_get_resp) with the group's slices of the decoded
 * key and value columns, keys and paths in device memory; its replies are
 * ranges of the reply pool like those of the other read groups.  The queries
 * the render leaves to the host (LEFT TO THE HOST above: a key to escape, a leaf
 * more than JY_UJSON_RENDER_DEPTH segments down) are answered through on_host
 * with the command's words under the contract above: after that phase's keyed
 * groups, together with and in command order among the phase's JY_CMD_HOST
 * commands.  For JY_DEVICE input their words take one further small copy, made
 * only when a group left something.  Such a query with on_host NULL fails the
 * call with JY_EINVAL at that group, under the failure rule above.
 * sizes_out[8] = the six above, then {UJSON GETs rendered on the device, UJSON
 * GETs left to on_host}.
 * Under JY_RESP_UJSON_WRITE a JY_CMD_UJSON_WRITE group is ONE call of the core
 * of jy_ujson_write_keys with the group's slices of the decoded op, key and
 * value (leaf) columns in device memory, to the column of `identity`; its
 * replies are the shared +OK.  sizes_out stays eight entries; what the write
 * groups did is read with jy_ujson_write_keys_info.  A group that fails (a
 * 64-bit leaf collision) stops the call under the failure rule above.
 * LOCKING as for jy_ujson_get_resp, which a flagged call contains: the render
 * reads the leaf store and the keyed write puts into it, so the caller holds
 * the lock it puts leaves under, and on a node the call is made under
 * jy_node_lock_type(node, JY_UJSON). */
typedef struct jy_resp_sink jy_resp_sink;
int32_t jy_resp_sink_write(jy_resp_sink* sink, const uint8_t* bytes, uint64_t n);
typedef int32_t (*jy_resp_host_fn)(void* ctx, uint64_t cmd, uint64_t nwords, const uint8_t* const* words,
                                   const uint64_t* lens, jy_resp_sink* sink);
int32_t jy_resp_exec(jy_engine* eng, uint64_t nconn, const uint8_t* req_bytes, int32_t req_mem,
                     const uint64_t* conn_offs /* host [nconn + 1] */, uint64_t identity, jy_resp_host_fn on_host,
                     void* ctx, uint64_t* sizes_out /* host [6] */);
int32_t jy_resp_exec_opts(jy_engine* eng, uint64_t nconn, const uint8_t* req_bytes, int32_t req_mem,
                          const uint64_t* conn_offs /* host [nconn + 1] */, uint64_t identity,
                          jy_resp_host_fn on_host, void* ctx, uint32_t flags /* JY_RESP_* */,
                          uint64_t* sizes_out /* host [8] */);
int32_t jy_resp_replies(jy_engine* eng, uint64_t nconn, uint64_t cap_bytes, uint8_t* reply_bytes,
                        uint64_t* conn_reply_offs /* [nconn + 1] */, uint64_t* conn_used /* [nconn] */,
                        uint8_t* conn_err /* [nconn] */, uint64_t* sizes_out /* host [2] */, int32_t mem);

/* ---- State digest in key-hash buckets (jy_*_state_digest) ----
 * Whether two stores hold the same state, and where they differ, without
 * moving the state: the canonical digest of the slots [slot0, slot0 + nslots),
 * computed on the GPU and split into `nbuckets` buckets by key hash.
 * The digest of a range is the digest of its jy_*_state_wire dump: a WRAPPING
 * 64-bit SUM over keys of per-key hashes, keyed by the key STRING and by
 * replica IDS (never by slot or column), in which any changed field changes
 * the sum (csrc/jy_digest.hpp has the hash functions).  So it depends on
 * neither key order, slot order, column order nor the shard count: a node's
 * digest is the wrapping sum of its shards' digests, and stores that hold the
 * same data agree.  Every slot of the range is a key, bottom state included;
 * counter cells and UJSON vv entries equal to 0 contribute nothing; counters
 * read the registered and allocated columns, as jy_counter_state_wire does.
 * BUCKETS: nbuckets = B is a power of two, 1 <= B <= 2^20.  With kh =
 * dbytes(key) (FNV-1a 64 over the key's bytes, then dcomb with its length),
 *     bucket(kh, B) = 0                                  if B == 1
 *                   = dmix(kh ^ 0x7A00) >> (64 - log2 B)  otherwise
 * (dmix: the splitmix64 step).  Peers must agree on this formula and on B.
 * out[B][4] is OVERWRITTEN (not accumulated) with, per bucket, {digest, keys,
 * items, w3}: items = the non-zero cells (counters), registers (TREG: one a
 * key), entries (TLOG) or elements (UJSON); w3 = the wrapping sum of the cell
 * values (counters), the value bytes (TREG, TLOG) or the cloud dots (UJSON).
 * Chunks of a range, and shards of a node, add up row by row (wrapping).
 * Read-only, like jy_*_state_wire: no state, pending set, arena or key
 * directory changes.  `mem` says where `out` lives; JY_HOST blocks, JY_DEVICE
 * leaves `out` complete after jy_sync.  A range that reaches past the
 * interned keys returns JY_ERANGE, a type that is no counter JY_ETYPE
 * (jy_counter_state_digest), an nbuckets that is 0, no power of two or above
 * 2^20 JY_EINVAL; each sets jy_last_error and writes nothing.  nslots == 0
 * gives an all-zero out.  The TLOG call settles outstanding merges first (as
 * every TLOG state read does).
 * Under a node these calls read state that converges change: they are made
 * under jy_node_lock_type(node, type), NEVER under JY_NODE_NOFENCE. */
int32_t jy_counter_state_digest(jy_engine* eng, int32_t type, uint64_t slot0, uint64_t nslots, uint32_t nbuckets,
                                uint64_t* out /* [nbuckets][4] */, int32_t mem);
int32_t jy_treg_state_digest(jy_engine* eng, uint64_t slot0, uint64_t nslots, uint32_t nbuckets,
                             uint64_t* out /* [nbuckets][4] */, int32_t mem);
int32_t jy_tlog_state_digest(jy_engine* eng, uint64_t slot0, uint64_t nslots, uint32_t nbuckets,
                             uint64_t* out /* [nbuckets][4] */, int32_t mem);
int32_t jy_ujson_state_digest(jy_engine* eng, uint64_t slot0, uint64_t nslots, uint32_t nbuckets,
                              uint64_t* out /* [nbuckets][4] */, int32_t mem);
/* the slots of [slot0, slot0 + nslots) whose key falls into a bucket whose
 * bit is set in bucket_bits (HOST memory, (nbuckets + 63) / 64 words, bucket b
 * = bit b & 63 of word b >> 6), ascending: the list jy_*_state_wire_slots
 * takes.  *n_out (host) always receives their number; if cap < that number
 * nothing else is written (JY_OK: the two-phase convention of the wire
 * calls), else slots_out (`mem`) receives them.  Read-only; errors and
 * locking as the digest calls. */
int32_t jy_state_bucket_slots(jy_engine* eng, int32_t type, uint64_t slot0, uint64_t nslots, uint32_t nbuckets,
                              const uint64_t* bucket_bits, uint64_t cap, uint32_t* slots_out, uint64_t* n_out,
                              int32_t mem);

/* the counter snapshot's cell writer stores by output position while a key's
 * rows (signs x registered columns) fit this many mask bits, and falls back
 * to a lane per key above it (same output; for tests of that boundary) */
uint32_t jy_counter_state_mask_rows(void);

/* cumulative converge counters since the engine was made (synchronising):
 * [0] touched state elements, [1] touched state cloud dots, [2] elements
 * written, [3] cloud dots written, [4] delta elements, [5] delta cloud dots,
 * [6] delta documents, [7] converge calls.  Bench / telemetry only: the
 * bytes a converge really moved.  [0..3] count the regular merge path only. */
int32_t jy_ujson_stats(jy_engine* eng, uint64_t* out8);
/* the same eight, then the in-place layout of long documents:
 * [8] delta docs converged in place, [9] / [10] their state elements / cloud
 * dots (examined by the join, never read), [11] / [12] elements / cloud dots
 * appended, [13] cloud dots folded into the vv, [14] documents promoted to
 * the per-column layout, [15] documents demoted to the regular path */
int32_t jy_ujson_stats_ext(jy_engine* eng, uint64_t* out16);
/* UJSON in-place layout (an engine choice, invisible in every result): a
 * document whose merged state holds at least min_elems elements keeps one
 * element run and one cloud run per replica column with room behind it, so
 * a delta whose dots all lie above what the document's column holds (the
 * usual case: fresh inserts) is appended where it lies instead of rewriting
 * the document.  0 stops promotions (documents already in the layout stay).
 * Default 512 (env JY_UJ_LONG_MIN); needs ujson_columns <= 64. */
int32_t jy_ujson_set_inplace(jy_engine* eng, uint32_t min_elems);

/* ---- multi-GPU routing: the exchange step of a key-hash-sharded node ----
 * Replaces nothing in the reference (every node holds every key there); it is
 * the intra-node analogue of Cluster.broadcast_deltas (cluster.pony:209-213).
 * Runs have a FIXED capacity per destination, so the all-to-all is an
 * equal-split collective and the counts travel on the device with the data:
 * no host round trip per batch.
 *
 * Sender: jy_treg_route_part partitions n ingested TREG entries (owner
 * shard, slot on the owner, ts, pre, lr) into nshards runs:
 *   recs_dev  u64[nshards][cap][4] {slot, ts, pre, lr'}, 16-B aligned; lr' of a
 *             value > 8 bytes addresses the run's own bytes (8-byte granules)
 *   bytes_dev u8[nshards][cap_byte], cap_byte a multiple of 8
 *   hdr_dev   u64[nshards][2]: records / value bytes placed per destination
 *             (written by the call); entries keep their input order in a run
 *             and the placed ones are a prefix of each destination's sequence
 *   ovf_dev   u32[1 + n]: [0] = entries that did not fit (ZERO on entry), then
 *             their input indices -- the caller sends those in a later round.
 * Receiver: jy_treg_converge_routed merges nsrc received runs (the same
 * layout, source-major, each source's hdr row) in one launch; a key named by
 * several sources is exact (LWW join).  All pointers are device memory
 * except the `mem`-tagged inputs; both calls only enqueue. */
void jy_keys_owner(uint64_t n, const uint8_t* key_bytes, const uint64_t* key_offs, uint32_t nshards,
                   uint32_t* owner_out);
int32_t jy_treg_route_part(jy_engine* eng, uint64_t n, const uint32_t* owner, const uint32_t* slot,
                           const uint64_t* ts, const uint64_t* pre, const uint64_t* lr, uint32_t nshards,
                           uint64_t cap, uint64_t cap_byte, int32_t mem, uint64_t* recs_dev, uint8_t* bytes_dev,
                           uint64_t* hdr_dev, uint32_t* ovf_dev);
/* The same partition on the shard `self` (< nshards) that owns part of its
 * own batch: the entries with owner == self are merged into eng's registers
 * where they lie (the keyed LWW merge, enqueued before the partition) and
 * never enter a run; run `self` stays empty (hdr row 0), its overflow list
 * never names them.  The receivers' merge is unchanged (an empty run costs
 * one launch that reads its count), and at nshards == 1 the caller may skip
 * it and the run buffers altogether. */
int32_t jy_treg_route_part_self(jy_engine* eng, uint64_t n, const uint32_t* owner, const uint32_t* slot,
                                const uint64_t* ts, const uint64_t* pre, const uint64_t* lr, uint32_t nshards,
                                uint32_t self, uint64_t cap, uint64_t cap_byte, int32_t mem, uint64_t* recs_dev,
                                uint8_t* bytes_dev, uint64_t* hdr_dev, uint32_t* ovf_dev);
int32_t jy_treg_converge_routed(jy_engine* eng, uint32_t nsrc, uint64_t cap, uint64_t cap_byte,
                                const uint64_t* recs_dev, const uint8_t* bytes_dev, const uint64_t* hdr_dev);
/* The same merge when the byte runs were received straight into this
 * engine's arena: jy_arena_reserve(eng, JY_TREG, nsrc * cap_byte, &dst,
 * &rebase) hands out the arena's tail (dst stays valid until the next call
 * that grows that arena), the exchange (or, for the sender's own run,
 * jy_treg_route_part with bytes_dev = dst) writes there, and
 * jy_treg_converge_routed_at merges with the runs at arena offset `rebase`
 * -- no append copy of the byte runs. */
int32_t jy_arena_reserve(jy_engine* eng, int32_t type, uint64_t bytes, uint8_t** dev_out, uint64_t* rebase_out);
int32_t jy_treg_converge_routed_at(jy_engine* eng, uint32_t nsrc, uint64_t cap, uint64_t cap_byte,
                                   const uint64_t* recs_dev, const uint64_t* hdr_dev, uint64_t rebase);

/* ---- cross-shard key resolution (k_keyroute.hip): `_data_for(key)`
 * (repo_treg.pony:37-42, every repo_*.pony) when the key's slot lives on
 * another GPU.  All pointers are device memory; the calls only enqueue.
 * Sender: jy_keys_route_part computes every key's owner (jy_key_owner, on the
 * device) and regroups the keys by owner for a variable all-to-all:
 *   owner_out u32[n], pos_out u32[n] (each key's index in owner order),
 *   send_lens u64[n] and send_bytes u8[total key bytes] in owner order,
 *   counts_out u64[2 * nshards]: keys per owner, then bytes per owner.
 * Owner: jy_keys_intern_lens interns the n received keys (lengths + bytes)
 *   in its directory -- create on miss, like jy_keys_intern_mem -- and
 *   writes their slots (it synchronises, as interning does).
 * Sender, once the slots came back in its owner order:
 *   jy_keys_route_back writes slots_out[i] = answers[pos[i]]. */
int32_t jy_keys_route_part(jy_engine* eng, uint64_t n, const uint8_t* key_bytes, const uint64_t* key_offs,
                           uint32_t nshards, uint32_t* owner_out, uint32_t* pos_out, uint64_t* send_lens,
                           uint8_t* send_bytes, uint64_t* counts_out);
int32_t jy_keys_intern_lens(jy_engine* eng, int32_t type, uint64_t n, const uint8_t* bytes, const uint64_t* lens,
                            uint32_t* slots_out);
int32_t jy_keys_route_back(jy_engine* eng, uint64_t n, const uint32_t* pos, const uint32_t* answers,
                           uint32_t* slots_out);

/* ---- routing TLOG logs and UJSON documents (k_route_csr.hip) ----
 * The CSR counterpart of the TREG pair above: a key travels with its whole
 * log / document.  Each destination gets one RUN of jy_route_words(type,
 * cap_k, caps) u64 words, a complete converge batch of cap_k records (TLOG
 * caps = {cap_e}; UJSON caps = {cap_e, cap_v, cap_c} for elements, vv
 * entries, cloud dots); runs_dev is u64[nshards][words], 16-B aligned.
 * Keys keep their input order in a run; the first key of a destination that
 * does not fit (records, entries or long-value bytes) and every later one go
 * to ovf_dev (u32[1 + n]: [0] the count, ZERO before the first call; calls
 * append key_base + their input index, so the chunks of one batch -- key
 * ranges passed as offset pointers with the full entry arrays -- share one
 * list); unused records are holes the receiver skips.  hdr_dev
 * u64[nshards][8] receives per run the keys, the entries per CSR and (TLOG)
 * the value bytes placed (zeroed by the call).  Offsets are absolute: a
 * chunk's ent_offs[0] may be > 0 and nent bounds the entries it names.  TLOG value bytes go to bytes_dev
 * (u8[nshards][cap_byte], cap_byte a multiple of 8); UJSON runs need
 * cap_k >= 2 (the last record is a hole spanning the unused capacity).
 * Receiver: nsrc received runs, source-major; each source's run is merged
 * in turn (TLOG rewrites the runs' value handles in place).  Device-memory
 * pointers except the `mem`-tagged inputs; the calls only enqueue.  A
 * device batch with an owner >= nshards drops that key (counted in
 * jy_skipped). */
uint64_t jy_route_words(int32_t type, uint64_t cap_k, const uint64_t* caps);
int32_t jy_tlog_route_part(jy_engine* eng, uint64_t n, const uint32_t* owner, const uint32_t* slot,
                           const uint64_t* cutoff, const uint64_t* ent_offs, uint64_t nent, const uint64_t* ts,
                           const uint64_t* pre, const uint64_t* lr, uint32_t nshards, uint64_t cap_k, uint64_t cap_e,
                           uint64_t cap_byte, uint64_t key_base, int32_t mem, uint64_t* runs_dev, uint8_t* bytes_dev,
                           uint64_t* hdr_dev, uint32_t* ovf_dev);
int32_t jy_tlog_converge_routed(jy_engine* eng, uint32_t nsrc, uint64_t cap_k, uint64_t cap_e, uint64_t cap_byte,
                                uint64_t* runs_dev, const uint8_t* bytes_dev);
int32_t jy_ujson_route_part(jy_engine* eng, uint64_t n, const uint32_t* owner, const uint32_t* slot,
                            const uint64_t* el_offs, uint64_t nel, const uint64_t* dots, const uint64_t* elems,
                            const uint64_t* vv_offs, uint64_t nvv, const uint64_t* vv, const uint64_t* cloud_offs,
                            uint64_t ncloud, const uint64_t* cloud, uint32_t nshards, uint64_t cap_k, uint64_t cap_e,
                            uint64_t cap_v, uint64_t cap_c, uint64_t key_base, int32_t mem, uint64_t* runs_dev,
                            uint64_t* hdr_dev, uint32_t* ovf_dev);
int32_t jy_ujson_converge_routed(jy_engine* eng, uint32_t nsrc, uint64_t cap_k, uint64_t cap_e, uint64_t cap_v,
                                 uint64_t cap_c, const uint64_t* runs_dev);

/* ---- the node: every GPU of one Jylis node behind one handle (jy_node.hip) ----
 * Replaces, for the whole node, Database.converge_deltas (jylis/database.pony:50-51)
 * -> RepoManager.converge_deltas -> RepoManagerCore.converge_deltas
 * (jylis/repo_manager.pony:30-31,92-93): ONE call per decoded peer batch, its
 * keys hash-sharded over the node's GPUs (owner = jy_key_owner(key, S)).  The
 * reference has no sharding (every node holds every key); the exchange step
 * is the intra-node analogue of Cluster.broadcast_deltas (cluster.pony:205-213).
 *
 * A node has S shards (one engine each).  One process may drive all of them
 * (the Pony host: nlocal = S) or several processes one each (nlocal = 1,
 * rank0 = the process's rank, one ncclUniqueId shared by all of them).
 * Per converge call, per shard: the batch the process passed is cut into
 * nlocal contiguous key ranges, one per local shard (its ingest); each ingest
 * shard hashes its keys on the device and regroups keys and payload by owner;
 * the per-owner counts are exchanged (RCCL, or a host transposition for the
 * copy fabric) and read back once; the payload moves with grouped
 * ncclSend/ncclRecv over xGMI (or device copies); each owner interns the keys
 * it received in its device directory (_data_for, create on miss) and
 * merges them -- TREG and counters all sources in one launch (LWW / max are
 * joins, repeats are exact), TLOG and UJSON one source after another (a key
 * two peers sent is merged twice, exactly).  No slot crosses the host and
 * no key is resolved by a round trip: the key bytes travel with their delta.
 *
 * Every process of a multi-process node makes the same node calls in the
 * same order (they are collectives), each with its own batch (possibly
 * empty).  Errors: JY_* codes, detail in jy_node_last_error.  Reads, local
 * writes and flushes go to the owner's engine (jy_node_engine).
 *
 * One node per process, shared by every CRDT type (round 5).  The converge
 * calls ENQUEUE: a call checks its arguments, copies host inputs into a
 * pinned block the node owns (JY_HOST inputs are free to reuse when it
 * returns) and queues a job; one worker thread per node runs the jobs in call
 * order -- the count exchange, the key directory's miss count and every other
 * host wait of a converge happen there, never on the caller's thread (a Pony
 * scheduler thread).  The five RepoManager actors may call from five threads
 * at once: their jobs run one at a time, so the node's ONE communicator sees
 * one group at a time, issued from one thread (database.pony:18-23 makes the
 * five actors; cluster.pony:205-213 is the broadcast this replaces).  A
 * queued job's failure is returned by the node's next call (converge, fence,
 * lock, sync, stats) and its detail by jy_node_last_error.
 * JY_DEVICE inputs are read by the worker later, and on streams of the node's
 * own (the read-back stream reads offsets, value lengths and value heads
 * beside the engine stream): they must be complete device-wide before the
 * call (no pending write on any stream) and stay valid and unchanged until
 * jy_node_fence (every queued job issued to its streams) AND the GPU work
 * reading them has finished -- jy_node_sync returns after both.  The engines of a node (jy_node_engine) are shared
 * with the worker: use them between jy_node_lock and jy_node_unlock (the
 * lock first waits for every job queued before it), or after jy_node_sync
 * with no node call in flight. */
typedef struct jy_node jy_node;
#define JY_NODE_MAX_SHARDS 64
#define JY_FABRIC_RCCL 0 /* RCCL communicator over the shards' GPUs (one GPU per shard)   */
#define JY_FABRIC_COPY 1 /* device copies: one process, shards may share a GPU (tests)      */
typedef struct jy_node_config {
  uint32_t nshards;                     /* S: key shards of the node                        */
  uint32_t nlocal;                      /* shards this process drives: rank0 .. rank0+nlocal-1 */
  uint32_t rank0;                       /* first local shard                               */
  uint32_t fabric;                      /* JY_FABRIC_*                                     */
  int32_t devices[JY_NODE_MAX_SHARDS];  /* HIP device of each local shard                  */
  uint8_t unique_id[128];               /* RCCL: one ncclUniqueId for every process of the
                                           node (jy_node_unique_id on one of them); with
                                           nlocal == nshards an all-zero id means "make one" */
  jy_config engine;                     /* each shard's engine (device overridden)         */
} jy_node_config;

int32_t jy_node_unique_id(uint8_t* id_out /* 128 bytes */);
int32_t jy_node_create(const jy_node_config* cfg, jy_node** out);
/* the one-process node of an FFI host without struct layouts (the Pony
 * host): nshards shards on devices[0..nshards), every one local, an RCCL
 * communicator of its own (fabric JY_FABRIC_RCCL) or device copies */
int32_t jy_node_create_local(uint32_t nshards, const int32_t* devices, uint32_t fabric, const jy_config* engine,
                             jy_node** out);
/* The process's shared node (round 5): the first call makes a one-process
 * node over every visible GPU (jy_node_create_local, RCCL, `engine` for each
 * shard); later calls return the same node.  Reference counted: the last
 * jy_node_release destroys it.  The five GPU repos of a Jylis process (one
 * RepoManager actor each, database.pony:18-22) share it, so one communicator
 * and one engine per GPU serve every CRDT type. */
int32_t jy_node_acquire_local(const jy_config* engine, jy_node** out);
void jy_node_release(jy_node* node);
/* GPUs visible to this process (0 without a GPU or HIP runtime) */
int32_t jy_device_count(void);
void jy_node_destroy(jy_node* node);
/* the detail of the calling thread's last failed node call (per thread, like
 * errno: the repos call one node from their own threads) */
const char* jy_node_last_error(const jy_node* node);
uint32_t jy_node_nshards(const jy_node* node);
/* the engine of local shard `shard` (global index), NULL if not local */
jy_engine* jy_node_engine(jy_node* node, uint32_t shard);
uint32_t jy_node_shard_of(const jy_node* node, const uint8_t* key, uint64_t len);
/* register a replica identity on every local shard (the same column on all:
 * every process registers the cluster's identities in one order).  A known
 * identity is answered without waiting for the worker; a new one takes the
 * node's lock (not a fence) */
int32_t jy_node_replica_col(jy_node* node, uint64_t replica_id, uint32_t* col_out);
/* every queued job issued and its GPU work finished on every shard's streams
 * (blocks); then a queued job's failure, if any -- the streams are drained on
 * that path too, so JY_DEVICE inputs may be freed once it returns */
int32_t jy_node_sync(jy_node* node);
/* every job queued before this call issued to the GPU streams (blocks until
 * the worker took them, not for the GPU); device inputs of those calls are
 * no longer read by the host side, and the GPU reads them in stream order */
int32_t jy_node_fence(jy_node* node);
/* exclusive use of the node's engines: waits for the jobs queued before it
 * (as jy_node_fence), then holds the node's lock until jy_node_unlock.  The
 * lock is held even when an earlier job's failure is returned. */
int32_t jy_node_lock(jy_node* node);
void jy_node_unlock(jy_node* node);
/* the same, waiting only for the jobs of CRDT type `type` queued before it
 * (round 6): the types' engine states are disjoint and every engine call the
 * holder makes is ordered after the issued jobs on the engine stream, so a
 * TREG read does not wait for queued UJSON converges.  JY_NODE_NOFENCE waits
 * for no job (a read of state no converge changes: deltas_size, flush).  The
 * lock is held even when a job's failure is returned.  The wire-form flushes
 * (jy_*_flush_wire) are engine calls made under JY_NODE_NOFENCE as well: they
 * read no state a converge changes, but the worker may be growing the key
 * directory they read the names from, so the lock is needed.  The state
 * snapshots (jy_*_state_wire) are different: they read state that converges
 * change, so they are made under jy_node_lock_type(node, type), NOT under
 * JY_NODE_NOFENCE. */
#define JY_NODE_NOFENCE (-1)
int32_t jy_node_lock_type(jy_node* node, int32_t type);
/* jobs queued or running: of CRDT type `type`, or all with type < 0 */
int32_t jy_node_pending(jy_node* node, int32_t type, uint64_t* n_out);
/* the worker reclaims a shard's TREG / TLOG value arena after that type's
 * jobs once its dead bytes pass twice the live ones (+ 1 MiB): the policy the
 * Pony glue ran after every drain under the lock.  Off by default; callers
 * that pack value handles must consume them under the lock. */
int32_t jy_node_arena_gc(jy_node* node, uint32_t enable);
/* The payload schedule one shard of the exchange issues (host logic only, no
 * GPU; the node's exchange runs exactly this): for S shards, shard `rank`,
 * W count granules, nwires wire columns (granule, element bytes) and the
 * shard's per-peer element counts send_cnt / recv_cnt [S][W], the ordered
 * operations ops_out[i] = {kind (0 own part copied, 1 send, 2 receive), wire,
 * peer, source offset, destination offset, bytes}, at most cap of them;
 * *nops_out = how many there are.  Tests check it for S = 2..8 (every send
 * meets a receive of the same size, one peer order on every rank). */
int32_t jy_node_exchange_plan(uint32_t S, uint32_t rank, uint32_t W, uint32_t nwires, const int32_t* wire_gran,
                              const int32_t* wire_esize, const uint64_t* send_cnt, const uint64_t* recv_cnt,
                              uint64_t cap, uint64_t* ops_out, uint64_t* nops_out);

/* Converge one decoded peer batch (per process).  Keys: n strings (key_bytes,
 * key_offs[n + 1]).  `mem` = JY_HOST (staged per ingest shard) or JY_DEVICE
 * (readable by every local shard's GPU).  Offsets may start above 0.
 *   counters: key i's cells are [cell_offs[i], cell_offs[i+1]) of (sign 0 = P /
 *             1 = N, NULL: all P; col = jy_node_replica_col; val): s = max(s, val)
 *   TREG:     (ts[i], value bytes [val_offs[i], val_offs[i+1]))
 *   TLOG:     cutoff[i]; entries [ent_offs[i], ent_offs[i+1]) of (ts, value bytes
 *             [val_offs[e], val_offs[e+1])), canonical order (as jy_tlog_converge)
 *   UJSON:    as jy_ujson_converge, per document (dots carry node columns) */
int32_t jy_node_counter_converge(jy_node* node, int32_t type, uint64_t n, const uint8_t* key_bytes,
                                 const uint64_t* key_offs, const uint64_t* cell_offs, const uint8_t* sign,
                                 const uint16_t* col, const uint64_t* val, int32_t mem);
int32_t jy_node_treg_converge(jy_node* node, uint64_t n, const uint8_t* key_bytes, const uint64_t* key_offs,
                              const uint64_t* ts, const uint8_t* val_bytes, const uint64_t* val_offs, int32_t mem);
int32_t jy_node_tlog_converge(jy_node* node, uint64_t n, const uint8_t* key_bytes, const uint64_t* key_offs,
                              const uint64_t* cutoff, const uint64_t* ent_offs, const uint64_t* ts,
                              const uint8_t* val_bytes, const uint64_t* val_offs, int32_t mem);
int32_t jy_node_ujson_converge(jy_node* node, uint64_t n, const uint8_t* key_bytes, const uint64_t* key_offs,
                               const uint64_t* el_offs, const uint64_t* dots, const uint64_t* elems,
                               const uint64_t* vv_offs, const uint64_t* vv, const uint64_t* cloud_offs,
                               const uint64_t* cloud, int32_t mem);
/* Dense counter blocks arriving MIXED (the bench's routed PNCOUNT step, and a
 * peer that shards like this node: it flushes shard by shard).  This process
 * ingests ncols peer columns for the keys of every owner: vals_p / vals_n
 * are device arrays [ncols][S][nslots] (vals_n NULL for GCOUNT), block
 * [c][d] holding owner d's slots [slot0, slot0 + nslots).  cols_all[r * ncols
 * + c] is the column of shard r's c-th peer (every process passes the whole
 * table).  Column c of every shard crosses in one exchange; the owner merges
 * the S received columns with one block converge while column c + 1 is in
 * flight on a second stream.  Device memory only. */
int32_t jy_node_counter_converge_block(jy_node* node, int32_t type, uint32_t ncols, const uint16_t* cols_all,
                                       uint32_t slot0, uint32_t nslots, const uint64_t* vals_p,
                                       const uint64_t* vals_n);
/* telemetry of the node's last converge call (not on the reference's
 * surface): [0] keys ingested, [1] keys received, [2] bytes sent, [3] bytes
 * received (this process's local shards), [4] exchange calls so far */
int32_t jy_node_stats(jy_node* node, uint64_t* out5);

#ifdef __cplusplus
}
#endif
#endif /* JYLIS_GPU_H */
