// k_uj_path.hip -- UJSON path reads: the elements of a document whose leaf lies
// at or under a path, selected in HBM (jy_ujson_path_read).
//
// RepoUJSON is a path-addressed store (repo_ujson.pony:68-110): GET renders the
// leaves under a path, path-scoped CLR and SET remove them.  With documents
// (k_ujson.hip) and leaves (k_leaf.hip) both on the device, which elements a
// path selects is decided here and only the matches travel.  The leaf encoding
// (jy_leaf.hpp) makes it a byte comparison: a path encoded like a leaf's path,
// without the terminator, is a byte prefix of the leaf's encoding iff its
// segments are a prefix of the leaf's path -- the length words keep the segment
// boundaries aligned, and no segment length is the terminator FF FF FF FF.
//
// The query (slots, paths) is host memory and checked in full before anything
// is launched, so no device loop runs over an unchecked length.  Then:
//   sizes            jy_ujson_sizes_of + jy_scan_u64: eo[n + 1], the examined
//                    elements of every query (a JY_NO_SLOT query: none); the
//                    total is read back (first wait)
//   k_uj_path_match  flattened over the examined elements, a lane per element:
//                    its query by two wave_last_le searches per tile and a
//                    short bisect (as k_uj_gather_items: a document of 10^5
//                    elements spreads over many tiles); the handle through
//                    uj_elem_at (jy_internal.hpp, factored out of
//                    k_uj_gather_items<true>: regular pool or per-column long
//                    layout); the leaf table walked as k_leaf_lookup does;
//                    AFTER the walk the path against the leaf's leading bytes,
//                    8 at a time (path_prefix, noinline).  Writes the handle,
//                    the keep flag, the kept byte length and the lr.
//   scans            jy_scan_u64 over the flags and over the kept lengths
//                    and the read-back of their totals (second and last wait:
//                    "sizes only" when a capacity is short)
//   k_uj_path_offs   el_offs[i] = the flag scan at query i's first element
//   k_uj_path_compact  matched handles, their lr and skip (the path's length),
//                    and leaf_offs, each to its scanned position
//   k_wire_gather    LeafTailSrc (jy_wire.hpp: LeafSrc plus a per-item skip),
//                    balanced by output bytes: the relative leaves
//
// The path bytes are NOT staged in LDS: every lane of a tile inside one query
// reads the same one to three path words, which a wave loads as one broadcast
// line from L2; the lane's own dependent chain (handle, probe, leaf line) is
// what it waits for.  The staged form was not built, so there is no A/B.
//
// Roofline: latency-bound.  Per examined element one 16-byte element record,
// one probe chain (two dependent 8-byte loads at load factor <= 1/2) and one
// line of leaf bytes; per match its bytes once more, in the gather.  Times
// against the reads it replaces: DESIGN.md, "UJSON path reads"; nothing here
// was tuned to a profile.
//
// The kernels and the core (path_select, path_compact) are in jy_uj_path.hpp,
// which jy_ujson_get_resp (k_uj_render.hip) runs too; this file is the public
// call: the host checks, the slots to the device, and the outputs.

#include "jy_uj_path.hpp"

namespace {

// no element examined: every query's result is empty
int32_t nothing_matched(jy_engine* eng, int32_t mem, u64 n, u64* el_offs, u64* leaf_offs) {
  if (!el_offs) return empty_batch(eng, mem, {leaf_offs});  // (a sizing call without arrays)
  if (mem == JY_DEVICE) JY_HIP(eng, hipMemsetAsync(el_offs, 0, (n + 1) * 8, eng->stream));
  else std::memset(el_offs, 0, (n + 1) * 8);
  return empty_batch(eng, mem, {leaf_offs});
}

}  // namespace

extern "C" {

int32_t jy_ujson_path_read(jy_engine* eng, uint64_t n, const uint32_t* slots, const uint8_t* path_bytes,
                           const uint64_t* path_offs, uint32_t flags, uint64_t cap_el, uint64_t cap_bytes,
                           uint64_t* el_offs, uint64_t* elems, uint8_t* leaf_bytes, uint64_t* leaf_offs,
                           uint64_t* sizes_out, int32_t mem) {
  JY_HIP(eng, hipSetDevice(eng->device));
  for (int q = 0; q < 4; q++) sizes_out[q] = 0;
  JY_TRY(mem_check(eng, mem));
  if (flags & ~JY_PATH_LEAVES) return eng->fail(JY_EINVAL, "unknown path read flags");
  const bool leaves = flags & JY_PATH_LEAVES;
  if (!leaves) leaf_bytes = nullptr, leaf_offs = nullptr;
  if (n == 0) return empty_batch(eng, mem, {el_offs, leaf_offs});
  if (!slots || !path_offs) return eng->fail(JY_EINVAL, "slots and path_offs must not be null");
  // ---- the whole query is checked here, before any launch ----
  JY_TRY(path_query_check(eng, n, path_bytes, path_offs));
  const u64 nk = eng->nkeys[JY_UJSON];
  u64 holes = 0;
  for (u64 i = 0; i < n; i++) {
    if (slots[i] == JY_NO_SLOT) holes++;
    else if (slots[i] >= nk) return eng->fail(JY_ERANGE, "a path read names a slot past the interned keys");
  }
  if (holes == n) return nothing_matched(eng, mem, n, el_offs, leaf_offs);  // (no key may exist at all)

  Tmp tmp(eng);
  // the query -> the device (the caller's arrays outlive the call's first wait)
  u32* ds;
  const uint8_t* pb;
  const u64* po;
  JY_TRY(tmp.get(&ds, n));
  JY_HIP(eng, hipMemcpyAsync(ds, slots, n * 4, hipMemcpyHostToDevice, eng->stream));
  JY_TRY(path_stage(eng, tmp, n, path_bytes, path_offs, &pb, &po));
  PathSel S;
  JY_TRY(path_select(eng, tmp, n, ds, holes != 0, pb, po, leaves, S));
  sizes_out[2] = S.me;
  if (S.me == 0) return nothing_matched(eng, mem, n, el_offs, leaf_offs);
  const u64 m = S.m, bytes = S.bytes;
  sizes_out[0] = m;
  sizes_out[1] = bytes;
  sizes_out[3] = S.missing;
  if (cap_el < m || cap_bytes < bytes) return JY_OK;  // sizes only
  if (!el_offs || !elems) return eng->fail(JY_EINVAL, "el_offs or elems is null");
  if (leaves && (!leaf_offs || (bytes && !leaf_bytes))) return eng->fail(JY_EINVAL, "leaf_bytes or leaf_offs is null");

  // ---- compact, gather ----
  u64 *dq, *de, *dlo = nullptr, *klr = nullptr;
  u32* skip = nullptr;
  uint8_t* ob = nullptr;
  JY_TRY(tmp.out(&dq, el_offs, n + 1, mem));
  JY_TRY(tmp.out(&de, elems, m, mem));
  if (leaves) {
    JY_TRY(tmp.out(&dlo, leaf_offs, m + 1, mem));
    JY_TRY(tmp.get(&klr, m));
    JY_TRY(tmp.get(&skip, m));
    JY_TRY(tmp.out(&ob, leaf_bytes, bytes, mem));
  }
  JY_TRY(path_compact(eng, S, dq, de, klr, skip, dlo));
  if (leaves) JY_TRY(gather(eng, LeafTailSrc{eng->leaf.bytes, klr, skip}, dlo, m, bytes, ob));
  JY_TRY(emit(eng, mem, el_offs, dq, (n + 1) * 8));
  JY_TRY(emit(eng, mem, elems, de, m * 8));
  if (leaves) {
    JY_TRY(emit(eng, mem, leaf_bytes, ob, bytes));
    JY_TRY(emit(eng, mem, leaf_offs, dlo, (m + 1) * 8));
  }
  return host_sync(eng, mem);
}

}  // extern "C"
