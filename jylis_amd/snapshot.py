"""Snapshot files: the state of an Engine or a Node on disk, and back.

save() walks every type's state as wire batches (Engine.snapshot /
Node.snapshot: jy_*_state_wire, the arrays jy_node_*_converge takes) and
writes each chunk to its own file; load() converges the chunks into a target
through its converge_wire().  This is the persistence the reference leaves
open (repo_manager.pony:100,107 "TODO: disk persistence?"), and the same
chunks bring a late peer up to date or feed a node with another shard count.

The file set is a directory:
  manifest.json              format version, the types, the chunk list with
                             each array's length, and the source's REPLICA ID
                             TABLE [jy_replica_id(c) for c in range(count)]
  t<type>_s<shard>_c<n>.npz  numpy.savez of one chunk's arrays (WIRE_ARRAYS
                             names and dtypes); arrays only, never pickled,
                             and loaded with allow_pickle=False

Columns are engine-local: a chunk's counter `col` and the top 16 bits of
UJSON `dots`, `vv` and `cloud` name the SOURCE's columns.  load() registers
the manifest's replica ids on the target, rewrites those columns to the
target's (remap_columns) and restores the ascending dot order converge
expects (sort_dots).  One chunk is resident at a time, in save and in load.

UJSON elements are opaque u64 handles, as on the flush wire.  With
save(leaves=True) every UJSON chunk also holds leaf_bytes / leaf_offs, the
encoded (path, value) leaf of each element from the source's device leaf
store (jy_ujson_leaves_get), and the manifest records "ujson_leaves": true;
load() then puts the leaves into the target's leaf store before it converges
the chunk, so the target can render its documents (ujson_doc.DeviceLeaves).
Without the flag the files are what they always were: handles only, the
leaves staying wherever the source's host layer keeps them.
"""
import json
import os

import numpy as np

from ._lib import GCOUNT, PNCOUNT, UJSON
from .engine import DOT_SEQ_BITS, DOT_SEQ_MASK, WIRE_ARRAYS, WIRE_OPTIONAL, has_leaves

FORMAT = "jylis-snapshot"
VERSION = 1
TYPES = (0, 1, 2, 3, 4)
_UJSON_DOTS = (("el_offs", "dots", "elems"), ("vv_offs", "vv", None), ("cloud_offs", "cloud", None))


def replica_ids(source):
    """the source's replica id table: ids[c] = jy_replica_id(c)"""
    if hasattr(source, "replica_ids"):
        return source.replica_ids()
    return [source.replica_id(c) for c in range(source.replica_count())]


def chunks_of(source, ctype, max_keys=65536, leaves=False):
    """(shard, wire batch) of one type, host arrays: an Engine is shard 0"""
    kw = {"leaves": True} if leaves and ctype == UJSON else {}
    if hasattr(source, "engines"):
        yield from source.snapshot(ctype, max_keys, **kw)
    else:
        for batch in source.snapshot(ctype, max_keys, **kw):
            yield 0, batch


def remap_columns(ctype, batch, col_map):
    """a wire batch with its columns rewritten: col_map[source column] = target
    column.  Touches the counters' `col` and the top 16 bits of UJSON `dots`,
    `vv` and `cloud`, nothing else (TREG / TLOG carry no column)."""
    out = dict(batch)
    m = np.asarray(col_map, np.uint64)
    if ctype in (GCOUNT, PNCOUNT):
        out["col"] = m[np.asarray(batch["col"], np.int64)].astype(np.uint16)
    elif ctype == UJSON:
        for _, name, _ in _UJSON_DOTS:
            d = np.asarray(batch[name], np.uint64)
            out[name] = (m[(d >> np.uint64(DOT_SEQ_BITS)).astype(np.int64)] << np.uint64(DOT_SEQ_BITS)) | (
                d & np.uint64(DOT_SEQ_MASK))
    return out


def sort_dots(ctype, batch):
    """UJSON: every document's dots, vv entries and cloud ascending again (a
    column remap permutes the column-major order); other types unchanged"""
    if ctype != UJSON:
        return batch
    out = dict(batch)
    for offs, name, payload in _UJSON_DOTS:
        o = np.asarray(batch[offs], np.int64)
        d = np.asarray(batch[name], np.uint64)
        order = np.lexsort((d, np.repeat(np.arange(len(o) - 1), np.diff(o))))
        out[name] = d[order]
        if payload:
            out[payload] = np.asarray(batch[payload], np.uint64)[order]
            if has_leaves(batch):  # the leaves are parallel to the elements: they move with them
                out["leaf_bytes"], out["leaf_offs"] = permute_items(batch["leaf_bytes"], batch["leaf_offs"], order)
    return out


def permute_items(item_bytes, item_offs, order):
    """the packed items (bytes, offs[n + 1]) order[0], order[1], ... packed again
    (a permutation, or any selection of them)"""
    b = np.asarray(item_bytes, np.uint8)
    o = np.asarray(item_offs, np.uint64).astype(np.int64)
    order = np.asarray(order, np.int64)
    lens = np.diff(o)[order]
    offs = np.zeros(len(order) + 1, np.int64)
    np.cumsum(lens, out=offs[1:])
    src = np.repeat(o[:-1][order] - offs[:-1], lens) + np.arange(int(offs[-1]))
    return b[src], offs.astype(np.uint64)


def save(source, path, types=TYPES, max_keys=65536, leaves=False):
    """write the state of `source` (an Engine or a Node) under directory `path`
    -> the manifest (also written to path/manifest.json).  leaves=True: the
    UJSON chunks carry their leaves (leaf_bytes, leaf_offs) and the manifest
    says "ujson_leaves": true; without it neither file differs from before."""
    from .repo import wire_to_host
    os.makedirs(path, exist_ok=True)
    chunks = []
    for ctype in types:
        counts = {}
        for shard, batch in chunks_of(source, ctype, max_keys, leaves):
            batch = wire_to_host(ctype, batch)
            c = counts.get(shard, 0)
            counts[shard] = c + 1
            name = f"t{ctype}_s{shard}_c{c}.npz"
            np.savez(os.path.join(path, name), **batch)
            chunks.append({"type": int(ctype), "shard": int(shard), "chunk": c, "file": name,
                           "sizes": {k: int(len(v)) for k, v in batch.items()}})
    # (the ids after the chunks: every column a chunk names is registered by then)
    manifest = {"format": FORMAT, "version": VERSION, "types": [int(t) for t in types],
                "replica_ids": [int(i) for i in replica_ids(source)], "chunks": chunks}
    if leaves:
        manifest["ujson_leaves"] = True
    with open(os.path.join(path, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)
    return manifest


def read_chunk(path, entry):
    """one chunk's arrays, checked against the manifest entry and WIRE_ARRAYS"""
    ctype = entry["type"]
    with np.load(os.path.join(path, entry["file"]), allow_pickle=False) as z:
        spec = [(name, dt) for name, dt, _, _ in WIRE_ARRAYS[ctype]]
        optional = [(name, dt) for name, dt in WIRE_OPTIONAL[ctype]]
        if optional and all(name in z.files for name, _ in optional):  # all of them or none
            spec += optional
        if sorted(z.files) != sorted(name for name, _ in spec):
            raise ValueError(f"{entry['file']}: arrays {sorted(z.files)} are not a type {ctype} wire batch")
        batch = {}
        for name, dt in spec:
            a = z[name]  # (an object array raises here: pickles are never loaded)
            if a.dtype != np.dtype(dt) or a.ndim != 1 or len(a) != entry["sizes"][name]:
                raise ValueError(f"{entry['file']}: {name} is {a.dtype}[{a.shape}], not what the manifest lists")
            batch[name] = a
    return batch


def load(path, target):
    """converge the snapshot under `path` into `target` (an Engine or a Node):
    registers the source's replica ids, then one converge_wire per chunk in
    manifest order -> the manifest"""
    with open(os.path.join(path, "manifest.json")) as f:
        manifest = json.load(f)
    if manifest.get("format") != FORMAT or manifest.get("version") != VERSION:
        raise ValueError(f"unknown snapshot format {manifest.get('format')!r} version {manifest.get('version')!r}")
    col_map = [target.replica_col(i) for i in manifest["replica_ids"]]
    same = col_map == list(range(len(col_map)))
    for entry in manifest["chunks"]:
        ctype = entry["type"]
        batch = read_chunk(path, entry)
        if not same:
            batch = sort_dots(ctype, remap_columns(ctype, batch, col_map))
        target.converge_wire(ctype, batch)
    return manifest
