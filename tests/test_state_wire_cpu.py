"""The host half of the state snapshot in wire form (jy_*_state_wire), without
a GPU: the four calls are declared alike in the header, _lib.SIGNATURES and
ffi.pony, and jylis_amd.snapshot saves and loads wire batches bit for bit,
keeps chunk order, remaps columns and rejects what it must not load."""
import json
import os
import re

import numpy as np
import pytest

from test_pony_glue import header_arity, pony_decls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("jy_counter_state_wire", "jy_treg_state_wire", "jy_tlog_state_wire", "jy_ujson_state_wire")


def test_header_binding_and_pony_declare_the_calls():
    from jylis_amd import _lib
    from jylis_amd.engine import WIRE_ARRAYS, WIRE_SIZES
    hdr, decl = header_arity(), pony_decls()
    for name in CALLS:
        assert name in hdr, f"{name} is not declared in include/jylis_gpu.h"
        assert name in _lib.SIGNATURES and name in decl
        assert hdr[name] == len(_lib.SIGNATURES[name][1]) == decl[name]
    # engine, [type], slot0, nslots, capacities (none for the keys), outputs, sizes_out, mem
    for ctype, name in ((0, CALLS[0]), (2, CALLS[1]), (3, CALLS[2]), (4, CALLS[3])):
        head = 2 if ctype == 0 else 1
        assert hdr[name] == head + 2 + (len(WIRE_SIZES[ctype]) - 1) + len(WIRE_ARRAYS[ctype]) + 2
    text = open(os.path.join(ROOT, "include", "jylis_gpu.h")).read()
    assert re.search(r"jy_node_lock_type\(node, type\), NOT under JY_NODE_NOFENCE", text)


def _u64(*x):
    return np.array(x, np.uint64)


def _dot(col, seq):
    return (col << 48) | seq


def _batches():
    """hand-made wire batches, two chunks for TREG: {ctype: [batch, ...]}"""
    kb = np.frombuffer(b"abcde", np.uint8)
    cnt = {"key_bytes": kb, "key_offs": _u64(0, 1, 3, 5), "cell_offs": _u64(0, 0, 2, 3),
           "sign": np.array([0, 0, 0], np.uint8), "col": np.array([0, 2, 1], np.uint16),
           "val": _u64(7, 2**64 - 1, 9)}
    pn = dict(cnt, sign=np.array([0, 1, 1], np.uint8))
    treg = [{"key_bytes": kb[:3], "key_offs": _u64(0, 1, 3), "ts": _u64(5, 0),
             "val_bytes": np.frombuffer(b"\x00\xffxyz", np.uint8), "val_offs": _u64(0, 5, 5)},
            {"key_bytes": kb[3:], "key_offs": _u64(0, 2), "ts": _u64(2**63), "val_bytes": np.zeros(0, np.uint8),
             "val_offs": _u64(0, 0)}]
    tlog = {"key_bytes": kb[:2], "key_offs": _u64(0, 1, 2), "cutoff": _u64(3, 0), "ent_offs": _u64(0, 0, 2),
            "ts": _u64(9, 4), "val_bytes": np.frombuffer(b"qrs", np.uint8), "val_offs": _u64(0, 1, 3)}
    uj = {"key_bytes": kb[:3], "key_offs": _u64(0, 1, 3), "el_offs": _u64(0, 3, 3),
          "dots": _u64(_dot(0, 4), _dot(1, 1), _dot(2, 6)), "elems": _u64(11, 12, 13),
          "vv_offs": _u64(0, 2, 3), "vv": _u64(_dot(0, 4), _dot(2, 6), _dot(1, 3)),
          "cloud_offs": _u64(0, 1, 2), "cloud": _u64(_dot(1, 9), _dot(0, 2**48 - 1))}
    return {0: [cnt], 1: [pn], 2: treg, 3: [tlog], 4: [uj]}


class FakeSource:
    """what snapshot.save asks of an Engine"""

    def __init__(self, ids):
        self.ids, self.b = list(ids), _batches()

    def replica_count(self):
        return len(self.ids)

    def replica_id(self, c):
        return self.ids[c]

    def snapshot(self, ctype, max_keys=65536):
        yield from self.b[ctype]


class FakeTarget:
    """records converge_wire calls; hands out columns for ids as `cols` says"""

    def __init__(self, cols):
        self.cols, self.got, self.asked = dict(cols), [], []

    def replica_col(self, rid):
        self.asked.append(rid)
        return self.cols[rid]

    def converge_wire(self, ctype, batch):
        self.got.append((ctype, batch))


IDS = [101, 202, 303]


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), k


def test_round_trip_bit_for_bit_and_in_order(tmp_path):
    from jylis_amd import snapshot
    src = FakeSource(IDS)
    man = snapshot.save(src, str(tmp_path))
    assert man["version"] == snapshot.VERSION and man["replica_ids"] == IDS and man["types"] == [0, 1, 2, 3, 4]
    assert [(c["type"], c["shard"], c["chunk"]) for c in man["chunks"]] == [
        (0, 0, 0), (1, 0, 0), (2, 0, 0), (2, 0, 1), (3, 0, 0), (4, 0, 0)]
    assert json.load(open(tmp_path / "manifest.json")) == man
    assert man["chunks"][2]["sizes"]["val_bytes"] == 5
    tgt = FakeTarget({101: 0, 202: 1, 303: 2})
    snapshot.load(str(tmp_path), tgt)
    assert tgt.asked == IDS
    want = [(t, b) for t in range(5) for b in src.b[t]]
    assert [t for t, _ in tgt.got] == [t for t, _ in want]
    for (_, got), (_, exp) in zip(tgt.got, want):
        _same(exp, got)


def test_column_remap_touches_columns_only(tmp_path):
    from jylis_amd import snapshot
    src = FakeSource(IDS)
    col_map = [2, 0, 1]  # source columns [0, 1, 2] -> target [2, 0, 1]
    for ctype in range(5):
        for b in src.b[ctype]:
            r = snapshot.remap_columns(ctype, b, col_map)
            assert set(r) == set(b)
            for k in b:
                if ctype in (0, 1) and k == "col":
                    assert r[k].dtype == np.uint16 and r[k].tolist() == [col_map[c] for c in b[k].tolist()]
                elif ctype == 4 and k in ("dots", "vv", "cloud"):
                    assert r[k].dtype == np.uint64
                    assert (r[k] >> np.uint64(48)).tolist() == [col_map[int(c)] for c in (b[k] >> np.uint64(48))]
                    assert (r[k] & np.uint64(2**48 - 1)).tolist() == (b[k] & np.uint64(2**48 - 1)).tolist()
                else:
                    assert np.asarray(r[k]).tobytes() == np.asarray(b[k]).tobytes(), (ctype, k)
    # through load(): remapped, and every UJSON document's dots ascending again
    snapshot.save(src, str(tmp_path))
    tgt = FakeTarget({101: 2, 202: 0, 303: 1})
    snapshot.load(str(tmp_path), tgt)
    got = {t: b for t, b in tgt.got}
    assert got[0]["col"].tolist() == [2, 1, 0] and got[1]["col"].tolist() == [2, 1, 0]
    assert got[0]["val"].tolist() == [7, 2**64 - 1, 9]
    uj = got[4]
    assert uj["dots"].tolist() == [_dot(0, 1), _dot(1, 6), _dot(2, 4)] and uj["elems"].tolist() == [12, 13, 11]
    assert uj["vv"].tolist() == [_dot(1, 6), _dot(2, 4), _dot(0, 3)]
    assert uj["cloud"].tolist() == [_dot(0, 9), _dot(2, 2**48 - 1)]
    _same(src.b[3][0], got[3])


def test_unknown_version_is_rejected(tmp_path):
    from jylis_amd import snapshot
    snapshot.save(FakeSource(IDS), str(tmp_path))
    man = json.load(open(tmp_path / "manifest.json"))
    man["version"] = snapshot.VERSION + 1
    json.dump(man, open(tmp_path / "manifest.json", "w"))
    tgt = FakeTarget({101: 0, 202: 1, 303: 2})
    with pytest.raises(ValueError, match="version"):
        snapshot.load(str(tmp_path), tgt)
    assert not tgt.got


def test_object_arrays_are_rejected(tmp_path):
    from jylis_amd import snapshot
    man = snapshot.save(FakeSource(IDS), str(tmp_path))
    entry = man["chunks"][2]
    b = dict(np.load(tmp_path / entry["file"]))
    b["ts"] = np.array([{"a": 1}, None], dtype=object)
    np.savez(tmp_path / entry["file"], **b)
    tgt = FakeTarget({101: 0, 202: 1, 303: 2})
    with pytest.raises(ValueError):
        snapshot.load(str(tmp_path), tgt)
    assert all(t != 2 for t, _ in tgt.got)
