"""The UJSON leaf store's host-side pieces, without a GPU: the four calls are
declared alike in the header, the ctypes table and the Pony FFI; the header
states the handle formula and the lock rule; jy_leaf.hpp's hash and length
guard, compiled into a stand-alone host program, agree with ujson_doc; the
numpy restatement of "a batch with leaves"; snapshot files that carry leaves."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import leaves_ref as R
from jylis_amd import ujson_doc as U
from test_pony_glue import header_arity, pony_decls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_CALLS = ["jy_ujson_leaves_put", "jy_ujson_leaves_get", "jy_ujson_leaves_reserve", "jy_ujson_leaves_usage"]

LEAVES = [((), ""), ((), "1"), (("a",), '"x"'), (("a", "b"), "true"), (("ключ", "é"), '"日本語"'), (("",), "null"),
          (("a" * 300, "b"), '"' + "z" * 1000 + '"'), (("k",) * 20, "3.5")]


def test_the_four_calls_are_declared_alike():
    from jylis_amd import _lib
    hdr, pony = header_arity(), pony_decls()
    for name in NEW_CALLS:
        assert name in hdr and name in pony and name in _lib.SIGNATURES, name
        assert hdr[name] == pony[name] == len(_lib.SIGNATURES[name][1]), name
        assert _lib.SIGNATURES[name][0] is _lib.I32
    assert hdr["jy_ujson_leaves_put"] == 6 and hdr["jy_ujson_leaves_get"] == 9


def test_the_header_states_the_handle_formula_and_the_lock_rule():
    text = " ".join(open(os.path.join(ROOT, "include", "jylis_gpu.h")).read().split()).replace(" * ", " ")
    assert "handle = FNV-1a 64 over the encoding, a result of 0 replaced by 1" in text
    assert "each path segment as a 4-byte little-endian length plus its bytes, then FF FF FF FF, then the value text" in text
    assert "jy_node_lock_type(node, JY_UJSON), NEVER under JY_NODE_NOFENCE" in text
    assert "leaf_bytes / leaf_offs[nel + 1], parallel to `elems`" in text
    own = " ".join(open(os.path.join(ROOT, "jylis_amd", "csrc", "jy_leaf.hpp")).read().split()).replace(" // ", " ")
    assert "handle = FNV-1a 64 over that encoding, a result of 0 replaced by 1" in own
    assert "APPEND-ONLY" in own


def _host_compiler():
    for cc in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/bin/amdclang++"):
        path = shutil.which(cc)
        if path:
            return path
    raise RuntimeError("no host C++ compiler found")


def test_host_check_program(tmp_path):
    """tools/leaf_host_check.cpp, built with the host compiler (no sanitizer):
    jy_leaf.hpp's hash against handles computed by ujson_doc, and its length
    guard on a decreasing pair, a length of 3 and a length of 2^24"""
    exe = str(tmp_path / "leaf_host_check")
    subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-Wall", "-o", exe,
                    os.path.join(ROOT, "tools", "leaf_host_check.cpp")], check=True)
    table = U.LeafTable()
    rng = np.random.default_rng(5)
    lines = []
    for path, value in LEAVES + [R.leaf_of_length(n) for n in (4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65)] + \
            [((), "".join(chr(int(c)) for c in rng.integers(32, 0x2FF, int(n)))) for n in rng.integers(0, 40, 24)]:
        enc = U._encode(path, value)
        assert table.handle(path, value) == R.handle_of(enc) and U._decode(enc) == (tuple(path), value)
        lines.append(f"{enc.hex()} {R.handle_of(enc):x}")
    good = tmp_path / "pairs.txt"
    good.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(good)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == f"ok {len(lines)}", out.stdout + out.stderr
    # the program does compare: one wrong handle fails it
    wrong = tmp_path / "wrong.txt"
    wrong.write_text(lines[0] + "\n" + lines[1].split()[0] + " 1234\n")
    out = subprocess.run([exe, str(wrong)], capture_output=True, text=True)
    assert out.returncode == 1 and "pair 1" in out.stdout, out.stdout


def test_the_restatement_of_a_batch_with_leaves():
    encs = [U._encode(p, v) for p, v in LEAVES[:4]]
    table = {R.handle_of(e): e for e in encs}
    hs = [R.handle_of(e) for e in encs]
    elems = np.array([hs[2], hs[0], 0xDEAD, hs[2], 0, hs[3]], np.uint64)  # a repeat, an unknown handle, handle 0
    lb, lo = R.batch_leaves(elems, table)
    assert lb.dtype == np.uint8 and lo.dtype == np.uint64 and len(lo) == len(elems) + 1 and lo[0] == 0
    assert R.unpack(lb, lo) == [encs[2], encs[0], b"", encs[2], b"", encs[3]]
    assert int(lo[-1]) == len(lb) == 2 * len(encs[2]) + len(encs[0]) + len(encs[3])
    lb, lo = R.batch_leaves(np.zeros(0, np.uint64), table)
    assert len(lb) == 0 and lo.tolist() == [0]


def test_permute_items_moves_and_selects():
    from jylis_amd.snapshot import permute_items
    items = [b"abcd", b"", b"efghijk", b"l", b"mnopqrstu"]
    lb, lo = R.pack(items)
    for order in ([4, 3, 2, 1, 0], [2, 0], [1], [], [3, 3, 0]):
        b, o = permute_items(lb, lo, np.array(order, np.int64))
        assert b.dtype == np.uint8 and o.dtype == np.uint64 and R.unpack(b, o) == [items[i] for i in order]


# ---- snapshot files ----------------------------------------------------------

IDS = [0x1111, 0x2222, 0x3333]


def _chunk(leaves):
    """a hand-built UJSON chunk of two documents: 'a' holds three elements
    (columns 2, 0, 1 in dot order 0, 1, 2), 'bb' one"""
    from jylis_amd.engine import DOT_SEQ_BITS
    encs = [U._encode(p, v) for p, v in LEAVES[:4]]
    dot = lambda c, n: (c << DOT_SEQ_BITS) | n
    w = {"key_bytes": np.frombuffer(b"abb", np.uint8), "key_offs": np.array([0, 1, 3], np.uint64),
         "el_offs": np.array([0, 3, 4], np.uint64),
         "dots": np.array([dot(0, 5), dot(1, 2), dot(2, 9), dot(1, 1)], np.uint64),
         "elems": np.array([R.handle_of(e) for e in encs], np.uint64),
         "vv_offs": np.array([0, 2, 2], np.uint64), "vv": np.array([dot(0, 5), dot(2, 9)], np.uint64),
         "cloud_offs": np.array([0, 0, 1], np.uint64), "cloud": np.array([dot(1, 1)], np.uint64)}
    if leaves:
        w["leaf_bytes"], w["leaf_offs"] = R.pack(encs)
    return w


class _Source:
    def __init__(self):
        self.asked = []

    def replica_count(self):
        return len(IDS)

    def replica_id(self, c):
        return IDS[c]

    def snapshot(self, ctype, max_keys=65536, **kw):
        self.asked.append((ctype, kw))
        if ctype == 4:
            yield _chunk(kw.get("leaves", False))


class _Target:
    def __init__(self, ids):
        self.ids, self.got = list(ids), []

    def replica_col(self, rid):
        return self.ids.index(rid)

    def converge_wire(self, ctype, w):
        self.got.append((ctype, w))


def test_snapshot_files_carry_the_leaves(tmp_path):
    from jylis_amd import snapshot
    from jylis_amd.engine import WIRE_ARRAYS, WIRE_OPTIONAL
    src = _Source()
    m = snapshot.save(src, str(tmp_path / "with"), leaves=True)
    assert m["ujson_leaves"] is True and m["version"] == 1
    assert (4, {"leaves": True}) in src.asked and (2, {}) in src.asked  # only UJSON is asked for leaves
    entry, = m["chunks"]
    with np.load(str(tmp_path / "with" / entry["file"]), allow_pickle=False) as z:
        want = _chunk(True)
        assert sorted(z.files) == sorted(want)
        for name, dt in [(n, d) for n, d, _, _ in WIRE_ARRAYS[4]] + list(WIRE_OPTIONAL[4]):
            assert z[name].dtype == np.dtype(dt) and z[name].tolist() == want[name].tolist(), name
    assert entry["sizes"]["leaf_offs"] == 5 and entry["sizes"]["leaf_bytes"] == len(_chunk(True)["leaf_bytes"])
    # the same columns on the target: the chunk arrives as written
    tgt = _Target(IDS)
    snapshot.load(str(tmp_path / "with"), tgt)
    (ctype, got), = tgt.got
    assert ctype == 4 and sorted(got) == sorted(want)
    for name in want:
        assert np.asarray(got[name]).tolist() == want[name].tolist(), name
    # other columns: the dots are remapped and re-sorted, and every leaf moves with its element
    tgt = _Target([IDS[2], IDS[1], IDS[0]])
    snapshot.load(str(tmp_path / "with"), tgt)
    (_, got), = tgt.got
    assert got["elems"].tolist() != want["elems"].tolist() and sorted(got["elems"].tolist()) == sorted(want["elems"].tolist())
    assert [R.handle_of(b) for b in R.unpack(got["leaf_bytes"], got["leaf_offs"])] == got["elems"].tolist()
    assert got["el_offs"].tolist() == want["el_offs"].tolist()


def test_snapshot_files_without_the_flag_are_unchanged(tmp_path):
    from jylis_amd import snapshot
    from jylis_amd.engine import WIRE_ARRAYS
    src = _Source()
    m = snapshot.save(src, str(tmp_path / "plain"))
    assert "ujson_leaves" not in m and all(kw == {} for _, kw in src.asked)
    assert sorted(m) == ["chunks", "format", "replica_ids", "types", "version"]
    entry, = m["chunks"]
    with np.load(str(tmp_path / "plain" / entry["file"]), allow_pickle=False) as z:
        assert sorted(z.files) == sorted(name for name, _, _, _ in WIRE_ARRAYS[4])
    # a version-1 manifest without the flag loads, and its chunks carry no leaves
    assert json.load(open(str(tmp_path / "plain" / "manifest.json")))["version"] == 1
    tgt = _Target(IDS)
    snapshot.load(str(tmp_path / "plain"), tgt)
    (_, got), = tgt.got
    assert "leaf_bytes" not in got and "leaf_offs" not in got
    # one leaf array without the other is no wire batch
    bad = dict(_chunk(True))
    del bad["leaf_offs"]
    np.savez(str(tmp_path / "plain" / entry["file"]), **bad)
    with pytest.raises(ValueError):
        snapshot.load(str(tmp_path / "plain"), _Target(IDS))
