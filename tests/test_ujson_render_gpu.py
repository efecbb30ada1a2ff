"""UJSON GET as RESP reply bytes, rendered on the GPU (jy_ujson_get_resp,
jylis_amd/csrc/k_uj_render.hip).  Every reply is compared byte for byte with
b"$%d\\r\\n%s\\r\\n" around ujson_doc.render_stored_order of the leaves
DeviceLeaves.under returns for the query, and canonically with
UJSONDocs.get_paths.  The sizes of the sweeps are the code's own constants,
read from the headers."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from jylis_amd import ujson_doc as U
from test_ujson_doc import IDENT_A, IDENT_B, _replay, _session

pytestmark = pytest.mark.gpu
UJSON = 4
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "jylis_amd", "csrc")
EMPTY = b"$0\r\n\r\n"


def _const(header, name):
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, open(os.path.join(CSRC, header)).read())
    assert m, (header, name)
    return int(m.group(1))


BLOCK_KEYS = _const("jy_sort.hpp", "kThreads") * _const("jy_sort.hpp", "kSub")  # jysort::kBlockKeys
STAGE = _const("jy_wire.hpp", "kStage")
TILE_ITEMS = _const("jy_dscan.hpp", "kThreads") * _const("jy_dscan.hpp", "kPer")  # jydscan::kTileItems
MASK_TILE = _const("jy_wire.hpp", "kThreads") * _const("k_uj_render.hip", "kMaskPer")  # the ancestor-mask scan's tile
DEPTH = _const("jy_uj_render.hpp", "kRenderDepth")


def frame(text):
    t = text.encode()
    return b"$%d\r\n%s\r\n" % (len(t), t)


def _docs(eng, ident=IDENT_A):
    from jylis_amd.repo import RepoUJSON
    return U.UJSONDocs(U.GpuDocs(RepoUJSON(eng)), ident, U.DeviceLeaves(eng))


def ins_many(docs, items):
    """INS of (key, path, value text) leaves: one put, one write"""
    eng = docs.b.r.eng
    encs = [U._encode(tuple(p), v) for _, p, v in items]
    offs = np.zeros(len(encs) + 1, np.uint64)
    offs[1:] = np.cumsum([len(e) for e in encs], dtype=np.uint64)
    hs = eng.ujson_leaves_put(np.frombuffer(b"".join(encs), np.uint8), offs)
    assert all(int(h) for h in hs)
    docs.b.write([("INS", k, int(h)) for (k, _, _), h in zip(items, hs)], docs.identity)


def check(docs, keys, paths, flagged=None):
    """the call against the host rule -> the replies UJSONDocs.get_resp returns"""
    eng = docs.b.r.eng
    keys, paths = list(keys), [tuple(p) for p in paths]
    r = eng.ujson_get_resp(keys, paths)
    rb, ro, oh = r["reply_bytes"].tobytes(), [int(x) for x in r["reply_offs"]], [int(x) for x in r["on_host"]]
    assert r["reply_offs"].dtype == np.uint64 and r["on_host"].dtype == np.uint8
    found = docs.leaves.under(docs.b.r.slots_of(keys), paths, leaves=True)
    texts = docs.get_paths(keys, paths)
    want, rendered = [], 0
    assert ro[0] == 0 and ro[-1] == len(rb) == r["sizes"][0]
    for i in range(len(keys)):
        leaves = [leaf for _, leaf in found[i]]
        w = frame(U.render_stored_order(leaves))
        want.append(w)
        got = rb[ro[i]:ro[i + 1]]
        if oh[i]:
            assert got == b"", i
            continue
        assert oh[i] == 0
        assert got == w, (i, keys[i], paths[i], got[:200], w[:200])
        text = got[got.index(b"\r\n") + 2:-2].decode()
        assert U.canonical(text) == U.canonical(texts[i]), (i, text[:200], texts[i][:200])
        rendered += len(set(leaves))
    if flagged is not None:
        assert [i for i in range(len(keys)) if oh[i]] == sorted(flagged)
    sizes = r["sizes"]
    NO = 0xFFFFFFFF
    assert sizes[1] == sum(int(s) != NO for s in docs.b.r.slots_of(keys))
    assert sizes[2] == rendered and sizes[4] == sum(oh) and sizes[5] == 0
    assert sizes[3] == eng.ujson_path_read_caps(docs.b.r.slots_of(keys), paths, False, 0, 0)[0][2]
    whole = docs.get_resp(keys, paths)
    assert whole == want  # the same whichever side rendered
    return whole


# ---- the docs' session -------------------------------------------------------------

def test_docs_session(engine):
    """the reference's UJSON docs session (tests/golden/kat_docs.json): every GET
    canonically equals what the doc shows"""
    dev = _docs(engine)
    paths = [(), ("created_at",), ("contact",), ("contact", "email"), ("roles",), ("nothing",)]
    gets = 0
    for st in _session():
        if st[0] != "GET":
            _replay(dev, [st])
            keys = [st[1]] * len(paths) + ["no-such-key"]
            check(dev, keys, paths + [()])
            continue
        got = check(dev, [st[1]], [tuple(st[2])])[0]
        text = got[got.index(b"\r\n") + 2:-2].decode()
        assert U.canonical(text) == U.canonical(st[3]), (st, text)
        gets += 1
    assert gets >= 4


def test_docs_roles(engine):
    gold = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "kat_docs.json")))["ujson_doc_roles"]
    dev = _docs(engine)
    for v in ('"user"', '"vendor"', '"admin"'):
        dev.ins("users:my-user", ("roles",), v)
    dev.rm("users:my-user", ("roles",), '"vendor"')
    assert len(gold["expect_elements"]) == 2
    assert check(dev, ["users:my-user"], [()]) == [frame('{"roles":["admin","user"]}')]
    assert check(dev, ["users:my-user"], [("roles",)]) == [frame('["admin","user"]')]
    dev.clr("users:my-user")
    assert check(dev, ["users:my-user"], [()]) == [EMPTY]


# ---- order edges -------------------------------------------------------------------

def test_order_edges(engine):
    from jylis_amd.engine import Engine
    from jylis_amd.repo import RepoUJSON
    dev = _docs(engine)
    items = []
    # keys equal through 8, 16, 24 bytes and beyond (40, 200), differing in the last byte;
    # in reverse, so that insertion order is not the answer
    for n in (8, 16, 24, 40, 200):
        for last in "zma":
            items.append(("eq", ("p" * n + last,), str(n)))
            items.append(("eq", ("top", "p" * n + last, "x"), '"%s"' % last))
    # key lengths 1, 255 and 256 at one node (the little-endian length word sorts 256 first)
    for k in ("z", "k" * 255, "q" * 256, "ab"):
        items.append(("lens", (k,), "1"))
        items.append(("lens", ("in", k), "2"))
    # a leaf that is a prefix of the next
    for v in ("1", "12", "123", '"1"', '"12"'):
        items += [("pre", (), v), ("pre", ("a",), v), ("pre", ("a", "b"), v)]
    ins_many(dev, items)
    # the same leaf under two dots: the same INS on a second replica, converged
    engB = Engine(device=0)
    try:
        other = U.UJSONDocs(U.GpuDocs(RepoUJSON(engB)), IDENT_B, U.DeviceLeaves(engB))
        other.ins("pre", ("a",), "12")
        other.ins("pre", (), "1")
        dev.b.r.converge_deltas(other.b.r.flush_deltas())
    finally:
        engB.close()
    slot = dev.b.r.slots_of(["pre"])
    sizes, eo, el, _, _ = engine.ujson_path_read(slot, [("a",)], leaves=False)
    assert el.tolist().count(dev.leaves.handle(("a",), "12")) == 2  # path_read shows it twice
    got = check(dev, ["eq", "eq", "lens", "lens", "pre", "pre", "pre"],
                [(), ("top",), (), ("in",), (), ("a",), ("a", "b")])
    assert got[3] == frame('{"%s":2,"z":2,"ab":2,"%s":2}' % ("q" * 256, "k" * 255))
    assert got[5] == frame('[{"b":["1","12",1,12,123]},"1","12",1,12,123]')  # ... rendered once
    assert got[6] == frame('["1","12",1,12,123]')
    assert got[0].index(b'"ppppppppa"') < got[0].index(b'"ppppppppm"') < got[0].index(b'"ppppppppz"')


# ---- structure ---------------------------------------------------------------------

SHAPES = {
    "bare": ([((), "1")], "1"),
    "set": ([((), "2"), ((), "1"), ((), "12")], "[1,12,2]"),
    "map": ([(("b",), "2"), (("a",), "1")], '{"a":1,"b":2}'),
    "map+values": ([((), "2"), (("k",), "1")], '[{"k":1},2]'),
    "deep": ([(("a", "b", "c"), "1")], '{"a":{"b":{"c":1}}}'),
    "all": ([(("a", "b", "c"), "1"), (("a", "b"), "2"), (("a",), "3"), ((), "4")], '[{"a":[{"b":[{"c":1},2]},3]},4]'),
    "one map": ([(("a",), "1"), (("b",), "2"), ((), "3"), ((), "4")], '[{"a":1,"b":2},3,4]'),
}


def test_structure(engine):
    dev = _docs(engine)
    ins_many(dev, [(name, p, v) for name, (leaves, _) in SHAPES.items() for p, v in leaves])
    dev.set("void", (), "{}")  # an empty document
    names = list(SHAPES)
    got = check(dev, names, [()] * len(names))
    assert got == [frame(SHAPES[k][1]) for k in names]
    # a path equal to a leaf's whole path: a bare value; under a node; matching nothing
    got = check(dev, ["deep", "all", "all", "all", "map"], [("a", "b", "c"), ("a", "b"), ("a",), ("a", "b", "c"), ("c",)])
    assert got == [frame("1"), frame('[{"c":1},2]'), frame('[{"b":[{"c":1},2]},3]'), frame("1"), EMPTY]
    # no match, a missing key and an empty document, each at the first, middle and last query
    voids = [("map", ("zz",)), ("nobody", ()), ("void", ())]
    for key, path in voids:
        for at in (0, 2, 4):
            qs = [("all", ()), ("set", ()), ("map+values", ()), ("deep", ("a",))]
            qs.insert(at, (key, path))
            got = check(dev, [k for k, _ in qs], [p for _, p in qs])
            assert got[at] == EMPTY and EMPTY not in got[:at] + got[at + 1:]
    got = check(dev, [k for k, _ in voids], [p for _, p in voids])
    assert got == [EMPTY] * 3
    # the same key in several queries with different paths
    got = check(dev, ["all"] * 5, [(), ("a",), ("a", "b"), ("a", "b", "c"), ("b",)])
    assert len(set(got)) == 5 and got[4] == EMPTY
    # paths=None: the whole documents
    r = engine.ujson_get_resp(names)
    assert r["reply_bytes"].tobytes() == b"".join(frame(SHAPES[k][1]) for k in names)


# ---- size sweeps -------------------------------------------------------------------

SWEEP = sorted({1, 2, 63, 64, 65} | {c + d for c in (BLOCK_KEYS, STAGE, TILE_ITEMS, MASK_TILE, 256) for d in (-1, 0, 1)})


def _flat(n):
    return [((), '"v%05d"' % (i * 7919 % n)) for i in range(n)] if n % 2 else \
        [(("k%05d" % (i * 7919 % n),), str(i)) for i in range(n)]


def _nested(n):
    out = []
    for i in range(n):
        j = i * 7919 % n
        out.append((("t%d" % (j % 5), "m%d" % (j % 11), "k%d" % j)[:1 + j % 3] + (("leaf%d" % j,) if j % 4 else ()), str(j)))
    return out


def test_size_sweep(engine):
    """one flat and one nested document of L leaves, for L around every tile,
    staging and block edge (the documents' own keys, one query each, and all of
    them in one call)"""
    assert {BLOCK_KEYS, STAGE, TILE_ITEMS} <= set(SWEEP) and (BLOCK_KEYS, STAGE, TILE_ITEMS) == (1024, 1024, 2048)
    dev = _docs(engine)
    items = []
    for n in SWEEP:
        items += [("flat%d" % n, p, v) for p, v in _flat(n)] + [("nest%d" % n, p, v) for p, v in _nested(n)]
    ins_many(dev, items)
    keys = [k % n for n in SWEEP for k in ("flat%d", "nest%d")]
    for k in keys:
        check(dev, [k], [()])
    check(dev, keys + ["nest%d" % TILE_ITEMS] * 2, [()] * len(keys) + [("t1",), ("t2", "m3")])


def test_many_queries(engine):
    """kTileItems + 1 queries of one to three leaves: query boundaries straddle
    every tile and staging edge, and the mask's reset runs at every position"""
    dev = _docs(engine)
    n = TILE_ITEMS + 1
    items = []
    for i in range(n):
        k = "q%04d" % i
        items.append((k, ("a",) * (i % 3), str(i)))
        if i % 3 > 0:
            items.append((k, ("a", "b")[:i % 2 + 1], '"s%d"' % i))
        if i % 3 > 1:
            items.append((k, (), "null"))
    ins_many(dev, items)
    keys = ["q%04d" % (i * 5 % n) for i in range(n)]
    got = check(dev, keys, [()] * n)
    assert len(set(got)) == n


# ---- limits ------------------------------------------------------------------------

def test_limits(engine):
    dev = _docs(engine)
    deep = lambda d: tuple("s%d" % (i % 2) for i in range(d))
    items = [("d%d" % d, deep(d), "1") for d in (DEPTH - 1, DEPTH, DEPTH + 1)]
    items += [("d%d" % d, deep(d)[:3], "2") for d in (DEPTH - 1, DEPTH, DEPTH + 1)]
    bad = {"k1f": "a\x1fb", "kq": 'a"b', "kbs": "a\\b", "knul": "\x00"}
    good = {"k20": "a b", "k7f": "a\x7fb", "kutf": "añb→", "klong": "x" * 300}
    for name, k in list(bad.items()) + list(good.items()):
        items += [(name, ("top", k, "z"), "1"), (name, ("other",), "2"), (name, (), "3")]
    ins_many(dev, items)
    keys = ["d%d" % (DEPTH - 1), "d%d" % DEPTH, "d%d" % (DEPTH + 1)]
    check(dev, keys, [()] * 3, flagged=[2])
    # the depth is the RELATIVE depth: one segment down, the deepest leaf renders
    check(dev, keys, [("s0",)] * 3, flagged=[])
    check(dev, ["d%d" % (DEPTH + 1)] * 2, [("s0", "s1"), ("s1",)], flagged=[])
    names = list(bad) + list(good)
    got = check(dev, names, [()] * len(names), flagged=range(len(bad)))
    assert got[len(bad)] == frame('[{"top":{"a b":{"z":1}},"other":2},3]')
    # a path that leaves the bad key above it renders; flagged queries between rendered ones
    mixed = ["k20", "k1f", "kq", "k7f", "kbs", "kq", "kutf"]
    paths = [(), (), ("other",), (), ("top",), ("top", 'a"b'), ("top",)]
    got = check(dev, mixed, paths, flagged=[1, 4])
    assert got[2] == frame("2") and got[5] == frame('{"z":1}')
    assert got[1] == frame(U.render_stored_order([(("top", "a\x1fb", "z"), "1"), (("other",), "2"), ((), "3")]))


# ---- contract ----------------------------------------------------------------------

def _contract_docs(engine):
    dev = _docs(engine)
    dev.set("d1", (), json.dumps({"alpha": {"k%d" % i: i for i in range(40)}, "b": ["x", "y", {"c": None}]}))
    dev.set("d2", (), json.dumps({"b": {"k": [1, 2, 3]}, "z": "text"}))
    return dev, ["d1", "d2", "nobody", "d1"], [("alpha",), (), (), ("b",)]


def test_two_phase(engine):
    dev, keys, paths = _contract_docs(engine)
    want = check(dev, keys, paths)
    total = sum(map(len, want))
    fresh = lambda: {"reply_bytes": np.full(total + 8, 0xCD, np.uint8), "reply_offs": np.full(6, 0xCDCD, np.uint64),
                     "on_host": np.full(5, 0xCD, np.uint8)}
    untouched = lambda o: all((a == (0xCD if a.dtype == np.uint8 else 0xCDCD)).all() for a in o.values())
    need = None
    for cap in (0, total - 1):
        out = fresh()
        sizes, _ = engine.ujson_get_resp_caps(keys, paths, cap, out=out)
        assert sizes[0] == total and sizes[1] == 3 and sizes[4] == 0 and untouched(out), cap
        need = sizes
    out = fresh()
    sizes, _ = engine.ujson_get_resp_caps(keys, paths, total, out=out)  # the exact capacity
    assert sizes == need
    assert out["reply_bytes"][:total].tobytes() == b"".join(want) and (out["reply_bytes"][total:] == 0xCD).all()
    assert out["reply_offs"][:5].tolist() == np.cumsum([0] + [len(w) for w in want]).tolist()
    assert out["reply_offs"][5] == 0xCDCD and out["on_host"].tolist() == [0, 0, 0, 0, 0xCD]
    # n == 0 writes the single offset 0
    r = engine.ujson_get_resp([], [])
    assert r["reply_offs"].tolist() == [0] and len(r["reply_bytes"]) == 0 and r["sizes"] == [0] * 6


@pytest.mark.parametrize("off", [0, 1, 3, 7])
def test_device_outputs_and_keys(engine, off):
    import torch
    dev, keys, paths = _contract_docs(engine)
    want = check(dev, keys, paths)
    total = sum(map(len, want))
    d = "cuda:0"
    buf = torch.full((total + 16,), 0xAB, dtype=torch.uint8, device=d)
    assert buf.data_ptr() % 8 == 0
    out = {"reply_bytes": buf[off:], "reply_offs": torch.empty(5, dtype=torch.int64, device=d),
           "on_host": torch.full((4,), 9, dtype=torch.uint8, device=d)}
    # device keys behave as host keys
    kb = b"".join(k.encode() for k in keys)
    ko = np.cumsum([0] + [len(k) for k in keys])
    dkeys = (torch.tensor(list(kb), dtype=torch.uint8, device=d), torch.tensor(ko, dtype=torch.int64, device=d))
    need, _ = engine.ujson_get_resp_caps(dkeys, paths, 0, device=True)
    sizes, _ = engine.ujson_get_resp_caps(dkeys, paths, total, device=True, out=out)
    engine.sync()
    assert sizes == need and sizes[0] == total
    raw = buf.cpu().numpy()
    assert raw[off:off + total].tobytes() == b"".join(want)
    assert (raw[:off] == 0xAB).all() and (raw[off + total:] == 0xAB).all()  # nothing outside the output
    assert out["reply_offs"].cpu().numpy().tolist() == np.cumsum([0] + [len(w) for w in want]).tolist()
    assert out["on_host"].cpu().numpy().tolist() == [0] * 4
    r = engine.ujson_get_resp(keys, paths, device=True)
    engine.sync()
    assert r["reply_bytes"].is_cuda and r["reply_bytes"].cpu().numpy().tobytes() == b"".join(want)


def _raw(eng, keys, pb, po):
    kb = np.frombuffer(b"".join(keys) or b"\0", np.uint8)
    ko = np.cumsum([0] + [len(k) for k in keys]).astype(np.uint64)
    pb = np.frombuffer(bytes(pb) or b"\0", np.uint8)
    po = np.asarray(po, np.uint64)
    ro = np.full(len(keys) + 1, 0xCDCD, np.uint64)
    oh = np.full(len(keys), 0xCD, np.uint8)
    sizes = (C.c_uint64 * 6)(*([7] * 6))
    rc = eng.lib.jy_ujson_get_resp(eng.h, len(keys), kb.ctypes.data, ko.ctypes.data, 0, pb.ctypes.data, po.ctypes.data,
                                   0, None, ro.ctypes.data, oh.ctypes.data, sizes, 0)
    return rc, [int(x) for x in sizes], ro, oh


def test_host_validation(engine):
    """malformed paths return the path read's codes and write nothing"""
    from jylis_amd._lib import JY_EINVAL, JY_ERANGE, JY_OK
    dev, keys, paths = _contract_docs(engine)
    k2 = [b"d1", b"d2"]
    a, b = U.encode_path(("alpha",)), U.encode_path(("b",))
    good = (k2, a + b, [0, len(a), len(a) + len(b)])
    cut = U.encode_path(("alpha", "beta"))[:-2]
    bad = [
        ((k2, a + b, [0, len(a) + len(b), len(a)]), JY_EINVAL, "ascending"),
        ((k2, a + cut, [0, len(a), len(a) + len(cut)]), JY_EINVAL, "cut short"),
        ((k2, a + b"\x02\x00", [0, len(a), len(a) + 2]), JY_EINVAL, "length word"),
        ((k2, a + b"\xff\xff\xff\xff", [0, len(a), len(a) + 4]), JY_ERANGE, "2^24"),
    ]
    skipped = engine.skipped()
    for args, code, word in bad:
        rc, sizes, ro, oh = _raw(engine, *args)
        assert rc == code and sizes == [0] * 6 and (ro == 0xCDCD).all() and (oh == 0xCD).all(), (word, rc, sizes)
        assert word in engine.lib.jy_last_error(engine.h).decode()
        rc, sizes, ro, oh = _raw(engine, *good)
        assert rc == JY_OK and sizes[0] > 0 and sizes[1] == 2 and (ro == 0xCDCD).all()  # sizes only
    assert engine.skipped() == skipped
    check(dev, keys, paths)


def test_read_only(engine):
    dev, keys, paths = _contract_docs(engine)
    dev.ins("d2", ("b", "more"), '"text"')  # a pending delta
    wire = lambda a: {k: np.asarray(v).tobytes() for k, v in a.items()} if isinstance(a, dict) else a
    before = (engine.digest(UJSON, 4).tolist(), engine.ujson_leaves_usage(), engine.ujson_deltas_size(),
              wire(engine.state_wire(UJSON, 0, engine.nkeys(UJSON))))
    for _ in range(2):
        check(dev, keys, paths)
    after = (engine.digest(UJSON, 4).tolist(), engine.ujson_leaves_usage(), engine.ujson_deltas_size(),
             wire(engine.state_wire(UJSON, 0, engine.nkeys(UJSON))))
    assert before == after
    # the pending batch is what it would have been: flushed after the reads on this
    # engine, and without any read on a twin
    from jylis_amd.engine import Engine
    twin_eng = Engine(device=0)
    try:
        twin, _, _ = _contract_docs(twin_eng)
        twin.ins("d2", ("b", "more"), '"text"')
        assert wire(engine.flush_wire(UJSON)) == wire(twin_eng.flush_wire(UJSON))
    finally:
        twin_eng.close()


# ---- the node ----------------------------------------------------------------------

def test_node_agrees_with_one_engine(engine):
    from jylis_amd.node import Node
    from jylis_amd.repo import RepoUJSON
    one = _docs(engine)
    node = Node(2, "copy")
    try:
        shards = [U.UJSONDocs(U.GpuDocs(RepoUJSON(node.engine(s))), IDENT_A,
                              U.DeviceLeaves(node.engine(s), lock=lambda: node.locked(UJSON))) for s in (0, 1)]
        keys = ["doc%d" % i for i in range(24)]
        assert {node.shard_of(k.encode()) for k in keys} == {0, 1}
        for i, k in enumerate(keys):
            items = [(k, ("a", "k%d" % j)[:1 + j % 2], str(i * j)) for j in range(1 + i % 5)] + [(k, (), '"%s"' % k)]
            items += [(k, ('q"',), "1")] if i % 7 == 3 else []
            ins_many(one, items)
            with node.locked(UJSON):
                ins_many(shards[node.shard_of(k.encode())], items)
        q = [keys[i * 5 % 24] for i in range(40)] + ["nobody"]
        paths = [((), ("a",), ("a", "k1"))[i % 3] for i in range(len(q))]
        want = engine.ujson_get_resp(q, paths)
        rb, ro, oh = node.get_resp(UJSON, q, paths=paths)
        assert rb == want["reply_bytes"].tobytes() and ro.tolist() == want["reply_offs"].tolist()
        assert oh.tolist() == want["on_host"].tolist() and 0 < sum(oh.tolist()) < len(q)
        check(one, q, paths)
    finally:
        node.close()
