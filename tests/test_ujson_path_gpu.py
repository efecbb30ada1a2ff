"""UJSON path reads on the GPU (jy_ujson_path_read, jylis_amd/csrc/k_uj_path.hip)
against a Python restatement made of the reads they replace: ujson_read of the
same slots, ujson_leaves_get of the handles, _decode, a tuple-prefix filter and
the relative leaf re-encoded.  Every comparison is exact: el_offs, elems (order
included), leaf_offs, leaf_bytes, sizes."""
import ctypes as C
import json

import numpy as np
import pytest

import leaves_ref as R
from jylis_amd import ujson_doc as U
from test_ujson_doc import IDENT_A, IDENT_B, OracleDocs, _replay, _session

pytestmark = pytest.mark.gpu
UJSON = 4
NO = 0xFFFFFFFF
# encoded path lengths 0, 5, 7, 8, 9, 12, 16, 17: the word loop's tails
LEN_PATHS = [(), ("a",), ("abc",), ("abcd",), ("abcde",), ("abcdefgh",), ("a", "bcdefgh"), ("abcdefghijklm",)]


def restate(eng, slots, paths, leaves=True):
    """what jy_ujson_path_read returns, from the reads it replaces"""
    slots = [int(s) for s in slots]
    live = sorted({s for s in slots if s != NO})
    per = {}
    if live:
        eo, _, elems, _, _, _ = eng.ujson_read(np.array(live, np.uint32))
        encs = R.unpack(*eng.ujson_leaves_get(elems))
        per = {s: [(int(elems[j]), encs[j]) for j in range(int(eo[i]), int(eo[i + 1]))] for i, s in enumerate(live)}
    el_offs, el, items, examined, missing = [0], [], [], 0, 0
    for s, p in zip(slots, paths):
        for h, enc in per.get(s, []):
            examined += 1
            if not enc:
                missing += 1
                continue
            q, v = U._decode(enc)
            if q[:len(p)] == tuple(p):
                el.append(h)
                items.append(U._encode(q[len(p):], v))
        el_offs.append(len(el))
    lb, lo = R.pack(items)
    return [len(el), len(lb) if leaves else 0, examined, missing], el_offs, el, lb.tolist(), lo.tolist()


def check(eng, slots, paths):
    """the call against the restatement, with and without the leaves -> the restatement"""
    slots = np.asarray(slots, np.uint32)
    for leaves in (True, False):
        want = restate(eng, slots, paths, leaves)
        sizes, eo, el, lb, lo = eng.ujson_path_read(slots, paths, leaves)
        assert sizes == want[0], (sizes, want[0])
        assert eo.dtype == np.uint64 and eo.tolist() == want[1]
        assert el.dtype == np.uint64 and el.tolist() == want[2]
        if leaves:
            assert lo.dtype == np.uint64 and lo.tolist() == want[4]
            assert lb.dtype == np.uint8 and lb.tolist() == want[3]
        else:
            assert lb is None and lo is None
    return restate(eng, slots, paths, True)


class HostFiltered:
    """a DeviceLeaves without `under`: UJSONDocs over it reads elements + leaves
    and filters on the host, as before the device path"""

    def __init__(self, dl):
        self.handle, self.leaves, self.leaf = dl.handle, dl.leaves, dl.leaf


def _docs(eng, ident=IDENT_A):
    from jylis_amd.repo import RepoUJSON
    repo = RepoUJSON(eng)
    dl = U.DeviceLeaves(eng)
    return U.UJSONDocs(U.GpuDocs(repo), ident, dl), U.UJSONDocs(U.GpuDocs(repo), ident, HostFiltered(dl))


def _canon(texts):
    return [U.canonical(t) for t in texts]


def _same_renders(dev, old, keys, paths, pool=None):
    """get_many at each of `paths` and one get_paths with a path of `pool` per key"""
    pool = pool or paths
    assert dev._device_paths() and not old._device_paths()
    for q in paths:
        got = dev.get_many(keys, q)
        assert _canon(got) == _canon(old.get_many(keys, q)), q
        assert got == [dev.get(k, q) for k in keys[:2]] + got[2:]
    mixed = [pool[(i + len(keys[0])) % len(pool)] for i in range(len(keys))]
    got = dev.get_paths(keys, mixed)
    assert _canon(got) == _canon([old.get_many([k], p)[0] for k, p in zip(keys, mixed)])
    return got


def test_docs_session(oracle_mod, engine):
    """the reference's docs session through the device path: every GET renders
    what the doc shows, what the host-filtered path renders, and the raw call
    equals the restatement after every step"""
    O = oracle_mod
    dev, old = _docs(engine)
    want_repo = O.Repo(O.UJSON, IDENT_A)
    want = U.UJSONDocs(OracleDocs(want_repo), IDENT_A, U.LeafTable())
    keys = sorted({st[1] for st in _session()}) + ["no-such-key"]
    paths = [(), ("a",), ("contact",), ("contact", "email")]
    for st in _session():
        _replay(dev, [st])
        _replay(want, [st])
        if st[0] == "GET":
            continue
        _same_renders(dev, old, keys, paths)
        slots = dev.b.r.slots_of(keys)
        for q in paths:
            assert _canon(dev.get_many(keys, q)) == _canon(want.get_many(keys, q))
            check(engine, slots, [q] * len(keys))
        from helpers import assert_state_equal
        assert_state_equal(O.UJSON, want_repo.state(), dev.b.r.state())


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_path_histories(oracle_mod, engine, seed):
    """the seeded path-command histories of test_path_commands_gpu_vs_oracle,
    written through the device _under (path-scoped CLR and SET): after every
    step the renders of both paths and the oracle's agree, and the state read
    back with ujson_read equals the oracle's"""
    from helpers import assert_state_equal
    O = oracle_mod
    rng = np.random.default_rng(500 + seed)
    dev, old = _docs(engine)
    want_repo = O.Repo(O.UJSON, IDENT_A)
    want = U.UJSONDocs(OracleDocs(want_repo), IDENT_A, U.LeafTable())
    keys = [f"u{i}" for i in range(5)]
    paths = [(), ("a",), ("a", "b"), ("c",), ("a", "c")]
    vals = ['"x"', '"y"', "1", "true", "null", '{"p":1}', '{"p":[1,2],"q":"z"}', "[3,4]"]
    for step in range(60):
        k = keys[int(rng.integers(0, len(keys)))]
        p = paths[int(rng.integers(0, len(paths)))]
        x = rng.random()
        v = vals[int(rng.integers(0, len(vals)))]
        for d in (want, dev):
            if x < 0.35:
                if not v.startswith(("{", "[")):
                    d.ins(k, p, v)
            elif x < 0.55:
                if not v.startswith(("{", "[")):
                    d.rm(k, p, v)
            elif x < 0.75:
                d.set(k, p, v)
            else:
                d.clr(k, p)
        q = paths[step % len(paths)]
        got = _same_renders(dev, old, keys, [q], paths)
        mixed = [paths[(i + len(keys[0])) % len(paths)] for i in range(len(keys))]
        assert _canon(got) == _canon([want.get(kk, pp) for kk, pp in zip(keys, mixed)])
        assert _canon(dev.get_many(keys, q)) == _canon(want.get_many(keys, q))
        assert_state_equal(O.UJSON, want_repo.state(), dev.b.r.state())
        if step % 6 == 5:
            slots = dev.b.r.slots_of(keys + ["absent"])
            for qq in paths:
                check(engine, slots, [qq] * len(slots))


# ---- path lengths and near misses -------------------------------------------------

def _ins(docs, key, leaves):
    """INS of (path, value text) leaves -> their handles"""
    hs = [docs.leaves.handle(p, v) for p, v in leaves]
    docs.b.write([("INS", key, h) for h in hs], docs.identity)
    return hs


def test_path_lengths_and_near_misses(engine):
    dev, _ = _docs(engine)
    assert [len(U.encode_path(p)) for p in LEN_PATHS] == [0, 5, 7, 8, 9, 12, 16, 17]
    leaves = []
    for p in LEN_PATHS:  # a leaf at each path, one below it, one beside it
        leaves += [(p, "1"), (p + ("z",), '"deep"'), (p[:-1] + ((p[-1] if p else "") + "x",), "2")]
    leaves += [((), ""), (("abc", "d"), "3"), (("ab", "x"), "4"), (("abcdefghijklm", "n", "o"), "true")]
    leaves = sorted(set(leaves))
    hs = _ins(dev, "doc", leaves)
    by_handle = dict(zip(hs, leaves))
    slot = int(dev.b.r.slots_of(["doc"])[0])
    # one batch, the packed paths' offsets not 8-aligned: 0 5 12 12 21 29 41 58 75
    order = [1, 2, 0, 4, 3, 5, 7, 6]
    paths = [LEN_PATHS[i] for i in order]
    po = np.cumsum([0] + [len(U.encode_path(p)) for p in paths])
    assert any(int(x) % 8 for x in po[1:-1])
    want = check(engine, [slot] * len(paths), paths)
    for i, p in enumerate(paths):  # and against the leaves themselves
        got = [by_handle[h] for h in want[2][want[1][i]:want[1][i + 1]]]
        assert sorted(got) == sorted(l for l in leaves if l[0][:len(p)] == p), p
        assert len(got) >= 2
    # the near misses, each a query of its own
    near = [("abc", "d"),                          # a leaf's whole path: it matches, the relative path is empty
            ("abc", "d", "e"),                     # one segment longer than the leaf's path
            ("ab",),                               # a string prefix of "abc", not a segment prefix
            ("abc", "d", "a-segment-much-longer-than-any-leaf-of-this-document" * 3),  # longer than any whole encoding
            ("",)]                                 # the empty segment: not the 4-byte leaf ((), "")
    want = check(engine, [slot] * len(near), near)
    sel = lambda i: sorted(by_handle[h] for h in want[2][want[1][i]:want[1][i + 1]])
    assert sel(0) == [(("abc", "d"), "3")]
    assert R.unpack(np.array(want[3], np.uint8), np.array(want[4], np.uint64))[0] == U._encode((), "3")
    assert sel(1) == [] and sel(3) == [] and sel(4) == []
    assert sel(2) == [(("ab", "x"), "4")]
    # the 4-byte leaf: matched by the empty path alone, as its whole encoding
    sizes, eo, el, lb, lo = engine.ujson_path_read([slot], [()])
    items = dict(zip(el.tolist(), R.unpack(lb, lo)))
    assert items[dev.leaves.handle((), "")] == b"\xff\xff\xff\xff" and sizes[0] == len(leaves)


# ---- documents -------------------------------------------------------------------

TOPS = ("alpha", "b", "gamma-delta", "ü")


def _big_doc(n, salt=""):
    doc = {t: {} for t in TOPS}
    for i in range(n):
        doc[TOPS[i % 4]][f"k{salt}{i}"] = i if i % 3 else f"v{i}" * (i % 7)
    return json.dumps(doc)


@pytest.mark.parametrize("inplace", [None, 0, 1, 3])
def test_documents(engine, inplace):
    """empty documents, missing keys, repeated slots, a leaf under two dots, and
    tiles that cross documents and workgroups -- in the regular layout and, with
    the in-place layout on, in the per-column long layout (appended to and trimmed)"""
    from jylis_amd.engine import Engine
    from jylis_amd.repo import RepoUJSON
    if inplace is not None:
        engine.ujson_set_inplace(inplace)
    dev, old = _docs(engine)
    dev.set("big", (), _big_doc(300))
    dev.set("empty", (), "{}")
    for i in range(6):
        dev.set(f"small{i}", (), _big_doc(1 + 2 * i, salt=f"s{i}"))
    dev.ins("small1", ("alpha", "twice"), "7")
    # a leaf held under two dots: the same INS on a second replica, converged
    engB = Engine(device=0)
    try:
        other = U.UJSONDocs(U.GpuDocs(RepoUJSON(engB)), IDENT_B, U.DeviceLeaves(engB))
        other.ins("small1", ("alpha", "twice"), "7")
        other.ins("big", ("b", "k1"), "1")
        dev.b.r.converge_deltas(other.b.r.flush_deltas())
    finally:
        engB.close()
    # the long document appended to and trimmed: new leaves, the oldest ones removed
    for i in range(300, 320):
        dev.ins("big", (TOPS[i % 4], f"k{i}"), str(i))
    for i in (4, 5, 7, 8):
        dev.rm("big", (TOPS[i % 4], f"k{i}"), str(i))
    if inplace:
        st = engine.ujson_stats()
        assert st["promoted"] > 0 and st["inplace_docs"] > 0
    keys = ["big", "empty", "absent"] + [f"small{i}" for i in range(6)]
    slots = dev.b.r.slots_of(keys)
    assert int(slots[2]) == NO and NO not in [int(s) for s in np.delete(slots, 2)]
    paths = [(), ("alpha",), ("b", "k1"), ("gamma-delta",), ("ü",), ("nothing",), ("b",)]
    # 257 queries: the 300-element document many times over, between empty and small ones
    qs = [(int(slots[(5 * i) % len(slots)]) if i % 3 else int(slots[0]), paths[i % len(paths)]) for i in range(257)]
    want = check(engine, [s for s, _ in qs], [p for _, p in qs])
    assert want[0][2] > 40 * 256 and want[0][3] == 0  # many tiles
    # the same slot in two queries with different paths; an empty document; no such key
    want = check(engine, [slots[0], slots[1], slots[0], slots[2], slots[0]], [("b",), (), ("alpha",), (), ("b", "k1")])
    assert want[1][1] == want[1][2] and want[1][3] == want[1][4]
    two = dev.leaves.handle(("b", "k1"), "1")
    assert want[2][want[1][4]:want[1][5]] == [two, two]  # under two dots: twice
    w1 = check(engine, [dev.b.r.slots_of(["small1"])[0]], [("alpha",)])
    assert w1[2].count(dev.leaves.handle(("alpha", "twice"), "7")) == 2
    check(engine, [NO, NO], [(), ("a",)])
    _same_renders(dev, old, keys, paths)
    sizes, eo, el, lb, lo = engine.ujson_path_read(np.zeros(0, np.uint32), [])
    assert sizes == [0, 0, 0, 0] and eo.tolist() == [0] and lo.tolist() == [0] and len(el) == 0 and len(lb) == 0


def test_missing_leaves(engine):
    dev, _ = _docs(engine)
    hs = _ins(dev, "doc", [(("a",), "1"), (("a", "b"), "2"), (("c",), "3")])
    dev.b.write([("INS", "doc", 0xDEAD0001), ("INS", "doc", 0xDEAD0002), ("INS", "other", 0xDEAD0003)], IDENT_A)
    slots = dev.b.r.slots_of(["doc", "other"])
    want = check(engine, slots, [(), ()])
    assert want[0] == [3, sum(len(U._encode(p, v)) for p, v in [(("a",), "1"), (("a", "b"), "2"), (("c",), "3")]), 6, 3]
    assert sorted(want[2]) == sorted(hs) and want[1] == [0, 3, 3]
    want = check(engine, slots[:1], [("a",)])
    assert want[0][0] == 2 and want[0][2:] == [5, 2]
    for leaves in (True, False):
        with pytest.raises(KeyError):
            dev.leaves.under(slots[:1], [("a",)], leaves)
    with pytest.raises(KeyError):
        dev.get("doc", ("a",))


def _session_docs(engine):
    dev, _ = _docs(engine)
    dev.set("d1", (), _big_doc(40))
    dev.set("d2", (), _big_doc(9, "x"))
    slots = dev.b.r.slots_of(["d1", "d2", "d1"])
    return dev, slots, [("alpha",), (), ("b",)]


def test_two_phase(engine):
    dev, slots, paths = _session_docs(engine)
    want = restate(engine, slots, paths)
    m, nb = want[0][:2]
    fresh = lambda: {"el_offs": np.full(4, 0xCDCD, np.uint64), "elems": np.full(m + 2, 0xCDCD, np.uint64),
                     "leaf_bytes": np.full(nb + 8, 0xCD, np.uint8), "leaf_offs": np.full(m + 3, 0xCDCD, np.uint64)}
    untouched = lambda o: all((a == (0xCD if a.dtype == np.uint8 else 0xCDCD)).all() for a in o.values())
    for cap_el, cap_bytes in ((m - 1, nb), (m, nb - 1), (0, 0)):
        out = fresh()
        sizes, _ = engine.ujson_path_read_caps(slots, paths, True, cap_el, cap_bytes, out=out)
        assert sizes == want[0] and untouched(out), (cap_el, cap_bytes)
    out = fresh()
    sizes, _ = engine.ujson_path_read_caps(slots, paths, True, m, nb, out=out)
    assert sizes == want[0] and out["el_offs"].tolist() == want[1] and out["elems"][:m].tolist() == want[2]
    assert out["leaf_offs"][:m + 1].tolist() == want[4] and out["leaf_bytes"][:nb].tolist() == want[3]
    assert (out["elems"][m:] == 0xCDCD).all() and (out["leaf_bytes"][nb:] == 0xCD).all()
    assert (out["leaf_offs"][m + 1:] == 0xCDCD).all()
    # without JY_PATH_LEAVES: null byte arrays, no bytes counted, cap_bytes ignored
    out = {k: v for k, v in fresh().items() if k in ("el_offs", "elems")}
    sizes, arrays = engine.ujson_path_read_caps(slots, paths, False, m, 0, out=out)
    assert sizes == [m, 0] + want[0][2:] and sorted(arrays) == ["el_offs", "elems"]
    assert out["el_offs"].tolist() == want[1] and out["elems"][:m].tolist() == want[2]
    out = {k: v for k, v in fresh().items() if k in ("el_offs", "elems")}
    sizes, _ = engine.ujson_path_read_caps(slots, paths, False, m - 1, 0, out=out)
    assert sizes[0] == m and untouched(out)


@pytest.mark.parametrize("off", [1, 3, 7])
def test_device_outputs(engine, off):
    import torch
    dev, slots, paths = _session_docs(engine)
    want = restate(engine, slots, paths)
    m, nb = want[0][:2]
    d = "cuda:0"
    buf = torch.full((nb + 16,), 0xAB, dtype=torch.uint8, device=d)
    assert buf.data_ptr() % 8 == 0
    out = {"el_offs": torch.empty(4, dtype=torch.int64, device=d), "elems": torch.empty(m, dtype=torch.int64, device=d),
           "leaf_bytes": buf[off:], "leaf_offs": torch.empty(m + 1, dtype=torch.int64, device=d)}
    need, _ = engine.ujson_path_read_caps(slots, paths, True, 0, 0, device=True)
    assert need == want[0]
    sizes, _ = engine.ujson_path_read_caps(slots, paths, True, m, nb, device=True, out=out)
    engine.sync()
    assert sizes == want[0]
    u64 = lambda t: t.cpu().numpy().view(np.uint64).tolist()
    assert u64(out["el_offs"]) == want[1] and u64(out["elems"]) == want[2] and u64(out["leaf_offs"]) == want[4]
    raw = buf.cpu().numpy()
    assert raw[off:off + nb].tolist() == want[3]
    assert (raw[:off] == 0xAB).all() and (raw[off + nb:] == 0xAB).all()  # nothing outside the output
    # the convenience form, device end to end
    sizes, eo, el, lb, lo = engine.ujson_path_read(slots, paths, device=True)
    engine.sync()
    assert all(t.is_cuda for t in (eo, el, lb, lo))
    assert [u64(eo), u64(el), lb.cpu().numpy().tolist(), u64(lo)] == list(want[1:])


def _raw(eng, slots, pb, po, flags=1):
    """the C call on hand-made query arrays (sizes only) -> (return code, sizes)"""
    s = np.asarray(slots, np.uint32)
    pb = np.frombuffer(bytes(pb) or b"\0", np.uint8)
    po = np.asarray(po, np.uint64)
    eo = np.full(len(s) + 1, 0xCDCD, np.uint64)
    sizes = (C.c_uint64 * 4)(7, 7, 7, 7)
    rc = eng.lib.jy_ujson_path_read(eng.h, len(s), s.ctypes.data, pb.ctypes.data, po.ctypes.data, flags, 0, 0,
                                    eo.ctypes.data, None, None, None, sizes, 0)
    return rc, [int(x) for x in sizes], eo


def test_host_validation(engine):
    """malformed queries are refused on the host -- nothing reaches the device --
    and a valid call after each one succeeds"""
    from jylis_amd._lib import JY_EINVAL, JY_ERANGE, JY_OK
    dev, slots, paths = _session_docs(engine)
    want = restate(engine, slots, paths)
    a, b = U.encode_path(("alpha",)), U.encode_path(("b",))
    s2 = slots[:2]
    good = (s2, a + b, [0, len(a), len(a) + len(b)])
    skipped = engine.skipped()
    cut = U.encode_path(("alpha", "beta"))[:-2]
    bad = [
        ((s2, a + b, [0, len(a) + len(b), len(a)]), JY_EINVAL, "ascending"),            # descending path_offs
        ((s2, a + cut, [0, len(a), len(a) + len(cut)]), JY_EINVAL, "cut short"),          # the last segment cut short
        ((s2, a + b"\x02\x00", [0, len(a), len(a) + 2]), JY_EINVAL, "length word"),       # ... inside its length word
        ((s2, a + b"\xff\xff\xff\xff", [0, len(a), len(a) + 4]), JY_ERANGE, "2^24"),     # a segment length of 0xFFFFFFFF
        (([slots[0], engine.nkeys(UJSON)], a + b, good[2]), JY_ERANGE, "past the interned keys"),  # a slot >= the key count
        ((s2, a + b, good[2], 2), JY_EINVAL, "flags"),                                   # an unknown flag
    ]
    for args, code, word in bad:
        rc, sizes, eo = _raw(engine, *args)
        assert rc == code and sizes == [0, 0, 0, 0] and (eo == 0xCDCD).all(), (word, rc, sizes)
        assert word in engine.lib.jy_last_error(engine.h).decode()
        rc, sizes, _ = _raw(engine, *good)
        assert rc == JY_OK and sizes[2] == 49 and sizes[0] > 0  # the next valid call
    assert engine.skipped() == skipped
    check(engine, slots, paths)
    assert restate(engine, slots, paths) == want


def test_read_only(engine):
    dev, slots, paths = _session_docs(engine)
    dev.ins("d2", ("b", "more"), '"text"')
    before = (engine.digest(UJSON, 4).tolist(), engine.ujson_leaves_usage(), engine.ujson_deltas_size())
    for _ in range(3):
        check(engine, slots, paths)
        engine.ujson_path_read(slots, paths, leaves=False)
        dev.get_paths(["d1", "d2", "nope"], [("alpha",), (), ("b",)])
    after = (engine.digest(UJSON, 4).tolist(), engine.ujson_leaves_usage(), engine.ujson_deltas_size())
    assert before == after
