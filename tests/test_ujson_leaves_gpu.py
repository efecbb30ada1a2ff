"""The UJSON leaf store on the GPU (jy_ujson_leaves_*, jylis_amd/csrc/k_leaf.hip)
and the wire batches that carry their leaves: put / get against the host
formula, the two-phase get, repeats racing in one launch, growth, unknown
handles, malformed input, batches with leaves against the numpy restatement
(tests/leaves_ref.py), and the gap they close -- a fresh process that received
a batch, a snapshot or a repair round can render its documents."""
import numpy as np
import pytest

import leaves_ref as R
from jylis_amd import ujson_doc as U
from test_ujson_doc import IDENT_A, IDENT_B, OracleDocs, _replay, _session

pytestmark = pytest.mark.gpu
UJSON = 4
LENGTHS = (4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 1000, 70000)
NESTED = ("a",)
# the docs session ends with a CLR of its only document: more writes, so that final states render something
EXTRA = [["SET", "doc:1", [], '{"a":{"b":1,"c":["x","y"]},"k":"v1","ü":"日本"}'], ["INS", "doc:1", ["a", "b"], "2"],
         ["SET", "doc:2", ["a"], '{"b":[true,null],"d":"z"}'], ["RM", "doc:1", ["a", "c"], '"x"'],
         ["SET", "users:my-user", ["contact"], '{"email":"e@x"}'], ["CLR", "doc:2", ["a", "d"]]]


def _steps():
    return _session() + EXTRA


def _leaves():
    """(path, value) of every length of LENGTHS, then paths and non-ASCII text"""
    out = [R.leaf_of_length(n) for n in LENGTHS]
    out += [R.leaf_of_length(n, ("p", "qq")) for n in (15, 16, 17, 65, 1000)]
    out += [(("ключ", "é"), '"日本語"'), (("",), "null"), (("a", "b"), '"ü"'), ((), '"x"')]
    return out


@pytest.fixture(scope="module")
def table():
    """the leaves, their encodings and their handles by LeafTable (computed once)"""
    lt = U.LeafTable()
    leaves = _leaves()
    encs = [U._encode(p, v) for p, v in leaves]
    hs = [lt.handle(p, v) for p, v in leaves]
    assert [len(e) for e in encs[:len(LENGTHS)]] == list(LENGTHS) and len(set(hs)) == len(hs)
    return leaves, encs, np.array(hs, np.uint64)


def _get(eng, handles):
    lb, lo = eng.ujson_leaves_get(np.asarray(handles, np.uint64))
    return R.unpack(lb, lo)


def test_put_get_host(engine, table):
    leaves, encs, hs = table
    got = engine.ujson_leaves_put(*R.pack(encs))
    assert got.tolist() == hs.tolist()
    assert _get(engine, hs) == encs
    assert _get(engine, hs[::-1]) == encs[::-1]
    n, used, cap, coll = engine.ujson_leaves_usage()
    assert n == len(encs) and coll == 0 and cap >= used == sum((len(e) + 7) // 8 * 8 for e in encs)
    # DeviceLeaves: LeafTable's interface over the same store
    dl = U.DeviceLeaves(engine)
    assert [dl.handle(p, v) for p, v in leaves[-4:]] == hs[-4:].tolist()
    assert dl.leaves(hs.tolist()) == [(tuple(p), v) for p, v in leaves] and dl.leaf(hs[0]) == leaves[0]
    assert engine.ujson_leaves_usage()[:2] == (n, used)
    with pytest.raises(KeyError):
        dl.leaf(12345)


@pytest.mark.parametrize("off", [1, 3, 7])
def test_put_get_device(engine, table, off):
    import torch
    leaves, encs, hs = table
    lb, lo = R.pack(encs)
    dev = "cuda:0"
    got = engine.ujson_leaves_put(torch.from_numpy(lb).to(dev), torch.from_numpy(lo.view(np.int64)).to(dev))
    engine.sync()
    assert got.cpu().numpy().view(np.uint64).tolist() == hs.tolist()
    # handles on the device, the output bytes starting `off` bytes past an 8-byte boundary
    order = np.random.default_rng(off).permutation(len(hs))
    h = torch.from_numpy(hs[order].view(np.int64)).to(dev)
    need, _, _ = engine.ujson_leaves_get_caps(h, 0, device=True)
    assert need == [sum(len(e) for e in encs), 0]
    buf = torch.full((need[0] + 16,), 0xAB, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 8 == 0
    offs = torch.empty(len(hs) + 1, dtype=torch.int64, device=dev)
    sizes, _, _ = engine.ujson_leaves_get_caps(h, need[0], device=True, out=(buf[off:], offs))
    engine.sync()
    assert sizes == need
    raw = buf.cpu().numpy()
    assert R.unpack(raw[off:off + need[0]], offs.cpu().numpy().view(np.uint64)) == [encs[i] for i in order]
    assert (raw[:off] == 0xAB).all() and (raw[off + need[0]:] == 0xAB).all()  # nothing outside the output


def test_two_phase_get(engine, table):
    _, encs, hs = table
    engine.ujson_leaves_put(*R.pack(encs[:6]))
    total = sum(len(e) for e in encs[:6])
    lb, lo = np.full(total + 8, 0xCD, np.uint8), np.full(7, 0xCDCD, np.uint64)
    sizes, _, _ = engine.ujson_leaves_get_caps(hs[:6], total - 1, out=(lb, lo))
    assert sizes == [total, 0] and (lb == 0xCD).all() and (lo == 0xCDCD).all()  # too small: nothing written
    sizes, _, _ = engine.ujson_leaves_get_caps(hs[:6], total, out=(lb, lo))
    assert sizes == [total, 0] and R.unpack(lb[:total], lo) == encs[:6] and (lb[total:] == 0xCD).all()
    lo = np.full(1, 0xCDCD, np.uint64)
    sizes, _, _ = engine.ujson_leaves_get_caps(np.zeros(0, np.uint64), 0, out=(lb, lo))
    assert sizes == [0, 0] and lo.tolist() == [0]  # n == 0: the single offset


def test_repeats_in_one_launch(engine):
    rng = np.random.default_rng(11)
    distinct = [U._encode(("r", str(i)), '"' + "y" * int(rng.integers(0, 40)) + '"') for i in range(64)]
    pick = np.concatenate([np.arange(64), rng.integers(0, 64, 4096 - 64)])
    rng.shuffle(pick)
    items = [distinct[i] for i in pick]
    got = engine.ujson_leaves_put(*R.pack(items))
    assert got.tolist() == [R.handle_of(b) for b in items]  # equal leaves, equal handles
    before = engine.ujson_leaves_usage()
    assert before[0] == 64 and before[1] == sum((len(e) + 7) // 8 * 8 for e in distinct) and before[3] == 0
    assert _get(engine, got) == items
    again = engine.ujson_leaves_put(*R.pack(items))
    assert again.tolist() == got.tolist() and engine.ujson_leaves_usage()[:2] == before[:2]
    assert engine.skipped() == 0


def test_growth_without_reserve(engine):
    batches = [[U._encode(("g", str(b), str(i)), str(i * 7 + b)) for i in range(3000)] for b in range(3)]
    caps, sample = [], None
    for b, items in enumerate(batches):
        got = engine.ujson_leaves_put(*R.pack(items))
        assert got.tolist() == [R.handle_of(x) for x in items]
        caps.append(engine.ujson_leaves_usage())
        if b == 0:
            sample = (got[::97].copy(), items[::97])
            assert _get(engine, sample[0]) == sample[1]
    assert [c[0] for c in caps] == [3000, 6000, 9000] and caps[-1][3] == 0
    # the arena was reallocated; the table made for the first put (8,192 entries for 3,000
    # leaves) cannot hold 9,000: reading every leaf back below shows the rehashes kept them
    assert caps[-1][2] > caps[0][2] and caps[-1][2] >= caps[-1][1]
    assert _get(engine, sample[0]) == sample[1]
    everything = [x for items in batches for x in items]
    assert _get(engine, [R.handle_of(x) for x in everything]) == everything
    # reserve: room made ahead, nothing lost
    engine.ujson_leaves_reserve(40000, 4 << 20)
    assert engine.ujson_leaves_usage()[2] >= 4 << 20 and _get(engine, sample[0]) == sample[1]


def test_unknown_handles_and_handle_zero(engine, table):
    _, encs, hs = table
    assert engine.ujson_leaves_get_caps(np.array([5, 0], np.uint64), 0)[0] == [0, 2]  # an empty store
    engine.ujson_leaves_put(*R.pack(encs[:3]))
    ask = np.array([hs[1], 0, 0xDEADBEEF, hs[0], hs[5], hs[2]], np.uint64)  # hs[5] was never put
    sizes, _, _ = engine.ujson_leaves_get_caps(ask, 0)
    assert sizes == [len(encs[1]) + len(encs[0]) + len(encs[2]), 3]
    assert _get(engine, ask) == [encs[1], b"", b"", encs[0], b"", encs[2]]


def test_malformed_host_input(engine, table):
    from jylis_amd.engine import EngineError
    _, encs, hs = table
    lb, lo = R.pack(encs[:4])
    bad = lo.copy()
    bad[2], bad[3] = lo[3], lo[2]  # decreasing offsets: rejected on the host, before any launch
    with pytest.raises(EngineError) as e:
        engine.ujson_leaves_put(lb, bad)
    assert e.value.code == -1 and engine.ujson_leaves_usage()[0] == 0 and engine.skipped() == 0
    # a 3-byte item between valid neighbours: skipped, counted, handle 0
    items = [encs[0], b"\xff\xff\xff", encs[1]]
    got = engine.ujson_leaves_put(*R.pack(items))
    assert got.tolist() == [int(hs[0]), 0, int(hs[1])]
    assert engine.skipped() == 1 and engine.ujson_leaves_usage()[0] == 2
    assert engine.ujson_leaves_put(*R.pack(encs[2:4])).tolist() == hs[2:4].tolist()  # the next valid call
    assert _get(engine, hs[:4]) == encs[:4] and engine.skipped() == 1


# ---- wire batches with leaves ---------------------------------------------------

def _written(O, eng, ident):
    """the docs session through DeviceLeaves plus a random history of opaque
    elements (no leaves behind them) -> (docs, {handle: encoding})"""
    from helpers import random_history
    from jylis_amd.repo import RepoUJSON
    repo = RepoUJSON(eng)
    docs = U.UJSONDocs(U.GpuDocs(repo), ident, U.DeviceLeaves(eng))
    _replay(docs, _steps())
    for b in random_history(O, O.UJSON, 77, nops=60, nkeys=5):
        repo.converge_deltas(b)
    host = U.LeafTable()
    mirror = U.UJSONDocs(OracleDocs(O.Repo(O.UJSON, ident)), ident, host)
    _replay(mirror, _steps(), check=False)
    return docs, {h: U._encode(p, v) for h, (p, v) in host._leaf.items()}


def _same_arrays(a, b):
    assert sorted(a) == sorted(b)
    for name in a:
        np.testing.assert_array_equal(np.asarray(a[name]), np.asarray(b[name]), err_msg=name)


def test_wire_batches_with_leaves(oracle_mod, engine):
    from jylis_amd.engine import WIRE_ARRAYS
    engine.ujson_set_inplace(1)
    docs, tab = _written(oracle_mod, engine, IDENT_A)
    assert engine.ujson_stats()["promoted"] > 0  # documents in the in-place long layout
    names = [name for name, _, _, _ in WIRE_ARRAYS[UJSON]]
    n = engine.nkeys(UJSON)

    def check(plain, full, mixed=True):
        assert list(plain) == names and list(full) == names + ["leaf_bytes", "leaf_offs"]
        _same_arrays(plain, {k: full[k] for k in names})  # leaves=False: array for array what it always was
        lb, lo = R.batch_leaves(full["elems"], tab)
        assert full["leaf_bytes"].dtype == np.uint8 and full["leaf_offs"].dtype == np.uint64
        np.testing.assert_array_equal(full["leaf_offs"], lo)
        np.testing.assert_array_equal(full["leaf_bytes"], lb)
        known = np.isin(full["elems"], np.array(sorted(tab), np.uint64))
        assert known.any() and known.all() != mixed  # a state dump: session leaves and opaque history elements
    check(engine.state_wire(UJSON, 0, n), engine.state_wire(UJSON, 0, n, leaves=True))
    check(engine.state_wire(UJSON, 1, n - 2), engine.state_wire(UJSON, 1, n - 2, leaves=True))
    slots = np.arange(0, n, 2, dtype=np.uint32)
    check(engine.state_wire_slots(UJSON, slots), engine.state_wire_slots(UJSON, slots, leaves=True))
    parts = list(engine.snapshot(UJSON, max_keys=3, leaves=True))
    assert len(parts) == (n + 2) // 3 and all("leaf_offs" in p for p in parts)
    # the flush: a second engine takes the same writes, one flushes plain, one with leaves
    from jylis_amd.engine import Engine
    other = Engine(device=0)
    try:
        other.ujson_set_inplace(1)
        _written(oracle_mod, other, IDENT_A)
        full = engine.ujson_flush_wire(leaves=True)
        assert len(full["elems"]) > 0 and engine.ujson_deltas_size() == 0
        check(other.ujson_flush_wire(), full, mixed=False)
        empty = engine.flush_wire(UJSON, leaves=True)  # nothing pending: an empty batch, one offset
        assert len(empty["elems"]) == 0 and empty["leaf_offs"].tolist() == [0] and len(empty["leaf_bytes"]) == 0
    finally:
        other.close()


def test_device_batch_with_leaves_stays_on_the_device(oracle_mod, engine):
    docs, tab = _written(oracle_mod, engine, IDENT_A)
    n = engine.nkeys(UJSON)
    host = engine.state_wire(UJSON, 0, n, leaves=True)
    dev = engine.state_wire(UJSON, 0, n, device=True, leaves=True)
    engine.sync()
    assert all(v.is_cuda for v in dev.values())
    from jylis_amd.repo import wire_to_host
    _same_arrays(host, wire_to_host(UJSON, dev))


# ---- the end-to-end gap ----------------------------------------------------------

def _render_all(docs, keys):
    return [[U.canonical(t) for t in docs.get_many(keys, p)] for p in ((), NESTED, ("a", "b"))]


def _session_keys():
    return sorted({st[1] for st in _steps()})


def _writer(eng, ident):
    from jylis_amd.repo import RepoUJSON
    return U.UJSONDocs(U.GpuDocs(RepoUJSON(eng)), ident, U.DeviceLeaves(eng))


def _remapped(src, dst, w):
    """a batch of src with its columns rewritten to dst's, as snapshot.load does"""
    from jylis_amd.snapshot import remap_columns, sort_dots
    col_map = [dst.replica_col(src.replica_id(c)) for c in range(src.replica_count())]
    return sort_dots(UJSON, remap_columns(UJSON, w, col_map))


def test_a_fresh_peer_renders_what_it_was_sent(oracle_mod, engine):
    from jylis_amd.engine import Engine, EngineError
    O = oracle_mod
    keys = _session_keys()
    A = _writer(engine, IDENT_A)
    engB = Engine(device=0)
    try:
        engB.replica_cols([IDENT_B, 0x77, IDENT_A])  # B's columns in another order
        B = _writer(engB, IDENT_B)
        want = U.UJSONDocs(OracleDocs(O.Repo(O.UJSON, IDENT_A)), IDENT_A, U.LeafTable())
        for st in _steps():
            if st[0] == "GET":
                assert U.canonical(B.get(st[1], tuple(st[2]))) == U.canonical(A.get(st[1], tuple(st[2]))) \
                    == U.canonical(st[3]), st
                continue
            _replay(A, [st], check=False)
            _replay(want, [st], check=False)
            engB.converge_wire(UJSON, _remapped(engine, engB, engine.flush_wire(UJSON, leaves=True)))
        assert _render_all(B, keys) == _render_all(A, keys) == _render_all(want, keys)
        assert any(x is not None for x in _render_all(B, keys)[1])  # the nested path renders something
        np.testing.assert_array_equal(engB.digest(UJSON, 16), engine.digest(UJSON, 16))
        # a peer that got the same batches WITHOUT leaves converges, but cannot render
        engC = Engine(device=0)
        try:
            engC.converge_wire(UJSON, _remapped(engine, engC, engine.state_wire(UJSON, 0, engine.nkeys(UJSON))))
            np.testing.assert_array_equal(engC.digest(UJSON, 16), engine.digest(UJSON, 16))
            with pytest.raises(KeyError):
                _writer(engC, IDENT_B).get(keys[0])
        finally:
            engC.close()
        # path-scoped writes on the receiver, on data it never wrote
        key = "doc:1"
        for d in (A, B, want):
            d.clr(key, NESTED)
            d.set(key, ("fresh", "er"), '{"n":[1,2],"s":"t"}')
        assert _render_all(B, keys) == _render_all(A, keys) == _render_all(want, keys)
        # a tampered batch: one handle altered, its leaf bytes unchanged
        A.ins(key, ("late",), '"leaf"')
        w = engine.flush_wire(UJSON, leaves=True)
        assert len(w["elems"]) > 0
        bad = dict(w, elems=w["elems"].copy())
        bad["elems"][len(bad["elems"]) // 2] ^= np.uint64(1 << 17)
        before = engB.digest(UJSON, 16)
        with pytest.raises(EngineError):
            engB.converge_wire(UJSON, _remapped(engine, engB, bad))
        np.testing.assert_array_equal(engB.digest(UJSON, 16), before)
        engB.converge_wire(UJSON, _remapped(engine, engB, w))  # the honest batch still lands
        assert U.canonical(B.get(key, ("late",))) == U.canonical('"leaf"')
    finally:
        engB.close()


def test_snapshot_with_leaves_restores_a_renderable_store(engine, tmp_path):
    from jylis_amd import snapshot
    from jylis_amd.engine import Engine
    keys = _session_keys()
    A = _writer(engine, IDENT_A)
    _replay(A, _steps(), check=False)
    m = snapshot.save(engine, str(tmp_path / "s"), types=(UJSON,), max_keys=2, leaves=True)
    assert m["ujson_leaves"] is True and all("leaf_offs" in c["sizes"] for c in m["chunks"])
    engB = Engine(device=0)
    try:
        engB.replica_cols([0x99, IDENT_B])
        snapshot.load(str(tmp_path / "s"), engB)
        assert _render_all(_writer(engB, IDENT_B), keys) == _render_all(A, keys)
        np.testing.assert_array_equal(engB.digest(UJSON, 16), engine.digest(UJSON, 16))
    finally:
        engB.close()


def test_antientropy_round_with_leaves():
    from jylis_amd import antientropy
    from jylis_amd.node import Node
    keys = _session_keys()
    a, b = Node(1, "copy"), Node(1, "copy")
    try:
        b.replica_col(0x4242)  # b's columns differ from a's
        a.replica_col(IDENT_A)
        A = _writer(a.engines[0], IDENT_A)
        for i, st in enumerate(s for s in _steps() if s[0] != "GET"):
            _replay(A, [st], check=False)
            w = a.flush_wire(UJSON, leaves=True)[0]
            if i % 2 == 0:  # b misses every other flush
                b.restore(UJSON, [w], col_ids=a.replica_ids())
        b.sync()
        assert not np.array_equal(a.digest(UJSON, 16), b.digest(UJSON, 16))
        r = antientropy.sync(a, b, UJSON, nbuckets=16, leaves=True)
        assert r["rounds"] == 1
        np.testing.assert_array_equal(a.digest(UJSON, 16), b.digest(UJSON, 16))
        assert _render_all(_writer(b.engines[0], IDENT_B), keys) == _render_all(A, keys)
    finally:
        a.close()
        b.close()


def test_node_snapshot_restore_reshards_the_leaves():
    from jylis_amd.node import Node
    from jylis_amd.repo import RepoUJSON
    keys = [f"doc{i}" for i in range(12)]
    a, b = Node(2, "copy"), Node(3, "copy")
    try:
        a.replica_col(IDENT_A)
        writers = [_writer(e, IDENT_A) for e in a.engines]
        for i, k in enumerate(keys):
            writers[a.shard_of(k)].set(k, (), '{"a":{"b":%d,"c":["x","y%d"]},"k":"%s"}' % (i, i, k))
        want = {k: U.canonical(writers[a.shard_of(k)].get(k)) for k in keys}
        assert all(e.nkeys(UJSON) > 0 for e in a.engines)
        batches = list(a.snapshot(UJSON, max_keys=4, leaves=True))
        assert all("leaf_bytes" in w for _, w in batches)
        b.restore(UJSON, batches, col_ids=a.replica_ids())
        b.sync()
        np.testing.assert_array_equal(a.digest(UJSON, 8), b.digest(UJSON, 8))
        readers = [U.UJSONDocs(U.GpuDocs(RepoUJSON(e)), IDENT_B, U.DeviceLeaves(e, lambda: b.locked(UJSON)))
                   for e in b.engines]
        owners = {b.shard_of(k) for k in keys}
        assert len(owners) == 3
        for k in keys:
            assert U.canonical(readers[b.shard_of(k)].get(k)) == want[k], k
            assert U.canonical(readers[b.shard_of(k)].get(k, ("a", "c"))) is not None
    finally:
        a.close()
        b.close()
