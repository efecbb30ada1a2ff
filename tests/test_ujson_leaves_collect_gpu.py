"""Collecting the UJSON leaf store on the GPU (jy_ujson_leaves_collect,
jylis_amd/csrc/k_leaf.hip) against the numpy restatement
(tests/leaves_collect_ref.py): which leaves survive, the exact counters, the
bytes of the survivors after the arena was rebuilt, probe chains after the
table was rebuilt, both document layouts, the pending deltas, `keep`, dead
pool runs, the auto-collecting DeviceLeaves, opaque handles, shrinking, bad
arguments and a node's shards."""
import ctypes as C

import numpy as np
import pytest

import leaves_collect_ref as CR
import leaves_ref as R
from jylis_amd import ujson_doc as U
from test_ujson_doc import IDENT_A, IDENT_B, OracleDocs, _replay
from test_ujson_inplace_gpu import _table
from test_ujson_leaves_gpu import LENGTHS, _steps

pytestmark = pytest.mark.gpu
UJSON = 4
IDS = [0xA1, 0xB2]  # the replica ids behind columns 0 and 1 of the hand-made batches
MIN_ARENA = 1 << 16  # kMinArena of k_leaf.hip


def _enc(i, tag="c"):
    return U._encode((tag, str(i)), '"value %d"' % i)


def _table_of(docs):
    """{key: [handles]} -> a full-state batch, each document's elements dealt over two replica columns"""
    rows = []
    for k, hs in docs.items():
        els, vv = {}, {}
        for i, h in enumerate(hs):
            c = i % 2
            vv[c] = vv.get(c, 0) + 1
            els[(c, vv[c])] = int(h)
        rows.append((k.encode(), els, vv, set()))
    return _table(IDS, rows)


def _converge(eng, docs):
    from jylis_amd.repo import RepoUJSON
    RepoUJSON(eng).converge_deltas(_table_of(docs))


def _state_elems(eng):
    n = eng.nkeys(UJSON)
    return eng.state_wire(UJSON, 0, n)["elems"] if n else np.zeros(0, np.uint64)


def _put(eng, encs):
    got = eng.ujson_leaves_put(*R.pack(encs))
    assert got.tolist() == [R.handle_of(e) for e in encs]
    return dict(zip(got.tolist(), encs))


def _get(eng, handles):
    """-> (items, handles the store does not hold)"""
    hs = np.asarray(list(handles), np.uint64)
    if len(hs) == 0:
        return [], 0
    need, _, _ = eng.ujson_leaves_get_caps(hs, 0)
    return R.unpack(*eng.ujson_leaves_get(hs)), need[1]


def _collect(eng, stored, pending=(), keep=(), shrink=False):
    """one collection checked against the restatement in full: out6, the usage,
    every kept leaf's bytes (asked for in reverse), every dropped handle missing
    -> the kept {handle: encoding}"""
    want, kept = CR.collect(stored, _state_elems(eng), pending, keep)
    got = eng.ujson_leaves_collect(np.asarray(list(keep), np.uint64) if len(keep) else None, shrink)
    assert tuple(got) == want, (tuple(got), want)
    assert eng.ujson_leaves_usage()[:2] == want[:2]
    order = sorted(kept)[::-1]
    assert _get(eng, order) == ([kept[h] for h in order], 0)
    gone = sorted(set(stored) - set(kept))
    assert _get(eng, gone) == ([b""] * len(gone), len(gone))
    return kept


def test_never_used_store(engine):
    assert tuple(engine.ujson_leaves_collect()) == (0,) * 6
    assert tuple(engine.ujson_leaves_collect(np.array([5, 0], np.uint64), shrink=True)) == (0,) * 6
    _converge(engine, {"d": [11, 12]})  # documents, still no store
    assert tuple(engine.ujson_leaves_collect()) == (0,) * 6
    stored = _put(engine, [_enc(1), _enc(2)])
    assert _get(engine, stored) == (list(stored.values()), 0)


def test_lengths(engine):
    """every length of LENGTHS, every second one INSerted (so it is live in the
    state AND in the pending delta).  The leaves are put one call each, so the
    arena holds them in put order: ... 64 (dead), 70000 (live), 1000 (dead), 65"""
    from jylis_amd.repo import RepoUJSON
    encs = [U._encode(*R.leaf_of_length(n)) for n in LENGTHS]
    assert [len(e) for e in encs] == list(LENGTHS) and LENGTHS[12] == 70000
    arena_order = list(range(10)) + [12, 11, 10]
    stored = {}
    for i in arena_order:
        stored.update(_put(engine, [encs[i]]))
    live = [R.handle_of(encs[i]) for i in range(0, len(encs), 2)]
    assert R.handle_of(encs[12]) in live and R.handle_of(encs[9]) not in live and R.handle_of(encs[11]) not in live
    RepoUJSON(engine).write([("INS", "doc%d" % (j % 2), h) for j, h in enumerate(live)], IDENT_A)
    assert sorted(_state_elems(engine).tolist()) == sorted(live)
    kept = _collect(engine, stored, pending=live)
    assert sorted(kept) == sorted(live)
    assert engine.ujson_leaves_usage()[1] == sum(CR.rounded(LENGTHS[i]) for i in range(0, len(encs), 2))
    # the next flush still finds every pending element's leaf, the long one included
    w = engine.flush_wire(UJSON, leaves=True)
    assert sorted(w["elems"].tolist()) == sorted(live)
    assert R.unpack(w["leaf_bytes"], w["leaf_offs"]) == [stored[int(h)] for h in w["elems"]]


@pytest.mark.parametrize("n", [500, 600])
def test_probe_chains_survive(engine, n):
    """500 leaves in the minimum 1,024-entry table (load 0.49: clusters); 600
    put as 500 + 100 cross one growth of the table"""
    encs = [_enc(i, "probe") for i in range(n)]
    stored = _put(engine, encs[:500])
    if n > 500:
        stored.update(_put(engine, encs[500:]))
    hs = list(stored)
    _converge(engine, {"d%d" % j: hs[j::20][:n // 20] for j in range(0, 20, 2)})  # every second handle
    kept = _collect(engine, stored)
    assert sorted(kept) == sorted(hs[0::2]) and len(kept) == n // 2


def test_all_live_then_all_dead(engine):
    encs = [_enc(i, "all") for i in range(40)] + [U._encode(*R.leaf_of_length(3001))]
    stored = _put(engine, encs)
    _converge(engine, {"a": list(stored)[:30], "b": list(stored)[30:]})
    before = engine.ujson_leaves_usage()
    for _ in range(2):
        assert _collect(engine, stored) == stored
        assert engine.ujson_leaves_usage() == before
    # nothing referenced: a second engine holds the same leaves under no document
    from jylis_amd.engine import Engine
    other = Engine(device=0)
    try:
        assert _put(other, encs) == stored
        assert _collect(other, stored) == {}
        assert other.ujson_leaves_usage()[:2] == (0, 0)
        assert _put(other, encs) == stored  # the same handles, stored anew
        assert other.ujson_leaves_usage()[:2] == before[:2] and _get(other, stored) == (encs, 0)
    finally:
        other.close()


def test_both_layouts(engine):
    engine.ujson_set_inplace(3)
    long_doc = _put(engine, [_enc(i, "long") for i in range(8)])
    short_doc = _put(engine, [_enc(i, "short") for i in range(2)])
    unreferenced = _put(engine, [_enc(i, "none") for i in range(5)])
    hs = list(long_doc)
    _converge(engine, {"long": hs[:6], "short": list(short_doc)})
    # an append-shaped delta: one more dot per column of the long document
    engine_ids = _table(IDS, [(b"long", {(0, 4): hs[6], (1, 4): hs[7]}, {}, {(0, 4), (1, 4)})])
    from jylis_amd.repo import RepoUJSON
    RepoUJSON(engine).converge_deltas(engine_ids)
    assert engine.ujson_stats()["promoted"] > 0
    assert sorted(_state_elems(engine).tolist()) == sorted(list(long_doc) + list(short_doc))
    kept = _collect(engine, {**long_doc, **short_doc, **unreferenced})
    assert kept == {**long_doc, **short_doc}


def test_pending_deltas_are_live(engine):
    from jylis_amd.repo import RepoUJSON
    repo = RepoUJSON(engine)
    stored = _put(engine, [_enc(7, "pend"), _enc(8, "other")])
    h, other = list(stored)
    repo.write([("INS", "doc", h)], IDENT_A)
    assert _state_elems(engine).tolist() == [h]
    # a peer's delta whose context covers the dot and carries no element
    repo.converge_deltas(_table([IDENT_A], [(b"doc", {}, {0: 1}, set())]))
    assert _state_elems(engine).tolist() == []
    kept = _collect(engine, stored, pending=[h])
    assert list(kept) == [h]
    w = engine.flush_wire(UJSON, leaves=True)
    assert w["elems"].tolist() == [h] and R.unpack(w["leaf_bytes"], w["leaf_offs"]) == [stored[h]]
    assert _collect(engine, kept) == {}


def test_keep(engine):
    import torch
    stored = _put(engine, [_enc(i, "keep") for i in range(6)])
    hs = list(stored)
    _converge(engine, {"d": hs[:2]})
    kept = _collect(engine, stored, keep=[hs[4]])
    assert sorted(kept) == sorted(hs[:2] + [hs[4]])
    # handle 0 is ignored, an unknown handle (twice) and a dropped one are counted
    want, kept2 = CR.collect(kept, _state_elems(engine), keep=[0, hs[4], 0x5151, 0x5151, hs[5]])
    dev = torch.from_numpy(np.array([0, hs[4], 0x5151, 0x5151, hs[5]], np.uint64).view(np.int64)).to("cuda:0")
    got = engine.ujson_leaves_collect(dev)
    assert tuple(got) == want and got.keep_without_leaf == 3 and kept2 == kept
    assert _get(engine, [hs[4]]) == ([stored[hs[4]]], 0)
    assert sorted(_collect(engine, kept)) == sorted(hs[:2])  # no keep: the handle loses its leaf
    assert _put(engine, [stored[hs[4]]]) == {hs[4]: stored[hs[4]]}  # and gets it back under the same handle


class _Recording(U.DeviceLeaves):
    """DeviceLeaves that remembers every leaf it was asked to store"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.put = {}

    def handle(self, path, value):
        h = super().handle(path, value)
        self.put[h] = U._encode(tuple(path), value)
        return h


def test_stale_runs_are_not_walked(engine):
    from jylis_amd.repo import RepoUJSON
    leaves = _Recording(engine)
    docs = U.UJSONDocs(U.GpuDocs(RepoUJSON(engine)), IDENT_A, leaves)
    keys = ["doc%d" % i for i in range(4)]
    for k in keys:
        docs.set(k, (), '{"a":"first","fixed":{"x":["%s",1]}}' % k)
    for rnd in range(10):
        for k in keys:
            docs.set(k, ("a",), '{"v":"%s round %d","w":[%d,"t"]}' % (k, rnd, rnd))
    before = docs.get_many(keys)
    digest = engine.digest(UJSON, 16)
    state = _state_elems(engine)
    assert len(leaves.put) > 3 * len(set(state.tolist()))  # the old values' leaves are still stored
    # the pending deltas still hold the old elements: they stay until the flush
    first = engine.ujson_leaves_collect()
    w = engine.flush_wire(UJSON, leaves=True)
    assert tuple(first) == CR.collect(leaves.put, state, w["elems"])[0]
    assert (np.diff(w["leaf_offs"].astype(np.int64)) > 0).all() and len(w["elems"]) > len(state)
    # flushed: exactly the leaves of the current render remain
    kept = _collect(engine, CR.collect(leaves.put, state, w["elems"])[1])
    assert sorted(kept) == sorted(set(state.tolist()))
    assert docs.get_many(keys) == before and all(U.canonical(t) is not None for t in before)
    np.testing.assert_array_equal(engine.digest(UJSON, 16), digest)


def test_session_replay_with_auto_collect(oracle_mod, engine):
    from jylis_amd.repo import RepoUJSON
    O = oracle_mod
    leaves = U.DeviceLeaves(engine, auto_collect=True, floor=0)
    docs = U.UJSONDocs(U.GpuDocs(RepoUJSON(engine)), IDENT_A, leaves)
    want = U.UJSONDocs(OracleDocs(O.Repo(O.UJSON, IDENT_A)), IDENT_A, U.LeafTable())
    gets = 0
    for st in _steps():
        if st[0] == "GET":
            got = docs.get(st[1], tuple(st[2]))
            assert U.canonical(got) == U.canonical(want.get(st[1], tuple(st[2]))) == U.canonical(st[3]), st
            gets += 1
            continue
        _replay(docs, [st], check=False)
        _replay(want, [st], check=False)
    keys = sorted({st[1] for st in _steps()})
    for path in ((), ("a",), ("a", "b")):
        assert [U.canonical(t) for t in docs.get_many(keys, path)] == \
            [U.canonical(t) for t in want.get_many(keys, path)]
    assert gets > 0 and leaves.collections >= 1


def test_opaque_handles(engine):
    stored = _put(engine, [_enc(i, "real") for i in range(5)])
    hs = list(stored)
    opaque = {"o1": [1001, 1002, 1003], "o2": [2001, 2002, 2003, 2004]}
    _converge(engine, {**opaque, "real": hs[:3]})
    want, kept = CR.collect(stored, _state_elems(engine))
    assert want[4] == 7 and sorted(kept) == sorted(hs[:3])
    assert _collect(engine, stored) == kept


def test_shrink(engine):
    first = [_enc(i, "shrink") for i in range(3000)]
    stored = _put(engine, first)
    hs = list(stored)
    _converge(engine, {"d%d" % j: hs[j * 8:j * 8 + 8] for j in range(8)})  # 64 of 3,000
    cap0 = engine.ujson_leaves_usage()[2]
    assert cap0 > MIN_ARENA
    kept = _collect(engine, stored)
    assert len(kept) == 64 and engine.ujson_leaves_usage()[2] == cap0
    kept = _collect(engine, kept, shrink=True)
    n, used, cap, coll = engine.ujson_leaves_usage()
    assert (n, coll) == (64, 0) and cap == max(MIN_ARENA, 2 * used) and cap < cap0
    second = _put(engine, [_enc(i, "again") for i in range(3000)])  # grows the table and the arena again
    n2, used2, cap2, coll2 = engine.ujson_leaves_usage()
    assert n2 == 3064 and cap2 >= used2 > cap and coll2 == 0
    everything = {**kept, **second}
    assert _get(engine, everything) == (list(everything.values()), 0)


def test_bad_arguments(engine):
    from jylis_amd import _lib
    stored = _put(engine, [_enc(i, "bad") for i in range(3)])
    before = engine.ujson_leaves_usage()
    out = np.full(6, 99, np.uint64)
    keep = np.array(list(stored), np.uint64)
    call = engine.lib.jy_ujson_leaves_collect
    assert call(engine.h, 0, None, _lib.HOST, 2, out.ctypes.data) == _lib.JY_EINVAL
    assert b"flags" in engine.lib.jy_last_error(engine.h)
    assert call(engine.h, 0, None, _lib.HOST, 0x80000001, out.ctypes.data) == _lib.JY_EINVAL
    assert call(engine.h, 3, C.c_void_p(keep.ctypes.data), 7, 0, out.ctypes.data) == _lib.JY_EINVAL
    assert b"keep_mem" in engine.lib.jy_last_error(engine.h)
    assert engine.ujson_leaves_usage() == before and _get(engine, stored) == (list(stored.values()), 0)
    # a router's rounds in flight refuse the call, as they refuse arena_collect
    engine._route_holds = {1}
    with pytest.raises(RuntimeError):
        engine.ujson_leaves_collect()
    engine._route_holds = set()
    assert engine.ujson_leaves_usage() == before


def test_node_collects_every_shard():
    from jylis_amd.engine import Engine
    from jylis_amd.node import Node
    from jylis_amd.repo import RepoUJSON
    node, src = Node(2, "copy"), Engine(device=0)
    try:
        rec = _Recording(src)
        A = U.UJSONDocs(U.GpuDocs(RepoUJSON(src)), IDENT_A, rec)
        keys = ["doc%d" % i for i in range(12)]
        ids = lambda: [src.replica_id(c) for c in range(src.replica_count())]
        for i, k in enumerate(keys):
            A.set(k, (), '{"a":{"b":%d,"c":["x%d","y%d"]},"k":"%s"}' % (i, i, i, k))
        w1 = src.flush_wire(UJSON, leaves=True)
        node.restore(UJSON, [w1], col_ids=ids())
        for k in keys:
            A.clr(k, ("a", "c"))  # two of every document's four elements
        w2 = src.flush_wire(UJSON, leaves=True)
        assert len(w1["elems"]) == 48 and len(w2["cloud"]) + len(w2["vv"]) > 0
        node.restore(UJSON, [w2], col_ids=ids())
        node.sync()
        # what each shard's store was given: the leaves of the documents it owns
        raw, ko, eo = w1["key_bytes"].tobytes(), w1["key_offs"].astype(np.int64), w1["el_offs"].astype(np.int64)
        stored = [{} for _ in range(2)]
        for i in range(len(ko) - 1):
            s = node.shard_of(raw[ko[i]:ko[i + 1]].decode())
            stored[s].update({int(h): rec.put[int(h)] for h in w1["elems"][eo[i]:eo[i + 1]]})
        assert all(stored)
        want = []
        for s, e in enumerate(node.engines):
            with node.locked(UJSON):
                want.append(CR.collect(stored[s], _state_elems(e))[0])
        got = node.ujson_leaves_collect()
        assert [tuple(g) for g in got] == want
        assert sum(g.kept for g in got) == 24 and sum(g.dropped for g in got) == 24
        assert sum(g.elements_without_leaf for g in got) == 0
        seen = 0
        for _, batch in node.snapshot(UJSON, max_keys=5, leaves=True):
            assert len(batch["leaf_offs"]) == len(batch["elems"]) + 1
            assert (np.diff(batch["leaf_offs"].astype(np.int64)) > 0).all()
            seen += len(batch["elems"])
        assert seen == 24
    finally:
        node.close()
        src.close()
