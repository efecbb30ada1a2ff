"""The state snapshot in wire form on the GPU (jy_*_state_wire): any slot
range's STATE as the arrays the same type's jy_node_*_converge takes --
against the CPU oracle, byte-exact hand-written expectations, range and tile
edges of the counter cell kernels (k_state_wire.hip), the two-phase and
read-only contracts, and the loops it exists for: restore into a fresh
engine, reshard a node, save to files and load."""
import numpy as np
import pytest

from helpers import assert_state_equal, join_rows, random_history, split_rows
from test_flush_wire_gpu import IDENT, OTHER, TYPES, _apply, _by_key, _deltas_size, _flush_wire, _random_ops

pytestmark = pytest.mark.gpu

THIRD = 0x5EED_0000_F1A5_0003
ID_FIELDS = {0: ("ids",), 1: ("p_ids", "n_ids"), 2: (), 3: (), 4: ("dot_ids", "vv_ids", "cloud_ids")}


@pytest.fixture
def engine2():
    from jylis_amd.engine import Engine
    e = Engine(device=0)
    yield e
    e.close()


def _names(ctype):
    from jylis_amd.engine import WIRE_ARRAYS
    return [(name, dt) for name, dt, _, _ in WIRE_ARRAYS[ctype]]


def _dump(eng, ctype):
    return eng.state_wire(ctype, 0, eng.nkeys(ctype))


def _same_wire(ctype, a, b):
    for name, dt in _names(ctype):
        x, y = np.asarray(a[name]), np.asarray(b[name])
        assert x.dtype == y.dtype == np.dtype(dt), name
        np.testing.assert_array_equal(x, y, err_msg=f"array {name}")


def _col_ids(eng):
    return np.array([eng.replica_id(c) for c in range(eng.replica_count())], np.uint64)


def _table(eng, ctype, w=None):
    from jylis_amd.repo import wire_to_table
    return wire_to_table(ctype, _dump(eng, ctype) if w is None else w, _col_ids(eng))


def _history(O, ctype, seed, nkeys=12):
    """~300 operations over `nkeys` keys on 3 replicas: the flushed batches, and
    every replica id in them, ascending"""
    batches = random_history(O, ctype, seed=seed, nrep=3, nops=300, nkeys=nkeys)
    ids = sorted({int(i) for b in batches for f in ID_FIELDS[ctype] for i in np.asarray(b[f]).tolist()})
    return batches, ids


def _populate(O, ctype, eng, seed, nkeys=12):
    """an engine and an oracle replica converged with the same history; the ids
    are registered ascending first, so a key's counter cells (ascending
    column) come in the oracle's order (ascending id)"""
    from jylis_amd.repo import REPOS
    batches, ids = _history(O, ctype, seed, nkeys)
    eng.replica_cols(ids)
    want, got = O.Repo(ctype, 99), REPOS[ctype](eng)
    for b in batches:
        want.converge(b)
        got.converge_deltas(b)
    return want, got


def _is_bottom(ctype, row):
    if ctype == 2:
        return int(row["ts"][0]) == 0 and int(row["val_offs"][-1]) == 0
    if ctype == 3:
        return int(row["cutoff"][0]) == 0 and int(row["ent_offs"][-1]) == 0
    return all(int(v[-1]) == 0 for k, v in row.items() if k.endswith("offs"))


def _assert_equals_oracle(ctype, want, table):
    """joined by key; keys in bottom state that the oracle's state() omits are
    dropped from the dump's side (their presence is pinned by the byte-exact cases)"""
    w, g = dict(split_rows(ctype, want.state())), dict(split_rows(ctype, table))
    for k in list(g):
        if k not in w:
            assert _is_bottom(ctype, g[k]), k
            del g[k]
    assert_state_equal(ctype, join_rows(ctype, w), join_rows(ctype, g))


# 1 ---------------------------------------------------------------------------
@pytest.mark.parametrize("ctype", TYPES)
def test_parity_with_the_oracle(oracle_mod, engine, ctype):
    want, _ = _populate(oracle_mod, ctype, engine, 910 + ctype)
    n = engine.nkeys(ctype)
    assert 8 <= n <= 12
    w = engine.state_wire(ctype, 0, n)
    assert len(w["key_offs"]) == n + 1
    _assert_equals_oracle(ctype, want, _table(engine, ctype, w))


# 2 ---------------------------------------------------------------------------
def _u64(*x):
    return np.array(x, np.uint64)


def _keys(*names):
    from jylis_amd.engine import encode_keys
    return encode_keys(list(names))


def _dot(col, seq):
    return (col << 48) | seq


def test_exact_pncount(engine):
    assert engine.replica_cols([IDENT, OTHER, THIRD]).tolist() == [0, 1, 2]
    kb, ko = _keys("zero", "n-only", "mixed", "big", "plain")
    # the input names each key's cells in no particular order (N before P, columns descending)
    engine.converge_wire(1, {"key_bytes": kb, "key_offs": ko, "cell_offs": _u64(0, 0, 1, 4, 5, 7),
                             "sign": np.array([1, 1, 0, 0, 0, 1, 0], np.uint8),
                             "col": np.array([1, 1, 2, 0, 1, 0, 0], np.uint16),
                             "val": _u64(5, 6, 4, 3, 2**64 - 1, 2, 1)})
    w = _dump(engine, 1)
    assert bytes(w["key_bytes"]) == b"zeron-onlymixedbigplain" and w["key_offs"].tolist() == [0, 4, 10, 15, 18, 23]
    assert w["cell_offs"].tolist() == [0, 0, 1, 4, 5, 7]
    assert w["sign"].tolist() == [1, 0, 0, 1, 0, 0, 1]
    assert w["col"].tolist() == [1, 0, 2, 1, 1, 0, 0]
    assert w["val"].tolist() == [5, 3, 4, 6, 2**64 - 1, 1, 2]
    for name, dt in _names(1):
        assert w[name].dtype == np.dtype(dt)


def test_exact_treg(engine):
    from jylis_amd.repo import RepoTREG
    big = bytes((i * 7 + 3) % 251 for i in range(70000))
    vals = [b"", b"8 bytes!", b"nine byte", big, b""]
    RepoTREG(engine).set(["v0", "v8", "v9", "big", "lost"], vals, [7, 7, 7, 7, 0])  # ("", 0) loses to the fresh register
    w = _dump(engine, 2)
    assert bytes(w["key_bytes"]) == b"v0v8v9biglost" and w["key_offs"].tolist() == [0, 2, 4, 6, 9, 13]
    assert w["ts"].tolist() == [7, 7, 7, 7, 0]
    assert w["val_offs"].tolist() == [0, 0, 8, 17, 70017, 70017]
    assert bytes(w["val_bytes"]) == b"".join(vals)


def test_exact_tlog(oracle_mod, engine):
    from jylis_amd.repo import RepoTLOG
    O = oracle_mod
    cmds = [("TRIMAT", "empty", 5), ("INS", "three", b"b", 4), ("INS", "three", b"a", 4), ("INS", "three", b"c", 9),
            ("INS", "cleared", b"gone", 3), ("CLR", "cleared")]
    want = O.Repo(O.TLOG, IDENT)
    want.tlog_trimat("empty", 5)
    for v, t in ((b"b", 4), (b"a", 4), (b"c", 9)):
        want.tlog_ins("three", v, t)
    want.tlog_ins("cleared", b"gone", 3)
    want.tlog_clr("cleared")
    RepoTLOG(engine).write(cmds)
    w = _dump(engine, 3)
    assert bytes(w["key_bytes"]) == b"emptythreecleared" and w["key_offs"].tolist() == [0, 5, 10, 17]
    # newest first; equal timestamps by value, descending (the log ascends by (ts, value))
    assert w["ent_offs"].tolist() == [0, 0, 3, 3]
    assert w["ts"].tolist() == [9, 4, 4] and bytes(w["val_bytes"]) == b"cba" and w["val_offs"].tolist() == [0, 1, 2, 3]
    assert w["cutoff"].tolist() == [5, 0, 4]  # CLR: the newest timestamp + 1
    assert_state_equal(3, _by_key(3, want.state()), _by_key(3, _table(engine, 3, w)))


def test_exact_ujson(engine):
    assert engine.replica_cols([IDENT, OTHER]).tolist() == [0, 1]
    kb, ko = _keys("two", "cleared", "never")
    batch = {"key_bytes": kb, "key_offs": ko, "el_offs": _u64(0, 2, 2, 2),
             "dots": _u64(_dot(0, 1), _dot(1, 1)), "elems": _u64(11, 12),
             "vv_offs": _u64(0, 2, 3, 3), "vv": _u64(_dot(0, 1), _dot(1, 1), _dot(0, 3)),
             "cloud_offs": _u64(0, 1, 1, 1), "cloud": _u64(_dot(1, 5))}
    engine.converge_wire(4, batch)
    _same_wire(4, batch, _dump(engine, 4))


# 3 ---------------------------------------------------------------------------
RANGES = [(0, 1), (0, 63), (0, 64), (1, 64), (3, 130), (192, 65), (0, 257), (256, 1), (257, 0)]


def _fill_257(eng, ctype):
    from jylis_amd.engine import encode_keys
    n = 257
    kb, ko = encode_keys([b"key-%03d" % i + b"." * (i % 11) for i in range(n)])
    if ctype == 2:
        vals = [bytes((i + j) % 256 for j in range((i * 7) % 23)) for i in range(n)]
        vb, vo = encode_keys(vals)
        eng.converge_wire(2, {"key_bytes": kb, "key_offs": ko, "ts": np.arange(1, n + 1, dtype=np.uint64),
                              "val_bytes": vb, "val_offs": vo})
        return
    nsigns = 1 if ctype == 0 else 2
    eng.replica_cols([IDENT, OTHER, THIRD])
    rng = np.random.default_rng(930 + ctype)
    dense = rng.integers(1, 2**63, (n, nsigns * 3), dtype=np.uint64) * (rng.random((n, nsigns * 3)) < 0.5)
    dense[::9] = 0  # keys with no cell
    cells = np.nonzero(dense)
    co = np.zeros(n + 1, np.uint64)
    co[1:] = np.cumsum((dense != 0).sum(1))
    eng.converge_wire(ctype, {"key_bytes": kb, "key_offs": ko, "cell_offs": co, "sign": (cells[1] // 3).astype(np.uint8),
                              "col": (cells[1] % 3).astype(np.uint16), "val": dense[cells]})


def _rows(ctype, w, s0, n):
    """records [s0, s0 + n) of a wire batch, as a wire batch"""
    def cut(offs, *arrs):
        o = np.asarray(w[offs]).astype(np.int64)
        lo, hi = int(o[s0]), int(o[s0 + n])
        return {offs: (o[s0:s0 + n + 1] - lo).astype(np.uint64), **{a: np.asarray(w[a])[lo:hi] for a in arrs}}
    out = cut("key_offs", "key_bytes")
    if ctype == 2:
        out.update(cut("val_offs", "val_bytes"), ts=np.asarray(w["ts"])[s0:s0 + n])
    else:
        out.update(cut("cell_offs", "sign", "col", "val"))
    return out


@pytest.mark.parametrize("ctype", [0, 1, 2])
def test_ranges_and_tile_edges(engine, ctype):
    from jylis_amd.engine import EngineError, WIRE_ARRAYS, WIRE_SIZES
    _fill_257(engine, ctype)
    assert engine.nkeys(ctype) == 257
    full = _dump(engine, ctype)
    if ctype != 2:
        assert 0 < len(full["val"]) and (np.diff(full["cell_offs"].astype(np.int64)) == 0).any()
    for s0, n in RANGES:
        _same_wire(ctype, _rows(ctype, full, s0, n), engine.state_wire(ctype, s0, n))
    # a range past the interned keys: JY_ERANGE, outputs untouched
    out = {name: np.full(64, 0xAB, dt) for name, dt, _, _ in WIRE_ARRAYS[ctype]}
    with pytest.raises(EngineError) as e:
        engine.state_wire_caps(ctype, 250, 8, [8] + [32] * (len(WIRE_SIZES[ctype]) - 1), out=out)
    assert e.value.code == -4
    for name, dt, _, _ in WIRE_ARRAYS[ctype]:
        assert (out[name] == np.full(64, 0xAB, dt)).all(), name


def _cells_from_export(eng, ctype, n):
    """the cells of slots [0, n) from the dense export: an independent reference"""
    ncols = eng.replica_count()
    dump = eng.counter_export(ctype, ncols, 0, n)  # [sign][col][slot]
    arr = dump.transpose(2, 0, 1).reshape(n, -1)
    slot, r = np.nonzero(arr)
    co = np.zeros(n + 1, np.uint64)
    co[1:] = np.cumsum((arr != 0).sum(1))
    return {"cell_offs": co, "sign": (r // ncols).astype(np.uint8), "col": (r % ncols).astype(np.uint16),
            "val": arr[slot, r]}


@pytest.mark.parametrize("ctype", [0, 1])
def test_counter_columns_at_and_past_the_mask_width(engine, ctype):
    """the column count grown at run time to exactly the tile writer's mask
    width (rows = signs x columns), then one column past it (the lane-per-key
    fallback), non-zero values in the first and the last column"""
    from jylis_amd.engine import encode_keys
    nsigns = ctype + 1
    width = engine.counter_state_mask_rows()
    assert width % nsigns == 0
    n = 70
    kb, ko = encode_keys([b"w%d" % i for i in range(n)])
    for ncols in (width // nsigns, width // nsigns + 1):
        engine.replica_cols([1000 + c for c in range(ncols)])
        assert engine.replica_count() == ncols
        last = ncols - 1
        key = np.repeat(np.arange(n), 2 * nsigns)
        sign = np.tile(np.repeat(np.arange(nsigns), 2), n).astype(np.uint8)
        col = np.tile(np.array([0, last] * nsigns), n).astype(np.uint16)
        val = (key * 1000 + ncols + sign).astype(np.uint64) * (key % 5 != 2)  # every fifth key stays 0 there
        co = np.arange(0, 2 * nsigns * n + 1, 2 * nsigns, dtype=np.uint64)
        engine.converge_wire(ctype, {"key_bytes": kb, "key_offs": ko, "cell_offs": co, "sign": sign, "col": col,
                                     "val": val})
        w = _dump(engine, ctype)
        ref = _cells_from_export(engine, ctype, n)
        assert int(ref["col"].max()) == last and len(ref["val"]) > n
        for name in ref:
            np.testing.assert_array_equal(ref[name], w[name], err_msg=f"{name} at {ncols} columns")
        for s0, k in ((1, 64), (33, 37)):
            _same_wire(ctype, _rows(ctype, w, s0, k), engine.state_wire(ctype, s0, k))


# 4 ---------------------------------------------------------------------------
@pytest.mark.parametrize("ctype", TYPES)
def test_two_phase_contract(oracle_mod, engine, ctype):
    from jylis_amd.engine import WIRE_ARRAYS, WIRE_SIZES
    from jylis_amd.repo import wire_to_host
    _populate(oracle_mod, ctype, engine, 940 + ctype)
    n = engine.nkeys(ctype)
    need, _ = engine.state_wire_caps(ctype, 0, n, [0] * len(WIRE_SIZES[ctype]))
    assert need[0] == n and need[1] > 0 and need[2] > 0, need
    for i in range(1, len(need)):
        if need[i] == 0:
            continue  # (an array this state leaves empty cannot be short)
        caps = list(need)
        caps[i] -= 1
        out = {name: np.full(need[idx] + plus, 0xAB, dt) for name, dt, idx, plus in WIRE_ARRAYS[ctype]}
        sizes, _ = engine.state_wire_caps(ctype, 0, n, caps, out=out)
        assert sizes == need, WIRE_SIZES[ctype][i]
        for name, dt, _, _ in WIRE_ARRAYS[ctype]:
            assert (out[name] == np.array(0xAB, dt)).all(), (WIRE_SIZES[ctype][i], name)
    sizes, host = engine.state_wire_caps(ctype, 0, n, need)
    assert sizes == need
    _same_wire(ctype, host, _dump(engine, ctype))
    sizes, dev = engine.state_wire_caps(ctype, 0, n, need, device=True)
    engine.sync()
    assert sizes == need and all(v.is_cuda for v in dev.values())
    _same_wire(ctype, host, wire_to_host(ctype, dev))
    # nslots == 0: the empty batch
    sizes, out = engine.state_wire_caps(ctype, n, 0, [0] * len(need))
    assert sizes == [0] * len(need)
    assert all(len(out[name]) == plus and not out[name].any() for name, _, _, plus in WIRE_ARRAYS[ctype])


# 5 ---------------------------------------------------------------------------
@pytest.mark.parametrize("ctype", TYPES)
def test_read_only(oracle_mod, engine, engine2, ctype):
    from jylis_amd.repo import REPOS
    O = oracle_mod
    ops = _random_ops(O, ctype, O.Repo(ctype, IDENT), np.random.default_rng(950 + ctype), 150)
    got, twin = REPOS[ctype](engine, IDENT), REPOS[ctype](engine2, IDENT)
    _apply(ctype, got, ops)
    _apply(ctype, twin, ops)
    before, pending = got.state(), _deltas_size(ctype, engine)
    assert pending > 0
    chunks = list(got.snapshot_wire(max_keys=5))
    assert sum(len(c["key_offs"]) - 1 for c in chunks) == engine.nkeys(ctype)
    assert _deltas_size(ctype, engine) == pending
    assert_state_equal(ctype, before, got.state())
    ta, tb = _flush_wire(ctype, got), _flush_wire(ctype, twin)
    assert set(ta) == set(tb) and len(ta["key_offs"]) - 1 == pending
    for k in ta:
        np.testing.assert_array_equal(np.asarray(ta[k]), np.asarray(tb[k]), err_msg=f"field {k}")
    assert_state_equal(ctype, before, got.state())


# 6 ---------------------------------------------------------------------------
@pytest.mark.parametrize("ctype", TYPES)
def test_restore(oracle_mod, engine, engine2, ctype):
    from jylis_amd.node import Node
    from jylis_amd.repo import REPOS
    _, a = _populate(oracle_mod, ctype, engine, 960 + ctype)
    dump = _dump(engine, ctype)
    ids = _col_ids(engine).tolist()
    # the engine-level path the repos use, into a fresh engine with A's columns
    assert engine2.replica_cols(ids).tolist() == list(range(len(ids)))
    engine2.converge_wire(ctype, dump)
    assert_state_equal(ctype, a.state(), REPOS[ctype](engine2).state())
    _same_wire(ctype, dump, _dump(engine2, ctype))
    # jy_node_*_converge on a one-shard node
    node = Node(1, "copy")
    try:
        assert [node.replica_col(i) for i in ids] == list(range(len(ids)))
        node.restore(ctype, [dump])
        node.sync()
        _same_wire(ctype, dump, _dump(node.engines[0], ctype))
    finally:
        node.close()
    # into A itself: idempotent
    before, pending = a.state(), _deltas_size(ctype, engine)
    engine.converge_wire(ctype, dump)
    assert_state_equal(ctype, before, a.state())
    assert _deltas_size(ctype, engine) == pending
    _same_wire(ctype, dump, _dump(engine, ctype))


# 7 ---------------------------------------------------------------------------
def test_ujson_inplace_layout(oracle_mod, engine, engine2):
    from jylis_amd.repo import RepoUJSON
    O = oracle_mod
    engine.ujson_set_inplace(4)
    engine2.ujson_set_inplace(0)
    for e in (engine, engine2):
        e.replica_cols([IDENT, OTHER])
    writers = [O.Repo(O.UJSON, IDENT), O.Repo(O.UJSON, OTHER)]
    want, a, b = O.Repo(O.UJSON, 99), RepoUJSON(engine), RepoUJSON(engine2)
    for rnd in range(6):  # fresh inserts, batch after batch: "long" passes the threshold and keeps growing
        r = writers[rnd % 2]
        for e in range(3):
            r.ujson_ins("long", 10 * rnd + e + 1)
        if rnd == 0:
            r.ujson_ins("short", 99)
        t = r.flush().table()
        for repo in (want, a, b):
            (repo.converge if repo is want else repo.converge_deltas)(t)
    st = engine.ujson_stats()
    assert st["promoted"] > 0 and engine2.ujson_stats()["promoted"] == 0, st
    w = _dump(engine, 4)
    assert np.diff(w["el_offs"].astype(np.int64)).tolist() == [18, 1]
    _same_wire(4, _dump(engine2, 4), w)
    _assert_equals_oracle(4, want, _table(engine, 4, w))


# 8 ---------------------------------------------------------------------------
def test_tlog_after_a_spill(oracle_mod):
    from jylis_amd import synth as S
    from jylis_amd.engine import Engine
    from jylis_amd.repo import RepoTLOG
    O = oracle_mod
    eng = Engine(device=0, entry_capacity=1024)
    try:
        st, dl = S.tlog_tables(4000, seed=S.BASE_SEED + 41, rounds=6, mean_state=4, mean_delta=3)
        want, got = O.Repo(O.TLOG), RepoTLOG(eng)
        for b in [st] + dl:
            want.converge(b)
            got.converge_deltas(b)
        chunks = list(eng.snapshot(O.TLOG, max_keys=1500))  # settles the merges in flight, spilled ones included
        assert eng.tlog_stats()["spills"] > 0, eng.tlog_stats()
        assert len(chunks) == -(-eng.nkeys(O.TLOG) // 1500)
        from jylis_amd.repo import concat_tables, wire_to_table
        table = concat_tables([wire_to_table(O.TLOG, c, ()) for c in chunks])
        _assert_equals_oracle(O.TLOG, want, table)
    finally:
        eng.close()


# 9 ---------------------------------------------------------------------------
def test_node_resharding(oracle_mod):
    from jylis_amd.engine import key_owner
    from jylis_amd.node import Node
    from jylis_amd.repo import REPOS
    O = oracle_mod
    A, B = Node(2, "copy"), Node(3, "copy")

    def rows_of(node, ctype):
        rows = {}
        for sh, eng in enumerate(node.engines):
            part = dict(split_rows(ctype, REPOS[ctype](eng).state()))
            assert all(key_owner(k, node.S) == sh for k in part)
            rows.update(part)
        return rows

    try:
        B.replica_col(THIRD)  # B's columns differ from A's
        for ctype in TYPES:
            for b in random_history(O, ctype, seed=990 + ctype, nrep=3, nops=300, nkeys=40):
                A.converge_table(ctype, b)
        A.sync()
        for ctype in TYPES:
            B.restore(ctype, A.snapshot(ctype, max_keys=16), col_ids=A.replica_ids())
        B.sync()
        for ctype in TYPES:
            ra, rb = rows_of(A, ctype), rows_of(B, ctype)
            assert 30 <= len(ra) <= 40 and set(ra) == set(rb)
            assert_state_equal(ctype, join_rows(ctype, ra), join_rows(ctype, rb))
    finally:
        A.close()
        B.close()


# 10 --------------------------------------------------------------------------
def test_files(oracle_mod, engine, engine2, tmp_path):
    from jylis_amd import snapshot
    from jylis_amd.repo import REPOS
    wants = {ctype: _populate(oracle_mod, ctype, engine, 1000 + ctype)[0] for ctype in TYPES}
    assert engine2.replica_col(0xDEAD) == 0  # a different id first: every column differs
    man = snapshot.save(engine, str(tmp_path), max_keys=5)
    assert man["replica_ids"] == _col_ids(engine).tolist()
    assert len(man["chunks"]) == sum(-(-engine.nkeys(t) // 5) for t in TYPES)
    snapshot.load(str(tmp_path), engine2)
    assert _col_ids(engine2).tolist() == [0xDEAD] + man["replica_ids"]
    for ctype in TYPES:
        st = REPOS[ctype](engine2).state()
        assert_state_equal(ctype, REPOS[ctype](engine).state(), st)
        _assert_equals_oracle(ctype, wants[ctype], st)
