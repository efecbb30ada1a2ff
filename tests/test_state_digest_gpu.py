"""The state digest on the GPU (jy_*_state_digest), its key-hash buckets, the
slots of buckets (jy_state_bucket_slots), the slot-list dumps
(jy_*_state_wire_slots) and the repair path built on them -- against the CPU
oracle's canonical digests and tests/digest_ref.py."""
import numpy as np
import pytest

import digest_ref as R
from helpers import assert_state_equal, join_rows, split_rows
from test_state_wire_gpu import (IDENT, OTHER, THIRD, TYPES, _col_ids, _dump, _populate, _same_wire, _table,
                                 engine2)  # noqa: F401  (engine2: a fixture)

pytestmark = pytest.mark.gpu

IDS = [IDENT, OTHER, THIRD]
SEED = 1100  # histories for which the oracle holds every key (checked in test 1 before any comparison)


def _t4(x):
    """four digest words as Python ints (an array row, or the oracle's tuple)"""
    return tuple(int(v) for v in (x.ravel() if isinstance(x, np.ndarray) else x))[:4]


def _sum(d):
    with np.errstate(over="ignore"):
        return _t4(np.asarray(d, np.uint64).sum(axis=0, dtype=np.uint64))


def _add(a, b):
    with np.errstate(over="ignore"):
        return a + b


def _keys(n):
    return [b"key-%03d" % i + b"." * (i % 11) for i in range(n)]


def _wire(ctype, keys, seed):
    """a wire batch over source columns 0..2 (= IDS): random content for `keys`"""
    from jylis_amd.engine import encode_keys
    rng = np.random.default_rng(seed)
    n = len(keys)
    kb, ko = encode_keys(list(keys))
    w = {"key_bytes": kb, "key_offs": ko}
    offs = lambda counts: np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    if ctype in (0, 1):
        ns = ctype + 1
        dense = rng.integers(1, 2**63, (n, ns * 3), dtype=np.uint64) * (rng.random((n, ns * 3)) < 0.5)
        dense[::9] = 0
        _, r = np.nonzero(dense)
        w.update(cell_offs=offs((dense != 0).sum(1)), sign=(r // 3).astype(np.uint8), col=(r % 3).astype(np.uint16),
                 val=dense[np.nonzero(dense)])
    elif ctype == 2:
        vals = [bytes(rng.integers(0, 256, int(rng.choice([0, 1, 8, 9, 24])), dtype=np.uint8)) for _ in range(n)]
        vb, vo = encode_keys(vals)
        w.update(ts=rng.integers(1, 1000, n).astype(np.uint64), val_bytes=vb, val_offs=vo)
    elif ctype == 3:
        cnt = rng.integers(0, 5, n)
        ts = np.concatenate([np.sort(rng.choice(np.arange(10, 1000), int(c), replace=False))[::-1] for c in cnt]
                            + [np.zeros(0, np.int64)]).astype(np.uint64)
        vals = [bytes(rng.integers(0, 256, int(rng.choice([0, 3, 8, 9, 20])), dtype=np.uint8)) for _ in range(len(ts))]
        vb, vo = encode_keys(vals) if vals else (np.zeros(0, np.uint8), np.zeros(1, np.uint64))
        w.update(cutoff=(rng.integers(0, 10, n) * (rng.random(n) < 0.3)).astype(np.uint64), ent_offs=offs(cnt), ts=ts,
                 val_bytes=vb, val_offs=vo)
    else:
        dots, vv, cloud, ne, nv, nc = [], [], [], [], [], []
        for _ in range(n):
            a, b, c = len(dots), len(vv), len(cloud)
            for col in range(3):
                k = int(rng.integers(0, 4))
                if k:
                    dots += [(col << 48) | s for s in range(1, k + 1) if rng.random() < 0.8]
                    vv.append((col << 48) | k)
                    if rng.random() < 0.3:
                        cloud.append((col << 48) | (k + 2))
            ne.append(len(dots) - a), nv.append(len(vv) - b), nc.append(len(cloud) - c)
        u = lambda x: np.array(x, np.uint64)
        w.update(el_offs=offs(ne), dots=u(dots), elems=rng.integers(1, 2**62, len(dots)).astype(np.uint64),
                 vv_offs=offs(nv), vv=u(vv), cloud_offs=offs(nc), cloud=u(cloud))
    return w


def _remap(ctype, w, col_map):
    from jylis_amd.snapshot import remap_columns, sort_dots
    return sort_dots(ctype, remap_columns(ctype, w, col_map))


def _fill(eng, ctype, n=257, seed=7, ids=IDS, keys=None):
    """`n` keys of random content into eng, its columns registered in the order of `ids`"""
    cols = eng.replica_cols(ids).tolist()
    col_map = [cols[ids.index(i)] for i in IDS]
    eng.converge_wire(ctype, _remap(ctype, _wire(ctype, _keys(n) if keys is None else keys, seed), col_map))


def _ref(eng, ctype, B, w=None):
    return R.wire_digest(ctype, _dump(eng, ctype) if w is None else w, _col_ids(eng), B)


# 1 ---------------------------------------------------------------------------
@pytest.mark.parametrize("ctype", TYPES)
def test_oracle_parity(oracle_mod, engine, ctype):
    O = oracle_mod
    want, _ = _populate(O, ctype, engine, SEED)
    n = engine.nkeys(ctype)
    assert int(O.digest_repo(want)[1]) == n  # the oracle holds every key the engine interned
    got = engine.digest(ctype, 1)
    assert got.shape == (1, 4) and got.dtype == np.uint64
    w = _dump(engine, ctype)
    if ctype in (0, 1):
        ncols = engine.replica_count()
        names = engine.key_names(ctype, 0, n)  # jy_keys_export
        from jylis_amd.engine import encode_keys
        kb, ko = encode_keys(names)
        ref = O.digest_counter_dense(kb, ko, _col_ids(engine), engine.counter_export(ctype, ncols, 0, n))
    else:
        ref = O.digest_table(ctype, _table(engine, ctype, w))
    assert _t4(got) == _t4(ref)
    assert _t4(got) == _t4(O.digest_repo(want))


# 2, 3, 9, 10 -----------------------------------------------------------------
RANGES = [(0, 0), (0, 1), (1, 63), (63, 2), (64, 64), (255, 2), (256, 1), (0, 257)]


@pytest.mark.parametrize("ctype", TYPES)
def test_buckets(engine, ctype):
    _fill(engine, ctype)
    w = _dump(engine, ctype)
    for B in (1, 2, 64, 4096, 1 << 20):
        d = engine.digest(ctype, B)
        assert d.shape == (B, 4)
        np.testing.assert_array_equal(d, _ref(engine, ctype, B, w), err_msg=f"B = {B}")
        assert int(d[:, 1].sum()) == 257
        if B == 4096:
            assert (d[:, 1] == 0).any() and not d[d[:, 1] == 0].any()
    # chunked (max_keys) and whole-range calls agree, on the host and on the device
    whole = engine.digest(ctype, 64)
    np.testing.assert_array_equal(engine.digest(ctype, 64, max_keys=100), whole)
    dev = engine.digest(ctype, 64, max_keys=100, device=True)
    engine.sync()
    np.testing.assert_array_equal(dev.cpu().numpy().view(np.uint64), whole)


def _rows_of(ctype, w, idx):
    """records idx (ascending) of a wire batch, as a wire batch"""
    from jylis_amd.engine import WIRE_ARRAYS
    idx = np.asarray(idx, np.int64)
    out = {}
    per_item = {"key_offs": ("key_bytes",), "cell_offs": ("sign", "col", "val"), "el_offs": ("dots", "elems"),
                "vv_offs": ("vv",), "cloud_offs": ("cloud",), "ent_offs": ("ts",) if ctype == 3 else ()}
    def cut(offs, arrs, sel):
        o = np.asarray(w[offs]).astype(np.int64)
        take = np.concatenate([np.arange(o[i], o[i + 1]) for i in sel] + [np.zeros(0, np.int64)]).astype(np.int64)
        out[offs] = np.concatenate([[0], np.cumsum(o[sel + 1] - o[sel])]).astype(np.uint64)
        for a in arrs:
            out[a] = np.asarray(w[a])[take]
        return take
    for offs, arrs in per_item.items():
        if offs in w and offs != "val_offs":
            took = cut(offs, arrs, idx)
            if offs == "ent_offs":
                cut("val_offs", ("val_bytes",), took)
    if ctype == 2:
        cut("val_offs", ("val_bytes",), idx)
        out["ts"] = np.asarray(w["ts"])[idx]
    if ctype == 3:
        out["cutoff"] = np.asarray(w["cutoff"])[idx]
    return {name: out[name] for name, _, _, _ in WIRE_ARRAYS[ctype]}


@pytest.mark.parametrize("ctype", TYPES)
def test_ranges(engine, ctype):
    _fill(engine, ctype)
    ids = _col_ids(engine)
    got = {}
    for s0, n in RANGES:
        got[s0, n] = engine.digest(ctype, 64, s0, n)
        np.testing.assert_array_equal(got[s0, n], R.wire_digest(ctype, engine.state_wire(ctype, s0, n), ids, 64),
                                      err_msg=f"range {s0, n}")
    assert not got[0, 0].any()
    # adjacent ranges sum, wrapping, to their union
    np.testing.assert_array_equal(_add(got[0, 1], got[1, 63]), engine.digest(ctype, 64, 0, 64))
    parts = _add(_add(engine.digest(ctype, 64, 0, 64), got[64, 64]), engine.digest(ctype, 64, 128, 129))
    np.testing.assert_array_equal(parts, got[0, 257])


@pytest.mark.parametrize("ctype", TYPES)
def test_contracts(engine, ctype):
    from jylis_amd import _lib
    from jylis_amd.engine import EngineError
    from test_flush_wire_gpu import _deltas_size
    _fill(engine, ctype)
    before, pending = _dump(engine, ctype), _deltas_size(ctype, engine)
    host = engine.digest(ctype, 64)
    dev = engine.digest(ctype, 64, device=True)
    engine.sync()
    np.testing.assert_array_equal(host, dev.cpu().numpy().view(np.uint64))
    big = engine.digest(ctype, 4096, device=True)  # (the direct global-atomic form)
    engine.sync()
    np.testing.assert_array_equal(engine.digest(ctype, 4096), big.cpu().numpy().view(np.uint64))
    _same_wire(ctype, before, _dump(engine, ctype))  # read-only
    assert _deltas_size(ctype, engine) == pending
    for args, code in (((64, 250, 8), _lib.JY_ERANGE), ((64, 258, 0), _lib.JY_ERANGE), ((0, 0, 1), _lib.JY_EINVAL),
                       ((3, 0, 1), _lib.JY_EINVAL), ((1 << 21, 0, 1), _lib.JY_EINVAL)):
        with pytest.raises(EngineError) as e:
            engine.digest_range(ctype, *args)
        assert e.value.code == code and str(e.value), args
        assert engine.lib.jy_last_error(engine.h)
    if ctype == 2:
        out = np.zeros(4, np.uint64)
        rc = engine.lib.jy_counter_state_digest(engine.h, 2, 0, 0, 1, out.ctypes.data, 0)
        assert rc == _lib.JY_ETYPE and engine.lib.jy_last_error(engine.h)


@pytest.mark.parametrize("ctype", TYPES)
def test_bucket_slots_and_slot_list_dumps(engine, ctype):
    from jylis_amd import _lib
    from jylis_amd.engine import EngineError, WIRE_SIZES
    _fill(engine, ctype)
    full = _dump(engine, ctype)
    bk = np.array(R.key_buckets(full, 64))
    pick = [3, 17, 40, 63, int(bk[0])]
    want = np.nonzero(np.isin(bk, pick))[0]
    got = engine.bucket_slots(ctype, 64, pick)
    assert got.dtype == np.uint32 and got.tolist() == want.tolist() and 0 < len(want) < 257
    assert engine.bucket_slots(ctype, 64, range(64)).tolist() == list(range(257))
    assert engine.bucket_slots(ctype, 64, []).tolist() == []
    sub = engine.bucket_slots(ctype, 64, pick, 100, 100)
    assert sub.tolist() == [s for s in want.tolist() if 100 <= s < 200]
    # a short cap writes only n_out
    import ctypes as C
    bits = np.zeros(1, np.uint64)
    for b in pick:
        bits[0] |= np.uint64(1 << b)
    out, k = np.full(300, 0xABABABAB, np.uint32), C.c_uint64(0)
    assert engine.lib.jy_state_bucket_slots(engine.h, ctype, 0, 257, 64, bits.ctypes.data, len(want) - 1,
                                            out.ctypes.data, C.byref(k), 0) == 0
    assert k.value == len(want) and (out == 0xABABABAB).all()
    # the list dump = the rows of the full dump the list picks
    for slots in (want, np.arange(257), np.array([256]), np.array([0, 2, 255])):
        _same_wire(ctype, _rows_of(ctype, full, slots), engine.state_wire_slots(ctype, slots))
    _same_wire(ctype, engine.state_wire(ctype, 5, 0), engine.state_wire_slots(ctype, np.zeros(0, np.uint32)))
    need, _ = engine.state_wire_slots_caps(ctype, want, [0] * len(WIRE_SIZES[ctype]))
    dev = engine.state_wire_slots(ctype, want, device=True)
    engine.sync()
    from jylis_amd.repo import wire_to_host
    _same_wire(ctype, _rows_of(ctype, full, want), wire_to_host(ctype, dev))
    sizes = (C.c_uint64 * 8)()  # a null list with n > 0
    fn = getattr(engine.lib, {0: "jy_counter", 1: "jy_counter", 2: "jy_treg", 3: "jy_tlog", 4: "jy_ujson"}[ctype]
                 + "_state_wire_slots")
    nargs = len(_lib.SIGNATURES[fn.__name__][1])
    head = [engine.h] + ([ctype] if ctype < 2 else []) + [3, None, 0]
    assert fn(*head, *([0] * (nargs - len(head) - 2)), sizes, 0) == _lib.JY_EINVAL
    for bad, code in (([5, 4], _lib.JY_EINVAL), ([4, 4], _lib.JY_EINVAL), ([0, 257], _lib.JY_ERANGE)):
        with pytest.raises(EngineError) as e:
            engine.state_wire_slots(ctype, np.array(bad))
        assert e.value.code == code and str(e.value), bad


@pytest.mark.parametrize("ncols", [64, 65])
def test_counter_list_dump_at_both_writers(engine, ncols):
    """PNCOUNT at 128 rows (the tile writer) and 130 (the lane writer)"""
    from jylis_amd.engine import encode_keys
    engine.replica_cols([1000 + c for c in range(ncols)])
    n = 70
    kb, ko = encode_keys([b"w%d" % i for i in range(n)])
    key = np.repeat(np.arange(n), 4)
    engine.converge_wire(1, {"key_bytes": kb, "key_offs": ko, "cell_offs": np.arange(0, 4 * n + 1, 4, dtype=np.uint64),
                             "sign": np.tile(np.array([0, 0, 1, 1], np.uint8), n),
                             "col": np.tile(np.array([0, ncols - 1] * 2, np.uint16), n),
                             "val": (key * 1000 + 7).astype(np.uint64) * (key % 5 != 2)})
    full = _dump(engine, 1)
    for slots in (np.arange(0, 70, 3), np.array([1, 2, 33, 34, 35, 69])):
        _same_wire(1, _rows_of(1, full, slots), engine.state_wire_slots(1, slots))
    np.testing.assert_array_equal(engine.digest(1, 64), _ref(engine, 1, 64, full))


# 4 ---------------------------------------------------------------------------
@pytest.mark.parametrize("ctype", TYPES)
def test_slot_and_column_independence(engine, engine2, ctype):
    from jylis_amd.engine import encode_keys
    _fill(engine, ctype, n=60)
    engine2.intern(ctype, encode_keys(_keys(60)[::-1]))  # the same keys, slots in reverse order
    _fill(engine2, ctype, n=60, ids=[THIRD, IDENT, OTHER])
    assert engine.key_names(ctype, 0, 1) != engine2.key_names(ctype, 0, 1)
    a, b = engine.digest(ctype, 64), engine2.digest(ctype, 64)
    assert a[:, 1].sum() == 60
    np.testing.assert_array_equal(a, b)


# 5 ---------------------------------------------------------------------------
def _one(ctype, key, **arrs):
    from jylis_amd.engine import encode_keys
    kb, ko = encode_keys([key])
    u = lambda x: np.array(x, np.uint64)
    w = {"key_bytes": kb, "key_offs": ko}
    if ctype in (0, 1):
        w.update(cell_offs=u([0, 1]), sign=np.array([arrs["sign"]], np.uint8), col=np.array([arrs["col"]], np.uint16),
                 val=u([arrs["val"]]))
    elif ctype == 2:
        v = arrs["value"]
        w.update(ts=u([arrs["ts"]]), val_bytes=np.frombuffer(v, np.uint8), val_offs=u([0, len(v)]))
    elif ctype == 3:
        ents = arrs.get("ents", [])
        vb = b"".join(v for _, v in ents)
        w.update(cutoff=u([arrs.get("cutoff", 0)]), ent_offs=u([0, len(ents)]), ts=u([t for t, _ in ents]),
                 val_bytes=np.frombuffer(vb, np.uint8), val_offs=u(np.cumsum([0] + [len(v) for _, v in ents])))
    else:
        w.update(el_offs=u([0, len(arrs.get("dots", []))]), dots=u(arrs.get("dots", [])),
                 elems=u(arrs.get("elems", [])), vv_offs=u([0, len(arrs.get("vv", []))]), vv=u(arrs.get("vv", [])),
                 cloud_offs=u([0, len(arrs.get("cloud", []))]), cloud=u(arrs.get("cloud", [])))
    return w


FIELD_CASES = {
    "counter cell": (0, dict(sign=0, col=1, val=2**63 + 5)),
    "counter cell 2^64 - 1": (1, dict(sign=1, col=2, val=2**64 - 1)),
    "treg timestamp": (2, "ts"),
    "treg value byte": (2, "byte"),
    "tlog cutoff": (3, dict(cutoff=10)),  # above every cutoff of _wire, below every entry
    "tlog entry": (3, dict(ents=[(5000, b"one more entry")])),
    "ujson element": (4, dict(dots=[(1 << 48) | 900], elems=[77], cloud=[(1 << 48) | 900])),
    "ujson vv entry": (4, dict(vv=[(2 << 48) | 5000])),
    "ujson cloud dot": (4, dict(cloud=[(0 << 48) | 7000])),
}


@pytest.mark.parametrize("case", sorted(FIELD_CASES))
def test_every_field_is_seen_in_its_bucket_only(engine, case):
    ctype, delta = FIELD_CASES[case]
    _fill(engine, ctype, n=60)
    key = _keys(60)[23]
    if ctype == 2:  # a register with a value byte below 0xFF: one field changed so that the delta wins
        full = _dump(engine, 2)
        vo = full["val_offs"].astype(np.int64)
        s = next(i for i in range(60) if vo[i + 1] > vo[i] and int(full["val_bytes"][vo[i + 1] - 1]) < 0xFF)
        key, val, ts = _keys(60)[s], bytes(full["val_bytes"][vo[s]:vo[s + 1]]), int(full["ts"][s])
        # (equal timestamps: the larger value wins; the length stays)
        delta = dict(ts=ts + 1, value=val) if delta == "ts" else dict(ts=ts, value=val[:-1] + bytes([val[-1] + 1]))
        assert len(delta["value"]) == len(val)
    twin = engine.digest(ctype, 64)
    engine.converge_wire(ctype, _one(ctype, key, **delta))
    now = engine.digest(ctype, 64)
    rows = np.nonzero((twin != now).any(axis=1))[0].tolist()
    assert rows == [R.bucket(R.dbytes(key), 64)], case
    assert twin[rows[0], 0] != now[rows[0], 0] and twin[rows[0], 1] == now[rows[0], 1]
    np.testing.assert_array_equal(now, _ref(engine, ctype, 64))


# 6 ---------------------------------------------------------------------------
EDGE_VALUES = [b"", b"\x00", b"\x80" * 8, b"\xff" * 9, bytes([0, 0x80, 0xFF] * 8), bytes([0xFF, 0, 0x80] * 100)]
EDGE_KEYS = [b"k", b"K" * 200, b"\x80\xfe\xffkey\x00\x81", b"plain", b"other", b"sixth"]


def _check_against_the_oracle(O, eng, ctype):
    w = _dump(eng, ctype)
    got = eng.digest(ctype, 1)
    assert _t4(got) == _t4(O.digest_table(ctype, _table(eng, ctype, w)))
    np.testing.assert_array_equal(eng.digest(ctype, 64), _ref(eng, ctype, 64, w))
    return w


def test_byte_edges_treg(oracle_mod, engine):
    from jylis_amd.repo import RepoTREG
    RepoTREG(engine).set(EDGE_KEYS, EDGE_VALUES, [7] * 6)
    w = _check_against_the_oracle(oracle_mod, engine, 2)
    assert np.diff(w["val_offs"].astype(np.int64)).tolist() == [0, 1, 8, 9, 24, 300]


def test_byte_edges_tlog(oracle_mod, engine):
    cut = _one(3, b"cut-only", cutoff=9)
    engine.converge_wire(3, cut)
    for key, m in zip(EDGE_KEYS[:3], (1, 70, 300)):
        ents = [(10000 - j, EDGE_VALUES[(j + m) % 6]) for j in range(m)]  # newest first
        engine.converge_wire(3, _one(3, key, ents=ents))
    w = _check_against_the_oracle(oracle_mod, engine, 3)
    assert np.diff(w["ent_offs"].astype(np.int64)).tolist() == [0, 1, 70, 300] and w["cutoff"].tolist() == [9, 0, 0, 0]


def test_byte_edges_ujson(oracle_mod, engine):
    engine.replica_cols(IDS)
    dots = [(c << 48) | s for c in range(3) for s in range(1, 101)]
    engine.converge_wire(4, _one(4, EDGE_KEYS[1], dots=dots, elems=list(range(1, 301)),
                                 vv=[(c << 48) | 100 for c in range(3)]))
    engine.converge_wire(4, _one(4, EDGE_KEYS[2], cloud=[(1 << 48) | 9]))
    w = _check_against_the_oracle(oracle_mod, engine, 4)
    assert np.diff(w["el_offs"].astype(np.int64)).tolist() == [300, 0]


# 7 ---------------------------------------------------------------------------
def test_ujson_inplace_layout(oracle_mod, engine, engine2):
    from jylis_amd.repo import RepoUJSON
    O = oracle_mod
    engine.ujson_set_inplace(3)
    engine2.ujson_set_inplace(0)
    for e in (engine, engine2):
        e.replica_cols([IDENT, OTHER])
    writers = [O.Repo(O.UJSON, IDENT), O.Repo(O.UJSON, OTHER)]
    want, a, b = O.Repo(O.UJSON, 99), RepoUJSON(engine), RepoUJSON(engine2)
    for rnd in range(6):
        r = writers[rnd % 2]
        for e in range(3):
            r.ujson_ins("long", 10 * rnd + e + 1)
        if rnd == 0:
            r.ujson_ins("short", 99)
        t = r.flush().table()
        for repo in (want, a, b):
            (repo.converge if repo is want else repo.converge_deltas)(t)
    assert engine.ujson_stats()["promoted"] > 0 and engine2.ujson_stats()["promoted"] == 0
    assert int(O.digest_repo(want)[1]) == engine.nkeys(4)
    np.testing.assert_array_equal(a.digest(64), b.digest(64))
    assert _t4(a.digest(1)) == _t4(O.digest_repo(want))


def test_tlog_after_a_spill(oracle_mod):
    from jylis_amd import synth as S
    from jylis_amd.engine import Engine
    from jylis_amd.repo import RepoTLOG
    O = oracle_mod
    eng, twin = Engine(device=0, entry_capacity=1024), Engine(device=0)
    try:
        st, dl = S.tlog_tables(4000, seed=S.BASE_SEED + 41, rounds=6, mean_state=4, mean_delta=3)
        want, got, other = O.Repo(O.TLOG), RepoTLOG(eng), RepoTLOG(twin)
        for b in [st] + dl:
            want.converge(b)
            got.converge_deltas(b)
            other.converge_deltas(b)
        d = got.digest(64, max_keys=1500)  # settles the merges in flight, spilled ones included
        assert eng.tlog_stats()["spills"] > 0, eng.tlog_stats()
        np.testing.assert_array_equal(d, other.digest(64))
        assert int(O.digest_repo(want)[1]) == eng.nkeys(3)
        assert _sum(d) == _t4(O.digest_repo(want))
    finally:
        eng.close()
        twin.close()


# 8 ---------------------------------------------------------------------------
@pytest.mark.parametrize("ncols", [1, 64, 65])
def test_counter_widths(oracle_mod, ncols):
    """more ids registered than counter_columns allocates: the digest reads
    min(registered, allocated) columns, and the rest hold nothing"""
    from jylis_amd.engine import Engine, encode_keys
    O = oracle_mod
    eng = Engine(device=0, counter_columns=ncols)
    try:
        eng.replica_cols([5000 + 3 * c for c in range(ncols + 6)])
        n = 40
        kb, ko = encode_keys([b"c%d" % i for i in range(n)])
        cols = sorted({0, ncols // 2, ncols - 1})
        m = len(cols)
        key = np.repeat(np.arange(n), 2 * m)
        eng.converge_wire(1, {"key_bytes": kb, "key_offs": ko,
                              "cell_offs": np.arange(0, 2 * m * n + 1, 2 * m, dtype=np.uint64),
                              "sign": np.tile(np.repeat(np.arange(2), m), n).astype(np.uint8),
                              "col": np.tile(np.array(cols * 2, np.uint16), n),
                              "val": (key * 977 + 13).astype(np.uint64) * (key % 4 != 1)})
        assert eng.replica_count() == ncols + 6
        dense = eng.counter_export(1, ncols, 0, n)  # (the columns past it were never allocated)
        want = O.digest_counter_dense(kb, ko, _col_ids(eng), dense)
        assert _t4(eng.digest(1, 1)) == _t4(want) and int(want[2]) > 0
        assert _sum(eng.digest(1, 64)) == _t4(want)
    finally:
        eng.close()


# 11 --------------------------------------------------------------------------
def _node_fill(node, ctype, keys, seed, ids):
    cols = [node.replica_col(i) for i in ids]
    col_map = [cols[ids.index(i)] for i in IDS]
    node.converge_wire(ctype, _remap(ctype, _wire(ctype, keys, seed), col_map))


def _node_rows(node, ctype):
    from jylis_amd.repo import wire_to_table
    rows, ids = {}, node.replica_ids()
    for _, w in node.snapshot(ctype, max_keys=100):
        rows.update(dict(split_rows(ctype, wire_to_table(ctype, w, ids))))
    for row in rows.values():  # a counter's cells come in column order: by replica id instead
        for pre in {0: ("",), 1: ("p_", "n_")}.get(ctype, ()):
            order = np.argsort(row[pre + "ids"], kind="stable")
            row[pre + "ids"], row[pre + "vals"] = row[pre + "ids"][order], row[pre + "vals"][order]
    return rows


@pytest.mark.parametrize("ctype", TYPES)
def test_node_digest_and_repair(ctype):
    from jylis_amd import antientropy
    from jylis_amd.node import Node
    keys = _keys(257)
    h2, h3 = keys[10:13] + [b"only-on-a"], keys[200:203] + [b"only-on-b"]
    # on the CPU: the keys H2 and H3 touch leave buckets clean at B = 64
    touched = {R.bucket(R.dbytes(k), 64) for k in h2 + h3}
    all_b = {R.bucket(R.dbytes(k), 64) for k in keys}
    assert len(h2 + h3) <= 8 and len(all_b - touched) >= 1
    A, B = Node(2, "copy"), Node(3, "copy")
    try:
        _node_fill(A, ctype, keys, 7, IDS)
        _node_fill(B, ctype, keys, 7, [THIRD, OTHER, IDENT])
        A.sync(), B.sync()
        da, db = A.digest(ctype, 64), B.digest(ctype, 64)  # S = 2 and S = 3, the same history
        assert int(da[:, 1].sum()) == 257
        np.testing.assert_array_equal(da, db)
        _node_fill(A, ctype, h2, 8, IDS)
        _node_fill(B, ctype, h3, 9, [THIRD, OTHER, IDENT])
        A.sync(), B.sync()
        da, db = A.digest(ctype, 64), B.digest(ctype, 64)
        bad = antientropy.diff(da, db)
        assert 0 < len(bad) <= len(touched) and set(bad.tolist()) <= touched
        expect = int(da[bad, 1].sum() + db[bad, 1].sum())
        res = antientropy.sync(A, B, ctype, 64)
        assert res == {"rounds": 1, "buckets": len(bad), "keys_sent": expect}
        assert expect < 257
        np.testing.assert_array_equal(A.digest(ctype, 64), B.digest(ctype, 64))
        ra, rb = _node_rows(A, ctype), _node_rows(B, ctype)
        assert len(ra) == 259 and set(ra) == set(rb)
        assert_state_equal(ctype, join_rows(ctype, ra), join_rows(ctype, rb))
    finally:
        A.close()
        B.close()
