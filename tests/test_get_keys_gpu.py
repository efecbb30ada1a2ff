"""Keyed batch reads on the GPU (jy_treg_get_keys, jy_tlog_get_keys,
jy_counter_get_keys; k_get.hip) against tests/get_ref.py over the CPU oracle's
state, byte-exact.

The TLOG state (about 2,000 keys) is built once, by converging and writing
through the existing repo against the oracle: logs of 0 (after CLR), 1, 63,
64, 65, 255, 256, 257 and 5,000 entries -- the wave and workgroup edges of the
entry gather's 256-thread tile, and one log spread over many tiles -- among
short ones; keys of 1, 8, 16, 17 and 40 bytes; values of 0, 1, 8, 9, 16, 17
and 300 bytes; equal timestamps; raised cutoffs (moved segment bases); merges
that rebuilt and inserted in place; a pool small enough to compact; an arena
collection at the end (rewritten handles)."""
import numpy as np
import pytest

import get_ref
import resp_ref
from get_ref import ALL

pytestmark = pytest.mark.gpu

IDENT = 0x5EED_0000_0000_6E75
VLENS = (0, 1, 8, 9, 16, 17, 300)
# log length -> key (the key lengths 1, 8, 16, 17 and 40 bytes among them)
SPECIAL = {1: b"a", 63: b"len8key_", 64: b"sixteen-byte-key", 65: b"seventeen-bytes-k", 255: b"k40-" + b"y" * 36,
           256: b"log256", 257: b"log257", 5000: b"hot5000"}
CLEARED = b"cleared"
MISSING = (b"nobody", b"k9999", b"", b"seventeen-bytes-K")


def _val(j):
    n = VLENS[j % len(VLENS)]
    return ((b"pfx-%05d-" % j) * 31)[:n]


def _ts(j):
    return 1000 + j - (1 if j % 16 == 1 else 0)  # entry 16 q + 1 ties with entry 16 q: two values at one timestamp


@pytest.fixture(scope="module")
def world(oracle_mod):
    """(engine, repo, the oracle's state table, its keys) -- read-only for the tests"""
    from jylis_amd.engine import Engine
    from jylis_amd.repo import RepoTLOG
    O = oracle_mod
    assert [len(k) for k in SPECIAL.values()][:5] == [1, 8, 16, 17, 40]
    rng = np.random.default_rng(20)
    eng = Engine(device=0, entry_capacity=1024)
    want, got = O.Repo(O.TLOG, IDENT), RepoTLOG(eng, IDENT)
    a, b = O.Repo(O.TLOG, 11), O.Repo(O.TLOG, 13)

    def both(batch):
        want.converge(batch)
        got.converge_deltas(batch)

    def write(cmds):
        for c in cmds:
            getattr(want, "tlog_" + c[0].lower())(*c[1:])
        got.write(cmds)

    # peer a: the special logs (three entries too many where a cutoff will drop them), a log to clear, short logs
    extra = {257: 3, 5000: 3}
    for n, k in SPECIAL.items():
        for j in range(n + extra.get(n, 0)):
            a.tlog_ins(k, _val(j), _ts(j))
    for j in range(3):
        a.tlog_ins(CLEARED, _val(j + 1), 5 + j)
    short = [b"k%04d" % i for i in range(1980)]
    for i, k in enumerate(short):
        for j in range(1 + i % 6):
            a.tlog_ins(k, _val(i + j), 100 + 3 * j + (i % 2))
    mids = [b"mid%d" % i for i in range(8)]
    for i, k in enumerate(mids):
        for j in range(90 + 5 * i):
            a.tlog_ins(k, _val(j + i), 5000 + 10 * j)
    both(a.flush().table())
    # local writes: a cleared log, raised cutoffs (the segment base moves), empty logs created by TRIMAT
    write([("CLR", CLEARED), ("TRIMAT", SPECIAL[257], _ts(3)), ("TRIM", SPECIAL[5000], 5000)] +
          [("TRIM", k, 2) for k in short[20:40]] + [("TRIMAT", k, 104) for k in short[40:60]] +
          [("TRIMAT", b"only-cutoff", 77)])
    # peer b, merge after merge: entries just above a log's oldest (the prefix moves into the front room),
    # appends, ties, and fresh keys
    for merge in range(4):
        for i, k in enumerate(mids):
            b.tlog_ins(k, b"old%d" % merge, 5000 + 10 * (merge + 1) + 1)
            b.tlog_ins(k, b"tie%d" % merge, 5000 + 10 * (merge + 2))
            for q in range(int(rng.integers(0, 4))):
                b.tlog_ins(k, _val(merge * 8 + q), 9000 + 10 * merge + q)
        for k in short[100 + 50 * merge:150 + 50 * merge]:
            b.tlog_ins(k, _val(merge), 50 + merge)
            b.tlog_ins(k, b"new-%d" % merge, 400 + merge)
        b.tlog_ins(b"fresh%d" % merge, _val(6), merge)
        both(b.flush().table())
    stats = eng.tlog_stats()
    assert stats["compactions"] >= 1, stats  # the pool was compacted along the way
    eng.arena_collect(3)  # every handle rewritten
    st = want.state()
    kb, ko = st["key_bytes"].tobytes(), np.asarray(st["key_offs"], np.int64)
    keys = [kb[ko[i]:ko[i + 1]] for i in range(len(ko) - 1)]
    lens = dict(zip(keys, np.diff(np.asarray(st["ent_offs"], np.int64)).tolist()))
    for n, k in SPECIAL.items():
        assert lens[k] == n, (k, lens[k])
    assert lens[CLEARED] == 0 and lens[b"only-cutoff"] == 0 and 1900 < len(keys) < 2100
    yield eng, got, st, keys
    eng.close()


TLOG_NAMES = ("found", "size", "cutoff", "ent_offs", "ts", "val_bytes", "val_offs")
TREG_NAMES = ("found", "ts", "val_bytes", "val_offs")


def _host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _same(got, ref, names):
    assert got["sizes"] == ref["sizes"], (got["sizes"], ref["sizes"])
    for name in names:
        g = _host(got[name]).view(ref[name].dtype)
        np.testing.assert_array_equal(g, ref[name], err_msg=name)


def _check_tlog(eng, st, keys, counts=None, device=False):
    got = eng.tlog_get_keys(keys, None if counts is None else np.array(counts, np.uint64), device=device)
    if device:
        eng.sync()
    ref = get_ref.tlog_get(st, keys, counts)
    _same(got, ref, TLOG_NAMES)
    size = ref["size"].tolist()
    cs = [ALL] * len(keys) if counts is None else counts
    assert got["sizes"][0] == sum(min(s, c) for s, c in zip(size, cs))
    assert got["sizes"][1] == int(np.diff(ref["val_offs"].astype(np.int64)).sum())
    return got


def test_tlog_lengths_times_counts(world):
    """every tile-edge length under counts 0, 1, len - 1, len, len + 1, 2^64 - 1 and NULL"""
    eng, _, st, _ = world
    keys = [CLEARED] + list(SPECIAL.values())
    lens = [0] + list(SPECIAL)
    for name, counts in (("0", [0] * len(keys)), ("1", [1] * len(keys)), ("len-1", [max(n - 1, 0) for n in lens]),
                         ("len", lens), ("len+1", [n + 1 for n in lens]), ("max", [ALL] * len(keys)), ("null", None)):
        got = _check_tlog(eng, st, keys, counts)
        assert got["found"].tolist() == [1] * len(keys), name
        assert got["size"].tolist() == lens, name
    # counts mixed within one query
    mixed = [3, 0, ALL, 64, 1, 255, 300, 10, 4999]
    got = _check_tlog(eng, st, keys, mixed)
    assert got["sizes"][0] == sum(min(a, c) for a, c in zip(lens, mixed))


def test_tlog_count_10_moves_10_entries_of_the_long_log(world):
    eng, _, st, _ = world
    got = _check_tlog(eng, st, [SPECIAL[5000], b"k0005"], [10, 10])
    assert got["size"].tolist() == [5000, 6] and got["ent_offs"].tolist() == [0, 10, 16]


def test_tlog_missing_keys_and_empty_queries(world):
    eng, _, st, keys = world
    hit = [SPECIAL[65], b"k0005", SPECIAL[255]]
    q = [MISSING[0], hit[0], MISSING[1], hit[1], MISSING[2], hit[2], MISSING[3]]
    got = _check_tlog(eng, st, q)
    assert got["found"].tolist() == [0, 1, 0, 1, 0, 1, 0]
    got = _check_tlog(eng, st, list(MISSING), [ALL, 0, 3, 1])  # only missing keys
    assert got["sizes"] == [0, 0, 0] and got["ent_offs"].tolist() == [0] * 5
    got = eng.tlog_get_keys([])  # n == 0: the single offset 0
    assert got["sizes"] == [0, 0, 0] and got["ent_offs"].tolist() == [0] and got["val_offs"].tolist() == [0]
    # an existing key with an empty log keeps its cutoff: CLR, and a TRIMAT that created the key
    got = _check_tlog(eng, st, [CLEARED, b"only-cutoff"])
    assert got["found"].tolist() == [1, 1] and got["size"].tolist() == [0, 0]
    assert got["cutoff"].tolist() == [8, 77]


def test_tlog_one_key_three_times_with_three_counts(world):
    eng, _, st, _ = world
    k = SPECIAL[257]
    got = _check_tlog(eng, st, [k, b"k0002", k, k], [2, ALL, 257, 0])
    assert np.diff(got["ent_offs"].astype(np.int64)).tolist() == [2, 3, 257, 0]


def test_tlog_every_key_in_one_query(world):
    """~2,000 queries (over the host cache's batch bound: the device directory
    answers) and ~9,000 entries: many tiles, most queries short, some empty"""
    eng, _, st, keys = world
    rng = np.random.default_rng(3)
    order = [keys[i] for i in rng.permutation(len(keys))]
    _check_tlog(eng, st, order)
    _check_tlog(eng, st, order, [3] * len(order))
    _check_tlog(eng, st, order[:700], [int(c) for c in rng.integers(0, 9, 700)])  # the host cache path


def test_tlog_device_keys_and_device_outputs(world):
    import torch
    from jylis_amd.engine import encode_keys
    eng, _, st, keys = world
    q = [SPECIAL[5000], MISSING[0], SPECIAL[64], b"k0033", CLEARED, SPECIAL[1], SPECIAL[255], MISSING[3]]
    counts = [300, 1, ALL, 2, 5, 1, 254, 9]
    kb, ko = encode_keys(q)
    dev = f"cuda:{eng.device}"
    dkeys = (torch.from_numpy(kb.copy()).to(dev), torch.from_numpy(ko.astype(np.int64)).to(dev))
    ref = get_ref.tlog_get(st, q, counts)
    for keys_arg in (dkeys, q):
        for device in (False, True):
            got = eng.tlog_get_keys(keys_arg, np.array(counts, np.uint64), device=device)
            if device:
                eng.sync()
                assert got["ts"].is_cuda
            _same(got, ref, TLOG_NAMES)


def test_tlog_short_capacities_write_nothing(world):
    """cap_ent alone short, cap_val_bytes alone short: exact sizes, every output keeps its pattern"""
    eng, _, st, _ = world
    q = [SPECIAL[63], MISSING[0], SPECIAL[257]]
    ref = get_ref.tlog_get(st, q, [ALL, 1, 100])
    ne, nb = ref["sizes"][0], ref["sizes"][1]
    assert ne == 163 and nb > 0
    for cap_e, cap_b in ((ne - 1, nb), (ne, nb - 1), (0, 0)):
        out = {"found": np.full(3, 0xAB, np.uint8), "size": np.full(3, 0xAB, np.uint64),
               "cutoff": np.full(3, 0xAB, np.uint64), "ent_offs": np.full(4, 0xAB, np.uint64),
               "ts": np.full(max(cap_e, 1), 0xAB, np.uint64), "val_bytes": np.full(max(cap_b, 1), 0xAB, np.uint8),
               "val_offs": np.full(cap_e + 1, 0xAB, np.uint64)}
        sizes, a = eng.tlog_get_keys_caps(q, np.array([ALL, 1, 100], np.uint64), cap_e, cap_b, out=out)
        assert sizes == ref["sizes"]
        for name, arr in a.items():
            assert (arr == 0xAB).all(), (name, cap_e, cap_b)
    sizes, a = eng.tlog_get_keys_caps(q, np.array([ALL, 1, 100], np.uint64), ne, nb)  # exactly enough
    assert sizes == ref["sizes"]
    np.testing.assert_array_equal(a["ts"][:ne], ref["ts"])
    np.testing.assert_array_equal(a["val_bytes"][:nb], ref["val_bytes"])


def test_tlog_repo_get_many_and_single_reads(world):
    _, repo, st, keys = world
    rng = np.random.default_rng(5)
    q = [SPECIAL[65], MISSING[0], CLEARED, SPECIAL[256]] + [keys[i] for i in rng.integers(0, len(keys), 12)]
    ref = get_ref.tlog_get(st, q)
    many = repo.get_many(q)
    assert many == [get_ref.tlog_reply(ref, i) for i in range(len(q))]
    assert many == [repo.get(k) for k in q]
    counts = [2, 1, None, 0] + [int(c) for c in rng.integers(0, 5, 12)]
    refc = get_ref.tlog_get(st, q, counts)
    assert repo.get_many(q, counts) == [get_ref.tlog_reply(refc, i) for i in range(len(q))]
    assert [repo.get(k, c) for k, c in zip(q, counts)] == [get_ref.tlog_reply(refc, i) for i in range(len(q))]
    assert [repo.size(k) for k in q] == ref["size"].tolist()
    assert [repo.cutoff(k) for k in q] == ref["cutoff"].tolist()


def test_tlog_read_settles_converges_in_flight(oracle_mod):
    """merges are only enqueued (a small pool: some spill); the keyed read settles them first"""
    from jylis_amd import synth as S
    from jylis_amd.engine import Engine
    from jylis_amd.repo import RepoTLOG
    O = oracle_mod
    eng = Engine(device=0, entry_capacity=1024)
    try:
        st, dl = S.tlog_tables(1500, seed=S.BASE_SEED + 77, rounds=3, mean_state=4, mean_delta=3)
        want, got = O.Repo(O.TLOG), RepoTLOG(eng)
        for b in [st] + dl:
            want.converge(b)
            got.converge_deltas(b)
        ws = want.state()
        kb, ko = ws["key_bytes"].tobytes(), np.asarray(ws["key_offs"], np.int64)
        keys = [kb[ko[i]:ko[i + 1]] for i in range(0, len(ko) - 1, 3)] + [b"absent"]
        _check_tlog(eng, ws, keys, [i % 6 for i in range(len(keys))])
        _check_tlog(eng, ws, keys)
    finally:
        eng.close()


# ---- TREG ----
def test_treg_get_keys(oracle_mod, engine):
    from jylis_amd.repo import RepoTREG
    O = oracle_mod
    want, got = O.Repo(O.TREG, IDENT), RepoTREG(engine, IDENT)
    assert engine.treg_get_keys([b"x", b"y"])["found"].tolist() == [0, 0]  # before any key exists
    peer = O.Repo(O.TREG, 11)
    names = [b"r%03d" % i for i in range(300)] + list(SPECIAL.values())
    for i, k in enumerate(names):
        peer.treg_set(k, _val(i), 10 + i % 4)
    peer.treg_set(b"bottom", b"", 0)  # a key converged to ("", 0): found, unlike a key never touched
    batch = peer.flush().table()
    want.converge(batch)
    got.converge_deltas(batch)
    # timestamp ties decided by the value: on the 8-byte prefix, behind it, and by length
    ties = [(b"t0", b"sameprefA", 7), (b"t0", b"sameprefB", 7), (b"t1", b"sameprefixed-long-value-2", 7),
            (b"t1", b"sameprefixed-long-value-1", 7), (b"t2", b"abcdefgh", 7), (b"t2", b"abcdefghi", 7),
            (b"t3", b"zz", 6), (b"t3", b"a", 7)]
    # ... and slots repeated inside one SET batch: their duplicates wait for a fold when the read comes
    reps = [(b"r007", b"first", 50), (b"r007", b"x" * 300, 51), (b"r007", b"second", 51), (b"r008", b"", 99)]
    for k, v, ts in ties + reps:
        want.treg_set(k, v, ts)
    got.set([k for k, _, _ in ties + reps], [v for _, v, _ in ties + reps], [ts for _, _, ts in ties + reps])
    q = [b"never", b"bottom", b"t0", b"t1", b"t2", b"t3", b"r007", b"r008", b"r007"] + names + [b"", b"r0070"]
    for collected in (False, True):
        st = want.state()
        ref = get_ref.treg_get(st, q)
        assert ref["found"][:2].tolist() == [0, 1] and ref["ts"][:2].tolist() == [0, 0]
        _same(engine.treg_get_keys(q), ref, TREG_NAMES)
        d = engine.treg_get_keys(q, device=True)
        engine.sync()
        _same(d, ref, TREG_NAMES)
        many = got.get_many(q)
        assert many == [get_ref.treg_reply(ref, i) for i in range(len(q))]
        assert many[:9] == [got.get(k) for k in q[:9]] == [want.treg_get(k) for k in q[:9]]
        assert many[0] is None and many[1] == (b"", 0)
        engine.arena_collect(2)
    # a short capacity: the size, and nothing written
    ref = get_ref.treg_get(want.state(), q)
    out = {"found": np.full(len(q), 0xAB, np.uint8), "ts": np.full(len(q), 0xAB, np.uint64),
           "val_bytes": np.full(ref["sizes"][0], 0xAB, np.uint8), "val_offs": np.full(len(q) + 1, 0xAB, np.uint64)}
    sizes, a = engine.treg_get_keys_caps(q, ref["sizes"][0] - 1, out=out)
    assert sizes == ref["sizes"] and all((arr == 0xAB).all() for arr in a.values())
    assert engine.treg_get_keys([])["val_offs"].tolist() == [0]


# ---- counters ----
@pytest.mark.parametrize("ctype", [0, 1])
def test_counter_get_keys(oracle_mod, engine, ctype):
    from helpers import random_history
    from jylis_amd.repo import REPOS
    O = oracle_mod
    want, got = O.Repo(ctype, IDENT), REPOS[ctype](engine, IDENT)
    f, v = engine.counter_get_keys(ctype, [b"k0", b"zz"])
    assert f.tolist() == [0, 0] and v.tolist() == [0, 0]  # before any key exists
    for b in random_history(O, ctype, seed=60 + ctype, nops=150):
        want.converge(b)
        got.converge_deltas(b)
    if ctype == 1:
        want.pncount_dec("neg", 5)
        want.pncount_inc("neg", 2)
        got.dec(["neg"], [5], IDENT)
        got.inc(["neg"], [2], IDENT)
    q = [b"absent"] + [b"k%d" % i for i in range(12)] + [b"neg", b"k3", b""]
    rf, rv = get_ref.counter_get(want.state(), q, pn=ctype == 1)
    f, v = engine.counter_get_keys(ctype, q)
    np.testing.assert_array_equal(f, rf)
    np.testing.assert_array_equal(v, rv)
    assert v.dtype == rv.dtype and f[0] == 0 and v[0] == 0
    assert v.tolist() == [int(x) for x in got.get(q)]
    if ctype == 1:
        assert int(v[13]) == -3 == want.pncount_get("neg")


# ---- the node: a query split over four shards keeps its order ----
def test_node_get_keeps_query_order(oracle_mod):
    from helpers import random_history
    from jylis_amd.node import Node
    O = oracle_mod
    node = Node(4, "copy")
    try:
        wants = {}
        for ctype in (O.GCOUNT, O.PNCOUNT, O.TREG, O.TLOG):
            wants[ctype] = O.Repo(ctype, 5)
            for b in random_history(O, ctype, seed=90 + ctype, nops=120, nkeys=40):
                wants[ctype].converge(b)
                node.converge_table(ctype, b)
        node.sync()
        q = [b"k%d" % i for i in (7, 39, 0, 41, 7, 13, 22, 5, 99, 31, 2)]
        assert len({node.shard_of(k) for k in q}) == 4
        for ctype in (O.GCOUNT, O.PNCOUNT):
            _, rv = get_ref.counter_get(wants[ctype].state(), q, pn=ctype == O.PNCOUNT)
            assert node.get(ctype, q) == [int(x) for x in rv]
        ref = get_ref.treg_get(wants[O.TREG].state(), q)
        assert node.get(O.TREG, q) == [get_ref.treg_reply(ref, i) for i in range(len(q))]
        counts = [None, 1, 0, 3, 2, None, 1, 4, 2, 0, 9]
        ref = get_ref.tlog_get(wants[O.TLOG].state(), q, counts)
        assert node.get(O.TLOG, q, counts) == [get_ref.tlog_reply(ref, i) for i in range(len(q))]
        ref = get_ref.tlog_get(wants[O.TLOG].state(), q)
        assert node.get(O.TLOG, q) == [get_ref.tlog_reply(ref, i) for i in range(len(q))]
    finally:
        node.close()


# ---- a type without a key: what the column form writes, and what it leaves ----
K_THREADS = 256  # a workgroup of the read kernels (kThreads, jy_wire.hpp)
PAT = 0xCD


@pytest.fixture(scope="module")
def fresh_engine():
    """nothing interned, and never written: the reads create no key"""
    from jylis_amd.engine import Engine
    eng = Engine(device=0)
    yield eng
    assert [eng.nkeys(t) for t in range(4)] == [0, 0, 0, 0]
    eng.close()


def _patterned(eng, spec, device):
    """spec: name -> (elements, bytes each, leading elements the call zeroes) -> PAT-filled arrays"""
    import torch
    out = {}
    for name, (k, width, _) in spec.items():
        if device:
            raw = torch.full((k * width,), PAT, dtype=torch.uint8, device=f"cuda:{eng.device}")
            out[name] = raw if width == 1 else raw.view(torch.int64)
        else:
            out[name] = np.full(k * width, PAT, np.uint8).view(np.uint8 if width == 1 else np.uint64)
    return out


def _only_zeroed(out, spec, what):
    for name, (k, width, zeroed) in spec.items():
        want = np.full(k * width, PAT, np.uint8)
        want[:zeroed * width] = 0
        np.testing.assert_array_equal(_host(out[name]).view(np.uint8), want, err_msg=f"{what}: {name}")


@pytest.mark.parametrize("n", [1, 2, 65, K_THREADS + 1])
def test_a_type_without_a_key_answers_bottom_and_writes_no_more(fresh_engine, n):
    """include/jylis_gpu.h: a key never interned gives found 0 and the type's
    bottom -- ts 0 and an empty value (val_offs all 0), size 0, cutoff 0 and no
    entries (ent_offs all 0; of val_offs[entries + 1] the one element 0),
    counter value 0 -- and sizes_out all 0.  Every array is one element longer
    than the call may use and filled with 0xCD: the bytes past the answer, and
    the whole of ts (TLOG) and val_bytes, keep the fill.  One lane, one past a
    wave's 64 and one past a workgroup; host and device keys and outputs."""
    import ctypes as C
    from jylis_amd import _lib as L
    eng = fresh_engine
    keys = [b"q%d" % (i % 7) for i in range(n - 1)] + [b""]  # repeats from n = 9 on, and the empty key
    cap_e, cap_b = 3, 5
    treg = {"found": (n + 1, 1, n), "ts": (n + 1, 8, n), "val_bytes": (cap_b + 1, 1, 0), "val_offs": (n + 2, 8, n + 1)}
    tlog = {"found": (n + 1, 1, n), "size": (n + 1, 8, n), "cutoff": (n + 1, 8, n), "ent_offs": (n + 2, 8, n + 1),
            "ts": (cap_e + 1, 8, 0), "val_bytes": (cap_b + 1, 1, 0), "val_offs": (cap_e + 2, 8, 1)}
    ctr = {"found": (n + 1, 1, n), "out": (n + 1, 8, n)}
    for device in (False, True):
        q = _device_keys(eng, keys) if device else keys
        tag = f"n={n} device={device}"
        out = _patterned(eng, treg, device)
        sizes, _ = eng.treg_get_keys_caps(q, cap_b, device, out)
        eng.sync()
        assert sizes == [0, 0], tag
        _only_zeroed(out, treg, "TREG " + tag)
        for counts in (None, np.arange(n, dtype=np.uint64)):
            out = _patterned(eng, tlog, device)
            sizes, _ = eng.tlog_get_keys_caps(q, counts, cap_e, cap_b, device, out)
            eng.sync()
            assert sizes == [0, 0, 0], tag
            _only_zeroed(out, tlog, "TLOG " + tag)
        for ctype in (0, 1):
            out = _patterned(eng, ctr, device)
            _, kb, ko, nq, kmem = eng._query(q)
            ptrs = [C.c_void_p(a.data_ptr() if device else a.ctypes.data) for a in (out["found"], out["out"])]
            mem = L.DEVICE if device else L.HOST
            eng._check(eng.lib.jy_counter_get_keys(eng.h, ctype, nq, kb, ko, kmem, *ptrs, mem))
            eng.sync()
            _only_zeroed(out, ctr, f"counter {ctype} " + tag)


def _device_keys(eng, keys):
    import torch
    from jylis_amd.engine import encode_keys
    kb, ko = encode_keys(keys)
    dev = f"cuda:{eng.device}"
    kb = kb if len(kb) else np.zeros(1, np.uint8)
    return torch.from_numpy(kb.copy()).to(dev), torch.from_numpy(ko.astype(np.int64)).to(dev)


# ---- the column form and the reply form sit on one read ----
def test_column_and_reply_forms_agree_on_the_shared_read():
    """20 logs (one of K_THREADS + 44 entries, so its entries span two tiles;
    raised cutoffs; an emptied one) and 20 registers; one query of 65 keys --
    found, missing, repeated -- read in both forms.  What the reply form
    reports in sizes_out is the column form's found count and entry count, and
    its bytes are the column answer formatted by resp_ref: SIZE and CUTOFF
    replies carry size[] and cutoff[], GET replies every entry."""
    from jylis_amd import _lib as L
    from jylis_amd.engine import Engine
    from jylis_amd.repo import RepoTLOG, RepoTREG
    eng = Engine(device=0)
    try:
        logs, regs = [b"log%02d" % i for i in range(20)], [b"reg%02d" % i for i in range(20)]
        lens = [K_THREADS + 44 if i == 7 else 1 + i % 5 for i in range(20)]
        tl, tr = RepoTLOG(eng, IDENT), RepoTREG(eng, IDENT)
        tl.write([("INS", k, _val(i + j), _ts(j)) for i, k in enumerate(logs) for j in range(lens[i])])
        tl.write([("TRIMAT", logs[3], _ts(2)), ("TRIM", logs[7], K_THREADS + 40), ("CLR", logs[9])])
        tr.set(regs, [_val(i) for i in range(20)], [10 + i % 4 for i in range(20)])
        n = 65

        def pick(ks, i):  # every fourth missing, key 7 every fifth time, the others spread
            return b"missing%d" % i if i % 4 == 3 else ks[(7 * i) % 20 if i % 5 else 7]

        # TLOG: GET, SIZE and CUTOFF mixed; the reply form gives SIZE and CUTOFF the count 0, so the column form is asked that
        q = [pick(logs, i) for i in range(n)]
        what = np.array([(L.TLOG_RD_GET, L.TLOG_RD_GET, L.TLOG_RD_SIZE, L.TLOG_RD_GET, L.TLOG_RD_CUTOFF)[i % 5]
                         for i in range(n)], np.uint8)
        counts = np.array([(ALL, 2, 9, 0, 1, K_THREADS + 1)[i % 6] for i in range(n)], np.uint64)
        eff = np.where(what == L.TLOG_RD_GET, counts, np.uint64(0))
        for device in (False, True):
            col = eng.tlog_get_keys(q, eff, device=device)
            rep = eng.tlog_get_resp(q, counts, what, device=device)
            eng.sync()
            col = {k: (v if k == "sizes" else _host(v)) for k, v in col.items()}
            assert col["found"].tolist() == [0 if i % 4 == 3 else 1 for i in range(n)]
            assert col["sizes"][0] > K_THREADS and col["size"].max() == K_THREADS + 40 and col["cutoff"].max() > 0
            rb, ro, _ = resp_ref.tlog(col, what)
            assert rep["sizes"] == [len(rb), col["sizes"][0], col["sizes"][2]]
            np.testing.assert_array_equal(_host(rep["reply_offs"]).view(np.uint64), ro)
            assert _host(rep["reply_bytes"]).tobytes() == rb
        q = [pick(regs, i) for i in range(n)]
        for device in (False, True):
            col = eng.treg_get_keys(q, device=device)
            rep = eng.treg_get_resp(q, device=device)
            eng.sync()
            col = {k: (v if k == "sizes" else _host(v)) for k, v in col.items()}
            rb, ro, _ = resp_ref.treg(col)
            assert rep["sizes"] == [len(rb), col["sizes"][1]] and col["sizes"][1] == n - n // 4
            np.testing.assert_array_equal(_host(rep["reply_offs"]).view(np.uint64), ro)
            assert _host(rep["reply_bytes"]).tobytes() == rb
    finally:
        eng.close()
