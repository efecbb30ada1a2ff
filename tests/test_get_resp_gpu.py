"""RESP replies on the GPU (jy_treg_get_resp, jy_tlog_get_resp,
jy_counter_get_resp; k_resp.hip) against tests/resp_ref.py over the CPU
oracle's state, byte-exact.

The states and the queries are the case tables of tests/resp_cases.py, whose
coverage tests/test_get_resp_cpu.py asserts without a GPU.  Each state is
built once, by converging and writing through the repo against the oracle,
and only read afterwards.  Every case is read with host and device keys, into
host and device outputs, into a device buffer that starts 1, 3 and 7 bytes
past an 8-byte boundary, and with a capacity one byte short (sizes only: the
buffer keeps its fill).

Writer paths: the TREG case "missing_run" has workgroups whose piece offsets
exceed the writer's LDS stage (kStage, restated as resp_cases.K_STAGE) and
are read from memory; every other case runs the staged path."""
import numpy as np
import pytest

import get_ref
import resp_cases as RC
import resp_ref

pytestmark = pytest.mark.gpu

FILL = 0xAB


def _host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _device_keys(eng, keys):
    import torch
    from jylis_amd.engine import encode_keys
    kb, ko = encode_keys(keys)
    dev = f"cuda:{eng.device}"
    kb = kb if len(kb) else np.zeros(1, np.uint8)
    return torch.from_numpy(kb.copy()).to(dev), torch.from_numpy(ko.astype(np.int64)).to(dev)


def _check(eng, keys, call, caps, want):
    """call(keys, device) -> the Engine answer; caps(keys, cap, device, out) ->
    (sizes, arrays); want = (bytes, offs, pieces, sizes)"""
    import torch
    rb, ro, _, sizes = want
    n = len(keys)
    ref = np.frombuffer(rb, np.uint8)

    def same(got):
        assert got["sizes"] == sizes, (got["sizes"], sizes)
        np.testing.assert_array_equal(_host(got["reply_offs"]).view(np.uint64), ro)
        np.testing.assert_array_equal(_host(got["reply_bytes"]), ref)

    dkeys = _device_keys(eng, keys) if n else keys
    for keys_arg in (keys, dkeys):
        same(call(keys_arg, False))
        got = call(keys_arg, True)
        eng.sync()
        assert got["reply_offs"].is_cuda
        same(got)
    if n == 0:
        return
    total = len(rb)
    dev = f"cuda:{eng.device}"
    # a device buffer that starts 1, 3 and 7 bytes past an 8-byte boundary, guarded on both sides
    for mis in (1, 3, 7):
        buf = torch.full((total + 32,), FILL, dtype=torch.uint8, device=dev)
        assert buf.data_ptr() % 8 == 0
        out = {"reply_bytes": buf[8 + mis:8 + mis + total], "reply_offs": torch.zeros(n + 1, dtype=torch.int64, device=dev)}
        got_sizes, _ = caps(keys, total, True, out)
        eng.sync()
        assert got_sizes == sizes
        h = buf.cpu().numpy()
        np.testing.assert_array_equal(h[8 + mis:8 + mis + total], ref)
        assert (h[:8 + mis] == FILL).all() and (h[8 + mis + total:] == FILL).all(), mis
        np.testing.assert_array_equal(out["reply_offs"].cpu().numpy().view(np.uint64), ro)
    # one byte short: sizes only, host and device
    out = {"reply_bytes": np.full(total, FILL, np.uint8), "reply_offs": np.full(n + 1, FILL, np.uint64)}
    got_sizes, a = caps(keys, total - 1, False, out)
    assert got_sizes == sizes and all((arr == FILL).all() for arr in a.values())
    out = {"reply_bytes": torch.full((total,), FILL, dtype=torch.uint8, device=dev),
           "reply_offs": torch.full((n + 1,), FILL, dtype=torch.int64, device=dev)}
    got_sizes, a = caps(dkeys, total - 1, True, out)
    eng.sync()
    assert got_sizes == sizes and all(bool((arr == FILL).all()) for arr in a.values())


def _unchanged(eng, ctype, fn):
    """fn() reads only: key count, pending set, arena usage (and the TLOG layout) stay"""
    def snap():
        s = [eng.nkeys(ctype)]
        if ctype in (0, 1):
            s.append(eng.counter_deltas_size(ctype))
        else:
            s.append(eng.treg_deltas_size() if ctype == 2 else eng.tlog_deltas_size())
            s.append(eng.arena_usage(ctype))
        if ctype == 3:
            lay = eng.tlog_layout(np.arange(eng.nkeys(3), dtype=np.uint32))
            s.append({k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in lay.items()})
        return s
    before = snap()
    fn()
    assert snap() == before


# ---- TLOG ----
@pytest.fixture(scope="module")
def tlog_world(oracle_mod):
    from jylis_amd.engine import Engine
    from jylis_amd.repo import RepoTLOG
    O = oracle_mod
    eng = Engine(device=0, entry_capacity=1024)
    want, got = O.Repo(O.TLOG, RC.IDENT), RepoTLOG(eng, RC.IDENT)
    RC.apply_steps(RC.tlog_steps(O), want, got)
    eng.arena_collect(3)  # every handle rewritten before the reads
    eng.tlog_get_keys([RC.CLEARED])  # (settles the merges: the layout below is the settled one)
    st = want.state()
    yield eng, got, st, RC.tlog_queries(RC.state_keys(st))
    eng.close()


TLOG_CASES = ("every_key", "repeated", "count_0", "count_1", "count_9", "count_10", "count_11", "count_all",
              "count_one_past", "mixed_what", "n0", "hot_alone", "hot_among_255")


@pytest.mark.parametrize("name", TLOG_CASES)
def test_tlog_replies(tlog_world, name):
    eng, _, st, cases = tlog_world
    assert set(cases) == set(TLOG_CASES)
    keys, counts, what = cases[name]
    cnt = None if counts is None else np.array(counts, np.uint64)
    wh = None if what is None else np.array(what, np.uint8)
    want = RC.tlog_expect(st, cases[name])
    _unchanged(eng, 3, lambda: _check(
        eng, keys, lambda k, device: eng.tlog_get_resp(k, cnt, wh, device=device),
        lambda k, cap, device, out: eng.tlog_get_resp_caps(k, cnt, wh, cap, device, out), want))


def test_tlog_what_is_checked_before_anything_is_written(tlog_world):
    from jylis_amd.engine import EngineError
    eng, _, _, _ = tlog_world
    out = {"reply_bytes": np.full(64, FILL, np.uint8), "reply_offs": np.full(3, FILL, np.uint64)}
    with pytest.raises(EngineError):
        eng.tlog_get_resp_caps([RC.CLEARED, b"a"], None, np.array([0, 3], np.uint8), 64, False, out)
    assert all((arr == FILL).all() for arr in out.values())


def test_tlog_repo_get_resp(tlog_world):
    _, repo, st, _ = tlog_world
    q = [RC.SPECIAL[65], RC.MISSING[0], RC.CLEARED, RC.TSEDGE]
    rb, ro = repo.get_resp(q, [2, None, 1, None], [0, 0, 2, 1])
    want = RC.tlog_expect(st, (q, [2, None, 1, None], [0, 0, 2, 1]))
    assert rb == want[0] and ro.tolist() == want[1].tolist()


# ---- TREG ----
@pytest.fixture(scope="module")
def treg_world(oracle_mod):
    from jylis_amd.engine import Engine
    from jylis_amd.repo import RepoTREG
    O = oracle_mod
    eng = Engine(device=0)
    got = RepoTREG(eng, RC.IDENT)
    want = O.Repo(O.TREG, RC.IDENT)
    RC.apply_steps(RC.treg_steps(O), want, got)
    yield eng, got, want
    eng.close()


@pytest.mark.parametrize("name", ("every_key", "missing_run", "n0", "one_missing", "one_found"))
def test_treg_replies(treg_world, name):
    """the first read folds the pending duplicates of the repeated SETs"""
    eng, got, want = treg_world
    st = want.state()
    case = RC.treg_queries(RC.state_keys(st))[name]
    exp = RC.treg_expect(st, case)
    _unchanged(eng, 2, lambda: _check(
        eng, case[0], lambda k, device: eng.treg_get_resp(k, device=device),
        lambda k, cap, device, out: eng.treg_get_resp_caps(k, cap, device, out), exp))
    rb, ro = got.get_resp(case[0])
    assert rb == exp[0] and ro.tolist() == exp[1].tolist()


def test_treg_before_any_key(engine):
    r = engine.treg_get_resp([b"x", b"", b"x"])
    assert r["reply_bytes"].tobytes() == b"$-1\r\n" * 3 and r["reply_offs"].tolist() == [0, 5, 10, 15]
    assert r["sizes"] == [15, 0]
    r = engine.tlog_get_resp([b"x", b"y"], None, np.array([0, 1], np.uint8))
    assert r["reply_bytes"].tobytes() == b"*0\r\n:0\r\n" and r["sizes"] == [8, 0, 0]
    r = engine.counter_get_resp(1, [b"x"])
    assert r["reply_bytes"].tobytes() == b":0\r\n" and r["sizes"] == [4, 0]


# ---- counters ----
@pytest.mark.parametrize("ctype", [0, 1])
def test_counter_replies(oracle_mod, engine, ctype):
    from jylis_amd.engine import EngineError
    from jylis_amd.repo import REPOS
    O = oracle_mod
    want, got = O.Repo(ctype, RC.IDENT), REPOS[ctype](engine, RC.IDENT)
    RC.apply_steps(RC.counter_steps(O, ctype), want, got)  # through counter_converge_keys
    st = want.state()
    for name, case in RC.counter_queries(RC.state_keys(st)).items():
        exp = RC.counter_expect(st, case, ctype == 1)
        _unchanged(engine, ctype, lambda: _check(
            engine, case[0], lambda k, device: engine.counter_get_resp(ctype, k, device=device),
            lambda k, cap, device, out: engine.counter_get_resp_caps(ctype, k, cap, device, out), exp))
        rb, ro = got.get_resp(case[0])
        assert rb == exp[0] and ro.tolist() == exp[1].tolist()
    with pytest.raises(EngineError):
        engine.counter_get_resp(2, [b"k"])  # JY_ETYPE


# ---- the host mirror: the same commands, the same bytes ----
def test_replies_equal_the_host_mirrors(oracle_mod):
    """about 50 commands go to a jyh_db (host_repo.hip: its Respond formats on
    the host) and, through the keyed writes, to an Engine; every GET / SIZE /
    CUTOFF asked of both: the mirror's replies laid end to end are reply_bytes"""
    from jylis_amd.engine import Engine
    from jylis_amd.host import Database
    from jylis_amd.repo import REPOS
    ident = 7
    db, eng = Database(0, ident), Engine(device=0)
    try:
        repos = {c: REPOS[c](eng, ident) for c in (0, 1, 2, 3)}
        keys = {"GCOUNT": [b"g%d" % i for i in range(4)], "PNCOUNT": [b"p%d" % i for i in range(4)],
                "TREG": [b"r%d" % i for i in range(4)], "TLOG": [b"l%d" % i for i in range(4)]}
        ncmd = 0
        for i in range(13):
            k = i % 4
            v = (b"value-%02d-" % i) * (i % 4)
            cmds = [("GCOUNT", "INC", keys["GCOUNT"][k], 10**i - 1), ("PNCOUNT", "INC", keys["PNCOUNT"][k], 3 * i),
                    ("PNCOUNT", "DEC", keys["PNCOUNT"][(k + 1) % 4], 10**i), ("TREG", "SET", keys["TREG"][k], v, 9 + i % 3),
                    ("TLOG", "INS", keys["TLOG"][k % 3], v, 5 + i // 2)]
            for c in cmds[:4 if i == 12 else 5]:
                assert db.apply(*[w if isinstance(w, (str, bytes)) else str(w) for w in c]) == b"+OK\r\n"
                ncmd += 1
                t, op = c[0], c[1]
                if t == "GCOUNT":
                    repos[0].inc([c[2]], np.array([c[3]], np.uint64), ident)
                elif t == "PNCOUNT":
                    getattr(repos[1], op.lower())([c[2]], np.array([c[3]], np.uint64), ident)
                elif t == "TREG":
                    repos[2].set([c[2]], [c[3]], [c[4]])
                else:
                    repos[3].write([("INS", c[2], c[3], c[4])])
        assert 45 <= ncmd <= 70
        for t, ctype in (("GCOUNT", 0), ("PNCOUNT", 1), ("TREG", 2)):
            q = keys[t] + [b"nobody"]
            mirror = b"".join(db.apply(t, "GET", k) for k in q)
            rb, ro = repos[ctype].get_resp(q)
            assert rb == mirror, t
        q = keys["TLOG"] + [b"nobody"]
        for op, what, count in (("GET", 0, None), ("GET", 0, 2), ("SIZE", 1, None), ("CUTOFF", 2, None)):
            mirror = b"".join(db.apply("TLOG", op, k, *([str(count)] if count else [])) for k in q)
            rb, ro = repos[3].get_resp(q, None if count is None else [count] * len(q), [what] * len(q))
            assert rb == mirror, op
    finally:
        eng.close()
        db.close()


# ---- the node: a query split over two shards keeps its order ----
def test_node_get_resp_keeps_query_order(oracle_mod):
    from helpers import random_history
    from jylis_amd.node import Node
    O = oracle_mod
    node = Node(2, "copy")
    try:
        wants = {}
        for ctype in (O.GCOUNT, O.PNCOUNT, O.TREG, O.TLOG):
            wants[ctype] = O.Repo(ctype, 5)
            for b in random_history(O, ctype, seed=190 + ctype, nops=120, nkeys=40):
                wants[ctype].converge(b)
                node.converge_table(ctype, b)
        node.sync()
        q = [b"k%d" % (i * 7 % 50) for i in range(200)]  # keys 40..49 were never written
        shards = [node.shard_of(k) for k in q]
        assert set(shards) == {0, 1} and any(a != b for a, b in zip(shards, shards[1:]))
        for ctype in (O.GCOUNT, O.PNCOUNT):
            rb, ro = node.get_resp(ctype, q)
            exp = resp_ref.counter(node.get(ctype, q))
            assert rb == exp[0] and ro.tolist() == exp[1].tolist()
        rb, ro = node.get_resp(O.TREG, q)
        exp = resp_ref.from_treg(node.get(O.TREG, q))
        assert rb == exp[0] and ro.tolist() == exp[1].tolist()
        counts = [None if i % 3 == 0 else i % 4 for i in range(len(q))]
        rb, ro = node.get_resp(O.TLOG, q, counts)
        exp = resp_ref.from_tlog(node.get(O.TLOG, q, counts))
        assert rb == exp[0] and ro.tolist() == exp[1].tolist()
        ref = get_ref.tlog_get(wants[O.TLOG].state(), q, counts)
        what = [i % 3 for i in range(len(q))]
        rb, ro = node.get_resp(O.TLOG, q, counts, what)
        exp = resp_ref.tlog(ref, what)
        assert rb == exp[0] and ro.tolist() == exp[1].tolist()
    finally:
        node.close()
