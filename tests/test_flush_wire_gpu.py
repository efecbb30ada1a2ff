"""The wire-form flush on the GPU (jy_*_flush_wire): flush_deltas() as the
arrays the same type's jy_node_*_converge takes -- key strings from the
device key directory, value bytes from the arenas, built by the gather
kernels of k_flush_wire.hip -- against the CPU oracle's flush, the slot-form
flush, byte-exact expectations, and through the loop it exists for: node A
writes and flushes to device memory, node B converges those tensors."""
import numpy as np
import pytest

from helpers import assert_state_equal, join_rows, random_write, split_rows

pytestmark = pytest.mark.gpu

IDENT = 0x5EED_0000_F1A5_0001
OTHER = 0x5EED_0000_F1A5_0002
TYPES = [0, 1, 2, 3, 4]


class _Recorder:
    """forwards helpers.random_write's calls to an oracle replica and keeps them"""

    def __init__(self, repo):
        self.repo, self.ops = repo, []

    def __getattr__(self, name):
        def call(*a):
            self.ops.append((name,) + a)
            return getattr(self.repo, name)(*a)
        return call


def _random_ops(O, ctype, want, rng, nops, nkeys=12):
    rec = _Recorder(want)
    for _ in range(nops):
        random_write(O, ctype, rec, f"k{int(rng.integers(nkeys))}", rng, val_len=30)
    return rec.ops


def _apply(ctype, repo, ops):
    """the recorded oracle writes on a GPU repo, in order"""
    if ctype in (0, 1):
        for name, sign in (("gcount_inc", 0), ("pncount_inc", 0), ("pncount_dec", 1)):
            sel = [o for o in ops if o[0] == name]
            if sel:
                vals = np.array([o[2] for o in sel], np.int64)
                (repo.dec if sign else repo.inc)([o[1] for o in sel], vals, IDENT)
    elif ctype == 2:
        repo.set([o[1] for o in ops], [o[2] for o in ops], [o[3] for o in ops])
    elif ctype == 3:
        code = {"tlog_ins": "INS", "tlog_trimat": "TRIMAT", "tlog_trim": "TRIM", "tlog_clr": "CLR"}
        repo.write([(code[o[0]],) + o[1:] for o in ops])
    else:
        code = {"ujson_ins": "INS", "ujson_rm": "RM", "ujson_clr": "CLR"}
        repo.write([(code[o[0]],) + o[1:] for o in ops], IDENT)


def _by_key(ctype, t):
    return join_rows(ctype, split_rows(ctype, t))


def _flush_wire(ctype, repo):
    return repo.flush_wire(IDENT) if ctype in (0, 1) else repo.flush_wire()


def _flush_slots(ctype, repo):
    return repo.flush_deltas(IDENT) if ctype in (0, 1) else repo.flush_deltas()


def _deltas_size(ctype, eng):
    return eng.counter_deltas_size(ctype) if ctype in (0, 1) else (
        eng.treg_deltas_size, eng.tlog_deltas_size, eng.ujson_deltas_size)[ctype - 2]()


def _check_offsets(w, sizes_of):
    """every offsets array starts at 0, never decreases and ends at its total"""
    for name, total in sizes_of.items():
        o = np.asarray(w[name]).astype(np.int64)
        assert o[0] == 0 and (np.diff(o) >= 0).all() and o[-1] == total, name


@pytest.fixture
def engine2():
    from jylis_amd.engine import Engine
    e = Engine(device=0)
    yield e
    e.close()


# 1 ---------------------------------------------------------------------------
@pytest.mark.parametrize("ctype", TYPES)
def test_parity_with_the_oracle(oracle_mod, engine, ctype):
    """the same ~300 random local writes over 12 keys on an oracle replica and
    the GPU repo, flushed three times (clearing and re-marking)"""
    from jylis_amd.repo import REPOS
    O = oracle_mod
    rng = np.random.default_rng(810 + ctype)
    want = O.Repo(ctype, IDENT)
    got = REPOS[ctype](engine, IDENT)
    for _ in range(3):
        _apply(ctype, got, _random_ops(O, ctype, want, rng, 100))
        assert got.deltas_size() == want.deltas_size() > 0
        assert_state_equal(ctype, _by_key(ctype, want.flush().table()), _by_key(ctype, _flush_wire(ctype, got)))
        assert got.deltas_size() == 0
    assert_state_equal(ctype, want.state(), got.state())


# 2 ---------------------------------------------------------------------------
@pytest.mark.parametrize("ctype", TYPES)
def test_agrees_with_the_slot_form(oracle_mod, engine, engine2, ctype):
    """the same pending set on two engines: flush_deltas() on one and
    flush_wire() on the other give identical tables, row for row"""
    from jylis_amd.repo import REPOS
    O = oracle_mod
    rng = np.random.default_rng(820 + ctype)
    ops = _random_ops(O, ctype, O.Repo(ctype, IDENT), rng, 150)
    a, b = REPOS[ctype](engine, IDENT), REPOS[ctype](engine2, IDENT)
    _apply(ctype, a, ops)
    _apply(ctype, b, ops)
    ta, tb = _flush_slots(ctype, a), _flush_wire(ctype, b)
    assert len(ta["key_offs"]) > 1
    assert set(ta) == set(tb)
    for k in ta:
        np.testing.assert_array_equal(np.asarray(ta[k]), np.asarray(tb[k]), err_msg=f"field {k}")


# 3 ---------------------------------------------------------------------------
KEY_LENS = [1, 7, 8, 9, 15, 16, 17, 40]


def _edge_values(rng):
    lens = list(range(25)) + [255, 256, 257]
    return [bytes(rng.integers(0, 256, n).astype(np.uint8)) for n in lens]


def _edge_keys(n):
    """distinct keys of lengths KEY_LENS in turn (the tag keeps them distinct)"""
    keys = []
    for i in range(n):
        L = KEY_LENS[i % len(KEY_LENS)]
        keys.append((bytes([65 + i % 26, 97 + (i // 26) % 26]) + b"#" * 40)[:L] if L > 1 else bytes([33 + i // 8]))
    assert len(set(keys)) == n
    return keys


def _strings(buf, offs):
    raw, o = bytes(np.asarray(buf, np.uint8)), np.asarray(offs).astype(np.int64)
    return [raw[o[i]:o[i + 1]] for i in range(len(o) - 1)]


@pytest.mark.parametrize("device", [False, True])
def test_byte_edges_treg(engine, device):
    """values of every length 0..24, 255..257, one 70,000-byte value among
    8-byte ones, key lengths over the directory's word and tail paths"""
    from jylis_amd.repo import RepoTREG, wire_to_host
    rng = np.random.default_rng(830)
    vals = _edge_values(rng)
    vals += [b"8bytes_%d" % i for i in range(6)] + [bytes(rng.integers(0, 256, 70000).astype(np.uint8))]
    vals += [b"8bytes_%d" % i for i in range(6, 9)]
    keys = _edge_keys(len(vals))
    ts = np.arange(1, len(vals) + 1, dtype=np.uint64)
    RepoTREG(engine).set(keys, vals, ts)
    w = engine.flush_wire(2, device=device)
    engine.sync()
    w = wire_to_host(2, w)
    assert _strings(w["key_bytes"], w["key_offs"]) == keys  # slot order = order of first use
    assert _strings(w["val_bytes"], w["val_offs"]) == vals
    np.testing.assert_array_equal(w["ts"], ts)
    _check_offsets(w, {"key_offs": sum(map(len, keys)), "val_offs": sum(map(len, vals))})
    assert len(w["key_bytes"]) == sum(map(len, keys)) and len(w["val_bytes"]) == sum(map(len, vals))


def test_byte_edges_tlog(engine):
    """the same values as log entries: one key per value, and one key holding all of them"""
    from jylis_amd.repo import RepoTLOG
    rng = np.random.default_rng(831)
    vals = _edge_values(rng) + [b"8bytes_0", bytes(rng.integers(0, 256, 70000).astype(np.uint8)), b"8bytes_1"]
    keys = _edge_keys(len(vals))
    cmds = [("INS", k, v, 10 + i) for i, (k, v) in enumerate(zip(keys, vals))]
    cmds += [("INS", b"all-of-them", v, 100 + i) for i, v in enumerate(vals)]
    RepoTLOG(engine).write(cmds)
    w = engine.flush_wire(3)
    assert _strings(w["key_bytes"], w["key_offs"]) == keys + [b"all-of-them"]
    want = vals + vals[::-1]  # a log's entries newest first
    assert _strings(w["val_bytes"], w["val_offs"]) == want
    np.testing.assert_array_equal(w["ent_offs"], np.concatenate([np.arange(len(vals)),
                                                                 [len(vals), 2 * len(vals)]]).astype(np.uint64))
    np.testing.assert_array_equal(w["ts"][len(vals):], 100 + np.arange(len(vals))[::-1])
    _check_offsets(w, {"key_offs": len(w["key_bytes"]), "ent_offs": len(want), "val_offs": sum(map(len, want))})


# 4 ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 5000])
def test_pending_counts(engine, n):
    """pending keys across the gather's tile and the scans' boundaries"""
    from jylis_amd.engine import WIRE_ARRAYS
    from jylis_amd.repo import RepoGCOUNT, RepoTREG, wire_to_host
    rng = np.random.default_rng(840 + n)
    keys = [b"key-%d" % i for i in range(n)]
    vals = [bytes(rng.integers(0, 256, int(L)).astype(np.uint8)) for L in rng.integers(0, 21, n)]
    g, t = RepoGCOUNT(engine, IDENT), RepoTREG(engine)
    if n:
        g.inc(keys, np.arange(1, n + 1), IDENT)
        t.set(keys, vals, np.full(n, 3, np.uint64))
    wc = engine.flush_wire(0, col=engine.replica_col(IDENT))
    wt = engine.flush_wire(2, device=True)
    engine.sync()
    wt = wire_to_host(2, wt)
    for ctype, w in ((0, wc), (2, wt)):
        for name, _, _, plus in WIRE_ARRAYS[ctype]:
            if plus:
                assert len(w[name]) == n + 1 and int(w[name][0]) == 0, name
    assert _strings(wc["key_bytes"], wc["key_offs"]) == keys
    np.testing.assert_array_equal(wc["cell_offs"], np.arange(n + 1))
    np.testing.assert_array_equal(wc["val"], np.arange(1, n + 1))
    assert not wc["sign"].any() and (wc["col"] == engine.replica_col(IDENT)).all()
    assert _strings(wt["key_bytes"], wt["key_offs"]) == keys
    assert _strings(wt["val_bytes"], wt["val_offs"]) == vals
    assert _deltas_size(0, engine) == 0 and _deltas_size(2, engine) == 0


@pytest.mark.parametrize("device", [False, True])
def test_crowded_tiles(engine, device):
    """5,000 pending keys whose values are 0 or 1 byte long: a 2 KB output
    tile of the value gather then spans more items than the workgroup stages
    in LDS (1,024 offsets), so its lanes search the offsets in global memory;
    flushed twice, the second time in one call with remembered capacities"""
    from jylis_amd.repo import RepoTREG, wire_to_host
    rng = np.random.default_rng(845)
    n = 5000
    keys = [b"c%d" % i for i in range(n)]
    repo = RepoTREG(engine)
    for ts in (1, 2):
        vals = [bytes([int(x)]) if x else b"" for x in rng.integers(0, 256, n) * rng.integers(0, 2, n)]
        assert 1500 < sum(map(len, vals)) < 3500
        repo.set(keys, vals, np.full(n, ts, np.uint64))
        w = engine.flush_wire(2, device=device)
        engine.sync()
        w = wire_to_host(2, w)
        assert _strings(w["key_bytes"], w["key_offs"]) == keys
        assert _strings(w["val_bytes"], w["val_offs"]) == vals
        assert _deltas_size(2, engine) == 0


# 5 ---------------------------------------------------------------------------
@pytest.mark.parametrize("ctype", [1, 2, 3, 4])
def test_two_phase(oracle_mod, engine, engine2, ctype):
    """one capacity short by one element, each output in turn: nothing written,
    nothing cleared, the sizes reported; then exact capacities give the bytes a
    fresh engine gives, and the pending set is gone"""
    from jylis_amd.engine import WIRE_SIZES
    from jylis_amd.repo import REPOS
    O = oracle_mod
    rng = np.random.default_rng(850 + ctype)
    ops = _random_ops(O, ctype, O.Repo(ctype, IDENT), rng, 120)
    a, b = REPOS[ctype](engine, IDENT), REPOS[ctype](engine2, IDENT)
    _apply(ctype, a, ops)
    _apply(ctype, b, ops)
    col = engine.replica_col(IDENT)
    pending = _deltas_size(ctype, engine)
    need, _ = engine.flush_wire_caps(ctype, [0] * len(WIRE_SIZES[ctype]), col=col)
    assert need[0] == pending > 0 and need[1] > 0
    for i, total in enumerate(need):
        if total == 0:
            continue  # (nothing of this kind is pending: no capacity can be short)
        caps = list(need)
        caps[i] -= 1
        sizes, out = engine.flush_wire_caps(ctype, caps, col=col)
        assert sizes == need, WIRE_SIZES[ctype][i]
        assert not any(np.asarray(v).any() for v in out.values()), WIRE_SIZES[ctype][i]
        assert _deltas_size(ctype, engine) == pending
    sizes, out = engine.flush_wire_caps(ctype, need, col=col)
    fresh = engine2.flush_wire(ctype, col=engine2.replica_col(IDENT))
    assert sizes == need and list(out) == list(fresh)
    for k in fresh:
        np.testing.assert_array_equal(out[k], fresh[k], err_msg=k)
    assert _deltas_size(ctype, engine) == 0
    assert len(_flush_slots(ctype, a)["key_offs"]) == 1
    assert engine.flush_wire_caps(ctype, need, col=col)[0] == [0] * len(need)


# 6 ---------------------------------------------------------------------------
def test_device_interned_names(engine):
    """keys interned from HBM (jy_keys_intern_mem): no host name table, no jy_keys_export"""
    import torch
    from jylis_amd.engine import encode_keys
    keys = [b"dev-%d-" % i + b"x" * (i % 23) for i in range(300)]
    kb, ko = encode_keys(keys)
    slots = engine.intern_device(2, torch.from_numpy(kb.copy()).to("cuda:0"),
                                 torch.from_numpy(ko.view(np.int64).copy()).to("cuda:0")).cpu().numpy()
    pick = np.arange(0, 300, 3)
    vals = [b"value-of-%d" % i for i in pick]
    pre, lr = engine.pack_values(2, vals)
    engine.treg_set(slots[pick].view(np.uint32), np.full(len(pick), 9, np.uint64), pre, lr)
    w = engine.flush_wire(2)
    order = np.argsort(slots[pick], kind="stable")
    assert _strings(w["key_bytes"], w["key_offs"]) == [keys[pick[i]] for i in order]
    assert _strings(w["val_bytes"], w["val_offs"]) == [vals[i] for i in order]
    assert "_slot_names" not in engine.__dict__


# 7 ---------------------------------------------------------------------------
def test_structural_cases(oracle_mod, engine):
    from jylis_amd.repo import RepoPNCOUNT, RepoTLOG, RepoTREG, RepoUJSON
    O = oracle_mod
    # TLOG: a cutoff-only delta (TRIMAT after the entry was flushed), beside a key with an entry
    wl, gl = O.Repo(O.TLOG, IDENT), RepoTLOG(engine)
    wl.tlog_ins("cut", b"old", 5), gl.write([("INS", "cut", b"old", 5)])
    wl.flush(), gl.flush_wire()
    wl.tlog_trimat("cut", 9), wl.tlog_ins("ent", b"fresh-entry-value", 7)
    gl.write([("TRIMAT", "cut", 9), ("INS", "ent", b"fresh-entry-value", 7)])
    t = gl.flush_wire()
    assert_state_equal(O.TLOG, _by_key(O.TLOG, wl.flush().table()), _by_key(O.TLOG, t))
    assert t["ent_offs"].tolist() == [0, 0, 1] and t["cutoff"].tolist() == [9, 0]
    # TREG: a key whose SET only lost
    wr, gr = O.Repo(O.TREG, IDENT), RepoTREG(engine)
    wr.treg_set("reg", b"winner", 5), gr.set(["reg"], [b"winner"], [5])
    wr.flush(), gr.flush_wire()
    wr.treg_set("reg", b"loser-longer-than-eight", 1), gr.set(["reg"], [b"loser-longer-than-eight"], [1])
    t = gr.flush_wire()
    assert_state_equal(O.TREG, wr.flush().table(), t)
    assert t["ts"].tolist() == [0] and t["val_offs"].tolist() == [0, 0]
    # UJSON: a cloud dot and no elements (RM of a flushed insert: its dot, the
    # replica's second, cannot fold into the delta's empty version vector)
    wu, gu = O.Repo(O.UJSON, IDENT), RepoUJSON(engine)
    for e in (3, 4):
        wu.ujson_ins("doc", e)
    gu.write([("INS", "doc", 3), ("INS", "doc", 4)], IDENT)
    wu.flush(), gu.flush_wire()
    wu.ujson_rm("doc", 4), gu.write([("RM", "doc", 4)], IDENT)
    t = gu.flush_wire()
    assert_state_equal(O.UJSON, wu.flush().table(), t)
    assert t["el_offs"].tolist() == [0, 0] and t["cloud_offs"].tolist() == [0, 1]
    # PNCOUNT: a key with only DEC
    wp, gp = O.Repo(O.PNCOUNT, IDENT), RepoPNCOUNT(engine, IDENT)
    wp.pncount_dec("down", 7), gp.dec(["down"], [7], IDENT)
    t = gp.flush_wire()
    assert_state_equal(O.PNCOUNT, wp.flush().table(), t)
    assert t["p_offs"].tolist() == [0, 0] and t["n_offs"].tolist() == [0, 1] and t["n_vals"].tolist() == [7]


# 8 ---------------------------------------------------------------------------
@pytest.mark.parametrize("ctype", TYPES)
def test_flush_on_a_converges_on_b(oracle_mod, ctype):
    """node A (S = 2, copy fabric): local writes on the owners' engines, one
    wire flush per shard into device memory; node B converges those tensors
    as they are.  B must equal an oracle replica that converged the oracle
    writer's flush.  Nothing is decoded on the host in between."""
    from jylis_amd.engine import key_owner
    from jylis_amd.node import Node
    from jylis_amd.repo import REPOS
    O = oracle_mod
    rng = np.random.default_rng(880 + ctype)
    A, B = Node(2, "copy"), Node(2, "copy")
    try:
        for node in (A, B):  # the same columns on both: no mapping between them
            assert [node.replica_col(r) for r in (OTHER, IDENT)] == [0, 1]
        writer = O.Repo(ctype, IDENT)
        ops = _random_ops(O, ctype, writer, rng, 160, nkeys=24)
        for sh in range(2):
            mine = [o for o in ops if key_owner(o[1], 2) == sh]
            assert mine
            _apply(ctype, REPOS[ctype](A.engine(sh), IDENT), mine)
        batches = A.flush_wire(ctype, device=True, identity=IDENT)
        A.sync()
        for e in A.engines:
            e.sync()
        assert len(batches) == 2 and all(v.is_cuda for w in batches for v in w.values())
        for w in batches:
            assert w["key_offs"].numel() > 1
            B.converge_wire(ctype, w)
        B.sync()
        peer = O.Repo(ctype)
        peer.converge(writer.flush().table())
        rows = {}
        for sh, eng in enumerate(B.engines):
            part = dict(split_rows(ctype, REPOS[ctype](eng).state()))
            assert all(key_owner(k, 2) == sh for k in part)
            rows.update(part)
        assert_state_equal(ctype, _by_key(ctype, peer.state()), join_rows(ctype, rows))
        assert all(_deltas_size(ctype, e) == 0 for e in A.engines)
    finally:
        A.close()
        B.close()


def test_node_flush_to_host_is_one_table(oracle_mod):
    """Node.flush_wire(device=False): the shards' rows in one oracle-format table"""
    from jylis_amd.engine import key_owner
    from jylis_amd.node import Node
    from jylis_amd.repo import RepoTREG
    O = oracle_mod
    A = Node(2, "copy")
    try:
        writer = O.Repo(O.TREG, IDENT)
        ops = _random_ops(O, O.TREG, writer, np.random.default_rng(890), 80, nkeys=24)
        for sh in range(2):
            _apply(O.TREG, RepoTREG(A.engine(sh)), [o for o in ops if key_owner(o[1], 2) == sh])
        t = A.flush_wire(O.TREG)
        assert_state_equal(O.TREG, _by_key(O.TREG, writer.flush().table()), _by_key(O.TREG, t))
    finally:
        A.close()
