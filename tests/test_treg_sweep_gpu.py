"""TREG merges (k_treg.hip) swept along their own geometry, against the CPU
oracle: treg_cases.py builds the cases (the order matrix, claim layouts, fold
depths, dense blocks, SETs, routed batches; every keyed sweep again in the
whole-line form).  Around EVERY engine call: the state is read first (a read
folds) and the pending duplicate list is then empty; after the call
Engine.treg_claim_info() counts exactly the duplicates the launch declares (a
SET batch folds its own repeats inside the call: 0 there); a raw read of EVERY
interned slot equals the model's (ts, prefix, length), and every slot that no
entry replaced is bit-identical to before, arena reference included;
Engine.skipped() moved by what the launch declares.  The state is compared
with the oracle's (assert_state_equal, value bytes read back from the arena)
at each sweep's end: per call the whole-file raw read against the model, which
test_treg_sweep_cpu.py holds against the oracle, is the check.
test_treg_sweep_cpu.py checks the same cases against the oracle alone."""
import numpy as np
import pytest

import treg_cases as C
from helpers import assert_state_equal
from test_route_gpu import _Node, _dev

pytestmark = pytest.mark.gpu

LEN_MASK = np.uint64((1 << 24) - 1)
N_CLAIM, N_DENSE = 40000, 2200
WHOLE = pytest.mark.parametrize("flags", [0, 1], ids=["lean", "whole-lines"])  # g. CFG_TREG_WHOLE_LINES
MEM = pytest.mark.parametrize("device", [False, True], ids=["host", "device"])


class _File:
    """an engine's register file of n slots next to the model and the oracle"""

    def __init__(self, O, flags, n):
        from jylis_amd.engine import Engine, encode_keys
        self.O, self.n = O, n
        self.eng = Engine(device=0, flags=flags, key_capacity=max(n, 1024))
        keys = [C.key_of(s) for s in range(n)]
        self.all = np.arange(n, dtype=np.uint32)
        assert (self.eng.intern(O.TREG, keys) == self.all).all()
        kb, ko = encode_keys(keys)
        self.want = O.Repo(O.TREG, 9)
        self.want.converge({"key_bytes": kb, "key_offs": ko, "ts": np.zeros(n, np.uint64),
                            "val_bytes": np.zeros(0, np.uint8), "val_offs": np.zeros(n + 1, np.uint64)})
        self.eng.treg_converge(self.all[:1], np.zeros(1, np.uint64), np.zeros(1, np.uint64), np.zeros(1, np.uint64))
        self.model = C.Model(n)
        self.ts, self.pre, self.len = (np.zeros(n, np.uint64) for _ in range(3))
        self.raw = self.eng.treg_read(self.all)

    def close(self):
        self.eng.close()

    def apply(self, L, device=False):
        eng, O = self.eng, self.O
        assert eng.treg_claim_info()["pending"] == 0  # the read before folded
        pre, lr = eng.pack_values(O.TREG, L["vals"])
        ts = np.array(L["ts"], np.uint64)
        args = (ts, pre, lr) if L["kind"] == "block" else (L["slots"], ts, pre, lr)
        if device or L["device_only"]:
            args = [_dev(a, None) for a in args]
        skipped = eng.skipped()
        if L["kind"] == "block":
            eng.treg_converge_block(L["slot0"], *args)
        else:
            (eng.treg_set if L["kind"] == "set" else eng.treg_converge)(*args)
        # jy_treg_set_batch folds its own repeats inside the call; a block launch claims nothing
        assert eng.treg_claim_info()["pending"] == (L["dups"] if L["kind"] == "keyed" else 0)
        if L["kind"] == "set":
            for s, t, v in zip(L["slots"], L["ts"], L["vals"]):
                self.want.treg_set(C.key_of(int(s)), v, t)
        else:
            self.want.converge(C.table(L))
        hit = sorted(self.model.apply(L))
        for s in hit:
            v = self.model.val[s]
            self.ts[s], self.pre[s], self.len[s] = self.model.ts[s], C.pre_of(v), len(v)
        raw = eng.treg_read(self.all)
        assert eng.treg_claim_info()["pending"] == 0
        np.testing.assert_array_equal(raw[0], self.ts)
        np.testing.assert_array_equal(raw[1], self.pre)
        np.testing.assert_array_equal(raw[2] & LEN_MASK, self.len)
        same = np.ones(self.n, bool)
        same[hit] = False
        for new, old in zip(raw, self.raw):  # not replaced: bit-identical, the arena reference included
            np.testing.assert_array_equal(new[same], old[same])
        assert eng.skipped() - skipped == L["skips"]
        self.raw = raw
        return set(hit)

    def run(self, cases, device=False):
        for c in cases:
            for L in c["launches"]:
                hit = self.apply(L, device)
            if c["expect"] is not None:
                for s, (t, v) in c["expect"].items():
                    assert (self.model.ts[s], self.model.val[s]) == (t, v), (c["name"], s)
            assert not (c["same_lr"] & hit), c["name"]

    def check_oracle(self):
        from jylis_amd.repo import RepoTREG
        assert_state_equal(self.O.TREG, self.want.state(), RepoTREG(self.eng).state())


def _sweep(O, flags, n, cases, device=False):
    f = _File(O, flags, n)
    try:
        f.run(cases, device)
        f.check_oracle()
        return f
    except BaseException:
        f.close()
        raise


@WHOLE
@MEM
@pytest.mark.parametrize("reps", [1, 6])
def test_order_matrix(oracle_mod, flags, device, reps):
    """a. every (state, delta) pair through the keyed form; reps = 6 names each probe's slot six times, so
    the probes also pass through the three fold rounds and the one-wave tail"""
    pairs = C.order_pairs()
    _sweep(oracle_mod, flags, len(pairs), [C.order_case(pairs, "keyed", reps)], device).close()


@WHOLE
@MEM
def test_order_matrix_dense(oracle_mod, flags, device):
    """a. in the dense form: the pairs as two block batches at slot 65"""
    pairs = C.order_pairs()
    _sweep(oracle_mod, flags, 65 + len(pairs), [C.order_case(pairs, block_at=65)], device).close()


@WHOLE
def test_claim_geometry(oracle_mod, flags):
    """b. every layout in three consecutive launches at fresh timestamps over a file whose bitmaps a launch
    of up to 1,024 entries resets by memset and a larger one slice by slice; odd layouts from device memory"""
    f = _File(oracle_mod, flags, N_CLAIM)
    try:
        info = f.eng.treg_claim_info()
        assert info["seen_words"] * 32 >= N_CLAIM and 4096 < info["seen_words"] * 4 <= 8192
        assert {k: info[k] for k in ("unroll", "routed_unroll", "fold_rounds", "tile")} == \
            {"unroll": C.UNROLL, "routed_unroll": C.ROUTED_UNROLL, "fold_rounds": C.FOLD_ROUNDS, "tile": C.TILE}
        clock = C._Clock()
        for i, lay in enumerate(C.claim_layouts(N_CLAIM, info["seen_words"])):
            f.run([C.geometry_case(lay, clock)], device=i % 2 == 1)
        f.check_oracle()
    finally:
        f.close()


def test_no_slot_in_a_host_batch(oracle_mod):
    """b. jy_treg_converge checks a host batch's slots (slots_check): JY_NO_SLOT there is refused with
    JY_ERANGE and nothing is merged; only a device batch carries such entries to the kernel, which skips them"""
    from jylis_amd._lib import JY_ERANGE
    from jylis_amd.engine import EngineError
    f = _File(oracle_mod, 0, 64)
    try:
        L = C.launch("keyed", [3, C.NO_SLOT, 5], [9, 9, 9], [b"a", b"b", b"c"])
        pre, lr = f.eng.pack_values(oracle_mod.TREG, L["vals"])
        with pytest.raises(EngineError) as ei:
            f.eng.treg_converge(L["slots"], np.array(L["ts"], np.uint64), pre, lr)
        assert ei.value.code == JY_ERANGE
        for new, old in zip(f.eng.treg_read(f.all), f.raw):
            np.testing.assert_array_equal(new, old)
        L["device_only"] = True
        assert f.apply(L) == {3, 5}
        f.check_oracle()
    finally:
        f.close()


@WHOLE
@MEM
def test_fold_depth(oracle_mod, flags, device):
    """c. one slot named m times in one launch, for every m around the fold's rounds and the tail's chunks"""
    cases, n = C.fold_cases()
    _sweep(oracle_mod, flags, n, cases, device).close()


@WHOLE
@MEM
def test_dense_blocks(oracle_mod, flags, device):
    """d. block batches at every start and size; one winner in a stale batch; all stale; equal to the state"""
    _sweep(oracle_mod, flags, N_DENSE, C.dense_cases(N_DENSE), device).close()


def _flushed(f):
    slots, ts, pre, lr = f.eng.treg_flush()
    return {C.key_of(int(s)): (int(t), f.eng.value_bytes(f.O.TREG, p, l)) for s, t, p, l in zip(slots, ts, pre, lr)}


def _oracle_flushed(f):
    t = f.want.flush().table()
    vb, vo = bytes(np.asarray(t["val_bytes"], np.uint8)), t["val_offs"]
    return {k: (int(x), vb[int(vo[i]):int(vo[i + 1])]) for i, (k, x) in enumerate(zip(f.O.split_keys(t), t["ts"]))}


@MEM
@pytest.mark.parametrize("sweep", ["order", "order x6", "fold"])
def test_set(oracle_mod, device, sweep):
    """e. the order matrix and the fold depths as local SETs: state, deltas_size and the flushed delta are the
    oracle's (a losing SET still creates the delta key, with ("", 0))"""
    pairs = C.order_pairs()
    if sweep == "fold":
        cases, n = C.fold_cases("set")
    else:
        cases, n = [C.order_case(pairs, "set", 6 if "x6" in sweep else 1)], len(pairs)
    f = _sweep(oracle_mod, 0, n, cases, device)
    try:
        assert f.eng.treg_deltas_size() == f.want.deltas_size() > 0
        got = _flushed(f)
        assert got == _oracle_flushed(f)
        if sweep != "fold":
            assert got == {C.key_of(i): p["delta"] if p["replaced"] else (0, b"") for i, p in enumerate(pairs)}
        assert f.eng.treg_deltas_size() == 0
    finally:
        f.close()


@pytest.mark.parametrize("direct", [True, False])
def test_routed_and_owned(oracle_mod, direct):
    """f. the order matrix through TregRouter on LocalFabric, S = 2: every pair on a key of each owner; a
    pair's state is ingested on one rank and its delta on the other, so each register meets its delta once
    from a peer's run (the value bytes rebased into the owner's arena) and once from the shard's own batch"""
    from jylis_amd.engine import encode_keys
    from jylis_amd.route import LocalFabric, TregRouter, owners
    O, pairs = oracle_mod, C.order_pairs()
    own = lambda k: int(owners(np.frombuffer(k, np.uint8), np.array([0, len(k)], np.uint64), 2)[0])
    keys = C.routed_keys(pairs, own)

    def batch(idx, what):
        ks = [k for i in idx for k in keys[i]]
        ents = [pairs[i][what] for i in idx for _ in keys[i]]
        kb, ko = encode_keys(ks)
        vb, vo = encode_keys([v for _, v in ents])
        return {"key_bytes": kb, "key_offs": ko, "ts": np.array([t for t, _ in ents], np.uint64), "val_bytes": vb,
                "val_offs": vo}

    even, odd = list(range(0, len(pairs), 2)), list(range(1, len(pairs), 2))
    node = _Node(2)
    try:
        router = TregRouter(node.engs, LocalFabric(2), self_direct=direct)
        want, held = O.Repo(O.TREG), []
        for bs in ([batch(even, "state"), batch(odd, "state")], [batch(odd, "delta"), batch(even, "delta")]):
            for b in bs:
                want.converge(b)
            held.append([node.ingest(r, b) for r, b in enumerate(bs)])
            router.step(held[-1])
            router.drain()
        for e in node.engs:
            e.sync()
            assert e.treg_claim_info()["pending"] == 0 and e.skipped() == 0  # no key twice in one source's run
        got = node.union_state()
        assert got == {k: (p["expect"][0], p["expect"][1]) for p, row in zip(pairs, keys) for k in row}
        st = want.state()
        vb, vo = bytes(np.asarray(st["val_bytes"], np.uint8)), st["val_offs"]
        assert got == {k: (int(t), vb[int(vo[i]):int(vo[i + 1])]) for i, (k, t) in enumerate(zip(O.split_keys(st), st["ts"]))}
    finally:
        node.close()
