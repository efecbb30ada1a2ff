"""The column-block merge stores only the 128-B lines a batch changes.

k_block_max<true> reads the delta and the state of every cell and stores
max(state, delta) for a lane only if a lane of its wave in the same 128-B
line of the slab advanced a cell.  These tests pin that the rule never skips
a store the join needs and never writes outside the run: after EVERY call the
whole exported slab (every column, named in `cols` or not, and every slot
inside and outside the run) is compared with numpy.maximum on uint64.

Shapes: K = 1024 + 18 slots = two 512-cell tiles and a ragged third whose
only wave holds one full 8-lane group and one more vector; R = 3 columns out
of 4 registered, in a non-identity order; GCOUNT (1 sign) and PNCOUNT (2
signs, so rows > 1 and the sign pitch is used)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 1024 + 18   # slots of a full run
KT = 1280       # interned slots: the ragged last wave (cells 1024..1151) ends inside the export
XCOLS = 8       # exported columns: 4 registered (3 merged into, 1 never) + 4 never registered
ORDER = [2, 0, 3]


class Slab:
    """one counter type of one engine beside its numpy model"""

    def __init__(self, engine, ctype):
        from jylis_amd import synth as S
        self.e, self.ctype, self.nsigns = engine, ctype, 1 + ctype
        slots = engine.intern(ctype, S.counter_keys(KT))
        assert (slots == np.arange(KT)).all()
        cols = engine.replica_cols([11, 22, 33, 44])
        assert (cols == np.arange(4)).all()
        self.cols = cols[ORDER]
        self.exp = np.zeros((self.nsigns, XCOLS, KT), np.uint64)

    def export(self):
        return self.e.counter_export(self.ctype, XCOLS, 0, KT)

    def state(self, slot0=0, n=K):
        """the model's cells of a run, shaped like a batch: [sign][3][n]"""
        return self.exp[:, self.cols.astype(np.int64), slot0:slot0 + n].copy()

    def apply(self, slot0, vals, what):
        """one converge_block of vals [sign][3][n] at slot0, then the whole slab against the model"""
        vals = np.ascontiguousarray(vals, np.uint64)
        assert vals.shape[:2] == (self.nsigns, 3)
        n = vals.shape[2]
        if self.ctype == 0:
            self.e.gcount_converge_block(self.cols, slot0, vals[0])
        else:
            self.e.pncount_converge_block(self.cols, slot0, vals[0], vals[1])
        for c, col in enumerate(self.cols):
            run = self.exp[:, int(col), slot0:slot0 + n]
            np.maximum(run, vals[:, c], out=run)
        got = self.export()
        np.testing.assert_array_equal(got, self.exp, err_msg=what)
        return got


def _seeded(nsigns, n, seed):
    from jylis_amd import synth as S
    return S.counter_state_np(n, 3, nsigns, seed, wrap_frac=False)


# cells of the full run at slot0 = 0 (a vector is 2 cells, an 8-lane group 16,
# a wave 128, a tile 512)
POSITIONS = [
    0, 1,            # first slot of the run; .x and .y of lane 0 (first lane of a group and of a wave)
    14, 15,          # last lane of the first 8-lane group
    16, 17,          # first lane of the second group
    112, 113,        # first lane of the last group of wave 0
    126, 127,        # last lane of wave 0
    128, 129,        # first lane of wave 1
    510, 511, 512,   # last lane of tile 0, first of tile 1
    1022, 1023,      # last lane of the last full wave
    1024,            # first lane of the ragged last wave
    1038, 1039,      # the last full vector of the last full group before the tail
    1040, 1041,      # the ragged group of the last wave; the last slot of the run
]


@pytest.mark.parametrize("ctype", [0, 1])
def test_one_changed_cell_in_a_stale_batch(engine, ctype):
    sl = Slab(engine, ctype)
    sl.apply(0, _seeded(sl.nsigns, K, 5), "initial state")
    for j, p in enumerate(POSITIONS):
        sg, c = j % sl.nsigns, j % 3
        d = sl.state()
        d[sg, c, p] += np.uint64(1 + j)
        sl.apply(0, d, f"one changed cell: slot {p} sign {sg} batch column {c}")
        assert sl.exp[sg, int(sl.cols[c]), p] == d[sg, c, p]
    # the same with everything else strictly behind the state, not equal to it
    for j, p in enumerate(POSITIONS[::3]):
        sg, c = (j + 1) % sl.nsigns, (j + 2) % 3
        d = sl.state() - np.uint64(1)
        d[sg, c, p] += np.uint64(2)
        sl.apply(0, d, f"one changed cell among cells behind the state: slot {p}")


# (state, delta): the compare is unsigned and 64 bits wide
WIDTH = [
    (0x0000000100000005, 0x0000000100000006),  # differs in the low 32 bits only: delta wins
    (0x0000000100000006, 0x0000000100000005),  # ... state wins
    (0x0000000100000000, 0x0000000200000000),  # differs in the high 32 bits only: delta wins
    (0x0000000200000000, 0x00000001FFFFFFFF),  # high says state, low says delta: state wins
    (0x00000001FFFFFFFF, 0x0000000200000000),  # high says delta, low says state: delta wins
    (0x7FFFFFFFFFFFFFFF, 0x8000000000000000),  # delta >= 2^63 against state < 2^63: delta wins
    (0x8000000000000005, 0x0000000000000007),  # the reverse: state wins
    (0xFFFFFFFFFFFFFFFF, 0x7FFFFFFFFFFFFFFF),  # state wins
    (0x0000000300000003, 0x0000000300000003),  # equal: nothing changes
    (0x8000000000000000, 0x8000000000000000),  # equal at the sign bit
]


@pytest.mark.parametrize("ctype", [0, 1])
def test_comparison_width(engine, ctype):
    sl = Slab(engine, ctype)
    base = _seeded(sl.nsigns, K, 6) & np.uint64(0xFFFFFFF)
    # each pair alone in its own wave, once in .x and once in .y
    where = [(j % sl.nsigns, j % 3, 128 * (j % 8) + 34 + 2 * (j // 8) + y) for j in range(len(WIDTH)) for y in (0, 1)]
    pairs = [w for w in WIDTH for _ in (0, 1)]
    for (sg, c, p), (s, _) in zip(where, pairs):
        base[sg, c, p] = np.uint64(s)
    sl.apply(0, base, "initial state")
    for (sg, c, p), (s, dv) in zip(where, pairs):
        d = sl.state()
        assert d[sg, c, p] == np.uint64(s)
        d[sg, c, p] = np.uint64(dv)
        sl.apply(0, d, f"state {s:#x} delta {dv:#x} at slot {p}")
        assert sl.exp[sg, int(sl.cols[c]), p] == np.uint64(max(s, dv))


@pytest.mark.parametrize("ctype", [0, 1])
def test_wholly_stale_batch(engine, ctype):
    from jylis_amd import synth as S
    sl = Slab(engine, ctype)
    st = _seeded(sl.nsigns, K, 7)
    sl.apply(0, st, "initial state")
    fresh = S.counter_delta_np(st, 0, 7)
    once = sl.apply(0, fresh, "fresh batch")
    assert (once != sl.apply(0, st, "initial state again")).sum() == 0
    twice = sl.apply(0, fresh, "the same fresh batch again")
    assert once.tobytes() == twice.tobytes()
    behind = sl.state() - np.uint64(3)
    assert sl.apply(0, behind, "every cell behind the state").tobytes() == once.tobytes()
    assert sl.apply(0, np.zeros_like(st), "all zero").tobytes() == once.tobytes()


# (slot0, nslots): even slot0 off the 16-slot line grid, partial groups at
# both ends, runs inside one or two lines, and the scalar kernel's odd runs
RUNS = [(2, 1040), (14, 1030), (16, 1026), (6, 20), (10, 4), (30, 2), (254, 516),
        (1, 1041), (3, 1000), (2, 1037), (15, 1), (0, 1041)]


@pytest.mark.parametrize("ctype", [0, 1])
def test_alignment(engine, ctype):
    from jylis_amd import synth as S
    sl = Slab(engine, ctype)
    sl.apply(0, _seeded(sl.nsigns, KT, 8), "initial state, every interned slot")
    for j, (slot0, n) in enumerate(RUNS):
        tag = f"slot0 {slot0} nslots {n}"
        sl.apply(slot0, S.counter_delta_np(sl.state(slot0, n), j, 8), tag + ": fresh")
        for p in sorted({0, n - 1, n // 2}):
            d = sl.state(slot0, n)
            d[j % sl.nsigns, j % 3, p] += np.uint64(9)
            sl.apply(slot0, d, tag + f": one changed cell at {p} of the run")
        before = sl.export()
        assert sl.apply(slot0, sl.state(slot0, n), tag + ": stale").tobytes() == before.tobytes()


@pytest.mark.parametrize("ctype", [0, 1])
def test_random_mix_out_of_order(engine, ctype):
    """a seeded chain as in test_parity_counters.py, its rounds applied out of
    order so that some cells of every later call are stale"""
    from jylis_amd import synth as S
    sl = Slab(engine, ctype)
    seed = S.BASE_SEED + 1 + ctype
    st = S.counter_state_np(K, 3, sl.nsigns, seed, wrap_frac=(ctype == 1))
    sl.apply(0, st, "initial state")
    chain, cur = [], st
    for rnd in range(3):
        cur = S.counter_delta_np(cur, rnd, seed)
        chain.append(cur)
    for rnd in (2, 0, 1, 2):
        sl.apply(0, chain[rnd], f"round {rnd}")
    want = st
    for b in chain:
        want = np.maximum(want, b)
    np.testing.assert_array_equal(sl.state(), want)
