"""The device scan, select and sort primitives on their own (jy_dscan.hpp,
jy_sort.hpp, jy_scan.hpp), and the device round split built on them
(jy_drounds.hpp, against put_ref.units_ref), through the test-only entry
points of tests/prims_check.hip, which include those headers unchanged.

The reference is numpy on the host with exact integers: every comparison is
array_equal.  The sizes are the smallest at which each code path of the
primitives exists (the 2048-item tile, the 8-tile one-workgroup scan, the
2048-chunk and 1024-ticket limits, the 64-word look-back window, the 1024-key
sort block); every output is followed by a sentinel-filled margin that must
come back untouched."""
import ctypes as C
import functools

import numpy as np
import pytest

import prims_lib
import put_ref

pytestmark = pytest.mark.gpu

MARGIN = 256  # items of sentinel after every device array
SENT = {np.dtype(np.uint64): 0xA5A5A5A5A5A5A5A5, np.dtype(np.uint32): 0xA5A5A5A5, np.dtype(np.uint8): 0xA5}
SIGNED = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32, np.dtype(np.uint8): np.uint8}
SUM, MAX = 0, 1
TILE = 2048


@pytest.fixture(scope="module")
def lib():
    return prims_lib.load()


@pytest.fixture(scope="module")
def eng():
    from jylis_amd.engine import Engine
    e = Engine(device=0)
    yield e
    e.close()


def _dev(x):
    """a device copy of the host array x with MARGIN sentinel items after it"""
    import torch
    x = np.ascontiguousarray(x)
    buf = np.full(x.size + MARGIN, SENT[x.dtype], x.dtype)
    buf[:x.size] = x
    return torch.from_numpy(buf.view(SIGNED[x.dtype])).cuda()


def _dev_fill(n, dtype):
    """n + MARGIN sentinel items on the device: an output nothing has written yet"""
    return _dev(np.full(n, SENT[np.dtype(dtype)], dtype))


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


def _check(t, want, what=""):
    """the device array t holds `want`, then nothing but sentinels"""
    want = np.asarray(want)
    got = _host(t, want.dtype)
    np.testing.assert_array_equal(got[:want.size], want, err_msg=what)
    assert (got[want.size:] == SENT[want.dtype]).all(), f"{what}: a store past item {want.size}"


# ---- scan ------------------------------------------------------------------

@functools.lru_cache(maxsize=16)
def _scan_values(n, kind, dtype):
    rng = np.random.default_rng(1000 + n % 9973)
    top = int(np.iinfo(dtype).max)
    if kind == "small":
        x = rng.integers(0, 1000, n, dtype)
    elif kind == "full":  # sums wrap
        x = rng.integers(0, top, n, dtype, endpoint=True)
    elif kind == "zeros":
        x = np.zeros(n, dtype)
    elif kind == "last":
        x = np.zeros(n, dtype)
        x[n - 1:] = top // 3
    elif kind == "ramp":  # descending: the running maximum is item 0 throughout
        x = (top - np.arange(n, dtype=np.uint64)).astype(dtype)
    elif kind == "spike":
        x = rng.integers(0, 1000, n, dtype)
        x[n // 2:n // 2 + 1] = top
    x.setflags(write=False)
    return x


def _scan_ref(x, op, incl):
    x64 = x.astype(np.uint64)
    inc = np.cumsum(x64, dtype=np.uint64) if op == SUM else np.maximum.accumulate(x64)
    if not incl:
        inc = np.concatenate([np.zeros(1, np.uint64), inc[:-1]])[:x.size]
    return inc.astype(x.dtype)  # a u32 storer keeps the low word


def _run_scan(eng, lib, x, op, incl, inplace, what):
    fn = lib.jyt_scan_u64 if x.dtype == np.uint64 else lib.jyt_scan_u32
    din = _dev(x)
    dout = din if inplace else _dev_fill(x.size, x.dtype)
    eng._check(fn(eng.h, op, int(incl), x.size, din.data_ptr(), dout.data_ptr()))
    _check(dout, _scan_ref(x, op, incl), what)
    if not inplace:
        _check(din, x, what + " (the input)")


SCAN_SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049,
              16384,      # the last one-workgroup size
              16385,      # the first three-launch size
              4194304,    # 2048 tiles: T = 1, k_scan_mid completely full
              4194305,    # 2049 tiles: T = 2, a one-item last tile
              4196353]    # 2050 tiles: T = 2, a short last chunk and a one-item last tile


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_scan_sum_exclusive_sizes(eng, lib, n):
    for kind in ("small", "full"):
        _run_scan(eng, lib, _scan_values(n, kind, np.uint64), SUM, False, False, f"n={n} {kind}")


@pytest.mark.parametrize("inplace", [False, True], ids=["separate", "inplace"])
@pytest.mark.parametrize("dtype", [np.uint64, np.uint32], ids=["u64", "u32"])
@pytest.mark.parametrize("incl", [True, False], ids=["incl", "excl"])
@pytest.mark.parametrize("op", [SUM, MAX], ids=["sum", "max"])
@pytest.mark.parametrize("n", [1, 2049, 16385, 4196353])
def test_scan_matrix(eng, lib, n, op, incl, dtype, inplace):
    kinds = ("small", "full", "zeros", "last") + (("ramp", "spike") if op == MAX else ())
    for kind in kinds:
        _run_scan(eng, lib, _scan_values(n, kind, dtype), op, incl, inplace, f"n={n} {kind}")


@pytest.mark.parametrize("rows,W", [(1, 1), (3, 5), (2048, 2), (2049, 7), (9, 2048)])
def test_scan_colmajor(eng, lib, rows, W):
    rng = np.random.default_rng(rows * 31 + W)
    for top in (1000, 2**64 - 1):
        m = rng.integers(0, top, (rows, W), np.uint64, endpoint=True)
        a = _dev(np.concatenate([m.ravel(), np.array([12345], np.uint64)]))  # the extra word is never read
        eng._check(lib.jyt_scan_colmajor(eng.h, rows, W, a.data_ptr()))
        flat = m.T.ravel()  # column after column
        inc = np.cumsum(flat, dtype=np.uint64)
        exc = np.concatenate([np.zeros(1, np.uint64), inc[:-1]])
        want = np.concatenate([exc.reshape(W, rows).T.ravel(), inc[-1:]])  # a[rows * W] = the grand total
        _check(a, want, f"{rows}x{W} top={top}")


# ---- select ----------------------------------------------------------------

SELECT_SIZES = [0, 1, 2047, 2048, 2049,
                64 * TILE + 1, 130 * TILE + 5,  # the look-back walks beyond one window, beyond two
                2097152,                        # 1024 tiles: G = 1
                2097153, 2099201]               # G = 2: the last workgroup holds one tile, two
PATTERNS = ["none", "all", "first", "last", "every2049", "p0.001", "p0.5", "p0.999"]


def _flags(n, pattern, seed=0):
    f = np.zeros(n, np.uint8)
    if pattern == "all":
        f[:] = 1
    elif pattern == "first":
        f[:1] = 1
    elif pattern == "last":
        f[n - 1:] = 1
    elif pattern == "every2049":
        f[::2049] = 1
    elif pattern.startswith("p"):
        f = (np.random.default_rng(n % 9973 + seed).random(n) < float(pattern[1:])).astype(np.uint8)
    return f


def _run_select(eng, lib, f, what):
    n = f.size
    dflags, out, count = _dev(f), _dev_fill(n, np.uint32), _dev_fill(1, np.uint32)
    eng._check(lib.jyt_select_flags(eng.h, n, dflags.data_ptr(), out.data_ptr(), count.data_ptr()))
    want = np.flatnonzero(f).astype(np.uint32)
    _check(count, np.array([want.size], np.uint32), what + " count")
    got = _host(out, np.uint32)
    np.testing.assert_array_equal(got[:want.size], want, err_msg=what)
    assert (got[want.size:] == SENT[np.dtype(np.uint32)]).all(), f"{what}: a store past the count"


@pytest.mark.parametrize("n,pattern", [(n, p) for n in SELECT_SIZES for p in (PATTERNS if n else ["none"])])
def test_select(eng, lib, n, pattern):
    _run_select(eng, lib, _flags(n, pattern), f"n={n} {pattern}")


def test_select_growth_and_reuse(engine, lib):
    """a fresh engine: the status array grows for the large launch, and the
    small one after it meets the large one's words"""
    for n in (10, 2099201, 10):
        _run_select(engine, lib, _flags(n, "p0.5", seed=n), f"n={n}")


def test_select_epoch_wrap(engine, lib):
    """the 22-bit epoch of the status words wraps to 1, never 0, and counts on"""
    lib.jyt_dscan_epoch_set(engine.h, 2**22 - 4)
    for i in range(8):  # epochs 2^22 - 3, - 2, - 1, then 1, 2, 3, 4, 5
        _run_select(engine, lib, _flags(130 * TILE, "p0.5", seed=100 + i), f"select {i}")
    assert lib.jyt_dscan_epoch_get(engine.h) == 5


@pytest.mark.parametrize("n", [0, 1, 2047, 2048, 2049, 64 * TILE + 1, 130 * TILE + 5])
@pytest.mark.parametrize("kind", ["random", "ones"])
def test_lookback_scan(eng, lib, n, kind):
    """the non-generic jyscan::lookback under tickets (sums stay below 2^40)"""
    x = np.random.default_rng(n % 9973).integers(0, 2**20, n, np.uint32) if kind == "random" else np.ones(n, np.uint32)
    din, out = _dev(x), _dev_fill(n, np.uint64)
    eng._check(lib.jyt_lookback_scan(eng.h, n, din.data_ptr(), out.data_ptr()))
    _check(out, _scan_ref(x.astype(np.uint64), SUM, False), f"n={n}")


# ---- sort ------------------------------------------------------------------

SORT_SIZES = [0, 1, 2, 255, 256, 257, 1023, 1024, 1025, 4099, 65536,
              66561]  # 66 blocks: the histogram scan has 16,896 items (three launches)
SORT_RANGES = [(0, 8), (0, 64), (32, 40), (32, 43), (32, 33), (5, 18), (7, 7), (56, 64)]


def _sort_keys(n, lo, hi, kind, rng):
    """random u64 keys, every bit live; `kind` shapes the field [lo, hi) alone"""
    keys = rng.integers(0, 2**64 - 1, n, np.uint64, endpoint=True)
    w = hi - lo
    if kind == "random" or w == 0:
        return keys
    top = (1 << w) - 1
    if kind == "equal":
        f = np.full(n, rng.integers(0, top, dtype=np.uint64, endpoint=True), np.uint64)
    elif kind == "two":
        f = rng.choice(rng.integers(0, top, 2, np.uint64, endpoint=True), n)
    else:
        f = np.sort(rng.integers(0, top, n, np.uint64, endpoint=True))
        if kind == "reverse":
            f = f[::-1]
    return (keys & ~np.uint64(top << lo)) | (f << np.uint64(lo))


@pytest.mark.parametrize("lo,hi", SORT_RANGES)
@pytest.mark.parametrize("n", SORT_SIZES)
def test_sort_bits(eng, lib, n, lo, hi):
    rng = np.random.default_rng(n * 64 + lo + hi)
    hw = lib.jyt_sort_hist_words(n)
    passes = 0 if n < 2 else -(-(hi - lo) // 8)
    for kind in ("random", "equal", "two", "sorted", "reverse"):
        keys = _sort_keys(n, lo, hi, kind, rng)
        a, b, hist = _dev(keys), _dev_fill(n, np.uint64), _dev_fill(hw, np.uint64)
        which = C.c_int32(-7)
        eng._check(lib.jyt_sort_bits(eng.h, n, a.data_ptr(), b.data_ptr(), hist.data_ptr(), lo, hi, C.byref(which)))
        assert which.value == passes & 1  # no pass: the result stays in a
        field = (keys >> np.uint64(lo)) & np.uint64((1 << (hi - lo)) - 1)
        want = keys[np.argsort(field, kind="stable")]  # stable, and by nothing outside [lo, hi)
        what = f"n={n} [{lo},{hi}) {kind}"
        _check(b if which.value else a, want, what)
        for t in (a if which.value else b, hist):  # the other buffer and the histogram: nothing past their end
            got = _host(t, np.uint64)
            assert (got[-MARGIN:] == SENT[np.dtype(np.uint64)]).all(), what
            assert passes or (got == SENT[np.dtype(np.uint64)]).all(), what


def test_sort_sizes_pinned(lib):
    assert [lib.jyt_sort_bits_for(c) for c in (0, 1, 2, 3, 256, 257, 2**32, 2**63 + 1)] == [0, 0, 1, 2, 8, 9, 32, 64]
    for n in SORT_SIZES:
        assert lib.jyt_sort_hist_words(n) == max(1, -(-n // 1024)) * 256 + 1


# ---- wave_last_le ------------------------------------------------------------

@pytest.mark.parametrize("shape", ["mixed", "unit", "empty"])
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 4095, 4096, 4097, 262145])  # 1 to 4 levels of the 64-ary search
def test_wave_last_le(eng, lib, n, shape):
    rng = np.random.default_rng(n + 5)
    if shape == "mixed":  # runs of equal offsets (empty segments) at the start, in the middle and at the end
        lens = rng.choice(np.array([0, 0, 1, 2, 3, 17, 300], np.uint64), n)
        k = min(5, n // 4)
        for s in (0, n // 2, n - k):
            lens[s:s + k] = 0
    else:
        lens = np.full(n, 1 if shape == "unit" else 0, np.uint64)
    offs = np.concatenate([np.zeros(1, np.uint64), np.cumsum(lens, dtype=np.uint64)])
    end = int(offs[n])
    x = np.concatenate([offs, offs + np.uint64(1), offs[offs > 0] - np.uint64(1),
                        np.array([0, max(end - 1, 0), end, end + 5], np.uint64)])
    doffs, dx, out = _dev(offs), _dev(x), _dev_fill(x.size, np.uint64)
    eng._check(lib.jyt_last_le(eng.h, n, doffs.data_ptr(), x.size, dx.data_ptr(), out.data_ptr()))
    want = (np.searchsorted(offs, x, "right") - 1).astype(np.uint64)  # the last k in [0, n] with offs[k] <= x
    _check(out, want, f"n={n} {shape}")


# ---- block_excl --------------------------------------------------------------

@pytest.mark.parametrize("kind", ["random", "ones"])
@pytest.mark.parametrize("threads", [256, 1024])  # the widths the engine instantiates
def test_block_excl(eng, lib, threads, kind):
    nb = 3
    x = (np.random.default_rng(threads).integers(0, 2**64 - 1, nb * threads, np.uint64, endpoint=True)
         if kind == "random" else np.ones(nb * threads, np.uint64))
    din, pre, tot = _dev(x), _dev_fill(x.size, np.uint64), _dev_fill(nb, np.uint64)
    eng._check(lib.jyt_block_excl(eng.h, threads, nb, din.data_ptr(), pre.data_ptr(), tot.data_ptr()))
    inc = np.cumsum(x.reshape(nb, threads), axis=1, dtype=np.uint64)  # wraps mod 2^64 like the kernel
    _check(pre, (inc - x.reshape(nb, threads)).ravel(), "prefix")
    _check(tot, inc[:, -1], "total")


# ---- the device round split ------------------------------------------------------

def _one_slot(k, others, op=None):
    """slot 7 named k times among `others` slots named once, shuffled; ops all INS, or op(j) for slot 7's j-th"""
    rng = np.random.default_rng(k * 31 + others)
    slots = np.concatenate([np.full(k, 7, np.uint32), 100 + np.arange(others, dtype=np.uint32)])
    slots = slots[rng.permutation(slots.size)]
    ops = np.full(slots.size, put_ref.INS, np.uint8)
    if op:
        ops[slots == 7] = [op(j) for j in range(k)]
    return ops, slots


def _broken_run(at):
    """ten INS to slot 3 with the one at `at` a TRIM, five INS to slot 1 in between"""
    slots = np.array([3, 1, 3, 3, 1, 3, 3, 1, 3, 3, 1, 3, 3, 1, 3], np.uint32)
    ops = np.full(slots.size, put_ref.INS, np.uint8)
    ops[np.flatnonzero(slots == 3)[at]] = put_ref.TRIM
    return ops, slots


def _zipf(n):
    rng = np.random.default_rng(65537)
    return rng.integers(0, 4, n).astype(np.uint8) * (rng.random(n) < 0.3), (rng.zipf(1.3, n) % 5000).astype(np.uint32)


DROUNDS_CASES = {
    "n1": lambda: (np.array([put_ref.TRIM], np.uint8), np.array([5], np.uint32)),
    "n2_same_slot": lambda: (np.array([put_ref.INS, put_ref.INS], np.uint8), np.array([9, 9], np.uint32)),
    "slot_x63": lambda: _one_slot(63, 20),
    "slot_x64": lambda: _one_slot(64, 20),
    "slot_x65": lambda: _one_slot(65, 20),
    "slot_x130": lambda: _one_slot(130, 20),
    "run_broken_first": lambda: _broken_run(0),
    "run_broken_middle": lambda: _broken_run(5),
    "run_broken_last": lambda: _broken_run(9),
    "distinct_2048": lambda: (np.zeros(2048, np.uint8), np.random.default_rng(1).permutation(2048).astype(np.uint32)),
    "distinct_2049": lambda: (np.zeros(2049, np.uint8), np.random.default_rng(2).permutation(2049).astype(np.uint32)),
    "zipf_65537": lambda: _zipf(65537),
}


def _run_drounds(eng, lib, ops, slots, unit_max, idx=None):
    ops, slots = np.ascontiguousarray(ops, np.uint8), np.ascontiguousarray(slots, np.uint32)
    sel = np.arange(ops.size, dtype=np.uint32) if idx is None else np.ascontiguousarray(idx, np.uint32)
    n = sel.size
    want = put_ref.units_ref(ops[sel], slots[sel], unit_max)
    dslot, dop = _dev(slots), _dev(ops)
    didx = None if idx is None else _dev(sel)
    h64 = SENT[np.dtype(np.uint64)]
    ru, ro, uoff = np.full(2, h64, np.uint64), np.full(n + 1 + MARGIN, h64, np.uint64), np.full(n + 1 + MARGIN, h64, np.uint64)
    uslot, cmd = np.full(n + MARGIN, 0xA5A5A5A5, np.uint32), np.full(n + MARGIN, 0xA5A5A5A5, np.uint32)
    eng._check(lib.jyt_drounds(eng.h, n, dslot.data_ptr(), didx.data_ptr() if didx is not None else None,
                               dop.data_ptr() if unit_max > 1 else None, put_ref.INS, unit_max,
                               lib.jyt_sort_bits_for(int(slots.max()) + 1), ru.ctypes.data, ro.ctypes.data,
                               uslot.ctypes.data, uoff.ctypes.data, cmd.ctypes.data))
    rounds = np.array([r for r, _, _ in want], np.int64)
    R, U = int(rounds.max()) + 1, len(want)
    assert (int(ru[0]), int(ru[1])) == (R, U)
    np.testing.assert_array_equal(ro[:R + 1], np.searchsorted(rounds, np.arange(R + 1)))
    np.testing.assert_array_equal(uslot[:U], [s for _, s, _ in want])
    np.testing.assert_array_equal(uoff[:U + 1], np.concatenate([[0], np.cumsum([len(ix) for _, _, ix in want])]))
    np.testing.assert_array_equal(cmd[:n], sel[np.concatenate([ix for _, _, ix in want])])
    assert (ro[R + 1:] == h64).all() and (uoff[U + 1:] == h64).all()
    assert (uslot[U:] == 0xA5A5A5A5).all() and (cmd[n:] == 0xA5A5A5A5).all()
    _check(dslot, slots, "the slots")  # the inputs as they were
    _check(dop, ops, "the ops")
    if didx is not None:
        _check(didx, sel, "the index list")
    return R, U


@pytest.mark.parametrize("unit_max", [64, 1])
@pytest.mark.parametrize("case", sorted(DROUNDS_CASES))
def test_drounds_against_units_ref(eng, lib, case, unit_max):
    """R, U, the round offsets and every unit's slot and commands, in the
    device's order, equal put_ref.units_ref exactly"""
    ops, slots = DROUNDS_CASES[case]()
    _run_drounds(eng, lib, ops, slots, unit_max)


@pytest.mark.parametrize("unit_max", [64, 1])
def test_drounds_index_list(eng, lib, unit_max):
    """an index list that leaves out every third command: the others alone are
    split, and named by their own indices"""
    ops, slots = _one_slot(130, 20)
    idx = np.flatnonzero(np.arange(ops.size) % 3 != 2)
    _run_drounds(eng, lib, ops, slots, unit_max, idx)
    ops, slots = _zipf(4099)
    _run_drounds(eng, lib, ops, slots, unit_max, np.flatnonzero(np.arange(ops.size) % 3 != 0))


@pytest.mark.parametrize("k", [4095, 4096, 4097, 4098])
def test_drounds_readback_boundary_unit_1(eng, lib, k):
    """one slot named k times: k rounds, k + 1 offsets.  The first copy brings
    4,097 offsets back: 4,098 is the first count that needs the second copy."""
    ops, slots = _one_slot(k, 5)
    assert _run_drounds(eng, lib, ops, slots, 1) == (k, k + 5)


def test_drounds_readback_boundary_unit_64(eng, lib):
    """4,097 commands to one slot, INS and TRIM in turn: no two share a unit,
    so 4,097 rounds and 4,098 offsets, the second copy's first count"""
    ops, slots = _one_slot(4097, 5, op=lambda j: put_ref.TRIM if j % 2 else put_ref.INS)
    assert _run_drounds(eng, lib, ops, slots, 64) == (4097, 4097 + 5)
