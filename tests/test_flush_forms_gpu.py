"""The slot-form (jy_*_flush) and wire-form (jy_*_flush_wire) flushes share
one pending set, one peek and one clear per type (k_flush_wire.hip).  What
that sharing can get wrong and the per-form tests do not reach: the two forms
taking turns on ONE engine's pending set, a short capacity that must leave
the set for the other form, and the host-side state the shared clear resets.
257 pending keys: one more than the 256-thread block of the peek and clear
kernels."""
import ctypes as C

import numpy as np
import pytest

from helpers import assert_state_equal
from test_flush_wire_gpu import IDENT, OTHER, TYPES, _apply, _by_key, _deltas_size, _flush_slots, _flush_wire

pytestmark = pytest.mark.gpu

N = 257
JY_ERANGE = -4
FORMS = {"slot": _flush_slots, "wire": _flush_wire}
ORDERS = [("slot", "wire"), ("wire", "slot")]


def _value(rng):
    """0-20 bytes: inline (<= 8) and arena values"""
    return bytes(rng.integers(0, 256, int(rng.integers(0, 21))).astype(np.uint8))


def _batch(ctype, lo, rng):
    """oracle write calls that leave exactly the N keys k<lo> .. k<lo + N - 1> pending"""
    ops = []
    for i in range(lo, lo + N):
        k = f"k{i}"
        if ctype == 0:
            ops.append(("gcount_inc", k, int(rng.integers(1, 1 << 62))))
        elif ctype == 1:  # only INC, only DEC, both: every mask, and the slot form's zero fill
            if i % 3 != 1:
                ops.append(("pncount_inc", k, int(rng.integers(1, 1 << 62))))
            if i % 3 != 0:
                ops.append(("pncount_dec", k, int(rng.integers(1, 1 << 62))))
        elif ctype == 2:
            ops.append(("treg_set", k, _value(rng), int(rng.integers(0, 6))))
        elif ctype == 3:
            for j in range(1 + i % 3):  # (the first one above every cutoff: the log changes, the key is pending)
                ops.append(("tlog_ins", k, _value(rng), int(rng.integers(5 if j else 30, 40))))
            if i % 5 == 0:
                ops.append(("tlog_trimat", k, int(rng.integers(0, 30))))
        else:
            for _ in range(1 + i % 2):
                ops.append(("ujson_ins", k, int(rng.integers(1, 8))))
            if i % 4 == 0:
                ops.append(("ujson_rm", k, int(rng.integers(1, 8))))
    return ops


def _write(ctype, want, got, ops):
    for name, *a in ops:
        getattr(want, name)(*a)
    _apply(ctype, got, ops)
    assert got.deltas_size() == want.deltas_size() == N


def _pair(oracle_mod, engine, ctype, seed):
    from jylis_amd.repo import REPOS
    return oracle_mod.Repo(ctype, IDENT), REPOS[ctype](engine, IDENT), np.random.default_rng(seed)


def _same(ctype, want_table, got_table):
    assert_state_equal(ctype, _by_key(ctype, want_table), _by_key(ctype, got_table))


# 1 ---------------------------------------------------------------------------
@pytest.mark.parametrize("first,second", ORDERS)
@pytest.mark.parametrize("ctype", TYPES)
def test_forms_take_turns_on_one_pending_set(oracle_mod, engine, ctype, first, second):
    """batch 1, flush with one form: the other form then finds nothing; batch 2
    over overlapping keys, flushed with the other form, is the oracle's
    flush_deltas of batch 2 alone"""
    want, got, rng = _pair(oracle_mod, engine, ctype, 900 + ctype)
    _write(ctype, want, got, _batch(ctype, 0, rng))
    _same(ctype, want.flush().table(), FORMS[first](ctype, got))
    assert _deltas_size(ctype, engine) == 0
    assert len(FORMS[second](ctype, got)["key_offs"]) == 1
    _write(ctype, want, got, _batch(ctype, N // 2, rng))
    _same(ctype, want.flush().table(), FORMS[second](ctype, got))
    assert _deltas_size(ctype, engine) == 0
    assert len(FORMS[first](ctype, got)["key_offs"]) == 1
    assert_state_equal(ctype, want.state(), got.state())


# 2 ---------------------------------------------------------------------------
def _out(dtype, n):
    """an output array no flush may touch: all ones"""
    return np.full(max(n, 1), np.iinfo(dtype).max, dtype)


def _untouched(arrays):
    return all((a == np.iinfo(a.dtype).max).all() for a in arrays)


def _slot_call(engine, ctype, caps):
    """one slot-form flush call into fresh host arrays of exactly `caps` -> (rc, sizes, arrays)"""
    lib, HOST = engine.lib, 0
    u32, u64 = np.uint32, np.uint64
    if ctype in (0, 1):
        arrays = [_out(u32, caps[0]), _out(u64, (ctype + 1) * caps[0]), _out(u32, caps[0])]
        sizes = [C.c_uint64()]
        rc = lib.jy_counter_flush(engine.h, ctype, caps[0], *[a.ctypes.data for a in arrays], C.byref(sizes[0]), HOST)
    elif ctype == 2:
        arrays = [_out(u32, caps[0])] + [_out(u64, caps[0]) for _ in range(3)]
        sizes = [C.c_uint64()]
        rc = lib.jy_treg_flush(engine.h, caps[0], *[a.ctypes.data for a in arrays], C.byref(sizes[0]), HOST)
    elif ctype == 3:
        arrays = [_out(u32, caps[0]), _out(u64, caps[0]), _out(u64, caps[0] + 1)] + [_out(u64, caps[1]) for _ in range(3)]
        sizes = [C.c_uint64(), C.c_uint64()]
        rc = lib.jy_tlog_flush(engine.h, *caps, *[a.ctypes.data for a in arrays], *map(C.byref, sizes), HOST)
    else:
        R = engine.ujson_columns
        arrays = [_out(u32, caps[0]), _out(u64, caps[0] + 1), _out(u64, caps[1]), _out(u64, caps[1]),
                  _out(u64, caps[0] * R), _out(u64, caps[0] + 1), _out(u64, caps[2])]
        sizes = [C.c_uint64() for _ in range(3)]
        rc = lib.jy_ujson_flush(engine.h, *caps, *[a.ctypes.data for a in arrays], *map(C.byref, sizes), HOST)
    return rc, [s.value for s in sizes], arrays


@pytest.mark.parametrize("then", ["slot", "wire"])
@pytest.mark.parametrize("ctype", [1, 2])
def test_short_slot_capacity_is_an_error_and_clears_nothing(oracle_mod, engine, ctype, then):
    """slot-form counter and TREG flush with room for pending - 1 keys:
    JY_ERANGE, *n_out = pending, nothing written or cleared; the next flush
    of either form returns all of it"""
    want, got, rng = _pair(oracle_mod, engine, ctype, 910 + ctype)
    _write(ctype, want, got, _batch(ctype, 0, rng))
    rc, sizes, arrays = _slot_call(engine, ctype, [N - 1])
    assert rc == JY_ERANGE and sizes == [N]
    assert b"flush output capacity is smaller than the pending delta count" in engine.lib.jy_last_error(engine.h)
    assert _untouched(arrays)
    assert _deltas_size(ctype, engine) == N
    _same(ctype, want.flush().table(), FORMS[then](ctype, got))
    assert _deltas_size(ctype, engine) == 0


@pytest.mark.parametrize("then", ["slot", "wire"])
@pytest.mark.parametrize("ctype", [3, 4])
def test_short_slot_capacity_reports_sizes_and_clears_nothing(oracle_mod, engine, ctype, then):
    """slot-form TLOG and UJSON flush, each capacity one short in turn: JY_OK,
    the sizes, nothing written or cleared; then either form returns all of it"""
    want, got, rng = _pair(oracle_mod, engine, ctype, 920 + ctype)
    _write(ctype, want, got, _batch(ctype, 0, rng))
    rc, need, _ = _slot_call(engine, ctype, [0] * (ctype - 1))
    assert rc == 0 and need[0] == N and need[1] > 0
    for i, total in enumerate(need):
        if total == 0:
            continue  # (nothing of this kind is pending: no capacity can be short)
        caps = list(need)
        caps[i] -= 1
        rc, sizes, arrays = _slot_call(engine, ctype, caps)
        assert rc == 0 and sizes == need and _untouched(arrays), i
        assert _deltas_size(ctype, engine) == N
    _same(ctype, want.flush().table(), FORMS[then](ctype, got))
    assert _deltas_size(ctype, engine) == 0


def test_short_wire_capacity_leaves_the_set_to_the_slot_form(oracle_mod, engine):
    """the same for one wire form (TREG): sizes only, then the slot form returns all of it"""
    ctype = 2
    want, got, rng = _pair(oracle_mod, engine, ctype, 930)
    _write(ctype, want, got, _batch(ctype, 0, rng))
    need, _ = engine.flush_wire_caps(ctype, [0, 0, 0])
    assert need[0] == N and need[1] > 0 and need[2] > 0
    for i in range(3):
        caps = list(need)
        caps[i] -= 1
        sizes, out = engine.flush_wire_caps(ctype, caps)
        assert sizes == need and not any(np.asarray(v).any() for v in out.values()), i
        assert _deltas_size(ctype, engine) == N
    _same(ctype, want.flush().table(), _flush_slots(ctype, got))
    assert _deltas_size(ctype, engine) == 0


# 3 ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["slot", "wire"])
def test_counter_flush_frees_the_replica_column(engine, form):
    """pending counter deltas belong to one replica column until a flush of
    either form clears them: then a write under another column succeeds"""
    from jylis_amd.engine import EngineError
    from jylis_amd.repo import RepoPNCOUNT
    got = RepoPNCOUNT(engine, IDENT)
    keys = [f"k{i}" for i in range(N)]
    got.inc(keys, np.arange(1, N + 1), IDENT)
    with pytest.raises(EngineError, match="another replica column"):
        got.dec(keys[:3], np.arange(1, 4), OTHER)
    assert len(FORMS[form](1, got)["key_offs"]) == N + 1
    got.dec(keys[:3], np.arange(1, 4), OTHER)
    assert got.deltas_size() == 3
    t = got.flush_wire(OTHER) if form == "slot" else got.flush_deltas(OTHER)
    assert len(t["key_offs"]) == 4 and len(t["p_ids"]) == 0
    np.testing.assert_array_equal(t["n_ids"], np.full(3, OTHER, np.uint64))
    np.testing.assert_array_equal(t["n_vals"], np.arange(1, 4).astype(np.uint64))
