"""One wire formatter per type, two stores: the flush formats the PENDING
store, the snapshots format the STATE, the digest reads the state through the
same readers (jy_wire.hpp).  On an engine whose every key was written locally
only, a key's pending delta IS its state, so the two sources must give the
same arrays -- and the digest of a range must agree with the digest of what
its snapshot restores."""
import numpy as np
import pytest

from test_state_wire_gpu import IDENT, OTHER, _col_ids

pytestmark = pytest.mark.gpu

N = 257  # one past a 256-thread workgroup; eight 32-slot counter tiles plus one
VAL_LENS = [0, 7, 8, 9, 15, 16, 17, 70000]  # inline / arena boundary, 8-byte granules, many gather tiles
PN, TREG, TLOG, UJSON = 1, 2, 3, 4
UJ_SIZES = (0, 1, 2, 600)  # elements a document ends with


def _keys():
    """N distinct keys of lengths 0..40 cycling (the empty key exists once: its
    later places in the cycle take 41 bytes)"""
    keys = []
    for i in range(N):
        L = i % 41 or (41 if i else 0)
        keys.append((b"%03d" % i + b"~" * 41)[:L] if L >= 3 else (bytes([48 + i // 41]) * L))
    assert len(set(keys)) == N and {len(k) for k in keys} == set(range(42))
    return keys


def _value(rng, L):
    return bytes(rng.integers(0, 256, L).astype(np.uint8))


def _write(eng, ctype, after_ins=None):
    """local writes only -> the ascending slots of the written keys (slot i = key i).
    UJSON: after_ins() runs between the INS batch and the RM batch"""
    from jylis_amd.repo import REPOS
    rng = np.random.default_rng(1200 + ctype)
    keys = _keys()
    eng.replica_cols([OTHER, IDENT])  # the written column is 1, not 0
    assert eng.intern(ctype, keys).tolist() == list(range(N))
    repo = REPOS[ctype](eng, IDENT)
    if ctype == PN:
        # i % 4: 0 interned but unwritten, 1 INC only, 2 DEC only, 3 both
        inc = [i for i in range(N) if i % 4 in (1, 3)]
        dec = [i for i in range(N) if i % 4 in (2, 3)]
        repo.inc([keys[i] for i in inc], np.array([3 * i + 1 for i in inc], np.int64), IDENT)
        repo.dec([keys[i] for i in dec], np.array([5 * i + 2 for i in dec], np.int64), IDENT)
        written = sorted(set(inc) | set(dec))
    elif ctype == TREG:
        written = list(range(N))
        repo.set(keys, [_value(rng, VAL_LENS[i % 8]) for i in written], np.arange(1, N + 1, dtype=np.uint64))
    elif ctype == TLOG:
        # 0 to 5 entries per key (more than 4: the merge's slow tile path), distinct ts per key
        cmds = [("INS", keys[i], _value(rng, VAL_LENS[(i + e) % 8]), 10 * i + e + 1)
                for i in range(N) for e in range(i % 6)]
        repo.write(cmds)
        written = [i for i in range(N) if i % 6]
    else:
        # documents of 0, 1, 2 and 600 elements: one more is inserted, and an RM batch removes it
        eng.ujson_set_inplace(3)
        size = lambda i: UJ_SIZES[i % 4]
        elem = lambda i, e: (i << 20) | (e + 1)
        repo.write([("INS", keys[i], elem(i, e)) for i in range(N) for e in range(size(i) + 1)], IDENT)
        if after_ins:
            after_ins()
        repo.write([("RM", keys[i], elem(i, size(i))) for i in range(N)], IDENT)
        written = list(range(N))
    return np.array(written, np.uint32)


def _deltas_size(eng, ctype):
    return eng.counter_deltas_size(ctype) if ctype == PN else (
        eng.treg_deltas_size, eng.tlog_deltas_size, eng.ujson_deltas_size)[ctype - 2]()


def _select_col(w, col):
    """a counter batch's cells of one column"""
    keep = w["col"] == col
    n = len(w["cell_offs"]) - 1
    seg = np.repeat(np.arange(n), np.diff(w["cell_offs"].astype(np.int64)))
    offs = np.concatenate([[0], np.cumsum(np.bincount(seg[keep], minlength=n))]).astype(np.uint64)
    return dict(w, cell_offs=offs, sign=w["sign"][keep], col=w["col"][keep], val=w["val"][keep])


def _same(ctype, a, b):
    from jylis_amd.engine import WIRE_ARRAYS
    for name, dt, _, _ in WIRE_ARRAYS[ctype]:
        x, y = np.asarray(a[name]), np.asarray(b[name])
        assert x.dtype == y.dtype == np.dtype(dt), name
        np.testing.assert_array_equal(x, y, err_msg=f"array {name}")


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("ctype", [PN, TREG, TLOG])
def test_pending_and_state_format_alike(engine, ctype, device):
    """state_wire_slots(pending slots) before the flush == flush_wire, array for
    array; the snapshot's host and device outputs are equal too"""
    from jylis_amd.repo import wire_to_host
    slots = _write(engine, ctype)
    assert _deltas_size(engine, ctype) == len(slots) > 0
    col = engine.replica_col(IDENT)
    state = engine.state_wire_slots(ctype, slots)
    state_dev = engine.state_wire_slots(ctype, slots, device=True)
    engine.sync()
    _same(ctype, state, wire_to_host(ctype, state_dev))
    flushed = engine.flush_wire(ctype, device=device, col=col)
    engine.sync()
    flushed = wire_to_host(ctype, flushed)
    assert _deltas_size(engine, ctype) == 0
    if ctype == PN:
        assert (flushed["col"] == col).all()
        state = _select_col(state, col)
    _same(ctype, state, flushed)
    assert len(flushed["key_offs"]) - 1 == len(slots)


def _fresh(src):
    from jylis_amd.engine import Engine
    e = Engine(device=0)
    e.ujson_set_inplace(3)
    ids = _col_ids(src).tolist()
    assert e.replica_cols(ids).tolist() == list(range(len(ids)))
    return e


def _el_counts(w):
    return np.diff(np.asarray(w["el_offs"]).astype(np.int64))


def test_ujson_pending_and_state_converge_alike(engine):
    """the delta and the state may split a dot differently between vv and cloud:
    what they converge to is compared, not their arrays.  The INS batch and the
    RM batch are flushed apart and converged in order (a pending delta takes an
    RM's dots into its context only, as the reference does: an element inserted
    and removed inside ONE flush interval still travels in that delta), so the
    second delta carries removed dots and no element."""
    engine.replica_cols([OTHER, IDENT])
    a, b = _fresh(engine), _fresh(engine)
    try:
        def flush_ins():
            ins = engine.flush_wire(UJSON)
            assert _el_counts(ins).tolist() == [UJ_SIZES[i % 4] + 1 for i in range(N)]
            a.converge_wire(UJSON, ins)
            assert _el_counts(a.state_wire(UJSON, 0, N)).sum() == sum(UJ_SIZES[i % 4] + 1 for i in range(N))

        _write(engine, UJSON, after_ins=flush_ins)
        state = engine.state_wire(UJSON, 0, N)
        rm = engine.flush_wire(UJSON)
        # every document is pending again; the RM delta holds no element, only the removed dots
        assert len(rm["key_offs"]) - 1 == N and len(rm["elems"]) == 0
        assert len(rm["vv"]) + len(rm["cloud"]) >= N
        assert _el_counts(state).tolist() == [UJ_SIZES[i % 4] for i in range(N)]
        a.converge_wire(UJSON, rm)
        b.converge_wire(UJSON, state)
        # an element really disappeared from every document of A
        assert _el_counts(a.state_wire(UJSON, 0, N)).tolist() == [UJ_SIZES[i % 4] for i in range(N)]
        want = engine.digest(UJSON, 16)
        assert want[:, 1].sum() == N
        np.testing.assert_array_equal(a.digest(UJSON, 16), want)
        np.testing.assert_array_equal(b.digest(UJSON, 16), want)
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("ctype", [PN, TREG, TLOG, UJSON])
def test_digest_and_snapshot_of_one_engine(engine, ctype):
    """both consumers of the state readers on the same engine: the digest in one
    call == its wrapping sum over chunks of 100 slots == the digest of an engine
    restored from snapshot(max_keys=100)"""
    _write(engine, ctype)
    whole = engine.digest(ctype, 8)
    assert whole[:, 1].sum() == N
    np.testing.assert_array_equal(engine.digest(ctype, 8, max_keys=100), whole)
    chunks = list(engine.snapshot(ctype, max_keys=100))
    assert [len(w["key_offs"]) - 1 for w in chunks] == [100, 100, 57]
    restored = _fresh(engine)
    try:
        for w in chunks:
            restored.converge_wire(ctype, w)
        np.testing.assert_array_equal(restored.digest(ctype, 8), whole)
    finally:
        restored.close()
