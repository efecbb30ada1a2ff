"""The host round split of the slot-form calls (jy_tlog_converge, jy_tlog_write,
jy_ujson_converge, jy_ujson_write with host arrays; abi_logs.hip over
jy_rounds.hpp).

Every case is one batch of seven items over three keys in the pattern
[a, b, a, c, a, b, a] -- four rounds {0,1,3} {2,5} {4} {6}, each a strict
subset of the one before.  Engine A takes the batch in one call, engine B its
items in seven one-item calls, in order; state_wire and flush_wire of the two
are compared byte for byte, and engine A against the CPU oracle."""
import numpy as np
import pytest

from helpers import assert_state_equal
from test_parity_tlog import _canon as _tlog_canon, _log_batch
from test_put_keys_gpu import _check_oracle, _table, _tlog_columns, _wires_equal, pair  # noqa: F401
from test_ujson_write_gpu import _canon_ujson

pytestmark = pytest.mark.gpu

IDENT = 0x5EED_0000_0000_0A0B
TLOG, UJSON = 3, 4
KEYS = ["a", "b", "a", "c", "a", "b", "a"]
LONG = b"a value past eight bytes"


def _concat(parts):
    """one-item batch tables -> one batch table naming their keys in order"""
    cat = {}
    for k in parts[0]:
        if k.endswith("offs"):
            acc, base = [np.zeros(1, np.uint64)], 0
            for p in parts:
                acc.append(np.asarray(p[k], np.uint64)[1:] + np.uint64(base))
                base = int(acc[-1][-1]) if len(acc[-1]) else base
            cat[k] = np.concatenate(acc)
        else:
            cat[k] = np.concatenate([np.asarray(p[k]) for p in parts])
    return cat


def test_tlog_converge_rounds(oracle_mod, pair):
    """deltas of 0, 1 and 3 entries; the empty one (a cutoff only) is b's second,
    in the second round; one value lives in the arena"""
    from jylis_amd.repo import RepoTLOG
    O = oracle_mod
    a, b = pair
    logs = [("a", 0, _tlog_canon([(b"a1", 5), (b"a0", 3), (LONG, 1)])),
            ("b", 0, [(b"b0", 4)]),
            ("a", 4, _tlog_canon([(b"a2", 9), (b"a1", 5), (b"a!", 5)])),
            ("c", 2, []),
            ("a", 0, [(b"a3", 7)]),
            ("b", 5, []),
            ("a", 8, [(b"a4", 8)])]
    assert [k for k, _, _ in logs] == KEYS and sorted(len(e) for _, _, e in logs) == [0, 0, 1, 1, 1, 3, 3]
    want = O.Repo(O.TLOG)
    want.converge(_log_batch(logs))
    RepoTLOG(a).converge_deltas(_log_batch(logs))
    rb = RepoTLOG(b)
    for one in logs:
        rb.converge_deltas(_log_batch([one]))
    sw, fw = _wires_equal(TLOG, a, b)
    _check_oracle(TLOG, a, want, sw, None)  # (a converge leaves nothing to flush)
    assert RepoTLOG(a).get("a") == [(b"a2", 9), (b"a4", 8)] and RepoTLOG(a).cutoff("b") == 5


def _call_tlog_write(eng, ops, slots, ts, arg, pre, lr):
    """jy_tlog_write with host arrays; a column given as None is passed as NULL"""
    from jylis_amd import engine as E
    cols = [E._arg(x, t) for x, t in ((ops, np.uint8), (slots, np.uint32), (ts, np.uint64), (arg, np.uint64),
                                      (pre, np.uint64), (lr, np.uint64))]
    eng._check(eng.lib.jy_tlog_write(eng.h, len(slots), *[p for _, p, _ in cols], E.HOST))


def test_tlog_write_rounds(oracle_mod, pair):
    """INS, TRIM 1, TRIMAT and CLR on key a, in an order that matters (TRIM 1
    and CLR before the INS would find an empty log); the one-item calls pass
    only the columns their op reads (an INS: no arg)"""
    O = oracle_mod
    a, b = pair
    cmds = [("INS", "a", LONG, 5), ("INS", "b", b"b0", 3), ("TRIM", "a", 1), ("TRIMAT", "c", 4),
            ("TRIMAT", "a", 3), ("INS", "b", b"b1", 2), ("CLR", "a")]
    assert [c[1] for c in cmds] == KEYS
    want = O.Repo(O.TLOG, IDENT)
    for c in cmds:
        getattr(want, "tlog_" + c[0].lower())(*c[1:])
    ops, keys, ts, arg, vals = _tlog_columns(cmds)
    uses = {"INS": (True, False, True), "TRIMAT": (True, False, False), "TRIM": (False, True, False),
            "CLR": (False, False, False)}
    for eng in (a, b):
        slots = eng.intern(TLOG, keys)
        pre, lr = eng.pack_values(TLOG, vals)
        if eng is a:
            _call_tlog_write(a, ops, slots, ts, arg, pre, lr)
            continue
        for i, c in enumerate(cmds):
            t, g, v = uses[c[0]]
            s = slice(i, i + 1)
            _call_tlog_write(b, ops[s], slots[s], ts[s] if t else None, arg[s] if g else None,
                             pre[s] if v else None, lr[s] if v else None)
    assert a.tlog_deltas_size() == b.tlog_deltas_size() == want.deltas_size() == 3
    sw, fw = _wires_equal(TLOG, a, b)
    assert a.tlog_deltas_size() == b.tlog_deltas_size() == 0
    _check_oracle(TLOG, a, want, sw, fw)


def _ujson_parts(O):
    """seven one-doc deltas of one replica, flushed after every command"""
    r = O.Repo(O.UJSON, 3)
    cmds = [("ins", "a", 1), ("ins", "b", 2), ("ins", "a", 3), ("ins", "c", 4), ("rm", "a", 1), ("clr", "b"),
            ("ins", "a", 5)]
    assert [c[1] for c in cmds] == KEYS
    parts = []
    for c in cmds:
        getattr(r, "ujson_" + c[0])(*c[1:])
        parts.append(r.flush().table())
    return parts


def test_ujson_converge_rounds(oracle_mod, pair):
    """inserts (an empty cloud), an observed remove and a clear (no elements)"""
    from jylis_amd.repo import RepoUJSON
    O = oracle_mod
    a, b = pair
    parts = _ujson_parts(O)
    clouds = [int(p["cloud_offs"][-1]) for p in parts]
    assert all(len(p["key_offs"]) == 2 for p in parts) and 0 in clouds
    cat = _concat(parts)
    assert len(cat["key_offs"]) == 8
    want = O.Repo(O.UJSON, 9)
    want.converge(cat)
    RepoUJSON(a).converge_deltas(cat)
    rb = RepoUJSON(b)
    for p in parts:
        rb.converge_deltas(p)
    _wires_equal(UJSON, a, b)
    assert_state_equal(O.UJSON, want.state(), RepoUJSON(a).state())
    assert RepoUJSON(a).elements("a") == {3, 5} and RepoUJSON(a).elements("b") == set()


def test_ujson_write_rounds(oracle_mod, pair):
    """INS, RM and CLR in an order that matters (the RM of 5 sits between two
    INS of 5); the one-item CLR passes no element column"""
    from jylis_amd import engine as E
    from jylis_amd.repo import RepoUJSON
    O = oracle_mod
    a, b = pair
    cmds = [("INS", "a", 5), ("INS", "b", 1), ("INS", "a", 6), ("INS", "c", 2), ("RM", "a", 5), ("CLR", "b"),
            ("INS", "a", 5)]
    assert [c[1] for c in cmds] == KEYS
    want = O.Repo(O.UJSON, IDENT)
    for c in cmds:
        getattr(want, "ujson_" + c[0].lower())(*c[1:])
    codes = {"INS": E._lib.UJSON_INS, "RM": E._lib.UJSON_RM, "CLR": E._lib.UJSON_CLR}
    ops = np.array([codes[c[0]] for c in cmds], np.uint8)
    elems = np.array([c[2] if len(c) > 2 else 0 for c in cmds], np.uint64)

    def call(eng, o, s, e, col):
        cols = [E._arg(x, t) for x, t in ((o, np.uint8), (s, np.uint32), (e, np.uint64))]
        eng._check(eng.lib.jy_ujson_write(eng.h, len(s), *[p for _, p, _ in cols], col, E.HOST))

    for eng in (a, b):
        slots = eng.intern(UJSON, KEYS)
        col = int(eng.replica_cols([IDENT])[0])
        if eng is a:
            call(a, ops, slots, elems, col)
            continue
        for i, c in enumerate(cmds):
            s = slice(i, i + 1)
            call(b, ops[s], slots[s], elems[s] if c[0] != "CLR" else None, col)
    assert a.ujson_deltas_size() == b.ujson_deltas_size() == want.deltas_size() == 3
    sw, fw = _wires_equal(UJSON, a, b)
    assert a.ujson_deltas_size() == b.ujson_deltas_size() == 0
    assert _canon_ujson(_table(a, UJSON, fw)) == _canon_ujson(want.flush().table())
    assert_state_equal(O.UJSON, want.state(), RepoUJSON(a).state())
    assert RepoUJSON(a).elements("a") == {5, 6}
