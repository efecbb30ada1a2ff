"""RESP execute on the GPU (jy_resp_exec / jy_resp_replies, k_resp_out.hip;
Engine.resp_exec): request bytes in, one reply byte stream per connection out.

Replies are byte-exact.  The oracle is the host mirror (jylis_amd.host.Database)
fed the same commands one at a time; where stated, a second check runs
jylis_amd.resp_in.exec_resp on a fresh engine and compares bytes, used / closed
and the state afterwards (state_wire and flush_wire of each type).  Replies
that are plain arithmetic (+OK, a counter's decimal) are written out by hand
where the mirror would need thousands of single calls.  The inputs are
tests/resp_exec_cases.py's, whose coverage tests/test_resp_exec_cpu.py asserts."""
import json
import os

import numpy as np
import pytest

import resp_exec_cases as XC
import resp_in_cases as RC
import resp_in_ref as ref
from resp_in_ref import request as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "kat_docs.json")
OK = b"+OK\r\n"
FILL = 0xAB


def _host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _no_host(words):
    raise AssertionError("no HOST command expected: %r" % (words,))


def _mirror(conns, db=None):
    """each connection's complete commands through Database.apply, one at a time
    -> (replies per connection, used, closed)"""
    from jylis_amd.host import Database
    own = db is None
    db = db or Database(device=0, identity=1)
    try:
        out = []
        for c in conns:
            cmds, used, err = ref.frame(c, 0, len(c))
            out.append((b"".join(db.apply(*[c[o:o + n] for o, n in words]) for words in cmds), used, bool(err)))
        return out
    finally:
        if own:
            db.close()


def _states_equal(a, b, col_a, col_b):
    from jylis_amd import _lib
    for ctype in (_lib.GCOUNT, _lib.PNCOUNT, _lib.TREG, _lib.TLOG):
        n = a.nkeys(ctype)
        assert n == b.nkeys(ctype), ctype
        if n == 0:
            continue
        for wa, wb in ((a.state_wire(ctype, 0, n), b.state_wire(ctype, 0, n)),
                       (a.flush_wire(ctype, col=col_a), b.flush_wire(ctype, col=col_b))):
            assert wa.keys() == wb.keys()
            for name in wa:
                np.testing.assert_array_equal(_host(wa[name]), _host(wb[name]), err_msg="%s %s" % (ctype, name))


def _digests(e):
    from jylis_amd import _lib
    return [(e.nkeys(t), e.digest(t).tolist() if e.nkeys(t) else None)
            for t in (_lib.GCOUNT, _lib.PNCOUNT, _lib.TREG, _lib.TLOG)]


def _fed(run, conns, feeds):
    """`run(buffers)` over the connections cut into `feeds` heartbeats, tails kept
    -> (replies per connection, whether any connection was closed)"""
    got, pending, closed = [b""] * len(conns), [b""] * len(conns), False
    for f in range(feeds):
        cut = [c[len(c) * f // feeds:len(c) * (f + 1) // feeds] for c in conns]
        pending = [p + x for p, x in zip(pending, cut)]
        for i, (reply, used, err) in enumerate(run(pending)):
            closed |= err
            got[i] += reply
            pending[i] = pending[i][used:]
    assert pending == [b""] * len(conns)
    return got, closed


def _doc_conns():
    kat = json.load(open(GOLD))
    return [b"".join(b for b, _, _ in RC.doc_requests(kat, name, typ))
            for name, typ in (("treg_doc", "TREG"), ("tlog_doc", "TLOG"), ("gcount_doc", "GCOUNT"),
                              ("pncount_doc", "PNCOUNT"))]


# ---- 1 ----
@pytest.mark.parametrize("feeds", [1, 3])
def test_docs_sessions_and_mixed_tables(feeds):
    """the docs' sessions, the phase table, every kind with the HOST help texts and
    the binary-safe values: one heartbeat, and cut into three with the tails kept"""
    from jylis_amd.engine import Engine
    from jylis_amd.host import Database
    from jylis_amd.resp_in import exec_resp
    conns = RC.phases() + [b"".join(RC.kinds(False)[0])] + RC.tricky() + _doc_conns()
    want = [r for r, _, _ in _mirror(conns)]
    db = Database(device=0, identity=1)  # answers the HOST commands of both runs
    a, b = Engine(device=0), Engine(device=0)
    try:
        on_host = lambda words: db.apply(*words)
        got, closed = _fed(lambda bufs: a.resp_exec(bufs, 1, on_host), conns, feeds)
        assert got == want and not closed
        old, closed = _fed(lambda bufs: exec_resp(b, bufs, 1, on_host), conns, feeds)
        assert old == want and not closed
        _states_equal(a, b, a.replica_col(1), b.replica_col(1))
    finally:
        a.close()
        b.close()
        db.close()


# ---- 2 ----
def test_permutation(engine):
    conns = XC.permutation()
    got = engine.resp_exec(conns, 1, _no_host)
    assert got == _mirror(conns)
    assert got[0][0] == b"$-1\r\n" + OK + b"*2\r\n$5\r\nfresh\r\n:7\r\n"  # the second GET a sees the SET
    assert got[1][0] == OK + b"*2\r\n$5\r\nother\r\n:9\r\n"


# ---- 3 ----
@pytest.mark.parametrize("name", sorted(XC.empty_ranges()))
def test_empty_ranges(engine, name):
    conns = XC.empty_ranges()[name]
    got = engine.resp_exec(conns, 1, _no_host)
    want = [(OK if c == XC.W else b"", len(c) if c == XC.W else 0, c == XC.BAD) for c in conns]
    assert got == want
    raw = engine.resp_exec(conns, 1, _no_host, device=True)
    engine.sync()
    offs = _host(raw["conn_reply_offs"]).astype(np.int64)
    assert offs.tolist() == np.concatenate([[0], np.cumsum([len(r) for r, _, _ in want])]).astype(np.int64).tolist()
    assert raw["sizes"][0] == sum(c == XC.W for c in conns) and raw["sizes"][1] == int(offs[-1])


# ---- 4 ----
def test_violation_mid_stream(engine):
    from jylis_amd import _lib
    good = R("TREG", "SET", "v1", "one", 1) + R("TREG", "SET", "v2", "two", 2)
    conns = [good + b"*2\r\n$x\r\n" + R("TREG", "SET", "v3", "three", 3), R("TREG", "SET", "w", "w", 4)]
    got = engine.resp_exec(conns, 1, _no_host)
    assert got == [(OK + OK, len(good), True), (OK, len(conns[1]), False)]
    assert engine.nkeys(_lib.TREG) == 3
    after = engine.resp_exec([R("TREG", "GET", k) for k in ("v1", "v2", "v3", "w")], 1, _no_host)
    assert [r for r, _, _ in after] == [b"*2\r\n$3\r\none\r\n:1\r\n", b"*2\r\n$3\r\ntwo\r\n:2\r\n", b"$-1\r\n",
                                        b"*2\r\n$1\r\nw\r\n:4\r\n"]


# ---- 5 ----
@pytest.mark.parametrize("n", XC.BOUNDARY_COUNTS)
def test_assembly_constants(engine, n):
    """command counts one below, at and one above the scan's tile (jy_dscan.hpp
    kTileItems) and the gather's staged offsets (jy_wire.hpp kStage)"""
    assert n in (XC.GATHER_STAGE - 1, XC.GATHER_STAGE, XC.GATHER_STAGE + 1, XC.SCAN_TILE - 1, XC.SCAN_TILE,
                 XC.SCAN_TILE + 1)
    conns = XC.ok_heartbeat(n)
    got = engine.resp_exec(conns, 1, _no_host)
    assert sum(len(r) for r, _, _ in got) == 5 * n
    for (reply, used, closed), c in zip(got, conns):
        assert reply == OK * (len(reply) // 5) and used == len(c) and not closed
    assert [len(r) // 5 for r, _, _ in got] == [len(ref.frame(c, 0, len(c))[0]) for c in conns]
    engine.resp_exec(XC.digits_setup(), 1, _no_host)
    conns, want = XC.digits_heartbeat(n)
    got = engine.resp_exec(conns, 1, _no_host)
    assert [r for r, _, _ in got] == want


# ---- 6 ----
def test_long_reply_between_short_ones(engine):
    value = bytes(range(256)) * 4096  # 1 MiB
    conn = R("TREG", "SET", "big", value, 5) + R("TREG", "GET", "big") + R("TREG", "SET", "small", "s", 6)
    got = engine.resp_exec([R("GCOUNT", "INC", "n", 1), conn, R("GCOUNT", "INC", "n", 1)], 1, _no_host)
    assert got[1] == (OK + b"*2\r\n$1048576\r\n" + value + b"\r\n:5\r\n" + OK, len(conn), False)
    assert got[0][0] == OK and got[2][0] == OK


def test_long_log_beside_many_connections(engine):
    """a TLOG GET whose reply is longer than one workgroup's bytes of the gather
    (256 lanes x 8 bytes) beside 300 one-command connections"""
    log = b"".join(R("TLOG", "INS", "long", "entry number %d" % i, 1000 + i) for i in range(120)) + \
        R("TLOG", "GET", "long")
    singles = [R("TLOG", "INS", "log%d" % (i % 50), "entry %d" % i, i) if i % 3 else R("TLOG", "SIZE", "log%d" % (i % 50))
               for i in range(300)]
    conns = singles[:150] + [log] + singles[150:]
    want = _mirror([log])[0]
    assert len(want[0]) > 120 * 5 + 2048
    got = engine.resp_exec(conns, 1, _no_host)
    assert got[150] == want
    for i, (reply, used, closed) in enumerate(got[:150] + got[151:]):
        assert used == len(singles[i]) and not closed
        assert reply == OK if i % 3 else reply[:1] == b":" and reply[-2:] == b"\r\n"


# ---- 7 ----
def _host_conns():
    a = R("GCOUNT", "INC", "hx", 1) + R("UJSON", "SET", "doc", "a", "1") + R("UJSON", "GET", "doc") + \
        R("GCOUNT", "GET", "hx") + R("SYSTEM", "GETLOG") + R("GCOUNT", "INC", "hx", 2)
    b = R("SYSTEM", "GETLOG") + R("TREG", "SET", "hr", "v", 3) + R("UJSON", "GET", "doc2") + R("TREG", "GET", "hr")
    return [a, b, R("NOPE", "GET", "k")]


def test_host_commands_interleaved(engine):
    from jylis_amd.host import Database
    conns = _host_conns()
    want = _mirror(conns)
    db = Database(device=0, identity=1)
    try:
        assert engine.resp_exec(conns, 1, lambda words: db.apply(*words)) == want
    finally:
        db.close()


def test_host_answers_in_pieces_and_empty(engine):
    """an answer written by two jy_resp_sink_write calls, answers of zero bytes, and
    more zero-byte replies in a row than the gather stages offsets for"""
    conns = [R("SYSTEM", "A") + R("GCOUNT", "INC", "z", 1) + R("SYSTEM", "B"), R("SYSTEM", "C")]
    ans = {b"A": [b"+first ", b"half\r\n"], b"B": b"", b"C": []}
    got = engine.resp_exec(conns, 1, lambda words: ans[words[1]])
    assert got == [(b"+first half\r\n" + OK, len(conns[0]), False), (b"", len(conns[1]), False)]
    n = XC.GATHER_STAGE + 76
    conns = [R("GCOUNT", "INC", "z", 1) + R("SYSTEM", "B") * n + R("GCOUNT", "GET", "z"), R("SYSTEM", "A")]
    got = engine.resp_exec(conns, 1, lambda words: ans[words[1]])
    assert got == [(OK + b":2\r\n", len(conns[0]), False), (b"+first half\r\n", len(conns[1]), False)]


def test_host_command_without_a_callback(engine):
    from jylis_amd import _lib
    from jylis_amd.engine import EngineError
    engine.resp_exec([R("GCOUNT", "INC", "keep", 4)], 1, None)  # no HOST command: no callback needed
    before = _digests(engine)
    with pytest.raises(EngineError) as e:
        engine.resp_exec([R("GCOUNT", "INC", "keep", 1) + R("SYSTEM", "GETLOG")], 1, None)
    assert e.value.code == _lib.JY_EINVAL
    assert _digests(engine) == before
    with pytest.raises(EngineError) as e:  # ... and the earlier result is gone
        engine.resp_replies_caps(1, 64)
    assert e.value.code == _lib.JY_EINVAL


def test_host_callback_raising(engine):
    from jylis_amd import _lib
    from jylis_amd.engine import EngineError

    class Boom(Exception):
        pass

    def on_host(words):
        raise Boom(words[1])

    conns = [R("TREG", "SET", "p0", "zero", 1) + R("SYSTEM", "GETLOG") + R("TREG", "SET", "p2", "two", 2)]
    with pytest.raises(Boom):
        engine.resp_exec(conns, 1, on_host)
    with pytest.raises(EngineError) as e:
        engine.resp_replies_caps(1, 1 << 10)
    assert e.value.code == _lib.JY_EINVAL
    got = engine.resp_exec([R("TREG", "GET", "p0") + R("TREG", "GET", "p2")], 1, _no_host)
    assert got[0][0] == b"*2\r\n$4\r\nzero\r\n:1\r\n" + b"$-1\r\n"  # phase 0 stands, phase 2 never ran


# ---- 8 ----
def test_memory_forms(engine):
    import torch
    from jylis_amd import _lib
    from jylis_amd.engine import Engine, EngineError
    dev = f"cuda:{engine.device}"
    fresh = Engine(device=0)
    try:
        with pytest.raises(EngineError) as e:  # nothing retained yet
            fresh.resp_replies_caps(0, 0)
        assert e.value.code == _lib.JY_EINVAL
    finally:
        fresh.close()
    conns = _host_conns() + XC.permutation()
    want = _mirror(conns)
    buf, offs = ref.join(conns)
    hbuf = np.frombuffer(buf, np.uint8)
    n, nconn = len(buf), len(conns)
    from jylis_amd.host import Database
    for mis in (0, 1, 3, 7):  # request bytes in device memory, off an 8-byte boundary
        e2, db = Engine(device=0), Database(device=0, identity=1)
        try:
            pad = torch.full((n + 32,), FILL, dtype=torch.uint8, device=dev)
            assert pad.data_ptr() % 8 == 0
            dreq = pad[8 + mis:8 + mis + n]
            dreq.copy_(torch.from_numpy(hbuf.copy()))
            torch.cuda.synchronize()
            assert e2.resp_exec((dreq, offs), 1, lambda words: db.apply(*words)) == want
        finally:
            e2.close()
            db.close()
    # the retained result copied out: host and device, reply_bytes off an 8-byte boundary
    db = Database(device=0, identity=1)
    try:
        sizes = engine.resp_exec_raw(conns, 1, lambda words: db.apply(*words))
    finally:
        db.close()
    total = sizes[1]
    all_bytes = b"".join(r for r, _, _ in want)
    assert total == len(all_bytes) and sizes[0] == sum(len(ref.frame(c, 0, len(c))[0]) for c in conns)
    want_offs = np.concatenate([[0], np.cumsum([len(r) for r, _, _ in want])]).astype(np.uint64)
    for device in (False, True):
        for mis in (0, 1, 3, 7):
            # every output a byte buffer full of FILL (8 bytes an element for the u64 arrays)
            if device:
                mk = lambda nbytes: torch.full((nbytes,), FILL, dtype=torch.uint8, device=dev)
            else:
                mk = lambda nbytes: np.full(nbytes, FILL, np.uint8)
            rb = mk(total + 16)
            out = {"reply_bytes": rb[8 + mis:], "conn_reply_offs": mk(8 * (nconn + 1)),
                   "conn_used": mk(8 * nconn), "conn_err": mk(nconn)}
            # one byte short: sizes only, the poisoned outputs untouched
            got, _ = engine.resp_replies_caps(nconn, total - 1, device, out)
            engine.sync()
            assert got == [total, nconn]
            for k, v in list(out.items()) + [("all", rb)]:
                assert (_host(v).view(np.uint8) == FILL).all(), k
            got, _ = engine.resp_replies_caps(nconn, total, device, out)
            engine.sync()
            assert got == [total, nconn]
            assert _host(out["reply_bytes"])[:total].tobytes() == all_bytes
            assert (_host(rb)[:8 + mis] == FILL).all() and (_host(rb)[8 + mis + total:] == FILL).all()
            np.testing.assert_array_equal(_host(out["conn_reply_offs"]).view(np.uint64), want_offs)
            assert _host(out["conn_used"]).view(np.uint64).tolist() == [u for _, u, _ in want]
            assert _host(out["conn_err"]).tolist() == [int(c) for _, _, c in want]
    with pytest.raises(EngineError) as e:  # a wrong nconn
        engine.resp_replies_caps(nconn + 1, total)
    assert e.value.code == _lib.JY_EINVAL
    # a second exec replaces the first result
    assert engine.resp_exec([R("GCOUNT", "INC", "second", 1)], 1, None) == [(OK, len(R("GCOUNT", "INC", "second", 1)), False)]
    got, a = engine.resp_replies_caps(1, 5)
    assert got == [5, 1] and a["reply_bytes"][:5].tobytes() == OK


# ---- 9 ----
def test_every_kind(engine):
    """one command of each JY_CMD_*, and TLOG SIZE / CUTOFF / GET k 2 in one read
    group (the device-memory what / count of the TLOG reply writer)"""
    from jylis_amd.host import Database
    setup = [R("TLOG", "INS", "t", "e%d" % i, 10 + i) for i in range(5)] + [R("TLOG", "TRIMAT", "t", 11)]
    kinds = [R("GCOUNT", "INC", "g", 5), R("GCOUNT", "GET", "g"), R("PNCOUNT", "INC", "p", 3), R("PNCOUNT", "DEC", "p", 9),
             R("PNCOUNT", "GET", "p"), R("TREG", "SET", "r", "val", 4), R("TREG", "GET", "r"),
             R("TLOG", "INS", "t2", "x", 1), R("TLOG", "SIZE", "t"), R("TLOG", "CUTOFF", "t"), R("TLOG", "GET", "t", 2),
             R("TLOG", "GET", "t"), R("TLOG", "GET", "missing", 0), R("SYSTEM", "GETLOG")]
    conns = [b"".join(setup)] + kinds
    d = ref.decode(*ref.join(conns))
    assert set(d["cmd_kind"].tolist()) == set(range(ref.HOST, ref.TLOG_READ + 1))
    rd = [g for g in range(len(d["group_class"])) if d["group_class"][g] == ref.TLOG_READ]
    assert len(rd) == 1 and int(d["group_offs"][rd[0] + 1] - d["group_offs"][rd[0]]) == 5
    # the reads see the setup only if they run after it: feed the setup first
    db = Database(device=0, identity=1)
    try:
        on_host = lambda words: db.apply(*words)
        want = _mirror(conns)
        first = engine.resp_exec(conns[:1], 1, on_host)
        assert first == want[:1]
        assert engine.resp_exec(kinds, 1, on_host) == want[1:]
    finally:
        db.close()
