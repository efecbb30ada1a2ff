"""RESP requests on the GPU (jy_resp_decode, k_resp_in.hip;
jylis_amd/resp_in.exec_resp) against tests/resp_in_ref.py, element for element.

The buffers are the case tables of tests/resp_in_cases.py, whose coverage
tests/test_resp_in_cpu.py asserts without a GPU.  Each batch is decoded by the
reference once per module."""
import functools
import json
import os

import numpy as np
import pytest

import resp_in_cases as RC
import resp_in_ref as ref
from resp_in_ref import request as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "kat_docs.json")
ARRAYS = ("conn_used", "conn_err", "cmd_conn", "cmd_kind", "cmd_phase", "cmd_word_offs", "word_off", "word_len",
          "row_cmd", "key_bytes", "key_offs", "val_bytes", "val_offs", "num", "op", "group_phase", "group_class",
          "group_offs")
FILL = 0xAB


def _host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _same(got, want):
    assert got["sizes"] == want["sizes"], (got["sizes"], want["sizes"])
    for name in ARRAYS:
        g = _host(got[name])
        np.testing.assert_array_equal(g.view(want[name].dtype), want[name], err_msg=name)


@functools.lru_cache(maxsize=None)
def _batch(name):
    """a case table joined and decoded by the reference, once -> (bytes, conn_offs, expected)"""
    bufs = {"prefix": RC.prefix_sweep, "corrupt": RC.corruption_sweep, "pipelined": RC.pipelined,
            "phases": RC.phases, "kinds": lambda: RC.kinds()[0], "tricky": RC.tricky,
            "rounds": RC.round_boundaries, "residues": RC.residues,
            "mixed": lambda: RC.phases() + RC.tricky() + RC.round_boundaries() + RC.residues() + RC.kinds(False)[0]}[name]()
    buf, offs = ref.join(bufs)
    return buf, offs, ref.decode(buf, offs)


def _decode_and_compare(engine, name, device=False):
    buf, offs, want = _batch(name)
    got = engine.resp_decode((buf, offs), device=device)
    if device:
        engine.sync()
    _same(got, want)
    return got, want


def test_prefix_sweep(engine):
    """every prefix of a three-command buffer a connection of its own, one call"""
    got, want = _decode_and_compare(engine, "prefix")
    buf, offs, _ = _batch("prefix")
    assert not _host(got["conn_err"]).any()
    for c in (0, 58, 59, 60, 98, 99, len(RC.THREE)):  # the commands of each prefix, as words
        assert ref.commands(got, buf, c) == ref.commands(want, buf, c)
        assert len(ref.commands(got, buf, c)) == sum(c >= e for e in RC.THREE_ENDS)


def test_corruption_sweep(engine):
    """every single-byte corruption of the framing bytes of a two-command buffer"""
    got, want = _decode_and_compare(engine, "corrupt")
    assert 0 < int(_host(got["conn_err"]).sum()) < len(want["conn_err"])


def test_pipelining(engine):
    """20,000 pipelined commands on one connection beside 300 single-command
    connections, and a command carrying a 1 MiB value"""
    got, want = _decode_and_compare(engine, "pipelined", device=True)
    assert want["sizes"][0] == 20000 + 300 + 2 and int(np.diff(want["val_offs"].astype(np.int64)).max()) == 1 << 20
    assert int(want["cmd_phase"].max()) > 10000


def test_phases(engine):
    got, want = _decode_and_compare(engine, "phases")
    conn, phase = _host(got["cmd_conn"]), _host(got["cmd_phase"])
    assert phase[conn == 0].tolist() == list(range(20)) and phase[conn == 1].tolist() == [0, 0, 1, 2, 2, 3]


def test_kinds_and_the_16_mib_rule(engine):
    got, want = _decode_and_compare(engine, "kinds")
    names = RC.kinds()[1]
    assert _host(got["cmd_kind"]).tolist() == [getattr(ref, n) for n in names]


@pytest.mark.parametrize("name", ["tricky", "rounds", "residues"])
def test_case_tables(engine, name):
    _decode_and_compare(engine, name)
    _decode_and_compare(engine, name, device=True)


def test_memory_and_capacities(engine):
    import torch
    buf, offs, want = _batch("mixed")
    dev = f"cuda:{engine.device}"
    n = len(buf)
    # host and device input, host and device output
    hbuf = np.frombuffer(buf, np.uint8)
    for mis in (0, 1, 3, 7):  # the request bytes 1, 3 and 7 bytes off an 8-byte boundary
        pad = torch.full((n + 32,), FILL, dtype=torch.uint8, device=dev)
        assert pad.data_ptr() % 8 == 0
        dreq = pad[8 + mis:8 + mis + n]
        dreq.copy_(torch.from_numpy(hbuf.copy()))
        torch.cuda.synchronize()
        for device in (False, True):
            got = engine.resp_decode((dreq, offs), device=device)
            engine.sync()
            _same(got, want)
    mis = np.zeros(n + 16, np.uint8)
    mis[3:3 + n] = hbuf
    _same(engine.resp_decode((mis[3:3 + n], offs), device=False), want)
    # each capacity one short: sizes only, every array keeps its fill
    sizes = want["sizes"]
    nconn = len(offs) - 1
    for short in range(6):
        if sizes[short] == 0:
            continue
        caps = list(sizes)
        caps[short] -= 1
        for device in (False, True):
            if device:
                mk = lambda k, dt: torch.full((k + 1,), FILL, dtype=getattr(torch, dt), device=dev)
            else:
                mk = lambda k, dt: np.full(k + 1, FILL, {"uint8": np.uint8, "int32": np.uint32, "int64": np.uint64}[dt])
            mkh = lambda k, dt: np.full(k + 1, FILL, dt)
            cc, cw, cr, ck, cv, cg = caps
            out = {"conn_used": mk(nconn, "int64"), "conn_err": mk(nconn, "uint8"), "cmd_conn": mk(cc, "int32"),
                   "cmd_kind": mk(cc, "uint8"), "cmd_phase": mk(cc, "int32"), "cmd_word_offs": mk(cc + 1, "int64"),
                   "word_off": mk(cw, "int64"), "word_len": mk(cw, "int64"), "row_cmd": mk(cr, "int32"),
                   "key_bytes": mk(ck, "uint8"), "key_offs": mk(cr + 1, "int64"), "val_bytes": mk(cv, "uint8"),
                   "val_offs": mk(cr + 1, "int64"), "num": mk(cr, "int64"), "op": mk(cr, "uint8"),
                   "group_phase": mkh(cg, np.uint32), "group_class": mkh(cg, np.uint8),
                   "group_offs": mkh(cg + 1, np.uint64)}
            before = {k: _host(v).copy() for k, v in out.items()}
            got_sizes, _ = engine.resp_decode_caps((buf, offs), caps, device, out)
            engine.sync()
            assert got_sizes == sizes
            for k, v in out.items():
                np.testing.assert_array_equal(_host(v), before[k], err_msg=f"{k} written with capacity {short} short")
    # no connection, and connections without a byte
    got = engine.resp_decode([], device=False)
    assert got["sizes"] == [0] * 6 and got["group_offs"].tolist() == [0] and got["key_offs"].tolist() == [0]
    got = engine.resp_decode([b"", b"", b""], device=False)
    assert got["sizes"] == [0] * 6 and got["conn_used"].tolist() == [0, 0, 0] and got["conn_err"].tolist() == [0, 0, 0]


def _wire_equal(a, b, ctype, col):
    n = a.nkeys(ctype)
    assert n == b.nkeys(ctype)
    for wa, wb in ((a.state_wire(ctype, 0, n), b.state_wire(ctype, 0, n)),
                   (a.flush_wire(ctype, col=col), b.flush_wire(ctype, col=col))):
        assert wa.keys() == wb.keys()
        for name in wa:
            np.testing.assert_array_equal(_host(wa[name]), _host(wb[name]), err_msg=name)


def test_hand_off(engine):
    """a decoded group's device columns passed untouched to the keyed writes
    leave the engine as the same commands given from Python lists do"""
    from jylis_amd import _lib
    from jylis_amd.engine import Engine
    from jylis_amd.resp_in import run_group
    long_v = b"long value " * 40
    sets = [("k%d" % (i % 7), b"v%d" % i if i % 4 else long_v + b"%d" % i, 100 + (i * 7) % 13) for i in range(40)]
    tl = [(ref.TLOG_INS, "l%d" % (i % 5), b"e%d" % (i % 11), 50 + i % 9) for i in range(60)] + \
         [(ref.TLOG_TRIMAT, "l1", b"", 52), (ref.TLOG_TRIM, "l2", b"", 3), (ref.TLOG_CLR, "l3", b"", 0),
          (ref.TLOG_INS, "l3", long_v, 99)]
    incs = [("c%d" % (i % 6), i * 3 + 1) for i in range(30)]
    opname = {ref.TLOG_INS: "INS", ref.TLOG_TRIMAT: "TRIMAT", ref.TLOG_TRIM: "TRIM", ref.TLOG_CLR: "CLR"}
    conns = [b"".join(R("TREG", "SET", k, v, ts) for k, v, ts in sets),
             b"".join(R("TLOG", "INS", k, v, ts) if op == ref.TLOG_INS else
                      R("TLOG", opname[op], k) if op == ref.TLOG_CLR else R("TLOG", opname[op], k, ts)
                      for op, k, v, ts in tl),
             b"".join(R("GCOUNT", "INC", k, v) for k, v in incs),
             b"".join(R("PNCOUNT", "DEC", k, v) for k, v in incs)]
    other = Engine(device=0)
    try:
        col, ocol = engine.replica_col(7), other.replica_col(7)
        d = engine.resp_decode(conns, device=True)
        assert d["group_class"].tolist() == [_lib.CMD_GCOUNT_INC, _lib.CMD_PNCOUNT_DEC, _lib.CMD_TREG_SET,
                                             _lib.CMD_TLOG_WRITE]
        for g in range(4):
            assert run_group(engine, d, g, col) == [b"+OK\r\n"] * int(d["group_offs"][g + 1] - d["group_offs"][g])
        other.treg_set_keys([k for k, _, _ in sets], [ts for _, _, ts in sets], [v for _, v, _ in sets])
        other.tlog_write_keys([op for op, _, _, _ in tl], [k for _, k, _, _ in tl], ts=[ts for _, _, _, ts in tl],
                              arg=[ts for _, _, _, ts in tl], values=[v for _, _, v, _ in tl])
        other.counter_write_keys(_lib.GCOUNT, 0, ocol, [k for k, _ in incs], [v for _, v in incs])
        other.counter_write_keys(_lib.PNCOUNT, 1, ocol, [k for k, _ in incs], [v for _, v in incs])
        for ctype in (_lib.TREG, _lib.TLOG, _lib.GCOUNT, _lib.PNCOUNT):
            _wire_equal(engine, other, ctype, col)
    finally:
        other.close()


def _exec_against_mirror(engine, conns, feeds=1):
    """exec_resp over `conns` against the host mirror fed the same commands one
    at a time; `feeds`: the buffers are cut into that many heartbeats, the tails kept"""
    from jylis_amd.host import Database
    from jylis_amd.resp_in import exec_resp
    db = Database(device=0, identity=1)
    try:
        want = []
        for c in conns:
            cmds, used, err = ref.frame(c, 0, len(c))
            assert used == len(c) and not err
            want.append(b"".join(db.apply(*[c[o:o + n] for o, n in words]) for words in cmds))
        got = [b""] * len(conns)
        pending = [b""] * len(conns)
        for f in range(feeds):
            cut = [c[len(c) * f // feeds:len(c) * (f + 1) // feeds] for c in conns]
            pending = [p + x for p, x in zip(pending, cut)]
            res = exec_resp(engine, pending, 1, lambda words: db.apply(*words))
            for i, (reply, used, closed) in enumerate(res):
                assert not closed
                got[i] += reply
                pending[i] = pending[i][used:]
        assert pending == [b""] * len(conns)
        assert got == want
    finally:
        db.close()


def test_end_to_end_docs_sessions(engine):
    kat = json.load(open(GOLD))
    conns = [b"".join(b for b, _, _ in RC.doc_requests(kat, name, typ))
             for name, typ in (("treg_doc", "TREG"), ("tlog_doc", "TLOG"), ("gcount_doc", "GCOUNT"),
                               ("pncount_doc", "PNCOUNT"))]
    _exec_against_mirror(engine, conns)


def test_end_to_end_mixed(engine):
    """several connections, every kind, HOST commands with their help texts, in
    one heartbeat and cut into three"""
    conns = RC.phases() + [b"".join(RC.kinds(False)[0])] + RC.tricky()
    _exec_against_mirror(engine, conns)


def test_end_to_end_fed_in_pieces():
    from jylis_amd.engine import Engine
    e = Engine(device=0)
    try:
        _exec_against_mirror(e, RC.phases() + RC.tricky(), feeds=3)
    finally:
        e.close()
