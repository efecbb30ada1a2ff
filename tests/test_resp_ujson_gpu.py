"""UJSON GET decoded and answered on the GPU (jy_resp_decode_opts and
jy_resp_exec_opts with JY_RESP_UJSON_GET; k_resp_in.hip, k_uj_render.hip,
k_resp_out.hip).

The decoder is compared array by array with tests/resp_ujson_cases.py's
reference, whose inputs tests/test_resp_ujson_cpu.py asserts the coverage of.
Execute replies are byte-exact against jylis_amd.resp_in.exec_resp(...,
ujson_get=True) on a second engine (state compared afterwards with state_wire)
and against UJSONDocs.apply one command at a time on a third; connections of
one heartbeat use keys of their own, so the order between them is free."""
import functools
import json
import os

import numpy as np
import pytest

import resp_in_ref as ref
import resp_ujson_cases as UC
from resp_in_ref import request as R
from resp_ujson_cases import get as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARRAYS = ("conn_used", "conn_err", "cmd_conn", "cmd_kind", "cmd_phase", "cmd_word_offs", "word_off", "word_len",
          "row_cmd", "key_bytes", "key_offs", "val_bytes", "val_offs", "num", "op", "group_phase", "group_class",
          "group_offs")
OK = b"+OK\r\n"
EMPTY = b"$0\r\n\r\n"
FILL = 0xAB
IDENT = 1
UJSON = 4


def _host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _same(got, want):
    assert got["sizes"] == want["sizes"], (got["sizes"], want["sizes"])
    for name in ARRAYS:
        np.testing.assert_array_equal(_host(got[name]).view(want[name].dtype), want[name], err_msg=name)


@functools.lru_cache(maxsize=None)
def _batch(name):
    """decoder inputs joined and decoded by the reference, once -> (bytes, conn_offs, expected)"""
    bufs = {"paths": UC.path_word_counts, "segments": UC.segment_lengths, "binary": UC.binary_segments,
            "edge": UC.block_edge, "phases": UC.phases, "cuts": lambda: [b for b, _, _ in UC.cuts()],
            "mixed": lambda: (UC.path_word_counts() + UC.segment_lengths() + UC.binary_segments() + UC.block_edge() +
                              UC.phases() + [b for b, _, _ in UC.cuts()] + UC.with_ujson_commands())}[name]()
    buf, offs = ref.join(bufs)
    return buf, offs, UC.decode(buf, offs, UC.FLAG)


# ---- the decoder ----
@pytest.mark.parametrize("name", ["paths", "segments", "binary", "edge", "phases", "cuts"])
def test_decode(engine, name):
    buf, offs, want = _batch(name)
    assert (want["cmd_kind"] == UC.UJSON_GET).any()
    _same(engine.resp_decode((buf, offs), ujson_get=True), want)
    got = engine.resp_decode((buf, offs), device=True, ujson_get=True)
    engine.sync()
    _same(got, want)
    if name == "cuts":
        cuts = UC.cuts()
        assert _host(got["conn_used"]).tolist() == [u for _, u, _ in cuts]
        assert _host(got["conn_err"]).tolist() == [int(c) for _, _, c in cuts]
    if name == "phases":
        assert _host(got["cmd_phase"]).tolist() == [0, 1, 1, 2, 3, 0, 1, 2, 3, 3]
        assert _host(got["group_class"]).tolist() == [ref.TREG_GET, UC.UJSON_GET, ref.TREG_GET, UC.UJSON_GET]


def test_decode_memory_and_capacities(engine):
    import torch
    buf, offs, want = _batch("mixed")
    dev = f"cuda:{engine.device}"
    n = len(buf)
    hbuf = np.frombuffer(buf, np.uint8)
    # device input at an odd byte address, host and device output
    pad = torch.full((n + 32,), FILL, dtype=torch.uint8, device=dev)
    assert pad.data_ptr() % 8 == 0
    for mis in (1, 3):
        dreq = pad[8 + mis:8 + mis + n]
        dreq.copy_(torch.from_numpy(hbuf.copy()))
        for device in (False, True):
            got = engine.resp_decode((dreq, offs), device=device, ujson_get=True)
            engine.sync()
            _same(got, want)
    # host input at an odd byte address
    odd = np.full(n + 16, FILL, np.uint8)
    odd[3:3 + n] = hbuf
    assert odd[3:3 + n].ctypes.data % 2 == 1
    _same(engine.resp_decode((odd[3:3 + n], offs), ujson_get=True), want)
    # flags 0: jy_resp_decode_opts is jy_resp_decode on an input that holds UJSON commands
    plain = ref.decode(buf, offs)
    assert (plain["cmd_kind"] != want["cmd_kind"]).any()
    sizes, a = engine.resp_decode_caps((buf, offs), plain["sizes"], opts=True)
    sizes0, a0 = engine.resp_decode_caps((buf, offs), plain["sizes"])
    assert sizes == sizes0 == plain["sizes"]
    for name in ARRAYS:
        np.testing.assert_array_equal(a[name], a0[name], err_msg=name)
        k = len(plain[name])
        np.testing.assert_array_equal(a[name][:k].view(plain[name].dtype), plain[name], err_msg=name)
    da, da0 = (engine.resp_decode_caps((buf, offs), plain["sizes"], True, opts=o)[1] for o in (True, False))
    engine.sync()
    for name in ARRAYS:  # ... and with device output
        k = len(plain[name])
        np.testing.assert_array_equal(_host(da[name])[:k], _host(da0[name])[:k], err_msg=name)
        np.testing.assert_array_equal(_host(da[name])[:k].view(plain[name].dtype), plain[name], err_msg=name)
    # each capacity one short: sizes only (the value bytes include the paths), every array keeps its fill
    sizes = want["sizes"]
    assert sizes[4] > plain["sizes"][4]
    nconn = len(offs) - 1
    for short in range(6):
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
            got_sizes, _ = engine.resp_decode_caps((buf, offs), caps, device, out, ujson_get=True)
            engine.sync()
            assert got_sizes == sizes
            for k, v in out.items():
                np.testing.assert_array_equal(_host(v), before[k], err_msg=f"{k} written with capacity {short} short")


# ---- execute ----
def _docs(eng):
    from jylis_amd import ujson_doc as U
    from jylis_amd.repo import RepoUJSON
    return U.UJSONDocs(U.GpuDocs(RepoUJSON(eng)), IDENT, U.DeviceLeaves(eng))


class Trio:
    """three engines fed the same bytes: a = UJSONDocs.resp_exec (the one call), b =
    resp_in.exec_resp(ujson_get=True) (the loop), c = one command at a time"""

    def __init__(self):
        from jylis_amd.engine import Engine
        from jylis_amd.host import Database
        self.engines = [Engine(device=0) for _ in range(3)]
        self.docs = [_docs(e) for e in self.engines]
        self.db = Database(device=0, identity=IDENT)  # c's commands of the other types
        self.left = []   # the UJSON GETs a's callback answered
        self.sizes = None

    def close(self):
        for x in self.engines + [self.db]:
            x.close()

    @staticmethod
    def host(words):
        """the answer to a HOST command that is no UJSON command"""
        return b"+host %d\r\n" % len(words)

    def _answer(self, i):
        def f(words):
            if words and bytes(words[0]) == b"UJSON":
                return self.docs[i].apply(words)
            return self.host(words)
        return f

    def run(self, conns):
        """-> the (replies, used, closed) of the three, asserted equal"""
        from jylis_amd.resp_in import exec_resp
        a, b, c = self.docs
        spy = a.apply

        def apply(words):
            if bytes(words[1]) == b"GET":
                self.left.append([bytes(w) for w in words])
            return spy(words)
        a.apply = apply
        try:
            raw = a.resp_exec(conns, IDENT, self.host, device=True)
        finally:
            del a.apply
        self.engines[0].sync()
        self.sizes = raw["sizes"]
        rb, ro = _host(raw["reply_bytes"]).tobytes(), _host(raw["conn_reply_offs"]).astype(np.int64)
        got = [(rb[ro[i]:ro[i + 1]], int(_host(raw["conn_used"])[i]), bool(_host(raw["conn_err"])[i]))
               for i in range(len(conns))]
        with b.leaves.lock():
            loop = exec_resp(self.engines[1], conns, IDENT, self._answer(1), ujson_get=True)
        assert got == loop
        one = []
        for buf in conns:
            cmds, used, err = ref.frame(buf, 0, len(buf))
            out = b""
            for words in cmds:
                ws = [buf[o:o + n] for o, n in words]
                if ws and ws[0] == b"UJSON":
                    out += c.apply(ws)
                else:
                    out += self.host(ws) if ws[0] == b"SYSTEM" else self.db.apply(*ws)
            one.append((out, used, bool(err)))
        assert got == one
        return got

    def check_state(self):
        a, b = self.engines[:2]
        n = a.nkeys(UJSON)
        assert n == b.nkeys(UJSON)
        if n:
            wa, wb = a.state_wire(UJSON, 0, n), b.state_wire(UJSON, 0, n)
            assert wa.keys() == wb.keys()
            for name in wa:
                np.testing.assert_array_equal(_host(wa[name]), _host(wb[name]), err_msg=name)


@pytest.fixture
def trio():
    t = Trio()
    try:
        yield t
    finally:
        t.close()


def _session_conn():
    """the docs' UJSON session (tests/golden/kat_docs.json) as one connection's requests"""
    steps = json.load(open(os.path.join(ROOT, "tests", "golden", "kat_docs.json")))["ujson_doc"]["steps"]
    out = []
    for st in steps:
        words = ["UJSON", st[0], st[1], *st[2]] + ([st[3]] if st[0] in ("SET", "INS", "RM") else [])
        out.append(R(*words))
    return out


def _fed(run, conns, feeds):
    got, pending = [b""] * len(conns), [b""] * len(conns)
    for f in range(feeds):
        cut = [c[len(c) * f // feeds:len(c) * (f + 1) // feeds] for c in conns]
        pending = [p + x for p, x in zip(pending, cut)]
        for i, (reply, used, err) in enumerate(run(pending)):
            assert not err
            got[i] += reply
            pending[i] = pending[i][used:]
    assert pending == [b""] * len(conns)
    return got


@pytest.mark.parametrize("feeds", [1, 3])
def test_exec_sessions_and_interleaving(trio, feeds):
    """the docs' session; nested maps and sets; a missing key, a path without a leaf, a
    path that is a proper prefix of a segment; UJSON GETs interleaved with every
    other kind and with UJSON writes; one heartbeat, and three with the tails kept"""
    nested = [R("UJSON", "SET", "n", '{"a":{"b":{"c":[1,2,"x"],"d":true},"e":null},"abc":7,"s":[3,4]}'),
              G("n"), G("n", "a"), G("n", "a", "b", "c"), G("n", "ab"), G("n", "a", "zz"), G("none"), G("none", "a"),
              R("UJSON", "INS", "n", "s", "5"), G("n", "s"), R("UJSON", "RM", "n", "s", "3"), G("n", "s"),
              R("UJSON", "CLR", "n", "a", "b"), G("n"), G("n", "abc")]
    mixed = [R("GCOUNT", "INC", "g", 5), G("m"), R("GCOUNT", "GET", "g"), R("UJSON", "SET", "m", "k", '"v"'), G("m"),
             R("PNCOUNT", "DEC", "p", 2), R("PNCOUNT", "INC", "p", 9), G("m", "k"), R("PNCOUNT", "GET", "p"),
             R("TREG", "SET", "t", "reg", 4), G("m"), R("TREG", "GET", "t"), R("TLOG", "INS", "l", "entry", 7),
             G("m", "k"), R("TLOG", "GET", "l"), R("TLOG", "SIZE", "l"), R("SYSTEM", "GETLOG"), G("m")]
    conns = [b"".join(_session_conn()), b"".join(nested), b"".join(mixed), b"", G("none-either")]
    got = _fed(trio.run, conns, feeds)
    trio.check_state()
    assert got[4] == EMPTY and got[3] == b""
    n = got[1]
    assert n.count(b"$0\r\n\r\n") == 4  # n/ab (a proper prefix of abc), n/a/zz, none, none/a
    assert b'"abc":7' in n and n.endswith(b"$1\r\n7\r\n")
    if feeds == 1:
        want = UC.decode(*ref.join(conns), UC.FLAG)
        ngets = int((want["cmd_kind"] == UC.UJSON_GET).sum())
        assert ngets > 20 and trio.sizes[6] == ngets and trio.sizes[7] == 0 and not trio.left
        assert trio.sizes[0] == want["sizes"][0] and trio.sizes[3] == want["sizes"][5]


def test_exec_two_dots_and_device_input(trio):
    """a leaf held under two dots (the same INS from a second replica, converged)
    renders once; the same heartbeat from device memory"""
    import torch
    from jylis_amd import ujson_doc as U
    from jylis_amd.engine import Engine
    from jylis_amd.repo import RepoUJSON
    writes = [R("UJSON", "INS", "two", "tags", '"x"') + R("UJSON", "INS", "two", "n", "deep", "1")]
    assert trio.run(writes) == [(OK + OK, len(writes[0]), False)]
    other = Engine(device=0)
    try:
        od = U.UJSONDocs(U.GpuDocs(RepoUJSON(other)), 2, U.DeviceLeaves(other))
        od.ins("two", ("tags",), '"x"')
        od.ins("two", ("n", "deep"), "1")
        delta = od.b.r.flush_deltas()
        for d in trio.docs:
            d.b.r.converge_deltas(delta)
    finally:
        other.close()
    a = trio.docs[0]
    el = trio.engines[0].ujson_path_read(a.b.r.slots_of(["two"]), [("tags",)], leaves=False)[2]
    assert el.tolist().count(a.leaves.handle(("tags",), '"x"')) == 2  # the path read shows it twice
    reads = [G("two") + G("two", "tags"), G("two", "n") + G("two", "n", "deep") + R("SYSTEM", "GETLOG")]
    got = trio.run(reads)
    frame = lambda t: b"$%d\r\n%s\r\n" % (len(t), t.encode())
    assert got[0][0] == frame('{"n":{"deep":1},"tags":"x"}') + frame('"x"')  # ... rendered once
    assert got[1][0] == frame('{"deep":1}') + frame("1") + Trio.host([b"SYSTEM", b"GETLOG"])
    # device input
    buf, offs = ref.join(reads)
    dreq = torch.from_numpy(np.frombuffer(buf, np.uint8).copy()).to(f"cuda:{trio.engines[0].device}")
    assert a.resp_exec((dreq, offs), IDENT, Trio.host) == got


def test_exec_fallback(trio):
    """a map key holding '"' and a leaf 32 levels below the queried path go to the
    callback, in command order among the HOST commands; one level deeper is rendered
    on the device"""
    import torch
    from jylis_amd import _lib
    from jylis_amd.engine import EngineError
    from test_ujson_render_gpu import DEPTH, ins_many
    assert DEPTH == 31
    deep = tuple("l%d" % i for i in range(DEPTH + 2))  # 33 segments
    for d in trio.docs:
        ins_many(d, [("q", ('we"ird',), "1"), ("q", ("plain",), "2"), ("deep", deep, "3")])
    conns = [G("q") + R("SYSTEM", "GETLOG") + G("q", "plain") + G("deep", deep[0]) + G("deep", *deep[:2]) +
             R("SYSTEM", "GETLOG"),
             G("deep", *deep[:2]) + G("q")]
    got = trio.run(conns)
    assert trio.sizes[7] == 3 and trio.sizes[6] == 3 and trio.sizes[2] == 2
    # phase 0 holds both GETs of q, phase 2 the deep one
    assert trio.left == [[b"UJSON", b"GET", b"q"], [b"UJSON", b"GET", b"q"], [b"UJSON", b"GET", b"deep", b"l0"]]
    assert got[0][0].startswith(b'$%d\r\n{' % len('{"plain":2,"we"ird":1}')) and b'we"ird' in got[0][0]
    # device input: the flagged commands' words come down in one further copy
    eng, docs = trio.engines[0], trio.docs[0]
    buf, offs = ref.join(conns)
    dreq = torch.from_numpy(np.frombuffer(buf, np.uint8).copy()).to(f"cuda:{eng.device}")
    assert docs.resp_exec((dreq, offs), IDENT, Trio.host) == got
    # a flagged query and no callback: JY_EINVAL at that group, nothing retained
    with pytest.raises(EngineError) as e:
        eng.resp_exec([G("q", "plain"), G("q")], IDENT, None, ujson_get=True)
    assert e.value.code == _lib.JY_EINVAL
    with pytest.raises(EngineError):
        eng.resp_replies_caps(2, 0)
    assert eng.resp_exec([G("q", "plain")], IDENT, None, ujson_get=True) == [(b"$1\r\n2\r\n", len(G("q", "plain")), False)]


def test_exec_no_ujson_key_and_assembly(engine):
    """an engine without a UJSON key; UJSON replies between +OK and long TLOG replies
    on one connection"""
    assert engine.nkeys(UJSON) == 0
    docs = _docs(engine)
    assert docs.resp_exec([G("nothing") + G("nothing", "a", "b"), G("x")], IDENT) == \
        [(EMPTY * 2, len(G("nothing") + G("nothing", "a", "b")), False), (EMPTY, len(G("x")), False)]
    # a key and a segment that are not UTF-8: binary-safe on the device and through apply
    odd = G(b"\xffkey", b"\xfe\r\n")
    assert docs.resp_exec([odd], IDENT) == engine.resp_exec([odd], IDENT, docs.apply) == [(EMPTY, len(odd), False)]
    ins = b"".join(R("TLOG", "INS", "long", "entry number %d" % i, 1000 + i) for i in range(120))
    text = '{"k":["%s",1]}' % ("v" * 300)
    conn = ins + R("UJSON", "SET", "doc", text) + R("TLOG", "GET", "long") + G("doc") + R("TREG", "SET", "t", "v", 1) + \
        G("doc", "k") + R("TLOG", "GET", "long")
    got = docs.resp_exec([R("GCOUNT", "INC", "n", 1), conn, G("doc")], IDENT)
    log = _host(engine.tlog_get_resp(["long"])["reply_bytes"]).tobytes()
    whole = docs.get_resp(["doc", "doc"], [(), ("k",)])
    assert len(log) > 2048 and len(whole[0]) > 300
    assert got[1] == (OK * 121 + log + whole[0] + OK + whole[1] + log, len(conn), False)
    assert got[0][0] == OK and got[2][0] == EMPTY  # phase 0: before the SET of its connection's phase 1
