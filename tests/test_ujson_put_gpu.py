"""UJSON INS / RM / CLR by key string on the GPU (jy_resp_decode_opts and
jy_resp_exec_opts with JY_RESP_UJSON_WRITE, jy_ujson_write_keys; k_resp_in.hip,
k_uj_put.hip, k_leaf.hip, k_resp_out.hip).

The decoder is compared array by array with tests/ujson_put_cases.py's
reference, whose inputs tests/test_ujson_put_cpu.py asserts the coverage of.  The
keyed call is compared with UJSONDocs.apply, one command at a time on a second
engine: documents, pending set, wire-form flush and rendered replies.  Execute
replies are byte-exact against jylis_amd.resp_in.exec_resp with the same flags on
a second engine and against the callback-only path on a third; connections use
keys of their own there, and one key written from two connections is compared
with the loop alone (the callback-only path knows no phases among UJSON commands)."""
import functools

import numpy as np
import pytest

import resp_in_ref as ref
import resp_ujson_cases as UC
import ujson_put_cases as PC
from resp_in_ref import request as R
from resp_ujson_cases import get as G

pytestmark = pytest.mark.gpu

ARRAYS = ("conn_used", "conn_err", "cmd_conn", "cmd_kind", "cmd_phase", "cmd_word_offs", "word_off", "word_len",
          "row_cmd", "key_bytes", "key_offs", "val_bytes", "val_offs", "num", "op", "group_phase", "group_class",
          "group_offs")
OK = b"+OK\r\n"
FILL = 0xAB
IDENT = 1
UJSON = 4
INS, RM, CLR = PC.INS, PC.RM, PC.CLR


def _host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _same(got, want):
    assert got["sizes"] == want["sizes"], (got["sizes"], want["sizes"])
    for name in ARRAYS:
        np.testing.assert_array_equal(_host(got[name]).view(want[name].dtype), want[name], err_msg=name)


@functools.lru_cache(maxsize=None)
def _batch(name, flags):
    """decoder inputs joined and decoded by the reference, once -> (bytes, conn_offs, expected)"""
    bufs = {"paths": PC.path_word_counts, "values": PC.value_lengths, "binary": PC.binary_values,
            "edge": PC.block_edge, "phases": PC.phases, "cuts": lambda: [b for b, _, _ in PC.cuts()],
            "mixed": PC.all_inputs}[name]()
    buf, offs = ref.join(bufs)
    return buf, offs, (PC.decode if flags & PC.FLAG_WRITE else UC.decode)(buf, offs, flags)


# ---- the decoder ----
@pytest.mark.parametrize("name", ["paths", "values", "binary", "edge", "phases", "cuts"])
def test_decode(engine, name):
    for flags in (2, 3):
        buf, offs, want = _batch(name, flags)
        assert (want["cmd_kind"] == PC.UJSON_WRITE).any()
        _same(engine.resp_decode((buf, offs), ujson_get=bool(flags & 1), ujson_write=True), want)
        got = engine.resp_decode((buf, offs), device=True, ujson_get=bool(flags & 1), ujson_write=True)
        engine.sync()
        _same(got, want)
    if name == "cuts":
        assert _host(got["conn_used"]).tolist() == [u for _, u, _ in PC.cuts()]
        assert _host(got["conn_err"]).tolist() == [int(c) for _, _, c in PC.cuts()]
    if name == "phases":
        assert _host(got["cmd_phase"]).tolist() == [0, 1, 2, 3, 3, 4, 4, 0, 0, 1, 1, 2, 3, 4]
    if name == "values":  # 255 bytes on the device, 256 the host's
        assert _host(got["cmd_kind"]).tolist()[-2:] == [PC.UJSON_WRITE, ref.HOST]


def test_decode_memory_capacities_and_old_flags(engine):
    import torch
    buf, offs, want = _batch("mixed", 3)
    dev = f"cuda:{engine.device}"
    n = len(buf)
    hbuf = np.frombuffer(buf, np.uint8)
    # device input at an odd byte address, host and device output
    pad = torch.full((n + 32,), FILL, dtype=torch.uint8, device=dev)
    for mis in (1, 3):
        dreq = pad[8 + mis:8 + mis + n]
        dreq.copy_(torch.from_numpy(hbuf.copy()))
        for device in (False, True):
            got = engine.resp_decode((dreq, offs), device=device, ujson_get=True, ujson_write=True)
            engine.sync()
            _same(got, want)
    # host input at an odd byte address
    odd = np.full(n + 16, FILL, np.uint8)
    odd[3:3 + n] = hbuf
    assert odd[3:3 + n].ctypes.data % 2 == 1
    _same(engine.resp_decode((odd[3:3 + n], offs), ujson_get=True, ujson_write=True), want)
    # flags 0 and the GET flag alone: today's outputs on an input that holds UJSON writes
    for flags in (0, 1):
        old = _batch("mixed", flags)[2]
        assert (old["cmd_kind"] != want["cmd_kind"]).any() and not (old["cmd_kind"] == PC.UJSON_WRITE).any()
        for device in (False, True):
            got = engine.resp_decode((buf, offs), device=device, ujson_get=bool(flags))
            engine.sync()
            _same(got, old)
    sizes0, a0 = engine.resp_decode_caps((buf, offs), _batch("mixed", 0)[2]["sizes"], opts=True)
    _same({**{k: a0[k][:len(v)] for k, v in _batch("mixed", 0)[2].items() if k != "sizes"}, "sizes": sizes0},
          _batch("mixed", 0)[2])
    # each capacity one short: sizes only (the value bytes include the leaves), every array keeps its fill
    sizes = want["sizes"]
    assert sizes[4] > _batch("mixed", 1)[2]["sizes"][4]
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
            got_sizes, _ = engine.resp_decode_caps((buf, offs), caps, device, out, ujson_get=True, ujson_write=True)
            engine.sync()
            assert got_sizes == sizes
            for k, v in out.items():
                np.testing.assert_array_equal(_host(v), before[k], err_msg=f"{k} written with capacity {short} short")


# ---- the keyed call against UJSONDocs.apply ----
def _docs(eng):
    from jylis_amd import ujson_doc as U
    from jylis_amd.repo import RepoUJSON
    return U.UJSONDocs(U.GpuDocs(RepoUJSON(eng)), IDENT, U.DeviceLeaves(eng))


class Pair:
    """a: the keyed call; b: UJSONDocs.apply, one command at a time"""

    def __init__(self, inplace=None):
        from jylis_amd.engine import Engine
        self.engines = [Engine(device=0) for _ in range(2)]
        if inplace is not None:
            for e in self.engines:
                e.ujson_set_inplace(inplace)
        self.docs = [_docs(e) for e in self.engines]
        self.keys = []

    def close(self):
        for e in self.engines:
            e.close()

    def batch(self, cmds, device=False):
        """cmds: (op, key, path, value text or None) -> a's info after the call"""
        from jylis_amd.engine import encode_keys
        ops = np.array([c[0] for c in cmds], np.uint8)
        keys = encode_keys([c[1] for c in cmds])
        leaves = encode_keys([b"" if c[0] == CLR else PC.encode_leaf([p.encode() for p in c[2]], c[3].encode())
                              for c in cmds])
        if device:
            import torch
            dev = f"cuda:{self.engines[0].device}"
            t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x).view(dt).copy()).to(dev)
            ops, keys, leaves = t(ops, np.uint8), (t(keys[0], np.uint8), t(keys[1], np.int64)), \
                (t(leaves[0], np.uint8), t(leaves[1], np.int64))
        self.docs[0].b.r.write_keys(ops, keys, leaves, IDENT)
        for op, key, path, value in cmds:
            words = ["UJSON", ("INS", "RM", "CLR")[op], key, *path] + ([value] if op != CLR else [])
            assert self.docs[1].apply([w.encode() for w in words]) == OK
        self.keys = sorted(set(self.keys) | {c[1] for c in cmds})
        return self.engines[0].ujson_write_keys_info()

    def check(self, flush=True):
        a, b = self.engines
        da, db = self.docs
        assert a.nkeys(UJSON) == b.nkeys(UJSON)
        sa, sb = da.b.r.slots_of(self.keys), db.b.r.slots_of(self.keys)
        np.testing.assert_array_equal(sa, sb)
        live = np.array([s for s in sa if int(s) != 0xFFFFFFFF], np.uint32)
        if len(live):
            for x, y in zip(a.ujson_read(live), b.ujson_read(live)):
                np.testing.assert_array_equal(x, y)
            ks = [k for k, s in zip(self.keys, sa) if int(s) != 0xFFFFFFFF]
            assert da.get_resp(ks, [()] * len(ks)) == db.get_resp(ks, [()] * len(ks))
        assert a.ujson_deltas_size() == b.ujson_deltas_size()
        if flush:
            wa, wb = a.flush_wire(UJSON), b.flush_wire(UJSON)
            assert wa.keys() == wb.keys()
            for name in wa:
                np.testing.assert_array_equal(_host(wa[name]), _host(wb[name]), err_msg=name)


@pytest.fixture
def pair():
    p = Pair()
    try:
        yield p
    finally:
        p.close()


@pytest.mark.parametrize("device", [False, True])
def test_write_keys_rounds(pair, device):
    # no repeats: one round
    info = pair.batch([(INS, "k%d" % i, ("p", "q%d" % (i % 3)), str(i)) for i in range(40)], device)
    assert (info["rounds_last"], info["applied"], info["skipped"], info["leaves_put"]) == (1, 40, 0, 40)
    pair.check()
    # one key 5 times among 300 commands: five rounds
    cmds = [(INS, "n%d" % i, ("a",), '"v%d"' % i) for i in range(295)]
    hot = [(INS, "hot", ("t",), '"x"'), (INS, "hot", ("t",), '"y"'), (RM, "hot", ("t",), '"x"'), (CLR, "hot", (), None),
           (INS, "hot", ("u",), "7")]
    for j, c in enumerate(hot):
        cmds.insert(3 + 60 * j, c)
    before = pair.engines[0].ujson_write_keys_info()
    info = pair.batch(cmds, device)
    assert (info["rounds_last"], info["applied"], info["skipped"]) == (5, 300, 0)
    assert info["calls"] == before["calls"] + 1 and info["rounds_total"] == before["rounds_total"] + 5
    pair.check(flush=False)
    assert pair.docs[0].get_resp(["hot"], [()]) == [b'$7\r\n{"u":7}\r\n']
    pair.check()


@pytest.mark.parametrize("device", [False, True])
def test_write_keys_missing_keys_and_order(pair, device):
    a = pair.engines[0]
    # RM / CLR of missing keys: nothing created, and counted
    info = pair.batch([(RM, "ghost", ("a",), "1"), (CLR, "ghost2", (), None)], device)
    assert a.nkeys(UJSON) == 0 and (info["applied"], info["skipped"], info["rounds_last"]) == (0, 2, 0)
    assert a.ujson_deltas_size() == 0
    # an RM before the INS that creates its key, in one batch; a missing key among applied commands
    info = pair.batch([(RM, "new", ("x",), "1"), (INS, "new", ("x",), "1"), (CLR, "ghost", (), None),
                       (INS, "other", (), "true")], device)
    assert (info["applied"], info["skipped"], info["rounds_last"], info["leaves_put"]) == (3, 1, 2, 2)
    assert a.nkeys(UJSON) == 2
    pair.check(flush=False)
    assert pair.docs[0].get_resp(["new"], [()]) == [b'$7\r\n{"x":1}\r\n']
    # the same leaf inserted twice: two dots
    pair.batch([(INS, "two", ("tags",), '"x"'), (INS, "two", ("tags",), '"x"')], device)
    el = a.ujson_read(pair.docs[0].b.r.slots_of(["two"]))[2]
    assert len(el) == 2 and el[0] == el[1]
    pair.check(flush=False)
    # an RM of a leaf that was never put does not grow the store
    usage = a.ujson_leaves_usage()
    info = pair.batch([(RM, "two", ("never",), '"put"'), (RM, "new", ("y",), "2")], device)
    assert a.ujson_leaves_usage() == usage and info["leaves_put"] == 0 and info["applied"] == 2
    pair.check()


def test_write_keys_long_document():
    """a document in the per-column layout: RM and CLR walk the column runs"""
    p = Pair(inplace=4)
    try:
        p.batch([(INS, "long", ("f%d" % i,), str(i)) for i in range(12)] + [(INS, "short", (), "1")])
        p.check(flush=False)
        p.batch([(RM, "long", ("f3",), "3"), (INS, "long", ("f3",), "33"), (RM, "long", ("f7",), "7")], device=True)
        p.check(flush=False)
        assert b'"f3":33' in p.docs[0].get_resp(["long"], [()])[0]
        p.batch([(CLR, "long", (), None), (INS, "long", ("z",), "0")])
        p.check()
        assert p.docs[0].get_resp(["long"], [()]) == [b'$7\r\n{"z":0}\r\n']
    finally:
        p.close()


def test_write_keys_errors(pair):
    from jylis_amd import _lib
    from jylis_amd.engine import EngineError, encode_keys
    import torch
    a = pair.engines[0]
    pair.batch([(INS, "k", ("a",), "1")])
    state = lambda: (a.nkeys(UJSON), a.ujson_deltas_size(), a.ujson_leaves_usage(),
                     [x.tolist() for x in a.ujson_read(np.array([0], np.uint32))], a.ujson_write_keys_info())
    before = state()
    keys, leaves = encode_keys(["k", "fresh"]), encode_keys([PC.encode_leaf([b"a"], b"2")] * 2)
    down = (leaves[0], np.array([0, 9, 5], np.uint64))
    huge = (keys[0], np.array([0, 1, (1 << 24) + 1], np.uint64))
    dev = lambda x: tuple(torch.from_numpy(np.ascontiguousarray(y).view(np.int64 if y.dtype == np.uint64 else np.uint8)
                                           .copy()).to(f"cuda:{a.device}") for y in x)
    for device in (False, True):
        mv = (lambda x: dev(x)) if device else (lambda x: x)
        ops = lambda *o: mv((np.array(o, np.uint8),))[0]
        for args, code in (((ops(0, 3), mv(keys), mv(leaves)), _lib.JY_EINVAL),
                           ((ops(0, 0), mv(keys), mv(down)), _lib.JY_EINVAL),
                           ((ops(0, 0), mv((keys[0], np.array([0, 6, 1], np.uint64))), mv(leaves)), _lib.JY_EINVAL)):
            with pytest.raises(EngineError) as e:
                a.ujson_write_keys(*args, IDENT)
            assert e.value.code == code
            assert state() == before
    with pytest.raises(EngineError) as e:  # a length over its limit (host arrays: no byte is read)
        a.ujson_write_keys(np.array([0, 0], np.uint8), huge, leaves, IDENT)
    assert e.value.code == _lib.JY_ERANGE and state() == before
    # a malformed INS leaf (shorter than its terminator): JY_EINVAL before any document changes
    with pytest.raises(EngineError) as e:
        a.ujson_write_keys(np.array([0, 0], np.uint8), encode_keys(["k", "k"]),
                           (leaves[0], np.array([0, 9, 11], np.uint64)), IDENT)
    assert e.value.code == _lib.JY_EINVAL and state()[3] == before[3] and state()[1] == before[1]
    pair.check()


# ---- execute ----
class Trio:
    """three engines fed the same bytes: a = UJSONDocs.resp_exec(ujson_write=True),
    b = resp_in.exec_resp with both flags (the loop), c = every UJSON command
    through the callback (Engine.resp_exec without flags)"""

    def __init__(self):
        from jylis_amd.engine import Engine
        self.engines = [Engine(device=0) for _ in range(3)]
        self.docs = [_docs(e) for e in self.engines]
        self.applied = []  # the UJSON commands a's callback answered

    def close(self):
        for x in self.engines:
            x.close()

    @staticmethod
    def host(words):
        return b"+host %d\r\n" % len(words)

    def _answer(self, i):
        def f(words):
            if words and bytes(words[0]) == b"UJSON":
                return self.docs[i].apply(words)
            return self.host(words)
        return f

    def run(self, conns, third=True):
        from jylis_amd.resp_in import exec_resp
        a, b, c = self.docs
        spy = a.apply

        def apply(words):
            self.applied.append([bytes(w) for w in words])
            return spy(words)
        a.apply = apply
        try:
            got = a.resp_exec(conns, IDENT, self.host, ujson_write=True)
        finally:
            del a.apply
        with b.leaves.lock():
            loop = exec_resp(self.engines[1], conns, IDENT, self._answer(1), ujson_get=True, ujson_write=True)
        assert got == loop
        if third:
            with c.leaves.lock():
                assert got == self.engines[2].resp_exec(conns, IDENT, self._answer(2))
        return got

    def check_state(self, third=True):
        def read(e):  # (the flush empties the pending set: each engine is read once)
            n = e.nkeys(UJSON)
            return n, e.ujson_deltas_size(), e.state_wire(UJSON, 0, n), e.flush_wire(UJSON)
        na, da, sa, fa = read(self.engines[0])
        for other in self.engines[1:3 if third else 2]:
            nb, db, sb, fb = read(other)
            assert (na, da) == (nb, db)
            for wa, wb in ((sa, sb), (fa, fb)):
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


def test_exec_sessions(trio):
    """INS | GET | RM | GET sessions on several connections with keys of their own,
    SET and a CLR with a path interleaved, a value that is not plain"""
    conns = []
    for c in range(5):
        k = "doc%d" % c
        s = [PC.ins(k, "tags", '"a%d"' % c), PC.ins(k, "tags", '"b"'), PC.ins(k, "n", "deep", str(c)), G(k), G(k, "tags"),
             PC.rm(k, "tags", '"b"'), PC.rm(k, "tags", '"never"'), G(k)]
        if c % 2:
            s += [R("UJSON", "SET", k, "m", '{"x":[1,2]}'), G(k, "m"), PC.ins(k, "m", "x", "3"),
                  R("UJSON", "CLR", k, "m"), G(k), PC.ins(k, "f", "1.0"), G(k, "f")]
        else:
            s += [PC.clr(k), G(k), PC.ins(k, "again", "true"), R("GCOUNT", "INC", "g", 2), G(k), PC.rm("nokey%d" % c, "1"),
                  PC.clr("nokey%d" % c), G("nokey%d" % c)]
        conns.append(b"".join(s))
    conns += [b"", PC.clr("nothing")]
    got = trio.run(conns)
    trio.check_state()
    assert got[6] == (OK, len(conns[6]), False) and got[5][0] == b""
    assert got[0][0].endswith(OK + OK + b"$0\r\n\r\n") and b'$14\r\n{"again":true}\r\n' in got[0][0]
    # only SET, the CLR with a path and the value 1.0 came to the callback
    assert sorted(set(w[1] for w in trio.applied)) == [b"CLR", b"INS", b"SET"]
    assert [w for w in trio.applied if w[1] == b"INS"] == [[b"UJSON", b"INS", b"doc%d" % c, b"f", b"1.0"] for c in (1, 3)]
    assert all(len(w) == 4 for w in trio.applied if w[1] == b"CLR")
    info = trio.engines[0].ujson_write_keys_info()
    assert info["calls"] >= 4 and info["rounds_total"] > info["calls"]  # INS INS INS on one connection: three rounds
    assert trio.engines[0].nkeys(UJSON) == 5


def test_exec_shared_key_and_device_input(trio):
    """one key written from two connections: stream order inside a group, as the loop applies it"""
    import torch
    conns = [PC.ins("shared", "t", '"x"') + PC.ins("shared", "u", "1") + G("shared") + PC.rm("shared", "t", '"y"'),
             PC.ins("shared", "t", '"y"') + PC.rm("shared", "t", '"x"') + G("shared") + PC.clr("own") + G("shared")]
    got = trio.run(conns, third=False)
    trio.check_state(third=False)
    # phase 0: INS x, INS u (connection 0), INS y, RM x (connection 1): the RM sees the first connection's x
    assert got[0][0] == OK + OK + b'$15\r\n{"t":"y","u":1}\r\n' + OK
    assert got[1][0] == OK + OK + b'$15\r\n{"t":"y","u":1}\r\n' + OK + b'$7\r\n{"u":1}\r\n'
    # the same kind of heartbeat from device memory
    more = [PC.ins("shared", "v", "2") + G("shared"), PC.clr("shared") + G("shared")]
    buf, offs = ref.join(more)
    a, b = trio.docs[:2]
    dreq = torch.from_numpy(np.frombuffer(buf, np.uint8).copy()).to(f"cuda:{trio.engines[0].device}")
    assert a.resp_exec((dreq, offs), IDENT, Trio.host, ujson_write=True) == b.resp_exec(more, IDENT, Trio.host,
                                                                                       ujson_write=True)
    trio.check_state(third=False)


def test_exec_without_callback(engine):
    from jylis_amd import _lib
    from jylis_amd.engine import EngineError
    plain = PC.ins("k", "a", "1") + PC.rm("k", "a", "2") + PC.clr("k")
    assert engine.resp_exec([plain], IDENT, None, ujson_write=True) == [(OK * 3, len(plain), False)]
    assert engine.ujson_write_keys_info()["rounds_last"] == 3
    for left in (PC.ins("k", "a", "1.0"), R("UJSON", "SET", "k", "1"), PC.clr("k", "a")):
        with pytest.raises(EngineError) as e:
            engine.resp_exec([plain + left], IDENT, None, ujson_get=True, ujson_write=True)
        assert e.value.code == _lib.JY_EINVAL
    # the write flag alone leaves UJSON GET with the host
    with pytest.raises(EngineError):
        engine.resp_exec([G("k")], IDENT, None, ujson_write=True)
    assert engine.resp_exec([G("k")], IDENT, None, ujson_get=True, ujson_write=True) == [(b"$0\r\n\r\n", len(G("k")), False)]
