"""Keyed batch writes on the GPU (jy_values_pack_mem, jy_counter_write_keys,
jy_treg_set_keys, jy_tlog_write_keys; k_put.hip).

Every case runs two engines and compares them bit for bit on state_wire and
flush_wire: engine A takes the slot path (jy_keys_intern + jy_values_pack + the
write call, host rounds for repeated keys), engine B the keyed call, with host
arrays or device arrays.  Both are also checked against the CPU oracle's
writes, one command at a time."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

IDENT = 0x5EED_0000_0000_9A7E
GCOUNT, PNCOUNT, TREG, TLOG = 0, 1, 2, 3
OPS = {"INS": 0, "TRIMAT": 1, "TRIM": 2, "CLR": 3}
MEMS = ["host", "device"]


@pytest.fixture()
def pair():
    from jylis_amd.engine import Engine
    a, b = Engine(device=0), Engine(device=0)
    try:
        yield a, b
    finally:
        a.close()
        b.close()


def _dev(x, dtype):
    import torch
    a = np.ascontiguousarray(x, dtype)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a.copy()).cuda()


def _strings(items, mem):
    from jylis_amd.engine import encode_keys
    b, o = encode_keys(items)
    return (b, o) if mem == "host" else (_dev(b, np.uint8), _dev(o, np.uint64))


def _col(x, dtype, mem):
    return np.ascontiguousarray(x, dtype) if mem == "host" else _dev(x, dtype)


def _wires_equal(ctype, a, b, col=0, flush=True):
    """state_wire over every slot and flush_wire, array by array; -> B's (state, flush)"""
    assert a.nkeys(ctype) == b.nkeys(ctype)
    n = a.nkeys(ctype)
    sa, sb = a.state_wire(ctype, 0, n), b.state_wire(ctype, 0, n)
    fa = fb = None
    if flush:
        fa, fb = a.flush_wire(ctype, col=col), b.flush_wire(ctype, col=col)
    for wa, wb in ((sa, sb), (fa, fb)):
        if wa is None:
            continue
        assert list(wa) == list(wb)
        for name in wa:
            np.testing.assert_array_equal(np.asarray(wa[name]), np.asarray(wb[name]), err_msg=name)
    return sb, fb


def _table(eng, ctype, wire):
    from jylis_amd.repo import _col_ids, wire_to_table
    return wire_to_table(ctype, wire, _col_ids(eng))


def _cut(b, o, i):
    return bytes(np.asarray(b, np.uint8)[int(o[i]):int(o[i + 1])])


def _canon(ctype, t, drop_empty=False):
    ko = np.asarray(t["key_offs"], np.uint64)
    out = {}
    for i in range(len(ko) - 1):
        k = _cut(t["key_bytes"], ko, i)
        if ctype in (GCOUNT, PNCOUNT):
            row = []
            for p in ("",) if ctype == GCOUNT else ("p_", "n_"):
                o = np.asarray(t[p + "offs"], np.uint64)
                s, e = int(o[i]), int(o[i + 1])
                row.append(sorted(zip(np.asarray(t[p + "ids"], np.uint64)[s:e].tolist(),
                                      np.asarray(t[p + "vals"], np.uint64)[s:e].tolist())))
            out[k] = row
        elif ctype == TREG:
            out[k] = (int(t["ts"][i]), _cut(t["val_bytes"], np.asarray(t["val_offs"], np.uint64), i))
        else:
            eo, vo = np.asarray(t["ent_offs"], np.uint64), np.asarray(t["val_offs"], np.uint64)
            out[k] = (int(t["cutoff"][i]),
                      [(_cut(t["val_bytes"], vo, j), int(t["ts"][j])) for j in range(int(eo[i]), int(eo[i + 1]))])
    return out


def _check_oracle(ctype, eng, want, state_wire, flush_wire):
    assert _canon(ctype, _table(eng, ctype, state_wire)) == _canon(ctype, want.state())
    if flush_wire is not None:
        assert _canon(ctype, _table(eng, ctype, flush_wire)) == _canon(ctype, want.flush().table())


# ---- value packing -------------------------------------------------------------
LENS = [0, 1, 7, 8, 9, 15, 16, 17, 255, 70000, 3, 12, 8, 9]


@pytest.mark.parametrize("ctype", [TREG, TLOG])
@pytest.mark.parametrize("mem", MEMS)
def test_values_pack_mem(pair, mem, ctype):
    """the same handles and the same arena bytes as jy_values_pack, twice in a
    row (the first has to grow the 64 KiB arena for its 70,000-byte value, the
    second starts from the arena end the first left)"""
    import put_ref as P
    a, b = pair
    rng = np.random.default_rng(11)
    for rnd in range(2):
        vals = [bytes(rng.integers(0, 256, n, dtype=np.uint8)) for n in (LENS if rnd == 0 else LENS[::-1] + [13])]
        before = a.arena_usage(ctype)[0]
        assert before == b.arena_usage(ctype)[0]
        pre_a, lr_a = a.pack_values(ctype, vals)
        pre_b, lr_b = b.values_pack_mem(ctype, _strings(vals, mem))
        if mem == "device":
            b.sync()
            pre_b, lr_b = pre_b.cpu().numpy().view(np.uint64), lr_b.cpu().numpy().view(np.uint64)
        pre_r, lr_r, tail = P.pack_ref(vals, before)
        np.testing.assert_array_equal(pre_a, pre_r)
        np.testing.assert_array_equal(lr_a, lr_r)
        np.testing.assert_array_equal(pre_b, pre_r)
        np.testing.assert_array_equal(lr_b, lr_r)
        na, nb = a.arena_usage(ctype)[0], b.arena_usage(ctype)[0]
        assert na == nb == before + len(tail)
        assert a.arena_read(ctype, before, na - before) == b.arena_read(ctype, before, nb - before) == tail
    # host handles out of device values, and the other way round
    vals = [b"", b"12345678", b"123456789", b"x" * 40]
    pre_r, lr_r, _ = P.pack_ref(vals, b.arena_usage(ctype)[0])
    pre_b, lr_b = b.values_pack_mem(ctype, _strings(vals, mem), device_out=(mem == "host"))
    if mem == "host":
        b.sync()
        pre_b, lr_b = pre_b.cpu().numpy().view(np.uint64), lr_b.cpu().numpy().view(np.uint64)
    np.testing.assert_array_equal(pre_b, pre_r)
    np.testing.assert_array_equal(lr_b, lr_r)


def test_bad_host_batches_apply_nothing(pair):
    from jylis_amd.engine import EngineError
    _, b = pair
    kb = np.frombuffer(b"abcd", np.uint8)
    good = np.array([0, 2, 4], np.uint64)
    with pytest.raises(EngineError) as e:  # offsets that do not ascend
        b.tlog_write_keys(np.zeros(2, np.uint8), (kb, np.array([0, 3, 2], np.uint64)), np.zeros(2, np.uint64),
                          np.zeros(2, np.uint64), (kb, good))
    assert e.value.code == -1
    with pytest.raises(EngineError) as e:  # an unknown op
        b.tlog_write_keys(np.array([0, 4], np.uint8), (kb, good), np.zeros(2, np.uint64), np.zeros(2, np.uint64),
                          (kb, good))
    assert e.value.code == -1
    with pytest.raises(EngineError) as e:  # INS without a value column
        b.tlog_write_keys(np.zeros(2, np.uint8), (kb, good), np.zeros(2, np.uint64))
    assert e.value.code == -1
    with pytest.raises(EngineError) as e:  # value offsets that do not ascend
        b.treg_set_keys((kb, good), np.zeros(2, np.uint64), (kb, np.array([0, 3, 1], np.uint64)))
    assert e.value.code == -1
    assert b.nkeys(TLOG) == 0 and b.nkeys(TREG) == 0 and b.tlog_deltas_size() == 0


# ---- TLOG ----------------------------------------------------------------------
def _tlog_columns(cmds):
    n = len(cmds)
    ops = np.array([OPS[c[0]] for c in cmds], np.uint8)
    ts, arg, vals = np.zeros(n, np.uint64), np.zeros(n, np.uint64), [b""] * n
    for i, c in enumerate(cmds):
        if c[0] == "INS":
            vals[i], ts[i] = c[2], c[3]
        elif c[0] == "TRIMAT":
            ts[i] = c[2]
        elif c[0] == "TRIM":
            arg[i] = c[2]
    return ops, [c[1] for c in cmds], ts, arg, vals


def _tlog_apply(O, want, a, b, cmds, mem):
    """the same batch through the oracle, the slot path (A) and the keyed call (B)"""
    for c in cmds:
        if c[0] == "INS":
            want.tlog_ins(c[1], c[2], c[3])
        elif c[0] == "TRIMAT":
            want.tlog_trimat(c[1], c[2])
        elif c[0] == "TRIM":
            want.tlog_trim(c[1], c[2])
        else:
            want.tlog_clr(c[1])
    ops, keys, ts, arg, vals = _tlog_columns(cmds)
    slots = a.intern(TLOG, keys)
    pre, lr = a.pack_values(TLOG, vals)
    a.tlog_write(ops, slots, ts, arg, pre, lr)
    b.tlog_write_keys(_col(ops, np.uint8, mem), _strings(keys, mem), _col(ts, np.uint64, mem),
                      _col(arg, np.uint64, mem), _strings(vals, mem))


def _tlog_check(O, want, a, b, flush=True):
    sw, fw = _wires_equal(TLOG, a, b, flush=flush)
    if flush:
        assert a.tlog_deltas_size() == b.tlog_deltas_size() == 0
    _check_oracle(TLOG, b, want, sw, fw)


def _random_cmds(rng, keys, n):
    alphabet = np.frombuffer(b"ab\x00\xff", np.uint8)
    cmds = []
    for _ in range(n):
        k = keys[int(rng.integers(0, len(keys)))]
        r = rng.random()
        if r < 0.7:
            v = b"sharedp_" * int(rng.integers(0, 3)) + bytes(rng.choice(alphabet, int(rng.integers(0, 5))))
            cmds.append(("INS", k, v, int(rng.integers(0, 12))))
        elif r < 0.8:
            cmds.append(("TRIMAT", k, int(rng.integers(0, 14))))
        elif r < 0.93:
            cmds.append(("TRIM", k, int(rng.integers(0, 7))))
        else:
            cmds.append(("CLR", k))
    return cmds


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257])
@pytest.mark.parametrize("mem", MEMS)
def test_tlog_batch_sizes(oracle_mod, pair, mem, n):
    """random batches of n commands over about n / 3 keys (most keys repeat),
    twice: the second batch meets logs, cutoffs and keys the first one made,
    next to keys that do not exist yet"""
    O = oracle_mod
    a, b = pair
    want = O.Repo(O.TLOG, IDENT)
    rng = np.random.default_rng(1000 + n)
    for rnd in range(2):
        keys = [f"log{i}" for i in range(rnd * (n // 6 + 1), rnd * (n // 6 + 1) + n // 3 + 1)]
        _tlog_apply(O, want, a, b, _random_cmds(rng, keys, n), mem)
        _tlog_check(O, want, a, b, flush=rnd == 1)


@pytest.mark.parametrize("rep", [2, 64, 65, 130])
@pytest.mark.parametrize("mem", MEMS)
def test_tlog_hot_key_rounds(oracle_mod, pair, mem, rep):
    """one key named `rep` times among 20 unrepeated keys: ceil(rep / 64) rounds;
    a batch with no repeated key: one round"""
    O = oracle_mod
    a, b = pair
    want = O.Repo(O.TLOG, IDENT)
    rng = np.random.default_rng(rep)
    cold = [("INS", f"cold{i}", b"c%d" % i, 5 + i) for i in range(20)]
    hot = [("INS", "hot", b"value-%03d" % int(rng.integers(0, rep)), int(rng.integers(0, 40))) for _ in range(rep)]
    cmds = cold + hot
    order = rng.permutation(len(cmds))
    r0 = b.tlog_write_rounds()
    _tlog_apply(O, want, a, b, [cmds[i] for i in order], mem)
    r1 = b.tlog_write_rounds()
    assert r1["calls"] == r0["calls"] + 1 and r1["last"] == -(-rep // 64)
    _tlog_check(O, want, a, b, flush=False)
    _tlog_apply(O, want, a, b, [("INS", f"cold{i}", b"again", 3) for i in range(20)] + [("TRIM", "hot", 2)], mem)
    r2 = b.tlog_write_rounds()
    assert r2["last"] == 1 and r2["total"] == r1["total"] + 1
    _tlog_check(O, want, a, b)


@pytest.mark.parametrize("mem", MEMS)
def test_tlog_stretches_and_edges(oracle_mod, pair, mem):
    """INS stretches broken by TRIM 1, TRIMAT, CLR and a TRIM past the end; the
    same (ts, value) twice in one stretch; equal ts with values that share
    their first 8 and their first 16 bytes; INS below the cutoff; value lengths
    around the 8-byte handle and the 16-byte second word, and one of 70,000
    bytes; then an arena collection on both engines"""
    O = oracle_mod
    a, b = pair
    want = O.Repo(O.TLOG, IDENT)
    rng = np.random.default_rng(77)
    big = bytes(rng.integers(0, 256, 70000, dtype=np.uint8))
    first = [("INS", "old", b"seed", 10), ("INS", "old", b"seed2", 12), ("TRIMAT", "cut", 50), ("INS", "cut", b"kept", 60)]
    _tlog_apply(O, want, a, b, first, mem)
    _tlog_check(O, want, a, b, flush=False)
    lens = [0, 1, 7, 8, 9, 15, 16, 17, 255]
    k = "s"
    cmds = [("INS", k, b"x" * n, 20) for n in lens]                       # equal ts, shared prefixes of every length
    cmds += [("INS", k, b"prefix__A", 21), ("INS", k, b"prefix__B", 21), ("INS", k, b"prefix__A", 21)]  # a duplicate
    cmds += [("INS", k, b"0123456789abcdef_1", 22), ("INS", k, b"0123456789abcdef_0", 22)]
    cmds += [("TRIM", k, 1)]
    cmds += [("INS", k, b"after trim", 5), ("INS", k, big, 30), ("INS", k, b"t31", 31)]  # the first is below the cutoff
    cmds += [("TRIMAT", k, 30)]
    cmds += [("INS", k, b"u", 40), ("INS", k, b"u", 40), ("INS", k, b"v", 40)]
    cmds += [("TRIM", k, 99)]                                               # past the end: nothing
    cmds += [("INS", k, b"w", 41)]
    cmds += [("CLR", k)]
    cmds += [("INS", k, b"last", 41), ("INS", k, b"last", 42), ("INS", k, big[:300], 42)]
    # interleaved with an existing log, a log under a cutoff and new keys
    other = [("INS", "old", b"seed", 10), ("INS", "old", b"new", 11), ("INS", "cut", b"below", 49),
             ("INS", "cut", b"kept", 60), ("INS", "cut", b"above", 61), ("CLR", "empty"), ("TRIM", "fresh", 0),
             ("INS", "fresh2", big[:9], 1)]
    mixed, i, j = [], 0, 0
    while i < len(cmds) or j < len(other):
        if j < len(other) and (i >= len(cmds) or rng.random() < 0.25):
            mixed.append(other[j])
            j += 1
        else:
            mixed.append(cmds[i])
            i += 1
    _tlog_apply(O, want, a, b, mixed, mem)
    assert b.tlog_write_rounds()["last"] == 9  # key "s": five INS stretches and four other commands
    sw, _ = _wires_equal(TLOG, a, b, flush=False)
    _check_oracle(TLOG, b, want, sw, None)
    la, lb = a.arena_collect(TLOG), b.arena_collect(TLOG)
    assert la == lb
    _tlog_apply(O, want, a, b, [("INS", k, big, 43), ("INS", "old", b"post-gc", 13)], mem)
    _tlog_check(O, want, a, b)


def test_tlog_write_device_slots_may_repeat(oracle_mod, pair):
    """jy_tlog_write(JY_DEVICE): a device batch that names a slot many times is
    applied in command order (it used to skip both copies of a repeated slot)"""
    O = oracle_mod
    a, b = pair
    want = O.Repo(O.TLOG, IDENT)
    rng = np.random.default_rng(3)
    cmds = _random_cmds(rng, ["p", "q", "r"], 150) + [("INS", f"u{i}", b"only", 1) for i in range(5)]
    for c in cmds:
        {"INS": lambda: want.tlog_ins(c[1], c[2], c[3]), "TRIMAT": lambda: want.tlog_trimat(c[1], c[2]),
         "TRIM": lambda: want.tlog_trim(c[1], c[2]), "CLR": lambda: want.tlog_clr(c[1])}[c[0]]()
    ops, keys, ts, arg, vals = _tlog_columns(cmds)
    for eng, dev in ((a, False), (b, True)):
        slots = eng.intern(TLOG, keys)
        pre, lr = eng.pack_values(TLOG, vals)
        cols = [(ops, np.uint8), (slots, np.uint32), (ts, np.uint64), (arg, np.uint64), (pre, np.uint64),
                (lr, np.uint64)]
        if dev:
            import torch
            cols = [(torch.from_numpy(np.ascontiguousarray(x, t).view(np.int32 if t == np.uint32 else
                                                                     np.int64 if t == np.uint64 else t)).cuda(), t)
                    for x, t in cols]
        eng.tlog_write(*[x for x, _ in cols])
    assert b.tlog_write_rounds()["last"] > 1
    _tlog_check(O, want, a, b)


# ---- counters and TREG: the same key shapes, with repeats ---------------------
def _keys_with_repeats(rng, n):
    base = [f"k{i}" for i in range(max(1, n // 2))] + ["k" * 300]
    ks = [base[int(rng.integers(0, len(base)))] for _ in range(n)]
    if n >= 3:
        ks[0] = ks[n // 2] = ks[-1] = "hot"
    return ks


@pytest.mark.parametrize("ctype", [GCOUNT, PNCOUNT])
@pytest.mark.parametrize("n", [1, 65, 257])
@pytest.mark.parametrize("mem", MEMS)
def test_counter_write_keys(oracle_mod, pair, mem, n, ctype):
    O = oracle_mod
    a, b = pair
    want = O.Repo(ctype, IDENT)
    rng = np.random.default_rng(n + ctype)
    col = a.replica_col(IDENT)
    assert b.replica_col(IDENT) == col
    for rnd in range(2):
        for sign in range(1 + ctype):
            ks = _keys_with_repeats(rng, n) + ([f"new{rnd}"] if rnd else [])
            v = rng.integers(0, 1 << 62, len(ks), dtype=np.uint64)
            v[::3] = np.uint64(2**64 - 1) - rng.integers(0, 1 << 20, len(v[::3]), dtype=np.uint64)  # wraps
            for k, x in zip(ks, v):
                if ctype == GCOUNT:
                    want.gcount_inc(k, int(x))
                else:
                    (want.pncount_dec if sign else want.pncount_inc)(k, int(x.view(np.int64)))
            a.counter_write(ctype, sign, col, a.intern(ctype, ks), v)
            b.counter_write_keys(ctype, sign, col, _strings(ks, mem), _col(v, np.uint64, mem))
    sw, fw = _wires_equal(ctype, a, b, col=col)
    _check_oracle(ctype, b, want, sw, fw)


@pytest.mark.parametrize("n", [1, 64, 65, 257])
@pytest.mark.parametrize("mem", MEMS)
def test_treg_set_keys(oracle_mod, pair, mem, n):
    """SET batches with repeated keys, timestamp ties, shared prefixes and the
    value lengths around the handle's 8 bytes; the second batch meets the
    registers of the first and new keys"""
    O = oracle_mod
    a, b = pair
    want = O.Repo(O.TREG, IDENT)
    rng = np.random.default_rng(500 + n)
    for rnd in range(2):
        ks = _keys_with_repeats(rng, n) + ([f"new{rnd}"] if rnd else [])
        vals = [b"prefix__" * int(rng.integers(0, 3)) + b"y" * LENS[int(rng.integers(0, 9))] for _ in ks]
        if rnd == 0:
            vals[0] = bytes(rng.integers(0, 256, 70000, dtype=np.uint8))
        ts = rng.integers(0, 6, len(ks)).astype(np.uint64)
        for k, v, t in zip(ks, vals, ts):
            want.treg_set(k, v, int(t))
        pre, lr = a.pack_values(TREG, vals)
        a.treg_set(a.intern(TREG, ks), ts, pre, lr)
        b.treg_set_keys(_strings(ks, mem), _col(ts, np.uint64, mem), _strings(vals, mem))
        if rnd == 0:
            _wires_equal(TREG, a, b, flush=False)
    assert a.arena_collect(TREG) == b.arena_collect(TREG)
    sw, fw = _wires_equal(TREG, a, b)
    _check_oracle(TREG, b, want, sw, fw)


# ---- the node --------------------------------------------------------------------
def test_node_write_against_node_get(oracle_mod):
    """Node.write at S = 2 on the copy fabric: each shard's commands in order,
    one keyed write per shard; Node.get reads back what the oracle holds"""
    from jylis_amd.node import Node
    O = oracle_mod
    rng = np.random.default_rng(9)
    node = Node(2, "copy")
    try:
        keys = [f"n{i}" for i in range(12)]
        cmds = _random_cmds(rng, keys, 120)
        want = O.Repo(O.TLOG, IDENT)
        for c in cmds:
            {"INS": lambda: want.tlog_ins(c[1], c[2], c[3]), "TRIMAT": lambda: want.tlog_trimat(c[1], c[2]),
             "TRIM": lambda: want.tlog_trim(c[1], c[2]), "CLR": lambda: want.tlog_clr(c[1])}[c[0]]()
        node.write(TLOG, cmds)
        assert {node.shard_of(k) for k in keys} == {0, 1}
        state = _canon(TLOG, want.state())
        got = node.get(TLOG, keys)
        for k, g in zip(keys, got):
            assert g == state.get(k.encode(), (0, []))[1], k
        sets = [("SET", keys[int(rng.integers(0, 12))], b"v%d" % i, int(rng.integers(0, 5))) for i in range(60)]
        wt = O.Repo(O.TREG, IDENT)
        for _, k, v, t in sets:
            wt.treg_set(k, v, t)
        node.write(TREG, sets)
        regs = _canon(TREG, wt.state())
        for k, g in zip(keys, node.get(TREG, keys)):
            assert g == ((regs[k.encode()][1], regs[k.encode()][0]) if k.encode() in regs else None), k
        incs = [("INC" if rng.random() < 0.6 else "DEC", keys[int(rng.integers(0, 12))], int(rng.integers(1, 99)))
                for _ in range(80)]
        wp = O.Repo(O.PNCOUNT, IDENT)
        for op, k, v in incs:
            (wp.pncount_inc if op == "INC" else wp.pncount_dec)(k, v)
        node.write(PNCOUNT, incs, identity=IDENT)
        assert node.get(PNCOUNT, keys) == [wp.pncount_get(k) for k in keys]
    finally:
        node.close()
