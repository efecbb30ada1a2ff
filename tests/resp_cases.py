"""The case tables of the RESP reply tests, shared by tests/test_get_resp_cpu.py
(which asserts coverage conditions on the expected output, on the oracle
alone) and tests/test_get_resp_gpu.py (which runs them on the engine).

A state is a list of steps, each ("converge", batch table) or ("write",
commands); the CPU test applies them to an oracle repo, the GPU test to an
oracle repo and to the engine's repo alike.
"""
import numpy as np

import get_ref
import resp_ref
from get_ref import ALL

IDENT = 0x5EED_0000_0000_6E75
VLENS = (0, 1, 7, 8, 9, 10, 16, 17, 99, 100, 300)
# log length -> key (the key lengths 1, 8, 16, 17 and 40 bytes among them)
SPECIAL = {1: b"a", 9: b"len8key_", 10: b"sixteen-byte-key", 11: b"seventeen-bytes-k", 63: b"k40-" + b"y" * 36}
SPECIAL.update({n: b"log%d" % n for n in (64, 65, 99, 100, 101, 255, 256, 257, 999, 1000, 5000)})
CLEARED = b"cleared"
ONLY_CUTOFF = b"only-cutoff"
TSEDGE = b"tsedge"  # one-digit and twenty-digit timestamps beside empty values
BIG = b"bigvalue"   # a four-digit $<len>
MISSING = (b"nobody", b"k9999", b"", b"seventeen-bytes-K")
SHORT = [b"k%04d" % i for i in range(120)]
# the writer (k_wire_gather, jy_wire.hpp) stages a workgroup's slice of the
# piece offsets in LDS when it has at most kStage = 1024 of them, and reads
# them from memory otherwise.  A workgroup writes 2,048 bytes; only a run of
# missing TREG keys ($-1\r\n: 5 bytes and 4 pieces a reply, 1,640 pieces a
# workgroup) is dense enough for the second path.
K_STAGE = 1024
TILE_BYTES = 2048
TREG_MISSING_RUN = 600  # 3,000 bytes of nil replies: at least one whole workgroup inside the run


def val(j):
    n = VLENS[j % len(VLENS)]
    return ((b"v%05d-" % j) * 50)[:n]


def ts_of(j):
    return 1000 + j - (1 if j % 16 == 1 else 0)  # entry 16 q + 1 ties with entry 16 q: two values at one timestamp


def apply_steps(steps, want, got=None):
    """run the steps on the oracle repo `want` and, when given, on the GPU repo `got`"""
    for kind, arg in steps:
        if kind == "converge":
            want.converge(arg)
            if got is not None:
                got.converge_deltas(arg)
        elif want.ctype == 3:  # TLOG commands
            for c in arg:
                getattr(want, "tlog_" + c[0].lower())(*c[1:])
            if got is not None:
                got.write(arg)
        else:  # TREG SETs, one call: a key repeated in it leaves pending duplicates
            for k, v, ts in arg:
                want.treg_set(k, v, ts)
            if got is not None:
                got.set([k for k, _, _ in arg], [v for _, v, _ in arg], [ts for _, _, ts in arg])


def state_keys(st):
    kb, ko = np.asarray(st["key_bytes"], np.uint8).tobytes(), np.asarray(st["key_offs"], np.int64)
    return [kb[ko[i]:ko[i + 1]] for i in range(len(ko) - 1)]


# ---- TLOG ----
def tlog_steps(O):
    a, b = O.Repo(O.TLOG, 11), O.Repo(O.TLOG, 13)
    extra = {257: 3, 5000: 3}  # three entries too many where a raised cutoff drops them
    for n, k in SPECIAL.items():
        for j in range(n + extra.get(n, 0)):
            a.tlog_ins(k, val(j), ts_of(j))
    for j in range(3):
        a.tlog_ins(CLEARED, val(j + 1), 5 + j)
    for i, k in enumerate(SHORT):
        for j in range(1 + i % 6):
            a.tlog_ins(k, val(i + j), 100 + 3 * j + (i % 2))
    for v, ts in ((b"", 0), (b"", 5), (b"x", 9), (b"", 7), (b"", 10**19), (b"", 2**64 - 1), (b"", 3), (b"", 4)):
        a.tlog_ins(TSEDGE, v, ts)
    a.tlog_ins(BIG, b"B" * 1000, 42)
    steps = [("converge", a.flush().table())]
    steps.append(("write", [("CLR", CLEARED), ("TRIMAT", SPECIAL[257], ts_of(3)), ("TRIMAT", SPECIAL[5000], ts_of(3)),
                            ("TRIMAT", ONLY_CUTOFF, 77)] + [("TRIM", k, 2) for k in SHORT[20:40]]))
    for i, k in enumerate(SHORT[50:90]):
        b.tlog_ins(k, val(i), 50 + i)
        b.tlog_ins(k, b"new-%d" % i, 400 + i)
    steps.append(("converge", b.flush().table()))
    return steps


def tlog_queries(keys):
    """name -> (keys, counts or None, what or None); `keys`: the state's keys"""
    G, S, C = resp_ref.GET, resp_ref.SIZE, resp_ref.CUTOFF
    sp, lens = list(SPECIAL.values()), list(SPECIAL)
    rng = np.random.default_rng(7)
    order = [keys[i] for i in rng.permutation(len(keys))]
    cases = {"every_key": (order + list(MISSING), None, None)}
    k257 = SPECIAL[257]
    cases["repeated"] = ([k257, SHORT[2], k257, k257, SHORT[2]], [2, ALL, 257, 0, 1], None)
    edge = [CLEARED, TSEDGE] + sp[:12]
    for c in (0, 1, 9, 10, 11, ALL):
        cases["count_%s" % ("all" if c == ALL else c)] = (edge, [c] * len(edge), None)
    cases["count_one_past"] = ([CLEARED] + sp, [1] + [n + 1 for n in lens], None)
    mixed = [SPECIAL[65], CLEARED, MISSING[0], ONLY_CUTOFF, SPECIAL[257], MISSING[2], TSEDGE, SHORT[25]]
    cases["mixed_what"] = (mixed * 3, [ALL, 3, 0] * len(mixed),
                           [G] * len(mixed) + [S] * len(mixed) + [C, G, S, C, C, G, C, S])
    cases["n0"] = ([], None, None)
    hot = SPECIAL[5000]
    cases["hot_alone"] = ([hot], None, None)
    others = (SHORT + sp[:11] + [CLEARED, TSEDGE, BIG] + list(MISSING) + SHORT)[:255]
    assert len(others) == 255
    cases["hot_among_255"] = (others[:100] + [hot] + others[100:], None, None)
    return cases


def tlog_expect(st, case):
    """-> (reply bytes, offs, pieces, sizes [reply bytes, entries, keys found])"""
    keys, counts, what = case
    ans = get_ref.tlog_get(st, keys, counts)
    rb, ro, pieces = resp_ref.tlog(ans, what)
    return rb, ro, pieces, [len(rb), resp_ref.tlog_entries(ans, what), ans["sizes"][2]]


# ---- TREG ----
TREG_TS = (0, 9, 10, 2**64 - 1, 12345)


def treg_steps(O):
    p = O.Repo(O.TREG, 11)
    for i in range(110):  # each value length under each timestamp edge
        p.treg_set(b"r%03d" % i, val(i), TREG_TS[i % len(TREG_TS)])
    p.treg_set(b"bottom", b"", 0)  # converged to ("", 0): interned, unlike a key never touched
    p.treg_set(BIG, b"B" * 1000, 3)
    # a key repeated in one SET call: its duplicates wait for the fold the read runs
    reps = [(b"r007", b"first", 50), (b"r007", b"x" * 300, 51), (b"r007", b"second", 51), (b"r008", b"", 99),
            (b"r008", b"", 99), (b"fresh", b"f", 1)]
    return [("converge", p.flush().table()), ("write", reps)]


def treg_queries(keys):
    run = [b"gone%04d" % i for i in range(TREG_MISSING_RUN)]
    base = [b"never", b"bottom", b"r007", b"r008", b"r007", b"", BIG] + sorted(keys)
    return {"every_key": (base + list(MISSING),),           # staged offsets throughout
            "missing_run": (base[:9] + run + base[9:40],),  # the unstaged offsets path inside the run
            "n0": ([],), "one_missing": ([b"never"],), "one_found": ([b"r005"],)}


def treg_expect(st, case):
    ans = get_ref.treg_get(st, case[0])
    rb, ro, pieces = resp_ref.treg(ans)
    return rb, ro, pieces, [len(rb), ans["sizes"][1]]


# ---- counters ----
def counter_steps(O, ctype):
    p = O.Repo(ctype, 11)
    if ctype == O.GCOUNT:
        p.gcount_inc(b"g0", 0)
        for k in range(1, 20):
            p.gcount_inc(b"nines%d" % k, 10**k - 1)
            p.gcount_inc(b"ten%d" % k, 10**k)
        p.gcount_inc(b"max", 2**64 - 1)
    else:
        p.pncount_inc(b"zero", 5)
        p.pncount_dec(b"zero", 5)
        p.pncount_dec(b"m1", 1)
        p.pncount_dec(b"m10", 10)
        p.pncount_inc(b"imax", 2**63 - 1)
        p.pncount_dec(b"imin", 2**63)
        for k in (1, 9, 18):
            p.pncount_inc(b"p%d" % k, 10**k)
            p.pncount_dec(b"n%d" % k, 10**k - 1)
    return [("converge", p.flush().table())]


def counter_queries(keys):
    return {"every_key": ([b"absent"] + sorted(keys) + [b"", sorted(keys)[0]],), "n0": ([],)}


def counter_expect(st, case, pn):
    found, vals = get_ref.counter_get(st, case[0], pn=pn)
    rb, ro, pieces = resp_ref.counter(vals.tolist())
    return rb, ro, pieces, [len(rb), int(found.sum())]
