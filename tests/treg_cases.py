"""Case generators for the TREG boundary sweeps (pure numpy / Python).

The TREG merge (jylis_amd/csrc/k_treg.hip) writes its (ts, value) compare out
once per kernel form, on top of a first-occurrence claim (jy_claim_rows) with a
contiguous fast path, a ballot-aggregated path and two alternating bitmaps.
The generators below place chosen pairs and chosen slot layouts on that
geometry.  test_treg_sweep_cpu.py checks every generator against the oracle
alone (and the geometry tags against a tiling model of its own);
test_treg_sweep_gpu.py runs them through the engine.

A LAUNCH is one engine call: {"kind": "keyed" | "block" | "set", "slots",
"ts", "vals", "dups", "skips", "device_only"}; entry i names slots[i] (a block
launch: slot0 + i) with (ts[i], vals[i]).  "dups" is the number of entries that
are not the first of their slot: what one keyed launch must leave in the
pending duplicate list.  A CASE is a name, its launches, its tags and the
declared outcome per slot: "replaced" or "kept", and the (ts, value) expected.
Slot s carries the key key_of(s): the tests intern the keys in slot order."""
import struct

import numpy as np

NO_SLOT = 0xFFFFFFFF

# the kernels' geometry.  The first four are what jy_treg_claim_info reports of
# the build (asserted by test_treg_sweep_cpu.py); the rest are fixed in the
# source: 64 lanes, 256 threads, kAgg words aggregated per row, 64-record tail
# chunks, 2 records per lane in a fold round, and a slice clear while the
# bitmap is at most 4096 bytes per workgroup.
UNROLL, ROUTED_UNROLL, FOLD_ROUNDS, TILE = 4, 2, 3, 1024
LANES, THREADS, AGG, TAIL_CHUNK, FOLD_TILE, CLEAR_PER_WG = 64, 256, 3, 64, 512, 4096
WAVE = LANES * UNROLL  # entries of one wave of a keyed launch

SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)
STARTS = (0, 1, 31, 32, 33, 63)
DENSE_STARTS = (0, 1, 63, 64, 65)
FOLD_M = (1, 2, 3, 4, 5, 6, 67, 68, 69, 133)
TAIL_RECORDS = (0, 1, 2, 63, 64, 65, 129)
WINNER_AT = (0, 63, 64, 255, 256, 1023, 1024)  # and n - 1
MAX_AT = (0, 1, 4, -1)  # the maximum at the first, second, fifth and last occurrence
ROW_WORDS = (1, 3, 4, 64)
SAME_SLOT_LANES = (2, 3, 64)
SHARED_AGAIN = (1, 32, 64)

TIES = [  # test_parity_treg.py's list: (state, delta) at equal timestamps
    (b"", b"a"), (b"a", b""), (b"abc", b"abd"), (b"abcdefgh", b"abcdefgh\x00"),
    (b"abcdefghij", b"abcdefghik"), (b"abcdefghijk", b"abcdefghij"), (b"\xff", b"\x00\x00"),
    (b"same-long-value!", b"same-long-value!"), (b"a\x00", b"a"), (b"zzzzzzzzzzzzzzzzzzzz1", b"zzzzzzzzzzzzzzzzzzzz2"),
]
VALUE_LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 24, 25)
DIFF_AT = (0, 7, 8, 15, 16, 17)  # and the last byte
H = 1 << 32
TS_PAIRS = {  # (state ts, delta ts): the later one wins whatever the values
    "low word": (7 * H + 5, 7 * H + 6), "low word, bit 31": (2**31 - 1, 2**31), "high word": (H + 5, 2 * H + 5),
    "high word, bit 63": (5, 2**63 + 5), "high against low": (H + 9, 2 * H + 3), "2^63 - 1 | 2^63": (2**63 - 1, 2**63),
    "2^64 - 1": (2**64 - 2, 2**64 - 1), "2^64 - 1 against 1": (1, 2**64 - 1),
}
TS_TIES = (2**63, 2**64 - 1)  # equal timestamps with bit 63 set: the value decides


def key_of(slot):
    return b"g%06d" % slot


def pre_of(val):
    """the handle's prefix word: the first 8 value bytes, big-endian, zero padded"""
    return int.from_bytes(val[:8].ljust(8, b"\0"), "big")


def launch(kind, slots, ts, vals, dups=0, device_only=False):
    slots = np.asarray(slots, np.uint32)
    assert len(slots) == len(ts) == len(vals)
    return {"kind": kind, "slots": slots, "ts": [int(t) for t in ts], "vals": list(vals), "dups": dups, "skips": 0,
            "device_only": device_only}


def block(slot0, ts, vals):
    L = launch("block", slot0 + np.arange(len(ts)), ts, vals)
    L["slot0"] = slot0
    return L


def _csr(items):
    offs = np.zeros(len(items) + 1, np.uint64)
    offs[1:] = np.cumsum([len(x) for x in items], dtype=np.uint64)
    return np.frombuffer(b"".join(items), np.uint8), offs


def table(L):
    """a launch as the oracle's batch table (entries without a slot left out)"""
    keep = [i for i, s in enumerate(L["slots"]) if s != NO_SLOT]
    kb, ko = _csr([key_of(int(L["slots"][i])) for i in keep])
    vb, vo = _csr([L["vals"][i] for i in keep])
    return {"key_bytes": kb, "key_offs": ko, "ts": np.array([L["ts"][i] for i in keep], np.uint64), "val_bytes": vb,
            "val_offs": vo}


class Model:
    """the register file as plain Python: LWW by (ts, value) in Python's own int and bytes order"""

    def __init__(self, n):
        self.ts, self.val = [0] * n, [b""] * n

    def apply(self, L):
        """-> the slots an entry of the launch replaced"""
        hit = set()
        for s, t, v in zip(L["slots"], L["ts"], L["vals"]):
            s = int(s)
            if s != NO_SLOT and (t, v) > (self.ts[s], self.val[s]):
                self.ts[s], self.val[s] = t, v
                hit.add(s)
        return hit


class _Clock:
    """fresh, growing timestamps: every launch of a geometry sweep wins everywhere"""

    def __init__(self, t=1000):
        self.t = t

    def __call__(self):
        self.t += 1
        return self.t


def gval(t, i):
    """entry i's value in a launch at time t: distinct, ordered by i, every fifth one longer than 8 bytes"""
    v = struct.pack(">II", t & 0xFFFFFFFF, i)
    return v + b"-long" + bytes([i & 0xFF]) if i % 5 == 3 else v


# ---- a. the order matrix ---------------------------------------------------------------------
def _pair(name, state, delta, replaced=None, same_lr=False):
    """replaced: what the pair's construction says; None = Python's order of (ts, bytes), as
    test_parity_treg.py takes it for TIES (the CPU test holds both against the oracle)"""
    if replaced is None:
        replaced = delta > state
    return {"name": name, "state": state, "delta": delta, "replaced": replaced,
            "expect": delta if replaced else state, "same_lr": same_lr}


def order_pairs():
    out = []
    for name, (lo, hi) in TS_PAIRS.items():  # the values pull the other way
        out.append(_pair(f"ts {name}, later", (lo, b"m"), (hi, b"a"), True))
        out.append(_pair(f"ts {name}, earlier", (hi, b"m"), (lo, b"z"), False))
        out.append(_pair(f"ts {name}, later, long", (lo, b"m" * 12), (hi, b"a" * 12), True))
        out.append(_pair(f"ts {name}, earlier, long", (hi, b"m" * 12), (lo, b"z" * 12), False))
    for t in TS_TIES:
        out.append(_pair(f"ts tie {t}, greater value", (t, b"m"), (t, b"n"), True))
        out.append(_pair(f"ts tie {t}, smaller value", (t, b"n"), (t, b"m"), False))
        out.append(_pair(f"ts tie {t}, equal", (t, b"m" * 9), (t, b"m" * 9), False, same_lr=True))
    T = 7
    for a, b in TIES:
        out.append(_pair(f"TIES {a!r} {b!r}", (T, a), (T, b), None, same_lr=a == b))
    for a, b in ((b"\x7f", b"\x80"), (b"\x7fzzzzzzz", b"\x80"), (b"\x7f" * 8, b"\xff" * 8),
                 (b"\x7f" + b"z" * 10, b"\x80" + b"a" * 10), (b"abcd\x7fzzz", b"abcd\x80")):
        out.append(_pair(f"top bit {a!r} < {b!r}", (T, a), (T, b), True))
        out.append(_pair(f"top bit {b!r} > {a!r}", (T, b), (T, a), False))
    for n in VALUE_LENGTHS:
        x = bytes(range(0x41, 0x41 + n))
        for d in sorted({d for d in DIFF_AT + (n - 1,) if 0 <= d < n}):
            for lo, hi in ((x[d], x[d] + 1), (0x7F, 0x80)):  # a step up; a step across the sign bit of a byte
                a, b = x[:d] + bytes([lo]) + x[d + 1:], x[:d] + bytes([hi]) + x[d + 1:]
                out.append(_pair(f"len {n} differs at {d}: {lo:#x} < {hi:#x}", (T, a), (T, b), True))
                out.append(_pair(f"len {n} differs at {d}: {hi:#x} > {lo:#x}", (T, b), (T, a), False))
        out.append(_pair(f"len {n} equal", (T, x), (T, x), False, same_lr=True))
    x = bytes(range(0x61, 0x61 + 25))
    for n in (8, 15, 16, 24):  # a proper prefix against the value one byte longer
        out.append(_pair(f"prefix {n}/{n + 1}", (T, x[:n]), (T, x[:n + 1]), True))
        out.append(_pair(f"prefix {n + 1}/{n}", (T, x[:n + 1]), (T, x[:n]), False))
    for n in (8, 9, 16):  # a trailing NUL: in a partial 8-byte step it reads like the padding
        out.append(_pair(f"len {n} + NUL, longer", (T, x[:n]), (T, x[:n] + b"\0"), True))
        out.append(_pair(f"len {n} + NUL, shorter", (T, x[:n] + b"\0"), (T, x[:n]), False))
    return out


def order_case(pairs, kind="keyed", reps=1, block_at=None):
    """pair i on slot i: one launch of every state, one of every probe.  reps > 1 names each probe's slot
    reps times in the probe launch (copies a whole sweep of pairs apart: other rows, waves and, through the
    duplicate list, the fold's rounds and its tail).  block_at: both launches as block batches at that slot."""
    P, s0 = len(pairs), block_at or 0
    st = [p["state"] for p in pairs]
    pr = [p["delta"] for p in pairs] * reps
    if block_at is not None:
        Ls = [block(s0, [t for t, _ in st], [v for _, v in st]), block(s0, [t for t, _ in pr], [v for _, v in pr])]
    else:
        Ls = [launch("keyed", np.arange(P), [t for t, _ in st], [v for _, v in st]),
              launch(kind, np.tile(np.arange(P), reps), [t for t, _ in pr], [v for _, v in pr], dups=P * (reps - 1))]
    return {"name": f"order matrix x{reps} {kind}", "launches": Ls, "tags": {"reps": reps}, "nslots": s0 + P,
            "outcome": {s0 + i: "replaced" if p["replaced"] else "kept" for i, p in enumerate(pairs)},
            "expect": {s0 + i: p["expect"] for i, p in enumerate(pairs)},
            "same_lr": {s0 + i for i, p in enumerate(pairs) if p["same_lr"]}}


# ---- b. claim geometry ----------------------------------------------------------------------
def clear_mode(n, seen_words):
    """how a keyed launch of n entries resets the other bitmap (claim_bits)"""
    grid = max(1, -(-n // TILE))
    nbytes = (seen_words * 4 + 15) & ~15
    return ("memset", grid, 0) if nbytes > grid * CLEAR_PER_WG else ("slice", grid, (-(-nbytes // grid) + 15) & ~15)


def _scatter(rng, k, lo, hi, avoid=()):
    """k distinct slots of [lo, hi), none of `avoid`, in no order"""
    pool = np.setdiff1d(np.arange(lo, hi), np.asarray(list(avoid), np.int64))
    return rng.choice(pool, k, replace=False)


def _layout(name, slots, dups, device_only=False, **tags):
    return {"name": name, "slots": np.asarray(slots, np.int64), "dups": dups, "device_only": device_only, "tags": tags}


def claim_layouts(N, seen_words):
    """slot layouts of one keyed launch each, over a file of N slots whose claim bitmaps hold seen_words
    words.  Tags: fast = the waves (entry index // 256) whose 256 entries are one ascending run."""
    rng = np.random.default_rng(7)
    out = []
    full = lambda n: tuple(range(n // WAVE))
    # the fast path: contiguous runs
    for n in (WAVE, TILE + WAVE):
        for s0 in STARTS:
            out.append(_layout(f"run of {n} at {s0}", s0 + np.arange(n), 0, fast=full(n), start=s0, size=n))
        out.append(_layout(f"run of {n} to the last slot", N - n + np.arange(n), 0, fast=full(n), start=N - n, size=n,
                           last=True))
    # ... broken by one lane: entry j repeats entry i's slot
    n, s0, i = TILE + WAVE, 33, 5
    for rel, j in (("row", 9), ("wave", LANES + 9), ("workgroup", WAVE + 9), ("grid", TILE + 9)):
        s = s0 + np.arange(n)
        s[j] = s[i]
        out.append(_layout(f"run broken in another {rel}", s, 1, fast=tuple(w for w in full(n) if w != j // WAVE),
                           broken=(i, j, rel)))
    # the fast path and the general path on shared bitmap words
    for k in SHARED_AGAIN:
        s0 = 64
        again = s0 + rng.choice(WAVE, k, replace=False)
        w1 = np.concatenate([again, _scatter(rng, WAVE - k, 2048, 8192)])
        out.append(_layout(f"wave 1 names {k} of wave 0's slots", np.concatenate([s0 + np.arange(WAVE), rng.permutation(w1)]),
                           k, fast=(0,), shared=k))
    for s0 in (1, 31, 33, 63):  # the run's first and last bit, and the bits just outside it
        edge = [s0, s0 + WAVE - 1, s0 - 1, s0 + WAVE]
        w1 = np.concatenate([edge, _scatter(rng, WAVE - 4, 2048, 8192)])
        out.append(_layout(f"wave 1 names the ends of the run at {s0}", np.concatenate([s0 + np.arange(WAVE), w1[::-1]]),
                           2, fast=(0,), ends=s0))
    # aggregation: one row (row 1 of the wave) on a chosen number of bitmap words; rows 0, 2, 3 elsewhere
    def wave_with(row, tag, dups, **tags):
        rest = _scatter(rng, WAVE - LANES, 20480, 32768)  # past every w(k) used below
        s = np.concatenate([rest[:LANES], row, rest[LANES:]])
        return _layout(tag, s, dups, fast=(), agg_row=1, **tags)
    w = lambda k: 9216 + 32 * k  # first slot of a word
    out.append(wave_with(np.tile(rng.permutation(w(0) + np.arange(32)), 2), "row on 1 word, every slot twice", 32, words=1))
    out.append(wave_with(rng.permutation(w(2) + 5 + np.arange(64)), "row on 3 words", 0, words=3))
    out.append(wave_with(rng.permutation(np.concatenate([w(k) + 3 + np.arange(16) for k in (10, 12, 15, 19)])),
                         "row on 4 words", 0, words=4))
    out.append(wave_with(np.array([w(30 + k) + 7 for k in range(64)]), "row on 64 words", 0, words=64))
    for k in SAME_SLOT_LANES:
        row = _scatter(rng, LANES, w(100), w(160))
        row[rng.choice(LANES, k, replace=False)] = w(200) + 11
        out.append(wave_with(row, f"{k} lanes of a row on one slot", k - 1, same=k))
    a, b, c = w(300) + np.arange(20), w(301) + np.arange(30), w(302) + np.arange(13)
    row = np.concatenate([a, a[:1], b, c])  # word 300's group holds a repeat; 301's and 302's do not
    out.append(wave_with(row[rng.permutation(64)], "a group with a repeat next to one without", 1, words=3, mixed=True))
    # ragged sizes
    for n in SIZES:
        out.append(_layout(f"ragged run of {n}", 33 + np.arange(n), 0, fast=full(n), size=n))
        out.append(_layout(f"ragged scatter of {n}", _scatter(rng, n, 0, N), 0, fast=(), size=n))
        s = _scatter(rng, n, 0, N)
        rep = np.arange(7, n, 7)
        s[rep] = s[rep - 3]
        out.append(_layout(f"ragged scatter of {n} with repeats", s, len(rep), fast=(), size=n))
    # entries without a slot: first and last lane of row 1, the whole of row 2 (a device batch)
    for rep in (0, 1):
        s = _scatter(rng, WAVE, 0, N)
        s[[LANES, 2 * LANES - 1]] = NO_SLOT
        s[2 * LANES:3 * LANES] = NO_SLOT
        if rep:
            s[3 * LANES + 4] = s[3]
        out.append(_layout(f"no-slot entries, {rep} repeats", s, rep, device_only=True, fast=(), holes=2 + LANES))
    # the slice clear: the first and last byte of the bitmap, both sides of every workgroup's slice
    for n in (TILE + 1, 2 * TILE + 1):
        mode, grid, per = clear_mode(n, seen_words)
        assert mode == "slice", (n, seen_words)
        named = list(range(8)) + list(range(N - 8, N))
        for g in range(1, grid):
            named += [s for s in (per * 8 * g - 1, per * 8 * g) if s < N]
        named = sorted(set(named))
        s = np.concatenate([named, _scatter(rng, n - len(named), 0, N, named)])
        out.append(_layout(f"slice clear, {grid} slices", rng.permutation(s), 0, fast=(), size=n, slices=grid,
                           edges=tuple(named)))
    return out


def geometry_case(lay, clock, kind="keyed", launches=3):
    """a layout applied in consecutive launches at fresh timestamps: each wins everywhere, the
    third claims on the bitmap the first one used"""
    Ls, exp = [], {}
    for _ in range(launches):
        t = clock()
        s = lay["slots"]
        Ls.append(launch(kind, s, [t] * len(s), [gval(t, i) for i in range(len(s))], lay["dups"], lay["device_only"]))
    for i, x in enumerate(lay["slots"]):  # the last launch's greatest value of every slot
        if x != NO_SLOT:
            exp[int(x)] = max(exp.get(int(x), (0, b"")), (t, gval(t, i)))
    return {"name": lay["name"], "launches": Ls, "tags": lay["tags"], "expect": exp,
            "outcome": {s: "replaced" for s in exp}, "same_lr": set()}


# ---- c. fold depth --------------------------------------------------------------------------
LONG = b"fold-depth-long-value-"


def fold_cases(kind="keyed"):
    """one slot named m times in one launch (own slot and own launch per case: the tail then holds
    m - (FOLD_ROUNDS + 1) records), two and three slots interleaved, and 700 slots x 6"""
    out, clock, nxt = [], _Clock(), [0]

    def slot():
        nxt[0] += 1
        return nxt[0] - 1

    def case(name, slots, ents, m, setup=None, same_lr=False, **tags):
        exp = {}
        for s, e in zip(slots, ents):
            exp[int(s)] = max(exp.get(int(s), setup or (0, b"")), e)
        Ls = [launch("keyed", sorted(exp), [setup[0]] * len(exp), [setup[1]] * len(exp))] if setup else []
        Ls.append(launch(kind, slots, [t for t, _ in ents], [v for _, v in ents], dups=len(slots) - len(exp)))
        tags.update(m=m, tail=max(0, m - (FOLD_ROUNDS + 1)) * len(exp))
        out.append({"name": name, "launches": Ls, "tags": tags, "expect": exp,
                    "outcome": {s: "kept" if same_lr else "replaced" for s in exp},
                    "same_lr": set(exp) if same_lr else set()})

    mixed = lambda j: b"v%05d" % j if j % 2 == 0 else LONG + b"%05d" % j
    for m in FOLD_M:
        t0 = clock.t = clock.t + 1000
        asc = [(t0 + j, mixed(j)) for j in range(m)]
        case(f"m={m} ascending", [slot()] * m, asc, m, order="asc")
        case(f"m={m} descending", [slot()] * m, asc[::-1], m, order="desc")
        last = [(t0, LONG + bytes([(j * 37) % m])) for j in range(m)]
        case(f"m={m} equal ts, last byte", [slot()] * m, last, m, order="last byte")
        for at in sorted({a % m for a in MAX_AT if a < m}):
            ents = [(t0 + j, mixed(j)) for j in range(m - 1)]
            ents.insert(at, (t0 + m, b"the maximum"))
            case(f"m={m} maximum at {at}", [slot()] * m, ents, m, max_at=at)
        same = (t0, LONG + b"same")  # the state itself again, each copy at its own arena offset
        case(f"m={m} equal to the state", [slot()] * m, [same] * m, m, setup=same, same_lr=True, equal=True)
    for k in (2, 3):
        m, t0 = 69, clock() + 1000
        ss = [slot() for _ in range(k)]
        slots = [ss[i % k] for i in range(k * m)]
        ents = [(t0 + (i * 29) % (k * m), mixed(i)) for i in range(k * m)]
        case(f"{k} slots interleaved, m=69 each", slots, ents, m, interleaved=k)
    ss, m, t0 = [slot() for _ in range(700)], 6, clock() + 5000
    slots = [ss[k] for r in range(m) for k in range(700)]
    ents = [(t0 + (r * 5 + k) % m, mixed(k % 50)) for r in range(m) for k in range(700)]
    case("700 slots x 6", slots, ents, m, wide=700)
    return out, nxt[0]


# ---- d. dense block geometry ----------------------------------------------------------------
def dense_cases(N):
    """block batches over a file of N slots: every start with every size class, one winner in a stale
    batch of the largest size, a batch that loses everywhere, a batch equal to the state"""
    out, clock = [], _Clock()
    starts = DENSE_STARTS + ("last",)

    def case(name, s0, ents, outcome, **tags):
        L = block(s0, [t for t, _ in ents], [v for _, v in ents])
        out.append({"name": name, "launches": [L], "tags": dict(tags, start=s0, size=len(ents)), "expect": None,
                    "outcome": outcome, "same_lr": set()})

    for k, n in enumerate(SIZES):
        for st in (starts if n == SIZES[-1] else (starts[k % len(starts)], starts[(k + 3) % len(starts)])):
            s0, t = (N - n if st == "last" else st), clock()
            case(f"block of {n} at {st}", s0, [(t, gval(t, i)) for i in range(n)], "replaced", where=st)
    n, s0 = SIZES[-1], 65
    t = clock()
    state = [(t, gval(t, i)) for i in range(n)]
    case("the state of the stale batches", s0, state, "replaced", where=65)
    for at in WINNER_AT + (n - 1,):
        ents = [(t - 1, b"stale" + gval(t, i)) for i in range(n)]
        ents[at] = state[at] = (clock(), b"winner at %d, a long value" % at)
        case(f"one winner at {at}", s0, ents, "one", winner=at)
    case("loses everywhere", s0, [(t - 1, b"\xff" * 12) for _ in range(n)], "kept", loses=True)
    case("equal to the state", s0, list(state), "kept", equal=True)
    return out


# ---- f. routed and owned --------------------------------------------------------------------
def routed_keys(pairs, owner_of, S=2):
    """per pair one key of every owner shard: keys[i][d] belongs to shard d"""
    keys = []
    for i in range(len(pairs)):
        row, j = [], 0
        for d in range(S):
            while owner_of(b"r%d-%d" % (i, j)) != d:
                j += 1
            row.append(b"r%d-%d" % (i, j))
            j += 1
        keys.append(row)
    return keys
