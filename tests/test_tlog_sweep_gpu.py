"""TLOG merge: sweeps built around k_tlog.hip's own constants (64-key tiles and
64-item passes, the 4-entry fast path and short-segment shortcut, 4-record
search windows aligned to the pool index, 3 interpolation rounds, 2048-entry
compaction tiles with 1024 logs staged in LDS), each case carrying the outcome
it was built to reach.

After EVERY converge: state == oracle, check_layout / check_entries over
Engine.tlog_layout, and the skipped count.  Separately (the coverage guard),
tlog_layout.classify names what each key's merge did from the layout before
and after, and the case's expected outcome must match: a literal in the
case where the case was built for one outcome, tlog_layout.expected_outcome
(the merge's stated rules over the segment's front room and capacity read
from the layout) for the search sweep's thousands of probes.

The case generators are plain python (test_tlog_sweep_cpu.py checks them
against the oracle alone).  A case: key, steps (deltas that build its state),
probe (the delta under test), decl = (interleaving, newer, duplicate,
below-cutoff) entry counts of the probe, expect, path (skip / fast / slow: what
the case aims at inside the kernel, not observable), malformed."""
import collections

import numpy as np
import pytest

from helpers import assert_state_equal
from test_parity_tlog import _canon, _log_batch
from tlog_layout import (check_entries, check_layout, classify, expected_outcome, merge_model, row)

pytestmark = pytest.mark.gpu

P = b"prefix!!"  # 8 bytes: longer values sharing it differ only in the arena
BIG = (1 << 64) - 1
PAIR = (P + b"tail-a", P + b"tail-b")  # differ only after byte 8


def fresh_cap(n):
    """capacity a fresh log of n entries is given (a power of two >= 4 n + 4,
    an eighth of its free room kept in front): the CPU check's stand-in for a
    layout read, and a size guide for the generators"""
    c = 4
    while c < 4 * n + 4:
        c *= 2
    return c - (c - n) // 8


def _val(i):
    """state values: long ones sharing P (9..20 bytes), short ones, the empty one"""
    if i % 5 == 0:
        return P + b"m" + (b"%d" % i) + b"x" * (i % 9)
    if i % 5 == 3:
        return b""
    return b"s%d" % i


def _below(v):
    return v[:-1]  # a proper prefix sorts below; of a long value it still shares P


def _above(v):
    return v + b"\x01"


def case(key, steps, probe, decl, expect=None, path="slow", malformed=False, tag=()):
    return dict(key=key, steps=steps, probe=probe, decl=decl, expect=expect, path=path, malformed=malformed, tag=tag)


def resolve(step, log, cap):
    """a step is (cutoff, [(value, ts)]) or ("fill", k): newer entries up to len == cap - k"""
    if step[0] != "fill":
        return step
    top = log[-1][0]
    return 0, [(b"f%d" % i, top + 1 + i) for i in range(cap - step[1] - len(log))]


# ---- a. search sweep ---------------------------------------------------------
SEARCH_L = (1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 16, 17, 31, 32, 33, 63, 64, 65, 200)
SEARCH_GROUPS = ((1, 2, 3, 4, 5), (7, 8, 9), (12, 13), (16, 17), (31, 32, 33), (63, 64, 65), (200,))
SHAPES = ("even", "old_far", "new_far", "end_max", "zero_old")
FLAVOURS = ("between", "tie_below", "tie_above", "dup", "triple0", "triple1", "triple2", "triple3")


def _predrop(L):
    """extra oldest entries, dropped by a cutoff raise before the probe, move a
    log's base up by as many: _predrop(L)[r] of them put a fresh log of L live
    entries at base mod 4 == r (fresh segments start at multiples of 8, behind
    an eighth of their free room)"""
    out = {}
    for d in range(24):
        n, c = L + d, 4
        while c < 4 * n + 4:
            c *= 2
        out.setdefault(((c - n) // 8 + d) % 4, d)
    return [out[r] for r in range(4)]


def shape_ts(shape, L):
    if shape == "even":
        return [1000 + 10 * i for i in range(L)]
    if shape == "old_far":  # L - 1 entries within [10^6, 10^6 + 2 L), the oldest at 1
        return [1] + [10**6 + 2 * i for i in range(L - 1)]
    if shape == "new_far":  # ... the newest at 2^40
        return [10**6 + 2 * i for i in range(L - 1)] + [1 << 40]
    if shape == "end_max":
        return [BIG - 3 * (L - 1 - i) for i in range(L)]
    return [10 * i for i in range(L)]  # zero_old


def probes(L):
    if L <= 17:
        return list(range(L + 1))
    return sorted({*range(5), L // 2 - 1, L // 2, L // 2 + 1, *range(L - 5, L + 1)})


def search_cases(Ls):
    out = []
    for L in Ls:
        for si, shape in enumerate(SHAPES):
            # the pre-dropped prefix needs timestamps below the shape's oldest
            droppable = L <= 17 and shape_ts(shape, L)[0] >= 100
            for p in probes(L):
                for fl in FLAVOURS:
                    for r in (range(4) if droppable and shape == "even" else [(p + si) % 4]):
                        d = _predrop(L)[r] if droppable else 0
                        ts = shape_ts(shape, L)
                        vals = [_val(i) for i in range(L)]
                        if fl.startswith("triple"):
                            if L < 3 or p > L - 3:
                                continue
                            ts[p + 1] = ts[p + 2] = ts[p]
                            vals[p:p + 3] = [P + b"-b", P + b"-d", b"t2"]  # ascending
                            place = int(fl[-1])
                            ent, rank = ((P + b"-a", P + b"-c", b"q", b"t3")[place], ts[p]), p + place
                        elif fl == "between":
                            if p == 0:
                                if ts[0] == 0:
                                    continue
                                ent = (b"new", ts[0] - 1)
                            elif p == L:
                                if ts[-1] == BIG:
                                    continue
                                ent = (b"new", ts[-1] + 1)
                            else:
                                ent = (PAIR[p % 2], ts[p - 1] + 1)
                            rank = p
                        elif fl == "tie_below":
                            if p == L:
                                continue
                            vals[p] = vals[p] or P + b"not-empty"  # nothing sorts below the empty value
                            ent, rank = (_below(vals[p]), ts[p]), p
                        elif fl == "tie_above":
                            if p == 0:
                                continue
                            ent, rank = (_above(vals[p - 1]), ts[p - 1]), p
                        else:  # dup
                            if p == L:
                                continue
                            ent, rank = (vals[p], ts[p]), p
                        log = list(zip(vals, ts))
                        steps = [(0, [(b"d%d" % i, 10 + 2 * i) for i in range(d)] + log)]
                        if d:
                            steps.append((60, []))  # pre-dropped timestamps < 60 <= the shape's oldest - 1
                        if fl == "dup":
                            decl, path = (0, 0, 1, 0), "slow"
                        elif rank == L:
                            decl, path = (0, 1, 0, 0), ("fast" if ent[1] > max(ts) else "slow")
                        else:
                            decl, path = (1, 0, 0, 0), "slow"
                        out.append(case(f"a/{L}/{shape}/{p}/{fl}/{r}", steps, (0, [ent]), decl, None, path,
                                        tag=(L, fl, rank)))
    return out


# ---- c. fast-path edges ------------------------------------------------------
BASE3 = [(b"s1", 100), (P + b"long-one", 200), (b"", 300)]


def fast_cases():
    out = []
    st = [(50, BASE3)]
    new = lambda n, t0=400: [(b"n%d" % i, t0 + i) for i in range(n)]  # noqa: E731
    for n in range(6):  # 5 entries: the first size that is not fast
        out.append(case(f"c/size{n}", st, (0, new(n)), (0, n, 0, 0), "append" if n else "unchanged",
                        "fast" if n <= 4 else "slow"))
    for m in (1, 4, 6):  # room: len + M == cap fits, cap + 1 is rebuilt
        out.append(case(f"c/fits{m}", st + [("fill", m)], (0, new(m, 10**6)), (0, m, 0, 0), "append",
                        "fast" if m <= 4 else "slow"))
        out.append(case(f"c/over{m}", st + [("fill", m - 1)], (0, new(m, 10**6)), (0, m, 0, 0), "rebuild"))
    out.append(case("c/cut_below", st, (10, new(1)), (0, 1, 0, 0), "append", "fast"))
    out.append(case("c/cut_equal", st, (50, new(2)), (0, 2, 0, 0), "append", "fast"))
    # a raised cutoff on an emptied log needs no drop search, but the fast path takes only
    # cd <= cut: the key is walked as a slow one and appended (labelled slow, not fast)
    out.append(case("c/cut_above_empty", st + [(1000, [])], (2000, new(1, 3000)), (0, 1, 0, 0), "append"))
    out.append(case("c/cut_above_empty_only", st + [(1000, [])], (2000, []), (0, 0, 0, 0), "unchanged"))
    out.append(case("c/cut_above_live", st, (150, new(1)), (0, 1, 0, 0), "append"))
    out.append(case("c/cut_above_live_only", st, (250, []), (0, 0, 0, 0), "append"))  # a pure drop: base moves up
    out.append(case("c/kept_prefix", st, (0, [(b"k", 400), (b"o1", 40), (b"o0", 30)]), (0, 1, 0, 2), "append", "fast"))
    out.append(case("c/tie_newest_above", st, (0, [(b"a", 300)]), (0, 1, 0, 0), "append"))
    out.append(case("c/tie_newest_below", [(50, BASE3[:2] + [(b"z", 300)])], (0, [(b"a", 300)]), (1, 0, 0, 0),
                    "insert_up"))
    out.append(case("c/same_ts_ordered", st, (0, [(PAIR[1], 500), (PAIR[0], 500)]), (0, 2, 0, 0), "append"))
    out.append(case("c/same_ts_misordered", st, (0, [(PAIR[0], 500), (PAIR[1], 500)]), (0, 0, 0, 0), "unchanged",
                    "skip", malformed=True))
    out.append(case("c/fresh4", [], (0, new(4)), (0, 4, 0, 0), "rebuild"))
    out.append(case("c/only_dups", st, (0, list(BASE3)), (0, 0, 3, 0), "unchanged"))
    return out


# ---- d. move sweep -----------------------------------------------------------
MOVED = (1, 63, 64, 65, 128, 129)
DELTA_N = (1, 4, 5, 9)
PRE = 6  # entries an earlier cutoff raise dropped: front room


def _long_log(L):
    return [(_val(i), 1000 + 10 * i) for i in range(L)]


def _between(i, k=0):
    """an entry ranked i in _long_log (strictly between entries i - 1 and i)"""
    return (PAIR[k % 2] + b"%d" % k, 1000 + 10 * i - 5 + k % 4)


def _mix(L, ranks, n, drop_to=None):
    """a delta of n entries over _long_log(L) cut at PRE: kept interleaving ones
    at `ranks`, the rest newer / duplicates / below the cutoff, round robin"""
    ents = [_between(r, k) for k, r in enumerate(ranks)]
    kinds = collections.Counter(inter=len(ents))
    k = 0
    while len(ents) < n:
        kind = ("newer", "dup", "below")[k % 3]
        if kind == "newer":
            ents.append((b"w%d" % k, 10**6 + k))
        elif kind == "dup":
            ents.append(_long_log(L)[L - 1 - k])  # near the newest end: no rank below the moved side
        else:
            ents.append((b"b%d" % k, 1000 + k))  # < the cutoff 1000 + 10 PRE
        kinds[kind] += 1
        k += 1
    return ents, (kinds["inter"], kinds["newer"], kinds["dup"], kinds["below"])


def move_cases():
    out = []
    i = 0
    for moved in MOVED:
        for n in DELTA_N:
            for direction in ("insert_up", "insert_down"):
                ni = {1: 1, 4: 1, 5: 2, 9: 3}[n]
                # one interleaving entry moves the shorter side: at most half of the log
                fits = [L for L in (70, 130, 200) if L - PRE > (2 * moved if ni == 1 else moved + 1)]
                if not fits:
                    continue
                L = fits[i % len(fits)]
                i += 1
                if direction == "insert_up":  # the suffix from the smallest rank: len - minrank entries
                    lo = L - moved
                    ranks = [lo] + [max(lo, L - 1 - j) for j in range(ni - 1)]
                else:  # the prefix below the largest rank: mx - drop entries
                    hi = PRE + moved
                    ranks = [hi] + [min(hi, PRE + 1 + j) for j in range(ni - 1)]
                ents, decl = _mix(L, ranks, n)
                steps = [(0, _long_log(L)), (1000 + 10 * PRE, [])]
                out.append(case(f"d/{direction}/{moved}/{n}/{L}", steps, (0, ents), decl, direction,
                                tag=(direction, moved, n)))
    L, half = 70, (70 + PRE) // 2  # dn == up goes up: rank - PRE == L - rank
    out.append(case("d/tie_goes_up", [(0, _long_log(L)), (1000 + 10 * PRE, [])], (0, [_between(half)]),
                    (1, 0, 0, 0), "insert_up", tag=("insert_up", L - half, 1)))
    # a 1-entry log has no front room: the older entry cannot go down
    out.append(case("d/no_front_forces_up", [(0, [(b"only", 500)])], (0, [(b"older", 400)]), (1, 0, 0, 0),
                    "insert_up", tag=("insert_up", 1, 1)))
    # one free entry at the tail, two kept: up does not fit, down does -- it moves L - 2 - PRE entries, up would move 1
    # (the probe ties with the newest filled entry, its value below it: rank len - 1)
    full = [(0, _long_log(70)), (1000 + 10 * PRE, []), ("fill", 1)]
    tie_top = lambda log: (0, [(b"top", 10**7), (b"e", log[-1][0])])  # noqa: E731
    out.append(case("d/full_forces_down", full, tie_top, (1, 1, 0, 0), "insert_down", tag=("forced_down", 0, 2)))
    out.append(case("d/neither_fits", full[:2] + [("fill", 0)], tie_top, (1, 1, 0, 0), "rebuild",
                    tag=("rebuild", 0, 2)))
    # rebuilds: a raised cutoff with an overflowing delta; item counts (survivors
    # + delta entries) across 64 and 128; neighbours in one tile whose items
    # straddle the 64-item passes
    out.append(case("d/rebuild_drop", [(0, BASE3)], (150, [(b"r%d" % j, 400 + j) for j in range(14)]), (0, 14, 0, 0),
                    "rebuild", tag=("rebuild", 16, 14)))
    for n in (40, 40, 40, 63, 64, 65, 127, 128, 129):
        out.append(case(f"d/rebuild_fresh/{n}/{len(out)}", [], (0, [(_val(j), 7 + 3 * j) for j in range(n)]),
                        (0, n, 0, 0), "rebuild", tag=("rebuild", n, n)))
    for n in (100, 200):  # a 20-entry log interleaved by a delta it has no room for: 120 and 220 items
        ents = [(b"i%d" % j, 150 + 7 * j) for j in range(n)]
        out.append(case(f"d/rebuild_merge/{n}", [(0, [(b"s%d" % j, 100 + 100 * j) for j in range(20)])], (0, ents),
                        (n, 0, 0, 0), "rebuild", tag=("rebuild", 20 + n, n)))
    return out


# ---- b. tile geometry --------------------------------------------------------
TILE_ND = (1, 63, 64, 65, 128, 129, 200)
TILE_F = (0, 1, 63, 64, 65, 128, 129, 191)
SLOW_STATE = [(b"s%d" % j, 100 + 100 * j) for j in range(4)]  # cut 50: timestamps 100 .. 400


def _slow_delta(n, salt):
    """n entries for a key holding SLOW_STATE: kept newer ones, duplicates and
    entries below the cutoff all within its first 9, the rest below the cutoff"""
    if n == 1:
        return [SLOW_STATE[2]], (0, 0, 1, 0)
    newer = [(b"w%d.%d" % (salt, j), 1000 + j) for j in range(min(3, n))]
    dup = SLOW_STATE[1:1 + max(0, min(3, n - 3))]
    below = [(b"b%04d" % j, 40 - j % 40) for j in range(max(0, n - 6))]
    return newer + dup + below, (0, len(newer), len(dup), len(below))


TILE_TABLE = ((1, 0), (1, 1), (63, 63), (64, 0), (64, 64), (65, 1), (65, 65), (128, 63), (128, 128), (129, 129),
              (200, 64), (200, 191))
assert {nd for nd, _ in TILE_TABLE} == set(TILE_ND) and {F for _, F in TILE_TABLE} == set(TILE_F)


def tile_batches():
    """one batch (cases probed together, in this order) per (nd, F) of
    TILE_TABLE: slow keys at tile lanes 0 and 63 (F slow entries between them)
    and at lane 0 of the next tile, fast keys elsewhere.  With F > 64 lane 63's
    entries come in pass 1 and later"""
    out = []
    for nd, F in TILE_TABLE:
        batch = []
        n63 = F // 2 if nd >= 64 else 0
        n0 = F - n63
        for lane in range(nd):
            key = f"b/{nd}/{F}/{lane}"
            slow = {0: n0, 63: n63, 64: 5}.get(lane, 0)
            if slow:
                ents, decl = _slow_delta(slow, lane)
                batch.append(case(key, [(50, SLOW_STATE)], (0, ents), decl, "append" if decl[1] else "unchanged"))
            else:
                batch.append(case(key, [(50, SLOW_STATE[:1])], (0, [(b"f", 1000 + lane)]), (0, 1, 0, 0), "append",
                                  "fast"))
        out.append(batch)
    return out


QUEUE = (0, 1, 63, 64, 65, 130)
QLOG = [(b"q%d" % j, 100 + 10 * j) for j in range(140)]


def queue_tiles():
    """64-key tiles, one batch: Q queued entry searches (duplicates of a
    140-entry log, all from lane 0's key) with no drop search, then with R keys
    raising their cutoff into a 2-entry log (a drop search each):
    R + Q == 64 fills the queue exactly, R == 64 with Q > 0 flushes the drop
    searches first, Q == 65 / 130 take two and three search passes"""
    out = []
    for R in (0, 63, 64):
        for Q in QUEUE:
            tile = []
            for lane in range(64):
                key = f"q/{R}/{Q}/{lane}"
                raises = lane >= 64 - R
                if lane == 0 and Q:
                    cut = 105 if raises else 0  # drops the oldest entry; the duplicates start above it
                    ents = QLOG[1:1 + Q]
                    tile.append(case(key, [(0, QLOG)], (cut, ents), (0, 0, Q, 0), "append" if raises else "unchanged"))
                elif raises:
                    tile.append(case(key, [(0, [(b"a", 10), (b"b", 20)])], (15, []), (0, 0, 0, 0), "append"))
                else:
                    tile.append(case(key, [(0, [(b"a", 10)])], (0, [(b"n", 30)]), (0, 1, 0, 0), "append", "fast"))
            out.append(tile)
    return out


# ---- the runner --------------------------------------------------------------
class Sweep:
    def __init__(self, O, eng):
        from jylis_amd.repo import RepoTLOG
        self.O, self.eng = O, eng
        self.want, self.got = O.Repo(O.TLOG), RepoTLOG(eng)
        self.model = {}  # key -> ([(ts, value)] ascending, cutoff)
        self.rows = {}
        self.skipped = 0
        self.seen = collections.Counter()

    def converge(self, logs, malformed=()):
        """logs: [(key, cutoff, entries newest first)] -> the unconditional checks"""
        good = [l for l in logs if l[0] not in malformed]
        if good:
            self.want.converge(_log_batch(good))
        self.got.converge_deltas(_log_batch(logs))
        self.skipped += len(malformed)
        self.check()

    def check(self):
        state = self.got.state()
        assert_state_equal(self.O.TLOG, self.want.state(), state)
        slots = self.got._sorted_slots()
        self.layout = self.eng.tlog_layout(slots)
        check_layout(self.layout)
        check_entries(self.layout, state)
        assert self.eng.skipped() == self.skipped
        names = [self.got.names[int(s)].decode() for s in slots]
        self.rows = {k: row(self.layout, i) for i, k in enumerate(names)}

    def run(self, cases, batches=None):
        """build the cases' states step by step (one converge per step for all
        of them), then probe them (all in one converge, or one per batch of
        `batches`); -> {key: (before, after, stats)}, the coverage guard asserted"""
        for c in cases:
            self.model.setdefault(c["key"], ([], 0))
        for i in range(max(len(c["steps"]) for c in cases)):
            logs = []
            for c in cases:
                if i < len(c["steps"]):
                    log, cut = self.model[c["key"]]
                    dcut, ents = resolve(c["steps"][i], log, self.rows.get(c["key"], (0, 0, 0, 0))[3])
                    self.model[c["key"]] = merge_model(log, cut, dcut, ents)[:2]
                    logs.append((c["key"], dcut, _canon(ents)))
            self.converge(logs)
        res = {}
        for batch in batches or [cases]:
            res.update(self.probe(batch))
        return res

    def probe(self, cases):
        before = dict(self.rows)
        logs, stats = [], {}
        for c in cases:
            log, cut = self.model[c["key"]]
            dcut, ents = c["probe"](log) if callable(c["probe"]) else c["probe"]
            if c["malformed"]:
                logs.append((c["key"], dcut, list(ents)))  # as given: the order is the point
                continue
            nlog, ncut, st = merge_model(log, cut, dcut, ents)
            assert (st["inter"], st["newer"], st["dup"], st["below"]) == tuple(c["decl"]), (c["key"], st)
            self.model[c["key"]] = (nlog, ncut)
            stats[c["key"]] = st
            logs.append((c["key"], dcut, _canon(ents)))
        # no key twice: the host path then hands the batch to the merge as ONE round in the order
        # given (it splits repeated keys into rounds), so case i is delta key i -- lane i % 64 of
        # key tile i // 64, which the tile, queue and rebuild cases are placed by
        assert len({l[0] for l in logs}) == len(logs)
        self.converge(logs, malformed={c["key"] for c in cases if c["malformed"]})
        res, wrong = {}, []
        for c in cases:
            k = c["key"]
            b = before.get(k, (0, 0, 0, 0))
            st = stats.get(k)
            got = classify(b, self.rows[k], st["drop"] if st else 0, st["inter"] if st else 0, bool(st and st["inter"]))
            rule = expected_outcome(b, st) if st else "unchanged"
            if c["expect"] and c["expect"] != rule:
                wrong.append((k, "the case table says", c["expect"], "the rules say", rule, b, st))
            if got != (c["expect"] or rule):
                wrong.append((k, "aimed at", c["expect"] or rule, "took", got, b, self.rows[k], st))
            self.seen[(c["path"], got)] += 1
            res[k] = (b, self.rows[k], st)
        assert not wrong, (len(wrong), wrong[:8])
        return res


# ---- the tests ---------------------------------------------------------------
@pytest.mark.parametrize("Ls", SEARCH_GROUPS, ids=lambda g: "L" + "-".join(map(str, g)))
def test_search_sweep(oracle_mod, engine, Ls):
    """a: one key per (log length, timestamp shape, probe rank, flavour); a
    duplicate leaves state AND layout unchanged; for L <= 17 every flavour is
    probed at every residue of base mod 4 (ts_interp's windows are aligned to
    the pool index)"""
    sw = Sweep(oracle_mod, engine)
    cases = search_cases(Ls)
    res = sw.run(cases)
    residues = collections.defaultdict(set)
    for c in cases:
        L, fl, _ = c["tag"]
        before, after, _ = res[c["key"]]
        residues[(L, fl)].add(before[0] % 4)
        if fl == "dup":
            assert before == after, c["key"]
    short = {k: sorted(v) for k, v in sorted(residues.items()) if k[0] <= 17 and len(v) < 4}
    assert not short, f"base mod 4 residues probed per (L, flavour), incomplete ones: {short}"
    assert {o for _, o in sw.seen} == {"unchanged", "append", "insert_up", "insert_down"}, sw.seen


def test_fast_path_edges(oracle_mod, engine):
    """c: delta sizes 0..5, room exactly / one short (cap read from the layout),
    delta cutoff below / equal / above on an empty and a live log, a kept
    prefix, a tie with the newest, equal timestamps in and out of value order,
    a fresh key, duplicates only"""
    sw = Sweep(oracle_mod, engine)
    cases = fast_cases()
    res = sw.run(cases)
    for m in (1, 4, 6):
        b, a, _ = res[f"c/fits{m}"]
        assert b[2] + m == b[3] and a[2] == a[3], (b, a)  # len + M == cap: fits, now full
        b, _, _ = res[f"c/over{m}"]
        assert b[2] + m == b[3] + 1, b
    assert sw.skipped == 1
    assert {o for _, o in sw.seen} == {"unchanged", "append", "insert_up", "rebuild"}


def test_move_sweep(oracle_mod, engine):
    """d: in-place inserts moving 1 / 63 / 64 / 65 / 128 / 129 entries up and
    down with deltas of 1 / 4 / 5 / 9 entries (4 | 5: short-segment shortcut |
    bisect), the choice between the directions, and rebuilds through
    k_tlog_commit"""
    sw = Sweep(oracle_mod, engine)
    cases = move_cases()
    res = sw.run(cases)
    reached = collections.defaultdict(set)
    for c in cases:
        direction, moved, n = c["tag"]
        b, _, st = res[c["key"]]
        if direction == "insert_up":
            assert b[2] - st["minrank"] == moved, (c["key"], b, st)
        elif direction == "insert_down":
            assert st["mx"] - st["drop"] == moved, (c["key"], b, st)
        elif direction == "forced_down":
            assert st["mx"] - st["drop"] > b[2] - st["minrank"], (c["key"], b, st)  # down moves more
        reached[direction].add((moved, n))
    for direction in ("insert_up", "insert_down"):
        assert {m for m, _ in reached[direction]} >= set(MOVED), reached[direction]
        assert {n for _, n in reached[direction]} >= set(DELTA_N), reached[direction]
        for m in (63, 64, 65):
            assert {(m, 4), (m, 5)} <= reached[direction], (direction, m)
    assert {o for _, o in sw.seen} == {"insert_up", "insert_down", "rebuild"}, sw.seen
    # the three 40-item rebuilds straddle the commit's 64-item passes only as neighbours in one key tile
    at = [i for i, c in enumerate(cases) if c["key"].startswith("d/rebuild_fresh/40/")]
    assert len(at) == 3 and at[2] == at[0] + 2 and at[0] // 64 == at[2] // 64, at


def test_tile_geometry(oracle_mod, engine):
    """b: batch sizes around the 64-key tile with slow keys at lanes 0, 63 and
    the next tile's lane 0, slow entries per tile around one and two 64-entry
    passes (kept, below-cutoff and duplicate entries in pass 0 and later), and
    search queues of 0 .. 130 items with and without drop searches"""
    sw = Sweep(oracle_mod, engine)
    batches = tile_batches()
    batches.append([c for t in queue_tiles() for c in t])
    cases = [c for b in batches for c in b]
    sw.run(cases, batches)
    assert set(sw.seen) == {("fast", "append"), ("slow", "append"), ("slow", "unchanged")}, sw.seen
    # the geometry aimed at holds only if key i of a probe batch is lane i % 64 of tile i // 64:
    # the keys were interned in this order, so their slots ascend along every batch (Sweep.probe
    # checks that a batch reaches the merge as one round, in the order given)
    from jylis_amd._lib import TLOG
    for batch in batches:
        slots = engine.lookup(TLOG, [c["key"] for c in batch]).astype(np.int64)
        assert (np.diff(slots) > 0).all()
    assert len(batches[-1]) % 64 == 0 and all(c["key"].endswith(f"/{i % 64}") for i, c in enumerate(batches[-1]))


def test_repeated_slots_in_a_device_batch(oracle_mod, engine):
    """b, k_tlog_prep: a slot named twice or three times in ONE merge (only a
    device batch can: a host batch is split into rounds before the merge),
    copies in one tile and in different tiles, beside a routed-run hole
    (JY_NO_SLOT): each repeated key is left untouched and counted once, the hole
    is not counted, every other key merges"""
    import torch
    from jylis_amd._lib import JY_NO_SLOT, TLOG
    sw = Sweep(oracle_mod, engine)
    keys = [f"r/{i}" for i in range(140)]
    sw.converge([(k, 0, [(b"s", 10)]) for k in keys])
    slots = engine.intern(TLOG, keys).astype(np.int64)
    nd = 140
    slot = slots.copy()
    slot[5] = slots[3]                  # two copies in one tile
    slot[20] = slot[21] = slots[19]     # three copies in one tile
    slot[100] = slots[40]               # two copies in different tiles
    slot[130] = slot[70] = slots[10]    # three copies over three tiles
    slot[4] = slot[101] = JY_NO_SLOT    # holes beside them
    repeated = {int(slots[i]) for i in (3, 19, 40, 10)}
    pre, lr = engine.pack_values(TLOG, [b"n%d" % i for i in range(nd)])
    dev = lambda a, t: torch.from_numpy(np.ascontiguousarray(a).view(t)).to("cuda:0")  # noqa: E731
    engine.tlog_converge(dev(slot.astype(np.uint32), np.int32), dev(np.zeros(nd, np.uint64), np.int64),
                         dev(np.arange(nd + 1, dtype=np.uint64), np.int64),
                         dev(np.arange(nd, dtype=np.uint64) + 100, np.int64), dev(pre, np.int64), dev(lr, np.int64))
    merged = [(keys[i], 0, [(b"n%d" % i, 100 + i)]) for i in range(nd)
              if int(slot[i]) == int(slots[i]) and int(slot[i]) not in repeated]
    assert len(merged) == nd - 2 - 4 - 6
    sw.want.converge(_log_batch(merged))
    sw.skipped += 4
    sw.check()


def _small_engine():
    from jylis_amd.engine import Engine
    return Engine(device=0, entry_capacity=1024)


def test_rebuilds_that_spill(oracle_mod):
    """d: on a 1024-entry pool one merge's rebuilt logs do not fit: they spill,
    the pool is compacted and the re-merge gives the exact join"""
    eng = _small_engine()
    try:
        sw = Sweep(oracle_mod, eng)
        sw.converge([(f"s/{i}", 0, _canon([(_val(j), 10 + j) for j in range(5)])) for i in range(10)])
        st = eng.tlog_stats()
        assert st["spills"] == 0 and st["compactions"] == 0, st
        assert sw.layout["used"] == 10 * 32
        # 30 fresh 5-entry logs (32 pool entries each) and 10 grown past their room: 1280 + more > 1024 - 320
        logs = [(f"s/{i}", 0, _canon([(b"g%d" % j, 100 + j) for j in range(40)])) for i in range(10)]
        logs += [(f"s/{i}", 0, _canon([(_val(j), 10 + j) for j in range(5)])) for i in range(10, 40)]
        sw.converge(logs)
        st = eng.tlog_stats()
        assert st["spills"] == 1 and st["compactions"] == 1 and st["merges"] == 3, st
    finally:
        eng.close()


def cmp_front(n):
    return n // 8 + 2 if n else 0


def _big_log(n, t0, step):
    """n entries t0, t0 + step, ...: mostly short values (a state read fetches every long one)"""
    return [(_val(j) if j % 50 == 0 else b"s%d" % j, t0 + step * j) for j in range(n)]


def test_compaction_sweep(oracle_mod):
    """e: a compaction over two logs of 5000 and 4500 live entries -- the first
    fills output tile 0 from its front room on, all of tile 1 and part of tile
    2 (2048 entries each), the second starts and ends inside tiles -- a run
    of 1150 empty logs between two live ones inside one output tile (more than
    the 1024 logs a tile stages in LDS), tiles of 1-entry logs (staged in LDS)
    and logs whose capacity exceeds twice their length; afterwards every
    compacted log sits behind cmp_front(len) free entries, and an append, an
    up-insert and a down-insert into every long log still match"""
    eng = _small_engine()
    try:
        sw = Sweep(oracle_mod, eng)
        longs = {"e/0long": _big_log(5000, 1000, 10), "e/0long2": _big_log(4500, 1000, 10)}
        sw.converge([("e/0long", 0, _canon(longs["e/0long"]))])  # spills on the 1024-entry pool
        assert eng.tlog_stats()["compactions"] == 1
        logs = [("e/0long2", 0, _canon(longs["e/0long2"])), ("e/1a", 0, [(b"a", 5)])]
        logs += [(f"e/2empty{i:04d}", 7 + i, []) for i in range(1100)]  # a cutoff, no entries
        logs += [(f"e/2gone{i:04d}", 0, [(b"x", 3)]) for i in range(50)]
        logs += [("e/3b", 0, [(b"b", 5)])]
        logs += [(f"e/4one{i:04d}", 0, [(_val(i), 50 + i)]) for i in range(400)]  # cap 8 > 2 len
        sw.converge(logs)
        sw.converge([(f"e/2gone{i:04d}", 100, []) for i in range(50)])  # emptied by a cutoff
        assert eng.tlog_stats()["compactions"] == 1
        for k, log in longs.items():  # what the compaction's copy tiles will see
            assert sw.rows[k][2] == len(log) > 2 * 2048
        free = sw.layout["pcap"] - sw.layout["used"]
        longs["e/5big"] = [(b"B%d" % j, 10 + 2 * j) for j in range(17000)]
        assert fresh_cap(17000) > free, (free, "the trigger no longer overflows the pool")
        # this merge's rebuild does not fit: it spills, the pool is compacted, the spill re-merged
        b = _log_batch([("e/5big", 0, _canon(longs["e/5big"]))])
        sw.want.converge(b)
        sw.got.converge_deltas(b)
        # the fronts first, straight from the layout, so that a wrong front room is named as such
        slots = sw.got._sorted_slots()
        lay = eng.tlog_layout(slots)
        bad = [(sw.got.names[int(s)], int(f), int(n)) for s, f, n in zip(slots, lay["front"], lay["len"])
               if sw.got.names[int(s)] != b"e/5big" and int(f) != cmp_front(int(n))]  # e/5big: rebuilt afterwards
        assert not bad, f"(key, front, len) with front != cmp_front(len) after the compaction: {bad[:8]}"
        sw.check()
        st = eng.tlog_stats()
        assert st["compactions"] == 2 and st["spills"] == 2, st
        for k in ("e/0long", "e/0long2"):
            assert sw.rows[k][3] >= 2 * len(longs[k])
        # one more batch of appends, then an up-insert and a down-insert per long log
        sw.converge([(k, 0, [(b"app", 10**9)]) for k in longs])
        for k, log in longs.items():
            for name, at in (("insert_up", len(log) - 3), ("insert_down", 3)):
                before = dict(sw.rows)
                sw.converge([(k, 0, [(_above(log[at - 1][0]), log[at - 1][1])])])  # a tie: ranked `at`
                assert classify(before[k], sw.rows[k], 0, 1, True) == name, (k, name, before[k], sw.rows[k])
    finally:
        eng.close()
