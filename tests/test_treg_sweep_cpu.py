"""The TREG sweeps' generators, without a GPU: every generator of treg_cases.py
runs against the oracle alone -- the outcome each case declares is what an
O.Repo(O.TREG) shows after the case's launches, Python's bytes order agrees
with the oracle on every value pair, timestamps at and above 2^63 are
unsigned there, the declared duplicate counts follow from the slot arrays --
and a tiling model of this file's own (which bitmap words, rows, waves and
workgroups an entry index lands on) agrees with the tags the generators
attach.  The geometry the generators assume is the one the library was built
with (jy_treg_claim_info of no engine)."""
import numpy as np
import pytest

import treg_cases as C

N_CLAIM, WORDS_CLAIM = 40000, 1250  # the claim sweep's file, as test_treg_sweep_gpu.py builds it
N_DENSE = 2200


def test_geometry_is_the_builds():
    from jylis_amd.engine import treg_build_info
    assert treg_build_info() == {"unroll": C.UNROLL, "routed_unroll": C.ROUTED_UNROLL, "fold_rounds": C.FOLD_ROUNDS,
                                 "tile": C.TILE}
    assert C.TILE == C.THREADS * C.UNROLL and C.WAVE == C.LANES * C.UNROLL
    assert C.FOLD_TILE == C.THREADS * 2 and C.TAIL_CHUNK == C.LANES
    assert tuple(m - (C.FOLD_ROUNDS + 1) for m in C.FOLD_M if m > C.FOLD_ROUNDS) == C.TAIL_RECORDS


_table = C.table


def _dups(L):
    s = [int(x) for x in L["slots"] if x != C.NO_SLOT]
    return len(s) - len(set(s))


def _check(O, cases, n, sets=False):
    """the cases in order on one oracle repo and one Model: after each, the declared outcome is the oracle's"""
    want, model = O.Repo(O.TREG, 9), C.Model(n)
    for c in cases:
        before = {}
        for L in c["launches"]:
            assert L["dups"] == (_dups(L) if L["kind"] != "block" else 0), c["name"]
            assert L["skips"] == 0
            named = {int(s) for s in L["slots"] if s != C.NO_SLOT}
            assert max(named) < n
            for s in named:
                before.setdefault(s, (model.ts[s], model.val[s]))
            if L["kind"] == "set" and sets:
                for s, t, v in zip(L["slots"], L["ts"], L["vals"]):
                    want.treg_set(C.key_of(int(s)), v, t)
            else:
                want.converge(_table(L))
            hit = model.apply(L)
        last = c["launches"][-1]
        named = {int(s) for s in last["slots"] if s != C.NO_SLOT}
        exp = c["expect"] if c["expect"] is not None else {s: (model.ts[s], model.val[s]) for s in named}
        for s, e in exp.items():
            assert want.treg_get(C.key_of(s)) == (e[1], e[0]) and (model.ts[s], model.val[s]) == e, (c["name"], s)
        out = c["outcome"]
        if out == "one":
            assert hit == {last["slot0"] + c["tags"]["winner"]}, c["name"]
        elif out in ("replaced", "kept"):
            assert hit == (named if out == "replaced" else set()), c["name"]
        else:  # per slot, against the state before the case's last launch
            for s, o in out.items():
                assert (s in hit) == (o == "replaced"), (c["name"], s)
        assert not (c["same_lr"] & hit)
    return want, model


def test_order_matrix(oracle_mod):
    """a. (and e., g.): every pair alone against the oracle, Python's order against the oracle's"""
    O, pairs = oracle_mod, C.order_pairs()
    for p in pairs:
        r = O.Repo(O.TREG)
        for t, v in (p["state"], p["delta"]):
            r.converge(_table(C.launch("keyed", [0], [t], [v])))
        assert r.treg_get(C.key_of(0)) == (p["expect"][1], p["expect"][0]), p["name"]
        assert p["replaced"] == (p["delta"] > p["state"]), p["name"]  # Python's (int, bytes) order
        assert not (p["same_lr"] and p["replaced"])
        w = O.Repo(O.TREG, 3)  # as local SETs: a losing SET still creates the delta key, with ("", 0)
        w.converge(_table(C.launch("keyed", [0], [p["state"][0]], [p["state"][1]])))
        w.treg_set(C.key_of(0), p["delta"][1], p["delta"][0])
        assert w.deltas_size() == 1
        d = w.flush().table()
        got = (int(d["ts"][0]), bytes(d["val_bytes"]))
        assert got == (p["delta"] if p["replaced"] else (0, b"")), p["name"]
    for reps in (1, 6):
        for kind in ("keyed", "set"):
            _check(O, [C.order_case(pairs, kind, reps)], len(pairs), sets=True)
    _check(O, [C.order_case(pairs, block_at=65)], 65 + len(pairs))


def test_order_matrix_coverage():
    pairs = C.order_pairs()
    ts = {(p["state"][0], p["delta"][0]) for p in pairs}
    for lo, hi in C.TS_PAIRS.values():
        assert (lo, hi) in ts and (hi, lo) in ts
    words = lambda t: (t >> 32, t & 0xFFFFFFFF)
    kinds = {(words(a)[0] != words(b)[0], words(a)[1] != words(b)[1]) for a, b in C.TS_PAIRS.values()}
    assert kinds == {(False, True), (True, False), (True, True)}
    assert any((a >> 32 < b >> 32) and (a & 0xFFFFFFFF) > (b & 0xFFFFFFFF) for a, b in C.TS_PAIRS.values())
    assert (2**63 - 1, 2**63) in ts and any(2**64 - 1 in x for x in ts)
    assert all((t, t) in ts for t in C.TS_TIES) and min(C.TS_TIES) >= 2**63
    vals = [(p["state"][1], p["delta"][1]) for p in pairs if p["state"][0] == p["delta"][0]]
    assert all(t in vals for t in C.TIES)
    assert {len(a) for a, _ in vals} >= set(C.VALUE_LENGTHS)
    first_diff = lambda a, b: next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), None)
    diffs = {(len(a), first_diff(a, b)) for a, b in vals if len(a) == len(b)}
    for n in C.VALUE_LENGTHS:
        for d in C.DIFF_AT + (n - 1,):
            if 0 <= d < n:
                assert (n, d) in diffs
    prefix = {(len(a), len(b)) for a, b in vals if a != b and (a.startswith(b) or b.startswith(a))}
    assert {(8, 9), (9, 8), (16, 17), (17, 16)} <= prefix
    assert all((x, x + b"\0") in vals and (x + b"\0", x) in vals for x in (bytes(range(0x61, 0x61 + n)) for n in (8, 9, 16)))
    assert any(a[0] >= 0x80 > b[0] for a, b in vals if a and b)
    assert any(p["same_lr"] and len(p["delta"][1]) > 8 for p in pairs)


# ---- the tiling model: where an entry index lands ---------------------------------------------
def _place(i):
    """entry i of a keyed launch -> (workgroup, wave, row of the wave, lane)"""
    return i // (256 * 4), i // 256, (i % 256) // 64, i % 64


def _fast_waves(slots):
    out = []
    for w in range(len(slots) // 256):
        run = slots[256 * w:256 * (w + 1)]
        if all(int(run[i]) == int(run[0]) + i for i in range(256)) and C.NO_SLOT not in run:
            out.append(w)
    return tuple(out)


def _row_words(slots, wave, row):
    return sorted({int(s) >> 5 for s in slots[256 * wave + 64 * row:256 * wave + 64 * (row + 1)]})


def test_claim_geometry(oracle_mod):
    """b. tags against the tiling model, duplicate counts against the arrays, coverage of the issue's
    list, and the outcome of three launches per layout against the oracle"""
    lays = C.claim_layouts(N_CLAIM, WORDS_CLAIM)
    by = lambda k: [l for l in lays if k in l["tags"]]
    for l in lays:
        s, t = l["slots"], l["tags"]
        assert t["fast"] == _fast_waves(s), l["name"]
        valid = s[s != C.NO_SLOT]
        assert l["dups"] == len(valid) - len(set(valid.tolist())) and valid.max() < N_CLAIM, l["name"]
        mode, grid, per = ("memset", 1, 0) if WORDS_CLAIM * 4 > 4096 * max(1, (len(s) + 1023) // 1024) else \
            ("slice", (len(s) + 1023) // 1024, None)
        assert C.clear_mode(len(s), WORDS_CLAIM)[0] == mode == ("memset" if len(s) <= 1024 else "slice"), l["name"]
    runs = [l for l in lays if l["name"].startswith("run of")]
    assert {(l["tags"]["size"], l["tags"]["start"]) for l in runs} >= {(n, s) for n in (256, 1280) for s in C.STARTS}
    assert all(l["dups"] == 0 and len(l["tags"]["fast"]) == l["tags"]["size"] // 256 for l in runs)
    assert any(int(l["slots"][-1]) == N_CLAIM - 1 for l in runs if l["tags"].get("last"))
    rel = {}
    for l in by("broken"):
        i, j, name = l["tags"]["broken"]
        (gi, wi, ri, _), (gj, wj, rj, _) = _place(i), _place(j)
        rel[name] = "row" if (wi, ri) == (wj, rj) else "wave" if wi == wj else "workgroup" if gi == gj else "grid"
        assert l["slots"][i] == l["slots"][j] and l["dups"] == 1 and wj not in l["tags"]["fast"]
    assert rel == {k: k for k in ("row", "wave", "workgroup", "grid")}
    assert sorted(l["tags"]["shared"] for l in by("shared")) == sorted(C.SHARED_AGAIN)
    for l in by("shared") + by("ends"):
        w0, w1 = set(l["slots"][:256].tolist()), l["slots"][256:].tolist()
        assert len(w1) == 256 and l["dups"] == len(w0 & set(w1))
        assert sorted(w1) != w1 and {s >> 5 for s in w0} & {s >> 5 for s in w1}
    for l in by("ends"):
        s0, w1 = l["tags"]["ends"], set(l["slots"][256:].tolist())
        assert s0 % 32 and {s0, s0 + 255, s0 - 1, s0 + 256} <= w1 and l["dups"] == 2
    assert sorted(l["tags"]["ends"] for l in by("ends")) == [1, 31, 33, 63]
    words = {}
    for l in by("agg_row"):
        ws = _row_words(l["slots"], 0, l["tags"]["agg_row"])
        if "words" in l["tags"]:
            assert len(ws) == l["tags"]["words"], l["name"]
            words[len(ws)] = l
        row = l["slots"][64:128].tolist()
        if "same" in l["tags"]:
            assert max(row.count(x) for x in row) == l["tags"]["same"] and l["dups"] == l["tags"]["same"] - 1
        if l["tags"].get("mixed"):
            groups = [[x for x in row if x >> 5 == w] for w in ws]
            assert sorted(len(g) - len(set(g)) for g in groups) == [0, 0, 1]
    assert set(words) == set(C.ROW_WORDS) and 4 > C.AGG >= 3
    assert sorted(l["tags"]["same"] for l in by("same")) == sorted(C.SAME_SLOT_LANES)
    for kind in ("ragged run", "ragged scatter of", "with repeats"):
        assert sorted(l["tags"]["size"] for l in lays if kind in l["name"] and
                      ("repeats" in kind or "repeats" not in l["name"])) == sorted(C.SIZES)
    assert all(l["tags"]["size"] % 256 for l in lays if "ragged run" in l["name"] and l["tags"]["size"] not in (256, 1024))
    for l in by("holes"):
        s = l["slots"]
        assert l["device_only"] and (s == C.NO_SLOT).sum() == l["tags"]["holes"]
        assert s[64] == s[127] == C.NO_SLOT and (s[128:192] == C.NO_SLOT).all() and s[65] != C.NO_SLOT
    assert sorted(l["dups"] for l in by("holes")) == [0, 1]
    assert sorted(l["tags"]["slices"] for l in by("slices")) == [2, 3]
    for l in by("slices"):
        grid = (len(l["slots"]) + 1023) // 1024
        nbytes = (WORDS_CLAIM * 4 + 15) // 16 * 16
        per = ((nbytes + grid - 1) // grid + 15) // 16 * 16
        named = set(l["slots"].tolist())
        want = set(range(8)) | set(range(N_CLAIM - 8, N_CLAIM))
        for g in range(1, grid):
            want |= {per * 8 * g - 1, per * 8 * g}
        assert want <= named and (N_CLAIM - 1) >> 5 == WORDS_CLAIM - 1, l["name"]
    clock = C._Clock()
    _check(oracle_mod, [C.geometry_case(l, clock) for l in lays], N_CLAIM)


def test_fold_depth(oracle_mod):
    """c. every m, order and place of the maximum occurs; duplicates = entries - distinct slots"""
    for kind in ("keyed", "set"):
        cases, n = C.fold_cases(kind)
        _check(oracle_mod, cases, n, sets=True)
    single = [c for c in cases if "order" in c["tags"] or "max_at" in c["tags"] or "equal" in c["tags"]]
    assert {c["tags"]["m"] for c in single} == set(C.FOLD_M)
    assert {c["tags"]["tail"] for c in single if c["tags"]["m"] > C.FOLD_ROUNDS} == set(C.TAIL_RECORDS)
    for m in C.FOLD_M:
        mine = [c for c in single if c["tags"]["m"] == m]
        assert {c["tags"].get("order") for c in mine} >= {"asc", "desc", "last byte"}
        assert {c["tags"]["max_at"] for c in mine if "max_at" in c["tags"]} == {a % m for a in C.MAX_AT if a < m}
        assert any(c["tags"].get("equal") for c in mine)
        for c in mine:
            L = c["launches"][-1]
            assert len(L["slots"]) == m and L["dups"] == m - 1 and len(set(L["slots"].tolist())) == 1
            ents = list(zip(L["ts"], L["vals"]))
            if c["tags"].get("order") in ("asc", "desc"):
                assert ents == sorted(ents, reverse=c["tags"]["order"] == "desc") and len(set(ents)) == m
            if c["tags"].get("order") == "last byte":
                assert len({t for t, _ in ents}) == 1 and len({v[:-1] for _, v in ents}) == 1 and len(ents[0][1]) > 16
            if "max_at" in c["tags"]:
                assert ents.index(max(ents)) == c["tags"]["max_at"]
    inter = {c["tags"]["interleaved"]: c for c in cases if "interleaved" in c["tags"]}
    assert set(inter) == {2, 3}
    for k, c in inter.items():
        s = c["launches"][-1]["slots"].tolist()
        assert all(s.count(x) == 69 for x in set(s)) and len(set(s)) == k and s[0] != s[1]
        assert c["launches"][-1]["dups"] == k * 68 and k * (69 - 4) > C.TAIL_CHUNK  # a slot spans tail chunks
    wide = [c for c in cases if "wide" in c["tags"]][0]["launches"][-1]
    assert len(set(wide["slots"].tolist())) == 700 and len(wide["slots"]) == 4200 and wide["dups"] == 3500
    assert 700 * (6 - 1 - C.FOLD_ROUNDS) > C.FOLD_TILE  # every round's list is longer than one stride


def test_dense_blocks(oracle_mod):
    """d. every start and every size; one winner at each listed position; all stale; all equal"""
    cases = C.dense_cases(N_DENSE)
    _check(oracle_mod, cases, N_DENSE)
    runs = [c for c in cases if "where" in c["tags"] and c["name"].startswith("block of")]
    assert {c["tags"]["size"] for c in runs} == set(C.SIZES)
    assert {c["tags"]["where"] for c in runs} == set(C.DENSE_STARTS) | {"last"}
    assert {c["tags"]["where"] for c in runs if c["tags"]["size"] == max(C.SIZES)} == set(C.DENSE_STARTS) | {"last"}
    for c in runs:
        L = c["launches"][0]
        assert L["slot0"] == (N_DENSE - len(L["ts"]) if c["tags"]["where"] == "last" else c["tags"]["where"])
        assert L["slots"].tolist() == list(range(L["slot0"], L["slot0"] + len(L["ts"]))) and L["slots"][-1] < N_DENSE
    assert {c["tags"]["winner"] for c in cases if "winner" in c["tags"]} == set(C.WINNER_AT) | {max(C.SIZES) - 1}
    assert [c["outcome"] for c in cases if c["tags"].get("loses") or c["tags"].get("equal")] == ["kept", "kept"]
    assert all(c["tags"]["size"] == max(C.SIZES) for c in cases if c["outcome"] in ("one", "kept"))


def test_routed_keys():
    """f. every pair has a key of each owner shard"""
    from jylis_amd.route import owners
    own = lambda k: int(owners(np.frombuffer(k, np.uint8), np.array([0, len(k)], np.uint64), 2)[0])
    keys = C.routed_keys(C.order_pairs()[:40], own)
    assert all([own(k) for k in row] == [0, 1] for row in keys) and len({k for row in keys for k in row}) == 80


def test_timestamps_are_unsigned_in_the_oracle(oracle_mod):
    O = oracle_mod
    r = O.Repo(O.TREG)
    for t, v in ((2**63 - 1, b"b"), (2**63, b"a"), (5, b"z")):
        r.converge(_table(C.launch("keyed", [0], [t], [v])))
    assert r.treg_get(C.key_of(0)) == (b"a", 2**63)
    r.converge(_table(C.launch("keyed", [0], [2**64 - 1], [b""])))
    assert r.treg_get(C.key_of(0)) == (b"", 2**64 - 1)
