"""The UJSON sweeps' generators and invariant check, without a GPU: every
generator of ujson_cases.py runs against the oracle alone -- each probe is a
well-formed delta (or, in the skip sweep, breaks exactly the rule it names),
and the outcome each case declares is what the oracle's state shows before and
after -- and check_raw passes on the oracle's states and fails on hand-made
violations."""
import numpy as np
import pytest

import ujson_cases as C


def _raw(table, R):
    """an oracle state table in Engine.ujson_read's form"""
    docs = C.doc_states(table)
    keys = sorted(docs)
    dots, elems, cloud, eo, co = [], [], [], [0], [0]
    vv = np.zeros((max(len(keys), 1), R), np.uint64)
    for i, k in enumerate(keys):
        els, v, cl = docs[k]
        for (c, q), e in sorted(els.items()):
            dots.append((c << C.SEQ_BITS) | q), elems.append(e)
        for c, n in v.items():
            vv[i, c] = n
        cloud += [(c << C.SEQ_BITS) | q for c, q in sorted(cl)]
        eo.append(len(dots)), co.append(len(cloud))
    a = lambda x: np.array(x, np.uint64)
    return keys, (a(eo), a(dots), a(elems), vv[:len(keys)], a(co), a(cloud))


def _check_cases(O, cases, R=16):
    """the oracle alone: build every case's state, converge the probes, compare"""
    assert len({c["key"] for c in cases}) == len(cases)
    want = O.Repo(O.UJSON, 1)
    bs = C.batches(cases)
    before = {}
    for n, batch in enumerate(bs):
        if n == len(bs) - 1:
            before = C.doc_states(want.state())
        for c, d, probe in batch:
            rule = C.violation(d, R)
            if probe and c["malformed"]:
                assert rule == c["expect"] or (rule is None and (c["repeat"] > 1 or c["hole"])), (c["key"], rule)
            else:
                assert rule is None, (c["key"], rule)
        docs = C.applied(batch)
        if docs:
            want.converge(C.oracle_table(docs))
        keys, raw = _raw(want.state(), R)
        C.check_raw(raw, [keys.index(c["key"]) for c in cases if c["ctx_free"] and c["key"] in keys])
    after = C.doc_states(want.state())
    for c in cases:
        b, a = before.get(c["key"], C.EMPTY), after.get(c["key"], C.EMPTY)
        got, declared = C.observed(c, b, a), c["after"] if c["sweep"] in ("inplace", "tile") else c["expect"]
        assert got == declared, (c["key"], c.get("tag"), "oracle", got, "declared", declared)
        if c["malformed"]:
            assert a == b, c["key"]
    assert sum(c["skips"] for c in cases) == sum(1 for c in cases if c["malformed"] and not c["hole"])
    return before, after


def test_search_cases(oracle_mod):
    cases = C.search_cases()
    _check_cases(oracle_mod, cases)
    tags = {c["tag"] for c in cases}
    for straddle in (False, True):
        for L in C.SEARCH_L:
            if straddle and L < 2:
                continue
            for side in C.SEARCH_SIDES:
                mine = {t for t in tags if t[0] == side and t[1] == L and t[4] == straddle}
                assert {t[3] for t in mine if t[2] == "equal"} == set(C.ranks(L, True)), (side, L)
                assert {t[3] for t in mine if t[2] != "equal"} == set(C.ranks(L, False)), (side, L)
                if L:
                    assert {"below", "above"} <= {t[2] for t in mine}
    assert C.ranks(8, True)[-1] == 7 and C.ranks(65, True)[-1] == 64  # the window's last position
    assert C.ranks(64, False) == [0, 1, 2, 3, 4, 31, 32, 33, 60, 61, 62, 63, 64]
    assert {c["expect"] for c in cases} == {"kept", "dropped", "replaced", "added", "deduplicated"}
    for L in C.SEARCH_L:  # replaced at every equal rank, the window's last position included
        assert {c["tag"][3] for c in cases if c["expect"] == "replaced" and c["tag"][1] == L} == set(C.ranks(L, True))
    for c in cases:  # a straddling segment's neighbours: (c, SEQ_MAX - 1) next to (c + 1, 2)
        assert c["dot"][1] <= C.SEQ_MAX
    assert any(c["dot"] == (3, C.SEQ_MAX) for c in cases) and any(c["dot"] == (4, 1) for c in cases)


def test_join_cases(oracle_mod):
    cases = C.join_cases()
    before, _ = _check_cases(oracle_mod, cases)
    assert len({c["tag"] for c in cases}) == 2 * 2 * 3 * 3 * 3 == len(cases)
    for c in cases:  # the state is the combination the case names
        pos, smap, sctx, dmap, dctx = c["tag"]
        doc, d = before[c["key"]], c["dot"]
        assert (d in doc[0]) == smap
        assert (d[1] <= doc[1].get(d[0], 0), d in doc[2]) == (sctx == "vv", sctx == "cloud")
        segs = [sorted(doc[0]), sorted(doc[2]), [x[:2] for x in c["probe"]["el"]], c["probe"]["cl"]]
        for seg in segs:
            if d in seg:
                assert seg[0 if pos == "first" else -1] == d
    assert {c["expect"] for c in cases} == {None, 41, 42}
    # the replace bit and the keep rule, each decided both ways
    assert {c["expect"] for c in cases if c["tag"][1] and c["tag"][3] == "diff"} == {41, 42}
    assert {c["expect"] for c in cases if c["tag"][1] and c["tag"][3] is None} == {None, 41}


@pytest.mark.parametrize("R", [16, 1, 2, 64])
def test_fold_cases(oracle_mod, R):
    col = 3 if R == 16 else R - 1
    cases = C.fold_cases(col)
    _check_cases(oracle_mod, cases, R)
    tags = {c["tag"] for c in cases}
    for n in C.FOLD_N:
        for v in C.FOLD_V + (C.SEQ_MAX - n,):
            names = {t[2] for t in tags if t[:2] == (v, n)}
            assert {"split1", "split%d" % n, "gap0", "gap%d" % (n - 1)} <= names
            assert n > 9 or {"split%d" % k for k in range(1, n + 1)} <= names
            assert v == 0 or {"deltavv1", "deltavv%d" % n} <= names
            assert n < 2 or {"interleaved", "both1"} <= names
    assert max(c["expect"][1] for c in cases) == C.SEQ_MAX
    assert {c["expect"][0] for c in cases} >= {0, 1, 2, 3, 4, 5, 8, 9, 63, 64, 65}


@pytest.mark.parametrize("kind", C.COUNT_KINDS)
@pytest.mark.parametrize("N", C.DOC_COUNTS)
def test_count_cases(oracle_mod, N, kind):
    cases = C.count_cases(N, kind)
    assert len(cases) == N
    _check_cases(oracle_mod, cases)
    paths = [c["path"].split("/")[0] for c in cases]
    assert [i for i, p in enumerate(paths) if p == "items"] == sorted({0, N // 2, N - 1})
    assert N < 3 or "empty" in paths
    assert sum(len(c["probe"][kind]) for c in cases) <= C.TILE  # one item tile over all N documents


def test_skip_cases(oracle_mod):
    R = 16
    cases = C.skip_cases(R)
    _check_cases(oracle_mod, cases, R)
    bad = [c for c in cases if c["malformed"]]
    assert {c["expect"] for c in bad} == {"column", "seq0", "equal", "descending", "vv_order", "vv_column",
                                          "repeated", "hole"}
    for rule in ("column", "seq0", "equal", "descending"):
        assert {c["path"] for c in bad if c["expect"] == rule} >= {"el/first", "el/last", "cl/first", "cl/last"}
    for rule in ("vv_order", "vv_column"):
        assert {c["path"] for c in bad if c["expect"] == rule} >= {"vv/first", "vv/last"}
    # the tile edges: documents 255 | 256 at element 256, documents 511 | 512 at cloud dot 512
    docs = [c for c, _, _ in C.batches(cases)[-1]]
    for kind, i in (("el", C.DOC_TILE - 1), ("cl", 2 * C.DOC_TILE - 1)):
        assert docs[i]["malformed"] and docs[i]["path"] == kind + "/tile-edge" and not docs[i + 1]["malformed"]
        assert sum(len(c["probe"][kind]) for c in docs[:i + 1]) == (i + 1)
    assert sum(c["skips"] for c in cases) == len(bad) - 1


def _check_layout(cases, before):
    """the offsets the generator laid out are those of the oracle's states and the probes, in batch order"""
    off = dict(A=0, C=0, B=0, D=0)
    for c in cases:
        assert c["lay"] == off, c["key"]
        if "seg" in c:
            sp = C.SPACES[c["side"]]
            sz = C.space_sizes(before.get(c["key"], C.EMPTY), c["probe"])[sp]
            assert c["seg"] == (off[sp], sz), c["key"]
            f0, f1, mapped = C.whole_tiles(off[sp], sz)
            assert (c["whole"], c["mapped"]) == (f0 < f1, mapped), c["key"]
            assert c["path"].split("/")[1] == ("map" if mapped else "whole-ids" if f0 < f1 else "ids")
        for k, v in C.space_sizes(before.get(c["key"], C.EMPTY), c["probe"]).items():
            off[k] += v
    return off


def test_tile_cases(oracle_mod):
    cases = C.tile_cases()
    before, _ = _check_cases(oracle_mod, cases)
    _check_layout(cases, before)
    targets = [c for c in cases if "seg" in c]
    assert {c["tag"] for c in targets} == {(s, L, o) for s in C.SPACES for L in C.TILE_LENGTHS for o in C.TILE_OFFSETS}
    for c in targets:
        side, L, o = c["tag"]
        assert c["seg"][0] % C.TILE == o and c["seg"][1] == L
        assert c["mapped"] == (L > C.LONG_SEG)  # past kLongSeg a segment always holds a whole tile
    for side in C.SPACES:  # whole tiles that stay on the ids path, segments with none, mapped ones
        assert {c["path"] for c in targets if c["side"] == side} == {side + "/map", side + "/whole-ids", side + "/ids"}


def test_wave_cases(oracle_mod):
    cases = C.wave_cases()
    before, _ = _check_cases(oracle_mod, cases)
    off = _check_layout(cases, before)
    targets = [c for c in cases if "seg" in c]
    assert all(c["mapped"] for c in targets)
    for c in targets:  # the role from the oracle's own layout
        if len(c["tag"]) == 4:
            L, o, p, fl = c["tag"]
            assert c["role"] == C.wave_role(c["seg"][0], p, fl)
    # every place against a wave's range, in a tile the map names
    assert {c["role"] for c in targets if c["in_map"]} == {"none", "d0", "d1-1", "below-d0", "above-d1-1", "inside"}
    for p in C.WAVE_POSITIONS:
        assert {c["tag"][3] for c in targets if len(c["tag"]) == 4 and c["tag"][2] == p} == {"equal", "below", "above"}
    last = cases[-1]
    assert last["role"] == "ragged" and last["mapped"] and off["A"] % C.WAVE == 1
    assert sum(last["seg"]) == off["A"]


def test_inplace_cases(oracle_mod):
    cases = C.inplace_cases()
    _check_cases(oracle_mod, cases, 4)
    assert {c["path"] for c in cases} >= {"trim", "demote", "trim/resend", "demote/resend", "append/ecap",
                                          "append/regrow", "append/fold-gap", "append/no-fold"}
    for n in C.JOB_DOCS:
        for how in ("demote", "regrow"):
            jobs = C.job_cases(n, how)
            assert len(jobs) == n
            _check_cases(oracle_mod, jobs, 4)
    assert C.JOB_DOCS[0] < C.JOB_BUF < C.JOB_DOCS[2] and C.JOB_BUF in C.JOB_DOCS


def _read(docs, R=4):
    """[(elements [(c, q)], vv {c: n}, cloud [(c, q)])] -> a raw read"""
    dots, cloud, eo, co = [], [], [0], [0]
    vv = np.zeros((len(docs), R), np.uint64)
    for i, (els, v, cl) in enumerate(docs):
        dots += [(c << C.SEQ_BITS) | q for c, q in els]
        cloud += [(c << C.SEQ_BITS) | q for c, q in cl]
        for c, n in v.items():
            vv[i, c] = n
        eo.append(len(dots)), co.append(len(cloud))
    a = lambda x: np.array(x, np.uint64)
    return a(eo), a(dots), a(dots), vv, a(co), a(cloud)


def test_check_raw():
    good = [([(0, 1), (0, 5), (1, 2)], {0: 3, 1: 2}, [(0, 5), (0, 7), (2, 2)]),
            ([], {}, []),
            ([(0, 1)], {0: 1}, []),                      # a document may start below the one before
            ([(3, C.SEQ_MAX)], {}, [(3, C.SEQ_MAX)])]
    C.check_raw(_read(good))
    C.check_raw(_read([]))
    for bad in ([([(0, 5), (0, 5)], {0: 9}, [])],                 # equal element dots
                [([(1, 1), (0, 2)], {0: 9, 1: 9}, [])],           # descending element dots
                [([], {}, [(0, 7), (0, 5)])],                     # descending cloud
                [([], {}, [(0, 5), (0, 5)])],                     # equal cloud dots
                [([], {0: 5}, [(0, 5)])],                         # a cloud dot at its vv entry
                [([], {0: 5}, [(0, 3)])],                         # below it
                [([], {0: 5}, [(0, 6)])],                         # vv + 1: not compacted
                [([], {}, [(2, 1)])],                             # 0 + 1
                [([(0, 6)], {0: 5}, [(0, 8)])],                   # an element outside the context
                [([(0, 6)], {0: 5}, []), ([], {}, [(0, 6)])],     # ... that another document's cloud holds
                [([], {}, [(4, 2)])]):                            # a column outside the vv
        with pytest.raises(AssertionError):
            C.check_raw(_read(bad))
    C.check_raw(_read([([(0, 6)], {0: 5}, [])]), exempt=[0])
