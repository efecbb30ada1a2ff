"""The TLOG sweeps' helpers and case tables, checked without a GPU:
tlog_layout.check_layout / classify on hand-made layouts, and every case
generator of test_tlog_sweep_gpu.py against the oracle alone -- the deltas
are accepted (or, the malformed ones, re-sorted) as intended, and the counts
of kept-interleaving, kept-newer, duplicate and below-cutoff entries the
oracle's converge shows equal what each case declares."""
import numpy as np
import pytest

import test_tlog_sweep_gpu as G
from test_parity_tlog import _canon, _log_batch
from tlog_layout import (OUTCOMES, check_entries, check_layout, classify, expected_outcome, merge_model,
                         oracle_counts, table_logs)


def _layout(rows, pcap=1000):
    cols = list(zip(*rows)) if rows else [[]] * 4
    lay = {c: np.array(v, np.uint64) for c, v in zip(("base", "front", "len", "cap"), cols)}
    lay["cutoff"] = lay["newest"] = np.zeros(len(rows), np.uint64)
    lay["pcap"], lay["used"] = pcap, 0
    return lay


def test_check_layout():
    good = [(10, 2, 5, 8), (20, 2, 8, 8), (0, 0, 0, 0), (500, 100, 1, 500)]
    check_layout(_layout(good))
    check_layout(_layout([(5, 5, 1, 4), (9, 0, 0, 100)]))  # an empty log owns nothing
    for bad in ([(10, 2, 5, 9), (20, 2, 8, 8)],      # [8, 19) and [18, 28): one entry shared
                [(10, 2, 5, 8), (20, 3, 8, 8)],      # the same from the front room's side
                [(10, 2, 9, 8)],                     # len > cap
                [(990, 0, 1, 11)],                   # base + cap > pcap
                [(3, 4, 1, 8)]):                     # front > base
        with pytest.raises(AssertionError):
            check_layout(_layout(bad))


def test_check_entries():
    lay = _layout([(0, 0, 2, 4)])
    lay["cutoff"], lay["newest"] = np.array([5], np.uint64), np.array([9], np.uint64)
    tab = _log_batch([("k", 5, [(b"b", 9), (b"a", 9)])])
    check_entries(lay, tab)
    for ents, newest, cut in (([(b"a", 9), (b"b", 9)], 9, 5), ([(b"b", 9), (b"a", 8)], 8, 5),
                              ([(b"b", 9), (b"a", 4)], 9, 5), ([(b"b", 9), (b"b", 9)], 9, 5)):
        lay["newest"] = np.array([newest], np.uint64)
        with pytest.raises(AssertionError):
            check_entries(lay, _log_batch([("k", cut, ents)]))


def test_classify_names_every_outcome():
    before = (100, 10, 20, 40)
    got = [classify(before, before, 0, 0, False),
           classify(before, (103, 13, 19, 37), 3, 0, False),   # base + drop, nothing inside the log
           classify(before, (103, 13, 20, 37), 3, 2, True),    # base + drop, interleaved
           classify(before, (101, 11, 20, 39), 3, 2, True),    # base + drop - Mi
           classify(before, (400, 5, 21, 100), 0, 1, True)]    # outside [90, 140)
    assert tuple(got) == OUTCOMES
    assert classify((0, 0, 0, 0), (8, 0, 1, 8), 0, 0, False) == "rebuild"  # a fresh key
    assert classify(before, (89, 0, 21, 100), 0, 0, False) == "rebuild"
    with pytest.raises(AssertionError):
        classify(before, (104, 14, 20, 36), 3, 2, True)


def test_expected_outcome_follows_the_stated_choice():
    st = dict(M=1, inter=1, drop=0, minrank=3, mx=3)
    assert expected_outcome((100, 10, 20, 40), st) == "insert_down"          # 3 down, 17 up
    assert expected_outcome((100, 10, 6, 40), st) == "insert_up"             # 3 == 3: up
    assert expected_outcome((100, 0, 20, 40), st) == "insert_up"             # no front room
    assert expected_outcome((100, 0, 20, 40), dict(st, drop=1)) == "insert_down"  # the dropped prefix is room
    two = dict(M=2, inter=1, drop=0, minrank=19, mx=19)
    assert expected_outcome((100, 10, 20, 21), two) == "insert_down"         # up does not fit
    assert expected_outcome((100, 10, 20, 20), two) == "rebuild"
    assert expected_outcome((100, 10, 20, 20), dict(M=0, inter=0, drop=0, minrank=20, mx=0)) == "unchanged"
    assert expected_outcome((100, 10, 20, 20), dict(M=1, inter=0, drop=0, minrank=20, mx=0)) == "rebuild"


def _check_cases(O, cases):
    """the oracle alone: build each case's state, converge its probe, compare"""
    want = O.Repo(O.TLOG)
    model = {c["key"]: ([], 0) for c in cases}
    for i in range(max(len(c["steps"]) for c in cases)):
        logs = []
        for c in cases:
            if i < len(c["steps"]):
                log, cut = model[c["key"]]
                dcut, ents = G.resolve(c["steps"][i], log, G.fresh_cap(len(log)) if log else 0)
                model[c["key"]] = merge_model(log, cut, dcut, ents)[:2]
                logs.append((c["key"], dcut, _canon(ents)))
        want.converge(_log_batch(logs))
    before = table_logs(want.state())
    for k, (c, l) in before.items():
        assert model[k.decode()] == (l, c), k
    logs, probes = [], {}
    for c in cases:
        dcut, ents = c["probe"](model[c["key"]][0]) if callable(c["probe"]) else c["probe"]
        probes[c["key"]] = (dcut, ents)
        if c["malformed"]:
            # not a log as given: the engine skips it; in canonical order it is an ordinary delta
            assert list(ents) != _canon(ents), c["key"]
            continue
        assert list(ents) == list(dict.fromkeys(ents)), c["key"]
        logs.append((c["key"], dcut, _canon(ents)))
    want.converge(_log_batch(logs))
    after = table_logs(want.state())
    for c in cases:
        if c["malformed"]:
            continue
        k = c["key"].encode()
        dcut, ents = probes[c["key"]]
        got = oracle_counts(before.get(k, (0, [])), after[k], dcut, ents)
        assert got == tuple(c["decl"]), (c["key"], "oracle", got, "declared", c["decl"])
        log, cut = model[c["key"]]
        nlog, ncut, st = merge_model(log, cut, dcut, ents)
        assert (ncut, nlog) == after[k], c["key"]
        assert (st["inter"], st["newer"], st["dup"], st["below"]) == got
        assert c["expect"] in OUTCOMES + (None,) and c["path"] in ("skip", "fast", "slow")


@pytest.mark.parametrize("Ls", G.SEARCH_GROUPS, ids=lambda g: "L" + "-".join(map(str, g)))
def test_search_cases(oracle_mod, Ls):
    cases = G.search_cases(Ls)
    assert len({c["key"] for c in cases}) == len(cases)
    _check_cases(oracle_mod, cases)
    for L in Ls:
        mine = [c for c in cases if c["tag"][0] == L]
        assert {c["tag"][1] for c in mine} == set(G.FLAVOURS if L >= 3 else G.FLAVOURS[:4])
        for fl in ("between", "tie_above"):
            assert {c["tag"][2] for c in mine if c["tag"][1] == fl} >= set(G.probes(L)) - {0}, (L, fl)
        for fl in ("tie_below", "dup"):
            assert {c["tag"][2] for c in mine if c["tag"][1] == fl} >= set(G.probes(L)) - {L}, (L, fl)
    assert sorted(L for g in G.SEARCH_GROUPS for L in g) == sorted(G.SEARCH_L)


def test_fast_move_and_tile_cases(oracle_mod):
    for cases in (G.fast_cases(), G.move_cases(), [c for b in G.tile_batches() for c in b],
                  [c for t in G.queue_tiles() for c in t]):
        assert len({c["key"] for c in cases}) == len(cases)
        _check_cases(oracle_mod, cases)
    assert [len(b) for b in G.tile_batches()] == [nd for nd, _ in G.TILE_TABLE]
    assert all(len(t) == 64 for t in G.queue_tiles())
    moves = G.move_cases()
    for direction in ("insert_up", "insert_down"):
        assert {c["tag"][1] for c in moves if c["tag"][0] == direction} >= set(G.MOVED)
        assert {c["tag"][2] for c in moves if c["tag"][0] == direction} >= set(G.DELTA_N)
