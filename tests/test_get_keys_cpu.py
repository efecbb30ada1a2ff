"""The keyed reads' reference (tests/get_ref.py) against the reference's own
known answers, and the three calls' declarations.  Runs without a GPU.

tests/golden/kat_docs.json holds the docs' TLOG and TREG sessions with their
replies.  They are replayed through the CPU oracle, and get_ref -- what the
GPU tests compare jy_*_get_keys with -- must reproduce every recorded GET /
GET key 1 / SIZE / CUTOFF reply from the oracle's state table."""
import json
import os
import re

import get_ref
from test_pony_glue import header_arity, pony_decls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "kat_docs.json")


def _kat():
    with open(GOLD) as f:
        return json.load(f)


def test_tlog_doc_replies(oracle_mod):
    O = oracle_mod
    r = O.Repo(O.TLOG)
    reads = 0
    for step in _kat()["tlog_doc"]["steps"]:
        op, key = step[0], step[1]
        if op == "INS":
            r.tlog_ins(key, step[2], step[3])
        elif op == "TRIM":
            r.tlog_trim(key, step[2])
        elif op == "TRIMAT":
            r.tlog_trimat(key, step[2])
        elif op == "CLR":
            r.tlog_clr(key)
        else:
            reads += 1
            st = r.state()
            if op in ("SIZE", "CUTOFF"):
                ref = get_ref.tlog_get(st, [key], [0])
                assert ref["sizes"][:2] == [0, 0]  # count 0 returns no entry
                assert int(ref["size" if op == "SIZE" else "cutoff"][0]) == step[2]
            else:
                ref = get_ref.tlog_get(st, [key], [1] if op == "GET1" else None)
                exp = [(v.encode(), ts) for v, ts in step[2]]
                assert get_ref.tlog_reply(ref, 0) == exp
                assert ref["sizes"][0] == len(exp) == min(int(ref["size"][0]), 1 if op == "GET1" else get_ref.ALL)
            # a key nobody wrote, beside it: found 0, nothing else
            miss = get_ref.tlog_get(st, ["nobody", key, "nobody"], [5, 0, None])
            assert miss["found"].tolist() == [0, 1, 0] and miss["ent_offs"].tolist() == [0, 0, 0, 0]
            assert int(miss["size"][0]) == int(miss["cutoff"][2]) == 0
    assert reads >= 4


def test_treg_doc_replies(oracle_mod):
    O = oracle_mod
    r = O.Repo(O.TREG)
    reads = 0
    for step in _kat()["treg_doc"]["steps"]:
        if step[0] == "SET":
            r.treg_set(step[1], step[2], step[3])
            continue
        reads += 1
        ref = get_ref.treg_get(r.state(), [step[1], "nobody"])
        exp = step[2]
        assert get_ref.treg_reply(ref, 0) == (None if exp is None else (exp[0].encode(), exp[1]))
        assert get_ref.treg_reply(ref, 1) is None
        assert ref["sizes"] == [0 if exp is None else len(exp[0].encode()), 0 if exp is None else 1]
    assert reads >= 2


def test_entries_returned_are_the_sum_of_min_size_count(oracle_mod):
    """what holds without a GPU: the entries returned are sum(min(size, count))
    and the bytes their values' bytes -- a long log under count 10 gives 10"""
    O = oracle_mod
    r = O.Repo(O.TLOG)
    for t in range(300):
        r.tlog_ins("long", b"v%03d" % t, t)
    for t in range(3):
        r.tlog_ins("short", b"abcdefghij", t)
    ref = get_ref.tlog_get(r.state(), ["long", "short", "none"], [10, 10, 10])
    assert ref["size"].tolist() == [300, 3, 0]
    assert ref["sizes"] == [10 + 3, 10 * 4 + 3 * 10, 2]
    assert get_ref.tlog_reply(ref, 0) == [(b"v%03d" % t, t) for t in range(299, 289, -1)]


def _lib_signatures():
    text = open(os.path.join(ROOT, "jylis_amd", "_lib.py")).read()
    out = {}
    for m in re.finditer(r'"(jy_[a-z0-9_]+)":\s*\(\w+,\s*\[([^\]]*)\]\)', text):
        out[m.group(1)] = len([a for a in m.group(2).split(",") if a.strip()])
    return out


def test_the_three_calls_are_declared_alike():
    hdr, pony, lib = header_arity(), pony_decls(), _lib_signatures()
    want = {"jy_treg_get_keys": 12, "jy_tlog_get_keys": 17, "jy_counter_get_keys": 9}
    for name, arity in want.items():
        assert hdr.get(name) == arity, (name, "include/jylis_gpu.h", hdr.get(name))
        assert lib.get(name) == arity, (name, "jylis_amd/_lib.py", lib.get(name))
        assert pony.get(name) == arity, (name, "pony/jylis_gpu/ffi.pony", pony.get(name))
    glue = open(os.path.join(ROOT, "pony", "jylis_gpu", "repo_logs_gpu.pony")).read()
    assert "@jy_treg_get_keys(" in glue and "@jy_tlog_get_keys(" in glue
    assert "NOT COMPILE-CHECKED" in glue
