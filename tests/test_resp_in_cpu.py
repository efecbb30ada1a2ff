"""RESP requests without a GPU: the reference decoder (tests/resp_in_ref.py),
the rules as plain C++ (jylis_amd/csrc/jy_resp_in.hpp through
tests/resp_in_check.cpp) and the case tables of tests/resp_in_cases.py.

1. resp_in_ref against hand-written literals, one per row of the class table
   of include/jylis_gpu.h "RESP requests", and the docs' TREG and TLOG sessions
   (tests/golden/kat_docs.json) written as requests.
2. tests/resp_in_check.cpp built with the address and undefined-behaviour
   sanitizers and run as a program of its own.
3. Conditions on the case tables, so that a GPU pass means something."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import resp_in_cases as RC
import resp_in_ref as ref
from resp_in_ref import request as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "kat_docs.json")


def _one(buf):
    return ref.decode(buf, np.array([0, len(buf)], np.uint64))


# ---- 1. literals ----
def test_request_writes_what_a_client_sends():
    assert R("TREG", "GET", "k") == b"*3\r\n$4\r\nTREG\r\n$3\r\nGET\r\n$1\r\nk\r\n"
    assert R() == b"*0\r\n"
    assert R("TLOG", "INS", "k", b"a\r\nb", 12) == b"*5\r\n$4\r\nTLOG\r\n$3\r\nINS\r\n$1\r\nk\r\n$4\r\na\r\nb\r\n$2\r\n12\r\n"


@pytest.mark.parametrize("words, kind, num, op, value", [
    (("GCOUNT", "INC", "k", "12"), ref.GCOUNT_INC, 12, 0, b""),
    (("GCOUNT", "GET", "k"), ref.GCOUNT_GET, 0, 0, b""),
    (("PNCOUNT", "INC", "k", "-2"), ref.PNCOUNT_INC, 2**64 - 2, 0, b""),
    (("PNCOUNT", "DEC", "k", "+3"), ref.PNCOUNT_DEC, 3, 0, b""),
    (("PNCOUNT", "GET", "k"), ref.PNCOUNT_GET, 0, 0, b""),
    (("TREG", "SET", "k", "hello", "10"), ref.TREG_SET, 10, 0, b"hello"),
    (("TREG", "GET", "k"), ref.TREG_GET, 0, 0, b""),
    (("TLOG", "INS", "k", "e", "5"), ref.TLOG_WRITE, 5, ref.TLOG_INS, b"e"),
    (("TLOG", "TRIMAT", "k", "4"), ref.TLOG_WRITE, 4, ref.TLOG_TRIMAT, b""),
    (("TLOG", "TRIM", "k", "3"), ref.TLOG_WRITE, 3, ref.TLOG_TRIM, b""),
    (("TLOG", "CLR", "k"), ref.TLOG_WRITE, 0, ref.TLOG_CLR, b""),
    (("TLOG", "GET", "k"), ref.TLOG_READ, ref.ALL, ref.RD_GET, b""),
    (("TLOG", "GET", "k", "2"), ref.TLOG_READ, 2, ref.RD_GET, b""),
    (("TLOG", "GET", "k", "two"), ref.TLOG_READ, ref.ALL, ref.RD_GET, b""),
    (("TLOG", "SIZE", "k"), ref.TLOG_READ, 0, ref.RD_SIZE, b""),
    (("TLOG", "CUTOFF", "k"), ref.TLOG_READ, 0, ref.RD_CUTOFF, b""),
])
def test_class_table_literals(words, kind, num, op, value):
    buf = R(*words)
    d = _one(buf)
    assert d["sizes"] == [1, len(words), 1, 1, len(value), 1]
    assert d["conn_used"].tolist() == [len(buf)] and d["conn_err"].tolist() == [0]
    assert d["cmd_kind"].tolist() == [kind] and d["cmd_phase"].tolist() == [0] and d["cmd_conn"].tolist() == [0]
    assert ref.commands(d, buf) == [[w.encode() for w in words]]
    assert d["row_cmd"].tolist() == [0] and d["num"].tolist() == [num] and d["op"].tolist() == [op]
    assert bytes(d["key_bytes"]) == b"k" and d["key_offs"].tolist() == [0, 1]
    assert bytes(d["val_bytes"]) == value and d["val_offs"].tolist() == [0, len(value)]
    assert (d["group_phase"].tolist(), d["group_class"].tolist(), d["group_offs"].tolist()) == ([0], [kind], [0, 1])


def test_host_and_framing_literals():
    d = _one(R("UJSON", "GET", "doc") + R() + R("TREG", "SET", "k", "v"))
    assert d["cmd_kind"].tolist() == [ref.HOST] * 3 and d["cmd_phase"].tolist() == [0, 0, 0]
    assert d["sizes"] == [3, 7, 0, 0, 0, 0] and d["cmd_word_offs"].tolist() == [0, 3, 3, 7]
    assert d["group_offs"].tolist() == [0]
    # a tail: used stops at the last complete command
    whole = R("GCOUNT", "GET", "k")
    for cut in range(1, len(whole)):
        d = _one(whole + whole[:cut])
        assert d["conn_used"].tolist() == [len(whole)] and d["conn_err"].tolist() == [0] and d["sizes"][0] == 1
    # violations: an inline command, a string where a header must stand, a header among the words, $-1
    for bad in (b"GET k\r\n", b"$3\r\nGET\r\n", b"*2\r\n$3\r\nGET\r\n*1\r\n", b"*1\r\n$-1\r\n", b"*-1\r\n", b"*1\r\n$3\r\nGETxx"):
        d = _one(whole + bad)
        assert d["conn_used"].tolist() == [len(whole)] and d["conn_err"].tolist() == [1] and d["sizes"][0] == 1, bad
    # nothing after the first violation is decoded
    d = _one(whole + b"x" + whole)
    assert d["sizes"][0] == 1 and d["conn_err"].tolist() == [1]
    # phases: a kind change inside a connection, HOST a kind of its own; rows sorted by (phase, kind)
    a = R("TREG", "SET", "k", "v", 1) + R("TREG", "SET", "j", "w", 2) + R("TREG", "GET", "k") + R("SYSTEM", "X") + \
        R("TREG", "GET", "j")
    b = R("TREG", "GET", "q")
    buf, offs = ref.join([a, b])
    d = ref.decode(buf, offs)
    assert d["cmd_phase"].tolist() == [0, 0, 1, 2, 3, 0]
    assert d["row_cmd"].tolist() == [0, 1, 5, 2, 4]
    assert d["group_phase"].tolist() == [0, 0, 1, 3] and d["group_offs"].tolist() == [0, 2, 3, 4, 5]
    assert d["group_class"].tolist() == [ref.TREG_SET, ref.TREG_GET, ref.TREG_GET, ref.TREG_GET]
    assert bytes(d["key_bytes"]) == b"kjqkj" and bytes(d["val_bytes"]) == b"vw"
    assert d["val_offs"].tolist() == [0, 1, 2, 2, 2, 2]


def test_docs_sessions_as_requests():
    """the docs' TREG and TLOG sessions: every step decodes to the class and
    the arguments the docs' command line shows"""
    kat = json.load(open(GOLD))
    for name, typ, writes, reads in (("treg_doc", "TREG", ref.TREG_SET, ref.TREG_GET),
                                     ("tlog_doc", "TLOG", ref.TLOG_WRITE, ref.TLOG_READ)):
        steps = RC.doc_requests(kat, name, typ)
        buf = b"".join(b for b, _, _ in steps)
        d = _one(buf)
        assert d["sizes"][0] == len(steps) and d["conn_used"].tolist() == [len(buf)] and not d["conn_err"][0]
        got = ref.commands(d, buf)
        for k, (_, words, expect) in enumerate(steps):
            assert got[k] == [w.encode() for w in words]
            assert d["cmd_kind"][k] == (writes if expect == "OK" else reads), words
        # a session alternates: its phases count the kind changes
        kinds = d["cmd_kind"].tolist()
        assert d["cmd_phase"].tolist() == np.cumsum([0] + [a != b for a, b in zip(kinds, kinds[1:])]).tolist()
        assert d["sizes"][2] == len(steps)


# ---- 2. the rules as plain C++ ----
def _host_compiler():
    for cc in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        path = shutil.which(cc) if cc else None
        if path:
            return path
    return None


def test_rules_stand_alone(tmp_path):
    """1 and 20 digit lengths, 2^64 - 1 and 2^64, the signed forms and the i64
    edges, every prefix of a token, the class table (tests/resp_in_check.cpp)"""
    cc = _host_compiler()
    if cc is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "resp_in_check")
    subprocess.run([cc, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "resp_in_check.cpp")],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
    # its sequential decoder agrees with the Python one on a mixed batch
    bufs = RC.phases() + RC.tricky() + RC.round_boundaries() + RC.prefix_sweep() + RC.corruption_sweep()[:200]
    buf, offs = ref.join(bufs)
    path = tmp_path / "batch.bin"
    path.write_bytes(np.uint64(len(bufs)).tobytes() + offs.tobytes() + buf)
    out = subprocess.run([exe, str(path), "1"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    got = json.loads(out.stdout)
    d = ref.decode(buf, offs)
    assert got["commands"] == d["sizes"][0] and got["rows"] == d["sizes"][2]
    assert got["closed"] == int(d["conn_err"].sum()) and got["used"] == int(d["conn_used"].sum())


# ---- 3. what the case tables cover ----
def _tokens(bufs):
    buf, offs = ref.join(bufs)
    toks = []
    for c in range(len(bufs)):
        ref.frame(buf, int(offs[c]), int(offs[c + 1]), toks)
    return buf, toks


def test_sweep_buffers():
    assert 100 <= len(RC.THREE) <= 140
    d = _one(RC.THREE)
    assert d["sizes"][0] == 3 and d["cmd_kind"].tolist() == [ref.TREG_SET, ref.TLOG_READ, ref.HOST]
    pre = RC.prefix_sweep()
    assert len(pre) == len(RC.THREE) + 1 and pre[0] == b"" and pre[-1] == RC.THREE
    buf, offs = ref.join(pre)
    d = ref.decode(buf, offs)
    assert not d["conn_err"].any()  # a prefix is never malformed
    assert RC.THREE_ENDS == (59, 99, 127)
    assert d["conn_used"].tolist() == [max([0] + [e for e in RC.THREE_ENDS if e <= n]) for n in range(len(pre))]
    # the corruption sweep: both outcomes occur, and a value's own \r\n is not framing
    assert _one(RC.TWO)["sizes"][0] == 2
    assert len(RC.framing_positions(RC.TWO)) == len(RC.TWO) - len(b"TLOGINSkv\r\n7GCOUNTGETk")
    cor = RC.corruption_sweep()
    buf, offs = ref.join(cor)
    d = ref.decode(buf, offs)
    assert len(cor) >= 5 * len(RC.framing_positions(RC.TWO)) and 0 < int(d["conn_err"].sum()) < len(cor)
    assert {0, 1, 2} == set(np.bincount(d["cmd_conn"], minlength=len(cor)).tolist())


def test_every_token_kind_starts_at_every_residue():
    buf, toks = _tokens(RC.residues() + RC.tricky())
    for first in (42, 36):
        assert {p % 8 for p, b in toks if b == first} == set(range(8)), first


def test_values_that_look_like_framing():
    bufs = RC.tricky()
    buf, offs = ref.join(bufs)
    d = ref.decode(buf, offs)
    assert not d["conn_err"].any() and d["conn_used"].tolist() == [len(b) for b in bufs]
    vals = [bytes(d["val_bytes"][int(a):int(b)]) for a, b in zip(d["val_offs"][:-1], d["val_offs"][1:])]
    assert RC.FAKE in vals and _one(RC.FAKE)["sizes"][0] == 1  # a value holds a well-formed command
    assert b"$" in vals and b"*" in vals
    assert any(len(v) > 2 * 256 for v in vals)  # spans more than two workgroups' bytes
    # '$' and '*' stand where a token would start if a reader skipped the length: right after a \r\n
    assert any(b"\r\n$3\r\n" in v for v in vals) and any(b"\r\n*2\r\n" in v for v in vals)
    keys = [bytes(d["key_bytes"][int(a):int(b)]) for a, b in zip(d["key_offs"][:-1], d["key_offs"][1:])]
    assert RC.FAKE in keys


def test_round_boundaries():
    bufs = RC.round_boundaries()
    assert b"" in bufs
    counts = []
    for b in bufs:
        toks = []
        cmds, used, err = ref.frame(b, 0, len(b), toks)
        assert used == len(b) and not err
        counts.append(len(toks))
    assert set(RC.TOKEN_COUNTS) | {0} == set(counts)
    assert counts.count(64) == 2 and counts.count(65) == 2 and counts.count(1025) == 2


def test_kinds_table():
    bufs, names = RC.kinds(with_big=False)
    buf, offs = ref.join(bufs)
    d = ref.decode(buf, offs)
    assert d["sizes"][0] == len(bufs) and not d["conn_err"].any()
    assert d["cmd_kind"].tolist() == [getattr(ref, n) for n in names]
    assert set(d["cmd_kind"].tolist()) == set(range(10))  # every class
    assert {ref.TLOG_INS, ref.TLOG_TRIMAT, ref.TLOG_TRIM, ref.TLOG_CLR} == \
        set(d["op"][d["cmd_kind"][d["row_cmd"]] == ref.TLOG_WRITE].tolist())
    lens = np.diff(d["key_offs"].astype(np.int64))
    vlens = np.diff(d["val_offs"].astype(np.int64))
    assert (lens == 0).any() and (vlens[d["cmd_kind"][d["row_cmd"]] == ref.TREG_SET] == 0).any()
    big, names = RC.kinds()
    assert [n for n in names[-3:]] == ["TREG_SET", "HOST", "HOST"] and len(big[-3]) > 2**24


def test_phases_and_pipelining_tables():
    bufs = RC.phases()
    buf, offs = ref.join(bufs)
    d = ref.decode(buf, offs)
    assert d["cmd_phase"][d["cmd_conn"] == 0].tolist() == list(range(20))  # SET / GET / INS / GET, five times
    assert d["cmd_phase"][d["cmd_conn"] == 1].tolist() == [0, 0, 1, 2, 2, 3]
    assert d["cmd_phase"][d["cmd_conn"] == 2].tolist() == [0, 1, 2, 3]
    assert len(d["group_offs"]) - 1 > 20
    pipe = RC.pipelined(ncmd=300, nsingle=6, big=5000)
    assert len(pipe) == 8 and max(len(b) for b in pipe) > 5000
