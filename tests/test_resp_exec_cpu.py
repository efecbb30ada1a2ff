"""RESP execute without a GPU: the assembly rules as plain C++
(jylis_amd/csrc/jy_resp_out.hpp through tests/resp_out_check.cpp), conditions on
the inputs of tests/test_resp_exec_gpu.py so that a GPU pass means something,
and the new entry points in the header, the Python binding and the Pony FFI."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import resp_exec_cases as XC
import resp_in_ref as ref
from test_pony_glue import header_arity, pony_decls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_compiler():
    for cc in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        path = shutil.which(cc) if cc else None
        if path:
            return path
    return None


def test_rules_stand_alone(tmp_path):
    """row_range, host_range, group_of and first_cmd_of run sequentially over small
    heartbeats, under the address and undefined-behaviour sanitizers"""
    cc = _host_compiler()
    if cc is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "resp_out_check")
    subprocess.run([cc, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "resp_out_check.cpp")],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr


def test_permutation_is_one():
    d = ref.decode(*ref.join(XC.permutation()))
    rc = d["row_cmd"].tolist()
    assert sorted(rc) == list(range(5)) and rc != list(range(5))  # a permutation, not the identity
    # a read after a write in its own connection: GET a (phase 2) follows SET a (phase 1)
    assert d["cmd_kind"].tolist() == [ref.TREG_GET, ref.TREG_SET, ref.TREG_GET, ref.TREG_SET, ref.TREG_GET]
    assert d["cmd_phase"].tolist() == [0, 1, 2, 0, 1] and d["cmd_conn"].tolist() == [0, 0, 0, 1, 1]


def test_boundary_counts_straddle_the_constants():
    assert XC.SCAN_TILE == 2048 and XC.GATHER_STAGE == 1024  # read from jy_dscan.hpp and jy_wire.hpp
    assert sorted(XC.BOUNDARY_COUNTS) == [1023, 1024, 1025, 2047, 2048, 2049]
    for n in (XC.GATHER_STAGE - 1, XC.SCAN_TILE + 1):
        conns = XC.ok_heartbeat(n)
        d = ref.decode(*ref.join(conns))
        assert d["sizes"][0] == n and d["sizes"][5] == 1 and len(conns) == 3 and all(conns)
        assert {5 * k % 8 for k in range(n)} == set(range(8))  # every residue mod 8
        conns, want = XC.digits_heartbeat(n)
        assert ref.decode(*ref.join(conns))["sizes"][0] == n
        assert {len(b":%d\r\n" % v) - 3 for v in XC.DIGIT_VALUES} == set(range(1, 21))
        assert sum(map(len, want)) == sum(len(b":%d\r\n" % XC.DIGIT_VALUES[i % 20]) for i in range(n))


def test_empty_range_positions():
    cases = XC.empty_ranges()
    done = lambda c: len(ref.frame(c, 0, len(c))[0])
    has = {name: [done(c) > 0 for c in conns] for name, conns in cases.items()}
    assert has["first"] == [False, True, True] and has["last"] == [True, True, False]
    assert has["middle"] == [True, False, False, True] and has["all"] == [False] * 3 and has["none"] == []
    assert ref.frame(XC.PART, 0, len(XC.PART)) == ([], 0, 0)  # only an incomplete command: used 0, not closed
    assert ref.frame(XC.BAD, 0, len(XC.BAD)) == ([], 0, 1)    # malformed from byte 0: closed
    assert has["incomplete"] == [True, False, True] and has["malformed"] == [True, False, True]
    assert has["mixed"] == [False, True, False, False, False, True, False]


def test_new_symbols_are_declared_alike():
    from jylis_amd import _lib
    hdr, pony = header_arity(), pony_decls()
    for name, arity in (("jy_resp_sink_write", 3), ("jy_resp_exec", 9), ("jy_resp_replies", 9)):
        assert hdr.get(name) == arity, (name, hdr.get(name))
        assert pony.get(name) == arity, (name, pony.get(name))
        assert len(_lib.SIGNATURES[name][1]) == arity, name
    text = open(os.path.join(ROOT, "include", "jylis_gpu.h")).read()
    assert "(*jy_resp_host_fn)(void* ctx, uint64_t cmd, uint64_t nwords" in text
    assert len(_lib.RESP_HOST_FN._argtypes_) == 6  # ctx, cmd, nwords, words, lens, sink
    from jylis_amd.engine import Engine
    assert callable(Engine.resp_exec)
