"""The host round split (jylis_amd/csrc/jy_rounds.hpp) on its own: a plain
C++ program, built with the host compiler and the address and
undefined-behaviour sanitizers, run as a child process."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_compiler():
    # oracle/Makefile: CXX ?= g++
    for cc in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        path = shutil.which(cc) if cc else None
        if path:
            return path
    return None


def test_round_split_and_gather(tmp_path):
    """n = 0 and 1; distinct slots build nothing; [a,b,a,c,a,b,a] gives the
    rounds {0,1,3} {2,5} {4} {6}; 1,000 copies of one slot give 1,000 rounds
    and 1,000 indices; a null column gathers zeros (tests/rounds_check.cpp)"""
    cc = _host_compiler()
    if cc is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "rounds_check")
    subprocess.run([cc, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "rounds_check.cpp")],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
