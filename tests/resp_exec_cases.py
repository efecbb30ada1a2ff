"""The request buffers tests/test_resp_exec_cpu.py and tests/test_resp_exec_gpu.py
share (RESP execute: jy_resp_exec, k_resp_out.hip).  The CPU file asserts what
they cover, the GPU file executes them."""
import os
import re

from resp_in_ref import request as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jylis_amd", "csrc")


def _const(header, name):
    """`constexpr <type> name = <integer>;` of a csrc header"""
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, open(os.path.join(CSRC, header)).read())
    assert m, (header, name)
    return int(m.group(1))


# the assembly's own constants: the device scan works in tiles of kTileItems
# = kThreads * kPer items (jy_dscan.hpp, behind jy_scan_u64), the gather stages at
# most kStage offsets of a workgroup's slice in LDS (jy_wire.hpp)
SCAN_TILE = _const("jy_dscan.hpp", "kThreads") * _const("jy_dscan.hpp", "kPer")
GATHER_STAGE = _const("jy_wire.hpp", "kStage")
BOUNDARY_COUNTS = tuple(c + d for c in (GATHER_STAGE, SCAN_TILE) for d in (-1, 0, 1))


# ---- 2: rows out of command order ----
def permutation():
    """GET a, SET a, GET a beside SET b, GET b: the rows sort by (phase, kind), so
    row_cmd is no identity, and the second GET a follows a write in its own connection"""
    return [R("TREG", "GET", "a") + R("TREG", "SET", "a", "fresh", 7) + R("TREG", "GET", "a"),
            R("TREG", "SET", "b", "other", 9) + R("TREG", "GET", "b")]


# ---- 3: connections without a complete command ----
W = R("GCOUNT", "INC", "e", 1)  # a connection with one complete command
PART = R("TREG", "SET", "half", "value", 1)[:-3]  # only an incomplete command: used 0, not closed
BAD = b"PING\r\n"  # malformed from byte 0: closed, nothing answered


def empty_ranges():
    """name -> connection buffers"""
    return {
        "first": [b"", W, W],
        "last": [W, W, b""],
        "middle": [W, b"", b"", W],
        "all": [b"", b"", b""],
        "none": [],
        "incomplete": [W, PART, W],
        "malformed": [W, BAD, W],
        "mixed": [b"", W, PART, BAD, b"", W, b""],
    }


# ---- 5: command counts around the assembly's constants ----
DIGIT_VALUES = [10**(d - 1) + d for d in range(1, 20)] + [2**64 - 1]  # 1 .. 20 digits


def ok_heartbeat(n):
    """n writes over three connections: every reply is +OK, 5 bytes, so reply k
    starts at residue 5 k mod 8"""
    cut = (n // 3, n // 3 + n // 2)
    one = [R("GCOUNT", "INC", "w%d" % (i % 11), 1) for i in range(n)]
    return [b"".join(one[:cut[0]]), b"".join(one[cut[0]:cut[1]]), b"".join(one[cut[1]:])]


def digits_setup():
    return [b"".join(R("GCOUNT", "INC", "d%d" % i, v) for i, v in enumerate(DIGIT_VALUES))]


def digits_heartbeat(n):
    """n GCOUNT GETs of values of 1 .. 20 digits over three connections -> (buffers, expected replies)"""
    cut = (n // 3, n // 3 + n // 2)
    one = [R("GCOUNT", "GET", "d%d" % (i % 20)) for i in range(n)]
    rep = [b":%d\r\n" % DIGIT_VALUES[i % 20] for i in range(n)]
    return ([b"".join(one[:cut[0]]), b"".join(one[cut[0]:cut[1]]), b"".join(one[cut[1]:])],
            [b"".join(rep[:cut[0]]), b"".join(rep[cut[0]:cut[1]]), b"".join(rep[cut[1]:])])
