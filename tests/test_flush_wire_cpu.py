"""The host half of the wire-form flush (jy_*_flush_wire), without a GPU:
jylis_amd.repo.wire_to_table is the inverse of the table -> arrays marshalling
of Node.converge_table / Node.ujson_args for all five types, and the four
calls are declared in the header and bound in _lib.SIGNATURES."""
import os
import re

import numpy as np
import pytest

from helpers import assert_state_equal, random_history

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("jy_counter_flush_wire", "jy_treg_flush_wire", "jy_tlog_flush_wire", "jy_ujson_flush_wire")


def _marshal(ctype, table):
    """Node.converge_table's arrays for one batch table, captured instead of
    sent: (wire batch {name: array}, col_ids).  Replica ids get columns in
    order of first use, as a node's dictionary hands them out."""
    from jylis_amd.engine import WIRE_ARRAYS
    from jylis_amd.node import Node

    class Capture(Node):
        def __init__(self):  # no library, no GPU: only the marshalling runs
            self.ids, self.got = {}, None

        def replica_col(self, rid):
            return self.ids.setdefault(int(rid), len(self.ids))

        def counter_converge(self, ctype, kb, ko, cell_offs, col, val, sign=None):
            self.got = [kb, ko, cell_offs, np.zeros(len(col), np.uint8) if sign is None else sign, col, val]

        def treg_converge(self, *a):
            self.got = list(a)

        def tlog_converge(self, *a):
            self.got = list(a)

        def ujson_converge(self, *a):
            self.got = list(a)

        def __del__(self):
            pass

    cap = Capture()
    cap.converge_table(ctype, table)
    names = [name for name, _, _, _ in WIRE_ARRAYS[ctype]]
    assert len(names) == len(cap.got)
    col_ids = np.zeros(len(cap.ids), np.uint64)
    for rid, c in cap.ids.items():
        col_ids[c] = rid
    return dict(zip(names, cap.got)), col_ids


@pytest.mark.parametrize("ctype", [0, 1, 2, 3, 4])
def test_wire_to_table_inverts_the_converge_marshalling(oracle_mod, ctype):
    from jylis_amd.repo import wire_to_table
    batches = random_history(oracle_mod, ctype, seed=700 + ctype, nops=200)
    assert any(len(b["key_offs"]) > 1 for b in batches)
    for b in batches:
        arrays, col_ids = _marshal(ctype, b)
        assert_state_equal(ctype, b, wire_to_table(ctype, arrays, col_ids))


def test_wire_to_table_empty_batch():
    from helpers import join_rows
    from jylis_amd.engine import WIRE_ARRAYS
    from jylis_amd.repo import wire_to_table
    for ctype in range(5):
        arrays = {name: np.zeros(plus, dt) for name, dt, _, plus in WIRE_ARRAYS[ctype]}
        t = wire_to_table(ctype, arrays, np.zeros(0, np.uint64))
        want = join_rows(ctype, {})
        assert set(t) == set(want)
        for k in want:
            assert len(t[k]) == len(want[k]), k


def test_header_and_binding_declare_the_calls():
    from jylis_amd import _lib
    from jylis_amd.engine import WIRE_ARRAYS, WIRE_SIZES
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jylis_gpu.h")).read(), flags=re.S)
    for name in CALLS:
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
        assert m, f"{name} is not declared in include/jylis_gpu.h"
        assert name in _lib.SIGNATURES
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1])
    # engine, [type, col], capacities, outputs, sizes_out, mem
    for ctype, name in ((0, CALLS[0]), (2, CALLS[1]), (3, CALLS[2]), (4, CALLS[3])):
        head = 3 if ctype == 0 else 1
        assert len(_lib.SIGNATURES[name][1]) == head + len(WIRE_SIZES[ctype]) + len(WIRE_ARRAYS[ctype]) + 2
