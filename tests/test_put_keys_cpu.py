"""Keyed batch writes, the parts that need no GPU: the value handles'
formula, the cut of a TLOG batch into units and rounds, and the boundary's
declarations."""
import itertools
import os
import re

import numpy as np

import put_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "jylis_gpu.h")


def _header():
    return open(HEADER).read()


def test_pack_ref_follows_the_headers_formula():
    """pre = first 8 bytes big-endian, zero padded; lr = len, or
    arena_offset << 24 | len with long values on 8-byte granules, in call
    order, from the rounded-up arena end"""
    rng = np.random.default_rng(5)
    lens = [0, 1, 7, 8, 9, 15, 16, 17, 255, 70000, 3, 12]
    vals = [bytes(rng.integers(0, 256, n, dtype=np.uint8)) for n in lens]
    for arena_len in (0, 5, 8, 1001):
        pre, lr, tail = P.pack_ref(vals, arena_len)
        at = -(-arena_len // 8) * 8
        assert tail[:at - arena_len] == b"\0" * (at - arena_len)
        for v, p, l in zip(vals, pre, lr):
            want = 0
            for j in range(8):
                want = (want << 8) | (v[j] if j < len(v) else 0)
            assert int(p) == want
            if len(v) <= 8:
                assert int(l) == len(v)
            else:
                assert int(l) == (at << 24) | len(v) and at % 8 == 0
                o = at - arena_len
                assert tail[o:o + len(v)] == v
                at += -(-len(v) // 8) * 8
        assert len(tail) == at - arena_len
    text = re.sub(r"\s*\n \* ?", " ", _header())
    assert "arena_offset << 24 | len" in text and "8-byte granules" in text


def test_units_and_rounds_by_hand():
    I, T, C = P.INS, P.TRIM, P.CLR
    # key 0: INS INS | TRIM | INS ; key 1: CLR | INS   (call order interleaved)
    ops = [I, C, I, T, I, I]
    slots = [0, 1, 0, 0, 1, 0]
    assert P.units_ref(ops, slots) == [(0, 0, [0, 2]), (0, 1, [1]), (1, 0, [3]), (1, 1, [4]), (2, 0, [5])]
    # a stretch longer than a unit is cut: 130 INS to one key take 3 rounds
    u = P.units_ref([I] * 130 + [I], [7] * 130 + [9])
    assert [(r, s, len(ix)) for r, s, ix in u] == [(0, 7, 64), (0, 9, 1), (1, 7, 64), (2, 7, 2)]
    # no repeated key: one round, one command per unit
    u = P.units_ref([I, T, C, I], [3, 1, 2, 0])
    assert [r for r, _, _ in u] == [0] * 4 and sorted(i for _, _, ix in u for i in ix) == [0, 1, 2, 3]
    assert -(-10000 // P.UNIT_MAX) == 157


def test_unit_of_one_is_the_host_round_rule():
    """with unit_max = 1 a command's round is the number of earlier commands
    that name its slot (JyRounds' rule, jy_rounds.hpp), whatever the ops are;
    a round lists its commands in slot order, each command once"""
    rng = np.random.default_rng(11)
    for trial in range(60):
        n, nslots = int(rng.integers(1, 201)), int(rng.integers(1, 9))
        slots = rng.integers(0, nslots, n).tolist()
        ops = rng.integers(0, 4, n).tolist()
        seen, want = {}, []
        for i, s in enumerate(slots):
            want.append((seen.get(s, 0), s, [i]))
            seen[s] = seen.get(s, 0) + 1
        want.sort(key=lambda u: (u[0], u[1]))
        assert P.units_ref(ops, slots, 1) == want, trial


def test_rounds_equal_command_order_brute_force():
    """every command string of length <= 6 over {INS, TRIM, CLR} on two keys:
    applying the units round by round leaves what one command at a time does.
    Timestamps and values come from the position, so strings hold duplicates,
    timestamp ties and INS below a cutoff; units of at most 2 and of at most 64."""
    sym = [(op, k) for op in (P.INS, P.TRIM, P.CLR) for k in (0, 1)]
    checked = 0
    for n in range(1, 7):
        for s in itertools.product(sym, repeat=n):
            cmds, slots = [], []
            for i, (op, k) in enumerate(s):
                if op == P.INS:
                    cmds.append((P.INS, (i * 5) % 3, b"v%d" % (i % 2)))
                elif op == P.TRIM:
                    cmds.append((P.TRIM, 1 + i % 2))
                else:
                    cmds.append((P.CLR,))
                slots.append(k)
            want = P.apply_in_order(cmds, slots)
            for unit_max in (2, 64):
                got, rounds = P.apply_in_rounds(cmds, slots, unit_max)
                assert got == want, (s, unit_max)
                assert rounds <= n
            checked += 1
    assert checked == sum(6 ** n for n in range(1, 7))


def _params(name):
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text)
    assert m, f"{name} is not declared in include/jylis_gpu.h"
    return [p.strip() for p in m.group(1).split(",")]


def test_declarations_of_the_four_calls():
    from jylis_amd import _lib
    for name, n in (("jy_values_pack_mem", 9), ("jy_counter_write_keys", 9), ("jy_treg_set_keys", 8),
                    ("jy_tlog_write_keys", 10)):
        ps = _params(name)
        assert len(ps) == n, (name, ps)
        assert ps[0].startswith("jy_engine*") and ps[-1].startswith("int32_t")
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.I32 and len(args) == n


def test_header_text_allows_repeats_in_device_batches():
    text = re.sub(r"\s*\n \* ?", " ", _header())
    assert "one command per key" not in text
    assert "one entry per key" not in text
    assert "keys may repeat any number of times" in text
