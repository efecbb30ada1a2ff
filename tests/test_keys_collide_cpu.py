"""The key directory's collision cases without a GPU: the hash model's inverter
round-trips, every builder of keys_cases.py holds what it claims under the
model at every table size the GPU tests reach, the audit reports nothing on a
sound table and exactly the broken rule on a corrupted one, and the cases can
tell a subtly wrong directory from a right one (the mutation check)."""
import copy
import os
import random
import re

import pytest

import keys_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_solve_round_trips():
    r = random.Random(5)
    for n in (8, 16, 17, 23, 24, 25, 32, 33, 40, 4097):
        for _ in range(40 if n == 4097 else 400):
            pre = 8 * r.randrange((n - 8) // 8 + 1)
            prefix, suffix, t = r.randbytes(pre), r.randbytes(n - 8 - pre), r.getrandbits(64)
            key = K.solve(prefix, suffix, t)
            assert len(key) == n and key[:pre] == prefix and key[pre + 8:] == suffix
            assert K.table_hash(key) == t, K.show(key)


def test_hash_model_words():
    """zero filled words, the length in the seed: a key and the key with a NUL appended differ"""
    assert len({K.table_hash(b""), K.table_hash(b"\0"), K.table_hash(b"\0" * 8), K.table_hash(b"\0" * 9)}) == 4
    assert K.key_words(b"abc") == (0x636261, 0) and K.key_words(b"x" * 9)[1] == 0x78
    assert K.key_words(b"0123456789abcdefXYZ") == K.key_words(b"0123456789abcdef")


def _claims(case, keys=None):
    keys, f = keys or case["keys"], case["facts"]
    assert len(set(keys)) == len(keys), case["name"]
    hs = [K.table_hash(k) for k in keys]
    if f["same"] == "hash":
        assert len(set(hs)) == 1, case["name"]
    for lg in K.LG_RANGE:
        assert len({K.home_of(h, lg) for h in hs}) == 1, (case["name"], lg)
        if f["home"]:
            assert K.home_of(hs[0], lg) == {"first": 0, "mid": 1 << (lg - 1), "last": (1 << lg) - 1}[f["home"]]
    if f["same"] in ("hash", "home_tag"):
        assert len({h & K.M32 for h in hs}) == 1, case["name"]
    if f["same"] == "home_tag":
        assert len({h >> 44 for h in hs}) == 1 and len({h >> 32 & 0xFFF for h in hs}) == len(hs), case["name"]
    if f["same"] == "home":
        assert len({h & K.M32 for h in hs}) == len(hs), case["name"]
    if f["prefix16"]:
        assert len({k[:16] for k in keys}) == 1 and len({len(k) for k in keys}) == 1 and len(keys[0]) > 16, case["name"]


def test_builders_hold_their_claims():
    a, b, c = K.cases_a(), K.cases_b(), K.cases_c()
    for case in a + b + c:
        _claims(case)
    assert [[len(k) for k in x["keys"]] for x in a] == [[8, 16, 24], [16] * 4, [0, 8, 16]]
    k8, k16, k24 = a[0]["keys"]
    assert k16.startswith(k8) and k24.startswith(k16)
    assert a[2]["keys"][0] == b"" and K.table_hash(a[2]["keys"][1]) == K.table_hash(b"")
    # b: every length, the difference at every place it can be put; four keys or more in a chain
    assert all(len(x["keys"]) >= 4 for x in b)
    w = b[0]["keys"]
    assert {len(k) for k in w} == {16} and len({k[:8] for k in w}) == 1 and len({k[8:] for k in w}) == len(w)
    w = b[1]["keys"]
    assert {len(k) for k in w} == {17} and len({k[:8] for k in w}) == 1 and len({k[16:] for k in w}) == len(w)
    tails = {}
    for x in b[2:]:
        n = len(x["keys"][0])
        diff = {i // 8 * 8 for k in x["keys"][1:] for i in range(n) if k[i] != x["keys"][0][i]}
        tails.setdefault(n, set()).add(tuple(sorted(diff)))
    full = lambda n: n // 8 * 8
    assert tails == {24: {(16,)}, 32: {(16,), (24,)}, 25: {(16,), (16, 24)}, 33: {(16,), (24,), (24, 32)},
                     4097: {(16,), (4088,), (4088, 4096)}}
    assert all(max(d) >= full(n) - 8 for n, ds in tails.items() for d in ds if len(d) > 1)
    assert {(x["facts"]["same"], x["facts"]["home"]) for x in c} == {(s, h) for s in ("home", "home_tag") for h in K.HOMES}
    assert all(len(x["keys"]) == K.CHAIN for x in c) and K.CHAIN > 256


def test_orders_and_launch_sizes():
    case = K.cases_b()[0]
    for keys in (case["keys"], K.cases_c()[0]["keys"]):
        seq = K.one_launch(keys)
        assert len(seq) > 257 and set(seq) == set(keys) and all(seq.count(k) >= 2 for k in keys)
        firsts = [seq.index(k) for k in keys]
        assert firsts != sorted(firsts)  # slots by first occurrence are not the keys' order
        assert all(seq[i] in keys[-len(K.REPEAT_AT) - 1:] for i in K.REPEAT_AT + (len(seq) - 1,))
    assert [len(l[0]) for l in K.deliver(case, "one key per launch")] == [1] * len(case["keys"])
    half = K.deliver(case, "half, lookup, all")
    assert [c for _, c in half] == [True, False, True] and set(half[0][0]) < set(half[1][0]) == set(case["keys"])
    rep = K.deliver(case, "launches repeated")
    assert len(rep) == 2 and rep[0] == rep[1]
    assert K.SCAN_TILE == 2048 and K.LAUNCH_EDGES == (1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049)
    e = K.cases_e()
    assert tuple(len(x["launches"][0][0]) for x in e) == K.LAUNCH_EDGES
    seen = set()
    for x in e:
        seq = x["launches"][0][0]
        assert not seen & set(seq)  # all new
        seen |= set(seq)
        n = len(seq)
        if n > 8:
            assert n // 8 <= n - len(set(seq)) <= n // 4
        edges = [g for g in (64, 256, K.SCAN_TILE) if g < n]
        assert len(x["pairs"]) == len(edges)
        for g, pair in zip(edges, x["pairs"]):
            assert [seq[g - 1], seq[g]] == pair
            _claims(dict(x, facts=dict(x["facts"], same="home_tag")), pair)


def test_growth_cases():
    f = K.cases_f()
    assert len(f) == 3
    for x in f[:2]:
        n, at = 0, []
        for keys, create, tcap in x["steps"]:
            assert create and len(set(keys)) == len(keys)
            n += len(keys)
            at.append((n, tcap))
        assert at == [(300, 1024), (512, 1024), (513, 2048), (1024, 2048), (1025, 4096)]
        _claims(x)
    steps = f[2]["steps"]
    assert [sum(len(k) for k in s[0]) for s in steps] == [65536, 1] and f[2]["bytes"] == (65536, 65537)
    assert len(set(steps[0][0])) == len(steps[0][0]) and max(len(k) for k in steps[0][0]) == 4097
    _claims(f[2])


# ---- the audit, audited ---------------------------------------------------------------------------
def _sound():
    d, want = K.ModelDir(), {}
    keys = [b"natural %d" % i for i in range(700)] + [b"", b"k" * 16, b"l" * 17, b"m" * 4097] + K.cases_c()[5]["keys"]
    assert d.intern(keys) == K.first_occurrence(keys, want)
    return d, list(want)


def test_audit_passes_a_sound_table():
    d, keys = _sound()
    T = d.read()
    assert T["tcap"] == 2048 and K.audit(keys, T) == []
    assert K.check_claim(K.cases_c()[5], {k: i for i, k in enumerate(keys)}, T) == []
    assert K.audit([], K.ModelDir().read()) == [("size", "tcap 0 lg 0 n 0, 0 entries read")]  # no table yet


def _first_empty_from(table, p):
    while table[p] != K.EMPTY:
        p = (p + 1) % len(table)
    return p


def _corrupt(rule, T, r):
    table, n = T["table"], T["n"]
    full = [p for p, e in enumerate(table) if e != K.EMPTY]
    p = r.choice(full)
    s = table[p] & K.M32
    if rule == "slot-once":  # a second entry of a slot, at the end of its own run
        table[_first_empty_from(table, K.home_of(T["khash"][s], T["lg"]))] = table[p]
    elif rule == "pending":
        table[p] |= K.PENDING
    elif rule == "tag":
        table[p] ^= 1 << 40
    elif rule == "hole":  # the last entry of a run, moved two entries on
        q = _first_empty_from(table, p)
        q2 = _first_empty_from(table, (q + 1) % len(table))
        table[q2], table[(q - 1) % len(table)] = table[(q - 1) % len(table)], K.EMPTY
    elif rule == "kw":
        T["kw"][s] = (T["kw"][s][0], T["kw"][s][1] ^ 1 << 56)
    elif rule == "kref":
        T["kref"][s] += 1
    elif rule == "khash":  # (the tag's bits left alone)
        T["khash"][s] ^= 1 << 33
    else:
        assert rule == "stray-entry"
        table[_first_empty_from(table, p)] = (table[p] >> 32) << 32 | n


@pytest.mark.parametrize("rule", [r for r in K.RULES if r != "size"])
def test_audit_names_the_broken_rule(rule):
    d, keys = _sound()
    for seed in range(5):
        T = copy.deepcopy(d.read())
        _corrupt(rule, T, random.Random(seed))
        got = K.audit(keys, T)
        assert got and {g[0] for g in got} == {rule}, (rule, seed, got[:3])


def test_audit_names_a_wrong_size():
    small = {"tcap": 512, "lg": 9, "n": 0, "blen": 0, "table": [K.EMPTY] * 512, "kref": [], "khash": [], "kw": []}
    assert [g[0] for g in K.audit([], small)] == ["size"]
    assert [g[0] for g in K.audit([], dict(small, tcap=1024, lg=11, table=[K.EMPTY] * 1024))] == ["size"]
    d = K.ModelDir()  # a sound table of 1024 entries with more than half of them taken
    d._grow = lambda need, grow=d._grow: grow(1)
    keys = [b"natural %d" % i for i in range(600)]
    d.intern(keys)
    T = d.read()
    assert T["tcap"] == 1024 and [g[0] for g in K.audit(keys, T)] == ["size"]


# ---- the mutation check -----------------------------------------------------------------------------
def _run(case, launches, fault, tcaps=None, bytes_after=None):
    """the launches on a model directory against the dict -> None, or what went wrong first"""
    d, want = K.ModelDir(fault), {}
    try:
        for i, (keys, create) in enumerate(launches):
            if d.intern(keys, create) != K.first_occurrence(keys, want, create):
                return "launch %d: slots differ from the dict's" % i
            if len(d.keys) != len(want):
                return "launch %d: %d keys, the dict has %d" % (i, len(d.keys), len(want))
            T = d.read()
            if tcaps and tcaps[i] and T["tcap"] != tcaps[i]:
                return "launch %d: table of %d, wanted %d" % (i, T["tcap"], tcaps[i])
            bad = K.audit(list(want), T)
            if bad:
                return "launch %d: audit %s" % (i, bad[0][0])
            bad = [b for c in K.claims_of(case) for b in K.check_claim(c, want, T)]
            if bad:
                return "launch %d: claim: %s" % (i, bad[0])
    except IndexError:
        return "a walk left the table"
    return None


def _growth_launches(case):
    """f. each step, then a lookup of every key so far"""
    out, tcaps, sofar = [], [], []
    for keys, create, tcap in case["steps"]:
        sofar = sofar + keys
        out += [(keys, create), (sofar, False)]
        tcaps += [tcap, tcap]
    return out, tcaps


def _every_run(fault, light=False):
    """(case name, order) -> outcome, for families a-d and f"""
    for case in K.cases_a() + K.cases_b() + K.cases_c():
        for order in K.ORDERS:
            if light and case["family"] == "c" and order == "one key per launch":
                continue  # (the chains a key at a time: the GPU's to run, slow in Python)
            yield case["name"], order, _run(case, K.deliver(case, order), fault)
    for case in K.cases_f():
        launches, tcaps = _growth_launches(case)
        yield case["name"], "growth", _run(case, launches, fault, tcaps)


def test_cases_pass_on_the_sound_model():
    bad = [(n, o, r) for n, o, r in _every_run(None, light=True) if r]
    assert not bad, bad[:3]
    for case in K.cases_e():
        assert _run(case, case["launches"], None) is None


# which case catches which fault (the first in case order, and how), as this test found them
CAUGHT_BY = {
    "first-tag": ("a: lengths 8, 16, 24, each starting with the one before", "one key per launch"),
    "join-any": ("a: lengths 8, 16, 24, each starting with the one before", "one launch"),
    "no-wrap": ("c: 300 keys, one home (last)", "one launch"),
    "stale-home": ("f: table 1024 -> 2048 -> 4096 under c: 300 keys, one home (last)", "growth"),
}


@pytest.mark.parametrize("fault", K.FAULTS)
def test_mutation_is_caught(fault):
    """One line of the model directory broken at a time; at least one case of
    families a-d or f then differs from the dict or fails the audit.  Found:

      first-tag   a (8/16/24 bytes, one hash), one key per launch: launch 1's
                  slot is the first key's.  Every a, b and one-tag c case
                  catches it in every order but "one launch" alone (nothing
                  final to probe); the chains of 300 different tags never do
      join-any    a (8/16/24 bytes, one hash), one launch: the keys of one tag
                  fold into one slot.  Every a, b and one-tag c case, in every
                  order but "one key per launch" (nothing PENDING to join)
      no-wrap     c, 300 keys at the last home, every order, and f over them:
                  the entries past the table's end are missing from the read
                  (audit: slot-once).  No case of a or b, and no chain at the
                  first or middle home, notices
      stale-home  f alone, at 512 -> 513 keys under either wrapped chain: the
                  rehash into 2048 entries leaves the chain around entry 1023,
                  far from its home 2047 (audit: hole).  No case of a-d grows
                  a table that holds keys, so none notices

    Each order of d and each family is needed by some fault."""
    name, order = CAUGHT_BY[fault]
    first = next(((n, o, r) for n, o, r in _every_run(fault, light=True) if r), None)
    assert first is not None, "no case notices " + fault
    assert first[:2] == (name, order), first


def test_entry_point_is_bound():
    from jylis_amd import _lib
    from jylis_amd.engine import Engine
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jylis_gpu.h")).read(), flags=re.S)
    assert re.search(r"\bjy_keys_table_read\s*\(", text)
    assert len(_lib.SIGNATURES["jy_keys_table_read"][1]) == 9 and callable(Engine.keys_table)
    assert hasattr(_lib.load(), "jy_keys_table_read")
