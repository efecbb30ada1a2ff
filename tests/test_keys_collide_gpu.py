"""Constructed hash collisions against the device key directory (k_keys.hip).

The oracle is test_keys_gpu.py's first-occurrence dict.  keys_cases.py builds
keys that share a whole 64-bit table hash, or a table position and a tag, so
the probe's and the claim's "tag matches, key does not" branches, wrapped and
long chains and clustered rehashes run on every launch here -- natural keys
share a tag about once in 2^32 compares.  After every launch: the slots and
the key count are the dict's, the directory read back (Engine.keys_table)
passes keys_cases.audit against the exported key strings, and the collision
the case claims is read from the table itself (equal tags, one unbroken run
from the common home), so a wrong construction fails instead of passing.
tests/test_keys_collide_cpu.py holds the builders to their claims and shows
that these cases tell a subtly wrong directory from a right one."""
import numpy as np
import pytest

import keys_cases as K
from test_keys_gpu import first_occurrence

pytestmark = pytest.mark.gpu

A, B, C_ = K.cases_a(), K.cases_b(), K.cases_c()
_id = lambda case: case["name"]


class Driver:
    """one type's directory of an engine beside the dict, checked after every launch"""

    def __init__(self, eng, ctype, mem, case, order=""):
        self.eng, self.ctype, self.mem, self.case, self.table, self.i = eng, ctype, mem, case, {}, 0
        self.what = "%s [%s, %s, type %d]" % (case["name"], order, mem, ctype)

    def send(self, keys, create=True):
        if self.mem == "host":
            return self.eng.intern(self.ctype, keys) if create else self.eng.lookup(self.ctype, keys)
        import torch
        from jylis_amd.engine import encode_keys
        kb, ko = encode_keys(keys)
        return self.eng.intern_device(self.ctype, torch.from_numpy(kb.copy()).cuda(),
                                      torch.from_numpy(ko.astype(np.int64)).cuda(),
                                      create=create).cpu().numpy().view(np.uint32)

    def launch(self, keys, create=True, tcap=None):
        what = "%s launch %d" % (self.what, self.i)
        self.i += 1
        got = self.send(keys, create)
        want = first_occurrence(keys, self.table) if create else \
            np.array([self.table.get(k, K.NO_SLOT) for k in keys], np.uint32)
        for j in np.flatnonzero(got != want)[:4]:
            pytest.fail("%s: input %d, key %s: slot %d, the dict's %d" % (what, j, K.show(keys[j]), got[j], want[j]))
        assert self.eng.nkeys(self.ctype) == len(self.table), what
        return self.check(what, tcap)

    def check(self, what, tcap=None):
        T = self.eng.keys_table(self.ctype)
        names = self.eng.key_names(self.ctype, 0, T["n"])
        assert names == list(self.table), "%s: the exported keys are not the dict's in slot order" % what
        bad = K.audit(names, T)
        assert bad == [], "%s: audit: %s" % (what, "; ".join("%s (%s)" % b for b in bad[:4]))
        for c in K.claims_of(self.case):
            bad = K.check_claim(c, self.table, T)
            assert bad == [], "%s: claim of %s: %s" % (what, ", ".join(K.show(k) for k in c["keys"][:4]), "; ".join(bad))
        assert tcap is None or T["tcap"] == tcap, "%s: table of %d entries, wanted %d" % (what, T["tcap"], tcap)
        return T


def test_model_is_the_devices_hash(engine):
    """without this every other test here could pass on keys that do not collide"""
    from jylis_amd._lib import TLOG
    lens = [0, 1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 100, 1200, 4097]
    keys = [bytes((i * 31 + n) & 0xFF for i in range(n)) for n in lens] + [(b"%d:" % n + b"x" * n)[:n] for n in lens[1:]]
    d = Driver(engine, TLOG, "device", {"name": "natural keys", "keys": [], "facts": {}})
    T = d.launch(keys)
    for k in keys:
        got = int(T["khash"][d.table[k]])
        assert got == K.table_hash(k), "key %s: hash %#018x, the model's %#018x" % (K.show(k), got, K.table_hash(k))


@pytest.mark.parametrize("case", A + B + C_, ids=_id)
def test_collisions_device(engine, case):
    """a-d: every collision set in the four orders, each order in the directory of another type"""
    for ctype, order in enumerate(K.ORDERS):
        d = Driver(engine, ctype, "device", case, order)
        for keys, create in K.deliver(case, order):
            d.launch(keys, create)
        assert len(d.table) == len(case["keys"]), d.what


@pytest.mark.parametrize("case", A + B, ids=_id)
def test_collisions_host(engine, case):
    """a, b through the host calls: the host cache's misses reach the directory; run twice, the second from the cache"""
    for ctype, order in zip((4, 3, 2, 1), K.ORDERS):
        d = Driver(engine, ctype, "host", case, order)
        for rnd in range(2):
            d.what = "%s [%s, host, type %d, run %d]" % (case["name"], order, ctype, rnd)
            for keys, create in K.deliver(case, order):
                d.launch(keys, create)
        assert len(d.table) == len(case["keys"]), d.what


def test_launch_sizes(engine):
    """e: all-new launches around a wave, a workgroup and a scan tile, one after another into one directory"""
    from jylis_amd._lib import PNCOUNT
    cases = K.cases_e()
    d = Driver(engine, PNCOUNT, "device", cases[0])
    for case in cases:
        d.case, d.what = case, case["name"]
        (keys, create), = case["launches"]
        d.launch(keys, create)
        for pair in case["pairs"]:
            assert d.table[pair[0]] != d.table[pair[1]], "%s: %s and %s" % (d.what, K.show(pair[0]), K.show(pair[1]))
    T = d.check("e, after every launch")
    for case in cases:  # every pair still one home and one tag in the grown table
        for pair in K.claims_of(case):
            assert K.check_claim(pair, d.table, T) == [], case["name"]


@pytest.mark.parametrize("case", K.cases_f(), ids=_id)
def test_growth_at_the_edges(engine, case):
    """f: the table, the slot arrays and the key bytes grow exactly at their thresholds, under a cluster"""
    from jylis_amd._lib import TREG
    d = Driver(engine, TREG, "device", case, "growth")
    sofar = []
    for i, (keys, create, tcap) in enumerate(case["steps"]):
        T = d.launch(keys, create, tcap)
        sofar += keys
        d.launch(sofar, False, tcap)  # every earlier key is found again
        if "bytes" in case:
            assert T["blen"] == case["bytes"][i], d.what
    assert len(d.table) == len(sofar)


def test_length_limit(engine):
    """g: a key of 2^24 - 1 bytes is interned and found again; one of 2^24 bytes is refused and changes nothing"""
    from jylis_amd._lib import TLOG
    from jylis_amd.engine import EngineError
    d = Driver(engine, TLOG, "device", {"name": "g: the length limit", "keys": [], "facts": {}})
    longest = (np.arange(K.MAX_KEY, dtype=np.uint32) % 251).astype(np.uint8).tobytes()
    T = d.launch([b"before", longest, b"after"])
    assert int(T["kref"][1]) == len(b"before") << 24 | K.MAX_KEY
    d.launch([longest, b"after", longest[:-1]], False)
    d.launch([longest], True)
    with pytest.raises(EngineError, match="16 MiB"):
        d.send([b"new", longest + b"\0"])
    assert engine.nkeys(TLOG) == 3
    d.check("g: after the refusal")
    d.launch([b"new"])


def test_colliding_keys_address_their_own_state(engine):
    """one counter and one register per colliding key of every a and b set, written and read by key string"""
    from jylis_amd._lib import GCOUNT
    col = engine.replica_col(0xC0111DE)
    for n, case in enumerate(A + B):
        # counters: a cell per key, its value the key's own
        val = np.array([1000 * n + i + 1 for i in range(len(case["keys"]))], np.uint64)
        engine.counter_converge_keys(GCOUNT, case["keys"], np.full(len(val), col, np.uint16), val,
                                     cell_key=np.arange(len(val), dtype=np.uint32))
        found, got = engine.counter_get_keys(GCOUNT, case["keys"])
        for k, f, g, w in zip(case["keys"], found, got, val):
            assert f == 1 and g == w, "%s: counter of key %s reads %d, wrote %d" % (case["name"], K.show(k), g, w)
        # registers: each key SET to a value naming it
        vals = [b"value of %d/%d" % (n, i) for i in range(len(case["keys"]))]
        engine.treg_set_keys(case["keys"], np.arange(1, len(vals) + 1, dtype=np.uint64), vals)
        r = engine.treg_get_keys(case["keys"])
        vb, vo = bytes(np.asarray(r["val_bytes"], np.uint8)), np.asarray(r["val_offs"], np.int64)
        for i, k in enumerate(case["keys"]):
            got = vb[vo[i]:vo[i + 1]]
            assert r["found"][i] == 1 and got == vals[i] and r["ts"][i] == i + 1, \
                "%s: register of key %s reads %r, wrote %r" % (case["name"], K.show(k), got, vals[i])
    from jylis_amd._lib import TREG
    total = sum(len(c["keys"]) for c in A + B)
    assert engine.nkeys(GCOUNT) == engine.nkeys(TREG) == total
