"""Constructed hash collisions against the device key directory (k_keys.hip):
a model of its table hash with an inverter, an audit of a directory read
(Engine.keys_table), a linear-probing model of the directory, and the case
builders tests/test_keys_collide_cpu.py checks and
tests/test_keys_collide_gpu.py executes.  Pure Python: no GPU, no torch.

The table hash folds 8-byte little-endian words (zero filled past the key, as
jy_ld8u reads them) into a state seeded by the length; a fold is a xor, an odd
multiply and a xorshift, the finaliser two more of the same -- every step a
bijection of the 64-bit state.  So for any prefix of whole words, any suffix
and any 64-bit target, the one word between them can be solved: keys can be
given a whole hash, or a table position (the top lg bits) and a tag (the low
32 bits), at will.  What cannot be steered is a difference of fewer than 8
bytes: keys that share their first 16 bytes need a whole word in the tail, so
from 24 bytes up (17 to 23 bytes leave at most 2^56 candidates for a 45-bit
match)."""
import functools
import os
import random
import re
import struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jylis_amd", "csrc")


def _const(header, name):
    """`constexpr <type> name = <integer>;` of a csrc header"""
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, open(os.path.join(CSRC, header)).read())
    assert m, (header, name)
    return int(m.group(1))


SCAN_TILE = _const("jy_dscan.hpp", "kThreads") * _const("jy_dscan.hpp", "kPer")  # jydscan::kTileItems
M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
C1, C2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
C1_INV, C2_INV = pow(C1, -1, 1 << 64), pow(C2, -1, 1 << 64)
EMPTY = M64
PENDING = 0x80000000
NO_SLOT = 0xFFFFFFFF
MAX_KEY = (1 << 24) - 1  # JY_LR_LEN_MASK
LAUNCH_EDGES = (1, 63, 64, 65, 255, 256, 257, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1)
REPEAT_AT = (0, 63, 64, 255, 256, 257)  # and the last index
HOMES = {"first": 0x00000, "mid": 0x80000, "last": 0xFFFFF}  # the hash's top 20 bits: one home at every lg <= 20
LG_RANGE = (10, 11, 12, 13)


# ---- the hash and its inverse -------------------------------------------------------------------
def _words(b):
    """little-endian 8-byte words of b, the last zero filled"""
    pad = b + b"\0" * (-len(b) % 8)
    return struct.unpack("<%dQ" % (len(pad) // 8), pad)


def _seed(n):
    return ((n * 0x9E3779B97F4A7C15) ^ 0xCBF29CE484222325) & M64


def _mix(h, w):
    h = ((h ^ w) * C1) & M64
    return h ^ (h >> 31)


def _unshift(h, k):
    y = h
    for _ in range(64 // k + 1):
        y = h ^ (y >> k)
    return y


def _unmix(h, w):
    """the state before word w folded in to give h"""
    return ((_unshift(h, 31) * C1_INV) & M64) ^ w


def _final(h):
    h ^= h >> 30
    h = (h * C1) & M64
    h ^= h >> 27
    h = (h * C2) & M64
    return h ^ (h >> 31)


def _unfinal(t):
    h = _unshift(t, 31)
    h = _unshift((h * C2_INV) & M64, 27)
    return _unshift((h * C1_INV) & M64, 30)


def _table_hash(key):
    h = _seed(len(key))
    for w in (_words(key) or (0,)):  # the empty key folds one zero word
        h = ((h ^ w) * C1) & M64
        h ^= h >> 31
    return _final(h)


_cached_hash = functools.lru_cache(maxsize=1 << 16)(_table_hash)


def table_hash(key):
    """k_keys.hip's table_hash of the key bytes"""
    return _cached_hash(bytes(key))


def solve(prefix, suffix, target):
    """prefix + w + suffix, w the one 8-byte word that makes the key hash to target"""
    assert len(prefix) % 8 == 0
    n = len(prefix) + 8 + len(suffix)
    h = _seed(n)
    for w in _words(prefix):
        h = _mix(h, w)
    t = _unfinal(target)
    for w in reversed(_words(suffix)):
        t = _unmix(t, w)
    w = h ^ ((_unshift(t, 31) * C1_INV) & M64)
    return prefix + struct.pack("<Q", w) + suffix


def home_of(h, lg):
    return h >> (64 - lg)


def key_words(key):
    """the directory's kw of a key: its bytes 0..7 and 8..15, zero filled"""
    return struct.unpack("<2Q", (key[:16] + b"\0" * 16)[:16])


def show(key):
    """a key for a failure message: its length and (the start of) its bytes in hex"""
    return "%d B %s%s" % (len(key), key[:40].hex(), "..." if len(key) > 40 else "")


# ---- the audit of a directory read ------------------------------------------------------------
RULES = ("slot-once", "stray-entry", "pending", "tag", "khash", "kref", "kw", "hole", "size")


def _ints(x):
    x = x.tolist() if hasattr(x, "tolist") else list(x)
    return [int(v) for r in x for v in r] if x and isinstance(x[0], (list, tuple)) else [int(v) for v in x]


def audit(keys, T):
    """keys: the key bytes in slot order (jy_keys_export); T: Engine.keys_table's
    dict (tcap, lg, n, blen, table, kref, khash, kw) -> [(rule, what)], empty
    for a sound directory"""
    out = []
    tcap, lg, n = int(T["tcap"]), int(T["lg"]), int(T["n"])
    table, kref, khash, kw = _ints(T["table"]), _ints(T["kref"]), _ints(T["khash"]), _ints(T["kw"])
    if tcap != 1 << lg or tcap < 1024 or tcap < 2 * n or len(table) != tcap:
        out.append(("size", "tcap %d lg %d n %d, %d entries read" % (tcap, lg, n, len(table))))
    if not (len(keys) == len(kref) == len(khash) == n and len(kw) == 2 * n):
        out.append(("size", "%d keys, kref %d khash %d kw %d for n %d" % (len(keys), len(kref), len(khash), len(kw), n)))
        return out
    if int(T["blen"]) != sum(len(k) for k in keys):
        out.append(("kref", "blen %d, the keys hold %d bytes" % (int(T["blen"]), sum(len(k) for k in keys))))
    # entries behind p with no EMPTY one among them (all of them in a full table)
    run = [0] * len(table)
    if EMPTY in table:
        p0 = table.index(EMPTY)
        r = 0
        for d in range(1, len(table) + 1):
            p = (p0 + d) % len(table)
            run[p] = r
            r = 0 if table[p] == EMPTY else r + 1
    else:
        run = [len(table)] * len(table)
    seen = [0] * n
    for p, e in enumerate(table):
        if e == EMPTY:
            continue
        s = e & M32
        if s & PENDING:
            out.append(("pending", "entry %d = %#018x" % (p, e)))
            s &= PENDING - 1
        if s >= n:
            out.append(("stray-entry", "entry %d = %#018x names slot %d of %d" % (p, e, s, n)))
            continue
        seen[s] += 1
        if e >> 32 != khash[s] & M32:
            out.append(("tag", "entry %d tag %#010x, slot %d hash %#018x, key %s" % (p, e >> 32, s, khash[s], show(keys[s]))))
        if lg and (p - home_of(khash[s], lg)) % tcap > run[p]:
            out.append(("hole", "entry %d of slot %d, home %d, %d entries behind it, key %s" %
                        (p, s, home_of(khash[s], lg), run[p], show(keys[s]))))
    at = 0
    for s, k in enumerate(keys):
        if seen[s] != 1:
            out.append(("slot-once", "slot %d in %d entries, key %s" % (s, seen[s], show(k))))
        if khash[s] != table_hash(k):
            out.append(("khash", "slot %d hash %#018x, the model's %#018x, key %s" % (s, khash[s], table_hash(k), show(k))))
        if kref[s] != (at << 24 | len(k)):
            out.append(("kref", "slot %d kref %d << 24 | %d, wanted %d << 24 | %d, key %s" %
                        (s, kref[s] >> 24, kref[s] & MAX_KEY, at, len(k), show(k))))
        if (kw[2 * s], kw[2 * s + 1]) != key_words(k):
            out.append(("kw", "slot %d kw %#018x %#018x, key %s" % (s, kw[2 * s], kw[2 * s + 1], show(k))))
        at += len(k)
    return out


def check_claim(case, slot_of, T):
    """the collision a case claims, read back from the directory: the case's
    keys interned so far (slot_of: key -> slot) have one home -- one hash, or
    one tag, where the case says so -- and their entries sit in one unbroken
    run from that home (exactly the run, when the directory holds nothing
    else), across the table's end where the case wraps -> [what is wrong]"""
    keys = [k for k in case["keys"] if k in slot_of]
    if not keys:
        return []
    out, facts = [], case["facts"]
    tcap, lg = int(T["tcap"]), int(T["lg"])
    table, khash = _ints(T["table"]), _ints(T["khash"])
    place = {e & (PENDING - 1): p for p, e in enumerate(table) if e != EMPTY}
    slots = [slot_of[k] for k in keys]
    if len(set(slots)) != len(keys):
        return ["keys share a slot: %s" % sorted(slots)]
    homes = {home_of(khash[s], lg) for s in slots}
    if len(homes) != 1:
        return ["%d homes %s" % (len(homes), sorted(homes)[:8])]
    home = homes.pop()
    if facts["same"] == "hash" and len({khash[s] for s in slots}) != 1:
        out.append("hashes differ")
    if facts["same"] in ("hash", "home_tag") and len({table[place[s]] >> 32 for s in slots}) != 1:
        out.append("tags differ")
    if facts["same"] == "home" and len({table[place[s]] >> 32 for s in slots}) != len(slots):
        out.append("tags repeat")
    if facts.get("home") and home != {"first": 0, "mid": tcap // 2, "last": tcap - 1}[facts["home"]]:
        out.append("home %d of %d is not the %s" % (home, tcap, facts["home"]))
    dist = sorted((place[s] - home) % tcap for s in slots)
    holes = [d for d in range(dist[-1] + 1) if table[(home + d) % tcap] == EMPTY]
    if holes:
        out.append("an EMPTY entry %d past home %d inside the run" % (holes[0], home))
    if int(T["n"]) == len(keys) and dist != list(range(len(keys))):
        out.append("run from home %d at distances %s" % (home, dist[:8]))
    if facts.get("home") == "last" and len(keys) > 1 and not any(place[s] < home for s in slots):
        out.append("the run does not wrap")
    return out


# ---- a linear-probing model of the directory -----------------------------------------------
FAULTS = ("first-tag", "join-any", "no-wrap", "stale-home")


class ModelDir:
    """The directory's table, a launch at a time, in plain Python: probe every
    key against the final entries, grow, claim in input order (PENDING
    entries carry the input index, an equal key joins), slots by first
    occurrence, commit.  `fault` breaks one line of it (the mutation check):
      first-tag   the probe stops at the first entry with the key's tag
      join-any    a claim joins any PENDING entry with its tag
      no-wrap     the walk goes p + 1 without the mask
      stale-home  a rehash places slots by the table's old lg"""

    def __init__(self, fault=None):
        assert fault is None or fault in FAULTS
        self.fault, self.tcap, self.lg, self.table, self.keys, self.khash = fault, 0, 0, [], [], []

    def _next(self, p):
        return p + 1 if self.fault == "no-wrap" else (p + 1) & (self.tcap - 1)

    def _grow(self, need):
        want, lg = 1024, 10
        while want < 2 * need:
            want, lg = want << 1, lg + 1
        if self.table and want <= self.tcap:
            return
        home_lg = self.lg if self.fault == "stale-home" and self.lg else lg
        self.tcap, self.lg = want, lg
        self.table = [EMPTY] * (2 * want)  # (the upper half: where a walk without the wrap lands)
        for s, h in enumerate(self.khash):
            p = home_of(h, home_lg)
            while self.table[p] != EMPTY:
                p = self._next(p)
            self.table[p] = (h & M32) << 32 | s

    def _probe(self, key, h):
        p = home_of(h, self.lg)
        while self.table[p] != EMPTY:
            e = self.table[p]
            if e >> 32 == h & M32 and not e & PENDING and (self.fault == "first-tag" or self.keys[e & M32] == key):
                return e & M32
            p = self._next(p)
        return NO_SLOT

    def intern(self, keys, create=True):
        self._grow(max(len(self.keys), 1))
        hs = [table_hash(k) for k in keys]
        res = [self._probe(k, h) for k, h in zip(keys, hs)]
        miss = [i for i, s in enumerate(res) if s == NO_SLOT]
        if not create or not miss:
            return res
        if any(len(keys[i]) > MAX_KEY for i in miss):
            raise ValueError("key longer than 16 MiB")
        self._grow(len(self.keys) + len(miss))
        owner, pos = {}, {}
        for i in miss:
            p = home_of(hs[i], self.lg)
            while True:
                e = self.table[p]
                if e == EMPTY:
                    self.table[p] = (hs[i] & M32) << 32 | PENDING | i
                    owner[i], pos[i] = i, p
                    break
                if e >> 32 == hs[i] & M32 and e & PENDING:
                    j = e & (PENDING - 1)
                    if self.fault == "join-any" or keys[j] == keys[i]:
                        owner[i] = j
                        break
                p = self._next(p)
        for i in miss:
            if owner[i] == i:  # (claims land in input order here: the claimer is the first occurrence)
                self.table[pos[i]] = (hs[i] & M32) << 32 | len(self.keys)
                self.keys.append(keys[i])
                self.khash.append(hs[i])
            res[i] = self.table[pos[owner[i]]] & M32
        return res

    def read(self):
        """what Engine.keys_table returns"""
        kref, at = [], 0
        for k in self.keys:
            kref.append(at << 24 | len(k))
            at += len(k)
        return {"tcap": self.tcap, "lg": self.lg, "n": len(self.keys), "blen": at, "table": self.table[:self.tcap],
                "kref": kref, "khash": list(self.khash), "kw": [key_words(k) for k in self.keys]}


def first_occurrence(keys, table, create=True):
    """the oracle: a dict handing out dense slots in order of first occurrence"""
    out = []
    for k in keys:
        if create and k not in table:
            table[k] = len(table)
        out.append(table.get(k, NO_SLOT))
    return out


# ---- the cases ------------------------------------------------------------------------------------
def _rng(name):
    return random.Random("keys_cases:" + name)


def _case(family, name, keys, same, home=None, prefix16=False):
    return {"family": family, "name": "%s: %s" % (family, name), "keys": keys,
            "facts": {"same": same, "home": home, "prefix16": prefix16}}


def _target(top20, mid12, tag):
    """a hash with its home (top 20 bits), bits 32..43 and tag given; bits 44.. below the top 20: none left"""
    return top20 << 44 | (mid12 & 0xFFF) << 32 | tag


def cases_a():
    """a. one 64-bit hash, different keys"""
    r = _rng("a")
    t = r.getrandbits(64)
    k8 = solve(b"", b"", t)
    k16 = solve(k8, b"", t)
    k24 = solve(k16, b"", t)
    out = [_case("a", "lengths 8, 16, 24, each starting with the one before", [k8, k16, k24], "hash")]
    t = r.getrandbits(64)
    pair = [solve(struct.pack("<Q", r.getrandbits(64)), b"", t) for _ in range(4)]
    assert len({k[:8] for k in pair}) == len({k[8:] for k in pair}) == 4
    out.append(_case("a", "length 16, both words different", pair, "hash"))
    t = table_hash(b"")
    out.append(_case("a", "the empty key's hash on keys of 0, 8 and 16 bytes",
                     [b"", solve(b"", b"", t), solve(b"prefix:0", b"", t)], "hash"))
    return out


TAIL_LENGTHS = (24, 32, 25, 33, 4097)
PER_CHAIN = 5


def cases_b():
    """b. one home and one tag, hashes differing in bits 32..43 only"""
    r = _rng("b")
    out = []

    def targets(n):
        top, tag = r.getrandbits(20), r.getrandbits(32)
        return [_target(top, i + 1, tag) for i in range(n)]

    w0 = b"samew0:b"
    out.append(_case("b", "length 16, one w0, other w1", [solve(w0, b"", t) for t in targets(PER_CHAIN)], "home_tag"))
    # 17 bytes: one w0 and one length; the tail is one byte, too little to steer, so w1 differs too
    out.append(_case("b", "length 17, one w0, other w1 and last byte",
                     [solve(w0, bytes([0x41 + i]), t) for i, t in enumerate(targets(PER_CHAIN))], "home_tag"))
    head = b"sixteen bytes:b:"
    for n in TAIL_LENGTHS:
        fill = bytes((7 * i + n) & 0xFF for i in range(n))
        full = n // 8 * 8  # the bytes in whole words
        places = {"the word at 16": (16, False)}
        if full - 8 > 16:
            places["the last whole word"] = (full - 8, False)
        if n % 8:
            places["the last whole word and the last byte"] = (full - 8, True)
        for what, (at, last) in places.items():
            keys = []
            for i, t in enumerate(targets(PER_CHAIN)):
                suffix = fill[at + 8:n - 1] + bytes([0x61 + i]) if last else fill[at + 8:]
                keys.append(solve(head + fill[16:at], suffix, t))
            assert all(len(k) == n and k[:16] == head for k in keys)
            out.append(_case("b", "length %d, 16 bytes shared, other in %s" % (n, what), keys, "home_tag", prefix16=True))
    return out


CHAIN = 300


def cases_c():
    """c. chains longer than a workgroup: one home; one home and one tag; at the table's start, middle and end"""
    r = _rng("c")
    out = []
    for where, top in HOMES.items():
        tags = r.sample(range(1 << 32), CHAIN)
        keys = [solve(b"", b"c%d" % i, _target(top, r.getrandbits(12), tags[i])) for i in range(CHAIN)]
        out.append(_case("c", "%d keys, one home (%s)" % (CHAIN, where), keys, "home", home=where))
        tag = r.getrandbits(32)
        keys = [solve(b"", b"", _target(top, i, tag)) for i in range(CHAIN)]
        out.append(_case("c", "%d keys, one home (%s) and one tag" % (CHAIN, where), keys, "home_tag", home=where))
    return out


ORDERS = ("one launch", "one key per launch", "half, lookup, all", "launches repeated")


def one_launch(keys):
    """every key at least twice in one launch, the later keys first at the
    lane, wave and workgroup edges (input indices 0, 63, 64, 255, 256, 257 and
    the last)"""
    k = len(keys)
    n = max(3 * k, 320)
    seq = [keys[i % k] for i in range(n)]
    for j, at in enumerate(REPEAT_AT + (n - 1,)):
        seq[at] = keys[-1 - j % k]
    assert all(seq.count(x) >= 2 for x in keys)
    return seq


def deliver(case, order):
    """d. a collision set as launches: [(keys, create)]"""
    keys = case["keys"]
    if order == "one launch":
        return [(one_launch(keys), True)]
    if order == "one key per launch":
        return [([k], True) for k in keys]
    if order == "half, lookup, all":
        return [(keys[::2], True), (keys, False), (keys, True)]
    assert order == "launches repeated"
    return [(one_launch(keys), True)] * 2


def cases_e():
    """e. all-new batches of every size around a wave, a workgroup and a scan
    tile: a quarter of each repeats an earlier key of the batch, and a pair of
    keys with one home and one tag sits across each edge inside the batch"""
    r = _rng("e")
    out = []
    for n in LAUNCH_EDGES:
        seq, pairs = [None] * n, []
        for edge in (64, 256, SCAN_TILE):
            if edge < n:
                top, tag = r.getrandbits(20), r.getrandbits(32)
                pair = [solve(b"e%07d" % n, b"%d" % edge, _target(top, i, tag)) for i in range(2)]
                seq[edge - 1], seq[edge] = pair
                pairs.append(pair)
        free = [i for i in range(n) if seq[i] is None]
        for j, i in enumerate(free):
            seq[i] = b"launch %d key %d" % (n, j)
        for i in r.sample(free[1:], len(free) // 4):  # a repeat of an earlier entry
            seq[i] = seq[r.randrange(i)]
        c = _case("e", "a launch of %d" % n, [k for p in pairs for k in p], "home_tag")
        c["launches"], c["pairs"] = [(seq, True)], pairs
        out.append(c)
    return out


def fillers(tag, n):
    return [b"filler %s %d" % (tag, i) for i in range(n)]


def cases_f():
    """f. growth at the edges: steps of (keys, create) with the table size wanted after each (None: any)"""
    out = []
    for chain in (c for c in cases_c() if c["facts"]["home"] == "last"):
        steps = [(chain["keys"], True, 1024), (fillers(b"f512", 512 - CHAIN), True, 1024), ([b"the 513th"], True, 2048)]
        steps.append((fillers(b"f1024", 1024 - 513), True, 2048))
        steps.append(([b"the 1025th"], True, 4096))
        c = _case("f", "table 1024 -> 2048 -> 4096 under " + chain["name"], chain["keys"], chain["facts"]["same"], home="last")
        c["steps"] = steps
        out.append(c)
    long_keys = next(c for c in cases_b() if c["name"].endswith("length 4097, 16 bytes shared, other in the last whole word"))
    room = 65536 - sum(len(k) for k in long_keys["keys"])
    fill = [b"%04d" % i + b"x" * 60 for i in range(room // 64)]
    fill[-1] += b"y" * (room - 64 * len(fill))
    c = _case("f", "key bytes 65536, then one more, under " + long_keys["name"], long_keys["keys"], "home_tag", prefix16=True)
    c["steps"] = [(long_keys["keys"] + fill, True, None), ([b"!"], True, None)]
    c["bytes"] = (65536, 65537)
    out.append(c)
    return out


def claims_of(case):
    """the collision sets a case claims, each as a case of its own for check_claim"""
    return [dict(case, keys=p) for p in case["pairs"]] if "pairs" in case else [case]
