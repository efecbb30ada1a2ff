"""Case generators for the UJSON converge sweeps (test_ujson_sweep_cpu.py checks
them against the oracle alone, test_ujson_sweep_gpu.py runs them through the
engine) and the invariant check over a raw Engine.ujson_read.  Plain Python
and numpy.

Replica column c carries replica id c + 1 (the GPU test registers the ids in
that order), so the oracle's order by id is the engine's order by packed dot.

A delta is {"el": [(col, seq, elem)], "vv": [(col, n)], "cl": [(col, seq)]},
its items in the order they are sent.  A case is a dict:
  key        the document
  steps      the deltas that build its state, one converge each
  probe      the delta under test
  expect     the outcome it was built to reach (a literal, per sweep below)
  path       what it aims at inside the kernel (a label, not observable)
  malformed  the engine must skip the probe
  skips      what the probe adds to Engine.skipped()
and, where a sweep needs them: dot (the dot `expect` speaks of), what
("element" / "cloud"), col, ctx_free (the document holds an element outside
its context on purpose), repeat (the probe is sent this many times in the
batch), hole (the probe's slot is JY_NO_SLOT), stats (declared ujson_stats
differences of the probe's converge).
Cases of one sweep are separate documents of one batch: batches() lays the
i-th steps of all cases into converge i, the probes into the last."""
import numpy as np

# the kernel constants the cases are built around
TILE = 256        # k_ujson.hip:73,85 JY_UJ_THREADS -> kTile, one item per thread
DOC_TILE = 256    # k_ujson.hip:86 kDocTile
LONG_SEG = 512    # k_ujson.hip:817 kLongSeg = 2 * kTile
LDS_DOCS = 1023   # k_ujson.hip:87 kLdsDocs
WIN_WIDE = 8      # k_ujson.hip:1229,1249,1261 Win<8>
WIN_NARROW = 4    # k_ujson.hip:1230,1250,1386 Win<4>
WAVE = 64         # k_ujson.hip:145 wave_lbs' 64-ary probes
TRIM_SPAN = 256   # jy_internal.hpp:456 kTrimSpan
JOB_BUF = 128     # k_ujson.hip:493 JobBuf::kCap
MAX_R = 64        # k_ujson.hip:579 kMaxR: the in-place layout's widest vv
SEQ_BITS = 48     # jy_internal.hpp:21 JY_DOT_SEQ_BITS
# The largest seq the packed dot (48 bits), the table form (uint64) and the
# oracle (uint64) all carry: the packed dot's is the limit.
SEQ_MAX = (1 << SEQ_BITS) - 1
NO_SLOT = 0xFFFFFFFF  # _lib.py:14 JY_NO_SLOT


def ids(R):
    return list(range(1, R + 1))


def delta(els=None, vv=None, cl=None):
    """a well-formed delta from {(c, q): e}, {c: n}, {(c, q)}"""
    return {"el": [(c, q, e) for (c, q), e in sorted((els or {}).items())],
            "vv": sorted((vv or {}).items()), "cl": sorted(cl or ())}


def case(key, steps, probe, expect, path, malformed=False, **kw):
    c = dict(key=key, steps=steps, probe=probe, expect=expect, path=path, malformed=malformed,
             skips=1 if malformed else 0, repeat=1, hole=False, ctx_free=False)
    c.update(kw)
    return c


def batches(cases):
    """-> [[(case, delta, is_probe)]]: converge i holds every case's i-th step, the last one the probes"""
    out = []
    for i in range(max([len(c["steps"]) for c in cases] + [0])):
        out.append([(c, c["steps"][i], False) for c in cases if i < len(c["steps"])])
    out.append([(c, c["probe"], True) for c in cases for _ in range(c["repeat"])])
    return [b for b in out if b]


def applied(batch):
    """the docs of a batch the reference applies: all but the probes the engine must skip"""
    return [(c, d) for c, d, probe in batch if not (probe and c["malformed"])]


def keys_of(docs):
    bs = [c["key"].encode() for c, _ in docs]
    offs = np.zeros(len(bs) + 1, np.uint64)
    offs[1:] = np.cumsum([len(b) for b in bs], dtype=np.uint64)
    return np.frombuffer(b"".join(bs), np.uint8), offs


def oracle_table(docs):
    """[(case, delta)] -> a batch table in the oracle's format"""
    t = {k: [] for k in ("dot_ids", "dot_seqs", "elems", "vv_ids", "vv_seqs", "cloud_ids", "cloud_seqs")}
    eo, vo, co = [0], [0], [0]
    for _, d in docs:
        for c, q, e in d["el"]:
            t["dot_ids"].append(c + 1), t["dot_seqs"].append(q), t["elems"].append(e)
        for c, n in d["vv"]:
            t["vv_ids"].append(c + 1), t["vv_seqs"].append(n)
        for c, q in d["cl"]:
            t["cloud_ids"].append(c + 1), t["cloud_seqs"].append(q)
        eo.append(len(t["elems"])), vo.append(len(t["vv_ids"])), co.append(len(t["cloud_ids"]))
    out = {k: np.array(v, np.uint64) for k, v in t.items()}
    out["key_bytes"], out["key_offs"] = keys_of(docs)
    out["el_offs"], out["vv_offs"], out["cloud_offs"] = (np.array(x, np.uint64) for x in (eo, vo, co))
    return out


def engine_arrays(docs):
    """[(case, delta)] -> (el_offs, dots, elems, vv_offs, vv, cloud_offs, cloud), packed, in the order given"""
    dots, elems, vv, cloud, eo, vo, co = [], [], [], [], [0], [0], [0]
    for _, d in docs:
        for c, q, e in d["el"]:
            dots.append((c << SEQ_BITS) | q), elems.append(e)
        for c, n in d["vv"]:
            vv.append((c << SEQ_BITS) | n)
        for c, q in d["cl"]:
            cloud.append((c << SEQ_BITS) | q)
        eo.append(len(dots)), vo.append(len(vv)), co.append(len(cloud))
    a = lambda x: np.array(x, np.uint64)
    return a(eo), a(dots), a(elems), a(vo), a(vv), a(co), a(cloud)


def doc_states(table):
    """an oracle state table -> {key: ({(c, q): e}, {c: n}, {(c, q)})}"""
    kb, ko = np.asarray(table["key_bytes"], np.uint8).tobytes(), np.asarray(table["key_offs"], np.int64)
    eo, vo, co = (np.asarray(table[k], np.int64) for k in ("el_offs", "vv_offs", "cloud_offs"))
    col = lambda k: (np.asarray(table[k], np.uint64).astype(np.int64) - 1).tolist()
    num = lambda k: np.asarray(table[k], np.uint64).tolist()
    di, dq, de, vi, vq, ci, cq = (col("dot_ids"), num("dot_seqs"), num("elems"), col("vv_ids"), num("vv_seqs"),
                                  col("cloud_ids"), num("cloud_seqs"))
    out = {}
    for i in range(len(ko) - 1):
        els = {(di[j], dq[j]): de[j] for j in range(eo[i], eo[i + 1])}
        vv = {vi[j]: vq[j] for j in range(vo[i], vo[i + 1])}
        cl = {(ci[j], cq[j]) for j in range(co[i], co[i + 1])}
        out[kb[ko[i]:ko[i + 1]].decode()] = (els, vv, cl)
    return out


EMPTY = ({}, {}, set())


def in_context(doc, d):
    return d[1] <= doc[1].get(d[0], 0) or d in doc[2]


# ---- the invariants of a raw read ---------------------------------------------------
def check_raw(read, exempt=()):
    """Engine.ujson_read's (el_offs, dots, elems, vv[n][R], cloud_offs, cloud):
    element dots and cloud dots strictly ascending per document, no cloud dot
    at or below its column's vv entry or equal to it + 1 (the cloud is
    compacted), every element dot inside the context.  `exempt`: indices of
    documents that hold an element outside their context on purpose."""
    eo, dots, _, vv, co, cloud = read
    eo, co = np.asarray(eo, np.int64), np.asarray(co, np.int64)
    dots, cloud, vv = np.asarray(dots, np.uint64), np.asarray(cloud, np.uint64), np.asarray(vv, np.uint64)
    n = len(eo) - 1
    R = vv.shape[1] if n else 1
    mask = np.uint64(SEQ_MAX)

    def split(offs, a):
        doc = np.repeat(np.arange(n), np.diff(offs))
        c = (a >> np.uint64(SEQ_BITS)).astype(np.int64)
        assert (c < R).all(), "a dot's column is outside the vv"
        return doc, c, a & mask

    def ascending(offs, a, what):
        if len(a) > 1:
            inner = np.ones(len(a) - 1, bool)
            inner[offs[1:-1][(offs[1:-1] > 0) & (offs[1:-1] < len(a))] - 1] = False
            bad = np.nonzero(inner & (a[1:] <= a[:-1]))[0]
            assert len(bad) == 0, f"{what} dots not strictly ascending at item {int(bad[0]) + 1}"

    assert eo[-1] == len(dots) and co[-1] == len(cloud)
    ascending(eo, dots, "element")
    ascending(co, cloud, "cloud")
    cdoc, cc, cq = split(co, cloud)
    cv = vv[cdoc, cc] if len(cloud) else np.zeros(0, np.uint64)
    bad = np.nonzero(cq <= cv)[0]
    assert len(bad) == 0, f"cloud dot {int(bad[0]) if len(bad) else 0} at or below its vv entry"
    bad = np.nonzero(cq == cv + np.uint64(1))[0]
    assert len(bad) == 0, f"cloud dot {int(bad[0]) if len(bad) else 0} is vv + 1: not compacted"
    edoc, ec, eq = split(eo, dots)
    if len(dots):
        covered = eq <= vv[edoc, ec]
        if len(exempt):
            covered |= np.isin(edoc, np.asarray(list(exempt), np.int64))
        # (document, dot) of the rest must be a (document, cloud dot): dots ranked, then paired with the doc
        _, rank = np.unique(np.concatenate([dots, cloud]), return_inverse=True)
        ke = (edoc.astype(np.uint64) << np.uint64(32)) | rank[:len(dots)].astype(np.uint64)
        kc = (cdoc.astype(np.uint64) << np.uint64(32)) | rank[len(dots):].astype(np.uint64)
        bad = np.nonzero(~covered & ~np.isin(ke, kc))[0]
        assert len(bad) == 0, f"element {int(bad[0]) if len(bad) else 0} outside its document's context"


# ---- what the oracle's states show of a case -------------------------------------------
def observed(c, before, after):
    """the outcome of case c's probe read off its document before and after"""
    if c["sweep"] in ("search", "join"):
        d = c["dot"]
        if c["what"] == "cloud":
            return "deduplicated" if in_context(before, d) else "kept" if in_context(after, d) else "lost"
        b, a = before[0].get(d), after[0].get(d)
        if c["sweep"] == "join":
            return a
        if b is not None:
            return "dropped" if a is None else "kept" if a == b else "replaced"
        return "added" if a is not None else "dropped"
    if c["sweep"] == "fold":
        col = c["col"]
        merged = max(before[1].get(col, 0), dict(c["probe"]["vv"]).get(col, 0))
        return (after[1].get(col, 0) - merged, after[1].get(col, 0))
    if c["sweep"] == "count":
        return (len(after[0]), len(after[2]), sum(after[1].values()))
    if c["sweep"] == "skip":
        return violation(c["probe"], c["R"]) or ("repeated" if c["repeat"] > 1 else "hole" if c["hole"] else None)
    if c["sweep"] in ("inplace", "tile"):  # compared with the case's `after`: (elements, cloud dots)
        return (len(after[0]), len(after[2]))
    raise KeyError(c["sweep"])


def violation(d, R):
    """the validation rule of k_uj_items a delta breaks (the first one), or None"""
    for kind in ("el", "cl"):
        prev = None
        for it in d[kind]:
            c, q = it[0], it[1]
            if c >= R:
                return "column"
            if q < 1:
                return "seq0"
            if prev is not None and (c, q) == prev:
                return "equal"
            if prev is not None and (c, q) < prev:
                return "descending"
            prev = (c, q)
    prev = None
    for c, _ in d["vv"]:
        if c >= R:
            return "vv_column"
        if prev is not None and c <= prev:
            return "vv_order"
        prev = c
    return None


# ---- a. search windows ------------------------------------------------------------------
SEARCH_L = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65)
SEARCH_SIDES = ("state_el", "state_cloud", "delta_el", "delta_cloud")


def ranks(L, equal):
    """probe ranks of a segment of L: 0..L absent (0..L-1 equal); past 17 the
    five lowest, the three around the middle and the five highest"""
    top = L - 1 if equal else L
    if top < 0:
        return []
    if L <= 17:
        return list(range(top + 1))
    m = L // 2
    return sorted({0, 1, 2, 3, 4, m - 1, m, m + 1, top - 4, top - 3, top - 2, top - 1, top})


def segment(L, straddle, col):
    """L sorted dots two seqs apart; straddle: the first half ends column col
    one below SEQ_MAX, the second half starts column col + 1 at seq 2"""
    if not straddle:
        return [(col, 2 * (j + 1)) for j in range(L)]
    h = (L + 1) // 2
    big = SEQ_MAX - 2 * h - 1
    return [(col, big + 2 * (j + 1)) for j in range(h)] + [(col + 1, 2 * (j - h + 1)) for j in range(h, L)]


def absent_at(ents, r, col):
    """dots that fall between ents[r - 1] and ents[r]"""
    L = len(ents)
    if L == 0:
        return [(col, 5)]
    if r == L:
        return [(ents[-1][0], ents[-1][1] + 1)]
    out = [(ents[r][0], ents[r][1] - 1)]
    if r and ents[r - 1][0] != ents[r][0]:
        out.append((ents[r - 1][0], ents[r - 1][1] + 1))  # (c, SEQ_MAX) next to (c + 1, 1)
    return out


def search_cases(Ls=SEARCH_L):
    """expect: the element at `dot` is "kept", "dropped", "replaced" or
    "added"; the cloud dot is "deduplicated" or "kept" """
    out = []
    E1, E2 = 1000, 5000

    def add(side, L, fl, r, steps, probe, dot, what, expect, straddle, **kw):
        out.append(case("a%05d" % len(out), steps, probe, expect, f"{side}/{what}", sweep="search", dot=dot,
                        what=what, tag=(side, L, fl, r, straddle), **kw))

    for straddle in (False, True):
        for L in Ls:
            if straddle and L < 2:
                continue  # no second column to straddle into
            ents = segment(L, straddle, 3)
            seg_els = {d: E1 + j for j, d in enumerate(ents)}
            probes = [("equal", r, ents[r]) for r in ranks(L, True)]
            for r in ranks(L, False):
                fl = "below" if r == 0 and L else "above" if r == L else "between"
                probes += [(fl, r, p) for p in absent_at(ents, r, 3)]
            for fl, r, p in probes:
                eq = fl == "equal"
                one = delta({p: E2}, None, {p})
                # the state's elements searched by a delta element (Win<8> wa)
                add("state_el", L, fl, r, [delta(seg_els, None, ents)], one, p, "element", "kept" if eq else "added",
                    straddle)
                # the state's cloud searched by a delta element (Win<4> wsc) and by a delta cloud dot (Win<8> wsc)
                add("state_cloud", L, fl, r, [delta(None, None, ents)], one, p, "element",
                    "dropped" if eq else "added", straddle)
                add("state_cloud", L, fl, r, [delta(None, None, ents)], delta(None, None, {p}), p, "cloud",
                    "deduplicated" if eq else "kept", straddle)
                # the delta's elements searched by a state element (Win<8> wb): the delta's map holds it
                # (kept: the state saw it), lacks it unseen (kept) or lacks it seen (dropped)
                st = [delta({p: E2}, None, {p})]
                add("delta_el", L, fl, r, st, delta(seg_els, None, ents), p, "element", "kept", straddle)
                if eq:  # ... and replaces it where the state holds it outside its context
                    add("delta_el", L, fl, r, [delta({p: E2})], delta(seg_els, None, ents), p, "element", "replaced",
                        straddle, ctx_free=True)
                else:
                    add("delta_el", L, fl, r, st, delta(seg_els, None, set(ents) | {p}), p, "element", "dropped",
                        straddle)
                # the delta's cloud searched by a state element (Win<4> wdc) and a state cloud dot (U3's w1)
                add("delta_cloud", L, fl, r, st, delta(None, None, ents), p, "element", "dropped" if eq else "kept",
                    straddle)
    return out


# ---- b. the join rule, one dot ----------------------------------------------------------
def join_cases():
    """expect: the element handle under `dot` after the join, or None"""
    out = []
    E1, E2, c, q = 41, 42, 1, 5
    for pos in ("first", "last"):
        f = 2 if pos == "first" else 0  # the other items of every segment lie after / before the dot
        for smap in (True, False):
            for sctx in ("vv", "cloud", None):
                for dmap in ("same", "diff", None):
                    for dctx in ("vv", "cloud", None):
                        d = (c, q)
                        s_el, s_cl = {(f, 10): 11, (f, 12): 12}, {(f, 10), (f, 12)}
                        if smap:
                            s_el[d] = E1
                        if sctx == "cloud":
                            s_cl.add(d)
                        state = delta(s_el, {c: q if sctx == "vv" else q - 2}, s_cl)
                        p_el, p_cl = {(f, 14): 13}, {(f, 14), (f, 20)}
                        if dmap:
                            p_el[d] = E1 if dmap == "same" else E2
                        if dctx == "cloud":
                            p_cl.add(d)
                        probe = delta(p_el, {c: q} if dctx == "vv" else None, p_cl)
                        if smap:
                            want = None if dctx and not dmap else E2 if dmap == "diff" and sctx is None else E1
                        else:
                            want = (E1 if dmap == "same" else E2) if dmap and sctx is None else None
                        out.append(case("b%03d" % len(out), [state], probe, want, "tile", sweep="join", dot=d,
                                        what="element", ctx_free=sctx is None,
                                        tag=(pos, smap, sctx, dmap, dctx)))
    return out


# ---- c. the fold rule -------------------------------------------------------------------
FOLD_V = (0, 1, 1000)
FOLD_N = (1, 2, 3, 4, 5, 8, 9, 64, 65)


def fold_cases(col):
    """expect: (dots folded into the vv, the vv entry afterwards).  The state's
    share of a run never starts at v + 1: a state holds no such cloud dot."""
    out = []

    def add(v, n, name, dset, sset, folded, dvv=None, svv=None, extra=()):
        last = v + n
        el = {(col, last): 77}
        s_el, d_el = (el, None) if last in sset else (None, el) if last in dset else (None, None)
        svv = v if svv is None else svv
        state = delta(s_el, {col: svv} if svv else None, {(col, q) for q in sset | set(extra)})
        probe = delta(d_el, {col: dvv} if dvv else None, {(col, q) for q in dset})
        out.append(case("c%04d" % len(out), [state], probe, (folded, v + folded), "tile", sweep="fold", col=col,
                        tag=(v, n, name)))

    for n in FOLD_N:
        for v in FOLD_V + (SEQ_MAX - n,):  # the last: the run ends at SEQ_MAX
            run = list(range(v + 1, v + n + 1))
            mid = max(1, n // 2)
            ks = list(range(1, n + 1)) if n <= 9 else [1, mid, n - 1, n]
            for k in ks:  # the delta holds the run's first k dots, the state the rest
                add(v, n, "split%d" % k, set(run[:k]), set(run[k:]), n)
            if n >= 2:
                add(v, n, "interleaved", set(run[0::2]), set(run[1::2]), n)
                for k in sorted({1, mid} - {n}):  # some dots in both sides
                    add(v, n, "both%d" % k, set(run[:k + 1]) | {run[-1]}, set(run[k:]), n)
            for g in sorted({0, n // 2, n - 1}):  # one gap: the run stops there
                add(v, n, "gap%d" % g, set(run[:mid]) - {run[g]}, set(run[mid:]) - {run[g]}, g)
            if v >= 1:  # the delta's vv entry is the merged one, over a state cloud dot it covers
                low = v >= 2
                for k in sorted({1, mid, n}):
                    add(v, n, "deltavv%d" % k, set(run[:k]), set(run[k:]), n, dvv=v, svv=v - 2 if low else 0,
                        extra=(v,) if low else ())
    return out


# ---- e. document counts -----------------------------------------------------------------
DOC_COUNTS = (1, 255, 256, 257, 1023, 1024, 1025, 1100)
COUNT_KINDS = ("el", "cl", "vv")


def count_cases(N, kind):
    """N documents, items in the first, a middle and the last one only; the
    rest empty or (every odd one, unless the vv is the kind) vv-only.  steps:
    the keys are new; probe: they exist.  expect: (elements, cloud dots, sum
    of the vv) afterwards."""
    carriers = {0, N // 2, N - 1}
    carry = {"el": (delta({(0, 1): 7, (0, 2): 8, (1, 1): 9}, None, {(0, 1), (0, 2), (1, 1)}),
                    delta({(0, 3): 10, (2, 1): 11}, None, {(0, 1), (0, 3), (2, 1)}), (4, 0, 5)),
             "cl": (delta(None, None, {(0, 2), (0, 4), (1, 3)}), delta(None, None, {(0, 1), (0, 3), (1, 3)}),
                    (0, 1, 4)),
             "vv": (delta(None, {0: 3, 2: 1}), delta(None, {0: 2, 1: 5, 2: 4}), (0, 0, 12))}[kind]
    out = []
    for i in range(N):
        if i in carriers:
            step, probe, want = carry
            path = "items"
        elif i % 2 and kind != "vv":
            step, probe, want = delta(None, {3: 1 + i % 5}), delta(None, {3: 2, 4: 1}), (0, 0, max(1 + i % 5, 2) + 1)
            path = "vv-only"
        else:
            step, probe, want = delta(), delta(), (0, 0, 0)
            path = "empty"
        out.append(case("e%04d" % i, [step], probe, want, path + ("/unstaged" if N > LDS_DOCS else "/lds"),
                        sweep="count"))
    return out


# ---- g. skips ---------------------------------------------------------------------------
def skip_cases(R=16):
    """expect: the rule the probe breaks ("column", "seq0", "equal",
    "descending", "vv_order", "vv_column"), "repeated", "hole", or None (a
    good neighbour).  A first dot of column R is followed by nothing (any dot
    after it is in a column >= R too, or descends), so "column" and
    "vv_column" at the first item stand alone in their segment."""
    out = []
    base = delta({(0, 1): 5, (1, 2): 6}, None, {(0, 1), (1, 2), (2, 4)})
    ok = {"el": [(4, 1, 21)], "vv": [(5, 2)], "cl": [(4, 1)]}

    def add(expect, probe, path, **kw):
        bad = expect is not None
        out.append(case("g%04d" % len(out), [base], probe, expect, path, malformed=bad, sweep="skip", R=R, **kw))

    def dots(kind, items):
        return [(c, q, 30 + j) for j, (c, q) in enumerate(items)] if kind == "el" else list(items)

    rules = {"column": {"first": [(R, 5)], "last": [(0, 2), (3, 1), (R, 5)]},
             "seq0": {"first": [(0, 0), (0, 2)], "last": [(0, 2), (1, 0)]},
             "equal": {"first": [(0, 2), (0, 2), (1, 1)], "last": [(0, 2), (1, 1), (1, 1)]},
             "descending": {"first": [(0, 3), (0, 2), (1, 1)], "last": [(0, 2), (1, 3), (1, 1)],
                            "column": [(1, 1), (0, 2)]}}
    for kind in ("el", "cl"):
        for rule, places in rules.items():
            for where, items in places.items():
                add(rule, dict(ok, **{kind: dots(kind, items)}), f"{kind}/{where}")
    for rule, places in {"vv_order": {"first": [(1, 1), (0, 2), (2, 1)], "last": [(0, 1), (2, 1), (1, 1)],
                                      "equal": [(0, 1), (0, 2)]},
                         "vv_column": {"first": [(R, 1)], "last": [(0, 1), (R, 1)]}}.items():
        for where, items in places.items():
            add(rule, dict(ok, vv=items), f"vv/{where}")

    # a bad document next to a good one across a tile edge: the bad one is
    # document 255 and its elements end at item 256, the good one is document
    # 256; the same with the cloud at document 511 | 512 and item 512
    def count(kind):
        return sum(len(c["probe"][kind]) for c in out)

    def pad_to(ndocs, kind, nitems):
        """good documents up to ndocs of them, one item of `kind` each, the last one the rest of nitems"""
        while len(out) < ndocs:
            rem = nitems - count(kind)
            assert rem >= 0
            k = rem if ndocs - len(out) == 1 else min(1, rem)
            items = [(6, 10 + j) for j in range(k)]
            add(None, {"el": dots("el", items) if kind == "el" else [], "vv": [], "cl": list(items)}, "pad")

    pad_to(DOC_TILE - 1, "el", TILE - 3)
    assert len(out) == DOC_TILE - 1 and count("el") == TILE - 3, (len(out), count("el"))
    add("descending", {"el": dots("el", [(0, 5), (0, 7), (0, 6)]), "vv": [], "cl": [(0, 5)]}, "el/tile-edge")
    assert count("el") == TILE
    add(None, delta({(0, 5): 50, (0, 6): 51}, None, {(0, 5), (0, 6)}), "el/tile-edge")
    pad_to(2 * DOC_TILE - 1, "cl", 2 * TILE - 3)
    assert len(out) == 2 * DOC_TILE - 1 and count("cl") == 2 * TILE - 3, (len(out), count("cl"))
    add("equal", {"el": [], "vv": [], "cl": [(0, 5), (0, 6), (0, 6)]}, "cl/tile-edge")
    assert count("cl") == 2 * TILE
    add(None, delta(None, None, {(0, 1), (0, 5)}), "cl/tile-edge")
    # a slot named twice (both copies skipped, counted once) and a JY_NO_SLOT hole (not counted)
    add("repeated", delta({(0, 2): 9}, None, {(0, 2)}), "claim", repeat=2)
    add("hole", delta({(0, 2): 9}, None, {(0, 2)}), "hole", hole=True)
    out[-1]["skips"] = 0
    return out


# ---- f. the in-place layout -------------------------------------------------------------
INPLACE_LONG_MIN = 8  # Engine.ujson_set_inplace: every document below is promoted by its step
INPLACE_STATS = ("promoted", "demoted", "inplace_docs", "inplace_folded", "inplace_added_el", "inplace_added_cloud")
JOB_DOCS = (127, 128, 129, 200)


def _inplace(out, state, probe, path, after, **stats):
    st = dict.fromkeys(INPLACE_STATS, 0)
    st.update(stats)
    out.append(case("f%03d" % len(out), [state], probe, st, path, sweep="inplace", stats=st, after=after,
                    step_stats={"promoted": 1}))


def inplace_cases():
    """R = 4, long_min 8.  expect: the ujson_stats differences of the probe's
    converge (a demoted document is merged on the regular path and promoted
    again); after: (elements, cloud dots) of the document afterwards.  No
    counter tells an append into the run's room from one into a regrown run
    ("append/ecap", "append/regrow", job_cases' "regrow/job"): those paths are
    labels, and a wrong capacity test shows only as a wrong state."""
    out = []
    run = {(0, q): 100 + q for q in range(1, 301)}
    full = delta(run, {0: 300})
    back = dict(demoted=1, promoted=1)
    # a context dot removes the live element at run index i: trimmed below kTrimSpan, demoted at or past it
    for i in (0, TRIM_SPAN - 2, TRIM_SPAN - 1, TRIM_SPAN):
        trim = i < TRIM_SPAN
        _inplace(out, full, delta(None, None, {(0, i + 1)}), "trim" if trim else "demote", (299, 0),
                 **(dict(inplace_docs=1) if trim else back))
    # a vv entry covers the run's first m elements (uj_item_long reads 8 at once, searches past them);
    # more than kTrimSpan of them demote; the delta may hold some of them
    for m in (7, 8, 9, TRIM_SPAN - 1, TRIM_SPAN, TRIM_SPAN + 1):
        for resend in (False, True):
            els = {(0, 2): 102, (0, m): 100 + m} if resend else None
            trim = m <= TRIM_SPAN
            _inplace(out, full, delta(els, {0: m}), ("trim" if trim else "demote") + ("/resend" if resend else ""),
                     (300 - m + (2 if resend else 0), 0), **(dict(inplace_docs=1) if trim else back))
    # ten elements: the column run's capacity is 2 * 10 + 16 = 36 (roomy, k_ujson.hip:313).  An append
    # reaches it exactly (in place) or passes it by one (a regrown run); the dots continue the vv and the
    # cloud run is empty, so they fold
    ten = delta({(0, q): 100 + q for q in range(1, 11)}, {0: 10})
    for k, path in ((26, "append/ecap"), (27, "append/regrow")):
        new = {(0, q): 200 + q for q in range(11, 11 + k)}
        _inplace(out, ten, delta(new, None, set(new)), path, (10 + k, 0), inplace_docs=1, inplace_added_el=k,
                 inplace_folded=k)
    # ... with a gap: the dots before it fold, the one after it starts the cloud run; and none contiguous
    new = {(0, 11): 1, (0, 12): 2, (0, 14): 3}
    _inplace(out, ten, delta(new, None, set(new)), "append/fold-gap", (13, 1), inplace_docs=1, inplace_added_el=3,
             inplace_folded=2, inplace_added_cloud=1)
    new = {(0, 12): 1, (0, 13): 2}
    _inplace(out, ten, delta(new, None, set(new)), "append/no-fold", (12, 2), inplace_docs=1, inplace_added_el=2,
             inplace_added_cloud=2)
    return out


def job_cases(n, how):
    """n long documents of one document tile (n <= 256), each demoted (a vv
    entry above the state's, in another column) or regrown (an append past its run's 2 * 8 + 16)
    by the probes' converge: one copy job each"""
    assert n <= DOC_TILE
    out = []
    eight = delta({(0, q): q for q in range(1, 9)}, {0: 8})
    new = {(0, q): 50 + q for q in range(9, 49)}
    for _ in range(n):
        if how == "demote":
            _inplace(out, eight, delta(None, {1: 5}), "demote/job", (8, 0), demoted=1, promoted=1)
        else:
            _inplace(out, eight, delta(new, None, set(new)), "regrow/job", (48, 0), inplace_docs=1,
                     inplace_added_el=40, inplace_folded=40)
    return out


# ---- d. tile geometry -------------------------------------------------------------------
TILE_LENGTHS = (255, 256, 257, 511, 512, 513, 767, 768, 769, 1025)
TILE_OFFSETS = (0, 1, 255)
# the item spaces k_uj_docs lays the documents of a batch into, in batch order: the touched state's
# elements (ao) and cloud (co), the delta's elements (deoff) and cloud (dcoff)
SPACES = {"state_el": "A", "state_cloud": "C", "delta_el": "B", "delta_cloud": "D"}
WAVE_POSITIONS = (63, 64, 65, 255, 256, 257)
WAVE_LENGTHS = (513, 769)


def space_sizes(state, probe):
    """what a document adds to each space in its probe's converge (state: its (elements, vv, cloud) then)"""
    return {"A": len(state[0]), "C": len(state[2]), "B": len(probe["el"]), "D": len(probe["cl"])}


def whole_tiles(off, sz):
    """the whole tiles [f0, f1) of a segment (k_uj_docs' ids lambda), and whether it names them in the
    tile map: only a segment longer than kLongSeg does"""
    f0, f1 = (off + TILE - 1) // TILE, (off + sz) // TILE
    return f0, f1, sz > LONG_SEG and f0 < f1


class _Lay:
    """documents laid one after another into the four spaces of one batch"""

    def __init__(self, prefix):
        self.off, self.out, self.prefix = dict(A=0, C=0, B=0, D=0), [], prefix

    def add(self, state, probe, after, path, **kw):
        st = (dict.fromkeys(x[:2] for x in state["el"]), {}, set(state["cl"])) if state else EMPTY
        c = case("%s%04d" % (self.prefix, len(self.out)), [state] if state else [], probe, after, path, sweep="tile",
                 after=after, lay=dict(self.off), **kw)
        for k, v in space_sizes(st, probe).items():
            self.off[k] += v
        self.out.append(c)
        return c

    def pad(self, sp, offmod):
        """a filler document that brings space sp to offmod (mod the tile): its items lie in column 5"""
        n = (offmod - self.off[sp]) % TILE
        if n == 0:
            return
        els, cl = {(5, q): q for q in range(1, n + 1)}, {(5, 2 * q) for q in range(1, n + 1)}
        if sp == "A":
            self.add(delta(els, {5: n}), delta(), (n, 0), "filler")
        elif sp == "C":
            self.add(delta(None, None, cl), delta(), (0, n), "filler")
        elif sp == "B":
            self.add(None, delta(els, {5: n}), (n, 0), "filler")
        else:
            self.add(None, delta(None, None, cl), (0, n), "filler")

    def target(self, side, offmod, state, probe, after, **kw):
        sp = SPACES[side]
        self.pad(sp, offmod)
        off = self.off[sp]
        sz = space_sizes((state["el"], {}, state["cl"]), probe)[sp]
        f0, f1, mapped = whole_tiles(off, sz)
        # declared from the length and the offset alone: a whole tile fits behind the partial first one
        whole = sz >= (-offmod) % TILE + TILE
        assert off % TILE == offmod and whole == (f0 < f1), (side, off, sz)
        path = side + ("/map" if mapped else "/whole-ids" if whole else "/ids")
        return self.add(state, probe, after, path, side=side, seg=(off, sz), whole=whole, mapped=mapped, **kw)


def _seg(L, col=3):
    return [(col, 2 * (j + 1)) for j in range(L)]


def tile_cases():
    """Documents whose state-element, state-cloud, delta-element or delta-cloud
    segment has a length around one, two, three and four tiles, at offsets 0,
    1 and 255 past a tile's start in its space.  expect = after: (elements,
    cloud dots) of the document afterwards.  path: whether the segment names
    whole tiles in the tile map ("map"), holds a whole tile but is short
    ("whole-ids"), or holds none ("ids")."""
    lay = _Lay("d")
    below = (2, 7)  # below everything of column 3
    for side in SPACES:
        for L in TILE_LENGTHS:
            for offmod in TILE_OFFSETS:
                S, m = _seg(L), L // 2
                gap, top = (3, S[m][1] + 1), (3, 2 * L + 1)  # between S[m] and S[m + 1]; above everything
                if side == "state_el":
                    # a different element under S[m] (the state's stays), three new dots, two removals
                    state = delta({d: 1000 + j for j, d in enumerate(S)}, None, S)
                    probe = delta({S[m]: 9, gap: 10, below: 11, top: 12}, None, {gap, below, top, S[1], S[L - 2]})
                    after = (L + 1, L + 3)
                elif side == "state_cloud":
                    # an element the state saw (dropped), a new one, two cloud dots it holds, three it lacks
                    state = delta(None, None, S)
                    probe = delta({S[m]: 9, gap: 10}, None, {gap, S[0], S[L - 1], top, below})
                    after = (1, L + 3)
                elif side == "delta_el":
                    # the state holds S[m], saw S[0]; its other two elements the delta never saw
                    state = delta({S[m]: 5, gap: 6, below: 7}, None, {S[m], gap, below, S[0]})
                    probe = delta({d: 2000 + j for j, d in enumerate(S)}, None, S)
                    after = (L + 1, L + 2)
                else:
                    # the delta's cloud removes the state's first, middle and last element, not the one between
                    state = delta({S[m]: 5, gap: 6, S[L - 1]: 7, S[0]: 8}, None, {S[m], gap, S[L - 1], S[0]})
                    probe = delta(None, None, S)
                    after = (1, L + 1)
                lay.target(side, offmod, state, probe, after, tag=(side, L, offmod))
    return lay.out


def wave_role(off, p, fl):
    """where a delta dot at (equal), just below or just above the state element at segment position p
    sits against the dot range [d0, d1) of the wave that holds space item off + p"""
    lane = (off + p) % WAVE
    if fl == "equal":
        return "d0" if lane == 0 else "d1-1" if lane == WAVE - 1 else "inside"
    if fl == "below":
        return "below-d0" if lane == 0 else "inside"
    return "above-d1-1" if lane == WAVE - 1 else "inside"


def wave_cases():
    """State-element segments that own whole tiles, one delta dot each: at the
    state element of position 63, 64, 65, 255, 256 or 257 (a context dot:
    it removes the element), just below it or just above it (an element:
    added).  path names the dot's place against its wave's dot range; "none":
    the delta holds no dot at all, only a vv entry over the first ten elements,
    so every wave takes the shortcut and the vv alone decides.  In a tile the
    map names every lane is live (f1 * 256 <= the segment's end), so a ragged
    wave is only ever the launch's last: the last document ends the space 1
    past a wave's start."""
    lay = _Lay("w")
    for L in WAVE_LENGTHS:
        S = _seg(L)
        state = delta({d: 1000 + j for j, d in enumerate(S)}, None, S)
        for offmod in TILE_OFFSETS:
            for p in WAVE_POSITIONS:
                for fl in ("equal", "below", "above"):
                    if fl == "equal":
                        probe, after = delta(None, None, {S[p]}), (L - 1, L)
                    else:
                        x = (3, S[p][1] + (-1 if fl == "below" else 1))
                        probe, after = delta({x: 9}, None, {x}), (L + 1, L + 1)
                    c = lay.target("state_el", offmod, state, probe, after, tag=(L, offmod, p, fl))
                    off, f0, f1 = c["seg"][0], *whole_tiles(*c["seg"])[:2]
                    c["role"] = wave_role(off, p, fl)
                    c["in_map"] = c["mapped"] and f0 <= (off + p) // TILE < f1
                    c["path"] += "/" + c["role"]
            c = lay.target("state_el", offmod, state, delta(None, {3: S[9][1]}), (L - 10, L - 10), tag=(L, offmod))
            c["role"], c["in_map"] = "none", c["mapped"]
            c["path"] += "/none"
    # the ragged last wave: the space ends one item into a wave, inside this document's end tile
    L = 769
    S = _seg(L)
    c = lay.target("state_el", 0, delta({d: 1000 + j for j, d in enumerate(S)}, None, S),
                   delta(None, None, {S[L - 1]}), (L - 1, L), tag=("ragged",))
    c["role"], c["in_map"] = "ragged", False
    c["path"] += "/ragged"
    assert lay.off["A"] % WAVE == 1
    return lay.out
