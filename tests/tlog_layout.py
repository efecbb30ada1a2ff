"""TLOG segment layout: checks over Engine.tlog_layout reads and a plain model
of one key's merge (numpy / python only; nothing here touches the GPU).

A layout is what Engine.tlog_layout returns: u64 columns base, front, len,
cap, cutoff, newest (one row per log) and the ints pcap (pool capacity) and
used (the bump pointer).  A log owns the pool interval [base - front,
base + cap)."""
import numpy as np

OUTCOMES = ("unchanged", "append", "insert_up", "insert_down", "rebuild")


def row(layout, i):
    """(base, front, len, cap) of log i as ints"""
    return tuple(int(layout[c][i]) for c in ("base", "front", "len", "cap"))


def check_layout(layout):
    """every non-empty log lies inside the pool with its front room below it,
    holds no more than its capacity, and shares no pool entry with another"""
    base, front, n, cap = (np.asarray(layout[c]).astype(object) for c in ("base", "front", "len", "cap"))
    live = [i for i in range(len(base)) if n[i] > 0]
    for i in live:
        assert front[i] <= base[i], f"log {i}: front room {front[i]} reaches below the pool (base {base[i]})"
        assert n[i] <= cap[i], f"log {i}: len {n[i]} > cap {cap[i]}"
        assert base[i] + cap[i] <= layout["pcap"], f"log {i}: [{base[i]}, +{cap[i]}) past the pool ({layout['pcap']})"
    live.sort(key=lambda i: base[i])
    for a, b in zip(live, live[1:]):
        assert base[a] + cap[a] <= base[b] - front[b], (
            f"logs {a} and {b} overlap: [{base[a] - front[a]}, {base[a] + cap[a]}) and "
            f"[{base[b] - front[b]}, {base[b] + cap[b]})")


def check_entries(layout, table):
    """the entries read back (a state table whose rows are the layout's rows):
    strictly ordered, later timestamp then greater value first; `newest` is
    the first entry's timestamp; nothing is below the cutoff"""
    offs = np.asarray(table["ent_offs"]).astype(np.int64)
    ts = np.asarray(table["ts"], np.uint64)
    vb, vo = bytes(np.asarray(table["val_bytes"], np.uint8)), np.asarray(table["val_offs"]).astype(np.int64)
    assert len(offs) - 1 == len(layout["len"])
    for i in range(len(offs) - 1):
        a, b = int(offs[i]), int(offs[i + 1])
        assert b - a == int(layout["len"][i]), f"log {i}: {b - a} entries read, len {layout['len'][i]}"
        assert int(table["cutoff"][i]) == int(layout["cutoff"][i])
        if a == b:
            continue
        ents = [(int(ts[j]), vb[int(vo[j]):int(vo[j + 1])]) for j in range(a, b)]
        assert all(x > y for x, y in zip(ents, ents[1:])), f"log {i}: entries not strictly newest first"
        assert ents[0][0] == int(layout["newest"][i]), f"log {i}: newest {layout['newest'][i]} != {ents[0][0]}"
        assert ents[-1][0] >= int(layout["cutoff"][i]), f"log {i}: an entry below the cutoff"


def classify(before, after, drop, Mi, interleaves):
    """what a merge did to one key, from its (base, front, len, cap) before and
    after: drop = state entries its raised cutoff removed, Mi = kept delta
    entries ranked inside the log, interleaves = Mi > 0.  (A down-insert with
    drop == Mi == every kept entry would read as unchanged: cases avoid it.)"""
    if tuple(before) == tuple(after):
        return "unchanged"
    ob, of, _, oc = before
    nb = after[0]
    if not (ob - of <= nb < ob + max(oc, 1)) or oc == 0:
        return "rebuild"
    if interleaves and nb == ob + drop - Mi:
        return "insert_down"
    if nb == ob + drop:
        return "insert_up" if interleaves else "append"
    raise AssertionError(f"no outcome explains {before} -> {after} (drop {drop}, Mi {Mi})")


def merge_model(log, cut, dcut, dents):
    """one key's join in plain python.  log: [(ts, value)] ascending, cut its
    cutoff; the delta (dcut, [(value, ts)]).  -> (new log, new cutoff, stats):
    drop (state entries the cutoff removes), below / dup / newer / inter (delta
    entries under the merged cutoff, already in the log, kept above every state
    entry, kept inside the log), M = newer + inter, minrank / mx (smallest and
    largest rank of a kept entry inside the log; rank = state entries older
    than it, the dropped ones included)"""
    ncut = max(cut, dcut)
    have = set(log)
    st = dict(drop=sum(1 for e in log if e[0] < ncut), below=0, dup=0, newer=0, inter=0, minrank=len(log), mx=0)
    kept = []
    for v, t in dents:
        e = (t, v)
        if t < ncut:
            st["below"] += 1
        elif e in have:
            st["dup"] += 1
        else:
            r = sum(1 for x in log if x < e)
            if r == len(log):
                st["newer"] += 1
            else:
                st["inter"] += 1
                st["minrank"] = min(st["minrank"], r)
                st["mx"] = max(st["mx"], r)
            kept.append(e)
    st["M"] = st["newer"] + st["inter"]
    return sorted([e for e in log if e[0] >= ncut] + kept), ncut, st


def expected_outcome(before, st):
    """where an accepted delta goes, by the merge's stated rules: no kept entry
    and no drop changes nothing; without an interleaving entry it is an append
    if len + M fits the segment; an interleaving one is inserted in place,
    moving the prefix down when that fits (Mi entries of front room, the dropped
    prefix counted) and moves fewer entries than moving the suffix up (a tie
    goes up) or when up does not fit; when neither fits the log is rebuilt"""
    _, front, n, cap = before
    M, Mi, drop = st["M"], st["inter"], st["drop"]
    if M == 0 and drop == 0:
        return "unchanged"
    up_ok = n + M <= cap
    if Mi == 0 and up_ok:
        return "append"
    dn_ok = Mi <= front + drop and n + (M - Mi) <= cap
    up, dn = n - st["minrank"], st["mx"] - drop
    if dn_ok and (not up_ok or dn < up):
        return "insert_down"
    return "insert_up" if up_ok else "rebuild"


def table_logs(table):
    """a TLOG state table -> {key bytes: (cutoff, [(ts, value)] ascending)}"""
    kb, ko = bytes(np.asarray(table["key_bytes"], np.uint8)), np.asarray(table["key_offs"]).astype(np.int64)
    vb, vo = bytes(np.asarray(table["val_bytes"], np.uint8)), np.asarray(table["val_offs"]).astype(np.int64)
    eo, ts = np.asarray(table["ent_offs"]).astype(np.int64), np.asarray(table["ts"], np.uint64)
    out = {}
    for i in range(len(ko) - 1):
        ents = [(int(ts[j]), vb[int(vo[j]):int(vo[j + 1])]) for j in range(int(eo[i]), int(eo[i + 1]))]
        out[kb[int(ko[i]):int(ko[i + 1])]] = (int(table["cutoff"][i]), sorted(ents))
    return out


def oracle_counts(before, after, dcut, dents):
    """(inter, newer, dup, below) of a delta from one key's (cutoff, log) before
    and after the oracle's converge"""
    bcut, blog = before
    acut, alog = after
    assert acut == max(bcut, dcut)
    have, now = set(blog), set(alog)
    top = max(blog) if blog else None
    inter = newer = dup = below = 0
    for v, t in dents:
        e = (t, v)
        if t < acut:
            below += 1
            assert e not in now
        elif e in have:
            dup += 1
        else:
            assert e in now
            if top is None or e > top:
                newer += 1
            else:
                inter += 1
    assert now == {e for e in have if e[0] >= acut} | {(t, v) for v, t in dents if t >= acut}
    return inter, newer, dup, below
