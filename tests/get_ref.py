"""Reference of the keyed reads (jy_*_get_keys) in numpy / pure Python.

Input: an oracle Repo.state() table (oracle/oracle.py's layout), the query
keys and, for TLOG, the counts.  Output: the arrays the calls return, built
from the table's wire order -- TLOG entries newest first, on equal timestamps
the greater value first -- so a comparison with the engine is byte-exact.
"""
import numpy as np

ALL = 2**64 - 1


def _b(k):
    return k.encode() if isinstance(k, str) else bytes(k)


def _rows(table):
    """key bytes -> row index of a state table"""
    kb = np.asarray(table["key_bytes"], np.uint8).tobytes()
    ko = np.asarray(table["key_offs"], np.int64)
    return {kb[ko[i]:ko[i + 1]]: i for i in range(len(ko) - 1)}


def _pack(values):
    offs = np.zeros(len(values) + 1, np.uint64)
    if values:
        offs[1:] = np.cumsum([len(v) for v in values], dtype=np.uint64)
    return np.frombuffer(b"".join(values), np.uint8).copy(), offs


def treg_get(table, keys):
    """-> {"found" u8[n], "ts" u64[n], "val_bytes", "val_offs" u64[n + 1], "sizes" [value bytes, found]}"""
    rows = _rows(table)
    vb = np.asarray(table["val_bytes"], np.uint8).tobytes()
    vo = np.asarray(table["val_offs"], np.int64)
    ts = np.asarray(table["ts"], np.uint64)
    found, ots, vals = [], [], []
    for k in keys:
        i = rows.get(_b(k))
        found.append(0 if i is None else 1)
        ots.append(0 if i is None else int(ts[i]))
        vals.append(b"" if i is None else vb[vo[i]:vo[i + 1]])
    ob, oo = _pack(vals)
    return {"found": np.array(found, np.uint8), "ts": np.array(ots, np.uint64), "val_bytes": ob, "val_offs": oo,
            "sizes": [len(ob), int(sum(found))]}


def tlog_get(table, keys, counts=None):
    """counts: None (every entry) or one per key (None / 2^64 - 1: every entry) ->
    {"found", "size", "cutoff", "ent_offs" u64[n + 1], "ts", "val_bytes",
    "val_offs" u64[entries + 1], "sizes" [entries, value bytes, found]}"""
    rows = _rows(table)
    eo = np.asarray(table["ent_offs"], np.int64)
    vb = np.asarray(table["val_bytes"], np.uint8).tobytes()
    vo = np.asarray(table["val_offs"], np.int64)
    ts = np.asarray(table["ts"], np.uint64)
    cut = np.asarray(table["cutoff"], np.uint64)
    found, size, cutoff, offs, ots, vals = [], [], [], [0], [], []
    for q, k in enumerate(keys):
        i = rows.get(_b(k))
        c = ALL if counts is None or counts[q] is None else int(counts[q])
        n = 0 if i is None else int(eo[i + 1] - eo[i])
        found.append(0 if i is None else 1)
        size.append(n)
        cutoff.append(0 if i is None else int(cut[i]))
        for j in range(min(n, c)):  # the table's order: newest first
            e = int(eo[i]) + j
            ots.append(int(ts[e]))
            vals.append(vb[vo[e]:vo[e + 1]])
        offs.append(len(ots))
    ob, oo = _pack(vals)
    return {"found": np.array(found, np.uint8), "size": np.array(size, np.uint64),
            "cutoff": np.array(cutoff, np.uint64), "ent_offs": np.array(offs, np.uint64),
            "ts": np.array(ots, np.uint64), "val_bytes": ob, "val_offs": oo,
            "sizes": [len(ots), len(ob), int(sum(found))]}


def counter_get(table, keys, pn=False):
    """-> (found u8[n], values: u64 sums mod 2^64; pn: (sum P - sum N) as int64)"""
    rows = _rows(table)

    def total(prefix, i):
        o = np.asarray(table[prefix + "offs"], np.int64)
        return sum(int(v) for v in np.asarray(table[prefix + "vals"], np.uint64)[o[i]:o[i + 1]])

    found, out = [], []
    for k in keys:
        i = rows.get(_b(k))
        found.append(0 if i is None else 1)
        if i is None:
            out.append(0)
        elif pn:
            out.append((total("p_", i) - total("n_", i)) % 2**64)
        else:
            out.append(total("", i) % 2**64)
    vals = np.array(out, np.uint64)
    return np.array(found, np.uint8), vals.view(np.int64) if pn else vals


def tlog_reply(ref, q):
    """query q of a tlog_get answer as GET replies it: [(value, ts)]"""
    eo, vo, vb = ref["ent_offs"], ref["val_offs"], ref["val_bytes"].tobytes()
    return [(vb[int(vo[j]):int(vo[j + 1])], int(ref["ts"][j])) for j in range(int(eo[q]), int(eo[q + 1]))]


def treg_reply(ref, q):
    """query q of a treg_get answer as GET replies it: (value, ts), or None"""
    if not ref["found"][q]:
        return None
    vo, vb = ref["val_offs"], ref["val_bytes"].tobytes()
    return vb[int(vo[q]):int(vo[q + 1])], int(ref["ts"][q])
