"""The canonical state digest restated in Python / NumPy (a test helper, not
collected): dmix, dcomb, dbytes, the d_* functions and the bucket formula of
jylis_amd/csrc/jy_digest.hpp, and the per-bucket [B, 4] array of a wire batch
(Engine.state_wire's arrays) given the replica id of every column."""
import numpy as np

M = (1 << 64) - 1
TAG_LOG, TAG_ENT, TAG_DOC, TAG_EL, TAG_VV, TAG_CL, TAG_REG, TAG_CNT, TAG_CELL, TAG_BUCKET = (
    0x7100, 0x7200, 0x7300, 0x7400, 0x7500, 0x7600, 0x7700, 0x7800, 0x7900, 0x7A00)


def dmix(x):
    x = (x + 0x9E3779B97F4A7C15) & M
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M
    return x ^ (x >> 31)


def dcomb(a, b):
    return dmix(a ^ dmix(b))


def dbytes(b):
    h = 0xCBF29CE484222325
    for c in bytes(b):
        h = ((h ^ c) * 0x100000001B3) & M
    return dcomb(h, len(b))


def d_reg(kh, ts, vh):
    return dcomb(kh, dcomb(TAG_REG, dcomb(ts, vh)))


def d_log(kh, cutoff):
    return dcomb(kh, dcomb(TAG_LOG, cutoff))


def d_ent(kh, rank, ts, vh):
    return dcomb(kh, dcomb(TAG_ENT ^ ((rank << 16) & M), dcomb(ts, vh)))


def d_doc(kh):
    return dcomb(kh, TAG_DOC)


def d_el(kh, rid, seq, elem):
    return dcomb(kh, dcomb(TAG_EL, dcomb(rid, dcomb(seq, elem))))


def d_vv(kh, rid, n):
    return dcomb(kh, dcomb(TAG_VV, dcomb(rid, n)))


def d_cl(kh, rid, seq):
    return dcomb(kh, dcomb(TAG_CL, dcomb(rid, seq)))


def d_cnt(kh):
    return dcomb(kh, TAG_CNT)


def d_cell(kh, sign, rid, v):
    return dcomb(kh, dcomb(TAG_CELL ^ (sign << 16), dcomb(rid, v)))


def bucket(kh, nbuckets):
    lg = int(nbuckets).bit_length() - 1
    assert 1 << lg == nbuckets and 0 <= lg <= 20
    return 0 if lg == 0 else dmix(kh ^ TAG_BUCKET) >> (64 - lg)


def _strings(bytes_, offs):
    b, o = bytes(np.asarray(bytes_, np.uint8)), [int(x) for x in np.asarray(offs)]
    return [b[o[i]:o[i + 1]] for i in range(len(o) - 1)]


def _ints(a):
    return [int(x) for x in np.asarray(a, np.uint64)]


def key_buckets(w, nbuckets):
    """the bucket of every record of a wire batch"""
    return [bucket(dbytes(k), nbuckets) for k in _strings(w["key_bytes"], w["key_offs"])]


def wire_digest(ctype, w, col_ids, nbuckets=1):
    """[nbuckets, 4] uint64: per bucket {digest, keys, items, bytes-or-cloud} of
    the wire batch w; col_ids[c] = the replica id of column c"""
    ids = _ints(col_ids)
    keys = _strings(w["key_bytes"], w["key_offs"])
    rows = {}  # bucket -> its four words (sparse: nbuckets may be 2^20)
    off = {k: _ints(v) for k, v in w.items() if k.endswith("_offs")}
    val = {k: _ints(w[k]) for k in w if not k.endswith("_offs") and not k.endswith("_bytes") and k != "sign"}
    if ctype in (2, 3):
        vals = _strings(w["val_bytes"], w["val_offs"])
    for i, k in enumerate(keys):
        kh = dbytes(k)
        r = rows.setdefault(bucket(kh, nbuckets), [0, 0, 0, 0])
        r[1] += 1
        if ctype in (0, 1):
            r[0] += d_cnt(kh)
            sign = _ints(w["sign"]) if ctype == 1 else None
            for j in range(off["cell_offs"][i], off["cell_offs"][i + 1]):
                v = val["val"][j]
                if v:
                    r[0] += d_cell(kh, sign[j] if sign else 0, ids[val["col"][j]], v)
                    r[2] += 1
                    r[3] += v
        elif ctype == 2:
            r[0] += d_reg(kh, val["ts"][i], dbytes(vals[i]))
            r[2] += 1
            r[3] += len(vals[i])
        elif ctype == 3:
            r[0] += d_log(kh, val["cutoff"][i])
            a = off["ent_offs"][i]
            for j in range(a, off["ent_offs"][i + 1]):
                r[0] += d_ent(kh, j - a, val["ts"][j], dbytes(vals[j]))
                r[2] += 1
                r[3] += len(vals[j])
        elif ctype == 4:
            r[0] += d_doc(kh)
            for j in range(off["el_offs"][i], off["el_offs"][i + 1]):
                d = val["dots"][j]
                r[0] += d_el(kh, ids[d >> 48], d & ((1 << 48) - 1), val["elems"][j])
                r[2] += 1
            for j in range(off["vv_offs"][i], off["vv_offs"][i + 1]):
                d = val["vv"][j]
                if d & ((1 << 48) - 1):
                    r[0] += d_vv(kh, ids[d >> 48], d & ((1 << 48) - 1))
            for j in range(off["cloud_offs"][i], off["cloud_offs"][i + 1]):
                d = val["cloud"][j]
                r[0] += d_cl(kh, ids[d >> 48], d & ((1 << 48) - 1))
                r[3] += 1
        else:
            raise ValueError(ctype)
    out = np.zeros((nbuckets, 4), np.uint64)
    for b, r in rows.items():
        out[b] = [x & M for x in r]
    return out


def table_to_wire(ctype, t, col_ids):
    """an oracle-format table -> a wire batch over the columns of col_ids (the
    inverse of jylis_amd.repo.wire_to_table, for the CPU tests)"""
    col = {int(x): c for c, x in enumerate(np.asarray(col_ids, np.uint64))}
    w = {"key_bytes": np.asarray(t["key_bytes"], np.uint8), "key_offs": np.asarray(t["key_offs"], np.uint64)}
    n = len(w["key_offs"]) - 1
    if ctype in (0, 1):
        cells = [[] for _ in range(n)]
        for g, pre in enumerate(("",) if ctype == 0 else ("p_", "n_")):
            o = _ints(t[pre + "offs"])
            for i in range(n):
                for j in range(o[i], o[i + 1]):
                    cells[i].append((g, col[int(t[pre + "ids"][j])], int(t[pre + "vals"][j])))
        flat = [c for cs in cells for c in sorted(cs)]
        w["cell_offs"] = np.cumsum([0] + [len(c) for c in cells]).astype(np.uint64)
        w["sign"] = np.array([c[0] for c in flat], np.uint8)
        w["col"] = np.array([c[1] for c in flat], np.uint16)
        w["val"] = np.array([c[2] for c in flat], np.uint64)
    elif ctype in (2, 3):
        for k in ("ts", "val_bytes", "val_offs") + (("cutoff", "ent_offs") if ctype == 3 else ()):
            w[k] = np.asarray(t[k])
    else:
        for offs, packed, i, q, payload in (("el_offs", "dots", "dot_ids", "dot_seqs", "elems"),
                                            ("vv_offs", "vv", "vv_ids", "vv_seqs", None),
                                            ("cloud_offs", "cloud", "cloud_ids", "cloud_seqs", None)):
            w[offs] = np.asarray(t[offs], np.uint64)
            w[packed] = np.array([(col[int(a)] << 48) | int(b) for a, b in zip(t[i], t[q])], np.uint64)
            if payload:
                w[payload] = np.asarray(t[payload], np.uint64)
    return w
