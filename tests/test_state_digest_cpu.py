"""The state digest's host-side pieces, without a GPU: the nine calls are
declared alike in the header, the ctypes table and the Pony FFI; the Python
restatement of the digest (tests/digest_ref.py) agrees with the oracle's;
antientropy.diff; the header states the bucket formula."""
import os
import re

import numpy as np
import pytest

import digest_ref as R
from helpers import random_history
from test_pony_glue import header_arity, pony_decls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_CALLS = ["jy_counter_state_digest", "jy_treg_state_digest", "jy_tlog_state_digest", "jy_ujson_state_digest",
             "jy_state_bucket_slots", "jy_counter_state_wire_slots", "jy_treg_state_wire_slots",
             "jy_tlog_state_wire_slots", "jy_ujson_state_wire_slots"]


def test_the_nine_calls_are_declared_alike():
    from jylis_amd import _lib
    hdr, pony = header_arity(), pony_decls()
    for name in NEW_CALLS:
        assert name in hdr and name in pony and name in _lib.SIGNATURES, name
        assert hdr[name] == pony[name] == len(_lib.SIGNATURES[name][1]), name
        assert _lib.SIGNATURES[name][0] is _lib.I32
    # a slot-list dump takes its range twin's arguments with (slot0, nslots) -> (n, slots, slots_mem)
    for t in ("counter", "treg", "tlog", "ujson"):
        assert hdr[f"jy_{t}_state_wire_slots"] == hdr[f"jy_{t}_state_wire"] + 1


def test_the_header_states_the_bucket_formula():
    text = " ".join(open(os.path.join(ROOT, "include", "jylis_gpu.h")).read().split())
    text = text.replace(" * ", " ")
    assert "bucket(kh, B) = 0 if B == 1 = dmix(kh ^ 0x7A00) >> (64 - log2 B) otherwise" in text
    assert re.search(r"jy_node_lock_type\(node, type\), NEVER under JY_NODE_NOFENCE", text)
    own = " ".join(open(os.path.join(ROOT, "jylis_amd", "csrc", "jy_digest.hpp")).read().split()).replace(" // ", " ")
    assert "dmix(kh ^ 0x7A00) >> (64 - log2 B)" in own


def _col_ids(t, fields, seed):
    ids = np.unique(np.concatenate([np.asarray(t[f], np.uint64) for f in fields] + [np.zeros(0, np.uint64)]))
    return ids[np.random.default_rng(seed).permutation(len(ids))]  # any column order


@pytest.mark.parametrize("B", [1, 64])
@pytest.mark.parametrize("ctype", [2, 3, 4])
def test_ref_equals_the_oracle_table_digest(oracle_mod, ctype, B):
    O = oracle_mod
    r = O.Repo(ctype)
    for b in random_history(O, ctype, 20 + ctype, nops=200, **({} if ctype == 4 else {"val_len": 20})):
        r.converge(b)
    t = r.state()
    ids = _col_ids(t, ("dot_ids", "vv_ids", "cloud_ids") if ctype == 4 else (), 3)
    d = R.wire_digest(ctype, R.table_to_wire(ctype, t, ids), ids, B)
    assert d.shape == (B, 4)
    with np.errstate(over="ignore"):
        assert tuple(int(x) for x in d.sum(axis=0, dtype=np.uint64)) == tuple(int(x) for x in O.digest_table(ctype, t))
    assert tuple(int(x) for x in O.digest_table(ctype, t)) == tuple(int(x) for x in O.digest_repo(r))
    if B == 64:
        assert (d[:, 1] > 0).sum() > 1  # the keys spread over buckets
        assert R.key_buckets(R.table_to_wire(ctype, t, ids), 1) == [0] * (len(t["key_offs"]) - 1)


@pytest.mark.parametrize("B", [1, 64])
@pytest.mark.parametrize("ctype", [0, 1])
def test_ref_equals_the_oracle_dense_counter_digest(oracle_mod, ctype, B):
    O = oracle_mod
    r = O.Repo(ctype)
    for b in random_history(O, ctype, 30 + ctype, nops=200, nkeys=30):
        r.converge(b)
    t = r.state()
    pres = ("",) if ctype == 0 else ("p_", "n_")
    ids = _col_ids(t, [p + "ids" for p in pres], 4)
    w = R.table_to_wire(ctype, t, ids)
    n = len(w["key_offs"]) - 1
    dense = np.zeros((len(pres), len(ids), n), np.uint64)
    key = np.repeat(np.arange(n), np.diff(w["cell_offs"].astype(np.int64)))
    dense[w["sign"].astype(np.int64), w["col"].astype(np.int64), key] = w["val"]
    want = O.digest_counter_dense(w["key_bytes"], w["key_offs"], ids, dense, threads=2)
    d = R.wire_digest(ctype, w, ids, B)
    with np.errstate(over="ignore"):
        assert tuple(int(x) for x in d.sum(axis=0, dtype=np.uint64)) == tuple(int(x) for x in want)
    assert tuple(int(x) for x in want) == tuple(int(x) for x in O.digest_repo(r))


def test_antientropy_diff():
    from jylis_amd.antientropy import diff
    a = np.arange(32, dtype=np.uint64).reshape(8, 4)
    assert diff(a, a.copy()).tolist() == []
    b = a.copy()
    b[2, 0] ^= np.uint64(1 << 63)
    b[5, 3] += np.uint64(1)
    b[7, 1] = 0
    assert diff(a, b).tolist() == [2, 5, 7] and diff(b, a).tolist() == [2, 5, 7]
    assert diff(a[:1], b[:1]).tolist() == []
    with pytest.raises(ValueError):
        diff(a, a[:4])
    with pytest.raises(ValueError):
        diff(a.reshape(4, 8), a.reshape(4, 8))
