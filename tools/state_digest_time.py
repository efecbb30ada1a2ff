"""Timing of the state digest (jy_*_state_digest) on one engine, against the
state_wire device fill of the same range and against the route the engine
offered for the same answer before it (state to the host, the oracle's digest
there).

  --part pncount  N PNCOUNT keys x 64 columns x 2 signs in ONE call, at two
                  fills: dense (every cell non-zero) and sparse (one non-zero
                  cell per key), for B in {1, 4096, 2^20}:
      global / lds1k / lds4k
                  the digest into device memory with each accumulation form
                  (JY_DIGEST_ACC: no LDS stage; LDS rows up to 1,024 buckets;
                  up to 4,096), three runs each, alternating
      wire_fill   the state_wire fill call of the same range into preallocated
                  device arrays, same session
      hash        jy_state_bucket_slots with no bucket named: the key-hash pass,
                  a select that selects nothing and the count's read-back -- an
                  upper bound of the hash pass alone
      old         dense fill, once: jy_counter_export + jy_keys_export to the
                  host + or_digest_counter_dense there; the digests must be equal
  --part treg     N TREG keys (16-byte keys, 24-byte values, the mix of
                  tools/flush_wire_time.py): the same figures; old = state_wire
                  to the host + wire_to_table + or_digest_table, once

Times are wall clock around calls that end in a device synchronise, in ms;
every figure is listed with all its runs.  Each part is one process.  --out
merges the part's figures into a JSON file (profiles/state_digest_time.json)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from flush_wire_time import _fixed  # noqa: E402
from state_wire_time import timed  # noqa: E402

PNCOUNT, TREG = 1, 2
BUCKETS = (1, 4096, 1 << 20)
FORMS = ("global", "lds1k", "lds4k")


def digest_ab(eng, ctype, n):
    """per B: each form's three alternating runs (after one warm-up round), and that all forms agree"""
    out = {}
    for B in BUCKETS:
        runs, rows = {f: [] for f in FORMS}, {}
        for r in range(1 + 3):
            for form in FORMS:
                os.environ["JY_DIGEST_ACC"] = form
                # (the output tensor is dropped at once, so every run reuses the same cached block)
                _, t = timed(eng, lambda: eng.digest_range(ctype, B, 0, n, device=True), 1, warmup=0)
                if r:
                    runs[form] += t
                else:
                    rows[form] = eng.digest_range(ctype, B, 0, n)
        os.environ.pop("JY_DIGEST_ACC")
        assert all(np.array_equal(rows[f], rows[FORMS[0]]) for f in FORMS)
        out[str(B)] = {f + "_ms": statistics.median(runs[f]) for f in FORMS}
        out[str(B)].update({f + "_runs": runs[f] for f in FORMS})
        _, t = timed(eng, lambda: eng.digest_range(ctype, B, 0, n, device=True), 3)
        out[str(B)]["default_ms"], out[str(B)]["default_runs"] = statistics.median(t), t
    return out


def wire_fill(eng, ctype, n, reps):
    import torch
    from jylis_amd.engine import TORCH_DTYPE, WIRE_ARRAYS, WIRE_SIZES
    need, _ = eng.state_wire_caps(ctype, 0, n, [0] * len(WIRE_SIZES[ctype]))
    bufs = {name: torch.empty(max(need[idx] + plus, 1), dtype=getattr(torch, TORCH_DTYPE[dt]), device="cuda:0")
            for name, dt, idx, plus in WIRE_ARRAYS[ctype]}
    ms, runs = timed(eng, lambda: eng.state_wire_caps(ctype, 0, n, need, device=True, out=bufs), reps)
    del bufs
    torch.cuda.empty_cache()
    return ms, runs


def common(eng, ctype, n, reps):
    res = {"digest": digest_ab(eng, ctype, n)}
    res["wire_fill_ms"], res["wire_fill_runs"] = wire_fill(eng, ctype, n, reps)
    res["hash_ms"], res["hash_runs"] = timed(eng, lambda: eng.bucket_slots(ctype, 4096, []), reps)
    for B in BUCKETS:
        d = res["digest"][str(B)]
        d["wire_fill_over_digest"] = res["wire_fill_ms"] / d["default_ms"]
        d["hash_share_upper_bound"] = res["hash_ms"] / d["default_ms"]
    return res


def part_pncount(a):
    import torch
    import oracle as O
    from jylis_amd.engine import Engine, encode_keys
    n, ncols = a.n, 64
    out = {"n": n, "columns": ncols, "signs": 2}
    for fill in ("dense", "sparse"):
        eng = Engine(device=0, key_capacity=max(n, 1024), counter_columns=ncols)
        eng.replica_cols([5000 + c for c in range(ncols)])
        eng.intern(PNCOUNT, _fixed(b"cnt:", n, 16))
        if fill == "dense":
            vp = torch.arange(1, ncols * n + 1, dtype=torch.int64, device="cuda:0").reshape(ncols, n)
            vn = vp + 7
        else:
            vp = torch.zeros((ncols, n), dtype=torch.int64, device="cuda:0")
            k = torch.arange(n, device="cuda:0")
            vp[k % ncols, k] = k + 1
            vn = torch.zeros_like(vp)
        eng.pncount_converge_block(np.arange(ncols, dtype=np.uint16), 0, vp, vn)
        eng.sync()
        del vp, vn
        torch.cuda.empty_cache()
        res = common(eng, PNCOUNT, n, a.reps)
        got = eng.digest_range(PNCOUNT, 1, 0, n)
        assert int(got[0, 1]) == n and int(got[0, 2]) == (2 * ncols * n if fill == "dense" else n)
        if fill == "dense":
            t0 = time.perf_counter()
            dense = eng.counter_export(PNCOUNT, ncols, 0, n)
            kb, ko = encode_keys(eng.key_names(PNCOUNT, 0, n))
            ids = np.array([eng.replica_id(c) for c in range(ncols)], np.uint64)
            want = O.digest_counter_dense(kb, ko, ids, dense)
            res["old_ms"] = (time.perf_counter() - t0) * 1e3
            assert tuple(int(x) for x in want) == tuple(int(x) for x in got[0]), (want, got)
            res["old_over_digest_b1"] = res["old_ms"] / res["digest"]["1"]["default_ms"]
            del dense
        eng.close()
        out[fill] = res
    return {"pncount": out}


def part_treg(a):
    import oracle as O
    from jylis_amd.engine import Engine
    from jylis_amd.repo import wire_to_table
    n = a.n
    vals = _fixed(b"value:", n, 24)
    eng = Engine(device=0, key_capacity=max(n, 1024), arena_capacity=max(int(vals[1][-1]) * 2, 1 << 16))
    slots = eng.intern(TREG, _fixed(b"key:", n, 16))
    pre, lr = eng.pack_values(TREG, vals)
    eng.treg_converge(slots, np.full(n, 7, np.uint64), pre, lr)
    eng.sync()
    res = {"n": n, "key_bytes": 16, "value_bytes": 24}
    res.update(common(eng, TREG, n, a.reps))
    got = eng.digest_range(TREG, 1, 0, n)
    t0 = time.perf_counter()
    want = O.digest_table(TREG, wire_to_table(TREG, eng.state_wire(TREG, 0, n), ()))
    res["old_ms"] = (time.perf_counter() - t0) * 1e3
    assert tuple(int(x) for x in want) == tuple(int(x) for x in got[0]), (want, got)
    res["old_over_digest_b1"] = res["old_ms"] / res["digest"]["1"]["default_ms"]
    eng.close()
    return {"treg": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("treg", "pncount"), required=True)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    res = part_treg(a) if a.part == "treg" else part_pncount(a)
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        old = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                old = json.load(f)
        old.update(res)
        with open(a.out, "w") as f:
            json.dump(old, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
