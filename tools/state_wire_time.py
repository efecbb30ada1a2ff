"""Timing of the state snapshot in wire form (jy_*_state_wire) against the
only routes the engine offered for the same arrays before it, on one engine.

  --part treg     N TREG keys (16-byte keys, 24-byte values, the mix of
                  tools/flush_wire_time.py):
      a_device    state_wire into device memory (size call + fill call)
      a_host      state_wire into host memory
      a_old       jy_treg_read + jy_keys_export + one jy_arena_read per value,
                  at --old-n keys (default 64K) and scaled linearly to N: its
                  per-value round trips make 1M slow
  --part pncount  N PNCOUNT keys x 64 columns x 2 signs in ONE chunk, at two
                  fills: dense (every cell non-zero) and sparse (one non-zero
                  cell per key):
      tile / lane the fill call (count + scan + cell writer) into preallocated
                  device arrays, with the tile writer and with the
                  lane-per-key writer (JY_STATE_CELLS=lane), three runs each,
                  alternating; `size` is the sizing call alone (count + scan)
      host        state_wire into host memory
      old         jy_counter_export + jy_keys_export to host + the NumPy
                  conversion of the dense block to cells, once, at N
      bytes       slab bytes read by the count, cells read and written by the
                  writer, masks and offsets: over the fill time, as a fraction
                  of the 6.29 TB/s copy ceiling

Times are wall clock around calls that end in a device synchronise, in ms;
every figure is listed with all its runs.  Each part is one process; run the
parts one after the other, each under its own time limit.  --out merges the
part's figures into a JSON file (profiles/state_wire_time.json)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from flush_wire_time import _fixed  # noqa: E402

COPY_CEILING = 6.29e12  # B/s, measured float4 copy on the MI355X
PNCOUNT, TREG = 1, 2


def timed(eng, fn, reps, warmup=1):
    out = []
    for r in range(warmup + reps):
        eng.sync()
        t0 = time.perf_counter()
        fn()
        eng.sync()
        if r >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), out


def part_treg(a):
    from jylis_amd.engine import Engine

    def bed(n):
        vals = _fixed(b"value:", n, 24)
        eng = Engine(device=0, key_capacity=max(n, 1024), arena_capacity=max(int(vals[1][-1]) * 2, 1 << 16))
        slots = eng.intern(TREG, _fixed(b"key:", n, 16))
        pre, lr = eng.pack_values(TREG, vals)
        eng.treg_converge(slots, np.full(n, 7, np.uint64), pre, lr)
        eng.sync()
        return eng

    res = {"n": a.n, "key_bytes": 16, "value_bytes": 24}
    eng = bed(a.n)
    res["a_device_ms"], res["a_device_runs"] = timed(eng, lambda: eng.state_wire(TREG, 0, a.n, device=True), a.reps)
    res["a_host_ms"], res["a_host_runs"] = timed(eng, lambda: eng.state_wire(TREG, 0, a.n), a.reps)
    w = eng.state_wire(TREG, 0, a.n)
    assert len(w["key_offs"]) == a.n + 1 and int(w["val_offs"][-1]) == 24 * a.n
    eng.close()

    eng = bed(a.old_n)

    def old():
        slots = np.arange(a.old_n, dtype=np.uint32)
        ts, pre, lr = eng.treg_read(slots)
        names = eng.key_names(TREG, 0, a.old_n)
        vals = [eng.value_bytes(TREG, p, l) for p, l in zip(pre, lr)]
        assert len(names) == len(vals) == a.old_n and len(vals[-1]) == 24
    ms, runs = timed(eng, old, max(1, a.reps // 2), warmup=0)
    eng.close()
    res["a_old_n"], res["a_old_ms_at_n"], res["a_old_runs"] = a.old_n, ms, runs
    res["a_old_ms_scaled"] = ms * a.n / a.old_n
    res["ratio_old_over_host"] = res["a_old_ms_scaled"] / res["a_host_ms"]
    return {"treg": res}


def cells_from_export(eng, n, ncols):
    """the old route's cells: the dense export walked on the host"""
    dump = eng.counter_export(PNCOUNT, ncols, 0, n)
    names = eng.key_names(PNCOUNT, 0, n)
    arr = dump.transpose(2, 0, 1).reshape(n, -1)
    nz = arr != 0
    slot, r = np.nonzero(nz)
    co = np.zeros(n + 1, np.uint64)
    co[1:] = np.cumsum(nz.sum(1))
    return names, co, (r // ncols).astype(np.uint8), (r % ncols).astype(np.uint16), arr[slot, r]


def part_pncount(a):
    import torch
    from jylis_amd.engine import TORCH_DTYPE, WIRE_ARRAYS, WIRE_SIZES, Engine
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
        need, _ = eng.state_wire_caps(PNCOUNT, 0, n, [0] * len(WIRE_SIZES[PNCOUNT]))
        ncells = need[2]
        assert ncells == (2 * ncols * n if fill == "dense" else n), need
        bufs = {name: torch.empty(max(need[idx] + plus, 1), dtype=getattr(torch, TORCH_DTYPE[dt]), device="cuda:0")
                for name, dt, idx, plus in WIRE_ARRAYS[PNCOUNT]}
        res = {"cells": ncells}
        res["size_ms"], res["size_runs"] = timed(
            eng, lambda: eng.state_wire_caps(PNCOUNT, 0, n, [0] * len(need)), a.reps)
        runs = {"tile": [], "lane": []}
        for r in range(1 + 3):  # one warm-up pair, then three alternating pairs
            for writer in ("tile", "lane"):
                os.environ["JY_STATE_CELLS"] = writer
                _, t = timed(eng, lambda: eng.state_wire_caps(PNCOUNT, 0, n, need, device=True, out=bufs), 1, warmup=0)
                if r:
                    runs[writer] += t
        os.environ.pop("JY_STATE_CELLS")
        slab = 2 * ncols * n * 8
        # count: the slab once, counts and masks out; writer: masks and offsets in, the named
        # cells in (8 B each) and out (11 B each); the key strings: 16 B in and out, their offsets
        algo = slab + n * (8 + 16) + n * (16 + 8) + ncells * (8 + 11) + n * (16 * 2 + 8 * 3)
        for writer in ("tile", "lane"):
            ms = statistics.median(runs[writer])
            res[writer + "_ms"], res[writer + "_runs"] = ms, runs[writer]
            res[writer + "_fraction_of_copy_ceiling"] = algo / (ms * 1e-3) / COPY_CEILING
        res["algorithmic_bytes"] = algo
        res["host_ms"], res["host_runs"] = timed(eng, lambda: eng.state_wire(PNCOUNT, 0, n), 2, warmup=0)
        w = eng.state_wire(PNCOUNT, 0, n)
        t0 = time.perf_counter()
        names, co, sign, col, val = cells_from_export(eng, n, ncols)
        res["old_ms"] = (time.perf_counter() - t0) * 1e3
        assert len(names) == n
        for got, want in ((w["cell_offs"], co), (w["sign"], sign), (w["col"], col), (w["val"], val)):
            assert np.array_equal(np.asarray(got), want)
        res["ratio_old_over_host"] = res["old_ms"] / res["host_ms"]
        eng.close()
        del bufs
        torch.cuda.empty_cache()
        out[fill] = res
    return {"pncount": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("treg", "pncount"), required=True)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--old-n", type=int, default=1 << 16)
    ap.add_argument("--reps", type=int, default=5)
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
