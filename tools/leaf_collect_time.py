"""Timing of the UJSON leaf store's collection (jy_ujson_leaves_collect) on one
engine, in wall-clock ms of the whole call (it is synchronising: its one wait
and the final one are inside), next to the only alternative a user had before
it existed:

  collect     Engine.ujson_leaves_collect() on a store of N distinct leaves of
              24 bytes, half of them referenced: N / 16 documents of 8 elements,
              built with one ujson_converge.  No `keep`, no shrink.
  get_put     the live handles' leaves read with ujson_leaves_get (its sizing
              and its fill call, device arrays) and put into a fresh engine
              whose store was reserved for them, then a sync of that engine

Every figure is the median of --reps runs after a warm-up, listed with all its
runs; each run makes fresh engines.  collect_event_ms is the same call between
two HIP events on the engine stream.  --out writes the JSON."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
UJSON = 4
PER_DOC = 8


def main():
    import torch
    from jylis_amd.engine import DOT_SEQ_BITS, Engine
    from leaf_store_time import fixed
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = "cuda:0"
    ndocs = a.n // (2 * PER_DOC)
    nlive = ndocs * PER_DOC
    # a leaf: path ("k",), then the terminator, then a 15-digit value: 24 bytes
    lb, lo = fixed(b"\x01\x00\x00\x00k\xff\xff\xff\xff", a.n, 24)
    kb, ko = fixed(b"doc:", ndocs, 12)
    # document i: elements 8 i .. 8 i + 7 under the dots (column 0, 1 .. 8), a version vector that covers them
    eo = np.arange(ndocs + 1, dtype=np.uint64) * np.uint64(PER_DOC)
    dots = np.tile(np.arange(1, PER_DOC + 1, dtype=np.uint64), ndocs)
    vo = np.arange(ndocs + 1, dtype=np.uint64)
    vv = np.full(ndocs, PER_DOC, np.uint64)
    co, cloud = np.zeros(ndocs + 1, np.uint64), np.zeros(0, np.uint64)
    assert DOT_SEQ_BITS == 48  # (column 0: a packed dot is its sequence number)
    runs = {k: [] for k in ("collect", "collect_event", "get_put")}

    for r in range(a.reps + 1):  # run 0 is the warm-up
        eng = Engine(device=0, key_capacity=[1024, 1024, 1024, 1024, max(ndocs, 1024)])
        eng.replica_col(0x5EED)  # column 0
        eng.ujson_leaves_reserve(a.n, 32 * a.n)
        h = eng.ujson_leaves_put(torch.from_numpy(lb).to(dev), torch.from_numpy(lo.view(np.int64)).to(dev))
        eng.sync()
        live = h[:nlive].contiguous()
        slots = eng.intern(UJSON, (kb, ko))
        eng.ujson_converge(slots, eo, dots, live.cpu().numpy().view(np.uint64), vo, vv, co, cloud)
        eng.sync()
        assert eng.ujson_leaves_usage()[:2] == (a.n, 24 * a.n)
        # ---- the alternative: read the live leaves, put them into a fresh reserved engine ----
        other = Engine(device=0)
        other.ujson_leaves_reserve(nlive, 32 * nlive)
        other.sync()
        t0 = time.perf_counter()
        glb, glo = eng.ujson_leaves_get(live, device=True)
        h2 = other.ujson_leaves_put(glb, glo)
        other.sync()
        runs["get_put"].append((time.perf_counter() - t0) * 1e3)
        assert torch.equal(h2, live) and other.ujson_leaves_usage()[:2] == (nlive, 24 * nlive)
        other.close()
        # ---- the collection ----
        s = torch.cuda.ExternalStream(eng.stream(), device=dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        eng.sync()
        e0.record(s)
        t0 = time.perf_counter()
        got = eng.ujson_leaves_collect()
        runs["collect"].append((time.perf_counter() - t0) * 1e3)
        e1.record(s)
        e1.synchronize()
        runs["collect_event"].append(e0.elapsed_time(e1))
        assert tuple(got) == (nlive, 24 * nlive, a.n - nlive, 24 * (a.n - nlive), 0, 0), got
        back, _ = eng.ujson_leaves_get(live[::4097].contiguous(), device=True)
        assert torch.equal(back.cpu(), torch.from_numpy(lb.reshape(a.n, 24)[:nlive:4097].reshape(-1).copy()))
        eng.close()
    res = {"n": a.n, "leaf_bytes": 24, "docs": ndocs, "elements_per_doc": PER_DOC, "live": nlive, "reps": a.reps}
    for k, v in runs.items():
        res[k + "_ms"], res[k + "_runs"] = statistics.median(v[1:]), v[1:]
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
