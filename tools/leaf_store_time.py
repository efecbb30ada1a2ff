"""Timing of the UJSON leaf store (jy_ujson_leaves_put / _get) on one engine,
by HIP events on the engine stream around each call, in ms:

  put_first   one put of N distinct leaves of 24 bytes into a store reserved
              for them (no rehash, no reallocation inside the call)
  put_again   the same batch once more: every leaf is already present
  get         one get of the same N handles into preallocated device arrays
              (the fill call; the sizing call is `get_size`)
  keys_wire   for comparison, the fill call of jy_ujson_state_wire over N
              empty documents with 24-byte keys: the same gather kernel, fed
              from the key directory

Inputs and outputs are device arrays.  Every figure is the median of --reps
runs after a warm-up, listed with all its runs; a run of put_first needs a
fresh engine, so each run makes its own.  --out writes the JSON."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
UJSON = 4


def fixed(prefix, n, width):
    """n items of `width` bytes: prefix + a zero-padded decimal index"""
    digits = width - len(prefix)
    raw = b"".join(prefix + b"%0*d" % (digits, i) for i in range(n))
    return np.frombuffer(raw, np.uint8).copy(), np.arange(n + 1, dtype=np.uint64) * np.uint64(width)


def main():
    import torch
    from jylis_amd.engine import WIRE_SIZES, Engine
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = "cuda:0"
    # a leaf: path ("k",), then the terminator, then a 15-digit value: 24 bytes
    lb, lo = fixed(b"\x01\x00\x00\x00k\xff\xff\xff\xff", a.n, 24)
    warm_b, warm_o = fixed(b"\x01\x00\x00\x00w\xff\xff\xff\xff", 4096, 24)
    kb, ko = fixed(b"key:", a.n, 24)
    runs = {k: [] for k in ("put_first", "put_again", "get_size", "get", "keys_wire")}

    def timed(eng, name, fn):
        s = torch.cuda.ExternalStream(eng.stream(), device=dev)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        eng.sync()
        t0.record(s)
        out = fn()
        t1.record(s)
        eng.sync()
        t1.synchronize()
        runs[name].append(t0.elapsed_time(t1))
        return out

    for r in range(a.reps + 1):  # run 0 is the warm-up
        eng = Engine(device=0, key_capacity=[1024, 1024, 1024, 1024, max(a.n, 1024)])
        # room for the worst case of every put below (a put counts each item as new): no growth inside a timed call
        eng.ujson_leaves_reserve(2 * a.n + 16384, 80 * (a.n + 8192))
        dwb, dwo = torch.from_numpy(warm_b).to(dev), torch.from_numpy(warm_o.view(np.int64)).to(dev)
        eng.ujson_leaves_put(dwb, dwo)  # kernels loaded
        eng.ujson_leaves_get(eng.ujson_leaves_put(dwb, dwo), device=True)
        dlb, dlo = torch.from_numpy(lb).to(dev), torch.from_numpy(lo.view(np.int64)).to(dev)
        h = timed(eng, "put_first", lambda: eng.ujson_leaves_put(dlb, dlo))
        h2 = timed(eng, "put_again", lambda: eng.ujson_leaves_put(dlb, dlo))
        assert eng.ujson_leaves_usage()[0] == a.n + 4096 and torch.equal(h, h2)
        need = timed(eng, "get_size", lambda: eng.ujson_leaves_get_caps(h, 0, device=True))[0]
        assert need == [24 * a.n, 0], need
        out = (torch.empty(need[0], dtype=torch.uint8, device=dev), torch.empty(a.n + 1, dtype=torch.int64, device=dev))
        timed(eng, "get", lambda: eng.ujson_leaves_get_caps(h, need[0], device=True, out=out))
        assert torch.equal(out[0], dlb)
        eng.intern(UJSON, (kb, ko))
        caps, _ = eng.state_wire_caps(UJSON, 0, a.n, [0] * len(WIRE_SIZES[UJSON]), device=True)
        timed(eng, "keys_wire", lambda: eng.state_wire_caps(UJSON, 0, a.n, caps, device=True))
        eng.close()
    res = {"n": a.n, "leaf_bytes": 24, "reps": a.reps}
    for k, v in runs.items():
        res[k + "_ms"], res[k + "_runs"] = statistics.median(v[1:]), v[1:]
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
