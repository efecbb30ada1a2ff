"""Timing of the keyed writes (jy_tlog_write_keys, jy_treg_set_keys) against the
path they replace, on one engine, wall-clock ms per whole write (every engine
call of the write and its waits included; the engine is synchronised before the
clock stops):

  (a) keys_host    the keyed call with host arrays
  (b) slot_path    Engine.intern + Engine.pack_values + Engine.tlog_write /
                   treg_set with host arrays: what the repos did (a TLOG batch
                   that repeats keys is split into host rounds by occurrence)
  (c) keys_device  the keyed call with device arrays (already in HBM)

Workloads, --n commands each, values of 4 to 40 bytes, unique timestamps:
  tlog/distinct    TLOG INS, every command its own key
  tlog/zipf        TLOG INS, Zipf(1.1) keys: one key repeats thousands of times
  treg/distinct, treg/zipf   the same keys as TREG SETs
Every run starts from a fresh engine.  After a warm-up round, --rounds rounds
alternate the variants in one process; each figure is the median over the
rounds, listed with its runs.  --out writes the JSON."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TREG, TLOG = 2, 3


def main():
    import torch
    from jylis_amd.engine import Engine, encode_keys
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--zipf", type=float, default=1.1)
    ap.add_argument("--out")
    a = ap.parse_args()
    n = a.n
    rng = np.random.default_rng(7)
    vlen = rng.integers(4, 41, n)
    vo = np.zeros(n + 1, np.uint64)
    vo[1:] = np.cumsum(vlen, dtype=np.uint64)
    vb = rng.integers(97, 123, int(vo[-1]), dtype=np.uint8)
    ts = (np.arange(n) + 1).astype(np.uint64)
    ops = np.zeros(n, np.uint8)
    arg = np.zeros(n, np.uint64)
    keysets = {"distinct": np.arange(n), "zipf": (rng.zipf(a.zipf, n) - 1) % n}

    def dev(x):
        x = np.ascontiguousarray(x)
        return torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).cuda()

    def run(ctype, form, variant):
        kb, ko = encode_keys([b"key:%07d" % i for i in keysets[form]])
        eng = Engine(device=0, key_capacity=[1024, 1024, n + 1024, n + 1024, 1024], entry_capacity=4 * n,
                     arena_capacity=4 * int(vo[-1]) + (1 << 20))
        try:
            if variant == "keys_device":
                cols = [dev(x) for x in (ops, kb, ko, ts, arg, vb, vo)]
            eng.sync()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if variant == "slot_path":
                slots = eng.intern(ctype, (kb, ko))
                pre, lr = eng.pack_values(ctype, (vb, vo))
                if ctype == TLOG:
                    eng.tlog_write(ops, slots, ts, arg, pre, lr)
                else:
                    eng.treg_set(slots, ts, pre, lr)
            elif variant == "keys_host":
                if ctype == TLOG:
                    eng.tlog_write_keys(ops, (kb, ko), ts, arg, (vb, vo))
                else:
                    eng.treg_set_keys((kb, ko), ts, (vb, vo))
            else:
                o, dkb, dko, dts, da, dvb, dvo = cols
                if ctype == TLOG:
                    eng.tlog_write_keys(o, (dkb, dko), dts, da, (dvb, dvo))
                else:
                    eng.treg_set_keys((dkb, dko), dts, (dvb, dvo))
            eng.sync()
            ms = (time.perf_counter() - t0) * 1e3
            rounds = eng.tlog_write_rounds()["last"] if ctype == TLOG and variant != "slot_path" else None
            return ms, eng.nkeys(ctype), rounds
        finally:
            eng.close()

    rows = {}
    for r in range(a.rounds + 1):  # round 0 is the warm-up
        for ctype, tname in ((TLOG, "tlog"), (TREG, "treg")):
            for form in ("distinct", "zipf"):
                row = rows.setdefault(f"{tname}/{form}", {"commands": n})
                for variant in ("keys_host", "slot_path", "keys_device"):
                    ms, nk, rounds = run(ctype, form, variant)
                    row["keys"] = nk
                    if rounds is not None:
                        row["rounds"] = rounds
                    if r:
                        row.setdefault(variant + "_runs", []).append(round(ms, 3))
    cnt = np.bincount(keysets["zipf"])
    for row in rows.values():
        for v in ("keys_host", "slot_path", "keys_device"):
            row[v + "_ms"] = statistics.median(row[v + "_runs"])
    res = {"commands": n, "value_len": [4, 40], "zipf": a.zipf, "zipf_hottest_key_repeats": int(cnt.max()),
           "rounds": a.rounds, "rows": rows}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
