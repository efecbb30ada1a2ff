"""Timing of the keyed TLOG reads (jy_tlog_get_keys) against the reads they
replace, on one engine, wall-clock ms per whole read (every engine call of the
read, its waits and its copies to the host included):

  (a) get_keys    Engine.tlog_get_keys(keys, counts): lookup, sizing, entry
                  gather and value bytes in one call (two when the answer
                  outgrew the capacities of the read before)
  (b) replaced    Engine.lookup + Engine.tlog_read (sizes + every entry of every
                  log) + one Engine.value_bytes per RETURNED entry (a blocking
                  jy_arena_read for each value over 8 bytes) -- what RepoTLOG.get
                  did; host outputs only, it has no device form
  (c) wire_slots  Engine.state_wire_slots of the same slots, for count = all
                  only (it has no count): the one batched path to value bytes
                  there was; returns the key strings too

Workload: --logs logs whose lengths are Zipf distributed (clipped), plus one
log of --big entries; values of 4 to 40 bytes.  A query is the big log and
--queries - 1 others picked with Zipf popularity.  Counts 1, 10 and all;
outputs to the host and to the device.  After a warm-up round, --rounds rounds
alternate (a), (b) and (c) in one process; each figure is the median over the
rounds, listed with its runs and with the bytes that reached the host.
--out writes the JSON."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TLOG = 3
ALL = 2**64 - 1


def main():
    import torch
    from jylis_amd.engine import Engine
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", type=int, default=1 << 16)
    ap.add_argument("--big", type=int, default=100_000)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--zipf", type=float, default=2.0)
    ap.add_argument("--out")
    a = ap.parse_args()
    rng = np.random.default_rng(11)
    lens = np.minimum(rng.zipf(a.zipf, a.logs), 1024).astype(np.int64)
    lens = np.append(lens, a.big)  # the last log is the long one
    L = len(lens)
    eo = np.zeros(L + 1, np.uint64)
    eo[1:] = np.cumsum(lens, dtype=np.uint64)
    nent = int(eo[-1])
    # canonical logs: newest first, one entry per timestamp
    ts = (np.repeat(lens, lens) - (np.arange(nent) - np.repeat(eo[:-1].astype(np.int64), lens))).astype(np.uint64)
    vlen = rng.integers(4, 41, nent)
    vo = np.zeros(nent + 1, np.uint64)
    vo[1:] = np.cumsum(vlen, dtype=np.uint64)
    vb = rng.integers(97, 123, int(vo[-1]), dtype=np.uint8)

    eng = Engine(device=0, key_capacity=[1024, 1024, 1024, L + 1024, 1024], entry_capacity=2 * nent,
                 arena_capacity=2 * int(vo[-1]) + (1 << 20))
    keys = [b"log:%07d" % i for i in range(L)]
    slots = eng.intern(TLOG, keys)
    pre, lr = eng.pack_values(TLOG, (vb, vo))
    eng.tlog_converge(slots, np.zeros(L, np.uint64), eo, ts, pre, lr)
    eng.sync()
    assert eng.skipped() == 0

    pop = np.unique((rng.zipf(1.1, 8 * a.queries) - 1) % a.logs)[:a.queries - 1]
    qi = np.sort(np.append(pop, L - 1))
    q = [keys[i] for i in qi]
    nbytes = lambda arrs: int(sum(x.nbytes for x in arrs))

    def get_keys(count, device):
        cnt = None if count is None else np.full(len(q), count, np.uint64)
        r = eng.tlog_get_keys(q, cnt, device=device)
        if device:
            eng.sync()
        host = 0 if device else nbytes([r[k] for k in ("found", "size", "cutoff", "ent_offs", "ts", "val_bytes",
                                                       "val_offs")])
        return r["sizes"], host

    def replaced(count):
        s = eng.lookup(TLOG, q)
        cut, offs, t, p, l = eng.tlog_read(s)
        vals, got = 0, 0
        for i in range(len(q)):
            lo, hi = int(offs[i]), int(offs[i + 1])
            for j in range(lo, lo + min(hi - lo, ALL if count is None else count)):
                vals += len(eng.value_bytes(TLOG, p[j], l[j]))
                got += 1
        return [got, vals], nbytes((s, cut, offs, t, p, l)) + vals

    def wire_slots(device):
        s = np.sort(eng.lookup(TLOG, q))
        w = eng.state_wire_slots(TLOG, s, device=device)
        if device:
            eng.sync()
        return [len(w["ts"]), len(w["val_bytes"])], 0 if device else nbytes(w.values()) + s.nbytes

    def wall(fn):
        eng.sync()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        return (time.perf_counter() - t0) * 1e3, r

    rows = {}
    for r in range(a.rounds + 1):  # round 0 is the warm-up
        for device in (False, True):
            mem = "device" if device else "host"
            for name, count in (("1", 1), ("10", 10), ("all", None)):
                want = int((lens[qi] if count is None else np.minimum(lens[qi], count)).sum())
                ta, (sz, ba) = wall(lambda: get_keys(count, device))
                assert sz[0] == want, (sz, want)
                row = rows.setdefault(f"{name}/{mem}", {"count": name, "outputs": mem, "entries": sz[0],
                                                        "value_bytes": sz[1], "get_keys_host_bytes": ba,
                                                        "get_keys_runs": []})
                if r:
                    row["get_keys_runs"].append(round(ta, 3))
                if not device:
                    tb, (szb, bb) = wall(lambda: replaced(count))
                    assert szb == sz[:2], (szb, sz)
                    row["replaced_host_bytes"] = bb
                    if r:
                        row.setdefault("replaced_runs", []).append(round(tb, 3))
                if count is None:
                    tc, (szc, bc) = wall(lambda: wire_slots(device))
                    assert szc == sz[:2], (szc, sz)
                    row["wire_slots_host_bytes"] = bc
                    if r:
                        row.setdefault("wire_slots_runs", []).append(round(tc, 3))
    for row in rows.values():
        for v in ("get_keys", "replaced", "wire_slots"):
            if v + "_runs" in row:
                row[v + "_ms"] = statistics.median(row[v + "_runs"])
    res = {"logs": L, "entries": nent, "big": a.big, "queries": len(q), "queried_entries": int(lens[qi].sum()),
           "value_len": [4, 40], "rounds": a.rounds, "rows": rows}
    eng.close()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
