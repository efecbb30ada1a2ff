"""Timing of RESP execute end to end, ms per whole heartbeat, request bytes in
host memory to per-connection reply bytes in host memory:

  (a) exec       Engine.resp_exec(buffers, identity, on_host): jy_resp_exec and
                 jy_resp_replies, the replies assembled per connection on the
                 GPU and cut into one bytes object per connection here.
  (b) exec_resp  jylis_amd.resp_in.exec_resp on an engine of the same type with
                 the same buffers: the Python loop over the group table, one
                 keyed call per group, the replies cut per command and stitched
                 per connection on the host.  This was the only path before
                 jy_resp_exec: the baseline.

Workloads: --commands connections with one TREG SET each ("set"), as many
TREG GETs against that state ("get"), and ONE connection alternating SET / GET
for --alternating commands ("alternating": a phase per command, the worst
case).  Each variant has an engine of its own, so both execute every workload
on the same state.  After a warm-up round, --rounds rounds alternate the
variants in one process; each figure is the median over the rounds, listed with
its runs.  The two variants' replies are compared byte for byte in every round.
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


def request(*words):
    ws = [w if isinstance(w, bytes) else str(w).encode() for w in words]
    return b"*%d\r\n" % len(ws) + b"".join(b"$%d\r\n%s\r\n" % (len(w), w) for w in ws)


def main():
    import torch
    from jylis_amd.engine import Engine
    from jylis_amd.resp_in import exec_resp
    ap = argparse.ArgumentParser()
    ap.add_argument("--commands", type=int, default=1 << 16)
    ap.add_argument("--alternating", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    rng = np.random.default_rng(5)
    n = a.commands
    vlen = rng.integers(4, 41, n)
    loads = {
        "set": [request("TREG", "SET", b"reg:%07d" % i, bytes(rng.integers(97, 123, int(vlen[i]), dtype=np.uint8)),
                        int(rng.integers(1, 2**40))) for i in range(n)],
        "get": [request("TREG", "GET", b"reg:%07d" % i) for i in range(n)],
        "alternating": [b"".join(request("TREG", "SET", "alt", "v%d" % i, i + 1) if i % 2 == 0 else
                                 request("TREG", "GET", "alt") for i in range(a.alternating))],
    }
    engines = {"exec": Engine(device=0), "exec_resp": Engine(device=0)}
    no_host = lambda words: b""
    run = {"exec": lambda bufs: engines["exec"].resp_exec(bufs, 1, no_host),
           "exec_resp": lambda bufs: exec_resp(engines["exec_resp"], bufs, 1, no_host)}

    def wall(eng, fn):
        eng.sync()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        eng.sync()
        return (time.perf_counter() - t0) * 1e3, r

    rows = {}
    for rnd in range(a.rounds + 1):  # round 0 is the warm-up
        for name, bufs in loads.items():
            row = rows.setdefault(name, {"connections": len(bufs), "request_bytes": sum(map(len, bufs))})
            got = {}
            for variant in (("exec", "exec_resp") if rnd % 2 else ("exec_resp", "exec")):
                t, got[variant] = wall(engines[variant], lambda: run[variant](bufs))
                if rnd:
                    row.setdefault(variant + "_runs", []).append(round(t, 3))
            assert got["exec"] == got["exec_resp"], name
            row["reply_bytes"] = sum(len(r) for r, _, _ in got["exec"])
            sizes = engines["exec"].resp_exec_raw(bufs, 1, no_host) if rnd == 0 else None
            if sizes:  # (the warm-up round runs (a) once more to record what the call did)
                exec_resp(engines["exec_resp"], bufs, 1, no_host)  # keep the two states alike
                row.update(dict(zip(Engine.RESP_EXEC_SIZES, sizes)))
    for row in rows.values():
        for v in ("exec", "exec_resp"):
            row[v + "_ms"] = statistics.median(row[v + "_runs"])
        row["exec_resp_over_exec"] = round(row["exec_resp_ms"] / row["exec_ms"], 2)
    res = {"commands": n, "alternating": a.alternating, "value_len": [4, 40], "rounds": a.rounds,
           "baseline": "jylis_amd.resp_in.exec_resp: the path before jy_resp_exec", "rows": rows}
    for e in engines.values():
        e.close()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
