"""Timing of RESP execute with UJSON INS / RM decoded and applied on the device
(UJSONDocs.resp_exec(ujson_write=True): jy_resp_exec_opts with
JY_RESP_UJSON_WRITE, one jy_ujson_write_keys per group) against the same call
without the write flag, where every UJSON write is a JY_CMD_HOST command
answered by the UJSONDocs.apply callback: the same documents on two engines
(the writes change state, so each variant keeps its own), the same request
bytes, wall-clock ms per heartbeat (the call, its waits, the callbacks and the
copy of the replies to the host).

Documents: the population of tools/resp_exec_ujson_time.py -- --docs documents
with Zipf distributed sizes and one of --big elements.  A heartbeat is --conns
connections of one UJSON INS and one UJSON RM each (the RM removes what the INS
added), documents picked with Zipf popularity, so popular documents repeat
inside a group and the keyed write runs several rounds.

After a warm-up round, --rounds rounds alternate the two variants in one
process; each figure is the median over the rounds, with the runs and their
spread (min, max) beside it, and the keyed calls and rounds of a heartbeat from
jy_ujson_write_keys_info.  On the warm-up round the replies and the written
documents of the two engines are checked to be equal.  --bench FILE merges
recorded `python bench.py` lines ({"label": ..., "result": {...}} a line) into
the output.  --out writes the JSON."""
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
IDENT = 0x5EED


def request(*words):
    return b"*%d\r\n" % len(words) + b"".join(b"$%d\r\n%s\r\n" % (len(w), w) for w in words)


def main():
    import torch
    from jylis_amd import ujson_doc as U
    from jylis_amd.engine import Engine, encode_keys, pack_dot
    from jylis_amd.repo import RepoUJSON
    from ujson_get_resp_time import leaves_of
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1 << 14)
    ap.add_argument("--big", type=int, default=20_000)
    ap.add_argument("--conns", type=int, nargs="+", default=[16, 256, 2048])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--zipf", type=float, default=2.0)
    ap.add_argument("--bench")
    ap.add_argument("--out")
    a = ap.parse_args()
    rng = np.random.default_rng(7)
    sizes = np.minimum(rng.zipf(a.zipf, a.docs), 1024).astype(np.int64)
    sizes = np.append(sizes, a.big)
    D = len(sizes)
    eo = np.zeros(D + 1, np.uint64)
    eo[1:] = np.cumsum(sizes, dtype=np.uint64)
    nel = int(eo[-1])
    lb = np.frombuffer(b"".join(b"".join(leaves_of(d, int(n))) for d, n in enumerate(sizes)), np.uint8)
    lo = np.arange(nel + 1, dtype=np.uint64) * np.uint64(37)

    def populated():
        eng = Engine(device=0, key_capacity=[1024, 1024, 1024, 1024, D + 1024])
        eng.ujson_leaves_reserve(nel + 1024, 40 * nel + (1 << 16))
        handles = eng.ujson_leaves_put(lb, lo)
        assert (handles != 0).all()
        slots = eng.intern(UJSON, encode_keys([b"doc:%07d" % d for d in range(D)]))
        col = int(eng.replica_cols([IDENT])[0])
        seq = np.arange(1, nel + 1, dtype=np.uint64) - np.repeat(eo[:-1], sizes)
        eng.ujson_converge(slots, eo, pack_dot(np.full(nel, col), seq), handles, np.arange(D + 1, dtype=np.uint64),
                           pack_dot(np.full(D, col), sizes.astype(np.uint64)), np.zeros(D + 1, np.uint64),
                           np.zeros(0, np.uint64))
        eng.sync()
        return eng, U.UJSONDocs(U.GpuDocs(RepoUJSON(eng)), IDENT, U.DeviceLeaves(eng))

    (eng_a, docs_a), (eng_b, docs_b) = populated(), populated()

    def heartbeat(nconn):
        pop = (rng.zipf(1.1, nconn) - 1) % a.docs
        conns, touched = [], set()
        for c in range(nconn):
            key = b"doc:%07d" % int(pop[c])
            touched.add(key)
            leaf = (key, b"w", b"c%d" % c, b'"beat"')
            conns.append(request(b"UJSON", b"INS", *leaf) + request(b"UJSON", b"RM", *leaf))
        return conns, sorted(touched)

    def on_device(conns):
        return docs_a.resp_exec(conns, IDENT, ujson_write=True)

    def by_callback(conns):
        return docs_b.resp_exec(conns, IDENT)

    def wall(eng, fn, conns):
        eng.sync()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn(conns)
        return (time.perf_counter() - t0) * 1e3, r

    rows = {}
    for nconn in a.conns:
        conns, touched = heartbeat(nconn)
        row = rows.setdefault(str(nconn), {"connections": nconn, "commands": 2 * nconn, "documents": len(touched),
                                           "request_bytes": sum(map(len, conns)), "on_device_runs": [],
                                           "by_callback_runs": []})
        for r in range(a.rounds + 1):  # round 0 is the warm-up
            i0 = eng_a.ujson_write_keys_info()
            ta, ra = wall(eng_a, on_device, conns)
            i1 = eng_a.ujson_write_keys_info()
            tb, rb = wall(eng_b, by_callback, conns)
            if r:
                row["on_device_runs"].append(round(ta, 3))
                row["by_callback_runs"].append(round(tb, 3))
            else:
                row["keyed_calls"] = i1["calls"] - i0["calls"]
                row["rounds"] = i1["rounds_total"] - i0["rounds_total"]
                assert ra == rb and all(x == (b"+OK\r\n" * 2, len(c), False) for x, c in zip(ra, conns))
                sa, sb = docs_a.b.r.slots_of(touched), docs_b.b.r.slots_of(touched)
                assert (sa == sb).all()
                for x, y in zip(eng_a.ujson_read(sa), eng_b.ujson_read(sb)):
                    assert (x == y).all()
                assert eng_a.ujson_deltas_size() == eng_b.ujson_deltas_size() >= len(touched)
        for name in ("on_device", "by_callback"):
            runs = row[name + "_runs"]
            row[name + "_ms"] = statistics.median(runs)
            row[name + "_spread"] = [min(runs), max(runs)]
        row["ratio_callback_over_device"] = round(row["by_callback_ms"] / row["on_device_ms"], 2)
    res = {"docs": D, "elements": nel, "big": a.big, "rounds": a.rounds, "rows": rows,
           "not_measured": "device request bytes; heartbeats that mix UJSON writes with other commands; a node of "
                           "several shards; a per-kernel trace"}
    if a.bench and os.path.exists(a.bench):
        res["bench"] = [json.loads(line) for line in open(a.bench) if line.strip()]
    eng_a.close()
    eng_b.close()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
