"""Timing of RESP execute with UJSON GET decoded and rendered on the device
(Engine.resp_exec(ujson_get=True), jy_resp_exec_opts) against the same call
without the flag, where every UJSON GET is a JY_CMD_HOST command answered by
the UJSONDocs.apply callback: one engine, the same documents, the same request
bytes, wall-clock ms per heartbeat (the call, its waits, the callbacks and the
copy of the replies to the host).

Documents: the shape of tools/ujson_get_resp_time.py -- --docs documents with
Zipf distributed sizes and one of --big elements, every leaf at a path (top,
sub, key).  A heartbeat is --conns connections of --per-conn UJSON GETs each,
documents picked with Zipf popularity, paths cycling through (), (top,) and
(top, sub); one connection in 64 asks for the big document.

After a warm-up round, --rounds rounds alternate the two variants in one
process; each figure is the median over the rounds, with the runs and their
spread (min, max) beside it.  The replies of the two are checked to be
canonically equal on the warm-up round.  --bench FILE merges recorded
`python bench.py` lines ({"label": ..., "result": {...}} a line) into the
output, so the headline runs of a session stand beside these figures.
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
    ap.add_argument("--per-conn", type=int, default=2)
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
    docs = U.UJSONDocs(U.GpuDocs(RepoUJSON(eng)), IDENT, U.DeviceLeaves(eng))
    paths = [(), (b"t0",), (b"t0", b"s07")]

    def heartbeat(nconn):
        pop = (rng.zipf(1.1, nconn * a.per_conn) - 1) % a.docs
        conns = []
        for c in range(nconn):
            cmds = []
            for j in range(a.per_conn):
                d = D - 1 if (c % 64 == 0 and j == 0) else int(pop[c * a.per_conn + j])
                cmds.append(request(b"UJSON", b"GET", b"doc:%07d" % d, *paths[(c + j) % 3]))
            conns.append(b"".join(cmds))
        return conns

    def on_device(conns):
        return docs.resp_exec(conns, IDENT)

    def by_callback(conns):
        return eng.resp_exec(conns, IDENT, docs.apply)

    def wall(fn, conns):
        eng.sync()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn(conns)
        return (time.perf_counter() - t0) * 1e3, r

    def texts(reply):
        out, at = [], 0
        while at < len(reply):
            e = reply.index(b"\r\n", at)
            n = int(reply[at + 1:e])
            out.append(U.canonical(reply[e + 2:e + 2 + n].decode()))
            at = e + 2 + n + 2
        return out

    rows = {}
    for nconn in a.conns:
        conns = heartbeat(nconn)
        row = rows.setdefault(str(nconn), {"connections": nconn, "commands": nconn * a.per_conn,
                                           "request_bytes": sum(map(len, conns)), "on_device_runs": [],
                                           "by_callback_runs": []})
        for r in range(a.rounds + 1):  # round 0 is the warm-up
            ta, ra = wall(on_device, conns)
            tb, rb = wall(by_callback, conns)
            if r:
                row["on_device_runs"].append(round(ta, 3))
                row["by_callback_runs"].append(round(tb, 3))
            else:
                row["reply_bytes"] = sum(len(x[0]) for x in ra)
                assert [u for _, u, _ in ra] == [u for _, u, _ in rb] == [len(c) for c in conns]
                for i in range(0, nconn, max(1, nconn // 32)):
                    assert texts(ra[i][0]) == texts(rb[i][0]), i
        for name in ("on_device", "by_callback"):
            runs = row[name + "_runs"]
            row[name + "_ms"] = statistics.median(runs)
            row[name + "_spread"] = [min(runs), max(runs)]
        row["ratio_callback_over_device"] = round(row["by_callback_ms"] / row["on_device_ms"], 2)
    res = {"docs": D, "elements": nel, "big": a.big, "per_conn": a.per_conn, "rounds": a.rounds, "rows": rows,
           "not_measured": "device request bytes; UJSON writes in the heartbeat; a node of several shards"}
    if a.bench and os.path.exists(a.bench):
        res["bench"] = [json.loads(line) for line in open(a.bench) if line.strip()]
    eng.close()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
