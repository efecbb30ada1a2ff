"""Timing of UJSON GET as reply bytes rendered on the device
(jy_ujson_get_resp) against what it replaces, on one engine and the same
documents, wall-clock ms per whole batch of GETs (every engine call, its waits
and its copies to the host included):

  (a) get_resp   Engine.ujson_get_resp: key strings and paths in, reply bytes
                 out (the sizing call and the fill call of a first read; one
                 call once the capacity is known)
  (b) replaced   UJSONDocs.get_paths -- one path read, every relative leaf
                 copied to the host, decoded, put into a tree and printed --
                 plus the `$<len>\\r\\n...\\r\\n` framing a caller adds

Workloads, both over the population of tools/ujson_path_time.py (--docs
documents with Zipf distributed sizes and one document of --big elements, every
leaf at a path (top, sub, key)):
  big     the big document and --queries - 1 others picked with Zipf popularity
  small   --small documents picked uniformly among those of at most 8 leaves
each at the paths (), (top,) and (top, sub).  After a warm-up round, --rounds
rounds alternate (a) and (b) in one process; each figure is the median over the
rounds, listed with its runs.  (a) and (b) are checked to give canonically
equal texts on the warm-up round.  --out writes the JSON."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
UJSON = 4
TOPS, SUBS = 4, 25


def leaves_of(doc, n):
    """the n leaves of document `doc`: fixed-width encodings, 37 bytes each"""
    return [b"\x02\x00\x00\x00t%d\x03\x00\x00\x00s%02d\x0a\x00\x00\x00%010d\xff\xff\xff\xff1%05d"
            % (i % TOPS, (i // TOPS) % SUBS, (doc * 7 + i) % 10**10, i % 10**5) for i in range(n)]


def main():
    import torch
    from jylis_amd.engine import Engine, encode_keys, pack_dot
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1 << 16)
    ap.add_argument("--big", type=int, default=100_000)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--small", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--zipf", type=float, default=2.0)
    ap.add_argument("--out")
    a = ap.parse_args()
    rng = np.random.default_rng(7)
    sizes = np.minimum(rng.zipf(a.zipf, a.docs), 1024).astype(np.int64)
    sizes = np.append(sizes, a.big)  # the last document is the big one
    D = len(sizes)
    eo = np.zeros(D + 1, np.uint64)
    eo[1:] = np.cumsum(sizes, dtype=np.uint64)
    nel = int(eo[-1])
    raw = b"".join(b"".join(leaves_of(d, int(n))) for d, n in enumerate(sizes))
    lb = np.frombuffer(raw, np.uint8)
    lo = np.arange(nel + 1, dtype=np.uint64) * np.uint64(37)
    assert len(lb) == 37 * nel

    eng = Engine(device=0, key_capacity=[1024, 1024, 1024, 1024, D + 1024])
    eng.ujson_leaves_reserve(nel + 1024, 40 * nel + (1 << 16))
    handles = eng.ujson_leaves_put(lb, lo)
    assert (handles != 0).all()
    slots = eng.intern(UJSON, encode_keys([b"doc:%07d" % d for d in range(D)]))
    col = int(eng.replica_cols([0x5EED])[0])
    seq = np.arange(1, nel + 1, dtype=np.uint64) - np.repeat(eo[:-1], sizes)
    vo = np.arange(D + 1, dtype=np.uint64)
    eng.ujson_converge(slots, eo, pack_dot(np.full(nel, col), seq), handles, vo,
                       pack_dot(np.full(D, col), sizes.astype(np.uint64)), np.zeros(D + 1, np.uint64),
                       np.zeros(0, np.uint64))
    eng.sync()
    assert eng.skipped() == 0

    from jylis_amd import ujson_doc as U
    from jylis_amd.repo import RepoUJSON
    docs = U.UJSONDocs(U.GpuDocs(RepoUJSON(eng)), 0x5EED, U.DeviceLeaves(eng))
    key_of = lambda d: b"doc:%07d" % d
    pop = np.unique((rng.zipf(1.1, 8 * a.queries) - 1) % a.docs)[:a.queries - 1]
    small = rng.choice(np.nonzero(sizes[:-1] <= 8)[0], a.small, replace=False)
    loads = {"big": [key_of(d) for d in sorted(pop.tolist())] + [key_of(D - 1)],
             "small": [key_of(d) for d in small.tolist()]}
    leaves = {"big": int(sizes[pop].sum() + a.big), "small": int(sizes[small].sum())}
    paths = {"all": (), "quarter": ("t0",), "hundredth": ("t0", "s07")}

    def get_resp(keys, p):
        r = eng.ujson_get_resp(keys, [p] * len(keys))
        assert r["sizes"][4] == 0 and r["sizes"][5] == 0
        return r["reply_bytes"].tobytes(), r["reply_offs"], r["sizes"]

    def replaced(keys, p):
        texts = docs.get_paths([k.decode() for k in keys], [p] * len(keys))
        out = []
        for t in texts:
            t = t.encode()
            out.append(b"$%d\r\n%s\r\n" % (len(t), t))
        return out

    def wall(fn):
        eng.sync()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        return (time.perf_counter() - t0) * 1e3, r

    rows = {}
    for r in range(a.rounds + 1):  # round 0 is the warm-up
        for load, keys in loads.items():
            for name, p in paths.items():
                ta, (rb, ro, sz) = wall(lambda: get_resp(keys, p))
                tb, old = wall(lambda: replaced(keys, p))
                row = rows.setdefault(f"{load}/{name}", {"path": list(p), "queries": len(keys),
                                                         "leaves_in_documents": leaves[load], "examined": sz[3],
                                                         "leaves_rendered": sz[2], "reply_bytes": sz[0],
                                                         "get_resp_runs": [], "replaced_runs": []})
                if r:
                    row["get_resp_runs"].append(round(ta, 3))
                    row["replaced_runs"].append(round(tb, 3))
                else:  # the two variants answer alike
                    ro = [int(x) for x in ro]
                    assert len(old) == len(keys) and sum(map(len, old)) == len(rb)
                    for i in range(0, len(keys), max(1, len(keys) // 64)):
                        got = rb[ro[i]:ro[i + 1]]
                        text = lambda b: U.canonical(b[b.index(b"\r\n") + 2:-2].decode())
                        assert text(got) == text(old[i]), (load, name, i)
    for row in rows.values():
        row["get_resp_ms"] = statistics.median(row["get_resp_runs"])
        row["replaced_ms"] = statistics.median(row["replaced_runs"])
        row["speedup"] = round(row["replaced_ms"] / row["get_resp_ms"], 2)
    res = {"docs": D, "elements": nel, "big": a.big, "rounds": a.rounds, "rows": rows,
           "not_measured": "device outputs (device=True) and device key strings; a node of several shards"}
    eng.close()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
