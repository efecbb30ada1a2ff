"""Timing of UJSON path reads (jy_ujson_path_read) against the reads they
replace, on one engine, wall-clock ms per whole read (every engine call of the
read, its waits and its copies to the host included):

  (a) path_read   Engine.ujson_path_read: the sizing call and the fill call
  (b) replaced    host outputs:   Engine.ujson_read (sizes + contents) of the same
                                  slots, then Engine.ujson_leaves_get of every
                                  element -- what UJSONDocs did before, with the
                                  host's decode-and-filter left out
                  device outputs: Engine.state_wire_slots(leaves=True, device=True)
                                  of the same slots, the only device-resident form
                                  of "the documents and their leaves"

Workload: --docs documents whose sizes are Zipf distributed (clipped), plus
one document of --big elements; every leaf has a path (top, sub, key) with 4
tops and 25 subs, so the path (top,) selects about 1/4 and (top, sub) about
1/100 of a document.  A query set is the big document and --queries - 1 other
documents picked with Zipf popularity, all with the same path.  After a warm-up,
--rounds rounds alternate (a) and (b) for every path and both output memories
in one process; each figure is the median over the rounds, listed with its runs
and with the bytes that reached the host.  --out writes the JSON."""
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
    return [b"\x02\x00\x00\x00t%d\x03\x00\x00\x00s%02d\x0a\x00\x00\x00%010d\xff\xff\xff\xff%06d"
            % (i % TOPS, (i // TOPS) % SUBS, (doc * 7 + i) % 10**10, i % 10**6) for i in range(n)]


def main():
    import torch
    from jylis_amd.engine import Engine, encode_keys, pack_dot
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1 << 16)
    ap.add_argument("--big", type=int, default=100_000)
    ap.add_argument("--queries", type=int, default=256)
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

    pop = np.unique((rng.zipf(1.1, 8 * a.queries) - 1) % a.docs)[:a.queries - 1]
    q = np.sort(np.append(slots[pop], slots[-1])).astype(np.uint32)
    examined = int(sizes[pop].sum() + a.big)
    paths = {"all": (), "quarter": ("t0",), "hundredth": ("t0", "s07")}
    nbytes = lambda arrs: int(sum(x.numel() * x.element_size() if hasattr(x, "numel") else x.nbytes for x in arrs))

    def path_read(p, device):
        sz, o, el, b, l = eng.ujson_path_read(q, [p] * len(q), True, device)
        if device:
            eng.sync()
        return sz, (0 if device else nbytes((o, el, b, l)))

    def replaced(device):
        if device:
            w = eng.state_wire_slots(UJSON, q, device=True, leaves=True)
            eng.sync()
            return len(w["elems"]), 0
        out = eng.ujson_read(q)
        b, l = eng.ujson_leaves_get(out[2])
        return len(out[2]), nbytes(out + (b, l))

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
            for name, p in paths.items():
                ta, (sz, ba) = wall(lambda: path_read(p, device))
                tb, (nb, bb) = wall(lambda: replaced(device))
                assert sz[2] == examined == nb and sz[3] == 0, (sz, examined, nb)
                row = rows.setdefault(f"{name}/{mem}", {"path": list(p), "outputs": mem, "matched": sz[0],
                                                        "matched_share": round(sz[0] / examined, 4),
                                                        "leaf_bytes": sz[1], "path_read_host_bytes": ba,
                                                        "replaced_host_bytes": bb, "path_read_runs": [],
                                                        "replaced_runs": []})
                if r:
                    row["path_read_runs"].append(round(ta, 3))
                    row["replaced_runs"].append(round(tb, 3))
    for row in rows.values():
        row["path_read_ms"] = statistics.median(row["path_read_runs"])
        row["replaced_ms"] = statistics.median(row["replaced_runs"])
        row["replaced_spread_ms"] = round(max(row["replaced_runs"]) - min(row["replaced_runs"]), 3)
    res = {"docs": D, "elements": nel, "big": a.big, "queries": len(q), "examined": examined, "leaf_len": 37,
           "rounds": a.rounds, "lds_staging": "not built", "rows": rows}
    eng.close()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
