"""Timing of the RESP reply reads (jy_*_get_resp) against the keyed reads they
sit on, on one engine, wall-clock ms per whole read (every engine call of the
read, its waits and its copies to the host included):

  (a) get_resp     Engine.tlog_get_resp(keys, counts): the keyed read plus the
                   piece sizing, one scan and the reply writer; reply_bytes and
                   reply_offs leave the call
  (b) get_keys     Engine.tlog_get_keys(keys, counts) alone: the columns, not
                   formatted -- the floor of any host-formatting path
  (c) get_keys+fmt (b), then its columns formatted on the host by the host
                   mirror's Respond rules.  The formatter is this tool's own
                   Python over the numpy columns -- one bytes join with a
                   "%d" per number, a step per returned entry, as
                   RepoTLOG.get_many walks them; it is not compiled code.
                   Host outputs only.

Workload: the state and the queries of tools/get_keys_time.py (--logs Zipf(2)
logs plus one of --big entries, values of 4 to 40 bytes; the big log and
--queries - 1 others).  Counts 1, 10 and all; outputs to the host and to the
device.  Then TREG GET and PNCOUNT GET of --keys keys, (a) against (b).  After
a warm-up round, --rounds rounds alternate the variants in one process; each
figure is the median over the rounds, listed with its runs and with the bytes
that reached the host.  (a) and (c) are checked to produce the same bytes.
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
PNCOUNT, TREG, TLOG = 1, 2, 3


def format_tlog(r):
    """the columns of a tlog_get_keys answer as GET replies"""
    vb, vo, eo, ts = r["val_bytes"].tobytes(), r["val_offs"].tolist(), r["ent_offs"].tolist(), r["ts"].tolist()
    out = []
    for i in range(len(eo) - 1):
        out.append(b"*%d\r\n" % (eo[i + 1] - eo[i]))
        out += [b"*2\r\n$%d\r\n%s\r\n:%d\r\n" % (vo[j + 1] - vo[j], vb[vo[j]:vo[j + 1]], ts[j])
                for j in range(eo[i], eo[i + 1])]
    return b"".join(out)


def format_treg(r):
    vb, vo, ts, found = r["val_bytes"].tobytes(), r["val_offs"].tolist(), r["ts"].tolist(), r["found"].tolist()
    return b"".join(b"*2\r\n$%d\r\n%s\r\n:%d\r\n" % (vo[i + 1] - vo[i], vb[vo[i]:vo[i + 1]], ts[i]) if found[i]
                    else b"$-1\r\n" for i in range(len(ts)))


def main():
    import torch
    from jylis_amd.engine import Engine
    from jylis_amd.repo import RepoPNCOUNT, RepoTREG
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", type=int, default=1 << 16)
    ap.add_argument("--big", type=int, default=100_000)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--keys", type=int, default=1 << 16)
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
    ts = (np.repeat(lens, lens) - (np.arange(nent) - np.repeat(eo[:-1].astype(np.int64), lens))).astype(np.uint64)
    vlen = rng.integers(4, 41, nent)
    vo = np.zeros(nent + 1, np.uint64)
    vo[1:] = np.cumsum(vlen, dtype=np.uint64)
    vb = rng.integers(97, 123, int(vo[-1]), dtype=np.uint8)

    eng = Engine(device=0, key_capacity=[1024, a.keys + 1024, a.keys + 1024, L + 1024, 1024], entry_capacity=2 * nent,
                 arena_capacity=2 * int(vo[-1]) + (1 << 20))
    keys = [b"log:%07d" % i for i in range(L)]
    slots = eng.intern(TLOG, keys)
    pre, lr = eng.pack_values(TLOG, (vb, vo))
    eng.tlog_converge(slots, np.zeros(L, np.uint64), eo, ts, pre, lr)
    # TREG and PNCOUNT: --keys keys each, written through the keyed writes
    rkeys = [b"reg:%07d" % i for i in range(a.keys)]
    RepoTREG(eng, 7).set(rkeys, [bytes(vb[int(vo[i]):int(vo[i + 1])]) for i in range(a.keys)],
                         rng.integers(1, 2**40, a.keys).astype(np.uint64))
    pn = RepoPNCOUNT(eng, 7)
    pn.inc(rkeys, rng.integers(0, 2**40, a.keys).astype(np.uint64), 7)
    pn.dec(rkeys[::2], rng.integers(0, 2**41, a.keys // 2).astype(np.uint64), 7)
    eng.sync()
    assert eng.skipped() == 0

    pop = np.unique((rng.zipf(1.1, 8 * a.queries) - 1) % a.logs)[:a.queries - 1]
    qi = np.sort(np.append(pop, L - 1))
    q = [keys[i] for i in qi]
    nbytes = lambda arrs: int(sum(x.nbytes for x in arrs))

    def wall(fn):
        eng.sync()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        return (time.perf_counter() - t0) * 1e3, r

    def resp(call, device):
        r = call(device)
        if device:
            eng.sync()
        return r, 0 if device else nbytes([r["reply_bytes"], r["reply_offs"]])

    def cols(call, names, device, fmt=None):
        r = call(device)
        if device:
            eng.sync()
        return r, 0 if device else nbytes([r[k] for k in names]), fmt(r) if fmt else None

    TL = ("found", "size", "cutoff", "ent_offs", "ts", "val_bytes", "val_offs")
    rows = {}

    def record(row, name, t, keep):
        if keep:
            row.setdefault(name + "_runs", []).append(round(t, 3))

    for rnd in range(a.rounds + 1):  # round 0 is the warm-up
        for device in (False, True):
            mem = "device" if device else "host"
            for name, count in (("1", 1), ("10", 10), ("all", None)):
                cnt = None if count is None else np.full(len(q), count, np.uint64)
                want = int((lens[qi] if count is None else np.minimum(lens[qi], count)).sum())
                row = rows.setdefault(f"tlog/{name}/{mem}", {"read": "TLOG GET", "count": name, "outputs": mem,
                                                              "queries": len(q)})
                ta, (ra, ba) = wall(lambda: resp(lambda d: eng.tlog_get_resp(q, cnt, device=d), device))
                assert ra["sizes"][1] == want
                row.update(entries=want, reply_bytes=ra["sizes"][0], get_resp_host_bytes=ba)
                record(row, "get_resp", ta, rnd)
                tb, (rb, bb, _) = wall(lambda: cols(lambda d: eng.tlog_get_keys(q, cnt, device=d), TL, device))
                row.update(get_keys_host_bytes=bb)
                record(row, "get_keys", tb, rnd)
                if not device:
                    tc, (rc, bc, text) = wall(lambda: cols(lambda d: eng.tlog_get_keys(q, cnt, device=d), TL, device,
                                                           format_tlog))
                    assert text == ra["reply_bytes"].tobytes()
                    record(row, "get_keys_fmt", tc, rnd)
            for kind in ("treg", "pncount"):
                row = rows.setdefault(f"{kind}/{mem}", {"read": kind.upper() + " GET", "outputs": mem,
                                                        "queries": len(rkeys)})
                if kind == "treg":
                    ta, (ra, ba) = wall(lambda: resp(lambda d: eng.treg_get_resp(rkeys, device=d), device))
                    tb, (rb, bb, _) = wall(lambda: cols(lambda d: eng.treg_get_keys(rkeys, device=d),
                                                        ("found", "ts", "val_bytes", "val_offs"), device))
                    if rnd == 0 and not device:
                        assert format_treg(rb) == ra["reply_bytes"].tobytes()
                else:
                    ta, (ra, ba) = wall(lambda: resp(lambda d: eng.counter_get_resp(PNCOUNT, rkeys, device=d), device))

                    def pn_cols(d):
                        f, v = eng.counter_get_keys(PNCOUNT, rkeys, device=d)
                        return {"found": f, "out": v}
                    tb, (rb, bb, _) = wall(lambda: cols(pn_cols, ("found", "out"), device))
                    if rnd == 0 and not device:
                        assert b"".join(b":%d\r\n" % v for v in rb["out"].tolist()) == ra["reply_bytes"].tobytes()
                row.update(reply_bytes=ra["sizes"][0], get_resp_host_bytes=ba, get_keys_host_bytes=bb)
                record(row, "get_resp", ta, rnd)
                record(row, "get_keys", tb, rnd)
    for row in rows.values():
        for v in ("get_resp", "get_keys", "get_keys_fmt"):
            if v + "_runs" in row:
                row[v + "_ms"] = statistics.median(row[v + "_runs"])
    res = {"logs": L, "entries": nent, "big": a.big, "queries": len(q), "queried_entries": int(lens[qi].sum()),
           "keys": a.keys, "value_len": [4, 40], "rounds": a.rounds,
           "host_formatter": "this tool's Python over the numpy columns (bytes join, one step per entry)",
           "rows": rows}
    eng.close()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
