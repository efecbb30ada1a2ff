"""Timing of the RESP request decoder (jy_resp_decode) against the same rules run
sequentially on one CPU core, ms per whole batch:

  (a) decode       Engine.resp_decode(buffer, device=True): every engine call of
                   the decode (the sizing call too, when the capacities of the
                   last decode do not fit), its waits, the group table's copy to
                   the host; wall clock around the call and a sync.  Measured
                   with the request bytes in host memory (staged by the call)
                   and already in device memory.
  (b) sequential   tests/resp_in_check.cpp -- jy_resp_in.hpp as plain C++, -O2,
                   no sanitizer -- framing and classifying the same buffer one
                   connection and one token after the other, as a child
                   process; its own clock around the decode loop (reading the
                   file is not counted).  It gathers no key or value bytes and
                   sorts no rows: the floor of any host parser.

Workloads: --commands connections with one TREG SET each, values of 4 to 40
bytes ("heartbeat"), and the same commands pipelined on one connection
("pipelined").  After a warm-up round, --rounds rounds alternate the variants
in one process; each figure is the median over the rounds, listed with its
runs.  (a) and (b) are checked to count the same commands, rows and bytes.
--out writes the JSON."""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def request(*words):
    ws = [w if isinstance(w, bytes) else str(w).encode() for w in words]
    return b"*%d\r\n" % len(ws) + b"".join(b"$%d\r\n%s\r\n" % (len(w), w) for w in ws)


def build_seq(tmp):
    cc = next((p for p in (shutil.which(c) for c in (os.environ.get("CXX") or "g++", "c++", "clang++")) if p), None)
    if cc is None:
        raise SystemExit("no host C++ compiler for variant (b)")
    exe = os.path.join(tmp, "resp_in_seq")
    subprocess.run([cc, "-std=c++17", "-O2", "-o", exe, os.path.join(ROOT, "tests", "resp_in_check.cpp")], check=True)
    return exe


def main():
    import torch
    from jylis_amd.engine import Engine
    ap = argparse.ArgumentParser()
    ap.add_argument("--commands", type=int, default=1 << 16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seq", help="a built tests/resp_in_check.cpp (default: built here with the host compiler)")
    ap.add_argument("--out")
    a = ap.parse_args()
    rng = np.random.default_rng(5)
    n = a.commands
    vlen = rng.integers(4, 41, n)
    cmds = [request("TREG", "SET", b"reg:%07d" % i, bytes(rng.integers(97, 123, int(vlen[i]), dtype=np.uint8)),
                    int(rng.integers(1, 2**40))) for i in range(n)]
    req = b"".join(cmds)
    heart = np.zeros(n + 1, np.uint64)
    heart[1:] = np.cumsum([len(c) for c in cmds], dtype=np.uint64)
    loads = {"heartbeat": heart, "pipelined": np.array([0, len(req)], np.uint64)}

    tmp = tempfile.mkdtemp(prefix="resp_decode_time_")
    seq = a.seq or build_seq(tmp)
    files = {}
    for name, offs in loads.items():
        files[name] = os.path.join(tmp, name + ".bin")
        with open(files[name], "wb") as f:
            f.write(np.uint64(len(offs) - 1).tobytes() + offs.tobytes() + req)

    eng = Engine(device=0)
    hreq = np.frombuffer(req, np.uint8)
    dreq = torch.from_numpy(hreq.copy()).to(f"cuda:{eng.device}")
    rows = {}

    def wall(fn):
        eng.sync()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        eng.sync()
        return (time.perf_counter() - t0) * 1e3, r

    for rnd in range(a.rounds + 1):  # round 0 is the warm-up
        for name, offs in loads.items():
            row = rows.setdefault(name, {"connections": len(offs) - 1, "commands": n, "request_bytes": len(req)})
            for variant, src in (("decode_host_in", hreq), ("decode_device_in", dreq)):
                t, d = wall(lambda: eng.resp_decode((src, offs), device=True))
                assert d["sizes"][0] == n and d["sizes"][2] == n and d["sizes"][5] == 1, d["sizes"]
                if rnd:
                    row.setdefault(variant + "_runs", []).append(round(t, 3))
            used = int(d["conn_used"].sum().item())
            out = subprocess.run([seq, files[name], "1"], capture_output=True, text=True, check=True)
            s = json.loads(out.stdout)
            assert s["commands"] == n and s["rows"] == n and s["used"] == used == len(req) and s["closed"] == 0
            if rnd:
                row.setdefault("sequential_runs", []).append(round(s["ms"], 3))
    for row in rows.values():
        for v in ("decode_host_in", "decode_device_in", "sequential"):
            row[v + "_ms"] = statistics.median(row[v + "_runs"])
    res = {"commands": n, "value_len": [4, 40], "rounds": a.rounds,
           "sequential": "tests/resp_in_check.cpp, -O2, one core: frames and classifies, gathers and sorts nothing",
           "rows": rows}
    eng.close()
    shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
