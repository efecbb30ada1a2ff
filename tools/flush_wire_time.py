"""Timing of the wire-form flush (jy_treg_flush_wire) against the path it
replaces, on one engine: N pending TREG keys, 16-byte keys, 24-byte values
(config 3's key shape at one eighth of a shard with the default N = 1M).

  (a) wire flush into device memory, HIP events on the engine stream
  (b) wire flush into host memory, wall clock
  (c) the slot-form path, RepoTREG.flush_deltas as it stands: jy_treg_flush
      (JY_HOST), jy_keys_export of the shard's names (the host name table is
      dropped before each run, as on a shard whose keys were interned on the
      device), one jy_arena_read per value.  Run at --slot-n pending keys
      (default 64K) and scaled linearly to N: its per-value round trips make
      1M slow.
  balance: 4,096 pending keys with one 70,000-byte value among 8-byte ones
      against 4,096 keys of the same total bytes, both as (a).

Every figure is the median of --reps runs after --warmup runs; the pending
set is rebuilt (one SET batch with a later timestamp) before each run.
Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _fixed(prefix, n, width):
    """n distinct byte strings of `width` bytes as (uint8 bytes, uint64 offsets)"""
    idx = np.arange(n, dtype=np.uint64)
    buf = np.full((n, width), ord("."), np.uint8)
    buf[:, :len(prefix)] = np.frombuffer(prefix, np.uint8)
    for d in range(10):  # decimal digits of the index at the tail
        buf[:, width - 1 - d] = (48 + (idx // np.uint64(10 ** d)) % np.uint64(10)).astype(np.uint8)
    return buf.reshape(-1), (np.arange(n + 1, dtype=np.uint64) * np.uint64(width))


class Bed:
    def __init__(self, n, vals, key_width=16):
        from jylis_amd.engine import Engine
        self.n = n
        self.eng = Engine(device=0, key_capacity=max(n, 1024), arena_capacity=max(int(vals[1][-1]) * 2, 1 << 16))
        self.slots = self.eng.intern(2, _fixed(b"key:", n, key_width))
        self.pre, self.lr = self.eng.pack_values(2, vals)
        self.ts = 0

    def mark(self):
        self.ts += 1
        self.eng.treg_set(self.slots, np.full(self.n, self.ts, np.uint64), self.pre, self.lr)
        self.eng.sync()

    def close(self):
        self.eng.close()


def timed_device(bed, reps, warmup):
    import torch
    stream = torch.cuda.ExternalStream(bed.eng.stream())
    out = []
    for r in range(warmup + reps):
        bed.mark()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        w = bed.eng.flush_wire(2, device=True)
        t1.record(stream)
        t1.synchronize()
        assert w["key_offs"].numel() == bed.n + 1
        if r >= warmup:
            out.append(t0.elapsed_time(t1))
    return statistics.median(out), out


def timed_host(bed, reps, warmup, fn):
    out = []
    for r in range(warmup + reps):
        bed.mark()
        t0 = time.perf_counter()
        t = fn()
        dt = (time.perf_counter() - t0) * 1e3
        assert len(t["key_offs"]) == bed.n + 1
        if r >= warmup:
            out.append(dt)
    return statistics.median(out), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--slot-n", type=int, default=1 << 16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    from jylis_amd.repo import RepoTREG

    res = {"n": a.n, "key_bytes": 16, "value_bytes": 24, "reps": a.reps, "warmup": a.warmup}
    bed = Bed(a.n, _fixed(b"value:", a.n, 24))
    res["a_wire_device_ms"], res["a_runs"] = timed_device(bed, a.reps, a.warmup)
    res["b_wire_host_ms"], res["b_runs"] = timed_host(bed, a.reps, a.warmup, lambda: bed.eng.flush_wire(2))
    bed.close()
    # per key: 16 B of key read + 16 B written, 24 B of value read + 24 B written, ~36 B of records and
    # offsets (kref 8, ts 8, key_offs 8, val_offs 8, slot 4), and the peek of the pending registers
    # (flag 4 + ts 8 + handle 16 read, the same cleared: the slot-form flush's own traffic)
    algo = a.n * (16 * 2 + 24 * 2 + 36 + 2 * 28)
    res["a_algorithmic_bytes"] = algo
    res["a_algorithmic_GBps"] = algo / (res["a_wire_device_ms"] * 1e-3) / 1e9

    bed = Bed(a.slot_n, _fixed(b"value:", a.slot_n, 24))
    repo = RepoTREG(bed.eng)

    def slot_form():
        del repo.names[:]  # the shard's names come from the device directory (jy_keys_export)
        return repo.flush_deltas()
    ms, runs = timed_host(bed, a.reps, a.warmup, slot_form)
    bed.close()
    res["c_slot_form_n"], res["c_slot_form_ms_at_n"], res["c_runs"] = a.slot_n, ms, runs
    res["c_slot_form_ms_scaled"] = ms * a.n / a.slot_n
    res["ratio_c_over_b"] = res["c_slot_form_ms_scaled"] / res["b_wire_host_ms"]

    # balance: the same output bytes as one long value among short ones, and spread evenly
    nb = 4096
    lens = np.full(nb, 8, np.uint64)
    lens[nb // 2] = 70000
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    body = np.random.default_rng(1).integers(0, 256, int(offs[-1])).astype(np.uint8)
    bed = Bed(nb, (body, offs))
    res["balance_long_ms"], res["balance_long_runs"] = timed_device(bed, a.reps, a.warmup)
    bed.close()
    each = int(offs[-1]) // nb
    bed = Bed(nb, (body[:each * nb], np.arange(nb + 1, dtype=np.uint64) * np.uint64(each)))
    res["balance_even_ms"], res["balance_even_runs"] = timed_device(bed, a.reps, a.warmup)
    bed.close()
    res["balance_value_bytes"] = [int(offs[-1]), each * nb]
    res["balance_ratio"] = res["balance_long_ms"] / res["balance_even_ms"]

    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
