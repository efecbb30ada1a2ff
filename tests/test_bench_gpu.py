"""bench.py end to end on a small shard: a plain run prints the headline line
without the --full legs, and --dump-outputs writes the converged state of its
seeded stream (recomputed here in numpy)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_dumps_the_converged_state(tmp_path):
    import bench
    from jylis_amd import synth as S
    # more keys than the dump writes whole (windows are sampled); even, so the
    # headline's vector kernel runs, and no multiple of its 512-cell tile
    K, R, nb, W, N = 20002, 8, 2, 1, 2
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(N), "--warmup",
                        str(W), "--keys", str(K), "--replicas", str(R), "--batches", str(nb), "--dump-outputs",
                        str(tmp_path / "out")], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["metric"] == bench.METRIC and line["unit"] == "merges/s" and line["dtype"] == "u64"
    assert line["higher_is_better"] is True and line["steps"] == N and line["warmup"] == W
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(2 * R * K * 1e3 / line["ms_per_step"])
    for k in ("cpu_baseline", "cpu_baseline_parallel", "first_cycle_changes", "verified"):
        assert k not in line  # --full only

    seed = S.BASE_SEED + 2
    best = chain = S.counter_state_np(K, R, 2, seed)
    applied = {i % nb for i in range(W + N)}
    for j in range(max(applied) + 1):
        chain = S.counter_delta_np(chain, j, seed)
        if j in applied:
            best = np.maximum(best, chain)
    slots = np.concatenate([np.arange(s0, s0 + n) for s0, n in bench.dump_slots(K)])
    got = {f[:-4]: np.load(tmp_path / "out" / f) for f in sorted(os.listdir(tmp_path / "out"))}
    assert sorted(got) == ["slots", "state_hi32", "state_lo32", "value_hi32", "value_lo32"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    assert got["slots"].tolist() == slots.tolist()

    def u64(name):
        return (got[name + "_hi32"].astype(np.uint64) << np.uint64(32)) | got[name + "_lo32"].astype(np.uint64)
    assert np.array_equal(u64("state"), best[:, :, slots])
    want = best[0].sum(axis=0, dtype=np.uint64) - best[1].sum(axis=0, dtype=np.uint64)
    assert np.array_equal(u64("value"), want[slots])
