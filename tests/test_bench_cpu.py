"""bench.py host logic that runs without a GPU: the hang watchdog exits
non-zero (a routed collective that hangs is a failure, not a clean line),
and the parallel CPU baseline sizes itself to the CPUs it may really use."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_watchdog_exits_nonzero():
    code = ("import sys, time; sys.path.insert(0, %r); import bench; "
            "bench.watchdog(0.3, {'metric': 'm', 'value': 1.0}, 0); time.sleep(20); print('not reached')" % ROOT)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=60)
    assert p.returncode == 3, (p.returncode, p.stdout, p.stderr)
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert "error" in line["routed"] and line["value"] == 1.0
    assert "not reached" not in p.stdout


def test_watchdog_cancelled_phase_exits_zero():
    code = ("import sys; sys.path.insert(0, %r); import bench; "
            "d = bench.watchdog(5.0, {}, 0); d.cancel(); print('done')" % ROOT)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.strip() == "done"


def test_cpu_share_is_the_usable_set():
    sys.path.insert(0, ROOT)
    import bench
    n, how = bench.cpu_share()
    assert 1 <= n <= (os.cpu_count() or 1)
    if hasattr(os, "sched_getaffinity"):
        assert n <= len(os.sched_getaffinity(0))
    assert "sched_getaffinity" in how or "cpu_count" in how


def test_launch_cmd_is_one_rank_per_gpu():
    sys.path.insert(0, ROOT)
    import bench
    cmd = bench.launch_cmd(["--gpus", "8", "--steps", "5"], 8, 29555)
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nnodes=1" in cmd and "--nproc-per-node=8" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[cmd.index("--master-port") + 1] == "29555"
    i = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[i + 1:] == ["--gpus", "8", "--steps", "5"]


def test_world_check():
    sys.path.insert(0, ROOT)
    import bench

    class A:
        gpus, backend = 2, "nccl"
    assert bench.world_check(A, 2, 8) is None
    assert "WORLD_SIZE" in bench.world_check(A, 1, 8)
    assert "visible" in bench.world_check(A, 2, 1)
    A.backend = "gloo"  # a rehearsal may put both ranks on one GPU
    assert bench.world_check(A, 2, 1) is None


def test_dump_slots_are_fixed_and_in_range():
    sys.path.insert(0, ROOT)
    import bench
    assert bench.dump_slots(4096) == [(0, 4096)]  # a small shard is written whole
    K = 16 * 1024 * 1024
    wins = bench.dump_slots(K)
    assert wins == bench.dump_slots(K)  # seeded: the same sample in every run
    assert len(wins) == bench.DUMP_WINDOWS
    assert all(0 <= s0 and s0 + n <= K and n == bench.DUMP_WINDOW for s0, n in wins)
    # two float64 halves of a [2][64][sampled] state stay under the 64 MB a dump may take
    assert 2 * 8 * 2 * 64 * sum(n for _, n in wins) <= 48 << 20


def test_halves_hold_u64_exactly():
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    a = np.array([0, 1, 2**32 - 1, 2**32, 2**53 + 1, 2**64 - 1], np.uint64)
    hi, lo = bench._halves(a)
    assert hi.dtype == lo.dtype == np.float64
    assert ((hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)).tolist() == a.tolist()
    hi, lo = bench._halves(np.array([-1, -2**63], np.int64))  # i64 bits
    assert hi.tolist() == [2.0**32 - 1, 2.0**31] and lo.tolist() == [2.0**32 - 1, 0.0]


def test_plain_run_is_the_default(monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 3
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


def _bench(env_extra, *argv):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(env_extra)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True,
                          timeout=300, env=env, cwd=ROOT)


def test_mismatched_world_exits_nonzero():
    p = _bench({"WORLD_SIZE": "1"}, "--gpus", "2")
    assert p.returncode == 2, (p.returncode, p.stderr)
    assert "WORLD_SIZE 1 but --gpus 2" in p.stderr and not p.stdout.strip()


def test_too_few_gpus_exits_nonzero():
    # no WORLD_SIZE: the launcher counts the GPUs in a child first (none here)
    p = _bench({}, "--gpus", "2")
    assert p.returncode == 2, (p.returncode, p.stderr)
    assert "GPU(s) visible" in p.stderr and not p.stdout.strip()
