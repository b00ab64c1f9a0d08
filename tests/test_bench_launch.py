"""bench.py's launcher (CPU, gloo): `--gpus N` without torch.distributed.run starts N ranks itself,
each rank joins a world of exactly N, and a world that does not match --gpus is an error."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env(**extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR",
                                                             "MASTER_PORT")}
    env.update(CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="1", **extra)
    return env


def _run(args, **extra):
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                          timeout=240, env=_env(**extra), cwd=ROOT)


def test_gpus_n_spawns_n_ranked_workers():
    r = _run(["--gpus", "3", "--check-launch"])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout            # only rank 0 prints
    d = json.loads(lines[0])
    assert d["world_size"] == 3 and d["n_gpus"] == 3 and d["backend"] == "gloo"
    assert sorted(x[0] for x in d["ranks"]) == [0, 1, 2]
    assert all(rk == lr for rk, lr, _ in d["ranks"])     # one node: local rank == rank


def test_single_process_default():
    r = _run(["--check-launch"])
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["world_size"] == 1 and d["ranks"] == [[0, 0, -1]]


def test_world_mismatch_fails():
    r = _run(["--gpus", "2", "--check-launch"], WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    assert r.returncode != 0 and "--gpus 2" in r.stderr


def test_strong_scaling_plan():
    sys.path.insert(0, ROOT)
    import bench
    a = bench.parse_args(["--gpus", "8", "--global-batch", "4096"])
    plans = [bench.batch_plan(a, 8, r, 512) for r in range(8)]
    assert all(p["B"] == 512 and p["scaling"] == "strong" and p["B_global"] == 4096 for p in plans)
    assert plans[3]["lo"] == 1536 and plans[3]["hi"] == 2048
    a = bench.parse_args(["--global-batch", "4096"])
    assert bench.batch_plan(a, 1, 0, 512)["B"] == 4096
    a = bench.parse_args(["--gpus", "4"])
    p = bench.batch_plan(a, 4, 2, 512)
    assert p["B"] == 512 and p["B_global"] == 2048 and p["scaling"] == "weak"


def test_plain_run_is_lean_and_full_restores_the_extras():
    """Without --full nothing but the timed steps runs (no instrumented pass, no CPU baseline);
    --full turns both back on, and its --no-* options still narrow it."""
    sys.path.insert(0, ROOT)
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.full, a.kernel_events, a.no_cpu_baseline, a.dump_outputs) == (False, False, True, None)
    assert (a.steps, a.warmup) == (7, 2)
    a = bench.parse_args(["--full"])
    assert (a.full, a.kernel_events, a.no_cpu_baseline) == (True, True, False)
    a = bench.parse_args(["--full", "--no-cpu-baseline", "--no-kernel-events"])
    assert (a.full, a.kernel_events, a.no_cpu_baseline) == (True, False, True)


def test_dump_outputs_writes_seeded_bounded_arrays(tmp_path):
    """--dump-outputs: float32 / float64 .npy files, the same from call to call, a fixed sample of an
    array over its share of the byte budget, nothing written without the option."""
    import types

    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    g = torch.Generator().manual_seed(3)
    big = torch.randn(bench.DUMP_BUDGET_BYTES // 4 // 3 + 1000, generator=g)    # over a third of the budget
    arrays = {"x": torch.randn(7, 3, generator=g), "e": torch.randn(5, generator=g).double(), "big": big,
              "none": None}
    bench.dump_outputs(types.SimpleNamespace(dump_outputs=None), 0, arrays)
    assert not list(tmp_path.iterdir())
    for d in ("a", "b"):
        bench.dump_outputs(types.SimpleNamespace(dump_outputs=str(tmp_path / d)), 0, arrays)
    got = {f: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(got) == ["big.npy", "e.npy", "x.npy"]
    assert got["x.npy"].dtype == np.float32 and np.array_equal(got["x.npy"], arrays["x"].numpy())
    assert got["e.npy"].dtype == np.float64 and np.array_equal(got["e.npy"], arrays["e"].numpy())
    assert got["big.npy"].shape == (bench.DUMP_BUDGET_BYTES // 3 // 4,)
    assert np.isin(got["big.npy"], big.numpy()).all()
    assert sum(a.nbytes for a in got.values()) <= bench.DUMP_BUDGET_BYTES
    assert all(np.array_equal(a, np.load(tmp_path / "b" / f)) for f, a in got.items())
    bench.dump_outputs(types.SimpleNamespace(dump_outputs=str(tmp_path / "a")), 2, {"x": arrays["x"]})
    assert os.path.exists(tmp_path / "a" / "x.rank2.npy")


def test_every_workload_is_registered():
    """Each --workload choice parses (row †g's segno_train included)."""
    sys.path.insert(0, ROOT)
    import bench
    for wl in ("egno", "segno", "segno_gravity", "egno_train", "segno_train", "egno_rollout", "sim_charged"):
        assert bench.parse_args(["--workload", wl]).workload == wl
