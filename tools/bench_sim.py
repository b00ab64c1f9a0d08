"""Timings of the N-body simulators (csrc/nonode_sim.hip) on the GPU: the tiled multi-workgroup kernels at every
size, and beside them the resident one-workgroup kernels at N = 1,024. One JSON line per measurement on stdout and
appended to --out (DESIGN.md section 3.8.1 quotes them; raw lines in profiles/sim/bench_sim_tiled.jsonl).

python tools/bench_sim.py [--reps 5] [--shapes 1x1024,8x1024,1x4096,1x20000,1x100000] [--out FILE] [--limit 240]

The driver starts one child process per shape under a time limit of its own (timeout -k 10 LIMIT) and stops at the
first child that does not end cleanly: nothing more is started on a device after a fault or a hang. A child
(--child SxN) draws one random system per simulator on the device and times whole calls of the C entries with
device events: T steps of gravity, then T steps of charged, alternated `reps` times after one warm-up call of
each (at N <= 1,024 the resident and the tiled kernel alternate as well, in the same process). It reports the
median over the reps with the spread (min, max) beside it, as

  ms_per_step   call time / force evaluations of the call (the tiled entries launch one kernel per evaluation:
                T for gravity, T - 1 for charged; the resident kernels evaluate T + 1 and T times in one launch)
  gpairs_per_s  S N^2 pair interactions per force evaluation (self pairs included: the kernels are branch-free
                over j) over ms_per_step, in 10^9 pairs per second

Steps per call: chosen per shape so that a call lasts a good fraction of a second where it can; one step at
N = 100,000 is 10^10 pairs, so that shape runs few.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = "1x1024,8x1024,1x4096,1x20000,1x100000"


def steps_for(S, N):
    """Steps per timed call: about 2 x 10^11 pair interactions, at least 4 and at most 400 steps."""
    return int(min(400, max(4, 2e11 // (S * N * N))))


def child(S, N, reps, T):
    import torch
    sys.path.insert(0, ROOT)
    from no_node_comparison_amd import _lib, sim

    L = _lib.lib()
    dev = torch.device("cuda:0")
    r, c = ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(L.nonode_sim_tiled_shape(ctypes.byref(r), ctypes.byref(c)))
    g = torch.Generator(device="cpu").manual_seed(S * 1000003 + N)
    rnd = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)   # noqa: E731
    std = (N / 5.) ** (1 / 3)      # ChargedParticlesSim's loc_std: the density of the reference's systems
    gp, gv = rnd(S, N, 3).to(dev), rnd(S, N, 3).to(dev)
    gm = (1 + 0.1 * rnd(S, N)).to(dev)
    cl, cv = (rnd(S, 3, N) * std).to(dev), (rnd(S, 3, N) * 0.3).to(dev)
    cq = (torch.randint(0, 2, (S, N), generator=g) * 2 - 1).to(torch.float64).to(dev)
    gout = [torch.empty(S, 1, N, 3, dtype=torch.float64, device=dev) for _ in range(3)]
    cout = [torch.empty(S, 1, 3, N, dtype=torch.float64, device=dev) for _ in range(2)]
    nbytes = L.nonode_sim_tiled_workspace_bytes(S, N)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    st = _lib.stream_of(ws)
    P = _lib.ptr
    # sample_freq = T for gravity (one sample, at step 0), T / 2 for charged (one sample, at step T / 2)
    grav = (S, N, T, T, 0.001, 1.0, 0.1, P(gp), P(gv), P(gm), *[P(t) for t in gout])
    chrg = (S, N, T, T // 2, 0.001, 100.0, 1.0, P(cl), P(cv), P(cq), *[P(t) for t in cout])
    arms = {("gravity", "tiled"): (lambda: L.nonode_sim_gravity_tiled(*grav, P(ws), nbytes, st), T),
            ("charged", "tiled"): (lambda: L.nonode_sim_charged_tiled(*chrg, P(ws), nbytes, st), T - 1)}
    if N <= sim.RESIDENT_NMAX:
        arms[("gravity", "resident")] = (lambda: L.nonode_sim_gravity(*grav, st), T + 1)
        arms[("charged", "resident")] = (lambda: L.nonode_sim_charged(*chrg, st), T)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _lib.check(fn())
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    for fn, _ in arms.values():
        timed(fn)                                   # warm-up: code objects, the workspace's first touch
    ms = {k: [] for k in arms}
    for _ in range(reps):
        for k, (fn, _) in arms.items():             # the arms alternate within every repetition
            ms[k].append(timed(fn))
    for (what, kernel), (_, evals) in arms.items():
        per = sorted(t / evals for t in ms[(what, kernel)])
        med = statistics.median(per)
        rate = lambda t: S * N * N / (t * 1e-3) / 1e9   # noqa: E731
        print(json.dumps({"bench": "sim", "sim": what, "kernel": kernel, "S": S, "N": N, "T": T, "reps": reps,
                          "tile_receivers": r.value, "tile_senders": c.value,
                          "ms_per_step": round(med, 5), "ms_per_step_min": round(per[0], 5),
                          "ms_per_step_max": round(per[-1], 5), "gpairs_per_s": round(rate(med), 2),
                          "gpairs_per_s_min": round(rate(per[-1]), 2), "gpairs_per_s_max": round(rate(per[0]), 2),
                          "device": torch.cuda.get_device_name(0)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--steps", type=int, default=0, help="steps per timed call (default: by shape)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim", "bench_sim_tiled.jsonl"))
    ap.add_argument("--limit", type=int, default=240, help="seconds each child may take")
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        S, N = (int(v) for v in a.child.split("x"))
        T = a.steps or steps_for(S, N)
        return child(S, N, a.reps, T + T % 2)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for shape in a.shapes.split(","):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", shape,
               "--reps", str(a.reps), "--steps", str(a.steps)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        with open(a.out, "a") as f:
            f.write(p.stdout)
        if p.returncode != 0:
            print(f"bench_sim: {shape} ended with status {p.returncode}; nothing more is started", file=sys.stderr)
            return p.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
