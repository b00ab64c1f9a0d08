"""The four-wave layer's tile-segment boundary: whatever a workgroup carries from one chunk to the next
(bias vectors read before the barrier, the cuts and its unit range held as scalars) must not change a
bit. NONODE_WGS caps the layer grid, so that one workgroup
walks several chunks and ends on a chunk of another shape; the capped runs are compared bitwise with
the uncapped one, and every run with the float64 oracle at the bar of test_gpu_edge_walk (1e-5)."""
import numpy as np
import pytest
import torch

import no_node_comparison_amd as pkg
from oracle import torch_ref as tr
from tests import _segment_case as sc
from tests.conftest import check_rel, maxnorm_rel

TOL = 1e-5


def test_boundary_switches_query():
    """The debug query names the levers the build carries (bits PREB, UCUT). None of them adds an
    LDS table, so the launch's LDS formula chooses no fallback path: every launch of the four-wave
    EGNO kernel runs the same code, which the GPU tests below walk."""
    s = pkg.lib().nonode_debug_boundary_switches()
    assert 0 <= s < 4


# N = 20, CG = 4: 9 graph-frames = two full C2 chunks (5 tiles, cuts [0, 24, 48, 72, 95]) and a one-graph
#   chunk of 2 tiles with the packed 4-row last tile; B = 3 < CG: gr % ef_mod wraps inside a chunk, and the
#   edge-feature period is shorter than a chunk. B = 5: the period is longer than a chunk and wraps in one.
# N = 5: chunk shape (1, 4, 4, 4), cuts [0, 1, 2, 3, 4]: every segment a single unit.
# N = 8: runs of 3 t + 1 units.
@pytest.mark.gpu
@pytest.mark.parametrize("B,N,T,cg", [(3, 20, 3, 4), (5, 20, 2, 4), (3, 5, 4, 0), (2, 8, 3, 0)])
def test_egno_one_workgroup_walks_several_chunks(monkeypatch, B, N, T, cg):
    if cg:
        monkeypatch.setenv("NONODE_CG", str(cg))
    m = sc.egno(T, seed=B * 100 + N)
    case = sc.egno_case(B, N, T, seed=N)
    ref = sc.egno_oracle(m, case, T)
    free, one, two = sc.capped_runs(monkeypatch, lambda: sc.egno_run(m, case), (None, 1, 2))
    for tag, out in (("uncapped", free), ("WGS=1", one), ("WGS=2", two)):
        for name, o, r in zip("xvh", out, ref):
            check_rel(f"{tag} {name}", o, r, TOL)
    sc.assert_bitwise("xvh", one, free, "one workgroup differs from the uncapped grid")
    sc.assert_bitwise("xvh", two, free, "two workgroups differ from the uncapped grid")


@pytest.mark.gpu
def test_egno_guard_recompute_in_a_segments_first_iteration(monkeypatch):
    """test_gpu_edge_walk's guard case (edge features x 3e4: the first SiLU leaves the fp16 range and the
    units take the column-scaled recompute) with one workgroup walking every chunk; its range assertion
    and its bar: 1e-5, or twice the error of the reference's own ops in fp32 where that is larger."""
    B, N, T, scale = 2, 20, 4, 3e4
    monkeypatch.setenv("NONODE_CG", "4")
    monkeypatch.setenv("NONODE_WGS", "1")
    m = sc.egno(T, seed=B * 7 + N)
    case = sc.egno_case(B, N, T, seed=N + 1)
    case["edge_fea"] = (case["edge_fea"] * scale).astype(np.float32)
    p = sc.sd_np(m)
    w1 = p["layers.0.edge_message_net.scalar_net.mlp.0.weight"][:, -2:]
    assert float(np.abs(case["edge_fea"].astype(np.float64) @ w1.T).max()) > 2 * 65504.0
    xr, vr, hr = sc.egno_oracle(m, case, T)
    assert np.isfinite(xr).all() and np.isfinite(hr).all()
    p32 = {k: torch.tensor(v, dtype=torch.float32) for k, v in p.items()}
    t = lambda a: torch.tensor(np.ascontiguousarray(a))  # noqa: E731
    with torch.no_grad():
        f32 = tr.egno_forward(p32, t(case["x"]).float(), t(case["h"]).float(), t(case["row"]).long(),
                              t(case["col"]).long(), t(case["edge_fea"]).float(), t(case["v"]).float(),
                              t(case["loc_mean"]).float(), t(case["t_out"]).float(), n_layers=2, T=T)
    x, v, h = sc.egno_run(m, case)
    for name, out, f, ref in (("x", x, f32[0], xr), ("v", v, f32[1], vr), ("h", h, f32[2], hr)):
        check_rel(f"guard WGS=1 {name}", out, ref, max(TOL, 2 * maxnorm_rel(f.numpy(), ref)))


@pytest.mark.gpu
def test_egno_two_feature_ksteps_capped_and_uncapped(monkeypatch):
    """in_edge_nf = 4, the widest the model takes (its constructor rejects more): |r|^2 and four scalar
    edge inputs are five features, the KF = 2 instance of the kernel (two k-steps of four)."""
    B, N, T = 3, 5, 2
    m = sc.egno(T, seed=61, in_edge_nf=4)
    case = sc.egno_case(B, N, T, seed=6, in_edge_nf=4)
    ref = sc.egno_oracle(m, case, T)
    free, one = sc.capped_runs(monkeypatch, lambda: sc.egno_run(m, case), (None, 1))
    for tag, out in (("uncapped", free), ("WGS=1", one)):
        for name, o, r in zip("xvh", out, ref):
            check_rel(f"KF=2 {tag} {name}", o, r, TOL)
    sc.assert_bitwise("xvh", one, free, "KF = 2: one workgroup differs from the uncapped grid")


@pytest.mark.gpu
def test_segno_four_waves_fused_substeps_capped_and_uncapped(monkeypatch):
    """SEGNO, N = 20, B = 4, 3 substeps: uncapped, every workgroup runs its one chunk's substeps fused;
    capped to one workgroup, it walks the four chunks substep by substep."""
    B, N, T = 4, 20, 3
    m = sc.segno(seed=N + B)
    case = sc.segno_case(B, N, seed=B)
    ref = sc.segno_oracle(m, case, T)
    free, one = sc.capped_runs(monkeypatch, lambda: sc.segno_run(m, case, T), (None, 1))
    names = ("xo", "ho", "vo")
    for tag, out in (("uncapped", free), ("WGS=1", one)):
        for name, o, r in zip(names, out, ref):
            check_rel(f"segno {tag} {name}", o, r, TOL)
    sc.assert_bitwise(names, one, free, "SEGNO: one workgroup differs from the uncapped grid")


@pytest.mark.gpu
def test_egno_training_forward_capped_equals_uncapped(monkeypatch):
    """The taped forward (message and force sums saved for the reverse pass), N = 20, B = 3, T = 2, CG = 4."""
    B, N, T = 3, 20, 2
    monkeypatch.setenv("NONODE_CG", "4")
    m = sc.egno(T, seed=77).train()
    case = sc.egno_case(B, N, T, seed=8)
    free, one = sc.capped_runs(monkeypatch, lambda: sc.egno_run(m, case, grad=True), (None, 1))
    sc.assert_bitwise("xvh", one, free, "training forward: one workgroup differs from the uncapped grid")
