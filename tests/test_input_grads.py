"""Input gradients of EGNO (x, v, h, loc_mean) and unrolled rollout training, CPU side: the float64
restatement (oracle/torch_ref.py, autograd-capable) against the reference's own autograd recorded in
tests/golden/egno_input_grads.npz, the frame -> input-slot maps of the multi-input model, and the
refusals that are raised before any device work.

Tolerance: 1e-5 max-norm relative per tensor, the bar tests/test_torch_ref.py uses for the reference's
fp32 autograd gradients (themselves ~5e-6 from float64).
"""
import numpy as np
import pytest
import torch

import no_node_comparison_amd as pkg
from oracle import torch_ref as tr
from tests.conftest import load_golden, maxnorm_rel, params_of

GTOL = 1e-5


def seed0_params(fx, dtype=torch.float64, grad=True):
    """The seed-0 EGNO initialisation (tests/golden/init_seed0.npz) the fixture was recorded with, checked
    against the fixture's per-tensor weight sums."""
    p = params_of(load_golden("init_seed0"), "egno::")
    for k, v in p.items():
        ws = float(fx["wsum::" + k])
        assert abs(float(v.astype(np.float64).sum()) - ws) <= 1e-6 * max(1.0, abs(ws)), k
    return {k: torch.tensor(v).to(dtype).requires_grad_(grad) for k, v in p.items()}


def loss_like_reference(x, loc_true, T, B, N):
    """criterion(loc_pred, loc_true).mean((0, 1, 3)).mean() (main_simulation_simple_no.py:268-276), x
    T-major rows [T*BN, 3], loc_true [B, N, T, 3]."""
    pred = x.reshape(T, B, N, 3).permute(1, 2, 0, 3)
    return ((pred - loc_true) ** 2).mean((0, 1, 3)).mean()


def prepare_inputs_ref(loc, vel, ea_o, row, col, N, charges):
    """prepare_inputs (main_simulation_simple_no.py:329-339): loc, vel, loc_mean stay on the tape; nodes
    (:333) and edge_attr (:338) are detached."""
    x, v, ea, nodes, lm = tr.prepare_inputs(loc, vel, ea_o, row, col, N, charges)
    return x, v, ea.detach(), nodes.detach(), lm


def rollout_ref(p, loc, vel, ea_o, row, col, N, B, T, traj_len, charges, t_out_all, t_in=None, **kw):
    """The loop of rollout_fn (:357-371) with gradients enabled, on the restatement: positions
    [traj_len*T, BN, 3]. t_in [B]: frame t_in - 1 of each sample restarts the next segment (None: last).
    kw: per segment keyword lists for tr.egno_forward (lrelu_masks / lrelu_record)."""
    x, v, ea, nodes, lm = prepare_inputs_ref(loc, vel, ea_o, row, col, N, charges)
    preds = []
    sel = (t_in.reshape(-1).long() - 1) if t_in is not None else torch.full((B,), T - 1)
    for i in range(traj_len):
        kwi = {k: val[i] for k, val in kw.items()}
        xo, vo, _ = tr.egno_forward(p, x, nodes, row, col, ea, v, lm, t_out_all[:, i * T:(i + 1) * T] - i * T, T=T,
                                    **kwi)
        preds.append(xo.reshape(T, B * N, 3))
        la = xo.reshape(T, B, N, 3)[sel, torch.arange(B)]
        va = vo.reshape(T, B, N, 3)[sel, torch.arange(B)]
        x, v, ea, nodes, lm = prepare_inputs_ref(la, va, ea_o, row, col, N, charges)
    return torch.cat(preds)


def _d(fx, k):
    return torch.tensor(fx[k]).double()


def test_one_step_input_gradients_of_the_restatement_match_the_reference():
    fx = load_golden("egno_input_grads")
    B, N, T = int(fx["cfg::B"]), int(fx["cfg::N"]), int(fx["cfg::T"])
    p = seed0_params(fx)
    x, v, h, lm = (_d(fx, "one::" + k).requires_grad_(True) for k in ("x", "v", "h", "loc_mean"))
    xo, _, _ = tr.egno_forward(p, x, h, torch.tensor(fx["in::row"]), torch.tensor(fx["in::col"]),
                               _d(fx, "one::edge_attr"), v, lm, torch.tensor(fx["one::t_out"]), T=T)
    loss = loss_like_reference(xo, _d(fx, "one::loc_true"), T, B, N)
    loss.backward()
    assert abs(float(loss.detach()) - float(fx["one::loss"])) <= 1e-6 * abs(float(fx["one::loss"]))
    for name, t in (("g_x", x), ("g_v", v), ("g_h", h), ("g_loc_mean", lm)):
        err = maxnorm_rel(t.grad.numpy(), fx["one::" + name])
        assert err < GTOL, (name, err)


def test_two_chained_segments_of_the_restatement_match_the_reference():
    fx = load_golden("egno_input_grads")
    B, N, T, S = (int(fx["cfg::" + k]) for k in ("B", "N", "T", "traj_len"))
    p = seed0_params(fx)
    loc, vel = _d(fx, "raw::loc").requires_grad_(True), _d(fx, "raw::vel").requires_grad_(True)
    preds = rollout_ref(p, loc, vel, _d(fx, "raw::edge_attr_o"), torch.tensor(fx["in::row"]),
                        torch.tensor(fx["in::col"]), N, B, T, S, _d(fx, "raw::charges"),
                        torch.tensor(fx["two::t_out"]), t_in=torch.tensor(fx["two::t_in"]))
    assert maxnorm_rel(preds.detach().numpy(), fx["two::loc_preds"]) < 1e-6
    loss = loss_like_reference(preds.reshape(S * T * B * N, 3), _d(fx, "two::loc_true"), S * T, B, N)
    loss.backward()
    assert abs(float(loss.detach()) - float(fx["two::loss"])) <= 1e-6 * abs(float(fx["two::loss"]))
    for name, t in (("g_loc", loc), ("g_vel", vel)):
        err = maxnorm_rel(t.grad.numpy(), fx["two::" + name])
        assert err < GTOL, (name, err)
    for k, t in p.items():
        ref = fx["two::grad::" + k]
        if np.abs(ref).max() == 0:
            assert t.grad is None or float(t.grad.abs().max()) == 0, k
        else:
            err = maxnorm_rel(t.grad.numpy(), ref)
            assert err < GTOL, (k, err)


@pytest.mark.parametrize("I,T,want", [(2, 5, [0, 0, 1, 1, 1]), (3, 10, [0, 0, 0, 1, 1, 1, 2, 2, 2, 2]),
                                      (3, 4, [0, 1, 2, 2]), (4, 3, [3, 3, 3])])
def test_frame_inputs_to_slot_map(I, T, want):
    """repeat_elements_to_exact_shape (EGNO/utils.py:115-131): each input T // I times in order, then the
    last input T % I more times; the input-gradient kernels add frame t into slot frame_inputs(T)[t]."""
    m = pkg.EGNO(n_layers=1, in_node_nf=1, in_edge_nf=1, hidden_nf=64, with_v=True, num_timesteps=T, num_inputs=I)
    ref = [i for i in range(I) for _ in range(T // I)] + [I - 1] * (T % I)
    assert ref == want
    assert m.frame_inputs(T) == want
    assert len(want) == T and all(0 <= s < I for s in want)


def test_edge_fea_that_requires_grad_is_refused_before_any_device_work():
    B, N, T = 1, 3, 4
    m = pkg.EGNO(n_layers=1, in_node_nf=1, in_edge_nf=1, hidden_nf=64, with_v=True, num_timesteps=T)
    r, c = tr.full_edges(B, N)
    ef = torch.zeros(B * N * (N - 1), 1, requires_grad=True)
    z = torch.zeros(B * N, 3)
    with pytest.raises(NotImplementedError, match="detach"):
        m(z, torch.zeros(B * N, 1), [r, c], ef, v=z, loc_mean=z)   # CPU tensors: a device call would raise NonodeError
    with torch.no_grad(), pytest.raises(pkg.NonodeError):          # without gradients the flag means nothing
        m(z, torch.zeros(B * N, 1), [r, c], ef, v=z, loc_mean=z)


def test_rollout_train_refuses_several_inputs_before_any_device_work():
    m = pkg.EGNO(n_layers=1, in_node_nf=1, in_edge_nf=1, hidden_nf=64, with_v=True, num_timesteps=4, num_inputs=2)
    with pytest.raises(ValueError, match="num_inputs"):
        pkg.harness.egno_rollout_train(m, None, None, None, None, None, None, None, 3, 2, 1, num_steps=4)
    m1 = pkg.EGNO(n_layers=1, in_node_nf=1, in_edge_nf=1, hidden_nf=64, with_v=True, num_timesteps=4)
    with pytest.raises(ValueError, match="num_inputs"):
        pkg.harness.egno_rollout_train(m1, None, None, None, None, None, None, None, 3, 2, 1, num_steps=4,
                                       timesteps_in=torch.ones(1, 2, dtype=torch.long))


@pytest.mark.parametrize("T,modes", [(4, 2), (10, 2), (8, 5), (5, 3)])
def test_loc_mean_gradient_formula_matches_autograd_of_the_spectral_term(T, modes):
    """dL/dloc_mean of one layer (x - lm; X + spectral(X); + lm) is minus the adjoint of the spectral term
    on the x channel, summed over frames: the closed form the flat path evaluates in torch (and
    input_lm_grad_kernel on the device) against float64 autograd of the restatement's own ops."""
    from no_node_comparison_amd.autograd import _tconvx_lm_grad
    g = torch.Generator().manual_seed(T * 10 + modes)
    BN = 7
    x, v, lm0 = (torch.randn(BN, 3, generator=g, dtype=torch.float64) for _ in range(3))
    w = 0.1 * torch.rand(2, 2, modes, 2, generator=g, dtype=torch.float64)
    gxo, gvo = (torch.randn(T * BN, 3, generator=g, dtype=torch.float64) for _ in range(2))
    lm = lm0.clone().requires_grad_(True)
    xx, vv, lmr = x.repeat(T, 1) + torch.arange(T * BN * 3).reshape(T * BN, 3) * 1e-2, v.repeat(T, 1), lm.repeat(T, 1)
    X = torch.stack([xx - lmr, vv], -1).reshape(T, BN, 3, 2)
    X = X + tr._spectral(X, w)
    xo, vo = X[..., 0].reshape(T * BN, 3) + lmr, X[..., 1].reshape(T * BN, 3)
    ((xo * gxo).sum() + (vo * gvo).sum()).backward()
    got = _tconvx_lm_grad(gxo, gvo, w, T, modes)
    assert maxnorm_rel(got.numpy(), lm.grad.numpy()) < 1e-6   # (float32 trig tables inside the closed form)
