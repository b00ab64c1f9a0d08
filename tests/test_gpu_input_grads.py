"""GPU parity of EGNO's input gradients (x, v, h, loc_mean: nonode_egno_backward_inputs), the taping
rule for frozen / eval() models, the differentiable prepare_inputs (nonode_prepare_inputs_bwd) and
unrolled rollout training (harness.egno_rollout_train).

Truth is float64 torch autograd of the restatement (oracle/torch_ref.py), evaluated at the HIP forward's
own LeakyReLU decisions (model._train_state_sink, tests.test_gpu_train._hip_lrelu_masks, as
test_gpu_train.py:234-288), or the reference's own autograd (tests/golden/egno_input_grads.npz).

Tolerance: the project's fixed bar for gradients against float64, 1e-5 max-norm relative per tensor
(GTOL_F64), for x, v, h, the unrolled gradients and loc_mean alike. loc_mean is the cancellation-prone
one (x - lm ... + lm: the identity parts cancel); the kernel takes it from the spectral term directly.
Measured on an MI355X (worst case of this file): loc_mean 2.7e-7 against float64 (single input, the
N = 33 case; multi-input 2.7e-7, flat 9.8e-8) and 3.1e-7 against the reference's fp32 autograd; x, v, h
<= 4.8e-7; unrolled loc / vel 7.5e-7 against float64 and 1.9e-6 against the reference's fp32 autograd.
The fp32 torch restatement's own autograd is 1.5e-7, 5.4e-7, 2.5e-7, 6.6e-7 from float64 on loc_mean at
the (2,5,10), (3,9,4), (1,20,10), (1,33,2) cases (HIP: 1.1e-7, 1.1e-7, 2.5e-7, 2.7e-7), so the fixed bar
holds with room and no case-dependent bar is used.
"""
import numpy as np
import pytest
import torch

import no_node_comparison_amd as pkg
from oracle import torch_ref as tr
from tests.conftest import check_rel, load_golden, params_of
from tests.test_gpu_parity import DEV, _dev, _egno_case, _egno_full
from tests.test_gpu_train import GTOL_F64, _hip_lrelu_masks
from tests.test_input_grads import loss_like_reference, rollout_ref

pytestmark = pytest.mark.gpu
NAMES = ("x", "v", "h", "loc_mean")


def _model(T=10, modes=2, seed=0, in_node=2, num_inputs=1, **opts):
    torch.manual_seed(seed)
    return pkg.EGNO(n_layers=4, in_node_nf=in_node, in_edge_nf=2, hidden_nf=64, with_v=True, num_modes=modes,
                    num_timesteps=T, time_emb_dim=32, num_inputs=num_inputs, device=DEV, **opts)


def _weights(T, B, N, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, N, T, 3, generator=g), torch.randn(T * B * N, 3, generator=g),
            torch.randn(T * B * N, 64, generator=g))


def _loss(x, v, h, w, T, B, N):
    """The reference's loss on x plus small linear terms in v and h, so every output's reverse is exercised."""
    loc_true, wv, wh = (t.to(device=x.device, dtype=x.dtype) for t in w)
    return loss_like_reference(x, loc_true, T, B, N) + 1e-3 * (v * wv).sum() + 1e-4 * (h * wh).sum()


def _hip_run(m, inp, w, T, B, N, wants=NAMES, t_in=None):
    """One taped forward + backward: (loss, outputs, {input name: grad or None}, LeakyReLU masks or None)."""
    leaf = {k: (inp[k].detach().clone().requires_grad_(k in wants) if inp[k] is not None else None) for k in NAMES}
    m.zero_grad(set_to_none=True)
    m._train_state_sink = []
    kw = dict(timesteps_in=t_in) if t_in is not None else {}
    out = m(leaf["x"], leaf["h"], [inp["row"], inp["col"]], inp["edge_fea"], v=leaf["v"], loc_mean=leaf["loc_mean"],
            timesteps_out=inp["t_out"], **kw)
    state = m._train_state_sink.pop()
    del m._train_state_sink
    BN = leaf["x"].shape[-2]
    masks = _hip_lrelu_masks(state, m.n_layers, T, BN) if m.use_time_conv else None
    loss = _loss(*out, w, T, B, N)
    loss.backward()
    torch.cuda.synchronize()
    return loss, out, {k: (leaf[k].grad if leaf[k] is not None else None) for k in NAMES}, masks


def _f64_run(m, case, w, T, B, N, masks, **opts):
    """float64 autograd of the restatement at the given LeakyReLU decisions: (loss, input leaves, params)."""
    dt = torch.float64
    p = {k: q.detach().cpu().to(dt).requires_grad_(True) for k, q in m.state_dict().items()}
    t = {k: torch.as_tensor(val) for k, val in case.items()}
    leaf = {k: t[k].to(dt).requires_grad_(True) for k in NAMES}
    kw = dict(lrelu_masks=masks) if masks is not None else {}
    out = tr.egno_forward(p, leaf["x"], leaf["h"], t["row"], t["col"], t["edge_fea"].to(dt), leaf["v"],
                          leaf["loc_mean"], t["t_out"], T=T, **opts, **kw)
    loss = _loss(*out, w, T, B, N)
    loss.backward()
    return loss, leaf, p


def _check_inputs(tag, got, ref, skip=()):
    for k in NAMES:
        if k in skip:
            continue
        assert got[k] is not None, (tag, k)
        assert tuple(got[k].shape) == tuple(ref[k].shape), (tag, k, got[k].shape)
        check_rel(f"{tag} d/d{k}", got[k], ref[k].grad, GTOL_F64)


# ---- 1. the reference's own input gradients (fixture), one step ---------------------------------
def _seed0_model(T):
    m = _model(T=T, seed=0)
    m.load_state_dict({k: torch.tensor(v) for k, v in params_of(load_golden("init_seed0"), "egno::").items()})
    return m


def test_one_step_input_gradients_match_reference_golden():
    fx = load_golden("egno_input_grads")
    B, N, T = int(fx["cfg::B"]), int(fx["cfg::N"]), int(fx["cfg::T"])
    m = _seed0_model(T).train()
    leaf = {k: _dev(fx["one::" + k]).requires_grad_(True) for k in NAMES}
    x, _, _ = m(leaf["x"], leaf["h"], [_dev(fx["in::row"]), _dev(fx["in::col"])], _dev(fx["one::edge_attr"]),
                v=leaf["v"], loc_mean=leaf["loc_mean"], timesteps_out=_dev(fx["one::t_out"]))
    loss = loss_like_reference(x, _dev(fx["one::loc_true"]), T, B, N)
    loss.backward()
    torch.cuda.synchronize()
    assert abs(float(loss.detach()) - float(fx["one::loss"])) <= 1e-5 * abs(float(fx["one::loss"]))
    for k in NAMES:
        assert leaf[k].grad is not None, k
        check_rel(f"fixture d/d{k}", leaf[k].grad, fx["one::g_" + k], GTOL_F64)


# ---- 2. against float64 --------------------------------------------------------------------------
# shapes: ragged BN against the 16-row tiles, N = 33: the edge backward's large-N form; Bt < B: one
# timesteps_out row shared by the batch; in_node_nf 1; 5 modes at T = 8 (the Nyquist bin); norm;
# use_time_conv=False (loc_mean unused: gradient None); T = 13: the kernels' frame bound 16 (T <= 10: 10)
CASES = {
    "b2n5t13": dict(B=2, N=5, T=13), "b2n5t10": dict(B=2, N=5, T=10), "b3n9t4": dict(B=3, N=9, T=4),
    "b1n20t10": dict(B=1, N=20, T=10),
    "b1n33t2": dict(B=1, N=33, T=2), "bt1": dict(B=3, N=9, T=4, bt1=True), "in_node1": dict(B=2, N=5, T=10, in_node=1),
    "modes2_t8": dict(B=2, N=5, T=8, modes=2), "modes5_t8": dict(B=2, N=5, T=8, modes=5),
    "norm": dict(B=2, N=5, T=10, opts=dict(norm=True)), "no_tconv": dict(B=3, N=9, T=4, opts=dict(use_time_conv=False)),
}


def _case(c, seed):
    B, N, T = c["B"], c["N"], c["T"]
    case = _egno_case(B, N, T, seed=seed)
    if c.get("bt1"):
        case["t_out"] = case["t_out"][:1]
    if c.get("in_node", 2) == 1:
        case["h"] = case["h"][:, :1]
    return case


@pytest.mark.parametrize("name", sorted(CASES))
def test_input_gradients_match_f64_autograd(name):
    c = CASES[name]
    B, N, T, opts = c["B"], c["N"], c["T"], c.get("opts", {})
    m = _model(T=T, modes=c.get("modes", 2), seed=N + T, in_node=c.get("in_node", 2), **opts).train()
    case = _case(c, seed=B * 10 + N)
    w = _weights(T, B, N, seed=T)
    loss, _, g, masks = _hip_run(m, {k: _dev(v) for k, v in case.items()}, w, T, B, N)
    lr, leaf, _ = _f64_run(m, case, w, T, B, N, masks, **opts)
    assert abs(float(loss.detach()) - float(lr.detach())) <= 1e-5 * abs(float(lr.detach()))
    if not m.use_time_conv:
        assert g["loc_mean"] is None and leaf["loc_mean"].grad is None
    _check_inputs(name, g, leaf, skip=() if m.use_time_conv else ("loc_mean",))


# ---- 3. multi-input: per-slot gradients ---------------------------------------------------------
def _frames_ref(p, x, h, row, col, ef, v, lm, t_in, t_out, fidx, T, masks, hidden=64, ted=32):
    """EGNO.forward with num_inputs > 1 (egno.py:37-111) on the restatement's ops, spread to frames:
    frame t reads slot fidx[t] of x, v, loc_mean [I, BN, 3], h [I, BN, F], ef [I, E, ne]; the embedding
    input is [h, time_emb(t_in), time_emb(t_out)] (egno.py:70)."""
    BN, E = x.shape[1], row.shape[0]
    f = torch.tensor(fidx)

    def emb(t):
        e = tr.timestep_embedding(t, ted)
        return e.permute(1, 0, 2)[:, None].repeat(1, BN // e.shape[0], 1, 1).reshape(T, BN, -1)

    hh = tr._lin(torch.cat([h[f], emb(t_in[:, f]), emb(t_out)], -1).reshape(T * BN, -1), p, "embedding")
    off = (torch.arange(T) * BN).repeat_interleave(E)
    row_t, col_t = row.repeat(T) + off, col.repeat(T) + off
    xx, vv, lmm, eft = (a[f].reshape(T * a.shape[1], -1) for a in (x, v, lm, ef))
    for i in range(4):
        h3 = hh.reshape(T, BN, hidden)
        y = tr._spectral(h3, p[f"time_conv_modules.{i}.t_conv.weights1"])
        hh = (h3 + torch.where(masks[i], y, 0.01 * y)).reshape(T * BN, hidden)
        X = torch.stack([xx - lmm, vv], -1).reshape(T, BN, 3, 2)
        X = X + tr._spectral(X, p[f"time_conv_x_modules.{i}.t_conv.weights1"])
        xx, vv = X[..., 0].reshape(T * BN, 3) + lmm, X[..., 1].reshape(T * BN, 3)
        xx, vv, hh = tr.egnn_layer(p, f"layers.{i}", xx, hh, row_t, col_t, eft, vv)
    return xx, vv, hh


@pytest.mark.parametrize("I,T", [(3, 10), (2, 5)])
def test_multi_input_gradients_per_slot_match_f64_autograd(I, T):
    B, N = 2, 5
    BN, E = B * N, B * N * (N - 1)
    m = _model(T=T, seed=I, num_inputs=I).train()
    g = torch.Generator().manual_seed(T)
    x, lm = torch.randn(I, BN, 3, generator=g), 0.3 * torch.randn(I, BN, 3, generator=g)
    v = 0.5 * torch.randn(I, BN, 3, generator=g)
    h = torch.cat([v.norm(dim=-1, keepdim=True), torch.randint(0, 2, (I, BN, 1), generator=g).float() * 2 - 1], -1)
    ef = torch.randn(I, E, 2, generator=g).abs()
    row, col = tr.full_edges(B, N)
    t_in = torch.arange(-I + 1, 1).repeat(B, 1)
    t_out = torch.arange(1, T + 1).repeat(B, 1)
    w = _weights(T, B, N, seed=I)
    inp = dict(x=x, v=v, h=h, loc_mean=lm, edge_fea=ef, row=row, col=col, t_out=t_out)
    loss, _, got, masks = _hip_run(m, {k: a.to(DEV) for k, a in inp.items()}, w, T, B, N, t_in=t_in.to(DEV))
    dt = torch.float64
    p = {k: q.detach().cpu().to(dt) for k, q in m.state_dict().items()}
    leaf = {k: inp[k].to(dt).requires_grad_(True) for k in NAMES}
    out = _frames_ref(p, leaf["x"], leaf["h"], row, col, ef.to(dt), leaf["v"], leaf["loc_mean"], t_in, t_out,
                      m.frame_inputs(T), T, masks)
    lr = _loss(*out, w, T, B, N)
    lr.backward()
    assert abs(float(loss.detach()) - float(lr.detach())) <= 1e-5 * abs(float(lr.detach()))
    for k in NAMES:
        assert got[k].shape[0] == I
    _check_inputs(f"I={I} T={T}", got, leaf)


# ---- 4. frozen / eval() models --------------------------------------------------------------------
def test_frozen_eval_model_tapes_the_forward_for_inputs_that_require_grad():
    c = CASES["b2n5t10"]
    B, N, T = c["B"], c["N"], c["T"]
    m = _model(T=T, seed=N + T).train()
    case = _case(c, seed=B * 10 + N)
    inp = {k: _dev(v) for k, v in case.items()}
    w = _weights(T, B, N, seed=T)
    _, _, g_train, _ = _hip_run(m, inp, w, T, B, N)
    m.eval()
    for q in m.parameters():
        q.requires_grad_(False)
    loss, out, g, masks = _hip_run(m, inp, w, T, B, N, wants=("x", "v"))
    assert all(o.grad_fn is not None for o in out)
    assert g["h"] is None and g["loc_mean"] is None
    assert all(q.grad is None for q in m.parameters())
    _, leaf, _ = _f64_run(m, case, w, T, B, N, masks)
    for k in ("x", "v"):
        check_rel(f"frozen d/d{k}", g[k], leaf[k].grad, GTOL_F64)
        assert torch.equal(g[k], g_train[k]), k   # the same kernels as the training-mode run of case 2
    with torch.no_grad():   # gradients disabled: the inference forward, nothing taped
        xo, _, _ = m(inp["x"].clone().requires_grad_(True), inp["h"], [inp["row"], inp["col"]], inp["edge_fea"],
                     v=inp["v"], loc_mean=inp["loc_mean"], timesteps_out=inp["t_out"])
    assert xo.grad_fn is None and not xo.requires_grad


def test_frozen_eval_segno_tapes_the_single_input_forward():
    from tests.test_gpu_train_segno import _case as segno_case
    B, N, T = 2, 5, 4
    torch.manual_seed(3)
    m = pkg.SEGNO(in_node_nf=1, in_edge_nf=2, hidden_nf=64, n_layers=8, recurrent=True, device=DEV).eval()
    for q in m.parameters():
        q.requires_grad_(False)
    his, x, v, r, c, ea, target = segno_case(B, N, seed=11)
    xl, vl = _dev(x).requires_grad_(True), _dev(v).requires_grad_(True)
    xo, ho, vo = m(_dev(his), xl, [_dev(r), _dev(c)], vl, _dev(ea), T=T)
    assert xo.grad_fn is not None and vo.grad_fn is not None
    (torch.nn.functional.mse_loss(xo, _dev(target)) + 1e-2 * vo.sum()).backward()
    torch.cuda.synchronize()
    assert all(q.grad is None for q in m.parameters())
    dt = torch.float64
    p = {k: q.detach().cpu().to(dt) for k, q in m.state_dict().items()}
    xr, vr = x.to(dt).requires_grad_(True), v.to(dt).requires_grad_(True)
    xf, _, vf = tr.segno_forward_step(p, his.to(dt), xr, r, c, vr, ea.to(dt), T=T, dense_mean=False)
    (torch.nn.functional.mse_loss(xf, target.to(dt)) + 1e-2 * vf.sum()).backward()
    check_rel("segno frozen d/dx", xl.grad, xr.grad, GTOL_F64)
    check_rel("segno frozen d/dv", vl.grad, vr.grad, GTOL_F64)
    # forward_step from an embedded h: the same rule
    hl = torch.randn(B * N, 64, device=DEV).requires_grad_(True)
    xo2, _, _ = m.forward_step(hl, _dev(x), [_dev(r), _dev(c)], _dev(v), _dev(ea), T=T)
    assert xo2.grad_fn is not None
    xo2.sum().backward()
    assert hl.grad is not None and all(q.grad is None for q in m.parameters())


# ---- 5. parameter gradients unchanged ----------------------------------------------------------------
def test_parameter_gradients_are_bitwise_equal_with_and_without_input_gradients():
    c = CASES["b3n9t4"]
    B, N, T = c["B"], c["N"], c["T"]
    m = _model(T=T, seed=5).train()
    inp = {k: _dev(v) for k, v in _case(c, seed=7).items()}
    w = _weights(T, B, N, seed=1)
    _hip_run(m, inp, w, T, B, N, wants=())
    plain = {k: q.grad.clone() for k, q in m.named_parameters()}
    _, _, g, _ = _hip_run(m, inp, w, T, B, N)
    assert all(g[k] is not None for k in NAMES)
    for k, q in m.named_parameters():
        assert torch.equal(q.grad, plain[k]), k


# ---- 6. unrolled training ------------------------------------------------------------------------------
def _rollout_train(m, loc, vel, eao, q, B, N, T, S, t_in, t_out, truth):
    """prepare_inputs + egno_rollout_train + the loss over all S*T frames, backpropagated: (preds, loss,
    LeakyReLU masks per segment)."""
    edges = pkg.harness.get_edges(B, N, DEV)
    m.zero_grad(set_to_none=True)
    m._train_state_sink = []
    x, v, ea, nodes, lm = pkg.harness.prepare_inputs(loc, vel, eao, edges, N, 1, q)
    assert x.grad_fn is not None and v.grad_fn is not None and lm.grad_fn is not None
    assert not ea.requires_grad and not nodes.requires_grad
    preds = pkg.harness.egno_rollout_train(m, nodes, x, edges, v, eao, ea, lm, N, S, B, charges=q, num_steps=T,
                                           timesteps_in=t_in, timesteps_out=t_out)
    masks = [_hip_lrelu_masks(s, m.n_layers, T, B * N) for s in m._train_state_sink]
    del m._train_state_sink
    assert tuple(preds.shape) == (S * T, B * N, 3) and preds.grad_fn is not None
    loss = loss_like_reference(preds.reshape(S * T * B * N, 3), truth, S * T, B, N)
    loss.backward()
    torch.cuda.synchronize()
    with torch.no_grad():
        ref, _, _ = pkg.harness.egno_rollout(m, nodes, x, edges, v, eao, ea, lm, N, S, B, charges=q, num_steps=T,
                                             timesteps_in=t_in, timesteps_out=t_out)
    check_rel("rollout_train preds vs egno_rollout", preds, ref, 1e-5)
    return preds, loss, masks


def test_unrolled_training_matches_reference_golden():
    fx = load_golden("egno_input_grads")
    B, N, T, S = (int(fx["cfg::" + k]) for k in ("B", "N", "T", "traj_len"))
    m = _seed0_model(T).train()
    loc, vel = _dev(fx["raw::loc"]).requires_grad_(True), _dev(fx["raw::vel"]).requires_grad_(True)
    preds, loss, _ = _rollout_train(m, loc, vel, _dev(fx["raw::edge_attr_o"]), _dev(fx["raw::charges"]), B, N, T, S,
                                    _dev(fx["two::t_in"]), _dev(fx["two::t_out"]), _dev(fx["two::loc_true"]))
    check_rel("unrolled preds", preds, fx["two::loc_preds"], 1e-5)
    assert abs(float(loss.detach()) - float(fx["two::loss"])) <= 1e-5 * abs(float(fx["two::loss"]))
    check_rel("unrolled d/dloc", loc.grad, fx["two::g_loc"], GTOL_F64)
    check_rel("unrolled d/dvel", vel.grad, fx["two::g_vel"], GTOL_F64)
    for k, q in m.named_parameters():
        ref = fx["two::grad::" + k]
        if np.abs(ref).max() == 0:
            assert q.grad is None or float(q.grad.abs().max()) <= 1e-6, k
        else:
            check_rel(f"unrolled grad {k}", q.grad, ref, GTOL_F64)


def test_unrolled_training_matches_f64_autograd():
    B, N, T, S = 3, 9, 4, 2
    m = _model(T=T, seed=13).train()
    *_, (loc, vel, q, eao) = _egno_full(B, N, T, seed=14)
    loc, vel = loc.clone().requires_grad_(True), vel.clone().requires_grad_(True)
    t_in = torch.tensor([T, 1, T - 1], device=DEV)
    t_out = torch.arange(1, S * T + 1, device=DEV).repeat(B, 1)
    truth = torch.randn(B, N, S * T, 3, generator=torch.Generator().manual_seed(15))
    _, loss, masks = _rollout_train(m, loc, vel, eao, q, B, N, T, S, t_in, t_out, truth.to(DEV))
    dt = torch.float64
    d = lambda a: a.detach().cpu().to(dt)  # noqa: E731
    p = {k: d(a).requires_grad_(True) for k, a in m.state_dict().items()}
    lr_, vr_ = d(loc).requires_grad_(True), d(vel).requires_grad_(True)
    r, c = tr.full_edges(B, N)
    preds = rollout_ref(p, lr_, vr_, d(eao), r, c, N, B, T, S, d(q), t_out.cpu(), t_in=t_in.cpu(), lrelu_masks=masks)
    lref = loss_like_reference(preds.reshape(S * T * B * N, 3), truth.to(dt), S * T, B, N)
    lref.backward()
    assert abs(float(loss.detach()) - float(lref.detach())) <= 1e-5 * abs(float(lref.detach()))
    check_rel("unrolled f64 d/dloc", loc.grad, lr_.grad, GTOL_F64)
    check_rel("unrolled f64 d/dvel", vel.grad, vr_.grad, GTOL_F64)
    for k, a in m.named_parameters():
        ref = p[k].grad
        if ref is None or float(ref.abs().max()) == 0:
            assert a.grad is None or float(a.grad.abs().max()) == 0, k
        else:
            check_rel(f"unrolled f64 grad {k}", a.grad, ref, GTOL_F64)


# ---- 7. prepare_inputs backward alone --------------------------------------------------------------------
def test_prepare_inputs_backward_matches_autograd_and_zeroes_unselected_frames():
    F, B, N = 4, 3, 5
    g = torch.Generator().manual_seed(2)
    loc, vel = torch.randn(F, B, N, 3, generator=g), torch.randn(F, B, N, 3, generator=g)
    q = torch.randint(0, 2, (B, N, 1), generator=g).float() * 2 - 1
    wx, wv, wl = (torch.randn(B * N, 3, generator=g) for _ in range(3))
    t_in = torch.tensor([4, 1, 2])
    r, c = tr.full_edges(B, N)
    eao = (q.reshape(-1, 1)[r] * q.reshape(-1, 1)[c])
    ll, vl = loc.to(DEV).requires_grad_(True), vel.to(DEV).requires_grad_(True)
    x, v, ea, nodes, lm = pkg.harness.prepare_inputs(ll, vl, eao.to(DEV), [r.to(DEV), c.to(DEV)], N, 1, q.to(DEV),
                                                     t_in=t_in.to(DEV))
    assert not ea.requires_grad and not nodes.requires_grad
    ((x * wx.to(DEV)).sum() + (v * wv.to(DEV)).sum() + (lm * wl.to(DEV)).sum()).backward()
    torch.cuda.synchronize()
    dt = torch.float64
    lr_, vr_ = loc.to(dt).requires_grad_(True), vel.to(dt).requires_grad_(True)
    sel = t_in - 1
    xr, vr, _, _, lmr = tr.prepare_inputs(lr_[sel, torch.arange(B)], vr_[sel, torch.arange(B)], eao.to(dt), r, c, N,
                                          q.to(dt))
    ((xr * wx).sum() + (vr * wv).sum() + (lmr * wl).sum()).backward()
    check_rel("prepare_inputs d/dloc", ll.grad, lr_.grad, 1e-6)   # sums of N = 5 fp32 terms
    check_rel("prepare_inputs d/dvel", vl.grad, vr_.grad, 1e-6)
    for b in range(B):
        for f in range(F):
            if f != int(sel[b]):
                assert float(ll.grad[f, b].abs().max()) == 0 and float(vl.grad[f, b].abs().max()) == 0, (f, b)
    # values match the forward's (unchanged) outputs off the tape
    with torch.no_grad():
        x0, v0, ea0, n0, lm0 = pkg.harness.prepare_inputs(loc.to(DEV), vel.to(DEV), eao.to(DEV), [r.to(DEV), c.to(DEV)],
                                                          N, 1, q.to(DEV), t_in=t_in.to(DEV))
    for a, b in ((x, x0), (v, v0), (ea, ea0), (nodes, n0), (lm, lm0)):
        assert torch.equal(a.detach(), b)


# ---- 8. flat=True -------------------------------------------------------------------------------------
def test_flat_loc_mean_and_input_gradients_match_f64_autograd():
    B, N, T = 2, 5, 4
    m = _model(T=T, seed=9, flat=True).train()
    case = _egno_case(B, N, T, seed=8)
    w = _weights(T, B, N, seed=4)
    inp = {k: _dev(v) for k, v in case.items()}
    leaf = {k: inp[k].clone().requires_grad_(True) for k in NAMES}
    m.zero_grad(set_to_none=True)
    m._train_bwd_sink = []
    out = m(leaf["x"], leaf["h"], [inp["row"], inp["col"]], inp["edge_fea"], v=leaf["v"], loc_mean=leaf["loc_mean"],
            timesteps_out=inp["t_out"])
    loss = _loss(*out, w, T, B, N)
    loss.backward()
    torch.cuda.synchronize()
    sink = dict(m._train_bwd_sink)
    del m._train_bwd_sink
    masks = [_hip_lrelu_masks(sink[i], 1, T, B * N)[0] for i in range(m.n_layers)]
    lr, ref, _ = _f64_run(m, case, w, T, B, N, masks, flat=True)
    assert abs(float(loss.detach()) - float(lr.detach())) <= 1e-5 * abs(float(lr.detach()))
    _check_inputs("flat", {k: leaf[k].grad for k in NAMES}, ref)
