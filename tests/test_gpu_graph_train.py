"""EGNO(graph="trainable"): training on arbitrary edge lists (csrc/nonode_graph_train.hip,
autograd.GraphLayerTrain) against float64 torch autograd of the op-by-op restatement
(oracle/torch_ref.egnn_layer / egno_forward, which take any row / col), max-norm relative error per
tensor at the project's fixed gradient bar of 1e-5.

Shapes: tests/_graph_case.sparse_graph(37) and (80): two isolated nodes, a receiver of in-degree 40, a
self loop, a duplicate edge, a shuffled list, ragged 16-node tiles. TimeConv's LeakyReLU has a kink, so
the whole-model reference is evaluated at the HIP reverse's own branch decisions (model._train_bwd_sink,
as tests/test_gpu_options.py does for flat=True), with at most 16 flipped decisions per layer, each at
the kink.
"""
import numpy as np
import pytest
import torch

import no_node_comparison_amd as pkg
from no_node_comparison_amd import _lib, autograd, graph
from oracle import torch_ref as tr
from tests._graph_case import edge_features, egno_case, sparse_graph
from tests.conftest import check_rel, load_golden, maxnorm_rel, params_of
from tests.test_gpu_graph import _dev, _egno, _layer_graph, _layer_inputs
from tests.test_gpu_train import _hip_lrelu_masks

pytestmark = pytest.mark.gpu
TOL = 1e-5
DEV = "cuda"
P = _lib.ptr
F64 = torch.float64
LAYER_KEYS = [f"{mlp}.mlp.{k}.{wb}" for mlp in ("edge_message_net.scalar_net", "coord_net", "node_v_net", "node_net")
              for k in (0, 2) for wb in ("weight", "bias")]


@pytest.fixture(scope="module")
def egno_fx():
    return load_golden("egno_fwd")


def _model(fx, **kw):
    """The fixture's trained weights (without the TimeConv ones for use_time_conv=False)."""
    sd = params_of(fx)
    if not kw.get("use_time_conv", True):
        sd = {k: v for k, v in sd.items() if not k.startswith("time_conv")}
    return _egno(sd, **kw)


def _t64(a):
    return torch.tensor(np.ascontiguousarray(a)).to(F64)


# ---- the layer entry ---------------------------------------------------------------------------------
def _hip_layer(m, layer, n_frames, n, row, col, h, x, v, ef, gx, gv, gh, cap_bytes=None):
    """nonode_egnn_layer_graph (its workspace kept as the state), then the reverse over the frame groups:
    (h_out, x_out, g_h_in, g_x_in, g_v_in, [16 parameter gradients]) as device tensors."""
    L = pkg.lib()
    edges = [_dev(row), _dev(col)]
    csr = graph.csr(edges, n)
    scsr = graph.csr_by_sender(edges, n)
    blobs, _ = m._packed()
    bb = m._packed_bwd()
    dh, dx, dv, de = _dev(h), _dev(x), _dev(v), _dev(ef)
    ho, xo = torch.empty_like(dh), torch.empty_like(dx)
    ws_bytes = L.nonode_egnn_layer_graph_workspace_bytes(n_frames, n)
    state = torch.empty((ws_bytes + 3) // 4, dtype=torch.float32, device=DEV)
    E = len(row)
    _lib.check(L.nonode_egnn_layer_graph(_lib.VARIANT_EGNO, n_frames, n, E, ef.shape[-1], ef.shape[0], P(dh), P(dx), P(dv),
                                         P(de), P(blobs[layer]), P(csr[0]), P(csr[1]), P(csr[2]), 0.0, 1.0, 0, P(ho), P(xo),
                                         None, P(state), ws_bytes, _lib.stream_of(dh)))
    g = autograd.graph_layer_reverse(n_frames, n, E, ef.shape[-1], ef.shape[0], dh, dx, dv, de.reshape(-1, ef.shape[-1]),
                                     blobs[layer], bb[layer], state, csr, scsr, _dev(gx), _dev(gv), _dev(gh), cap_bytes)
    torch.cuda.synchronize()
    return (ho, xo) + tuple(g)


def _f64_layer(m, layer, n, row_t, col_t, h, x, v, ef_t, gx, gv, gh, dtype=F64, norm=False):
    """Autograd of oracle/torch_ref.egnn_layer for the loss sum(x' gx) + sum(v' gv) + sum(h' gh):
    ((x', h'), g_h, g_x, g_v, [16 parameter gradients])."""
    pre = f"layers.{layer}"
    p = {k: q.detach().cpu().to(dtype).requires_grad_(True) for k, q in m.state_dict().items() if k.startswith(pre)}
    c = lambda a: torch.tensor(a).to(dtype)  # noqa: E731
    hh, xx, vv = (c(a).requires_grad_(True) for a in (h, x, v))
    xo, vo, ho = tr.egnn_layer(p, pre, xx, hh, torch.tensor(row_t), torch.tensor(col_t), c(ef_t), vv, norm=norm)
    ((xo * c(gx)).sum() + (vo * c(gv)).sum() + (ho * c(gh)).sum()).backward()
    return (xo.detach(), ho.detach()), hh.grad, xx.grad, vv.grad, [p[f"{pre}.{k}"].grad for k in LAYER_KEYS]


def _check_layer(tag, got, ref, bar=TOL):
    errs = [check_rel(f"{tag} x_out", got[1], ref[0][0], bar), check_rel(f"{tag} h_out", got[0], ref[0][1], bar)]
    for name, a, b in zip(("dL/dh", "dL/dx", "dL/dv"), got[2:5], ref[1:4]):
        errs.append(check_rel(f"{tag} {name}", a, b, bar))
    for name, a, b in zip(LAYER_KEYS, got[5], ref[4]):
        errs.append(check_rel(f"{tag} grad {name}", a.reshape(b.shape), b, bar))
    return max(errs)


def _out_grads(nt, seed):
    rng = np.random.RandomState(seed)
    return [rng.randn(nt, k).astype(np.float32) for k in (3, 3, 64)]   # gx, gv, gh


@pytest.mark.parametrize("norm", [False, True], ids=["plain", "norm_radial"])
@pytest.mark.parametrize("n_frames,ef_frames", [(1, 1), (3, 1), (3, 3)])
@pytest.mark.parametrize("n", [37, 80])
def test_layer_reverse_matches_f64_autograd(egno_fx, n, n_frames, ef_frames, norm):
    m = _egno(params_of(egno_fx), norm=norm)
    row, col, h, x, v, ef, row_t, col_t, ef_t = _layer_inputs(n, n_frames, ef_frames, seed=n + n_frames)
    gx, gv, gh = _out_grads(n_frames * n, n)
    got = _hip_layer(m, 1, n_frames, n, row, col, h, x, v, ef, gx, gv, gh)
    ref = _f64_layer(m, 1, n, row_t, col_t, h, x, v, ef_t, gx, gv, gh, norm=norm)
    _check_layer("layer", got, ref)
    graph.sync_checks()


def test_training_forward_is_bitwise_the_inference_layer(egno_fx):
    """GraphLayerTrain's forward (no time convolution: the layer alone) against nonode_egnn_layer_graph."""
    n, T = 37, 10
    m = _model(egno_fx, graph="trainable", use_time_conv=False)
    row, col, h, x, v, ef, *_ = _layer_inputs(n, T, 1, seed=5)
    blobs, _ = m._packed()
    ho, xo, _ = _layer_graph(_lib.VARIANT_EGNO, blobs[2], T, n, row, col, h, x, v, ef)
    edges = [_dev(row), _dev(col)]
    g = (graph.csr(edges, n), graph.csr_by_sender(edges, n))
    ht, xt, vt = autograd.GraphLayerTrain.apply(m, 2, n, len(row), g, _dev(h).requires_grad_(True), _dev(x), _dev(v),
                                                None, _dev(ef[0]), *autograd._flat_layer_params(m, 2))
    assert ht.requires_grad and np.array_equal(ht.detach().cpu().numpy(), ho)
    assert np.array_equal(xt.detach().cpu().numpy(), xo) and np.array_equal(vt.detach().cpu().numpy(), v)
    graph.sync_checks()


def test_layer_reverse_with_the_clamp_mask_active():
    """Positions x 7: some mean-force components pass +-100 (zero gradient through the clamp) and some do
    not. Cancellation-prone, so the bar follows tests/test_gpu_weight_scales.py: max(1e-5, 2 x the fp32
    torch path's own error against float64, measured here)."""
    n = 37
    fx = load_golden("egno_fwd")
    torch.manual_seed(43)   # 22 of the 111 components clamp, the nearest 10% from the kink
    m = pkg.EGNO(n_layers=1, in_node_nf=2, in_edge_nf=2, hidden_nf=64, with_v=True, num_modes=2, num_timesteps=10,
                 time_emb_dim=32, device=DEV).eval()
    row, col = sparse_graph(n)
    rng = np.random.RandomState(37)
    x = (fx["in::x"][:n] * 7).astype(np.float32)
    v = fx["in::v"][:n].astype(np.float32)
    h = rng.randn(n, 64).astype(np.float32)
    ef = edge_features(len(row), 2)
    gx, gv, gh = _out_grads(n, 3)
    ref = _f64_layer(m, 0, n, row, col, h, x, v, ef, gx, gv, gh)
    # the clamp's state on the float64 reference: mean force per receiver
    p = {k: q.detach().cpu().to(F64) for k, q in m.state_dict().items()}
    xx, hh = _t64(x), _t64(h)
    r, c = torch.tensor(row), torch.tensor(col)
    rij = xx[r] - xx[c]
    msg = tr._mlp(torch.cat([(rij * rij).sum(-1, keepdim=True), hh[r], hh[c], _t64(ef)], -1), p,
                  "layers.0.edge_message_net.scalar_net", last_act=True)
    mean_f = tr._scatter(rij * tr._mlp(msg, p, "layers.0.coord_net"), r, n, True).abs()
    print(f"clamped components: {int((mean_f > 100).sum())} of {mean_f.numel()}, nearest to the kink "
          f"{float(((mean_f - 100).abs() / 100).min()):.3f}")
    assert bool((mean_f > 100).any()) and bool((mean_f[mean_f > 0] < 100).any())
    assert float(((mean_f - 100).abs() / 100).min()) > 0.01
    f32 = _f64_layer(m, 0, n, row, col, h, x, v, ef, gx, gv, gh, dtype=torch.float32)
    floor = max([maxnorm_rel(a.numpy(), b.numpy()) for a, b in zip(f32[1:4], ref[1:4])] +
                [maxnorm_rel(a.numpy(), b.numpy()) for a, b in zip(f32[4], ref[4])])
    print(f"fp32 torch path against float64: {floor:.3e}")
    got = _hip_layer(m, 0, 1, n, row, col, h, x, v, ef[None], gx, gv, gh)
    _check_layer("clamp", got, ref, max(TOL, 2 * floor))
    graph.sync_checks()


def test_layer_reverse_is_bitwise_reproducible_and_list_order_free(egno_fx):
    n, n_frames = 80, 3
    m = _egno(params_of(egno_fx))
    row, col, h, x, v, ef, *_ = _layer_inputs(n, n_frames, 3, seed=9)
    gx, gv, gh = _out_grads(n_frames * n, 9)
    a = _hip_layer(m, 1, n_frames, n, row, col, h, x, v, ef, gx, gv, gh)
    b = _hip_layer(m, 1, n_frames, n, row, col, h, x, v, ef, gx, gv, gh)
    assert all(torch.equal(s, t) for s, t in zip(a[2:5], b[2:5]))
    # without duplicate edges both CSRs, and with them every sum order, do not depend on the list order
    row, col = sparse_graph(n, simple=True)
    ef = np.stack([edge_features(len(row), 2, f) for f in range(3)])
    perm = np.random.RandomState(3).permutation(len(row))
    a = _hip_layer(m, 1, n_frames, n, row, col, h, x, v, ef, gx, gv, gh)
    b = _hip_layer(m, 1, n_frames, n, row[perm], col[perm], h, x, v, ef[:, perm], gx, gv, gh)
    assert all(torch.equal(s, t) for s, t in zip(a[2:5], b[2:5]))
    graph.sync_checks()


def test_frame_groups_of_one_frame(egno_fx):
    """The operand cap set so that each group is one frame: the input gradients are bitwise those of the
    single group, the weight gradients (accumulated over the groups) within the bar of float64 both ways."""
    n, n_frames = 37, 3
    m = _egno(params_of(egno_fx))
    row, col, h, x, v, ef, row_t, col_t, ef_t = _layer_inputs(n, n_frames, 3, seed=13)
    gx, gv, gh = _out_grads(n_frames * n, 13)
    one_frame = len(row) * 400 * 4
    assert autograd.graph_frame_groups(n_frames, len(row)) == [(0, 3)]
    assert autograd.graph_frame_groups(n_frames, len(row), one_frame) == [(0, 1), (1, 2), (2, 3)]
    a = _hip_layer(m, 1, n_frames, n, row, col, h, x, v, ef, gx, gv, gh)
    b = _hip_layer(m, 1, n_frames, n, row, col, h, x, v, ef, gx, gv, gh, cap_bytes=one_frame)
    assert all(torch.equal(s, t) for s, t in zip(a[2:5], b[2:5]))
    ref = _f64_layer(m, 1, n, row_t, col_t, h, x, v, ef_t, gx, gv, gh)
    _check_layer("one group", a, ref)
    _check_layer("three groups", b, ref)
    graph.sync_checks()


def test_layer_reverse_at_n130_past_the_fused_limit(egno_fx):
    """One fully connected graph of N = 130 passed as a list (E = 16,770): the fused training refuses
    N > 115."""
    from oracle import harness as oh
    N = 130
    m = _egno(params_of(egno_fx))
    rng = np.random.RandomState(130)
    row, col = oh.full_edges(1, N)
    assert len(row) == 16770
    x = (rng.randn(N, 3) * (N / 5.0) ** (1.0 / 3.0)).astype(np.float32)
    v = (rng.randn(N, 3) * 0.5).astype(np.float32)
    h = (rng.randn(N, 64) * 0.5).astype(np.float32)
    q = rng.randint(0, 2, N) * 2.0 - 1.0
    ef = np.stack([q[row] * q[col], ((x[row].astype(np.float64) - x[col]) ** 2).sum(1)], 1).astype(np.float32)
    gx, gv, gh = _out_grads(N, 130)
    got = _hip_layer(m, 0, 1, N, row, col, h, x, v, ef[None], gx, gv, gh)
    ref = _f64_layer(m, 0, N, row, col, h, x, v, ef, gx, gv, gh)
    _check_layer("N=130", got, ref)
    graph.sync_checks()


def test_dropped_edge_rows_reach_no_sum(egno_fx):
    """A device list with one index out of range: nonode_graph_build drops that edge and flags the list, and
    the reverse equals, bitwise, that of the list without it (operand rows of a dropped edge are zero). The
    flag surfaces as ValueError at the next boundary call. No out-of-range address is touched: every index
    the kernels read comes from the range-checked CSRs."""
    n = 37
    graph.sync_checks()
    m = _egno(params_of(egno_fx))
    row, col, h, x, v, ef, *_ = _layer_inputs(n, 1, 1, seed=21)
    gx, gv, gh = _out_grads(n, 21)
    keep = np.arange(len(row)) != 11
    good = _hip_layer(m, 1, 1, n, row[keep], col[keep], h, x, v, ef[:, keep], gx, gv, gh)
    graph.sync_checks()
    bad_col = col.copy()
    bad_col[11] = n
    bad = _hip_layer(m, 1, 1, n, row, bad_col, h, x, v, ef, gx, gv, gh)
    with pytest.raises(ValueError, match="outside"):
        graph.sync_checks()
    assert all(torch.equal(s, t) for s, t in zip(good[2:5], bad[2:5]))
    for a, b in zip(good[5], bad[5]):
        assert bool(torch.isfinite(b).all())
        check_rel("dropped edge grad", b, a.cpu().numpy(), 1e-6)
    graph.sync_checks()


# ---- the whole model -------------------------------------------------------------------------------------
OPTS = {"default": {}, "norm": dict(norm=True), "no_time_conv": dict(use_time_conv=False)}


def _inputs(c, grad=True):
    t = {k: _dev(c[k]) for k in ("x", "h", "v", "loc_mean", "edge_fea", "t_out")}
    if grad:
        for k in ("x", "h", "v", "loc_mean"):
            t[k].requires_grad_(True)
    return t, [_dev(c["row"]), _dev(c["col"])]


def _loss(x, v, h, target, wv, wh, scale):
    return (((x - target) ** 2).mean() + 1e-3 * (v * wv).sum() + 1e-4 * (h * wh).sum()) * scale


def _run_model(m, c, weights, scale=1.0):
    """One taped forward + backward: (outputs, loss, input gradients, LeakyReLU masks or None)."""
    t, edges = _inputs(c)
    m.zero_grad(set_to_none=True)
    m._train_bwd_sink = []
    x, v, h = m(t["x"], t["h"], edges, t["edge_fea"], v=t["v"], loc_mean=t["loc_mean"], timesteps_out=t["t_out"])
    loss = _loss(x, v, h, *[_dev(w) for w in weights], scale)
    loss.backward()
    torch.cuda.synchronize()
    sink = dict(m._train_bwd_sink)
    del m._train_bwd_sink
    masks = None
    if m.use_time_conv:
        assert sorted(sink) == list(range(m.n_layers))
        masks = [_hip_lrelu_masks(sink[i], 1, m.num_timesteps, c["x"].shape[0])[0] for i in range(m.n_layers)]
    gin = {k: t[k].grad for k in ("x", "h", "v", "loc_mean")}
    return (x.detach(), v.detach(), h.detach()), float(loss.detach()), gin, masks


def _f64_model(m, c, weights, opts, scale=1.0, **kw):
    p = {k: q.detach().cpu().to(F64).requires_grad_(True) for k, q in m.state_dict().items()}
    t = {k: _t64(c[k]).requires_grad_(True) for k in ("x", "h", "v", "loc_mean")}
    out = tr.egno_forward(p, t["x"], t["h"], torch.tensor(c["row"]), torch.tensor(c["col"]), _t64(c["edge_fea"]), t["v"],
                          t["loc_mean"], torch.tensor(c["t_out"]), T=m.num_timesteps, **opts, **kw)
    loss = _loss(*out, *[_t64(w) for w in weights], scale)
    loss.backward()
    return [o.detach() for o in out], float(loss.detach()), p, {k: t[k].grad for k in t}


def _weights(n, T, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((T * n, 3)).astype(np.float32), rng.standard_normal((T * n, 3)).astype(np.float32),
            rng.standard_normal((T * n, 64)).astype(np.float32))


def _check_model(tag, m, c, opts, scale=1.0):
    T, n = m.num_timesteps, c["x"].shape[0]
    w = _weights(n, T, n)
    outs, loss, gin, masks = _run_model(m, c, w, scale)
    kw = {}
    if masks is not None:
        ys = []
        _f64_model(m, c, w, opts, scale, lrelu_record=ys)
        for i, (mk, y) in enumerate(zip(masks, ys)):
            flip = mk != (y > 0)
            assert int(flip.sum()) <= 16, (i, int(flip.sum()))
            if flip.any():
                assert float(y[flip].abs().max()) <= 1e-5 * float(y.abs().max()), i   # at the kink
        kw = dict(lrelu_masks=masks)
    ro, rl, p, rin = _f64_model(m, c, w, opts, scale, **kw)
    assert abs(loss - rl) <= 1e-5 * abs(rl), (loss, rl)
    for name, a, b in zip("xvh", outs, ro):
        check_rel(f"{tag} out {name}", a, b, TOL)
    for k, q in m.named_parameters():
        ref = p[k].grad
        if ref is None or float(ref.abs().max()) == 0:
            assert q.grad is None or float(q.grad.abs().max()) <= 1e-6 * scale, k
            continue
        check_rel(f"{tag} grad {k}", q.grad, ref, TOL)
    for k in ("x", "h", "v", "loc_mean"):
        if k == "loc_mean" and not m.use_time_conv:
            assert gin[k] is None or float(gin[k].abs().max()) == 0   # not read without time convolutions
            continue
        check_rel(f"{tag} dL/d{k}", gin[k], rin[k], TOL)
    return gin


@pytest.mark.parametrize("name", sorted(OPTS))
@pytest.mark.parametrize("n", [37, 80])
def test_model_gradients_match_f64_autograd(egno_fx, n, name):
    m = _model(egno_fx, graph="trainable", **OPTS[name]).train()
    _check_model(name, m, egno_case(egno_fx, n), OPTS[name])
    graph.sync_checks()


def test_frozen_model_returns_the_same_input_gradients(egno_fx):
    """eval() with every parameter frozen and x.requires_grad_(): the tape is entered for the inputs alone."""
    n = 37
    c = egno_case(egno_fx, n)
    w = _weights(n, 10, n)
    m = _egno(params_of(egno_fx), graph="trainable").train()
    _, _, want, _ = _run_model(m, c, w)
    m.eval()
    for q in m.parameters():
        q.requires_grad_(False)
    _, _, got, _ = _run_model(m, c, w)
    assert all(q.grad is None for q in m.parameters())
    for k in ("x", "h", "v", "loc_mean"):
        assert torch.equal(got[k], want[k]), k
    graph.sync_checks()


@pytest.mark.parametrize("scale", [2.0 ** -20, 2.0 ** 10], ids=["2^-20", "2^10"])
def test_model_gradients_at_other_magnitudes(egno_fx, scale):
    """The loss x 2^-20 and x 2^10: the column scaling before the fp16 split keeps the bar."""
    m = _egno(params_of(egno_fx), graph="trainable").train()
    _check_model(f"scale {scale:g}", m, egno_case(egno_fx, 37), {}, scale)
    graph.sync_checks()


def test_three_adam_steps_repack_the_blobs(egno_fx):
    """After three optimizer steps the taped forward runs on the model's current parameters (forward and
    backward blobs re-packed): its outputs against the float64 restatement at those parameters."""
    n = 37
    c = egno_case(egno_fx, n)
    m = _egno(params_of(egno_fx), graph="trainable").train()
    w = _weights(n, 10, 1)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        t, edges = _inputs(c, grad=False)
        x, v, h = m(t["x"], t["h"], edges, t["edge_fea"], v=t["v"], loc_mean=t["loc_mean"], timesteps_out=t["t_out"])
        loss = _loss(x, v, h, *[_dev(a) for a in w], 1.0)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert all(np.isfinite(losses)) and losses[2] != losses[0]
    t, edges = _inputs(c, grad=False)
    x, v, h = m(t["x"], t["h"], edges, t["edge_fea"], v=t["v"], loc_mean=t["loc_mean"], timesteps_out=t["t_out"])
    assert x.requires_grad
    torch.cuda.synchronize()
    p = {k: q.detach().cpu().to(F64) for k, q in m.state_dict().items()}
    ro = tr.egno_forward(p, _t64(c["x"]), _t64(c["h"]), torch.tensor(c["row"]), torch.tensor(c["col"]),
                         _t64(c["edge_fea"]), _t64(c["v"]), _t64(c["loc_mean"]), torch.tensor(c["t_out"]), T=10)
    for name, a, b in zip("xvh", (x, v, h), ro):
        check_rel(f"after 3 steps {name}", a, b, TOL)
    graph.sync_checks()


def test_taped_forward_on_an_invalid_device_list_poisons_and_raises(egno_fx):
    """The forward's mechanism holds on the tape: the bad edge is dropped from both CSRs (nothing reads out
    of range), the outputs are NaN-filled behind the flag, and the error surfaces at the next boundary call."""
    n = 37
    graph.sync_checks()
    m = _egno(params_of(egno_fx), graph="trainable").train()
    c = dict(egno_case(egno_fx, n))
    c["col"] = c["col"].copy()
    c["col"][11] = n
    t, edges = _inputs(c, grad=False)
    out = m(t["x"], t["h"], edges, t["edge_fea"], v=t["v"], loc_mean=t["loc_mean"], timesteps_out=t["t_out"])
    torch.cuda.synchronize()
    assert out[0].requires_grad and all(bool(torch.isnan(o).all()) for o in out)
    with pytest.raises(ValueError, match="outside"):
        graph.sync_checks()
    graph.sync_checks()


# ---- unchanged paths ---------------------------------------------------------------------------------------
def test_trainable_in_eval_is_bitwise_any(egno_fx):
    sd = params_of(egno_fx)
    c = egno_case(egno_fx, 80)
    outs = []
    for g in ("trainable", "any"):
        m = _egno(sd, graph=g)
        t, edges = _inputs(c, grad=False)
        with torch.no_grad():
            outs.append(m(t["x"], t["h"], edges, t["edge_fea"], v=t["v"], loc_mean=t["loc_mean"],
                          timesteps_out=t["t_out"]))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    graph.sync_checks()


def test_known_full_list_takes_the_fused_training_path(egno_fx):
    from tests.test_gpu_parity import _egno_case
    B, N, T = 3, 20, 10
    c = _egno_case(B, N, T, seed=23)
    sd = params_of(egno_fx)
    edges = pkg.harness.get_edges(B, N, DEV)
    grads = []
    for g in ("trainable", "full"):
        m = _egno(sd, graph=g).train()
        n_csr = len(graph._csr)
        x, v, h = m(_dev(c["x"]), _dev(c["h"]), edges, _dev(c["edge_fea"]), v=_dev(c["v"]),
                    loc_mean=_dev(c["loc_mean"]), timesteps_out=_dev(c["t_out"]))
        assert len(graph._csr) == n_csr
        ((x ** 2).mean() + 1e-3 * (h ** 2).mean()).backward()
        torch.cuda.synchronize()
        grads.append({k: q.grad.clone() for k, q in m.named_parameters()})
    assert all(torch.equal(grads[0][k], grads[1][k]) for k in grads[1])
