"""SEGNO(graph="any", trainable=True): training on arbitrary edge lists and device-built neighbour graphs
(csrc/nonode_graph_train.hip's SEGNO instantiations, nonode_segno_forward_train_graph,
autograd.SEGNOGraphTrain / SEGNOGraphStepTrain, harness.segno_rollout_train_graph) against float64 torch
autograd of the op-by-op restatement (oracle/torch_ref.gcl / segno_forward_step with dense_mean=False, which
take any row / col), max-norm relative error per tensor at the project's fixed gradient bar of 1e-5.

Weights: the segno_fwd fixture's. Graphs: tests/_graph_case.sparse_graph(37) and (80): two isolated nodes, a
receiver of in-degree 40, a self loop, a duplicate edge, a shuffled list, ragged 16-node tiles. SEGNO's
per-edge clamp has a kink at |r_k c| = 100: the float64 reference asserts that no component lies in
[99, 101] (with the fixture's weights c is of order 1e-3, so none clamps; the clamp test scales coord_mlp.2
up until 10-50% do).
"""
import numpy as np
import pytest
import torch

import no_node_comparison_amd as pkg
from no_node_comparison_amd import _lib, autograd, graph, harness
from oracle import torch_ref as tr
from tests._graph_case import edge_features, segno_case, sparse_graph
from tests._neighbor_ref import neighbor_ref
from tests.conftest import check_rel, load_golden, maxnorm_rel, params_of
from tests.test_gpu_graph import _dev, _layer_inputs

pytestmark = pytest.mark.gpu
TOL = 1e-5
DEV = "cuda"
P = _lib.ptr
F64 = torch.float64
GCL_KEYS = [f"module.{mlp}.{k}.{wb}" for mlp in ("edge_mlp", "coord_mlp") for k in (0, 2) for wb in ("weight", "bias")] + \
           [None] * 4 + [f"module.node_mlp.{k}.{wb}" for k in (0, 2) for wb in ("weight", "bias")]
# sparse_graph(37) with coord_mlp.2 x CLAMP_SCALE and the inputs of _layer_inputs(37, 1, 1, CLAMP_SEED): see
# test_substep_reverse_with_the_clamp_mask_active (found on the CPU with clamp_state below)
CLAMP_SCALE, CLAMP_SEED = 370.0, 5   # 17.9% of the 474 components clamp, the nearest 2.8% from the kink


@pytest.fixture(scope="module")
def segno_fx():
    return load_golden("segno_fwd")


def _segno(sd, device=DEV, **kw):
    kw.setdefault("recurrent", True)
    torch.manual_seed(0)
    m = pkg.SEGNO(in_node_nf=1, in_edge_nf=2, hidden_nf=64, n_layers=8, device=device, graph="any", trainable=True, **kw)
    m.load_state_dict({k: torch.tensor(v) for k, v in sd.items()})
    return m.train()


def _t(a, dtype=F64):
    return torch.tensor(np.ascontiguousarray(a)).to(dtype)


def _p64(m, dtype=F64):
    return {k: q.detach().cpu().to(dtype).requires_grad_(True) for k, q in m.state_dict().items()}


def edge_translations(p, h, x, row, col, ea, tanh=False):
    """r_k c of every edge and component (gcl.py:97-99, before the clamp), at the dtype of p."""
    diff = x[row] - x[col]
    m = torch.nn.functional.silu(tr._lin(torch.nn.functional.silu(tr._lin(
        torch.cat([h[row], h[col], (diff ** 2).sum(1, keepdim=True), ea], 1), p, "module.edge_mlp.0")), p, "module.edge_mlp.2"))
    c = tr._lin(torch.nn.functional.silu(tr._lin(m, p, "module.coord_mlp.0")), p, "module.coord_mlp.2")
    return diff * (torch.tanh(c) if tanh else c)


def clamp_state(p, h, x, row, col, ea, tanh=False):
    """(fraction of the edge components that clamp, the nearest one's relative distance from +-100)."""
    with torch.no_grad():
        f = edge_translations(p, h, x, row, col, ea, tanh).abs()
    if f.numel() == 0:
        return 0.0, 1.0
    return float((f > 100).double().mean()), float(((f - 100).abs() / 100).min())


def _assert_off_the_kink(p, h, x, row, col, ea, tanh=False):
    with torch.no_grad():
        f = edge_translations(p, h, x, row, col, ea, tanh).abs()
    assert not bool(((f >= 99) & (f <= 101)).any())


# ---- 1. one substep --------------------------------------------------------------------------------------
def _hip_substep(m, n, row, col, h, x, v, ef, gx, gv, gh, dt):
    """nonode_egnn_layer_graph (variant SEGNO, its workspace kept as the state), then the substep's reverse:
    (h_out, x_out, v_out, g_h_in, g_x_in, g_v_in, [16 parameter gradients, the node_v ones None])."""
    L = pkg.lib()
    edges = [_dev(row), _dev(col)]
    csr, scsr = graph.csr(edges, n), graph.csr_by_sender(edges, n)
    blob, bb = m._packed(), m._packed_bwd()
    dh, dx, dv, de = _dev(h), _dev(x), _dev(v), _dev(ef)
    ho, xo, vo = torch.empty_like(dh), torch.empty_like(dx), torch.empty_like(dv)
    ws_bytes = L.nonode_egnn_layer_graph_workspace_bytes(1, n)
    state = torch.empty((ws_bytes + 3) // 4, dtype=torch.float32, device=DEV)
    E = len(row)
    cw, rec = float(m.coords_weight), int(bool(m.recurrent))
    _lib.check(L.nonode_egnn_layer_graph(_lib.VARIANT_SEGNO, 1, n, E, 2, 1, P(dh), P(dx), P(dv), P(de), P(blob), P(csr[0]),
                                         P(csr[1]), P(csr[2]), dt, cw, rec, P(ho), P(xo), P(vo), P(state), ws_bytes,
                                         _lib.stream_of(dh)))
    g = autograd.graph_layer_reverse(1, n, E, 2, 1, dh, dx, dv, de, blob, bb, state, csr, scsr, _dev(gx), _dev(gv),
                                     _dev(gh), variant=_lib.VARIANT_SEGNO, segno=(dt, cw, rec))
    torch.cuda.synchronize()
    return (ho, xo, vo) + tuple(g)


def _f64_substep(m, row, col, h, x, v, ef, gx, gv, gh, n_sub, dtype=F64, off_kink=True):
    """Autograd of oracle/torch_ref.gcl(dense_mean=False) for the loss sum(x' gx) + sum(v' gv) + sum(h' gh):
    ((h', x', v'), g_h, g_x, g_v, [16 parameter gradients in GCL_KEYS order, None where there is none])."""
    p = _p64(m, dtype)
    hh, xx, vv = (_t(a, dtype).requires_grad_(True) for a in (h, x, v))
    r, c, ea = torch.tensor(row), torch.tensor(col), _t(ef, dtype)
    if off_kink:
        _assert_off_the_kink(p, hh, xx, r, c, ea, m.tanh)
    ho, xo, vo = tr.gcl(p, hh, r, c, xx, vv, ea, n_sub, recurrent=bool(m.recurrent), coords_weight=m.coords_weight,
                        dense_mean=False, tanh=m.tanh)
    ((xo * _t(gx, dtype)).sum() + (vo * _t(gv, dtype)).sum() + (ho * _t(gh, dtype)).sum()).backward()
    return ((ho.detach(), xo.detach(), vo.detach()), hh.grad, xx.grad, vv.grad,
            [p[k].grad if k is not None else None for k in GCL_KEYS])


def _check_substep(tag, got, ref, bar=TOL):
    errs = []
    for name, a, b in zip(("h_out", "x_out", "v_out"), got[:3], ref[0]):
        errs.append(check_rel(f"{tag} {name}", a, b, bar))
    for name, a, b in zip(("dL/dh", "dL/dx", "dL/dv"), got[3:6], ref[1:4]):
        errs.append(check_rel(f"{tag} {name}", a, b, bar))
    n = 0
    for name, a, b in zip(GCL_KEYS, got[6], ref[4]):
        if name is None:
            assert a is None
            continue
        n += 1
        errs.append(check_rel(f"{tag} grad {name}", a.reshape(b.shape), b, bar))
    assert n == 12
    return max(errs)


def _out_grads(n, seed):
    rng = np.random.RandomState(seed)
    return [rng.randn(n, k).astype(np.float32) for k in (3, 3, 64)]   # gx, gv, gh


@pytest.mark.parametrize("tanh", [False, True], ids=["plain", "tanh"])
@pytest.mark.parametrize("cw", [1.0, 0.5])
@pytest.mark.parametrize("recurrent", [True, False], ids=["recurrent", "plain_h"])
@pytest.mark.parametrize("n", [37, 80])
def test_substep_reverse_matches_f64_autograd(segno_fx, n, recurrent, cw, tanh):
    m = _segno(params_of(segno_fx), recurrent=recurrent, coords_weight=cw, tanh=tanh)
    row, col, h, x, v, ef, *_ = _layer_inputs(n, 1, 1, seed=n + 1)
    gx, gv, gh = _out_grads(n, n)
    got = _hip_substep(m, n, row, col, h, x, v, ef[0], gx, gv, gh, 1.0 / 3)
    ref = _f64_substep(m, row, col, h, x, v, ef[0], gx, gv, gh, 3)
    _check_substep("substep", got, ref)
    graph.sync_checks()


# ---- 2. the clamp ----------------------------------------------------------------------------------------
def _clamp_case(segno_fx, device):
    n = 37
    m = _segno(params_of(segno_fx), device=device)
    with torch.no_grad():
        m.module.coord_mlp[2].weight.mul_(CLAMP_SCALE)
        m.module.coord_mlp[2].bias.mul_(CLAMP_SCALE)
    row, col, h, x, v, ef, *_ = _layer_inputs(n, 1, 1, seed=CLAMP_SEED)
    return m, n, row, col, h, x, v, ef[0]


def test_substep_reverse_with_the_clamp_mask_active(segno_fx):
    """coord_mlp.2 scaled up: in the float64 reference between 10% and 50% of the edge components clamp (zero
    gradient through them) and none lies within 1% of +-100. Cancellation-prone, so the bar is that of
    test_layer_reverse_with_the_clamp_mask_active: max(1e-5, 2 x the fp32 torch path's own error against
    float64, measured here)."""
    m, n, row, col, h, x, v, ef = _clamp_case(segno_fx, DEV)
    p = _p64(m)
    frac, nearest = clamp_state(p, _t(h), _t(x), torch.tensor(row), torch.tensor(col), _t(ef))
    print(f"clamped components: {frac:.3f} of {3 * len(row)}, nearest to the kink {nearest:.4f}")
    assert 0.10 <= frac <= 0.50 and nearest > 0.01
    gx, gv, gh = _out_grads(n, 3)
    ref = _f64_substep(m, row, col, h, x, v, ef, gx, gv, gh, 3, off_kink=False)
    f32 = _f64_substep(m, row, col, h, x, v, ef, gx, gv, gh, 3, dtype=torch.float32, off_kink=False)
    floor = max([maxnorm_rel(a.numpy(), b.numpy()) for a, b in zip(f32[1:4], ref[1:4])] +
                [maxnorm_rel(a.numpy(), b.numpy()) for a, b in zip(f32[4], ref[4]) if b is not None])
    print(f"fp32 torch path against float64: {floor:.3e}")
    got = _hip_substep(m, n, row, col, h, x, v, ef, gx, gv, gh, 1.0 / 3)
    _check_substep("clamp", got, ref, max(TOL, 2 * floor))
    graph.sync_checks()


# ---- 3. the whole model ----------------------------------------------------------------------------------
def _target(c, seed=5):
    rng = np.random.RandomState(seed)
    return (c["x"] + 0.3 * c["v"] + 0.05 * rng.randn(*c["x"].shape)).astype(np.float32)


def _hip_model_step(m, c, T, target, edges=None, edge_attr=None, loss_fn=None):
    """One taped forward + backward: (outputs (x, h, v), loss, [dL/dhis, dL/dx, dL/dv])."""
    ins = [_dev(c[k]).requires_grad_(True) for k in ("his", "x", "v")]
    edges = edges if edges is not None else [_dev(c["row"]), _dev(c["col"])]
    ea = edge_attr if edge_attr is not None else _dev(c["edge_attr"])
    m.zero_grad(set_to_none=True)
    xo, ho, vo = m(ins[0], ins[1], edges, ins[2], ea, T=T)
    loss = torch.nn.functional.mse_loss(xo, _dev(target)) if loss_fn is None else loss_fn(xo, ho, vo, _dev)
    loss.backward()
    torch.cuda.synchronize()
    return (xo.detach(), ho.detach(), vo.detach()), float(loss.detach()), [t.grad for t in ins]


def _f64_model_step(m, c, T, target, loss_fn=None):
    p = _p64(m)
    his, x, v = (_t(c[k]).requires_grad_(True) for k in ("his", "x", "v"))
    r, cc, ea = torch.tensor(c["row"]), torch.tensor(c["col"]), _t(c["edge_attr"])
    h = tr._lin(his, p, "embedding")
    xx, vv = x, v
    for _ in range(T):
        _assert_off_the_kink(p, h.detach(), xx.detach(), r, cc, ea, m.tanh)
        h, xx, vv = tr.gcl(p, h, r, cc, xx, vv, ea, T, recurrent=bool(m.recurrent), coords_weight=m.coords_weight,
                           dense_mean=False, tanh=m.tanh)
    loss = torch.nn.functional.mse_loss(xx, _t(target)) if loss_fn is None else loss_fn(xx, h, vv, _t)
    loss.backward()
    return (xx.detach(), h.detach(), vv.detach()), float(loss.detach()), p, [his.grad, x.grad, v.grad]


def _check_param_grads(tag, m, p, bar=TOL):
    """Every parameter against the float64 reference (the conventions of test_gpu_train_segno._check_grads);
    returns the number of live ones."""
    n = 0
    for k, q in m.named_parameters():
        ref = p[k].grad
        if ref is None or float(ref.abs().max()) == 0:
            assert q.grad is None or float(q.grad.abs().max()) == 0, k
            continue
        if float(ref.abs().max()) < 1e-12:   # zero in exact arithmetic (the attention output bias)
            assert float(q.grad.abs().max()) < 1e-7, k
            continue
        n += 1
        check_rel(f"{tag} grad {k}", q.grad, ref, bar)
    return n


def _check_model(tag, m, c, T, loss_fn=None):
    """One step on the case's list against float64: returns (number of live parameters, the input gradients)."""
    target = _target(c)
    outs, loss, gin = _hip_model_step(m, c, T, target, loss_fn=loss_fn)
    ro, rl, p, rin = _f64_model_step(m, c, T, target, loss_fn=loss_fn)
    assert abs(loss - rl) <= 1e-5 * abs(rl), (loss, rl)
    for name, a, b in zip("xhv", outs, ro):
        check_rel(f"{tag} out {name}", a, b, TOL)
    live = _check_param_grads(tag, m, p)
    for name, a, b in zip(("his", "x", "v"), gin, rin):
        check_rel(f"{tag} dL/d{name}", a, b, TOL)
    return live, gin


@pytest.mark.parametrize("T", [3, 10])
def test_model_gradients_match_f64_autograd(segno_fx, T):
    """One MSE step: the 12 GCL and the two embedding gradients (coord_mlp_vel has none), dL/dx, dL/dv, dL/dhis."""
    m = _segno(params_of(segno_fx))
    live, _ = _check_model(f"T={T}", m, segno_case(segno_fx, 37), T)
    assert live == 14
    assert all(q.grad is None or float(q.grad.abs().max()) == 0 for k, q in m.named_parameters() if "coord_mlp_vel" in k)
    graph.sync_checks()


# ---- 4. the reference's own gradients --------------------------------------------------------------------
def test_shuffled_full_list_matches_the_reference_gradients():
    """tests/golden/segno_grad.npz with its full list shuffled and edge_attr permuted alike: a list never seen
    takes the general path."""
    gd = load_golden("segno_grad")
    T = int(gd["cfg::T"])
    m = _segno(params_of(gd))
    perm = np.random.RandomState(4).permutation(len(gd["in::row"]))
    edges = [_dev(gd["in::row"][perm]), _dev(gd["in::col"][perm])]
    assert graph.known_full(edges, gd["in::x"].shape[0]) is None
    xo, _, _ = m(_dev(gd["in::his"]), _dev(gd["in::x"]), edges, _dev(gd["in::v"]), _dev(gd["in::edge_attr"][perm]), T=T)
    loss = torch.nn.MSELoss()(xo, _dev(gd["in::loc_end"]))
    loss.backward()
    torch.cuda.synchronize()
    check_rel("x", xo, gd["out::x"], TOL)
    assert abs(float(loss.detach()) - float(gd["out::loss"])) <= 1e-5 * abs(float(gd["out::loss"]))
    n = 0
    for k, q in m.named_parameters():
        if "grad::" + k not in gd:
            assert q.grad is None or float(q.grad.abs().max()) == 0, k   # coord_mlp_vel: not on the path
            continue
        n += 1
        check_rel(f"grad {k}", q.grad, gd["grad::" + k], TOL)
    assert n == 14
    graph.sync_checks()


# ---- 5. forward equality ---------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [4, 0])
def test_training_forward_is_bitwise_the_inference_forward(segno_fx, T):
    """nonode_segno_forward_train_graph against nonode_segno_forward_step_graph from one embedded h."""
    n = 37
    m = _segno(params_of(segno_fx))
    c = segno_case(segno_fx, n)
    h = _dev((np.random.RandomState(5).randn(n, 64) * 0.5).astype(np.float32))
    args = (h, _dev(c["x"]), [_dev(c["row"]), _dev(c["col"])], _dev(c["v"]), _dev(c["edge_attr"]))
    xa, ha, va = m.forward_step(*args, T=T)
    assert xa.requires_grad and ha.requires_grad and va.requires_grad
    with torch.no_grad():
        xb, hb, vb = m.forward_step(*args, T=T)
    torch.cuda.synchronize()
    for a, b in ((xa, xb), (ha, hb), (va, vb)):
        assert not b.requires_grad and torch.equal(a.detach(), b)
    if T == 0:
        assert torch.equal(xa.detach(), args[1]) and torch.equal(ha.detach(), h) and torch.equal(va.detach(), args[3])
    graph.sync_checks()


# ---- 6. reproducibility ----------------------------------------------------------------------------------
def test_backward_is_bitwise_reproducible_and_list_order_free(segno_fx):
    n, T = 80, 4
    m = _segno(params_of(segno_fx))
    c = segno_case(segno_fx, n)
    target = _target(c)
    _, _, a = _hip_model_step(m, c, T, target)
    pa = {k: q.grad.clone() for k, q in m.named_parameters() if q.grad is not None}
    _, _, b = _hip_model_step(m, c, T, target)
    assert all(torch.equal(s, t) for s, t in zip(a, b))
    assert all(torch.equal(pa[k], q.grad) for k, q in m.named_parameters() if q.grad is not None)
    # without duplicate edges both CSRs, and with them every sum order, do not depend on the list order
    c = segno_case(segno_fx, n, simple=True)
    perm = np.random.RandomState(3).permutation(len(c["row"]))
    cp = dict(c, row=c["row"][perm], col=c["col"][perm], edge_attr=c["edge_attr"][perm])
    _, _, a = _hip_model_step(m, c, T, target)
    _, _, b = _hip_model_step(m, cp, T, target)
    assert all(torch.equal(s, t) for s, t in zip(a, b))
    graph.sync_checks()


# ---- 7. isolated nodes and dropped edges -----------------------------------------------------------------
def _full_loss(seed):
    def loss_fn(x, h, v, conv):
        rng = np.random.RandomState(seed)
        wx, wv, wh = (conv(rng.randn(*t.shape).astype(np.float32)) for t in (x, v, h))
        return (x * wx).sum() + (v * wv).sum() + 0.1 * (h * wh).sum()
    return loss_fn


def test_a_graph_without_edges(segno_fx):
    """E = 0 on n = 5: every node isolated (x' = x + v dt, the edge and coordinate MLPs without gradient)."""
    n, T = 5, 3
    m = _segno(params_of(segno_fx))
    e = np.zeros(0, dtype=np.int64)
    c = dict(his=segno_fx["in::his"][:n], x=segno_fx["in::x"][:n], v=segno_fx["in::v"][:n], row=e, col=e,
             edge_attr=np.zeros((0, 2), dtype=np.float32))
    live, _ = _check_model("E=0", m, c, T, loss_fn=_full_loss(7))
    assert live == 6   # node_mlp's four and the embedding's two
    graph.sync_checks()


def test_dropped_edge_rows_reach_no_sum(segno_fx):
    """A device list with one index out of range: nonode_graph_build drops that edge and flags the list; the
    tape node trains on the kept edges (input gradients bitwise those of the list without it, the dropped
    edge's operand rows zero) and the flag surfaces as ValueError at graph.sync_checks(). No out-of-range
    address is touched: every index the kernels read comes from the range-checked CSRs."""
    n, T, drop = 37, 3, 11
    graph.sync_checks()
    m = _segno(params_of(segno_fx))
    c = segno_case(segno_fx, n)
    h = (np.random.RandomState(8).randn(n, 64) * 0.5).astype(np.float32)
    gx = _dev(np.random.RandomState(9).randn(n, 3).astype(np.float32))

    def run(row, col, ea):
        edges = [_dev(row), _dev(col)]
        g = (n, len(row), graph.csr(edges, n), graph.csr_by_sender(edges, n))
        ins = [_dev(a).requires_grad_(True) for a in (h, c["x"], c["v"])]
        m.zero_grad(set_to_none=True)
        m._train_ops_sink = []
        xo, _, _ = autograd.segno_graph_step_train(m, ins[0], ins[1], ins[2], _dev(ea), T, g)
        (xo * gx).sum().backward()
        torch.cuda.synchronize()
        sink = m._train_ops_sink
        del m._train_ops_sink
        return [t.grad for t in ins], {k: q.grad.clone() for k, q in m.named_parameters() if q.grad is not None}, sink

    keep = np.arange(len(c["row"])) != drop
    good, pgood, _ = run(c["row"][keep], c["col"][keep], c["edge_attr"][keep])
    graph.sync_checks()
    bad_col = c["col"].copy()
    bad_col[drop] = n
    bad, pbad, sink = run(c["row"], bad_col, c["edge_attr"])
    with pytest.raises(ValueError, match="outside"):
        graph.sync_checks()
    assert all(torch.equal(s, t) for s, t in zip(good, bad))
    assert len(sink) == 1 and sink[0][:2] == (0, T)
    eops = sink[0][3].view(T, len(c["row"]), 400)
    assert not bool(eops[:, drop].any()) and bool(eops[:, drop - 1].any())
    for k in pgood:
        assert bool(torch.isfinite(pbad[k]).all())
        check_rel(f"dropped edge grad {k}", pbad[k], pgood[k], 1e-6)
    graph.sync_checks()


# ---- 8. substep groups -----------------------------------------------------------------------------------
def test_substep_groups_of_one_substep(segno_fx):
    """model.graph_ops_cap_bytes = one substep's edge operands: T groups. The input gradients are bitwise those
    of the single group; the weight gradients (added over the groups) within the bar of float64 both ways."""
    n, T = 37, 4
    m = _segno(params_of(segno_fx))
    c = segno_case(segno_fx, n)
    E = len(c["row"])
    assert autograd.graph_frame_groups(T, E) == [(0, T)]
    assert autograd.graph_frame_groups(T, E, E * 400 * 4) == [(t, t + 1) for t in range(T)]
    _, one = _check_model("one group", m, c, T)
    m.graph_ops_cap_bytes = E * 400 * 4
    m._train_ops_sink = []
    _, many = _check_model("T groups", m, c, T)
    assert [s[:2] for s in m._train_ops_sink] == [(t, t + 1) for t in reversed(range(T))]
    del m._train_ops_sink
    assert all(torch.equal(s, t) for s, t in zip(one, many))
    graph.sync_checks()


# ---- 9. a frozen model -----------------------------------------------------------------------------------
def test_frozen_model_returns_input_gradients_only(segno_fx):
    n, T = 37, 3
    m = _segno(params_of(segno_fx))
    c = segno_case(segno_fx, n)
    target = _target(c)
    _, _, want = _hip_model_step(m, c, T, target)
    m.eval()
    for q in m.parameters():
        q.requires_grad_(False)
    _, _, got = _hip_model_step(m, c, T, target)
    assert all(q.grad is None for q in m.parameters())
    assert all(torch.equal(s, t) for s, t in zip(got, want))
    graph.sync_checks()


# ---- 10. several inputs ----------------------------------------------------------------------------------
@pytest.mark.parametrize("agg", ["sum", "attn"])
def test_multi_input_gradients_match_f64_autograd(segno_fx, agg):
    """I = 2 (model.py:53-92, 104-139): two integrator segments on the general path and the fold between them
    (torch ops on the tape)."""
    n, T, I = 37, 3, 2
    sd = params_of(segno_fx)
    torch.manual_seed(9)
    m = pkg.SEGNO(in_node_nf=1, in_edge_nf=2, hidden_nf=64, n_layers=8, recurrent=True, multiple_agg=agg, device=DEV,
                  graph="any", trainable=True)
    m.load_state_dict({k: torch.tensor(v) for k, v in sd.items()}, strict=False)   # (attn: its MLP keeps its init)
    m.train()
    row, col = sparse_graph(n)
    g = torch.Generator().manual_seed(10)
    x = torch.randn(n, I, 3, generator=g)
    v = torch.randn(n, I, 3, generator=g) * 0.5
    his = v.norm(dim=-1, keepdim=True)
    ea = torch.tensor(edge_features(len(row), 2, 3))
    in_steps = torch.tensor([0, 2])
    steps = [2, T]
    target = torch.randn(n, 3, generator=g)
    m.zero_grad(set_to_none=True)
    xo, _, _ = m(_dev(his), _dev(x), [_dev(row), _dev(col)], _dev(v), _dev(ea), T=T, in_steps=in_steps)
    loss = torch.nn.functional.mse_loss(xo, _dev(target))
    loss.backward()
    torch.cuda.synchronize()
    p = _p64(m)
    r, c = torch.tensor(row), torch.tensor(col)
    h = tr._lin(his.to(F64), p, "embedding")
    xs, vs = x.to(F64), v.to(F64)

    def fold(ls, vls, hs):
        if agg == "sum":
            return ls.sum(1), vls.sum(1), hs.sum(1)
        speed = vls.norm(dim=-1, keepdim=True)
        z = torch.tanh(tr._lin(torch.cat([speed, hs], -1), p, "enc_attn_net.attn_mlp.0"))
        a = tr._lin(z, p, "enc_attn_net.attn_mlp.2").softmax(dim=1)
        return (a * ls).sum(1), (a * vls).sum(1), (a * hs).sum(1)

    h_, x_, v_ = h[:, 0], xs[:, 0], vs[:, 0]
    for i, st in enumerate(steps):
        hi, xi, vi = h_, x_, v_
        for _ in range(st):
            _assert_off_the_kink(p, hi.detach(), xi.detach(), r, c, ea.to(F64))
            hi, xi, vi = tr.gcl(p, hi, r, c, xi, vi, ea.to(F64), st, dense_mean=False)
        if i < len(steps) - 1:
            x_, v_, h_ = fold(torch.stack([xs[:, i + 1], xi], 1), torch.stack([vs[:, i + 1], vi], 1),
                              torch.stack([h[:, i + 1], hi], 1))
    lr = torch.nn.functional.mse_loss(xi, target.to(F64))
    lr.backward()
    check_rel(f"{agg} x", xo, xi, TOL)
    assert abs(float(loss.detach()) - float(lr.detach())) <= 1e-5 * abs(float(lr.detach()))
    assert _check_param_grads(agg, m, p) == (17 if agg == "attn" else 14)
    graph.sync_checks()


# ---- 11. a neighbour graph built on the device -----------------------------------------------------------
def test_training_on_a_neighbor_graph_equals_its_trimmed_list(segno_fx):
    """B = 3, N = 7, k = 4 with a cut-off that leaves some rows short (a -1 tail): the padded NeighborGraph
    with its CSR by sender against its trimmed explicit list, bitwise, and both against float64."""
    B, N, k, r_cut, T = 3, 7, 4, 1.6, 3
    n = B * N
    rs = np.random.RandomState(12)
    x = (rs.randn(n, 3) * 1.2).astype(np.float32)
    ref = neighbor_ref(x, B, N, k, r_cut)
    assert 0 < ref["E"] < ref["cap"] and int(ref["deg"].min()) < k <= int(ref["deg"].max())
    ng = graph.neighbor_graph(_dev(x), B, N, k, r_cut, by_sender=True)
    assert ng.has_sender_csr() and ng.capacity == ref["cap"]
    E = ref["E"]
    row, col = ref["rows"][:E].astype(np.int64), ref["col"][:E].astype(np.int64)
    ea = rs.randn(ref["cap"], 2).astype(np.float32)
    ea_pad = _dev(ea)
    ea_pad[E:] = float("nan")              # the tail is never read
    c = dict(his=np.abs(rs.randn(n, 1)).astype(np.float32), x=x, v=(rs.randn(n, 3) * 0.3).astype(np.float32),
             row=row, col=col, edge_attr=ea[:E])
    m = _segno(params_of(segno_fx))
    loss_fn = _full_loss(13)
    target = _target(c)
    pad = _hip_model_step(m, c, T, target, edges=ng, edge_attr=ea_pad, loss_fn=loss_fn)
    ppad = {k_: q.grad.clone() for k_, q in m.named_parameters() if q.grad is not None}
    live, trimmed = _check_model("trimmed list", m, c, T, loss_fn=loss_fn)
    assert live == 14
    lists = ng.edge_index()
    assert np.array_equal(lists[0].cpu().numpy(), row) and np.array_equal(lists[1].cpu().numpy(), col)
    for a, b in zip(pad[2], trimmed):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    ro, _, p, rin = _f64_model_step(m, c, T, target, loss_fn=loss_fn)
    for name, a, b in zip("xhv", pad[0], ro):
        check_rel(f"padded out {name}", a, b, TOL)
    for name, a, b in zip(("his", "x", "v"), pad[2], rin):
        check_rel(f"padded dL/d{name}", a, b, TOL)
    for k_, q in ppad.items():
        if p[k_].grad is not None and float(p[k_].grad.abs().max()) > 0:
            check_rel(f"padded grad {k_}", q, p[k_].grad, TOL)
    graph.sync_checks()


# ---- 12. unrolled rollout training -----------------------------------------------------------------------
def test_rollout_train_graph_matches_a_f64_loop_on_its_graphs(segno_fx):
    B, N, k, steps = 2, 6, 3, [2, 3]
    n = B * N
    rs = np.random.RandomState(14)
    loc0 = (rs.randn(n, 3) * 1.2).astype(np.float32)
    vel0 = (rs.randn(n, 3) * 0.3).astype(np.float32)
    q = (rs.randint(0, 2, (n, 1)) * 2.0 - 1.0).astype(np.float32)
    target = rs.randn(len(steps), n, 3).astype(np.float32)
    m = _segno(params_of(segno_fx))
    loc, vel = _dev(loc0).requires_grad_(True), _dev(vel0).requires_grad_(True)
    m.zero_grad(set_to_none=True)
    preds, graphs = harness.segno_rollout_train_graph(m, loc, vel, _dev(q), B, len(steps), steps, k=k, return_graphs=True)
    assert preds.shape == (len(steps), n, 3) and preds.grad_fn is not None and len(graphs) == len(steps)
    loss = torch.nn.functional.mse_loss(preds, _dev(target))
    loss.backward()
    torch.cuda.synchronize()
    lists = [[t.cpu() for t in g.edge_index()] for g in graphs]
    p = _p64(m)
    x, v = _t(loc0).requires_grad_(True), _t(vel0).requires_grad_(True)
    qq = _t(q)
    xi, vi, out = x, v, []
    for (r, c), T in zip(lists, steps):
        his = vi.detach().norm(dim=1, keepdim=True)
        ea = torch.cat([qq[r] * qq[c], ((xi.detach()[r] - xi.detach()[c]) ** 2).sum(1, keepdim=True)], 1)
        h = tr._lin(his, p, "embedding")
        for _ in range(T):
            _assert_off_the_kink(p, h.detach(), xi.detach(), r, c, ea)
            h, xi, vi = tr.gcl(p, h, r, c, xi, vi, ea, T, dense_mean=False)
        out.append(xi)
    out = torch.stack(out)
    lr = torch.nn.functional.mse_loss(out, _t(target))
    lr.backward()
    check_rel("rollout preds", preds, out, TOL)
    assert abs(float(loss.detach()) - float(lr.detach())) <= 1e-5 * abs(float(lr.detach()))
    assert _check_param_grads("rollout", m, p) == 14
    check_rel("rollout dL/dloc", loc.grad, x.grad, TOL)
    check_rel("rollout dL/dvel", vel.grad, v.grad, TOL)
    graph.sync_checks()


# ---- bug_compat ------------------------------------------------------------------------------------------
def test_bug_compat_keeps_returning_its_inputs(segno_fx):
    n = 37
    m = _segno(params_of(segno_fx), bug_compat=True)
    c = segno_case(segno_fx, n)
    x, v = _dev(c["x"]), _dev(c["v"])
    xo, ho, vo = m(_dev(c["his"]), x, [_dev(c["row"]), _dev(c["col"])], v, _dev(c["edge_attr"]), T=3)
    assert xo is x and vo is v and ho.shape == (n, 64) and ho.requires_grad
    graph.sync_checks()
