"""Training on device-built neighbour graphs: the CSR by sender of a NeighborGraph
(nonode_neighbor_by_sender) bitwise against graph.csr_by_sender of the compacted list, a taped forward of
EGNO(graph="trainable") on the padded graph against the compacted one and float64 autograd, the taped
featuriser (harness.prepare_inputs_graph(tape=True)), unrolled rollout training on graphs rebuilt every
segment (harness.egno_rollout_train_graph) against float64 autograd of the same loop in torch
(oracle/torch_ref.py), and that none of it reads the device.

Shapes: B = 2 graphs of N = 37 nodes (no multiple of the 16-receiver tile, more than one workgroup of the
per-node kernels), k = 6, a cut-off that leaves a -1 tail, T = 4 frames and 2 layers: the smallest at which
every path of the padded list (tail rows, ragged tiles, several senders per wave round) is taken. The hub
case has one sender of out-degree 199 (more than the 64 lanes of the rank sort's round).
"""
import numpy as np
import pytest
import torch

import no_node_comparison_amd as pkg
from no_node_comparison_amd import graph, harness
from oracle import torch_ref as tr
from tests._graph_case import sparse_graph
from tests._neighbor_ref import neighbor_ref
from tests.conftest import check_rel, maxnorm_rel
from tests.test_gpu_graph_train import _check_model, _f64_model, _loss, _weights
from tests.test_gpu_neighbor import _rollout_inputs, _points
from tests.test_gpu_train import _hip_lrelu_masks

pytestmark = pytest.mark.gpu
TOL = 1e-5      # the project's gradient bar (tests/test_gpu_graph_train.py)
MARGIN = 4      # later rollout segments: max(TOL, MARGIN x the float32 torch loop's own error) (tests/test_gpu_neighbor.py)
DEV = "cuda"
F64 = torch.float64


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a)).to(DEV)


def _model(T=4, n_layers=2, seed=0, device=DEV, **kw):
    """An untrained EGNO(graph="trainable") in train mode."""
    torch.manual_seed(seed)
    m = pkg.EGNO(n_layers=n_layers, in_node_nf=2, in_edge_nf=2, hidden_nf=64, with_v=True, num_modes=2,
                 num_timesteps=T, time_emb_dim=32, device=device, graph="trainable", **kw)
    return m.train()


# ---- 1. the CSR by sender ------------------------------------------------------------------------------
def hub_points(N=200):
    """N - 1 points on a sphere of radius 1e25 around a point at the origin (index 0). In exact arithmetic no
    199 points can each have the centre as their nearest neighbour (at equal radii that needs pairwise angles
    above 60 degrees: twelve points at the most), so the hub is made through the builder's total order (d2, j):
    every float32 squared distance here overflows to +inf, all candidates tie, and the tie goes to the smallest
    index: the centre for every other node, node 1 for the centre."""
    rs = np.random.RandomState(5)
    u = rs.randn(N - 1, 3)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return np.concatenate([np.zeros((1, 3)), u * 1e25]).astype(np.float32)


def _nan_points():
    x = _points(2, 37, 4)
    x[40, 1] = np.nan
    return x


SENDER_CASES = {
    "cap0": (1, 1, 4, None, lambda: _points(1, 1, 11)),
    "pairs": (2, 2, 1, None, lambda: _points(2, 2, 11)),
    "knn": (3, 37, 6, None, lambda: _points(3, 37, 11)),
    "full": (1, 37, 64, None, lambda: _points(1, 37, 11)),
    "k16": (2, 80, 16, None, lambda: _points(2, 80, 11)),
    "cutoff": (2, 37, 6, 1.5, lambda: _points(2, 37, 11)),
    "hub": (1, 200, 1, None, hub_points),
    "nan": (2, 37, 6, None, _nan_points),
    "full130": (1, 130, 64, None, lambda: _points(1, 130, 11)),   # out-degrees up to 129: three rounds of the sort
}


@pytest.mark.parametrize("name", sorted(SENDER_CASES))
def test_sender_csr_is_bitwise_the_compacted_lists(name):
    B, N, k, r_cut, points = SENDER_CASES[name]
    with np.errstate(over="ignore", invalid="ignore"):
        x = points()
        ref = neighbor_ref(x, B, N, k, r_cut)
    out_deg = np.bincount(ref["col"][:ref["E"]], minlength=B * N)
    if name == "hub":       # checked of the numpy reference first
        assert out_deg[0] == 199 and out_deg[1] == 1 and not out_deg[2:].any()
    if name == "full":
        assert np.all(out_deg == 36)
    if name == "cutoff":
        assert (ref["deg"] == 0).any() and 0 < ref["E"] < ref["cap"]
    if name == "nan":
        assert out_deg[40] == 0 and ref["deg"][40] == 0
    ng = graph.neighbor_graph(_dev(x), B, N, k, r_cut, by_sender=True)
    again = graph.neighbor_graph(_dev(x), B, N, k, r_cut, by_sender=True)
    plain = graph.neighbor_graph(_dev(x), B, N, k, r_cut)
    assert plain.srow_ptr is None and plain.seid is None and plain.valid is None
    lifted = plain.with_sender_csr()
    assert lifted is not plain and lifted.rows is plain.rows and lifted.with_sender_csr() is lifted
    assert ng.with_sender_csr() is ng
    E = int(ng.n_edges)
    cap = ng.capacity
    assert E == ref["E"] and cap == ref["cap"] and np.array_equal(ng.col.cpu().numpy(), ref["col"])
    for t, shape in ((ng.srow_ptr, (B * N + 1,)), (ng.seid, (cap,)), (ng.valid, (cap,))):
        assert t.dtype == torch.int32 and tuple(t.shape) == shape and t.is_cuda
    srow_ptr, seid, _ = graph.csr_by_sender(ng.edge_index(), B * N)
    assert torch.equal(ng.srow_ptr, srow_ptr)
    assert torch.equal(ng.seid[:E], seid)
    assert bool((ng.seid[E:] == -1).all())
    assert torch.equal(ng.valid, (torch.arange(cap, device=DEV) < E).to(torch.int32))
    assert np.array_equal(np.diff(ng.srow_ptr.cpu().numpy()), out_deg)
    for other in (again, lifted):
        for a in ("srow_ptr", "seid", "valid"):
            assert torch.equal(getattr(other, a), getattr(ng, a)), a
    got = graph.csr_by_sender(ng, B * N)
    assert got[0] is ng.srow_ptr and got[1] is ng.seid and got[2] is ng.valid
    graph.sync_checks()


# ---- 2. a taped forward on the padded graph --------------------------------------------------------------
def _taped_run(m, x, h, v, lm, t_out, edges, ef, w):
    """One taped forward + backward on `edges`: (outputs, input gradients, parameter gradients, masks)."""
    ins = [t.clone().requires_grad_(True) for t in (x, h, v, lm)]
    m.zero_grad(set_to_none=True)
    m._train_bwd_sink = []
    out = m(ins[0], ins[1], edges, ef, v=ins[2], loc_mean=ins[3], timesteps_out=t_out)
    _loss(*out, *w, 1.0).backward()
    torch.cuda.synchronize()
    sink = dict(m._train_bwd_sink)
    del m._train_bwd_sink
    masks = None
    if m.use_time_conv:
        masks = [_hip_lrelu_masks(sink[i], 1, m.num_timesteps, x.shape[0])[0] for i in range(m.n_layers)]
    return ([o.detach() for o in out], [t.grad for t in ins],
            {k: q.grad.clone() for k, q in m.named_parameters() if q.grad is not None}, masks)


@pytest.mark.parametrize("name,opts", [("default", {}), ("norm", dict(norm=True)),
                                       ("no_time_conv", dict(use_time_conv=False)),
                                       ("norm_no_time_conv", dict(norm=True, use_time_conv=False))])
def test_taped_forward_on_the_padded_graph_equals_the_compacted_list(name, opts):
    B, N, k, T = 2, 37, 6, 4
    n = B * N
    rs = np.random.RandomState(21)
    x = _points(B, N, 11)
    v = (rs.randn(n, 3) * 0.3).astype(np.float32)
    h = rs.randn(n, 2).astype(np.float32)
    lm = np.repeat(x.reshape(B, N, 3).mean(1, keepdims=True), N, 1).reshape(n, 3).astype(np.float32)
    t_out = np.arange(T, dtype=np.float32)[None]
    ng = graph.neighbor_graph(_dev(x), B, N, k, 3.0, by_sender=True)
    E = int(ng.n_edges)
    assert 0 < E < ng.capacity             # a non-empty tail
    ef = rs.randn(ng.capacity, 2).astype(np.float32)
    ef_nan = _dev(ef)
    ef_nan[E:] = float("nan")              # the tail is never read
    m = _model(T, **opts)
    w = [_dev(a) for a in _weights(n, T, n)]
    dx, dh, dv, dlm, dt = _dev(x), _dev(h), _dev(v), _dev(lm), _dev(t_out)
    pad = _taped_run(m, dx, dh, dv, dlm, dt, ng, ef_nan, w)
    comp = _taped_run(m, dx, dh, dv, dlm, dt, ng.edge_index(), _dev(ef[:E]), w)
    for tag, a, b in zip(("x", "v", "h"), pad[0], comp[0]):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), tag
    for tag, a, b in zip(("x", "h", "v", "loc_mean"), pad[1], comp[1]):
        if tag == "loc_mean" and not m.use_time_conv:
            assert a is None or not bool(a.any())
            continue
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), tag
    assert sorted(pad[2]) == sorted(comp[2])
    for key in pad[2]:
        assert bool(torch.isfinite(pad[2][key]).all()), key
        if float(comp[2][key].abs().max()) == 0:
            assert not bool(pad[2][key].any()), key
            continue
        check_rel(f"{name} padded vs compacted grad {key}", pad[2][key], comp[2][key], TOL)
    # both against float64 autograd: the compacted run through _check_model, the padded one by the same
    # comparison at the same decisions (its forward is bitwise the compacted one's)
    row, col = (t.cpu().numpy() for t in ng.edge_index())
    c = dict(x=x, h=h, v=v, loc_mean=lm, t_out=t_out, row=row, col=col, edge_fea=ef[:E])
    fopts = dict(n_layers=m.n_layers, **opts)
    _check_model(f"{name} compacted", m, c, fopts)
    kw = dict(lrelu_masks=pad[3]) if pad[3] is not None else {}
    ro, _, p, rin = _f64_model(m, c, _weights(n, T, n), fopts, **kw)
    for tag, a, b in zip("xvh", pad[0], ro):
        check_rel(f"{name} padded out {tag}", a, b, TOL)
    for key, q in m.named_parameters():
        r = p[key].grad
        if r is None or float(r.abs().max()) == 0:
            assert key not in pad[2] or float(pad[2][key].abs().max()) <= 1e-6, key
            continue
        check_rel(f"{name} padded grad {key}", pad[2][key], r, TOL)
    for tag, a in zip(("x", "h", "v", "loc_mean"), pad[1]):
        if tag == "loc_mean" and not m.use_time_conv:
            continue
        check_rel(f"{name} padded dL/d{tag}", a, rin[tag], TOL)
    graph.sync_checks()


# ---- 3. the taped featuriser -------------------------------------------------------------------------------
def test_prepare_inputs_graph_on_the_tape():
    F, B, N, k = 4, 3, 5, 2
    rs = np.random.RandomState(31)
    loc = rs.randn(F, B, N, 3).astype(np.float32)
    vel = (rs.randn(F, B, N, 3) * 0.3).astype(np.float32)
    q = rs.choice([-1.0, 1.0], size=(B, N, 1)).astype(np.float32)
    t_in = np.array([4, 1, 2])
    fr = t_in - 1
    wx, wv, wl = (rs.randn(B * N, 3).astype(np.float32) for _ in range(3))
    dl, dv_ = _dev(loc).requires_grad_(True), _dev(vel).requires_grad_(True)
    x, v, ea, nodes, lm, ng = harness.prepare_inputs_graph(dl, dv_, N, _dev(q), _dev(t_in), k=k, tape=True)
    assert x.grad_fn is not None and v.grad_fn is not None and lm.grad_fn is not None
    assert nodes.grad_fn is None and ea.grad_fn is None and not nodes.requires_grad and not ea.requires_grad
    assert isinstance(ng, graph.NeighborGraph) and ng.has_sender_csr()
    ((x * _dev(wx)).sum() + (v * _dev(wv)).sum() + (lm * _dev(wl)).sum()).backward()
    x0, v0, ea0, nodes0, lm0, ng0 = harness.prepare_inputs_graph(_dev(loc), _dev(vel), N, _dev(q), _dev(t_in), k=k)
    torch.cuda.synchronize()
    assert ng0.srow_ptr is None      # the default builds the receiver CSR alone
    for a, b in ((x, x0), (v, v0), (ea, ea0), (nodes, nodes0), (lm, lm0), (ng.col, ng0.col), (ng.row_ptr, ng0.row_ptr)):
        assert torch.equal(a.detach(), b)
    # float64 autograd of the torch restatement on the selected frames
    l64, v64 = torch.tensor(loc).to(F64).requires_grad_(True), torch.tensor(vel).to(F64).requires_grad_(True)
    row, col = (t.cpu() for t in ng.edge_index())
    q64 = torch.tensor(q).to(F64)
    eo = (q64.reshape(-1)[row] * q64.reshape(-1)[col])[:, None]
    ar = torch.arange(B)
    rx, rv, _, _, rlm = tr.prepare_inputs(l64[torch.tensor(fr), ar], v64[torch.tensor(fr), ar], eo, row, col, N, q64)
    ((rx * torch.tensor(wx)).sum() + (rv * torch.tensor(wv)).sum() + (rlm * torch.tensor(wl)).sum()).backward()
    check_rel("prepare_inputs_graph dL/dloc", dl.grad, l64.grad, 1e-6)
    check_rel("prepare_inputs_graph dL/dvel", dv_.grad, v64.grad, 1e-6)
    keep = np.zeros((F, B), dtype=bool)
    keep[fr, np.arange(B)] = True
    for g in (dl.grad, dv_.grad):
        assert not g.cpu().numpy()[~keep].any()      # unselected frames: exact zeros
        assert g.cpu().numpy()[keep].any()


# ---- 4. unrolled training on rebuilt graphs -------------------------------------------------------------------
def torch_rollout(p, loc, vel, q, lists, B, N, T, fr, t_out, n_layers, masks=None):
    """The loop of egno_rollout_train_graph in torch on the fixed lists `lists` (one (row, col) per segment):
    oracle/torch_ref.prepare_inputs with detached nodes / edge_attr, torch_ref.egno_forward, frame fr[b] of
    sample b as the next input. masks[i]: segment i's per-layer LeakyReLU decisions. Returns loc_preds
    [len(lists) * T, BN, 3] in the dtype of loc."""
    preds = []
    qf = q.reshape(-1)
    ar = torch.arange(B)
    for i, (row, col) in enumerate(lists):
        row, col = torch.as_tensor(row).long(), torch.as_tensor(col).long()
        eo = (qf[row] * qf[col])[:, None]
        x, v, ea, nodes, lm = tr.prepare_inputs(loc, vel, eo, row, col, N, q)
        t = (t_out[:, i * T:(i + 1) * T] - i * T).to(loc.dtype)
        kw = {} if masks is None else dict(lrelu_masks=masks[i])
        lo, vo, _ = tr.egno_forward(p, x, nodes.detach(), row, col, ea.detach(), v, lm, t, n_layers=n_layers, T=T, **kw)
        preds.append(lo.reshape(T, B * N, 3))
        loc, vel = lo.reshape(T, B, N, 3)[fr, ar], vo.reshape(T, B, N, 3)[fr, ar]
    return torch.cat(preds)


def _torch_grads(m, loc, vel, q, lists, B, N, T, fr, target, masks, dtype):
    p = {k: t.detach().cpu().to(dtype).requires_grad_(True) for k, t in m.state_dict().items()}
    l, v = (torch.tensor(a).to(dtype).requires_grad_(True) for a in (loc, vel))
    L = len(lists)
    t_out = torch.arange(T * L)[None]
    preds = torch_rollout(p, l, v, torch.tensor(q).to(dtype), lists, B, N, T, torch.as_tensor(fr), t_out, m.n_layers,
                          masks)
    zero = torch.zeros((), dtype=dtype)
    loss = _loss(preds, zero, zero, torch.tensor(target).to(dtype), zero, zero, 1.0)
    loss.backward()
    out = {"loss": loss.detach().reshape(1), "dL/dloc": l.grad, "dL/dvel": v.grad}
    out.update({f"grad {k}": t.grad for k, t in p.items() if t.grad is not None})
    return preds.detach(), out


def _check_rollout_train(tag, B, N, T, L, seed, t_in, **source):
    """egno_rollout_train_graph + backward against float64 autograd of torch_rollout on the graphs the driver
    used, at the HIP reverse's LeakyReLU decisions; every quantity at max(TOL, MARGIN x e32), e32 the error of
    the float32 torch loop (same lists, same decisions) against the float64 one for that quantity."""
    n = B * N
    loc, vel, q = _rollout_inputs(B, N, seed)
    # The untrained model as it is, without damping its coordinate and velocity heads: checked on the CPU with
    # the float64 loop alone at T = 4 and these seeds, the positions stay finite and of moderate size over the
    # segments (largest |loc| 5.5 -> 7.3 on the rebuilt 6-NN graphs, 5.8 -> 22.5 on the fixed sparse list).
    m = _model(T)
    target = _weights(n, L * T, n)[0].reshape(L * T, n, 3)
    dl, dv = _dev(loc).requires_grad_(True), _dev(vel).requires_grad_(True)
    ti = None if t_in is None else _dev(np.asarray(t_in))
    m.zero_grad(set_to_none=True)
    m._train_bwd_sink = []
    preds, graphs = harness.egno_rollout_train_graph(m, dl, dv, _dev(q), N, B, L, timesteps_in=ti,
                                                     return_graphs=True, **source)
    assert preds.grad_fn is not None and tuple(preds.shape) == (L * T, n, 3) and len(graphs) == L
    zero = torch.zeros((), device=DEV)
    loss = _loss(preds, zero, zero, _dev(target), zero, zero, 1.0)
    loss.backward()
    torch.cuda.synchronize()
    sink = m._train_bwd_sink
    del m._train_bwd_sink
    # the sink fills in backward order: the last segment first, and within a segment the last layer first
    assert [i for i, _ in sink] == list(range(m.n_layers - 1, -1, -1)) * L
    masks = []
    for s in range(L):
        seg = dict(sink[(L - 1 - s) * m.n_layers:(L - s) * m.n_layers])
        masks.append([_hip_lrelu_masks(seg[i], 1, T, n)[0] for i in range(m.n_layers)])
    got_preds = preds.detach().cpu().numpy()
    assert np.isfinite(got_preds).all()
    fr = np.full(B, T - 1) if t_in is None else (np.asarray(t_in) - 1) % T
    lists, start = [], loc.reshape(-1, 3)
    for i, g in enumerate(graphs):
        if i:
            start = got_preds[(i - 1) * T:i * T].reshape(T, B, N, 3)[fr, np.arange(B)].reshape(-1, 3)
        if isinstance(g, graph.NeighborGraph):
            ref = neighbor_ref(start, B, N, source["k"], source.get("r_cut"))
            assert g.has_sender_csr() and int(g.n_edges) == ref["E"]
            for a in ("row_ptr", "col", "rows", "eid"):
                assert np.array_equal(getattr(g, a).cpu().numpy(), ref[a]), (i, a)
            lists.append(tuple(t.cpu().numpy() for t in g.edge_index()))
        else:
            assert g is source["edges"]
            lists.append(tuple(t.cpu().numpy() for t in g))
    p64, r64 = _torch_grads(m, loc, vel, q, lists, B, N, T, fr, target, masks, F64)
    p32, r32 = _torch_grads(m, loc, vel, q, lists, B, N, T, fr, target, masks, torch.float32)
    got = {"loss": loss.detach().reshape(1), "dL/dloc": dl.grad, "dL/dvel": dv.grad}
    got.update({f"grad {k}": t.grad for k, t in m.named_parameters() if t.grad is not None})
    lines, failed = [], []
    for i in range(L):
        own = maxnorm_rel(p32[i * T:(i + 1) * T].numpy(), p64[i * T:(i + 1) * T].numpy())
        err = maxnorm_rel(got_preds[i * T:(i + 1) * T], p64[i * T:(i + 1) * T].numpy())
        lines.append((f"loc_preds segment {i + 1}", err, own, max(TOL, MARGIN * own)))
    for key, ref in r64.items():
        if float(ref.abs().max()) == 0:
            assert key not in got or not bool(got[key].any()), key
            continue
        own = maxnorm_rel(r32[key].numpy(), ref.numpy())
        lines.append((key, maxnorm_rel(got[key].detach().cpu().numpy(), ref.numpy()), own, max(TOL, MARGIN * own)))
    for key, err, own, bar in lines:
        print(f"{tag} {key}: error {err:.3e}  e32 {own:.3e}  bar {bar:.3e}")
        if not err < bar:
            failed.append((key, err, bar))
    assert not failed, failed
    graph.sync_checks()


def test_unrolled_training_on_rebuilt_graphs():
    _check_rollout_train("knn", 2, 37, 4, 2, 3, [0, 3], k=6)


def test_unrolled_training_on_a_fixed_list():
    row, col = sparse_graph(37)
    _check_rollout_train("fixed", 1, 37, 4, 2, 43, None, edges=[_dev(row), _dev(col)])


# ---- 5. nothing reads the device ---------------------------------------------------------------------------------
def test_training_on_rebuilt_graphs_does_not_synchronise():
    B, N, k, T = 2, 37, 6, 4
    n = B * N
    loc, vel, q = _rollout_inputs(B, N, 53)
    m = _model(T)
    opt = torch.optim.Adam(m.parameters(), lr=1e-4)
    a = dict(loc=_dev(loc), vel=_dev(vel), q=_dev(q), t_in=_dev(np.array([0, 3])),
             w=[_dev(t) for t in _weights(n, T, 1)], target=_dev(_weights(n, 2 * T, 2)[0].reshape(2 * T, n, 3)),
             t_out=_dev(np.arange(T, dtype=np.float32)[None]), zero=torch.zeros((), device=DEV))

    def run():
        ng = graph.neighbor_graph(a["loc"].reshape(n, 3), B, N, k, 3.0, by_sender=True)
        assert ng.has_sender_csr()
        loc_g = a["loc"].clone().requires_grad_(True)
        x, v, ea, nodes, lm, g = harness.prepare_inputs_graph(loc_g, a["vel"], N, a["q"], k=k, r_cut=3.0, tape=True)
        opt.zero_grad(set_to_none=True)
        out = m(x, nodes, g, ea, v=v, loc_mean=lm, timesteps_out=a["t_out"])
        _loss(*out, *a["w"], 1.0).backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
        preds = harness.egno_rollout_train_graph(m, loc_g, a["vel"], a["q"], N, B, 2, k=k, r_cut=3.0,
                                                 timesteps_in=a["t_in"])
        _loss(preds, a["zero"], a["zero"], a["target"], a["zero"], a["zero"], 1.0).backward()

    run()                                   # warm-up: weight packing, allocator, the optimizer's state
    torch.cuda.synchronize()
    probe = torch.ones(1, device=DEV)
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            raises = False
        except RuntimeError:
            raises = True
        if raises:
            run()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    if not raises:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not raise on .item() in this torch build")


# ---- 6. optimizer steps on a graph rebuilt each step ------------------------------------------------------------
def test_three_adam_steps_on_a_graph_rebuilt_each_step():
    """Re-packed blobs and a fresh sender CSR per step: the taped outputs of the third step against the eval
    forward (graph="any") on the same graph and weights."""
    B, N, k, T = 2, 37, 6, 4
    n = B * N
    loc, vel, q = _rollout_inputs(B, N, 61)
    m = _model(T)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    w = [_dev(t) for t in _weights(n, T, 1)]
    t_out = _dev(np.arange(T, dtype=np.float32)[None])
    rs = np.random.RandomState(7)
    losses, cols = [], []
    for step in range(3):
        jit = _dev(loc + (rs.randn(B, N, 3) * 0.3).astype(np.float32))
        x, v, ea, nodes, lm, g = harness.prepare_inputs_graph(jit, _dev(vel), N, _dev(q), k=k, r_cut=3.0, tape=True)
        opt.zero_grad(set_to_none=True)
        out = m(x, nodes, g, ea, v=v, loc_mean=lm, timesteps_out=t_out)
        assert out[0].grad_fn is not None
        loss = _loss(*out, *w, 1.0)
        loss.backward()
        if step == 2:
            ev = pkg.EGNO(n_layers=m.n_layers, in_node_nf=2, in_edge_nf=2, hidden_nf=64, with_v=True, num_modes=2,
                          num_timesteps=T, time_emb_dim=32, device=DEV, graph="any")
            ev.load_state_dict(m.state_dict())
            with torch.no_grad():
                ref = ev.eval()(x, nodes, g, ea, v=v, loc_mean=lm, timesteps_out=t_out)
            for tag, a_, b_ in zip("xvh", out, ref):
                check_rel(f"step 3 taped vs eval {tag}", a_, b_, 1e-6)
        opt.step()
        losses.append(float(loss.detach()))
        cols.append(g.col.cpu().numpy().copy())
    assert all(np.isfinite(losses)) and losses[2] != losses[0]
    assert any(not np.array_equal(cols[0], c) for c in cols[1:])      # the graph did change
    graph.sync_checks()
