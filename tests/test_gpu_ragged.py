"""GPU tests of graphs of mixed sizes in one batch: graph.RaggedBatch / neighbor_graph_ragged, the sizes=
argument of harness.prepare_inputs_graph / conserved_energy, and the four general-graph rollout drivers.

Builder: bitwise against tests/_ragged_ref.ragged_neighbor_ref (tests/_neighbor_ref.neighbor_ref per graph).
Equal sizes: bitwise the equal-size path (the kernels are the same; a graph's bounds come from the descriptor).
Featuriser, energies: against oracle/harness.py per graph (tests/_ragged_ref.py), rtol = atol = 1e-6.
Models: the padded graph against its compacted list, torch.equal.
Rollouts: every segment's graph bitwise the reference on the positions the driver started it from; positions
and energies against the float64 oracle on the driver's own lists with each graph's own mean, frame choice and
energy, by the rule of tests/test_gpu_neighbor._check_segments (segment 1 at 1e-5, later ones at
max(1e-5, 4 x the float32 oracle's own error)). The oracle's forward runs on the whole batch at once: no edge
crosses a graph boundary (asserted), so that is the per-graph forward.
Unrolled training: float64 autograd of the torch loop on the driver's own lists (EGNO: at the HIP reverse's
LeakyReLU decisions), every quantity at max(1e-5, 4 x e32).
"""
import itertools

import numpy as np
import pytest
import torch

from no_node_comparison_amd import graph, harness
from oracle import egno as oe
from oracle import segno as osg
from oracle import torch_ref as tr
from tests._ragged_ref import offsets, ragged_energy, ragged_neighbor_ref, ragged_prepare_inputs
from tests.conftest import check_rel, maxnorm_rel, params_of
from tests.test_gpu_graph_train import _loss, _weights
from tests.test_gpu_neighbor import (CUT_R, _assert_bitwise, _check_segments, _close, _edge_lists, _egno, _segno,
                                     egno_fx, segno_fx)  # noqa: F401  (fixtures)
from tests.test_gpu_neighbor_train import MARGIN, TOL, _model
from tests.test_gpu_segno_graph_train import _p64
from tests.test_gpu_segno_graph_train import _segno as _segno_train
from tests.test_gpu_train import _hip_lrelu_masks

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
SIZES = (1, 2, 5, 37, 64, 65, 130, 3, 1)     # the smallest sizes that reach every branch of the builder
ROLL = (5, 37, 1, 20, 2)                     # n = 65: the last 16-node tile holds one row


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a)).to(DEV)


def _cloud():
    return (np.random.RandomState(11).randn(308, 3) * 1.5).astype(np.float32)


def _build(x, sizes, k, r_cut=None, **kw):
    ng = graph.neighbor_graph_ragged(_dev(x), sizes, k, r_cut, **kw)
    torch.cuda.synchronize()
    assert ng.n_nodes is None and ng.batch.sizes == tuple(sizes) and ng.capacity == ng.batch.capacity(k)
    return ng


def _no_edge_leaves_its_graph(ref, sizes):
    off = offsets(sizes)
    of = np.repeat(np.arange(len(sizes)), sizes)
    E = ref["E"]
    assert np.array_equal(of[ref["rows"][:E]], of[ref["col"][:E]])
    assert np.all(ref["deg"] <= np.repeat(np.asarray(sizes) - 1, sizes)) and off[-1] == len(of)


# ---- 1. the builder ----------------------------------------------------------------------------------------
BUILDER = {(1, None): (306, 306), (6, None): (1804, 1804), (64, None): (17872, 17872), (6, 1.5): (1207, 1804),
           (64, 1.5): (1840, 17872), (16, 2.0): (3117, 4764)}


@pytest.mark.parametrize("k,r_cut", list(BUILDER))
def test_builder_matches_the_ragged_reference_bitwise(k, r_cut):
    x = _cloud()
    ref = ragged_neighbor_ref(x, SIZES, k, r_cut)
    assert (ref["E"], ref["cap"]) == BUILDER[(k, r_cut)]
    _no_edge_leaves_its_graph(ref, SIZES)
    off = offsets(SIZES)
    deg = [ref["deg"][off[g]:off[g + 1]] for g in range(len(SIZES))]
    assert all(not deg[g].any() for g in (0, 8))               # graphs of one node
    if (k, r_cut) == (64, None):
        assert np.all(deg[4] == 63) and np.all(deg[5] == 64) and np.all(deg[6] == 64)
    if (k, r_cut) == (6, 1.5):
        assert all((deg[g] == 0).any() and (deg[g] == 6).any() for g in (3, 4, 5, 6))
    if (k, r_cut) == (64, 1.5):
        assert ref["deg"].max() == 24
    _assert_bitwise(_build(x, SIZES, k, r_cut), ref)


def test_nothing_leaks_across_graph_boundaries():
    """Every graph holds the first N_g points of one common cloud: a node's nearest point in the neighbouring
    graph is at distance 0."""
    cloud = (np.random.RandomState(5).randn(130, 3) * 1.5).astype(np.float32)
    x = np.concatenate([cloud[:n] for n in SIZES])
    ref = ragged_neighbor_ref(x, SIZES, 6)
    assert ref["E"] == ref["cap"] == 1804
    _no_edge_leaves_its_graph(ref, SIZES)
    _assert_bitwise(_build(x, SIZES, 6), ref)


# ---- 3. equal sizes reproduce the equal-size path -----------------------------------------------------------
@pytest.mark.parametrize("sizes", [(37, 37, 37), (80, 80)])
def test_equal_sizes_are_bitwise_the_equal_size_path(sizes):
    B, N = len(sizes), sizes[0]
    n = B * N
    rs = np.random.RandomState(17)
    x = (rs.randn(n, 3) * 1.5).astype(np.float32)
    for k, r_cut in ((6, None), (16, 2.0), (64, None)):
        a = graph.neighbor_graph_ragged(_dev(x), sizes, k, r_cut, by_sender=True)
        b = graph.neighbor_graph(_dev(x), B, N, k, r_cut, by_sender=True)
        assert a.capacity == b.capacity
        for name in ("row_ptr", "col", "rows", "eid", "srow_ptr", "seid", "valid"):
            assert torch.equal(getattr(a, name), getattr(b, name)), (k, r_cut, name)
    F = 3
    loc, vel = rs.randn(F, n, 3).astype(np.float32), (rs.randn(F, n, 3) * 0.3).astype(np.float32)
    q = rs.choice([-1.0, 1.0], size=n).astype(np.float32)
    t_in = _dev(np.arange(B) % F)
    got = harness.prepare_inputs_graph(_dev(loc), _dev(vel), None, _dev(q), t_in, k=6, r_cut=2.0, sizes=sizes)
    want = harness.prepare_inputs_graph(_dev(loc.reshape(F, B, N, 3)), _dev(vel.reshape(F, B, N, 3)), N, _dev(q), t_in,
                                        k=6, r_cut=2.0)
    for name, a, b in zip(("x", "v", "edge_attr", "nodes", "loc_mean"), got, want):
        assert torch.equal(a, b), name
    assert torch.equal(got[5].col, want[5].col) and torch.equal(got[5].row_ptr, want[5].row_ptr)
    for kind in ("charged", "gravity"):
        w = _dev(q) if kind == "charged" else _dev(np.abs(rs.randn(n)).astype(np.float32) + 0.5)
        e_r = harness.conserved_energy(kind, _dev(loc), _dev(vel), w, None, sizes=sizes)
        e_e = harness.conserved_energy(kind, _dev(loc), _dev(vel), w, B)
        assert e_r.shape == (F, B) and torch.equal(e_r, e_e), kind


# ---- 4. special inputs ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("r_cut", [None, 2.0])
def test_builder_with_a_nan_coordinate(r_cut):
    x = _cloud()
    x[60, 1] = np.nan                      # a node of the 64-graph
    ref = ragged_neighbor_ref(x, SIZES, 6, r_cut)
    assert ref["deg"][60] == 0 and 60 not in ref["col"]
    _assert_bitwise(_build(x, SIZES, 6, r_cut), ref)


def test_builder_with_coincident_nodes():
    x = _cloud()
    x[10] = x[14]                          # in the 37-graph
    x[200] = x[180]                        # in the 130-graph
    x[1] = x[2]                            # the two nodes of the 2-graph
    ref = ragged_neighbor_ref(x, SIZES, 6)
    assert 14 in ref["col"][ref["row_ptr"][10]:ref["row_ptr"][11]]
    _assert_bitwise(_build(x, SIZES, 6), ref)


@pytest.mark.parametrize("k,r_cut", [(4, 1.0), (3, None)])
def test_builder_on_a_lattice_breaks_ties_by_index(k, r_cut):
    """The points of tests/test_gpu_neighbor._lattice() as graphs of 37 and 20: ties at the k-th place."""
    pts = np.array(list(itertools.product(range(4), range(4), range(3))), dtype=np.float32)[:37]
    x = np.concatenate([pts, pts[:20]])
    ref = ragged_neighbor_ref(x, (37, 20), k, r_cut)
    _assert_bitwise(_build(x, (37, 20), k, r_cut), ref)


# ---- 5. the CSR by sender -------------------------------------------------------------------------------------
def test_sender_csr_of_a_ragged_graph():
    x = _cloud()
    ng = _build(x, SIZES, 6, 1.5, by_sender=True)
    E = int(ng.n_edges.item())
    assert E == 1207 and ng.has_sender_csr()
    srow_ptr, seid, _ = graph.csr_by_sender(ng.edge_index(), 308)
    graph.sync_checks()
    assert torch.equal(ng.srow_ptr, srow_ptr) and torch.equal(ng.seid[:E], seid)
    assert ng.valid[:E].all() and not ng.valid[E:].any() and (ng.seid[E:] == -1).all()
    plain = _build(x, SIZES, 6, 1.5)
    assert not plain.has_sender_csr()
    late = plain.with_sender_csr()
    assert late.batch is plain.batch and late.n_nodes is None
    for name in ("srow_ptr", "seid", "valid"):
        assert torch.equal(getattr(late, name), getattr(ng, name)), name
    own = graph.csr_by_sender(ng, 308)
    assert own[0] is ng.srow_ptr and own[1] is ng.seid and own[2] is ng.valid


# ---- 6. the featuriser ----------------------------------------------------------------------------------------
FEAT = (3, 7, 1, 5)


def _feat_inputs(frames):
    n = sum(FEAT)
    rs = np.random.RandomState(31)
    shape = (frames, n, 3) if frames > 1 else (n, 3)
    loc = rs.randn(*shape).astype(np.float32)
    vel = (rs.randn(*shape) * 0.3).astype(np.float32)
    q = rs.choice([-1.0, 1.0], size=n).astype(np.float32)
    t_in = np.array([0, 2, 4, 1]) if frames > 1 else None      # frames -1 (the last), 1, 3, 0
    return loc, vel, q, t_in


def _select(a, t_in, sizes):
    """Frame (t_in[g] - 1) mod F of graph g's rows of a [F, n, 3]."""
    if t_in is None:
        return a
    off = offsets(sizes)
    fr = (np.asarray(t_in) - 1) % a.shape[0]
    return np.concatenate([a[fr[g], off[g]:off[g + 1]] for g in range(len(sizes))])


@pytest.mark.parametrize("frames,r_cut", [(4, None), (1, None), (4, 1.2), (1, 1.2)])
def test_prepare_inputs_graph_with_sizes_matches_the_oracle_per_graph(frames, r_cut):
    k = 3
    loc, vel, q, t_in = _feat_inputs(frames)
    batch = graph.RaggedBatch(FEAT, DEV)
    x, v, ea, nodes, lm, ng = harness.prepare_inputs_graph(
        _dev(loc), _dev(vel), None, _dev(q), _dev(t_in) if t_in is not None else None, k=k, r_cut=r_cut, sizes=batch)
    torch.cuda.synchronize()
    loc_s, vel_s = _select(loc, t_in, FEAT), _select(vel, t_in, FEAT)
    assert torch.equal(x, _dev(loc_s)) and torch.equal(v, _dev(vel_s))
    assert ng.batch is batch
    _assert_bitwise(ng, ragged_neighbor_ref(loc_s, FEAT, k, r_cut))
    E = int(ng.n_edges.item())
    assert ea.shape == (ng.capacity, 2) and (E < ng.capacity) == (r_cut is not None)
    row, col = (t.cpu().numpy() for t in ng.edge_index())
    ea_r, nodes_r, lm_r = ragged_prepare_inputs(loc_s.astype(np.float64), vel_s.astype(np.float64),
                                                q.astype(np.float64), FEAT, row, col)
    _close(ea[:E], ea_r)
    _close(nodes, nodes_r)
    _close(lm, lm_r)
    assert not ea[E:].any()                                     # rows at or past n_edges are zero
    x2, v2, ea2, nodes2, lm2, e2 = harness.prepare_inputs_graph(_dev(loc_s), _dev(vel_s), None, _dev(q), edges=ng,
                                                                sizes=batch)
    assert e2 is ng and torch.equal(ea2, ea) and torch.equal(nodes2, nodes) and torch.equal(lm2, lm)
    ea3 = harness.prepare_inputs_graph(_dev(loc_s), _dev(vel_s), None, _dev(q), edges=ng.edge_index(), sizes=FEAT)[2]
    assert ea3.shape == (E, 2) and torch.equal(ea3, ea[:E])
    # the energies of the same frames, per graph
    if frames > 1:
        en = harness.conserved_energy("charged", _dev(loc), _dev(vel), _dev(q), None, sizes=batch)
        assert en.shape == (frames, len(FEAT))
        want = np.stack([ragged_energy("charged", loc[f].astype(np.float64), vel[f].astype(np.float64),
                                       q.astype(np.float64), FEAT) for f in range(frames)])
        check_rel("ragged energy", en, want, 1e-6)


# ---- 7. the featuriser on the tape -------------------------------------------------------------------------------
def test_prepare_inputs_graph_with_sizes_on_the_tape():
    F, k = 4, 2
    n, G = sum(FEAT), len(FEAT)
    loc, vel, q, t_in = _feat_inputs(F)
    fr = (t_in - 1) % F
    off = offsets(FEAT)
    rs = np.random.RandomState(32)
    wx, wv, wl = (rs.randn(n, 3).astype(np.float32) for _ in range(3))
    dl, dv_ = _dev(loc).requires_grad_(True), _dev(vel).requires_grad_(True)
    x, v, ea, nodes, lm, ng = harness.prepare_inputs_graph(dl, dv_, None, _dev(q), _dev(t_in), k=k, tape=True,
                                                           sizes=FEAT)
    assert x.grad_fn is not None and v.grad_fn is not None and lm.grad_fn is not None
    assert nodes.grad_fn is None and ea.grad_fn is None and ng.has_sender_csr() and ng.batch is not None
    ((x * _dev(wx)).sum() + (v * _dev(wv)).sum() + (lm * _dev(wl)).sum()).backward()
    x0, v0, ea0, nodes0, lm0, ng0 = harness.prepare_inputs_graph(_dev(loc), _dev(vel), None, _dev(q), _dev(t_in), k=k,
                                                                 sizes=FEAT)
    torch.cuda.synchronize()
    for a, b in ((x, x0), (v, v0), (ea, ea0), (nodes, nodes0), (lm, lm0), (ng.col, ng0.col), (ng.row_ptr, ng0.row_ptr)):
        assert torch.equal(a.detach(), b)
    # float64 autograd of the per-graph restatement: the selected frame's rows, the graph's own mean
    l64, v64 = torch.tensor(loc).to(F64).requires_grad_(True), torch.tensor(vel).to(F64).requires_grad_(True)
    rx = torch.cat([l64[fr[g], off[g]:off[g + 1]] for g in range(G)])
    rv = torch.cat([v64[fr[g], off[g]:off[g + 1]] for g in range(G)])
    rlm = torch.cat([rx[off[g]:off[g + 1]].mean(0, keepdim=True).expand(FEAT[g], 3) for g in range(G)])
    ((rx * torch.tensor(wx)).sum() + (rv * torch.tensor(wv)).sum() + (rlm * torch.tensor(wl)).sum()).backward()
    check_rel("ragged prepare_inputs_graph dL/dloc", dl.grad, l64.grad, 1e-6)
    check_rel("ragged prepare_inputs_graph dL/dvel", dv_.grad, v64.grad, 1e-6)
    keep = np.zeros((F, n), dtype=bool)
    for g in range(G):
        keep[fr[g], off[g]:off[g + 1]] = True
    for g in (dl.grad, dv_.grad):
        assert not g.cpu().numpy()[~keep].any()      # unselected frames: exact zeros
        assert g.cpu().numpy()[keep].any()


# ---- 8. the models on a ragged graph ---------------------------------------------------------------------------
def _per_graph_mean(x, sizes):
    off = offsets(sizes)
    return torch.cat([x[off[g]:off[g + 1]].mean(0, keepdim=True).expand(sizes[g], 3) for g in range(len(sizes))])


@pytest.mark.parametrize("mode", ["any", "trainable"])
@pytest.mark.parametrize("r_cut", [None, CUT_R])
def test_models_on_a_ragged_graph_equal_the_compacted_list(egno_fx, segno_fx, r_cut, mode):  # noqa: F811
    n, k = sum(ROLL), 6
    rs = np.random.RandomState(21)
    x = _dev((np.random.RandomState(11).randn(n, 3) * 1.5).astype(np.float32))
    v = _dev((rs.randn(n, 3) * 0.3).astype(np.float32))
    h = _dev(rs.randn(n, 2).astype(np.float32))
    ng = graph.neighbor_graph_ragged(x, ROLL, k, r_cut)
    E = int(ng.n_edges.item())
    assert (E < ng.capacity) == (r_cut is not None) and ng.capacity == ng.batch.capacity(k) == 364
    ef = _dev(rs.randn(ng.capacity, 2).astype(np.float32))
    ef_nan = ef.clone()
    ef_nan[E:] = float("nan")          # the tail is never read
    lm = _per_graph_mean(x, ROLL).contiguous()
    me, ms = _egno(egno_fx, graph=mode), _segno(segno_fx)
    with torch.no_grad():
        full = me(x, h, ng, ef_nan, v=v, loc_mean=lm)
        comp = me(x, h, ng.edge_index(), ef[:E].contiguous(), v=v, loc_mean=lm)
        sfull = ms(h[:, :1].contiguous(), x, ng, v, ef_nan, T=5)
        scomp = ms(h[:, :1].contiguous(), x, ng.edge_index(), v, ef[:E].contiguous(), T=5)
    graph.sync_checks()
    lone = offsets(ROLL)[2]                # the node of the graph of one node
    for a, b in zip(full + sfull, comp + scomp):
        assert torch.isfinite(a).all() and torch.equal(a, b)
        assert torch.isfinite(a.reshape(-1, n, a.shape[-1])[:, lone]).all()


# ---- 9 / 10. the rollouts ---------------------------------------------------------------------------------------
def _rollout_inputs():
    rs = np.random.RandomState(7)
    n = sum(ROLL)
    loc = (rs.randn(n, 3) * 1.5).astype(np.float32)
    vel = (rs.randn(n, 3) * 0.3).astype(np.float32)
    q = rs.choice([-1.0, 1.0], size=n).astype(np.float32)
    return loc, vel, q


def _oracle_egno(p, loc, vel, q, lists, sizes, T, t_in, t_out, dt):
    """The oracle loop in dtype dt, segment i on lists[i]: each graph's own mean, energy and next frame."""
    p = {k: v.astype(dt) for k, v in p.items()}
    loc, vel, q = loc.astype(dt), vel.astype(dt), q.astype(dt)
    off, G, n = offsets(sizes), len(sizes), sum(sizes)
    fr = np.full(G, -1) if t_in is None else np.asarray(t_in).reshape(-1) - 1
    preds, ens = [], []
    for i, (row, col) in enumerate(lists):
        ea, nodes, lm = ragged_prepare_inputs(loc, vel, q, sizes, row, col)
        t = (t_out[:, i * T:(i + 1) * T] - i * T).astype(dt)
        lo, vo, _ = oe.egno_forward(p, loc, nodes, row, col, ea, vel, lm, t, T=T)
        assert lo.dtype == dt
        la, va = lo.reshape(T, n, 3), vo.reshape(T, n, 3)
        preds.append(la)
        ens.append(np.stack([ragged_energy("charged", la[j], va[j], q, sizes) for j in range(T)]))
        loc = np.concatenate([la[fr[g], off[g]:off[g + 1]] for g in range(G)])
        vel = np.concatenate([va[fr[g], off[g]:off[g + 1]] for g in range(G)])
    return preds, ens


def test_egno_rollout_on_a_ragged_batch(egno_fx):  # noqa: F811
    k, T, L = 6, 10, 3
    n, G = sum(ROLL), len(ROLL)
    loc, vel, q = _rollout_inputs()
    t_in = np.array([0, 3, 5, 0, 2])
    m = _egno(egno_fx, T)
    batch = graph.RaggedBatch(ROLL, DEV)
    preds, en, en_all, graphs = harness.egno_rollout_graph(
        m, _dev(loc), _dev(vel), _dev(q), None, None, L, k=k, timesteps_in=_dev(t_in), energy_dataset="charged",
        return_graphs=True, sizes=batch)
    lists = _edge_lists(graphs)
    preds = preds.cpu().numpy()
    assert preds.shape == (L * T, n, 3) and en.shape == (L, G, 1) and en_all.shape == (L * T, G, 1)
    assert len(graphs) == L and np.isfinite(preds).all() and all(g.batch is batch for g in graphs)
    start = loc
    for i, g in enumerate(graphs):
        if i:
            start = _select(preds[(i - 1) * T:i * T], t_in, ROLL)
        ref = ragged_neighbor_ref(start, ROLL, k)
        _no_edge_leaves_its_graph(ref, ROLL)
        _assert_bitwise(g, ref)
    p = params_of(egno_fx)
    t_out = np.arange(T * L)[None, :]
    p64, e64 = _oracle_egno(p, loc, vel, q, lists, ROLL, T, t_in, t_out, np.float64)
    p32, e32 = _oracle_egno(p, loc, vel, q, lists, ROLL, T, t_in, t_out, np.float32)
    _check_segments("egno ragged loc", [preds[i * T:(i + 1) * T] for i in range(L)], p64, p32)
    ea = en_all.cpu().numpy()[..., 0]
    _check_segments("egno ragged energy", [ea[i * T:(i + 1) * T] for i in range(L)], e64, e32)
    assert torch.equal(en, en_all[T - 1::T])


def test_segno_rollout_on_a_ragged_batch(segno_fx):  # noqa: F811
    k, steps = 6, [5, 7, 6]
    n, G = sum(ROLL), len(ROLL)
    loc, vel, q = _rollout_inputs()
    m = _segno(segno_fx)
    preds, en, graphs = harness.segno_rollout_graph(m, _dev(loc), _dev(vel), _dev(q), None, len(steps), steps, k=k,
                                                    energy_dataset="charged", return_graphs=True, sizes=ROLL)
    lists = _edge_lists(graphs)
    preds, en = preds.cpu().numpy(), en.cpu().numpy()
    assert preds.shape == (len(steps), n, 3) and en.shape == (len(steps), G, 1) and np.isfinite(preds).all()
    start = loc
    for i, g in enumerate(graphs):
        if i:
            start = preds[i - 1]
        ref = ragged_neighbor_ref(start, ROLL, k)
        assert np.array_equal(ref["deg"], np.repeat([min(k, s - 1) for s in ROLL], ROLL))   # pure k-NN
        _assert_bitwise(g, ref)
    out = {}
    for dt in (np.float64, np.float32):
        p = {kk: v.astype(dt) for kk, v in params_of(segno_fx).items()}
        x, v, qd = loc.astype(dt), vel.astype(dt), q.astype(dt)
        ps, es = [], []
        for (row, col), T in zip(lists, steps):
            his = np.sqrt(np.sum(v ** 2, axis=1))[:, None]
            prod = qd.reshape(-1, 1)[row] * qd.reshape(-1, 1)[col]
            ea = np.concatenate([prod, np.sum((x[row] - x[col]) ** 2, axis=1)[:, None]], axis=1).astype(dt)
            x, _, v = osg.forward_step(p, oe.linear(his, p, "embedding"), x, row, col, v, ea, T=T)
            assert x.dtype == dt
            ps.append(x)
            es.append(ragged_energy("charged", x, v, qd, ROLL)[:, None])
        out[dt] = (ps, es)
    _check_segments("segno ragged loc", list(preds), out[np.float64][0], out[np.float32][0])
    _check_segments("segno ragged energy", list(en), out[np.float64][1], out[np.float32][1])


# ---- 11. unrolled training ----------------------------------------------------------------------------------------
def _torch_egno_rollout(p, loc, vel, q, lists, sizes, T, fr, t_out, n_layers, masks):
    """The loop of egno_rollout_train_graph(sizes=...) in torch on the lists of the segments: the featurisation
    of oracle/torch_ref.prepare_inputs with the per-graph loc_mean written out, nodes and edge_attr detached,
    torch_ref.egno_forward, frame fr[g] of graph g's rows as the next input."""
    off, G, n = offsets(sizes), len(sizes), sum(sizes)
    preds = []
    for i, (row, col) in enumerate(lists):
        row, col = torch.as_tensor(row).long(), torch.as_tensor(col).long()
        lm = torch.cat([loc[off[g]:off[g + 1]].mean(0, keepdim=True).expand(sizes[g], 3) for g in range(G)])
        nodes = torch.cat([vel.norm(dim=1, keepdim=True), q.reshape(-1, 1)], 1)
        ea = torch.cat([(q[row] * q[col])[:, None], ((loc[row] - loc[col]) ** 2).sum(1, keepdim=True)], 1)
        t = (t_out[:, i * T:(i + 1) * T] - i * T).to(loc.dtype)
        lo, vo, _ = tr.egno_forward(p, loc, nodes.detach(), row, col, ea.detach(), vel, lm, t, n_layers=n_layers, T=T,
                                    lrelu_masks=masks[i])
        lo, vo = lo.reshape(T, n, 3), vo.reshape(T, n, 3)
        preds.append(lo)
        loc = torch.cat([lo[fr[g], off[g]:off[g + 1]] for g in range(G)])
        vel = torch.cat([vo[fr[g], off[g]:off[g + 1]] for g in range(G)])
    return torch.cat(preds)


def _torch_egno_grads(m, loc, vel, q, lists, sizes, T, fr, target, masks, dtype):
    p = {k: t.detach().cpu().to(dtype).requires_grad_(True) for k, t in m.state_dict().items()}
    l, v = (torch.tensor(a).to(dtype).requires_grad_(True) for a in (loc, vel))
    t_out = torch.arange(T * len(lists))[None]
    preds = _torch_egno_rollout(p, l, v, torch.tensor(q).to(dtype), lists, sizes, T, fr, t_out, m.n_layers, masks)
    zero = torch.zeros((), dtype=dtype)
    loss = _loss(preds, zero, zero, torch.tensor(target).to(dtype), zero, zero, 1.0)
    loss.backward()
    out = {"loss": loss.detach().reshape(1), "dL/dloc": l.grad, "dL/dvel": v.grad}
    out.update({f"grad {k}": t.grad for k, t in p.items() if t.grad is not None})
    return preds.detach(), out


def _compare(tag, got, r64, r32):
    failed = []
    for key, ref in r64.items():
        if float(ref.abs().max()) < 1e-12:   # zero, in exact arithmetic at least (tests/test_gpu_segno_graph_train.py)
            assert key not in got or got[key] is None or float(got[key].abs().max()) < 1e-7, key
            continue
        own = maxnorm_rel(r32[key].numpy(), ref.numpy())
        err = maxnorm_rel(got[key].detach().cpu().numpy(), ref.numpy())
        bar = max(TOL, MARGIN * own)
        print(f"{tag} {key}: error {err:.3e}  e32 {own:.3e}  bar {bar:.3e}")
        if not err < bar:
            failed.append((key, err, bar))
    assert not failed, failed


def test_unrolled_egno_training_on_a_ragged_batch():
    # The inputs of the rollout tests (seed 7) and the untrained two-layer model of tests/test_gpu_neighbor_train.py
    # at T = 4: checked on the CPU, the float64 loop alone, on the 6-NN lists rebuilt from its own positions,
    # has the largest |position| at 4.3 in the first and 5.6 in the second segment (seeds 3 and 5 reach 12 and 17).
    k, T, L = 6, 4, 2
    n, G = sum(ROLL), len(ROLL)
    loc, vel, q = _rollout_inputs()
    t_in = np.array([0, 3, 1, 0, 2])
    fr = (t_in - 1) % T
    m = _model(T)
    target = _weights(n, L * T, n)[0].reshape(L * T, n, 3)
    dl, dv = _dev(loc).requires_grad_(True), _dev(vel).requires_grad_(True)
    m.zero_grad(set_to_none=True)
    m._train_bwd_sink = []
    preds, graphs = harness.egno_rollout_train_graph(m, dl, dv, _dev(q), None, None, L, k=k, timesteps_in=_dev(t_in),
                                                     return_graphs=True, sizes=ROLL)
    assert preds.grad_fn is not None and tuple(preds.shape) == (L * T, n, 3) and len(graphs) == L
    zero = torch.zeros((), device=DEV)
    loss = _loss(preds, zero, zero, _dev(target), zero, zero, 1.0)
    loss.backward()
    torch.cuda.synchronize()
    sink = m._train_bwd_sink
    del m._train_bwd_sink
    assert [i for i, _ in sink] == list(range(m.n_layers - 1, -1, -1)) * L
    masks = []
    for s in range(L):
        seg = dict(sink[(L - 1 - s) * m.n_layers:(L - s) * m.n_layers])
        masks.append([_hip_lrelu_masks(seg[i], 1, T, n)[0] for i in range(m.n_layers)])
    got_preds = preds.detach().cpu().numpy()
    assert np.isfinite(got_preds).all()
    lists, start = [], loc
    for i, g in enumerate(graphs):
        if i:
            start = _select(got_preds[(i - 1) * T:i * T], t_in, ROLL)
        assert g.has_sender_csr() and g.batch is not None
        _assert_bitwise(g, ragged_neighbor_ref(start, ROLL, k))
        lists.append(tuple(t.cpu().numpy() for t in g.edge_index()))
    p64, r64 = _torch_egno_grads(m, loc, vel, q, lists, ROLL, T, fr, target, masks, F64)
    p32, r32 = _torch_egno_grads(m, loc, vel, q, lists, ROLL, T, fr, target, masks, torch.float32)
    got = {"loss": loss.detach().reshape(1), "dL/dloc": dl.grad, "dL/dvel": dv.grad}
    got.update({f"grad {k_}": t.grad for k_, t in m.named_parameters() if t.grad is not None})
    for i in range(L):
        got[f"loc_preds segment {i + 1}"] = preds.detach()[i * T:(i + 1) * T]
        r64[f"loc_preds segment {i + 1}"], r32[f"loc_preds segment {i + 1}"] = p64[i * T:(i + 1) * T], p32[i * T:(i + 1) * T]
    _compare("egno ragged train", got, r64, r32)
    graph.sync_checks()


def _torch_segno_grads(m, loc, vel, q, lists, steps, target, dtype):
    p = _p64(m, dtype)
    x, v = (torch.tensor(a).to(dtype).requires_grad_(True) for a in (loc, vel))
    qq = torch.tensor(q).to(dtype).reshape(-1, 1)
    xi, vi, out = x, v, []
    for (r, c), T in zip(lists, steps):
        r, c = torch.as_tensor(r).long(), torch.as_tensor(c).long()
        his = vi.detach().norm(dim=1, keepdim=True)
        ea = torch.cat([qq[r] * qq[c], ((xi.detach()[r] - xi.detach()[c]) ** 2).sum(1, keepdim=True)], 1)
        h = tr._lin(his, p, "embedding")
        for _ in range(T):
            h, xi, vi = tr.gcl(p, h, r, c, xi, vi, ea, T, dense_mean=False)
        out.append(xi)
    out = torch.stack(out)
    loss = torch.nn.functional.mse_loss(out, torch.tensor(target).to(dtype))
    loss.backward()
    res = {"loss": loss.detach().reshape(1), "dL/dloc": x.grad, "dL/dvel": v.grad}
    res.update({f"grad {k}": t.grad for k, t in p.items() if t.grad is not None})
    for i in range(len(steps)):
        res[f"loc_preds segment {i + 1}"] = out.detach()[i]
    return res


def test_unrolled_segno_training_on_a_ragged_batch(segno_fx):  # noqa: F811
    # The same inputs (seed 7) and the golden SEGNO weights: checked on the CPU, the float64 loop alone on its own
    # 6-NN lists has the largest |position| at 3.7 and 3.8 in the two segments.
    k, steps = 6, [2, 3]
    n = sum(ROLL)
    loc0, vel0, q = _rollout_inputs()
    target = np.random.RandomState(14).randn(len(steps), n, 3).astype(np.float32)
    m = _segno_train(params_of(segno_fx))
    loc, vel = _dev(loc0).requires_grad_(True), _dev(vel0).requires_grad_(True)
    m.zero_grad(set_to_none=True)
    preds, graphs = harness.segno_rollout_train_graph(m, loc, vel, _dev(q), None, len(steps), steps, k=k,
                                                      return_graphs=True, sizes=ROLL)
    assert preds.shape == (len(steps), n, 3) and preds.grad_fn is not None and len(graphs) == len(steps)
    loss = torch.nn.functional.mse_loss(preds, _dev(target))
    loss.backward()
    torch.cuda.synchronize()
    got_preds = preds.detach().cpu().numpy()
    lists, start = [], loc0
    for i, g in enumerate(graphs):
        if i:
            start = got_preds[i - 1]
        assert g.has_sender_csr()
        _assert_bitwise(g, ragged_neighbor_ref(start, ROLL, k))
        lists.append(tuple(t.cpu().numpy() for t in g.edge_index()))
    r64 = _torch_segno_grads(m, loc0, vel0, q, lists, steps, target, F64)
    r32 = _torch_segno_grads(m, loc0, vel0, q, lists, steps, target, torch.float32)
    got = {"loss": loss.detach().reshape(1), "dL/dloc": loc.grad, "dL/dvel": vel.grad}
    got.update({f"grad {k_}": t.grad for k_, t in m.named_parameters() if t.grad is not None})
    for i in range(len(steps)):
        got[f"loc_preds segment {i + 1}"] = preds.detach()[i]
    _compare("segno ragged train", got, r64, r32)
    graph.sync_checks()


# ---- 12. nothing reads the device -------------------------------------------------------------------------------
def test_ragged_rollout_loops_do_not_synchronise(egno_fx, segno_fx):  # noqa: F811
    k, T = 6, 4
    n = sum(ROLL)
    loc, vel, q = _rollout_inputs()
    me, ms, mt = _egno(egno_fx), _segno(segno_fx), _model(T)
    batch = graph.RaggedBatch(ROLL, DEV)
    a = dict(loc=_dev(loc), vel=_dev(vel), q=_dev(q), t_in=_dev(np.array([0, 3, 5, 0, 2])),
             t_in4=_dev(np.array([0, 3, 1, 0, 2])), target=_dev(_weights(n, 2 * T, 2)[0].reshape(2 * T, n, 3)),
             zero=torch.zeros((), device=DEV))

    def run():
        harness.egno_rollout_graph(me, a["loc"], a["vel"], a["q"], None, None, 2, k=k, r_cut=3.0, timesteps_in=a["t_in"],
                                   energy_dataset="charged", sizes=batch)
        harness.segno_rollout_graph(ms, a["loc"], a["vel"], a["q"], None, 2, [3, 4], k=k, energy_dataset="charged",
                                    sizes=batch)
        mt.zero_grad(set_to_none=True)
        loc_g = a["loc"].clone().requires_grad_(True)
        preds = harness.egno_rollout_train_graph(mt, loc_g, a["vel"], a["q"], None, None, 2, k=k, r_cut=3.0,
                                                 timesteps_in=a["t_in4"], sizes=batch)
        _loss(preds, a["zero"], a["zero"], a["target"], a["zero"], a["zero"], 1.0).backward()

    run()                                   # warm-up: weight packing, allocator
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
