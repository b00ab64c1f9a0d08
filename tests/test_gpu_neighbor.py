"""GPU tests of the neighbour-graph builder (graph.neighbor_graph, csrc/nonode_neighbor.hip), of the
featuriser on an explicit list (harness.prepare_inputs_graph) and of the general-graph rollout drivers
(harness.egno_rollout_graph / segno_rollout_graph).

Builder: bitwise against tests/_neighbor_ref.py (numpy, the builder's float32 arithmetic literally).
Models: a NeighborGraph with [capacity, .] features against its compacted list, torch.equal.
Featuriser: against oracle.harness.prepare_inputs on the returned list, rtol = atol = 1e-6.
Rollouts: every segment's graph bitwise against the numpy reference applied to the positions the segment
started from, and the trajectories against the float64 oracle loop run segment by segment ON THE RETURNED
GRAPHS (so the comparison does not hang on a near-tie between two runs' positions). Bars: 1e-5 (max-norm
relative) on the first segment; on later segments max(1e-5, 4 x the error of the same oracle loop in float32
against float64 on the same graphs), the form of the bar in tests/test_gpu_weight_scales.py with a margin
of 4 because the HIP path's fp16x3 products sit a little above plain fp32 (the float32 oracle's own errors
on the CPU, EGNO setup below: 1.9e-7 / 6.3e-7 / 3.3e-6 for segments 1 / 2 / 3, positions growing from 6 to
155). The figures measured on the MI355X are in profiles/graph/parity_rollout.txt.
"""
import itertools

import numpy as np
import pytest
import torch

import no_node_comparison_amd as pkg
from no_node_comparison_amd import graph, harness
from oracle import egno as oe
from oracle import harness as oh
from oracle import segno as osg
from tests._graph_case import sparse_graph
from tests._neighbor_ref import cutoff_straddlers, d2_contracted, d2_unfused, neighbor_ref, tied_pairs
from tests.conftest import check_rel, load_golden, maxnorm_rel, params_of

pytestmark = pytest.mark.gpu
TOL = 1e-5
MARGIN = 4
DEV = "cuda"


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a)).to(DEV)


def _points(B, N, seed, scale=1.5):
    return (np.random.RandomState(seed).randn(B * N, 3) * scale).astype(np.float32)


def _lattice():
    """The first 37 points of the 4 x 4 x 3 integer lattice, twice."""
    pts = np.array(list(itertools.product(range(4), range(4), range(3))), dtype=np.float32)[:37]
    return np.concatenate([pts, pts])


def _build(x, B, N, k, r_cut=None):
    ng = graph.neighbor_graph(_dev(x), B, N, k, r_cut)
    torch.cuda.synchronize()
    return ng


def _assert_bitwise(ng, ref):
    got = {n: getattr(ng, n).cpu().numpy() for n in ("row_ptr", "col", "rows", "eid")}
    E = int(got["row_ptr"][-1])
    assert ng.capacity == ref["cap"] and E == ref["E"] and int(ng.n_edges.item()) == E
    for n in ("row_ptr", "col", "rows", "eid"):
        assert got[n].dtype == np.int32 and got[n].shape == ref[n].shape, n
        assert np.array_equal(got[n], ref[n]), n
    assert np.all(got["col"][E:] == -1) and np.all(got["rows"][E:] == -1)
    rp, col = got["row_ptr"], got["col"]
    for r in range(len(rp) - 1):
        assert np.all(np.diff(col[rp[r]:rp[r + 1]]) > 0)   # senders ascending within each row
    return E


# ---- 1. the builder ----------------------------------------------------------------------------------
CUT_R = 1.5   # with _points(2, 37, 11): empty rows and rows of degree k (asserted of the reference below)

BUILDER_CASES = [(1, 1, 4, None), (2, 2, 1, None), (3, 37, 6, None), (1, 37, 64, None), (2, 80, 16, None),
                 (1, 130, 64, None), (1, 200, 16, None), (2, 37, 6, CUT_R)]


@pytest.mark.parametrize("B,N,k,r_cut", BUILDER_CASES)
def test_builder_matches_the_numpy_reference_bitwise(B, N, k, r_cut):
    x = _points(B, N, 11)
    ref = neighbor_ref(x, B, N, k, r_cut)
    if r_cut is not None:
        assert (ref["deg"] == 0).any() and (ref["deg"] == k).any() and ref["E"] < ref["cap"]
    if k > N - 1:
        assert np.all(ref["deg"] == N - 1)
    E = _assert_bitwise(_build(x, B, N, k, r_cut), ref)
    if N == 1:
        assert E == 0


@pytest.mark.parametrize("k,r_cut", [(4, 1.0), (3, None)])
def test_builder_on_a_lattice_breaks_ties_by_index(k, r_cut):
    """Many exactly equal distances: with the cut-off degrees 1 to 4 and E = 276; without it, ties at the
    k-th place."""
    x = _lattice()
    ref = neighbor_ref(x, 2, 37, k, r_cut)
    if r_cut is not None:
        assert ref["E"] == 276 and ref["deg"].min() == 1 and ref["deg"].max() == 4
    _assert_bitwise(_build(x, 2, 37, k, r_cut), ref)


def test_builder_with_coincident_nodes():
    x = _points(2, 37, 3)
    x[5] = x[9]
    x[37 + 20] = x[37 + 2]
    ref = neighbor_ref(x, 2, 37, 6)
    assert 9 in ref["col"][ref["row_ptr"][5]:ref["row_ptr"][6]]
    _assert_bitwise(_build(x, 2, 37, 6), ref)


@pytest.mark.parametrize("r_cut", [None, 2.0])
def test_builder_with_a_nan_coordinate(r_cut):
    x = _points(2, 37, 4)
    x[40, 1] = np.nan
    ref = neighbor_ref(x, 2, 37, 6, r_cut)
    assert ref["deg"][40] == 0 and 40 not in ref["col"]
    _assert_bitwise(_build(x, 2, 37, 6, r_cut), ref)


def test_builder_with_large_positions():
    x = _points(2, 37, 6) * np.float32(1e8)
    _assert_bitwise(_build(x, 2, 37, 6), neighbor_ref(x, 2, 37, 6))
    _assert_bitwise(_build(x, 2, 37, 6, 2e8), neighbor_ref(x, 2, 37, 6, 2e8))


def test_builder_and_featuriser_do_not_contract_the_distance():
    """Receivers at the origin (d = -x_j exactly) with senders whose individually rounded d2 tie, or meet
    float32(r_cut)^2, while the contracted d2 (fma(dz, dz, fma(dx, dx, dy dy)), what the compiler emits when
    it may fuse) do not: a build that fuses picks the other sender, or the other side of the cut-off."""
    pairs = tied_pairs(16)
    G = len(pairs)
    x = np.zeros((G, 3, 3), dtype=np.float32)
    for g, (a, b) in enumerate(pairs):
        x[g, 1], x[g, 2] = a, b
        assert d2_unfused(a) == d2_unfused(b) and d2_contracted(b) < d2_contracted(a)
    x = x.reshape(-1, 3)
    ref = neighbor_ref(x, G, 3, 1)
    assert all(ref["col"][ref["row_ptr"][3 * g]] == 3 * g + 1 for g in range(G))   # the tie goes to the lower index
    _assert_bitwise(_build(x, G, 3, 1), ref)
    for pt, r_cut, cand in cutoff_straddlers(2):
        xs = np.stack([np.zeros(3, dtype=np.float32), pt])
        ref = neighbor_ref(xs, 1, 2, 1, r_cut)
        assert ref["E"] == (2 if cand else 0)
        _assert_bitwise(_build(xs, 1, 2, 1, r_cut), ref)
    # the featuriser's distance column, bitwise the individually rounded one
    z = np.zeros((G, 3, 3), dtype=np.float32)
    ea, ng = harness.prepare_inputs_graph(_dev(x.reshape(G, 3, 3)), _dev(z), 3, k=2)[2::3]
    torch.cuda.synchronize()
    rows, col = ng.rows.cpu().numpy(), ng.col.cpu().numpy()
    assert np.array_equal(ea.cpu().numpy()[:, 0], d2_unfused(x[rows] - x[col]))
    assert (d2_unfused(x[rows] - x[col]) != d2_contracted(x[rows] - x[col])).any()


def test_builder_agrees_with_graph_csr_and_repeats_bitwise():
    x = _points(2, 80, 8)
    a, b = _build(x, 2, 80, 16, 2.0), _build(x, 2, 80, 16, 2.0)
    for n in ("row_ptr", "col", "rows", "eid"):
        assert torch.equal(getattr(a, n), getattr(b, n)), n
    E = int(a.n_edges.item())
    assert 0 < E < a.capacity
    rp, col, eid = graph.csr(a.edge_index(), 160)
    graph.sync_checks()
    assert torch.equal(rp, a.row_ptr) and torch.equal(col, a.col[:E]) and torch.equal(eid, a.eid[:E])
    own = graph.csr(a, 160)
    assert own[0] is a.row_ptr and own[1] is a.col and own[2] is a.eid
    assert graph.known_full(a, 160) is None


# ---- 2. the models on a NeighborGraph ------------------------------------------------------------------
@pytest.fixture(scope="module")
def egno_fx():
    return load_golden("egno_fwd")


@pytest.fixture(scope="module")
def segno_fx():
    return load_golden("segno_fwd")


def _egno(fx, T=10, graph="any", **kw):
    m = pkg.EGNO(n_layers=4, in_node_nf=2, in_edge_nf=2, hidden_nf=64, with_v=True, num_modes=2, num_timesteps=T,
                 time_emb_dim=32, device=DEV, graph=graph, **kw)
    m.load_state_dict({k: torch.tensor(v) for k, v in params_of(fx).items()})
    return m.eval()


def _segno(fx, **kw):
    m = pkg.SEGNO(in_node_nf=1, in_edge_nf=2, hidden_nf=64, n_layers=8, recurrent=True, device=DEV, graph="any", **kw)
    m.load_state_dict({k: torch.tensor(v) for k, v in params_of(fx).items()})
    return m.eval()


@pytest.mark.parametrize("mode", ["any", "trainable"])
@pytest.mark.parametrize("r_cut", [None, CUT_R])
def test_models_on_a_neighbor_graph_equal_the_compacted_list(egno_fx, segno_fx, r_cut, mode):
    """mode "trainable": EGNO(graph="trainable") off the tape (SEGNO has "any" only)."""
    B, N, k = 2, 37, 6
    n = B * N
    rs = np.random.RandomState(21)
    x = _dev(_points(B, N, 11))
    v = _dev((rs.randn(n, 3) * 0.3).astype(np.float32))
    h = _dev(rs.randn(n, 2).astype(np.float32))
    ng = graph.neighbor_graph(x, B, N, k, r_cut)
    E = int(ng.n_edges.item())
    assert (E < ng.capacity) == (r_cut is not None)
    ef = _dev(rs.randn(ng.capacity, 2).astype(np.float32))
    ef_nan = ef.clone()
    ef_nan[E:] = float("nan")          # the tail is never read
    lm = x.reshape(B, N, 3).mean(1, keepdim=True).expand(B, N, 3).reshape(n, 3).contiguous()
    me, ms = _egno(egno_fx, graph=mode), _segno(segno_fx)
    with torch.no_grad():
        full = me(x, h, ng, ef_nan, v=v, loc_mean=lm)
        comp = me(x, h, ng.edge_index(), ef[:E].contiguous(), v=v, loc_mean=lm)
        sfull = ms(h[:, :1].contiguous(), x, ng, v, ef_nan, T=5)
        scomp = ms(h[:, :1].contiguous(), x, ng.edge_index(), v, ef[:E].contiguous(), T=5)
    graph.sync_checks()
    for a, b in zip(full + sfull, comp + scomp):
        assert torch.isfinite(a).all() and torch.equal(a, b)


# ---- 3. the featuriser -----------------------------------------------------------------------------------
def _close(got, ref):
    np.testing.assert_allclose(got.cpu().numpy().astype(np.float64), ref, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("frames,r_cut", [(4, None), (1, None), (1, 1.2)])
def test_prepare_inputs_graph_matches_the_oracle_on_its_list(frames, r_cut):
    B, N, k = 3, 7, 3
    rs = np.random.RandomState(31)
    shape = (frames, B, N, 3) if frames > 1 else (B, N, 3)
    loc = rs.randn(*shape).astype(np.float32)
    vel = (rs.randn(*shape) * 0.3).astype(np.float32)
    q = rs.choice([-1.0, 1.0], size=(B, N, 1)).astype(np.float32)
    t_in = np.array([0, 2, 4]) if frames > 1 else None     # frames -1 (the last), 1, 3
    x, v, ea, nodes, lm, ng = harness.prepare_inputs_graph(
        _dev(loc), _dev(vel), N, _dev(q), _dev(t_in) if t_in is not None else None, k=k, r_cut=r_cut)
    torch.cuda.synchronize()
    if frames > 1:
        sel = t_in - 1
        loc_s, vel_s = loc[sel, np.arange(B)], vel[sel, np.arange(B)]
    else:
        loc_s, vel_s = loc, vel
    assert torch.equal(x, _dev(loc_s.reshape(-1, 3))) and torch.equal(v, _dev(vel_s.reshape(-1, 3)))
    _assert_bitwise(ng, neighbor_ref(loc_s.reshape(-1, 3), B, N, k, r_cut))
    E = int(ng.n_edges.item())
    assert ea.shape == (ng.capacity, 2) and (E < ng.capacity) == (r_cut is not None)
    row, col = (t.cpu().numpy() for t in ng.edge_index())
    qf = q.reshape(-1).astype(np.float64)
    eo = (qf[row] * qf[col])[:, None]
    _, _, ea_r, nodes_r, lm_r = oh.prepare_inputs(loc_s.astype(np.float64), vel_s.astype(np.float64), eo, row, col, N,
                                                  q.astype(np.float64))
    _close(ea[:E], ea_r)
    _close(nodes, nodes_r)
    _close(lm, lm_r)
    if r_cut is None:
        assert E == ng.capacity            # (no tail to check)
    else:
        assert not ea[E:].any()            # rows at or past n_edges are zero
    # a fixed list: the same features, one row per entry; without charges the distance alone
    x2, v2, ea2, nodes2, lm2, e2 = harness.prepare_inputs_graph(_dev(loc_s), _dev(vel_s), N, _dev(q), edges=ng)
    assert e2 is ng and torch.equal(ea2, ea) and torch.equal(nodes2, nodes) and torch.equal(lm2, lm)
    plain = ng.edge_index()
    ea3 = harness.prepare_inputs_graph(_dev(loc_s), _dev(vel_s), N, edges=plain)[2]
    assert ea3.shape == (E, 1) and torch.equal(ea3[:, 0], ea[:E, 1])


# ---- 4. the rollouts ---------------------------------------------------------------------------------------
def _rollout_inputs(B, N, seed):
    rs = np.random.RandomState(seed)
    loc = (rs.randn(B, N, 3) * 1.5).astype(np.float32)
    vel = (rs.randn(B, N, 3) * 0.3).astype(np.float32)
    q = rs.choice([-1.0, 1.0], size=(B, N, 1)).astype(np.float32)
    return loc, vel, q


def _edge_lists(graphs):
    torch.cuda.synchronize()
    return [tuple(t.cpu().numpy() for t in (g.edge_index() if isinstance(g, graph.NeighborGraph) else g))
            for g in graphs]


def _oracle_egno(p, loc, vel, q, lists, B, N, T, t_in, t_out, dt):
    """The oracle loop (egno_forward + prepare_inputs + conserved_energy) in dtype dt, segment i on lists[i]."""
    p = {k: v.astype(dt) for k, v in p.items()}
    loc, vel, q = loc.astype(dt), vel.astype(dt), q.astype(dt)
    qf = q.reshape(-1)
    preds, ens = [], []
    fr = np.full(B, -1) if t_in is None else np.asarray(t_in).reshape(-1) - 1
    for i, (row, col) in enumerate(lists):
        eo = (qf[row] * qf[col])[:, None]
        x, v, ea, nodes, lm = oh.prepare_inputs(loc, vel, eo, row, col, N, q)
        t = (t_out[:, i * T:(i + 1) * T] - i * T).astype(dt)
        lo, vo, _ = oe.egno_forward(p, x, nodes, row, col, ea, v, lm, t, T=T)
        assert lo.dtype == dt
        preds.append(lo.reshape(T, B * N, 3))
        la, va = lo.reshape(T, B, N, 3), vo.reshape(T, B, N, 3)
        ens.append(np.stack([oh.conserved_energy("charged", la[j], va[j], q, B) for j in range(T)]))
        loc, vel = la[fr, np.arange(B)], va[fr, np.arange(B)]
    return preds, ens


def _check_segments(tag, got, r64, r32):
    """got, r64, r32: per-segment arrays. Segment 1 at TOL, later ones at max(TOL, MARGIN x the float32
    oracle's own error). Returns the measured (error, float32 oracle error) pairs."""
    out = []
    for i, (g, a, b) in enumerate(zip(got, r64, r32)):
        own = maxnorm_rel(b, a)
        bar = TOL if i == 0 else max(TOL, MARGIN * own)
        err = maxnorm_rel(g, a)
        print(f"{tag} segment {i + 1}: error {err:.3e}  float32 oracle {own:.3e}  bar {bar:.3e}")
        out.append((err, own))
        check_rel(f"{tag} segment {i + 1}", g, a, bar)
    return out


def test_egno_rollout_on_a_rebuilt_knn_graph(egno_fx):
    B, N, k, T, L = 2, 37, 6, 10, 3
    loc, vel, q = _rollout_inputs(B, N, 3)    # (the float64 oracle's positions grow 6 -> 10 -> 162 over the segments)
    t_in = np.array([0, 3])
    m = _egno(egno_fx, T)
    preds, en, en_all, graphs = harness.egno_rollout_graph(
        m, _dev(loc), _dev(vel), _dev(q), N, B, L, k=k, timesteps_in=_dev(t_in), energy_dataset="charged",
        return_graphs=True)
    lists = _edge_lists(graphs)
    preds = preds.cpu().numpy()
    assert preds.shape == (L * T, B * N, 3) and en.shape == (L, B, 1) and en_all.shape == (L * T, B, 1)
    assert len(graphs) == L and np.isfinite(preds).all()
    # every segment's graph is the reference's on the positions it started from
    fr = (t_in - 1) % T
    start = loc.reshape(-1, 3)
    for i, g in enumerate(graphs):
        if i:
            seg = preds[(i - 1) * T:i * T].reshape(T, B, N, 3)
            start = seg[fr, np.arange(B)].reshape(-1, 3)
        _assert_bitwise(g, neighbor_ref(start, B, N, k))
    p = params_of(egno_fx)
    t_out = np.arange(T * L)[None, :]
    p64, e64 = _oracle_egno(p, loc, vel, q, lists, B, N, T, t_in, t_out, np.float64)
    p32, e32 = _oracle_egno(p, loc, vel, q, lists, B, N, T, t_in, t_out, np.float32)
    _check_segments("egno knn loc", [preds[i * T:(i + 1) * T] for i in range(L)], p64, p32)
    ea = en_all.cpu().numpy()[..., 0]
    _check_segments("egno knn energy", [ea[i * T:(i + 1) * T] for i in range(L)], e64, e32)
    assert torch.equal(en, en_all[T - 1::T])


def test_egno_rollout_on_a_fixed_list(egno_fx):
    B, N, T, L = 1, 37, 10, 2
    loc, vel, q = _rollout_inputs(B, N, 43)
    row, col = sparse_graph(N)
    m = _egno(egno_fx, T)
    edges = [_dev(row), _dev(col)]
    preds, en, en_all, graphs = harness.egno_rollout_graph(m, _dev(loc), _dev(vel), _dev(q), N, B, L, edges=edges,
                                                           energy_dataset="charged", return_graphs=True)
    graph.sync_checks()
    assert all(g is edges for g in graphs)
    preds, ea = preds.cpu().numpy(), en_all.cpu().numpy()
    t_out = np.arange(T * L)[None, :]
    refs = []
    for dt in (np.float64, np.float32):
        p = {k: v.astype(dt) for k, v in params_of(egno_fx).items()}
        qd = q.astype(dt)
        eo = (qd.reshape(-1)[row] * qd.reshape(-1)[col])[:, None]
        x, v, ef, nodes, lm = oh.prepare_inputs(loc.astype(dt), vel.astype(dt), eo, row, col, N, qd)
        refs.append(oh.egno_rollout(p, nodes, x, row, col, v, eo, ef, lm, N, L, B, qd, T=T, t_out=t_out.astype(dt)))
    (p64, _, e64), (p32, _, e32) = refs
    seg = lambda a: [a[i * T:(i + 1) * T] for i in range(L)]   # noqa: E731
    _check_segments("egno fixed loc", seg(preds), seg(p64), seg(p32))
    _check_segments("egno fixed energy", seg(ea), seg(e64), seg(e32))


def test_segno_rollout_on_a_rebuilt_knn_graph(segno_fx):
    B, N, k = 2, 37, 6
    steps = [5, 7, 6]
    loc, vel, q = _rollout_inputs(B, N, 47)
    loc, vel = loc.reshape(-1, 3), vel.reshape(-1, 3)
    m = _segno(segno_fx)
    preds, en, graphs = harness.segno_rollout_graph(m, _dev(loc), _dev(vel), _dev(q), B, len(steps), steps, k=k,
                                                    energy_dataset="charged", return_graphs=True)
    lists = _edge_lists(graphs)
    preds, en = preds.cpu().numpy(), en.cpu().numpy()
    assert preds.shape == (len(steps), B * N, 3) and en.shape == (len(steps), B, 1) and np.isfinite(preds).all()
    start = loc
    for i, g in enumerate(graphs):
        if i:
            start = preds[i - 1]
        ref = neighbor_ref(start, B, N, k)
        assert np.all(ref["deg"] == k)      # pure k-NN: every node keeps an incoming edge
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
            lp, ee = oh.segno_rollout(p, his, x, row, col, v, ea, 1, [T], qd, B)
            _, _, v = osg.forward_step(p, oe.linear(his, p, "embedding"), x, row, col, v, ea, T=T)
            x = lp[0]
            assert x.dtype == dt
            ps.append(x)
            es.append(ee[0])
        out[dt] = (ps, es)
    _check_segments("segno knn loc", list(preds), out[np.float64][0], out[np.float32][0])
    _check_segments("segno knn energy", list(en), out[np.float64][1], out[np.float32][1])


def test_rollout_loops_do_not_synchronise(egno_fx, segno_fx):
    B, N, k = 2, 37, 6
    loc, vel, q = _rollout_inputs(B, N, 53)
    me, ms = _egno(egno_fx), _segno(segno_fx)
    a = dict(loc=_dev(loc), vel=_dev(vel), q=_dev(q), t_in=_dev(np.array([0, 3])))

    def run():
        harness.egno_rollout_graph(me, a["loc"], a["vel"], a["q"], N, B, 2, k=k, r_cut=3.0, timesteps_in=a["t_in"],
                                   energy_dataset="charged")
        harness.segno_rollout_graph(ms, a["loc"].reshape(-1, 3), a["vel"].reshape(-1, 3), a["q"], B, 2, [3, 4], k=k,
                                    energy_dataset="charged")

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
