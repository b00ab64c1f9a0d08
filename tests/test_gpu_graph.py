"""GPU tests of the general-graph path (EGNO / SEGNO graph="any"; nonode_graph_build,
nonode_egnn_layer_graph, nonode_egno_forward_graph, nonode_segno_forward_step_graph) against the float64
numpy oracle, which tests/test_graph_golden.py pins to the reference on such a graph.

Metric: check_rel (max-norm relative). Bar: TOL = 1e-5; where inputs are pushed out of the fp16 range,
max(1e-5, 2 x the fp32 restatement's own error) as test_egno_guard_path_matches_oracle does it.
The graphs are those of tests/_graph_case.py (n = 37 and 80: isolated nodes, an in-degree-40 receiver,
a self loop, a duplicate edge, a shuffled list)."""
import numpy as np
import pytest
import torch

import no_node_comparison_amd as pkg
from no_node_comparison_amd import _lib, graph
from oracle import egno as oe
from oracle import harness as oh
from oracle import segno as osg
from oracle import torch_ref as tr
from tests._graph_case import ISOLATED, edge_features, egno_case, segno_case, sparse_graph
from tests.conftest import check_rel, load_golden, maxnorm_rel, params_of

pytestmark = pytest.mark.gpu
TOL = 1e-5
DEV = "cuda"
P = _lib.ptr


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a)).to(DEV)


def _sd_np(model):
    return {k: v.detach().cpu().numpy().astype(np.float64) for k, v in model.state_dict().items()}


def _f64(case, keep=("row", "col", "t_out", "t_in")):
    return {k: (v.astype(np.float64) if k not in keep else v) for k, v in case.items()}


def _egno(sd=None, seed=0, T=10, **kw):
    torch.manual_seed(seed)
    m = pkg.EGNO(n_layers=4, in_node_nf=2, in_edge_nf=2, hidden_nf=64, with_v=True, num_modes=2, num_timesteps=T,
                 time_emb_dim=32, device=DEV, **kw)
    if sd is not None:
        m.load_state_dict({k: torch.tensor(v) for k, v in sd.items()})
    return m.eval()


def _segno(sd=None, seed=0, **kw):
    torch.manual_seed(seed)
    m = pkg.SEGNO(in_node_nf=1, in_edge_nf=2, hidden_nf=64, n_layers=8, recurrent=True, device=DEV, **kw)
    if sd is not None:
        m.load_state_dict({k: torch.tensor(v) for k, v in sd.items()})
    return m.eval()


@pytest.fixture(scope="module")
def egno_fx():
    return load_golden("egno_fwd")


@pytest.fixture(scope="module")
def segno_fx():
    return load_golden("segno_fwd")


def _run_egno(m, c, multi=False):
    kw = dict(v=_dev(c["v"]), loc_mean=_dev(c["loc_mean"]), timesteps_out=_dev(c["t_out"]))
    if multi:
        kw["timesteps_in"] = _dev(c["t_in"])
    with torch.no_grad():
        out = m(_dev(c["x"]), _dev(c["h"]), [_dev(c["row"]), _dev(c["col"])], _dev(c["edge_fea"]), **kw)
    torch.cuda.synchronize()
    return [o.cpu() for o in out]


def _run_segno(m, c, T):
    with torch.no_grad():
        out = m(_dev(c["his"]), _dev(c["x"]), [_dev(c["row"]), _dev(c["col"])], _dev(c["v"]), _dev(c["edge_attr"]), T=T)
    torch.cuda.synchronize()
    return [o.cpu() for o in out]   # (x, h, v)


# ---- 1. the CSR ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
def test_csr_is_the_lexsort_of_the_list(dtype):
    n = 37
    row, col = sparse_graph(n)
    order = np.lexsort((np.arange(len(row)), col, row))
    want_ptr = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=n))])
    builds = []
    for _ in range(2):
        graph._csr.clear()
        rp, cc, ee = graph.csr([_dev(row).to(dtype), _dev(col).to(dtype)], n)
        builds.append([t.cpu().numpy() for t in (rp, cc, ee)])
    graph.sync_checks()
    for rp, cc, ee in builds:
        assert rp.dtype == np.int32 and np.array_equal(rp, want_ptr)
        assert np.array_equal(cc, col[order]) and np.array_equal(ee, order)


def test_csr_of_an_empty_list():
    e = torch.empty(0, dtype=torch.int64, device=DEV)
    rp, cc, ee = graph.csr([e, e.clone()], 37)
    assert rp.shape == (38,) and int(rp.abs().max()) == 0 and cc.numel() == 0 and ee.numel() == 0
    graph.sync_checks()


# ---- 2. the layer entry ----------------------------------------------------------------------------
def _layer_inputs(n, n_frames, ef_frames, seed):
    rng = np.random.RandomState(seed)
    row, col = sparse_graph(n)
    E = len(row)
    nt = n_frames * n
    h = (rng.randn(nt, 64) * 0.5).astype(np.float32)
    x = rng.randn(nt, 3).astype(np.float32) * 1.5
    v = rng.randn(nt, 3).astype(np.float32) * 0.5
    ef = np.stack([edge_features(E, 2, seed + f) for f in range(ef_frames)])          # [ef_frames, E, 2]
    off = (np.arange(n_frames) * n).repeat(E)
    row_t, col_t = np.tile(row, n_frames) + off, np.tile(col, n_frames) + off
    ef_t = np.concatenate([ef[f % ef_frames] for f in range(n_frames)])
    return row, col, h, x, v, ef, row_t, col_t, ef_t


def _layer_graph(variant, blob, n_frames, n, row, col, h, x, v, ef, dt=0.0, cw=1.0, recurrent=0):
    L = pkg.lib()
    rp, cc, ee = graph.csr([_dev(row), _dev(col)], n)
    dh, dx, dv, de = _dev(h), _dev(x), _dev(v), _dev(ef)
    ho, xo, vo = torch.empty_like(dh), torch.empty_like(dx), torch.empty_like(dv)
    ws_bytes = L.nonode_egnn_layer_graph_workspace_bytes(n_frames, n)
    ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.float32, device=DEV)
    _lib.check(L.nonode_egnn_layer_graph(variant, n_frames, n, len(row), ef.shape[-1], ef.shape[0], P(dh), P(dx), P(dv),
                                         P(de), P(blob), P(rp), P(cc), P(ee), dt, cw, recurrent, P(ho), P(xo), P(vo),
                                         P(ws), ws_bytes, _lib.stream_of(dh)))
    torch.cuda.synchronize()
    return ho.cpu().numpy(), xo.cpu().numpy(), vo.cpu().numpy()


@pytest.mark.parametrize("n", [37, 80])
@pytest.mark.parametrize("n_frames", [1, 3])
def test_egno_layer_graph_matches_oracle(egno_fx, n, n_frames):
    m = _egno(params_of(egno_fx))
    row, col, h, x, v, ef, row_t, col_t, ef_t = _layer_inputs(n, n_frames, n_frames, seed=n + n_frames)
    blobs, _ = m._packed()
    ho, xo, _ = _layer_graph(_lib.VARIANT_EGNO, blobs[1], n_frames, n, row, col, h, x, v, ef)
    p = _sd_np(m)
    f = lambda a: a.astype(np.float64)  # noqa: E731
    xr, _, hr = oe.egnn_layer(p, "layers.1", f(x), f(h), row_t, col_t, f(ef_t), f(v))
    check_rel("x", xo, xr, TOL)
    check_rel("h", ho, hr, TOL)
    # the isolated nodes on their own: no force term, x = x + phi_v(h) v
    iso = np.array([fr * n + i for fr in range(n_frames) for i in ISOLATED])
    x_iso = f(x)[iso] + oe.base_mlp(f(h)[iso], p, "layers.1.node_v_net") * f(v)[iso]
    check_rel("isolated x", xo[iso], x_iso, TOL)


@pytest.mark.parametrize("n", [37, 80])
@pytest.mark.parametrize("n_frames", [1, 3])
def test_segno_layer_graph_matches_oracle(segno_fx, n, n_frames):
    m = _segno(params_of(segno_fx))
    row, col, h, x, v, ef, row_t, col_t, ef_t = _layer_inputs(n, n_frames, 1, seed=2 * n + n_frames)
    T = 4
    ho, xo, vo = _layer_graph(_lib.VARIANT_SEGNO, m._packed(), n_frames, n, row, col, h, x, v, ef, dt=1.0 / T,
                              recurrent=1)
    f = lambda a: a.astype(np.float64)  # noqa: E731
    hr, xr, vr = osg.gcl_forward(_sd_np(m), f(h), row_t, col_t, f(x), f(v), f(ef_t), n_layers=T)
    check_rel("x", xo, xr, TOL)
    check_rel("v", vo, vr, TOL)
    check_rel("h", ho, hr, TOL)
    iso = np.array([fr * n + i for fr in range(n_frames) for i in ISOLATED])
    assert np.array_equal(vo[iso], v[iso])   # no incoming edge: v unchanged, bit for bit


# ---- 3. whole models --------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [37, 80])
def test_egno_any_matches_oracle(egno_fx, n):
    m = _egno(params_of(egno_fx), graph="any")
    c = egno_case(egno_fx, n)
    x, v, h = _run_egno(m, c)
    xr, vr, hr = oe.egno_forward(_sd_np(m), **_f64(c), T=10)
    check_rel("x", x, xr, TOL)
    check_rel("v", v, vr, TOL)
    check_rel("h", h, hr, TOL)
    graph.sync_checks()


def test_egno_any_multi_input_matches_oracle(egno_fx):
    n, I = 37, 3
    m = _egno(seed=11, graph="any", num_inputs=I)
    c = egno_case(egno_fx, n)
    rng = np.random.RandomState(5)
    E = len(c["row"])
    stack = lambda a, s: np.stack([a + s * rng.randn(*a.shape).astype(np.float32) for _ in range(I)])  # noqa: E731
    c.update(x=stack(c["x"], 0.05), h=stack(c["h"], 0.05), v=stack(c["v"], 0.05), loc_mean=stack(c["loc_mean"], 0.0),
             edge_fea=np.stack([edge_features(E, 2, 20 + i) for i in range(I)]),
             t_in=np.arange(-I + 1, 1)[None].astype(np.int64))
    x, v, h = _run_egno(m, c, multi=True)
    xr, vr, hr = oe.egno_forward_multi(_sd_np(m), **_f64(c), T=10)
    check_rel("x", x, xr, TOL)
    check_rel("v", v, vr, TOL)
    check_rel("h", h, hr, TOL)


@pytest.mark.parametrize("opts", [dict(norm=True), dict(use_time_conv=False)], ids=["norm", "no_time_conv"])
def test_egno_any_options_match_oracle(egno_fx, opts):
    m = _egno(seed=12, graph="any", **opts)
    c = egno_case(egno_fx, 37)
    x, v, h = _run_egno(m, c)
    xr, vr, hr = oe.egno_forward(_sd_np(m), **_f64(c), T=10, **opts)
    check_rel("x", x, xr, TOL)
    check_rel("v", v, vr, TOL)
    check_rel("h", h, hr, TOL)


@pytest.mark.parametrize("n", [37, 80])
def test_segno_any_matches_oracle(segno_fx, n):
    m = _segno(params_of(segno_fx), graph="any")
    c = segno_case(segno_fx, n)
    x, h, v = _run_segno(m, c, 10)
    xr, hr, vr = osg.forward(_sd_np(m), **_f64(c), T=10, bug_compat=False)
    check_rel("x", x, xr, TOL)
    check_rel("v", v, vr, TOL)
    check_rel("h", h, hr, TOL)


def test_segno_any_tanh_matches_oracle(segno_fx):
    m = _segno(seed=13, graph="any", tanh=True)
    c = segno_case(segno_fx, 37)
    x, h, v = _run_segno(m, c, 10)
    xr, hr, vr = osg.forward(_sd_np(m), **_f64(c), T=10, bug_compat=False, tanh=True)
    check_rel("x", x, xr, TOL)
    check_rel("v", v, vr, TOL)
    check_rel("h", h, hr, TOL)


def test_segno_any_keeps_bug_compat(segno_fx):
    m = _segno(params_of(segno_fx), graph="any", bug_compat=True)
    c = segno_case(segno_fx, 37)
    xi, vi = _dev(c["x"]), _dev(c["v"])
    with torch.no_grad():
        x, h, v = m(_dev(c["his"]), xi, [_dev(c["row"]), _dev(c["col"])], vi, _dev(c["edge_attr"]), T=10)
    assert x is xi and v is vi


# ---- 4. the range guard -----------------------------------------------------------------------------
def test_egno_any_guard_path_matches_oracle(egno_fx):
    """Edge features x 1e6: the first layer's edge-feature pre-activation leaves the fp16 range, so the
    64x64 products of those tiles take mm64's exact f32 path."""
    m = _egno(params_of(egno_fx), graph="any")
    c = egno_case(egno_fx, 37)
    c["edge_fea"] = (c["edge_fea"] * 1e6).astype(np.float32)
    p = _sd_np(m)
    w1 = p["layers.0.edge_message_net.scalar_net.mlp.0.weight"][:, -2:]
    assert float(np.abs(c["edge_fea"].astype(np.float64) @ w1.T).max()) > 2 * 65504.0
    xr, vr, hr = oe.egno_forward(p, **_f64(c), T=10)
    assert np.isfinite(xr).all() and np.isfinite(vr).all() and np.isfinite(hr).all()
    p32 = {k: torch.tensor(v, dtype=torch.float32) for k, v in p.items()}
    t = lambda a: torch.tensor(np.ascontiguousarray(a))  # noqa: E731
    with torch.no_grad():
        f32 = tr.egno_forward(p32, t(c["x"]).float(), t(c["h"]).float(), t(c["row"]).long(), t(c["col"]).long(),
                              t(c["edge_fea"]).float(), t(c["v"]).float(), t(c["loc_mean"]).float(),
                              t(c["t_out"]).float(), T=10)
    x, v, h = _run_egno(m, c)
    for name, out, f, ref in (("x", x, f32[0], xr), ("v", v, f32[1], vr), ("h", h, f32[2], hr)):
        check_rel(f"guard {name}", out, ref, max(TOL, 2 * maxnorm_rel(f.numpy(), ref)))


def test_segno_any_guard_path_matches_oracle(segno_fx):
    """Positions x 300 (|r|^2 enters as the radial input and as an edge attribute), T = 4."""
    T = 4
    m = _segno(params_of(segno_fx), graph="any")
    c = segno_case(segno_fx, 37)
    x = c["x"].astype(np.float64) * 300.0
    d2 = ((x[c["row"]] - x[c["col"]]) ** 2).sum(1)
    assert float(d2.max()) > 65504.0
    c["x"] = x.astype(np.float32)
    x = c["x"].astype(np.float64)
    c["edge_attr"] = np.stack([c["edge_attr"][:, 0], ((x[c["row"]] - x[c["col"]]) ** 2).sum(1)], 1).astype(np.float32)
    p = _sd_np(m)
    xr, hr, vr = osg.forward(p, **_f64(c), T=T, bug_compat=False)
    assert np.isfinite(xr).all() and np.isfinite(hr).all()
    p32 = {k: torch.tensor(v, dtype=torch.float32) for k, v in p.items()}
    t = lambda a: torch.tensor(np.ascontiguousarray(a))  # noqa: E731
    with torch.no_grad():
        f32 = tr.segno_forward_step(p32, t(c["his"]).float(), t(c["x"]).float(), t(c["row"]).long(), t(c["col"]).long(),
                                    t(c["v"]).float(), t(c["edge_attr"]).float(), T=T, dense_mean=False)
    xo, ho, vo = _run_segno(m, c, T)
    for name, out, f, ref in (("x", xo, f32[0], xr), ("h", ho, f32[1], hr), ("v", vo, f32[2], vr)):
        check_rel(f"guard {name}", out, ref, max(TOL, 2 * maxnorm_rel(f.numpy(), ref)))


# ---- 5. determinism and list order ---------------------------------------------------------------------
def _permuted(c, key, seed=3):
    perm = np.random.RandomState(seed).permutation(len(c["row"]))
    d = dict(c)
    d.update(row=c["row"][perm], col=c["col"][perm])
    d[key] = c[key][perm]
    return d


@pytest.mark.parametrize("n", [37, 80])
def test_egno_any_is_bitwise_reproducible_and_list_order_free(egno_fx, n):
    m = _egno(params_of(egno_fx), graph="any")
    c = egno_case(egno_fx, n)
    a, b = _run_egno(m, c), _run_egno(m, c)
    assert all(torch.equal(s, t) for s, t in zip(a, b))
    # without duplicate edges the CSR, and with it every sum order, does not depend on the list order
    s = egno_case(egno_fx, n, simple=True)
    a, b = _run_egno(m, s), _run_egno(m, _permuted(s, "edge_fea"))
    assert all(torch.equal(s_, t_) for s_, t_ in zip(a, b))


@pytest.mark.parametrize("n", [37, 80])
def test_segno_any_is_bitwise_reproducible_and_list_order_free(segno_fx, n):
    m = _segno(params_of(segno_fx), graph="any")
    c = segno_case(segno_fx, n)
    a, b = _run_segno(m, c, 10), _run_segno(m, c, 10)
    assert all(torch.equal(s, t) for s, t in zip(a, b))
    s = segno_case(segno_fx, n, simple=True)
    a, b = _run_segno(m, s, 10), _run_segno(m, _permuted(s, "edge_attr"), 10)
    assert all(torch.equal(s_, t_) for s_, t_ in zip(a, b))


# ---- 6. beyond the fused path's reach ----------------------------------------------------------------
def test_layer_graph_runs_n500_where_the_fused_layer_cannot(egno_fx):
    """One EGNO layer on one fully connected graph of N = 500 (E = 249,500) passed as a list. The fused
    entry refuses it: its LDS sender table would need 12,288 + 72 x 500 floats of a 40,704-float budget."""
    N = 500
    m = _egno(params_of(egno_fx))
    rng = np.random.RandomState(500)
    row, col = oh.full_edges(1, N)
    sigma = (N / 5.0) ** (1.0 / 3.0)
    x = (rng.randn(N, 3) * sigma).astype(np.float32)
    v = (rng.randn(N, 3) * 0.5).astype(np.float32)
    h = (rng.randn(N, 64) * 0.5).astype(np.float32)
    q = rng.randint(0, 2, N) * 2.0 - 1.0
    ef = np.stack([q[row] * q[col], ((x[row].astype(np.float64) - x[col]) ** 2).sum(1)], 1).astype(np.float32)
    blobs, _ = m._packed()
    ho, xo, _ = _layer_graph(_lib.VARIANT_EGNO, blobs[0], 1, N, row, col, h, x, v, ef[None])
    f = lambda a: a.astype(np.float64)  # noqa: E731
    xr, _, hr = oe.egnn_layer(_sd_np(m), "layers.0", f(x), f(h), row, col, f(ef), f(v))
    check_rel("x", xo, xr, TOL)
    check_rel("h", ho, hr, TOL)
    dh, dx, dv, de = _dev(h), _dev(x), _dev(v), _dev(ef)
    h2, x2 = torch.empty_like(dh), torch.empty_like(dx)
    rc = pkg.lib().nonode_egnn_layer(_lib.VARIANT_EGNO, 1, N, 2, 1, P(dh), P(dx), P(dv), P(de), P(blobs[0]), 0.0, 1.0, 0,
                                     P(h2), P(x2), None, _lib.stream_of(dh))
    assert rc == 3   # NONODE_EUNSUPPORTED


# ---- 7. the full graph both ways ----------------------------------------------------------------------
def test_full_graph_through_both_paths(egno_fx):
    from tests.test_gpu_parity import _egno_case
    B, N, T = 3, 20, 10
    c = _egno_case(B, N, T, seed=21)
    sd = params_of(egno_fx)
    xr, vr, hr = oe.egno_forward({k: v.astype(np.float64) for k, v in sd.items()}, **_f64(c), T=T)
    n_csr = len(graph._csr)
    any_out = _run_egno(_egno(sd, graph="any"), c)       # a never-seen copy of the list: the general path
    assert len(graph._csr) == min(n_csr + 1, graph._CACHE)
    full_out = _run_egno(_egno(sd), c)
    for out in (any_out, full_out):   # (no bitwise claim between the two: their sum orders differ)
        check_rel("x", out[0], xr, TOL)
        check_rel("v", out[1], vr, TOL)
        check_rel("h", out[2], hr, TOL)
    graph.sync_checks()


# ---- 8. an invalid device list ------------------------------------------------------------------------
@pytest.mark.parametrize("bad", ["n_nodes", -1])
def test_invalid_device_list_poisons_and_raises(egno_fx, bad):
    """One index out of range on the device. nonode_graph_build range-checks every index, sets the flag
    and DROPS that edge from the CSR, and the layer kernels read senders only from the CSR: this test
    touches no out-of-range address by construction. The outputs are NaN-filled behind the flag and the
    error surfaces at the next boundary call."""
    n = 37
    graph.sync_checks()
    m = _egno(params_of(egno_fx), graph="any")
    c = egno_case(egno_fx, n)
    good = _run_egno(m, c)
    assert all(bool(torch.isfinite(o).all()) for o in good)
    b = dict(c)
    b["col"] = c["col"].copy()
    b["col"][11] = n if bad == "n_nodes" else -1
    out = _run_egno(m, b)
    assert all(bool(torch.isnan(o).all()) for o in out)
    with pytest.raises(ValueError, match="outside"):
        graph.sync_checks()
    again = _run_egno(m, c)
    assert all(bool(torch.isfinite(o).all()) for o in again)
    graph.sync_checks()


# ---- 9. a known-full list keeps the fused path ---------------------------------------------------------
def test_any_takes_the_fused_path_for_a_known_full_list(egno_fx):
    from tests.test_gpu_parity import _egno_case
    B, N, T = 3, 20, 10
    c = _egno_case(B, N, T, seed=22)
    sd = params_of(egno_fx)
    edges = pkg.harness.get_edges(B, N, DEV)
    outs = []
    for m in (_egno(sd, graph="any"), _egno(sd)):
        n_csr = len(graph._csr)
        with torch.no_grad():
            outs.append(m(_dev(c["x"]), _dev(c["h"]), edges, _dev(c["edge_fea"]), v=_dev(c["v"]),
                          loc_mean=_dev(c["loc_mean"]), timesteps_out=_dev(c["t_out"])))
        assert len(graph._csr) == n_csr
    assert all(torch.equal(a, b) for a, b in zip(*outs))
