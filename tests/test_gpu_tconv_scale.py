"""TimeConv forward and reverse on the GPU at the spectral term's own scale (tests/_tconv_ref.py): the
TimeConv weights are multiplied by an exact power of two that makes max|y| ~ max|h|, so the fixed 1e-5 bar on
h_out = h + LeakyReLU(y) and on g_h_in = g_out + adjoint term is a 1e-5 bar on y and on the adjoint term
(at the shipped weights both are ~1e-3 of what they are added to, and an error of ~0.7 % in them passes every
other test). The packed fp16 hi / lo fragments are bit-identical to those of the shipped weights.

Through the C ABI (nonode_pack_tconv, nonode_egno_tconv, nonode_egno_tconv_bwd) against float64, for every
compiled instance and every form of the kernels (sizes from the device's CU count, _tconv_ref.bn_sizes), and
through the whole model (first-layer kernel with the embedding fused, per-frame variant, the training forward's
mask words feeding nonode_egno_backward) with every TimeConv's weights x 2^9. Every instance is also launched
8 times on the same inputs at the C2 / C4 size and must repeat bitwise (see the comment above LAUNCHES).

Measured on an MI355X (256 CUs), worst metric per group, bar 1e-5: see profiles/tconv_scale/measured.txt.
"""
import os

import pytest
import torch

import no_node_comparison_amd as pkg
from no_node_comparison_amd import _lib
from oracle import torch_ref as tr
from tests import _tconv_ref as R
from tests.conftest import _PARITY, check_rel, maxnorm_rel
from tests.test_gpu_input_grads import _frames_ref
from tests.test_gpu_input_grads import _model as _model_inputs
from tests.test_gpu_parity import DEV, _egno, _egno_full
from tests.test_gpu_train import _hip_lrelu_masks, _loss_like_reference

pytestmark = pytest.mark.gpu


def _bn(name):
    return R.bn_sizes(torch.cuda.get_device_properties(0).multi_processor_count)[name]


def _check(name, got, ref, scale, bar=R.BAR):
    """Print, record (the parity report of tests/conftest.py) and assert rel(got, ref, scale) < bar."""
    assert bool(torch.isfinite(got).all()), name
    err = R.rel(got, ref, scale)
    test = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0]
    print(f"{name}: {err:.3e} (bar {bar:.0e})")
    _PARITY.append({"test": test, "quantity": name, "maxnorm_rel": err, "bar": float(bar)})
    assert err < bar, (name, err, bar)


def _nan_like(t):
    return torch.full_like(t, float("nan"))


def _dev_case(c, tw, gout_h=None):
    """Device copies in the C ABI's layout ([T * BN] rows) and the packed TimeConv blob of weights tw."""
    T, modes, BN = c["T"], c["modes"], c["BN"]
    L = pkg.lib()
    d = {k: c[k].reshape(T * BN, -1).to(DEV).contiguous() for k in ("h", "x", "v", "gout_x", "gout_v")}
    d["gout_h"] = (c["gout_h"] if gout_h is None else gout_h).reshape(T * BN, 64).to(DEV).contiguous()
    d["loc_mean"], d["tw"], d["txw"] = (a.to(DEV).contiguous() for a in (c["loc_mean"], tw, c["txw"]))
    d["blob"] = torch.empty(L.nonode_tconv_blob_floats(modes), dtype=torch.float32, device=DEV)
    _lib.check(L.nonode_pack_tconv(_lib.ptr(d["tw"]), modes, T, _lib.ptr(d["blob"]), _lib.stream_of(d["blob"])))
    return d


def _forward(c, d):
    L, P = pkg.lib(), _lib.ptr
    ho, xo, vo = _nan_like(d["h"]), _nan_like(d["x"]), _nan_like(d["v"])
    _lib.check(L.nonode_egno_tconv(c["BN"], c["T"], c["modes"], P(d["h"]), P(d["x"]), P(d["v"]), P(d["loc_mean"]),
                                   P(d["blob"]), P(d["txw"]), P(ho), P(xo), P(vo), _lib.stream_of(ho)))
    torch.cuda.synchronize()
    return ho.cpu(), xo.cpu(), vo.cpu()


def _amplified_case(T, modes, BN):
    c = R.case(T, modes, BN, seed=R.seed_of(T, modes, BN))
    return c, R.amplify(c["h"], c["tw"])[0]


FWD = ([(T, m, "small") for T, m in R.FWD_SMALL] + [(T, m, "xcd") for T, m in R.FWD_INSTANCES]
       + [(T, m, "four") for T, m in R.FWD_INSTANCES])


@pytest.mark.parametrize("T,modes,size", FWD)
def test_tconv_forward_at_spectral_scale(T, modes, size):
    c, tw = _amplified_case(T, modes, _bn(size))
    r = R.reference(c, tw, reverse=False)
    assert 0.5 <= float(r["y"].abs().max()) / float(c["h"].abs().max()) <= 2
    ho, xo, vo = _forward(c, _dev_case(c, tw))
    for name, got in (("h_out", ho), ("x_out", xo), ("v_out", vo)):
        _check(f"fwd T={T} modes={modes} {size} {name}", got, r[name], R.scale_of(r, name))


@pytest.mark.parametrize("T,modes", [(10, 2), (16, 2)])
def test_tconv_forward_f32_fallback_tile(T, modes):
    """The h of columns 16..31 x 8192: this tile's spectrum passes H16_LIMIT and takes the f32 mixing, tiles 0
    and 2 of the same launch stay on fp16x3. The scaled tile and the rest are compared separately, each
    against its own max|LeakyReLU(y_ref)|."""
    c, tw = _amplified_case(T, modes, _bn("small"))
    c["h"][:, 16:32] *= 8192
    r = R.reference(c, tw, reverse=False)
    ho, xo, vo = _forward(c, _dev_case(c, tw))
    lr = torch.nn.functional.leaky_relu(r["y"], R.SLOPE)
    big = torch.zeros(c["BN"], dtype=torch.bool)
    big[16:32] = True
    assert float(lr[:, big].abs().max()) > 1000 * float(lr[:, ~big].abs().max())
    ho = ho.reshape(T, c["BN"], 64)
    for tag, sel in (("f32 tile", big), ("fp16x3 tiles", ~big)):
        _check(f"fallback T={T} {tag} h_out", ho[:, sel], r["h_out"][:, sel], float(lr[:, sel].abs().max()))
    _check(f"fallback T={T} x_out", xo, r["x_out"], R.scale_of(r, "x_out"))
    _check(f"fallback T={T} v_out", vo, r["v_out"], R.scale_of(r, "v_out"))


GRADS = ("g_h_in", "g_x_in", "g_v_in", "g_tw", "g_txw")


def _reverse(c, d, ws):
    L, P = pkg.lib(), _lib.ptr
    out = {"g_h_in": _nan_like(d["h"]), "g_x_in": _nan_like(d["x"]), "g_v_in": _nan_like(d["v"]),
           "g_tw": _nan_like(d["tw"]), "g_txw": _nan_like(d["txw"])}
    _lib.check(L.nonode_egno_tconv_bwd(c["BN"], c["T"], c["modes"], P(d["h"]), P(d["x"]), P(d["v"]), P(d["loc_mean"]),
                                       P(d["blob"]), P(d["tw"]), P(d["txw"]), P(d["gout_h"]), P(d["gout_x"]),
                                       P(d["gout_v"]), *(P(out[k]) for k in GRADS), P(ws), ws.numel() * 4,
                                       _lib.stream_of(ws)))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("T,modes,size", R.REV_CASES)
def test_tconv_reverse_at_spectral_scale(T, modes, size):
    """Amplified TimeConv weights and an output gradient that is exactly 0 where |y_ref| < 1e-4 max|y_ref|
    (the kernel's LeakyReLU decision is irrelevant there; every element is compared). g_h_in is measured against
    the adjoint term alone. The workspace starts as NaN, and a second call on the used workspace must give
    bitwise the same outputs (the LDS accumulator hand-off and the block-order reductions are deterministic)."""
    BN = _bn(size)
    c, tw = _amplified_case(T, modes, BN)
    r = R.reference(c, tw)
    assert r["zeroed"] <= R.MAX_ZEROED
    d = _dev_case(c, tw, gout_h=r["gout_h"])
    ws_bytes = pkg.lib().nonode_egno_tconv_bwd_workspace_bytes(BN, T, modes)
    ws = torch.full(((ws_bytes + 3) // 4,), float("nan"), dtype=torch.float32, device=DEV)
    out = _reverse(c, d, ws)
    for k in GRADS:
        _check(f"rev T={T} modes={modes} {size} {k}", out[k].cpu(), r[k], R.scale_of(r, k))
    M = min(modes, T // 2 + 1)
    if modes > M:   # the rfft has no bins >= M: exactly 0 in both weight gradients (indexed by the full mode count)
        assert float(out["g_tw"][:, :, M:].abs().max()) == 0 and float(out["g_txw"][:, :, M:].abs().max()) == 0
    again = _reverse(c, d, ws)
    for k in GRADS:
        assert torch.equal(out[k], again[k]), k


# ---- the same launch again and again at the C2 / C4 size ------------------------------------------------------
# With the fp16x3 mixing compiled into the 4-mode builds (guard `MM > 2` in tconv_kernel widened to `MM > 4`),
# about half of the launches at this size put one channel of one 16-column tile 10-20 % of max|y| off, another
# tile each time, and the rest of the launches are right: a single launch at a few hundred tiles mostly passes.
# So every compiled instance is launched LAUNCHES times on the same inputs at 640 tiles (two or three workgroups
# per CU at once): the first result is held to the bar, the others must equal it bitwise.
LAUNCHES = 8


@pytest.mark.parametrize("T,modes", R.FWD_INSTANCES)
def test_tconv_forward_repeats_bitwise_at_c2_size(T, modes):
    c, tw = _amplified_case(T, modes, _bn("c2"))
    r = R.reference(c, tw, reverse=False)
    d = _dev_case(c, tw)
    first = _forward(c, d)
    for name, got in zip(("h_out", "x_out", "v_out"), first):
        _check(f"fwd T={T} modes={modes} c2 {name}", got, r[name], R.scale_of(r, name))
    for i in range(1, LAUNCHES):
        for name, a, b in zip(("h_out", "x_out", "v_out"), first, _forward(c, d)):
            assert torch.equal(a, b), (name, i, R.rel(b, a.double(), R.scale_of(r, name)))


@pytest.mark.parametrize("T,modes", R.FWD_INSTANCES)
def test_tconv_reverse_repeats_bitwise_at_c4_size(T, modes):
    """nonode_egno_tconv_bwd (its forward recompute of the LeakyReLU decisions, tconvx_bwd_kernel,
    tconv_bwd_kernel over two or three trips, tconv_wgrad_reduce) LAUNCHES times on one workspace; the accuracy of
    these instances is test_tconv_reverse_at_spectral_scale's."""
    BN = _bn("c2")
    c, tw = _amplified_case(T, modes, BN)
    d = _dev_case(c, tw)
    ws_bytes = pkg.lib().nonode_egno_tconv_bwd_workspace_bytes(BN, T, modes)
    ws = torch.full(((ws_bytes + 3) // 4,), float("nan"), dtype=torch.float32, device=DEV)
    first = _reverse(c, d, ws)
    for k in GRADS:
        assert bool(torch.isfinite(first[k]).all()), k
    for i in range(1, LAUNCHES):
        again = _reverse(c, d, ws)
        for k in GRADS:
            assert torch.equal(first[k], again[k]), (k, i)


# ---- the whole model with every TimeConv's weights x 2^9 ----------------------------------------------------
def _amplify_model(m, k=9):
    with torch.no_grad():
        for mod in m.time_conv_modules:
            mod.t_conv.weights1.mul_(2.0 ** k)
    return m


def _flips_lie_at_the_kink(masks, ys):
    for layer, (mk, y) in enumerate(zip(masks, ys)):
        flip = mk != (y > 0)
        assert int(flip.sum()) <= 64, (layer, int(flip.sum()))
        if flip.any():
            assert float(y[flip].abs().max()) <= 1e-5 * float(y.abs().max()), layer


@pytest.mark.parametrize("B,N", [(3, 7), (52, 20)])
@pytest.mark.parametrize("T,modes", [(10, 2), (8, 5), (16, 9)])
def test_egno_amplified_tconv_forward_and_gradients(T, modes, B, N):
    """Inference forward (first TimeConv with the embedding fused) and one training step (the training
    forward's mask words into nonode_egno_backward) against float64 torch autograd of oracle/torch_ref.py at
    the HIP forward's own LeakyReLU decisions. Bar as tests/test_gpu_weight_scales.py: 1e-5, or twice the
    error of the same restatement in fp32 where that is larger (four amplified layers grow h about tenfold;
    the fp32 conditioning of the later layers is the reference's own)."""
    m = _amplify_model(_egno(T=T, modes=modes, seed=100 * T + modes))
    x, nodes, edges, ea, v, lm, t, _ = _egno_full(B, N, T, seed=B + N)
    loc_true = torch.randn(B, N, T, 3, generator=torch.Generator().manual_seed(T))
    with torch.no_grad():
        inf = m(x, nodes, edges, ea, v=v, loc_mean=lm, timesteps_out=t)
    m.train()
    m.zero_grad(set_to_none=True)
    m._train_state_sink = []
    out = m(x, nodes, edges, ea, v=v, loc_mean=lm, timesteps_out=t)
    masks = _hip_lrelu_masks(m._train_state_sink.pop(), m.n_layers, T, B * N)
    del m._train_state_sink
    loss, _ = _loss_like_reference(out[0], loc_true.to(DEV), T, B, N)
    loss.backward()
    torch.cuda.synchronize()
    r, c = tr.full_edges(B, N)
    sd = m.state_dict()

    def torch_run(dt, **kw):
        p = {k: q.detach().cpu().to(dt).requires_grad_(True) for k, q in sd.items()}
        d = lambda a: a.detach().cpu().to(dt)  # noqa: E731
        o = tr.egno_forward(p, d(x), d(nodes), r, c, d(ea), d(v), d(lm), t.cpu(), T=T, lrelu_masks=masks, **kw)
        lo, _ = _loss_like_reference(o[0], loc_true.to(dt), T, B, N)
        lo.backward()
        return lo, [a.detach() for a in o], p

    ys = []
    l64, o64, p64 = torch_run(torch.float64, lrelu_record=ys)
    l32, o32, p32 = torch_run(torch.float32)
    _flips_lie_at_the_kink(masks, ys)
    tag = f"amplified T={T} modes={modes} B={B} N={N}"
    for name, a_inf, a_trn, ref, f32 in zip("xvh", inf, out, o64, o32):
        bar = max(R.BAR, 2 * maxnorm_rel(f32.numpy(), ref.numpy()))
        check_rel(f"{tag} inference {name}", a_inf, ref, bar)
        check_rel(f"{tag} training forward {name}", a_trn, ref, bar)
    lref = float(l64.detach())
    assert abs(float(loss.detach()) - lref) <= max(R.BAR * abs(lref), 2 * abs(float(l32.detach()) - lref))
    for k, q in m.named_parameters():
        ref = p64[k].grad
        if ref is None or float(ref.abs().max()) == 0:
            assert q.grad is None or float(q.grad.abs().max()) == 0, k
        else:
            bar = max(R.BAR, 2 * maxnorm_rel(p32[k].grad.numpy(), ref.numpy()))
            check_rel(f"{tag} grad {k}", q.grad, ref, bar)


def test_egno_amplified_tconv_multi_input_forward():
    """num_inputs = 3 (the per-frame variant of the first-layer TimeConv kernel), T = 10, 2 modes, B = 3, N = 7,
    TimeConv weights x 2^9: the inference forward and the training forward against the float64 frames reference
    of tests/test_gpu_input_grads.py at the training forward's LeakyReLU decisions; same bar rule."""
    I, T, B, N = 3, 10, 3, 7
    BN, E = B * N, B * N * (N - 1)
    m = _amplify_model(_model_inputs(T=T, seed=7, num_inputs=I))
    g = torch.Generator().manual_seed(T)
    x, lm = torch.randn(I, BN, 3, generator=g), 0.3 * torch.randn(I, BN, 3, generator=g)
    v = 0.5 * torch.randn(I, BN, 3, generator=g)
    h = torch.cat([v.norm(dim=-1, keepdim=True), torch.randint(0, 2, (I, BN, 1), generator=g).float() * 2 - 1], -1)
    ef = torch.randn(I, E, 2, generator=g).abs()
    row, col = tr.full_edges(B, N)
    t_in, t_out = torch.arange(-I + 1, 1).repeat(B, 1), torch.arange(1, T + 1).repeat(B, 1)
    dv = lambda a: a.to(DEV)  # noqa: E731

    def run():
        return m(dv(x), dv(h), [dv(row), dv(col)], dv(ef), v=dv(v), loc_mean=dv(lm), timesteps_in=dv(t_in),
                 timesteps_out=dv(t_out))

    m.eval()
    with torch.no_grad():
        inf = run()
    m.train()
    m._train_state_sink = []
    out = run()
    masks = _hip_lrelu_masks(m._train_state_sink.pop(), m.n_layers, T, BN)
    del m._train_state_sink
    torch.cuda.synchronize()
    refs = []
    for dt in (torch.float64, torch.float32):
        p = {k: q.detach().cpu().to(dt) for k, q in m.state_dict().items()}
        with torch.no_grad():
            refs.append(_frames_ref(p, x.to(dt), h.to(dt), row, col, ef.to(dt), v.to(dt), lm.to(dt), t_in, t_out,
                                    m.frame_inputs(T), T, masks))
    for name, a_inf, a_trn, ref, f32 in zip("xvh", inf, out, *refs):
        bar = max(R.BAR, 2 * maxnorm_rel(f32.numpy(), ref.numpy()))
        check_rel(f"amplified multi-input inference {name}", a_inf, ref, bar)
        check_rel(f"amplified multi-input training forward {name}", a_trn, ref, bar)
