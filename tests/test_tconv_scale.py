"""CPU checks of tests/_tconv_ref.py, the reference and inputs of tests/test_gpu_tconv_scale.py: the float64
reference against an independent written-out real DFT and against oracle/egno_grad.py's hand-written reverse,
the exactness and effect of the power-of-two amplification, the share of zeroed output gradients, and the
sensitivity of the metric itself (why the amplification is needed at all)."""
import functools

import numpy as np
import pytest
import torch

from oracle import egno_grad as og
from tests import _tconv_ref as R

# (2,2); the Nyquist bins (8,5), (10,6), (12,7); (11,9): modes clamp to 6; (16,9); (10,1)
PAIRS = [(2, 2), (8, 5), (10, 6), (12, 7), (11, 9), (16, 9), (10, 1)]
BN = 5


def _real_dft(x, w, T):
    """The formula above tconv_pack_kernel, written out: x [T, rows, Cin], w [Cin, Cout, modes, 2].
    Yr = A^T Xr + B^T Xs, Yi = B^T Xr - A^T Xs with A = c_m Wr / T, B = c_m Wi / T, Xr = sum_t x cos,
    Xs = sum_t x sin; y[t] = sum_m Yr cos - Yi sin; c_m = 1 for m = 0 and 2 m = T, else 2."""
    M = min(w.shape[2], T // 2 + 1)
    y = np.zeros((T,) + x.shape[1:-1] + (w.shape[1],))
    t = np.arange(T)
    for m in range(M):
        cos, sin = np.cos(2 * np.pi * m * t / T), np.sin(2 * np.pi * m * t / T)
        cm = 1.0 if (m == 0 or 2 * m == T) else 2.0
        A, B = cm / T * w[:, :, m, 0], cm / T * w[:, :, m, 1]
        Xr, Xs = np.tensordot(cos, x, (0, 0)), np.tensordot(sin, x, (0, 0))
        Yr, Yi = Xr @ A + Xs @ B, Xr @ B - Xs @ A
        y += cos.reshape((T,) + (1,) * (x.ndim - 1)) * Yr - sin.reshape((T,) + (1,) * (x.ndim - 1)) * Yi
    return y


def _case(T, modes):
    c = R.case(T, modes, BN, seed=R.seed_of(T, modes, BN))
    tw, _ = R.amplify(c["h"], c["tw"])
    return c, tw


def _close(got, ref, tol):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.abs(got - ref).max() <= tol * np.abs(ref).max()


@pytest.mark.parametrize("T,modes", PAIRS)
def test_forward_reference_equals_written_out_real_dft(T, modes):
    c, tw = _case(T, modes)
    r = R.reference(c, tw, reverse=False)
    n = lambda a: a.double().numpy()  # noqa: E731
    y = _real_dft(n(c["h"]), n(tw), T)
    assert _close(r["y"], y, 1e-12)
    assert _close(r["h_out"], n(c["h"]) + np.where(y > 0, y, 0.01 * y), 1e-12)
    lm = n(c["loc_mean"])
    X = np.stack([n(c["x"]) - lm, n(c["v"])], -1)
    X = X + _real_dft(X, n(c["txw"]), T)
    assert _close(r["x_out"], X[..., 0] + lm, 1e-12)
    assert _close(r["v_out"], X[..., 1], 1e-12)


@pytest.mark.parametrize("T,modes", PAIRS)
def test_autograd_reference_equals_oracle_spectral_bwd(T, modes):
    c, tw = _case(T, modes)
    r = R.reference(c, tw)
    M = min(modes, T // 2 + 1)
    n = lambda a: a.double().numpy()  # noqa: E731
    pad = lambda g: np.concatenate([g, np.zeros(g.shape[:2] + (modes - M, 2))], 2)  # noqa: E731  bins >= M: zero
    w, wx = n(tw)[:, :, :M], n(c["txw"])[:, :, :M]
    y, X = og.spectral_fwd(n(c["h"]), w)
    gout = n(r["gout_h"])
    gx, gw = og.spectral_bwd(gout * np.where(y > 0, 1.0, R.SLOPE), n(c["h"]), X, w)
    assert _close(r["g_h_in"], gout + gx, 1e-10)
    assert _close(r["g_h_in"] - r["gout_h"].double(), gx, 1e-10)   # the adjoint term alone
    assert _close(r["g_tw"], pad(gw), 1e-10)
    X0 = np.stack([n(c["x"]) - n(c["loc_mean"]), n(c["v"])], -1)
    gX = np.stack([n(c["gout_x"]), n(c["gout_v"])], -1)
    gX0, gwx = og.spectral_bwd(gX, X0, og.spectral_fwd(X0, wx)[1], wx)
    assert _close(r["g_x_in"], (gX + gX0)[..., 0], 1e-10)
    assert _close(r["g_v_in"], (gX + gX0)[..., 1], 1e-10)
    assert _close(r["g_txw"], pad(gwx), 1e-10)
    if modes > M:
        assert float(r["g_tw"][:, :, M:].abs().max()) == 0 and float(r["g_txw"][:, :, M:].abs().max()) == 0


def _gpu_cases():
    """Every (T, modes, BN) of tests/test_gpu_tconv_scale.py's tables, at the MI355X's sizes."""
    bn = R.bn_sizes(R.CU_MI355X)
    cases = [(T, m, bn["small"]) for T, m in R.FWD_SMALL]
    cases += [(T, m, bn[k]) for k in ("xcd", "four", "c2") for T, m in R.FWD_INSTANCES]
    cases += [(T, m, bn[k]) for T, m, k in R.REV_CASES]
    return sorted(set(cases), key=lambda c: (c[2], c[0], c[1]))


@functools.lru_cache(maxsize=None)
def _amplified(T, modes, BN):
    c = R.case(T, modes, BN, seed=R.seed_of(T, modes, BN))
    tw, k = R.amplify(c["h"], c["tw"])
    r = R.reference(c, tw, reverse=False)
    exact = torch.equal(torch.ldexp(tw, torch.tensor(-k)), c["tw"]) and torch.equal(tw, c["tw"] * float(2.0 ** k))
    return k, exact, float(r["y"].abs().max()) / float(c["h"].abs().max()), r["zeroed"]


@pytest.mark.parametrize("T,modes,BN", _gpu_cases())
def test_amplification_is_exact_and_brings_y_to_the_scale_of_h(T, modes, BN):
    k, exact, ratio, _ = _amplified(T, modes, BN)
    assert isinstance(k, int) and exact
    assert 0.5 <= ratio <= 2, ratio


@pytest.mark.parametrize("T,modes,BN", _gpu_cases())
def test_zeroed_share_of_the_output_gradient_is_small(T, modes, BN):
    assert _amplified(T, modes, BN)[3] <= R.MAX_ZEROED


@pytest.mark.parametrize("T,modes", [(10, 2), (16, 9)])
def test_metric_sees_a_relative_error_of_1e_3_in_one_mode_only_at_amplified_weights(T, modes):
    """One mode's 64 x 64 matrix times (1 + 1e-3) in the "got" path: above the bar on the h_out metric at the
    amplified weights; at the shipped weights the same error stays below the bar at the scale of h, which is
    all the output comparisons before this file could see."""
    c = R.case(T, modes, 37, seed=R.seed_of(T, modes, 37))
    tw, _ = R.amplify(c["h"], c["tw"])

    def got_ref(w):
        wp = w.clone()
        wp[:, :, 1] *= 1 + 1e-3
        return R.reference(c, wp, reverse=False)["h_out"], R.reference(c, w, reverse=False)

    got, r = got_ref(tw)
    assert R.rel(got, r["h_out"], R.scale_of(r, "h_out")) > R.BAR
    got, r = got_ref(c["tw"])
    assert R.rel(got, r["h_out"], float(r["h_out"].abs().max())) < R.BAR
