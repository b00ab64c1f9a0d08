"""Shared helper of tests/test_tconv_scale.py and tests/test_gpu_tconv_scale.py (not collected).

TimeConv computes h_out = h + LeakyReLU(y) with y the truncated-DFT channel mix of h (layer_no.py:96-126),
and at the initial weights max|y| ~ 1.5e-3 max|h|: a comparison of h_out at 1e-5 of max|h| lets an error of
~0.7 % of y pass, and the reverse (g_h_in = g_out + adjoint term) hides its mixing the same way. Recovering
y from h_out - h in fp32 does not help: it resolves no better than the rounding of the residual add.

The device used here instead: multiply TimeConv's weights1 by an exact power of two 2^k with
k = round(log2(max|h| / max|y0|)), y0 the float64 spectral term at the unscaled weights. The packed fp16
hi / lo fragments are normalised by their own power of two (tconv_pack_h16_kernel), so they stay bit-identical
and every mantissa operation of the kernel is the one the shipped weights get; only exponents move. Then
max|y| ~ max|h|, and an output comparison at 1e-5 is a comparison at y's own scale.

The float64 reference is oracle/torch_ref.py's _spectral in the expression of egno.py:99-108 (as
oracle/torch_ref.py's egno_forward restates it), the reverse torch autograd of that expression.
"""
import math

import torch
import torch.nn.functional as F

from oracle import torch_ref as tr

SLOPE = 0.01          # TimeConv's LeakyReLU (layer_no.py:123)
KINK = 1e-4           # |y| below KINK max|y|: the output gradient there is set to exactly 0
MAX_ZEROED = 2e-3     # condition on the inputs: at most 0.2 % of gout_h may be zeroed that way
BAR = 1e-5            # the project's fixed fp32 bar
CU_MI355X = 256       # compute units of the MI355X (the CPU checks generate the GPU cases at its sizes)

# (T, modes) of the forward at BN_small: mode bounds 2 / 4 / 9 x frame bounds 10 / 16, the Nyquist bins
# (8,5), (10,6), (12,7), modes clamped to T // 2 + 1 (11,9), T = 2
FWD_SMALL = [(10, 1), (10, 2), (16, 2), (2, 2), (9, 3), (10, 4), (16, 4), (10, 5), (8, 5), (10, 6), (12, 7), (11, 9),
             (16, 9)]
# one (T, modes) per compiled forward instance, run at BN_xcd and BN_four
FWD_INSTANCES = [(10, 2), (16, 2), (10, 4), (16, 4), (10, 5), (16, 9)]
# (T, modes, size name) of the reverse: every MM at TB = 16, TB = 10 and the Nyquist bin, the clamp, the
# two-group form's second trip, the one-group form's second trip
REV_CASES = ([(16, m, "small") for m in range(1, 10)] + [(10, m, "small") for m in range(1, 7)]
             + [(8, 5, "small"), (11, 9, "small"), (10, 2, "two_trips"), (16, 2, "two_trips"), (10, 5, "four"),
                (16, 4, "four"), (16, 9, "four")])


def bn_sizes(cu):
    """Column counts by the forms of the kernels they reach, for a device of `cu` compute units.
    small: 3 tiles of 16 columns, ragged: the forward's five-wave form without the XCD order.
    xcd: 65 tiles, ragged: five-wave, XCD order, grid 72 > tiles (workgroups that return early).
    four: cu + 1 tiles: the forward's four-wave form; tconv_bwd_kernel with MM > 2 (one tile per workgroup
    and trip, min(cu, 256) workgroups) takes a second trip with a single tile.
    two_trips: the two-group reverse (MM <= 2, two tiles per workgroup and trip) goes into its second trip
    with one tile, group 1 past the last tile.
    c2: B = 512, N = 20 (the C2 / C4 size): 640 tiles, two or three workgroups resident per CU at once."""
    return {"small": 37, "xcd": 1030, "four": 16 * cu + 4, "two_trips": 2 * 16 * min(cu, 256) + 4, "c2": 512 * 20}


def case(T, modes, BN, seed):
    """Inputs of one TimeConv + TimeConv_x block and the gradients of its outputs, float32 from a seeded
    generator; weights as the reference initialises them (layer_no.py:203-205: rand * 1 / (in * out))."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return dict(T=T, modes=modes, BN=BN, h=2 * rn(T, BN, 64), x=rn(T, BN, 3), v=rn(T, BN, 3), loc_mean=rn(BN, 3),
                gout_h=rn(T, BN, 64), gout_x=rn(T, BN, 3), gout_v=rn(T, BN, 3),
                tw=torch.rand(64, 64, modes, 2, generator=g) / (64 * 64),
                txw=torch.rand(2, 2, modes, 2, generator=g) / 4)


def amplify(h, w):
    """(w 2^k, k) with k = round(log2(max|h| / max|y0|)), y0 the float64 spectral term at w."""
    y0 = tr._spectral(h.double(), w.double())
    k = int(round(math.log2(float(h.abs().max()) / float(y0.abs().max()))))
    return torch.ldexp(w, torch.tensor(k)), k


def block(h, x, v, lm, tw, txw):
    """egno.py:99-108 on [T, BN, .] arrays: returns (h_out, x_out, v_out, y)."""
    y = tr._spectral(h, tw)
    X = torch.stack([x - lm, v], -1)
    X = X + tr._spectral(X, txw)
    return h + F.leaky_relu(y, SLOPE), X[..., 0] + lm, X[..., 1], y


def seed_of(T, modes, BN):
    """The seed of case (T, modes, BN) in both test files (the CPU file checks the GPU file's own inputs)."""
    return (T * 16 + modes) * 100003 + BN


def reference(c, tw, chunk=1024, reverse=True):
    """Float64 forward and (reverse=True) reverse of the block for case c at TimeConv weights tw.

    The output gradient gout_h is set to exactly 0 wherever |y_ref| < KINK max|y_ref|, so that the LeakyReLU
    decision taken there does not matter and no element is left out of a comparison; `gout_h` (float32, to
    be passed to the code under test) and `zeroed`, the share of such elements, are returned with the
    reference. The reverse is torch autograd in column chunks (the columns are independent; the weight
    gradients add up in the leaves)."""
    d = lambda k: c[k].double()  # noqa: E731
    tw64 = tw.double().requires_grad_(True)
    txw64 = d("txw").requires_grad_(True)
    with torch.no_grad():
        h_out, x_out, v_out, y = block(d("h"), d("x"), d("v"), d("loc_mean"), tw64, txw64)
    ymax = float(y.abs().max())
    small = y.abs() < KINK * ymax
    gout_h = torch.where(small, torch.zeros((), dtype=torch.float32), c["gout_h"])
    r = dict(h_out=h_out, x_out=x_out, v_out=v_out, y=y, gout_h=gout_h, zeroed=float(small.double().mean()))
    r["scale_h_out"] = float(F.leaky_relu(y, SLOPE).abs().max())   # the spectral term alone
    if not reverse:
        return r
    gh, gx, gv = [], [], []
    for lo in range(0, c["BN"], chunk):
        s = slice(lo, lo + chunk)
        hl, xl, vl = (d(k)[:, s].clone().requires_grad_(True) for k in ("h", "x", "v"))
        ho, xo, vo, _ = block(hl, xl, vl, d("loc_mean")[s], tw64, txw64)
        ((ho * gout_h[:, s].double()).sum() + (xo * d("gout_x")[:, s]).sum() + (vo * d("gout_v")[:, s]).sum()).backward()
        gh.append(hl.grad), gx.append(xl.grad), gv.append(vl.grad)
    r.update(g_h_in=torch.cat(gh, 1), g_x_in=torch.cat(gx, 1), g_v_in=torch.cat(gv, 1), g_tw=tw64.grad,
             g_txw=txw64.grad)
    r["scale_g_h_in"] = float((r["g_h_in"] - gout_h.double()).abs().max())   # the adjoint term alone
    return r


def scale_of(r, name):
    return r.get("scale_" + name, None) or float(r[name].abs().max())


def rel(got, ref, scale):
    """max|got - ref| / scale, in float64."""
    got = torch.as_tensor(got).detach().cpu().double().reshape(ref.shape)
    return float((got - ref.double()).abs().max()) / scale
