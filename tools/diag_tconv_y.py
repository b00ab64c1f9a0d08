"""Diagnostic: accuracy of TimeConv's spectral term y from nonode_egno_tconv against float64, at y's own
scale. The TimeConv weights are multiplied by the exact power of two that makes max|y| ~ max|h|
(tests/_tconv_ref.py: the packed fp16 hi / lo fragments stay bit-identical), so "rel" = max|h_out - ref| /
max|LeakyReLU(y_ref)| resolves y to fp32 rounding. (Until round 6 this tool recovered y as
LeakyReLU^-1(h_out - h) at the shipped weights, which resolves y no better than the rounding of the residual
add, 3e-3 ... 7e-3 of max|y|: its "rel" column could not tell a good build from one 0.5 % off.)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import no_node_comparison_amd as pkg  # noqa: E402
from tests import _tconv_ref as R  # noqa: E402

DEV = "cuda"
L = pkg._lib.lib()
P = pkg._lib.ptr
for T, modes, BN in [(T, m, bn) for bn in (1024, 10240) for T in (8, 16) for m in (2, 3, 4, 5, 9)]:
    c = R.case(T, modes, BN, seed=R.seed_of(T, modes, BN))
    tw, k = R.amplify(c["h"], c["tw"])
    r = R.reference(c, tw, reverse=False)
    d = lambda a: a.to(DEV).contiguous()  # noqa: E731
    hd, xd, vd = (d(c[n].reshape(T * BN, -1)) for n in ("h", "x", "v"))
    lmd, twd, txw = d(c["loc_mean"]), d(tw), d(c["txw"])
    blob = torch.empty(L.nonode_tconv_blob_floats(modes), dtype=torch.float32, device=DEV)
    pkg._lib.check(L.nonode_pack_tconv(P(twd), modes, T, P(blob), pkg._lib.stream_of(blob)))
    ho, xo, vo = torch.empty_like(hd), torch.empty_like(xd), torch.empty_like(vd)
    pkg._lib.check(L.nonode_egno_tconv(BN, T, modes, P(hd), P(xd), P(vd), P(lmd), P(blob), P(txw), P(ho), P(xo),
                                       P(vo), pkg._lib.stream_of(hd)))
    torch.cuda.synchronize()
    rels = {n: R.rel(got, r[n], R.scale_of(r, n)) for n, got in (("h_out", ho), ("x_out", xo), ("v_out", vo))}
    print(f"BN={BN} T={T} modes={modes}: weights x 2^{k}  max|y|/max|h| {float(r['y'].abs().max() / c['h'].abs().max()):.2f}  "
          f"rel {rels['h_out']:.3e}  (x_out {rels['x_out']:.2e}, v_out {rels['v_out']:.2e})", flush=True)
