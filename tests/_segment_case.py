"""Helpers of test_gpu_segment_boundary: small EGNO / SEGNO cases on complete graphs, their float64
oracle, and runs of one case under a cap on the layer grid (NONODE_WGS), so that one workgroup walks
several chunks and carries its state from chunk to chunk."""
import numpy as np
import torch

import no_node_comparison_amd as pkg
from oracle import egno as oe
from oracle import harness as oh
from oracle import segno as osg

DEV = "cuda"
# nonode_debug_boundary_switches: the tile-segment boundary's levers of the build under test
PREB, UCUT = 1, 2


def dev(a):
    return torch.tensor(np.ascontiguousarray(a)).to(DEV)


def sd_np(model):
    return {k: v.detach().cpu().numpy().astype(np.float64) for k, v in model.state_dict().items()}


def synthetic_charged(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    sigma = (N / 5.0) ** (1.0 / 3.0)
    loc = torch.randn(B, N, 3, generator=g) * sigma
    vel = torch.randn(B, N, 3, generator=g)
    vel = vel / vel.norm(dim=-1, keepdim=True) * 0.5
    q = (torch.randint(0, 2, (B, N, 1), generator=g) * 2 - 1).float()
    return loc, vel, q


def egno(T, seed, in_edge_nf=2, n_layers=2):
    torch.manual_seed(seed)
    return pkg.EGNO(n_layers=n_layers, in_node_nf=2, in_edge_nf=in_edge_nf, hidden_nf=64, with_v=True, num_modes=2,
                    num_timesteps=T, time_emb_dim=32, device=DEV).eval()


def egno_case(B, N, T, seed, in_edge_nf=2):
    """The charged-particle inputs of B samples; in_edge_nf > 2 appends seeded normal edge features."""
    loc, vel, q = synthetic_charged(B, N, seed)
    r, c = oh.full_edges(B, N)
    qq = q.reshape(-1, 1).numpy()
    eao = (qq[r] * qq[c]).astype(np.float32)
    x, v, ea, nodes, lm = oh.prepare_inputs(loc.numpy(), vel.numpy(), eao, r, c, N, q.numpy())
    if in_edge_nf > ea.shape[1]:
        extra = np.random.default_rng(seed).standard_normal((ea.shape[0], in_edge_nf - ea.shape[1]))
        ea = np.concatenate([ea, extra.astype(ea.dtype)], 1)
    t_out = np.tile(np.arange(1, T + 1), (B, 1))
    return dict(x=x, h=nodes, row=r, col=c, edge_fea=ea, v=v, loc_mean=lm, t_out=t_out)


def egno_oracle(m, case, T, n_layers=2):
    return oe.egno_forward(sd_np(m), **{k: (v.astype(np.float64) if k not in ("row", "col", "t_out") else v)
                                         for k, v in case.items()}, n_layers=n_layers, T=T)


def egno_run(m, case, grad=False):
    """(x, v, h) on the host; grad: the taped (training) forward of a model in train mode."""
    with torch.enable_grad() if grad else torch.no_grad():
        out = m(dev(case["x"]), dev(case["h"]), [dev(case["row"]), dev(case["col"])], dev(case["edge_fea"]),
                v=dev(case["v"]), loc_mean=dev(case["loc_mean"]), timesteps_out=dev(case["t_out"]))
    torch.cuda.synchronize()
    return [o.detach().cpu() for o in out]


def segno(seed):
    torch.manual_seed(seed)
    return pkg.SEGNO(in_node_nf=1, in_edge_nf=2, hidden_nf=64, n_layers=8, recurrent=True, device=DEV).eval()


def segno_case(B, N, seed):
    loc, vel, q = synthetic_charged(B, N, seed)
    r, c = oh.full_edges(B, N)
    x = loc.reshape(-1, 3).numpy().astype(np.float64)
    v = vel.reshape(-1, 3).numpy().astype(np.float64)
    qq = q.reshape(-1, 1).numpy()
    ea = np.concatenate([qq[r] * qq[c], ((x[r] - x[c]) ** 2).sum(1, keepdims=True)], 1)
    return dict(his=np.sqrt((v ** 2).sum(1, keepdims=True)), x=x, row=r, col=c, v=v, ea=ea)


def segno_oracle(m, case, T):
    return osg.forward(sd_np(m), case["his"], case["x"], case["row"], case["col"], case["v"], case["ea"], T=T,
                       bug_compat=False)


def segno_run(m, case, T):
    f = lambda a: dev(a.astype(np.float32))  # noqa: E731
    with torch.no_grad():
        out = m(f(case["his"]), f(case["x"]), [dev(case["row"]), dev(case["col"])], f(case["v"]), f(case["ea"]), T=T)
    torch.cuda.synchronize()
    return [o.cpu() for o in out]


def capped_runs(monkeypatch, run, caps):
    """run() once per cap on the layer grid (None: uncapped), in order."""
    outs = []
    for cap in caps:
        if cap is None:
            monkeypatch.delenv("NONODE_WGS", raising=False)
        else:
            monkeypatch.setenv("NONODE_WGS", str(cap))
        outs.append(run())
    monkeypatch.delenv("NONODE_WGS", raising=False)
    return outs


def assert_bitwise(names, a, b, what):
    for name, u, w in zip(names, a, b):
        assert torch.equal(u, w), f"{name}: {what}"
