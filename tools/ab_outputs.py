"""Save the C2 EGNO forward and C3 SEGNO outputs of the library NONODE_LIB points at, for bitwise
A/B comparison of kernel variants, and the general-graph and flat=True cases for the A/B of two whole
trees (run the copy of this file in each tree): EGNO / SEGNO graph="any" forwards and one
EGNO(graph="trainable") step (every parameter gradient and dL/dx, dL/dv, dL/dh, dL/dloc_mean; once more
with an operand cap that forces several frame groups) on tests/_graph_case.sparse_graph(80) and (37),
T = 10, and one EGNO(flat=True) training step at B = 2, N = 5. Every seed is fixed.
Usage (GPU box): NONODE_LIB=ab/lib_x.so python3 tools/ab_outputs.py out.npz
        python3 tools/ab_outputs.py --cmp a.npz b.npz"""
import os
import sys

import numpy as np

if sys.argv[1] == "--cmp":
    a, b = np.load(sys.argv[2]), np.load(sys.argv[3])
    for k in sorted(set(a.files) ^ set(b.files)):
        print(f"{k}: identical=False (in one file only)")
    for k in a.files:
        if k not in b.files:
            continue
        d = np.abs(a[k].astype(np.float64) - b[k])
        print(f"{k}: identical={np.array_equal(a[k], b[k])} maxabs={d.max():.3e} "
              f"maxnorm_rel={d.max() / max(np.abs(a[k]).max(), 1e-30):.3e}")
    sys.exit(0)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import bench  # noqa: E402
import no_node_comparison_amd as pkg  # noqa: E402

dev = torch.device("cuda:0")
torch.manual_seed(0)
m = pkg.EGNO(n_layers=4, in_node_nf=2, in_edge_nf=2, hidden_nf=64, with_v=True, num_modes=2, num_timesteps=10,
             time_emb_dim=32, device=dev).eval()
c = bench.build_egno_case(512, 20, 10, seed=1234, dev=dev)
out = {}
with torch.no_grad():
    x, v, h = m(c["x"], c["h"], c["edges"], c["edge_fea"], v=c["v"], loc_mean=c["loc_mean"], timesteps_out=c["t_out"])
    out.update(egno_x=x, egno_v=v, egno_h=h)
    s = pkg.SEGNO(in_node_nf=1, in_edge_nf=2, hidden_nf=64, n_layers=4, recurrent=True, device=dev).eval()
    ea = torch.cat([c["edge_fea"][:, :1], c["edge_fea"][:, 1:]], 1)
    xs, hs, vs = s(c["v"].norm(dim=-1, keepdim=True), c["x"], c["edges"], c["v"], ea, T=10)
    out.update(segno_x=xs, segno_h=hs, segno_v=vs)


def egno(**kw):
    torch.manual_seed(0)
    return pkg.EGNO(n_layers=4, in_node_nf=2, in_edge_nf=2, hidden_nf=64, with_v=True, num_modes=2, num_timesteps=10,
                    time_emb_dim=32, device=dev, **kw)


def train_step(tag, model, x, h, edges, ef, v, lm):
    """One taped forward and backward of a fixed weighted loss: outputs, parameter and input gradients."""
    ins = {k: t.clone().requires_grad_(True) for k, t in (("x", x), ("h", h), ("v", v), ("loc_mean", lm))}
    model.train().zero_grad(set_to_none=True)
    res = model(ins["x"], ins["h"], edges, ef, v=ins["v"], loc_mean=ins["loc_mean"])
    g = torch.Generator(device="cpu").manual_seed(5)
    loss = sum((o * torch.randn(o.shape, generator=g).to(dev)).sum() for o in res)
    loss.backward()
    out.update({f"{tag}_out_{k}": o.detach() for k, o in zip("xvh", res)})
    out.update({f"{tag}_grad_{k}": p.grad for k, p in model.named_parameters() if p.grad is not None})
    out.update({f"{tag}_dL_d{k}": t.grad for k, t in ins.items() if t.grad is not None})


def node_inputs(n, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda *shape: torch.randn(*shape, generator=g).to(dev)  # noqa: E731
    x = r(n, 3)
    return x, r(n, 2), r(n, 3), x.mean(0, keepdim=True).expand(n, 3).contiguous()


from tests._graph_case import edge_features, sparse_graph  # noqa: E402

for n in (80, 37):
    row, col = sparse_graph(n)
    edges = [torch.tensor(row).to(dev), torch.tensor(col).to(dev)]
    ef = torch.tensor(edge_features(len(row), 2)).to(dev)
    x, h, v, lm = node_inputs(n, 100 + n)
    with torch.no_grad():
        res = egno(graph="any").eval()(x, h, edges, ef, v=v, loc_mean=lm)
        out.update({f"graph{n}_egno_{k}": o for k, o in zip("xvh", res)})
        torch.manual_seed(0)
        sg = pkg.SEGNO(in_node_nf=1, in_edge_nf=2, hidden_nf=64, n_layers=4, recurrent=True, device=dev, graph="any").eval()
        res = sg(v.norm(dim=-1, keepdim=True), x, edges, v, ef, T=10)
        out.update({f"graph{n}_segno_{k}": o for k, o in zip("xhv", res)})
    train_step(f"graph{n}_train", egno(graph="trainable"), x, h, edges, ef, v, lm)
    m = egno(graph="trainable")
    m.graph_ops_cap_bytes = 3 * len(row) * 1600   # three frames per group: four groups for T = 10
    train_step(f"graph{n}_train_groups", m, x, h, edges, ef, v, lm)
B, N = 2, 5
c = bench.build_egno_case(B, N, 10, seed=4321, dev=dev)
train_step("flat_train", egno(flat=True), c["x"], c["h"], c["edges"], c["edge_fea"], c["v"], c["loc_mean"])
np.savez(sys.argv[1], **{k: t.float().cpu().numpy() for k, t in out.items()})
print("saved", sys.argv[1])
