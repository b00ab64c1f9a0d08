"""Timings of the general-graph path (EGNO graph="any", csrc/nonode_graph.hip) on the GPU. One JSON
line per case on stdout (DESIGN.md section 3.7 quotes them; raw lines under profiles/graph/).

python tools/bench_graph.py [--case price|knn|knn_train|knn_rollout|ragged_rollout|knn_rollout_train|segno_train|cells|cells_rollout|knn_cells|knn_cells_rollout|all] [--reps 7] [--iters 20] [--arm both|ours]

  price  the C2 graph (B = 512, N = 20, T = 10: 5120 fully connected graphs per layer launch) through
         the fused layer entry (nonode_egnn_layer) and, passed as an edge list, through the general one
         (nonode_egnn_layer_graph: projection + edge walk + node update). Per-layer time of each, the
         two alternated `reps` times on the same box; the ratio is the price of generality.
  knn    8 graphs x 1000 nodes, the 16 nearest neighbours of each node as its senders, T = 10, 4
         layers: EGNO(graph="any") per forward against oracle/torch_ref.egno_forward (the reference's own
         formulation: gathers, Linear, index_add) in fp32 on the same device, alternated likewise; and
         the edge walk's share of the fp16x3 ceiling from the layer's time as an upper bound on the edge
         walk's own (kernel times proper: rocprofv3 --kernel-trace --stats of this script, in a run of
         its own).
  knn_train  the knn case trained: one forward + backward of EGNO(graph="trainable").train() (loss on x; every
         parameter's gradient) against fp32 autograd of oracle/torch_ref.egno_forward on the same device,
         alternated likewise. --arm ours runs the HIP arm alone (for a rocprofv3 --kernel-trace --stats run
         of its own: the per-kernel split).
  knn_rollout  the knn case rolled out: traj_len = 4 segments, the 16-neighbour graph rebuilt from the
         predicted positions every segment. harness.egno_rollout_graph (device-side builder and featuriser)
         against the loop a user writes without them: knn_graph below (cdist + topk), torch featurisation
         on that list, model(graph="any"), alternated likewise. --arm ours runs the first arm alone (for a
         rocprofv3 --kernel-trace --stats run of its own: the builder's and the featuriser's share).
  ragged_rollout  graphs of mixed sizes in one batch: eight systems of 250 .. 1750 nodes (8000 in all, the node count
         of knn_rollout), k = 16, T = 10, 4 layers, traj_len = 4, the damped heads of knn_rollout.
         harness.egno_rollout_graph(sizes=...) on the batch in one call against the same eight systems rolled out
         one after another through the equal-size driver with batch_size = 1 (eight times the launches, each at
         a fraction of the machine), alternated likewise, after one check that the two agree per system. Whole-
         rollout times (host loop and every launch), not kernel times.
  knn_rollout_train  the knn case trained through an unrolled rollout: traj_len = 2 segments, the graph rebuilt
         from the predicted positions every segment, forward + backward of a loss on every predicted frame.
         harness.egno_rollout_train_graph (the padded NeighborGraph with its device-built CSR by sender on the
         tape, the taped featuriser: nothing read back) against the route without them: per segment
         ng.edge_index() (one host synchronisation), edge_fea[:E], a taped forward on the compacted list (both
         CSRs through graph.csr / graph.csr_by_sender's cached-list builds) and the frame choice and loc_mean as
         torch ops on the tape, alternated likewise. --arm ours runs the first arm alone.
  segno_train  SEGNO trained on the knn graph: 8 graphs x 1000 nodes, k = 16 (the device-built NeighborGraph with its
         CSR by sender, edge_attr [capacity, 2]), T = 10 substeps, one forward + backward of
         SEGNO(graph="any", trainable=True).train() (MSE on x; every live parameter's gradient) against fp32 autograd
         of oracle/torch_ref.segno_forward_step (dense_mean=False) on the graph's list on the same device, alternated
         likewise. --arm ours runs the HIP arm alone.
  cells  the neighbour-graph builder alone under a cut-off, the brute-force search (method="brute") against the
         cell list (method="cells"), alternated likewise: uniform points in a cube at about 12 candidates per
         receiver (r_cut = 1.5, side 10 (N / 1000)^(1/3)), k = 16, one graph of 1,000 .. 100,000 nodes and
         8 x 1000; one line per shape, with whether the two gave the same arrays.
  cells_rollout  knn_rollout under that cut-off at 8 x 1000 and 1 x 20,000, the graph rebuilt every segment by
         either search (harness.egno_rollout_graph(neighbor_method=...)), alternated likewise.
  knn_cells  the builder alone on the pure k-NN graph (r_cut=None, k = 16, the same cubes and shapes): method="brute"
         against the k-NN search on the cell list (method="knn_cells"), alternated likewise, one line per shape;
         and one line under a loose cut-off (r_cut = 3.6, some 195 candidates per receiver) at 1 x 50,000,
         method="cells" against "knn_cells".
  knn_cells_rollout  cells_rollout without the cut-off at 1 x 20,000, "brute" against "knn_cells".
Times are device events around `iters` back-to-back calls after a warm-up; each case reports the median
over the reps and the spread (min, max) beside it.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import no_node_comparison_amd as pkg  # noqa: E402
from no_node_comparison_amd import _lib, autograd, graph, harness  # noqa: E402
from oracle import torch_ref as tr  # noqa: E402

DEV = torch.device("cuda:0")
FP16X3_PEAK_TFLOPS = 2500.0 / 3.0   # bench.py: dense fp16 MFMA peak / 3 (fp16x3 split products)
MAC_PER_EDGE = 8448                 # bench.py: edge MLP + coordinate MLP of one edge
MAC_PER_NODE = 24640


def timed(fn, iters):
    """ms per call: device events around `iters` back-to-back calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def alternate(arms, reps, iters):
    """{name: [ms per rep]}: every arm warmed up, then the arms alternated `reps` times."""
    for fn in arms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            out[k].append(timed(fn, iters))
    return out


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "reps": len(ms)}


def synthetic(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    sigma = (N / 5.0) ** (1.0 / 3.0)
    loc = torch.randn(B, N, 3, generator=g) * sigma
    vel = torch.randn(B, N, 3, generator=g)
    vel = vel / vel.norm(dim=-1, keepdim=True) * 0.5
    q = (torch.randint(0, 2, (B, N, 1), generator=g) * 2 - 1).float()
    return loc.to(DEV), vel.to(DEV), q.to(DEV)


def model(T, **kw):
    torch.manual_seed(0)
    return pkg.EGNO(n_layers=4, in_node_nf=2, in_edge_nf=2, hidden_nf=64, with_v=True, num_modes=2, num_timesteps=T,
                    time_emb_dim=32, device=DEV, **kw).eval()


def case_price(args):
    B, N, T = 512, 20, 10
    L, P = pkg.lib(), _lib.ptr
    m = model(T)
    blobs, _ = m._packed()
    loc, vel, q = synthetic(B, N, 1)
    rows, cols = graph.full_edges(B, N, DEV)
    x1, v1 = loc.reshape(-1, 3), vel.reshape(-1, 3)
    ef = torch.cat([(q.reshape(-1, 1)[rows] * q.reshape(-1, 1)[cols]), ((x1[rows] - x1[cols]) ** 2).sum(1, keepdim=True)],
                   1).contiguous()
    n, E = B * N, rows.numel()
    torch.manual_seed(1)
    h = (torch.randn(T * n, 64, device=DEV) * 0.5).contiguous()
    x, v = x1.repeat(T, 1).contiguous(), v1.repeat(T, 1).contiguous()
    ho, xo = torch.empty_like(h), torch.empty_like(x)
    ho2, xo2 = torch.empty_like(h), torch.empty_like(x)
    rp, cc, ee = graph.csr([rows.clone(), cols.clone()], n)
    ws_bytes = L.nonode_egnn_layer_graph_workspace_bytes(T, n)
    ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.float32, device=DEV)
    s = _lib.stream_of(h)

    def fused():
        _lib.check(L.nonode_egnn_layer(_lib.VARIANT_EGNO, T * B, N, 2, B, P(h), P(x), P(v), P(ef), P(blobs[0]), 0.0, 1.0, 0,
                                       P(ho), P(xo), None, s))

    def general():
        _lib.check(L.nonode_egnn_layer_graph(_lib.VARIANT_EGNO, T, n, E, 2, 1, P(h), P(x), P(v), P(ef), P(blobs[0]), P(rp),
                                             P(cc), P(ee), 0.0, 1.0, 0, P(ho2), P(xo2), None, P(ws), ws_bytes, s))

    t = alternate({"fused": fused, "general": general}, args.reps, args.iters)
    torch.cuda.synchronize()
    err = float((ho - ho2).abs().max() / ho.abs().max())
    f, g = stats(t["fused"]), stats(t["general"])
    return {"case": "price", "shape": {"B": B, "N": N, "T": T, "edges_per_layer": T * E},
            "fused_layer": f, "general_layer": g, "ratio_general_over_fused": g["median_ms"] / f["median_ms"],
            "ratio_per_rep": [b / a for a, b in zip(t["fused"], t["general"])],
            "h_maxnorm_rel_general_vs_fused": err, "iters": args.iters}


def knn_graph(loc, k):
    """rows (receivers), cols (their k nearest neighbours) of B graphs, node ids offset per graph."""
    B, N, _ = loc.shape
    d = torch.cdist(loc, loc)
    d.diagonal(dim1=1, dim2=2).fill_(float("inf"))
    nb = d.topk(k, dim=2, largest=False).indices                     # [B, N, k]
    off = (torch.arange(B, device=loc.device) * N)[:, None, None]
    rows = (torch.arange(N, device=loc.device)[None, :, None] + off).expand(B, N, k).reshape(-1)
    return rows.contiguous(), (nb + off).reshape(-1).contiguous()


def case_knn(args):
    B, N, T, K = 8, 1000, 10, 16
    m = model(T, graph="any")
    loc, vel, q = synthetic(B, N, 2)
    rows, cols = knn_graph(loc, K)
    x, v = loc.reshape(-1, 3).contiguous(), vel.reshape(-1, 3).contiguous()
    qq = q.reshape(-1, 1)
    ef = torch.cat([qq[rows] * qq[cols], ((x[rows] - x[cols]) ** 2).sum(1, keepdim=True)], 1).contiguous()
    h = torch.cat([v.norm(dim=1, keepdim=True), qq], 1).contiguous()
    lm = loc.mean(1, keepdim=True).repeat(1, N, 1).reshape(-1, 3).contiguous()
    t_out = torch.arange(1, T + 1, device=DEV).repeat(B, 1)
    n, E = B * N, rows.numel()
    p32 = {k_: t.detach().float() for k_, t in m.state_dict().items()}
    tf = t_out.float()

    def ours():
        with torch.no_grad():
            return m(x, h, [rows, cols], ef, v=v, loc_mean=lm, timesteps_out=t_out)

    def ref():
        with torch.no_grad(), torch.device(DEV):   # (torch_ref's factory calls take the default device)
            return tr.egno_forward(p32, x, h, rows, cols, ef, v, lm, tf, T=T)

    t = alternate({"general": ours, "torch_ref": ref}, args.reps, max(args.iters // 4, 3))
    a, b = ours(), ref()
    torch.cuda.synchronize()
    err = [float((u - w).abs().max() / w.abs().max()) for u, w in zip(a, b)]
    # one layer through the C entry: the three launches' time bounds the edge walk's from above
    L, P = pkg.lib(), _lib.ptr
    blobs, _ = m._packed()
    rp, cc, ee = graph.csr([rows, cols], n)
    torch.manual_seed(3)
    hh = (torch.randn(T * n, 64, device=DEV) * 0.5).contiguous()
    xx, vv = x.repeat(T, 1).contiguous(), v.repeat(T, 1).contiguous()
    ho, xo = torch.empty_like(hh), torch.empty_like(xx)
    ws_bytes = L.nonode_egnn_layer_graph_workspace_bytes(T, n)
    ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.float32, device=DEV)
    s = _lib.stream_of(hh)

    def layer():
        _lib.check(L.nonode_egnn_layer_graph(_lib.VARIANT_EGNO, T, n, E, 2, 1, P(hh), P(xx), P(vv), P(ef), P(blobs[0]),
                                             P(rp), P(cc), P(ee), 0.0, 1.0, 0, P(ho), P(xo), None, P(ws), ws_bytes, s))

    tl = stats(alternate({"layer": layer}, args.reps, args.iters)["layer"])
    flop_edges = 2.0 * T * E * MAC_PER_EDGE
    flop_layer = flop_edges + 2.0 * T * n * MAC_PER_NODE
    g, r = stats(t["general"]), stats(t["torch_ref"])
    return {"case": "knn", "shape": {"graphs": B, "nodes_per_graph": N, "k": K, "T": T, "layers": 4, "E": E},
            "general_forward": g, "torch_ref_fp32_forward": r, "speedup_over_torch_ref": r["median_ms"] / g["median_ms"],
            "speedup_per_rep": [b_ / a_ for a_, b_ in zip(t["general"], t["torch_ref"])],
            "maxnorm_rel_vs_torch_ref_xvh": err,
            "layer_three_launches": tl, "layer_algorithmic_gflop": flop_layer / 1e9,
            "layer_frac_of_fp16x3_peak": flop_layer / (tl["median_ms"] * 1e-3) / 1e12 / FP16X3_PEAK_TFLOPS,
            "edge_walk_algorithmic_gflop": flop_edges / 1e9,
            "edge_walk_frac_of_fp16x3_peak_lower_bound": flop_edges / (tl["median_ms"] * 1e-3) / 1e12 / FP16X3_PEAK_TFLOPS,
            "peak_basis": "dense fp16 MFMA peak / 3 (fp16x3 split products), as bench.py --full prices the fused layer"}


def case_knn_train(args):
    B, N, T, K = 8, 1000, 10, 16
    m = model(T, graph="trainable").train()
    loc, vel, q = synthetic(B, N, 2)
    rows, cols = knn_graph(loc, K)
    x, v = loc.reshape(-1, 3).contiguous(), vel.reshape(-1, 3).contiguous()
    qq = q.reshape(-1, 1)
    ef = torch.cat([qq[rows] * qq[cols], ((x[rows] - x[cols]) ** 2).sum(1, keepdim=True)], 1).contiguous()
    h = torch.cat([v.norm(dim=1, keepdim=True), qq], 1).contiguous()
    lm = loc.mean(1, keepdim=True).repeat(1, N, 1).reshape(-1, 3).contiguous()
    t_out = torch.arange(1, T + 1, device=DEV).repeat(B, 1)
    n, E = B * N, rows.numel()
    target = x.repeat(T, 1) + 0.1
    p32 = {k_: t.detach().float().clone().requires_grad_(True) for k_, t in m.state_dict().items()}
    tf = t_out.float()

    def ours():
        m.zero_grad(set_to_none=True)
        xo, _, _ = m(x, h, [rows, cols], ef, v=v, loc_mean=lm, timesteps_out=t_out)
        ((xo - target) ** 2).mean().backward()

    def ref():
        for t in p32.values():
            t.grad = None
        with torch.device(DEV):   # (torch_ref's factory calls take the default device)
            xo, _, _ = tr.egno_forward(p32, x, h, rows, cols, ef, v, lm, tf, T=T)
        ((xo - target) ** 2).mean().backward()

    arms = {"trainable": ours} if args.arm == "ours" else {"trainable": ours, "torch_ref": ref}
    t = alternate(arms, args.reps, max(args.iters // 4, 3))
    g = stats(t["trainable"])
    res = {"case": "knn_train", "shape": {"graphs": B, "nodes_per_graph": N, "k": K, "T": T, "layers": 4, "E": E},
           "trainable_fwd_bwd": g, "trainable_per_rep_ms": t["trainable"],
           "frame_groups_per_layer": len(autograd.graph_frame_groups(T, E))}
    if args.arm != "ours":
        r = stats(t["torch_ref"])
        ours()
        ref()
        torch.cuda.synchronize()
        gerr = {k_: float((q_.grad - p32[k_].grad).abs().max() / p32[k_].grad.abs().max())
                for k_, q_ in m.named_parameters() if p32[k_].grad is not None and float(p32[k_].grad.abs().max()) > 0}
        # (the loss reads x alone: the last layer's node_net has no gradient in either arm)
        res.update({"torch_ref_fp32_fwd_bwd": r, "torch_ref_per_rep_ms": t["torch_ref"],
                    "speedup_over_torch_ref": r["median_ms"] / g["median_ms"],
                    "speedup_per_rep": [b_ / a_ for a_, b_ in zip(t["trainable"], t["torch_ref"])],
                    "faster_on_every_alternation": all(a_ < b_ for a_, b_ in zip(t["trainable"], t["torch_ref"])),
                    "worst_grad_maxnorm_rel_vs_torch_ref_fp32": max(gerr.values())})
    return res


def case_knn_rollout(args):
    B, N, T, K, SEG, DAMP = 8, 1000, 10, 16, 4, 0.01
    loc, vel, q = synthetic(B, N, 2)
    t_out = torch.arange(1, T * SEG + 1, device=DEV).repeat(B, 1)
    m = model(T, graph="any")
    # what the undamped model does from these inputs, for the record (one rollout, not timed)
    up, _, _, ug = harness.egno_rollout_graph(m, loc, vel, q, N, B, SEG, k=K, timesteps_out=t_out, return_graphs=True)
    undamped = {"segment_absmax": [repr(float(up[i * T:(i + 1) * T].abs().max())) for i in range(SEG)],
                "segment_n_edges": [int(g.n_edges.item()) for g in ug]}
    # the untrained model's rollout overflows in the third segment from these inputs (the fourth would then be
    # timed on an empty graph in one arm and on NaN distances in the other): the last layers of the coordinate
    # and velocity heads are scaled down so that the positions stay bounded (the line records both rollouts' magnitudes)
    with torch.no_grad():
        for layer in m.layers:
            for head in (layer.coord_net, layer.node_v_net):
                head.mlp[2].weight.mul_(DAMP)
                head.mlp[2].bias.mul_(DAMP)
    qq = q.reshape(-1, 1)

    def ours():
        return harness.egno_rollout_graph(m, loc, vel, q, N, B, SEG, k=K, timesteps_out=t_out)[0]

    def by_hand():
        x, v = loc, vel
        preds = []
        with torch.no_grad():
            for i in range(SEG):
                rows, cols = knn_graph(x, K)
                x1, v1 = x.reshape(-1, 3), v.reshape(-1, 3)
                ef = torch.cat([qq[rows] * qq[cols], ((x1[rows] - x1[cols]) ** 2).sum(1, keepdim=True)], 1)
                h = torch.cat([v1.norm(dim=1, keepdim=True), qq], 1)
                lm = x.mean(1, keepdim=True).repeat(1, N, 1).reshape(-1, 3)
                xo, vo, _ = m(x1, h, [rows, cols], ef, v=v1, loc_mean=lm,
                              timesteps_out=t_out[:, i * T:(i + 1) * T] - i * T)
                preds.append(xo.reshape(T, B * N, 3))
                x, v = xo.reshape(T, B, N, 3)[-1], vo.reshape(T, B, N, 3)[-1]
        return torch.cat(preds)

    arms = {"rollout_graph": ours} if args.arm == "ours" else {"rollout_graph": ours, "by_hand": by_hand}
    iters = max(args.iters // 4, 3)
    t = alternate(arms, args.reps, iters)
    g = stats(t["rollout_graph"])
    res = {"case": "knn_rollout", "shape": {"graphs": B, "nodes_per_graph": N, "k": K, "T": T, "layers": 4,
                                            "traj_len": SEG, "capacity": B * N * K},
           "iters_per_rep": iters,
           "model": f"untrained, last layers of coord_net and node_v_net scaled by {DAMP} (both arms)",
           "undamped_rollout": undamped,
           "rollout_graph": g, "rollout_graph_per_rep_ms": t["rollout_graph"]}
    last = ours()[-1]
    res.update({"last_frame_finite": bool(torch.isfinite(last).all()), "last_frame_absmax": float(last.abs().max())})
    if args.arm != "ours":
        r = stats(t["by_hand"])
        a, b = ours(), by_hand()
        torch.cuda.synchronize()
        # (the two arms may break a distance tie differently, after which the trajectories part: the first
        # segment, where both start from the same positions, is the comparable one)
        res.update({"by_hand_cdist_topk": r, "by_hand_per_rep_ms": t["by_hand"],
                    "speedup_over_by_hand": r["median_ms"] / g["median_ms"],
                    "speedup_per_rep": [b_ / a_ for a_, b_ in zip(t["rollout_graph"], t["by_hand"])],
                    "not_slower_on_any_alternation": all(a_ <= b_ for a_, b_ in zip(t["rollout_graph"], t["by_hand"])),
                    "first_segment_maxnorm_rel_vs_by_hand": float((a[:T] - b[:T]).abs().max() / b[:T].abs().max())})
    return res


def case_ragged_rollout(args):
    SIZES, T, K, SEG, DAMP = (250, 500, 750, 1000, 1000, 1250, 1500, 1750), 10, 16, 4, 0.01
    G, n = len(SIZES), sum(SIZES)
    gen = torch.Generator().manual_seed(2)
    parts = []
    for s in SIZES:   # each system at the knn case's density for its own size
        sigma = (s / 5.0) ** (1.0 / 3.0)
        lo, ve = torch.randn(s, 3, generator=gen) * sigma, torch.randn(s, 3, generator=gen)
        parts.append((lo, ve / ve.norm(dim=-1, keepdim=True) * 0.5, (torch.randint(0, 2, (s, 1), generator=gen) * 2 - 1).float()))
    loc, vel, q = (torch.cat([p[i] for p in parts]).to(DEV) for i in range(3))
    off = np.concatenate([[0], np.cumsum(SIZES)])
    t_out = torch.arange(1, T * SEG + 1, device=DEV).unsqueeze(0)   # shared timesteps: one row
    m = model(T, graph="any")
    with torch.no_grad():   # the damped heads of the knn_rollout case: the positions stay bounded over the segments
        for layer in m.layers:
            for head in (layer.coord_net, layer.node_v_net):
                head.mlp[2].weight.mul_(DAMP)
                head.mlp[2].bias.mul_(DAMP)
    batch = graph.RaggedBatch(SIZES, DEV)
    one = [(loc[off[g]:off[g + 1]].reshape(1, SIZES[g], 3).contiguous(), vel[off[g]:off[g + 1]].reshape(1, SIZES[g], 3).contiguous(),
            q[off[g]:off[g + 1]].contiguous()) for g in range(G)]

    def ragged():
        return harness.egno_rollout_graph(m, loc, vel, q, None, None, SEG, k=K, timesteps_out=t_out, sizes=batch)[0]

    def one_by_one():
        return [harness.egno_rollout_graph(m, lo, ve, qq, SIZES[g], 1, SEG, k=K, timesteps_out=t_out)[0]
                for g, (lo, ve, qq) in enumerate(one)]

    # before timing: the batch's positions against each system rolled out alone, segment 1 at 1e-5, later segments
    # at 1e-5 too here (the two arms run the same kernels on the same lists unless a tie breaks differently, which
    # the builder's total order excludes); the figures go into the line
    a, b = ragged(), one_by_one()
    torch.cuda.synchronize()
    parity = []
    for i in range(SEG):
        err = max(float((a[i * T:(i + 1) * T, off[g]:off[g + 1]] - b[g][i * T:(i + 1) * T]).abs().max() /
                        b[g][i * T:(i + 1) * T].abs().max()) for g in range(G))
        parity.append(err)
    if not all(e < 1e-5 for e in parity):
        raise SystemExit(f"ragged_rollout: the batch and the systems rolled out alone differ: {parity}")
    iters = max(args.iters // 4, 3)
    t = alternate({"ragged": ragged, "one_by_one": one_by_one}, args.reps, iters)
    ra, rb = stats(t["ragged"]), stats(t["one_by_one"])
    return {"case": "ragged_rollout", "what": "whole-rollout time (host loop and every launch), not a kernel time",
            "shape": {"sizes": list(SIZES), "n_total": n, "k": K, "T": T, "layers": 4, "traj_len": SEG,
                      "capacity": batch.capacity(K)},
            "iters_per_rep": iters,
            "model": f"untrained, last layers of coord_net and node_v_net scaled by {DAMP} (both arms)",
            "segment_maxnorm_rel_vs_one_by_one": parity,
            "ragged_one_call": ra, "ragged_per_rep_ms": t["ragged"],
            "one_by_one_batch_size_1": rb, "one_by_one_per_rep_ms": t["one_by_one"],
            "speedup_over_one_by_one": rb["median_ms"] / ra["median_ms"],
            "not_slower": ra["median_ms"] <= rb["median_ms"],
            "not_slower_on_any_alternation": all(x <= y for x, y in zip(t["ragged"], t["one_by_one"])),
            "last_frame_absmax": float(a[-1].abs().max())}


def case_knn_rollout_train(args):
    B, N, T, K, SEG, DAMP = 8, 1000, 10, 16, 2, 0.01
    loc, vel, q = synthetic(B, N, 2)
    t_out = torch.arange(1, T * SEG + 1, device=DEV).repeat(B, 1)
    m = model(T, graph="trainable").train()
    with torch.no_grad():   # the damped heads of the knn_rollout case: the positions stay bounded over the segments
        for layer in m.layers:
            for head in (layer.coord_net, layer.node_v_net):
                head.mlp[2].weight.mul_(DAMP)
                head.mlp[2].bias.mul_(DAMP)
    target = loc.reshape(1, B * N, 3) + 0.1

    def ours():
        m.zero_grad(set_to_none=True)
        preds = harness.egno_rollout_train_graph(m, loc, vel, q, N, B, SEG, k=K, timesteps_out=t_out)
        ((preds - target) ** 2).mean().backward()
        return preds

    def compacted():
        m.zero_grad(set_to_none=True)
        x, v = loc, vel
        preds = []
        for i in range(SEG):
            x1, v1 = x.reshape(-1, 3), v.reshape(-1, 3)
            _, _, ea, nodes, _, ng = harness.prepare_inputs_graph(x.detach(), v.detach(), N, q, k=K)
            edges = ng.edge_index()                                   # reads the edge count back
            lm = x.mean(1, keepdim=True).repeat(1, N, 1).reshape(-1, 3)
            xo, vo, _ = m(x1, nodes, edges, ea[:edges[0].numel()], v=v1, loc_mean=lm,
                          timesteps_out=t_out[:, i * T:(i + 1) * T] - i * T)
            preds.append(xo.reshape(T, B * N, 3))
            x, v = xo.reshape(T, B, N, 3)[-1], vo.reshape(T, B, N, 3)[-1]
        preds = torch.cat(preds)
        ((preds - target) ** 2).mean().backward()
        return preds

    arms = {"rollout_train_graph": ours} if args.arm == "ours" else {"rollout_train_graph": ours,
                                                                       "compacted_list": compacted}
    iters = max(args.iters // 4, 3)
    t = alternate(arms, args.reps, iters)
    g = stats(t["rollout_train_graph"])
    res = {"case": "knn_rollout_train", "shape": {"graphs": B, "nodes_per_graph": N, "k": K, "T": T, "layers": 4,
                                                  "traj_len": SEG, "capacity": B * N * K},
           "iters_per_rep": iters,
           "model": f"untrained, last layers of coord_net and node_v_net scaled by {DAMP} (both arms)",
           "rollout_train_graph_fwd_bwd": g, "rollout_train_graph_per_rep_ms": t["rollout_train_graph"]}
    last = ours()[-1].detach()
    res.update({"last_frame_finite": bool(torch.isfinite(last).all()), "last_frame_absmax": float(last.abs().max())})
    if args.arm != "ours":
        r = stats(t["compacted_list"])
        a = ours().detach()
        ga = {k_: p.grad.clone() for k_, p in m.named_parameters() if p.grad is not None}
        b = compacted().detach()
        torch.cuda.synchronize()
        gerr = {k_: float((ga[k_] - p.grad).abs().max() / p.grad.abs().max()) for k_, p in m.named_parameters()
                if p.grad is not None and k_ in ga and float(p.grad.abs().max()) > 0}
        res.update({"compacted_list_fwd_bwd": r, "compacted_list_per_rep_ms": t["compacted_list"],
                    "speedup_over_compacted_list": r["median_ms"] / g["median_ms"],
                    "speedup_per_rep": [b_ / a_ for a_, b_ in zip(t["rollout_train_graph"], t["compacted_list"])],
                    "faster_on_every_alternation": all(a_ < b_ for a_, b_ in zip(t["rollout_train_graph"],
                                                                                 t["compacted_list"])),
                    "preds_maxnorm_rel_vs_compacted_list": float((a - b).abs().max() / b.abs().max()),
                    "worst_grad_maxnorm_rel_vs_compacted_list": max(gerr.values())})
    return res


def case_segno_train(args):
    B, N, T, K = 8, 1000, 10, 16
    torch.manual_seed(0)
    m = pkg.SEGNO(in_node_nf=1, in_edge_nf=2, hidden_nf=64, n_layers=8, recurrent=True, device=DEV, graph="any",
                  trainable=True).train()
    loc, vel, q = synthetic(B, N, 2)
    x, v, ea, nodes, _, ng = harness.prepare_inputs_graph(loc, vel, N, q, k=K, tape=True)
    his = nodes[:, :1].contiguous()
    rows, cols = ng.edge_index()          # (reads the edge count once, outside the timed region: the torch arm's list)
    E = rows.numel()
    ea_list = ea[:E].contiguous()
    target = x + 0.1
    p32 = {k_: t.detach().float().clone().requires_grad_(True) for k_, t in m.state_dict().items()}

    def ours():
        m.zero_grad(set_to_none=True)
        xo, _, _ = m(his, x, ng, v, ea, T=T)
        ((xo - target) ** 2).mean().backward()

    def ref():
        for t in p32.values():
            t.grad = None
        with torch.device(DEV):   # (torch_ref's factory calls take the default device)
            xo, _, _ = tr.segno_forward_step(p32, his, x, rows, cols, v, ea_list, T=T, dense_mean=False)
        ((xo - target) ** 2).mean().backward()

    arms = {"trainable": ours} if args.arm == "ours" else {"trainable": ours, "torch_ref": ref}
    t = alternate(arms, args.reps, max(args.iters // 4, 3))
    g = stats(t["trainable"])
    res = {"case": "segno_train", "shape": {"graphs": B, "nodes_per_graph": N, "k": K, "T": T, "E": E,
                                            "capacity": ng.capacity},
           "trainable_fwd_bwd": g, "trainable_per_rep_ms": t["trainable"],
           "substep_groups": len(autograd.graph_frame_groups(T, ng.capacity)),
           "state_bytes": int(pkg.lib().nonode_segno_graph_train_state_bytes(B * N, T))}
    if args.arm != "ours":
        r = stats(t["torch_ref"])
        ours()
        ref()
        torch.cuda.synchronize()
        gerr = {k_: float((q_.grad - p32[k_].grad).abs().max() / p32[k_].grad.abs().max())
                for k_, q_ in m.named_parameters()
                if q_.grad is not None and p32[k_].grad is not None and float(p32[k_].grad.abs().max()) > 0}
        res.update({"torch_ref_fp32_fwd_bwd": r, "torch_ref_per_rep_ms": t["torch_ref"],
                    "speedup_over_torch_ref": r["median_ms"] / g["median_ms"],
                    "speedup_per_rep": [b_ / a_ for a_, b_ in zip(t["trainable"], t["torch_ref"])],
                    "worst_grad_maxnorm_rel_vs_torch_ref_fp32": max(gerr.values()), "grads_compared": len(gerr)})
    return res


def uniform_cube(B, N, seed):
    """B x N uniform points in a cube whose side grows with N^(1/3) from 10 at N = 1000: with r_cut = 1.5 about
    12 candidates per receiver at every size (11.5 at N = 1000; fewer near the faces)."""
    g = torch.Generator().manual_seed(seed)
    side = 10.0 * (N / 1000.0) ** (1.0 / 3.0)
    return (torch.rand(B * N, 3, generator=g) * side).to(DEV), side


CELLS_SHAPES = ((1, 1000), (1, 4000), (1, 10000), (1, 20000), (1, 50000), (1, 100000), (8, 1000))
CELLS_K, CELLS_RCUT = 16, 1.5


def case_cells(args):
    """The builder alone (graph.neighbor_graph: every launch of one build and its output allocations), method=
    "brute" against method="cells", alternated; one line per shape."""
    out = []
    for B, N in CELLS_SHAPES:
        x, side = uniform_cube(B, N, 7)
        arms = {m: (lambda m=m: graph.neighbor_graph(x, B, N, CELLS_K, CELLS_RCUT, method=m)) for m in ("brute", "cells")}
        a, b = arms["brute"](), arms["cells"]()
        same = all(torch.equal(getattr(a, n), getattr(b, n)) for n in ("row_ptr", "col", "rows", "eid"))
        E = int(a.n_edges.item())
        iters = args.iters if N <= 20000 else max(args.iters // 4, 3)
        t = alternate(arms, args.reps, iters)
        br, ce = stats(t["brute"]), stats(t["cells"])
        out.append({"case": "cells", "shape": {"graphs": B, "nodes_per_graph": N, "k": CELLS_K, "r_cut": CELLS_RCUT,
                                               "cube_side": side, "cells_per_axis": max(g for g in range(1, 700) if 4 * g ** 3 <= max(N, 4))},
                    "iters_per_rep": iters, "mean_degree": E / (B * N), "cells_bitwise_equal_to_brute": same,
                    "brute": br, "cells": ce, "brute_per_rep_ms": t["brute"], "cells_per_rep_ms": t["cells"],
                    "speedup": br["median_ms"] / ce["median_ms"],
                    "cells_faster_on_every_alternation": all(c < b_ for b_, c in zip(t["brute"], t["cells"]))})
    return out


def case_cells_rollout(args):
    """knn_rollout with a cut-off (uniform cube, r_cut = 1.5, k = 16, traj_len = 4, the damped heads), the graph
    rebuilt every segment by either search: harness.egno_rollout_graph(neighbor_method=...), alternated."""
    T, SEG, DAMP = 10, 4, 0.01
    out = []
    for B, N in ((8, 1000), (1, 20000)):
        x, side = uniform_cube(B, N, 9)
        loc = x.reshape(B, N, 3)
        _, vel, q = synthetic(B, N, 2)
        t_out = torch.arange(1, T * SEG + 1, device=DEV).repeat(B, 1)
        m = model(T, graph="any")
        with torch.no_grad():
            for layer in m.layers:
                for head in (layer.coord_net, layer.node_v_net):
                    head.mlp[2].weight.mul_(DAMP)
                    head.mlp[2].bias.mul_(DAMP)
        arms = {meth: (lambda meth=meth: harness.egno_rollout_graph(
            m, loc, vel, q, N, B, SEG, k=CELLS_K, r_cut=CELLS_RCUT, timesteps_out=t_out, neighbor_method=meth)[0])
            for meth in ("brute", "cells")}
        a, b = arms["brute"](), arms["cells"]()
        same = bool(torch.equal(a, b))
        iters = max(args.iters // 4, 3)
        t = alternate(arms, args.reps, iters)
        br, ce = stats(t["brute"]), stats(t["cells"])
        out.append({"case": "cells_rollout", "shape": {"graphs": B, "nodes_per_graph": N, "k": CELLS_K, "r_cut": CELLS_RCUT,
                                                       "cube_side": side, "T": T, "layers": 4, "traj_len": SEG},
                    "iters_per_rep": iters, "model": f"untrained, last layers of coord_net and node_v_net scaled by {DAMP}",
                    "positions_bitwise_equal": same, "last_frame_finite": bool(torch.isfinite(a[-1]).all()),
                    "brute": br, "cells": ce, "brute_per_rep_ms": t["brute"], "cells_per_rep_ms": t["cells"],
                    "speedup": br["median_ms"] / ce["median_ms"],
                    "cells_faster_on_every_alternation": all(c < b_ for b_, c in zip(t["brute"], t["cells"]))})
    return out


KNN_LOOSE_RCUT = 3.6   # about 195 candidates per receiver in the uniform cube (one node per unit volume)


def _knn_cells_line(args, B, N, r_cut, base, label):
    """One line of case knn_cells: the builder alone, method `base` against "knn_cells", alternated."""
    x, side = uniform_cube(B, N, 7)
    arms = {m: (lambda m=m: graph.neighbor_graph(x, B, N, CELLS_K, r_cut, method=m)) for m in (base, "knn_cells")}
    a, b = arms[base](), arms["knn_cells"]()
    same = all(torch.equal(getattr(a, n), getattr(b, n)) for n in ("row_ptr", "col", "rows", "eid"))
    E = int(a.n_edges.item())
    iters = args.iters if N <= 20000 else max(args.iters // 4, 3)
    t = alternate(arms, args.reps, iters)
    ba, kc = stats(t[base]), stats(t["knn_cells"])
    return {"case": "knn_cells", "row": label,
            "shape": {"graphs": B, "nodes_per_graph": N, "k": CELLS_K, "r_cut": r_cut, "cube_side": side,
                      "cells_per_axis": max(g for g in range(1, 700) if 4 * g ** 3 <= max(N, 4))},
            "iters_per_rep": iters, "mean_degree": E / (B * N), "baseline": base, "knn_cells_bitwise_equal_to_baseline": same,
            base: ba, "knn_cells": kc, base + "_per_rep_ms": t[base], "knn_cells_per_rep_ms": t["knn_cells"],
            "speedup": ba["median_ms"] / kc["median_ms"],
            "knn_cells_faster_on_every_alternation": all(c < b_ for b_, c in zip(t[base], t["knn_cells"]))}


def case_knn_cells(args):
    """The builder alone on the pure k-NN graph (k = 16, r_cut=None, the uniform cube of case cells): method="brute"
    against method="knn_cells", one line per shape; then one line under a loose cut-off at 1 x 50,000, where the
    cut-off's own cell search (method="cells") walks a box of some 200 candidates per receiver, against "knn_cells"."""
    out = [_knn_cells_line(args, B, N, None, "brute", "pure k-NN") for B, N in CELLS_SHAPES]
    out.append(_knn_cells_line(args, 1, 50000, KNN_LOOSE_RCUT, "cells", "loose cut-off"))
    return out


def case_knn_cells_rollout(args):
    """cells_rollout without the cut-off at 1 x 20,000 (k = 16, traj_len = 4, the damped heads): the graph rebuilt
    every segment by the brute-force search or by "knn_cells", alternated."""
    T, SEG, DAMP = 10, 4, 0.01
    B, N = 1, 20000
    x, side = uniform_cube(B, N, 9)
    loc = x.reshape(B, N, 3)
    _, vel, q = synthetic(B, N, 2)
    t_out = torch.arange(1, T * SEG + 1, device=DEV).repeat(B, 1)
    m = model(T, graph="any")
    with torch.no_grad():
        for layer in m.layers:
            for head in (layer.coord_net, layer.node_v_net):
                head.mlp[2].weight.mul_(DAMP)
                head.mlp[2].bias.mul_(DAMP)
    arms = {meth: (lambda meth=meth: harness.egno_rollout_graph(
        m, loc, vel, q, N, B, SEG, k=CELLS_K, timesteps_out=t_out, neighbor_method=meth)[0])
        for meth in ("brute", "knn_cells")}
    a, b = arms["brute"](), arms["knn_cells"]()
    same = bool(torch.equal(a, b))
    iters = max(args.iters // 4, 3)
    t = alternate(arms, args.reps, iters)
    br, kc = stats(t["brute"]), stats(t["knn_cells"])
    return {"case": "knn_cells_rollout", "shape": {"graphs": B, "nodes_per_graph": N, "k": CELLS_K, "r_cut": None,
                                                   "cube_side": side, "T": T, "layers": 4, "traj_len": SEG},
            "iters_per_rep": iters, "model": f"untrained, last layers of coord_net and node_v_net scaled by {DAMP}",
            "positions_bitwise_equal": same, "last_frame_finite": bool(torch.isfinite(a[-1]).all()),
            "brute": br, "knn_cells": kc, "brute_per_rep_ms": t["brute"], "knn_cells_per_rep_ms": t["knn_cells"],
            "speedup": br["median_ms"] / kc["median_ms"],
            "knn_cells_faster_on_every_alternation": all(c < b_ for b_, c in zip(t["brute"], t["knn_cells"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="all", choices=["price", "knn", "knn_train", "knn_rollout", "ragged_rollout", "knn_rollout_train", "segno_train",
                                                    "cells", "cells_rollout", "knn_cells", "knn_cells_rollout", "all"])
    ap.add_argument("--arm", default="both", choices=["both", "ours"], help="knn_train, knn_rollout, knn_rollout_train, segno_train: the HIP arm alone")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_graph.py measures on the GPU: no ROCm device found")
    for name, fn in (("price", case_price), ("knn", case_knn), ("knn_train", case_knn_train),
                     ("knn_rollout", case_knn_rollout), ("ragged_rollout", case_ragged_rollout),
                     ("knn_rollout_train", case_knn_rollout_train),
                     ("segno_train", case_segno_train), ("cells", case_cells), ("cells_rollout", case_cells_rollout),
                     ("knn_cells", case_knn_cells), ("knn_cells_rollout", case_knn_cells_rollout)):
        if args.case in (name, "all"):
            res = fn(args)
            for line in res if isinstance(res, list) else [res]:
                line["device"] = torch.cuda.get_device_name(0)
                print(json.dumps(line), flush=True)
    graph.sync_checks()


if __name__ == "__main__":
    main()
