"""GPU counterparts of the reference's hot-path callers.

prepare_inputs / conserved_energy / egno_rollout / segno_rollout keep the reference's argument
meaning and return values (EGNO/main_simulation_simple_no.py:311-384, SEGNO/train_nbody.py:200-236,
utils.py:197-219) but run as HIP kernels (csrc/nonode_rollout.hip): the rollouts are ONE C call
each (segments, re-featurisation and per-frame energies on the device, no host round trip).
Like the models, these have no CPU path: tensors must be on the ROCm device.

General graphs (models built with graph="any"): prepare_inputs_graph featurises on an explicit edge list,
and egno_rollout_graph / segno_rollout_graph chain model(...) segments on a k-NN / cut-off graph rebuilt on
the device from every segment's start (graph.neighbor_graph) or on a fixed list, without a host round trip
(csrc/nonode_neighbor.hip). The functions above stay full-graph. With sizes= (a graph.RaggedBatch or a host
sequence of sizes) prepare_inputs_graph, conserved_energy and the four *_rollout*_graph drivers take graphs of
mixed sizes in one batch, through the same kernels and the same segment loops (_Layout).
"""
import ctypes

import torch

from . import _lib
from .graph import full_edges  # noqa: F401  (re-exported: get_edges counterpart)

ENERGY_KIND = {"charged": 0, "gravity": 1}


def _f32(t):
    return t.detach().to(torch.float32).contiguous() if t is not None else None


def get_edges(batch_size, n_nodes, device="cpu"):
    """NBodyDataset.get_edges (dataset_simple.py:101-111) for the fully connected graph."""
    r, c = full_edges(batch_size, n_nodes, device)
    return [r, c]


def prepare_inputs(loc, vel, edge_attr_o, edges, n_nodes, num_inputs=1, charges=None, t_in=None):
    """main_simulation_simple_no.py:311-339 (nonode_prepare_inputs; num_inputs > 1 per input slot).

    loc, vel: [B, N, 3] (one frame) or [F, B, N, 3] with ``t_in`` [B] choosing frame t_in-1 per
    sample (rollout_fn's loc_all[timesteps_in.T - 1]). edges must be the dataset's fully connected
    list (only its size is used: the kernel indexes pairs implicitly). Returns
    (loc [BN,3], vel [BN,3], edge_attr [E, n_eo+1], nodes [BN, 1(+1)], loc_mean [BN,3]).

    num_inputs == 1 with gradients enabled and a loc or vel that requires grad: the returned loc, vel
    and loc_mean are on the autograd tape (backward: nonode_prepare_inputs_bwd), as in the reference;
    nodes and edge_attr are detached, as the reference detaches them (:333, :338)."""
    if num_inputs == 1 and torch.is_grad_enabled() and (loc.requires_grad or vel.requires_grad):
        x, v, lm, ea, nodes = _PrepareInputs.apply(loc, vel, edge_attr_o, edges, n_nodes, charges, t_in)
        return x, v, ea, nodes, lm
    with torch.no_grad():
        return _prepare_inputs(loc, vel, edge_attr_o, edges, n_nodes, num_inputs, charges, t_in)


def _prepare_inputs(loc, vel, edge_attr_o, edges, n_nodes, num_inputs=1, charges=None, t_in=None):
    """prepare_inputs off the tape (callers hold torch.no_grad())."""
    if num_inputs > 1:
        return _prepare_inputs_multi(loc, vel, edge_attr_o, edges, n_nodes, num_inputs, charges)
    _lib.require_device(loc, vel, edge_attr_o, charges)
    if loc.dim() == 3:
        loc, vel = loc.unsqueeze(0), vel.unsqueeze(0)
    F, B, N = loc.shape[0], loc.shape[1], loc.shape[2]
    if N != n_nodes:
        raise ValueError(f"prepare_inputs: loc has {N} nodes per graph, n_nodes={n_nodes}")
    E = B * N * (N - 1)
    if edges is not None and edges[0].numel() != E:
        raise ValueError("prepare_inputs: edges must be the fully connected list of B graphs")
    eo = _f32(edge_attr_o).reshape(E, -1)
    n_eo = eo.shape[1]
    loc, vel = _f32(loc), _f32(vel)
    q = _f32(charges).reshape(-1) if charges is not None else None
    ti = t_in.reshape(-1).to(torch.int32).contiguous() if t_in is not None else None
    dev = loc.device
    BN = B * N
    x = torch.empty(BN, 3, device=dev)
    v = torch.empty(BN, 3, device=dev)
    nodes = torch.empty(BN, 2 if q is not None else 1, device=dev)
    ea = torch.empty(E, n_eo + 1, device=dev)
    lm = torch.empty(BN, 3, device=dev)
    L = _lib.lib()
    _lib.check(L.nonode_prepare_inputs(B, N, F, _lib.ptr(loc), _lib.ptr(vel), _lib.ptr(ti), _lib.ptr(q), _lib.ptr(eo),
                                       n_eo, _lib.ptr(x), _lib.ptr(v), _lib.ptr(nodes), _lib.ptr(ea), _lib.ptr(lm),
                                       _lib.stream_of(loc)))
    return x, v, ea, nodes, lm


class _PrepareInputs(torch.autograd.Function):
    """prepare_inputs (num_inputs == 1) on the autograd tape for loc and vel: forward the featurisation
    kernel, backward nonode_prepare_inputs_bwd (the selected frame gets g_x + the per-graph mean of
    g_loc_mean and g_v, every other frame zero)."""

    @staticmethod
    def forward(ctx, loc, vel, edge_attr_o, edges, n_nodes, charges, t_in):
        x, v, ea, nodes, lm = _prepare_inputs(loc, vel, edge_attr_o, edges, n_nodes, 1, charges, t_in)
        ctx.shape, ctx.dtypes = tuple(loc.shape), (loc.dtype, vel.dtype)
        ctx.ti = t_in.reshape(-1).to(torch.int32).contiguous() if t_in is not None else None
        ctx.mark_non_differentiable(ea, nodes)
        ctx.set_materialize_grads(False)
        return x, v, lm, ea, nodes

    @staticmethod
    def backward(ctx, gx, gv, glm, _gea, _gnodes):
        batch = getattr(ctx, "batch", None)   # a RaggedBatch (prepare_inputs_graph(sizes=...)): [(F,) n_total, 3]
        lead = 4 if batch is None else 3
        shape = ctx.shape if len(ctx.shape) == lead else (1,) + ctx.shape
        ref = next(g for g in (gx, gv, glm) if g is not None)
        dev = ref.device
        gx, gv, glm = _f32(gx), _f32(gv), _f32(glm)
        g_loc = torch.empty(shape, device=dev) if ctx.needs_input_grad[0] else None
        g_vel = torch.empty(shape, device=dev) if ctx.needs_input_grad[1] else None
        grads = (_lib.ptr(ctx.ti), _lib.ptr(gx), _lib.ptr(gv), _lib.ptr(glm), _lib.ptr(g_loc), _lib.ptr(g_vel),
                 _lib.stream_of(ref))
        if batch is None:
            _lib.check(_lib.lib().nonode_prepare_inputs_bwd(shape[1], shape[2], shape[0], *grads))
        else:
            _lib.check(_lib.lib().nonode_prepare_inputs_bwd_ragged(batch.n_graphs, batch.n_total, shape[0],
                                                                   _lib.ptr(batch.graph_ptr), *grads))
        g_loc = g_loc.reshape(ctx.shape).to(ctx.dtypes[0]) if g_loc is not None else None
        g_vel = g_vel.reshape(ctx.shape).to(ctx.dtypes[1]) if g_vel is not None else None
        return g_loc, g_vel, None, None, None, None, None


def _prepare_inputs_multi(loc, vel, edge_attr_o, edges, n_nodes, num_inputs, charges):
    """main_simulation_simple_no.py:313-327 (num_inputs = I > 1), literally: loc, vel are transposed
    on their first two axes and reshaped to I slots of B*N rows ([B, I, N, 3] from the loader gives
    one slot per input); each slot is featurised like a single input (per-graph mean, |v| (+ q),
    [edge_attr_o, |x_i - x_j|^2]). Returns x, v, loc_mean [I, BN, 3], edge_attr [I, E, n_eo+1],
    nodes [I, BN, 1(+1)]."""
    I = num_inputs
    lt = loc.transpose(0, 1).contiguous().reshape(I, -1, n_nodes, 3)
    vt = vel.transpose(0, 1).contiguous().reshape(I, -1, n_nodes, 3)
    outs = [_prepare_inputs(lt[i], vt[i], edge_attr_o, edges, n_nodes, 1, charges) for i in range(I)]
    x, v, ea, nodes, lm = (torch.stack([o[k] for o in outs]) for k in range(5))
    return x, v, ea, nodes, lm


@torch.no_grad()
def egno_rollout_multi(model, nodes, loc, edges, vel, edge_attr_o, edge_attr, loc_mean, n_nodes, traj_len,
                       batch_size, charges=None, num_steps=10, timesteps_in=None, timesteps_out=None,
                       energy_dataset=None):
    """rollout_fn (main_simulation_simple_no.py:342-384) for num_inputs > 1: per segment the HIP
    forward, then the frames timesteps_in - 1 of each sample become the next inputs and go through
    prepare_inputs exactly as the reference passes them ([I, B, N, 3], which prepare_inputs
    transposes). Returns (loc_preds [traj_len*T, BN, 3], energies, energies_allsteps) like
    egno_rollout."""
    T = model.num_timesteps
    B, N = batch_size, n_nodes
    t_in = timesteps_in if timesteps_in.dim() == 2 else timesteps_in.unsqueeze(-1)
    bidx = torch.arange(B, device=loc.device).unsqueeze(0).expand(t_in.shape[1], -1)
    preds = torch.empty(traj_len * T, B * N, 3, device=loc.device)
    en_all = []
    for i in range(traj_len):
        t_out = timesteps_out[:, i * T:(i + 1) * T] - i * T
        x, v, _ = model(loc, nodes, edges, edge_attr, v=vel, loc_mean=loc_mean, timesteps_out=t_out,
                        timesteps_in=t_in)
        preds[i * T:(i + 1) * T] = x.reshape(T, B * N, 3)
        loc_all, vel_all = x.view(T, B, N, 3), v.view(T, B, N, 3)
        sel = (t_in.T - 1).long()
        loc, vel = loc_all[sel, bidx], vel_all[sel, bidx]
        loc, vel, edge_attr, nodes, loc_mean = prepare_inputs(loc, vel, edge_attr_o, edges, N, t_in.shape[1],
                                                              charges)
        if energy_dataset is not None:
            en_all.append(conserved_energy(energy_dataset, loc_all.reshape(T, B * N, 3),
                                           vel_all.reshape(T, B * N, 3), charges, B))
    if energy_dataset is None:
        return preds, None, None
    en_all = torch.cat(en_all).unsqueeze(-1)
    return preds, en_all[T - 1::T], en_all


@torch.no_grad()
def conserved_energy(dataset, loc, vel, charges, batch_size, *, sizes=None):
    """conserved_energy_fun (utils.py:197-219) on the GPU: loc, vel [..., B*N, 3] (leading frame
    axes allowed), charges (charged) or masses (gravity) [B*N] -> energies [..., B].
    sizes (a graph.RaggedBatch or a host sequence): G graphs of mixed sizes, loc, vel [..., n_total, 3],
    charges [n_total] -> [..., G], each energy over the graph's own nodes; batch_size None or len(sizes)."""
    batch = None
    if sizes is not None:
        from .graph import as_batch
        batch = as_batch(sizes, loc.device)
        if batch_size is not None and batch_size != batch.n_graphs:
            raise ValueError(f"conserved_energy: batch_size = {batch_size} with {batch.n_graphs} sizes")
        if loc.dim() < 2 or loc.shape[-2] != batch.n_total or charges.numel() != batch.n_total:
            raise ValueError(f"conserved_energy: loc must be [..., {batch.n_total}, 3] and charges hold "
                             f"{batch.n_total} values, got {tuple(loc.shape)}, {charges.numel()}")
    _lib.require_device(loc, vel, charges)
    B = batch_size if batch is None else batch.n_graphs
    lead = loc.shape[:-2]
    BN = loc.shape[-2] if loc.dim() >= 2 else loc.numel() // 3
    loc, vel = _f32(loc).reshape(-1, BN, 3), _f32(vel).reshape(-1, BN, 3)
    F, N = loc.shape[0], BN // B
    w = _f32(charges).reshape(-1)
    out = torch.empty(F, B, device=loc.device)
    io = (_lib.ptr(loc), _lib.ptr(vel), _lib.ptr(w), _lib.ptr(out), _lib.stream_of(loc))
    if batch is None:
        _lib.check(_lib.lib().nonode_energy(ENERGY_KIND[dataset], F, B, N, *io))
    else:
        _lib.check(_lib.lib().nonode_energy_ragged(ENERGY_KIND[dataset], F, B, BN, _lib.ptr(batch.graph_ptr), *io))
    return out.reshape(*lead, B) if len(lead) else out.reshape(B)


@torch.no_grad()
def egno_rollout(model, nodes, loc, edges, vel, edge_attr_o, edge_attr, loc_mean, n_nodes, traj_len,
                 batch_size, charges=None, num_steps=10, timesteps_in=None, timesteps_out=None,
                 energy_dataset=None):
    """rollout_fn (main_simulation_simple_no.py:342-384), num_inputs == 1, as one native call.

    Returns (loc_preds [traj_len*T, BN, 3], energies [traj_len, B, 1] or None,
    energies_allsteps [traj_len*T, B, 1] or None). Unlike the reference, ``timesteps_out`` is not
    modified in place (the reference's ``t_out -= i*T`` writes into the caller's tensor)."""
    from .egno import EGNO
    if not isinstance(model, EGNO):
        raise TypeError("egno_rollout drives no_node_comparison_amd.EGNO (its packed weights)")
    if model.num_inputs > 1:
        return egno_rollout_multi(model, nodes, loc, edges, vel, edge_attr_o, edge_attr, loc_mean, n_nodes,
                                  traj_len, batch_size, charges, num_steps, timesteps_in, timesteps_out,
                                  energy_dataset)
    T = model.num_timesteps
    if num_steps != T:
        raise ValueError("rollout_fn reshapes each segment into num_steps == model.num_timesteps frames")
    _lib.require_device(loc, nodes, vel, edge_attr, loc_mean, model.embedding.weight)
    if model.flat:
        # nonode_egno_rollout runs the 64-wide SiLU layer kernels on standard layer blobs only: a flat
        # model (256-wide Tanh blobs, nonode_pack_layer_flat) rolls out segment by segment instead
        return _egno_rollout_segments(model, nodes, loc, edges, vel, edge_attr_o, edge_attr, loc_mean, n_nodes,
                                      traj_len, batch_size, charges, timesteps_in, timesteps_out, energy_dataset)
    B, N = batch_size, n_nodes
    BN, E = B * N, B * N * (N - 1)
    dev = loc.device
    if timesteps_out is None:
        timesteps_out = torch.arange(T * traj_len, device=dev).unsqueeze(0)
    t_all = _f32(timesteps_out)
    if t_all.shape[1] != T * traj_len:
        raise ValueError(f"timesteps_out must have {T * traj_len} columns")
    Bt = t_all.shape[0]
    ti = timesteps_in.reshape(-1).to(torch.int32).contiguous() if timesteps_in is not None else None
    eo = _f32(edge_attr_o).reshape(E, -1)
    q = _f32(charges).reshape(-1) if charges is not None else None
    x, h, v, ef = _f32(loc), _f32(nodes), _f32(vel), _f32(edge_attr)
    lm = _f32(loc_mean) if loc_mean is not None else None   # unused without time convolutions
    blobs, tblobs = model._packed()
    L = _lib.lib()
    P = ctypes.c_void_p * model.n_layers
    blob_p = P(*[blobs[i].data_ptr() for i in range(model.n_layers)])
    tcw_p, tcx_p, _keep = model.tconv_arrays(tblobs)
    ew, eb = _f32(model.embedding.weight), _f32(model.embedding.bias)
    preds = torch.empty(traj_len * T, BN, 3, device=dev)
    en_all = torch.empty(traj_len * T, B, device=dev) if energy_dataset is not None else None
    ws_bytes = L.nonode_egno_rollout_workspace_bytes(B, N, T, Bt, model.in_node_nf, model.in_edge_nf)
    ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.float32, device=dev)
    kind = ENERGY_KIND[energy_dataset] if energy_dataset is not None else -1
    _lib.check(L.nonode_egno_rollout(
        B, N, T, model.n_layers, model.in_node_nf, model.in_edge_nf, model.time_emb_dim, model.num_modes, Bt,
        traj_len, _lib.ptr(x), _lib.ptr(h), _lib.ptr(v), _lib.ptr(lm), _lib.ptr(ef), _lib.ptr(t_all), _lib.ptr(ti),
        _lib.ptr(q), _lib.ptr(eo), eo.shape[1], kind, _lib.ptr(q), _lib.ptr(ew), _lib.ptr(eb), blob_p, tcw_p, tcx_p,
        _lib.ptr(preds), _lib.ptr(en_all), _lib.ptr(ws), ws_bytes, _lib.stream_of(x)))
    if en_all is None:
        return preds, None, None
    en_all = en_all.unsqueeze(-1)
    return preds, en_all[T - 1::T], en_all


def egno_rollout_train(model, nodes, loc, edges, vel, edge_attr_o, edge_attr, loc_mean, n_nodes, traj_len,
                       batch_size, charges=None, num_steps=10, timesteps_in=None, timesteps_out=None):
    """The loop of rollout_fn (main_simulation_simple_no.py:357-371), num_inputs == 1, on the autograd
    tape: per segment model(...), then frame timesteps_in - 1 of each sample (None: the last) through the
    differentiable prepare_inputs, so a loss on the returned loc_preds [traj_len*T, BN, 3] backpropagates
    through every segment to the parameters and to the initial loc, vel, loc_mean (unrolled rollout
    training). nodes and edge_attr are re-featurised detached, as the reference does; no energies.
    Several inputs (num_inputs > 1) are not unrolled: ValueError."""
    from .egno import EGNO
    if not isinstance(model, EGNO):
        raise TypeError("egno_rollout_train drives no_node_comparison_amd.EGNO")
    if model.num_inputs > 1 or (timesteps_in is not None and timesteps_in.dim() == 2 and timesteps_in.shape[1] > 1):
        raise ValueError("egno_rollout_train unrolls the single-input model (num_inputs == 1)")
    T = model.num_timesteps
    if num_steps != T:
        raise ValueError("rollout_fn reshapes each segment into num_steps == model.num_timesteps frames")
    B, N = batch_size, n_nodes
    if timesteps_out is None:
        timesteps_out = torch.arange(T * traj_len, device=loc.device).unsqueeze(0)
    if timesteps_out.shape[1] != T * traj_len:
        raise ValueError(f"timesteps_out must have {T * traj_len} columns")
    ti = timesteps_in.reshape(-1) if timesteps_in is not None else None
    preds = []
    for i in range(traj_len):
        t_out = timesteps_out[:, i * T:(i + 1) * T] - i * T
        x, v, _ = model(loc, nodes, edges, edge_attr, v=vel, loc_mean=loc_mean, timesteps_out=t_out)
        preds.append(x.reshape(T, B * N, 3))
        if i + 1 < traj_len:
            loc, vel, edge_attr, nodes, loc_mean = prepare_inputs(x.reshape(T, B, N, 3), v.reshape(T, B, N, 3),
                                                                  edge_attr_o, edges, N, 1, charges, t_in=ti)
    return torch.cat(preds)


@torch.no_grad()
def _egno_rollout_segments(model, nodes, loc, edges, vel, edge_attr_o, edge_attr, loc_mean, n_nodes, traj_len,
                           batch_size, charges, timesteps_in, timesteps_out, energy_dataset):
    """rollout_fn (main_simulation_simple_no.py:342-384), num_inputs == 1, as a loop of model(...)
    segments: per segment the model's own forward (flat=True: nonode_egno_forward_flat), the frame
    t_in - 1 of each sample re-featurised by prepare_inputs (loc_all[timesteps_in.T - 1]), and the
    per-frame energies. Same returns as egno_rollout."""
    T = model.num_timesteps
    B, N = batch_size, n_nodes
    BN = B * N
    dev = loc.device
    if timesteps_out is None:
        timesteps_out = torch.arange(T * traj_len, device=dev).unsqueeze(0)
    if timesteps_out.shape[1] != T * traj_len:
        raise ValueError(f"timesteps_out must have {T * traj_len} columns")
    ti = timesteps_in.reshape(-1) if timesteps_in is not None else None   # None: the last frame (t_in = T)
    preds = torch.empty(traj_len * T, BN, 3, device=dev)
    en_all = []
    for i in range(traj_len):
        t_out = timesteps_out[:, i * T:(i + 1) * T] - i * T
        x, v, _ = model(loc, nodes, edges, edge_attr, v=vel, loc_mean=loc_mean, timesteps_out=t_out)
        preds[i * T:(i + 1) * T] = x.reshape(T, BN, 3)
        if energy_dataset is not None:
            en_all.append(conserved_energy(energy_dataset, x.reshape(T, BN, 3), v.reshape(T, BN, 3), charges, B))
        loc, vel, edge_attr, nodes, loc_mean = prepare_inputs(x.reshape(T, B, N, 3), v.reshape(T, B, N, 3),
                                                              edge_attr_o, edges, N, 1, charges, t_in=ti)
    if energy_dataset is None:
        return preds, None, None
    en_all = torch.cat(en_all).unsqueeze(-1)
    return preds, en_all[T - 1::T], en_all


@torch.no_grad()
def segno_rollout(model, h, loc, edge_index, vel, edge_attr, traj_len, num_steps=10, charges=None,
                  energy_dataset=None, batch_size=None, in_steps=None):
    """rollout_fn (train_nbody.py:200-236): num_prev == 1 as one native call; several previous
    frames (loc, vel [BN, I, 3], in_steps) as a segment loop over SEGNO's multi-input forward.

    Returns (loc_preds [traj_len, BN, 3], energies [traj_len, B, 1] or None)."""
    from .graph import check_full_graph, finish
    from .segno import SEGNO
    if not isinstance(model, SEGNO):
        raise TypeError("segno_rollout drives no_node_comparison_amd.SEGNO (its packed weights)")
    if model.bug_compat:
        raise ValueError("segno_rollout integrates (bug_compat=True would return the inputs every segment)")
    if loc.dim() == 3:
        return _segno_rollout_multi(model, h, loc, edge_index, vel, edge_attr, traj_len, num_steps, charges,
                                    energy_dataset, in_steps)
    _lib.require_device(loc, h, vel, edge_attr, charges, model.embedding.weight)
    BN = loc.shape[0]
    B, N = check_full_graph(edge_index, BN)
    steps = list(num_steps) if isinstance(num_steps, (list, tuple)) else [int(num_steps)] * traj_len
    if len(steps) != traj_len:
        raise ValueError("num_steps should be a list of length traj_len")
    dev = loc.device
    x, v, his, ea = _f32(loc), _f32(vel), _f32(h), _f32(edge_attr)
    q = _f32(charges).reshape(-1)
    rows, cols = edge_index
    prod = (q[rows.long()] * q[cols.long()]).reshape(-1, 1).contiguous()   # prod_charges (train_nbody.py:203)
    blob = model._packed()
    L = _lib.lib()
    preds = torch.empty(traj_len, BN, 3, device=dev)
    en = torch.empty(traj_len, B, device=dev) if energy_dataset is not None else None
    ws_bytes = L.nonode_segno_rollout_workspace_bytes(B, N, model.in_node_nf, model.in_edge_nf)
    ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.float32, device=dev)
    kind = ENERGY_KIND[energy_dataset] if energy_dataset is not None else -1
    steps_arr = (ctypes.c_int * traj_len)(*[int(s) for s in steps])
    ew, eb = _f32(model.embedding.weight), _f32(model.embedding.bias)
    _lib.check(L.nonode_segno_rollout(
        B, N, model.in_node_nf, model.in_edge_nf, traj_len, steps_arr, _lib.ptr(his), _lib.ptr(x), _lib.ptr(v),
        _lib.ptr(ea), _lib.ptr(prod), 1, kind, _lib.ptr(q), _lib.ptr(ew), _lib.ptr(eb), _lib.ptr(blob),
        float(model.coords_weight), int(bool(model.recurrent)), _lib.ptr(preds), _lib.ptr(en), _lib.ptr(ws), ws_bytes,
        _lib.stream_of(x)))
    finish((preds, en))
    return preds, (en.unsqueeze(-1) if en is not None else None)


@torch.no_grad()
def _segno_rollout_multi(model, h, loc, edge_index, vel, edge_attr, traj_len, num_steps, charges, energy_dataset,
                         in_steps):
    """train_nbody.py:200-236 with num_prev = I > 1: each segment's prediction is appended to the
    window of the last I frames (the oldest dropped), |v| and the last frame's distances are
    recomputed, and in_steps shifts by the segment's substeps (:221-233)."""
    from .graph import check_full_graph
    if in_steps is None:
        raise ValueError("a multi-input SEGNO rollout needs in_steps (train_nbody.py:114)")
    BN = loc.shape[0]
    B, N = check_full_graph(edge_index, BN)
    steps = list(num_steps) if isinstance(num_steps, (list, tuple)) else [int(num_steps)] * traj_len
    if len(steps) != traj_len:
        raise ValueError("num_steps should be a list of length traj_len")
    rows, cols = (t.long() for t in edge_index)
    q = _f32(charges).reshape(-1)
    prod = (q[rows] * q[cols]).reshape(-1, 1)
    preds = torch.empty(traj_len, BN, 3, device=loc.device)
    en = []
    loc, vel = _f32(loc), _f32(vel)
    for i, T in enumerate(steps):
        loc_p, _, vel_p = model(h, loc, edge_index, vel, edge_attr, T=T, in_steps=in_steps)
        if energy_dataset is not None:
            en.append(conserved_energy(energy_dataset, loc_p, vel_p, charges, B))
        preds[i] = loc_p
        loc = torch.cat((loc[:, 1:, :], loc_p.unsqueeze(1)), dim=1)
        vel = torch.cat((vel[:, 1:, :], vel_p.unsqueeze(1)), dim=1)
        h = torch.sqrt(torch.sum(vel ** 2, dim=-1)).unsqueeze(-1)
        loc_dist = torch.sum((loc[rows, -1, :] - loc[cols, -1, :]) ** 2, 1).unsqueeze(1)
        st = in_steps.tolist() if torch.is_tensor(in_steps) else list(in_steps)
        in_steps = torch.tensor(st[1:] + [T], device=loc.device) - T
        edge_attr = torch.cat([prod, loc_dist], 1)
    return preds, (torch.stack(en).unsqueeze(-1) if en else None)


# ---- general graphs: featurisation on an explicit list, rollouts on k-NN / cut-off graphs ----

def _graph_source(k, r_cut, edges, who, neighbor_method=None):
    if (k is None) == (edges is None):
        raise ValueError(f"{who}: give exactly one of k (a neighbour graph built from the positions, with an "
                         "optional r_cut) and edges (a fixed list)")
    if edges is not None and r_cut is not None:
        raise ValueError(f"{who}: r_cut goes with k (a fixed edge list has no cut-off)")
    if edges is not None and neighbor_method is not None:
        raise ValueError(f"{who}: neighbor_method goes with k (a fixed edge list is not searched for)")
    if k is not None:
        from . import graph as _graph
        _graph.neighbor_args(k, r_cut)
        _graph.neighbor_method(neighbor_method, r_cut)


def prepare_inputs_graph(loc, vel, n_nodes, charges=None, t_in=None, *, k=None, r_cut=None, edges=None, tape=False,
                         sizes=None, neighbor_method=None):
    """prepare_inputs (main_simulation_simple_no.py:311-339, num_inputs == 1) on an explicit edge list
    instead of the implicit fully connected one. loc, vel: [B, N, 3] or [F, B, N, 3] with t_in [B] choosing
    frame t_in - 1 per sample (a python index taken modulo F on the device, as nonode_prepare_inputs takes it:
    0 is the last frame, and a value past F wraps where python would raise). The graph is either built from the SELECTED positions (k, optional r_cut:
    graph.neighbor_graph) or given (edges: any [rows, cols] list or a NeighborGraph). Returns
    (x [BN, 3], v [BN, 3], edge_attr, nodes [BN, 1(+1)], loc_mean [BN, 3], edges) with edge_attr[e] =
    [q_r q_c, |x_r - x_c|^2] ([|x_r - x_c|^2] without charges), one row per entry of the list; for a
    NeighborGraph that is [capacity, .] with the rows at or past its device-side edge count zero.
    Two launches (nonode_prepare_nodes, nonode_edge_features) besides the builder's; memory is
    O(BN + len(list)) and nothing is read back to the host. Off the autograd tape by default.

    tape=True (training on the graph): a graph built here (k) carries its CSR by sender
    (graph.neighbor_graph(by_sender=True)), and with gradients enabled and a loc or vel that requires grad
    the returned x, v and loc_mean are on the autograd tape (backward: nonode_prepare_inputs_bwd, as
    prepare_inputs' own: the selected frame gets g_x + the per-graph mean of g_loc_mean, and g_v; every
    other frame zero). nodes, edge_attr and the graph are not differentiable: the reference detaches the
    first two (main_simulation_simple_no.py:333,338), and the choice of neighbours is discrete, built from
    the detached positions, so no gradient flows through it.

    sizes (a graph.RaggedBatch, or a host sequence of sizes, wrapped; n_nodes must then be None): G graphs of
    mixed sizes. loc, vel [n_total, 3] or [F, n_total, 3], t_in one value per graph, charges n_total values;
    the mean is each graph's own, k builds through graph.neighbor_graph_ragged, and the tape's reverse is
    nonode_prepare_inputs_bwd_ragged. Same returns.

    neighbor_method (with k only): the search that builds the graph, graph.neighbor_graph's method= (None /
    "brute", "cells" under a finite r_cut, "auto"; "knn_cells" / "knn_auto" for any r_cut, None included): the same
    graph bit for bit, built faster on large graphs."""
    _graph_source(k, r_cut, edges, "prepare_inputs_graph", neighbor_method)
    batch = None
    if sizes is not None:
        if n_nodes is not None:
            raise ValueError("prepare_inputs_graph: give n_nodes (equal sizes) or sizes (mixed sizes), not both")
        from .graph import as_batch
        batch = as_batch(sizes, loc.device)
    if tape and torch.is_grad_enabled() and (loc.requires_grad or vel.requires_grad):
        box = []
        x, v, lm, ea, nodes = _PrepareInputsGraph.apply(loc, vel, n_nodes, charges, t_in, k, r_cut, edges, box, batch,
                                                        neighbor_method)
        return x, v, ea, nodes, lm, box[0]
    with torch.no_grad():
        return _prepare_inputs_graph(loc, vel, n_nodes, charges, t_in, k, r_cut, edges, bool(tape), batch,
                                     neighbor_method)


class _PrepareInputsGraph(torch.autograd.Function):
    """prepare_inputs_graph on the autograd tape for loc and vel: _PrepareInputs with the featurisation on an
    explicit list. The graph (not a tensor) leaves through `box`."""

    @staticmethod
    def forward(ctx, loc, vel, n_nodes, charges, t_in, k, r_cut, edges, box, batch, method=None):
        x, v, ea, nodes, lm, g = _prepare_inputs_graph(loc, vel, n_nodes, charges, t_in, k, r_cut, edges, True, batch,
                                                       method)
        box.append(g)
        ctx.batch = batch
        ctx.shape, ctx.dtypes = tuple(loc.shape), (loc.dtype, vel.dtype)
        ctx.ti = t_in.reshape(-1).to(torch.int32).contiguous() if t_in is not None else None
        ctx.mark_non_differentiable(ea, nodes)
        ctx.set_materialize_grads(False)
        return x, v, lm, ea, nodes

    @staticmethod
    def backward(ctx, gx, gv, glm, _gea, _gnodes):
        return _PrepareInputs.backward(ctx, gx, gv, glm, _gea, _gnodes) + (None, None, None, None)


def _prepare_inputs_graph(loc, vel, n_nodes, charges, t_in, k, r_cut, edges, by_sender, batch=None, method=None):
    """prepare_inputs_graph off the tape (callers hold torch.no_grad()). batch: a RaggedBatch or None."""
    from . import graph as _graph
    _graph_source(k, r_cut, edges, "prepare_inputs_graph", method)
    if batch is None:
        if loc.dim() not in (3, 4) or loc.shape != vel.shape or loc.shape[-1] != 3:
            raise ValueError(f"prepare_inputs_graph: loc, vel must be [B, N, 3] or [F, B, N, 3] alike, got "
                             f"{tuple(loc.shape)}, {tuple(vel.shape)}")
        if loc.dim() == 3:
            loc, vel = loc.unsqueeze(0), vel.unsqueeze(0)
        F, B, N = loc.shape[0], loc.shape[1], loc.shape[2]
        if N != n_nodes:
            raise ValueError(f"prepare_inputs_graph: loc has {N} nodes per graph, n_nodes={n_nodes}")
        BN = B * N
    else:
        B, BN = batch.n_graphs, batch.n_total
        if loc.dim() not in (2, 3) or loc.shape != vel.shape or tuple(loc.shape[-2:]) != (BN, 3):
            raise ValueError(f"prepare_inputs_graph: with sizes, loc, vel must be [{BN}, 3] or [F, {BN}, 3] alike, "
                             f"got {tuple(loc.shape)}, {tuple(vel.shape)}")
        if loc.dim() == 2:
            loc, vel = loc.unsqueeze(0), vel.unsqueeze(0)
        F = loc.shape[0]
    if charges is not None and charges.numel() != BN:
        raise ValueError(f"prepare_inputs_graph: charges must hold {BN} values, got {charges.numel()}")
    if t_in is not None and t_in.numel() != B:
        raise ValueError(f"prepare_inputs_graph: t_in must hold one value per sample ({B}), got {t_in.numel()}")
    if edges is not None:
        rows, cols = _graph._split(edges)
        if rows.dim() != 1 or rows.shape != cols.shape or rows.dtype != cols.dtype or \
                rows.dtype not in (torch.int32, torch.int64):
            raise ValueError("prepare_inputs_graph: edges must be two 1-D int32 or int64 tensors of one length")
    _lib.require_device(loc, vel, charges, t_in, *(() if edges is None else (rows, cols)))
    loc, vel = _f32(loc), _f32(vel)
    q = _f32(charges).reshape(-1) if charges is not None else None
    ti = t_in.reshape(-1).to(torch.int32).contiguous() if t_in is not None else None
    dev = loc.device
    x = torch.empty(BN, 3, device=dev)
    v = torch.empty(BN, 3, device=dev)
    nodes = torch.empty(BN, 2 if q is not None else 1, device=dev)
    lm = torch.empty(BN, 3, device=dev)
    L = _lib.lib()
    s = _lib.stream_of(loc)
    io = (_lib.ptr(loc), _lib.ptr(vel), _lib.ptr(ti), _lib.ptr(q), _lib.ptr(x), _lib.ptr(v), _lib.ptr(nodes),
          _lib.ptr(lm), s)
    if batch is None:
        _lib.check(L.nonode_prepare_nodes(B, N, F, *io))
    else:
        _lib.check(L.nonode_prepare_nodes_ragged(B, BN, F, _lib.ptr(batch.graph_ptr), *io))
    if edges is None:
        edges = (_graph.neighbor_graph(x, B, N, k, r_cut, by_sender=by_sender, method=method) if batch is None else
                 _graph.neighbor_graph_ragged(x, batch, k, r_cut, by_sender=by_sender, method=method))
        rows, cols = edges.rows, edges.col
    n_edges = edges.n_edges if isinstance(edges, _graph.NeighborGraph) else None
    rows, cols = rows.contiguous(), cols.contiguous()
    ea = torch.empty(rows.numel(), 2 if q is not None else 1, device=dev)
    _lib.check(L.nonode_edge_features(rows.numel(), BN, _lib.ptr(rows), _lib.ptr(cols), rows.element_size(),
                                      _lib.ptr(n_edges), _lib.ptr(x), _lib.ptr(q), _lib.ptr(ea), s))
    return x, v, ea, nodes, lm, edges


def _general_model(model, cls, who):
    if not isinstance(model, cls):
        raise TypeError(f"{who} drives no_node_comparison_amd.{cls.__name__} (its packed weights)")
    if model.graph not in ("any", "trainable"):
        raise ValueError(f'{who} needs a model built with graph="any" (or "trainable"), got graph={model.graph!r}: '
                         "the full-graph drivers take the fully connected list")


class _Layout:
    """How a driver's n_total rows split into graphs: B graphs of N rows (batch None), or the graphs of a
    graph.RaggedBatch (sizes=; N None). The one thing in which the equal-size and the mixed-size call of a
    driver differ: its segment loop asks this object for the views and passes it on."""

    def __init__(self, who, loc, n_nodes, batch_size, sizes):
        if sizes is None:
            self.batch, self.B, self.N = None, int(batch_size), n_nodes
            self.n_total = self.B * self.N if n_nodes is not None else None
            return
        from .graph import as_batch
        self.batch = as_batch(sizes, loc.device)
        self.B, self.N, self.n_total = self.batch.n_graphs, None, self.batch.n_total
        if batch_size is not None and batch_size != self.B:
            raise ValueError(f"{who}: batch_size = {batch_size} with {self.B} sizes (leave it None with sizes)")
        if n_nodes is not None and any(s != n_nodes for s in self.batch.sizes):
            raise ValueError(f"{who}: n_nodes = {n_nodes} with sizes {self.batch.sizes!r} (leave it None with sizes)")

    def first(self, who, loc, vel):
        """The shape check of the driver's loc, vel: [B, N, 3] (EGNO, equal sizes) or [n_total, 3]."""
        want = (self.B, self.N, 3) if self.batch is None else (self.n_total, 3)
        if tuple(loc.shape) != want or loc.shape != vel.shape:
            raise ValueError(f"{who}: loc, vel must be [{', '.join(map(str, want))}], got {tuple(loc.shape)}, "
                             f"{tuple(vel.shape)}")

    def shared_timesteps(self, who, timesteps_out):
        if self.batch is not None and timesteps_out is not None and timesteps_out.dim() == 2 and \
                timesteps_out.shape[0] > 1:
            raise ValueError(f"{who}: a batch of mixed sizes takes shared timesteps only (timesteps_out with one "
                             f"row, got {timesteps_out.shape[0]}): the embedding maps rows to nodes by equal division")

    def frames(self, t, T=None):
        """t [(T) n_total, 3] as prepare_inputs_graph takes it: [(T,) B, N, 3] or [(T,) n_total, 3]."""
        lead = () if T is None else (T,)
        return t.reshape(*lead, self.B, self.N, 3) if self.batch is None else t.reshape(*lead, self.n_total, 3)

    def prepare(self, loc, vel, charges, t_in=None, **kw):
        return prepare_inputs_graph(loc, vel, self.N, charges, t_in, sizes=self.batch, **kw)

    def energy(self, dataset, x, v, charges):
        return conserved_energy(dataset, x, v, charges, self.B, sizes=self.batch)


def _segno_layout(who, loc, vel, batch_size, sizes):
    """The _Layout of a SEGNO driver's loc, vel [n_total, 3] after their shape check: batch_size graphs of
    n_total / batch_size rows, or the graphs of sizes."""
    if sizes is not None:
        lay = _Layout(who, loc, None, batch_size, sizes)
        lay.first(who, loc, vel)
        return lay
    B = int(batch_size)
    if loc.dim() != 2 or loc.shape[1] != 3 or loc.shape != vel.shape or B < 1 or loc.shape[0] % B:
        raise ValueError(f"{who}: loc, vel must be [BN, 3] with BN a multiple of batch_size={B}, got "
                         f"{tuple(loc.shape)}, {tuple(vel.shape)}")
    return _Layout(who, loc, loc.shape[0] // B, B, None)


@torch.no_grad()
def egno_rollout_graph(model, loc, vel, charges, n_nodes, batch_size, traj_len, *, k=None, r_cut=None, edges=None,
                       timesteps_in=None, timesteps_out=None, energy_dataset=None, return_graphs=False, sizes=None,
                       neighbor_method=None):
    """rollout_fn (main_simulation_simple_no.py:342-384), num_inputs == 1, on a general graph, as a loop of
    model(...) segments like _egno_rollout_segments. loc, vel [B, N, 3]. Per segment: prepare_inputs_graph
    on the current frame (k: the neighbour graph is rebuilt from that frame on the device; edges: the
    topology is fixed and only the features are recomputed), the forward, frame timesteps_in - 1 of each
    sample (None: the last) as the next input, conserved_energy per frame if asked. Nothing in the loop
    reads the device. Returns (loc_preds [traj_len*T, BN, 3], energies, energies_allsteps) as egno_rollout
    does, and with return_graphs=True also the list of the segments' graphs.
    sizes (a graph.RaggedBatch or a host sequence; n_nodes and batch_size None): G graphs of mixed sizes in
    the one loop. loc, vel [n_total, 3], timesteps_in [G], timesteps_out shared (one row); loc_preds
    [traj_len*T, n_total, 3], energies [.., G, 1].
    neighbor_method (with k): the search behind every segment's graph, as in prepare_inputs_graph ("knn_cells" /
    "knn_auto" also without a cut-off, the drivers' default graph)."""
    from .egno import EGNO
    _general_model(model, EGNO, "egno_rollout_graph")
    if model.num_inputs > 1:
        raise NotImplementedError("egno_rollout_graph rolls the single-input model out (num_inputs == 1)")
    if model.flat:
        raise NotImplementedError("egno_rollout_graph does not run with flat=True (general graphs)")
    _graph_source(k, r_cut, edges, "egno_rollout_graph", neighbor_method)
    T = model.num_timesteps
    lay = _Layout("egno_rollout_graph", loc, n_nodes, batch_size, sizes)
    lay.first("egno_rollout_graph", loc, vel)
    lay.shared_timesteps("egno_rollout_graph", timesteps_out)
    B, BN = lay.B, lay.n_total
    if timesteps_in is not None and timesteps_in.numel() != B:
        raise ValueError(f"egno_rollout_graph: timesteps_in must hold one value per sample ({B}), got "
                         f"{timesteps_in.numel()}")
    _lib.require_device(loc, vel, charges, model.embedding.weight)
    dev = loc.device
    if timesteps_out is None:
        timesteps_out = torch.arange(T * traj_len, device=dev).unsqueeze(0)
    if timesteps_out.shape[1] != T * traj_len:
        raise ValueError(f"timesteps_out must have {T * traj_len} columns")
    ti = timesteps_in.reshape(-1) if timesteps_in is not None else None   # None: the last frame (t_in = T)
    preds = torch.empty(traj_len * T, BN, 3, device=dev)
    en_all, graphs = [], []
    x, v, edge_attr, nodes, loc_mean, g = lay.prepare(loc, vel, charges, k=k, r_cut=r_cut, edges=edges,
                                                      neighbor_method=neighbor_method)
    for i in range(traj_len):
        graphs.append(g)
        t_out = timesteps_out[:, i * T:(i + 1) * T] - i * T
        x, v, _ = model(x, nodes, g, edge_attr, v=v, loc_mean=loc_mean, timesteps_out=t_out)
        preds[i * T:(i + 1) * T] = x.reshape(T, BN, 3)
        if energy_dataset is not None:
            en_all.append(lay.energy(energy_dataset, x.reshape(T, BN, 3), v.reshape(T, BN, 3), charges))
        if i + 1 < traj_len:
            x, v, edge_attr, nodes, loc_mean, g = lay.prepare(lay.frames(x, T), lay.frames(v, T), charges, ti, k=k,
                                                              r_cut=r_cut, edges=edges,
                                                              neighbor_method=neighbor_method)
    tail = (graphs,) if return_graphs else ()
    if energy_dataset is None:
        return (preds, None, None) + tail
    en_all = torch.cat(en_all).unsqueeze(-1)
    return (preds, en_all[T - 1::T], en_all) + tail


def egno_rollout_train_graph(model, loc, vel, charges, n_nodes, batch_size, traj_len, *, k=None, r_cut=None,
                             edges=None, timesteps_in=None, timesteps_out=None, return_graphs=False, sizes=None,
                             neighbor_method=None):
    """The loop of egno_rollout_graph on the autograd tape (unrolled rollout training on a general graph),
    num_inputs == 1, for a model built with graph="trainable". loc, vel [B, N, 3]. Per segment:
    prepare_inputs_graph(tape=True) on the selected frame (k: the neighbour graph, with its CSR by sender, is
    rebuilt on the device from that frame's detached positions; edges: the list is fixed), then model(...).
    Returns loc_preds [traj_len*T, BN, 3] with a grad_fn (and with return_graphs=True also the list of the
    segments' graphs): a loss on it backpropagates through every segment to the parameters and to the
    initial loc and vel. No gradient flows through the choice of neighbours (it is discrete) or through
    nodes / edge_attr (detached, as the reference does at main_simulation_simple_no.py:333,338). No
    energies. Nothing in the loop or in the backward reads the device.
    sizes: G graphs of mixed sizes, as in egno_rollout_graph (loc, vel [n_total, 3], timesteps_in [G], shared
    timesteps_out; the per-graph mean and its reverse are each graph's own). neighbor_method as there ("knn_cells" /
    "knn_auto" included)."""
    from . import graph as _graph
    from .egno import EGNO
    who = "egno_rollout_train_graph"
    if not isinstance(model, EGNO):
        raise TypeError(f"{who} drives no_node_comparison_amd.EGNO (its packed weights)")
    if model.graph != "trainable":
        raise ValueError(f'{who} needs a model built with graph="trainable", got graph={model.graph!r}')
    if model.num_inputs > 1:
        raise NotImplementedError(f"{who} unrolls the single-input model (num_inputs == 1)")
    if model.flat:
        raise NotImplementedError(f"{who} does not run with flat=True (general graphs)")
    _graph_source(k, r_cut, edges, who, neighbor_method)
    T = model.num_timesteps
    lay = _Layout(who, loc, n_nodes, batch_size, sizes)
    lay.first(who, loc, vel)
    lay.shared_timesteps(who, timesteps_out)
    B, BN = lay.B, lay.n_total
    if timesteps_in is not None and timesteps_in.numel() != B:
        raise ValueError(f"{who}: timesteps_in must hold one value per sample ({B}), got {timesteps_in.numel()}")
    _lib.require_device(loc, vel, charges, model.embedding.weight)
    if timesteps_out is None:
        timesteps_out = torch.arange(T * traj_len, device=loc.device).unsqueeze(0)
    if timesteps_out.shape[1] != T * traj_len:
        raise ValueError(f"timesteps_out must have {T * traj_len} columns")
    ti = timesteps_in.reshape(-1) if timesteps_in is not None else None   # None: the last frame (t_in = T)
    if isinstance(edges, _graph.NeighborGraph):
        edges = edges.with_sender_csr()   # (a graph that came out of a rollout)
    preds, graphs = [], []
    x, v, t_in = loc, vel, None
    for i in range(traj_len):
        x, v, edge_attr, nodes, loc_mean, g = lay.prepare(x, v, charges, t_in, k=k, r_cut=r_cut, edges=edges, tape=True,
                                                          neighbor_method=neighbor_method)
        graphs.append(g)
        t_out = timesteps_out[:, i * T:(i + 1) * T] - i * T
        x, v, _ = model(x, nodes, g, edge_attr, v=v, loc_mean=loc_mean, timesteps_out=t_out)
        preds.append(x.reshape(T, BN, 3))
        x, v, t_in = lay.frames(x, T), lay.frames(v, T), ti
    preds = torch.cat(preds)
    return (preds, graphs) if return_graphs else preds


@torch.no_grad()
def segno_rollout_graph(model, loc, vel, charges, batch_size, traj_len, num_steps=10, *, k=None, r_cut=None,
                        edges=None, energy_dataset=None, return_graphs=False, sizes=None, neighbor_method=None):
    """rollout_fn (train_nbody.py:200-236), num_prev == 1, on a general graph, as a loop of model(...)
    segments. loc, vel [BN, 3]; his = |v|; num_steps an int or a list of length traj_len. The graph (k:
    rebuilt on the device; edges: fixed) and the edge attributes [q_r q_c, |x_r - x_c|^2] come from each
    segment's start and stay frozen over its substeps, as in nonode_segno_forward_step_graph. Nothing in
    the loop reads the device. Returns (loc_preds [traj_len, BN, 3], energies [traj_len, B, 1] or None), and
    with return_graphs=True also the list of the segments' graphs.
    sizes (a graph.RaggedBatch or a host sequence; batch_size None or len(sizes)): G graphs of mixed sizes in
    the one loop. loc, vel [n_total, 3]; energies [traj_len, G, 1].
    neighbor_method (with k): the search behind every segment's graph, as in prepare_inputs_graph ("knn_cells" /
    "knn_auto" also without a cut-off, the drivers' default graph)."""
    from .segno import SEGNO
    _general_model(model, SEGNO, "segno_rollout_graph")
    if model.bug_compat:
        raise ValueError("segno_rollout_graph integrates (bug_compat=True would return the inputs every segment)")
    _graph_source(k, r_cut, edges, "segno_rollout_graph", neighbor_method)
    lay = _segno_layout("segno_rollout_graph", loc, vel, batch_size, sizes)
    steps = list(num_steps) if isinstance(num_steps, (list, tuple)) else [int(num_steps)] * traj_len
    if len(steps) != traj_len:
        raise ValueError("num_steps should be a list of length traj_len")
    _lib.require_device(loc, vel, charges, model.embedding.weight)
    preds = torch.empty(traj_len, lay.n_total, 3, device=loc.device)
    en, graphs = [], []
    x, v = loc, vel
    for i, T in enumerate(steps):
        x, v, edge_attr, nodes, _, g = lay.prepare(lay.frames(x), lay.frames(v), charges, k=k, r_cut=r_cut, edges=edges,
                                                   neighbor_method=neighbor_method)
        graphs.append(g)
        x, _, v = model(nodes[:, :1], x, g, v, edge_attr, T=int(T))
        preds[i] = x
        if energy_dataset is not None:
            en.append(lay.energy(energy_dataset, x, v, charges))
    tail = (graphs,) if return_graphs else ()
    return (preds, (torch.stack(en).unsqueeze(-1) if en else None)) + tail


def segno_rollout_train_graph(model, loc, vel, charges, batch_size, traj_len, num_steps=10, *, k=None, r_cut=None,
                              edges=None, return_graphs=False, sizes=None, neighbor_method=None):
    """The loop of segno_rollout_graph on the autograd tape (unrolled rollout training on a general graph),
    num_prev == 1, for a model built with graph="any", trainable=True. loc, vel [BN, 3]; num_steps an int or a
    list of length traj_len. Per segment: prepare_inputs_graph(tape=True) on the previous segment's predicted
    x, v (k: the neighbour graph, with its CSR by sender, is rebuilt on the device from the detached positions;
    edges: the list is fixed), then model(...). Returns loc_preds [traj_len, BN, 3] with a grad_fn (and with
    return_graphs=True also the list of the segments' graphs): a loss on it backpropagates through every segment
    to the parameters and to the initial loc and vel. No gradient flows through the choice of neighbours (it is
    discrete) or through his = |v| and edge_attr (detached: the reference builds them from data,
    train_nbody.py:121-123,230-233, as egno_rollout_train_graph does). No energies. Nothing in the loop or in
    the backward reads the device. sizes: G graphs of mixed sizes, and neighbor_method ("knn_cells" / "knn_auto"
    included), as in segno_rollout_graph."""
    from . import graph as _graph
    from .segno import SEGNO
    who = "segno_rollout_train_graph"
    if not isinstance(model, SEGNO):
        raise TypeError(f"{who} drives no_node_comparison_amd.SEGNO (its packed weights)")
    if model.graph != "any" or not model.trainable:
        raise ValueError(f'{who} needs a model built with graph="any", trainable=True, got graph={model.graph!r}, '
                         f"trainable={model.trainable!r}")
    if model.bug_compat:
        raise ValueError(f"{who} integrates (bug_compat=True would return the inputs every segment)")
    _graph_source(k, r_cut, edges, who, neighbor_method)
    lay = _segno_layout(who, loc, vel, batch_size, sizes)
    steps = list(num_steps) if isinstance(num_steps, (list, tuple)) else [int(num_steps)] * traj_len
    if len(steps) != traj_len:
        raise ValueError("num_steps should be a list of length traj_len")
    _lib.require_device(loc, vel, charges, model.embedding.weight)
    if isinstance(edges, _graph.NeighborGraph):
        edges = edges.with_sender_csr()   # (a graph that came out of a rollout)
    preds, graphs = [], []
    x, v = loc, vel
    for T in steps:
        x, v, edge_attr, nodes, _, g = lay.prepare(lay.frames(x), lay.frames(v), charges, k=k, r_cut=r_cut,
                                                   edges=edges, tape=True, neighbor_method=neighbor_method)
        graphs.append(g)
        x, _, v = model(nodes[:, :1].detach(), x, g, v, edge_attr.detach(), T=int(T))
        preds.append(x)
    preds = torch.stack(preds)
    return (preds, graphs) if return_graphs else preds
