"""Training entry for EGNO: loss.backward() of run_epoch (main_simulation_simple_no.py:267-280).

EGNOTrain is a torch.autograd.Function around the C ABI: its forward runs
nonode_egno_forward_train (same kernels and outputs as the inference forward, plus the saved
state), its backward runs nonode_egno_backward and returns the gradient of every parameter. The
reference's training loop (criterion, loss.backward(), optimizer.step()) runs unchanged on top.
Where x, v, h or loc_mean requires grad, the backward runs nonode_egno_backward_inputs instead (the
same launches plus the input-gradient kernels) and returns those gradients too, as the reference's
plain-torch forward does; edge_fea gets none (EGNO.forward refuses an edge_fea that requires grad).
"""
import ctypes

import torch

from . import _lib


_f32 = _lib.f32


class EGNOTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, x, h, edge_fea, v, loc_mean, t_out, t_in, B, N, slots, *params):
        # t_in is None for a single input; else the inputs are per frame (num_inputs > 1) and t_in
        # [Bt, T] is each frame's input time (nonode_egno_forward_train_frames)
        # slots (multi-input, EGNO._forward_multi): x, h, v, loc_mean are the caller's [I, BN, .] tensors
        # (the tape's inputs, so their gradients come back per slot) and slots = (frame -> slot map,
        # (x, h, v, loc_mean) spread to the frames [T*BN, .]), which the kernels read
        L = _lib.lib()
        T = model.num_timesteps
        dev = x.device
        ctx.in_dtypes = tuple(t.dtype if t is not None else None for t in (x, h, v, loc_mean))
        ctx.in_shapes = tuple(t.shape if t is not None else None for t in (x, h, v, loc_mean))
        if slots is not None:
            ctx.frame_input, (x, h, v, loc_mean) = list(slots[0]), slots[1]
            ctx.n_inputs = ctx.in_shapes[0][0]
        else:   # one input, or (t_in without slots) one input per frame
            ctx.n_inputs = 1 if t_in is None else T
            ctx.frame_input = [0] * T if t_in is None else list(range(T))
        x, h, v, ef = _f32(x), _f32(h), _f32(v), _f32(edge_fea)
        tt = model._t_out_f32(t_out)   # cached per tensor / version: no int64 -> f32 copy per step
        lm = _f32(loc_mean)   # None: unused without time convolutions
        emb_cols = model.time_emb_dim * (1 if t_in is None else 2)
        Bt = tt.shape[0]
        blobs, tblobs = model._packed()
        ws_bytes = L.nonode_egno_workspace_bytes(B, N, T, Bt)
        x_out, v_out, h_out, ws = _lib.alloc_outputs(T * B * N, model.hidden_nf, ws_bytes, dev)
        st_bytes = L.nonode_egno_train_state_bytes(B, N, T, model.n_layers, model.in_node_nf, emb_cols)
        state = torch.empty((st_bytes + 3) // 4, dtype=torch.float32, device=dev)
        P = ctypes.c_void_p * model.n_layers
        tcw_p, tcx_p, _keep = model.tconv_arrays(tblobs)
        ew, eb = _f32(model.embedding.weight), _f32(model.embedding.bias)
        head = (B, N, T, model.n_layers, model.in_node_nf, model.in_edge_nf, model.time_emb_dim, model.num_modes, Bt,
                _lib.ptr(x), _lib.ptr(h), _lib.ptr(v), _lib.ptr(lm), _lib.ptr(ef))
        tail = (_lib.ptr(ew), _lib.ptr(eb), P(*[blobs[i].data_ptr() for i in range(model.n_layers)]), tcw_p, tcx_p,
                _lib.ptr(x_out), _lib.ptr(v_out), _lib.ptr(h_out), _lib.ptr(state), st_bytes, _lib.ptr(ws), ws_bytes,
                _lib.stream_of(x))
        if t_in is None:
            _lib.check(L.nonode_egno_forward_train(*head, _lib.ptr(tt), *tail))
        else:
            ti = _f32(t_in)
            _lib.check(L.nonode_egno_forward_train_frames(*head, _lib.ptr(ti), _lib.ptr(tt), *tail))
        ctx.frames = t_in is not None
        # outputs the loss does not use (v, h for the reference's loss on x) arrive as None rather
        # than as zero-filled tensors: the library zeroes its own output-gradient buffers for them
        ctx.set_materialize_grads(False)
        ctx.model, ctx.B, ctx.N, ctx.Bt = model, B, N, Bt
        ctx.state, ctx.lm, ctx.ef = state, lm, ef
        ctx.ew = ew
        ctx.n_params = len(params)
        sink = getattr(model, "_train_state_sink", None)
        if sink is not None:   # tests: the saved state (its head holds TimeConv's LeakyReLU decisions)
            sink.append(state)
        # the backward repacks the parameters' current values: saving them lets autograd's version
        # check raise if any was modified in place between forward and backward (e.g. an optimizer
        # step before a second backward), instead of returning gradients for the wrong weights
        ctx.save_for_backward(*params)
        return x_out, v_out, h_out

    @staticmethod
    def backward(ctx, gx, gv, gh):
        model, B, N, Bt = ctx.model, ctx.B, ctx.N, ctx.Bt
        _ = ctx.saved_tensors   # raises if a parameter changed in place since the forward
        L = _lib.lib()
        T = model.num_timesteps
        dev = ctx.state.device
        nl = model.n_layers
        bblobs = model._packed_bwd()
        grads = {name: torch.empty_like(p) for name, p in model.named_parameters()}
        lg = (_lib.LayerGrads * nl)()
        for i in range(nl):
            names = model.layer_param_names(i)
            lg[i] = _lib.LayerGrads(*[grads[nm].data_ptr() for nm in names])
        P = ctypes.c_void_p * nl
        tw_p = txw_p = g_tc = g_tcx = None   # use_time_conv=False: no TimeConv arrays
        if model.use_time_conv:
            tw = [_f32(m.t_conv.weights1) for m in model.time_conv_modules]
            txw = [_f32(m.t_conv.weights1) for m in model.time_conv_x_modules]
            tw_p, txw_p = P(*[t.data_ptr() for t in tw]), P(*[t.data_ptr() for t in txw])
            g_tc = P(*[grads[f"time_conv_modules.{i}.t_conv.weights1"].data_ptr() for i in range(nl)])
            g_tcx = P(*[grads[f"time_conv_x_modules.{i}.t_conv.weights1"].data_ptr() for i in range(nl)])
        ws_bytes = L.nonode_egno_backward_workspace_bytes(B, N, T, model.num_modes)
        ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.float32, device=dev)
        gx = _f32(gx) if gx is not None else torch.zeros(T * B * N, 3, device=dev)
        gv = _f32(gv) if gv is not None else None
        gh = _f32(gh) if gh is not None else None
        head = (B, N, T, nl, model.in_node_nf, model.in_edge_nf, model.time_emb_dim)
        tail = (model.num_modes, Bt,
                _lib.ptr(ctx.lm), _lib.ptr(ctx.ef), P(*[bblobs[i].data_ptr() for i in range(nl)]),
                tw_p, txw_p, _lib.ptr(ctx.state),
                _lib.ptr(gx), _lib.ptr(gv), _lib.ptr(gh), lg, g_tc, g_tcx,
                _lib.ptr(grads["embedding.weight"]), _lib.ptr(grads["embedding.bias"]), _lib.ptr(ws), ws_bytes,
                _lib.stream_of(gx))
        # input gradients (x, h, v, loc_mean: arguments 1, 2, 4, 5), per input slot [n_inputs, BN, .]
        want_x, want_h, want_v, want_lm = (ctx.needs_input_grad[k] for k in (1, 2, 4, 5))
        want_lm = want_lm and ctx.lm is not None and model.use_time_conv   # else the forward did not read it
        want_h = want_h and model.in_node_nf > 0
        g_in = [None] * 4
        if want_x or want_h or want_v or want_lm:
            I, BN = ctx.n_inputs, B * N
            new = lambda want, k: torch.empty(I, BN, k, device=dev) if want else None  # noqa: E731
            g_in = [new(want_x, 3), new(want_h, model.in_node_nf), new(want_v, 3), new(want_lm, 3)]
            fi = (ctypes.c_int * T)(*ctx.frame_input)
            ig = _lib.InputGrads(I, fi, _lib.ptr(ctx.ew), _lib.ptr(g_in[0]), _lib.ptr(g_in[2]), _lib.ptr(g_in[1]),
                                 _lib.ptr(g_in[3]))
            _lib.check(L.nonode_egno_backward_inputs(int(ctx.frames), *head, 1, *tail, ctypes.byref(ig)))
            g_in = [g.reshape(shp).to(dt) if g is not None else None
                    for g, shp, dt in zip(g_in, ctx.in_shapes, ctx.in_dtypes)]
        elif ctx.frames:
            _lib.check(L.nonode_egno_backward_frames(*head, 1, *tail))
        else:
            _lib.check(L.nonode_egno_backward(*head, *tail))
        ctx.state = None
        out = [grads[name] for name, _ in model.named_parameters()]
        g_x, g_h, g_v, g_lm = g_in
        return (None, g_x, g_h, None, g_v, g_lm) + (None,) * 5 + tuple(out)


def egno_forward_train(model, x, h, edge_fea, v, loc_mean, t_out, B, N, t_in=None, slots=None):
    """EGNO forward that records the kernels' backward on the autograd tape (t_in: per-frame
    multi-input form, see EGNO._forward_multi; slots: see EGNOTrain.forward)."""
    params = [p for _, p in model.named_parameters()]
    return EGNOTrain.apply(model, x, h, edge_fea, v, loc_mean, t_out, t_in, B, N, slots, *params)


def _segno_forward(ctx, model, h, x, v, edge_attr, T, B, N):
    """nonode_segno_forward_train from an embedded h (f32, contiguous): (x, h, v) after T substeps;
    ctx keeps the saved state for _segno_backward."""
    L = _lib.lib()
    dev = x.device
    x, v, ea = _f32(x), _f32(v), _f32(edge_attr)
    blob = model._packed()
    n = B * N
    x_out = torch.empty(n, 3, device=dev)
    v_out = torch.empty(n, 3, device=dev)
    h_out = torch.empty(n, model.hidden_nf, device=dev)
    st_bytes = L.nonode_segno_train_state_bytes(B, N, T)
    state = torch.empty((st_bytes + 3) // 4, dtype=torch.float32, device=dev)
    _lib.check(L.nonode_segno_forward_train(B, N, T, model.in_edge_nf, _lib.ptr(h), _lib.ptr(x), _lib.ptr(v),
                                            _lib.ptr(ea), _lib.ptr(blob), float(model.coords_weight),
                                            int(bool(model.recurrent)), _lib.ptr(x_out), _lib.ptr(v_out),
                                            _lib.ptr(h_out), _lib.ptr(state), st_bytes, _lib.stream_of(x)))
    ctx.model, ctx.T, ctx.B, ctx.N = model, T, B, N
    ctx.state, ctx.ea = state, ea
    ctx.set_materialize_grads(False)   # unused outputs: None, zeroed by the library (see EGNOTrain)
    return x_out, h_out, v_out


def _segno_backward(ctx, gx, gh, gv, want_h, want_x, want_v):
    """nonode_segno_backward: ({GCL parameter name: gradient}, g_h, g_x, g_v) with each input gradient
    None unless wanted (the library writes only the requested ones)."""
    model, T, B, N = ctx.model, ctx.T, ctx.B, ctx.N
    L = _lib.lib()
    dev = ctx.state.device
    n = B * N
    bblob = model._packed_bwd()
    names = model.gcl_param_names()
    named = dict(model.named_parameters())
    grads = {nm: torch.empty_like(named[nm]) for nm in names if nm is not None}
    lg = _lib.LayerGrads(*[grads[nm].data_ptr() if nm is not None else None for nm in names])
    ws_bytes = L.nonode_segno_backward_workspace_bytes(B, N)
    ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.float32, device=dev)
    gx = _f32(gx) if gx is not None else None
    gv = _f32(gv) if gv is not None else None
    gh = _f32(gh) if gh is not None else None
    g_h = torch.empty(n, model.hidden_nf, device=dev) if want_h else None
    g_x = torch.empty(n, 3, device=dev) if want_x else None
    g_v = torch.empty(n, 3, device=dev) if want_v else None
    _lib.check(L.nonode_segno_backward(B, N, T, model.in_edge_nf, float(model.coords_weight),
                                       int(bool(model.recurrent)), _lib.ptr(ctx.ea), _lib.ptr(bblob),
                                       _lib.ptr(ctx.state), _lib.ptr(gx), _lib.ptr(gv), _lib.ptr(gh),
                                       ctypes.byref(lg), _lib.ptr(g_h), _lib.ptr(g_x), _lib.ptr(g_v),
                                       _lib.ptr(ws), ws_bytes, _lib.stream_of(ws)))
    ctx.state = None
    return grads, g_h, g_x, g_v


class SEGNOStepTrain(torch.autograd.Function):
    """SEGNO.forward_step (SEGNO/models/model.py:95-102) on the autograd tape: T substeps of
    SEGNO_GCL (gcl.py:111-119) from an embedded h. Forward: nonode_segno_forward_train (one launch
    for the T substeps, saving each substep's state); backward: nonode_segno_backward (gradients of
    the shared GCL weights and of h, x, v)."""

    @staticmethod
    def forward(ctx, model, h, x, v, edge_attr, T, B, N, *params):
        ctx.save_for_backward(*params)   # version check of the parameters (see EGNOTrain.forward)
        return _segno_forward(ctx, model, _f32(h), x, v, edge_attr, T, B, N)

    @staticmethod
    def backward(ctx, gx, gh, gv):
        model = ctx.model
        _ = ctx.saved_tensors   # raises if a parameter changed in place since the forward
        grads, g_h, g_x, g_v = _segno_backward(ctx, gx, gh, gv, *ctx.needs_input_grad[1:4])
        out = [grads.get(nm) for nm, _ in model.module.named_parameters(prefix="module")]
        return (None, g_h, g_x, g_v, None, None, None, None) + tuple(out)


def segno_step_train(model, h, x, v, edge_attr, T, B, N):
    """forward_step that records the kernels' backward on the autograd tape."""
    params = [p for _, p in model.module.named_parameters()]
    return SEGNOStepTrain.apply(model, h, x, v, edge_attr, T, B, N, *params)


class SEGNOTrain(torch.autograd.Function):
    """SEGNO.forward in training with one input (SEGNO/models/model.py:53-102, train_nbody.py:168): the
    embedding Linear (model.py:73) and forward_step's T substeps as ONE node of the tape. The
    embedding runs as nonode_embedding_forward and its weight gradient as nonode_embedding_backward
    from the g_h the reverse pass returns, instead of broadcast torch ops and their autograd reverse."""

    @staticmethod
    def forward(ctx, model, his, x, v, edge_attr, T, B, N, *params):
        L = _lib.lib()
        ctx.his_dtype = his.dtype
        his = _f32(his)
        h = torch.empty(B * N, model.hidden_nf, device=x.device)
        ew, eb = _f32(model.embedding.weight), _f32(model.embedding.bias)
        _lib.check(L.nonode_embedding_forward(B * N, his.shape[1], _lib.ptr(his), _lib.ptr(ew), _lib.ptr(eb),
                                              _lib.ptr(h), _lib.stream_of(his)))
        # his through save_for_backward: autograd checks its version (an in-place edit after the
        # forward raises instead of silently changing the embedding gradient)
        ctx.save_for_backward(his, *params)
        return _segno_forward(ctx, model, h, x, v, edge_attr, T, B, N)

    @staticmethod
    def backward(ctx, gx, gh, gv):
        model = ctx.model
        his = ctx.saved_tensors[0]
        grads, g_h, g_x, g_v = _segno_backward(ctx, gx, gh, gv, True, *ctx.needs_input_grad[2:4])
        L = _lib.lib()
        n, din = his.shape
        gw = torch.empty_like(model.embedding.weight)
        gb = torch.empty_like(model.embedding.bias)
        ws_bytes = L.nonode_embedding_backward_workspace_bytes(n, din)
        ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.float32, device=g_h.device)
        _lib.check(L.nonode_embedding_backward(n, din, _lib.ptr(his), _lib.ptr(g_h), _lib.ptr(gw), _lib.ptr(gb),
                                               _lib.ptr(ws), ws_bytes, _lib.stream_of(g_h)))
        # dL/dhis of the embedding Linear (model.py:73), only when the caller's his requires grad
        g_his = (g_h @ _f32(model.embedding.weight)).to(ctx.his_dtype) if ctx.needs_input_grad[1] else None
        out = [grads.get(nm) for nm, _ in model.module.named_parameters(prefix="module")]
        return (None, g_his, g_x, g_v, None, None, None, None, gw, gb) + tuple(out)


def segno_train(model, his, x, v, edge_attr, T, B, N):
    """SEGNO.forward (one input, training): embedding + T substeps on the autograd tape."""
    params = [model.embedding.weight, model.embedding.bias] + [p for _, p in model.module.named_parameters()]
    return SEGNOTrain.apply(model, his, x, v, edge_attr, T, B, N, *params)


# ---- EGNO(flat=True) training (main_simulation_simple_no.py --flat; basic.py:38-40) ------------------
# One autograd node per layer: TimeConv + TimeConv_x (nonode_egno_tconv / nonode_egno_tconv_bwd) and the
# flat EGNN layer (nonode_egnn_layer_flat / nonode_egnn_layer_flat_bwd: the per-node and per-edge reverse
# of the 256-wide Tanh MLPs as HIP kernels). The weight gradients are sums over nodes or edges of the
# operand rows the reverse kernels write, i.e. plain GEMMs (torch.mm on the device: hipBLASLt / rocBLAS).
# The embedding Linear and the T-fold replication (egno.py:63-96) stay torch ops on the tape.
_FN = dict(GHP=0, GM=64, GF=128, GX=132, GA=136, GB=392, T=648, GT=904, U=1160, GU=1416, GPHI=1672, STRIDE=1676)
_FE = dict(A=0, M=256, C1=320, GZ3=576, GZ2=832, GPRE=896, GC=1152, S=1153, FE=1154, STRIDE=1160)


def _flat_layer_params(model, i):
    lay = model.layers[i]
    e, c, v, n = (lay.edge_message_net.scalar_net.mlp, lay.coord_net.mlp, lay.node_v_net.mlp, lay.node_net.mlp)
    return [e[0].weight, e[0].bias, e[2].weight, e[2].bias, c[0].weight, c[0].bias, c[2].weight, c[2].bias,
            v[0].weight, v[0].bias, v[2].weight, v[2].bias, n[0].weight, n[0].bias, n[2].weight, n[2].bias]


def _tconvx_lm_grad(gxo, gvo, txw, T, modes):
    """dL/dloc_mean [BN, 3] of one layer's x - loc_mean; TimeConv_x; + loc_mean (egno.py:103-107) from the
    gradients gxo, gvo [T*BN, 3] of TimeConv_x's outputs: the identity parts cancel, leaving minus the
    adjoint of the spectral term on the x channel summed over the frames (torch ops, the formula of
    input_lm_grad_kernel in csrc/nonode_train.hip)."""
    import math
    M = min(modes, T // 2 + 1)
    dev = gxo.device
    G = torch.stack([gxo, gvo], -1).reshape(T, -1, 2)                      # [T, BN*3, channel o]
    m = torch.arange(M, dtype=torch.float64, device=dev)
    ang = 2 * math.pi * m[:, None] * torch.arange(T, dtype=torch.float64, device=dev)[None] / T
    cm = torch.where((m == 0) | (2 * m == T), 1.0, 2.0) / T
    C, S = torch.cos(ang).to(G.dtype), torch.sin(ang).to(G.dtype)           # [M, T]
    cm = cm.to(G.dtype)[:, None]
    gYr = torch.einsum("mt,tno->mno", cm * C, G)
    gYi = -torch.einsum("mt,tno->mno", cm * S, G)
    wr, wi = txw[0, :, :M, 0].t()[:, None], txw[0, :, :M, 1].t()[:, None]   # input channel 0: [M, 1, o]
    gxr = (gYr * wr + gYi * wi).sum(-1)                                     # [M, BN*3]
    gxi = (-gYr * wi + gYi * wr).sum(-1)
    spec = (gxr * C.sum(1)[:, None] - gxi * S.sum(1)[:, None]).sum(0)
    return -spec.reshape(-1, 3)


def _layer_tconv(model, i, BN, h, x, v, loc_mean, tblobs, s):
    """The head of a per-layer tape node: TimeConv (+ TimeConv_x) of layer i on h [T*BN, 64], x, v
    [T*BN, 3] (f32, contiguous; nonode_egno_tconv). Returns (loc_mean as f32, ht, xt, vt, v_out): the
    EGNN layer's inputs and the v the node returns (the layer leaves v alone; without time convolutions
    the inputs themselves and a copy of v)."""
    if not model.use_time_conv:
        return None, h, x, v, v.clone()
    L = _lib.lib()
    T = model.num_timesteps
    n, dev = T * BN, h.device
    lm = _f32(loc_mean)
    tcx = _f32(model.time_conv_x_modules[i].t_conv.weights1)
    ht, xt, vt = torch.empty(n, 64, device=dev), torch.empty(n, 3, device=dev), torch.empty(n, 3, device=dev)
    _lib.check(L.nonode_egno_tconv(BN, T, model.num_modes, _lib.ptr(h), _lib.ptr(x), _lib.ptr(v), _lib.ptr(lm),
                                   _lib.ptr(tblobs[i]), _lib.ptr(tcx), _lib.ptr(ht), _lib.ptr(xt), _lib.ptr(vt), s))
    return lm, ht, xt, vt, vt


def _layer_tconv_bwd(model, i, BN, h, x, v, lm, p_tw, p_txw, ght, gxt, gvt, want_lm, s):
    """The tail of a per-layer tape node's backward: nonode_egno_tconv_bwd from the gradients ght, gxt, gvt
    of the EGNN layer's inputs. Returns (g_h, g_x, g_v, g_loc_mean or None, g_weights1 of TimeConv and of
    TimeConv_x in their parameters' dtypes)."""
    L = _lib.lib()
    T = model.num_timesteps
    g_h, g_x, g_v = torch.empty_like(h), torch.empty_like(x), torch.empty_like(v)
    tw, txw = _f32(p_tw), _f32(p_txw)      # kept alive over the call
    g_tw, g_txw = torch.empty_like(tw), torch.empty_like(txw)
    ws_bytes = L.nonode_egno_tconv_bwd_workspace_bytes(BN, T, model.num_modes)
    ws = torch.empty((ws_bytes + 3) // 4, device=h.device)
    _, tblobs = model._packed()
    _lib.check(L.nonode_egno_tconv_bwd(BN, T, model.num_modes, _lib.ptr(h), _lib.ptr(x), _lib.ptr(v), _lib.ptr(lm),
                                       _lib.ptr(tblobs[i]), _lib.ptr(tw), _lib.ptr(txw), _lib.ptr(ght),
                                       _lib.ptr(gxt), _lib.ptr(gvt), _lib.ptr(g_h), _lib.ptr(g_x), _lib.ptr(g_v),
                                       _lib.ptr(g_tw), _lib.ptr(g_txw), _lib.ptr(ws), ws_bytes, s))
    sink = getattr(model, "_train_bwd_sink", None)
    if sink is not None:   # tests: the workspace head holds the LeakyReLU decisions the reverse used
        sink.append((i, ws))
    g_lm = _tconvx_lm_grad(gxt, gvt, txw, T, model.num_modes) if want_lm else None
    return g_h, g_x, g_v, g_lm, g_tw.to(p_tw.dtype), g_txw.to(p_txw.dtype)


def _layer_tape(model, node, head, hh, xx, vv, lm, edge_fea):
    """One tape node `node` (FlatLayerTrain / GraphLayerTrain, called with (model, i, *head, h, x, v, loc_mean,
    edge_fea, *layer parameters)) per layer; returns (x, v, h) as EGNO.forward does."""
    for i in range(model.n_layers):
        params = _flat_layer_params(model, i)
        if model.use_time_conv:
            params += [model.time_conv_modules[i].t_conv.weights1, model.time_conv_x_modules[i].t_conv.weights1]
        hh, xx, vv = node.apply(model, i, *head, hh, xx, vv, lm, edge_fea, *params)
    return xx, vv, hh


class FlatLayerTrain(torch.autograd.Function):
    """TimeConv (+ TimeConv_x) of layer i, then its flat EGNN layer (egno.py:99-111 with flat=True)."""

    @staticmethod
    def forward(ctx, model, i, B, N, h, x, v, loc_mean, ef, *params):
        L = _lib.lib()
        T = model.num_timesteps
        dev = h.device
        n = T * B * N
        h, x, v, ef = _f32(h), _f32(x), _f32(v), _f32(ef)
        blobs, tblobs = model._packed()
        s = _lib.stream_of(h)
        lm, ht, xt, vt, v_out = _layer_tconv(model, i, B * N, h, x, v, loc_mean, tblobs, s)
        state = torch.empty(L.nonode_egnn_layer_flat_state_floats(T * B, N), device=dev)
        h_out, x_out = torch.empty(n, 64, device=dev), torch.empty(n, 3, device=dev)
        _lib.check(L.nonode_egnn_layer_flat(T * B, N, model.in_edge_nf, B, _lib.ptr(ht), _lib.ptr(xt), _lib.ptr(vt),
                                            _lib.ptr(ef), _lib.ptr(blobs[i]), _lib.ptr(h_out), _lib.ptr(x_out),
                                            _lib.ptr(state), s))
        ctx.set_materialize_grads(False)
        ctx.model, ctx.i, ctx.B, ctx.N = model, i, B, N
        ctx.keep = (h, x, v, lm, ef, ht, xt, vt, state)
        ctx.save_for_backward(*params)
        return h_out, x_out, v_out

    @staticmethod
    def backward(ctx, gh, gx, gv):
        model, i, B, N = ctx.model, ctx.i, ctx.B, ctx.N
        params = ctx.saved_tensors
        h, x, v, lm, ef, ht, xt, vt, state = ctx.keep
        ctx.keep = None
        L = _lib.lib()
        T = model.num_timesteps
        dev = h.device
        n, E = T * B * N, T * B * N * (N - 1)
        z = lambda k: torch.zeros(n, k, device=dev)  # noqa: E731
        gh = _f32(gh) if gh is not None else z(64)
        gx = _f32(gx) if gx is not None else z(3)
        gv = _f32(gv) if gv is not None else z(3)
        blobs, _ = model._packed()
        bb = model._packed_bwd()
        nops = torch.empty(n, _FN["STRIDE"], device=dev)
        eops = torch.empty(E, _FE["STRIDE"], device=dev)
        gvt = torch.empty(n, 3, device=dev)
        s = _lib.stream_of(gh)
        _lib.check(L.nonode_egnn_layer_flat_bwd(T * B, N, model.in_edge_nf, B, _lib.ptr(ht), _lib.ptr(xt), _lib.ptr(vt),
                                                _lib.ptr(ef), _lib.ptr(blobs[i]), _lib.ptr(bb[i]), _lib.ptr(state),
                                                _lib.ptr(gx), _lib.ptr(gv), _lib.ptr(gh), _lib.ptr(nops), _lib.ptr(eops),
                                                _lib.ptr(gvt), s))
        cols = lambda a, k, w: a[:, k:k + w]  # noqa: E731
        F_, E_ = _FN, _FE
        GA, GB = cols(nops, F_["GA"], 256), cols(nops, F_["GB"], 256)
        gpre, a_, m_ = cols(eops, E_["GPRE"], 256), cols(eops, E_["A"], 256), cols(eops, E_["M"], 64)
        gz3, gz2, c1 = cols(eops, E_["GZ3"], 256), cols(eops, E_["GZ2"], 64), cols(eops, E_["C1"], 256)
        gc, sr = eops[:, E_["GC"]], eops[:, E_["S"]]
        gt, t_ = cols(nops, F_["GT"], 256), cols(nops, F_["T"], 256)
        gu, u_ = cols(nops, F_["GU"], 256), cols(nops, F_["U"], 256)
        gphi = nops[:, F_["GPHI"]]
        M = state[n * 512:n * 576].view(n, 64)
        w1 = params[0]
        ne = model.in_edge_nf
        # the first Linear's columns [s, h_i, h_j, e] (EGNO order): GA / GB carry its h_i / h_j parts
        dw1 = torch.cat([(gpre.t() @ sr)[:, None], GA.t() @ ht, GB.t() @ ht] +
                        ([gpre.t() @ eops[:, E_["FE"]:E_["FE"] + ne]] if ne else []), 1)
        grads = [dw1, GA.sum(0), gz2.t() @ a_, gz2.sum(0),              # edge MLP
                 gz3.t() @ m_, gz3.sum(0), (gc @ c1)[None], gc.sum()[None],   # coord MLP
                 gt.t() @ ht, gt.sum(0), (gphi @ t_)[None], gphi.sum()[None],  # node_v MLP
                 gu.t() @ torch.cat([ht, M], 1), gu.sum(0), gh.t() @ u_, gh.sum(0)]   # node MLP
        ght = cols(nops, F_["GHP"], 64) + GA @ w1[:, 1:65] + GB @ w1[:, 65:129]
        gxt = cols(nops, F_["GX"], 3).contiguous()
        ght = ght.contiguous()
        grads = [g.reshape(p.shape).to(p.dtype) for g, p in zip(grads, params[:16])]
        if not model.use_time_conv:
            return (None,) * 4 + (ght, gxt, gvt, None, None) + tuple(grads)
        tail = _layer_tconv_bwd(model, i, B * N, h, x, v, lm, params[16], params[17], ght, gxt, gvt,
                                ctx.needs_input_grad[7], s)
        return (None,) * 4 + tail[:4] + (None,) + tuple(grads) + tail[4:]


def _embed_frames(model, x, h, v, loc_mean, t_out, BN):
    """The head of EGNO.forward (egno.py:37-96, num_inputs == 1) as torch ops on the tape: the time
    embedding, the embedding Linear and the T-fold replication. Returns (h [T*BN, 64], x, v [T*BN, 3],
    loc_mean as f32 or None without time convolutions)."""
    import math
    T = model.num_timesteps
    dim, half = model.time_emb_dim, model.time_emb_dim // 2
    # get_timestep_embedding (layer_no.py:8-17)
    freqs = torch.exp(torch.arange(half, dtype=torch.float32, device=x.device) * -(math.log(10000) / (half - 1)))
    ang = t_out.float()[..., None] * freqs
    temb = torch.cat([torch.sin(ang), torch.cos(ang)], dim=-1)
    if dim % 2 == 1:
        temb = torch.nn.functional.pad(temb, (0, 1))
    Bt = temb.shape[0]
    temb = temb.permute(1, 0, 2)[:, None].repeat(1, BN // Bt, 1, 1).reshape(T, BN, -1)   # egno.py:66
    hh = model.embedding(torch.cat([h.float()[None].expand(T, -1, -1), temb], -1).reshape(T * BN, -1))
    xx, vv = x.float().repeat(T, 1), v.float().repeat(T, 1)                             # egno.py:89-96
    lm = loc_mean.float() if model.use_time_conv else None
    return hh, xx, vv, lm


def egno_flat_train(model, x, h, edge_fea, v, loc_mean, t_out, B, N):
    """EGNO(flat=True).forward in training (egno.py:37-111, num_inputs == 1): the time embedding and the
    embedding Linear as torch ops, then one FlatLayerTrain node per layer."""
    hh, xx, vv, lm = _embed_frames(model, x, h, v, loc_mean, t_out, B * N)
    return _layer_tape(model, FlatLayerTrain, (B, N), hh, xx, vv, lm, edge_fea)


# ---- EGNO(graph="trainable") training on any edge list (csrc/nonode_graph_train.hip) ------------------
# One autograd node per layer, as FlatLayerTrain: TimeConv + TimeConv_x, then the graph layer
# (nonode_egnn_layer_graph, whose workspace is the saved state) and its reverse
# (nonode_egnn_layer_graph_bwd: HIP kernels for everything per node and per edge). The weight gradients
# are sums over nodes or edges of outer products of the operand rows the reverse writes: GEMMs on the
# device, accumulated over groups of frames.
#
# GRAPH_OPS_CAP_BYTES bounds the per-edge operand buffer of one group (400 floats per edge and frame):
# the reverse runs frames [f0, f1) per call with (f1 - f0) * E * 1600 bytes under the cap (at least one
# frame). 1 GiB: a group then still holds several hundred thousand rows, enough for the GEMMs to run at
# their large-K rate (a k-NN graph of 8 x 1000 nodes with 16 neighbours is 5 frames per group), while the
# transient stays a fraction of a percent of the device's HBM however many frames or edges a model has.
# (A model attribute `graph_ops_cap_bytes`, if set, takes its place for that model.)
GRAPH_OPS_CAP_BYTES = 1 << 30
_GN = dict(GHP=0, GM=64, GZ=128, Z=192, GT=256, T=320, GA=384, GB=448, GF=512, GX=516, STRIDE=520)
_GE = dict(GZ1=0, GZ2=64, A=128, X8=192, GZ3=200, GC=264, M=268, ONE=332, C1=336, STRIDE=400)
_NEG_LN2 = -0.6931471805599453   # the forward's state keeps M in the packed blob's log2-domain scale


def _tn(X, Y, split=256):
    """X^T Y of tall operands X [rows, a], Y [rows, b] (column slices of an operand buffer). A 64 x 64 result
    alone gives the GEMM a handful of workgroups for a million rows, so the rows are cut into `split` equal
    chunks, multiplied as one batch and added in chunk order (a fixed order: deterministic)."""
    rows = X.shape[0]
    c = rows // split
    if c < 64:
        return X.t() @ Y
    main = c * split
    out = torch.bmm(X[:main].unflatten(0, (split, c)).transpose(1, 2), Y[:main].unflatten(0, (split, c))).sum(0)
    return out if main == rows else out + X[main:].t() @ Y[main:]


def graph_frame_groups(n_frames, E, cap_bytes=None):
    """[(f0, f1), ...]: the frame groups of one layer's reverse under the operand cap."""
    cap = GRAPH_OPS_CAP_BYTES if cap_bytes is None else cap_bytes
    per = max(1, int(cap // max(1, E * _GE["STRIDE"] * 4)))
    return [(f0, min(f0 + per, n_frames)) for f0 in range(0, n_frames, per)]


def graph_w1_columns(variant, e1, e1h, ne):
    """The gradient of the edge MLP's first Linear [64, 129 + ne] from the two products that hold its parts:
    e1 = [gz1 | gz2]^T [a | 1, s, e] (rows 0..63: column 65 the radial input s, columns 66.. the ne edge
    features) and e1h = [GA | GB]^T h [128, 64] (rows 0..63 the h_i block, 64..127 the h_j block). EGNO's
    input order is [s, h_i, h_j, e] (basic.py:152-154), SEGNO's [h_i, h_j, s, e] (gcl.py:78). A pure function
    of its arguments (any device)."""
    s_col, e_cols = e1[:64, 65:66], ([e1[:64, 66:66 + ne]] if ne else [])
    if variant == _lib.VARIANT_EGNO:
        return torch.cat([s_col, e1h[:64], e1h[64:]] + e_cols, 1)
    return torch.cat([e1h[:64], e1h[64:], s_col] + e_cols, 1)


def _graph_weight_grads(variant, nops, eops, hs, Ms, gho, ne, E):
    """The 16 parameter gradients (nonode_layer_weights order) of the rows of one operand group: nops [rows, 520],
    eops [.., 400] as the reverse kernels wrote them, hs / Ms the layer inputs and message sums of those rows
    (Ms in the state's log2-domain scale), gho the gradient of h_out for them (None = 0). SEGNO has no
    node_v MLP: its four entries are None (the gt, t and gphi slots of nops are not read)."""
    dev = nops.device
    N_, E_ = _GN, _GE
    nc = lambda k, w=64: nops[:, N_[k]:N_[k] + w]  # noqa: E731
    hM = torch.cat([hs, Ms * _NEG_LN2], 1)
    gz, z_ = nc("GZ"), nc("Z")
    # node level: [GA | GB]^T h, gt^T h, gz^T [h | M], gho^T z, gphi^T t
    e1h = _tn(nc("GA", 128), hs)
    if E:
        # edge level: [gz1 | gz2]^T [a | 1, s, e] and [gz3 | gc]^T [m | 1 | c1]
        e1 = _tn(eops[:, E_["GZ1"]:E_["GZ1"] + 128], eops[:, E_["A"]:E_["A"] + 72])
        e2 = _tn(eops[:, E_["GZ3"]:E_["GZ3"] + 65], eops[:, E_["M"]:E_["M"] + 132])
    else:
        e1, e2 = torch.zeros(128, 72, device=dev), torch.zeros(65, 132, device=dev)
    if gho is not None:
        dn2, dbn2 = _tn(gho, z_), gho.sum(0)
    else:
        dn2, dbn2 = torch.zeros(64, 64, device=dev), torch.zeros(64, device=dev)
    if variant == _lib.VARIANT_EGNO:
        gt = nc("GT")
        gphi = nops[:, N_["GF"] + 3:N_["GF"] + 4]
        node_v = [_tn(gt, hs), gt.sum(0), _tn(gphi, nc("T")), gphi.sum(0)]
    else:
        node_v = [None] * 4
    return [graph_w1_columns(variant, e1, e1h, ne), e1[:64, 64], e1[64:, :64], e1[64:, 64],   # edge MLP
            e2[:64, :64], e2[:64, 64], e2[64:, 68:132], e2[64, 64:65],                         # coord MLP
            *node_v,                                                                           # node_v MLP
            _tn(gz, hM), gz.sum(0), dn2, dbn2]                                                 # node MLP


def graph_layer_reverse(n_frames, n, E, ne, ef_frames, h, x, v, ef, blob, bblob, state, csr, scsr, gx, gv, gh,
                        cap_bytes=None, want_w=True, variant=_lib.VARIANT_EGNO, segno=None):
    """The reverse of the graph layer plus the weight-gradient GEMMs. h [n_frames*n, 64],
    x, v [.., 3], ef [ef_frames * E, ne] (f32, contiguous), state: the workspace nonode_egnn_layer_graph
    filled, csr = (row_ptr, col, eid), scsr = (srow_ptr, seid, valid) of graph.csr / graph.csr_by_sender,
    gx, gv, gh: gradients of the layer's outputs (None = 0). Returns (g_h_in, g_x_in, g_v_in, grads) with
    grads the 16 parameter gradients in nonode_layer_weights order (edge, coord, node_v, node MLP; None with
    want_w=False, a frozen model's input gradients).
    variant EGNO (the default): nonode_egnn_layer_graph_bwd over the frame groups; the first Linear's columns
    [s, h_i, h_j, e]. variant SEGNO with segno = (dt, coords_weight, recurrent): ONE substep (n_frames =
    ef_frames = 1) through nonode_segno_layer_graph_bwd; the first Linear's columns [h_i, h_j, s, e]
    (gcl.py:78) and the four node_v gradients None (autograd.segno_graph_reverse walks the substeps and
    groups their operands itself)."""
    L = _lib.lib()
    dev = h.device
    nt = n_frames * n
    row_ptr, col, eid = csr
    srow_ptr, seid, valid = scsr
    g_h, g_x, g_v = torch.empty(nt, 64, device=dev), torch.empty(nt, 3, device=dev), torch.empty(nt, 3, device=dev)
    M = state[2 * nt * 64:3 * nt * 64].view(nt, 64)
    s = _lib.stream_of(h)
    N_, E_ = _GN, _GE
    if variant != _lib.VARIANT_EGNO:
        if n_frames != 1 or ef_frames != 1 or segno is None:
            raise ValueError("graph_layer_reverse: SEGNO reverses one substep (n_frames = ef_frames = 1) with "
                             "segno=(dt, coords_weight, recurrent)")
        nops = torch.empty(n, N_["STRIDE"], device=dev)
        eops = torch.empty(E, E_["STRIDE"], device=dev)
        _segno_substep_bwd(L, n, E, ne, h, x, v, ef, blob, bblob, state, csr, scsr, gx, gv, gh, segno, nops, eops,
                           g_h, g_x, g_v, s)
        return g_h, g_x, g_v, (_graph_weight_grads(variant, nops, eops, h, M, gh, ne, E) if want_w else None)
    total = None
    for f0, f1 in graph_frame_groups(n_frames, E, cap_bytes):
        nf = f1 - f0
        nops = torch.empty(nf * n, N_["STRIDE"], device=dev)
        eops = torch.empty(nf * E, E_["STRIDE"], device=dev)
        _lib.check(L.nonode_egnn_layer_graph_bwd(
            _lib.VARIANT_EGNO, n_frames, n, E, ne, ef_frames, f0, f1, _lib.ptr(h), _lib.ptr(x), _lib.ptr(v),
            _lib.ptr(ef) if ne else None, _lib.ptr(blob), _lib.ptr(bblob), _lib.ptr(state), _lib.ptr(row_ptr),
            _lib.ptr(col), _lib.ptr(eid), _lib.ptr(srow_ptr), _lib.ptr(seid), _lib.ptr(valid), _lib.ptr(gx), _lib.ptr(gv),
            _lib.ptr(gh), _lib.ptr(nops), _lib.ptr(eops) if E else None, _lib.ptr(g_h), _lib.ptr(g_x), _lib.ptr(g_v), s))
        if not want_w:
            continue
        grads = _graph_weight_grads(variant, nops, eops, h[f0 * n:f1 * n], M[f0 * n:f1 * n],
                                    gh[f0 * n:f1 * n] if gh is not None else None, ne, E)
        total = grads if total is None else [a + b for a, b in zip(total, grads)]
    return g_h, g_x, g_v, total


def _segno_substep_bwd(L, n, E, ne, h, x, v, ef, blob, bblob, ws, csr, scsr, gx, gv, gh, segno, nops, eops, g_h, g_x,
                       g_v, s):
    """nonode_segno_layer_graph_bwd of one substep (h, x, v: its inputs; ws: its layer workspace)."""
    row_ptr, col, eid = csr
    srow_ptr, seid, valid = scsr
    dt, cw, recurrent = segno
    _lib.check(L.nonode_segno_layer_graph_bwd(
        n, E, ne, _lib.ptr(h), _lib.ptr(x), _lib.ptr(v), _lib.ptr(ef) if ne else None, _lib.ptr(blob), _lib.ptr(bblob),
        _lib.ptr(ws), _lib.ptr(row_ptr), _lib.ptr(col), _lib.ptr(eid), _lib.ptr(srow_ptr), _lib.ptr(seid),
        _lib.ptr(valid), _lib.ptr(gx), _lib.ptr(gv), _lib.ptr(gh), float(dt), float(cw), int(bool(recurrent)),
        _lib.ptr(nops), _lib.ptr(eops) if E else None, _lib.ptr(g_h), _lib.ptr(g_x), _lib.ptr(g_v), s))


class GraphLayerTrain(torch.autograd.Function):
    """TimeConv (+ TimeConv_x) of layer i, then its EGNN layer on an explicit edge list (egno.py:99-111
    with any `edges`)."""

    @staticmethod
    def forward(ctx, model, i, n, E, graph, h, x, v, loc_mean, ef, *params):
        L = _lib.lib()
        T = model.num_timesteps
        dev = h.device
        nt = T * n
        h, x, v, ef = _f32(h), _f32(x), _f32(v), _f32(ef)
        blobs, tblobs = model._packed()
        s = _lib.stream_of(h)
        lm, ht, xt, vt, v_out = _layer_tconv(model, i, n, h, x, v, loc_mean, tblobs, s)
        row_ptr, col, eid = graph[0]
        st_bytes = L.nonode_egnn_layer_graph_workspace_bytes(T, n)
        state = torch.empty((st_bytes + 3) // 4, device=dev)   # the layer's workspace is the saved state
        h_out, x_out = torch.empty(nt, 64, device=dev), torch.empty(nt, 3, device=dev)
        _lib.check(L.nonode_egnn_layer_graph(
            _lib.VARIANT_EGNO, T, n, E, model.in_edge_nf, 1, _lib.ptr(ht), _lib.ptr(xt), _lib.ptr(vt), _lib.ptr(ef),
            _lib.ptr(blobs[i]), _lib.ptr(row_ptr), _lib.ptr(col), _lib.ptr(eid), 0.0, 1.0, 0, _lib.ptr(h_out),
            _lib.ptr(x_out), None, _lib.ptr(state), st_bytes, s))
        ctx.set_materialize_grads(False)
        ctx.model, ctx.i, ctx.n, ctx.E, ctx.graph = model, i, n, E, graph
        ctx.keep = (h, x, v, lm, ef, ht, xt, vt, state)
        ctx.save_for_backward(*params)
        return h_out, x_out, v_out

    @staticmethod
    def backward(ctx, gh, gx, gv):
        model, i, n, E = ctx.model, ctx.i, ctx.n, ctx.E
        params = ctx.saved_tensors   # raises if a parameter changed in place since the forward
        h, x, v, lm, ef, ht, xt, vt, state = ctx.keep
        ctx.keep = None
        gh, gx, gv = _f32(gh), _f32(gx), _f32(gv)
        blobs, _ = model._packed()
        bb = model._packed_bwd()
        T = model.num_timesteps
        ght, gxt, gvt, grads = graph_layer_reverse(T, n, E, model.in_edge_nf, 1, ht, xt, vt, ef, blobs[i], bb[i], state,
                                                   ctx.graph[0], ctx.graph[1], gx, gv, gh,
                                                   getattr(model, "graph_ops_cap_bytes", None),
                                                   want_w=any(ctx.needs_input_grad[10:26]))
        grads = [g.reshape(p.shape).to(p.dtype) for g, p in zip(grads, params[:16])] if grads else [None] * 16
        if not model.use_time_conv:
            return (None,) * 5 + (ght, gxt, gvt, None, None) + tuple(grads)
        tail = _layer_tconv_bwd(model, i, n, h, x, v, lm, params[16], params[17], ght, gxt, gvt,
                                ctx.needs_input_grad[8], _lib.stream_of(h))
        return (None,) * 5 + tail[:4] + (None,) + tuple(grads) + tail[4:]


def egno_graph_train(model, x, h, edge_index, edge_fea, v, loc_mean, t_out):
    """EGNO(graph="trainable").forward on the tape (egno.py:37-111, num_inputs == 1, any edge list): the
    time embedding and the embedding Linear as torch ops, then one GraphLayerTrain node per layer.
    A graph.NeighborGraph with its CSR by sender runs with E = capacity and edge_fea [capacity, in_edge_nf]:
    the kernels read only entries the two CSRs name, and the reverse zeroes the edge operand rows of the tail
    (valid == 0), so nothing here reads the edge count back. No gradient flows through the choice of
    neighbours (it is discrete) or through edge_fea (detached, as the reference does at
    main_simulation_simple_no.py:333,338)."""
    from . import graph as _graph
    n = h.shape[0]
    E = _graph._split(edge_index)[0].numel()
    csr = _graph.csr(edge_index, n, device=x.device)
    scsr = _graph.csr_by_sender(edge_index, n, device=x.device)
    hh, xx, vv, lm = _embed_frames(model, x, h, v, loc_mean, t_out, n)
    return _layer_tape(model, GraphLayerTrain, (n, E, (csr, scsr)), hh, xx, vv, lm, edge_fea)


# ---- SEGNO(graph="any", trainable=True) training on any edge list ------------------------------------------
# forward_step's T substeps (model.py:95-102) as ONE autograd node: nonode_segno_forward_train_graph saves
# every substep's inputs and its layer workspace (T n 266 floats; 1.4 GB at n = 25,600 and 50 substeps), the
# backward walks the substeps T-1 .. 0 through nonode_segno_layer_graph_bwd. The operand rows of several
# substeps go into one buffer (the frame-group mechanism with substeps in place of frames, bounded by
# GRAPH_OPS_CAP_BYTES / model.graph_ops_cap_bytes) and each group gets one set of weight-gradient GEMMs,
# added in the order of the walk.

def _segno_graph_state(state, T, n):
    """(hs [T, n, 64], ws [T, n * 196], xs [T, n, 3], vs [T, n, 3]) views of the training forward's state
    (include/nonode.h: nonode_segno_forward_train_graph)."""
    o1, o2, o3 = T * n * 64, T * n * 260, T * n * 263
    return (state[:o1].view(T, n, 64), state[o1:o2].view(T, n * 196), state[o2:o3].view(T, n, 3),
            state[o3:T * n * 266].view(T, n, 3))


def _segno_graph_forward(ctx, model, h, x, v, edge_attr, T, graph):
    """nonode_segno_forward_train_graph from an embedded h (f32, contiguous): (x, h, v) after T substeps; ctx
    keeps the saved state for segno_graph_reverse. graph = (n, E, csr, scsr)."""
    L = _lib.lib()
    n, E, csr, _ = graph
    dev = x.device
    x, v, ea = _f32(x), _f32(v), _f32(edge_attr)
    blob = model._packed()
    x_out, v_out, h_out = (torch.empty(n, k, device=dev) for k in (3, 3, model.hidden_nf))
    st_bytes = L.nonode_segno_graph_train_state_bytes(n, T)
    state = torch.empty(st_bytes // 4, dtype=torch.float32, device=dev)
    _lib.check(L.nonode_segno_forward_train_graph(
        n, E, T, model.in_edge_nf, _lib.ptr(h), _lib.ptr(x), _lib.ptr(v), _lib.ptr(ea) if model.in_edge_nf else None,
        _lib.ptr(blob), _lib.ptr(csr[0]), _lib.ptr(csr[1]), _lib.ptr(csr[2]), float(model.coords_weight),
        int(bool(model.recurrent)), _lib.ptr(x_out), _lib.ptr(v_out), _lib.ptr(h_out), _lib.ptr(state), st_bytes,
        _lib.stream_of(x)))
    ctx.model, ctx.T, ctx.graph, ctx.state = model, T, graph, state
    ctx.set_materialize_grads(False)   # unused outputs: None, taken as zero by the reverse kernels
    sink = getattr(model, "_train_ops_sink", None)
    ctx.ops_sink = sink   # tests: the operand buffers of the backward's groups
    return (x_out, h_out, v_out), (x, v, ea)


def segno_graph_reverse(model, T, graph, state, ea, gx, gh, gv, want_w=True, cap_bytes=None, ops_sink=None):
    """The reverse of the T substeps: ({GCL parameter name: gradient} or {} with want_w=False, g_h, g_x, g_v)
    of the inputs. gx, gh, gv: gradients of the outputs (None = 0)."""
    L = _lib.lib()
    n, E, csr, scsr = graph
    ne = model.in_edge_nf
    dev = state.device
    if T == 0:   # the inputs passed through
        return {}, gh, gx, gv
    gx, gh, gv = _f32(gx), _f32(gh), _f32(gv)
    blob, bblob = model._packed(), model._packed_bwd()
    hs, ws, xs, vs = _segno_graph_state(state, T, n)
    segno = (1.0 / T, model.coords_weight, model.recurrent)
    s = _lib.stream_of(state)
    N_, E_ = _GN, _GE
    total = None
    for t0, t1 in reversed(graph_frame_groups(T, E, cap_bytes)):
        g = t1 - t0
        nops = torch.empty(g * n, N_["STRIDE"], device=dev)
        eops = torch.empty(g * E, E_["STRIDE"], device=dev)
        ghos = [None] * g
        for t in range(t1 - 1, t0 - 1, -1):
            k = t - t0
            ghos[k] = gh
            g_h, g_x, g_v = torch.empty(n, 64, device=dev), torch.empty(n, 3, device=dev), torch.empty(n, 3, device=dev)
            _segno_substep_bwd(L, n, E, ne, hs[t], xs[t], vs[t], ea, blob, bblob, ws[t], csr, scsr, gx, gv, gh, segno,
                               nops[k * n:(k + 1) * n], eops[k * E:(k + 1) * E], g_h, g_x, g_v, s)
            gh, gx, gv = g_h, g_x, g_v
        if ops_sink is not None:
            ops_sink.append((t0, t1, nops, eops))
        if not want_w:
            continue
        Ms = torch.cat([ws[t][2 * n * 64:3 * n * 64].view(n, 64) for t in range(t0, t1)])
        if all(q is None for q in ghos):
            gho = None
        else:
            gho = torch.cat([q if q is not None else torch.zeros(n, 64, device=dev) for q in ghos])
        grads = _graph_weight_grads(_lib.VARIANT_SEGNO, nops, eops, hs[t0:t1].reshape(g * n, 64), Ms, gho, ne, E)
        total = grads if total is None else [a + b if a is not None else None for a, b in zip(total, grads)]
    named = dict(model.named_parameters())
    out = {}
    if total is not None:
        for nm, gr in zip(model.gcl_param_names(), total):
            if nm is not None:
                out[nm] = gr.reshape(named[nm].shape).to(named[nm].dtype)
    return out, gh, gx, gv


def _segno_graph_backward(ctx, gx, gh, gv, want_w):
    model = ctx.model
    out = segno_graph_reverse(model, ctx.T, ctx.graph, ctx.state, ctx.ea, gx, gh, gv, want_w,
                              getattr(model, "graph_ops_cap_bytes", None), ctx.ops_sink)
    ctx.state = None
    return out


class SEGNOGraphStepTrain(torch.autograd.Function):
    """SEGNO.forward_step (SEGNO/models/model.py:95-102) on any edge list, on the autograd tape: T substeps of
    SEGNO_GCL (gcl.py:111-119) from an embedded h. It serves forward_step, his wider than 40 features and the
    multi-input forward (SEGNO._step)."""

    @staticmethod
    def forward(ctx, model, h, x, v, edge_attr, T, graph, *params):
        h = _f32(h)
        outs, (x, v, ea) = _segno_graph_forward(ctx, model, h, x, v, edge_attr, T, graph)
        ctx.ea = ea
        # the parameters (the backward repacks their current values) and the inputs through
        # save_for_backward: an in-place edit of any of them after the forward raises in the backward
        ctx.save_for_backward(h, x, v, ea, *params)
        return outs

    @staticmethod
    def backward(ctx, gx, gh, gv):
        model = ctx.model
        _ = ctx.saved_tensors   # the version check
        grads, g_h, g_x, g_v = _segno_graph_backward(ctx, gx, gh, gv, any(ctx.needs_input_grad[7:]))
        out = [grads.get(nm) for nm, _ in model.module.named_parameters(prefix="module")]
        return (None, g_h, g_x, g_v, None, None, None) + tuple(out)


def segno_graph_step_train(model, h, x, v, edge_attr, T, graph):
    """forward_step on any edge list that records the kernels' backward on the autograd tape."""
    params = [p for _, p in model.module.named_parameters()]
    return SEGNOGraphStepTrain.apply(model, h, x, v, edge_attr, T, graph, *params)


class SEGNOGraphTrain(torch.autograd.Function):
    """SEGNO.forward in training with one input (SEGNO/models/model.py:53-102) on any edge list: the embedding
    Linear (model.py:73; nonode_embedding_forward / _backward) and forward_step's T substeps as ONE node of
    the tape, like SEGNOTrain."""

    @staticmethod
    def forward(ctx, model, his, x, v, edge_attr, T, graph, *params):
        L = _lib.lib()
        ctx.his_dtype = his.dtype
        his = _f32(his)
        n = graph[0]
        h = torch.empty(n, model.hidden_nf, device=x.device)
        ew, eb = _f32(model.embedding.weight), _f32(model.embedding.bias)
        _lib.check(L.nonode_embedding_forward(n, his.shape[1], _lib.ptr(his), _lib.ptr(ew), _lib.ptr(eb),
                                              _lib.ptr(h), _lib.stream_of(his)))
        outs, (x, v, ea) = _segno_graph_forward(ctx, model, h, x, v, edge_attr, T, graph)
        ctx.ea = ea
        ctx.save_for_backward(his, x, v, ea, *params)   # version checks, as SEGNOGraphStepTrain
        return outs

    @staticmethod
    def backward(ctx, gx, gh, gv):
        model = ctx.model
        his = ctx.saved_tensors[0]
        want_w = any(ctx.needs_input_grad[7:])
        grads, g_h, g_x, g_v = _segno_graph_backward(ctx, gx, gh, gv, want_w)
        gw = gb = g_his = None
        if g_h is not None and want_w:
            L = _lib.lib()
            n, din = his.shape
            gw = torch.empty_like(model.embedding.weight)
            gb = torch.empty_like(model.embedding.bias)
            ws_bytes = L.nonode_embedding_backward_workspace_bytes(n, din)
            ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.float32, device=g_h.device)
            _lib.check(L.nonode_embedding_backward(n, din, _lib.ptr(his), _lib.ptr(g_h), _lib.ptr(gw), _lib.ptr(gb),
                                                   _lib.ptr(ws), ws_bytes, _lib.stream_of(g_h)))
        if g_h is not None and ctx.needs_input_grad[1]:   # dL/dhis of the embedding Linear (model.py:73)
            g_his = (g_h @ _f32(model.embedding.weight)).to(ctx.his_dtype)
        out = [grads.get(nm) for nm, _ in model.module.named_parameters(prefix="module")]
        return (None, g_his, g_x, g_v, None, None, None, gw, gb) + tuple(out)


def segno_graph_train(model, his, x, v, edge_attr, T, graph):
    """SEGNO.forward (one input) on any edge list: embedding + T substeps on the autograd tape."""
    params = [model.embedding.weight, model.embedding.bias] + [p for _, p in model.module.named_parameters()]
    return SEGNOGraphTrain.apply(model, his, x, v, edge_attr, T, graph, *params)
