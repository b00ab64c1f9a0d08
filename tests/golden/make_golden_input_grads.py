"""Generate tests/golden/egno_input_grads.npz: the REFERENCE's autograd with respect to EGNO's inputs,
and through two chained rollout segments.

The reference's EGNO.forward (EGNO/model/egno.py:37-111) is plain torch, so it differentiates with
respect to x, v, h and loc_mean; its prepare_inputs (main_simulation_simple_no.py:311-339) keeps loc,
vel and loc_mean on the tape and detaches only nodes (:333) and edge_attr (:338). Seed-0 weights (the
constructor's initialisation, tests/golden/init_seed0.npz's "egno::" entries), B=2, N=5, T=10,
charged inputs with charges. Recorded:

  one::   one step: x, v, h, loc_mean are leaves that require grad; the loss of :273-276 against the
          next T frames; the four input gradients and the loss.
  two::   two chained segments as the loop of rollout_fn (:357-371) chains them, with gradients
          enabled: the reference's model, frame timesteps_in - 1 of each sample, the reference's
          prepare_inputs; the loss over all 2T predicted frames; the gradients with respect to the
          initial loc and vel [B, N, 3] and every parameter gradient. timesteps_in differs per sample
          (T and T - 3), so the second segment starts from different frames.

Test infrastructure only (build container). Data only; no reference source is copied. The reference
modules, their stubs and the input helpers come from make_golden.py. Re-run:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_input_grads.py
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as mg  # noqa: E402  (imports the reference and installs its stubs)

_np = mg._np


def _loss(loc_pred, loc_true, T, B, N):
    """main_simulation_simple_no.py:268-276 on T-major rows [T*BN, 3] against loc_true [B, N, T, 3]."""
    pred = loc_pred.reshape(T, -1, 3).transpose(0, 1)
    pred = mg._to_dense_batch(pred, torch.arange(B).repeat_interleave(N))[0]
    losses = torch.nn.MSELoss(reduction="none")(pred, loc_true[:, :, :pred.size(2)]).mean((0, 1, 3))
    return losses.mean()


def main(B=2, N=5, T=10, traj_len=2):
    loc_all, vel_all, q = mg.charged_trajectories(B, N)
    start = 20
    loc0 = torch.tensor(np.ascontiguousarray(loc_all[:, start]))
    vel0 = torch.tensor(np.ascontiguousarray(vel_all[:, start]))
    charges = torch.tensor(q)
    eao = mg.edge_attr_o(q).reshape(-1, 1)
    edges = mg.full_edges(B, N)
    torch.manual_seed(0)
    model = mg.EGNO(n_layers=4, in_node_nf=2, in_edge_nf=2, hidden_nf=64, with_v=True, num_modes=2,
                    num_timesteps=T, time_emb_dim=32)
    model.train()
    fx = {f"wsum::{k}": np.array(float(v.double().sum())) for k, v in model.state_dict().items()}
    fx.update({"cfg::B": np.array(B), "cfg::N": np.array(N), "cfg::T": np.array(T),
               "cfg::traj_len": np.array(traj_len), "raw::loc": _np(loc0), "raw::vel": _np(vel0),
               "raw::charges": q, "raw::edge_attr_o": _np(eao), "in::row": _np(edges[0]), "in::col": _np(edges[1])})

    # ---- one step: gradients of the loss with respect to x, v, h, loc_mean ----
    x, v, ea, nodes, lm = mg.egno_main.prepare_inputs(loc0, vel0, eao, edges, N, 1, charges)
    x, v, h, lm = (t.detach().clone().requires_grad_(True) for t in (x, v, nodes, lm))
    t_out = torch.arange(1, T + 1).repeat(B, 1)
    loc_true = torch.tensor(loc_all[:, start + 1:start + 1 + T]).transpose(1, 2)   # [B, N, T, 3]
    model.zero_grad()
    xp, _, _ = model(x, h, edges, ea, v=v, loc_mean=lm, timesteps_out=t_out)
    loss = _loss(xp, loc_true, T, B, N)
    loss.backward()
    fx.update({"one::x": _np(x), "one::v": _np(v), "one::h": _np(h), "one::loc_mean": _np(lm),
               "one::edge_attr": _np(ea), "one::t_out": _np(t_out), "one::loc_true": _np(loc_true),
               "one::loss": _np(loss), "one::g_x": _np(x.grad), "one::g_v": _np(v.grad), "one::g_h": _np(h.grad),
               "one::g_loc_mean": _np(lm.grad)})

    # ---- two chained segments (rollout_fn's loop :357-371, gradients enabled) ----
    loc, vel = loc0.clone().requires_grad_(True), vel0.clone().requires_grad_(True)
    t_in = torch.tensor([[T], [T - 3]])                                             # [B, 1]
    t_out_all = torch.arange(1, T * traj_len + 1).repeat(B, 1)
    bidx = torch.arange(B).unsqueeze(0).expand(t_in.size(1), -1)
    truth = torch.tensor(loc_all[:, start + 1:start + 1 + T * traj_len]).transpose(1, 2)   # [B, N, 2T, 3]
    model.zero_grad()
    lc, vl, eattr, nodes, lm = mg.egno_main.prepare_inputs(loc, vel, eao, edges, N, 1, charges)
    preds = []
    for i in range(traj_len):
        to = t_out_all[:, i * T:(i + 1) * T] - i * T
        lc, vl, _ = model(lc, nodes, edges, eattr, v=vl, loc_mean=lm, timesteps_out=to, timesteps_in=t_in)
        preds.append(lc)
        loc_seg, vel_seg = lc.view(T, B, N, 3), vl.view(T, B, N, 3)
        lc = loc_seg[t_in.T - 1, bidx].squeeze(0)
        vl = vel_seg[t_in.T - 1, bidx].squeeze(0)
        lc, vl, eattr, nodes, lm = mg.egno_main.prepare_inputs(lc, vl, eao, edges, N, t_in.size(1), charges)
    preds = torch.stack(preds)                                                      # [traj_len, T*BN, 3]
    # the loss of :273-276 over all traj_len*T frames (frame i*T + t of the truth against segment i's frame t)
    loss2 = _loss(preds.reshape(traj_len * T * B * N, 3), truth, traj_len * T, B, N)
    loss2.backward()
    fx.update({"two::t_in": _np(t_in), "two::t_out": _np(t_out_all), "two::loc_true": _np(truth),
               "two::loc_preds": _np(preds.reshape(traj_len * T, B * N, 3)), "two::loss": _np(loss2),
               "two::g_loc": _np(loc.grad), "two::g_vel": _np(vel.grad)})
    for k, p in model.named_parameters():
        fx["two::grad::" + k] = _np(p.grad) if p.grad is not None else np.zeros(tuple(p.shape), np.float32)
    np.savez_compressed(os.path.join(HERE, "egno_input_grads.npz"), **fx)
    print("wrote egno_input_grads.npz")


if __name__ == "__main__":
    main()
