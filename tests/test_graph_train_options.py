"""Host logic of EGNO(graph="trainable") (CPU only): the keyword value, what a forward refuses and in
which order before any device work, and the C symbols of the reverse pass."""
import ctypes
import os

import pytest
import torch

import no_node_comparison_amd as pkg
from no_node_comparison_amd import _lib, autograd
from no_node_comparison_amd._lib import NonodeError
from tests._graph_case import edge_features, sparse_graph

N = 37


def _egno(**kw):
    return pkg.EGNO(n_layers=2, in_node_nf=2, in_edge_nf=2, hidden_nf=64, with_v=True, num_modes=2, num_timesteps=4,
                    time_emb_dim=32, **kw)


def _args(edges=None, inputs=1):
    row, col = sparse_graph(N)
    edges = edges if edges is not None else [torch.tensor(row), torch.tensor(col)]
    ef = torch.tensor(edge_features(len(row)))
    lead = (inputs,) if inputs > 1 else ()
    if inputs > 1:
        ef = ef[None].repeat(inputs, 1, 1)
    kw = dict(v=torch.randn(*lead, N, 3), loc_mean=torch.zeros(*lead, N, 3))
    return [torch.randn(*lead, N, 3), torch.randn(*lead, N, 2), edges, ef], kw


def test_trainable_is_a_value_of_egno_only():
    assert _egno(graph="trainable").graph == "trainable"
    with pytest.raises(ValueError, match="graph"):
        pkg.SEGNO(in_node_nf=1, in_edge_nf=2, hidden_nf=64, n_layers=4, recurrent=True, graph="trainable")
    with pytest.raises(ValueError, match="graph"):
        _egno(graph="bogus")


def test_taped_forward_on_cpu_tensors_has_no_cpu_path():
    """The taped forward is accepted as far as the device check (graph="any" refuses it as inference only)."""
    a, kw = _args()
    with pytest.raises(NonodeError, match="no CPU path"):
        _egno(graph="trainable").train()(*a, **kw)
    m = _egno(graph="trainable").eval()   # an input on the tape, in eval mode
    a[0].requires_grad_(True)
    with pytest.raises(NonodeError, match="no CPU path"):
        m(*a, **kw)
    with torch.no_grad(), pytest.raises(NonodeError, match="no CPU path"):   # untaped: graph="any"'s entry
        m(*a, **kw)


def test_refusals_come_in_order():
    """flat=True, then multi-input training, then edge_fea's gradient, then the device, then the host list's
    range: each case holds every later fault as well."""
    row, col = sparse_graph(N)
    bad = col.copy()
    bad[7] = N
    bad_edges = [torch.tensor(row), torch.tensor(bad)]
    a, kw = _args(bad_edges, inputs=2)
    a[3].requires_grad_(True)
    with pytest.raises(NotImplementedError, match="flat"):
        _egno(graph="trainable", flat=True, num_inputs=2).train()(*a, **kw)
    with pytest.raises(NotImplementedError, match="num_inputs"):
        _egno(graph="trainable", num_inputs=2).train()(*a, **kw)
    a, kw = _args(bad_edges)
    a[3].requires_grad_(True)
    with pytest.raises(NotImplementedError, match="edge_fea"):
        _egno(graph="trainable").train()(*a, **kw)
    a[3] = a[3].detach()
    with pytest.raises(NonodeError, match="no CPU path"):
        _egno(graph="trainable").train()(*a, **kw)


@pytest.mark.parametrize("bad", [N, -1])
def test_host_list_with_an_index_out_of_range_raises(monkeypatch, bad):
    """(The device check of the tensors comes first, so it is switched off here to reach the edge check.)"""
    row, col = sparse_graph(N)
    col = col.copy()
    col[7] = bad
    a, kw = _args([torch.tensor(row), torch.tensor(col)])
    monkeypatch.setattr(_lib, "require_device", lambda *t: None)
    with pytest.raises(ValueError, match="outside"):
        _egno(graph="trainable").train()(*a, **kw)


def test_frame_groups_respect_the_cap():
    """The per-edge operand buffer of one group stays under the cap, down to one frame per group."""
    row = 400 * 4
    assert autograd.GRAPH_OPS_CAP_BYTES == 1 << 30
    assert autograd.graph_frame_groups(10, 128000) == [(0, 5), (5, 10)]          # 5 x 128000 rows: 0.95 GiB
    assert autograd.graph_frame_groups(10, 100, cap_bytes=3 * 100 * row) == [(0, 3), (3, 6), (6, 9), (9, 10)]
    assert autograd.graph_frame_groups(3, 100, cap_bytes=1) == [(0, 1), (1, 2), (2, 3)]
    assert autograd.graph_frame_groups(4, 0) == [(0, 4)]


def test_reverse_symbols_are_exported():
    so = os.path.join(os.path.dirname(pkg.__file__), "libnonode.so")
    L = ctypes.CDLL(so)
    for name in ("nonode_graph_edge_mask", "nonode_egnn_layer_graph_bwd_node_floats",
                 "nonode_egnn_layer_graph_bwd_edge_floats", "nonode_egnn_layer_graph_bwd"):
        assert hasattr(L, name), name
    L = pkg.lib()
    assert L.nonode_egnn_layer_graph_bwd_node_floats(3, 37) == 3 * 37 * 520
    assert L.nonode_egnn_layer_graph_bwd_edge_floats(3, 1000) == 3 * 1000 * 400
