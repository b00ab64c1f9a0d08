"""Host logic of SEGNO(graph="any", trainable=True) (CPU only): the keyword, what a taped forward refuses and
in which order before any device work, the C symbols of the training path, and the column assembly of the
first edge Linear's gradient for SEGNO's input order."""
import ctypes
import os

import pytest
import torch

import no_node_comparison_amd as pkg
from no_node_comparison_amd import _lib, autograd, graph
from no_node_comparison_amd._lib import NonodeError
from tests._graph_case import edge_features, sparse_graph

N = 37


def _segno(**kw):
    return pkg.SEGNO(in_node_nf=1, in_edge_nf=2, hidden_nf=64, n_layers=4, recurrent=True, **kw)


def _args(edges=None, inputs=1):
    """(his, x, edges, v, edge_attr) on sparse_graph(N); inputs > 1: the [BN, I, .] multi-input layout."""
    row, col = sparse_graph(N)
    edges = edges if edges is not None else [torch.tensor(row), torch.tensor(col)]
    mid = (inputs,) if inputs > 1 else ()
    return [torch.randn(N, *mid, 1), torch.randn(N, *mid, 3), edges, torch.randn(N, *mid, 3),
            torch.tensor(edge_features(len(row)))]


def _bare_neighbor_graph():
    """A NeighborGraph over host tensors without its CSR by sender (the refusal reads no tensor)."""
    z = torch.zeros(N * 4, dtype=torch.int32)
    return graph.NeighborGraph(z, z.clone(), torch.zeros(N + 1, dtype=torch.int32), z.clone(), N)


def test_trainable_is_a_keyword_of_graph_any():
    m = _segno(graph="any", trainable=True)
    assert m.trainable is True and m.graph == "any"
    assert _segno(graph="any").trainable is False and _segno().trainable is False
    with pytest.raises(ValueError, match="trainable"):
        _segno(graph="full", trainable=True)
    with pytest.raises(ValueError, match="trainable"):
        _segno(trainable=True)
    with pytest.raises(TypeError):   # keyword-only
        pkg.SEGNO(1, 2, 64, "cpu", torch.nn.SiLU(), 4, 1.0, True, False, False, True, True, False, None, False, "any", True)
    with pytest.raises(ValueError, match="graph"):   # EGNO's spelling stays refused
        _segno(graph="trainable")


def test_without_the_keyword_a_taped_forward_stays_inference_only():
    with pytest.raises(NotImplementedError, match="general graphs: inference only"):
        _segno(graph="any").train()(*_args())


def test_taped_forward_on_cpu_tensors_has_no_cpu_path():
    a = _args()
    with pytest.raises(NonodeError, match="no CPU path"):
        _segno(graph="any", trainable=True).train()(*a)
    with pytest.raises(NonodeError, match="no CPU path"):
        _segno(graph="any", trainable=True).train().forward_step(torch.randn(N, 64), *a[1:])
    m = _segno(graph="any", trainable=True).eval()   # an input on the tape, in eval mode
    a[1].requires_grad_(True)
    with pytest.raises(NonodeError, match="no CPU path"):
        m(*a)
    for agg in ("sum", "attn"):
        mm = _segno(graph="any", trainable=True, multiple_agg=agg).train()
        with pytest.raises(NonodeError, match="no CPU path"):
            mm(*_args(inputs=2), T=3, in_steps=torch.tensor([0, 2]))


@pytest.mark.parametrize("entry", ["forward", "forward_step", "multi"])
def test_refusals_come_in_order(entry):
    """edge_attr's gradient, then a NeighborGraph without its CSR by sender, then the device, then the host
    list's range: each case holds every later fault as well."""
    def call(m, a):
        if entry == "forward":
            return m(*a)
        if entry == "forward_step":
            return m.forward_step(torch.randn(N, 64), *a[1:])
        return m(*a, T=3, in_steps=torch.tensor([0, 2]))

    inputs = 2 if entry == "multi" else 1
    kw = dict(multiple_agg="sum") if entry == "multi" else {}
    m = _segno(graph="any", trainable=True, **kw).train()
    a = _args(_bare_neighbor_graph(), inputs)
    a[4] = torch.randn(N * 4, 2, requires_grad=True)
    with pytest.raises(NotImplementedError, match="edge_attr"):
        call(m, a)
    a[4] = a[4].detach()
    with pytest.raises(NotImplementedError, match="CSR by sender"):
        call(m, a)
    row, col = sparse_graph(N)
    bad = col.copy()
    bad[7] = N
    a = _args([torch.tensor(row), torch.tensor(bad)], inputs)
    with pytest.raises(NonodeError, match="no CPU path"):
        call(m, a)


@pytest.mark.parametrize("bad", [N, -1])
def test_host_list_with_an_index_out_of_range_raises(monkeypatch, bad):
    """(The device check of the tensors comes first, so it is switched off here to reach the edge check.)"""
    row, col = sparse_graph(N)
    col = col.copy()
    col[7] = bad
    a = _args([torch.tensor(row), torch.tensor(col)])
    monkeypatch.setattr(_lib, "require_device", lambda *t: None)
    with pytest.raises(ValueError, match="outside"):
        _segno(graph="any", trainable=True).train()(*a)


def test_training_symbols_are_exported_and_the_state_size_needs_no_gpu():
    so = os.path.join(os.path.dirname(pkg.__file__), "libnonode.so")
    L = ctypes.CDLL(so)
    names = ("nonode_segno_graph_train_state_bytes", "nonode_segno_forward_train_graph", "nonode_segno_layer_graph_bwd")
    for name in names:
        assert hasattr(L, name) and name in _lib.SYMBOLS, name
    L = pkg.lib()
    assert L.nonode_segno_graph_train_state_bytes(37, 4) == 4 * 37 * 266 * 4
    assert L.nonode_segno_graph_train_state_bytes(25600, 50) == 50 * 25600 * 266 * 4   # C5: 1.36 GB
    assert L.nonode_segno_graph_train_state_bytes(37, 0) == 0
    assert L.nonode_segno_graph_train_state_bytes(0, 4) == 0


def test_entries_refuse_bad_arguments_before_any_launch():
    L = pkg.lib()
    nul = [None] * 16
    rc = L.nonode_segno_layer_graph_bwd(0, 10, 2, *nul, 0.25, 1.0, 1, *[None] * 6)
    assert rc == 3 and b"segno_layer_graph_bwd" in L.nonode_last_error()     # NONODE_EUNSUPPORTED
    rc = L.nonode_segno_layer_graph_bwd(37, 10, 5, *nul, 0.25, 1.0, 1, *[None] * 6)
    assert rc == 3
    rc = L.nonode_segno_layer_graph_bwd(37, 10, 2, *nul, 0.25, 1.0, 1, *[None] * 6)
    assert rc == 1 and b"null pointer" in L.nonode_last_error()              # NONODE_EINVAL
    rc = L.nonode_segno_forward_train_graph(37, -1, 4, 2, *[None] * 8, 1.0, 1, *[None] * 4, 0, None)
    assert rc == 3
    rc = L.nonode_segno_forward_train_graph(37, 10, 4, 2, *[None] * 8, 1.0, 1, *[None] * 4, 0, None)
    assert rc == 1
    # the EGNO entry keeps its signature and its refusal of the SEGNO variant
    rc = L.nonode_egnn_layer_graph_bwd(_lib.VARIANT_SEGNO, 1, 37, 10, 2, 1, 0, 1, *[None] * 22)
    assert rc == 3 and b"EGNO only" in L.nonode_last_error()


@pytest.mark.parametrize("ne", [0, 2, 4])
def test_w1_columns_follow_each_variants_input_order(ne):
    """A hand-built operand product: entry (r, c) of e1 is 1000 r + c and of e1h 0.5 + 100 r + c, so every
    column of the assembled gradient names where it came from."""
    e1 = (1000.0 * torch.arange(128)[:, None] + torch.arange(72)[None, :]).float()
    e1h = (0.5 + 100.0 * torch.arange(128)[:, None] + torch.arange(64)[None, :]).float()
    s_col, e_cols = e1[:64, 65:66], e1[:64, 66:66 + ne]
    hi, hj = e1h[:64], e1h[64:]
    w = autograd.graph_w1_columns(_lib.VARIANT_SEGNO, e1, e1h, ne)   # [h_i, h_j, s, e]  (gcl.py:78)
    assert w.shape == (64, 129 + ne)
    assert torch.equal(w[:, :64], hi) and torch.equal(w[:, 64:128], hj)
    assert torch.equal(w[:, 128:129], s_col) and torch.equal(w[:, 129:], e_cols)
    w = autograd.graph_w1_columns(_lib.VARIANT_EGNO, e1, e1h, ne)    # [s, h_i, h_j, e]  (basic.py:152-154)
    assert w.shape == (64, 129 + ne)
    assert torch.equal(w[:, :1], s_col) and torch.equal(w[:, 1:65], hi)
    assert torch.equal(w[:, 65:129], hj) and torch.equal(w[:, 129:], e_cols)
    # the layout matches the module's own first Linear
    assert _segno(graph="any", trainable=True).module.edge_mlp[0].weight.shape == (64, 131)
