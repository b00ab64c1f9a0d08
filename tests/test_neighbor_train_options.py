"""Host logic of training on device-built neighbour graphs (CPU only): the sender-CSR entry's symbols and
workspace query, a NeighborGraph that carries its CSR by sender, and what the taped forward, the taped
featuriser and the unrolled training driver refuse before any device work."""
import os
import re
import subprocess

import pytest
import torch

import no_node_comparison_amd as pkg
from no_node_comparison_amd import _lib, graph, harness
from no_node_comparison_amd._lib import NonodeError
from tests.conftest import ROOT
from tests.test_neighbor_options import B, N, _egno, _host_graph, _segno

NEW = ("nonode_neighbor_by_sender_workspace_bytes", "nonode_neighbor_by_sender")


def _host_graph_by_sender():
    """_host_graph (the directed ring i <- i + 1) with its CSR by sender, on host tensors."""
    g = _host_graph()
    n = B * N
    ar = torch.arange(n, dtype=torch.int32)
    seid = ((ar // N) * N + (ar % N + N - 1) % N).to(torch.int32)   # sender s sends to s - 1 only: position s - 1
    return graph.NeighborGraph(g.rows, g.col, g.row_ptr, g.eid, N, srow_ptr=torch.arange(n + 1, dtype=torch.int32),
                               seid=seid, valid=torch.ones(n, dtype=torch.int32))


def _forward(m, ng):
    n = B * N
    return m(torch.randn(n, 3), torch.randn(n, 2), ng, torch.randn(ng.capacity, 2), v=torch.randn(n, 3),
             loc_mean=torch.zeros(n, 3))


def test_new_symbols_are_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "nonode.h")).read()
    L = pkg.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r" T (nonode_[a-z0-9_]+)", out))
    for s in NEW:
        assert s in _lib.SYMBOLS
        assert re.search(r"^(?:size_t|int)\s+" + s + r"\(", header, re.M)
        assert s in exported and hasattr(L, s)


def test_workspace_query_needs_no_gpu():
    L = pkg.lib()
    assert L.nonode_neighbor_by_sender_workspace_bytes(8000 * 16, 8000) == (8000 + 8000 * 16) * 4
    assert L.nonode_neighbor_by_sender_workspace_bytes(0, 3) == 3 * 4   # N = 1: the out-degrees alone
    assert L.nonode_neighbor_by_sender_workspace_bytes(-1, 10) == 0
    assert L.nonode_neighbor_by_sender_workspace_bytes(10, 0) == 0
    assert L.nonode_neighbor_by_sender_workspace_bytes(10, -4) == 0


def test_constructor_keeps_its_positional_arguments():
    g = _host_graph()
    assert g.srow_ptr is None and g.seid is None and g.valid is None and not g.has_sender_csr()
    with pytest.raises(TypeError):
        graph.NeighborGraph(g.rows, g.col, g.row_ptr, g.eid, N, g.row_ptr)   # the new three are keyword-only
    gs = _host_graph_by_sender()
    assert gs.has_sender_csr() and gs.with_sender_csr() is gs
    assert len(gs) == 2 and gs[0] is gs.rows and gs[1] is gs.col


def test_taped_forward_takes_a_graph_with_its_sender_csr():
    """Fails at the parent commit, where every NeighborGraph is refused on the tape."""
    m = _egno(graph="trainable").train()
    with pytest.raises(NonodeError, match="no CPU path"):   # past the graph check: stopped by the host tensors
        _forward(m, _host_graph_by_sender())
    with pytest.raises(NotImplementedError, match=r"\.edge_index\(\)") as e:
        _forward(m, _host_graph())
    assert "by_sender=True" in str(e.value)


def test_other_refusals_of_the_taped_forward_keep_their_order():
    gs = _host_graph_by_sender()
    with pytest.raises(NotImplementedError, match="flat=True"):
        _forward(_egno(graph="trainable", flat=True).train(), gs)
    n = B * N
    m2 = _egno(graph="trainable", num_inputs=2).train()
    with pytest.raises(NotImplementedError, match="num_inputs=1"):
        m2(torch.randn(2, n, 3), torch.randn(2, n, 2), gs, torch.randn(2, gs.capacity, 2), v=torch.randn(2, n, 3),
           loc_mean=torch.zeros(2, n, 3), timesteps_in=torch.zeros(1, 2))
    m = _egno(graph="trainable").train()
    with pytest.raises(NotImplementedError, match="no gradient for edge_fea"):
        m(torch.randn(n, 3), torch.randn(n, 2), gs, torch.randn(gs.capacity, 2, requires_grad=True),
          v=torch.randn(n, 3), loc_mean=torch.zeros(n, 3))
    with pytest.raises(ValueError):
        _segno(graph="trainable")


def test_csr_by_sender_returns_the_graphs_own_tensors():
    gs = _host_graph_by_sender()
    before = len(graph._csr_sender)
    srow_ptr, seid, valid = graph.csr_by_sender(gs, B * N)
    assert srow_ptr is gs.srow_ptr and seid is gs.seid and valid is gs.valid
    assert len(graph._csr_sender) == before
    with pytest.raises(ValueError, match="by_sender=True"):
        graph.csr_by_sender(_host_graph(), B * N)
    with pytest.raises(ValueError, match="covers"):
        graph.csr_by_sender(gs, B * N + 1)


def test_with_sender_csr_has_no_cpu_path():
    with pytest.raises(NonodeError, match="no CPU path"):
        _host_graph().with_sender_csr()
    with pytest.raises(NonodeError, match="no CPU path"):
        graph.neighbor_graph(torch.zeros(B * N, 3), B, N, 3, by_sender=True)


def test_taped_featuriser_has_no_cpu_path():
    z = torch.zeros(B, N, 3)
    with pytest.raises(NonodeError, match="no CPU path"):
        harness.prepare_inputs_graph(z, z, N, k=3, tape=True)
    zg = torch.zeros(B, N, 3, requires_grad=True)
    with pytest.raises(NonodeError, match="no CPU path"):
        harness.prepare_inputs_graph(zg, z, N, k=3, tape=True)
    with pytest.raises(NonodeError, match="no CPU path"):
        harness.prepare_inputs_graph(zg, z, N, edges=_host_graph_by_sender(), tape=True)
    with pytest.raises(TypeError):
        harness.prepare_inputs_graph(z, z, N, None, None, 3, None, None, True)   # tape is keyword-only


def test_driver_refusals_come_before_any_device_work():
    z = torch.zeros(B, N, 3)
    q = torch.ones(B * N)
    drive = harness.egno_rollout_train_graph
    with pytest.raises(TypeError, match="EGNO"):
        drive(_segno(graph="any"), z, z, q, N, B, 2, k=3)
    for kind in ("full", "any"):
        with pytest.raises(ValueError, match='graph="trainable"'):
            drive(_egno(graph=kind).train(), z, z, q, N, B, 2, k=3)
    with pytest.raises(NotImplementedError, match="num_inputs"):
        drive(_egno(graph="trainable", num_inputs=2).train(), z, z, q, N, B, 2, k=3)
    with pytest.raises(NotImplementedError, match="flat"):
        drive(_egno(graph="trainable", flat=True).train(), z, z, q, N, B, 2, k=3)
    m = _egno(graph="trainable").train()
    for kw in (dict(), dict(k=3, edges=_host_graph_by_sender())):
        with pytest.raises(ValueError, match="exactly one of k"):
            drive(m, z, z, q, N, B, 2, **kw)
    with pytest.raises(ValueError, match="k must be"):
        drive(m, z, z, q, N, B, 2, k=65)
    with pytest.raises(NonodeError, match="no CPU path"):
        drive(m, z, z, q, N, B, 2, k=3)
    with pytest.raises(NonodeError, match="no CPU path"):
        drive(m, z, z, q, N, B, 2, edges=_host_graph_by_sender())
