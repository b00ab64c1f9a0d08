"""Host logic of graphs of mixed sizes in one batch (graph.RaggedBatch, graph.neighbor_graph_ragged, the
sizes= argument of harness.prepare_inputs_graph / conserved_energy and of the general-graph rollout drivers),
CPU only: the exported symbols, the workspace query, the descriptor's arithmetic, what is refused before any
device work, and the numpy reference of the ragged builder against a float64 brute force."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import no_node_comparison_amd as pkg
from no_node_comparison_amd import _lib, graph, harness
from no_node_comparison_amd._lib import NonodeError
from tests._ragged_ref import ragged_brute_force_sets, ragged_neighbor_ref
from tests.conftest import ROOT

NEW = ("nonode_neighbor_graph_ragged_workspace_bytes", "nonode_neighbor_graph_ragged", "nonode_prepare_nodes_ragged",
       "nonode_prepare_inputs_bwd_ragged", "nonode_energy_ragged")
SIZES = (1, 2, 5, 37, 64, 65, 130, 3, 1)
SMALL = (3, 7, 1, 5)
NT = sum(SMALL)


def _egno(**kw):
    return pkg.EGNO(n_layers=2, in_node_nf=2, in_edge_nf=2, hidden_nf=64, with_v=True, num_modes=2, num_timesteps=4,
                    time_emb_dim=32, **kw)


def _segno(**kw):
    return pkg.SEGNO(in_node_nf=1, in_edge_nf=2, hidden_nf=64, n_layers=4, recurrent=True, **kw)


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
    q = L.nonode_neighbor_graph_ragged_workspace_bytes
    assert q(308, 130, 6) == (308 + 308 * 6) * 4
    assert q(8000, 1750, 16) == (8000 + 8000 * 16) * 4
    assert q(45, 37, 64) == (45 + 45 * 36) * 4      # k > n_max - 1
    assert q(3, 1, 4) == 3 * 4                      # graphs of one node: the degrees alone
    assert q(308, 130, 0) == 0 and q(308, 130, 65) == 0


def test_ragged_batch_arithmetic_on_the_host():
    b = graph.RaggedBatch(SIZES, "cpu")
    assert b.sizes == SIZES and b.n_graphs == 9 and b.n_total == 308 and b.n_max == 130
    assert b.graph_ptr.dtype == torch.int32 and b.graph_ptr.tolist() == [0, 1, 3, 8, 45, 109, 174, 304, 307, 308]
    assert b.graph_of.dtype == torch.int32 and b.graph_of.shape == (308,)
    assert b.graph_of.tolist() == [g for g, n in enumerate(SIZES) for _ in range(n)]
    assert [b.capacity(k) for k in (1, 6, 16, 64)] == [306, 1804, 4764, 17872]
    x = (np.random.RandomState(11).randn(308, 3) * 1.5).astype(np.float32)
    for k in (1, 6, 16, 64):
        assert ragged_neighbor_ref(x, SIZES, k)["cap"] == b.capacity(k)
    for same in (list(SIZES), np.array(SIZES), np.array(SIZES, dtype=np.int32), torch.tensor(SIZES)):
        assert graph.RaggedBatch(same, "cpu").sizes == SIZES
    assert graph.as_batch(b, torch.device("cpu")) is b


def test_sizes_are_checked_before_any_device_work():
    with pytest.raises(ValueError, match="on the host"):
        graph.RaggedBatch(torch.empty(3, dtype=torch.int64, device="meta"), "cpu")   # (a device tensor, no GPU needed)
    for bad in ((), [], (3, 0, 2), (3, -1), (2.0, 3.0), np.array([2.5, 3.0]), (True, 2), torch.tensor([1.0, 2.0])):
        with pytest.raises(ValueError, match="sizes"):
            graph.RaggedBatch(bad, "cpu")
    with pytest.raises(ValueError, match="2\\^30"):
        graph.RaggedBatch((2 ** 29, 2 ** 29), "cpu")
    z = torch.zeros(NT, 3)
    with pytest.raises(ValueError, match="sizes"):
        harness.prepare_inputs_graph(z, z, None, k=3, sizes=(3, 0, 7, 6))
    with pytest.raises(ValueError, match="sizes"):
        graph.neighbor_graph_ragged(z, (), 3)


def test_sizes_with_n_nodes_or_another_batch_size_is_refused():
    z = torch.zeros(NT, 3)
    q = torch.ones(NT)
    with pytest.raises(ValueError, match="not both"):
        harness.prepare_inputs_graph(z, z, 4, k=3, sizes=SMALL)
    with pytest.raises(ValueError, match="n_nodes"):
        harness.egno_rollout_graph(_egno(graph="any").eval(), z, z, q, 4, None, 2, k=3, sizes=SMALL)
    with pytest.raises(ValueError, match="batch_size"):
        harness.egno_rollout_graph(_egno(graph="any").eval(), z, z, q, None, 3, 2, k=3, sizes=SMALL)
    with pytest.raises(ValueError, match="batch_size"):
        harness.segno_rollout_graph(_segno(graph="any").eval(), z, z, q, 3, 2, k=3, sizes=SMALL)
    with pytest.raises(ValueError, match="batch_size"):
        harness.conserved_energy("charged", z, z, q, 3, sizes=SMALL)


def test_tensors_of_the_wrong_length_are_refused():
    z, short = torch.zeros(NT, 3), torch.zeros(NT - 1, 3)
    q = torch.ones(NT)
    with pytest.raises(ValueError, match="x must be"):
        graph.neighbor_graph_ragged(short, SMALL, 3)
    with pytest.raises(ValueError, match="x must be"):
        graph.neighbor_graph_ragged(torch.zeros(len(SMALL), max(SMALL), 3), SMALL, 3)
    with pytest.raises(ValueError, match="loc, vel must be"):
        harness.prepare_inputs_graph(short, short, None, k=3, sizes=SMALL)
    with pytest.raises(ValueError, match="charges"):
        harness.prepare_inputs_graph(z, z, None, torch.ones(NT + 1), k=3, sizes=SMALL)
    f = torch.zeros(4, NT, 3)
    with pytest.raises(ValueError, match="t_in"):
        harness.prepare_inputs_graph(f, f, None, q, torch.tensor([1, 2, 3]), k=3, sizes=SMALL)
    with pytest.raises(ValueError, match="loc, vel must be"):
        harness.egno_rollout_graph(_egno(graph="any").eval(), short, short, q, None, None, 2, k=3, sizes=SMALL)
    with pytest.raises(ValueError, match="timesteps_in"):
        harness.egno_rollout_graph(_egno(graph="any").eval(), z, z, q, None, None, 2, k=3, sizes=SMALL,
                                   timesteps_in=torch.tensor([1, 2, 3]))
    with pytest.raises(ValueError, match="loc, vel must be"):
        harness.segno_rollout_graph(_segno(graph="any").eval(), short, short, q, None, 2, k=3, sizes=SMALL)
    with pytest.raises(ValueError, match="loc must be"):
        harness.conserved_energy("charged", short, short, q, None, sizes=SMALL)


def test_several_rows_of_timesteps_out_are_refused_on_a_ragged_batch():
    z = torch.zeros(NT, 3)
    q = torch.ones(NT)
    t_out = torch.arange(8).repeat(len(SMALL), 1)
    with pytest.raises(ValueError, match="shared timesteps"):
        harness.egno_rollout_graph(_egno(graph="any").eval(), z, z, q, None, None, 2, k=3, sizes=SMALL,
                                   timesteps_out=t_out)
    with pytest.raises(ValueError, match="shared timesteps"):
        harness.egno_rollout_train_graph(_egno(graph="trainable").train(), z, z, q, None, None, 2, k=3, sizes=SMALL,
                                         timesteps_out=t_out)
    # EGNO.forward itself, on a NeighborGraph that carries a batch (host tensors: the constructor touches no device)
    b = graph.RaggedBatch(SMALL, "cpu")
    rows = torch.arange(NT, dtype=torch.int32)
    ng = graph.NeighborGraph(rows, rows.clone(), torch.arange(NT + 1, dtype=torch.int32), rows.clone(), None, batch=b)
    assert ng.n_nodes is None and ng.batch is b and ng.capacity == NT
    with pytest.raises(ValueError, match="shared timesteps"):
        _egno(graph="any").eval()(z, torch.zeros(NT, 2), ng, torch.zeros(NT, 2), v=z, loc_mean=z,
                                  timesteps_out=torch.arange(4).repeat(2, 1))


def test_host_tensors_have_no_cpu_path():
    z = torch.zeros(NT, 3)
    q = torch.ones(NT)
    with pytest.raises(NonodeError, match="no CPU path"):
        graph.neighbor_graph_ragged(z, SMALL, 3)
    with pytest.raises(NonodeError, match="no CPU path"):
        graph.neighbor_graph_ragged(z, graph.RaggedBatch(SMALL, "cpu"), 3)
    with pytest.raises(NonodeError, match="no CPU path"):
        harness.prepare_inputs_graph(z, z, None, q, k=3, sizes=SMALL)
    with pytest.raises(NonodeError, match="no CPU path"):
        harness.conserved_energy("charged", z, z, q, None, sizes=SMALL)
    with pytest.raises(NonodeError, match="no CPU path"):
        harness.egno_rollout_graph(_egno(graph="any").eval(), z, z, q, None, None, 2, k=3, sizes=SMALL)
    with pytest.raises(NonodeError, match="no CPU path"):
        harness.segno_rollout_graph(_segno(graph="any").eval(), z, z, q, None, 2, k=3, sizes=SMALL)


def test_the_existing_limits_still_raise_with_sizes():
    z = torch.zeros(NT, 3)
    q = torch.ones(NT)
    with pytest.raises(ValueError, match="k must be"):
        graph.neighbor_graph_ragged(z, SMALL, 65)
    with pytest.raises(ValueError, match="r_cut"):
        graph.neighbor_graph_ragged(z, SMALL, 3, 0.0)
    with pytest.raises(ValueError, match="exactly one of k"):
        harness.prepare_inputs_graph(z, z, None, sizes=SMALL)
    with pytest.raises(NotImplementedError, match="flat"):
        harness.egno_rollout_graph(_egno(graph="any", flat=True).eval(), z, z, q, None, None, 2, k=3, sizes=SMALL)
    with pytest.raises(NotImplementedError, match="num_inputs"):
        harness.egno_rollout_graph(_egno(graph="any", num_inputs=2).eval(), z, z, q, None, None, 2, k=3, sizes=SMALL)
    with pytest.raises(ValueError, match="bug_compat"):
        harness.segno_rollout_graph(_segno(graph="any", bug_compat=True).eval(), z, z, q, None, 2, k=3, sizes=SMALL)


@pytest.mark.parametrize("k,r_cut", [(4, None), (6, 1.2)])
def test_ragged_numpy_reference_agrees_with_a_float64_brute_force(k, r_cut):
    """Well-separated seeded points (no near-ties for float32 to break differently): per receiver the same
    neighbour set of its own graph, rows by ascending sender, the (-1, -1, p) tail up to sum cap_g."""
    sizes = (1, 23, 2, 9, 3)
    n = sum(sizes)
    x = np.random.RandomState(5).randn(n, 3).astype(np.float32) * 2.0
    ref = ragged_neighbor_ref(x, sizes, k, r_cut)
    want = ragged_brute_force_sets(x, sizes, k, r_cut)
    rp, col, rows = ref["row_ptr"], ref["col"], ref["rows"]
    assert ref["cap"] == sum(m * min(k, m - 1) for m in sizes) == graph.RaggedBatch(sizes, "cpu").capacity(k)
    assert col.shape == rows.shape == (ref["cap"],) and rp.shape == (n + 1,)
    for r in range(n):
        mine = col[rp[r]:rp[r + 1]]
        assert set(int(c) for c in mine) == want[r]
        assert np.all(np.diff(mine) > 0) and np.all(rows[rp[r]:rp[r + 1]] == r)
    assert ref["deg"][0] == 0                       # the graph of one node
    E = ref["E"]
    assert rp[-1] == E and np.all(col[E:] == -1) and np.all(rows[E:] == -1)
    assert np.array_equal(ref["eid"], np.arange(ref["cap"]))
    if r_cut is not None:
        assert E < ref["cap"]
