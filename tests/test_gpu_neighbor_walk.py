"""GPU test of the candidate walk both cell-list searches share (walk_segments, csrc/nonode_neighbor.hip). A receiver's
runs of cells go to groups of 16 lanes (four or more runs), 32 (two or three) or all 64 (one), so a mistake shows at a
count of runs per receiver and a length of run, not at a size of graph: small uniform clouds with forty nodes piled
onto one point, so that one cell holds a long run. Bit for bit, no tolerance."""
import functools

import numpy as np
import pytest

from no_node_comparison_amd import graph
from tests._neighbor_gpu import assert_ref, dev, same_graph
from tests._neighbor_ref import neighbor_ref
from tests._ragged_ref import ragged_neighbor_ref
from tests.test_neighbor_cells_options import _debug

pytestmark = pytest.mark.gpu
K = 16
CASES = {"300 at 0.3": ((300,), 0.3), "160 at 0.45": ((160,), 0.45), "24, 40, 160 at 0.45": ((24, 40, 160), 0.45)}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(x, sizes, r_cut, the numpy reference), computed once."""
    sizes, r_cut = CASES[name]
    rng = np.random.default_rng(0)
    x = rng.uniform(0, 1.5, (sum(sizes), 3)).astype(np.float32)
    x[:40] = x[0] + rng.normal(0, 1e-3, (40, 3)).astype(np.float32)
    x.setflags(write=False)
    ref = neighbor_ref(x, 1, sizes[0], K, r_cut) if len(sizes) == 1 else ragged_neighbor_ref(x, list(sizes), K, r_cut)
    return x, sizes, r_cut, ref


def _runs(name):
    """Per receiver (its number of runs, the length of its longest run), on the host through
    nonode_debug_neighbor_cells (the kernels' own grid and box functions): run (cx, cy) of the receiver's box holds
    its graph's nodes in the cells (cx, cy, z_lo .. z_hi)."""
    x, sizes, r_cut, _ = _case(name)
    d = _debug(x, sizes, r_cut)
    out, g0 = [], 0
    for g, n in zip(d["grid"], sizes):
        cnt = np.zeros((g, g, g), dtype=np.int64)
        np.add.at(cnt, tuple(d["cell"][g0:g0 + n].T), 1)
        for lo0, lo1, lo2, hi0, hi1, hi2 in d["range"][g0:g0 + n]:
            runs = cnt[lo0:hi0 + 1, lo1:hi1 + 1, lo2:hi2 + 1].sum(axis=2)
            out.append((runs.size, int(runs.max())))
        g0 += n
    return out


def test_the_inputs_hold_every_lane_grouping_with_a_run_that_loops():
    runs = [r for name in CASES for r in _runs(name)]
    assert any(n == 1 for n, _ in runs)                               # all 64 lanes on one run
    assert any(n in (2, 3) and longest > 32 for n, longest in runs)   # 32-lane groups, one of them loops
    # 16-lane groups whose last round is partly idle, one group looping while others have finished
    assert any(n >= 4 and n % 4 and longest > 16 for n, longest in runs)


@pytest.mark.parametrize("name", list(CASES))
def test_both_cell_searches_equal_brute_and_brute_the_numpy_reference(name):
    x, sizes, r_cut, ref = _case(name)
    xd = dev(x)
    batch = graph.RaggedBatch(sizes, xd.device)
    if len(sizes) == 1:
        build = lambda m: graph.neighbor_graph(xd, 1, sizes[0], K, r_cut, method=m, by_sender=True)   # noqa: E731
    else:
        build = lambda m: graph.neighbor_graph_ragged(xd, batch, K, r_cut, method=m, by_sender=True)   # noqa: E731
    brute = build("brute")
    assert_ref(brute, ref)
    assert 0 < ref["E"] < ref["cap"]
    for method in ("cells", "knn_cells"):
        same_graph(brute, build(method), sender=True)
