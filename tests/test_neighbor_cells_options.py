"""Host logic of the cell-list search for cut-off neighbour graphs (graph.neighbor_graph(method="cells"),
nonode_neighbor_graph_cells), CPU only: the exported symbols, the workspace query, what is refused before any
device work, the grid rule, and the covering property of the binning through nonode_debug_neighbor_cells,
which runs the very functions the kernels run (csrc/nonode_cells.h) on host arrays.

Covering: for every ordered pair (i, j) of a graph that the brute-force contract admits (d2_unfused(x_i - x_j)
<= float32(r_cut)^2, individually rounded float32 operations), the sender's cell lies inside the receiver's
searched range on all three axes. Nothing else is needed for the cell search to find the same candidates.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import no_node_comparison_amd as pkg
from no_node_comparison_amd import _lib, graph, harness
from tests._neighbor_ref import d2_unfused, r2_of
from tests.conftest import ROOT

NEW = ("nonode_neighbor_graph_cells_workspace_bytes", "nonode_neighbor_graph_cells", "nonode_debug_neighbor_cells")


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
    """(n_total (8 + min(k, n_max - 1)) + 8 G + 1) ints: sorted positions 4, degrees 1, rows at the pitch, the
    nodes' buckets 1, the cell table and its scan n_total + G each (+ 1), the bounding boxes 6 G."""
    q = pkg.lib().nonode_neighbor_graph_cells_workspace_bytes
    assert q(8, 8000, 1000, 16) == (8000 * (8 + 16) + 8 * 8 + 1) * 4 == 768260
    assert q(1, 20000, 20000, 16) == (20000 * 24 + 8 + 1) * 4
    assert q(5, 45, 37, 64) == (45 * (8 + 36) + 40 + 1) * 4      # k > n_max - 1
    assert q(3, 3, 1, 4) == (3 * 8 + 24 + 1) * 4                 # graphs of one node
    for bad in ((0, 8000, 1000, 16), (8, 0, 1000, 16), (8, 8000, 0, 16), (8, 8000, 8001, 16), (8, 8000, 1000, 0),
                (8, 8000, 1000, 65), (9, 8, 1, 4), (1, 2 ** 30, 4, 4)):
        assert q(*bad) == 0, bad


def _egno(**kw):
    return pkg.EGNO(n_layers=2, in_node_nf=2, in_edge_nf=2, hidden_nf=64, with_v=True, num_modes=2, num_timesteps=4,
                    time_emb_dim=32, **kw)


def _segno(**kw):
    return pkg.SEGNO(in_node_nf=1, in_edge_nf=2, hidden_nf=64, n_layers=4, recurrent=True, **kw)


def test_method_is_checked_on_host_tensors_before_any_device_work():
    """CPU tensors throughout: a NonodeError ("no CPU path") would mean require_device came first."""
    z = torch.zeros(12, 3)
    sizes = (3, 7, 2)
    for build in (lambda **kw: graph.neighbor_graph(z, 2, 6, 3, **kw),
                  lambda **kw: graph.neighbor_graph_ragged(z, sizes, 3, **kw)):
        with pytest.raises(ValueError, match="cut-off"):
            build(method="cells")
        with pytest.raises(ValueError, match="cut-off"):
            build(r_cut=None, method="cells")
        with pytest.raises(ValueError, match="finite"):
            build(r_cut=1e30, method="cells")
        with pytest.raises(ValueError, match="method must be"):
            build(r_cut=1.0, method="grid")
        with pytest.raises(ValueError, match="method must be"):
            build(method="grid")
        for ok in (None, "brute", "auto"):          # today's path: the device is what is missing
            with pytest.raises(_lib.NonodeError, match="no CPU path"):
                build(r_cut=1.0, method=ok)
        with pytest.raises(_lib.NonodeError, match="no CPU path"):
            build(r_cut=1.0, method="cells")
        with pytest.raises(_lib.NonodeError, match="no CPU path"):
            build(r_cut=1e30, method="auto")         # auto with a cut-off that has no finite square: brute
    assert graph.neighbor_method(None, None) == graph.neighbor_method("brute", 1.0) == "brute"
    assert graph.neighbor_method("cells", 1.5, 10) == "cells"
    assert graph.neighbor_method("auto", None, 10 ** 6) == "brute"
    assert graph.neighbor_method("auto", 1.5, 2) == "brute"
    # the measured crossover: cells from that size of the largest graph on
    n = graph.CELLS_AUTO_MIN_NODES
    assert isinstance(n, int) and n > 64
    assert graph.neighbor_method("auto", 1.5, n) == "cells" and graph.neighbor_method("auto", 1.5, n - 1) == "brute"
    assert graph.neighbor_method("auto", 1e30, n) == "brute"


def test_neighbor_method_in_the_harness_is_checked_before_any_device_work():
    z = torch.zeros(2, 6, 3)
    f = z.reshape(12, 3)
    q = torch.ones(12)
    edges = [torch.zeros(4, dtype=torch.int64), torch.ones(4, dtype=torch.int64)]
    me, mt = _egno(graph="any").eval(), _egno(graph="trainable").train()
    ms, mst = _segno(graph="any").eval(), _segno(graph="any", trainable=True).train()
    calls = [lambda **kw: harness.prepare_inputs_graph(z, z, 6, **kw),
             lambda **kw: harness.prepare_inputs_graph(z, z, 6, tape=True, **kw),
             lambda **kw: harness.prepare_inputs_graph(f, f, None, sizes=(5, 7), **kw),
             lambda **kw: harness.egno_rollout_graph(me, z, z, q, 6, 2, 2, **kw),
             lambda **kw: harness.egno_rollout_train_graph(mt, z, z, q, 6, 2, 2, **kw),
             lambda **kw: harness.segno_rollout_graph(ms, f, f, q, 2, 2, 3, **kw),
             lambda **kw: harness.segno_rollout_train_graph(mst, f, f, q, 2, 2, 3, **kw)]
    for call in calls:
        with pytest.raises(ValueError, match="neighbor_method goes with k"):
            call(edges=edges, neighbor_method="cells")
        with pytest.raises(ValueError, match="neighbor_method goes with k"):
            call(edges=edges, neighbor_method="brute")
        with pytest.raises(ValueError, match="cut-off"):
            call(k=3, neighbor_method="cells")
        with pytest.raises(ValueError, match="finite"):
            call(k=3, r_cut=1e30, neighbor_method="cells")
        with pytest.raises(ValueError, match="method must be"):
            call(k=3, r_cut=1.0, neighbor_method="grid")
        with pytest.raises(_lib.NonodeError, match="no CPU path"):
            call(k=3, r_cut=1.0, neighbor_method="cells")


def test_the_c_entry_refuses_before_any_launch():
    """Arguments refused on the host: nothing is launched, so no device is needed (the pointers are never read)."""
    L = pkg.lib()
    x = np.zeros((12, 3), dtype=np.float32)
    out = [np.zeros(64, dtype=np.int32) for _ in range(4)]
    ws = np.zeros(4096, dtype=np.int32)
    P = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else ctypes.c_void_p(0)   # noqa: E731
    gp = np.array([0, 5, 12], dtype=np.int32)
    go = np.repeat(np.arange(2, dtype=np.int32), [5, 7])

    def call(G=2, n_total=12, n_max=6, k=3, cap=36, r2=1.0, graph_ptr=None, graph_of=None, ws_bytes=ws.nbytes):
        return L.nonode_neighbor_graph_cells(G, n_total, n_max, k, cap, r2, P(graph_ptr), P(graph_of), P(x),
                                             *(P(o) for o in out), P(ws), ws_bytes, ctypes.c_void_p(0))

    EINVAL = 1
    for kw, what in ((dict(r2=float("inf")), "finite"), (dict(r2=float("nan")), "finite"), (dict(r2=0.0), "r2_max"),
                     (dict(k=65), "k in"), (dict(cap=37), "cap"), (dict(G=0), "G=0"),
                     (dict(graph_ptr=gp), "go together"), (dict(graph_of=go), "go together"),
                     (dict(n_max=5), "equal sizes"), (dict(ws_bytes=16), "workspace")):
        assert call(**kw) == EINVAL, kw
        assert what in L.nonode_last_error().decode(), (kw, L.nonode_last_error().decode())


# ---- the grid rule -------------------------------------------------------------------------------------------
def _debug(x, sizes, r_cut, equal=False):
    """nonode_debug_neighbor_cells on host arrays -> dict(rr, grid [G], box [G, 9], cell [n, 3], range [n, 6])."""
    L = pkg.lib()
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, 3)
    G, n = len(sizes), int(sum(sizes))
    assert x.shape[0] == n
    gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    rr = np.zeros(1, dtype=np.float32)
    grid = np.full(G, -7, dtype=np.int32)
    box = np.zeros((G, 9), dtype=np.float32)
    cell = np.full((n, 3), -7, dtype=np.int32)
    rng = np.full((n, 6), -7, dtype=np.int32)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)   # noqa: E731
    rc = L.nonode_debug_neighbor_cells(G, n, int(max(sizes)), float(r2_of(r_cut)),
                                       ctypes.c_void_p(0) if equal else P(gp), P(x), P(rr), P(grid), P(box), P(cell),
                                       P(rng))
    assert rc == 0, L.nonode_last_error().decode()
    return dict(rr=rr[0], grid=grid, box=box, cell=cell, range=rng)


@pytest.mark.parametrize("N", [1, 2, 7, 8, 63, 64, 1000])
def test_grid_rule(N):
    """g is a function of N alone with g^3 <= N (here: the largest g with 4 g^3 <= N), so a graph's cells and
    the bucket of its non-finite nodes fit the N + 1 table entries it owns; a graph of one node has g = 1."""
    x = np.random.RandomState(N).rand(N + 5, 3).astype(np.float32)
    d = _debug(x, (N, 5), 0.3)
    g = int(d["grid"][0])
    assert g >= 1 and g ** 3 <= N and g ** 3 + 1 <= N + 1
    assert g == max(1, max(c for c in range(1, 12) if 4 * c ** 3 <= max(N, 4)))
    assert 4 * (g + 1) ** 3 > N
    if N == 1:
        assert g == 1
    assert d["grid"][1] == 1                       # (the graph of 5)
    assert d["cell"].min() >= 0 and d["cell"][:N].max() <= g - 1
    # equal sizes (a null descriptor) is the same rule
    assert _debug(np.concatenate([x[:N], x[:N]]), (N, N), 0.3, equal=True)["grid"].tolist() == [g, g]


# ---- the covering property ------------------------------------------------------------------------------------
def _lattice8():
    return np.stack(np.meshgrid(*[np.arange(8)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)


def _cases():
    rs = np.random.RandomState(11)
    gauss = (rs.randn(1000, 3) * 1.5).astype(np.float32)
    uni = (rs.rand(1000, 3) * 10).astype(np.float32)
    out = [("gaussian", gauss, (1000,), 0.6), ("uniform", uni, (1000,), 1.5),
           ("uniform, mixed sizes", uni[:327], (1, 2, 37, 250, 37), 1.5)]
    out += [(f"lattice r_cut={r}", _lattice8(), (512,), r) for r in (1.0, 2.0, 1.5, float(np.sqrt(np.float32(3.0))))]
    out.append(("positions x 1.5e8", gauss * np.float32(1.5e8), (1000,), 0.6 * 1.5e8))
    out.append(("coordinates of 1e-20", (uni * np.float32(1e-20)).astype(np.float32), (1000,), 1.5e-20))
    co = gauss[:400].copy()
    co[100:200] = co[7]
    out.append(("100 coincident nodes", co, (400,), 0.6))
    out.append(("all coincident", np.repeat(gauss[:1], 64, 0), (64,), 0.5))
    out.append(("elongated", (rs.rand(1000, 3) * np.array([100, 0.01, 0.01])).astype(np.float32), (1000,), 0.5))
    outl = uni.copy()
    outl[17] = 1e4
    out.append(("one outlier at 1e4", outl, (1000,), 1.5))
    far = uni[:300].copy()
    far[3], far[250] = 3e38, -3e38
    out.append(("two nodes at +-3e38", far, (300,), 1.5))
    bad = uni[:300].copy()
    bad[5, 1], bad[77, 0], bad[78, 2] = np.nan, np.inf, -np.inf
    out.append(("a NaN and an inf", bad, (300,), 1.5))
    out.append(("a NaN and an inf, mixed sizes", bad, (100, 1, 199), 1.5))
    return out


CASES = _cases()


@pytest.mark.parametrize("name,x,sizes,r_cut", CASES, ids=[c[0] for c in CASES])
def test_every_admitted_pair_is_covered(name, x, sizes, r_cut):
    d = _debug(x, sizes, r_cut)
    r2 = r2_of(r_cut)
    assert np.isfinite(r2) and r2 > 0
    assert d["rr"] * d["rr"] > r2 and d["rr"] <= np.sqrt(np.float64(r2)) * 1.01 + 1e-37
    cell, rng = d["cell"], d["range"]
    fin = np.isfinite(x).all(1)
    # non-finite nodes have no cell and search nothing; finite ones have one inside the grid
    assert (cell[~fin] == -1).all() and (rng[~fin] == -1).all()
    off = np.concatenate([[0], np.cumsum(sizes)])
    pairs = 0
    for gi, n in enumerate(sizes):
        sl = slice(off[gi], off[gi + 1])
        g = d["grid"][gi]
        xg, cg, rg, fg = x[sl], cell[sl], rng[sl], fin[sl]
        assert (cg[fg] >= 0).all() and (cg[fg] <= g - 1).all()
        assert (rg[fg] >= 0).all() and (rg[fg] <= g - 1).all() and (rg[fg, :3] <= rg[fg, 3:]).all()
        assert (rg[fg, :3] <= cg[fg]).all() and (cg[fg] <= rg[fg, 3:]).all()      # a receiver searches its own cell
        with np.errstate(invalid="ignore", over="ignore"):
            d2 = d2_unfused(xg[:, None, :] - xg[None, :, :])                        # [i, j], the contract's float32
            adm = (d2 <= r2) & ~np.eye(n, dtype=bool)
        i, j = np.nonzero(adm)
        assert fg[i].all() and fg[j].all()                  # a non-finite node is in no admitted pair
        ok = (rg[i, :3] <= cg[j]).all(1) & (cg[j] <= rg[i, 3:]).all(1)
        assert ok.all(), f"{name}: graph {gi}: {np.count_nonzero(~ok)} of {i.size} admitted pairs not covered"
        pairs += i.size
    if "all rows empty" not in name:
        assert pairs > 0                                    # (the case does exercise the property)


def test_the_cases_degenerate_as_documented():
    """An extent that overflows puts every finite node into cell 0 (inv_w = 0 and the NaN of inf x 0); a cut-off
    wider than the cloud makes the cells cut-off wide, so every node is in cell 0 of a grid that still has g per
    axis; at the benchmark's density a search box is three cells wide."""
    name, x, sizes, r_cut = next(c for c in CASES if c[0].startswith("two nodes"))
    d = _debug(x, sizes, r_cut)
    assert (d["box"][0, 6:] == 0).all() and (d["cell"] == 0).all() and (d["range"] == 0).all()
    name, x, sizes, r_cut = next(c for c in CASES if c[0] == "uniform")
    wide = _debug(x, sizes, 40.0)
    assert (wide["cell"] == 0).all() and (wide["range"][:, :3] == 0).all()   # width = rr > extent: one cell in use
    d = _debug(x, sizes, r_cut)
    g = d["grid"][0]
    assert g == 6 and len({tuple(c) for c in d["cell"]}) > g ** 3 // 2    # 4 g^3 <= 1000: g = 6, cells in use
    span = d["range"][:, 3:] - d["range"][:, :3] + 1
    assert span.max() <= 4 and np.median(span) <= 3                        # a box is 3 cells wide, rarely 4
