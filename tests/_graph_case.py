"""The seeded sparse test graphs of the general-graph (graph="any") tests and of
tests/golden/make_golden_graph.py, and their node inputs cut from the forward fixtures. Helpers only.

sparse_graph(n): n = 37 or 80 nodes (neither a multiple of the 16-receiver tile);
  - nodes 0 and 17 have no incoming edge (they still send);
  - node 5 has in-degree 40: more than two tiles' worth of padded steps for its tile-mates. Its senders
    are distinct while n - 1 >= 40 (n = 80); at n = 37 every other node once and four of them twice;
  - every other node, the last included, draws 1-6 distinct senders other than itself (the last node
    keeps an incoming edge: the reference's dense segment mean sizes its matrix by max(row) + 1);
  - extras: a self loop at node 3 and the edge (9 <- 4) twice;
  - the whole list is shuffled.
simple=True leaves out the self loop, the double edge and node 5's repeated senders (in-degree
min(40, n - 1)): a graph without duplicate edges, whose CSR does not depend on the list order.
"""
import numpy as np

ISOLATED = (0, 17)
HUB, HUB_DEG = 5, 40


def sparse_graph(n, seed=0, simple=False):
    """(row, col) int64 arrays: row = receiver, col = sender."""
    rng = np.random.RandomState(1000 + 7 * n + seed)
    rows, cols = [], []
    for i in range(n):
        if i in ISOLATED:
            continue
        others = np.array([j for j in range(n) if j != i])
        if i == HUB:
            send = list(rng.permutation(others)[:min(HUB_DEG, n - 1)])
            if not simple and len(send) < HUB_DEG:
                send += list(rng.permutation(others)[:HUB_DEG - len(send)])
        else:
            send = list(rng.permutation(others)[:rng.randint(1, 7)])
        rows += [i] * len(send)
        cols += [int(j) for j in send]
    if not simple:
        rows += [3, 9, 9]
        cols += [3, 4, 4]
    perm = rng.permutation(len(rows))
    return np.asarray(rows, dtype=np.int64)[perm], np.asarray(cols, dtype=np.int64)[perm]


def edge_features(E, ne=2, seed=0):
    """Random edge features, distinct per edge (a wrong original-edge index shows)."""
    return np.random.RandomState(77 + seed).randn(E, ne).astype(np.float32)


def egno_case(fx, n, seed=0, simple=False):
    """EGNO inputs on sparse_graph(n): the first n node rows of the egno_fwd fixture `fx`, one row of
    its timesteps_out (Bt = 1), random edge features."""
    row, col = sparse_graph(n, seed, simple)
    return dict(x=fx["in::x"][:n], h=fx["in::h"][:n], row=row, col=col, edge_fea=edge_features(len(row), 2, seed),
                v=fx["in::v"][:n], loc_mean=fx["in::loc_mean"][:n], t_out=fx["in::t_out"][:1])


def segno_case(fx, n, seed=0, simple=False):
    """SEGNO inputs on sparse_graph(n) from the segno_fwd fixture `fx` (his, x, v rows; random edge_attr)."""
    row, col = sparse_graph(n, seed, simple)
    return dict(his=fx["in::his"][:n], x=fx["in::x"][:n], row=row, col=col, v=fx["in::v"][:n],
                edge_attr=edge_features(len(row), 2, seed + 1))
