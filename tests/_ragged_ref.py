"""References for a batch of graphs of mixed sizes (graph.RaggedBatch), each built from the equal-size
reference applied per graph with B = 1, N = N_g. Helpers only.

ragged_neighbor_ref   tests/_neighbor_ref.neighbor_ref per graph, indices offset, concatenated, then the
                      (-1, -1, p) tail up to sum cap_g
ragged_prepare_inputs oracle.harness.prepare_inputs per graph on the edges whose receiver is in the graph
ragged_energy         oracle.harness.conserved_energy per graph
"""
import numpy as np

from oracle import harness as oh
from tests._neighbor_ref import brute_force_sets, neighbor_ref


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def ragged_neighbor_ref(x, sizes, k, r_cut=None):
    """x [n_total, 3] -> dict(row_ptr, col, rows, eid, E, cap, deg) as neighbor_ref gives it, for the batch."""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, 3)
    off = offsets(sizes)
    assert x.shape[0] == off[-1]
    col, rows, deg, cap = [], [], [], 0
    for g, n in enumerate(sizes):
        ref = neighbor_ref(x[off[g]:off[g + 1]], 1, n, k, r_cut)
        E = ref["E"]
        col.append(ref["col"][:E] + off[g])
        rows.append(ref["rows"][:E] + off[g])
        deg.append(ref["deg"])
        cap += ref["cap"]
    col, rows, deg = np.concatenate(col), np.concatenate(rows), np.concatenate(deg)
    E = col.size
    tail = np.full(cap - E, -1, dtype=np.int64)
    row_ptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    return dict(row_ptr=row_ptr, col=np.concatenate([col, tail]).astype(np.int32),
                rows=np.concatenate([rows, tail]).astype(np.int32), eid=np.arange(cap, dtype=np.int32), E=E, cap=cap,
                deg=deg.astype(np.int32))


def ragged_brute_force_sets(x, sizes, k, r_cut=None):
    """Per receiver, the set of its k nearest nodes of its own graph (within r_cut), float64 brute force."""
    off = offsets(sizes)
    out = []
    for g, n in enumerate(sizes):
        out += [{int(j) + int(off[g]) for j in s} for s in brute_force_sets(x[off[g]:off[g + 1]], 1, n, k, r_cut)]
    return out


def ragged_prepare_inputs(loc, vel, q, sizes, row, col):
    """loc, vel [n_total, 3], q [n_total] (or None), the list row, col (global indices, no edge across graphs)
    -> (edge_attr [E, 1 + (q is not None)], nodes, loc_mean) in loc's dtype, edge_attr in the list's order."""
    off = offsets(sizes)
    E = row.size
    ea = np.zeros((E, 2 if q is not None else 1), dtype=loc.dtype)
    nodes, lm = [], []
    for g, n in enumerate(sizes):
        sel = np.nonzero((row >= off[g]) & (row < off[g + 1]))[0]
        r, c = row[sel] - off[g], col[sel] - off[g]
        assert ((c >= 0) & (c < n)).all()
        lg, vg = loc[off[g]:off[g + 1]][None], vel[off[g]:off[g + 1]][None]
        qg = q[off[g]:off[g + 1]].reshape(1, n, 1) if q is not None else None
        eo = (qg.reshape(-1)[r] * qg.reshape(-1)[c])[:, None] if q is not None else np.zeros((sel.size, 0), loc.dtype)
        _, _, ea_g, nodes_g, lm_g = oh.prepare_inputs(lg, vg, eo, r, c, n, qg)
        ea[sel] = ea_g
        nodes.append(nodes_g)
        lm.append(lm_g)
    return ea, np.concatenate(nodes), np.concatenate(lm)


def ragged_energy(dataset, loc, vel, w, sizes):
    """loc, vel [n_total, 3], w [n_total] -> [G], oracle.harness.conserved_energy per graph."""
    off = offsets(sizes)
    return np.array([np.atleast_1d(oh.conserved_energy(dataset, loc[off[g]:off[g + 1]], vel[off[g]:off[g + 1]],
                                                       w[off[g]:off[g + 1]], 1))[0] for g in range(len(sizes))])
