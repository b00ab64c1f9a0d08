"""Inputs of the k-NN cell search's exactness tests (graph.neighbor_graph(method="knn_cells"),
nonode_neighbor_graph_knn_cells), shared by tests/test_neighbor_knn_cells_options.py (CPU, against the numpy
reference through nonode_debug_neighbor_knn_cells) and tests/test_gpu_neighbor_knn_cells.py (GPU, against
method="brute"). Helpers only.

A family is a function (n, seed) -> (x [n, 3] float32, r_cut or None): n points of one kind, cut into graphs by the
caller. SIZES are the graph sizes at which the grid has g = 1, 1, 1, 2, 3, 4, 5, 6 cells per axis (g the largest
integer with 4 g^3 <= N), KS the row lengths asked for.
"""
import numpy as np

SIZES = (1, 2, 31, 32, 108, 257, 500, 1000)
KS = (1, 6, 16, 64)
RAGGED = (1, 3, 40, 500)


def gaussian(n, seed):
    return (np.random.RandomState(seed).randn(n, 3) * 1.5).astype(np.float32), None


def uniform(n, seed):
    return (np.random.RandomState(seed).rand(n, 3) * 10).astype(np.float32), None


def lattice(n, seed):
    """The first n points of an integer lattice (n = 512: 8^3): ties at the k-th place, D at lattice distances."""
    s = int(np.ceil(n ** (1.0 / 3.0) - 1e-9))
    return np.stack(np.meshgrid(*[np.arange(s)] * 3, indexing="ij"), -1).reshape(-1, 3)[:n].astype(np.float32), None


def coincident(n, seed):
    """A quarter of the nodes at one point (D = 0 for them), every fifth of the rest doubled."""
    x, _ = gaussian(n, seed)
    x[n // 4:n // 2] = x[0]
    twin = np.arange(n // 2 + 1, n, 5)
    x[twin] = x[twin - 1]
    return x, None


def all_coincident(n, seed):
    return np.repeat(gaussian(1, seed)[0], n, 0), None


def two_clusters(n, seed):
    """Two dense clusters far apart: the shell grows through empty cells for k above a cluster's size."""
    x = (np.random.RandomState(seed).randn(n, 3) * 0.05).astype(np.float32)
    x[n // 6:] += np.float32(1000.0)
    return x, None


def elongated(n, seed):
    return (np.random.RandomState(seed).rand(n, 3) * np.array([100, 0.01, 0.01])).astype(np.float32), None


def outlier(n, seed):
    x, _ = uniform(n, seed)
    x[n // 2] = 1e4
    return x, None


def huge(n, seed):
    return gaussian(n, seed)[0] * np.float32(1.5e8), None


def tiny(n, seed):
    return (uniform(n, seed)[0] * np.float32(1e-20)).astype(np.float32), None


def far_pair(n, seed):
    """Two nodes at +-3e38: the extent overflows (one cell), and their distances do."""
    x, _ = uniform(n, seed)
    if n >= 4:
        x[1], x[n - 2] = 3e38, -3e38
    return x, None


def nonfinite(n, seed):
    x, _ = uniform(n, seed)
    if n >= 8:
        x[2, 1], x[n // 2, 0], x[n // 2 + 1, 2], x[n - 1] = np.nan, np.inf, -np.inf, (np.inf, np.nan, 0.0)
    return x, None


def nonfinite_cut(n, seed):
    return nonfinite(n, seed)[0], 1.5


def many_nonfinite(n, seed):
    """More non-finite nodes than finite ones: fewer than k finite candidates without a cut-off."""
    x, _ = uniform(n, seed)
    x[::3, 0] = np.inf
    x[1::3, 1] = np.nan
    return x, None


def tight_cut(n, seed):
    return uniform(n, seed)[0], 0.8        # about 2 candidates per receiver at n = 1000


def loose_cut(n, seed):
    return uniform(n, seed)[0], 4.0        # some 200 candidates per receiver at n = 1000


def overflow_cut(n, seed):
    return gaussian(n, seed)[0], 1e30      # float32(r_cut)^2 = inf


FAMILIES = dict(gaussian=gaussian, uniform=uniform, lattice=lattice, coincident=coincident,
                all_coincident=all_coincident, two_clusters=two_clusters, elongated=elongated, outlier=outlier,
                huge=huge, tiny=tiny, far_pair=far_pair, nonfinite=nonfinite, nonfinite_cut=nonfinite_cut,
                many_nonfinite=many_nonfinite, tight_cut=tight_cut, loose_cut=loose_cut, overflow_cut=overflow_cut)


def cases():
    """[(id, family, sizes, k)]: every family at every size and every k, the lattice also at 8^3, and every family
    on mixed sizes with graphs of one and two nodes."""
    out = [(f"{fam}-N{n}-k{k}", fam, (n,), k) for fam in FAMILIES for n in SIZES for k in KS]
    out += [(f"lattice-N512-k{k}", "lattice", (512,), k) for k in KS]
    out += [(f"{fam}-mixed-k16", fam, (37, 1, 250, 2, 108), 16) for fam in FAMILIES]
    return out


def points(fam, sizes, seed=11):
    return FAMILIES[fam](int(sum(sizes)), seed)
