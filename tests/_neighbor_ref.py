"""The numpy reference of graph.neighbor_graph (csrc/nonode_neighbor.hip), in the builder's float32
arithmetic taken literally, so that it is compared bitwise. Helpers only.

Per receiver i of a graph: d = x_i - x_j componentwise (float32), d2 = (dx*dx + dy*dy) + dz*dz on float32
arrays (every operation rounded on its own), candidates j != i with d2 <= r2_max true (r2_max =
float32(r_cut) * float32(r_cut), +inf without a cut-off; a NaN distance is no candidate), the first k of
np.lexsort((j, d2)), listed by ascending j.
"""
import numpy as np


def r2_of(r_cut):
    return np.float32(np.inf) if r_cut is None else np.float32(r_cut) * np.float32(r_cut)


def neighbor_ref(x, B, N, k, r_cut=None):
    """x [B*N, 3] -> dict(row_ptr [B*N + 1], col [cap], rows [cap], eid [cap], E, cap, deg [B*N]) int32,
    the builder's outputs with its (-1, -1, p) tail."""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(B * N, 3)
    r2 = r2_of(r_cut)
    kk = min(k, N - 1)
    cap = B * N * kk
    row_ptr = np.zeros(B * N + 1, dtype=np.int32)
    col, rows = [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(B * N):
            g0 = (r // N) * N
            xg = x[g0:g0 + N]
            d = x[r][None, :] - xg
            dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == np.float32
            j = np.arange(N)
            cand = (d2 <= r2) & (j != r - g0)
            jc, dc = j[cand], d2[cand]
            keep = np.sort(jc[np.lexsort((jc, dc))[:k]])
            col += [g0 + int(c) for c in keep]
            rows += [r] * len(keep)
            row_ptr[r + 1] = row_ptr[r] + len(keep)
    E = len(col)
    col = np.asarray(col + [-1] * (cap - E), dtype=np.int32)
    rows = np.asarray(rows + [-1] * (cap - E), dtype=np.int32)
    return dict(row_ptr=row_ptr, col=col, rows=rows, eid=np.arange(cap, dtype=np.int32), E=E, cap=cap,
                deg=np.diff(row_ptr))


def brute_force_sets(x, B, N, k, r_cut=None):
    """Per receiver, the set of its k nearest nodes (within r_cut) by a float64 brute force."""
    x = np.asarray(x, dtype=np.float64).reshape(B, N, 3)
    out = []
    for b in range(B):
        d2 = ((x[b][:, None, :] - x[b][None, :, :]) ** 2).sum(-1)
        for i in range(N):
            order = [j for j in np.argsort(d2[i], kind="stable") if j != i and
                     (r_cut is None or d2[i, j] <= float(r_cut) ** 2)]
            out.append({b * N + int(j) for j in order[:k]})
    return out


# ---- inputs that tell individually rounded distances from contracted ones ----
# With the receiver at the origin d = -x_j exactly, so d2 depends on the sender alone. The contracted form
# below is what a compiler emits for dist2 when it may fuse: fma(dz, dz, fma(dx, dx, fl(dy dy))). For
# components in [1, 2) both forms are computed exactly here (a 48-bit product plus a float32 of the same
# magnitude fits a float64), and they differ by one ulp for about a quarter of the points.

def d2_unfused(p):
    p = np.asarray(p, dtype=np.float32)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    return (x * x + y * y) + z * z


def d2_contracted(p):
    p = np.asarray(p, dtype=np.float32)
    x, y, z = (p[..., i].astype(np.float64) for i in range(3))
    yy = (p[..., 1] * p[..., 1]).astype(np.float64)
    t = (x * x + yy).astype(np.float32).astype(np.float64)
    return (z * z + t).astype(np.float32)


def _samples(seed, n=200000):
    p = (1.0 + np.random.RandomState(seed).rand(n, 3)).astype(np.float32)
    return p, d2_unfused(p), d2_contracted(p)


def tied_pairs(n_pairs, seed=0):
    """[(a, b)] float32 points whose individually rounded d2 from the origin TIE while the contracted
    d2 of b is the smaller: with a before b in index order, the order (d2, j) ranks a first and a
    contracting build ranks b first."""
    p, u, f = _samples(seed)
    order = np.argsort(u.view(np.uint32), kind="stable")
    out = []
    for i in np.nonzero(u[order][1:] == u[order][:-1])[0]:
        a, b = order[i], order[i + 1]
        if f[a] != f[b]:
            a, b = (a, b) if f[a] > f[b] else (b, a)
            out.append((p[a], p[b]))
            if len(out) == n_pairs:
                return out
    raise AssertionError("not enough tied pairs in the sample")


def cutoff_straddlers(n_each, seed=1):
    """[(point, r_cut, candidate)]: float32(r_cut)^2 equals the smaller of the point's individually
    rounded and contracted d2, which differ: `candidate` (d2_unfused <= r2) is what the contract says, and
    a contracting build says the opposite. n_each cases of either answer."""
    p, u, f = _samples(seed)
    out = {True: [], False: []}
    for i in np.nonzero(u != f)[0]:
        m = min(u[i], f[i])
        rc = np.sqrt(m, dtype=np.float32)
        for rc in (np.nextafter(rc, np.float32(0)), rc, np.nextafter(rc, np.float32(4))):
            if rc * rc == m:
                cand = bool(u[i] <= m)
                if len(out[cand]) < n_each:
                    out[cand].append((p[i], float(rc), cand))
                break
        if len(out[True]) == n_each and len(out[False]) == n_each:
            return out[True] + out[False]
    raise AssertionError("not enough straddling points in the sample")
