"""Fully connected, equal-size graph batches — the only topology the reference builds.

The reference materialises int64 edge lists per batch (EGNO/simulation/dataset_simple.py:64-71,
101-111; SEGNO/dataset_nbody.py:84-94): receiver row i, sender col j, ordered (b, i, j != i).
The kernels index that pattern implicitly, so the boundary checks that the caller's edge_index is
exactly it.

- Host (CPU) edge tensors are checked on the spot: ValueError otherwise.
- Device edge tensors are checked on the device without blocking the host (the reference's loop
  builds fresh edge tensors every batch, main_simulation_simple_no.py:217-218, so a check per new
  tensor is on the step's path): ``nonode_check_full_edges`` sets a device flag on any mismatch; the
  forward that used the edges ends with ``finish()``, which NaN-fills its outputs if the flag is set
  (``nonode_poison_if_flagged``) and copies the flag to pinned host memory behind an event. The next
  boundary call on that device that finds the event complete and the flag set raises ValueError
  (``sync_checks()`` waits for it). So a wrong edge list never yields silently wrong numbers: its
  forward's outputs are NaN, and the error is raised one call later at most.
- Edge lists made by ``full_edges`` on the device (the ``get_edges`` counterpart, one kernel) are valid
  by construction and enter the cache without a check.

General graphs (``EGNO`` / ``SEGNO`` with ``graph="any"``, inference): any other edge list becomes a CSR
by receiver (``csr``, one ``nonode_graph_build`` per edge tensor pair, cached the same way), which the
graph kernels of csrc/nonode_graph.hip walk. An index outside [0, n_nodes) raises ValueError at once for a
host list; for a device list it goes through the same flag / ``finish()`` / deferred ValueError mechanism,
with ``nonode_graph_build`` as the flag's writer (it drops the bad edge, so no kernel reads out of range).
Training on such a list (``EGNO(graph="trainable")``, ``SEGNO(graph="any", trainable=True)``) also needs the CSR by
sender and, for a device list, the mask of the edges the build kept (``csr_by_sender``, cached per edge tensor pair
as well).

Neighbour graphs (``neighbor_graph``, csrc/nonode_neighbor.hip): the k-NN / cut-off graph of an equal-size
batch, built on the device from the positions as a ``NeighborGraph``, which carries its own CSR (valid by
construction: no check, no cache entry) and goes wherever an edge list goes. A rollout rebuilds it every
segment (harness.egno_rollout_graph / segno_rollout_graph). Built with ``by_sender=True`` (or through
``NeighborGraph.with_sender_csr()``) it also carries the CSR by sender and the tail mask of the reverse pass,
made on the device from the padded list (``nonode_neighbor_by_sender``), so EGNO(graph="trainable") and
SEGNO(graph="any", trainable=True) train on it with nothing read back (harness.egno_rollout_train_graph /
segno_rollout_train_graph unroll a rollout on such graphs). Under a finite cut-off the builder can search a cell
list instead of all the nodes of a graph (``method="cells"``, ``nonode_neighbor_graph_cells``): the same arrays bit
for bit, O(cells the cut-off box touches) per receiver instead of O(N); ``method="auto"`` chooses by the size of
the largest graph (``neighbor_method``). ``method="knn_cells"`` (``nonode_neighbor_graph_knn_cells``) searches the
same cell list with a radius found per receiver, so it also builds the pure k-NN graph (``r_cut=None``) and a
graph under a loose cut-off without looking at every node: again the same arrays bit for bit; ``"knn_auto"``
chooses between it and ``"brute"`` by the size.

Graphs of mixed sizes in one batch (``RaggedBatch``, ``neighbor_graph_ragged``): the descriptor holds the sizes
on the host and their prefix sum and node -> graph map on the device, uploaded once; the builder, the node
featuriser, its reverse and the energy kernel read a graph's bounds from it where the equal-size calls divide
(the same kernels: equal sizes are the degenerate case and give the same bits). The CSR layer kernels need
nothing else: a mixed batch is just another CSR over n_total nodes, a graph of one node a row of degree 0.
The NeighborGraph of such a batch has ``n_nodes`` None and ``batch`` set. The embedding kernels map rows of
``timesteps_out`` to nodes by equal division, so a mixed batch takes shared timesteps (one row) only.
"""
import math
import operator
from collections import OrderedDict

import numpy as np
import torch

# validated edge tensors, keyed by address / version / shape. Each entry holds a reference to its
# tensors, so their memory cannot be freed and reused by a different edge list while the entry
# exists (a key built from addresses alone would then match a tensor it never checked).
_checked = OrderedDict()
_CACHE = 8
_states = {}


def _key(rows, cols, E, n_nodes):
    return (rows.data_ptr(), cols.data_ptr(), rows._version, cols._version, E, n_nodes, str(rows.device),
            rows.dtype, cols.dtype)


def _remember(key, B, N, rows, cols):
    _checked[key] = (B, N, rows, cols)
    _checked.move_to_end(key)
    while len(_checked) > _CACHE:
        _checked.popitem(last=False)


def _full_edges_host(B, N, device):
    """Pure elementwise index arithmetic (no boolean mask: nothing synchronises on a device)."""
    e = torch.arange(B * N * (N - 1), device=device)
    per = N * (N - 1)
    b, rem = e // per, e % per
    i, k = rem // (N - 1), rem % (N - 1)
    return b * N + i, b * N + k + (k >= i).to(torch.int64)


def full_edges(B, N, device="cpu"):
    """Edge list of B fully connected N-node graphs in the reference order (row, col), int64.
    On a ROCm device: one nonode_full_edges launch, and the pair is known valid (no check later)."""
    device = torch.device(device)
    if device.type != "cuda":
        return _full_edges_host(B, N, device)
    from . import _lib
    E = B * N * (N - 1)
    rows = torch.empty(E, dtype=torch.int64, device=device)
    cols = torch.empty(E, dtype=torch.int64, device=device)
    _lib.check(_lib.lib().nonode_full_edges(B, N, _lib.ptr(rows), _lib.ptr(cols), _lib.stream_of(rows)))
    _remember(_key(rows, cols, E, B * N), B, N, rows, cols)
    return rows, cols


def _split(edge_index):
    if isinstance(edge_index, NeighborGraph):
        return edge_index.rows, edge_index.col
    if isinstance(edge_index, (list, tuple)):
        if len(edge_index) != 2:
            raise ValueError("edge_index must be [rows, cols]")
        return edge_index[0], edge_index[1]
    if torch.is_tensor(edge_index) and edge_index.dim() == 2 and edge_index.shape[0] == 2:
        return edge_index[0], edge_index[1]
    raise ValueError("edge_index must be a pair of index tensors or a [2, E] tensor")


_NOT_FULL = ("edge_index is not the dataset's fully connected edge list (receiver i, sender j != i, ordered "
             "by sample, i, j); the MI355X kernels index that pattern implicitly")
_BAD_INDEX = "edge_index holds a node index outside [0, n_nodes)"

# general graphs (EGNO / SEGNO graph="any"): the CSR by receiver of an edge tensor pair, built once
# per pair on the device and cached under the keys of _checked, with the same bound; each entry holds
# a reference to the edge tensors for the same reason
_csr = OrderedDict()


class _DeviceChecks:
    """Pending device-side edge checks of one device (see the module docstring)."""

    def __init__(self, device):
        self.flag = torch.zeros(1, dtype=torch.int32, device=device)
        self.host = torch.zeros(1, dtype=torch.int32, pin_memory=True)
        self.event = None      # recorded after the flag's copy to self.host
        self.in_flight = []    # cache keys whose checks that copy covers
        self.unconfirmed = []  # cache keys checked after it (not covered by a copy yet)
        self.csr_keys = set()  # those of them whose flag writer is nonode_graph_build (csr below)

    def pending(self):
        return bool(self.in_flight or self.unconfirmed)

    def poll(self, block=False):
        """Read the flag copy if it has landed; raise ValueError if a check failed."""
        if self.event is None:
            return
        if block:
            self.event.synchronize()
        elif not self.event.query():
            return
        bad = int(self.host[0]) != 0
        self.event = None
        if not bad:
            self.csr_keys.difference_update(self.in_flight)
            self.in_flight = []
            return
        # which of the checked lists failed is not known: forget every unconfirmed one (a later use
        # re-checks it), clear the flag behind the checks already launched, report
        keys = self.in_flight + self.unconfirmed
        for k in keys:
            _checked.pop(k, None)
            _csr.pop(k, None)
            _csr_sender.pop(k, None)
        self.in_flight, self.unconfirmed = [], []
        self.flag.zero_()
        self.host.zero_()
        what = _NOT_FULL if not any(k in self.csr_keys for k in keys) else _BAD_INDEX
        self.csr_keys.clear()
        raise ValueError(what + " (found by the device-side check of an earlier call, whose outputs "
                         "were filled with NaN)")

    def launch(self, rows, cols, E, B, N):
        from . import _lib
        if rows.dtype != cols.dtype or rows.dtype not in (torch.int32, torch.int64):
            rows, cols = rows.to(torch.int64), cols.to(torch.int64)
        rows, cols = rows.contiguous(), cols.contiguous()
        _lib.check(_lib.lib().nonode_check_full_edges(_lib.ptr(rows), _lib.ptr(cols), rows.element_size(), E, B, N,
                                                      _lib.ptr(self.flag), _lib.stream_of(rows)))

    def finish(self, outs):
        """After a forward on edges with pending checks: NaN-fill its fp32 outputs if the flag is
        set, and copy the flag to the host behind an event (one copy in flight at a time)."""
        import ctypes
        from . import _lib
        bufs = [t for t in outs if torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32
                and t.is_contiguous()][:4]
        if bufs:
            P = ctypes.c_void_p * len(bufs)
            C = ctypes.c_longlong * len(bufs)
            _lib.check(_lib.lib().nonode_poison_if_flagged(_lib.ptr(self.flag), len(bufs),
                                                           P(*[t.data_ptr() for t in bufs]),
                                                           C(*[t.numel() for t in bufs]), _lib.stream_of(bufs[0])))
        if self.event is None and self.unconfirmed:
            self.host.copy_(self.flag, non_blocking=True)
            self.event = torch.cuda.Event()
            self.event.record()
            self.in_flight, self.unconfirmed = self.unconfirmed, []


def _state(device):
    st = _states.get(device)
    if st is None:
        st = _states[device] = _DeviceChecks(device)
    return st


def check_full_graph(edge_index, n_nodes):
    """Return (B, N) for an edge list of B fully connected N-node graphs covering n_nodes nodes.
    Host tensors: ValueError at once if edge_index is anything else. Device tensors: checked on the
    device (module docstring); a failed check raises ValueError at a later call."""
    rows, cols = _split(edge_index)
    E = rows.numel()
    if cols.numel() != E or n_nodes <= 0 or E % n_nodes:
        raise ValueError(f"edge_index with {E} edges is not a fully connected batch over {n_nodes} nodes")
    N = E // n_nodes + 1
    if n_nodes % N or N < 2:
        raise ValueError(f"edge_index with {E} edges is not a fully connected batch over {n_nodes} nodes")
    B = n_nodes // N
    if rows.device != cols.device:
        raise ValueError("edge_index rows and cols must be on one device")
    on_device = rows.is_cuda
    if on_device:
        _state(rows.device).poll()
    key = _key(rows, cols, E, n_nodes)
    hit = _checked.get(key)
    if hit is not None:
        _checked.move_to_end(key)
        return hit[0], hit[1]
    if on_device:
        st = _state(rows.device)
        st.launch(rows, cols, E, B, N)
        st.unconfirmed.append(key)
    else:
        r, c = _full_edges_host(B, N, rows.device)
        if not (torch.equal(rows.to(torch.int64), r) and torch.equal(cols.to(torch.int64), c)):
            raise ValueError(_NOT_FULL)
    _remember(key, B, N, rows, cols)
    return B, N


def finish(outs):
    """Pass a forward's outputs (a tuple of tensors) through the pending edge checks of their device
    (NaN-filled if one failed; see the module docstring). Returns outs."""
    dev = next((t.device for t in outs if torch.is_tensor(t) and t.is_cuda), None)
    if dev is not None:
        st = _states.get(dev)
        if st is not None and st.pending():
            st.finish(outs)
    return outs


def sync_checks(device=None):
    """Wait for the device-side edge checks issued so far and raise ValueError if one failed."""
    for dev, st in list(_states.items()):
        if device is not None and dev != torch.device(device):
            continue
        st.poll(block=True)
        if st.unconfirmed:        # checks launched after the last copy: copy the flag once more
            st.finish(())
            st.poll(block=True)


# ---- general graphs: any edge list, as a CSR by receiver ----

def known_full(edge_index, n_nodes):
    """(B, N) if this very edge tensor pair is already known to be the fully connected list (a hit in
    the cache of check_full_graph, which lists made by full_edges on the device enter), else None."""
    if isinstance(edge_index, NeighborGraph):
        return None
    rows, cols = _split(edge_index)
    hit = _checked.get(_key(rows, cols, rows.numel(), n_nodes))
    return None if hit is None else (hit[0], hit[1])


def check_host_range(edge_index, n_nodes):
    """Host (CPU) edge tensors: ValueError at once for an index outside [0, n_nodes). Device tensors
    are range-checked by nonode_graph_build (csr), without blocking the host."""
    rows, cols = _split(edge_index)
    if cols.numel() != rows.numel() or rows.dim() != 1 or cols.dim() != 1:
        raise ValueError("edge_index rows and cols must be 1-D tensors of one length")
    if rows.device != cols.device:
        raise ValueError("edge_index rows and cols must be on one device")
    if not rows.is_cuda and rows.numel():
        lo = min(int(rows.min()), int(cols.min()))
        hi = max(int(rows.max()), int(cols.max()))
        if lo < 0 or hi >= n_nodes:
            raise ValueError(_BAD_INDEX + f": found {lo if lo < 0 else hi} with n_nodes = {n_nodes}")


def csr(edge_index, n_nodes, device=None):
    """(row_ptr [n_nodes + 1], col [E], eid [E]) int32 device tensors: the edge list (row = receiver,
    col = sender, any topology; self loops and duplicate edges kept) as a CSR by receiver, each row
    ordered by (sender, original index), so the result is a pure function of the edge set. One
    nonode_graph_build per edge tensor pair (cached like check_full_graph's verdicts). A host list is
    checked on the spot (ValueError) and copied to `device` (default: the current ROCm device); a device
    list with an index outside [0, n_nodes) has that edge dropped, the device flag set (finish() then
    NaN-fills the forward's outputs) and ValueError raised by a later call or sync_checks().
    A NeighborGraph gives its own CSR: no launch, no cache entry (its -1 tail is no edge to check)."""
    if isinstance(edge_index, NeighborGraph):
        covered = edge_index.row_ptr.numel() - 1
        if n_nodes != covered:
            raise ValueError(f"csr: the NeighborGraph covers {covered} nodes, n_nodes = {n_nodes}")
        return edge_index.row_ptr, edge_index.col, edge_index.eid
    rows, cols = _split(edge_index)
    check_host_range(edge_index, n_nodes)
    E = rows.numel()
    if n_nodes <= 0 or E >= 2 ** 31:
        raise ValueError(f"csr: n_nodes = {n_nodes}, E = {E} (n_nodes >= 1, E < 2^31)")
    dev = rows.device if rows.is_cuda else torch.device(device if device is not None else "cuda")
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    st = _state(dev)
    st.poll()
    key = _key(rows, cols, E, n_nodes) + (str(dev),)
    hit = _csr.get(key)
    if hit is not None:
        _csr.move_to_end(key)
        return hit[0], hit[1], hit[2]
    from . import _lib
    r, c = rows, cols
    if r.dtype != c.dtype or r.dtype not in (torch.int32, torch.int64):
        r, c = r.to(torch.int64), c.to(torch.int64)
    r, c = r.to(dev).contiguous(), c.to(dev).contiguous()
    row_ptr = torch.empty(n_nodes + 1, dtype=torch.int32, device=dev)
    col = torch.empty(E, dtype=torch.int32, device=dev)
    eid = torch.empty(E, dtype=torch.int32, device=dev)
    L = _lib.lib()
    ws_bytes = L.nonode_graph_workspace_bytes(E, n_nodes)
    ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.int32, device=dev)
    _lib.check(L.nonode_graph_build(_lib.ptr(r), _lib.ptr(c), r.element_size(), E, n_nodes, _lib.ptr(row_ptr),
                                    _lib.ptr(col), _lib.ptr(eid), _lib.ptr(st.flag), _lib.ptr(ws), ws_bytes,
                                    _lib.stream_of(row_ptr)))
    if rows.is_cuda:   # (a host list was range-checked above: nothing pending for it)
        st.unconfirmed.append(key)
        st.csr_keys.add(key)
    _csr[key] = (row_ptr, col, eid, rows, cols)
    while len(_csr) > _CACHE:
        _csr.popitem(last=False)
    return row_ptr, col, eid


# ---- neighbour graphs built on the device (k-NN / cut-off; csrc/nonode_neighbor.hip) ----

class NeighborGraph:
    """A k-NN / cut-off graph of B equal-size graphs, built on the device by ``neighbor_graph``: int32
    device tensors ``row_ptr`` [B N + 1], ``col``, ``rows``, ``eid`` [capacity] (the CSR by receiver,
    rows ordered by sender, and the receiver of every entry), ``capacity`` = B N min(k, N - 1) (known on
    the host), ``n_edges`` = ``row_ptr[-1:]`` (the edge count, a one-element device view: reading it
    synchronises) and ``n_nodes`` = N. Entries at or past the edge count are (-1, -1): the graph kernels
    read only what the CSR names, so per-edge features for it are [capacity, .] and their tail is never read.

    It behaves as the pair [rows, col] (len 2, indexing, iteration), so it goes wherever an edge list goes:
    EGNO / SEGNO built with graph="any" (and EGNO(graph="trainable") off the tape), graph.csr (which
    returns this object's own CSR without a launch).

    Built with ``neighbor_graph(..., by_sender=True)``, or through ``with_sender_csr()``, it also carries the
    CSR by sender of the reverse pass: ``srow_ptr`` [B N + 1], ``seid`` [capacity] (each sender's positions,
    ascending; -1 at and past the edge count) and ``valid`` [capacity] (1 below the edge count, 0 for the
    tail), all None otherwise. With them EGNO(graph="trainable") and SEGNO(graph="any", trainable=True) train on it
    (graph.csr_by_sender returns them without a launch); no gradient flows through the choice of neighbours, which is discrete.

    A graph of a batch of mixed sizes (``neighbor_graph_ragged``) has ``n_nodes`` None and ``batch`` its
    RaggedBatch (None on an equal-size graph); ``capacity`` is then ``batch.capacity(k)``."""

    def __init__(self, rows, col, row_ptr, eid, n_nodes, *, srow_ptr=None, seid=None, valid=None, batch=None):
        self.rows, self.col, self.row_ptr, self.eid = rows, col, row_ptr, eid
        self.capacity = rows.numel()
        self.n_edges = row_ptr[-1:]
        self.n_nodes = n_nodes
        self.batch = batch
        self.srow_ptr, self.seid, self.valid = srow_ptr, seid, valid

    def has_sender_csr(self):
        return self.srow_ptr is not None and self.seid is not None and self.valid is not None

    def with_sender_csr(self):
        """This graph with its CSR by sender: self if it has one, else a NeighborGraph over the same
        tensors plus srow_ptr, seid, valid (one nonode_neighbor_by_sender call on the current stream,
        asynchronous, nothing read back). What lets a graph that came out of a rollout be trained on."""
        if self.has_sender_csr():
            return self
        srow_ptr, seid, valid = _sender_csr(self.rows, self.col, self.row_ptr)
        return NeighborGraph(self.rows, self.col, self.row_ptr, self.eid, self.n_nodes, srow_ptr=srow_ptr,
                             seid=seid, valid=valid, batch=self.batch)

    def __len__(self):
        return 2

    def __getitem__(self, i):
        return (self.rows, self.col)[i]

    def __iter__(self):
        return iter((self.rows, self.col))

    def edge_index(self):
        """The compacted int64 [rows[:E], col[:E]]. SYNCHRONISES the host (it reads the edge count): for
        inspection, tests and training, not for a rollout loop."""
        E = int(self.n_edges.item())
        return [self.rows[:E].to(torch.int64), self.col[:E].to(torch.int64)]


def neighbor_args(k, r_cut):
    """(k, r2_max) of a neighbour graph after the host-side checks: k an integer in [1, 64]; r_cut None
    (r2_max = +inf) or > 0, squared in float32. ValueError otherwise."""
    try:
        k = operator.index(k)
    except TypeError:
        k = 0
    if isinstance(k, bool) or not 1 <= k <= 64:
        raise ValueError(f"neighbor_graph: k must be an int in [1, 64], got {k!r}")
    r2 = math.inf
    if r_cut is not None:
        if not float(r_cut) > 0:
            raise ValueError(f"neighbor_graph: r_cut must be > 0 (or None), got {r_cut!r}")
        with np.errstate(over="ignore"):
            r2 = float(np.float32(r_cut) * np.float32(r_cut))
        if not r2 > 0:
            raise ValueError(f"neighbor_graph: r_cut = {r_cut!r} squares to zero in float32")
    return k, r2


# method="auto": the size of the largest graph from which the cell-list search is taken under a finite cut-off.
# Measured (profiles/graph/bench_cells.jsonl): the smallest measured N at which the
# cell list beat the brute-force search in every alternation, as it did at every larger measured N.
# Measured on the MI355X at about 12 candidates per receiver, k = 16: 10,000 (1.38 x there; the brute-force search
# is the faster one at 4,000 and below, where the cell list's five extra launches cost more than the search saves).
# None would mean not measured, and "auto" would be "brute".
CELLS_AUTO_MIN_NODES = 10000

# method="knn_auto": the size of the largest graph from which the k-NN cell search ("knn_cells") is taken, for any
# r_cut. Measured the same way (profiles/graph/bench_knn_cells.jsonl: uniform points,
# k = 16, no cut-off): the smallest measured N from which "knn_cells" beat "brute" in every alternation there and
# at every larger measured N. Measured on the MI355X: 10,000 (1.64 x there; at 4,000 and below, and at 8 x 1,000, the
# cell list's five extra launches cost more than the search saves). None would mean no such size, and "knn_auto"
# would be "brute".
KNN_CELLS_AUTO_MIN_NODES = 10000


def neighbor_method(method, r_cut, n_max=0):
    """The search a neighbour-graph build runs, "brute", "cells" or "knn_cells", from its method= argument, on the
    host and before any device work. None / "brute": one wave per receiver over all the nodes of its graph (any
    r_cut). "cells": the cell-list search, which needs a cut-off whose float32 square is finite (ValueError
    otherwise); the same arrays, bit for bit. "auto": "cells" when such a cut-off is given and the largest graph
    has at least CELLS_AUTO_MIN_NODES nodes, else "brute". "knn_cells": the k-NN search on the cell list, which
    finds its radius per receiver and so takes any r_cut, None included; the same arrays, bit for bit.
    "knn_auto": "knn_cells" when the largest graph has at least KNN_CELLS_AUTO_MIN_NODES nodes, else "brute".
    Anything else: ValueError."""
    if method is None or method == "brute":
        return "brute"
    if method == "knn_cells":
        return "knn_cells"
    if method == "knn_auto":
        return "knn_cells" if KNN_CELLS_AUTO_MIN_NODES is not None and n_max >= KNN_CELLS_AUTO_MIN_NODES else "brute"
    if method not in ("cells", "auto"):
        raise ValueError('neighbor_graph: method must be None, "brute", "cells", "auto", "knn_cells" or "knn_auto", '
                         f"got {method!r}")
    finite = False
    if r_cut is not None:
        with np.errstate(over="ignore"):
            finite = bool(np.isfinite(np.float32(r_cut) * np.float32(r_cut)))
    if method == "auto":
        return "cells" if finite and CELLS_AUTO_MIN_NODES is not None and n_max >= CELLS_AUTO_MIN_NODES else "brute"
    if r_cut is None:
        raise ValueError('neighbor_graph: method="cells" needs a cut-off (r_cut=None is the pure k-NN graph, which '
                         "only the brute-force search builds)")
    if not finite:
        raise ValueError(f'neighbor_graph: method="cells" needs a finite float32(r_cut)^2, got r_cut = {r_cut!r}')
    return "cells"


def _sender_csr(rows, col, row_ptr):
    """(srow_ptr, seid, valid) of a device-built graph: nonode_neighbor_by_sender on the padded list and its
    device-side count, on the stream of `rows`."""
    from . import _lib
    _lib.require_device(rows, col, row_ptr)
    dev = row_ptr.device
    cap, n_total = rows.numel(), row_ptr.numel() - 1
    srow_ptr = torch.empty(n_total + 1, dtype=torch.int32, device=dev)
    seid, valid = (torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(2))
    L = _lib.lib()
    ws_bytes = L.nonode_neighbor_by_sender_workspace_bytes(cap, n_total)
    ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.int32, device=dev)
    _lib.check(L.nonode_neighbor_by_sender(cap, n_total, _lib.ptr(rows), _lib.ptr(col), _lib.ptr(row_ptr),
                                           _lib.ptr(srow_ptr), _lib.ptr(seid), _lib.ptr(valid), _lib.ptr(ws),
                                           ws_bytes, _lib.stream_of(row_ptr)))
    return srow_ptr, seid, valid


def neighbor_graph(x, batch_size, n_nodes, k, r_cut=None, *, by_sender=False, method=None):
    """The k-nearest-neighbour graph (with r_cut: among the nodes within r_cut) of x [B N, 3], B = batch_size
    graphs of N = n_nodes consecutive rows, as a NeighborGraph: one nonode_neighbor_graph call, asynchronous,
    nothing read back. Receiver i keeps the min(k, candidates) nodes j != i of its graph with the smallest
    (d2, j), d2 = ((dx dx) + (dy dy)) + (dz dz) in individually rounded float32 operations and candidates
    the j with d2 <= float32(r_cut)^2 (r_cut=None: every j; a NaN distance is never a candidate). The result
    is a pure function of the positions, bitwise the same from run to run. k in [1, 64].
    by_sender=True also builds the CSR by sender (NeighborGraph.srow_ptr, seid, valid: one
    nonode_neighbor_by_sender call on the same stream), which training on the graph needs. The graph is a
    discrete function of x: nothing here is differentiable, and no gradient flows through it.
    method (neighbor_method): None / "brute" searches all N nodes per receiver; "cells" (a finite cut-off only)
    searches a cell list instead, one nonode_neighbor_graph_cells call, and returns the same arrays bit for bit,
    faster on large graphs; "auto" chooses by the size. "knn_cells" (any r_cut, None included) is the k-NN search
    on the cell list, one nonode_neighbor_graph_knn_cells call, the same arrays bit for bit; "knn_auto" chooses
    between it and "brute" by the size."""
    from . import _lib
    B, N = int(batch_size), int(n_nodes)
    k, r2 = neighbor_args(k, r_cut)
    method = neighbor_method(method, r_cut, N)
    if B < 1 or N < 1 or x.dim() != 2 or tuple(x.shape) != (B * N, 3):
        raise ValueError(f"neighbor_graph: x must be [batch_size * n_nodes, 3] = [{B * N}, 3], got {tuple(x.shape)}")
    _lib.require_device(x)
    return _build_neighbor_graph(x, k, r2, by_sender, B, N, None, method)


def _build_neighbor_graph(x, k, r2, by_sender, B, N, batch, method="brute"):
    """The builder's call behind neighbor_graph (B graphs of N rows; batch None) and neighbor_graph_ragged
    (batch a RaggedBatch; B, N unused), after their host checks: outputs, workspace, one C call, and the CSR
    by sender if asked. method "cells" / "knn_cells": the cell-list entries (equal sizes: null descriptors) in place
    of either."""
    from . import _lib
    x = _lib.f32(x)
    dev = x.device
    n_total, cap = (B * N, B * N * min(k, N - 1)) if batch is None else (batch.n_total, batch.capacity(k))
    row_ptr = torch.empty(n_total + 1, dtype=torch.int32, device=dev)
    col, eid, rows = (torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(3))
    L = _lib.lib()
    out = (_lib.ptr(row_ptr), _lib.ptr(col), _lib.ptr(eid), _lib.ptr(rows))
    G, n_max = (B, N) if batch is None else (batch.n_graphs, batch.n_max)
    desc = (None, None) if batch is None else (batch.graph_ptr, batch.graph_of)
    described = (G, n_total, n_max, k, cap, r2, _lib.ptr(desc[0]), _lib.ptr(desc[1]))
    # the entry, what its workspace query takes, its arguments before x
    if method in ("cells", "knn_cells"):
        name, sizes, lead = "nonode_neighbor_graph_" + method, (G, n_total, n_max, k), described
    elif batch is None:
        name, sizes, lead = "nonode_neighbor_graph", (B, N, k), (B, N, k, r2)
    else:
        name, sizes, lead = "nonode_neighbor_graph_ragged", (n_total, n_max, k), described
    ws_bytes = getattr(L, name + "_workspace_bytes")(*sizes)
    ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.int32, device=dev)
    _lib.check(getattr(L, name)(*lead, _lib.ptr(x), *out, _lib.ptr(ws), ws_bytes, _lib.stream_of(x)))
    n_nodes = N if batch is None else None
    if not by_sender:
        return NeighborGraph(rows, col, row_ptr, eid, n_nodes, batch=batch)
    srow_ptr, seid, valid = _sender_csr(rows, col, row_ptr)
    return NeighborGraph(rows, col, row_ptr, eid, n_nodes, srow_ptr=srow_ptr, seid=seid, valid=valid, batch=batch)


class RaggedBatch:
    """G graphs of mixed sizes in one batch, graph g the N_g consecutive rows from graph_ptr[g] on: what the
    device-side pieces (neighbor_graph_ragged, harness.prepare_inputs_graph / conserved_energy and the
    rollout drivers with sizes=) take instead of (batch_size, n_nodes). ``sizes`` is a HOST sequence of ints
    >= 1 (list, tuple, numpy array or CPU tensor; a device tensor raises ValueError, as reading it would
    synchronise). Attributes: ``sizes`` (tuple), ``n_graphs``, ``n_total``, ``n_max``, ``graph_ptr`` (int32
    [G + 1] on `device`, the exclusive prefix sum) and ``graph_of`` (int32 [n_total], node -> graph).
    Built once, with two small uploads here; everything that takes it reuses it, so a rollout loop uploads
    nothing and reads nothing back. device="cpu" is allowed (the arithmetic alone)."""

    def __init__(self, sizes, device):
        if torch.is_tensor(sizes):
            if sizes.device.type != "cpu":
                raise ValueError("RaggedBatch: sizes must be on the host (a list, tuple, numpy array or CPU tensor): "
                                 "reading a device tensor would synchronise")
            sizes = sizes.reshape(-1).tolist()
        elif isinstance(sizes, np.ndarray):
            sizes = sizes.reshape(-1).tolist()
        try:
            sizes = tuple(sizes)
            if any(isinstance(s, bool) for s in sizes):
                raise TypeError
            sizes = tuple(operator.index(s) for s in sizes)
        except TypeError:
            raise ValueError("RaggedBatch: sizes must be a sequence of ints") from None
        if not sizes or any(s < 1 for s in sizes):
            raise ValueError(f"RaggedBatch: sizes must hold at least one graph and every size must be >= 1, got {sizes!r}")
        if sum(sizes) >= 2 ** 30:
            raise ValueError(f"RaggedBatch: n_total = {sum(sizes)} (must be < 2^30)")
        self.sizes = sizes
        self.n_graphs, self.n_total, self.n_max = len(sizes), sum(sizes), max(sizes)
        ptr = np.zeros(self.n_graphs + 1, dtype=np.int32)
        np.cumsum(np.asarray(sizes, dtype=np.int64), out=ptr[1:])
        of = np.repeat(np.arange(self.n_graphs, dtype=np.int32), sizes)
        self.graph_ptr = torch.from_numpy(ptr).to(device)
        self.graph_of = torch.from_numpy(of).to(device)
        self.device = self.graph_ptr.device

    def capacity(self, k):
        """sum_g N_g min(k, N_g - 1): the length of a neighbour graph's padded list (host arithmetic)."""
        return sum(n * min(k, n - 1) for n in self.sizes)


def as_batch(sizes, device):
    """sizes as a RaggedBatch on `device`: itself if it is one (it must live there), else a new one."""
    if isinstance(sizes, RaggedBatch):
        if sizes.device != torch.device(device):
            raise ValueError(f"the RaggedBatch lives on {sizes.device}, the tensors on {device}")
        return sizes
    return RaggedBatch(sizes, device)


def neighbor_graph_ragged(x, batch, k, r_cut=None, *, by_sender=False, method=None):
    """neighbor_graph for a batch of mixed sizes: x [n_total, 3], batch a RaggedBatch (or a host sequence of
    sizes, wrapped: repeated callers pass the RaggedBatch). Receiver r of graph g keeps the min(k, N_g - 1,
    candidates) nodes j != r of its own graph with the smallest (d2, j), d2 and the candidates as in
    neighbor_graph; a graph of one node has rows of degree 0. One nonode_neighbor_graph_ragged call,
    asynchronous, nothing read back; bitwise a pure function of the positions and the sizes, and for equal
    sizes bitwise neighbor_graph's arrays. The NeighborGraph has n_nodes None, batch the descriptor and
    capacity == batch.capacity(k). method as in neighbor_graph ("auto" goes by the largest graph)."""
    from . import _lib
    k, r2 = neighbor_args(k, r_cut)
    neighbor_method(method, r_cut)
    if not isinstance(batch, RaggedBatch):
        batch = RaggedBatch(batch, x.device)
    method = neighbor_method(method, r_cut, batch.n_max)
    if x.dim() != 2 or tuple(x.shape) != (batch.n_total, 3):
        raise ValueError(f"neighbor_graph_ragged: x must be [n_total, 3] = [{batch.n_total}, 3], got {tuple(x.shape)}")
    _lib.require_device(x, batch.graph_ptr)
    if batch.device != x.device:
        raise ValueError(f"neighbor_graph_ragged: the RaggedBatch lives on {batch.device}, x on {x.device}")
    if batch.capacity(k) >= 2 ** 31:
        raise ValueError(f"neighbor_graph_ragged: capacity {batch.capacity(k)} (must be < 2^31)")
    return _build_neighbor_graph(x, k, r2, by_sender, 0, 0, batch, method)


# the second CSR of the reverse pass (EGNO graph="trainable"), cached per edge tensor pair like _csr
_csr_sender = OrderedDict()


def csr_by_sender(edge_index, n_nodes, device=None):
    """(srow_ptr [n_nodes + 1], seid [E], valid [E] or None) int32 device tensors for the reverse pass of
    the graph layer: the same edge list as a CSR by SENDER (nonode_graph_build with rows and cols swapped;
    each row ordered by (receiver, original index), seid the original edge index), and the mask of the
    edges the build kept (None for a host list, which was range-checked: every edge is kept). Cached per
    edge tensor pair, as csr is; a device list's bad index goes through csr's flag mechanism.
    A NeighborGraph that carries its sender CSR (neighbor_graph(by_sender=True) / with_sender_csr()) gives
    its own (srow_ptr, seid, valid): no launch, no cache entry. One without it raises ValueError."""
    if isinstance(edge_index, NeighborGraph):
        covered = edge_index.row_ptr.numel() - 1
        if n_nodes != covered:
            raise ValueError(f"csr_by_sender: the NeighborGraph covers {covered} nodes, n_nodes = {n_nodes}")
        if not edge_index.has_sender_csr():
            raise ValueError("csr_by_sender: this NeighborGraph carries no CSR by sender (its list has a -1 tail, "
                             "which nonode_graph_build does not take): build it with neighbor_graph(by_sender=True) "
                             "or call with_sender_csr()")
        return edge_index.srow_ptr, edge_index.seid, edge_index.valid
    rows, cols = _split(edge_index)
    row_ptr, _, eid = csr(edge_index, n_nodes, device)   # checks, polls, and the receiver CSR's cache
    dev = row_ptr.device
    E = rows.numel()
    key = _key(rows, cols, E, n_nodes) + (str(dev),)
    hit = _csr_sender.get(key)
    if hit is not None:
        _csr_sender.move_to_end(key)
        return hit[0], hit[1], hit[2]
    from . import _lib
    r, c = rows, cols
    if r.dtype != c.dtype or r.dtype not in (torch.int32, torch.int64):
        r, c = r.to(torch.int64), c.to(torch.int64)
    r, c = r.to(dev).contiguous(), c.to(dev).contiguous()
    srow_ptr = torch.empty(n_nodes + 1, dtype=torch.int32, device=dev)
    scol = torch.empty(E, dtype=torch.int32, device=dev)
    seid = torch.empty(E, dtype=torch.int32, device=dev)
    L = _lib.lib()
    ws_bytes = L.nonode_graph_workspace_bytes(E, n_nodes)
    ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.int32, device=dev)
    st = _state(dev)
    s = _lib.stream_of(srow_ptr)
    _lib.check(L.nonode_graph_build(_lib.ptr(c), _lib.ptr(r), r.element_size(), E, n_nodes, _lib.ptr(srow_ptr),
                                    _lib.ptr(scol), _lib.ptr(seid), _lib.ptr(st.flag), _lib.ptr(ws), ws_bytes, s))
    valid = None
    if rows.is_cuda and E:
        valid = torch.empty(E, dtype=torch.int32, device=dev)
        _lib.check(L.nonode_graph_edge_mask(_lib.ptr(row_ptr), _lib.ptr(eid), n_nodes, E, _lib.ptr(valid), s))
    _csr_sender[key] = (srow_ptr, seid, valid, rows, cols)
    while len(_csr_sender) > _CACHE:
        _csr_sender.popitem(last=False)
    return srow_ptr, seid, valid
