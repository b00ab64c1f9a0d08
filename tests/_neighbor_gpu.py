"""What the GPU tests of the neighbour-graph searches share: uploads and the two bitwise comparisons."""
import numpy as np
import torch

DEV = "cuda"
NAMES = ("row_ptr", "col", "rows", "eid")
SENDER = ("srow_ptr", "seid", "valid")


def dev(a):
    return torch.tensor(np.ascontiguousarray(a)).to(DEV)


def same_graph(a, b, sender=False):
    for n in NAMES + (SENDER if sender else ()):
        assert torch.equal(getattr(a, n), getattr(b, n)), n
    assert a.capacity == b.capacity and a.n_nodes == b.n_nodes


def assert_ref(ng, ref):
    """ng against a numpy reference (tests/_neighbor_ref.py / tests/_ragged_ref.py), the -1 tail included."""
    got = {n: getattr(ng, n).cpu().numpy() for n in NAMES}
    E = int(got["row_ptr"][-1])
    assert ng.capacity == ref["cap"] and E == ref["E"]
    for n in NAMES:
        assert got[n].dtype == np.int32 and got[n].shape == ref[n].shape, n
        assert np.array_equal(got[n], ref[n]), n
    assert np.all(got["col"][E:] == -1) and np.all(got["rows"][E:] == -1)
