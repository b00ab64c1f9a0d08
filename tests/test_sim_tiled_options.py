"""Host logic of the tiled N-body simulators (nonode_sim_gravity_tiled / nonode_sim_charged_tiled, sim.py's
``kernel=`` and ``with_edges=``), CPU only: the exported symbols, the workspace query, what the entries refuse
before any device work, and what the Python layer raises on the host."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import no_node_comparison_amd as pkg
from no_node_comparison_amd import _lib, sim
from tests.conftest import ROOT

NEW = ("nonode_sim_tiled_shape", "nonode_sim_tiled_workspace_bytes", "nonode_sim_gravity_tiled",
       "nonode_sim_charged_tiled")
EINVAL = 1
NMAX = 1 << 20      # the stated bound on N (include/nonode.h)


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


def tile_shape():
    r, c = ctypes.c_int(0), ctypes.c_int(0)
    assert pkg.lib().nonode_sim_tiled_shape(ctypes.byref(r), ctypes.byref(c)) == 0
    return r.value, c.value


def test_tile_shape_is_reported():
    r, c = tile_shape()
    assert r % 64 == 0 and 64 <= r <= 1024 and c >= 1
    assert pkg.lib().nonode_sim_tiled_shape(None, None) == EINVAL


def test_workspace_query_needs_no_gpu():
    """two position buffers [3][S N] and the velocities [S N][3], float64."""
    q = pkg.lib().nonode_sim_tiled_workspace_bytes
    assert q(1, 20000) == 9 * 20000 * 8
    assert q(8, 1025) == 9 * 8 * 1025 * 8
    for bad in ((1, 0), (0, 100), (-1, 100), (1, -5), (1, NMAX + 1), (2048, NMAX), (2 ** 16, 2 ** 15)):
        assert q(*bad) == 0, bad
    assert q(1, NMAX) > 0 and q(2047, NMAX) > 0
    last = 0
    for n in (1, 2, 63, 64, 65, 1024, 1025, 20000, 100000, NMAX):
        assert q(1, n) > last
        last = q(1, n)
        assert q(1, n) <= q(2, n) <= q(3, n)


def _P(a):
    return ctypes.c_void_p(a)


def _call(entry, S=2, N=5, T=40, freq=10, null=None, ws_short=0, ws=0x90000):
    """The entry on dummy non-null host addresses (never dereferenced: every refusal comes first)."""
    L = pkg.lib()
    n_ptr = 6 if entry == "gravity" else 5
    ptrs = [_P(0x10000 * (k + 1)) for k in range(n_ptr)]
    if null is not None:
        ptrs[null] = _P(0)
    nbytes = L.nonode_sim_tiled_workspace_bytes(S, N) - ws_short
    fn = L.nonode_sim_gravity_tiled if entry == "gravity" else L.nonode_sim_charged_tiled
    return fn(S, N, T, freq, 0.001, 1.0, 0.1, *ptrs, _P(ws), max(nbytes, 0), _P(0))


@pytest.mark.parametrize("entry", ["gravity", "charged"])
def test_the_c_entries_refuse_before_any_launch(entry):
    L = pkg.lib()
    name = f"sim_{entry}_tiled"
    for kw, what in ((dict(T=45, freq=10), "sample_freq"), (dict(T=0), "T=0"), (dict(freq=0), "sample_freq"),
                     (dict(S=0), "S=0"), (dict(N=0), "N=0"), (dict(N=NMAX + 1), "N="), (dict(S=2048, N=NMAX), "S="),
                     (dict(null=0), "null"), (dict(null=2), "null"), (dict(null=4), "null"), (dict(ws=0), "null"),
                     (dict(ws_short=1), "workspace"), (dict(ws=0x90004), "aligned")):
        assert _call(entry, **kw) == EINVAL, kw
        msg = L.nonode_last_error().decode()
        assert what in msg and name in msg, (kw, msg)
    if entry == "gravity":
        assert _call(entry, null=5) == EINVAL and "null" in L.nonode_last_error().decode()
    else:
        assert _call(entry, N=1) == EINVAL and "N=1" in L.nonode_last_error().decode()   # charged needs a pair


def test_kernel_keyword_is_checked_on_the_host():
    g, c = sim.GravitySim(n_balls=1025), sim.ChargedParticlesSim(n_balls=1025, box_size=50.)
    import torch
    q, l0 = torch.zeros(1, 1025, dtype=torch.float64), torch.zeros(1, 3, 1025, dtype=torch.float64)
    calls = [lambda **kw: g.sample_trajectory_batch(T=20, sample_freq=10, **kw),
             lambda **kw: c.sample_trajectories(1, T=20, sample_freq=10, **kw),
             lambda **kw: c.integrate(q, l0, l0, 20, 10, **kw),
             lambda **kw: sim.generate_dataset(g, 1, 20, 10, **kw),
             lambda **kw: sim.generate_dataset(c, 1, 20, 10, **kw)]
    for call in calls:
        with pytest.raises(ValueError, match="kernel must be"):
            call(kernel="nope")
        with pytest.raises(ValueError, match="n_balls <= 1024"):
            call(kernel="resident")
    for small in (sim.GravitySim(n_balls=5).sample_trajectory_batch,
                  lambda **kw: sim.ChargedParticlesSim(n_balls=5).sample_trajectories(1, **kw)):
        with pytest.raises(ValueError, match="kernel must be"):
            small(kernel="Tiled")


def test_with_edges_and_kernel_are_in_the_signatures():
    p = inspect.signature(sim.ChargedParticlesSim.sample_trajectories).parameters
    assert p["with_edges"].default is True and p["kernel"].default is None
    for f in (sim.GravitySim.sample_trajectory_batch, sim.ChargedParticlesSim.integrate, sim.generate_dataset):
        assert inspect.signature(f).parameters["kernel"].default is None


def test_no_cpu_path_is_still_the_refusal_without_a_gpu():
    """Valid keywords pass every host check and reach the device check (device="cpu": on any machine)."""
    import torch
    for kernel in (None, "tiled"):
        with pytest.raises(_lib.NonodeError, match="no CPU path"):
            sim.GravitySim(n_balls=1100).sample_trajectory_batch(T=20, sample_freq=10, device="cpu", kernel=kernel)
        with pytest.raises(_lib.NonodeError, match="no CPU path"):
            sim.ChargedParticlesSim(n_balls=1100, box_size=50.).sample_trajectories(
                1, T=20, sample_freq=10, device="cpu", kernel=kernel, with_edges=False)
        q, l0 = torch.zeros(1, 1100, dtype=torch.float64), torch.zeros(1, 3, 1100, dtype=torch.float64)
        with pytest.raises(_lib.NonodeError, match="no CPU path"):
            sim.ChargedParticlesSim(n_balls=1100, box_size=50.).integrate(q, l0, l0, 20, 10, kernel=kernel)
    with pytest.raises(_lib.NonodeError, match="no CPU path"):
        sim.GravitySim(n_balls=5).sample_trajectory_batch(T=20, sample_freq=10, device="cpu", kernel="resident")
    if not torch.cuda.is_available():
        with pytest.raises(_lib.NonodeError, match="no CPU path"):
            sim.GravitySim(n_balls=1100).sample_trajectory_batch(T=20, sample_freq=10)


def test_the_reference_box_does_not_hold_a_large_draw():
    """The reference's assertion |loc| < 3 box_size stays: box_size = 5 trips it at n_balls = 1100."""
    np.random.seed(0)
    with pytest.raises(AssertionError):
        sim.ChargedParticlesSim(n_balls=1100).sample_trajectories(1, T=20, sample_freq=10, device="cpu")
