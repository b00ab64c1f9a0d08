"""The tiled N-body simulators (csrc/nonode_sim.hip, sim.py ``kernel="tiled"``) on the GPU.

Up to 1024 bodies they must reproduce the resident kernels bit for bit: the same per-pair helpers, every force sum
over j = 0 .. N-1 in ascending order, the same place for every rounding of the integrator. Above 1024 there is no
resident kernel, and they are held to the oracle (oracle/sim.py) at the bar tests/test_gpu_sim.py holds the resident
kernels to, SIMTOL = 1e-7 max-norm relative. That bar has margin to spare: permuting the particle order, which
changes the order of every force sum, moves the oracle's own results by <= 3e-15 relative at these sizes and
horizons."""
import ctypes

import numpy as np
import pytest
import torch

import no_node_comparison_amd as pkg
from oracle import sim as osim
from tests.conftest import check_rel
from tests.test_oracle_sim import charged_initial_states, gravity_initial_state

pytestmark = pytest.mark.gpu
SIMTOL = 1e-7
BOX = 50.          # holds every draw used here (loc_std grows as N ** (1/3); the reference asserts |loc| < 3 box)


def _tile_shape():
    r, c = ctypes.c_int(0), ctypes.c_int(0)
    assert pkg.lib().nonode_sim_tiled_shape(ctypes.byref(r), ctypes.byref(c)) == 0
    return r.value, c.value


R, C = _tile_shape()
EDGES = sorted({n for n in (R - 1, R + 1, C - 1, C + 1)})      # N on the tile's boundaries
GRAVITY_CASES = [(1, 2, 40, 20), (20, 3, 60, 20), (257, 1, 40, 20), (1024, 2, 20, 10)] + \
    [(n, 2, 40, 20) for n in EDGES if 1 <= n <= 1024]
CHARGED_CASES = [(n, 2 if n <= 200 else 1) for n in sorted({2, 5, 20, 200, 1024} | {n for n in EDGES if 2 <= n <= 1024})]


def _gravity(n, B, T, freq, kernel, seed=11, **kw):
    np.random.seed(seed + n)
    return pkg.sim.GravitySim(noise_var=0, n_balls=n).sample_trajectory_batch(T=T, sample_freq=freq, batch_size=B,
                                                                             kernel=kernel, **kw)


def _charged(n, S, T, freq, kernel, seed=23, **kw):
    np.random.seed(seed + n)
    return pkg.sim.ChargedParticlesSim(noise_var=0., n_balls=n, box_size=BOX).sample_trajectories(
        S, T=T, sample_freq=freq, kernel=kernel, **kw)


@pytest.mark.parametrize("n,B,T,freq", GRAVITY_CASES)
def test_gravity_tiled_equals_resident_bit_for_bit(n, B, T, freq):
    tiled, resident = _gravity(n, B, T, freq, "tiled"), _gravity(n, B, T, freq, "resident")
    assert tiled[0].shape == (B, T // freq, n, 3)
    for name, a, b in zip(("pos", "vel", "force", "mass"), tiled, resident):
        assert np.array_equal(a, b), (name, np.abs(a - b).max())
    assert np.isfinite(tiled[0]).all() and np.isfinite(tiled[2]).all()


@pytest.mark.parametrize("n,S", CHARGED_CASES)
def test_charged_tiled_equals_resident_bit_for_bit(n, S):
    T, freq = 40, 10          # T // freq - 1 = 3 samples
    tiled, resident = _charged(n, S, T, freq, "tiled"), _charged(n, S, T, freq, "resident")
    assert tiled[0].shape == (S, 3, 3, n)
    for name, a, b in zip(("loc", "vel", "edges", "charges"), tiled, resident):
        assert np.array_equal(a, b), (name, np.abs(a - b).max())
    assert np.isfinite(tiled[0]).all()


ABOVE = sorted({1025, 1100} | ({C + 1} if C + 1 > 1024 else set()))


@pytest.mark.parametrize("n,B", [(n, 2 if n == 1025 else 1) for n in ABOVE])
def test_gravity_above_1024_matches_oracle(n, B):
    T, freq = 40, 20
    pos, vel, force, mass = _gravity(n, B, T, freq, None)
    p0, v0, m = gravity_initial_state(11 + n, n, B, T, freq)
    assert np.array_equal(mass, m)
    P, V, F = osim.gravity_trajectory(p0, v0, m, T, freq)
    for name, got, want in (("pos", pos, P), ("vel", vel, V), ("force", force, F)):
        check_rel(f"gravity N={n} {name}", got, want, SIMTOL)


@pytest.mark.parametrize("n", ABOVE)
def test_charged_above_1024_matches_oracle(n):
    T, freq = 40, 10
    loc, vel, _, q = _charged(n, 1, T, freq, None, with_edges=False)
    (q0, l0, v0), = charged_initial_states(23 + n, n, 1, T, freq, box=BOX)
    assert np.array_equal(q[0], q0)
    L, V = osim.charged_trajectory(l0, v0, q0, T, freq)
    check_rel(f"charged N={n} loc", loc[0], L, SIMTOL)
    check_rel(f"charged N={n} vel", vel[0], V, SIMTOL)


def test_default_dispatch():
    """kernel=None: the resident kernel's bits at N = 1024, the tiled kernel's at N = 1025."""
    for n, same in ((1024, "resident"), (1025, "tiled")):
        for run in (lambda k: _gravity(n, 1, 20, 10, k), lambda k: _charged(n, 1, 30, 10, k)):
            for a, b in zip(run(None), run(same)):
                assert np.array_equal(a, b)
    with pytest.raises(ValueError):
        _gravity(1025, 1, 20, 10, "resident")


def test_with_edges_false():
    full = _charged(20, 2, 40, 10, None)
    lean = _charged(20, 2, 40, 10, None, with_edges=False)
    assert lean[2] is None and full[2].shape == (2, 20, 20)
    for k in (0, 1, 3):
        assert np.array_equal(full[k], lean[k])


def test_device_outputs_above_1024():
    n = 1100
    pos, vel, force, mass = _gravity(n, 1, 20, 10, None, as_numpy=False)
    for t in (pos, vel, force):
        assert t.is_cuda and t.dtype == torch.float64 and t.shape == (1, 2, n, 3)
    assert isinstance(mass, np.ndarray) and mass.shape == (1, n, 1)
    loc, v, edges, q = _charged(n, 1, 30, 10, None, as_numpy=False, with_edges=False)
    for t in (loc, v):
        assert t.is_cuda and t.dtype == torch.float64 and t.shape == (1, 2, 3, n)
    assert edges is None and q.shape == (1, n, 1)
    assert torch.isfinite(pos).all() and torch.isfinite(loc).all()
