"""The N-body simulators (csrc/nonode_sim.hip, sim.py) where tests/test_gpu_sim.py and tests/test_gpu_sim_tiled.py
do not look: packed batches on several workgroups, parameters off their defaults, a clamped step, odd sampling
schedules, the observation noise, and what ``integrate`` does with its inputs.

Every GPU result is held to the oracle (oracle/sim.py) at SIMTOL = 1e-7, max-norm relative; two runs of the same
kernel, and the tiled against the resident kernel, are held to np.array_equal. The cases, their oracle results and
the two CPU-side preconditions (the oracle moves by more than 1000 SIMTOL when the parameter does; it moves by less
than SIMTOL / 1000 when the particles are permuted) come from tests/sim_cases.py and are asserted again without a
GPU in tests/test_sim_inputs.py."""
import ctypes

import numpy as np
import pytest
import torch

import no_node_comparison_amd as pkg
from oracle import sim as osim
from tests import sim_cases as sc
from tests.conftest import check_rel
from tests.sim_cases import BOX, SIMTOL
from tests.test_oracle_sim import charged_initial_states, gravity_initial_state

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _tile_shape():
    r, c = ctypes.c_int(0), ctypes.c_int(0)
    assert pkg.lib().nonode_sim_tiled_shape(ctypes.byref(r), ctypes.byref(c)) == 0
    return r.value, c.value


R, C = _tile_shape()


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(DEV) for a in arrays]


def _np(tensors):
    return [t.cpu().numpy() for t in tensors]


def _charged(n, **kw):
    return pkg.sim.ChargedParticlesSim(n_balls=n, box_size=BOX, **kw)


def _check_charged(what, got, want):
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape, (what, got[0].shape, want[0].shape)
    if want[0].size:
        check_rel(f"{what} loc", got[0], want[0], SIMTOL)
        check_rel(f"{what} vel", got[1], want[1], SIMTOL)


def _check_gravity(what, got, want):
    for name, g, w in zip(("pos", "vel", "force"), got, want):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        check_rel(f"{what} {name}", g, w, SIMTOL)


# ---- A: batches across workgroups ----
AT, AFREQ = 30, 3


def _charged_batched_vs_alone(n, S, kernel):
    """The batched run; trajectory s of it equals the same state integrated alone, bit for bit; every trajectory
    matches the oracle. A dropped blockIdx.x * G (or s = blockIdx.x / tiles) term leaves every trajectory past the
    first workgroup unwritten or a copy of another: both checks see it."""
    q, l0, v0 = sc.stack_charged(charged_initial_states(300 + n, n, S, AT, AFREQ, box=BOX))
    sim = _charged(n)
    qd, ld, vd = _dev(q, l0, v0)
    loc, vel = _np(sim.integrate(qd, ld, vd, AT, AFREQ, kernel=kernel))
    assert loc.shape == (S, AT // AFREQ - 1, 3, n)
    for s in range(S):
        a_loc, a_vel = _np(sim.integrate(qd[s:s + 1], ld[s:s + 1], vd[s:s + 1], AT, AFREQ, kernel=kernel))
        assert np.array_equal(loc[s], a_loc[0]) and np.array_equal(vel[s], a_vel[0]), (n, S, s)
    _check_charged(f"charged N={n} S={S}", (loc, vel), sc.charged_oracle(q, l0, v0, AT, AFREQ))
    return loc, vel, (qd, ld, vd)


@pytest.mark.parametrize("n,S", [(2, 65), (3, 22), (5, 25), (7, 10), (20, 7), (32, 3), (33, 2)])
def test_charged_resident_batch_across_workgroups(n, S):
    """G = 64 // n trajectories per workgroup (1 above 32): (2, 65) three workgroups, the last holds one; (3, 22)
    G = 21 with lane 63 idle; (5, 25) G = 12; (7, 10) G = 9; (20, 7) G = 3, the last holds one; (32, 3); (33, 2)."""
    _charged_batched_vs_alone(n, S, "resident")


@pytest.mark.parametrize("n,S,resident_too", [(257, 3, True), (513, 2, True), (1025, 2, False)])
def test_charged_tiled_batch_across_tiles(n, S, resident_too):
    """Several receiver tiles and several trajectories at once: s = blockIdx.x / tiles with tiles > 1 and s > 0."""
    loc, vel, (qd, ld, vd) = _charged_batched_vs_alone(n, S, "tiled")
    if resident_too:
        r_loc, r_vel = _np(_charged(n).integrate(qd, ld, vd, AT, AFREQ, kernel="resident"))
        assert np.array_equal(loc, r_loc) and np.array_equal(vel, r_vel)


def _gravity_batched_vs_alone(n, B, kernel):
    p0, v0, m = gravity_initial_state(500 + n, n, B, AT, AFREQ)
    sim = pkg.sim.GravitySim(n_balls=n)
    pd, vd, md = _dev(p0, v0, m[:, :, 0])
    got = _np(sim.integrate(pd, vd, md, AT, AFREQ, kernel=kernel))
    assert got[0].shape == (B, AT // AFREQ, n, 3)
    for b in range(B):
        alone = _np(sim.integrate(pd[b:b + 1], vd[b:b + 1], md[b:b + 1], AT, AFREQ, kernel=kernel))
        for g, a in zip(got, alone):
            assert np.array_equal(g[b], a[0]), (n, B, b)
    _check_gravity(f"gravity N={n} B={B}", got, osim.gravity_trajectory(p0, v0, m, AT, AFREQ))


@pytest.mark.parametrize("n,B", [(1, 65), (20, 50), (32, 3), (33, 2)])
def test_gravity_resident_batch_across_workgroups(n, B):
    """(1, 65): G = 64, two workgroups, the last holds one; (20, 50): the reference's own batch, G = 3 and 17
    workgroups, the last holds 2 of 3."""
    _gravity_batched_vs_alone(n, B, "resident")


def test_gravity_tiled_batch_across_tiles():
    _gravity_batched_vs_alone(513, 3, "tiled")


# ---- B: parameters off their defaults ----
def _preconditions(sens, noise):
    assert sens > 1000 * SIMTOL, sens
    assert noise < SIMTOL / 1000, noise


@pytest.mark.parametrize("n,kernel", [(40, "resident"), (600, "tiled")])
@pytest.mark.parametrize("name", list(sc.CHARGED_PARAMS))
def test_charged_parameters_off_default(name, n, kernel):
    """interaction_strength = 1.7, neutral particles from charge_prob = (0.4, 0.2, 0.4), vel_norm = 0.8,
    loc_std = 1.5, and all of them, through sample_trajectories, against the oracle at the same values.
    Measured on the CPU, max-norm relative over the velocities, N = 40 (63 steps) / N = 600 (21 steps):
    the oracle at the moved value against the oracle at the default: strength 0.13 / 0.53, neutral made charged
    0.19 / 0.21, vel_norm 0.54 / 0.33, loc_std 0.10 / 0.38, all 0.68 / 0.41 (an ignored strength, or a kernel that
    treated q = 0 as charged, misses SIMTOL by six orders); a permutation of the particles: <= 3.4e-16."""
    simkw, cp = sc.CHARGED_PARAMS[name]
    (q, l0, v0), _, want, sens, noise = sc.charged_param_case(name, n)
    _preconditions(sens, noise)
    T, freq, S = sc.horizon(n)
    np.random.seed(sc.PSEED + n)
    kw = dict(charge_prob=cp) if cp else {}
    loc, vel, _, charges = _charged(n, **simkw).sample_trajectories(S, T=T, sample_freq=freq, kernel=kernel,
                                                                    with_edges=False, **kw)
    assert np.array_equal(charges[:, :, 0], q)
    _check_charged(f"charged {name} N={n}", (loc, vel), want)


@pytest.mark.parametrize("n,kernel", [(37, "resident"), (600, "tiled")])
@pytest.mark.parametrize("name", list(sc.GRAVITY_PARAMS))
def test_gravity_parameters_off_default(name, n, kernel):
    """interaction_strength = 2.5, softening = 0.03, dt = 0.004, and all three with loc_std = 2, through
    sample_trajectory_batch, against the oracle at the same values.
    Measured on the CPU, max-norm relative over the velocities, N = 37 (63 steps) / N = 600 (21 steps):
    moved against default: G 0.84 / 0.81, softening 0.30 / 0.53 (softening passed unsquared would be 0.03 against
    0.0009 under the root, further off than 0.1 is), dt 0.98 / 1.9, all 2.5 / 8.6; a permutation of the
    particles: <= 1.3e-13."""
    simkw = sc.GRAVITY_PARAMS[name]
    (p0, v0, m), _, want, sens, noise = sc.gravity_param_case(name, n)
    _preconditions(sens, noise)
    T, freq, B = sc.horizon(n)
    np.random.seed(sc.PSEED + n)
    *got, mass = pkg.sim.GravitySim(n_balls=n, **simkw).sample_trajectory_batch(T=T, sample_freq=freq, batch_size=B,
                                                                               kernel=kernel)
    assert np.array_equal(mass, m)
    _check_gravity(f"gravity {name} N={n}", got, want)


@pytest.mark.parametrize("n,kernel", [(37, "resident"), (600, "tiled")])
def test_gravity_coincident_bodies_without_softening(n, kernel):
    """softening = 0 with pos0[b, 5] = pos0[b, 4] (and at N = 600 bodies 511 and 512, either side of the sender
    chunk): the r2 > 0 guard is all that keeps the self pairs and the coincident pairs finite. Finite, and the
    oracle's. Measured on the CPU: softening 0 against 0.1 moves the velocities by 688 / 38 relative (N = 37 /
    600); a permutation of the particles by <= 9.2e-15."""
    (p0, v0, m), okw, want, sens, noise = sc.gravity_coincident_case(n)
    _preconditions(sens, noise)
    T, freq, _ = sc.horizon(n)
    got = _np(pkg.sim.GravitySim(n_balls=n, **okw).integrate(*_dev(p0, v0, m[:, :, 0]), T, freq, kernel=kernel))
    assert all(np.isfinite(g).all() for g in got)
    _check_gravity(f"gravity coincident N={n}", got, want)


# ---- C: a clamped step, bit for bit ----
def test_charged_clamped_steps_tiled_equals_resident():
    """tests/sim_cases.py clamp_case: two like-charged pairs at rest, 0.05 apart along the diagonal (bodies 3 and
    300) and 0.06 apart along x (bodies 511 and 512), among 600 bodies. Measured on the CPU: the clamp is active in
    19 of the 63 steps, and without it the velocities move by 0.37 relative."""
    (q, l0, v0), want, sens, active = sc.clamp_case()
    assert sens > 1000 * SIMTOL and active >= 10, (sens, active)
    sim, d = _charged(sc.CN), _dev(q, l0, v0)
    tiled = _np(sim.integrate(*d, sc.CT, sc.CFREQ, kernel="tiled"))
    resident = _np(sim.integrate(*d, sc.CT, sc.CFREQ, kernel="resident"))
    assert np.array_equal(tiled[0], resident[0]) and np.array_equal(tiled[1], resident[1])
    _check_charged("charged clamped tiled", tiled, want)
    _check_charged("charged clamped resident", resident, want)
    # the first sample follows CFREQ kicks from rest: a clamped component is at most CFREQ dt max_F = 0.7 (unclamped,
    # the diagonal pair alone would reach 1.6 per component and the x pair 1.9), negative on body 3, positive on 300
    first = resident[1][0, 0]
    cap = sc.CFREQ * 0.1 * (1 + 1e-12)
    assert np.all(first[:, 3] < -0.5) and np.all(first[:, 300] > 0.5) and np.all(np.abs(first[:, [3, 300]]) <= cap)
    assert first[0, 511] < -0.5 and first[0, 512] > 0.5 and np.all(np.abs(first[0, [511, 512]]) <= cap)


# ---- D: schedules ----
SCHEDULES = [(21, 1), (21, 3), (21, 7), (7, 7), (35, 5)]


@pytest.mark.parametrize("T,freq", SCHEDULES)
def test_charged_schedules(T, freq):
    """Odd sample_freq, sample_freq = 1, odd T, and T == sample_freq (no sample at all: empty [S, 0, 3, N] outputs,
    as the reference returns), resident at N = 20 and both kernels one body past a receiver tile. The tiled
    launcher then sets `row` on even and odd steps, i.e. samples out of both workspace buffers."""
    for n, kernels in ((20, ("resident",)), (R + 1, ("resident", "tiled"))):
        runs = []
        for kernel in kernels:
            np.random.seed(700 + n)
            loc, vel, _, charges = _charged(n).sample_trajectories(2, T=T, sample_freq=freq, kernel=kernel,
                                                                   with_edges=False)
            runs.append((loc, vel))
        q, l0, v0 = sc.stack_charged(charged_initial_states(700 + n, n, 2, T, freq, box=BOX))
        assert np.array_equal(charges[:, :, 0], q)
        want = sc.charged_oracle(q, l0, v0, T, freq)
        assert want[0].shape == (2, T // freq - 1, 3, n)
        for kernel, got in zip(kernels, runs):
            _check_charged(f"charged {kernel} N={n} T={T} freq={freq}", got, want)
        if len(runs) == 2:
            assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])


@pytest.mark.parametrize("T,freq", SCHEDULES)
def test_gravity_schedules(T, freq):
    """As above for gravity, which samples before the step: T == sample_freq is one sample, the initial state.
    The tiled kernel takes the sample of step t from workspace buffer t & 1: odd sample_freq reads both."""
    for n, kernels in ((20, ("resident",)), (R + 1, ("resident", "tiled"))):
        runs = []
        for kernel in kernels:
            np.random.seed(800 + n)
            *got, mass = pkg.sim.GravitySim(n_balls=n).sample_trajectory_batch(T=T, sample_freq=freq, batch_size=2,
                                                                              kernel=kernel)
            runs.append(got)
        p0, v0, m = gravity_initial_state(800 + n, n, 2, T, freq)
        assert np.array_equal(mass, m)
        want = osim.gravity_trajectory(p0, v0, m, T, freq)
        assert want[0].shape == (2, T // freq, n, 3)
        for kernel, got in zip(kernels, runs):
            _check_gravity(f"gravity {kernel} N={n} T={T} freq={freq}", got, want)
        if len(runs) == 2:
            for a, b in zip(*runs):
                assert np.array_equal(a, b)
        if T == freq:
            assert np.array_equal(runs[0][0][:, 0], p0) and np.array_equal(runs[0][1][:, 0], v0)


# ---- E: noise, exactly ----
NOISE = 0.01
EPS = np.finfo(np.float64).eps


def _assert_noise(name, noisy, clean, draw):
    """noisy == clean + NOISE * draw to within the two roundings of that expression (one multiply, one add)."""
    prod = NOISE * draw
    want = clean + prod
    bound = EPS * (np.abs(prod) + np.abs(want))
    assert noisy.shape == want.shape
    assert np.all(np.abs(noisy - want) <= bound), (name, np.abs(noisy - want).max())
    assert np.abs(noisy - clean).max() > NOISE       # the draws are there: max |z| > 1 among hundreds


def test_charged_noise_is_the_reference_draws():
    """S = 3: each simulation's two randn(T_save, 3, n) follow its own initial state, so the states and the noise
    of consecutive simulations interleave in the RNG stream."""
    n, S, T, freq, seed = 5, 3, 40, 10, 31
    out = {}
    for var in (0.0, NOISE):
        np.random.seed(seed)
        out[var] = _charged(n, noise_var=var).sample_trajectories(S, T=T, sample_freq=freq)
    states = charged_initial_states(seed, n, S, T, freq, box=BOX, with_noise=True)
    assert np.array_equal(out[0.0][3], out[NOISE][3]) and np.array_equal(out[NOISE][3][:, :, 0],
                                                                         np.stack([s[0][:, 0] for s in states]))
    _assert_noise("loc", out[NOISE][0], out[0.0][0], np.stack([s[3] for s in states]))
    _assert_noise("vel", out[NOISE][1], out[0.0][1], np.stack([s[4] for s in states]))


def test_gravity_noise_is_the_reference_draws():
    """Three randn(B, T_save, N, 3) after the velocities: for pos, vel and force, in that order."""
    n, B, T, freq, seed = 6, 2, 40, 10, 37
    out = {}
    for var in (0, NOISE):
        np.random.seed(seed)
        out[var] = pkg.sim.GravitySim(n_balls=n, noise_var=var).sample_trajectory_batch(T=T, sample_freq=freq,
                                                                                      batch_size=B)
    _, _, m = gravity_initial_state(seed, n, B, T, freq)       # leaves the RNG where the noise draws begin
    draws = [np.random.randn(B, T // freq, n, 3) for _ in range(3)]
    assert np.array_equal(out[0][3], m) and np.array_equal(out[NOISE][3], m)
    for k, name in enumerate(("pos", "vel", "force")):
        _assert_noise(name, out[NOISE][k], out[0][k], draws[k])


# ---- F: inputs ----
def test_non_contiguous_inputs_give_the_contiguous_result():
    n, S, T, freq = 20, 7, 30, 3
    q, l0, v0 = sc.stack_charged(charged_initial_states(900, n, S, T, freq, box=BOX))
    qd, ld, vd = _dev(q, l0, v0)
    lt, vt = (t.transpose(1, 2).contiguous().transpose(1, 2) for t in (ld, vd))    # [S, N, 3] storage
    qt = torch.stack([qd, qd], dim=2)[:, :, 0]
    assert not lt.is_contiguous() and not qt.is_contiguous() and torch.equal(lt, ld)
    for kernel in ("resident", "tiled"):
        want = _np(_charged(n).integrate(qd, ld, vd, T, freq, kernel=kernel))
        got = _np(_charged(n).integrate(qt, lt, vt, T, freq, kernel=kernel))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    p0, v0, m = gravity_initial_state(901, n, S, T, freq)
    pd, vd, md = _dev(p0, v0, m[:, :, 0])
    pt, vt = (t.transpose(1, 2).contiguous().transpose(1, 2) for t in (pd, vd))    # [B, 3, N] storage
    mt = torch.stack([md, md], dim=2)[:, :, 1]
    assert not pt.is_contiguous() and not mt.is_contiguous()
    for kernel in ("resident", "tiled"):
        want = _np(pkg.sim.GravitySim(n_balls=n).integrate(pd, vd, md, T, freq, kernel=kernel))
        got = _np(pkg.sim.GravitySim(n_balls=n).integrate(pt, vt, mt, T, freq, kernel=kernel))
        for g, w in zip(got, want):
            assert np.array_equal(g, w)


def test_refusals_come_before_any_launch_on_device_tensors():
    """float32, a wrong shape and mixed devices are refused for device tensors as for host ones
    (tests/test_sim_inputs.py), and the outputs of a good call afterwards are the oracle's."""
    n, S, T, freq = 5, 2, 30, 3
    q, l0, v0 = sc.stack_charged(charged_initial_states(902, n, S, T, freq, box=BOX))
    qd, ld, vd = _dev(q, l0, v0)
    sim = _charged(n)
    with pytest.raises(TypeError, match="loc0"):
        sim.integrate(qd, ld.float(), vd, T, freq)
    with pytest.raises(ValueError, match="vel0"):
        sim.integrate(qd, ld, vd.transpose(1, 2), T, freq)
    with pytest.raises(ValueError, match="loc0"):
        sim.integrate(qd, ld.cpu(), vd, T, freq)
    _check_charged("charged after refusals", _np(sim.integrate(qd, ld, vd, T, freq)),
                   sc.charged_oracle(q, l0, v0, T, freq))


def test_side_stream_gives_the_default_stream_bits():
    n, S, T, freq = 20, 7, 30, 3
    q, l0, v0 = sc.stack_charged(charged_initial_states(903, n, S, T, freq, box=BOX))
    p0, w0, m = gravity_initial_state(904, n, S, T, freq)
    cd, gd = _dev(q, l0, v0), _dev(p0, w0, m[:, :, 0])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    for kernel in ("resident", "tiled"):
        runs = (lambda: _charged(n).integrate(*cd, T, freq, kernel=kernel),
                lambda: pkg.sim.GravitySim(n_balls=n).integrate(*gd, T, freq, kernel=kernel))
        for run in runs:
            want = _np(run())
            with torch.cuda.stream(side):
                got = run()
            side.synchronize()
            for g, w in zip(_np(got), want):
                assert np.array_equal(g, w)
