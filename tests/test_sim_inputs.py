"""What ChargedParticlesSim.integrate and GravitySim.integrate refuse on the host (sim.py), CPU only: dtype, shape
and device checks come before any device work and name the argument, and a correct CPU tensor still reaches the
"no CPU path" refusal. Also the CPU-side preconditions of tests/test_gpu_sim_batches.py's cases
(tests/sim_cases.py), so that they are asserted on machines without a GPU as well."""
import inspect

import numpy as np
import pytest
import torch

from no_node_comparison_amd import _lib, sim
from tests import sim_cases as sc
from tests.sim_cases import SIMTOL

S, N = 2, 5


def _charged_args(**kw):
    a = dict(q=torch.zeros(S, N, dtype=torch.float64), loc0=torch.zeros(S, 3, N, dtype=torch.float64),
             vel0=torch.zeros(S, 3, N, dtype=torch.float64))
    a.update(kw)
    return a["q"], a["loc0"], a["vel0"]


def _gravity_args(**kw):
    a = dict(pos0=torch.zeros(S, N, 3, dtype=torch.float64), vel0=torch.zeros(S, N, 3, dtype=torch.float64),
             mass=torch.ones(S, N, dtype=torch.float64))
    a.update(kw)
    return a["pos0"], a["vel0"], a["mass"]


CASES = [(lambda **kw: sim.ChargedParticlesSim(n_balls=N).integrate(*_charged_args(**kw), 30, 3),
          ("q", "loc0", "vel0"), {"q": (S, N), "loc0": (S, 3, N), "vel0": (S, 3, N)}),
         (lambda **kw: sim.GravitySim(n_balls=N).integrate(*_gravity_args(**kw), 30, 3),
          ("mass", "pos0", "vel0"), {"mass": (S, N), "pos0": (S, N, 3), "vel0": (S, N, 3)})]


@pytest.mark.parametrize("call,names,shapes", CASES, ids=["charged", "gravity"])
def test_integrate_refuses_wrong_dtypes(call, names, shapes):
    """A float32 tensor would make the float64 kernel read past the end of the buffer."""
    for name in names:
        for dtype in (torch.float32, torch.float16, torch.int64):
            with pytest.raises(TypeError, match=rf"\b{name} must be float64"):
                call(**{name: torch.zeros(shapes[name], dtype=dtype)})
        with pytest.raises(TypeError, match=rf"\b{name} must be a torch.Tensor"):
            call(**{name: np.zeros(shapes[name])})


@pytest.mark.parametrize("call,names,shapes", CASES, ids=["charged", "gravity"])
def test_integrate_refuses_wrong_shapes(call, names, shapes):
    main = names[0]
    for name in names[1:]:
        good = shapes[name]
        bad = [good[::-1], (good[0], good[2], good[1]), good[1:], good + (1,),
               (good[0] + 1,) + good[1:], (good[0], good[1] + 1, good[2]), (good[0], good[1], good[2] + 1)]
        for shape in bad:
            with pytest.raises(ValueError, match=rf"\b{name} must have shape"):
                call(**{name: torch.zeros(shape, dtype=torch.float64)})
    for shape in ((S, N, 1), (S * N,), (0, N), (S, 0)):
        with pytest.raises(ValueError, match=rf"\b{main} must have shape"):
            call(**{main: torch.zeros(shape, dtype=torch.float64)})


@pytest.mark.parametrize("call,names,shapes", CASES, ids=["charged", "gravity"])
def test_integrate_refuses_mixed_devices(call, names, shapes):
    """The meta device stands for "another device" where there is no GPU."""
    for name in names[1:]:
        with pytest.raises(ValueError, match=rf"\b{name} is on meta"):
            call(**{name: torch.zeros(shapes[name], dtype=torch.float64, device="meta")})
    with pytest.raises(ValueError, match="one device"):
        call(**{names[0]: torch.zeros(shapes[names[0]], dtype=torch.float64, device="meta")})


def test_integrate_refuses_bad_schedules():
    for T, freq in ((30, 4), (0, 1), (30, 0), (-30, 3), (30, -3)):
        with pytest.raises(ValueError, match="sample_freq"):
            sim.ChargedParticlesSim(n_balls=N).integrate(*_charged_args(), T, freq)
        with pytest.raises(ValueError, match="sample_freq"):
            sim.GravitySim(n_balls=N).integrate(*_gravity_args(), T, freq)


def test_a_correct_cpu_tensor_reaches_the_device_refusal():
    """Every host check passes, contiguous or not, T == sample_freq included; then "no CPU path"."""
    q, l0, v0 = _charged_args()
    p0, w0, m = _gravity_args()
    for T, freq in ((30, 3), (7, 7)):
        for kernel in (None, "resident", "tiled"):
            with pytest.raises(_lib.NonodeError, match="no CPU path"):
                sim.ChargedParticlesSim(n_balls=N).integrate(q, l0, v0, T, freq, kernel=kernel)
            with pytest.raises(_lib.NonodeError, match="no CPU path"):
                sim.GravitySim(n_balls=N).integrate(p0, w0, m, T, freq, kernel=kernel)
    with pytest.raises(_lib.NonodeError, match="no CPU path"):
        sim.ChargedParticlesSim(n_balls=N).integrate(q, torch.zeros(S, N, 3, dtype=torch.float64).transpose(1, 2), v0,
                                                     30, 3)
    with pytest.raises(_lib.NonodeError, match="no CPU path"):
        sim.GravitySim(n_balls=N).integrate(torch.zeros(S, 3, N, dtype=torch.float64).transpose(1, 2), w0, m, 30, 3)


def test_the_host_checks_come_first():
    """A wrong dtype or shape on a CPU tensor is named as such, not as a missing GPU; the kernel keyword is
    checked before the device as well."""
    with pytest.raises(TypeError, match="vel0 must be float64"):
        sim.ChargedParticlesSim(n_balls=N).integrate(*_charged_args(vel0=torch.zeros(S, 3, N)), 30, 3)
    with pytest.raises(ValueError, match="kernel must be"):
        sim.GravitySim(n_balls=N).integrate(*_gravity_args(), 30, 3, kernel="nope")
    big = torch.zeros(1, 1025, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match="n_balls <= 1024"):
        sim.GravitySim(n_balls=1025).integrate(big, big, torch.ones(1, 1025, dtype=torch.float64), 30, 3,
                                               kernel="resident")


def test_gravity_integrate_mirrors_the_charged_signature():
    g = inspect.signature(sim.GravitySim.integrate).parameters
    assert list(g) == ["self", "pos0", "vel0", "mass", "T", "sample_freq", "kernel"] and g["kernel"].default is None
    c = inspect.signature(sim.ChargedParticlesSim.integrate).parameters
    assert list(c) == ["self", "q", "loc0", "vel0", "T", "sample_freq", "kernel"]
    assert "self.integrate(" in inspect.getsource(sim.GravitySim.sample_trajectory_batch)


# ---- the CPU-side preconditions of tests/test_gpu_sim_batches.py ----
@pytest.mark.parametrize("n", [40, 600])
@pytest.mark.parametrize("name", list(sc.CHARGED_PARAMS))
def test_charged_parameter_cases_are_not_blind(name, n):
    _, _, want, sens, noise = sc.charged_param_case(name, n)
    assert sens > 1000 * SIMTOL and noise < SIMTOL / 1000, (sens, noise)
    assert want[0].shape == (sc.horizon(n)[2], 2, 3, n) and np.isfinite(want[0]).all()


@pytest.mark.parametrize("n", [37, 600])
@pytest.mark.parametrize("name", list(sc.GRAVITY_PARAMS) + ["coincident"])
def test_gravity_parameter_cases_are_not_blind(name, n):
    case = sc.gravity_coincident_case(n) if name == "coincident" else sc.gravity_param_case(name, n)
    (p0, _, _), _, want, sens, noise = case
    assert sens > 1000 * SIMTOL and noise < SIMTOL / 1000, (sens, noise)
    assert all(np.isfinite(w).all() for w in want)
    if name == "coincident":
        assert np.array_equal(p0[:, 5], p0[:, 4]) and (n < 600 or np.array_equal(p0[:, 512], p0[:, 511]))


def test_the_clamp_case_clamps():
    """19 of 63 steps have a clamped component, and without the clamp the velocities move by 0.37 relative."""
    (q, l0, v0), want, sens, active = sc.clamp_case()
    assert sens > 1000 * SIMTOL and active >= 10, (sens, active)
    first = want[1][0, 0]
    cap = sc.CFREQ * 0.1 * (1 + 1e-12)
    assert np.all(first[:, 3] < -0.5) and np.all(first[:, 300] > 0.5) and np.all(np.abs(first[:, [3, 300]]) <= cap)
    assert first[0, 511] < -0.5 and first[0, 512] > 0.5 and np.all(np.abs(first[0, [511, 512]]) <= cap)
