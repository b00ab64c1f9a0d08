"""Cases the simulator tests share (tests/test_gpu_sim_batches.py on the GPU, tests/test_sim_inputs.py on the CPU):
initial states, the oracle called with a case's own parameters, and the two CPU-side preconditions that keep a case
from passing blind. No GPU here.

sensitivity(case)   the oracle at the case's moved parameter against the oracle at the default, max-norm relative
                    over velocities: must exceed 1000 SIMTOL, or the GPU check could not tell right from wrong
reorder_noise(case) the oracle under a permutation of the particles against itself: must stay below SIMTOL / 1000,
                    or a correct kernel with another summation order could miss SIMTOL
"""
import functools

import numpy as np

from oracle import sim as osim
from tests.conftest import maxnorm_rel
from tests.test_oracle_sim import charged_initial_states, gravity_initial_state

SIMTOL = 1e-7
BOX = 50.            # holds every charged draw used here (the reference asserts |loc| < 3 box)
PSEED = 4100


def horizon(n):
    """(T, sample_freq, batch) of a parameter case: 63 steps and two trajectories at the resident sizes, 21 steps
    and one trajectory at n = 600, where an oracle force evaluation costs 13 ms on the host."""
    return (63, 21, 2) if n <= 64 else (21, 7, 1)


# name -> (constructor keywords, charge_prob); None = the default (1/2, 0, 1/2)
CHARGED_PARAMS = {
    "strength": (dict(interaction_strength=1.7), None),
    "neutral": ({}, (0.4, 0.2, 0.4)),
    "vel_norm": (dict(vel_norm=0.8), None),
    "loc_std": (dict(loc_std=1.5), None),
    "all": (dict(interaction_strength=1.7, vel_norm=0.8, loc_std=1.5), (0.4, 0.2, 0.4)),
}
# name -> GravitySim constructor keywords
GRAVITY_PARAMS = {
    "G": dict(interaction_strength=2.5),
    "softening": dict(softening=0.03),
    "dt": dict(dt=0.004),
    "all": dict(interaction_strength=2.5, softening=0.03, dt=0.004, loc_std=2),
}


def stack_charged(states):
    """[(q [n, 1], loc [3, n], vel [3, n]), ...] -> q [S, n], loc0 [S, 3, n], vel0 [S, 3, n]."""
    return (np.stack([s[0][:, 0] for s in states]), np.stack([s[1] for s in states]),
            np.stack([s[2] for s in states]))


def charged_oracle(q, l0, v0, T, freq, **kw):
    """oracle/sim.py over a stacked batch: loc, vel [S, T / freq - 1, 3, n]."""
    out = [osim.charged_trajectory(l0[s], v0[s], q[s][:, None], T, freq, **kw) for s in range(len(q))]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def _perm(n, seed=5):
    return np.random.RandomState(seed).permutation(n)


def charged_reorder_noise(a, q, l0, v0, T, freq, **kw):
    """a: the oracle's result on the unpermuted state."""
    p = _perm(q.shape[1])
    b = charged_oracle(q[:, p], l0[:, :, p], v0[:, :, p], T, freq, **kw)
    return max(maxnorm_rel(b[k], a[k][..., p]) for k in range(2))


def gravity_reorder_noise(a, p0, v0, m, T, freq, **kw):
    p = _perm(p0.shape[1])
    b = osim.gravity_trajectory(p0[:, p], v0[:, p], m[:, p], T, freq, **kw)
    return max(maxnorm_rel(b[k], a[k][:, :, p]) for k in range(3))


# ---- B: parameters off their defaults ----
@functools.lru_cache(maxsize=None)
def charged_param_case(name, n):
    """(states, oracle keywords, want (loc, vel), sensitivity, reorder noise) of a charged parameter case; the GPU
    side draws the same states from np.random.seed(PSEED + n). Cached: callers leave the arrays unchanged."""
    simkw, cp = CHARGED_PARAMS[name]
    PT, PFREQ, S = horizon(n)
    drawkw = {k: simkw[k] for k in ("vel_norm", "loc_std") if k in simkw}
    okw = dict(strength=simkw.get("interaction_strength", 1.0))
    moved = dict(drawkw, **({"charge_prob": cp} if cp else {}))
    q, l0, v0 = stack_charged(charged_initial_states(PSEED + n, n, S, PT, PFREQ, box=BOX, **moved))
    want = charged_oracle(q, l0, v0, PT, PFREQ, **okw)
    if name == "neutral":      # the same state with every neutral particle charged
        assert (q == 0).any()
        base = charged_oracle(np.where(q == 0, 1.0, q), l0, v0, PT, PFREQ)
    else:                      # the default parameters from the same seed
        base = charged_oracle(*stack_charged(charged_initial_states(PSEED + n, n, S, PT, PFREQ, box=BOX)), PT, PFREQ)
    noise = charged_reorder_noise(want, q, l0, v0, PT, PFREQ, **okw)
    return (q, l0, v0), okw, want, maxnorm_rel(want[1], base[1]), noise


def _gravity_okw(simkw):
    return dict(dt=simkw.get("dt", 0.001), G=simkw.get("interaction_strength", 1.0),
                softening=simkw.get("softening", 0.1))


@functools.lru_cache(maxsize=None)
def gravity_param_case(name, n):
    simkw = GRAVITY_PARAMS[name]
    PT, PFREQ, B = horizon(n)
    okw = _gravity_okw(simkw)
    p0, v0, m = gravity_initial_state(PSEED + n, n, B, PT, PFREQ, loc_std=simkw.get("loc_std", 1.0))
    want = osim.gravity_trajectory(p0, v0, m, PT, PFREQ, **okw)
    base = osim.gravity_trajectory(*gravity_initial_state(PSEED + n, n, B, PT, PFREQ), PT, PFREQ)
    noise = gravity_reorder_noise(want, p0, v0, m, PT, PFREQ, **okw)
    return (p0, v0, m), okw, want, maxnorm_rel(want[1], base[1]), noise


@functools.lru_cache(maxsize=None)
def gravity_coincident_case(n):
    """softening = 0 with coincident bodies: (4, 5) in every trajectory and, where there is a second sender chunk,
    the pair that straddles it (n - 1 on n // 2 otherwise). The r2 > 0 guard of the pair helper fires on these and
    on every self pair; nothing else keeps the sums finite."""
    PT, PFREQ, B = horizon(n)
    p0, v0, m = gravity_initial_state(PSEED + 7 + n, n, B, PT, PFREQ)
    j = 512 if n > 512 else n - 1
    i = 511 if n > 512 else n // 2
    p0[:, 5] = p0[:, 4]
    p0[:, j] = p0[:, i]
    okw = dict(softening=0.0)
    with np.errstate(divide="ignore"):
        want = osim.gravity_trajectory(p0, v0, m, PT, PFREQ, **okw)
        base = osim.gravity_trajectory(p0, v0, m, PT, PFREQ)
        noise = gravity_reorder_noise(want, p0, v0, m, PT, PFREQ, **okw)
    return (p0, v0, m), okw, want, maxnorm_rel(want[1], base[1]), noise


# ---- C: a clamped step ----
CT, CFREQ, CN = 63, 7, 600


@functools.lru_cache(maxsize=None)
def clamp_case():
    """One trajectory of CN bodies (three receiver tiles, two sender chunks) holding two like-charged pairs at rest:
    bodies (3, 300), 0.05 apart along the diagonal, so all three components clamp, positive on one body and
    negative on the other, across two receiver tiles; bodies (511, 512), 0.06 apart along x only, across the
    sender chunk, where a per-component clamp differs from a clamp of the norm.
    Returns (q, l0, v0), want, unclamped sensitivity, steps with an active clamp."""
    q, l0, v0 = stack_charged(charged_initial_states(977, CN, 1, CT, CFREQ, box=BOX))
    a = np.array([0.3, -0.2, 0.1])
    b = np.array([-0.4, 0.25, -0.15])
    l0[0, :, 3], l0[0, :, 300] = a, a + 0.05 / np.sqrt(3.0)
    l0[0, :, 511], l0[0, :, 512] = b, b + np.array([0.06, 0.0, 0.0])
    q[0, [3, 300]] = 1.0
    q[0, [511, 512]] = -1.0
    v0[0][:, [3, 300, 511, 512]] = 0.0
    want = charged_oracle(q, l0, v0, CT, CFREQ)
    free = charged_oracle(q, l0, v0, CT, CFREQ, max_F=1e300)
    # steps at which some component is clamped: replay the positions with the oracle's own update
    loc, vel, active = l0[0].copy(), v0[0].copy(), 0
    for i in range(CT):
        if i:
            loc = loc + 0.001 * vel
        raw = osim.charged_forces(loc, q[0][:, None], 1.0, 1e300)
        active += bool((np.abs(raw) > 100.0).any())
        vel = vel + 0.001 * np.clip(raw, -100.0, 100.0)
    return (q, l0, v0), want, maxnorm_rel(want[1], free[1]), active
