"""Synthetic N-body data on the GPU: drop-in ChargedParticlesSim / GravitySim
(synthetic_sim.py:149-296, 299-481) and generate_dataset (generate_dataset.py:62-104).

Initial conditions are drawn on the host with numpy in exactly the reference's call order
(np.random.choice / randn per simulation, then the observation-noise draws), so a given
np.random.seed reproduces the reference's datasets; the time integration runs in one kernel launch
for every trajectory of a batch up to 1024 bodies, and in one launch per step of tiled
multi-workgroup kernels above that (csrc/nonode_sim.hip, float64; ``kernel=`` chooses). Outputs are
numpy arrays in the reference's shapes; ``as_numpy=False`` keeps the trajectories on the GPU.
"""
import os

import numpy as np
import torch

from . import _lib


def _dev_f64(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(device)


RESIDENT_NMAX = 1024   # nonode_sim_gravity / nonode_sim_charged: one workgroup holds a trajectory


def _pick_kernel(kernel, n):
    """The simulator kernel for n bodies: "resident" (one workgroup per trajectory, n <= 1024) or "tiled"
    (receiver tiles, one launch per step, any n). None keeps the resident kernel wherever it serves."""
    if kernel is None:
        return "resident" if n <= RESIDENT_NMAX else "tiled"
    if kernel not in ("resident", "tiled"):
        raise ValueError(f"kernel must be None, 'resident' or 'tiled', not {kernel!r}")
    if kernel == "resident" and n > RESIDENT_NMAX:
        raise ValueError(f"kernel='resident' holds a trajectory in one workgroup: n_balls <= {RESIDENT_NMAX}, "
                         f"not {n} (use kernel='tiled' or None)")
    return kernel


def _tiled_workspace(S, n, dev):
    nbytes = _lib.lib().nonode_sim_tiled_workspace_bytes(S, n)
    if nbytes == 0:
        raise ValueError(f"the tiled simulators take n_balls <= 2**20 and S * n_balls < 2**31, not S={S}, "
                         f"n_balls={n}")
    return torch.empty(nbytes // 8, dtype=torch.float64, device=dev), nbytes


def _check_state(who, T, sample_freq, main, others):
    """The host checks of an integrate(): every argument a float64 tensor of its stated shape, all on one
    device, sample_freq dividing T. main = (name, tensor, shape words) fixes S and N; others = [(name, tensor,
    shape given S and N, shape words)]. Raises TypeError / ValueError naming the argument; returns the tensors
    made contiguous. No device work: a CPU tensor passes (require_device refuses it afterwards)."""
    name, t, words = main
    for nm, a in [(name, t)] + [(o[0], o[1]) for o in others]:
        if not isinstance(a, torch.Tensor):
            raise TypeError(f"{who}: {nm} must be a torch.Tensor, not {type(a).__name__}")
        if a.dtype != torch.float64:
            raise TypeError(f"{who}: {nm} must be float64, not {a.dtype}")
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"{who}: {name} must have shape {words}, not {tuple(t.shape)}")
    S, n = t.shape
    for nm, a, shape, w in others:
        if tuple(a.shape) != shape(S, n):
            raise ValueError(f"{who}: {nm} must have shape {w} = {shape(S, n)} (from {name} {tuple(t.shape)}), "
                             f"not {tuple(a.shape)}")
        if a.device != t.device:
            raise ValueError(f"{who}: {nm} is on {a.device}, {name} on {t.device}: one device for all")
    if int(T) != T or int(sample_freq) != sample_freq or T <= 0 or sample_freq <= 0 or T % sample_freq:
        raise ValueError(f"{who}: T={T} sample_freq={sample_freq} (positive integers, sample_freq divides T)")
    return [t.contiguous()] + [o[1].contiguous() for o in others]


def _default_device():
    if not torch.cuda.is_available():
        raise _lib.NonodeError("no CPU path: the simulators run on a ROCm GPU (the CPU restatement is "
                               "oracle/sim.py, test infrastructure)")
    return torch.device("cuda")


class ChargedParticlesSim:
    """synthetic_sim.py:149-296 (charged particles, leapfrog with clamped Coulomb forces).

    Any n_balls up to 2**20 (S * n_balls < 2**31): up to 1024 one workgroup integrates a trajectory in one
    launch, above that the tiled kernel runs one launch per step (``kernel=``). The initial positions are
    drawn with loc_std * (n_balls / 5) ** (1/3) and must lie within 3 * box_size, as in the reference: the
    default box_size = 5 does not hold a large system (at n_balls = 1100 the largest draw is about 25), so
    pass a box_size that does."""

    def __init__(self, n_balls=5, box_size=5., loc_std=1., vel_norm=0.5, interaction_strength=1., noise_var=0.):
        self.n_balls = n_balls
        self.box_size = box_size
        self.loc_std = loc_std * (float(n_balls) / 5.) ** (1 / 3)
        self.vel_norm = vel_norm
        self.interaction_strength = interaction_strength
        self.noise_var = noise_var
        self._charge_types = np.array([-1., 0., 1.])
        self._delta_T = 0.001
        self._max_F = 0.1 / self._delta_T
        self.dim = 3

    def _clamp(self, loc, vel):
        """Elastic walls at +-box_size (synthetic_sim.py:194-218), applied to the initial state."""
        assert np.all(loc < self.box_size * 3) and np.all(loc > -self.box_size * 3)
        over = loc > self.box_size
        loc[over] = 2 * self.box_size - loc[over]
        vel[over] = -np.abs(vel[over])
        under = loc < -self.box_size
        loc[under] = -2 * self.box_size - loc[under]
        vel[under] = np.abs(vel[under])
        return loc, vel

    def _draw(self, T_save, charge_prob):
        n = self.n_balls
        charges = np.random.choice(self._charge_types, size=(n, 1), p=charge_prob)
        loc = np.random.randn(self.dim, n) * self.loc_std
        vel = np.random.randn(self.dim, n)
        vel = vel * self.vel_norm / np.sqrt((vel ** 2).sum(axis=0)).reshape(1, -1)
        loc, vel = self._clamp(loc, vel)
        return charges, loc, vel

    def sample_trajectories(self, S, T=10000, sample_freq=10, charge_prob=(1. / 2, 0, 1. / 2), device=None,
                            as_numpy=True, kernel=None, with_edges=True):
        """S consecutive sample_trajectory calls (the reference's RNG order) integrated together (one launch
        with the resident kernel, one per step with the tiled one; ``kernel`` as in integrate).
        Returns loc, vel [S, T_save, 3, N], edges [S, N, N], charges [S, N, 1]. edges = q q^T is float64 on
        the host, 8 N^2 bytes per trajectory (3.2 GB at N = 20,000): with_edges=False returns None in its
        place and never forms it."""
        assert T % sample_freq == 0
        _pick_kernel(kernel, self.n_balls)
        n, T_save = self.n_balls, T // sample_freq - 1
        q, l0, v0, noise = [], [], [], []
        for _ in range(S):
            c, l, v = self._draw(T_save, list(charge_prob))
            q.append(c); l0.append(l); v0.append(v)
            noise.append((np.random.randn(T_save, self.dim, n), np.random.randn(T_save, self.dim, n)))
        q, l0, v0 = np.stack(q), np.stack(l0), np.stack(v0)
        dev = torch.device(device) if device is not None else _default_device()
        _lib.require_device(torch.empty(0, device=dev))
        ql, ld, vd = _dev_f64(q.reshape(S, n), dev), _dev_f64(l0, dev), _dev_f64(v0, dev)
        loc_d, vel_d = self.integrate(ql, ld, vd, T, sample_freq, kernel=kernel)
        if self.noise_var:
            loc_d += _dev_f64(np.stack([a for a, _ in noise]), dev) * self.noise_var
            vel_d += _dev_f64(np.stack([b for _, b in noise]), dev) * self.noise_var
        edges = q @ np.transpose(q, (0, 2, 1)) if with_edges else None
        if not as_numpy:
            return loc_d, vel_d, edges, q
        return loc_d.cpu().numpy(), vel_d.cpu().numpy(), edges, q

    def integrate(self, q, loc0, vel0, T, sample_freq, kernel=None):
        """The time integration of synthetic_sim.py:241-296 for S trajectories already on the GPU:
        q [S, N], loc0 / vel0 [S, 3, N] float64 (after _clamp) -> loc, vel [S, T_save, 3, N].
        kernel: None (the resident kernel, one launch, when N <= 1024, else the tiled one, one launch per
        step), "tiled" (at any N; the same bits as the resident kernel where both run) or "resident"
        (ValueError when N > 1024)."""
        q, loc0, vel0 = _check_state("ChargedParticlesSim.integrate", T, sample_freq, ("q", q, "[S, N]"),
                                     [("loc0", loc0, lambda S, n: (S, 3, n), "[S, 3, N]"),
                                      ("vel0", vel0, lambda S, n: (S, 3, n), "[S, 3, N]")])
        S, n = q.shape
        kernel = _pick_kernel(kernel, n)
        _lib.require_device(q, loc0, vel0)
        T_save = T // sample_freq - 1
        loc_d = torch.empty(S, T_save, 3, n, dtype=torch.float64, device=q.device)
        vel_d = torch.empty_like(loc_d)
        if T_save == 0:   # T == sample_freq: the reference returns empty arrays; nothing to launch
            return loc_d, vel_d
        args = (S, n, T, sample_freq, self._delta_T, self._max_F, float(self.interaction_strength), _lib.ptr(loc0),
                _lib.ptr(vel0), _lib.ptr(q), _lib.ptr(loc_d), _lib.ptr(vel_d))
        if kernel == "resident":
            _lib.check(_lib.lib().nonode_sim_charged(*args, _lib.stream_of(q)))
        else:
            ws, nbytes = _tiled_workspace(S, n, q.device)
            _lib.check(_lib.lib().nonode_sim_charged_tiled(*args, _lib.ptr(ws), nbytes, _lib.stream_of(q)))
        return loc_d, vel_d

    def sample_trajectory(self, T=10000, sample_freq=10, charge_prob=(1. / 2, 0, 1. / 2), kernel=None):
        """synthetic_sim.py:220-296: loc, vel [T_save, 3, N], edges [N, N], charges [N, 1]."""
        loc, vel, edges, q = self.sample_trajectories(1, T, sample_freq, charge_prob, kernel=kernel)
        return loc[0], vel[0], edges[0], q[0]


class GravitySim:
    """synthetic_sim.py:299-481 (softened gravity, kick-drift-kick). Any n_balls up to 2**20
    (batch_size * n_balls < 2**31); above 1024 the tiled kernel runs one launch per step (``kernel=``)."""

    def __init__(self, n_balls=100, loc_std=1, vel_norm=0.5, interaction_strength=1, noise_var=0, dt=0.001,
                 softening=0.1):
        self.n_balls = n_balls
        self.loc_std = loc_std
        self.vel_norm = vel_norm
        self.interaction_strength = interaction_strength
        self.noise_var = noise_var
        self.dt = dt
        self.softening = softening
        self.dim = 3

    def sample_trajectory_batch(self, T=10000, sample_freq=10, batch_size=1, device=None, as_numpy=True,
                                kernel=None):
        """synthetic_sim.py:407-456: pos, vel, force [B, T_save, N, 3], mass [B, N, 1] (device tensors with
        as_numpy=False; mass stays the host array it was drawn as).
        kernel: None (the resident kernel, one launch, when N <= 1024, else the tiled one, one launch per
        step), "tiled" (at any N; the same bits as the resident kernel where both run) or "resident"
        (ValueError when N > 1024)."""
        assert T % sample_freq == 0
        T_save, N = T // sample_freq, self.n_balls
        kernel = _pick_kernel(kernel, N)
        mass = np.ones((batch_size, N, 1))
        mass += np.random.randn(batch_size, N, 1) * self.loc_std * 0.1
        pos = np.random.randn(batch_size, N, self.dim)
        vel = np.random.randn(batch_size, N, self.dim)
        for b in range(batch_size):
            vel[b] -= np.mean(mass[b] * vel[b], 0) / np.mean(mass[b])
        noise = [np.random.randn(batch_size, T_save, N, self.dim) for _ in range(3)]
        dev = torch.device(device) if device is not None else _default_device()
        _lib.require_device(torch.empty(0, device=dev))
        pd, vd, md = _dev_f64(pos, dev), _dev_f64(vel, dev), _dev_f64(mass.reshape(batch_size, N), dev)
        out = self.integrate(pd, vd, md, T, sample_freq, kernel=kernel)
        if self.noise_var:
            for t, z in zip(out, noise):
                t += _dev_f64(z, dev) * self.noise_var
        if not as_numpy:
            return out[0], out[1], out[2], mass
        return out[0].cpu().numpy(), out[1].cpu().numpy(), out[2].cpu().numpy(), mass

    def integrate(self, pos0, vel0, mass, T, sample_freq, kernel=None):
        """The time integration of synthetic_sim.py:435-450 for B trajectories already on the GPU:
        pos0 / vel0 [B, N, 3], mass [B, N] float64 -> pos, vel, force [B, T_save, N, 3], T_save = T / sample_freq.
        kernel as in sample_trajectory_batch."""
        mass, pos0, vel0 = _check_state("GravitySim.integrate", T, sample_freq, ("mass", mass, "[B, N]"),
                                        [("pos0", pos0, lambda B, n: (B, n, 3), "[B, N, 3]"),
                                         ("vel0", vel0, lambda B, n: (B, n, 3), "[B, N, 3]")])
        B, N = mass.shape
        kernel = _pick_kernel(kernel, N)
        _lib.require_device(pos0, vel0, mass)
        T_save = T // sample_freq
        out = [torch.empty(B, T_save, N, 3, dtype=torch.float64, device=mass.device) for _ in range(3)]
        args = (B, N, T, sample_freq, float(self.dt), float(self.interaction_strength), float(self.softening),
                _lib.ptr(pos0), _lib.ptr(vel0), _lib.ptr(mass), *[_lib.ptr(t) for t in out])
        if kernel == "resident":
            _lib.check(_lib.lib().nonode_sim_gravity(*args, _lib.stream_of(mass)))
        else:
            ws, nbytes = _tiled_workspace(B, N, mass.device)
            _lib.check(_lib.lib().nonode_sim_gravity_tiled(*args, _lib.ptr(ws), nbytes, _lib.stream_of(mass)))
        return out[0], out[1], out[2]

    def sample_trajectory(self, T=10000, sample_freq=10, kernel=None):
        """synthetic_sim.py:360-404 (the single-trajectory form; its RNG draws differ from the batch
        form only in shape): pos, vel, force [T_save, N, 3], mass [N, 1]."""
        pos, vel, force, mass = self.sample_trajectory_batch(T, sample_freq, 1, kernel=kernel)
        return pos[0], vel[0], force[0], mass[0]


def generate_dataset(sim, num_sims, length, sample_freq, kernel=None):
    """generate_dataset.py:62-104: gravity in batches of 50 (sample_trajectory_batch), charged one
    simulation at a time in the reference; here every charged simulation of the split is integrated
    together (same RNG order). Returns loc, vel, edges, charges as the reference stacks them.
    kernel: passed to the simulator (None, "resident" or "tiled")."""
    if isinstance(sim, GravitySim):
        parts = [sim.sample_trajectory_batch(T=length, sample_freq=sample_freq, batch_size=50, kernel=kernel)
                 for _ in range(num_sims // 50 + (num_sims % 50 > 0))]
        return tuple(np.concatenate([p[k] for p in parts], axis=0) for k in range(4))
    return sim.sample_trajectories(num_sims, T=length, sample_freq=sample_freq, kernel=kernel)


def dataset_suffix(simulation, n_balls, initial_vel=1, suffix=""):
    """File-name suffix of generate_dataset.py:46-59 ('_charged20_initvel1small', ...)."""
    return f"_{simulation}{n_balls}_initvel{initial_vel}{suffix}"


def save_dataset(outdir, split, name_suffix, loc, vel, edges, charges):
    """The four .npy files per split that generate_dataset.py:130-147 writes."""
    os.makedirs(outdir, exist_ok=True)
    for key, arr in (("loc", loc), ("vel", vel), ("edges", edges), ("charges", charges)):
        np.save(os.path.join(outdir, f"{key}_{split}{name_suffix}.npy"), arr)
