// N-body simulators on the GPU: the reference's synthetic data generators.
//
//   sim_charged_kernel  ChargedParticlesSim.sample_trajectory (synthetic_sim.py:220-296): Coulomb
//                       forces q_i q_j (x_i - x_j) / |x_i - x_j|^3, per-component clamp +-max_F,
//                       the reference's leapfrog (initial half kick, then drift / sample / kick)
//   sim_gravity_kernel  GravitySim.sample_trajectory_batch (synthetic_sim.py:407-481): softened
//                       gravity a_i = G sum_j m_j (x_j - x_i) (|x_j - x_i|^2 + s^2)^-3/2,
//                       kick-drift-kick, samples (x, v, a m) every sample_freq steps
//
// float64 like the reference's numpy. One thread per particle; a workgroup holds floor(64 / N)
// whole trajectories when N <= 32 (three at N = 20, so 60 of 64 lanes work), else one trajectory
// of ceil(N / 64) waves. The positions of the current step live in LDS. The per-pair arithmetic
// mirrors the reference's expression order (squared distance of ChargedParticlesSim._l2 as
// |a|^2 + |b|^2 - 2 a.b); x^(3/2) is x sqrt(x) (within an ulp of numpy's pow). dmul / dadd / dsub are
// HIP's _rn forms, plain operators to the compiler, which contracts a product that feeds a sum into an
// FMA: the same way wherever the same helper is inlined. The integrator's updates are FMAs by name.
// Short horizons agree to rounding; the reference's numpy reductions sum in a different order,
// and both trajectories are chaotic over long ones.
//
// The resident kernels stop at SIM_NMAX = 1024 bodies (a workgroup). sim_gravity_tiled_kernel and
// sim_charged_tiled_kernel serve any N up to 2^20 with one launch per time step and the same per-pair
// helpers and sender order, so their trajectories equal the resident ones bit for bit.
//
// Included at the end of nonode.hip (same translation unit).

namespace {

constexpr int SIM_NMAX = 1024;

__device__ __forceinline__ double dmul(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ double dadd(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ double dsub(double a, double b) { return __dsub_rn(a, b); }
// a b + c in one rounding: the kicks and drifts (what contraction made of them in the resident kernels, written
// out so that no kernel's surrounding code can decide otherwise)
__device__ __forceinline__ double dfma(double a, double b, double c) { return fma(a, b, c); }

// ---- the per-pair arithmetic, one copy for the resident and the tiled kernels ----
// |x|^2 as ChargedParticlesSim._l2 forms its row norms
__device__ __forceinline__ double sim_norm2(const double x[3]) {
  return dadd(dadd(dmul(x[0], x[0]), dmul(x[1], x[1])), dmul(x[2], x[2]));
}
// F += strength q_i q_j (x - x_j) / |x - x_j|^3 with |x - x_j|^2 = |x|^2 + |x_j|^2 - 2 x.x_j; the self pair adds
// an exact 0 (fill_diagonal(forces_size, 0)) without a branch, so the divide / sqrt chains of consecutive
// senders can overlap
__device__ __forceinline__ void sim_charged_pair(double F[3], bool self, const double x[3], double ni, double qi,
                                                 double xj0, double xj1, double xj2, double nj, double qj,
                                                 double strength) {
  const double dot = dadd(dadd(dmul(x[0], xj0), dmul(x[1], xj1)), dmul(x[2], xj2));
  const double l2 = self ? 1.0 : dsub(dadd(ni, nj), dmul(2.0, dot));
  const double fs = self ? 0.0 : dmul(strength, qi * qj) / dmul(l2, sqrt(l2));
  F[0] = dadd(F[0], dmul(fs, dsub(x[0], xj0)));
  F[1] = dadd(F[1], dmul(fs, dsub(x[1], xj1)));
  F[2] = dadd(F[2], dmul(fs, dsub(x[2], xj2)));
}
// v += dt clamp(F, +-max_F) per component (synthetic_sim.py:256-262, 283-290)
__device__ __forceinline__ void sim_charged_kick(double v[3], const double F[3], double max_F, double dt) {
  for (int d = 0; d < 3; ++d) {
    const double f = F[d] > max_F ? max_F : (F[d] < -max_F ? -max_F : F[d]);
    v[d] = dfma(dt, f, v[d]);
  }
}
// A += m_j (x_j - x) (|x_j - x|^2 + s^2)^-3/2 (compute_acceleration_batch, synthetic_sim.py:458-481)
__device__ __forceinline__ void sim_gravity_pair(double A[3], const double x[3], double xj0, double xj1, double xj2,
                                                 double mj, double soft2) {
  const double dx = dsub(xj0, x[0]), dy = dsub(xj1, x[1]), dz = dsub(xj2, x[2]);
  const double r2 = dadd(dadd(dadd(dmul(dx, dx), dmul(dy, dy)), dmul(dz, dz)), soft2);
  const double inv = r2 > 0.0 ? 1.0 / dmul(r2, sqrt(r2)) : 0.0;
  A[0] = dadd(A[0], dmul(dmul(dx, inv), mj));
  A[1] = dadd(A[1], dmul(dmul(dy, inv), mj));
  A[2] = dadd(A[2], dmul(dmul(dz, inv), mj));
}

struct SimChargedArgs {
  int S, per_wg, N, T, freq, T_save;
  double dt, max_F, strength;
  const double* loc0; const double* vel0;   // [S][3][N] (already clamped / normalised)
  const double* q;                          // [S][N]
  double* loc_out; double* vel_out;         // [S][T_save][3][N]
};

// thread -> (trajectory, particle): G trajectories of N particles per workgroup
struct SimSlot {
  int s, i, base;   // trajectory, particle, first LDS slot of the trajectory
  bool act;
};
__device__ __forceinline__ SimSlot sim_slot(int S, int N, int G) {
  SimSlot r;
  const int t = threadIdx.x, ls = t / N;
  r.i = t - ls * N;
  r.s = blockIdx.x * G + ls;
  r.base = ls * N;
  r.act = ls < G && r.s < S;
  return r;
}

__global__ __launch_bounds__(1024) void sim_charged_kernel(SimChargedArgs a) {
  __shared__ double sx[3][SIM_NMAX];
  __shared__ double sq[SIM_NMAX];
  __shared__ double sn[SIM_NMAX];   // |x_j|^2 (ChargedParticlesSim._l2's row norms)
  const int N = a.N;
  const SimSlot sl = sim_slot(a.S, N, a.per_wg);
  const int s = sl.s, i = sl.i, o = sl.base;
  const bool act = sl.act;
  double x[3] = {0.0, 0.0, 0.0}, v[3] = {0.0, 0.0, 0.0}, qi = 0.0;
  if (act) {
    for (int d = 0; d < 3; ++d) {
      x[d] = a.loc0[((size_t)s * 3 + d) * N + i];
      v[d] = a.vel0[((size_t)s * 3 + d) * N + i];
    }
    qi = a.q[(size_t)s * N + i];
    sq[o + i] = qi;
  }
  auto kick = [&]() {
    if (act) {
      sx[0][o + i] = x[0]; sx[1][o + i] = x[1]; sx[2][o + i] = x[2];
      sn[o + i] = sim_norm2(x);
    }
    __syncthreads();
    if (act) {
      double F[3] = {0.0, 0.0, 0.0};
      const double ni = sn[o + i];
      // the sums keep the reference's j order
#pragma unroll 4
      for (int j = 0; j < N; ++j)
        sim_charged_pair(F, j == i, x, ni, qi, sx[0][o + j], sx[1][o + j], sx[2][o + j], sn[o + j], sq[o + j],
                         a.strength);
      sim_charged_kick(v, F, a.max_F, a.dt);
    }
    __syncthreads();
  };
  kick();   // the half step before the loop (synthetic_sim.py:240-262)
  int counter = 0;
  for (int t = 1; t < a.T; ++t) {
    if (act)
      for (int d = 0; d < 3; ++d) x[d] = dfma(a.dt, v[d], x[d]);
    if (t % a.freq == 0) {
      if (act && counter < a.T_save)
        for (int d = 0; d < 3; ++d) {
          const size_t o = (((size_t)s * a.T_save + counter) * 3 + d) * N + i;
          a.loc_out[o] = x[d];
          a.vel_out[o] = v[d];
        }
      ++counter;
    }
    kick();
  }
}

struct SimGravityArgs {
  int S, per_wg, N, T, freq, T_save;
  double dt, G, soft2;
  const double* pos0; const double* vel0;   // [S][N][3]
  const double* m;                          // [S][N]
  double* pos_out; double* vel_out; double* force_out;   // [S][T_save][N][3]
};

__global__ __launch_bounds__(1024) void sim_gravity_kernel(SimGravityArgs a) {
  __shared__ double sx[3][SIM_NMAX];
  __shared__ double sm[SIM_NMAX];
  const int N = a.N;
  const SimSlot sl = sim_slot(a.S, N, a.per_wg);
  const int s = sl.s, i = sl.i, o = sl.base;
  const bool act = sl.act;
  double x[3] = {0.0, 0.0, 0.0}, v[3] = {0.0, 0.0, 0.0}, acc[3] = {0.0, 0.0, 0.0}, mi = 0.0;
  if (act) {
    for (int d = 0; d < 3; ++d) {
      x[d] = a.pos0[((size_t)s * N + i) * 3 + d];
      v[d] = a.vel0[((size_t)s * N + i) * 3 + d];
    }
    mi = a.m[(size_t)s * N + i];
    sm[o + i] = mi;
  }
  auto accel = [&]() {   // compute_acceleration_batch (synthetic_sim.py:458-481)
    if (act) { sx[0][o + i] = x[0]; sx[1][o + i] = x[1]; sx[2][o + i] = x[2]; }
    __syncthreads();
    if (act) {
      double A[3] = {0.0, 0.0, 0.0};
#pragma unroll 4
      for (int j = 0; j < N; ++j) sim_gravity_pair(A, x, sx[0][o + j], sx[1][o + j], sx[2][o + j], sm[o + j], a.soft2);
      for (int d = 0; d < 3; ++d) acc[d] = dmul(a.G, A[d]);
    }
    __syncthreads();
  };
  accel();
  const double hdt = a.dt / 2.0;
  for (int t = 0; t < a.T; ++t) {
    if (t % a.freq == 0 && act) {
      const int k = t / a.freq;
      for (int d = 0; d < 3; ++d) {
        const size_t o = (((size_t)s * a.T_save + k) * N + i) * 3 + d;
        a.pos_out[o] = x[d];
        a.vel_out[o] = v[d];
        a.force_out[o] = dmul(acc[d], mi);
      }
    }
    if (act)
      for (int d = 0; d < 3; ++d) {
        v[d] = dfma(acc[d], hdt, v[d]);   // (1/2) kick
        x[d] = dfma(v[d], a.dt, x[d]);    // drift
      }
    accel();
    if (act)
      for (int d = 0; d < 3; ++d) v[d] = dfma(acc[d], hdt, v[d]);
  }
}

// trajectories per workgroup and threads per workgroup
int sim_group(int N) { return N <= 32 ? 64 / N : 1; }
int sim_block(int N) { return N <= 32 ? 64 : ((N + 63) / 64) * 64; }

// ---- tiled simulators: any N up to SIMT_NMAX, one launch per time step ----
// A workgroup owns SIMT_R receivers of one trajectory, one thread each (x, v, m_i / q_i in registers), and
// stages that trajectory's senders through LDS SIMT_C at a time; every thread accumulates over j = 0 .. N-1 in
// ascending order with the helpers above, so the sums are the resident kernels' sums bit for bit. Positions are
// double-buffered in the workspace as SoA planes (a step reads `cur`, which every workgroup of the trajectory
// reads, and writes the drifted positions to `nxt`); the kernel boundary orders the steps.
#ifndef NONODE_SIM_TILE_RECEIVERS
#define NONODE_SIM_TILE_RECEIVERS 256
#endif
#ifndef NONODE_SIM_TILE_SENDERS
#define NONODE_SIM_TILE_SENDERS 512
#endif
constexpr int SIMT_R = NONODE_SIM_TILE_RECEIVERS, SIMT_C = NONODE_SIM_TILE_SENDERS;
constexpr int SIMT_NMAX = 1 << 20;
static_assert(SIMT_R % 64 == 0 && SIMT_R >= 64 && SIMT_R <= 1024 && SIMT_C >= 1 && SIMT_C <= 2048, "tile shape");

// workspace (doubles, M = S N): pos[2][3][M] (buffer, axis, particle), then vel[M][3]
struct SimTiledWs {
  double* pos[2];
  double* vel;
};
SimTiledWs sim_tiled_ws(void* workspace, size_t M) {
  double* w = (double*)workspace;
  return {{w, w + 3 * M}, w + 6 * M};
}

// the initial state into the workspace: src element (s, i, d) at s * 3 N + i * stride_i + d * stride_d
__global__ __launch_bounds__(256) void sim_tiled_init_kernel(int S, int N, int stride_i, int stride_d,
                                                             const double* x0, const double* v0, double* pos,
                                                             double* vel) {
  const size_t M = (size_t)S * N, p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= M) return;
  const size_t s = p / N, i = p - s * N;
  for (int d = 0; d < 3; ++d) {
    const size_t o = s * 3 * N + i * stride_i + (size_t)d * stride_d;
    pos[d * M + p] = x0[o];
    vel[p * 3 + d] = v0[o];
  }
}

struct SimTiledSlot {
  int s, i, tid;
  size_t p;     // s N + i, the particle's index in the workspace planes
  size_t row;   // s N, the first particle of the trajectory
  bool act;
};
__device__ __forceinline__ SimTiledSlot sim_tiled_slot(int N, int tiles) {
  SimTiledSlot r;
  r.tid = threadIdx.x;
  r.s = blockIdx.x / tiles;
  r.i = (blockIdx.x - r.s * tiles) * SIMT_R + r.tid;
  r.act = r.i < N;
  r.row = (size_t)r.s * N;
  r.p = r.row + (r.act ? r.i : 0);
  return r;
}

struct SimGravityTiledArgs {
  int N, tiles, T_save, t, freq;
  double dt, G, soft2;
  size_t M;
  const double* m;                                       // [S][N]
  const double* cur; double* nxt; double* vel;           // workspace planes
  double* pos_out; double* vel_out; double* force_out;   // [S][T_save][N][3]
};

__global__ __launch_bounds__(SIMT_R) void sim_gravity_tiled_kernel(SimGravityTiledArgs a) {
  __shared__ double sx[3][SIMT_C];
  __shared__ double sm[SIMT_C];
  const int N = a.N;
  const SimTiledSlot sl = sim_tiled_slot(N, a.tiles);
  double x[3], v[3], A[3] = {0.0, 0.0, 0.0};
  for (int d = 0; d < 3; ++d) {
    x[d] = a.cur[d * a.M + sl.p];
    v[d] = a.vel[sl.p * 3 + d];
  }
  const double mi = a.m[sl.p];
  for (int c0 = 0; c0 < N; c0 += SIMT_C) {
    const int n = N - c0 < SIMT_C ? N - c0 : SIMT_C;
    if (c0) __syncthreads();
    for (int k = sl.tid; k < n; k += SIMT_R) {
      const size_t q = sl.row + c0 + k;
      sx[0][k] = a.cur[q]; sx[1][k] = a.cur[a.M + q]; sx[2][k] = a.cur[2 * a.M + q];
      sm[k] = a.m[q];
    }
    __syncthreads();
    if (sl.act) {
#pragma unroll 4
      for (int j = 0; j < n; ++j) sim_gravity_pair(A, x, sx[0][j], sx[1][j], sx[2][j], sm[j], a.soft2);
    }
  }
  if (!sl.act) return;
  const double hdt = a.dt / 2.0;
  double acc[3];
  for (int d = 0; d < 3; ++d) {
    acc[d] = dmul(a.G, A[d]);
    if (a.t > 0) v[d] = dfma(acc[d], hdt, v[d]);   // the second half kick of step t - 1
  }
  if (a.t % a.freq == 0) {
    const size_t o = (((size_t)sl.s * a.T_save + a.t / a.freq) * N + sl.i) * 3;
    for (int d = 0; d < 3; ++d) {
      a.pos_out[o + d] = x[d];
      a.vel_out[o + d] = v[d];
      a.force_out[o + d] = dmul(acc[d], mi);
    }
  }
  for (int d = 0; d < 3; ++d) {
    v[d] = dfma(acc[d], hdt, v[d]);   // (1/2) kick
    a.vel[sl.p * 3 + d] = v[d];
    a.nxt[d * a.M + sl.p] = dfma(v[d], a.dt, x[d]);   // drift
  }
}

struct SimChargedTiledArgs {
  int N, tiles, T_save, row;   // row: the sample row this step writes, or -1
  double dt, max_F, strength;
  size_t M;
  const double* q;                               // [S][N]
  const double* cur; double* nxt; double* vel;   // workspace planes
  double* loc_out; double* vel_out;              // [S][T_save][3][N]
};

__global__ __launch_bounds__(SIMT_R) void sim_charged_tiled_kernel(SimChargedTiledArgs a) {
  __shared__ double sx[3][SIMT_C];
  __shared__ double sq[SIMT_C];
  __shared__ double sn[SIMT_C];   // |x_j|^2
  const int N = a.N;
  const SimTiledSlot sl = sim_tiled_slot(N, a.tiles);
  double x[3], v[3], F[3] = {0.0, 0.0, 0.0};
  for (int d = 0; d < 3; ++d) {
    x[d] = a.cur[d * a.M + sl.p];
    v[d] = a.vel[sl.p * 3 + d];
  }
  const double qi = a.q[sl.p], ni = sim_norm2(x);
  for (int c0 = 0; c0 < N; c0 += SIMT_C) {
    const int n = N - c0 < SIMT_C ? N - c0 : SIMT_C;
    if (c0) __syncthreads();
    for (int k = sl.tid; k < n; k += SIMT_R) {
      const size_t p = sl.row + c0 + k;
      const double xj[3] = {a.cur[p], a.cur[a.M + p], a.cur[2 * a.M + p]};
      sx[0][k] = xj[0]; sx[1][k] = xj[1]; sx[2][k] = xj[2];
      sn[k] = sim_norm2(xj);
      sq[k] = a.q[p];
    }
    __syncthreads();
    if (sl.act) {
      const int jself = sl.i - c0;
#pragma unroll 4
      for (int j = 0; j < n; ++j)
        sim_charged_pair(F, j == jself, x, ni, qi, sx[0][j], sx[1][j], sx[2][j], sn[j], sq[j], a.strength);
    }
  }
  if (!sl.act) return;
  sim_charged_kick(v, F, a.max_F, a.dt);
  for (int d = 0; d < 3; ++d) {
    x[d] = dfma(a.dt, v[d], x[d]);
    a.vel[sl.p * 3 + d] = v[d];
    a.nxt[d * a.M + sl.p] = x[d];
  }
  if (a.row >= 0)
    for (int d = 0; d < 3; ++d) {
      const size_t o = (((size_t)sl.s * a.T_save + a.row) * 3 + d) * N + sl.i;
      a.loc_out[o] = x[d];
      a.vel_out[o] = v[d];
    }
}

// the checks the two tiled entries share; 0 or a status with the message set
int sim_tiled_check(const char* who, int S, int N, int n_min, int T, int sample_freq, bool null_ptr,
                    const void* workspace, size_t workspace_bytes) {
  if (S <= 0 || N < n_min || N > SIMT_NMAX || (long long)S * N >= (1ll << 31) || T <= 0 || sample_freq <= 0 ||
      T % sample_freq)
    return fail(NONODE_EINVAL, "%s: S=%d N=%d T=%d sample_freq=%d (N in [%d, %d], S N < 2^31, sample_freq divides T)",
                who, S, N, T, sample_freq, n_min, SIMT_NMAX);
  if (null_ptr || !workspace) return fail(NONODE_EINVAL, "%s: null pointer", who);
  if (workspace_bytes < nonode_sim_tiled_workspace_bytes(S, N))
    return fail(NONODE_EINVAL, "%s: workspace %zu < %zu", who, workspace_bytes, nonode_sim_tiled_workspace_bytes(S, N));
  if ((uintptr_t)workspace % alignof(double))
    return fail(NONODE_EINVAL, "%s: workspace is not 8-byte aligned", who);
  return NONODE_OK;
}

}  // namespace

extern "C" {

int nonode_sim_charged(int S, int N, int T, int sample_freq, double dt, double max_F, double strength,
                       const double* loc0, const double* vel0, const double* charges, double* loc_out,
                       double* vel_out, void* stream) {
  if (S <= 0 || N < 2 || N > SIM_NMAX || T <= 0 || sample_freq <= 0 || T % sample_freq)
    return fail(NONODE_EINVAL, "sim_charged: S=%d N=%d T=%d sample_freq=%d", S, N, T, sample_freq);
  if (!loc0 || !vel0 || !charges || !loc_out || !vel_out) return fail(NONODE_EINVAL, "sim_charged: null pointer");
  const int G = sim_group(N);
  SimChargedArgs a{S, G, N, T, sample_freq, T / sample_freq - 1, dt, max_F, strength, loc0, vel0, charges, loc_out,
                   vel_out};
  ProfScope prof(PROF_SIM_CHARGED, (hipStream_t)stream);
  hipLaunchKernelGGL(sim_charged_kernel, dim3((S + G - 1) / G), dim3(sim_block(N)), 0, (hipStream_t)stream, a);
  return check_launch("sim_charged_kernel");
}

int nonode_sim_gravity(int S, int N, int T, int sample_freq, double dt, double G, double softening,
                       const double* pos0, const double* vel0, const double* mass, double* pos_out, double* vel_out,
                       double* force_out, void* stream) {
  if (S <= 0 || N < 1 || N > SIM_NMAX || T <= 0 || sample_freq <= 0 || T % sample_freq)
    return fail(NONODE_EINVAL, "sim_gravity: S=%d N=%d T=%d sample_freq=%d", S, N, T, sample_freq);
  if (!pos0 || !vel0 || !mass || !pos_out || !vel_out || !force_out)
    return fail(NONODE_EINVAL, "sim_gravity: null pointer");
  const int Gs = sim_group(N);
  SimGravityArgs a{S, Gs, N, T, sample_freq, T / sample_freq, dt, G, softening * softening, pos0, vel0, mass,
                   pos_out, vel_out, force_out};
  ProfScope prof(PROF_SIM_GRAVITY, (hipStream_t)stream);
  hipLaunchKernelGGL(sim_gravity_kernel, dim3((S + Gs - 1) / Gs), dim3(sim_block(N)), 0, (hipStream_t)stream, a);
  return check_launch("sim_gravity_kernel");
}

int nonode_sim_tiled_shape(int* receivers, int* senders) {
  if (!receivers || !senders) return fail(NONODE_EINVAL, "sim_tiled_shape: null pointer");
  *receivers = SIMT_R;
  *senders = SIMT_C;
  return NONODE_OK;
}

size_t nonode_sim_tiled_workspace_bytes(int S, int N) {
  if (S <= 0 || N <= 0 || N > SIMT_NMAX || (long long)S * N >= (1ll << 31)) return 0;
  return 9 * (size_t)S * N * sizeof(double);   // pos[2][3][S N] + vel[S N][3]
}

int nonode_sim_gravity_tiled(int S, int N, int T, int sample_freq, double dt, double G, double softening,
                             const double* pos0, const double* vel0, const double* mass, double* pos_out,
                             double* vel_out, double* force_out, void* workspace, size_t workspace_bytes,
                             void* stream) {
  if (int rc = sim_tiled_check("sim_gravity_tiled", S, N, 1, T, sample_freq,
                               !pos0 || !vel0 || !mass || !pos_out || !vel_out || !force_out, workspace,
                               workspace_bytes))
    return rc;
  hipStream_t st = (hipStream_t)stream;
  const size_t M = (size_t)S * N;
  const SimTiledWs ws = sim_tiled_ws(workspace, M);
  const int tiles = (N + SIMT_R - 1) / SIMT_R;
  ProfScope prof(PROF_SIM_GRAVITY, st);
  hipLaunchKernelGGL(sim_tiled_init_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, S, N, 3, 1, pos0,
                     vel0, ws.pos[0], ws.vel);
  if (int rc = check_launch("sim_tiled_init_kernel")) return rc;
  for (int t = 0; t < T; ++t) {
    SimGravityTiledArgs a{N, tiles, T / sample_freq, t, sample_freq, dt, G, softening * softening, M, mass,
                          ws.pos[t & 1], ws.pos[(t + 1) & 1], ws.vel, pos_out, vel_out, force_out};
    hipLaunchKernelGGL(sim_gravity_tiled_kernel, dim3((unsigned)tiles * S), dim3(SIMT_R), 0, st, a);
    if (int rc = check_launch("sim_gravity_tiled_kernel")) return rc;
  }
  return NONODE_OK;
}

int nonode_sim_charged_tiled(int S, int N, int T, int sample_freq, double dt, double max_F, double strength,
                             const double* loc0, const double* vel0, const double* charges, double* loc_out,
                             double* vel_out, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = sim_tiled_check("sim_charged_tiled", S, N, 2, T, sample_freq,
                               !loc0 || !vel0 || !charges || !loc_out || !vel_out, workspace, workspace_bytes))
    return rc;
  hipStream_t st = (hipStream_t)stream;
  const size_t M = (size_t)S * N;
  const SimTiledWs ws = sim_tiled_ws(workspace, M);
  const int tiles = (N + SIMT_R - 1) / SIMT_R;
  ProfScope prof(PROF_SIM_CHARGED, st);
  hipLaunchKernelGGL(sim_tiled_init_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, S, N, 1, N, loc0,
                     vel0, ws.pos[0], ws.vel);
  if (int rc = check_launch("sim_tiled_init_kernel")) return rc;
  // step t kicks at x_t and drifts to x_{t+1}, the sample of step t + 1; the kick and drift of step T - 1 reach
  // no sample (the reference's last kick is unused as well), so that launch is left out
  for (int t = 0; t + 1 < T; ++t) {
    const int row = (t + 1) % sample_freq == 0 ? (t + 1) / sample_freq - 1 : -1;
    SimChargedTiledArgs a{N, tiles, T / sample_freq - 1, row, dt, max_F, strength, M, charges, ws.pos[t & 1],
                          ws.pos[(t + 1) & 1], ws.vel, loc_out, vel_out};
    hipLaunchKernelGGL(sim_charged_tiled_kernel, dim3((unsigned)tiles * S), dim3(SIMT_R), 0, st, a);
    if (int rc = check_launch("sim_charged_tiled_kernel")) return rc;
  }
  return NONODE_OK;
}

}  // extern "C"
