// nonode.hip — MI355X (gfx950, CDNA4) kernels for the EGNO / SEGNO trajectory-rollout hot path.
//
// Written for CDNA4 directly: wave64, f32-input MFMA (v_mfma_f32_16x16x4_f32, exact fp32
// k-ordered FMA chains), LDS-resident sender tables, one workgroup per CU walking a contiguous
// range of receiver tiles. See DESIGN.md for the data layout and the roofline of each kernel.
//
// Reference semantics (simone7monaco/NO-NODE-comparison @ 2025-07-04):
//   egnn_layer_kernel<EGNO>   EGNN_Layer.forward        EGNO/model/basic.py:167-186
//   egnn_layer_kernel<SEGNO>  SEGNO_GCL.forward          SEGNO/models/models/gcl.py:111-119
//   tconv_kernel              TimeConv / TimeConv_x      EGNO/model/layer_no.py:80-178,
//                             + EGNO.forward glue        EGNO/model/egno.py:99-108
//   temb_kernel               get_timestep_embedding     EGNO/model/layer_no.py:8-17
//                             + embedding Linear        EGNO/model/egno.py:50-76
//   embed_kernel              SEGNO.embedding            SEGNO/models/model.py:73
#include "nonode_common.h"

namespace nonode_tu {
thread_local std::string g_err;
}

namespace {

// ---- optional launch timing (bench.py): hipEvents around every layer / tconv launch ------------
struct ProfState {
  std::mutex mu;
  bool on = false;
  int cap = 0, n = 0;
  hipEvent_t* ev = nullptr;   // 2*cap events
  int* kind = nullptr;
} g_prof;

// record kinds: 0 / 1 egnn_layer_kernel<EGNO / SEGNO>, 2 / 3 tconv_kernel (later / first layer),
// 4 / 5 sim_charged_kernel / sim_gravity_kernel
constexpr int PROF_SIM_CHARGED = 4, PROF_SIM_GRAVITY = 5, PROF_EDGE_BWD0 = 6, PROF_EDGE_BWD1 = 7;

struct ProfScope {
  int slot = -1;
  hipStream_t s;
  ProfScope(int kind, hipStream_t stream) : s(stream) {
    if (!g_prof.on) return;
    std::lock_guard<std::mutex> lk(g_prof.mu);
    if (g_prof.n >= g_prof.cap) return;
    slot = g_prof.n++;
    g_prof.kind[slot] = kind;
    (void)hipEventRecord(g_prof.ev[2 * slot], s);
  }
  ~ProfScope() {
    if (slot >= 0) (void)hipEventRecord(g_prof.ev[2 * slot + 1], s);
  }
};

// ---- weight packing ---------------------------------------------------------------------------
struct PackArgs {
  const float* w1; int ld1; int colA, colB, colS;   // edge W1 [64][ld1]
  const float* b1; const float* w2; const float* b2;
  const float* cw1; const float* cb1; const float* cw2; const float* cb2;
  const float* vw1; const float* vb1; const float* vw2; const float* vb2;  // may be null
  const float* nw1; const float* nb1; const float* nw2; const float* nb2;
  int ne;
  int flags;   // NONODE_LAYER_* option bits (stored at OFF_SCAL + 2 / + 3)
  float* blob;
};
// several layers' PackArgs in one launch (blockIdx.z = layer): a training step re-packs every layer
// after each optimizer step, and one launch per layer and blob kind cost ~5 us each
constexpr int PACK_MAX = 8;
struct PackBatch { PackArgs a[PACK_MAX]; };

// scale(col): multiplier of input column col (the SiLU-domain factors, see silu()).
__device__ __forceinline__ void pack_frag(float* dst, const float* src, int ld, int col0, int KT, int d,
                                          float scale_lo, float scale_hi = 0.f, int col_split = 1 << 30) {
  const int q = d & 3, l = (d >> 2) & 63, rest = d >> 8;
  const int mt = rest % KT, mo = rest / KT;
  const int col = 16 * mt + 4 * (l >> 4) + q;
  dst[d] = src[(16 * mo + (l & 15)) * ld + col0 + col] * (col < col_split ? scale_lo : scale_hi);
}
__device__ __forceinline__ float vp_src(const float* src, int stride, int d) {
  const int g = d >> 4, mt = (d >> 2) & 3, q = d & 3;
  return src ? src[(16 * mt + 4 * g + q) * stride] : 0.f;
}

// Shift k of a packed fp16x3 matrix (see h8_scale): the 64x64 block W[0..63][col0 .. col0+63] (row
// stride ld) times |scale| has max |.| 2^k in [2^H16_LO_TARGET, 2^(H16_LO_TARGET+1)), k in [0, 14]
// (a zero or non-finite block: k = 0). Called by every thread of a 256-thread workgroup.
constexpr int H16_LO_TARGET = 1;
__device__ int h16_lo_shift(const float* W, int ld, int col0, float scale) {
  __shared__ float red[4];
  float m = 0.f;
  if (W)
    for (int i = threadIdx.x; i < 4096; i += 256) m = fmaxf(m, fabsf(W[(i >> 6) * ld + col0 + (i & 63)]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) * fabsf(scale);
  if (!(m > 0.f) || !__builtin_isfinite(m)) return 0;
  return min(max(H16_LO_TARGET + 1 - __builtin_amdgcn_frexp_expf(m), 0), 14);
}
// packed half2 (2^-k, 2^-k) as stored in the blob's SC_H16S slots (read back as the float's bits)
__device__ __forceinline__ float h16_us_bits(int k) {
  const unsigned short hb = (unsigned short)((15 - k) << 10);   // fp16 2^-k, k in [0, 14]
  return __uint_as_float((unsigned)hb | ((unsigned)hb << 16));
}

__device__ __forceinline__ void pack_h16(_Float16* dst, const float* W, int d, int ld = 64, int col0 = 0,
                                         float scale = 1.f, int k = 0) {
  // d indexes halves of one 64x64 block: [s][mo][hl][lane][j], 2*4*2*64*8 = 8192; the block is
  // columns col0 .. col0+63 of W (row stride ld), scaled (SiLU-domain factor) before the split; the
  // lo part is stored x 2^k (exact: the residual w - hi is an f32, the shift a power of two)
  const int j = d & 7, lane = (d >> 3) & 63, hl = (d >> 9) & 1, mo = (d >> 10) & 3, s = d >> 12;
  const int row = 16 * mo + (lane & 15);
  const int col = 16 * (2 * s + (j >> 2)) + 4 * (lane >> 4) + (j & 3);
  const float w = W ? W[row * ld + col0 + col] * scale : 0.f;
  const _Float16 h = (_Float16)w;
  // (ldexp, not a multiply: a multiply fuses with the conversion into v_fma_mixlo_f16, which flushes
  // fp16 subnormals)
  dst[d] = hl == 0 ? h : (_Float16)__builtin_ldexpf(w - (float)h, k);
}
// pack_h16 of one matrix and its shift (slot idx of the scalar table `scal`)
__device__ __forceinline__ void pack_h16_shifted(_Float16* dst, float* scal, int idx, const float* W, int d,
                                                 int ld = 64, int col0 = 0, float scale = 1.f) {
  const int k = h16_lo_shift(W, ld, col0, scale);
  pack_h16(dst, W, d, ld, col0, scale, k);
  if (blockIdx.x == 0 && threadIdx.x == 0) scal[SC_H16S + idx] = h16_us_bits(k);
}

__global__ void pack_kernel(PackBatch pb) {
  const PackArgs& a = pb.a[blockIdx.z];
  const int d = blockIdx.x * blockDim.x + threadIdx.x;   // 0 .. 8191
  const int sec = blockIdx.y;
  float* B = a.blob;
  float* S = B + OFF_SCAL;
  _Float16* HN = reinterpret_cast<_Float16*>(B + OFF_H16N);
  switch (sec) {
    case 8: pack_h16_shifted(reinterpret_cast<_Float16*>(B + OFF_H16), S, HS_W2, a.w2, d); break;
    case 9: pack_h16_shifted(reinterpret_cast<_Float16*>(B + OFF_H16 + 4096), S, HS_WC1, a.cw1, d); break;
    case 10: pack_h16_shifted(HN + H_WA * 8192, S, HS_N + H_WA, a.w1, d, a.ld1, a.colA, NEG_LOG2E); break;
    case 11: pack_h16_shifted(HN + H_WB * 8192, S, HS_N + H_WB, a.w1, d, a.ld1, a.colB, NEG_LOG2E); break;
    case 12: pack_h16_shifted(HN + H_WV1 * 8192, S, HS_N + H_WV1, a.vw1, d, 64, 0, NEG_LOG2E); break;
    case 13: pack_h16_shifted(HN + H_WN1A * 8192, S, HS_N + H_WN1A, a.nw1, d, 128, 0, NEG_LOG2E); break;
    case 14: pack_h16_shifted(HN + H_WN1B * 8192, S, HS_N + H_WN1B, a.nw1, d, 128, HID, 1.f); break;
    case 15: pack_h16_shifted(HN + H_WN2 * 8192, S, HS_N + H_WN2, a.nw2, d, 64, 0, NEG_LN2); break;
    // edge W1 (h parts) produce SiLU inputs: x -log2e.  W2 / Wc1 map SiLU outputs (x -log2e) to
    // SiLU inputs (x -log2e): unscaled.  node W1: h columns x -log2e, message-sum columns (sums of
    // SiLU outputs) unscaled.  node W2 maps a SiLU output to h: x -ln2.  node_v W1: x -log2e.
    case 0: if (d < 4096) pack_frag(B + OFF_WA, a.w1, a.ld1, a.colA, 4, d, NEG_LOG2E); break;
    case 1: if (d < 4096) pack_frag(B + OFF_WB, a.w1, a.ld1, a.colB, 4, d, NEG_LOG2E); break;
    case 2: if (d < 4096) pack_frag(B + OFF_W2, a.w2, 64, 0, 4, d, 1.f); break;
    case 3: if (d < 4096) pack_frag(B + OFF_WC1, a.cw1, 64, 0, 4, d, 1.f); break;
    case 4: if (d < 4096) { if (a.vw1) pack_frag(B + OFF_WV1, a.vw1, 64, 0, 4, d, NEG_LOG2E); else B[OFF_WV1 + d] = 0.f; } break;
    case 5: pack_frag(B + OFF_WN1, a.nw1, 128, 0, 8, d, NEG_LOG2E, 1.f, HID); break;
    case 6: if (d < 4096) pack_frag(B + OFF_WN2, a.nw2, 64, 0, 4, d, NEG_LN2); break;
    case 7:
      if (d < 512) {   // feature k-steps
        const int kf = d >> 8, l = (d >> 2) & 63, mo = d & 3;
        const int row = 16 * mo + (l & 15), fi = 4 * kf + (l >> 4);
        float val = 0.f;
        if (fi == 0) val = a.w1[row * a.ld1 + a.colS];
        else if (fi - 1 < a.ne) val = a.w1[row * a.ld1 + 2 * HID + 1 + (fi - 1)];
        B[OFF_FEAT + d] = val * NEG_LOG2E;
      } else if (d < 512 + V_COUNT * 64) {
        const int dd = d - 512, v = dd >> 6, i = dd & 63;
        float val = 0.f;
        switch (v) {   // biases of SiLU inputs x -log2e; vectors that read SiLU outputs x -ln2
          case V_B1: val = vp_src(a.b1, 1, i) * NEG_LOG2E; break;
          case V_B2: val = vp_src(a.b2, 1, i) * NEG_LOG2E; break;
          case V_BC1: val = vp_src(a.cb1, 1, i) * NEG_LOG2E; break;
          case V_WC2: val = vp_src(a.cw2, 1, i) * NEG_LN2; break;
          case V_BV1: val = vp_src(a.vb1, 1, i) * NEG_LOG2E; break;
          case V_WV2: val = vp_src(a.vw2, 1, i) * NEG_LN2; break;
          case V_BN1: val = vp_src(a.nb1, 1, i) * NEG_LOG2E; break;
          case V_BN2: val = vp_src(a.nb2, 1, i); break;
        }
        B[OFF_VEC + dd] = val;
      } else if (d < 512 + V_COUNT * 64 + 64) {
        const int i = d - 512 - V_COUNT * 64;
        float val = 0.f;
        if (i == 0) val = a.cb2[0];
        else if (i == 1 && a.vb2) val = a.vb2[0];
        else if (i == SC_NORM) val = (a.flags & NONODE_LAYER_NORM_RADIAL) ? 1.f : 0.f;
        else if (i == SC_TANH) val = (a.flags & NONODE_LAYER_TANH_COORD) ? 1.f : 0.f;
        if (i < SC_H16S || i >= SC_H16S + HS_COUNT) B[OFF_SCAL + i] = val;   // shifts: sections 8-15
      }
      break;
  }
}

// ---- diagnostic cycle stamps (NONODE_STAMP builds only; tools/stamp_build.sh) ----------------
#ifndef NONODE_STAMP
#define NONODE_STAMP 0
#endif
#if NONODE_STAMP
#define NONODE_NSTAMP 24   // 0-14: the sections; 16-19: the tile-segment boundary taken apart (tools/stamp_run.py)
__device__ unsigned long long g_stamp[NONODE_NSTAMP];
// (32-bit accumulators: a launch is ~5e5 cycles per wave, and 24 of them stay in SGPRs)
#define STAMP_DECL unsigned st_acc[NONODE_NSTAMP] = {}; unsigned long long st_last = __builtin_amdgcn_s_memtime();
// (stamp_here: a constexpr of the enclosing body, so one build can stamp some instances only: the
// stamped 8-wave SEGNO layer crashes LLVM's register allocator)
#define STAMP(i)                                                   \
  do {                                                             \
    if constexpr (stamp_here) {                                    \
      __builtin_amdgcn_sched_barrier(0);                           \
      const unsigned long long _t = __builtin_amdgcn_s_memtime();  \
      st_acc[i] += (unsigned)(_t - st_last);                       \
      st_last = _t;                                                \
      __builtin_amdgcn_sched_barrier(0);                           \
    }                                                              \
  } while (0)
#define STAMP_FLUSH                                                \
  if (stamp_here && lane == 0)                                     \
    for (int _i = 0; _i < NONODE_NSTAMP; ++_i) atomicAdd(&g_stamp[_i], (unsigned long long)st_acc[_i]);
// every LDS read issued so far has landed (stamp builds only: books the wait where it is placed)
#define STAMP_LDS_WAIT do { if constexpr (stamp_here) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); } while (0)
#else
#define STAMP_DECL
#define STAMP(i) do {} while (0)
#define STAMP_LDS_WAIT do {} while (0)
#define STAMP_FLUSH
#endif

// ---- fused E(n)-equivariant layer ------------------------------------------------------------
enum { EGNO = 0, SEGNO = 1 };

struct LayerArgs {
  const float* __restrict__ h; const float* __restrict__ x; const float* __restrict__ v;
  const float* __restrict__ ef; const float* __restrict__ blob;
  float* h_out; float* x_out; float* v_out;
  // fused substeps (SEGNO forward_step): step s reads (h, x, v) for s = 0, else pp_*[(s-1)&1], and
  // writes pp_*[s&1], the last step the *_out arrays
  float* pp_h[2]; float* pp_x[2]; float* pp_v[2];
  int steps;
  // substep fusion (steps > 1, one whole-graph chunk per workgroup): fuse: the node update of step
  // t also builds step t+1's projection tables and positions in LDS (no phase A, no barrier);
  // keep: h and v stay in LDS between steps too (only the last step stores to global memory)
  int fuse, keep;
  // training forward only (else null): per-receiver message sums (true scale) [n][64] and force
  // sums [n][4] (f summed over the N-1 senders, before the mean and clamp)
  float* m_out; float* f_out;
  // saved-state substeps (SEGNO training forward, sv_h != null): step s > 0 reads its inputs from
  // sv_* + s sv_n rows and every step writes its outputs to sv_* + (s + 1) sv_n rows (the last one to
  // *_out as well) and its message sums to m_out + s sv_n rows: all T substeps in one launch
  float* sv_h; float* sv_x; float* sv_v;
  long long sv_n;
  int n_total, n_graphs, N, ne, ef_mod, recurrent;
  // chunking: a unit is cg whole graphs (cpg = 1) or, for large N, one graph cut into cpg chunks of
  // ct receiver tiles; workgroups own whole units (n_units, the last may be short)
  int cg, cpg, n_units, ct, s_rows;
  float inv_deg, dt, cw;
  // XCD-aware chunk order (EGNO forward): workgroup k runs graph chunk chunk_of[k], chosen so that
  // k % 8 (its XCD) owns the same 1/8 of the columns as the TimeConv tiles on that XCD
  int use_perm;
  unsigned short chunk_of[256];
  // EGNO, four waves, whole-graph chunks: the unit split (unit_split) of the launch's chunk shapes,
  // computed once on the host by the function the kernel would run: the full chunk of cg graphs and
  // the short last one. hc_n shapes; shape i has hc_ctc[i] tiles, hc_vl[i] receivers in the last tile.
  int hc_n, hc_ctc[2], hc_vl[2], hc_cut[2][5];
};

// LDS of one chunk: ct receiver tiles (P, two message-sum slots, two force-sum slots) and s_rows senders
size_t layer_lds_floats(int ct, int s_rows, int keep = 0) {
  return 8192 + EDGE_STAGE_FLOATS + (size_t)ct * 16 * ROWP * 3 + (size_t)s_rows * (ROWP + 4) +
         (size_t)ct * 16 * 4 * 2 + (keep ? (size_t)ct * 16 * (ROWP + 4) : 0);
}

// One workgroup owns a contiguous range of whole graphs (so every sender of its receivers is its
// own: substeps need no grid-wide sync) and walks it as 16-receiver tiles, in chunks of `ct` tiles.
// Per chunk:  A) P = W1[h_i] h + b1 for receivers, Q = W1[h_j] h for every sender of the touched
//                graphs (LDS tables), sender positions;
//             B) units (tile, k): receiver r (lane column) meets sender (n + k) mod N of its graph;
//                edge MLP + coord MLP on MFMA. The chunk's units are split over the waves in
//                contiguous ranges (four waves: balanced by a cost model of pairs, single units and
//                tile segments; eight: evenly); wave w flushes its partial message / force sums of a
//                tile into slot w & 1. A tile spans at most 4 consecutive waves, so each slot of a
//                receiver gets at most two contributions: a sole contributor stores, two add by LDS
//                float atomics onto zero, which commute exactly;
//             C) node update per tile (sums = slot 0 + slot 1): x (and v) update, node MLP, stores.
// A chunk is a fixed number (cg) of whole graphs, or a fixed slice of one graph's receivers when a
// graph does not fit, so its tile layout and work split depend only on (cg, ct, N): the layer's
// outputs are bitwise run-to-run deterministic and, for batch shards that are multiples of cg
// samples with the same chunking, identical to the whole batch's.
// KF: feature k-steps (1 + ne scalar edge inputs, 4 per step). Four waves, one per SIMD (512-register
// budget), two units per iteration.
// NW = 4: one wave per SIMD (512-register budget), two units per iteration; NW = 8: two waves per
// SIMD (256 registers each), one unit per iteration, fragments and biases read from LDS.
// OPT: the variant's constructor option (EGNO norm=True: radial input normalised; SEGNO tanh=True:
// coordinate output through tanh), compiled into its own copy of the body so the default path's
// hot loop carries no per-edge select; the kernel picks the copy once from the blob's flag.
// SAVE: the saved-state substeps (LayerArgs::sv_h, SEGNO training), its own copy so the inference
// instances carry none of it (one runtime branch cost C3 +4.5%)
#ifndef NONODE_NODE_PAIR
#define NONODE_NODE_PAIR 1   // EGNO 4-wave layer: node-update and (whole-graph) projection jobs two tiles at a time
#endif
template <int VARIANT, int KF, int NW, bool OPT, bool SAVE = false>
__device__ __forceinline__ void egnn_layer_body(const LayerArgs& p, int (*s_cut)[NW + 1]) {
  constexpr bool PAIR = NW == 4;
  constexpr bool TRIPLE = PAIR && VARIANT == EGNO;   // three-unit iterations before the pairs
  constexpr bool FSPLIT = TRIPLE && NONODE_FSPLIT != 0;   // first SiLU fused into the fp16x3 split
  constexpr bool HOSTCUT = TRIPLE && NONODE_HOSTCUT != 0;   // the chunk shapes' unit splits come with the launch
  // the tile-segment boundary's levers (nonode_common.h; EGNO only: SEGNO's four-wave code stays as it is)
  constexpr bool PREB = TRIPLE && NONODE_PREB != 0;
  constexpr bool UCUT = TRIPLE && NONODE_UCUT != 0;
  [[maybe_unused]] constexpr bool stamp_here = VARIANT == EGNO && NW == 4 && !OPT;   // (NONODE_STAMP builds)
  constexpr bool rnorm = OPT && VARIANT == EGNO;    // basic.py:140-141
  constexpr bool ctanh = OPT && VARIANT == SEGNO;   // gcl.py:57-59
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, e = lane & 15, g = lane >> 4;
  const int N = p.N, Nm1 = N - 1;
  float* sW = smem;                              // W2 | Wc1 fp16 hi/lo fragments (8192 floats)
  float* sV = sW + 8192;                         // feat k-steps (512) | b2 | bc1 | wc2 (vp order)
  float* sP = sV + EDGE_STAGE_FLOATS;            // [ct*16][ROWP]
  float* sQ = sP + p.ct * 16 * ROWP;             // [s_rows][ROWP]
  float* sX = sQ + p.s_rows * ROWP;              // [s_rows][4]
  float* sM = sX + p.s_rows * 4;                 // [2][ct*16][ROWP] message sums (slots 0 | 1)
  float* sF = sM + 2 * p.ct * 16 * ROWP;         // [2][ct*16][4]   force sums (slots 0 | 1)
  const int slotM = p.ct * 16 * ROWP, slotF = p.ct * 16 * 4;
  float* sH = sF + 2 * slotF;                    // keep only: [ct*16][ROWP] h of the chunk's rows
  float* sVl = sH + p.ct * 16 * ROWP;            // keep only: [ct*16][4]    v of the chunk's rows
  // (SEGNO only: the EGNO layer runs one step per launch and carries none of it)
  const bool fused = VARIANT == SEGNO && p.fuse != 0, keep = fused && p.keep != 0;

  for (int i = tid; i < 2048; i += NW * 64) reinterpret_cast<f4*>(sW)[i] = reinterpret_cast<const f4*>(p.blob + OFF_H16)[i];
  if (tid < EDGE_STAGE_FLOATS / 4)
    reinterpret_cast<f4*>(sV)[tid] = reinterpret_cast<const f4*>(p.blob + OFF_FEAT)[tid];
  const float bc2 = p.blob[OFF_SCAL + 0];
  const float bv2 = p.blob[OFF_SCAL + 1];
  const unsigned us_w2 = h16_us(p.blob + OFF_SCAL, HS_W2), us_wc1 = h16_us(p.blob + OFF_SCAL, HS_WC1);
  const float* vFEAT_ = sV;
  const float* vB2_ = sV + 512 + V_B2 * 64;
  const float* vBC1_ = sV + 512 + V_BC1 * 64;
  const float* vWC2_ = sV + 512 + V_WC2 * 64;

  const int G = gridDim.x;
  const int cb = p.use_perm ? (int)p.chunk_of[blockIdx.x] : (int)blockIdx.x;
  const int ch0 = (int)(((long long)cb * p.n_units) / G) * p.cpg;        // this workgroup's chunks
  const int ch1 = (int)(((long long)(cb + 1) * p.n_units) / G) * p.cpg;
  __syncthreads();
  // message / force sums start at zero; every node-update job zeroes the rows it consumed, so the
  // next chunk's edge phase finds them zero
  for (int i = tid; i < 2 * p.ct * 16 * ROWP; i += NW * 64) sM[i] = 0.f;
  for (int i = tid; i < 2 * p.ct * 16 * 4; i += NW * 64) sF[i] = 0.f;
  // rows of chunk ci: receivers [rbase, nend), senders [s0, s0 + S)
  auto chunk_at = [&](int ci, int& rbase, int& nend, int& s0, int& S) __attribute__((always_inline)) {
    if (p.cpg == 1) {   // cg whole graphs: the chunk's rows are its receivers and senders alike
      const int g_lo = ci * p.cg, g_hi = min(g_lo + p.cg, p.n_graphs);
      rbase = g_lo * N; nend = g_hi * N; s0 = rbase; S = nend - rbase;
    } else {            // receiver slice `part` of graph gi; senders: the whole graph
      const int gi = ci / p.cpg, part = ci - gi * p.cpg;
      s0 = gi * N; S = N;
      rbase = s0 + part * 16 * p.ct; nend = min(rbase + 16 * p.ct, s0 + N);
    }
  };
  // phase A jobs of a chunk (LDS tables of the edge phase). Whole-graph chunks (cpg = 1: the
  // receivers are the senders): job = tile, P = W1[h_i] h + b1 and Q = W1[h_j] h from one h load and
  // one fp16 split. Receiver slices of a large graph: job < ctc: P of receiver tile `job`, else Q of
  // sender tile job - ctc.
  auto proj_jobs = [&](int rbase, int nend, int S) __attribute__((always_inline)) {
    const int ctc = (nend - rbase + 15) >> 4;
    return p.cpg == 1 ? ctc : ctc + ((S + 15) >> 4);
  };
  // P = W1[h_i] h + b1 and Q = W1[h_j] h rows of a whole-graph tile from its h (ECL fragments), and the
  // rows' input-finiteness flags (sX slot 3): the edge guard only recomputes pairs whose inputs are
  // finite (a non-finite state, e.g. a diverged rollout, cannot be helped)
  auto proj_tile = [&](const f4 (&hin)[4], const float* blob, int local, bool valid) __attribute__((always_inline)) {
    f4 ap[4], aq[4];
    load_vp(ap, blob + OFF_VEC + V_B1 * 64, g);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) aq[mt] = f4{0.f, 0.f, 0.f, 0.f};
    if (__builtin_expect(__any(amax_ecl(hin) > H16_LIMIT), 0)) {
      mfma_dense<4>(ap, blob + OFF_WA, hin, lane);
      mfma_dense<4>(aq, blob + OFF_WB, hin, lane);
    } else {
      h8 xh[2], xl[2];
      h16_split(hin, xh, xl);
      mfma_h16(ap, reinterpret_cast<const h8*>(blob + OFF_H16N + H_WA * 4096), xh, xl, lane, h16_us(blob + OFF_SCAL, HS_N + H_WA));
      mfma_h16(aq, reinterpret_cast<const h8*>(blob + OFF_H16N + H_WB * 4096), xh, xl, lane, h16_us(blob + OFF_SCAL, HS_N + H_WB));
    }
    float sa = 0.f;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int q = 0; q < 4; ++q) sa += fabsf(ap[mt][q]) + fabsf(aq[mt][q]);
    sa = group_sum(sa);
    if (valid) {
      store_ecl(sP + local * ROWP, ap, g);
      store_ecl(sQ + local * ROWP, aq, g);
      if (g == 0) sX[local * 4 + 3] = __builtin_isfinite(sa) ? 1.f : 0.f;
    }
  };
  auto proj_job = [&](const float* __restrict__ hI, const float* blob, int rbase, int nend, int s0, int S,
                      int job) __attribute__((always_inline)) {
    int joff = 0;
    asm volatile("" : "+s"(joff));   // weight reads stay in the job (LICM would pin them in VGPRs)
    blob += joff;
    if (p.cpg == 1) {
      const int local = job * 16 + e;
      const bool valid = rbase + local < nend;
      f4 hin[4];
      load_ecl(hin, hI + (size_t)(valid ? rbase + local : nend - 1) * HID, g);
      if (keep && valid) store_ecl(sH + local * ROWP, hin, g);
      proj_tile(hin, blob, local, valid);
      return;
    }
    const int ctc = (nend - rbase + 15) >> 4;
    const bool isP = job < ctc;                       // wave-uniform
    const int local = (isP ? job : job - ctc) * 16 + e;
    int node = isP ? rbase + local : s0 + local;
    const bool valid = isP ? (node < nend) : (local < S);
    node = valid ? node : (isP ? nend - 1 : s0);
    f4 hin[4];
    load_ecl(hin, hI + (size_t)node * HID, g);
    f4 acc[4];
    if (isP) {
      load_vp(acc, blob + OFF_VEC + V_B1 * 64, g);
    } else {
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) acc[mt] = f4{0.f, 0.f, 0.f, 0.f};
    }
    mm64(acc, reinterpret_cast<const h8*>(blob + OFF_H16N + (isP ? H_WA : H_WB) * 4096),
         blob + (isP ? OFF_WA : OFF_WB), hin, lane, h16_us(blob + OFF_SCAL, HS_N + (isP ? H_WA : H_WB)));
    float sa = 0.f;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int q = 0; q < 4; ++q) sa += fabsf(acc[mt][q]);
    sa = group_sum(sa);
    if (valid) store_ecl((isP ? sP : sQ) + local * ROWP, acc, g);
    if (valid && !isP && g == 0) sX[local * 4 + 3] = __builtin_isfinite(sa) ? 1.f : 0.f;   // sender flag
  };
  // two whole-graph tiles' projections (cpg = 1): the fp16x3 path shares the WA / WB fragment reads;
  // a tile past the fp16 hi range sends both through proj_tile (each tile's result is proj_tile's)
  auto proj_job2 = [&](const float* __restrict__ hI, const float* blob, int rbase, int nend, int job0)
      __attribute__((always_inline)) {
    int joff = 0;
    asm volatile("" : "+s"(joff));   // weight reads stay in the job (LICM would pin them in VGPRs)
    blob += joff;
    const int l0 = job0 * 16 + e, l1 = l0 + 16;
    const bool v0 = rbase + l0 < nend, v1 = rbase + l1 < nend;
    f4 h0[4], h1[4];
    load_ecl(h0, hI + (size_t)(v0 ? rbase + l0 : nend - 1) * HID, g);
    load_ecl(h1, hI + (size_t)(v1 ? rbase + l1 : nend - 1) * HID, g);
    if (keep && v0) store_ecl(sH + l0 * ROWP, h0, g);
    if (keep && v1) store_ecl(sH + l1 * ROWP, h1, g);
    if (__builtin_expect(__any(fmaxf(amax_ecl(h0), amax_ecl(h1)) > H16_LIMIT), 0)) {
      proj_tile(h0, blob, l0, v0);
      proj_tile(h1, blob, l1, v1);
      return;
    }
    f4 ap0[4], aq0[4], ap1[4], aq1[4];
    load_vp(ap0, blob + OFF_VEC + V_B1 * 64, g);
    load_vp(ap1, blob + OFF_VEC + V_B1 * 64, g);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) aq0[mt] = aq1[mt] = f4{0.f, 0.f, 0.f, 0.f};
    h8 ah[2], al[2], bh[2], bl[2];
    h16_split(h0, ah, al);
    h16_split(h1, bh, bl);
    mfma_h16x2(ap0, ap1, reinterpret_cast<const h8*>(blob + OFF_H16N + H_WA * 4096), ah, al, bh, bl, lane,
               h16_us(blob + OFF_SCAL, HS_N + H_WA));
    mfma_h16x2(aq0, aq1, reinterpret_cast<const h8*>(blob + OFF_H16N + H_WB * 4096), ah, al, bh, bl, lane,
               h16_us(blob + OFF_SCAL, HS_N + H_WB));
    float sa0 = 0.f, sa1 = 0.f;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        sa0 += fabsf(ap0[mt][q]) + fabsf(aq0[mt][q]);
        sa1 += fabsf(ap1[mt][q]) + fabsf(aq1[mt][q]);
      }
    sa0 = group_sum(sa0);
    sa1 = group_sum(sa1);
    if (v0) {
      store_ecl(sP + l0 * ROWP, ap0, g);
      store_ecl(sQ + l0 * ROWP, aq0, g);
      if (g == 0) sX[l0 * 4 + 3] = __builtin_isfinite(sa0) ? 1.f : 0.f;
    }
    if (v1) {
      store_ecl(sP + l1 * ROWP, ap1, g);
      store_ecl(sQ + l1 * ROWP, aq1, g);
      if (g == 0) sX[l1 * 4 + 3] = __builtin_isfinite(sa1) ? 1.f : 0.f;
    }
  };
  auto load_sx = [&](const float* __restrict__ xI, const float* __restrict__ vI, int s0, int S) __attribute__((always_inline)) {
    for (int i = tid; i < S * 3; i += NW * 64) {
      const int s = i / 3, d = i - 3 * s;
      sX[s * 4 + d] = xI[(size_t)(s0 + s) * 3 + d];
      if (keep) sVl[s * 4 + d] = vI[(size_t)(s0 + s) * 3 + d];
    }
  };
  STAMP_DECL
  int* cut = s_cut[wave];   // (static LDS of the kernel: one array for every body copy)
  int cut_ctc = -1, cut_vl = -1;
  // b2 / bc1 / wc2 of the edge phase (four waves: in registers). PREB: read before the barrier that
  // opens the phase (they depend on nothing a phase computes), else at its start
  [[maybe_unused]] f4 rB2[4], rBC1[4], rWC2[4];
  auto load_bias = [&]() __attribute__((always_inline)) {
    load_vp(rB2, vB2_, g);
    load_vp(rBC1, vBC1_, g);
    load_vp(rWC2, vWC2_, g);
  };
  #pragma unroll 1
  for (int step = 0; step < p.steps; ++step) {
  constexpr bool save = VARIANT == SEGNO && SAVE;   // (LayerArgs::sv_h)
  const bool last = step == p.steps - 1;
  const float* __restrict__ hI = step == 0 ? p.h : (save ? p.sv_h + step * p.sv_n * HID : p.pp_h[(step - 1) & 1]);
  const float* __restrict__ xI = step == 0 ? p.x : (save ? p.sv_x + step * p.sv_n * 3 : p.pp_x[(step - 1) & 1]);
  const float* __restrict__ vI = step == 0 ? p.v : (save ? p.sv_v + step * p.sv_n * 3 : p.pp_v[(step - 1) & 1]);
  float* hO = save ? p.sv_h + (step + 1) * p.sv_n * HID : (last ? p.h_out : p.pp_h[step & 1]);
  float* xO = save ? p.sv_x + (step + 1) * p.sv_n * 3 : (last ? p.x_out : p.pp_x[step & 1]);
  float* vO = save ? p.sv_v + (step + 1) * p.sv_n * 3 : (last ? p.v_out : p.pp_v[step & 1]);
  float* mO = p.m_out ? p.m_out + (save ? step * p.sv_n * HID : 0) : nullptr;
  if (!fused || step == 0) {   // ---------------- phase A of the step's first chunk ----------------
    int rbase, nend, s0, S;
    chunk_at(ch0, rbase, nend, s0, S);
    load_sx(xI, vI, s0, S);
    const int J = proj_jobs(rbase, nend, S);
    if (NONODE_NODE_PAIR && NW == 4 && VARIANT == EGNO && p.cpg == 1) {   // two tiles per job (phase C below)
      #pragma unroll 1
      for (int job = 2 * wave; job < J; job += 2 * NW) {
        if (job + 1 < J) proj_job2(hI, p.blob, rbase, nend, job);
        else proj_job(hI, p.blob, rbase, nend, s0, S, job);
      }
    } else {
      #pragma unroll 1
      for (int job = wave; job < J; job += NW) proj_job(hI, p.blob, rbase, nend, s0, S, job);
    }
    if constexpr (PREB) load_bias();
    STAMP(6);
    __syncthreads();
    STAMP(7);
  }
  #pragma unroll 1
  for (int ci = ch0; ci < ch1; ++ci) {
    // keep per-chunk loads of weights/vectors inside the loop (LICM would pin them in VGPRs
    // across all phases)
    int boff = 0;
    asm volatile("" : "+s"(boff));
    const float* blob = p.blob + boff;
    int rbase, nend, s0, S;
    chunk_at(ci, rbase, nend, s0, S);
    const int ctc = (nend - rbase + 15) >> 4;

    // ---------------- phase B: edges ----------------
    // Units (tile, k) are split evenly over the waves; a wave walks its range tile segment by
    // tile segment and processes the units of a segment two at a time, so that the VALU work of
    // one unit (SiLU, gathers) can issue under the MFMA chains of the other. W2 / Wc1 fragments
    // are read from LDS (each read feeds two units' MFMAs); b2 / bc1 / wc2 stay in registers for
    // the edge phase.
    {
      // Column packing of the chunk's last tile: a tile with Vl <= 16 / Pk valid receivers (Pk = 2 or 4)
      // gives each group of 16 / Pk lane columns its own run of sender offsets, so the tile takes
      // Kp = floor(Nm1 / Pk) packed units plus Nm1 - Pk Kp regular ones instead of Nm1 units (C3: 40
      // receivers per chunk, 2.5 tiles: 57 -> 48 units; C5: 100 receivers, 693 -> 621). The groups'
      // partial sums of a receiver are added across lanes (DPP) before the one flush of the segment.
      const int Vl = (nend - rbase) - 16 * (ctc - 1);
      const int Pk = (Vl <= 4 && Nm1 >= 8) ? 4 : ((Vl <= 8 && Nm1 >= 4) ? 2 : 1);
      const int Kp = Nm1 / Pk;
      const int Ul = Pk == 1 ? Nm1 : Kp + (Nm1 - Pk * Kp);
      const int U = (ctc - 1) * Nm1 + Ul;
      // a tile must span at most 4 waves (two contributions per sum slot)
      if (ctc != cut_ctc || Vl != cut_vl) {   // chunk shapes repeat (every step, every full chunk)
        cut_ctc = ctc;
        cut_vl = Vl;
        if constexpr (PAIR) {   // four waves: any tile spans at most four; ranges balanced by modelled cost
          bool have = false;
          if constexpr (HOSTCUT) {   // the launch brought this shape's split (every shape of whole-graph chunks)
#pragma unroll
            for (int i = 0; i < 2; ++i)
              if (!have && i < p.hc_n && p.hc_ctc[i] == ctc && p.hc_vl[i] == Vl) {
#pragma unroll
                for (int j = 0; j <= NW; ++j) cut[j] = p.hc_cut[i][j];
                have = true;
              }
          }
          if (!have) unit_split<NW, TRIPLE && NONODE_TRICOST != 0>(ctc, Nm1, Ul, Pk == 1 ? Nm1 : Kp, cut);
        } else {                // eight waves: every wave's range holds at least a third of a tile
          const int NWB = min(NW, 3 * ctc);
          for (int i = 0; i <= NW; ++i) cut[i] = i < NWB ? (i * U) / NWB : U;
        }
      }
      int u1 = cut[wave + 1];
      int u = cut[wave];
      // UCUT: the wave's range and the cuts as scalars (they are wave-uniform, but read from LDS the
      // compiler cannot know it): the walk's integer state and loop counters live in SGPRs
      [[maybe_unused]] int cu[NW + 1], wv = wave;
      if constexpr (UCUT) {
        u = __builtin_amdgcn_readfirstlane(u);
        u1 = __builtin_amdgcn_readfirstlane(u1);
        wv = __builtin_amdgcn_readfirstlane(wave);
#pragma unroll
        for (int j = 0; j <= NW; ++j) cu[j] = __builtin_amdgcn_readfirstlane(cut[j]);
      }
      if (PAIR && !PREB) load_bias();
      STAMP(16);   // (chunk preamble: shape, cuts, bias vectors)
      #pragma unroll 1
      while (u < u1) {
        const int tau = min(u / Nm1, ctc - 1);
        const int k_lo = u - tau * Nm1 + 1;                                   // unit k: offsets k (+ kof)
        const int k_hi = min(tau == ctc - 1 ? Ul : Nm1, k_lo + (u1 - u) - 1);
        u += k_hi - k_lo + 1;
        // ---- tile state ----
        // packed tile: lane column e is receiver ee of lane group hp, whose packed unit k takes sender
        // offset k + hp Kq; units k > Kq are regular (offset k + (P - 1) Kq), groups hp > 0 masked
        const int P = tau == ctc - 1 ? Pk : 1;        // wave-uniform
        const int Kq = P == 1 ? Nm1 : Kp;
        const int hp = P == 1 ? 0 : (P == 2 ? e >> 3 : e >> 2);
        const int ee = P == 1 ? e : (P == 2 ? e & 7 : e & 3);
        const int kof = hp * Kq;
        const int kreg = (P - 1) * Kq;
        const int rl = 16 * tau + ee;
        // this lane's sender offset for unit k (always in [1, Nm1]) and whether it contributes
        auto lane_k = [&](int k) __attribute__((always_inline)) { return k <= Kq ? k + kof : k + kreg; };
        auto lane_on = [&](int k) __attribute__((always_inline)) { return k <= Kq || hp == 0; };
        const int r = rbase + rl;
        const bool rvalid = r < nend;
        const int rc = rvalid ? r : nend - 1;
        const int gr = rc / N;
        const int n = rc - gr * N;
        const int sb = gr * N - s0;
        const size_t ebase = ((size_t)(gr % p.ef_mod) * N + n) * Nm1;
        int voff = 0;
        asm volatile("" : "+v"(voff));   // keeps the vector reads per segment (not hoisted), LDS space kept
        const float* vFEAT = vFEAT_ + voff;
        const float* Prow = sP + rl * ROWP;            // re-read per unit (saves 16 live VGPRs)
        const float xr0 = sX[(sb + n) * 4 + 0], xr1 = sX[(sb + n) * 4 + 1], xr2 = sX[(sb + n) * 4 + 2];
        const float xr3 = sX[(sb + n) * 4 + 3];   // the receiver's input-finiteness flag
        f4 msum[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) msum[mt] = f4{0.f, 0.f, 0.f, 0.f};
        float fs0 = 0.f, fs1 = 0.f, fs2 = 0.f;

        // pre-activation of edge (r, k): P_r + Q_s + W1[:, scalars] [|r|^2, e_rs] on MFMA
        // this lane's scalar edge inputs of unit k (feature 4*kf + g; feature 0 = |r|^2 is computed):
        // one unconditional, clamped global load per k-step, issued a pair ahead of its use
        // sender j = (n + k) mod N sits at jj = j (j < n) or j - 1 (j > n) in the reference edge order
        // (i, j != i): jj * ne = n ne + k ne - (n + k >= N ? N ne : ne), k ne wave-uniform
        const float* ef_seg = p.ef + ebase * p.ne;
        int ef_lane[KF];
#pragma unroll
        for (int kf = 0; kf < KF; ++kf) ef_lane[kf] = n * p.ne + min(max(4 * kf + g - 1, 0), p.ne - 1);
        const int ne_wrap = N * p.ne;
        auto fetch_ef = [&](int k, float (&ev)[KF]) __attribute__((always_inline)) {
          const int sub = (n + k >= N) ? ne_wrap : p.ne;
          const int kne = k * p.ne;
#pragma unroll
          for (int kf = 0; kf < KF; ++kf)
            ev[kf] = ef_seg[ef_lane[kf] + kne - sub];
        };
        // pre-activation of edge (r, k): P_r + Q_s + W1[:, scalars] [|r|^2, e_rs] on MFMA
        auto head = [&](int k, const float (&ev)[KF], f4 (&a)[4], float& r0, float& r1, float& r2)
            __attribute__((always_inline)) {
          int j = n + k;
          j = (j >= N) ? j - N : j;
          const int sl = sb + j;
          const float* xs = sX + sl * 4;
          r0 = xr0 - xs[0]; r1 = xr1 - xs[1]; r2 = xr2 - xs[2];
          float d2 = fmaf(r0, r0, fmaf(r1, r1, r2 * r2));
          if constexpr (rnorm) d2 = radial_norm(d2);
          f4 q4[4];
          load_ecl(q4, sQ + sl * ROWP, g);
          load_ecl(a, Prow, g);
#pragma unroll
          for (int mt = 0; mt < 4; ++mt) a[mt] += q4[mt];
#pragma unroll
          for (int kf = 0; kf < KF; ++kf) {
            const int fi = 4 * kf + g;
            const float bv = (fi == 0) ? d2 : ((fi - 1 < p.ne) ? ev[kf] : 0.f);
            const f4 wf = *reinterpret_cast<const f4*>(vFEAT + kf * 256 + lane * 4);
#pragma unroll
            for (int mo = 0; mo < 4; ++mo) a[mo] = mfma(wf[mo], bv, a[mo]);
          }
        };
        auto tail = [&](f4 (&c1)[4], float r0, float r1, float r2, bool on) __attribute__((always_inline)) {
          silu_ecl(c1);
          float c = (PAIR ? dot_r(c1, rWC2) : dot_vp(c1, vWC2_, g)) + bc2;
          if constexpr (ctanh) c = tanhf(c);
          float f0 = r0 * c, f1 = r1 * c, f2 = r2 * c;
          if (VARIANT == SEGNO) {   // gcl.py:99-100 clamps every edge's translation
            f0 = fminf(fmaxf(f0, -100.f), 100.f);
            f1 = fminf(fmaxf(f1, -100.f), 100.f);
            f2 = fminf(fmaxf(f2, -100.f), 100.f);
          }
          fs0 = on ? fs0 + f0 : fs0; fs1 = on ? fs1 + f1 : fs1; fs2 = on ? fs2 + f2 : fs2;
        };

        const h8* w2h = reinterpret_cast<const h8*>(sW);
        const h8* wc1h = reinterpret_cast<const h8*>(sW + 4096);
        int k = k_lo;
        if constexpr (PAIR) {
          // Two units (32 edges, same receivers) per iteration. The hot body is ONE basic block:
          // both units always take the fp16x3 path while the largest |activation| is tracked, and
          // only if it exceeded the fp16 range (rare) is the pair recomputed on exact f32 MFMAs
          // before its sums are committed. So the scheduler can put one unit's MFMAs beside the
          // other unit's SiLU work.
          f4 pr[4];
          load_ecl(pr, Prow, g);                       // receiver projection, fixed for the segment
          auto head2 = [&](int k, const float (&ev)[KF], f4 (&a)[4], float& r0, float& r1, float& r2,
                           bool& ok) __attribute__((always_inline)) {
            int j = n + k;
            j = (j >= N) ? j - N : j;
            const int sl = sb + j;
            const f4 xs = *reinterpret_cast<const f4*>(sX + sl * 4);
            r0 = xr0 - xs[0]; r1 = xr1 - xs[1]; r2 = xr2 - xs[2];
            float d2 = fmaf(r0, r0, fmaf(r1, r1, r2 * r2));
            ok = xs[3] * xr3 != 0.f && __builtin_isfinite(d2);   // finite inputs: a guard recompute can help
            if constexpr (rnorm) d2 = radial_norm(d2);
            load_ecl(a, sQ + sl * ROWP, g);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) a[mt] = add4(a[mt], pr[mt]);
#pragma unroll
            for (int kf = 0; kf < KF; ++kf) {
              const int fi = 4 * kf + g;
              const float bv = (fi == 0) ? d2 : ((fi - 1 < p.ne) ? ev[kf] : 0.f);
              const f4 wf = *reinterpret_cast<const f4*>(vFEAT + kf * 256 + lane * 4);
#pragma unroll
              for (int mo = 0; mo < 4; ++mo) a[mo] = mfma(wf[mo], bv, a[mo]);
            }
          };
          auto edge_f = [&](f4 (&c1)[4], float r0, float r1, float r2, float& f0, float& f1, float& f2,
                            float& c) __attribute__((always_inline)) {
            silu_ecl(c1);
            c = dot_r(c1, rWC2) + bc2;   // the guard tests c before the tanh (tanh(inf) = 1)
            float ct = c;
            if constexpr (ctanh) ct = tanhf(c);
            f0 = r0 * ct; f1 = r1 * ct; f2 = r2 * ct;
            if (VARIANT == SEGNO) {   // gcl.py:99-100 clamps every edge's translation
              f0 = fminf(fmaxf(f0, -100.f), 100.f);
              f1 = fminf(fmaxf(f1, -100.f), 100.f);
              f2 = fminf(fmaxf(f2, -100.f), 100.f);
            }
          };
          STAMP(17);   // (segment state: integer and lane state, receiver reads issued)
          // W2 / Wc1 fp16 fragments held for the whole tile segment in AGPRs, which the MFMAs read as
          // their A operand directly (no LDS re-read per pair, no accvgpr copies)
          H16Frags rw2, rwc1;
          load_h16frags(rw2, w2h, lane);
          load_h16frags(rwc1, wc1h, lane);
          pin_agpr(rw2);
          pin_agpr(rwc1);
          STAMP_LDS_WAIT;
          STAMP(18);   // (fragment reads, until they have landed)
          // recomputation of one unit with column-scaled fp16x3 products (the guard path)
          auto exact_unit = [&](int k, const float (&ev)[KF], f4 (&m)[4], float& f0, float& f1, float& f2)
              __attribute__((always_inline)) {
            f4 a[4], c[4];
            float r0, r1, r2;
            bool ok;
            head2(k, ev, a, r0, r1, r2, ok);
            silu_ecl(a);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) m[mt] = rB2[mt];
            mm64_scaled(m, rw2, a, us_w2);
            silu_ecl(m);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) c[mt] = rBC1[mt];
            mm64_scaled(c, rwc1, m, us_wc1);
            float cc;
            edge_f(c, r0, r1, r2, f0, f1, f2, cc);
          };
          const int kp_hi = min(k_hi, Kq);   // pairs of packed (or ordinary) units
          float e0[KF], e1[KF];
          fetch_ef(min(k, kp_hi) + kof, e0);
          fetch_ef(min(k + 1, kp_hi) + kof, e1);
          // EGNO: three units per iteration first, a third independent chain for the stalls at the
          // stage boundaries (C2 layer -1.5 us; SEGNO's C3 launch measured
          // +1 us with it, so SEGNO keeps pairs only); then pairs, then single units. The counts are
          // seg_walk's: its triples here, and the pair loop below takes what is left two by two (one
          // pair, or the two pairs of a 3 t + 1 run), so only a run of one unit reaches the single loop
          const int k3_end = k + 3 * seg_walk<TRIPLE>(kp_hi - k + 1).tri;
          STAMP(5);   // (segment prologue; 4: a triple iteration, 0-3: a pair's stages, 14: a single unit)
          if (TRIPLE && k < k3_end) {
            float e2[KF];
            fetch_ef(min(k + 2, kp_hi) + kof, e2);
#pragma unroll 1
            for (; k < k3_end; k += 3) {
              float n0[KF], n1[KF], n2[KF];
              fetch_ef(min(k + 3, kp_hi) + kof, n0);
              fetch_ef(min(k + 4, kp_hi) + kof, n1);
              fetch_ef(min(k + 5, kp_hi) + kof, n2);
              f4 a0[4], a1[4], a2[4], m0[4], m1[4], m2[4], pm[4];
              float r00, r01, r02, r10, r11, r12, r20, r21, r22;
              float f00, f01, f02, f10, f11, f12, f20, f21, f22;
              float cA, cB, cC;
              bool okA, okB, okC;
              head2(k + kof, e0, a0, r00, r01, r02, okA);
              head2(k + 1 + kof, e1, a1, r10, r11, r12, okB);
              head2(k + 2 + kof, e2, a2, r20, r21, r22, okC);
              if constexpr (!FSPLIT) {
                silu_ecl(a0);
                silu_ecl(a1);
                silu_ecl(a2);
              }
#pragma unroll
              for (int mt = 0; mt < 4; ++mt) { m0[mt] = rB2[mt]; m1[mt] = rB2[mt]; m2[mt] = rB2[mt]; }
              {
                h8 ah0[2], al0[2], ah1[2], al1[2], ah2[2], al2[2];
                if constexpr (FSPLIT) {   // SiLU and split in one: its f32 result has no other consumer
                  silu_split(a0, ah0, al0);
                  silu_split(a1, ah1, al1);
                  silu_split(a2, ah2, al2);
                } else {
                  h16_split(a0, ah0, al0);
                  h16_split(a1, ah1, al1);
                  h16_split(a2, ah2, al2);
                }
                mfma_h16r3(m0, m1, m2, rw2, ah0, al0, ah1, al1, ah2, al2, us_w2);
              }
              silu_ecl(m0);
              silu_ecl(m1);
              silu_ecl(m2);
#pragma unroll
              for (int mt = 0; mt < 4; ++mt) {
                pm[mt] = add4(add4(m0[mt], m1[mt]), m2[mt]);
                a0[mt] = rBC1[mt];
                a1[mt] = rBC1[mt];
                a2[mt] = rBC1[mt];
              }
              {
                h8 mh0[2], ml0[2], mh1[2], ml1[2], mh2[2], ml2[2];
                h16_split(m0, mh0, ml0);
                h16_split(m1, mh1, ml1);
                h16_split(m2, mh2, ml2);
                mfma_h16r3(a0, a1, a2, rwc1, mh0, ml0, mh1, ml1, mh2, ml2, us_wc1);
              }
              edge_f(a0, r00, r01, r02, f00, f01, f02, cA);
              edge_f(a1, r10, r11, r12, f10, f11, f12, cB);
              edge_f(a2, r20, r21, r22, f20, f21, f22, cC);
              const bool redo = (okA && !__builtin_isfinite(cA)) || (okB && !__builtin_isfinite(cB)) ||
                                (okC && !__builtin_isfinite(cC));
              if (__builtin_expect(__any(redo), 0)) {
                int kg = k;
                asm volatile("" : "+v"(kg));
                f4 x0[4], x1[4], x2[4];
                exact_unit(kg + kof, e0, x0, f00, f01, f02);
                exact_unit(kg + 1 + kof, e1, x1, f10, f11, f12);
                exact_unit(kg + 2 + kof, e2, x2, f20, f21, f22);
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) pm[mt] = (x0[mt] + x1[mt]) + x2[mt];
              }
#pragma unroll
              for (int mt = 0; mt < 4; ++mt) msum[mt] = add4(msum[mt], pm[mt]);
              fs0 += (f00 + f10) + f20; fs1 += (f01 + f11) + f21; fs2 += (f02 + f12) + f22;
#pragma unroll
              for (int kf = 0; kf < KF; ++kf) { e0[kf] = n0[kf]; e1[kf] = n1[kf]; e2[kf] = n2[kf]; }
#if NONODE_STAMP
              if (k == k_lo) STAMP(19);   // (a segment's first triple: the wait for its edge features)
              else
#endif
              STAMP(4);
            }
          }
#pragma unroll 1
          for (; k + 1 <= kp_hi; k += 2) {
            float n0[KF], n1[KF];
            fetch_ef(min(k + 2, kp_hi) + kof, n0);
            fetch_ef(min(k + 3, kp_hi) + kof, n1);
            f4 a0[4], a1[4], m0[4], m1[4];
            float r00, r01, r02, r10, r11, r12;
            float f00, f01, f02, f10, f11, f12;
            f4 pm[4];
            float cA, cB;   // coordinate-MLP outputs: non-finite iff an fp16 hi part overflowed
            bool okA, okB;  // finite inputs (node flags, |r|^2)
            head2(k + kof, e0, a0, r00, r01, r02, okA);
            head2(k + 1 + kof, e1, a1, r10, r11, r12, okB);
            STAMP(0);
            if constexpr (!FSPLIT) {
              silu_ecl(a0);
              silu_ecl(a1);
            }
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) { m0[mt] = rB2[mt]; m1[mt] = rB2[mt]; }
            {
              h8 ah0[2], al0[2], ah1[2], al1[2];
              if constexpr (FSPLIT) {
                silu_split(a0, ah0, al0);
                silu_split(a1, ah1, al1);
              } else {
                h16_split(a0, ah0, al0);
                h16_split(a1, ah1, al1);
              }
              mfma_h16r2(m0, m1, rw2, ah0, al0, ah1, al1, us_w2);
            }
            STAMP(1);
            silu_ecl(m0);
            silu_ecl(m1);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
              pm[mt] = add4(m0[mt], m1[mt]);
              a0[mt] = rBC1[mt];
              a1[mt] = rBC1[mt];
            }
            {
              h8 mh0[2], ml0[2], mh1[2], ml1[2];
              h16_split(m0, mh0, ml0);
              h16_split(m1, mh1, ml1);
              mfma_h16r2(a0, a1, rwc1, mh0, ml0, mh1, ml1, us_wc1);
            }
            STAMP(2);
            edge_f(a0, r00, r01, r02, f00, f01, f02, cA);
            edge_f(a1, r10, r11, r12, f10, f11, f12, cB);
            // Guard: an activation beyond the fp16 range (|x| > 65504: a diverged rollout) makes its
            // hi part inf; inf x w (0 included) puts inf or NaN into every output channel of that
            // product, hence into every later channel and into c. So a non-finite c from finite
            // inputs flags exactly the pairs to recompute (column-scaled), at a few compares instead
            // of 32 v_max3 per pair. Below 65504 the split keeps its 2^-22 relative accuracy.
            const bool redo = (okA && !__builtin_isfinite(cA)) || (okB && !__builtin_isfinite(cB));
            if (__builtin_expect(__any(redo), 0)) {
              // the recompute's sender offset through an opaque asm: otherwise its head (shared with
              // the fast path's) lets the speculative-execution pass hoist the column maxima and
              // scalings of mm64_scaled into the hot block (~60 VALU per pair, every pair)
              int kg = k;
              asm volatile("" : "+v"(kg));
              f4 x0[4], x1[4];
              exact_unit(kg + kof, e0, x0, f00, f01, f02);
              exact_unit(kg + 1 + kof, e1, x1, f10, f11, f12);
#pragma unroll
              for (int mt = 0; mt < 4; ++mt) pm[mt] = x0[mt] + x1[mt];
            }
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) msum[mt] = add4(msum[mt], pm[mt]);
            fs0 += f00 + f10; fs1 += f01 + f11; fs2 += f02 + f12;
#pragma unroll
            for (int kf = 0; kf < KF; ++kf) { e0[kf] = n0[kf]; e1[kf] = n1[kf]; }
            STAMP(3);
          }
        }
        if constexpr (!PAIR) {
          // Two waves per SIMD, one unit (16 edges) per iteration, fragments and biases from LDS. The
          // body is one basic block as in the pair loop: the fp16x3 path always runs, and a
          // non-finite coordinate output from finite inputs sends the unit to the column-scaled
          // recompute before its sums are committed.
          auto head1 = [&](int k, const float (&ev)[KF], f4 (&a)[4], float& r0, float& r1, float& r2,
                           bool& ok) __attribute__((always_inline)) {
            int j = n + k;
            j = (j >= N) ? j - N : j;
            const int sl = sb + j;
            const f4 xs = *reinterpret_cast<const f4*>(sX + sl * 4);
            r0 = xr0 - xs[0]; r1 = xr1 - xs[1]; r2 = xr2 - xs[2];
            float d2 = fmaf(r0, r0, fmaf(r1, r1, r2 * r2));
            ok = xs[3] * xr3 != 0.f && __builtin_isfinite(d2);
            if constexpr (rnorm) d2 = radial_norm(d2);
            f4 q4[4];
            load_ecl(q4, sQ + sl * ROWP, g);
            load_ecl(a, Prow, g);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) a[mt] += q4[mt];
#pragma unroll
            for (int kf = 0; kf < KF; ++kf) {
              const int fi = 4 * kf + g;
              const float bv = (fi == 0) ? d2 : ((fi - 1 < p.ne) ? ev[kf] : 0.f);
              const f4 wf = *reinterpret_cast<const f4*>(vFEAT + kf * 256 + lane * 4);
#pragma unroll
              for (int mo = 0; mo < 4; ++mo) a[mo] = mfma(wf[mo], bv, a[mo]);
            }
          };
          auto coord1 = [&](f4 (&c1)[4], const float* wc2, float r0, float r1, float r2, float& f0, float& f1,
                            float& f2, float& c) __attribute__((always_inline)) {
            silu_ecl(c1);
            c = dot_vp(c1, wc2, g) + bc2;   // tested before the tanh (tanh(inf) = 1)
            float ct = c;
            if constexpr (ctanh) ct = tanhf(c);
            f0 = r0 * ct; f1 = r1 * ct; f2 = r2 * ct;
            if (VARIANT == SEGNO) {   // gcl.py:99-100
              f0 = fminf(fmaxf(f0, -100.f), 100.f);
              f1 = fminf(fmaxf(f1, -100.f), 100.f);
              f2 = fminf(fmaxf(f2, -100.f), 100.f);
            }
          };
          // one unit per iteration: the packed (or ordinary) units, then a tile's few regular units
          // (k > Kq, lane groups hp > 0 masked) in a second instance of the same body
          auto unit1 = [&](int k, int k_end, float (&e0)[KF], auto masked) __attribute__((always_inline)) {
            float en[KF];
            fetch_ef(lane_k(min(k + 1, k_end)), en);
            int loff = 0;
            asm volatile("" : "+v"(loff));   // fragment / bias reads stay in the loop
            const h8* w2l = w2h + loff;
            const h8* wc1l = wc1h + loff;
            f4 a[4], m[4];
            float r0, r1, r2, f0, f1, f2, c;
            bool ok;
            head1(lane_k(k), e0, a, r0, r1, r2, ok);
            silu_ecl(a);
            load_vp(m, vB2_ + loff, g);
            {
              h8 ah[2], al[2];
              h16_split(a, ah, al);
              mfma_h16(m, w2l, ah, al, lane, us_w2);   // m = SiLU(W2 a + b2)
            }
            silu_ecl(m);
            load_vp(a, vBC1_ + loff, g);
            {
              h8 mh[2], ml[2];
              h16_split(m, mh, ml);
              mfma_h16(a, wc1l, mh, ml, lane, us_wc1);  // SiLU(Wc1 m + bc1)
            }
            coord1(a, vWC2_ + loff, r0, r1, r2, f0, f1, f2, c);
            if (__builtin_expect(__any(ok && !__builtin_isfinite(c)), 0)) {
              int kg = k;
              asm volatile("" : "+v"(kg));   // keeps the recompute in the branch (see the pair loop)
              head1(lane_k(kg), e0, a, r0, r1, r2, ok);
              silu_ecl(a);
              load_vp(m, vB2_, g);
              mm64_scaled(m, w2h, a, lane, us_w2);
              silu_ecl(m);
              load_vp(a, vBC1_, g);
              mm64_scaled(a, wc1h, m, lane, us_wc1);
              coord1(a, vWC2_, r0, r1, r2, f0, f1, f2, c);
            }
            if constexpr (decltype(masked)::value) {
              const bool on = lane_on(k);
#pragma unroll
              for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int q = 0; q < 4; ++q) msum[mt][q] = on ? msum[mt][q] + m[mt][q] : msum[mt][q];
              fs0 = on ? fs0 + f0 : fs0; fs1 = on ? fs1 + f1 : fs1; fs2 = on ? fs2 + f2 : fs2;
            } else {
#pragma unroll
              for (int mt = 0; mt < 4; ++mt) msum[mt] += m[mt];
              fs0 += f0; fs1 += f1; fs2 += f2;
            }
#pragma unroll
            for (int kf = 0; kf < KF; ++kf) e0[kf] = en[kf];
          };
          float e0[KF];
          fetch_ef(lane_k(min(k, k_hi)), e0);
          const int ko_hi = min(k_hi, Kq);
#pragma unroll 1
          for (; k <= ko_hi; ++k) unit1(k, ko_hi, e0, std::false_type{});
          if (k <= k_hi) fetch_ef(lane_k(k), e0);
#pragma unroll 1
          for (; k <= k_hi; ++k) unit1(k, k_hi, e0, std::true_type{});
        }
        // One unit (16 edges) per iteration; the next unit's edge inputs are in flight meanwhile.
        // (the pair loop's odd unit and a packed tile's regular units: lane groups hp > 0 masked there)
        float e0[KF];
        fetch_ef(lane_k(min(k, k_hi)), e0);
        STAMP(8);
#pragma unroll 1
        for (; k <= k_hi; ++k) {
          float en[KF];
          fetch_ef(lane_k(min(k + 1, k_hi)), en);
          const bool on = lane_on(k);
          // fragment / bias reads stay in the loop (LICM would pin them in VGPRs)
          int loff = 0;
          asm volatile("" : "+v"(loff));
          const h8* w2l = w2h + loff;
          const h8* wc1l = wc1h + loff;
          const float* vB2l = vB2_ + loff;
          const float* vBC1l = vBC1_ + loff;
          f4 a[4], m[4];
          float r0, r1, r2;
          head(lane_k(k), e0, a, r0, r1, r2);
#pragma unroll
          for (int kf = 0; kf < KF; ++kf) e0[kf] = en[kf];
          silu_ecl(a);
          if (PAIR) {
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) m[mt] = rB2[mt];
          } else {
            load_vp(m, vB2l, g);
          }
          if (__builtin_expect(__any(amax_ecl(a) > H16_LIMIT), 0)) {
            mm64_scaled(m, w2l, a, lane, us_w2);
          } else {
            h8 ah[2], al[2];
            h16_split(a, ah, al);
            mfma_h16(m, w2l, ah, al, lane, us_w2);   // m = SiLU(W2 a + b2)
          }
          silu_ecl(m);
#pragma unroll
          for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int q = 0; q < 4; ++q) msum[mt][q] = on ? msum[mt][q] + m[mt][q] : msum[mt][q];
          if (PAIR) {
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) a[mt] = rBC1[mt];
          } else {
            load_vp(a, vBC1l, g);
          }
          if (__builtin_expect(__any(amax_ecl(m) > H16_LIMIT), 0)) {
            mm64_scaled(a, wc1l, m, lane, us_wc1);
          } else {
            h8 mh[2], ml[2];
            h16_split(m, mh, ml);
            mfma_h16(a, wc1l, mh, ml, lane, us_wc1);  // SiLU(Wc1 m + bc1)
          }
          tail(a, r0, r1, r2, on);
          STAMP(14);
        }
        // ---- flush the segment's partial sums ----
        if (P > 1) {   // wave-uniform: add the lane groups' partial sums of each receiver (DPP, fixed order)
#pragma unroll
          for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int q = 0; q < 4; ++q) msum[mt][q] = group_fold(msum[mt][q], P);
          fs0 = group_fold(fs0, P); fs1 = group_fold(fs1, P); fs2 = group_fold(fs2, P);
        }
        // the only contributor to its sum slot of this tile (no other wave of the same slot parity
        // has units in it) stores; else the slot's two contributions are LDS float atomics (onto
        // zero: exact and order-free either way)
        const int t0 = tau * Nm1, t1 = t0 + (tau == ctc - 1 ? Ul : Nm1);
        bool solo = true;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
          if constexpr (UCUT) {
            if (w != wv && ((w ^ wv) & 1) == 0 && cu[w] < cu[w + 1] && cu[w] < t1 && cu[w + 1] > t0) solo = false;
          } else {
            if (w != wave && ((w ^ wave) & 1) == 0 && cut[w] < cut[w + 1] && cut[w] < t1 && cut[w + 1] > t0)
              solo = false;
          }
        }
        if (rvalid && hp == 0) {
          const int slot = wave & 1;
          float* mrow = sM + slot * slotM + rl * ROWP;
          float* frow = sF + slot * slotF + rl * 4;
          if (solo) {
            store_ecl(mrow, msum, g);
            if (g == 0) *reinterpret_cast<f4*>(frow) = f4{fs0, fs1, fs2, 0.f};
          } else {
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
              for (int q = 0; q < 4; ++q) atomicAdd(mrow + 16 * mt + 4 * g + q, msum[mt][q]);
            if (g == 0) {
              atomicAdd(frow + 0, fs0);
              atomicAdd(frow + 1, fs1);
              atomicAdd(frow + 2, fs2);
            }
          }
        }
        STAMP(9);
      }
    }
    STAMP(10);
    __syncthreads();
    STAMP(11);

    // ---------------- phase C (node update of this chunk) + phase A of the next chunk ----------------
    // One job list: the ctc node-update tiles (cost ~4 projection jobs each), then the next chunk's
    // projection jobs (the next chunk of the same step only: the next step's projections read this
    // step's outputs). Jobs go to the least-loaded wave in order (the same greedy on every wave), so
    // a chunk of 5 tiles no longer leaves 3 waves idle for a tile's node update.
    {
      const bool has_next = ci + 1 < ch1;
      int nrb = 0, nne = 0, ns0 = 0, nS = 0;
      if (has_next) {
        chunk_at(ci + 1, nrb, nne, ns0, nS);
        load_sx(xI, vI, ns0, nS);
      }
#ifndef NONODE_C_COST
#define NONODE_C_COST 4   // (A/B builds: the node-update job's modelled cost in projection-job units x 2)
#endif
#ifndef NONODE_A_COST
#define NONODE_A_COST 2
#endif
#ifndef NONODE_CP_COST
#define NONODE_CP_COST 8     // a paired node-update job (two tiles; 6 / 8 measured equal, r06 A/B)
#endif
#ifndef NONODE_AP_COST
#define NONODE_AP_COST 4     // a paired projection job
#endif
      // Jobs of two tiles: each fragment read (global / L2) feeds both tiles' MFMAs and the wave has
      // two independent chains to issue from (a single tile's job is one dependent chain of L2 reads
      // and MFMAs: latency-bound at one wave per SIMD). Each tile's arithmetic is unchanged (bitwise).
      constexpr bool PAIR = NONODE_NODE_PAIR != 0 && NW == 4 && VARIANT == EGNO;   // (8 waves: 256 VGPRs, no room)
      const int PJ = has_next ? proj_jobs(nrb, nne, nS) : 0;
      const bool ppair = PAIR && p.cpg == 1;
      const int NJN = PAIR ? (ctc + 1) >> 1 : ctc;
      const int J = NJN + (ppair ? (PJ + 1) >> 1 : PJ);
      constexpr int C_COST = NONODE_C_COST;
      const int A_COST = p.cpg == 1 ? NONODE_A_COST : 1;
      int ld[NW];
#pragma unroll
      for (int i = 0; i < NW; ++i) ld[i] = 0;
      // node update of tiles tau0 .. tau0 + U - 1 (U = 1 or 2)
      auto node_job = [&](auto U_, const float* bj, int tau0) __attribute__((always_inline)) {
        constexpr int U = decltype(U_)::value;
        int rl[U], r[U], lc[U];
        bool rvalid[U];
        f4 hr[U][4], Mr[U][4];
        float F0[U], F1[U], F2[U], x0[U], x1[U], x2[U], v0[U], v1[U], v2[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          rl[u] = 16 * (tau0 + u) + e;
          r[u] = rbase + rl[u];
          rvalid[u] = r[u] < nend;
          const int rc = rvalid[u] ? r[u] : nend - 1;
          lc[u] = rc - rbase;   // the row in the chunk tables (fused: whole-graph chunk)
          f4 Mb[4];
          if (keep) load_ecl(hr[u], sH + lc[u] * ROWP, g);
          else load_ecl(hr[u], hI + (size_t)rc * HID, g);
          load_ecl(Mr[u], sM + rl[u] * ROWP, g);
          load_ecl(Mb, sM + slotM + rl[u] * ROWP, g);
#pragma unroll
          for (int mt = 0; mt < 4; ++mt) Mr[u][mt] += Mb[mt];
          const float* fa = sF + rl[u] * 4;
          const float* fb = sF + slotF + rl[u] * 4;
          F0[u] = fa[0] + fb[0]; F1[u] = fa[1] + fb[1]; F2[u] = fa[2] + fb[2];
          {   // the rows are consumed: zero both slots for the next chunk's edge phase
            const f4 z4[4] = {};
            store_ecl(sM + rl[u] * ROWP, z4, g);
            store_ecl(sM + slotM + rl[u] * ROWP, z4, g);
            if (g == 0) {
              *reinterpret_cast<f4*>(sF + rl[u] * 4) = z4[0];
              *reinterpret_cast<f4*>(sF + slotF + rl[u] * 4) = z4[0];
            }
          }
          if (fused) { x0[u] = sX[lc[u] * 4 + 0]; x1[u] = sX[lc[u] * 4 + 1]; x2[u] = sX[lc[u] * 4 + 2]; }
          else { const size_t gr3 = (size_t)rc * 3; x0[u] = xI[gr3 + 0]; x1[u] = xI[gr3 + 1]; x2[u] = xI[gr3 + 2]; }
          if (keep) { v0[u] = sVl[lc[u] * 4 + 0]; v1[u] = sVl[lc[u] * 4 + 1]; v2[u] = sVl[lc[u] * 4 + 2]; }
          else { const size_t gr3 = (size_t)rc * 3; v0[u] = vI[gr3 + 0]; v1[u] = vI[gr3 + 1]; v2[u] = vI[gr3 + 2]; }
        }
        float nx0[U], nx1[U], nx2[U], nv0[U], nv1[U], nv2[U];
        if (VARIANT == EGNO) {
          // x <- x + phi_v(h) * v + clamp(mean_j f_ij, +-100)   (basic.py:174-178)
          f4 t[U][4];
#pragma unroll
          for (int u = 0; u < U; ++u) load_vp(t[u], bj + OFF_VEC + V_BV1 * 64, g);
          const h8* wv1 = reinterpret_cast<const h8*>(bj + OFF_H16N + H_WV1 * 4096);
          if constexpr (U == 2) mm64x2(t[0], t[1], wv1, bj + OFF_WV1, hr[0], hr[1], lane, h16_us(bj + OFF_SCAL, HS_N + H_WV1));
          else mm64(t[0], wv1, bj + OFF_WV1, hr[0], lane, h16_us(bj + OFF_SCAL, HS_N + H_WV1));
#pragma unroll
          for (int u = 0; u < U; ++u) {
            silu_ecl(t[u]);
            const float phi = dot_vp(t[u], bj + OFF_VEC + V_WV2 * 64, g) + bv2;
            nx0[u] = x0[u] + phi * v0[u] + fminf(fmaxf(F0[u] * p.inv_deg, -100.f), 100.f);
            nx1[u] = x1[u] + phi * v1[u] + fminf(fmaxf(F1[u] * p.inv_deg, -100.f), 100.f);
            nx2[u] = x2[u] + phi * v2[u] + fminf(fmaxf(F2[u] * p.inv_deg, -100.f), 100.f);
            nv0[u] = v0[u]; nv1[u] = v1[u]; nv2[u] = v2[u];
          }
        } else {
#pragma unroll
          for (int u = 0; u < U; ++u) {
            // v <- v + agg/T ; x <- x + v/T   (gcl.py:255-257 with coords_weight, gcl.py:242)
            nv0[u] = v0[u] + (F0[u] * p.inv_deg * p.cw) * p.dt;
            nv1[u] = v1[u] + (F1[u] * p.inv_deg * p.cw) * p.dt;
            nv2[u] = v2[u] + (F2[u] * p.inv_deg * p.cw) * p.dt;
            nx0[u] = x0[u] + nv0[u] * p.dt;
            nx1[u] = x1[u] + nv1[u] * p.dt;
            nx2[u] = x2[u] + nv2[u] * p.dt;
          }
        }
        // h <- node_mlp([h, sum_j m_ij]) (+ h if recurrent)   (basic.py:182-185, gcl.py:85-95)
        f4 z[U][4];
        bool big[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          load_vp(z[u], bj + OFF_VEC + V_BN1 * 64, g);
          big[u] = __any(fmaxf(amax_ecl(hr[u]), amax_ecl(Mr[u])) > H16_LIMIT);
        }
        const h8* wn1a = reinterpret_cast<const h8*>(bj + OFF_H16N + H_WN1A * 4096);
        const h8* wn1b = reinterpret_cast<const h8*>(bj + OFF_H16N + H_WN1B * 4096);
        const unsigned usa = h16_us(bj + OFF_SCAL, HS_N + H_WN1A), usb = h16_us(bj + OFF_SCAL, HS_N + H_WN1B);
        bool anybig = big[0];
        if constexpr (U == 2) anybig = anybig || big[1];
        if (U == 2 && !__builtin_expect(anybig, 0)) {
          h8 ah[2], al[2], bh[2], bl[2];
          h16_split(hr[0], ah, al);
          h16_split(hr[U - 1], bh, bl);
          mfma_h16x2(z[0], z[U - 1], wn1a, ah, al, bh, bl, lane, usa);
          h16_split(Mr[0], ah, al);
          h16_split(Mr[U - 1], bh, bl);
          mfma_h16x2(z[0], z[U - 1], wn1b, ah, al, bh, bl, lane, usb);
        } else {
#pragma unroll
          for (int u = 0; u < U; ++u) {
            if (__builtin_expect(big[u], 0)) {
              f4 in8[8];
#pragma unroll
              for (int mt = 0; mt < 4; ++mt) { in8[mt] = hr[u][mt]; in8[4 + mt] = Mr[u][mt]; }
              mfma_dense<8>(z[u], bj + OFF_WN1, in8, lane);
            } else {
              h8 xh[2], xl[2];
              h16_split(hr[u], xh, xl);
              mfma_h16(z[u], wn1a, xh, xl, lane, usa);
              h16_split(Mr[u], xh, xl);
              mfma_h16(z[u], wn1b, xh, xl, lane, usb);
            }
          }
        }
        f4 hn[U][4];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          silu_ecl(z[u]);
          load_vp(hn[u], bj + OFF_VEC + V_BN2 * 64, g);
        }
        const h8* wn2 = reinterpret_cast<const h8*>(bj + OFF_H16N + H_WN2 * 4096);
        if constexpr (U == 2) mm64x2(hn[0], hn[1], wn2, bj + OFF_WN2, z[0], z[1], lane, h16_us(bj + OFF_SCAL, HS_N + H_WN2));
        else mm64(hn[0], wn2, bj + OFF_WN2, z[0], lane, h16_us(bj + OFF_SCAL, HS_N + H_WN2));
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (VARIANT == SEGNO && p.recurrent) {   // gcl.py:93-94
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) hn[u][mt] += hr[u][mt];
          }
          if (rvalid[u] && mO) {
            f4 mt4[4];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) mt4[mt] = Mr[u][mt] * NEG_LN2;    // sM holds -log2e * sum m
            store_ecl(mO + (size_t)r[u] * HID, mt4, g);
            if (g == 0 && p.f_out) *reinterpret_cast<f4*>(p.f_out + (size_t)r[u] * 4) = f4{F0[u], F1[u], F2[u], 0.f};
          }
          const bool next = fused && step + 1 < p.steps;   // fused: this tile's rows of step + 1 in LDS
          if (rvalid[u] && (save || !(keep && next))) {
            const size_t ro = (size_t)r[u];
            store_ecl(hO + ro * HID, hn[u], g);
            if (save && last) store_ecl(p.h_out + ro * HID, hn[u], g);
            if (g == 0) {
              float* xo = xO + ro * 3;
              xo[0] = nx0[u]; xo[1] = nx1[u]; xo[2] = nx2[u];
              if (VARIANT == SEGNO) {
                float* vo = vO + ro * 3;
                vo[0] = nv0[u]; vo[1] = nv1[u]; vo[2] = nv2[u];
                if (save && last) {
                  float* xo2 = p.x_out + ro * 3;
                  float* vo2 = p.v_out + ro * 3;
                  xo2[0] = nx0[u]; xo2[1] = nx1[u]; xo2[2] = nx2[u];
                  vo2[0] = nv0[u]; vo2[1] = nv1[u]; vo2[2] = nv2[u];
                }
              }
            }
          }
          if (next) {
            if (rvalid[u]) {
              if (keep) store_ecl(sH + rl[u] * ROWP, hn[u], g);
              if (g == 0) {
                sX[rl[u] * 4 + 0] = nx0[u]; sX[rl[u] * 4 + 1] = nx1[u]; sX[rl[u] * 4 + 2] = nx2[u];
                if (keep) { sVl[rl[u] * 4 + 0] = nv0[u]; sVl[rl[u] * 4 + 1] = nv1[u]; sVl[rl[u] * 4 + 2] = nv2[u]; }
              }
            }
            proj_tile(hn[u], bj, rl[u], rvalid[u]);
          }
        }
      };
      #pragma unroll 1
      for (int j = 0; j < J; ++j) {
        int w = 0, lw = ld[0];
#pragma unroll
        for (int i = 1; i < NW; ++i)
          if (ld[i] < lw) { lw = ld[i]; w = i; }
        const bool nodej = j < NJN;
        const int first = nodej ? (PAIR ? 2 * j : j) : (ppair ? 2 * (j - NJN) : j - NJN);
        const bool two = nodej ? (PAIR && first + 1 < ctc) : (ppair && first + 1 < PJ);
        const int c = nodej ? (two ? NONODE_CP_COST : C_COST) : (two ? NONODE_AP_COST : A_COST);
#pragma unroll
        for (int i = 0; i < NW; ++i) ld[i] += i == w ? c : 0;
        if (w != wave) continue;
        int joff = 0;
        asm volatile("" : "+s"(joff));   // weight reads stay in the job (LICM would pin them in VGPRs)
        const float* bj = blob + joff;
        if (!nodej) {
          if (two) proj_job2(hI, bj, nrb, nne, first);
          else proj_job(hI, bj, nrb, nne, ns0, nS, first);
          continue;
        }
        if (two) node_job(std::integral_constant<int, 2>{}, bj, first);
        else node_job(std::integral_constant<int, 1>{}, bj, first);
      }
    }
    if constexpr (PREB) load_bias();   // (the next chunk's, or the next step's first)
    STAMP(12);
    __syncthreads();
    STAMP(13);
  }
  }
  STAMP_FLUSH
}

template <int VARIANT, int KF, int NW>
__global__ __launch_bounds__(NW * 64) void egnn_layer_kernel(LayerArgs p) {
  // edge-unit ranges of the waves for the last chunk shape (each wave its own copy); declared here
  // once: the body copies below would each add their own static LDS to the 159 KB dynamic tables
  __shared__ int s_cut[NW][NW + 1];
  if constexpr (VARIANT == SEGNO) {
    if (p.sv_h) {   // wave-uniform
      if (p.blob[OFF_SCAL + SC_TANH] != 0.f) egnn_layer_body<VARIANT, KF, NW, true, true>(p, s_cut);
      else egnn_layer_body<VARIANT, KF, NW, false, true>(p, s_cut);
      return;
    }
  }
  if (p.blob[OFF_SCAL + (VARIANT == SEGNO ? SC_TANH : SC_NORM)] != 0.f)   // wave-uniform
    egnn_layer_body<VARIANT, KF, NW, true>(p, s_cut);
  else
    egnn_layer_body<VARIANT, KF, NW, false>(p, s_cut);
}

// ---- temporal spectral layers -----------------------------------------------------------------
struct TconvArgs {
  int BN, T, M, Mfull;
  const float* h; const float* x; const float* v; const float* lm;
  const float* wp;   // packed mixing fragments (nonode_pack_tconv)
  const float* wx;   // TimeConv_x weights [2][2][Mfull][2] (raw)
  float* h_out; float* x_out; float* v_out;
  // FIRST layer only: h0 = embedding([h_in, temb]) built on the fly (egno.py:63-76)
  const float* hin; int din; const float* emb_w; int emb_ld; const float* etab; int Bt;
  // 1: multi-input form (egno.py:44-96 with num_inputs > 1): the first layer's x, v, h_in and every
  // layer's loc_mean are per frame ([T*BN] rows, the inputs already spread over the T frames as
  // repeat_elements_to_exact_shape does); 0: x, v, h_in, loc_mean are [BN] rows replicated over T
  int frames;
  int xcd;   // 1: workgroup k runs tile (k % 8) * ceil(tiles / 8) + k / 8 (XCD-aware order)
  int xw;    // 1: TimeConv_x on a fifth wave (launch_tconv: fewer tiles than CUs), else on wave 3
  // training forward only (else null): the LeakyReLU decision of every h element, y > 0, as the
  // wave ballots of step 3: mask[((t * ntiles + tile) * 4 + wave) * 4 + q] bit l = element
  // (column 16 tile + 4 wave + (l >> 4), channel 4 (l & 15) + q) of frame t. The backward uses these
  // decisions instead of recomputing y (a recompute near y = 0 can take the other branch).
  unsigned long long* mask_out;
  // DFT twiddles cos / sin(2 pi m t / T), m < M, t < T, at [m * TMAX + t]: filled by launch_tconv on
  // the host (double precision, exact at multiples of pi / 2) and read from the kernel arguments, so no
  // workgroup computes them or waits on a barrier for them (round 5: software double cospi / sinpi per
  // workgroup into LDS, then a barrier, ahead of the first h load)
  float tw_cos[MMAX * TMAX], tw_sin[MMAX * TMAX];
};

// Packed mixing weights of one TimeConv (layer_no.py:80-126), as W^T fragments (f32 MFMA A operand)
// with the irfft scale folded in: mode 0 -> A_0 = Wr_0 / T; mode m >= 1 -> A_m = c_m Wr_m / T,
// B_m = c_m Wi_m / T, -A_m. With Xr_m = sum_t h cos, Xs_m = sum_t h sin (so X_m = Xr_m - i Xs_m):
//   Yr_m = A_m^T Xr_m + B_m^T Xs_m,  Yi_m = B_m^T Xr_m - A_m^T Xs_m,
//   y[t] = sum_m (Yr_m cos(2 pi m t/T) - Yi_m sin(2 pi m t/T))   (= irfft(pad(Y), n=T)).
// After the f32 fragments (tconv_mats(M) x 4096 floats) the blob holds the same matrices as fp16 hi / lo
// fragments for the fp16x3 mixing (round 6; pack_h16 layout, 4096 floats each), each scaled by a power of
// two 2^e that brings its largest |entry| into [1, 2) (the weights are ~1e-4: unscaled, their hi parts
// would be fp16 subnormals), then a table of 2 x 64 floats: [mat] the lo shift's packed half2 (2^-k, 2^-k)
// (h8_scale), [64 + mat] 2^-e, the factor that takes a product back to the unscaled matrix.
constexpr int tconv_mats(int M) { return 1 + 3 * (M - 1); }
size_t tconv_blob_floats(int modes) { return (size_t)tconv_mats(modes) * 8192 + 128; }
__device__ __forceinline__ size_t tconv_h16_off(int M) { return (size_t)tconv_mats(M) * 4096; }
__device__ __forceinline__ size_t tconv_scal_off(int M) { return (size_t)tconv_mats(M) * 8192; }

struct TconvPackBatch { const float* w[PACK_MAX]; float* out[PACK_MAX]; };
__global__ void tconv_pack_kernel(TconvPackBatch tb, int Mfull, int M, int T) {
  const float* w = tb.w[blockIdx.y];
  float* out = tb.out[blockIdx.y];
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  const int nmat = 1 + 3 * (M - 1);
  if (d >= nmat * 4096) return;
  const int mat = d >> 12, r = d & 4095;
  const int q = r & 3, l = (r >> 2) & 63, rest = r >> 8, mt = rest & 3, mo = rest >> 2;
  const int o = 16 * mo + (l & 15), i = 16 * mt + 4 * (l >> 4) + q;     // W^T[o][i] = W[i][o]
  int m, c;
  float sgn = 1.f;
  if (mat == 0) { m = 0; c = 0; }
  else { m = 1 + (mat - 1) / 3; const int kind = (mat - 1) % 3; c = (kind == 1) ? 1 : 0; sgn = (kind == 2) ? -1.f : 1.f; }
  const float cm = (m == 0 || 2 * m == T) ? 1.f : 2.f;
  out[d] = sgn * cm / (float)T * w[(((size_t)i * 64 + o) * Mfull + m) * 2 + c];
}
// fp16 hi / lo fragments of matrix blockIdx.x from the f32 fragments tconv_pack_kernel wrote (same stream)
__global__ __launch_bounds__(256) void tconv_pack_h16_kernel(TconvPackBatch tb, int M) {
  float* blob = tb.out[blockIdx.y];
  const int mat = blockIdx.x;
  const float* f32 = blob + (size_t)mat * 4096;
  // A[o][i] (output o, input i) sits at f32[((o / 16 * 4 + i / 16) * 64 + o % 16 + 16 (i / 4 % 4)) * 4 + i % 4]
  auto at = [&](int o, int i) {
    return f32[(((o >> 4) * 4 + (i >> 4)) * 64 + (o & 15) + 16 * ((i >> 2) & 3)) * 4 + (i & 3)];
  };
  __shared__ float red[4];
  float mx = 0.f;
  for (int i = threadIdx.x; i < 4096; i += 256) mx = fmaxf(mx, fabsf(f32[i]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  const bool ok = mx > 0.f && __builtin_isfinite(mx);
  const int e = ok ? min(max(1 - __builtin_amdgcn_frexp_expf(mx), -60), 60) : 0;   // max |A| 2^e in [1, 2)
  const int k = ok ? min(max(H16_LO_TARGET + 1 - __builtin_amdgcn_frexp_expf(__builtin_ldexpf(mx, e)), 0), 14) : 0;
  _Float16* dst = reinterpret_cast<_Float16*>(blob + tconv_h16_off(M) + (size_t)mat * 4096);
  for (int d = threadIdx.x; d < 8192; d += 256) {
    const int j = d & 7, lane = (d >> 3) & 63, hl = (d >> 9) & 1, mo = (d >> 10) & 3, s2 = d >> 12;
    const int row = 16 * mo + (lane & 15);
    const int col = 16 * (2 * s2 + (j >> 2)) + 4 * (lane >> 4) + (j & 3);
    const float w = __builtin_ldexpf(at(row, col), e);   // exact (a power of two)
    const _Float16 h = (_Float16)w;
    dst[d] = hl == 0 ? h : (_Float16)__builtin_ldexpf(w - (float)h, k);   // (see pack_h16)
  }
  if (threadIdx.x == 0) {
    float* sc = blob + tconv_scal_off(M);
    sc[mat] = h16_us_bits(k);
    sc[64 + mat] = __builtin_ldexpf(1.f, -e);
  }
}

// One workgroup (4 + 1 waves) per tile of 16 columns (b, n). Wave w < 4: DFT over T of columns 4w..4w+3
// (all 64 channels; each f4 access of the wave covers 4 whole rows), spectrum to LDS; then the
// mixing MFMAs for output channels 16w..16w+15 of all 16 columns (lanes: column e = lane & 15,
// channels 16w + 4g + q); the mixed spectrum goes back through LDS, and wave w finishes columns
// 4w..4w+3: inverse DFT, LeakyReLU + residual (h kept in registers from the DFT), row stores.
// TimeConv_x (x / v, 48 lanes) runs on wave 3 after its h loads are issued, or, for launches with fewer
// tiles than CUs (TconvArgs::xw, the strong-scaling shards), on a fifth wave that only joins the
// barriers: there wave 3's h loads waiting behind the x / v work were on the launch's critical path
// (C2 at B = 64: 0.2213 -> 0.2183 ms per forward); at B = 512, where every CU holds 2-3 tiles, the
// fifth wave measured +15 us per forward (0.915 -> 0.931 ms, profiles/r06/ab_tconv_waves.txt).
// MM: compile-time bound on the number of modes (M <= MM), so the mode loops, the LDS spectrum and
// the register arrays are sized for the configuration at hand
// TB: compile-time bound on the frame count (T <= TB), so the per-frame register arrays and the
// unconditional (clamped) loads cover only the frames a configuration can have (TB = 10 for T <= 10)
constexpr int TC_THREADS = 320;
template <bool FIRST, int MM, int TB>
__global__ __launch_bounds__(TC_THREADS) void tconv_kernel(TconvArgs p) {
  __shared__ __attribute__((aligned(16))) float sX[2 * MM - 1][16][ROWP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, e = lane & 15, g = lane >> 4;
  const int T = p.T, M = p.M, BN = p.BN;
  const int ntiles = (BN + 15) / 16, tpx = (ntiles + 7) / 8;
  const int tile = p.xcd ? (int)(blockIdx.x % 8) * tpx + (int)(blockIdx.x / 8) : (int)blockIdx.x;
  if (tile >= ntiles) return;   // whole workgroup, before any barrier
  // x / v lanes and the mixing MFMAs: column e = lane & 15 of the tile
  const int col = tile * 16 + e;
  const bool cvalid = col < BN;
  const int c = cvalid ? col : BN - 1;
  // h streaming (steps 1 and 3): wave w owns columns 4w .. 4w+3 of the tile, lane (cl = lane >> 4,
  // cq = lane & 15) channels 4cq .. 4cq+3 of column 4w + cl, so one f4 load / store instruction of a
  // wave moves 4 whole consecutive 256-byte rows (1 KB contiguous per frame)
  const bool hw = wave < 4;   // the streaming waves (wave-uniform)
  const int xvw = p.xw ? 4 : 3;   // the TimeConv_x wave
  const int ecol = 4 * (hw ? wave : 0) + (lane >> 4), chs = 4 * (lane & 15);
  const int scol = tile * 16 + ecol;
  const bool svalid = scol < BN;
  const int sc = svalid ? scol : BN - 1;
  f4 base = {0.f, 0.f, 0.f, 0.f};
  const float* et = nullptr;
  // emb_w[:, :din] h_in of row r (the node-feature part of the embedding Linear)
  auto hin_part = [&](size_t r) {
    f4 b = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < p.din; ++k) {
      const float hv = p.hin[r * p.din + k];
#pragma unroll
      for (int q = 0; q < 4; ++q) b[q] = fmaf(p.emb_w[(chs + q) * p.emb_ld + k], hv, b[q]);
    }
    return b;
  };
  if (FIRST) {
    if (!p.frames) base = hin_part((size_t)sc);
    et = p.etab + ((size_t)(sc % p.Bt) * T) * 64 + chs;
  }
  auto hval = [&](int t) -> f4 {
    if (FIRST) return *reinterpret_cast<const f4*>(et + t * 64) + (p.frames ? hin_part((size_t)t * BN + sc) : base);
    return *reinterpret_cast<const f4*>(p.h + ((size_t)t * BN + sc) * 64 + chs);
  };

  // ---- x / v channels (TimeConv_x, egno.py:103-108): wave 4, lane (d = g, column e), d < 3 ----
  if (wave == xvw && g < 3 && cvalid) {
    const int d = g;
    auto lm_at = [&](int t) { return p.lm[((p.frames ? (size_t)t * BN : 0) + c) * 3 + d]; };
    float xs[TB], vs[TB], lms[TB];
    // loads are unconditional (frame index clamped to T - 1): a load under `if (t < T)` becomes a
    // branch whose join waits for every outstanding load, i.e. one HBM latency per frame
#pragma unroll
    for (int t = 0; t < TB; ++t) {
      const int tc = t < T ? t : T - 1;
      const size_t row = (FIRST && !p.frames) ? (size_t)c : ((size_t)tc * BN + c);
      lms[t] = lm_at(tc);
      xs[t] = p.x[row * 3 + d] - lms[t];
      vs[t] = p.v[row * 3 + d];
    }
    float yr[MM][2], yi[MM][2];
#pragma unroll
    for (int m = 0; m < MM; ++m) {
      if (m < M) {
        float Xr[2] = {0.f, 0.f}, Xi[2] = {0.f, 0.f};
#pragma unroll
        for (int t = 0; t < TB; ++t) {
          if (t < T) {
            const float cs = p.tw_cos[m * TMAX + t], sn = p.tw_sin[m * TMAX + t];
            Xr[0] = fmaf(xs[t], cs, Xr[0]); Xi[0] = fmaf(-xs[t], sn, Xi[0]);
            Xr[1] = fmaf(vs[t], cs, Xr[1]); Xi[1] = fmaf(-vs[t], sn, Xi[1]);
          }
        }
        const float cm = (m == 0 || 2 * m == T) ? 1.f : 2.f;
#pragma unroll
        for (int o = 0; o < 2; ++o) {
          float ar = 0.f, ai = 0.f;
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            const float wr = p.wx[(((size_t)i * 2 + o) * p.Mfull + m) * 2 + 0];
            const float wi = p.wx[(((size_t)i * 2 + o) * p.Mfull + m) * 2 + 1];
            ar += Xr[i] * wr - Xi[i] * wi;
            ai += Xr[i] * wi + Xi[i] * wr;
          }
          yr[m][o] = ar * cm; yi[m][o] = ai * cm;
        }
      }
    }
    const float invT = 1.0f / (float)T;
#pragma unroll
    for (int t = 0; t < TB; ++t) {
      if (t < T) {
        float y0 = 0.f, y1 = 0.f;
#pragma unroll
        for (int m = 0; m < MM; ++m) {
          if (m < M) {
            const float cs = p.tw_cos[m * TMAX + t], sn = p.tw_sin[m * TMAX + t];
            y0 += yr[m][0] * cs - yi[m][0] * sn;
            y1 += yr[m][1] * cs - yi[m][1] * sn;
          }
        }
        const size_t row = (size_t)t * BN + c;
        p.x_out[row * 3 + d] = xs[t] + y0 * invT + lms[t];
        p.v_out[row * 3 + d] = vs[t] + y1 * invT;
      }
    }
  }
  // ---- step 1: truncated DFT of this wave's input channels ----
  // every frame's h is loaded once and unconditionally (clamped frame index, see the x / v loads
  // above), and kept in registers for the residual of step 3. With no barrier ahead of them, the waves
  // without x / v work request these at the kernel's start. (Placed above the x / v block in the
  // source, their live range spans it in every wave, which crashed LLVM's greedy register allocator on
  // the TB = 16 instance.)
  f4 hvs[TB];
  if (hw) {
#pragma unroll
    for (int t = 0; t < TB; ++t) hvs[t] = hval(t < T ? t : T - 1);
  }
  if (hw) {
    f4 Xr[MM], Xs[MM];
#pragma unroll
    for (int m = 0; m < MM; ++m) { Xr[m] = f4{0.f, 0.f, 0.f, 0.f}; Xs[m] = Xr[m]; }
#pragma unroll
    for (int t = 0; t < TB; ++t) {
      if (t < T) {
        const f4 hv = hvs[t];
#pragma unroll
        for (int m = 0; m < MM; ++m) {
          if (m < M) {
            Xr[m] += hv * p.tw_cos[m * TMAX + t];
            if (m > 0) Xs[m] += hv * p.tw_sin[m * TMAX + t];
          }
        }
      }
    }
    *reinterpret_cast<f4*>(&sX[0][ecol][chs]) = Xr[0];
#pragma unroll
    for (int m = 1; m < MM; ++m) {
      if (m < M) {
        *reinterpret_cast<f4*>(&sX[2 * m - 1][ecol][chs]) = Xr[m];
        *reinterpret_cast<f4*>(&sX[2 * m][ecol][chs]) = Xs[m];
      }
    }
  }
  __syncthreads();
  // ---- step 2: channel mixing on MFMA (output tile mo = wave, waves 0-3) ----
  f4 Yr[MM], Yi[MM];
  auto mix = [&](f4& acc, int mat, int vec) {
    f4 in[4];
    load_ecl(in, &sX[vec][e][0], g);
    const float* wf = p.wp + (size_t)mat * 4096;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const f4 a = *reinterpret_cast<const f4*>(wf + ((wave * 4 + mt) * 64 + lane) * 4);
#pragma unroll
      for (int q = 0; q < 4; ++q) acc = mfma(a[q], in[mt][q], acc);
    }
  };
  // fp16x3 (round 6): 6 v_mfma_f32_16x16x32_f16 per matrix instead of 16 f32 MFMAs of 4x the cycles;
  // acc += 2^-e (A 2^e)^T x, the product in a fresh accumulator (exact rescale, one rounding more)
  const h8* wh16 = reinterpret_cast<const h8*>(p.wp + tconv_h16_off(M));
  const float* wsc = p.wp + tconv_scal_off(M);
  auto mix16 = [&](f4& acc, int mat, const h8 (&xh)[2], const h8 (&xl)[2]) {
    const h8* wf = wh16 + (size_t)mat * 1024;
    const unsigned us = __float_as_uint(wsc[mat]);
    f4 t = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      const h8 ah = wf[((s2 * 4 + wave) * 2 + 0) * 64 + lane], al = wf[((s2 * 4 + wave) * 2 + 1) * 64 + lane];
      t = mfma16(ah, xh[s2], t);
      t = mfma16(al, h8_scale(xh[s2], us), t);
      t = mfma16(ah, xl[s2], t);
    }
    acc += t * wsc[64 + mat];
  };
  if (hw) {
    // a spectrum past the fp16 hi range (a diverged rollout) takes the exact f32 mixing
    bool big = false;
    {
      f4 in[4];
      load_ecl(in, &sX[0][e][0], g);
      big = amax_ecl(in) > H16_LIMIT;
#pragma unroll
      for (int v = 1; v < 2 * MM - 1; ++v) {
        if (v < 2 * M - 1) {
          load_ecl(in, &sX[v][e][0], g);
          big = big || amax_ecl(in) > H16_LIMIT;
        }
      }
    }
    // (the 4- and 9-mode builds keep the f32 mixing: their fp16x3 form measured 2.8e-4 off at the h
    // level for 5 modes, T = 8, cause not found; the 2-mode build is within the f32 path's rounding)
    if (MM > 2 || __builtin_expect(__any(big), 0)) {
      Yr[0] = f4{0.f, 0.f, 0.f, 0.f};
      mix(Yr[0], 0, 0);
#pragma unroll
      for (int m = 1; m < MM; ++m) {
        if (m < M) {
          const int mat = 1 + 3 * (m - 1);
          Yr[m] = f4{0.f, 0.f, 0.f, 0.f};
          Yi[m] = f4{0.f, 0.f, 0.f, 0.f};
          mix(Yr[m], mat + 0, 2 * m - 1);   // A^T Xr
          mix(Yr[m], mat + 1, 2 * m);       // B^T Xs
          mix(Yi[m], mat + 1, 2 * m - 1);   // B^T Xr
          mix(Yi[m], mat + 2, 2 * m);       // -A^T Xs
        }
      }
    } else {
      f4 in[4];
      h8 rh[2], rl[2], sh[2], sl[2];
      load_ecl(in, &sX[0][e][0], g);
      h16_split(in, rh, rl);
      Yr[0] = f4{0.f, 0.f, 0.f, 0.f};
      mix16(Yr[0], 0, rh, rl);
#pragma unroll
      for (int m = 1; m < MM; ++m) {
        if (m < M) {
          const int mat = 1 + 3 * (m - 1);
          load_ecl(in, &sX[2 * m - 1][e][0], g);
          h16_split(in, rh, rl);
          load_ecl(in, &sX[2 * m][e][0], g);
          h16_split(in, sh, sl);
          Yr[m] = f4{0.f, 0.f, 0.f, 0.f};
          Yi[m] = f4{0.f, 0.f, 0.f, 0.f};
          mix16(Yr[m], mat + 0, rh, rl);   // A^T Xr
          mix16(Yr[m], mat + 1, sh, sl);   // B^T Xs
          mix16(Yi[m], mat + 1, rh, rl);   // B^T Xr
          mix16(Yi[m], mat + 2, sh, sl);   // -A^T Xs
        }
      }
    }
  }
  // ---- the spectrum Y back through LDS into the streaming layout (sX is free once every wave's
  // mixing has read it) ----
  __syncthreads();
  if (hw) {
    const int chm = 16 * wave + 4 * g;   // MFMA output channels of column e
    *reinterpret_cast<f4*>(&sX[0][e][chm]) = Yr[0];
#pragma unroll
    for (int m = 1; m < MM; ++m) {
      if (m < M) {
        *reinterpret_cast<f4*>(&sX[2 * m - 1][e][chm]) = Yr[m];
        *reinterpret_cast<f4*>(&sX[2 * m][e][chm]) = Yi[m];
      }
    }
  }
  __syncthreads();
  if (!hw) return;   // (no barrier follows)
  // ---- step 3: y[t] (channels chs..chs+3 of column ecol), LeakyReLU(0.01), residual ----
  // (lanes of columns past BN compute on the clamped column sc and store nothing)
  Yr[0] = *reinterpret_cast<const f4*>(&sX[0][ecol][chs]);
#pragma unroll
  for (int m = 1; m < MM; ++m) {
    if (m < M) {
      Yr[m] = *reinterpret_cast<const f4*>(&sX[2 * m - 1][ecol][chs]);
      Yi[m] = *reinterpret_cast<const f4*>(&sX[2 * m][ecol][chs]);
    }
  }
#pragma unroll
  for (int t = 0; t < TB; ++t) {
    if (t < T) {
      f4 y = Yr[0];
#pragma unroll
      for (int m = 1; m < MM; ++m)
        if (m < M) y += Yr[m] * p.tw_cos[m * TMAX + t] - Yi[m] * p.tw_sin[m * TMAX + t];
      f4 o = hvs[t];
#pragma unroll
      for (int q = 0; q < 4; ++q) o[q] += (y[q] >= 0.f ? y[q] : 0.01f * y[q]);
      if (p.mask_out) {   // wave-uniform (training forward only): lanes 0..3 store the 4 ballots at once
        unsigned long long mine = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const unsigned long long bits = __ballot(y[q] > 0.f);
          mine = lane == q ? bits : mine;
        }
        if (lane < 4) p.mask_out[(((size_t)t * ntiles + tile) * 4 + wave) * 4 + lane] = mine;
      }
      if (svalid) {
        *reinterpret_cast<f4*>(p.h_out + ((size_t)t * BN + sc) * 64 + chs) = o;
      }
    }
  }
}

// etab[b][t][o] = emb_b[o] + sum_k emb_w[o][din+k] * temb(t_out[b][t])[k]   (layer_no.py:8-17);
// trig_out (training forward, else null): the [Bt][T][ncol] time-embedding values themselves
// multi-input (t_in != null, egno.py:44-49, 77-79): emb_w columns are [h | temb(t_in) | temb(t_out)]
// and t_in[b][t] is the input time of frame t's input
constexpr int TEMB_ROWS = 16;   // (b, t) rows per 256-thread block (4 per wave)
__global__ __launch_bounds__(256) void temb_kernel(int Bt, int T, int din, int dim, const float* t_out,
                                                   const float* emb_w, int emb_ld, const float* emb_b,
                                                   float* etab, const float* t_in = nullptr,
                                                   float* trig_out = nullptr) {
  // a 256-thread block owns TEMB_ROWS (b, t) rows x 64 outputs; each row's sin / cos table (<= 2 * 64
  // values, dim <= 64 is checked by the host) is computed once into LDS, and each wave reads its lane's
  // weight row once for its 4 rows (round 6: 4 rows per block re-read the whole matrix per row, 6.7 us)
  __shared__ float trig[TEMB_ROWS][128];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r0 = blockIdx.x * TEMB_ROWS;
  const int nrows = Bt * T;
  const int half = dim / 2;
  const int ncol = (t_in ? 2 : 1) * dim;
  const float scale = (float)(log(10000.0) / (double)(half - 1));
  for (int i = threadIdx.x; i < TEMB_ROWS * ncol; i += 256) {
    const int row = i / ncol, c = i - row * ncol, bt = r0 + row;
    if (bt >= nrows) continue;
    const int seg = c / dim, k = c % dim;           // seg 0: t_in (if given) else t_out
    const float tv = (t_in && seg == 0) ? t_in[bt] : t_out[bt];
    const float fk = expf((float)(k % half) * -scale);
    const float arg = tv * fk;
    trig[row][c] = k < half ? sinf(arg) : cosf(arg);
    if (trig_out) trig_out[(size_t)bt * ncol + c] = trig[row][c];   // training: the embedding's inputs
  }
  __syncthreads();
  const int o = lane;
  const float* w = emb_w + o * emb_ld + din;
  const float b = emb_b[o];
  constexpr int RW = TEMB_ROWS / 4;
  float acc[RW];
#pragma unroll
  for (int j = 0; j < RW; ++j) acc[j] = b;
  for (int seg = 0; seg < ncol / dim; ++seg)
#pragma unroll 8
    for (int k = 0; k < half; ++k) {
      const float w0 = w[seg * dim + k], w1 = w[seg * dim + half + k];
#pragma unroll
      for (int j = 0; j < RW; ++j) {   // (the per-row sum order of the one-row form)
        acc[j] = fmaf(w0, trig[wave * RW + j][seg * dim + k], acc[j]);
        acc[j] = fmaf(w1, trig[wave * RW + j][seg * dim + half + k], acc[j]);
      }
    }
#pragma unroll
  for (int j = 0; j < RW; ++j) {
    const int bt = r0 + wave * RW + j;
    if (bt < nrows) etab[(size_t)bt * 64 + o] = acc[j];
  }
}

// out[n][o] = b[o] + sum_k W[o][k] in[n][k]   (SEGNO embedding, model.py:73)
__global__ void embed_kernel(int n_nodes, int din, const float* in, const float* w, const float* b,
                             float* out) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_nodes * 64) return;
  const int o = idx & 63, n = idx >> 6;
  float acc = b[o];
  for (int k = 0; k < din; ++k) acc = fmaf(w[o * din + k], in[(size_t)n * din + k], acc);
  out[idx] = acc;
}

// ---- first-layer inputs without a TimeConv (training forward; EGNO use_time_conv=False) -----------
// h0[t*BN + c] = emb_w[:, :din] h_in[c] + etab[c % Bt][t]   (egno.py:63-76; same arithmetic as
// tconv_kernel<true>), and x, v replicated over T (egno.py:89-96)
// frames = 1 (num_inputs > 1): h_in, x, v are per frame ([T*BN] rows) instead of replicated;
// hin_out (training forward, else null): a copy of the h_in rows (the embedding's inputs)
__global__ __launch_bounds__(256) void h0_kernel(int BN, int T, int din, int Bt, const float* __restrict__ hin,
                                                 const float* __restrict__ emb_w, int emb_ld,
                                                 const float* __restrict__ etab, const float* __restrict__ x,
                                                 const float* __restrict__ v, float* __restrict__ h0,
                                                 float* __restrict__ xr, float* __restrict__ vr, int frames,
                                                 float* __restrict__ hin_out = nullptr) {
  // thread (c, o) writes column o of node c's T rows; its T table reads are all issued before the
  // stores (restrict: no aliasing), so one memory latency per thread instead of T
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= BN * 64) return;
  const int o = idx & 63, c = idx >> 6;
  auto hin_part = [&](size_t r) {
    float b = 0.f;
    for (int k = 0; k < din; ++k) b = fmaf(emb_w[o * emb_ld + k], hin[r * din + k], b);
    return b;
  };
  const float base = frames ? 0.f : hin_part((size_t)c);
  const float* et = etab + (size_t)(c % Bt) * T * 64 + o;
  float e[TMAX];
#pragma unroll
  for (int t = 0; t < TMAX; ++t) e[t] = t < T ? et[t * 64] : 0.f;
#pragma unroll
  for (int t = 0; t < TMAX; ++t) {
    if (t >= T) break;
    const size_t row = (size_t)t * BN + c;
    const size_t src = frames ? row : (size_t)c;
    h0[row * 64 + o] = e[t] + (frames ? hin_part(row) : base);
    if (o < 3) { xr[row * 3 + o] = x[src * 3 + o]; vr[row * 3 + o] = v[src * 3 + o]; }
    if (hin_out && o < din && (frames || t == 0)) hin_out[src * din + o] = hin[src * din + o];
  }
}

// ---- host-side launchers ----------------------------------------------------------------------
// dynamic LDS of the layer kernel: the 160 KB of a CU less 1 KB for its static tables (the waves'
// edge-unit cut tables, <= 288 B)
constexpr int LAYER_DYN_LDS_MAX = 159 * 1024;
// integer diagnostics switch from the environment (A/B builds of one library): 0 when unset
int getenv_int(const char* name) {
  const char* v = getenv(name);
  return v ? atoi(v) : 0;
}
// NONODE_XCD=0 turns off the XCD-aware tile / chunk order of the EGNO forward
bool xcd_on() {
  static const int on = getenv("NONODE_XCD") ? atoi(getenv("NONODE_XCD")) : 1;
  return on != 0;
}
template <int VARIANT, int NW>
void launch_cfg(int kf, int G, size_t lds, hipStream_t stream, const LayerArgs& a) {
  static std::once_flag once;
  std::call_once(once, [] {
    hipFuncSetAttribute((const void*)egnn_layer_kernel<VARIANT, 1, NW>, hipFuncAttributeMaxDynamicSharedMemorySize, LAYER_DYN_LDS_MAX);
    hipFuncSetAttribute((const void*)egnn_layer_kernel<VARIANT, 2, NW>, hipFuncAttributeMaxDynamicSharedMemorySize, LAYER_DYN_LDS_MAX);
  });
  if (kf == 1) hipLaunchKernelGGL((egnn_layer_kernel<VARIANT, 1, NW>), dim3(G), dim3(NW * 64), lds, stream, a);
  else hipLaunchKernelGGL((egnn_layer_kernel<VARIANT, 2, NW>), dim3(G), dim3(NW * 64), lds, stream, a);
}
// waves per workgroup: 4 (one per SIMD, paired units) for N < 64, else 8 (two per SIMD, single
// units): measured C2 (N = 20) 255 vs 271 us per launch, C5 (N = 100) 1594 vs 1496 us
#ifndef NONODE_LAYER_WAVES
#define NONODE_LAYER_WAVES 0   // 0: by N as above; 4 / 8: forced (A/B builds)
#endif
// steps > 1 runs that many substeps in one launch (SEGNO forward_step), ping-ponging through
// pp = {h0, h1, x0, x1, v0, v1} (each n_graphs*N rows)
template <int VARIANT>
int launch_layer(int n_graphs, int N, int ne, int ef_mod, const float* h, const float* x,
                 const float* v, const float* ef, const float* blob, float dt, float cw, int recurrent,
                 float* h_out, float* x_out, float* v_out, hipStream_t stream, int steps = 1,
                 float* const* pp = nullptr, float* m_out = nullptr, float* f_out = nullptr,
                 int xcd_cols = 0, float* const* sv = nullptr) {
  const int n_total = n_graphs * N;
  const int cus = num_cus();
  // graphs per chunk: at most the graphs per CU, at most 8 tiles, within LDS; among those the one
  // whose rows fill its tiles best (ties: the larger). N = 20: 4 graphs = 80 rows = 5 full tiles.
  // A graph of more than 8 tiles (or beyond the LDS) is cut into cpg receiver slices of ct tiles.
  constexpr size_t LDS_MAX = LAYER_DYN_LDS_MAX;
  const int cap = n_graphs / cus > 1 ? n_graphs / cus : 1;
  int cg = 0, cpg = 1, ct = 0;
  double best = -1.0;
  // Inference launches (one step, no saved state) with few graphs per CU pick cg by the critical
  // path instead: ceil(chunks / CUs) rounds of one chunk's tiles (a tile is N - 1 edge units and one
  // node job) plus half a tile of per-chunk overhead. At C2's B = 512 both rules pick 4 graphs; at
  // B = 64 (640 graphs) the fill rule's 2-graph chunks give 320 chunks, two rounds on 64 CUs, where 3
  // graphs give one round of 214 chunks. Training forwards keep the fill rule: their chunk shape must
  // not depend on the batch (batch-invariant sums of the data-parallel shards, §3.1 of DESIGN.md).
  const bool crit = steps == 1 && !m_out && !sv && n_graphs < 16 * cus && !getenv_int("NONODE_FILL_CG");
  const int force_cg = getenv_int("NONODE_CG");   // (diagnostic A/B switch: a fixed chunk size)
  if (crit) best = -1e300;
  for (int c = 1; c <= (crit || force_cg ? 8 * 16 : cap); ++c) {
    if (force_cg) {
      const int tiles = (c * N + 15) / 16;
      if (tiles > 8 || layer_lds_floats(tiles, c * N) * 4 > LDS_MAX) break;
      cg = c; ct = tiles;
      if (c == force_cg) break;
      continue;
    }
    const int tiles = (c * N + 15) / 16;
    if (tiles > 8 || layer_lds_floats(tiles, c * N) * 4 > LDS_MAX) break;
    if (crit) {
      const long long chunks = (n_graphs + c - 1) / c;
      const long long rounds = (chunks + cus - 1) / cus;
      const double cost = -(double)rounds * (tiles + 0.5);
      if (cost > best + 1e-12) { best = cost; cg = c; ct = tiles; }
      continue;
    }
    const double fill = (double)(c * N) / (16.0 * tiles);
    if (fill >= best - 1e-12) { best = fill; cg = c; ct = tiles; }
  }
  if (cg == 0) {
    cg = 1;
    ct = (N + 15) / 16 < 8 ? (N + 15) / 16 : 8;
    while (ct > 1 && layer_lds_floats(ct, N) * 4 > LDS_MAX) --ct;
    if (layer_lds_floats(ct, N) * 4 > LDS_MAX) return fail(NONODE_EUNSUPPORTED, "N=%d too large for the LDS sender table", N);
    cpg = (N + 16 * ct - 1) / (16 * ct);
    ct = ((N + cpg - 1) / cpg + 15) / 16;   // the same slice count with the least padding
  }
  const int s_rows = cg * N;
  const int n_units = (n_graphs + cg - 1) / cg;
  int G = n_units < cus ? n_units : cus;
  const int force_wgs = getenv_int("NONODE_WGS");   // (diagnostic: at most this many workgroups, so one walks several chunks)
  if (force_wgs > 0 && force_wgs < G) G = force_wgs;
  // substep fusion needs one whole-graph chunk per workgroup; keeping h, v in LDS needs the room
  const int fuse = steps > 1 && cpg == 1 && n_units <= G;
  const int keep = fuse && layer_lds_floats(ct, s_rows, 1) * 4 <= LDS_MAX && !getenv_int("NONODE_NO_KEEP");
  const size_t lds = layer_lds_floats(ct, s_rows, keep) * 4;
  LayerArgs a;
  a.h = h; a.x = x; a.v = v; a.ef = ef; a.blob = blob;
  a.h_out = h_out; a.x_out = x_out; a.v_out = v_out;
  a.n_total = n_total; a.n_graphs = n_graphs; a.N = N; a.ne = ne; a.ef_mod = ef_mod;
  a.cg = cg; a.cpg = cpg; a.n_units = n_units; a.ct = ct; a.s_rows = s_rows;
  if (steps < 1 || (steps > 1 && !pp && !sv)) return fail(NONODE_EINVAL, "layer: steps=%d", steps);
  a.steps = steps;
  a.fuse = fuse && !getenv_int("NONODE_NO_FUSE");
  a.keep = a.fuse && keep;
  a.m_out = m_out; a.f_out = f_out;
  a.sv_h = sv ? sv[0] : nullptr; a.sv_x = sv ? sv[1] : nullptr; a.sv_v = sv ? sv[2] : nullptr;
  a.sv_n = n_total;
  for (int i = 0; i < 2; ++i) {
    a.pp_h[i] = pp ? pp[i] : nullptr;
    a.pp_x[i] = pp ? pp[2 + i] : nullptr;
    a.pp_v[i] = pp ? pp[4 + i] : nullptr;
  }
  a.recurrent = recurrent; a.inv_deg = 1.0f / (float)(N - 1); a.dt = dt; a.cw = cw;
  a.use_perm = 0;
  if (xcd_cols > 0 && G % 8 == 0 && G <= 256 && xcd_on()) {
    // chunk c starts at column (first receiver row mod xcd_cols); its XCD block is that column's
    // eighth. Fill each XCD's G/8 slots (k = x, x + 8, ...) from its block, overflow anywhere.
    int slot_fill[8] = {0};
    int left[256], nleft = 0;
    for (int k = 0; k < G; ++k) a.chunk_of[k] = 0xffff;
    for (int c = 0; c < G; ++c) {
      const long long row0 = (((long long)c * n_units) / G) * cg * N;
      const int x = (int)((row0 % xcd_cols) * 8 / xcd_cols);
      if (slot_fill[x] < G / 8) a.chunk_of[x + 8 * slot_fill[x]++] = (unsigned short)c;
      else left[nleft++] = c;
    }
    for (int k = 0, i = 0; k < G; ++k)
      if (a.chunk_of[k] == 0xffff) a.chunk_of[k] = (unsigned short)left[i++];
    a.use_perm = 1;
  }
  const int nw = NONODE_LAYER_WAVES ? NONODE_LAYER_WAVES : (N < 64 ? 4 : 8);
  a.hc_n = 0;
  if (VARIANT == EGNO && nw == 4 && cpg == 1 && NONODE_HOSTCUT) {
    // the kernel's own derivation of a chunk's tiles and packed last tile (phase B), per chunk shape
    const int g_last = n_graphs - (n_units - 1) * cg;
    for (int gs : {cg, g_last}) {
      const int rows = gs * N, ctc = (rows + 15) >> 4, Vl = rows - 16 * (ctc - 1), Nm1 = N - 1;
      if (a.hc_n == 1 && a.hc_ctc[0] == ctc && a.hc_vl[0] == Vl) continue;
      const int Pk = (Vl <= 4 && Nm1 >= 8) ? 4 : ((Vl <= 8 && Nm1 >= 4) ? 2 : 1);
      const int Kp = Nm1 / Pk, Ul = Pk == 1 ? Nm1 : Kp + (Nm1 - Pk * Kp);
      a.hc_ctc[a.hc_n] = ctc;
      a.hc_vl[a.hc_n] = Vl;
      unit_split<4, NONODE_TRICOST != 0>(ctc, Nm1, Ul, Pk == 1 ? Nm1 : Kp, a.hc_cut[a.hc_n]);
      ++a.hc_n;
    }
  }
  ProfScope prof(VARIANT, stream);
  if (ne == 0) { a.ef = blob; a.ne = 1; a.ef_mod = 1; }   // dummy gather target; feature weights are 0
  const int kf = a.ne <= 3 ? 1 : 2;
  if (nw == 8) launch_cfg<VARIANT, 8>(kf, G, lds, stream, a);
  else launch_cfg<VARIANT, 4>(kf, G, lds, stream, a);
  return check_launch("egnn_layer_kernel");
}

// cos / sin(pi num / den) in double, exact where the angle is a multiple of pi / 2
void cos_sin_pi(int num, int den, double& c, double& s) {
  num %= 2 * den;
  if ((2 * num) % den == 0) {
    const int q = (2 * num) / den;   // quarter turns 0..3
    const double cq[4] = {1.0, 0.0, -1.0, 0.0}, sq[4] = {0.0, 1.0, 0.0, -1.0};
    c = cq[q]; s = sq[q];
    return;
  }
  const double ang = 3.14159265358979323846 * (double)num / (double)den;
  c = cos(ang); s = sin(ang);
}
int launch_tconv(bool first, const TconvArgs& a_in, hipStream_t stream) {
  TconvArgs a = a_in;
  for (int m = 0; m < MMAX; ++m)
    for (int t = 0; t < TMAX; ++t) {
      double c = 0.0, sn = 0.0;
      if (m < a.M && t < a.T) cos_sin_pi(2 * m * t, a.T, c, sn);
      a.tw_cos[m * TMAX + t] = (float)c;
      a.tw_sin[m * TMAX + t] = (float)sn;
    }
  const int ntiles = (a.BN + 15) / 16;
  a.xcd = xcd_on() && ntiles >= 64;
  a.xw = ntiles < num_cus() && !getenv_int("NONODE_TC_NOXW");
  const int grid = a.xcd ? 8 * ((ntiles + 7) / 8) : ntiles;
  ProfScope prof(first ? 3 : 2, stream);
  auto go = [&](auto kt, auto kf) {
    const int threads = a.xw ? TC_THREADS : 256;
    if (first) hipLaunchKernelGGL(kt, dim3(grid), dim3(threads), 0, stream, a);
    else hipLaunchKernelGGL(kf, dim3(grid), dim3(threads), 0, stream, a);
  };
  if (a.T <= 10) {
    if (a.M <= 2) go(tconv_kernel<true, 2, 10>, tconv_kernel<false, 2, 10>);
    else if (a.M <= 4) go(tconv_kernel<true, 4, 10>, tconv_kernel<false, 4, 10>);
    else go(tconv_kernel<true, MMAX, 10>, tconv_kernel<false, MMAX, 10>);
  } else {
    if (a.M <= 2) go(tconv_kernel<true, 2, TMAX>, tconv_kernel<false, 2, TMAX>);
    else if (a.M <= 4) go(tconv_kernel<true, 4, TMAX>, tconv_kernel<false, 4, TMAX>);
    else go(tconv_kernel<true, MMAX, TMAX>, tconv_kernel<false, MMAX, TMAX>);
  }
  return check_launch("tconv_kernel");
}

int effective_modes(int T, int modes) {
  const int half = T / 2 + 1;
  return modes < half ? modes : half;
}

}  // namespace

// ================================ C ABI ========================================================
namespace {
// the validated PackArgs of one layer (nonode_pack_layer's rules)
int pack_args(const nonode_layer_weights* w, int variant, int hidden, int n_edge_feat, float* blob, PackArgs* out) {
  if (!w || !blob) return fail(NONODE_EINVAL, "pack_layer: null pointer");
  const int flags = variant & ~0xff;
  variant &= 0xff;
  if (flags & ~(NONODE_LAYER_NORM_RADIAL | NONODE_LAYER_TANH_COORD))
    return fail(NONODE_EINVAL, "pack_layer: unknown option bits 0x%x", flags);
  if (hidden != HID) return fail(NONODE_EUNSUPPORTED, "pack_layer: hidden=%d (only 64)", hidden);
  if (n_edge_feat < 0 || n_edge_feat > 4) return fail(NONODE_EUNSUPPORTED, "pack_layer: n_edge_feat=%d", n_edge_feat);
  if (!w->edge_w1 || !w->edge_b1 || !w->edge_w2 || !w->edge_b2 || !w->coord_w1 || !w->coord_b1 ||
      !w->coord_w2 || !w->coord_b2 || !w->node_w1 || !w->node_b1 || !w->node_w2 || !w->node_b2)
    return fail(NONODE_EINVAL, "pack_layer: missing weight pointer");
  if ((flags & NONODE_LAYER_NORM_RADIAL) && variant != NONODE_VARIANT_EGNO)
    return fail(NONODE_EINVAL, "pack_layer: NORM_RADIAL is an EGNO option");
  if ((flags & NONODE_LAYER_TANH_COORD) && variant != NONODE_VARIANT_SEGNO)
    return fail(NONODE_EINVAL, "pack_layer: TANH_COORD is a SEGNO option");
  if (variant == NONODE_VARIANT_EGNO && (!w->vel_w1 || !w->vel_b1 || !w->vel_w2 || !w->vel_b2))
    return fail(NONODE_EINVAL, "pack_layer: EGNO needs node_v_net weights");
  PackArgs& a = *out;
  a.ld1 = 2 * HID + 1 + n_edge_feat;
  if (variant == NONODE_VARIANT_EGNO) { a.colS = 0; a.colA = 1; a.colB = 1 + HID; }       // [s,h_i,h_j,e]
  else if (variant == NONODE_VARIANT_SEGNO) { a.colA = 0; a.colB = HID; a.colS = 2 * HID; }  // [h_i,h_j,s,e]
  else return fail(NONODE_EINVAL, "pack_layer: variant %d", variant);
  a.w1 = w->edge_w1; a.b1 = w->edge_b1; a.w2 = w->edge_w2; a.b2 = w->edge_b2;
  a.cw1 = w->coord_w1; a.cb1 = w->coord_b1; a.cw2 = w->coord_w2; a.cb2 = w->coord_b2;
  const bool egno = variant == NONODE_VARIANT_EGNO;
  a.vw1 = egno ? w->vel_w1 : nullptr; a.vb1 = egno ? w->vel_b1 : nullptr;
  a.vw2 = egno ? w->vel_w2 : nullptr; a.vb2 = egno ? w->vel_b2 : nullptr;
  a.nw1 = w->node_w1; a.nb1 = w->node_b1; a.nw2 = w->node_w2; a.nb2 = w->node_b2;
  a.ne = n_edge_feat;
  a.flags = flags;
  a.blob = blob;
  return NONODE_OK;
}
}  // namespace

extern "C" {

size_t nonode_tconv_blob_floats(int modes) { return (modes >= 1 && modes <= MMAX) ? tconv_blob_floats(modes) : 0; }

const char* nonode_version(void) { return "nonode-mi355x 0.1 (gfx950)"; }
const char* nonode_last_error(void) { return g_err.c_str(); }
size_t nonode_layer_blob_floats(void) { return BLOB_FLOATS; }

int nonode_pack_layer(const nonode_layer_weights* w, int variant, int hidden, int n_edge_feat,
                      float* blob, void* stream) {
  return nonode_pack_layers(&w, 1, variant, hidden, n_edge_feat, &blob, stream);
}
int nonode_pack_layers(const nonode_layer_weights* const* w, int n_layers, int variant, int hidden,
                       int n_edge_feat, float* const* blobs, void* stream) {
  if (!w || !blobs || n_layers < 0) return fail(NONODE_EINVAL, "pack_layers: null pointer");
  // every layer is validated before the first launch: a bad entry leaves every blob untouched
  std::vector<PackArgs> args(n_layers);
  for (int l = 0; l < n_layers; ++l)
    if (int rc = pack_args(w[l], variant, hidden, n_edge_feat, blobs[l], &args[l])) return rc;
  for (int l0 = 0; l0 < n_layers; l0 += PACK_MAX) {
    const int cnt = n_layers - l0 < PACK_MAX ? n_layers - l0 : PACK_MAX;
    PackBatch pb{};
    for (int k = 0; k < cnt; ++k) pb.a[k] = args[l0 + k];
    hipLaunchKernelGGL(pack_kernel, dim3(32, 16, cnt), dim3(256), 0, (hipStream_t)stream, pb);
    if (int rc = check_launch("pack_kernel")) return rc;
  }
  return NONODE_OK;
}
int nonode_pack_tconv(const float* tconv_w, int modes, int T, float* blob, void* stream) {
  return nonode_pack_tconvs(&tconv_w, 1, modes, T, &blob, stream);
}
int nonode_pack_tconvs(const float* const* tconv_w, int n_layers, int modes, int T, float* const* blobs,
                       void* stream) {
  if (!tconv_w || !blobs || n_layers < 0) return fail(NONODE_EINVAL, "pack_tconv: null pointer");
  if (modes < 1 || modes > MMAX || T < 1 || T > TMAX)
    return fail(NONODE_EUNSUPPORTED, "pack_tconv: modes=%d T=%d", modes, T);
  const int M = effective_modes(T, modes);
  const int n = tconv_mats(M) * 4096;   // the f32 fragments (tconv_pack_kernel)
  for (int l = 0; l < n_layers; ++l)   // validated before the first launch
    if (!tconv_w[l] || !blobs[l]) return fail(NONODE_EINVAL, "pack_tconv: null pointer");
  for (int l0 = 0; l0 < n_layers; l0 += PACK_MAX) {
    const int cnt = n_layers - l0 < PACK_MAX ? n_layers - l0 : PACK_MAX;
    TconvPackBatch tb{};
    for (int k = 0; k < cnt; ++k) {
      tb.w[k] = tconv_w[l0 + k];
      tb.out[k] = blobs[l0 + k];
    }
    hipLaunchKernelGGL(tconv_pack_kernel, dim3((n + 255) / 256, cnt), dim3(256), 0, (hipStream_t)stream, tb, modes,
                       M, T);
    if (int rc = check_launch("tconv_pack_kernel")) return rc;
    hipLaunchKernelGGL(tconv_pack_h16_kernel, dim3(tconv_mats(M), cnt), dim3(256), 0, (hipStream_t)stream, tb, M);
    if (int rc = check_launch("tconv_pack_h16_kernel")) return rc;
  }
  return NONODE_OK;
}

int nonode_egno_tconv(int BN, int T, int modes, const float* h, const float* x, const float* v,
                      const float* loc_mean, const float* tconv_blob, const float* tconvx_w,
                      float* h_out, float* x_out, float* v_out, void* stream) {
  if (BN <= 0 || T <= 0 || T > TMAX || modes <= 0 || modes > MMAX)
    return fail(NONODE_EUNSUPPORTED, "tconv: BN=%d T=%d modes=%d (T<=%d, modes<=%d)", BN, T, modes, TMAX, MMAX);
  if (!h || !x || !v || !loc_mean || !tconv_blob || !tconvx_w || !h_out || !x_out || !v_out)
    return fail(NONODE_EINVAL, "tconv: null pointer");
  if (h_out == h) return fail(NONODE_EINVAL, "tconv: h_out may not alias h");
  TconvArgs a{};
  a.BN = BN; a.T = T; a.M = effective_modes(T, modes); a.Mfull = modes;
  a.h = h; a.x = x; a.v = v; a.lm = loc_mean; a.wp = tconv_blob; a.wx = tconvx_w;
  a.h_out = h_out; a.x_out = x_out; a.v_out = v_out;
  return launch_tconv(false, a, (hipStream_t)stream);
}

int nonode_egnn_layer(int variant, int n_graphs, int N, int n_edge_feat, int ef_mod,
                      const float* h, const float* x, const float* v, const float* edge_fea,
                      const float* blob, float dt, float coords_weight, int recurrent,
                      float* h_out, float* x_out, float* v_out, void* stream) {
  if (n_graphs <= 0 || N < 2 || ef_mod <= 0 || n_edge_feat < 0 || n_edge_feat > 4)
    return fail(NONODE_EUNSUPPORTED, "egnn_layer: n_graphs=%d N=%d ef_mod=%d ne=%d", n_graphs, N, ef_mod, n_edge_feat);
  if (!h || !x || !v || !blob || !h_out || !x_out || (n_edge_feat > 0 && !edge_fea))
    return fail(NONODE_EINVAL, "egnn_layer: null pointer");
  if (h_out == h || x_out == x) return fail(NONODE_EINVAL, "egnn_layer: outputs may not alias inputs");
  if (variant == NONODE_VARIANT_EGNO)
    return launch_layer<EGNO>(n_graphs, N, n_edge_feat, ef_mod, h, x, v, edge_fea, blob, dt, coords_weight,
                              recurrent, h_out, x_out, v_out, (hipStream_t)stream);
  if (variant == NONODE_VARIANT_SEGNO) {
    if (!v_out || v_out == v) return fail(NONODE_EINVAL, "egnn_layer: SEGNO needs a distinct v_out");
    return launch_layer<SEGNO>(n_graphs, N, n_edge_feat, ef_mod, h, x, v, edge_fea, blob, dt, coords_weight,
                               recurrent, h_out, x_out, v_out, (hipStream_t)stream);
  }
  return fail(NONODE_EINVAL, "egnn_layer: variant %d", variant);
}

size_t nonode_egno_workspace_bytes(int B, int N, int T, int Bt) {
  const size_t n = (size_t)B * N * T;
  return (n * 64 + n * 3 + (size_t)Bt * T * 64 + 64) * sizeof(float);
}
// the flat layer's part starts at the common part rounded up to 256 bytes (its P, Q, M, F rows are
// read and written as 16-byte vectors; (67n + 64 Bt T + 64) floats is only 8-byte aligned for n = 2 mod 4)
static size_t flat_ws_offset(int B, int N, int T, int Bt) {
  return (nonode_egno_workspace_bytes(B, N, T, Bt) + 255) & ~(size_t)255;
}
size_t nonode_egno_flat_workspace_bytes(int B, int N, int T, int Bt) {
  return flat_ws_offset(B, N, T, Bt) + (size_t)B * N * T * 580 * sizeof(float);
}

}  // extern "C"

namespace {
// nonode_egno_forward / nonode_egno_forward_frames: frames = 1 takes per-frame x, h, v, loc_mean and
// edge_fea (and t_in for the input-time embedding), frames = 0 the single input replicated over T
// nonode_flat.hip (included at the end of this unit): one EGNN layer with flat=True
int launch_flat_layer(int n_graphs, int N, int ne, int ef_mod, const float* h, const float* x, const float* v,
                      const float* ef, const float* blob, float* h_out, float* x_out, float* ws, hipStream_t s);
// The model's sequence after an entry's own validation, on BN node columns (egno.py:84-107): the
// time-embedding table, then per layer TimeConv and layer(l, h_in, x_in, h_out, x_out) -> status. The
// workspace starts with h | x | embedding table (nonode_egno_workspace_bytes).
template <typename Layer>
int egno_forward_seq(int frames, int BN, int T, int n_layers, int in_node, int time_emb_dim, int modes, int Bt,
                     const float* x, const float* h, const float* v, const float* loc_mean, const float* t_in,
                     const float* t_out, const float* emb_w, const float* emb_b, const float* const* tconv_blobs,
                     const float* const* tconvx_w, float* x_out, float* v_out, float* h_out, void* workspace,
                     hipStream_t s, Layer layer) {
  const size_t n = (size_t)BN * T;
  float* hB = (float*)workspace;
  float* xB = hB + n * 64;
  float* etab = xB + n * 3;
  const int emb_ld = in_node + (t_in ? 2 : 1) * time_emb_dim;
  hipLaunchKernelGGL(temb_kernel, dim3((Bt * T + TEMB_ROWS - 1) / TEMB_ROWS), dim3(256), 0, s, Bt, T, in_node, time_emb_dim,
                     t_out, emb_w, emb_ld, emb_b, etab, t_in);
  if (int rc = check_launch("temb_kernel")) return rc;
  if (!tconv_blobs) {
    // layer l reads buffer (L - l) & 1 and writes (L - 1 - l) & 1 of {h_out | x_out, hB | xB}, so the
    // last layer writes h_out, x_out; v (unchanged by EGNN_Layer, basic.py:186) is replicated once
    float* hb[2] = {h_out, hB};
    float* xb[2] = {x_out, xB};
    const int L = n_layers;
    hipLaunchKernelGGL(h0_kernel, dim3((BN * 64 + 255) / 256), dim3(256), 0, s, BN, T, in_node, Bt, h, emb_w, emb_ld,
                       etab, x, v, hb[L & 1], xb[L & 1], v_out, frames);
    if (int rc = check_launch("h0_kernel")) return rc;
    for (int l = 0; l < L; ++l) {
      const int i = (L - l) & 1, o = (L - 1 - l) & 1;
      if (int rc = layer(l, hb[i], xb[i], hb[o], xb[o])) return rc;
    }
    return NONODE_OK;
  }
  for (int l = 0; l < n_layers; ++l) {
    TconvArgs a{};
    a.BN = BN; a.T = T; a.M = effective_modes(T, modes); a.Mfull = modes;
    a.wp = tconv_blobs[l]; a.wx = tconvx_w[l]; a.frames = frames;
    a.h_out = hB; a.x_out = xB; a.v_out = v_out;
    if (l == 0) {
      a.h = nullptr; a.x = x; a.v = v; a.lm = loc_mean;
      a.hin = h; a.din = in_node; a.emb_w = emb_w; a.emb_ld = emb_ld; a.etab = etab; a.Bt = Bt;
    } else {
      a.h = h_out; a.x = x_out; a.v = v_out; a.lm = loc_mean;
    }
    if (int rc = launch_tconv(l == 0, a, s)) return rc;
    if (int rc = layer(l, hB, xB, h_out, x_out)) return rc;
  }
  return NONODE_OK;
}
// flat: the blobs are flat-layer blobs (nonode_pack_layer_flat), the workspace has the flat layer's
// n x 580 floats after the common part (nonode_egno_flat_workspace_bytes)
int egno_forward_impl(int frames, int flat, int B, int N, int T, int n_layers, int in_node, int n_edge_feat,
                        int time_emb_dim, int modes, int Bt,
                        const float* x, const float* h, const float* v, const float* loc_mean,
                        const float* edge_fea, const float* t_in, const float* t_out,
                        const float* emb_w, const float* emb_b,
                        const float* const* blobs, const float* const* tconv_blobs,
                        const float* const* tconvx_w,
                        float* x_out, float* v_out, float* h_out,
                        void* workspace, size_t workspace_bytes, void* stream) {
  if (B <= 0 || N < 2 || T <= 0 || T > TMAX || n_layers < 1 || in_node < 0 || in_node > 8 ||
      modes < 1 || modes > MMAX || time_emb_dim < 4 || time_emb_dim > 64 || (time_emb_dim & 1) ||
      Bt <= 0 || (B * N) % Bt != 0)
    return fail(NONODE_EUNSUPPORTED,
                "egno_forward: B=%d N=%d T=%d layers=%d in_node=%d modes=%d temb=%d Bt=%d", B, N, T,
                n_layers, in_node, modes, time_emb_dim, Bt);
  // use_time_conv=False (egno.py:99-107 skipped): both TimeConv arrays null
  const bool tc = tconv_blobs != nullptr;
  if (!x || !h || !v || (tc && !loc_mean) || !t_out || !emb_w || !emb_b || !blobs || tc != (tconvx_w != nullptr) ||
      !x_out || !v_out || !h_out || !workspace)
    return fail(NONODE_EINVAL, "egno_forward: null pointer");
  const size_t ws_need = flat ? nonode_egno_flat_workspace_bytes(B, N, T, Bt) : nonode_egno_workspace_bytes(B, N, T, Bt);
  if (workspace_bytes < ws_need)
    return fail(NONODE_EINVAL, "egno_forward: workspace %zu < %zu", workspace_bytes, ws_need);
  hipStream_t s = (hipStream_t)stream;
  const int BN = B * N;
  float* flat_ws = (float*)((char*)workspace + flat_ws_offset(B, N, T, Bt));
  auto layer = [&](int l, const float* hi, const float* xi, float* ho, float* xo) {
    if (flat)
      return launch_flat_layer(T * B, N, n_edge_feat, frames ? T * B : B, hi, xi, v_out, edge_fea, blobs[l], ho, xo,
                               flat_ws, s);
    return launch_layer<EGNO>(T * B, N, n_edge_feat, frames ? T * B : B, hi, xi, v_out, edge_fea, blobs[l], 0.f, 1.f,
                              0, ho, xo, nullptr, s, 1, nullptr, nullptr, nullptr, BN);
  };
  return egno_forward_seq(frames, BN, T, n_layers, in_node, time_emb_dim, modes, Bt, x, h, v, loc_mean, t_in, t_out, emb_w,
                          emb_b, tconv_blobs, tconvx_w, x_out, v_out, h_out, workspace, s, layer);
}
// The two SEGNO step entries' prologue: the embedding when no h_in is given (*hc = the h the substeps
// start from) and, for T == 0, the copies that are the whole step (*done)
int segno_step_prologue(size_t n, int T, int in_node, const float* his, const float* h_in, const float* x,
                        const float* v, const float* emb_w, const float* emb_b, float* hemb, float* x_out, float* v_out,
                        float* h_out, hipStream_t s, const float** hc, bool* done) {
  *hc = h_in;
  *done = T == 0;
  if (!h_in) {
    hipLaunchKernelGGL(embed_kernel, dim3((unsigned)((n * 64 + 255) / 256)), dim3(256), 0, s, (int)n, in_node,
                       his, emb_w, emb_b, hemb);
    if (int rc = check_launch("embed_kernel")) return rc;
    *hc = hemb;
  }
  if (T == 0) {
    hipMemcpyAsync(h_out, *hc, n * 64 * sizeof(float), hipMemcpyDeviceToDevice, s);
    hipMemcpyAsync(x_out, x, n * 3 * sizeof(float), hipMemcpyDeviceToDevice, s);
    hipMemcpyAsync(v_out, v, n * 3 * sizeof(float), hipMemcpyDeviceToDevice, s);
    return check_launch("segno T=0 copy");
  }
  return NONODE_OK;
}
}  // namespace

extern "C" {

int nonode_egno_forward(int B, int N, int T, int n_layers, int in_node, int n_edge_feat,
                        int time_emb_dim, int modes, int Bt,
                        const float* x, const float* h, const float* v, const float* loc_mean,
                        const float* edge_fea, const float* t_out,
                        const float* emb_w, const float* emb_b,
                        const float* const* blobs, const float* const* tconv_blobs,
                        const float* const* tconvx_w,
                        float* x_out, float* v_out, float* h_out,
                        void* workspace, size_t workspace_bytes, void* stream) {
  return egno_forward_impl(0, 0, B, N, T, n_layers, in_node, n_edge_feat, time_emb_dim, modes, Bt, x, h, v, loc_mean,
                           edge_fea, nullptr, t_out, emb_w, emb_b, blobs, tconv_blobs, tconvx_w, x_out, v_out, h_out,
                           workspace, workspace_bytes, stream);
}

int nonode_egno_forward_flat(int B, int N, int T, int n_layers, int in_node, int n_edge_feat,
                             int time_emb_dim, int modes, int Bt,
                             const float* x, const float* h, const float* v, const float* loc_mean,
                             const float* edge_fea, const float* t_in, const float* t_out,
                             const float* emb_w, const float* emb_b,
                             const float* const* blobs, const float* const* tconv_blobs,
                             const float* const* tconvx_w,
                             float* x_out, float* v_out, float* h_out,
                             void* workspace, size_t workspace_bytes, void* stream) {
  return egno_forward_impl(t_in ? 1 : 0, 1, B, N, T, n_layers, in_node, n_edge_feat, time_emb_dim, modes, Bt, x, h, v,
                           loc_mean, edge_fea, t_in, t_out, emb_w, emb_b, blobs, tconv_blobs, tconvx_w, x_out, v_out,
                           h_out, workspace, workspace_bytes, stream);
}

int nonode_egno_forward_frames(int B, int N, int T, int n_layers, int in_node, int n_edge_feat,
                               int time_emb_dim, int modes, int Bt,
                               const float* x, const float* h, const float* v, const float* loc_mean,
                               const float* edge_fea, const float* t_in, const float* t_out,
                               const float* emb_w, const float* emb_b,
                               const float* const* blobs, const float* const* tconv_blobs,
                               const float* const* tconvx_w,
                               float* x_out, float* v_out, float* h_out,
                               void* workspace, size_t workspace_bytes, void* stream) {
  return egno_forward_impl(1, 0, B, N, T, n_layers, in_node, n_edge_feat, time_emb_dim, modes, Bt, x, h, v, loc_mean,
                           edge_fea, t_in, t_out, emb_w, emb_b, blobs, tconv_blobs, tconvx_w, x_out, v_out, h_out,
                           workspace, workspace_bytes, stream);
}

size_t nonode_segno_workspace_bytes(int B, int N) {
  const size_t n = (size_t)B * N;
  return (3 * n * 64 + 4 * n * 3 + 64) * sizeof(float);   // embedding | h ping-pong | x, v ping-pong
}

int nonode_segno_forward_step(int B, int N, int T, int in_node, int n_edge_feat,
                              const float* his, const float* h_in, const float* x, const float* v,
                              const float* edge_attr, const float* emb_w, const float* emb_b,
                              const float* blob, float coords_weight, int recurrent,
                              float* x_out, float* v_out, float* h_out,
                              void* workspace, size_t workspace_bytes, void* stream) {
  if (B <= 0 || N < 2 || T < 0 || in_node < 0 || in_node > 8 || n_edge_feat < 0 || n_edge_feat > 4)
    return fail(NONODE_EUNSUPPORTED, "segno_forward_step: B=%d N=%d T=%d in_node=%d ne=%d", B, N, T, in_node,
                n_edge_feat);
  if (!x || !v || !blob || !x_out || !v_out || !h_out || !workspace || (!h_in && (!his || !emb_w || !emb_b)))
    return fail(NONODE_EINVAL, "segno_forward_step: null pointer");
  if (workspace_bytes < nonode_segno_workspace_bytes(B, N))
    return fail(NONODE_EINVAL, "segno_forward_step: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)B * N;
  float* hemb = (float*)workspace;
  float* pp[6] = {hemb + n * 64, hemb + 2 * n * 64, hemb + 3 * n * 64, hemb + 3 * n * 64 + n * 3,
                  hemb + 3 * n * 64 + 2 * n * 3, hemb + 3 * n * 64 + 3 * n * 3};
  const float* hc;
  bool done;
  if (int rc = segno_step_prologue(n, T, in_node, his, h_in, x, v, emb_w, emb_b, hemb, x_out, v_out, h_out, s, &hc, &done))
    return rc;
  if (done) return NONODE_OK;
  // all T substeps in one launch: each workgroup owns whole samples, so substep t+1 only needs
  // its own workgroup's substep-t results (model.py:95-102, gcl.py:111-119)
  return launch_layer<SEGNO>(B, N, n_edge_feat, B, hc, x, v, edge_attr, blob, 1.0f / (float)T, coords_weight,
                             recurrent, h_out, x_out, v_out, s, T, pp);
}

// ---- whole models on an explicit edge list (host glue; the layer kernels live in nonode_graph.hip) ----
static size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

size_t nonode_egno_graph_workspace_bytes(int n_nodes, int T, int Bt) {
  if (n_nodes <= 0 || T <= 0 || Bt <= 0) return 0;
  return align256(nonode_egno_workspace_bytes(1, n_nodes, T, Bt)) +
         nonode_tu::graph_layer_ws_floats((long long)n_nodes * T) * sizeof(float);
}

int nonode_egno_forward_graph(int n_nodes, long long E, int T, int n_layers, int in_node, int n_edge_feat,
                              int time_emb_dim, int modes, int Bt, const float* x, const float* h, const float* v,
                              const float* loc_mean, const float* edge_fea, const float* t_in, const float* t_out,
                              const float* emb_w, const float* emb_b, const float* const* blobs,
                              const float* const* tconv_blobs, const float* const* tconvx_w, const int* row_ptr,
                              const int* col, const int* eid, float* x_out, float* v_out, float* h_out,
                              void* workspace, size_t workspace_bytes, void* stream) {
  if (n_nodes <= 0 || E < 0 || T <= 0 || T > TMAX || n_layers < 1 || in_node < 0 || in_node > 8 || modes < 1 ||
      modes > MMAX || time_emb_dim < 4 || time_emb_dim > 64 || (time_emb_dim & 1) || Bt <= 0 || n_nodes % Bt != 0 ||
      n_edge_feat < 0 || n_edge_feat > 4)
    return fail(NONODE_EUNSUPPORTED, "egno_forward_graph: n_nodes=%d E=%lld T=%d layers=%d in_node=%d modes=%d temb=%d Bt=%d",
                n_nodes, E, T, n_layers, in_node, modes, time_emb_dim, Bt);
  const bool tc = tconv_blobs != nullptr;
  if (!x || !h || !v || (tc && !loc_mean) || !t_out || !emb_w || !emb_b || !blobs || tc != (tconvx_w != nullptr) ||
      !row_ptr || (E > 0 && (!col || !eid || (n_edge_feat > 0 && !edge_fea))) || !x_out || !v_out || !h_out || !workspace)
    return fail(NONODE_EINVAL, "egno_forward_graph: null pointer");
  if (workspace_bytes < nonode_egno_graph_workspace_bytes(n_nodes, T, Bt))
    return fail(NONODE_EINVAL, "egno_forward_graph: workspace %zu < %zu", workspace_bytes,
                nonode_egno_graph_workspace_bytes(n_nodes, T, Bt));
  hipStream_t s = (hipStream_t)stream;
  const int frames = t_in ? 1 : 0;
  float* lws = (float*)((char*)workspace + align256(nonode_egno_workspace_bytes(1, n_nodes, T, Bt)));
  // frame f owns node rows f n_nodes .. and shares the one CSR (egno.py:84-96); v is unchanged by the layer
  auto layer = [&](int l, const float* hi, const float* xi, float* ho, float* xo) {
    return nonode_tu::graph_layer(NONODE_VARIANT_EGNO, T, n_nodes, E, n_edge_feat, frames ? T : 1, hi, xi, v_out,
                                  edge_fea, blobs[l], row_ptr, col, eid, 0.f, 1.f, 0, ho, xo, nullptr, lws, s);
  };
  return egno_forward_seq(frames, n_nodes, T, n_layers, in_node, time_emb_dim, modes, Bt, x, h, v, loc_mean, t_in, t_out,
                          emb_w, emb_b, tconv_blobs, tconvx_w, x_out, v_out, h_out, workspace, s, layer);
}

size_t nonode_segno_graph_workspace_bytes(int n_nodes) {
  if (n_nodes <= 0) return 0;
  return align256(nonode_segno_workspace_bytes(1, n_nodes)) + nonode_tu::graph_layer_ws_floats(n_nodes) * sizeof(float);
}

int nonode_segno_forward_step_graph(int n_nodes, long long E, int T, int in_node, int n_edge_feat, const float* his,
                                    const float* h_in, const float* x, const float* v, const float* edge_attr,
                                    const float* emb_w, const float* emb_b, const float* blob, const int* row_ptr,
                                    const int* col, const int* eid, float coords_weight, int recurrent, float* x_out,
                                    float* v_out, float* h_out, void* workspace, size_t workspace_bytes, void* stream) {
  if (n_nodes <= 0 || E < 0 || T < 0 || in_node < 0 || in_node > 8 || n_edge_feat < 0 || n_edge_feat > 4)
    return fail(NONODE_EUNSUPPORTED, "segno_forward_step_graph: n_nodes=%d E=%lld T=%d in_node=%d ne=%d", n_nodes, E, T,
                in_node, n_edge_feat);
  if (!x || !v || !blob || !row_ptr || (E > 0 && (!col || !eid || (n_edge_feat > 0 && !edge_attr))) || !x_out ||
      !v_out || !h_out || !workspace || (!h_in && (!his || !emb_w || !emb_b)))
    return fail(NONODE_EINVAL, "segno_forward_step_graph: null pointer");
  if (workspace_bytes < nonode_segno_graph_workspace_bytes(n_nodes))
    return fail(NONODE_EINVAL, "segno_forward_step_graph: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)n_nodes;
  float* hemb = (float*)workspace;
  float* pph[2] = {hemb + n * 64, hemb + 2 * n * 64};
  float* ppx[2] = {hemb + 3 * n * 64, hemb + 3 * n * 64 + n * 3};
  float* ppv[2] = {hemb + 3 * n * 64 + 2 * n * 3, hemb + 3 * n * 64 + 3 * n * 3};
  float* lws = (float*)((char*)workspace + align256(nonode_segno_workspace_bytes(1, n_nodes)));
  const float* hc;
  bool done;
  if (int rc = segno_step_prologue(n, T, in_node, his, h_in, x, v, emb_w, emb_b, hemb, x_out, v_out, h_out, s, &hc, &done))
    return rc;
  if (done) return NONODE_OK;
  // T substeps of the shared layer with the edge attributes frozen (model.py:95-102), dt = 1/T
  const float* hi = hc; const float* xi = x; const float* vi = v;
  for (int t = 0; t < T; ++t) {
    const bool last = t == T - 1;
    float* ho = last ? h_out : pph[t & 1];
    float* xo = last ? x_out : ppx[t & 1];
    float* vo = last ? v_out : ppv[t & 1];
    if (int rc = nonode_tu::graph_layer(NONODE_VARIANT_SEGNO, 1, n_nodes, E, n_edge_feat, 1, hi, xi, vi, edge_attr, blob,
                                        row_ptr, col, eid, 1.0f / (float)T, coords_weight, recurrent, ho, xo, vo, lws, s))
      return rc;
    hi = ho; xi = xo; vi = vo;
  }
  return NONODE_OK;
}

// state of the SEGNO training forward on an edge list (floats, n = n_nodes; layout in nonode.h)
static size_t segno_graph_state_floats(int n_nodes, int T) { return (size_t)T * (size_t)n_nodes * 266; }

size_t nonode_segno_graph_train_state_bytes(int n_nodes, int T) {
  if (n_nodes <= 0 || T <= 0) return 0;
  return segno_graph_state_floats(n_nodes, T) * sizeof(float);
}

int nonode_segno_forward_train_graph(int n_nodes, long long E, int T, int n_edge_feat, const float* h, const float* x,
                                     const float* v, const float* edge_attr, const float* blob, const int* row_ptr,
                                     const int* col, const int* eid, float coords_weight, int recurrent, float* x_out,
                                     float* v_out, float* h_out, void* state, size_t state_bytes, void* stream) {
  if (n_nodes <= 0 || E < 0 || T < 0 || n_edge_feat < 0 || n_edge_feat > 4 || (long long)n_nodes * (T > 0 ? T : 1) > (1ll << 30))
    return fail(NONODE_EUNSUPPORTED, "segno_forward_train_graph: n_nodes=%d E=%lld T=%d ne=%d", n_nodes, E, T, n_edge_feat);
  if (!h || !x || !v || !blob || !row_ptr || (E > 0 && (!col || !eid || (n_edge_feat > 0 && !edge_attr))) || !x_out ||
      !v_out || !h_out || (T > 0 && !state))
    return fail(NONODE_EINVAL, "segno_forward_train_graph: null pointer");
  if (h_out == h || x_out == x || v_out == v)
    return fail(NONODE_EINVAL, "segno_forward_train_graph: outputs may not alias inputs");
  if (state_bytes < nonode_segno_graph_train_state_bytes(n_nodes, T))
    return fail(NONODE_EINVAL, "segno_forward_train_graph: state too small");
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)n_nodes;
  float* hs = (float*)state;                 // [T][n][64]
  float* ws = hs + (size_t)T * n * 64;       // [T][n * 196]: P | Q | M | F of each substep
  float* xs = ws + (size_t)T * n * 196;      // [T][n][3]
  float* vs = xs + (size_t)T * n * 3;        // [T][n][3]
  float* h0 = T ? hs : h_out; float* x0 = T ? xs : x_out; float* v0 = T ? vs : v_out;   // T = 0: the inputs pass through
  if (hipMemcpyAsync(h0, h, n * 64 * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess ||
      hipMemcpyAsync(x0, x, n * 3 * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess ||
      hipMemcpyAsync(v0, v, n * 3 * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess)
    return fail(NONODE_ELAUNCH, "segno_forward_train_graph: copy");
  // substep t reads its saved inputs and writes substep t + 1's (the last one: the outputs); its layer
  // workspace is the state the reverse reads (model.py:95-102, dt = 1/T)
  for (int t = 0; t < T; ++t) {
    const bool last = t == T - 1;
    if (int rc = nonode_tu::graph_layer(NONODE_VARIANT_SEGNO, 1, n_nodes, E, n_edge_feat, 1, hs + t * n * 64,
                                        xs + t * n * 3, vs + t * n * 3, edge_attr, blob, row_ptr, col, eid,
                                        1.0f / (float)T, coords_weight, recurrent, last ? h_out : hs + (t + 1) * n * 64,
                                        last ? x_out : xs + (t + 1) * n * 3, last ? v_out : vs + (t + 1) * n * 3,
                                        ws + t * n * 196, s))
      return rc;
  }
  return NONODE_OK;
}

int nonode_profile_begin(int max_records) {
  std::lock_guard<std::mutex> lk(g_prof.mu);
  if (max_records <= 0 || max_records > (1 << 20)) return fail(NONODE_EINVAL, "profile_begin: %d", max_records);
  if (g_prof.ev) {
    for (int i = 0; i < 2 * g_prof.cap; ++i) (void)hipEventDestroy(g_prof.ev[i]);
    delete[] g_prof.ev;
    delete[] g_prof.kind;
  }
  g_prof.ev = new hipEvent_t[2 * max_records];
  g_prof.kind = new int[max_records];
  for (int i = 0; i < 2 * max_records; ++i)
    if (hipEventCreate(&g_prof.ev[i]) != hipSuccess) return fail(NONODE_ELAUNCH, "profile_begin: hipEventCreate");
  g_prof.cap = max_records;
  g_prof.n = 0;
  g_prof.on = true;
  return NONODE_OK;
}

int nonode_profile_end(float* ms_out, int* kind_out, int max_out) {
  std::lock_guard<std::mutex> lk(g_prof.mu);
  g_prof.on = false;
  const int n = g_prof.n < max_out ? g_prof.n : max_out;
  for (int i = 0; i < n; ++i) {
    if (hipEventSynchronize(g_prof.ev[2 * i + 1]) != hipSuccess) return -fail(NONODE_ELAUNCH, "profile_end: sync");
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, g_prof.ev[2 * i], g_prof.ev[2 * i + 1]);
    if (ms_out) ms_out[i] = ms;
    if (kind_out) kind_out[i] = g_prof.kind[i];
  }
  g_prof.n = 0;
  return n;
}

// Diagnostic (host only, no GPU; not part of the C ABI in nonode.h): the four-wave layer kernel's split of
// a chunk's edge units and each wave's walk, from the very functions the kernel runs (unit_split,
// seg_walk). The chunk has ctc tiles of Nm1 units, the last one Ul units with packed limit Ql.
// cut[5]: wave w takes units [cut[w], cut[w + 1]). rows: per tile segment of a wave, in order,
// {wave, tile, k_lo, k_hi, triples, pairs, singles, regular units} (8 ints; at most max_rows segments
// are written). Returns the number of segments, or -1 for arguments the kernel never sees.
int nonode_debug_edge_walk(int variant, int ctc, int Nm1, int Ul, int Ql, int* cut, int* rows, int max_rows) {
  if ((variant != NONODE_VARIANT_EGNO && variant != NONODE_VARIANT_SEGNO) || ctc < 1 || ctc > 8 || Nm1 < 1 ||
      Ul < 1 || Ul > Nm1 || Ql < 0 || Ql > Ul || !cut)
    return -1;
  const bool egno = variant == NONODE_VARIANT_EGNO;
  if (egno) unit_split<4, NONODE_TRICOST != 0>(ctc, Nm1, Ul, Ql, cut);
  else unit_split<4, false>(ctc, Nm1, Ul, Ql, cut);
  int n = 0;
  for (int wave = 0; wave < 4; ++wave) {
    int u = cut[wave];
    const int u1 = cut[wave + 1];
    while (u < u1) {   // the kernel's segment loop
      const int tau = imin(u / Nm1, ctc - 1);
      const int k_lo = u - tau * Nm1 + 1;
      const int k_hi = imin(tau == ctc - 1 ? Ul : Nm1, k_lo + (u1 - u) - 1);
      u += k_hi - k_lo + 1;
      const int kp_hi = imin(k_hi, tau == ctc - 1 ? Ql : Nm1);
      const int lp = imax(kp_hi - k_lo + 1, 0);
      const SegWalk w = egno ? seg_walk<true>(lp) : seg_walk<false>(lp);
      if (rows && n < max_rows) {
        const int row[8] = {wave, tau, k_lo, k_hi, w.tri, w.pair, w.one, k_hi - k_lo + 1 - lp};
        memcpy(rows + 8 * n, row, sizeof(row));
      }
      ++n;
    }
  }
  return n;
}

// the build's edge-walk switches: bit 0 NONODE_WALK2, 1 NONODE_TRICOST, 2 NONODE_FSPLIT, 3 NONODE_HOSTCUT
int nonode_debug_edge_switches(void) {
  return (NONODE_WALK2 ? 1 : 0) | (NONODE_TRICOST ? 2 : 0) | (NONODE_FSPLIT ? 4 : 0) | (NONODE_HOSTCUT ? 8 : 0);
}

// the build's tile-segment boundary levers: bit 0 NONODE_PREB, 1 NONODE_UCUT
int nonode_debug_boundary_switches(void) {
  return (NONODE_PREB ? 1 : 0) | (NONODE_UCUT ? 2 : 0);
}

#if NONODE_STAMP
// diagnostic builds only: read and clear the accumulated per-section wave cycles (NONODE_NSTAMP = 24 slots)
int nonode_debug_stamps(unsigned long long* out24) {
  if (hipDeviceSynchronize() != hipSuccess) return fail(NONODE_ELAUNCH, "stamps: sync");
  if (hipMemcpyFromSymbol(out24, HIP_SYMBOL(g_stamp), NONODE_NSTAMP * sizeof(unsigned long long)) != hipSuccess)
    return fail(NONODE_ELAUNCH, "stamps: copy");
  unsigned long long z[NONODE_NSTAMP] = {};
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_stamp), z, sizeof(z)) != hipSuccess) return fail(NONODE_ELAUNCH, "stamps: clear");
  return NONODE_OK;
}
#endif

}  // extern "C"

// training path (forward with saved state + backward), same translation unit
#include "nonode_train.hip"
#include "nonode_rollout.hip"
#include "nonode_sim.hip"
#include "nonode_data.hip"
#include "nonode_flat.hip"
