// nonode_graph_common.h — the general-graph layer's forward arithmetic, defined once for
// nonode_graph.hip (inference) and nonode_graph_train.hip (whose reverse kernels recompute it): the
// frame / tile indexing, the CSR row walk, the LDS staging of the forward blob's edge phase, the edge
// step and the node step's pre-activations. Included by those two units only.
#pragma once
#include "nonode_bwd_common.h"

namespace {

// ---- tiles -----------------------------------------------------------------------------------------
// One wave per 16 nodes of one frame. A launch covers frames f0 .. f0 + nf - 1 (the forward: all of
// them, f0 = 0); frame f owns node rows f n_nodes .., and a tile never straddles a frame.
struct Tile {
  int fr, fa, nc;   // frame relative to the launch / absolute, node (clamped to the frame)
  bool rvalid;
  size_t fbase, r, rr;   // first row of the frame, this node's row / its row relative to the launch
};
__device__ __forceinline__ bool tile_of(int n_nodes, int f0, int nf, int e, int wave, Tile& t) {
  const int tpf = (n_nodes + 15) >> 4;
  const int w = blockIdx.x * 4 + wave;
  t.fr = w / tpf;
  if (t.fr >= nf) return false;
  const int n = (w - t.fr * tpf) * 16 + e;
  t.rvalid = n < n_nodes;
  t.nc = t.rvalid ? n : n_nodes - 1;
  t.fa = f0 + t.fr;
  t.fbase = (size_t)t.fa * n_nodes;
  t.r = t.fbase + t.nc;
  t.rr = (size_t)t.fr * n_nodes + t.nc;
  return true;
}

// ---- CSR row walk ----------------------------------------------------------------------------------
// Column e of the wave walks row nc of a CSR; step k pairs it with the row's k-th entry, up to the
// tile's largest degree kmax (wave-uniform). A column past its own degree is masked by the caller
// (k < deg) and re-reads its first entry (a row without entries: node nc itself and edge 0), so a
// masked lane computes on finite, in-range data.
struct CsrRow {
  int rp, deg, kmax;
  __device__ __forceinline__ CsrRow(const int* row_ptr, int nc, bool rvalid) {
    rp = row_ptr[nc];
    deg = rvalid ? row_ptr[nc + 1] - rp : 0;
    kmax = deg;
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) kmax = max(kmax, __shfl_xor(kmax, o));
    kmax = __builtin_amdgcn_readfirstlane(kmax);
  }
  // the k-th entry's other endpoint and original edge index (call it for k + 1 before step k's
  // gathers: the indices stay a step ahead)
  __device__ __forceinline__ void entry(const int* col, const int* eid, int nc, int k, int& j, int& id) const {
    if (deg > 0) {
      const int idx = rp + (k < deg ? k : 0);
      j = col[idx];
      id = eid[idx];
    } else {
      j = nc;
      id = 0;
    }
  }
  // the edge index alone
  __device__ __forceinline__ int edge(const int* eid, int k) const { return deg > 0 ? eid[rp + (k < deg ? k : 0)] : 0; }
};

// ---- edge phase ------------------------------------------------------------------------------------
// W2 | Wc1 fp16 hi/lo fragments (8192 floats at sW) and the edge-phase vectors FEAT | b2 | bc1 | wc2
// (EDGE_STAGE_FLOATS at sV) of the forward blob, staged by a 256-thread workgroup; the caller
// synchronises before edge_weights()
__device__ __forceinline__ void stage_edge_weights(float* sW, float* sV, const float* blob, int tid) {
  for (int i = tid; i < 2048; i += 256) reinterpret_cast<f4*>(sW)[i] = reinterpret_cast<const f4*>(blob + OFF_H16)[i];
  if (tid < EDGE_STAGE_FLOATS / 4) reinterpret_cast<f4*>(sV)[tid] = reinterpret_cast<const f4*>(blob + OFF_FEAT)[tid];
}
struct EdgeWeights {
  const h8* w2h; const h8* wc1h;
  const float* vFEAT; const float* vB2; const float* vBC1; const float* vWC2;
  const float* blob;
  float bc2;
  bool rnorm, ctanh;
  unsigned us_w2, us_wc1;
};
__device__ __forceinline__ EdgeWeights edge_weights(const float* sW, const float* sV, const float* blob) {
  EdgeWeights w;
  w.vFEAT = sV;
  w.vB2 = sV + 512 + V_B2 * 64;
  w.vBC1 = sV + 512 + V_BC1 * 64;
  w.vWC2 = sV + 512 + V_WC2 * 64;
  w.w2h = reinterpret_cast<const h8*>(sW);
  w.wc1h = reinterpret_cast<const h8*>(sW + 4096);
  w.blob = blob;
  const float* scal = blob + OFF_SCAL;
  w.bc2 = scal[0];
  w.rnorm = scal[SC_NORM] != 0.f;
  w.ctanh = scal[SC_TANH] != 0.f;
  w.us_w2 = h16_us(scal, HS_W2);
  w.us_wc1 = h16_us(scal, HS_WC1);
  return w;
}

// what the edge step reads of the layer, and of its receiver (column e of the wave)
struct EdgeInputs {
  const float* x; const float* Q; const float* efb;   // efb: the frame's edge features [E][ne]
  int ne;
  f4 pr[4];             // the receiver's P row
  float xr0, xr1, xr2;  // its position
};
// what one edge step computes: the three activations (log2 domain), r = x_r - x_s, |r|^2 raw and as the
// radial input, the coordinate scalar
struct EdgeStep {
  f4 a[4], m[4], c1[4];
  float r0, r1, r2, d2raw, d2, c;
};
// The forward of one edge step (basic.py:170-173): sender row s, edge id. act(z, i) applies SiLU in
// place to pre-activation i = 0, 1, 2 (the reverse pass keeps SiLU' there).
template <int KF, typename Act>
__device__ __forceinline__ void edge_step(const EdgeWeights& w, const EdgeInputs& in, size_t s, int id, int lane, int g,
                                          Act& act, EdgeStep& o) {
  o.r0 = in.xr0 - in.x[s * 3 + 0];
  o.r1 = in.xr1 - in.x[s * 3 + 1];
  o.r2 = in.xr2 - in.x[s * 3 + 2];
  o.d2raw = fmaf(o.r0, o.r0, fmaf(o.r1, o.r1, o.r2 * o.r2));
  o.d2 = w.rnorm ? radial_norm(o.d2raw) : o.d2raw;
  // pre-activation P_r + Q_s + W1[:, scalars] [|r|^2, e_rs]: the scalar inputs as f32 MFMA k-steps
  load_ecl(o.a, in.Q + s * HID, g);
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) o.a[mt] += in.pr[mt];
#pragma unroll
  for (int kf = 0; kf < KF; ++kf) {
    const int fi = 4 * kf + g;
    float bv = 0.f;
    if (fi == 0) bv = o.d2;
    else if (fi - 1 < in.ne) bv = in.efb[(size_t)id * in.ne + (fi - 1)];
    const f4 wf = *reinterpret_cast<const f4*>(w.vFEAT + kf * 256 + lane * 4);
#pragma unroll
    for (int mo = 0; mo < 4; ++mo) o.a[mo] = mfma(wf[mo], bv, o.a[mo]);
  }
  act(o.a, 0);
  load_vp(o.m, w.vB2, g);
  mm64(o.m, w.w2h, w.blob + OFF_W2, o.a, lane, w.us_w2);
  act(o.m, 1);
  load_vp(o.c1, w.vBC1, g);
  mm64(o.c1, w.wc1h, w.blob + OFF_WC1, o.m, lane, w.us_wc1);
  act(o.c1, 2);
  o.c = dot_vp(o.c1, w.vWC2, g) + w.bc2;
  if (w.ctanh) o.c = tanhf(o.c);
}

// ---- node phase ------------------------------------------------------------------------------------
// phi_v's hidden pre-activation WV1 h + bv1 (basic.py:174-176), log2 domain
__device__ __forceinline__ void node_phi_pre(f4 (&t)[4], const float* bj, const f4 (&hr)[4], int lane, int g) {
  load_vp(t, bj + OFF_VEC + V_BV1 * 64, g);
  mm64(t, reinterpret_cast<const h8*>(bj + OFF_H16N + H_WV1 * 4096), bj + OFF_WV1, hr, lane,
       h16_us(bj + OFF_SCAL, HS_N + H_WV1));
}
// phi_v(h) from its hidden activation
__device__ __forceinline__ float node_phi(const f4 (&t)[4], const float* bj, int g) {
  return dot_vp(t, bj + OFF_VEC + V_WV2 * 64, g) + bj[OFF_SCAL + 1];
}
// the node MLP's hidden pre-activation WN1 [h, M] + bn1 (basic.py:182-183): fp16x3, or exact f32 MFMAs
// when an input of the tile leaves the fp16 hi range
__device__ __forceinline__ void node_hidden_pre(f4 (&z)[4], const float* bj, const f4 (&hr)[4], const f4 (&Mr)[4],
                                                int lane, int g) {
  load_vp(z, bj + OFF_VEC + V_BN1 * 64, g);
  if (__builtin_expect(__any(fmaxf(amax_ecl(hr), amax_ecl(Mr)) > H16_LIMIT), 0)) {
    f4 in8[8];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) { in8[mt] = hr[mt]; in8[4 + mt] = Mr[mt]; }
    mfma_dense<8>(z, bj + OFF_WN1, in8, lane);
  } else {
    h8 xh[2], xl[2];
    h16_split(hr, xh, xl);
    mfma_h16(z, reinterpret_cast<const h8*>(bj + OFF_H16N + H_WN1A * 4096), xh, xl, lane, h16_us(bj + OFF_SCAL, HS_N + H_WN1A));
    h16_split(Mr, xh, xl);
    mfma_h16(z, reinterpret_cast<const h8*>(bj + OFF_H16N + H_WN1B * 4096), xh, xl, lane, h16_us(bj + OFF_SCAL, HS_N + H_WN1B));
  }
}

}  // namespace
