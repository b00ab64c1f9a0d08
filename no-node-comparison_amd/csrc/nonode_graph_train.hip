// The reverse of the E(n)-equivariant layer on an explicit edge list (autograd of EGNN_Layer.forward,
// basic.py:167-186, with aggregate basic.py:6-31 and InvariantScalarNet basic.py:107-144; and of one
// substep of SEGNO_GCL.forward, gcl.py:111-119): training on gfx950 for the CSR graph kernels of
// nonode_graph.hip. The node and edge kernels are templated on the variant, as the forward's are.
//
// A translation unit of its own (built with the default machine scheduler). The forward recompute
// calls the forward's own edge step and node pre-activations (nonode_graph_common.h, on the forward
// layer blob of nonode_pack_layer), keeping SiLU' where the forward applies SiLU in place; the
// transposed products read the backward blob (nonode_pack_layer_bwd: true-scale W^T fp16 hi/lo fragments), every
// gradient column scaled by a power of two into [2^11, 2^12) before the fp16 split.
//
//   graph_node_bwd_kernel  per 16-node tile: h' = node_mlp([h, M]) and x' = x + phi_v(h) v +
//                          clamp(F / max(deg, 1), +-100) reversed: dL/dM, dL/dF (clamp mask and 1 / count
//                          applied), the part of dL/dh that does not pass through the edges, dL/dv, and
//                          the node-side operands of the weight gradients. SEGNO: v' = v + cw (F /
//                          max(deg, 1)) dt, x' = x + v' dt reversed (no clamp at the mean, no phi_v)
//   graph_edge_bwd_kernel  one wave per 16 receivers (the walk of graph_edge_kernel): per step the edge
//                          and coordinate MLPs recomputed with their sigmoids kept, then reversed.
//                          SEGNO: dL/dF passes per edge and component where |r_k c| <= 100 (gcl.py:99-100).
//                          The receiver sums (GA = sum gz1, the receiver's share of dL/dx) stay in
//                          registers and are added in CSR order; gz1, dL/dr and the operand rows of
//                          the edge-level weight gradients go to edge_ops at the edge's ORIGINAL
//                          index (so they line up with edge_fea)
//   graph_post_kernel      one wave per 16 senders, walking the CSR by sender: GB = sum gz1 and the
//                          sender's share of dL/dx in CSR order, then dL/dh = part + W_A^T GA + W_B^T GB
//   graph_zero_dropped_kernel  zero rows of edge_ops for edges the CSR build dropped
// No float atomics: the input gradients are bitwise reproducible and, for a list without duplicate
// edges, independent of the list's order.
#include "nonode_graph_common.h"

namespace {

enum { EGNO = 0, SEGNO = 1 };

// node_ops row (floats; SEGNO writes neither GT nor T, and its gphi is 0)
enum : int { GN_GHP = 0, GN_GM = 64, GN_GZ = 128, GN_Z = 192, GN_GT = 256, GN_T = 320, GN_GA = 384, GN_GB = 448,
             GN_GF = 512 /* dL/dF x3, gphi */, GN_GX = 516 /* receiver share of dL/dx x3, 0 */, GN_STRIDE = 520 };
// edge_ops row (floats). Ordered so that the edge-level weight gradients are two tall products over the
// edges, [gz1 | gz2]^T [a | 1, s, e] and [gz3 | gc]^T [m | 1 | c1] (each bias gradient a product with the
// ones column): no matrix-vector product and no separate column sum over a million rows
enum : int { GE_GZ1 = 0, GE_GZ2 = 64, GE_A = 128, GE_X8 = 192 /* 1, s, e_0 .. e_3, 0, 0 */, GE_GZ3 = 200,
             GE_GC = 264 /* gc, dL/dr x3 */, GE_M = 268, GE_ONE = 332 /* 1, 0, 0, 0 */, GE_C1 = 336, GE_STRIDE = 400 };

struct GraphBwdArgs {
  int n_nodes, f0, nf, ne, ef_frames;   // frames f0 .. f0 + nf - 1 of the launch
  long long E;
  const float* h; const float* x; const float* v; const float* ef;
  const float* blob; const float* bb;
  const float* P; const float* Q; const float* M; const float* F;   // the forward's state
  const int* row_ptr; const int* col; const int* eid;               // CSR by receiver
  const int* srow_ptr; const int* seid;                             // CSR by sender
  const int* valid;
  const float* gxo; const float* gvo; const float* gho;             // gradients of the outputs (null = 0)
  float* nops; float* eops;                                         // rows relative to frame f0
  float* gh; float* gx; float* gv;                                  // gradients of the inputs
  float dt, cw; int recurrent;                                      // SEGNO (gcl.py:111-119)
};

// a' = SiLU in the log2 domain (silu_ecl's expression) and d = SiLU'(z) of the true pre-activation
// z = -ln2 z', from the one sigmoid s = 1 / (1 + 2^z'): d = s (1 + z (1 - s))
__device__ __forceinline__ void silu2_keep(const f4 (&zp)[4], f4 (&a)[4], f4 (&d)[4]) {
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float z = zp[mt][q];   // a may be zp
      const float s = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(z));
      a[mt][q] = z * s;
      d[mt][q] = s * fmaf(z * NEG_LN2, 1.f - s, 1.f);
    }
}
// the edge step's activation for the reverse pass: d[i] = SiLU' of pre-activation i
struct SiluKeep {
  f4 d[3][4];
  __device__ __forceinline__ void operator()(f4 (&z)[4], int i) { silu2_keep(z, z, d[i]); }
};

// ---- node reverse (basic.py:174-185 reversed; the per-node count of aggregate, basic.py:28) ---------
// SEGNO (gcl.py:85-95, 111-119 reversed): g_v_in = g_v' + dt g_x', dL/dF = g_v_in cw dt / max(deg, 1)
template <int VARIANT>
__global__ __launch_bounds__(256) void graph_node_bwd_kernel(GraphBwdArgs p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, e = lane & 15, g = lane >> 4;
  Tile t;
  if (!tile_of(p.n_nodes, p.f0, p.nf, e, wave, t)) return;
  const size_t r = t.r;
  const float* bj = p.blob;
  const float* bb = p.bb;
  const h8* BH = reinterpret_cast<const h8*>(bb + BOFF_H16);
  f4 hr[4], Mr[4];
  load_ecl(hr, p.h + r * HID, g);
  load_ecl(Mr, p.M + r * HID, g);
  const f4 Fr = *reinterpret_cast<const f4*>(p.F + r * 4);
  const float inv = 1.f / fmaxf(Fr[3], 1.f);
  // forward recompute: phi_v(h) (EGNO) and the node MLP's hidden layer
  f4 tt[4], dt[4];
  float phi = 0.f;
  if (VARIANT == EGNO) {
    f4 tp[4];
    node_phi_pre(tp, bj, hr, lane, g);
    silu2_keep(tp, tt, dt);
    phi = node_phi(tt, bj, g);
  }
  f4 zp[4], z[4], dz[4];
  node_hidden_pre(zp, bj, hr, Mr, lane, g);
  silu2_keep(zp, z, dz);
  float gx0 = 0.f, gx1 = 0.f, gx2 = 0.f, gv0 = 0.f, gv1 = 0.f, gv2 = 0.f;
  if (p.gxo) { gx0 = p.gxo[r * 3 + 0]; gx1 = p.gxo[r * 3 + 1]; gx2 = p.gxo[r * 3 + 2]; }
  if (p.gvo) { gv0 = p.gvo[r * 3 + 0]; gv1 = p.gvo[r * 3 + 1]; gv2 = p.gvo[r * 3 + 2]; }
  float gphi = 0.f, gF0, gF1, gF2;
  f4 gt[4], gh[4];
  if (VARIANT == EGNO) {
    const float v0 = p.v[r * 3 + 0], v1 = p.v[r * 3 + 1], v2 = p.v[r * 3 + 2];
    gphi = gx0 * v0 + gx1 * v1 + gx2 * v2;
    // clamp(F / count, +-100) passes the gradient inside [-100, 100]
    const float F0 = Fr[0] * inv, F1 = Fr[1] * inv, F2 = Fr[2] * inv;
    gF0 = (F0 >= -100.f && F0 <= 100.f) ? gx0 * inv : 0.f;
    gF1 = (F1 >= -100.f && F1 <= 100.f) ? gx1 * inv : 0.f;
    gF2 = (F2 >= -100.f && F2 <= 100.f) ? gx2 * inv : 0.f;
    // gt = gphi wv2 (.) silu'(tp);  gh = WV1^T gt
    load_vp(gt, bb + BOFF_VEC + BV_WV2 * 64, g);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) gt[mt] *= gphi;
    mul4(gt, dt);
    zero4(gh);
    mm64_cs(gh, BH + BH_WV1T * 1024, gt, lane, h16_us(bb + BOFF_SCAL, BH_WV1T));
  } else {
    // v' = v + cw (F / count) dt, x' = x + v' dt: no clamp at the mean (the per-edge clamp's mask is
    // graph_edge_bwd_kernel's), no phi_v
    gv0 = fmaf(p.dt, gx0, gv0); gv1 = fmaf(p.dt, gx1, gv1); gv2 = fmaf(p.dt, gx2, gv2);
    const float f = p.cw * p.dt * inv;
    gF0 = gv0 * f; gF1 = gv1 * f; gF2 = gv2 * f;
  }
  // node MLP reverse: gz = WN2^T gho (.) silu'(zp), gh += WN1h^T gz, gM = WN1m^T gz
  f4 gho[4], gz[4], gM[4];
  if (p.gho) load_ecl(gho, p.gho + r * HID, g);
  else zero4(gho);
  if (VARIANT == SEGNO) {   // h' = node_mlp([h, M]) + h if recurrent (gcl.py:93-94)
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) gh[mt] = p.recurrent ? gho[mt] : f4{0.f, 0.f, 0.f, 0.f};
  }
  zero4(gz);
  mm64_cs(gz, BH + BH_WN2T * 1024, gho, lane, h16_us(bb + BOFF_SCAL, BH_WN2T));
  mul4(gz, dz);
  mm64_cs(gh, BH + BH_WN1TH * 1024, gz, lane, h16_us(bb + BOFF_SCAL, BH_WN1TH));
  zero4(gM);
  mm64_cs(gM, BH + BH_WN1TM * 1024, gz, lane, h16_us(bb + BOFF_SCAL, BH_WN1TM));
  if (t.rvalid) {
    float* o = p.nops + t.rr * GN_STRIDE;
    f4 zt[4], ttrue[4];
    scale4(zt, z, NEG_LN2);       // true-scale activations: the operands of dWn2 and dwv2
    if (VARIANT == EGNO) scale4(ttrue, tt, NEG_LN2);
    store_ecl(o + GN_GHP, gh, g);
    store_ecl(o + GN_GM, gM, g);
    store_ecl(o + GN_GZ, gz, g);
    store_ecl(o + GN_Z, zt, g);
    if (VARIANT == EGNO) {
      store_ecl(o + GN_GT, gt, g);
      store_ecl(o + GN_T, ttrue, g);
    }
    if (g == 0) {
      *reinterpret_cast<f4*>(o + GN_GF) = f4{gF0, gF1, gF2, gphi};
      if (VARIANT == EGNO) {
        p.gv[r * 3 + 0] = gv0 + phi * gx0;
        p.gv[r * 3 + 1] = gv1 + phi * gx1;
        p.gv[r * 3 + 2] = gv2 + phi * gx2;
      } else {
        p.gv[r * 3 + 0] = gv0;
        p.gv[r * 3 + 1] = gv1;
        p.gv[r * 3 + 2] = gv2;
      }
    }
  }
}

// ---- edge reverse (basic.py:170-173, 107-144 reversed) on the receiver CSR -----------------------
// LDS: W2 | Wc1 (forward blob) and W2^T | Wc1^T (backward blob) fp16 hi/lo fragments, the forward's
// edge-phase vectors, and the true-scale wc2 and W1[:, s] vectors
constexpr int GEB_VEC = 16384, GEB_WC2T = GEB_VEC + EDGE_STAGE_FLOATS, GEB_WS = GEB_WC2T + 64;
constexpr int GEB_LDS_FLOATS = GEB_WS + 64;
template <int VARIANT, int KF>
__global__ __launch_bounds__(256) void graph_edge_bwd_kernel(GraphBwdArgs p) {
  extern __shared__ __attribute__((aligned(16))) float sW[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, e = lane & 15, g = lane >> 4;
  stage_edge_weights(sW, sW + GEB_VEC, p.blob, tid);
  for (int i = tid; i < 2048; i += 256)
    reinterpret_cast<f4*>(sW + 8192)[i] = reinterpret_cast<const f4*>(p.bb + BOFF_H16 + BH_W2T * 4096)[i];
  if (tid < 16) reinterpret_cast<f4*>(sW + GEB_WC2T)[tid] = reinterpret_cast<const f4*>(p.bb + BOFF_VEC + BV_WC2 * 64)[tid];
  else if (tid < 32) reinterpret_cast<f4*>(sW + GEB_WS)[tid - 16] = reinterpret_cast<const f4*>(p.bb + BOFF_VEC + BV_WS * 64)[tid - 16];
  __syncthreads();
  static_assert(BH_WC1T == BH_W2T + 1, "W2^T | Wc1^T are staged as one block");
  const EdgeWeights w = edge_weights(sW, sW + GEB_VEC, p.blob);
  const h8* w2th = reinterpret_cast<const h8*>(sW + 8192);
  const h8* wc1th = reinterpret_cast<const h8*>(sW + 12288);
  const unsigned us_w2t = h16_us(p.bb + BOFF_SCAL, BH_W2T), us_wc1t = h16_us(p.bb + BOFF_SCAL, BH_WC1T);

  Tile t;
  if (!tile_of(p.n_nodes, p.f0, p.nf, e, wave, t)) return;
  const size_t r = t.r;
  const CsrRow row(p.row_ptr, t.nc, t.rvalid);
  EdgeInputs in;
  in.x = p.x; in.Q = p.Q; in.ne = p.ne;
  in.efb = p.ef + (size_t)(t.fa % p.ef_frames) * (size_t)p.E * p.ne;
  float* erow0 = p.eops + (size_t)t.fr * (size_t)p.E * GE_STRIDE;
  const float* nrow = p.nops + t.rr * GN_STRIDE;
  f4 gM[4], GA[4];
  load_ecl(in.pr, p.P + r * HID, g);
  load_ecl(gM, nrow + GN_GM, g);
  const f4 gF = *reinterpret_cast<const f4*>(nrow + GN_GF);
  in.xr0 = p.x[r * 3 + 0]; in.xr1 = p.x[r * 3 + 1]; in.xr2 = p.x[r * 3 + 2];
  zero4(GA);
  float gxa0 = 0.f, gxa1 = 0.f, gxa2 = 0.f;
  int jn, idn;
  row.entry(p.col, p.eid, t.nc, 0, jn, idn);
#pragma unroll 1
  for (int k = 0; k < row.kmax; ++k) {
    const int j = jn, id = idn;
    const bool on = k < row.deg;
    row.entry(p.col, p.eid, t.nc, k + 1, jn, idn);
    // ---- forward recompute, the sigmoids kept as SiLU' ----
    SiluKeep act;
    EdgeStep st;
    edge_step<KF>(w, in, t.fbase + j, id, lane, g, act, st);
    const f4 (&a)[4] = st.a, (&m)[4] = st.m, (&c1)[4] = st.c1;
    const f4 (&d1)[4] = act.d[0], (&dm)[4] = act.d[1], (&dc)[4] = act.d[2];
    const float r0 = st.r0, r1 = st.r1, r2 = st.r2, d2raw = st.d2raw, d2 = st.d2, c = st.c;
    const bool rnorm = w.rnorm, ctanh = w.ctanh;
    // ---- reverse ----
    // f_ij = r c, F_i = sum_j f_ij; SEGNO clamps every component of f_ij to +-100 (gcl.py:99-100), which
    // passes the gradient inside [-100, 100]
    float gf0 = gF[0], gf1 = gF[1], gf2 = gF[2];
    if (VARIANT == SEGNO) {
      const float f0 = r0 * c, f1 = r1 * c, f2 = r2 * c;
      gf0 = (f0 >= -100.f && f0 <= 100.f) ? gf0 : 0.f;
      gf1 = (f1 >= -100.f && f1 <= 100.f) ? gf1 : 0.f;
      gf2 = (f2 >= -100.f && f2 <= 100.f) ? gf2 : 0.f;
    }
    float gc = gf0 * r0 + gf1 * r1 + gf2 * r2;
    if (ctanh) gc *= 1.f - c * c;
    f4 gz3[4];
    load_vp(gz3, sW + GEB_WC2T, g);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) gz3[mt] *= gc;
    mul4(gz3, dc);
    f4 gz2[4];   // gm = Wc1^T gz3 + gM_i, then (.) silu'(z2)
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) gz2[mt] = gM[mt];
    mm64_cs(gz2, wc1th, gz3, lane, us_wc1t);
    mul4(gz2, dm);
    f4 gz1[4];
    zero4(gz1);
    mm64_cs(gz1, w2th, gz2, lane, us_w2t);
    mul4(gz1, d1);
    // the radial input s = |r|^2 (normalised: s / max(s, 1e-12), whose slope is 1e12 below 1e-12, else 0)
    const float gs = dot_vp(gz1, sW + GEB_WS, g);
    const float dsd = rnorm ? (d2raw < 1e-12f ? 1e12f : 0.f) : 1.f;
    const float gd = 2.f * gs * dsd;
    const float dr0 = fmaf(gd, r0, gf0 * c), dr1 = fmaf(gd, r1, gf1 * c), dr2 = fmaf(gd, r2, gf2 * c);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int q = 0; q < 4; ++q) GA[mt][q] = on ? GA[mt][q] + gz1[mt][q] : GA[mt][q];
    gxa0 = on ? gxa0 + dr0 : gxa0;
    gxa1 = on ? gxa1 + dr1 : gxa1;
    gxa2 = on ? gxa2 + dr2 : gxa2;
    if (on) {
      float* o = erow0 + (size_t)id * GE_STRIDE;
      f4 tr[4];
      store_ecl(o + GE_GZ1, gz1, g);
      scale4(tr, a, NEG_LN2);
      store_ecl(o + GE_A, tr, g);
      store_ecl(o + GE_GZ2, gz2, g);
      scale4(tr, m, NEG_LN2);
      store_ecl(o + GE_M, tr, g);
      store_ecl(o + GE_GZ3, gz3, g);
      scale4(tr, c1, NEG_LN2);
      store_ecl(o + GE_C1, tr, g);
      if (g == 0) {
        float ev[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (q < p.ne) ev[q] = in.efb[(size_t)id * p.ne + q];
        *reinterpret_cast<f4*>(o + GE_X8) = f4{1.f, d2, ev[0], ev[1]};
        *reinterpret_cast<f4*>(o + GE_X8 + 4) = f4{ev[2], ev[3], 0.f, 0.f};
        *reinterpret_cast<f4*>(o + GE_GC) = f4{gc, dr0, dr1, dr2};
        *reinterpret_cast<f4*>(o + GE_ONE) = f4{1.f, 0.f, 0.f, 0.f};
      }
    }
  }
  if (t.rvalid) {
    float* o = p.nops + t.rr * GN_STRIDE;
    store_ecl(o + GN_GA, GA, g);
    if (g == 0) *reinterpret_cast<f4*>(o + GN_GX) = f4{gxa0, gxa1, gxa2, 0.f};
  }
}

// ---- sender sums and the input gradients of h and x ------------------------------------------------
__global__ __launch_bounds__(256) void graph_post_kernel(GraphBwdArgs p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, e = lane & 15, g = lane >> 4;
  Tile t;
  if (!tile_of(p.n_nodes, p.f0, p.nf, e, wave, t)) return;
  const size_t r = t.r;
  const CsrRow row(p.srow_ptr, t.nc, t.rvalid);
  const float* erow0 = p.eops + (size_t)t.fr * (size_t)p.E * GE_STRIDE;
  f4 GB[4];
  zero4(GB);
  float gs0 = 0.f, gs1 = 0.f, gs2 = 0.f;
#pragma unroll 1
  for (int k = 0; k < row.kmax; ++k) {
    const bool on = k < row.deg;
    const int id = row.edge(p.seid, k);
    const float* o = erow0 + (size_t)id * GE_STRIDE;
    f4 gz1[4];
    load_ecl(gz1, o + GE_GZ1, g);
    const f4 t0 = *reinterpret_cast<const f4*>(o + GE_GC);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int q = 0; q < 4; ++q) GB[mt][q] = on ? GB[mt][q] + gz1[mt][q] : GB[mt][q];
    gs0 = on ? gs0 + t0[1] : gs0;
    gs1 = on ? gs1 + t0[2] : gs1;
    gs2 = on ? gs2 + t0[3] : gs2;
  }
  float* nrow = p.nops + t.rr * GN_STRIDE;
  const float* bb = p.bb;
  const h8* BH = reinterpret_cast<const h8*>(bb + BOFF_H16);
  f4 gh[4], GA[4];
  load_ecl(gh, nrow + GN_GHP, g);
  load_ecl(GA, nrow + GN_GA, g);
  mm64_cs(gh, BH + BH_WAT * 1024, GA, lane, h16_us(bb + BOFF_SCAL, BH_WAT));
  mm64_cs(gh, BH + BH_WBT * 1024, GB, lane, h16_us(bb + BOFF_SCAL, BH_WBT));
  if (t.rvalid) {
    store_ecl(nrow + GN_GB, GB, g);
    store_ecl(p.gh + r * HID, gh, g);
    if (g == 0) {
      const f4 gr = *reinterpret_cast<const f4*>(nrow + GN_GX);
      float g0 = 0.f, g1 = 0.f, g2 = 0.f;
      if (p.gxo) { g0 = p.gxo[r * 3 + 0]; g1 = p.gxo[r * 3 + 1]; g2 = p.gxo[r * 3 + 2]; }
      p.gx[r * 3 + 0] = g0 + gr[0] - gs0;
      p.gx[r * 3 + 1] = g1 + gr[1] - gs1;
      p.gx[r * 3 + 2] = g2 + gr[2] - gs2;
    }
  }
}

// rows of edges the CSR build dropped (valid[e] == 0) are zero in every frame: one wave per row
__global__ __launch_bounds__(256) void graph_zero_dropped_kernel(const int* __restrict__ valid, long long E, int nf,
                                                                 float* eops) {
  const int lane = threadIdx.x & 63;
  const long long rows = E * nf, stride = (long long)gridDim.x * 4;
  for (long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += stride) {
    if (valid[row % E]) continue;
    f4* o = reinterpret_cast<f4*>(eops + (size_t)row * GE_STRIDE);
    o[lane] = f4{0.f, 0.f, 0.f, 0.f};
    if (lane + 64 < GE_STRIDE / 4) o[lane + 64] = f4{0.f, 0.f, 0.f, 0.f};
  }
}

// valid[eid[p]] = 1 for the CSR's kept entries p < row_ptr[n_nodes]
__global__ __launch_bounds__(256) void graph_mark_kernel(const int* __restrict__ row_ptr, const int* __restrict__ eid,
                                                         int n_nodes, long long E, int* valid) {
  const long long pos = (long long)blockIdx.x * 256 + threadIdx.x;
  if (pos >= E || pos >= row_ptr[n_nodes]) return;
  valid[eid[pos]] = 1;
}

// validation (EUNSUPPORTED / EINVAL before any launch) and the launches of one variant's reverse
template <int VARIANT>
int graph_layer_bwd(const char* who, int n_frames, int n_nodes, long long E, int n_edge_feat, int ef_frames, int f0,
                    int f1, const float* h, const float* x, const float* v, const float* edge_fea, const float* blob,
                    const float* bblob, const float* state, const int* row_ptr, const int* col, const int* eid,
                    const int* srow_ptr, const int* seid, const int* valid, const float* g_x, const float* g_v,
                    const float* g_h, float dt, float cw, int recurrent, float* node_ops, float* edge_ops,
                    float* g_h_in, float* g_x_in, float* g_v_in, hipStream_t s) {
  const long long n_total = (long long)n_frames * n_nodes;
  if (n_frames <= 0 || n_nodes <= 0 || n_total > (1ll << 30) || E < 0 || E >= (1ll << 31) || n_edge_feat < 0 ||
      n_edge_feat > 4 || ef_frames <= 0 || f0 < 0 || f1 <= f0 || f1 > n_frames)
    return fail(NONODE_EUNSUPPORTED, "%s: n_frames=%d n_nodes=%d E=%lld ne=%d ef_frames=%d frames [%d, %d)", who,
                n_frames, n_nodes, E, n_edge_feat, ef_frames, f0, f1);
  if (!h || !x || !v || !blob || !bblob || !state || !row_ptr || !srow_ptr || !node_ops || !g_h_in || !g_x_in || !g_v_in ||
      (E > 0 && (!col || !eid || !seid || !edge_ops || (n_edge_feat > 0 && !edge_fea))))
    return fail(NONODE_EINVAL, "%s: null pointer", who);
  GraphBwdArgs a;
  a.n_nodes = n_nodes; a.f0 = f0; a.nf = f1 - f0; a.ne = n_edge_feat; a.ef_frames = ef_frames; a.E = E;
  a.h = h; a.x = x; a.v = v; a.ef = n_edge_feat ? edge_fea : blob; a.blob = blob; a.bb = bblob;
  const size_t n = (size_t)n_total;
  a.P = state; a.Q = state + n * HID; a.M = state + 2 * n * HID; a.F = state + 3 * n * HID;
  a.row_ptr = row_ptr; a.col = col; a.eid = eid; a.srow_ptr = srow_ptr; a.seid = seid; a.valid = valid;
  a.gxo = g_x; a.gvo = g_v; a.gho = g_h;
  a.nops = node_ops; a.eops = edge_ops;
  a.gh = g_h_in; a.gx = g_x_in; a.gv = g_v_in;
  a.dt = dt; a.cw = cw; a.recurrent = recurrent;
  static std::once_flag once;   // (one per variant)
  std::call_once(once, [] {
    hipFuncSetAttribute((const void*)graph_edge_bwd_kernel<VARIANT, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, GEB_LDS_FLOATS * 4);
    hipFuncSetAttribute((const void*)graph_edge_bwd_kernel<VARIANT, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, GEB_LDS_FLOATS * 4);
  });
  const int tpf = (n_nodes + 15) / 16;
  const unsigned blocks = (unsigned)(((long long)a.nf * tpf + 3) / 4);
  if (valid && E > 0) {
    const long long rows = E * a.nf;
    const unsigned zb = (unsigned)(rows / 4 + 1 < 4096 ? rows / 4 + 1 : 4096);
    hipLaunchKernelGGL(graph_zero_dropped_kernel, dim3(zb), dim3(256), 0, s, valid, E, a.nf, edge_ops);
    if (int rc = check_launch("graph_zero_dropped_kernel")) return rc;
  }
  hipLaunchKernelGGL(graph_node_bwd_kernel<VARIANT>, dim3(blocks), dim3(256), 0, s, a);
  if (int rc = check_launch("graph_node_bwd_kernel")) return rc;
  if (n_edge_feat <= 3) hipLaunchKernelGGL((graph_edge_bwd_kernel<VARIANT, 1>), dim3(blocks), dim3(256), GEB_LDS_FLOATS * 4, s, a);
  else hipLaunchKernelGGL((graph_edge_bwd_kernel<VARIANT, 2>), dim3(blocks), dim3(256), GEB_LDS_FLOATS * 4, s, a);
  if (int rc = check_launch("graph_edge_bwd_kernel")) return rc;
  hipLaunchKernelGGL(graph_post_kernel, dim3(blocks), dim3(256), 0, s, a);
  return check_launch("graph_post_kernel");
}

}  // namespace

extern "C" {

int nonode_graph_edge_mask(const int* row_ptr, const int* eid, int n_nodes, long long E, int* valid, void* stream) {
  if (E < 0 || E >= (1ll << 31) || n_nodes <= 0) return fail(NONODE_EINVAL, "graph_edge_mask: E=%lld n_nodes=%d", E, n_nodes);
  if (E == 0) return NONODE_OK;
  if (!row_ptr || !eid || !valid) return fail(NONODE_EINVAL, "graph_edge_mask: null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(valid, 0, (size_t)E * sizeof(int), s) != hipSuccess) return fail(NONODE_ELAUNCH, "graph_edge_mask: memset");
  hipLaunchKernelGGL(graph_mark_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, s, row_ptr, eid, n_nodes, E, valid);
  return check_launch("graph_mark_kernel");
}

size_t nonode_egnn_layer_graph_bwd_node_floats(int n_frames, int n_nodes) {
  if (n_frames <= 0 || n_nodes <= 0) return 0;
  return (size_t)n_frames * n_nodes * GN_STRIDE;
}
size_t nonode_egnn_layer_graph_bwd_edge_floats(int n_frames, long long E) {
  if (n_frames <= 0 || E <= 0) return 0;
  return (size_t)n_frames * (size_t)E * GE_STRIDE;
}

int nonode_egnn_layer_graph_bwd(int variant, int n_frames, int n_nodes, long long E, int n_edge_feat, int ef_frames,
                                int f0, int f1, const float* h, const float* x, const float* v, const float* edge_fea,
                                const float* blob, const float* bblob, const float* state, const int* row_ptr,
                                const int* col, const int* eid, const int* srow_ptr, const int* seid, const int* valid,
                                const float* g_x, const float* g_v, const float* g_h, float* node_ops, float* edge_ops,
                                float* g_h_in, float* g_x_in, float* g_v_in, void* stream) {
  if (variant != NONODE_VARIANT_EGNO) return fail(NONODE_EUNSUPPORTED, "egnn_layer_graph_bwd: variant %d (EGNO only)", variant);
  return graph_layer_bwd<EGNO>("egnn_layer_graph_bwd", n_frames, n_nodes, E, n_edge_feat, ef_frames, f0, f1, h, x, v,
                               edge_fea, blob, bblob, state, row_ptr, col, eid, srow_ptr, seid, valid, g_x, g_v, g_h, 0.f,
                               1.f, 0, node_ops, edge_ops, g_h_in, g_x_in, g_v_in, (hipStream_t)stream);
}

int nonode_segno_layer_graph_bwd(int n_nodes, long long E, int n_edge_feat, const float* h, const float* x,
                                 const float* v, const float* edge_attr, const float* blob, const float* bblob,
                                 const float* state, const int* row_ptr, const int* col, const int* eid,
                                 const int* srow_ptr, const int* seid, const int* valid, const float* g_x,
                                 const float* g_v, const float* g_h, float dt, float coords_weight, int recurrent,
                                 float* node_ops, float* edge_ops, float* g_h_in, float* g_x_in, float* g_v_in,
                                 void* stream) {
  return graph_layer_bwd<SEGNO>("segno_layer_graph_bwd", 1, n_nodes, E, n_edge_feat, 1, 0, 1, h, x, v, edge_attr, blob,
                                bblob, state, row_ptr, col, eid, srow_ptr, seid, valid, g_x, g_v, g_h, dt, coords_weight,
                                recurrent, node_ops, edge_ops, g_h_in, g_x_in, g_v_in, (hipStream_t)stream);
}

}  // extern "C"
