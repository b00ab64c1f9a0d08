// The E(n)-equivariant layer on an explicit edge list (EGNN_Layer.forward, basic.py:167-186;
// SEGNO_GCL.forward, gcl.py:111-119, for any `edges`): inference on gfx950.
//
// A translation unit of its own (built with the default machine scheduler). It reads the packed layer
// blob of nonode_pack_layer unchanged (fp16 hi/lo fragments for the fp16x3 products, f32 fragments for
// the range guard's exact path, the scalar-input k-steps, the log2-domain SiLU scalings) and keeps the
// fused kernel's arithmetic per edge. The tile indexing, the CSR row walk, the edge step and the node
// step's pre-activations are nonode_graph_common.h's, which the reverse pass (nonode_graph_train.hip)
// calls as well.
//
//   graph_*_kernel (build)  the edge list as a CSR by receiver, rows ordered by (sender, original
//                           index): a pure function of the edge set
//   graph_proj_kernel       P = W1[h_i] h + b1, Q = W1[h_j] h per node (phase A of the fused kernel,
//                           held in global memory)
//   graph_edge_kernel       one wave per 16 receivers (the 16 MFMA columns, ECL layout); step k pairs
//                           column e with the k-th entry of its CSR row, to the tile's largest degree;
//                           a column past its own degree is masked by select. Message and force sums
//                           stay in registers and are added in CSR order: no float atomics, bitwise
//                           reproducible sums
//   graph_node_kernel       the node update per 16-node tile with the segment mean's count.clamp(min=1)
#include "nonode_graph_common.h"

namespace {

enum { EGNO = 0, SEGNO = 1 };

// ---- CSR by receiver ----------------------------------------------------------------------------
// count the receivers' valid edges; an index outside [0, n_nodes) sets the flag and the edge is dropped
template <typename I>
__global__ __launch_bounds__(256) void graph_count_kernel(const I* __restrict__ rows, const I* __restrict__ cols,
                                                          long long E, int n_nodes, int* cnt, int* flag) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  const long long r = (long long)rows[e], c = (long long)cols[e];
  if (r < 0 || r >= n_nodes || c < 0 || c >= n_nodes) *flag = 1;
  else atomicAdd(cnt + r, 1);
}
// row_ptr = exclusive prefix sum of cnt (one workgroup, 1024 rows per round), cnt <- row_ptr (the fill's cursors)
__global__ __launch_bounds__(1024) void graph_scan_kernel(int n_nodes, int* cnt, int* row_ptr) {
  __shared__ int part[16];
  __shared__ int carry;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < n_nodes; base += 1024) {
    const int i = base + tid;
    const int c = i < n_nodes ? cnt[i] : 0;
    int s = c;   // inclusive scan inside the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(s, o);
      if (lane >= o) s += t;
    }
    if (lane == 63) part[wave] = s;
    __syncthreads();
    int off = carry;
    for (int w = 0; w < wave; ++w) off += part[w];
    if (i < n_nodes) {
      row_ptr[i] = off + s - c;
      cnt[i] = off + s - c;
    }
    __syncthreads();
    if (tid == 1023) carry = off + s;
    __syncthreads();
  }
  if (tid == 0) row_ptr[n_nodes] = carry;
}
// every valid edge takes the next free slot of its receiver's row (any order: graph_sort_kernel orders it)
template <typename I>
__global__ __launch_bounds__(256) void graph_fill_kernel(const I* __restrict__ rows, const I* __restrict__ cols,
                                                         long long E, int n_nodes, int* cursor, int* tcol, int* teid) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  const long long r = (long long)rows[e], c = (long long)cols[e];
  if (r < 0 || r >= n_nodes || c < 0 || c >= n_nodes) return;
  const int slot = atomicAdd(cursor + r, 1);
  tcol[slot] = (int)c;
  teid[slot] = (int)e;
}
// one wave per row: entry i goes to its rank under (sender, original index), a total order
__global__ __launch_bounds__(256) void graph_sort_kernel(int n_nodes, const int* __restrict__ row_ptr,
                                                         const int* __restrict__ tcol, const int* __restrict__ teid,
                                                         int* __restrict__ col, int* __restrict__ eid) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= n_nodes) return;
  const int p0 = row_ptr[r], d = row_ptr[r + 1] - p0;
  for (int i = lane; i < d; i += 64) {
    const int ci = tcol[p0 + i], ei = teid[p0 + i];
    int rank = 0;
    for (int m = 0; m < d; ++m) {
      const int cm = tcol[p0 + m], em = teid[p0 + m];
      rank += (cm < ci || (cm == ci && em < ei)) ? 1 : 0;
    }
    col[p0 + rank] = ci;
    eid[p0 + rank] = ei;
  }
}

// ---- the layer ------------------------------------------------------------------------------------
struct GraphArgs {
  int n_frames, n_nodes, n_total, ne, ef_frames, recurrent;
  long long E;
  const float* __restrict__ h; const float* __restrict__ x; const float* __restrict__ v;
  const float* __restrict__ ef; const float* __restrict__ blob;
  const int* __restrict__ row_ptr; const int* __restrict__ col; const int* __restrict__ eid;
  float* P; float* Q; float* M; float* F;   // workspace [n][64] x 3, [n][4] = (force sum, degree)
  float* h_out; float* x_out; float* v_out;
  float dt, cw;
};
constexpr int GRAPH_WS_ROW = 3 * HID + 4;   // workspace floats per node row

// P, Q rows of 16 nodes per wave (the fused kernel's proj_tile)
__global__ __launch_bounds__(256) void graph_proj_kernel(GraphArgs p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, e = lane & 15, g = lane >> 4;
  const int r0 = (blockIdx.x * 4 + wave) * 16;
  if (r0 >= p.n_total) return;
  const bool rvalid = r0 + e < p.n_total;
  const int r = rvalid ? r0 + e : p.n_total - 1;
  const float* blob = p.blob;
  f4 hin[4], ap[4], aq[4];
  load_ecl(hin, p.h + (size_t)r * HID, g);
  load_vp(ap, blob + OFF_VEC + V_B1 * 64, g);
  zero4(aq);
  if (__builtin_expect(__any(amax_ecl(hin) > H16_LIMIT), 0)) {
    mfma_dense<4>(ap, blob + OFF_WA, hin, lane);
    mfma_dense<4>(aq, blob + OFF_WB, hin, lane);
  } else {
    h8 xh[2], xl[2];
    h16_split(hin, xh, xl);
    mfma_h16(ap, reinterpret_cast<const h8*>(blob + OFF_H16N + H_WA * 4096), xh, xl, lane, h16_us(blob + OFF_SCAL, HS_N + H_WA));
    mfma_h16(aq, reinterpret_cast<const h8*>(blob + OFF_H16N + H_WB * 4096), xh, xl, lane, h16_us(blob + OFF_SCAL, HS_N + H_WB));
  }
  if (rvalid) {
    store_ecl(p.P + (size_t)r * HID, ap, g);
    store_ecl(p.Q + (size_t)r * HID, aq, g);
  }
}

// The edge walk. W2 / Wc1 fp16 fragments and the edge-phase vectors are staged in LDS once per
// workgroup (35 KB: four workgroups per CU); every 64x64 product goes through mm64 (fp16x3, or exact
// f32 MFMAs when the tile's activations leave the fp16 hi range).
struct SiluInPlace {
  __device__ __forceinline__ void operator()(f4 (&z)[4], int) const { silu_ecl(z); }
};
template <int VARIANT, int KF>
__global__ __launch_bounds__(256) void graph_edge_kernel(GraphArgs p) {
  __shared__ __attribute__((aligned(16))) float sW[8192 + EDGE_STAGE_FLOATS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, e = lane & 15, g = lane >> 4;
  stage_edge_weights(sW, sW + 8192, p.blob, tid);
  __syncthreads();
  const EdgeWeights w = edge_weights(sW, sW + 8192, p.blob);
  Tile t;
  if (!tile_of(p.n_nodes, 0, p.n_frames, e, wave, t)) return;
  const size_t r = t.r;
  const CsrRow row(p.row_ptr, t.nc, t.rvalid);
  EdgeInputs in;
  in.x = p.x; in.Q = p.Q; in.ne = p.ne;
  in.efb = p.ef + (size_t)(t.fa % p.ef_frames) * (size_t)p.E * p.ne;
  load_ecl(in.pr, p.P + r * HID, g);
  in.xr0 = p.x[r * 3 + 0]; in.xr1 = p.x[r * 3 + 1]; in.xr2 = p.x[r * 3 + 2];
  f4 msum[4];
  zero4(msum);
  float fs0 = 0.f, fs1 = 0.f, fs2 = 0.f;
  SiluInPlace act;
  int jn, idn;
  row.entry(p.col, p.eid, t.nc, 0, jn, idn);
#pragma unroll 1
  for (int k = 0; k < row.kmax; ++k) {
    const int j = jn, id = idn;
    const bool on = k < row.deg;
    row.entry(p.col, p.eid, t.nc, k + 1, jn, idn);   // the next step's indices, a step ahead of their gathers
    EdgeStep st;
    edge_step<KF>(w, in, t.fbase + j, id, lane, g, act, st);
    float f0 = st.r0 * st.c, f1 = st.r1 * st.c, f2 = st.r2 * st.c;
    if (VARIANT == SEGNO) {   // gcl.py:99-100 clamps every edge's translation
      f0 = fminf(fmaxf(f0, -100.f), 100.f);
      f1 = fminf(fmaxf(f1, -100.f), 100.f);
      f2 = fminf(fmaxf(f2, -100.f), 100.f);
    }
    // select, not a multiply by zero: nothing of a padded lane reaches the sums
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int q = 0; q < 4; ++q) msum[mt][q] = on ? msum[mt][q] + st.m[mt][q] : msum[mt][q];
    fs0 = on ? fs0 + f0 : fs0;
    fs1 = on ? fs1 + f1 : fs1;
    fs2 = on ? fs2 + f2 : fs2;
  }
  if (t.rvalid) {
    store_ecl(p.M + r * HID, msum, g);
    if (g == 0) *reinterpret_cast<f4*>(p.F + r * 4) = f4{fs0, fs1, fs2, (float)row.deg};
  }
}

// node update of 16 rows per wave (the fused kernel's node job): an isolated node has F = M = 0 and
// count.clamp(min=1) = 1 (basic.py:6-31 aggregate, gcl.py unsorted_segment_mean)
template <int VARIANT>
__global__ __launch_bounds__(256) void graph_node_kernel(GraphArgs p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, e = lane & 15, g = lane >> 4;
  const int r0 = (blockIdx.x * 4 + wave) * 16;
  if (r0 >= p.n_total) return;
  const bool rvalid = r0 + e < p.n_total;
  const size_t r = rvalid ? r0 + e : p.n_total - 1;
  const float* bj = p.blob;
  f4 hr[4], Mr[4];
  load_ecl(hr, p.h + r * HID, g);
  load_ecl(Mr, p.M + r * HID, g);
  const f4 Fr = *reinterpret_cast<const f4*>(p.F + r * 4);
  const float inv = 1.f / fmaxf(Fr[3], 1.f);
  const float x0 = p.x[r * 3 + 0], x1 = p.x[r * 3 + 1], x2 = p.x[r * 3 + 2];
  const float v0 = p.v[r * 3 + 0], v1 = p.v[r * 3 + 1], v2 = p.v[r * 3 + 2];
  float nx0, nx1, nx2, nv0 = v0, nv1 = v1, nv2 = v2;
  if (VARIANT == EGNO) {
    // x <- x + phi_v(h) v + clamp(mean_j f_ij, +-100)   (basic.py:174-181)
    f4 t[4];
    node_phi_pre(t, bj, hr, lane, g);
    silu_ecl(t);
    const float phi = node_phi(t, bj, g);
    nx0 = x0 + phi * v0 + fminf(fmaxf(Fr[0] * inv, -100.f), 100.f);
    nx1 = x1 + phi * v1 + fminf(fmaxf(Fr[1] * inv, -100.f), 100.f);
    nx2 = x2 + phi * v2 + fminf(fmaxf(Fr[2] * inv, -100.f), 100.f);
  } else {
    // v <- v + cw mean_j f_ij dt ; x <- x + v dt   (gcl.py:111-119)
    nv0 = v0 + (Fr[0] * inv * p.cw) * p.dt;
    nv1 = v1 + (Fr[1] * inv * p.cw) * p.dt;
    nv2 = v2 + (Fr[2] * inv * p.cw) * p.dt;
    nx0 = x0 + nv0 * p.dt;
    nx1 = x1 + nv1 * p.dt;
    nx2 = x2 + nv2 * p.dt;
  }
  // h <- node_mlp([h, sum_j m_ij]) (+ h if recurrent)   (basic.py:182-185, gcl.py:85-95)
  f4 z[4], hn[4];
  node_hidden_pre(z, bj, hr, Mr, lane, g);
  silu_ecl(z);
  load_vp(hn, bj + OFF_VEC + V_BN2 * 64, g);
  mm64(hn, reinterpret_cast<const h8*>(bj + OFF_H16N + H_WN2 * 4096), bj + OFF_WN2, z, lane, h16_us(bj + OFF_SCAL, HS_N + H_WN2));
  if (VARIANT == SEGNO && p.recurrent) {   // gcl.py:93-94
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) hn[mt] += hr[mt];
  }
  if (rvalid) {
    store_ecl(p.h_out + r * HID, hn, g);
    if (g == 0) {
      float* xo = p.x_out + r * 3;
      xo[0] = nx0; xo[1] = nx1; xo[2] = nx2;
      if (VARIANT == SEGNO) {
        float* vo = p.v_out + r * 3;
        vo[0] = nv0; vo[1] = nv1; vo[2] = nv2;
      }
    }
  }
}

template <int VARIANT>
int launch_graph_layer(const GraphArgs& a, hipStream_t s) {
  const int node_blocks = (a.n_total + 63) / 64;
  const int tpf = (a.n_nodes + 15) / 16;
  const int edge_blocks = (int)(((long long)a.n_frames * tpf + 3) / 4);
  hipLaunchKernelGGL(graph_proj_kernel, dim3(node_blocks), dim3(256), 0, s, a);
  if (int rc = check_launch("graph_proj_kernel")) return rc;
  if (a.ne <= 3) hipLaunchKernelGGL((graph_edge_kernel<VARIANT, 1>), dim3(edge_blocks), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((graph_edge_kernel<VARIANT, 2>), dim3(edge_blocks), dim3(256), 0, s, a);
  if (int rc = check_launch("graph_edge_kernel")) return rc;
  hipLaunchKernelGGL(graph_node_kernel<VARIANT>, dim3(node_blocks), dim3(256), 0, s, a);
  return check_launch("graph_node_kernel");
}

}  // namespace

namespace nonode_tu {

size_t graph_layer_ws_floats(long long n_total) { return (size_t)n_total * GRAPH_WS_ROW; }

int graph_scan(int n, int* cnt, int* row_ptr, hipStream_t s) {
  hipLaunchKernelGGL(graph_scan_kernel, dim3(1), dim3(1024), 0, s, n, cnt, row_ptr);
  return check_launch("graph_scan_kernel");
}

int graph_layer(int variant, int n_frames, int n_nodes, long long E, int ne, int ef_frames, const float* h,
                const float* x, const float* v, const float* ef, const float* blob, const int* row_ptr,
                const int* col, const int* eid, float dt, float cw, int recurrent, float* h_out, float* x_out,
                float* v_out, float* ws, hipStream_t s) {
  const long long n_total = (long long)n_frames * n_nodes;
  if (n_frames <= 0 || n_nodes <= 0 || n_total > (1ll << 30) || E < 0 || E >= (1ll << 31) || ne < 0 || ne > 4 ||
      ef_frames <= 0)
    return fail(NONODE_EUNSUPPORTED, "egnn_layer_graph: n_frames=%d n_nodes=%d E=%lld ne=%d ef_frames=%d", n_frames,
                n_nodes, E, ne, ef_frames);
  GraphArgs a;
  a.n_frames = n_frames; a.n_nodes = n_nodes; a.n_total = (int)n_total; a.ne = ne; a.ef_frames = ef_frames;
  a.recurrent = recurrent; a.E = E;
  a.h = h; a.x = x; a.v = v; a.ef = ne ? ef : blob; a.blob = blob;
  a.row_ptr = row_ptr; a.col = col; a.eid = eid;
  const size_t n = (size_t)n_total;
  a.P = ws; a.Q = ws + n * HID; a.M = ws + 2 * n * HID; a.F = ws + 3 * n * HID;
  a.h_out = h_out; a.x_out = x_out; a.v_out = v_out;
  a.dt = dt; a.cw = cw;
  if (variant == NONODE_VARIANT_EGNO) return launch_graph_layer<EGNO>(a, s);
  if (variant == NONODE_VARIANT_SEGNO) return launch_graph_layer<SEGNO>(a, s);
  return fail(NONODE_EINVAL, "egnn_layer_graph: variant %d", variant);
}

}  // namespace nonode_tu

extern "C" {

size_t nonode_graph_workspace_bytes(long long E, int n_nodes) {
  if (E < 0 || n_nodes < 0) return 0;
  return ((size_t)n_nodes + 1 + 2 * (size_t)E) * sizeof(int);
}

int nonode_graph_build(const void* rows, const void* cols, int idx_bytes, long long E, int n_nodes, int* row_ptr,
                       int* col, int* eid, int* flag, void* workspace, size_t workspace_bytes, void* stream) {
  if (E < 0 || E >= (1ll << 31) || n_nodes <= 0 || (idx_bytes != 4 && idx_bytes != 8))
    return fail(NONODE_EINVAL, "graph_build: E=%lld n_nodes=%d idx_bytes=%d", E, n_nodes, idx_bytes);
  if (!row_ptr || !flag || !workspace || (E > 0 && (!rows || !cols || !col || !eid)))
    return fail(NONODE_EINVAL, "graph_build: null pointer");
  if (workspace_bytes < nonode_graph_workspace_bytes(E, n_nodes))
    return fail(NONODE_EINVAL, "graph_build: workspace %zu < %zu", workspace_bytes,
                nonode_graph_workspace_bytes(E, n_nodes));
  hipStream_t s = (hipStream_t)stream;
  int* cnt = (int*)workspace;
  int* tcol = cnt + n_nodes + 1;
  int* teid = tcol + E;
  if (hipMemsetAsync(cnt, 0, ((size_t)n_nodes + 1) * sizeof(int), s) != hipSuccess)
    return fail(NONODE_ELAUNCH, "graph_build: memset");
  const unsigned eb = (unsigned)((E + 255) / 256);
  if (E > 0) {
    if (idx_bytes == 8)
      hipLaunchKernelGGL(graph_count_kernel<long long>, dim3(eb), dim3(256), 0, s, (const long long*)rows,
                         (const long long*)cols, E, n_nodes, cnt, flag);
    else
      hipLaunchKernelGGL(graph_count_kernel<int>, dim3(eb), dim3(256), 0, s, (const int*)rows, (const int*)cols, E,
                         n_nodes, cnt, flag);
    if (int rc = check_launch("graph_count_kernel")) return rc;
  }
  hipLaunchKernelGGL(graph_scan_kernel, dim3(1), dim3(1024), 0, s, n_nodes, cnt, row_ptr);
  if (int rc = check_launch("graph_scan_kernel")) return rc;
  if (E == 0) return NONODE_OK;
  if (idx_bytes == 8)
    hipLaunchKernelGGL(graph_fill_kernel<long long>, dim3(eb), dim3(256), 0, s, (const long long*)rows,
                       (const long long*)cols, E, n_nodes, cnt, tcol, teid);
  else
    hipLaunchKernelGGL(graph_fill_kernel<int>, dim3(eb), dim3(256), 0, s, (const int*)rows, (const int*)cols, E,
                       n_nodes, cnt, tcol, teid);
  if (int rc = check_launch("graph_fill_kernel")) return rc;
  hipLaunchKernelGGL(graph_sort_kernel, dim3((n_nodes + 3) / 4), dim3(256), 0, s, n_nodes, row_ptr, tcol, teid, col, eid);
  return check_launch("graph_sort_kernel");
}

size_t nonode_egnn_layer_graph_workspace_bytes(int n_frames, int n_nodes) {
  if (n_frames <= 0 || n_nodes <= 0) return 0;
  return nonode_tu::graph_layer_ws_floats((long long)n_frames * n_nodes) * sizeof(float);
}

int nonode_egnn_layer_graph(int variant, int n_frames, int n_nodes, long long E, int n_edge_feat, int ef_frames,
                            const float* h, const float* x, const float* v, const float* edge_fea, const float* blob,
                            const int* row_ptr, const int* col, const int* eid, float dt, float coords_weight,
                            int recurrent, float* h_out, float* x_out, float* v_out, void* workspace,
                            size_t workspace_bytes, void* stream) {
  if (!h || !x || !v || !blob || !row_ptr || !h_out || !x_out || !workspace ||
      (E > 0 && (!col || !eid || (n_edge_feat > 0 && !edge_fea))))
    return fail(NONODE_EINVAL, "egnn_layer_graph: null pointer");
  if (h_out == h || x_out == x) return fail(NONODE_EINVAL, "egnn_layer_graph: outputs may not alias inputs");
  if (variant == NONODE_VARIANT_SEGNO && (!v_out || v_out == v))
    return fail(NONODE_EINVAL, "egnn_layer_graph: SEGNO needs a distinct v_out");
  if (n_frames > 0 && n_nodes > 0 && workspace_bytes < nonode_egnn_layer_graph_workspace_bytes(n_frames, n_nodes))
    return fail(NONODE_EINVAL, "egnn_layer_graph: workspace too small");
  return nonode_tu::graph_layer(variant, n_frames, n_nodes, E, n_edge_feat, ef_frames, h, x, v, edge_fea, blob, row_ptr,
                                col, eid, dt, coords_weight, recurrent, h_out, x_out, v_out, (float*)workspace,
                                (hipStream_t)stream);
}

}  // extern "C"
