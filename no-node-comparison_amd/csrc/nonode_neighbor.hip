// Neighbour graphs built on the device, and featurisation on an explicit edge list: what a rollout on
// a k-NN / cut-off graph needs every segment (the reference builds only fully connected graphs, so
// nothing here stands in for reference code but the featurisation's arithmetic,
// main_simulation_simple_no.py:311-339 / train_nbody.py:222-234, on the pairs a list names).
//
// A translation unit of its own (default machine scheduler). Every distance is computed with
// individually rounded f32 operations, so a numpy restatement gives the same bits and the graph is a
// pure function of the positions. Floating-point contraction is switched off for the whole unit by the
// pragma below: HIP's default is -ffp-contract=fast, and this toolchain's __fmul_rn / __fadd_rn are
// plain * and + inside a header compiled with contraction on, which the backend fuses into v_fmac_f32
// even here: so the arithmetic below is written with the plain operators, under the pragma
// (tests/test_gpu_neighbor.py has senders whose unfused distances tie and whose fused ones do not).
//
//   neighbor_select_kernel  one wave per receiver: the min(k, candidates) smallest candidates under
//                           the total order (d2, j), kept sorted across the 64 lanes; the row written
//                           by ascending sender at a fixed pitch, and its degree
//   cell_bbox / _count / _fill_kernel, neighbor_select_cells_kernel  the same rows under a finite cut-off from
//                           a cell list (nonode_neighbor_graph_cells): each graph's nodes binned into a
//                           uniform grid and sorted by cell, one wave per receiver over the cells its cut-off
//                           box touches
//   neighbor_select_knn_cells_kernel  the same rows for ANY r2_max (+inf: the pure k-NN graph) from the same cell
//                           list (nonode_neighbor_graph_knn_cells): a box of cells that holds k other nodes bounds
//                           the k-th distance, and the cut-off search with that bound finds the rest
//                           (every search: candidate_key, topk_chunk; both cell searches: walk_segments)
//   (scan)                  row_ptr = exclusive prefix sum of the degrees (nonode_graph.hip's
//                           one-workgroup scan)
//   neighbor_compact_kernel fixed-pitch rows -> CSR (col, rows, eid), and the -1 tail
//   sender_count / _fill / _sort_kernel  the same graph as a CSR by sender (what the reverse pass of the
//                           graph layer walks), from the padded list and its device-side count: integer
//                           atomics count and claim slots, a rank sort per sender then orders each row
//                           by position, so the result is bitwise reproducible
//   node_features_kernel   the node side of prepare_inputs (frame choice, |v|, q, per-graph mean)
//   edge_features_kernel    [q_r q_c, |x_r - x_c|^2] per listed edge below a device-side count
//
// A batch is B graphs of N consecutive rows, or graphs of mixed sizes named by graph_ptr [G + 1] (the prefix
// sum of the sizes) and graph_of [n_total] (the *_ragged entries): the same kernels, which take a graph's
// bounds from graph_rows (nonode_common.h) where the equal-size call divides.
#include "nonode_common.h"

#include <algorithm>

#pragma clang fp contract(off)

#include "nonode_cells.h"

namespace {

typedef unsigned long long u64;
constexpr u64 KEY_NONE = ~0ull;   // a non-candidate: above every (d2, j) key

__device__ __forceinline__ u64 shfl64(u64 v, int src) {
  const unsigned lo = (unsigned)__shfl((int)(unsigned)v, src);
  const unsigned hi = (unsigned)__shfl((int)(unsigned)(v >> 32), src);
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 shfl_up64(u64 v) {   // lane l takes lane l - 1's value (lane 0 keeps its own)
  const unsigned lo = (unsigned)__shfl_up((int)(unsigned)v, 1);
  const unsigned hi = (unsigned)__shfl_up((int)(unsigned)(v >> 32), 1);
  return ((u64)hi << 32) | lo;
}
// stages j = from, from/2 .. 1 of a bitonic network; the 64-lane block that lane belongs to at size
// `blk` sorts ascending when (lane & blk) == 0 (blk = 64: all lanes ascending)
__device__ __forceinline__ u64 bitonic_stages(u64 v, int lane, int blk, int from) {
  const bool up = (lane & blk) == 0;
  for (int j = from; j > 0; j >>= 1) {
    const u64 o = shfl64(v, lane ^ j);
    const bool lower = (lane & j) == 0;
    const u64 mn = v < o ? v : o, mx = v < o ? o : v;
    v = (lower == up) ? mn : mx;
  }
  return v;
}
// the wave's 64 keys, ascending by lane
__device__ __forceinline__ u64 bitonic_sort(u64 v, int lane) {
  for (int blk = 2; blk <= 64; blk <<= 1) v = bitonic_stages(v, lane, blk, blk >> 1);
  return v;
}

// d2 = ((d0 d0) + (d1 d1)) + (d2 d2), every operation rounded to f32 on its own
__host__ __device__ __forceinline__ float dist2(float a0, float a1, float a2, float b0, float b1, float b2) {
  const float d0 = a0 - b0, d1 = a1 - b1, d2 = a2 - b2;
  return ((d0 * d0) + (d1 * d1)) + (d2 * d2);
}
// THE key of sender j (index inside its graph) at distance d2 from receiver i: the total order (d2, j) every search
// keeps the smallest of; KEY_NONE for a non-candidate (the receiver itself, a distance above r2_max or NaN).
// d2 >= +0 where the compare holds (a NaN fails it), so its bits order as an unsigned integer.
__host__ __device__ __forceinline__ u64 candidate_key(float d2, int j, int i, float r2_max) {
  return j != i && d2 <= r2_max ? ((u64)__builtin_bit_cast(unsigned, d2) << 32) | (unsigned)j : KEY_NONE;
}

// The keep-the-k-smallest body both searches share. Lane l of `best` holds the l-th smallest key seen so far
// (ascending). Of a chunk of 64 candidate keys (KEY_NONE: none in that lane) only the keys below the kk-th
// best matter (that bound only falls, so a key at or above it never reaches the final kk): none, the chunk is
// skipped; a few (INSERT_MAX), each is inserted at its rank (one ballot, one lane shift); more, the chunk is
// sorted and merged in. The keys of a row are distinct, so what `best` ends as is the kk smallest of the set
// of keys fed in, whatever the order and the chunking they came in.
constexpr int INSERT_MAX = 8;
__device__ __forceinline__ void topk_chunk(u64& best, u64 key, int kk, int lane) {
  const u64 kth = shfl64(best, kk - 1);
  u64 below = __ballot(key < kth);
  if (!below) return;
  if (__popcll(below) <= INSERT_MAX) {
    while (below) {   // (wave-uniform)
      const u64 nk = shfl64(key, __ffsll((long long)below) - 1);
      below &= below - 1;
      const int pos = __popcll(__ballot(best < nk));
      const u64 up = shfl_up64(best);
      best = lane < pos ? best : (lane == pos ? nk : up);
    }
    return;
  }
  key = bitonic_sort(key, lane);
  // best ascending, the chunk descending: the lane-wise minimum holds the 64 smallest of the 128
  // as a bitonic sequence, which one merge pass sorts
  const u64 rev = shfl64(key, 63 - lane);
  best = bitonic_stages(best < rev ? best : rev, lane, 64, 32);
}
// the row of receiver r from its kk best keys: the kept senders by ascending index at tmp [n_total][pitch]
// (global index), and the degree
__device__ __forceinline__ void topk_write(u64 best, int kk, int lane, int r, int g0, int pitch,
                                           int* __restrict__ tmp, int* __restrict__ deg) {
  const bool kept = lane < kk && best != KEY_NONE;
  const int d = __popcll(__ballot(kept));
  // the kept senders by ascending index (the sentinel sorts last)
  u64 byj = kept ? (u64)(unsigned)best : KEY_NONE;
  byj = bitonic_sort(byj, lane);
  if (lane < d) tmp[(size_t)r * pitch + lane] = g0 + (int)(unsigned)byj;
  if (lane == 0) deg[r] = d;
}

// The graph of node r: graph_of null, equal sizes (graph gi = r / n_each, rows gi n_each .. + n_each); otherwise
// graph gi = graph_of[r] of n_graphs, rows graph_ptr[gi] .. graph_ptr[gi + 1] (graph_rows holds them to [0, n_total]).
struct NodeGraph {
  int gi, g0, n;
};
__device__ __forceinline__ NodeGraph node_graph(int r, int n_total, int n_each, int n_graphs,
                                                const int* __restrict__ graph_ptr, const int* __restrict__ graph_of) {
  if (!graph_of) return NodeGraph{r / n_each, (r / n_each) * n_each, n_each};
  const int gi = imin(imax(graph_of[r], 0), n_graphs - 1);
  const GraphRows gr = graph_rows(graph_ptr, gi, 0, n_total);
  return NodeGraph{gi, gr.r0, gr.n};
}

// The receiver of a wave, r = g0 + i of graph gi (N rows from g0 on), kk = min(k, N - 1) held to the pitch, so
// nothing leaves x, tmp or deg whatever the descriptor says. gi, g0, N and kk are wave-uniform, in scalar registers.
struct Receiver {
  int r, gi, g0, N, kk, i;
  float x[3];   // its coordinates
};
// everything but the coordinates. False: a graph of one node, the row's degree 0 is written, the wave is done.
__device__ __forceinline__ bool receiver_rows(Receiver& rc, int r, int lane, int n_total, int n_each, int k, int pitch,
                                              int n_graphs, const int* __restrict__ graph_ptr,
                                              const int* __restrict__ graph_of, int* __restrict__ deg) {
  const NodeGraph ng = node_graph(r, n_total, n_each, n_graphs, graph_ptr, graph_of);
  rc.r = r;
  rc.gi = __builtin_amdgcn_readfirstlane(ng.gi);
  rc.g0 = __builtin_amdgcn_readfirstlane(ng.g0);
  rc.N = __builtin_amdgcn_readfirstlane(ng.n);
  rc.kk = imin(imin(k, rc.N - 1), pitch);
  rc.i = r - rc.g0;
  if (rc.kk > 0) return true;
  if (lane == 0) deg[r] = 0;
  return false;
}

// One wave per receiver, striding over all N nodes of its graph (the brute-force search: any r2_max, +inf
// included); the chunks go through topk_chunk.
// tmp [n_total][pitch]: the row's senders (global index) ascending; deg [n_total].
__global__ __launch_bounds__(256) void neighbor_select_kernel(int n_total, int n_each, int k, int pitch, float r2_max,
                                                              int n_graphs, const int* __restrict__ graph_ptr,
                                                              const int* __restrict__ graph_of,
                                                              const float* __restrict__ x, int* __restrict__ tmp,
                                                              int* __restrict__ deg) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n_total) return;   // (wave-uniform)
  Receiver rc;
  if (!receiver_rows(rc, r, lane, n_total, n_each, k, pitch, n_graphs, graph_ptr, graph_of, deg)) return;
  const float xi0 = x[(size_t)r * 3 + 0], xi1 = x[(size_t)r * 3 + 1], xi2 = x[(size_t)r * 3 + 2];
  u64 best = KEY_NONE;
  for (int base = 0; base < rc.N; base += 64) {
    const int j = base + lane;
    u64 key = KEY_NONE;
    if (j < rc.N && j != rc.i) {   // (its own row is not read)
      const size_t s = (size_t)(rc.g0 + j) * 3;
      key = candidate_key(dist2(xi0, xi1, xi2, x[s + 0], x[s + 1], x[s + 2]), j, rc.i, r2_max);
    }
    topk_chunk(best, key, rc.kk, lane);
  }
  topk_write(best, rc.kk, lane, r, rc.g0, pitch, tmp, deg);
}

// ---- the cell-list search (a finite r2_max): the same rows from the cells a receiver's cut-off box touches ----
// nonode_cells.h has the grid rule, the binning function, the search box and why they miss no candidate.
// Graph gi of a batch (rows g0 .. g0 + N) owns the N + 1 entries from g0 + gi on of one table of
// n_total + n_graphs entries: its g^3 <= N / CELL_FILL cells, z fastest, then the bucket of its non-finite
// nodes. Counts and slot claims are integer atomics, so the order of the nodes inside a cell differs from run
// to run; that cannot show in the result, as a row is the top k of a SET of keys under a total order
// (topk_chunk), then sorted by sender. Every index below is held inside its array whatever the descriptor says.

// bb [n_graphs][6], zero before: every graph's bounding box over its finite nodes as integer-ordered maxima
// (cell_grid reads it back). A wave whose 64 nodes belong to one graph reduces first and sends six atomics.
__global__ __launch_bounds__(256) void cell_bbox_kernel(int n_total, int n_each, int n_graphs,
                                                        const int* __restrict__ graph_ptr,
                                                        const int* __restrict__ graph_of, const float* __restrict__ x,
                                                        unsigned* bb) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r - (int)(threadIdx.x & 63) >= n_total) return;   // (wave-uniform: lane 0 holds a node below)
  unsigned m[6] = {0u, 0u, 0u, 0u, 0u, 0u};   // 0: below every finite key
  int gi = -1;
  if (r < n_total) {
    gi = node_graph(r, n_total, n_each, n_graphs, graph_ptr, graph_of).gi;
    const float x0 = x[(size_t)r * 3 + 0], x1 = x[(size_t)r * 3 + 1], x2 = x[(size_t)r * 3 + 2];
    if (cell_finite(x0, x1, x2)) {
      m[3] = cell_key(x0); m[4] = cell_key(x1); m[5] = cell_key(x2);
      m[0] = ~m[3]; m[1] = ~m[4]; m[2] = ~m[5];
    }
  }
  const int gf = __builtin_amdgcn_readfirstlane(gi);
  if (__all(gi == gf || gi < 0)) {
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const unsigned t = (unsigned)__shfl_xor((int)m[a], o);
        m[a] = m[a] > t ? m[a] : t;
      }
    }
    if ((threadIdx.x & 63) != 0) return;
  }
  if (gi < 0) return;
#pragma unroll
  for (int a = 0; a < 6; ++a)
    if (m[a]) atomicMax(bb + (size_t)gi * 6 + a, m[a]);
}

// bucket[r] = the table entry of node r (its cell, or its graph's trailing bucket), counted in cnt
__global__ __launch_bounds__(256) void cell_count_kernel(int n_total, int n_each, int n_graphs, float rr,
                                                         const int* __restrict__ graph_ptr,
                                                         const int* __restrict__ graph_of, const float* __restrict__ x,
                                                         const unsigned* __restrict__ bb, int* cnt,
                                                         int* __restrict__ bucket) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n_total) return;
  const NodeGraph ng = node_graph(r, n_total, n_each, n_graphs, graph_ptr, graph_of);
  const CellGrid cg = cell_grid(bb + (size_t)ng.gi * 6, ng.n, rr);
  const float x0 = x[(size_t)r * 3 + 0], x1 = x[(size_t)r * 3 + 1], x2 = x[(size_t)r * 3 + 2];
  int c = cg.g * cg.g * cg.g;
  if (cell_finite(x0, x1, x2))
    c = (cell_of(x0, cg.lo[0], cg.inv_w[0], cg.g) * cg.g + cell_of(x1, cg.lo[1], cg.inv_w[1], cg.g)) * cg.g +
        cell_of(x2, cg.lo[2], cg.inv_w[2], cg.g);
  const int idx = imin(ng.g0 + ng.gi + c, n_total + n_graphs - 1);
  bucket[r] = idx;
  atomicAdd(cnt + idx, 1);
}
// every node takes the next free slot of its bucket (cursor: the scan of the counts): sorted [n_total] =
// (x, y, z, the node's row index as bits), every node exactly once
__global__ __launch_bounds__(256) void cell_fill_kernel(int n_total, const float* __restrict__ x,
                                                        const int* __restrict__ bucket, int* cursor,
                                                        f4* __restrict__ sorted) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n_total) return;
  const int slot = atomicAdd(cursor + bucket[r], 1);
  if (slot >= 0 && slot < n_total)
    sorted[slot] = f4{x[(size_t)r * 3 + 0], x[(size_t)r * 3 + 1], x[(size_t)r * 3 + 2], __int_as_float(r)};
}

// Both searches on the cell list run one wave per receiver, taken in sorted order (neighbouring waves walk the same
// cells), the receiver and its coordinates from the wave's slot. Their preamble is receiver_rows' written out in
// each kernel: behind a function that returns whether to go on, both kernels measured 0.1 - 0.3 % slower from
// 10,000 nodes on; written out they take the parent's time.

// THE candidate walk: nseg segments of the sorted order, segment u = sorted[p .. e) from seg(u, p, e) (p = e = 0
// before: an empty one). A segment holds about a third of a wave at cut-off-wide cells, so the 64 lanes take several
// at once: groups of 16 lanes (32 with two or three segments, all 64 with one) each stride over one segment, and every
// round's 64 keys are one chunk of topk_chunk. Same dist2 and key as neighbor_select_kernel.
template <class Seg>
__device__ __forceinline__ void walk_segments(u64& best, int nseg, Seg seg, const Receiver& rc, int n_total, int lane,
                                              float r2_max, const f4* __restrict__ sorted) {
  const int sh = nseg >= 4 ? 4 : (nseg >= 2 ? 5 : 6);   // log2 of the lanes per segment
  const int grp = lane >> sh, sub = lane & ((1 << sh) - 1);
  for (int u0 = 0; u0 < nseg; u0 += 64 >> sh) {
    const int u = u0 + grp;
    int p = 0, e = 0;
    if (u < nseg) seg(u, p, e);
    p += sub;
    e = imin(e, n_total);
    while (__any(p < e)) {
      u64 key = KEY_NONE;
      if (p >= 0 && p < e) {
        const f4 o = sorted[p];
        key = candidate_key(dist2(rc.x[0], rc.x[1], rc.x[2], o[0], o[1], o[2]), __float_as_int(o[3]) - rc.g0, rc.i,
                            r2_max);
      }
      topk_chunk(best, key, rc.kk, lane);
      p += 1 << sh;
    }
  }
}
// A graph's part of cell_start (entries tab on, held below last). With z the fastest cell index, the cells
// (cx, cy, z_lo .. z_hi) of a box are one run of the sorted order: cell_start[first cell] .. cell_start[last cell + 1].
struct CellTable {
  const int* __restrict__ cell_start;
  int tab, last, g;
  __device__ __forceinline__ void cells(const CellSeg& sg, int& p, int& e) const {
    p = cell_start[imin(tab + sg.c0, last)];
    e = cell_start[imin(tab + sg.c1, last) + 1];
  }
  // every run of box b
  __device__ __forceinline__ void walk_box(u64& best, const CellBox& b, const Receiver& rc, int n_total, int lane,
                                           float r2_max, const f4* __restrict__ sorted) const {
    walk_segments(best, box_runs(b), [&](int u, int& p, int& e) { cells(box_run(b, u, g), p, e); }, rc, n_total, lane,
                  r2_max, sorted);
  }
};
__device__ __forceinline__ CellBox uniform_box(const CellBox& b) {   // the same in every lane: scalar registers
  CellBox u;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    u.lo[a] = __builtin_amdgcn_readfirstlane(b.lo[a]);
    u.hi[a] = __builtin_amdgcn_readfirstlane(b.hi[a]);
  }
  return u;
}

// The cut-off search: the runs of the receiver's cut-off box.
__global__ __launch_bounds__(256) void neighbor_select_cells_kernel(
    int n_total, int n_each, int k, int pitch, float r2_max, float rr, int n_graphs, const int* __restrict__ graph_ptr,
    const int* __restrict__ graph_of, const f4* __restrict__ sorted, const int* __restrict__ cell_start,
    const unsigned* __restrict__ bb, int* __restrict__ tmp, int* __restrict__ deg) {
  const int lane = threadIdx.x & 63;
  const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= n_total) return;   // (wave-uniform)
  const f4 me = sorted[s];
  const int r = __builtin_amdgcn_readfirstlane(__float_as_int(me[3]));
  if (r < 0 || r >= n_total) return;   // (the fill wrote every slot: never)
  const NodeGraph ng = node_graph(r, n_total, n_each, n_graphs, graph_ptr, graph_of);
  Receiver rc;
  rc.r = r;
  rc.g0 = __builtin_amdgcn_readfirstlane(ng.g0); rc.N = __builtin_amdgcn_readfirstlane(ng.n);
  rc.gi = __builtin_amdgcn_readfirstlane(ng.gi);
  rc.kk = imin(imin(k, rc.N - 1), pitch); rc.i = r - rc.g0;
  if (rc.kk <= 0) {   // a graph of one node: no pair
    if (lane == 0) deg[r] = 0;
    return;
  }
  rc.x[0] = me[0]; rc.x[1] = me[1]; rc.x[2] = me[2];
  if (!cell_finite(rc.x[0], rc.x[1], rc.x[2])) {   // a non-finite receiver: no pair
    if (lane == 0) deg[rc.r] = 0;
    return;
  }
  const CellGrid cg = cell_grid(bb + (size_t)rc.gi * 6, rc.N, rr);
  const CellTable ct{cell_start, rc.g0 + rc.gi, n_total + n_graphs - 1, cg.g};
  u64 best = KEY_NONE;
  ct.walk_box(best, uniform_box(cell_box(cg, rc.x[0], rc.x[1], rc.x[2], rr)), rc, n_total, lane, r2_max, sorted);
  topk_write(best, rc.kk, lane, rc.r, rc.g0, pitch, tmp, deg);
}

// ---- the k-NN search on the cell list (any r2_max, +inf included): the radius is found per receiver ----
// nonode_cells.h has the two phases, why they are exact and when a receiver walks its whole graph instead.
// Same grid kernels as above (built with rr = 0: the width is extent / g), same walk.
// Every branch below is wave-uniform (all lanes hold the same receiver).
__global__ __launch_bounds__(256) void neighbor_select_knn_cells_kernel(
    int n_total, int n_each, int k, int pitch, float r2_max, int n_graphs, const int* __restrict__ graph_ptr,
    const int* __restrict__ graph_of, const f4* __restrict__ sorted, const int* __restrict__ cell_start,
    const unsigned* __restrict__ bb, int* __restrict__ tmp, int* __restrict__ deg) {
  const int lane = threadIdx.x & 63;
  const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= n_total) return;   // (wave-uniform)
  const f4 me = sorted[s];
  const int r = __builtin_amdgcn_readfirstlane(__float_as_int(me[3]));
  if (r < 0 || r >= n_total) return;   // (the fill wrote every slot: never)
  const NodeGraph ng = node_graph(r, n_total, n_each, n_graphs, graph_ptr, graph_of);
  Receiver rc;
  rc.r = r;
  rc.g0 = __builtin_amdgcn_readfirstlane(ng.g0); rc.N = __builtin_amdgcn_readfirstlane(ng.n);
  rc.gi = __builtin_amdgcn_readfirstlane(ng.gi);
  rc.kk = imin(imin(k, rc.N - 1), pitch); rc.i = r - rc.g0;
  if (rc.kk <= 0) {   // a graph of one node: no pair
    if (lane == 0) deg[r] = 0;
    return;
  }
  rc.x[0] = me[0]; rc.x[1] = me[1]; rc.x[2] = me[2];
  const float xi0 = rc.x[0], xi1 = rc.x[1], xi2 = rc.x[2];
  const int kk = rc.kk;
  u64 best = KEY_NONE;
  bool whole = !cell_finite(xi0, xi1, xi2) || kk >= rc.N - 1;
  if (!whole) {
    const CellGrid cg = cell_grid(bb + (size_t)rc.gi * 6, rc.N, 0.f);
    const int g = cg.g;
    const CellTable ct{cell_start, rc.g0 + rc.gi, n_total + n_graphs - 1, g};
    const int c0 = __builtin_amdgcn_readfirstlane(cell_of(xi0, cg.lo[0], cg.inv_w[0], g));
    const int c1 = __builtin_amdgcn_readfirstlane(cell_of(xi1, cg.lo[1], cg.inv_w[1], g));
    const int c2 = __builtin_amdgcn_readfirstlane(cell_of(xi2, cg.lo[2], cg.inv_w[2], g));
    // phase 1: the shell box, grown until it holds kk nodes beside the receiver (or is the grid; hw <= g)
    CellBox b1;
    for (int hw = 1;; ++hw) {
      b1 = shell_box(c0, c1, c2, hw, g);
      if (box_covers_grid(b1, g)) break;
      int cnt = 0;
      for (int u = lane; u < box_runs(b1); u += 64) {
        int p, e;
        ct.cells(box_run(b1, u, g), p, e);
        cnt += e - p;
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
      if (__builtin_amdgcn_readfirstlane(cnt) - 1 >= kk) break;
    }
    ct.walk_box(best, b1, rc, n_total, lane, r2_max, sorted);
    // phase 2: what the cut-off search with r2 = D walks outside the shell box
    const u64 kth = shfl64(best, kk - 1);
    const float D = kth != KEY_NONE ? __uint_as_float((unsigned)(kth >> 32)) : r2_max;
    float rr = 0.f;
    if (!cell_finite(D) || !knn_rr(D, &rr)) {
      whole = true;
    } else {
      const CellBox b2 = uniform_box(cell_box(cg, xi0, xi1, xi2, rr));
      if (!box_inside(b2, b1))
        walk_segments(best, 2 * box_runs(b2), [&](int u, int& p, int& e) {
          const CellSeg sg = box_run_outside(b2, b1, u >> 1, u & 1, g);
          if (sg.c0 <= sg.c1) ct.cells(sg, p, e);
        }, rc, n_total, lane, r2_max, sorted);
    }
  }
  if (whole) {   // the brute-force search on the graph's run of the sorted order, its non-finite bucket included
    best = KEY_NONE;
    walk_segments(best, 1, [&](int, int& p, int& e) { p = rc.g0; e = rc.g0 + rc.N; }, rc, n_total, lane, r2_max,
                  sorted);
  }
  topk_write(best, kk, lane, rc.r, rc.g0, pitch, tmp, deg);
}

// thread t = r pitch + l of the n_total pitch fixed-pitch slots: entry l of row r moves to row_ptr[r] + l;
// position t of the outputs, when it is at or past the edge count, gets the tail's (-1, -1, t). The
// outputs hold cap <= n_total pitch entries (equal sizes: cap = n_total pitch) and no store leaves [0, cap).
__global__ __launch_bounds__(256) void neighbor_compact_kernel(long long cap, int n_total, int pitch,
                                                               const int* __restrict__ row_ptr,
                                                               const int* __restrict__ tmp, int* __restrict__ col,
                                                               int* __restrict__ eid, int* __restrict__ rows) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)n_total * pitch) return;
  const int r = (int)(t / pitch), l = (int)(t - (long long)r * pitch);
  const int p0 = row_ptr[r], d = row_ptr[r + 1] - p0;
  const long long p = (long long)p0 + l;
  if (l < d && p >= 0 && p < cap) {
    col[p] = tmp[t];
    rows[p] = r;
    eid[p] = (int)p;
  }
  if (t >= row_ptr[n_total] && t < cap) {
    col[t] = -1;
    rows[t] = -1;
    eid[t] = (int)t;
  }
}

// The node side of prepare_inputs, one 256-thread block per graph (graph_rows: N rows each, or the batch's
// own graph_ptr): frame t_in[b] - 1 (python index; null: the last frame) of loc, vel [F][n_total][3] ->
// x, v [n_total][3], nodes = [|v|] or [|v|, q], loc_mean [n_total][3]. The mean's sum is a fixed tree
// (per-thread strided partial sums, then halving in LDS) that depends on the graph's size alone.
__global__ __launch_bounds__(256) void node_features_kernel(int n_total, int n_each, int F,
                                                            const int* __restrict__ graph_ptr,
                                                            const float* __restrict__ loc,
                                                            const float* __restrict__ vel, const int* __restrict__ t_in,
                                                            const float* __restrict__ q, float* __restrict__ x_out,
                                                            float* __restrict__ v_out, float* __restrict__ nodes,
                                                            float* __restrict__ loc_mean) {
  __shared__ float part[3][256];
  const int b = blockIdx.x, tid = threadIdx.x;
  int f = F - 1;
  if (t_in) f = ((t_in[b] - 1) % F + F) % F;
  const GraphRows gr = graph_rows(graph_ptr, b, n_each, n_total);
  const int N = gr.n;
  const size_t BN = (size_t)n_total, r0 = (size_t)gr.r0;
  const float* lf = loc + ((size_t)f * BN + r0) * 3;
  const float* vf = vel + ((size_t)f * BN + r0) * 3;
  const int nn = q ? 2 : 1;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  for (int i = tid; i < N; i += 256) {
    const size_t r = r0 + i;
    const float x0 = lf[i * 3 + 0], x1 = lf[i * 3 + 1], x2 = lf[i * 3 + 2];
    const float v0 = vf[i * 3 + 0], v1 = vf[i * 3 + 1], v2 = vf[i * 3 + 2];
    x_out[r * 3 + 0] = x0; x_out[r * 3 + 1] = x1; x_out[r * 3 + 2] = x2;
    v_out[r * 3 + 0] = v0; v_out[r * 3 + 1] = v1; v_out[r * 3 + 2] = v2;
    nodes[r * nn] = sqrtf(((v0 * v0) + (v1 * v1)) + (v2 * v2));
    if (q) nodes[r * nn + 1] = q[r];
    s0 += x0; s1 += x1; s2 += x2;
  }
  part[0][tid] = s0; part[1][tid] = s1; part[2][tid] = s2;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      part[0][tid] += part[0][tid + o];
      part[1][tid] += part[1][tid + o];
      part[2][tid] += part[2][tid + o];
    }
    __syncthreads();
  }
  if (!loc_mean) return;
  const float m0 = part[0][0] / (float)N, m1 = part[1][0] / (float)N, m2 = part[2][0] / (float)N;
  for (int i = tid; i < N; i += 256) {
    const size_t r = r0 + i;
    loc_mean[r * 3 + 0] = m0; loc_mean[r * 3 + 1] = m1; loc_mean[r * 3 + 2] = m2;
  }
}

// edge_attr[p] = [q_r q_c, |x_r - x_c|^2] (without q: the distance alone) for p below the count
// (*n_edges, or cap when n_edges is null); zero at and past it, and for a pair with an index outside
// [0, n_nodes) (which the model's CSR build reports)
template <typename I>
__global__ __launch_bounds__(256) void edge_features_kernel(long long cap, int n_nodes, const I* __restrict__ rows,
                                                            const I* __restrict__ cols, const int* __restrict__ n_edges,
                                                            const float* __restrict__ x, const float* __restrict__ q,
                                                            float* __restrict__ ea) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= cap) return;
  const long long n = n_edges ? (long long)*n_edges : cap;
  float prod = 0.f, d2 = 0.f;
  if (p < n) {
    const long long r = (long long)rows[p], c = (long long)cols[p];
    if (r >= 0 && r < n_nodes && c >= 0 && c < n_nodes) {
      d2 = dist2(x[r * 3 + 0], x[r * 3 + 1], x[r * 3 + 2], x[c * 3 + 0], x[c * 3 + 1], x[c * 3 + 2]);
      if (q) prod = q[r] * q[c];
    }
  }
  if (q) {
    ea[p * 2 + 0] = prod;
    ea[p * 2 + 1] = d2;
  } else {
    ea[p] = d2;
  }
}

// ---- the same graph as a CSR by sender (the reverse pass of the graph layer) ----
// the edge count E = row_ptr[n_total], held to [0, cap]
__device__ __forceinline__ long long edge_count(const int* __restrict__ row_ptr, int n_total, long long cap) {
  const long long E = row_ptr[n_total];
  return E < 0 ? 0 : (E < cap ? E : cap);
}
// valid[p] = p < E; every entry below E counts towards its sender's out-degree (a sender outside
// [0, n_total), which neighbor_graph never writes, is skipped here and in the fill)
__global__ __launch_bounds__(256) void sender_count_kernel(long long cap, int n_total, const int* __restrict__ col,
                                                           const int* __restrict__ row_ptr, int* cnt,
                                                           int* __restrict__ valid) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= cap) return;
  const bool live = p < edge_count(row_ptr, n_total, cap);
  valid[p] = live ? 1 : 0;
  if (!live) return;
  const int c = col[p];
  if (c >= 0 && c < n_total) atomicAdd(cnt + c, 1);
}
// every entry below E takes the next free slot of its sender's row (any order: sender_sort_kernel
// orders it); seid starts as -1 everywhere, which is what its tail at and past E keeps
__global__ __launch_bounds__(256) void sender_fill_kernel(long long cap, int n_total, const int* __restrict__ col,
                                                          const int* __restrict__ row_ptr, int* cursor,
                                                          int* __restrict__ tpos, int* __restrict__ seid) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= cap) return;
  seid[p] = -1;   // (the sort, a later launch, overwrites every position a sender's row covers)
  if (p >= edge_count(row_ptr, n_total, cap)) return;
  const int c = col[p];
  if (c < 0 || c >= n_total) return;
  tpos[atomicAdd(cursor + c, 1)] = (int)p;
}
// one wave per sender: position p goes to its rank among the row's positions (all distinct), so the row
// is ascending p = (receiver, original index) whatever order the fill claimed its slots in. A row of any
// length (a hub sends to up to N - 1 receivers): 64 entries per round, each against the whole row.
__global__ __launch_bounds__(256) void sender_sort_kernel(int n_total, const int* __restrict__ srow_ptr,
                                                          const int* __restrict__ tpos, int* __restrict__ seid) {
  const int s = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (s >= n_total) return;
  const int p0 = srow_ptr[s], d = srow_ptr[s + 1] - p0;
  for (int i = lane; i < d; i += 64) {
    const int pi = tpos[p0 + i];
    int rank = 0;
    for (int m = 0; m < d; ++m) rank += tpos[p0 + m] < pi ? 1 : 0;
    seid[p0 + rank] = pi;
  }
}

long long neighbor_capacity(int B, int N, int k) { return (long long)B * N * (k < N - 1 ? k : N - 1); }

// The cell-list builder's workspace, in ints: sorted (4 n_total, first: 16-byte rows), deg, tmp (as the brute-force
// builder's), bucket (n_total), then bb (6 G) and cnt (n_total + G) side by side (one memset), cell_start
// (n_total + G + 1).
size_t cells_workspace_ints(int G, int n_total, int pitch) {
  return (size_t)n_total * (8 + (size_t)pitch) + 8 * (size_t)G + 1;
}

// The builder's launches for a batch over n_total rows whose largest graph has n_max: the workspace rows
// at the fixed pitch min(k, n_max - 1), the outputs with cap entries. graph_of null: equal sizes, every
// graph n_max rows (cap = n_total pitch); otherwise the n_graphs graphs graph_ptr / graph_of name.
// CELLS (finite r2_max) / KNN_CELLS (any r2_max; the grid of rr = 0) build the cell list before their search. Every
// grid is a function of n_total and the pitch; nothing is read back.
enum Search { BRUTE, CELLS, KNN_CELLS };
int launch_neighbor_graph(Search how, const char* who, int n_total, int n_max, int k, long long cap, float r2_max,
                          int n_graphs, const int* graph_ptr, const int* graph_of, const float* x, int* row_ptr,
                          int* col, int* eid, int* rows, void* workspace, hipStream_t s) {
  const int pitch = k < n_max - 1 ? k : n_max - 1;
  if (pitch == 0) {   // graphs of one node: no pair at all
    if (hipMemsetAsync(row_ptr, 0, ((size_t)n_total + 1) * sizeof(int), s) != hipSuccess)
      return fail(NONODE_ELAUNCH, "%s: memset", who);
    return NONODE_OK;
  }
  const dim3 per_node((n_total + 255) / 256), per_wave((n_total + 3) / 4);
  int* deg = (int*)workspace + (how == BRUTE ? 0 : 4 * (size_t)n_total);
  int* tmp = deg + n_total;
  if (how == BRUTE) {
    hipLaunchKernelGGL(neighbor_select_kernel, per_wave, dim3(256), 0, s, n_total, n_max, k, pitch, r2_max, n_graphs,
                       graph_ptr, graph_of, x, tmp, deg);
    if (int rc = check_launch("neighbor_select_kernel")) return rc;
  } else {
    f4* sorted = (f4*)workspace;
    int* bucket = tmp + (size_t)n_total * pitch;
    unsigned* bb = (unsigned*)(bucket + n_total);
    int* cnt = (int*)(bb + 6 * (size_t)n_graphs);
    int* cell_start = cnt + n_total + n_graphs;
    const float rr = how == KNN_CELLS ? 0.f : cell_rr(r2_max);
    if (hipMemsetAsync(bb, 0, (6 * (size_t)n_graphs + (size_t)n_total + n_graphs) * sizeof(int), s) != hipSuccess)
      return fail(NONODE_ELAUNCH, "%s: memset", who);
    hipLaunchKernelGGL(cell_bbox_kernel, per_node, dim3(256), 0, s, n_total, n_max, n_graphs, graph_ptr, graph_of, x,
                       bb);
    if (int rc = check_launch("cell_bbox_kernel")) return rc;
    hipLaunchKernelGGL(cell_count_kernel, per_node, dim3(256), 0, s, n_total, n_max, n_graphs, rr, graph_ptr, graph_of,
                       x, bb, cnt, bucket);
    if (int rc = check_launch("cell_count_kernel")) return rc;
    if (int rc = nonode_tu::graph_scan(n_total + n_graphs, cnt, cell_start, s)) return rc;
    hipLaunchKernelGGL(cell_fill_kernel, per_node, dim3(256), 0, s, n_total, x, bucket, cnt, sorted);
    if (int rc = check_launch("cell_fill_kernel")) return rc;
    if (how == KNN_CELLS)
      hipLaunchKernelGGL(neighbor_select_knn_cells_kernel, per_wave, dim3(256), 0, s, n_total, n_max, k, pitch, r2_max,
                         n_graphs, graph_ptr, graph_of, sorted, cell_start, bb, tmp, deg);
    else
      hipLaunchKernelGGL(neighbor_select_cells_kernel, per_wave, dim3(256), 0, s, n_total, n_max, k, pitch, r2_max, rr,
                         n_graphs, graph_ptr, graph_of, sorted, cell_start, bb, tmp, deg);
    if (int rc = check_launch(how == KNN_CELLS ? "neighbor_select_knn_cells_kernel" : "neighbor_select_cells_kernel"))
      return rc;
  }
  if (int rc = nonode_tu::graph_scan(n_total, deg, row_ptr, s)) return rc;
  const long long slots = (long long)n_total * pitch;
  hipLaunchKernelGGL(neighbor_compact_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, s, cap, n_total,
                     pitch, row_ptr, tmp, col, eid, rows);
  return check_launch("neighbor_compact_kernel");
}

// The host diagnostics' graph gi: its rows and its grid at radius rr, through the functions the kernels run.
struct HostGraph {
  GraphRows rows;
  CellGrid cg;
};
HostGraph host_graph(const int* graph_ptr, int gi, int n_max, int n_total, const float* x, float rr) {
  const GraphRows rows = graph_rows(graph_ptr, gi, n_max, n_total);
  unsigned bb[6] = {0u, 0u, 0u, 0u, 0u, 0u};
  for (int r = rows.r0; r < rows.r0 + rows.n; ++r) {
    const float* p = x + (size_t)r * 3;
    if (!cell_finite(p[0], p[1], p[2])) continue;
    for (int a = 0; a < 3; ++a) {
      const unsigned key = cell_key(p[a]);
      if (~key > bb[a]) bb[a] = ~key;
      if (key > bb[3 + a]) bb[3 + a] = key;
    }
  }
  return HostGraph{rows, cell_grid(bb, rows.n, rr)};
}

int launch_node_features(int n_graphs, int n_total, int n_each, int F, const int* graph_ptr, const float* loc,
                         const float* vel, const int* t_in, const float* charges, float* x_out, float* v_out,
                         float* nodes, float* loc_mean, hipStream_t s) {
  hipLaunchKernelGGL(node_features_kernel, dim3(n_graphs), dim3(256), 0, s, n_total, n_each, F, graph_ptr, loc, vel,
                     t_in, charges, x_out, v_out, nodes, loc_mean);
  return check_launch("node_features_kernel");
}

}  // namespace

extern "C" {

size_t nonode_neighbor_graph_workspace_bytes(int B, int N, int k) {
  if (B <= 0 || N <= 0 || k < 1 || k > 64) return 0;
  // the degrees, the fixed-pitch rows
  return ((size_t)B * N + (size_t)neighbor_capacity(B, N, k)) * sizeof(int);
}

int nonode_neighbor_graph(int B, int N, int k, float r2_max, const float* x, int* row_ptr, int* col, int* eid,
                          int* rows, void* workspace, size_t workspace_bytes, void* stream) {
  if (B <= 0 || N <= 0 || k < 1 || k > 64 || !(r2_max > 0.f) || (long long)B * N >= (1ll << 30) ||
      neighbor_capacity(B, N, k) >= (1ll << 31))
    return fail(NONODE_EINVAL, "neighbor_graph: B=%d N=%d k=%d r2_max=%g (k in [1, 64], r2_max > 0)", B, N, k,
                (double)r2_max);
  const long long cap = neighbor_capacity(B, N, k);
  if (!x || !row_ptr || !workspace || (cap > 0 && (!col || !eid || !rows)))
    return fail(NONODE_EINVAL, "neighbor_graph: null pointer");
  if (workspace_bytes < nonode_neighbor_graph_workspace_bytes(B, N, k))
    return fail(NONODE_EINVAL, "neighbor_graph: workspace %zu < %zu", workspace_bytes,
                nonode_neighbor_graph_workspace_bytes(B, N, k));
  return launch_neighbor_graph(BRUTE, "neighbor_graph", B * N, N, k, cap, r2_max, B, nullptr, nullptr, x, row_ptr, col,
                               eid, rows, workspace, (hipStream_t)stream);
}

size_t nonode_neighbor_graph_ragged_workspace_bytes(int n_total, int n_max, int k) {
  if (n_total <= 0 || n_max <= 0 || n_max > n_total || k < 1 || k > 64) return 0;
  // the degrees, the rows at the fixed pitch min(k, n_max - 1)
  return ((size_t)n_total + (size_t)n_total * (k < n_max - 1 ? k : n_max - 1)) * sizeof(int);
}

size_t nonode_neighbor_graph_cells_workspace_bytes(int G, int n_total, int n_max, int k) {
  if (G < 1 || n_total < G || n_total >= (1 << 30) || n_max <= 0 || n_max > n_total || k < 1 || k > 64) return 0;
  return cells_workspace_ints(G, n_total, k < n_max - 1 ? k : n_max - 1) * sizeof(int);
}

size_t nonode_neighbor_graph_knn_cells_workspace_bytes(int G, int n_total, int n_max, int k) {
  return nonode_neighbor_graph_cells_workspace_bytes(G, n_total, n_max, k);   // the same list, the same rows
}

// The host checks and the launches of the entries that take (G, ..., descriptors). CELLS wants a finite r2_max; both
// cell searches take null descriptors for equal sizes (n_total = G n_max) and a 16-byte aligned workspace.
static int neighbor_graph_entry(Search how, const char* who, int G, int n_total, int n_max, int k, long long cap,
                                float r2_max, const int* graph_ptr, const int* graph_of, const float* x,
                                int* row_ptr, int* col, int* eid, int* rows, void* workspace, size_t workspace_bytes,
                                void* stream) {
  const bool finite = how == CELLS, cells = how != BRUTE;
  const size_t need = cells ? nonode_neighbor_graph_cells_workspace_bytes(G, n_total, n_max, k)
                            : nonode_neighbor_graph_ragged_workspace_bytes(n_total, n_max, k);
  if (G < 1 || n_total < G || n_total >= (1 << 30) || n_max < 1 || n_max > n_total || k < 1 || k > 64 ||
      !(r2_max > 0.f) || (finite && !cell_finite(r2_max)) || cap < 0 || cap >= (1ll << 31) ||
      cap > (long long)n_total * (k < n_max - 1 ? k : n_max - 1))
    return fail(NONODE_EINVAL, "%s: G=%d n_total=%d n_max=%d k=%d cap=%lld r2_max=%g (k in [1, 64], r2_max > 0%s, "
                "cap <= n_total min(k, n_max - 1))", who, G, n_total, n_max, k, cap, (double)r2_max,
                finite ? " and finite" : "");
  if (cells && (graph_ptr == nullptr) != (graph_of == nullptr))
    return fail(NONODE_EINVAL, "%s: graph_ptr and graph_of go together (both null: equal sizes)", who);
  if (cells && !graph_of && (long long)G * n_max != n_total)
    return fail(NONODE_EINVAL, "%s: equal sizes need n_total = G n_max, got G=%d n_max=%d n_total=%d", who, G, n_max,
                n_total);
  if ((!cells && (!graph_ptr || !graph_of)) || !x || !row_ptr || !workspace || (cap > 0 && (!col || !eid || !rows)))
    return fail(NONODE_EINVAL, "%s: null pointer", who);
  if (cells && ((size_t)workspace & 15) != 0) return fail(NONODE_EINVAL, "%s: workspace not 16-byte aligned", who);
  if (workspace_bytes < need) return fail(NONODE_EINVAL, "%s: workspace %zu < %zu", who, workspace_bytes, need);
  return launch_neighbor_graph(how, who, n_total, n_max, k, cap, r2_max, G, graph_ptr, graph_of, x, row_ptr, col, eid,
                               rows, workspace, (hipStream_t)stream);
}

int nonode_neighbor_graph_ragged(int G, int n_total, int n_max, int k, long long cap, float r2_max,
                                 const int* graph_ptr, const int* graph_of, const float* x, int* row_ptr, int* col,
                                 int* eid, int* rows, void* workspace, size_t workspace_bytes, void* stream) {
  return neighbor_graph_entry(BRUTE, "neighbor_graph_ragged", G, n_total, n_max, k, cap, r2_max, graph_ptr, graph_of, x,
                              row_ptr, col, eid, rows, workspace, workspace_bytes, stream);
}

int nonode_neighbor_graph_cells(int G, int n_total, int n_max, int k, long long cap, float r2_max,
                                const int* graph_ptr, const int* graph_of, const float* x, int* row_ptr, int* col,
                                int* eid, int* rows, void* workspace, size_t workspace_bytes, void* stream) {
  return neighbor_graph_entry(CELLS, "neighbor_graph_cells", G, n_total, n_max, k, cap, r2_max, graph_ptr, graph_of, x,
                              row_ptr, col, eid, rows, workspace, workspace_bytes, stream);
}

int nonode_neighbor_graph_knn_cells(int G, int n_total, int n_max, int k, long long cap, float r2_max,
                                    const int* graph_ptr, const int* graph_of, const float* x, int* row_ptr, int* col,
                                    int* eid, int* rows, void* workspace, size_t workspace_bytes, void* stream) {
  return neighbor_graph_entry(KNN_CELLS, "neighbor_graph_knn_cells", G, n_total, n_max, k, cap, r2_max, graph_ptr,
                              graph_of, x, row_ptr, col, eid, rows, workspace, workspace_bytes, stream);
}

// Diagnostic (host arrays, no GPU): the grid, the binning and the search boxes of the cell-list search, from
// the very functions its kernels run (nonode_cells.h).
int nonode_debug_neighbor_cells(int G, int n_total, int n_max, float r2_max, const int* graph_ptr, const float* x,
                                float* rr_out, int* grid, float* box, int* cell, int* range) {
  if (G < 1 || n_total < G || n_max < 1 || n_max > n_total || !(r2_max > 0.f) || !cell_finite(r2_max) || !x ||
      (!graph_ptr && (long long)G * n_max != n_total))
    return fail(NONODE_EINVAL, "debug_neighbor_cells: G=%d n_total=%d n_max=%d r2_max=%g", G, n_total, n_max,
                (double)r2_max);
  const float rr = cell_rr(r2_max);
  if (rr_out) *rr_out = rr;
  for (int gi = 0; gi < G; ++gi) {
    const HostGraph hg = host_graph(graph_ptr, gi, n_max, n_total, x, rr);
    const int g0 = hg.rows.r0, n = hg.rows.n;
    const CellGrid& cg = hg.cg;
    if (grid) grid[gi] = cg.g;
    if (box)
      for (int a = 0; a < 3; ++a) {
        box[gi * 9 + a] = cg.lo[a];
        box[gi * 9 + 3 + a] = cg.hi[a];
        box[gi * 9 + 6 + a] = cg.inv_w[a];
      }
    for (int r = g0; r < g0 + n; ++r) {
      const float* p = x + (size_t)r * 3;
      const bool fin = cell_finite(p[0], p[1], p[2]);
      const CellBox bx = fin ? cell_box(cg, p[0], p[1], p[2], rr) : CellBox{{-1, -1, -1}, {-1, -1, -1}};
      for (int a = 0; a < 3; ++a) {
        if (cell) cell[(size_t)r * 3 + a] = fin ? cell_of(p[a], cg.lo[a], cg.inv_w[a], cg.g) : -1;
        if (range) {
          range[(size_t)r * 6 + a] = bx.lo[a];
          range[(size_t)r * 6 + 3 + a] = bx.hi[a];
        }
      }
    }
  }
  return NONODE_OK;
}

// Diagnostic (host arrays, no GPU): the k-NN search on the cell list, receiver by receiver, through the functions
// neighbor_select_knn_cells_kernel runs (nonode_cells.h, dist2, the same keys): a sequential restatement of its
// flow, with a sort where the wave keeps its 64 best.
int nonode_debug_neighbor_knn_cells(int G, int n_total, int n_max, int k, float r2_max, const int* graph_ptr,
                                    const float* x, int* nbr, int* deg, int* stats, float* d_out) {
  if (G < 1 || n_total < G || n_max < 1 || n_max > n_total || k < 1 || k > 64 || !(r2_max > 0.f) || !x ||
      (!graph_ptr && (long long)G * n_max != n_total))
    return fail(NONODE_EINVAL, "debug_neighbor_knn_cells: G=%d n_total=%d n_max=%d k=%d r2_max=%g", G, n_total, n_max,
                k, (double)r2_max);
  const int pitch = k < n_max - 1 ? k : n_max - 1;
  for (int gi = 0; gi < G; ++gi) {
    const HostGraph hg = host_graph(graph_ptr, gi, n_max, n_total, x, 0.f);
    const int g0 = hg.rows.r0, n = hg.rows.n;
    const float* xg = x + (size_t)g0 * 3;
    const CellGrid& cg = hg.cg;
    const int g = cg.g, nc = g * g * g;
    // the graph's part of the sorted order: its nodes by cell (the order inside a cell does not matter), the
    // non-finite ones in the trailing bucket nc; start = its part of cell_start
    std::vector<int> bucket(n), start(nc + 2, 0), order(n);
    for (int j = 0; j < n; ++j) {
      const float* p = xg + (size_t)j * 3;
      bucket[j] = nc;
      if (cell_finite(p[0], p[1], p[2]))
        bucket[j] = (cell_of(p[0], cg.lo[0], cg.inv_w[0], g) * g + cell_of(p[1], cg.lo[1], cg.inv_w[1], g)) * g +
                    cell_of(p[2], cg.lo[2], cg.inv_w[2], g);
      ++start[bucket[j] + 1];
    }
    for (int c = 0; c <= nc; ++c) start[c + 1] += start[c];
    {
      std::vector<int> cursor(start.begin(), start.end() - 1);
      for (int j = 0; j < n; ++j) order[cursor[bucket[j]]++] = j;
    }
    const int kk = imin(imin(k, n - 1), pitch);
    std::vector<u64> keys;
    for (int i = 0; i < n; ++i) {
      const int r = g0 + i;
      const float xi0 = xg[i * 3], xi1 = xg[i * 3 + 1], xi2 = xg[i * 3 + 2];
      int st[16] = {0, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 0, 0, g};
      float D = -1.f;
      keys.clear();
      auto feed = [&](int p, int e) {
        for (; p < e; ++p) {
          const int j = order[p];
          const float d2 = dist2(xi0, xi1, xi2, xg[j * 3], xg[j * 3 + 1], xg[j * 3 + 2]);
          ++st[13];
          const u64 key = candidate_key(d2, j, i, r2_max);
          if (key != KEY_NONE) keys.push_back(key);
        }
      };
      if (kk > 0) {
        bool whole = !cell_finite(xi0, xi1, xi2) || kk >= n - 1;
        if (!whole) {
          const int c0 = cell_of(xi0, cg.lo[0], cg.inv_w[0], g), c1 = cell_of(xi1, cg.lo[1], cg.inv_w[1], g),
                    c2 = cell_of(xi2, cg.lo[2], cg.inv_w[2], g);
          CellBox b1;
          int hw = 1;
          for (;; ++hw) {
            b1 = shell_box(c0, c1, c2, hw, g);
            if (box_covers_grid(b1, g)) break;
            int cnt = 0;
            for (int u = 0; u < box_runs(b1); ++u) {
              const CellSeg sg = box_run(b1, u, g);
              cnt += start[sg.c1 + 1] - start[sg.c0];
            }
            if (cnt - 1 >= kk) break;
          }
          st[0] = hw;
          for (int a = 0; a < 3; ++a) st[1 + a] = b1.lo[a], st[4 + a] = b1.hi[a];
          for (int u = 0; u < box_runs(b1); ++u) {
            const CellSeg sg = box_run(b1, u, g);
            feed(start[sg.c0], start[sg.c1 + 1]);
          }
          D = r2_max;
          if ((int)keys.size() >= kk) {
            std::nth_element(keys.begin(), keys.begin() + (kk - 1), keys.end());
            D = __builtin_bit_cast(float, (unsigned)(keys[kk - 1] >> 32));
          }
          float rr = 0.f;
          if (!cell_finite(D) || !knn_rr(D, &rr)) {
            whole = true;
          } else {
            const CellBox b2 = cell_box(cg, xi0, xi1, xi2, rr);
            for (int a = 0; a < 3; ++a) st[7 + a] = b2.lo[a], st[10 + a] = b2.hi[a];
            if (!box_inside(b2, b1))
              for (int u = 0; u < 2 * box_runs(b2); ++u) {
                const CellSeg sg = box_run_outside(b2, b1, u >> 1, u & 1, g);
                if (sg.c0 <= sg.c1) feed(start[sg.c0], start[sg.c1 + 1]);
              }
          }
        }
        if (whole) {
          keys.clear();
          feed(0, n);
        }
        st[14] = whole ? 1 : 0;
      }
      std::sort(keys.begin(), keys.end());
      const int d = imin((int)keys.size(), kk);
      std::vector<int> row(d);
      for (int l = 0; l < d; ++l) row[l] = (int)(unsigned)keys[l];
      std::sort(row.begin(), row.end());
      if (deg) deg[r] = d;
      if (nbr)
        for (int l = 0; l < pitch; ++l) nbr[(size_t)r * pitch + l] = l < d ? g0 + row[l] : -1;
      if (stats)
        for (int a = 0; a < 16; ++a) stats[(size_t)r * 16 + a] = st[a];
      if (d_out) d_out[r] = D;
    }
  }
  return NONODE_OK;
}

size_t nonode_neighbor_by_sender_workspace_bytes(long long cap, int n_total) {
  if (cap < 0 || cap >= (1ll << 31) || n_total <= 0) return 0;
  // the out-degrees / fill cursors, the rows as the fill claimed them
  return ((size_t)n_total + (size_t)cap) * sizeof(int);
}

int nonode_neighbor_by_sender(long long cap, int n_total, const int* rows, const int* col, const int* row_ptr,
                              int* srow_ptr, int* seid, int* valid, void* workspace, size_t workspace_bytes,
                              void* stream) {
  (void)rows;   // the receiver of an entry is not needed: the list is receiver-major, so ascending p is the order
  if (cap < 0 || cap >= (1ll << 31) || n_total <= 0 || n_total >= (1 << 30))
    return fail(NONODE_EINVAL, "neighbor_by_sender: cap=%lld n_total=%d", cap, n_total);
  if (!srow_ptr) return fail(NONODE_EINVAL, "neighbor_by_sender: null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (cap == 0) {   // no pair at all
    if (hipMemsetAsync(srow_ptr, 0, ((size_t)n_total + 1) * sizeof(int), s) != hipSuccess)
      return fail(NONODE_ELAUNCH, "neighbor_by_sender: memset");
    return NONODE_OK;
  }
  if (!col || !row_ptr || !seid || !valid || !workspace) return fail(NONODE_EINVAL, "neighbor_by_sender: null pointer");
  if (workspace_bytes < nonode_neighbor_by_sender_workspace_bytes(cap, n_total))
    return fail(NONODE_EINVAL, "neighbor_by_sender: workspace %zu < %zu", workspace_bytes,
                nonode_neighbor_by_sender_workspace_bytes(cap, n_total));
  int* cnt = (int*)workspace;
  int* tpos = cnt + n_total;
  if (hipMemsetAsync(cnt, 0, (size_t)n_total * sizeof(int), s) != hipSuccess)
    return fail(NONODE_ELAUNCH, "neighbor_by_sender: memset");
  const unsigned blocks = (unsigned)((cap + 255) / 256);
  hipLaunchKernelGGL(sender_count_kernel, dim3(blocks), dim3(256), 0, s, cap, n_total, col, row_ptr, cnt, valid);
  if (int rc = check_launch("sender_count_kernel")) return rc;
  if (int rc = nonode_tu::graph_scan(n_total, cnt, srow_ptr, s)) return rc;
  hipLaunchKernelGGL(sender_fill_kernel, dim3(blocks), dim3(256), 0, s, cap, n_total, col, row_ptr, cnt, tpos, seid);
  if (int rc = check_launch("sender_fill_kernel")) return rc;
  hipLaunchKernelGGL(sender_sort_kernel, dim3((n_total + 3) / 4), dim3(256), 0, s, n_total, srow_ptr, tpos, seid);
  return check_launch("sender_sort_kernel");
}

int nonode_prepare_nodes(int B, int N, int F, const float* loc, const float* vel, const int* t_in,
                         const float* charges, float* x_out, float* v_out, float* nodes, float* loc_mean,
                         void* stream) {
  if (B <= 0 || N <= 0 || F <= 0 || (long long)F * B * N >= (1ll << 30))
    return fail(NONODE_EINVAL, "prepare_nodes: B=%d N=%d F=%d", B, N, F);
  if (!loc || !vel || !x_out || !v_out || !nodes) return fail(NONODE_EINVAL, "prepare_nodes: null pointer");
  return launch_node_features(B, B * N, N, F, nullptr, loc, vel, t_in, charges, x_out, v_out, nodes, loc_mean,
                              (hipStream_t)stream);
}

int nonode_prepare_nodes_ragged(int G, int n_total, int F, const int* graph_ptr, const float* loc, const float* vel,
                                const int* t_in, const float* charges, float* x_out, float* v_out, float* nodes,
                                float* loc_mean, void* stream) {
  if (G < 1 || n_total < G || F <= 0 || (long long)F * n_total >= (1ll << 30))
    return fail(NONODE_EINVAL, "prepare_nodes_ragged: G=%d n_total=%d F=%d", G, n_total, F);
  if (!graph_ptr || !loc || !vel || !x_out || !v_out || !nodes)
    return fail(NONODE_EINVAL, "prepare_nodes_ragged: null pointer");
  return launch_node_features(G, n_total, 0, F, graph_ptr, loc, vel, t_in, charges, x_out, v_out, nodes, loc_mean,
                              (hipStream_t)stream);
}

int nonode_edge_features(long long cap, int n_nodes, const void* rows, const void* cols, int idx_bytes,
                         const int* n_edges, const float* x, const float* charges, float* edge_attr, void* stream) {
  if (cap < 0 || cap >= (1ll << 31) || n_nodes <= 0 || (idx_bytes != 4 && idx_bytes != 8))
    return fail(NONODE_EINVAL, "edge_features: cap=%lld n_nodes=%d idx_bytes=%d", cap, n_nodes, idx_bytes);
  if (cap == 0) return NONODE_OK;
  if (!rows || !cols || !x || !edge_attr) return fail(NONODE_EINVAL, "edge_features: null pointer");
  const unsigned blocks = (unsigned)((cap + 255) / 256);
  hipStream_t s = (hipStream_t)stream;
  if (idx_bytes == 8)
    hipLaunchKernelGGL(edge_features_kernel<long long>, dim3(blocks), dim3(256), 0, s, cap, n_nodes,
                       (const long long*)rows, (const long long*)cols, n_edges, x, charges, edge_attr);
  else
    hipLaunchKernelGGL(edge_features_kernel<int>, dim3(blocks), dim3(256), 0, s, cap, n_nodes, (const int*)rows,
                       (const int*)cols, n_edges, x, charges, edge_attr);
  return check_launch("edge_features_kernel");
}

}  // extern "C"
