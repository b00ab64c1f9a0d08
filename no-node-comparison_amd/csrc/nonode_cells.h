// nonode_cells.h — the uniform grid of the cut-off and k-NN neighbour searches (nonode_neighbor.hip): the grid rule,
// the binning function, a receiver's search boxes and the radius of the k-NN search, written once as
// __host__ __device__ functions that the kernels and the host entries nonode_debug_neighbor_cells /
// nonode_debug_neighbor_knn_cells share (as seg_walk is shared with nonode_debug_edge_walk), so what a test
// checks on the host is what the device runs.
//
// Why the search misses no candidate. Everything is per axis, with fl() the
// rounding of one f32 operation, and rests on rounded operations being monotone, not on a margin:
//   - rr is a float with fl(rr rr) > r2_max (cell_rr).
//   - Take a sender with x_j > fl(x_i + rr). Rounding is monotone and x_j is a float, so x_j > x_i + rr in
//     the reals, hence d = fl(x_j - x_i) >= rr, fl(d d) >= fl(rr rr) > r2_max, and dist2's sum of rounded
//     non-negative terms is at least its first term: j is no candidate. The same below fl(x_i - rr).
//   - So every candidate has fl(x_i - rr) <= x_j <= fl(x_i + rr), and cell_of is monotone in x (a rounded
//     subtraction of lo, a rounded product with inv_w >= 0, floor, clamp), so
//     cell_of(x_i - rr) <= cell_of(x_j) <= cell_of(x_i + rr): the box cell_box returns.
// The cell width max(rr, extent / g) only decides how many cells that box spans (three per axis, rarely
// four), never whether it covers. A graph whose extent is stretched (an outlier, a diverged rollout) puts
// most nodes into few cells and the search degrades towards the brute-force one inside them: still the
// same graph, only slower. An extent that overflows to inf gives inv_w = 0: every finite node lands in
// cell 0 (0 x = 0, and the NaN of inf x 0 maps to cell 0 as well).
// A node with a non-finite coordinate has no cell: under a finite r2_max it is nobody's candidate and has
// none (inf - x = inf squares to inf, inf - inf is NaN). It stays out of the bounding box and goes to a
// trailing bucket of the sort, so the sorted order still holds every node exactly once.
//
// The k-NN search on the same grid (neighbor_select_knn_cells_kernel): the radius is
// found per receiver instead of being given. The grid is built with rr = 0, so the width is extent / g alone.
//   Phase 1: the shell box [c - s, c + s] (clamped) around the receiver's own cell c, s grown from 1 until the
//     box holds kk other nodes (cell_start differences) or covers the grid, is fed to the keep-the-k-smallest
//     body. D = the kk-th smallest d2 found; fewer than kk found: D = r2_max if that is finite.
//   Phase 2: the cut-off search above with r2_max := D, i.e. cell_box(x_i, rr) with fl(rr rr) > D (knn_rr), of
//     which only the cells outside the shell box are still to be walked (box_run_outside): every node is in
//     one cell, so no key is fed twice.
//   Exact, because: (1) D is the kk-th smallest d2 over a SUBSET of the candidates, so the kk-th smallest over
//     all of them is <= D and every one of the true kk smallest keys has d2 <= D (ties at D included), or, with
//     D = r2_max, every candidate has; (2) by the covering argument above, which holds for d2 <= r2 with any
//     r2 and its rr, every j with d2 <= D has its cell in cell_box(x_i, rr); (3) so the keys fed, shell box and
//     box 2 together, are a set of candidates that contains the true kk smallest, and the kk smallest of that
//     set are the kk smallest of all. What the shell box feeds beyond box 2 are real candidates and do no harm.
//   A zero extent on an axis gives w = 0 and inv_w = +inf there (also a width that underflows, and the NaN
//     width of a graph without a finite node): cell_of is then 0 for x <= lo (-inf, and the NaN of 0 inf) and
//     g - 1 for x > lo (+inf): still one monotone function of x, which is all (2) uses, so the behaviour is
//     kept; with zero extent every node has x = lo and lands in cell 0.
//   The receiver walks its whole graph instead (the brute-force search on the sorted copy, the non-finite
//     bucket included) when it has a non-finite coordinate, when kk = N_g - 1 (every other node is wanted), when
//     D is not finite (fewer than kk finite nodes under r2_max = +inf, where a node at +-inf is a candidate with
//     d2 = inf, or a d2 that overflowed), or when knn_rr finds no radius.
#pragma once

#pragma clang fp contract(off)

namespace {

// the grid aims at CELL_FILL nodes per cell: g cells per axis, g the largest integer with
// g^3 CELL_FILL <= N (at least 1), a function of N alone that host and device compute alike
constexpr int CELL_FILL = 4;
__host__ __device__ __forceinline__ int cells_per_axis(int n) {
  const int m = n / CELL_FILL;
  if (m < 8) return 1;
  int g = (int)cbrtf((float)m);   // an estimate: the two loops make it exact
  if (g < 1) g = 1;
  while ((long long)g * g * g > m) --g;
  while ((long long)(g + 1) * (g + 1) * (g + 1) <= m) ++g;
  return g;
}

__host__ __device__ __forceinline__ bool cell_finite(float v) {
  return (__builtin_bit_cast(unsigned, v) & 0x7F800000u) != 0x7F800000u;
}
__host__ __device__ __forceinline__ bool cell_finite(float a, float b, float c) {
  return cell_finite(a) && cell_finite(b) && cell_finite(c);
}

// finite floats as unsigned integers in the same order (-0 below +0), so that an integer atomic max gives
// a bounding box that does not depend on the order of its updates. No finite float has key 0 or ~0.
__host__ __device__ __forceinline__ unsigned cell_key(float v) {
  const unsigned b = __builtin_bit_cast(unsigned, v);
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__host__ __device__ __forceinline__ float cell_unkey(unsigned k) {
  return __builtin_bit_cast(float, k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}

// A graph's grid from its bounding box bb[6]: bb[a] = max over the finite nodes of ~cell_key(x_a) (the
// lower corner), bb[3 + a] = max of cell_key(x_a) (the upper one), zero where the graph has no finite node
// (nothing is binned then). Width per axis max(rr, extent / g); inv_w its rounded reciprocal, 0 for an
// extent that overflowed.
struct CellGrid {
  int g;
  float lo[3], hi[3], inv_w[3];
};
__host__ __device__ __forceinline__ CellGrid cell_grid(const unsigned* bb, int n, float rr) {
  CellGrid cg;
  cg.g = cells_per_axis(n);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    cg.lo[a] = cell_unkey(~bb[a]);
    cg.hi[a] = cell_unkey(bb[3 + a]);
    const float w = (cg.hi[a] - cg.lo[a]) / (float)cg.g;
    cg.inv_w[a] = 1.0f / (w > rr ? w : rr);   // (a NaN width, no finite node: rr)
  }
  return cg;
}

// THE binning function: clamp(floor((x - lo) inv_w), 0, g - 1), monotone in x; NaN -> 0
__host__ __device__ __forceinline__ int cell_of(float x, float lo, float inv_w, int g) {
  const float t = floorf((x - lo) * inv_w);
  if (!(t >= 0.f)) return 0;
  return t >= (float)(g - 1) ? g - 1 : (int)t;
}

// the cells receiver x searches: cell_of(x - rr) .. cell_of(x + rr) on every axis
struct CellBox {
  int lo[3], hi[3];
};
__host__ __device__ __forceinline__ CellBox cell_box(const CellGrid& cg, float x0, float x1, float x2, float rr) {
  const float x[3] = {x0, x1, x2};
  CellBox b;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    b.lo[a] = cell_of(x[a] - rr, cg.lo[a], cg.inv_w[a], cg.g);
    b.hi[a] = cell_of(x[a] + rr, cg.lo[a], cg.inv_w[a], cg.g);
  }
  return b;
}

// The search radius of a finite r2_max > 0, computed once on the host: a little above its square root and,
// which is all the covering argument asks, with fl(rr rr) > r2_max (the loop runs only where r2_max is
// subnormal and the product's rounding is coarse).
inline float cell_rr(float r2_max) {
  float rr = sqrtf(r2_max) * (1.0f + 0x1p-20f);
  while (!(rr * rr > r2_max)) rr *= 1.0f + 0x1p-10f;
  return rr;
}

// ---- the k-NN search on the grid (header comment) ----

// the shell box of half-width s around cell c, clamped to the grid
__host__ __device__ __forceinline__ CellBox shell_box(int c0, int c1, int c2, int s, int g) {
  const int c[3] = {c0, c1, c2};
  CellBox b;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    b.lo[a] = c[a] - s > 0 ? c[a] - s : 0;
    b.hi[a] = c[a] + s < g - 1 ? c[a] + s : g - 1;
  }
  return b;
}
__host__ __device__ __forceinline__ bool box_covers_grid(const CellBox& b, int g) {
  return b.lo[0] <= 0 && b.lo[1] <= 0 && b.lo[2] <= 0 && b.hi[0] >= g - 1 && b.hi[1] >= g - 1 && b.hi[2] >= g - 1;
}
__host__ __device__ __forceinline__ bool box_inside(const CellBox& b, const CellBox& in) {
  return b.lo[0] >= in.lo[0] && b.lo[1] >= in.lo[1] && b.lo[2] >= in.lo[2] && b.hi[0] <= in.hi[0] &&
         b.hi[1] <= in.hi[1] && b.hi[2] <= in.hi[2];
}

// Cells c0 .. c1 (z fastest) of a graph's grid: one contiguous run of the sorted order; c0 > c1: none.
struct CellSeg {
  int c0, c1;
};
__host__ __device__ __forceinline__ int box_runs(const CellBox& b) {
  return (b.hi[0] - b.lo[0] + 1) * (b.hi[1] - b.lo[1] + 1);
}
// run u of box b, u < box_runs(b): the cells (cx, cy, z_lo .. z_hi), (cx, cy) = (lo0 + u / ny, lo1 + u % ny)
__host__ __device__ __forceinline__ CellSeg box_run(const CellBox& b, int u, int g) {
  const int ny = b.hi[1] - b.lo[1] + 1;
  const int c = ((b.lo[0] + u / ny) * g + b.lo[1] + u % ny) * g;
  return CellSeg{c + b.lo[2], c + b.hi[2]};
}
// half h (0: below, 1: above) of run u of box b, without the cells of box `in`: a run whose (cx, cy) is outside
// in's is whole in its lower half; one inside leaves z_lo .. in.lo2 - 1 below and in.hi2 + 1 .. z_hi above
__host__ __device__ __forceinline__ CellSeg box_run_outside(const CellBox& b, const CellBox& in, int u, int h, int g) {
  const int ny = b.hi[1] - b.lo[1] + 1;
  const int cx = b.lo[0] + u / ny, cy = b.lo[1] + u % ny;
  const int c = (cx * g + cy) * g;
  const bool over = cx >= in.lo[0] && cx <= in.hi[0] && cy >= in.lo[1] && cy <= in.hi[1];
  if (!over) return h == 0 ? CellSeg{c + b.lo[2], c + b.hi[2]} : CellSeg{1, 0};
  if (h == 0) return CellSeg{c + b.lo[2], c + (b.hi[2] < in.lo[2] - 1 ? b.hi[2] : in.lo[2] - 1)};
  return CellSeg{c + (b.lo[2] > in.hi[2] + 1 ? b.lo[2] : in.hi[2] + 1), c + b.hi[2]};
}

// The search radius of a finite D >= 0, found per receiver on the device: a float rr with fl(rr rr) > D, which
// is all the covering argument asks (cell_rr's property). From just above the square root, and from 2^-74 (the
// smallest power of two whose square is not zero) where D is zero or tiny; raised by 2^-10 a few times (the
// product's rounding is coarse where it is subnormal), then by a quarter a time, 64 steps at the most; a
// product that overflows is +inf > D. False: none found (the receiver walks its whole graph).
__host__ __device__ __forceinline__ bool knn_rr(float D, float* rr_out) {
  float rr = sqrtf(D) * (1.0f + 0x1p-20f);
  if (!(rr >= 0x1p-74f)) rr = 0x1p-74f;
  for (int it = 0; it < 64; ++it) {
    if (rr * rr > D) {
      *rr_out = rr;
      return true;
    }
    rr *= it < 4 ? 1.0f + 0x1p-10f : 1.25f;
  }
  return false;
}

}  // namespace
