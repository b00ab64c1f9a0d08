// nonode_cells.h — the uniform grid of the cut-off neighbour search (nonode_neighbor.hip): the grid rule, the
// binning function and a receiver's search box, written once as __host__ __device__ functions that the
// kernels and the host entry nonode_debug_neighbor_cells share (as seg_walk is shared with
// nonode_debug_edge_walk), so what a test checks on the host is what the device runs.
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

}  // namespace
