/*
 * local_grid.h -- the uniform grid over the bounding box of a cloud that local.hip (k nearest neighbours, local kriging)
 * and shepard.hip (modified quadratic Shepard) bin their centres on: the same cell function, the same grid size, the same
 * batch size from which targets are processed in cell order, the same fixed-order wave sum.  The binning itself is
 * sinterp_grid_bin (common.h; defined once, in local.hip).
 *
 * The cell-function contract.  The search of local.hip and the sweep of shepard.hip are exact because the SAME function
 * lk_axis_cell that binned the centres is asked about the target, and because it is non-decreasing in the coordinate: a
 * subtraction of, a division by and a multiplication with constants, then a truncation, each monotone under rounding.
 * The binning is compiled in local.hip (FMA contraction on), the sweep's queries in shepard.hip (contraction off), and
 * the two agree bit for bit because nothing in lk_axis_cell can be contracted: no product feeds an addition or a
 * subtraction.  The pragma in its body keeps that true if the expression is ever edited.
 */
#ifndef SINTERP_LOCAL_GRID_H
#define SINTERP_LOCAL_GRID_H

#include <math.h>

#define LK_SORT_MIN 4096          /* batches of at least this many targets are processed in cell order */

struct LkGrid { double lo[3], hi[3]; };

/* cell index of coordinate v on an axis of g cells over [lo, hi]; non-decreasing in v; NaN and a degenerate axis -> 0 */
__host__ __device__ __forceinline__ int lk_axis_cell(double v, double lo, double hi, int g)
{
#pragma clang fp contract(off)
  const double f = hi > lo ? (v - lo) / (hi - lo) : 0.0;
  const double t = f * (double)g;
  if (!(t > 0.0)) return 0;
  return t >= (double)(g - 1) ? g - 1 : (int)t;
}

template <int DIM>
__device__ __forceinline__ size_t lk_cell(const LkGrid &G, int g, const double (&v)[DIM])
{
  size_t cell = 0;
#pragma unroll
  for (int c = DIM - 1; c >= 0; c--) cell = cell * (size_t)g + (size_t)lk_axis_cell(v[c], G.lo[c], G.hi[c], g);
  return cell;
}

static inline int lk_grid_size(size_t n, int dim)
{
  const double cells = (double)n / 8.0;            /* ~8 centres per cell: a 3^dim block holds k = 64 in 2-D at the first ring */
  int g = (int)floor(pow(cells < 1.0 ? 1.0 : cells, 1.0 / dim));
  const int gmax = dim == 1 ? (1 << 20) : (dim == 2 ? 1024 : 100);
  return g < 1 ? 1 : (g > gmax ? gmax : g);
}

/* words of the cell-offset array that sinterp_grid_bin fills: ncell + 1 offsets and the scratch of its scan */
static inline size_t lk_off_words(size_t ncell) { return ncell + 1 + ncell / 1024 + 8; }

/* fixed-order sum over the 64 lanes (every lane receives it: a + b and b + a are the same bits).  The additions are plain;
   a product handed in is rounded, or fused with the first addition, as the CALLER's contraction setting says: the
   instructions of a contract(off) region (shepard.hip) carry no contract flag wherever this function is defined. */
__device__ __forceinline__ double lk_sum(double v)
{
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

#endif
