/*
 * variogram.hip -- the binned pair sums of the empirical semivariogram: for every unordered pair of sites closer than h_max
 * the pair count, sum (f_i - f_j)^2, sum h and sum sqrt|f_i - f_j| of its lag bin.  Memory O(N + cells + bins), work
 * proportional to the pairs inside the pruning stencil, no N x N object anywhere (DESIGN_VARIOGRAM.md).
 *
 *   range pass        sinterp_bbox_keys over the sites and over f as a 1-D point set, vg_finite_kernel counts the non-finite
 *                     entries of both; 112 bytes come back and decide GSL_EDOM, the three shifts and the grid.
 *   binning           sinterp_grid_bin (local.hip) on a grid whose cells are not smaller than about h_max on the longest axis;
 *                     vg_gather_kernel writes records {x[dim], f} and the cell of every place in cell order.
 *   vg_pair_kernel    one thread per site i in cell order.  It walks the grid rows of the HALF stencil: its own row from the
 *                     place behind i to the end of cell cx + R0, and every row that is lexicographically ahead over cells
 *                     cx - R0 .. cx + R0 (axis 0 runs fastest, so each row piece is one contiguous run of records).  Every
 *                     unordered pair within reach is met exactly once.  A small cloud has few sites per compute unit and long
 *                     runs: gridDim.y = split workgroups share the 256 sites of a block, workgroup s taking every split-th
 *                     record of every run, so that about 2048 workgroups are in flight (split <= 16).
 *
 * Exactness.  This file is compiled with -ffp-contract=off: r2 = ((dx*dx) + (dy*dy)) + (dz*dz), edge2[b] = (b*w)*(b*w) with
 * w = h_max / n_bins, edge2[n_bins] = h_max*h_max are the same IEEE operations a numpy reference performs.  Every term is
 * quantised to a 64-bit integer q = rint(ldexp(t, shift)) < 2^63 and added with INTEGER atomics only: the low word, and one
 * carry into the high word each time the low word wraps.  Integer addition is associative and commutative, so the seven
 * words of a bin do not depend on the order of the rows, the slot order the binning's atomics hand out, the grid, the
 * launch shape or the run.  There is no floating-point atomic and no floating-point sum in this file.
 *
 * LDS.  A workgroup accumulates into C copies of the histogram [bin][word][copy] (copy = thread & (C - 1): lanes that meet
 * the same bin in one instruction land on C neighbouring words instead of one), C = 512 / n_bins rounded down to a power of
 * two in 1 .. 16: at most 28 KiB, plus the n_bins + 1 squared edges.  One flush per workgroup: the copies of a word pair are
 * summed as 128-bit integers in registers and added to the global words with one 64-bit atomic each plus the carry.
 */
#include "common.h"
#include <math.h>
#include "rbf_phi.h"              /* with_dim */
#include "local_grid.h"           /* LkGrid, lk_off_words */

#define VG_HEAD 256               /* bytes: LkGrid | box keys of x at 64 | box keys of f at 112 | non-finite count at 160 | pairs tested at 168 */
#define VG_THREADS 256
#define VG_WORDS 7
typedef unsigned long long vg_u64;

/* entries of x (the dim leading columns of every row) and of f that are NaN or infinite */
__global__ void __launch_bounds__(256)
vg_finite_kernel(const double *__restrict__ x, size_t n, size_t xtda, int dim, const double *__restrict__ f, vg_u64 *__restrict__ bad)
{
  unsigned cnt = 0;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    for (int c = 0; c < dim; c++) cnt += !(fabs(x[i * xtda + c]) < INFINITY);
    cnt += !(fabs(f[i]) < INFINITY);
  }
  if (cnt) atomicAdd(bad, (vg_u64)cnt);
}

template <int DIM>
__global__ void __launch_bounds__(256)
vg_gather_kernel(const double *__restrict__ x, size_t n, size_t xtda, const double *__restrict__ f, const unsigned *__restrict__ cellid,
                 const unsigned *__restrict__ slot, const unsigned *__restrict__ offset, double *__restrict__ rec, unsigned *__restrict__ cell_at)
{
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const unsigned cell = cellid[i];
    const size_t p = (size_t)offset[cell] + slot[i];
    double *r = rec + p * (DIM + 1);
#pragma unroll
    for (int c = 0; c < DIM; c++) r[c] = x[i * xtda + c];
    r[DIM] = f[i];
    cell_at[p] = cell;
  }
}

struct VgParams {
  double w, h_max;                /* bin width h_max / n_bins as the host rounded it, and the cut-off */
  int n_bins, copies;             /* copies: a power of two */
  int g, reach[3];                /* cells per axis; cells to visit on either side per axis (0 on an axis that is absent) */
  int shift[3];
  int split;                      /* gridDim.y: workgroup (bx, s) takes every split-th record of the runs of its 256 sites */
};

/* lo/hi += q as a 128-bit integer: the carry is one more integer add, made exactly when the low word wrapped */
__device__ __forceinline__ void vg_add128(vg_u64 *lo, vg_u64 *hi, vg_u64 q)
{
  if (!q) return;
  const vg_u64 old = atomicAdd(lo, q);
  if (old + q < old) atomicAdd(hi, 1ULL);
}

__device__ __forceinline__ vg_u64 vg_quantise(double t, int shift) { return (vg_u64)rint(ldexp(t, shift)); }

template <int DIM>
__global__ void __launch_bounds__(VG_THREADS)
vg_pair_kernel(VgParams P, unsigned n, const unsigned *__restrict__ off, const unsigned *__restrict__ cell_at, const double *__restrict__ rec,
               vg_u64 *__restrict__ acc, vg_u64 *__restrict__ tested_out)
{
  extern __shared__ double vg_lds[];
  double *s_edge2 = vg_lds;                                            /* n_bins + 1 */
  vg_u64 *s_hist = (vg_u64 *)(vg_lds + P.n_bins + 1);                  /* [n_bins][7][copies] */
  vg_u64 *s_tested = s_hist + (size_t)P.n_bins * VG_WORDS * P.copies;
  const int nb = P.n_bins, C = P.copies;
  for (int b = threadIdx.x; b <= nb; b += VG_THREADS) {
    const double e = (double)b * P.w;
    s_edge2[b] = b < nb ? e * e : P.h_max * P.h_max;
  }
  for (int k = threadIdx.x; k < nb * VG_WORDS * C; k += VG_THREADS) s_hist[k] = 0ULL;
  if (threadIdx.x == 0) *s_tested = 0ULL;
  __syncthreads();

  const unsigned p = blockIdx.x * VG_THREADS + threadIdx.x;
  if (p < n) {
    const double cut2 = s_edge2[nb], inv_w = 1.0 / P.w;
    const unsigned copy = threadIdx.x & (unsigned)(C - 1);
    double xi[DIM];
#pragma unroll
    for (int c = 0; c < DIM; c++) xi[c] = rec[(size_t)p * (DIM + 1) + c];
    const double fi = rec[(size_t)p * (DIM + 1) + DIM];
    const unsigned ci = cell_at[p], g = (unsigned)P.g;
    int cx, cy = 0, cz = 0;
    if constexpr (DIM == 1) cx = (int)ci;
    else {
      cx = (int)(ci % g);
      const unsigned up = ci / g;
      if constexpr (DIM == 2) cy = (int)up;
      else { cy = (int)(up % g); cz = (int)(up / g); }
    }
    const int x0 = cx - P.reach[0] > 0 ? cx - P.reach[0] : 0, x1 = cx + P.reach[0] < P.g - 1 ? cx + P.reach[0] : P.g - 1;
    const int rz = DIM == 3 ? P.reach[2] : 0, ry = DIM >= 2 ? P.reach[1] : 0;
    vg_u64 tested = 0;
    for (int dz = 0; dz <= rz; dz++) {
      const int z = cz + dz;
      if (z >= P.g) break;
      for (int dy = dz > 0 ? -ry : 0; dy <= ry; dy++) {
        const int y = cy + dy;
        if (y < 0 || y >= P.g) continue;
        const size_t row = ((size_t)z * g + (size_t)y) * g;                 /* 0 in 1-D, y g in 2-D */
        const unsigned e = off[row + (size_t)x1 + 1];
        const unsigned b0 = (dz == 0 && dy == 0) ? p + 1 : off[row + (size_t)x0];
        for (unsigned j = b0 + blockIdx.y; j < e; j += (unsigned)P.split) {
          const double *r = rec + (size_t)j * (DIM + 1);
          double r2;
          { const double d = xi[0] - r[0]; r2 = d * d; }
#pragma unroll
          for (int c = 1; c < DIM; c++) { const double d = xi[c] - r[c]; r2 = r2 + d * d; }
          tested++;
          if (!(r2 < cut2)) continue;
          const double h = sqrt(r2);
          int b = (int)(h * inv_w);
          b = b < 0 ? 0 : (b > nb - 1 ? nb - 1 : b);
          while (r2 < s_edge2[b]) b--;                                       /* edge2[0] = 0 <= r2 */
          while (r2 >= s_edge2[b + 1]) b++;                                  /* r2 < edge2[n_bins] */
          const double df = fi - r[DIM];
          vg_u64 *hb = s_hist + (size_t)b * VG_WORDS * C + copy;
          atomicAdd(hb, 1ULL);
          vg_add128(hb + 1 * C, hb + 2 * C, vg_quantise(df * df, P.shift[0]));
          vg_add128(hb + 3 * C, hb + 4 * C, vg_quantise(h, P.shift[1]));
          vg_add128(hb + 5 * C, hb + 6 * C, vg_quantise(sqrt(fabs(df)), P.shift[2]));
        }
      }
    }
    if (tested) atomicAdd(s_tested, tested);
  }
  __syncthreads();

  /* the flush: thread (bin, k) owns the count (k = 0) or the word pair of sum k - 1 */
  for (int idx = threadIdx.x; idx < nb * 4; idx += VG_THREADS) {
    const int b = idx >> 2, k = idx & 3;
    const vg_u64 *hb = s_hist + (size_t)b * VG_WORDS * C;
    vg_u64 *gb = acc + (size_t)b * VG_WORDS;
    if (k == 0) {
      vg_u64 cnt = 0;
      for (int c = 0; c < C; c++) cnt += hb[c];
      if (cnt) atomicAdd(gb, cnt);
    } else {
      const int wl = 2 * k - 1;
      vg_u64 lo = 0, hi = 0;
      for (int c = 0; c < C; c++) {
        const vg_u64 l = hb[wl * C + c];
        lo += l;
        hi += hb[(wl + 1) * C + c] + (vg_u64)(lo < l);
      }
      if (lo) {
        const vg_u64 old = atomicAdd(gb + wl, lo);
        hi += (vg_u64)(old + lo < old);
      }
      if (hi) atomicAdd(gb + wl + 1, hi);
    }
  }
  if (threadIdx.x == 0 && *s_tested) atomicAdd(tested_out, *s_tested);
}

/* the order-preserving keys of sinterp_bbox_keys back to doubles */
static double vg_unkey(vg_u64 k)
{
  const vg_u64 u = (k >> 63) ? (k & 0x7fffffffffffffffULL) : ~k;
  double v;
  memcpy(&v, &u, sizeof v);
  return v;
}

static int vg_shift_of(double bound)
{
  int e = 0;
  (void)frexp(bound, &e);
  return 62 - e;
}

/* cells per axis and the reach per axis: cells about h_max wide on the longest axis, at least two sites per cell on
   average, and a stencil whose cell visits stay proportional to n */
static void vg_choose_grid(size_t n, int dim, const double *lo, const double *hi, double h_max, int *g_out, int *reach)
{
  double longest = 0.0;
  for (int c = 0; c < dim; c++) if (hi[c] - lo[c] > longest) longest = hi[c] - lo[c];
  const int gmax = dim == 1 ? (1 << 20) : (dim == 2 ? 1024 : 100);
  double cap = floor(pow((double)n / 2.0, 1.0 / dim));
  if (cap > gmax) cap = gmax;
  double want = longest > 0.0 ? floor(longest / h_max) : 1.0;
  if (!(want < cap)) want = cap;
  int g = want < 1.0 ? 1 : (int)want;
  for (;;) {
    double visits = 1.0;
    for (int c = 0; c < 3; c++) reach[c] = 0;
    for (int c = 0; c < dim; c++) {
      const double side = (hi[c] - lo[c]) / g;
      /* two sites closer than h_max on this axis differ by at most floor(h_max / side) + 1 cells; the slack of 1e-6 of a
         cell covers the rounding of lk_axis_cell (below 1e-9 of a cell at g <= 2^20) */
      double r = side > 0.0 ? floor(h_max / side + 1e-6) + 1.0 : 0.0;
      if (r > g - 1) r = g - 1;
      reach[c] = (int)r;
      visits *= (2.0 * r + 1.0) * g;
    }
    if (g == 1 || visits <= 32.0 * (double)n + 1024.0) break;
    g = g * 3 / 4;
    if (g < 1) g = 1;
  }
  *g_out = g;
}

extern "C" int gsl_sinterp_hip_variogram(gsl_sinterp_hip_ctx *ctx, const double *d_x, size_t n, int dim, size_t xtda, const double *d_f,
                                         double h_max, int n_bins, unsigned long long *acc, int shift[3])
{
  /* the arguments first: nothing here touches the device */
  REQUIRE(ctx, dim >= 1 && dim <= 3 && n_bins >= 1 && n_bins <= 256 && h_max > 0.0 && h_max < INFINITY, ST_EINVAL);
  REQUIRE(ctx, xtda >= (size_t)dim && n <= 0x7fffffffULL, ST_EINVAL);
  REQUIRE(ctx, ctx != NULL && acc != NULL && shift != NULL && (n == 0 || (d_x != NULL && d_f != NULL)), ST_EFAULT);
  memset(acc, 0, (size_t)n_bins * VG_WORDS * sizeof *acc);
  shift[0] = 0; shift[1] = vg_shift_of(h_max); shift[2] = 0;
  ctx->vg_pairs_tested = 0;
  if (n < 2) return ST_SUCCESS;
  HIP_OK(ctx, hipSetDevice(ctx->device));

  const size_t ncell_max = n / 2 + 64;
  const size_t acc_bytes = round_up((size_t)n_bins * VG_WORDS * sizeof(vg_u64), 256);
  const size_t off_bytes = round_up(lk_off_words(ncell_max) * 4, 16), cell_bytes = round_up(n * 4, 16);
  void *buf = NULL;
  ctx->local_key.id = 0;                               /* local kriging's pack shares this buffer: it is rewritten */
  int st = sinterp_localbuf(ctx, VG_HEAD + acc_bytes + off_bytes + cell_bytes + n * (size_t)(dim + 1) * sizeof(double), &buf);
  if (st) return st;
  char *b = (char *)buf;
  LkGrid *grid = (LkGrid *)b;
  vg_u64 *d_box = (vg_u64 *)(b + 64), *d_fbox = (vg_u64 *)(b + 112), *d_bad = (vg_u64 *)(b + 160), *d_tested = (vg_u64 *)(b + 168);
  vg_u64 *d_acc = (vg_u64 *)(b + VG_HEAD);
  unsigned *off = (unsigned *)(b + VG_HEAD + acc_bytes), *cell_at = (unsigned *)(b + VG_HEAD + acc_bytes + off_bytes);
  double *rec = (double *)(b + VG_HEAD + acc_bytes + off_bytes + cell_bytes);

  /* ---- the range pass */
  size_t blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  st = sinterp_bbox_keys(ctx, d_x, n, xtda, dim, d_box);
  if (!st) st = sinterp_bbox_keys(ctx, d_f, n, 1, 1, d_fbox);
  if (st) return st;
  HIP_OK(ctx, hipMemsetAsync(d_bad, 0, 2 * sizeof(vg_u64), ctx->stream));
  hipLaunchKernelGGL(vg_finite_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, d_x, n, xtda, dim, d_f, d_bad);
  LAUNCH_CHECK(ctx);
  vg_u64 head[14];                                     /* x keys [0, 6), f keys [6, 12), non-finite count, pairs tested */
  HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
  HIP_OK(ctx, hipMemcpy(head, d_box, sizeof head, hipMemcpyDeviceToHost));
  if (head[12] != 0) {
    snprintf(ctx->err, sizeof ctx->err, "gsl_sinterp_hip_variogram: %llu non-finite entries in the sites or the response", head[12]);
    return ST_EDOM;
  }
  double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  for (int c = 0; c < dim; c++) { lo[c] = vg_unkey(head[2 * c]); hi[c] = vg_unkey(head[2 * c + 1]); }
  const double spread = vg_unkey(head[7]) - vg_unkey(head[6]);
  if (!(spread < INFINITY) || !(spread * spread < INFINITY))
    return sinterp_fail(ctx, ST_EDOM, "gsl_sinterp_hip_variogram: the squared range of the response overflows", hipSuccess, __FILE__, __LINE__);
  if (spread > 0.0) { shift[0] = vg_shift_of(spread * spread); shift[2] = vg_shift_of(sqrt(spread)); }

  /* ---- the binning */
  VgParams P;
  P.w = h_max / (double)n_bins; P.h_max = h_max; P.n_bins = n_bins;
  P.copies = 1;
  while (P.copies < 16 && 2 * P.copies * n_bins <= 512) P.copies *= 2;
  vg_choose_grid(n, dim, lo, hi, h_max, &P.g, P.reach);
  for (int k = 0; k < 3; k++) P.shift[k] = shift[k];
  const size_t pair_blocks = (n + VG_THREADS - 1) / VG_THREADS;
  P.split = (int)((2048 + pair_blocks - 1) / pair_blocks);
  P.split = P.split > 16 ? 16 : P.split;
  REQUIRE(ctx, P.w > 0.0, ST_EINVAL);                  /* h_max / n_bins underflowed */
  size_t ncell = 1;
  for (int c = 0; c < dim; c++) ncell *= (size_t)P.g;
  REQUIRE(ctx, ncell <= ncell_max, ST_EFAILED);
  void *tmp = NULL;
  st = sinterp_sortbuf2(ctx, n * 8, &tmp);
  if (st) return st;
  unsigned *cellid = (unsigned *)tmp, *slot = cellid + n;
  st = sinterp_grid_bin(ctx, d_x, n, dim, xtda, P.g, grid, d_box, off, cellid, slot);
  if (st) return st;
  with_dim(dim, [&](auto D) {
    hipLaunchKernelGGL((vg_gather_kernel<decltype(D)::value>), dim3((unsigned)blocks), dim3(256), 0, ctx->stream, d_x, n, xtda, d_f,
                       (const unsigned *)cellid, (const unsigned *)slot, (const unsigned *)off, rec, cell_at);
  });
  LAUNCH_CHECK(ctx);

  /* ---- the pairs */
  HIP_OK(ctx, hipMemsetAsync(d_acc, 0, (size_t)n_bins * VG_WORDS * sizeof(vg_u64), ctx->stream));
  const size_t lds = ((size_t)n_bins + 1) * sizeof(double) + ((size_t)n_bins * VG_WORDS * P.copies + 1) * sizeof(vg_u64);
  with_dim(dim, [&](auto D) {
    hipLaunchKernelGGL((vg_pair_kernel<decltype(D)::value>), dim3((unsigned)pair_blocks, (unsigned)P.split), dim3(VG_THREADS), lds,
                       ctx->stream, P, (unsigned)n, (const unsigned *)off, (const unsigned *)cell_at, (const double *)rec, d_acc, d_tested);
  });
  LAUNCH_CHECK(ctx);
  HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
  HIP_OK(ctx, hipMemcpy(acc, d_acc, (size_t)n_bins * VG_WORDS * sizeof(vg_u64), hipMemcpyDeviceToHost));
  HIP_OK(ctx, hipMemcpy(&ctx->vg_pairs_tested, d_tested, sizeof(vg_u64), hipMemcpyDeviceToHost));
  return ST_SUCCESS;
}

extern "C" unsigned long long gsl_sinterp_hip_variogram_pairs_tested(const gsl_sinterp_hip_ctx *ctx) { return ctx ? ctx->vg_pairs_tested : 0; }

/* the bounding box of the sites as doubles, box[2c] = min and box[2c + 1] = max of coordinate c < dim (the facade's
   default cut-off is a third of its diagonal); NaN coordinates are skipped, n = 0 gives GSL_EINVAL */
extern "C" int gsl_sinterp_hip_bbox(gsl_sinterp_hip_ctx *ctx, const double *d_x, size_t n, int dim, size_t xtda, double *box)
{
  REQUIRE(ctx, dim >= 1 && dim <= 3 && xtda >= (size_t)dim && n >= 1, ST_EINVAL);
  REQUIRE(ctx, ctx != NULL && d_x != NULL && box != NULL, ST_EFAULT);
  HIP_OK(ctx, hipSetDevice(ctx->device));
  vg_u64 keys[6], *d_box = (vg_u64 *)((char *)ctx->d_scratch + 1024);
  int st = sinterp_bbox_keys(ctx, d_x, n, xtda, dim, d_box);
  if (st) return st;
  HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
  HIP_OK(ctx, hipMemcpy(keys, d_box, sizeof keys, hipMemcpyDeviceToHost));
  for (int c = 0; c < 2 * dim; c++) box[c] = vg_unkey(keys[c]);
  return ST_SUCCESS;
}
