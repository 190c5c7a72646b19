/*
 * shepard.hip -- Renka's modified quadratic Shepard method (ACM TOMS 660 / 661, the Franke-Nielson construction) in 2-D
 * and 3-D: a C1 interpolant of scattered data that is local, needs no mesh, no solve and no shape parameter, reproduces
 * quadratics and has an analytic gradient ("Modified Shepard").
 *
 *   s(y) = sum_i W_i(y) Q_i(y) / sum_i W_i(y),
 *   W_i(y) = ((Rw_i - r_i)_+ / (Rw_i r_i))^2,   r_i = |y - x_i|,
 *   Q_i(y) = f_i + c_i . m((y - x_i) / Rq_i),   m(u) = (u_0 .. u_{d-1}, u_a u_b for a <= b, row-major).
 *
 *   shepard_fit_kernel     one wave per node.  The k = max(nq, nw) + 2 nearest sites come from gsl_sinterp_hip_knn (slot 0
 *                          is the node itself); Rq, Rw are the distances to the (nq + 1)-th, (nw + 1)-th nearest OTHER site
 *                          and only sites STRICTLY inside Rq enter the fit (a site on the radius has weight 0, so nothing
 *                          depends on how the search broke a tie).  Lane j holds row j of the weighted design matrix
 *                          omega_ij m((x_j - x_i) / Rq_i), omega = (Rq - r) / (Rq r), and the right-hand side
 *                          omega (f_j - f_i).  Columns are scaled to unit 2-norm, then nc Householder steps in the fixed
 *                          column order (no pivoting: the leading d x d block of R is the R of the linear fit), every
 *                          sum the fixed 64-lane butterfly.  Rank rule on rho(k) = min |R_jj| / max |R_jj|, j < k:
 *                          rho(nc) >= sqrt(eps) quadratic, else rho(d) >= sqrt(eps) linear, else constant.
 *   shepard_pack (once     the nodes binned by sinterp_grid_bin (local.hip); records {x[d], f, Rw, 1/Rq, c[nc]} (80 B in 2-D,
 *   per model)             128 B in 3-D) in cell order and ROW order inside a cell; per cell the box of its nodes and its
 *                          largest Rw; the largest Rw of all.
 *   shepard_sweep_kernel   one target per lane: the cells of the index block that covers y +- max Rw, a cell skipped when
 *                          its box is farther than its own largest Rw, the records of a cell in row order.
 *
 * Summation order and the cull.  A record takes part iff r2 < fl(Rw^2) and Rw - sqrt(r2) > 0, r2 the FMA chain of the
 * other sweeps.  A record that does not take part adds nothing, so the sums are those of the participating records in
 * (cell, row) order -- a function of (model, target) alone -- PROVIDED the two culls never drop a participating record:
 *   cell box    per axis gap_c = max(lo_c - y_c, y_c - hi_c, 0) over the box [lo, hi] of the cell's own nodes.  For a node
 *               in it |fl(y_c - x_c)| >= gap_c (rounding is monotone), and the chain lb2 = fma(gap_c, gap_c, lb2) is below
 *               the node's r2 term by term.  The cell is skipped when lb2 >= fl(Rmax_cell^2) >= fl(Rw_i^2): then r2 >=
 *               fl(Rw_i^2) and the record would have failed the first test.
 *   index block lk_axis_cell is non-decreasing and bins the nodes too (local_grid.h, "The cell-function contract": that
 *               also says why the binning, compiled with contraction on, and the queries made here agree), so a node in a
 *               cell below a_c = cell(t), t = fl(y_c - R'), has x_c < t and fl(y_c - x_c) >= fl(y_c - t); the block starts
 *               at a_c only when fl(y_c - t) >= Rmax was CHECKED (otherwise at 0), and then r2 >= fl(Rmax^2) >= fl(Rw_i^2)
 *               again.  The high side is symmetric.
 * The slots that the binning hands out come from atomics and vary from run to run; this pack ranks the rows of a cell
 * instead.  Value and value + gradient are one body (GRAD), contraction is off and every fused operation is written out,
 * so the value bits do not depend on GRAD.
 */
#include "common.h"
#include <math.h>
#include <float.h>
#include <type_traits>
#include "chol_potrf.h"
#include "local_grid.h"

#pragma clang fp contract(off)

#define SH_HEAD 256                /* bytes: LkGrid | box keys at 64 | outside counter (64 bits) at 128 | largest Rw (bits) at 136 */
#define SH_FIT_CHUNK 8192          /* nodes per neighbour search of the fit: at most 64 x 12 bytes each */
#define SH_SQRT_EPS 1.4901161193847656e-08   /* GSL_SQRT_DBL_EPSILON */
#define SH_FIT_ID 0xffffffffffffffffULL      /* model id under which the fit keeps local.hip's pack between its chunks */

template <int DIM> struct ShDim {
  static constexpr int NC = DIM == 2 ? 5 : 9;          /* monomials */
  static constexpr int RECD = DIM == 2 ? 10 : 16;      /* doubles per record */
};

__device__ __forceinline__ double sh_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

/* ---- fit ------------------------------------------------------------------------------------------------------------ */
/* block b fits node node0 + b from row b of idx / r2 (k entries each, ascending key, slot 0 the node itself).
   counts: [0] linear fallbacks, [1] constant fallbacks, [2] nodes with a coincident site (outputs NaN). */
template <int DIM>
__global__ void __launch_bounds__(64)
shepard_fit_kernel(const double *__restrict__ x, size_t xtda, const double *__restrict__ f, size_t node0, int k,
                   const int *__restrict__ idx, const double *__restrict__ r2v, int nq, int nw, double *__restrict__ rq,
                   double *__restrict__ rw, double *__restrict__ coef, unsigned *__restrict__ counts)
{
  constexpr int NC = ShDim<DIM>::NC;
  const int lane = threadIdx.x;
  const size_t i = node0 + blockIdx.x;
  const int *id = idx + (size_t)blockIdx.x * (size_t)k;
  const double *rr = r2v + (size_t)blockIdx.x * (size_t)k;
  const double r2_near = rr[1];                        /* the nearest OTHER site (uniform) */
  if (!(r2_near > 0.0)) {                              /* coincident (or no neighbour at all: a NaN coordinate) */
    if (lane == 0) { rq[i] = sh_nan(); rw[i] = sh_nan(); atomicAdd(&counts[2], 1u); }
    if (lane < NC) coef[i * NC + lane] = sh_nan();
    return;
  }
  const double Rq = sqrt(rr[nq + 1]), Rw = sqrt(rr[nw + 1]);
  const double inv_rq = 1.0 / Rq;
  double a[NC], b = 0.0;
#pragma unroll
  for (int c = 0; c < NC; c++) a[c] = 0.0;
  if (lane >= 1 && lane < k && id[lane] >= 0) {
    const size_t j = (size_t)id[lane];
    const double r = sqrt(rr[lane]);
    if (r < Rq) {
      const double w = (Rq - r) / (Rq * r);
      double u[DIM];
#pragma unroll
      for (int c = 0; c < DIM; c++) u[c] = (x[j * xtda + c] - x[i * xtda + c]) * inv_rq;
#pragma unroll
      for (int c = 0; c < DIM; c++) a[c] = w * u[c];
      int q = DIM;
#pragma unroll
      for (int c = 0; c < DIM; c++)
#pragma unroll
        for (int e = c; e < DIM; e++) a[q++] = w * (u[c] * u[e]);
      b = w * (f[j] - f[i]);
    }
  }
  /* columns to unit 2-norm; a zero column stays zero and its R_jj = 0 makes the fit deficient */
  double nrm[NC];
#pragma unroll
  for (int c = 0; c < NC; c++) {
    nrm[c] = sqrt(lk_sum(a[c] * a[c]));
    if (nrm[c] > 0.0) a[c] = a[c] / nrm[c];
  }
  /* Householder, rows = lanes, pivot row of column c = lane c.  Afterwards R_jc (j < c) is lane j's a[c], R_cc = diag[c]
     and lane j < NC holds (Q^T b)_j */
  double diag[NC];
#pragma unroll
  for (int c = 0; c < NC; c++) {
    const double xv = lane >= c ? a[c] : 0.0;
    const double sigma = lk_sum(xv * xv);
    const double xc = lane_bcast(a[c], c);
    const double len = sqrt(sigma);
    const double alpha = xc > 0.0 ? -len : len;
    diag[c] = alpha;
    if (sigma > 0.0) {                                 /* uniform */
      const double v = lane == c ? xv - alpha : xv;    /* |v_c| = |x_c| + len: no cancellation */
      const double vtv = 2.0 * fma(fabs(xc), len, sigma);
#pragma unroll
      for (int e = c + 1; e < NC; e++) {
        const double tau = 2.0 * lk_sum(v * a[e]) / vtv;   /* v = 0 in the lanes above the pivot row */
        a[e] = fma(-tau, v, a[e]);
      }
      const double tau = 2.0 * lk_sum(v * b) / vtv;
      b = fma(-tau, v, b);
    }
  }
  double dmin = INFINITY, dmax = 0.0, lmin = INFINITY, lmax = 0.0;
#pragma unroll
  for (int c = 0; c < NC; c++) {
    const double d = fabs(diag[c]);
    dmin = fmin(dmin, d); dmax = fmax(dmax, d);
    if (c < DIM) { lmin = fmin(lmin, d); lmax = fmax(lmax, d); }
  }
  const int ncol = dmin / dmax >= SH_SQRT_EPS ? NC : (lmin / lmax >= SH_SQRT_EPS ? DIM : 0);   /* NaN (0 / 0) compares false */
  /* back substitution on the leading ncol x ncol block (every lane, the same bits), then the column scaling undone */
  double z[NC];
#pragma unroll
  for (int c = 0; c < NC; c++) z[c] = 0.0;
#pragma unroll
  for (int j = NC - 1; j >= 0; j--) {
    double s = lane_bcast(b, j);
#pragma unroll
    for (int e = j + 1; e < NC; e++) s = fma(-lane_bcast(a[e], j), z[e], s);     /* z[e] = 0 for e >= ncol */
    z[j] = j < ncol ? s / diag[j] : 0.0;
  }
#pragma unroll
  for (int c = 0; c < NC; c++)
    if (lane == c) coef[i * NC + c] = c < ncol ? z[c] / nrm[c] : 0.0;
  if (lane == 0) {
    rq[i] = Rq; rw[i] = Rw;
    if (ncol == DIM) atomicAdd(&counts[0], 1u);
    if (ncol == 0) atomicAdd(&counts[1], 1u);
  }
}

/* ---- pack ----------------------------------------------------------------------------------------------------------- */
/* the rows of every cell, in the order the binning's atomics handed out (not kept: sh_record_kernel ranks them) */
__global__ void __launch_bounds__(256)
sh_scatter_kernel(size_t n, const unsigned *__restrict__ cellid, const unsigned *__restrict__ slot, const unsigned *__restrict__ offset,
                  int *__restrict__ unordered)
{
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) unordered[offset[cellid[i]] + slot[i]] = (int)i;
}

/* one thread per node: its place in its cell = the number of smaller rows there; then its record */
template <int DIM>
__global__ void __launch_bounds__(256)
sh_record_kernel(const double *__restrict__ x, size_t n, size_t xtda, const double *__restrict__ f, const double *__restrict__ rq,
                 const double *__restrict__ rw, const double *__restrict__ coef, const unsigned *__restrict__ cellid,
                 const unsigned *__restrict__ offset, const int *__restrict__ unordered, int *__restrict__ rows, double *__restrict__ rec)
{
  constexpr int NC = ShDim<DIM>::NC, RECD = ShDim<DIM>::RECD;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const unsigned cell = cellid[i];
    const unsigned b = offset[cell], e = offset[cell + 1];
    unsigned rank = 0;
    for (unsigned p = b; p < e; p++) rank += (size_t)unordered[p] < i;
    const size_t p = (size_t)b + rank;
    rows[p] = (int)i;
    double *r = rec + p * RECD;
#pragma unroll
    for (int c = 0; c < DIM; c++) r[c] = x[i * xtda + c];
    r[DIM] = f[i]; r[DIM + 1] = rw[i]; r[DIM + 2] = 1.0 / rq[i];
#pragma unroll
    for (int c = 0; c < NC; c++) r[DIM + 3 + c] = coef[i * NC + c];
#pragma unroll
    for (int c = DIM + 3 + NC; c < RECD; c++) r[c] = 0.0;
  }
}

/* one thread per cell: {lo[3], hi[3], largest Rw, 0}; an empty cell has largest Rw 0 and is never entered */
template <int DIM>
__global__ void __launch_bounds__(256)
sh_cell_kernel(size_t ncell, const unsigned *__restrict__ offset, const double *__restrict__ rec, double *__restrict__ stat,
               unsigned long long *__restrict__ rmax_bits)
{
  constexpr int RECD = ShDim<DIM>::RECD;
  const size_t cell = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (cell >= ncell) return;
  double lo[3] = {0.0, 0.0, 0.0}, hi[3] = {0.0, 0.0, 0.0}, big = 0.0;
  const unsigned b = offset[cell], e = offset[cell + 1];
  for (unsigned p = b; p < e; p++) {
    const double *r = rec + (size_t)p * RECD;
#pragma unroll
    for (int c = 0; c < DIM; c++) {
      lo[c] = p == b ? r[c] : fmin(lo[c], r[c]);
      hi[c] = p == b ? r[c] : fmax(hi[c], r[c]);
    }
    if (r[DIM + 1] > big) big = r[DIM + 1];
  }
  double *o = stat + cell * 8;
#pragma unroll
  for (int c = 0; c < 3; c++) { o[c] = lo[c]; o[3 + c] = hi[c]; }
  o[6] = big; o[7] = 0.0;
  if (big > 0.0) atomicMax(rmax_bits, (unsigned long long)__double_as_longlong(big));   /* positive doubles order as their bits */
}

/* ---- sweep ---------------------------------------------------------------------------------------------------------- */
template <int DIM, bool GRAD>
__global__ void __launch_bounds__(256)
shepard_sweep_kernel(const LkGrid *__restrict__ grid, int g, const unsigned *__restrict__ off, const double *__restrict__ stat,
                     const int *__restrict__ rows, const double *__restrict__ rec, const unsigned long long *__restrict__ rmax_bits,
                     const double *__restrict__ yv, size_t ytda, size_t m, const int *__restrict__ perm, double *__restrict__ sout,
                     double *__restrict__ gout, size_t gtda, int *__restrict__ leaf, unsigned long long *__restrict__ n_outside)
{
  constexpr int RECD = ShDim<DIM>::RECD;
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= m) return;
  const size_t t = perm ? (size_t)perm[k] : k;
  double y[DIM];
  bool isnan_y = false;
#pragma unroll
  for (int c = 0; c < DIM; c++) { y[c] = yv[t * ytda + c]; isnan_y |= y[c] != y[c]; }
  double s = sh_nan(), gr[DIM];
#pragma unroll
  for (int c = 0; c < DIM; c++) gr[c] = sh_nan();
  int count = 0;
  if (!isnan_y) {
    const LkGrid G = *grid;
    const double rmax = __longlong_as_double((long long)*rmax_bits), rwide = rmax * (1.0 + 1e-7);
    int ia[3] = {0, 0, 0}, ib[3] = {0, 0, 0};
#pragma unroll
    for (int c = 0; c < DIM; c++) {
      const double tl = y[c] - rwide, th = y[c] + rwide;
      ia[c] = y[c] - tl >= rmax ? lk_axis_cell(tl, G.lo[c], G.hi[c], g) : 0;
      ib[c] = th - y[c] >= rmax ? lk_axis_cell(th, G.lo[c], G.hi[c], g) : g - 1;
    }
    double sw = 0.0, swq = 0.0, ga[DIM], gb[DIM], gc[DIM];
#pragma unroll
    for (int c = 0; c < DIM; c++) { ga[c] = 0.0; gb[c] = 0.0; gc[c] = 0.0; }
    double best_r2 = INFINITY;
    unsigned best_p = 0;
    for (int i2 = ia[2]; i2 <= ib[2]; i2++)
      for (int i1 = ia[1]; i1 <= ib[1]; i1++)
        for (int i0 = ia[0]; i0 <= ib[0]; i0++) {
          const size_t cell = ((size_t)i2 * (size_t)g + (size_t)i1) * (size_t)g + (size_t)i0;
          const double *cs = stat + cell * 8;
          double lb2 = 0.0;
#pragma unroll
          for (int c = 0; c < DIM; c++) {
            const double gap = fmax(fmax(cs[c] - y[c], y[c] - cs[3 + c]), 0.0);
            lb2 = fma(gap, gap, lb2);
          }
          const double big = cs[6];
          if (lb2 >= big * big) continue;              /* also every empty cell: big = 0 */
          const unsigned pe = off[cell + 1];
          for (unsigned p = off[cell]; p < pe; p++) {
            const double *r = (const double *)__builtin_assume_aligned(rec + (size_t)p * RECD, 16);
            double d[DIM], r2 = 0.0;
#pragma unroll
            for (int c = 0; c < DIM; c++) { d[c] = y[c] - r[c]; r2 = fma(d[c], d[c], r2); }
            const double Rw = r[DIM + 1];
            if (!(r2 < Rw * Rw)) continue;
            const double rr = sqrt(r2), tt = Rw - rr;
            if (!(tt > 0.0)) continue;
            const double w = tt / (Rw * rr), W = w * w;
            if (!(W > 0.0)) continue;                  /* w * w underflowed */
            count++;
            if (r2 < best_r2 || (r2 == best_r2 && rows[p] < rows[best_p])) { best_r2 = r2; best_p = p; }
            const double fi = r[DIM], inv_rq = r[DIM + 2];
            double u[DIM];
#pragma unroll
            for (int c = 0; c < DIM; c++) u[c] = d[c] * inv_rq;
            /* Q = f + sum c_a u_a + sum c_ab u_a u_b; dq[a] = dQ/du_a */
            double Q = fi, dq[DIM];
#pragma unroll
            for (int c = 0; c < DIM; c++) { Q = fma(r[DIM + 3 + c], u[c], Q); dq[c] = r[DIM + 3 + c]; }
            int q = DIM + 3 + DIM;
#pragma unroll
            for (int c = 0; c < DIM; c++)
#pragma unroll
              for (int e = c; e < DIM; e++) {
                const double cq = r[q++];
                Q = fma(cq, u[c] * u[e], Q);
                if (GRAD) { dq[c] = fma(cq, u[e], dq[c]); dq[e] = fma(cq, u[c], dq[e]); }
              }
            sw += W;
            swq = fma(W, Q, swq);
            if (GRAD) {
              const double h = -2.0 * w / (r2 * rr);   /* grad W = h (y - x) */
#pragma unroll
              for (int c = 0; c < DIM; c++) {
                const double gw = h * d[c];
                ga[c] = fma(W, dq[c] * inv_rq, ga[c]);
                gb[c] = fma(Q, gw, gb[c]);
                gc[c] += gw;
              }
            }
          }
        }
    if (count > 0) {
      if (best_r2 == 0.0 || !(sw < INFINITY)) {        /* on a node, or within ~1e-154 of one: that node's value and gradient */
        const double *r = rec + (size_t)best_p * RECD;
        s = r[DIM];
#pragma unroll
        for (int c = 0; c < DIM; c++) gr[c] = r[DIM + 3 + c] * r[DIM + 2];
        if (best_r2 == 0.0) count = 1;
      } else {
        s = swq / sw;
        if (GRAD) {
#pragma unroll
          for (int c = 0; c < DIM; c++) gr[c] = (ga[c] + fma(-s, gc[c], gb[c])) / sw;
        }
      }
    } else {
      atomicAdd(n_outside, 1ULL);
    }
  }
  if (sout) sout[t] = s;
  if (GRAD) {
#pragma unroll
    for (int c = 0; c < DIM; c++) gout[t * gtda + c] = gr[c];
  }
  if (leaf) leaf[t] = count > 0 ? count : -1;
}

/* ---- host ----------------------------------------------------------------------------------------------------------- */
struct sh_model {
  const LkGrid *grid;
  const unsigned *off;
  const double *stat;
  const int *rows;
  const double *rec;
  unsigned long long *n_outside;
  const unsigned long long *rmax_bits;
  int g;
};

template <class F> static void sh_with_dim(int dim, F &&f)
{
  if (dim == 2) f(std::integral_constant<int, 2>());
  else f(std::integral_constant<int, 3>());
}

/* the packed nodes, cached per model like local.hip's */
static int shepard_pack(gsl_sinterp_hip_ctx *ctx, const double *d_x, size_t n, int dim, size_t xtda, const double *d_f, const double *d_rq,
                        const double *d_rw, const double *d_coef, unsigned long long model_id, sh_model *out)
{
  gsl_sinterp_hip_ctx::CentKey &key = ctx->shep_key;
  const bool cached = sinterp_key_vouches(key, model_id, d_x, d_coef, n, xtda, dim);
  const int g = cached ? ctx->shep_g : lk_grid_size(n, dim);
  size_t ncell = 1;
  for (int c = 0; c < dim; c++) ncell *= (size_t)g;
  const size_t recd = dim == 2 ? ShDim<2>::RECD : ShDim<3>::RECD;
  const size_t off_bytes = round_up(lk_off_words(ncell) * 4, 16), stat_bytes = ncell * 8 * sizeof(double);
  const size_t rows_bytes = round_up(n * sizeof(int), 16);
  const size_t bytes = SH_HEAD + off_bytes + stat_bytes + rows_bytes + n * recd * sizeof(double);
  if (!cached) key.id = 0;                         /* the buffer may move or be rewritten */
  void *buf = NULL;
  int st = sinterp_shepbuf(ctx, bytes, &buf);
  if (st) return st;
  char *b = (char *)buf;
  LkGrid *grid = (LkGrid *)b;
  unsigned *off = (unsigned *)(b + SH_HEAD);
  double *stat = (double *)(b + SH_HEAD + off_bytes);
  int *rows = (int *)(b + SH_HEAD + off_bytes + stat_bytes);
  double *rec = (double *)(b + SH_HEAD + off_bytes + stat_bytes + rows_bytes);
  unsigned long long *rmax_bits = (unsigned long long *)(b + 136);
  out->grid = grid; out->off = off; out->stat = stat; out->rows = rows; out->rec = rec; out->n_outside = (unsigned long long *)(b + 128);
  out->rmax_bits = rmax_bits; out->g = g;
  if (cached) return ST_SUCCESS;
  void *tmp = NULL;
  st = sinterp_sortbuf2(ctx, 3 * n * 4, &tmp);
  if (st) return st;
  unsigned *cellid = (unsigned *)tmp, *slot = cellid + n;
  int *unordered = (int *)(slot + n);
  st = sinterp_grid_bin(ctx, d_x, n, dim, xtda, g, grid, (unsigned long long *)(b + 64), off, cellid, slot);
  if (st) return st;
  HIP_OK(ctx, hipMemsetAsync(rmax_bits, 0, sizeof *rmax_bits, ctx->stream));
  size_t blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(sh_scatter_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, n, (const unsigned *)cellid, (const unsigned *)slot,
                     (const unsigned *)off, unordered);
  sh_with_dim(dim, [&](auto D) {
    constexpr int DIM = decltype(D)::value;
    hipLaunchKernelGGL((sh_record_kernel<DIM>), dim3((unsigned)blocks), dim3(256), 0, ctx->stream, d_x, n, xtda, d_f, d_rq, d_rw, d_coef,
                       (const unsigned *)cellid, (const unsigned *)off, (const int *)unordered, rows, rec);
    hipLaunchKernelGGL((sh_cell_kernel<DIM>), dim3((unsigned)((ncell + 255) / 256)), dim3(256), 0, ctx->stream, ncell, (const unsigned *)off,
                       (const double *)rec, stat, rmax_bits);
  });
  LAUNCH_CHECK(ctx);
  ctx->shep_g = g;
  ctx->shep_packs++;
  sinterp_key_set(key, model_id, d_x, d_coef, n, xtda, dim);
  return ST_SUCCESS;
}

extern "C" int gsl_sinterp_hip_shepard_fit(gsl_sinterp_hip_ctx *ctx, const double *d_x, size_t n, int dim, size_t xtda, const double *d_f,
                                           size_t nq, size_t nw, double *d_rq, double *d_rw, double *d_coef, size_t *h_counts)
{
  if (h_counts) h_counts[0] = h_counts[1] = h_counts[2] = 0;
  /* the arguments first: nothing here touches the device */
  REQUIRE(ctx, dim == 2 || dim == 3, ST_EINVAL);
  const size_t nc = dim == 2 ? ShDim<2>::NC : ShDim<3>::NC, k = (nq > nw ? nq : nw) + 2;
  REQUIRE(ctx, nq >= nc && nw >= 1 && nq <= 62 && nw <= 62 && k <= n && n <= 0x7fffffffULL && xtda >= (size_t)dim, ST_EINVAL);
  REQUIRE(ctx, ctx != NULL && d_x != NULL && d_f != NULL && d_rq != NULL && d_rw != NULL && d_coef != NULL, ST_EFAULT);
  HIP_OK(ctx, hipSetDevice(ctx->device));
  const size_t chunk = n < SH_FIT_CHUNK ? n : SH_FIT_CHUNK;
  const size_t idx_bytes = round_up(chunk * k * sizeof(int), 256);
  void *buf = NULL;
  int st = sinterp_workspace(ctx, 256 + idx_bytes + chunk * k * sizeof(double), &buf);
  if (st) return st;
  unsigned *counts = (unsigned *)buf;
  int *idx = (int *)((char *)buf + 256);
  double *r2 = (double *)((char *)buf + 256 + idx_bytes);
  HIP_OK(ctx, hipMemsetAsync(counts, 0, 3 * sizeof(unsigned), ctx->stream));
  ctx->local_key.id = 0;                               /* the search's pack of the nodes: built by the first chunk, dropped at the end */
  for (size_t c0 = 0; c0 < n && !st; c0 += chunk) {
    const size_t mc = n - c0 < chunk ? n - c0 : chunk;
    st = gsl_sinterp_hip_knn(ctx, d_x, n, dim, xtda, d_x + c0 * xtda, mc, xtda, k, idx, r2, SH_FIT_ID);
    if (st) break;
    sh_with_dim(dim, [&](auto D) {
      hipLaunchKernelGGL((shepard_fit_kernel<decltype(D)::value>), dim3((unsigned)mc), dim3(64), 0, ctx->stream, d_x, xtda, d_f, c0, (int)k,
                         (const int *)idx, (const double *)r2, (int)nq, (int)nw, d_rq, d_rw, d_coef, counts);
    });
  }
  ctx->local_key.id = 0;
  if (st) return st;
  LAUNCH_CHECK(ctx);
  unsigned h[3] = {0, 0, 0};
  HIP_OK(ctx, hipMemcpyAsync(h, counts, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
  HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
  ctx->shep_fits++;
  if (h_counts) { h_counts[0] = h[0]; h_counts[1] = h[1]; h_counts[2] = h[2]; }
  if (h[2])
    return sinterp_fail(ctx, ST_EDOM, "shepard_fit: coincident sites (the weights of a node whose nearest other site is at distance 0 are undefined)",
                        hipSuccess, __FILE__, __LINE__);
  return ST_SUCCESS;
}

extern "C" int gsl_sinterp_hip_shepard_eval(gsl_sinterp_hip_ctx *ctx, const double *d_x, size_t n, int dim, size_t xtda, const double *d_f,
                                            const double *d_rq, const double *d_rw, const double *d_coef, const double *d_y, size_t m,
                                            size_t ytda, double *d_s, double *d_g, size_t gtda, int *d_leaf, size_t *h_n_outside,
                                            unsigned long long model_id)
{
  if (h_n_outside) *h_n_outside = 0;
  REQUIRE(ctx, dim == 2 || dim == 3, ST_EINVAL);
  REQUIRE(ctx, n >= 1 && n <= 0x7fffffffULL && m <= 0x7fffffffULL && xtda >= (size_t)dim && ytda >= (size_t)dim, ST_EINVAL);
  REQUIRE(ctx, d_g == NULL || gtda >= (size_t)dim, ST_EINVAL);
  REQUIRE(ctx, ctx != NULL && d_x != NULL && d_f != NULL && d_rq != NULL && d_rw != NULL && d_coef != NULL && (m == 0 || d_y != NULL), ST_EFAULT);
  if (m == 0 || (!d_s && !d_g && !d_leaf)) return ST_SUCCESS;
  HIP_OK(ctx, hipSetDevice(ctx->device));
  sh_model sm;
  int st = shepard_pack(ctx, d_x, n, dim, xtda, d_f, d_rq, d_rw, d_coef, model_id, &sm);
  if (st) return st;
  int *perm = NULL;                                    /* large batches in cell order: the lanes of a wave read the same records */
  if (m >= LK_SORT_MIN) {
    st = sinterp_sort_targets(ctx, d_y, m, ytda, dim, 64, &perm);
    if (st) return st;
  }
  HIP_OK(ctx, hipMemsetAsync(sm.n_outside, 0, sizeof *sm.n_outside, ctx->stream));
  const dim3 grid((unsigned)((m + 255) / 256)), block(256);
  sh_with_dim(dim, [&](auto D) {
    constexpr int DIM = decltype(D)::value;
    if (d_g)
      hipLaunchKernelGGL((shepard_sweep_kernel<DIM, true>), grid, block, 0, ctx->stream, sm.grid, sm.g, sm.off, sm.stat, sm.rows, sm.rec,
                         sm.rmax_bits, d_y, ytda, m, (const int *)perm, d_s, d_g, gtda, d_leaf, sm.n_outside);
    else
      hipLaunchKernelGGL((shepard_sweep_kernel<DIM, false>), grid, block, 0, ctx->stream, sm.grid, sm.g, sm.off, sm.stat, sm.rows, sm.rec,
                         sm.rmax_bits, d_y, ytda, m, (const int *)perm, d_s, (double *)NULL, (size_t)0, d_leaf, sm.n_outside);
  });
  LAUNCH_CHECK(ctx);
  /* the uncovered targets are the status: with h_n_outside it waits for the batch (everything else has been stored by
     then); without, the call stays asynchronous and the caller reads NaN / -1 */
  long long outside = 0;
  st = sinterp_outside_count(ctx, sm.n_outside, h_n_outside ? &outside : NULL,
                             "shepard_eval: target(s) outside every node's radius of influence (value and gradient NaN, leaf -1 there)");
  if (h_n_outside) *h_n_outside = (size_t)outside;
  return st;
}

extern "C" unsigned long long gsl_sinterp_hip_shepard_pack_count(const gsl_sinterp_hip_ctx *ctx) { return ctx ? ctx->shep_packs : 0ULL; }
extern "C" unsigned long long gsl_sinterp_hip_shepard_fit_count(const gsl_sinterp_hip_ctx *ctx) { return ctx ? ctx->shep_fits : 0ULL; }
