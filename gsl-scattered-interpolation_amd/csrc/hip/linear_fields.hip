/*
 * linear_fields.hip -- K responses and their per-simplex gradients on the piecewise-linear types, from ONE locate.
 *
 * A third consumer of d_located, next to natural.hip and cubic.hip: the unchanged linear path (bary.hip: DAG or
 * imported triangles; mesh3.hip: tetrahedra) locates every target once, and the sweep here turns the simplex it found
 * into nf values and, when asked, nf gradients.  Compiled with -ffp-contract=off like the locate kernels, and the
 * coordinates and the value come from the very lines they use (linear_finish.h: solve_node + BARY_INTERP, tet_coords +
 * TET_INTERP), so S[k][q] holds the bits the scalar kernel stores when its response table is bound to column q.
 *
 * No per-simplex response table is built: the dim + 1 vertex rows of F are gathered through the vertex ids.
 *
 * Shape.  The sweep moves bytes: per target one record and (dim + 1) nf gathered doubles in, nf (1 + dim) doubles out.
 * A workgroup takes 256 consecutive targets in two phases:
 *   1. one lane per target: record, coordinates, and what the gradient needs (2-D: the LU; 3-D: the inverse) into LDS,
 *      structure-of-arrays (conflict-free for neighbouring lanes, a broadcast when a wave shares a target);
 *   2. the lanes run over the (target, field) pairs of the 256 rows in row-major order: lane l of a pass holds pair
 *      p = pass * 256 + l, so the lanes of a wave read consecutive doubles of a vertex row of F and store consecutive
 *      doubles of S (and runs of dim doubles of G) -- whole 64-byte segments when stda = nf, whatever nf is; one lane per
 *      target with a loop over q would make every store of a wave a stride-stda scatter.
 * The vertex rows are read with 8-byte loads: an odd nf or ftda leaves a row 8-byte aligned only.
 *
 * Gradient of field q in the located simplex, raw coordinates, d_i = f_i - f_last (a cage vertex, or an id out of range,
 * carries 0 as in the value):
 *   2-D  record: P M = L U, M = the standardised edge matrix.  value = f_2 + d^T M^-1 b, b_a = s_a (y_a - x_a), so
 *        grad_a = s_a (M^-T d)_a = s_a (P^T L^-T U^-T d)_a: two triangular solves with the record's LU per field
 *        (backward stable: the error is relative to the gradient, not to |M^-1| |d|);
 *   3-D  record: inv = M^-1 (rows = coordinates).  grad_a = scale_a sum_i inv[3 i + a] d_i.
 * A function of (record, vertex rows) alone: every target of a simplex gets the same bits.
 */
#include "common.h"
#include "linear_finish.h"
#include <math.h>

#define LF_ROWS 256                 /* targets per workgroup = lanes */
#define LF_VALID 8                  /* flag bits 0-2: BARY_INTERP's mask; 3: located; 4: rows of the LU swapped */
#define LF_SWAPPED 16

__device__ __forceinline__ double lf_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

/* d_vert [3 n]: the DAG's pidx (insertion order, < 0 = cage) or the triangles of an imported mesh (row order) */
__global__ void __launch_bounds__(LF_ROWS)
bary_fields_kernel(int n_simplices, const NodeRec *__restrict__ rec, const int *__restrict__ vert, int n_points,
                   const double *__restrict__ F, unsigned nf, size_t ftda, double s0, double s1, const int *__restrict__ located,
                   const double *__restrict__ targets, size_t m, size_t ttda, double *__restrict__ S, size_t stda,
                   double *__restrict__ G, size_t gtda)
{
  __shared__ double s_c[2][LF_ROWS], s_lu[4][LF_ROWS];
  __shared__ int s_v[3][LF_ROWS], s_flag[LF_ROWS];
  const size_t base = (size_t)blockIdx.x * LF_ROWS;
  const unsigned lane = threadIdx.x;
  {
    const size_t k = base + lane;
    int flag = 0;
    if (k < m) {
      const int t = located[k];
      if (t >= 0 && t < n_simplices) {
        const NodeRec r = load_rec(rec, t);
        double c0, c1;
        solve_node(r, targets[k * ttda], targets[k * ttda + 1], s0, s1, c0, c1);
        s_c[0][lane] = c0; s_c[1][lane] = c1;
        s_lu[0][lane] = r.u00; s_lu[1][lane] = r.u01; s_lu[2][lane] = r.l10; s_lu[3][lane] = r.u11;
        flag = LF_VALID | (META_SWAPPED(r.meta) ? LF_SWAPPED : 0);
#pragma unroll
        for (int i = 0; i < 3; i++) {
          const int id = vert[3 * (size_t)t + i];
          const bool data = id >= 0 && id < n_points;              /* tree_bind_kernel's rule */
          s_v[i][lane] = data ? id : 0;
          if (data) flag |= 1 << i;
        }
      }
    }
    s_flag[lane] = flag;
  }
  __syncthreads();
  const size_t left = m - base;
  const unsigned rows = left < LF_ROWS ? (unsigned)left : LF_ROWS;
  const unsigned pairs = rows * nf;                                /* <= 256 * 64 */
  for (unsigned p = lane; p < pairs; p += LF_ROWS) {
    const unsigned kk = p / nf, q = p - kk * nf;
    const size_t k = base + kk;
    const int flag = s_flag[kk];
    if (!(flag & LF_VALID)) {
      S[k * stda + q] = lf_nan();
      if (G) { G[k * gtda + 2 * q] = lf_nan(); G[k * gtda + 2 * q + 1] = lf_nan(); }
      continue;
    }
    const double f0 = (flag & 1) ? F[(size_t)s_v[0][kk] * ftda + q] : 0.0;
    const double f1 = (flag & 2) ? F[(size_t)s_v[1][kk] * ftda + q] : 0.0;
    const double f2 = (flag & 4) ? F[(size_t)s_v[2][kk] * ftda + q] : 0.0;
    const double c0 = s_c[0][kk], c1 = s_c[1][kk];
    BARY_INTERP(interp, c0, c1, flag, f0, f1, f2);
    S[k * stda + q] = interp;
    if (G) {
      const double u00 = s_lu[0][kk], u01 = s_lu[1][kk], l10 = s_lu[2][kk], u11 = s_lu[3][kk];
      const double d0 = f0 - f2, d1 = f1 - f2;
      const double w0 = d0 / u00;                                  /* U^T w = d */
      const double w1 = (d1 - u01 * w0) / u11;
      const double v0 = w0 - l10 * w1;                             /* L^T v = w */
      const bool sw = flag & LF_SWAPPED;                           /* z = P^T v */
      G[k * gtda + 2 * q] = s0 * (sw ? w1 : v0);
      G[k * gtda + 2 * q + 1] = s1 * (sw ? v0 : w1);
    }
  }
}

struct LfGeom3 { double shift[3], scale[3]; };

__global__ void __launch_bounds__(LF_ROWS)
mesh3_fields_kernel(int n_tet, const TetRec *__restrict__ rec, const int *__restrict__ tet, int n_points,
                    const double *__restrict__ F, unsigned nf, size_t ftda, LfGeom3 geo, const int *__restrict__ located,
                    const double *__restrict__ targets, size_t m, size_t ttda, double *__restrict__ S, size_t stda,
                    double *__restrict__ G, size_t gtda)
{
  __shared__ double s_c[4][LF_ROWS], s_inv[9][LF_ROWS];
  __shared__ int s_v[4][LF_ROWS], s_flag[LF_ROWS];                 /* flag bits 0-3: vertex i carries a datum; 4: located */
  const size_t base = (size_t)blockIdx.x * LF_ROWS;
  const unsigned lane = threadIdx.x;
  {
    const size_t k = base + lane;
    int flag = 0;
    if (k < m) {
      const int t = located[k];
      if (t >= 0 && t < n_tet) {
        const TetRec r = load_tet(rec, t);
        const double z[3] = {geo.scale[0] * (targets[k * ttda] - geo.shift[0]), geo.scale[1] * (targets[k * ttda + 1] - geo.shift[1]),
                             geo.scale[2] * (targets[k * ttda + 2] - geo.shift[2])};
        double c[4];
        tet_coords(r, z, c);
#pragma unroll
        for (int i = 0; i < 4; i++) s_c[i][lane] = c[i];
#pragma unroll
        for (int i = 0; i < 9; i++) s_inv[i][lane] = r.inv[i];
        flag = 16;
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int id = tet[4 * (size_t)t + i];
          const bool data = id >= 0 && id < n_points;              /* mesh3_bind_kernel's rule */
          s_v[i][lane] = data ? id : 0;
          if (data) flag |= 1 << i;
        }
      }
    }
    s_flag[lane] = flag;
  }
  __syncthreads();
  const size_t left = m - base;
  const unsigned rows = left < LF_ROWS ? (unsigned)left : LF_ROWS;
  const unsigned pairs = rows * nf;
  for (unsigned p = lane; p < pairs; p += LF_ROWS) {
    const unsigned kk = p / nf, q = p - kk * nf;
    const size_t k = base + kk;
    const int flag = s_flag[kk];
    if (!(flag & 16)) {
      S[k * stda + q] = lf_nan();
      if (G) { G[k * gtda + 3 * q] = lf_nan(); G[k * gtda + 3 * q + 1] = lf_nan(); G[k * gtda + 3 * q + 2] = lf_nan(); }
      continue;
    }
    const double f0 = (flag & 1) ? F[(size_t)s_v[0][kk] * ftda + q] : 0.0;
    const double f1 = (flag & 2) ? F[(size_t)s_v[1][kk] * ftda + q] : 0.0;
    const double f2 = (flag & 4) ? F[(size_t)s_v[2][kk] * ftda + q] : 0.0;
    const double f3 = (flag & 8) ? F[(size_t)s_v[3][kk] * ftda + q] : 0.0;
    const double c[4] = {s_c[0][kk], s_c[1][kk], s_c[2][kk], s_c[3][kk]};
    S[k * stda + q] = TET_INTERP(c, f0, f1, f2, f3);
    if (G) {
      const double d0 = f0 - f3, d1 = f1 - f3, d2 = f2 - f3;
#pragma unroll
      for (int a = 0; a < 3; a++)
        G[k * gtda + 3 * q + a] = geo.scale[a] * ((s_inv[a][kk] * d0 + s_inv[3 + a][kk] * d1) + s_inv[6 + a][kk] * d2);
    }
  }
}

/* the checks both entries share; everything here precedes any work on the device */
static int lf_check(gsl_sinterp_hip_ctx *ctx, int n_simplices, const void *d_records, const int *d_vertices, int n_points, const double *d_F,
                    int nf, size_t ftda, const double *h_geom, const int *d_located, const double *d_targets, size_t m, size_t ttda,
                    double *d_S, size_t stda, double *d_G, size_t gtda, int dim, uintptr_t align)
{
  REQUIRE(ctx, nf >= 1 && nf <= GSL_SINTERP_MAX_FIELDS && ftda >= (size_t)nf && stda >= (size_t)nf, ST_EINVAL);
  REQUIRE(ctx, !d_G || gtda >= (size_t)nf * (size_t)dim, ST_EINVAL);
  REQUIRE(ctx, ttda >= (size_t)dim, ST_EINVAL);
  REQUIRE(ctx, n_simplices > 0 && n_points >= 0, ST_EINVAL);
  REQUIRE(ctx, d_records && d_vertices && d_F && h_geom && (m == 0 || (d_located && d_targets && d_S)), ST_EFAULT);
  REQUIRE(ctx, ((uintptr_t)d_records & align) == 0, ST_EINVAL);
  REQUIRE(ctx, m < 0xffffffffULL, ST_EINVAL);
  return ST_SUCCESS;
}

extern "C" int gsl_sinterp_hip_bary_fields_eval(gsl_sinterp_hip_ctx *ctx, int n_simplices, const void *d_records, const int *d_vertices,
                                                int n_points, const double *d_F, int nf, size_t ftda, const double *h_scale,
                                                const int *d_located, const double *d_targets, size_t m, size_t ttda, double *d_S,
                                                size_t stda, double *d_G, size_t gtda)
{
  REQUIRE(ctx, ctx != NULL, ST_EFAULT);
  int st = lf_check(ctx, n_simplices, d_records, d_vertices, n_points, d_F, nf, ftda, h_scale, d_located, d_targets, m, ttda, d_S, stda,
                    d_G, gtda, 2, 63);
  if (st) return st;
  if (m == 0) return ST_SUCCESS;
  HIP_OK(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(bary_fields_kernel, dim3((unsigned)((m + LF_ROWS - 1) / LF_ROWS)), dim3(LF_ROWS), 0, ctx->stream, n_simplices,
                     (const NodeRec *)d_records, d_vertices, n_points, d_F, (unsigned)nf, ftda, h_scale[0], h_scale[1], d_located, d_targets, m,
                     ttda, d_S, stda, d_G, gtda);
  LAUNCH_CHECK(ctx);
  return ST_SUCCESS;
}

extern "C" int gsl_sinterp_hip_mesh3_fields_eval(gsl_sinterp_hip_ctx *ctx, int n_tet, const void *d_records, const int *d_tet, int n_points,
                                                 const double *d_F, int nf, size_t ftda, const double *h_geom, const int *d_located,
                                                 const double *d_targets, size_t m, size_t ttda, double *d_S, size_t stda, double *d_G,
                                                 size_t gtda)
{
  REQUIRE(ctx, ctx != NULL, ST_EFAULT);
  int st = lf_check(ctx, n_tet, d_records, d_tet, n_points, d_F, nf, ftda, h_geom, d_located, d_targets, m, ttda, d_S, stda, d_G, gtda, 3,
                    127);
  if (st) return st;
  if (m == 0) return ST_SUCCESS;
  HIP_OK(ctx, hipSetDevice(ctx->device));
  LfGeom3 geo;
  for (int j = 0; j < 3; j++) { geo.shift[j] = h_geom[j]; geo.scale[j] = h_geom[3 + j]; }
  hipLaunchKernelGGL(mesh3_fields_kernel, dim3((unsigned)((m + LF_ROWS - 1) / LF_ROWS)), dim3(LF_ROWS), 0, ctx->stream, n_tet,
                     (const TetRec *)d_records, d_tet, n_points, d_F, (unsigned)nf, ftda, geo, d_located, d_targets, m, ttda, d_S, stda, d_G,
                     gtda);
  LAUNCH_CHECK(ctx);
  return ST_SUCCESS;
}

/* the route helper of the located sweeps, for callers outside this library's C++ (tests pick batch sizes on either
   side of the size at which the locate reorders its targets) */
extern "C" int gsl_sinterp_hip_sort_wanted(size_t m) { return sinterp_sort_wanted(m) ? 1 : 0; }
