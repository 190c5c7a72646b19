/*
 * cubic.hip -- Clough-Tocher C1 piecewise-cubic interpolation on a 2-D mesh, with gradients.
 *
 * Three steps ("Clough-Tocher"):
 *   1. vertex gradients g_i (Nielson / Renka's global estimator, as scipy's CloughTocher2DInterpolator): minimise the
 *      sum over the undirected mesh edges of the integral of (h'')^2, h the cubic Hermite along the edge.  With
 *      e = x_j - x_i, L = |e|, E = e e^T / L^3 that is the SPD system
 *          block (i, i) = sum_j 4 E,   block (i, j) = 2 E,   r_i = sum_j 6 (f_j - f_i) e / L^3,
 *      solved here by conjugate gradients preconditioned with the inverse 2x2 diagonal blocks.  A is never stored: one
 *      thread per vertex walks its row of the vertex -> neighbour CSR and forms E from the two points.  Every dot
 *      product is a two-stage reduction in a fixed order (256-wide tree per workgroup, then one workgroup over the
 *      partial sums), so the same mesh and data give the same bits from run to run.  alpha, beta and the stopping
 *      verdict live in a small record on the device (CtScal); once the verdict is in, the remaining launches of a
 *      batch return at once, so the host may look every few iterations without changing the result.
 *   2. cubic_pack_kernel: one 160-byte record per triangle -- the barycentric map and the 12 independent Bezier
 *      ordinates of the Clough-Tocher split; the 7 ordinates that are plain averages are rebuilt per target.
 *   3. cubic_sweep_kernel<GRAD>: one target per lane, in the triangle the linear path located.  With b the barycentric
 *      coordinates, b_min = b_j their smallest, a_i = b_i - b_min and a_4 = 3 b_min, the value is the cubic Bernstein
 *      form P(a) over the 19 ordinates.  The body forms the four quadratic forms Q_i = (dP/da_i) / 3 and returns
 *      s = sum a_i Q_i (Euler's identity for a cubic form), so value and gradient come from the same numbers and the
 *      value bits do not depend on GRAD.  Chain rule: ds/db_i = 3 Q_i (i != j), ds/db_j = 3 (3 Q_4 - sum_{i != j} Q_i).
 *
 * Built without FMA contraction (Makefile, HIP_EXACT_SRC): a value is a function of (mesh, f, g, target) alone.
 */
#include "common.h"
#include <math.h>

enum { ST_EMAXITER = 11 };

#define CT_FLAT_TOL 1e-14      /* natural.hip's rule: |orientation| <= tol * (sum of the squared edge lengths) */
#define CT_DIAG_TOL 1e-14      /* a diagonal block with det <= tol * d00 * d11 has no two non-collinear edges */
#define CT_CHECK_EVERY 8       /* iterations between two host looks at the stopping verdict */

/* ordinate slots of a record: the three vertex values, the six edge ordinates, the three interior ones */
enum { C3000, C0300, C0030, C2100, C2010, C1200, C0210, C1020, C0120, C0111, C1011, C1101, CT_NORD };

/* x0 = the third vertex; b_1 = m[0] dx + m[1] dy, b_2 = m[2] dx + m[3] dy, b_3 = 1 - b_1 - b_2 with (dx, dy) = y - x0.
   meta bit 0: flat (or bad vertex ids); then c[0], c[1] hold the gradient of the plane through the three data (NaN
   when there is none) and the value is the piecewise-linear one. */
struct __attribute__((aligned(16))) CtRec {
  double x0[2];
  double m[4];
  double c[CT_NORD];
  int meta, pad[3];
};
static_assert(sizeof(CtRec) == GSL_SINTERP_CUBIC_RECORD_BYTES, "Clough-Tocher record size");

struct CtScal {
  double rz[2];      /* r . z of the current / next iteration (slot = iteration & 1) */
  double pq, rr, bb;
  int done;          /* 0 running, 1 converged (or b = 0), 2 breakdown (p . A p <= 0) */
  int iters;
};

__device__ __forceinline__ double ct_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

/* sum of the workgroup's 256 values in a fixed order; every thread of the workgroup must call it */
__device__ __forceinline__ double ct_block_sum(double v, double *s)
{
  s[threadIdx.x] = v;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
    __syncthreads();
  }
  const double r = s[0];
  __syncthreads();
  return r;
}

/* ---- vertex gradients: PCG ------------------------------------------------------------------------------------- */

/* row i of the CSR, clamped to the arrays */
__device__ __forceinline__ void ct_row(const int *__restrict__ off, size_t n_adj, int i, size_t &e0, size_t &e1)
{
  const int a = off[i], b = off[i + 1];
  e0 = a < 0 ? 0 : (size_t)a;
  e1 = b < 0 ? 0 : (size_t)b;
  if (e1 > n_adj) e1 = n_adj;
  if (e0 > e1) e0 = e1;
}

/* diagonal blocks (inverted), right-hand side, x = 0, r = b, z = D^-1 r, p = z; partial sums of r . z and b . b */
__global__ void __launch_bounds__(256)
cubic_setup_kernel(int n, const int *__restrict__ off, const int *__restrict__ adj, size_t n_adj, const double *__restrict__ pts,
                   const double *__restrict__ f, double *__restrict__ dinv, double *__restrict__ x, double *__restrict__ r,
                   double *__restrict__ z, double *__restrict__ p, double *__restrict__ part_a, double *__restrict__ part_b)
{
  __shared__ double s[256];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  double rz = 0.0, bb = 0.0;
  if (i < n) {
    const double xi = pts[2 * (size_t)i], yi = pts[2 * (size_t)i + 1], fi = f[i];
    double d00 = 0.0, d01 = 0.0, d11 = 0.0, r0 = 0.0, r1 = 0.0;
    size_t e0, e1;
    ct_row(off, n_adj, i, e0, e1);
    for (size_t e = e0; e < e1; e++) {
      const int j = adj[e];
      if (j < 0 || j >= n || j == i) continue;
      const double ex = pts[2 * (size_t)j] - xi, ey = pts[2 * (size_t)j + 1] - yi;
      const double l2 = ex * ex + ey * ey;
      if (!(l2 > 0.0)) continue;
      const double l3 = l2 * sqrt(l2);
      d00 += 4.0 * ex * ex / l3; d01 += 4.0 * ex * ey / l3; d11 += 4.0 * ey * ey / l3;
      const double w = 6.0 * (f[j] - fi) / l3;
      r0 += w * ex; r1 += w * ey;
    }
    const double det = d00 * d11 - d01 * d01;
    double i00 = 0.0, i01 = 0.0, i11 = 0.0;
    if (det > CT_DIAG_TOL * d00 * d11 && det < INFINITY) { i00 = d11 / det; i01 = -d01 / det; i11 = d00 / det; }
    else { r0 = 0.0; r1 = 0.0; }                             /* left out of the system: g = 0 */
    dinv[3 * (size_t)i] = i00; dinv[3 * (size_t)i + 1] = i01; dinv[3 * (size_t)i + 2] = i11;
    const double z0 = i00 * r0 + i01 * r1, z1 = i01 * r0 + i11 * r1;
    x[2 * (size_t)i] = 0.0; x[2 * (size_t)i + 1] = 0.0;
    r[2 * (size_t)i] = r0; r[2 * (size_t)i + 1] = r1;
    z[2 * (size_t)i] = z0; z[2 * (size_t)i + 1] = z1;
    p[2 * (size_t)i] = z0; p[2 * (size_t)i + 1] = z1;
    rz = r0 * z0 + r1 * z1; bb = r0 * r0 + r1 * r1;
  }
  const double a = ct_block_sum(rz, s), b = ct_block_sum(bb, s);
  if (threadIdx.x == 0) { part_a[blockIdx.x] = a; part_b[blockIdx.x] = b; }
}

/* q = A p, one thread per vertex; partial sums of p . q.  A row that was left out of the system has p = 0 and keeps q = 0. */
__global__ void __launch_bounds__(256)
cubic_spmv(int n, const int *__restrict__ off, const int *__restrict__ adj, size_t n_adj, const double *__restrict__ pts,
           const double *__restrict__ dinv, const double *__restrict__ p, double *__restrict__ q, double *__restrict__ part_a,
           const CtScal *__restrict__ scal)
{
  __shared__ double s[256];
  if (scal->done) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  double pq = 0.0;
  if (i < n) {
    double q0 = 0.0, q1 = 0.0;
    const bool used = dinv[3 * (size_t)i] != 0.0 || dinv[3 * (size_t)i + 2] != 0.0;
    if (used) {
      const double xi = pts[2 * (size_t)i], yi = pts[2 * (size_t)i + 1];
      const double p0 = p[2 * (size_t)i], p1 = p[2 * (size_t)i + 1];
      size_t e0, e1;
      ct_row(off, n_adj, i, e0, e1);
      for (size_t e = e0; e < e1; e++) {
        const int j = adj[e];
        if (j < 0 || j >= n || j == i) continue;
        const double ex = pts[2 * (size_t)j] - xi, ey = pts[2 * (size_t)j + 1] - yi;
        const double l2 = ex * ex + ey * ey;
        if (!(l2 > 0.0)) continue;
        const double l3 = l2 * sqrt(l2);
        const double w = (4.0 * (ex * p0 + ey * p1) + 2.0 * (ex * p[2 * (size_t)j] + ey * p[2 * (size_t)j + 1])) / l3;
        q0 += w * ex; q1 += w * ey;
      }
      pq = p0 * q0 + p1 * q1;
    }
    q[2 * (size_t)i] = q0; q[2 * (size_t)i + 1] = q1;
  }
  const double a = ct_block_sum(pq, s);
  if (threadIdx.x == 0) part_a[blockIdx.x] = a;
}

/* second stage of the dot products, one workgroup: thread t adds partial sums t, t + 256, ... in that order, then the
   tree.  mode 0: after the set-up (r . z, b . b); 1: after the product (p . q); 2: after the update of iteration `it`
   (the new r . z, r . r): counts the iteration and gives the stopping verdict. */
__global__ void __launch_bounds__(256)
cubic_reduce_kernel(int mode, int n_part, const double *__restrict__ part_a, const double *__restrict__ part_b, CtScal *scal,
                    double rtol2, int it)
{
  __shared__ double s[256];
  const int was_done = mode == 0 ? 0 : scal->done;
  __syncthreads();
  if (was_done) return;
  double a = 0.0, b = 0.0;
  for (int k = threadIdx.x; k < n_part; k += 256) {
    a += part_a[k];
    if (mode != 1) b += part_b[k];
  }
  a = ct_block_sum(a, s);
  b = ct_block_sum(b, s);
  if (threadIdx.x != 0) return;
  if (mode == 0) {
    scal->rz[0] = a; scal->rz[1] = 0.0; scal->pq = 0.0; scal->rr = b; scal->bb = b; scal->iters = 0;
    scal->done = b > 0.0 ? 0 : 1;                            /* b = 0: g = 0 solves it */
  } else if (mode == 1) {
    scal->pq = a;
    if (!(a > 0.0)) scal->done = 2;
  } else {
    scal->rz[(it + 1) & 1] = a; scal->rr = b; scal->iters = it + 1;
    if (b <= rtol2 * scal->bb) scal->done = 1;
    else if (!(a > 0.0)) scal->done = 2;
  }
}

/* x += alpha p, r -= alpha q, z = D^-1 r; partial sums of r . z and r . r */
__global__ void __launch_bounds__(256)
cubic_update_kernel(int n, const double *__restrict__ dinv, const double *__restrict__ p, const double *__restrict__ q,
                    double *__restrict__ x, double *__restrict__ r, double *__restrict__ z, double *__restrict__ part_a,
                    double *__restrict__ part_b, const CtScal *__restrict__ scal, int it)
{
  __shared__ double s[256];
  if (scal->done) return;
  const double alpha = scal->rz[it & 1] / scal->pq;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  double rz = 0.0, rr = 0.0;
  if (i < n) {
    const size_t k = 2 * (size_t)i;
    x[k] += alpha * p[k]; x[k + 1] += alpha * p[k + 1];
    const double r0 = r[k] - alpha * q[k], r1 = r[k + 1] - alpha * q[k + 1];
    const double i00 = dinv[3 * (size_t)i], i01 = dinv[3 * (size_t)i + 1], i11 = dinv[3 * (size_t)i + 2];
    const double z0 = i00 * r0 + i01 * r1, z1 = i01 * r0 + i11 * r1;
    r[k] = r0; r[k + 1] = r1; z[k] = z0; z[k + 1] = z1;
    rz = r0 * z0 + r1 * z1; rr = r0 * r0 + r1 * r1;
  }
  const double a = ct_block_sum(rz, s), b = ct_block_sum(rr, s);
  if (threadIdx.x == 0) { part_a[blockIdx.x] = a; part_b[blockIdx.x] = b; }
}

/* p = z + beta p */
__global__ void __launch_bounds__(256)
cubic_direction_kernel(int n, const double *__restrict__ z, double *__restrict__ p, const CtScal *__restrict__ scal, int it)
{
  if (scal->done) return;
  const double beta = scal->rz[(it + 1) & 1] / scal->rz[it & 1];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t k = 2 * (size_t)i;
  p[k] = z[k] + beta * p[k]; p[k + 1] = z[k + 1] + beta * p[k + 1];
}

extern "C" int gsl_sinterp_hip_mesh_cubic_gradients(gsl_sinterp_hip_ctx *ctx, int n_points, const int *d_offsets, const int *d_adjacent,
                                                    size_t n_adjacent, const double *d_points, const double *d_f, double rtol, int maxiter,
                                                    double *d_g, int *h_iterations, double *h_residual)
{
  REQUIRE(ctx, ctx != NULL, ST_EFAULT);
  HIP_OK(ctx, hipSetDevice(ctx->device));
  REQUIRE(ctx, d_offsets && d_points && d_f && d_g && (n_adjacent == 0 || d_adjacent), ST_EFAULT);
  REQUIRE(ctx, n_points >= 1 && n_adjacent <= 0x7fffffffULL, ST_EINVAL);
  REQUIRE(ctx, rtol > 0.0 && rtol < 1.0 && maxiter >= 1, ST_EINVAL);
  if (h_iterations) *h_iterations = 0;
  if (h_residual) *h_residual = 0.0;
  const size_t n = (size_t)n_points;
  const int nb = (int)((n + 255) / 256);
  /* [CtScal | 256 B] [dinv 3n] [r z p q: 2n each] [two rows of partial sums] */
  const size_t head = 256, bytes = head + (3 * n + 8 * n + 2 * (size_t)nb) * sizeof(double);
  void *buf = NULL;
  int st = sinterp_workspace(ctx, bytes, &buf);
  if (st) return st;
  CtScal *scal = (CtScal *)buf;
  double *dinv = (double *)((char *)buf + head), *r = dinv + 3 * n, *z = r + 2 * n, *p = z + 2 * n, *q = p + 2 * n;
  double *part_a = q + 2 * n, *part_b = part_a + nb;
  const double rtol2 = rtol * rtol;
  hipLaunchKernelGGL(cubic_setup_kernel, dim3(nb), dim3(256), 0, ctx->stream, n_points, d_offsets, d_adjacent, n_adjacent, d_points, d_f,
                     dinv, d_g, r, z, p, part_a, part_b);
  hipLaunchKernelGGL(cubic_reduce_kernel, dim3(1), dim3(256), 0, ctx->stream, 0, nb, part_a, part_b, scal, rtol2, 0);
  LAUNCH_CHECK(ctx);
  CtScal h;
  memset(&h, 0, sizeof h);
  for (int it = 0; it < maxiter; it++) {
    hipLaunchKernelGGL(cubic_spmv, dim3(nb), dim3(256), 0, ctx->stream, n_points, d_offsets, d_adjacent, n_adjacent, d_points, dinv, p, q,
                       part_a, scal);
    hipLaunchKernelGGL(cubic_reduce_kernel, dim3(1), dim3(256), 0, ctx->stream, 1, nb, part_a, part_b, scal, rtol2, it);
    hipLaunchKernelGGL(cubic_update_kernel, dim3(nb), dim3(256), 0, ctx->stream, n_points, dinv, p, q, d_g, r, z, part_a, part_b, scal, it);
    hipLaunchKernelGGL(cubic_reduce_kernel, dim3(1), dim3(256), 0, ctx->stream, 2, nb, part_a, part_b, scal, rtol2, it);
    hipLaunchKernelGGL(cubic_direction_kernel, dim3(nb), dim3(256), 0, ctx->stream, n_points, z, p, scal, it);
    LAUNCH_CHECK(ctx);
    if ((it + 1) % CT_CHECK_EVERY == 0 || it + 1 == maxiter) {
      HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
      HIP_OK(ctx, hipMemcpy(&h, scal, sizeof h, hipMemcpyDeviceToHost));
      if (h.done) break;
    }
  }
  if (h_iterations) *h_iterations = h.iters;
  if (h_residual) *h_residual = h.bb > 0.0 ? sqrt(h.rr / h.bb) : 0.0;
  if (h.done == 1) return ST_SUCCESS;
  if (h.done == 2) return sinterp_fail(ctx, ST_EFAILED, "cubic gradients: conjugate gradients broke down (p . A p <= 0)", hipSuccess, __FILE__, __LINE__);
  return sinterp_fail(ctx, ST_EMAXITER, "cubic gradients: maxiter reached before the relative residual met rtol", hipSuccess, __FILE__, __LINE__);
}

/* ---- records ----------------------------------------------------------------------------------------------------- */

__global__ void __launch_bounds__(256)
cubic_pack_kernel(int n_tri, const int *__restrict__ tri, const int *__restrict__ nbr, int n_points, const double *__restrict__ pts,
                  const double *__restrict__ f, const double *__restrict__ g, CtRec *__restrict__ rec)
{
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_tri) return;
  const int i1 = tri[3 * (size_t)t], i2 = tri[3 * (size_t)t + 1], i3 = tri[3 * (size_t)t + 2];
  const bool bad = i1 < 0 || i1 >= n_points || i2 < 0 || i2 >= n_points || i3 < 0 || i3 >= n_points;
  const size_t a1 = bad ? 0 : (size_t)i1, a2 = bad ? 0 : (size_t)i2, a3 = bad ? 0 : (size_t)i3;
  const double x1 = pts[2 * a1], y1 = pts[2 * a1 + 1], x2 = pts[2 * a2], y2 = pts[2 * a2 + 1], x3 = pts[2 * a3], y3 = pts[2 * a3 + 1];
  const double f1 = f[a1], f2 = f[a2], f3 = f[a3];
  const double e12x = x2 - x1, e12y = y2 - y1, e23x = x3 - x2, e23y = y3 - y2, e31x = x1 - x3, e31y = y1 - y3;
  /* T = [v1 - v3, v2 - v3] as columns; b_1, b_2 = T^-1 (y - v3) */
  const double ta = e31x, tb = -e23x, tc = e31y, td = -e23y;
  const double det = ta * td - tb * tc;
  const double len2 = (e12x * e12x + e12y * e12y) + (e23x * e23x + e23y * e23y) + (e31x * e31x + e31y * e31y);
  const bool flat = bad || !(fabs(det) > CT_FLAT_TOL * len2);
  double c[CT_NORD];
#pragma unroll
  for (int k = 0; k < CT_NORD; k++) c[k] = 0.0;
  const double m0 = td / det, m1 = -tb / det, m2 = -tc / det, m3 = ta / det;
  if (flat) {
    double gx = (f1 - f3) * m0 + (f2 - f3) * m2, gy = (f1 - f3) * m1 + (f2 - f3) * m3;
    if (bad || !(fabs(gx) < INFINITY && fabs(gy) < INFINITY)) { gx = ct_nan(); gy = ct_nan(); }
    c[0] = gx; c[1] = gy;
  } else {
    const double g1x = g[2 * a1], g1y = g[2 * a1 + 1], g2x = g[2 * a2], g2y = g[2 * a2 + 1], g3x = g[2 * a3], g3y = g[2 * a3 + 1];
    const double df12 = g1x * e12x + g1y * e12y, df21 = -(g2x * e12x + g2y * e12y);
    const double df23 = g2x * e23x + g2y * e23y, df32 = -(g3x * e23x + g3y * e23y);
    const double df31 = g3x * e31x + g3y * e31y, df13 = -(g1x * e31x + g1y * e31y);
    const double c3000 = f1, c2100 = (df12 + 3.0 * f1) / 3.0, c2010 = (df13 + 3.0 * f1) / 3.0;
    const double c0300 = f2, c1200 = (df21 + 3.0 * f2) / 3.0, c0210 = (df23 + 3.0 * f2) / 3.0;
    const double c0030 = f3, c1020 = (df31 + 3.0 * f3) / 3.0, c0120 = (df32 + 3.0 * f3) / 3.0;
    const double c2001 = (c2100 + c2010 + c3000) / 3.0, c0201 = (c1200 + c0300 + c0210) / 3.0, c0021 = (c1020 + c0120 + c0030) / 3.0;
    /* edge factors: barycentric coordinates, in this triangle, of the centroid of the neighbour across edge k */
    double gam[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      gam[k] = -0.5;
      const int nb = nbr[3 * (size_t)t + k];
      if (nb < 0 || nb >= n_tri || nb == t) continue;
      const int j1 = tri[3 * (size_t)nb], j2 = tri[3 * (size_t)nb + 1], j3 = tri[3 * (size_t)nb + 2];
      if (j1 < 0 || j1 >= n_points || j2 < 0 || j2 >= n_points || j3 < 0 || j3 >= n_points) continue;
      const double cx = (pts[2 * (size_t)j1] + pts[2 * (size_t)j2] + pts[2 * (size_t)j3]) / 3.0 - x3;
      const double cy = (pts[2 * (size_t)j1 + 1] + pts[2 * (size_t)j2 + 1] + pts[2 * (size_t)j3 + 1]) / 3.0 - y3;
      double b[3];
      b[0] = m0 * cx + m1 * cy; b[1] = m2 * cx + m3 * cy; b[2] = 1.0 - b[0] - b[1];
      const double u = b[(k + 2) % 3], v = b[(k + 1) % 3];        /* k = 0: (c2, c1); 1: (c0, c2); 2: (c1, c0) */
      const double den = 2.0 - 3.0 * u - 3.0 * v;                 /* = 3 c_k - 1 < 0 for a neighbour across that edge */
      if (den < 0.0) gam[k] = (2.0 * u + v - 1.0) / den;
    }
    c[C3000] = c3000; c[C0300] = c0300; c[C0030] = c0030;
    c[C2100] = c2100; c[C2010] = c2010; c[C1200] = c1200; c[C0210] = c0210; c[C1020] = c1020; c[C0120] = c0120;
    c[C0111] = (gam[0] * (-c0300 + 3.0 * c0210 - 3.0 * c0120 + c0030) + (-c0300 + 2.0 * c0210 - c0120 + c0021 + c0201)) / 2.0;
    c[C1011] = (gam[1] * (-c0030 + 3.0 * c1020 - 3.0 * c2010 + c3000) + (-c0030 + 2.0 * c1020 - c2010 + c2001 + c0021)) / 2.0;
    c[C1101] = (gam[2] * (-c3000 + 3.0 * c2100 - 3.0 * c1200 + c0300) + (-c3000 + 2.0 * c2100 - c1200 + c2001 + c0201)) / 2.0;
  }
  double2 *o = reinterpret_cast<double2 *>(rec + t);
  o[0] = make_double2(x3, y3);
  o[1] = make_double2(m0, m1);
  o[2] = make_double2(m2, m3);
#pragma unroll
  for (int k = 0; k < CT_NORD / 2; k++) o[3 + k] = make_double2(c[2 * k], c[2 * k + 1]);
  *reinterpret_cast<int4 *>(o + 9) = make_int4(flat ? 1 : 0, 0, 0, 0);
}

/* ---- sweep --------------------------------------------------------------------------------------------------------- */

/* One target per lane.  located[k] = the triangle the linear path found (-1: outside / NaN target), lin[k] = its
   piecewise-linear value, used for a flat triangle only; lin and values may be the same array (each lane reads its own
   entry before it writes it).  grad (GRAD only): row k at grad + k * gtda. */
template <bool GRAD>
__global__ void __launch_bounds__(256)
cubic_sweep_kernel(int n_tri, const CtRec *__restrict__ rec, const int *__restrict__ located, const double *lin,
                   const double *__restrict__ targets, size_t m, size_t ttda, double *values, double *__restrict__ grad, size_t gtda)
{
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= m) return;
  const int t = located[k];
  if (t < 0 || t >= n_tri) {
    values[k] = ct_nan();
    if (GRAD) { grad[k * gtda] = ct_nan(); grad[k * gtda + 1] = ct_nan(); }
    return;
  }
  const double2 *p = reinterpret_cast<const double2 *>(rec + t);
  const double2 o = p[0], ma = p[1], mb = p[2];
  const double2 ca = p[3], cb = p[4], cc = p[5], cd = p[6], ce = p[7], cf = p[8];
  const int meta = reinterpret_cast<const int4 *>(p + 9)->x;
  if (meta & 1) {
    values[k] = lin[k];
    if (GRAD) { grad[k * gtda] = ca.x; grad[k * gtda + 1] = ca.y; }
    return;
  }
  const double dx = targets[k * ttda] - o.x, dy = targets[k * ttda + 1] - o.y;
  const double b1 = ma.x * dx + ma.y * dy, b2 = mb.x * dx + mb.y * dy, b3 = 1.0 - b1 - b2;
  const int j = (b1 <= b2 && b1 <= b3) ? 1 : (b2 <= b3 ? 2 : 3);
  const double mn = j == 1 ? b1 : (j == 2 ? b2 : b3);
  const double a1 = b1 - mn, a2 = b2 - mn, a3 = b3 - mn, a4 = 3.0 * mn;
  const double c3000 = ca.x, c0300 = ca.y, c0030 = cb.x, c2100 = cb.y, c2010 = cc.x, c1200 = cc.y;
  const double c0210 = cd.x, c1020 = cd.y, c0120 = ce.x, c0111 = ce.y, c1011 = cf.x, c1101 = cf.y;
  const double c2001 = (c2100 + c2010 + c3000) / 3.0, c0201 = (c1200 + c0300 + c0210) / 3.0, c0021 = (c1020 + c0120 + c0030) / 3.0;
  const double c1002 = (c1101 + c1011 + c2001) / 3.0, c0102 = (c1101 + c0111 + c0201) / 3.0, c0012 = (c1011 + c0111 + c0021) / 3.0;
  const double c0003 = (c1002 + c0102 + c0012) / 3.0;
  /* Q_i = (dP/da_i) / 3; the a_1 a_2 a_3 products are left out (one of the three is 0, and the form whose index is j is
     used in the value only, with the factor a_j = 0) */
  const double a11 = a1 * a1, a22 = a2 * a2, a33 = a3 * a3, a44 = a4 * a4;
  const double a12 = 2.0 * a1 * a2, a13 = 2.0 * a1 * a3, a14 = 2.0 * a1 * a4, a23 = 2.0 * a2 * a3, a24 = 2.0 * a2 * a4, a34 = 2.0 * a3 * a4;
  const double q1 = a11 * c3000 + a12 * c2100 + a13 * c2010 + a14 * c2001 + a22 * c1200 + a24 * c1101 + a33 * c1020 + a34 * c1011 + a44 * c1002;
  const double q2 = a11 * c2100 + a12 * c1200 + a14 * c1101 + a22 * c0300 + a23 * c0210 + a24 * c0201 + a33 * c0120 + a34 * c0111 + a44 * c0102;
  const double q3 = a11 * c2010 + a13 * c1020 + a14 * c1011 + a22 * c0210 + a23 * c0120 + a24 * c0111 + a33 * c0030 + a34 * c0021 + a44 * c0012;
  const double q4 = a11 * c2001 + a12 * c1101 + a13 * c1011 + a14 * c1002 + a22 * c0201 + a23 * c0111 + a24 * c0102 + a33 * c0021 + a34 * c0012 +
                    a44 * c0003;
  values[k] = a1 * q1 + a2 * q2 + a3 * q3 + a4 * q4;
  if (GRAD) {
    /* ds/db_i = 3 Q_i away from j; b_j enters through every a_i = b_i - b_j and through a_4 = 3 b_j */
    const double h1 = j == 1 ? 3.0 * q4 - (q2 + q3) : q1;
    const double h2 = j == 2 ? 3.0 * q4 - (q1 + q3) : q2;
    const double h3 = j == 3 ? 3.0 * q4 - (q1 + q2) : q3;
    const double u = 3.0 * (h1 - h3), v = 3.0 * (h2 - h3);      /* b_3 = 1 - b_1 - b_2 */
    grad[k * gtda] = u * ma.x + v * mb.x;
    grad[k * gtda + 1] = u * ma.y + v * mb.y;
  }
}

extern "C" int gsl_sinterp_hip_mesh_cubic_pack(gsl_sinterp_hip_ctx *ctx, int n_tri, const int *d_tri, const int *d_nbr, int n_points,
                                               const double *d_points, const double *d_f, const double *d_g, void *d_ctrec)
{
  REQUIRE(ctx, ctx != NULL, ST_EFAULT);
  HIP_OK(ctx, hipSetDevice(ctx->device));
  REQUIRE(ctx, n_tri > 0 && n_points >= 3, ST_EINVAL);
  REQUIRE(ctx, d_tri && d_nbr && d_points && d_f && d_g && d_ctrec, ST_EFAULT);
  REQUIRE(ctx, ((uintptr_t)d_ctrec & 15) == 0, ST_EINVAL);
  hipLaunchKernelGGL(cubic_pack_kernel, dim3((n_tri + 255) / 256), dim3(256), 0, ctx->stream, n_tri, d_tri, d_nbr, n_points, d_points, d_f,
                     d_g, (CtRec *)d_ctrec);
  LAUNCH_CHECK(ctx);
  return ST_SUCCESS;
}

extern "C" int gsl_sinterp_hip_mesh_cubic_eval(gsl_sinterp_hip_ctx *ctx, int n_tri, const void *d_ctrec, const int *d_located,
                                               const double *d_linear_values, const double *d_targets, size_t m, size_t ttda,
                                               double *d_values, double *d_grad, size_t gtda)
{
  REQUIRE(ctx, ctx != NULL, ST_EFAULT);
  HIP_OK(ctx, hipSetDevice(ctx->device));
  REQUIRE(ctx, n_tri > 0 && ttda >= 2 && (d_grad == NULL || gtda >= 2), ST_EINVAL);
  REQUIRE(ctx, d_ctrec && (m == 0 || (d_located && d_linear_values && d_targets && d_values)), ST_EFAULT);
  REQUIRE(ctx, ((uintptr_t)d_ctrec & 15) == 0, ST_EINVAL);
  if (m == 0) return ST_SUCCESS;
  REQUIRE(ctx, (m + 255) / 256 < 0x7fffffffULL, ST_EINVAL);
  const dim3 grid((unsigned)((m + 255) / 256));
  if (d_grad)
    hipLaunchKernelGGL(cubic_sweep_kernel<true>, grid, dim3(256), 0, ctx->stream, n_tri, (const CtRec *)d_ctrec, d_located, d_linear_values,
                       d_targets, m, ttda, d_values, d_grad, gtda);
  else
    hipLaunchKernelGGL(cubic_sweep_kernel<false>, grid, dim3(256), 0, ctx->stream, n_tri, (const CtRec *)d_ctrec, d_located, d_linear_values,
                       d_targets, m, ttda, d_values, (double *)NULL, (size_t)0);
  LAUNCH_CHECK(ctx);
  return ST_SUCCESS;
}
