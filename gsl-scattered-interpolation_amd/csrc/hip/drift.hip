/*
 * drift.hip -- the polynomial drift of universal kriging ("Universal kriging"):
 *
 *     s(y) = p(u(y))^T c + sum_j w_j phi(|y - x_j|),     [K P; P^T 0] [w; c] = [f; 0],     K = Phi + nugget I.
 *
 * The basis lives in STANDARDISED coordinates u_a = (y_a - shift_a) scale_a (shift = the centre of the sites' bounding
 * box, scale = 1 / half-extent per axis): monomials in raw coordinates of UTM size would cost every digit of S = P^T K^-1 P.
 * Term order: 1; u_1 .. u_d; u_a u_b for a <= b, lexicographic.  q = C(d + order, order) <= 10.
 *
 * Here: the basis fill (P, one column per term), the tail add after a plain sweep (values and gradients, several
 * fields), the fixed-order reductions behind S = P^T B and T = P^T A, the combine of the variance
 *
 *     sigma^2(y) = phi(0) - |L^-1 k|^2 + r^T S^-1 r,     r = p(u(y)) - B^T k(y),     B = K^-1 P,
 *
 * and the combine of Dubrule's leave-one-out rule with a drift, diag_i = (K^-1)_ii - B_i S^-1 B_i^T.  S^-1 is always
 * applied through the host Cholesky factor S = Ls Ls^T (gsl_sinterp_hip_drift_factor): x^T S^-1 x = |Ls^-1 x|^2.
 * Everything small (geometry, coefficients, Ls) reaches the kernels BY VALUE: no device state, any context may call.
 */
#include "common.h"
#include <float.h>
#include <math.h>
#include "rbf_phi.h"   /* with_dim, ic */

#define DRIFT_MAXQ GSL_SINTERP_DRIFT_MAX_TERMS
#define DRIFT_FB 8     /* fields per launch of the tail add: their coefficients travel by value */

constexpr int drift_q(int dim, int order) { return order == 0 ? 1 : order == 1 ? dim + 1 : (dim + 1) * (dim + 2) / 2; }

struct DriftGeom { double shift[3], scale[3]; };
struct DriftCoef { double c[DRIFT_FB][DRIFT_MAXQ]; };
struct DriftTri { double l[DRIFT_MAXQ * (DRIFT_MAXQ + 1) / 2]; };       /* Ls, row-major packed lower triangle */

template <int DIM>
__device__ __forceinline__ void drift_u(const DriftGeom &g, const double *__restrict__ y, double (&u)[DIM])
{
#pragma unroll
  for (int a = 0; a < DIM; a++) u[a] = (y[a] - g.shift[a]) * g.scale[a];
}

/* p(u), the one definition of the term order */
template <int DIM, int ORDER>
__device__ __forceinline__ void drift_terms(const double (&u)[DIM], double (&p)[drift_q(DIM, ORDER)])
{
  p[0] = 1.0;
#pragma unroll
  for (int a = 0; a < DIM; a++) p[1 + a] = u[a];
  if constexpr (ORDER == 2) {
    int t = 1 + DIM;
#pragma unroll
    for (int a = 0; a < DIM; a++)
#pragma unroll
      for (int b = a; b < DIM; b++) p[t++] = u[a] * u[b];
  }
}

/* p(u)^T c in the one order every caller shares: the value bits of a target do not depend on the entry it came through */
template <int DIM, int ORDER>
__device__ __forceinline__ double drift_value(const double (&u)[DIM], const double *c)
{
  double p[drift_q(DIM, ORDER)];
  drift_terms<DIM, ORDER>(u, p);
  double acc = c[0];
#pragma unroll
  for (int t = 1; t < drift_q(DIM, ORDER); t++) acc = fma(c[t], p[t], acc);
  return acc;
}

/* d(p^T c)/dy_a in raw coordinates: the chain rule through scale */
template <int DIM, int ORDER>
__device__ __forceinline__ void drift_gradient(const DriftGeom &g, const double (&u)[DIM], const double *c, double (&d)[DIM])
{
#pragma unroll
  for (int a = 0; a < DIM; a++) d[a] = c[1 + a];
  if constexpr (ORDER == 2) {
    int t = 1 + DIM;
#pragma unroll
    for (int a = 0; a < DIM; a++)
#pragma unroll
      for (int b = a; b < DIM; b++) {
        if (a == b) {
          d[a] = fma(2.0 * c[t], u[a], d[a]);
        } else {
          d[a] = fma(c[t], u[b], d[a]);
          d[b] = fma(c[t], u[a], d[b]);
        }
        t++;
      }
  }
#pragma unroll
  for (int a = 0; a < DIM; a++) d[a] *= g.scale[a];
}

/* ------------------------------------------------------------------------ */
/* P: column t at P + t * ldp, one thread per site */
template <int DIM, int ORDER>
__global__ void __launch_bounds__(256)
drift_basis_kernel(DriftGeom g, const double *__restrict__ x, size_t n, size_t xtda, double *__restrict__ P, size_t ldp)
{
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double u[DIM], p[drift_q(DIM, ORDER)];
  drift_u<DIM>(g, x + i * xtda, u);
  drift_terms<DIM, ORDER>(u, p);
#pragma unroll
  for (int t = 0; t < drift_q(DIM, ORDER); t++) P[(size_t)t * ldp + i] = p[t];
}

/* the tail after a plain sweep: s[k * stda + f] += p(u_k)^T c_f and g[k * gtda + f * DIM + a] += d/dy_a, f < nf <= DRIFT_FB.
   One thread per target; either output may be NULL.  The value is s + tail, one rounding, as add_const_kernel adds the mean */
template <int DIM, int ORDER>
__global__ void __launch_bounds__(256)
drift_add_kernel(DriftGeom g, DriftCoef c, int nf, const double *__restrict__ y, size_t m, size_t ytda, double *__restrict__ s,
                 size_t stda, double *__restrict__ gr, size_t gtda)
{
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < m; k += stride) {
    double u[DIM];
    drift_u<DIM>(g, y + k * ytda, u);
    for (int f = 0; f < nf; f++) {
      if (s) s[k * stda + f] = s[k * stda + f] + drift_value<DIM, ORDER>(u, c.c[f]);
      if (gr) {
        double d[DIM];
        drift_gradient<DIM, ORDER>(g, u, c.c[f], d);
#pragma unroll
        for (int a = 0; a < DIM; a++) gr[k * gtda + (size_t)f * DIM + a] = gr[k * gtda + (size_t)f * DIM + a] + d[a];
      }
    }
  }
}

/* G[a * ncols + b] = sum_i P_a[i] Y_b[i]: one workgroup per entry, every partial sum in a fixed order (thread t takes
   i = t, t + 256, ..; a shuffle tree; the four wave sums in one expression): the same bits every run */
__global__ void __launch_bounds__(256)
drift_gram_kernel(const double *__restrict__ P, size_t ldp, const double *__restrict__ Y, size_t ldy, size_t n, int ncols,
                  double *__restrict__ G)
{
  __shared__ double s_red[4];
  const int a = blockIdx.x / ncols, b = blockIdx.x % ncols;
  double acc = 0;
  for (size_t i = threadIdx.x; i < n; i += 256) acc = fma(P[(size_t)a * ldp + i], Y[(size_t)b * ldy + i], acc);
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) G[blockIdx.x] = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

/* |Ls^-1 r|^2 by forward substitution, r overwritten */
template <int Q>
__device__ __forceinline__ double drift_quad(const DriftTri &L, double (&r)[Q])
{
  double acc = 0.0;
#pragma unroll
  for (int i = 0; i < Q; i++) {
    double v = r[i];
#pragma unroll
    for (int j = 0; j < i; j++) v = fma(-L.l[i * (i + 1) / 2 + j], r[j], v);
    v /= L.l[i * (i + 1) / 2 + i];
    r[i] = v;
    acc = fma(v, v, acc);
  }
  return acc;
}

/* var_k = (1 - q_k) + |Ls^-1 (p(u_k) - bk_k)|^2 with bk_k = B^T k(y_k) at bk + k * Q.  No clamping. */
template <int DIM, int ORDER>
__global__ void __launch_bounds__(256)
drift_var_combine_kernel(DriftGeom g, DriftTri L, const double *__restrict__ y, size_t rows, size_t ytda, const double *__restrict__ bk,
                         const double *__restrict__ qn, double *__restrict__ var)
{
  constexpr int Q = drift_q(DIM, ORDER);
  const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= rows) return;
  double u[DIM], r[Q];
  drift_u<DIM>(g, y + k * ytda, u);
  drift_terms<DIM, ORDER>(u, r);
#pragma unroll
  for (int t = 0; t < Q; t++) r[t] -= bk[k * Q + t];
  var[k] = (1.0 - qn[k]) + drift_quad<Q>(L, r);
}

/* the joint covariance's T (krige_cov.hip): row k of bk, B^T k(y_k) on entry, becomes t_k = Ls^-1 (p(u_k) - bk_k), the forward
   substitution of drift_quad with Ls in registers.  ORDER 0 is ordinary kriging: p = 1, Q = 1, Ls = sqrt(1^T b). */
template <int DIM, int ORDER>
__global__ void __launch_bounds__(256)
drift_cov_terms_kernel(DriftGeom g, DriftTri L, const double *__restrict__ y, size_t rows, size_t ytda, double *__restrict__ bk)
{
  constexpr int Q = drift_q(DIM, ORDER);
  const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= rows) return;
  double r[Q];
  if constexpr (ORDER == 0) {
    r[0] = 1.0;
  } else {
    double u[DIM];
    drift_u<DIM>(g, y + k * ytda, u);
    drift_terms<DIM, ORDER>(u, r);
  }
#pragma unroll
  for (int t = 0; t < Q; t++) r[t] -= bk[k * Q + t];
  (void)drift_quad<Q>(L, r);
#pragma unroll
  for (int t = 0; t < Q; t++) bk[k * Q + t] = r[t];
}

/* diag_i = g_i - |Ls^-1 B_i|^2; e[f][i] = w[f][i] / diag_i, v_i = 1 / diag_i (loo_combine_kernel with the drift's correction) */
template <int Q>
__global__ void __launch_bounds__(256)
drift_loo_combine_kernel(DriftTri L, size_t n, int nf, const double *__restrict__ gd, const double *__restrict__ B, size_t ldb,
                         const double *__restrict__ w, size_t ldw, double *__restrict__ e, size_t lde, double *__restrict__ v)
{
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double r[Q];
#pragma unroll
  for (int t = 0; t < Q; t++) r[t] = B[(size_t)t * ldb + i];
  const double d = gd[i] - drift_quad<Q>(L, r);
  v[i] = 1.0 / d;
  for (int f = 0; f < nf; f++) e[(size_t)f * lde + i] = w[(size_t)f * ldw + i] / d;
}

/* ------------------------------------------------------------------------ */
static DriftGeom make_geom(int dim, const double *h_shift, const double *h_scale)
{
  DriftGeom g;
  for (int a = 0; a < 3; a++) { g.shift[a] = a < dim ? h_shift[a] : 0.0; g.scale[a] = a < dim ? h_scale[a] : 1.0; }
  return g;
}

static DriftTri make_tri(int q, const double *h_L)
{
  DriftTri t;
  memset(&t, 0, sizeof t);
  for (int i = 0; i < q; i++)
    for (int j = 0; j <= i; j++) t.l[i * (i + 1) / 2 + j] = h_L[i * q + j];
  return t;
}

/* (dim, order in 1..2) -> kernel instance */
template <class F> static void with_dim_order(int dim, int order, F &&f)
{
  with_dim(dim, [&](auto D) {
    if (order == 1) f(D, ic<1>());
    else f(D, ic<2>());
  });
}

template <class F> static void with_q(int q, F &&f)
{
  switch (q) {
    case 2: f(ic<2>()); break;
    case 3: f(ic<3>()); break;
    case 4: f(ic<4>()); break;
    case 6: f(ic<6>()); break;
    default: f(ic<10>()); break;
  }
}

extern "C" size_t gsl_sinterp_hip_drift_terms(int dim, int order)
{
  return dim >= 1 && dim <= 3 && order >= 0 && order <= 2 ? (size_t)drift_q(dim, order) : 0;
}

/* S = Ls Ls^T on the host; a pivot not above 64 DBL_EPSILON times that diagonal entry of S before elimination, or not
   finite, means the drift functions are linearly dependent on the sites */
extern "C" int gsl_sinterp_hip_drift_factor(size_t q, const double *h_S, double *h_L)
{
  if (!h_S || !h_L) return ST_EFAULT;
  if (q < 1 || q > DRIFT_MAXQ) return ST_EINVAL;
  for (size_t i = 0; i < q * q; i++) h_L[i] = 0.0;
  for (size_t j = 0; j < q; j++) {
    double d = h_S[j * q + j];
    for (size_t k = 0; k < j; k++) d -= h_L[j * q + k] * h_L[j * q + k];
    if (!(d > 64.0 * DBL_EPSILON * h_S[j * q + j]) || !isfinite(d)) return ST_EDOM;
    const double l = sqrt(d);
    h_L[j * q + j] = l;
    for (size_t i = j + 1; i < q; i++) {
      double v = 0.5 * (h_S[i * q + j] + h_S[j * q + i]);               /* S is symmetric up to the rounding of two reductions */
      for (size_t k = 0; k < j; k++) v -= h_L[i * q + k] * h_L[j * q + k];
      h_L[i * q + j] = v / l;
    }
  }
  return ST_SUCCESS;
}

int sinterp_drift_basis(gsl_sinterp_hip_ctx *ctx, int order, const double *h_shift, const double *h_scale, const double *d_x, size_t n,
                        int dim, size_t xtda, double *d_P, size_t ldp)
{
  const DriftGeom g = make_geom(dim, h_shift, h_scale);
  const dim3 grid((unsigned)((n + 255) / 256));
  with_dim_order(dim, order, [&](auto D, auto O) {
    hipLaunchKernelGGL((drift_basis_kernel<decltype(D)::value, decltype(O)::value>), grid, dim3(256), 0, ctx->stream, g, d_x, n, xtda, d_P, ldp);
  });
  LAUNCH_CHECK(ctx);
  return ST_SUCCESS;
}

int sinterp_drift_gram(gsl_sinterp_hip_ctx *ctx, const double *d_P, size_t ldp, const double *d_Y, size_t ldy, size_t n, int q, int ncols,
                       double *d_G)
{
  hipLaunchKernelGGL(drift_gram_kernel, dim3((unsigned)(q * ncols)), dim3(256), 0, ctx->stream, d_P, ldp, d_Y, ldy, n, ncols, d_G);
  LAUNCH_CHECK(ctx);
  return ST_SUCCESS;
}

int sinterp_drift_var_combine(gsl_sinterp_hip_ctx *ctx, int order, const double *h_shift, const double *h_scale, const double *h_L, int dim,
                              const double *d_y, size_t rows, size_t ytda, const double *d_bk, const double *d_q, double *d_var)
{
  const DriftGeom g = make_geom(dim, h_shift, h_scale);
  const DriftTri L = make_tri(drift_q(dim, order), h_L);
  const dim3 grid((unsigned)((rows + 255) / 256));
  with_dim_order(dim, order, [&](auto D, auto O) {
    hipLaunchKernelGGL((drift_var_combine_kernel<decltype(D)::value, decltype(O)::value>), grid, dim3(256), 0, ctx->stream, g, L, d_y, rows,
                       ytda, d_bk, d_q, d_var);
  });
  LAUNCH_CHECK(ctx);
  return ST_SUCCESS;
}

int sinterp_drift_cov_terms(gsl_sinterp_hip_ctx *ctx, int order, const double *h_shift, const double *h_scale, const double *h_L, int dim,
                            const double *d_y, size_t rows, size_t ytda, double *d_bk)
{
  static const double zero[3] = {0.0, 0.0, 0.0}, one[3] = {1.0, 1.0, 1.0};
  const DriftGeom g = order == 0 ? make_geom(dim, zero, one) : make_geom(dim, h_shift, h_scale);
  const DriftTri L = make_tri(drift_q(dim, order), h_L);
  const dim3 grid((unsigned)((rows + 255) / 256));
  with_dim(dim, [&](auto D) {
    constexpr int d = decltype(D)::value;
    if (order == 0) hipLaunchKernelGGL((drift_cov_terms_kernel<d, 0>), grid, dim3(256), 0, ctx->stream, g, L, d_y, rows, ytda, d_bk);
    else if (order == 1) hipLaunchKernelGGL((drift_cov_terms_kernel<d, 1>), grid, dim3(256), 0, ctx->stream, g, L, d_y, rows, ytda, d_bk);
    else hipLaunchKernelGGL((drift_cov_terms_kernel<d, 2>), grid, dim3(256), 0, ctx->stream, g, L, d_y, rows, ytda, d_bk);
  });
  LAUNCH_CHECK(ctx);
  return ST_SUCCESS;
}

extern "C" int gsl_sinterp_hip_drift_basis(gsl_sinterp_hip_ctx *ctx, int order, const double *h_shift, const double *h_scale,
                                           const double *d_x, size_t n, int dim, size_t xtda, double *d_P, size_t ldp)
{
  REQUIRE(ctx, ctx != NULL, ST_EFAULT);
  HIP_OK(ctx, hipSetDevice(ctx->device));
  REQUIRE(ctx, dim >= 1 && dim <= 3 && (order == 1 || order == 2) && xtda >= (size_t)dim && ldp >= n, ST_EINVAL);
  REQUIRE(ctx, h_shift && h_scale && (n == 0 || (d_x && d_P)), ST_EFAULT);
  if (n == 0) return ST_SUCCESS;
  return sinterp_drift_basis(ctx, order, h_shift, h_scale, d_x, n, dim, xtda, d_P, ldp);
}

extern "C" int gsl_sinterp_hip_drift_add(gsl_sinterp_hip_ctx *ctx, int order, const double *h_shift, const double *h_scale,
                                         const double *h_coef, size_t nf, const double *d_y, size_t m, int dim, size_t ytda,
                                         double *d_s, size_t stda, double *d_g, size_t gtda)
{
  REQUIRE(ctx, ctx != NULL, ST_EFAULT);
  HIP_OK(ctx, hipSetDevice(ctx->device));
  REQUIRE(ctx, dim >= 1 && dim <= 3 && (order == 1 || order == 2) && ytda >= (size_t)dim, ST_EINVAL);
  REQUIRE(ctx, nf >= 1 && nf <= GSL_SINTERP_MAX_FIELDS && (!d_s || stda >= nf) && (!d_g || gtda >= nf * (size_t)dim), ST_EINVAL);
  REQUIRE(ctx, h_shift && h_scale && h_coef && (m == 0 || d_y), ST_EFAULT);
  if (m == 0 || (!d_s && !d_g)) return ST_SUCCESS;
  const DriftGeom g = make_geom(dim, h_shift, h_scale);
  const int q = drift_q(dim, order);
  size_t blocks = (m + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  for (size_t f0 = 0; f0 < nf; f0 += DRIFT_FB) {
    const int nb = (int)(nf - f0 < DRIFT_FB ? nf - f0 : DRIFT_FB);
    DriftCoef c;
    memset(&c, 0, sizeof c);
    for (int f = 0; f < nb; f++)
      for (int t = 0; t < q; t++) c.c[f][t] = h_coef[(f0 + f) * q + t];
    with_dim_order(dim, order, [&](auto D, auto O) {
      hipLaunchKernelGGL((drift_add_kernel<decltype(D)::value, decltype(O)::value>), dim3((unsigned)blocks), dim3(256), 0, ctx->stream, g, c, nb,
                         d_y, m, ytda, d_s ? d_s + f0 : NULL, stda, d_g ? d_g + f0 * dim : NULL, gtda);
    });
    LAUNCH_CHECK(ctx);
  }
  return ST_SUCCESS;
}

extern "C" int gsl_sinterp_hip_loo_combine_drift(gsl_sinterp_hip_ctx *ctx, size_t n, size_t nf, const double *d_g, const double *d_B,
                                                 size_t ldb, size_t q, const double *h_L, const double *d_w, size_t ldw, double *d_e,
                                                 size_t lde, double *d_v)
{
  REQUIRE(ctx, ctx != NULL, ST_EFAULT);
  HIP_OK(ctx, hipSetDevice(ctx->device));
  REQUIRE(ctx, nf <= GSL_SINTERP_MAX_FIELDS && (nf == 0 || (ldw >= n && lde >= n)) && ldb >= n, ST_EINVAL);
  REQUIRE(ctx, q == 2 || q == 3 || q == 4 || q == 6 || q == 10, ST_EINVAL);
  REQUIRE(ctx, h_L && (n == 0 || (d_g && d_B && d_v && (nf == 0 || (d_w && d_e)))), ST_EFAULT);
  if (n == 0) return ST_SUCCESS;
  const DriftTri L = make_tri((int)q, h_L);
  with_q((int)q, [&](auto Q) {
    hipLaunchKernelGGL((drift_loo_combine_kernel<decltype(Q)::value>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, L, n, (int)nf,
                       d_g, d_B, ldb, d_w, ldw, d_e, lde, d_v);
  });
  LAUNCH_CHECK(ctx);
  return ST_SUCCESS;
}
