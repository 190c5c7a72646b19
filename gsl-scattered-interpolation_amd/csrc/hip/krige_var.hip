/*
 * krige_var.hip -- the kriging variance at M targets from the Cholesky factor K = Phi + nugget I = L L^T that the
 * kriging solve (solve.hip, route 7) leaves behind:
 *
 *     sigma^2(y) = C(0) - |L^-1 k(y)|^2 + (1 - b^T k(y))^2 / d,     k(y)_j = C(|y - x_j|),  b = K^-1 1,  d = 1^T b,
 *
 * the variance of the underlying field (the nugget is measurement noise), sill C(0) = 1.  The targets are processed in
 * chunks of rows of a work matrix Z (row = target, column = centre, pitch ldw = N rounded up to 128):
 *
 *     fill      Z[k][j] = phi(|y_k - x_j|)                                     (rbf_phi.h: the arithmetic of the fill)
 *     solve     Z <- Z L^-T, blocked forward substitution from the right over 128-column blocks J:
 *                 Z[:, J] -= Z[:, :J] L[J, :J]^T                               (gemm.hip, fp64 MFMA, stream-K)
 *                 Z[:, J] <- Z[:, J] L_JJ^-T,  q_k += sum_j Z[k][J j]^2         (krige_trsm128_kernel, below)
 *     combine   var_k = 1 - q_k + (1 - a_k)^2 / d,    a = b^T k from the culled sweep (rbf.hip) with b as weights.
 *
 * M N^2 flops, all of them in the GEMM; the N^2 doubles of the factor stay resident for as long as variances are wanted.
 * The inverted 32 x 32 diagonal blocks of L that the diagonal step multiplies with are formed once per model
 * (gsl_sinterp_hip_krige_variance_prepare).  Only the lower triangle of the factor, diagonal included, is read: the
 * strict upper triangle holds whatever the factorisation kept there.
 */
#include "common.h"
#include <math.h>
#include <stdlib.h>
#include "trsm128.h"
#include "rbf_phi.h"

#define KV_RP 128   /* rows of a pass are padded to this (zero rows): every update then takes the full-tile GEMM path */

/* ------------------------------------------------------------------------ */
/* cross-covariance fill: block = 256 threads -> 16 rows (targets) x 128 columns (centres), 2 columns (16 B) per lane.
   Rows >= rows (padding of the pass) and columns >= n (padding of the last block) are written as zeros, so they pass
   through the substitution as zeros and add nothing to q.  The column-0 blocks also clear q for the pass. */
template <int KIND, int DIM>
__global__ void __launch_bounds__(256)
krige_cross_fill_kernel(double coef, const double *__restrict__ tbl, const double *__restrict__ x, size_t n, size_t xtda,
                        const double *__restrict__ y, size_t rows, size_t ytda, double *__restrict__ Z, size_t ldw,
                        double *__restrict__ q)
{
  __shared__ double s_t0[kind_uses_exp2(KIND) ? TBL_N : 1];
  if (kind_uses_exp2(KIND)) s_t0[threadIdx.x] = tbl[threadIdx.x];      /* TBL_N = 256 = the block */
  __syncthreads();
  const size_t j0 = ((size_t)blockIdx.x * 64 + (threadIdx.x & 63)) * 2;
  const size_t ibase = (size_t)blockIdx.y * 16 + (threadIdx.x >> 6) * 4;
  if (blockIdx.x == 0 && (threadIdx.x & 63) < 4) q[ibase + (threadIdx.x & 63)] = 0.0;
  const bool ca = j0 < n, cb = j0 + 1 < n;
  double xa[DIM], xb[DIM];
#pragma unroll
  for (int c = 0; c < DIM; c++) { xa[c] = ca ? x[j0 * xtda + c] : 0.0; xb[c] = cb ? x[(j0 + 1) * xtda + c] : 0.0; }
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const size_t i = ibase + r;
    double va = 0.0, vb = 0.0;
    if (i < rows && ca) {
      double ra = 0.0, rb = 0.0;
#pragma unroll
      for (int c = 0; c < DIM; c++) {
        const double yi = y[i * ytda + c];
        const double da = yi - xa[c], db = yi - xb[c];
        ra = fma(da, da, ra); rb = fma(db, db, rb);
      }
      va = phi_r2<KIND, 1>(ra, coef, s_t0, s_t0);
      vb = cb ? phi_r2<KIND, 1>(rb, coef, s_t0, s_t0) : 0.0;
    }
    *reinterpret_cast<double2 *>(Z + i * ldw + j0) = make_double2(va, vb);       /* Z 16-byte aligned, ldw and j0 even */
  }
}

/* ------------------------------------------------------------------------ */
/* inverse of every 32 x 32 diagonal block of L (identity padding past n): lane c solves L_bb x = e_c by forward
   substitution with x in registers, Dinv[b][i][c] = (L_bb^-1)[i][c] -- the layout chol_diag128_block writes and the
   row solves read as MFMA B fragments */
__global__ void __launch_bounds__(64)
krige_inv32_kernel(const double *__restrict__ L, size_t lda, size_t n, double *__restrict__ Dinv)
{
  __shared__ double sL[CB][CB + 1];
  const size_t j0 = (size_t)blockIdx.x * CB;
  const int nb = (int)((n - j0) < CB ? (n - j0) : CB);
  const int lane = threadIdx.x;
  for (int e = lane; e < CB * CB; e += 64) {
    const int r = e / CB, c = e % CB;
    double v = r == c ? 1.0 : 0.0;
    if (r < nb && c <= r) v = L[(j0 + r) * lda + j0 + c];                         /* lower triangle only */
    sL[r][c] = v;
  }
  __syncthreads();
  if (lane >= CB) return;
  double xv[CB];
#pragma unroll
  for (int i = 0; i < CB; i++) {
    double v = (i == lane) ? 1.0 : 0.0;
#pragma unroll
    for (int k = 0; k < i; k++) v = fma(-sL[i][k], xv[k], v);
    xv[i] = v / sL[i][i];
  }
  double *out = Dinv + (size_t)blockIdx.x * (CB * CB);
#pragma unroll
  for (int i = 0; i < CB; i++) out[i * CB + lane] = xv[i];
}

int sinterp_krige_inv32(gsl_sinterp_hip_ctx *ctx, size_t n, const double *d_llt, size_t lda, double *d_dinv)
{
  hipLaunchKernelGGL(krige_inv32_kernel, dim3((unsigned)((n + CB - 1) / CB)), dim3(64), 0, ctx->stream, d_llt, lda, n, d_dinv);
  LAUNCH_CHECK(ctx);
  return ST_SUCCESS;
}

/* ------------------------------------------------------------------------ */
/* the diagonal step: Z[:, J] <- Z[:, J] L_JJ^-T for the 128-column block J at j0, and q_k += |Z[k][J]|^2.
   The same body as chol_trsm128_kernel (chol.hip), shared through trsm128.h: 64 rows per workgroup, wave w owns rows
   16w .. 16w+15 for all four 32-column steps c (no workgroup barrier between the steps),
       Y_c = Z_c - sum_{p<c} X_p L_cp^T,     X_c = Y_c Dinv_c^T,
   the Z tile, the six off-diagonal 32 x 32 blocks of L_JJ and the four Dinv blocks staged in LDS with one round trip.
   This kernel's own part: the right-hand matrix (Z, ldw) and the factor (L, lda) are different buffers, rows of L and
   Dinv blocks past n (the last, partial block) read as zeros, and the squared row norms are accumulated on the way out:
   a workgroup owns the same rows at every step of the recursion, so q needs no atomics.  rows is a multiple of 64 (KV_RP). */
__global__ void __launch_bounds__(256)
krige_trsm128_kernel(double *__restrict__ Z, size_t ldw, const double *__restrict__ L, size_t lda, size_t n, size_t j0,
                     const double *__restrict__ Dinvg, double *__restrict__ q)
{
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int tid = threadIdx.x;
  const size_t row0 = (size_t)blockIdx.x * 64;
  trsm128_stage(sm, tid,
                [=](int r) { return Z + (row0 + r) * ldw + j0; },
                [=](int bi, int bj, int r, int k) { const size_t gr = j0 + bi * 32 + r; return gr < n ? L[gr * lda + j0 + bj * 32 + k] : 0.0; },
                [=](int b, int r, int k) { const size_t blk = j0 / CB + b; return blk * CB < n ? Dinvg[blk * 1024 + r * 32 + k] : 0.0; });
  __syncthreads();
  const int lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4;
  double qs[4] = {0.0, 0.0, 0.0, 0.0};                      /* this lane's share of |X[row fq + 4 rg]|^2 */
  trsm128_solve(sm, tid, [=, &qs](int c, int f, int rg, double v) {
    Z[(row0 + wave * 16 + fq + 4 * rg) * ldw + j0 + c * 32 + f * 16 + fr] = v;
    qs[rg] = fma(v, v, qs[rg]);
  });
#pragma unroll
  for (int rg = 0; rg < 4; rg++) {
    double v = qs[rg];
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 8);
    if (fr == 0) q[row0 + wave * 16 + fq + 4 * rg] += v;
  }
}

/* var_k = 1 - q_k + (1 - a_k)^2 / d; a_k = b^T k(y_k) is in var[k] on entry.  No clamping: at a data site with nugget 0
   the result is rounding residue of either sign. */
__global__ void __launch_bounds__(256)
krige_combine_kernel(double *__restrict__ var, const double *__restrict__ q, size_t rows, double denom)
{
  const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= rows) return;
  const double t = 1.0 - var[k];
  var[k] = (1.0 - q[k]) + t * t / denom;
}

__global__ void __launch_bounds__(256)
krige_ones_kernel(double *__restrict__ b, size_t n)
{
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) b[i] = 1.0;
}

/* v < 0 -> 0 (a NaN stays a NaN) */
__global__ void __launch_bounds__(256)
clamp_nonnegative_kernel(double *__restrict__ v, size_t m)
{
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < m; k += stride)
    if (v[k] < 0.0) v[k] = 0.0;
}

/* ------------------------------------------------------------------------ */
template <int KIND>
static void launch_cross_fill(gsl_sinterp_hip_ctx *ctx, double coef, const double *tbl, const double *d_x, size_t n, int dim, size_t xtda,
                              const double *d_y, size_t rows, size_t ytda, double *Z, size_t ldw, size_t rows_pad, double *q)
{
  const dim3 grid((unsigned)(ldw / 128), (unsigned)(rows_pad / 16));
  with_dim(dim, [&](auto D) {
    hipLaunchKernelGGL((krige_cross_fill_kernel<KIND, decltype(D)::value>), grid, dim3(256), 0, ctx->stream, coef, tbl, d_x, n, xtda, d_y, rows,
                       ytda, Z, ldw, q);
  });
}

/* Z[:, c0 : c0 + cw] -= Z[:, k0 : k0 + kw] L[c0 : c0 + cw, k0 : k0 + kw]^T; a partial last block (c0 + cw = n, not a
   multiple of 128) goes in a call of its own so that the blocks before it keep the full-tile path */
int sinterp_kv_update(const KvPass &p, size_t c0, size_t cw, size_t k0, size_t kw)
{
  if (cw == 0 || kw == 0) return ST_SUCCESS;
  const size_t whole = cw / PB * PB;
  int st = ST_SUCCESS;
  if (whole)
    st = sinterp_gemm_minus(p.ctx, p.rows_pad, whole, kw, p.Z + k0, p.ldw, p.L + c0 * p.lda + k0, p.lda, 0, p.Z + c0, p.ldw, 0);
  if (!st && cw > whole)
    st = sinterp_gemm_minus(p.ctx, p.rows_pad, cw - whole, kw, p.Z + k0, p.ldw, p.L + (c0 + whole) * p.lda + k0, p.lda, 0,
                            p.Z + c0 + whole, p.ldw, 0);
  return st;
}

int sinterp_kv_diag(const KvPass &p, size_t j0)
{
  const size_t lds = (size_t)TRSM128_LDS * sizeof(double);
  int st = sinterp_func_lds(p.ctx, (const void *)krige_trsm128_kernel, (int)lds);
  if (st) return st;
  hipLaunchKernelGGL(krige_trsm128_kernel, dim3((unsigned)(p.rows_pad / 64)), dim3(256), lds, p.ctx->stream, p.Z, p.ldw, p.L, p.lda, p.n,
                     j0, p.dinv, p.q);
  return ST_SUCCESS;
}

/* columns [j0, j0 + w) given that everything left of j0 has been applied: halve (on a 128-column boundary) down to
   single blocks */
static int kv_solve_range(const KvPass &p, size_t j0, size_t w)
{
  if (w <= PB) return sinterp_kv_diag(p, j0);
  size_t w1 = ((w / 2 + PB - 1) / PB) * PB;
  if (w1 >= w) w1 = w - PB;
  int st = kv_solve_range(p, j0, w1);
  if (!st) st = sinterp_kv_update(p, j0 + w1, w - w1, j0, w1);
  if (!st) st = kv_solve_range(p, j0 + w1, w - w1);
  return st;
}

/* Left-looking over panels of `panel` columns: the update of a panel reads ALL columns left of it in one product with
   K = j0, then the panel is solved on its own.  panel = 128 (the default) is the plain left-looking recursion: one
   update and one diagonal step per block.  Wider panels (developer switch GSL_SINTERP_KRIGE_PANEL = columns) recurse
   inside the panel as the factorisation's chol_split does; kept for tools/krige_variance_time.py, the default is the
   simpler scheme ("Kriging variance": what has and has not been measured). */
static int kv_solve(const KvPass &p, size_t panel)
{
  for (size_t j0 = 0; j0 < p.n; j0 += panel) {
    const size_t w = p.n - j0 < panel ? p.n - j0 : panel;
    int st = sinterp_kv_update(p, j0, w, 0, j0);
    if (!st) st = kv_solve_range(p, j0, w);
    if (st) return st;
  }
  return ST_SUCCESS;
}

/* the fill and the whole substitution for the joint covariance (krige_cov.hip): a run-time kind, the default panel */
int sinterp_kv_cross_fill(gsl_sinterp_hip_ctx *ctx, int kind, double coef, const double *tbl, const double *d_x, size_t n, int dim,
                          size_t xtda, const double *d_y, size_t rows, size_t ytda, double *Z, size_t ldw, size_t rows_pad, double *q)
{
  with_kind(kind, [&](auto K) {
    if constexpr (kind_is_pd(decltype(K)::value))            /* the callers require kind_is_pd(kind) */
      launch_cross_fill<decltype(K)::value>(ctx, coef, tbl, d_x, n, dim, xtda, d_y, rows, ytda, Z, ldw, rows_pad, q);
  });
  LAUNCH_CHECK(ctx);
  return ST_SUCCESS;
}

int sinterp_kv_solve(const KvPass &p) { return kv_solve(p, PB); }

extern "C" size_t gsl_sinterp_hip_krige_variance_work(size_t n, size_t chunk)
{
  /* Z (rows padded to KV_RP, pitch n rounded up to 128) + q + two words to align Z to 16 bytes */
  return round_up(chunk ? chunk : 1, KV_RP) * (round_up(n, PB) + 1) + 2;
}

extern "C" int gsl_sinterp_hip_krige_variance_prepare(gsl_sinterp_hip_ctx *ctx, size_t n, const double *d_llt, size_t lda,
                                                      double *d_b, double *d_dinv, double *h_denom)
{
  REQUIRE(ctx, ctx != NULL, ST_EFAULT);
  HIP_OK(ctx, hipSetDevice(ctx->device));
  EXCLUSIVE_SECTION(ctx);
  REQUIRE(ctx, lda >= n, ST_EINVAL);
  REQUIRE(ctx, h_denom != NULL && (n == 0 || (d_llt && d_b && d_dinv)), ST_EFAULT);
  *h_denom = 0.0;
  if (n == 0) return ST_SUCCESS;
  hipLaunchKernelGGL(krige_ones_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_b, n);
  int st = sinterp_krige_inv32(ctx, n, d_llt, lda, d_dinv);
  if (st) return st;
  st = sinterp_cholesky_svx_multi(ctx, n, d_llt, lda, d_b, n, 1);                 /* b = (L L^T)^-1 1 */
  if (st) return st;
  double *h_b = (double *)malloc(n * sizeof(double));
  if (!h_b) return sinterp_fail(ctx, ST_ENOMEM, "krige_variance_prepare: host buffer", hipSuccess, __FILE__, __LINE__);
  hipError_t e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = hipMemcpy(h_b, d_b, n * sizeof(double), hipMemcpyDeviceToHost);
  if (e != hipSuccess) { free(h_b); return sinterp_fail(ctx, ST_EFAILED, "krige_variance_prepare: read back", e, __FILE__, __LINE__); }
  double sum = 0.0;
  for (size_t i = 0; i < n; i++) sum += h_b[i];                                   /* once per model: fixed order on the host */
  free(h_b);
  *h_denom = sum;
  if (!(sum != 0.0) || sum != sum)
    return sinterp_fail(ctx, ST_EDOM, "krige_variance_prepare: 1^T K^-1 1 = 0 (degenerate covariance matrix)", hipSuccess, __FILE__, __LINE__);
  return ST_SUCCESS;
}

extern "C" int gsl_sinterp_hip_krige_variance(gsl_sinterp_hip_ctx *ctx, int kind, double eps, const double *d_x, size_t n, int dim,
                                              size_t xtda, const double *d_llt, size_t lda, const double *d_b, const double *d_dinv,
                                              double denom, const double *d_y, size_t m, size_t ytda, double *d_var, double *d_work,
                                              size_t chunk)
{
  REQUIRE(ctx, ctx != NULL, ST_EFAULT);
  HIP_OK(ctx, hipSetDevice(ctx->device));
  EXCLUSIVE_SECTION(ctx);                          /* the stream-K updates spin on sibling workgroups */
  REQUIRE(ctx, dim >= 1 && dim <= 3 && xtda >= (size_t)dim && ytda >= (size_t)dim && lda >= n && chunk >= 1, ST_EINVAL);
  REQUIRE(ctx, kind_is_pd(kind), ST_EINVAL);       /* covariances: positive definite kernels */
  REQUIRE(ctx, (m == 0 || n == 0) || (d_x && d_llt && d_b && d_dinv && d_y && d_var && d_work), ST_EFAULT);
  if (m == 0 || n == 0) return ST_SUCCESS;
  if (chunk > ((size_t)1 << 19)) chunk = (size_t)1 << 19;      /* rows / 16 is a grid dimension */
  /* developer switch (tools/krige_variance_time.py): the panel width of the recursion, read once */
  static const size_t panel = [] {
    const int v = sinterp_env_int("GSL_SINTERP_KRIGE_PANEL", 0);
    return v >= PB ? (size_t)v / PB * PB : (size_t)PB;
  }();
  int st = sinterp_streamk_prepare(ctx);
  if (st) return st;
  const double *tbl = NULL;
  st = sinterp_rbf_exp2_table(ctx, &tbl);
  if (st) return st;
  const double coef = kernel_coef(kind, eps);
  /* a = b^T k(y) for every target at once, parked in d_var until the combine of its pass */
  st = gsl_sinterp_hip_rbf_eval(ctx, kind, eps, d_x, n, dim, xtda, d_b, d_y, m, ytda, d_var);
  if (st) return st;
  KvPass p;
  p.ctx = ctx; p.ldw = round_up(n, PB); p.L = d_llt; p.lda = lda; p.n = n; p.dinv = d_dinv;
  p.Z = (double *)(((uintptr_t)d_work + 15) & ~(uintptr_t)15);
  const size_t chunk_pad = round_up(chunk, KV_RP);
  p.q = p.Z + chunk_pad * p.ldw;
  for (size_t k0 = 0; k0 < m; k0 += chunk) {
    const size_t rows = m - k0 < chunk ? m - k0 : chunk;
    p.rows_pad = round_up(rows, KV_RP);
    with_kind(kind, [&](auto K) {
      if constexpr (kind_is_pd(decltype(K)::value))          /* kind_is_pd(kind) was required above */
        launch_cross_fill<decltype(K)::value>(ctx, coef, tbl, d_x, n, dim, xtda, d_y + k0 * ytda, rows, ytda, p.Z, p.ldw, p.rows_pad, p.q);
    });
    LAUNCH_CHECK(ctx);
    st = kv_solve(p, panel);
    if (st) return st;
    hipLaunchKernelGGL(krige_combine_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, ctx->stream, d_var + k0, (const double *)p.q,
                       rows, denom);
    LAUNCH_CHECK(ctx);
  }
  return ST_SUCCESS;
}

/* ------------------------------------------------------------------------ */
/* The variance of universal kriging (drift.hip):
       sigma^2(y) = 1 - |L^-1 k|^2 + r^T S^-1 r,     r = p(u(y)) - B^T k(y),     B = K^-1 P,  S = P^T B = Ls Ls^T.
   |L^-1 k|^2 is the recursion above, untouched; B^T k comes per pass from the fields sweep with the q columns of B as
   weights, into a rows x q scratch behind q; drift_var_combine_kernel takes the place of krige_combine_kernel. */
extern "C" size_t gsl_sinterp_hip_ukrige_variance_work(size_t n, size_t chunk, size_t q)
{
  return gsl_sinterp_hip_krige_variance_work(n, chunk) + round_up(chunk ? chunk : 1, KV_RP) * q;
}

extern "C" int gsl_sinterp_hip_ukrige_variance(gsl_sinterp_hip_ctx *ctx, int kind, double eps, int order, const double *h_shift,
                                               const double *h_scale, const double *d_x, size_t n, int dim, size_t xtda,
                                               const double *d_llt, size_t lda, const double *d_B, size_t ldb, const double *d_dinv,
                                               const double *h_L, const double *d_y, size_t m, size_t ytda, double *d_var,
                                               double *d_work, size_t chunk)
{
  REQUIRE(ctx, ctx != NULL, ST_EFAULT);
  HIP_OK(ctx, hipSetDevice(ctx->device));
  EXCLUSIVE_SECTION(ctx);                          /* the stream-K updates spin on sibling workgroups */
  REQUIRE(ctx, dim >= 1 && dim <= 3 && xtda >= (size_t)dim && ytda >= (size_t)dim && lda >= n && ldb >= n && chunk >= 1, ST_EINVAL);
  REQUIRE(ctx, kind_is_pd(kind) && (order == 1 || order == 2), ST_EINVAL);
  REQUIRE(ctx, h_shift && h_scale && h_L, ST_EFAULT);
  REQUIRE(ctx, (m == 0 || n == 0) || (d_x && d_llt && d_B && d_dinv && d_y && d_var && d_work), ST_EFAULT);
  if (m == 0 || n == 0) return ST_SUCCESS;
  if (chunk > ((size_t)1 << 19)) chunk = (size_t)1 << 19;      /* rows / 16 is a grid dimension */
  const size_t q = gsl_sinterp_hip_drift_terms(dim, order);
  int st = sinterp_streamk_prepare(ctx);
  if (st) return st;
  const double *tbl = NULL;
  st = sinterp_rbf_exp2_table(ctx, &tbl);
  if (st) return st;
  const double coef = kernel_coef(kind, eps);
  KvPass p;
  p.ctx = ctx; p.ldw = round_up(n, PB); p.L = d_llt; p.lda = lda; p.n = n; p.dinv = d_dinv;
  p.Z = (double *)(((uintptr_t)d_work + 15) & ~(uintptr_t)15);
  const size_t chunk_pad = round_up(chunk, KV_RP);
  p.q = p.Z + chunk_pad * p.ldw;
  double *bk = p.q + chunk_pad;                    /* rows x q: B^T k(y) of the pass */
  for (size_t k0 = 0; k0 < m; k0 += chunk) {
    const size_t rows = m - k0 < chunk ? m - k0 : chunk;
    p.rows_pad = round_up(rows, KV_RP);
    st = gsl_sinterp_hip_rbf_eval_fields(ctx, kind, eps, NULL, d_x, n, dim, xtda, d_B, ldb, q, d_y + k0 * ytda, rows, ytda, bk, q, 0);
    if (st) return st;
    with_kind(kind, [&](auto K) {
      if constexpr (kind_is_pd(decltype(K)::value))          /* kind_is_pd(kind) was required above */
        launch_cross_fill<decltype(K)::value>(ctx, coef, tbl, d_x, n, dim, xtda, d_y + k0 * ytda, rows, ytda, p.Z, p.ldw, p.rows_pad, p.q);
    });
    LAUNCH_CHECK(ctx);
    st = kv_solve(p, PB);                          /* the default panel; GSL_SINTERP_KRIGE_PANEL is krige_variance's developer switch */
    if (st) return st;
    st = sinterp_drift_var_combine(ctx, order, h_shift, h_scale, h_L, dim, d_y + k0 * ytda, rows, ytda, bk, p.q, d_var + k0);
    if (st) return st;
  }
  return ST_SUCCESS;
}

extern "C" int gsl_sinterp_hip_krige_variance_clamp(gsl_sinterp_hip_ctx *ctx, double *d_v, size_t m)
{
  REQUIRE(ctx, ctx != NULL, ST_EFAULT);
  HIP_OK(ctx, hipSetDevice(ctx->device));
  REQUIRE(ctx, m == 0 || d_v, ST_EFAULT);
  if (m == 0) return ST_SUCCESS;
  size_t blocks = (m + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(clamp_nonnegative_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, d_v, m);
  LAUNCH_CHECK(ctx);
  return ST_SUCCESS;
}
