/*
 * krige_cov.hip -- the joint posterior covariance of kriging at two target sets and conditional simulation, from the
 * Cholesky factor K = L L^T and the drift data that the variance entries (krige_var.hip) already use:
 *
 *     Sigma_ab = C(|ya_i - yb_j|) - Z_a Z_b^T + T_a T_b^T,     Z = k(Y)^T L^-T,   row i of T: t_i = Ls^-1 (p(u(y_i)) - B^T k(y_i)),
 *
 * B = K^-1 P, S = P^T B = Ls Ls^T; ordinary kriging is q = 1 with B = b = K^-1 1 and Ls = sqrt(1^T b).  Sill 1, the nugget
 * is measurement noise (C has none, also for coincident targets).  The diagonal of Sigma_aa is the kriging variance.
 *
 *     T         the fields sweep (rbf.hip) with the q columns of B as weights, then sinterp_drift_cov_terms (drift.hip)
 *     Z         ALL rows at once, Z_a on top of Z_b (rows of each padded to 128, pitch n rounded up to 128): the fill and
 *               ONE blocked substitution of krige_var.hip serve both sets
 *     seed      Cov[i][j] = C(|ya_i - yb_j|) + t_i . t_j                   (krige_cov_seed_kernel)
 *     product   Cov -= Z_a Z_b^T                                           (gemm.hip, fp64 MFMA, straight into the output)
 *     mirror    with one set only the tiles on and below the diagonal are seeded and multiplied; the strict lower triangle
 *               is then copied to the upper one: symmetric to the bit  (krige_cov_mirror_kernel)
 *
 * (ma + mb) N^2 flops in the substitution, ma mb N in the product.  Simulation factors Sigma_YY + jitter I with the blocked
 * Cholesky (chol.hip) and multiplies the factor with the caller's standard normals through the same GEMM.
 */
#include "common.h"
#include <math.h>
#include "chol_potrf.h"
#include "rbf_phi.h"

#define KC_RP 128   /* rows of a target set are padded to this, as a pass of the variance is */
#define KC_FILL_ROWS ((size_t)1 << 19)   /* rows / 16 is a grid dimension of the fill and of the seed */

/* ------------------------------------------------------------------------ */
/* seed: the workgroup shape of krige_cross_fill_kernel -- 256 threads -> 16 rows (targets of a) x 128 columns (targets of
   b), 2 columns per lane: one 16-byte store where `wide` (Cov 16-byte aligned, ctda even), two 8-byte stores otherwise.
   A lane keeps the coordinates and the Q entries of t of its two columns in registers; the row's are wave-uniform.
   Nothing outside ma x mb is written.  lower: the tiles strictly above the diagonal are skipped (row0 = the first row of
   this launch in the whole matrix).  A NaN distance gives NaN whatever the kernel makes of it. */
template <int KIND, int DIM, int Q>
__global__ void __launch_bounds__(256)
krige_cov_seed_kernel(double coef, const double *__restrict__ tbl, const double *__restrict__ ya, size_t ma, size_t yatda,
                      const double *__restrict__ ta, const double *__restrict__ yb, size_t mb, size_t ybtda,
                      const double *__restrict__ tb, double *__restrict__ C, size_t ctda, size_t row0, int lower, int wide)
{
  __shared__ double s_t0[kind_uses_exp2(KIND) ? TBL_N : 1];
  if (kind_uses_exp2(KIND)) s_t0[threadIdx.x] = tbl[threadIdx.x];      /* TBL_N = 256 = the block */
  __syncthreads();
  if (lower && (size_t)blockIdx.x * 128 > row0 + (size_t)blockIdx.y * 16 + 15) return;
  const size_t j0 = ((size_t)blockIdx.x * 64 + (threadIdx.x & 63)) * 2;
  const size_t ibase = (size_t)blockIdx.y * 16 + (threadIdx.x >> 6) * 4;
  const bool ca = j0 < mb, cb = j0 + 1 < mb;
  if (!ca) return;
  const size_t j1 = cb ? j0 + 1 : j0;                                  /* the second column of the last odd pair is not stored */
  double xa[DIM], xb[DIM], tja[Q], tjb[Q];
#pragma unroll
  for (int c = 0; c < DIM; c++) { xa[c] = yb[j0 * ybtda + c]; xb[c] = yb[j1 * ybtda + c]; }
#pragma unroll
  for (int t = 0; t < Q; t++) { tja[t] = tb[j0 * Q + t]; tjb[t] = tb[j1 * Q + t]; }
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const size_t i = ibase + r;
    if (i >= ma) break;
    double ra = 0.0, rb = 0.0;
#pragma unroll
    for (int c = 0; c < DIM; c++) {
      const double yi = ya[i * yatda + c];
      const double da = yi - xa[c], db = yi - xb[c];
      ra = fma(da, da, ra); rb = fma(db, db, rb);
    }
    double va = phi_r2<KIND, 1>(ra, coef, s_t0, s_t0), vb = phi_r2<KIND, 1>(rb, coef, s_t0, s_t0);
#pragma unroll
    for (int t = 0; t < Q; t++) {
      const double ti = ta[i * Q + t];
      va = fma(ti, tja[t], va); vb = fma(ti, tjb[t], vb);
    }
    if (ra != ra) va = ra;
    if (rb != rb) vb = rb;
    double *out = C + i * ctda + j0;
    if (wide && cb) {
      *reinterpret_cast<double2 *>(out) = make_double2(va, vb);        /* C 16-byte aligned, ctda and j0 even */
    } else {
      out[0] = va;
      if (cb) out[1] = vb;
    }
  }
}

/* lower -> upper in 32 x 32 tiles through LDS: the workgroup of tile (ti, tj), tj >= ti, reads the tile (tj, ti) below the
   diagonal by rows and writes its transpose by rows (both coalesced; the column read of the 33-double pitch touches 64
   different banks per half wave).  On the diagonal tile only the entries above the diagonal are written. */
__global__ void __launch_bounds__(256)
krige_cov_mirror_kernel(double *__restrict__ C, size_t ctda, size_t m)
{
  __shared__ double s[32][33];
  const size_t ti = blockIdx.y, tj = blockIdx.x;
  if (tj < ti) return;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) {
    const size_t gr = tj * 32 + r, gc = ti * 32 + tx;
    if (gr < m && gc < m) s[r][tx] = C[gr * ctda + gc];
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const size_t gr = ti * 32 + r, gc = tj * 32 + tx;
    if (gr < m && gc < m && gc > gr) C[gr * ctda + gc] = s[tx][r];
  }
}

/* ------------------------------------------------------------------------ */
/* simulation, before the factorisation: A[i][i] += jitter */
__global__ void __launch_bounds__(256)
krige_sim_jitter_kernel(double *__restrict__ A, size_t lda, size_t m, double jitter)
{
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < m) A[i * lda + i] += jitter;
}

/* simulation, after it: the strict upper triangle of the factor is zeroed (the factorisation leaves its input there),
   Out[i][s] = mean_i and W[i][s] = -sqrt(sigma2) Zn[i][s] (W dense, m x n_draws), so that Out -= A W finishes the draws.
   fail: the factorisation met a pivot that is not positive -- every entry of Out is NaN and nothing else is touched.
   Row i is served by the workgroups with blockIdx.y = i mod gridDim.y, its columns by blockIdx.x. */
__global__ void __launch_bounds__(256)
krige_sim_stage_kernel(double *__restrict__ A, size_t lda, size_t m, const double *__restrict__ mean, const double *__restrict__ zn,
                       size_t ztda, size_t n_draws, double scale, double *__restrict__ out, size_t otda, double *__restrict__ W, int fail)
{
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  for (size_t i = blockIdx.y; i < m; i += gridDim.y) {
    if (c < n_draws) {
      out[i * otda + c] = fail ? __longlong_as_double(0x7FF8000000000000LL) : mean[i];
      if (!fail) W[i * n_draws + c] = -scale * zn[i * ztda + c];
    }
    if (!fail && c > i && c < m) A[i * lda + c] = 0.0;
  }
}

/* ------------------------------------------------------------------------ */
/* (kind, dim, order) -> seed instance; Q = the number of drift functions (gsl_sinterp_hip_drift_terms) */
template <class F> static void with_kind_dim_order(int kind, int dim, int order, F &&f)
{
  with_kind(kind, [&](auto K) {
    if constexpr (kind_is_pd(decltype(K)::value)) {          /* the callers require kind_is_pd(kind) */
      with_dim(dim, [&](auto D) {
        constexpr int d = decltype(D)::value;
        if (order == 0) f(K, D, ic<1>());
        else if (order == 1) f(K, D, ic<d + 1>());
        else f(K, D, ic<(d + 1) * (d + 2) / 2>());
      });
    }
  });
}

struct KcLayout {
  double *Z, *qn, *ta, *tb;
  size_t ldw, ma_pad, mb_pad;
};

static KcLayout kc_layout(double *d_work, size_t n, size_t ma, size_t mb, size_t q, bool sym)
{
  KcLayout w;
  w.ldw = round_up(n, PB);
  w.ma_pad = round_up(ma, KC_RP);
  w.mb_pad = sym ? 0 : round_up(mb, KC_RP);
  w.Z = (double *)(((uintptr_t)d_work + 15) & ~(uintptr_t)15);
  w.qn = w.Z + (w.ma_pad + w.mb_pad) * w.ldw;
  w.ta = w.qn + (w.ma_pad + w.mb_pad);
  w.tb = sym ? w.ta : w.ta + ma * q;
  return w;
}

extern "C" size_t gsl_sinterp_hip_krige_covariance_work(size_t n, size_t ma, size_t mb, size_t q)
{
  /* Z_a over Z_b (rows padded to 128, pitch n rounded up to 128) + their squared row norms + T_a, T_b + two words to
     align Z to 16 bytes; mb = 0: one set */
  const size_t rows = round_up(ma ? ma : 1, KC_RP) + (mb ? round_up(mb, KC_RP) : 0);
  return rows * (round_up(n, PB) + 1) + (ma + mb) * q + 2;
}

/* T and Z of one target set: rows of T at d_t, rows of Z from row z0 of the work matrix */
static int kc_fill_set(gsl_sinterp_hip_ctx *ctx, int kind, double eps, double coef, const double *tbl, int order, const double *h_shift,
                       const double *h_scale, const double *h_L, const double *d_x, size_t n, int dim, size_t xtda, const double *d_B,
                       size_t ldb, size_t q, const double *d_y, size_t m, size_t ytda, const KcLayout &w, size_t z0, size_t m_pad,
                       double *d_t)
{
  int st = gsl_sinterp_hip_rbf_eval_fields(ctx, kind, eps, NULL, d_x, n, dim, xtda, d_B, ldb, q, d_y, m, ytda, d_t, q, 0);
  if (!st) st = sinterp_drift_cov_terms(ctx, order, h_shift, h_scale, h_L, dim, d_y, m, ytda, d_t);
  for (size_t r0 = 0; r0 < m_pad && !st; r0 += KC_FILL_ROWS) {
    const size_t rp = m_pad - r0 < KC_FILL_ROWS ? m_pad - r0 : KC_FILL_ROWS;
    const size_t rows = r0 >= m ? 0 : (m - r0 < rp ? m - r0 : rp);
    st = sinterp_kv_cross_fill(ctx, kind, coef, tbl, d_x, n, dim, xtda, d_y + r0 * ytda, rows, ytda, w.Z + (z0 + r0) * w.ldw, w.ldw, rp,
                               w.qn + z0 + r0);
  }
  return st;
}

extern "C" int gsl_sinterp_hip_krige_covariance(gsl_sinterp_hip_ctx *ctx, int kind, double eps, int order, const double *h_shift,
                                                const double *h_scale, const double *d_x, size_t n, int dim, size_t xtda,
                                                const double *d_llt, size_t lda, const double *d_B, size_t ldb, const double *d_dinv,
                                                const double *h_L, const double *d_ya, size_t ma, size_t yatda, const double *d_yb,
                                                size_t mb, size_t ybtda, double *d_cov, size_t ctda, double *d_work)
{
  REQUIRE(ctx, ctx != NULL, ST_EFAULT);
  HIP_OK(ctx, hipSetDevice(ctx->device));
  EXCLUSIVE_SECTION(ctx);                          /* the stream-K updates spin on sibling workgroups */
  const bool sym = d_yb == NULL;
  if (sym) mb = ma;
  REQUIRE(ctx, dim >= 1 && dim <= 3 && xtda >= (size_t)dim && yatda >= (size_t)dim && (sym || ybtda >= (size_t)dim), ST_EINVAL);
  REQUIRE(ctx, n >= 1 && lda >= n && ldb >= n && ctda >= mb, ST_EINVAL);
  REQUIRE(ctx, kind_is_pd(kind) && order >= 0 && order <= 2, ST_EINVAL);
  REQUIRE(ctx, h_L && (order == 0 || (h_shift && h_scale)), ST_EFAULT);
  if (ma == 0 || mb == 0) return ST_SUCCESS;
  REQUIRE(ctx, d_x && d_llt && d_B && d_dinv && d_ya && d_cov && d_work, ST_EFAULT);
  const size_t q = gsl_sinterp_hip_drift_terms(dim, order);
  int st = sinterp_streamk_prepare(ctx);
  if (st) return st;
  const double *tbl = NULL;
  st = sinterp_rbf_exp2_table(ctx, &tbl);
  if (st) return st;
  const double coef = kernel_coef(kind, eps);
  const KcLayout w = kc_layout(d_work, n, ma, mb, q, sym);
  st = kc_fill_set(ctx, kind, eps, coef, tbl, order, h_shift, h_scale, h_L, d_x, n, dim, xtda, d_B, ldb, q, d_ya, ma, yatda, w, 0, w.ma_pad,
                   w.ta);
  if (!st && !sym)
    st = kc_fill_set(ctx, kind, eps, coef, tbl, order, h_shift, h_scale, h_L, d_x, n, dim, xtda, d_B, ldb, q, d_yb, mb, ybtda, w, w.ma_pad,
                     w.mb_pad, w.tb);
  if (st) return st;
  KvPass p;
  p.ctx = ctx; p.Z = w.Z; p.ldw = w.ldw; p.rows_pad = w.ma_pad + w.mb_pad; p.L = d_llt; p.lda = lda; p.n = n; p.dinv = d_dinv; p.q = w.qn;
  st = sinterp_kv_solve(p);                        /* one pass: Z_a and Z_b together */
  if (st) return st;
  const double *yb = sym ? d_ya : d_yb;
  const size_t ybt = sym ? yatda : ybtda;
  const int wide = ((((uintptr_t)d_cov) & 15) == 0) && (ctda & 1) == 0;
  for (size_t r0 = 0; r0 < ma; r0 += KC_FILL_ROWS) {
    const size_t rows = ma - r0 < KC_FILL_ROWS ? ma - r0 : KC_FILL_ROWS;
    const dim3 grid((unsigned)((mb + 127) / 128), (unsigned)((rows + 15) / 16));
    with_kind_dim_order(kind, dim, order, [&](auto K, auto D, auto Q) {
      hipLaunchKernelGGL((krige_cov_seed_kernel<decltype(K)::value, decltype(D)::value, decltype(Q)::value>), grid, dim3(256), 0, ctx->stream,
                         coef, tbl, d_ya + r0 * yatda, rows, yatda, (const double *)w.ta + r0 * q, yb, mb, ybt, (const double *)w.tb,
                         d_cov + r0 * ctda, ctda, r0, sym ? 1 : 0, wide);
    });
    LAUNCH_CHECK(ctx);
  }
  const double *Zb = sym ? w.Z : w.Z + w.ma_pad * w.ldw;
  st = sinterp_gemm_minus(ctx, ma, mb, w.ldw, w.Z, w.ldw, Zb, w.ldw, 0, d_cov, ctda, sym ? 1 : 0);
  if (st) return st;
  if (sym && ma > 1) {
    const unsigned nt = (unsigned)((ma + 31) / 32);
    hipLaunchKernelGGL(krige_cov_mirror_kernel, dim3(nt, nt), dim3(256), 0, ctx->stream, d_cov, ctda, ma);
    LAUNCH_CHECK(ctx);
  }
  return ST_SUCCESS;
}

/* ------------------------------------------------------------------------ */
/* Conditional simulation on top of the two entries above: the m x m work matrix A (pitch m rounded up to even) and the
   m x n_draws scaled normals in front of the covariance's own work */
static inline size_t ks_lda(size_t m) { return round_up(m, 2); }

extern "C" size_t gsl_sinterp_hip_krige_simulate_work(size_t n, size_t m, size_t n_draws, size_t q)
{
  return m * ks_lda(m) + round_up(m * n_draws, 2) + 2 + gsl_sinterp_hip_krige_covariance_work(n, m, 0, q);
}

extern "C" int gsl_sinterp_hip_krige_simulate(gsl_sinterp_hip_ctx *ctx, int kind, double eps, int order, const double *h_shift,
                                              const double *h_scale, const double *d_x, size_t n, int dim, size_t xtda,
                                              const double *d_llt, size_t lda, const double *d_B, size_t ldb, const double *d_dinv,
                                              const double *h_L, const double *d_y, size_t m, size_t ytda, const double *d_mean,
                                              double sigma2, double jitter, const double *d_zn, size_t ztda, size_t n_draws,
                                              double *d_out, size_t otda, double *d_work)
{
  REQUIRE(ctx, ctx != NULL, ST_EFAULT);
  HIP_OK(ctx, hipSetDevice(ctx->device));
  EXCLUSIVE_SECTION(ctx);
  REQUIRE(ctx, n_draws >= 1 && ztda >= n_draws && otda >= n_draws, ST_EINVAL);
  REQUIRE(ctx, isfinite(sigma2) && sigma2 > 0.0 && isfinite(jitter) && jitter >= 0.0, ST_EINVAL);
  if (m == 0) return ST_SUCCESS;
  REQUIRE(ctx, d_mean && d_zn && d_out && d_work, ST_EFAULT);
  const size_t ldm = ks_lda(m);
  double *A = (double *)(((uintptr_t)d_work + 15) & ~(uintptr_t)15);
  double *W = A + m * ldm;
  double *cov_work = W + round_up(m * n_draws, 2);
  int st = gsl_sinterp_hip_krige_covariance(ctx, kind, eps, order, h_shift, h_scale, d_x, n, dim, xtda, d_llt, lda, d_B, ldb, d_dinv, h_L, d_y,
                                            m, ytda, NULL, 0, 0, A, ldm, cov_work);
  if (st) return st;
  hipLaunchKernelGGL(krige_sim_jitter_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, ctx->stream, A, ldm, m, jitter);
  LAUNCH_CHECK(ctx);
  int info = 0;
  st = sinterp_cholesky_decomp1_sym(ctx, m, A, ldm, &info);          /* waits for the pivot status */
  if (st && st != ST_EDOM) return st;
  const int fail = st == ST_EDOM;
  const size_t cols = fail ? n_draws : (m > n_draws ? m : n_draws);
  const dim3 grid((unsigned)((cols + 255) / 256), (unsigned)(m < 32768 ? m : 32768));
  hipLaunchKernelGGL(krige_sim_stage_kernel, grid, dim3(256), 0, ctx->stream, A, ldm, m, d_mean, d_zn, ztda, n_draws, sqrt(sigma2), d_out,
                     otda, W, fail);
  LAUNCH_CHECK(ctx);
  if (fail) {
    snprintf(ctx->err, sizeof ctx->err,
             "krige_simulate: the joint covariance of the targets plus jitter is not positive definite (pivot %d of %zu): targets on data "
             "sites of a nugget-free model, or repeated targets; every draw is NaN -- pass a jitter such as 1e-10", info, m);
    return ST_EDOM;
  }
  return sinterp_gemm_minus(ctx, m, n_draws, m, A, ldm, W, n_draws, 1, d_out, otda, 0);        /* Out = mean + sqrt(sigma2) A Zn */
}
