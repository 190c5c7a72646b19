/*
 * loo.hip -- leave-one-out residuals and variances from the Cholesky factor K = L L^T that the inits of routes 1 and 7
 * leave behind ("Leave-one-out").  Both come from the diagonal of the inverse,
 *
 *     g_i = (K^-1)_ii = sum_{k >= i} (L^-1)_ki^2 = |row i of L^-T|^2,
 *
 * plain SPD interpolant (Rippa):  e_i = w_i / g_i,  v_i = 1 / g_i;
 * ordinary kriging (Dubrule):     (A^-1)_ii = g_i - b_i^2 / d with b = K^-1 1, d = 1^T b:  e_i = w_i / (A^-1)_ii, v_i = 1 / (A^-1)_ii.
 *
 * g is the recursion of the kriging variance (krige_var.hip: Z <- Z L^-T, squared row norms on the way) started from
 * Z = I and made triangular.  Row i of L^-T is zero left of column i, so with the rows taken in chunks of c rows from c0
 * (both multiples of 128):
 *
 *     seed      Z[c0 + r][j] = (c0 + r == j) for j >= c0; columns < c0 are never written and never read
 *     step J    (128-column blocks from c0 / 128 on) rows [c0, R_J) are alive, R_J = min(c0 + c, 128 (J + 1)):
 *                 Z[c0 : min(c0 + c, 128 J), J] -= Z[same rows, c0 : 128 J] L[J, c0 : 128 J]^T     (sinterp_kv_update)
 *                 Z[c0 : R_J, J] <- Z[c0 : R_J, J] L_JJ^-T,  q_i += |Z[i][J]|^2                      (sinterp_kv_diag)
 *               the rows of later row blocks are still zero in column block J and are skipped
 *     result    g[c0 + r] = q[r]
 *
 * N^3 / 3 + O(c N^2) flops against N^3 for the variance entry at M = N.
 */
#include "common.h"
#include "chol_potrf.h"

/* rows of Z per pass: chunk rounded up to 128, at most n rounded up to 128 (and 2^19: rows / 16 is a grid dimension) */
static inline size_t loo_chunk_rows(size_t n, size_t chunk)
{
  size_t c = round_up(chunk ? chunk : 1, PB);
  const size_t all = round_up(n, PB);
  if (c > all) c = all;
  if (c > ((size_t)1 << 19)) c = (size_t)1 << 19;
  return c;
}

/* ------------------------------------------------------------------------ */
/* seed of one chunk: the workgroup shape of krige_cross_fill_kernel -- 256 threads -> 16 rows x 128 columns, 2 columns
   (one 16-byte store) per lane.  Row r of Z is row c0 + r of the identity, written from column c0 on (blockIdx.x counts
   128-column blocks from c0); rows >= n are zero.  The first column block also clears q. */
__global__ void __launch_bounds__(256)
loo_seed_kernel(double *__restrict__ Z, size_t ldw, size_t c0, size_t n, double *__restrict__ q)
{
  const size_t j0 = c0 + ((size_t)blockIdx.x * 64 + (threadIdx.x & 63)) * 2;
  const size_t rbase = (size_t)blockIdx.y * 16 + (threadIdx.x >> 6) * 4;
  if (blockIdx.x == 0 && (threadIdx.x & 63) < 4) q[rbase + (threadIdx.x & 63)] = 0.0;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const size_t i = c0 + rbase + r;
    const bool live = i < n;
    *reinterpret_cast<double2 *>(Z + (rbase + r) * ldw + j0) =                   /* Z 16-byte aligned, ldw and j0 even */
        make_double2(live && i == j0 ? 1.0 : 0.0, live && i == j0 + 1 ? 1.0 : 0.0);
  }
}

/* diag_i = g_i (b == NULL) or g_i - b_i^2 / denom; e[q][i] = w[q][i] / diag_i, v_i = 1 / diag_i.  One thread per site,
   the fields in a loop: every access of a wave is one contiguous run of a column.  No clamping. */
__global__ void __launch_bounds__(256)
loo_combine_kernel(size_t n, int nf, const double *__restrict__ g, const double *__restrict__ b, double denom,
                   const double *__restrict__ w, size_t ldw, double *__restrict__ e, size_t lde, double *__restrict__ v)
{
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double d = g[i];
  if (b) { const double bi = b[i]; d -= bi * bi / denom; }
  v[i] = 1.0 / d;
  for (int q = 0; q < nf; q++) e[(size_t)q * lde + i] = w[(size_t)q * ldw + i] / d;
}

/* ------------------------------------------------------------------------ */
extern "C" size_t gsl_sinterp_hip_chol_inv_diag_work(size_t n, size_t chunk)
{
  /* Z (pitch n rounded up to 128) + q + the inverted 32 x 32 diagonal blocks + two words to align Z to 16 bytes */
  const size_t c = loo_chunk_rows(n, chunk);
  return c * (round_up(n, PB) + 1) + (n + CB - 1) / CB * (CB * CB) + 2;
}

extern "C" int gsl_sinterp_hip_chol_inv_diag(gsl_sinterp_hip_ctx *ctx, size_t n, const double *d_llt, size_t lda, double *d_g,
                                             double *d_work, size_t chunk)
{
  REQUIRE(ctx, ctx != NULL, ST_EFAULT);
  HIP_OK(ctx, hipSetDevice(ctx->device));
  EXCLUSIVE_SECTION(ctx);                          /* the stream-K updates spin on sibling workgroups */
  REQUIRE(ctx, lda >= n && chunk >= 1, ST_EINVAL);
  REQUIRE(ctx, n == 0 || (d_llt && d_g && d_work), ST_EFAULT);
  if (n == 0) return ST_SUCCESS;
  int st = sinterp_streamk_prepare(ctx);
  if (st) return st;
  const size_t c = loo_chunk_rows(n, chunk);
  KvPass p;
  p.ctx = ctx; p.ldw = round_up(n, PB); p.L = d_llt; p.lda = lda; p.n = n;
  p.Z = (double *)(((uintptr_t)d_work + 15) & ~(uintptr_t)15);
  p.q = p.Z + c * p.ldw;
  double *dinv = p.q + c;
  p.dinv = dinv;
  st = sinterp_krige_inv32(ctx, n, d_llt, lda, dinv);
  if (st) return st;
  for (size_t c0 = 0; c0 < n; c0 += c) {
    const size_t rows = p.ldw - c0 < c ? p.ldw - c0 : c;                         /* the chunk's rows, padded to 128 */
    hipLaunchKernelGGL(loo_seed_kernel, dim3((unsigned)((p.ldw - c0) / PB), (unsigned)(rows / 16)), dim3(256), 0, ctx->stream, p.Z, p.ldw,
                       c0, n, p.q);
    LAUNCH_CHECK(ctx);
    for (size_t j0 = c0; j0 < n; j0 += PB) {
      const size_t cw = n - j0 < PB ? n - j0 : PB;
      p.rows_pad = j0 - c0 < rows ? j0 - c0 : rows;                              /* rows above block J's own */
      st = sinterp_kv_update(p, j0, cw, c0, j0 - c0);
      if (st) return st;
      p.rows_pad = j0 + PB - c0 < rows ? j0 + PB - c0 : rows;                    /* R_J - c0 */
      st = sinterp_kv_diag(p, j0);
      if (st) return st;
    }
    const size_t live = n - c0 < rows ? n - c0 : rows;
    HIP_OK(ctx, hipMemcpyAsync(d_g + c0, p.q, live * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  }
  return ST_SUCCESS;
}

extern "C" int gsl_sinterp_hip_loo_combine(gsl_sinterp_hip_ctx *ctx, size_t n, size_t nf, const double *d_g, const double *d_b,
                                           double denom, const double *d_w, size_t ldw, double *d_e, size_t lde, double *d_v)
{
  REQUIRE(ctx, ctx != NULL, ST_EFAULT);
  HIP_OK(ctx, hipSetDevice(ctx->device));
  REQUIRE(ctx, nf <= GSL_SINTERP_MAX_FIELDS && (nf == 0 || (ldw >= n && lde >= n)), ST_EINVAL);
  REQUIRE(ctx, n == 0 || (d_g && d_v && (nf == 0 || (d_w && d_e))), ST_EFAULT);
  if (n == 0) return ST_SUCCESS;
  hipLaunchKernelGGL(loo_combine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, n, (int)nf, d_g, d_b, denom, d_w, ldw,
                     d_e, lde, d_v);
  LAUNCH_CHECK(ctx);
  return ST_SUCCESS;
}
