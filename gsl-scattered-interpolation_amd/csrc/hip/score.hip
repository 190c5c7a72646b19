/*
 * score.hip -- the scalars of the model-selection criteria ("Model selection") from what one solve on routes
 * 1 / 7 leaves on the device: the Cholesky factor K = L L^T, the right-hand side f, the weights w and, for the
 * leave-one-out criterion, g = diag(K^-1) (loo.hip) with kriging's b = K^-1 1:
 *
 *     out[0] = sum_i 2 log L_ii            log|K|, a sum of logs (the product of N pivots over- or underflows long before)
 *     out[1] = sum_i f_i w_i               f^T K^-1 f, or (f - mu 1)^T K^-1 (f - mu 1) for kriging (1^T w = 0)
 *     out[2] = sum_i (w_i / diag_i)^2      the squared leave-one-out residuals; diag_i as loo_combine_kernel forms it
 *     out[3] = number of bad sites         L_ii or diag_i not > 0 or not finite
 *
 * ONE workgroup of 1024 threads: thread t adds sites t, t + 1024, .. in that order, then the 1024 partial sums are added
 * pairwise through LDS (t += t + 512, 256, .. 1).  No atomics, nothing depends on a grid: the same bits for the same
 * input on every run.  The diagonal is read with a stride of lda + 1 doubles, one 64-byte segment per site -- N
 * segments beside the N^3 / 3 flops that produced the factor.
 */
#include "common.h"
#include <math.h>

#define SCORE_THREADS 1024

__global__ void __launch_bounds__(SCORE_THREADS)
score_reduce_kernel(size_t n, const double *__restrict__ L, size_t lda, const double *__restrict__ f, const double *__restrict__ w,
                    const double *__restrict__ g, const double *__restrict__ b, double denom, double *__restrict__ out)
{
  __shared__ double s_log[SCORE_THREADS], s_fw[SCORE_THREADS], s_e2[SCORE_THREADS];
  __shared__ unsigned s_bad[SCORE_THREADS];
  const unsigned t = threadIdx.x;
  double a_log = 0.0, a_fw = 0.0, a_e2 = 0.0;
  unsigned bad = 0;
  for (size_t i = t; i < n; i += SCORE_THREADS) {
    const double lii = L[i * (lda + 1)], wi = w[i];
    bad += !(lii > 0.0 && isfinite(lii));
    a_log += 2.0 * log(lii);
    a_fw = fma(f[i], wi, a_fw);
    if (g) {
      double d = g[i];
      if (b) { const double bi = b[i]; d -= bi * bi / denom; }
      bad += !(d > 0.0 && isfinite(d));
      const double e = wi / d;
      a_e2 = fma(e, e, a_e2);
    }
  }
  s_log[t] = a_log; s_fw[t] = a_fw; s_e2[t] = a_e2; s_bad[t] = bad;
  __syncthreads();
  for (unsigned h = SCORE_THREADS / 2; h > 0; h >>= 1) {
    if (t < h) { s_log[t] += s_log[t + h]; s_fw[t] += s_fw[t + h]; s_e2[t] += s_e2[t + h]; s_bad[t] += s_bad[t + h]; }
    __syncthreads();
  }
  if (t == 0) { out[0] = s_log[0]; out[1] = s_fw[0]; out[2] = s_e2[0]; out[3] = (double)s_bad[0]; }
}

extern "C" int gsl_sinterp_hip_score_reduce(gsl_sinterp_hip_ctx *ctx, size_t n, const double *d_llt, size_t lda, const double *d_f,
                                            const double *d_w, const double *d_g, const double *d_b, double denom, double *d_out)
{
  REQUIRE(ctx, ctx != NULL, ST_EFAULT);
  HIP_OK(ctx, hipSetDevice(ctx->device));
  REQUIRE(ctx, lda >= n, ST_EINVAL);
  REQUIRE(ctx, n == 0 || (d_llt && d_f && d_w && d_out), ST_EFAULT);
  if (!d_out) return ST_SUCCESS;                   /* n == 0 and nowhere to write the zeros */
  hipLaunchKernelGGL(score_reduce_kernel, dim3(1), dim3(SCORE_THREADS), 0, ctx->stream, n, d_llt, lda, d_f, d_w, d_g, d_g ? d_b : NULL, denom,
                     d_out);
  LAUNCH_CHECK(ctx);
  return ST_SUCCESS;
}
