/*
 * rbf_phi.h -- the radial kernels phi(r^2) as the fill and the sweeps evaluate them (table-driven exp2 / log),
 * shared by rbf.hip and krige_var.hip so that a covariance is the same number wherever it is formed.
 * The tables themselves live in rbf.hip (g_rbf_tables); other translation units get the device address of the
 * exp2 table from sinterp_rbf_exp2_table (common.h).
 */
#ifndef SINTERP_RBF_PHI_H
#define SINTERP_RBF_PHI_H

#define TBL_BITS 8
#define TBL_N (1 << TBL_BITS)

/* tables live in global memory (built once per context on first use) and are
   copied into LDS by each workgroup */
#define LOG_BITS 8
#define LOG_N (1 << LOG_BITS)
#define LOG_COPIES 8                  /* LDS replicas of the (1/c, ln c) table: one per PAIR of lanes of a ds_read_b128 pass */
#define LOG_LDS (LOG_N * LOG_COPIES * 2)   /* doubles: 32 KiB */

/* 2^t for t <= 0 (and moderate t > 0): t*256 = k + f, |f| <= 1/2;
   2^t = 2^(k>>8) * T[k&255] * exp(f ln2/256), degree-4 Taylor (|arg| <= 1.36e-3,
   truncation 3.8e-17) */
__device__ __forceinline__ double exp2_tbl(double t, const double *__restrict__ tbl)
{
  t = fmax(t, -1100.0);
  const double ts = t * (double)TBL_N;
  const double kf = rint(ts);
  const double f = ts - kf;                       /* exact */
  const int k = (int)kf;
  const double a = f * (0.693147180559945309417232 / TBL_N);
  double p = fma(a, 1.0 / 24.0, 1.0 / 6.0);
  p = fma(p, a, 0.5);
  p = fma(p, a, 1.0);
  p = fma(p, a, 1.0);
  return ldexp(tbl[k & (TBL_N - 1)] * p, k >> TBL_BITS);
}

/* ln(v), v >= 0 finite: v = 2^e m with m in [1/2, 1) from v_frexp_mant_f64 / v_frexp_exp_i32_f64
   (one instruction each; splitting the high word with integer ops costs five more).  Table index =
   top 8 mantissa bits; c_i = (1 + (i+0.5)/256)/2 is the midpoint of m's bin, u = m/c_i - 1,
   |u| <= 2^-9, log1p(u) to u^5 (|u|^6/6 < 1e-17);  ln v = e ln2 + ln c_i + log1p(u).
   (Until round 3: 128 entries, |u| <= 2^-8, one more term -- the larger table trades one FMA of the ~22 VALU
   instructions per pair for nothing: C2 sweep 2.87 -> 2.80 ms.)
   The lookup is data dependent per lane; a plain LDS table costs ~3x in bank conflicts (measured:
   31 % of the TPS sweep).  The table is therefore stored as 8 interleaved copies of the 16-byte
   pair {1/c_i, ln c_i}: row i is 128 bytes = 32 banks, lane l reads copy l & 7, so a 16-lane pass of the
   ds_read_b128 meets at most a two-way conflict (lanes l and l + 8) whatever the indices are -- 16 cycles per
   wave and pair against >= 80 of VALU work (16 copies of 128 entries, conflict free, were the same 32 KiB).
   v = 0 gives a finite value (m = 0 -> u = -1), which the callers multiply by r^2 = 0. */
template <int COPIES>
__device__ __forceinline__ double log_tbl(double v, const double *__restrict__ lt_lane)
{
  const int idx = (__double2hiint(v) >> (20 - LOG_BITS)) & (LOG_N - 1);
  const double2 t = *reinterpret_cast<const double2 *>(lt_lane + idx * (COPIES * 2));
  const double m = __builtin_amdgcn_frexp_mant(v);
  const int e = __builtin_amdgcn_frexp_exp(v);
  const double u = fma(m, t.x, -1.0);
  double p = fma(u, 0.2, -0.25);
  p = fma(p, u, 1.0 / 3.0);
  p = fma(p, u, -0.5);
  p = fma(p, u, 1.0);
  return fma((double)e, 0.693147180559945309417232, fma(p, u, t.y));
}

template <int KIND, int COPIES>
__device__ __forceinline__ double phi_r2(double r2, double coef, const double *__restrict__ t0,
                                         const double *__restrict__ lt_lane)
{
  if (KIND == GSL_SINTERP_RBF_GAUSSIAN) {
    return exp2_tbl(r2 * coef, t0);                /* coef = -eps^2 log2(e) */
  } else if (KIND == GSL_SINTERP_RBF_WENDLAND) {
    /* coef = eps; exactly 0 at and beyond the support radius (u <= 0); a NaN distance stays NaN */
    const double t = coef * sqrt(r2), u = 1.0 - t, u2 = u * u;
    return u <= 0.0 ? 0.0 : (u2 * u2) * fma(4.0, t, 1.0);
  } else {
    /* r^2 ln r = 0.5 r^2 ln r^2; the 0.5 is folded into the caller's weight (coef = 0.5 in fill).
       r2 = 0 (target on a centre): log_tbl returns a finite value, the product is exactly 0 */
    return (coef * r2) * log_tbl<COPIES>(r2, lt_lane);
  }
}

/* phi as phi_r2 returns it (the same expressions: the same bits) and, from the same exp2 / sqrt / log, the radial
   factor of the gradient:  grad_y phi(|y - x|) = psi(r^2) (y - x),  psi = phi'(r) / r.  *psi receives psi WITHOUT
   its constant, which the sweeps apply once per target (rbf_grad_scale in rbf.hip):
       Gaussian    psi = -2 eps^2 phi               *psi = phi
       Wendland    psi = -20 eps^2 (1 - eps r)_+^3  *psi = (1 - eps r)_+^3
       thin-plate  psi = ln r^2 + 1                 *psi = ln r^2 + 1   (the constant 2 undoes the caller's half weight)
   None of them divides and none is singular at r = 0: the thin-plate psi is the finite log_tbl(0) + 1 there, and the
   callers multiply it by y - x = 0. */
template <int KIND, int COPIES>
__device__ __forceinline__ double phi_psi_r2(double r2, double coef, const double *__restrict__ t0,
                                             const double *__restrict__ lt_lane, double *__restrict__ psi)
{
  if (KIND == GSL_SINTERP_RBF_GAUSSIAN) {
    const double v = exp2_tbl(r2 * coef, t0);
    *psi = v;
    return v;
  } else if (KIND == GSL_SINTERP_RBF_WENDLAND) {
    const double t = coef * sqrt(r2), u = 1.0 - t, u2 = u * u;
    *psi = u <= 0.0 ? 0.0 : u2 * u;
    return u <= 0.0 ? 0.0 : (u2 * u2) * fma(4.0, t, 1.0);
  } else {
    const double L = log_tbl<COPIES>(r2, lt_lane);
    *psi = L + 1.0;
    return (coef * r2) * L;
  }
}

#endif
