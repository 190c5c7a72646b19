/*
 * rbf_phi.h -- the radial kernels phi(r^2) as the fill and the sweeps evaluate them (table-driven exp2 / log),
 * shared by rbf.hip and krige_var.hip so that a covariance is the same number wherever it is formed, and the host-side
 * dispatch from a run-time kind / dimension to a kernel instance (with_kind, with_dim).
 * The tables themselves live in rbf.hip (g_rbf_tables); other translation units get the device address of the
 * exp2 table from sinterp_rbf_exp2_table (common.h).
 */
#ifndef SINTERP_RBF_PHI_H
#define SINTERP_RBF_PHI_H

#include <type_traits>

/* What a kind needs and how it is swept, as constexpr traits: every "load the exp2 table", every s_t0 size and the choice
   between the plain and the culled sweep ask these, so a new kind is one line here, one case each in kernel_coef and
   with_kind below (the only switch that maps a run-time kind to a kernel instance) and one branch in phi_r2 / phi_psi_r2.
     kind_uses_exp2   phi goes through exp2_tbl: the 256-entry table is copied to LDS
     kind_uses_log    phi goes through log_tbl (thin-plate)
     kind_is_culled   decays fast enough to be cut off: per-pair take test, tile culling, target sort (Gaussian, Wendland).
                      The Matern kinds and the inverse multiquadric take the plain sweep: every centre, input order
     kind_is_pd       positive definite: Cholesky route, usable as a kriging covariance */
constexpr bool kind_uses_exp2(int kind)
{
  return kind == GSL_SINTERP_RBF_GAUSSIAN || kind == GSL_SINTERP_RBF_MATERN32 || kind == GSL_SINTERP_RBF_MATERN52;
}
constexpr bool kind_uses_log(int kind) { return kind == GSL_SINTERP_RBF_TPS; }
constexpr bool kind_is_culled(int kind) { return kind == GSL_SINTERP_RBF_GAUSSIAN || kind == GSL_SINTERP_RBF_WENDLAND; }
constexpr bool kind_is_known(int kind) { return kind >= GSL_SINTERP_RBF_GAUSSIAN && kind <= GSL_SINTERP_RBF_IMQ; }
constexpr bool kind_is_pd(int kind) { return kind_is_known(kind) && kind != GSL_SINTERP_RBF_TPS; }

/* the per-kind constant that phi_r2 / phi_psi_r2 receive as coef */
static inline double kernel_coef(int kind, double eps)
{
  switch (kind) {
    case GSL_SINTERP_RBF_GAUSSIAN: return -(eps * eps) * 1.44269504088896340735992;
    case GSL_SINTERP_RBF_WENDLAND: return eps;
    case GSL_SINTERP_RBF_MATERN32: return 1.73205080756887729352745 * eps;      /* t = sqrt(3) eps r */
    case GSL_SINTERP_RBF_MATERN52: return 2.23606797749978969640917 * eps;      /* t = sqrt(5) eps r */
    case GSL_SINTERP_RBF_IMQ: return eps * eps;
    default: return 0.5;                                                         /* thin-plate: the half of r^2 ln r^2 */
  }
}

/* host side: a run-time kind / dimension picks the kernel instance.  f is a generic lambda that receives the value as a
   std::integral_constant and launches <decltype(arg)::value>; its result is passed on.  An unknown kind names the
   thin-plate instance: callers that accept only some kinds check first (kind_is_known, kind_is_pd). */
template <int V> using ic = std::integral_constant<int, V>;

template <class F> static auto with_kind(int kind, F &&f)
{
  switch (kind) {
    case GSL_SINTERP_RBF_WENDLAND: return f(ic<GSL_SINTERP_RBF_WENDLAND>());
    case GSL_SINTERP_RBF_GAUSSIAN: return f(ic<GSL_SINTERP_RBF_GAUSSIAN>());
    case GSL_SINTERP_RBF_MATERN32: return f(ic<GSL_SINTERP_RBF_MATERN32>());
    case GSL_SINTERP_RBF_MATERN52: return f(ic<GSL_SINTERP_RBF_MATERN52>());
    case GSL_SINTERP_RBF_IMQ: return f(ic<GSL_SINTERP_RBF_IMQ>());
    default: return f(ic<GSL_SINTERP_RBF_TPS>());
  }
}

template <class F> static auto with_dim(int dim, F &&f)
{
  switch (dim) {
    case 1: return f(ic<1>());
    case 2: return f(ic<2>());
    default: return f(ic<3>());
  }
}

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
  } else if (KIND == GSL_SINTERP_RBF_MATERN32) {
    /* coef = sqrt(3) eps; (1 + t) e^-t as e + t e: one FMA, exactly 1 at t = 0 (exp2_tbl(-0) = 1) */
    const double t = coef * sqrt(r2), e = exp2_tbl(t * -1.44269504088896340735992, t0);
    return fma(t, e, e);
  } else if (KIND == GSL_SINTERP_RBF_MATERN52) {
    /* coef = sqrt(5) eps; (1 + t + t^2/3) e^-t, the polynomial by Horner */
    const double t = coef * sqrt(r2), e = exp2_tbl(t * -1.44269504088896340735992, t0);
    return fma(t, fma(t, 1.0 / 3.0, 1.0), 1.0) * e;
  } else if (KIND == GSL_SINTERP_RBF_IMQ) {
    /* coef = eps^2; the correctly rounded sqrt and division (no rsq refinement): exactly 1 at r2 = 0 */
    return 1.0 / sqrt(fma(coef, r2, 1.0));
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
       Matern 3/2  psi = -3 eps^2 e^-t              *psi = e^-t                 t = sqrt(3) eps r
       Matern 5/2  psi = -(5 eps^2 / 3) (1 + t) e^-t   *psi = (1 + t) e^-t      t = sqrt(5) eps r
       inv. multiquadric  psi = -eps^2 phi^3        *psi = phi^3
   None of them divides by r and none is singular at r = 0: the thin-plate psi is the finite log_tbl(0) + 1 there, and the
   callers multiply it by y - x = 0.  (The Matern 1/2 kernel exp(-eps r) is absent for this reason: its psi = -eps e^-t / r.) */
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
  } else if (KIND == GSL_SINTERP_RBF_MATERN32) {
    const double t = coef * sqrt(r2), e = exp2_tbl(t * -1.44269504088896340735992, t0);
    *psi = e;
    return fma(t, e, e);
  } else if (KIND == GSL_SINTERP_RBF_MATERN52) {
    const double t = coef * sqrt(r2), e = exp2_tbl(t * -1.44269504088896340735992, t0);
    *psi = fma(t, e, e);
    return fma(t, fma(t, 1.0 / 3.0, 1.0), 1.0) * e;
  } else if (KIND == GSL_SINTERP_RBF_IMQ) {
    const double v = 1.0 / sqrt(fma(coef, r2, 1.0));
    *psi = (v * v) * v;
    return v;
  } else {
    const double L = log_tbl<COPIES>(r2, lt_lane);
    *psi = L + 1.0;
    return (coef * r2) * L;
  }
}

#endif
