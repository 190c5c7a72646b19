/*
 * rbf.hip -- radial-kernel matrix fill and the N x M evaluation sweep.
 *
 * The reference holds no RBF code (README:18-26); SURVEY.md 3.3/3.4 fixes what
 * is computed:  Phi_ij = phi(|x_i - x_j|)  and  s(y_k) = sum_j w_j phi(|y_k - x_j|)
 * with j ascending (one accumulator per target, so the summation order is the
 * CPU oracle's; only exp/log rounding and FMA contraction differ).
 *
 *   fill : HBM-write bound (8 B per entry), 16-byte stores, centres via cache.
 *   eval : fp64-VALU bound (~N x 16 ops per target); centre tiles + weights
 *          staged through LDS and broadcast to the wave, TPT targets per lane
 *          for ILP; exp / log evaluated with 256-entry LDS tables and short
 *          polynomials (<= 2 ulp, far inside the 1e-10 parity tolerance).
 */
#include "common.h"
#include <math.h>
#include <stdlib.h>
#include "rbf_phi.h"

/* (dimension, tile size) of the culled sweeps: cull_tile_size gives 8 / 16 / 32 in two dimensions, 32 otherwise */
template <class F> static auto with_dim_tile(int dim, int ct, F &&f)
{
  switch (dim) {
    case 1: return f(ic<1>(), ic<32>());
    case 2: return ct == 8 ? f(ic<2>(), ic<8>()) : ct == 16 ? f(ic<2>(), ic<16>()) : f(ic<2>(), ic<32>());
    default: return f(ic<3>(), ic<32>());
  }
}

/* developer switch: "1" turns the tile culling (read once per process) off */
static bool no_cull() { return SINTERP_ENV_ONCE("GSL_SINTERP_NO_CULL"); }

struct RbfTables {
  double exp2_frac[TBL_N];      /* 2^(i/256)                          */
  double log_pair[LOG_N][2];    /* {1/c_i, ln c_i}, c_i = (1 + (i+0.5)/LOG_N)/2 */
};

__device__ RbfTables g_rbf_tables;
static bool g_tables_ready[64] = {false};

static int ensure_tables(gsl_sinterp_hip_ctx *ctx)
{
  if (ctx->device < 64 && g_tables_ready[ctx->device]) return ST_SUCCESS;
  static RbfTables h;
  for (int i = 0; i < TBL_N; i++) h.exp2_frac[i] = exp2((double)i / TBL_N);
  for (int i = 0; i < LOG_N; i++) {
    double c = 0.5 * (1.0 + ((double)i + 0.5) / LOG_N);   /* bin midpoint of the frexp mantissa in [1/2, 1) */
    h.log_pair[i][0] = 1.0 / c;
    h.log_pair[i][1] = log(c);
  }
  HIP_OK(ctx, hipMemcpyToSymbol(HIP_SYMBOL(g_rbf_tables), &h, sizeof h, 0, hipMemcpyHostToDevice));
  if (ctx->device < 64) g_tables_ready[ctx->device] = true;
  return ST_SUCCESS;
}

/* device address of the exp2 table (built on first use), for kernels of other translation units that evaluate
   phi through rbf_phi.h */
int sinterp_rbf_exp2_table(gsl_sinterp_hip_ctx *ctx, const double **d_tbl)
{
  int st = ensure_tables(ctx);
  if (st) return st;
  void *p = NULL;
  HIP_OK(ctx, hipGetSymbolAddress(&p, HIP_SYMBOL(g_rbf_tables)));
  *d_tbl = (const double *)p;                     /* exp2_frac is the first member */
  return ST_SUCCESS;
}

template <int COPIES>
__device__ __forceinline__ void load_tables(double *s_t0, double *s_lt, int kind)
{
  if (kind_uses_exp2(kind)) {
    for (int i = threadIdx.x; i < TBL_N; i += blockDim.x) s_t0[i] = g_rbf_tables.exp2_frac[i];
  } else if (kind_uses_log(kind)) {
    /* eight loads in flight: one at a time, the 16 trips of the replicated table are 16 global round trips (~25 us) per workgroup */
#pragma unroll 8
    for (int i = threadIdx.x; i < LOG_N * COPIES * 2; i += blockDim.x) s_lt[i] = g_rbf_tables.log_pair[i / (COPIES * 2)][i & 1];
  }
}

/* ------------------------------------------------------------------------ */
/* fill: block = 256 threads -> 16 rows x 128 cols, 2 columns (16 B) per lane */
/* SHIFT (thin-plate spline, round 4): the entry leaves as Phi_ij + s sum_a P_a[i] P_a[j] with s = cmul |Phi|_inf / n read from
   norm_bits (tps_rownorm_kernel) -- the shifted SPD matrix of solve.hip in ONE pass over HBM; until round 3 the plain fill was
   followed by a read of the whole matrix for its norm and a read-modify-write for the shift (61 + 61 us at N = 4096). */
template <int KIND, int DIM, bool SHIFT = false>
__global__ void __launch_bounds__(256)
rbf_fill_kernel(double coef, const double *__restrict__ x, size_t n, size_t xtda, double *__restrict__ phi, size_t lda, int lower_only,
                const double *__restrict__ Pk = nullptr, int pk = 0, double cmul = 0.0, const unsigned long long *__restrict__ norm_bits = nullptr)
{
  /* lower_only: tiles that lie entirely above the diagonal are not written (the Cholesky route reads the lower
     triangle only; half of the HBM writes of the fill) */
  if (lower_only && (size_t)blockIdx.x * 128 > (size_t)blockIdx.y * 16 + 15) return;
  __shared__ double s_t0[kind_uses_exp2(KIND) ? TBL_N : 1];
  __shared__ __attribute__((aligned(16))) double s_lt[kind_uses_log(KIND) ? LOG_N * 2 : 2];   /* one copy: the fill is HBM-write bound */
  load_tables<1>(s_t0, s_lt, KIND);
  const double *lt_lane = s_lt;
  __syncthreads();
  const size_t j0 = ((size_t)blockIdx.x * 64 + (threadIdx.x & 63)) * 2;
  const size_t ibase = (size_t)blockIdx.y * 16 + (threadIdx.x >> 6) * 4;
  if (j0 >= n) return;
  const bool two = j0 + 1 < n;
  double xa[DIM], xb[DIM];
#pragma unroll
  for (int c = 0; c < DIM; c++) { xa[c] = x[j0 * xtda + c]; xb[c] = two ? x[(j0 + 1) * xtda + c] : 0.0; }
  double pja[4] = {0, 0, 0, 0}, pjb[4] = {0, 0, 0, 0}, pir[4][4] = {{0}}, sh = 0.0;
  if (SHIFT) {
    sh = cmul * __longlong_as_double((long long)*norm_bits) / (double)n;
#pragma unroll
    for (int a = 0; a < 4; a++)
      if (a < pk) { pja[a] = Pk[(size_t)a * n + j0]; pjb[a] = two ? Pk[(size_t)a * n + j0 + 1] : 0.0; }
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
      for (int a = 0; a < 4; a++) pir[r][a] = (a < pk && ibase + r < n) ? Pk[(size_t)a * n + ibase + r] : 0.0;   /* uniform over the wave; all in flight before the rows */
  }
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const size_t i = ibase + r;
    if (i >= n) break;
    double ra = 0.0, rb = 0.0;
#pragma unroll
    for (int c = 0; c < DIM; c++) {
      const double xi = x[i * xtda + c];
      const double da = xi - xa[c], db = xi - xb[c];
      ra = fma(da, da, ra); rb = fma(db, db, rb);
    }
    double va = phi_r2<KIND, 1>(ra, coef, s_t0, lt_lane);
    double vb = phi_r2<KIND, 1>(rb, coef, s_t0, lt_lane);
    if (KIND == GSL_SINTERP_RBF_TPS) { va = ra > 0.0 ? va : 0.0; vb = rb > 0.0 ? vb : 0.0; }   /* phi(0) = 0 exactly in the matrix */
    if (SHIFT) {
      double acca = 0.0, accb = 0.0;
#pragma unroll
      for (int a = 0; a < 4; a++)
        if (a < pk) { acca = fma(pir[r][a], pja[a], acca); accb = fma(pir[r][a], pjb[a], accb); }
      va = fma(sh, acca, va); vb = fma(sh, accb, vb);
    }
    double *dst = phi + i * lda + j0;
    /* non-temporal: 1 GB of matrix is written once and read back by the factorisation long after (C3 init 32.66 -> 32.55 ms) */
    if (two && ((((uintptr_t)dst) & 15) == 0)) { typedef double v2d __attribute__((ext_vector_type(2))); v2d vv = {va, vb}; __builtin_nontemporal_store(vv, reinterpret_cast<v2d *>(dst)); }
    else { dst[0] = va; if (two) dst[1] = vb; }
  }
}

/* A target with a NaN coordinate has r^2 = NaN for every centre: the naive sum (oracle) is NaN.  The
   Gaussian sweeps compare r^2 against the cut-off (false for NaN), so they restore the NaN at the end. */
template <int DIM>
__device__ __forceinline__ bool nan_target(const double (&yy)[DIM])
{
  bool isn = false;
#pragma unroll
  for (int c = 0; c < DIM; c++) isn |= (yy[c] != yy[c]);
  return isn;
}

/* ------------------------------------------------------------------------ */
/* The sweeps:  s(y) = sum_j w_j phi(|y - x_j|)  and, with GRAD,  grad s(y) = sum_j w_j psi(r_j^2) (y - x_j),  psi = phi'(r) / r
   (rbf_phi.h: phi_psi_r2), from ONE pass over the centres -- the exp2 / sqrt / log of a (target, centre) pair and the
   difference y - x_j are shared, the gradient adds one product and DIM FMAs per pair and DIM accumulators per target.
   There is one body per sweep -- rbf_sweep over every centre, rbf_sweep_cull over the tiles near the workgroup -- and
   GRAD only selects the per-pair term and the store (sweep_term, sweep_store); the four __global__ kernels are wrappers.

   Value.  sweep_term keeps acc = fma(w_j, phi, acc) with one take-criterion and one order whatever GRAD is, so the value
   that comes with a gradient has the bits gsl_sinterp_hip_rbf_eval_model returns for the same model and target.

   Take-criterion.  One take[] per (target, centre) pair selects the value term and the gradient term (Gaussian: term above
   2^-72 of the kernel maximum; Wendland: inside the support) -- the gradient too is a function of (model, target) alone,
   bit-reproducible across batch size and grouping.  A dropped Gaussian gradient term is
   |w_j| 2 eps^2 r exp(-(eps r)^2) = |w_j| 2 eps t exp(-t^2) with t = eps r beyond the cut-off t_c = sqrt(72 ln 2) = 7.07, where
   t exp(-t^2) decreases: each is below |w_j| 2 eps t_c 2^-72 < |w_j| 14.2 eps 2^-72, the dropped mass of a component below
   N max|w| 14.2 eps 2^-72 = N max|w| eps 3e-21.

   Non-finite targets.  A NaN coordinate gives NaN in the value and in every gradient component, for every kind.  The
   Gaussian / Wendland comparisons are false for NaN, so sweep_store restores the NaN.  The Matern kinds rely on the same
   restore: exp2_tbl clamps its argument with fmax(t, -1100), which swallows a NaN (the factor 1 + t still carries it into
   phi, but psi of Matern 3/2 is the bare exponential); the inverse multiquadric carries the NaN through sqrt and is
   restored all the same.  An infinite coordinate of a Matern target meets inf * 0: not pinned.  The thin-plate value needs nothing:
   r^2 = NaN goes through log_tbl into every term, and only the gradient is set.  An infinite coordinate of a Gaussian /
   Wendland target fails the criterion for every centre: no term is taken, value and gradient are 0 (terms are SELECTED,
   never multiplied by 0, so inf - x_j does no harm).

   Fields.  A third mode of the same two bodies (NF > 1 weights per staged centre, FLD): K weight vectors on the same centres,
   NF accumulators per target, phi and take still computed once per pair.  Field q has the bits of the value sweep run on
   column q: the same terms, order, take-criterion and kernel choice (rbf_sweep_dispatch); NF = 1 is the code of the two
   modes above, instruction for instruction.

   Target order.  The value entry sorts large batches with the two-level reorder and stores through its map (omap); the
   gradient entry takes the one-level permutation route (sinterp_sort_targets; the kernels read and write through perm)
   whatever the batch size: the two-level reorder's result path carries one scalar per target. */

/* one (target, centre) pair: d = y - x_j, r2 = |d|^2, wj the centre's NF weights (one per field of the block; NF = 1 in
   the value and value + gradient modes); the terms are added only when take is set.  phi and take are computed once per
   pair: a further field costs its FMA and its select */
template <int KIND, int DIM, bool GRAD, int NF>
__device__ __forceinline__ void sweep_term(double r2, const double (&d)[DIM], const double (&wj)[NF], double coef, bool take,
                                           const double *s_t0, const double *lt_lane, double (&acc)[NF], double (&gacc)[DIM])
{
  if constexpr (GRAD) {
    static_assert(NF == 1, "the gradient sweep carries one field");
    double psi;
    const double ph = phi_psi_r2<KIND, LOG_COPIES>(r2, coef, s_t0, lt_lane, &psi);
    const double a = fma(wj[0], ph, acc[0]);
    const double p = wj[0] * psi;                /* a product of its own: the value's FMA is untouched */
    acc[0] = take ? a : acc[0];
#pragma unroll
    for (int c = 0; c < DIM; c++) { const double ga = fma(p, d[c], gacc[c]); gacc[c] = take ? ga : gacc[c]; }
  } else {
    const double ph = phi_r2<KIND, LOG_COPIES>(r2, coef, s_t0, lt_lane);
#pragma unroll
    for (int q = 0; q < NF; q++) { const double a = fma(wj[q], ph, acc[q]); acc[q] = take ? a : acc[q]; }
  }
}

/* The fields mode of the two sweeps (FLD): K weight vectors on the same centres, NF of them per pass.  w (plain sweep)
   points at the first column of the pass, column q at w + q * ldw; xs (culled sweep) holds {x, w_0 .. w_{K-1}} records of
   rs = DIM + K doubles and q0 is the first field of the pass; s points at the pass's first output column, target k's
   field q at s[k * stda + q].  nfa <= NF fields are live: a ragged last block neither reads a weight nor writes a result
   beyond them (the idle accumulators run on zero weights). */
struct sweep_fields {
  size_t ldw, stda;
  int nfa, q0, rs;
};

/* value sweep: s through omap when given.  GRAD: s may be NULL (gradient only); row k of g = g + k * gtda, DIM entries
   written, the constant of psi (rbf_grad_scale) applied here, once per target */
template <int KIND, int DIM, int TPT, bool GRAD, int NF, bool FLD>
__device__ __forceinline__ void sweep_store(const size_t (&kidx)[TPT], size_t m, const double (&yy)[TPT][DIM], const double (&acc)[TPT][NF],
                                            const double (&gacc)[TPT][DIM], double *__restrict__ s, const unsigned *__restrict__ omap,
                                            double *__restrict__ g, size_t gtda, double gscale, const sweep_fields &F)
{
#pragma unroll
  for (int t = 0; t < TPT; t++) {
    if (kidx[t] >= m) continue;
    const bool isn = nan_target<DIM>(yy[t]);
    if constexpr (FLD) {                         /* the NaN rule holds for every field of the row */
#pragma unroll
      for (int q = 0; q < NF; q++)
        if (q < F.nfa) s[kidx[t] * F.stda + q] = (KIND != GSL_SINTERP_RBF_TPS && isn) ? NAN : acc[t][q];
      continue;
    }
    const double v = (KIND != GSL_SINTERP_RBF_TPS && isn) ? NAN : acc[t][0];
    if constexpr (GRAD) {
      if (s) s[kidx[t]] = v;
#pragma unroll
      for (int c = 0; c < DIM; c++) g[kidx[t] * gtda + c] = isn ? NAN : gscale * gacc[t][c];
    } else {
      s[omap ? (size_t)omap[kidx[t]] : kidx[t]] = v;
    }
  }
}

/* sweep over every centre: TPT targets per lane, centre tile of TJ entries in LDS */
#define EV_THREADS 256
#define EV_TJ 512

template <int KIND, int DIM, int TPT, bool GRAD, int NF = 1, bool FLD = false, int TJ = EV_TJ>
__device__ __forceinline__ void rbf_sweep(double coef, const double *__restrict__ x, size_t n, size_t xtda, const double *__restrict__ w,
                                          const double *__restrict__ y, size_t m, size_t ytda, const int *__restrict__ perm,
                                          double *__restrict__ s, const unsigned *__restrict__ omap, double *__restrict__ g, size_t gtda,
                                          double gscale, const sweep_fields F = sweep_fields())
{
  static_assert(FLD || NF == 1, "several weights per centre: the fields mode");
  constexpr int REC = DIM + NF;
  __shared__ double s_t0[kind_uses_exp2(KIND) ? TBL_N : 1];
  __shared__ __attribute__((aligned(16))) double s_lt[kind_uses_log(KIND) ? LOG_LDS : 2];
  __shared__ double s_c[TJ * REC];                /* per centre: x[0..DIM-1], w[0..NF-1] */
  load_tables<LOG_COPIES>(s_t0, s_lt, KIND);
  const double *lt_lane = s_lt + (threadIdx.x & (LOG_COPIES - 1)) * 2;

  /* slot i of the (optionally cell-sorted) order -> target index; a lane's TPT targets are
     ADJACENT slots so they are spatial neighbours too */
  const size_t k0 = (((size_t)blockIdx.x * EV_THREADS) + threadIdx.x) * TPT;
  size_t kidx[TPT];
  double yy[TPT][DIM], acc[TPT][NF], gacc[TPT][DIM];
#pragma unroll
  for (int t = 0; t < TPT; t++) {
    const size_t slot = k0 + (size_t)t;
    kidx[t] = slot < m ? (perm ? (size_t)perm[slot] : slot) : m;
#pragma unroll
    for (int q = 0; q < NF; q++) acc[t][q] = 0.0;
#pragma unroll
    for (int c = 0; c < DIM; c++) { yy[t][c] = kidx[t] < m ? y[kidx[t] * ytda + c] : 0.0; gacc[t][c] = 0.0; }
  }

  for (size_t jt = 0; jt < n; jt += TJ) {
    const int cnt = (int)((n - jt) < (size_t)TJ ? (n - jt) : (size_t)TJ);
    __syncthreads();
    for (int e = threadIdx.x; e < cnt; e += EV_THREADS) {
#pragma unroll
      for (int c = 0; c < DIM; c++) s_c[e * REC + c] = x[(jt + e) * xtda + c];
      if constexpr (FLD) {
#pragma unroll
        for (int q = 0; q < NF; q++)
          s_c[e * REC + DIM + q] = q < F.nfa ? (KIND == GSL_SINTERP_RBF_TPS ? 0.5 : 1.0) * w[(size_t)q * F.ldw + jt + e] : 0.0;
      } else {
        s_c[e * REC + DIM] = (KIND == GSL_SINTERP_RBF_TPS ? 0.5 : 1.0) * w[jt + e];
      }
    }
    __syncthreads();
#pragma unroll 2
    for (int e = 0; e < cnt; e++) {
      double xc[DIM], wj[NF];
#pragma unroll
      for (int c = 0; c < DIM; c++) xc[c] = s_c[e * REC + c];
#pragma unroll
      for (int q = 0; q < NF; q++) wj[q] = s_c[e * REC + DIM + q];
      double d[TPT][DIM], r2[TPT];
#pragma unroll
      for (int t = 0; t < TPT; t++) {
        r2[t] = 0.0;
#pragma unroll
        for (int c = 0; c < DIM; c++) { d[t][c] = yy[t][c] - xc[c]; r2[t] = fma(d[t][c], d[t][c], r2[t]); }
      }
      bool take[TPT];
#pragma unroll
      for (int t = 0; t < TPT; t++) take[t] = true;          /* thin-plate, Matern, inverse multiquadric: every term */
      if (KIND == GSL_SINTERP_RBF_GAUSSIAN) {
        /* Every distance is computed; a target takes a term only when it is above 2^-72 of the
           kernel's maximum -- a function of the (target, centre) pair alone, so the value does not
           depend on which targets share the wave (bit-reproducible whatever the target order).
           The exponential is skipped when NO lane of the wave takes the term (wave-uniform branch).
           Dropped terms are < 2^-72 |w_j| each, i.e. a relative error <= N max|w| 2.1e-22 on O(1)
           values -- ten orders below the 1e-10 parity tolerance (tests/test_gpu_rbf.py). */
        bool need = false;
#pragma unroll
        for (int t = 0; t < TPT; t++) { take[t] = r2[t] * coef > -72.0; need |= take[t]; }
        if (__builtin_amdgcn_ballot_w64(need) == 0) continue;
      }
      if (KIND == GSL_SINTERP_RBF_WENDLAND) {
        /* outside the support the term is exactly 0: skipping it changes nothing (wave-uniform skip of the sqrt) */
        bool need = false;
#pragma unroll
        for (int t = 0; t < TPT; t++) { take[t] = r2[t] * (coef * coef) < 1.0; need |= take[t]; }
        if (__builtin_amdgcn_ballot_w64(need) == 0) continue;
      }
#pragma unroll
      for (int t = 0; t < TPT; t++)
        sweep_term<KIND, DIM, GRAD, NF>(r2[t], d[t], wj, KIND == GSL_SINTERP_RBF_TPS ? 1.0 : coef, take[t], s_t0, lt_lane, acc[t], gacc[t]);
    }
  }
  sweep_store<KIND, DIM, TPT, GRAD, NF, FLD>(kidx, m, yy, acc, gacc, s, omap, g, gtda, gscale, F);
}

template <int KIND, int DIM, int TPT>
__global__ void __launch_bounds__(EV_THREADS)
rbf_eval_kernel(double coef, const double *__restrict__ x, size_t n, size_t xtda, const double *__restrict__ w,
                const double *__restrict__ y, size_t m, size_t ytda, double *__restrict__ s, const int *__restrict__ perm,
                const unsigned *__restrict__ omap)
{
  rbf_sweep<KIND, DIM, TPT, false>(coef, x, n, xtda, w, y, m, ytda, perm, s, omap, nullptr, 0, 0.0);
}

template <int KIND, int DIM, int TPT>
__global__ void __launch_bounds__(EV_THREADS)
rbf_grad_kernel(double coef, double gscale, const double *__restrict__ x, size_t n, size_t xtda, const double *__restrict__ w,
                const double *__restrict__ y, size_t m, size_t ytda, double *__restrict__ s, double *__restrict__ g, size_t gtda,
                const int *__restrict__ perm)
{
  rbf_sweep<KIND, DIM, TPT, true>(coef, x, n, xtda, w, y, m, ytda, perm, s, nullptr, g, gtda, gscale);
}

/* Fields: NF accumulators per target, one target per lane (the NF chains give the ILP that the second target buys the
   scalar sweep).  Two block sizes, both measured ("Several fields"): a pass of RBF_NF = 8 fields costs 1.6 scalar
   sweeps, a pass of RBF_NF_SMALL = 4 costs 1.25, so K fields go in passes of 8 while more than 4 are left and the last
   <= 4 in a pass of 4 (fields_pass).  EV_TJ_F: centre records per LDS tile of the plain fields sweep -- 256 keeps the
   thin-plate instances (32 KiB log table beside the tile) at 3 workgroups per CU, 512 leaves 2 and is 9 % slower. */
#ifndef RBF_NF
#define RBF_NF 8
#endif
#ifndef RBF_NF_SMALL
#define RBF_NF_SMALL 4
#endif
#ifndef EV_TJ_F
#define EV_TJ_F 256
#endif
/* fields of the pass that starts with `left` fields to go */
static inline int fields_pass(int left) { return left > RBF_NF_SMALL ? (left < RBF_NF ? left : RBF_NF) : left; }

template <int KIND, int DIM, int NF>
__global__ void __launch_bounds__(EV_THREADS)
rbf_fields_kernel(double coef, const double *__restrict__ x, size_t n, size_t xtda, const double *__restrict__ w, size_t ldw, int nfa,
                  const double *__restrict__ y, size_t m, size_t ytda, double *__restrict__ s, size_t stda, const int *__restrict__ perm)
{
  const sweep_fields F = {ldw, stda, nfa, 0, 0};
  rbf_sweep<KIND, DIM, 1, false, NF, true, EV_TJ_F>(coef, x, n, xtda, w, y, m, ytda, perm, s, nullptr, nullptr, 0, 0.0, F);
}

/* ------------------------------------------------------------------------ */
/* Gaussian sweep with tile culling.  At the shape parameters this path is used with
   (eps ~ 2 N^(1/d)) a target only sees centres within r = sqrt(72 ln 2)/eps of itself -- a few per
   cent of the cloud -- yet the plain sweep still computes every distance.  Here the centres are
   put in Morton cell order (sort.hip), packed as {x, w} and cut into tiles of CT consecutive
   (hence spatially compact) centres with a bounding box each; a workgroup -- whose 512 targets are
   neighbours too, thanks to the target sort -- first collects the tiles whose box comes within
   the cut-off of ITS targets' box (one ballot per 64 tiles, kept as bit masks: ascending order,
   no atomics) and then runs the usual inner loop over those tiles only.  The criterion is the
   one of the per-centre early-out (term < 2^-72 of the kernel maximum), applied to a lower bound
   of the distance, so only terms below that bound are dropped; the summation order is the (fixed)
   Morton order of the centres instead of their input order. */
/* Tile size CT (template parameter: 8, 16 or 32 centres; 128 until round 2).  A target tests every centre of the tiles its
   workgroup keeps; smaller tiles hug the cut-off disc more closely.  Sweep phase, ms -- round 2: C4 (2-D, N = 8192, M = 1e7)
   2.41 / 1.97 / 1.73 / 1.58 and C3 (3-D, N = 16384, M = 1e6) 1.96 / 1.75 / 1.70 / 1.74 for CT = 128 / 64 / 32 / 16; round 3 (targets
   physically reordered by Morton cell, a workgroup = a 2 x 2 block of target cells): C4 1.41 / 1.25 / 1.18 and C3 1.29 / 1.30 / 1.34
   for CT = 32 / 16 / 8; with the kept tiles batched CULL_STAGE centres per LDS stage (one pair of barriers per 64 centres instead
   of per tile): C4 1.25 / 1.19 / 1.18 for CT = 16 / 8 / 4, C3 1.255 / 1.253 / 1.29 for CT = 32 / 16 / 8.  So: 8 in two dimensions,
   32 otherwise -- and the next larger size while the tile count would exceed
   CULL_MAX_TILES (the kept-tile bit mask in LDS).  The tile size changes which centres are TESTED, never which terms a target
   takes nor their order: results are bit-identical for every CT. */
#define CULL_MAX_TILES 8192
#ifndef CULL_STAGE
#define CULL_STAGE 64       /* centres per LDS stage of the culled sweep (a multiple of every tile size) */
#endif
static inline int cull_tile_size(int dim, size_t n)
{
  int ct = dim == 2 ? 8 : 32;
  while (ct < 32 && (n + ct - 1) / ct > CULL_MAX_TILES) ct *= 2;
  return ct;
}

#define CT_THREADS 64
/* FLD: records {x, w_0 .. w_{nf-1}} of DIM + nf doubles, every field's weight packed once (column q of w at w + q * ldw) */
template <int DIM, int CT, bool FLD>
__device__ __forceinline__ void centre_pack(const double *__restrict__ x, size_t n, size_t xtda, const double *__restrict__ w,
                                            const int *__restrict__ perm, double *__restrict__ xs, double *__restrict__ tbox, int nf, size_t ldw)
{
  constexpr int NW = (CT + 63) / 64;
  __shared__ double s_lo[DIM][NW], s_hi[DIM][NW];
  const size_t i = (size_t)blockIdx.x * CT + threadIdx.x;
  const bool ok = threadIdx.x < CT && i < n;
  double v[DIM];
  if (ok) {
    const size_t j = (size_t)perm[i];
    if constexpr (FLD) {
      const size_t rs = (size_t)(DIM + nf);
#pragma unroll
      for (int c = 0; c < DIM; c++) { v[c] = x[j * xtda + c]; xs[i * rs + c] = v[c]; }
      for (int q = 0; q < nf; q++) xs[i * rs + DIM + q] = w[(size_t)q * ldw + j];
    } else {
#pragma unroll
      for (int c = 0; c < DIM; c++) { v[c] = x[j * xtda + c]; xs[i * (DIM + 1) + c] = v[c]; }
      xs[i * (DIM + 1) + DIM] = w[j];
    }
  }
#pragma unroll
  for (int c = 0; c < DIM; c++) {
    double lo = ok ? v[c] : INFINITY, hi = ok ? v[c] : -INFINITY;
    for (int off = 32; off > 0; off >>= 1) { lo = fmin(lo, __shfl_xor(lo, off)); hi = fmax(hi, __shfl_xor(hi, off)); }
    if ((threadIdx.x & 63) == 0) { s_lo[c][threadIdx.x >> 6] = lo; s_hi[c][threadIdx.x >> 6] = hi; }
  }
  __syncthreads();
  if (threadIdx.x < DIM) {
    const int c = threadIdx.x;
    double l = s_lo[c][0], h = s_hi[c][0];
    for (int w = 1; w < NW; w++) { l = fmin(l, s_lo[c][w]); h = fmax(h, s_hi[c][w]); }
    tbox[(size_t)blockIdx.x * (2 * DIM) + 2 * c] = l;
    tbox[(size_t)blockIdx.x * (2 * DIM) + 2 * c + 1] = h;
  }
}

template <int DIM, int CT>
__global__ void __launch_bounds__(CT_THREADS)
centre_pack_kernel(const double *__restrict__ x, size_t n, size_t xtda, const double *__restrict__ w,
                   const int *__restrict__ perm, double *__restrict__ xs, double *__restrict__ tbox)
{
  centre_pack<DIM, CT, false>(x, n, xtda, w, perm, xs, tbox, 1, 0);
}

template <int DIM, int CT>
__global__ void __launch_bounds__(CT_THREADS)
centre_pack_fields_kernel(const double *__restrict__ x, size_t n, size_t xtda, const double *__restrict__ w, size_t ldw, int nf,
                          const int *__restrict__ perm, double *__restrict__ xs, double *__restrict__ tbox)
{
  centre_pack<DIM, CT, true>(x, n, xtda, w, perm, xs, tbox, nf, ldw);
}

#ifdef SINTERP_DIAG_PROF
/* developer build only (make prof): pair counters of the culled sweep -- [0] pair-lanes the kernel evaluated (every lane
   of a wave pays for a centre that ANY of its targets takes), [1] pairs inside the cut-off (the useful ones), [2] centres
   staged in LDS x targets of the workgroup (what survives the tile culling).  tools/gauss_pairs.py reads them. */
__device__ unsigned long long g_cull_stats[4];
extern "C" int gsl_sinterp_hip_debug_cull_stats(unsigned long long *out, int reset)
{
  hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_cull_stats), sizeof(unsigned long long) * 4);
  if (e == hipSuccess && reset) { unsigned long long z[4] = {0, 0, 0, 0}; e = hipMemcpyToSymbol(HIP_SYMBOL(g_cull_stats), z, sizeof z); }
  return (int)e;
}
#define CULL_STAT(i, v) st_##i += (v)
#else
#define CULL_STAT(i, v) do { } while (0)
#endif

/* KIND = Gaussian: cut-off 2^-72 of the kernel maximum (coef = -eps^2 log2 e); KIND = Wendland: the support
   radius itself (coef = eps), so culling drops terms that are exactly 0 */
#ifndef CULL_THREADS
#define CULL_THREADS 128   /* 256 / 128 / 64 threads: C3 sweep 1.34 / 1.26 / 1.27 ms, C4 1.71 ms throughout */
#endif
template <int KIND, int DIM, int TPT, int CT, bool GRAD, int NF = 1, bool FLD = false>
__device__ __forceinline__ void rbf_sweep_cull(double coef, const double *__restrict__ xs, size_t n, const double *__restrict__ tbox,
                                               unsigned ntiles, const double *__restrict__ y, size_t m, size_t ytda,
                                               const int *__restrict__ perm, double *__restrict__ s, const unsigned *__restrict__ omap,
                                               double *__restrict__ g, size_t gtda, double gscale, const sweep_fields F = sweep_fields())
{
  static_assert(FLD || NF == 1, "several weights per centre: the fields mode");
  constexpr int REC = DIM + NF;
  __shared__ double s_t0[TBL_N];
  __shared__ __attribute__((aligned(16))) double s_c[CULL_STAGE * REC];
  constexpr int NWV = CULL_THREADS / 64;
  __shared__ double s_blo[DIM][NWV], s_bhi[DIM][NWV];
  __shared__ unsigned long long s_mask[CULL_MAX_TILES / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < TBL_N; i += CULL_THREADS) s_t0[i] = g_rbf_tables.exp2_frac[i];

  const size_t k0 = (((size_t)blockIdx.x * CULL_THREADS) + tid) * TPT;
  size_t kidx[TPT];
  double yy[TPT][DIM], acc[TPT][NF], gacc[TPT][DIM];
#pragma unroll
  for (int t = 0; t < TPT; t++) {
    const size_t slot = k0 + (size_t)t;
    kidx[t] = slot < m ? (perm ? (size_t)perm[slot] : slot) : m;
#pragma unroll
    for (int q = 0; q < NF; q++) acc[t][q] = 0.0;
#pragma unroll
    for (int c = 0; c < DIM; c++) { yy[t][c] = kidx[t] < m ? y[kidx[t] * ytda + c] : 0.0; gacc[t][c] = 0.0; }
  }
  /* bounding box of this workgroup's targets */
#pragma unroll
  for (int c = 0; c < DIM; c++) {
    double lo = INFINITY, hi = -INFINITY;
#pragma unroll
    for (int t = 0; t < TPT; t++) if (kidx[t] < m) { lo = fmin(lo, yy[t][c]); hi = fmax(hi, yy[t][c]); }
    for (int off = 32; off > 0; off >>= 1) { lo = fmin(lo, __shfl_xor(lo, off)); hi = fmax(hi, __shfl_xor(hi, off)); }
    if (lane == 0) { s_blo[c][wave] = lo; s_bhi[c][wave] = hi; }
  }
  __syncthreads();
  double blo[DIM], bhi[DIM];
#pragma unroll
  for (int c = 0; c < DIM; c++) {
    blo[c] = s_blo[c][0]; bhi[c] = s_bhi[c][0];
#pragma unroll
    for (int w = 1; w < NWV; w++) { blo[c] = fmin(blo[c], s_blo[c][w]); bhi[c] = fmax(bhi[c], s_bhi[c][w]); }
  }
  /* tiles within the cut-off of the box: one bit per tile */
  const unsigned nmask = (ntiles + 63) / 64;
  for (unsigned base = 0; base < ntiles; base += CULL_THREADS) {
    const unsigned t = base + tid;
    bool keep = false;
    if (t < ntiles) {
      double d2 = 0.0;
#pragma unroll
      for (int c = 0; c < DIM; c++) {
        const double tl = tbox[(size_t)t * (2 * DIM) + 2 * c], th = tbox[(size_t)t * (2 * DIM) + 2 * c + 1];
        const double gap = fmax(0.0, fmax(tl - bhi[c], blo[c] - th));
        d2 = fma(gap, gap, d2);
      }
      keep = KIND == GSL_SINTERP_RBF_GAUSSIAN ? d2 * coef > -72.0 : d2 * (coef * coef) < 1.0;
    }
    const unsigned long long b = __builtin_amdgcn_ballot_w64(keep);
    if (lane == 0 && (base / 64 + wave) < nmask) s_mask[base / 64 + wave] = b;
  }
  __syncthreads();

#ifdef SINTERP_DIAG_PROF
  unsigned long long st_0 = 0, st_1 = 0, st_2 = 0;       /* counted by every culled sweep, with or without the gradient */
#endif
  /* the kept tiles, ascending, CULL_STAGE centres per LDS stage (several small tiles share one pair of barriers) */
  unsigned mi = 0;
  unsigned long long mask = nmask ? s_mask[0] : 0ULL;
  for (;;) {
    int cnt = 0;
    __syncthreads();                                       /* the previous stage has been consumed */
    while (cnt + CT <= CULL_STAGE) {
      while (!mask && mi + 1 < nmask) mask = s_mask[++mi];
      if (!mask) break;
      const unsigned t = mi * 64 + (unsigned)__builtin_ctzll(mask);
      mask &= mask - 1;
      const size_t c0 = (size_t)t * CT;
      const int tc = (int)((n - c0) < (size_t)CT ? (n - c0) : (size_t)CT);
      if constexpr (FLD) {
        /* the pass's NF weights out of the record's K: entry e = (centre r, word c) of the staged tile */
        for (int e = tid; e < tc * REC; e += CULL_THREADS) {
          const int r = e / REC, c = e - r * REC;
          const double *rec = xs + (c0 + (size_t)r) * (size_t)F.rs;
          s_c[cnt * REC + e] = c < DIM ? rec[c] : (c - DIM < F.nfa ? rec[DIM + F.q0 + (c - DIM)] : 0.0);
        }
      } else {
        for (int e = tid; e < tc * (DIM + 1); e += CULL_THREADS) s_c[cnt * (DIM + 1) + e] = xs[c0 * (DIM + 1) + e];
      }
      cnt += tc;
    }
    if (cnt == 0) break;
    __syncthreads();
#pragma unroll 2
    for (int e = 0; e < cnt; e++) {
      double xc[DIM], wj[NF];
#pragma unroll
      for (int c = 0; c < DIM; c++) xc[c] = s_c[e * REC + c];
#pragma unroll
      for (int q = 0; q < NF; q++) wj[q] = s_c[e * REC + DIM + q];
      double d[TPT][DIM], r2[TPT];
      bool take[TPT], need = false;
#pragma unroll
      for (int tt = 0; tt < TPT; tt++) {
        r2[tt] = 0.0;
#pragma unroll
        for (int c = 0; c < DIM; c++) { d[tt][c] = yy[tt][c] - xc[c]; r2[tt] = fma(d[tt][c], d[tt][c], r2[tt]); }
        take[tt] = KIND == GSL_SINTERP_RBF_GAUSSIAN ? r2[tt] * coef > -72.0 : r2[tt] * (coef * coef) < 1.0;
        need |= take[tt];
      }
      CULL_STAT(2, TPT);
      if (__builtin_amdgcn_ballot_w64(need) == 0) continue;
      CULL_STAT(0, TPT);
#pragma unroll
      for (int tt = 0; tt < TPT; tt++) CULL_STAT(1, take[tt] ? 1 : 0);
      /* per-target criterion (see rbf_sweep): a culled tile holds only centres every target of
         the workgroup would reject, so the value is the sum over the centres with term > 2^-72, in
         Morton order -- independent of the workgroup / wave the target landed in */
#pragma unroll
      for (int tt = 0; tt < TPT; tt++)
        sweep_term<KIND, DIM, GRAD, NF>(r2[tt], d[tt], wj, coef, take[tt], s_t0, (const double *)NULL, acc[tt], gacc[tt]);
    }
  }
  sweep_store<KIND, DIM, TPT, GRAD, NF, FLD>(kidx, m, yy, acc, gacc, s, omap, g, gtda, gscale, F);
#ifdef SINTERP_DIAG_PROF
  for (int off = 32; off > 0; off >>= 1) { st_0 += __shfl_xor(st_0, off); st_1 += __shfl_xor(st_1, off); st_2 += __shfl_xor(st_2, off); }
  if (lane == 0) { atomicAdd(&g_cull_stats[0], st_0); atomicAdd(&g_cull_stats[1], st_1); atomicAdd(&g_cull_stats[2], st_2); }
#endif
}

template <int KIND, int DIM, int TPT, int CT>
__global__ void __launch_bounds__(CULL_THREADS)
rbf_eval_gauss_cull_kernel(double coef, const double *__restrict__ xs, size_t n, const double *__restrict__ tbox, unsigned ntiles,
                           const double *__restrict__ y, size_t m, size_t ytda, double *__restrict__ s, const int *__restrict__ perm,
                const unsigned *__restrict__ omap)
{
  rbf_sweep_cull<KIND, DIM, TPT, CT, false>(coef, xs, n, tbox, ntiles, y, m, ytda, perm, s, omap, nullptr, 0, 0.0);
}

template <int KIND, int DIM, int TPT, int CT>
__global__ void __launch_bounds__(CULL_THREADS)
rbf_grad_cull_kernel(double coef, double gscale, const double *__restrict__ xs, size_t n, const double *__restrict__ tbox, unsigned ntiles,
                     const double *__restrict__ y, size_t m, size_t ytda, double *__restrict__ s, double *__restrict__ g, size_t gtda,
                     const int *__restrict__ perm)
{
  rbf_sweep_cull<KIND, DIM, TPT, CT, true>(coef, xs, n, tbox, ntiles, y, m, ytda, perm, s, nullptr, g, gtda, gscale);
}

template <int KIND, int DIM, int CT, int NF>
__global__ void __launch_bounds__(CULL_THREADS)
rbf_fields_cull_kernel(double coef, const double *__restrict__ xs, int rs, int q0, int nfa, size_t n, const double *__restrict__ tbox,
                       unsigned ntiles, const double *__restrict__ y, size_t m, size_t ytda, double *__restrict__ s, size_t stda,
                       const int *__restrict__ perm)
{
  const sweep_fields F = {0, stda, nfa, q0, rs};
  rbf_sweep_cull<KIND, DIM, 1, CT, false, NF, true>(coef, xs, n, tbox, ntiles, y, m, ytda, perm, s, nullptr, nullptr, 0, 0.0, F);
}

/* The packed centres of the culled sweeps: Morton order, {x, w} records, one bounding box per tile of ct centres.  They
   depend on the model only: reused when the caller vouches for the model (model_id != 0), whichever culled sweep -- value
   or value + gradient -- packed them. */
struct cull_model {
  const double *xs, *tbox;
  unsigned ntiles;
  int ct;
};

/* nf = 0: the scalar records {x, w} in the context's first slot.  nf >= 1: the fields records {x, w_0 .. w_{nf-1}} in a
   slot of their own, keyed by nf and ldw too -- a fields model and its field 0 used as a scalar model share id, d_x and
   d_w, and each of the two is packed once per model id whatever the order of the calls. */
static int cull_pack(gsl_sinterp_hip_ctx *ctx, int kind, const double *d_x, size_t n, int dim, size_t xtda, const double *d_w,
                     unsigned long long model_id, cull_model *out, int nf = 0, size_t ldw = 0)
{
  gsl_sinterp_hip_ctx::CentKey &key = nf ? ctx->cent_key_f : ctx->cent_key;
  const bool cached = model_id != 0 && key.id == model_id && key.x == d_x && key.w == d_w && key.n == n && key.xtda == xtda &&
                      key.dim == dim && key.kind == kind && key.nf == nf && key.ldw == ldw;
  int *d_cperm = NULL;
  int st = ST_SUCCESS;
  if (!cached) {
    key.id = 0;
    st = sinterp_sort_centres(ctx, d_x, n, xtda, dim, 8, &d_cperm);
    if (st) return st;
  }
  const int ct = cull_tile_size(dim, n);
  const unsigned ntiles = (unsigned)((n + ct - 1) / ct);
  const size_t rec = (size_t)(dim + (nf ? nf : 1)), bytes = (n * rec + (size_t)ntiles * 2 * dim) * sizeof(double);
  void *buf = NULL;
  st = nf ? sinterp_centbuf_fields(ctx, bytes, &buf) : sinterp_centbuf(ctx, bytes, &buf);
  if (st) return st;
  double *xs = (double *)buf, *tbox = xs + n * rec;
  out->xs = xs; out->tbox = tbox; out->ntiles = ntiles; out->ct = ct;
  if (cached) return ST_SUCCESS;
  with_dim_tile(dim, ct, [&](auto D, auto C) {
    if (nf)
      hipLaunchKernelGGL((centre_pack_fields_kernel<decltype(D)::value, decltype(C)::value>), dim3(ntiles), dim3(CT_THREADS), 0, ctx->stream,
                         d_x, n, xtda, d_w, ldw, nf, (const int *)d_cperm, xs, tbox);
    else
      hipLaunchKernelGGL((centre_pack_kernel<decltype(D)::value, decltype(C)::value>), dim3(ntiles), dim3(CT_THREADS), 0, ctx->stream,
                         d_x, n, xtda, d_w, (const int *)d_cperm, xs, tbox);
  });
  LAUNCH_CHECK(ctx);
  if (model_id != 0) {
    key.id = model_id; key.x = d_x; key.w = d_w; key.n = n; key.xtda = xtda; key.ldw = ldw; key.dim = dim; key.kind = kind; key.nf = nf;
  }
  return ST_SUCCESS;
}

/* ------------------------------------------------------------------------ */
/* the constant of psi (rbf_phi.h), applied once per target by sweep_store */
static double rbf_grad_scale(int kind, double eps)
{
  switch (kind) {
    case GSL_SINTERP_RBF_GAUSSIAN: return -2.0 * (eps * eps);
    case GSL_SINTERP_RBF_WENDLAND: return -20.0 * (eps * eps);
    case GSL_SINTERP_RBF_MATERN32: return -3.0 * (eps * eps);
    case GSL_SINTERP_RBF_MATERN52: return -(5.0 / 3.0) * (eps * eps);
    case GSL_SINTERP_RBF_IMQ: return -(eps * eps);
    default: return 2.0;                                                  /* thin-plate: the centre tile holds w / 2 */
  }
}

static bool known_kind(int kind) { return kind_is_known(kind); }

template <int KIND>
static int launch_fill(gsl_sinterp_hip_ctx *ctx, double coef, const double *d_x, size_t n, int dim, size_t xtda,
                       double *d_phi, size_t lda, int lower_only)
{
  dim3 grid((unsigned)((n + 127) / 128), (unsigned)((n + 15) / 16));
  with_dim(dim, [&](auto D) {
    hipLaunchKernelGGL((rbf_fill_kernel<KIND, decltype(D)::value>), grid, dim3(256), 0, ctx->stream, coef, d_x, n, xtda, d_phi, lda, lower_only);
  });
  LAUNCH_CHECK(ctx);
  return ST_SUCCESS;
}

#define TN_R 2   /* rows per wave: 8 per workgroup, n / 8 workgroups (16 rows per workgroup left one wave per SIMD: 76 us at N = 4096) */
/* |Phi|_inf = max_i sum_j |phi(|x_i - x_j|)| from the coordinates (nothing of the matrix is read): TN_R rows per wave, a
   wave's lanes stride over the columns, fixed summation order (lane partial sums, then the butterfly) -> reproducible */
template <int DIM>
__global__ void __launch_bounds__(256)
tps_rownorm_kernel(double coef, const double *__restrict__ x, size_t n, size_t xtda, unsigned long long *__restrict__ out)
{
  __shared__ double s_t0[1];
  __shared__ __attribute__((aligned(16))) double s_lt[LOG_LDS];        /* the sweep's replicated table: this kernel is VALU / LDS bound */
  load_tables<LOG_COPIES>(s_t0, s_lt, GSL_SINTERP_RBF_TPS);
  const double *lt_lane = s_lt + (threadIdx.x & (LOG_COPIES - 1)) * 2;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const size_t ibase = (size_t)blockIdx.x * (4 * TN_R) + (threadIdx.x >> 6) * TN_R;
  double xi[TN_R][DIM], acc[TN_R];
#pragma unroll
  for (int r = 0; r < TN_R; r++) {
    acc[r] = 0.0;
#pragma unroll
    for (int c = 0; c < DIM; c++) xi[r][c] = ibase + r < n ? x[(ibase + r) * xtda + c] : 0.0;
  }
#pragma unroll 8
  for (size_t j = lane; j < n; j += 64) {          /* eight columns' coordinates in flight (one at a time: a load latency per step) */
    double xj[DIM];
#pragma unroll
    for (int c = 0; c < DIM; c++) xj[c] = x[j * xtda + c];
#pragma unroll
    for (int r = 0; r < TN_R; r++) {
      double r2 = 0.0;
#pragma unroll
      for (int c = 0; c < DIM; c++) { const double d = xi[r][c] - xj[c]; r2 = fma(d, d, r2); }
      const double v = phi_r2<GSL_SINTERP_RBF_TPS, LOG_COPIES>(r2, coef, s_t0, lt_lane);
      acc[r] += r2 > 0.0 ? fabs(v) : 0.0;
    }
  }
#pragma unroll
  for (int r = 0; r < TN_R; r++) {
    double a = acc[r];
    for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off);
    if (lane == 0 && ibase + r < n) atomicMax(out, (unsigned long long)__double_as_longlong(a));   /* a >= 0: bit order == value order */
  }
}

/* thin-plate spline matrix with the shift of the SPD route applied in flight (both triangles): d_norm receives the bit
   pattern of |Phi|_inf, Pk = k standardised polynomial columns of length n */
int sinterp_tps_fill_shifted(gsl_sinterp_hip_ctx *ctx, const double *d_x, size_t n, int dim, size_t xtda, double *d_phi, size_t lda,
                             const double *d_Pk, int k, double cmul, unsigned long long *d_norm)
{
  REQUIRE(ctx, dim >= 1 && dim <= 3 && xtda >= (size_t)dim && lda >= n && (n + 15) / 16 <= 65535, ST_EINVAL);
  int st = ensure_tables(ctx);
  if (st) return st;
  const double coef = kernel_coef(GSL_SINTERP_RBF_TPS, 0.0);
  HIP_OK(ctx, hipMemsetAsync(d_norm, 0, sizeof(unsigned long long), ctx->stream));
  const dim3 ngrid((unsigned)((n + 4 * TN_R - 1) / (4 * TN_R))), grid((unsigned)((n + 127) / 128), (unsigned)((n + 15) / 16));
  with_dim(dim, [&](auto D) {
    constexpr int DIM = decltype(D)::value;
    hipLaunchKernelGGL(tps_rownorm_kernel<DIM>, ngrid, dim3(256), 0, ctx->stream, coef, d_x, n, xtda, d_norm);
    hipLaunchKernelGGL((rbf_fill_kernel<GSL_SINTERP_RBF_TPS, DIM, true>), grid, dim3(256), 0, ctx->stream, coef, d_x, n, xtda, d_phi, lda, 0,
                       d_Pk, k, cmul, (const unsigned long long *)d_norm);
  });
  LAUNCH_CHECK(ctx);
  return ST_SUCCESS;
}

extern "C" int gsl_sinterp_hip_rbf_fill(gsl_sinterp_hip_ctx *ctx, int kind, double eps, const double *d_x, size_t n,
                                        int dim, size_t xtda, double *d_phi, size_t lda)
{
  return sinterp_rbf_fill_ex(ctx, kind, eps, d_x, n, dim, xtda, d_phi, lda, 0);
}

int sinterp_rbf_fill_ex(gsl_sinterp_hip_ctx *ctx, int kind, double eps, const double *d_x, size_t n, int dim, size_t xtda,
                        double *d_phi, size_t lda, int lower_only)
{
  REQUIRE(ctx, ctx != NULL, ST_EFAULT);
  HIP_OK(ctx, hipSetDevice(ctx->device));      /* one context per device: bind before any launch */
  REQUIRE(ctx, dim >= 1 && dim <= 3 && xtda >= (size_t)dim && lda >= n, ST_EINVAL);
  REQUIRE(ctx, known_kind(kind), ST_EINVAL);
  REQUIRE(ctx, n == 0 || (d_x && d_phi), ST_EFAULT);
  REQUIRE(ctx, (n + 15) / 16 <= 65535, ST_EINVAL);
  if (n == 0) return ST_SUCCESS;
  int st = ensure_tables(ctx);
  if (st) return st;
  const double coef = kernel_coef(kind, eps);
  return with_kind(kind, [&](auto K) { return launch_fill<decltype(K)::value>(ctx, coef, d_x, n, dim, xtda, d_phi, lda, lower_only); });
}

/* ------------------------------------------------------------------------ */
/* One sweep as the host sees it: the model, the targets (read through perm when given) and where the results go.
   g == NULL: the value sweep, s stored through omap when given; else value + gradient, s may be NULL. */
struct sweep_job {
  double coef;
  const double *x; size_t n; int dim; size_t xtda; const double *w;
  const double *y; size_t m, ytda; const int *perm;
  double *s; const unsigned *omap;
  double *g; size_t gtda; double gscale;
  unsigned long long model_id;
  int nf; size_t ldw, stda;          /* nf >= 1: the fields sweep -- column q of w at w + q * ldw, target k's field q at s[k * stda + q] */
};

template <int KIND, int TPT>
static int launch_sweep(gsl_sinterp_hip_ctx *ctx, const sweep_job &j)
{
  const size_t per_block = (size_t)EV_THREADS * TPT;
  const dim3 grid((unsigned)((j.m + per_block - 1) / per_block)), block(EV_THREADS);
  with_dim(j.dim, [&](auto D) {
    constexpr int DIM = decltype(D)::value;
    if constexpr (TPT == 1) {
      if (j.nf) {                                 /* passes of RBF_NF fields, the last <= RBF_NF_SMALL in the small instance */
        for (int q0 = 0, nfa; q0 < j.nf; q0 += nfa) {
          nfa = fields_pass(j.nf - q0);
          if (nfa > RBF_NF_SMALL)
            hipLaunchKernelGGL((rbf_fields_kernel<KIND, DIM, RBF_NF>), grid, block, 0, ctx->stream, j.coef, j.x, j.n, j.xtda,
                               j.w + (size_t)q0 * j.ldw, j.ldw, nfa, j.y, j.m, j.ytda, j.s + q0, j.stda, j.perm);
          else
            hipLaunchKernelGGL((rbf_fields_kernel<KIND, DIM, RBF_NF_SMALL>), grid, block, 0, ctx->stream, j.coef, j.x, j.n, j.xtda,
                               j.w + (size_t)q0 * j.ldw, j.ldw, nfa, j.y, j.m, j.ytda, j.s + q0, j.stda, j.perm);
        }
        return;
      }
    }
    if (j.g)
      hipLaunchKernelGGL((rbf_grad_kernel<KIND, DIM, TPT>), grid, block, 0, ctx->stream, j.coef, j.gscale, j.x, j.n, j.xtda, j.w, j.y, j.m,
                         j.ytda, j.s, j.g, j.gtda, j.perm);
    else
      hipLaunchKernelGGL((rbf_eval_kernel<KIND, DIM, TPT>), grid, block, 0, ctx->stream, j.coef, j.x, j.n, j.xtda, j.w, j.y, j.m, j.ytda,
                         j.s, j.perm, j.omap);
  });
  LAUNCH_CHECK(ctx);
  return ST_SUCCESS;
}

template <int KIND, int TPT>
static int launch_sweep_cull(gsl_sinterp_hip_ctx *ctx, const sweep_job &j)
{
  cull_model cm;
  int st = cull_pack(ctx, KIND, j.x, j.n, j.dim, j.xtda, j.w, j.model_id, &cm, j.nf, j.ldw);
  if (st) return st;
  const size_t per_block = (size_t)CULL_THREADS * TPT;
  const dim3 grid((unsigned)((j.m + per_block - 1) / per_block)), block(CULL_THREADS);
  with_dim_tile(j.dim, cm.ct, [&](auto D, auto C) {
    constexpr int DIM = decltype(D)::value, CT = decltype(C)::value;
    if constexpr (TPT == 1) {
      if (j.nf) {
        for (int q0 = 0, nfa; q0 < j.nf; q0 += nfa) {
          nfa = fields_pass(j.nf - q0);
          if (nfa > RBF_NF_SMALL)
            hipLaunchKernelGGL((rbf_fields_cull_kernel<KIND, DIM, CT, RBF_NF>), grid, block, 0, ctx->stream, j.coef, cm.xs, j.dim + j.nf, q0,
                               nfa, j.n, cm.tbox, cm.ntiles, j.y, j.m, j.ytda, j.s + q0, j.stda, j.perm);
          else
            hipLaunchKernelGGL((rbf_fields_cull_kernel<KIND, DIM, CT, RBF_NF_SMALL>), grid, block, 0, ctx->stream, j.coef, cm.xs, j.dim + j.nf,
                               q0, nfa, j.n, cm.tbox, cm.ntiles, j.y, j.m, j.ytda, j.s + q0, j.stda, j.perm);
        }
        return;
      }
    }
    if (j.g)
      hipLaunchKernelGGL((rbf_grad_cull_kernel<KIND, DIM, TPT, CT>), grid, block, 0, ctx->stream, j.coef, j.gscale, cm.xs, j.n, cm.tbox,
                         cm.ntiles, j.y, j.m, j.ytda, j.s, j.g, j.gtda, j.perm);
    else
      hipLaunchKernelGGL((rbf_eval_gauss_cull_kernel<KIND, DIM, TPT, CT>), grid, block, 0, ctx->stream, j.coef, cm.xs, j.n, cm.tbox,
                         cm.ntiles, j.y, j.m, j.ytda, j.s, j.perm, j.omap);
  });
  LAUNCH_CHECK(ctx);
  return ST_SUCCESS;
}

/* Which kernel runs, for the value and for the value + gradient entry alike. */
static int rbf_sweep_dispatch(gsl_sinterp_hip_ctx *ctx, int kind, const sweep_job &j)
{
  /* The culled kernel sums in the Morton order of the centres, the plain one in input order.  Which of the two
     runs must not depend on the batch (a target's value is a function of the model and the target alone, so a
     batch split into shards -- or a single-point call -- returns the bits of the one-batch result): it is chosen
     by N only; small batches simply run the culled kernel without the target sort. */
  const bool culled = kind_is_culled(kind) && !no_cull() && j.n >= 1024 && (j.n + 31) / 32 <= CULL_MAX_TILES;
  /* few targets: 1 per lane keeps more CUs busy; many: 2 per lane for ILP.
     Culled, 3-D: one target per lane also for large batches -- a workgroup's 256 targets span half the box of 512, and
     in three dimensions that removes more tested-and-rejected centres than the second accumulator chain gains
     (C3 sweep 1.70 -> 1.34 ms; 2-D C4: 1.74 vs 1.77 ms, unchanged) */
  /* Fields: the same kernel choice by N (the bit rule: field q = the scalar sweep on column q), always one target per lane */
  const bool one = j.nf || j.m < (size_t)(culled ? CULL_THREADS : EV_THREADS) * 2 * 512 || (culled && j.dim == 3);
  return with_kind(kind, [&](auto K) {
    constexpr int KIND = decltype(K)::value;
    if constexpr (kind_is_culled(KIND))             /* the other kinds have no culled instances: nothing to cull */
      if (culled) return one ? launch_sweep_cull<KIND, 1>(ctx, j) : launch_sweep_cull<KIND, 2>(ctx, j);
    return one ? launch_sweep<KIND, 1>(ctx, j) : launch_sweep<KIND, 2>(ctx, j);
  });
}

/* Gaussian / Wendland: group the targets spatially so that whole waves skip negligible (Wendland: zero) terms
   together (the kinds that are not culled take every term: nothing to skip, no sort) */
static bool wants_target_sort(int kind, size_t m) { return kind_is_culled(kind) && sinterp_sort_wanted(m); }

extern "C" int gsl_sinterp_hip_rbf_eval(gsl_sinterp_hip_ctx *ctx, int kind, double eps, const double *d_x, size_t n,
                                        int dim, size_t xtda, const double *d_w, const double *d_y, size_t m,
                                        size_t ytda, double *d_s)
{
  return gsl_sinterp_hip_rbf_eval_model(ctx, kind, eps, d_x, n, dim, xtda, d_w, d_y, m, ytda, d_s, 0ULL);
}

extern "C" int gsl_sinterp_hip_rbf_eval_model(gsl_sinterp_hip_ctx *ctx, int kind, double eps, const double *d_x, size_t n,
                                              int dim, size_t xtda, const double *d_w, const double *d_y, size_t m,
                                              size_t ytda, double *d_s, unsigned long long model_id)
{
  REQUIRE(ctx, ctx != NULL, ST_EFAULT);
  HIP_OK(ctx, hipSetDevice(ctx->device));      /* one context per device: bind before any launch */
  REQUIRE(ctx, dim >= 1 && dim <= 3 && xtda >= (size_t)dim && ytda >= (size_t)dim, ST_EINVAL);
  REQUIRE(ctx, known_kind(kind), ST_EINVAL);
  REQUIRE(ctx, m == 0 || (d_y && d_s && (n == 0 || (d_x && d_w))), ST_EFAULT);
  if (m == 0) return ST_SUCCESS;
  int st = ensure_tables(ctx);
  if (st) return st;
  sweep_job j = {kernel_coef(kind, eps), d_x, n, dim, xtda, d_w, d_y, m, ytda, NULL, d_s, NULL, NULL, 0, 0.0, model_id, 0, 0, 0};
  if (wants_target_sort(kind, m)) {
    /* large batches: the targets are physically put in cell order (sort.hip, two-level reorder), swept contiguously, each
       result stored through the order's map, and the values gathered back -- one random pass instead of the three of
       the permutation route (histogram atomics, perm scatter, gather + scatter inside the sweep) */
    if (sinterp_sort_reorder_is_two_level(m)) {
      sinterp_sorted srt;
      st = sinterp_sort_reorder(ctx, d_y, m, ytda, dim, 64, &srt, (const unsigned long long *)NULL);
      if (st) return st;
      if (srt.two_level) {
        j.y = (const double *)srt.ys; j.ytda = (size_t)dim; j.s = srt.res1; j.omap = (const unsigned *)srt.inv;
        st = rbf_sweep_dispatch(ctx, kind, j);
        if (st) return st;
        return sinterp_unsort(ctx, &srt, m, d_s, (int *)NULL);
      }
    }
    int *d_perm = NULL;
    st = sinterp_sort_targets(ctx, d_y, m, ytda, dim, 64, &d_perm);
    if (st) return st;
    j.perm = d_perm;
  }
  return rbf_sweep_dispatch(ctx, kind, j);
}

/* s[k] += c_0 + sum_a c_a y[k][a] (the operations of add_poly_kernel / add_const_kernel in solve.hip: the same bits) and
   g[k][a] += c_a; linear = 0: c_1 .. c_dim are all zero (kriging's mean), only c_0 is added */
__global__ void __launch_bounds__(256)
grad_tail_kernel(double *__restrict__ s, double *__restrict__ g, size_t gtda, size_t m, const double *__restrict__ y, size_t ytda, int dim,
                 double c0, double c1, double c2, double c3, int linear)
{
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < m; k += stride) {
    if (s && !linear) s[k] = s[k] + c0;
    if (!linear) continue;
    if (s) {
      double t = fma(c1, y[k * ytda], c0);
      if (dim > 1) t = fma(c2, y[k * ytda + 1], t);
      if (dim > 2) t = fma(c3, y[k * ytda + 2], t);
      s[k] = s[k] + t;
    }
    g[k * gtda] += c1;
    if (dim > 1) g[k * gtda + 1] += c2;
    if (dim > 2) g[k * gtda + 2] += c3;
  }
}

extern "C" int gsl_sinterp_hip_rbf_eval_grad(gsl_sinterp_hip_ctx *ctx, int kind, double eps, const double *h_tail, const double *d_x,
                                             size_t n, int dim, size_t xtda, const double *d_w, const double *d_y, size_t m,
                                             size_t ytda, double *d_s, double *d_g, size_t gtda, unsigned long long model_id)
{
  REQUIRE(ctx, ctx != NULL, ST_EFAULT);
  HIP_OK(ctx, hipSetDevice(ctx->device));      /* one context per device: bind before any launch */
  REQUIRE(ctx, dim >= 1 && dim <= 3 && xtda >= (size_t)dim && ytda >= (size_t)dim && gtda >= (size_t)dim, ST_EINVAL);
  REQUIRE(ctx, known_kind(kind), ST_EINVAL);
  REQUIRE(ctx, m == 0 || (d_y && d_g && (n == 0 || (d_x && d_w))), ST_EFAULT);
  if (m == 0) return ST_SUCCESS;
  int st = ensure_tables(ctx);
  if (st) return st;
  /* one level of target sort whatever the batch size: the two-level reorder's result path carries one scalar per target */
  int *d_perm = NULL;
  if (wants_target_sort(kind, m)) {
    st = sinterp_sort_targets(ctx, d_y, m, ytda, dim, 64, &d_perm);
    if (st) return st;
  }
  const sweep_job j = {kernel_coef(kind, eps), d_x, n, dim, xtda, d_w, d_y, m, ytda, d_perm, d_s, NULL, d_g, gtda, rbf_grad_scale(kind, eps),
                       model_id, 0, 0, 0};
  st = rbf_sweep_dispatch(ctx, kind, j);
  if (st || !h_tail) return st;
  /* tail c_0 + sum_a c_a y_a: the affine thin-plate polynomial, or kriging's {mu, 0, ...}; h_tail[0 .. dim] only */
  int linear = 0;
  for (int a = 1; a <= dim; a++) linear |= h_tail[a] != 0.0;
  if (!linear && !d_s) return ST_SUCCESS;
  size_t blocks = (m + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(grad_tail_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, d_s, d_g, gtda, m, d_y, ytda, dim, h_tail[0],
                     h_tail[1], dim > 1 ? h_tail[2] : 0.0, dim > 2 ? h_tail[3] : 0.0, linear);
  LAUNCH_CHECK(ctx);
  return ST_SUCCESS;
}

/* ------------------------------------------------------------------------ */
/* Several fields on one set of centres: field q of the sweep has the bits of gsl_sinterp_hip_rbf_eval_model on column q */
extern "C" int gsl_sinterp_hip_rbf_fields_block(void) { return RBF_NF; }
extern "C" int gsl_sinterp_hip_rbf_fields_block_small(void) { return RBF_NF_SMALL; }

/* s[k][q] += c_0(q) + sum_a c_a(q) y[k][a] for FT_Q fields per launch, the coefficients as kernel arguments; per field
   the operations of grad_tail_kernel (linear = 0: only c_0 is added), so field 0 keeps the bits of the scalar path */
#define FT_Q 8
struct fields_tail { double c[FT_Q][4]; int linear[FT_Q]; };

__global__ void __launch_bounds__(256)
fields_tail_kernel(double *__restrict__ s, size_t stda, int nq, size_t m, const double *__restrict__ y, size_t ytda, int dim, fields_tail T)
{
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < m; k += stride) {
#pragma unroll
    for (int q = 0; q < FT_Q; q++) {
      if (q >= nq) break;
      if (!T.linear[q]) { s[k * stda + q] = s[k * stda + q] + T.c[q][0]; continue; }
      double t = fma(T.c[q][1], y[k * ytda], T.c[q][0]);
      if (dim > 1) t = fma(T.c[q][2], y[k * ytda + 1], t);
      if (dim > 2) t = fma(T.c[q][3], y[k * ytda + 2], t);
      s[k * stda + q] = s[k * stda + q] + t;
    }
  }
}

extern "C" int gsl_sinterp_hip_rbf_eval_fields(gsl_sinterp_hip_ctx *ctx, int kind, double eps, const double *h_tail, const double *d_x,
                                               size_t n, int dim, size_t xtda, const double *d_w, size_t ldw, size_t nf,
                                               const double *d_y, size_t m, size_t ytda, double *d_s, size_t stda,
                                               unsigned long long model_id)
{
  REQUIRE(ctx, ctx != NULL, ST_EFAULT);
  HIP_OK(ctx, hipSetDevice(ctx->device));      /* one context per device: bind before any launch */
  REQUIRE(ctx, dim >= 1 && dim <= 3 && xtda >= (size_t)dim && ytda >= (size_t)dim, ST_EINVAL);
  REQUIRE(ctx, known_kind(kind), ST_EINVAL);
  REQUIRE(ctx, nf >= 1 && nf <= GSL_SINTERP_MAX_FIELDS && ldw >= n && stda >= nf, ST_EINVAL);
  REQUIRE(ctx, m == 0 || (d_y && d_s && (n == 0 || (d_x && d_w))), ST_EFAULT);
  if (m == 0) return ST_SUCCESS;
  int st = ensure_tables(ctx);
  if (st) return st;
  /* one level of target sort, as the gradient entry: the two-level reorder's result path carries one scalar per target */
  int *d_perm = NULL;
  if (wants_target_sort(kind, m)) {
    st = sinterp_sort_targets(ctx, d_y, m, ytda, dim, 64, &d_perm);
    if (st) return st;
  }
  const sweep_job j = {kernel_coef(kind, eps), d_x, n, dim, xtda, d_w, d_y, m, ytda, d_perm, d_s, NULL, NULL, 0, 0.0, model_id,
                       (int)nf, ldw, stda};
  st = rbf_sweep_dispatch(ctx, kind, j);
  if (st || !h_tail) return st;
  size_t blocks = (m + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  for (size_t q0 = 0; q0 < nf; q0 += FT_Q) {
    fields_tail T;
    memset(&T, 0, sizeof T);
    const int nq = (int)(nf - q0 < FT_Q ? nf - q0 : FT_Q);
    for (int q = 0; q < nq; q++) {
      const double *c = h_tail + (q0 + q) * (size_t)(dim + 1);
      for (int a = 0; a <= dim; a++) { T.c[q][a] = c[a]; if (a) T.linear[q] |= c[a] != 0.0; }
    }
    hipLaunchKernelGGL(fields_tail_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, d_s + q0, stda, nq, m, d_y, ytda, dim, T);
  }
  LAUNCH_CHECK(ctx);
  return ST_SUCCESS;
}
