/*
 * local.hip -- local kriging, ordinary or with a linear drift: for every target the k <= 64 nearest centres are found exactly
 * and kriging is solved on them alone (a "moving neighbourhood").  Memory O(N + M k), work O(M k^3), no N x N matrix anywhere.
 *
 *   sinterp_grid_bin              bounding box of a cloud, a uniform g^dim grid over it (row-major: axis 0 runs fastest, so
 *                                 the cells of one grid row are ONE contiguous run), histogram and scan: the cell, the place
 *                                 inside the cell and the cell offsets.  Also the first half of shepard.hip's pack.
 *   local_pack (once per model)   that binning, then the gather of the centres into cell order as records {x[dim], f,
 *                                 original index}.
 *   local_krige_kernel            one wave per target: search (growing rings of cells, 64 candidates per step merged into a
 *                                 sorted list of the best k by rank counting), fill of K_S with lane = row, Cholesky with the
 *                                 3 (+ dim with a drift) right-hand sides riding it, fixed-order reductions (lk_sum).
 *
 * Neighbour set: the k smallest keys (r2_j, j), r2 the FMA chain of the sweeps, listed in ascending key order.  The keys are
 * totally ordered and the merge keeps exactly the k smallest of everything seen, so the set does not depend on the order
 * in which cells or records are visited (the order inside a cell is that of the histogram's atomics and varies from run to
 * run).
 *
 * Stop rule.  lk_axis_cell is non-decreasing in the coordinate, and the SAME function bins the centres and is asked here
 * (local_grid.h, "The cell-function contract").  After ring R every cell of the index block [a_c, b_c] (per axis, clamped to the grid) has been visited; an unvisited centre has,
 * on some axis c, a cell index > b_c or < a_c.  For the high side take any coordinate t with lk_axis_cell(t) <= b_c: by
 * monotonicity every centre with index > b_c has x_c > t, hence fl(y_c - x_c) <= fl(y_c - t) <= 0 when t >= y_c and
 * r2 = fl(.. + d_c^2 ..) >= fl(fl(y_c - t)^2) (every later fma adds a non-negative term and rounding is monotone).  The low
 * side is symmetric.  t is taken a millionth of a cell inside the block and CHECKED with lk_axis_cell; a t that fails the
 * check gives the bound 0, which only costs another ring.  The scan ends when the smallest such bound over all open sides
 * exceeds the k-th r2 (strictly: an unvisited centre at an equal r2 could still win on the index), or the block is the grid.
 *
 * Padding.  KMAX in {16, 32, 64} is the compile-time row length, k <= KMAX the run-time one.  Rows i >= k are unit rows
 * (K[i][i] = 1, zeros elsewhere, right-hand sides 0) and rows i < k have zeros in the columns >= k, so K = diag(K_S, I).
 * In column J < k a padding lane computes v = 0 - sum 0 * l = 0 and keeps an exact 0; in column J >= k every broadcast
 * L[J][kk], kk < J, is an exact 0, so v = a[J] unchanged, the pivot is 1, 1/sqrt(1) = 1 and the real lanes (which hold
 * a[J] = 0) are not touched; the right-hand sides of the padding lanes stay 0 and add +0 to every reduction, whose tree is
 * the same 64-lane butterfly for every KMAX.  x + (+0) = x for every x, so no bit of the result depends on KMAX or on the
 * padding.  Lanes >= KMAX hold all-zero rows and behave like padding lanes whose diagonal is never reached.
 */
#include "common.h"
#include <math.h>
#include <float.h>
#include "chol_potrf.h"
#include "rbf_phi.h"

#include "local_grid.h"           /* LkGrid, lk_axis_cell, lk_cell, lk_grid_size, lk_sum, LK_SORT_MIN: shared with shepard.hip */

#define LK_HEAD 256               /* bytes: LkGrid | box keys at 64 | failure counter (64 bits) at 128 */
#define LK_NONE 0x7fffffff        /* index of an empty list entry: (inf, LK_NONE) is above every real key */

__global__ void lk_head_kernel(const unsigned long long *__restrict__ box, int dim, LkGrid *__restrict__ out)
{
  if (threadIdx.x >= 6) return;
  const int c = threadIdx.x >> 1;
  double v = 0.0;
  if (c < dim) {                                   /* the order-preserving keys of sinterp_bbox_keys back to doubles */
    const unsigned long long k = box[threadIdx.x];
    const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffULL) : ~k;
    v = __longlong_as_double((long long)u);
  }
  if (threadIdx.x & 1) out->hi[c] = v; else out->lo[c] = v;
}

/* one atomic per centre: the returned count is the centre's slot inside its cell */
template <int DIM>
__global__ void __launch_bounds__(256)
lk_hist_kernel(const double *__restrict__ x, size_t n, size_t xtda, const LkGrid *__restrict__ grid, int g, unsigned *__restrict__ cellid,
               unsigned *__restrict__ slot, unsigned *__restrict__ count)
{
  const LkGrid G = *grid;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    double v[DIM];
#pragma unroll
    for (int c = 0; c < DIM; c++) v[c] = x[i * xtda + c];
    const unsigned cell = (unsigned)lk_cell<DIM>(G, g, v);
    cellid[i] = cell;
    slot[i] = atomicAdd(&count[cell], 1u);
  }
}

template <int DIM>
__global__ void __launch_bounds__(256)
lk_gather_kernel(const double *__restrict__ x, size_t n, size_t xtda, const double *__restrict__ f, const unsigned *__restrict__ cellid,
                 const unsigned *__restrict__ slot, const unsigned *__restrict__ offset, double *__restrict__ rec)
{
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    double *r = rec + ((size_t)offset[cellid[i]] + slot[i]) * (DIM + 2);
#pragma unroll
    for (int c = 0; c < DIM; c++) r[c] = x[i * xtda + c];
    r[DIM] = f ? f[i] : 0.0;
    r[DIM + 1] = __longlong_as_double((long long)i);
  }
}

/* ------------------------------------------------------------------------ */
__device__ __forceinline__ bool lk_less(double ar, int ai, double br, int bi) { return ar < br || (ar == br && ai < bi); }

/* The search state of one wave.  The sorted list of the best <= k keys lives one entry per lane in registers (b*) and in
   the first half of the LDS arrays; the second half takes the 64 candidates of a step. */
struct LkList {
  double *s_r2; int *s_id; unsigned *s_pos;        /* [128] each */
  double br2; int bid; unsigned bpos;              /* this lane's entry */
  double kr2; int kid;                             /* the k-th key (uniform); (inf, LK_NONE) while the list is not full */
};

/* records [b, e) of the cell order against the list: 64 per step.  A candidate that does not beat the k-th key is
   dropped at once; a step without a survivor costs the distance only.  Otherwise every survivor and every list entry
   counts the keys below its own (uniform LDS reads: broadcasts) -- its place in the merged order, no atomics -- and the
   entries placed below k are scattered to the new list. */
template <int DIM>
__device__ __forceinline__ void lk_scan_run(LkList &L, const double (&y)[DIM], const double *__restrict__ rec, unsigned b, unsigned e, int k,
                                            int lane)
{
  for (unsigned p0 = b; p0 < e; p0 += 64) {
    const unsigned p = p0 + lane;
    double cr2 = INFINITY;
    int cid = LK_NONE;
    if (p < e) {
      const double *r = rec + (size_t)p * (DIM + 2);
      double r2 = 0.0;
#pragma unroll
      for (int c = 0; c < DIM; c++) { const double d = y[c] - r[c]; r2 = fma(d, d, r2); }
      const int id = (int)__double_as_longlong(r[DIM + 1]);
      if (lk_less(r2, id, L.kr2, L.kid)) { cr2 = r2; cid = id; }
    }
    if (!__any(cid != LK_NONE)) continue;          /* wave-uniform */
    L.s_r2[64 + lane] = cr2; L.s_id[64 + lane] = cid; L.s_pos[64 + lane] = p;
    __syncthreads();                               /* the workgroup is this wave */
    int rb = lane, rc = 0;
#pragma unroll 4
    for (int q = 0; q < 64; q++) {
      const double tr = L.s_r2[64 + q], ur = L.s_r2[q];
      const int ti = L.s_id[64 + q], ui = L.s_id[q];
      rb += lk_less(tr, ti, L.br2, L.bid);
      rc += lk_less(tr, ti, cr2, cid);
      rc += lk_less(ur, ui, cr2, cid);
    }
    __syncthreads();
    L.s_r2[lane] = INFINITY; L.s_id[lane] = LK_NONE; L.s_pos[lane] = 0u;
    __syncthreads();
    if (L.bid != LK_NONE && rb < k) { L.s_r2[rb] = L.br2; L.s_id[rb] = L.bid; L.s_pos[rb] = L.bpos; }
    if (cid != LK_NONE && rc < k) { L.s_r2[rc] = cr2; L.s_id[rc] = cid; L.s_pos[rc] = p; }
    __syncthreads();
    L.br2 = L.s_r2[lane]; L.bid = L.s_id[lane]; L.bpos = L.s_pos[lane];
    L.kr2 = L.s_r2[k - 1]; L.kid = L.s_id[k - 1];
  }
}

/* the exact k nearest centres of y (header: the stop rule).  Everything that steers the loops is wave-uniform. */
template <int DIM>
__device__ __forceinline__ void lk_search(LkList &L, const double (&y)[DIM], const LkGrid &G, int g, const unsigned *__restrict__ off,
                                          const double *__restrict__ rec, int k, int lane)
{
  int ci[3] = {0, 0, 0};
#pragma unroll
  for (int c = 0; c < DIM; c++) ci[c] = __builtin_amdgcn_readfirstlane(lk_axis_cell(y[c], G.lo[c], G.hi[c], g));
  L.br2 = INFINITY; L.bid = LK_NONE; L.bpos = 0u; L.kr2 = INFINITY; L.kid = LK_NONE;
  L.s_r2[lane] = INFINITY; L.s_id[lane] = LK_NONE; L.s_pos[lane] = 0u;
  __syncthreads();
  for (int R = 0;; R++) {
    int a[3] = {0, 0, 0}, b[3] = {0, 0, 0};
#pragma unroll
    for (int c = 0; c < DIM; c++) { a[c] = ci[c] - R > 0 ? ci[c] - R : 0; b[c] = ci[c] + R < g - 1 ? ci[c] + R : g - 1; }
    for (int i2 = a[2]; i2 <= b[2]; i2++)
      for (int i1 = a[1]; i1 <= b[1]; i1++) {
        /* a grid row on the shell of the block in axis 1 or 2 is new along its whole length; an inner row brings its two ends */
        const bool whole = R == 0 || (DIM >= 2 && (i1 - ci[1] == R || ci[1] - i1 == R)) || (DIM == 3 && (i2 - ci[2] == R || ci[2] - i2 == R));
        const size_t row = ((size_t)i2 * (size_t)g + (size_t)i1) * (size_t)g;
        if (whole) {
          lk_scan_run<DIM>(L, y, rec, __builtin_amdgcn_readfirstlane(off[row + a[0]]), __builtin_amdgcn_readfirstlane(off[row + b[0] + 1]), k, lane);
        } else {
          if (ci[0] - R >= 0)
            lk_scan_run<DIM>(L, y, rec, __builtin_amdgcn_readfirstlane(off[row + ci[0] - R]),
                             __builtin_amdgcn_readfirstlane(off[row + ci[0] - R + 1]), k, lane);
          if (ci[0] + R <= g - 1)
            lk_scan_run<DIM>(L, y, rec, __builtin_amdgcn_readfirstlane(off[row + ci[0] + R]),
                             __builtin_amdgcn_readfirstlane(off[row + ci[0] + R + 1]), k, lane);
        }
      }
    bool closed = true;
    double lb = INFINITY;
#pragma unroll
    for (int c = 0; c < DIM; c++) {
      const double lo = G.lo[c], hi = G.hi[c];
      if (!(hi > lo)) continue;                    /* every centre is in cell 0 of this axis: nothing lies outside */
      if (b[c] < g - 1) {
        closed = false;
        const double t = lo + (hi - lo) * (((double)(b[c] + 1) - 1e-6) / (double)g);
        const double gap = lk_axis_cell(t, lo, hi, g) <= b[c] ? fmax(t - y[c], 0.0) : 0.0;
        lb = fmin(lb, gap * gap);
      }
      if (a[c] > 0) {
        closed = false;
        const double t = lo + (hi - lo) * (((double)a[c] + 1e-6) / (double)g);
        const double gap = lk_axis_cell(t, lo, hi, g) >= a[c] ? fmax(y[c] - t, 0.0) : 0.0;
        lb = fmin(lb, gap * gap);
      }
    }
    if (closed) break;
    if (L.kid != LK_NONE && lb > L.kr2) break;
  }
}

/* ------------------------------------------------------------------------ */
template <int DIM>
__global__ void __launch_bounds__(64)
local_knn_kernel(const LkGrid *__restrict__ grid, int g, const unsigned *__restrict__ off, const double *__restrict__ rec,
                 const double *__restrict__ yv, size_t ytda, const int *__restrict__ perm, int k, int *__restrict__ idx,
                 double *__restrict__ r2out)
{
  __shared__ double s_r2[128];
  __shared__ int s_id[128];
  __shared__ unsigned s_pos[128];
  const int lane = threadIdx.x;
  const size_t t = perm ? (size_t)perm[blockIdx.x] : (size_t)blockIdx.x;
  double y[DIM];
  bool isnan_y = false;
#pragma unroll
  for (int c = 0; c < DIM; c++) { y[c] = yv[t * ytda + c]; isnan_y |= y[c] != y[c]; }
  if (isnan_y) {
    if (lane < k) { idx[t * (size_t)k + lane] = -1; if (r2out) r2out[t * (size_t)k + lane] = NAN; }
    return;
  }
  const LkGrid G = *grid;
  LkList L;
  L.s_r2 = s_r2; L.s_id = s_id; L.s_pos = s_pos;
  lk_search<DIM>(L, y, G, g, off, rec, k, lane);
  if (lane < k) {
    const bool have = L.bid != LK_NONE;
    idx[t * (size_t)k + lane] = have ? L.bid : -1;
    if (r2out) r2out[t * (size_t)k + lane] = have ? L.br2 : NAN;
  }
}

/* The two combine stages of local_krige_kernel, from u = L^-1 k_S, v = L^-1 1, g = L^-1 f_S (one entry per lane): every
   sum in lk_sum's fixed order, everything the same on every lane.  Ordinary kriging: */
__device__ __forceinline__ void lk_combine_ordinary(double bu, double bv, double bg, double phi0, double &s, double &var)
{
  const double dd = lk_sum(bv * bv), vg = lk_sum(bv * bg), uu = lk_sum(bu * bu), vu = lk_sum(bv * bu);
  const double mu = vg / dd;
  const double ug = lk_sum(bu * fma(-mu, bv, bg));
  const double tt = 1.0 - vu;
  s = mu + ug; var = (phi0 - uu) + tt * tt / dd;
}

/* UNIVERSAL kriging with a linear drift ("Universal kriging"): bp = L^-1 of the DIM coordinate columns in the
   local basis u = (x_i - y) / h, h = the distance of the k-th (farthest) neighbour: at the target p = e_0, and the columns
   of P_S = [1 | u] are of order one whatever the units of the coordinates.  With V = L^-1 P_S = [bv | bp]:
       S = V^T V (lk_sum reductions, the same on every lane), a scalar Cholesky S = Ls Ls^T on every lane,
       c = S^-1 V^T g,   s = c_0 + u^T (g - V c),   sigma^2 = phi(0) - u^T u + r^T S^-1 r,   r = e_0 - V^T u.
   Sets bad for an S pivot not above 64 u times that diagonal entry of S before elimination, or not finite (a collinear /
   coplanar neighbourhood). */
template <int DIM>
__device__ __forceinline__ void lk_combine_universal(double bu, double bv, double bg, const double (&bp)[DIM], double phi0, bool &bad,
                                                     double &s, double &var)
{
  constexpr int Q = DIM + 1;
  double V[Q];
  V[0] = bv;
#pragma unroll
  for (int c = 0; c < DIM; c++) V[1 + c] = bp[c];
  double S[Q][Q], Vg[Q], r[Q];
#pragma unroll
  for (int p = 0; p < Q; p++) {
#pragma unroll
    for (int q = 0; q <= p; q++) S[p][q] = lk_sum(V[p] * V[q]);
    Vg[p] = lk_sum(V[p] * bg);
    r[p] = (p == 0 ? 1.0 : 0.0) - lk_sum(V[p] * bu);
  }
  const double uu = lk_sum(bu * bu);
  /* S = Ls Ls^T in place (lower triangle) */
#pragma unroll
  for (int j = 0; j < Q; j++) {
    const double s0 = S[j][j];
    double d = s0;
#pragma unroll
    for (int q = 0; q < j; q++) d = fma(-S[j][q], S[j][q], d);
    bad |= !(d > 64.0 * DBL_EPSILON * s0) || !(d < INFINITY);
    const double lj = sqrt(d);
    S[j][j] = lj;
#pragma unroll
    for (int p = j + 1; p < Q; p++) {
      double v = S[p][j];
#pragma unroll
      for (int q = 0; q < j; q++) v = fma(-S[p][q], S[j][q], v);
      S[p][j] = v / lj;
    }
  }
  /* c = S^-1 V^T g (two triangular solves); |Ls^-1 r|^2 */
  double c[Q], rr = 0.0;
#pragma unroll
  for (int p = 0; p < Q; p++) {
    double v = Vg[p], w = r[p];
#pragma unroll
    for (int q = 0; q < p; q++) { v = fma(-S[p][q], c[q], v); w = fma(-S[p][q], r[q], w); }
    c[p] = v / S[p][p];
    r[p] = w / S[p][p];
    rr = fma(r[p], r[p], rr);
  }
#pragma unroll
  for (int p = Q - 1; p >= 0; p--) {
    double v = c[p];
#pragma unroll
    for (int q = p + 1; q < Q; q++) v = fma(-S[q][p], c[q], v);
    c[p] = v / S[p][p];
  }
  double res = bg;                                  /* this lane's entry of g - V c */
#pragma unroll
  for (int p = 0; p < Q; p++) res = fma(-c[p], V[p], res);
  s = c[0] + lk_sum(bu * res); var = (phi0 - uu) + rr;
}

/* One wave per target: search, fill, factorisation with the right-hand sides riding it, combine (header; DESIGN.md, "Local
   kriging").  Lane i owns row i of K_S in registers; column J is formed left-looking,
       V_J[i] = K[i][J] - sum_{kk<J} L[i][kk] L[J][kk],   L[i][J] = V_J[i] / sqrt(V_J[J]),
   with L[J][kk] read from lane J, and as soon as column J exists the right-hand sides take their step of the forward
   substitution (lane J's entry becomes final, the lanes below it are updated): k_S, 1 and f_S, and with DRIFT the NP = DIM
   coordinate columns of lk_combine_universal.  Failed (NaN in value and variance, counted): a pivot not above
   64 u (phi(0) + nugget) or not finite -- the rounding residue of an exactly singular system, two coincident sites
   without a nugget, has either sign; with DRIFT also h = 0 and a failed pivot of S. */
template <int KIND, int DIM, int KMAX, bool DRIFT>
__global__ void __launch_bounds__(64)
local_krige_kernel(double coef, double nugget, const double *__restrict__ tbl, const LkGrid *__restrict__ grid, int g,
                   const unsigned *__restrict__ off, const double *__restrict__ rec, const double *__restrict__ yv, size_t ytda,
                   const int *__restrict__ perm, int k, double *__restrict__ sout, double *__restrict__ vout, int *__restrict__ idx,
                   unsigned long long *__restrict__ n_failed)
{
  constexpr int NP = DRIFT ? DIM : 0;
  __shared__ double s_t0[kind_uses_exp2(KIND) ? TBL_N : 1];
  __shared__ double s_r2[128];
  __shared__ int s_id[128];
  __shared__ unsigned s_pos[128];
  __shared__ double s_x[DIM][64];
  const int lane = threadIdx.x;
  if (kind_uses_exp2(KIND)) {
#pragma unroll
    for (int q = 0; q < TBL_N / 64; q++) s_t0[lane + 64 * q] = tbl[lane + 64 * q];
  }
  const size_t t = perm ? (size_t)perm[blockIdx.x] : (size_t)blockIdx.x;
  double y[DIM];
  bool isnan_y = false;
#pragma unroll
  for (int c = 0; c < DIM; c++) { y[c] = yv[t * ytda + c]; isnan_y |= y[c] != y[c]; }
  if (isnan_y) {                                   /* no neighbours; not a failed pivot */
    if (idx && lane < k) idx[t * (size_t)k + lane] = -1;
    if (lane == 0) { if (sout) sout[t] = NAN; if (vout) vout[t] = NAN; }
    return;
  }
  const LkGrid G = *grid;
  LkList L;
  L.s_r2 = s_r2; L.s_id = s_id; L.s_pos = s_pos;
  lk_search<DIM>(L, y, G, g, off, rec, k, lane);   /* its first barrier also covers the table */
  const bool real = lane < k && L.bid != LK_NONE;
  if (idx && lane < k) idx[t * (size_t)k + lane] = real ? L.bid : -1;
  if (!sout && !vout) return;
  bool bad = __any(lane < k && !real);             /* fewer than k centres with a finite distance */

  /* ---- fill */
  double xi[DIM], fi = 0.0;
#pragma unroll
  for (int c = 0; c < DIM; c++) xi[c] = 0.0;
  if (real) {
    const double *r = rec + (size_t)L.bpos * (DIM + 2);
#pragma unroll
    for (int c = 0; c < DIM; c++) xi[c] = r[c];
    fi = r[DIM];
  }
#pragma unroll
  for (int c = 0; c < DIM; c++) s_x[c][lane] = xi[c];
  __syncthreads();
  const double phi0 = phi_r2<KIND, 1>(0.0, coef, s_t0, s_t0);
  const double diag = phi0 + nugget;
  double a[KMAX];
#pragma unroll
  for (int j = 0; j < KMAX; j++) {
    double r2 = 0.0;
#pragma unroll
    for (int c = 0; c < DIM; c++) { const double d = xi[c] - s_x[c][j]; r2 = fma(d, d, r2); }
    const double v = phi_r2<KIND, 1>(r2, coef, s_t0, s_t0);
    a[j] = (real && j < k) ? (j == lane ? diag : v) : (j == lane ? 1.0 : 0.0);
    /* one entry at a time: left alone the scheduler interleaves all KMAX kernel evaluations and runs out of registers
       (no instruction is emitted; the clobber keeps the LDS reads of the next entry behind this point) */
    asm volatile("" : "+v"(a[j]) : : "memory");
  }
  double bu = real ? phi_r2<KIND, 1>(L.br2, coef, s_t0, s_t0) : 0.0;      /* k_S */
  double bv = real ? 1.0 : 0.0;                                           /* 1: with DRIFT the constant term of the drift */
  double bg = real ? fi : 0.0;                                            /* f_S */
  double bp[NP > 0 ? NP : 1];                                             /* the coordinate columns, u = (x_i - y) / h */
  if constexpr (DRIFT) {
    /* the neighbours arrive nearest first: lane k - 1 holds the farthest.  h = 0 (k coincident sites at the target) fails */
    const double h = sqrt(lane_bcast(L.br2, k - 1));
    bad |= !(h > 0.0) || !(h < INFINITY);
    const double hinv = 1.0 / h;
#pragma unroll
    for (int c = 0; c < NP; c++) bp[c] = real ? (xi[c] - y[c]) * hinv : 0.0;
  }

  /* ---- factorisation and the 3 + NP forward substitutions */
  const double dmin = diag * (64.0 * DBL_EPSILON);
#pragma unroll
  for (int J = 0; J < KMAX; J++) {
    double v = a[J];
#pragma unroll
    for (int kk = 0; kk < J; kk++) v = fma(-a[kk], lane_bcast(a[kk], J), v);
    const double d = lane_bcast(v, J);
    bad |= !(d > dmin) || !(d < INFINITY);
    const double rinv = 1.0 / sqrt(d);
    const double l = lane >= J ? v * rinv : 0.0;   /* the part of row i right of the diagonal is cleared on the way */
    a[J] = l;
    const double uJ = lane_bcast(bu, J) * rinv, vJ = lane_bcast(bv, J) * rinv, gJ = lane_bcast(bg, J) * rinv;
    bu = lane == J ? uJ : fma(-l, uJ, bu);
    bv = lane == J ? vJ : fma(-l, vJ, bv);
    bg = lane == J ? gJ : fma(-l, gJ, bg);
#pragma unroll
    for (int c = 0; c < NP; c++) {
      const double pJ = lane_bcast(bp[c], J) * rinv;
      bp[c] = lane == J ? pJ : fma(-l, pJ, bp[c]);
    }
  }

  /* ---- combine */
  double s, var;
  if constexpr (DRIFT) lk_combine_universal<DIM>(bu, bv, bg, bp, phi0, bad, s, var);
  else lk_combine_ordinary(bu, bv, bg, phi0, s, var);
  if (bad) { s = NAN; var = NAN; }
  if (lane == 0) {
    if (sout) sout[t] = s;
    if (vout) vout[t] = var;
    if (bad) atomicAdd(n_failed, 1ULL);
  }
}

/* ------------------------------------------------------------------------ */
struct lk_model {
  const LkGrid *grid;
  const unsigned *off;
  const double *rec;
  unsigned long long *n_failed;
  int g;
};

/* common.h.  The steps: sinterp_bbox_keys, the head, the histogram whose atomics hand every point its slot, the scan. */
int sinterp_grid_bin(gsl_sinterp_hip_ctx *ctx, const double *d_x, size_t n, int dim, size_t xtda, int g, LkGrid *d_grid,
                     unsigned long long *d_box, unsigned *d_off, unsigned *d_cellid, unsigned *d_slot)
{
  size_t ncell = 1;
  for (int c = 0; c < dim; c++) ncell *= (size_t)g;
  int st = sinterp_bbox_keys(ctx, d_x, n, xtda, dim, d_box);
  if (st) return st;
  hipLaunchKernelGGL(lk_head_kernel, dim3(1), dim3(64), 0, ctx->stream, (const unsigned long long *)d_box, dim, d_grid);
  HIP_OK(ctx, hipMemsetAsync(d_off, 0, ncell * 4, ctx->stream));
  size_t blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  with_dim(dim, [&](auto D) {
    hipLaunchKernelGGL((lk_hist_kernel<decltype(D)::value>), dim3((unsigned)blocks), dim3(256), 0, ctx->stream, d_x, n, xtda,
                       (const LkGrid *)d_grid, g, d_cellid, d_slot, d_off);
  });
  sinterp_scan_u32(ctx, d_off, ncell, d_off + ncell + 1);
  LAUNCH_CHECK(ctx);
  return ST_SUCCESS;
}

/* the packed centres of the local route, cached per model like the culled sweep's (cull_pack in rbf.hip) */
static int local_pack(gsl_sinterp_hip_ctx *ctx, const double *d_x, size_t n, int dim, size_t xtda, const double *d_f,
                      unsigned long long model_id, lk_model *out)
{
  gsl_sinterp_hip_ctx::CentKey &key = ctx->local_key;
  const bool cached = sinterp_key_vouches(key, model_id, d_x, d_f, n, xtda, dim);
  const int g = cached ? ctx->local_g : lk_grid_size(n, dim);
  size_t ncell = 1;
  for (int c = 0; c < dim; c++) ncell *= (size_t)g;
  const size_t off_bytes = round_up(lk_off_words(ncell) * 4, 16);
  const size_t bytes = LK_HEAD + off_bytes + n * (size_t)(dim + 2) * sizeof(double);
  if (!cached) key.id = 0;                         /* the buffer may move or be rewritten */
  void *buf = NULL;
  int st = sinterp_localbuf(ctx, bytes, &buf);
  if (st) return st;
  char *b = (char *)buf;
  LkGrid *grid = (LkGrid *)b;
  unsigned *off = (unsigned *)(b + LK_HEAD);
  double *rec = (double *)(b + LK_HEAD + off_bytes);
  out->grid = grid; out->off = off; out->rec = rec; out->n_failed = (unsigned long long *)(b + 128); out->g = g;
  if (cached) return ST_SUCCESS;
  void *tmp = NULL;
  st = sinterp_sortbuf2(ctx, n * 8, &tmp);
  if (st) return st;
  unsigned *cellid = (unsigned *)tmp, *slot = cellid + n;
  st = sinterp_grid_bin(ctx, d_x, n, dim, xtda, g, grid, (unsigned long long *)(b + 64), off, cellid, slot);
  if (st) return st;
  size_t blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  with_dim(dim, [&](auto D) {
    hipLaunchKernelGGL((lk_gather_kernel<decltype(D)::value>), dim3((unsigned)blocks), dim3(256), 0, ctx->stream, d_x, n, xtda, d_f,
                       (const unsigned *)cellid, (const unsigned *)slot, (const unsigned *)off, rec);
  });
  LAUNCH_CHECK(ctx);
  ctx->local_g = g;
  ctx->local_packs++;
  sinterp_key_set(key, model_id, d_x, d_f, n, xtda, dim);
  return ST_SUCCESS;
}

/* targets in cell order for large batches: neighbouring waves then read the same cells */
static int local_target_order(gsl_sinterp_hip_ctx *ctx, const double *d_y, size_t m, size_t ytda, int dim, int **d_perm)
{
  *d_perm = NULL;
  if (m < LK_SORT_MIN) return ST_SUCCESS;
  return sinterp_sort_targets(ctx, d_y, m, ytda, dim, 64, d_perm);
}

template <int KIND, int DIM>
static void launch_local_krige(gsl_sinterp_hip_ctx *ctx, double coef, double nugget, const double *tbl, const lk_model &lm, const double *d_y,
                               size_t m, size_t ytda, const int *perm, int k, bool drift, double *d_s, double *d_var, int *d_idx)
{
  auto go = [&](auto KMAX, auto DRIFT) {
    hipLaunchKernelGGL((local_krige_kernel<KIND, DIM, decltype(KMAX)::value, decltype(DRIFT)::value>), dim3((unsigned)m), dim3(64), 0,
                       ctx->stream, coef, nugget, tbl, lm.grid, lm.g, lm.off, lm.rec, d_y, ytda, perm, k, d_s, d_var, d_idx, lm.n_failed);
  };
  auto with_kmax = [&](auto DRIFT) {
    if (k <= 16) go(ic<16>(), DRIFT);
    else if (k <= 32) go(ic<32>(), DRIFT);
    else go(ic<64>(), DRIFT);
  };
  if (drift) with_kmax(std::true_type()); else with_kmax(std::false_type());
}

extern "C" int gsl_sinterp_hip_local_pack(gsl_sinterp_hip_ctx *ctx, const double *d_x, size_t n, int dim, size_t xtda, const double *d_f,
                                          unsigned long long model_id)
{
  REQUIRE(ctx, n >= 1 && n <= 0x7fffffffULL && dim >= 1 && dim <= 3 && xtda >= (size_t)dim, ST_EINVAL);
  REQUIRE(ctx, ctx != NULL && d_x != NULL, ST_EFAULT);
  HIP_OK(ctx, hipSetDevice(ctx->device));
  lk_model lm;
  return local_pack(ctx, d_x, n, dim, xtda, d_f, model_id, &lm);
}

extern "C" int gsl_sinterp_hip_knn(gsl_sinterp_hip_ctx *ctx, const double *d_x, size_t n, int dim, size_t xtda, const double *d_y, size_t m,
                                   size_t ytda, size_t k, int *d_idx, double *d_r2, unsigned long long model_id)
{
  /* the arguments first: nothing here touches the device */
  REQUIRE(ctx, k >= 1 && k <= 64 && k <= n && dim >= 1 && dim <= 3, ST_EINVAL);
  REQUIRE(ctx, xtda >= (size_t)dim && ytda >= (size_t)dim && n <= 0x7fffffffULL && m <= 0x7fffffffULL, ST_EINVAL);
  REQUIRE(ctx, ctx != NULL && d_x != NULL && (m == 0 || (d_y != NULL && d_idx != NULL)), ST_EFAULT);
  if (m == 0) return ST_SUCCESS;
  HIP_OK(ctx, hipSetDevice(ctx->device));
  lk_model lm;
  int st = local_pack(ctx, d_x, n, dim, xtda, NULL, model_id, &lm);
  if (st) return st;
  int *perm = NULL;
  st = local_target_order(ctx, d_y, m, ytda, dim, &perm);
  if (st) return st;
  with_dim(dim, [&](auto D) {
    hipLaunchKernelGGL((local_knn_kernel<decltype(D)::value>), dim3((unsigned)m), dim3(64), 0, ctx->stream, lm.grid, lm.g, lm.off, lm.rec, d_y,
                       ytda, (const int *)perm, (int)k, d_idx, d_r2);
  });
  LAUNCH_CHECK(ctx);
  return ST_SUCCESS;
}

/* what the two local-kriging entries do once they have checked their arguments; `what` is the entry's failure message */
static int local_krige_run(gsl_sinterp_hip_ctx *ctx, int kind, double eps, double nugget, const double *d_x, size_t n, int dim, size_t xtda,
                           const double *d_f, const double *d_y, size_t m, size_t ytda, size_t k, double *d_s, double *d_var, int *d_idx,
                           size_t *h_n_failed, unsigned long long model_id, bool drift, const char *what)
{
  if (m == 0 || (!d_s && !d_var && !d_idx)) return ST_SUCCESS;
  HIP_OK(ctx, hipSetDevice(ctx->device));
  lk_model lm;
  int st = local_pack(ctx, d_x, n, dim, xtda, d_f, model_id, &lm);
  if (st) return st;
  const double *tbl = NULL;
  st = sinterp_rbf_exp2_table(ctx, &tbl);
  if (st) return st;
  int *perm = NULL;
  st = local_target_order(ctx, d_y, m, ytda, dim, &perm);
  if (st) return st;
  HIP_OK(ctx, hipMemsetAsync(lm.n_failed, 0, sizeof *lm.n_failed, ctx->stream));
  const double coef = kernel_coef(kind, eps);
  with_kind(kind, [&](auto K) {
    if constexpr (kind_is_pd(decltype(K)::value))            /* kind_is_pd(kind) was required by the entries */
      with_dim(dim, [&](auto D) {
        launch_local_krige<decltype(K)::value, decltype(D)::value>(ctx, coef, nugget, tbl, lm, d_y, m, ytda, perm, (int)k, drift, d_s, d_var,
                                                                   d_idx);
      });
  });
  LAUNCH_CHECK(ctx);
  /* the failed pivots are the status: always wait for the batch (everything else has been stored by then) */
  long long failed = 0;
  st = sinterp_outside_count(ctx, lm.n_failed, &failed, what);
  if (h_n_failed) *h_n_failed = (size_t)failed;
  return st;
}

extern "C" int gsl_sinterp_hip_local_krige(gsl_sinterp_hip_ctx *ctx, int kind, double eps, double nugget, const double *d_x, size_t n, int dim,
                                           size_t xtda, const double *d_f, const double *d_y, size_t m, size_t ytda, size_t k, double *d_s,
                                           double *d_var, int *d_idx, size_t *h_n_failed, unsigned long long model_id)
{
  if (h_n_failed) *h_n_failed = 0;
  REQUIRE(ctx, k >= 1 && k <= 64 && k <= n && dim >= 1 && dim <= 3, ST_EINVAL);
  REQUIRE(ctx, kind_is_pd(kind) && nugget >= 0.0 && nugget < INFINITY && eps > 0.0 && eps < INFINITY, ST_EINVAL);
  REQUIRE(ctx, xtda >= (size_t)dim && ytda >= (size_t)dim && n <= 0x7fffffffULL && m <= 0x7fffffffULL, ST_EINVAL);
  REQUIRE(ctx, ctx != NULL && d_x != NULL && d_f != NULL && (m == 0 || d_y != NULL), ST_EFAULT);
  return local_krige_run(ctx, kind, eps, nugget, d_x, n, dim, xtda, d_f, d_y, m, ytda, k, d_s, d_var, d_idx, h_n_failed, model_id, false,
                         "local_krige: a neighbourhood's covariance matrix is not positive definite (value and variance NaN there)");
}

/* the same entry with a linear drift: k >= dim + 2 neighbours */
extern "C" int gsl_sinterp_hip_local_ukrige(gsl_sinterp_hip_ctx *ctx, int kind, double eps, double nugget, const double *d_x, size_t n, int dim,
                                            size_t xtda, const double *d_f, const double *d_y, size_t m, size_t ytda, size_t k, double *d_s,
                                            double *d_var, int *d_idx, size_t *h_n_failed, unsigned long long model_id)
{
  if (h_n_failed) *h_n_failed = 0;
  REQUIRE(ctx, dim >= 1 && dim <= 3 && k >= (size_t)dim + 2 && k <= 64 && k <= n, ST_EINVAL);
  REQUIRE(ctx, kind_is_pd(kind) && nugget >= 0.0 && nugget < INFINITY && eps > 0.0 && eps < INFINITY, ST_EINVAL);
  REQUIRE(ctx, xtda >= (size_t)dim && ytda >= (size_t)dim && n <= 0x7fffffffULL && m <= 0x7fffffffULL, ST_EINVAL);
  REQUIRE(ctx, ctx != NULL && d_x != NULL && d_f != NULL && (m == 0 || d_y != NULL), ST_EFAULT);
  return local_krige_run(ctx, kind, eps, nugget, d_x, n, dim, xtda, d_f, d_y, m, ytda, k, d_s, d_var, d_idx, h_n_failed, model_id, true,
                         "local_ukrige: a neighbourhood's covariance matrix is not positive definite, or its sites do not determine a linear drift (value and variance NaN there)");
}

extern "C" unsigned long long gsl_sinterp_hip_local_pack_count(const gsl_sinterp_hip_ctx *ctx) { return ctx ? ctx->local_packs : 0ULL; }
