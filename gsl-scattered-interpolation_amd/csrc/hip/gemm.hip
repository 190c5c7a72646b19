/*
 * gemm.hip -- the Level-3 building block of the dense solves: C -= A * op(B) on
 * v_mfma_f64_16x16x4_f64 (gfx950).  The reference factorizations are Level-2
 * (linalg/cholesky.c:105-116 gaxpy via cblas/source_gemv_r.h:60-75;
 * linalg/lu.c:105-119 rank-1 updates); the blocked drivers in chol.hip / lu.hip
 * move all O(N^3) work here (the role gsl_blas_dsyrk / dgemm / dtrsm,
 * blas/blas.c:1334,1649,2105, would play in a blocked GSL routine).
 *
 * Tiling (one workgroup = 256 threads = 4 waves, 2x2):
 *   block tile 128 x 128, K step 16, double-buffered LDS, register-staged
 *   prefetch of the next K step issued before the MFMAs of the current one;
 *   each wave owns a 64 x 64 sub-tile = 4 x 4 MFMA fragments (16 accumulators
 *   of 4 f64 -> 128 VGPRs), 64 MFMAs per K step.
 * LDS images:
 *   A (and B when stored [n][k]) as [row][16 + 2]: the fragment read
 *   (row = lane&15, k = lane>>4) is a conflict-free ds_read_b64 because the
 *   row pitch (18 doubles) is = 2 mod 4;
 *   B stored [k][n] as [k][128 + 16]: consecutive lanes read consecutive n.
 * MFMA operand maps (cdna_hip_programming.md section 3): A[i=lane&15][k=lane>>4],
 *   B[k=lane>>4][j=lane&15], D[row=(lane>>4)+4*reg][col=lane&15].
 */
#include "common.h"
#include <stdlib.h>
#include <string.h>
#include "chol_potrf.h"
#include "gemm_plan.h"           /* GT_BM / GT_BN / GT_BK, DM_STAGES, SK_*: the tile constants the dispatch rule shares */

static_assert(GEMM_RIDER_LDS == DIAG128_LDS_BYTES + 16, "gemm_plan.h: the rider's LDS image");
#define GT_LDA (GT_BK + 2)      /* 18 */
#define GT_LDBN (GT_BN + 16)    /* 144 */
#define GT_ASZ (GT_BM * GT_LDA) /* 2304 doubles */
#define GT_BSZ 2304             /* max(128*18, 16*144) */

struct GemmArgs {
  size_t m, n, k;
  const double *A; size_t lda;
  const double *B; size_t ldb;
  double *C; size_t ldc;
  int lower_only;
  int tiles_m, tiles_n;
  unsigned n_active;   /* tiles that are launched: all, or the lower trapezoid when lower_only */
};

__device__ __forceinline__ double2 ld2(const double *p, bool ok0, bool ok1, bool vec)
{
  if (vec && ok1) return *reinterpret_cast<const double2 *>(p);
  double2 v;
  v.x = ok0 ? p[0] : 0.0;
  v.y = ok1 ? p[1] : 0.0;
  return v;
}

template <int B_IS_KN, bool FULL>
__global__ void __launch_bounds__(256, 2)
gemm_minus_kernel(GemmArgs g)
{
  __shared__ __attribute__((aligned(16))) double sA[2][GT_ASZ];
  __shared__ __attribute__((aligned(16))) double sB[2][GT_BSZ];

  /* XCD-aware tile order: blocks b and b+8 share an XCD (and its L2), so give
     each XCD a contiguous run of tiles (bijective for any grid size) */
  const unsigned nwg = gridDim.x, bid = blockIdx.x;
  const unsigned q = nwg / 8, r = nwg % 8, xcd = bid % 8;
  const unsigned tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + bid / 8;
  int tm, tn;
  if (!g.lower_only) {
    tm = (int)(tile / g.tiles_n); tn = (int)(tile % g.tiles_n);
  } else {
    /* only the lower trapezoid is launched (row tm holds min(tm+1, tiles_n) tiles), so every XCD
       gets the same number of equally heavy tiles; consecutive ids share the A row panel */
    const unsigned tri = (unsigned)g.tiles_n * (unsigned)(g.tiles_n + 1) / 2;
    if (tile < tri) {
      tm = (int)((sqrt(8.0 * (double)tile + 1.0) - 1.0) * 0.5);
      while ((unsigned)(tm + 1) * (unsigned)(tm + 2) / 2 <= tile) tm++;
      while ((unsigned)tm * (unsigned)(tm + 1) / 2 > tile) tm--;
      tn = (int)(tile - (unsigned)tm * (unsigned)(tm + 1) / 2);
    } else {
      const unsigned t2 = tile - tri;
      tm = g.tiles_n + (int)(t2 / g.tiles_n); tn = (int)(t2 % g.tiles_n);
    }
  }

  const size_t row0 = (size_t)tm * GT_BM, col0 = (size_t)tn * GT_BN;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;

  const bool vecA = ((g.lda & 1) == 0) && ((((uintptr_t)g.A) & 15) == 0);
  const bool vecB = ((g.ldb & 1) == 0) && ((((uintptr_t)g.B) & 15) == 0);

  double4_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc[i][j] = (double4_t){0.0, 0.0, 0.0, 0.0};

  double2 ra[4], rb[4];

  auto fetch = [&](size_t k0) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int c = tid + 256 * i;
      if (FULL) {   /* whole tiles, 16-byte aligned operands: no predicates */
        { const int rr = c >> 3, kc = (c & 7) * 2;
          ra[i] = *reinterpret_cast<const double2 *>(g.A + (row0 + rr) * g.lda + k0 + kc); }
        if (B_IS_KN) { const int kk = c >> 6, nc = (c & 63) * 2;
          rb[i] = *reinterpret_cast<const double2 *>(g.B + (k0 + kk) * g.ldb + col0 + nc); }
        else { const int rr = c >> 3, kc = (c & 7) * 2;
          rb[i] = *reinterpret_cast<const double2 *>(g.B + (col0 + rr) * g.ldb + k0 + kc); }
        continue;
      }
      { /* A: 128 rows x 8 chunks of 2 */
        const int rr = c >> 3, kc = (c & 7) * 2;
        const size_t grow = row0 + rr, gk = k0 + kc;
        const bool okr = grow < g.m;
        ra[i] = ld2(g.A + grow * g.lda + gk, okr && gk < g.k, okr && gk + 1 < g.k, vecA);
      }
      if (B_IS_KN) { /* B[k][n]: 16 rows x 64 chunks of 2 */
        const int kk = c >> 6, nc = (c & 63) * 2;
        const size_t gk = k0 + kk, gcol = col0 + nc;
        const bool okk = gk < g.k;
        rb[i] = ld2(g.B + gk * g.ldb + gcol, okk && gcol < g.n, okk && gcol + 1 < g.n, vecB);
      } else { /* B[n][k]: 128 rows x 8 chunks of 2 */
        const int rr = c >> 3, kc = (c & 7) * 2;
        const size_t gn = col0 + rr, gk = k0 + kc;
        const bool okn = gn < g.n;
        rb[i] = ld2(g.B + gn * g.ldb + gk, okn && gk < g.k, okn && gk + 1 < g.k, vecB);
      }
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int c = tid + 256 * i;
      { const int rr = c >> 3, kc = (c & 7) * 2;
        *reinterpret_cast<double2 *>(&sA[buf][rr * GT_LDA + kc]) = ra[i]; }
      if (B_IS_KN) { const int kk = c >> 6, nc = (c & 63) * 2;
        *reinterpret_cast<double2 *>(&sB[buf][kk * GT_LDBN + nc]) = rb[i]; }
      else { const int rr = c >> 3, kc = (c & 7) * 2;
        *reinterpret_cast<double2 *>(&sB[buf][rr * GT_LDA + kc]) = rb[i]; }
    }
  };

  const size_t nsteps = (g.k + GT_BK - 1) / GT_BK;
  fetch(0);
  stash(0);
  __syncthreads();

  for (size_t s = 0; s < nsteps; s++) {
    const int buf = (int)(s & 1);
    if (s + 1 < nsteps) fetch((s + 1) * GT_BK);   /* in flight under the MFMAs */
    const double *a_base = &sA[buf][(wr * 64 + fr) * GT_LDA + fq];
    const double *b_base = B_IS_KN ? &sB[buf][fq * GT_LDBN + wc * 64 + fr] : &sB[buf][(wc * 64 + fr) * GT_LDA + fq];
#pragma unroll
    for (int kk = 0; kk < GT_BK / 4; kk++) {
      double af[4], bf[4];
#pragma unroll
      for (int i = 0; i < 4; i++) af[i] = a_base[i * 16 * GT_LDA + kk * 4];
#pragma unroll
      for (int j = 0; j < 4; j++) bf[j] = B_IS_KN ? b_base[kk * 4 * GT_LDBN + j * 16] : b_base[j * 16 * GT_LDA + kk * 4];
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++)
          acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
    if (s + 1 < nsteps) stash(buf ^ 1);           /* other buffer: last read before the previous barrier */
    __syncthreads();
  }

  /* epilogue: C -= acc.  D[row=(lane>>4)+4*reg][col=lane&15] */
#pragma unroll
  for (int i = 0; i < 4; i++) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const size_t gcol = col0 + wc * 64 + j * 16 + fr;
#pragma unroll
      for (int rg = 0; rg < 4; rg++) {
        const size_t grow = row0 + wr * 64 + i * 16 + fq + 4 * rg;
        if ((FULL || (grow < g.m && gcol < g.n)) && (!g.lower_only || gcol <= grow)) {
          double *p = g.C + grow * g.ldc + gcol;
          *p = *p - acc[i][j][rg];
        }
      }
    }
  }
}


/* ------------------------------------------------------------------------ */
/* Full-tile NT variant with direct-to-LDS loads (global_load_lds_dwordx4) and a 3-stage ring:
   the operand tiles of K-steps s+1 and s+2 are in flight while step s feeds the MFMAs, no VGPR
   staging, no ds_write pass, one raw s_barrier + one counted vmcnt wait per K-step.
   LDS image per stage and operand: 128 rows x 16 doubles, unpadded (a DMA wave-instruction writes
   1 KiB linearly = 8 rows), 16-byte slot index XOR-swizzled with (row>>1)&7 -- applied to the
   per-lane SOURCE address of the DMA and to the fragment read, so the (row = lane&15,
   k = lane>>4) ds_read_b64 stays bank-conflict free.  DM_STAGES (gemm_plan.h) is the ring depth. */

__device__ __forceinline__ void dma16(const double *gsrc, double *ldst)
{
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)gsrc,
                                   (__attribute__((address_space(3))) void *)ldst, 16, 0, 0);
}

/* WR = wave rows: 2 -> 128x128 tile, 4 waves, 1 wave/SIMD;  4 -> 256x128 tile, 8 waves, 2 waves/SIMD
   (a wave's DMA issue / wait gaps are then covered by its SIMD partner's MFMAs). */
template <int WR>
__global__ void __launch_bounds__(128 * WR, 1)
gemm_minus_dma_nt_kernel(GemmArgs g)
{
  constexpr int BM = 64 * WR;
  constexpr int NW = 2 * WR;                           /* waves */
  constexpr int A_TILE = BM * GT_BK, B_TILE = GT_BN * GT_BK;
  constexpr int A_CH = BM / 8 / NW, B_CH = (GT_BN / 8) / NW;   /* 1-KiB chunks per wave: 4,4 or 4,2 */
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double *sA = smem;                                   /* [DM_STAGES][A_TILE] */
  double *sB = smem + DM_STAGES * A_TILE;

  const unsigned nwg = gridDim.x, bid = blockIdx.x;
  const unsigned q = nwg / 8, r = nwg % 8, xcd = bid % 8;
  const unsigned tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + bid / 8;
  int tm, tn;
  if (!g.lower_only) {
    tm = (int)(tile / g.tiles_n); tn = (int)(tile % g.tiles_n);
  } else {
    /* row tm of tiles holds min(R*(tm+1), tiles_n) active tiles, R = BM/128 */
    constexpr unsigned R = BM / GT_BN;
    const unsigned full_rows = (unsigned)g.tiles_n / R;             /* rows of the triangular part */
    const unsigned tri = R * full_rows * (full_rows + 1) / 2;
    if (tile < tri) {
      const double t = (double)tile / (double)R;
      tm = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
      while (R * (unsigned)(tm + 1) * (unsigned)(tm + 2) / 2 <= tile) tm++;
      while (R * (unsigned)tm * (unsigned)(tm + 1) / 2 > tile) tm--;
      tn = (int)(tile - R * (unsigned)tm * (unsigned)(tm + 1) / 2);
    } else {
      const unsigned t2 = tile - tri;
      tm = (int)full_rows + (int)(t2 / g.tiles_n); tn = (int)(t2 % g.tiles_n);
    }
  }
  const size_t row0 = (size_t)tm * BM, col0 = (size_t)tn * GT_BN;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;

  /* DMA source addresses of this lane */
  const double *srcA[A_CH], *srcB[B_CH];
#pragma unroll
  for (int i = 0; i < A_CH; i++) {
    const int rr = (wave * A_CH + i) * 8 + (lane >> 3);
    srcA[i] = g.A + (row0 + rr) * g.lda + (((lane & 7) ^ ((rr >> 1) & 7)) << 1);
  }
#pragma unroll
  for (int i = 0; i < B_CH; i++) {
    const int rr = (wave * B_CH + i) * 8 + (lane >> 3);
    srcB[i] = g.B + (col0 + rr) * g.ldb + (((lane & 7) ^ ((rr >> 1) & 7)) << 1);
  }
  auto issue = [&](int stage, size_t k0) {
#pragma unroll
    for (int i = 0; i < A_CH; i++) dma16(srcA[i] + k0, sA + stage * A_TILE + (wave * A_CH + i) * 128);
#pragma unroll
    for (int i = 0; i < B_CH; i++) dma16(srcB[i] + k0, sB + stage * B_TILE + (wave * B_CH + i) * 128);
  };

  /* fragment read offsets (doubles) within a stage: row*16 + ((slot ^ sw)*2 + (k&1)) */
  const int sw = (fr >> 1) & 7;
  int koff[4];
#pragma unroll
  for (int kk = 0; kk < 4; kk++) koff[kk] = (((kk * 2 + (fq >> 1)) ^ sw) << 1) + (fq & 1);
  const int arow = (wr * 64 + fr) * GT_BK, brow = (wc * 64 + fr) * GT_BK;

  double4_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc[i][j] = (double4_t){0.0, 0.0, 0.0, 0.0};

  const size_t nsteps = g.k / GT_BK;
  issue(0, 0);
  if (nsteps > 1) issue(1, GT_BK);

  for (size_t s = 0; s < nsteps; s++) {
    /* stage s has landed once at most the DMAs of stage s+1 are still outstanding */
    if (s + 1 < nsteps) {
      if (A_CH + B_CH == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    } else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (s + 2 < nsteps) issue((int)((s + 2) % DM_STAGES), (s + 2) * GT_BK);   /* ring slot read at step s-1 */
    const double *a_base = sA + (s % DM_STAGES) * A_TILE + arow;
    const double *b_base = sB + (s % DM_STAGES) * B_TILE + brow;
#pragma unroll
    for (int kk = 0; kk < 4; kk++) {
      double af[4], bf[4];
#pragma unroll
      for (int i = 0; i < 4; i++) af[i] = a_base[i * 16 * GT_BK + koff[kk]];
#pragma unroll
      for (int j = 0; j < 4; j++) bf[j] = b_base[j * 16 * GT_BK + koff[kk]];
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++)
          acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
  }

#pragma unroll
  for (int i = 0; i < 4; i++) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const size_t gcol = col0 + wc * 64 + j * 16 + fr;
#pragma unroll
      for (int rg = 0; rg < 4; rg++) {
        const size_t grow = row0 + wr * 64 + i * 16 + fq + 4 * rg;
        if (!g.lower_only || gcol <= grow) {
          double *p = g.C + grow * g.ldc + gcol;
          *p = *p - acc[i][j][rg];
        }
      }
    }
  }
}

/* ------------------------------------------------------------------------ */
/* Stream-K form of the DMA kernel.  With one workgroup per tile the launch time is quantised in
   whole tiles per CU: 8192^2 lower / 256x128 tiles = 1056 tiles = 4.1 rounds on 256 CUs (a fifth,
   almost empty round costs 20 %), 2048^2 lower = 136 tiles of 128x128 leaves 120 CUs idle.  Here
   the launch is G persistent workgroups (G <= #CUs) and the unit of work is one K-step of one
   tile: workgroup w owns the contiguous range [total*w/G, total*(w+1)/G) of the (tile, K-step)
   space, so every CU gets the same number of MFMA steps whatever the tile count.
   A tile whose K range is cut is finished by the workgroup holding its FIRST K-step (the owner);
   the others store their accumulators to their private slot and raise a flag.  A non-owner
   segment is always the first thing its workgroup does, so the owner (which reaches the tile
   last) finds the flags already set and never waits on a workgroup that itself waits.  Partials
   are added in ascending workgroup order: the summation order is a pure function of the shape,
   results are reproducible run to run.
   Partials and flags are exchanged with agent-scope atomic loads/stores (sc1: coherent across
   the 8 XCD L2s) and an explicit vmcnt(0) + barrier before the flag, so no L2 writeback /
   invalidate is needed.  The owner clears the flag it consumed: launches on one stream are
   serialised, so the buffers are reusable by the next launch (and by a hipGraph replay). */
#ifdef SINTERP_DIAG_PROF
/* per workgroup: s_memtime at start / end, the summed cycles of the four phases of its segments (prologue until
   the first MFMA, K loop, partial publish or fix-up wait, C epilogue), s_memrealtime at start / end (tools/gemm_phases.py) */
__device__ unsigned long long g_gemm_ts[1024 * 8];
extern "C" int gsl_sinterp_hip_debug_gemm_ts(unsigned long long *out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_gemm_ts), sizeof(g_gemm_ts)); }
extern "C" int gsl_sinterp_hip_debug_gemm_ts_clear(void)
{
  static const unsigned long long zero[1024 * 8] = {0};
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_gemm_ts), zero, sizeof(g_gemm_ts));
}
__device__ __forceinline__ unsigned long long gemm_stamp()
{
  unsigned long long t;
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
  __builtin_amdgcn_sched_barrier(0);
  return t;
}
__device__ __forceinline__ unsigned long long gemm_rstamp()
{
  unsigned long long t;
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
  __builtin_amdgcn_sched_barrier(0);
  return t;
}
#define GEMM_TS_INIT() unsigned long long ph_[4] = {0, 0, 0, 0}, ts_ = 0; const unsigned long long t0_ = gemm_stamp(), r0_ = gemm_rstamp()
#define GEMM_TS_BEGIN() (ts_ = gemm_stamp())
#define GEMM_TS_MARK(slot) do { const unsigned long long t_ = gemm_stamp(); ph_[slot] += t_ - ts_; ts_ = t_; } while (0)
/* unconditional stamp whose interval goes to slot a when `cond` (wave-uniform), else to slot b: a stamp inside a
   branch of the non-pipelined K loop, or a condition the compiler takes for divergent, makes the gfx950 backend fail
   with "illegal VGPR to SGPR copy" */
#define GEMM_TS_MARK_SEL(cond, a, b) do { const unsigned long long t_ = gemm_stamp(), d_ = t_ - ts_; const bool c_ = (cond); \
    ph_[a] += c_ ? d_ : 0ull; ph_[b] += c_ ? 0ull : d_; ts_ = t_; } while (0)
#define GEMM_TS_FINISH() do { const unsigned long long t1_ = gemm_stamp(), r1_ = gemm_rstamp(); \
    if (threadIdx.x == 0 && blockIdx.x < 1024) { unsigned long long *o_ = g_gemm_ts + blockIdx.x * 8; \
      o_[0] = t0_; o_[1] = t1_; o_[2] = ph_[0]; o_[3] = ph_[1]; o_[4] = ph_[2]; o_[5] = ph_[3]; o_[6] = r0_; o_[7] = r1_; } } while (0)
#else
#define GEMM_TS_INIT() do { } while (0)
#define GEMM_TS_BEGIN() do { } while (0)
#define GEMM_TS_MARK(slot) do { } while (0)
#define GEMM_TS_MARK_SEL(cond, a, b) do { } while (0)
#define GEMM_TS_FINISH() do { } while (0)
#endif

struct StreamK {
  unsigned steps;               /* K-steps per tile */
  unsigned total;               /* tiles * steps */
  unsigned base, rem;           /* total = G*base + rem: workgroup w starts at w*base + min(w, rem) */
  unsigned dp_rounds;           /* whole tiles first: round r gives tile r*G + w to workgroup w; the (tile, K-step) space
                                   of total/steps tiles AFTER those dp_rounds*G tiles is then split as above */
  double *partial;              /* [G][BM*128] */
  unsigned *flags;              /* [G] */
  /* RIDER launches of one round only (dp_rounds = 0): the first pri_tiles tiles -- those that cover the block the rider waits
     for -- are taken out of the (tile, K-step) space above and cut into pri_nsl K-slices of pri_sl steps each; workgroup w <
     pri_tiles * pri_nsl computes slice w % pri_nsl of tile w / pri_nsl FIRST, and its range of the remaining space is shorter
     by pri_sl steps.  The holder of a tile's slice 0 adds the other slices in ascending order and stores the tile: it is
     complete after about pri_sl steps plus the exchange instead of at the end of the launch. */
  unsigned pri_tiles, pri_sl, pri_nsl;
  unsigned pri_base;            /* the slices' partials and flags: slot / flag pri_base + w behind the G regular ones (a workgroup
                                   may hold a slice AND an open partial of its range); one word, the K loop is short of SGPRs */
};

/* the rider workgroup of a Cholesky trailing update (sinterp_rider, common.h) */
struct RiderArgs {
  int *info; size_t j0; double *dinv; double *fb; size_t ldf; int nrhs;
  unsigned *counter, *abort_word;
  unsigned need;                /* covering tiles: tile 0 (256x128, 128x128), tiles 0..2 (64x64) */
};
#define RIDER_MAX_POLLS (1u << 22)   /* x (>= 0.5 us sleep + one L2 miss): seconds, the longest update takes milliseconds */

/* Launched as the LAST workgroup of the update (all owners are resident before it).  One lane polls the panel's counter
   relaxed, then ONE agent-scope acquire; the owners stored the block write-through and drained before they counted, so the
   plain (vector) loads of chol_diag128_block see the updated block.  No owner ever waits for the rider.  The poll is
   bounded: on time-out the rider sets the abort word and leaves, the driver reports GSL_EFAILED. */
template <int NW>
__device__ __forceinline__ void gemm_rider(const GemmArgs &g, const RiderArgs &rd, double *smem)
{
  const int tid = threadIdx.x;
  unsigned *okw = reinterpret_cast<unsigned *>(smem + DIAG128_LDS_BYTES / sizeof(double));
  if (tid == 0) {
    unsigned ok = 0;
    for (unsigned spins = 0; spins < RIDER_MAX_POLLS; spins++) {
      if (__hip_atomic_load(rd.counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= rd.need) { ok = 1; break; }
      __builtin_amdgcn_s_sleep(32);
    }
    if (ok) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    else __hip_atomic_store(rd.abort_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *okw = ok;
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __syncthreads();
  if (*okw == 0) return;
  chol_diag128_block<NW>(smem, g.C, g.ldc, rd.j0, rd.info, (double *)nullptr, rd.dinv, rd.fb, rd.ldf, rd.nrhs, tid);
}

template <int BM, int BN>
__device__ __forceinline__ void decode_tile(const GemmArgs &g, unsigned tile, int &tm, int &tn)
{
  if (!g.lower_only) {
    tm = (int)(tile / g.tiles_n); tn = (int)(tile % g.tiles_n);
  } else {
    constexpr unsigned R = BM / BN;
    const unsigned full_rows = (unsigned)g.tiles_n / R;
    const unsigned tri = R * full_rows * (full_rows + 1) / 2;
    if (tile < tri) {
      const double t = (double)tile / (double)R;
      tm = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
      while (R * (unsigned)(tm + 1) * (unsigned)(tm + 2) / 2 <= tile) tm++;
      while (R * (unsigned)tm * (unsigned)(tm + 1) / 2 > tile) tm--;
      tn = (int)(tile - R * (unsigned)tm * (unsigned)(tm + 1) / 2);
    } else {
      const unsigned t2 = tile - tri;
      tm = (int)full_rows + (int)(t2 / g.tiles_n); tn = (int)(t2 % g.tiles_n);
    }
  }
}

/* Tile configurations (block tile BM x BN, wave tile WM x WN):
     256x128 / 64x64, 8 waves, 144 KiB LDS -- large updates, 2 waves per SIMD;
     128x128 / 64x32, 8 waves,  96 KiB     -- mid-size updates (K = 512 .. 2048 levels of the recursions), 2 waves per SIMD;
      64x64  / 32x16, 8 waves, 128 KiB     -- updates with few 128-tiles (the K <= 512 levels): 4x the workgroups, a
                                             128-wide panel update is otherwise one 13.7 us tile per CU on a fraction
                                             of the CUs; 4-step groups (below), 2 waves per SIMD;
     128x128 / 64x64 and 64x64 / 32x32 on 4 waves (one per SIMD): the round-4 dispatch (GSL_SINTERP_GEMM_RULE_R4=1).
   With one wave per SIMD the matrix pipe idles through every LDS round trip, barrier and DMA wait of that wave;
   the second wave of the 8-wave tiles covers them (K = 256 level of C3: 1.39 -> 1.11 ms). */
/* SS consecutive 16-wide K sub-steps form one "group" = the unit between two barriers (and the unit of the
   stream-K split); ST groups are resident in the LDS ring.  SS = 1, ST = 3 is the pipeline described above.
   The small 64x64 tile spends only 0.43 us of MFMA work per 16-wide step -- less than a DMA round trip and
   comparable to a barrier -- so it runs SS = 4, ST = 2 (128 KiB): a K = 128 update has its WHOLE operand
   panel in flight from the first instruction and crosses two barriers instead of eight. */
/* PIPE (ST = 3, SS = 1 only): the K loop is software-pipelined ACROSS its barrier.  In the plain loop every wave
   meets at the barrier with an empty MFMA queue and must then wait out an LDS round trip before its first
   MFMA of the new step: a bubble of a few hundred cycles per 8192-cycle step on every SIMD.  Here the last
   quarter of a step's MFMAs (its fragments are already in registers) is issued AFTER the barrier and after the
   first fragment loads of the next step, so the matrix pipe stays fed through the rendezvous; the barrier also
   moves one quarter-step earlier relative to the DMA ring, which now runs three steps ahead instead of two. */
/* BKN: the B operand is stored [k][n] (C -= A B, the N.N updates of the LU route) instead of [n][k].  Its LDS image per
   step is then 16 k-rows of BN doubles, each row one linear 1-KiB DMA wave-instruction (BN = 128), rows pitched
   BN + 16 doubles apart so that the (k = lane>>4, n = lane&15) fragment read -- 16 consecutive doubles per k-row,
   k-rows 32 banks apart -- is conflict-free; no swizzle needed. */
/* RIDER: the launch has one workgroup more than the G that share the update; it factors the next panel's diagonal block
   (gemm_rider).  The owners of the tiles that cover that block store them write-through and count in.  Instantiated for the
   two 8-wave N.T configurations the dispatch rule ships below the 256x128 tile. */
template <int BM, int BN, int WM, int WN, int SS = 1, int ST = DM_STAGES, bool PIPE = false, bool BKN = false, bool RIDER = false>
__global__ void __launch_bounds__((BM / WM) * (BN / WN) * 64)
gemm_minus_streamk_kernel(GemmArgs g, StreamK x, RiderArgs rd)
{
  static_assert(ST == 3 || ST == 2, "ring depth");
  static_assert(!PIPE || (ST == 3 && SS == 1), "pipelined loop: three-deep ring of single steps");
  static_assert(!BKN || BN == 128, "k-row = one 1-KiB DMA instruction");
  constexpr int WCOLS = BN / WN;                        /* waves along n */
  constexpr int NW = (BM / WM) * WCOLS;
  constexpr int NT = NW * 64;                           /* threads */
  constexpr int FM = WM / 16, FN = WN / 16;             /* MFMA fragments per wave */
  constexpr int BPITCH = BN + 16;                       /* BKN: doubles between the k-rows of the B image */
  constexpr int A_TILE = BM * GT_BK, B_TILE = BKN ? GT_BK * BPITCH : BN * GT_BK;
  constexpr int A_CH = BM / 8 / NW, B_CH = (BN / 8) / NW;
  static_assert(A_CH >= 1 && B_CH >= 1 && A_CH * 8 * NW == BM && B_CH * 8 * NW == BN, "tile / wave split");
  constexpr int PER_GROUP = SS * (A_CH + B_CH);         /* DMA wave-instructions a wave issues per group */
  static_assert(PER_GROUP <= 32, "vmcnt immediate");
  constexpr size_t GK = (size_t)GT_BK * SS;             /* K extent of a group */
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double *sA = smem;
  double *sB = smem + ST * SS * A_TILE;

  /* not the 256x128 tile: its K loop runs at 256 VGPRs with 44 bytes of scratch already, the hand-off code made that 48 to 68 */
  static_assert(!RIDER || (!BKN && NW == 8 && BM <= 128), "rider: N.T updates on 8 waves");
  if constexpr (RIDER) {
    if (blockIdx.x == gridDim.x - 1) { gemm_rider<NW>(g, rd, smem); return; }
  }
  const unsigned G = gridDim.x - (RIDER ? 1u : 0u), bid = blockIdx.x;
  const unsigned q = G / 8, r = G % 8, xcd = bid % 8;
  const unsigned gl = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + bid / 8;   /* XCD-contiguous ranges */
  constexpr bool PRI = RIDER;
  constexpr unsigned PRI_SLOT_SCALE = (256 * GT_BN) / (BM * BN);   /* pri_base counts slots of 256 x 128 doubles */
  const unsigned pri_wgs = PRI ? x.pri_tiles * x.pri_nsl : 0u;   /* holders of a priority K-slice */
  auto start_of = [&](unsigned w) -> unsigned {
    const unsigned v = w * x.base + (w < x.rem ? w : x.rem);
    if constexpr (PRI) return v - (w < pri_wgs ? w : pri_wgs) * x.pri_sl;
    return v;
  };
  auto start_cap = [&](unsigned w) -> unsigned { const unsigned v = start_of(w); return v < x.total ? v : x.total; };
  unsigned it = __builtin_amdgcn_readfirstlane(start_cap(gl));
  const unsigned it_end = __builtin_amdgcn_readfirstlane(start_cap(gl + 1));
  unsigned tile = __builtin_amdgcn_readfirstlane(it / x.steps);
  const unsigned dp_tiles = x.dp_rounds * G;
  unsigned round = 0;
  bool pri_pending = PRI && gl < pri_wgs;
  GEMM_TS_INIT();

  /* Whole-tile rounds first: the 32 workgroups of an XCD hold 32 consecutive tiles of the same round and
     walk K more or less in step, so operand panels are shared in their L2; then the stream-K remainder. */
  for (;;) {
    const bool dp = round < x.dp_rounds;
    const bool pr = PRI && pri_pending;                /* this workgroup's K-slice of a priority tile (never with dp rounds) */
    if (!dp && !pr && it >= it_end) break;
    const unsigned tile_first = (dp || pr) ? 0u : tile * x.steps, tile_end = tile_first + x.steps;
    unsigned s0 = dp ? 0u : it - tile_first;
    unsigned s1 = dp ? x.steps : (it_end < tile_end ? it_end - tile_first : x.steps);
    unsigned gtile = dp ? round * G + gl : dp_tiles + tile;
    if constexpr (PRI) {
      if (pr) { s0 = (gl % x.pri_nsl) * x.pri_sl; s1 = s0 + x.pri_sl; gtile = gl / x.pri_nsl; }
      else if (!dp) gtile += x.pri_tiles;
    }
    const bool hand = RIDER && gtile < rd.need;          /* a tile the rider waits for */
    int tm, tn;
    decode_tile<BM, BN>(g, gtile, tm, tn);
    const size_t row0 = (size_t)tm * BM, col0 = (size_t)tn * BN;
    GEMM_TS_BEGIN();

    double4_t acc[FM][FN];
    /* Tiles with at most 8 fragments per wave (64 x 64, and 128 x 128 on 8 waves): the owner fetches its C tile during
       its LAST K-step -- 8 to 32 values per thread, issued after the ring's final DMA wait, so no hand-counted vmcnt
       follows them, and in flight under that step's MFMAs -- and the epilogue is a plain store instead of a
       read-modify-write whose load latency nothing covers.  Same arithmetic: whole tiles keep their bits.
       Like every kernel here it relies on the caller having ordered the producer of C before the call on the
       context's stream; where in the launch C is read does not make an unordered writer safe. */
    constexpr bool CPRE = FM * FN <= 8;
    /* Larger wave tiles (64 x 64: no spare registers for a prefetch), N.T operands: the owner's accumulators START as the
       C tile and every K-step subtracts from it, as in gemm_minus_smallk_kernel; the epilogue is a plain store, no
       load and no subtract, whose drain overlaps the next segment's set-up.  The arithmetic is
       ((C - a1 b1) - a2 b2) ... - partials in ascending workgroup order, where it was C - (sum of all of them).
       The [k][n] instantiations keep the read-modify-write epilogue and their bits (the LU pivot sequences). */
    constexpr bool CACC = !CPRE && !BKN;
    static_assert(!(CACC && RIDER), "the rider's hand-off stores come from the prefetched-C epilogue");
    double4_t cpre[CPRE ? FM : 1][CPRE ? FN : 1];
    auto load_cpre = [&]() {
      if constexpr (CPRE) {
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        const int lane = tid & 63, wave = tid >> 6;
        const int wr = wave / WCOLS, wc = wave % WCOLS;
        const int fr = lane & 15, fq = lane >> 4;
#pragma unroll
        for (int i = 0; i < FM; i++)
#pragma unroll
          for (int j = 0; j < FN; j++)
#pragma unroll
            for (int rg = 0; rg < 4; rg++)
              cpre[i][j][rg] = g.C[(row0 + wr * WM + i * 16 + fq + 4 * rg) * g.ldc + col0 + wc * WN + j * 16 + fr];
      }
    };
    {
      /* Everything lane-dependent is derived from a laundered thread id INSIDE the segment: left to
         itself the compiler hoists it all out of the while loop, runs out of VGPRs (the 8-wave
         variant has 256 including the 128 accumulators) and spills operands of the K loop -- and
         a scratch reload's s_waitcnt vmcnt(0) also drains the DMA ring. */
      int tid = threadIdx.x;
      asm volatile("" : "+v"(tid));
      const int lane = tid & 63, wave = tid >> 6;
      const int wr = wave / WCOLS, wc = wave % WCOLS;
      const int fr = lane & 15, fq = lane >> 4;
      const int sw = (fr >> 1) & 7;
      int koff[4];
#pragma unroll
      for (int kk = 0; kk < 4; kk++) koff[kk] = (((kk * 2 + (fq >> 1)) ^ sw) << 1) + (fq & 1);
      const int arow = (wr * WM + fr) * GT_BK, brow = BKN ? fq * BPITCH + wc * WN + fr : (wc * WN + fr) * GT_BK;

      const double *srcA[A_CH], *srcB[B_CH];
#pragma unroll
      for (int i = 0; i < A_CH; i++) {
        const int rr = (wave * A_CH + i) * 8 + (lane >> 3);
        srcA[i] = g.A + (row0 + rr) * g.lda + (((lane & 7) ^ ((rr >> 1) & 7)) << 1);
      }
#pragma unroll
      for (int i = 0; i < B_CH; i++) {
        const int rr = (wave * B_CH + i) * 8 + (lane >> 3);
        if constexpr (BKN) srcB[i] = g.B + (size_t)(wave * B_CH + i) * g.ldb + col0 + lane * 2;   /* chunk = k-row of the step */
        else srcB[i] = g.B + (col0 + rr) * g.ldb + (((lane & 7) ^ ((rr >> 1) & 7)) << 1);
      }
      /* one group = SS sub-steps, each its own [rows][16] swizzled image (slot = stage * SS + sub-step) */
      auto issue = [&](int stage, size_t k0) {
#pragma unroll
        for (int ss = 0; ss < SS; ss++) {
#pragma unroll
          for (int i = 0; i < A_CH; i++) dma16(srcA[i] + k0 + ss * GT_BK, sA + (stage * SS + ss) * A_TILE + (wave * A_CH + i) * 128);
#pragma unroll
          for (int i = 0; i < B_CH; i++) {
            if constexpr (BKN) dma16(srcB[i] + (k0 + ss * GT_BK) * g.ldb, sB + (stage * SS + ss) * B_TILE + (wave * B_CH + i) * BPITCH);
            else dma16(srcB[i] + k0 + ss * GT_BK, sB + (stage * SS + ss) * B_TILE + (wave * B_CH + i) * 128);
          }
        }
      };

      if constexpr (!CACC) {
#pragma unroll
        for (int i = 0; i < FM; i++)
#pragma unroll
          for (int j = 0; j < FN; j++) acc[i][j] = (double4_t){0.0, 0.0, 0.0, 0.0};
      } else if (s0 == 0) {
        /* owner: the C tile goes straight into the accumulators, entries above the diagonal included (they feed only
           entries that are never stored).  Issued before the ring's first DMA: older than every DMA group, so each
           counted vmcnt wait of the K loop -- all of which leave only DMA groups outstanding -- covers these loads too,
           and their latency shares the window in which the ring fills.  One lane pointer walks down the 16 row groups:
           64 addresses up front do not fit beside the accumulators (the loop runs at 256 VGPRs) */
        const __attribute__((address_space(1))) double *cl =
            (const __attribute__((address_space(1))) double *)(g.C + (row0 + wr * WM + fq) * g.ldc + col0 + wc * WN + fr);
#pragma unroll
        for (int i = 0; i < FM; i++)
#pragma unroll
          for (int rg = 0; rg < 4; rg++) {
#pragma unroll
            for (int j = 0; j < FN; j++) acc[i][j][rg] = cl[j * 16];
            cl += 4 * g.ldc;
            asm volatile("" : "+v"(cl));
          }
      } else {
        /* -0.0: negate_c() below turns it into the +0.0 these segments have always started from.  Made here, from a
           laundered register: as a loop invariant it would be kept, and spilled, across the segments */
        double z = 0.0;
        asm volatile("" : "+v"(z));
        z = -z;
#pragma unroll
        for (int i = 0; i < FM; i++)
#pragma unroll
          for (int j = 0; j < FN; j++) acc[i][j] = (double4_t){z, z, z, z};
      }
      /* -C in the owner's accumulators: the MFMAs add the products, the epilogue negates once more.  Negation is exact,
         so this is ((C - a1 b1) - a2 b2) ... bit for bit.  Every segment negates, owner or not: one path, so the
         compiler's wait for the loaded values stands exactly once, here, behind the ring's first DMAs and outside the
         K loop.  (It is a vmcnt(0) -- the backend does not count across direct-to-LDS loads in flight -- so the owner
         starts its K loop with all three groups landed instead of the first; they were issued back to back.) */
      auto negate_c = [&]() {
        if constexpr (CACC) {
#pragma unroll
          for (int i = 0; i < FM; i++)
#pragma unroll
            for (int j = 0; j < FN; j++) acc[i][j] = -acc[i][j];
        }
      };

      __syncthreads();                                   /* the ring is free: previous segment fully read */
      if constexpr (PIPE) {
        auto wait_keep = [&](int groups) {               /* all but the last `groups` issued groups have landed */
          static_assert(PER_GROUP == 4 || PER_GROUP == 6 || PER_GROUP == 8, "vmcnt immediate");
          if (groups >= 2) {
            if constexpr (PER_GROUP == 8) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
            else if constexpr (PER_GROUP == 6) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
          } else if (groups == 1) {
            if constexpr (PER_GROUP == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            else if constexpr (PER_GROUP == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
          } else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        };
        auto load_frag = [&](int stage, int kk, double (&af)[FM], double (&bf)[FN]) {
          const double *a_base = sA + stage * A_TILE + arow;
          const double *b_base = sB + stage * B_TILE + brow;
#pragma unroll
          for (int i = 0; i < FM; i++) af[i] = a_base[i * 16 * GT_BK + koff[kk]];
#pragma unroll
          for (int j = 0; j < FN; j++) bf[j] = BKN ? b_base[kk * 4 * BPITCH + j * 16] : b_base[j * 16 * GT_BK + koff[kk]];
        };
        auto mma = [&](const double (&af)[FM], const double (&bf)[FN]) {
#pragma unroll
          for (int i = 0; i < FM; i++)
#pragma unroll
            for (int j = 0; j < FN; j++)
              acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[i], bf[j], acc[i][j], 0, 0, 0);
        };
        const unsigned nst = s1 - s0;
        issue(0, (size_t)s0 * GK);
        if (nst > 1) issue(1, (size_t)(s0 + 1) * GK);
        if (nst > 2) issue(2, (size_t)(s0 + 2) * GK);
        negate_c();
        wait_keep(nst > 2 ? 2 : (int)nst - 1);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        GEMM_TS_MARK(0);
        double af0[FM], bf0[FN], af1[FM], bf1[FN];
        load_frag(0, 0, af0, bf0);
        /* all steps but the last: the rendezvous sits between the third and the fourth quarter of the step */
        for (unsigned rel = 0; rel + 1 < nst; rel++) {
          const int stage = (int)(rel % 3);
          load_frag(stage, 1, af1, bf1);
          mma(af0, bf0);
          load_frag(stage, 2, af0, bf0);
          mma(af1, bf1);
          load_frag(stage, 3, af1, bf1);
          mma(af0, bf0);
          /* (stage, 3) is in af1/bf1; every LDS read of `stage` has returned; stage+1 has landed for this wave once
             only the group issued after it (rel+2, if it exists) is outstanding; after the barrier that holds for
             every wave, and `stage` may be refilled */
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          /* tell the compiler's s_waitcnt pass that af1 / bf1 are settled HERE (it cannot see through the asm wait
             above and would otherwise put a full lgkmcnt(0) between the next step's loads and the deferred MFMAs) */
#pragma unroll
          for (int i = 0; i < FM; i++) asm volatile("" : "+v"(af1[i]));
#pragma unroll
          for (int j = 0; j < FN; j++) asm volatile("" : "+v"(bf1[j]));
          wait_keep(rel + 2 < nst ? 1 : 0);
          __builtin_amdgcn_s_barrier();
          __builtin_amdgcn_sched_barrier(0);
          if (rel + 3 < nst) issue(stage, (size_t)(s0 + rel + 3) * GK);
          load_frag((int)((rel + 1) % 3), 0, af0, bf0);
          __builtin_amdgcn_sched_barrier(0);             /* keep the loads in front of the deferred MFMAs */
          mma(af1, bf1);                                 /* runs while the new fragments fly (counted lgkmcnt: no merge of paths here) */
        }
        if (s0 == 0) load_cpre();                        /* owner: every DMA of the segment has landed, no counted wait follows */
        {
          const int stage = (int)((nst - 1) % 3);
          load_frag(stage, 1, af1, bf1);
          mma(af0, bf0);
          load_frag(stage, 2, af0, bf0);
          mma(af1, bf1);
          load_frag(stage, 3, af1, bf1);
          mma(af0, bf0);
          mma(af1, bf1);
        }
        GEMM_TS_MARK(1);
      } else {
      issue(0, (size_t)s0 * GK);
      if (s0 + 1 < s1) issue(1, (size_t)(s0 + 1) * GK);
      negate_c();
      for (unsigned s = s0; s < s1; s++) {
        const unsigned rel = s - s0;
        /* group s has landed once at most the DMAs of group s+1 are still outstanding */
        if (s + 1 < s1) {
          if constexpr (PER_GROUP == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
          else if constexpr (PER_GROUP == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
          else if constexpr (PER_GROUP == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
          else { static_assert(PER_GROUP == 4 || PER_GROUP == 6 || PER_GROUP == 8 || PER_GROUP == 16, "vmcnt immediate"); asm volatile("s_waitcnt vmcnt(16)" ::: "memory"); }
        } else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        GEMM_TS_MARK_SEL(__builtin_amdgcn_readfirstlane(s) == __builtin_amdgcn_readfirstlane(s0), 0, 1);   /* first group landed */
        if (s0 == 0 && s + 1 == s1) load_cpre();         /* owner: after the last DMA wait of the segment */
        if constexpr (ST == 3) {
          if (s + 2 < s1) issue((int)((rel + 2) % 3), (size_t)(s + 2) * GK);   /* ring slot read at step s-1 */
        }
        const int stage = (int)(rel % ST);
#pragma unroll
        for (int ss = 0; ss < SS; ss++) {
          const double *a_base = sA + (stage * SS + ss) * A_TILE + arow;
          const double *b_base = sB + (stage * SS + ss) * B_TILE + brow;
#pragma unroll
          for (int kk = 0; kk < 4; kk++) {
            double af[FM], bf[FN];
#pragma unroll
            for (int i = 0; i < FM; i++) af[i] = a_base[i * 16 * GT_BK + koff[kk]];
#pragma unroll
            for (int j = 0; j < FN; j++) bf[j] = BKN ? b_base[kk * 4 * BPITCH + j * 16] : b_base[j * 16 * GT_BK + koff[kk]];
#pragma unroll
            for (int i = 0; i < FM; i++)
#pragma unroll
              for (int j = 0; j < FN; j++)
                acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[i], bf[j], acc[i][j], 0, 0, 0);
          }
        }
        if constexpr (ST == 2) {
          /* two-deep ring: the stage just read is refilled with group s+2 once every wave has left it */
          if (s + 2 < s1) {
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
            issue(stage, (size_t)(s + 2) * GK);
          }
        }
      }
      GEMM_TS_MARK(1);
      }
    }

    /* epilogue: its own laundered copies, so nothing of it is live across the K loop */
    int tid = threadIdx.x;
    size_t row0e = row0, col0e = col0;
    asm volatile("" : "+v"(tid), "+s"(row0e), "+s"(col0e));
    const int lane = tid & 63, wave = tid >> 6;
    const int wr = wave / WCOLS, wc = wave % WCOLS;
    const int fr = lane & 15, fq = lane >> 4;
    if (s0 != 0) {
      /* not the owner: publish the partial tile */
      double *pp = x.partial + (size_t)(gl + (pr ? x.pri_base * PRI_SLOT_SCALE : 0u)) * (BM * BN) + tid;
#pragma unroll
      for (int i = 0; i < FM; i++) {
#pragma unroll
        for (int j = 0; j < FN; j++)
#pragma unroll
          for (int rg = 0; rg < 4; rg++)
            __hip_atomic_store(pp + ((i * FN + j) * 4 + rg) * NT, acc[i][j][rg], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_sched_barrier(0);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (tid == 0) __hip_atomic_store(x.flags + gl + (pr ? x.pri_base : 0u), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      GEMM_TS_MARK(2);
    } else {
      if (s1 < x.steps) {
        unsigned *const fl = x.flags + (pr ? x.pri_base : 0u);
        const double *const pbase = x.partial + (size_t)(pr ? x.pri_base * PRI_SLOT_SCALE : 0u) * (BM * BN);
        for (unsigned w = gl + 1; w < G; w++) {
          if (pr ? w >= gl + x.pri_nsl : start_of(w) >= tile_end) break;
          if (tid == 0)
            while (__hip_atomic_load(fl + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) __builtin_amdgcn_s_sleep(8);
          __syncthreads();
          const double *pp = pbase + (size_t)w * (BM * BN) + tid;
#pragma unroll
          for (int i = 0; i < FM; i++) {
#pragma unroll
            for (int j = 0; j < FN; j++)
#pragma unroll
              for (int rg = 0; rg < 4; rg++)
                acc[i][j][rg] += __hip_atomic_load(pp + ((i * FN + j) * 4 + rg) * NT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __builtin_amdgcn_sched_barrier(0);            /* 16 loads in flight at a time */
          }
          if (tid == 0) __hip_atomic_store(fl + w, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
      GEMM_TS_MARK(2);
#pragma unroll
      for (int i = 0; i < FM; i++) {
#pragma unroll
        for (int j = 0; j < FN; j++) {
          const size_t gcol = col0e + wc * WN + j * 16 + fr;
#pragma unroll
          for (int rg = 0; rg < 4; rg++) {
            const size_t grow = row0e + wr * WM + i * 16 + fq + 4 * rg;
            if (!g.lower_only || gcol <= grow) {
              double *p = g.C + grow * g.ldc + gcol;
              double v;
              if constexpr (CPRE) v = cpre[i][j][rg] - acc[i][j][rg];
              else if constexpr (CACC) v = -acc[i][j][rg];
              else v = *p - acc[i][j][rg];
              if (hand) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   /* write-through: read by the rider */
              else *p = v;
            }
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      if constexpr (RIDER) {
        if (hand) {
          /* every storing wave drains, then one lane counts the tile in (cdna_hip_programming.md, Guideline 16) */
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          __syncthreads();
          if (tid == 0) __hip_atomic_fetch_add(rd.counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
#ifdef SINTERP_DIAG_PROF
      if constexpr (!CACC) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   /* CACC: the drain is stamped where the shipped kernel pays it, in the next prologue */
      GEMM_TS_MARK(3);
#endif
    }
    if (dp) round++;
    else if (pr) pri_pending = false;
    else { it = tile_first + s1; tile++; }
  }
  GEMM_TS_FINISH();
}

int sinterp_streamk_prepare(gsl_sinterp_hip_ctx *ctx)
{
  if (ctx->sk_wgs) return ST_SUCCESS;
  if (SINTERP_ENV_ONCE("GSL_SINTERP_NO_STREAMK")) return ST_SUCCESS;
  int cus = 0;
  HIP_OK(ctx, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
  if (cus <= 0) return ST_SUCCESS;
  /* one slot per workgroup + SK_PRI_SLOTS slots for the K-slices of priority tiles (rider launches) */
  HIP_OK(ctx, hipMalloc((void **)&ctx->d_sk_partial, (size_t)(cus + SK_PRI_SLOTS) * 256 * GT_BN * sizeof(double)));
  HIP_OK(ctx, hipMalloc((void **)&ctx->d_sk_flags, (size_t)cus * 2 * sizeof(unsigned)));   /* second half: flags of the priority K-slices */
  HIP_OK(ctx, hipMemset(ctx->d_sk_flags, 0, (size_t)cus * 2 * sizeof(unsigned)));
  HIP_OK(ctx, hipDeviceSynchronize());
  ctx->sk_wgs = cus;
  return ST_SUCCESS;
}

/* ------------------------------------------------------------------------ */
/* Small-K, skinny-N update (the K = 32 / 64 levels of the recursions): C[m x BN] -= A[m x K] B^T,
   B stored [BN][K], K <= 64.  Everything a workgroup needs -- its 128 x K slice of A, all of B and
   its C tile -- is fetched in ONE global round trip; the A slice is negated on its way into LDS
   and the accumulators start as C, so the epilogue is a plain store. */
template <int BN>
__global__ void __launch_bounds__(256)
gemm_minus_smallk_kernel(GemmArgs g)
{
  constexpr int NF = BN / 16;                  /* n fragments per wave */
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int K = (int)g.k, LD = K + 2;
  double *sA = smem;                           /* [128][LD] */
  double *sB = smem + 128 * LD;                /* [BN][LD]  */
  const size_t row0 = (size_t)blockIdx.x * 128;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int kch = K / 2;                       /* 16-byte chunks per row */

  /* C tile -> accumulators (row clamped, masked later) */
  double4_t acc[2][NF];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < NF; j++) {
      const size_t gcol = j * 16 + fr;
#pragma unroll
      for (int rg = 0; rg < 4; rg++) {
        const size_t grow = row0 + wave * 32 + i * 16 + fq + 4 * rg;
        const size_t rcl = grow < g.m ? grow : g.m - 1;
        acc[i][j][rg] = g.C[rcl * g.ldc + gcol];
      }
    }
  /* operands -> LDS */
  for (int c = tid; c < 128 * kch; c += 256) {
    const int rr = c / kch, kc = (c % kch) * 2;
    const size_t grow = row0 + rr, rcl = grow < g.m ? grow : g.m - 1;
    const double2 v = *reinterpret_cast<const double2 *>(g.A + rcl * g.lda + kc);
    *reinterpret_cast<double2 *>(&sA[rr * LD + kc]) = make_double2(-v.x, -v.y);
  }
  for (int c = tid; c < BN * kch; c += 256) {
    const int rr = c / kch, kc = (c % kch) * 2;
    *reinterpret_cast<double2 *>(&sB[rr * LD + kc]) = *reinterpret_cast<const double2 *>(g.B + (size_t)rr * g.ldb + kc);
  }
  __syncthreads();
  const double *a_base = sA + (wave * 32 + fr) * LD + fq;
  const double *b_base = sB + fr * LD + fq;
  for (int kk = 0; kk < K; kk += 4) {
    double af[2], bf[NF];
#pragma unroll
    for (int i = 0; i < 2; i++) af[i] = a_base[i * 16 * LD + kk];
#pragma unroll
    for (int j = 0; j < NF; j++) bf[j] = b_base[j * 16 * LD + kk];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int j = 0; j < NF; j++) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[i], bf[j], acc[i][j], 0, 0, 0);
  }
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < NF; j++) {
      const size_t gcol = j * 16 + fr;
#pragma unroll
      for (int rg = 0; rg < 4; rg++) {
        const size_t grow = row0 + wave * 32 + i * 16 + fq + 4 * rg;
        if (grow < g.m && (!g.lower_only || gcol <= grow)) g.C[grow * g.ldc + gcol] = acc[i][j][rg];
      }
    }
}

/* the N.T stream-K configuration the last gsl_sinterp_hip_gemm_minus call of the process launched: 2 * cfg + (whole
   tiles only), or -1 for any other kernel (tests/test_gpu_gemm_mid.py checks that GSL_SINTERP_GEMM_CFG took effect) */
static int g_gemm_last_cfg = -1;
extern "C" int gsl_sinterp_hip_debug_gemm_last_cfg(void) { return __atomic_load_n(&g_gemm_last_cfg, __ATOMIC_RELAXED); }

/* the switches of the dispatch rule: read once per process, except the developer override GSL_SINTERP_GEMM_CFG
   ("<cfg>" or "<cfg>w", tools/gemm_cfg_sweep.py), which is read at every call */
static GemmSwitches gemm_switches(void)
{
  static const GemmSwitches once = [] {
    GemmSwitches s = GemmSwitches();
    s.no_dma = sinterp_env_flag("GSL_SINTERP_NO_DMA_GEMM");
    s.no_w8 = sinterp_env_flag("GSL_SINTERP_NO_GEMM8");
    s.rule_r4 = sinterp_env_flag("GSL_SINTERP_GEMM_RULE_R4");
    s.no_t64 = sinterp_env_flag("GSL_SINTERP_NO_GEMM64");
    s.no_group = sinterp_env_flag("GSL_SINTERP_NO_GEMM_GROUP");
    s.no_pipe = sinterp_env_flag("GSL_SINTERP_NO_GEMM_PIPE");
    s.no_hybrid = sinterp_env_flag("GSL_SINTERP_NO_HYBRID_SK");
    s.no_kn = sinterp_env_flag("GSL_SINTERP_NO_KN_STREAMK");
    s.rider_slices = sinterp_env_int("GSL_SINTERP_RIDER_SLICES", 0);
    return s;
  }();
  GemmSwitches s = once;
  const char *ov = getenv("GSL_SINTERP_GEMM_CFG");
  s.cfg_override = ov ? atoi(ov) : -1;
  s.cfg_whole = ov && strchr(ov, 'w') != NULL;
  return s;
}

/* attr: what the kernel's dynamic-LDS limit is raised to (0: the launch needs none) */
template <class Kernel, class... Args>
static int gemm_launch(gsl_sinterp_hip_ctx *ctx, const GemmPlan &p, int attr, Kernel kernel, const Args &...args)
{
  if (attr) { int ast = sinterp_func_lds(ctx, (const void *)kernel, attr); if (ast) return ast; }
  hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(p.block), p.lds, ctx->stream, args...);
  LAUNCH_CHECK(ctx);
  return ST_SUCCESS;
}

/* one case label per shipped instantiation: (family, cfg, pipe, ride, grouped) */
static constexpr unsigned plan_key(int family, int cfg = -1, bool pipe = false, bool ride = false, bool grouped = false)
{
  return (unsigned)family << 6 | (unsigned)(cfg + 1) << 3 | (pipe ? 4u : 0u) | (ride ? 2u : 0u) | (grouped ? 1u : 0u);
}

int sinterp_gemm_minus(gsl_sinterp_hip_ctx *ctx, size_t m, size_t n, size_t k, const double *A, size_t lda,
                       const double *B, size_t ldb, int b_is_kn, double *C, size_t ldc, int lower_only,
                       const sinterp_rider *rider, int *attached)
{
  if (attached) *attached = 0;
  if (m == 0 || n == 0 || k == 0) return ST_SUCCESS;
  GemmShape s;
  s.m = m; s.n = n; s.k = k; s.lower_only = lower_only != 0; s.b_is_kn = b_is_kn != 0;
  s.ab_aligned = ((lda & 1) == 0) && ((ldb & 1) == 0) && ((((uintptr_t)A) & 15) == 0) && ((((uintptr_t)B) & 15) == 0);
  s.c_aligned = ((((uintptr_t)C) & 15) == 0) && (ldc & 1) == 0;
  s.rider_offered = rider && attached;
  const GemmPlan p = gemm_plan(s, (unsigned)ctx->sk_wgs, gemm_switches());

  GemmArgs g;
  g.m = m; g.n = n; g.k = k; g.A = A; g.lda = lda; g.B = B; g.ldb = ldb; g.C = C; g.ldc = ldc;
  g.lower_only = lower_only;
  g.tiles_m = p.tiles_m; g.tiles_n = p.tiles_n; g.n_active = p.n_active;
  StreamK x;
  x.steps = p.steps; x.total = p.total; x.base = p.base; x.rem = p.rem; x.dp_rounds = p.dp_rounds;
  x.partial = ctx->d_sk_partial; x.flags = ctx->d_sk_flags;
  x.pri_tiles = p.pri_tiles; x.pri_sl = p.pri_sl; x.pri_nsl = p.pri_nsl; x.pri_base = p.pri_base;
  RiderArgs rd = RiderArgs();
  if (p.ride) {
    rd.info = rider->info; rd.j0 = rider->j0; rd.dinv = rider->dinv; rd.fb = rider->fb; rd.ldf = rider->ldf;
    rd.nrhs = rider->fb ? rider->nrhs : 0; rd.counter = rider->counter; rd.abort_word = rider->abort_word;
    rd.need = p.need;
    *attached = 1;
  }
  __atomic_store_n(&g_gemm_last_cfg, gemm_plan_last_cfg(p), __ATOMIC_RELAXED);

#define STREAMK(...) return gemm_launch(ctx, p, (int)p.lds, gemm_minus_streamk_kernel<__VA_ARGS__>, g, x, rd)
  switch (plan_key(p.family, p.cfg, p.pipe, p.ride, p.grouped)) {
    /*                    family      cfg       pipe   ride   grouped          BM   BN   WM  WN SS ST PIPE   BKN    RIDER */
    case plan_key(GEMM_SK_NT, SK_256,   false):                       STREAMK(256, 128, 64, 64);
    case plan_key(GEMM_SK_NT, SK_256,   true):                        STREAMK(256, 128, 64, 64, 1, 3, true);
    case plan_key(GEMM_SK_NT, SK_128,   false):                       STREAMK(128, 128, 64, 64);
    case plan_key(GEMM_SK_NT, SK_128,   true):                        STREAMK(128, 128, 64, 64, 1, 3, true);
    case plan_key(GEMM_SK_NT, SK_128W8, false):                       STREAMK(128, 128, 64, 32);
    case plan_key(GEMM_SK_NT, SK_128W8, true):                        STREAMK(128, 128, 64, 32, 1, 3, true);
    case plan_key(GEMM_SK_NT, SK_128W8, true,  true):                 STREAMK(128, 128, 64, 32, 1, 3, true,  false, true);
    case plan_key(GEMM_SK_NT, SK_64W8G, false, false, true):          STREAMK(64,  64,  32, 16, 4, 2);
    case plan_key(GEMM_SK_NT, SK_64W8G, false, true,  true):          STREAMK(64,  64,  32, 16, 4, 2, false, false, true);
    case plan_key(GEMM_SK_NT, SK_64,    false, false, false):         STREAMK(64,  64,  32, 32);
    case plan_key(GEMM_SK_NT, SK_64,    false, false, true):          STREAMK(64,  64,  32, 32, 4, 2);
    case plan_key(GEMM_SK_KN256, -1,    true):                        STREAMK(256, 128, 64, 64, 1, 3, true,  true);
    case plan_key(GEMM_SK_KN128, -1,    true):                        STREAMK(128, 128, 64, 64, 1, 3, true,  true);
    case plan_key(GEMM_SMALLK32): return gemm_launch(ctx, p, 160 * 1024, gemm_minus_smallk_kernel<32>, g);
    case plan_key(GEMM_SMALLK64): return gemm_launch(ctx, p, 160 * 1024, gemm_minus_smallk_kernel<64>, g);
    case plan_key(GEMM_DMA256):   return gemm_launch(ctx, p, (int)p.lds, gemm_minus_dma_nt_kernel<4>, g);
    case plan_key(GEMM_DMA128):   return gemm_launch(ctx, p, (int)p.lds, gemm_minus_dma_nt_kernel<2>, g);
    case plan_key(GEMM_PLAIN):
      if (p.b_is_kn) return p.full ? gemm_launch(ctx, p, 0, gemm_minus_kernel<1, true>, g) : gemm_launch(ctx, p, 0, gemm_minus_kernel<1, false>, g);
      return p.full ? gemm_launch(ctx, p, 0, gemm_minus_kernel<0, true>, g) : gemm_launch(ctx, p, 0, gemm_minus_kernel<0, false>, g);
  }
#undef STREAMK
  return sinterp_fail(ctx, ST_EFAILED, "gemm_minus: plan without a kernel", hipSuccess, __FILE__, __LINE__);
}

extern "C" int gsl_sinterp_hip_gemm_minus(gsl_sinterp_hip_ctx *ctx, size_t m, size_t n, size_t k, const double *d_a,
                                          size_t lda, const double *d_b, size_t ldb, int b_is_kn, double *d_c,
                                          size_t ldc, int lower_only)
{
  REQUIRE(ctx, ctx != NULL, ST_EFAULT);
  HIP_OK(ctx, hipSetDevice(ctx->device));      /* one context per device: bind before any launch */
  EXCLUSIVE_SECTION(ctx);
  REQUIRE(ctx, lda >= k && ldc >= n && ldb >= (b_is_kn ? n : k), ST_EINVAL);
  REQUIRE(ctx, (m == 0 || n == 0 || k == 0) || (d_a && d_b && d_c), ST_EFAULT);
  int st = sinterp_streamk_prepare(ctx);
  if (st) return st;
  return sinterp_gemm_minus(ctx, m, n, k, d_a, lda, d_b, ldb, b_is_kn, d_c, ldc, lower_only);
}
