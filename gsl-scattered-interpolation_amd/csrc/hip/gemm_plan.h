/*
 * gemm_plan.h -- the dispatch rule of the trailing update C -= A op(B) (gemm.hip): which kernel, which tile
 * configuration, how the (tile, K-step) space is split among the workgroups, the rider's priority slices and the
 * launch dimensions.  Host integer arithmetic on (shape, alignment, CU count, switches) and nothing else: no device, no
 * environment, no pointers, no statics, so it compiles with a plain C++17 compiler and tests/test_gemm_plan.py pins
 * every decision.  sinterp_gemm_minus (gemm.hip) turns a plan into kernel arguments and one launch.
 */
#ifndef SINTERP_GEMM_PLAN_H
#define SINTERP_GEMM_PLAN_H

#include <stddef.h>

#define GT_BM 128
#define GT_BN 128
#define GT_BK 16
#define DM_STAGES 3              /* LDS ring depth of the DMA kernels */
#define SK_PRI_SLOTS 32          /* K-slices of priority tiles per launch */
#define GEMM_RIDER_LDS 128272u   /* the rider's potrf128 image + its poll result: DIAG128_LDS_BYTES + 16 (gemm.hip asserts it) */

struct GemmShape {
  size_t m, n, k;
  bool lower_only, b_is_kn;
  bool ab_aligned;              /* A and B 16-byte aligned, lda and ldb even */
  bool c_aligned;               /* C 16-byte aligned, ldc even: the rider writes and reads the block with vector accesses */
  bool rider_offered;           /* the caller passed a rider and somewhere to report that it was attached */
};

/* one member per GSL_SINTERP_* switch that the dispatch reads (gemm.hip: gemm_switches) */
struct GemmSwitches {
  bool no_dma, no_w8, rule_r4, no_t64, no_group, no_pipe, no_hybrid, no_kn;
  int rider_slices;             /* 0 = default */
  int cfg_override;             /* GSL_SINTERP_GEMM_CFG: the tile configuration, -1 = none ... */
  bool cfg_whole;               /* ... and its "w" suffix: whole tiles only, no K split */
};

/* Tile configurations of the stream-K update (the values of GSL_SINTERP_GEMM_CFG) */
enum { SK_256 = 0,      /* 256x128, 8 waves of 64x64 */
       SK_128 = 1,      /* 128x128, 4 waves of 64x64 */
       SK_64 = 2,       /* 64x64,   4 waves of 32x32 (4-step groups when K allows) */
       SK_128W8 = 5,    /* 128x128, 8 waves of 64x32 */
       SK_64W8G = 6 };  /* 64x64,   8 waves of 32x16, 4-step groups */
static inline int sk_tile(int cfg) { return cfg == SK_128 || cfg == SK_128W8 ? 128 : cfg == SK_256 ? 256 : 64; }

enum GemmFamily {
  GEMM_SMALLK32, GEMM_SMALLK64,   /* gemm_minus_smallk_kernel<32>, <64> */
  GEMM_SK_NT,                     /* gemm_minus_streamk_kernel, B stored [n][k]: cfg, pipe, ride and grouped pick the instantiation */
  GEMM_DMA256, GEMM_DMA128,       /* gemm_minus_dma_nt_kernel<4>, <2>: one tile per workgroup */
  GEMM_SK_KN256, GEMM_SK_KN128,   /* gemm_minus_streamk_kernel, B stored [k][n], 256- and 128-row tiles */
  GEMM_PLAIN                      /* gemm_minus_kernel<b_is_kn, full> */
};

struct GemmPlan {
  GemmFamily family;
  bool b_is_kn, full;           /* GEMM_PLAIN: the template arguments (full is not set for the other families) */
  /* GEMM_SK_NT (cfg = -1 elsewhere) */
  int cfg;
  bool whole, grouped, pipe, ride;
  unsigned G;                   /* stream-K (N.T and [k][n]): workgroups that share the update; the rider is one more */
  int tiles_m, tiles_n;         /* GemmArgs of the launch */
  unsigned n_active;
  /* the scalar members of StreamK (gemm.hip) */
  unsigned steps, total, base, rem, dp_rounds, pri_tiles, pri_sl, pri_nsl, pri_base;
  unsigned need;                /* RiderArgs::need */
  unsigned grid, block;
  size_t lds;                   /* dynamic LDS of the launch */
};

/* what gsl_sinterp_hip_debug_gemm_last_cfg reports for a launch of this plan */
static inline int gemm_plan_last_cfg(const GemmPlan &p) { return p.family == GEMM_SK_NT ? 2 * p.cfg + (p.whole ? 1 : 0) : -1; }

/* tiles of configuration c (tile shape only; see the table above gemm_minus_streamk_kernel); tm / tn start as the
   128-tile counts and leave as the GemmArgs of that configuration */
static inline unsigned tiles_of(const GemmShape &s, int c, int &tm, int &tn)
{
  if (c == SK_256) {
    tm = (int)(s.m / 256);
    if (!s.lower_only) return (unsigned)tm * (unsigned)tn;
    const unsigned fr_ = (unsigned)tn / 2;
    return 2 * fr_ * (fr_ + 1) / 2 + ((unsigned)tm - fr_) * (unsigned)tn;
  }
  const int bt = sk_tile(c);
  tm = (int)(s.m / bt); tn = (int)(s.n / bt);
  if (s.lower_only && tm < tn) tn = tm;
  const unsigned tm_ = (unsigned)tm, tn_ = (unsigned)tn;
  return s.lower_only ? tn_ * (tn_ + 1) / 2 + (tm_ - tn_) * tn_ : tm_ * tn_;
}

/* the dispatch rule, fitted to every update shape of the N = 4096 / 8192 / 16384 recursions (tools/gemm_cfg_sweep.py,
   DESIGN.md section 3): the 256x128 tile once every CU gets >= 128 of its K-steps, 64x64 tiles while 128-tiles would
   fill at most 3/4 of the CUs, 128x128 tiles (8 waves) between; always the hybrid split (whole tiles only lost) */
static inline int sk_rule(const GemmShape &s, bool can256, int tm128, int tn128, unsigned steps, unsigned cus)
{
  int tm = tm128, tn = tn128;
  if (can256 && (unsigned long long)tiles_of(s, SK_256, tm, tn) * steps >= 128ull * cus) return SK_256;
  tm = tm128; tn = tn128;
  if (4ull * tiles_of(s, SK_128, tm, tn) <= 3ull * cus) return SK_64W8G;
  return SK_128W8;
}

/* cus: the persistent workgroups the context prepared buffers for (= CUs of the device); 0 = stream-K not prepared */
static inline GemmPlan gemm_plan(const GemmShape &s, unsigned cus, const GemmSwitches &sw)
{
  const size_t m = s.m, n = s.n, k = s.k;
  const bool lower_only = s.lower_only;
  GemmPlan p = GemmPlan();
  p.cfg = -1;
  p.b_is_kn = s.b_is_kn;
  p.block = 256;
  p.tiles_m = (int)((m + GT_BM - 1) / GT_BM);
  p.tiles_n = (int)((n + GT_BN - 1) / GT_BN);
  if (lower_only && p.tiles_m < p.tiles_n) p.tiles_n = p.tiles_m;   /* columns right of the square part are all above the diagonal */
  unsigned grid = (unsigned)p.tiles_m * (unsigned)p.tiles_n;
  if (lower_only) {
    const unsigned tn_ = (unsigned)p.tiles_n;
    grid = tn_ * (tn_ + 1) / 2 + ((unsigned)p.tiles_m - tn_) * tn_;
  }
  p.n_active = grid;
  const int tm128 = p.tiles_m, tn128 = p.tiles_n;
  const bool full = (m % GT_BM == 0) && (n % GT_BN == 0) && (k % GT_BK == 0) && s.ab_aligned;
  /* skinny small-K update: one round trip */
  if (!s.b_is_kn && (n == 32 || n == 64) && k <= 64 && (k % 4) == 0 && k >= 4 && s.ab_aligned) {
    p.family = n == 32 ? GEMM_SMALLK32 : GEMM_SMALLK64;
    p.grid = (unsigned)p.tiles_m;
    p.lds = (size_t)(128 + n) * (k + 2) * sizeof(double);
    return p;
  }
  if (full && !s.b_is_kn && k >= 4 * GT_BK && !sw.no_dma) {
    if (cus > 0) {
      /* stream-K: G persistent workgroups share the (tile, K-step) space evenly */
      unsigned steps = (unsigned)(k / GT_BK);              /* groups per tile; rescaled below for the grouped 64x64 variants */
      const bool can256 = !sw.no_w8 && (m % 256 == 0) && (!lower_only || (tn128 % 2) == 0);
      int cfg;
      bool whole = false;
      if (sw.rule_r4) {
        /* round 4: 256x128 when every CU gets >= 16 K-steps of it, 64x64 when 128-tiles fill at most half of the CUs */
        cfg = SK_128;
        { int tm = tm128, tn = tn128; const unsigned t8 = tiles_of(s, SK_256, tm, tn);
          if (can256 && (unsigned long long)t8 * steps >= 16ull * cus) cfg = SK_256; }
        if (cfg == SK_128 && !sw.no_t64 && 2u * grid <= cus) cfg = SK_64;
      } else {
        cfg = sk_rule(s, can256, tm128, tn128, steps, cus);
        if (sw.no_t64 && cfg == SK_64W8G) cfg = SK_128W8;
      }
      /* developer override (tools/gemm_cfg_sweep.py): "<cfg>" or "<cfg>w" (whole tiles, no K split), where the shape allows it */
      const int want_cfg = sw.cfg_override;
      if ((want_cfg == SK_256 && can256) || want_cfg == SK_128 || want_cfg == SK_64 || want_cfg == SK_128W8 || want_cfg == SK_64W8G) {
        cfg = want_cfg;
        whole = sw.cfg_whole;
      }
      int tm = tm128, tn = tn128;
      const unsigned tiles = tiles_of(s, cfg, tm, tn);
      if (cfg == SK_64W8G && (sw.no_group || (k % (4 * GT_BK)) != 0)) cfg = SK_64;   /* ungrouped 64x64 tiles */
      const bool grouped = (cfg == SK_64 && !sw.no_group && (k % (4 * GT_BK)) == 0) || cfg == SK_64W8G;
      if (grouped) steps = (unsigned)(k / (4 * GT_BK));
      if (sw.no_hybrid) whole = false;
      /* the rider rides on the 128x128 and 64x64 8-wave configurations, when the block it factors is covered by the first
         tiles of the enumeration (lower_only, at least 128 x 128) and a CU can be left to it */
      const bool ride = s.rider_offered && lower_only && m >= 128 && n >= 128 && cus >= 2 && !whole &&
                        ((cfg == SK_128W8 && !sw.no_pipe) || cfg == SK_64W8G) && s.c_aligned;
      const unsigned cus_g = ride ? cus - 1 : cus;
      unsigned G, dp_rounds;
      unsigned long long total64;
      if (whole) {
        /* whole tiles only: one tile per workgroup and round, the last round partly filled */
        G = tiles < cus ? tiles : cus;
        dp_rounds = tiles / G;
        total64 = (unsigned long long)(tiles - dp_rounds * G) * steps;
      } else {
        total64 = (unsigned long long)tiles * steps;
        unsigned long long want = total64 / (grouped ? 4 : 16);   /* >= 16 K-steps (of 16) per workgroup ... */
        if (want < tiles) want = tiles;                     /* ... but never fewer workgroups than tiles */
        if (want > cus_g) want = cus_g;
        G = (unsigned)(want ? want : 1);
        /* many tiles: all but the last full round (and the remainder) as whole tiles */
        dp_rounds = (!sw.no_hybrid && tiles / G >= 2) ? tiles / G - 1 : 0;
        total64 = (unsigned long long)(tiles - dp_rounds * G) * steps;
      }
      if (total64 < 0x7fffffffull) {
        p.family = GEMM_SK_NT;
        p.cfg = cfg; p.whole = whole; p.grouped = grouped; p.ride = ride; p.G = G;
        p.pipe = !sw.no_pipe && (cfg == SK_256 || cfg == SK_128 || cfg == SK_128W8);
        p.tiles_m = tm; p.tiles_n = tn;
        p.steps = steps; p.dp_rounds = dp_rounds;
        p.total = (unsigned)total64;
        if (whole) { p.base = steps; p.rem = 0; }        /* workgroup w: the w-th remaining tile, if any */
        else { p.base = p.total / G; p.rem = p.total % G; }
        p.pri_tiles = 0; p.pri_sl = 0; p.pri_nsl = 1;
        p.pri_base = cus;
        if (ride) {
          p.need = cfg == SK_64W8G ? 3u : 1u;
          if (dp_rounds == 0) {
            /* one round: without a split the covering tiles end when the launch ends.  S slices per tile (the largest
               divisor of the step count up to the wanted number), every holder keeping at least half of its share
               for its own range */
            unsigned S = sw.rider_slices > 0 ? (unsigned)sw.rider_slices : 4u;
            if (S > steps) S = steps;
            while (S > 1 && (steps % S) != 0) S--;
            while (S > 1 && (p.need * S > G || p.need * S > SK_PRI_SLOTS || 2 * (steps / S) > p.base || p.need >= tiles)) {
              S--;
              while (S > 1 && (steps % S) != 0) S--;
            }
            if (S > 1) {
              p.pri_tiles = p.need; p.pri_nsl = S; p.pri_sl = steps / S;
              p.total -= p.need * steps;                  /* the space the ranges share; base / rem still count the slices */
            }
          }
        }
        const bool w8 = cfg == SK_256 || cfg == SK_128W8 || cfg == SK_64W8G;
        const int bt = sk_tile(cfg), bn = cfg == SK_256 ? 128 : bt;
        const int ring = grouped ? 2 * 4 : DM_STAGES;     /* 4-step groups run a two-deep ring */
        p.grid = G + (ride ? 1u : 0u);
        p.block = w8 ? 512 : 256;
        p.lds = (size_t)ring * (bt + bn) * GT_BK * sizeof(double);
        if (ride && p.lds < GEMM_RIDER_LDS) p.lds = GEMM_RIDER_LDS;
        return p;
      }
    }
    /* 256x128 tiles (8 waves) when the rows split evenly and there is enough work for every CU */
    const bool w8 = !sw.no_w8 && (m % 256 == 0) && (!lower_only || (tn128 % 2) == 0) && grid >= 1024;
    if (w8) {
      p.family = GEMM_DMA256;
      p.tiles_m = (int)(m / 256);
      p.grid = (unsigned)p.tiles_m * (unsigned)p.tiles_n;
      if (lower_only) {
        const unsigned fr_ = (unsigned)p.tiles_n / 2;
        p.grid = 2 * fr_ * (fr_ + 1) / 2 + ((unsigned)p.tiles_m - fr_) * (unsigned)p.tiles_n;
      }
      p.block = 512;
      p.lds = (size_t)DM_STAGES * (256 + 128) * GT_BK * sizeof(double);   /* 144 KiB */
      return p;
    }
    p.family = GEMM_DMA128;
    p.grid = grid;
    p.lds = (size_t)DM_STAGES * (128 + 128) * GT_BK * sizeof(double);     /* 96 KiB */
    return p;
  }
  if (s.b_is_kn && full && !lower_only && !sw.no_dma && !sw.no_kn && cus > 0 && k >= 4 * GT_BK) {
    /* C -= A B with B stored [k][n] (the N.N updates of the LU route): the stream-K DMA pipeline with a [k][n] B image */
    const unsigned steps = (unsigned)(k / GT_BK);
    int tm = tm128;
    unsigned tiles = grid;
    bool big = false;
    if ((m % 256) == 0) {
      const unsigned t8 = (unsigned)(m / 256) * (unsigned)tn128;
      if ((unsigned long long)t8 * steps >= 16ull * cus) { big = true; tm = (int)(m / 256); tiles = t8; }
    }
    unsigned long long total64 = (unsigned long long)tiles * steps;
    unsigned long long want = total64 / 16;
    if (want < tiles) want = tiles;
    if (want > (unsigned long long)cus) want = (unsigned long long)cus;
    const unsigned G = (unsigned)(want ? want : 1);
    const unsigned dp_rounds = (tiles / G >= 2) ? tiles / G - 1 : 0;
    total64 = (unsigned long long)(tiles - dp_rounds * G) * steps;
    if (total64 < 0x7fffffffull) {
      p.family = big ? GEMM_SK_KN256 : GEMM_SK_KN128;
      p.pipe = true;
      p.G = G; p.tiles_m = tm;
      p.steps = steps; p.dp_rounds = dp_rounds;
      p.total = (unsigned)total64; p.base = p.total / G; p.rem = p.total % G;
      p.pri_tiles = 0; p.pri_sl = 0; p.pri_nsl = 1; p.pri_base = 0;
      p.grid = G;
      p.block = big ? 512 : 256;
      p.lds = (size_t)DM_STAGES * ((big ? 256 : 128) * GT_BK + GT_BK * (128 + 16)) * sizeof(double);   /* 150 KiB, 102 KiB */
      return p;
    }
  }
  p.family = GEMM_PLAIN;
  p.full = full;
  p.grid = grid;
  return p;
}

#endif
