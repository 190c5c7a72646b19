/* Prints the plans of csrc/hip/gemm_plan.h for the records on standard input (tests/test_gemm_plan.py).
   One record per line, integers separated by blanks:
     m n k lower_only b_is_kn ab_aligned c_aligned rider_offered cus
     no_dma no_w8 rule_r4 no_t64 no_group no_pipe no_hybrid no_kn rider_slices cfg_override cfg_whole
   One plan per line, the family by name and then the PLAN_COLUMNS of the test in order. */
#include <stdio.h>
#include "gemm_plan.h"

static const char *family_name(GemmFamily f)
{
  switch (f) {
    case GEMM_SMALLK32: return "smallk32";
    case GEMM_SMALLK64: return "smallk64";
    case GEMM_SK_NT: return "sk_nt";
    case GEMM_DMA256: return "dma256";
    case GEMM_DMA128: return "dma128";
    case GEMM_SK_KN256: return "sk_kn256";
    case GEMM_SK_KN128: return "sk_kn128";
    case GEMM_PLAIN: return "plain";
  }
  return "?";
}

int main(void)
{
  char line[512];
  while (fgets(line, sizeof line, stdin)) {
    unsigned long long m, n, k;
    int v[17];
    unsigned cus;
    if (sscanf(line, "%llu %llu %llu %d %d %d %d %d %u %d %d %d %d %d %d %d %d %d %d %d", &m, &n, &k, &v[0], &v[1], &v[2], &v[3], &v[4],
               &cus, &v[5], &v[6], &v[7], &v[8], &v[9], &v[10], &v[11], &v[12], &v[13], &v[14], &v[15]) != 20) {
      fprintf(stderr, "bad record: %s", line);
      return 1;
    }
    GemmShape s;
    s.m = (size_t)m; s.n = (size_t)n; s.k = (size_t)k;
    s.lower_only = v[0] != 0; s.b_is_kn = v[1] != 0; s.ab_aligned = v[2] != 0; s.c_aligned = v[3] != 0; s.rider_offered = v[4] != 0;
    GemmSwitches sw;
    sw.no_dma = v[5] != 0; sw.no_w8 = v[6] != 0; sw.rule_r4 = v[7] != 0; sw.no_t64 = v[8] != 0; sw.no_group = v[9] != 0;
    sw.no_pipe = v[10] != 0; sw.no_hybrid = v[11] != 0; sw.no_kn = v[12] != 0;
    sw.rider_slices = v[13]; sw.cfg_override = v[14]; sw.cfg_whole = v[15] != 0;
    const GemmPlan p = gemm_plan(s, cus, sw);
    printf("%s %d %d %d %d %d %d %d %u %d %d %u %u %u %u %u %u %u %u %u %u %u %u %u %zu %d\n", family_name(p.family), (int)p.b_is_kn,
           (int)p.full, p.cfg, (int)p.whole, (int)p.grouped, (int)p.pipe, (int)p.ride, p.G, p.tiles_m, p.tiles_n, p.n_active, p.steps,
           p.total, p.base, p.rem, p.dp_rounds, p.pri_tiles, p.pri_sl, p.pri_nsl, p.pri_base, p.need, p.grid, p.block, p.lds,
           gemm_plan_last_cfg(p));
  }
  return 0;
}
