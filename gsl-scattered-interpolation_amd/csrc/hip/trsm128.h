/*
 * trsm128.h -- the row solve against a 128-wide diagonal block of a Cholesky factor, X = B L^-T for a 64-row strip per
 * workgroup, as one body for chol_trsm128_kernel (chol.hip: the rows below a panel, in place in A) and
 * krige_trsm128_kernel (krige_var.hip: the work matrix Z of the kriging variance and of the leave-one-out diagonal).
 *
 * Block substitution over the four 32-column blocks c, every step an MFMA product:
 *     Y_c = B_c - sum_{p<c} X_p L_cp^T,     X_c = Y_c Dinv_c^T,
 * wave w owns rows 16w .. 16w+15 for all four steps, so the steps need no workgroup barrier: 144 dependent
 * v_mfma_f64_16x16x4_f64 per wave.  The B tile, the six off-diagonal 32 x 32 blocks of L and the four inverted diagonal
 * blocks are staged in LDS with one memory round trip.  The kernels differ only in where those operands come from and in
 * what happens to X on its way out; they say so with callables.  Pass lambdas that capture by value: a kernel argument
 * reached through a by-reference capture is no longer known to be __restrict__, and the address arithmetic grows.
 */
#ifndef SINTERP_TRSM128_H
#define SINTERP_TRSM128_H

#include "chol_potrf.h"

/* LDS of the body, in doubles: Bt[64][TR_LD], then the 6 off-diagonal blocks of L ((bi, bj) at bi(bi-1)/2 + bj), then
   the 4 inverted diagonal blocks, all [32][PQ].  A kernel's own LDS starts behind it. */
#define TRSM128_LDS (64 * TR_LD + 10 * PBLK)

/* The staging: one round trip, every global load is issued before the first LDS store.
     brow(r)              pointer to the 128 entries of row r (0..63) of the B tile, 16-byte aligned
     lent(bi, bj, r, k)   entry (r, k) of the 32 x 32 block (bi, bj), bi > bj, of the diagonal block of L
     dent(b, r, k)        entry (r, k) of the inverted diagonal block b (0..3)
     more_loads()         called behind the loads above and in front of the LDS stores: global loads of the kernel's own
                          that belong in the same round trip */
template <class BRow, class LEnt, class DEnt, class More>
__device__ __forceinline__ void trsm128_stage(double *sm, int tid, BRow brow, LEnt lent, DEnt dent, More more_loads)
{
  double *Bt = sm, *Lb = Bt + 64 * TR_LD, *Dvb = Lb + 6 * PBLK;
  double2 vb[16];
  double vl[24], vd[16];
  const int r8 = tid >> 5, k = tid & 31;
#pragma unroll
  for (int t = 0; t < 16; t++) {
    const int e = t * 256 + tid, r = e >> 6, k2 = (e & 63) * 2;
    vb[t] = *reinterpret_cast<const double2 *>(brow(r) + k2);
  }
#pragma unroll
  for (int t = 0; t < 24; t++) {
    constexpr int BI[6] = {1, 2, 2, 3, 3, 3}, BJ[6] = {0, 0, 1, 0, 1, 2};
    const int b = t >> 2, r = (t & 3) * 8 + r8;
    vl[t] = lent(BI[b], BJ[b], r, k);
  }
#pragma unroll
  for (int t = 0; t < 16; t++) vd[t] = dent(t >> 2, (t & 3) * 8 + r8, k);
  more_loads();
#pragma unroll
  for (int t = 0; t < 16; t++) {
    const int e = t * 256 + tid, r = e >> 6, k2 = (e & 63) * 2;
    Bt[r * TR_LD + k2] = vb[t].x; Bt[r * TR_LD + k2 + 1] = vb[t].y;
  }
#pragma unroll
  for (int t = 0; t < 24; t++) Lb[(t >> 2) * PBLK + ((t & 3) * 8 + r8) * PQ + k] = vl[t];
#pragma unroll
  for (int t = 0; t < 16; t++) Dvb[(t >> 2) * PBLK + ((t & 3) * 8 + r8) * PQ + k] = vd[t];
}

template <class BRow, class LEnt, class DEnt>
__device__ __forceinline__ void trsm128_stage(double *sm, int tid, BRow brow, LEnt lent, DEnt dent)
{
  trsm128_stage(sm, tid, brow, lent, dent, [] {});
}

/* The solve, after the barrier behind the staging.  X replaces B in Bt (every wave writes its own rows only), and
   out(c, f, rg, v) receives every finished entry: v = X[16 wave + (lane >> 4) + 4 rg][32 c + 16 f + (lane & 15)]. */
template <class Out>
__device__ __forceinline__ void trsm128_solve(double *sm, int tid, Out out)
{
  double *Bt = sm;
  const double *Lb = Bt + 64 * TR_LD, *Dvb = Lb + 6 * PBLK;
  const int lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4;
  double *arow = Bt + (wave * 16 + fr) * TR_LD + fq;        /* A-operand view of this wave's rows */
  double *drow = Bt + (wave * 16 + fq) * TR_LD + fr;        /* accumulator (D layout) view */
#pragma unroll
  for (int c = 0; c < 4; c++) {
    double4_t acc[2];
#pragma unroll
    for (int f = 0; f < 2; f++)
#pragma unroll
      for (int rg = 0; rg < 4; rg++) acc[f][rg] = drow[4 * rg * TR_LD + c * 32 + f * 16];
#pragma unroll
    for (int p = 0; p < c; p++) {
      const double *lb = Lb + (c * (c - 1) / 2 + p) * PBLK + fr * PQ + fq;
#pragma unroll
      for (int kk = 0; kk < 8; kk++) {
        const double a = -arow[p * 32 + kk * 4];
#pragma unroll
        for (int f = 0; f < 2; f++) acc[f] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, lb[f * 16 * PQ + kk * 4], acc[f], 0, 0, 0);
      }
    }
    /* Y -> LDS (own rows), then X_c = Y Dinv_c^T (Dinv lower triangular: fragment f needs K = 16(f+1)) */
#pragma unroll
    for (int f = 0; f < 2; f++)
#pragma unroll
      for (int rg = 0; rg < 4; rg++) drow[4 * rg * TR_LD + c * 32 + f * 16] = acc[f][rg];
    const double *db = Dvb + c * PBLK + fr * PQ + fq;
#pragma unroll
    for (int f = 0; f < 2; f++) {
      acc[f] = (double4_t){0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int kk = 0; kk < (f + 1) * 4; kk++)
        acc[f] = __builtin_amdgcn_mfma_f64_16x16x4f64(arow[c * 32 + kk * 4], db[f * 16 * PQ + kk * 4], acc[f], 0, 0, 0);
    }
#pragma unroll
    for (int f = 0; f < 2; f++)
#pragma unroll
      for (int rg = 0; rg < 4; rg++) {
        drow[4 * rg * TR_LD + c * 32 + f * 16] = acc[f][rg];
        out(c, f, rg, acc[f][rg]);
      }
  }
}

#endif
