/*
 * linear_finish.h -- the records of the piecewise-linear paths and the few operations that turn a located simplex into
 * a value: shared by the locate kernels (bary.hip, mesh3.hip) and by the fields sweep (linear_fields.hip), so that a
 * value is the same sequence of separately rounded fp64 operations wherever it is formed.  Every translation unit that
 * includes this is built with -ffp-contract=off (Makefile, HIP_EXACT_SRC).
 */
#ifndef SINTERP_HIP_LINEAR_FINISH_H
#define SINTERP_HIP_LINEAR_FINISH_H

#include "common.h"

/* ---- 2-D: DAG nodes and imported triangles (bary.hip has the layout's rationale) ---- */
struct __attribute__((aligned(64))) NodeRec {
  double x0, x1;
  double u00, u01, l10, u11;
  int child[3];
  int meta;
};
static_assert(sizeof(NodeRec) == GSL_SINTERP_TREE_RECORD_BYTES, "record size");

#define META_TYPE(m) ((m) & 3)
#define META_SWAPPED(m) (((m) >> 2) & 1)
#define META_SINGULAR(m) (((m) >> 3) & 1)
#define META_NCHILD(m) (((m) >> 4) & 3)

/* coords <- U^-1 L^-1 P ((y - x0) * scale)   (linear_simplex.c:644-649)      */
__device__ __forceinline__ void solve_node(const NodeRec &r, double y0, double y1, double s0, double s1,
                                           double &c0, double &c1)
{
  double b0 = (y0 - r.x0) * s0;
  double b1 = (y1 - r.x1) * s1;
  const bool sw = META_SWAPPED(r.meta);
  double t0 = sw ? b1 : b0;
  double t1 = sw ? b0 : b1;
  t1 -= r.l10 * t0;
  t1 = t1 / r.u11;
  t0 -= r.u01 * t1;
  t0 = t0 / r.u00;
  c0 = t0; c1 = t1;
}

__device__ __forceinline__ NodeRec load_rec(const NodeRec *__restrict__ rec, int k)
{
  /* four 16-byte loads of one aligned 64-byte line */
  const double2 *p = reinterpret_cast<const double2 *>(rec + k);
  double2 a = p[0], b = p[1], c = p[2];
  int4 d = *reinterpret_cast<const int4 *>(p + 3);
  NodeRec r;
  r.x0 = a.x; r.x1 = a.y; r.u00 = b.x; r.u01 = b.y; r.l10 = c.x; r.u11 = c.y;
  r.child[0] = d.x; r.child[1] = d.y; r.child[2] = d.z; r.meta = d.w;
  return r;
}

/* interp_point (linear_simplex.c:678-711): declares `double OUT`, the value in the simplex with coordinates (C0, C1); MASK
   bit i set = vertex i is a data point (not a cage seed).  A macro, not a function: the statements reach the compiler as
   they stood in the four kernels of bary.hip, whose instructions the move into this header therefore leaves as they were
   (an inlined function turned their branches into selects). */
#define BARY_INTERP(OUT, C0, C1, MASK, F0, F1, F2)                     \
  double OUT##_tot = 0, OUT = 0;                                       \
  OUT##_tot += (C0);                                                   \
  if ((MASK) & 1) OUT += (C0) * (F0);                                  \
  OUT##_tot += (C1);                                                   \
  if ((MASK) & 2) OUT += (C1) * (F1);                                  \
  if ((MASK) & 4) OUT += (1 - OUT##_tot) * (F2)

/* ---- 3-D: imported tetrahedra (mesh3.hip has the layout's rationale) ---- */
struct __attribute__((aligned(128))) TetRec {
  double x[3];
  double inv[9];
  int nbr[4];
  int meta;
  int pad[3];
};
static_assert(sizeof(TetRec) == GSL_SINTERP_MESH3_RECORD_BYTES, "record size");

#define TET_SINGULAR(m) ((m) & 1)

/* eight 16-byte loads of one aligned 128-byte line */
__device__ __forceinline__ TetRec load_tet(const TetRec *__restrict__ rec, int t)
{
  const double2 *p = reinterpret_cast<const double2 *>(rec + t);
  const double2 a = p[0], b = p[1], c = p[2], d = p[3], e = p[4], f = p[5];
  const int4 n = *reinterpret_cast<const int4 *>(p + 6), m = *reinterpret_cast<const int4 *>(p + 7);
  TetRec r;
  r.x[0] = a.x; r.x[1] = a.y; r.x[2] = b.x;
  r.inv[0] = b.y; r.inv[1] = c.x; r.inv[2] = c.y; r.inv[3] = d.x; r.inv[4] = d.y; r.inv[5] = e.x;
  r.inv[6] = e.y; r.inv[7] = f.x; r.inv[8] = f.y;
  r.nbr[0] = n.x; r.nbr[1] = n.y; r.nbr[2] = n.z; r.nbr[3] = n.w;
  r.meta = m.x; r.pad[0] = r.pad[1] = r.pad[2] = 0;
  return r;
}

/* barycentric coordinates of the standardised target z in the record's tetrahedron */
__device__ __forceinline__ void tet_coords(const TetRec &r, const double z[3], double c[4])
{
  const double b0 = z[0] - r.x[0], b1 = z[1] - r.x[1], b2 = z[2] - r.x[2];
  c[0] = r.inv[0] * b0 + r.inv[1] * b1 + r.inv[2] * b2;
  c[1] = r.inv[3] * b0 + r.inv[4] * b1 + r.inv[5] * b2;
  c[2] = r.inv[6] * b0 + r.inv[7] * b1 + r.inv[8] * b2;
  c[3] = 1.0 - (c[0] + c[1] + c[2]);
}

/* the value in a tetrahedron: this association order, nothing else */
#define TET_INTERP(C, F0, F1, F2, F3) ((((C)[0] * (F0) + (C)[1] * (F1)) + (C)[2] * (F2)) + (C)[3] * (F3))

#endif
