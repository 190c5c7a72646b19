/*
 * natural.hip -- natural-neighbour (Sibson) interpolation on a 2-D Delaunay mesh.
 *
 * s(y) = sum_i A_i f_i / sum_i A_i, A_i = the area the Voronoi cell of the target y steals from site i.  The areas come
 * from the CAVITY of y (the triangles whose circumcircle contains y) without building a cell: in coordinates relative
 * to y, with every triangle counter-clockwise, C_t the circumcentre of t, g(i, j) the circumcentre of (y, v_i, v_j) and
 * m_i = v_i / 2, every edge i -> j of a cavity triangle a (neighbour b across it) adds
 *     b in the cavity, counted once (a < b):   e = cross(C_b, C_a) / 2,   A_i += e,  A_j -= e
 *     otherwise (cavity boundary, hull):       A_i += [cross(g, C_a) + cross(m_i, g)] / 2
 *                                              A_j += [cross(C_a, g) + cross(g, m_j)] / 2
 * Only num = sum A_i f_i and den = sum A_i are kept (the interior edges cancel in den).  The cavity is the located
 * triangle T0 (unconditionally) plus everything reachable from it across edges whose neighbour passes the strict
 * in-circle test; flat triangles never belong to it.  A Delaunay cavity has no interior vertex, its dual graph is a
 * tree: a depth-first walk that never returns across its entry edge visits every cavity triangle once.
 *
 * Special cases, functions of (mesh, target) only: a target equal to a vertex of T0 returns that vertex's datum; a
 * target within rounding of a cavity-boundary edge (cross(v_i, v_j) <= 1e-12 |v_j - v_i|^2: the hull, or a needle-thin
 * configuration) returns the piecewise-linear value of T0, the interpolant's limit there; index -1 gives NaN.
 *
 * Built without FMA contraction (Makefile, HIP_EXACT_SRC): cross(a, b) is then exactly -cross(b, a), so an interior
 * edge adds the same bits whichever of its two triangles the walk meets first, and the walk and the scan differ only
 * in the order of their sums.
 */
#include "common.h"
#include <math.h>

/* 80 bytes = five 16-byte loads; n_tri records and a trailer whose v[0] holds the metric (the per-axis factors).
   Vertices in metric coordinates, counter-clockwise; nbr[k] = the neighbour across the
   edge opposite vertex k (the edge v[k+1] -> v[k+2]); c = circumcentre - v[0] (so that circumcentre - y is formed from
   two short vectors); meta bit 0: flat, bit 1: vertices 1 and 2 are exchanged against the mesh's order (the response
   table keeps the mesh's). */
struct __attribute__((aligned(16))) NnRec {
  double v[3][2];
  double c[2];
  int nbr[3];
  int meta;
};
static_assert(sizeof(NnRec) == GSL_SINTERP_NATURAL_RECORD_BYTES, "natural-neighbour record size");

struct __attribute__((aligned(32))) NnTab { double f[3]; int mask, pad; };     /* bary.hip's LeafRec (tree_bind_kernel) */
static_assert(sizeof(NnTab) == GSL_SINTERP_TREE_LEAFTAB_BYTES, "leaf table size");

#define NN_FLAT(meta) ((meta) & 1)
#define NN_SWAPPED(meta) (((meta) >> 1) & 1)
#define NN_STACK GSL_SINTERP_NATURAL_STACK   /* pending cavity triangles per lane (LDS) */
#define NN_MAX_POPS 1024     /* a Delaunay cavity is a tree; a cycle (rounding on cocircular sites) ends here -> scan */
#define NN_EDGE_TOL 1e-12
#define NN_FLAT_TOL 1e-14

__device__ __forceinline__ double cross2(double ax, double ay, double bx, double by) { return ax * by - ay * bx; }

__global__ void __launch_bounds__(256)
natural_pack_kernel(int n_tri, const int *__restrict__ tri, const int *__restrict__ nbr, int n_points,
                    const double *__restrict__ points, double s0, double s1, NnRec *__restrict__ rec)
{
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t > n_tri) return;
  NnRec r;
  if (t == n_tri) {                                          /* trailer: the metric, for the evaluation kernels */
    for (int i = 0; i < 3; i++) { r.v[i][0] = s0; r.v[i][1] = s1; r.nbr[i] = -1; }
    r.c[0] = r.c[1] = 0.0; r.meta = 1;
    rec[t] = r;
    return;
  }
  bool bad = false;
  for (int i = 0; i < 3; i++) {
    const int id = tri[3 * t + i];
    if (id < 0 || id >= n_points) { bad = true; r.v[i][0] = r.v[i][1] = 0.0; }
    else { r.v[i][0] = points[2 * (size_t)id] * s0; r.v[i][1] = points[2 * (size_t)id + 1] * s1; }
    const int nb = nbr[3 * t + i];
    r.nbr[i] = (nb >= 0 && nb < n_tri && nb != t) ? nb : -1;
  }
  int meta = 0;
  double orient = cross2(r.v[1][0] - r.v[0][0], r.v[1][1] - r.v[0][1], r.v[2][0] - r.v[0][0], r.v[2][1] - r.v[0][1]);
  if (orient < 0.0) {
    double q = r.v[1][0]; r.v[1][0] = r.v[2][0]; r.v[2][0] = q;
    q = r.v[1][1]; r.v[1][1] = r.v[2][1]; r.v[2][1] = q;
    const int w = r.nbr[1]; r.nbr[1] = r.nbr[2]; r.nbr[2] = w;
    meta |= 2;
    orient = -orient;
  }
  const double bx = r.v[1][0] - r.v[0][0], by = r.v[1][1] - r.v[0][1], cx = r.v[2][0] - r.v[0][0], cy = r.v[2][1] - r.v[0][1];
  const double ex = r.v[2][0] - r.v[1][0], ey = r.v[2][1] - r.v[1][1];
  const double b2 = bx * bx + by * by, c2 = cx * cx + cy * cy, e2 = ex * ex + ey * ey;
  orient = cross2(bx, by, cx, cy);
  if (bad || !(orient > NN_FLAT_TOL * (b2 + c2 + e2))) { meta |= 1; r.c[0] = r.c[1] = 0.0; }
  else {
    const double d = 2.0 * orient;
    r.c[0] = (cy * b2 - by * c2) / d;
    r.c[1] = (bx * c2 - cx * b2) / d;
    if (!(fabs(r.c[0]) < INFINITY && fabs(r.c[1]) < INFINITY)) { meta |= 1; r.c[0] = r.c[1] = 0.0; }
  }
  r.meta = meta;
  rec[t] = r;
}

__device__ __forceinline__ NnRec nn_load(const NnRec *__restrict__ rec, int t)
{
  const double2 *p = reinterpret_cast<const double2 *>(rec + t);
  const double2 a = p[0], b = p[1], c = p[2], d = p[3];
  const int4 w = *reinterpret_cast<const int4 *>(p + 4);
  NnRec r;
  r.v[0][0] = a.x; r.v[0][1] = a.y; r.v[1][0] = b.x; r.v[1][1] = b.y; r.v[2][0] = c.x; r.v[2][1] = c.y;
  r.c[0] = d.x; r.c[1] = d.y;
  r.nbr[0] = w.x; r.nbr[1] = w.y; r.nbr[2] = w.z; r.meta = w.w;
  return r;
}

/* strict in-circle test of y against the counter-clockwise triangle r, in coordinates relative to y */
__device__ __forceinline__ bool nn_incircle(const NnRec &r, double y0, double y1)
{
  const double ax = r.v[0][0] - y0, ay = r.v[0][1] - y1, bx = r.v[1][0] - y0, by = r.v[1][1] - y1;
  const double cx = r.v[2][0] - y0, cy = r.v[2][1] - y1;
  const double a2 = ax * ax + ay * ay, b2 = bx * bx + by * by, c2 = cx * cx + cy * cy;
  const double det = cross2(ax, ay, bx, by) * c2 + cross2(bx, by, cx, cy) * a2 + cross2(cx, cy, ax, ay) * b2;
  return det > 0.0;
}

/* the three vertex data of a record's triangle, in the record's (counter-clockwise) vertex order */
__device__ __forceinline__ void nn_data(const NnTab *__restrict__ tab, int t, int meta, double f[3])
{
  const double2 p = *reinterpret_cast<const double2 *>(tab + t);
  const double f2 = tab[t].f[2];
  const bool sw = NN_SWAPPED(meta);
  f[0] = p.x; f[1] = sw ? f2 : p.y; f[2] = sw ? p.y : f2;
}

struct NnAcc { double num, den; bool lin; };

/* cavity-boundary edge i -> j of the triangle with circumcentre (ca0, ca1) - y; (ix, iy), (jx, jy) = v_i - y, v_j - y */
__device__ __forceinline__ void nn_boundary_edge(double ix, double iy, double jx, double jy, double ca0, double ca1, double fi,
                                                 double fj, NnAcc &acc)
{
  const double a2 = cross2(ix, iy, jx, jy);
  const double dx = jx - ix, dy = jy - iy;
  if (!(a2 > NN_EDGE_TOL * (dx * dx + dy * dy))) { acc.lin = true; return; }
  const double i2 = ix * ix + iy * iy, j2 = jx * jx + jy * jy, d = 2.0 * a2;
  const double g0 = (jy * i2 - iy * j2) / d, g1 = (ix * j2 - jx * i2) / d;
  const double Ai = 0.5 * (cross2(g0, g1, ca0, ca1) + cross2(0.5 * ix, 0.5 * iy, g0, g1));
  const double Aj = 0.5 * (cross2(ca0, ca1, g0, g1) + cross2(g0, g1, 0.5 * jx, 0.5 * jy));
  acc.num += Ai * fi + Aj * fj;
  acc.den += Ai + Aj;
}

/* interior edge i -> j of a triangle (circumcentre ca - y) shared with a cavity neighbour (cb - y).  Without FMA
   contraction cross(cb, ca) = -cross(ca, cb) bit for bit: the edge adds the same bits from either side. */
__device__ __forceinline__ void nn_interior_edge(double ca0, double ca1, double cb0, double cb1, double fi, double fj, NnAcc &acc)
{
  const double e = 0.5 * cross2(cb0, cb1, ca0, ca1);
  acc.num += e * fi - e * fj;
}

/* One target per lane.  located[k] = the triangle the linear path found (-1: outside / NaN target), lin[k] = its
   piecewise-linear value; lin and values may be the same array (each lane reads its own entry before it writes it).
   The pending cavity triangles of a lane live in LDS (stk[level][lane]: conflict-free), the 2-bit entry-edge index of
   every level in one 64-bit register.  A lane whose stack would overflow `cap`, or that pops more than NN_MAX_POPS
   triangles, queues its target for natural_scan_kernel: todo[0] = count, todo[1 ..] = target indices. */
__global__ void __launch_bounds__(256)
natural_sweep_kernel(int n_tri, const NnRec *__restrict__ rec, const NnTab *__restrict__ tab, const int *__restrict__ located,
                     const double *lin, const double *__restrict__ targets, size_t m, size_t ttda, int cap, double *values,
                     unsigned *__restrict__ todo)
{
  __shared__ int stk[NN_STACK][256];
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= m) return;
  const double s0 = rec[n_tri].v[0][0], s1 = rec[n_tri].v[0][1];      /* the trailer record: the metric */
  const int lane = threadIdx.x;
  const int t0 = located[k];
  if (t0 < 0 || t0 >= n_tri) { values[k] = __longlong_as_double(0x7ff8000000000000LL); return; }
  const double y0 = targets[k * ttda] * s0, y1 = targets[k * ttda + 1] * s1;
  NnRec ra = nn_load(rec, t0);
  double f[3];
  nn_data(tab, t0, ra.meta, f);
#pragma unroll
  for (int i = 0; i < 3; i++)
    if (ra.v[i][0] - y0 == 0.0 && ra.v[i][1] - y1 == 0.0) { values[k] = f[i]; return; }
  if (NN_FLAT(ra.meta)) { values[k] = lin[k]; return; }
  NnAcc acc;
  acc.num = 0.0; acc.den = 0.0; acc.lin = false;
  bool queue = false;
  unsigned long long slots = 0;
  int sp = 0, cur = t0, entry = 3, pops = 0;
  for (;;) {
    const double ca0 = ra.c[0] + (ra.v[0][0] - y0), ca1 = ra.c[1] + (ra.v[0][1] - y1);
#pragma unroll
    for (int e = 0; e < 3; e++) {
      if (e == entry) continue;
      const int i = (e + 1) % 3, j = (e + 2) % 3;
      const int b = ra.nbr[e];
      bool in = false;
      NnRec rb;
      if (b >= 0 && b < n_tri) {
        rb = nn_load(rec, b);
        in = !NN_FLAT(rb.meta) && nn_incircle(rb, y0, y1);
      }
      if (in) {
        const int s = rb.nbr[0] == cur ? 0 : (rb.nbr[1] == cur ? 1 : (rb.nbr[2] == cur ? 2 : 3));
        if (s == 3 || sp >= cap) { queue = true; continue; }      /* links not mutual, or no room: the scan decides */
        nn_interior_edge(ca0, ca1, rb.c[0] + (rb.v[0][0] - y0), rb.c[1] + (rb.v[0][1] - y1), f[i], f[j], acc);
        stk[sp][lane] = b;
        slots = (slots << 2) | (unsigned long long)s;
        sp++;
      } else {
        nn_boundary_edge(ra.v[i][0] - y0, ra.v[i][1] - y1, ra.v[j][0] - y0, ra.v[j][1] - y1, ca0, ca1, f[i], f[j], acc);
      }
    }
    if (queue || acc.lin || sp == 0) break;
    if (++pops > NN_MAX_POPS) { queue = true; break; }
    sp--;
    cur = stk[sp][lane];
    entry = (int)(slots & 3ULL);
    slots >>= 2;
    ra = nn_load(rec, cur);
    nn_data(tab, cur, ra.meta, f);
  }
  if (acc.lin) { values[k] = lin[k]; return; }
  if (queue) {
    const unsigned slot = atomicAdd(&todo[0], 1u);
    todo[1 + slot] = (unsigned)k;
    return;
  }
  values[k] = acc.den > 0.0 ? acc.num / acc.den : lin[k];      /* den = the area of y's Voronoi cell */
}

/* One workgroup per queued target: every thread tests its share of ALL triangles with the same in-circle rule, adds
   the same edge terms (an interior edge once, from its smaller triangle; the neighbour is re-tested), and the 256
   partial sums are reduced in a fixed order.  The walk has already dealt with targets outside, on a site, or in a
   flat T0. */
__global__ void __launch_bounds__(256)
natural_scan_kernel(int n_tri, const NnRec *__restrict__ rec, const NnTab *__restrict__ tab, const int *__restrict__ located,
                    const double *lin, const double *__restrict__ targets, size_t ttda, double *values,
                    const unsigned *__restrict__ todo)
{
  __shared__ double s_num[256], s_den[256];
  __shared__ int s_lin;
  const double s0 = rec[n_tri].v[0][0], s1 = rec[n_tri].v[0][1];
  const unsigned count = todo[0];
  for (unsigned q = blockIdx.x; q < count; q += gridDim.x) {
    const size_t k = todo[1 + q];
    const int t0 = located[k];
    const double y0 = targets[k * ttda] * s0, y1 = targets[k * ttda + 1] * s1;
    if (threadIdx.x == 0) s_lin = 0;
    __syncthreads();
    NnAcc acc;
    acc.num = 0.0; acc.den = 0.0; acc.lin = false;
    for (int t = threadIdx.x; t < n_tri; t += blockDim.x) {
      const NnRec ra = nn_load(rec, t);
      if (!(t == t0 || (!NN_FLAT(ra.meta) && nn_incircle(ra, y0, y1)))) continue;
      double f[3];
      nn_data(tab, t, ra.meta, f);
      const double ca0 = ra.c[0] + (ra.v[0][0] - y0), ca1 = ra.c[1] + (ra.v[0][1] - y1);
#pragma unroll
      for (int e = 0; e < 3; e++) {
        const int i = (e + 1) % 3, j = (e + 2) % 3;
        const int b = ra.nbr[e];
        bool in = false;
        NnRec rb;
        if (b >= 0 && b < n_tri) {
          rb = nn_load(rec, b);
          in = b == t0 || (!NN_FLAT(rb.meta) && nn_incircle(rb, y0, y1));
        }
        if (in) {
          if (t < b) nn_interior_edge(ca0, ca1, rb.c[0] + (rb.v[0][0] - y0), rb.c[1] + (rb.v[0][1] - y1), f[i], f[j], acc);
        } else {
          nn_boundary_edge(ra.v[i][0] - y0, ra.v[i][1] - y1, ra.v[j][0] - y0, ra.v[j][1] - y1, ca0, ca1, f[i], f[j], acc);
        }
      }
    }
    s_num[threadIdx.x] = acc.num; s_den[threadIdx.x] = acc.den;
    if (acc.lin) atomicOr(&s_lin, 1);
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if ((int)threadIdx.x < w) { s_num[threadIdx.x] += s_num[threadIdx.x + w]; s_den[threadIdx.x] += s_den[threadIdx.x + w]; }
      __syncthreads();
    }
    if (threadIdx.x == 0) values[k] = (!s_lin && s_den[0] > 0.0) ? s_num[0] / s_den[0] : lin[k];
    __syncthreads();
  }
}

extern "C" int gsl_sinterp_hip_mesh_natural_pack(gsl_sinterp_hip_ctx *ctx, int n_tri, const int *d_tri, const int *d_nbr, int n_points,
                                                 const double *d_points, const double *h_metric, void *d_nnrec)
{
  REQUIRE(ctx, ctx != NULL, ST_EFAULT);
  HIP_OK(ctx, hipSetDevice(ctx->device));
  REQUIRE(ctx, n_tri > 0 && n_points >= 3, ST_EINVAL);
  REQUIRE(ctx, d_tri && d_nbr && d_points && h_metric && d_nnrec, ST_EFAULT);
  REQUIRE(ctx, ((uintptr_t)d_nnrec & 15) == 0, ST_EINVAL);
  REQUIRE(ctx, h_metric[0] > 0.0 && h_metric[1] > 0.0 && h_metric[0] < INFINITY && h_metric[1] < INFINITY, ST_EINVAL);
  hipLaunchKernelGGL(natural_pack_kernel, dim3(n_tri / 256 + 1), dim3(256), 0, ctx->stream, n_tri, d_tri, d_nbr, n_points, d_points,
                     h_metric[0], h_metric[1], (NnRec *)d_nnrec);
  LAUNCH_CHECK(ctx);
  return ST_SUCCESS;
}

extern "C" int gsl_sinterp_hip_mesh_natural_eval(gsl_sinterp_hip_ctx *ctx, int n_tri, const void *d_nnrec, const void *d_leaftab,
                                                 const int *d_located, const double *d_linear_values, const double *d_targets, size_t m,
                                                 size_t ttda, int depth_cap, double *d_values, long long *h_n_scanned)
{
  REQUIRE(ctx, ctx != NULL, ST_EFAULT);
  HIP_OK(ctx, hipSetDevice(ctx->device));
  REQUIRE(ctx, n_tri > 0 && ttda >= 2 && depth_cap >= 0, ST_EINVAL);
  REQUIRE(ctx, d_nnrec && d_leaftab && (m == 0 || (d_located && d_linear_values && d_targets && d_values)), ST_EFAULT);
  REQUIRE(ctx, ((uintptr_t)d_nnrec & 15) == 0, ST_EINVAL);
  if (h_n_scanned) *h_n_scanned = 0;
  if (m == 0) return ST_SUCCESS;
  REQUIRE(ctx, m < 0xffffffffULL, ST_EINVAL);
  const int cap = depth_cap == 0 || depth_cap > NN_STACK ? NN_STACK : depth_cap;
  void *buf = NULL;
  int st = sinterp_walkbuf(ctx, (m + 1) * sizeof(unsigned), &buf);       /* queue of the scan */
  if (st) return st;
  unsigned *todo = (unsigned *)buf;
  HIP_OK(ctx, hipMemsetAsync(todo, 0, sizeof(unsigned), ctx->stream));
  hipLaunchKernelGGL(natural_sweep_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, ctx->stream, n_tri, (const NnRec *)d_nnrec,
                     (const NnTab *)d_leaftab, d_located, d_linear_values, d_targets, m, ttda, cap, d_values, todo);
  hipLaunchKernelGGL(natural_scan_kernel, dim3(256), dim3(256), 0, ctx->stream, n_tri, (const NnRec *)d_nnrec, (const NnTab *)d_leaftab,
                     d_located, d_linear_values, d_targets, ttda, d_values, (const unsigned *)todo);
  LAUNCH_CHECK(ctx);
  if (h_n_scanned) {
    unsigned c = 0;
    HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
    HIP_OK(ctx, hipMemcpy(&c, todo, sizeof c, hipMemcpyDeviceToHost));
    *h_n_scanned = (long long)c;
  }
  return ST_SUCCESS;
}
