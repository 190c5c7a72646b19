/*
 * mesh3.hip -- imported tetrahedral meshes: piecewise-linear interpolation in 3-D.
 * Compiled with -ffp-contract=off like bary.hip: a coordinate or a value is the same sequence of separately rounded
 * fp64 operations wherever it is computed (walk, scan, final value), so the result of a target does not depend on the
 * route that found its tetrahedron.
 *
 * The 3-D twin of bary.hip's "Imported triangulations": QHull / CGAL arrays (simplices [4 n], neighbours [4 n],
 * neighbour k across the face opposite vertex k, -1 on the hull), located by a grid seed and a walk over the neighbour
 * links.  The reference has no 3-D path to restate (its flip logic aborts): PARITY UNPINNED; the
 * conventions (standardisation, closed containment rule, least violating simplex, MESH_GAP) are the 2-D path's.
 *
 * HBM layout: one 128-byte, 128-byte-aligned record per tetrahedron
 *     x[3]      standardised coordinates of the LAST vertex (the origin of the barycentric frame)
 *     inv[9]    inverse of the standardised 3x3 edge matrix [v0 - v3 | v1 - v3 | v2 - v3], row-major, formed once
 *     nbr[4]    neighbour across the face opposite vertex k, -1 = hull
 *     meta      bit 0: singular (flat or not finite): such a record never contains a target
 * so a containment test is 3 subtractions and 9 multiplications + 6 additions, c3 = 1 - (c0 + c1 + c2): no divide
 * on the walk.  A separate 32-byte table {f(v0) .. f(v3)} is bound to one response column and read once per target.
 */
#include "common.h"
#include "linear_finish.h"   /* TetRec, load_tet, tet_coords, TET_INTERP: shared with linear_fields.hip */
#include <math.h>
#include <stdlib.h>

struct __attribute__((aligned(32))) TetTab { double f[4]; };
static_assert(sizeof(TetTab) == GSL_SINTERP_MESH3_TABLE_BYTES, "response table size");

#define MESH3_SINGULAR_REL 1e-12   /* |det| <= this x the product of the three edge lengths: flat */
#define MESH3_SEED_RINGS 4         /* empty seed cells look this many shells of cells around themselves */
#define MESH3_EXTRA_STEPS 8        /* steps the walk still takes after it has seen a violation <= MESH_GAP */

struct Mesh3Geom { double shift[3], scale[3]; };
struct Mesh3Grid { double lo[3], w[3]; int G; };

/* ------------------------------------------------------------------------ */
__global__ void mesh3_pack_kernel(int n_tet, const int *__restrict__ tet, const int *__restrict__ nbr, int n_points,
                                  const double *__restrict__ points, Mesh3Geom g, TetRec *__restrict__ rec)
{
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_tet) return;
  double v[4][3];
  bool ids_ok = true;
  for (int i = 0; i < 4; i++) {
    const int id = tet[4 * t + i];
    const bool ok = id >= 0 && id < n_points;
    ids_ok = ids_ok && ok;
    for (int j = 0; j < 3; j++) v[i][j] = ok ? g.scale[j] * (points[3 * (size_t)id + j] - g.shift[j]) : 0.0;
  }
  double e[3][3];                                   /* e[i] = v_i - v_3, the columns of the edge matrix */
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) e[i][j] = v[i][j] - v[3][j];
  /* cofactors: rows of the inverse are (e1 x e2, e2 x e0, e0 x e1) / det */
  double c[3][3];
  for (int i = 0; i < 3; i++) {
    const double *a = e[(i + 1) % 3], *b = e[(i + 2) % 3];
    c[i][0] = a[1] * b[2] - a[2] * b[1];
    c[i][1] = a[2] * b[0] - a[0] * b[2];
    c[i][2] = a[0] * b[1] - a[1] * b[0];
  }
  const double det = e[0][0] * c[0][0] + e[0][1] * c[0][1] + e[0][2] * c[0][2];
  double len = 1.0;
  for (int i = 0; i < 3; i++) len *= sqrt(e[i][0] * e[i][0] + e[i][1] * e[i][1] + e[i][2] * e[i][2]);
  const bool singular = !ids_ok || !(fabs(det) <= 1.79769313486231570815e+308) || !(fabs(det) > MESH3_SINGULAR_REL * len);
  TetRec r;
  for (int j = 0; j < 3; j++) r.x[j] = v[3][j];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) r.inv[3 * i + j] = singular ? 0.0 : c[i][j] / det;
  for (int i = 0; i < 4; i++) {
    const int nb = nbr[4 * t + i];
    r.nbr[i] = (nb >= 0 && nb < n_tet) ? nb : -1;   /* the walk indexes with these */
  }
  r.meta = singular ? 1 : 0;
  r.pad[0] = r.pad[1] = r.pad[2] = 0;
  rec[t] = r;
}

__global__ void mesh3_bind_kernel(int n_tet, const int *__restrict__ tet, int n_points, const double *__restrict__ response,
                                  TetTab *__restrict__ tab)
{
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_tet) return;
  TetTab r;
  for (int i = 0; i < 4; i++) {
    const int id = tet[4 * t + i];
    r.f[i] = (id >= 0 && id < n_points) ? response[id] : 0.0;
  }
  tab[t] = r;
}

/* the closed rule: all four coordinates in [0, 1] (false on NaN) */
__device__ __forceinline__ bool tet_inside(const double c[4])
{
  return c[0] >= 0 && c[0] <= 1 && c[1] >= 0 && c[1] <= 1 && c[2] >= 0 && c[2] <= 1 && c[3] >= 0 && c[3] <= 1;
}

/* bary.hip's violation() in four coordinates: how far the worst coordinate lies outside [0, 1] */
__device__ __forceinline__ double tet_violation(const double c[4])
{
  double worst = 0;
  for (int i = 0; i < 4; i++) {
    if ((c[i] < 0) && (-c[i] > worst)) worst = -c[i];
    else if ((c[i] > 1) && (c[i] - 1 > worst)) worst = c[i] - 1;
  }
  return worst;
}

__device__ __forceinline__ void tet_finish(const TetRec &r, const TetTab *__restrict__ tab, int t, const double z[3], size_t k,
                                           double *__restrict__ values, int *__restrict__ tet_out, int packed)
{
  double c[4];
  tet_coords(r, z, c);
  const double4 f = *reinterpret_cast<const double4 *>(tab + t);
  const double v = TET_INTERP(c, f.x, f.y, f.z, f.w);
  store_result(values, tet_out, k, v, t, packed);
}

/* ------------------------------------------------------------------------ */
/* seed grid: G x G x G cells over the points' bounding box */
__device__ __forceinline__ int mesh3_cell(const Mesh3Grid &g, double y0, double y1, double y2)
{
  const double top = (double)(g.G - 1);
  const int ix = (y0 == y0 && g.w[0] > 0.0) ? (int)fmin(fmax((y0 - g.lo[0]) / g.w[0], 0.0), top) : 0;
  const int iy = (y1 == y1 && g.w[1] > 0.0) ? (int)fmin(fmax((y1 - g.lo[1]) / g.w[1], 0.0), top) : 0;
  const int iz = (y2 == y2 && g.w[2] > 0.0) ? (int)fmin(fmax((y2 - g.lo[2]) / g.w[2], 0.0), top) : 0;
  return (iz * g.G + iy) * g.G + ix;
}

__global__ void mesh3_seed_init_kernel(int *__restrict__ seed, size_t cells)
{
  const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c < cells) seed[c] = -1;
}

/* cell -> the largest index of a non-singular tetrahedron whose centroid lies in it (atomicMax: deterministic);
   seed[cells] -> the largest non-singular index of all, where the fill sends a cell with nothing around it */
__global__ void __launch_bounds__(256)
mesh3_seed_kernel(int n_tet, const int *__restrict__ tet, const TetRec *__restrict__ rec, int n_points,
                  const double *__restrict__ points, Mesh3Grid g, size_t cells, int *__restrict__ seed)
{
  __shared__ int s_max;
  if (threadIdx.x == 0) s_max = -1;
  __syncthreads();
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n_tet && !TET_SINGULAR(rec[t].meta)) {    /* singular also covers a vertex id out of range */
    double c[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < 4; i++) {
      const int v = tet[4 * t + i];
      for (int j = 0; j < 3; j++) c[j] += points[3 * (size_t)v + j];
    }
    atomicMax(&seed[mesh3_cell(g, c[0] / 4.0, c[1] / 4.0, c[2] / 4.0)], t);
    atomicMax(&s_max, t);
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_max >= 0) atomicMax(&seed[cells], s_max);
}

/* empty cells take the first filled cell of the surrounding shells, in a fixed order: deterministic */
__global__ void mesh3_seed_fill_kernel(const int *__restrict__ seed_in, int *__restrict__ seed_out, int G)
{
  const size_t cells = (size_t)G * G * G;
  const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cells) return;
  int s = seed_in[c];
  const int cx = (int)(c % G), cy = (int)((c / G) % G), cz = (int)(c / ((size_t)G * G));
  for (int r = 1; r <= MESH3_SEED_RINGS && s < 0; r++)
    for (int dz = -r; dz <= r && s < 0; dz++)
      for (int dy = -r; dy <= r && s < 0; dy++)
        for (int dx = -r; dx <= r && s < 0; dx++) {
          if (abs(dx) != r && abs(dy) != r && abs(dz) != r) continue;
          const int x = cx + dx, y = cy + dy, z = cz + dz;
          if (x < 0 || y < 0 || z < 0 || x >= G || y >= G || z >= G) continue;
          s = seed_in[((size_t)z * G + y) * G + x];
        }
  if (s < 0) s = seed_in[cells];                    /* nothing nearby: any non-singular tetrahedron */
  seed_out[c] = s < 0 ? 0 : s;                      /* a mesh of flat tetrahedra only: the walk hands over to the scan */
}

/* ------------------------------------------------------------------------ */
/* Walk: one target per lane.  todo: [0] = count, [1..] = indices of the targets left to the exhaustive scan; packed:
   store_result's modes (batches of >= 4096 targets arrive in cell order: neighbouring lanes start from neighbouring seeds
   and walk through the same few tetrahedra, whose 128-byte records the wave then shares).

   In 3-D a target within rounding of an edge or a vertex can fail the closed test of every tetrahedron around it and
   circle through them, so the walk carries the least violating tetrahedron seen so far (smaller index on a tie); from
   the first violation <= MESH_GAP on it takes MESH3_EXTRA_STEPS further steps and, if no containing tetrahedron turns
   up, accepts that best one.  Everything is a function of (mesh, target): no state shared between lanes. */
__global__ void __launch_bounds__(256)
mesh3_walk_kernel(int n_tet, const TetRec *__restrict__ rec, const TetTab *__restrict__ tab, const int *__restrict__ seed,
                  Mesh3Grid g, Mesh3Geom geo, int convex, int max_steps, const double *__restrict__ targets, size_t m, size_t ttda,
                  double *__restrict__ values, int *__restrict__ tet_out, unsigned long long *__restrict__ n_outside,
                  unsigned *__restrict__ todo, int packed)
{
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= m) return;
  const double y0 = targets[k * ttda], y1 = targets[k * ttda + 1], y2 = targets[k * ttda + 2];
  const double z[3] = {geo.scale[0] * (y0 - geo.shift[0]), geo.scale[1] * (y1 - geo.shift[1]), geo.scale[2] * (y2 - geo.shift[2])};
  int t = seed[mesh3_cell(g, y0, y1, y2)];
  int found = -2;                                              /* -2 walking, -1 outside, -3 exhaustive scan */
  if (!(y0 == y0 && y1 == y1 && y2 == y2)) found = -1;         /* NaN target: outside, like the 2-D path */
  TetRec cur;
  int cur_t = -1;                                              /* whose record cur holds */
  int best = -1, extra = 0;
  double best_viol = INFINITY;
  for (int step = 0; found == -2; step++) {
    if (step >= max_steps || t < 0 || t >= n_tet) break;
    cur = load_tet(rec, t);
    cur_t = t;
    if (TET_SINGULAR(cur.meta)) { found = -3; break; }         /* a walk that arrives at a flat tetrahedron: the scan decides */
    double c[4];
    tet_coords(cur, z, c);
    if (tet_inside(c)) { found = t; break; }
    if (!(c[0] == c[0] && c[1] == c[1] && c[2] == c[2] && c[3] == c[3])) { found = -3; break; }
    const double viol = tet_violation(c);
    if (viol < best_viol || (viol == best_viol && t < best)) { best_viol = viol; best = t; }
    if (best_viol <= MESH_GAP && ++extra > MESH3_EXTRA_STEPS) break;
    /* the face to cross: opposite the most negative coordinate that has a neighbour (the first of equal ones) */
    int next = -1;
    double low = 0.0, lowest = 0.0;
    for (int i = 0; i < 4; i++) {
      if (c[i] < lowest) lowest = c[i];
      if (c[i] < 0.0 && cur.nbr[i] >= 0 && (next < 0 || c[i] < low)) { low = c[i]; next = cur.nbr[i]; }
    }
    if (next < 0) {                                            /* only hull faces in the way */
      if (best_viol > MESH_GAP) found = (lowest < 0.0 && convex) ? -1 : -3;
      break;
    }
    t = next;
  }
  if (found == -2) found = best_viol <= MESH_GAP ? best : -3;  /* budget spent, hull reached or step bound: the best seen, if it is one */
  if (found >= 0) {
    if (found != cur_t) cur = load_tet(rec, found);
    tet_finish(cur, tab, found, z, k, values, tet_out, packed);
    return;
  }
  if (found == -3) {
    const unsigned slot = atomicAdd(&todo[0], 1u);
    todo[1 + slot] = (unsigned)k;
    return;
  }
  store_result(values, tet_out, k, __longlong_as_double(0x7ff8000000000000LL), -1, packed);
  atomicAdd(n_outside, 1ULL);
}

/* exhaustive scan: one workgroup per queued target; the least violating non-singular tetrahedron (0 = containing),
   smallest index on a tie, accepted up to MESH_GAP */
__global__ void __launch_bounds__(256)
mesh3_scan_kernel(int n_tet, const TetRec *__restrict__ rec, const TetTab *__restrict__ tab, Mesh3Geom geo,
                  const double *__restrict__ targets, size_t ttda, double *__restrict__ values, int *__restrict__ tet_out,
                  unsigned long long *__restrict__ n_outside, const unsigned *__restrict__ todo, int packed)
{
  __shared__ unsigned long long s_viol;
  __shared__ int s_best;
  const unsigned count = todo[0];
  for (unsigned q = blockIdx.x; q < count; q += gridDim.x) {
    const size_t k = todo[1 + q];
    const double z[3] = {geo.scale[0] * (targets[k * ttda] - geo.shift[0]), geo.scale[1] * (targets[k * ttda + 1] - geo.shift[1]),
                         geo.scale[2] * (targets[k * ttda + 2] - geo.shift[2])};
    if (threadIdx.x == 0) { s_viol = ~0ULL; s_best = 0x7fffffff; }
    __syncthreads();
    double my_viol = INFINITY;
    int my_t = 0x7fffffff;
    for (int t = threadIdx.x; t < n_tet; t += blockDim.x) {
      const TetRec r = load_tet(rec, t);
      double c[4];
      tet_coords(r, z, c);
      if (TET_SINGULAR(r.meta) || !(c[0] == c[0] && c[1] == c[1] && c[2] == c[2] && c[3] == c[3])) continue;
      const double viol = tet_inside(c) ? 0.0 : tet_violation(c);
      if (viol < my_viol) { my_viol = viol; my_t = t; }          /* ascending t: the first of equal violations stays */
    }
    if (my_t != 0x7fffffff) atomicMin(&s_viol, (unsigned long long)__double_as_longlong(my_viol));   /* viol >= 0: bits ordered */
    __syncthreads();
    if (my_t != 0x7fffffff && (unsigned long long)__double_as_longlong(my_viol) == s_viol) atomicMin(&s_best, my_t);
    __syncthreads();
    if (threadIdx.x == 0) {
      const int t = s_best;
      if (t != 0x7fffffff && __longlong_as_double((long long)s_viol) <= MESH_GAP) tet_finish(load_tet(rec, t), tab, t, z, k, values, tet_out, packed);
      else {
        store_result(values, tet_out, k, __longlong_as_double(0x7ff8000000000000LL), -1, packed);
        atomicAdd(n_outside, 1ULL);
      }
    }
    __syncthreads();
  }
}

/* ------------------------------------------------------------------------ */
static Mesh3Grid mesh3_grid(const double *h_geom, int G)
{
  Mesh3Grid mg;
  for (int j = 0; j < 3; j++) { mg.lo[j] = h_geom[6 + j]; mg.w[j] = (h_geom[9 + j] - h_geom[6 + j]) / G; }
  mg.G = G;
  return mg;
}

static Mesh3Geom mesh3_geom(const double *h_geom)
{
  Mesh3Geom g;
  for (int j = 0; j < 3; j++) { g.shift[j] = h_geom[j]; g.scale[j] = h_geom[3 + j]; }
  return g;
}

/* h_geom[12] = shift(3), scale(3), bounding box of the points lo(3), hi(3); d_seed: 2 G^3 + 2 ints */
extern "C" int gsl_sinterp_hip_mesh3_pack(gsl_sinterp_hip_ctx *ctx, int n_tet, const int *d_tet, const int *d_nbr, int n_points,
                                          const double *d_points, const double *h_geom, int G, void *d_records, int *d_seed)
{
  REQUIRE(ctx, ctx != NULL, ST_EFAULT);
  HIP_OK(ctx, hipSetDevice(ctx->device));
  REQUIRE(ctx, n_tet > 0 && n_points >= 4 && G >= 1 && G <= GSL_SINTERP_MESH3_MAX_GRID, ST_EINVAL);
  REQUIRE(ctx, d_tet && d_nbr && d_points && h_geom && d_records && d_seed, ST_EFAULT);
  REQUIRE(ctx, ((uintptr_t)d_records & 127) == 0, ST_EINVAL);
  hipLaunchKernelGGL(mesh3_pack_kernel, dim3((n_tet + 255) / 256), dim3(256), 0, ctx->stream, n_tet, d_tet, d_nbr, n_points, d_points,
                     mesh3_geom(h_geom), (TetRec *)d_records);
  const size_t cells = (size_t)G * G * G;
  int *raw = d_seed + cells;                                   /* [cells] per-cell maxima + [1] the maximum of all */
  hipLaunchKernelGGL(mesh3_seed_init_kernel, dim3((unsigned)((cells + 1 + 255) / 256)), dim3(256), 0, ctx->stream, raw, cells + 1);
  hipLaunchKernelGGL(mesh3_seed_kernel, dim3((n_tet + 255) / 256), dim3(256), 0, ctx->stream, n_tet, d_tet, (const TetRec *)d_records,
                     n_points, d_points, mesh3_grid(h_geom, G), cells, raw);
  hipLaunchKernelGGL(mesh3_seed_fill_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, ctx->stream, (const int *)raw, d_seed, G);
  LAUNCH_CHECK(ctx);
  return ST_SUCCESS;
}

extern "C" int gsl_sinterp_hip_mesh3_bind(gsl_sinterp_hip_ctx *ctx, int n_tet, const int *d_tet, int n_points,
                                          const double *d_response, void *d_table)
{
  REQUIRE(ctx, ctx != NULL, ST_EFAULT);
  HIP_OK(ctx, hipSetDevice(ctx->device));
  REQUIRE(ctx, n_tet > 0 && n_points >= 4, ST_EINVAL);
  REQUIRE(ctx, d_tet && d_response && d_table, ST_EFAULT);
  REQUIRE(ctx, ((uintptr_t)d_table & 31) == 0, ST_EINVAL);
  hipLaunchKernelGGL(mesh3_bind_kernel, dim3((n_tet + 255) / 256), dim3(256), 0, ctx->stream, n_tet, d_tet, n_points, d_response,
                     (TetTab *)d_table);
  LAUNCH_CHECK(ctx);
  return ST_SUCCESS;
}

extern "C" int gsl_sinterp_hip_mesh3_eval(gsl_sinterp_hip_ctx *ctx, int n_tet, const void *d_records, const void *d_table,
                                          const int *d_seed, int G, const double *h_geom, int convex, const double *d_targets,
                                          size_t m, size_t ttda, double *d_values, int *d_tet, long long *h_n_outside)
{
  REQUIRE(ctx, ctx != NULL, ST_EFAULT);
  HIP_OK(ctx, hipSetDevice(ctx->device));
  REQUIRE(ctx, n_tet > 0 && ttda >= 3 && G >= 1 && G <= GSL_SINTERP_MESH3_MAX_GRID, ST_EINVAL);
  REQUIRE(ctx, d_records && d_table && d_seed && h_geom && (m == 0 || (d_targets && d_values)), ST_EFAULT);
  if (h_n_outside) *h_n_outside = 0;
  if (m == 0) return ST_SUCCESS;
  REQUIRE(ctx, m < 0xffffffffULL, ST_EINVAL);
  unsigned long long *d_count = (unsigned long long *)ctx->d_scratch;
  HIP_OK(ctx, hipMemsetAsync(d_count, 0, sizeof(unsigned long long), ctx->stream));
  void *buf = NULL;
  int st = sinterp_walkbuf(ctx, (m + 1) * sizeof(unsigned), &buf);      /* queue of the exhaustive scan */
  if (st) return st;
  unsigned *todo = (unsigned *)buf;
  HIP_OK(ctx, hipMemsetAsync(todo, 0, sizeof(unsigned), ctx->stream));
  /* batches of >= 4096 targets: the 2-D path's reorder (cell order, two-level from 2^18 targets), results through the
     order's map, un-sorted afterwards.  A result depends on (mesh, target) only: same bits either way. */
  sinterp_route r;
  st = sinterp_route_begin(ctx, d_targets, m, ttda, 3, 64, (const unsigned long long *)NULL, d_values, d_tet, sinterp_sort_wanted(m), &r);
  if (st) return st;
  /* a straight walk from a grid seed crosses a handful of tetrahedra; the bound only guards against cycles and long
     detours in badly shaped (non-Delaunay) input: whatever exceeds it without a best violation <= MESH_GAP is scanned */
  const int max_steps = 64 + 6 * G;
  const Mesh3Geom geo = mesh3_geom(h_geom);
  hipLaunchKernelGGL(mesh3_walk_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, ctx->stream, n_tet, (const TetRec *)d_records,
                     (const TetTab *)d_table, d_seed, mesh3_grid(h_geom, G), geo, convex, max_steps, r.y, m, r.ytda, r.values, r.leaf,
                     d_count, todo, r.packed);
  hipLaunchKernelGGL(mesh3_scan_kernel, dim3(256), dim3(256), 0, ctx->stream, n_tet, (const TetRec *)d_records, (const TetTab *)d_table,
                     geo, r.y, r.ytda, r.values, r.leaf, d_count, (const unsigned *)todo, r.packed);
  LAUNCH_CHECK(ctx);
  st = sinterp_route_end(ctx, &r, m, d_values, d_tet);
  if (st) return st;
  return sinterp_outside_count(ctx, d_count, h_n_outside, "mesh3_eval: %llu target(s) outside the tetrahedral mesh");
}
