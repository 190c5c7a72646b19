/*
 * simplex_mesh.c -- imported triangulations: QHull / CGAL style arrays (points, triangles, neighbours) instead of
 * the history DAG that simplex_tree_init builds.  The reference lists this as future work (README:28-31); what it
 * fixes is the per-triangle arithmetic -- calculate_bary_coords / contains_point / interp_point
 * (interpolation/linear_simplex.c:607-711) -- and the link convention of a leaf (linear_simplex.h:62-63: link i =
 * neighbour opposite vertex i), both kept here.  All evaluation runs on the GPU (csrc/hip/bary.hip, "Imported
 * triangulations"); this file validates, derives neighbour links when they are not given, and mirrors the arrays.
 * The same arrays in 3-D (tetrahedra: simplices [4 n], neighbour k across the face opposite vertex k) are imported by
 * simplex_mesh_import_nd and evaluated by csrc/hip/mesh3.hip; there the reference has nothing to restate (its 3-D
 * build aborts), so only the conventions are carried over.
 */
#include "gsl_sinterp.h"
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

struct simplex_mesh {
  size_t n_tri, n_points, dim;   /* dim = 2 (triangles) or 3 (tetrahedra) */
  int *tri, *nbr;        /* [(dim + 1) n_tri] */
  int *node;             /* [n_tri] DAG node (from_tree) or NULL */
  double *points;        /* [dim n_points], row order, packed */
  double shift[3], scale[3], lo[3], hi[3];
  int convex;
};

void simplex_mesh_free(simplex_mesh *mesh)
{
  if (!mesh) return;
  free(mesh->tri); free(mesh->nbr); free(mesh->node); free(mesh->points);
  free(mesh);
}

size_t simplex_mesh_n_triangles(const simplex_mesh *mesh) { return mesh ? mesh->n_tri : 0; }
size_t simplex_mesh_n_points(const simplex_mesh *mesh) { return mesh ? mesh->n_points : 0; }
size_t simplex_mesh_dim(const simplex_mesh *mesh) { return mesh ? mesh->dim : 0; }
const int *simplex_mesh_triangles(const simplex_mesh *mesh) { return mesh ? mesh->tri : NULL; }
const int *simplex_mesh_neighbours(const simplex_mesh *mesh) { return mesh ? mesh->nbr : NULL; }
const int *simplex_mesh_tree_nodes(const simplex_mesh *mesh) { return mesh ? mesh->node : NULL; }
void simplex_mesh_set_convex(simplex_mesh *mesh, int convex) { if (mesh) mesh->convex = convex != 0; }
int simplex_mesh_convex(const simplex_mesh *mesh) { return mesh ? mesh->convex : 0; }
const double *simplex_mesh_points(const simplex_mesh *mesh) { return mesh ? mesh->points : NULL; }
void simplex_mesh_bbox(const simplex_mesh *mesh, double *lo, double *hi)
{
  for (size_t j = 0; j < mesh->dim; j++) { lo[j] = mesh->lo[j]; hi[j] = mesh->hi[j]; }
}
void simplex_mesh_geometry(const simplex_mesh *mesh, double *shift, double *scale)
{
  for (size_t j = 0; j < mesh->dim; j++) { shift[j] = mesh->shift[j]; scale[j] = mesh->scale[j]; }
}

static simplex_mesh *mesh_alloc(size_t nt, size_t np, int with_nodes, size_t dim)
{
  simplex_mesh *m = (simplex_mesh *)calloc(1, sizeof *m);
  if (!m) return NULL;
  m->n_tri = nt; m->n_points = np; m->dim = dim; m->convex = 1;
  m->tri = (int *)malloc((dim + 1) * nt * sizeof(int));
  m->nbr = (int *)malloc((dim + 1) * nt * sizeof(int));
  m->points = (double *)malloc(dim * np * sizeof(double));
  if (with_nodes) m->node = (int *)malloc(nt * sizeof(int));
  if (!m->tri || !m->nbr || !m->points || (with_nodes && !m->node)) { simplex_mesh_free(m); return NULL; }
  return m;
}

static void mesh_bbox(simplex_mesh *m)
{
  const size_t d = m->dim;
  for (size_t j = 0; j < d; j++) { m->lo[j] = m->points[j]; m->hi[j] = m->points[j]; }
  for (size_t r = 1; r < m->n_points; r++)
    for (size_t j = 0; j < d; j++) {
      const double v = m->points[d * r + j];
      if (v < m->lo[j]) m->lo[j] = v;
      if (v > m->hi[j]) m->hi[j] = v;
    }
}

/* neighbour links by edge matching: every edge (a, b), a < b, with the triangle and the slot opposite to it, sorted */
typedef struct { int a, b, t, slot; } mesh_edge;
static int edge_cmp(const void *x, const void *y)
{
  const mesh_edge *p = (const mesh_edge *)x, *q = (const mesh_edge *)y;
  if (p->a != q->a) return p->a < q->a ? -1 : 1;
  if (p->b != q->b) return p->b < q->b ? -1 : 1;
  return p->t < q->t ? -1 : (p->t > q->t);
}

static int derive_neighbours(simplex_mesh *m)
{
  const size_t ne = 3 * m->n_tri;
  mesh_edge *e = (mesh_edge *)malloc(ne * sizeof *e);
  if (!e) return GSL_ENOMEM;
  for (size_t t = 0; t < m->n_tri; t++)
    for (int k = 0; k < 3; k++) {
      const int u = m->tri[3 * t + (k + 1) % 3], v = m->tri[3 * t + (k + 2) % 3];   /* the edge opposite vertex k */
      mesh_edge *x = &e[3 * t + k];
      x->a = u < v ? u : v; x->b = u < v ? v : u; x->t = (int)t; x->slot = k;
    }
  qsort(e, ne, sizeof *e, edge_cmp);
  for (size_t i = 0; i < 3 * m->n_tri; i++) m->nbr[i] = -1;
  int status = GSL_SUCCESS;
  for (size_t i = 0; i < ne;) {
    size_t j = i + 1;
    while (j < ne && e[j].a == e[i].a && e[j].b == e[i].b) j++;
    if (j - i == 2) {
      m->nbr[3 * e[i].t + e[i].slot] = e[i + 1].t;
      m->nbr[3 * e[i + 1].t + e[i + 1].slot] = e[i].t;
    } else if (j - i > 2) status = GSL_EINVAL;          /* an edge shared by three triangles: not a triangulation */
    i = j;
  }
  free(e);
  return status;
}

/* Convexity of an imported mesh, decided from its boundary (the edges without a neighbour): convex = ONE closed loop
   whose turns all have the sign of the loop's orientation (collinear boundary points allowed).  A hole, a concave
   outline, several components or a non-manifold boundary vertex all answer 0, and the locate step then never takes a
   boundary edge in the walking direction as proof that the target lies outside (exhaustive scan instead). */
static int mesh_detect_convex(const simplex_mesh *m)
{
  const size_t np = m->n_points, nt = m->n_tri;
  int *next = (int *)malloc(np * sizeof(int));
  if (!next) return 0;
  for (size_t i = 0; i < np; i++) next[i] = -1;
  size_t n_edges = 0;
  int first = -1, ok = 1;
  for (size_t t = 0; t < nt && ok; t++) {
    const int *v = m->tri + 3 * t;
    const double *p0 = m->points + 2 * v[0], *p1 = m->points + 2 * v[1], *p2 = m->points + 2 * v[2];
    const double orient = (p1[0] - p0[0]) * (p2[1] - p0[1]) - (p1[1] - p0[1]) * (p2[0] - p0[0]);
    for (int k = 0; k < 3; k++) {
      if (m->nbr[3 * t + k] >= 0) continue;
      int a = v[(k + 1) % 3], b = v[(k + 2) % 3];               /* the edge opposite vertex k, in the triangle's order */
      if (orient < 0) { const int tmp = a; a = b; b = tmp; }    /* walk every boundary edge counter-clockwise */
      if (next[a] >= 0) { ok = 0; break; }                      /* two boundary edges leave one vertex: not a simple loop */
      next[a] = b;
      if (first < 0) first = a;
      n_edges++;
    }
  }
  if (ok && (first < 0 || n_edges < 3)) ok = 0;
  if (ok) {
    size_t seen = 0;
    int a = first;
    do {
      const int b = next[a];
      if (b < 0 || next[b] < 0) { ok = 0; break; }
      const int c = next[b];
      const double *pa = m->points + 2 * a, *pb = m->points + 2 * b, *pc = m->points + 2 * c;
      const double ux = pb[0] - pa[0], uy = pb[1] - pa[1], wx = pc[0] - pb[0], wy = pc[1] - pb[1];
      const double cross = ux * wy - uy * wx, tol = 1e-12 * sqrt((ux * ux + uy * uy) * (wx * wx + wy * wy));
      if (cross < -tol) { ok = 0; break; }                      /* a right turn on a counter-clockwise loop: concave */
      a = b;
      seen++;
    } while (a != first && seen <= n_edges);
    if (ok && (a != first || seen != n_edges)) ok = 0;          /* more boundary edges than this loop: holes / components */
  }
  free(next);
  return ok;
}

simplex_mesh *simplex_mesh_import(const gsl_matrix *points, const int *triangles, const int *neighbours, size_t n_triangles)
{
  if (!points || !triangles) GSL_ERROR_NULL("simplex_mesh_import: null argument", GSL_EFAULT);
  if (points->size2 < 2 || points->size1 < 3 || n_triangles < 1 || n_triangles > (size_t)INT_MAX / 3 || points->size1 > (size_t)INT_MAX)
    GSL_ERROR_NULL("simplex_mesh_import: need >= 3 points with 2 coordinates and >= 1 triangle", GSL_EINVAL);
  const size_t np = points->size1;
  for (size_t i = 0; i < 3 * n_triangles; i++) {
    if (triangles[i] < 0 || (size_t)triangles[i] >= np) GSL_ERROR_NULL("simplex_mesh_import: vertex id out of range", GSL_EINVAL);
    if (neighbours && (neighbours[i] < -1 || neighbours[i] >= (int)n_triangles))
      GSL_ERROR_NULL("simplex_mesh_import: neighbour id out of range", GSL_EINVAL);
  }
  for (size_t t = 0; t < n_triangles; t++)
    if (triangles[3 * t] == triangles[3 * t + 1] || triangles[3 * t] == triangles[3 * t + 2] || triangles[3 * t + 1] == triangles[3 * t + 2])
      GSL_ERROR_NULL("simplex_mesh_import: triangle with a repeated vertex", GSL_EINVAL);
  simplex_mesh *m = mesh_alloc(n_triangles, np, 0, 2);
  if (!m) GSL_ERROR_NULL("simplex_mesh_import: out of memory", GSL_ENOMEM);
  memcpy(m->tri, triangles, 3 * n_triangles * sizeof(int));
  for (size_t r = 0; r < np; r++) { m->points[2 * r] = points->data[r * points->tda]; m->points[2 * r + 1] = points->data[r * points->tda + 1]; }
  mesh_bbox(m);
  /* the standardisation simplex_tree_init would use for these points (linear_simplex.c:226-247 as restated in
     simplex_tree.c): centre of the bounding box, 1 / extent */
  for (int j = 0; j < 2; j++) {
    m->shift[j] = (m->lo[j] + m->hi[j]) / 2.0;
    m->scale[j] = (m->hi[j] - m->lo[j] <= 0) ? 1.0 : 1.0 / (m->hi[j] - m->lo[j]);
  }
  if (neighbours) {
    memcpy(m->nbr, neighbours, 3 * n_triangles * sizeof(int));
    /* every link must be answered by the neighbour, across the same edge */
    for (size_t t = 0; t < n_triangles; t++)
      for (int k = 0; k < 3; k++) {
        const int nb = m->nbr[3 * t + k];
        if (nb < 0) continue;
        const int u = m->tri[3 * t + (k + 1) % 3], v = m->tri[3 * t + (k + 2) % 3];
        int ok = 0;
        if (nb == (int)t) { simplex_mesh_free(m); GSL_ERROR_NULL("simplex_mesh_import: a triangle is its own neighbour", GSL_EINVAL); }
        for (int q = 0; q < 3 && !ok; q++)
          if (m->nbr[3 * nb + q] == (int)t) {
            const int a = m->tri[3 * nb + (q + 1) % 3], b = m->tri[3 * nb + (q + 2) % 3];
            ok = (a == u && b == v) || (a == v && b == u);
          }
        if (!ok) { simplex_mesh_free(m); GSL_ERROR_NULL("simplex_mesh_import: neighbour links are not mutual", GSL_EINVAL); }
      }
  } else {
    const int st = derive_neighbours(m);
    if (st != GSL_SUCCESS) { simplex_mesh_free(m); GSL_ERROR_NULL("simplex_mesh_import: cannot derive neighbour links", st); }
  }
  m->convex = mesh_detect_convex(m);                    /* simplex_mesh_set_convex overrides */
  return m;
}

/* ------------------------------------------------------------------------ */
/* Tetrahedral meshes (dim = 3).  Same conventions one dimension up: link k = the neighbour across the FACE opposite
   vertex k, -1 on the hull. */

/* what the locate kernels index with: ids in range, no repeated vertex, no self-neighbour, every link answered by the
   neighbour across the same face (the dim shared vertex ids match as a set).  0 = fine, otherwise which rule failed. */
enum { MESH_OK = 0, MESH_BAD_VERTEX, MESH_BAD_LINK, MESH_REPEATED, MESH_SELF, MESH_NOT_MUTUAL };
static int mesh_check_arrays(const simplex_mesh *m)
{
  const size_t w = m->dim + 1, nt = m->n_tri, np = m->n_points;
  for (size_t i = 0; i < w * nt; i++) {
    if (m->tri[i] < 0 || (size_t)m->tri[i] >= np) return MESH_BAD_VERTEX;
    if (m->nbr[i] < -1 || m->nbr[i] >= (int)nt) return MESH_BAD_LINK;
  }
  for (size_t t = 0; t < nt; t++) {
    const int *v = m->tri + w * t;
    for (size_t a = 0; a < w; a++)
      for (size_t b = a + 1; b < w; b++)
        if (v[a] == v[b]) return MESH_REPEATED;
  }
  for (size_t t = 0; t < nt; t++) {
    const int *v = m->tri + w * t;
    for (size_t k = 0; k < w; k++) {
      const int nb = m->nbr[w * t + k];
      if (nb < 0) continue;
      if (nb == (int)t) return MESH_SELF;
      const int *u = m->tri + w * (size_t)nb;
      int found = 0;
      for (size_t q = 0; q < w && !found; q++) {
        if (m->nbr[w * (size_t)nb + q] != (int)t) continue;
        /* no repeated ids on either side: the face of t is a subset of the face of nb <=> the two are equal */
        int same = 1;
        for (size_t a = 0; a < w && same; a++) {
          if (a == k) continue;
          int in = 0;
          for (size_t b = 0; b < w; b++) if (b != q && u[b] == v[a]) in = 1;
          same = in;
        }
        found = same;
      }
      if (!found) return MESH_NOT_MUTUAL;
    }
  }
  return MESH_OK;
}

/* neighbour links by face matching: every face (a < b < c) with the tetrahedron and the slot opposite to it, sorted */
typedef struct { int a, b, c, t, slot; } mesh_face;
static int face_cmp(const void *x, const void *y)
{
  const mesh_face *p = (const mesh_face *)x, *q = (const mesh_face *)y;
  if (p->a != q->a) return p->a < q->a ? -1 : 1;
  if (p->b != q->b) return p->b < q->b ? -1 : 1;
  if (p->c != q->c) return p->c < q->c ? -1 : 1;
  return p->t < q->t ? -1 : (p->t > q->t);
}

static void sort3(int *a, int *b, int *c)
{
  int t;
  if (*b < *a) { t = *a; *a = *b; *b = t; }
  if (*c < *b) { t = *b; *b = *c; *c = t; }
  if (*b < *a) { t = *a; *a = *b; *b = t; }
}

static int derive_neighbours3(simplex_mesh *m)
{
  const size_t nf = 4 * m->n_tri;
  mesh_face *f = (mesh_face *)malloc(nf * sizeof *f);
  if (!f) return GSL_ENOMEM;
  for (size_t t = 0; t < m->n_tri; t++)
    for (int k = 0; k < 4; k++) {
      mesh_face *x = &f[4 * t + k];
      x->a = m->tri[4 * t + (k + 1) % 4]; x->b = m->tri[4 * t + (k + 2) % 4]; x->c = m->tri[4 * t + (k + 3) % 4];
      sort3(&x->a, &x->b, &x->c);
      x->t = (int)t; x->slot = k;
    }
  qsort(f, nf, sizeof *f, face_cmp);
  for (size_t i = 0; i < nf; i++) m->nbr[i] = -1;
  int status = GSL_SUCCESS;
  for (size_t i = 0; i < nf;) {
    size_t j = i + 1;
    while (j < nf && f[j].a == f[i].a && f[j].b == f[i].b && f[j].c == f[i].c) j++;
    if (j - i == 2) {
      m->nbr[4 * f[i].t + f[i].slot] = f[i + 1].t;
      m->nbr[4 * f[i + 1].t + f[i + 1].slot] = f[i].t;
    } else if (j - i > 2) status = GSL_EINVAL;          /* a face shared by three tetrahedra: not a tetrahedralisation */
    i = j;
  }
  free(f);
  return status;
}

/* Convexity of a tetrahedral mesh, decided from its boundary faces (link -1): convex = the boundary is ONE closed
   2-manifold (every boundary edge in exactly two boundary faces, all faces connected through edges) and across every
   boundary edge the far vertex of the adjacent face lies on or behind this face's plane (relative tolerance 1e-12, as
   in 2-D; coplanar hull faces allowed).  The outward side of a face is the one its tetrahedron's fourth vertex is not
   on; a flat boundary tetrahedron cannot orient its face and answers 0, like every other doubt. */
typedef struct { int a, b, face, far; } mesh_bedge;        /* boundary edge a < b of boundary face `face`, far = its third vertex */
static int bedge_cmp(const void *x, const void *y)
{
  const mesh_bedge *p = (const mesh_bedge *)x, *q = (const mesh_bedge *)y;
  if (p->a != q->a) return p->a < q->a ? -1 : 1;
  if (p->b != q->b) return p->b < q->b ? -1 : 1;
  return p->face < q->face ? -1 : (p->face > q->face);
}

static int uf_find(int *parent, int i)
{
  while (parent[i] != i) { parent[i] = parent[parent[i]]; i = parent[i]; }
  return i;
}

static int mesh_detect_convex3(const simplex_mesh *m)
{
  const size_t nt = m->n_tri;
  size_t nb = 0;
  for (size_t i = 0; i < 4 * nt; i++) nb += m->nbr[i] < 0;
  if (nb < 4 || nb > (size_t)INT_MAX / 3) return 0;
  mesh_bedge *e = (mesh_bedge *)malloc(3 * nb * sizeof *e);
  double *plane = (double *)malloc(4 * nb * sizeof(double));    /* outward normal and one point's id per boundary face */
  int *parent = (int *)malloc(nb * sizeof(int));
  int ok = e && plane && parent;
  size_t fi = 0;
  for (size_t t = 0; t < nt && ok; t++)
    for (int k = 0; k < 4 && ok; k++) {
      if (m->nbr[4 * t + k] >= 0) continue;
      const int *v = m->tri + 4 * t;
      const int id[3] = {v[(k + 1) % 4], v[(k + 2) % 4], v[(k + 3) % 4]};
      const double *p0 = m->points + 3 * (size_t)id[0], *p1 = m->points + 3 * (size_t)id[1], *p2 = m->points + 3 * (size_t)id[2];
      const double *pi = m->points + 3 * (size_t)v[k];
      const double u[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]}, w[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
      double n[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
      const double r[3] = {pi[0] - p0[0], pi[1] - p0[1], pi[2] - p0[2]};
      const double side = n[0] * r[0] + n[1] * r[1] + n[2] * r[2];
      const double tol = 1e-12 * sqrt((n[0] * n[0] + n[1] * n[1] + n[2] * n[2]) * (r[0] * r[0] + r[1] * r[1] + r[2] * r[2]));
      if (!(fabs(side) > tol)) { ok = 0; break; }                 /* flat tetrahedron (or NaN): the face has no outward side */
      const double sg = side > 0 ? -1.0 : 1.0;                    /* the fourth vertex is inside: the normal points away from it */
      plane[4 * fi] = sg * n[0]; plane[4 * fi + 1] = sg * n[1]; plane[4 * fi + 2] = sg * n[2]; plane[4 * fi + 3] = (double)id[0];
      for (int j = 0; j < 3; j++) {
        const int a = id[j], b = id[(j + 1) % 3];
        mesh_bedge *x = &e[3 * fi + j];
        x->a = a < b ? a : b; x->b = a < b ? b : a; x->face = (int)fi; x->far = id[(j + 2) % 3];
      }
      parent[fi] = (int)fi;
      fi++;
    }
  if (ok) {
    qsort(e, 3 * nb, sizeof *e, bedge_cmp);
    for (size_t i = 0; i < 3 * nb && ok; i += 2) {
      /* exactly two boundary faces per boundary edge */
      if (i + 1 >= 3 * nb || e[i].a != e[i + 1].a || e[i].b != e[i + 1].b) { ok = 0; break; }
      if (i + 2 < 3 * nb && e[i + 2].a == e[i].a && e[i + 2].b == e[i].b) { ok = 0; break; }
      for (int s = 0; s < 2 && ok; s++) {                         /* the far vertex of each face against the other's plane */
        const mesh_bedge *me = &e[i + s], *other = &e[i + 1 - s];
        const double *n = plane + 4 * (size_t)me->face;
        const double *p0 = m->points + 3 * (size_t)n[3], *q = m->points + 3 * (size_t)other->far;
        const double r[3] = {q[0] - p0[0], q[1] - p0[1], q[2] - p0[2]};
        const double h = n[0] * r[0] + n[1] * r[1] + n[2] * r[2];
        const double tol = 1e-12 * sqrt((n[0] * n[0] + n[1] * n[1] + n[2] * n[2]) * (r[0] * r[0] + r[1] * r[1] + r[2] * r[2]));
        if (!(h <= tol)) ok = 0;                                  /* in front of the plane: a reflex edge */
      }
      const int ra = uf_find(parent, e[i].face), rb = uf_find(parent, e[i + 1].face);
      if (ra != rb) parent[ra] = rb;
    }
    const int root = ok ? uf_find(parent, 0) : 0;
    for (size_t i = 1; i < nb && ok; i++)
      if (uf_find(parent, (int)i) != root) ok = 0;                /* a cavity or a second component */
  }
  free(e); free(plane); free(parent);
  return ok;
}

static simplex_mesh *mesh_import3(const gsl_matrix *points, const int *simplices, const int *neighbours, size_t n)
{
  if (points->size2 < 3 || points->size1 < 4 || n < 1 || n > (size_t)INT_MAX / 4 || points->size1 > (size_t)INT_MAX)
    GSL_ERROR_NULL("simplex_mesh_import_nd: need >= 4 points with 3 coordinates and >= 1 tetrahedron", GSL_EINVAL);
  const size_t np = points->size1;
  simplex_mesh *m = mesh_alloc(n, np, 0, 3);
  if (!m) GSL_ERROR_NULL("simplex_mesh_import_nd: out of memory", GSL_ENOMEM);
  memcpy(m->tri, simplices, 4 * n * sizeof(int));
  if (neighbours) memcpy(m->nbr, neighbours, 4 * n * sizeof(int));
  else for (size_t i = 0; i < 4 * n; i++) m->nbr[i] = -1;
  switch (mesh_check_arrays(m)) {
    case MESH_OK: break;
    case MESH_BAD_VERTEX: simplex_mesh_free(m); GSL_ERROR_NULL("simplex_mesh_import_nd: vertex id out of range", GSL_EINVAL);
    case MESH_BAD_LINK: simplex_mesh_free(m); GSL_ERROR_NULL("simplex_mesh_import_nd: neighbour id out of range", GSL_EINVAL);
    case MESH_REPEATED: simplex_mesh_free(m); GSL_ERROR_NULL("simplex_mesh_import_nd: tetrahedron with a repeated vertex", GSL_EINVAL);
    case MESH_SELF: simplex_mesh_free(m); GSL_ERROR_NULL("simplex_mesh_import_nd: a tetrahedron is its own neighbour", GSL_EINVAL);
    default: simplex_mesh_free(m); GSL_ERROR_NULL("simplex_mesh_import_nd: neighbour links are not mutual across the same face", GSL_EINVAL);
  }
  for (size_t r = 0; r < np; r++)
    for (int j = 0; j < 3; j++) m->points[3 * r + j] = points->data[r * points->tda + j];
  mesh_bbox(m);
  for (int j = 0; j < 3; j++) {                         /* as in 2-D: centre of the bounding box, 1 / extent */
    m->shift[j] = (m->lo[j] + m->hi[j]) / 2.0;
    m->scale[j] = (m->hi[j] - m->lo[j] <= 0) ? 1.0 : 1.0 / (m->hi[j] - m->lo[j]);
  }
  if (!neighbours) {
    const int st = derive_neighbours3(m);
    if (st != GSL_SUCCESS) { simplex_mesh_free(m); GSL_ERROR_NULL("simplex_mesh_import_nd: cannot derive neighbour links", st); }
  }
  m->convex = mesh_detect_convex3(m);                   /* simplex_mesh_set_convex overrides */
  return m;
}

simplex_mesh *simplex_mesh_import_nd(const gsl_matrix *points, size_t dim, const int *simplices, const int *neighbours, size_t n_simplices)
{
  if (!points || !simplices) GSL_ERROR_NULL("simplex_mesh_import_nd: null argument", GSL_EFAULT);
  if (dim == 2) return simplex_mesh_import(points, simplices, neighbours, n_simplices);
  if (dim != 3) GSL_ERROR_NULL("simplex_mesh_import_nd: triangles (dim 2) and tetrahedra (dim 3) only", GSL_EUNIMPL);
  return mesh_import3(points, simplices, neighbours, n_simplices);
}

simplex_mesh *simplex_mesh_from_tree(simplex_tree *tree, gsl_matrix *data)
{
  if (!tree || !data) GSL_ERROR_NULL("simplex_mesh_from_tree: null argument", GSL_EFAULT);
  if (tree->dim != 2) GSL_ERROR_NULL("simplex_mesh_from_tree: 2-D trees only", GSL_EUNIMPL);
  const int n = tree->n_simplexes, np = tree->n_points;
  int *index = (int *)malloc((size_t)n * sizeof(int));          /* DAG node -> triangle, -1 = not exported */
  if (!index) GSL_ERROR_NULL("simplex_mesh_from_tree: out of memory", GSL_ENOMEM);
  size_t nt = 0;
  for (int k = 0; k < n; k++) {
    index[k] = -1;
    if (!LEAF(k)) continue;
    if (POINT(k, 0) < 0 || POINT(k, 1) < 0 || POINT(k, 2) < 0) continue;      /* touches the cage: outside the hull */
    index[k] = (int)nt++;
  }
  if (nt == 0 || np < 3) { free(index); GSL_ERROR_NULL("simplex_mesh_from_tree: the tree has no triangle of data points", GSL_EINVAL); }
  simplex_mesh *m = mesh_alloc(nt, (size_t)np > data->size1 ? (size_t)np : data->size1, 1, 2);
  if (!m) { free(index); GSL_ERROR_NULL("simplex_mesh_from_tree: out of memory", GSL_ENOMEM); }
  for (size_t r = 0; r < m->n_points; r++) {
    m->points[2 * r] = r < data->size1 ? data->data[r * data->tda] : 0.0;
    m->points[2 * r + 1] = r < data->size1 ? data->data[r * data->tda + 1] : 0.0;
  }
  for (int k = 0; k < n; k++) {
    const int t = index[k];
    if (t < 0) continue;
    m->node[t] = k;
    for (int i = 0; i < 3; i++) {
      m->tri[3 * t + i] = (int)gsl_permutation_get(tree->shuffle, (size_t)POINT(k, i));   /* insertion index -> data row */
      const simplex_index nb = LINK(k, i);
      m->nbr[3 * t + i] = nb > 0 ? index[nb] : -1;              /* a leaf's link 0 = none; cage neighbours -> hull */
    }
  }
  free(index);
  mesh_bbox(m);
  for (int j = 0; j < 2; j++) { m->shift[j] = gsl_vector_get(tree->shift, j); m->scale[j] = gsl_vector_get(tree->scale, j); }
  return m;
}

/* ------------------------------------------------------------------------ */
/* Which metric makes a 2-D mesh Delaunay (natural-neighbour interpolation needs one: csrc/hip/natural.hip walks the
   triangles whose circumcircle contains the target).  Locally Delaunay in coordinates x_j * s_j: across every interior
   edge the neighbour's opposite vertex d is not strictly inside the circumcircle of the triangle (a, b, c), in
   determinant form, relative to d and for the counter-clockwise order:
       det = cross(a, b) |c|^2 + cross(b, c) |a|^2 + cross(c, a) |b|^2  <=  1e-9 * (the same sum over absolute values).
   Flat triangles (|orientation| <= 1e-14 * the sum of the squared edge lengths: the rule of natural_pack_kernel) are
   skipped on either side; cocircular neighbours give det = 0 to rounding, so lattices pass. */
static int tri_flat(const double p[3][2], double *orient)
{
  const double bx = p[1][0] - p[0][0], by = p[1][1] - p[0][1], cx = p[2][0] - p[0][0], cy = p[2][1] - p[0][1];
  const double ex = p[2][0] - p[1][0], ey = p[2][1] - p[1][1];
  *orient = bx * cy - by * cx;
  return !(fabs(*orient) > 1e-14 * ((bx * bx + by * by) + (cx * cx + cy * cy) + (ex * ex + ey * ey)));
}

static int mesh_locally_delaunay(const simplex_mesh *m, double s0, double s1)
{
  for (size_t t = 0; t < m->n_tri; t++) {
    double p[3][2], q[3][2], orient, qo;
    for (int i = 0; i < 3; i++) { p[i][0] = m->points[2 * (size_t)m->tri[3 * t + i]] * s0; p[i][1] = m->points[2 * (size_t)m->tri[3 * t + i] + 1] * s1; }
    if (tri_flat(p, &orient)) continue;
    for (int k = 0; k < 3; k++) {
      const int nb = m->nbr[3 * t + k];
      if (nb < 0 || (size_t)nb < t) continue;               /* every interior edge once; the test is symmetric */
      int slot = -1;
      for (int j = 0; j < 3; j++) {
        if (m->nbr[3 * (size_t)nb + j] == (int)t) slot = j;
        q[j][0] = m->points[2 * (size_t)m->tri[3 * (size_t)nb + j]] * s0; q[j][1] = m->points[2 * (size_t)m->tri[3 * (size_t)nb + j] + 1] * s1;
      }
      if (slot < 0 || tri_flat(q, &qo)) continue;
      const double sg = orient > 0 ? 1.0 : -1.0;
      const double ax = p[0][0] - q[slot][0], ay = p[0][1] - q[slot][1], bx = p[1][0] - q[slot][0], by = p[1][1] - q[slot][1];
      const double cx = p[2][0] - q[slot][0], cy = p[2][1] - q[slot][1];
      const double a2 = ax * ax + ay * ay, b2 = bx * bx + by * by, c2 = cx * cx + cy * cy;
      const double det = sg * ((ax * by - ay * bx) * c2 + (bx * cy - by * cx) * a2 + (cx * ay - cy * ax) * b2);
      const double mag = (fabs(ax * by) + fabs(ay * bx)) * c2 + (fabs(bx * cy) + fabs(by * cx)) * a2 + (fabs(cx * ay) + fabs(cy * ax)) * b2;
      if (det > 1e-9 * mag) return 0;
    }
  }
  return 1;
}

int simplex_mesh_delaunay_metric(const simplex_mesh *mesh)
{
  if (!mesh || mesh->dim != 2) return 0;
  if (mesh_locally_delaunay(mesh, 1.0, 1.0)) return 1;
  if (mesh->scale[0] > 0 && mesh->scale[1] > 0 && mesh_locally_delaunay(mesh, mesh->scale[0], mesh->scale[1])) return 2;
  return 0;
}

/* ------------------------------------------------------------------------ */
/* Vertex -> neighbour CSR of a 2-D mesh (the rows of the gradient system of csrc/hip/cubic.hip): every undirected edge
   of the triangulation once per endpoint, hull edges included, the neighbours of a vertex ascending.  Every triangle
   corner files its two edge partners under the vertex (a counting sort by vertex: O(n)); an interior edge is then
   filed twice per endpoint, so every row (6 entries on average) is sorted by insertion and made unique. */
int simplex_mesh_vertex_adjacency(const simplex_mesh *mesh, int *offsets, int *neighbours, size_t capacity, size_t *n_entries)
{
  if (!mesh || !offsets || !n_entries) GSL_ERROR("simplex_mesh_vertex_adjacency: null argument", GSL_EFAULT);
  if (mesh->dim != 2) GSL_ERROR("simplex_mesh_vertex_adjacency: 2-D meshes only", GSL_EUNSUP);
  const size_t np = mesh->n_points, nt = mesh->n_tri;
  if (6 * nt > (size_t)INT_MAX) GSL_ERROR("simplex_mesh_vertex_adjacency: mesh too large", GSL_EINVAL);
  int *raw = (int *)malloc((6 * nt + 1) * sizeof(int)), *start = (int *)calloc(np + 1, sizeof(int));
  if (!raw || !start) { free(raw); free(start); GSL_ERROR("simplex_mesh_vertex_adjacency: out of memory", GSL_ENOMEM); }
  for (size_t k = 0; k < 3 * nt; k++) start[mesh->tri[k] + 1] += 2;
  for (size_t i = 0; i < np; i++) start[i + 1] += start[i];
  for (size_t i = 0; i <= np; i++) offsets[i] = start[i];              /* offsets: the fill cursors for now */
  for (size_t t = 0; t < nt; t++)
    for (int a = 0; a < 3; a++) {
      const int v = mesh->tri[3 * t + a];
      raw[offsets[v]++] = mesh->tri[3 * t + (a + 1) % 3];
      raw[offsets[v]++] = mesh->tri[3 * t + (a + 2) % 3];
    }
  size_t total = 0;
  for (size_t i = 0; i < np; i++) {
    int *row = raw + start[i];
    const int len = start[i + 1] - start[i];
    for (int a = 1; a < len; a++) {
      const int key = row[a];
      int b = a - 1;
      for (; b >= 0 && row[b] > key; b--) row[b + 1] = row[b];
      row[b + 1] = key;
    }
    offsets[i] = (int)total;
    for (int a = 0; a < len; a++) {
      if (row[a] == (int)i || (a > 0 && row[a] == row[a - 1])) continue;
      if (neighbours && total < capacity) neighbours[total] = row[a];
      total++;
    }
  }
  offsets[np] = (int)total;
  *n_entries = total;
  free(raw); free(start);
  if (neighbours && total > capacity) GSL_ERROR("simplex_mesh_vertex_adjacency: neighbour array too short (6 n_triangles always suffices)", GSL_EBADLEN);
  return GSL_SUCCESS;
}

/* ------------------------------------------------------------------------ */
/* Binary checkpoint of a mesh (gsl_matrix_fwrite conventions: native byte order, GSL_EFAILED on a short transfer):
     2-D: magic "GSLSMSH1" | n_tri, n_points, has_nodes, convex (int64) | triangles | neighbours | [tree nodes] | points |
          shift, scale, lo, hi;
     3-D: magic "GSLSMSH2" | n_simplices, n_points, has_nodes (0), convex, dim (int64) | simplices | neighbours | points |
          shift, scale, lo, hi (dim doubles each).
   fread re-checks everything the import checks (ids in range, no repeated vertex, mutual links across the same edge /
   face): the locate kernels index with these arrays. */
static const char MESH_MAGIC[8] = {'G', 'S', 'L', 'S', 'M', 'S', 'H', '1'};
static const char MESH_MAGIC_ND[8] = {'G', 'S', 'L', 'S', 'M', 'S', 'H', '2'};

int simplex_mesh_fwrite(FILE *stream, const simplex_mesh *m)
{
  if (!stream || !m) GSL_ERROR("simplex_mesh_fwrite: null argument", GSL_EFAULT);
  const size_t d = m->dim, w = d + 1;
  const int64_t head[5] = {(int64_t)m->n_tri, (int64_t)m->n_points, m->node ? 1 : 0, m->convex, (int64_t)d};
  const size_t nh = d == 2 ? 4 : 5;                            /* a 2-D mesh keeps the GSLSMSH1 layout byte for byte */
  int ok = fwrite(d == 2 ? MESH_MAGIC : MESH_MAGIC_ND, 1, 8, stream) == 8 && fwrite(head, sizeof head[0], nh, stream) == nh;
  ok = ok && fwrite(m->tri, sizeof(int), w * m->n_tri, stream) == w * m->n_tri;
  ok = ok && fwrite(m->nbr, sizeof(int), w * m->n_tri, stream) == w * m->n_tri;
  if (m->node) ok = ok && fwrite(m->node, sizeof(int), m->n_tri, stream) == m->n_tri;
  ok = ok && fwrite(m->points, sizeof(double), d * m->n_points, stream) == d * m->n_points;
  double geo[12];
  for (size_t j = 0; j < d; j++) { geo[j] = m->shift[j]; geo[d + j] = m->scale[j]; geo[2 * d + j] = m->lo[j]; geo[3 * d + j] = m->hi[j]; }
  ok = ok && fwrite(geo, sizeof(double), 4 * d, stream) == 4 * d;
  if (!ok) GSL_ERROR("simplex_mesh_fwrite: fwrite failed", GSL_EFAILED);
  return GSL_SUCCESS;
}

simplex_mesh *simplex_mesh_fread(FILE *stream)
{
  if (!stream) GSL_ERROR_NULL("simplex_mesh_fread: null stream", GSL_EFAULT);
  char magic[8];
  int64_t head[5] = {0, 0, 0, 0, 2};
  if (fread(magic, 1, 8, stream) != 8 || (memcmp(magic, MESH_MAGIC, 8) != 0 && memcmp(magic, MESH_MAGIC_ND, 8) != 0))
    GSL_ERROR_NULL("simplex_mesh_fread: not a simplex_mesh checkpoint", GSL_EFAILED);
  const size_t nh = memcmp(magic, MESH_MAGIC, 8) == 0 ? 4 : 5;
  if (fread(head, sizeof head[0], nh, stream) != nh) GSL_ERROR_NULL("simplex_mesh_fread: short header", GSL_EFAILED);
  if (nh == 5 && head[4] != 3) GSL_ERROR_NULL("simplex_mesh_fread: corrupt header", GSL_EFAILED);   /* GSLSMSH2 holds 3-D meshes */
  const size_t d = (size_t)head[4], w = d + 1;
  if (head[0] < 1 || head[0] > INT_MAX / (int64_t)w || head[1] < (int64_t)w || head[1] > INT_MAX || (head[2] != 0 && head[2] != 1) ||
      (d == 3 && head[2] != 0))
    GSL_ERROR_NULL("simplex_mesh_fread: corrupt header", GSL_EFAILED);
  const size_t nt = (size_t)head[0], np = (size_t)head[1];
  {
    /* seekable stream: the counts must fit what is left of the file before anything is allocated for them */
    const long here = ftell(stream);
    if (here >= 0 && fseek(stream, 0L, SEEK_END) == 0) {
      const long end = ftell(stream);
      const long long need = 4LL * (2 * (long long)w + head[2]) * (long long)nt + 8LL * (long long)d * (long long)np + 32LL * (long long)d;
      if (fseek(stream, here, SEEK_SET) != 0) GSL_ERROR_NULL("simplex_mesh_fread: stream error", GSL_EFAILED);
      if (end >= here && (long long)(end - here) < need) GSL_ERROR_NULL("simplex_mesh_fread: short or corrupt checkpoint", GSL_EFAILED);
    }
  }
  simplex_mesh *m = mesh_alloc(nt, np, (int)head[2], d);
  if (!m) GSL_ERROR_NULL("simplex_mesh_fread: out of memory", GSL_ENOMEM);
  double geo[12];
  int ok = fread(m->tri, sizeof(int), w * nt, stream) == w * nt && fread(m->nbr, sizeof(int), w * nt, stream) == w * nt;
  if (m->node) ok = ok && fread(m->node, sizeof(int), nt, stream) == nt;
  ok = ok && fread(m->points, sizeof(double), d * np, stream) == d * np && fread(geo, sizeof(double), 4 * d, stream) == 4 * d;
  ok = ok && mesh_check_arrays(m) == MESH_OK;
  if (!ok) { simplex_mesh_free(m); GSL_ERROR_NULL("simplex_mesh_fread: short or corrupt checkpoint", GSL_EFAILED); }
  for (size_t j = 0; j < d; j++) { m->shift[j] = geo[j]; m->scale[j] = geo[d + j]; m->lo[j] = geo[2 * d + j]; m->hi[j] = geo[3 * d + j]; }
  m->convex = head[3] != 0;
  return m;
}
