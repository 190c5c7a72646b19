/*
 * gsl_sinterp.h -- host-side C API of the MI355X-native scattered-data
 * interpolation library (libgsl_sinterp.so).
 *
 * Part 1 keeps the reference's existing scattered-interpolation symbols
 * (interpolation/linear_simplex.h:105-179, interpolation/edge_flip.h:42-47)
 * with their signatures, flags, `simplex_tree` field order and accessor macros,
 * so a program written against the reference recompiles against this header.
 * They run on the host, exactly like the reference: the Delaunay history DAG is
 * built once on the CPU (2-D).
 *
 * Part 2 is the batched, GPU-only entry the reference lacks
 * (simplex_tree_device_*): the DAG is mirrored into HBM and M targets are
 * located + interpolated by one kernel.
 *
 * Part 3 is the gsl_sinterp facade shaped like gsl_interp
 * (interpolation/gsl_interp.h:49-71, interpolation/interp.c:30-138):
 * alloc(type, dim, n) / init / eval_e / eval / eval_many / free with three
 * types: Gaussian RBF, thin-plate-spline RBF, linear simplex (barycentric).
 *
 * There is no CPU fallback for parts 2 and 3: without a usable gfx950 device
 * they fail with GSL_EFAILED through the GSL error handler.
 */
#ifndef GSL_SINTERP_H
#define GSL_SINTERP_H

#include "gsl_sinterp_compat.h"
#include "gsl_sinterp_hip.h"
#include <assert.h>
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ======================================================================== */
/* Part 1: reference simplex_tree API (host)                                 */
/* ======================================================================== */
typedef int simplex_index;

typedef enum { leaf_type = 0, sub_dplus1_type, sub_d_type, sub_2_type } node_type;

typedef struct simplex_tree_node_struct {
  int points;          /* offset of this node's vertex ids in pidx[]  */
  simplex_index links; /* offset of this node's links in links[]      */
  node_type type : 2;
} simplex_tree_node;

typedef struct {
  gsl_matrix *simplex_matrix;
  gsl_permutation *perm;
  gsl_vector *coords;
  simplex_index current_simplex;
} simplex_tree_accel;

typedef struct simplex_tree_struct {
  int n_simplexes, max_simplexes;
  simplex_tree_node *simplexes;
  int n_pidx, max_pidx;
  int *pidx;
  int n_links, max_links;
  simplex_index *links;
  gsl_matrix *seed_points;
  int n_points;
  int max_points;
  int dim;
  gsl_vector *shift;
  gsl_vector *scale;
  gsl_vector *min;
  gsl_vector *max;
  gsl_permutation *shuffle;
  simplex_tree_accel *accel;
  simplex_index *new_simplexes;
  simplex_index *old_neighbors1;
  simplex_index *old_neighbors2;
  int *left_out;
  int *tmp_points1;
  gsl_vector *tmp_vec1, *tmp_vec2;
  gsl_matrix *tmp_mat;
} simplex_tree;

/* accessor macros with the reference's names; they expect a variable `tree` */
#define SIMP(I) (&(tree->simplexes[(I)]))
#define LINK(NODE, I) (tree->links[(I) + SIMP(NODE)->links])
#define SLINK(NODE, I) (SIMP(LINK(NODE, I)))
#define POINT(NODE, I) (tree->pidx[(I) + SIMP(NODE)->points])
#define LEAF(NODE) (leaf_type == SIMP(NODE)->type)

/* N_CHILDREN / DATA_POINT / FIND of the reference header (linear_simplex.h:67-102): number of
   children by node type, the vertex behind a vertex id (cage seed row when negative, data row
   shuffle[id] otherwise), and the "first index satisfying a predicate" loop. */
#define N_CHILDREN(NODE) _n_children(tree, NODE)
#define DATA_POINT(DATA, POINT) _data_point(tree, (DATA), (POINT))
#define FIND(VAR, PRED, ...)                                                   \
  for (VAR = 0; VAR < tree->dim + 1; VAR++) {                                  \
    if (PRED) break;                                                           \
  }                                                                            \
  assert(("Couldn't satisfy predicate: ", PRED, "" __VA_ARGS__ "", VAR < tree->dim + 1));

static inline int _n_children(simplex_tree *tree, simplex_index node)
{
  const node_type t = SIMP(node)->type;
  return t == sub_dplus1_type ? tree->dim + 1 : t == sub_d_type ? tree->dim : t == sub_2_type ? 2 : 0;
}

static inline gsl_vector_view _data_point(simplex_tree *tree, gsl_matrix *data, int point)
{
  return point < 0 ? gsl_matrix_row(tree->seed_points, (size_t)(-point - 1))
                   : gsl_matrix_row(data, gsl_permutation_get(tree->shuffle, (size_t)point));
}

#define SIMPLEX_TREE_DEFAULT 0
#define SIMPLEX_TREE_NOSTANDARDIZE (1 << 0)
#define SIMPLEX_TREE_ISOSCALE (1 << 1)

simplex_index simplex_tree_node_alloc(simplex_tree *tree);
simplex_tree *simplex_tree_alloc(int dim, int n_points);
int simplex_tree_init(simplex_tree *tree, gsl_matrix *data, gsl_vector *min, gsl_vector *max,
                      int init_flags, gsl_rng *rng);
void simplex_tree_free(simplex_tree *tree);
simplex_tree_accel *simplex_tree_accel_alloc(int dim);
void simplex_tree_accel_free(simplex_tree_accel *accel);
int point_in_simplex(simplex_tree *tree, simplex_index node, int point);
simplex_index find_leaf(simplex_tree *tree, gsl_matrix *data, gsl_vector *point,
                        simplex_tree_accel *accel);
simplex_index _find_leaf(simplex_tree *tree, simplex_index node, gsl_matrix *data,
                         gsl_vector *point, simplex_tree_accel *accel);
int insert_point(simplex_tree *tree, simplex_index leaf, gsl_matrix *data, gsl_vector *point,
                 simplex_tree_accel *accel);
int in_hypersphere(simplex_tree *tree, simplex_index node, gsl_matrix *data, int idx,
                   simplex_tree_accel *accel);
int in_hypersphere_points(simplex_tree *tree, int *points, gsl_matrix *data, int idx,
                          simplex_tree_accel *accel);
int calculate_hypersphere(simplex_tree *tree, simplex_index node, gsl_matrix *data,
                          gsl_vector *x0, double *r2, simplex_tree_accel *accel);
int calculate_hypersphere_points(simplex_tree *tree, int *points, gsl_matrix *data,
                                 gsl_vector *x0, double *r2, simplex_tree_accel *accel);
int calculate_bary_coords(simplex_tree *tree, simplex_index node, gsl_matrix *data,
                          gsl_vector *point, simplex_tree_accel *accel);
int contains_point(simplex_tree *tree, simplex_index node, gsl_matrix *data, gsl_vector *point,
                   simplex_tree_accel *accel);
double interp_point(simplex_tree *tree, simplex_index leaf, gsl_matrix *data,
                    gsl_vector *response, gsl_vector *point, simplex_tree_accel *accel);
int delaunay(simplex_tree *tree, simplex_index leaf, gsl_matrix *data, int face,
             simplex_tree_accel *accel);

/* ======================================================================== */
/* Part 2: batched GPU evaluation over a built tree                          */
/* ======================================================================== */
typedef struct simplex_tree_device simplex_tree_device;

/* Mirror `tree` (built over `data`) into the HBM of `device` (ordinal). */
simplex_tree_device *simplex_tree_device_alloc(simplex_tree *tree, gsl_matrix *data, int device);
void simplex_tree_device_free(simplex_tree_device *dev);
/* Bind the response column used by the following eval calls. */
int simplex_tree_device_set_response(simplex_tree_device *dev, const gsl_vector *response);
/* find_leaf + interp_point for every row of `targets` (M x 2, tda honoured).
   `leaf` may be NULL.  Rows outside the cage give leaf -1 / value NaN and the
   call returns GSL_EDOM (no abort). */
int simplex_tree_device_eval_many(simplex_tree_device *dev, const gsl_matrix *targets,
                                  gsl_vector *values, simplex_index *leaf);
/* Same, with targets / outputs already resident in HBM. */
int simplex_tree_device_eval_resident(simplex_tree_device *dev, const double *d_targets, size_t m,
                                      size_t ttda, double *d_values, simplex_index *d_leaf);
gsl_sinterp_hip_ctx *simplex_tree_device_ctx(simplex_tree_device *dev);
/* Several responses on the same tree, with per-leaf gradients, from ONE locate ("Several responses on a
   mesh"; csrc/hip/linear_fields.hip).  set_responses binds F, n_points x K (1 <= K <= 64, F->tda honoured, rows = rows of
   the data matrix); it and set_response are independent bindings, neither disturbs the other.  eval_fields_many:
   targets M x 2, S M x K, G (or NULL) M x 2 K with entry (k, 2 q + a) = d(field q)/dy_a, leaf (or NULL); tda of every
   matrix honoured.  Column q of S holds the bits eval_many returns with column q of F bound; the gradient is that of the
   affine function of the located leaf (cage vertices carry 0, as in the value), equal bits for every target of a leaf,
   and the value bits do not depend on G.  A row outside the cage gives NaN in S and G, leaf -1 and GSL_EDOM after every
   other row has been stored.  eval_fields_resident: row k of d_S at d_S + k * stda (stda >= K), of d_G at d_G + k * gtda
   (gtda >= 2 K), padding untouched; asynchronous, nothing is read back (no GSL_EDOM: the NaN rows and d_leaf tell).
   The unchanged locate of eval_many runs once, then the fields sweep.  On a multi-device mirror the first device
   evaluates every target (no sharding of field batches).  GSL_EINVAL: K = 0, K > 64, no responses bound, stda or gtda
   too small; GSL_EBADLEN: shapes; GSL_EFAULT: NULL. */
int simplex_tree_device_set_responses(simplex_tree_device *dev, const gsl_matrix *F);
size_t simplex_tree_device_n_responses(const simplex_tree_device *dev);     /* K of the last set_responses, 0 = none */
int simplex_tree_device_eval_fields_many(simplex_tree_device *dev, const gsl_matrix *targets, gsl_matrix *S, gsl_matrix *G,
                                         simplex_index *leaf);
int simplex_tree_device_eval_fields_resident(simplex_tree_device *dev, const double *d_targets, size_t m, size_t ttda, double *d_S,
                                             size_t stda, double *d_G, size_t gtda, simplex_index *d_leaf);
/* Mirror on several GPUs: the raw DAG arrays are replicated with one broadcast per array, every member
   packs its own records; eval_many shards the targets (eval_resident uses the first device). */
simplex_tree_device *simplex_tree_device_alloc_multi(simplex_tree *tree, gsl_matrix *data, const int *devices,
                                                     int n_devices);
int simplex_tree_device_n_devices(const simplex_tree_device *dev);
const char *simplex_tree_device_transport(const simplex_tree_device *dev);   /* "rccl" | "peer-copy" | "none" */

/* The reference's traversal / dump entries (interpolation/linear_simplex_integrity_check.h:11-21), same signatures:
   check_leaf_nodes walks the leaf adjacency depth first from the first leaf and applies fn to every leaf (the
   reference's order); check_delaunay returns 1 when the device-side checks pass; output_triangulation writes
   the gnuplot files of :246-284 (any name may be NULL). */
void check_leaf_nodes(simplex_tree *tree, void (*fn)(simplex_tree *, simplex_index));
int check_delaunay(simplex_tree *tree, gsl_matrix *data);
void output_triangulation(simplex_tree *tree, gsl_matrix *data, gsl_vector *response, int standardize_output,
                          char lines_filename[], char points_filename[], char circles_filename[]);
/* binary checkpoint of a built tree (native byte order; GSL_EFAILED on a short or corrupt stream) */
int simplex_tree_fwrite(FILE *stream, const simplex_tree *tree);
simplex_tree *simplex_tree_fread(FILE *stream);

/* check_leaf_nodes + check_delaunay of the reference (interpolation/linear_simplex_integrity_check.c:121-168;
   there an O(N^3) debug pass after every insertion) as two GPU kernels over the finished tree: O(leaves) and
   O(leaves x N).  Returns 1 when every predicate holds -- check_delaunay's own return convention (:162-168) --
   0 when a violation was found (counts in *leaf_violations / *delaunay_violations, either may be NULL), and a
   negative value (-GSL status, raised through the handler) when the check could not run. */
int simplex_tree_check_device(simplex_tree *tree, gsl_matrix *data, int device, long long *leaf_violations,
                              long long *delaunay_violations);

/* ======================================================================== */
/* Part 2b: imported triangulations (no history DAG)                          */
/* ======================================================================== */
/* The reference's README:28-31 lists "import triangulations from QHull / CGAL" as future work.  Such a triangulation
   comes as arrays: `triangles` [3 n] vertex ids = rows of `points`, `neighbours` [3 n] = triangle across the edge
   OPPOSITE vertex k of the triangle, -1 on the hull (the convention of QHull's neighbours and of the leaves'
   links in interpolation/linear_simplex.h:62-63).  neighbours == NULL: derived from the triangles (edge matching).
   Evaluation is the barycentric interpolation of interp_point (linear_simplex.c:678-711) in a triangle that contains
   the target under the closed rule of contains_point (:653-676), found on the GPU by a grid seed + a walk over the
   neighbour links.  A target outside the triangulation gives index -1, value NaN and GSL_EDOM. */
typedef struct simplex_mesh simplex_mesh;
typedef struct simplex_mesh_device simplex_mesh_device;
simplex_mesh *simplex_mesh_import(const gsl_matrix *points, const int *triangles, const int *neighbours, size_t n_triangles);
/* The same import in dim = 2 or 3.  dim = 2 is simplex_mesh_import (same mesh, same checkpoint bytes).  dim = 3: a
   tetrahedralisation in the same array form, `simplices` [4 n], `neighbours` [4 n] = the tetrahedron across the FACE opposite
   vertex k, -1 on the hull, or NULL (derived by face matching; a face shared by three tetrahedra is GSL_EINVAL).  Checked
   like the 2-D import: ids in range, no repeated vertex, no tetrahedron its own neighbour, links mutual across the same
   face.  Evaluated by csrc/hip/mesh3.hip (grid seed + walk over the face links; flat tetrahedra, which QHull returns for
   cospherical input, never contain a target).  Any other dim: GSL_EUNIMPL; points->size2 < dim or fewer than dim + 1
   points: GSL_EINVAL.  simplex_mesh_from_tree stays 2-D, and simplex_mesh_tree_nodes is NULL for a 3-D mesh. */
simplex_mesh *simplex_mesh_import_nd(const gsl_matrix *points, size_t dim, const int *simplices, const int *neighbours, size_t n_simplices);
/* the final triangulation of a built tree: its leaves without cage vertices, vertex order, neighbour links and
   standardisation kept, so that evaluation returns the bits of the DAG path wherever the containing leaf is unique */
simplex_mesh *simplex_mesh_from_tree(simplex_tree *tree, gsl_matrix *data);
void simplex_mesh_free(simplex_mesh *mesh);
size_t simplex_mesh_dim(const simplex_mesh *mesh);             /* 2 or 3 */
size_t simplex_mesh_n_triangles(const simplex_mesh *mesh);     /* number of simplices: triangles (dim 2), tetrahedra (dim 3) */
size_t simplex_mesh_n_points(const simplex_mesh *mesh);
const int *simplex_mesh_triangles(const simplex_mesh *mesh);   /* [(dim + 1) n] */
const int *simplex_mesh_neighbours(const simplex_mesh *mesh);  /* [(dim + 1) n] */
const int *simplex_mesh_tree_nodes(const simplex_mesh *mesh);  /* [n] DAG node of every triangle (from_tree), else NULL */
/* shift = centre of the points' bounding box, scale = 1 / extent per axis (1 for a zero extent); dim entries are written
   to each array: 2 for a 2-D mesh, as before, 3 for a 3-D one */
void simplex_mesh_geometry(const simplex_mesh *mesh, double *shift, double *scale);
/* convex = 1: a boundary edge in the walking direction proves the target outside (index -1, NaN, GSL_EDOM); 0: such walks
   are resolved by an exhaustive scan (meshes with holes / concave outlines).  simplex_mesh_import decides it from the
   boundary (one closed loop without a reflex turn = convex), simplex_mesh_from_tree exports convex = 1 (the hull of a
   Delaunay triangulation); simplex_mesh_set_convex overrides, simplex_mesh_convex reads the current setting.
   3-D: decided from the boundary faces -- every boundary edge in exactly two of them, one connected surface, and across
   every boundary edge the far vertex of the adjacent face on or behind this face's plane (relative tolerance 1e-12);
   any doubt (a cavity, a dent, a flat boundary tetrahedron whose face cannot be oriented) answers 0. */
void simplex_mesh_set_convex(simplex_mesh *mesh, int convex);
int simplex_mesh_convex(const simplex_mesh *mesh);
const double *simplex_mesh_points(const simplex_mesh *mesh);    /* [dim n_points], packed rows */
/* The metric in which a 2-D mesh is locally Delaunay (across every interior edge the neighbour's opposite vertex is not
   inside the circumcircle by more than 1e-9 relative, in determinant form; flat triangles are skipped): 1 = in the
   coordinates as given (QHull / CGAL output), 2 = in the mesh's standardised coordinates (simplex_mesh_geometry: a mesh
   exported from a simplex_tree, whose build standardises per axis), 0 = in neither, and for a 3-D mesh.  O(n). */
int simplex_mesh_delaunay_metric(const simplex_mesh *mesh);
/* Vertex -> neighbour CSR of a 2-D mesh: every undirected edge of the triangulation once per endpoint (hull edges
   included), the neighbours of a vertex ascending.  offsets [n_points + 1] is always filled and *n_entries receives
   offsets[n_points]; neighbours (may be NULL: count only) receives the entries when capacity >= *n_entries, otherwise
   GSL_EBADLEN (6 n_triangles always suffices).  Host, O(n).  GSL_EUNSUP for a 3-D mesh. */
int simplex_mesh_vertex_adjacency(const simplex_mesh *mesh, int *offsets, int *neighbours, size_t capacity, size_t *n_entries);
void simplex_mesh_bbox(const simplex_mesh *mesh, double *lo, double *hi);   /* dim entries each */
/* binary checkpoint of a mesh (gsl_matrix_fwrite conventions); fread re-validates ids and neighbour links.  A 2-D mesh
   writes the GSLSMSH1 layout; a 3-D mesh writes GSLSMSH2, whose header carries dim; fread accepts both */
int simplex_mesh_fwrite(FILE *stream, const simplex_mesh *mesh);
simplex_mesh *simplex_mesh_fread(FILE *stream);
simplex_mesh_device *simplex_mesh_device_alloc(const simplex_mesh *mesh, int device);
/* the mirror replicated over a device group (one broadcast of the raw arrays, every member packs its own records and
   seed grid); eval_many shards its targets like simplex_tree_device_alloc_multi's mirror */
simplex_mesh_device *simplex_mesh_device_alloc_multi(const simplex_mesh *mesh, const int *devices, int n_devices);
int simplex_mesh_device_n_devices(const simplex_mesh_device *dev);
void simplex_mesh_device_free(simplex_mesh_device *dev);
int simplex_mesh_device_set_response(simplex_mesh_device *dev, const gsl_vector *response);
/* targets: M x dim of the mesh (GSL_EBADLEN otherwise); eval_resident: ttda >= dim */
int simplex_mesh_device_eval_many(simplex_mesh_device *dev, const gsl_matrix *targets, gsl_vector *values, int *triangle);
int simplex_mesh_device_eval_resident(simplex_mesh_device *dev, const double *d_targets, size_t m, size_t ttda,
                                      double *d_values, int *d_triangle);
/* Several responses on the same mirror, with per-simplex gradients, from ONE locate: simplex_tree_device_set_responses /
   _eval_fields_many / _eval_fields_resident above, for a mesh of dim 2 or 3 (rows of F = rows of the points; targets
   M x dim; G M x (K dim), entry (k, q dim + a); gtda >= K dim).  Independent of set_response; the first device of a
   group evaluates every target. */
int simplex_mesh_device_set_responses(simplex_mesh_device *dev, const gsl_matrix *F);
size_t simplex_mesh_device_n_responses(const simplex_mesh_device *dev);
int simplex_mesh_device_eval_fields_many(simplex_mesh_device *dev, const gsl_matrix *targets, gsl_matrix *S, gsl_matrix *G, int *triangle);
int simplex_mesh_device_eval_fields_resident(simplex_mesh_device *dev, const double *d_targets, size_t m, size_t ttda, double *d_S,
                                             size_t stda, double *d_G, size_t gtda, int *d_triangle);
/* Natural-neighbour (Sibson) interpolation on the same mirror: C1 away from the sites, exact at them, reproduces linear
   functions, local, no shape parameter and no solve ("Natural neighbours").  Same shapes and status
   conventions as the two entries above; `triangle` receives the triangle that contains the target.  A target within
   rounding of the hull takes the piecewise-linear value, the interpolant's limit there.  Nothing is computed or kept for
   these entries until the first call: it asks the mesh for its metric (O(n) on the host), uploads its links and points
   once more and packs the natural-neighbour records, so `mesh` must still be alive then (later calls do not need it).  GSL_EINVAL: simplex_mesh_delaunay_metric is 0 (the mesh is not Delaunay);
   GSL_EUNSUP: a 3-D mesh, a mesh with convex = 0, a device group of more than one member. */
int simplex_mesh_device_eval_natural_many(simplex_mesh_device *dev, const gsl_matrix *targets, gsl_vector *values, int *triangle);
int simplex_mesh_device_eval_natural_resident(simplex_mesh_device *dev, const double *d_targets, size_t m, size_t ttda,
                                              double *d_values, int *d_triangle);
/* Clough-Tocher C1 piecewise-cubic interpolation on the same mirror, with gradients ("Clough-Tocher";
   csrc/hip/cubic.hip): interpolates the data and the vertex gradients, C1 everywhere, reproduces quadratics when the
   gradients are exact.  Needs no Delaunay property and no convexity: any 2-D mesh qualifies.
     bind_gradients   gradients [n_points x 2] to interpolate, or NULL = estimate them (the global estimator of scipy's
                      CloughTocher2DInterpolator, solved on the device by preconditioned conjugate gradients to the
                      options below; defaults rtol = 1e-12, maxiter = 1000).  Drops what an earlier binding computed.
                      simplex_mesh_device_set_response drops the gradients and the records as well.
     gradients        the gradients in use [n_points x 2] (estimates them now if that is still to do), the iterations
                      the estimate took (0 for bound gradients) and its relative residual; any output may be NULL.
                      GSL_EMAXITER: maxiter was reached before rtol; count and residual are still returned.
     eval_cubic_*     shapes and statuses of the linear entries; gradient (may be NULL) receives grad s in raw
                      coordinates, M x 2 (resident: row k at d_gradient + k * gtda, gtda >= 2); the value bits do not
                      depend on it.  A target outside gives NaN in the value and the gradient, triangle -1, GSL_EDOM.
   Nothing is computed, uploaded or kept for these entries until the first call of gradients / eval_cubic_*: it reads
   the mesh (adjacency, links, points), so `mesh` must still be alive then.  GSL_EUNSUP: a 3-D mesh, a device group
   of more than one member. */
int simplex_mesh_device_bind_gradients(simplex_mesh_device *dev, const gsl_matrix *gradients);
int simplex_mesh_device_set_gradient_options(simplex_mesh_device *dev, double rtol, size_t maxiter);
int simplex_mesh_device_gradients(simplex_mesh_device *dev, gsl_matrix *gradients, size_t *iterations, double *residual);
int simplex_mesh_device_eval_cubic_many(simplex_mesh_device *dev, const gsl_matrix *targets, gsl_vector *values, gsl_matrix *gradient,
                                        int *triangle);
int simplex_mesh_device_eval_cubic_resident(simplex_mesh_device *dev, const double *d_targets, size_t m, size_t ttda, double *d_values,
                                            double *d_gradient, size_t gtda, int *d_triangle);
gsl_sinterp_hip_ctx *simplex_mesh_device_ctx(simplex_mesh_device *dev);

/* ======================================================================== */
/* Part 3: gsl_sinterp facade                                                */
/* ======================================================================== */
typedef struct gsl_sinterp_struct gsl_sinterp;
#define GSL_SINTERP_MAX_DEVICES 64

typedef struct {
  const char *name;
  unsigned int min_size;
  void *(*alloc)(size_t dim, size_t size);
  int (*init)(gsl_sinterp *interp, const gsl_matrix *x, const gsl_vector *f);
  int (*eval_many)(const gsl_sinterp *interp, const gsl_matrix *y, gsl_vector *s, int *leaf);
  int (*eval_resident)(const gsl_sinterp *interp, const double *d_y, size_t m, size_t ytda,
                       double *d_s, int *d_leaf);
  void (*free)(void *state);
} gsl_sinterp_type;

struct gsl_sinterp_struct {
  const gsl_sinterp_type *type;
  size_t dim;
  size_t size;
  int device;        /* GPU ordinal; default 0 or $GSL_SINTERP_DEVICE */
  double shape;      /* shape parameter eps; <= 0 -> the type's default: Gaussian 2 * size^(1/dim), Wendland size^(1/dim) / 8,
                        Matern 3/2, 5/2 and inverse multiquadric size^(1/dim) (length scale 1/eps = the mean spacing) */
  int init_flags;    /* SIMPLEX_TREE_* flags (linear simplex type)            */
  gsl_rng *rng;      /* insertion-order rng (linear simplex type), may be NULL */
  void *state;
  int n_devices;     /* > 1: the model is replicated over devices[] and eval_many shards its targets */
  int devices[GSL_SINTERP_MAX_DEVICES];
  int solver;        /* GSL_SINTERP_SOLVER_* (RBF types); default = by kernel class          */
  int want_rcond;    /* estimate the reciprocal condition number at init (Cholesky solvers)  */
  double rcond;      /* the estimate of the last init, NaN when none was made                */
  int route;         /* solver route the last init took (gsl_sinterp_hip_rbf_solve_ex)       */
  double nugget;     /* kriging: added to the diagonal of the covariance matrix (>= 0, default 0) */
  int want_variance; /* kriging: the next init keeps the Cholesky factor for gsl_sinterp_eval_variance_* (default 0) */
  int want_loo;      /* positive definite RBF types (Gaussian / Wendland / Matern / inverse multiquadric) and kriging: the next init computes the leave-one-out residuals and variances (default 0) */
  size_t neighbours; /* kriging: > 0 = local kriging on that many nearest centres per target (gsl_sinterp_set_neighbours); 0 = the global model (default) */
  int drift;         /* kriging: order of the polynomial drift of the next init, 0 = ordinary kriging (default), 1 linear, 2 quadratic (gsl_sinterp_set_drift) */
};

extern const gsl_sinterp_type *gsl_sinterp_rbf_gaussian;
extern const gsl_sinterp_type *gsl_sinterp_rbf_tps;
/* the thin-plate spline with its affine tail: s(y) = sum_j w_j phi(|y - x_j|) + c_0 + sum_a c_a y_a with P^T w = 0
   (the (N + d + 1) saddle system; reproduces linear data exactly).  gsl_sinterp_poly reads c back. */
extern const gsl_sinterp_type *gsl_sinterp_rbf_tps_affine;
extern const gsl_sinterp_type *gsl_sinterp_rbf_wendland;    /* compactly supported C2 kernel (README:18-26 future list) */
extern const gsl_sinterp_type *gsl_sinterp_linear_simplex;
/* piecewise-linear interpolation over an IMPORTED triangulation (QHull / CGAL arrays, README:28-31 future list): set the
   triangles with gsl_sinterp_set_triangulation before gsl_sinterp_init(x, f); `leaf` of eval_many = triangle index */
extern const gsl_sinterp_type *gsl_sinterp_linear_mesh;
/* natural-neighbour (Sibson) interpolation, dim 2 only: C1 except at the data sites, exact at them, reproduces linear
   functions, local, no shape parameter and no solve.
     gsl_sinterp_natural_mesh     over an imported DELAUNAY triangulation, set up like gsl_sinterp_linear_mesh
                                  (gsl_sinterp_set_triangulation, then init); init gives GSL_EINVAL when
                                  simplex_mesh_delaunay_metric of the mesh is 0, GSL_EUNSUP when it is not convex;
     gsl_sinterp_natural_simplex  builds the Delaunay tree on the host exactly as gsl_sinterp_linear_simplex does
                                  (gsl_sinterp_set_tree_options is honoured), exports it with simplex_mesh_from_tree and
                                  evaluates on that mesh: no external triangulator is needed.
   eval_e / eval_many / eval_resident / eval_grid; `leaf` = the triangle of the mesh that contains the target; a target
   outside the hull gives NaN, -1 and GSL_EDOM.  One device only (a device list of more than one member: GSL_EUNSUP at
   init).  Gradients, fields, variance, leave-one-out, fit and set_neighbours: GSL_EUNSUP.  Checkpoints: type ids 12 /
   13 with the mesh payload of gsl_sinterp_linear_mesh. */
extern const gsl_sinterp_type *gsl_sinterp_natural_mesh, *gsl_sinterp_natural_simplex;
/* Clough-Tocher C1 piecewise-cubic interpolation, dim 2 only (scipy's CloughTocher2DInterpolator, griddata's "cubic"):
   interpolates the data and a gradient at every site, C1 everywhere -- the mesh method whose gradient is continuous.
     gsl_sinterp_cubic_mesh     over an imported triangulation, set up like gsl_sinterp_linear_mesh
                                (gsl_sinterp_set_triangulation, then init); no Delaunay property, no convexity needed;
     gsl_sinterp_cubic_simplex  builds the tree on the host as gsl_sinterp_natural_simplex does and evaluates on the
                                exported mesh.
   The gradients at the sites are estimated at init (gsl_sinterp_set_gradient_options; GSL_EMAXITER from init when the
   solve did not reach rtol) unless gsl_sinterp_set_gradients gave them; gsl_sinterp_get_gradients reads them back.
   eval_e / eval_many / eval_resident / eval_grid and gsl_sinterp_eval_grad_e / _many / _resident; `leaf` = the triangle
   that contains the target; a target outside the triangulation gives NaN (value and gradient), -1 and GSL_EDOM.  One
   device only (GSL_EUNSUP at init otherwise).  Fields, variance, leave-one-out, fit and set_neighbours: GSL_EUNSUP.
   Checkpoints: type ids 14 / 15, the mesh payload of gsl_sinterp_linear_mesh followed by the 2 N gradients; a restored
   interpolant does not estimate again. */
extern const gsl_sinterp_type *gsl_sinterp_cubic_mesh, *gsl_sinterp_cubic_simplex;
/* Modified quadratic Shepard interpolation ("modified-quadratic-shepard"; Renka's QSHEP2D / QSHEP3D, ACM TOMS 660 / 661),
   dim 2 or 3 (any other dim: GSL_EUNIMPL at alloc): the smooth interpolant for clouds past the size a dense solve holds and
   for 3-D clouds without a mesh.  C1 everywhere, exact at the data, reproduces quadratics, local, O(N) memory, no solve, no
   triangulation, no shape parameter, analytic gradient.  The method and its reproducibility contract:
   gsl_sinterp_hip_shepard_fit / _eval (gsl_sinterp_hip.h).
     gsl_sinterp_set_shepard(interp, nq, nw), before init: the number of neighbours behind the radius of the nodal fits and
       of the evaluation weights; 0 = the default, Renka's 13 / 19 in 2-D and 17 / 32 in 3-D.  GSL_EINVAL: another type, nq
       below the number of monomials (5 / 9) or above 62, nw above 62.  gsl_sinterp_init: GSL_EINVAL when size <
       max(nq, nw) + 2; GSL_EDOM when two sites coincide (the interpolant stays uninitialised).  Init searches the
       neighbours and fits every node on the device; nothing is solved globally.
     eval_e / eval_many / eval_resident / eval_grid (dim 2) and gsl_sinterp_eval_grad_e / _many / _resident; `leaf` = the number
       of nodes whose weight is positive at the target (1 at a site).  A target no node's radius covers gives NaN (value and
       gradient), -1 and GSL_EDOM after every other target has been stored; a NaN coordinate gives NaN and is no error.
     gsl_sinterp_get_gradients: the N x dim nodal gradients, iterations 0, residual 0.
     gsl_sinterp_shepard_stats: how many nodes fell back to a linear and to a constant nodal function (rank-deficient
       neighbourhoods: collinear or coplanar sites) and the largest radius of influence; each output may be NULL.
     gsl_sinterp_shepard_ctx: the device context of the interpolant (NULL before the first init), for the counters
       gsl_sinterp_hip_shepard_fit_count / _pack_count.
   One device only (a device list of more than one member: GSL_EUNSUP at init).  Fields, variance, leave-one-out, fit,
   set_neighbours: GSL_EUNSUP; set_solver, get_weights, mean, poly: GSL_EINVAL.  Checkpoints: type id 16 -- nq, nw, the
   fallback counts, centres, responses, radii and coefficients; a restored interpolant does not search or fit again and
   evaluates to the same bits. */
extern const gsl_sinterp_type *gsl_sinterp_shepard;
int gsl_sinterp_set_shepard(gsl_sinterp *interp, size_t nq, size_t nw);
int gsl_sinterp_shepard_stats(const gsl_sinterp *interp, size_t *n_linear, size_t *n_constant, double *rw_max);
gsl_sinterp_hip_ctx *gsl_sinterp_shepard_ctx(const gsl_sinterp *interp);
/* ordinary kriging with a Gaussian covariance exp(-(eps h)^2) and an optional nugget (README:24 future list):
   s(y) = mu + sum_j w_j C(|y - x_j|) with [C + nugget I, 1; 1^T, 0] [w; mu] = [f; 0].  nugget = 0 interpolates the data,
   nugget > 0 smooths (s(x_i) = f_i - nugget w_i); far from the data s -> mu.  gsl_sinterp_set_shape sets eps. */
extern const gsl_sinterp_type *gsl_sinterp_kriging;
/* Matern 3/2, Matern 5/2 and the inverse multiquadric (the standard menu next to the Gaussian):
       rbf-matern-3/2             phi(r) = (1 + t) exp(-t),          t = sqrt(3) eps r
       rbf-matern-5/2             phi(r) = (1 + t + t^2/3) exp(-t),  t = sqrt(5) eps r
       rbf-inverse-multiquadric   phi(r) = 1 / sqrt(1 + (eps r)^2)
   Positive definite in every dimension with phi(0) = 1: the Cholesky route (1), and every entry that accepts
   gsl_sinterp_rbf_gaussian accepts them -- eval, gradients, init_fields / eval_fields, set_loo, get_weights, device
   lists, checkpoints.  Length scale 1/eps; default eps = size^(1/dim).  Far better conditioned than the Gaussian at
   the same length scale.  Every centre contributes to every target: these sweeps are not culled.  A target with a NaN
   coordinate evaluates to NaN; the result for an infinite coordinate is not specified. */
extern const gsl_sinterp_type *gsl_sinterp_rbf_matern32, *gsl_sinterp_rbf_matern52, *gsl_sinterp_rbf_imq;
/* ordinary kriging with a Matern 3/2 / 5/2 covariance (sill 1, length scale 1/eps): "ordinary-kriging-matern-3/2" and
   "ordinary-kriging-matern-5/2"; everything gsl_sinterp_kriging offers -- set_nugget, mean, set_variance and the
   eval_variance entries, set_loo, fields -- on the covariances that are usually fitted.  Routes 7 / 8 as there. */
extern const gsl_sinterp_type *gsl_sinterp_kriging_matern32, *gsl_sinterp_kriging_matern52;

gsl_sinterp *gsl_sinterp_alloc(const gsl_sinterp_type *T, size_t dim, size_t size);
int gsl_sinterp_set_device(gsl_sinterp *interp, int device);
/* Multi-GPU: solve on the first device, ONE broadcast of the model (RCCL over xGMI),
   targets of gsl_sinterp_eval_many sharded contiguously over the devices, each shard copied back by its
   own GPU.  set_devices(n) = ordinals 0..n-1; the environment variable GSL_SINTERP_DEVICES ("4" or
   "0,2,5") sets the default at alloc time (GSL_SINTERP_DEVICE the single-device default). */
int gsl_sinterp_set_devices(gsl_sinterp *interp, int n_devices);
int gsl_sinterp_set_device_list(gsl_sinterp *interp, const int *devices, int n_devices);
int gsl_sinterp_n_devices(const gsl_sinterp *interp);
int gsl_sinterp_set_shape(gsl_sinterp *interp, double eps);
/* Solver breadth (linalg/cholesky.c:392-537, linalg/pcholesky.c, linalg/lu.c:204): GSL_SINTERP_SOLVER_DEFAULT picks
   by kernel class (Gaussian, Wendland, Matern, inverse multiquadric: Cholesky; thin-plate spline: shifted-SPD Cholesky, LU as fall-back); _CHOLESKY2 the
   diagonally scaled Cholesky; _PCHOLESKY the pivoted LDL^T for semi-definite / nuggeted kernel matrices;
   _LU_REFINE pivoted LU plus one refinement step.  gsl_sinterp_set_rcond(interp, 1) makes the next init estimate
   the reciprocal condition number of the kernel matrix (Cholesky solvers; gsl_linalg_cholesky_rcond), read back
   with gsl_sinterp_rcond (GSL_EINVAL when none is available). */
int gsl_sinterp_set_nugget(gsl_sinterp *interp, double nugget);     /* the three kriging types only (GSL_EINVAL otherwise) */
int gsl_sinterp_mean(const gsl_sinterp *interp, double *mean);     /* the estimated mean mu of an initialised kriging interpolant */
/* Kriging variance sigma^2(y) = C(0) - k^T K^-1 k + (1 - 1^T K^-1 k)^2 / (1^T K^-1 1) of the underlying field (the
   nugget is measurement noise): 0 at the data sites when nugget = 0, 1 + 1/(1^T K^-1 1) far from every site.
   gsl_sinterp_set_variance(interp, 1) BEFORE gsl_sinterp_init makes the init keep the Cholesky factor of K on the
   (first) device -- N^2 doubles for as long as the model lives, which is why it is opt-in; M targets then cost
   M N^2 flops.  Negative rounding residue is clamped to 0 (sqrt is safe).  GSL_EINVAL: not a kriging interpolant, not
   initialised, initialised without set_variance, or restored by gsl_sinterp_fread (a checkpoint carries no factor);
   GSL_EUNSUP: the init took the pivoted LDL^T route 8 (covariance matrix only semi-definite).  With a device list the
   factor lives on the first device, which evaluates every target. */
int gsl_sinterp_set_variance(gsl_sinterp *interp, int want);            /* the three kriging types only (GSL_EINVAL otherwise); before init */
/* Universal kriging: kriging with a polynomial drift (kt3d of GSLIB, UniversalKriging of PyKrige) on the three kriging types,
       s(y) = p(u(y))^T c + sum_j w_j C(|y - x_j|),     [K P; P^T 0] [w; c] = [f; 0],     K = C + nugget I.
   Ordinary kriging returns to one constant far from the data and its variance saturates at 1 + 1/(1^T K^-1 1): data with a
   trend is extrapolated badly and its error mis-stated.  With a drift the predictor reproduces every polynomial of the
   drift's order exactly -- also far outside the cloud -- and the variance grows with the distance as the trend's own
   uncertainty does.
   gsl_sinterp_set_drift(interp, order) BEFORE gsl_sinterp_init: 0 = ordinary kriging, the default, every bit as without the
   call; 1 = linear; 2 = quadratic.  The basis is taken in standardised coordinates u_a = (y_a - shift_a) scale_a, shift the
   centre of the sites' bounding box and scale 1 / half-extent per axis (1 for a zero extent), so that coordinates of UTM
   size cost no digits.  Term order: 1; u_1 .. u_d; u_a u_b for a <= b, lexicographic.  gsl_sinterp_drift_terms(dim, order) =
   q = C(dim + order, order), at most 10 (0 for arguments out of range).  gsl_sinterp_drift is the order in force: the one
   set, or the one a checkpoint brought.
   INIT (gsl_sinterp_route = 12): one fill and one Cholesky factorisation carry the fields and the q drift functions;
   the q x q system for c is solved on the host.  GSL_EDOM, the interpolant left uninitialised, when K is not positive
   definite -- there is NO pivoted route-8 fall-back with a drift: duplicate sites need a nugget -- or when the drift
   functions are linearly dependent on the sites (collinear sites for order 1, sites on a conic for order 2).  GSL_EINVAL
   when size < q.
   With a drift and neighbours == 0 these work as for ordinary kriging: eval_e / _many / _resident / _grid, eval_grad_*,
   init_fields / eval_fields_*, get_weights / get_field_weights (w only), set_variance with eval_variance_*
       sigma^2(y) = C(0) - k^T K^-1 k + r^T S^-1 r,   r = p(u(y)) - B^T k(y),   B = K^-1 P,   S = P^T B,
   clamped at 0, not bounded by the sill; set_loo with loo_* (Dubrule's rule with a drift: diag_i = (K^-1)_ii - B_i S^-1
   B_i^T); device lists (the coefficients travel by value to every member).  The value bits of a target are the same alone,
   in any batch, with or without the gradient, and as a column of a fields call.
   gsl_sinterp_drift_coefficients: c (q entries, in the term order above, for STANDARDISED coordinates) of field `field`;
   shift and scale (dim entries each, or NULL) tell the standardisation.  GSL_EINVAL: not a kriging interpolant, not
   initialised, initialised without a drift, no such field; GSL_EBADLEN: sizes.
   gsl_sinterp_mean / _field_mean: GSL_EUNSUP with a drift (there is no single mean).
   LOCAL route (gsl_sinterp_set_neighbours(k), k > 0) with order 1: every target solves universal kriging with a linear drift
   on its k nearest centres, in the local basis u = (x_i - y) / h, h the distance of the k-th neighbour
   (gsl_sinterp_hip_local_ukrige); eval_*, eval_variance_* and eval_local_many work, everything else is refused exactly as
   for the ordinary local route, and drift_coefficients is GSL_EUNSUP (every neighbourhood has its own).  A target whose
   neighbourhood does not determine the drift (collinear sites in 2-D, coplanar in 3-D), has a covariance matrix that is not
   positive definite, or has h = 0 gets NaN in value and variance and the call returns GSL_EDOM after every other target has
   been stored.  k < dim + 2: GSL_EINVAL at init; order 2 with k > 0: GSL_EUNSUP at init.
   Checkpoints: an interpolant with a drift is written under type id 17 / 18 / 19 (gsl_sinterp_kriging / _matern32 /
   _matern52); payload [centres | weights], a uint64 order, shift, scale, the q coefficients.  gsl_sinterp_fread into a
   kriging interpolant accepts its plain id and its drift id and sets the drift from the file; several fields: GSL_EUNSUP,
   as without a drift.  Ordinary checkpoints keep their bytes.
   The fit workspace (gsl_sinterp_fit_*) scores the ORDINARY model whatever the drift says: a drift-aware likelihood
   (REML) is not provided.  Not provided either: external-drift covariates, simple kriging, order > 2. */
int gsl_sinterp_set_drift(gsl_sinterp *interp, int order);   /* the three kriging types only (GSL_EINVAL otherwise; order outside 0..2: GSL_EINVAL); before init */
int gsl_sinterp_drift(const gsl_sinterp *interp);
size_t gsl_sinterp_drift_terms(size_t dim, int order);
int gsl_sinterp_drift_coefficients(const gsl_sinterp *interp, size_t field, gsl_vector *c /* q */, gsl_vector *shift /* dim or NULL */,
                                   gsl_vector *scale /* dim or NULL */);
int gsl_sinterp_eval_variance_e(const gsl_sinterp *interp, const gsl_vector *y, double *var);
int gsl_sinterp_eval_variance_many(const gsl_sinterp *interp, const gsl_matrix *y, gsl_vector *var);
int gsl_sinterp_eval_variance_resident(const gsl_sinterp *interp, const double *d_y, size_t m, size_t ytda, double *d_var);
/* Joint posterior covariance and conditional simulation (return_cov / sample_y of scikit-learn, LU simulation of GSLIB) for
   the three kriging types, ordinary or with a drift of order 1 or 2, from what gsl_sinterp_set_variance keeps.  For target
   sets Ya (ma rows) and Yb (mb rows; NULL = Ya), sill 1, the nugget measurement noise as in eval_variance_*:
       Cov[i][j] = Cov[Z(ya_i), Z(yb_j) | data] = C(|ya_i - yb_j|) - k(ya_i)^T K^-1 k(yb_j) + r(ya_i)^T S^-1 r(yb_j),
   r = p(u(y)) - B^T k(y), B = K^-1 P, S = P^T B (ordinary kriging: p = 1, B = K^-1 1).  C carries no nugget, also for
   coincident targets (C = 1).  The diagonal of the one-set form is the kriging variance of eval_variance_* BEFORE their
   clamp: NOTHING is clamped here, so where sigma^2 = 0 (a data site of a nugget-free model) the diagonal carries rounding
   residue of either sign; the variance entries stay the clamped ones.  With yb == NULL only the lower triangle is computed
   and then mirrored: Cov is symmetric to the bit.  Cost: (ma + mb) N^2 flops for the substitution the variance does too,
   plus ma mb N for the product.
   gsl_sinterp_simulate_*: conditional realisations at the m rows of y from standard normals Zn (m x S) that the CALLER
   supplies -- the library draws no random numbers, every result is reproducible:
       Out[:, s] = s(Y) + sqrt(sigma2) A Zn[:, s],     A A^T = Cov(Y, Y) + jitter I,
   A the lower Cholesky factor taken in target order (value i of a draw depends on the normals 0 .. i only), s(Y) field 0's
   predictor: a column of Zn that is all zeros returns the bits of gsl_sinterp_eval_many, equal columns give equal bits.
   sigma2 scales the unit-sill model to the units of f: pass 1, or what gsl_sinterp_fit_sigma2 returned.  The matrix is
   factored by the library's blocked Cholesky; when it is not numerically positive definite -- targets on data sites of a
   nugget-free model, repeated targets -- every entry of Out is NaN and the call returns GSL_EDOM through the handler: pass a
   jitter such as 1e-10.  There is no pivoted fall-back and no automatic jitter.
   STATE: exactly the conditions of eval_variance_* (GSL_EINVAL: not a kriging interpolant, not initialised, initialised
   without set_variance, restored by fread; GSL_EUNSUP: route 8), and GSL_EUNSUP with neighbours > 0 (the local route has no
   joint model), before anything touches the device.  ARGUMENTS: GSL_EFAULT a NULL argument; GSL_EBADLEN ya / yb / y without
   dim columns, Cov not ma x mb, Zn or Out not m x S with S >= 1; GSL_EINVAL ctda < mb, ztda or otda < S, sigma2 not finite or
   <= 0, jitter not finite or < 0; ma, mb or m = 0 succeeds and writes nothing.  Every tda is honoured and padding left
   untouched; a target with a NaN coordinate gives NaN in its row and column of Cov and is no error.  With a device list the
   first device does the work.  Work memory is the grow-only workspace of the variance entries, which holds ALL of Z at once
   here: when it cannot grow -- m so large that m^2 doubles, or (ma + mb) N doubles, do not fit -- GSL_ENOMEM through the
   handler, the outputs untouched.
   Not provided: random-number generation, draws for more than field 0, the local route, sharding over a device group,
   checkpoints of a factor, a pivoted or eigenvalue factor for a singular covariance, sequential simulation. */
int gsl_sinterp_eval_covariance_many(const gsl_sinterp *interp, const gsl_matrix *ya, const gsl_matrix *yb /* or NULL = ya */,
                                     gsl_matrix *Cov /* ma x mb */);
int gsl_sinterp_eval_covariance_resident(const gsl_sinterp *interp, const double *d_ya, size_t ma, size_t yatda,
                                         const double *d_yb /* or NULL */, size_t mb, size_t ybtda, double *d_cov, size_t ctda /* >= mb */);
int gsl_sinterp_simulate_many(const gsl_sinterp *interp, const gsl_matrix *y /* m x dim */, double sigma2, double jitter,
                              const gsl_matrix *Zn /* m x S */, gsl_matrix *Out /* m x S */);
int gsl_sinterp_simulate_resident(const gsl_sinterp *interp, const double *d_y, size_t m, size_t ytda, double sigma2, double jitter,
                                  const double *d_zn, size_t ztda, size_t n_draws, double *d_out, size_t otda);
/* Local kriging (a moving neighbourhood) for clouds past the size a dense N x N factorisation holds:
   gsl_sinterp_set_neighbours(interp, k), 1 <= k <= GSL_SINTERP_MAX_NEIGHBOURS = 64, BEFORE gsl_sinterp_init makes the init
   upload the centres and the responses and bin them on a grid -- nothing is factored, gsl_sinterp_route is 11 -- and every
   evaluation solve ordinary kriging on the k nearest centres of each target (exact search; ties go to the smaller row of x):
   memory O(N + M k), work O(M k^3).  eval_e / _many / _resident / _grid return the local predictor; eval_variance_e / _many /
   _resident the local variance, clamped at 0, WITHOUT gsl_sinterp_set_variance (no factor is kept);
   gsl_sinterp_eval_local_many returns value, variance and the neighbour rows (idx: m x k ints, nearest first) from one pass,
   each output may be NULL.  The formulas and the bit-reproducibility contract: gsl_sinterp_hip_local_krige.
   A target whose neighbourhood has a covariance matrix that is not positive definite (coincident sites without a nugget)
   gets NaN in value and variance; every other target is stored and the call returns GSL_EDOM (eval_e: by status, as for a
   target outside the cage of the linear types).  A target with a NaN coordinate gets NaN and is no error.
   k = 0 (the default) is the global model: init and every bit as without this call.  Shape, nugget and device are honoured
   as usual; with a device list the first device evaluates every target.  The fit workspace ignores the setting: fit eps and
   the nugget on a subsample, then predict on the full cloud with this route.
   set_neighbours: GSL_EINVAL for another type than the three kriging types, k > 64, k > size.  With k > 0 there is no global
   weight vector, mean or factor: the gradient entries, init_fields, the eval_fields / field entries, get_weights, mean,
   fwrite / fread and the leave-one-out accessors return GSL_EUNSUP without touching the device.  eval_local_many: GSL_EINVAL
   when the interpolant was not initialised with k > 0, GSL_EBADLEN for a size mismatch.
   Not provided: search by radius or by octant, gradients (the predictor jumps where the neighbour set changes), several
   fields, simple kriging, a quadratic drift (gsl_sinterp_set_drift(2) with k > 0: GSL_EUNSUP at init; a linear one is
   provided, see gsl_sinterp_set_drift), sharding over a device group, checkpoints, k > 64. */
#define GSL_SINTERP_MAX_NEIGHBOURS 64
int gsl_sinterp_set_neighbours(gsl_sinterp *interp, size_t k);
int gsl_sinterp_eval_local_many(const gsl_sinterp *interp, const gsl_matrix *y, gsl_vector *s /* or NULL */, gsl_vector *var /* or NULL */,
                                int *idx /* y->size1 x k, or NULL */);
/* Leave-one-out cross-validation (Rippa's rule for the positive definite RBF types, Dubrule's for ordinary kriging): how
   good the fit is, and a score for a shape parameter or nugget, without N refits.
       e_i = f_i - s^(-i)(x_i)     the residual at site i of the model built without site i,
       v_i                         positive definite RBF types: the squared power function phi(0) - k^T K_-i^-1 k at x_i;
                                   kriging: the variance of the prediction error of the OBSERVATION f_i, i.e. what
                                   eval_variance of the model without site i returns at x_i, plus the nugget.
   Both come from the diagonal of the inverse of the Cholesky factor the init computes anyway: diag_i = (K^-1)_ii, for
   kriging (A^-1)_ii = (K^-1)_ii - b_i^2 / (1^T b) with b = K^-1 1;  e_i = w_i / diag_i, v_i = 1 / diag_i.
   gsl_sinterp_set_loo(interp, 1) BEFORE the init makes gsl_sinterp_init / gsl_sinterp_init_fields compute them on the
   (first) device at about the price of a second factorisation (N^3 / 3 flops) and keep N (K + 1) doubles on the host; the
   factor itself is not kept for it.  K fields share the diagonal: E is size x K.  Nothing is clamped: where rounding left
   a diag_i non-positive (a kernel matrix at the edge of positive definiteness) v_i is returned as computed.
   set_loo(0), the default, leaves the init and every evaluation exactly as they are.
   GSL_EINVAL: another type than gsl_sinterp_rbf_gaussian / _wendland / _matern32 / _matern52 / _imq and the three kriging
   types, not initialised, initialised
   without set_loo, or restored by gsl_sinterp_fread (a checkpoint carries no leave-one-out data, and reading one drops
   what was held); GSL_EUNSUP: the init took a route without a Cholesky factor (an explicit gsl_sinterp_set_solver, the
   pivoted LDL^T route 8 of kriging): gsl_sinterp_route is then neither 1 nor 7; GSL_EDOM: kriging on no more sites than
   it has mean / drift functions (size 1; size <= gsl_sinterp_drift_terms with a drift): the model without a site does not
   exist, the init itself succeeds and evaluates; GSL_EBADLEN: E is not size x K
   (K = gsl_sinterp_n_fields; E->tda honoured, padding untouched), v does not have size entries. */
int gsl_sinterp_set_loo(gsl_sinterp *interp, int want);
int gsl_sinterp_loo_residuals(const gsl_sinterp *interp, gsl_matrix *E);
int gsl_sinterp_loo_variance(const gsl_sinterp *interp, gsl_vector *v);
/* Model selection: score a shape parameter eps or a nugget on the data, and fit either by a 1-D search.  GSL's workspace
   idiom: gsl_sinterp_fit_alloc copies the centres and the response to the (first) device and allocates the N x N matrix
   ONCE; every evaluation then runs the fill, one Cholesky factorisation with the response riding it and a device-side
   reduction, and copies 32 bytes back.  The types gsl_sinterp_set_loo accepts (Gaussian, Wendland, Matern 3/2 and 5/2,
   inverse multiquadric, the three kriging types).  The interpolant only names type, dim, size and device: it needs no
   init, is not changed, and may be freed before the workspace.
     GSL_SINTERP_FIT_LOO  (1/N) sum e_i^2, e_i the leave-one-out residuals of gsl_sinterp_set_loo (Rippa; Dubrule for
                          kriging), from the same factor;
     GSL_SINTERP_FIT_ML   the negative log-likelihood of a Gaussian process with covariance s2 K, concentrated over the
                          process variance s2 (and, for kriging, over the constant mean mu): with w = K^-1 f (kriging:
                          K^-1 (f - mu 1), mu the mean the solve returns; 1^T w = 0, so f.w is the quadratic form there too)
                          and s2 = f.w / N,   score = 0.5 [N log(2 pi s2) + log|K| + N].
                          K = Phi + nugget I with the nugget relative to a sill of 1, as everywhere else.  Plain maximum
                          likelihood, NOT restricted likelihood (REML): the estimate of mu costs no degree of freedom.
   COST of one evaluation: one fill + one factorisation (N^3 / 3 flops) for ML; about two factorisations for LOO (the
   diagonal of K^-1 is a second N^3 / 3).  Nothing is allocated or freed on the device after fit_alloc, except that the
   first LOO evaluation allocates the buffers of the diagonal (2048 x N doubles at most).
   A CANDIDATE THAT DOES NOT FACTOR IS NOT AN ERROR: when K is not numerically positive definite (or a pivot, a
   leave-one-out diagonal or f.w comes out non-positive or non-finite) *score = +infinity, the return is GSL_SUCCESS and
   the error handler is not called; a score is never NaN on success.  The handler is called, with *score = NaN, for a
   NULL argument (GSL_EFAULT), an unknown criterion, eps not finite or <= 0, a nugget that is negative or, for a
   non-kriging type, not 0 (GSL_EINVAL), and HIP errors.
   THE SEARCH (fit_shape over eps, fit_nugget over the nugget) works in t = log(parameter) and is fixed, so that results
   are reproducible: n_grid points equally spaced in t from lo to hi, both included -- the profile need not be unimodal,
   hence the grid --; then a golden-section search on the two cells around the FIRST smallest grid value (one cell at an
   end), until the bracket is no wider than tol in t or max_eval evaluations are spent.  The result is the lowest-scoring
   point ever evaluated (never worse than the grid's best) and *score_best the value fit_score returns there; nothing is
   evaluated twice.  Defaults n_grid = 9, tol = 1e-2, max_eval = 40 (gsl_sinterp_fit_set_search; GSL_EINVAL for
   n_grid < 3, tol not > 0, max_eval < n_grid -- checked before the workspace pointer).  GSL_EINVAL: lo <= 0, hi <= lo or
   not finite; fit_nugget on a non-kriging type (and nugget_lo > 0 is needed: compare nugget 0 through fit_score);
   GSL_EDOM, outputs NaN: every candidate scored +infinity.  fit_n_eval / fit_trace: the evaluations of the last search
   in order (param and score need fit_n_eval entries, GSL_EBADLEN otherwise).  fit_sigma2: s2 = f.w / N of the last
   finite score handed back -- fit_score's, or the best of a search (GSL_EINVAL before there is one); with the model's
   sill at 1, s2 times gsl_sinterp_eval_variance_* is the prediction variance in the units of f.
   fit_alloc: GSL_EFAULT (a NULL argument), GSL_EINVAL (another type), GSL_EBADLEN (x not size x dim, f not size long),
   GSL_EFAILED / GSL_ENOMEM (no device, no memory), each through the handler with NULL returned.
   A K-field model is fitted on one response, then gsl_sinterp_set_shape + gsl_sinterp_init_fields.  With a device list
   the first device does all the work.  Not provided: gradients of the criteria, a simultaneous 2-D search (alternate the
   two entries), anisotropic length scales, REML, the thin-plate types (no shape parameter). */
#define GSL_SINTERP_FIT_LOO 0   /* mean squared leave-one-out residual, (1/N) sum e_i^2 (Rippa; Dubrule for kriging)    */
#define GSL_SINTERP_FIT_ML  1   /* negative concentrated log-likelihood, 0.5 [N log(2 pi s2) + log|K| + N], s2 = f.w / N */
typedef struct gsl_sinterp_fit_workspace gsl_sinterp_fit_workspace;
gsl_sinterp_fit_workspace *gsl_sinterp_fit_alloc(const gsl_sinterp *interp, const gsl_matrix *x, const gsl_vector *f);
void   gsl_sinterp_fit_free(gsl_sinterp_fit_workspace *w);
int    gsl_sinterp_fit_score(gsl_sinterp_fit_workspace *w, int criterion, double eps, double nugget, double *score);
int    gsl_sinterp_fit_shape(gsl_sinterp_fit_workspace *w, int criterion, double nugget, double eps_lo, double eps_hi,
                             double *eps_best, double *score_best);
int    gsl_sinterp_fit_nugget(gsl_sinterp_fit_workspace *w, int criterion, double eps, double nugget_lo, double nugget_hi,
                              double *nugget_best, double *score_best);
int    gsl_sinterp_fit_set_search(gsl_sinterp_fit_workspace *w, size_t n_grid, double tol, size_t max_eval);  /* 9, 1e-2, 40 */
size_t gsl_sinterp_fit_n_eval(const gsl_sinterp_fit_workspace *w);           /* evaluations of the last search */
int    gsl_sinterp_fit_trace(const gsl_sinterp_fit_workspace *w, gsl_vector *param, gsl_vector *score);  /* in order of evaluation */
int    gsl_sinterp_fit_sigma2(const gsl_sinterp_fit_workspace *w, double *s2); /* f.w / N of the last successful score */
/* Empirical semivariogram and the covariance model fitted to it: the first step of a kriging study, and the one estimator of
   eps, the nugget and the process variance that never forms a matrix -- memory O(N + bins), work proportional to the pairs
   closer than h_max -- so it runs on the whole cloud that gsl_sinterp_set_neighbours is for, where gsl_sinterp_fit_* needs a
   subsample.  GSL's workspace idiom:
     v = gsl_sinterp_variogram_alloc(dim, n_bins);  gsl_sinterp_variogram_compute(v, x, f, 0.0);
     gsl_sinterp_variogram_fit(v, gsl_sinterp_kriging_matern32, MATHERON, W_COUNT_H2, 0, 0, &eps, &nugget, &sigma2, NULL);
     gsl_sinterp_variogram_apply(v, interp);  gsl_sinterp_set_neighbours(interp, 32);  gsl_sinterp_init(interp, x, f);
   and sigma2 is what gsl_sinterp_simulate_* takes.
   compute / compute_resident: the binned pair sums of gsl_sinterp_hip_variogram (exact integers: the same bits for every row
   order and every run) of the n sites, n_bins equal bins on [0, h_max).  h_max <= 0 selects a third of the diagonal of the
   sites' bounding box (gstat's default); gsl_sinterp_variogram_h_max returns the value in force (NaN without a variogram).
   get: lag_b = sum h / N_b, count_b = N_b and
     GSL_SINTERP_VARIOGRAM_MATHERON  gamma_b = sum (f_i - f_j)^2 / (2 N_b);
     GSL_SINTERP_VARIOGRAM_CRESSIE   gamma_b = (1/2) (sum sqrt|f_i - f_j| / N_b)^4 / (0.457 + 0.494 / N_b)   (Cressie-Hawkins);
   every 128-bit sum is converted to a double with one rounding; an empty bin gives NaN, NaN, 0; any output may be NULL.
   fit_model (host arrays, no device): gamma(h) = c0 + c (1 - phi_kind(eps h)) with phi as gsl_sinterp_hip.h defines
   GSL_SINTERP_RBF_GAUSSIAN, _MATERN32 and _MATERN52 (any other kind: GSL_EINVAL).  Bins with count 0, a non-finite gamma or
   lag (and, under W_COUNT_H2, lag 0) are skipped; fewer than 3 usable bins: GSL_EDOM.  Weights N_b (W_COUNT), N_b / lag_b^2
   (W_COUNT_H2, gstat's default) or 1 (W_NONE).  For a fixed eps the model is linear: weighted least squares over (c0, c) with
   c0 >= 0 and c >= 0 (both free first; if a coefficient comes out negative, the better of the two one-column fits).  Over
   eps THE SEARCH of gsl_sinterp_fit_shape on the weighted sum of squares: t = log eps, n_grid points from eps_lo to eps_hi
   with the ends included, golden section on the two cells around the first smallest grid value until the bracket is no
   wider than tol or max_eval evaluations are spent, the best point ever evaluated wins.  0 selects the defaults 9, 1e-2, 40;
   GSL_EINVAL for n_grid < 3, tol not > 0, max_eval < n_grid, eps_lo <= 0, eps_hi <= eps_lo or not finite -- the numbers are
   judged before the pointers (GSL_EFAULT; wss may be NULL).  *wss: the weighted sum of squares at the answer.  A fitted
   c = 0 (pure nugget) is returned as such.  fit_model_n_eval / fit_model_trace: the evaluations of the last fit_model call
   of the process in order (GSL_EBADLEN unless both vectors have n_eval entries).
   fit: fit_model on get's arrays with the default search, for one of the three kriging types (an RBF type takes no nugget:
   GSL_EINVAL; mesh, tree and Shepard types: GSL_EUNSUP).  eps_lo <= 0 selects the bracket 0.1 / h_max .. 100 / h_max.
   *nugget = c0 / c, the library's relative nugget, *sigma2 = c.  A fitted c = 0 is GSL_EDOM with NaN outputs: the relative
   nugget does not exist.  GSL_EINVAL without a variogram.
   apply: gsl_sinterp_set_shape + gsl_sinterp_set_nugget with the last successful fit; GSL_EINVAL before one and for an
   interpolant of another type than the one fitted.  It calls the setters only, so the interpolant may then take
   gsl_sinterp_set_neighbours, a drift, a device list.
   STATUS: GSL_EFAULT a NULL argument; GSL_EBADLEN x not n x dim, f not n long, xtda < dim, a vector of get that is not n_bins
   long; GSL_EINVAL alloc with dim outside 1 .. 3 or n_bins outside 1 .. 256 (NULL returned), h_max NaN or infinite, an unknown
   estimator or weights, more than 2^31 - 1 sites; all through the handler and decided before anything touches a device.
   GSL_EDOM: a NaN or infinite site or response; the default h_max with fewer than 2 sites or sites that all coincide.
   GSL_EFAILED: no device.  A compute that fails leaves the workspace without a variogram (and every compute drops the
   fit).  The workspace owns a context on its device (set_device; default as gsl_sinterp_alloc), created by the first compute.
   Not provided: directional or anisotropic variograms, several responses, the variogram cloud, nested models, a residual
   variogram for universal kriging (pass the residuals as f), subsampling of the pairs, sharding over a device group. */
#define GSL_SINTERP_VARIOGRAM_MATHERON 0
#define GSL_SINTERP_VARIOGRAM_CRESSIE  1
#define GSL_SINTERP_VARIOGRAM_W_COUNT    0   /* N_b            */
#define GSL_SINTERP_VARIOGRAM_W_COUNT_H2 1   /* N_b / lag_b^2  */
#define GSL_SINTERP_VARIOGRAM_W_NONE     2   /* 1              */
typedef struct gsl_sinterp_variogram gsl_sinterp_variogram;
gsl_sinterp_variogram *gsl_sinterp_variogram_alloc(size_t dim, size_t n_bins);          /* dim 1..3, n_bins 1..256 */
int    gsl_sinterp_variogram_set_device(gsl_sinterp_variogram *v, int device);
int    gsl_sinterp_variogram_compute(gsl_sinterp_variogram *v, const gsl_matrix *x, const gsl_vector *f, double h_max);
int    gsl_sinterp_variogram_compute_resident(gsl_sinterp_variogram *v, const double *d_x, size_t n, size_t xtda, const double *d_f, double h_max);
int    gsl_sinterp_variogram_get(const gsl_sinterp_variogram *v, int estimator, gsl_vector *lag, gsl_vector *gamma, gsl_vector *count);
double gsl_sinterp_variogram_h_max(const gsl_sinterp_variogram *v);
int    gsl_sinterp_variogram_fit(gsl_sinterp_variogram *v, const gsl_sinterp_type *T, int estimator, int weights, double eps_lo, double eps_hi,
                                 double *eps, double *nugget /* c0 / c */, double *sigma2 /* c */, double *wss /* or NULL */);
int    gsl_sinterp_variogram_apply(const gsl_sinterp_variogram *v, gsl_sinterp *interp);
void   gsl_sinterp_variogram_free(gsl_sinterp_variogram *v);
int    gsl_sinterp_variogram_fit_model(int kind, int weights, const double *lag, const double *gamma, const double *count, size_t n_bins,
                                       double eps_lo, double eps_hi, size_t n_grid, double tol, size_t max_eval,
                                       double *eps, double *nugget_abs /* c0 */, double *psill /* c */, double *wss /* or NULL */);
size_t gsl_sinterp_variogram_fit_model_n_eval(void);
int    gsl_sinterp_variogram_fit_model_trace(gsl_vector *eps, gsl_vector *wss);
int gsl_sinterp_poly(const gsl_sinterp *interp, gsl_vector *c);    /* c_0 .. c_dim of an initialised gsl_sinterp_rbf_tps_affine interpolant */
int gsl_sinterp_set_solver(gsl_sinterp *interp, int solver);
int gsl_sinterp_set_rcond(gsl_sinterp *interp, int want);
int gsl_sinterp_rcond(const gsl_sinterp *interp, double *rcond);
int gsl_sinterp_route(const gsl_sinterp *interp);
int gsl_sinterp_set_tree_options(gsl_sinterp *interp, int init_flags, gsl_rng *rng);
/* gsl_sinterp_linear_mesh (dim 2 or 3), gsl_sinterp_natural_mesh and gsl_sinterp_cubic_mesh (dim 2): simplices [(dim + 1) n] (vertex = row of x), neighbours [(dim + 1) n] (opposite vertex k,
   -1 = boundary) or NULL (derived by edge / face matching); copied, validated by the next gsl_sinterp_init */
int gsl_sinterp_set_triangulation(gsl_sinterp *interp, const int *triangles, const int *neighbours, size_t n_triangles);
/* gsl_sinterp_cubic_mesh / _simplex (every other type: GSL_EINVAL).  set_gradients, before init: the N x 2 gradients
   to interpolate instead of the estimate (copied; GSL_EBADLEN for another shape; NULL returns to the estimate).
   set_gradient_options, before init: the stopping rule of the estimate, |r| / |b| <= rtol or maxiter iterations
   (defaults 1e-12, 1000; 0 < rtol < 1 and maxiter >= 1, otherwise GSL_EINVAL).  get_gradients, after init: the
   gradients in use (N x 2, may be NULL), the iterations the estimate took (0 for given or restored gradients) and its
   relative residual (either may be NULL).  get_gradients also serves gsl_sinterp_shepard: the N x dim nodal gradients,
   iterations 0, residual 0. */
int gsl_sinterp_set_gradients(gsl_sinterp *interp, const gsl_matrix *gradients);
int gsl_sinterp_set_gradient_options(gsl_sinterp *interp, double rtol, size_t maxiter);
int gsl_sinterp_get_gradients(const gsl_sinterp *interp, gsl_matrix *gradients, size_t *iterations, double *residual);
int gsl_sinterp_init(gsl_sinterp *interp, const gsl_matrix *x, const gsl_vector *f);
const char *gsl_sinterp_name(const gsl_sinterp *interp);
unsigned int gsl_sinterp_min_size(const gsl_sinterp *interp);
int gsl_sinterp_eval_e(const gsl_sinterp *interp, const gsl_vector *y, double *s);
double gsl_sinterp_eval(const gsl_sinterp *interp, const gsl_vector *y);
int gsl_sinterp_eval_many(const gsl_sinterp *interp, const gsl_matrix *y, gsl_vector *s, int *leaf);
int gsl_sinterp_eval_resident(const gsl_sinterp *interp, const double *d_y, size_t m, size_t ytda,
                              double *d_s, int *d_leaf);
/* Value and gradient (the counterpart of gsl_interp_eval_deriv_e, interpolation/gsl_interp.h:113-123, in dim dimensions):
   s(y) and ds/dy_a, a < dim, from one fused sweep (gsl_sinterp_hip_rbf_eval_grad) -- the analytic gradient of the radial
   sum plus the affine tail (gsl_sinterp_rbf_tps_affine) or nothing (kriging's mean is constant).  Every RBF-family
   type (kriging included) is supported; gsl_sinterp_linear_simplex and gsl_sinterp_linear_mesh give GSL_EUNSUP (their gradient is constant
   per leaf: gsl_sinterp_linear_eval_fields_* below, K = 1 after a plain init).  The value is bit-identical to gsl_sinterp_eval_many's for the same target; a target with a
   NaN coordinate gets NaN in the value and in every gradient component.
   eval_grad_many: y is m x dim, g is m x dim (g->tda honoured, padding untouched), s has m entries (s->stride honoured)
   or is NULL for a gradient-only call.  eval_grad_e: one target, g has dim entries; *s and g are NaN on failure.
   eval_grad_resident: everything in HBM, row k of the gradient at d_g + k * gtda (gtda >= dim), d_s may be NULL.
   GSL_EFAULT: a NULL argument; GSL_EUNSUP: a linear type; GSL_EBADLEN: y->size2 != dim, g not y->size1 x dim, s->size
   != y->size1; GSL_EINVAL: not initialised (or gtda < dim).  An interpolant restored by gsl_sinterp_fread evaluates
   gradients: centres, weights, mean and polynomial are all a gradient needs.  With a device list the first device
   evaluates every target, as gsl_sinterp_eval_resident and the variance entries do: gradient batches are not sharded
   over the group, and eval_grad_many copies through plain (not pinned, not pipelined) staging.
   gsl_sinterp_cubic_mesh / _simplex: the analytic gradient of the Clough-Tocher cubic in the micro-triangle of the
   target, continuous across every edge; same shapes; a target outside the triangulation gets NaN and GSL_EDOM (many / e;
   the resident entry does not read back).  d_s == NULL in the resident entry is GSL_EFAULT for these two types (the
   locate step passes its values through it).
   gsl_sinterp_shepard: the analytic gradient of the modified Shepard interpolant, continuous everywhere; same shapes, d_s
   may be NULL; a target no node covers gets NaN and GSL_EDOM (all three entries: the sweep reports its count). */
int gsl_sinterp_eval_grad_e(const gsl_sinterp *interp, const gsl_vector *y, double *s, gsl_vector *g);
int gsl_sinterp_eval_grad_many(const gsl_sinterp *interp, const gsl_matrix *y, gsl_vector *s /* may be NULL */, gsl_matrix *g);
int gsl_sinterp_eval_grad_resident(const gsl_sinterp *interp, const double *d_y, size_t m, size_t ytda,
                                   double *d_s /* may be NULL */, double *d_g, size_t gtda);
/* Several fields on one set of centres (the RBF family; SciPy's RBFInterpolator takes d of shape (N, K) the same way):
   temperature, pressure and humidity at the stations, or the components of a vector field.  gsl_sinterp_init_fields(x, F)
   takes F of size x K (F->tda honoured, 1 <= K <= GSL_SINTERP_MAX_FIELDS = 64) and solves all K weight vectors; the
   eval_fields entries return the K values of a target from ONE sweep, in which the distance, the take test and the kernel
   of a (target, centre) pair are computed once for all fields.
   WHICH TYPES SHARE THE FACTORISATION: gsl_sinterp_rbf_gaussian, _wendland, _matern32, _matern52, _imq and the three kriging
   types with the default solver and without gsl_sinterp_set_rcond pay ONE fill and ONE Cholesky factorisation for all K fields
   (gsl_sinterp_route 1 / 7).  gsl_sinterp_rbf_tps and gsl_sinterp_rbf_tps_affine, a non-default gsl_sinterp_set_solver,
   gsl_sinterp_set_rcond, and kriging on a covariance matrix that is only semi-definite solve field by field -- correct, at
   the price of K factorisations; gsl_sinterp_route is then the last field's, gsl_sinterp_rcond the first field's.
   To every other entry a K-field interpolant IS field 0's interpolant: eval_e / _many / _resident, the gradient entries,
   eval_grid, get_weights, mean and poly; gsl_sinterp_eval_many returns the bits of column 0 of eval_fields_many.  The
   kriging variance does not depend on the responses: gsl_sinterp_set_variance is honoured by init_fields (shared route)
   and the variance entries work unchanged.  gsl_sinterp_init after init_fields returns the interpolant to one field, a
   second init_fields may change K; the eval_fields entries work on a one-field interpolant with K = 1.
   gsl_sinterp_n_fields: 0 before the first init, 1 after gsl_sinterp_init / gsl_sinterp_fread (the natural-neighbour,
   Clough-Tocher and Shepard types: always 0; the linear types: K after gsl_sinterp_linear_init_fields).
   eval_fields_many: y is m x dim, S is m x K (S->tda honoured, padding untouched).  eval_fields_e: s has K entries, NaN
   on failure.  eval_fields_resident: everything in HBM, target k's field q at d_s[k * stda + q] (stda >= K).
   get_field_weights / field_mean (kriging) / field_poly (affine thin-plate spline) read field q back.
   GSL_EFAULT: a NULL argument; GSL_EUNSUP: gsl_sinterp_linear_simplex / gsl_sinterp_linear_mesh (several responses per
   leaf are the separate entries gsl_sinterp_linear_init_fields / _eval_fields_* below); GSL_EBADLEN: F->size1 != size,
   x not size x dim, y->size2 != dim, S not m x K, a vector whose length is not K / size / dim + 1, q >= K; GSL_EINVAL: not initialised, K = 0 or K > 64, stda < K, mean /
   poly asked of another type.  With a device list the model is broadcast whole and the first device evaluates every
   fields batch through plain staging (not sharded, not pipelined).  gsl_sinterp_fwrite of an interpolant with more than
   one field returns GSL_EUNSUP and writes nothing: the GSLSINT1 format holds one weight vector. */
int gsl_sinterp_init_fields(gsl_sinterp *interp, const gsl_matrix *x, const gsl_matrix *F);
size_t gsl_sinterp_n_fields(const gsl_sinterp *interp);
int gsl_sinterp_eval_fields_e(const gsl_sinterp *interp, const gsl_vector *y, gsl_vector *s);
int gsl_sinterp_eval_fields_many(const gsl_sinterp *interp, const gsl_matrix *y, gsl_matrix *S);
int gsl_sinterp_eval_fields_resident(const gsl_sinterp *interp, const double *d_y, size_t m, size_t ytda, double *d_s, size_t stda);
int gsl_sinterp_get_field_weights(const gsl_sinterp *interp, size_t q, gsl_vector *w);
int gsl_sinterp_field_mean(const gsl_sinterp *interp, size_t q, double *mean);
int gsl_sinterp_field_poly(const gsl_sinterp *interp, size_t q, gsl_vector *c);
/* Several responses on the piecewise-linear types, and their gradients ("Several responses on a mesh"): the
   separate entries the refusals of gsl_sinterp_init_fields and gsl_sinterp_eval_grad_* name.  They serve
   gsl_sinterp_linear_simplex and gsl_sinterp_linear_mesh (dim 2 and 3); every other type answers GSL_EUNSUP before
   anything touches the device.  SciPy's LinearNDInterpolator takes values of shape (N, K) the same way.
   linear_init_fields(x, F): F is size x K (F->tda honoured, 1 <= K <= GSL_SINTERP_MAX_FIELDS).  Builds the tree or
   validates the imported triangulation exactly as gsl_sinterp_init(x, column 0 of F) does -- set_tree_options,
   set_triangulation and the device(s) honoured -- then binds all K columns.  To every other entry the result IS field
   0's interpolant: eval_e / _many / _resident / _grid return the bits they return after gsl_sinterp_init(x, F[:, 0]);
   gsl_sinterp_n_fields is K.  gsl_sinterp_init afterwards returns the interpolant to one field; a second
   linear_init_fields may change K.  An interpolant initialised by gsl_sinterp_init or restored by gsl_sinterp_fread
   answers the eval entries with K = 1: the linear gradient entry.  gsl_sinterp_fwrite with K > 1 is GSL_EUNSUP and
   writes nothing.
   The eval entries locate every target ONCE (the unchanged locate of gsl_sinterp_eval_many) and take the K values and,
   when asked, the K gradients from the simplex found: column q of S holds the bits gsl_sinterp_eval_many returns
   after gsl_sinterp_init(x, F[:, q]); the gradient of field q is that of the affine function of the located simplex
   (on a leaf that touches the cage of gsl_sinterp_linear_simplex the cage vertices carry 0, as in the value), in raw
   coordinates, the same bits for every target of a simplex; the value bits do not depend on whether gradients are asked.
   eval_fields_e: s has K entries, g is K x dim or NULL; NaN on failure.  eval_fields_many: y m x dim, S m x K, G (or
   NULL) m x (K dim) with entry (k, q dim + a) = d(field q)/dy_a, leaf (or NULL) m ints; every tda honoured, padding
   untouched.  A target outside gives a NaN row, leaf -1 and GSL_EDOM after every other row has been stored.
   eval_fields_resident: everything in HBM, rows at d_S + k * stda and d_G + k * gtda; nothing is read back.
   GSL_EFAULT: NULL; GSL_EUNSUP: another type; GSL_EBADLEN: shapes; GSL_EINVAL: not initialised, K = 0 or K > 64, stda <
   K or gtda < K dim.  With a device list the first device evaluates every target of these entries (field batches are
   not sharded), and the _many entry copies through plain staging. */
int gsl_sinterp_linear_init_fields(gsl_sinterp *interp, const gsl_matrix *x, const gsl_matrix *F);
int gsl_sinterp_linear_eval_fields_e(const gsl_sinterp *interp, const gsl_vector *y, gsl_vector *s, gsl_matrix *g /* K x dim or NULL */);
int gsl_sinterp_linear_eval_fields_many(const gsl_sinterp *interp, const gsl_matrix *y, gsl_matrix *S, gsl_matrix *G /* or NULL */,
                                        int *leaf /* or NULL */);
int gsl_sinterp_linear_eval_fields_resident(const gsl_sinterp *interp, const double *d_y, size_t m, size_t ytda, double *d_S, size_t stda,
                                            double *d_G /* or NULL */, size_t gtda, int *d_leaf /* or NULL */);
/* Gridded front-end (interpolation/scattered_interp_example.c:175-217): evaluate on the regular grid
   x_i = min[0] + i (max[0]-min[0])/n0, y_j = min[1] + j (max[1]-min[1])/n1 (the reference's steps: range / n_grid,
   the upper bounds excluded) with n0 = grid->size1, n1 = grid->size2; grid(i, j) receives the value.  The
   targets are generated on the device; dim = 2 interpolants only.  gsl_sinterp_fprintf_grid writes the grid in
   the reference's /tmp/plot.dat form ("%g %g %g" per node, a blank line after each i). */
int gsl_sinterp_eval_grid(const gsl_sinterp *interp, const gsl_vector *min, const gsl_vector *max, gsl_matrix *grid);
int gsl_sinterp_fprintf_grid(FILE *stream, const gsl_vector *min, const gsl_vector *max, const gsl_matrix *grid);
/* Binary checkpoint of an INITIALISED interpolant (RBF: centres + solved weights; linear simplex: the built
   history DAG + data + response), gsl_matrix_fwrite / _fread conventions (native byte order, GSL_EFAILED on a
   short transfer).  fread needs an interpolant allocated with the same type, dim and size (GSL_EBADLEN
   otherwise) and leaves it ready to evaluate: nothing is solved or triangulated again. */
int gsl_sinterp_fwrite(FILE *stream, const gsl_sinterp *interp);
int gsl_sinterp_fread(FILE *stream, gsl_sinterp *interp);
/* RBF types: copy the solved weights (length size) to the host. */
int gsl_sinterp_get_weights(const gsl_sinterp *interp, gsl_vector *w);
void gsl_sinterp_free(gsl_sinterp *interp);

#ifdef __cplusplus
}
#endif
#endif
