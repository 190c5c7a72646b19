/*
 * gsl_sinterp_hip.h -- C-ABI of the MI355X (gfx950) kernels behind the
 * scattered-interpolation hot path.  Plain pointers and sizes only; every
 * `d_*` argument is a DEVICE pointer (hipMalloc / torch data_ptr), every
 * `h_*` argument a host pointer.  All entry points return a GSL status code
 * (include/gsl_sinterp_compat.h) and never abort; the text of the last failure
 * is kept per context (gsl_sinterp_hip_last_error).
 *
 * Work is enqueued on the context's stream and is asynchronous unless the
 * entry point has a host-side output (`info`, `signum`), in which case it
 * synchronises the stream before returning.
 *
 * Reference routines each entry point replaces (paths under the reference
 * tree, smithzvk/gsl-scattered-interpolation):
 *   tree_pack + bary_eval   interpolation/linear_simplex.c:331-402 (find_leaf/_find_leaf),
 *                           :607-651 (calculate_bary_coords), :653-676 (contains_point),
 *                           :678-711 (interp_point); linalg/lu.c:59-201 at d=2
 *   rbf_fill                (no reference code; README:18-26) Phi_ij = phi(|x_i-x_j|)
 *   cholesky_decomp1        linalg/cholesky.c:88-131  (gsl_linalg_cholesky_decomp1)
 *   cholesky_svx            linalg/cholesky.c:163-185 (gsl_linalg_cholesky_svx)
 *   lu_decomp / lu_svx      linalg/lu.c:59-124, :166-201 (gsl_linalg_LU_decomp / _svx)
 *   rbf_eval                (no reference code) s(y) = sum_j w_j phi(|y-x_j|)
 *   tree_check              interpolation/linear_simplex_integrity_check.c:62-119 (_check_leaf_nodes),
 *                           :134-160 (_check_delaunay)
 */
#ifndef GSL_SINTERP_HIP_H
#define GSL_SINTERP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gsl_sinterp_hip_ctx gsl_sinterp_hip_ctx;

/* radial kernels */
#define GSL_SINTERP_RBF_GAUSSIAN 0 /* phi(r) = exp(-(eps r)^2)                      */
#define GSL_SINTERP_RBF_TPS 1      /* phi(r) = r^2 ln r = 0.5 r^2 ln r^2, phi(0)=0  */
#define GSL_SINTERP_RBF_WENDLAND 2 /* phi(r) = (1 - eps r)_+^4 (4 eps r + 1): Wendland's C2 function, compact support of
                                      radius 1/eps, positive definite for dim <= 3 (the reference's README:18-26 lists
                                      compactly supported kernels as future work); Cholesky route, sweep with EXACT culling */
/* Matern 3/2 and 5/2 and the inverse multiquadric: positive definite in every dimension, length scale 1/eps, phi(0) = 1
   exactly.  Cholesky route, kriging covariances, and the PLAIN sweep: every centre in input order, nothing culled (the
   inverse multiquadric does not decay; the Matern cut-off radius at a usable eps spans a third of the cloud).  A NaN
   coordinate of a target gives NaN; the result for an INFINITE coordinate is not pinned (the Matern formula meets
   inf * 0 there).  Every other value of kind is unknown: GSL_EINVAL. */
#define GSL_SINTERP_RBF_MATERN32 3 /* phi(r) = (1 + t) exp(-t),          t = sqrt(3) eps r  */
#define GSL_SINTERP_RBF_MATERN52 4 /* phi(r) = (1 + t + t^2/3) exp(-t),  t = sqrt(5) eps r  */
#define GSL_SINTERP_RBF_IMQ 5      /* phi(r) = 1 / sqrt(1 + (eps r)^2)                      */

/* ---- context / memory --------------------------------------------------- */
int gsl_sinterp_hip_device_count(void); /* 0 when no GPU is visible */
/* stream: a hipStream_t owned by the caller (e.g. torch's current stream); NULL is
   the device's default stream, i.e. ordered with the caller's other default-stream
   work.  ctx_own_stream switches the context to a private non-blocking stream
   (for overlap with other streams; the caller then orders work explicitly). */
int gsl_sinterp_hip_ctx_create(gsl_sinterp_hip_ctx **ctx, int device, void *stream);
int gsl_sinterp_hip_ctx_own_stream(gsl_sinterp_hip_ctx *ctx);
void gsl_sinterp_hip_ctx_destroy(gsl_sinterp_hip_ctx *ctx);
int gsl_sinterp_hip_ctx_device(const gsl_sinterp_hip_ctx *ctx);   /* the ordinal the context was created on, -1 for NULL */
int gsl_sinterp_hip_sync(gsl_sinterp_hip_ctx *ctx);
const char *gsl_sinterp_hip_last_error(const gsl_sinterp_hip_ctx *ctx);
int gsl_sinterp_hip_malloc(gsl_sinterp_hip_ctx *ctx, void **d_ptr, size_t bytes);
int gsl_sinterp_hip_free(gsl_sinterp_hip_ctx *ctx, void *d_ptr);
int gsl_sinterp_hip_h2d(gsl_sinterp_hip_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
int gsl_sinterp_hip_d2h(gsl_sinterp_hip_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);
/* hipEvent pair on the context's stream (bench / roofline timing) */
int gsl_sinterp_hip_timer_start(gsl_sinterp_hip_ctx *ctx);
int gsl_sinterp_hip_timer_stop(gsl_sinterp_hip_ctx *ctx, float *h_ms);

/* ---- device groups: target shards over several GPUs of one node -------- */
/* One context per listed device (each on a private stream, so one host thread keeps all devices
   busy) and ONE collective: gsl_sinterp_hip_group_broadcast replicates a model buffer from member 0
   to every member -- ncclBroadcast over xGMI on a communicator made by ncclCommInitAll (RCCL is
   bound with dlopen when the first multi-device group is created).  A list that names one ordinal
   twice (one-GPU test boxes) or GSL_SINTERP_NO_RCCL=1 replicates with hipMemcpyPeerAsync instead;
   gsl_sinterp_hip_group_transport says which ("rccl" / "peer-copy" / "none").  There is no
   reduction and no all-to-all on the path; the factorisation runs on member 0 only. */
typedef struct gsl_sinterp_hip_group gsl_sinterp_hip_group;
int gsl_sinterp_hip_group_create(gsl_sinterp_hip_group **grp, const int *devices, int n_devices);
void gsl_sinterp_hip_group_destroy(gsl_sinterp_hip_group *grp);
int gsl_sinterp_hip_group_size(const gsl_sinterp_hip_group *grp);
int gsl_sinterp_hip_group_device(const gsl_sinterp_hip_group *grp, int member);
gsl_sinterp_hip_ctx *gsl_sinterp_hip_group_ctx(gsl_sinterp_hip_group *grp, int member);
const char *gsl_sinterp_hip_group_transport(const gsl_sinterp_hip_group *grp);
const char *gsl_sinterp_hip_group_last_error(const gsl_sinterp_hip_group *grp);
/* d_bufs[i]: `bytes` bytes on member i; member 0's content goes to all (stream ordered, asynchronous) */
int gsl_sinterp_hip_group_broadcast(gsl_sinterp_hip_group *grp, void *const *d_bufs, size_t bytes);
/* the shard rule: contiguous ceil(m/world)-sized shards, every target exactly once */
void gsl_sinterp_hip_shard_bounds(size_t m_total, int world, int rank, size_t *first, size_t *count);
/* asynchronous copies on the context's stream + pinned host staging for them */
int gsl_sinterp_hip_h2d_async(gsl_sinterp_hip_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
int gsl_sinterp_hip_d2h_async(gsl_sinterp_hip_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);
int gsl_sinterp_hip_d2d_async(gsl_sinterp_hip_ctx *ctx, void *d_dst, const void *d_src, size_t bytes);   /* both on the context's device */
int gsl_sinterp_hip_host_alloc(void **h_ptr, size_t bytes);
void gsl_sinterp_hip_host_free(void *h_ptr);
/* copy pipe of one context: an upload and a download stream beside the context's stream, so that the chunks of a host
   batch overlap H2D | sweep | D2H.  upload: later work on the context's stream waits for the copy; download: the copy
   waits for the work enqueued on the context's stream up to a mark (or so far).  Pinned host buffers, untouched until pipe_sync (which
   also synchronises the context's stream).  At most 64 copies between two syncs. */
typedef struct gsl_sinterp_hip_pipe gsl_sinterp_hip_pipe;
int gsl_sinterp_hip_pipe_create(gsl_sinterp_hip_ctx *ctx, gsl_sinterp_hip_pipe **out);
void gsl_sinterp_hip_pipe_destroy(gsl_sinterp_hip_pipe *pipe);
int gsl_sinterp_hip_pipe_upload(gsl_sinterp_hip_pipe *pipe, void *d_dst, const void *h_src, size_t bytes);
int gsl_sinterp_hip_pipe_mark(gsl_sinterp_hip_pipe *pipe, int *mark);      /* "the context's stream up to here" */
int gsl_sinterp_hip_pipe_download(gsl_sinterp_hip_pipe *pipe, int mark, void *h_dst, const void *d_src, size_t bytes);   /* mark < 0: now */
int gsl_sinterp_hip_pipe_sync(gsl_sinterp_hip_pipe *pipe);
/* number of negative entries of d_v[0 .. m) (-1 = outside the cage / mesh); synchronises the context's stream */
int gsl_sinterp_hip_count_negative(gsl_sinterp_hip_ctx *ctx, const int *d_v, size_t m, long long *h_count);

/* ---- barycentric evaluation over a host-built Delaunay history DAG ------- */
/* One 64-byte record per DAG node (see DESIGN.md "HBM layout"). */
#define GSL_SINTERP_TREE_RECORD_BYTES 64
#define GSL_SINTERP_TREE_LEAFTAB_BYTES 32

/* Build the node records on the device.  d_type[n_nodes] (0 leaf, 1 sub_{d+1},
   2 sub_d), d_pidx/d_links [3*n_nodes] exactly as the reference keeps them
   (linear_simplex.h:31-59), d_points [2*n_points] in INSERTION order
   (row shuffle[i] of the data matrix), h_geom[10] = seed_points(3x2, row-major),
   shift(2), scale(2).  The per-node 2x2 LU is computed with the reference's
   operation sequence (no FMA contraction) so it is bit-identical to the host. */
int gsl_sinterp_hip_tree_pack(gsl_sinterp_hip_ctx *ctx, int n_nodes, const int *d_type,
                              const int *d_pidx, const int *d_links, int n_points,
                              const double *d_points, const double *h_geom, void *d_records);
/* Per-node table of the three vertex responses (+ seed mask); d_response is in
   insertion order (response[shuffle[i]]). */
int gsl_sinterp_hip_tree_bind(gsl_sinterp_hip_ctx *ctx, int n_nodes, const int *d_pidx,
                              int n_points, const double *d_response, void *d_leaftab);
/* Locate + interpolate m targets (row k at d_targets + k*ttda).  d_leaf may be
   NULL.  Target outside the cage: leaf = -1, value = NaN, and *h_n_outside
   (may be NULL; forces a sync when given) counts them -> GSL_EDOM. */
int gsl_sinterp_hip_bary_eval(gsl_sinterp_hip_ctx *ctx, int n_nodes, const void *d_records,
                              const void *d_leaftab, const double *h_scale,
                              const double *d_targets, size_t m, size_t ttda, double *d_values,
                              int *d_leaf, long long *h_n_outside);

/* Imported triangulation (no DAG): records + seed grid, then locate + interpolate.  d_tri / d_nbr [3 n_tri] (vertex ids =
   rows of d_points; neighbour across the edge opposite vertex k, -1 = hull), d_points [2 n_points] in ROW order,
   h_geom[8] = shift(2), scale(2), bounding box lo0, lo1, hi0, hi1 of the points; G: cells per axis of the seed grid,
   d_seed: 2 G^2 ints.  Leaf table: gsl_sinterp_hip_tree_bind with d_pidx = d_tri.  convex = 0: a walk stopped by a
   hull edge is resolved by an exhaustive scan instead of "outside". */
int gsl_sinterp_hip_mesh_pack(gsl_sinterp_hip_ctx *ctx, int n_tri, const int *d_tri, const int *d_nbr, int n_points,
                              const double *d_points, const double *h_geom, int G, void *d_records, int *d_seed);
int gsl_sinterp_hip_mesh_eval(gsl_sinterp_hip_ctx *ctx, int n_tri, const void *d_records, const void *d_leaftab,
                              const int *d_seed, int G, const double *h_geom, int convex, const double *d_targets,
                              size_t m, size_t ttda, double *d_values, int *d_tri, long long *h_n_outside);

/* Imported tetrahedral mesh (csrc/hip/mesh3.hip): the same route one dimension up.  One 128-byte, 128-byte-aligned
   record per tetrahedron (standardised last vertex, inverse of the standardised 3x3 edge matrix, four neighbour ids, a
   meta word whose bit 0 marks a flat tetrahedron) and a 32-byte table of the four vertex responses.
   d_tet / d_nbr [4 n_tet] (vertex ids = rows of d_points; neighbour across the face opposite vertex k, -1 = hull),
   d_points [3 n_points] in ROW order, h_geom[12] = shift(3), scale(3), bounding box lo(3), hi(3) of the points;
   G <= GSL_SINTERP_MESH3_MAX_GRID: cells per axis of the seed grid, d_seed: 2 G^3 + 2 ints.  mesh3_bind fills the
   response table from d_response [n_points] (row order).  mesh3_eval: targets at d_targets + k * ttda, ttda >= 3;
   d_tet may be NULL; a target outside the mesh gives index -1 and NaN and is counted in *h_n_outside (may be NULL;
   forces a sync when given) -> GSL_EDOM.  convex = 0: a walk stopped by hull faces is resolved by an exhaustive scan
   instead of "outside". */
#define GSL_SINTERP_MESH3_RECORD_BYTES 128
#define GSL_SINTERP_MESH3_TABLE_BYTES 32
#define GSL_SINTERP_MESH3_MAX_GRID 160
int gsl_sinterp_hip_mesh3_pack(gsl_sinterp_hip_ctx *ctx, int n_tet, const int *d_tet, const int *d_nbr, int n_points,
                               const double *d_points, const double *h_geom, int G, void *d_records, int *d_seed);
int gsl_sinterp_hip_mesh3_bind(gsl_sinterp_hip_ctx *ctx, int n_tet, const int *d_tet, int n_points, const double *d_response,
                               void *d_table);
int gsl_sinterp_hip_mesh3_eval(gsl_sinterp_hip_ctx *ctx, int n_tet, const void *d_records, const void *d_table,
                               const int *d_seed, int G, const double *h_geom, int convex, const double *d_targets,
                               size_t m, size_t ttda, double *d_values, int *d_tet, long long *h_n_outside);

/* Several responses on the piecewise-linear types, with per-simplex gradients (csrc/hip/linear_fields.hip; DESIGN.md 4,
   "Several responses on a mesh").  A located sweep: d_located [m] = the simplex of every target as
   gsl_sinterp_hip_bary_eval, gsl_sinterp_hip_mesh_eval (bary_fields_eval) or gsl_sinterp_hip_mesh3_eval
   (mesh3_fields_eval) stored it for the same targets (run it first).  d_records: the records of tree_pack / mesh_pack /
   mesh3_pack, unchanged.  d_vertices [3 n_simplices] (d_tet [4 n_tet]): the vertex ids the matching *_bind call takes
   (the DAG's d_pidx, insertion order, < 0 = cage; or the triangles / tetrahedra of an imported mesh, row order).
   d_F: n_points x nf, row v at d_F + v * ftda, in that vertex order; no per-simplex table is built, the rows are
   gathered.  h_scale [2]: the scale tree_pack / mesh_pack were given; h_geom [12]: as for mesh3_pack (shift and scale
   are read).  1 <= nf <= GSL_SINTERP_MAX_FIELDS.
   d_S[k * stda + q] = field q at target k: the bits the scalar kernel stores in d_values[k] when its table is bound to
   column q (same coordinates, same order of operations, cage vertices masked).  One exception: a target the exact DAG
   walk left in a leaf whose record is flagged singular gets that record's own (non-finite) coordinates here, where
   the walk kept those of the last regular node it passed.
   d_G (may be NULL; the value bits do not depend on it): d_G[k * gtda + q * dim + a] = d/dy_a, in raw coordinates, of
   the affine function field q's value is taken from in the located simplex, formed from the record (2-D: two
   triangular solves with its LU; 3-D: its inverse) and the dim response differences, a cage vertex carrying 0 as in
   the value: constant per simplex, equal bits for every target in it.
   d_located[k] < 0 (or not below n_simplices): NaN in the nf values and the nf dim gradient components of row k.
   Padding between nf and stda, and between nf dim and gtda, is not written.  GSL_EINVAL (nf < 1, nf > 64, ftda or
   stda < nf, gtda < nf dim with d_G given, ttda < dim) and GSL_EFAULT (NULL) are decided before anything touches the
   device; m = 0 is success; asynchronous on the context's stream. */
int gsl_sinterp_hip_bary_fields_eval(gsl_sinterp_hip_ctx *ctx, int n_simplices, const void *d_records, const int *d_vertices,
                                     int n_points, const double *d_F, int nf, size_t ftda, const double *h_scale,
                                     const int *d_located, const double *d_targets, size_t m, size_t ttda, double *d_S,
                                     size_t stda, double *d_G, size_t gtda);
int gsl_sinterp_hip_mesh3_fields_eval(gsl_sinterp_hip_ctx *ctx, int n_tet, const void *d_records, const int *d_tet, int n_points,
                                      const double *d_F, int nf, size_t ftda, const double *h_geom, const int *d_located,
                                      const double *d_targets, size_t m, size_t ttda, double *d_S, size_t stda, double *d_G,
                                      size_t gtda);
/* 1 when a located sweep (bary_eval, mesh_eval, mesh3_eval) reorders a batch of m targets into cell order before it
   walks (the sorted-target route), 0 when it walks them as given: the route helper itself, GSL_SINTERP_NO_SORT included */
int gsl_sinterp_hip_sort_wanted(size_t m);

/* Natural-neighbour (Sibson) interpolation on a 2-D Delaunay mesh (csrc/hip/natural.hip; DESIGN.md 4, "Natural
   neighbours").  natural_pack: one 80-byte, 16-byte-aligned record per triangle in METRIC coordinates (raw coordinate
   times h_metric[axis]: {1, 1} for a mesh that is Delaunay as given, the mesh's per-axis scale for one that is Delaunay
   in standardised coordinates): vertices reordered counter-clockwise with the neighbour slots permuted to match, the
   circumcentre, a flat flag.  d_nnrec holds n_tri + 1 records; the last one carries the metric.  d_tri / d_nbr /
   d_points as for gsl_sinterp_hip_mesh_pack.
   natural_eval: d_located [m] = the triangle of every target and d_linear_values [m] = its piecewise-linear value, both
   as gsl_sinterp_hip_mesh_eval stored them for the same targets (run it first); d_leaftab = the response table of
   gsl_sinterp_hip_tree_bind.  d_values may be d_linear_values.  One lane per target walks the cavity; depth_cap = the
   pending triangles a lane may hold (0 = the default, GSL_SINTERP_NATURAL_STACK, also the maximum); a target that needs
   more is evaluated by a scan over all triangles, and *h_n_scanned (may be NULL; forces a sync when given) counts
   those.  A target on a site returns the datum; one within rounding of the hull returns the linear value; d_located
   < 0 gives NaN. */
#define GSL_SINTERP_NATURAL_RECORD_BYTES 80
#define GSL_SINTERP_NATURAL_STACK 16
int gsl_sinterp_hip_mesh_natural_pack(gsl_sinterp_hip_ctx *ctx, int n_tri, const int *d_tri, const int *d_nbr, int n_points,
                                      const double *d_points, const double *h_metric, void *d_nnrec);
int gsl_sinterp_hip_mesh_natural_eval(gsl_sinterp_hip_ctx *ctx, int n_tri, const void *d_nnrec, const void *d_leaftab,
                                      const int *d_located, const double *d_linear_values, const double *d_targets, size_t m,
                                      size_t ttda, int depth_cap, double *d_values, long long *h_n_scanned);

/* Clough-Tocher C1 piecewise-cubic interpolation on a 2-D mesh, with gradients (csrc/hip/cubic.hip; DESIGN.md 4,
   "Clough-Tocher").  No Delaunay property and no convexity is needed.
   cubic_gradients: the global estimate of grad f at the vertices (Nielson / Renka, scipy's CloughTocher2DInterpolator):
   the SPD system over the undirected mesh edges, solved by conjugate gradients preconditioned with the inverse 2x2
   diagonal blocks.  The CSR d_offsets [n_points + 1] / d_adjacent [n_adjacent] lists every undirected edge once per
   endpoint (simplex_mesh_vertex_adjacency); entries out of range, self-edges and edges of length 0 are skipped; a
   vertex without two non-collinear edges gets g = 0 and is left out.  d_g [2 n_points] receives the gradients.  The
   solve stops at |r| / |b| <= rtol or after maxiter iterations; *h_iterations / *h_residual (may be NULL) receive the
   count and the achieved relative residual in either case; GSL_EMAXITER (11) when rtol was not met.  Synchronises.
   The dot products are reduced in a fixed order: the same input gives the same bits.
   cubic_pack: one 160-byte, 16-byte-aligned record per triangle: the barycentric map (raw coordinates) and the 12
   independent Bezier ordinates; d_f [n_points], d_g [2 n_points]; d_tri / d_nbr / d_points as for
   gsl_sinterp_hip_mesh_pack.  d_ctrec holds n_tri records.
   cubic_eval: d_located [m] = the triangle of every target and d_linear_values [m] = its piecewise-linear value, both
   as gsl_sinterp_hip_mesh_eval stored them for the same targets (run it first); d_values may be d_linear_values.
   d_grad (may be NULL) receives the gradient in raw coordinates, row k at d_grad + k * gtda, gtda >= 2; the value bits
   do not depend on it.  d_located < 0 gives NaN in the value and the gradient; a flat triangle gives the linear value
   and the gradient of the plane through its data (NaN when there is none). */
#define GSL_SINTERP_CUBIC_RECORD_BYTES 160
int gsl_sinterp_hip_mesh_cubic_gradients(gsl_sinterp_hip_ctx *ctx, int n_points, const int *d_offsets, const int *d_adjacent,
                                         size_t n_adjacent, const double *d_points, const double *d_f, double rtol, int maxiter,
                                         double *d_g, int *h_iterations, double *h_residual);
int gsl_sinterp_hip_mesh_cubic_pack(gsl_sinterp_hip_ctx *ctx, int n_tri, const int *d_tri, const int *d_nbr, int n_points,
                                    const double *d_points, const double *d_f, const double *d_g, void *d_ctrec);
int gsl_sinterp_hip_mesh_cubic_eval(gsl_sinterp_hip_ctx *ctx, int n_tri, const void *d_ctrec, const int *d_located,
                                    const double *d_linear_values, const double *d_targets, size_t m, size_t ttda,
                                    double *d_values, double *d_grad, size_t gtda);

/* Device-side integrity checks of a DAG given as raw arrays (same arguments as tree_pack):
   what & 1: _check_leaf_nodes  (interpolation/linear_simplex_integrity_check.c:62-119), one thread per leaf;
   what & 2: _check_delaunay    (:134-160; circumsphere per linear_simplex.c:555-605), leaves x points.
   Counts of violating leaves / (leaf, point) pairs come back in *h_leaf_violations / *h_delaunay_violations
   (0 = the reference's asserts would all hold); h_first[3] (may be NULL) = first bad leaf of either check
   and one witness point, -1 when clean.  Synchronises the stream. */
int gsl_sinterp_hip_tree_check(gsl_sinterp_hip_ctx *ctx, int n_nodes, const int *d_type, const int *d_pidx,
                               const int *d_links, int n_points, const double *d_points, const double *h_geom,
                               int what, long long *h_leaf_violations, long long *h_delaunay_violations,
                               int *h_first);

/* ---- RBF: fill, dense solve, evaluation sweep ----------------------------- */
int gsl_sinterp_hip_rbf_fill(gsl_sinterp_hip_ctx *ctx, int kind, double eps, const double *d_x,
                             size_t n, int dim, size_t xtda, double *d_phi, size_t lda);
/* In-place A = L L^T, L in the lower triangle, original A kept in the strict
   upper triangle; *h_info = 0, or j+1 when pivot j <= 0 (-> GSL_EDOM). */
int gsl_sinterp_hip_cholesky_decomp1(gsl_sinterp_hip_ctx *ctx, size_t n, double *d_a, size_t lda,
                                     int *h_info);
int gsl_sinterp_hip_cholesky_svx(gsl_sinterp_hip_ctx *ctx, size_t n, const double *d_llt,
                                 size_t lda, double *d_x);
/* cholesky_decomp1 followed by the solve of nrhs (1 <= nrhs <= 5) right-hand sides in place: column q at d_x + q*ldx
   (ldx >= n) holds b_q on entry and A^-1 b_q on exit.  d_a, *h_info and the status as for cholesky_decomp1 (GSL_EDOM
   and the failing column; d_x is then undefined).  When n is a multiple of 128, lda is even and d_a is 16-byte
   aligned, the forward substitution runs inside the factorisation (d_x needs only 8-byte alignment); otherwise the
   two sweeps of cholesky_svx follow it. */
int gsl_sinterp_hip_cholesky_factor_solve(gsl_sinterp_hip_ctx *ctx, size_t n, double *d_a, size_t lda, int *h_info,
                                          double *d_x, size_t ldx, int nrhs);
/* PA = LU with partial pivoting; d_perm[n] (int32) as gsl_permutation content. */
int gsl_sinterp_hip_lu_decomp(gsl_sinterp_hip_ctx *ctx, size_t n, double *d_a, size_t lda,
                              int *d_perm, int *h_signum);
int gsl_sinterp_hip_lu_svx(gsl_sinterp_hip_ctx *ctx, size_t n, const double *d_lu, size_t lda,
                           const int *d_perm, double *d_x);
/* ---- solver breadth ---------------------------------- */
/* gsl_linalg_cholesky_decomp2 (linalg/cholesky.c:392-429): S_i = 1/sqrt(A_ii) -> d_s, A <- diag(S) A diag(S),
   then decomp1; svx2 (:431-462): x *= S, two sweeps, x *= S. */
int gsl_sinterp_hip_cholesky_decomp2(gsl_sinterp_hip_ctx *ctx, size_t n, double *d_a, size_t lda, double *d_s,
                                     int *h_info);
int gsl_sinterp_hip_cholesky_svx2(gsl_sinterp_hip_ctx *ctx, size_t n, const double *d_llt, size_t lda,
                                  const double *d_s, double *d_x);
/* gsl_linalg_cholesky_rcond (linalg/cholesky.c:499-537, linalg/condest.c:95-188): reciprocal 1-norm condition
   number of the matrix whose factor (with the original kept in the strict upper triangle) is d_llt. */
int gsl_sinterp_hip_cholesky_rcond(gsl_sinterp_hip_ctx *ctx, size_t n, const double *d_llt, size_t lda,
                                   double *h_rcond);
/* gsl_linalg_LU_refine (linalg/lu.c:204-252): one step of iterative refinement of d_x; d_work: n doubles. */
int gsl_sinterp_hip_lu_refine(gsl_sinterp_hip_ctx *ctx, size_t n, const double *d_a, size_t lda, const double *d_lu,
                              size_t ldlu, const int *d_perm, const double *d_b, double *d_x, double *d_work);
/* gsl_linalg_pcholesky_decomp / _svx (linalg/pcholesky.c:71-229): P A P^T = L D L^T with diagonal pivoting, for
   symmetric positive SEMI-definite matrices; L below the diagonal, D on it, the original in the strict upper
   triangle; d_perm[n] (int32) as gsl_permutation content.  Bit-identical to the reference-order CPU algorithm. */
int gsl_sinterp_hip_pcholesky_decomp(gsl_sinterp_hip_ctx *ctx, size_t n, double *d_a, size_t lda, int *d_perm);
int gsl_sinterp_hip_pcholesky_svx(gsl_sinterp_hip_ctx *ctx, size_t n, const double *d_ldlt, size_t lda,
                                  const int *d_perm, double *d_x);
/* gsl_linalg_pcholesky_decomp2 / _svx2 (linalg/pcholesky.c:231-353): the matrix is kept UNSCALED in the strict upper
   triangle, S_i = 1/sqrt(A_ii) -> d_s, pivoted LDL^T of diag(S) A diag(S); svx2: x *= S, svx, x *= S.
   gsl_linalg_pcholesky_rcond (:472-580): reciprocal 1-norm condition number of the matrix in the upper triangle (its
   diagonal rebuilt from L D L^T), for the UNSCALED decomposition like the reference's own test (test_cholesky.c:675-687). */
int gsl_sinterp_hip_pcholesky_decomp2(gsl_sinterp_hip_ctx *ctx, size_t n, double *d_a, size_t lda, int *d_perm, double *d_s);
int gsl_sinterp_hip_pcholesky_svx2(gsl_sinterp_hip_ctx *ctx, size_t n, const double *d_ldlt, size_t lda, const int *d_perm,
                                   const double *d_s, double *d_x);
int gsl_sinterp_hip_pcholesky_rcond(gsl_sinterp_hip_ctx *ctx, size_t n, const double *d_ldlt, size_t lda, const int *d_perm,
                                    double *h_rcond);

int gsl_sinterp_hip_rbf_eval(gsl_sinterp_hip_ctx *ctx, int kind, double eps, const double *d_x,
                             size_t n, int dim, size_t xtda, const double *d_w,
                             const double *d_y, size_t m, size_t ytda, double *d_s);

/* The same sweep for a model the caller promises not to change while it uses `model_id` (!= 0; a fresh id after
   every init): the Gaussian / Wendland sweep's per-model preprocessing -- Morton cell sort of the centres, packed
   {x, w} records, tile boxes -- is then done once per (model_id, d_x, d_w, n, dim, kind) and reused by later calls
   on this context (the single-point call behind gsl_sinterp_eval_e pays 1 launch instead of 9).  model_id = 0 is
   gsl_sinterp_hip_rbf_eval: nothing is assumed about the buffers, nothing cached.  Same bits either way.
   CONTRACT: the id vouches for the CONTENT of d_x / d_w, not just their addresses -- whoever rewrites either buffer (a
   new init into the same allocation, a checkpoint load, a broadcast) must pass a fresh id afterwards; reusing an id
   across re-filled buffers evaluates the OLD centres / weights silently.  The facade draws a new id in every init and
   fread (csrc/host/sinterp.c: next_model_id); ids are compared per context, so two contexts may use the same values. */
int gsl_sinterp_hip_rbf_eval_model(gsl_sinterp_hip_ctx *ctx, int kind, double eps, const double *d_x,
                                   size_t n, int dim, size_t xtda, const double *d_w,
                                   const double *d_y, size_t m, size_t ytda, double *d_s, unsigned long long model_id);

/* Value and gradient from one fused sweep:  d_s[k] = s(y_k)  and  d_g[k * gtda + a] = ds/dy_a (y_k), a < dim, with
       grad s(y) = sum_j w_j psi(r_j^2) (y - x_j),   psi = phi'(r) / r
   (Gaussian -2 eps^2 phi; Wendland -20 eps^2 (1 - eps r)_+^3; thin-plate ln r^2 + 1; Matern 3/2 -3 eps^2 exp(-t);
   Matern 5/2 -(5 eps^2 / 3) (1 + t) exp(-t); inverse multiquadric -eps^2 phi^3 -- none divides by r, none is singular
   at r = 0).  d_s may be NULL (gradient only); nothing beyond the dim columns of a row of d_g is written.  h_tail: NULL,
   or dim + 1 host doubles {c_0, c_1 .. c_dim} of an affine tail, s += c_0 + sum_a c_a y_a and g_a += c_a (the affine
   thin-plate polynomial; kriging passes {mu, 0, ..}); only h_tail[0 .. dim] is read.
   The value has the bits of gsl_sinterp_hip_rbf_eval_model (_eval_affine / krige_eval with the tail) for the same model
   and target: same terms, same order, and a target takes a gradient term exactly when it takes the value term, so value
   and gradient are functions of (model, target) alone whatever the batch.  A NaN coordinate gives NaN in the value and
   in every gradient component for every kind -- for the thin-plate kinds the value sweep returns that NaN too (r^2 =
   NaN reaches every term), so the two rules do not collide; an infinite coordinate of a Gaussian / Wendland target takes
   no term and gives 0 (Matern / inverse multiquadric: not pinned).  model_id as for _eval_model: the packed centres are shared with the value sweep, a gradient
   call after a value call with the same id reuses them.  Batches of >= 4096 Gaussian / Wendland targets are grouped
   through the one-level permutation for every batch size (GSL_SINTERP_NO_SORT=1 honoured).
   GSL_EINVAL: dim outside 1..3, unknown kind, xtda / ytda / gtda < dim; GSL_EFAULT: a NULL d_y or d_g with m > 0;
   m = 0 succeeds and touches nothing. */
int gsl_sinterp_hip_rbf_eval_grad(gsl_sinterp_hip_ctx *ctx, int kind, double eps, const double *h_tail,
                                  const double *d_x, size_t n, int dim, size_t xtda, const double *d_w,
                                  const double *d_y, size_t m, size_t ytda,
                                  double *d_s /* may be NULL */, double *d_g, size_t gtda,
                                  unsigned long long model_id);

/* Several fields on one set of centres: K weight vectors, one fused sweep.  The distance, the take test and phi of a
   (target, centre) pair are computed once and serve every field; a further field costs one FMA and one select per pair.
   d_w: column q at d_w + q * ldw (ldw >= n); d_s: target k's field q at d_s[k * stda + q] (stda >= nf, the layout of an
   m x nf gsl_matrix; nothing beyond the nf columns of a row is written).  h_tail: NULL, or nf * (dim + 1) host doubles,
   {c_0 .. c_dim} of field q at h_tail + q * (dim + 1), added as s_q += c_0 + sum_a c_a y_a (the affine thin-plate
   polynomials; kriging passes {mu_q, 0, ..}).  1 <= nf <= GSL_SINTERP_MAX_FIELDS.
   BIT RULE: field q has the bits of gsl_sinterp_hip_rbf_eval_model (_eval_affine / krige_eval with the tail) called with
   d_w = column q for the same centres, target and kind: the same terms in the same order (input order below N = 1024 and
   for the thin-plate, Matern and inverse multiquadric kinds, Morton order above), the same take criterion, the same choice of kernel by N.  A target with
   a NaN coordinate gives NaN in all nf outputs (every kind but thin-plate: restored at the store; thin-plate: through
   every term).  The fields are swept in passes of gsl_sinterp_hip_rbf_fields_block() fields (see there).  Batches of
   >= 4096 Gaussian / Wendland targets are grouped through the one-level permutation, as for _eval_grad.  model_id as
   for _eval_model; the packed {x, w_0 .. w_{nf-1}} records of the culled sweep are cached in a slot of their own (keyed by
   nf and ldw too), so scalar and fields calls on one model id do not evict each other.
   GSL_EINVAL: dim outside 1..3, unknown kind, xtda / ytda < dim, ldw < n, stda < nf, nf outside 1..64; GSL_EFAULT: a NULL
   pointer with work to do; m = 0 succeeds and touches nothing. */
#define GSL_SINTERP_MAX_FIELDS 64
int gsl_sinterp_hip_rbf_eval_fields(gsl_sinterp_hip_ctx *ctx, int kind, double eps, const double *h_tail,
                                    const double *d_x, size_t n, int dim, size_t xtda, const double *d_w, size_t ldw,
                                    size_t nf, const double *d_y, size_t m, size_t ytda, double *d_s, size_t stda,
                                    unsigned long long model_id);
/* the two compile-time field blocks of the sweep: passes of _block() fields while more than _block_small() are left, the
   last <= _block_small() fields in a pass of the small instance */
int gsl_sinterp_hip_rbf_fields_block(void);
int gsl_sinterp_hip_rbf_fields_block_small(void);
/* Positive definite kinds (all but thin-plate), nf right-hand sides: ONE fill, ONE Cholesky factorisation, nf solves.  d_w holds F on entry
   (column q = f_q at d_w + q * ldw) and the weights on exit; route 1.  The first min(nf, 5) columns ride the
   factorisation (gsl_sinterp_hip_cholesky_factor_solve), the others are solved against the finished factor five at a
   time; columns of different groups agree to rounding, not bitwise.  A GEMM-based triangular solve for very many fields
   is not provided.  GSL_EINVAL: the thin-plate kind (its shifted-SPD / Woodbury solve is per field), dim, lda / ldw < n,
   nf outside 1..64; GSL_EDOM: not positive definite. */
int gsl_sinterp_hip_rbf_solve_fields(gsl_sinterp_hip_ctx *ctx, int kind, double eps, const double *d_x, size_t n, int dim,
                                     size_t xtda, double *d_phi, size_t lda, double *d_w, size_t ldw, size_t nf, int *h_route);
/* Ordinary kriging of nf fields: nf + 1 right-hand sides (f_0 .. f_{nf-1}, 1) on one factor of K = Phi + nugget I,
   h_mean[nf] receives the means; route 7.  GSL_EDOM when K is not positive definite (nothing is retried here: the caller
   falls back to gsl_sinterp_hip_krige_solve per field, whose route 8 handles a semi-definite K; d_w is then undefined).
   The factor is left in the lower triangle of d_phi as krige_solve leaves it (gsl_sinterp_hip_krige_variance_prepare). */
int gsl_sinterp_hip_krige_solve_fields(gsl_sinterp_hip_ctx *ctx, int kind, double eps, double nugget, const double *d_x,
                                       size_t n, int dim, size_t xtda, double *d_phi, size_t lda, double *d_w, size_t ldw,
                                       size_t nf, double *h_mean, int *h_route);

/* "init" of an RBF interpolant in one call: fill d_phi (n x n scratch, lda), solve Phi w = f
   with d_w holding f on entry and w on exit.  *h_route reports the solver used:
   1 Cholesky (every positive definite kind: Gaussian, Wendland, Matern 3/2 and 5/2, inverse multiquadric) -- 2 shifted-SPD Cholesky + rank-(d+1) Woodbury correction
   (thin-plate spline; values agree with the LU route to ~1e-13) -- 3 pivoted LU (the
   reference's route, taken when the shifted matrix is not SPD or GSL_SINTERP_FORCE_LU=1). */
int gsl_sinterp_hip_rbf_solve(gsl_sinterp_hip_ctx *ctx, int kind, double eps, const double *d_x, size_t n,
                              int dim, size_t xtda, double *d_phi, size_t lda, double *d_w, int *h_route);

/* The same with an explicit solver (GSL_SINTERP_SOLVER_*) and an optional condition estimate:
     DEFAULT    the routes above;
     CHOLESKY2  scaled Cholesky, decomp2 + svx2 (route 4; SPD kernels);
     PCHOLESKY  pivoted LDL^T (route 5; semi-definite / nuggeted kernel matrices);
     LU_REFINE  pivoted LU + one gsl_linalg_LU_refine step (route 6; any kernel; needs a second n x n buffer,
                allocated inside).
   h_rcond (may be NULL): reciprocal condition number of the factored matrix for the Cholesky routes 1 and 4
   (of the SCALED matrix for 4), NaN for the others. */
#define GSL_SINTERP_SOLVER_DEFAULT 0
#define GSL_SINTERP_SOLVER_CHOLESKY2 1
#define GSL_SINTERP_SOLVER_PCHOLESKY 2
#define GSL_SINTERP_SOLVER_LU_REFINE 3
int gsl_sinterp_hip_rbf_solve_ex(gsl_sinterp_hip_ctx *ctx, int kind, double eps, const double *d_x, size_t n, int dim,
                                 size_t xtda, double *d_phi, size_t lda, double *d_w, int solver, double *h_rcond,
                                 int *h_route);

/* Thin-plate spline WITH its affine tail (the "N + d + 1" system):
       [Phi P; P^T 0] [w; c] = [f; 0],  P = [1, x],     s(y) = sum_j w_j phi(|y - x_j|) + c_0 + sum_a c_a y_a.
   d_w holds f on entry and w on exit, h_poly[0 .. dim] receives c (raw coordinates); h_poly needs dim + 1 doubles, and
   nothing past h_poly[dim] is read or written (by _eval_affine either).  Route 9: block elimination on the
   shifted SPD matrix of route 2 (one MFMA Cholesky, d + 2 right-hand sides, a (d+1) x (d+1) system on the host);
   route 10: pivoted LU of the augmented matrix (the reference route, linalg/lu.c:59-201; taken when the shifted
   matrix is not SPD or GSL_SINTERP_FORCE_LU=1) -- it needs d_phi with n + dim + 1 rows and lda >= n + dim + 1.
   kind must be GSL_SINTERP_RBF_TPS.  gsl_sinterp_hip_rbf_eval_affine = the RBF sweep + the polynomial. */
int gsl_sinterp_hip_rbf_solve_affine(gsl_sinterp_hip_ctx *ctx, int kind, double eps, const double *d_x, size_t n, int dim,
                                     size_t xtda, double *d_phi, size_t lda, double *d_w, double *h_poly, int *h_route);
int gsl_sinterp_hip_rbf_eval_affine(gsl_sinterp_hip_ctx *ctx, int kind, double eps, const double *h_poly, const double *d_x,
                                    size_t n, int dim, size_t xtda, const double *d_w, const double *d_y, size_t m,
                                    size_t ytda, double *d_s, unsigned long long model_id);

/* Ordinary kriging on a positive definite kernel used as covariance (GAUSSIAN, WENDLAND, MATERN32, MATERN52 or IMQ) with a nugget >= 0 (the
   reference's README:24 future list): d_w holds f on entry and the dual weights w on exit, *h_mean the estimated
   mean mu; s(y) = mu + sum_j w_j phi(|y - x_j|) (gsl_sinterp_hip_krige_eval = the RBF sweep + mu).  Route 7: Cholesky
   of K = Phi + nugget I with two right-hand sides; route 8: pivoted LDL^T when K is only semi-definite. */
int gsl_sinterp_hip_krige_solve(gsl_sinterp_hip_ctx *ctx, int kind, double eps, double nugget, const double *d_x, size_t n,
                                int dim, size_t xtda, double *d_phi, size_t lda, double *d_w, double *h_mean, int *h_route);
int gsl_sinterp_hip_krige_eval(gsl_sinterp_hip_ctx *ctx, int kind, double eps, double mean, const double *d_x, size_t n,
                               int dim, size_t xtda, const double *d_w, const double *d_y, size_t m, size_t ytda,
                               double *d_s, unsigned long long model_id);

/* Kriging variance at the targets from the factor K = Phi + nugget I = L L^T that krige_solve (route 7),
   cholesky_decomp1 or cholesky_factor_solve leave in the lower triangle of their matrix:
       sigma^2(y) = 1 - |L^-1 k(y)|^2 + (1 - b^T k(y))^2 / (1^T b),    k(y)_j = phi(|y - x_j|),  b = K^-1 1
   -- the variance of the underlying field (the nugget is measurement noise; sill phi(0) = 1): zero at the data sites
   when nugget = 0, 1 + 1/(1^T b) far from every site.  Cost: the N^2 doubles of the factor stay resident, M N^2 flops
   (fp64 MFMA GEMM) for M targets.  Only the lower triangle of d_llt, diagonal included, is read. */
/* from a factor left by cholesky_decomp1 / factor_solve (lower triangle = L): b = K^-1 1 -> d_b[n], the inverted
   32x32 diagonal blocks -> d_dinv[ceil(n/32) * 1024], *h_denom = 1^T b.  Synchronises.  GSL_EDOM when denom is 0 or NaN. */
int gsl_sinterp_hip_krige_variance_prepare(gsl_sinterp_hip_ctx *ctx, size_t n, const double *d_llt, size_t lda,
                                           double *d_b, double *d_dinv, double *h_denom);
/* doubles of workspace for `chunk` targets per pass */
size_t gsl_sinterp_hip_krige_variance_work(size_t n, size_t chunk);
/* d_var[k] = sigma^2(y_k), k < m; asynchronous on the context's stream; chunk >= 1 rows of d_work per pass.  d_work is
   the caller's (gsl_sinterp_hip_krige_variance_work doubles): the sweep and the GEMM called inside use the context's own
   buffers.  kind: any positive definite one (not TPS).  Not clamped: where sigma^2 = 0 the result is rounding residue of either sign. */
int gsl_sinterp_hip_krige_variance(gsl_sinterp_hip_ctx *ctx, int kind, double eps, const double *d_x, size_t n, int dim, size_t xtda,
                                   const double *d_llt, size_t lda, const double *d_b, const double *d_dinv,
                                   double denom, const double *d_y, size_t m, size_t ytda, double *d_var,
                                   double *d_work, size_t chunk);
/* d_v[k] < 0 -> 0 for k < m (NaN stays NaN); asynchronous.  The facade's variance entries apply it. */
int gsl_sinterp_hip_krige_variance_clamp(gsl_sinterp_hip_ctx *ctx, double *d_v, size_t m);

/* Local ordinary kriging (a moving neighbourhood): every target is kriged on its k <= 64 nearest centres alone -- memory
   O(N + M k), work O(M k^3), no N x N matrix, so N may be far past what a dense factorisation holds.
   NEIGHBOUR SET: with r2_j = the FMA chain of the sweeps (r2 = 0; d = y_c - x_jc; r2 = fma(d, d, r2), c < dim), S(y) is the k
   centres smallest under the key (r2_j, j), in ascending key order.  The search is exact (grid cells in growing rings
   until a lower bound on every unvisited cell exceeds the k-th key), not approximate and not limited to a ring count.  A
   target with a NaN coordinate has no neighbours: indices -1, r2 / value / variance NaN, and it is not a failure.
   Infinite coordinates are not specified.
   gsl_sinterp_hip_knn: d_idx[t * k + i] = the i-th neighbour of target t (original row of d_x), d_r2 (optional) its r2.
   gsl_sinterp_hip_local_krige: with K_S = [phi(|x_i - x_j|)] + nugget I = L L^T on S in that order, u = L^-1 k_S,
   v = L^-1 1, g = L^-1 f_S:   d = v.v,  mu = v.g / d,  s = mu + u.(g - mu v),  sigma^2 = phi(0) - u.u + (1 - v.u)^2 / d.
   Each of d_s, d_var, d_idx may be NULL.  sigma^2 is NOT clamped (gsl_sinterp_hip_krige_variance_clamp).  The result of a
   target depends on (model, target, k) alone: the same bits from run to run, alone or in a batch of any size, on any
   context.  FAILED PIVOTS: a target whose K_S has a pivot that is not > 0 (not above 64 u (phi(0) + nugget): the rounding
   residue of an exactly singular system has either sign) or not finite gets value and variance NaN; every other target is
   stored as usual, *h_n_failed (optional) receives the count and the return is GSL_EDOM.  local_krige synchronises (the
   count is its status); knn is asynchronous on the context's stream.
   The centres are binned once per model into a cell-ordered copy kept in the context, keyed by model_id as in
   gsl_sinterp_hip_rbf_eval_model (0 = do not cache); gsl_sinterp_hip_local_pack_count counts the packs of a context.
   GSL_EINVAL: k < 1, k > 64, k > n, dim outside 1 .. 3, xtda / ytda < dim, a kind that is not positive definite, nugget < 0
   or not finite, eps <= 0 or not finite -- all checked first; then GSL_EFAULT: a NULL context or a NULL required pointer
   (d_x, d_f; d_y and, for knn, d_idx when m > 0).  Nothing touches the device before these checks. */
int gsl_sinterp_hip_knn(gsl_sinterp_hip_ctx *ctx, const double *d_x, size_t n, int dim, size_t xtda, const double *d_y, size_t m,
                        size_t ytda, size_t k, int *d_idx /* m x k, ascending key, -1 = none */, double *d_r2 /* m x k or NULL */,
                        unsigned long long model_id);
int gsl_sinterp_hip_local_krige(gsl_sinterp_hip_ctx *ctx, int kind, double eps, double nugget, const double *d_x, size_t n, int dim,
                                size_t xtda, const double *d_f, const double *d_y, size_t m, size_t ytda, size_t k,
                                double *d_s /* or NULL */, double *d_var /* or NULL */, int *d_idx /* or NULL */,
                                size_t *h_n_failed /* or NULL */, unsigned long long model_id);
/* bin the centres now (what the first knn / local_krige call on a model does anyway); asynchronous.  The copy is keyed by
   d_f too: pass the responses local_krige will be called with (knn packs with NULL).  Same checks as above. */
int gsl_sinterp_hip_local_pack(gsl_sinterp_hip_ctx *ctx, const double *d_x, size_t n, int dim, size_t xtda, const double *d_f,
                               unsigned long long model_id);
unsigned long long gsl_sinterp_hip_local_pack_count(const gsl_sinterp_hip_ctx *ctx);

/* Empirical semivariogram: the binned sums over the unordered pairs i < j of sites closer than h_max -- memory
   O(N + cells + bins), work proportional to the pairs inside the pruning stencil, no N x N matrix, so it runs on the whole
   cloud that local kriging takes (DESIGN_VARIOGRAM.md).
   BIN RULE, on r2 so that a host reference reproduces it to the bit: r2 = ((dx*dx) + (dy*dy)) + (dz*dz) left to right over the
   axes present, no contraction; edge2[b] = e*e with e = b * (h_max / n_bins), edge2[n_bins] = h_max*h_max; a pair with
   r2 < edge2[n_bins] goes into the bin b with edge2[b] <= r2 < edge2[b + 1]; coincident sites (r2 = 0) fall into bin 0.
   acc (HOST, n_bins x 7 words), per bin b at acc[7 b + ..]:
     0      the pair count;
     1, 2   lo, hi of sum (f_i - f_j)^2;
     3, 4   lo, hi of sum h, h = sqrt(r2);
     5, 6   lo, hi of sum sqrt|f_i - f_j| (Cressie-Hawkins).
   The three sums are 128-bit fixed-point integers: a term t enters as q = (unsigned long long) rint(ldexp(t, shift[k])),
   shift[k] = 62 - E_k with E_k the frexp exponent of an upper bound of the terms -- (fmax - fmin)^2, h_max and
   sqrt(fmax - fmin), the range of f taken by a reduction pass; fmax = fmin gives shift[0] = shift[2] = 0 and terms 0.
   sum = (hi 2^64 + lo) 2^-shift[k].  Only integer additions are made, so the 7 words of a bin are the same for every row
   order of x, every grid, every launch shape and every run; the count and the words 1, 2 are a pure function of the input
   under IEEE arithmetic, the words 3 .. 6 contain one device sqrt per term.  A term with q = 0 still counts as a pair.
   n < 2: every word 0, shift = {0, shift of h_max, 0}, success, nothing touches the device (the input is not inspected).
   GSL_EINVAL: dim outside 1 .. 3, n_bins outside 1 .. 256, h_max not finite or <= 0, xtda < dim, n > 2^31 - 1 -- all checked
   first; then GSL_EFAULT: a NULL context, acc, shift or (n > 0) d_x, d_f.  GSL_EDOM, acc zeroed, before any pair is visited:
   a NaN or infinite entry in the dim leading columns of x or in f, or a range of f whose square overflows.  Synchronises.
   The sites are binned into the buffer of the local route: a pack cached by gsl_sinterp_hip_local_pack is dropped.
   gsl_sinterp_hip_variogram_pairs_tested: the unordered pairs whose r2 the last call on the context computed.
   gsl_sinterp_hip_bbox: box[2 c] = min, box[2 c + 1] = max of coordinate c < dim over the n >= 1 rows (NaN skipped; HOST,
   2 dim doubles); synchronises.  Same checks; n = 0 is GSL_EINVAL. */
int gsl_sinterp_hip_variogram(gsl_sinterp_hip_ctx *ctx, const double *d_x, size_t n, int dim, size_t xtda, const double *d_f,
                              double h_max, int n_bins, unsigned long long *acc /* HOST, n_bins x 7 */, int shift[3] /* HOST */);
unsigned long long gsl_sinterp_hip_variogram_pairs_tested(const gsl_sinterp_hip_ctx *ctx);
int gsl_sinterp_hip_bbox(gsl_sinterp_hip_ctx *ctx, const double *d_x, size_t n, int dim, size_t xtda, double *box /* HOST, 2 dim */);

/* Modified quadratic Shepard interpolation (Renka, ACM TOMS 660 / 661; Franke & Nielson 1980) in dim 2 or 3: C1, exact at the
   data, reproduces quadratics, local, O(N) memory, no solve, no mesh, no shape parameter, analytic gradient.
   With r2 the FMA chain of the sweeps, r = sqrt(r2), and integer parameters nq, nw:
     Rq_i, Rw_i   the distance from x_i to its (nq + 1)-th, (nw + 1)-th nearest OTHER site.  Only sites STRICTLY inside a radius
                  carry weight (a site on it has weight 0, so no result depends on how the search breaks a distance tie; on a
                  lattice fewer than nq sites may then take part).
     Q_i(y)       = f_i + c_i . m((y - x_i) / Rq_i), m(u) = the dim linear monomials u_0 .. u_{dim-1}, then u_a u_b for a <= b
                  in row-major order: nc = 5 (dim 2) or 9 (dim 3) coefficients per node.
     c_i          minimises sum_j omega_ij^2 (Q_i(x_j) - f_j)^2 over j != i with r_ij < Rq_i, omega_ij = (Rq_i - r_ij) / (Rq_i r_ij):
                  Householder QR of the weighted matrix, its columns scaled to unit 2-norm first (a zero column is deficient),
                  in that column order without pivoting, no normal equations.  RANK RULE, rho(k) = min |R_jj| / max |R_jj| over
                  j < k: rho(nc) >= GSL_SQRT_DBL_EPSILON: the quadratic fit; otherwise rho(dim) >= GSL_SQRT_DBL_EPSILON: the linear
                  fit on the first dim columns, quadratic coefficients 0; otherwise c_i = 0.
     W_i(y)       = ((Rw_i - r_i)_+ / (Rw_i r_i))^2,  s(y) = sum W_i Q_i / sum W_i,
                  grad s = sum (W_i grad Q_i + (Q_i - s) grad W_i) / sum W_i in raw coordinates.
   gsl_sinterp_hip_shepard_fit: d_rq[n], d_rw[n], d_coef[n x nc] from the sites d_x (n x dim, pitch xtda) and responses d_f.
   The neighbours come from gsl_sinterp_hip_knn with the sites as targets and k = max(nq, nw) + 2 (neighbour 0 is the node
   itself, hence nq, nw <= 62), in chunks of nodes so that the index buffers stay bounded; then one wave per node, every
   sum a fixed 64-lane butterfly: the same bits from run to run.  h_counts (3 entries, or NULL): nodes that took the linear
   fallback, the constant fallback, and nodes whose nearest other site is at r2 = 0 -- their weights are undefined, their
   outputs NaN and the return is GSL_EDOM.  Synchronises.  GSL_EINVAL: dim not 2 or 3, nq < nc, nw < 1, max(nq, nw) + 2 > 64
   or > n, xtda < dim -- checked first; then GSL_EFAULT: a NULL context or pointer.  Nothing touches the device before.
   gsl_sinterp_hip_shepard_eval: d_s[m] (or NULL), the gradient (row k at d_g + k * gtda, or NULL) and d_leaf[m] (or NULL)
   at the targets d_y (m x dim, pitch ytda).  d_leaf = the number of nodes with W_i > 0 (not bounded by 64).  SPECIAL TARGETS:
   r2 = 0 to a node: the f of the smallest such row, that node's gradient c_lin / Rq, leaf 1; sum W not finite (within
   ~1e-154 of a node): the same from the nearest node under the key (r2, row); no node with W > 0: NaN, NaN, -1; a NaN
   coordinate: NaN, NaN, -1 and no error.  h_n_outside != NULL: the call synchronises, stores the number of uncovered targets
   and returns GSL_EDOM when it is not 0 (every other target has been stored); NULL: asynchronous, no such status.
   A target's result depends on (model, target) alone: the same bits from run to run, alone or in a batch of any size
   (batches of 4096 and more run in cell order), with or without the gradient.  The nodes are packed once per model into
   cell-ordered records kept in the context, keyed by model_id as in gsl_sinterp_hip_rbf_eval_model (0 = do not cache);
   the _pack_count / _fit_count entries count the packs and fits of a context.  GSL_EINVAL: dim, xtda / ytda / gtda < dim;
   then GSL_EFAULT: a NULL context or model pointer, d_y with m > 0. */
int gsl_sinterp_hip_shepard_fit(gsl_sinterp_hip_ctx *ctx, const double *d_x, size_t n, int dim, size_t xtda, const double *d_f,
                                size_t nq, size_t nw, double *d_rq, double *d_rw, double *d_coef /* n x nc */,
                                size_t *h_counts /* linear fallbacks, constant fallbacks, coincident nodes; or NULL */);
int gsl_sinterp_hip_shepard_eval(gsl_sinterp_hip_ctx *ctx, const double *d_x, size_t n, int dim, size_t xtda, const double *d_f,
                                 const double *d_rq, const double *d_rw, const double *d_coef, const double *d_y, size_t m,
                                 size_t ytda, double *d_s /* or NULL */, double *d_g /* or NULL */, size_t gtda, int *d_leaf /* or NULL */,
                                 size_t *h_n_outside /* or NULL */, unsigned long long model_id);
unsigned long long gsl_sinterp_hip_shepard_pack_count(const gsl_sinterp_hip_ctx *ctx);
unsigned long long gsl_sinterp_hip_shepard_fit_count(const gsl_sinterp_hip_ctx *ctx);

/* Leave-one-out from a Cholesky factor K = L L^T (lower triangle of d_llt, as cholesky_decomp1, factor_solve, rbf_solve
   route 1 and krige_solve route 7 leave it): d_g[i] = (K^-1)_ii = |row i of L^-T|^2, i < n, in N^3 / 3 + O(chunk N^2)
   flops (fp64 MFMA GEMM) -- the recursion of the variance entry started from the identity, with the rows taken `chunk`
   at a time (rounded up to 128, at most n rounded up to 128) and the zero part of the triangle skipped.  Only the lower
   triangle of d_llt, diagonal included, is read; nothing is written outside d_g and d_work
   (gsl_sinterp_hip_chol_inv_diag_work doubles, which also hold the inverted 32 x 32 diagonal blocks formed here).
   Asynchronous on the context's stream.  g is the same bit for bit from run to run at a fixed chunk; different chunks
   agree to rounding only (their updates differ in K range and height, and the stream-K GEMM splits K by the tile count).
   GSL_EINVAL: lda < n or chunk == 0; GSL_EFAULT: a NULL pointer with n > 0; n == 0 succeeds and launches nothing. */
size_t gsl_sinterp_hip_chol_inv_diag_work(size_t n, size_t chunk);
int gsl_sinterp_hip_chol_inv_diag(gsl_sinterp_hip_ctx *ctx, size_t n, const double *d_llt, size_t lda, double *d_g,
                                  double *d_work, size_t chunk);
/* Leave-one-out residuals of nf weight vectors (column q at d_w + q * ldw) and the leave-one-out variance:
       diag_i = g_i (d_b == NULL: plain SPD interpolant, Rippa) or g_i - b_i^2 / denom (ordinary kriging, Dubrule; b = K^-1 1,
       denom = 1^T b as gsl_sinterp_hip_krige_variance_prepare returns them),
       d_e[q * lde + i] = d_w[q * ldw + i] / diag_i,   d_v[i] = 1 / diag_i.
   Not clamped: a diag_i that rounding made non-positive or non-finite is used as computed.  nf = 0 computes d_v only.
   GSL_EINVAL: nf > 64, ldw or lde < n with nf > 0; GSL_EFAULT: a NULL pointer (other than d_b) with work to do. */
int gsl_sinterp_hip_loo_combine(gsl_sinterp_hip_ctx *ctx, size_t n, size_t nf, const double *d_g, const double *d_b,
                                double denom, const double *d_w, size_t ldw, double *d_e, size_t lde, double *d_v);

/* ---- universal kriging: a polynomial drift (csrc/hip/drift.hip; DESIGN.md 4, "Universal kriging") ---- */
/* The model: s(y) = p(u(y))^T c + sum_j w_j phi(|y - x_j|),  [K P; P^T 0] [w; c] = [f; 0],  K = Phi + nugget I.
   The basis is taken in STANDARDISED coordinates u_a = (y_a - h_shift[a]) * h_scale[a] (the facade passes the centre of
   the sites' bounding box and 1 / half-extent per axis, 1 for a zero extent; monomials in raw coordinates of UTM size
   would cost every digit).  order 1: q = dim + 1 terms {1, u_1 .. u_d}; order 2: q = (dim + 1)(dim + 2) / 2, the products
   u_a u_b, a <= b, in lexicographic order behind them.  q <= GSL_SINTERP_DRIFT_MAX_TERMS.  h_shift / h_scale: dim host
   doubles.  Every entry below takes order 1 or 2 (GSL_EINVAL otherwise: order 0 is ordinary kriging, whose entries stay
   as they are) and checks its arguments before anything touches the device.
     drift_terms    q for (dim, order), order 0 included (1); 0 for arguments out of range.
     drift_factor   host only: S = Ls Ls^T of the q x q row-major h_S into the lower triangle of h_L (row-major, upper part
                    zeroed).  GSL_EDOM when a pivot is not above 64 DBL_EPSILON times that diagonal entry of S before
                    elimination, or not finite: the drift functions are linearly dependent on the sites.
     drift_basis    column t of P at d_P + t * ldp (ldp >= n), row i = term t at site i.
     ukrige_solve   route 12.  d_w holds F on entry (column f at d_w + f * ldw) and the weights on exit; ONE fill and ONE
                    factorisation carry the nf + q right-hand sides [F | P] (A = K^-1 F, B = K^-1 P), S = P^T B and
                    T = P^T A are reduced on the device in a fixed order (same bits every run), S c = T is solved on the
                    host through drift_factor, w = A - B c.  h_coef receives nf * q coefficients, field f at h_coef + f * q;
                    d_B (or NULL) receives B, column t at d_B + t * ldb; h_S (or NULL) the q * q entries of S; h_L (or NULL)
                    its factor as drift_factor returns it; d_dinv (or NULL; ceil(n / 32) * 1024 doubles) the inverted 32 x 32
                    diagonal blocks of L that ukrige_variance takes (what krige_variance_prepare returns).  The factor
                    is left in the lower triangle of d_phi as krige_solve leaves it.  GSL_EDOM: K is not positive definite
                    (there is NO pivoted route-8 fall-back with a drift) or S is not (drift_factor); GSL_EINVAL: 0 < n < q,
                    a kind that is not positive definite, nf outside 1..64, a pitch below n.  Synchronises.
     drift_add      the tail after a plain sweep: d_s[k * stda + f] += p(u(y_k))^T c_f and (d_g) d_g[k * gtda + f * dim + a]
                    += d/dy_a of it in raw coordinates, f < nf; either of d_s / d_g may be NULL.  h_coef as ukrige_solve
                    returns it; coefficients and geometry reach the kernel by value (8 fields per launch), so any context
                    may call.  The value bits of a target are those of the plain sweep plus ONE addition of p^T c, formed
                    in one fixed order: the same alone, in any batch, with or without gradients, for any nf.
     ukrige_variance  sigma^2(y) = 1 - |L^-1 k|^2 + r^T S^-1 r, r = p(u(y)) - B^T k(y): the recursion of krige_variance for
                    the second term, the fields sweep with the q columns of B as weights for B^T k (per pass of `chunk`
                    targets), then the combine.  d_dinv as ukrige_solve or krige_variance_prepare return it, h_L from
                    ukrige_solve or drift_factor.  The recursion always takes the default panel of 128 columns: the
                    developer switch GSL_SINTERP_KRIGE_PANEL belongs to krige_variance and its timing tool;
                    d_work: ukrige_variance_work(n, chunk, q) doubles.  Not clamped.
     loo_combine_drift  Dubrule's rule with a drift: diag_i = g_i - B_i S^-1 B_i^T (S^-1 through h_L), d_e[f * lde + i] =
                    d_w[f * ldw + i] / diag_i, d_v[i] = 1 / diag_i; g from gsl_sinterp_hip_chol_inv_diag.  q must be a
                    value drift_terms returns for order 1 or 2. */
/*   local_ukrige   gsl_sinterp_hip_local_krige with a LINEAR drift: the same arguments, search, statuses and bit contract (a
                    target's result does not depend on the batch).  Local basis u = (x_i - y) / h, h the distance of the
                    k-th neighbour, so p = e_0 at the target; with V = L^-1 [1 | u], g = L^-1 f_S, u = L^-1 k_S:
                    S = V^T V, c = S^-1 V^T g, s = c_0 + u^T (g - V c), sigma^2 = phi(0) - u^T u + r^T S^-1 r, r = e_0 - V^T u.
                    NaN in value and variance, counted in *h_n_failed, GSL_EDOM after every other target has been stored: a
                    failed pivot of K_S, a pivot of S not above 64 DBL_EPSILON times that diagonal entry before elimination
                    or not finite (a collinear / coplanar neighbourhood), h = 0.  GSL_EINVAL: k < dim + 2, and what
                    local_krige refuses. */
#define GSL_SINTERP_DRIFT_MAX_TERMS 10
int gsl_sinterp_hip_local_ukrige(gsl_sinterp_hip_ctx *ctx, int kind, double eps, double nugget, const double *d_x, size_t n, int dim,
                                 size_t xtda, const double *d_f, const double *d_y, size_t m, size_t ytda, size_t k, double *d_s,
                                 double *d_var, int *d_idx, size_t *h_n_failed, unsigned long long model_id);
size_t gsl_sinterp_hip_drift_terms(int dim, int order);
int gsl_sinterp_hip_drift_factor(size_t q, const double *h_S, double *h_L);
int gsl_sinterp_hip_drift_basis(gsl_sinterp_hip_ctx *ctx, int order, const double *h_shift, const double *h_scale,
                                const double *d_x, size_t n, int dim, size_t xtda, double *d_P, size_t ldp);
int gsl_sinterp_hip_ukrige_solve(gsl_sinterp_hip_ctx *ctx, int kind, double eps, double nugget, int order,
                                 const double *h_shift, const double *h_scale, const double *d_x, size_t n, int dim,
                                 size_t xtda, double *d_phi, size_t lda, double *d_w, size_t ldw, size_t nf,
                                 double *h_coef, double *d_B, size_t ldb, double *h_S, double *h_L, double *d_dinv,
                                 int *h_route);
int gsl_sinterp_hip_drift_add(gsl_sinterp_hip_ctx *ctx, int order, const double *h_shift, const double *h_scale,
                              const double *h_coef, size_t nf, const double *d_y, size_t m, int dim, size_t ytda,
                              double *d_s, size_t stda, double *d_g, size_t gtda);
size_t gsl_sinterp_hip_ukrige_variance_work(size_t n, size_t chunk, size_t q);
int gsl_sinterp_hip_ukrige_variance(gsl_sinterp_hip_ctx *ctx, int kind, double eps, int order, const double *h_shift,
                                    const double *h_scale, const double *d_x, size_t n, int dim, size_t xtda,
                                    const double *d_llt, size_t lda, const double *d_B, size_t ldb, const double *d_dinv,
                                    const double *h_L, const double *d_y, size_t m, size_t ytda, double *d_var,
                                    double *d_work, size_t chunk);
int gsl_sinterp_hip_loo_combine_drift(gsl_sinterp_hip_ctx *ctx, size_t n, size_t nf, const double *d_g, const double *d_B,
                                      size_t ldb, size_t q, const double *h_L, const double *d_w, size_t ldw, double *d_e,
                                      size_t lde, double *d_v);

/* ---- joint posterior covariance and conditional simulation (csrc/hip/krige_cov.hip) ---- */
/* For target sets Ya (ma rows) and Yb (mb rows), sill 1, the nugget measurement noise as in krige_variance:
       d_cov[i * ctda + j] = C(|ya_i - yb_j|) - z_i . z_j + t_i . t_j,   z = L^-1 k(y),   t = Ls^-1 (p(u(y)) - B^T k(y)),
   B = K^-1 P, S = P^T B = Ls Ls^T.  C carries no nugget, also for coincident targets (C = 1).  ONE body serves every order:
   order 1 or 2 takes d_B (column t at d_B + t * ldb), h_L, h_shift and h_scale as ukrige_variance does; order 0 is ordinary
   kriging, q = 1: d_B = b = K^-1 1 and h_L = {sqrt(1^T b)} (krige_variance_prepare), h_shift / h_scale not read (NULL).
   d_yb == NULL: Yb = Ya (mb and ybtda are not read): only the tiles on and below the diagonal are computed, the strict
   lower triangle is then copied to the upper one, so the result is symmetric to the bit.  Nothing is clamped: the diagonal
   is the kriging variance BEFORE the clamp, rounding residue of either sign where sigma^2 = 0.  Nothing outside the
   ma x mb window of d_cov is written (ctda >= mb).  A target with a NaN coordinate gives NaN in its row and column.
   All of Z_a, and of Z_b, is held at once in d_work (krige_covariance_work(n, ma, mb, q) doubles, mb = 0 for one set;
   q = drift_terms(dim, order)): rows padded to 128, pitch n rounded up to 128, Z_b stacked under Z_a so that one
   substitution pass serves both.  Asynchronous on the context's stream; every buffer is the caller's.
   GSL_EINVAL: dim, a pitch below its width, n = 0, a kind that is not positive definite, order outside 0..2; GSL_EFAULT: a
   NULL pointer with work to do; ma = 0 or mb = 0 succeeds and touches nothing. */
size_t gsl_sinterp_hip_krige_covariance_work(size_t n, size_t ma, size_t mb, size_t q);
int gsl_sinterp_hip_krige_covariance(gsl_sinterp_hip_ctx *ctx, int kind, double eps, int order, const double *h_shift,
                                     const double *h_scale, const double *d_x, size_t n, int dim, size_t xtda,
                                     const double *d_llt, size_t lda, const double *d_B, size_t ldb, const double *d_dinv,
                                     const double *h_L, const double *d_ya, size_t ma, size_t yatda, const double *d_yb,
                                     size_t mb, size_t ybtda, double *d_cov, size_t ctda, double *d_work);
/* Conditional simulation at the m rows of d_y, on top of the two entries above:
       d_out[i * otda + s] = d_mean[i] + sqrt(sigma2) (A Zn)[i][s],     A A^T = Sigma_YY + jitter I,   s < n_draws,
   A the lower Cholesky factor in target order (gsl_sinterp_hip_cholesky_decomp1 on an m x m work matrix), d_zn the caller's
   standard normals (m x n_draws, pitch ztda; no random numbers are drawn here), d_mean the predictor at the targets
   (krige_eval, or rbf_eval_model + drift_add).  A column of zeros returns the bits of d_mean; equal columns give equal
   bits; value i depends on the normals 0 .. i only.  d_work: krige_simulate_work(n, m, n_draws, q) doubles.  Waits for the
   pivot status of the factorisation.  GSL_EDOM: Sigma_YY + jitter I is not numerically positive definite (targets on data
   sites of a nugget-free model, repeated targets) -- every entry of d_out is NaN; there is no pivoted fall-back and no
   automatic jitter: pass one such as 1e-10.  GSL_EINVAL: n_draws = 0, ztda or otda < n_draws, sigma2 not finite or <= 0,
   jitter not finite or < 0, and what krige_covariance refuses; m = 0 succeeds and touches nothing. */
size_t gsl_sinterp_hip_krige_simulate_work(size_t n, size_t m, size_t n_draws, size_t q);
int gsl_sinterp_hip_krige_simulate(gsl_sinterp_hip_ctx *ctx, int kind, double eps, int order, const double *h_shift,
                                   const double *h_scale, const double *d_x, size_t n, int dim, size_t xtda,
                                   const double *d_llt, size_t lda, const double *d_B, size_t ldb, const double *d_dinv,
                                   const double *h_L, const double *d_y, size_t m, size_t ytda, const double *d_mean,
                                   double sigma2, double jitter, const double *d_zn, size_t ztda, size_t n_draws,
                                   double *d_out, size_t otda, double *d_work);

/* The scalars of the model-selection criteria (gsl_sinterp_fit_score).
   From a Cholesky factor (lower triangle of d_llt, as routes 1 / 7 leave it), the right-hand side d_f, the solved
   weights d_w and, optionally, g = diag(K^-1) (gsl_sinterp_hip_chol_inv_diag) and kriging's b = K^-1 1, denom = 1^T b:
     d_out[0] = sum_i 2 log L_ii            (log|K|; a sum of logs, never the log of a product)
     d_out[1] = sum_i f_i w_i               (the quadratic form: w = K^-1 f, or K^-1 (f - mu 1) with 1^T w = 0)
     d_out[2] = sum_i (w_i / diag_i)^2      diag_i = g_i, or g_i - b_i^2 / denom when d_b != NULL; 0 when d_g == NULL
     d_out[3] = number of i with L_ii not > 0 or not finite, or (d_g != NULL) diag_i not > 0 or not finite
   One launch, asynchronous on the context's stream.  One workgroup: every thread adds its sites in index order, the 1024
   partial sums are added in a fixed tree; no atomics, so the four numbers are the same bits from run to run.  Nothing is
   clamped: a bad site enters the sums as computed (log of a non-positive pivot is -inf or NaN) and is counted in
   d_out[3], which is always a finite count.  d_b is ignored without d_g.  Only the diagonal of d_llt is read.
   GSL_EINVAL: lda < n; GSL_EFAULT: a NULL context, or a NULL d_llt / d_f / d_w / d_out with n > 0; n == 0 succeeds and
   writes four zeros (to a non-NULL d_out). */
int gsl_sinterp_hip_score_reduce(gsl_sinterp_hip_ctx *ctx, size_t n, const double *d_llt, size_t lda, const double *d_f,
                                 const double *d_w, const double *d_g, const double *d_b, double denom, double *d_out);

/* Level-3 building block of both factorisations, exposed for tests and roofline
   measurement (role of gsl_blas_dgemm / dsyrk, blas/blas.c:1334,1649):
     C[m x n] -= A[m x k] * B^T  (b_is_kn = 0, B stored [n][k])
     C[m x n] -= A[m x k] * B    (b_is_kn = 1, B stored [k][n])
   lower_only != 0: C is square and only its lower triangle is updated. */
int gsl_sinterp_hip_gemm_minus(gsl_sinterp_hip_ctx *ctx, size_t m, size_t n, size_t k, const double *d_a,
                               size_t lda, const double *d_b, size_t ldb, int b_is_kn, double *d_c,
                               size_t ldc, int lower_only);

/* developer / test hook: targets of the last large barycentric batch on this context that the certified leaf walk left to the
   exact DAG kernel (meaningful when *h_leafwalk = 1: tree_pack built the locator data for the records in use) */
int gsl_sinterp_hip_bary_last_queue(gsl_sinterp_hip_ctx *ctx, unsigned *h_queued, int *h_leafwalk);

/* ---- gridded front-end: the targets of an n0 x n1 grid generated in HBM ---- */
/* row (i*n1 + j) of d_y (packed M x 2) = (min0 + step0*i, min1 + step1*j): the loop of
   interpolation/scattered_interp_example.c:183-197, same operations, so the same bits */
int gsl_sinterp_hip_grid_targets(gsl_sinterp_hip_ctx *ctx, double min0, double step0, size_t n0, double min1,
                                 double step1, size_t n1, double *d_y);

/* ---- synthetic clouds generated in HBM (bench / tests) ------- */
int gsl_sinterp_hip_synth_unit(gsl_sinterp_hip_ctx *ctx, uint64_t seed, uint64_t first,
                               double offset, double span, double *d_out, size_t count);

#ifdef __cplusplus
}
#endif
#endif
