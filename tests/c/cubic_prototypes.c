/* References the Clough-Tocher prototypes of include/gsl_sinterp.h and include/gsl_sinterp_hip.h with their declared
   types, and calls the entries that answer without a GPU: simplex_mesh_vertex_adjacency on a small mesh, the facade's
   allocation rules and status answers, and the argument errors of the device entries. */
#include <gsl_sinterp.h>
#include <stdio.h>

static int (*const p_adjacency)(const simplex_mesh *, int *, int *, size_t, size_t *) = &simplex_mesh_vertex_adjacency;
static int (*const p_bind)(simplex_mesh_device *, const gsl_matrix *) = &simplex_mesh_device_bind_gradients;
static int (*const p_options)(simplex_mesh_device *, double, size_t) = &simplex_mesh_device_set_gradient_options;
static int (*const p_gradients)(simplex_mesh_device *, gsl_matrix *, size_t *, double *) = &simplex_mesh_device_gradients;
static int (*const p_many)(simplex_mesh_device *, const gsl_matrix *, gsl_vector *, gsl_matrix *, int *) =
    &simplex_mesh_device_eval_cubic_many;
static int (*const p_resident)(simplex_mesh_device *, const double *, size_t, size_t, double *, double *, size_t, int *) =
    &simplex_mesh_device_eval_cubic_resident;
static int (*const p_solve)(gsl_sinterp_hip_ctx *, int, const int *, const int *, size_t, const double *, const double *, double, int,
                            double *, int *, double *) = &gsl_sinterp_hip_mesh_cubic_gradients;
static int (*const p_pack)(gsl_sinterp_hip_ctx *, int, const int *, const int *, int, const double *, const double *, const double *,
                           void *) = &gsl_sinterp_hip_mesh_cubic_pack;
static int (*const p_eval)(gsl_sinterp_hip_ctx *, int, const void *, const int *, const double *, const double *, size_t, size_t, double *,
                           double *, size_t) = &gsl_sinterp_hip_mesh_cubic_eval;
static int (*const p_set)(gsl_sinterp *, const gsl_matrix *) = &gsl_sinterp_set_gradients;
static int (*const p_set_options)(gsl_sinterp *, double, size_t) = &gsl_sinterp_set_gradient_options;
static int (*const p_get)(const gsl_sinterp *, gsl_matrix *, size_t *, double *) = &gsl_sinterp_get_gradients;
static const gsl_sinterp_type *const *const p_types[2] = {&gsl_sinterp_cubic_mesh, &gsl_sinterp_cubic_simplex};

#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main(void)
{
  gsl_set_error_handler_off();
  /* a kite cut along 0-2, and a fifth point that no triangle uses */
  double xy[10] = {0.0, 0.0, 2.0, -1.5, 3.0, 0.0, 2.0, 1.5, 9.0, 9.0};
  gsl_matrix_view X = gsl_matrix_view_array(xy, 5, 2);
  const int tri[6] = {0, 1, 2, 0, 2, 3};
  simplex_mesh *m = simplex_mesh_import(&X.matrix, tri, NULL, 2);
  CHECK(m != NULL);
  int off[6], adj[12];
  size_t cnt = 0;
  CHECK(p_adjacency(m, off, adj, 12, &cnt) == GSL_SUCCESS && cnt == 10);
  const int want_off[6] = {0, 3, 5, 8, 10, 10}, want_adj[10] = {1, 2, 3, 0, 2, 0, 1, 3, 0, 2};
  for (int i = 0; i < 6; i++) CHECK(off[i] == want_off[i]);
  for (int i = 0; i < 10; i++) CHECK(adj[i] == want_adj[i]);
  cnt = 0;
  CHECK(p_adjacency(m, off, NULL, 0, &cnt) == GSL_SUCCESS && cnt == 10 && off[5] == 10);      /* count only */
  CHECK(p_adjacency(m, off, adj, 9, &cnt) == GSL_EBADLEN && cnt == 10);
  CHECK(p_adjacency(NULL, off, adj, 12, &cnt) == GSL_EFAULT && p_adjacency(m, NULL, adj, 12, &cnt) == GSL_EFAULT);
  simplex_mesh_free(m);
  /* the facade: dim 2 only; what the types refuse */
  double gg[10] = {0}, g3[12] = {0};
  gsl_matrix_view G = gsl_matrix_view_array(gg, 4, 2), G3 = gsl_matrix_view_array(g3, 4, 3), G5 = gsl_matrix_view_array(gg, 5, 2);
  double ff[4] = {0};
  gsl_vector_view F = gsl_vector_view_array(ff, 4);
  gsl_matrix_view X4 = gsl_matrix_view_array(xy, 4, 2);
  for (int i = 0; i < 2; i++) {
    CHECK(gsl_sinterp_alloc(*p_types[i], 3, 8) == NULL && gsl_sinterp_alloc(*p_types[i], 1, 8) == NULL);
    gsl_sinterp *s = gsl_sinterp_alloc(*p_types[i], 2, 4);
    CHECK(s != NULL);
    CHECK(gsl_sinterp_set_neighbours(s, 2) == GSL_EUNSUP);
    CHECK(gsl_sinterp_eval_variance_resident(s, NULL, 0, 2, NULL) == GSL_EUNSUP);
    CHECK(gsl_sinterp_fit_alloc(s, &X4.matrix, &F.vector) == NULL);
    CHECK(gsl_sinterp_init_fields(s, &X4.matrix, &G.matrix) == GSL_EUNSUP);
    CHECK(gsl_sinterp_loo_variance(s, &F.vector) == GSL_EUNSUP);
    CHECK(gsl_sinterp_eval_grad_resident(s, NULL, 0, 2, NULL, NULL, 2) == GSL_EINVAL);         /* supported; not initialised */
    CHECK(gsl_sinterp_set_triangulation(s, tri, NULL, 2) == (i == 0 ? GSL_SUCCESS : GSL_EINVAL));
    CHECK(p_set(s, &G3.matrix) == GSL_EBADLEN && p_set(s, &G5.matrix) == GSL_EBADLEN);
    CHECK(p_set(s, &G.matrix) == GSL_SUCCESS && p_set(s, NULL) == GSL_SUCCESS);
    CHECK(p_set_options(s, 1e-10, 50) == GSL_SUCCESS && p_set_options(s, 0.0, 50) == GSL_EINVAL && p_set_options(s, 1e-10, 0) == GSL_EINVAL);
    CHECK(p_get(s, &G.matrix, NULL, NULL) == GSL_EINVAL);                                     /* not initialised */
    gsl_sinterp_free(s);
  }
  gsl_sinterp *s = gsl_sinterp_alloc(gsl_sinterp_cubic_mesh, 2, 4);
  CHECK(s != NULL && gsl_sinterp_init(s, &X4.matrix, &F.vector) == GSL_EINVAL);                /* no triangulation set */
  gsl_sinterp_free(s);
  s = gsl_sinterp_alloc(gsl_sinterp_linear_mesh, 2, 4);
  CHECK(s != NULL && p_set(s, &G.matrix) == GSL_EINVAL && p_set_options(s, 1e-10, 50) == GSL_EINVAL);
  CHECK(p_get(s, &G.matrix, NULL, NULL) == GSL_EINVAL);
  gsl_sinterp_free(s);
  /* NULL interpolant, mirror or context: GSL_EFAULT before anything else */
  CHECK(p_set(NULL, &G.matrix) == GSL_EFAULT && p_set_options(NULL, 1e-10, 50) == GSL_EFAULT && p_get(NULL, &G.matrix, NULL, NULL) == GSL_EFAULT);
  CHECK(p_bind(NULL, &G.matrix) == GSL_EFAULT && p_options(NULL, 1e-10, 50) == GSL_EFAULT);
  CHECK(p_gradients(NULL, &G.matrix, NULL, NULL) == GSL_EFAULT);
  CHECK(p_many(NULL, &X4.matrix, &F.vector, NULL, NULL) == GSL_EFAULT);
  CHECK(p_resident(NULL, NULL, 0, 2, NULL, NULL, 2, NULL) == GSL_EFAULT);
  CHECK(p_solve(NULL, 4, NULL, NULL, 0, NULL, NULL, 1e-12, 10, NULL, NULL, NULL) == GSL_EFAULT);
  CHECK(p_pack(NULL, 2, NULL, NULL, 4, NULL, NULL, NULL, NULL) == GSL_EFAULT);
  CHECK(p_eval(NULL, 2, NULL, NULL, NULL, NULL, 0, 2, NULL, NULL, 2) == GSL_EFAULT);
  printf("ok\n");
  return 0;
}
