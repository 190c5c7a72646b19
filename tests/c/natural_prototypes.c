/* References the natural-neighbour prototypes of include/gsl_sinterp.h and include/gsl_sinterp_hip.h with their declared
   types, and calls the entries that answer without a GPU: simplex_mesh_delaunay_metric on small meshes, the facade's
   allocation rules and status answers, and the argument errors of the device entries. */
#include <gsl_sinterp.h>
#include <stdio.h>

static int (*const p_metric)(const simplex_mesh *) = &simplex_mesh_delaunay_metric;
static int (*const p_many)(simplex_mesh_device *, const gsl_matrix *, gsl_vector *, int *) = &simplex_mesh_device_eval_natural_many;
static int (*const p_resident)(simplex_mesh_device *, const double *, size_t, size_t, double *, int *) =
    &simplex_mesh_device_eval_natural_resident;
static int (*const p_pack)(gsl_sinterp_hip_ctx *, int, const int *, const int *, int, const double *, const double *, void *) =
    &gsl_sinterp_hip_mesh_natural_pack;
static int (*const p_eval)(gsl_sinterp_hip_ctx *, int, const void *, const void *, const int *, const double *, const double *, size_t,
                           size_t, int, double *, long long *) = &gsl_sinterp_hip_mesh_natural_eval;
static const gsl_sinterp_type *const *const p_types[2] = {&gsl_sinterp_natural_mesh, &gsl_sinterp_natural_simplex};

#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main(void)
{
  gsl_set_error_handler_off();
  /* a kite in a square bounding box (standardising changes nothing): the diagonal 0-2 is the Delaunay one, 1-3 is not */
  double xy[8] = {0.0, 0.0, 2.0, -1.5, 3.0, 0.0, 2.0, 1.5};
  gsl_matrix_view X = gsl_matrix_view_array(xy, 4, 2);
  const int good[6] = {0, 1, 2, 0, 2, 3}, bad[6] = {0, 1, 3, 1, 2, 3};
  simplex_mesh *m = simplex_mesh_import(&X.matrix, good, NULL, 2);
  CHECK(m != NULL && p_metric(m) == 1);
  simplex_mesh_free(m);
  m = simplex_mesh_import(&X.matrix, bad, NULL, 2);
  CHECK(m != NULL && p_metric(m) == 0);
  simplex_mesh_free(m);
  /* stretched along x by 100, the same triangles: Delaunay in the standardised coordinates only */
  double wide[8] = {0.0, 0.0, 200.0, -1.5, 300.0, 0.0, 200.0, 1.5};
  gsl_matrix_view W = gsl_matrix_view_array(wide, 4, 2);
  m = simplex_mesh_import(&W.matrix, good, NULL, 2);
  CHECK(m != NULL && p_metric(m) == 2);
  simplex_mesh_free(m);
  CHECK(p_metric(NULL) == 0);
  /* the facade: dim 2 only */
  for (int i = 0; i < 2; i++) {
    CHECK(gsl_sinterp_alloc(*p_types[i], 3, 8) == NULL && gsl_sinterp_alloc(*p_types[i], 1, 8) == NULL);
    gsl_sinterp *s = gsl_sinterp_alloc(*p_types[i], 2, 4);
    CHECK(s != NULL);
    CHECK(gsl_sinterp_set_neighbours(s, 2) == GSL_EUNSUP);
    CHECK(gsl_sinterp_eval_grad_resident(s, NULL, 0, 2, NULL, NULL, 2) == GSL_EUNSUP);
    CHECK(gsl_sinterp_eval_variance_resident(s, NULL, 0, 2, NULL) == GSL_EUNSUP);
    CHECK(gsl_sinterp_set_triangulation(s, good, NULL, 2) == (i == 0 ? GSL_SUCCESS : GSL_EINVAL));
    gsl_sinterp_free(s);
  }
  gsl_sinterp *s = gsl_sinterp_alloc(gsl_sinterp_natural_mesh, 2, 4);
  double ff[4] = {0};
  gsl_vector_view F = gsl_vector_view_array(ff, 4);
  CHECK(s != NULL && gsl_sinterp_init(s, &X.matrix, &F.vector) == GSL_EINVAL);   /* no triangulation set */
  CHECK(gsl_sinterp_set_triangulation(s, bad, NULL, 2) == GSL_SUCCESS);
  CHECK(gsl_sinterp_init(s, &X.matrix, &F.vector) == GSL_EINVAL);                /* not Delaunay: refused before any device work */
  gsl_sinterp_free(s);
  /* device entries: argument errors come before any device work */
  CHECK(p_many(NULL, &X.matrix, &F.vector, NULL) == GSL_EFAULT);
  CHECK(p_resident(NULL, NULL, 0, 2, NULL, NULL) == GSL_EFAULT);
  CHECK(p_pack(NULL, 2, NULL, NULL, 4, NULL, NULL, NULL) == GSL_EFAULT);
  CHECK(p_eval(NULL, 2, NULL, NULL, NULL, NULL, NULL, 0, 2, 0, NULL, NULL) == GSL_EFAULT);
  printf("ok\n");
  return 0;
}
