/* References the local-kriging prototypes of include/gsl_sinterp.h and include/gsl_sinterp_hip.h with their declared types,
   and calls the entries that answer without a GPU (argument errors, the GSL_EUNSUP answers of the local route). */
#include <gsl_sinterp.h>
#include <stdio.h>

static int (*const p_set)(gsl_sinterp *, size_t) = &gsl_sinterp_set_neighbours;
static int (*const p_many)(const gsl_sinterp *, const gsl_matrix *, gsl_vector *, gsl_vector *, int *) = &gsl_sinterp_eval_local_many;
static int (*const p_knn)(gsl_sinterp_hip_ctx *, const double *, size_t, int, size_t, const double *, size_t, size_t, size_t, int *, double *,
                          unsigned long long) = &gsl_sinterp_hip_knn;
static int (*const p_krige)(gsl_sinterp_hip_ctx *, int, double, double, const double *, size_t, int, size_t, const double *, const double *,
                            size_t, size_t, size_t, double *, double *, int *, size_t *, unsigned long long) = &gsl_sinterp_hip_local_krige;
static int (*const p_pack)(gsl_sinterp_hip_ctx *, const double *, size_t, int, size_t, const double *, unsigned long long) =
    &gsl_sinterp_hip_local_pack;
static unsigned long long (*const p_count)(const gsl_sinterp_hip_ctx *) = &gsl_sinterp_hip_local_pack_count;

#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main(void)
{
  gsl_set_error_handler_off();
  const gsl_sinterp_type *yes[3] = {gsl_sinterp_kriging, gsl_sinterp_kriging_matern32, gsl_sinterp_kriging_matern52};
  const gsl_sinterp_type *no[4] = {gsl_sinterp_rbf_gaussian, gsl_sinterp_rbf_matern52, gsl_sinterp_rbf_tps, gsl_sinterp_linear_simplex};
  double yy[2] = {0.5, 0.5}, ss[1] = {0}, gg[2] = {0}, ww[100] = {0}, mean = 0;
  gsl_matrix_view Y = gsl_matrix_view_array(yy, 1, 2), G = gsl_matrix_view_array(gg, 1, 2);
  gsl_vector_view S = gsl_vector_view_array(ss, 1), W = gsl_vector_view_array(ww, 100);
  for (int t = 0; t < 3; t++) {
    gsl_sinterp *s = gsl_sinterp_alloc(yes[t], 2, 100);
    CHECK(s != NULL && s->neighbours == 0);
    CHECK(p_set(s, 16) == GSL_SUCCESS && s->neighbours == 16);
    CHECK(p_set(s, 65) == GSL_EINVAL && s->neighbours == 16);
    CHECK(gsl_sinterp_eval_grad_many(s, &Y.matrix, &S.vector, &G.matrix) == GSL_EUNSUP);
    CHECK(gsl_sinterp_get_weights(s, &W.vector) == GSL_EUNSUP);
    CHECK(gsl_sinterp_mean(s, &mean) == GSL_EUNSUP);
    CHECK(gsl_sinterp_loo_variance(s, &W.vector) == GSL_EUNSUP);
    CHECK(p_many(s, &Y.matrix, &S.vector, NULL, NULL) == GSL_EINVAL);               /* not initialised */
    CHECK(p_many(NULL, &Y.matrix, &S.vector, NULL, NULL) == GSL_EFAULT);
    CHECK(p_set(s, 0) == GSL_SUCCESS && s->neighbours == 0);
    CHECK(gsl_sinterp_mean(s, &mean) == GSL_EINVAL);                                /* global again: not initialised */
    gsl_sinterp_free(s);
  }
  for (int t = 0; t < 4; t++) {
    gsl_sinterp *s = gsl_sinterp_alloc(no[t], 2, 100);
    CHECK(s != NULL);
    CHECK(p_set(s, 16) == GSL_EINVAL && s->neighbours == 0);
    gsl_sinterp_free(s);
  }
  CHECK(p_set(NULL, 1) == GSL_EFAULT);
  CHECK(p_knn(NULL, NULL, 100, 2, 2, NULL, 1, 2, 8, NULL, NULL, 0) == GSL_EFAULT);
  CHECK(p_knn(NULL, NULL, 100, 2, 2, NULL, 1, 2, 0, NULL, NULL, 0) == GSL_EINVAL);
  CHECK(p_krige(NULL, GSL_SINTERP_RBF_MATERN52, 1.0, 0.0, NULL, 100, 2, 2, NULL, NULL, 1, 2, 8, NULL, NULL, NULL, NULL, 0) == GSL_EFAULT);
  CHECK(p_krige(NULL, GSL_SINTERP_RBF_TPS, 1.0, 0.0, NULL, 100, 2, 2, NULL, NULL, 1, 2, 8, NULL, NULL, NULL, NULL, 0) == GSL_EINVAL);
  CHECK(p_pack(NULL, NULL, 100, 2, 2, NULL, 0) == GSL_EFAULT);
  CHECK(p_count(NULL) == 0);
  printf("ok\n");
  return 0;
}
