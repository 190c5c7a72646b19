/* References the joint-covariance and simulation prototypes of include/gsl_sinterp.h and include/gsl_sinterp_hip.h with their
   declared types, and calls the entries that answer without a GPU (argument and state errors, the workspace sizes). */
#include <gsl_sinterp.h>
#include <stdio.h>

static int (*const p_cov)(const gsl_sinterp *, const gsl_matrix *, const gsl_matrix *, gsl_matrix *) = &gsl_sinterp_eval_covariance_many;
static int (*const p_covr)(const gsl_sinterp *, const double *, size_t, size_t, const double *, size_t, size_t, double *, size_t) =
    &gsl_sinterp_eval_covariance_resident;
static int (*const p_sim)(const gsl_sinterp *, const gsl_matrix *, double, double, const gsl_matrix *, gsl_matrix *) = &gsl_sinterp_simulate_many;
static int (*const p_simr)(const gsl_sinterp *, const double *, size_t, size_t, double, double, const double *, size_t, size_t, double *,
                           size_t) = &gsl_sinterp_simulate_resident;
static size_t (*const p_work)(size_t, size_t, size_t, size_t) = &gsl_sinterp_hip_krige_covariance_work;
static int (*const p_raw)(gsl_sinterp_hip_ctx *, int, double, int, const double *, const double *, const double *, size_t, int, size_t,
                          const double *, size_t, const double *, size_t, const double *, const double *, const double *, size_t, size_t,
                          const double *, size_t, size_t, double *, size_t, double *) = &gsl_sinterp_hip_krige_covariance;
static size_t (*const p_swork)(size_t, size_t, size_t, size_t) = &gsl_sinterp_hip_krige_simulate_work;
static int (*const p_sraw)(gsl_sinterp_hip_ctx *, int, double, int, const double *, const double *, const double *, size_t, int, size_t,
                           const double *, size_t, const double *, size_t, const double *, const double *, const double *, size_t, size_t,
                           const double *, double, double, const double *, size_t, size_t, double *, size_t, double *) =
    &gsl_sinterp_hip_krige_simulate;

#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main(void)
{
  gsl_set_error_handler_off();
  double yy[10] = {0}, cc[25] = {0}, zz[15] = {0}, oo[15] = {0};
  gsl_matrix_view Y = gsl_matrix_view_array(yy, 5, 2), Cv = gsl_matrix_view_array(cc, 5, 5);
  gsl_matrix_view Z = gsl_matrix_view_array(zz, 5, 3), O = gsl_matrix_view_array(oo, 5, 3);
  const gsl_sinterp_type *yes[3] = {gsl_sinterp_kriging, gsl_sinterp_kriging_matern32, gsl_sinterp_kriging_matern52};
  for (int t = 0; t < 3; t++) {
    gsl_sinterp *s = gsl_sinterp_alloc(yes[t], 2, 8);
    CHECK(s != NULL && gsl_sinterp_set_variance(s, 1) == GSL_SUCCESS);
    CHECK(p_cov(s, &Y.matrix, NULL, &Cv.matrix) == GSL_EINVAL);                         /* not initialised */
    CHECK(p_sim(s, &Y.matrix, 1.0, 0.0, &Z.matrix, &O.matrix) == GSL_EINVAL);
    CHECK(p_covr(s, yy, 5, 2, NULL, 0, 0, cc, 5) == GSL_EINVAL && p_simr(s, yy, 5, 2, 1.0, 0.0, zz, 3, 3, oo, 3) == GSL_EINVAL);
    CHECK(p_cov(s, NULL, NULL, &Cv.matrix) == GSL_EFAULT && p_sim(s, &Y.matrix, 1.0, 0.0, NULL, &O.matrix) == GSL_EFAULT);
    CHECK(p_cov(s, &Y.matrix, NULL, &O.matrix) == GSL_EBADLEN && p_sim(s, &Y.matrix, 1.0, 0.0, &Z.matrix, &Cv.matrix) == GSL_EBADLEN);
    CHECK(gsl_sinterp_set_neighbours(s, 4) == GSL_SUCCESS);
    CHECK(p_cov(s, &Y.matrix, NULL, &Cv.matrix) == GSL_EUNSUP && p_sim(s, &Y.matrix, 1.0, 0.0, &Z.matrix, &O.matrix) == GSL_EUNSUP);
    gsl_sinterp_free(s);
  }
  gsl_sinterp *g = gsl_sinterp_alloc(gsl_sinterp_rbf_gaussian, 2, 8);
  CHECK(g != NULL && p_cov(g, &Y.matrix, NULL, &Cv.matrix) == GSL_EINVAL && p_sim(g, &Y.matrix, 1.0, 0.0, &Z.matrix, &O.matrix) == GSL_EINVAL);
  gsl_sinterp_free(g);
  CHECK(p_cov(NULL, &Y.matrix, NULL, &Cv.matrix) == GSL_EFAULT && p_covr(NULL, yy, 5, 2, NULL, 0, 0, cc, 5) == GSL_EFAULT);
  CHECK(p_sim(NULL, &Y.matrix, 1.0, 0.0, &Z.matrix, &O.matrix) == GSL_EFAULT && p_simr(NULL, yy, 5, 2, 1.0, 0.0, zz, 3, 3, oo, 3) == GSL_EFAULT);
  CHECK(p_work(700, 65, 130, 3) >= (size_t)(128 + 256) * 768 + (65 + 130) * 3);
  CHECK(p_work(700, 65, 0, 1) >= (size_t)128 * 768 + 65 && p_work(700, 65, 0, 1) < p_work(700, 65, 1, 1));
  CHECK(p_swork(700, 65, 16, 1) >= p_work(700, 65, 0, 1) + 65 * 65 + 65 * 16);
  CHECK(p_raw(NULL, 0, 1.0, 0, NULL, NULL, NULL, 8, 2, 2, NULL, 8, NULL, 8, NULL, NULL, NULL, 4, 2, NULL, 0, 0, NULL, 4, NULL) == GSL_EFAULT);
  CHECK(p_sraw(NULL, 0, 1.0, 0, NULL, NULL, NULL, 8, 2, 2, NULL, 8, NULL, 8, NULL, NULL, NULL, 4, 2, NULL, 1.0, 0.0, NULL, 1, 1, NULL, 1, NULL) ==
        GSL_EFAULT);
  printf("ok\n");
  return 0;
}
