/* References the leave-one-out prototypes of include/gsl_sinterp.h and include/gsl_sinterp_hip.h with their declared types,
   and calls the entries that answer without a GPU (argument and state errors, the workspace size). */
#include <gsl_sinterp.h>
#include <stdio.h>

static int (*const p_set)(gsl_sinterp *, int) = &gsl_sinterp_set_loo;
static int (*const p_res)(const gsl_sinterp *, gsl_matrix *) = &gsl_sinterp_loo_residuals;
static int (*const p_var)(const gsl_sinterp *, gsl_vector *) = &gsl_sinterp_loo_variance;
static size_t (*const p_work)(size_t, size_t) = &gsl_sinterp_hip_chol_inv_diag_work;
static int (*const p_diag)(gsl_sinterp_hip_ctx *, size_t, const double *, size_t, double *, double *, size_t) = &gsl_sinterp_hip_chol_inv_diag;
static int (*const p_comb)(gsl_sinterp_hip_ctx *, size_t, size_t, const double *, const double *, double, const double *, size_t, double *,
                           size_t, double *) = &gsl_sinterp_hip_loo_combine;

#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main(void)
{
  gsl_set_error_handler_off();
  const gsl_sinterp_type *yes[3] = {gsl_sinterp_rbf_gaussian, gsl_sinterp_rbf_wendland, gsl_sinterp_kriging};
  const gsl_sinterp_type *no[4] = {gsl_sinterp_rbf_tps, gsl_sinterp_rbf_tps_affine, gsl_sinterp_linear_simplex, gsl_sinterp_linear_mesh};
  double ee[8] = {0}, vv[8] = {0};
  gsl_matrix_view E = gsl_matrix_view_array(ee, 8, 1);
  gsl_vector_view V = gsl_vector_view_array(vv, 8);
  for (int t = 0; t < 3; t++) {
    gsl_sinterp *s = gsl_sinterp_alloc(yes[t], 2, 8);
    CHECK(s != NULL && s->want_loo == 0);
    CHECK(p_set(s, 1) == GSL_SUCCESS && s->want_loo == 1);
    CHECK(p_res(s, &E.matrix) == GSL_EINVAL && p_var(s, &V.vector) == GSL_EINVAL);     /* not initialised */
    CHECK(p_res(s, NULL) == GSL_EFAULT && p_var(s, NULL) == GSL_EFAULT);
    CHECK(p_set(s, 0) == GSL_SUCCESS && s->want_loo == 0);
    gsl_sinterp_free(s);
  }
  for (int t = 0; t < 4; t++) {
    gsl_sinterp *s = gsl_sinterp_alloc(no[t], 2, 8);
    CHECK(s != NULL);
    CHECK(p_set(s, 1) == GSL_EINVAL && s->want_loo == 0);
    CHECK(p_res(s, &E.matrix) == GSL_EINVAL && p_var(s, &V.vector) == GSL_EINVAL);
    gsl_sinterp_free(s);
  }
  CHECK(p_set(NULL, 1) == GSL_EFAULT);
  CHECK(p_work(700, 256) >= (size_t)256 * 768 + 700);
  CHECK(p_diag(NULL, 8, NULL, 8, NULL, NULL, 128) == GSL_EFAULT);
  CHECK(p_comb(NULL, 8, 1, NULL, NULL, 1.0, NULL, 8, NULL, 8, NULL) == GSL_EFAULT);
  printf("ok\n");
  return 0;
}
