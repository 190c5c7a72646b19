/* References the value + gradient prototypes of include/gsl_sinterp.h and include/gsl_sinterp_hip.h with their declared
   types, and calls the entries that answer without a GPU (argument and state errors). */
#include <gsl_sinterp.h>
#include <math.h>
#include <stdio.h>

static int (*const p_e)(const gsl_sinterp *, const gsl_vector *, double *, gsl_vector *) = &gsl_sinterp_eval_grad_e;
static int (*const p_many)(const gsl_sinterp *, const gsl_matrix *, gsl_vector *, gsl_matrix *) = &gsl_sinterp_eval_grad_many;
static int (*const p_res)(const gsl_sinterp *, const double *, size_t, size_t, double *, double *, size_t) = &gsl_sinterp_eval_grad_resident;
static int (*const p_raw)(gsl_sinterp_hip_ctx *, int, double, const double *, const double *, size_t, int, size_t, const double *,
                          const double *, size_t, size_t, double *, double *, size_t, unsigned long long) = &gsl_sinterp_hip_rbf_eval_grad;

#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main(void)
{
  gsl_set_error_handler_off();
  gsl_sinterp *s = gsl_sinterp_alloc(gsl_sinterp_rbf_tps_affine, 2, 8);
  CHECK(s != NULL);
  double yy[2] = {0.25, 0.5}, gg[2] = {1.0, 2.0}, val = 3.0, dummy[4] = {0};
  gsl_vector_view y = gsl_vector_view_array(yy, 2), g = gsl_vector_view_array(gg, 2);
  CHECK(p_e(s, &y.vector, &val, &g.vector) == GSL_EINVAL);          /* not initialised */
  CHECK(isnan(val) && isnan(gg[0]) && isnan(gg[1]));
  gsl_matrix_view Y = gsl_matrix_view_array(yy, 1, 2), G = gsl_matrix_view_array(gg, 1, 2);
  CHECK(p_many(s, &Y.matrix, NULL, &G.matrix) == GSL_EINVAL);
  CHECK(p_many(s, &Y.matrix, NULL, NULL) == GSL_EFAULT);
  CHECK(p_res(s, dummy, 1, 2, NULL, dummy, 2) == GSL_EINVAL);
  CHECK(p_res(s, dummy, 1, 2, NULL, NULL, 2) == GSL_EFAULT);
  CHECK(p_raw(NULL, GSL_SINTERP_RBF_TPS, 0.0, NULL, NULL, 0, 2, 2, NULL, NULL, 0, 2, NULL, NULL, 2, 0ULL) == GSL_EFAULT);
  gsl_sinterp_free(s);
  printf("ok\n");
  return 0;
}
