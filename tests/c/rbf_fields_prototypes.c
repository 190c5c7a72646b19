/* References the fields prototypes of include/gsl_sinterp.h and include/gsl_sinterp_hip.h with their declared types, and
   calls the entries that answer without a GPU (argument and state errors). */
#include <gsl_sinterp.h>
#include <math.h>
#include <stdio.h>

static int (*const p_init)(gsl_sinterp *, const gsl_matrix *, const gsl_matrix *) = &gsl_sinterp_init_fields;
static size_t (*const p_n)(const gsl_sinterp *) = &gsl_sinterp_n_fields;
static int (*const p_e)(const gsl_sinterp *, const gsl_vector *, gsl_vector *) = &gsl_sinterp_eval_fields_e;
static int (*const p_many)(const gsl_sinterp *, const gsl_matrix *, gsl_matrix *) = &gsl_sinterp_eval_fields_many;
static int (*const p_res)(const gsl_sinterp *, const double *, size_t, size_t, double *, size_t) = &gsl_sinterp_eval_fields_resident;
static int (*const p_w)(const gsl_sinterp *, size_t, gsl_vector *) = &gsl_sinterp_get_field_weights;
static int (*const p_mean)(const gsl_sinterp *, size_t, double *) = &gsl_sinterp_field_mean;
static int (*const p_poly)(const gsl_sinterp *, size_t, gsl_vector *) = &gsl_sinterp_field_poly;
static int (*const p_raw)(gsl_sinterp_hip_ctx *, int, double, const double *, const double *, size_t, int, size_t, const double *, size_t,
                          size_t, const double *, size_t, size_t, double *, size_t, unsigned long long) = &gsl_sinterp_hip_rbf_eval_fields;
static int (*const p_block)(void) = &gsl_sinterp_hip_rbf_fields_block;
static int (*const p_small)(void) = &gsl_sinterp_hip_rbf_fields_block_small;
static int (*const p_solve)(gsl_sinterp_hip_ctx *, int, double, const double *, size_t, int, size_t, double *, size_t, double *, size_t,
                            size_t, int *) = &gsl_sinterp_hip_rbf_solve_fields;
static int (*const p_krige)(gsl_sinterp_hip_ctx *, int, double, double, const double *, size_t, int, size_t, double *, size_t, double *,
                            size_t, size_t, double *, int *) = &gsl_sinterp_hip_krige_solve_fields;

#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main(void)
{
  gsl_set_error_handler_off();
  gsl_sinterp *s = gsl_sinterp_alloc(gsl_sinterp_kriging, 2, 8);
  CHECK(s != NULL);
  CHECK(GSL_SINTERP_MAX_FIELDS == 64);
  CHECK(p_n(s) == 0 && p_n(NULL) == 0);
  CHECK(p_small() >= 1 && p_small() <= p_block() && p_block() <= GSL_SINTERP_MAX_FIELDS);
  double yy[2] = {0.25, 0.5}, ss[3] = {1.0, 2.0, 3.0}, dummy[24] = {0}, mean = 1.0;
  gsl_vector_view y = gsl_vector_view_array(yy, 2), sv = gsl_vector_view_array(ss, 3);
  CHECK(p_e(s, &y.vector, &sv.vector) == GSL_EINVAL);                /* not initialised */
  CHECK(isnan(ss[0]) && isnan(ss[1]) && isnan(ss[2]));
  gsl_matrix_view Y = gsl_matrix_view_array(yy, 1, 2), S = gsl_matrix_view_array(ss, 1, 3);
  CHECK(p_many(s, &Y.matrix, &S.matrix) == GSL_EINVAL);
  CHECK(p_many(s, &Y.matrix, NULL) == GSL_EFAULT);
  CHECK(p_res(s, dummy, 1, 2, dummy, 3) == GSL_EINVAL);
  CHECK(p_res(s, dummy, 1, 2, NULL, 3) == GSL_EFAULT);
  CHECK(p_w(s, 0, &sv.vector) == GSL_EINVAL && p_w(s, 0, NULL) == GSL_EFAULT);
  CHECK(p_mean(s, 0, &mean) == GSL_EINVAL && p_mean(s, 0, NULL) == GSL_EFAULT);
  CHECK(p_poly(s, 0, &sv.vector) == GSL_EINVAL);
  gsl_matrix_view X = gsl_matrix_view_array(dummy, 8, 2), F = gsl_matrix_view_array(dummy, 8, 3), Fshort = gsl_matrix_view_array(dummy, 7, 3);
  CHECK(p_init(s, &X.matrix, NULL) == GSL_EFAULT && p_init(NULL, &X.matrix, &F.matrix) == GSL_EFAULT);
  CHECK(p_init(s, &X.matrix, &Fshort.matrix) == GSL_EBADLEN);
  CHECK(p_raw(NULL, GSL_SINTERP_RBF_TPS, 0.0, NULL, NULL, 0, 2, 2, NULL, 0, 1, NULL, 0, 2, NULL, 1, 0ULL) == GSL_EFAULT);
  CHECK(p_solve(NULL, GSL_SINTERP_RBF_GAUSSIAN, 1.0, NULL, 0, 2, 2, NULL, 0, NULL, 0, 1, NULL) == GSL_EFAULT);
  CHECK(p_krige(NULL, GSL_SINTERP_RBF_GAUSSIAN, 1.0, 0.0, NULL, 0, 2, 2, NULL, 0, NULL, 0, 1, &mean, NULL) == GSL_EFAULT);
  gsl_sinterp_free(s);
  printf("ok\n");
  return 0;
}
