/* References the model-selection prototypes of include/gsl_sinterp.h and include/gsl_sinterp_hip.h with their declared
   types, and calls the entries that answer without a GPU (argument errors; the status of fit_alloc arrives through the
   GSL error handler, as for every GSL entry that returns a pointer). */
#include <gsl_sinterp.h>
#include <math.h>
#include <stdio.h>

static gsl_sinterp_fit_workspace *(*const p_alloc)(const gsl_sinterp *, const gsl_matrix *, const gsl_vector *) = &gsl_sinterp_fit_alloc;
static void (*const p_free)(gsl_sinterp_fit_workspace *) = &gsl_sinterp_fit_free;
static int (*const p_score)(gsl_sinterp_fit_workspace *, int, double, double, double *) = &gsl_sinterp_fit_score;
static int (*const p_shape)(gsl_sinterp_fit_workspace *, int, double, double, double, double *, double *) = &gsl_sinterp_fit_shape;
static int (*const p_nugget)(gsl_sinterp_fit_workspace *, int, double, double, double, double *, double *) = &gsl_sinterp_fit_nugget;
static int (*const p_search)(gsl_sinterp_fit_workspace *, size_t, double, size_t) = &gsl_sinterp_fit_set_search;
static size_t (*const p_neval)(const gsl_sinterp_fit_workspace *) = &gsl_sinterp_fit_n_eval;
static int (*const p_trace)(const gsl_sinterp_fit_workspace *, gsl_vector *, gsl_vector *) = &gsl_sinterp_fit_trace;
static int (*const p_sigma2)(const gsl_sinterp_fit_workspace *, double *) = &gsl_sinterp_fit_sigma2;
static int (*const p_reduce)(gsl_sinterp_hip_ctx *, size_t, const double *, size_t, const double *, const double *, const double *,
                             const double *, double, double *) = &gsl_sinterp_hip_score_reduce;

static int last_errno, n_calls;
static void record(const char *reason, const char *file, int line, int gsl_errno)
{
  (void)reason; (void)file; (void)line;
  last_errno = gsl_errno; n_calls++;
}

#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main(void)
{
  gsl_set_error_handler(&record);
  CHECK(GSL_SINTERP_FIT_LOO == 0 && GSL_SINTERP_FIT_ML == 1);
  double xx[16] = {0}, ff[8] = {0};
  gsl_matrix_view X = gsl_matrix_view_array(xx, 8, 2), X3 = gsl_matrix_view_array(xx, 5, 3), X7 = gsl_matrix_view_array(xx, 7, 2);
  gsl_vector_view F = gsl_vector_view_array(ff, 8), F7 = gsl_vector_view_array(ff, 7);
  const gsl_sinterp_type *no[4] = {gsl_sinterp_rbf_tps, gsl_sinterp_rbf_tps_affine, gsl_sinterp_linear_simplex, gsl_sinterp_linear_mesh};
  for (int t = 0; t < 4; t++) {
    gsl_sinterp *s = gsl_sinterp_alloc(no[t], 2, 8);
    CHECK(s != NULL);
    last_errno = 0;
    CHECK(p_alloc(s, &X.matrix, &F.vector) == NULL && last_errno == GSL_EINVAL);
    gsl_sinterp_free(s);
  }
  const gsl_sinterp_type *yes[8] = {gsl_sinterp_rbf_gaussian, gsl_sinterp_rbf_wendland, gsl_sinterp_rbf_matern32, gsl_sinterp_rbf_matern52,
                                    gsl_sinterp_rbf_imq, gsl_sinterp_kriging, gsl_sinterp_kriging_matern32, gsl_sinterp_kriging_matern52};
  for (int t = 0; t < 8; t++) {
    gsl_sinterp *s = gsl_sinterp_alloc(yes[t], 2, 8);
    CHECK(s != NULL);
    last_errno = 0; CHECK(p_alloc(s, &X3.matrix, &F.vector) == NULL && last_errno == GSL_EBADLEN);
    last_errno = 0; CHECK(p_alloc(s, &X7.matrix, &F.vector) == NULL && last_errno == GSL_EBADLEN);
    last_errno = 0; CHECK(p_alloc(s, &X.matrix, &F7.vector) == NULL && last_errno == GSL_EBADLEN);
    last_errno = 0; CHECK(p_alloc(s, NULL, &F.vector) == NULL && last_errno == GSL_EFAULT);
    last_errno = 0; CHECK(p_alloc(s, &X.matrix, NULL) == NULL && last_errno == GSL_EFAULT);
    CHECK(s->shape == 0.0 && gsl_sinterp_n_fields(s) == 0);                       /* the interpolant is not touched */
    gsl_sinterp_free(s);
  }
  last_errno = 0; CHECK(p_alloc(NULL, &X.matrix, &F.vector) == NULL && last_errno == GSL_EFAULT);
  double v = 0.0, p = 0.0;
  CHECK(p_score(NULL, GSL_SINTERP_FIT_ML, 1.0, 0.0, &v) == GSL_EFAULT && isnan(v));
  CHECK(p_shape(NULL, GSL_SINTERP_FIT_ML, 0.0, 1.0, 2.0, &p, &v) == GSL_EFAULT && isnan(p) && isnan(v));
  p = v = 0.0;
  CHECK(p_nugget(NULL, GSL_SINTERP_FIT_LOO, 1.0, 1e-4, 1.0, &p, &v) == GSL_EFAULT && isnan(p) && isnan(v));
  /* the numbers of the search are judged before the workspace pointer */
  CHECK(p_search(NULL, 2, 1e-2, 40) == GSL_EINVAL && p_search(NULL, 9, 0.0, 40) == GSL_EINVAL && p_search(NULL, 9, -1.0, 40) == GSL_EINVAL);
  CHECK(p_search(NULL, 9, 1e-2, 8) == GSL_EINVAL && p_search(NULL, 9, 1e-2, 40) == GSL_EFAULT);
  CHECK(p_neval(NULL) == 0);
  CHECK(p_trace(NULL, &F.vector, &F.vector) == GSL_EFAULT && p_sigma2(NULL, &v) == GSL_EFAULT && isnan(v));
  const int before = n_calls;
  p_free(NULL);                                                                   /* a no-op */
  CHECK(n_calls == before);
  CHECK(p_reduce(NULL, 8, NULL, 8, NULL, NULL, NULL, NULL, 1.0, NULL) == GSL_EFAULT);
  printf("ok\n");
  return 0;
}
