/* References the variogram prototypes of include/gsl_sinterp.h and include/gsl_sinterp_hip.h with their declared types, and
   calls the entries that answer without a GPU: argument and state errors, and the model fit on host arrays. */
#include <gsl_sinterp.h>
#include <math.h>
#include <stdio.h>

static gsl_sinterp_variogram *(*const p_alloc)(size_t, size_t) = &gsl_sinterp_variogram_alloc;
static int (*const p_dev)(gsl_sinterp_variogram *, int) = &gsl_sinterp_variogram_set_device;
static int (*const p_comp)(gsl_sinterp_variogram *, const gsl_matrix *, const gsl_vector *, double) = &gsl_sinterp_variogram_compute;
static int (*const p_compr)(gsl_sinterp_variogram *, const double *, size_t, size_t, const double *, double) = &gsl_sinterp_variogram_compute_resident;
static int (*const p_get)(const gsl_sinterp_variogram *, int, gsl_vector *, gsl_vector *, gsl_vector *) = &gsl_sinterp_variogram_get;
static double (*const p_hmax)(const gsl_sinterp_variogram *) = &gsl_sinterp_variogram_h_max;
static int (*const p_fit)(gsl_sinterp_variogram *, const gsl_sinterp_type *, int, int, double, double, double *, double *, double *, double *) =
    &gsl_sinterp_variogram_fit;
static int (*const p_apply)(const gsl_sinterp_variogram *, gsl_sinterp *) = &gsl_sinterp_variogram_apply;
static void (*const p_free)(gsl_sinterp_variogram *) = &gsl_sinterp_variogram_free;
static int (*const p_model)(int, int, const double *, const double *, const double *, size_t, double, double, size_t, double, size_t, double *,
                            double *, double *, double *) = &gsl_sinterp_variogram_fit_model;
static size_t (*const p_neval)(void) = &gsl_sinterp_variogram_fit_model_n_eval;
static int (*const p_trace)(gsl_vector *, gsl_vector *) = &gsl_sinterp_variogram_fit_model_trace;
static int (*const p_raw)(gsl_sinterp_hip_ctx *, const double *, size_t, int, size_t, const double *, double, int, unsigned long long *, int *) =
    &gsl_sinterp_hip_variogram;
static unsigned long long (*const p_tested)(const gsl_sinterp_hip_ctx *) = &gsl_sinterp_hip_variogram_pairs_tested;
static int (*const p_box)(gsl_sinterp_hip_ctx *, const double *, size_t, int, size_t, double *) = &gsl_sinterp_hip_bbox;

#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main(void)
{
  gsl_set_error_handler_off();
  CHECK(p_alloc(0, 15) == NULL && p_alloc(4, 15) == NULL && p_alloc(2, 0) == NULL && p_alloc(2, 257) == NULL);
  gsl_sinterp_variogram *v = p_alloc(2, 15);
  CHECK(v != NULL && isnan(p_hmax(v)) && isnan(p_hmax(NULL)));
  CHECK(p_dev(NULL, 0) == GSL_EFAULT && p_dev(v, -1) == GSL_EINVAL && p_dev(v, 0) == GSL_SUCCESS);
  double xx[16] = {0}, ff[8] = {0}, out[15] = {0};
  gsl_matrix_view X = gsl_matrix_view_array(xx, 8, 2), X3 = gsl_matrix_view_array(xx, 5, 3);
  gsl_vector_view F = gsl_vector_view_array(ff, 8), F7 = gsl_vector_view_array(ff, 7), O = gsl_vector_view_array(out, 15), O14 = gsl_vector_view_array(out, 14);
  CHECK(p_comp(NULL, &X.matrix, &F.vector, 1.0) == GSL_EFAULT && p_comp(v, NULL, &F.vector, 1.0) == GSL_EFAULT && p_comp(v, &X.matrix, NULL, 1.0) == GSL_EFAULT);
  CHECK(p_comp(v, &X3.matrix, &F.vector, 1.0) == GSL_EBADLEN && p_comp(v, &X.matrix, &F7.vector, 1.0) == GSL_EBADLEN);
  CHECK(p_comp(v, &X.matrix, &F.vector, NAN) == GSL_EINVAL && p_comp(v, &X.matrix, &F.vector, INFINITY) == GSL_EINVAL);
  CHECK(p_compr(NULL, xx, 8, 2, ff, 1.0) == GSL_EFAULT && p_compr(v, NULL, 8, 2, ff, 1.0) == GSL_EFAULT && p_compr(v, xx, 8, 2, NULL, 1.0) == GSL_EFAULT);
  CHECK(p_compr(v, xx, 8, 1, ff, 1.0) == GSL_EBADLEN && p_compr(v, xx, 8, 2, ff, NAN) == GSL_EINVAL);
  CHECK(p_get(NULL, 0, NULL, NULL, NULL) == GSL_EFAULT && p_get(v, 2, NULL, NULL, NULL) == GSL_EINVAL && p_get(v, 0, &O.vector, NULL, NULL) == GSL_EINVAL);
  (void)O14;
  double e = 0, c0 = 0, c = 0, w = 0;
  CHECK(p_fit(NULL, gsl_sinterp_kriging, 0, 1, 0, 0, &e, &c0, &c, &w) == GSL_EFAULT && p_fit(v, NULL, 0, 1, 0, 0, &e, &c0, &c, &w) == GSL_EFAULT);
  CHECK(p_fit(v, gsl_sinterp_rbf_gaussian, 0, 1, 0, 0, &e, &c0, &c, &w) == GSL_EINVAL && isnan(e) && isnan(c0) && isnan(c) && isnan(w));
  CHECK(p_fit(v, gsl_sinterp_linear_mesh, 0, 1, 0, 0, &e, &c0, &c, &w) == GSL_EUNSUP && p_fit(v, gsl_sinterp_shepard, 0, 1, 0, 0, &e, &c0, &c, &w) == GSL_EUNSUP);
  CHECK(p_fit(v, gsl_sinterp_kriging, 0, 1, 0, 0, &e, &c0, &c, &w) == GSL_EINVAL);          /* no variogram */
  gsl_sinterp *s = gsl_sinterp_alloc(gsl_sinterp_kriging_matern32, 2, 8);
  CHECK(s != NULL && p_apply(NULL, s) == GSL_EFAULT && p_apply(v, NULL) == GSL_EFAULT && p_apply(v, s) == GSL_EINVAL);
  gsl_sinterp_free(s);
  p_free(v);
  p_free(NULL);

  /* the model fit on an exact Matern 3/2 variogram: eps = 8, c0 = 0.2, c = 1.7 */
  double lag[15], gam[15], cnt[15];
  for (int b = 0; b < 15; b++) {
    lag[b] = (b + 0.5) * 0.5 / 15.0;
    const double t = sqrt(3.0) * 8.0 * lag[b];
    gam[b] = 0.2 + 1.7 * (1.0 - (1.0 + t) * exp(-t));
    cnt[b] = 100.0 * (b + 1);
  }
  CHECK(p_model(GSL_SINTERP_RBF_MATERN32, GSL_SINTERP_VARIOGRAM_W_COUNT_H2, lag, gam, cnt, 15, 0.5, 200.0, 9, 1e-8, 200, &e, &c0, &c, &w) == GSL_SUCCESS);
  CHECK(fabs(e - 8.0) < 8e-6 && fabs(c0 - 0.2) < 2e-6 && fabs(c - 1.7) < 1.7e-5 && w >= 0.0 && p_neval() >= 9 && p_neval() <= 200);
  double tp[200], tw[200];
  gsl_vector_view TP = gsl_vector_view_array(tp, p_neval()), TW = gsl_vector_view_array(tw, p_neval()), T1 = gsl_vector_view_array(tw, p_neval() - 1);
  CHECK(p_trace(NULL, NULL) == GSL_EFAULT && p_trace(&TP.vector, &T1.vector) == GSL_EBADLEN && p_trace(&TP.vector, &TW.vector) == GSL_SUCCESS);
  CHECK(tp[0] == 0.5 && tp[8] == 200.0 && tw[0] > w);
  CHECK(p_model(GSL_SINTERP_RBF_TPS, 1, lag, gam, cnt, 15, 0.5, 200.0, 0, 0.0, 0, &e, &c0, &c, &w) == GSL_EINVAL && isnan(e));
  CHECK(p_model(GSL_SINTERP_RBF_GAUSSIAN, 3, lag, gam, cnt, 15, 0.5, 200.0, 0, 0.0, 0, &e, &c0, &c, &w) == GSL_EINVAL);
  CHECK(p_model(GSL_SINTERP_RBF_GAUSSIAN, 1, lag, gam, cnt, 15, 0.0, 200.0, 0, 0.0, 0, &e, &c0, &c, &w) == GSL_EINVAL);
  CHECK(p_model(GSL_SINTERP_RBF_GAUSSIAN, 1, lag, gam, cnt, 15, 0.5, 200.0, 2, 0.0, 0, &e, &c0, &c, &w) == GSL_EINVAL);
  CHECK(p_model(GSL_SINTERP_RBF_GAUSSIAN, 1, NULL, gam, cnt, 15, 0.5, 200.0, 0, 0.0, 0, &e, &c0, &c, &w) == GSL_EFAULT);
  CHECK(p_model(GSL_SINTERP_RBF_GAUSSIAN, 1, lag, gam, cnt, 2, 0.5, 200.0, 0, 0.0, 0, &e, &c0, &c, &w) == GSL_EDOM);

  int shift[3] = {0, 0, 0};
  unsigned long long acc[7] = {0};
  CHECK(p_raw(NULL, NULL, 0, 2, 2, NULL, 1.0, 1, acc, shift) == GSL_EFAULT && p_raw(NULL, NULL, 0, 4, 4, NULL, 1.0, 1, acc, shift) == GSL_EINVAL);
  CHECK(p_raw(NULL, NULL, 0, 2, 2, NULL, 0.0, 1, acc, shift) == GSL_EINVAL && p_raw(NULL, NULL, 0, 2, 2, NULL, 1.0, 257, acc, shift) == GSL_EINVAL);
  CHECK(p_tested(NULL) == 0 && p_box(NULL, NULL, 1, 2, 2, NULL) == GSL_EFAULT && p_box(NULL, NULL, 0, 2, 2, NULL) == GSL_EINVAL);
  printf("ok\n");
  return 0;
}
