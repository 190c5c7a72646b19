/* References the modified Shepard prototypes of include/gsl_sinterp.h and include/gsl_sinterp_hip.h with their declared
   types, and calls the entries that answer without a GPU: the facade's allocation rules, the bounds of
   gsl_sinterp_set_shepard, the status answers and the argument errors of the raw entries. */
#include <gsl_sinterp.h>
#include <stdio.h>
#include <string.h>

static int (*const p_fit)(gsl_sinterp_hip_ctx *, const double *, size_t, int, size_t, const double *, size_t, size_t, double *, double *,
                          double *, size_t *) = &gsl_sinterp_hip_shepard_fit;
static int (*const p_eval)(gsl_sinterp_hip_ctx *, const double *, size_t, int, size_t, const double *, const double *, const double *,
                           const double *, const double *, size_t, size_t, double *, double *, size_t, int *, size_t *,
                           unsigned long long) = &gsl_sinterp_hip_shepard_eval;
static unsigned long long (*const p_packs)(const gsl_sinterp_hip_ctx *) = &gsl_sinterp_hip_shepard_pack_count;
static unsigned long long (*const p_fits)(const gsl_sinterp_hip_ctx *) = &gsl_sinterp_hip_shepard_fit_count;
static int (*const p_set)(gsl_sinterp *, size_t, size_t) = &gsl_sinterp_set_shepard;
static int (*const p_stats)(const gsl_sinterp *, size_t *, size_t *, double *) = &gsl_sinterp_shepard_stats;
static gsl_sinterp_hip_ctx *(*const p_ctx)(const gsl_sinterp *) = &gsl_sinterp_shepard_ctx;
static const gsl_sinterp_type *const *const p_type = &gsl_sinterp_shepard;

#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main(void)
{
  gsl_set_error_handler_off();
  CHECK(*p_type != NULL && strcmp((*p_type)->name, "modified-quadratic-shepard") == 0);
  CHECK(gsl_sinterp_alloc(*p_type, 1, 100) == NULL && gsl_sinterp_alloc(*p_type, 4, 100) == NULL);
  gsl_sinterp *s2 = gsl_sinterp_alloc(*p_type, 2, 100), *s3 = gsl_sinterp_alloc(*p_type, 3, 100);
  CHECK(s2 != NULL && s3 != NULL);
  CHECK(p_set(s2, 0, 0) == GSL_SUCCESS && p_set(s2, 5, 1) == GSL_SUCCESS && p_set(s2, 62, 62) == GSL_SUCCESS);
  CHECK(p_set(s2, 4, 10) == GSL_EINVAL && p_set(s2, 63, 10) == GSL_EINVAL && p_set(s2, 10, 63) == GSL_EINVAL);
  CHECK(p_set(s3, 8, 10) == GSL_EINVAL && p_set(s3, 9, 1) == GSL_SUCCESS);
  CHECK(p_set(NULL, 0, 0) == GSL_EFAULT);
  size_t nl = 7, nk = 7;
  double rw = 1.0;
  CHECK(p_stats(s2, &nl, &nk, &rw) == GSL_EINVAL && p_stats(NULL, &nl, &nk, &rw) == GSL_EFAULT);
  CHECK(p_ctx(s2) == NULL && p_ctx(NULL) == NULL);
  CHECK(p_packs(NULL) == 0 && p_fits(NULL) == 0);
  gsl_sinterp *g = gsl_sinterp_alloc(gsl_sinterp_rbf_gaussian, 2, 100);
  CHECK(g != NULL && p_set(g, 0, 0) == GSL_EINVAL && p_stats(g, NULL, NULL, NULL) == GSL_EINVAL && p_ctx(g) == NULL);
  /* the raw entries: the numbers first, then the pointers */
  double one[8] = {0};
  size_t counts[3] = {9, 9, 9}, outside = 9;
  CHECK(p_fit(NULL, one, 100, 1, 1, one, 13, 19, one, one, one, counts) == GSL_EINVAL);
  CHECK(p_fit(NULL, one, 100, 2, 2, one, 4, 19, one, one, one, counts) == GSL_EINVAL);
  CHECK(p_fit(NULL, one, 100, 2, 2, one, 13, 0, one, one, one, counts) == GSL_EINVAL);
  CHECK(p_fit(NULL, one, 100, 2, 2, one, 63, 19, one, one, one, counts) == GSL_EINVAL);
  CHECK(p_fit(NULL, one, 20, 2, 2, one, 13, 19, one, one, one, counts) == GSL_EINVAL);
  CHECK(p_fit(NULL, one, 100, 3, 2, one, 17, 32, one, one, one, counts) == GSL_EINVAL);
  CHECK(p_fit(NULL, one, 100, 2, 2, one, 13, 19, one, one, one, counts) == GSL_EFAULT);
  CHECK(counts[0] == 0 && counts[1] == 0 && counts[2] == 0);
  CHECK(p_eval(NULL, one, 100, 4, 4, one, one, one, one, one, 1, 4, one, NULL, 0, NULL, &outside, 0) == GSL_EINVAL);
  CHECK(p_eval(NULL, one, 100, 2, 2, one, one, one, one, one, 1, 1, one, NULL, 0, NULL, &outside, 0) == GSL_EINVAL);
  CHECK(p_eval(NULL, one, 100, 2, 2, one, one, one, one, one, 1, 2, one, one, 1, NULL, &outside, 0) == GSL_EINVAL);
  CHECK(p_eval(NULL, one, 100, 2, 2, one, one, one, one, one, 1, 2, one, NULL, 0, NULL, &outside, 0) == GSL_EFAULT && outside == 0);
  gsl_sinterp_free(s2); gsl_sinterp_free(s3); gsl_sinterp_free(g);
  printf("ok\n");
  return 0;
}
