/* References the Matern / inverse multiquadric types and kind constants of include/gsl_sinterp.h and
   include/gsl_sinterp_hip.h with their declared types, and calls the entries that answer without a GPU (names, minimum
   sizes, the switches per type, state errors). */
#include <gsl_sinterp.h>
#include <stdio.h>
#include <string.h>

#if GSL_SINTERP_RBF_MATERN32 != 3 || GSL_SINTERP_RBF_MATERN52 != 4 || GSL_SINTERP_RBF_IMQ != 5
#error "the kind constants of the Matern / inverse multiquadric kernels changed"
#endif
#if GSL_SINTERP_RBF_GAUSSIAN != 0 || GSL_SINTERP_RBF_TPS != 1 || GSL_SINTERP_RBF_WENDLAND != 2
#error "the kind constants of the older kernels changed"
#endif

static const gsl_sinterp_type *const *const p_types[5] = {&gsl_sinterp_rbf_matern32, &gsl_sinterp_rbf_matern52, &gsl_sinterp_rbf_imq,
                                                          &gsl_sinterp_kriging_matern32, &gsl_sinterp_kriging_matern52};
static const char *const names[5] = {"rbf-matern-3/2", "rbf-matern-5/2", "rbf-inverse-multiquadric", "ordinary-kriging-matern-3/2",
                                     "ordinary-kriging-matern-5/2"};

#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main(void)
{
  gsl_set_error_handler_off();
  double yy[3] = {0.1, 0.2, 0.3}, gg[3] = {0}, mean = 7.0, val = 7.0;
  for (int t = 0; t < 5; t++) {
    const int krige = t >= 3;
    for (size_t dim = 1; dim <= 3; dim++) {
      gsl_sinterp *s = gsl_sinterp_alloc(*p_types[t], dim, 1);                 /* min_size 1 */
      CHECK(s != NULL && s->type == *p_types[t]);
      CHECK(strcmp(gsl_sinterp_name(s), names[t]) == 0 && gsl_sinterp_min_size(s) == 1);
      gsl_vector_view Y = gsl_vector_view_array(yy, dim), G = gsl_vector_view_array(gg, dim);
      /* every switch the Gaussian / Gaussian-kriging type has */
      CHECK(gsl_sinterp_set_loo(s, 1) == GSL_SUCCESS && s->want_loo == 1);
      CHECK(gsl_sinterp_set_shape(s, 3.0) == GSL_SUCCESS);
      CHECK(gsl_sinterp_set_devices(s, 2) == GSL_SUCCESS && gsl_sinterp_n_devices(s) == 2);
      CHECK(gsl_sinterp_set_nugget(s, 1e-3) == (krige ? GSL_SUCCESS : GSL_EINVAL));
      CHECK(gsl_sinterp_set_variance(s, 1) == (krige ? GSL_SUCCESS : GSL_EINVAL) && s->want_variance == krige);
      CHECK(gsl_sinterp_set_solver(s, GSL_SINTERP_SOLVER_CHOLESKY2) == (krige ? GSL_EINVAL : GSL_SUCCESS));
      CHECK(gsl_sinterp_set_rcond(s, 1) == (krige ? GSL_EINVAL : GSL_SUCCESS));
      /* not initialised: state errors, nothing touches a device */
      CHECK(gsl_sinterp_eval_e(s, &Y.vector, &val) != GSL_SUCCESS);
      CHECK(gsl_sinterp_eval_grad_e(s, &Y.vector, &val, &G.vector) == GSL_EINVAL);
      CHECK(gsl_sinterp_loo_variance(s, &G.vector) == GSL_EINVAL);
      CHECK(gsl_sinterp_mean(s, &mean) == GSL_EINVAL);                         /* kriging: not initialised; others: not kriging */
      CHECK(gsl_sinterp_eval_variance_e(s, &Y.vector, &val) == GSL_EINVAL);
      CHECK(gsl_sinterp_n_fields(s) == 0);
      gsl_sinterp_free(s);
    }
    CHECK(gsl_sinterp_alloc(*p_types[t], 2, 0) == NULL);
  }
  /* the raw entries know six kinds; the affine solve stays thin-plate only (both answer before any device work) */
  CHECK(gsl_sinterp_hip_rbf_fill(NULL, GSL_SINTERP_RBF_IMQ, 1.0, NULL, 0, 2, 2, NULL, 0) == GSL_EFAULT);
  printf("ok\n");
  return 0;
}
