/* References the prototypes of the linear fields entries (include/gsl_sinterp.h parts 2, 2b and 3, include/gsl_sinterp_hip.h)
   with their declared types, and calls the ones that answer without a GPU (argument, type and state errors). */
#include <gsl_sinterp.h>
#include <math.h>
#include <stdio.h>

static int (*const p_init)(gsl_sinterp *, const gsl_matrix *, const gsl_matrix *) = &gsl_sinterp_linear_init_fields;
static int (*const p_e)(const gsl_sinterp *, const gsl_vector *, gsl_vector *, gsl_matrix *) = &gsl_sinterp_linear_eval_fields_e;
static int (*const p_many)(const gsl_sinterp *, const gsl_matrix *, gsl_matrix *, gsl_matrix *, int *) = &gsl_sinterp_linear_eval_fields_many;
static int (*const p_res)(const gsl_sinterp *, const double *, size_t, size_t, double *, size_t, double *, size_t, int *) =
    &gsl_sinterp_linear_eval_fields_resident;
static int (*const t_set)(simplex_tree_device *, const gsl_matrix *) = &simplex_tree_device_set_responses;
static size_t (*const t_n)(const simplex_tree_device *) = &simplex_tree_device_n_responses;
static int (*const t_many)(simplex_tree_device *, const gsl_matrix *, gsl_matrix *, gsl_matrix *, simplex_index *) =
    &simplex_tree_device_eval_fields_many;
static int (*const t_res)(simplex_tree_device *, const double *, size_t, size_t, double *, size_t, double *, size_t, simplex_index *) =
    &simplex_tree_device_eval_fields_resident;
static int (*const m_set)(simplex_mesh_device *, const gsl_matrix *) = &simplex_mesh_device_set_responses;
static size_t (*const m_n)(const simplex_mesh_device *) = &simplex_mesh_device_n_responses;
static int (*const m_many)(simplex_mesh_device *, const gsl_matrix *, gsl_matrix *, gsl_matrix *, int *) = &simplex_mesh_device_eval_fields_many;
static int (*const m_res)(simplex_mesh_device *, const double *, size_t, size_t, double *, size_t, double *, size_t, int *) =
    &simplex_mesh_device_eval_fields_resident;
static int (*const h_bary)(gsl_sinterp_hip_ctx *, int, const void *, const int *, int, const double *, int, size_t, const double *, const int *,
                           const double *, size_t, size_t, double *, size_t, double *, size_t) = &gsl_sinterp_hip_bary_fields_eval;
static int (*const h_mesh3)(gsl_sinterp_hip_ctx *, int, const void *, const int *, int, const double *, int, size_t, const double *, const int *,
                            const double *, size_t, size_t, double *, size_t, double *, size_t) = &gsl_sinterp_hip_mesh3_fields_eval;
static int (*const h_sort)(size_t) = &gsl_sinterp_hip_sort_wanted;

#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main(void)
{
  gsl_set_error_handler_off();
  double yy[2] = {0.25, 0.5}, ss[3] = {1.0, 2.0, 3.0}, gg[6] = {1.0, 1.0, 1.0, 1.0, 1.0, 1.0}, dummy[24] = {0};
  int leaf[1] = {7};
  gsl_vector_view y = gsl_vector_view_array(yy, 2), sv = gsl_vector_view_array(ss, 3);
  gsl_matrix_view Y = gsl_matrix_view_array(yy, 1, 2), S = gsl_matrix_view_array(ss, 1, 3), G = gsl_matrix_view_array(gg, 1, 6);
  gsl_matrix_view g = gsl_matrix_view_array(gg, 3, 2);
  gsl_matrix_view X = gsl_matrix_view_array(dummy, 8, 2), F = gsl_matrix_view_array(dummy, 8, 3), Fshort = gsl_matrix_view_array(dummy, 7, 3);
  gsl_matrix_view F0 = gsl_matrix_view_array_with_tda(dummy, 8, 0, 3);

  /* another type: one refusal, whatever else is wrong */
  gsl_sinterp *r = gsl_sinterp_alloc(gsl_sinterp_rbf_gaussian, 2, 8);
  CHECK(r != NULL);
  CHECK(p_init(r, &X.matrix, &F.matrix) == GSL_EUNSUP && p_init(r, &X.matrix, &Fshort.matrix) == GSL_EUNSUP);
  CHECK(p_many(r, &Y.matrix, &S.matrix, &G.matrix, leaf) == GSL_EUNSUP && p_res(r, dummy, 1, 2, dummy, 3, NULL, 0, NULL) == GSL_EUNSUP);
  CHECK(p_e(r, &y.vector, &sv.vector, &g.matrix) == GSL_EUNSUP && isnan(ss[0]) && isnan(ss[2]) && isnan(gg[0]) && isnan(gg[5]));
  gsl_sinterp_free(r);

  /* the two linear types, never initialised */
  const gsl_sinterp_type *types[2] = {gsl_sinterp_linear_simplex, gsl_sinterp_linear_mesh};
  for (int k = 0; k < 2; k++) {
    gsl_sinterp *s = gsl_sinterp_alloc(types[k], 2, 8);
    CHECK(s != NULL && gsl_sinterp_n_fields(s) == 0);
    CHECK(p_init(NULL, &X.matrix, &F.matrix) == GSL_EFAULT && p_init(s, NULL, &F.matrix) == GSL_EFAULT && p_init(s, &X.matrix, NULL) == GSL_EFAULT);
    CHECK(p_init(s, &X.matrix, &Fshort.matrix) == GSL_EBADLEN);
    CHECK(p_init(s, &X.matrix, &F0.matrix) == GSL_EINVAL);                    /* K = 0 */
    ss[0] = 1.0; gg[0] = 1.0;
    CHECK(p_e(s, &y.vector, &sv.vector, &g.matrix) == GSL_EINVAL && isnan(ss[0]) && isnan(gg[0]));     /* not initialised */
    CHECK(p_e(s, &y.vector, NULL, NULL) == GSL_EFAULT);
    CHECK(p_many(s, &Y.matrix, &S.matrix, NULL, NULL) == GSL_EINVAL && p_many(s, &Y.matrix, NULL, NULL, NULL) == GSL_EFAULT);
    CHECK(p_many(s, &S.matrix, &S.matrix, NULL, NULL) == GSL_EBADLEN);        /* targets 1 x 3 */
    CHECK(p_res(s, dummy, 1, 2, dummy, 3, dummy, 6, leaf) == GSL_EINVAL && p_res(s, dummy, 1, 2, NULL, 3, NULL, 0, NULL) == GSL_EFAULT);
    CHECK(p_res(NULL, dummy, 1, 2, dummy, 3, NULL, 0, NULL) == GSL_EFAULT);
    gsl_sinterp_free(s);
  }

  /* mirrors and raw entries: NULL comes first */
  CHECK(t_set(NULL, &F.matrix) == GSL_EFAULT && t_n(NULL) == 0 && t_many(NULL, &Y.matrix, &S.matrix, NULL, NULL) == GSL_EFAULT);
  CHECK(t_res(NULL, dummy, 1, 2, dummy, 3, NULL, 0, NULL) == GSL_EFAULT);
  CHECK(m_set(NULL, &F.matrix) == GSL_EFAULT && m_n(NULL) == 0 && m_many(NULL, &Y.matrix, &S.matrix, NULL, NULL) == GSL_EFAULT);
  CHECK(m_res(NULL, dummy, 1, 2, dummy, 3, NULL, 0, NULL) == GSL_EFAULT);
  CHECK(h_bary(NULL, 1, dummy, leaf, 3, dummy, 1, 1, dummy, leaf, dummy, 1, 2, dummy, 1, NULL, 0) == GSL_EFAULT);
  CHECK(h_mesh3(NULL, 1, dummy, leaf, 4, dummy, 1, 1, dummy, leaf, dummy, 1, 3, dummy, 1, NULL, 0) == GSL_EFAULT);
  CHECK(h_sort(1) == 0);
  printf("ok\n");
  return 0;
}
