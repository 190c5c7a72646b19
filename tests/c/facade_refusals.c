/* Walks the sixteen extern type pointers of include/gsl_sinterp.h and asks an interpolant that was never initialised for
   what only some families have: the weights, a solver, a grid, the affine polynomial, the kriging mean.  Every answer is
   a status; none may read the state of one family as another's.  Also: gsl_sinterp_alloc with a type that is not one of
   the sixteen.  No GPU is touched. */
#include <gsl_sinterp.h>
#include <stdio.h>

enum { RBF, TREE, MESH };
static const struct {
  const gsl_sinterp_type *const *type;
  int family, krige, affine, tps;
} types[16] = {
  {&gsl_sinterp_rbf_gaussian, RBF, 0, 0, 0},   {&gsl_sinterp_rbf_tps, RBF, 0, 0, 1},          {&gsl_sinterp_linear_simplex, TREE, 0, 0, 0},
  {&gsl_sinterp_rbf_wendland, RBF, 0, 0, 0},   {&gsl_sinterp_kriging, RBF, 1, 0, 0},          {&gsl_sinterp_rbf_tps_affine, RBF, 0, 1, 1},
  {&gsl_sinterp_linear_mesh, MESH, 0, 0, 0},   {&gsl_sinterp_rbf_matern32, RBF, 0, 0, 0},     {&gsl_sinterp_rbf_matern52, RBF, 0, 0, 0},
  {&gsl_sinterp_rbf_imq, RBF, 0, 0, 0},        {&gsl_sinterp_kriging_matern32, RBF, 1, 0, 0}, {&gsl_sinterp_kriging_matern52, RBF, 1, 0, 0},
  {&gsl_sinterp_natural_mesh, MESH, 0, 0, 0},  {&gsl_sinterp_natural_simplex, MESH, 0, 0, 0}, {&gsl_sinterp_cubic_mesh, MESH, 0, 0, 0},
  {&gsl_sinterp_cubic_simplex, MESH, 0, 0, 0},
};

#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d (type %d): %s\n", __LINE__, i, #cond); return 1; } } while (0)

int main(void)
{
  gsl_set_error_handler_off();
  double w[10], c3[3], lo[2] = {0.0, 0.0}, hi[2] = {1.0, 1.0}, g[16], mean;
  gsl_vector_view W = gsl_vector_view_array(w, 10), C3 = gsl_vector_view_array(c3, 3);
  gsl_vector_view LO = gsl_vector_view_array(lo, 2), HI = gsl_vector_view_array(hi, 2);
  gsl_matrix_view G = gsl_matrix_view_array(g, 4, 4);
  int i;
  for (i = 0; i < 16; i++) {
    gsl_sinterp *s = gsl_sinterp_alloc(*types[i].type, 2, 10);
    CHECK(s != NULL);
    CHECK(gsl_sinterp_get_weights(s, &W.vector) == GSL_EINVAL);         /* not an RBF interpolant / not initialised */
    CHECK(gsl_sinterp_eval_grid(s, &LO.vector, &HI.vector, &G.matrix) == GSL_EINVAL);        /* not initialised */
    CHECK(gsl_sinterp_poly(s, &C3.vector) == GSL_EINVAL);               /* affine only / not initialised */
    CHECK(gsl_sinterp_mean(s, &mean) == GSL_EINVAL);                    /* kriging only / not initialised */
    for (int solver = GSL_SINTERP_SOLVER_DEFAULT; solver <= GSL_SINTERP_SOLVER_LU_REFINE; solver++) {
      int want = GSL_SUCCESS;
      if (types[i].family != RBF) want = GSL_EINVAL;                    /* not an RBF interpolant */
      else if ((types[i].krige || types[i].affine) && solver != GSL_SINTERP_SOLVER_DEFAULT) want = GSL_EINVAL;
      else if (types[i].tps && (solver == GSL_SINTERP_SOLVER_CHOLESKY2 || solver == GSL_SINTERP_SOLVER_PCHOLESKY)) want = GSL_EINVAL;
      CHECK(gsl_sinterp_set_solver(s, solver) == want);
    }
    CHECK(gsl_sinterp_set_solver(s, GSL_SINTERP_SOLVER_LU_REFINE + 1) == GSL_EINVAL);        /* unknown solver: every type */
    gsl_sinterp_free(s);
  }
  /* a well-formed type that is not a row of the library's table */
  gsl_sinterp_type foreign = *gsl_sinterp_rbf_gaussian;
  foreign.name = "foreign";
  CHECK(gsl_sinterp_alloc(&foreign, 2, 10) == NULL);
  printf("ok\n");
  return 0;
}
