/* References the tetrahedral-mesh prototypes of include/gsl_sinterp.h and include/gsl_sinterp_hip.h with their declared types,
   and calls the entries that answer without a GPU: the host import in 3-D (validation, links by face matching, convexity,
   checkpoint) and the argument errors of the raw device entries. */
#include <gsl_sinterp.h>
#include <stdio.h>
#include <string.h>

static simplex_mesh *(*const p_import)(const gsl_matrix *, size_t, const int *, const int *, size_t) = &simplex_mesh_import_nd;
static size_t (*const p_dim)(const simplex_mesh *) = &simplex_mesh_dim;
static int (*const p_pack)(gsl_sinterp_hip_ctx *, int, const int *, const int *, int, const double *, const double *, int, void *, int *) =
    &gsl_sinterp_hip_mesh3_pack;
static int (*const p_bind)(gsl_sinterp_hip_ctx *, int, const int *, int, const double *, void *) = &gsl_sinterp_hip_mesh3_bind;
static int (*const p_eval)(gsl_sinterp_hip_ctx *, int, const void *, const void *, const int *, int, const double *, int, const double *,
                           size_t, size_t, double *, int *, long long *) = &gsl_sinterp_hip_mesh3_eval;

#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main(void)
{
  gsl_set_error_handler_off();
  /* the unit cube cut into five tetrahedra: a regular one in the middle and four corners */
  double xyz[24];
  for (int v = 0; v < 8; v++) { xyz[3 * v] = 2.0 * (v >> 2); xyz[3 * v + 1] = (v >> 1) & 1; xyz[3 * v + 2] = 4.0 * (v & 1) + 1.0; }
  gsl_matrix_view X = gsl_matrix_view_array(xyz, 8, 3);
  const int tet[20] = {0, 3, 5, 6, 0, 1, 3, 5, 0, 2, 3, 6, 0, 4, 5, 6, 3, 5, 6, 7};
  simplex_mesh *m = p_import(&X.matrix, 3, tet, NULL, 5);
  CHECK(m != NULL && p_dim(m) == 3 && simplex_mesh_n_triangles(m) == 5 && simplex_mesh_n_points(m) == 8);
  CHECK(simplex_mesh_convex(m) == 1 && simplex_mesh_tree_nodes(m) == NULL);
  const int *nb = simplex_mesh_neighbours(m);
  /* the middle tetrahedron touches every corner: the corner without vertex k lies across the face opposite vertex k */
  CHECK(nb[0] == 4 && nb[1] == 3 && nb[2] == 2 && nb[3] == 1);
  for (int t = 1; t < 5; t++) {
    int links = 0;
    for (int k = 0; k < 4; k++) links += nb[4 * t + k] == 0 ? 1 : (nb[4 * t + k] == -1 ? 0 : 100);
    CHECK(links == 1);
  }
  double shift[3], scale[3], lo[3], hi[3];
  simplex_mesh_geometry(m, shift, scale);
  simplex_mesh_bbox(m, lo, hi);
  CHECK(lo[0] == 0.0 && hi[0] == 2.0 && lo[2] == 1.0 && hi[2] == 5.0 && shift[1] == 0.5 && shift[2] == 3.0);
  CHECK(scale[0] == 0.5 && scale[1] == 1.0 && scale[2] == 0.25);
  CHECK(simplex_mesh_points(m)[3 * 7 + 2] == 5.0);
  simplex_mesh *again = p_import(&X.matrix, 3, tet, nb, 5);                     /* the derived links pass the validation */
  CHECK(again != NULL);
  simplex_mesh_free(again);
  FILE *fp = tmpfile();
  CHECK(fp != NULL && simplex_mesh_fwrite(fp, m) == GSL_SUCCESS);
  rewind(fp);
  char magic[8];
  CHECK(fread(magic, 1, 8, fp) == 8 && memcmp(magic, "GSLSMSH2", 8) == 0);
  rewind(fp);
  simplex_mesh *r = simplex_mesh_fread(fp);
  fclose(fp);
  CHECK(r != NULL && p_dim(r) == 3 && simplex_mesh_n_triangles(r) == 5 && simplex_mesh_convex(r) == 1);
  CHECK(memcmp(simplex_mesh_neighbours(r), nb, 20 * sizeof(int)) == 0 && memcmp(simplex_mesh_triangles(r), tet, sizeof tet) == 0);
  simplex_mesh_free(r);
  simplex_mesh_free(m);
  CHECK(p_import(&X.matrix, 4, tet, NULL, 4) == NULL);                          /* GSL_EUNIMPL */
  CHECK(p_import(NULL, 3, tet, NULL, 5) == NULL);
  const int own[4] = {0, 1, 1, 3};
  CHECK(p_import(&X.matrix, 3, own, NULL, 1) == NULL);                          /* repeated vertex */
  /* the facade: dim 2 and 3, nothing else */
  gsl_sinterp *s3 = gsl_sinterp_alloc(gsl_sinterp_linear_mesh, 3, 8);
  CHECK(s3 != NULL && gsl_sinterp_alloc(gsl_sinterp_linear_mesh, 4, 8) == NULL && gsl_sinterp_alloc(gsl_sinterp_linear_mesh, 1, 8) == NULL);
  double ff[8] = {0};
  gsl_vector_view F = gsl_vector_view_array(ff, 8);
  CHECK(gsl_sinterp_init(s3, &X.matrix, &F.vector) == GSL_EINVAL);             /* no triangulation set */
  CHECK(gsl_sinterp_set_triangulation(s3, tet, NULL, 5) == GSL_SUCCESS);
  gsl_sinterp_free(s3);
  /* raw device entries: argument errors come before any device work */
  CHECK(p_pack(NULL, 5, NULL, NULL, 8, NULL, NULL, 2, NULL, NULL) == GSL_EFAULT);
  CHECK(p_bind(NULL, 5, NULL, 8, NULL, NULL) == GSL_EFAULT);
  CHECK(p_eval(NULL, 5, NULL, NULL, NULL, 2, NULL, 1, NULL, 0, 3, NULL, NULL, NULL) == GSL_EFAULT);
  printf("ok\n");
  return 0;
}
