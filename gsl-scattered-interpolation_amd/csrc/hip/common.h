/*
 * common.h -- shared by the HIP translation units behind include/gsl_sinterp_hip.h.
 */
#ifndef SINTERP_HIP_COMMON_H
#define SINTERP_HIP_COMMON_H

#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "gsl_sinterp_hip.h"

/* GSL status codes used here (include/gsl_sinterp_compat.h, err/gsl_errno.h:40-74) */
enum { ST_SUCCESS = 0, ST_FAILURE = -1, ST_EDOM = 1, ST_EFAULT = 3, ST_EINVAL = 4, ST_EFAILED = 5, ST_ENOMEM = 8,
       ST_EBADLEN = 19 };

struct gsl_sinterp_hip_ctx {
  int device;
  hipStream_t stream;
  int owns_stream;
  hipEvent_t ev0, ev1;
  void *d_scratch;          /* small persistent scratch: counters / info words */
  size_t scratch_bytes;
  void *d_work;             /* growable workspace (factorisations) */
  size_t work_bytes;
  void *d_aux;              /* growable buffer of the solver route (right-hand sides, polynomial block) */
  size_t aux_bytes;
  void *d_inv;              /* inverted 64x64 diagonal blocks of the triangular sweeps */
  size_t inv_bytes;
  void *d_sort;             /* target permutation / reordered targets + cell counters of ONE batch (sort.hip) */
  size_t sort_bytes;
  void *d_sort2;            /* the same for the centres of the Gaussian sweep */
  size_t sort2_bytes;
  void *d_cent;             /* cell-ordered packed centres {x, w} + tile boxes of the Gaussian sweep */
  size_t cent_bytes;
  /* key of the packed centres currently in d_cent (gsl_sinterp_hip_rbf_eval_model); id 0 = nothing cached */
  struct CentKey { unsigned long long id; const void *x, *w; size_t n, xtda, ldw; int dim, kind, nf; } cent_key;   /* scalar: nf = 0, ldw = 0 */
  /* the fields sweep's records {x, w_0 .. w_{K-1}} have a slot of their own (a K-field model and its field 0 used as a
     scalar model share id, x and w: one slot would be repacked at every change of entry); nf and ldw tell its keys apart */
  void *d_cent_f;
  size_t cent_f_bytes;
  CentKey cent_key_f;
  /* local kriging (local.hip): the centres binned on a uniform grid and gathered into cell order as records
     {x, f, index}, [256 B head | cell offsets | records]; keyed like d_cent (w = the responses), local_g cells per axis;
     local_packs counts the packs of this context (gsl_sinterp_hip_local_pack_count) */
  void *d_local;
  size_t local_bytes;
  CentKey local_key;
  int local_g;
  unsigned long long local_packs;
  void *d_walk;             /* queue counter + queue of a located sweep, then the barycentric DAG walk's records and lists
                               (bary.hip: WalkLayout), rebuilt per batch */
  size_t walk_bytes;
  hipStream_t side_stream;  /* bary.hip: independent kernels of one evaluation run beside the main stream */
  hipEvent_t side_ev[4];    /* fork / join events of the side stream (created with the stream) */
  /* hipGraph cache: the recursive factorisation drivers issue ~1-2k small, fully static
     launches; they are captured once per (routine, arguments) and replayed.  The key holds every
     argument baked into the captured kernels, one word each (no folding: two different argument
     sets must never compare equal), plus the workspace pointer the graph was captured with. */
  hipStream_t cap_stream;
  enum { GRAPH_KEY_WORDS = 12 };
  struct GraphSlot { hipGraphExec_t exec; uintptr_t key[GRAPH_KEY_WORDS]; } graph[4];
  int use_graphs;
  /* stream-K GEMM (gemm.hip): one partial-tile slot + one flag per persistent workgroup */
  double *d_sk_partial;
  unsigned *d_sk_flags;
  int sk_wgs;               /* persistent workgroups = CUs of the device; 0 = not prepared */
  int chol_riders;          /* diagonal-block riders attached by the factorisation recorded in graph slot 0 (chol.hip) */
  /* dataflow sweeps (chol.hip): [0] = epoch of the last completed sweep, [1 + J] = epoch in which
     block J was last published.  Never reset (no memset node in the captured graphs): a sweep
     publishes with epoch + 1 and its last block advances the epoch. */
  unsigned *d_tf;
  size_t tf_count;
  unsigned long long *d_xq; /* hand-off buffer of the sweeps: per entry {epoch|lo32}, {epoch|hi32} */
  void *d_lu_coop;          /* cooperative LU panel: [generation, abort] + exchange slots (lu.hip) */
  /* jump table of the barycentric walk built by tree_pack over the data's bounding box (bary.hip):
     [64 B box keys][G*G node indices]; valid for records == jump_rec with jump_nodes nodes */
  void *d_jumpt;
  size_t jumpt_bytes;
  /* leaf-adjacency locator of the barycentric sweep (bary.hip, "Certified leaf walk"): seed grid + per-leaf line lists of the
     final edges and of the historic (flipped-away) edges that cross the leaf, valid for records == lw_rec */
  void *d_lw_a;             /* [64 B consts][seed Gs^2][off n_nodes + 1 + scan scratch] */
  void *d_lw_lines;         /* 3 doubles per line */
  size_t lw_a_bytes, lw_lines_bytes;
  const void *lw_rec;
  int lw_nodes, lw_Gs, lw_last;   /* lw_last: the last large batch went through the leaf walk */
  double lw_c[2], lw_lo[2], lw_w[2];
  const void *jump_rec;
  int jump_nodes, jump_G;
  int excl_depth;           /* nesting of sinterp_exclusive_begin/end */
  char err[512];
  /* modified Shepard (shepard.hip): the nodes binned on the grid of local.hip and gathered into cell order, rows ascending
     inside a cell, [256 B head | cell offsets | cell boxes | rows | records]; keyed like d_local (x = the centres, w = the
     coefficients), shep_g cells per axis; shep_packs / shep_fits count the packs and the fits of this context */
  void *d_shep;
  size_t shep_bytes;
  CentKey shep_key;
  int shep_g;
  unsigned long long shep_packs, shep_fits;
  unsigned long long vg_pairs_tested;   /* variogram.hip: unordered pairs whose r2 the last call computed */
};

/* A cached pack (local.hip, shepard.hip) is reused when the caller vouches for the model (id != 0) and every word that
   describes the cloud matches; setting a key with id 0 records nothing. */
static inline bool sinterp_key_vouches(const gsl_sinterp_hip_ctx::CentKey &key, unsigned long long id, const void *x, const void *w, size_t n,
                                       size_t xtda, int dim)
{
  return id != 0 && key.id == id && key.x == x && key.w == w && key.n == n && key.xtda == xtda && key.dim == dim;
}
static inline void sinterp_key_set(gsl_sinterp_hip_ctx::CentKey &key, unsigned long long id, const void *x, const void *w, size_t n,
                                   size_t xtda, int dim)
{
  if (id != 0) key = gsl_sinterp_hip_ctx::CentKey{id, x, w, n, xtda, 0, dim, 0, 0};
}

/* Graph helpers (shim.hip).  A key is up to GRAPH_KEY_WORDS - 1 argument words (unused words 0); the helpers append
   ctx->d_work.  sinterp_graph_try_launch sets *launched = 1 and launches the cached graph on the context's stream when
   slot `which` holds exactly this key.  Between sinterp_capture_begin / _end every launch on ctx->stream is recorded. */
struct sinterp_graph_key {
  uintptr_t w[gsl_sinterp_hip_ctx::GRAPH_KEY_WORDS - 1];
};
int sinterp_graph_try_launch(gsl_sinterp_hip_ctx *ctx, int which, const sinterp_graph_key &key, int *launched);
int sinterp_capture_begin(gsl_sinterp_hip_ctx *ctx, hipStream_t *saved);
int sinterp_capture_end(gsl_sinterp_hip_ctx *ctx, hipStream_t saved, int which, const sinterp_graph_key &key);

static inline int sinterp_fail(gsl_sinterp_hip_ctx *ctx, int status, const char *what, hipError_t e,
                               const char *file, int line)
{
  if (ctx)
    snprintf(ctx->err, sizeof ctx->err, "%s: %s (%s:%d)", what, e == hipSuccess ? "invalid argument" : hipGetErrorString(e),
             file, line);
  return status;
}

#define HIP_OK(ctx, call)                                                               \
  do {                                                                                  \
    hipError_t _e = (call);                                                             \
    if (_e != hipSuccess)                                                               \
      return sinterp_fail(ctx, _e == hipErrorOutOfMemory ? ST_ENOMEM : ST_EFAILED, #call, _e, __FILE__, __LINE__); \
  } while (0)

#define REQUIRE(ctx, cond, status)                                                      \
  do {                                                                                  \
    if (!(cond)) return sinterp_fail(ctx, status, "requirement failed: " #cond, hipSuccess, __FILE__, __LINE__); \
  } while (0)

#define LAUNCH_CHECK(ctx) HIP_OK(ctx, hipGetLastError())

static inline size_t round_up(size_t v, size_t to) { return (v + to - 1) / to * to; }

/* The GSL_SINTERP_* switches.  A flag is on iff its value begins with '1'.  These three read
   the environment at every call -- for the switches that tests flip inside one process; SINTERP_ENV_ONCE is the flag
   read once per process, the first time control reaches the site (a static of its own per site). */
static inline bool sinterp_env_flag(const char *name) { const char *v = getenv(name); return v && v[0] == '1'; }
static inline int sinterp_env_int(const char *name, int dflt) { const char *v = getenv(name); return v ? atoi(v) : dflt; }
static inline double sinterp_env_double(const char *name, double dflt) { const char *v = getenv(name); return v ? atof(v) : dflt; }
#define SINTERP_ENV_ONCE(name) ([] { static const bool on = sinterp_env_flag(name); return on; }())

/* hipFuncAttributeMaxDynamicSharedMemorySize is a PER-DEVICE attribute of a kernel: set it once per
   (kernel, device) pair (a process-wide flag would leave the second device of a process without it) */
int sinterp_func_lds(gsl_sinterp_hip_ctx *ctx, const void *func, int bytes);

/* Kernels that spin on other workgroups of their own launch (stream-K fix-up, dataflow sweeps, the
   cooperative LU panel) need all their workgroups co-resident; two of them running at once on one
   device (two contexts / streams) could each hold CUs while waiting for workgroups that cannot be
   scheduled.  Every entry point that launches such kernels brackets its launches with these: a
   process-wide per-device event chain orders the exclusive sections of ALL contexts of that device
   one after another on the GPU (nestable; the outermost pair does the work). */
int sinterp_exclusive_begin(gsl_sinterp_hip_ctx *ctx);
int sinterp_exclusive_end(gsl_sinterp_hip_ctx *ctx);

struct SinterpExclusive {      /* RAII form: every return path of an entry point leaves the section */
  gsl_sinterp_hip_ctx *ctx;
  int st;
  explicit SinterpExclusive(gsl_sinterp_hip_ctx *c) : ctx(c), st(sinterp_exclusive_begin(c)) {}
  ~SinterpExclusive() { if (st == ST_SUCCESS) (void)sinterp_exclusive_end(ctx); }
  SinterpExclusive(const SinterpExclusive &) = delete;
  SinterpExclusive &operator=(const SinterpExclusive &) = delete;
};
#define EXCLUSIVE_SECTION(ctx) SinterpExclusive _excl(ctx); if (_excl.st) return _excl.st

/* rbf.hip: the fill with the option of writing the tiles on / below the diagonal only */
int sinterp_rbf_fill_ex(gsl_sinterp_hip_ctx *ctx, int kind, double eps, const double *d_x, size_t n, int dim, size_t xtda,
                        double *d_phi, size_t lda, int lower_only);
int sinterp_tps_fill_shifted(gsl_sinterp_hip_ctx *ctx, const double *d_x, size_t n, int dim, size_t xtda, double *d_phi, size_t lda,
                             const double *d_Pk, int k, double cmul, unsigned long long *d_norm);

/* rbf.hip: device address of the 256-entry exp2 table that rbf_phi.h's exp2_tbl reads (built on first use) */
int sinterp_rbf_exp2_table(gsl_sinterp_hip_ctx *ctx, const double **d_tbl);

/* grow-only workspace owned by the context */
int sinterp_workspace(gsl_sinterp_hip_ctx *ctx, size_t bytes, void **out);

/* dense building blocks shared by the Cholesky and LU drivers (gemm.hip) */
/* C[m x n] -= A[m x k] * B^T   with B stored [n][k] (ldb)         -> b_is_kn = 0
   C[m x n] -= A[m x k] * B     with B stored [k][n] (ldb)         -> b_is_kn = 1
   lower_only: C is square on the diagonal, tiles strictly above it are skipped */
/* rider (optional, the Cholesky driver's trailing updates): one extra workgroup of the update's launch factors
   C[0:128, 0:128] -- the next panel's diagonal block -- as soon as the tiles that cover it are stored, doing what
   chol_diag128_kernel does (chol_potrf.h: chol_diag128_block).  It is attached only on the N.T stream-K path; *attached
   tells the caller whether its leaf may skip the launch of its own. */
struct sinterp_rider {
  int *info;                /* pivot status word of the factorisation */
  size_t j0;                /* first column of the block in the whole matrix */
  double *dinv;             /* receives the four inverted 32 x 32 diagonal blocks */
  double *fb; size_t ldf; int nrhs;   /* right-hand sides of the folded forward substitution (nrhs = 0: none) */
  unsigned *counter;        /* this panel's arrival counter, zero at launch: the owners of the covering tiles add to it */
  unsigned *abort_word;     /* set (and left set) when the rider gave up waiting */
};
int sinterp_gemm_minus(gsl_sinterp_hip_ctx *ctx, size_t m, size_t n, size_t k, const double *A, size_t lda,
                       const double *B, size_t ldb, int b_is_kn, double *C, size_t ldc, int lower_only,
                       const sinterp_rider *rider = NULL, int *attached = NULL);

/* allocates the stream-K buffers of the context; must be called OUTSIDE stream capture (the
   factorisation drivers call it before they start capturing).  Without it the GEMM falls back to
   the one-tile-per-workgroup kernels. */
int sinterp_streamk_prepare(gsl_sinterp_hip_ctx *ctx);

/* blocked triangular sweeps (chol.hip): the block being solved is read from b and
   written to xout (b != xout), the remaining right-hand side is updated in b.
   mode 0 Lower/NoTrans fwd, 1 Lower/Trans bwd, 2 Upper/NoTrans bwd */
int sinterp_trsv(gsl_sinterp_hip_ctx *ctx, size_t n, const double *T, size_t ldt, double *b, double *xout, int mode,
                 int unit);
/* the same for nrhs <= 5 right-hand sides stored at b + r*ldb / xout + r*ldb */
int sinterp_trsv_multi(gsl_sinterp_hip_ctx *ctx, size_t n, const double *T, size_t ldt, double *b, double *xout, size_t ldb,
                       int nrhs, int mode, int unit);
int sinterp_cholesky_svx_multi(gsl_sinterp_hip_ctx *ctx, size_t n, const double *d_llt, size_t lda, double *d_x, size_t ldx,
                               int nrhs);
/* gsl_sinterp_hip_cholesky_decomp1 for an input that is stored symmetrically (both triangles valid) */
int sinterp_cholesky_decomp1_sym(gsl_sinterp_hip_ctx *ctx, size_t n, double *d_a, size_t lda, int *h_info);
/* the same followed by the solve of nrhs right-hand sides in place (forward substitution folded into the factorisation when every panel is 128 wide) */
int sinterp_cholesky_factor_solve_sym(gsl_sinterp_hip_ctx *ctx, size_t n, double *d_a, size_t lda, int *h_info, double *d_x, size_t ldx,
                                      int nrhs);
/* the same for ANY number of right-hand sides: the first min(nrhs, 5) ride the factorisation as above, the rest are solved
   against the finished factor in groups of <= 5 (sinterp_cholesky_svx_multi) */
int sinterp_cholesky_factor_solve_many_sym(gsl_sinterp_hip_ctx *ctx, size_t n, double *d_a, size_t lda, int *h_info, double *d_x,
                                           size_t ldx, int nrhs);
/* krige_var.hip: the pieces of the blocked substitution Z <- Z L^-T that the kriging variance and the leave-one-out
   diagonal (loo.hip) share.  One pass works on rows_pad rows (a multiple of 128) of the work matrix Z (pitch ldw = n
   rounded up to 128, 16-byte aligned) against the lower triangle of L; q receives the squared row norms. */
struct KvPass {
  gsl_sinterp_hip_ctx *ctx;
  double *Z; size_t ldw, rows_pad;
  const double *L; size_t lda, n;
  const double *dinv;
  double *q;
};
/* Z[:, c0 : c0 + cw] -= Z[:, k0 : k0 + kw] L[c0 : c0 + cw, k0 : k0 + kw]^T (a partial last block in a call of its own) */
int sinterp_kv_update(const KvPass &p, size_t c0, size_t cw, size_t k0, size_t kw);
/* Z[:, j0 : j0 + 128] <- Z[:, j0 : j0 + 128] L_JJ^-T and q_k += |Z[k][j0 : j0 + 128]|^2 (krige_trsm128_kernel) */
int sinterp_kv_diag(const KvPass &p, size_t j0);
/* the fill Z[k][j] = phi(|y_k - x_j|) of rows_pad rows (a multiple of 16; rows >= rows and columns >= n are zeros; clears
   q) for a run-time positive definite kind, and the whole substitution Z <- Z L^-T of one pass at the default panel:
   what the joint covariance (krige_cov.hip) takes over from the variance entries */
int sinterp_kv_cross_fill(gsl_sinterp_hip_ctx *ctx, int kind, double coef, const double *tbl, const double *d_x, size_t n, int dim,
                          size_t xtda, const double *d_y, size_t rows, size_t ytda, double *Z, size_t ldw, size_t rows_pad, double *q);
int sinterp_kv_solve(const KvPass &p);
/* inverse of every 32 x 32 diagonal block of L -> d_dinv[ceil(n / 32) * 1024] (krige_inv32_kernel) */
int sinterp_krige_inv32(gsl_sinterp_hip_ctx *ctx, size_t n, const double *d_llt, size_t lda, double *d_dinv);
/* drift.hip: the launchers behind the universal-kriging entries of solve.hip and krige_var.hip (order 1 or 2, arguments
   checked by the callers).  basis: column t of P at d_P + t * ldp.  gram: d_G[a * ncols + b] = sum_i P_a[i] Y_b[i], a < q,
   b < ncols, fixed summation order.  var_combine: d_var[k] = (1 - d_q[k]) + |Ls^-1 (p(u(y_k)) - d_bk[k * q ..])|^2, h_L = the
   q x q row-major factor of gsl_sinterp_hip_drift_factor.  cov_terms (order 0 .. 2; order 0 = ordinary kriging: p = 1, q = 1,
   h_L = {sqrt(1^T b)}, h_shift / h_scale not read): row k of d_bk, B^T k(y_k) on entry, becomes t_k = Ls^-1 (p(u(y_k)) - B^T k(y_k)). */
int sinterp_drift_basis(gsl_sinterp_hip_ctx *ctx, int order, const double *h_shift, const double *h_scale, const double *d_x, size_t n,
                        int dim, size_t xtda, double *d_P, size_t ldp);
int sinterp_drift_gram(gsl_sinterp_hip_ctx *ctx, const double *d_P, size_t ldp, const double *d_Y, size_t ldy, size_t n, int q, int ncols,
                       double *d_G);
int sinterp_drift_var_combine(gsl_sinterp_hip_ctx *ctx, int order, const double *h_shift, const double *h_scale, const double *h_L, int dim,
                              const double *d_y, size_t rows, size_t ytda, const double *d_bk, const double *d_q, double *d_var);
int sinterp_drift_cov_terms(gsl_sinterp_hip_ctx *ctx, int order, const double *h_shift, const double *h_scale, const double *h_L, int dim,
                            const double *d_y, size_t rows, size_t ytda, double *d_bk);
/* second grow-only buffer for vectors that must outlive factorisation workspaces */
int sinterp_aux(gsl_sinterp_hip_ctx *ctx, size_t bytes, void **out);
int sinterp_invbuf(gsl_sinterp_hip_ctx *ctx, size_t bytes, void **out);
int sinterp_sortbuf(gsl_sinterp_hip_ctx *ctx, size_t bytes, void **out);
/* sort.hip: permutation that groups the targets by cell of a uniform grid (~per_cell each) */
int sinterp_sort_targets(gsl_sinterp_hip_ctx *ctx, const double *d_y, size_t m, size_t ytda, int dim, int per_cell,
                         int **d_perm_out);
/* The same sort, but the targets are physically gathered into cell order (dense [m][dim]) and the
   results come back through sinterp_unsort: the sweep kernels then read and write contiguously, the
   only scattered accesses are one 8*dim-byte write per target here and one 8(+4)-byte READ per target in
   the un-sort (a permutation-indirect kernel pays a scattered read AND partial-sector scattered writes).
   The arrays live in the context's sort buffer, laid out for this batch alone: they are valid until the next sort on
   the context. */
struct sinterp_sorted {
  double *ys;                   /* [m][dim] targets in cell order */
  double *vs;                   /* [m] values in cell order (filled by the sweep); room for [m] {value, leaf} pairs */
  int *ls;                      /* [m] leaf indices in cell order (barycentric sweep) */
  unsigned *cellid, *slot, *offset;
  unsigned long long *box;      /* bounding-box keys, box[2c] = min, box[2c+1] = max */
  bool two_level;               /* large batches (sort.hip, "two-level reorder"): slot[k] = position of target k in the coarse order; */
  unsigned *inv;                /*   inv[p] = coarse position of the target at cell-order position p: the sweep stores the result of */
  double *res1;                 /*   sorted target p at res1[inv[p]] (8 bytes, or a {value, leaf} pair), NOT at vs[p]; */
  unsigned *fin;                /*   (internal: slots of the out-of-window points between the two fine passes) */
  unsigned *tl_cnt; unsigned tl_nb, tl_nwg, tl_ch;   /* (internal: first coarse position of every (bin, workgroup) run, for the staged un-sort) */
};
int sinterp_sort_reorder(gsl_sinterp_hip_ctx *ctx, const double *d_y, size_t m, size_t ytda, int dim, int per_cell,
                         sinterp_sorted *out, const unsigned long long *box_in);
/* whether a batch of m targets takes the two-level route (results through inv / res1) */
bool sinterp_sort_reorder_is_two_level(size_t m);
int sinterp_unsort(gsl_sinterp_hip_ctx *ctx, const sinterp_sorted *s, size_t m, double *d_values, int *d_leaf);
/* vs holds {value, leaf-as-integer-bits} pairs (16 bytes per target; the vs region is sized for it) */
int sinterp_unsort_packed(gsl_sinterp_hip_ctx *ctx, const sinterp_sorted *s, size_t m, double *d_values, int *d_leaf);

/* the centres: cells visited in Morton order (consecutive runs are spatially compact), original
   index order inside a cell (deterministic summation order); uses its own buffer */
int sinterp_sort_centres(gsl_sinterp_hip_ctx *ctx, const double *d_x, size_t n, size_t xtda, int dim, int per_cell,
                         int **d_perm_out);
int sinterp_sortbuf2(gsl_sinterp_hip_ctx *ctx, size_t bytes, void **out);
/* exclusive scan of count[0..n) in place, total in count[n]; runsum: n/1024 + 2 entries of scratch (sort.hip) */
void sinterp_scan_u32(gsl_sinterp_hip_ctx *ctx, unsigned *count, size_t n, unsigned *runsum);
int sinterp_walkbuf(gsl_sinterp_hip_ctx *ctx, size_t bytes, void **out);

#define MESH_GAP 1e-9   /* imported meshes (bary.hip, mesh3.hip): a target within this much (standardised barycentric units) of a
                           simplex that no simplex contains under the floating-point closed test is given to the least violating one */

/* packed & 1: values is an array of {value, leaf} pairs (16 bytes, one store here and ONE gather per target in the
   un-sort pass instead of two).  packed & 2 (two-level reorder, sort.hip): leaf_out is not a leaf array but the map
   from the position in cell order to the position in the coarse order, where the result is stored. */
__device__ __forceinline__ void store_result(double *__restrict__ values, int *__restrict__ leaf_out, size_t k, double v, int leaf,
                                             int packed)
{
  if (packed & 2) {
    k = reinterpret_cast<const unsigned *>(leaf_out)[k];
    leaf_out = NULL;
  }
  if (packed & 1) {
    *reinterpret_cast<double2 *>(values + 2 * k) = make_double2(v, __longlong_as_double((long long)leaf));
  } else {
    values[k] = v;
    if (leaf_out) leaf_out[k] = leaf;
  }
}
/* Host side of the same convention (sort.hip): what a located sweep reads and where it stores.  Unsorted: the caller's
   arrays, packed = 0.  Sorted, one level: values = srt.vs, {value, leaf} pairs (bit 0) when a leaf output is wanted, no
   leaf array.  Sorted, two levels: values = srt.res1, leaf = srt.inv reinterpreted (bit 1), pairs likewise. */
struct sinterp_route {
  const double *y; size_t ytda;   /* the targets as the kernels see them */
  double *values; int *leaf;      /* store_result's arguments ... */
  int packed;                     /* ... and its mode */
  bool sorted; sinterp_sorted srt;
};
/* the batch size from which a located sweep reorders its targets, unless GSL_SINTERP_NO_SORT=1 (read per call) */
bool sinterp_sort_wanted(size_t m);
int sinterp_route_begin(gsl_sinterp_hip_ctx *ctx, const double *d_targets, size_t m, size_t ttda, int dim, int per_cell,
                        const unsigned long long *box_in, double *d_values, int *d_leaf, bool sort, sinterp_route *r);
/* the un-sort that matches r->packed into the caller's arrays, or nothing */
int sinterp_route_end(gsl_sinterp_hip_ctx *ctx, const sinterp_route *r, size_t m, double *d_values, int *d_leaf);
/* h_n_outside != NULL: waits for the stream, *h_n_outside = *d_count, and ST_EDOM with the message `what` when it is not 0 */
int sinterp_outside_count(gsl_sinterp_hip_ctx *ctx, const unsigned long long *d_count, long long *h_n_outside, const char *what);
/* sort.hip: bounding box of n points as order-preserving keys, box[2c] = min, box[2c+1] = max (device, 48 bytes) */
int sinterp_bbox_keys(gsl_sinterp_hip_ctx *ctx, const double *d_p, size_t n, size_t tda, int dim, unsigned long long *d_box);
/* local.hip: the n points of d_x binned on the g^dim grid over their bounding box (local_grid.h).  d_grid receives the
   box, d_box its keys (48 bytes), d_off[cell] the first place of the cell in cell order and d_off[ncell] = n (room for
   lk_off_words(ncell) words: the scan's scratch follows), d_cellid[i] the cell of point i and d_slot[i] its place inside
   the cell, in the order the atomics hand out. */
struct LkGrid;
int sinterp_grid_bin(gsl_sinterp_hip_ctx *ctx, const double *d_x, size_t n, int dim, size_t xtda, int g, LkGrid *d_grid,
                     unsigned long long *d_box, unsigned *d_off, unsigned *d_cellid, unsigned *d_slot);
int sinterp_centbuf(gsl_sinterp_hip_ctx *ctx, size_t bytes, void **out);
int sinterp_centbuf_fields(gsl_sinterp_hip_ctx *ctx, size_t bytes, void **out);
int sinterp_localbuf(gsl_sinterp_hip_ctx *ctx, size_t bytes, void **out);
int sinterp_shepbuf(gsl_sinterp_hip_ctx *ctx, size_t bytes, void **out);

#endif
