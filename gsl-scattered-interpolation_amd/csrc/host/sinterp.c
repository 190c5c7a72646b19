/*
 * sinterp.c -- (a) the batched GPU entry over a host-built simplex_tree
 * (simplex_tree_device_*) and (b) the gsl_sinterp facade.
 *
 * The facade follows the alloc / init / eval_e / eval / free convention of
 * gsl_interp (interpolation/gsl_interp.h:49-71; interpolation/interp.c:30-138):
 * alloc checks min_size (GSL_EINVAL) and allocation (GSL_ENOMEM), init
 * validates sizes, eval_e writes *s and returns a status (out of domain ->
 * NaN + GSL_EDOM, interp.c:131-135), eval raises through the GSL handler,
 * free is NULL-safe (interp.c:114-122).
 *
 * All numerical work is done by the HIP kernels behind include/gsl_sinterp_hip.h.
 * There is deliberately no CPU evaluation path here.
 */
#include "gsl_sinterp.h"
#include <limits.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#define HIP_TRY(call, ctx)                                                         \
  do {                                                                             \
    int _st = (call);                                                              \
    if (_st != GSL_SUCCESS) {                                                      \
      gsl_error(gsl_sinterp_hip_last_error(ctx), __FILE__, __LINE__, _st);         \
      return _st;                                                                  \
    }                                                                              \
  } while (0)

static int default_device(void)
{
  const char *s = getenv("GSL_SINTERP_DEVICE");
  return s ? atoi(s) : 0;
}

/* GSL_SINTERP_DEVICES: "4" = devices 0..3, or an explicit list "0,2,5" (SURVEY.md section 5, config row).
   Returns the number of entries written to list[], 0 when the variable is unset / unusable. */
#define SINTERP_MAX_DEVICES 64
static int env_device_list(int *list)
{
  const char *s = getenv("GSL_SINTERP_DEVICES");
  if (!s || !*s) return 0;
  if (!strchr(s, ',')) {
    int n = atoi(s);
    if (n < 1) return 0;
    if (n > SINTERP_MAX_DEVICES) n = SINTERP_MAX_DEVICES;
    for (int i = 0; i < n; i++) list[i] = i;
    return n;
  }
  int n = 0;
  while (*s && n < SINTERP_MAX_DEVICES) {
    char *end = NULL;
    long v = strtol(s, &end, 10);
    if (end == s) break;
    list[n++] = (int)v;
    s = (*end == ',') ? end + 1 : end;
  }
  return n;
}

/* ======================================================================== */
/* target shards over a device group (one host thread drives every member)   */
/* ======================================================================== */
typedef struct {
  gsl_sinterp_hip_group *grp;
  int n;
  /* grow-only per-member device buffers of a shard: targets, values, leaf indices */
  double *d_y[SINTERP_MAX_DEVICES], *d_s[SINTERP_MAX_DEVICES];
  int *d_leaf[SINTERP_MAX_DEVICES];
  size_t cap[SINTERP_MAX_DEVICES], cap_dim;
  /* pinned host staging for the asynchronous copies */
  void *h_stage;
  size_t h_bytes;
} shard_set;

typedef int (*shard_eval_fn)(void *state, int member, const double *d_y, size_t m, double *d_s, int *d_leaf);

static void shard_set_release(shard_set *ss)
{
  for (int i = 0; i < ss->n; i++) {
    gsl_sinterp_hip_ctx *c = gsl_sinterp_hip_group_ctx(ss->grp, i);
    gsl_sinterp_hip_free(c, ss->d_y[i]); gsl_sinterp_hip_free(c, ss->d_s[i]); gsl_sinterp_hip_free(c, ss->d_leaf[i]);
    ss->d_y[i] = ss->d_s[i] = NULL; ss->d_leaf[i] = NULL; ss->cap[i] = 0;
  }
  gsl_sinterp_hip_host_free(ss->h_stage);
  ss->h_stage = NULL; ss->h_bytes = 0;
  gsl_sinterp_hip_group_destroy(ss->grp);
  ss->grp = NULL; ss->n = 0;
}

/* Evaluate every row of y: member r takes the contiguous shard gsl_sinterp_hip_shard_bounds gives it.
   All H2D copies, sweeps and D2H copies are enqueued before the first synchronisation, so the members
   run concurrently; results come back per shard (no gather collective: each GPU copies its own shard to
   the host).  Returns the number of targets whose leaf came back negative in *n_neg. */
static int shard_eval_many(shard_set *ss, size_t dim, const gsl_matrix *y, gsl_vector *sv, int *leaf,
                           shard_eval_fn fn, void *state, int want_leaf, size_t *n_neg)
{
  const size_t m = y->size1;
  if (n_neg) *n_neg = 0;
  if (m == 0) return GSL_SUCCESS;
  const size_t o_s = m * dim * sizeof(double), o_l = o_s + m * sizeof(double), need = o_l + (want_leaf ? m * sizeof(int) : 0);
  if (need > ss->h_bytes) {
    gsl_sinterp_hip_host_free(ss->h_stage);
    ss->h_stage = NULL; ss->h_bytes = 0;
    if (gsl_sinterp_hip_host_alloc(&ss->h_stage, need) != GSL_SUCCESS) return GSL_ENOMEM;
    ss->h_bytes = need;
  }
  double *h_y = (double *)ss->h_stage, *h_s = (double *)((char *)ss->h_stage + o_s);
  int *h_l = want_leaf ? (int *)((char *)ss->h_stage + o_l) : NULL;
  const int packed = y->tda == dim;

  /* Staging is per shard: member r's rows are repacked (tda -> dim; one memcpy when the caller's matrix is already
     dense) and its H2D -> sweep -> D2H chain is enqueued before shard r+1 is touched, so the host-side repack of the
     later shards runs while the earlier members copy and compute (round 2 repacked all M rows element-wise before
     the first copy was enqueued: tens of ms of serial host time at C4's 160 MB in front of a ~0.2 ms/GPU sweep). */
  int st = GSL_SUCCESS;
  for (int r = 0; r < ss->n && !st; r++) {
    size_t first, cnt;
    gsl_sinterp_hip_shard_bounds(m, ss->n, r, &first, &cnt);
    if (!cnt) continue;
    gsl_sinterp_hip_ctx *c = gsl_sinterp_hip_group_ctx(ss->grp, r);
    if (cnt > ss->cap[r] || dim > ss->cap_dim) {
      gsl_sinterp_hip_free(c, ss->d_y[r]); gsl_sinterp_hip_free(c, ss->d_s[r]); gsl_sinterp_hip_free(c, ss->d_leaf[r]);
      ss->d_y[r] = ss->d_s[r] = NULL; ss->d_leaf[r] = NULL; ss->cap[r] = 0;
      st = gsl_sinterp_hip_malloc(c, (void **)&ss->d_y[r], cnt * 3 * sizeof(double));   /* room for any dim <= 3 */
      if (!st) st = gsl_sinterp_hip_malloc(c, (void **)&ss->d_s[r], cnt * sizeof(double));
      if (!st) st = gsl_sinterp_hip_malloc(c, (void **)&ss->d_leaf[r], cnt * sizeof(int));
      if (st) break;
      ss->cap[r] = cnt; ss->cap_dim = 3;
    }
    if (packed) memcpy(h_y + first * dim, y->data + first * dim, cnt * dim * sizeof(double));
    else
      for (size_t k = first; k < first + cnt; k++)
        for (size_t cc = 0; cc < dim; cc++) h_y[k * dim + cc] = y->data[k * y->tda + cc];
    st = gsl_sinterp_hip_h2d_async(c, ss->d_y[r], h_y + first * dim, cnt * dim * sizeof(double));
    if (!st) st = fn(state, r, ss->d_y[r], cnt, ss->d_s[r], want_leaf ? ss->d_leaf[r] : NULL);
    if (!st) st = gsl_sinterp_hip_d2h_async(c, h_s + first, ss->d_s[r], cnt * sizeof(double));
    if (!st && want_leaf) st = gsl_sinterp_hip_d2h_async(c, h_l + first, ss->d_leaf[r], cnt * sizeof(int));
    if (st) gsl_error(gsl_sinterp_hip_last_error(c), __FILE__, __LINE__, st);
  }
  size_t neg = 0;
  for (int r = 0; r < ss->n; r++) {                      /* always drain every member, also after a failure */
    int s2 = gsl_sinterp_hip_sync(gsl_sinterp_hip_group_ctx(ss->grp, r));
    if (!st && s2) { st = s2; gsl_error(gsl_sinterp_hip_last_error(gsl_sinterp_hip_group_ctx(ss->grp, r)), __FILE__, __LINE__, st); }
    if (st) continue;
    /* member r's shard goes back to the caller while the later members are still running */
    size_t first, cnt;
    gsl_sinterp_hip_shard_bounds(m, ss->n, r, &first, &cnt);
    if (sv->stride == 1) memcpy(sv->data + first, h_s + first, cnt * sizeof(double));
    else for (size_t k = first; k < first + cnt; k++) sv->data[k * sv->stride] = h_s[k];
    if (want_leaf)
      for (size_t k = first; k < first + cnt; k++) { neg += h_l[k] < 0; if (leaf) leaf[k] = h_l[k]; }
  }
  if (st) return st;
  if (n_neg) *n_neg = neg;
  return GSL_SUCCESS;
}

/* ======================================================================== */
/* host batches on ONE device: chunks pipelined over the copy pipe            */
/* ======================================================================== */
/* The facade's host-matrix entries (gsl_sinterp_eval_many, simplex_tree_device_eval_many) used to run
   repack -> hipMalloc -> H2D -> sweep -> D2H -> copy-out strictly in sequence, with pageable staging allocated per call.
   Here a batch is cut into chunks; chunk i is repacked into pinned staging and its H2D -> sweep -> D2H chain enqueued on
   the context's copy pipe (upload stream | context stream | download stream) while the host already repacks chunk i+1,
   so the PCIe directions and the sweep overlap and the per-call allocations are gone (grow-only buffers in the state).
   Results are bit-identical to the one-shot path: a value depends on (model, target) only. */
#define CHUNK_MIN ((size_t)1 << 19)      /* keeps every chunk on the large-batch kernels (two-level reorder from 2^18 targets) */
#define CHUNK_MAX_N 8
typedef struct {
  gsl_sinterp_hip_pipe *pipe;
  void *h_stage;                        /* pinned: targets | values | leaf */
  size_t h_bytes;
  double *d_y, *d_s;
  int *d_leaf;
  size_t cap;                           /* targets the device buffers hold (any dim <= 3) */
} chunk_set;

typedef int (*chunk_eval_fn)(void *state, const double *d_y, size_t m, double *d_s, int *d_leaf);

static void chunk_set_release(chunk_set *cs, gsl_sinterp_hip_ctx *c)
{
  if (cs->pipe) gsl_sinterp_hip_pipe_destroy(cs->pipe);
  cs->pipe = NULL;
  if (c) { gsl_sinterp_hip_free(c, cs->d_y); gsl_sinterp_hip_free(c, cs->d_s); gsl_sinterp_hip_free(c, cs->d_leaf); }
  cs->d_y = cs->d_s = NULL; cs->d_leaf = NULL; cs->cap = 0;
  gsl_sinterp_hip_host_free(cs->h_stage);
  cs->h_stage = NULL; cs->h_bytes = 0;
}

static int chunk_eval_many(chunk_set *cs, gsl_sinterp_hip_ctx *c, size_t dim, const gsl_matrix *y, gsl_vector *sv, int *leaf,
                           chunk_eval_fn fn, void *state, int want_leaf, size_t *n_neg)
{
  const size_t m = y->size1;
  if (n_neg) *n_neg = 0;
  if (m == 0) return GSL_SUCCESS;
  /* Dense caller buffers go over PCIe as they are: measured on the MI355X box (tools/pcie_probe), the runtime moves
     pageable memory at 38 GB/s (H2D) / 56 GB/s (D2H) against 30 / 22 GB/s for a single-threaded memcpy into / out of pinned
     staging -- which would then still have to be copied.  Strided matrices / vectors are repacked through pinned staging. */
  const int y_direct = y->tda == dim, s_direct = sv->stride == 1;
  const int l_down = want_leaf && leaf != NULL;          /* the indices only travel when the caller asked for them, straight into leaf */
  int st = GSL_SUCCESS;
  if (!cs->pipe) st = gsl_sinterp_hip_pipe_create(c, &cs->pipe);
  const size_t b_y = y_direct ? 0 : m * dim * sizeof(double), b_s = s_direct ? 0 : m * sizeof(double), need = b_y + b_s;
  if (!st && need > cs->h_bytes) {
    gsl_sinterp_hip_host_free(cs->h_stage);
    cs->h_stage = NULL; cs->h_bytes = 0;
    st = gsl_sinterp_hip_host_alloc(&cs->h_stage, need);
    if (!st) cs->h_bytes = need;
  }
  if (!st && m > cs->cap) {
    gsl_sinterp_hip_free(c, cs->d_y); gsl_sinterp_hip_free(c, cs->d_s); gsl_sinterp_hip_free(c, cs->d_leaf);
    cs->d_y = cs->d_s = NULL; cs->d_leaf = NULL; cs->cap = 0;
    st = gsl_sinterp_hip_malloc(c, (void **)&cs->d_y, m * 3 * sizeof(double));
    if (!st) st = gsl_sinterp_hip_malloc(c, (void **)&cs->d_s, m * sizeof(double));
    if (!st) st = gsl_sinterp_hip_malloc(c, (void **)&cs->d_leaf, m * sizeof(int));
    if (!st) cs->cap = m;
  }
  if (st) { gsl_error(gsl_sinterp_hip_last_error(c), __FILE__, __LINE__, st); return st; }
  double *h_y = y_direct ? y->data : (double *)cs->h_stage;
  double *h_s = s_direct ? sv->data : (double *)((char *)cs->h_stage + b_y);
  size_t nch = m / CHUNK_MIN;
  if (nch < 1) nch = 1;
  if (nch > CHUNK_MAX_N) nch = CHUNK_MAX_N;
  /* chunk i: [repack] -> H2D -> sweep enqueued; the download of chunk i-1 is enqueued AFTER the sweep of chunk i, so a
     host-blocking copy (pageable memory) waits while the GPU is busy with the next chunk, not in front of it */
  size_t pf = 0, pc = 0;
  int pmark = -1;
  for (size_t ch = 0; ch <= nch && !st; ch++) {
    size_t first = 0, cnt = 0;
    if (ch < nch) gsl_sinterp_hip_shard_bounds(m, (int)nch, (int)ch, &first, &cnt);
    if (cnt) {
      if (!y_direct)
        for (size_t k = first; k < first + cnt; k++)
          for (size_t cc = 0; cc < dim; cc++) h_y[k * dim + cc] = y->data[k * y->tda + cc];
      st = gsl_sinterp_hip_pipe_upload(cs->pipe, cs->d_y + first * dim, h_y + first * dim, cnt * dim * sizeof(double));
      if (!st) st = fn(state, cs->d_y + first * dim, cnt, cs->d_s + first, want_leaf ? cs->d_leaf + first : NULL);
    }
    int mark = -1;
    if (!st && cnt) st = gsl_sinterp_hip_pipe_mark(cs->pipe, &mark);         /* "sweep of this chunk done" */
    if (!st && pc) {
      st = gsl_sinterp_hip_pipe_download(cs->pipe, pmark, h_s + pf, cs->d_s + pf, pc * sizeof(double));
      if (!st && l_down) st = gsl_sinterp_hip_pipe_download(cs->pipe, pmark, leaf + pf, cs->d_leaf + pf, pc * sizeof(int));
    }
    pf = first; pc = cnt; pmark = mark;
  }
  /* the outside-the-cage verdict: counted on the device (one 8-byte read-back, not a host pass over m indices) */
  long long neg = 0;
  if (!st && want_leaf) st = gsl_sinterp_hip_count_negative(c, cs->d_leaf, m, &neg);
  int s2 = gsl_sinterp_hip_pipe_sync(cs->pipe);            /* always drain, also after a failure */
  if (!st) st = s2;
  if (st) { gsl_error(gsl_sinterp_hip_last_error(c), __FILE__, __LINE__, st); return st; }
  if (!s_direct) for (size_t k = 0; k < m; k++) sv->data[k * sv->stride] = h_s[k];
  if (n_neg) *n_neg = (size_t)neg;
  return GSL_SUCCESS;
}

/* ======================================================================== */
/* host batches on ONE device, in one shot: every `_many` entry that is not   */
/* on the chunk pipe (variance, gradient, fields, local kriging, cubic + grad) */
/* ======================================================================== */
/* host_stage_begin repacks the m x dim targets (tda honoured) into pageable memory and uploads them, with room behind
   them for every output of the list; the caller runs its resident entry on hs.d_y and out[i].d; host_stage_end downloads
   each output (straight into a dense destination, through the staging buffer and a scatter into a strided one) and
   frees everything, whatever happened in between.  Allocation per call and
   synchronous copies: these entries are not the throughput path (that is chunk_eval_many). */
typedef struct {
  size_t cols;          /* entries per target, m x cols dense on the device; 0 = not asked for: no room, no download */
  int is_int;           /* the doubles of a list come first (alignment) */
  double *dst;          /* doubles: entry (t, q) goes to dst[t * pitch + q] -- a gsl_vector's stride, a gsl_matrix's tda */
  size_t pitch;
  int *idst;            /* ints: m x cols dense; NULL = wanted on the device only */
  void *d;              /* set by host_stage_begin */
} stage_out;
#define STAGE_VECTOR(v) {(v) ? 1 : 0, 0, (v) ? (v)->data : NULL, (v) ? (v)->stride : 0, NULL, NULL}
#define STAGE_MATRIX(g) {(g)->size2, 0, (g)->data, (g)->tda, NULL, NULL}
#define STAGE_INTS(p, cols) {(cols), 1, NULL, 0, (p), NULL}

typedef struct {
  gsl_sinterp_hip_ctx *c;
  size_t m, in_bytes, out_bytes;
  double *h, *d_y;      /* h == NULL after host_stage_begin: out of host memory */
  stage_out *out;
  int n_out;
} host_stage;

static int host_stage_begin(host_stage *hs, gsl_sinterp_hip_ctx *c, const gsl_matrix *y, size_t dim, stage_out *out, int n_out)
{
  const size_t m = y->size1;
  memset(hs, 0, sizeof *hs);
  hs->c = c; hs->m = m; hs->out = out; hs->n_out = n_out; hs->in_bytes = m * dim * sizeof(double);
  size_t h_bytes = hs->in_bytes;                        /* the targets, later any one strided output */
  for (int i = 0; i < n_out; i++) {
    const size_t b = m * out[i].cols * (out[i].is_int ? sizeof(int) : sizeof(double));
    hs->out_bytes += b;
    if (!out[i].is_int && out[i].pitch != out[i].cols && b > h_bytes) h_bytes = b;
  }
  hs->h = (double *)malloc(h_bytes);
  if (!hs->h) return GSL_ENOMEM;
  for (size_t t = 0; t < m; t++)
    for (size_t a = 0; a < dim; a++) hs->h[t * dim + a] = y->data[t * y->tda + a];
  int s = gsl_sinterp_hip_malloc(c, (void **)&hs->d_y, hs->in_bytes + hs->out_bytes);
  if (s) return s;
  char *p = (char *)hs->d_y + hs->in_bytes;
  for (int i = 0; i < n_out; i++)
    if (out[i].cols) { out[i].d = p; p += m * out[i].cols * (out[i].is_int ? sizeof(int) : sizeof(double)); }
  return gsl_sinterp_hip_h2d(c, hs->d_y, hs->h, hs->in_bytes);
}

/* st: what happened so far (nothing is downloaded after a failure, nor without `download`); returns st, or the copy's */
static int host_stage_end(host_stage *hs, int st, int download)
{
  for (int i = 0; i < hs->n_out && !st && download; i++) {
    const stage_out *o = &hs->out[i];
    const size_t cnt = hs->m * o->cols;
    if (!cnt || (o->is_int && !o->idst)) continue;
    if (o->is_int) st = gsl_sinterp_hip_d2h(hs->c, o->idst, o->d, cnt * sizeof(int));
    else if (o->pitch == o->cols) st = gsl_sinterp_hip_d2h(hs->c, o->dst, o->d, cnt * sizeof(double));      /* dense: in place */
    else {
      st = gsl_sinterp_hip_d2h(hs->c, hs->h, o->d, cnt * sizeof(double));
      for (size_t t = 0; t < hs->m && !st; t++)
        for (size_t q = 0; q < o->cols; q++) o->dst[t * o->pitch + q] = hs->h[t * o->cols + q];
    }
  }
  gsl_sinterp_hip_free(hs->c, hs->d_y);
  free(hs->h);
  return st;
}

/* ======================================================================== */
/* several responses on a mirror (csrc/hip/linear_fields.hip): what the tree  */
/* and the mesh mirror share                                                  */
/* ======================================================================== */
/* the binding of set_responses on member 0 and the scratch of a fields batch: the values the locate writes (dropped) and,
   for a caller that keeps none, its simplex indices; grow-only */
typedef struct {
  double *d_F;                          /* n_points x nf, dense, in the vertex order of the mirror's ids */
  size_t nf, f_doubles;
  double *d_val;
  int *d_leaf;
  size_t cap;
  int tab_defined;                      /* the response table the locate reads holds defined bytes (zeros, or a response) */
} fields_set;

static void fields_set_release(fields_set *fs, gsl_sinterp_hip_ctx *c)
{
  if (c) { gsl_sinterp_hip_free(c, fs->d_F); gsl_sinterp_hip_free(c, fs->d_val); gsl_sinterp_hip_free(c, fs->d_leaf); }
  memset(fs, 0, sizeof *fs);
}

/* h: np x K dense, already in the mirror's vertex order.  The locate reads the scalar binding's response table whatever
   it holds (its values are dropped); a mirror that never had set_response gets a table of zeros once, so that no
   evaluation reads bytes nobody wrote.  response_bound is not touched: the scalar entries still ask for set_response. */
static int fields_bind(fields_set *fs, gsl_sinterp_hip_ctx *c, const double *h, size_t np, size_t K, int response_bound, void *d_tab,
                       size_t tab_bytes)
{
  int st = GSL_SUCCESS;
  const size_t cnt = (np > 0 ? np : 1) * K;
  if (cnt != fs->f_doubles) {
    gsl_sinterp_hip_free(c, fs->d_F); fs->d_F = NULL; fs->f_doubles = 0; fs->nf = 0;
    st = gsl_sinterp_hip_malloc(c, (void **)&fs->d_F, cnt * sizeof(double));
    if (!st) fs->f_doubles = cnt;
  }
  if (!st && np > 0) st = gsl_sinterp_hip_h2d(c, fs->d_F, h, np * K * sizeof(double));
  if (!st && !response_bound && !fs->tab_defined) {
    void *z = calloc(1, tab_bytes);
    if (!z) return GSL_ENOMEM;
    st = gsl_sinterp_hip_h2d(c, d_tab, z, tab_bytes);
    free(z);
  }
  if (!st) st = gsl_sinterp_hip_sync(c);
  if (!st) { fs->nf = K; fs->tab_defined = 1; } else fs->nf = 0;
  return st;
}

static int fields_scratch(fields_set *fs, gsl_sinterp_hip_ctx *c, size_t m)
{
  if (m <= fs->cap) return GSL_SUCCESS;
  gsl_sinterp_hip_free(c, fs->d_val); gsl_sinterp_hip_free(c, fs->d_leaf);
  fs->d_val = NULL; fs->d_leaf = NULL; fs->cap = 0;
  int st = gsl_sinterp_hip_malloc(c, (void **)&fs->d_val, m * sizeof(double));
  if (!st) st = gsl_sinterp_hip_malloc(c, (void **)&fs->d_leaf, m * sizeof(int));
  if (!st) fs->cap = m;
  return st;
}

/* the host batch of both mirrors: shapes, one-shot staging, the resident entry `fn`, the outside count.  A batch with a
   target outside is downloaded whole (NaN rows, index -1) before GSL_EDOM is raised. */
typedef int (*fields_resident_fn)(void *dev, const double *d_y, size_t m, size_t ytda, double *d_S, size_t stda, double *d_G, size_t gtda,
                                  int *d_leaf);
static int fields_eval_host(gsl_sinterp_hip_ctx *c, size_t dim, size_t K, const gsl_matrix *targets, gsl_matrix *S, gsl_matrix *G, int *leaf,
                            fields_resident_fn fn, void *dev)
{
  if (targets->size2 != dim) GSL_ERROR("eval_fields_many: targets must be M x dim of the mirror", GSL_EBADLEN);
  const size_t m = targets->size1;
  if (S->size1 != m || S->size2 != K) GSL_ERROR("eval_fields_many: S must be M x K", GSL_EBADLEN);
  if (G && (G->size1 != m || G->size2 != K * dim)) GSL_ERROR("eval_fields_many: G must be M x (K dim)", GSL_EBADLEN);
  if (m == 0) return GSL_SUCCESS;
  stage_out out[3] = {STAGE_MATRIX(S), {G ? K * dim : 0, 0, G ? G->data : NULL, G ? G->tda : 0, NULL, NULL}, STAGE_INTS(leaf, 1)};
  host_stage hs;
  int st = host_stage_begin(&hs, c, targets, dim, out, 3), es = GSL_SUCCESS;
  if (!hs.h) GSL_ERROR("eval_fields_many: out of memory", GSL_ENOMEM);
  long long outside_n = 0;
  if (!st) es = fn(dev, hs.d_y, m, dim, (double *)out[0].d, K, (double *)out[1].d, K * dim, (int *)out[2].d);
  if (!st && !es) st = gsl_sinterp_hip_count_negative(c, (const int *)out[2].d, m, &outside_n);
  st = host_stage_end(&hs, st, !es);
  if (st) GSL_ERROR(gsl_sinterp_hip_last_error(c), st);
  if (es) return es;
  if (outside_n) GSL_ERROR("eval_fields_many: target(s) outside the triangulation (NaN rows, index -1)", GSL_EDOM);
  return GSL_SUCCESS;
}

/* ======================================================================== */
/* simplex_tree_device                                                       */
/* ======================================================================== */
struct simplex_tree_device {
  gsl_sinterp_hip_ctx *ctx;        /* member 0 (the only one for a single-device mirror) */
  simplex_tree *tree; /* borrowed */
  int n_nodes, n_points;
  void *d_records, *d_leaftab;     /* member 0 */
  int *d_pidx;
  double scale[2];
  int response_bound;
  /* multi-GPU mirror (simplex_tree_device_alloc_multi): every member holds its own packed records,
     leaf table and vertex ids; ss.grp owns the contexts (ctx above aliases member 0's) */
  shard_set ss;
  void *m_records[SINTERP_MAX_DEVICES], *m_leaftab[SINTERP_MAX_DEVICES];
  int *m_pidx[SINTERP_MAX_DEVICES];
  chunk_set cs;                    /* single-device mirror: pipelined host batches */
  fields_set fs;                   /* simplex_tree_device_set_responses (member 0) */
};

gsl_sinterp_hip_ctx *simplex_tree_device_ctx(simplex_tree_device *dev) { return dev ? dev->ctx : NULL; }

void simplex_tree_device_free(simplex_tree_device *dev)
{
  if (!dev) return;
  if (dev->ctx) fields_set_release(&dev->fs, dev->ctx);
  if (dev->ss.grp) {
    for (int i = 0; i < dev->ss.n; i++) {
      gsl_sinterp_hip_ctx *c = gsl_sinterp_hip_group_ctx(dev->ss.grp, i);
      gsl_sinterp_hip_free(c, dev->m_records[i]); gsl_sinterp_hip_free(c, dev->m_leaftab[i]); gsl_sinterp_hip_free(c, dev->m_pidx[i]);
    }
    shard_set_release(&dev->ss);                   /* destroys the members' contexts, dev->ctx among them */
    free(dev);
    return;
  }
  if (dev->ctx) {
    chunk_set_release(&dev->cs, dev->ctx);
    gsl_sinterp_hip_free(dev->ctx, dev->d_records);
    gsl_sinterp_hip_free(dev->ctx, dev->d_leaftab);
    gsl_sinterp_hip_free(dev->ctx, dev->d_pidx);
    gsl_sinterp_hip_ctx_destroy(dev->ctx);
  }
  free(dev);
}

simplex_tree_device *simplex_tree_device_alloc(simplex_tree *tree, gsl_matrix *data, int device)
{
  if (!tree || tree->dim != 2) GSL_ERROR_NULL("simplex_tree_device_alloc: need a 2-D tree", GSL_EINVAL);
  if (tree->n_points > 0 && !data) GSL_ERROR_NULL("simplex_tree_device_alloc: data matrix required", GSL_EINVAL);
  const int n = tree->n_simplexes, np = tree->n_points;
  for (int k = 0; k < n; k++)
    if (tree->simplexes[k].points != 3 * k || tree->simplexes[k].links != 3 * k)
      GSL_ERROR_NULL("simplex_tree_device_alloc: unexpected node slot layout", GSL_ESANITY);

  simplex_tree_device *dev = (simplex_tree_device *)calloc(1, sizeof *dev);
  if (!dev) GSL_ERROR_NULL("simplex_tree_device_alloc: out of memory", GSL_ENOMEM);
  dev->tree = tree; dev->n_nodes = n; dev->n_points = np;
  dev->scale[0] = gsl_vector_get(tree->scale, 0);
  dev->scale[1] = gsl_vector_get(tree->scale, 1);

  int st = gsl_sinterp_hip_ctx_create(&dev->ctx, device, NULL);
  if (st != GSL_SUCCESS) {
    free(dev);
    GSL_ERROR_NULL("simplex_tree_device_alloc: no usable HIP device (GPU path has no CPU fallback)", GSL_EFAILED);
  }

  int *h_type = (int *)malloc((size_t)n * sizeof(int));
  double *h_pts = (double *)malloc((size_t)(np > 0 ? np : 1) * 2 * sizeof(double));
  double geom[10];
  int *d_type = NULL, *d_links = NULL;
  double *d_pts = NULL;
  st = GSL_ENOMEM;
  if (h_type && h_pts) {
    for (int k = 0; k < n; k++) h_type[k] = (int)tree->simplexes[k].type;
    for (int i = 0; i < np; i++) {
      const double *row = data->data + tree->shuffle->data[i] * data->tda;
      h_pts[2 * i] = row[0]; h_pts[2 * i + 1] = row[1];
    }
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 2; j++) geom[2 * i + j] = gsl_matrix_get(tree->seed_points, i, j);
    geom[6] = gsl_vector_get(tree->shift, 0); geom[7] = gsl_vector_get(tree->shift, 1);
    geom[8] = dev->scale[0]; geom[9] = dev->scale[1];

    gsl_sinterp_hip_ctx *c = dev->ctx;
    const size_t nb = (size_t)n * sizeof(int);
    st = gsl_sinterp_hip_malloc(c, (void **)&d_type, nb);
    if (!st) st = gsl_sinterp_hip_malloc(c, (void **)&dev->d_pidx, 3 * nb);
    if (!st) st = gsl_sinterp_hip_malloc(c, (void **)&d_links, 3 * nb);
    if (!st) st = gsl_sinterp_hip_malloc(c, (void **)&d_pts, (size_t)(np > 0 ? np : 1) * 2 * sizeof(double));
    if (!st) st = gsl_sinterp_hip_malloc(c, &dev->d_records, (size_t)n * GSL_SINTERP_TREE_RECORD_BYTES);
    if (!st) st = gsl_sinterp_hip_malloc(c, &dev->d_leaftab, (size_t)n * GSL_SINTERP_TREE_LEAFTAB_BYTES);
    if (!st) st = gsl_sinterp_hip_h2d(c, d_type, h_type, nb);
    if (!st) st = gsl_sinterp_hip_h2d(c, dev->d_pidx, tree->pidx, 3 * nb);
    if (!st) st = gsl_sinterp_hip_h2d(c, d_links, tree->links, 3 * nb);
    if (!st && np > 0) st = gsl_sinterp_hip_h2d(c, d_pts, h_pts, (size_t)np * 2 * sizeof(double));
    if (!st) st = gsl_sinterp_hip_tree_pack(c, n, d_type, dev->d_pidx, d_links, np, d_pts, geom, dev->d_records);
    if (!st) st = gsl_sinterp_hip_sync(c);
    gsl_sinterp_hip_free(c, d_type);
    gsl_sinterp_hip_free(c, d_links);
    gsl_sinterp_hip_free(c, d_pts);
  }
  free(h_type); free(h_pts);
  if (st != GSL_SUCCESS) {
    gsl_error(dev->ctx ? gsl_sinterp_hip_last_error(dev->ctx) : "out of memory", __FILE__, __LINE__, st);
    simplex_tree_device_free(dev);
    return NULL;
  }
  return dev;
}

/* Mirror `tree` on every device of the list.  The raw DAG arrays (node types, vertex ids, links, points:
   SURVEY.md 8(e)'s ~17 MB at N = 50 000) go to member 0 over PCIe ONCE and are replicated with one
   broadcast per array (RCCL over xGMI); every member then packs its own node records and jump table,
   so all members evaluate from an identical, locally built mirror. */
simplex_tree_device *simplex_tree_device_alloc_multi(simplex_tree *tree, gsl_matrix *data, const int *devices, int n_devices)
{
  if (n_devices == 1 && devices) return simplex_tree_device_alloc(tree, data, devices[0]);
  if (!devices || n_devices < 1 || n_devices > SINTERP_MAX_DEVICES)
    GSL_ERROR_NULL("simplex_tree_device_alloc_multi: bad device list", GSL_EINVAL);
  if (!tree || tree->dim != 2) GSL_ERROR_NULL("simplex_tree_device_alloc_multi: need a 2-D tree", GSL_EINVAL);
  if (tree->n_points > 0 && !data) GSL_ERROR_NULL("simplex_tree_device_alloc_multi: data matrix required", GSL_EINVAL);
  const int n = tree->n_simplexes, np = tree->n_points;
  for (int k = 0; k < n; k++)
    if (tree->simplexes[k].points != 3 * k || tree->simplexes[k].links != 3 * k)
      GSL_ERROR_NULL("simplex_tree_device_alloc_multi: unexpected node slot layout", GSL_ESANITY);
  simplex_tree_device *dev = (simplex_tree_device *)calloc(1, sizeof *dev);
  if (!dev) GSL_ERROR_NULL("simplex_tree_device_alloc_multi: out of memory", GSL_ENOMEM);
  dev->tree = tree; dev->n_nodes = n; dev->n_points = np;
  dev->scale[0] = gsl_vector_get(tree->scale, 0);
  dev->scale[1] = gsl_vector_get(tree->scale, 1);
  if (gsl_sinterp_hip_group_create(&dev->ss.grp, devices, n_devices) != GSL_SUCCESS) {
    free(dev);
    GSL_ERROR_NULL("simplex_tree_device_alloc_multi: cannot create the device group (GPU path has no CPU fallback)", GSL_EFAILED);
  }
  dev->ss.n = n_devices;
  dev->ctx = gsl_sinterp_hip_group_ctx(dev->ss.grp, 0);

  const size_t nb = (size_t)n * sizeof(int), pb = (size_t)(np > 0 ? np : 1) * 2 * sizeof(double);
  int *h_type = (int *)malloc(nb);
  double *h_pts = (double *)malloc(pb);
  double geom[10];
  int *d_type[SINTERP_MAX_DEVICES] = {0}, *d_links[SINTERP_MAX_DEVICES] = {0};
  double *d_pts[SINTERP_MAX_DEVICES] = {0};
  int st = (h_type && h_pts) ? GSL_SUCCESS : GSL_ENOMEM;
  if (!st) {
    for (int k = 0; k < n; k++) h_type[k] = (int)tree->simplexes[k].type;
    for (int i = 0; i < np; i++) {
      const double *row = data->data + tree->shuffle->data[i] * data->tda;
      h_pts[2 * i] = row[0]; h_pts[2 * i + 1] = row[1];
    }
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 2; j++) geom[2 * i + j] = gsl_matrix_get(tree->seed_points, i, j);
    geom[6] = gsl_vector_get(tree->shift, 0); geom[7] = gsl_vector_get(tree->shift, 1);
    geom[8] = dev->scale[0]; geom[9] = dev->scale[1];
  }
  for (int r = 0; r < n_devices && !st; r++) {
    gsl_sinterp_hip_ctx *c = gsl_sinterp_hip_group_ctx(dev->ss.grp, r);
    st = gsl_sinterp_hip_malloc(c, (void **)&d_type[r], nb);
    if (!st) st = gsl_sinterp_hip_malloc(c, (void **)&dev->m_pidx[r], 3 * nb);
    if (!st) st = gsl_sinterp_hip_malloc(c, (void **)&d_links[r], 3 * nb);
    if (!st) st = gsl_sinterp_hip_malloc(c, (void **)&d_pts[r], pb);
    if (!st) st = gsl_sinterp_hip_malloc(c, &dev->m_records[r], (size_t)n * GSL_SINTERP_TREE_RECORD_BYTES);
    if (!st) st = gsl_sinterp_hip_malloc(c, &dev->m_leaftab[r], (size_t)n * GSL_SINTERP_TREE_LEAFTAB_BYTES);
  }
  if (!st) {
    gsl_sinterp_hip_ctx *c0 = dev->ctx;
    st = gsl_sinterp_hip_h2d(c0, d_type[0], h_type, nb);
    if (!st) st = gsl_sinterp_hip_h2d(c0, dev->m_pidx[0], tree->pidx, 3 * nb);
    if (!st) st = gsl_sinterp_hip_h2d(c0, d_links[0], tree->links, 3 * nb);
    if (!st && np > 0) st = gsl_sinterp_hip_h2d(c0, d_pts[0], h_pts, (size_t)np * 2 * sizeof(double));
    /* model replication: the only collective of the path */
    if (!st) st = gsl_sinterp_hip_group_broadcast(dev->ss.grp, (void *const *)d_type, nb);
    if (!st) st = gsl_sinterp_hip_group_broadcast(dev->ss.grp, (void *const *)dev->m_pidx, 3 * nb);
    if (!st) st = gsl_sinterp_hip_group_broadcast(dev->ss.grp, (void *const *)d_links, 3 * nb);
    if (!st) st = gsl_sinterp_hip_group_broadcast(dev->ss.grp, (void *const *)d_pts, pb);
  }
  for (int r = 0; r < n_devices && !st; r++)
    st = gsl_sinterp_hip_tree_pack(gsl_sinterp_hip_group_ctx(dev->ss.grp, r), n, d_type[r], dev->m_pidx[r], d_links[r], np, d_pts[r],
                                   geom, dev->m_records[r]);
  for (int r = 0; r < n_devices; r++) {
    gsl_sinterp_hip_ctx *c = gsl_sinterp_hip_group_ctx(dev->ss.grp, r);
    int s2 = gsl_sinterp_hip_sync(c);
    if (!st) st = s2;
    gsl_sinterp_hip_free(c, d_type[r]); gsl_sinterp_hip_free(c, d_links[r]); gsl_sinterp_hip_free(c, d_pts[r]);
  }
  free(h_type); free(h_pts);
  if (st != GSL_SUCCESS) {
    gsl_error(gsl_sinterp_hip_last_error(dev->ctx), __FILE__, __LINE__, st);
    simplex_tree_device_free(dev);
    return NULL;
  }
  dev->d_records = dev->m_records[0]; dev->d_leaftab = dev->m_leaftab[0]; dev->d_pidx = dev->m_pidx[0];
  return dev;
}

int simplex_tree_device_n_devices(const simplex_tree_device *dev) { return dev ? (dev->ss.grp ? dev->ss.n : 1) : 0; }
const char *simplex_tree_device_transport(const simplex_tree_device *dev)
{
  return (dev && dev->ss.grp) ? gsl_sinterp_hip_group_transport(dev->ss.grp) : "none";
}

static int simplex_shard_eval(void *state, int member, const double *d_y, size_t m, double *d_s, int *d_leaf)
{
  simplex_tree_device *dev = (simplex_tree_device *)state;
  int st = gsl_sinterp_hip_bary_eval(gsl_sinterp_hip_group_ctx(dev->ss.grp, member), dev->n_nodes, dev->m_records[member],
                                     dev->m_leaftab[member], dev->scale, d_y, m, 2, d_s, d_leaf, NULL);
  return st == GSL_EDOM ? GSL_SUCCESS : st;
}

int simplex_tree_device_set_response(simplex_tree_device *dev, const gsl_vector *response)
{
  if (!dev) GSL_ERROR("simplex_tree_device_set_response: null device tree", GSL_EFAULT);
  const int np = dev->n_points;
  if (np > 0 && (!response || response->size < (size_t)np))
    GSL_ERROR("simplex_tree_device_set_response: response shorter than the point set", GSL_EBADLEN);
  double *h = (double *)malloc((size_t)(np > 0 ? np : 1) * sizeof(double));
  if (!h) GSL_ERROR("simplex_tree_device_set_response: out of memory", GSL_ENOMEM);
  for (int i = 0; i < np; i++) h[i] = gsl_vector_get(response, dev->tree->shuffle->data[i]);
  if (dev->ss.grp) {
    /* response (insertion order) -> member 0 -> one broadcast -> every member binds its own leaf table */
    double *d_r[SINTERP_MAX_DEVICES] = {0};
    const size_t rb = (size_t)(np > 0 ? np : 1) * sizeof(double);
    int st = GSL_SUCCESS;
    for (int r = 0; r < dev->ss.n && !st; r++) st = gsl_sinterp_hip_malloc(gsl_sinterp_hip_group_ctx(dev->ss.grp, r), (void **)&d_r[r], rb);
    if (!st && np > 0) st = gsl_sinterp_hip_h2d(dev->ctx, d_r[0], h, (size_t)np * sizeof(double));
    if (!st) st = gsl_sinterp_hip_group_broadcast(dev->ss.grp, (void *const *)d_r, rb);
    for (int r = 0; r < dev->ss.n && !st; r++)
      st = gsl_sinterp_hip_tree_bind(gsl_sinterp_hip_group_ctx(dev->ss.grp, r), dev->n_nodes, dev->m_pidx[r], np, d_r[r], dev->m_leaftab[r]);
    for (int r = 0; r < dev->ss.n; r++) {
      gsl_sinterp_hip_ctx *c = gsl_sinterp_hip_group_ctx(dev->ss.grp, r);
      int s2 = gsl_sinterp_hip_sync(c);
      if (!st) st = s2;
      gsl_sinterp_hip_free(c, d_r[r]);
    }
    free(h);
    HIP_TRY(st, dev->ctx);
    dev->response_bound = 1;
    return GSL_SUCCESS;
  }
  double *d_resp = NULL;
  int st = gsl_sinterp_hip_malloc(dev->ctx, (void **)&d_resp, (size_t)(np > 0 ? np : 1) * sizeof(double));
  if (!st && np > 0) st = gsl_sinterp_hip_h2d(dev->ctx, d_resp, h, (size_t)np * sizeof(double));
  if (!st) st = gsl_sinterp_hip_tree_bind(dev->ctx, dev->n_nodes, dev->d_pidx, np, d_resp, dev->d_leaftab);
  if (!st) st = gsl_sinterp_hip_sync(dev->ctx);
  gsl_sinterp_hip_free(dev->ctx, d_resp);
  free(h);
  HIP_TRY(st, dev->ctx);
  dev->response_bound = 1;
  return GSL_SUCCESS;
}

int simplex_tree_device_eval_resident(simplex_tree_device *dev, const double *d_targets, size_t m,
                                      size_t ttda, double *d_values, simplex_index *d_leaf)
{
  if (!dev) GSL_ERROR("simplex_tree_device_eval: null device tree", GSL_EFAULT);
  if (!dev->response_bound) GSL_ERROR("simplex_tree_device_eval: no response bound", GSL_EINVAL);
  HIP_TRY(gsl_sinterp_hip_bary_eval(dev->ctx, dev->n_nodes, dev->d_records, dev->d_leaftab, dev->scale,
                                    d_targets, m, ttda, d_values, d_leaf, NULL), dev->ctx);
  return GSL_SUCCESS;
}

static int simplex_chunk_eval(void *state, const double *d_y, size_t m, double *d_s, int *d_leaf)
{
  simplex_tree_device *dev = (simplex_tree_device *)state;
  return gsl_sinterp_hip_bary_eval(dev->ctx, dev->n_nodes, dev->d_records, dev->d_leaftab, dev->scale, d_y, m, 2, d_s, d_leaf,
                                   (long long *)NULL);     /* NULL: no host read-back, the call stays asynchronous */
}

int simplex_tree_device_eval_many(simplex_tree_device *dev, const gsl_matrix *targets,
                                  gsl_vector *values, simplex_index *leaf)
{
  if (!dev) GSL_ERROR("simplex_tree_device_eval_many: null device tree", GSL_EFAULT);
  if (!dev->response_bound) GSL_ERROR("simplex_tree_device_eval_many: no response bound", GSL_EINVAL);
  if (!targets || !values) GSL_ERROR("simplex_tree_device_eval_many: null argument", GSL_EFAULT);
  if (targets->size2 != 2) GSL_ERROR("simplex_tree_device_eval_many: targets must be M x 2", GSL_EBADLEN);
  const size_t m = targets->size1;
  if (values->size != m) GSL_ERROR("simplex_tree_device_eval_many: values length must equal target rows", GSL_EBADLEN);
  if (m == 0) return GSL_SUCCESS;
  if (dev->ss.grp) {
    size_t outside_n = 0;
    int sst = shard_eval_many(&dev->ss, 2, targets, values, leaf, &simplex_shard_eval, dev, 1, &outside_n);
    if (sst != GSL_SUCCESS) GSL_ERROR("simplex_tree_device_eval_many: sharded evaluation failed", sst);
    if (outside_n) GSL_ERROR("simplex_tree_device_eval_many: target(s) outside the caging simplex", GSL_EDOM);
    return GSL_SUCCESS;
  }

  /* single device: chunks over the copy pipe (H2D | sweep | D2H overlap); the leaf indices always come back, they
     carry the outside-the-cage verdict (index -1, value NaN) */
  size_t outside_n = 0;
  int st = chunk_eval_many(&dev->cs, dev->ctx, 2, targets, values, leaf, &simplex_chunk_eval, dev, 1, &outside_n);
  if (st != GSL_SUCCESS) GSL_ERROR("simplex_tree_device_eval_many: evaluation failed", st);
  const int eval_st = outside_n ? GSL_EDOM : GSL_SUCCESS;
  if (eval_st == GSL_EDOM) GSL_ERROR("simplex_tree_device_eval_many: target(s) outside the caging simplex", GSL_EDOM);
  return GSL_SUCCESS;
}

/* ---- several responses on the same tree (csrc/hip/linear_fields.hip) ---- */
size_t simplex_tree_device_n_responses(const simplex_tree_device *dev) { return dev ? dev->fs.nf : 0; }

int simplex_tree_device_set_responses(simplex_tree_device *dev, const gsl_matrix *F)
{
  if (!dev || !F) GSL_ERROR("simplex_tree_device_set_responses: null argument", GSL_EFAULT);
  const size_t np = (size_t)dev->n_points, K = F->size2;
  if (K < 1 || K > GSL_SINTERP_MAX_FIELDS) GSL_ERROR("simplex_tree_device_set_responses: 1 .. GSL_SINTERP_MAX_FIELDS responses", GSL_EINVAL);
  if (F->size1 < np) GSL_ERROR("simplex_tree_device_set_responses: fewer rows than the point set", GSL_EBADLEN);
  double *h = (double *)malloc((np > 0 ? np : 1) * K * sizeof(double));
  if (!h) GSL_ERROR("simplex_tree_device_set_responses: out of memory", GSL_ENOMEM);
  for (size_t i = 0; i < np; i++)                      /* insertion order, as set_response */
    memcpy(h + i * K, F->data + dev->tree->shuffle->data[i] * F->tda, K * sizeof(double));
  int st = fields_bind(&dev->fs, dev->ctx, h, np, K, dev->response_bound, dev->d_leaftab, (size_t)dev->n_nodes * GSL_SINTERP_TREE_LEAFTAB_BYTES);
  free(h);
  if (st == GSL_ENOMEM) GSL_ERROR("simplex_tree_device_set_responses: out of memory", GSL_ENOMEM);
  HIP_TRY(st, dev->ctx);
  return GSL_SUCCESS;
}

int simplex_tree_device_eval_fields_resident(simplex_tree_device *dev, const double *d_targets, size_t m, size_t ttda, double *d_S,
                                             size_t stda, double *d_G, size_t gtda, simplex_index *d_leaf)
{
  if (!dev) GSL_ERROR("simplex_tree_device_eval_fields_resident: null device tree", GSL_EFAULT);
  const size_t K = dev->fs.nf;
  if (K == 0) GSL_ERROR("simplex_tree_device_eval_fields_resident: no responses bound", GSL_EINVAL);
  if (m > 0 && (!d_targets || !d_S)) GSL_ERROR("simplex_tree_device_eval_fields_resident: null argument", GSL_EFAULT);
  if (ttda < 2) GSL_ERROR("simplex_tree_device_eval_fields_resident: target rows shorter than 2", GSL_EBADLEN);
  if (stda < K || (d_G && gtda < 2 * K)) GSL_ERROR("simplex_tree_device_eval_fields_resident: row pitch below K (values) or 2 K (gradients)", GSL_EINVAL);
  if (m == 0) return GSL_SUCCESS;
  gsl_sinterp_hip_ctx *c = dev->ctx;                    /* a multi-device mirror: member 0 evaluates every target */
  HIP_TRY(fields_scratch(&dev->fs, c, m), c);
  int *loc = d_leaf ? d_leaf : dev->fs.d_leaf;
  HIP_TRY(gsl_sinterp_hip_bary_eval(c, dev->n_nodes, dev->d_records, dev->d_leaftab, dev->scale, d_targets, m, ttda, dev->fs.d_val, loc,
                                    (long long *)NULL), c);
  HIP_TRY(gsl_sinterp_hip_bary_fields_eval(c, dev->n_nodes, dev->d_records, dev->d_pidx, dev->n_points, dev->fs.d_F, (int)K, K, dev->scale,
                                           loc, d_targets, m, ttda, d_S, stda, d_G, gtda), c);
  return GSL_SUCCESS;
}

static int tree_fields_fn(void *dev, const double *d_y, size_t m, size_t ytda, double *d_S, size_t stda, double *d_G, size_t gtda, int *d_leaf)
{
  return simplex_tree_device_eval_fields_resident((simplex_tree_device *)dev, d_y, m, ytda, d_S, stda, d_G, gtda, d_leaf);
}

int simplex_tree_device_eval_fields_many(simplex_tree_device *dev, const gsl_matrix *targets, gsl_matrix *S, gsl_matrix *G,
                                         simplex_index *leaf)
{
  if (!dev || !targets || !S) GSL_ERROR("simplex_tree_device_eval_fields_many: null argument", GSL_EFAULT);
  if (dev->fs.nf == 0) GSL_ERROR("simplex_tree_device_eval_fields_many: no responses bound", GSL_EINVAL);
  return fields_eval_host(dev->ctx, 2, dev->fs.nf, targets, S, G, leaf, &tree_fields_fn, dev);
}

/* reference: check_leaf_nodes / check_delaunay (linear_simplex_integrity_check.c:121-168) */
int simplex_tree_check_device(simplex_tree *tree, gsl_matrix *data, int device, long long *leaf_violations,
                              long long *delaunay_violations)
{
  if (leaf_violations) *leaf_violations = 0;
  if (delaunay_violations) *delaunay_violations = 0;
  if (!tree || tree->dim != 2) GSL_ERROR_VAL("simplex_tree_check_device: need a 2-D tree", GSL_EINVAL, -GSL_EINVAL);
  if (tree->n_points > 0 && !data) GSL_ERROR_VAL("simplex_tree_check_device: data matrix required", GSL_EINVAL, -GSL_EINVAL);
  const int n = tree->n_simplexes, np = tree->n_points;
  for (int k = 0; k < n; k++)
    if (tree->simplexes[k].points != 3 * k || tree->simplexes[k].links != 3 * k)
      GSL_ERROR_VAL("simplex_tree_check_device: unexpected node slot layout", GSL_ESANITY, -GSL_ESANITY);
  gsl_sinterp_hip_ctx *c = NULL;
  if (gsl_sinterp_hip_ctx_create(&c, device, NULL) != GSL_SUCCESS)
    GSL_ERROR_VAL("simplex_tree_check_device: no usable HIP device (GPU path has no CPU fallback)", GSL_EFAILED, -GSL_EFAILED);
  const size_t nb = (size_t)n * sizeof(int), pb = (size_t)(np > 0 ? np : 1) * 2 * sizeof(double);
  int *h_type = (int *)malloc(nb);
  double *h_pts = (double *)malloc(pb);
  int *d_type = NULL, *d_pidx = NULL, *d_links = NULL;
  double *d_pts = NULL, geom[10];
  long long lv = 0, dv = 0;
  int st = (h_type && h_pts) ? GSL_SUCCESS : GSL_ENOMEM;
  if (!st) {
    for (int k = 0; k < n; k++) h_type[k] = (int)tree->simplexes[k].type;
    for (int i = 0; i < np; i++) {
      const double *row = data->data + tree->shuffle->data[i] * data->tda;
      h_pts[2 * i] = row[0]; h_pts[2 * i + 1] = row[1];
    }
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 2; j++) geom[2 * i + j] = gsl_matrix_get(tree->seed_points, i, j);
    geom[6] = gsl_vector_get(tree->shift, 0); geom[7] = gsl_vector_get(tree->shift, 1);
    geom[8] = gsl_vector_get(tree->scale, 0); geom[9] = gsl_vector_get(tree->scale, 1);
    st = gsl_sinterp_hip_malloc(c, (void **)&d_type, nb);
    if (!st) st = gsl_sinterp_hip_malloc(c, (void **)&d_pidx, 3 * nb);
    if (!st) st = gsl_sinterp_hip_malloc(c, (void **)&d_links, 3 * nb);
    if (!st) st = gsl_sinterp_hip_malloc(c, (void **)&d_pts, pb);
    if (!st) st = gsl_sinterp_hip_h2d(c, d_type, h_type, nb);
    if (!st) st = gsl_sinterp_hip_h2d(c, d_pidx, tree->pidx, 3 * nb);
    if (!st) st = gsl_sinterp_hip_h2d(c, d_links, tree->links, 3 * nb);
    if (!st && np > 0) st = gsl_sinterp_hip_h2d(c, d_pts, h_pts, (size_t)np * 2 * sizeof(double));
    if (!st) st = gsl_sinterp_hip_tree_check(c, n, d_type, d_pidx, d_links, np, d_pts, geom, 3, &lv, &dv, NULL);
  }
  if (st) gsl_error(gsl_sinterp_hip_last_error(c), __FILE__, __LINE__, st);
  gsl_sinterp_hip_free(c, d_type); gsl_sinterp_hip_free(c, d_pidx); gsl_sinterp_hip_free(c, d_links); gsl_sinterp_hip_free(c, d_pts);
  gsl_sinterp_hip_ctx_destroy(c);
  free(h_type); free(h_pts);
  if (st) return -st;
  if (leaf_violations) *leaf_violations = lv;
  if (delaunay_violations) *delaunay_violations = dv;
  return (lv == 0 && dv == 0) ? 1 : 0;
}

/* ======================================================================== */
/* simplex_mesh_device: imported triangulations on one device or a group     */
/* ======================================================================== */
struct simplex_mesh_device {
  gsl_sinterp_hip_ctx *ctx;        /* member 0 */
  int n_tri, n_points, G, convex, n_members;
  int dim;                         /* 2: triangles (bary.hip), 3: tetrahedra (mesh3.hip) */
  double geom[12];                 /* shift, scale, bounding box lo, hi: dim entries each */
  void *m_records[SINTERP_MAX_DEVICES], *m_leaftab[SINTERP_MAX_DEVICES];
  int *m_tri[SINTERP_MAX_DEVICES], *m_seed[SINTERP_MAX_DEVICES];
  shard_set ss;                    /* n_members > 1: ss.grp owns the contexts */
  chunk_set cs;                    /* n_members == 1: pipelined host batches */
  int response_bound;
  /* natural neighbours: nothing is computed, uploaded or kept for them until the first natural evaluation, which asks
     the (borrowed) mesh for the metric it is Delaunay in (simplex_mesh_delaunay_metric; -1 = not asked yet), uploads its
     links and points once more and packs nn_rec */
  const simplex_mesh *mesh;
  int nn_metric;
  void *nn_rec;
  /* Clough-Tocher (csrc/hip/cubic.hip), by the same rule: nothing until the first cubic call.  ct_bound: the caller's
     gradients (host copy, NULL = estimate); ct_g / ct_rec: gradients and records on the device (NULL = still to do) */
  double *ct_bound, *ct_g;
  void *ct_rec;
  size_t ct_iters, ct_maxiter;
  double ct_rtol, ct_resid;
  /* grow-only: the triangle indices of a resident natural / cubic batch whose caller did not ask for them */
  int *sw_leaf;
  size_t sw_leaf_cap;
  fields_set fs;                   /* simplex_mesh_device_set_responses (member 0) */
};

gsl_sinterp_hip_ctx *simplex_mesh_device_ctx(simplex_mesh_device *dev) { return dev ? dev->ctx : NULL; }
int simplex_mesh_device_n_devices(const simplex_mesh_device *dev) { return dev ? dev->n_members : 0; }

static gsl_sinterp_hip_ctx *mesh_member_ctx(const simplex_mesh_device *dev, int r)
{
  return dev->ss.grp ? gsl_sinterp_hip_group_ctx(dev->ss.grp, r) : dev->ctx;
}

void simplex_mesh_device_free(simplex_mesh_device *dev)
{
  if (!dev) return;
  for (int r = 0; r < dev->n_members; r++) {
    gsl_sinterp_hip_ctx *c = mesh_member_ctx(dev, r);
    if (!c) continue;
    gsl_sinterp_hip_free(c, dev->m_records[r]); gsl_sinterp_hip_free(c, dev->m_leaftab[r]);
    gsl_sinterp_hip_free(c, dev->m_tri[r]); gsl_sinterp_hip_free(c, dev->m_seed[r]);
  }
  if (dev->ctx) {
    fields_set_release(&dev->fs, dev->ctx);
    gsl_sinterp_hip_free(dev->ctx, dev->nn_rec); gsl_sinterp_hip_free(dev->ctx, dev->sw_leaf);
    gsl_sinterp_hip_free(dev->ctx, dev->ct_g); gsl_sinterp_hip_free(dev->ctx, dev->ct_rec);
  }
  free(dev->ct_bound);
  if (dev->ss.grp) shard_set_release(&dev->ss);      /* destroys the members' contexts */
  else if (dev->ctx) { chunk_set_release(&dev->cs, dev->ctx); gsl_sinterp_hip_ctx_destroy(dev->ctx); }
  free(dev);
}

simplex_mesh_device *simplex_mesh_device_alloc_multi(const simplex_mesh *mesh, const int *devices, int n_devices)
{
  if (!mesh || !devices) GSL_ERROR_NULL("simplex_mesh_device_alloc: null argument", GSL_EFAULT);
  if (n_devices < 1 || n_devices > SINTERP_MAX_DEVICES) GSL_ERROR_NULL("simplex_mesh_device_alloc: bad device list", GSL_EINVAL);
  simplex_mesh_device *dev = (simplex_mesh_device *)calloc(1, sizeof *dev);
  if (!dev) GSL_ERROR_NULL("simplex_mesh_device_alloc: out of memory", GSL_ENOMEM);
  const size_t nt = simplex_mesh_n_triangles(mesh), np = simplex_mesh_n_points(mesh);
  const size_t d = simplex_mesh_dim(mesh), w = d + 1;
  dev->n_tri = (int)nt; dev->n_points = (int)np; dev->convex = simplex_mesh_convex(mesh); dev->n_members = n_devices;
  dev->dim = (int)d;
  if (d == 2) {
    /* about two triangles per seed cell */
    int G = (int)ceil(sqrt((double)nt / 2.0));
    dev->G = G < 1 ? 1 : (G > 2048 ? 2048 : G);
  } else {
    /* about four tetrahedra per seed cell; the cap keeps the two G^3 tables at 2 x 160^3 x 4 bytes = 33 MB */
    int G = (int)ceil(cbrt((double)nt / 4.0));
    dev->G = G < 1 ? 1 : (G > GSL_SINTERP_MESH3_MAX_GRID ? GSL_SINTERP_MESH3_MAX_GRID : G);
  }
  simplex_mesh_geometry(mesh, dev->geom, dev->geom + d);
  simplex_mesh_bbox(mesh, dev->geom + 2 * d, dev->geom + 3 * d);
  if (n_devices > 1) {
    if (gsl_sinterp_hip_group_create(&dev->ss.grp, devices, n_devices) != GSL_SUCCESS) {
      free(dev);
      GSL_ERROR_NULL("simplex_mesh_device_alloc: cannot create the device group (GPU path has no CPU fallback)", GSL_EFAILED);
    }
    dev->ss.n = n_devices;
    dev->ctx = gsl_sinterp_hip_group_ctx(dev->ss.grp, 0);
  } else if (gsl_sinterp_hip_ctx_create(&dev->ctx, devices[0], NULL) != GSL_SUCCESS) {
    free(dev);
    GSL_ERROR_NULL("simplex_mesh_device_alloc: no usable HIP device (GPU path has no CPU fallback)", GSL_EFAILED);
  }
  const size_t tb = w * nt * sizeof(int), pb = d * np * sizeof(double);
  const size_t rec_bytes = d == 2 ? GSL_SINTERP_TREE_RECORD_BYTES : GSL_SINTERP_MESH3_RECORD_BYTES;
  const size_t tab_bytes = d == 2 ? GSL_SINTERP_TREE_LEAFTAB_BYTES : GSL_SINTERP_MESH3_TABLE_BYTES;
  const size_t seed_ints = d == 2 ? 2 * (size_t)dev->G * dev->G : 2 * (size_t)dev->G * dev->G * dev->G + 2;
  int *d_nbr[SINTERP_MAX_DEVICES] = {0};
  double *d_pts[SINTERP_MAX_DEVICES] = {0};
  int st = GSL_SUCCESS;
  for (int r = 0; r < n_devices && !st; r++) {
    gsl_sinterp_hip_ctx *c = mesh_member_ctx(dev, r);
    st = gsl_sinterp_hip_malloc(c, (void **)&dev->m_tri[r], tb);
    if (!st) st = gsl_sinterp_hip_malloc(c, (void **)&d_nbr[r], tb);
    if (!st) st = gsl_sinterp_hip_malloc(c, (void **)&d_pts[r], pb);
    if (!st) st = gsl_sinterp_hip_malloc(c, &dev->m_records[r], nt * rec_bytes);
    if (!st) st = gsl_sinterp_hip_malloc(c, &dev->m_leaftab[r], nt * tab_bytes);
    if (!st) st = gsl_sinterp_hip_malloc(c, (void **)&dev->m_seed[r], seed_ints * sizeof(int));
  }
  if (!st) st = gsl_sinterp_hip_h2d(dev->ctx, dev->m_tri[0], simplex_mesh_triangles(mesh), tb);
  if (!st) st = gsl_sinterp_hip_h2d(dev->ctx, d_nbr[0], simplex_mesh_neighbours(mesh), tb);
  if (!st) st = gsl_sinterp_hip_h2d(dev->ctx, d_pts[0], simplex_mesh_points(mesh), pb);
  if (!st && dev->ss.grp) {                             /* model replication: the only collective of the path */
    st = gsl_sinterp_hip_group_broadcast(dev->ss.grp, (void *const *)dev->m_tri, tb);
    if (!st) st = gsl_sinterp_hip_group_broadcast(dev->ss.grp, (void *const *)d_nbr, tb);
    if (!st) st = gsl_sinterp_hip_group_broadcast(dev->ss.grp, (void *const *)d_pts, pb);
  }
  for (int r = 0; r < n_devices && !st; r++)            /* every member packs its own records and seed grid */
    st = (d == 2 ? gsl_sinterp_hip_mesh_pack : gsl_sinterp_hip_mesh3_pack)(mesh_member_ctx(dev, r), dev->n_tri, dev->m_tri[r], d_nbr[r],
                                                                           dev->n_points, d_pts[r], dev->geom, dev->G, dev->m_records[r],
                                                                           dev->m_seed[r]);
  for (int r = 0; r < n_devices; r++) {
    gsl_sinterp_hip_ctx *c = mesh_member_ctx(dev, r);
    int s2 = gsl_sinterp_hip_sync(c);
    if (!st) st = s2;
    gsl_sinterp_hip_free(c, d_nbr[r]); gsl_sinterp_hip_free(c, d_pts[r]);
  }
  dev->mesh = mesh; dev->nn_metric = -1;
  dev->ct_rtol = 1e-12; dev->ct_maxiter = 1000;
  if (st != GSL_SUCCESS) {
    gsl_error(gsl_sinterp_hip_last_error(dev->ctx), __FILE__, __LINE__, st);
    simplex_mesh_device_free(dev);
    return NULL;
  }
  return dev;
}

simplex_mesh_device *simplex_mesh_device_alloc(const simplex_mesh *mesh, int device)
{
  return simplex_mesh_device_alloc_multi(mesh, &device, 1);
}

/* forget the Clough-Tocher gradients and records (and, with `bound`, the caller's gradients) */
static void cubic_drop(simplex_mesh_device *dev, int bound)
{
  if (dev->ctx) { gsl_sinterp_hip_free(dev->ctx, dev->ct_g); gsl_sinterp_hip_free(dev->ctx, dev->ct_rec); }
  dev->ct_g = NULL; dev->ct_rec = NULL; dev->ct_iters = 0; dev->ct_resid = 0.0;
  if (bound) { free(dev->ct_bound); dev->ct_bound = NULL; }
}

int simplex_mesh_device_set_response(simplex_mesh_device *dev, const gsl_vector *response)
{
  if (!dev || !response) GSL_ERROR("simplex_mesh_device_set_response: null argument", GSL_EFAULT);
  if (response->size < (size_t)dev->n_points) GSL_ERROR("simplex_mesh_device_set_response: response shorter than the point set", GSL_EBADLEN);
  const size_t np = (size_t)dev->n_points, rb = np * sizeof(double);
  double *h = (double *)malloc(rb), *d_r[SINTERP_MAX_DEVICES] = {0};
  if (!h) GSL_ERROR("simplex_mesh_device_set_response: out of memory", GSL_ENOMEM);
  for (size_t i = 0; i < np; i++) h[i] = response->data[i * response->stride];
  int st = GSL_SUCCESS;
  for (int r = 0; r < dev->n_members && !st; r++) st = gsl_sinterp_hip_malloc(mesh_member_ctx(dev, r), (void **)&d_r[r], rb);
  if (!st) st = gsl_sinterp_hip_h2d(dev->ctx, d_r[0], h, rb);
  if (!st && dev->ss.grp) st = gsl_sinterp_hip_group_broadcast(dev->ss.grp, (void *const *)d_r, rb);
  for (int r = 0; r < dev->n_members && !st; r++)
    st = (dev->dim == 2 ? gsl_sinterp_hip_tree_bind : gsl_sinterp_hip_mesh3_bind)(mesh_member_ctx(dev, r), dev->n_tri, dev->m_tri[r],
                                                                                  dev->n_points, d_r[r], dev->m_leaftab[r]);
  for (int r = 0; r < dev->n_members; r++) {
    gsl_sinterp_hip_ctx *c = mesh_member_ctx(dev, r);
    int s2 = gsl_sinterp_hip_sync(c);
    if (!st) st = s2;
    gsl_sinterp_hip_free(c, d_r[r]);
  }
  free(h);
  if (st) GSL_ERROR(gsl_sinterp_hip_last_error(dev->ctx), st);
  dev->response_bound = 1;
  cubic_drop(dev, 1);                                   /* gradients and records belong to the response */
  return GSL_SUCCESS;
}

int simplex_mesh_device_eval_resident(simplex_mesh_device *dev, const double *d_targets, size_t m, size_t ttda,
                                      double *d_values, int *d_triangle)
{
  if (!dev) GSL_ERROR("simplex_mesh_device_eval_resident: null device mirror", GSL_EFAULT);
  if (!dev->response_bound) GSL_ERROR("simplex_mesh_device_eval_resident: no response bound", GSL_EINVAL);
  /* resident buffers live on ONE device: member 0 evaluates them */
  if (ttda < (size_t)dev->dim) GSL_ERROR("simplex_mesh_device_eval_resident: target rows shorter than the mesh's dimension", GSL_EBADLEN);
  int st = (dev->dim == 2 ? gsl_sinterp_hip_mesh_eval : gsl_sinterp_hip_mesh3_eval)(dev->ctx, dev->n_tri, dev->m_records[0], dev->m_leaftab[0],
                                                                                    dev->m_seed[0], dev->G, dev->geom, dev->convex, d_targets,
                                                                                    m, ttda, d_values, d_triangle, NULL);
  if (st) GSL_ERROR(gsl_sinterp_hip_last_error(dev->ctx), st);
  return GSL_SUCCESS;
}

static int mesh_shard_eval(void *state, int member, const double *d_y, size_t m, double *d_s, int *d_leaf)
{
  simplex_mesh_device *dev = (simplex_mesh_device *)state;
  return (dev->dim == 2 ? gsl_sinterp_hip_mesh_eval : gsl_sinterp_hip_mesh3_eval)(mesh_member_ctx(dev, member), dev->n_tri, dev->m_records[member],
                                                                                  dev->m_leaftab[member], dev->m_seed[member], dev->G, dev->geom,
                                                                                  dev->convex, d_y, m, (size_t)dev->dim, d_s, d_leaf,
                                                                                  (long long *)NULL);
}
static int mesh_chunk_eval(void *state, const double *d_y, size_t m, double *d_s, int *d_leaf) { return mesh_shard_eval(state, 0, d_y, m, d_s, d_leaf); }

int simplex_mesh_device_eval_many(simplex_mesh_device *dev, const gsl_matrix *targets, gsl_vector *values, int *triangle)
{
  if (!dev || !targets || !values) GSL_ERROR("simplex_mesh_device_eval_many: null argument", GSL_EFAULT);
  if (!dev->response_bound) GSL_ERROR("simplex_mesh_device_eval_many: no response bound", GSL_EINVAL);
  if (targets->size2 != (size_t)dev->dim) {
    if (dev->dim == 2) GSL_ERROR("simplex_mesh_device_eval_many: targets must be M x 2", GSL_EBADLEN);
    GSL_ERROR("simplex_mesh_device_eval_many: targets must be M x 3 (tetrahedral mesh)", GSL_EBADLEN);
  }
  const size_t m = targets->size1, d = (size_t)dev->dim;
  if (values->size != m) GSL_ERROR("simplex_mesh_device_eval_many: values length must equal target rows", GSL_EBADLEN);
  if (m == 0) return GSL_SUCCESS;
  size_t outside_n = 0;
  int st = dev->ss.grp ? shard_eval_many(&dev->ss, d, targets, values, triangle, &mesh_shard_eval, dev, 1, &outside_n)
                       : chunk_eval_many(&dev->cs, dev->ctx, d, targets, values, triangle, &mesh_chunk_eval, dev, 1, &outside_n);
  if (st != GSL_SUCCESS) GSL_ERROR("simplex_mesh_device_eval_many: evaluation failed", st);
  if (outside_n) GSL_ERROR("simplex_mesh_device_eval_many: target(s) outside the triangulation", GSL_EDOM);
  return GSL_SUCCESS;
}

/* ---- several responses on the same mirror (csrc/hip/linear_fields.hip) ---- */
size_t simplex_mesh_device_n_responses(const simplex_mesh_device *dev) { return dev ? dev->fs.nf : 0; }

int simplex_mesh_device_set_responses(simplex_mesh_device *dev, const gsl_matrix *F)
{
  if (!dev || !F) GSL_ERROR("simplex_mesh_device_set_responses: null argument", GSL_EFAULT);
  const size_t np = (size_t)dev->n_points, K = F->size2;
  if (K < 1 || K > GSL_SINTERP_MAX_FIELDS) GSL_ERROR("simplex_mesh_device_set_responses: 1 .. GSL_SINTERP_MAX_FIELDS responses", GSL_EINVAL);
  if (F->size1 < np) GSL_ERROR("simplex_mesh_device_set_responses: fewer rows than the point set", GSL_EBADLEN);
  double *h = (double *)malloc(np * K * sizeof(double));
  if (!h) GSL_ERROR("simplex_mesh_device_set_responses: out of memory", GSL_ENOMEM);
  for (size_t i = 0; i < np; i++) memcpy(h + i * K, F->data + i * F->tda, K * sizeof(double));
  const size_t tab_bytes = (size_t)dev->n_tri * (dev->dim == 2 ? GSL_SINTERP_TREE_LEAFTAB_BYTES : GSL_SINTERP_MESH3_TABLE_BYTES);
  int st = fields_bind(&dev->fs, dev->ctx, h, np, K, dev->response_bound, dev->m_leaftab[0], tab_bytes);
  free(h);
  if (st == GSL_ENOMEM) GSL_ERROR("simplex_mesh_device_set_responses: out of memory", GSL_ENOMEM);
  if (st) GSL_ERROR(gsl_sinterp_hip_last_error(dev->ctx), st);
  return GSL_SUCCESS;
}

int simplex_mesh_device_eval_fields_resident(simplex_mesh_device *dev, const double *d_targets, size_t m, size_t ttda, double *d_S,
                                             size_t stda, double *d_G, size_t gtda, int *d_triangle)
{
  if (!dev) GSL_ERROR("simplex_mesh_device_eval_fields_resident: null device mirror", GSL_EFAULT);
  const size_t K = dev->fs.nf, d = (size_t)dev->dim;
  if (K == 0) GSL_ERROR("simplex_mesh_device_eval_fields_resident: no responses bound", GSL_EINVAL);
  if (m > 0 && (!d_targets || !d_S)) GSL_ERROR("simplex_mesh_device_eval_fields_resident: null argument", GSL_EFAULT);
  if (ttda < d) GSL_ERROR("simplex_mesh_device_eval_fields_resident: target rows shorter than the mesh's dimension", GSL_EBADLEN);
  if (stda < K || (d_G && gtda < d * K))
    GSL_ERROR("simplex_mesh_device_eval_fields_resident: row pitch below K (values) or K dim (gradients)", GSL_EINVAL);
  if (m == 0) return GSL_SUCCESS;
  gsl_sinterp_hip_ctx *c = dev->ctx;                    /* resident buffers live on ONE device: member 0 evaluates them */
  int st = fields_scratch(&dev->fs, c, m);
  int *loc = d_triangle ? d_triangle : dev->fs.d_leaf;
  if (!st) st = (d == 2 ? gsl_sinterp_hip_mesh_eval : gsl_sinterp_hip_mesh3_eval)(c, dev->n_tri, dev->m_records[0], dev->m_leaftab[0], dev->m_seed[0],
                                                                                 dev->G, dev->geom, dev->convex, d_targets, m, ttda,
                                                                                 dev->fs.d_val, loc, (long long *)NULL);
  if (!st && d == 2) st = gsl_sinterp_hip_bary_fields_eval(c, dev->n_tri, dev->m_records[0], dev->m_tri[0], dev->n_points, dev->fs.d_F, (int)K, K,
                                                           dev->geom + 2, loc, d_targets, m, ttda, d_S, stda, d_G, gtda);
  if (!st && d == 3) st = gsl_sinterp_hip_mesh3_fields_eval(c, dev->n_tri, dev->m_records[0], dev->m_tri[0], dev->n_points, dev->fs.d_F, (int)K, K,
                                                            dev->geom, loc, d_targets, m, ttda, d_S, stda, d_G, gtda);
  if (st) GSL_ERROR(gsl_sinterp_hip_last_error(c), st);
  return GSL_SUCCESS;
}

static int mesh_fields_fn(void *dev, const double *d_y, size_t m, size_t ytda, double *d_S, size_t stda, double *d_G, size_t gtda, int *d_leaf)
{
  return simplex_mesh_device_eval_fields_resident((simplex_mesh_device *)dev, d_y, m, ytda, d_S, stda, d_G, gtda, d_leaf);
}

int simplex_mesh_device_eval_fields_many(simplex_mesh_device *dev, const gsl_matrix *targets, gsl_matrix *S, gsl_matrix *G, int *triangle)
{
  if (!dev || !targets || !S) GSL_ERROR("simplex_mesh_device_eval_fields_many: null argument", GSL_EFAULT);
  if (dev->fs.nf == 0) GSL_ERROR("simplex_mesh_device_eval_fields_many: no responses bound", GSL_EINVAL);
  return fields_eval_host(dev->ctx, (size_t)dev->dim, dev->fs.nf, targets, S, G, triangle, &mesh_fields_fn, dev);
}

/* ---- natural neighbours on the same mirror (csrc/hip/natural.hip) ---- */
static int natural_status(simplex_mesh_device *dev)
{
  if (dev->dim != 2) GSL_ERROR("simplex_mesh_device_eval_natural: 2-D meshes only", GSL_EUNSUP);
  if (!dev->convex) GSL_ERROR("simplex_mesh_device_eval_natural: the mesh is not convex", GSL_EUNSUP);
  if (dev->n_members > 1) GSL_ERROR("simplex_mesh_device_eval_natural: one device only (no sharding over a device group)", GSL_EUNSUP);
  if (dev->nn_metric < 0) dev->nn_metric = simplex_mesh_delaunay_metric(dev->mesh);     /* first use: O(n_tri) on the host */
  if (dev->nn_metric == 0)
    GSL_ERROR("simplex_mesh_device_eval_natural: the mesh is not Delaunay, neither as given nor in standardised coordinates", GSL_EINVAL);
  if (!dev->response_bound) GSL_ERROR("simplex_mesh_device_eval_natural: no response bound", GSL_EINVAL);
  return GSL_SUCCESS;
}

/* the natural-neighbour records, packed at the first use from a second upload of the mesh's links and points */
static int natural_pack_once(simplex_mesh_device *dev)
{
  if (dev->nn_rec) return GSL_SUCCESS;
  gsl_sinterp_hip_ctx *c = dev->ctx;
  const size_t tb = 3 * (size_t)dev->n_tri * sizeof(int), pb = 2 * (size_t)dev->n_points * sizeof(double);
  const double one[2] = {1.0, 1.0};
  int *d_nbr = NULL;
  double *d_pts = NULL;
  int st = gsl_sinterp_hip_malloc(c, &dev->nn_rec, ((size_t)dev->n_tri + 1) * GSL_SINTERP_NATURAL_RECORD_BYTES);
  if (!st) st = gsl_sinterp_hip_malloc(c, (void **)&d_nbr, tb);
  if (!st) st = gsl_sinterp_hip_malloc(c, (void **)&d_pts, pb);
  if (!st) st = gsl_sinterp_hip_h2d(c, d_nbr, simplex_mesh_neighbours(dev->mesh), tb);
  if (!st) st = gsl_sinterp_hip_h2d(c, d_pts, simplex_mesh_points(dev->mesh), pb);
  if (!st) st = gsl_sinterp_hip_mesh_natural_pack(c, dev->n_tri, dev->m_tri[0], d_nbr, dev->n_points, d_pts,
                                                  dev->nn_metric == 2 ? dev->geom + 2 : one, dev->nn_rec);
  int s2 = gsl_sinterp_hip_sync(c);
  if (!st) st = s2;
  gsl_sinterp_hip_free(c, d_nbr); gsl_sinterp_hip_free(c, d_pts);
  if (st) { gsl_sinterp_hip_free(c, dev->nn_rec); dev->nn_rec = NULL; }
  return st;
}

/* The natural-neighbour and Clough-Tocher entries, resident and chunked: locate + linear value by the unchanged linear
   path (batches >= 4096 through its sorted route), then the method's sweep (cubic = 0: the cavity sweep, 1: the cubic
   one, d_g its optional gradient) over the triangle found; the linear values pass through d_s.  Nothing is read back. */
static int mesh_locate_sweep(simplex_mesh_device *dev, int cubic, const double *d_y, size_t m, size_t ytda, double *d_s, double *d_g,
                             size_t gtda, int *d_leaf)
{
  int st = gsl_sinterp_hip_mesh_eval(dev->ctx, dev->n_tri, dev->m_records[0], dev->m_leaftab[0], dev->m_seed[0], dev->G, dev->geom, dev->convex,
                                     d_y, m, ytda, d_s, d_leaf, (long long *)NULL);
  if (st) return st;
  if (cubic) return gsl_sinterp_hip_mesh_cubic_eval(dev->ctx, dev->n_tri, dev->ct_rec, d_leaf, d_s, d_y, m, ytda, d_s, d_g, gtda);
  return gsl_sinterp_hip_mesh_natural_eval(dev->ctx, dev->n_tri, dev->nn_rec, dev->m_leaftab[0], d_leaf, d_s, d_y, m, ytda, 0, d_s,
                                           (long long *)NULL);
}
static int natural_chunk_eval(void *state, const double *d_y, size_t m, double *d_s, int *d_leaf)
{
  return mesh_locate_sweep((simplex_mesh_device *)state, 0, d_y, m, 2, d_s, NULL, 0, d_leaf);
}
static int cubic_chunk_eval(void *state, const double *d_y, size_t m, double *d_s, int *d_leaf)
{
  return mesh_locate_sweep((simplex_mesh_device *)state, 1, d_y, m, 2, d_s, NULL, 0, d_leaf);
}

/* a resident batch: the sweep needs the triangle indices also when the caller does not */
static int mesh_sweep_resident(simplex_mesh_device *dev, int cubic, const double *d_y, size_t m, size_t ytda, double *d_s, double *d_g,
                               size_t gtda, int *d_leaf)
{
  int st = GSL_SUCCESS;
  if (!d_leaf) {
    if (m > dev->sw_leaf_cap) {
      gsl_sinterp_hip_free(dev->ctx, dev->sw_leaf); dev->sw_leaf = NULL; dev->sw_leaf_cap = 0;
      st = gsl_sinterp_hip_malloc(dev->ctx, (void **)&dev->sw_leaf, m * sizeof(int));
      if (!st) dev->sw_leaf_cap = m;
    }
    d_leaf = dev->sw_leaf;
  }
  if (!st) st = mesh_locate_sweep(dev, cubic, d_y, m, ytda, d_s, d_g, gtda, d_leaf);
  if (st) GSL_ERROR(gsl_sinterp_hip_last_error(dev->ctx), st);
  return GSL_SUCCESS;
}

int simplex_mesh_device_eval_natural_resident(simplex_mesh_device *dev, const double *d_targets, size_t m, size_t ttda,
                                              double *d_values, int *d_triangle)
{
  if (!dev) GSL_ERROR("simplex_mesh_device_eval_natural_resident: null device mirror", GSL_EFAULT);
  int st = natural_status(dev);
  if (st) return st;
  if (ttda < 2) GSL_ERROR("simplex_mesh_device_eval_natural_resident: target rows shorter than the mesh's dimension", GSL_EBADLEN);
  if (m == 0) return GSL_SUCCESS;
  st = natural_pack_once(dev);
  if (st) GSL_ERROR(gsl_sinterp_hip_last_error(dev->ctx), st);
  return mesh_sweep_resident(dev, 0, d_targets, m, ttda, d_values, NULL, 0, d_triangle);
}

int simplex_mesh_device_eval_natural_many(simplex_mesh_device *dev, const gsl_matrix *targets, gsl_vector *values, int *triangle)
{
  if (!dev || !targets || !values) GSL_ERROR("simplex_mesh_device_eval_natural_many: null argument", GSL_EFAULT);
  int st = natural_status(dev);
  if (st) return st;
  if (targets->size2 != 2) GSL_ERROR("simplex_mesh_device_eval_natural_many: targets must be M x 2", GSL_EBADLEN);
  const size_t m = targets->size1;
  if (values->size != m) GSL_ERROR("simplex_mesh_device_eval_natural_many: values length must equal target rows", GSL_EBADLEN);
  if (m == 0) return GSL_SUCCESS;
  st = natural_pack_once(dev);
  if (st) GSL_ERROR(gsl_sinterp_hip_last_error(dev->ctx), st);
  size_t outside_n = 0;
  st = chunk_eval_many(&dev->cs, dev->ctx, 2, targets, values, triangle, &natural_chunk_eval, dev, 1, &outside_n);
  if (st != GSL_SUCCESS) GSL_ERROR("simplex_mesh_device_eval_natural_many: evaluation failed", st);
  if (outside_n) GSL_ERROR("simplex_mesh_device_eval_natural_many: target(s) outside the triangulation", GSL_EDOM);
  return GSL_SUCCESS;
}

/* ---- Clough-Tocher on the same mirror (csrc/hip/cubic.hip) ---- */
static int cubic_status(simplex_mesh_device *dev)
{
  if (dev->dim != 2) GSL_ERROR("simplex_mesh_device cubic: 2-D meshes only", GSL_EUNSUP);
  if (dev->n_members > 1) GSL_ERROR("simplex_mesh_device cubic: one device only (no sharding over a device group)", GSL_EUNSUP);
  if (!dev->response_bound) GSL_ERROR("simplex_mesh_device cubic: no response bound", GSL_EINVAL);
  return GSL_SUCCESS;
}

int simplex_mesh_device_bind_gradients(simplex_mesh_device *dev, const gsl_matrix *gradients)
{
  if (!dev) GSL_ERROR("simplex_mesh_device_bind_gradients: null device mirror", GSL_EFAULT);
  if (dev->dim != 2) GSL_ERROR("simplex_mesh_device_bind_gradients: 2-D meshes only", GSL_EUNSUP);
  if (gradients && (gradients->size1 != (size_t)dev->n_points || gradients->size2 != 2))
    GSL_ERROR("simplex_mesh_device_bind_gradients: gradients must be (number of points) x 2", GSL_EBADLEN);
  double *h = NULL;
  if (gradients) {
    h = (double *)malloc(2 * (size_t)dev->n_points * sizeof(double));
    if (!h) GSL_ERROR("simplex_mesh_device_bind_gradients: out of memory", GSL_ENOMEM);
    for (size_t i = 0; i < (size_t)dev->n_points; i++) {
      h[2 * i] = gradients->data[i * gradients->tda]; h[2 * i + 1] = gradients->data[i * gradients->tda + 1];
    }
  }
  cubic_drop(dev, 1);
  dev->ct_bound = h;
  return GSL_SUCCESS;
}

int simplex_mesh_device_set_gradient_options(simplex_mesh_device *dev, double rtol, size_t maxiter)
{
  if (!dev) GSL_ERROR("simplex_mesh_device_set_gradient_options: null device mirror", GSL_EFAULT);
  if (!(rtol > 0.0 && rtol < 1.0) || maxiter < 1 || maxiter > (size_t)INT_MAX)
    GSL_ERROR("simplex_mesh_device_set_gradient_options: need 0 < rtol < 1 and maxiter >= 1", GSL_EINVAL);
  dev->ct_rtol = rtol; dev->ct_maxiter = maxiter;
  return GSL_SUCCESS;
}

/* gradients (bound or estimated) and records, at the first use.  The per-vertex data come back from the response
   table the linear path keeps (vertex i of triangle t = entry i of row t); a vertex of no triangle has no datum
   there and needs none. */
static int cubic_prepare(simplex_mesh_device *dev)
{
  if (dev->ct_rec) return GSL_SUCCESS;
  gsl_sinterp_hip_ctx *c = dev->ctx;
  const size_t nt = (size_t)dev->n_tri, np = (size_t)dev->n_points;
  const size_t tb = 3 * nt * sizeof(int), pb = 2 * np * sizeof(double);
  const int *tri = simplex_mesh_triangles(dev->mesh);
  int *d_nbr = NULL, *d_off = NULL, *d_adj = NULL, *h_off = NULL, *h_adj = NULL;
  double *d_pts = NULL, *d_f = NULL;
  double *h_tab = (double *)malloc(nt * GSL_SINTERP_TREE_LEAFTAB_BYTES), *h_f = (double *)calloc(np, sizeof(double));
  size_t n_adj = 0;
  int st = (h_tab && h_f) ? GSL_SUCCESS : GSL_ENOMEM, solve = GSL_SUCCESS;
  if (!st) st = gsl_sinterp_hip_sync(c);
  if (!st) st = gsl_sinterp_hip_d2h(c, h_tab, dev->m_leaftab[0], nt * GSL_SINTERP_TREE_LEAFTAB_BYTES);
  if (!st)
    for (size_t t = 0; t < nt; t++)
      for (int i = 0; i < 3; i++) h_f[tri[3 * t + i]] = h_tab[4 * t + i];
  if (!st) st = gsl_sinterp_hip_malloc(c, (void **)&d_nbr, tb);
  if (!st) st = gsl_sinterp_hip_malloc(c, (void **)&d_pts, pb);
  if (!st) st = gsl_sinterp_hip_malloc(c, (void **)&d_f, np * sizeof(double));
  if (!st && !dev->ct_g) st = gsl_sinterp_hip_malloc(c, (void **)&dev->ct_g, pb);
  if (!st) st = gsl_sinterp_hip_h2d(c, d_nbr, simplex_mesh_neighbours(dev->mesh), tb);
  if (!st) st = gsl_sinterp_hip_h2d(c, d_pts, simplex_mesh_points(dev->mesh), pb);
  if (!st) st = gsl_sinterp_hip_h2d(c, d_f, h_f, np * sizeof(double));
  if (!st && dev->ct_bound) {
    st = gsl_sinterp_hip_h2d(c, dev->ct_g, dev->ct_bound, pb);
    dev->ct_iters = 0; dev->ct_resid = 0.0;
  } else if (!st) {
    h_off = (int *)malloc((np + 1) * sizeof(int)); h_adj = (int *)malloc((6 * nt + 1) * sizeof(int));
    if (!h_off || !h_adj) st = GSL_ENOMEM;
    if (!st) st = simplex_mesh_vertex_adjacency(dev->mesh, h_off, h_adj, 6 * nt, &n_adj);
    if (!st) st = gsl_sinterp_hip_malloc(c, (void **)&d_off, (np + 1) * sizeof(int));
    if (!st) st = gsl_sinterp_hip_malloc(c, (void **)&d_adj, (n_adj + 1) * sizeof(int));
    if (!st) st = gsl_sinterp_hip_h2d(c, d_off, h_off, (np + 1) * sizeof(int));
    if (!st && n_adj) st = gsl_sinterp_hip_h2d(c, d_adj, h_adj, n_adj * sizeof(int));
    if (!st) {
      int iters = 0;
      solve = gsl_sinterp_hip_mesh_cubic_gradients(c, dev->n_points, d_off, d_adj, n_adj, d_pts, d_f, dev->ct_rtol, (int)dev->ct_maxiter,
                                                   dev->ct_g, &iters, &dev->ct_resid);
      dev->ct_iters = (size_t)iters;
      if (solve != GSL_SUCCESS && solve != GSL_EMAXITER) st = solve;
    }
  }
  if (!st) st = gsl_sinterp_hip_malloc(c, &dev->ct_rec, nt * GSL_SINTERP_CUBIC_RECORD_BYTES);
  if (!st) st = gsl_sinterp_hip_mesh_cubic_pack(c, dev->n_tri, dev->m_tri[0], d_nbr, dev->n_points, d_pts, d_f, dev->ct_g, dev->ct_rec);
  int s2 = gsl_sinterp_hip_sync(c);
  if (!st) st = s2;
  gsl_sinterp_hip_free(c, d_nbr); gsl_sinterp_hip_free(c, d_pts); gsl_sinterp_hip_free(c, d_f);
  gsl_sinterp_hip_free(c, d_off); gsl_sinterp_hip_free(c, d_adj);
  free(h_tab); free(h_f); free(h_off); free(h_adj);
  if (st) {
    const size_t it = dev->ct_iters;
    const double rs = dev->ct_resid;
    cubic_drop(dev, 0);
    dev->ct_iters = it; dev->ct_resid = rs;
    GSL_ERROR(gsl_sinterp_hip_last_error(c), st);
  }
  /* maxiter reached: the gradients of the last iterate and their records stay usable; the caller hears about it once */
  if (solve == GSL_EMAXITER) GSL_ERROR("simplex_mesh_device cubic: the gradient estimate reached maxiter before rtol", GSL_EMAXITER);
  return GSL_SUCCESS;
}

int simplex_mesh_device_gradients(simplex_mesh_device *dev, gsl_matrix *gradients, size_t *iterations, double *residual)
{
  if (!dev) GSL_ERROR("simplex_mesh_device_gradients: null device mirror", GSL_EFAULT);
  int st = cubic_status(dev);
  if (st) return st;
  if (gradients && (gradients->size1 != (size_t)dev->n_points || gradients->size2 != 2))
    GSL_ERROR("simplex_mesh_device_gradients: gradients must be (number of points) x 2", GSL_EBADLEN);
  const int ps = cubic_prepare(dev);
  if (iterations) *iterations = dev->ct_iters;
  if (residual) *residual = dev->ct_resid;
  if (ps != GSL_SUCCESS && ps != GSL_EMAXITER) return ps;
  if (gradients) {
    const size_t np = (size_t)dev->n_points;
    double *h = (double *)malloc(2 * np * sizeof(double));
    if (!h) GSL_ERROR("simplex_mesh_device_gradients: out of memory", GSL_ENOMEM);
    st = gsl_sinterp_hip_d2h(dev->ctx, h, dev->ct_g, 2 * np * sizeof(double));
    if (!st)
      for (size_t i = 0; i < np; i++) { gradients->data[i * gradients->tda] = h[2 * i]; gradients->data[i * gradients->tda + 1] = h[2 * i + 1]; }
    free(h);
    if (st) GSL_ERROR(gsl_sinterp_hip_last_error(dev->ctx), st);
  }
  return ps;
}

/* locate + linear value by the unchanged linear path (batches >= 4096 through its sorted route), then the cubic sweep
   over the triangle it found; the linear values pass through d_values */
int simplex_mesh_device_eval_cubic_resident(simplex_mesh_device *dev, const double *d_targets, size_t m, size_t ttda, double *d_values,
                                            double *d_gradient, size_t gtda, int *d_triangle)
{
  if (!dev) GSL_ERROR("simplex_mesh_device_eval_cubic_resident: null device mirror", GSL_EFAULT);
  int st = cubic_status(dev);
  if (st) return st;
  if (m > 0 && (!d_targets || !d_values)) GSL_ERROR("simplex_mesh_device_eval_cubic_resident: null argument", GSL_EFAULT);
  if (ttda < 2) GSL_ERROR("simplex_mesh_device_eval_cubic_resident: target rows shorter than the mesh's dimension", GSL_EBADLEN);
  if (d_gradient && gtda < 2) GSL_ERROR("simplex_mesh_device_eval_cubic_resident: gradient rows shorter than the mesh's dimension", GSL_EBADLEN);
  if (m == 0) return GSL_SUCCESS;
  st = cubic_prepare(dev);
  if (st == GSL_EMAXITER && dev->ct_rec) st = GSL_SUCCESS;          /* reported by the call that estimated */
  if (st) return st;
  return mesh_sweep_resident(dev, 1, d_targets, m, ttda, d_values, d_gradient, gtda, d_triangle);
}

/* host batches.  Values only: the chunk pipe of the linear entries.  With gradients: one shot through host_stage */
int simplex_mesh_device_eval_cubic_many(simplex_mesh_device *dev, const gsl_matrix *targets, gsl_vector *values, gsl_matrix *gradient,
                                        int *triangle)
{
  if (!dev || !targets || !values) GSL_ERROR("simplex_mesh_device_eval_cubic_many: null argument", GSL_EFAULT);
  int st = cubic_status(dev);
  if (st) return st;
  if (targets->size2 != 2) GSL_ERROR("simplex_mesh_device_eval_cubic_many: targets must be M x 2", GSL_EBADLEN);
  const size_t m = targets->size1;
  if (values->size != m) GSL_ERROR("simplex_mesh_device_eval_cubic_many: values length must equal target rows", GSL_EBADLEN);
  if (gradient && (gradient->size1 != m || gradient->size2 != 2))
    GSL_ERROR("simplex_mesh_device_eval_cubic_many: gradient must be M x 2", GSL_EBADLEN);
  if (m == 0) return GSL_SUCCESS;
  gsl_sinterp_hip_ctx *c = dev->ctx;
  if (!gradient) {
    st = cubic_prepare(dev);
    if (st == GSL_EMAXITER && dev->ct_rec) st = GSL_SUCCESS;          /* reported by the call that estimated */
    if (st) return st;
    size_t neg = 0;
    st = chunk_eval_many(&dev->cs, c, 2, targets, values, triangle, &cubic_chunk_eval, dev, 1, &neg);
    if (st != GSL_SUCCESS) GSL_ERROR("simplex_mesh_device_eval_cubic_many: evaluation failed", st);
    if (neg) GSL_ERROR("simplex_mesh_device_eval_cubic_many: target(s) outside the triangulation", GSL_EDOM);
    return GSL_SUCCESS;
  }
  stage_out out[3] = {STAGE_VECTOR(values), STAGE_MATRIX(gradient), STAGE_INTS(triangle, 1)};
  host_stage hs;
  st = host_stage_begin(&hs, c, targets, 2, out, 3);
  if (!hs.h) GSL_ERROR("simplex_mesh_device_eval_cubic_many: out of memory", GSL_ENOMEM);
  int es = GSL_SUCCESS;
  long long outside_n = 0;
  if (!st) es = simplex_mesh_device_eval_cubic_resident(dev, hs.d_y, m, 2, (double *)out[0].d, (double *)out[1].d, 2, (int *)out[2].d);
  if (!st && !es) st = gsl_sinterp_hip_count_negative(c, (const int *)out[2].d, m, &outside_n);
  st = host_stage_end(&hs, st, !es);
  if (st) GSL_ERROR(gsl_sinterp_hip_last_error(c), st);
  if (es) return es;
  if (outside_n) GSL_ERROR("simplex_mesh_device_eval_cubic_many: target(s) outside the triangulation", GSL_EDOM);
  return GSL_SUCCESS;
}

/* ======================================================================== */
/* what a type is: one row of type_table (below, with the generic entries)    */
/* ======================================================================== */
enum { FAM_RBF, FAM_TREE, FAM_MESH, FAM_SHEPARD };      /* the struct behind gsl_sinterp.state: rbf_state, simplex_state, mesh_state, shepard_state */
enum { MESH_LINEAR, MESH_NATURAL, MESH_CUBIC };
typedef struct {
  gsl_sinterp_type pub;       /* first member: the extern gsl_sinterp_* pointers point here */
  int id;                     /* the type id of a GSLSINT1 checkpoint: never renumbered */
  int family;
  int kind, krige, affine, pd;/* FAM_RBF: the kernel, ordinary kriging (covariance + estimated mean), the affine tail, positive
                                 definite kernel (Cholesky routes 1 / 7, hence leave-one-out and the fit) */
  int method, imported;       /* FAM_MESH: the interpolant on the triangles; the mesh is imported (gsl_sinterp_set_triangulation)
                                 or exported from a host-built tree */
  const char *noun;           /* natural, cubic and Shepard types: what their refusals call them */
} type_desc;
static const type_desc *desc_of(const gsl_sinterp_type *T);     /* the row of T, NULL for a type that is not in the table */

/* "<...> natural-neighbour <...>" / "<...> Clough-Tocher <...>": the refusals the two 2-D mesh methods share.  fmt has one
   %s; the facade is single-threaded, the handler reads the text before it returns */
static int noun_error(const type_desc *d, const char *fmt, int status)
{
  static char reason[192];
  snprintf(reason, sizeof reason, fmt, d->noun);
  gsl_error(reason, __FILE__, __LINE__, status);
  return status;
}

/* ======================================================================== */
/* RBF types                                                                 */
/* ======================================================================== */
typedef struct {
  int kind;
  gsl_sinterp_hip_ctx *ctx;   /* member 0: fill + factorisation + solves run here ("replicas only" for the solve) */
  size_t n, dim;
  double eps;
  double *d_x; /* n x dim, packed  (member 0: start of the model buffer) */
  double *d_w; /* n x nf, column q at d_w + q*n (member 0: model buffer + n*dim); column 0 is the model of every scalar entry */
  /* several fields (gsl_sinterp_init_fields): nf weight vectors on the same centres, model buffer [x | w_0 | .. | w_{nf-1}];
     nf = 0 before the first init, 1 after gsl_sinterp_init / fread.  nf_alloc: the field count the buffers were sized for.
     f_mean / f_poly: kriging mean / affine polynomial of every field (`mean` / `poly` below stay field 0's) */
  size_t nf, nf_alloc;
  double f_mean[GSL_SINTERP_MAX_FIELDS], f_poly[GSL_SINTERP_MAX_FIELDS][4];
  /* device group (n_devices > 1): the model buffer [x | w ..] of every member; ss.grp owns the contexts */
  shard_set ss;
  double *m_model[SINTERP_MAX_DEVICES];
  /* id of the model the buffers hold (fresh after every init / fread): lets the sweep keep its per-model
     preprocessing between evaluations (gsl_sinterp_hip_rbf_eval_model) */
  unsigned long long model_id;
  /* ordinary kriging (gsl_sinterp_kriging): the kernel is the covariance, `mean` the estimated mean added by every sweep */
  int krige;
  double mean;
  /* thin-plate spline with its affine tail (gsl_sinterp_rbf_tps_affine): c_0 + sum_a c_a y_a added by every sweep */
  int affine;
  double poly[4];
  chunk_set cs;                /* single-device: pipelined host batches */
  /* kriging variance (gsl_sinterp_set_variance): the Cholesky factor of K kept from the init on member 0 with what
     gsl_sinterp_hip_krige_variance_prepare derives from it, and a grow-only workspace for the evaluation.
     var_state: 0 nothing kept (not asked for), 1 ready, 2 the init took route 8 (no factor), 3 restored from a checkpoint */
  int var_state;
  double *d_llt, *d_b, *d_dinv, *d_vwork;
  size_t llt_lda, vwork_doubles;
  double denom;
  /* leave-one-out (gsl_sinterp_set_loo): residuals (column q at loo_e + q * n, loo_nf columns) and variances of the last
     init, on the host.  loo_state: 0 nothing held (not asked for), 1 ready, 2 the init took a route without a Cholesky
     factor, 3 restored from a checkpoint, 4 kriging on no more sites than mean / drift functions (undefined) */
  int loo_state;
  size_t loo_nf;
  double *loo_e, *loo_v;
  /* local kriging (gsl_sinterp_set_neighbours, route 11): the neighbour count and nugget of the last init; 0 = the global
     model.  d_w then holds the RESPONSES: nothing is solved at init, every target solves its own small system */
  size_t local_k;
  double local_nugget;
  /* universal kriging (gsl_sinterp_set_drift, route 12): the order of the last init / fread (0 = ordinary kriging), the
     number of drift functions, the standardisation of their coordinates, the coefficients of every field, and -- kept with
     the factor for the variance -- B = K^-1 P on member 0 and the host Cholesky factor of S = P^T B */
  int drift, local_drift;     /* local_drift: the local route (local_k > 0) runs with a linear drift */
  size_t drift_q;
  double drift_shift[3], drift_scale[3];
  double f_coef[GSL_SINTERP_MAX_FIELDS][GSL_SINTERP_DRIFT_MAX_TERMS];
  double *d_B;
  double drift_L[GSL_SINTERP_DRIFT_MAX_TERMS * GSL_SINTERP_DRIFT_MAX_TERMS];
} rbf_state;

/* rows of the work matrix per pass of gsl_sinterp_hip_chol_inv_diag ("Leave-one-out") */
#define LOO_CHUNK 2048

static unsigned long long next_model_id(void)
{
  static unsigned long long counter = 0;               /* the facade is single-threaded like the reference */
  return ++counter;
}

/* default shape: Gaussian eps = 2 N^(1/d) (the C-configurations); Wendland: support radius of eight mean
   spacings of a unit box, eps = N^(1/d) / 8; Matern 3/2, 5/2 and inverse multiquadric: eps = N^(1/d), the length scale
   1/eps equal to the mean spacing */
static double rbf_default_eps(int kind, size_t n, size_t dim)
{
  return (kind == GSL_SINTERP_RBF_WENDLAND ? 0.125 : kind == GSL_SINTERP_RBF_GAUSSIAN ? 2.0 : 1.0) * pow((double)n, 1.0 / (double)dim);
}

/* kind / krige / affine come from the type's row of the table: gsl_sinterp_alloc fills them in */
static void *rbf_alloc(size_t dim, size_t size)
{
  rbf_state *st = (rbf_state *)calloc(1, sizeof *st);
  if (st) { st->n = size; st->dim = dim; }
  return st;
}

/* one accessor per state family (defined with the type table): NULL when the interpolant's type is of another family */
static rbf_state *rbf_of(const gsl_sinterp *interp);

/* the kept factor and everything derived from it (member 0's context must still be alive) */
static void rbf_release_variance(rbf_state *st)
{
  if (st->ctx) {
    gsl_sinterp_hip_free(st->ctx, st->d_llt); gsl_sinterp_hip_free(st->ctx, st->d_b);
    gsl_sinterp_hip_free(st->ctx, st->d_dinv); gsl_sinterp_hip_free(st->ctx, st->d_vwork);
    gsl_sinterp_hip_free(st->ctx, st->d_B);
  }
  st->d_llt = st->d_b = st->d_dinv = st->d_vwork = st->d_B = NULL;
  st->llt_lda = st->vwork_doubles = 0; st->denom = 0.0; st->var_state = 0;
}

static void rbf_release_loo(rbf_state *st)
{
  free(st->loo_e); free(st->loo_v);
  st->loo_e = st->loo_v = NULL; st->loo_nf = 0; st->loo_state = 0;
}

/* Leave-one-out from the factor in the lower triangle of d_llt (routes 1 and 7) and the solved weights in st->d_w: the
   diagonal of the inverse, the combine, and the copy to the host arrays of the state.  Kriging takes b = K^-1 1 and
   1^T b from the kept variance data when there is one, from temporaries otherwise.  Everything allocated here is freed
   again: the factor is not kept for this. */
static int rbf_compute_loo(rbf_state *st, const double *d_llt, size_t lda, size_t nf, const double *d_B)
{
  gsl_sinterp_hip_ctx *c = st->ctx;
  const size_t n = st->n;
  size_t chunk = (n + 127) / 128 * 128;
  if (chunk > LOO_CHUNK) chunk = LOO_CHUNK;
  double *d_out = NULL, *d_work = NULL, *d_tb = NULL, *d_tdinv = NULL;     /* d_out = [g | v | E] */
  const double *d_b = NULL;
  double denom = 0.0;
  st->loo_e = (double *)malloc(n * nf * sizeof(double));
  st->loo_v = (double *)malloc(n * sizeof(double));
  int s = st->loo_e && st->loo_v ? GSL_SUCCESS : GSL_ENOMEM;
  if (!s && st->krige && !st->drift) {
    if (st->var_state == 1) {
      d_b = st->d_b; denom = st->denom;
    } else {
      s = gsl_sinterp_hip_malloc(c, (void **)&d_tb, n * sizeof(double));
      if (!s) s = gsl_sinterp_hip_malloc(c, (void **)&d_tdinv, ((n + 31) / 32) * 1024 * sizeof(double));
      if (!s) s = gsl_sinterp_hip_krige_variance_prepare(c, n, d_llt, lda, d_tb, d_tdinv, &denom);
      d_b = d_tb;
    }
  }
  if (!s) s = gsl_sinterp_hip_malloc(c, (void **)&d_out, n * (nf + 2) * sizeof(double));
  if (!s) s = gsl_sinterp_hip_malloc(c, (void **)&d_work, gsl_sinterp_hip_chol_inv_diag_work(n, chunk) * sizeof(double));
  if (!s) s = gsl_sinterp_hip_chol_inv_diag(c, n, d_llt, lda, d_out, d_work, chunk);
  /* with a drift: Dubrule's rule takes B = K^-1 P and the factor of S = P^T B in place of b and 1^T b */
  if (!s) s = st->drift ? gsl_sinterp_hip_loo_combine_drift(c, n, nf, d_out, d_B, n, st->drift_q, st->drift_L, st->d_w, n, d_out + 2 * n, n, d_out + n)
                        : gsl_sinterp_hip_loo_combine(c, n, nf, d_out, d_b, denom, st->d_w, n, d_out + 2 * n, n, d_out + n);
  if (!s) s = gsl_sinterp_hip_d2h(c, st->loo_v, d_out + n, n * sizeof(double));
  if (!s) s = gsl_sinterp_hip_d2h(c, st->loo_e, d_out + 2 * n, n * nf * sizeof(double));
  if (s) (void)gsl_sinterp_hip_sync(c);                  /* nothing queued may still use the buffers freed below */
  gsl_sinterp_hip_free(c, d_out); gsl_sinterp_hip_free(c, d_work);
  gsl_sinterp_hip_free(c, d_tb); gsl_sinterp_hip_free(c, d_tdinv);
  if (s) { rbf_release_loo(st); return s; }
  st->loo_nf = nf; st->loo_state = 1;
  return GSL_SUCCESS;
}

static void rbf_release_devices(rbf_state *st)
{
  rbf_release_variance(st);
  if (st->ss.grp) {
    for (int r = 0; r < st->ss.n; r++) {
      gsl_sinterp_hip_free(gsl_sinterp_hip_group_ctx(st->ss.grp, r), st->m_model[r]);
      st->m_model[r] = NULL;
    }
    shard_set_release(&st->ss);
  } else if (st->ctx) {
    chunk_set_release(&st->cs, st->ctx);
    gsl_sinterp_hip_free(st->ctx, st->d_x);       /* one buffer: d_w points into it */
    gsl_sinterp_hip_ctx_destroy(st->ctx);
  }
  st->ctx = NULL; st->d_x = st->d_w = NULL; st->nf_alloc = 0; st->nf = 0;
}

static void rbf_free(void *vstate)
{
  rbf_state *st = (rbf_state *)vstate;
  if (!st) return;
  rbf_release_devices(st);
  rbf_release_loo(st);
  free(st);
}

static int rbf_prepare_devices(gsl_sinterp *interp, rbf_state *st, size_t nf);

/* the solve of ONE field on column d_w (f on entry, weights on exit) through the single-field raw entries */
static int rbf_solve_column(gsl_sinterp *interp, rbf_state *st, double *d_phi, size_t lda, double *d_w, double *mean, double *poly,
                            double *rcond, int *route)
{
  gsl_sinterp_hip_ctx *c = st->ctx;
  const size_t n = st->n, dim = st->dim;
  if (st->krige)
    return gsl_sinterp_hip_krige_solve(c, st->kind, st->eps, interp->nugget, st->d_x, n, (int)dim, dim, d_phi, lda, d_w, mean, route);
  if (st->affine)
    return gsl_sinterp_hip_rbf_solve_affine(c, st->kind, st->eps, st->d_x, n, (int)dim, dim, d_phi, lda, d_w, poly, route);
  return gsl_sinterp_hip_rbf_solve_ex(c, st->kind, st->eps, st->d_x, n, (int)dim, dim, d_phi, lda, d_w, interp->solver, rcond, route);
}

/* the standardisation of the drift's coordinates: shift = the centre of the sites' bounding box, scale = 1 / half-extent
   per axis (1 for a zero extent); x packed n x dim */
static void rbf_drift_geometry(const double *x, size_t n, size_t dim, double *shift, double *scale)
{
  for (size_t a = 0; a < dim; a++) {
    double lo = x[a], hi = x[a];
    for (size_t i = 1; i < n; i++) { const double v = x[i * dim + a]; if (v < lo) lo = v; if (v > hi) hi = v; }
    const double half = 0.5 * (hi - lo);
    shift[a] = lo + half;
    scale[a] = half > 0.0 ? 1.0 / half : 1.0;
  }
  for (size_t a = dim; a < 3; a++) { shift[a] = 0.0; scale[a] = 1.0; }
}

/* Whether the n centres (packed n x dim) lie in a hyperplane to rounding, so that [1, x] has dependent columns on them and
   the affine tail of the thin-plate spline is not determined: modified Gram-Schmidt on the centred coordinate columns; a
   column whose remainder is not above 1e-12 of its own norm depends on the ones before it (or has no extent).  Exactly
   collinear / coplanar input leaves a remainder of a few ulp, 1e-16; at 1e-12 the bordered system's condition number is
   past 1e12 and no digit of the tail is left.  -1: out of memory. */
static int centres_in_a_hyperplane(const double *x, size_t n, size_t dim)
{
  double *c = (double *)malloc(n * dim * sizeof(double));
  if (!c) return -1;
  int flat = 0;
  for (size_t a = 0; a < dim && !flat; a++) {
    double *ca = c + a * n, mean = 0.0, norm0 = 0.0, rem = 0.0;
    for (size_t i = 0; i < n; i++) mean += x[i * dim + a];
    mean /= (double)n;
    for (size_t i = 0; i < n; i++) { ca[i] = x[i * dim + a] - mean; norm0 += ca[i] * ca[i]; }
    for (size_t b = 0; b < a; b++) {
      const double *cb = c + b * n;
      double dot = 0.0;
      for (size_t i = 0; i < n; i++) dot += ca[i] * cb[i];
      for (size_t i = 0; i < n; i++) ca[i] -= dot * cb[i];
    }
    for (size_t i = 0; i < n; i++) rem += ca[i] * ca[i];
    if (!(sqrt(rem) > 1e-12 * sqrt(norm0))) flat = 1;
    else { const double inv = 1.0 / sqrt(rem); for (size_t i = 0; i < n; i++) ca[i] *= inv; }
  }
  free(c);
  return flat;
}

/* f(i, q) = fdata[i * frow + q * fcol], nf fields: gsl_sinterp_init (nf = 1) and gsl_sinterp_init_fields */
static int rbf_init_fields(gsl_sinterp *interp, const gsl_matrix *x, const double *fdata, size_t frow, size_t fcol, size_t nf)
{
  rbf_state *st = rbf_of(interp);
  const size_t n = st->n, dim = st->dim;
  const int nd = interp->n_devices > 1 ? interp->n_devices : 1;
  if (st->krige && interp->drift > 0 && n < gsl_sinterp_drift_terms(dim, interp->drift))
    GSL_ERROR("gsl_sinterp_init: universal kriging needs at least as many sites as drift functions", GSL_EINVAL);
  rbf_release_variance(st);                             /* the factor of the previous model, if one was kept */
  rbf_release_loo(st);                                  /* ... and its leave-one-out data */
  int s = rbf_prepare_devices(interp, st, nf);
  if (s) return s;
  st->nf = 0;                                           /* not initialised until the solve succeeds */
  gsl_sinterp_hip_ctx *c = st->ctx;
  st->model_id = next_model_id();                       /* the buffers are about to change */
  st->eps = interp->shape > 0 ? interp->shape : rbf_default_eps(st->kind, n, dim);
  st->local_k = 0;
  st->drift = 0; st->drift_q = 0;

  double *h_x = (double *)malloc(n * dim * sizeof(double));
  double *h_f = (double *)malloc(n * nf * sizeof(double));
  if (!h_x || !h_f) { free(h_x); free(h_f); GSL_ERROR("gsl_sinterp_init: out of memory", GSL_ENOMEM); }
  for (size_t i = 0; i < n; i++) {
    for (size_t cdim = 0; cdim < dim; cdim++) h_x[i * dim + cdim] = x->data[i * x->tda + cdim];
    for (size_t q = 0; q < nf; q++) h_f[q * n + i] = fdata[i * frow + q * fcol];
  }
  if (st->affine) {
    const int flat = centres_in_a_hyperplane(h_x, n, dim);
    if (flat) {
      free(h_x); free(h_f);
      if (flat < 0) GSL_ERROR("gsl_sinterp_init: out of memory", GSL_ENOMEM);
      GSL_ERROR("gsl_sinterp_init: affine thin-plate spline: the centres lie in a hyperplane (collinear / coplanar), the affine tail is not determined",
                GSL_EDOM);
    }
  }
  const size_t model_bytes = n * (dim + nf) * sizeof(double);
  double *d_phi = NULL;
  int route = 0;
  /* affine thin-plate spline: room for the (n + d + 1) augmented matrix of the pivoted-LU route (lda even) */
  const size_t lda = st->affine ? ((n + dim + 2) & ~(size_t)1) : n, phi_rows = st->affine ? n + dim + 1 : n;
  s = gsl_sinterp_hip_malloc(c, (void **)&d_phi, phi_rows * lda * sizeof(double));
  if (!s) s = gsl_sinterp_hip_h2d(c, st->d_x, h_x, n * dim * sizeof(double));
  if (!s) s = gsl_sinterp_hip_h2d(c, st->d_w, h_f, n * nf * sizeof(double));
  /* fill + dense solve on the device: Cholesky (Gaussian), shifted-SPD Cholesky with a
     Woodbury correction or pivoted LU (thin-plate spline) -- csrc/hip/solve.hip */
  double rcond = GSL_NAN;
  memset(st->f_mean, 0, sizeof st->f_mean); memset(st->f_poly, 0, sizeof st->f_poly);
  /* Several fields.  The kernel matrix depends on the centres only: every positive definite kind and kriging with the default solver
     and no condition estimate share ONE fill and ONE factorisation (routes 1 / 7).  Everything else -- both thin-plate
     types (their shifted-SPD / Woodbury solve is per field), an explicit solver, set_rcond, kriging on a semi-definite
     matrix (GSL_EDOM from the shared route) -- solves field by field, refilling d_phi each time: nf factorisations. */
  int shared = nf > 1 && st->kind != GSL_SINTERP_RBF_TPS && interp->solver == GSL_SINTERP_SOLVER_DEFAULT && !interp->want_rcond;
  /* universal kriging (route 12): the drift functions ride the one factorisation with the fields; no per-field route and
     no pivoted fall-back.  B is wanted by the variance (kept) and by leave-one-out (freed with the init) */
  const int drift = st->krige ? interp->drift : 0;
  double *d_B = NULL;
  if (!s && drift) {
    const size_t q = gsl_sinterp_drift_terms(dim, drift);
    rbf_drift_geometry(h_x, n, dim, st->drift_shift, st->drift_scale);
    if (interp->want_variance || interp->want_loo) s = gsl_sinterp_hip_malloc(c, (void **)&d_B, n * q * sizeof(double));
    if (!s && interp->want_variance) s = gsl_sinterp_hip_malloc(c, (void **)&st->d_dinv, ((n + 31) / 32) * 1024 * sizeof(double));
    double *coef = (double *)malloc(nf * q * sizeof(double));            /* field k's q coefficients at coef + k * q */
    if (!s && !coef) s = GSL_ENOMEM;
    if (!s) s = gsl_sinterp_hip_ukrige_solve(c, st->kind, st->eps, interp->nugget, drift, st->drift_shift, st->drift_scale, st->d_x, n, (int)dim,
                                             dim, d_phi, lda, st->d_w, n, nf, coef, d_B, n, NULL, st->drift_L, st->d_dinv, &route);
    if (!s) {
      memset(st->f_coef, 0, sizeof st->f_coef);
      for (size_t k = 0; k < nf; k++) memcpy(st->f_coef[k], coef + k * q, q * sizeof(double));
      st->drift = drift; st->drift_q = q;
    }
    free(coef);
    shared = 1;
  }
  if (!s && shared && !drift) {
    if (st->krige) {
      s = gsl_sinterp_hip_krige_solve_fields(c, st->kind, st->eps, interp->nugget, st->d_x, n, (int)dim, dim, d_phi, lda, st->d_w, n, nf,
                                             st->f_mean, &route);
      if (s == GSL_EDOM) {                              /* semi-definite: per field, where route 8 handles it; F again */
        shared = 0;
        s = gsl_sinterp_hip_h2d(c, st->d_w, h_f, n * nf * sizeof(double));
      }
    } else {
      s = gsl_sinterp_hip_rbf_solve_fields(c, st->kind, st->eps, st->d_x, n, (int)dim, dim, d_phi, lda, st->d_w, n, nf, &route);
    }
  }
  if (!s && !shared)
    for (size_t q = 0; q < nf && !s; q++)               /* rcond from the first field, the route of the last */
      s = rbf_solve_column(interp, st, d_phi, lda, st->d_w + q * n, &st->f_mean[q], st->f_poly[q],
                           interp->want_rcond && q == 0 ? &rcond : NULL, &route);
  st->mean = st->f_mean[0]; memcpy(st->poly, st->f_poly[0], sizeof st->poly);
  interp->rcond = rcond; interp->route = route;
  /* kriging variance asked for: route 7 left L in the lower triangle of d_phi -- keep it (N^2 doubles, member 0 only)
     with b = K^-1 1, the inverted diagonal blocks and 1^T b; route 8 has no Cholesky factor to keep */
  if (!s && st->krige && interp->want_variance) {
    if (route == 12) {                                  /* B, Ls and the inverted diagonal blocks came with the solve */
      st->d_llt = d_phi; st->llt_lda = lda; st->var_state = 1; d_phi = NULL; st->d_B = d_B;
    } else if (route == 7) {
      s = gsl_sinterp_hip_malloc(c, (void **)&st->d_b, n * sizeof(double));
      if (!s) s = gsl_sinterp_hip_malloc(c, (void **)&st->d_dinv, ((n + 31) / 32) * 1024 * sizeof(double));
      if (!s) s = gsl_sinterp_hip_krige_variance_prepare(c, n, d_phi, lda, st->d_b, st->d_dinv, &st->denom);
      if (!s) { st->d_llt = d_phi; st->llt_lda = lda; st->var_state = 1; d_phi = NULL; }
    } else {
      st->var_state = 2;
    }
  }
  /* leave-one-out asked for: routes 1 and 7 left L in the lower triangle of d_phi (with set_rcond too: the original
     stays ABOVE the diagonal), still alive here or just handed to the variance; every other route has no factor */
  if (!s && interp->want_loo) {
    /* kriging estimates its mean (1 term) or drift (q terms) from the data: with no more sites than terms the model
       without site i does not exist, Dubrule's diagonal is 0 in exact arithmetic and e_i = w_i / diag_i is 0 / 0 */
    const size_t loo_terms = st->krige ? (drift ? gsl_sinterp_drift_terms(dim, drift) : 1) : 0;
    if (n <= loo_terms) st->loo_state = 4;
    else if (route == 1 || route == 7 || route == 12) s = rbf_compute_loo(st, st->d_llt ? st->d_llt : d_phi, lda, nf, d_B);
    else st->loo_state = 2;
  }
  /* replicate the solved model: ONE broadcast of the weight vector (+ centres) */
  if (!s && st->ss.grp) s = gsl_sinterp_hip_group_broadcast(st->ss.grp, (void *const *)st->m_model, model_bytes);
  if (!s) s = gsl_sinterp_hip_sync(c);
  if (st->ss.grp)
    for (int r = 1; r < nd; r++) { int s2 = gsl_sinterp_hip_sync(gsl_sinterp_hip_group_ctx(st->ss.grp, r)); if (!s) s = s2; }
  gsl_sinterp_hip_free(c, d_phi);
  if (d_B != st->d_B) gsl_sinterp_hip_free(c, d_B);     /* not handed to the variance */
  free(h_x); free(h_f);
  if (s) { rbf_release_variance(st); rbf_release_loo(st); }
  if (s == GSL_EDOM && drift) {
    /* d_w holds neither the responses nor weights now: nothing may evaluate it */
    rbf_release_devices(st);
    GSL_ERROR("gsl_sinterp_init: universal kriging: the covariance matrix is not positive definite, or the drift functions are linearly dependent on the sites",
              GSL_EDOM);
  }
  if (s == GSL_EDOM) GSL_ERROR("gsl_sinterp_init: kernel matrix is not positive definite", GSL_EDOM);
  HIP_TRY(s, c);
  st->nf = nf;
  return GSL_SUCCESS;
}

static int local_init(gsl_sinterp *interp, const gsl_matrix *x, const gsl_vector *f);

static int rbf_init(gsl_sinterp *interp, const gsl_matrix *x, const gsl_vector *f)
{
  if (interp->neighbours > 0) return local_init(interp, x, f);
  return rbf_init_fields(interp, x, f->data, f->stride, 0, 1);
}

/* contexts (one, or a device group) + the model buffer [centres | weights of nf fields] of every member */
static int rbf_prepare_devices(gsl_sinterp *interp, rbf_state *st, size_t nf)
{
  const size_t n = st->n, dim = st->dim;
  const int nd = interp->n_devices > 1 ? interp->n_devices : 1;
  /* (re)build the device side when the requested device set changed */
  int same = st->ctx != NULL && ((nd == 1 && !st->ss.grp && gsl_sinterp_hip_ctx_device(st->ctx) == interp->device) ||
                                 (st->ss.grp && st->ss.n == nd));
  if (same && st->ss.grp)
    for (int r = 0; r < nd; r++) same = same && gsl_sinterp_hip_group_device(st->ss.grp, r) == interp->devices[r];
  if (!same) {
    rbf_release_devices(st);
    if (nd > 1) {
      if (gsl_sinterp_hip_group_create(&st->ss.grp, interp->devices, nd) != GSL_SUCCESS)
        GSL_ERROR("gsl_sinterp_init: cannot create the device group (GPU path has no CPU fallback)", GSL_EFAILED);
      st->ss.n = nd;
      st->ctx = gsl_sinterp_hip_group_ctx(st->ss.grp, 0);
    } else if (gsl_sinterp_hip_ctx_create(&st->ctx, interp->device, NULL) != GSL_SUCCESS) {
      st->ctx = NULL;
      GSL_ERROR("gsl_sinterp_init: no usable HIP device (GPU path has no CPU fallback)", GSL_EFAILED);
    }
  }
  /* the model = [centres | weights], one buffer per member: N (d + nf) 8 bytes, the broadcast payload; reallocated
     when the field count changes */
  const size_t model_bytes = n * (dim + nf) * sizeof(double);
  int s = GSL_SUCCESS;
  if (st->nf_alloc != nf) {
    if (st->ss.grp) {
      for (int r = 0; r < nd; r++) { gsl_sinterp_hip_free(gsl_sinterp_hip_group_ctx(st->ss.grp, r), st->m_model[r]); st->m_model[r] = NULL; }
    } else {
      gsl_sinterp_hip_free(st->ctx, st->d_x);
    }
    st->d_x = st->d_w = NULL; st->nf = 0;
    st->nf_alloc = nf;
  }
  if (st->ss.grp) {
    for (int r = 0; r < nd && !s; r++)
      if (!st->m_model[r]) s = gsl_sinterp_hip_malloc(gsl_sinterp_hip_group_ctx(st->ss.grp, r), (void **)&st->m_model[r], model_bytes);
    st->d_x = st->m_model[0];
  } else if (!st->d_x) {
    s = gsl_sinterp_hip_malloc(st->ctx, (void **)&st->d_x, model_bytes);
  }
  st->d_w = st->d_x ? st->d_x + n * dim : NULL;
  if (s) { gsl_error(gsl_sinterp_hip_last_error(st->ctx), __FILE__, __LINE__, s); return s; }
  return GSL_SUCCESS;
}

static int local_eval_resident(const gsl_sinterp *interp, const double *d_y, size_t m, size_t ytda, double *d_s, double *d_var, int *d_idx);
static int local_eval_many(const gsl_sinterp *interp, const gsl_matrix *y, gsl_vector *sv, gsl_vector *var, int *idx);

/* the sweep of an RBF-type model on context c (plain, + kriging mean, + affine tail) */
static int rbf_sweep(const rbf_state *st, gsl_sinterp_hip_ctx *c, const double *d_x, const double *d_w, const double *d_y, size_t m,
                     size_t ytda, double *d_s)
{
  if (st->drift) {                                      /* the unchanged plain sweep, then p(u)^T c; the coefficients go by value */
    int s = gsl_sinterp_hip_rbf_eval_model(c, st->kind, st->eps, d_x, st->n, (int)st->dim, st->dim, d_w, d_y, m, ytda, d_s, st->model_id);
    if (!s) s = gsl_sinterp_hip_drift_add(c, st->drift, st->drift_shift, st->drift_scale, st->f_coef[0], 1, d_y, m, (int)st->dim, ytda, d_s, 1, NULL, 0);
    return s;
  }
  if (st->krige)
    return gsl_sinterp_hip_krige_eval(c, st->kind, st->eps, st->mean, d_x, st->n, (int)st->dim, st->dim, d_w, d_y, m, ytda, d_s, st->model_id);
  if (st->affine)
    return gsl_sinterp_hip_rbf_eval_affine(c, st->kind, st->eps, st->poly, d_x, st->n, (int)st->dim, st->dim, d_w, d_y, m, ytda, d_s,
                                           st->model_id);
  return gsl_sinterp_hip_rbf_eval_model(c, st->kind, st->eps, d_x, st->n, (int)st->dim, st->dim, d_w, d_y, m, ytda, d_s, st->model_id);
}

static int rbf_eval_resident(const gsl_sinterp *interp, const double *d_y, size_t m, size_t ytda,
                             double *d_s, int *d_leaf)
{
  (void)d_leaf;
  const rbf_state *st = rbf_of(interp);
  if (!st->d_w || st->nf == 0) GSL_ERROR("gsl_sinterp_eval: interpolant not initialised", GSL_EINVAL);
  if (st->local_k) return local_eval_resident(interp, d_y, m, ytda, d_s, NULL, NULL);
  /* resident buffers live on ONE device: member 0 evaluates them (shard resident targets yourself with
     gsl_sinterp_hip_shard_bounds + one interpolant per device, as bench.py does per process) */
  HIP_TRY(rbf_sweep(st, st->ctx, st->d_x, st->d_w, d_y, m, ytda, d_s), st->ctx);
  return GSL_SUCCESS;
}

static int rbf_shard_eval(void *state, int member, const double *d_y, size_t m, double *d_s, int *d_leaf)
{
  (void)d_leaf;
  rbf_state *st = (rbf_state *)state;
  const double *model = st->m_model[member];
  return rbf_sweep(st, gsl_sinterp_hip_group_ctx(st->ss.grp, member), model, model + st->n * st->dim, d_y, m, st->dim, d_s);
}

static int rbf_chunk_eval(void *state, const double *d_y, size_t m, double *d_s, int *d_leaf)
{
  (void)d_leaf;
  const rbf_state *st = (const rbf_state *)state;
  return rbf_sweep(st, st->ctx, st->d_x, st->d_w, d_y, m, st->dim, d_s);
}

static int rbf_eval_many(const gsl_sinterp *interp, const gsl_matrix *y, gsl_vector *sv, int *leaf)
{
  rbf_state *st = rbf_of(interp);                       /* not const: the staging buffers are grow-only caches inside the state */
  if (!st->d_w || st->nf == 0) GSL_ERROR("gsl_sinterp_eval_many: interpolant not initialised", GSL_EINVAL);
  const size_t m = y->size1, dim = st->dim;
  if (m == 0) return GSL_SUCCESS;
  if (st->local_k) {
    if (leaf) for (size_t k = 0; k < m; k++) leaf[k] = -1;
    return local_eval_many(interp, y, sv, NULL, NULL);
  }
  if (st->ss.grp) {
    int sst = shard_eval_many(&st->ss, dim, y, sv, NULL, &rbf_shard_eval, st, 0, NULL);
    if (sst != GSL_SUCCESS) GSL_ERROR("gsl_sinterp_eval_many: sharded evaluation failed", sst);
  } else {
    int s = chunk_eval_many(&st->cs, st->ctx, dim, y, sv, NULL, &rbf_chunk_eval, st, 0, NULL);
    if (s != GSL_SUCCESS) GSL_ERROR("gsl_sinterp_eval_many: evaluation failed", s);
  }
  if (leaf) for (size_t k = 0; k < m; k++) leaf[k] = -1;
  return GSL_SUCCESS;
}

/* ---- local kriging (gsl_sinterp_set_neighbours; DESIGN.md, "Local kriging") ---- */
/* init with k > 0: centres and responses go to the (first) device and are binned; nothing is factored */
static int local_init(gsl_sinterp *interp, const gsl_matrix *x, const gsl_vector *f)
{
  rbf_state *st = rbf_of(interp);
  const size_t n = st->n, dim = st->dim;
  if (interp->drift > 1)
    GSL_ERROR("gsl_sinterp_init: the local route (gsl_sinterp_set_neighbours) takes a linear drift only", GSL_EUNSUP);
  if (interp->drift == 1 && interp->neighbours < dim + 2)
    GSL_ERROR("gsl_sinterp_init: local kriging with a linear drift needs at least dim + 2 neighbours", GSL_EINVAL);
  rbf_release_variance(st);
  rbf_release_loo(st);
  int s = rbf_prepare_devices(interp, st, 1);
  if (s) return s;
  st->nf = 0; st->local_k = 0; st->drift = 0; st->drift_q = 0; st->local_drift = 0;
  gsl_sinterp_hip_ctx *c = st->ctx;
  st->model_id = next_model_id();
  st->eps = interp->shape > 0 ? interp->shape : rbf_default_eps(st->kind, n, dim);
  double *h = (double *)malloc(n * (dim + 1) * sizeof(double));
  if (!h) GSL_ERROR("gsl_sinterp_init: out of memory", GSL_ENOMEM);
  for (size_t i = 0; i < n; i++) {
    for (size_t cdim = 0; cdim < dim; cdim++) h[i * dim + cdim] = x->data[i * x->tda + cdim];
    h[n * dim + i] = f->data[i * f->stride];
  }
  s = gsl_sinterp_hip_h2d(c, st->d_x, h, n * (dim + 1) * sizeof(double));        /* one buffer: [centres | responses] */
  if (!s) s = gsl_sinterp_hip_local_pack(c, st->d_x, n, (int)dim, dim, st->d_w, st->model_id);
  if (!s) s = gsl_sinterp_hip_sync(c);
  free(h);
  HIP_TRY(s, c);
  memset(st->f_mean, 0, sizeof st->f_mean); memset(st->f_poly, 0, sizeof st->f_poly);
  st->mean = GSL_NAN;                                   /* every neighbourhood estimates its own */
  interp->rcond = GSL_NAN; interp->route = 11;
  st->local_k = interp->neighbours; st->local_nugget = interp->nugget; st->local_drift = interp->drift;
  st->nf = 1;
  return GSL_SUCCESS;
}

/* value / variance (clamped at 0) / neighbour indices, each optional, from one pass on member 0 */
static int local_eval_resident(const gsl_sinterp *interp, const double *d_y, size_t m, size_t ytda, double *d_s, double *d_var, int *d_idx)
{
  const rbf_state *st = rbf_of(interp);
  if (m == 0) return GSL_SUCCESS;
  if (!d_y) GSL_ERROR("gsl_sinterp_eval: null argument", GSL_EFAULT);
  int s = (st->local_drift ? gsl_sinterp_hip_local_ukrige : gsl_sinterp_hip_local_krige)(st->ctx, st->kind, st->eps, st->local_nugget, st->d_x, st->n,
                                                                                          (int)st->dim, st->dim, st->d_w, d_y, m, ytda, st->local_k,
                                                                                          d_s, d_var, d_idx, NULL, st->model_id);
  if ((s == GSL_SUCCESS || s == GSL_EDOM) && d_var)     /* rounding residue where sigma^2 = 0; NaN stays NaN */
    HIP_TRY(gsl_sinterp_hip_krige_variance_clamp(st->ctx, d_var, m), st->ctx);
  if (s == GSL_EDOM)
    GSL_ERROR(st->local_drift ? "gsl_sinterp_eval: local kriging: a neighbourhood's covariance matrix is not positive definite, or its sites do not determine the drift (NaN at those targets)"
                              : "gsl_sinterp_eval: local kriging: the covariance matrix of a neighbourhood is not positive definite (NaN at those targets)",
              GSL_EDOM);
  HIP_TRY(s, st->ctx);
  return GSL_SUCCESS;
}

static int local_eval_many(const gsl_sinterp *interp, const gsl_matrix *y, gsl_vector *sv, gsl_vector *var, int *idx)
{
  const rbf_state *st = rbf_of(interp);
  gsl_sinterp_hip_ctx *c = st->ctx;
  const size_t m = y->size1, dim = st->dim, k = st->local_k;
  if (m == 0) return GSL_SUCCESS;
  stage_out out[3] = {STAGE_VECTOR(sv), STAGE_VECTOR(var), STAGE_INTS(idx, idx ? k : 0)};
  host_stage hs;
  int s = host_stage_begin(&hs, c, y, dim, out, 3), es = GSL_SUCCESS;
  if (!hs.h) GSL_ERROR("gsl_sinterp_eval_many: out of memory", GSL_ENOMEM);
  if (!s) es = local_eval_resident(interp, hs.d_y, m, dim, (double *)out[0].d, (double *)out[1].d, (int *)out[2].d);
  /* EDOM: everything has been stored, NaN where a pivot failed */
  s = host_stage_end(&hs, s, es == GSL_SUCCESS || es == GSL_EDOM);
  HIP_TRY(s, c);
  return es;                                            /* reported by the resident entry */
}

/* ======================================================================== */
/* linear simplex (barycentric) type                                         */
/* ======================================================================== */
typedef struct {
  size_t n;
  simplex_tree *tree;
  simplex_tree_device *dev;
  gsl_matrix *x; /* private copy of the centres: the tree keeps pointers into it */
  gsl_vector *f; /* private copy of the response (checkpoints); field 0 after gsl_sinterp_linear_init_fields */
  size_t nf;     /* fields held: 0 before the first init, 1 after init / fread, K after gsl_sinterp_linear_init_fields */
} simplex_state;
static simplex_state *tree_of(const gsl_sinterp *interp);

static void *simplex_alloc(size_t dim, size_t size)
{
  if (dim != 2) return NULL;
  simplex_state *st = (simplex_state *)calloc(1, sizeof *st);
  if (st) st->n = size;
  return st;
}

static void simplex_free(void *vstate)
{
  simplex_state *st = (simplex_state *)vstate;
  if (!st) return;
  simplex_tree_device_free(st->dev);
  simplex_tree_free(st->tree);
  gsl_matrix_free(st->x);
  gsl_vector_free(st->f);
  free(st);
}

/* mirror st->tree (built over st->x) on the interpolant's device(s) and bind st->f */
static int simplex_mirror(gsl_sinterp *interp, simplex_state *st)
{
  simplex_tree_device_free(st->dev);
  st->dev = interp->n_devices > 1 ? simplex_tree_device_alloc_multi(st->tree, st->x, interp->devices, interp->n_devices)
                                  : simplex_tree_device_alloc(st->tree, st->x, interp->device);
  st->nf = 0;
  if (!st->dev) return GSL_EFAILED;
  int s = simplex_tree_device_set_response(st->dev, st->f);
  if (!s) st->nf = 1;
  return s;
}

static int simplex_init(gsl_sinterp *interp, const gsl_matrix *x, const gsl_vector *f)
{
  simplex_state *st = tree_of(interp);
  simplex_tree_device_free(st->dev); st->dev = NULL;
  simplex_tree_free(st->tree); st->tree = NULL;
  gsl_matrix_free(st->x);
  st->x = gsl_matrix_alloc(st->n, 2);
  if (!st->x) return GSL_ENOMEM;
  for (size_t i = 0; i < st->n; i++) {
    gsl_matrix_set(st->x, i, 0, x->data[i * x->tda]);
    gsl_matrix_set(st->x, i, 1, x->data[i * x->tda + 1]);
  }
  st->tree = simplex_tree_alloc(2, (int)st->n);
  if (!st->tree) return GSL_ENOMEM;
  int s = simplex_tree_init(st->tree, st->x, NULL, NULL, interp->init_flags, interp->rng);
  if (s != GSL_SUCCESS) return s;
  gsl_vector_free(st->f);
  st->f = gsl_vector_alloc(st->n);
  if (!st->f) return GSL_ENOMEM;
  for (size_t i = 0; i < st->n; i++) gsl_vector_set(st->f, i, gsl_vector_get(f, i));
  return simplex_mirror(interp, st);
}

static int simplex_eval_many(const gsl_sinterp *interp, const gsl_matrix *y, gsl_vector *s, int *leaf)
{
  const simplex_state *st = tree_of(interp);
  if (!st->dev) GSL_ERROR("gsl_sinterp_eval_many: interpolant not initialised", GSL_EINVAL);
  return simplex_tree_device_eval_many(st->dev, y, s, leaf);
}

static int simplex_eval_resident(const gsl_sinterp *interp, const double *d_y, size_t m, size_t ytda,
                                 double *d_s, int *d_leaf)
{
  const simplex_state *st = tree_of(interp);
  if (!st->dev) GSL_ERROR("gsl_sinterp_eval_resident: interpolant not initialised", GSL_EINVAL);
  return simplex_tree_device_eval_resident(st->dev, d_y, m, ytda, d_s, d_leaf);
}

/* ======================================================================== */
/* the mesh-state types: linear, natural-neighbour or Clough-Tocher on a      */
/* mesh that is imported (README:28-31: QHull / CGAL meshes) or exported     */
/* from a host-built tree                                                    */
/* ======================================================================== */
typedef struct {
  size_t n, dim;             /* dim = 2 (triangles) or 3 (tetrahedra) */
  int *tri, *nbr;            /* the caller's triangulation (gsl_sinterp_set_triangulation), copied: [(dim + 1) n_tri] */
  size_t n_tri;
  simplex_mesh *mesh;
  simplex_mesh_device *dev;
  gsl_matrix *x;             /* private copies (checkpoints) */
  gsl_vector *f;
  size_t nf;                 /* the linear types: fields held (0 before the first init, 1 after init / fread, K after
                                gsl_sinterp_linear_init_fields) */
  /* the Clough-Tocher types only: g_set = the caller's gradients (gsl_sinterp_set_gradients; NULL = estimate), g = the
     gradients in use after init / fread, the stopping rule of the estimate (0 = the mirror's defaults) and what it took */
  gsl_matrix *g_set, *g;
  double g_rtol, g_resid;
  size_t g_maxiter, g_iters;
} mesh_state;

static mesh_state *mesh_of(const gsl_sinterp *interp);

static void *mesh_type_alloc(size_t dim, size_t size)
{
  if (dim != 2 && dim != 3) return NULL;                /* the natural and cubic types: dim = 2 only, refused by gsl_sinterp_alloc */
  mesh_state *st = (mesh_state *)calloc(1, sizeof *st);
  if (st) { st->n = size; st->dim = dim; }
  return st;
}

static void mesh_type_free(void *vstate)
{
  mesh_state *st = (mesh_state *)vstate;
  if (!st) return;
  simplex_mesh_device_free(st->dev);
  simplex_mesh_free(st->mesh);
  gsl_matrix_free(st->x);
  gsl_vector_free(st->f);
  if (st->g_set) gsl_matrix_free(st->g_set);
  if (st->g) gsl_matrix_free(st->g);
  free(st->tri); free(st->nbr);
  free(st);
}

/* Mirror st->mesh on the interpolant's device(s) and bind st->f: the last step of init and of gsl_sinterp_fread.  What
   the device entries of a method would refuse at every evaluation is refused once, here.  Clough-Tocher: then the
   gradients, `known` (the caller's, or a checkpoint's) or the estimate, which runs here so that
   gsl_sinterp_get_gradients and a GSL_EMAXITER verdict belong to init. */
static int mesh_type_mirror(gsl_sinterp *interp, mesh_state *st, const gsl_matrix *known)
{
  const type_desc *d = desc_of(interp->type);
  if (d->noun && interp->n_devices > 1) return noun_error(d, "gsl_sinterp_init: %s interpolants run on one device", GSL_EUNSUP);
  if (d->method == MESH_NATURAL) {
    if (!simplex_mesh_convex(st->mesh)) GSL_ERROR("gsl_sinterp_init: natural neighbours need a convex mesh", GSL_EUNSUP);
    if (simplex_mesh_delaunay_metric(st->mesh) == 0)
      GSL_ERROR("gsl_sinterp_init: natural neighbours need a Delaunay triangulation (simplex_mesh_delaunay_metric is 0)", GSL_EINVAL);
  }
  simplex_mesh_device_free(st->dev);
  st->nf = 0;
  st->dev = interp->n_devices > 1 ? simplex_mesh_device_alloc_multi(st->mesh, interp->devices, interp->n_devices)
                                  : simplex_mesh_device_alloc(st->mesh, interp->device);
  if (!st->dev) return GSL_EFAILED;
  int s = simplex_mesh_device_set_response(st->dev, st->f);
  if (!s) st->nf = 1;
  if (s || d->method != MESH_CUBIC) return s;
  if (st->g_rtol > 0.0) s = simplex_mesh_device_set_gradient_options(st->dev, st->g_rtol, st->g_maxiter);
  if (!s) s = simplex_mesh_device_bind_gradients(st->dev, known);
  if (s) return s;
  if (st->g) gsl_matrix_free(st->g);
  st->g = gsl_matrix_alloc(st->n, 2);
  if (!st->g) return GSL_ENOMEM;
  return simplex_mesh_device_gradients(st->dev, st->g, &st->g_iters, &st->g_resid);
}

/* every mesh-state type: checks, private copies of the data, the mesh (imported, or the tree of gsl_sinterp_linear_simplex --
   same flags, same generator -- exported and dropped: the mesh is all that is kept), the mirror */
static int mesh_type_init(gsl_sinterp *interp, const gsl_matrix *x, const gsl_vector *f)
{
  mesh_state *st = mesh_of(interp);
  const int imported = desc_of(interp->type)->imported;
  if (imported && !st->tri) GSL_ERROR("gsl_sinterp_init: no triangulation set (gsl_sinterp_set_triangulation)", GSL_EINVAL);
  if (imported && st->n < st->dim + 1) GSL_ERROR("gsl_sinterp_init: an imported triangulation needs at least dim + 1 points", GSL_EINVAL);
  simplex_mesh_device_free(st->dev); st->dev = NULL;
  simplex_mesh_free(st->mesh); st->mesh = NULL;
  gsl_matrix_free(st->x); gsl_vector_free(st->f);
  st->x = gsl_matrix_alloc(st->n, st->dim);
  st->f = gsl_vector_alloc(st->n);
  if (!st->x || !st->f) return GSL_ENOMEM;
  for (size_t i = 0; i < st->n; i++) {
    for (size_t j = 0; j < st->dim; j++) gsl_matrix_set(st->x, i, j, x->data[i * x->tda + j]);
    gsl_vector_set(st->f, i, gsl_vector_get(f, i));
  }
  if (imported) {
    st->mesh = simplex_mesh_import_nd(st->x, st->dim, st->tri, st->nbr, st->n_tri);
  } else {
    simplex_tree *tree = simplex_tree_alloc(2, (int)st->n);
    if (!tree) return GSL_ENOMEM;
    int s = simplex_tree_init(tree, st->x, NULL, NULL, interp->init_flags, interp->rng);
    if (s == GSL_SUCCESS) st->mesh = simplex_mesh_from_tree(tree, st->x);
    simplex_tree_free(tree);
    if (s != GSL_SUCCESS) return s;
  }
  if (!st->mesh) return GSL_EINVAL;
  return mesh_type_mirror(interp, st, st->g_set);
}

static int mesh_type_eval_many(const gsl_sinterp *interp, const gsl_matrix *y, gsl_vector *s, int *leaf)
{
  const mesh_state *st = mesh_of(interp);
  if (!st->dev) GSL_ERROR("gsl_sinterp_eval_many: interpolant not initialised", GSL_EINVAL);
  switch (desc_of(interp->type)->method) {
    case MESH_NATURAL: return simplex_mesh_device_eval_natural_many(st->dev, y, s, leaf);
    case MESH_CUBIC: return simplex_mesh_device_eval_cubic_many(st->dev, y, s, NULL, leaf);
    default: return simplex_mesh_device_eval_many(st->dev, y, s, leaf);
  }
}

static int mesh_type_eval_resident(const gsl_sinterp *interp, const double *d_y, size_t m, size_t ytda, double *d_s, int *d_leaf)
{
  const mesh_state *st = mesh_of(interp);
  if (!st->dev) GSL_ERROR("gsl_sinterp_eval_resident: interpolant not initialised", GSL_EINVAL);
  switch (desc_of(interp->type)->method) {
    case MESH_NATURAL: return simplex_mesh_device_eval_natural_resident(st->dev, d_y, m, ytda, d_s, d_leaf);
    case MESH_CUBIC: return simplex_mesh_device_eval_cubic_resident(st->dev, d_y, m, ytda, d_s, NULL, 0, d_leaf);
    default: return simplex_mesh_device_eval_resident(st->dev, d_y, m, ytda, d_s, d_leaf);
  }
}

/* ======================================================================== */
/* modified quadratic Shepard (csrc/hip/shepard.hip; DESIGN.md 4, "Modified    */
/* Shepard"): the fit at init, one sweep per evaluation, one device           */
/* ======================================================================== */
typedef struct {
  size_t n, dim, nc;         /* nc = 5 (dim 2) or 9 (dim 3) coefficients per node */
  size_t nq_set, nw_set;     /* gsl_sinterp_set_shepard; 0 = the default of the dimension */
  size_t nq, nw;             /* of the model held */
  gsl_sinterp_hip_ctx *ctx;
  double *d_model;           /* one buffer: [x n dim | f n | Rq n | Rw n | c n nc] */
  int ready;                 /* a model is held (init or fread succeeded) */
  unsigned long long model_id;
  size_t n_linear, n_constant;
  double rw_max;
} shepard_state;
static shepard_state *shepard_of(const gsl_sinterp *interp);

static double *shep_f(const shepard_state *st) { return st->d_model + st->n * st->dim; }
static double *shep_rq(const shepard_state *st) { return shep_f(st) + st->n; }
static double *shep_rw(const shepard_state *st) { return shep_rq(st) + st->n; }
static double *shep_coef(const shepard_state *st) { return shep_rw(st) + st->n; }
static size_t shep_model_doubles(const shepard_state *st) { return st->n * (st->dim + 3 + st->nc); }

static void *shepard_alloc(size_t dim, size_t size)
{
  if (dim != 2 && dim != 3) return NULL;                /* refused by gsl_sinterp_alloc */
  shepard_state *st = (shepard_state *)calloc(1, sizeof *st);
  if (st) { st->n = size; st->dim = dim; st->nc = dim == 2 ? 5 : 9; }
  return st;
}

static void shepard_free(void *vstate)
{
  shepard_state *st = (shepard_state *)vstate;
  if (!st) return;
  if (st->ctx) {
    gsl_sinterp_hip_free(st->ctx, st->d_model);
    gsl_sinterp_hip_ctx_destroy(st->ctx);
  }
  free(st);
}

/* the context on the interpolant's device and the model buffer; the model held so far is dropped */
static int shepard_prepare(gsl_sinterp *interp, shepard_state *st)
{
  st->ready = 0;
  if (interp->n_devices > 1) GSL_ERROR("gsl_sinterp_init: modified Shepard interpolants run on one device", GSL_EUNSUP);
  if (st->ctx && gsl_sinterp_hip_ctx_device(st->ctx) != interp->device) {
    gsl_sinterp_hip_free(st->ctx, st->d_model);
    gsl_sinterp_hip_ctx_destroy(st->ctx);
    st->ctx = NULL; st->d_model = NULL;
  }
  if (!st->ctx && gsl_sinterp_hip_ctx_create(&st->ctx, interp->device, NULL) != GSL_SUCCESS) {
    st->ctx = NULL;
    GSL_ERROR("gsl_sinterp_init: no usable HIP device (GPU path has no CPU fallback)", GSL_EFAILED);
  }
  if (!st->d_model) HIP_TRY(gsl_sinterp_hip_malloc(st->ctx, (void **)&st->d_model, shep_model_doubles(st) * sizeof(double)), st->ctx);
  st->model_id = next_model_id();                       /* the buffer is about to change */
  return GSL_SUCCESS;
}

static int shepard_init(gsl_sinterp *interp, const gsl_matrix *x, const gsl_vector *f)
{
  shepard_state *st = shepard_of(interp);
  const size_t n = st->n, dim = st->dim;
  const size_t nq = st->nq_set ? st->nq_set : (dim == 2 ? 13 : 17), nw = st->nw_set ? st->nw_set : (dim == 2 ? 19 : 32);   /* Renka's defaults */
  if (n < (nq > nw ? nq : nw) + 2) GSL_ERROR("gsl_sinterp_init: modified Shepard needs size >= max(nq, nw) + 2", GSL_EINVAL);
  int s = shepard_prepare(interp, st);
  if (s) return s;
  gsl_sinterp_hip_ctx *c = st->ctx;
  double *h = (double *)malloc(n * (dim + 1) * sizeof(double));
  if (!h) GSL_ERROR("gsl_sinterp_init: out of memory", GSL_ENOMEM);
  for (size_t i = 0; i < n; i++) {
    for (size_t a = 0; a < dim; a++) h[i * dim + a] = x->data[i * x->tda + a];
    h[n * dim + i] = f->data[i * f->stride];
  }
  size_t counts[3] = {0, 0, 0};
  s = gsl_sinterp_hip_h2d(c, st->d_model, h, n * (dim + 1) * sizeof(double));
  if (!s) s = gsl_sinterp_hip_shepard_fit(c, st->d_model, n, (int)dim, dim, shep_f(st), nq, nw, shep_rq(st), shep_rw(st), shep_coef(st), counts);
  if (!s) s = gsl_sinterp_hip_d2h(c, h, shep_rw(st), n * sizeof(double));
  double big = 0.0;
  if (!s) for (size_t i = 0; i < n; i++) if (h[i] > big) big = h[i];
  free(h);
  if (s == GSL_EDOM) GSL_ERROR("gsl_sinterp_init: coincident sites (modified Shepard weights are undefined at distance 0)", GSL_EDOM);
  HIP_TRY(s, c);
  st->nq = nq; st->nw = nw; st->n_linear = counts[0]; st->n_constant = counts[1]; st->rw_max = big;
  st->ready = 1;
  return GSL_SUCCESS;
}

/* value / gradient / leaf, each optional, from one sweep; uncovered targets are the status */
static int shepard_sweep(const shepard_state *st, const double *d_y, size_t m, size_t ytda, double *d_s, double *d_g, size_t gtda, int *d_leaf)
{
  size_t outside = 0;
  int s = gsl_sinterp_hip_shepard_eval(st->ctx, st->d_model, st->n, (int)st->dim, st->dim, shep_f(st), shep_rq(st), shep_rw(st), shep_coef(st),
                                       d_y, m, ytda, d_s, d_g, gtda, d_leaf, &outside, st->model_id);
  if (s == GSL_EDOM) GSL_ERROR("gsl_sinterp_eval: target(s) outside every node's radius of influence (NaN there)", GSL_EDOM);
  HIP_TRY(s, st->ctx);
  return GSL_SUCCESS;
}

static int shepard_eval_resident(const gsl_sinterp *interp, const double *d_y, size_t m, size_t ytda, double *d_s, int *d_leaf)
{
  const shepard_state *st = shepard_of(interp);
  if (!st->ready) GSL_ERROR("gsl_sinterp_eval_resident: interpolant not initialised", GSL_EINVAL);
  if (m == 0) return GSL_SUCCESS;
  if (!d_y || !d_s) GSL_ERROR("gsl_sinterp_eval_resident: null argument", GSL_EFAULT);
  if (ytda < st->dim) GSL_ERROR("gsl_sinterp_eval_resident: target rows shorter than dim", GSL_EBADLEN);
  return shepard_sweep(st, d_y, m, ytda, d_s, NULL, 0, d_leaf);
}

/* host batch: values (or NULL), gradient (or NULL), leaf (or NULL) through plain staging */
static int shepard_eval_host(const shepard_state *st, const gsl_matrix *y, gsl_vector *sv, gsl_matrix *g, int *leaf)
{
  const size_t m = y->size1, dim = st->dim;
  if (m == 0) return GSL_SUCCESS;
  stage_out out[3] = {STAGE_VECTOR(sv), {g ? dim : 0, 0, g ? g->data : NULL, g ? g->tda : 0, NULL, NULL}, STAGE_INTS(leaf, leaf ? 1 : 0)};
  host_stage hs;
  int s = host_stage_begin(&hs, st->ctx, y, dim, out, 3), es = GSL_SUCCESS;
  if (!hs.h) GSL_ERROR("gsl_sinterp_eval_many: out of memory", GSL_ENOMEM);
  if (!s) es = shepard_sweep(st, hs.d_y, m, dim, (double *)out[0].d, (double *)out[1].d, dim, (int *)out[2].d);
  s = host_stage_end(&hs, s, es == GSL_SUCCESS || es == GSL_EDOM);     /* EDOM: everything has been stored, NaN where uncovered */
  HIP_TRY(s, st->ctx);
  return es;                                            /* reported by shepard_sweep */
}

static int shepard_eval_many(const gsl_sinterp *interp, const gsl_matrix *y, gsl_vector *s, int *leaf)
{
  const shepard_state *st = shepard_of(interp);
  if (!st->ready) GSL_ERROR("gsl_sinterp_eval_many: interpolant not initialised", GSL_EINVAL);
  return shepard_eval_host(st, y, s, NULL, leaf);
}

/* ======================================================================== */
/* type table + generic entry points                                         */
/* ======================================================================== */
#define RBF_ROW(name, min_size, id, kind, krige, affine, pd)                                                       \
  {{name, min_size, &rbf_alloc, &rbf_init, &rbf_eval_many, &rbf_eval_resident, &rbf_free}, id, FAM_RBF, kind, krige, affine, pd, 0, 0, NULL}
#define MESH_ROW(name, id, method, imported, noun)                                                                 \
  {{name, 3, &mesh_type_alloc, &mesh_type_init, &mesh_type_eval_many, &mesh_type_eval_resident, &mesh_type_free}, id, FAM_MESH, 0, 0, 0, 0, \
   method, imported, noun}
/* one row per type, in the order of the checkpoint ids.  The checkpoints of 12 / 13 have the payload of 6, those of
   14 / 15 the same + the 2 N gradients; 16 has a payload of its own (gsl_sinterp_fwrite) */
static const type_desc type_table[] = {
  RBF_ROW("rbf-gaussian", 1, 0, GSL_SINTERP_RBF_GAUSSIAN, 0, 0, 1),
  RBF_ROW("rbf-thin-plate-spline", 1, 1, GSL_SINTERP_RBF_TPS, 0, 0, 0),
  {{"linear-simplex", 3, &simplex_alloc, &simplex_init, &simplex_eval_many, &simplex_eval_resident, &simplex_free}, 2, FAM_TREE, 0, 0, 0, 0, 0, 0, NULL},
  RBF_ROW("rbf-wendland-c2", 1, 3, GSL_SINTERP_RBF_WENDLAND, 0, 0, 1),
  RBF_ROW("ordinary-kriging-gaussian", 1, 4, GSL_SINTERP_RBF_GAUSSIAN, 1, 0, 1),
  RBF_ROW("rbf-thin-plate-spline-affine", 3, 5, GSL_SINTERP_RBF_TPS, 0, 1, 0),
  MESH_ROW("linear-imported-triangulation", 6, MESH_LINEAR, 1, NULL),
  RBF_ROW("rbf-matern-3/2", 1, 7, GSL_SINTERP_RBF_MATERN32, 0, 0, 1),
  RBF_ROW("rbf-matern-5/2", 1, 8, GSL_SINTERP_RBF_MATERN52, 0, 0, 1),
  RBF_ROW("rbf-inverse-multiquadric", 1, 9, GSL_SINTERP_RBF_IMQ, 0, 0, 1),
  RBF_ROW("ordinary-kriging-matern-3/2", 1, 10, GSL_SINTERP_RBF_MATERN32, 1, 0, 1),
  RBF_ROW("ordinary-kriging-matern-5/2", 1, 11, GSL_SINTERP_RBF_MATERN52, 1, 0, 1),
  MESH_ROW("natural-neighbour-imported-triangulation", 12, MESH_NATURAL, 1, "natural-neighbour"),
  MESH_ROW("natural-neighbour-simplex", 13, MESH_NATURAL, 0, "natural-neighbour"),
  MESH_ROW("clough-tocher-imported-triangulation", 14, MESH_CUBIC, 1, "Clough-Tocher"),
  MESH_ROW("clough-tocher-simplex", 15, MESH_CUBIC, 0, "Clough-Tocher"),
  {{"modified-quadratic-shepard", 7, &shepard_alloc, &shepard_init, &shepard_eval_many, &shepard_eval_resident, &shepard_free}, 16, FAM_SHEPARD,
   0, 0, 0, 0, 0, 0, "modified Shepard"},
};
#define N_TYPES (sizeof type_table / sizeof type_table[0])
const gsl_sinterp_type *gsl_sinterp_rbf_gaussian = &type_table[0].pub;
const gsl_sinterp_type *gsl_sinterp_rbf_tps = &type_table[1].pub;
const gsl_sinterp_type *gsl_sinterp_linear_simplex = &type_table[2].pub;
const gsl_sinterp_type *gsl_sinterp_rbf_wendland = &type_table[3].pub;
const gsl_sinterp_type *gsl_sinterp_kriging = &type_table[4].pub;
const gsl_sinterp_type *gsl_sinterp_rbf_tps_affine = &type_table[5].pub;
const gsl_sinterp_type *gsl_sinterp_linear_mesh = &type_table[6].pub;
const gsl_sinterp_type *gsl_sinterp_rbf_matern32 = &type_table[7].pub;
const gsl_sinterp_type *gsl_sinterp_rbf_matern52 = &type_table[8].pub;
const gsl_sinterp_type *gsl_sinterp_rbf_imq = &type_table[9].pub;
const gsl_sinterp_type *gsl_sinterp_kriging_matern32 = &type_table[10].pub;
const gsl_sinterp_type *gsl_sinterp_kriging_matern52 = &type_table[11].pub;
const gsl_sinterp_type *gsl_sinterp_natural_mesh = &type_table[12].pub;
const gsl_sinterp_type *gsl_sinterp_natural_simplex = &type_table[13].pub;
const gsl_sinterp_type *gsl_sinterp_cubic_mesh = &type_table[14].pub;
const gsl_sinterp_type *gsl_sinterp_cubic_simplex = &type_table[15].pub;
const gsl_sinterp_type *gsl_sinterp_shepard = &type_table[16].pub;

static const type_desc *desc_of(const gsl_sinterp_type *T)
{
  for (size_t i = 0; i < N_TYPES; i++)
    if (T == &type_table[i].pub) return &type_table[i];
  return NULL;
}

/* the state as its family's struct; NULL for an interpolant of another family.  gsl_sinterp_alloc admits the rows of the
   table only, so desc_of(interp->type) is never NULL */
static rbf_state *rbf_of(const gsl_sinterp *interp) { return desc_of(interp->type)->family == FAM_RBF ? (rbf_state *)interp->state : NULL; }
static simplex_state *tree_of(const gsl_sinterp *interp) { return desc_of(interp->type)->family == FAM_TREE ? (simplex_state *)interp->state : NULL; }
static mesh_state *mesh_of(const gsl_sinterp *interp) { return desc_of(interp->type)->family == FAM_MESH ? (mesh_state *)interp->state : NULL; }
static shepard_state *shepard_of(const gsl_sinterp *interp) { return desc_of(interp->type)->family == FAM_SHEPARD ? (shepard_state *)interp->state : NULL; }
static int mesh_method(const gsl_sinterp *interp, int method) { return mesh_of(interp) && desc_of(interp->type)->method == method; }

/* whether the interpolant is on, or will at the next init be on, the local route (route 11): asked by every entry that
   needs the global model, before anything touches the device */
static int is_local(const gsl_sinterp *interp)
{
  return desc_of(interp->type)->krige && (interp->neighbours > 0 || rbf_of(interp)->local_k > 0);
}

int gsl_sinterp_set_neighbours(gsl_sinterp *interp, size_t k)
{
  if (!interp) GSL_ERROR("gsl_sinterp_set_neighbours: null interpolant", GSL_EFAULT);
  const type_desc *d = desc_of(interp->type);
  if (d->noun) return noun_error(d, "gsl_sinterp_set_neighbours: not for %s interpolants", GSL_EUNSUP);
  if (!d->krige) GSL_ERROR("gsl_sinterp_set_neighbours: kriging interpolants only", GSL_EINVAL);
  if (k > GSL_SINTERP_MAX_NEIGHBOURS) GSL_ERROR("gsl_sinterp_set_neighbours: at most 64 neighbours", GSL_EINVAL);
  if (k > interp->size) GSL_ERROR("gsl_sinterp_set_neighbours: more neighbours than centres", GSL_EINVAL);
  interp->neighbours = k;
  return GSL_SUCCESS;
}

gsl_sinterp *gsl_sinterp_alloc(const gsl_sinterp_type *T, size_t dim, size_t size)
{
  if (!T) GSL_ERROR_NULL("gsl_sinterp_alloc: null type", GSL_EFAULT);
  const type_desc *d = desc_of(T);
  if (!d) GSL_ERROR_NULL("gsl_sinterp_alloc: not one of the gsl_sinterp types", GSL_EINVAL);
  if (size < T->min_size)
    GSL_ERROR_NULL("insufficient number of points for interpolation type", GSL_EINVAL);
  if (d->family == FAM_SHEPARD && dim != 2 && dim != 3)
    GSL_ERROR_NULL("gsl_sinterp_alloc: modified Shepard interpolants support dim = 2 and 3 only", GSL_EUNIMPL);
  if (dim < 1 || dim > 3) GSL_ERROR_NULL("gsl_sinterp_alloc: dim must be 1, 2 or 3", GSL_EINVAL);
  if (d->family == FAM_TREE && dim != 2)
    GSL_ERROR_NULL("gsl_sinterp_alloc: linear-simplex supports dim = 2 only", GSL_EUNIMPL);
  if (d->family == FAM_MESH && d->noun && dim != 2) {
    noun_error(d, "gsl_sinterp_alloc: %s interpolants support dim = 2 only", GSL_EUNIMPL);
    return NULL;
  }
  gsl_sinterp *interp = (gsl_sinterp *)calloc(1, sizeof *interp);
  if (!interp) GSL_ERROR_NULL("failed to allocate space for sinterp struct", GSL_ENOMEM);
  interp->type = T; interp->dim = dim; interp->size = size;
  interp->device = default_device();
  interp->n_devices = env_device_list(interp->devices);   /* GSL_SINTERP_DEVICES: count or list; 0 = single device */
  /* GSL_SINTERP_DEVICES = "1" (a COUNT of one) selects no ordinal: GSL_SINTERP_DEVICE keeps naming the device */
  if (interp->n_devices == 1 && getenv("GSL_SINTERP_DEVICES") && !strchr(getenv("GSL_SINTERP_DEVICES"), ',')) interp->n_devices = 0;
  if (interp->n_devices >= 1) interp->device = interp->devices[0];
  else { interp->n_devices = 1; interp->devices[0] = interp->device; }
  interp->shape = 0.0; interp->init_flags = SIMPLEX_TREE_DEFAULT; interp->rng = NULL;
  interp->solver = GSL_SINTERP_SOLVER_DEFAULT; interp->want_rcond = 0; interp->rcond = GSL_NAN; interp->route = 0;
  interp->state = T->alloc(dim, size);
  if (!interp->state) {
    free(interp);
    GSL_ERROR_NULL("failed to allocate space for sinterp state", GSL_ENOMEM);
  }
  rbf_state *st = rbf_of(interp);
  if (st) { st->kind = d->kind; st->krige = d->krige; st->affine = d->affine; }
  return interp;
}

int gsl_sinterp_set_device(gsl_sinterp *interp, int device)
{
  if (!interp) GSL_ERROR("gsl_sinterp_set_device: null interpolant", GSL_EFAULT);
  if (device < 0) GSL_ERROR("gsl_sinterp_set_device: negative ordinal", GSL_EINVAL);
  interp->device = device;
  interp->n_devices = 1; interp->devices[0] = device;
  return GSL_SUCCESS;
}

/* Evaluate on `n_devices` GPUs (ordinals 0 .. n_devices-1): the next gsl_sinterp_init solves on the first,
   replicates the model with one broadcast and gsl_sinterp_eval_many shards its targets. */
int gsl_sinterp_set_devices(gsl_sinterp *interp, int n_devices)
{
  if (!interp) GSL_ERROR("gsl_sinterp_set_devices: null interpolant", GSL_EFAULT);
  if (n_devices < 1 || n_devices > GSL_SINTERP_MAX_DEVICES) GSL_ERROR("gsl_sinterp_set_devices: bad device count", GSL_EINVAL);
  for (int i = 0; i < n_devices; i++) interp->devices[i] = i;
  interp->n_devices = n_devices; interp->device = 0;
  return GSL_SUCCESS;
}

int gsl_sinterp_set_device_list(gsl_sinterp *interp, const int *devices, int n_devices)
{
  if (!interp || !devices) GSL_ERROR("gsl_sinterp_set_device_list: null argument", GSL_EFAULT);
  if (n_devices < 1 || n_devices > GSL_SINTERP_MAX_DEVICES) GSL_ERROR("gsl_sinterp_set_device_list: bad device count", GSL_EINVAL);
  for (int i = 0; i < n_devices; i++) {
    if (devices[i] < 0) GSL_ERROR("gsl_sinterp_set_device_list: negative ordinal", GSL_EINVAL);
    interp->devices[i] = devices[i];
  }
  interp->n_devices = n_devices; interp->device = devices[0];
  return GSL_SUCCESS;
}

int gsl_sinterp_n_devices(const gsl_sinterp *interp) { return interp ? interp->n_devices : 0; }

int gsl_sinterp_set_shape(gsl_sinterp *interp, double eps)
{
  if (!interp) GSL_ERROR("gsl_sinterp_set_shape: null interpolant", GSL_EFAULT);
  interp->shape = eps;
  return GSL_SUCCESS;
}

int gsl_sinterp_set_nugget(gsl_sinterp *interp, double nugget)
{
  if (!interp) GSL_ERROR("gsl_sinterp_set_nugget: null interpolant", GSL_EFAULT);
  if (!desc_of(interp->type)->krige) GSL_ERROR("gsl_sinterp_set_nugget: kriging interpolants only", GSL_EINVAL);
  if (!(nugget >= 0.0)) GSL_ERROR("gsl_sinterp_set_nugget: the nugget must be >= 0", GSL_EDOM);
  interp->nugget = nugget;
  return GSL_SUCCESS;
}

int gsl_sinterp_set_drift(gsl_sinterp *interp, int order)
{
  if (!interp) GSL_ERROR("gsl_sinterp_set_drift: null interpolant", GSL_EFAULT);
  if (!desc_of(interp->type)->krige) GSL_ERROR("gsl_sinterp_set_drift: kriging interpolants only", GSL_EINVAL);
  if (order < 0 || order > 2) GSL_ERROR("gsl_sinterp_set_drift: the order must be 0 (ordinary kriging), 1 or 2", GSL_EINVAL);
  interp->drift = order;
  return GSL_SUCCESS;
}

int gsl_sinterp_drift(const gsl_sinterp *interp) { return interp ? interp->drift : 0; }

size_t gsl_sinterp_drift_terms(size_t dim, int order)
{
  return dim > 3 ? 0 : gsl_sinterp_hip_drift_terms((int)dim, order);     /* the one definition, next to the term order (drift.hip) */
}

int gsl_sinterp_drift_coefficients(const gsl_sinterp *interp, size_t field, gsl_vector *c, gsl_vector *shift, gsl_vector *scale)
{
  if (!interp || !c) GSL_ERROR("gsl_sinterp_drift_coefficients: null argument", GSL_EFAULT);
  if (!desc_of(interp->type)->krige) GSL_ERROR("gsl_sinterp_drift_coefficients: kriging interpolants only", GSL_EINVAL);
  if (is_local(interp)) GSL_ERROR("gsl_sinterp_drift_coefficients: not with gsl_sinterp_set_neighbours", GSL_EUNSUP);
  const rbf_state *st = rbf_of(interp);
  if (!st->d_w || st->nf == 0) GSL_ERROR("gsl_sinterp_drift_coefficients: interpolant not initialised", GSL_EINVAL);
  if (!st->drift) GSL_ERROR("gsl_sinterp_drift_coefficients: initialised without a drift (gsl_sinterp_mean answers)", GSL_EINVAL);
  if (field >= st->nf) GSL_ERROR("gsl_sinterp_drift_coefficients: no such field", GSL_EINVAL);
  if (c->size != st->drift_q || (shift && shift->size != st->dim) || (scale && scale->size != st->dim))
    GSL_ERROR("gsl_sinterp_drift_coefficients: c needs gsl_sinterp_drift_terms entries, shift and scale dim", GSL_EBADLEN);
  for (size_t t = 0; t < st->drift_q; t++) gsl_vector_set(c, t, st->f_coef[field][t]);
  for (size_t a = 0; a < st->dim; a++) {
    if (shift) gsl_vector_set(shift, a, st->drift_shift[a]);
    if (scale) gsl_vector_set(scale, a, st->drift_scale[a]);
  }
  return GSL_SUCCESS;
}

int gsl_sinterp_set_variance(gsl_sinterp *interp, int want)
{
  if (!interp) GSL_ERROR("gsl_sinterp_set_variance: null interpolant", GSL_EFAULT);
  if (!desc_of(interp->type)->krige) GSL_ERROR("gsl_sinterp_set_variance: kriging interpolants only", GSL_EINVAL);
  interp->want_variance = want != 0;
  return GSL_SUCCESS;
}

int gsl_sinterp_set_loo(gsl_sinterp *interp, int want)
{
  if (!interp) GSL_ERROR("gsl_sinterp_set_loo: null interpolant", GSL_EFAULT);
  if (!desc_of(interp->type)->pd)
    GSL_ERROR("gsl_sinterp_set_loo: positive definite RBF (Gaussian, Wendland, Matern, inverse multiquadric) and kriging interpolants only", GSL_EINVAL);
  interp->want_loo = want != 0;
  return GSL_SUCCESS;
}

/* whether leave-one-out data is held, as a status (the table of include/gsl_sinterp.h) */
static int loo_status(const gsl_sinterp *interp)
{
  const type_desc *d = desc_of(interp->type);
  if (d->noun) return noun_error(d, "gsl_sinterp_loo: not for %s interpolants", GSL_EUNSUP);
  if (!d->pd)
    GSL_ERROR("gsl_sinterp_loo: positive definite RBF (Gaussian, Wendland, Matern, inverse multiquadric) and kriging interpolants only", GSL_EINVAL);
  if (is_local(interp)) GSL_ERROR("gsl_sinterp_loo: local kriging (gsl_sinterp_set_neighbours) takes a route without a Cholesky factor", GSL_EUNSUP);
  const rbf_state *st = rbf_of(interp);
  if (!st->d_w || st->nf == 0) GSL_ERROR("gsl_sinterp_loo: interpolant not initialised", GSL_EINVAL);
  if (st->loo_state == 3)
    GSL_ERROR("gsl_sinterp_loo: the interpolant was restored by gsl_sinterp_fread; a checkpoint carries no leave-one-out data", GSL_EINVAL);
  if (st->loo_state == 2)
    GSL_ERROR("gsl_sinterp_loo: the init took a route without a Cholesky factor", GSL_EUNSUP);
  if (st->loo_state == 4)
    GSL_ERROR("gsl_sinterp_loo: kriging needs more sites than mean / drift functions (nothing is left to predict from once a site is deleted)", GSL_EDOM);
  if (st->loo_state != 1)
    GSL_ERROR("gsl_sinterp_loo: initialised without gsl_sinterp_set_loo", GSL_EINVAL);
  return GSL_SUCCESS;
}

int gsl_sinterp_loo_residuals(const gsl_sinterp *interp, gsl_matrix *E)
{
  if (!interp || !E) GSL_ERROR("gsl_sinterp_loo_residuals: null argument", GSL_EFAULT);
  int ls = loo_status(interp);
  if (ls) return ls;
  const rbf_state *st = rbf_of(interp);
  if (E->size1 != st->n || E->size2 != st->loo_nf) GSL_ERROR("gsl_sinterp_loo_residuals: E must be size x fields", GSL_EBADLEN);
  for (size_t i = 0; i < st->n; i++)
    for (size_t q = 0; q < st->loo_nf; q++) E->data[i * E->tda + q] = st->loo_e[q * st->n + i];
  return GSL_SUCCESS;
}

int gsl_sinterp_loo_variance(const gsl_sinterp *interp, gsl_vector *v)
{
  if (!interp || !v) GSL_ERROR("gsl_sinterp_loo_variance: null argument", GSL_EFAULT);
  int ls = loo_status(interp);
  if (ls) return ls;
  const rbf_state *st = rbf_of(interp);
  if (v->size != st->n) GSL_ERROR("gsl_sinterp_loo_variance: wrong length", GSL_EBADLEN);
  for (size_t i = 0; i < st->n; i++) gsl_vector_set(v, i, st->loo_v[i]);
  return GSL_SUCCESS;
}

/* ------------------------------------------------------------------------ */
/* Model selection ("Model selection"): a workspace that keeps the centres, the response and the N x N matrix
   on the device, so that scoring a candidate (eps, nugget) is fill + factorisation + reduction + 32 bytes back. */
struct gsl_sinterp_fit_workspace {
  int kind, krige;
  size_t n, dim;
  gsl_sinterp_hip_ctx *ctx;
  double *d_x, *d_f, *d_w, *d_out, *d_phi;       /* d_x: one buffer [x | f | w | out]; d_phi: the matrix */
  double *d_g, *d_work, *d_b, *d_dinv;           /* leave-one-out: allocated by the first FIT_LOO evaluation */
  size_t chunk;
  size_t n_grid, max_eval;                       /* the search */
  double tol;
  size_t n_eval;                                 /* the last search: its evaluations in order */
  double *tr_param, *tr_score;                   /* max_eval entries each */
  int have_sigma2;
  double sigma2;
};

gsl_sinterp_fit_workspace *gsl_sinterp_fit_alloc(const gsl_sinterp *interp, const gsl_matrix *x, const gsl_vector *f)
{
  if (!interp || !x || !f) GSL_ERROR_NULL("gsl_sinterp_fit_alloc: null argument", GSL_EFAULT);
  const type_desc *d = desc_of(interp->type);
  if (d->noun) {
    noun_error(d, "gsl_sinterp_fit_alloc: not for %s interpolants (nothing to fit)", GSL_EUNSUP);
    return NULL;
  }
  if (!d->pd)
    GSL_ERROR_NULL("gsl_sinterp_fit_alloc: positive definite RBF (Gaussian, Wendland, Matern, inverse multiquadric) and kriging interpolants only", GSL_EINVAL);
  const size_t n = interp->size, dim = interp->dim;
  if (x->size1 != n || x->size2 != dim) GSL_ERROR_NULL("gsl_sinterp_fit_alloc: x must be size x dim", GSL_EBADLEN);
  if (f->size != n) GSL_ERROR_NULL("gsl_sinterp_fit_alloc: f must have size entries", GSL_EBADLEN);
  gsl_sinterp_fit_workspace *w = (gsl_sinterp_fit_workspace *)calloc(1, sizeof *w);
  if (!w) GSL_ERROR_NULL("gsl_sinterp_fit_alloc: out of memory", GSL_ENOMEM);
  const rbf_state *st = rbf_of(interp);
  w->kind = st->kind; w->krige = st->krige; w->n = n; w->dim = dim;
  w->chunk = (n + 127) / 128 * 128;
  if (w->chunk > LOO_CHUNK) w->chunk = LOO_CHUNK;
  w->n_grid = 9; w->tol = 1e-2; w->max_eval = 40;
  w->tr_param = (double *)malloc(w->max_eval * sizeof(double));
  w->tr_score = (double *)malloc(w->max_eval * sizeof(double));
  double *h = (double *)malloc(n * (dim + 1) * sizeof(double));                  /* [x | f] packed */
  if (!w->tr_param || !w->tr_score || !h) {
    free(h); gsl_sinterp_fit_free(w);
    GSL_ERROR_NULL("gsl_sinterp_fit_alloc: out of memory", GSL_ENOMEM);
  }
  for (size_t i = 0; i < n; i++) {
    for (size_t a = 0; a < dim; a++) h[i * dim + a] = x->data[i * x->tda + a];
    h[n * dim + i] = f->data[i * f->stride];
  }
  if (gsl_sinterp_hip_ctx_create(&w->ctx, interp->devices[0], NULL) != GSL_SUCCESS) {
    w->ctx = NULL; free(h); gsl_sinterp_fit_free(w);
    GSL_ERROR_NULL("gsl_sinterp_fit_alloc: no usable HIP device (GPU path has no CPU fallback)", GSL_EFAILED);
  }
  int s = gsl_sinterp_hip_malloc(w->ctx, (void **)&w->d_x, (n * (dim + 2) + 4) * sizeof(double));
  if (!s) s = gsl_sinterp_hip_malloc(w->ctx, (void **)&w->d_phi, n * n * sizeof(double));
  if (!s) s = gsl_sinterp_hip_h2d(w->ctx, w->d_x, h, n * (dim + 1) * sizeof(double));
  free(h);
  if (s) {
    gsl_error(gsl_sinterp_hip_last_error(w->ctx), __FILE__, __LINE__, s);
    gsl_sinterp_fit_free(w);
    return NULL;
  }
  w->d_f = w->d_x + n * dim; w->d_w = w->d_f + n; w->d_out = w->d_w + n;
  return w;
}

void gsl_sinterp_fit_free(gsl_sinterp_fit_workspace *w)
{
  if (!w) return;
  if (w->ctx) {
    gsl_sinterp_hip_free(w->ctx, w->d_x); gsl_sinterp_hip_free(w->ctx, w->d_phi);
    gsl_sinterp_hip_free(w->ctx, w->d_g); gsl_sinterp_hip_free(w->ctx, w->d_work);
    gsl_sinterp_hip_free(w->ctx, w->d_b); gsl_sinterp_hip_free(w->ctx, w->d_dinv);
    gsl_sinterp_hip_ctx_destroy(w->ctx);
  }
  free(w->tr_param); free(w->tr_score);
  free(w);
}

/* what is wrong with (criterion, eps, nugget) for this workspace, or NULL */
static const char *fit_bad_args(const gsl_sinterp_fit_workspace *w, int criterion, double eps, double nugget)
{
  if (criterion != GSL_SINTERP_FIT_LOO && criterion != GSL_SINTERP_FIT_ML) return "unknown criterion";
  if (!(eps > 0.0) || !isfinite(eps)) return "eps must be finite and > 0";
  if (!(nugget >= 0.0) || !isfinite(nugget)) return "the nugget must be finite and >= 0";
  if (!w->krige && nugget != 0.0) return "the nugget must be 0 for a type that is not kriging";
  return NULL;
}

/* One evaluation, arguments already checked.  Returns a status WITHOUT calling the error handler (the text of a failure is
   the context's); a candidate that does not factor gives GSL_SUCCESS and *score = +infinity. */
static int fit_evaluate(gsl_sinterp_fit_workspace *w, int criterion, double eps, double nugget, double *score)
{
  gsl_sinterp_hip_ctx *c = w->ctx;
  const size_t n = w->n, dim = w->dim;
  const int loo = criterion == GSL_SINTERP_FIT_LOO;
  *score = GSL_NAN;
  int s = GSL_SUCCESS, route = 0;
  if (loo && !w->d_g) {
    s = gsl_sinterp_hip_malloc(c, (void **)&w->d_g, n * sizeof(double));
    if (!s) s = gsl_sinterp_hip_malloc(c, (void **)&w->d_work, gsl_sinterp_hip_chol_inv_diag_work(n, w->chunk) * sizeof(double));
    if (!s && w->krige) s = gsl_sinterp_hip_malloc(c, (void **)&w->d_b, n * sizeof(double));
    if (!s && w->krige) s = gsl_sinterp_hip_malloc(c, (void **)&w->d_dinv, ((n + 31) / 32) * 1024 * sizeof(double));
    if (s) {
      gsl_sinterp_hip_free(c, w->d_g); gsl_sinterp_hip_free(c, w->d_work); gsl_sinterp_hip_free(c, w->d_b); gsl_sinterp_hip_free(c, w->d_dinv);
      w->d_g = w->d_work = w->d_b = w->d_dinv = NULL;
      return s;
    }
  }
  double mean = 0.0, denom = 0.0, out[4] = {0.0, 0.0, 0.0, 0.0};
  s = gsl_sinterp_hip_d2d_async(c, w->d_w, w->d_f, n * sizeof(double));
  if (!s) s = w->krige ? gsl_sinterp_hip_krige_solve_fields(c, w->kind, eps, nugget, w->d_x, n, (int)dim, dim, w->d_phi, n, w->d_w, n, 1, &mean, &route)
                       : gsl_sinterp_hip_rbf_solve_fields(c, w->kind, eps, w->d_x, n, (int)dim, dim, w->d_phi, n, w->d_w, n, 1, &route);
  if (!s && loo) s = gsl_sinterp_hip_chol_inv_diag(c, n, w->d_phi, n, w->d_g, w->d_work, w->chunk);
  if (!s && loo && w->krige) s = gsl_sinterp_hip_krige_variance_prepare(c, n, w->d_phi, n, w->d_b, w->d_dinv, &denom);
  if (s == GSL_EDOM) { *score = INFINITY; return GSL_SUCCESS; }                   /* not positive definite: an expected candidate */
  if (!s) s = gsl_sinterp_hip_score_reduce(c, n, w->d_phi, n, w->d_f, w->d_w, loo ? w->d_g : NULL, loo && w->krige ? w->d_b : NULL, denom, w->d_out);
  if (!s) s = gsl_sinterp_hip_d2h(c, out, w->d_out, sizeof out);
  if (s) return s;
  const double N = (double)n, s2 = out[1] / N;
  double v = loo ? out[2] / N : 0.5 * (N * log(6.283185307179586 * s2) + out[0] + N);
  if (out[3] != 0.0 || !(out[1] > 0.0) || !isfinite(v)) { *score = INFINITY; return GSL_SUCCESS; }
  *score = v;
  w->sigma2 = s2; w->have_sigma2 = 1;
  return GSL_SUCCESS;
}

int gsl_sinterp_fit_score(gsl_sinterp_fit_workspace *w, int criterion, double eps, double nugget, double *score)
{
  if (score) *score = GSL_NAN;
  if (!w || !score) GSL_ERROR("gsl_sinterp_fit_score: null argument", GSL_EFAULT);
  const char *bad = fit_bad_args(w, criterion, eps, nugget);
  if (bad) GSL_ERROR(bad, GSL_EINVAL);
  HIP_TRY(fit_evaluate(w, criterion, eps, nugget, score), w->ctx);
  return GSL_SUCCESS;
}

/* the search of fit_shape (over_nugget = 0: `fixed` is the nugget) and fit_nugget (over_nugget = 1: `fixed` is eps) */
static int fit_search(gsl_sinterp_fit_workspace *w, int criterion, int over_nugget, double fixed, double lo, double hi, double *best,
                      double *score_best)
{
  if (best) *best = GSL_NAN;
  if (score_best) *score_best = GSL_NAN;
  if (!w || !best || !score_best) GSL_ERROR("gsl_sinterp_fit: null argument", GSL_EFAULT);
  if (over_nugget && !w->krige) GSL_ERROR("gsl_sinterp_fit_nugget: kriging interpolants only", GSL_EINVAL);
  if (!(lo > 0.0) || !(hi > lo) || !isfinite(hi)) GSL_ERROR("gsl_sinterp_fit: the bracket needs 0 < lo < hi < infinity", GSL_EINVAL);
  const char *bad = over_nugget ? fit_bad_args(w, criterion, fixed, lo) : fit_bad_args(w, criterion, lo, fixed);
  if (bad) GSL_ERROR(bad, GSL_EINVAL);
  w->n_eval = 0;
  const double tlo = log(lo), thi = log(hi);
  double p_best = GSL_NAN, s_best = INFINITY, s2_best = GSL_NAN;
  int status = GSL_SUCCESS;
  /* one evaluation at t (p != 0: at exactly p): recorded in the trace, the running best kept; +infinity once the budget is spent */
#define FIT_EVAL(t, p, dst)                                                                       \
  do {                                                                                            \
    (dst) = INFINITY;                                                                             \
    if (!status && w->n_eval < w->max_eval) {                                                     \
      const double _p = (p) != 0.0 ? (p) : exp(t);                                                \
      double _v = GSL_NAN;                                                                        \
      status = over_nugget ? fit_evaluate(w, criterion, fixed, _p, &_v) : fit_evaluate(w, criterion, _p, fixed, &_v); \
      if (!status) {                                                                              \
        w->tr_param[w->n_eval] = _p; w->tr_score[w->n_eval] = _v; w->n_eval++;                    \
        if (_v < s_best) { s_best = _v; p_best = _p; s2_best = w->sigma2; }                                       \
        (dst) = _v;                                                                               \
      }                                                                                           \
    }                                                                                             \
  } while (0)
  /* the grid: the first index of the smallest score */
  size_t k = 0;
  double g_best = INFINITY;
  for (size_t j = 0; j < w->n_grid && !status; j++) {
    const double t = tlo + (thi - tlo) * ((double)j / (double)(w->n_grid - 1));
    double v;
    FIT_EVAL(t, j == 0 ? lo : j == w->n_grid - 1 ? hi : 0.0, v);
    if (v < g_best) { g_best = v; k = j; }
  }
  if (!status && isfinite(g_best)) {
    /* golden section on the two cells around grid point k (one cell at an end) */
    const size_t ka = k > 0 ? k - 1 : 0, kb = k + 1 < w->n_grid ? k + 1 : k;
    double a = tlo + (thi - tlo) * ((double)ka / (double)(w->n_grid - 1)), b = tlo + (thi - tlo) * ((double)kb / (double)(w->n_grid - 1));
    const double r = 0.6180339887498949;               /* (sqrt 5 - 1) / 2 */
    double cpt = b - r * (b - a), dpt = a + r * (b - a), fc, fd;
    FIT_EVAL(cpt, 0.0, fc);
    FIT_EVAL(dpt, 0.0, fd);
    while (!status && b - a > w->tol && w->n_eval < w->max_eval) {
      if (fc <= fd) {
        b = dpt; dpt = cpt; fd = fc; cpt = b - r * (b - a);
        if (b - a > w->tol) FIT_EVAL(cpt, 0.0, fc);
      } else {
        a = cpt; cpt = dpt; fc = fd; dpt = a + r * (b - a);
        if (b - a > w->tol) FIT_EVAL(dpt, 0.0, fd);
      }
    }
  }
#undef FIT_EVAL
  HIP_TRY(status, w->ctx);
  if (!isfinite(s_best)) GSL_ERROR("gsl_sinterp_fit: no candidate in the bracket has a positive definite matrix", GSL_EDOM);
  *best = p_best; *score_best = s_best;
  w->sigma2 = s2_best;                                 /* of the score handed back, not of the last candidate tried */
  return GSL_SUCCESS;
}

int gsl_sinterp_fit_shape(gsl_sinterp_fit_workspace *w, int criterion, double nugget, double eps_lo, double eps_hi, double *eps_best,
                          double *score_best)
{
  return fit_search(w, criterion, 0, nugget, eps_lo, eps_hi, eps_best, score_best);
}

int gsl_sinterp_fit_nugget(gsl_sinterp_fit_workspace *w, int criterion, double eps, double nugget_lo, double nugget_hi,
                           double *nugget_best, double *score_best)
{
  return fit_search(w, criterion, 1, eps, nugget_lo, nugget_hi, nugget_best, score_best);
}

int gsl_sinterp_fit_set_search(gsl_sinterp_fit_workspace *w, size_t n_grid, double tol, size_t max_eval)
{
  /* the numbers first: they can be judged without a workspace */
  if (n_grid < 3 || !(tol > 0.0) || max_eval < n_grid) GSL_ERROR("gsl_sinterp_fit_set_search: needs n_grid >= 3, tol > 0, max_eval >= n_grid", GSL_EINVAL);
  if (!w) GSL_ERROR("gsl_sinterp_fit_set_search: null workspace", GSL_EFAULT);
  if (max_eval != w->max_eval) {
    double *p = (double *)malloc(max_eval * sizeof(double)), *q = (double *)malloc(max_eval * sizeof(double));
    if (!p || !q) { free(p); free(q); GSL_ERROR("gsl_sinterp_fit_set_search: out of memory", GSL_ENOMEM); }
    free(w->tr_param); free(w->tr_score);
    w->tr_param = p; w->tr_score = q; w->n_eval = 0;     /* the trace of the last search goes with its arrays */
  }
  w->n_grid = n_grid; w->tol = tol; w->max_eval = max_eval;
  return GSL_SUCCESS;
}

size_t gsl_sinterp_fit_n_eval(const gsl_sinterp_fit_workspace *w) { return w ? w->n_eval : 0; }

int gsl_sinterp_fit_trace(const gsl_sinterp_fit_workspace *w, gsl_vector *param, gsl_vector *score)
{
  if (!w || !param || !score) GSL_ERROR("gsl_sinterp_fit_trace: null argument", GSL_EFAULT);
  if (param->size != w->n_eval || score->size != w->n_eval) GSL_ERROR("gsl_sinterp_fit_trace: the vectors need gsl_sinterp_fit_n_eval entries", GSL_EBADLEN);
  for (size_t i = 0; i < w->n_eval; i++) {
    param->data[i * param->stride] = w->tr_param[i];
    score->data[i * score->stride] = w->tr_score[i];
  }
  return GSL_SUCCESS;
}

int gsl_sinterp_fit_sigma2(const gsl_sinterp_fit_workspace *w, double *s2)
{
  if (s2) *s2 = GSL_NAN;
  if (!w || !s2) GSL_ERROR("gsl_sinterp_fit_sigma2: null argument", GSL_EFAULT);
  if (!w->have_sigma2) GSL_ERROR("gsl_sinterp_fit_sigma2: no evaluation has returned a finite score yet", GSL_EINVAL);
  *s2 = w->sigma2;
  return GSL_SUCCESS;
}

/* ------------------------------------------------------------------------ */
/* Empirical variogram and the covariance model fitted to it (DESIGN_VARIOGRAM.md): the binned pair sums come from
   gsl_sinterp_hip_variogram as exact integers; everything below them is host arithmetic on n_bins numbers. */

/* 1 - phi_kind(eps h), phi as include/gsl_sinterp_hip.h defines the three covariances */
static double vario_rise(int kind, double eps, double h)
{
  if (kind == GSL_SINTERP_RBF_GAUSSIAN) { const double t = eps * h; return 1.0 - exp(-(t * t)); }
  if (kind == GSL_SINTERP_RBF_MATERN32) { const double t = sqrt(3.0) * eps * h; return 1.0 - (1.0 + t) * exp(-t); }
  const double t = sqrt(5.0) * eps * h;
  return 1.0 - (1.0 + t + t * t / 3.0) * exp(-t);
}

typedef struct {
  int kind;
  size_t m;                                            /* usable bins */
  const double *h, *y, *w;                             /* their lags, semivariances and weights */
} vario_problem;

static double vario_wss(const vario_problem *p, double eps, double c0, double c)
{
  double s = 0.0;
  for (size_t b = 0; b < p->m; b++) {
    const double r = p->y[b] - c0 - c * vario_rise(p->kind, eps, p->h[b]);
    s += p->w[b] * r * r;
  }
  return s;
}

/* gamma = c0 + c g(eps) by weighted least squares with c0 >= 0 and c >= 0: both free first; when a coefficient comes out
   negative (or the two columns are dependent) the better of the two one-column fits, the nugget-only one on a tie */
static double vario_wls(const vario_problem *p, double eps, double *c0_out, double *c_out)
{
  double sw = 0.0, sg = 0.0, sgg = 0.0, sy = 0.0, sgy = 0.0;
  for (size_t b = 0; b < p->m; b++) {
    const double g = vario_rise(p->kind, eps, p->h[b]), w = p->w[b];
    sw += w; sg += w * g; sgg += w * g * g; sy += w * p->y[b]; sgy += w * g * p->y[b];
  }
  const double det = sw * sgg - sg * sg;
  if (det > 0.0) {
    const double c = (sw * sgy - sg * sy) / det, c0 = (sy - c * sg) / sw;
    if (c0 >= 0.0 && c >= 0.0) { *c0_out = c0; *c_out = c; return vario_wss(p, eps, c0, c); }
  }
  double a0 = sy / sw, a1 = sgg > 0.0 ? sgy / sgg : 0.0;
  if (!(a0 > 0.0)) a0 = 0.0;
  if (!(a1 > 0.0)) a1 = 0.0;
  const double w0 = vario_wss(p, eps, a0, 0.0), w1 = vario_wss(p, eps, 0.0, a1);
  if (w1 < w0) { *c0_out = 0.0; *c_out = a1; return w1; }
  *c0_out = a0; *c_out = 0.0;
  return w0;
}

/* the evaluations of the last gsl_sinterp_variogram_fit_model in order (the facade is single-threaded) */
static struct { size_t n, cap; double *eps, *wss; } vario_trace;

/* The fixed search rule of fit_search over t = log eps, on the weighted sum of squares of vario_wls: n_grid points from lo to
   hi with the ends included, golden section on the two cells around the first smallest grid value, until the bracket is no
   wider than tol or max_eval evaluations are spent; the best point ever evaluated wins. */
static int vario_search(const vario_problem *p, double lo, double hi, size_t n_grid, double tol, size_t max_eval, double *eps_best,
                        double *c0_best, double *c_best, double *wss_best)
{
  if (max_eval > vario_trace.cap) {
    double *a = (double *)malloc(max_eval * sizeof(double)), *b = (double *)malloc(max_eval * sizeof(double));
    if (!a || !b) { free(a); free(b); return GSL_ENOMEM; }
    free(vario_trace.eps); free(vario_trace.wss);
    vario_trace.eps = a; vario_trace.wss = b; vario_trace.cap = max_eval;
  }
  vario_trace.n = 0;
  const double tlo = log(lo), thi = log(hi);
  double s_best = INFINITY;
#define VARIO_EVAL(t, pp, dst)                                                                    \
  do {                                                                                            \
    (dst) = INFINITY;                                                                             \
    if (vario_trace.n < max_eval) {                                                               \
      const double _p = (pp) != 0.0 ? (pp) : exp(t);                                              \
      double _c0, _c;                                                                             \
      const double _v = vario_wls(p, _p, &_c0, &_c);                                              \
      vario_trace.eps[vario_trace.n] = _p; vario_trace.wss[vario_trace.n] = _v; vario_trace.n++;  \
      if (_v < s_best) { s_best = _v; *eps_best = _p; *c0_best = _c0; *c_best = _c; }             \
      (dst) = _v;                                                                                 \
    }                                                                                             \
  } while (0)
  size_t k = 0;
  double g_best = INFINITY;
  for (size_t j = 0; j < n_grid; j++) {
    const double t = tlo + (thi - tlo) * ((double)j / (double)(n_grid - 1));
    double v;
    VARIO_EVAL(t, j == 0 ? lo : j == n_grid - 1 ? hi : 0.0, v);
    if (v < g_best) { g_best = v; k = j; }
  }
  if (isfinite(g_best)) {
    const size_t ka = k > 0 ? k - 1 : 0, kb = k + 1 < n_grid ? k + 1 : k;
    double a = tlo + (thi - tlo) * ((double)ka / (double)(n_grid - 1)), b = tlo + (thi - tlo) * ((double)kb / (double)(n_grid - 1));
    const double r = 0.6180339887498949;               /* (sqrt 5 - 1) / 2 */
    double cpt = b - r * (b - a), dpt = a + r * (b - a), fc, fd;
    VARIO_EVAL(cpt, 0.0, fc);
    VARIO_EVAL(dpt, 0.0, fd);
    while (b - a > tol && vario_trace.n < max_eval) {
      if (fc <= fd) {
        b = dpt; dpt = cpt; fd = fc; cpt = b - r * (b - a);
        if (b - a > tol) VARIO_EVAL(cpt, 0.0, fc);
      } else {
        a = cpt; cpt = dpt; fc = fd; dpt = a + r * (b - a);
        if (b - a > tol) VARIO_EVAL(dpt, 0.0, fd);
      }
    }
  }
#undef VARIO_EVAL
  *wss_best = s_best;
  return isfinite(s_best) ? GSL_SUCCESS : GSL_EDOM;
}

int gsl_sinterp_variogram_fit_model(int kind, int weights, const double *lag, const double *gamma, const double *count, size_t n_bins,
                                    double eps_lo, double eps_hi, size_t n_grid, double tol, size_t max_eval, double *eps, double *nugget_abs,
                                    double *psill, double *wss)
{
  if (eps) *eps = GSL_NAN;
  if (nugget_abs) *nugget_abs = GSL_NAN;
  if (psill) *psill = GSL_NAN;
  if (wss) *wss = GSL_NAN;
  vario_trace.n = 0;
  /* the numbers first */
  if (kind != GSL_SINTERP_RBF_GAUSSIAN && kind != GSL_SINTERP_RBF_MATERN32 && kind != GSL_SINTERP_RBF_MATERN52)
    GSL_ERROR("gsl_sinterp_variogram_fit_model: the kind must be a kriging covariance (Gaussian, Matern 3/2, Matern 5/2)", GSL_EINVAL);
  if (weights != GSL_SINTERP_VARIOGRAM_W_COUNT && weights != GSL_SINTERP_VARIOGRAM_W_COUNT_H2 && weights != GSL_SINTERP_VARIOGRAM_W_NONE)
    GSL_ERROR("gsl_sinterp_variogram_fit_model: unknown weights", GSL_EINVAL);
  if (n_grid == 0) n_grid = 9;
  if (tol == 0.0) tol = 1e-2;
  if (max_eval == 0) max_eval = 40;
  if (n_grid < 3 || !(tol > 0.0) || max_eval < n_grid)
    GSL_ERROR("gsl_sinterp_variogram_fit_model: needs n_grid >= 3, tol > 0, max_eval >= n_grid (0 = the defaults 9, 1e-2, 40)", GSL_EINVAL);
  if (!(eps_lo > 0.0) || !(eps_hi > eps_lo) || !isfinite(eps_hi))
    GSL_ERROR("gsl_sinterp_variogram_fit_model: the bracket needs 0 < eps_lo < eps_hi < infinity", GSL_EINVAL);
  if (!lag || !gamma || !count || !eps || !nugget_abs || !psill) GSL_ERROR("gsl_sinterp_variogram_fit_model: null argument", GSL_EFAULT);
  double *buf = (double *)malloc((n_bins ? n_bins : 1) * 3 * sizeof(double));
  if (!buf) GSL_ERROR("gsl_sinterp_variogram_fit_model: out of memory", GSL_ENOMEM);
  double *h = buf, *y = buf + n_bins, *w = buf + 2 * n_bins;
  size_t m = 0;
  for (size_t b = 0; b < n_bins; b++) {
    if (!(count[b] > 0.0) || !isfinite(count[b]) || !isfinite(gamma[b]) || !isfinite(lag[b]) || lag[b] < 0.0) continue;
    if (weights == GSL_SINTERP_VARIOGRAM_W_COUNT_H2 && !(lag[b] > 0.0)) continue;    /* a bin of coincident sites has no finite N / h^2 */
    h[m] = lag[b]; y[m] = gamma[b];
    w[m] = weights == GSL_SINTERP_VARIOGRAM_W_COUNT ? count[b] : weights == GSL_SINTERP_VARIOGRAM_W_COUNT_H2 ? count[b] / (lag[b] * lag[b]) : 1.0;
    m++;
  }
  if (m < 3) {
    free(buf);
    GSL_ERROR("gsl_sinterp_variogram_fit_model: fewer than 3 usable bins", GSL_EDOM);
  }
  const vario_problem p = {kind, m, h, y, w};
  double e = GSL_NAN, c0 = GSL_NAN, c = GSL_NAN, s = GSL_NAN;
  const int st = vario_search(&p, eps_lo, eps_hi, n_grid, tol, max_eval, &e, &c0, &c, &s);
  free(buf);
  if (st == GSL_ENOMEM) GSL_ERROR("gsl_sinterp_variogram_fit_model: out of memory", GSL_ENOMEM);
  if (st) GSL_ERROR("gsl_sinterp_variogram_fit_model: no candidate in the bracket has a finite sum of squares", GSL_EDOM);
  *eps = e; *nugget_abs = c0; *psill = c;
  if (wss) *wss = s;
  return GSL_SUCCESS;
}

size_t gsl_sinterp_variogram_fit_model_n_eval(void) { return vario_trace.n; }

int gsl_sinterp_variogram_fit_model_trace(gsl_vector *eps, gsl_vector *wss)
{
  if (!eps || !wss) GSL_ERROR("gsl_sinterp_variogram_fit_model_trace: null argument", GSL_EFAULT);
  if (eps->size != vario_trace.n || wss->size != vario_trace.n)
    GSL_ERROR("gsl_sinterp_variogram_fit_model_trace: the vectors need gsl_sinterp_variogram_fit_model_n_eval entries", GSL_EBADLEN);
  for (size_t i = 0; i < vario_trace.n; i++) {
    eps->data[i * eps->stride] = vario_trace.eps[i];
    wss->data[i * wss->stride] = vario_trace.wss[i];
  }
  return GSL_SUCCESS;
}

struct gsl_sinterp_variogram {
  size_t dim, n_bins;
  int device;
  gsl_sinterp_hip_ctx *ctx;                            /* created by the first compute */
  double *d_stage; size_t stage_cap;                   /* grow-only [x | f] of gsl_sinterp_variogram_compute */
  int have;                                            /* a variogram is held */
  double h_max;
  int shift[3];
  unsigned long long *acc;                             /* n_bins x 7 */
  const gsl_sinterp_type *fit_type;                    /* the last successful fit, NULL before one */
  double fit_eps, fit_nugget;
};

gsl_sinterp_variogram *gsl_sinterp_variogram_alloc(size_t dim, size_t n_bins)
{
  if (dim < 1 || dim > 3) GSL_ERROR_NULL("gsl_sinterp_variogram_alloc: dim must be 1, 2 or 3", GSL_EINVAL);
  if (n_bins < 1 || n_bins > 256) GSL_ERROR_NULL("gsl_sinterp_variogram_alloc: 1 .. 256 bins", GSL_EINVAL);
  gsl_sinterp_variogram *v = (gsl_sinterp_variogram *)calloc(1, sizeof *v);
  unsigned long long *acc = (unsigned long long *)calloc(n_bins * 7, sizeof *acc);
  if (!v || !acc) {
    free(v); free(acc);
    GSL_ERROR_NULL("gsl_sinterp_variogram_alloc: out of memory", GSL_ENOMEM);
  }
  v->dim = dim; v->n_bins = n_bins; v->device = default_device(); v->acc = acc; v->h_max = GSL_NAN;
  return v;
}

void gsl_sinterp_variogram_free(gsl_sinterp_variogram *v)
{
  if (!v) return;
  if (v->ctx) {
    gsl_sinterp_hip_free(v->ctx, v->d_stage);
    gsl_sinterp_hip_ctx_destroy(v->ctx);
  }
  free(v->acc);
  free(v);
}

int gsl_sinterp_variogram_set_device(gsl_sinterp_variogram *v, int device)
{
  if (!v) GSL_ERROR("gsl_sinterp_variogram_set_device: null workspace", GSL_EFAULT);
  if (device < 0) GSL_ERROR("gsl_sinterp_variogram_set_device: negative ordinal", GSL_EINVAL);
  if (v->ctx && device != v->device) {                 /* the context and its staging buffer belong to the old device */
    gsl_sinterp_hip_free(v->ctx, v->d_stage);
    gsl_sinterp_hip_ctx_destroy(v->ctx);
    v->ctx = NULL; v->d_stage = NULL; v->stage_cap = 0;
  }
  v->device = device;
  return GSL_SUCCESS;
}

double gsl_sinterp_variogram_h_max(const gsl_sinterp_variogram *v) { return v && v->have ? v->h_max : GSL_NAN; }

/* what every compute does first: the workspace loses its variogram and its fit */
static void vario_drop(gsl_sinterp_variogram *v)
{
  v->have = 0; v->h_max = GSL_NAN; v->fit_type = NULL;
  memset(v->acc, 0, v->n_bins * 7 * sizeof *v->acc);
}

static int vario_ctx(gsl_sinterp_variogram *v)
{
  if (v->ctx) return GSL_SUCCESS;
  if (gsl_sinterp_hip_ctx_create(&v->ctx, v->device, NULL) != GSL_SUCCESS) {
    v->ctx = NULL;
    GSL_ERROR("gsl_sinterp_variogram_compute: no usable HIP device (GPU path has no CPU fallback)", GSL_EFAILED);
  }
  return GSL_SUCCESS;
}

int gsl_sinterp_variogram_compute_resident(gsl_sinterp_variogram *v, const double *d_x, size_t n, size_t xtda, const double *d_f, double h_max)
{
  if (!v) GSL_ERROR("gsl_sinterp_variogram_compute_resident: null workspace", GSL_EFAULT);
  vario_drop(v);
  if (n > 0 && (!d_x || !d_f)) GSL_ERROR("gsl_sinterp_variogram_compute_resident: null argument", GSL_EFAULT);
  if (xtda < v->dim) GSL_ERROR("gsl_sinterp_variogram_compute_resident: rows shorter than the dimension", GSL_EBADLEN);
  if (!isfinite(h_max)) GSL_ERROR("gsl_sinterp_variogram_compute_resident: h_max must be finite (<= 0 selects a third of the box diagonal)", GSL_EINVAL);
  if (n > 0x7fffffffULL) GSL_ERROR("gsl_sinterp_variogram_compute_resident: at most 2^31 - 1 sites", GSL_EINVAL);
  const int st0 = vario_ctx(v);
  if (st0) return st0;
  if (!(h_max > 0.0)) {                                /* gstat's default: a third of the diagonal of the bounding box */
    double box[6], d2 = 0.0;
    if (n < 2) GSL_ERROR("gsl_sinterp_variogram_compute: the default h_max needs at least two sites", GSL_EDOM);
    HIP_TRY(gsl_sinterp_hip_bbox(v->ctx, d_x, n, (int)v->dim, xtda, box), v->ctx);
    for (size_t c = 0; c < v->dim; c++) { const double e = box[2 * c + 1] - box[2 * c]; d2 += e * e; }
    h_max = sqrt(d2) / 3.0;
    if (!(h_max > 0.0) || !isfinite(h_max))
      GSL_ERROR("gsl_sinterp_variogram_compute: the default h_max needs finite sites that do not all coincide", GSL_EDOM);
  }
  const int st = gsl_sinterp_hip_variogram(v->ctx, d_x, n, (int)v->dim, xtda, d_f, h_max, (int)v->n_bins, v->acc, v->shift);
  if (st) {
    memset(v->acc, 0, v->n_bins * 7 * sizeof *v->acc);
    HIP_TRY(st, v->ctx);
  }
  v->have = 1; v->h_max = h_max;
  return GSL_SUCCESS;
}

int gsl_sinterp_variogram_compute(gsl_sinterp_variogram *v, const gsl_matrix *x, const gsl_vector *f, double h_max)
{
  if (!v) GSL_ERROR("gsl_sinterp_variogram_compute: null workspace", GSL_EFAULT);
  vario_drop(v);
  if (!x || !f) GSL_ERROR("gsl_sinterp_variogram_compute: null argument", GSL_EFAULT);
  if (x->size2 != v->dim) GSL_ERROR("gsl_sinterp_variogram_compute: x must be n x dim", GSL_EBADLEN);
  if (f->size != x->size1) GSL_ERROR("gsl_sinterp_variogram_compute: f must have one entry per row of x", GSL_EBADLEN);
  if (!isfinite(h_max)) GSL_ERROR("gsl_sinterp_variogram_compute: h_max must be finite (<= 0 selects a third of the box diagonal)", GSL_EINVAL);
  if (x->size1 > 0x7fffffffULL) GSL_ERROR("gsl_sinterp_variogram_compute: at most 2^31 - 1 sites", GSL_EINVAL);
  const size_t n = x->size1, dim = v->dim;
  const int st0 = vario_ctx(v);
  if (st0) return st0;
  if (n == 0) return gsl_sinterp_variogram_compute_resident(v, NULL, 0, dim, NULL, h_max);
  double *h = (double *)malloc(n * (dim + 1) * sizeof(double));                  /* [x | f] packed */
  if (!h) GSL_ERROR("gsl_sinterp_variogram_compute: out of memory", GSL_ENOMEM);
  for (size_t i = 0; i < n; i++) {
    for (size_t a = 0; a < dim; a++) h[i * dim + a] = x->data[i * x->tda + a];
    h[n * dim + i] = f->data[i * f->stride];
  }
  int s = GSL_SUCCESS;
  if (n * (dim + 1) > v->stage_cap) {
    gsl_sinterp_hip_free(v->ctx, v->d_stage);
    v->d_stage = NULL; v->stage_cap = 0;
    s = gsl_sinterp_hip_malloc(v->ctx, (void **)&v->d_stage, n * (dim + 1) * sizeof(double));
    if (!s) v->stage_cap = n * (dim + 1);
  }
  if (!s) s = gsl_sinterp_hip_h2d(v->ctx, v->d_stage, h, n * (dim + 1) * sizeof(double));
  free(h);
  HIP_TRY(s, v->ctx);
  return gsl_sinterp_variogram_compute_resident(v, v->d_stage, n, dim, v->d_stage + n * dim, h_max);
}

/* (hi 2^64 + lo) 2^-shift as a double: the integer is converted with one rounding, the scaling is exact */
static double vario_sum(unsigned long long lo, unsigned long long hi, int shift)
{
  const unsigned __int128 s = ((unsigned __int128)hi << 64) | (unsigned __int128)lo;
  return ldexp((double)s, -shift);
}

/* lag, semivariance and count of bin b (NaN, NaN, 0 for an empty bin) */
static void vario_bin(const gsl_sinterp_variogram *v, int estimator, size_t b, double *lag, double *gamma, double *count)
{
  const unsigned long long *a = v->acc + 7 * b;
  const double nb = (double)a[0];
  *count = nb; *lag = GSL_NAN; *gamma = GSL_NAN;
  if (a[0] == 0) return;
  *lag = vario_sum(a[3], a[4], v->shift[1]) / nb;
  if (estimator == GSL_SINTERP_VARIOGRAM_MATHERON) *gamma = vario_sum(a[1], a[2], v->shift[0]) / (2.0 * nb);
  else {
    const double m = vario_sum(a[5], a[6], v->shift[2]) / nb, m2 = m * m;
    *gamma = 0.5 * (m2 * m2) / (0.457 + 0.494 / nb);
  }
}

int gsl_sinterp_variogram_get(const gsl_sinterp_variogram *v, int estimator, gsl_vector *lag, gsl_vector *gamma, gsl_vector *count)
{
  if (!v) GSL_ERROR("gsl_sinterp_variogram_get: null workspace", GSL_EFAULT);
  if (estimator != GSL_SINTERP_VARIOGRAM_MATHERON && estimator != GSL_SINTERP_VARIOGRAM_CRESSIE)
    GSL_ERROR("gsl_sinterp_variogram_get: unknown estimator", GSL_EINVAL);
  if (!v->have) GSL_ERROR("gsl_sinterp_variogram_get: no variogram computed", GSL_EINVAL);
  if ((lag && lag->size != v->n_bins) || (gamma && gamma->size != v->n_bins) || (count && count->size != v->n_bins))
    GSL_ERROR("gsl_sinterp_variogram_get: the vectors need n_bins entries", GSL_EBADLEN);
  for (size_t b = 0; b < v->n_bins; b++) {
    double l, g, c;
    vario_bin(v, estimator, b, &l, &g, &c);
    if (lag) lag->data[b * lag->stride] = l;
    if (gamma) gamma->data[b * gamma->stride] = g;
    if (count) count->data[b * count->stride] = c;
  }
  return GSL_SUCCESS;
}

int gsl_sinterp_variogram_fit(gsl_sinterp_variogram *v, const gsl_sinterp_type *T, int estimator, int weights, double eps_lo, double eps_hi,
                              double *eps, double *nugget, double *sigma2, double *wss)
{
  if (eps) *eps = GSL_NAN;
  if (nugget) *nugget = GSL_NAN;
  if (sigma2) *sigma2 = GSL_NAN;
  if (wss) *wss = GSL_NAN;
  if (!v || !T || !eps || !nugget || !sigma2) GSL_ERROR("gsl_sinterp_variogram_fit: null argument", GSL_EFAULT);
  v->fit_type = NULL;
  const type_desc *d = desc_of(T);
  if (!d) GSL_ERROR("gsl_sinterp_variogram_fit: not one of the gsl_sinterp types", GSL_EINVAL);
  if (d->family != FAM_RBF) GSL_ERROR("gsl_sinterp_variogram_fit: mesh and Shepard types have no covariance model", GSL_EUNSUP);
  if (!d->krige) GSL_ERROR("gsl_sinterp_variogram_fit: kriging types only (an RBF type takes no nugget)", GSL_EINVAL);
  if (estimator != GSL_SINTERP_VARIOGRAM_MATHERON && estimator != GSL_SINTERP_VARIOGRAM_CRESSIE)
    GSL_ERROR("gsl_sinterp_variogram_fit: unknown estimator", GSL_EINVAL);
  if (weights != GSL_SINTERP_VARIOGRAM_W_COUNT && weights != GSL_SINTERP_VARIOGRAM_W_COUNT_H2 && weights != GSL_SINTERP_VARIOGRAM_W_NONE)
    GSL_ERROR("gsl_sinterp_variogram_fit: unknown weights", GSL_EINVAL);
  if (!v->have) GSL_ERROR("gsl_sinterp_variogram_fit: no variogram computed", GSL_EINVAL);
  if (!(eps_lo > 0.0)) { eps_lo = 0.1 / v->h_max; eps_hi = 100.0 / v->h_max; }
  double *buf = (double *)malloc(v->n_bins * 3 * sizeof(double));
  if (!buf) GSL_ERROR("gsl_sinterp_variogram_fit: out of memory", GSL_ENOMEM);
  double *lag = buf, *gam = buf + v->n_bins, *cnt = buf + 2 * v->n_bins;
  for (size_t b = 0; b < v->n_bins; b++) vario_bin(v, estimator, b, lag + b, gam + b, cnt + b);
  double e, c0, c, s;
  const int st = gsl_sinterp_variogram_fit_model(d->kind, weights, lag, gam, cnt, v->n_bins, eps_lo, eps_hi, 0, 0.0, 0, &e, &c0, &c, &s);
  free(buf);
  if (st) return st;                                   /* the handler has been called */
  if (!(c > 0.0)) GSL_ERROR("gsl_sinterp_variogram_fit: the fitted model is a pure nugget (c = 0): the relative nugget does not exist", GSL_EDOM);
  *eps = e; *nugget = c0 / c; *sigma2 = c;
  if (wss) *wss = s;
  v->fit_type = T; v->fit_eps = e; v->fit_nugget = c0 / c;
  return GSL_SUCCESS;
}

int gsl_sinterp_variogram_apply(const gsl_sinterp_variogram *v, gsl_sinterp *interp)
{
  if (!v || !interp) GSL_ERROR("gsl_sinterp_variogram_apply: null argument", GSL_EFAULT);
  if (!v->fit_type) GSL_ERROR("gsl_sinterp_variogram_apply: no successful fit yet", GSL_EINVAL);
  if (interp->type != v->fit_type) GSL_ERROR("gsl_sinterp_variogram_apply: the interpolant is of another type than the one fitted", GSL_EINVAL);
  const int st = gsl_sinterp_set_shape(interp, v->fit_eps);
  return st ? st : gsl_sinterp_set_nugget(interp, v->fit_nugget);
}

/* whether variances can be evaluated, as a status (the table of include/gsl_sinterp.h) */
static int variance_status(const gsl_sinterp *interp)
{
  const type_desc *d = desc_of(interp->type);
  if (d->noun) return noun_error(d, "gsl_sinterp_eval_variance: not for %s interpolants", GSL_EUNSUP);
  if (!d->krige) GSL_ERROR("gsl_sinterp_eval_variance: kriging interpolants only", GSL_EINVAL);
  const rbf_state *st = rbf_of(interp);
  if (!st->d_w || st->nf == 0) GSL_ERROR("gsl_sinterp_eval_variance: interpolant not initialised", GSL_EINVAL);
  if (st->local_k) return GSL_SUCCESS;                  /* the local route keeps no factor and needs none */
  if (st->var_state == 3)
    GSL_ERROR("gsl_sinterp_eval_variance: the interpolant was restored by gsl_sinterp_fread; a checkpoint carries no factor", GSL_EINVAL);
  if (st->var_state == 2)
    GSL_ERROR("gsl_sinterp_eval_variance: the init took the pivoted LDL^T route (8), which keeps no Cholesky factor", GSL_EUNSUP);
  if (st->var_state != 1)
    GSL_ERROR("gsl_sinterp_eval_variance: initialised without gsl_sinterp_set_variance", GSL_EINVAL);
  return GSL_SUCCESS;
}

/* the grow-only workspace of the variance, covariance and simulation entries: at least `need` doubles */
static int variance_workspace(rbf_state *st, size_t need)
{
  if (need <= st->vwork_doubles) return GSL_SUCCESS;
  gsl_sinterp_hip_free(st->ctx, st->d_vwork);
  st->d_vwork = NULL; st->vwork_doubles = 0;
  int s = gsl_sinterp_hip_malloc(st->ctx, (void **)&st->d_vwork, need * sizeof(double));
  if (!s) st->vwork_doubles = need;
  return s;
}

int gsl_sinterp_eval_variance_resident(const gsl_sinterp *interp, const double *d_y, size_t m, size_t ytda, double *d_var)
{
  if (!interp) GSL_ERROR("gsl_sinterp_eval_variance: null interpolant", GSL_EFAULT);
  int vs = variance_status(interp);
  if (vs) return vs;
  rbf_state *st = rbf_of(interp);           /* the workspace is a grow-only cache inside the state */
  if (m == 0) return GSL_SUCCESS;
  if (!d_y || !d_var) GSL_ERROR("gsl_sinterp_eval_variance: null argument", GSL_EFAULT);
  if (st->local_k) return local_eval_resident(interp, d_y, m, ytda, NULL, d_var, NULL);
  size_t chunk = (m + 63) / 64 * 64;
  if (chunk > 8192) chunk = 8192;
  const size_t need = st->drift ? gsl_sinterp_hip_ukrige_variance_work(st->n, chunk, st->drift_q) : gsl_sinterp_hip_krige_variance_work(st->n, chunk);
  HIP_TRY(variance_workspace(st, need), st->ctx);
  /* the factor lives on member 0, which evaluates every target (as gsl_sinterp_eval_resident does) */
  if (st->drift) {
    HIP_TRY(gsl_sinterp_hip_ukrige_variance(st->ctx, st->kind, st->eps, st->drift, st->drift_shift, st->drift_scale, st->d_x, st->n, (int)st->dim,
                                            st->dim, st->d_llt, st->llt_lda, st->d_B, st->n, st->d_dinv, st->drift_L, d_y, m, ytda, d_var,
                                            st->d_vwork, chunk), st->ctx);
  } else {
    HIP_TRY(gsl_sinterp_hip_krige_variance(st->ctx, st->kind, st->eps, st->d_x, st->n, (int)st->dim, st->dim, st->d_llt, st->llt_lda,
                                           st->d_b, st->d_dinv, st->denom, d_y, m, ytda, d_var, st->d_vwork, chunk), st->ctx);
  }
  HIP_TRY(gsl_sinterp_hip_krige_variance_clamp(st->ctx, d_var, m), st->ctx);   /* rounding residue where sigma^2 = 0 */
  return GSL_SUCCESS;
}

int gsl_sinterp_eval_variance_many(const gsl_sinterp *interp, const gsl_matrix *y, gsl_vector *var)
{
  if (!interp || !y || !var) GSL_ERROR("gsl_sinterp_eval_variance_many: null argument", GSL_EFAULT);
  if (y->size2 != interp->dim) GSL_ERROR("target matrix must have dim columns", GSL_EBADLEN);
  if (var->size != y->size1) GSL_ERROR("output length must equal the number of targets", GSL_EBADLEN);
  const size_t m = y->size1, dim = interp->dim;
  int vs = variance_status(interp);
  if (vs || m == 0) return vs;
  const rbf_state *st = rbf_of(interp);
  if (st->local_k) return local_eval_many(interp, y, NULL, var, NULL);
  gsl_sinterp_hip_ctx *c = st->ctx;
  stage_out out[1] = {STAGE_VECTOR(var)};
  host_stage hs;
  int s = host_stage_begin(&hs, c, y, dim, out, 1), es = GSL_SUCCESS;
  if (!hs.h) GSL_ERROR("gsl_sinterp_eval_variance_many: out of memory", GSL_ENOMEM);
  if (!s) es = gsl_sinterp_eval_variance_resident(interp, hs.d_y, m, dim, (double *)out[0].d);
  s = host_stage_end(&hs, s, !es);
  HIP_TRY(s, c);
  return es;
}

int gsl_sinterp_eval_variance_e(const gsl_sinterp *interp, const gsl_vector *y, double *var)
{
  if (!interp || !y || !var) GSL_ERROR("gsl_sinterp_eval_variance_e: null argument", GSL_EFAULT);
  *var = GSL_NAN;
  if (y->size != interp->dim) GSL_ERROR("target must have dim components", GSL_EBADLEN);
  double yy[3], out = GSL_NAN;
  for (size_t c = 0; c < interp->dim; c++) yy[c] = gsl_vector_get(y, c);
  gsl_matrix_view Y = gsl_matrix_view_array(yy, 1, interp->dim);
  gsl_vector_view V = gsl_vector_view_array(&out, 1);
  int st = gsl_sinterp_eval_variance_many(interp, &Y.matrix, &V.vector);
  if (st == GSL_SUCCESS) *var = out;
  return st;
}

/* ---- joint covariance and conditional simulation (csrc/hip/krige_cov.hip) ---- */
/* the state conditions of the variance entries, and the local route refused: it has no joint model */
static int covariance_status(const gsl_sinterp *interp)
{
  if (is_local(interp))
    GSL_ERROR("gsl_sinterp_eval_covariance / _simulate: not with gsl_sinterp_set_neighbours (the local route has no joint model)", GSL_EUNSUP);
  return variance_status(interp);
}

/* what the raw entries take of the kept model: ordinary kriging is order 0, q = 1, B = b and the 1 x 1 factor sqrt(1^T b) */
typedef struct {
  int order;
  size_t q;
  const double *shift, *scale, *d_B, *h_L;
  double l1;
} joint_model;

static void joint_model_of(const rbf_state *st, joint_model *j)
{
  j->order = st->drift; j->q = st->drift ? st->drift_q : 1;
  j->shift = st->drift ? st->drift_shift : NULL; j->scale = st->drift ? st->drift_scale : NULL;
  j->d_B = st->drift ? st->d_B : st->d_b;
  j->l1 = sqrt(st->denom);
  j->h_L = st->drift ? st->drift_L : &j->l1;
}

int gsl_sinterp_eval_covariance_resident(const gsl_sinterp *interp, const double *d_ya, size_t ma, size_t yatda, const double *d_yb,
                                         size_t mb, size_t ybtda, double *d_cov, size_t ctda)
{
  if (!interp) GSL_ERROR("gsl_sinterp_eval_covariance: null interpolant", GSL_EFAULT);
  int vs = covariance_status(interp);
  if (vs) return vs;
  rbf_state *st = rbf_of(interp);           /* the workspace is a grow-only cache inside the state */
  if (!d_yb) { mb = ma; ybtda = yatda; }
  if (ma == 0 || mb == 0) return GSL_SUCCESS;
  if (!d_ya || !d_cov) GSL_ERROR("gsl_sinterp_eval_covariance: null argument", GSL_EFAULT);
  if (yatda < st->dim || ybtda < st->dim) GSL_ERROR("gsl_sinterp_eval_covariance: a target pitch is below dim", GSL_EINVAL);
  if (ctda < mb) GSL_ERROR("gsl_sinterp_eval_covariance: ctda is below the number of columns", GSL_EINVAL);
  joint_model j;
  joint_model_of(st, &j);
  HIP_TRY(variance_workspace(st, gsl_sinterp_hip_krige_covariance_work(st->n, ma, d_yb ? mb : 0, j.q)), st->ctx);
  /* the factor lives on member 0, which does all the work */
  HIP_TRY(gsl_sinterp_hip_krige_covariance(st->ctx, st->kind, st->eps, j.order, j.shift, j.scale, st->d_x, st->n, (int)st->dim, st->dim,
                                           st->d_llt, st->llt_lda, j.d_B, st->n, st->d_dinv, j.h_L, d_ya, ma, yatda, d_yb, mb, ybtda, d_cov,
                                           ctda, st->d_vwork), st->ctx);
  return GSL_SUCCESS;
}

/* an m x cols host matrix, repacked dense and uploaded into a device buffer of its own (the caller frees *d) */
static int upload_dense(gsl_sinterp_hip_ctx *c, const gsl_matrix *a, double **d)
{
  const size_t cnt = a->size1 * a->size2;
  *d = NULL;
  double *h = (double *)malloc(cnt * sizeof(double));
  if (!h) return GSL_ENOMEM;
  for (size_t i = 0; i < a->size1; i++)
    for (size_t k = 0; k < a->size2; k++) h[i * a->size2 + k] = a->data[i * a->tda + k];
  int s = gsl_sinterp_hip_malloc(c, (void **)d, cnt * sizeof(double));
  if (!s) s = gsl_sinterp_hip_h2d(c, *d, h, cnt * sizeof(double));
  free(h);
  return s;
}

int gsl_sinterp_eval_covariance_many(const gsl_sinterp *interp, const gsl_matrix *ya, const gsl_matrix *yb, gsl_matrix *Cov)
{
  if (!interp || !ya || !Cov) GSL_ERROR("gsl_sinterp_eval_covariance_many: null argument", GSL_EFAULT);
  const size_t dim = interp->dim, ma = ya->size1, mb = yb ? yb->size1 : ma;
  if (ya->size2 != dim || (yb && yb->size2 != dim)) GSL_ERROR("target matrix must have dim columns", GSL_EBADLEN);
  if (Cov->size1 != ma || Cov->size2 != mb) GSL_ERROR("gsl_sinterp_eval_covariance_many: Cov must be ma x mb", GSL_EBADLEN);
  int vs = covariance_status(interp);
  if (vs || ma == 0 || mb == 0) return vs;
  gsl_sinterp_hip_ctx *c = rbf_of(interp)->ctx;
  stage_out out[1] = {STAGE_MATRIX(Cov)};
  host_stage hs;
  double *d_yb = NULL;
  int s = host_stage_begin(&hs, c, ya, dim, out, 1), es = GSL_SUCCESS;
  if (!hs.h) GSL_ERROR("gsl_sinterp_eval_covariance_many: out of memory", GSL_ENOMEM);
  if (!s && yb) s = upload_dense(c, yb, &d_yb);
  if (!s) es = gsl_sinterp_eval_covariance_resident(interp, hs.d_y, ma, dim, d_yb, mb, dim, (double *)out[0].d, mb);
  s = host_stage_end(&hs, s, !es);
  gsl_sinterp_hip_free(c, d_yb);
  HIP_TRY(s, c);
  return es;
}

int gsl_sinterp_simulate_resident(const gsl_sinterp *interp, const double *d_y, size_t m, size_t ytda, double sigma2, double jitter,
                                  const double *d_zn, size_t ztda, size_t n_draws, double *d_out, size_t otda)
{
  if (!interp) GSL_ERROR("gsl_sinterp_simulate: null interpolant", GSL_EFAULT);
  int vs = covariance_status(interp);
  if (vs) return vs;
  rbf_state *st = rbf_of(interp);
  if (!isfinite(sigma2) || !(sigma2 > 0.0)) GSL_ERROR("gsl_sinterp_simulate: sigma2 must be finite and positive", GSL_EINVAL);
  if (!isfinite(jitter) || jitter < 0.0) GSL_ERROR("gsl_sinterp_simulate: jitter must be finite and not negative", GSL_EINVAL);
  if (n_draws < 1) GSL_ERROR("gsl_sinterp_simulate: at least one draw", GSL_EBADLEN);
  if (m == 0) return GSL_SUCCESS;
  if (!d_y || !d_zn || !d_out) GSL_ERROR("gsl_sinterp_simulate: null argument", GSL_EFAULT);
  if (ytda < st->dim) GSL_ERROR("gsl_sinterp_simulate: the target pitch is below dim", GSL_EINVAL);
  if (ztda < n_draws || otda < n_draws) GSL_ERROR("gsl_sinterp_simulate: ztda or otda is below the number of draws", GSL_EINVAL);
  joint_model j;
  joint_model_of(st, &j);
  /* [mean (m, rounded up to even) | the raw entry's work] */
  const size_t m2 = (m + 1) / 2 * 2;
  HIP_TRY(variance_workspace(st, m2 + gsl_sinterp_hip_krige_simulate_work(st->n, m, n_draws, j.q)), st->ctx);
  double *d_mean = st->d_vwork;
  HIP_TRY(rbf_sweep(st, st->ctx, st->d_x, st->d_w, d_y, m, ytda, d_mean), st->ctx);        /* field 0's predictor: the bits of eval */
  int s = gsl_sinterp_hip_krige_simulate(st->ctx, st->kind, st->eps, j.order, j.shift, j.scale, st->d_x, st->n, (int)st->dim, st->dim,
                                         st->d_llt, st->llt_lda, j.d_B, st->n, st->d_dinv, j.h_L, d_y, m, ytda, d_mean, sigma2, jitter, d_zn,
                                         ztda, n_draws, d_out, otda, st->d_vwork + m2);
  if (s == GSL_EDOM)
    GSL_ERROR("gsl_sinterp_simulate: the joint covariance of the targets plus jitter is not numerically positive definite (targets on data sites of a nugget-free model, or repeated targets): every draw is NaN; pass a jitter such as 1e-10",
              GSL_EDOM);
  HIP_TRY(s, st->ctx);
  return GSL_SUCCESS;
}

int gsl_sinterp_simulate_many(const gsl_sinterp *interp, const gsl_matrix *y, double sigma2, double jitter, const gsl_matrix *Zn,
                              gsl_matrix *Out)
{
  if (!interp || !y || !Zn || !Out) GSL_ERROR("gsl_sinterp_simulate_many: null argument", GSL_EFAULT);
  const size_t dim = interp->dim, m = y->size1, S = Zn->size2;
  if (y->size2 != dim) GSL_ERROR("target matrix must have dim columns", GSL_EBADLEN);
  if (S < 1 || Zn->size1 != m || Out->size1 != m || Out->size2 != S)
    GSL_ERROR("gsl_sinterp_simulate_many: Zn and Out must be m x S with S >= 1", GSL_EBADLEN);
  int vs = covariance_status(interp);
  if (vs) return vs;
  if (!isfinite(sigma2) || !(sigma2 > 0.0)) GSL_ERROR("gsl_sinterp_simulate: sigma2 must be finite and positive", GSL_EINVAL);
  if (!isfinite(jitter) || jitter < 0.0) GSL_ERROR("gsl_sinterp_simulate: jitter must be finite and not negative", GSL_EINVAL);
  if (m == 0) return GSL_SUCCESS;
  gsl_sinterp_hip_ctx *c = rbf_of(interp)->ctx;
  stage_out out[1] = {STAGE_MATRIX(Out)};
  host_stage hs;
  double *d_zn = NULL;
  int s = host_stage_begin(&hs, c, y, dim, out, 1), es = GSL_SUCCESS;
  if (!hs.h) GSL_ERROR("gsl_sinterp_simulate_many: out of memory", GSL_ENOMEM);
  if (!s) s = upload_dense(c, Zn, &d_zn);
  if (!s) es = gsl_sinterp_simulate_resident(interp, hs.d_y, m, dim, sigma2, jitter, d_zn, S, S, (double *)out[0].d, S);
  s = host_stage_end(&hs, s, !es || es == GSL_EDOM);      /* GSL_EDOM: every entry is NaN, and says so in Out */
  gsl_sinterp_hip_free(c, d_zn);
  HIP_TRY(s, c);
  return es;
}

int gsl_sinterp_eval_local_many(const gsl_sinterp *interp, const gsl_matrix *y, gsl_vector *s, gsl_vector *var, int *idx)
{
  if (!interp || !y) GSL_ERROR("gsl_sinterp_eval_local_many: null argument", GSL_EFAULT);
  if (!desc_of(interp->type)->krige) GSL_ERROR("gsl_sinterp_eval_local_many: kriging interpolants only", GSL_EINVAL);
  const rbf_state *st = rbf_of(interp);
  if (!st->d_w || st->nf == 0) GSL_ERROR("gsl_sinterp_eval_local_many: interpolant not initialised", GSL_EINVAL);
  if (!st->local_k) GSL_ERROR("gsl_sinterp_eval_local_many: initialised without gsl_sinterp_set_neighbours", GSL_EINVAL);
  if (y->size2 != interp->dim) GSL_ERROR("target matrix must have dim columns", GSL_EBADLEN);
  if ((s && s->size != y->size1) || (var && var->size != y->size1)) GSL_ERROR("output length must equal the number of targets", GSL_EBADLEN);
  if (!s && !var && !idx) return GSL_SUCCESS;
  return local_eval_many(interp, y, s, var, idx);
}

/* ---- value + gradient (RBF family): dispatch on the type here, no slot in gsl_sinterp_type ---- */
static int grad_status(const gsl_sinterp *interp)
{
  if (mesh_method(interp, MESH_NATURAL)) GSL_ERROR("gsl_sinterp_eval_grad: not for natural-neighbour interpolants", GSL_EUNSUP);
  if (mesh_method(interp, MESH_CUBIC)) return GSL_SUCCESS;     /* the one mesh method with a continuous gradient */
  if (shepard_of(interp)) return GSL_SUCCESS;
  if (!rbf_of(interp))
    GSL_ERROR("gsl_sinterp_eval_grad: RBF-family interpolants only (the piecewise-linear gradient is constant per leaf)", GSL_EUNSUP);
  if (is_local(interp))
    GSL_ERROR("gsl_sinterp_eval_grad: not with gsl_sinterp_set_neighbours (the local predictor is discontinuous where the neighbour set changes)", GSL_EUNSUP);
  return GSL_SUCCESS;
}

int gsl_sinterp_eval_grad_resident(const gsl_sinterp *interp, const double *d_y, size_t m, size_t ytda, double *d_s, double *d_g,
                                   size_t gtda)
{
  if (!interp) GSL_ERROR("gsl_sinterp_eval_grad_resident: null interpolant", GSL_EFAULT);
  if (m > 0 && (!d_y || !d_g)) GSL_ERROR("gsl_sinterp_eval_grad_resident: null argument", GSL_EFAULT);
  int gs = grad_status(interp);
  if (gs) return gs;
  const mesh_state *ms = mesh_of(interp);                /* Clough-Tocher: grad_status let no other mesh type through */
  if (ms) {
    if (!ms->dev) GSL_ERROR("gsl_sinterp_eval_grad: interpolant not initialised", GSL_EINVAL);
    if (m > 0 && !d_s) GSL_ERROR("gsl_sinterp_eval_grad_resident: Clough-Tocher interpolants need d_s (the locate step writes through it)", GSL_EFAULT);
    if (gtda < 2) GSL_ERROR("gsl_sinterp_eval_grad_resident: gradient rows shorter than dim", GSL_EINVAL);
    return simplex_mesh_device_eval_cubic_resident(ms->dev, d_y, m, ytda, d_s, d_g, gtda, NULL);
  }
  const shepard_state *sh = shepard_of(interp);
  if (sh) {
    if (!sh->ready) GSL_ERROR("gsl_sinterp_eval_grad: interpolant not initialised", GSL_EINVAL);
    if (ytda < sh->dim || gtda < sh->dim) GSL_ERROR("gsl_sinterp_eval_grad_resident: target or gradient rows shorter than dim", GSL_EINVAL);
    return m == 0 ? GSL_SUCCESS : shepard_sweep(sh, d_y, m, ytda, d_s, d_g, gtda, NULL);
  }
  const rbf_state *st = rbf_of(interp);
  if (!st->d_w || st->nf == 0) GSL_ERROR("gsl_sinterp_eval_grad: interpolant not initialised", GSL_EINVAL);
  /* the tail: the affine polynomial, or kriging's constant mean; member 0 evaluates every target (as
     gsl_sinterp_eval_resident does) */
  double tail[4] = {st->mean, 0.0, 0.0, 0.0};
  if (st->affine) memcpy(tail, st->poly, sizeof tail);
  HIP_TRY(gsl_sinterp_hip_rbf_eval_grad(st->ctx, st->kind, st->eps, (st->affine || (st->krige && !st->drift)) ? tail : NULL, st->d_x, st->n,
                                        (int)st->dim, st->dim, st->d_w, d_y, m, ytda, d_s, d_g, gtda, st->model_id), st->ctx);
  if (st->drift)                                        /* the drift and its gradient behind the plain sweep, as the value entries add it */
    HIP_TRY(gsl_sinterp_hip_drift_add(st->ctx, st->drift, st->drift_shift, st->drift_scale, st->f_coef[0], 1, d_y, m, (int)st->dim, ytda, d_s, 1,
                                      d_g, gtda), st->ctx);
  return GSL_SUCCESS;
}

int gsl_sinterp_eval_grad_many(const gsl_sinterp *interp, const gsl_matrix *y, gsl_vector *sv, gsl_matrix *g)
{
  if (!interp || !y || !g) GSL_ERROR("gsl_sinterp_eval_grad_many: null argument", GSL_EFAULT);
  int gs = grad_status(interp);
  if (gs) return gs;
  const size_t m = y->size1, dim = interp->dim;
  if (y->size2 != dim) GSL_ERROR("target matrix must have dim columns", GSL_EBADLEN);
  if (g->size1 != m || g->size2 != dim) GSL_ERROR("gradient matrix must be (number of targets) x dim", GSL_EBADLEN);
  if (sv && sv->size != m) GSL_ERROR("output length must equal the number of targets", GSL_EBADLEN);
  const mesh_state *ms = mesh_of(interp);                /* Clough-Tocher: grad_status let no other mesh type through */
  if (ms) {
    if (!ms->dev) GSL_ERROR("gsl_sinterp_eval_grad: interpolant not initialised", GSL_EINVAL);
    if (sv) return simplex_mesh_device_eval_cubic_many(ms->dev, y, sv, g, NULL);
    if (m == 0) return GSL_SUCCESS;
    gsl_vector *tmp = gsl_vector_alloc(m);                  /* a gradient-only call: the values are dropped */
    if (!tmp) GSL_ERROR("gsl_sinterp_eval_grad_many: out of memory", GSL_ENOMEM);
    const int cs = simplex_mesh_device_eval_cubic_many(ms->dev, y, tmp, g, NULL);
    gsl_vector_free(tmp);
    return cs;
  }
  const shepard_state *sh = shepard_of(interp);
  if (sh) {
    if (!sh->ready) GSL_ERROR("gsl_sinterp_eval_grad: interpolant not initialised", GSL_EINVAL);
    return shepard_eval_host(sh, y, sv, g, NULL);
  }
  const rbf_state *st = rbf_of(interp);
  if (!st->d_w || st->nf == 0) GSL_ERROR("gsl_sinterp_eval_grad: interpolant not initialised", GSL_EINVAL);
  if (m == 0) return GSL_SUCCESS;
  gsl_sinterp_hip_ctx *c = st->ctx;
  stage_out out[2] = {STAGE_MATRIX(g), STAGE_VECTOR(sv)};     /* no sv: no room for values, nothing downloaded for them */
  host_stage hs;
  int s = host_stage_begin(&hs, c, y, dim, out, 2), es = GSL_SUCCESS;
  if (!hs.h) GSL_ERROR("gsl_sinterp_eval_grad_many: out of memory", GSL_ENOMEM);
  if (!s) es = gsl_sinterp_eval_grad_resident(interp, hs.d_y, m, dim, (double *)out[1].d, (double *)out[0].d, dim);
  s = host_stage_end(&hs, s, !es);
  HIP_TRY(s, c);
  return es;
}

int gsl_sinterp_eval_grad_e(const gsl_sinterp *interp, const gsl_vector *y, double *s, gsl_vector *g)
{
  if (s) *s = GSL_NAN;
  if (g) for (size_t a = 0; a < g->size; a++) gsl_vector_set(g, a, GSL_NAN);
  if (!interp || !y || !s || !g) GSL_ERROR("gsl_sinterp_eval_grad_e: null argument", GSL_EFAULT);
  int gs = grad_status(interp);
  if (gs) return gs;
  if (y->size != interp->dim) GSL_ERROR("target must have dim components", GSL_EBADLEN);
  if (g->size != interp->dim) GSL_ERROR("gradient must have dim components", GSL_EBADLEN);
  double yy[3], gg[3], out = GSL_NAN;
  for (size_t c = 0; c < interp->dim; c++) yy[c] = gsl_vector_get(y, c);
  gsl_matrix_view Y = gsl_matrix_view_array(yy, 1, interp->dim), G = gsl_matrix_view_array(gg, 1, interp->dim);
  gsl_vector_view S = gsl_vector_view_array(&out, 1);
  int st = gsl_sinterp_eval_grad_many(interp, &Y.matrix, &S.vector, &G.matrix);
  if (st != GSL_SUCCESS) return st;
  *s = out;
  for (size_t c = 0; c < interp->dim; c++) gsl_vector_set(g, c, gg[c]);
  return GSL_SUCCESS;
}

/* ---- several fields on one set of centres (RBF family): dispatch on the type here, no slot in gsl_sinterp_type ---- */
static int fields_status(const gsl_sinterp *interp)
{
  const type_desc *d = desc_of(interp->type);
  if (d->noun) return noun_error(d, "gsl_sinterp fields: not for %s interpolants (one response)", GSL_EUNSUP);
  if (d->family != FAM_RBF)
    GSL_ERROR("gsl_sinterp fields: RBF-family interpolants only (several responses per leaf of the linear types: a separate entry)", GSL_EUNSUP);
  if (is_local(interp)) GSL_ERROR("gsl_sinterp fields: not with gsl_sinterp_set_neighbours (local kriging has one field)", GSL_EUNSUP);
  return GSL_SUCCESS;
}

int gsl_sinterp_init_fields(gsl_sinterp *interp, const gsl_matrix *x, const gsl_matrix *F)
{
  if (!interp || !x || !F) GSL_ERROR("gsl_sinterp_init_fields: null argument", GSL_EFAULT);
  int fs = fields_status(interp);
  if (fs) return fs;
  if (F->size1 != interp->size) GSL_ERROR("gsl_sinterp_init_fields: the response matrix must have size rows", GSL_EBADLEN);
  if (x->size1 != interp->size || x->size2 != interp->dim) GSL_ERROR("gsl_sinterp_init_fields: the centre matrix must be size x dim", GSL_EBADLEN);
  if (F->size2 < 1 || F->size2 > GSL_SINTERP_MAX_FIELDS) GSL_ERROR("gsl_sinterp_init_fields: 1 .. GSL_SINTERP_MAX_FIELDS fields", GSL_EINVAL);
  return rbf_init_fields(interp, x, F->data, F->tda, 1, F->size2);
}

static int linear_fields_status(const gsl_sinterp *interp);

size_t gsl_sinterp_n_fields(const gsl_sinterp *interp)
{
  if (!interp) return 0;
  if (tree_of(interp)) return tree_of(interp)->dev ? tree_of(interp)->nf : 0;
  if (mesh_method(interp, MESH_LINEAR)) return mesh_of(interp)->dev ? mesh_of(interp)->nf : 0;
  const rbf_state *st = rbf_of(interp);
  return st && st->d_w ? st->nf : 0;
}

int gsl_sinterp_eval_fields_resident(const gsl_sinterp *interp, const double *d_y, size_t m, size_t ytda, double *d_s, size_t stda)
{
  if (!interp) GSL_ERROR("gsl_sinterp_eval_fields_resident: null interpolant", GSL_EFAULT);
  if (m > 0 && (!d_y || !d_s)) GSL_ERROR("gsl_sinterp_eval_fields_resident: null argument", GSL_EFAULT);
  int fs = fields_status(interp);
  if (fs) return fs;
  const rbf_state *st = rbf_of(interp);
  if (!st->d_w || st->nf == 0) GSL_ERROR("gsl_sinterp_eval_fields: interpolant not initialised", GSL_EINVAL);
  if (stda < st->nf) GSL_ERROR("gsl_sinterp_eval_fields_resident: row pitch below the number of fields", GSL_EINVAL);
  /* the tails: the affine polynomials, or kriging's constant means; member 0 evaluates every target (as the gradient and
     variance entries do) */
  double tail[GSL_SINTERP_MAX_FIELDS * 4];
  const size_t td = st->dim + 1;
  for (size_t q = 0; q < st->nf; q++)
    for (size_t a = 0; a < td; a++) tail[q * td + a] = st->affine ? st->f_poly[q][a] : (a == 0 ? st->f_mean[q] : 0.0);
  HIP_TRY(gsl_sinterp_hip_rbf_eval_fields(st->ctx, st->kind, st->eps, (st->affine || (st->krige && !st->drift)) ? tail : NULL, st->d_x, st->n,
                                          (int)st->dim, st->dim, st->d_w, st->n, st->nf, d_y, m, ytda, d_s, stda, st->model_id), st->ctx);
  if (st->drift) {                                      /* f_coef rows are GSL_SINTERP_DRIFT_MAX_TERMS apart: pack q per field */
    double coef[GSL_SINTERP_MAX_FIELDS * GSL_SINTERP_DRIFT_MAX_TERMS];
    for (size_t q = 0; q < st->nf; q++) memcpy(coef + q * st->drift_q, st->f_coef[q], st->drift_q * sizeof(double));
    HIP_TRY(gsl_sinterp_hip_drift_add(st->ctx, st->drift, st->drift_shift, st->drift_scale, coef, st->nf, d_y, m, (int)st->dim, ytda, d_s, stda,
                                      NULL, 0), st->ctx);
  }
  return GSL_SUCCESS;
}

int gsl_sinterp_eval_fields_many(const gsl_sinterp *interp, const gsl_matrix *y, gsl_matrix *S)
{
  if (!interp || !y || !S) GSL_ERROR("gsl_sinterp_eval_fields_many: null argument", GSL_EFAULT);
  int fs = fields_status(interp);
  if (fs) return fs;
  const size_t m = y->size1, dim = interp->dim;
  if (y->size2 != dim) GSL_ERROR("target matrix must have dim columns", GSL_EBADLEN);
  if (S->size1 != m) GSL_ERROR("output matrix must have one row per target", GSL_EBADLEN);
  const rbf_state *st = rbf_of(interp);
  if (!st->d_w || st->nf == 0) GSL_ERROR("gsl_sinterp_eval_fields: interpolant not initialised", GSL_EINVAL);
  const size_t K = st->nf;
  if (S->size2 != K) GSL_ERROR("output matrix must have one column per field", GSL_EBADLEN);
  if (m == 0) return GSL_SUCCESS;
  gsl_sinterp_hip_ctx *c = st->ctx;
  stage_out out[1] = {STAGE_MATRIX(S)};
  host_stage hs;
  int s = host_stage_begin(&hs, c, y, dim, out, 1), es = GSL_SUCCESS;
  if (!hs.h) GSL_ERROR("gsl_sinterp_eval_fields_many: out of memory", GSL_ENOMEM);
  if (!s) es = gsl_sinterp_eval_fields_resident(interp, hs.d_y, m, dim, (double *)out[0].d, K);
  s = host_stage_end(&hs, s, !es);
  HIP_TRY(s, c);
  return es;
}

int gsl_sinterp_eval_fields_e(const gsl_sinterp *interp, const gsl_vector *y, gsl_vector *s)
{
  if (s) for (size_t q = 0; q < s->size; q++) gsl_vector_set(s, q, GSL_NAN);
  if (!interp || !y || !s) GSL_ERROR("gsl_sinterp_eval_fields_e: null argument", GSL_EFAULT);
  int fs = fields_status(interp);
  if (fs) return fs;
  if (y->size != interp->dim) GSL_ERROR("target must have dim components", GSL_EBADLEN);
  const size_t K = gsl_sinterp_n_fields(interp);
  if (K == 0) GSL_ERROR("gsl_sinterp_eval_fields: interpolant not initialised", GSL_EINVAL);
  if (s->size != K) GSL_ERROR("output must have one entry per field", GSL_EBADLEN);
  double yy[3], out[GSL_SINTERP_MAX_FIELDS];
  for (size_t c = 0; c < interp->dim; c++) yy[c] = gsl_vector_get(y, c);
  gsl_matrix_view Y = gsl_matrix_view_array(yy, 1, interp->dim), S = gsl_matrix_view_array(out, 1, K);
  int st = gsl_sinterp_eval_fields_many(interp, &Y.matrix, &S.matrix);
  if (st != GSL_SUCCESS) return st;
  for (size_t q = 0; q < K; q++) gsl_vector_set(s, q, out[q]);
  return GSL_SUCCESS;
}

/* ---- several responses and their gradients on the linear types: the separate entries (csrc/hip/linear_fields.hip) ---- */
static int linear_fields_status(const gsl_sinterp *interp)
{
  if (!tree_of(interp) && !mesh_method(interp, MESH_LINEAR))
    GSL_ERROR("gsl_sinterp_linear fields: gsl_sinterp_linear_simplex and gsl_sinterp_linear_mesh only", GSL_EUNSUP);
  return GSL_SUCCESS;
}

int gsl_sinterp_linear_init_fields(gsl_sinterp *interp, const gsl_matrix *x, const gsl_matrix *F)
{
  if (!interp || !x || !F) GSL_ERROR("gsl_sinterp_linear_init_fields: null argument", GSL_EFAULT);
  int fs = linear_fields_status(interp);
  if (fs) return fs;
  if (F->size1 != interp->size) GSL_ERROR("gsl_sinterp_linear_init_fields: the response matrix must have size rows", GSL_EBADLEN);
  if (x->size1 != interp->size || x->size2 != interp->dim) GSL_ERROR("gsl_sinterp_linear_init_fields: the centre matrix must be size x dim", GSL_EBADLEN);
  if (F->size2 < 1 || F->size2 > GSL_SINTERP_MAX_FIELDS) GSL_ERROR("gsl_sinterp_linear_init_fields: 1 .. GSL_SINTERP_MAX_FIELDS fields", GSL_EINVAL);
  /* gsl_sinterp_init with column 0 as the response: tree or imported triangulation, mirror, scalar binding */
  gsl_vector f0 = {F->size1, F->tda, F->data, NULL, 0};
  int s = interp->type->init(interp, x, &f0);
  if (s) return s;
  if (tree_of(interp)) {
    simplex_state *st = tree_of(interp);
    s = simplex_tree_device_set_responses(st->dev, F);
    st->nf = s ? 0 : F->size2;
  } else {
    mesh_state *st = mesh_of(interp);
    s = simplex_mesh_device_set_responses(st->dev, F);
    st->nf = s ? 0 : F->size2;
  }
  return s;
}

/* K of an initialised linear interpolant, 0 = not initialised.  An interpolant that came from gsl_sinterp_init or
   gsl_sinterp_fread holds one field whose matrix binding is made here, at the first use, from the private response copy */
static size_t linear_fields_ready(const gsl_sinterp *interp, int *status)
{
  *status = GSL_SUCCESS;
  if (tree_of(interp)) {
    const simplex_state *st = tree_of(interp);
    if (!st->dev || st->nf == 0) return 0;
    if (simplex_tree_device_n_responses(st->dev) == 0) {
      gsl_matrix_view F = gsl_matrix_view_array_with_tda(st->f->data, st->n, 1, st->f->stride);
      *status = simplex_tree_device_set_responses(st->dev, &F.matrix);
    }
    return *status ? 0 : st->nf;
  }
  const mesh_state *st = mesh_of(interp);
  if (!st->dev || st->nf == 0) return 0;
  if (simplex_mesh_device_n_responses(st->dev) == 0) {
    gsl_matrix_view F = gsl_matrix_view_array_with_tda(st->f->data, st->n, 1, st->f->stride);
    *status = simplex_mesh_device_set_responses(st->dev, &F.matrix);
  }
  return *status ? 0 : st->nf;
}

int gsl_sinterp_linear_eval_fields_resident(const gsl_sinterp *interp, const double *d_y, size_t m, size_t ytda, double *d_S, size_t stda,
                                            double *d_G, size_t gtda, int *d_leaf)
{
  if (!interp) GSL_ERROR("gsl_sinterp_linear_eval_fields_resident: null interpolant", GSL_EFAULT);
  if (m > 0 && (!d_y || !d_S)) GSL_ERROR("gsl_sinterp_linear_eval_fields_resident: null argument", GSL_EFAULT);
  int fs = linear_fields_status(interp);
  if (fs) return fs;
  const size_t K = linear_fields_ready(interp, &fs);
  if (fs) return fs;
  if (K == 0) GSL_ERROR("gsl_sinterp_linear_eval_fields: interpolant not initialised", GSL_EINVAL);
  if (stda < K || (d_G && gtda < K * interp->dim))
    GSL_ERROR("gsl_sinterp_linear_eval_fields_resident: row pitch below K (values) or K dim (gradients)", GSL_EINVAL);
  if (tree_of(interp)) return simplex_tree_device_eval_fields_resident(tree_of(interp)->dev, d_y, m, ytda, d_S, stda, d_G, gtda, d_leaf);
  return simplex_mesh_device_eval_fields_resident(mesh_of(interp)->dev, d_y, m, ytda, d_S, stda, d_G, gtda, d_leaf);
}

int gsl_sinterp_linear_eval_fields_many(const gsl_sinterp *interp, const gsl_matrix *y, gsl_matrix *S, gsl_matrix *G, int *leaf)
{
  if (!interp || !y || !S) GSL_ERROR("gsl_sinterp_linear_eval_fields_many: null argument", GSL_EFAULT);
  int fs = linear_fields_status(interp);
  if (fs) return fs;
  const size_t m = y->size1, dim = interp->dim;
  if (y->size2 != dim) GSL_ERROR("target matrix must have dim columns", GSL_EBADLEN);
  if (S->size1 != m) GSL_ERROR("output matrix must have one row per target", GSL_EBADLEN);
  const size_t K = linear_fields_ready(interp, &fs);
  if (fs) return fs;
  if (K == 0) GSL_ERROR("gsl_sinterp_linear_eval_fields: interpolant not initialised", GSL_EINVAL);
  if (S->size2 != K) GSL_ERROR("output matrix must have one column per field", GSL_EBADLEN);
  if (G && (G->size1 != m || G->size2 != K * dim)) GSL_ERROR("gradient matrix must be (number of targets) x (K dim)", GSL_EBADLEN);
  if (tree_of(interp)) return simplex_tree_device_eval_fields_many(tree_of(interp)->dev, y, S, G, leaf);
  return simplex_mesh_device_eval_fields_many(mesh_of(interp)->dev, y, S, G, leaf);
}

int gsl_sinterp_linear_eval_fields_e(const gsl_sinterp *interp, const gsl_vector *y, gsl_vector *s, gsl_matrix *g)
{
  if (s) for (size_t q = 0; q < s->size; q++) gsl_vector_set(s, q, GSL_NAN);
  if (g) for (size_t q = 0; q < g->size1; q++) for (size_t a = 0; a < g->size2; a++) gsl_matrix_set(g, q, a, GSL_NAN);
  if (!interp || !y || !s) GSL_ERROR("gsl_sinterp_linear_eval_fields_e: null argument", GSL_EFAULT);
  int fs = linear_fields_status(interp);
  if (fs) return fs;
  const size_t dim = interp->dim;
  if (y->size != dim) GSL_ERROR("target must have dim components", GSL_EBADLEN);
  const size_t K = gsl_sinterp_n_fields(interp);
  if (K == 0) GSL_ERROR("gsl_sinterp_linear_eval_fields: interpolant not initialised", GSL_EINVAL);
  if (s->size != K) GSL_ERROR("output must have one entry per field", GSL_EBADLEN);
  if (g && (g->size1 != K || g->size2 != dim)) GSL_ERROR("gradient must be K x dim", GSL_EBADLEN);
  double yy[3], out[GSL_SINTERP_MAX_FIELDS], gg[GSL_SINTERP_MAX_FIELDS * 3];
  for (size_t c = 0; c < dim; c++) yy[c] = gsl_vector_get(y, c);
  gsl_matrix_view Y = gsl_matrix_view_array(yy, 1, dim), S = gsl_matrix_view_array(out, 1, K), G = gsl_matrix_view_array(gg, 1, K * dim);
  int st = gsl_sinterp_linear_eval_fields_many(interp, &Y.matrix, &S.matrix, g ? &G.matrix : NULL, NULL);
  if (st != GSL_SUCCESS) return st;
  for (size_t q = 0; q < K; q++) {
    gsl_vector_set(s, q, out[q]);
    if (g) for (size_t a = 0; a < dim; a++) gsl_matrix_set(g, q, a, gg[q * dim + a]);
  }
  return GSL_SUCCESS;
}

/* the state of an initialised RBF-family interpolant when q names one of its fields, else NULL with *status set */
static const rbf_state *field_state(const gsl_sinterp *interp, size_t q, int *status)
{
  *status = fields_status(interp);
  if (*status) return NULL;
  const rbf_state *st = rbf_of(interp);
  if (!st->d_w || st->nf == 0) { *status = GSL_EINVAL; gsl_error("gsl_sinterp fields: interpolant not initialised", __FILE__, __LINE__, GSL_EINVAL); return NULL; }
  if (q >= st->nf) { *status = GSL_EBADLEN; gsl_error("gsl_sinterp fields: no such field", __FILE__, __LINE__, GSL_EBADLEN); return NULL; }
  return st;
}

int gsl_sinterp_get_field_weights(const gsl_sinterp *interp, size_t q, gsl_vector *w)
{
  if (!interp || !w) GSL_ERROR("gsl_sinterp_get_field_weights: null argument", GSL_EFAULT);
  int status;
  const rbf_state *st = field_state(interp, q, &status);
  if (!st) return status;
  if (w->size != st->n) GSL_ERROR("gsl_sinterp_get_field_weights: wrong length", GSL_EBADLEN);
  double *h = (double *)malloc(st->n * sizeof(double));
  if (!h) GSL_ERROR("gsl_sinterp_get_field_weights: out of memory", GSL_ENOMEM);
  int s = gsl_sinterp_hip_d2h(st->ctx, h, st->d_w + q * st->n, st->n * sizeof(double));
  if (!s) for (size_t i = 0; i < st->n; i++) gsl_vector_set(w, i, h[i]);
  free(h);
  HIP_TRY(s, st->ctx);
  return GSL_SUCCESS;
}

int gsl_sinterp_field_mean(const gsl_sinterp *interp, size_t q, double *mean)
{
  if (!interp || !mean) GSL_ERROR("gsl_sinterp_field_mean: null argument", GSL_EFAULT);
  int status;
  const rbf_state *st = field_state(interp, q, &status);
  if (!st) return status;
  if (!st->krige) GSL_ERROR("gsl_sinterp_field_mean: kriging interpolants only", GSL_EINVAL);
  if (interp->drift > 0 || st->drift) GSL_ERROR("gsl_sinterp_field_mean: with a drift there is no single mean (gsl_sinterp_drift_coefficients)", GSL_EUNSUP);
  *mean = st->f_mean[q];
  return GSL_SUCCESS;
}

int gsl_sinterp_field_poly(const gsl_sinterp *interp, size_t q, gsl_vector *c)
{
  if (!interp || !c) GSL_ERROR("gsl_sinterp_field_poly: null argument", GSL_EFAULT);
  int status;
  const rbf_state *st = field_state(interp, q, &status);
  if (!st) return status;
  if (!st->affine) GSL_ERROR("gsl_sinterp_field_poly: affine thin-plate-spline interpolants only", GSL_EINVAL);
  if (c->size != st->dim + 1) GSL_ERROR("gsl_sinterp_field_poly: vector length must be dim + 1", GSL_EBADLEN);
  for (size_t a = 0; a <= st->dim; a++) gsl_vector_set(c, a, st->f_poly[q][a]);
  return GSL_SUCCESS;
}

int gsl_sinterp_poly(const gsl_sinterp *interp, gsl_vector *c)
{
  if (!interp || !c) GSL_ERROR("gsl_sinterp_poly: null argument", GSL_EFAULT);
  if (!desc_of(interp->type)->affine) GSL_ERROR("gsl_sinterp_poly: affine thin-plate-spline interpolants only", GSL_EINVAL);
  const rbf_state *st = rbf_of(interp);
  if (!st->d_w || st->nf == 0) GSL_ERROR("gsl_sinterp_poly: interpolant not initialised", GSL_EINVAL);
  if (c->size != st->dim + 1) GSL_ERROR("gsl_sinterp_poly: vector length must be dim + 1", GSL_EBADLEN);
  for (size_t a = 0; a <= st->dim; a++) gsl_vector_set(c, a, st->poly[a]);
  return GSL_SUCCESS;
}

int gsl_sinterp_mean(const gsl_sinterp *interp, double *mean)
{
  if (!interp || !mean) GSL_ERROR("gsl_sinterp_mean: null argument", GSL_EFAULT);
  if (!desc_of(interp->type)->krige) GSL_ERROR("gsl_sinterp_mean: kriging interpolants only", GSL_EINVAL);
  if (is_local(interp)) GSL_ERROR("gsl_sinterp_mean: not with gsl_sinterp_set_neighbours (every neighbourhood estimates its own mean)", GSL_EUNSUP);
  if (interp->drift > 0 || rbf_of(interp)->drift) GSL_ERROR("gsl_sinterp_mean: with a drift there is no single mean (gsl_sinterp_drift_coefficients)", GSL_EUNSUP);
  const rbf_state *st = rbf_of(interp);
  if (!st->d_w || st->nf == 0) GSL_ERROR("gsl_sinterp_mean: interpolant not initialised", GSL_EINVAL);
  *mean = st->mean;
  return GSL_SUCCESS;
}

int gsl_sinterp_set_solver(gsl_sinterp *interp, int solver)
{
  if (!interp) GSL_ERROR("gsl_sinterp_set_solver: null interpolant", GSL_EFAULT);
  if (solver < GSL_SINTERP_SOLVER_DEFAULT || solver > GSL_SINTERP_SOLVER_LU_REFINE)
    GSL_ERROR("gsl_sinterp_set_solver: unknown solver", GSL_EINVAL);
  const type_desc *d = desc_of(interp->type);
  if (d->family != FAM_RBF) GSL_ERROR("gsl_sinterp_set_solver: not an RBF interpolant", GSL_EINVAL);
  /* kriging and the affine thin-plate spline solve saddle systems on routes of their own (7 / 8, 9 / 10): accepting a
     solver here and ignoring it at init would be a silent no-op */
  if ((d->krige || d->affine) && solver != GSL_SINTERP_SOLVER_DEFAULT)
    GSL_ERROR("gsl_sinterp_set_solver: kriging / affine thin-plate-spline interpolants choose their own route", GSL_EINVAL);
  if (d->kind == GSL_SINTERP_RBF_TPS && (solver == GSL_SINTERP_SOLVER_CHOLESKY2 || solver == GSL_SINTERP_SOLVER_PCHOLESKY))
    GSL_ERROR("gsl_sinterp_set_solver: the thin-plate-spline matrix is indefinite (zero diagonal): no Cholesky-type solver", GSL_EINVAL);
  interp->solver = solver;
  return GSL_SUCCESS;
}

int gsl_sinterp_set_rcond(gsl_sinterp *interp, int want)
{
  if (!interp) GSL_ERROR("gsl_sinterp_set_rcond: null interpolant", GSL_EFAULT);
  if (want && (desc_of(interp->type)->krige || desc_of(interp->type)->affine))
    GSL_ERROR("gsl_sinterp_set_rcond: no condition estimate on the kriging / affine thin-plate-spline routes", GSL_EINVAL);
  interp->want_rcond = want != 0;
  return GSL_SUCCESS;
}

int gsl_sinterp_rcond(const gsl_sinterp *interp, double *rcond)
{
  if (!interp || !rcond) GSL_ERROR("gsl_sinterp_rcond: null argument", GSL_EFAULT);
  *rcond = interp->rcond;
  if (interp->rcond != interp->rcond) GSL_ERROR("gsl_sinterp_rcond: no estimate available (set_rcond + a Cholesky solver + init)", GSL_EINVAL);
  return GSL_SUCCESS;
}

int gsl_sinterp_route(const gsl_sinterp *interp) { return interp ? interp->route : 0; }

int gsl_sinterp_set_triangulation(gsl_sinterp *interp, const int *triangles, const int *neighbours, size_t n_triangles)
{
  if (!interp || !triangles) GSL_ERROR("gsl_sinterp_set_triangulation: null argument", GSL_EFAULT);
  mesh_state *st = mesh_of(interp);
  if (!st || !desc_of(interp->type)->imported) GSL_ERROR("gsl_sinterp_set_triangulation: imported-triangulation interpolants only", GSL_EINVAL);
  const size_t w = st->dim + 1;                          /* ids per simplex */
  if (n_triangles < 1 || n_triangles > (size_t)INT_MAX / w) GSL_ERROR("gsl_sinterp_set_triangulation: bad triangle count", GSL_EINVAL);
  int *t = (int *)malloc(w * n_triangles * sizeof(int)), *nb = neighbours ? (int *)malloc(w * n_triangles * sizeof(int)) : NULL;
  if (!t || (neighbours && !nb)) { free(t); free(nb); GSL_ERROR("gsl_sinterp_set_triangulation: out of memory", GSL_ENOMEM); }
  memcpy(t, triangles, w * n_triangles * sizeof(int));
  if (nb) memcpy(nb, neighbours, w * n_triangles * sizeof(int));
  free(st->tri); free(st->nbr);
  st->tri = t; st->nbr = nb; st->n_tri = n_triangles;
  return GSL_SUCCESS;
}

/* ---- modified Shepard: settings, statistics, nodal gradients ---- */
int gsl_sinterp_set_shepard(gsl_sinterp *interp, size_t nq, size_t nw)
{
  if (!interp) GSL_ERROR("gsl_sinterp_set_shepard: null interpolant", GSL_EFAULT);
  shepard_state *st = shepard_of(interp);
  if (!st) GSL_ERROR("gsl_sinterp_set_shepard: modified Shepard interpolants only", GSL_EINVAL);
  if (nq != 0 && (nq < st->nc || nq > GSL_SINTERP_MAX_NEIGHBOURS - 2))
    GSL_ERROR("gsl_sinterp_set_shepard: nq must be 0 (default) or between the number of monomials (5 in 2-D, 9 in 3-D) and 62", GSL_EINVAL);
  if (nw > GSL_SINTERP_MAX_NEIGHBOURS - 2) GSL_ERROR("gsl_sinterp_set_shepard: nw must be 0 (default) or between 1 and 62", GSL_EINVAL);
  st->nq_set = nq; st->nw_set = nw;
  return GSL_SUCCESS;
}

int gsl_sinterp_shepard_stats(const gsl_sinterp *interp, size_t *n_linear, size_t *n_constant, double *rw_max)
{
  if (!interp) GSL_ERROR("gsl_sinterp_shepard_stats: null interpolant", GSL_EFAULT);
  const shepard_state *st = shepard_of(interp);
  if (!st) GSL_ERROR("gsl_sinterp_shepard_stats: modified Shepard interpolants only", GSL_EINVAL);
  if (!st->ready) GSL_ERROR("gsl_sinterp_shepard_stats: interpolant not initialised", GSL_EINVAL);
  if (n_linear) *n_linear = st->n_linear;
  if (n_constant) *n_constant = st->n_constant;
  if (rw_max) *rw_max = st->rw_max;
  return GSL_SUCCESS;
}

gsl_sinterp_hip_ctx *gsl_sinterp_shepard_ctx(const gsl_sinterp *interp)
{
  const shepard_state *st = interp ? shepard_of(interp) : NULL;
  return st ? st->ctx : NULL;
}

/* the nodal gradients grad Q_i(x_i) = (linear coefficients) / Rq_i, read back from the model */
static int shepard_get_gradients(const shepard_state *st, gsl_matrix *gradients, size_t *iterations, double *residual)
{
  if (!st->ready) GSL_ERROR("gsl_sinterp_get_gradients: interpolant not initialised", GSL_EINVAL);
  if (gradients && (gradients->size1 != st->n || gradients->size2 != st->dim))
    GSL_ERROR("gsl_sinterp_get_gradients: gradients must be size x dim", GSL_EBADLEN);
  if (gradients) {
    const size_t n = st->n, nc = st->nc;
    double *h = (double *)malloc(n * (nc + 2) * sizeof(double));      /* [Rq | Rw | c], contiguous in the model */
    if (!h) GSL_ERROR("gsl_sinterp_get_gradients: out of memory", GSL_ENOMEM);
    int s = gsl_sinterp_hip_d2h(st->ctx, h, shep_rq(st), n * (nc + 2) * sizeof(double));
    if (!s)
      for (size_t i = 0; i < n; i++)
        for (size_t a = 0; a < st->dim; a++) gradients->data[i * gradients->tda + a] = h[2 * n + i * nc + a] * (1.0 / h[i]);
    free(h);
    HIP_TRY(s, st->ctx);
  }
  if (iterations) *iterations = 0;
  if (residual) *residual = 0.0;
  return GSL_SUCCESS;
}

/* ---- the gradients of the Clough-Tocher types ---- */
int gsl_sinterp_set_gradients(gsl_sinterp *interp, const gsl_matrix *gradients)
{
  if (!interp) GSL_ERROR("gsl_sinterp_set_gradients: null interpolant", GSL_EFAULT);
  if (!mesh_method(interp, MESH_CUBIC)) GSL_ERROR("gsl_sinterp_set_gradients: Clough-Tocher interpolants only", GSL_EINVAL);
  mesh_state *st = mesh_of(interp);
  if (gradients && (gradients->size1 != st->n || gradients->size2 != 2))
    GSL_ERROR("gsl_sinterp_set_gradients: gradients must be size x 2", GSL_EBADLEN);
  gsl_matrix *copy = NULL;
  if (gradients) {
    copy = gsl_matrix_alloc(st->n, 2);
    if (!copy) GSL_ERROR("gsl_sinterp_set_gradients: out of memory", GSL_ENOMEM);
    for (size_t i = 0; i < st->n; i++)
      for (size_t j = 0; j < 2; j++) gsl_matrix_set(copy, i, j, gradients->data[i * gradients->tda + j]);
  }
  if (st->g_set) gsl_matrix_free(st->g_set);
  st->g_set = copy;
  return GSL_SUCCESS;
}

int gsl_sinterp_set_gradient_options(gsl_sinterp *interp, double rtol, size_t maxiter)
{
  if (!interp) GSL_ERROR("gsl_sinterp_set_gradient_options: null interpolant", GSL_EFAULT);
  if (!mesh_method(interp, MESH_CUBIC)) GSL_ERROR("gsl_sinterp_set_gradient_options: Clough-Tocher interpolants only", GSL_EINVAL);
  if (!(rtol > 0.0 && rtol < 1.0) || maxiter < 1 || maxiter > (size_t)INT_MAX)
    GSL_ERROR("gsl_sinterp_set_gradient_options: need 0 < rtol < 1 and maxiter >= 1", GSL_EINVAL);
  mesh_state *st = mesh_of(interp);
  st->g_rtol = rtol; st->g_maxiter = maxiter;
  return GSL_SUCCESS;
}

int gsl_sinterp_get_gradients(const gsl_sinterp *interp, gsl_matrix *gradients, size_t *iterations, double *residual)
{
  if (!interp) GSL_ERROR("gsl_sinterp_get_gradients: null interpolant", GSL_EFAULT);
  if (shepard_of(interp)) return shepard_get_gradients(shepard_of(interp), gradients, iterations, residual);
  if (!mesh_method(interp, MESH_CUBIC)) GSL_ERROR("gsl_sinterp_get_gradients: Clough-Tocher interpolants only", GSL_EINVAL);
  const mesh_state *st = mesh_of(interp);
  if (!st->dev || !st->g) GSL_ERROR("gsl_sinterp_get_gradients: interpolant not initialised", GSL_EINVAL);
  if (gradients && (gradients->size1 != st->n || gradients->size2 != 2))
    GSL_ERROR("gsl_sinterp_get_gradients: gradients must be size x 2", GSL_EBADLEN);
  if (gradients)
    for (size_t i = 0; i < st->n; i++)
      for (size_t j = 0; j < 2; j++) gradients->data[i * gradients->tda + j] = gsl_matrix_get(st->g, i, j);
  if (iterations) *iterations = st->g_iters;
  if (residual) *residual = st->g_resid;
  return GSL_SUCCESS;
}

int gsl_sinterp_set_tree_options(gsl_sinterp *interp, int init_flags, gsl_rng *rng)
{
  if (!interp) GSL_ERROR("gsl_sinterp_set_tree_options: null interpolant", GSL_EFAULT);
  interp->init_flags = init_flags; interp->rng = rng;
  return GSL_SUCCESS;
}

int gsl_sinterp_init(gsl_sinterp *interp, const gsl_matrix *x, const gsl_vector *f)
{
  if (!interp || !x || !f) GSL_ERROR("gsl_sinterp_init: null argument", GSL_EFAULT);
  if (x->size1 != interp->size || f->size != interp->size)
    GSL_ERROR("data must match size of interpolation object", GSL_EINVAL);
  if (x->size2 != interp->dim)
    GSL_ERROR("centre matrix must have dim columns", GSL_EINVAL);
  return interp->type->init(interp, x, f);
}

const char *gsl_sinterp_name(const gsl_sinterp *interp) { return interp->type->name; }
unsigned int gsl_sinterp_min_size(const gsl_sinterp *interp) { return interp->type->min_size; }

int gsl_sinterp_eval_many(const gsl_sinterp *interp, const gsl_matrix *y, gsl_vector *s, int *leaf)
{
  if (!interp || !y || !s) GSL_ERROR("gsl_sinterp_eval_many: null argument", GSL_EFAULT);
  if (y->size2 != interp->dim) GSL_ERROR("target matrix must have dim columns", GSL_EBADLEN);
  if (s->size != y->size1) GSL_ERROR("output length must equal the number of targets", GSL_EBADLEN);
  return interp->type->eval_many(interp, y, s, leaf);
}

int gsl_sinterp_eval_resident(const gsl_sinterp *interp, const double *d_y, size_t m, size_t ytda,
                              double *d_s, int *d_leaf)
{
  if (!interp) GSL_ERROR("gsl_sinterp_eval_resident: null interpolant", GSL_EFAULT);
  return interp->type->eval_resident(interp, d_y, m, ytda, d_s, d_leaf);
}

int gsl_sinterp_eval_e(const gsl_sinterp *interp, const gsl_vector *y, double *s)
{
  if (!interp || !y || !s) GSL_ERROR("gsl_sinterp_eval_e: null argument", GSL_EFAULT);
  if (y->size != interp->dim) { *s = GSL_NAN; GSL_ERROR("target must have dim components", GSL_EBADLEN); }
  double yy[3], out = GSL_NAN;
  for (size_t c = 0; c < interp->dim; c++) yy[c] = gsl_vector_get(y, c);
  gsl_matrix_view Y = gsl_matrix_view_array(yy, 1, interp->dim);
  gsl_vector_view S = gsl_vector_view_array(&out, 1);
  /* like gsl_interp_eval_e: report EDOM by status + NaN, never through the handler */
  gsl_error_handler_t *saved = gsl_set_error_handler_off();
  int st = interp->type->eval_many(interp, &Y.matrix, &S.vector, NULL);
  gsl_set_error_handler(saved);
  *s = (st == GSL_SUCCESS) ? out : GSL_NAN;
  if (st != GSL_SUCCESS && st != GSL_EDOM) GSL_ERROR("gsl_sinterp_eval_e: evaluation failed", st);
  return st;
}

double gsl_sinterp_eval(const gsl_sinterp *interp, const gsl_vector *y)
{
  double s;
  int st = gsl_sinterp_eval_e(interp, y, &s);
  if (st != GSL_SUCCESS) GSL_ERROR_VAL("interpolation error", st, GSL_NAN);
  return s;
}

int gsl_sinterp_get_weights(const gsl_sinterp *interp, gsl_vector *w)
{
  if (!interp || !w) GSL_ERROR("gsl_sinterp_get_weights: null argument", GSL_EFAULT);
  const rbf_state *st = rbf_of(interp);
  if (!st) GSL_ERROR("gsl_sinterp_get_weights: not an RBF interpolant", GSL_EINVAL);
  if (is_local(interp)) GSL_ERROR("gsl_sinterp_get_weights: not with gsl_sinterp_set_neighbours (no global weight vector exists)", GSL_EUNSUP);
  if (!st->d_w || st->nf == 0) GSL_ERROR("gsl_sinterp_get_weights: interpolant not initialised", GSL_EINVAL);
  if (w->size != st->n) GSL_ERROR("gsl_sinterp_get_weights: wrong length", GSL_EBADLEN);
  double *h = (double *)malloc(st->n * sizeof(double));
  if (!h) GSL_ERROR("gsl_sinterp_get_weights: out of memory", GSL_ENOMEM);
  int s = gsl_sinterp_hip_d2h(st->ctx, h, st->d_w, st->n * sizeof(double));
  if (!s) for (size_t i = 0; i < st->n; i++) gsl_vector_set(w, i, h[i]);
  free(h);
  HIP_TRY(s, st->ctx);
  return GSL_SUCCESS;
}

void gsl_sinterp_free(gsl_sinterp *interp)
{
  if (!interp) return;
  if (interp->type->free) interp->type->free(interp->state);
  free(interp);
}

/* ======================================================================== */
/* gridded front-end (interpolation/scattered_interp_example.c:175-217)      */
/* ======================================================================== */
static gsl_sinterp_hip_ctx *interp_ctx0(const gsl_sinterp *interp)
{
  const simplex_state *ts = tree_of(interp);
  const mesh_state *ms = mesh_of(interp);
  if (ts) return ts->dev ? ts->dev->ctx : NULL;
  if (ms) return ms->dev ? ms->dev->ctx : NULL;
  if (shepard_of(interp)) return shepard_of(interp)->ready ? shepard_of(interp)->ctx : NULL;
  return rbf_of(interp)->ctx;
}

int gsl_sinterp_eval_grid(const gsl_sinterp *interp, const gsl_vector *min, const gsl_vector *max, gsl_matrix *grid)
{
  if (!interp || !min || !max || !grid) GSL_ERROR("gsl_sinterp_eval_grid: null argument", GSL_EFAULT);
  if (interp->dim != 2) GSL_ERROR("gsl_sinterp_eval_grid: 2-D interpolants only", GSL_EINVAL);
  if (min->size != 2 || max->size != 2) GSL_ERROR("gsl_sinterp_eval_grid: min / max must have 2 components", GSL_EBADLEN);
  gsl_sinterp_hip_ctx *c = interp_ctx0(interp);
  if (!c) GSL_ERROR("gsl_sinterp_eval_grid: interpolant not initialised", GSL_EINVAL);
  const size_t n0 = grid->size1, n1 = grid->size2, m = n0 * n1;
  if (m == 0) return GSL_SUCCESS;
  /* scattered_interp_example.c:179-183: step = range / n_grid */
  const double min0 = gsl_vector_get(min, 0), min1 = gsl_vector_get(min, 1);
  const double xrange = (gsl_vector_get(max, 0) - min0), xstep = xrange / (double)n0;
  const double yrange = (gsl_vector_get(max, 1) - min1), ystep = yrange / (double)n1;
  double *d_y = NULL, *d_s = NULL, *h_s = (double *)malloc(m * sizeof(double));
  if (!h_s) GSL_ERROR("gsl_sinterp_eval_grid: out of memory", GSL_ENOMEM);
  int st = gsl_sinterp_hip_malloc(c, (void **)&d_y, m * 2 * sizeof(double));
  if (!st) st = gsl_sinterp_hip_malloc(c, (void **)&d_s, m * sizeof(double));
  if (!st) st = gsl_sinterp_hip_grid_targets(c, min0, xstep, n0, min1, ystep, n1, d_y);
  int est = GSL_SUCCESS;
  if (!st) {
    gsl_error_handler_t *saved = gsl_set_error_handler_off();       /* EDOM (node outside the cage) is reported below */
    est = interp->type->eval_resident(interp, d_y, m, 2, d_s, NULL);
    gsl_set_error_handler(saved);
    if (est != GSL_SUCCESS && est != GSL_EDOM) st = est;
  }
  if (!st) st = gsl_sinterp_hip_d2h(c, h_s, d_s, m * sizeof(double));
  size_t n_nan = 0;
  if (!st)
    for (size_t i = 0; i < n0; i++)
      for (size_t j = 0; j < n1; j++) { const double v = h_s[i * n1 + j]; n_nan += v != v; gsl_matrix_set(grid, i, j, v); }
  gsl_sinterp_hip_free(c, d_y); gsl_sinterp_hip_free(c, d_s);
  free(h_s);
  HIP_TRY(st, c);
  if (tree_of(interp) && n_nan) GSL_ERROR("gsl_sinterp_eval_grid: grid node(s) outside the caging simplex", GSL_EDOM);
  if (mesh_of(interp) && n_nan) GSL_ERROR("gsl_sinterp_eval_grid: grid node(s) outside the triangulation", GSL_EDOM);
  if (shepard_of(interp) && n_nan) GSL_ERROR("gsl_sinterp_eval_grid: grid node(s) outside every node's radius of influence", GSL_EDOM);
  return GSL_SUCCESS;
}

int gsl_sinterp_fprintf_grid(FILE *stream, const gsl_vector *min, const gsl_vector *max, const gsl_matrix *grid)
{
  if (!stream || !min || !max || !grid) GSL_ERROR("gsl_sinterp_fprintf_grid: null argument", GSL_EFAULT);
  if (min->size != 2 || max->size != 2) GSL_ERROR("gsl_sinterp_fprintf_grid: min / max must have 2 components", GSL_EBADLEN);
  const size_t n0 = grid->size1, n1 = grid->size2;
  const double min0 = gsl_vector_get(min, 0), min1 = gsl_vector_get(min, 1);
  const double xstep = (gsl_vector_get(max, 0) - min0) / (double)n0, ystep = (gsl_vector_get(max, 1) - min1) / (double)n1;
  for (size_t i = 0; i < n0; i++) {                                  /* scattered_interp_example.c:203-215 */
    for (size_t j = 0; j < n1; j++)
      if (fprintf(stream, "%g %g %g\n", min0 + xstep * (double)i, min1 + ystep * (double)j, gsl_matrix_get(grid, i, j)) < 0)
        GSL_ERROR("fprintf failed", GSL_EFAILED);
    if (fprintf(stream, "\n") < 0) GSL_ERROR("fprintf failed", GSL_EFAILED);
  }
  return GSL_SUCCESS;
}

/* ======================================================================== */
/* binary checkpoint of an initialised interpolant                           */
/*   magic "GSLSINT1" | type id | dim | size | eps | init_flags | payload    */
/*   RBF payload: centres (size x dim) | weights (size)                      */
/*   linear simplex payload: tree (simplex_tree_fwrite) | centres | response */
/* ======================================================================== */
static const char INTERP_MAGIC[8] = {'G', 'S', 'L', 'S', 'I', 'N', 'T', '1'};

/* 1 when the whole header went out */
/* the header id under which a kriging interpolant WITH a drift is written: 17 / 18 / 19 for the types 4 / 10 / 11 */
static uint64_t drift_type_id(const type_desc *d) { return d->id == 4 ? 17 : d->id == 10 ? 18 : 19; }

static int header_fwrite(FILE *stream, const gsl_sinterp *interp, double eps, int64_t flags)
{
  const rbf_state *rst = rbf_of(interp);
  const uint64_t id = rst && rst->drift ? drift_type_id(desc_of(interp->type)) : (uint64_t)desc_of(interp->type)->id;
  const uint64_t head[3] = {id, (uint64_t)interp->dim, (uint64_t)interp->size};
  return fwrite(INTERP_MAGIC, 1, 8, stream) == 8 && fwrite(head, sizeof head[0], 3, stream) == 3 &&
         fwrite(&eps, sizeof eps, 1, stream) == 1 && fwrite(&flags, sizeof flags, 1, stream) == 1;
}

int gsl_sinterp_fwrite(FILE *stream, const gsl_sinterp *interp)
{
  if (!stream || !interp) GSL_ERROR("gsl_sinterp_fwrite: null argument", GSL_EFAULT);
  if (is_local(interp)) GSL_ERROR("gsl_sinterp_fwrite: not with gsl_sinterp_set_neighbours (checkpoints hold a solved global model)", GSL_EUNSUP);
  if (tree_of(interp)) {
    const simplex_state *st = tree_of(interp);
    if (!st->dev || !st->tree || !st->x || !st->f) GSL_ERROR("gsl_sinterp_fwrite: interpolant not initialised", GSL_EINVAL);
    if (st->nf > 1) GSL_ERROR("gsl_sinterp_fwrite: the GSLSINT1 format holds one response (interpolant with several fields)", GSL_EUNSUP);
    if (!header_fwrite(stream, interp, 0.0, interp->init_flags)) GSL_ERROR("fwrite failed", GSL_EFAILED);
    int s = simplex_tree_fwrite(stream, st->tree);
    if (s) return s;
    for (size_t i = 0; i < st->n; i++) {
      const double row[3] = {gsl_matrix_get(st->x, i, 0), gsl_matrix_get(st->x, i, 1), gsl_vector_get(st->f, i)};
      if (fwrite(row, sizeof(double), 3, stream) != 3) GSL_ERROR("fwrite failed", GSL_EFAILED);
    }
    return GSL_SUCCESS;
  }
  if (mesh_of(interp)) {
    const mesh_state *st = mesh_of(interp);
    if (!st->dev || !st->mesh || !st->x || !st->f) GSL_ERROR("gsl_sinterp_fwrite: interpolant not initialised", GSL_EINVAL);
    if (st->nf > 1) GSL_ERROR("gsl_sinterp_fwrite: the GSLSINT1 format holds one response (interpolant with several fields)", GSL_EUNSUP);
    if (!header_fwrite(stream, interp, 0.0, 0)) GSL_ERROR("fwrite failed", GSL_EFAILED);
    int s = simplex_mesh_fwrite(stream, st->mesh);
    if (s) return s;
    for (size_t i = 0; i < st->n; i++) {
      const double fi = gsl_vector_get(st->f, i);
      if (fwrite(&fi, sizeof fi, 1, stream) != 1) GSL_ERROR("fwrite failed", GSL_EFAILED);
    }
    if (mesh_method(interp, MESH_CUBIC)) {
      if (!st->g) GSL_ERROR("gsl_sinterp_fwrite: interpolant not initialised", GSL_EINVAL);
      for (size_t i = 0; i < st->n; i++) {
        const double gi[2] = {gsl_matrix_get(st->g, i, 0), gsl_matrix_get(st->g, i, 1)};
        if (fwrite(gi, sizeof(double), 2, stream) != 2) GSL_ERROR("fwrite failed", GSL_EFAILED);
      }
    }
    return GSL_SUCCESS;
  }
  if (shepard_of(interp)) {
    /* payload: nq | nw | linear fallbacks | constant fallbacks (uint64 each) | the model buffer [x | f | Rq | Rw | c] */
    const shepard_state *st = shepard_of(interp);
    if (!st->ready) GSL_ERROR("gsl_sinterp_fwrite: interpolant not initialised", GSL_EINVAL);
    const size_t cnt = shep_model_doubles(st);
    const uint64_t par[4] = {(uint64_t)st->nq, (uint64_t)st->nw, (uint64_t)st->n_linear, (uint64_t)st->n_constant};
    double *h = (double *)malloc(cnt * sizeof(double));
    if (!h) GSL_ERROR("gsl_sinterp_fwrite: out of memory", GSL_ENOMEM);
    int s = gsl_sinterp_hip_d2h(st->ctx, h, st->d_model, cnt * sizeof(double));
    if (!s && (!header_fwrite(stream, interp, 0.0, 0) || fwrite(par, sizeof par[0], 4, stream) != 4 || fwrite(h, sizeof(double), cnt, stream) != cnt)) {
      free(h);
      GSL_ERROR("fwrite failed", GSL_EFAILED);
    }
    free(h);
    HIP_TRY(s, st->ctx);
    return GSL_SUCCESS;
  }
  const rbf_state *st = rbf_of(interp);
  if (!st->d_w || st->nf == 0) GSL_ERROR("gsl_sinterp_fwrite: interpolant not initialised", GSL_EINVAL);
  if (st->nf > 1) GSL_ERROR("gsl_sinterp_fwrite: the GSLSINT1 format holds one weight vector (interpolant with several fields)", GSL_EUNSUP);
  const size_t cnt = st->n * (st->dim + 1);
  double *h = (double *)malloc(cnt * sizeof(double));
  if (!h) GSL_ERROR("gsl_sinterp_fwrite: out of memory", GSL_ENOMEM);
  int s = gsl_sinterp_hip_d2h(st->ctx, h, st->d_x, cnt * sizeof(double));      /* the model buffer: [centres | weights] */
  int64_t flags = 0;
  if (st->krige && !st->drift) memcpy(&flags, &st->mean, sizeof flags);         /* ordinary kriging: the word carries the mean's bits */
  if (!s && (!header_fwrite(stream, interp, st->eps, flags) || fwrite(h, sizeof(double), cnt, stream) != cnt ||
             (st->affine && fwrite(st->poly, sizeof(double), 4, stream) != 4))) {      /* affine tail: c_0 .. c_3 behind the weights */
    free(h);
    GSL_ERROR("fwrite failed", GSL_EFAILED);
  }
  if (!s && st->drift) {                                /* drift: order | shift | scale | the q coefficients behind the weights */
    const uint64_t order = (uint64_t)st->drift;
    if (fwrite(&order, sizeof order, 1, stream) != 1 || fwrite(st->drift_shift, sizeof(double), st->dim, stream) != st->dim ||
        fwrite(st->drift_scale, sizeof(double), st->dim, stream) != st->dim ||
        fwrite(st->f_coef[0], sizeof(double), st->drift_q, stream) != st->drift_q) {
      free(h);
      GSL_ERROR("fwrite failed", GSL_EFAILED);
    }
  }
  free(h);
  HIP_TRY(s, st->ctx);
  return GSL_SUCCESS;
}

int gsl_sinterp_fread(FILE *stream, gsl_sinterp *interp)
{
  if (!stream || !interp) GSL_ERROR("gsl_sinterp_fread: null argument", GSL_EFAULT);
  if (desc_of(interp->type)->krige && interp->neighbours > 0)
    GSL_ERROR("gsl_sinterp_fread: not with gsl_sinterp_set_neighbours (checkpoints hold a solved global model)", GSL_EUNSUP);
  char magic[8];
  uint64_t head[3];
  double eps;
  int64_t flags;
  if (fread(magic, 1, 8, stream) != 8 || memcmp(magic, INTERP_MAGIC, 8) != 0)
    GSL_ERROR("gsl_sinterp_fread: not a gsl_sinterp checkpoint", GSL_EFAILED);
  if (fread(head, sizeof head[0], 3, stream) != 3 || fread(&eps, sizeof eps, 1, stream) != 1 ||
      fread(&flags, sizeof flags, 1, stream) != 1)
    GSL_ERROR("fread failed", GSL_EFAILED);
  /* a kriging interpolant accepts its plain id and its drift id: the file decides the drift */
  const int drift_file = desc_of(interp->type)->krige && head[0] == drift_type_id(desc_of(interp->type));
  if ((head[0] != (uint64_t)desc_of(interp->type)->id && !drift_file) || head[1] != interp->dim || head[2] != interp->size)
    GSL_ERROR("gsl_sinterp_fread: checkpoint does not match the type / dim / size of the interpolant", GSL_EBADLEN);
  if (tree_of(interp)) {
    simplex_state *st = tree_of(interp);
    simplex_tree *tree = simplex_tree_fread(stream);
    if (!tree) return GSL_EFAILED;
    if ((size_t)tree->n_points != st->n) { simplex_tree_free(tree); GSL_ERROR("gsl_sinterp_fread: tree / size mismatch", GSL_EBADLEN); }
    gsl_matrix *x = gsl_matrix_alloc(st->n, 2);
    gsl_vector *f = gsl_vector_alloc(st->n);
    int ok = x && f;
    for (size_t i = 0; ok && i < st->n; i++) {
      double row[3];
      ok = fread(row, sizeof(double), 3, stream) == 3;
      if (ok) { gsl_matrix_set(x, i, 0, row[0]); gsl_matrix_set(x, i, 1, row[1]); gsl_vector_set(f, i, row[2]); }
    }
    if (!ok) { simplex_tree_free(tree); gsl_matrix_free(x); gsl_vector_free(f); GSL_ERROR("fread failed", GSL_EFAILED); }
    simplex_tree_device_free(st->dev); st->dev = NULL;
    simplex_tree_free(st->tree); gsl_matrix_free(st->x); gsl_vector_free(st->f);
    st->tree = tree; st->x = x; st->f = f;
    interp->init_flags = (int)flags;
    return simplex_mirror(interp, st);                  /* upload + pack + bind: no triangulation */
  }
  if (mesh_of(interp)) {
    mesh_state *st = mesh_of(interp);
    simplex_mesh *mesh = simplex_mesh_fread(stream);
    if (!mesh) return GSL_EFAILED;
    if (simplex_mesh_n_points(mesh) != st->n || simplex_mesh_dim(mesh) != st->dim) {
      simplex_mesh_free(mesh);
      GSL_ERROR("gsl_sinterp_fread: mesh / size mismatch", GSL_EBADLEN);
    }
    gsl_matrix *x = gsl_matrix_alloc(st->n, st->dim);
    gsl_vector *f = gsl_vector_alloc(st->n);
    int ok = x && f;
    for (size_t i = 0; ok && i < st->n; i++) {
      double fi;
      ok = fread(&fi, sizeof fi, 1, stream) == 1;
      if (ok) {
        gsl_vector_set(f, i, fi);
        for (size_t j = 0; j < st->dim; j++) gsl_matrix_set(x, i, j, simplex_mesh_points(mesh)[st->dim * i + j]);
      }
    }
    gsl_matrix *g = NULL;                                /* Clough-Tocher: the gradients follow the response */
    if (ok && mesh_method(interp, MESH_CUBIC)) {
      g = gsl_matrix_alloc(st->n, 2);
      ok = g != NULL;
      for (size_t i = 0; ok && i < st->n; i++) ok = fread(g->data + i * g->tda, sizeof(double), 2, stream) == 2;
    }
    if (!ok) {
      simplex_mesh_free(mesh); gsl_matrix_free(x); gsl_vector_free(f);
      if (g) gsl_matrix_free(g);
      GSL_ERROR("fread failed", GSL_EFAILED);
    }
    simplex_mesh_device_free(st->dev); st->dev = NULL;
    simplex_mesh_free(st->mesh); gsl_matrix_free(st->x); gsl_vector_free(st->f);
    st->mesh = mesh; st->x = x; st->f = f;
    /* upload + pack + bind: nothing is re-imported; the stored gradients are bound: nothing is estimated again */
    const int s = mesh_type_mirror(interp, st, g);
    if (g) gsl_matrix_free(g);
    return s;
  }
  if (shepard_of(interp)) {
    shepard_state *st = shepard_of(interp);
    const size_t cnt = shep_model_doubles(st), n = st->n;
    uint64_t par[4];
    double *h = (double *)malloc(cnt * sizeof(double));
    if (!h) GSL_ERROR("gsl_sinterp_fread: out of memory", GSL_ENOMEM);
    if (fread(par, sizeof par[0], 4, stream) != 4 || fread(h, sizeof(double), cnt, stream) != cnt) { free(h); GSL_ERROR("fread failed", GSL_EFAILED); }
    if (par[0] < st->nc || par[0] > GSL_SINTERP_MAX_NEIGHBOURS - 2 || par[1] < 1 || par[1] > GSL_SINTERP_MAX_NEIGHBOURS - 2) {
      free(h);
      GSL_ERROR("gsl_sinterp_fread: corrupt modified Shepard checkpoint", GSL_EFAILED);
    }
    int s = shepard_prepare(interp, st);
    if (s) { free(h); return s; }
    s = gsl_sinterp_hip_h2d(st->ctx, st->d_model, h, cnt * sizeof(double));
    if (!s) s = gsl_sinterp_hip_sync(st->ctx);
    double big = 0.0;
    const double *h_rw = h + n * (st->dim + 2);
    for (size_t i = 0; i < n; i++) if (h_rw[i] > big) big = h_rw[i];
    free(h);
    HIP_TRY(s, st->ctx);
    st->nq = (size_t)par[0]; st->nw = (size_t)par[1]; st->n_linear = (size_t)par[2]; st->n_constant = (size_t)par[3]; st->rw_max = big;
    st->ready = 1;
    return GSL_SUCCESS;                                 /* nothing was searched or fitted */
  }
  rbf_state *st = rbf_of(interp);
  const size_t cnt = st->n * (st->dim + 1);
  double *h = (double *)malloc(cnt * sizeof(double));
  if (!h) GSL_ERROR("gsl_sinterp_fread: out of memory", GSL_ENOMEM);
  if (fread(h, sizeof(double), cnt, stream) != cnt) { free(h); GSL_ERROR("fread failed", GSL_EFAILED); }
  double poly[4] = {0.0, 0.0, 0.0, 0.0};
  if (st->affine && fread(poly, sizeof(double), 4, stream) != 4) { free(h); GSL_ERROR("fread failed", GSL_EFAILED); }
  uint64_t order = 0;
  double dshift[3] = {0.0, 0.0, 0.0}, dscale[3] = {1.0, 1.0, 1.0}, dcoef[GSL_SINTERP_DRIFT_MAX_TERMS];
  size_t dq = 0;
  if (drift_file) {
    int ok = fread(&order, sizeof order, 1, stream) == 1 && (order == 1 || order == 2);
    if (ok) dq = gsl_sinterp_drift_terms(st->dim, (int)order);
    ok = ok && fread(dshift, sizeof(double), st->dim, stream) == st->dim && fread(dscale, sizeof(double), st->dim, stream) == st->dim &&
         fread(dcoef, sizeof(double), dq, stream) == dq;
    if (!ok) { free(h); GSL_ERROR("gsl_sinterp_fread: short or corrupt drift block", GSL_EFAILED); }
  }
  rbf_release_variance(st);                             /* a factor kept by an earlier init belongs to another model */
  int s = rbf_prepare_devices(interp, st, 1);
  if (s) { free(h); return s; }
  st->nf = 1; st->local_k = 0;
  st->var_state = 3;                                    /* the checkpoint carries no factor */
  rbf_release_loo(st);
  st->loo_state = 3;                                    /* ... and no leave-one-out data */
  st->eps = eps;
  if (st->krige) memcpy(&st->mean, &flags, sizeof st->mean);
  if (st->krige) {                                      /* the file decides: a plain file switches a drift off, a drift file on */
    st->drift = (int)order; st->drift_q = dq; interp->drift = (int)order;
    memcpy(st->drift_shift, dshift, sizeof dshift); memcpy(st->drift_scale, dscale, sizeof dscale);
    memset(st->f_coef, 0, sizeof st->f_coef);
    memcpy(st->f_coef[0], dcoef, dq * sizeof(double));
    if (order) st->mean = 0.0;
  }
  if (st->affine) memcpy(st->poly, poly, sizeof poly);
  st->f_mean[0] = st->mean; memcpy(st->f_poly[0], st->poly, sizeof st->poly);
  st->model_id = next_model_id();
  s = gsl_sinterp_hip_h2d(st->ctx, st->d_x, h, cnt * sizeof(double));
  if (!s && st->ss.grp) s = gsl_sinterp_hip_group_broadcast(st->ss.grp, (void *const *)st->m_model, cnt * sizeof(double));
  if (!s) s = gsl_sinterp_hip_sync(st->ctx);
  if (st->ss.grp)
    for (int r = 1; r < st->ss.n; r++) { int s2 = gsl_sinterp_hip_sync(gsl_sinterp_hip_group_ctx(st->ss.grp, r)); if (!s) s = s2; }
  free(h);
  HIP_TRY(s, st->ctx);
  return GSL_SUCCESS;                                   /* nothing was filled, factorised or solved */
}
