"""-m gpu: local kriging (csrc/hip/local.hip) -- the exact k-nearest-neighbour search over the binned centres and ordinary
kriging on the k neighbours of every target, through the raw entries and the facade (gsl_sinterp_set_neighbours).

References, numpy fp64.  Neighbours: lexsort on (r2, row) per target, r2 the FMA chain the kernels use (emulated: math.fma
where the interpreter has it, else an error-free product and sum whose last rounding can differ in rare cases -- then r2 is
compared to 1 ulp instead of bit for bit).  The tests assert that the relative gap between the k-th and the (k+1)-th r2 is
> 1e-9 for every target they use and then demand EXACT index lists.  Values and variances: two independent routes -- a
Cholesky factor with three forward substitutions, and np.linalg.solve of the bordered (k + 1) system -- which must agree to
1e-11 before either is used; the project's tolerances apply: values 1e-10 max|f|, variances 1e-10 absolute."""
import math

import numpy as np
import pytest
import torch

from gpu_util import Canaried, bits, dev, ptr

pytestmark = pytest.mark.gpu
TOL = 1e-10
GAUSSIAN, MATERN32, MATERN52 = 0, 3, 4
SEED = 20261019
HAVE_FMA = hasattr(math, "fma")
_SPLIT = 134217729.0                                        # 2^27 + 1


def _two_prod(a):
    """a * a = p + e exactly (Dekker / Veltkamp)"""
    p = a * a
    t = _SPLIT * a
    hi = t - (t - a)
    lo = a - hi
    return p, ((hi * hi - p) + 2.0 * hi * lo) + lo * lo


def fma_r2(y, xs):
    """r2[t, q] of target y[t] against ITS candidate centres xs[t, q, :]: r2 = 0; d = y_c - x_c; r2 = fma(d, d, r2)"""
    y, xs = np.asarray(y, dtype=np.float64), np.asarray(xs, dtype=np.float64)
    r2 = np.zeros(xs.shape[:2])
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(y.shape[1]):
            d = y[:, None, c] - xs[:, :, c]
            if HAVE_FMA:
                r2 = np.vectorize(math.fma, otypes=[np.float64])(d, d, r2)
                continue
            p, e = _two_prod(d)
            s = p + r2
            bb = s - p
            err = (p - (s - bb)) + (r2 - bb)                # p + r2 = s + err exactly
            r2 = np.where(np.isfinite(s), s + (err + e), s)
    return r2


def ulps(a, b):
    ia, ib = bits(a).astype(np.int64), bits(b).astype(np.int64)
    return np.abs(ia - ib)


def ref_knn(y, x, k):
    """(idx m x k, r2 m x k, relative gap to the (k+1)-th r2 per target); a NaN target: idx -1, r2 NaN, gap inf.
    Plain numpy distances pick k + 9 candidates per target (plain and FMA distances differ in the last bits only), the FMA
    chain on those decides."""
    n = x.shape[0]
    bad = np.isnan(y).any(axis=1)
    yz = np.where(bad[:, None], 0.0, y)
    plain = np.zeros((len(y), n))
    for c in range(x.shape[1]):
        plain += (yz[:, None, c] - x[None, :, c]) ** 2
    q = min(k + 9, n)
    part = np.argpartition(plain, q - 1, axis=1)[:, :q] if q < n else np.tile(np.arange(n), (len(y), 1))
    del plain
    pr = fma_r2(yz, x[part])
    order = np.lexsort((part, pr), axis=-1)
    idx = np.take_along_axis(part, order, axis=1)
    rr = np.take_along_axis(pr, order, axis=1)
    gap = np.full(len(y), np.inf)
    if q > k:
        with np.errstate(invalid="ignore", divide="ignore"):
            gap = np.where(rr[:, k] > 0, (rr[:, k] - rr[:, k - 1]) / rr[:, k], np.inf)
    idx, rr = idx[:, :k].astype(np.int32), rr[:, :k].copy()
    idx[bad], rr[bad], gap[bad] = -1, np.nan, np.inf
    return idx, rr, gap


def phi(kind, eps, r2):
    r = np.sqrt(r2)
    if kind == GAUSSIAN:
        return np.exp(-(eps * eps) * r2)
    if kind == MATERN32:
        t = math.sqrt(3.0) * eps * r
        return (1.0 + t) * np.exp(-t)
    t = math.sqrt(5.0) * eps * r
    return (1.0 + t + t * t / 3.0) * np.exp(-t)


def ref_krige(kind, eps, nugget, x, f, y, idx):
    """(s, var) at the targets from their neighbour rows idx, by the two routes; asserts that the routes agree to 1e-11"""
    m, k = idx.shape
    xs, fs = x[idx], f[idx]                                                     # m x k x d, m x k
    K = phi(kind, eps, ((xs[:, :, None, :] - xs[:, None, :, :]) ** 2).sum(axis=3)) + nugget * np.eye(k)
    kv = phi(kind, eps, ((y[:, None, :] - xs) ** 2).sum(axis=2))                # m x k
    # route 1: Cholesky and three forward substitutions
    L = np.linalg.cholesky(K)
    rhs = np.stack([kv, np.ones((m, k)), fs], axis=2)
    sol = np.empty_like(rhs)
    for j in range(k):                                                          # forward substitution, batched over the targets
        sol[:, j, :] = (rhs[:, j, :] - np.einsum("tk,tkr->tr", L[:, j, :j], sol[:, :j, :])) / L[:, j, j][:, None]
    u, v, g = sol[:, :, 0], sol[:, :, 1], sol[:, :, 2]
    d = (v * v).sum(axis=1)
    mu = (v * g).sum(axis=1) / d
    s1 = mu + (u * (g - mu[:, None] * v)).sum(axis=1)
    v1 = 1.0 - (u * u).sum(axis=1) + (1.0 - (v * u).sum(axis=1)) ** 2 / d
    # route 2: the bordered system [K 1; 1^T 0] [w; lam] = [k; 1]
    A = np.zeros((m, k + 1, k + 1))
    A[:, :k, :k], A[:, :k, k], A[:, k, :k] = K, 1.0, 1.0
    b = np.concatenate([kv, np.ones((m, 1))], axis=1)
    wl = np.linalg.solve(A, b[:, :, None])[:, :, 0]
    s2 = (wl[:, :k] * fs).sum(axis=1)
    v2 = 1.0 - (wl[:, :k] * kv).sum(axis=1) - wl[:, k]
    fmax = np.abs(f).max()
    agree = max(np.abs(s1 - s2).max() / fmax, np.abs(v1 - v2).max())
    assert agree <= 1e-11, f"the two reference routes differ by {agree:.3e}"
    return s1, v1


def response(x):
    return 2.0 + np.sin(3.0 * x[:, 0]) + (np.cos(2.0 * x[:, 1]) if x.shape[1] > 1 else 0.0) + (0.5 * x[:, 2] if x.shape[1] > 2 else 0.0)


def default_eps(kind, n, dim):
    return (2.0 if kind == GAUSSIAN else 1.0) * n ** (1.0 / dim)


_clouds = {}


def cloud(n, dim):
    if (n, dim) not in _clouds:
        x = np.random.default_rng(SEED + 31 * dim + n).random((n, dim))
        f = response(x)
        x.setflags(write=False); f.setflags(write=False)
        _clouds[(n, dim)] = (x, f)
    return _clouds[(n, dim)]


def gpu_knn(ctx, x, y, k, want_r2=True, model_id=0):
    n, dim = x.shape
    m = y.shape[0]
    d_x, d_y = dev(x), dev(y)
    d_idx = torch.full((m, k), -7, dtype=torch.int32, device="cuda")
    d_r2 = torch.full((m, k), -7.0, dtype=torch.float64, device="cuda")
    st = ctx.knn(ptr(d_x), n, dim, dim, ptr(d_y), m, dim, k, ptr(d_idx), ptr(d_r2) if want_r2 else None, model_id)
    assert st == 0
    return d_idx.cpu().numpy(), d_r2.cpu().numpy()


def gpu_krige(ctx, kind, eps, nugget, x, f, y, k, model_id=0):
    n, dim = x.shape
    m = y.shape[0]
    d_x, d_f, d_y = dev(x), dev(f), dev(y)
    d_s = torch.full((m,), -7.0, dtype=torch.float64, device="cuda")
    d_v = torch.full((m,), -7.0, dtype=torch.float64, device="cuda")
    d_idx = torch.full((m, k), -7, dtype=torch.int32, device="cuda")
    st, failed = ctx.local_krige(kind, eps, nugget, ptr(d_x), n, dim, dim, ptr(d_f), ptr(d_y), m, dim, k, ptr(d_s), ptr(d_v), ptr(d_idx),
                                 model_id)
    return st, failed, d_s.cpu().numpy(), d_v.cpu().numpy(), d_idx.cpu().numpy()


def assert_r2(got, want):
    both_nan = np.isnan(got) & np.isnan(want)
    u = np.where(both_nan, 0, ulps(np.where(both_nan, 0.0, got), np.where(both_nan, 0.0, want)))
    print(f"r2: max ulp distance {u.max()} ({'math.fma' if HAVE_FMA else 'emulated FMA'})")
    assert u.max() <= (0 if HAVE_FMA else 1)


def knn_targets(x, k, m):
    """m targets: [0] inside, [1] a NaN row, then on centres, outside the box by 10 % and by 1e6 box widths, the rest inside
    the cloud.  Candidates whose k-th / (k+1)-th gap is not > 1e-9 are replaced by others -- the choice looks at the
    reference alone.  From 1e6 box widths away all centres are at nearly the same distance (the gap is about spacing /
    distance, ~1e-10 at N = 5000), so few candidates qualify there and in 1-D, where every far target on one side has the
    same list, there may be none: as many as qualify, up to 4, are used."""
    n, dim = x.shape
    rng = np.random.default_rng(SEED + 7 * n + dim + k)
    lo, hi = x.min(axis=0), x.max(axis=0)
    w = np.where(hi > lo, hi - lo, 1.0)

    def keep(c, need, at_least=None):
        _, _, gap = ref_knn(c, x, k)
        c = c[gap > 1e-9]
        assert len(c) >= (need if at_least is None else at_least), "not enough candidates with a clear k-th neighbour"
        return c[:need]

    def inside(q):
        return lo + w * rng.random((q, dim))

    def outside(q, by):                                              # one coordinate `by` box widths beyond the box
        p = inside(q)
        ax, up = rng.integers(dim, size=q), rng.random(q) < 0.5
        p[np.arange(q), ax] = np.where(up, hi[ax] + by * w[ax], lo[ax] - by * w[ax])
        return p

    def far(q):                                                      # 1e6 box widths away, towards a corner: there the
        side = rng.choice([-1.0, 1.0], size=(q, dim))                # projections of the nearest centres are furthest apart
        return (lo + hi) / 2 + side * w * 1e6 * (0.75 + 0.5 * rng.random((q, dim)))

    parts = [keep(inside(8), 1), np.full((1, dim), np.nan)]
    if m > 2:
        parts += [keep(x[rng.permutation(n)[:min(n, 40)]], min(n, 12)), keep(outside(64, 0.1), 12),
                  keep(far(3000), 4, at_least=0 if dim == 1 else 1)]
        rest = m - sum(len(p) for p in parts)
        parts.append(keep(inside(rest + 64), rest))
    return np.ascontiguousarray(np.vstack(parts)[:m])


# ---- 1. exactness of the search -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", (1, 2, 3))
@pytest.mark.parametrize("n,k", ((1, 1), (7, 7), (200, 5), (5000, 32), (5000, 64)))
def test_knn_is_exact(pkg, dim, n, k):
    x, _ = cloud(n, dim)
    y = knn_targets(x, k, 4133)
    want_idx, want_r2, gap = ref_knn(y, x, k)
    assert (gap > 1e-9).all()
    ctx = pkg.HipContext.on_torch_stream(0)
    for m in (1, 63, 65, 4133):                                      # both sides of the cell-order threshold (4096)
        idx, r2 = gpu_knn(ctx, x, y[:m], k)
        wrong = np.flatnonzero((idx != want_idx[:m]).any(axis=1))
        assert wrong.size == 0, f"m = {m}: {wrong.size} targets with another neighbour list, first {wrong[:5]}"
        assert (idx[1] == -1).all() if m > 1 else True               # the NaN row
        assert_r2(r2, want_r2[:m])
    ctx.close()


# ---- 2. ties ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (5, 6, 7, 8, 9))
def test_ties_go_to_the_smaller_index(pkg, k):
    g = np.arange(8.0)
    x = np.ascontiguousarray(np.stack(np.meshgrid(g, g, indexing="ij"), axis=2).reshape(-1, 2))
    x = x[np.random.default_rng(SEED).permutation(64)]               # rows in no geometric order
    y = np.ascontiguousarray(np.vstack([x, (x + 0.5)[(x < 7).all(axis=1)]]))      # lattice points and cell centres
    r2 = ((y[:, None, :] - x[None, :, :]) ** 2).sum(axis=2)          # small integers and quarters: exact
    want = np.lexsort((np.tile(np.arange(64), (len(y), 1)), r2), axis=-1)[:, :k].astype(np.int32)
    assert (np.sort(r2, axis=1)[:, k - 1] == np.sort(r2, axis=1)[:, k]).any()     # some lists are cut inside a tie
    ctx = pkg.HipContext.on_torch_stream(0)
    idx, got_r2 = gpu_knn(ctx, x, y, k)
    ctx.close()
    assert (idx == want).all()
    assert (got_r2 == np.take_along_axis(r2, want.astype(np.int64), axis=1)).all()


# ---- 3. degenerate clouds ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ("one_cell", "line"))
def test_degenerate_clouds(pkg, shape):
    rng = np.random.default_rng(SEED + 3)
    if shape == "one_cell":                                          # the outlier stretches the box: every other centre in one cell
        x = np.vstack([0.25 + 1e-3 * rng.random((4999, 2)), [[1000.25, 0.25]]])
        y = np.vstack([0.25 + 1e-3 * rng.random((120, 2)), [[500.0, 0.3]], [[1000.0, 0.2]]])
    else:                                                            # all centres on one line: the box has no width in y
        x = np.stack([rng.random(3000), np.full(3000, 0.75)], axis=1)
        y = np.vstack([np.stack([rng.random(60), np.full(60, 0.75)], axis=1), rng.random((60, 2))])
    x, y, k = np.ascontiguousarray(x), np.ascontiguousarray(y), 16
    want_idx, want_r2, gap = ref_knn(y, x, k)
    y, want_idx, want_r2 = y[gap > 1e-9], want_idx[gap > 1e-9], want_r2[gap > 1e-9]
    assert len(y) >= 100
    ctx = pkg.HipContext.on_torch_stream(0)
    idx, r2 = gpu_knn(ctx, x, y, k)
    ctx.close()
    assert (idx == want_idx).all()
    assert_r2(r2, want_r2)


# ---- 4. values and variances -------------------------------------------------------------------------------------------
_SHAPES = [(2, 200, 5), (3, 200, 5), (2, 5000, 32), (2, 5000, 64), (3, 5000, 32), (3, 5000, 64)]
_COV = [("kriging", GAUSSIAN, 0.0), ("kriging_matern32", MATERN32, 0.0), ("kriging_matern52", MATERN52, 1e-3)]
_M = 300


def value_case(kind, nugget, dim, n, k):
    x, f = cloud(n, dim)
    rng = np.random.default_rng(SEED + n + k + dim)
    y = np.ascontiguousarray(np.vstack([rng.random((_M - 10, dim)), -0.1 + 1.2 * rng.random((10, dim))]))
    idx, _, gap = ref_knn(y, x, k)
    assert (gap > 1e-9).all()
    eps = default_eps(kind, n, dim)
    s, v = ref_krige(kind, eps, nugget, x, f, y, idx.astype(np.int64))
    return x, f, y, eps, idx, s, v


# 1-D: Matern 5/2 with a nugget only (cond 8e3); the Gaussian reaches cond 5e9 at k = 64 there: no shape for a 1e-10 test
_VALUE_CASES = [c + s for c in _COV for s in _SHAPES] + [_COV[2] + s for s in ((1, 200, 5), (1, 5000, 32), (1, 5000, 64))]


@pytest.mark.parametrize("name,kind,nugget,dim,n,k", _VALUE_CASES)
def test_values_and_variances(pkg, name, kind, nugget, dim, n, k):
    x, f, y, eps, want_idx, want_s, want_v = value_case(kind, nugget, dim, n, k)
    fmax = np.abs(f).max()
    ctx = pkg.HipContext.on_torch_stream(0)
    st, failed, s, v, idx = gpu_krige(ctx, kind, eps, nugget, x, f, y, k)
    ctx.close()
    assert st == 0 and failed == 0
    assert (idx == want_idx).all()
    es, ev = np.abs(s - want_s).max() / fmax, np.abs(v - want_v).max()
    print(f"{name} dim {dim} n {n} k {k}: value err {es:.3e} max|f|, variance err {ev:.3e}, min var {v.min():.3e}")
    assert es <= TOL and ev <= TOL
    # the facade: three entries, one set of bits (the variance clamped at 0)
    si = pkg.Sinterp(name, dim, n, 0)
    assert si.set_nugget(nugget) == 0 and si.set_neighbours(k) == 0
    assert si.init(x, f) == 0 and si.route() == 11
    st1, s1, _ = si.eval_many(y)
    st2, v2 = si.eval_variance_many(y)                               # no set_variance: the local route keeps no factor
    st3, s3, v3, i3 = si.eval_local_many(y)
    assert (st1, st2, st3) == (0, 0, 0)
    assert (bits(s1) == bits(s)).all() and (bits(s3) == bits(s)).all()
    assert (bits(v2) == bits(np.maximum(v, 0.0))).all() and (bits(v3) == bits(v2)).all()
    assert (i3 == want_idx).all()
    st4, s4 = si.eval_e(y[0])
    st5, v5 = si.eval_variance_e(y[0])
    assert st4 == 0 and st5 == 0 and s4 == s[0] and v5 == max(v[0], 0.0)


# ---- 5. k = N: the local model is the global one ----------------------------------------------------------------------
def test_k_equal_n_is_the_global_model(pkg):
    n, dim, m = 48, 2, 500
    x, f = cloud(n, dim)
    y = np.ascontiguousarray(np.random.default_rng(SEED + 5).random((m, dim)) * 1.2 - 0.1)
    fmax = np.abs(f).max()
    for nugget in (1e-3, 0.0):
        g = pkg.Sinterp("kriging_matern52", dim, n, 0)
        assert g.set_nugget(nugget) == 0 and g.set_variance(1) == 0 and g.init(x, f) == 0 and g.route() == 7
        loc = pkg.Sinterp("kriging_matern52", dim, n, 0)
        assert loc.set_nugget(nugget) == 0 and loc.set_neighbours(n) == 0 and loc.init(x, f) == 0 and loc.route() == 11
        (_, gs, _), (_, gv) = g.eval_many(y), g.eval_variance_many(y)
        st, ls, lv, _ = loc.eval_local_many(y)
        assert st == 0
        es, ev = np.abs(ls - gs).max() / fmax, np.abs(lv - gv).max()
        print(f"nugget {nugget}: local vs global value {es:.3e} max|f|, variance {ev:.3e}")
        assert es <= TOL and ev <= TOL
        if nugget == 0.0:                                            # at the data sites: the data, and no uncertainty
            st, ss, sv, _ = loc.eval_local_many(x)
            assert st == 0 and np.abs(ss - f).max() <= TOL and (sv >= 0.0).all() and sv.max() <= TOL


# ---- 6. bits ----------------------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_the_batch(pkg):
    dim, n, k = 2, 5000, 32
    x, f = cloud(n, dim)
    y = np.ascontiguousarray(np.random.default_rng(SEED + 6).random((5000, dim)))
    eps = default_eps(MATERN52, n, dim)
    ctx, ctx2 = pkg.HipContext.on_torch_stream(0), pkg.HipContext.on_torch_stream(0)
    _, _, s5, v5, i5 = gpu_krige(ctx, MATERN52, eps, 1e-3, x, f, y, k)             # cell order (>= 4096 targets)
    _, _, s5b, v5b, i5b = gpu_krige(ctx, MATERN52, eps, 1e-3, x, f, y, k)
    _, _, s3, v3, i3 = gpu_krige(ctx, MATERN52, eps, 1e-3, x, f, y[:300], k)       # input order
    _, _, s1, v1, i1 = gpu_krige(ctx, MATERN52, eps, 1e-3, x, f, y[77:78], k)      # alone
    _, _, sc, vc, ic = gpu_krige(ctx2, MATERN52, eps, 1e-3, x, f, y, k)            # another context
    ctx.close(); ctx2.close()
    for s, v, i, sl in ((s5b, v5b, i5b, slice(None)), (s3, v3, i3, slice(0, 300)), (s1, v1, i1, slice(77, 78)), (sc, vc, ic, slice(None))):
        assert (bits(s) == bits(s5[sl])).all() and (bits(v) == bits(v5[sl])).all() and (i == i5[sl]).all()
    assert np.isfinite(s5).all() and np.isfinite(v5).all()


# ---- 7. layouts -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", (1, 2, 3))
def test_strided_layouts_and_canaries(pkg, dim):
    n, k, m = 700, 16, 130
    x, f = cloud(n, dim)
    y = np.ascontiguousarray(np.random.default_rng(SEED + 8 + dim).random((m, dim)))
    eps = default_eps(MATERN52, n, dim)
    ctx = pkg.HipContext.on_torch_stream(0)
    _, _, want_s, want_v, want_i = gpu_krige(ctx, MATERN52, eps, 1e-3, x, f, y, k)
    cx, cy, cf = Canaried(x, ld=dim + 3, off=1), Canaried(y, ld=dim + 2, off=1), Canaried(f, off=1)
    cs, cv = Canaried(np.zeros(m), off=1), Canaried(np.zeros(m), off=1)
    d_idx = torch.full((m * k + 64,), -7, dtype=torch.int32, device="cuda")
    st, failed = ctx.local_krige(MATERN52, eps, 1e-3, cx.ptr, n, dim, dim + 3, cf.ptr, cy.ptr, m, dim + 2, k, cs.ptr, cv.ptr,
                                 d_idx.data_ptr() + 4 * 32)
    assert st == 0 and failed == 0
    i = d_idx.cpu().numpy()
    assert (i[:32] == -7).all() and (i[32 + m * k:] == -7).all() and (i[32:32 + m * k].reshape(m, k) == want_i).all()
    assert (bits(cs.get()) == bits(want_s)).all() and (bits(cv.get()) == bits(want_v)).all()
    for c in (cx, cy, cf, cs, cv):
        assert c.padding_intact()
    cr = Canaried(np.zeros((m, k)), off=1)
    d_idx.fill_(-7)
    assert ctx.knn(cx.ptr, n, dim, dim + 3, cy.ptr, m, dim + 2, k, d_idx.data_ptr() + 4 * 32, cr.ptr) == 0
    i = d_idx.cpu().numpy()
    assert (i[:32] == -7).all() and (i[32 + m * k:] == -7).all() and (i[32:32 + m * k].reshape(m, k) == want_i).all()
    assert cr.padding_intact() and cx.padding_intact() and cy.padding_intact()
    ctx.close()


# ---- 8. failed pivots -------------------------------------------------------------------------------------------------
def test_failed_pivots_are_per_target(pkg):
    dim, n, k, m = 2, 2000, 16, 600
    x, f = cloud(n, dim)
    x, f = x.copy(), f.copy()
    x[1500] = x[3]                                                    # two coincident sites
    f[1500] = f[3]
    rng = np.random.default_rng(SEED + 9)
    y = np.ascontiguousarray(np.vstack([x[3] + 0.03 * (rng.random((200, dim)) - 0.5), rng.random((m - 200, dim))]))
    idx, _, gap = ref_knn(y, x, k)
    y, idx = np.ascontiguousarray(y[gap > 1e-9]), idx[gap > 1e-9]          # (the twins themselves as k-th and (k+1)-th: gap 0)
    m = len(y)
    both = (idx == 3).any(axis=1) & (idx == 1500).any(axis=1)
    assert 20 <= both.sum() <= m - 20
    eps = default_eps(MATERN52, n, dim)
    ctx = pkg.HipContext.on_torch_stream(0)
    st, failed, s, v, gi = gpu_krige(ctx, MATERN52, eps, 0.0, x, f, y, k)
    assert st == pkg.GSL_EDOM and failed == both.sum()
    assert (gi == idx).all()
    assert (np.isnan(s) == both).all() and (np.isnan(v) == both).all()
    want_s, want_v = ref_krige(MATERN52, eps, 0.0, x, f, y[~both], idx[~both].astype(np.int64))
    assert np.abs(s[~both] - want_s).max() / np.abs(f).max() <= TOL and np.abs(v[~both] - want_v).max() <= TOL
    st, failed, s, v, _ = gpu_krige(ctx, MATERN52, eps, 1e-6, x, f, y, k)        # a nugget separates them
    ctx.close()
    assert st == 0 and failed == 0 and np.isfinite(s).all() and np.isfinite(v).all()
    # the facade: GSL_EDOM, everything stored
    si = pkg.Sinterp("kriging_matern52", dim, n, 0)
    assert si.set_neighbours(k) == 0 and si.init(x, f) == 0
    st, fs, fv, _ = si.eval_local_many(y)
    assert st == pkg.GSL_EDOM and (np.isnan(fs) == both).all() and (np.isnan(fv) == both).all()
    st, one = si.eval_e(y[np.flatnonzero(both)[0]])
    assert st == pkg.GSL_EDOM and np.isnan(one)


# ---- 9. past dense N --------------------------------------------------------------------------------------------------
def test_past_dense_n(pkg):
    from scipy.spatial import cKDTree
    dim, n, k, m = 2, 200000, 16, 20000                              # a dense matrix would be 320 GB
    rng = np.random.default_rng(SEED + 10)
    x = np.ascontiguousarray(rng.random((n, dim)))
    f = response(x)
    y = np.ascontiguousarray(rng.random((m, dim)))
    eps = default_eps(MATERN52, n, dim)
    si = pkg.Sinterp("kriging_matern52", dim, n, 0)
    assert si.set_nugget(1e-3) == 0 and si.set_neighbours(k) == 0 and si.init(x, f) == 0 and si.route() == 11
    st, s, v, idx = si.eval_local_many(y)
    assert st == 0 and np.isfinite(s).all() and (v >= 0.0).all()
    st, s2, v2, idx2 = si.eval_local_many(y)
    assert st == 0 and (bits(s2) == bits(s)).all() and (bits(v2) == bits(v)).all() and (idx2 == idx).all()
    spot = rng.permutation(m)[:256]
    dist, nb = cKDTree(x).query(y[spot], k=k + 1)
    r2 = fma_r2(y[spot], x[nb])
    order = np.lexsort((nb, r2), axis=-1)
    nb, r2 = np.take_along_axis(nb, order, axis=1), np.take_along_axis(r2, order, axis=1)
    assert ((r2[:, k] - r2[:, k - 1]) / r2[:, k] > 1e-9).all()
    assert (idx[spot] == nb[:, :k]).all()
    want_s, want_v = ref_krige(MATERN52, eps, 1e-3, x, f, y[spot], nb[:, :k])
    assert np.abs(s[spot] - want_s).max() / np.abs(f).max() <= TOL and np.abs(v[spot] - np.maximum(want_v, 0.0)).max() <= TOL
    # the pack is cached per model: a raw context counts its packs
    ctx = pkg.HipContext.on_torch_stream(0)
    d_x, d_f, d_y = dev(x), dev(f), dev(y)
    d_s = torch.empty(m, dtype=torch.float64, device="cuda")
    for rep in range(3):
        st, failed = ctx.local_krige(MATERN52, eps, 1e-3, ptr(d_x), n, dim, dim, ptr(d_f), ptr(d_y), m, dim, k, ptr(d_s), None, None, 1234)
        assert st == 0 and ctx.local_pack_count() == 1
    assert (bits(d_s.cpu().numpy()) == bits(s)).all()
    st, failed = ctx.local_krige(MATERN52, eps, 1e-3, ptr(d_x), n, dim, dim, ptr(d_f), ptr(d_y), m, dim, k, ptr(d_s), None, None, 0)
    assert st == 0 and ctx.local_pack_count() == 2                   # model_id 0: nobody vouches for the model
    ctx.close()


# ---- 10. facade rules -------------------------------------------------------------------------------------------------
def test_facade_rules(pkg, tmp_path):
    dim, n, k = 2, 300, 12
    x, f = cloud(n, dim)
    y = np.ascontiguousarray(np.random.default_rng(SEED + 11).random((70, dim)))
    EUNSUP = pkg.capi.GSL_EUNSUP
    si = pkg.Sinterp("kriging_matern52", dim, n, 0)
    assert si.set_nugget(1e-3) == 0 and si.set_loo(1) == 0 and si.set_neighbours(k) == 0
    assert si.init(x, f) == 0 and si.route() == 11
    assert si.eval_grad_many(y)[0] == EUNSUP and si.eval_grad_e(y[0])[0] == EUNSUP
    assert si.init_fields(x, np.stack([f, f], axis=1)) == EUNSUP
    assert si.eval_fields_many(y)[0] == EUNSUP and si.eval_fields_e(y[0])[0] == EUNSUP
    assert si.field_weights(0)[0] == EUNSUP and si.field_mean(0)[0] == EUNSUP
    assert si.weights()[0] == EUNSUP and si.mean()[0] == EUNSUP
    assert si.fwrite(str(tmp_path / "local.bin")) == EUNSUP
    assert si.loo_residuals(out=np.zeros((n, 1)))[0] == EUNSUP and si.loo_variance()[0] == EUNSUP
    st, s, _ = si.eval_many(y)
    assert st == 0 and np.isfinite(s).all()
    # resident and gridded entries take the same route
    d_y = dev(y)
    d_s = torch.zeros(70, dtype=torch.float64, device="cuda")
    d_v = torch.zeros(70, dtype=torch.float64, device="cuda")
    assert si.eval_resident(ptr(d_y), 70, dim, ptr(d_s)) == 0 and si.eval_variance_resident(ptr(d_y), 70, dim, ptr(d_v)) == 0
    st, s3, v3, _ = si.eval_local_many(y)
    assert (bits(d_s.cpu().numpy()) == bits(s)).all() and (bits(s3) == bits(s)).all() and (bits(d_v.cpu().numpy()) == bits(v3)).all()
    st, grid = si.eval_grid([0.0, 0.0], [1.0, 1.0], 6, 5)
    gy = np.ascontiguousarray(np.stack(np.meshgrid((1.0 / 6) * np.arange(6), (1.0 / 5) * np.arange(5), indexing="ij"), axis=2).reshape(-1, 2))   # min + step * i
    assert st == 0 and (bits(grid.ravel()) == bits(si.eval_many(gy)[1])).all()
    # set_neighbours(0): init and every bit as on an interpolant that never heard of it
    plain = pkg.Sinterp("kriging_matern52", dim, n, 0)
    assert plain.set_nugget(1e-3) == 0 and plain.set_variance(1) == 0 and plain.init(x, f) == 0
    back = pkg.Sinterp("kriging_matern52", dim, n, 0)
    assert back.set_nugget(1e-3) == 0 and back.set_variance(1) == 0 and back.set_neighbours(k) == 0 and back.set_neighbours(0) == 0
    assert back.init(x, f) == 0 and back.route() == plain.route() == 7
    assert (bits(back.eval_many(y)[1]) == bits(plain.eval_many(y)[1])).all()
    assert (bits(back.eval_variance_many(y)[1]) == bits(plain.eval_variance_many(y)[1])).all()
    assert (bits(back.weights()[1]) == bits(plain.weights()[1])).all() and back.mean() == plain.mean()
    assert back.eval_local_many(y)[0] == pkg.GSL_EINVAL
    # the same interpolant re-initialised on the other route, both ways
    assert si.set_neighbours(0) == 0 and si.init(x, f) == 0 and si.route() == 7
    assert (bits(si.eval_many(y)[1]) == bits(plain.eval_many(y)[1])).all() and si.mean()[0] == 0
    assert si.set_neighbours(k) == 0 and si.init(x, f) == 0 and si.route() == 11
    assert (bits(si.eval_many(y)[1]) == bits(s)).all()
