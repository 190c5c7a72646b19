"""-m gpu: model selection -- the device-side reduction of a factor to the scalars of the criteria (csrc/hip/score.hip), the
scores of the fit workspace (negative concentrated log-likelihood, mean squared leave-one-out residual) and the 1-D
searches over the shape parameter and the nugget.

The reference is numpy fp64, never the code under test.  Every score is computed by two independent numpy routes,
  (A) Cholesky: log|K| from the factor's diagonal, everything else by solves against the factor,
  (B) eigvalsh for log|K| and np.linalg.inv for the rest,
and each case asserts on the CPU that they agree to REF_TOL = 1e-11 in the norm of the test, so the reference is well
inside the tolerances: |ML - ref| <= 1e-10 N (the project's RBF tolerance on the per-site likelihood), LOO relative 1e-10.
The searches are checked against the numpy profile, for which each test first asserts the conditions under which a grid +
golden-section search must find the minimum: an interior grid minimum and a strictly unimodal profile across the two cells
around it."""
import numpy as np
import pytest

from gpu_util import Canaried, bits, dev, ptr

pytestmark = pytest.mark.gpu
TOL = 1e-10
REF_TOL = 1e-11
LOO, ML = 0, 1
GOLDEN = 0.6180339887498949
#          raw kind, kriging
KINDS = {"gaussian": (0, False), "wendland": (2, False), "matern32": (3, False), "matern52": (4, False), "imq": (5, False),
         "kriging": (0, True), "kriging_matern32": (3, True), "kriging_matern52": (4, True)}


def phi(kind, eps, r):
    if kind == 0:
        return np.exp(-(eps * r) ** 2)
    if kind == 2:
        t = eps * r
        return np.where(t < 1.0, (1.0 - t) ** 4 * (4.0 * t + 1.0), 0.0)
    if kind == 3:
        t = np.sqrt(3.0) * eps * r
        return (1.0 + t) * np.exp(-t)
    if kind == 4:
        t = np.sqrt(5.0) * eps * r
        return (1.0 + t + t * t / 3.0) * np.exp(-t)
    assert kind == 5
    return 1.0 / np.sqrt(1.0 + (eps * r) ** 2)


def dist(x):
    return np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(axis=2))


def default_eps(name, n, dim):
    """each type's default shape; the 1-D Matern case uses 2 N"""
    kind = KINDS[name][0]
    if dim == 1 and kind in (3, 4):
        return 2.0 * n
    return (0.125 if kind == 2 else 2.0 if kind == 0 else 1.0) * n ** (1.0 / dim)


def smooth(orc, x):
    return orc.synth_response(x) + 3.0


def noisy(x):
    i = np.arange(len(x))
    return np.sin(3.0 * np.pi * x[:, 0]) * np.cos(2.0 * np.pi * x[:, 1]) + 0.35 * (((i + 1) * GOLDEN) % 1.0 - 0.5)


def scores(name, eps, nugget, r, f, route="A"):
    """(ML, LOO, sigma2, w) of one candidate in numpy; +inf scores when K does not factor (route A) / is not positive (B)"""
    kind, krige = KINDS[name]
    n = len(f)
    K = phi(kind, eps, r) + (nugget if krige else 0.0) * np.eye(n)
    one = np.ones(n)
    if route == "A":
        try:
            L = np.linalg.cholesky(K)
        except np.linalg.LinAlgError:
            return np.inf, np.inf, np.nan, None
        Li = np.linalg.solve(L, np.eye(n))                  # L^-1: triangular solves against the factor
        logdet = 2.0 * np.log(np.diag(L)).sum()
        Kf, b, g = Li.T @ (Li @ f), Li.T @ (Li @ one), (Li * Li).sum(axis=0)
    else:
        ev = np.linalg.eigvalsh(K)
        if not (ev > 0).all():
            return np.inf, np.inf, np.nan, None
        logdet = np.log(ev).sum()
        Ki = np.linalg.inv(K)
        Kf, b, g = Ki @ f, Ki @ one, np.diag(Ki).copy()
    w, diag = Kf, g
    if krige:
        w = Kf - (Kf.sum() / b.sum()) * b                   # w = K^-1 (f - mu 1), mu = 1^T K^-1 f / 1^T b
        diag = g - b * b / b.sum()                          # Dubrule
    fw = f @ w
    if not fw > 0 or not (diag > 0).all():
        return np.inf, np.inf, np.nan, None
    s2 = fw / n
    return 0.5 * (n * np.log(2.0 * np.pi * s2) + logdet + n), float(((w / diag) ** 2).mean()), s2, w


_cases = {}


def case(orc, name, dim, n, nugget):
    """centres, smooth response, default eps and the numpy reference (route A, checked here against route B) of one shape:
    computed once, shared, left unchanged"""
    key = (name, dim, n, nugget)
    if key not in _cases:
        x = orc.synth_centres(n, dim)
        f = smooth(orc, x)
        eps = default_eps(name, n, dim)
        r = dist(x)
        ml, loo, s2, w = scores(name, eps, nugget, r, f, "A")
        ml2, loo2, _, _ = scores(name, eps, nugget, r, f, "B")
        ref = (abs(ml - ml2) / n, abs(loo - loo2) / loo)
        print(f"reference {key}: Cholesky vs eigvalsh / inv: ML {ref[0]:.3e} per site, LOO {ref[1]:.3e} relative")
        for a in (x, f, w):
            a.setflags(write=False)
        _cases[key] = (x, f, eps, ml, loo, s2, w, ref)
    x, f, eps, ml, loo, s2, w, ref = _cases[key]
    assert ref[0] <= REF_TOL and ref[1] <= REF_TOL           # the reference itself is well inside TOL
    return x, f, eps, ml, loo, s2, w


def workspace(pkg, name, dim, n, x, f):
    s = pkg.Sinterp(name, dim, n, 0)
    fit = s.fit_workspace(x, np.array(f))
    return s, fit


# ---------------------------------------------------------------- 1. the raw reduction
_raw = {}


def raw_inputs(orc, n):
    """a Matern 5/2 matrix with its right-hand side, g and b in numpy (inputs only: the outputs are compared with numpy on
    the arrays the device holds)"""
    if n not in _raw:
        dim = 2
        x = orc.synth_centres(n, dim)
        f = smooth(orc, x)
        K = phi(4, default_eps("matern52", n, dim), dist(x))
        Ki = np.linalg.inv(K)
        g, b = np.diag(Ki).copy(), Ki @ np.ones(n)
        for a in (f, K, g, b):
            a.setflags(write=False)
        _raw[n] = (f, K, g, b)
    return _raw[n]


def reduce_reference(Ldiag, f, w, g, b, denom):
    """the four outputs and, for the three sums, the sum of |terms|"""
    with np.errstate(divide="ignore", invalid="ignore"):
        t0 = 2.0 * np.log(Ldiag)
    t1 = f * w
    bad = int((~((Ldiag > 0) & np.isfinite(Ldiag))).sum())
    t2 = np.zeros_like(f)
    if g is not None:
        diag = g - b * b / denom if b is not None else g
        with np.errstate(divide="ignore", invalid="ignore"):
            t2 = (w / diag) ** 2
        bad += int((~((diag > 0) & np.isfinite(diag))).sum())
    return [t0.sum(), t1.sum(), t2.sum(), float(bad)], [np.abs(t0).sum(), np.abs(t1).sum(), np.abs(t2).sum()]


@pytest.mark.parametrize("n", [1, 37, 128, 129, 1025])   # below one wave, one panel, a panel + 1, more than one pass of 1024 threads
def test_raw_reduction(pkg, orc, n):
    f, K, g, b = raw_inputs(orc, n)
    ctx = pkg.HipContext.on_torch_stream(0)
    lda = n + 3
    d_a = Canaried(np.array(K), ld=lda)
    d_f, d_w = Canaried(np.array(f)), Canaried(np.array(f))
    st, info = ctx.cholesky_factor_solve(n, d_a.ptr, lda, d_w.ptr, n, 1)
    assert st == 0 and info == 0
    ctx.sync()
    Ldiag, w = np.diag(d_a.get()).copy(), d_w.get()
    d_g, d_b = Canaried(np.array(g)), Canaried(np.array(b))
    denom = float(b.sum())
    for use_g, use_b in ((False, False), (True, False), (True, True), (False, True)):
        want, mass = reduce_reference(Ldiag, f, w, g if use_g else None, b if use_b and use_g else None, denom)
        got = []
        for rep in range(2):
            d_out = Canaried(np.full(4, 7.0))
            assert ctx.score_reduce(n, d_a.ptr, lda, d_f.ptr, d_w.ptr, d_g.ptr if use_g else None, d_b.ptr if use_b else None, denom,
                                    d_out.ptr) == 0
            ctx.sync()
            assert d_out.padding_intact()                    # nothing outside the 4 doubles is written
            got.append(d_out.get())
        assert np.array_equal(bits(got[0]), bits(got[1]))    # two calls: the same bits
        # one site with b: the kriging diagonal g - b^2 / (1^T b) is exactly 0 -- a bad site, counted, its term +inf
        degenerate = n == 1 and use_g and use_b
        with np.errstate(invalid="ignore"):
            err = [abs(got[0][q] - want[q]) / mass[q] if mass[q] else abs(got[0][q]) for q in range(3)]
        print(f"raw n {n} g {use_g} b {use_b}: |got - numpy| / sum |terms| = {err[0]:.2e} {err[1]:.2e} {err[2]:.2e}, count {got[0][3]}")
        assert max(err[:2]) <= 1e-13
        assert (got[0][2] == want[2] == np.inf) if degenerate else err[2] <= 1e-13
        assert got[0][3] == want[3] == (1.0 if degenerate else 0.0)     # the count matches exactly
        if not use_g:
            assert got[0][2] == 0.0
    for t in (d_a, d_f, d_w, d_g, d_b):
        assert t.padding_intact()
    ctx.close()


def test_raw_reduction_counts_bad_sites(pkg, orc):
    """planted data: a zero pivot, a negative and a NaN leave-one-out diagonal are counted; the count itself is never NaN"""
    n = 129
    f, K, g, b = raw_inputs(orc, n)
    ctx = pkg.HipContext.on_torch_stream(0)
    L = np.linalg.cholesky(K)
    w = np.linalg.solve(K, f)
    Lz = L.copy()
    Lz[40, 40] = 0.0
    Lz[128, 128] = -1.0
    gz = np.array(g)
    gz[7] = -gz[7]
    gz[100] = np.nan
    d_f, d_w, d_out = dev(np.array(f)), dev(w), Canaried(np.zeros(4))
    for Luse, guse, count in ((Lz, None, 2.0), (L, gz, 2.0), (Lz, gz, 4.0)):
        d_a = dev(Luse)
        d_g = dev(guse) if guse is not None else None
        assert ctx.score_reduce(n, ptr(d_a), n, ptr(d_f), ptr(d_w), ptr(d_g) if d_g is not None else None, None, 1.0, d_out.ptr) == 0
        ctx.sync()
        got = d_out.get()
        want, _ = reduce_reference(np.diag(Luse).copy(), f, w, guse, None, 1.0)
        print(f"planted: got {got}, numpy {want}")
        assert got[3] == count == want[3]
        assert abs(got[1] - want[1]) <= 1e-13 * np.abs(f * w).sum()          # the clean sum is not disturbed
        if guse is None:
            assert got[2] == 0.0
    assert d_out.padding_intact()
    ctx.close()


def test_raw_reduction_argument_checks(pkg):
    ctx = pkg.HipContext.on_torch_stream(0)
    buf = dev(np.ones(128))
    p = ptr(buf)
    args = dict(n=8, d_llt=p, lda=8, d_f=p, d_w=p, d_g=None, d_b=None, denom=1.0, d_out=p)
    call = lambda **kw: ctx.score_reduce(**{**args, **kw})
    assert call(lda=7) == pkg.GSL_EINVAL
    for name in ("d_llt", "d_f", "d_w", "d_out"):
        assert call(**{name: None}) == pkg.capi.GSL_EFAULT
    d_out = Canaried(np.full(4, 7.0))
    assert call(n=0, lda=0, d_llt=None, d_f=None, d_w=None, d_out=d_out.ptr) == 0
    ctx.sync()
    assert (d_out.get() == 0.0).all() and d_out.padding_intact()                 # n = 0 writes four zeros
    assert call(n=0, lda=0, d_llt=None, d_f=None, d_w=None, d_out=None) == 0
    ctx.close()


# ---------------------------------------------------------------- 2. the scores against numpy
SCORE_CASES = [
    ("matern32", 2, 37, 0.0),
    ("matern52", 2, 128, 0.0),
    ("imq", 3, 129, 0.0),
    ("gaussian", 2, 300, 0.0),
    ("wendland", 2, 300, 0.0),
    ("matern32", 1, 100, 0.0),
    ("kriging", 2, 300, 1e-3),
    ("kriging_matern32", 2, 129, 0.0),
    ("kriging_matern52", 3, 300, 1e-2),
    ("kriging_matern52", 2, 257, 1e-3),
]


@pytest.mark.parametrize("name,dim,n,nugget", SCORE_CASES)
def test_scores_match_numpy(pkg, orc, name, dim, n, nugget):
    x, f, eps, ml, loo, s2, _ = case(orc, name, dim, n, nugget)
    s, fit = workspace(pkg, name, dim, n, x, f)
    with pkg.capi.ErrorCalls() as calls:
        st, got_ml = fit.score(ML, eps, nugget)
        st2, got_s2 = fit.sigma2()
        st3, got_loo = fit.score(LOO, eps, nugget)
    print(f"{name} dim {dim} n {n} nugget {nugget}: ML {got_ml:.12g} (numpy {ml:.12g}, |d| / N = {abs(got_ml - ml) / n:.3e}), "
          f"LOO {got_loo:.12g} (numpy {loo:.12g}, relative {abs(got_loo - loo) / loo:.3e}), sigma2 relative {abs(got_s2 - s2) / s2:.3e}")
    assert st == 0 and st2 == 0 and st3 == 0 and calls == []
    assert abs(got_ml - ml) <= TOL * n
    assert abs(got_loo - loo) <= TOL * loo
    assert abs(got_s2 - s2) <= TOL * s2
    fit.close()


# ---------------------------------------------------------------- 3. consistency with what exists
@pytest.mark.parametrize("name,dim,n,nugget", [SCORE_CASES[1], SCORE_CASES[3], SCORE_CASES[8]])
def test_consistent_with_the_init(pkg, orc, name, dim, n, nugget):
    x, f, eps, _, _, _, _ = case(orc, name, dim, n, nugget)
    s, fit = workspace(pkg, name, dim, n, x, f)
    st, got_loo = fit.score(LOO, eps, nugget)
    st2, got_s2 = fit.sigma2()
    assert st == 0 and st2 == 0
    assert s.n_fields() == 0 and s._p.contents.shape == 0.0 and s._p.contents.want_loo == 0      # the interpolant is untouched
    m = pkg.Sinterp(name, dim, n, 0)
    assert m.set_shape(eps) == 0 and m.set_loo(1) == 0
    if KINDS[name][1]:
        assert m.set_nugget(nugget) == 0
    assert m.init(x, np.array(f)) == 0 and m.route() in (1, 7)
    st, E = m.loo_residuals()
    st2, w = m.weights()
    assert st == 0 and st2 == 0
    want_loo, want_s2 = float((E[:, 0] ** 2).mean()), float(f @ w) / n
    print(f"{name}: LOO {got_loo:.15g} vs mean(loo_residuals^2) {want_loo:.15g}; sigma2 {got_s2:.15g} vs f.w / N {want_s2:.15g}")
    assert abs(got_loo - want_loo) <= 1e-12 * want_loo       # the same weights and diagonal: only the order of the sum differs
    assert abs(got_s2 - want_s2) <= 1e-12 * abs(want_s2)
    fit.close()


# ---------------------------------------------------------------- 4. the searches
N_SEARCH, DIM_SEARCH = 150, 2
E0 = N_SEARCH ** 0.5
SEARCH_CASES = [
    ("kriging_matern52", 1e-2, E0 / 8, 4 * E0),
    ("kriging", 1e-2, E0 / 8, 4 * E0),
    ("kriging_matern32", 1e-2, E0 / 8, 4 * E0),
    ("matern32", 0.0, E0 / 4, 4 * E0),
]
N_GRID, SEARCH_TOL, MAX_EVAL, N_FINE = 9, 1e-2, 40, 201
_search = {}


def search_data(orc):
    if "data" not in _search:
        x = orc.synth_centres(N_SEARCH, DIM_SEARCH)
        f = noisy(x)
        r = dist(x)
        for a in (x, f, r):
            a.setflags(write=False)
        _search["data"] = (x, f, r)
    return _search["data"]


def profile_reference(key, score_at, lo, hi):
    """numpy's side of a search: the grid, its first minimum k (asserted interior), the fine profile across the two cells
    around it (asserted strictly unimodal) and its minimum.  score_at(p) is one numpy score, checked against route B.
    Returns (grid parameters, grid scores, p*, fine step in t)."""
    if key not in _search:
        t = np.linspace(np.log(lo), np.log(hi), N_GRID)
        gs = np.array([score_at(p, True) for p in np.exp(t)])
        k = int(np.argmin(gs))
        fine = np.linspace(t[max(k - 1, 0)], t[min(k + 1, N_GRID - 1)], N_FINE)
        fs = np.array([score_at(p, False) for p in np.exp(fine)])
        _search[key] = (np.exp(t), gs, k, fine, fs)
    p, gs, k, fine, fs = _search[key]
    assert 0 < k < N_GRID - 1 and np.isfinite(gs[k])                            # the grid minimum is interior
    j = int(np.argmin(fs))
    d = np.diff(fs)
    assert 0 < j < N_FINE - 1 and (d[:j] < 0).all() and (d[j:] > 0).all()       # strictly unimodal across the two cells
    return p, gs, float(np.exp(fine[j])), float(fine[1] - fine[0])


def checked_score(name, criterion, eps, nugget, r, f, both):
    """one numpy score (route A); with `both`, route B must agree to REF_TOL"""
    idx = 0 if criterion == ML else 1
    a = scores(name, eps, nugget, r, f, "A")[idx]
    if both:
        b = scores(name, eps, nugget, r, f, "B")[idx]
        assert abs(a - b) <= REF_TOL * (len(f) if criterion == ML else a)
    return a


def check_search(fit, criterion, over_nugget, fixed, lo, hi, grid_p, grid_s, p_star, step, numpy_score):
    n = N_SEARCH
    run = (lambda: fit.fit_nugget(criterion, fixed, lo, hi)) if over_nugget else (lambda: fit.fit_shape(criterion, lo, hi, fixed))
    point = (lambda p: fit.score(criterion, fixed, p)) if over_nugget else (lambda p: fit.score(criterion, p, fixed))
    st, best, score = run()
    n_eval = fit.n_eval()
    st_t, tp, ts = fit.trace()
    print(f"  best {best:.10g} (numpy {p_star:.10g}, |d log| = {abs(np.log(best) - np.log(p_star)):.3e}), score {score:.12g}, "
          f"{n_eval} evaluations")
    assert st == 0 and st_t == 0
    assert N_GRID + 2 <= n_eval <= MAX_EVAL
    assert abs(np.log(best) - np.log(p_star)) <= 2 * SEARCH_TOL + step
    at_best = numpy_score(best)
    assert at_best <= grid_s.min() + 1e-9 * (n if criterion == ML else grid_s.min())
    st2, again = point(best)
    assert st2 == 0 and bits(again) == bits(score)           # the value fit_score returns there, not a recomputation
    assert len(tp) == n_eval and len(ts) == n_eval
    assert np.abs(tp[:N_GRID] / grid_p - 1.0).max() <= 1e-14 and tp[0] == lo and tp[N_GRID - 1] == hi      # the grid, in order
    lim = TOL * n if criterion == ML else TOL * grid_s
    assert (np.abs(ts[:N_GRID] - grid_s) <= lim).all()
    assert score == ts.min() and best == tp[int(np.argmin(ts))]                 # the lowest-scoring point ever evaluated
    st3, best2, score2 = run()                                                  # a second identical search: the same bits
    assert st3 == 0 and bits(best2) == bits(best) and bits(score2) == bits(score) and fit.n_eval() == n_eval
    assert np.array_equal(bits(fit.trace()[2]), bits(ts))
    return best


@pytest.mark.parametrize("criterion", [ML, LOO])
@pytest.mark.parametrize("name,nugget,lo,hi", SEARCH_CASES)
def test_fit_shape(pkg, orc, name, nugget, lo, hi, criterion):
    x, f, r = search_data(orc)
    at = lambda eps, both=False: checked_score(name, criterion, eps, nugget, r, f, both)
    grid_p, grid_s, p_star, step = profile_reference(("shape", name, criterion), at, lo, hi)
    s, fit = workspace(pkg, name, DIM_SEARCH, N_SEARCH, x, f)
    print(f"fit_shape {name} criterion {criterion}:")
    with pkg.capi.ErrorCalls() as calls:
        check_search(fit, criterion, False, nugget, lo, hi, grid_p, grid_s, p_star, step, at)
    assert calls == []
    fit.close()


@pytest.mark.parametrize("criterion", [ML, LOO])
def test_fit_nugget(pkg, orc, criterion):
    """kriging Matern 5/2 at the shape numpy fits for the criterion (nugget 1e-2), nugget bracket [1e-4, 1]"""
    name, lo, hi = "kriging_matern52", 1e-4, 1.0
    x, f, r = search_data(orc)
    shape_at = lambda eps, both=False: checked_score(name, criterion, eps, 1e-2, r, f, both)
    eps = profile_reference(("shape", name, criterion), shape_at, *SEARCH_CASES[0][2:])[2]
    at = lambda nug, both=False: checked_score(name, criterion, eps, nug, r, f, both)
    grid_p, grid_s, p_star, step = profile_reference(("nugget", name, criterion), at, lo, hi)
    s, fit = workspace(pkg, name, DIM_SEARCH, N_SEARCH, x, f)
    print(f"fit_nugget {name} criterion {criterion} at eps {eps:.6g}:")
    check_search(fit, criterion, True, eps, lo, hi, grid_p, grid_s, p_star, step, at)
    fit.close()


# ---------------------------------------------------------------- 5. candidates that do not factor
def test_non_definite_candidates_score_infinity(pkg, orc):
    name, lo, hi = "gaussian", E0 / 64, 4 * E0
    x, f, r = search_data(orc)
    t = np.linspace(np.log(lo), np.log(hi), N_GRID)
    gs = np.array([scores(name, p, 0.0, r, f, "A")[0] for p in np.exp(t)])
    kb = int(np.argmin(gs))
    print(f"numpy grid scores {gs}")
    assert np.isinf(gs).any() and np.isfinite(gs[kb]) and 0 < kb < N_GRID - 1   # the case is what it is meant to be
    s, fit = workspace(pkg, name, DIM_SEARCH, N_SEARCH, x, f)
    with pkg.capi.ErrorCalls() as calls:
        st, best, score = fit.fit_shape(ML, lo, hi)
        st_t, tp, ts = fit.trace()
        again = [fit.score(ML, p) for p in tp]
    print(f"device trace {list(zip(tp, ts))}")
    assert st == 0 and st_t == 0 and calls == []             # a candidate that does not factor is not an error
    assert not np.isnan(ts).any() and ((ts == np.inf) | np.isfinite(ts)).all()
    assert all(a[0] == 0 and not np.isnan(a[1]) for a in again)
    assert np.isfinite(score) and np.exp(t[kb - 1]) < best < np.exp(t[kb + 1])
    # a bracket in which numpy fails everywhere: the device may or may not factor there -- either, but nothing in between
    lo2, hi2 = E0 / 4096, E0 / 2048
    assert all(np.isinf(scores(name, p, 0.0, r, f, "A")[0]) for p in np.exp(np.linspace(np.log(lo2), np.log(hi2), N_GRID)))
    with pkg.capi.ErrorCalls() as calls:
        st, best, score = fit.fit_shape(ML, lo2, hi2)
    if st == 0:
        assert np.isfinite(score) and lo2 <= best <= hi2 and calls == []
    else:
        assert st == pkg.GSL_EDOM and np.isnan(best) and np.isnan(score) and [c[1] for c in calls] == [pkg.GSL_EDOM]
        assert fit.n_eval() == N_GRID and (fit.trace()[2] == np.inf).all()
    fit.close()


def test_real_failures_go_through_the_handler(pkg, orc):
    x, f, r = search_data(orc)
    s, fit = workspace(pkg, "matern52", DIM_SEARCH, N_SEARCH, x, f)
    sk, kfit = workspace(pkg, "kriging_matern52", DIM_SEARCH, N_SEARCH, x, f)
    EINVAL = pkg.GSL_EINVAL
    with pkg.capi.ErrorCalls() as calls:
        for st, v in (fit.score(2, E0), fit.score(ML, 0.0), fit.score(ML, -1.0), fit.score(ML, np.inf), fit.score(ML, np.nan),
                      fit.score(ML, E0, 1e-3), kfit.score(ML, E0, -1e-3)):
            assert st == EINVAL and np.isnan(v)
        for st, p, v in (fit.fit_shape(ML, 0.0, E0), fit.fit_shape(ML, E0, E0), fit.fit_shape(ML, 2 * E0, E0), fit.fit_shape(ML, E0, np.inf),
                         fit.fit_shape(ML, E0, 2 * E0, nugget=1e-3), fit.fit_shape(3, E0, 2 * E0), fit.fit_nugget(ML, E0, 1e-4, 1.0),
                         kfit.fit_nugget(ML, E0, 0.0, 1.0), kfit.fit_nugget(ML, -E0, 1e-4, 1.0)):
            assert st == EINVAL and np.isnan(p) and np.isnan(v)
    assert [c[1] for c in calls] == [EINVAL] * 16
    assert fit.sigma2()[0] == EINVAL                         # no finite score yet
    assert fit.set_search(2, 1e-2, 40) == EINVAL and fit.set_search(9, 0.0, 40) == EINVAL and fit.set_search(9, 1e-2, 8) == EINVAL
    assert kfit.score(ML, E0, 0.0)[0] == 0                   # nugget 0 is compared through fit_score
    fit.close()
    kfit.close()


# ---------------------------------------------------------------- 6. reuse and cleanup
def test_one_workspace_serves_everything_in_any_order(pkg, orc):
    name, nugget, lo, hi = SEARCH_CASES[0]
    x, f, r = search_data(orc)
    s, fit = workspace(pkg, name, DIM_SEARCH, N_SEARCH, x, f)
    s.close()                                                # the workspace outlives the interpolant it was made from
    eps = 0.7 * E0
    st, ml0 = fit.score(ML, eps, nugget)
    st2, s2_0 = fit.sigma2()
    assert st == 0 and st2 == 0
    st, loo0 = fit.score(LOO, eps, nugget)                   # allocates the leave-one-out buffers, reuses the matrix
    assert st == 0
    st, ml1 = fit.score(ML, eps, nugget)                     # ... and the ML score after it has the same bits
    assert st == 0 and bits(ml1) == bits(ml0)
    a = fit.fit_shape(ML, lo, hi, nugget)
    b = fit.fit_shape(LOO, lo, hi, nugget)
    c = fit.fit_nugget(ML, a[1], 1e-4, 1.0)
    d = fit.fit_nugget(LOO, a[1], 1e-4, 1.0)
    assert a[0] == 0 and b[0] == 0 and c[0] == 0 and d[0] == 0
    st, s2_best = fit.sigma2()                               # of the score handed back: the search's best
    st2, v = fit.score(LOO, a[1], d[1])
    assert st == 0 and st2 == 0 and bits(v) == bits(d[2]) and bits(fit.sigma2()[1]) == bits(s2_best)
    st, loo1 = fit.score(LOO, eps, nugget)
    st2, ml2 = fit.score(ML, eps, nugget)
    assert st == 0 and st2 == 0 and bits(loo1) == bits(loo0) and bits(ml2) == bits(ml0) and bits(fit.sigma2()[1]) == bits(s2_0)
    # a second workspace that only ever searches gives the first one's bits
    s2, other = workspace(pkg, name, DIM_SEARCH, N_SEARCH, x, f)
    assert [bits(q) for q in other.fit_shape(LOO, lo, hi, nugget)[1:]] == [bits(q) for q in b[1:]]
    # the budget: a search stops at max_eval, and its trace is that long
    assert other.set_search(5, 1e-3, 7) == 0
    st, p, v = other.fit_shape(ML, lo, hi, nugget)
    assert st == 0 and other.n_eval() == 7 and len(other.trace()[1]) == 7 and np.isfinite(v)
    pkg.lib().gsl_sinterp_fit_free(None)                     # a no-op
    other.close()
    fit.close()
    fit.close()                                              # closing twice is harmless
