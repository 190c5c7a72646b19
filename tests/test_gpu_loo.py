"""-m gpu: leave-one-out residuals e_i = f_i - s^(-i)(x_i) and variances v_i from the Cholesky factor of the init
(csrc/hip/loo.hip): e_i = w_i / diag_i, v_i = 1 / diag_i with diag = diag(K^-1) (Rippa) or diag(K^-1) - b^2 / (1^T b)
(ordinary kriging, Dubrule).

The reference is numpy fp64, never the code under test:
  (a) ACTUAL DELETION for n <= 384: n solves with site i removed (the bordered system for kriging); the variance is the
      formula of reference_variance (test_gpu_krige_variance.py) on the reduced model at x_i, plus the nugget (for the
      plain types: the squared power function 1 - k^T K_-i^-1 k);
  (b) THE IDENTITY with np.linalg.inv for larger n.
Every case asserts on the CPU that (a) and (b) agree to REF_TOL = 1e-11 in the norms of the test, so the reference itself
is well inside TOL = 1e-10 (the project's RBF tolerance): residuals relative to max |e_ref| per field, variances absolute
(the sill is 1), g relative to max g."""
import numpy as np
import pytest

from gpu_util import Canaried, bits, dev, ptr
from test_gpu_krige_variance import dist, phi

pytestmark = pytest.mark.gpu
TOL = 1e-10
REF_TOL = 1e-11
GAUSSIAN, WENDLAND = 0, 2
KIND = {"gaussian": GAUSSIAN, "wendland": WENDLAND, "kriging": GAUSSIAN}


def default_eps(kind, n, dim):
    return (0.125 if kind == "wendland" else 2.0) * n ** (1.0 / dim)


def fields_of(orc, x, k):
    """k smooth, different responses on the centres"""
    f = orc.synth_response(x) + 3.0
    maps = [lambda v: v, np.sin, lambda v: v * v + 0.5 * v, np.cos, lambda v: np.exp(0.3 * v), lambda v: 1.0 / (2.0 + v * v)]
    return np.ascontiguousarray(np.stack([maps[q % len(maps)]((1.0 + q // len(maps)) * f) for q in range(k)], axis=1))


def loo_by_deletion(kind, eps, nugget, x, F):
    """(E, v) from n models built without one site each"""
    n, nf = F.shape
    krige = kind == "kriging"
    Phi = phi(KIND[kind], eps, dist(x, x))
    K = Phi + (nugget if krige else 0.0) * np.eye(n)
    E, v = np.empty((n, nf)), np.empty(n)
    for i in range(n):
        keep = np.arange(n) != i
        Kr, k = K[np.ix_(keep, keep)], Phi[keep, i]
        if krige:
            A = np.zeros((n, n))                            # [K_-i 1; 1^T 0] [w; mu] = [f_-i; 0]
            A[:n - 1, :n - 1] = Kr
            A[:n - 1, n - 1] = A[n - 1, :n - 1] = 1.0
            sol = np.linalg.solve(A, np.vstack([F[keep], np.zeros((1, nf))]))
            E[i] = F[i] - (sol[n - 1] + k @ sol[:n - 1])
            kb = np.linalg.solve(Kr, np.column_stack([k, np.ones(n - 1)]))       # reference_variance's formula, one target
            v[i] = 1.0 - k @ kb[:, 0] + (1.0 - kb[:, 1] @ k) ** 2 / kb[:, 1].sum() + nugget
        else:
            sol = np.linalg.solve(Kr, np.column_stack([F[keep], k]))
            E[i] = F[i] - k @ sol[:, :nf]
            v[i] = 1.0 - k @ sol[:, nf]
    return E, v


def loo_by_identity(kind, eps, nugget, x, F):
    """(E, v, g) from the inverse of the whole matrix"""
    n = len(x)
    krige = kind == "kriging"
    K = phi(KIND[kind], eps, dist(x, x)) + (nugget if krige else 0.0) * np.eye(n)
    g = np.diag(np.linalg.inv(K)).copy()
    W = np.linalg.solve(K, F)
    diag = g
    if krige:
        b = np.linalg.solve(K, np.ones(n))
        W = W - np.outer(b, (W.sum(axis=0)) / b.sum())      # w = K^-1 f - mu b, mu = 1^T K^-1 f / 1^T b
        diag = g - b * b / b.sum()
    return W / diag[:, None], 1.0 / diag, g


def res_err(got, want):
    """max over the fields of max_i |got - want| / max_i |want|"""
    return float((np.abs(got - want).max(axis=0) / np.abs(want).max(axis=0)).max())


_cases = {}


def case(orc, kind, dim, n, nugget, nf=1, first=0):
    """centres, responses and the reference of one shape: computed once, shared, left unchanged.  Returns
    (x, F, eps, E_ref, v_ref); the reference is the deletion (a), checked here against the identity (b)."""
    key = (kind, dim, n, nugget, nf, first)
    if key not in _cases:
        x = orc.synth_centres(first + n, dim)[first:].copy()
        F = fields_of(orc, x, nf)
        eps = default_eps(kind, n, dim)
        E, v = loo_by_deletion(kind, eps, nugget, x, F)
        E2, v2, _ = loo_by_identity(kind, eps, nugget, x, F)
        ref = (res_err(E2, E), float(np.abs(v2 - v).max()))
        print(f"reference {key}: deletion vs identity: residuals {ref[0]:.3e}, variances {ref[1]:.3e}")
        for a in (x, F, E, v):
            a.setflags(write=False)
        _cases[key] = (x, F, eps, E, v, ref)
    x, F, eps, E, v, ref = _cases[key]
    assert ref[0] <= REF_TOL and ref[1] <= REF_TOL           # the reference itself is well inside TOL
    return x, F, eps, E, v


def model(pkg, kind, dim, n, nugget=0.0, loo=True, variance=False, devices=None, eps=None):
    s = pkg.Sinterp(kind, dim, n, 0)
    if devices is not None:
        assert s.set_device_list(devices) == 0
    if kind == "kriging":
        assert s.set_nugget(nugget) == 0
        if variance:
            assert s.set_variance(1) == 0
    if eps is not None:
        assert s.set_shape(eps) == 0
    if loo:
        assert s.set_loo(1) == 0
    return s


# ---------------------------------------------------------------- 1. facade vs deletion
@pytest.mark.parametrize("kind,dim,n,nugget", [
    ("gaussian", 2, 300, 0.0),
    ("wendland", 2, 384, 0.0),        # exactly 3 blocks
    ("kriging", 2, 300, 0.0),
    ("kriging", 2, 384, 1e-3),
    ("kriging", 3, 300, 1e-2),
    ("kriging", 2, 100, 1e-3),        # one partial block
    ("kriging", 2, 129, 1e-3),        # one block + 1 column
    ("gaussian", 1, 100, 0.0),        # 1-D: the worst conditioning for which deletion and identity still agree to REF_TOL
])
def test_facade_matches_deletion(pkg, orc, kind, dim, n, nugget):
    x, F, eps, E, v = case(orc, kind, dim, n, nugget)
    s = model(pkg, kind, dim, n, nugget)
    assert s.init(x, F[:, 0].copy()) == 0 and s.route() in (1, 7)
    st, got_e = s.loo_residuals()
    st2, got_v = s.loo_variance()
    assert st == 0 and st2 == 0 and got_e.shape == (n, 1)
    er, ev = res_err(got_e, E), np.abs(got_v - v).max()
    print(f"{kind} dim {dim} n {n} nugget {nugget}: residuals {er:.3e} of max |e| = {np.abs(E).max():.3e}, variances {ev:.3e}, "
          f"min v = {got_v.min():.3e}")
    assert er < TOL and ev < TOL
    assert (got_v > 0.0).all()
    if kind == "kriging" and nugget == 0.0:
        # v_i is what eval_variance of the model WITHOUT site i returns at x_i (+ the nugget, 0 here)
        for i in (0, n // 2, n - 1):
            keep = np.arange(n) != i
            r = model(pkg, kind, dim, n - 1, nugget, loo=False, variance=True, eps=eps)
            assert r.init(np.ascontiguousarray(x[keep]), F[keep, 0].copy()) == 0 and r.route() == 7
            stv, var = r.eval_variance_many(np.ascontiguousarray(x[i:i + 1]))
            assert stv == 0 and abs(var[0] - got_v[i]) < 2 * TOL


# ---------------------------------------------------------------- 2. the raw entry
_raw = {}


def raw_reference(orc, n):
    """K, its inverse diagonal (b) and the device factor's inputs for the raw tests; kriging matrix with nugget 1e-3"""
    if n not in _raw:
        dim, nugget = 2, 1e-3
        x = orc.synth_centres(n, dim)
        f = orc.synth_response(x) + 3.0
        eps = orc.gaussian_eps(n, dim)
        K = phi(GAUSSIAN, eps, dist(x, x)) + nugget * np.eye(n)
        g = np.diag(np.linalg.inv(K)).copy()
        for a in (x, f, g):
            a.setflags(write=False)
        _raw[n] = (x, f, eps, nugget, g)
    return _raw[n]


@pytest.mark.parametrize("n", [700, 1280])        # a tail of 60 columns; exactly 10 blocks
def test_raw_entry_strided_and_chunked(pkg, orc, n):
    dim = 2
    x, f, eps, nugget, want = raw_reference(orc, n)
    ctx = pkg.HipContext.on_torch_stream(0)
    lda = n + 6
    d_x = dev(np.array(x))                                   # copies: the shared reference arrays are read-only
    d_phi = Canaried(np.zeros((n, n)), ld=lda)
    d_w = dev(np.array(f))
    st, route, _ = ctx.krige_solve(GAUSSIAN, eps, nugget, ptr(d_x), n, dim, dim, d_phi.ptr, lda, ptr(d_w))
    assert st == 0 and route == 7                            # L is in the lower triangle of d_phi now
    ctx.sync()
    a = d_phi.get()
    a[np.triu_indices(n, 1)] = np.nan                        # only the lower triangle may be read
    d_phi.set(a)
    out = {}
    for chunk in (128, 256, 512, 4096, 256):                 # several c0, a growing alive-row count, a single pass; 256 twice
        work = pkg.HipContext.chol_inv_diag_work(n, chunk)
        d_work = dev(np.full(work, np.nan))
        d_g = Canaried(np.zeros(n))
        st = ctx.chol_inv_diag(n, d_phi.ptr, lda, d_g.ptr, ptr(d_work), chunk)
        ctx.sync()
        assert st == 0
        got = d_g.get()
        err = np.abs(got - want).max() / want.max()
        print(f"raw n {n} chunk {chunk}: max |g - want| / max g = {err:.3e}")
        assert err < TOL
        assert d_g.padding_intact()
        if chunk in out:
            assert np.array_equal(bits(out[chunk]), bits(got))        # run to run at one chunk: bit for bit
        out[chunk] = got
    assert d_phi.padding_intact()
    for chunk in (128, 256, 512):
        assert np.abs(out[chunk] - out[4096]).max() / want.max() < 2 * TOL     # across chunks: to rounding
    ctx.close()


def test_raw_combine(pkg):
    rng = np.random.default_rng(5)
    n, nf, ldw, lde = 300, 3, 307, 301
    g = 1.0 + rng.random(n)
    b = rng.random(n) - 0.5
    denom = 7.25
    W = rng.standard_normal((nf, n))
    ctx = pkg.HipContext.on_torch_stream(0)
    d_g, d_b, d_w = dev(g), dev(b), Canaried(W, ld=ldw)
    for use_b in (False, True):
        diag = g - b * b / denom if use_b else g
        d_e, d_v = Canaried(np.zeros((nf, n)), ld=lde), Canaried(np.zeros(n))
        assert ctx.loo_combine(n, nf, ptr(d_g), ptr(d_b) if use_b else None, denom, d_w.ptr, ldw, d_e.ptr, lde, d_v.ptr) == 0
        ctx.sync()
        # one division each, no FMA to contract apart from b * b / denom: a few ulp
        assert np.abs(d_e.get() - W / diag).max() <= 1e-14 * np.abs(W / diag).max()
        assert np.abs(d_v.get() - 1.0 / diag).max() <= 1e-14
        assert d_e.padding_intact() and d_v.padding_intact() and d_w.padding_intact()
    ctx.close()


def test_raw_entry_argument_checks(pkg):
    ctx = pkg.HipContext.on_torch_stream(0)
    buf = dev(np.zeros(pkg.HipContext.chol_inv_diag_work(8, 128) + 64))
    p = ptr(buf)
    args = dict(n=8, d_llt=p, lda=8, d_g=p, d_work=p, chunk=128)
    call = lambda **kw: ctx.chol_inv_diag(**{**args, **kw})
    assert call(lda=7) == pkg.GSL_EINVAL and call(chunk=0) == pkg.GSL_EINVAL
    assert call(d_llt=None) == pkg.capi.GSL_EFAULT and call(d_g=None) == pkg.capi.GSL_EFAULT and call(d_work=None) == pkg.capi.GSL_EFAULT
    assert call(n=0, lda=0, d_llt=None, d_g=None, d_work=None) == 0                # nothing to do: nothing launched
    comb = dict(n=8, nf=2, d_g=p, d_b=None, denom=1.0, d_w=p, ldw=8, d_e=p, lde=8, d_v=p)
    ccall = lambda **kw: ctx.loo_combine(**{**comb, **kw})
    assert ccall(ldw=7) == pkg.GSL_EINVAL and ccall(lde=7) == pkg.GSL_EINVAL and ccall(nf=65) == pkg.GSL_EINVAL
    assert ccall(d_g=None) == pkg.capi.GSL_EFAULT and ccall(d_v=None) == pkg.capi.GSL_EFAULT and ccall(d_e=None) == pkg.capi.GSL_EFAULT
    assert ccall(n=0, d_g=None, d_w=None, d_e=None, d_v=None) == 0
    ctx.close()


# ---------------------------------------------------------------- 3. fields
@pytest.mark.parametrize("kind,nf,nugget", [("gaussian", 7, 0.0), ("kriging", 3, 1e-3)])
def test_fields_share_the_diagonal(pkg, orc, kind, nf, nugget):
    dim, n = 2, 300
    x, F, eps, E, v = case(orc, kind, dim, n, nugget, nf=nf)
    s = model(pkg, kind, dim, n, nugget)
    assert s.init_fields(x, F) == 0 and s.route() in (1, 7) and s.n_fields() == nf
    st, got_e = s.loo_residuals()
    st2, got_v = s.loo_variance()
    assert st == 0 and st2 == 0 and got_e.shape == (n, nf)
    per_field = np.abs(got_e - E).max(axis=0) / np.abs(E).max(axis=0)
    print(f"{kind} {nf} fields: residuals per field {per_field}, variances {np.abs(got_v - v).max():.3e}")
    assert per_field.max() < TOL and np.abs(got_v - v).max() < TOL
    # a strided E: the padding is left alone
    wide = np.full((n, nf + 2), 7.0)
    st, _ = s.loo_residuals(out=wide[:, :nf])
    assert st == 0 and np.array_equal(bits(wide[:, :nf]), bits(got_e)) and (wide[:, nf:] == 7.0).all()
    assert s.loo_residuals(out=np.zeros((n, nf + 1)))[0] == pkg.capi.GSL_EBADLEN
    assert s.loo_variance(out=np.zeros(n + 1))[0] == pkg.capi.GSL_EBADLEN
    # the variance does not depend on the responses: the one-field model's
    one = model(pkg, kind, dim, n, nugget)
    assert one.init(x, F[:, 0].copy()) == 0
    st, v1 = one.loo_variance()
    assert st == 0 and np.abs(v1 - got_v).max() < 2 * TOL


# ---------------------------------------------------------------- 4. states
def test_states(pkg, orc, tmp_path):
    dim, n, nugget = 2, 300, 1e-3
    x, F, eps, E, v = case(orc, "kriging", dim, n, nugget)
    f = F[:, 0].copy()
    y = np.ascontiguousarray(np.vstack([orc.synth_targets(0, 200, dim), x[:20]]))
    off = model(pkg, "kriging", dim, n, nugget, loo=False, variance=True)
    assert off.set_loo(0) == 0
    assert off.loo_residuals()[0] == pkg.GSL_EINVAL and off.loo_variance()[0] == pkg.GSL_EINVAL      # not initialised
    assert off.init(x, f) == 0
    assert off.loo_residuals()[0] == pkg.GSL_EINVAL and off.loo_variance()[0] == pkg.GSL_EINVAL      # initialised without set_loo
    on = model(pkg, "kriging", dim, n, nugget, variance=True)
    assert on.init(x, f) == 0
    st, e_on = on.loo_residuals()
    assert st == 0 and res_err(e_on, E) < TOL
    # the predictor, the weights and the kriging variance do not notice
    assert np.array_equal(bits(on.eval_many(y)[1]), bits(off.eval_many(y)[1]))
    assert np.array_equal(bits(on.weights()[1]), bits(off.weights()[1]))
    sv_on, var_on = on.eval_variance_many(y)
    sv_off, var_off = off.eval_variance_many(y)
    assert sv_on == 0 and sv_off == 0 and np.array_equal(bits(var_on), bits(var_off))
    # without set_variance b and 1^T b come from temporaries: the same numbers
    plain = model(pkg, "kriging", dim, n, nugget)
    assert plain.init(x, f) == 0
    assert np.array_equal(bits(plain.loo_residuals()[1]), bits(e_on))
    # a checkpoint carries no leave-one-out data, and reading one drops what was held
    path = tmp_path / "loo.bin"
    assert on.fwrite(str(path)) == 0
    r = model(pkg, "kriging", dim, n, nugget)
    assert r.fread(str(path)) == 0
    assert r.loo_residuals()[0] == pkg.GSL_EINVAL and r.loo_variance()[0] == pkg.GSL_EINVAL
    assert on.fread(str(path)) == 0 and on.loo_residuals()[0] == pkg.GSL_EINVAL
    # a device group: member 0 computes it
    grp = model(pkg, "kriging", dim, n, nugget, devices=[0, 0, 0])
    assert grp.init(x, f) == 0
    st, e_grp = grp.loo_residuals()
    assert st == 0 and np.array_equal(bits(e_grp), bits(e_on))
    assert np.array_equal(bits(grp.loo_variance()[1]), bits(plain.loo_variance()[1]))


def test_reinit_replaces_the_held_arrays(pkg, orc):
    dim, n, nugget = 2, 300, 1e-3
    xa, Fa, _, Ea, va = case(orc, "kriging", dim, n, nugget)
    xb, Fb, _, Eb, vb = case(orc, "kriging", dim, n, nugget, first=n)       # other sites AND other values
    s = model(pkg, "kriging", dim, n, nugget)
    assert s.init(xa, Fa[:, 0].copy()) == 0
    assert res_err(s.loo_residuals()[1], Ea) < TOL
    assert s.init(xb, Fb[:, 0].copy()) == 0
    st, e = s.loo_residuals()
    assert st == 0 and res_err(e, Eb) < TOL and np.abs(s.loo_variance()[1] - vb).max() < TOL
    assert res_err(Ea, Eb) > 1e-3                            # the two models are told apart by far more than TOL
    # a re-init without the switch drops them
    assert s.set_loo(0) == 0 and s.init(xa, Fa[:, 0].copy()) == 0
    assert s.loo_residuals()[0] == pkg.GSL_EINVAL


def test_routes_without_a_factor_are_unsupported(pkg, orc):
    n, dim = 300, 2
    x = orc.synth_centres(n, dim)
    f = orc.synth_response(x)
    routes = []
    for factor in (0.15, 0.05, 0.02, 0.01):                  # flat covariances: numerically semi-definite K
        flat = model(pkg, "kriging", dim, n, 0.0, eps=factor * orc.gaussian_eps(n, dim))
        assert flat.init(x, f) == 0                          # "no factor" does not fail the init
        routes.append(flat.route())
        st, e = flat.loo_residuals()
        if flat.route() == 8:
            assert st == pkg.GSL_EUNSUP and flat.loo_variance()[0] == pkg.GSL_EUNSUP
        else:
            assert st == 0 and flat.loo_variance()[0] == 0
    print("flat covariances: routes", routes)
    assert 8 in routes
    g = model(pkg, "gaussian", dim, n)
    assert g.set_solver(pkg.capi.SOLVER_PCHOLESKY) == 0
    assert g.init(x, f) == 0 and g.route() == 5
    assert g.loo_residuals()[0] == pkg.GSL_EUNSUP and g.loo_variance()[0] == pkg.GSL_EUNSUP
    # set_rcond with the default solver keeps route 1 and the factor in the lower triangle
    x2, F2, _, E2, v2 = case(orc, "gaussian", dim, n, 0.0)
    rc = model(pkg, "gaussian", dim, n)
    assert rc.set_rcond(1) == 0 and rc.init(x2, F2[:, 0].copy()) == 0 and rc.route() == 1
    st, e = rc.loo_residuals()
    assert st == 0 and res_err(e, E2) < TOL and np.abs(rc.loo_variance()[1] - v2).max() < TOL
