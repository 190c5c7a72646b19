"""-m gpu: the kriging variance sigma^2(y) = C(0) - k^T K^-1 k + (1 - b^T k)^2 / (1^T b), b = K^-1 1, evaluated from the
Cholesky factor that the kriging init keeps (csrc/hip/krige_var.hip).

The oracle has no variance, so the reference is the formula in numpy fp64 (np.linalg.solve on K built from the same
phi).  Against an 80-bit long-double Cholesky that reference is within 5.6e-14 absolute on every shape used here (worst:
1-D n = 300 and Wendland n = 700 with nugget 0, cond(K) ~ 1e6; <= 5e-15 elsewhere), so the project's RBF tolerance
TOL = 1e-10 is taken as an ABSOLUTE bound: the sill is 1 and relative error means nothing where sigma^2 -> 0.

Targets are always synth_targets(0, m, dim) followed by the first 20 data sites."""
import numpy as np
import pytest

from gpu_util import Canaried, bits, dev, ptr

pytestmark = pytest.mark.gpu
TOL = 1e-10
GAUSSIAN, WENDLAND = 0, 2
N_SITES = 20


def phi(kind, eps, r):
    if kind == GAUSSIAN:
        return np.exp(-(eps * r) ** 2)
    t = eps * r
    return np.where(t < 1.0, (1.0 - t) ** 4 * (4.0 * t + 1.0), 0.0)


def dist(a, b):
    return np.sqrt(((a[:, None, :] - b[None, :, :]) ** 2).sum(axis=2))


def reference_variance(kind, eps, nugget, x, y):
    """(variance at the rows of y, 1^T K^-1 1) in numpy fp64"""
    K = phi(kind, eps, dist(x, x)) + nugget * np.eye(len(x))
    k = phi(kind, eps, dist(y, x)).T                        # n x m
    Kik = np.linalg.solve(K, k)
    b = np.linalg.solve(K, np.ones(len(x)))
    return 1.0 - (k * Kik).sum(axis=0) + (1.0 - b @ k) ** 2 / b.sum(), b.sum()


_cases = {}


def case(orc, kind, dim, n, m, nugget, eps=None, first=0):
    """centres, response, targets and the numpy reference of one shape: computed once, shared, left unchanged"""
    key = (kind, dim, n, m, nugget, eps, first)
    if key not in _cases:
        x = orc.synth_centres(first + n, dim)[first:].copy()
        f = orc.synth_response(x) + 3.0 + first
        e = orc.gaussian_eps(n, dim) if eps is None else eps
        y = np.ascontiguousarray(np.vstack([orc.synth_targets(0, m, dim), x[:N_SITES]]))
        want, denom = reference_variance(kind, e, nugget, x, y)
        for a in (x, f, y, want):
            a.setflags(write=False)
        _cases[key] = (x, f, y, e, want, denom)
    return _cases[key]


def krige(pkg, dim, n, nugget, variance=True, eps=None, devices=None):
    s = pkg.Sinterp("kriging", dim, n, 0)
    if devices is not None:
        assert s.set_device_list(devices) == 0
    assert s.set_nugget(nugget) == 0
    if eps is not None:
        assert s.set_shape(eps) == 0
    if variance:
        assert s.set_variance(1) == 0
    return s


@pytest.mark.parametrize("dim,n,m,nugget", [
    (2, 700, 300, 0.0),       # tail block of 60 columns
    (2, 384, 300, 1e-3),      # exactly 3 blocks
    (3, 1200, 300, 1e-2),
    (1, 300, 300, 0.0),       # worst conditioning
    (2, 100, 65, 1e-3),       # one partial block; 64 + 1 rows
    (2, 129, 1, 1e-3),        # one block + 1 column; a single target
])
def test_facade_matches_the_formula(pkg, orc, dim, n, m, nugget):
    x, f, y, eps, want, denom = case(orc, GAUSSIAN, dim, n, m, nugget)
    s = krige(pkg, dim, n, nugget)
    assert s.init(x, f) == 0 and s.route() == 7
    st, got = s.eval_variance_many(y)
    assert st == 0
    err = np.abs(got - want).max()
    print(f"dim {dim} n {n} m {m} nugget {nugget}: max |got - want| = {err:.3e}, min got = {got.min():.3e}")
    assert err < TOL
    assert (got >= 0.0).all()
    if nugget == 0.0:
        assert np.abs(got[-N_SITES:]).max() < TOL          # the field is known at the data sites
    # the m targets alone (without the appended sites: exactly 65 rows, exactly one row)
    st, alone = s.eval_variance_many(y[:m])
    assert st == 0 and np.abs(alone - want[:m]).max() < TOL
    # far field: every covariance term is exactly 0, sigma^2 = 1 + 1 / (1^T K^-1 1)
    st, far = s.eval_variance_many(np.full((3, dim), 50.0))
    assert st == 0
    assert np.abs(far - (1.0 + 1.0 / denom)).max() <= 1e-12 * (1.0 + 1.0 / denom)


def raw_variance(pkg, orc, kind, n, m, nugget, eps):
    dim = 2
    x, f, y, eps, want, denom = case(orc, kind, dim, n, m, nugget, eps)
    mt = len(y)
    ctx = pkg.HipContext.on_torch_stream(0)
    xtda, ytda, lda = dim + 1, dim + 2, n + 6
    d_x, d_y = Canaried(x, ld=xtda), Canaried(y, ld=ytda)
    d_phi = Canaried(np.zeros((n, n)), ld=lda)
    d_w = dev(f)
    st, route, _ = ctx.krige_solve(kind, eps, nugget, d_x.ptr, n, dim, xtda, d_phi.ptr, lda, ptr(d_w))
    assert st == 0 and route == 7                            # L is in the lower triangle of d_phi now
    d_b = dev(np.zeros(n))
    d_dinv = dev(np.zeros((n + 31) // 32 * 1024))
    st, got_denom = ctx.krige_variance_prepare(n, d_phi.ptr, lda, ptr(d_b), ptr(d_dinv))
    assert st == 0 and abs(got_denom - denom) <= 1e-9 * abs(denom)
    out = {}
    # mt = 320 rows: five full passes of 64 / a pass of 192 and a shorter one of 128 (the padded height changes between
    # the passes) / one pass
    for chunk in (64, 192, 4096):
        work = pkg.HipContext.krige_variance_work(n, chunk)
        assert work >= n * chunk
        d_work = dev(np.full(work, np.nan))
        d_var = Canaried(np.zeros(mt))
        st = ctx.krige_variance(kind, eps, d_x.ptr, n, dim, xtda, d_phi.ptr, lda, ptr(d_b), ptr(d_dinv), got_denom,
                                d_y.ptr, mt, ytda, d_var.ptr, ptr(d_work), chunk)
        ctx.sync()
        assert st == 0
        got = d_var.get()
        err = np.abs(got - want).max()
        print(f"raw kind {kind} n {n} chunk {chunk}: max |got - want| = {err:.3e}, min got = {got.min():.3e}")
        assert err < TOL
        if nugget == 0.0:
            assert np.abs(got[-N_SITES:]).max() < TOL        # rounding residue of either sign: the raw entry does not clamp
        assert d_var.padding_intact()
        out[chunk] = got
    assert d_x.padding_intact() and d_y.padding_intact() and d_phi.padding_intact()
    assert max(np.abs(out[64] - out[4096]).max(), np.abs(out[192] - out[4096]).max()) < 2 * TOL       # not bit equal: the GEMM dispatch depends on the pass height
    ctx.close()


def test_raw_entry_strided_and_chunked(pkg, orc):
    raw_variance(pkg, orc, GAUSSIAN, 700, 300, 0.0, None)


def test_raw_entry_wendland(pkg, orc):
    n, dim = 384, 2
    raw_variance(pkg, orc, WENDLAND, n, 300, 1e-3, n ** (1.0 / dim) / 8.0)


def test_raw_entry_argument_checks(pkg):
    ctx = pkg.HipContext.on_torch_stream(0)
    buf = dev(np.zeros(4096))
    p = ptr(buf)
    args = dict(kind=GAUSSIAN, eps=1.0, d_x=p, n=8, dim=2, xtda=2, d_llt=p, lda=8, d_b=p, d_dinv=p, denom=1.0, d_y=p, m=4, ytda=2,
                d_var=p, d_work=p, chunk=4)
    call = lambda **kw: ctx.krige_variance(**{**args, **kw})
    assert call(dim=4) == pkg.GSL_EINVAL and call(dim=0) == pkg.GSL_EINVAL
    assert call(kind=1) == pkg.GSL_EINVAL                    # thin-plate spline: not a covariance
    assert call(lda=7) == pkg.GSL_EINVAL and call(chunk=0) == pkg.GSL_EINVAL
    assert call(d_llt=None) == pkg.capi.GSL_EFAULT and call(d_work=None) == pkg.capi.GSL_EFAULT
    assert call(m=0, d_y=None, d_var=None) == 0 and call(n=0, d_x=None) == 0      # nothing to do: nothing launched
    ctx.close()


def test_status_codes(pkg, orc, tmp_path):
    dim, n, m, nugget = 2, 384, 300, 1e-3
    x, f, y, eps, want, _ = case(orc, GAUSSIAN, dim, n, m, nugget)
    g = pkg.Sinterp("gaussian", dim, n, 0)
    assert g.set_variance(1) == pkg.GSL_EINVAL               # kriging interpolants only
    off = krige(pkg, dim, n, nugget, variance=False)
    assert off.eval_variance_many(y)[0] == pkg.GSL_EINVAL    # not initialised
    assert off.init(x, f) == 0
    assert off.eval_variance_many(y)[0] == pkg.GSL_EINVAL    # initialised without set_variance
    on = krige(pkg, dim, n, nugget)
    assert on.init(x, f) == 0
    st, got = on.eval_variance_many(y)
    assert st == 0 and np.abs(got - want).max() < TOL
    # the predictor does not notice the kept factor
    assert np.array_equal(bits(on.eval_many(y)[1]), bits(off.eval_many(y)[1]))
    # a checkpoint carries no factor
    path = tmp_path / "krige_var.bin"
    assert on.fwrite(str(path)) == 0
    r = krige(pkg, dim, n, nugget)
    assert r.fread(str(path)) == 0
    assert r.eval_variance_many(y)[0] == pkg.GSL_EINVAL
    assert np.array_equal(bits(r.eval_many(y)[1]), bits(on.eval_many(y)[1]))
    # ... and reading one into an interpolant that holds a factor drops that factor
    assert on.fread(str(path)) == 0 and on.eval_variance_many(y)[0] == pkg.GSL_EINVAL
    # a device group: the factor lives on member 0, which evaluates every target
    grp = krige(pkg, dim, n, nugget, devices=[0, 0, 0])
    assert grp.init(x, f) == 0
    st, sharded = grp.eval_variance_many(y)
    assert st == 0 and np.array_equal(bits(sharded), bits(got))


def test_pivoted_route_is_unsupported(pkg, orc):
    n, dim = 300, 2
    x = orc.synth_centres(n, dim)
    f = orc.synth_response(x)
    y = orc.synth_targets(0, 50, dim)
    routes = []
    for factor in (0.15, 0.05, 0.02, 0.01):                  # flat covariances: numerically semi-definite K
        flat = krige(pkg, dim, n, 0.0, eps=factor * orc.gaussian_eps(n, dim))
        assert flat.init(x, f) == 0
        routes.append(flat.route())
        st, v = flat.eval_variance_many(y)
        if flat.route() == 8:
            assert st == pkg.GSL_EUNSUP
        else:
            assert st == 0 and np.isfinite(v).all()
    print("flat covariances: routes", routes)
    assert 8 in routes


def test_reinit_replaces_the_kept_factor(pkg, orc):
    dim, n, m, nugget = 2, 300, 100, 1e-3
    xa, fa, ya, _, want_a, _ = case(orc, GAUSSIAN, dim, n, m, nugget)
    xb, fb, yb, _, want_b, _ = case(orc, GAUSSIAN, dim, n, m, nugget, first=n)     # other sites AND other values
    assert not np.array_equal(xa, xb)
    s = krige(pkg, dim, n, nugget)
    assert s.init(xa, fa) == 0
    st, got = s.eval_variance_many(ya)
    assert st == 0 and np.abs(got - want_a).max() < TOL
    assert s.init(xb, fb) == 0
    st, got = s.eval_variance_many(yb)
    assert st == 0 and np.abs(got - want_b).max() < TOL
    assert np.abs(want_a - want_b).max() > 1e-3              # the two models are told apart by far more than TOL


def test_single_target_entry_and_resident(pkg, orc):
    dim, n, m, nugget = 2, 384, 300, 1e-3
    x, f, y, eps, want, _ = case(orc, GAUSSIAN, dim, n, m, nugget)
    s = krige(pkg, dim, n, nugget)
    assert s.init(x, f) == 0
    st, many = s.eval_variance_many(y)
    st1, one = s.eval_variance_e(y[0])
    assert st == 0 and st1 == 0
    # the single-target entry is the batch entry at m = 1: bit for bit the value of a one-row batch, and within TOL of the
    # reference.  Row 0 of a LARGER batch agrees to rounding only (each is within TOL of the reference, hence within 2 TOL
    # of the other): its updates run at another height, and the stream-K GEMM splits K by the tile count.
    st0, row = s.eval_variance_many(y[:1])
    assert st0 == 0 and np.array_equal(bits(np.array([one])), bits(row))
    assert abs(one - want[0]) < TOL and abs(one - many[0]) < 2 * TOL
    d_y, d_v = dev(y), dev(np.zeros(len(y)))
    assert s.eval_variance_resident(ptr(d_y), len(y), dim, ptr(d_v)) == 0
    assert np.array_equal(bits(d_v.cpu().numpy()), bits(many))
