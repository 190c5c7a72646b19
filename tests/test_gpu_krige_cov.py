"""-m gpu: the joint posterior covariance of kriging and conditional simulation (csrc/hip/krige_cov.hip) against the numpy
reference of tests/krige_cov_ref.py.

On every shape used here the reference's two routes (bordered saddle system, Cholesky + Schur complement) agree to
<= 5.3e-14 absolute and its diagonal equals the pointwise variance formula to <= 3.0e-14 (tests/test_krige_cov_api.py prints
the figures of one shape; case() below asserts REF_TOL = 1e-11 on each).  The tolerance is the project's TOL = 1e-10 taken
as ABSOLUTE, the convention of test_gpu_krige_variance.py: the sill is 1.  The covariance of the targets alone has its
smallest eigenvalue >= 3e-5 on every shape, and numpy's Cholesky passes at jitter 0.

Targets are synth_targets(0, m, dim) followed by the first 20 data sites.  The shapes are the smallest that cross a
128-column block edge of the output (130, 200 targets), a 64-row edge (65) and a single row (1)."""
import numpy as np
import pytest

import krige_cov_ref as kc
import ukrige_ref as ref
from gpu_util import Canaried, bits, dev, ptr

pytestmark = pytest.mark.gpu
TOL = kc.TOL
N_SITES = 20
SIGMA2 = 2.5

SHAPES = [
    ("kriging", 2, 700, 65, 0.0, 0),
    ("kriging", 2, 129, 1, 1e-3, 0),
    ("kriging", 2, 384, 130, 1e-3, 0),
    ("kriging", 1, 300, 65, 0.0, 0),
    ("kriging_matern52", 2, 700, 130, 0.0, 1),
    ("kriging_matern32", 3, 400, 65, 1e-3, 2),
    ("kriging_matern52", 2, 100, 200, 0.0, 2),
    ("kriging", 3, 1200, 65, 1e-2, 1),
]
NUGGET_FREE = [s for s in SHAPES if s[4] == 0.0]

_cases = {}


class Case:
    pass


def case(orc, name, dim, n, m, nugget, order):
    """centres, response, targets and the checked numpy reference of one shape: computed once, shared, left unchanged"""
    key = (name, dim, n, m, nugget, order)
    if key not in _cases:
        c = Case()
        kind = ref.KIND[name]
        c.x = orc.synth_centres(n, dim)
        c.f = orc.synth_response(c.x) + 3.0
        c.y = np.ascontiguousarray(np.vstack([orc.synth_targets(0, m, dim), c.x[:N_SITES]]))
        c.m = m
        c.model = kc.CovModel(kind, ref.default_eps(kind, n, dim), nugget, order, c.x, c.f)
        c.defect = c.model.check(c.y)                                # asserts REF_TOL
        c.cov = c.model.covariance(c.y)                              # (m + 20)^2, the bordered route
        c.var = c.model.variance(c.y)
        for a in (c.x, c.f, c.y, c.cov, c.var):
            a.setflags(write=False)
        _cases[key] = c
    return _cases[key]


def model(pkg, name, dim, n, nugget, order, variance=True, devices=None, neighbours=0):
    s = pkg.Sinterp(name, dim, n, 0)
    if devices is not None:
        assert s.set_device_list(devices) == 0
    assert s.set_nugget(nugget) == 0 and s.set_drift(order) == 0
    if variance:
        assert s.set_variance(1) == 0
    if neighbours:
        assert s.set_neighbours(neighbours) == 0
    return s


def ready(pkg, orc, shape):
    name, dim, n, m, nugget, order = shape
    c = case(orc, *shape)
    s = model(pkg, name, dim, n, nugget, order)
    assert s.init(c.x, c.f) == 0 and s.route() == (12 if order else 7)
    return c, s


def symmetric_to_the_bit(a):
    return np.array_equal(bits(a), bits(a.T))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(str(v) for v in s))
def test_covariance_matches_the_reference(pkg, orc, shape):
    name, dim, n, m, nugget, order = shape
    c, s = ready(pkg, orc, shape)
    y, mt = c.y, len(c.y)
    # one set: symmetric to the bit, the diagonal is the variance
    st, got = s.eval_covariance_many(y)
    err = np.abs(got - c.cov).max()
    stv, var = s.eval_variance_many(y)
    ed = np.abs(np.diag(got) - var).max()
    print(f"{shape}: reference defect {c.defect[0]:.2e} / {c.defect[1]:.2e}; max |got - want| = {err:.3e}, diagonal against eval_variance_many "
          f"{ed:.3e}, min diagonal {np.diag(got).min():.3e}")
    assert st == 0 and stv == 0
    assert err < TOL and symmetric_to_the_bit(got)
    assert ed < TOL and np.abs(np.diag(got) - c.var).max() < TOL
    if nugget == 0.0:
        assert np.abs(got[-N_SITES:, :]).max() < TOL                  # the field is known at the data sites
    # the m targets alone: exactly 65 / 130 / 200 rows, exactly one row
    st, alone = s.eval_covariance_many(y[:m])
    ea = np.abs(alone - c.cov[:m, :m]).max()
    assert st == 0 and ea < TOL and symmetric_to_the_bit(alone)
    # two sets: a block and its transpose
    st, blk = s.eval_covariance_many(y[:3], y)
    st2, blk_t = s.eval_covariance_many(y, y[:3])
    eb, et = np.abs(blk - c.cov[:3]).max(), np.abs(blk_t - c.cov[:, :3]).max()
    print(f"   targets alone {ea:.3e}, 3 x {mt} block {eb:.3e}, its transpose {et:.3e}")
    assert st == 0 and st2 == 0 and eb < TOL and et < TOL
    # resident, ctda = mb + 3: the padding is left alone (one set: an odd or even pitch by the shape; two sets)
    d_y = dev(y)
    for rows_b in (None, mt):
        ma = mt if rows_b is None else 3
        d_cov = Canaried(np.zeros((ma, mt)), ld=mt + 3)
        assert s.eval_covariance_resident(ptr(d_y), ma, dim, None if rows_b is None else ptr(d_y), mt, dim, d_cov.ptr, mt + 3) == 0
        res = d_cov.get()
        assert d_cov.padding_intact()
        assert np.abs(res - c.cov[:ma]).max() < TOL
        if rows_b is None:
            assert symmetric_to_the_bit(res)
    # a NaN coordinate: NaN in that target's row and column, no error, the rest as before
    bad = y.copy()
    bad[2, dim - 1] = np.nan
    st, gn = s.eval_covariance_many(bad)
    keep = np.arange(mt) != 2
    assert st == 0 and np.isnan(gn[2]).all() and np.isnan(gn[:, 2]).all()
    assert np.abs(gn[np.ix_(keep, keep)] - c.cov[np.ix_(keep, keep)]).max() < TOL


def test_raw_entry_strided(pkg, orc):
    """ordinary kriging as q = 1 through the raw entry, strided x, y and L, an 8-byte aligned output with an odd pitch"""
    shape = SHAPES[0]
    name, dim, n, m, nugget, order = shape
    c = case(orc, *shape)
    kind, eps = ref.KIND[name], c.model.eps
    mt = len(c.y)
    ctx = pkg.HipContext.on_torch_stream(0)
    xtda, ytda, lda = dim + 1, dim + 2, n + 6
    d_x, d_y = Canaried(c.x, ld=xtda), Canaried(c.y, ld=ytda)
    d_phi = Canaried(np.zeros((n, n)), ld=lda)
    d_w = dev(c.f)
    st, route, _ = ctx.krige_solve(kind, eps, nugget, d_x.ptr, n, dim, xtda, d_phi.ptr, lda, ptr(d_w))
    assert st == 0 and route == 7                                    # L is in the lower triangle of d_phi now
    d_b, d_dinv = dev(np.zeros(n)), dev(np.zeros((n + 31) // 32 * 1024))
    st, denom = ctx.krige_variance_prepare(n, d_phi.ptr, lda, ptr(d_b), ptr(d_dinv))
    assert st == 0 and denom > 0.0
    L1 = np.array([np.sqrt(denom)])
    for ma, yb, off in ((mt, False, 1), (mt, False, 0), (3, True, 1)):
        mb = mt
        work = pkg.HipContext.krige_covariance_work(n, ma, mb if yb else 0, 1)
        d_work = dev(np.full(work, np.nan))
        d_cov = Canaried(np.zeros((ma, mb)), ld=mb + 1 + off, off=off)
        st = ctx.krige_covariance(kind, eps, 0, None, None, d_x.ptr, n, dim, xtda, d_phi.ptr, lda, ptr(d_b), n, ptr(d_dinv), L1, d_y.ptr, ma,
                                  ytda, d_y.ptr if yb else None, mb, ytda, d_cov.ptr, mb + 1 + off, ptr(d_work))
        ctx.sync()
        assert st == 0
        got = d_cov.get()
        err = np.abs(got - c.cov[:ma]).max()
        print(f"raw ma {ma} two sets {yb} offset {off}: max |got - want| = {err:.3e}")
        assert err < TOL and d_cov.padding_intact()
        if not yb:
            assert symmetric_to_the_bit(got)
    assert d_x.padding_intact() and d_y.padding_intact() and d_phi.padding_intact()
    # the argument checks of the raw entry
    p = ptr(d_work)
    args = dict(kind=kind, eps=eps, order=0, shift=None, scale=None, d_x=p, n=8, dim=2, xtda=2, d_llt=p, lda=8, d_B=p, ldb=8, d_dinv=p, L=L1,
                d_ya=p, ma=4, yatda=2, d_yb=None, mb=0, ybtda=0, d_cov=p, ctda=4, d_work=p)
    call = lambda **kw: ctx.krige_covariance(**{**args, **kw})
    EINVAL, EFAULT = pkg.GSL_EINVAL, pkg.capi.GSL_EFAULT
    assert call(dim=4) == EINVAL and call(kind=1) == EINVAL and call(order=3) == EINVAL and call(lda=7) == EINVAL and call(ldb=7) == EINVAL
    assert call(ctda=3) == EINVAL and call(d_yb=p, mb=5, ybtda=2, ctda=4) == EINVAL and call(d_yb=p, mb=4, ybtda=1) == EINVAL
    assert call(order=1) == EFAULT and call(L=None) == EFAULT and call(d_work=None) == EFAULT and call(d_dinv=None) == EFAULT
    assert call(ma=0, d_ya=None, d_cov=None) == 0 and call(d_yb=p, mb=0, ybtda=2, d_cov=None) == 0      # nothing to do: nothing launched
    ctx.close()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(str(v) for v in s))
def test_simulate_the_targets_alone(pkg, orc, shape):
    name, dim, n, m, nugget, order = shape
    c, s = ready(pkg, orc, shape)
    y, want = np.ascontiguousarray(c.y[:m]), c.cov[:m, :m]
    st, mean, _ = s.eval_many(y)
    assert st == 0
    # Zn = I: the factor itself
    st, out = s.simulate_many(y, SIGMA2, 0.0, np.eye(m))
    assert st == 0
    A = (out - mean[:, None]) / np.sqrt(SIGMA2)
    ea = np.abs(A @ A.T - want).max()
    print(f"{shape}: max |A A^T - Sigma_ref| = {ea:.3e}, max strict upper {np.abs(np.triu(A, 1)).max():.1e}")
    assert np.abs(np.triu(A, 1)).max() == 0.0                        # value i depends on the normals 0 .. i only
    assert ea < TOL
    # zeros, a fixed vector, the same vector
    z = np.cos(1.0 + 0.7 * np.arange(m))
    zn = np.ascontiguousarray(np.column_stack([np.zeros(m), z, z]))
    st, out = s.simulate_many(y, SIGMA2, 0.0, zn)
    ref_out = c.model.simulate(y, SIGMA2, 0.0, zn, cov=want)
    e1 = np.abs(out[:, 1] - ref_out[:, 1]).max()
    print(f"   draw against the reference: {e1:.3e} (bound {TOL * (1.0 + np.linalg.norm(z)):.3e})")
    assert st == 0
    assert np.array_equal(bits(out[:, 0]), bits(mean))               # the bits of eval_many
    assert np.array_equal(bits(out[:, 1]), bits(out[:, 2]))
    assert e1 < TOL * (1.0 + np.linalg.norm(z))
    # resident, strided normals and draws: the same bits, the padding left alone
    d_y, d_zn, d_out = dev(y), Canaried(zn, ld=5), Canaried(np.zeros((m, 3)), ld=4)
    assert s.simulate_resident(ptr(d_y), m, dim, SIGMA2, 0.0, d_zn.ptr, 5, 3, d_out.ptr, 4) == 0
    assert np.array_equal(bits(d_out.get()), bits(out)) and d_out.padding_intact() and d_zn.padding_intact()


@pytest.mark.parametrize("shape", NUGGET_FREE, ids=lambda s: "-".join(str(v) for v in s))
def test_simulate_through_the_data_sites(pkg, orc, shape):
    """the 20 sites appended, nugget 0: Sigma is singular there.  At jitter 0 the pivot is rounding residue, so neither
    status is asserted; at jitter 1e-10 the draws pass through the data: row i of A has |a_i|^2 = Sigma_ii + jitter <= TOL +
    jitter at a site, so |Out - f| <= sqrt(sigma2 (TOL + jitter)) |z|_2 + TOL max|f| (Cauchy-Schwarz; the mean's own TOL)."""
    name, dim, n, m, nugget, order = shape
    c, s = ready(pkg, orc, shape)
    y, mt = c.y, len(c.y)
    z = np.sin(0.3 + 1.1 * np.arange(mt))
    zn = np.ascontiguousarray(np.column_stack([z, -0.5 * z]))
    with pkg.capi.ErrorCalls() as calls:
        st, out = s.simulate_many(y, SIGMA2, 0.0, zn)
    print(f"{shape}: jitter 0 answers {st}")
    assert st in (0, pkg.GSL_EDOM)
    if st == pkg.GSL_EDOM:
        assert np.isnan(out).all() and [k[1] for k in calls] == [pkg.GSL_EDOM] and "jitter" in calls[0][0]
    else:
        assert len(calls) == 0
    jitter = 1e-10
    with pkg.capi.ErrorCalls() as calls:
        st, out = s.simulate_many(y, SIGMA2, jitter, zn)
    assert st == 0 and len(calls) == 0 and np.isfinite(out).all()
    fmax = np.abs(c.f).max()
    for col, zc in ((0, z), (1, -0.5 * z)):
        miss = np.abs(out[-N_SITES:, col] - c.f[:N_SITES]).max()
        bound = np.sqrt(SIGMA2 * (TOL + jitter)) * np.linalg.norm(zc) + TOL * fmax
        print(f"   jitter {jitter}: max |Out - f| at the sites = {miss:.3e} (bound {bound:.3e})")
        assert miss <= bound


def test_existing_entries_keep_their_bits(pkg, orc):
    """the workspace is shared with the variance entries: value and variance before and after a covariance and a simulation"""
    for shape in (SHAPES[2], SHAPES[4]):
        name, dim, n, m, nugget, order = shape
        c, s = ready(pkg, orc, shape)
        y = c.y
        st0, v0 = s.eval_variance_many(y)
        st1, s0, _ = s.eval_many(y)
        assert st0 == 0 and st1 == 0
        assert s.eval_covariance_many(y)[0] == 0 and s.eval_covariance_many(y[:3], y)[0] == 0
        assert s.simulate_many(y[:m], SIGMA2, 1e-10, np.ones((m, 2)))[0] == 0
        st0, v1 = s.eval_variance_many(y)
        st1, s1, _ = s.eval_many(y)
        assert st0 == 0 and st1 == 0
        assert np.array_equal(bits(v0), bits(v1)) and np.array_equal(bits(s0), bits(s1))
        # ... and a model that never saw the new entries agrees with both
        fresh = model(pkg, name, dim, n, nugget, order)
        assert fresh.init(c.x, c.f) == 0
        assert np.array_equal(bits(fresh.eval_variance_many(y)[1]), bits(v0)) and np.array_equal(bits(fresh.eval_many(y)[1]), bits(s0))


def test_status_codes(pkg, orc, tmp_path):
    shape = SHAPES[2]
    name, dim, n, m, nugget, order = shape
    c, on = ready(pkg, orc, shape)
    y, mt = c.y, len(c.y)
    EINVAL, EUNSUP = pkg.GSL_EINVAL, pkg.capi.GSL_EUNSUP
    zn = np.ones((mt, 2))

    def one_call(fn, status):
        with pkg.capi.ErrorCalls() as calls:
            r = fn()
        st = int(r[0] if isinstance(r, tuple) else r)
        assert st == status and [k[1] for k in calls] == [status], (st, calls)

    # initialised without set_variance
    off = model(pkg, name, dim, n, nugget, order, variance=False)
    assert off.init(c.x, c.f) == 0
    one_call(lambda: off.eval_covariance_many(y), EINVAL)
    one_call(lambda: off.simulate_many(y, 1.0, 0.0, zn), EINVAL)
    # the arguments of an initialised model
    for bad in (0.0, -1.0, np.inf, np.nan):
        one_call(lambda: on.simulate_many(y, bad, 0.0, zn), EINVAL)
    for bad in (-1e-12, np.inf, np.nan):
        one_call(lambda: on.simulate_many(y, 1.0, bad, zn), EINVAL)
    d_y, d_buf = dev(y), Canaried(np.zeros((mt, mt)))
    one_call(lambda: on.eval_covariance_resident(ptr(d_y), mt, dim, None, 0, 0, d_buf.ptr, mt - 1), EINVAL)
    one_call(lambda: on.eval_covariance_resident(ptr(d_y), mt, dim, ptr(d_y), 3, dim, d_buf.ptr, 2), EINVAL)
    one_call(lambda: on.simulate_resident(ptr(d_y), mt, dim, 1.0, 0.0, d_buf.ptr, 1, 2, d_buf.ptr, 2), EINVAL)
    one_call(lambda: on.simulate_resident(ptr(d_y), mt, dim, 1.0, 0.0, d_buf.ptr, 2, 2, d_buf.ptr, 1), EINVAL)
    one_call(lambda: on.eval_covariance_resident(None, mt, dim, None, 0, 0, d_buf.ptr, mt), pkg.capi.GSL_EFAULT)
    one_call(lambda: on.simulate_resident(ptr(d_y), mt, dim, 1.0, 0.0, None, 2, 2, d_buf.ptr, 2), pkg.capi.GSL_EFAULT)
    # no targets: success, nothing written
    with pkg.capi.ErrorCalls() as calls:
        assert on.eval_covariance_resident(None, 0, dim, None, 0, 0, None, 0) == 0
        assert on.eval_covariance_resident(ptr(d_y), 3, dim, ptr(d_y), 0, dim, d_buf.ptr, 0) == 0
        assert on.simulate_resident(None, 0, dim, 1.0, 0.0, None, 2, 2, None, 2) == 0
        assert on.eval_covariance_many(y[:0])[0] == 0 and on.eval_covariance_many(y, y[:0])[0] == 0
        assert on.simulate_many(y[:0], 1.0, 0.0, np.zeros((0, 2)))[0] == 0
    assert len(calls) == 0 and d_buf.padding_intact() and (d_buf.get() == 0.0).all()
    # the local route has no joint model
    loc = model(pkg, name, dim, n, nugget, order, neighbours=16)
    assert loc.init(c.x, c.f) == 0 and loc.route() == 11
    one_call(lambda: loc.eval_covariance_many(y), EUNSUP)
    one_call(lambda: loc.simulate_many(y, 1.0, 0.0, zn), EUNSUP)
    # a device group: the first device does the work
    st, got = on.eval_covariance_many(y)
    grp = model(pkg, name, dim, n, nugget, order, devices=[0, 0, 0])
    assert grp.init(c.x, c.f) == 0
    st2, sharded = grp.eval_covariance_many(y)
    assert st == 0 and st2 == 0 and np.array_equal(bits(sharded), bits(got))
    sts, draws = on.simulate_many(y, 1.0, 0.0, zn)
    sts2, draws2 = grp.simulate_many(y, 1.0, 0.0, zn)
    assert sts == 0 and sts2 == 0 and np.array_equal(bits(draws), bits(draws2))
    # a checkpoint carries no factor
    path = tmp_path / "krige_cov.bin"
    assert on.fwrite(str(path)) == 0
    r = model(pkg, name, dim, n, nugget, order)
    assert r.fread(str(path)) == 0
    one_call(lambda: r.eval_covariance_many(y), EINVAL)
    one_call(lambda: r.simulate_many(y, 1.0, 0.0, zn), EINVAL)


def test_pivoted_route_is_unsupported(pkg, orc):
    n, dim = 300, 2
    x = orc.synth_centres(n, dim)
    f = orc.synth_response(x)
    y = orc.synth_targets(0, 20, dim)
    seen = False
    for factor in (0.15, 0.05, 0.02, 0.01):                                    # flat covariances: numerically semi-definite K
        flat = pkg.Sinterp("kriging", dim, n, 0)
        assert flat.set_nugget(0.0) == 0 and flat.set_shape(factor * orc.gaussian_eps(n, dim)) == 0 and flat.set_variance(1) == 0
        assert flat.init(x, f) == 0
        if flat.route() == 8:
            seen = True
            assert flat.eval_covariance_many(y)[0] == pkg.capi.GSL_EUNSUP
            assert flat.simulate_many(y, 1.0, 1e-10, np.ones((20, 1)))[0] == pkg.capi.GSL_EUNSUP
    assert seen
