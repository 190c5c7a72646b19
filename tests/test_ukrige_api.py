"""Universal kriging (gsl_sinterp_set_drift) where it answers without a GPU: which types take the switch, its argument
errors, the number of drift functions, the refusals that hold with a drift, the checkpoint header, the argument checks of
the raw entries (decided before anything touches the device), and the numpy reference of tests/ukrige_ref.py against
itself (its two routes, Dubrule's rule with a drift against explicit deletion)."""
import struct

import numpy as np
import pytest

import ukrige_ref as ref

KRIGING = ("kriging", "kriging_matern32", "kriging_matern52")
DRIFT_ID = {"kriging": 17, "kriging_matern32": 18, "kriging_matern52": 19}
PLAIN_ID = {"kriging": 4, "kriging_matern32": 10, "kriging_matern52": 11}


def test_set_drift_is_for_the_kriging_types(pkg):
    for kind in pkg.Sinterp.TYPES:
        s = pkg.Sinterp(kind, 2, 100)
        assert s.drift() == 0                                         # the default: ordinary kriging
        for order in (1, 2, 0):
            st = s.set_drift(order)
            if kind in KRIGING:
                assert st == 0 and s.drift() == order, kind
            else:
                assert st == pkg.GSL_EINVAL and s.drift() == 0, kind
        s.close()
    assert pkg.lib().gsl_sinterp_set_drift(None, 1) == pkg.capi.GSL_EFAULT
    assert pkg.lib().gsl_sinterp_drift(None) == 0


@pytest.mark.parametrize("kind", KRIGING)
def test_orders_outside_0_to_2_are_invalid(pkg, kind):
    s = pkg.Sinterp(kind, 3, 50)
    assert s.set_drift(2) == 0
    for order in (-1, 3):
        assert s.set_drift(order) == pkg.GSL_EINVAL and s.drift() == 2   # the order in force stays


def test_drift_terms(pkg):
    want = {(1, 0): 1, (2, 0): 1, (3, 0): 1, (1, 1): 2, (2, 1): 3, (3, 1): 4, (1, 2): 3, (2, 2): 6, (3, 2): 10}
    for (dim, order), q in want.items():
        assert pkg.Sinterp.drift_terms(dim, order) == q == ref.n_terms(dim, order)
        assert pkg.HipContext.drift_terms(dim, order) == q
    for dim, order in ((0, 1), (4, 1), (2, -1), (2, 3)):
        assert pkg.Sinterp.drift_terms(dim, order) == 0 and pkg.HipContext.drift_terms(dim, order) == 0


@pytest.mark.parametrize("kind", KRIGING)
def test_refusals_with_a_drift(pkg, kind):
    s = pkg.Sinterp(kind, 2, 50)
    assert s.mean()[0] == pkg.GSL_EINVAL                              # ordinary, not initialised: the old answer
    assert s.set_drift(1) == 0
    assert s.mean()[0] == pkg.capi.GSL_EUNSUP
    assert s.field_mean(0)[0] == pkg.GSL_EINVAL                       # the field entries look for an initialised field first
    assert s.drift_coefficients()[0] == pkg.GSL_EINVAL               # not initialised
    assert s.set_drift(0) == 0
    assert s.mean()[0] == pkg.GSL_EINVAL
    g = pkg.Sinterp("gaussian", 2, 50)
    assert g.drift_coefficients()[0] == pkg.GSL_EINVAL               # not a kriging interpolant


def test_fewer_sites_than_drift_functions(pkg):
    s = pkg.Sinterp("kriging", 3, 9)                                  # q = 10
    assert s.set_drift(2) == 0
    x = np.random.default_rng(3).random((9, 3))
    assert s.init(x, x[:, 0].copy()) == pkg.GSL_EINVAL
    assert s.route() == 0


@pytest.mark.parametrize("kind", KRIGING)
def test_fread_header_checks(pkg, kind, tmp_path):
    """a hand-written GSLSINT1 header: a kriging interpolant takes its plain id and its drift id (the short payload then
    fails as a read error, GSL_EFAILED), every other id is GSL_EBADLEN"""
    dim, n = 2, 10
    s = pkg.Sinterp(kind, dim, n)
    header = lambda tid, d=dim, size=n: b"GSLSINT1" + struct.pack("<QQQdq", tid, d, size, 1.0, 0)

    def fread(blob):
        path = str(tmp_path / "h.bin")
        with open(path, "wb") as fp:
            fp.write(blob)
        return s.fread(path)

    for tid in range(20):
        want = pkg.capi.GSL_EFAILED if tid in (PLAIN_ID[kind], DRIFT_ID[kind]) else pkg.capi.GSL_EBADLEN
        assert fread(header(tid)) == want, tid
    assert fread(header(DRIFT_ID[kind], d=3)) == pkg.capi.GSL_EBADLEN
    assert fread(header(DRIFT_ID[kind], size=11)) == pkg.capi.GSL_EBADLEN
    # the drift block is validated before anything touches the device: an order outside 1..2 is a corrupt file
    body = np.zeros(n * (dim + 1)).tobytes()
    assert fread(header(DRIFT_ID[kind]) + body + struct.pack("<Q", 3)) == pkg.capi.GSL_EFAILED
    assert fread(header(DRIFT_ID[kind]) + body + struct.pack("<Q", 1) + np.zeros(2 * dim + 2).tobytes()) == pkg.capi.GSL_EFAILED  # one coefficient short
    g = pkg.Sinterp("gaussian", dim, n)                              # the drift ids belong to the kriging types
    path = str(tmp_path / "g.bin")
    with open(path, "wb") as fp:
        fp.write(header(17))
    assert g.fread(path) == pkg.capi.GSL_EBADLEN


def test_raw_entries_check_their_arguments_before_the_device(pkg):
    L, EINVAL, EFAULT = pkg.lib(), pkg.GSL_EINVAL, pkg.capi.GSL_EFAULT
    z = np.zeros(3)
    pd = lambda a: a.ctypes.data_as(pkg.capi._pd)
    # a NULL context is the first thing every entry reports
    assert L.gsl_sinterp_hip_drift_basis(None, 1, pd(z), pd(z), None, 10, 2, 2, None, 10) == EFAULT
    assert L.gsl_sinterp_hip_drift_add(None, 1, pd(z), pd(z), pd(z), 1, None, 1, 2, 2, None, 1, None, 0) == EFAULT
    assert L.gsl_sinterp_hip_ukrige_solve(None, 0, 1.0, 0.0, 1, pd(z), pd(z), None, 10, 2, 2, None, 10, None, 10, 1, pd(z), None, 0, None,
                                          None, None, None) == EFAULT
    assert L.gsl_sinterp_hip_ukrige_variance(None, 0, 1.0, 1, pd(z), pd(z), None, 10, 2, 2, None, 10, None, 10, None, pd(z), None, 1, 2, None,
                                             None, 64) == EFAULT
    assert L.gsl_sinterp_hip_loo_combine_drift(None, 10, 1, None, None, 10, 3, pd(z), None, 10, None, 10, None) == EFAULT
    # the host factor: S = Ls Ls^T, and the pivot rule
    S = np.array([[4.0, 2.0, 0.0], [2.0, 5.0, 1.0], [0.0, 1.0, 3.0]])
    st, Ls = pkg.HipContext.drift_factor(S)
    assert st == 0 and np.abs(Ls @ Ls.T - S).max() < 1e-15 and np.abs(np.triu(Ls, 1)).max() == 0.0
    v = np.array([1.0, 2.0, 3.0])
    st, Ls = pkg.HipContext.drift_factor(np.outer(v, v) + 1e-18 * np.eye(3))      # rank one: the second pivot fails
    assert st == pkg.GSL_EDOM
    assert pkg.HipContext.drift_factor(np.array([[np.nan]]))[0] == pkg.GSL_EDOM
    assert pkg.HipContext.drift_factor(np.array([[0.0]]))[0] == pkg.GSL_EDOM
    assert L.gsl_sinterp_hip_drift_factor(11, pd(z), pd(z)) == EINVAL
    assert L.gsl_sinterp_hip_drift_factor(1, None, pd(z)) == EFAULT
    assert pkg.HipContext.ukrige_variance_work(300, 64, 6) == pkg.HipContext.krige_variance_work(300, 64) + 128 * 6
    for name in ("drift_basis", "ukrige_solve", "drift_add", "ukrige_variance", "ukrige_variance_work", "loo_combine_drift"):
        assert callable(getattr(pkg.HipContext, name)), name


# ---- the reference against itself: the figures every GPU test leans on ----
GLOBAL = [(ref.GAUSSIAN, 2, 700, 0.0, 1), (ref.GAUSSIAN, 2, 384, 1e-3, 2), (ref.GAUSSIAN, 3, 1200, 1e-2, 1), (ref.GAUSSIAN, 1, 300, 0.0, 2),
          (ref.GAUSSIAN, 2, 100, 1e-3, 2), (ref.GAUSSIAN, 2, 129, 1e-3, 1), (ref.MATERN32, 2, 700, 0.0, 2), (ref.MATERN52, 3, 700, 0.0, 2)]
LOO = [(ref.GAUSSIAN, 2, 384, 1e-3, 1), (ref.GAUSSIAN, 3, 300, 1e-2, 2), (ref.GAUSSIAN, 2, 100, 1e-3, 2), (ref.GAUSSIAN, 2, 129, 1e-3, 1),
       (ref.MATERN32, 2, 300, 0.0, 2), (ref.MATERN52, 1, 100, 0.0, 1)]


@pytest.mark.parametrize("kind,dim,n,nugget,order", GLOBAL)
def test_reference_routes_agree(orc, kind, dim, n, nugget, order):
    x = orc.synth_centres(n, dim)
    f = orc.synth_response(x) + 3.0
    y = np.ascontiguousarray(np.vstack([orc.synth_targets(0, 300, dim), x[:20]]))
    m = ref.Model(kind, ref.default_eps(kind, n, dim), nugget, order, x, f)
    ev, es = m.check(y, np.abs(f).max())                              # asserts REF_TOL
    print(f"kind {kind} dim {dim} n {n} nugget {nugget} order {order}: values {ev:.2e}, variances {es:.2e}")
    far = np.full((2, dim), 50.0)
    assert np.abs(m.variance(far, schur=True) - m.far_variance(far)).max() <= 1e-12 * m.far_variance(far).max()


@pytest.mark.parametrize("kind,dim,n,nugget,order", LOO)
def test_reference_dubrule_with_drift_equals_deletion(orc, kind, dim, n, nugget, order):
    x = orc.synth_centres(n, dim)
    f = orc.synth_response(x) + 3.0
    eps = ref.default_eps(kind, n, dim)
    E, v = ref.loo_by_deletion(kind, eps, nugget, order, x, f)
    E2, v2 = ref.loo_by_identity(kind, eps, nugget, order, x, f)
    ee, ev = np.abs(E - E2).max() / np.abs(E).max(), (np.abs(v - v2) / np.maximum(1.0, np.abs(v))).max()
    print(f"kind {kind} dim {dim} n {n} nugget {nugget} order {order}: residuals {ee:.2e}, variances {ev:.2e}")
    assert ee < ref.REF_TOL and ev < ref.REF_TOL


@pytest.mark.parametrize("kind,dim,k", [(ref.MATERN32, 2, 16), (ref.MATERN32, 2, 4), (ref.MATERN32, 2, 5), (ref.MATERN52, 3, 32), (ref.MATERN52, 3, 5),
                                        (ref.GAUSSIAN, 2, 64)])
def test_reference_local_routes_agree(kind, dim, k):
    """local universal kriging, N = 5000, k = dim + 2 included: bordered system against Cholesky + Schur complement"""
    n, m = 5000, 400
    rng = np.random.default_rng(20261020 + 7 * dim + k)
    x, y = rng.random((n, dim)), rng.random((m, dim))
    f = 2.0 + np.sin(3.0 * x[:, 0]) + np.cos(2.0 * x[:, -1])
    idx = np.argsort(ref.dist(y, x), axis=1, kind="stable")[:, :k]
    nugget = 1e-3 if kind == ref.GAUSSIAN else 0.0
    _, _, es, ev = ref.local_ukrige(kind, ref.default_eps(kind, n, dim), nugget, x, f, y, idx)     # asserts REF_TOL
    print(f"kind {kind} dim {dim} k {k}: values {es.max():.2e}, variances {ev.max():.2e}")


def test_local_route_refusals(pkg):
    s = pkg.Sinterp("kriging_matern32", 2, 50)
    x = np.random.default_rng(2).random((50, 2))
    f = x[:, 0].copy()
    assert s.set_drift(2) == 0 and s.set_neighbours(16) == 0
    assert s.init(x, f) == pkg.capi.GSL_EUNSUP                       # a quadratic drift on the local route
    assert s.set_drift(1) == 0 and s.set_neighbours(3) == 0
    assert s.init(x, f) == pkg.GSL_EINVAL                            # k < dim + 2
    assert s.route() == 0
    assert s.set_neighbours(4) == 0 and s.drift_coefficients()[0] == pkg.capi.GSL_EUNSUP
    L, EINVAL, EFAULT = pkg.lib(), pkg.GSL_EINVAL, pkg.capi.GSL_EFAULT
    raw = lambda kind=4, eps=1.0, nugget=0.0, n=100, dim=2, k=8: L.gsl_sinterp_hip_local_ukrige(None, kind, eps, nugget, None, n, dim, dim, None,
                                                                                                None, 1, dim, k, None, None, None, None, 0)
    assert raw() == EFAULT
    for dim in (1, 2, 3):
        assert raw(dim=dim, k=dim + 1) == EINVAL and raw(dim=dim, k=dim + 2) == EFAULT
    assert raw(k=65, n=1000) == EINVAL and raw(k=101) == EINVAL and raw(dim=4) == EINVAL and raw(kind=1) == EINVAL
    assert raw(nugget=-1.0) == EINVAL and raw(eps=0.0) == EINVAL
    assert callable(pkg.HipContext.local_ukrige)
