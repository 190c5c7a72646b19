"""The extended-precision references of tests/tiny_ref.py against closed forms, and the inputs of
tests/test_gpu_tiny_models.py against the rules that make 1e-10 attainable there.  No GPU, no project code.

Closed forms:
    N = 1, positive definite kernel     w = f / phi(0), s(y) = w phi(|y - x|)
    N = 1, kriging                      s = f everywhere; sigma^2(y) = 2 (1 - phi(|y - x|))
    N = q, universal kriging            w = 0 and s is the polynomial through the q sites
    N = 2, thin-plate spline            [0 a; a 0] w = f:  w = (f_2, f_1) / a,  a = r^2 ln r
    affine thin-plate, affine data      w = 0 and the plane
    leave-one-out at N = 2              the other datum's prediction: f_1 - f_2 phi(r) / phi(0); kriging: f_1 - f_2

Inputs: every (type, dim, N, drift) of tiny_ref.small_cases() / edge_cases() / local_cases() has a system matrix of fp64
condition number <= 1e4, so that cond * 2^-52 ~ 2e-12 leaves 1e-10 attainable, and no k = N - 1 neighbourhood is decided by
less than the 1e-9 relative gap of tests/test_gpu_local.py."""
import mpmath as mp
import numpy as np
import pytest

import tiny_ref as T
import ukrige_ref

PD_KINDS = (T.GAUSSIAN, T.WENDLAND, T.MATERN32, T.MATERN52, T.IMQ)
FAR = np.array([[7.0, -3.0, 5.0], [-4.0, 9.0, 2.5]])


def test_kernels_at_zero_and_their_derivatives():
    for kind in range(6):
        assert T.phi(kind, 1.7, 0) == (0 if kind == T.TPS else 1)
        for r in (0.05, 0.3, 0.9):                              # psi r = phi'(r), by mpmath's own differentiation
            want = mp.diff(lambda t: T.phi(kind, 1.7 if kind != T.WENDLAND else 0.6, t), r)
            got = T.psi(kind, 1.7 if kind != T.WENDLAND else 0.6, r) * r
            assert abs(got - want) < mp.mpf(10) ** -30, (kind, r)
            assert abs(float(T.phi(kind, 1.7, r)) - T.np_phi(kind, 1.7, np.array(r))) < 1e-15
    assert T.phi(T.WENDLAND, 2.0, 0.5) == 0 and T.psi(T.WENDLAND, 2.0, 0.75) == 0


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_one_site_rbf(dim):
    x, f = np.full((1, dim), 0.3), np.array([1.75])
    y = np.vstack([x, FAR[:, :dim] * 0.1, np.full((1, dim), 0.35)])
    for kind in PD_KINDS:
        m = T.Model(kind, 1.3, x, f)
        assert m.w[0, 0] == 1.75                                 # phi(0) = 1
        r = np.sqrt(((y - x) ** 2).sum(axis=1))
        assert np.allclose(m.values(y)[:, 0], 1.75 * T.np_phi(kind, 1.3, r), rtol=1e-14, atol=0)


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_one_site_kriging_is_the_datum(dim):
    x, f = np.full((1, dim), 0.3), np.array([1.75])
    y = np.vstack([x, FAR[:, :dim] * 0.1])
    for kind in (T.GAUSSIAN, T.MATERN32, T.MATERN52):
        m = T.Model(kind, 1.3, x, f, tail=0)
        assert m.w[0, 0] == 0.0 and m.c[0, 0] == 1.75
        assert (m.values(y) == 1.75).all() and (m.gradient(y) == 0.0).all()
        k = T.np_phi(kind, 1.3, np.sqrt(((y - x) ** 2).sum(axis=1)))
        assert np.allclose(m.variance(y), 2.0 * (1.0 - k), rtol=1e-14, atol=1e-16) and m.variance(y)[0] == 0.0


@pytest.mark.parametrize("dim,order", [(1, 1), (2, 1), (3, 1), (1, 2), (2, 2), (3, 2)])
def test_universal_kriging_on_q_sites_is_the_polynomial_through_them(dim, order):
    q = ukrige_ref.n_terms(dim, order)
    x, F, _ = T.cloud(dim, q)
    f = F[:, 3]                                                  # no polynomial
    m = T.Model(T.MATERN32, T.default_eps(T.MATERN32, q, dim), x, f, tail=order)
    assert np.abs(m.w).max() < 1e-40
    shift, scale = ukrige_ref.geometry(x)
    c = np.linalg.solve(ukrige_ref.basis(x, shift, scale, order)[0], f)
    y = np.vstack([FAR[:, :dim], x])
    want = ukrige_ref.basis(y, shift, scale, order)[0] @ c
    got = m.values(y)[:, 0]
    assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()     # the fp64 polynomial, cond <= 1e4
    assert np.abs(got[2:] - f).max() < 1e-15


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_two_site_thin_plate(dim):
    x = np.zeros((2, dim))
    x[1, 0], f = 0.5, np.array([1.25, -0.75])
    a = float(mp.mpf("0.25") * mp.log(mp.mpf("0.5")))
    m = T.Model(T.TPS, 1.0, x, f)
    assert np.allclose(m.w[:, 0], [f[1] / a, f[0] / a], rtol=1e-15, atol=0)
    assert np.abs(m.values(x)[:, 0] - f).max() < 1e-15


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_affine_thin_plate_on_affine_data(dim):
    n = dim + 4
    x, _, y = T.cloud(dim, n)
    coef = np.array([1.5, 2.0, -5.0, 0.25])[:dim + 1]
    m = T.Model(T.TPS, 1.0, x, coef[0] + x @ coef[1:], tail="affine")
    # f itself is rounded to fp64, so w is not 1e-40 but up to cond * 2^-52 * max|f| <= 1e4 * 2.3e-16 * 8
    assert np.abs(m.w).max() < 2e-11 and np.abs(m.c[:, 0] - coef).max() < 1e-13
    ok = y[:-1]
    assert np.abs(m.values(ok)[:, 0] - (coef[0] + ok @ coef[1:])).max() < 1e-13
    assert np.abs(m.gradient(ok)[:, 0, :] - coef[1:]).max() < 1e-13


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_leave_one_out_on_two_sites(dim):
    x, F, _ = T.cloud(dim, 2)
    f = F[:, 0]
    r = np.sqrt(((x[0] - x[1]) ** 2).sum())
    for typ in T.PD_TYPES:
        kind, krige, _ = T.TYPES[typ]
        E, v = T.loo_by_deletion(typ, dim, x, f, nugget=T.nugget_of(typ))
        k = T.np_phi(kind, T.default_eps(kind, 2, dim), r)
        nug = T.nugget_of(typ)
        if krige:
            want_e, want_v = np.array([f[0] - f[1], f[1] - f[0]]), 2.0 * (1.0 - k) + 2.0 * nug
        else:
            want_e, want_v = np.array([f[0] - f[1] * k, f[1] - f[0] * k]), 1.0 - k * k
        assert np.allclose(E[:, 0], want_e, rtol=1e-13, atol=0) and np.allclose(v, want_v, rtol=1e-13, atol=0), typ


def test_the_fp64_twins_and_the_scores_agree_with_extended_precision():
    import test_gpu_fit
    for typ, dim, n, drift in [("matern52", 2, 5, 0), ("tps_affine", 2, 5, 0), ("kriging", 3, 8, 0), ("kriging_matern52", 2, 8, 2),
                               ("kriging_matern32", 1, 4, 1)]:
        x, F, y = T.cloud(dim, n)
        a = T.fit(typ, dim, x, F[:, :2], nugget=T.nugget_of(typ), drift=drift)
        b = T.np_fit(typ, dim, x, F[:, :2], nugget=T.nugget_of(typ), drift=drift)
        assert np.abs(a.values(y[:-1]) - b.values(y[:-1])).max() < 1e-11 and np.abs(a.w - b.w).max() < 1e-11 * np.abs(a.w).max()
        if T.TYPES[typ][1]:
            assert np.abs(a.variance(y[:-1]) - b.variance(y[:-1])).max() < 1e-11
        if typ in T.PD_TYPES and n > ukrige_ref.n_terms(dim, drift):
            (E, v), (E2, v2) = (fn(typ, dim, x, F[:, :2], nugget=T.nugget_of(typ), drift=drift) for fn in (T.loo_by_deletion, T.np_loo_by_deletion))
            assert np.abs(E - E2).max() < 1e-11 * np.abs(E).max() and np.abs(v - v2).max() < 1e-11
        if typ in T.PD_TYPES and not drift:
            eps = T.default_eps(T.TYPES[typ][0], n, dim)
            ml, loo = T.scores(typ, dim, x, F[:, 0], eps, nugget=T.nugget_of(typ))
            ml2, loo2, _, _ = test_gpu_fit.scores(typ, eps, T.nugget_of(typ), ukrige_ref.dist(x, x), F[:, 0])
            assert abs(ml - ml2) < 1e-11 * n and abs(loo - loo2) < 1e-11 * loo


def test_simplex_reference_against_scipy():
    from scipy.interpolate import LinearNDInterpolator
    from scipy.spatial import Delaunay
    for dim, n in ((2, 5), (3, 6)):
        x, F, y = T.cloud(dim, n)
        tri = Delaunay(x)
        S, G, where, margin = T.simplex_linear(x, F[:, :3], tri.simplices.tolist(), y[:-1])
        want = LinearNDInterpolator(tri, F[:, :3])(y[:-1])
        inside = ~np.isnan(want[:, 0])
        assert np.array_equal(inside, where >= 0) and inside.sum() > n
        assert np.abs(S[inside] - want[inside]).max() < 1e-13


# ------------------------------------------------------------------------------------------------- the inputs
def test_size_lists():
    assert T.small_sizes(1) == [1, 2, 3, 4, 5, 8] and T.small_sizes(3) == [3, 4, 5, 6, 7, 8] and T.small_sizes(4) == [4, 5, 6, 7, 8]
    assert T.small_sizes(7) == [7, 8, 9, 10, 11] and T.small_sizes(11) == [11, 12, 13, 14, 15]
    x, F, y = T.cloud(2, 5)
    assert y.shape == (T.M_TARGETS, 2) and np.isnan(y[-1]).all() and np.isfinite(y[:-1]).all() and np.array_equal(y[:5], x)
    outside = ((y[:-1] < 0.0) | (y[:-1] > 1.0)).any(axis=1)
    assert outside.sum() == 10 and np.abs(y[:-1] - 0.5).max() <= 0.6
    assert T.cloud(2, 129)[2].shape == (129 + 51, 2)


@pytest.mark.parametrize("which", ["small", "edge"])
def test_every_system_matrix_is_under_the_cap(which):
    worst = (0.0, None)
    for typ, dim, n, drift in (T.small_cases() if which == "small" else T.edge_cases()):
        x, _, _ = T.cloud(dim, n)
        assert x.min() >= 0.0 and x.max() <= 1.0
        c = np.linalg.cond(T.system_matrix(typ, dim, x, nugget=T.nugget_of(typ), drift=drift))
        worst = max(worst, (c, (typ, dim, n, drift)))
        assert c <= T.COND_CAP, (typ, dim, n, drift, c)
    print(f"{which}: worst condition number {worst[0]:.2e} at {worst[1]}")


def test_local_neighbourhoods_have_no_near_ties_and_are_under_the_cap():
    from test_gpu_local import ref_knn
    worst, tightest = 0.0, np.inf
    for typ, dim, n, k, drift in T.local_cases():
        x, _, y = T.cloud(dim, n)
        idx, gap = T.neighbour_sets(x, y, k)
        assert (gap > 1e-9).all(), (typ, dim, n, k, gap.min())
        tightest = min(tightest, gap.min())
        idx64, _, gap64 = ref_knn(y, x, k)                      # the fp64 search the device is held to agrees
        assert np.array_equal(idx64, idx) and (gap64 > 1e-9).all()
        for key in {tuple(sorted(row)) for row in idx[:-1].tolist()}:
            c = np.linalg.cond(T.system_matrix(typ, dim, x[list(key)], eps=T.default_eps(T.TYPES[typ][0], n, dim),
                                               nugget=T.nugget_of(typ), drift=drift))
            worst = max(worst, c)
            assert c <= T.COND_CAP, (typ, dim, n, k, drift, key, c)
    print(f"local: worst condition number {worst:.2e}, smallest neighbour gap {tightest:.2e}")


def test_every_cloud_meets_the_rule_and_no_seed_was_moved_without_it():
    """tiny_ref.unfit is the whole rule: every cloud the GPU file draws passes it, a cloud without a RESEED entry passes at
    count 0, and an entry is the smallest count that passes -- each smaller one has an objection, printed here"""
    shapes = T.cloud_shapes()
    keys = {(d, n, s) if s else (d, n) for d, n, s in shapes}
    assert set(T.RESEED) <= keys and all(v > 0 for v in T.RESEED.values())
    for dim, n, salt in shapes:
        assert T.unfit(dim, n, salt) is None, (dim, n, salt, T.unfit(dim, n, salt))
        for k in range(T.RESEED.get((dim, n, salt) if salt else (dim, n), 0)):
            why = T.unfit(dim, n, salt, k)
            print(f"cloud dim {dim} n {n} salt {salt}, count {k}: {why}")
            assert why is not None
