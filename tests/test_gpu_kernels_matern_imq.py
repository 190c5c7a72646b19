"""-m gpu: the Matern 3/2, Matern 5/2 and inverse multiquadric kernels through every layer -- raw fill, facade init + eval,
gradients, fields, kriging with its variance, leave-one-out, the raw cross-covariance entry, checkpoints, device lists.

    Matern 3/2   phi(r) = (1 + t) exp(-t),          t = sqrt(3) eps r      phi'(r)/r = -3 eps^2 exp(-t)
    Matern 5/2   phi(r) = (1 + t + t^2/3) exp(-t),  t = sqrt(5) eps r      phi'(r)/r = -(5 eps^2 / 3) (1 + t) exp(-t)
    inv. multiq. phi(r) = 1 / sqrt(1 + (eps r)^2)                           phi'(r)/r = -eps^2 phi^3

The oracle knows three kinds, so the reference is numpy fp64 with these formulas, never the code under test: a dense
solve, a naive sum over all centres, analytic gradients.  TOL = 1e-10 is the project's RBF tolerance on
max |got - want| / max |want|; variances are compared absolutely (the sill is 1), as test_gpu_krige_variance.py does.
Every case first asserts ON THE CPU that two independent reference computations agree to REF_TOL = 1e-11:
np.linalg.solve against a Cholesky solve (values), deletion refits against the identity (leave-one-out), the solve formula
against the factor formula (variance).  Shapes: eps = N^(1/d) in 2-D and 3-D (the types' default), eps = 2 N^(1/d) in 1-D
(the 1-D inverse multiquadric at N^(1/d) is too ill-conditioned for the two leave-one-out references to agree).

Bit rule of the fields (case 5).  Column q of the fused sweep is compared bit for bit with a scalar interpolant INITIALISED
on column q, and with the scalar sweep (gsl_sinterp_hip_rbf_eval_model) on the weights gsl_sinterp_get_field_weights returns
for column q: the first pins solve + sweep together at this size, the second the sweep alone."""
import numpy as np
import pytest

from gpu_util import Canaried, bits, dev, ptr

pytestmark = pytest.mark.gpu
TOL = 1e-10
REF_TOL = 1e-11
MATERN32, MATERN52, IMQ = 3, 4, 5
KIND = {"matern32": MATERN32, "matern52": MATERN52, "imq": IMQ, "kriging_matern32": MATERN32, "kriging_matern52": MATERN52}
RBF_TYPES = ("matern32", "matern52", "imq")
KRIGE_TYPES = ("kriging_matern32", "kriging_matern52")
N_SITES = 20


# ------------------------------------------------------------------------------------------------- numpy reference
def phi(kind, eps, r):
    if kind == MATERN32:
        t = np.sqrt(3.0) * eps * r
        return (1.0 + t) * np.exp(-t)
    if kind == MATERN52:
        t = np.sqrt(5.0) * eps * r
        return (1.0 + t + t * t / 3.0) * np.exp(-t)
    assert kind == IMQ
    return 1.0 / np.sqrt(1.0 + (eps * r) ** 2)


def psi(kind, eps, r):
    """phi'(r) / r"""
    if kind == MATERN32:
        return -3.0 * eps * eps * np.exp(-np.sqrt(3.0) * eps * r)
    if kind == MATERN52:
        t = np.sqrt(5.0) * eps * r
        return -(5.0 * eps * eps / 3.0) * (1.0 + t) * np.exp(-t)
    return -eps * eps * phi(IMQ, eps, r) ** 3


def dist(a, b):
    return np.sqrt(((a[:, None, :] - b[None, :, :]) ** 2).sum(axis=2))


def shape_eps(n, dim):
    return (2.0 if dim == 1 else 1.0) * n ** (1.0 / dim)


def relerr(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


def chol_solve(K, B):
    """K^-1 B through the Cholesky factor: the second, independent route of the references"""
    L = np.linalg.cholesky(K)
    return np.linalg.solve(L.T, np.linalg.solve(L, B))


def targets(orc, x, m):
    """m rows in all: synthetic targets followed by the first centres (at most 20)"""
    k = min(N_SITES, len(x))
    return np.ascontiguousarray(np.vstack([orc.synth_targets(0, m - k, x.shape[1]), x[:k]]))


def responses(orc, x, k):
    f = orc.synth_response(x) + 3.0
    maps = [lambda v: v, np.sin, lambda v: v * v + 0.5 * v, np.cos, lambda v: np.exp(0.3 * v), lambda v: 1.0 / (2.0 + v * v)]
    return np.ascontiguousarray(np.stack([maps[q % len(maps)]((1.0 + q // len(maps)) * f) for q in range(k)], axis=1))


def make(pkg, typ, dim, n, eps=None, nugget=None, variance=False, loo=False, devices=None):
    s = pkg.Sinterp(typ, dim, n, 0)
    if devices is not None:
        assert s.set_device_list(devices) == 0
    if nugget is not None:
        assert s.set_nugget(nugget) == 0
    if variance:
        assert s.set_variance(1) == 0
    if eps is not None:
        assert s.set_shape(eps) == 0
    if loo:
        assert s.set_loo(1) == 0
    return s


_values = {}


def value_case(orc, kind, dim, n, m):
    """centres, response, targets, weights, values and gradients of one shape: computed once, shared, left unchanged.  The
    values of the np.linalg.solve weights are checked against those of the Cholesky weights."""
    key = (kind, dim, n, m)
    if key not in _values:
        x = orc.synth_centres(n, dim)
        f = orc.synth_response(x) + 3.0
        y = targets(orc, x, m)
        eps = shape_eps(n, dim)
        K = phi(kind, eps, dist(x, x))
        r = dist(y, x)
        k = phi(kind, eps, r)
        w = np.linalg.solve(K, f)
        want = k @ w
        ref = relerr(k @ chol_solve(K, f), want)
        grad = np.einsum("ij,ija->ia", psi(kind, eps, r) * w[None, :], y[:, None, :] - x[None, :, :])
        print(f"reference {key}: solve vs Cholesky: values {ref:.3e}; cond(K) = {np.linalg.cond(K):.2e}")
        for a in (x, f, y, w, want, grad):
            a.setflags(write=False)
        _values[key] = (x, f, y, eps, w, want, grad, ref)
    x, f, y, eps, w, want, grad, ref = _values[key]
    assert ref <= REF_TOL
    return x, f, y, eps, w, want, grad


SHAPES = [(2, 37, 1000), (2, 700, 1000), (3, 1300, 300), (1, 200, 65)]   # N < 512; one tile + a part; three tiles - 236; 1-D


# ------------------------------------------------------------------------------------------------- 1. raw fill
@pytest.mark.parametrize("kind", [MATERN32, MATERN52, IMQ])
def test_raw_fill(pkg, orc, kind):
    ctx = pkg.HipContext.on_torch_stream(0)
    worst = 0.0
    for n in (1, 2, 129, 701):                       # odd n: the single-column tail and the unaligned store
        for dim in (1, 2, 3):
            x = orc.synth_centres(n, dim)
            eps = shape_eps(n, dim)
            want = phi(kind, eps, dist(x, x))
            lda, xtda = n + 3, dim + 1               # odd lda with odd n: rows at 8-byte aligned addresses only
            d_x = Canaried(x, ld=xtda)
            # lower_only off: the public fill writes both triangles
            d_phi = Canaried(np.zeros((n, n)), ld=lda)
            ctx.rbf_fill(kind, eps, d_x.ptr, n, dim, xtda, d_phi.ptr, lda)
            ctx.sync()
            got = d_phi.get()
            err = np.abs(got - want).max() / np.abs(want).max()
            worst = max(worst, err)
            assert err <= 1e-13, (kind, n, dim, err)
            assert (np.diag(got) == 1.0).all(), (kind, n, dim)                       # phi(0) = 1 exactly
            assert np.array_equal(bits(got), bits(got.T))                            # one expression: symmetric to the bit
            assert d_phi.padding_intact() and d_x.padding_intact()
            # lower_only on: the Cholesky route of the solve fills (and reads) the lower triangle only
            f = orc.synth_response(x) + 3.0
            d_phi = Canaried(np.zeros((n, n)), ld=lda)
            d_w = dev(np.array(f))
            st, route = ctx.rbf_solve(kind, eps, d_x.ptr, n, dim, xtda, d_phi.ptr, lda, ptr(d_w))
            ctx.sync()
            assert st == 0 and route == 1
            assert relerr(want @ d_w.cpu().numpy(), f) < TOL, (kind, n, dim)         # the solved system reproduces f
            assert d_phi.padding_intact()
    print(f"kind {kind}: worst fill error {worst:.3e}")
    ctx.close()


# ------------------------------------------------------------------------------------------------- 2. facade init + eval
@pytest.mark.parametrize("dim,n,m", SHAPES)
@pytest.mark.parametrize("typ", RBF_TYPES)
def test_facade_matches_the_reference(pkg, orc, typ, dim, n, m):
    x, f, y, eps, w, want, _ = value_case(orc, KIND[typ], dim, n, m)
    s = make(pkg, typ, dim, n, eps=None if dim > 1 else eps)        # 2-D / 3-D: the type's default shape IS N^(1/d)
    assert s.init(x, f) == 0 and s.route() == 1
    st, got, _ = s.eval_many(y)
    assert st == 0
    err = relerr(got, want)
    k = min(N_SITES, n)
    at_sites = np.abs(got[-k:] - f[:k]).max() / np.abs(f).max()
    print(f"{typ} dim {dim} n {n} m {m}: values {err:.3e}, s(x_i) - f_i {at_sites:.3e}")
    assert err < TOL and at_sites < TOL
    st, gw = s.weights()
    assert st == 0 and relerr(phi(KIND[typ], eps, dist(x, x)) @ gw, f) < TOL


# ------------------------------------------------------------------------------------------------- 3. two targets per lane
@pytest.mark.parametrize("typ", RBF_TYPES)
def test_two_targets_per_lane(pkg, orc, typ):
    dim, n, m = 2, 700, 262144 + 77                  # the first batch size that gets two targets per lane
    x, f, _, eps, w, _, _ = value_case(orc, KIND[typ], dim, n, 1000)
    y = orc.synth_targets(0, m, dim)
    s = make(pkg, typ, dim, n)
    assert s.init(x, f) == 0
    st, got, _ = s.eval_many(y)
    assert st == 0
    rows = np.sort(np.random.default_rng(7).choice(m, 2000, replace=False))
    rows[-1] = m - 1                                 # the last lane's second target
    want = phi(KIND[typ], eps, dist(y[rows], x)) @ w
    err = relerr(got[rows], want)
    print(f"{typ} m {m}: 2000 sampled rows {err:.3e}")
    assert err < TOL
    st, small, _ = s.eval_many(np.ascontiguousarray(y[:1000]))       # one target per lane: the same bits
    assert st == 0 and np.array_equal(bits(small), bits(got[:1000]))
    st, one = s.eval_e(y[0])
    assert st == 0 and np.array_equal(bits(np.array([one])), bits(got[:1]))


# ------------------------------------------------------------------------------------------------- 4. gradient
@pytest.mark.parametrize("dim,n,m", SHAPES)
@pytest.mark.parametrize("typ", RBF_TYPES)
def test_gradient(pkg, orc, typ, dim, n, m):
    x, f, y, eps, w, want, grad = value_case(orc, KIND[typ], dim, n, m)
    s = make(pkg, typ, dim, n, eps=eps)
    assert s.init(x, f) == 0
    st, val, g = s.eval_grad_many(y)
    assert st == 0 and g.shape == (m, dim)
    eg, ev = relerr(g, grad), relerr(val, want)
    print(f"{typ} dim {dim} n {n} m {m}: gradient {eg:.3e} of max |g| = {np.abs(grad).max():.3e}, value {ev:.3e}")
    assert eg < TOL and ev < TOL
    st, plain, _ = s.eval_many(y)
    assert st == 0 and np.array_equal(bits(val), bits(plain))                        # the value that comes with a gradient
    k = min(N_SITES, n)
    assert np.isfinite(g[-k:]).all() and np.isfinite(val[-k:]).all()                 # targets exactly on a centre
    st, v1, g1 = s.eval_grad_e(x[0])
    assert st == 0 and np.isfinite(v1) and np.isfinite(g1).all()
    assert np.array_equal(bits(g1), bits(g[m - k]))                                   # ... and a function of the target alone
    for c in range(dim):                                                             # a NaN coordinate, in every position
        bad = np.array(y[:3])
        bad[1, c] = np.nan
        st, vb, gb = s.eval_grad_many(bad)
        assert st == 0 and np.isnan(vb[1]) and np.isnan(gb[1]).all()
        assert np.array_equal(bits(vb[[0, 2]]), bits(val[[0, 2]])) and np.array_equal(bits(gb[[0, 2]]), bits(g[[0, 2]]))
        st, pb, _ = s.eval_many(bad)
        assert st == 0 and np.isnan(pb[1]) and np.array_equal(bits(pb[[0, 2]]), bits(val[[0, 2]]))


# ------------------------------------------------------------------------------------------------- 5. fields
_fields = {}


def fields_case(orc, kind, k):
    dim, n, m = 2, 300, 333
    key = (kind, k)
    if key not in _fields:
        x = orc.synth_centres(n, dim)
        F = responses(orc, x, k)
        y = targets(orc, x, m)
        eps = shape_eps(n, dim)
        K = phi(kind, eps, dist(x, x))
        ky = phi(kind, eps, dist(y, x))
        want = ky @ np.linalg.solve(K, F)
        ref = float((np.abs(ky @ chol_solve(K, F) - want).max(axis=0) / np.abs(want).max(axis=0)).max())
        for a in (x, F, y, want):
            a.setflags(write=False)
        _fields[key] = (x, F, y, eps, want, ref)
    x, F, y, eps, want, ref = _fields[key]
    assert ref <= REF_TOL
    return dim, n, m, x, F, y, eps, want


@pytest.mark.parametrize("k", [1, 3, 9, 13])         # 9: one block of 8 plus 1; 13: 8 + 4 + 1
@pytest.mark.parametrize("typ", RBF_TYPES)
def test_fields(pkg, orc, typ, k):
    kind = KIND[typ]
    dim, n, m, x, F, y, eps, want = fields_case(orc, kind, k)
    s = make(pkg, typ, dim, n, eps=eps)
    assert s.init_fields(x, F) == 0 and s.n_fields() == k
    assert s.route() == 1                                                            # one fill, one factorisation
    st, S = s.eval_fields_many(y)
    assert st == 0 and S.shape == (m, k)
    per_field = np.abs(S - want).max(axis=0) / np.abs(want).max(axis=0)
    print(f"{typ} {k} fields: per field {per_field.max():.3e}")
    assert per_field.max() < TOL
    ctx = pkg.HipContext.on_torch_stream(0)
    d_x, d_y = dev(np.array(x)), dev(np.array(y))
    for q in range(k):
        # the bit rule: the scalar sweep on column q's weights
        st, wq = s.field_weights(q)
        assert st == 0
        d_w, d_s = dev(wq), dev(np.zeros(m))
        ctx.rbf_eval(kind, eps, ptr(d_x), n, dim, dim, ptr(d_w), ptr(d_y), m, dim, ptr(d_s))
        ctx.sync()
        assert np.array_equal(bits(S[:, q]), bits(d_s.cpu().numpy())), (typ, k, q)
        # a scalar interpolant initialised on column q
        one = make(pkg, typ, dim, n, eps=eps)
        assert one.init(x, F[:, q].copy()) == 0 and one.route() == 1
        st, v, _ = one.eval_many(y)
        assert st == 0 and np.array_equal(bits(v), bits(S[:, q])), (typ, k, q)
    ctx.close()
    bad = np.array(y[:3])
    bad[1, 0] = np.nan
    st, Sb = s.eval_fields_many(bad)
    assert st == 0 and np.isnan(Sb[1]).all() and np.array_equal(bits(Sb[[0, 2]]), bits(S[[0, 2]]))


# ------------------------------------------------------------------------------------------------- 6. kriging
def krige_reference(kind, eps, nugget, x, f, y):
    """(values, mean, variance, 1^T K^-1 1, disagreement of the two routes for values / variance)"""
    n = len(x)
    K = phi(kind, eps, dist(x, x)) + nugget * np.eye(n)
    k = phi(kind, eps, dist(y, x)).T                                                 # n x m
    A = np.zeros((n + 1, n + 1))                                                     # the saddle system [K 1; 1^T 0] [w; mu] = [f; 0]
    A[:n, :n] = K
    A[:n, n] = A[n, :n] = 1.0
    sol = np.linalg.solve(A, np.append(f, 0.0))
    w, mu = sol[:n], sol[n]
    val = mu + w @ k
    ab = chol_solve(K, np.column_stack([f, np.ones(n)]))                             # a = K^-1 f, b = K^-1 1
    mu2 = ab[:, 0].sum() / ab[:, 1].sum()
    val2 = mu2 + (ab[:, 0] - mu2 * ab[:, 1]) @ k
    b = np.linalg.solve(K, np.ones(n))
    var = 1.0 - (k * np.linalg.solve(K, k)).sum(axis=0) + (1.0 - b @ k) ** 2 / b.sum()          # the solve formula
    L = np.linalg.cholesky(K)
    z = np.linalg.solve(L, k)
    var2 = 1.0 - (z * z).sum(axis=0) + (1.0 - ab[:, 1] @ k) ** 2 / ab[:, 1].sum()              # the factor formula
    return val, mu, var, b.sum(), max(relerr(val2, val), abs(mu2 - mu) / abs(mu)), float(np.abs(var2 - var).max())


_krige = {}


def krige_case(orc, kind, dim, n, m, nugget):
    key = (kind, dim, n, m, nugget)
    if key not in _krige:
        x = orc.synth_centres(n, dim)
        f = orc.synth_response(x) + 3.0
        y = targets(orc, x, m + N_SITES)
        eps = shape_eps(n, dim)
        val, mu, var, denom, ref_v, ref_var = krige_reference(kind, eps, nugget, x, f, y)
        print(f"reference {key}: saddle vs Cholesky: values {ref_v:.3e}; solve vs factor: variance {ref_var:.3e}")
        for a in (x, f, y, val, var):
            a.setflags(write=False)
        _krige[key] = (x, f, y, eps, val, mu, var, denom, ref_v, ref_var)
    x, f, y, eps, val, mu, var, denom, ref_v, ref_var = _krige[key]
    assert ref_v <= REF_TOL and ref_var <= REF_TOL
    return x, f, y, eps, val, mu, var, denom


@pytest.mark.parametrize("dim,n,m,nugget", [(2, 384, 300, 1e-3), (3, 300, 100, 1e-2)])
@pytest.mark.parametrize("typ", KRIGE_TYPES)
def test_kriging(pkg, orc, typ, dim, n, m, nugget):
    kind = KIND[typ]
    x, f, y, eps, val, mu, var, denom = krige_case(orc, kind, dim, n, m, nugget)
    s = make(pkg, typ, dim, n, nugget=nugget, variance=True)
    assert s.init(x, f) == 0 and s.route() == 7
    st, got, _ = s.eval_many(y)
    st2, gmu = s.mean()
    assert st == 0 and st2 == 0
    print(f"{typ} dim {dim} n {n} nugget {nugget}: values {relerr(got, val):.3e}, mean {abs(gmu - mu) / abs(mu):.3e}")
    assert relerr(got, val) < TOL and abs(gmu - mu) <= TOL * abs(mu)
    st, gvar = s.eval_variance_many(y)
    assert st == 0
    ev = np.abs(gvar - var).max()
    print(f"{typ} dim {dim} n {n} nugget {nugget}: variance {ev:.3e}, min {gvar.min():.3e}")
    assert ev < TOL and (gvar >= 0.0).all()
    st, far = s.eval_variance_many(np.full((3, dim), 1.0e3))                         # every covariance term is 0 there
    assert st == 0 and np.abs(far - (1.0 + 1.0 / denom)).max() <= 1e-12 * (1.0 + 1.0 / denom)
    # nugget 0: the model interpolates the data, and the field is known at the data sites
    x0, f0, y0, _, val0, mu0, var0, _ = krige_case(orc, kind, dim, n, m, 0.0)
    z = make(pkg, typ, dim, n, nugget=0.0, variance=True)
    assert z.init(x0, f0) == 0 and z.route() == 7
    st, got0, _ = z.eval_many(y0)
    assert st == 0 and relerr(got0, val0) < TOL
    assert np.abs(got0[-N_SITES:] - f0[:N_SITES]).max() < TOL * np.abs(f0).max()
    st, gvar0 = z.eval_variance_many(y0)
    print(f"{typ} dim {dim} n {n} nugget 0: variance {np.abs(gvar0 - var0).max():.3e}, at the sites {np.abs(gvar0[-N_SITES:]).max():.3e}")
    assert st == 0 and np.abs(gvar0 - var0).max() < TOL and np.abs(gvar0[-N_SITES:]).max() < TOL
    # the gradient entry adds the constant mean to the value only
    st, gval, g = s.eval_grad_many(y)
    assert st == 0 and np.array_equal(bits(gval), bits(got)) and np.isfinite(g).all()


# ------------------------------------------------------------------------------------------------- 7. leave-one-out
def loo_by_deletion(kind, krige, eps, nugget, x, F):
    """(E, v) from n models built without one site each"""
    n, nf = F.shape
    Phi = phi(kind, eps, dist(x, x))
    K = Phi + nugget * np.eye(n)
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
            kb = np.linalg.solve(Kr, np.column_stack([k, np.ones(n - 1)]))
            v[i] = 1.0 - k @ kb[:, 0] + (1.0 - kb[:, 1] @ k) ** 2 / kb[:, 1].sum() + nugget
        else:
            sol = np.linalg.solve(Kr, np.column_stack([F[keep], k]))
            E[i] = F[i] - k @ sol[:, :nf]
            v[i] = 1.0 - k @ sol[:, nf]
    return E, v


def loo_by_identity(kind, krige, eps, nugget, x, F):
    n = len(x)
    K = phi(kind, eps, dist(x, x)) + nugget * np.eye(n)
    diag = np.diag(np.linalg.inv(K)).copy()
    W = np.linalg.solve(K, F)
    if krige:
        b = np.linalg.solve(K, np.ones(n))
        W = W - np.outer(b, W.sum(axis=0) / b.sum())
        diag = diag - b * b / b.sum()
    return W / diag[:, None], 1.0 / diag


def res_err(got, want):
    return float((np.abs(got - want).max(axis=0) / np.abs(want).max(axis=0)).max())


_loo = {}


def loo_case(orc, typ, dim, n, nugget, nf):
    key = (typ, dim, n, nugget, nf)
    if key not in _loo:
        krige = typ in KRIGE_TYPES
        x = orc.synth_centres(n, dim)
        F = responses(orc, x, nf)
        eps = shape_eps(n, dim)
        E, v = loo_by_deletion(KIND[typ], krige, eps, nugget, x, F)
        E2, v2 = loo_by_identity(KIND[typ], krige, eps, nugget, x, F)
        ref = (res_err(E2, E), float(np.abs(v2 - v).max()))
        print(f"reference {key}: deletion vs identity: residuals {ref[0]:.3e}, variances {ref[1]:.3e}")
        for a in (x, F, E, v):
            a.setflags(write=False)
        _loo[key] = (x, F, eps, E, v, ref)
    x, F, eps, E, v, ref = _loo[key]
    assert ref[0] <= REF_TOL and ref[1] <= REF_TOL
    return x, F, eps, E, v


@pytest.mark.parametrize("dim,n", [(2, 300), (1, 100)])
@pytest.mark.parametrize("typ", RBF_TYPES + KRIGE_TYPES)
def test_leave_one_out(pkg, orc, typ, dim, n):
    nugget = 1e-3 if typ in KRIGE_TYPES else 0.0
    x, F, eps, E, v = loo_case(orc, typ, dim, n, nugget, 1)
    s = make(pkg, typ, dim, n, eps=eps, nugget=nugget if typ in KRIGE_TYPES else None, loo=True)
    assert s.init(x, F[:, 0].copy()) == 0 and s.route() == (7 if typ in KRIGE_TYPES else 1)
    st, got_e = s.loo_residuals()
    st2, got_v = s.loo_variance()
    assert st == 0 and st2 == 0 and got_e.shape == (n, 1)
    er, ev = res_err(got_e, E), float(np.abs(got_v - v).max())
    print(f"{typ} dim {dim} n {n}: residuals {er:.3e} of max |e| = {np.abs(E).max():.3e}, variances {ev:.3e}, min v = {got_v.min():.3e}")
    assert er < TOL and ev < TOL and (got_v > 0.0).all()


@pytest.mark.parametrize("typ", ("matern52", "kriging_matern32"))
def test_leave_one_out_fields_share_the_diagonal(pkg, orc, typ):
    dim, n, nf = 2, 300, 3
    nugget = 1e-3 if typ in KRIGE_TYPES else 0.0
    x, F, eps, E, v = loo_case(orc, typ, dim, n, nugget, nf)
    s = make(pkg, typ, dim, n, nugget=nugget if typ in KRIGE_TYPES else None, loo=True)
    assert s.init_fields(x, F) == 0 and s.route() in (1, 7) and s.n_fields() == nf
    st, got_e = s.loo_residuals()
    st2, got_v = s.loo_variance()
    assert st == 0 and st2 == 0 and got_e.shape == (n, nf)
    assert res_err(got_e, E) < TOL and np.abs(got_v - v).max() < TOL
    _, _, _, _, v1 = loo_case(orc, typ, dim, n, nugget, 1)                           # the variance does not depend on the responses
    assert np.abs(v1 - got_v).max() < 2 * TOL


# ------------------------------------------------------------------------------------------------- 8. raw cross-entries
@pytest.mark.parametrize("kind", [MATERN32, MATERN52, IMQ])
def test_raw_krige_variance_strided(pkg, orc, kind):
    dim, n, m, nugget = 2, 129, 65, 1e-3
    x = orc.synth_centres(n, dim)
    f = orc.synth_response(x) + 3.0
    y = targets(orc, x, m)
    eps = shape_eps(n, dim)
    _, _, want, denom, _, ref_var = krige_reference(kind, eps, nugget, x, f, y)
    assert ref_var <= REF_TOL
    ctx = pkg.HipContext.on_torch_stream(0)
    xtda, ytda, lda = dim + 1, dim + 2, n + 6
    d_x, d_y = Canaried(x, ld=xtda), Canaried(y, ld=ytda)
    d_phi = Canaried(np.zeros((n, n)), ld=lda)
    d_w = dev(f)
    st, route, _ = ctx.krige_solve(kind, eps, nugget, d_x.ptr, n, dim, xtda, d_phi.ptr, lda, ptr(d_w))
    assert st == 0 and route == 7
    d_b, d_dinv = dev(np.zeros(n)), dev(np.zeros((n + 31) // 32 * 1024))
    st, got_denom = ctx.krige_variance_prepare(n, d_phi.ptr, lda, ptr(d_b), ptr(d_dinv))
    assert st == 0 and abs(got_denom - denom) <= 1e-9 * abs(denom)
    for chunk in (64, 4096):                                                         # two passes (64 + 1 rows); one pass
        d_work = dev(np.full(pkg.HipContext.krige_variance_work(n, chunk), np.nan))
        d_var = Canaried(np.zeros(m))
        st = ctx.krige_variance(kind, eps, d_x.ptr, n, dim, xtda, d_phi.ptr, lda, ptr(d_b), ptr(d_dinv), got_denom, d_y.ptr, m, ytda,
                                d_var.ptr, ptr(d_work), chunk)
        ctx.sync()
        assert st == 0
        err = np.abs(d_var.get() - want).max()
        print(f"raw variance kind {kind} chunk {chunk}: {err:.3e}")
        assert err < TOL and d_var.padding_intact()
    assert d_x.padding_intact() and d_y.padding_intact() and d_phi.padding_intact()
    ctx.close()


def test_raw_entries_reject_what_they_do_not_know(pkg):
    ctx = pkg.HipContext.on_torch_stream(0)
    n, m, dim = 8, 4, 2
    buf = dev(np.zeros(4096))
    p = ptr(buf)
    for kind in (6, 7, -1):                                                          # 0 .. 5 are the kinds
        assert ctx.rbf_eval_grad(kind, 1.0, p, n, dim, dim, p, p, m, dim, p, p, dim) == pkg.GSL_EINVAL
        assert ctx.rbf_eval_fields(kind, 1.0, p, n, dim, dim, p, n, 2, p, m, dim, p, 2) == pkg.GSL_EINVAL
        assert pkg.lib().gsl_sinterp_hip_rbf_fill(ctx.handle, kind, 1.0, p, n, dim, dim, p, n) == pkg.GSL_EINVAL
        assert ctx.krige_solve(kind, 1.0, 0.0, p, n, dim, dim, p, n, p)[0] == pkg.GSL_EINVAL
        assert ctx.rbf_solve_fields(kind, 1.0, p, n, dim, dim, p, n, p, n, 2)[0] == pkg.GSL_EINVAL
    poly = np.zeros(4)
    for kind in (MATERN32, MATERN52, IMQ):                                           # the affine tail stays thin-plate only
        assert ctx.rbf_solve_affine(kind, 1.0, p, n, dim, dim, p, n + dim + 2, p, poly)[0] == pkg.GSL_EINVAL
    ctx.close()


# ------------------------------------------------------------------------------------------------- 9. checkpoint
@pytest.mark.parametrize("typ,other", [("matern52", "matern32"), ("kriging_matern32", "kriging_matern52")])
def test_checkpoint(pkg, orc, tmp_path, typ, other):
    dim, n, m = 2, 300, 333
    nugget = 1e-3 if typ in KRIGE_TYPES else None
    x = orc.synth_centres(n, dim)
    f = orc.synth_response(x) + 3.0
    y = targets(orc, x, m)
    s = make(pkg, typ, dim, n, nugget=nugget)
    assert s.init(x, f) == 0
    st, val, g = s.eval_grad_many(y)
    assert st == 0
    path = str(tmp_path / "model.bin")
    assert s.fwrite(path) == 0
    head = np.fromfile(path, dtype=np.uint64, count=4)
    assert bytes(head[:1].tobytes()) == b"GSLSINT1" and tuple(head[1:]) == ({"matern52": 8, "kriging_matern32": 10}[typ], dim, n)
    r = make(pkg, typ, dim, n, nugget=nugget)
    assert r.fread(path) == 0
    st, val2, g2 = r.eval_grad_many(y)
    st2, plain, _ = r.eval_many(y)
    assert st == 0 and st2 == 0
    assert np.array_equal(bits(val2), bits(val)) and np.array_equal(bits(g2), bits(g)) and np.array_equal(bits(plain), bits(val))
    if nugget is not None:
        assert r.mean() == s.mean()
    for wrong in (other, "gaussian" if nugget is None else "kriging"):               # the existing mismatch status
        assert make(pkg, wrong, dim, n).fread(path) == pkg.capi.GSL_EBADLEN


def test_gaussian_checkpoint_is_unchanged(pkg, orc, tmp_path):
    dim, n = 2, 300
    x = orc.synth_centres(n, dim)
    f = orc.synth_response(x) + 3.0
    blobs = []
    for name in ("a.bin", "b.bin"):
        s = pkg.Sinterp("gaussian", dim, n, 0)
        assert s.init(x, f) == 0 and s.fwrite(str(tmp_path / name)) == 0
        blobs.append((tmp_path / name).read_bytes())
    assert blobs[0] == blobs[1]
    # GSLSINT1 | type id 0 | dim | size | eps | flags 0 | centres | weights: layout and ids of the older types stay
    assert len(blobs[0]) == 8 + 3 * 8 + 8 + 8 + 8 * n * (dim + 1)
    assert blobs[0][:8] == b"GSLSINT1"
    assert tuple(np.frombuffer(blobs[0], dtype=np.uint64, count=3, offset=8)) == (0, dim, n)
    assert np.frombuffer(blobs[0], dtype=np.float64, count=1, offset=32)[0] == 2.0 * n ** 0.5
    assert np.array_equal(np.frombuffer(blobs[0], dtype=np.float64, count=n * dim, offset=48).reshape(n, dim), x)
    ids = {}
    for typ in ("tps", "wendland", "kriging", "matern32", "matern52", "imq", "kriging_matern32", "kriging_matern52"):
        t = pkg.Sinterp(typ, dim, n, 0)
        assert t.init(x, f) == 0 and t.fwrite(str(tmp_path / "t.bin")) == 0
        ids[typ] = int(np.fromfile(str(tmp_path / "t.bin"), dtype=np.uint64, count=2)[1])
    assert ids == {"tps": 1, "wendland": 3, "kriging": 4, "matern32": 7, "matern52": 8, "imq": 9, "kriging_matern32": 10,
                   "kriging_matern52": 11}


# ------------------------------------------------------------------------------------------------- 10. device list
@pytest.mark.parametrize("typ", ("matern32",))
def test_device_list(pkg, orc, typ):
    dim, n, m = 2, 300, 5000
    x = orc.synth_centres(n, dim)
    f = orc.synth_response(x) + 3.0
    y = orc.synth_targets(0, m, dim)
    single = make(pkg, typ, dim, n)
    assert single.init(x, f) == 0
    st, want, _ = single.eval_many(y)
    assert st == 0
    multi = make(pkg, typ, dim, n, devices=[0, 0, 0])                                # three members on one GPU: the shard plumbing
    assert multi.n_devices() == 3 and multi.init(x, f) == 0
    st, got, _ = multi.eval_many(y)
    assert st == 0 and np.array_equal(bits(got), bits(want))
