"""-m gpu: Clough-Tocher C1 piecewise-cubic interpolation on 2-D meshes, with gradients (csrc/hip/cubic.hip).  PARITY
UNPINNED: the reference has no cubic mesh method.  The oracle is scipy (CloughTocher2DInterpolator at tol = 1e-15,
maxiter = 100000, i.e. with its gradient iteration converged) plus a numpy RESTATEMENT written below: the 19 Bezier
ordinates of the split by the textbook formulas, the value as the cubic Bernstein form summed term by term from a table
of exponents, and the gradient by differentiating that table -- none of which the kernel does (it packs 12 ordinates,
rebuilds 7, and takes value and gradient from four quadratic forms).  Values are compared at the project's value
tolerance, 1e-10 max|f|.

Measured on the CPU while this file was written (scipy 1.15.3):
    restatement against scipy, values: <= 9e-16 max|f| on the five clouds below
    Richardson-extrapolated central differences of scipy's values, (4 D(h/2) - D(h)) / 3 at h = 1e-3, against the
    restatement's analytic gradient (N = 60, the targets kept by the micro-triangle rule): defect 4.7e-13 max|grad s|
    (1.9e-13 at h = 2e-3, where only 82 % of the draw survive the rule);
    GRAD_TOL below is 10 x that.  366 of the 398 drawn targets inside the hull are kept (92 %; cap: at least 80 %).

Observed on one MI355X (printed by every test; the full list is in DESIGN.md 4, "Clough-Tocher"):
    values against scipy: 5.8e-16 .. 8.5e-16 max|f| on the five clouds;  quadratics: value 4.4e-16, gradient 2.7e-14
    estimated gradients against the dense solve: 6.5e-13 .. 4.3e-11 (bounds cond * rtol 5.8e-12 .. 2.4e-9), 16 .. 19 iterations
    gradient against Richardson(scipy) 4.7e-13 max|grad s| (= the oracle's defect), against the restatement 3.5e-14
    across 155 interior edges: value jump 1.8e-9, gradient jump 3.4e-7 = the restatement's; at the sites 8.4e-15 max|g|
    N = 2000, M = 20000: 9.9e-16;  L-shaped 7.1e-16;  flipped edge 5.7e-16;  cubic_simplex, N = 500: 8.5e-16
"""
import numpy as np
import pytest

from gpu_util import bits

pytestmark = pytest.mark.gpu

TOL = 1e-10
RICHARDSON_DEFECT = 4.7e-13           # the oracle's own defect, measured on the CPU (docstring)
GRAD_TOL = 10.0 * RICHARDSON_DEFECT

# exponents (of b1', b2', b3', b4) of the 19 ordinates; the multinomial weight is 6 / (e1! e2! e3! e4!)
NAMES = ("3000", "2100", "2010", "2001", "1200", "1101", "1020", "1011", "1002", "0300", "0210", "0201", "0120", "0111", "0102",
         "0030", "0021", "0012", "0003")
FACT = (1.0, 1.0, 2.0, 6.0)


# ------------------------------------------------------------------------------------------------- the restatement
def barycentric(x, tri, it, y):
    """(b [M, 3], grad b [M, 3, 2]) of the targets y in the triangles it"""
    v = x[tri[it]]
    T = np.stack([v[:, 0] - v[:, 2], v[:, 1] - v[:, 2]], axis=-1)
    Ti = np.linalg.inv(T)
    c = np.einsum("mij,mj->mi", Ti, y - v[:, 2])
    b = np.concatenate([c, 1.0 - c.sum(axis=1, keepdims=True)], axis=1)
    gb = np.concatenate([Ti, -Ti.sum(axis=1, keepdims=True)], axis=1)
    return b, gb


def ordinates(x, tri, nbr, f, g, it):
    t = tri[it]
    v, (f1, f2, f3), gv = x[t], f[t].T, g[t]
    e12, e23, e31 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 1], v[:, 0] - v[:, 2]
    dot = lambda a, b: (a * b).sum(axis=1)
    df12, df21 = dot(gv[:, 0], e12), -dot(gv[:, 1], e12)
    df23, df32 = dot(gv[:, 1], e23), -dot(gv[:, 2], e23)
    df31, df13 = dot(gv[:, 2], e31), -dot(gv[:, 0], e31)
    c = {"3000": f1, "2100": (df12 + 3 * f1) / 3, "2010": (df13 + 3 * f1) / 3,
         "0300": f2, "1200": (df21 + 3 * f2) / 3, "0210": (df23 + 3 * f2) / 3,
         "0030": f3, "1020": (df31 + 3 * f3) / 3, "0120": (df32 + 3 * f3) / 3}
    c["2001"] = (c["2100"] + c["2010"] + c["3000"]) / 3
    c["0201"] = (c["1200"] + c["0300"] + c["0210"]) / 3
    c["0021"] = (c["1020"] + c["0120"] + c["0030"]) / 3
    G = []
    for k in range(3):
        m = nbr[it, k]
        cen = x[tri[np.maximum(m, 0)]].mean(axis=1)
        cb, _ = barycentric(x, tri, it, cen)
        u, w = cb[:, (k + 2) % 3], cb[:, (k + 1) % 3]
        with np.errstate(all="ignore"):
            G.append(np.where(m < 0, -0.5, (2 * u + w - 1) / (2 - 3 * u - 3 * w)))
    c["0111"] = (G[0] * (-c["0300"] + 3 * c["0210"] - 3 * c["0120"] + c["0030"]) + (-c["0300"] + 2 * c["0210"] - c["0120"] + c["0021"] + c["0201"])) / 2
    c["1011"] = (G[1] * (-c["0030"] + 3 * c["1020"] - 3 * c["2010"] + c["3000"]) + (-c["0030"] + 2 * c["1020"] - c["2010"] + c["2001"] + c["0021"])) / 2
    c["1101"] = (G[2] * (-c["3000"] + 3 * c["2100"] - 3 * c["1200"] + c["0300"]) + (-c["3000"] + 2 * c["2100"] - c["1200"] + c["2001"] + c["0201"])) / 2
    c["1002"] = (c["1101"] + c["1011"] + c["2001"]) / 3
    c["0102"] = (c["1101"] + c["0111"] + c["0201"]) / 3
    c["0012"] = (c["1011"] + c["0111"] + c["0021"]) / 3
    c["0003"] = (c["1002"] + c["0102"] + c["0012"]) / 3
    return c


def restatement(x, tri, nbr, f, g, it, y):
    """(s [M], grad s [M, 2], micro-triangle [M]) of the Clough-Tocher interpolant at the targets y in the triangles it"""
    x, f, g, y = (np.asarray(a, dtype=np.float64) for a in (x, f, g, y))
    c = ordinates(x, tri, nbr, f, g, it)
    b, gb = barycentric(x, tri, it, y)
    j = b.argmin(axis=1)
    rows = np.arange(len(y))
    mn = b[rows, j]
    a = np.concatenate([b - mn[:, None], 3 * mn[:, None]], axis=1)
    s = np.zeros(len(y))
    dsda = np.zeros((len(y), 4))
    for name in NAMES:
        e = [int(ch) for ch in name]
        w = 6.0 / np.prod([FACT[k] for k in e])
        s += w * c[name] * np.prod([a[:, i] ** e[i] for i in range(4)], axis=0)
        for i in range(4):
            if e[i]:
                d = list(e)
                d[i] -= 1
                dsda[:, i] += w * c[name] * e[i] * np.prod([a[:, q] ** d[q] for q in range(4)], axis=0)
    # a_i = b_i - b_j (i < 3), a_4 = 3 b_j
    dsdb = dsda[:, :3].copy()
    dsdb[rows, j] = 0.0
    dsdb[rows, j] = 3 * dsda[:, 3] - dsdb.sum(axis=1)
    return s, np.einsum("mi,mij->mj", dsdb, gb), j


def dense_gradient_system(x, tri, f):
    n = len(x)
    A, r = np.zeros((2 * n, 2 * n)), np.zeros(2 * n)
    edges = {(min(t[a], t[(a + 1) % 3]), max(t[a], t[(a + 1) % 3])) for t in tri for a in range(3)}
    for i, j in edges:
        for p, q in ((i, j), (j, i)):
            e = x[q] - x[p]
            L3 = np.hypot(*e) ** 3
            E = np.outer(e, e) / L3
            A[2 * p:2 * p + 2, 2 * p:2 * p + 2] += 4 * E
            A[2 * p:2 * p + 2, 2 * q:2 * q + 2] += 2 * E
            r[2 * p:2 * p + 2] += 6 * (f[q] - f[p]) * e / L3
    return A, r


# ------------------------------------------------------------------------------------------------- clouds and helpers
def response(x):
    return np.sin(3.0 * x[:, 0]) * np.cos(2.0 * x[:, 1]) + x[:, 0]


def clouds():
    rng = np.random.default_rng(1)
    a, b = np.meshgrid(np.arange(7.0), np.arange(7.0))
    return {"uniform 12": rng.random((12, 2)), "uniform 60": rng.random((60, 2)), "uniform 400": rng.random((400, 2)),
            "cluster 40 + 40": np.vstack([rng.random((40, 2)), 0.5 + 0.01 * rng.random((40, 2))]),
            "lattice 7 x 7": np.c_[a.ravel(), b.ravel()] / 6.0}


@pytest.fixture(scope="module")
def cases():
    """per cloud: points, QHull arrays, data, scipy's interpolator with converged gradients, 300 targets inside the hull"""
    from scipy.interpolate import CloughTocher2DInterpolator
    from scipy.spatial import Delaunay
    out = {}
    rng = np.random.default_rng(2)
    for name, x in clouds().items():
        d = Delaunay(x)
        f = response(x)
        ct = CloughTocher2DInterpolator(d, f, tol=1e-15, maxiter=100000)
        y = rng.random((900, 2)) * 0.9 + 0.05
        y = np.ascontiguousarray(y[d.find_simplex(y) >= 0][:300])
        assert len(y) == 300
        out[name] = dict(x=x, d=d, tri=np.ascontiguousarray(d.simplices, dtype=np.int32), nbr=np.ascontiguousarray(d.neighbors, dtype=np.int32),
                         f=f, ct=ct, g=np.ascontiguousarray(ct.grad[:, 0, :]), y=y)
    return out


def make(pkg, kind, x, f, tri=None, nbr=None, g=None, options=None, expect=0):
    s = pkg.Sinterp(kind, 2, len(x), 0)
    if tri is not None:
        assert s.set_triangulation(tri, nbr) == 0
    if g is not None:
        assert s.set_gradients(g) == 0
    if options is not None:
        assert s.set_gradient_options(*options) == 0
    assert s.init(np.ascontiguousarray(x), np.ascontiguousarray(f)) == expect
    return s


CLOUDS = ("uniform 12", "uniform 60", "uniform 400", "cluster 40 + 40", "lattice 7 x 7")


# ------------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("name", CLOUDS)
def test_values_with_scipys_gradients_match_scipy(pkg, cases, name):
    c = cases[name]
    s = make(pkg, "cubic_mesh", c["x"], c["f"], c["tri"], c["nbr"], g=c["g"])
    st, v, leaf = s.eval_many(c["y"], want_leaf=True)
    ref = c["ct"](c["y"])
    mine, _, _ = restatement(c["x"], c["tri"], c["nbr"], c["f"], c["g"], leaf, c["y"])
    fmax = np.abs(c["f"]).max()
    err, err_r = np.abs(v - ref).max() / fmax, np.abs(v - mine).max() / fmax
    print(f"cubic values, {name}: max |s - scipy| = {err:.2e} max|f|, against the restatement {err_r:.2e} (bound {TOL:.0e})")
    assert st == 0 and (leaf >= 0).all()
    assert err <= TOL and err_r <= TOL
    stg, g, it, res = s.get_gradients()
    assert stg == 0 and it == 0 and np.array_equal(bits(g), bits(c["g"]))


# ------------------------------------------------------------------------------------------------- estimated gradients
@pytest.mark.parametrize("name", CLOUDS)
def test_estimated_gradients_match_the_dense_solve(pkg, cases, name):
    c = cases[name]
    A, r = dense_gradient_system(c["x"], c["tri"], c["f"])
    g_dense = np.linalg.solve(A, r).reshape(-1, 2)
    cond = np.linalg.cond(A)
    s = make(pkg, "cubic_mesh", c["x"], c["f"], c["tri"], c["nbr"])
    st, g, it, res = s.get_gradients()
    err = np.linalg.norm(g - g_dense) / np.linalg.norm(g_dense)
    print(f"cubic gradients, {name}: {it} iterations, residual {res:.2e}, |g - g_dense| / |g_dense| = {err:.2e} "
          f"(bound cond * rtol = {cond * 1e-12:.2e}, cond = {cond:.2e}); against scipy's {np.abs(g - c['g']).max() / np.abs(c['g']).max():.2e}")
    assert st == 0 and 0 < it < 1000 and res <= 1e-12
    assert err <= cond * 1e-12
    again = make(pkg, "cubic_mesh", c["x"], c["f"], c["tri"], c["nbr"])
    st2, g2, it2, res2 = again.get_gradients()
    assert st2 == 0 and it2 == it and res2 == res and np.array_equal(bits(g2), bits(g))


def test_maxiter_is_reported(pkg, cases):
    c = cases["uniform 400"]
    with pkg.capi.ErrorCalls():
        s = make(pkg, "cubic_mesh", c["x"], c["f"], c["tri"], c["nbr"], options=(1e-12, 2), expect=pkg.capi.GSL_EMAXITER)
    st, g, it, res = s.get_gradients()
    print(f"cubic gradients, maxiter = 2 on N = 400: residual {res:.2e} after {it} iterations")
    assert st == 0 and it == 2 and 1e-12 < res < 1.0 and np.isfinite(g).all()


# ------------------------------------------------------------------------------------------------- quadratic precision
def test_quadratics_are_reproduced_with_exact_gradients(pkg, cases):
    c = cases["uniform 60"]
    x = c["x"]
    q = lambda p: 2 * p[:, 0] - p[:, 1] + 0.5 * p[:, 0] ** 2 - p[:, 0] * p[:, 1] + 0.3 * p[:, 1] ** 2
    dq = lambda p: np.c_[2 + p[:, 0] - p[:, 1], -1 - p[:, 0] + 0.6 * p[:, 1]]
    s = make(pkg, "cubic_mesh", x, q(x), c["tri"], c["nbr"], g=dq(x))
    y = np.random.default_rng(3).random((2000, 2)) * 0.6 + 0.2
    st, v, g = s.eval_grad_many(y)
    ev, eg = np.abs(v - q(y)).max() / np.abs(q(x)).max(), np.abs(g - dq(y)).max() / np.abs(dq(x)).max()
    print(f"cubic, quadratic data with exact gradients: value {ev:.2e} max|f|, gradient {eg:.2e} max|grad f| (bound {TOL:.0e})")
    assert st == 0 and ev <= TOL and eg <= TOL


# ------------------------------------------------------------------------------------------------- gradient
def richardson_targets(c, h, m=400, seed=4):
    """targets whose 8 stencil points lie in the target's own micro-triangle; (kept targets, their triangles, fraction kept)"""
    y = np.random.default_rng(seed).random((m, 2)) * 0.8 + 0.1
    it = c["d"].find_simplex(y)
    y, it = y[it >= 0], it[it >= 0]
    drawn = len(y)
    b0, _ = barycentric(c["x"], c["tri"], it, y)
    keep = np.ones(len(y), dtype=bool)
    for ax in range(2):
        for step in (h, -h, h / 2, -h / 2):
            p = y.copy()
            p[:, ax] += step
            b, _ = barycentric(c["x"], c["tri"], it, p)
            keep &= (b.min(axis=1) > 0) & (b.argmin(axis=1) == b0.argmin(axis=1))
    return np.ascontiguousarray(y[keep]), it[keep], keep.sum() / drawn


def richardson(ct, y, h):
    out = np.empty_like(y)
    for ax in range(2):
        e = np.zeros(2)
        e[ax] = 1.0
        D = lambda k: (ct(y + k * e) - ct(y - k * e)) / (2 * k)
        out[:, ax] = (4 * D(h / 2) - D(h)) / 3
    return out


def test_gradient_against_richardson_differences_of_scipy(pkg, cases):
    c = cases["uniform 60"]
    h = 1e-3
    y, it, kept = richardson_targets(c, h)
    assert kept >= 0.8 and len(y) >= 300
    ref = richardson(c["ct"], y, h)
    _, mine, _ = restatement(c["x"], c["tri"], c["nbr"], c["f"], c["g"], it, y)
    defect = np.abs(ref - mine).max() / np.abs(mine).max()
    s = make(pkg, "cubic_mesh", c["x"], c["f"], c["tri"], c["nbr"], g=c["g"])
    st, v, g = s.eval_grad_many(y)
    err, err_r = np.abs(g - ref).max() / np.abs(mine).max(), np.abs(g - mine).max() / np.abs(mine).max()
    print(f"cubic gradient, {len(y)} targets ({kept:.0%} of the draw): max |grad - Richardson(scipy)| = {err:.2e} max|grad s| "
          f"(bound {GRAD_TOL:.1e}); oracle's own defect {defect:.2e}; against the restatement's analytic gradient {err_r:.2e}")
    assert st == 0 and err <= GRAD_TOL
    # with and without the gradient output: the same value bits
    st0, v0, _ = s.eval_many(y)
    assert st0 == 0 and np.array_equal(bits(v0), bits(v))
    _, _, g_only = s.eval_grad_many(y, want_value=False)
    assert np.array_equal(bits(g_only), bits(g))
    # at the sites the gradient is the bound one and the value the datum
    stv, vv, gv = s.eval_grad_many(np.ascontiguousarray(c["x"]))
    eg, ev = np.abs(gv - c["g"]).max() / np.abs(c["g"]).max(), np.abs(vv - c["f"]).max() / np.abs(c["f"]).max()
    print(f"cubic at the 60 sites: gradient {eg:.2e} max|g|, value {ev:.2e} max|f| (bound {TOL:.0e})")
    assert stv == 0 and eg <= TOL and ev <= TOL


# ------------------------------------------------------------------------------------------------- C1 across edges
def test_value_and_gradient_are_continuous_across_edges(pkg, cases):
    c = cases["uniform 60"]
    x, tri, nbr = c["x"], c["tri"], c["nbr"]
    pts = []
    for t in range(len(tri)):
        for k in range(3):
            if nbr[t, k] > t:
                p, q = x[tri[t, (k + 1) % 3]], x[tri[t, (k + 2) % 3]]
                L = np.hypot(*(q - p))
                nrm = np.array([-(q - p)[1], (q - p)[0]]) / L
                pts.append(((p + q) / 2 + 1e-9 * L * nrm, (p + q) / 2 - 1e-9 * L * nrm, L))
    yp = np.ascontiguousarray([a for a, _, _ in pts])
    ym = np.ascontiguousarray([b for _, b, _ in pts])
    L = np.array([l for _, _, l in pts])
    s = make(pkg, "cubic_mesh", x, c["f"], tri, nbr, g=c["g"])
    (sp, vp, lp), (sm, vm, lm) = s.eval_many(yp, want_leaf=True), s.eval_many(ym, want_leaf=True)
    _, _, gp = s.eval_grad_many(yp)
    _, _, gm = s.eval_grad_many(ym)
    assert sp == sm == 0 and (lp != lm).sum() > len(L) // 2              # the pairs do straddle their edges
    rp, rgp, _ = restatement(x, tri, nbr, c["f"], c["g"], lp, yp)
    rm, rgm, _ = restatement(x, tri, nbr, c["f"], c["g"], lm, ym)
    gmax, fmax = max(np.abs(rgp).max(), np.abs(rgm).max()), np.abs(c["f"]).max()
    vj, gj, rj = np.abs(vp - vm), np.abs(gp - gm).max(axis=1), np.abs(rgp - rgm).max(axis=1)
    print(f"cubic across {len(L)} interior edges: value jump {vj.max():.2e}, gradient jump {gj.max():.2e} "
          f"(the restatement shows {rj.max():.2e}; max|grad s| = {gmax:.2e})")
    assert (vj <= 1e-9 * L * 2 * gmax + TOL * fmax).all()
    assert (gj <= rj + TOL * gmax).all()


# ------------------------------------------------------------------------------------------------- batches
@pytest.fixture(scope="module")
def big(pkg):
    from scipy.spatial import Delaunay
    rng = np.random.default_rng(5)
    x = rng.random((2000, 2))
    d = Delaunay(x)
    tri, nbr = np.ascontiguousarray(d.simplices, dtype=np.int32), np.ascontiguousarray(d.neighbors, dtype=np.int32)
    f = response(x)
    s = make(pkg, "cubic_mesh", x, f, tri, nbr)
    y = np.ascontiguousarray(rng.random((20000, 2)) * 1.02 - 0.01)       # a few fall outside the hull
    return dict(x=x, f=f, tri=tri, nbr=nbr, s=s, y=y)


def test_a_value_does_not_depend_on_its_batch(pkg, big):
    import torch
    s, y = big["s"], big["y"]
    with pkg.capi.ErrorCalls():
        st, v, g = s.eval_grad_many(y)                                   # >= 4096 targets: located through the sorted route
        st0, v0, leaf = s.eval_many(y, want_leaf=True)
    inside = leaf >= 0
    assert st == st0 == pkg.capi.GSL_EDOM and 0 < (~inside).sum() < 2000
    assert np.isnan(v[~inside]).all() and np.isnan(g[~inside]).all() and np.isfinite(v[inside]).all() and np.isfinite(g[inside]).all()
    assert np.array_equal(bits(v0), bits(v))
    st_it, gg, it, res = s.get_gradients()
    mine, mine_g, _ = restatement(big["x"], big["tri"], big["nbr"], big["f"], gg, leaf[inside], y[inside])
    err = np.abs(v[inside] - mine).max() / np.abs(big["f"]).max()
    print(f"cubic, N = 2000 ({it} iterations, residual {res:.2e}), M = 20000: against the restatement {err:.2e} max|f|, "
          f"gradient {np.abs(g[inside] - mine_g).max() / np.abs(mine_g).max():.2e}")
    assert err <= TOL
    k100 = np.nonzero(inside)[0][:100]
    st1, v1, g1 = s.eval_grad_many(np.ascontiguousarray(y[k100]))
    assert st1 == 0 and np.array_equal(bits(v1), bits(v[k100])) and np.array_equal(bits(g1), bits(g[k100]))
    for k in k100[:4]:
        se, ve, ge = s.eval_grad_e(y[k])
        assert se == 0 and bits(np.array([ve]))[0] == bits(v[k:k + 1])[0] and np.array_equal(bits(ge), bits(g[k]))
        s1, v1 = s.eval_e(y[k])
        assert s1 == 0 and bits(np.array([v1]))[0] == bits(v[k:k + 1])[0]
    # resident buffers
    ty = torch.from_numpy(y).cuda()
    tv = torch.empty(len(y), dtype=torch.float64, device="cuda")
    tg = torch.empty((len(y), 2), dtype=torch.float64, device="cuda")
    tl = torch.empty(len(y), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert s.eval_grad_resident(ty.data_ptr(), len(y), 2, tv.data_ptr(), tg.data_ptr(), 2) == 0
    tv2 = torch.empty(len(y), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    assert s.eval_resident(ty.data_ptr(), len(y), 2, tv2.data_ptr(), tl.data_ptr()) == 0
    torch.cuda.synchronize()
    same = lambda a, b: np.array_equal(bits(a[inside]), bits(b[inside])) and np.isnan(a[~inside]).all()
    assert same(tv.cpu().numpy(), v) and same(tv2.cpu().numpy(), v) and same(tg.cpu().numpy(), g)
    assert np.array_equal(tl.cpu().numpy(), leaf)


def test_targets_outside_and_nan_targets(pkg, cases):
    c = cases["uniform 60"]
    s = make(pkg, "cubic_mesh", c["x"], c["f"], c["tri"], c["nbr"])
    y = np.array([[0.5, 0.5], [-3.0, 0.5], [0.4, np.nan], [7.0, 7.0], [0.45, 0.55]])
    with pkg.capi.ErrorCalls():
        st, v, leaf = s.eval_many(y, want_leaf=True)
        stg, vg, g = s.eval_grad_many(y)
        se, ve = s.eval_e(y[1])
    ok = np.array([True, False, False, False, True])
    assert st == stg == se == pkg.capi.GSL_EDOM and np.isnan(ve)
    assert (leaf[~ok] == -1).all() and (leaf[ok] >= 0).all()
    assert np.isnan(v[~ok]).all() and np.isnan(g[~ok]).all() and np.isfinite(v[ok]).all() and np.isfinite(g[ok]).all()
    assert np.array_equal(bits(v[ok]), bits(vg[ok]))


# ------------------------------------------------------------------------------------------------- other meshes
def flip_one_interior_edge(x, tri, nbr):
    """the triangle array with the shared edge of one strictly convex pair of triangles exchanged for the other diagonal"""
    def cross(a, b, c):
        return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
    for t in range(len(tri)):
        for k in range(3):
            u = nbr[t, k]
            if u < 0:
                continue
            a, b, c = tri[t, k], tri[t, (k + 1) % 3], tri[t, (k + 2) % 3]      # the edge b-c is shared; a is opposite
            d = [v for v in tri[u] if v != b and v != c][0]
            s1, s2 = cross(x[a], x[d], x[b]), cross(x[a], x[d], x[c])
            area = abs(cross(x[a], x[b], x[c])) + abs(cross(x[d], x[b], x[c]))
            if s1 * s2 < 0 and min(abs(s1), abs(s2)) > 0.2 * area:
                out = tri.copy()
                out[t] = [a, b, d]
                out[u] = [a, d, c]
                return out
    raise AssertionError("no flippable edge")


def test_non_convex_and_non_delaunay_meshes(pkg, cases):
    from scipy.spatial import Delaunay
    rng = np.random.default_rng(6)
    # an L: the unit square without its upper right quarter; the triangles QHull puts across the notch are removed
    x = rng.random((400, 2))
    x = x[~((x[:, 0] > 0.5) & (x[:, 1] > 0.5))][:150]
    d = Delaunay(x)
    cen = x[d.simplices].mean(axis=1)
    tri_l = np.ascontiguousarray(d.simplices[~((cen[:, 0] > 0.5) & (cen[:, 1] > 0.5))], dtype=np.int32)
    assert len(tri_l) < len(d.simplices)
    mesh_l = pkg.SimplexMesh.from_arrays(x, tri_l)
    assert not mesh_l.convex()
    c = cases["uniform 60"]
    tri_f = flip_one_interior_edge(c["x"], c["tri"], c["nbr"])
    mesh_f = pkg.SimplexMesh.from_arrays(c["x"], tri_f)
    assert mesh_f.delaunay_metric() == 0
    for what, pts, tri, mesh in (("L-shaped, convex = 0", x, tri_l, mesh_l), ("one flipped edge", c["x"], tri_f, mesh_f)):
        f = response(pts)
        nbr = mesh.neighbours()
        s = make(pkg, "cubic_mesh", pts, f, tri)
        st_g, g, it, res = s.get_gradients()
        y = np.ascontiguousarray(rng.random((600, 2)) * 0.96 + 0.02)
        with pkg.capi.ErrorCalls():
            st, v, leaf = s.eval_many(y, want_leaf=True)
            _, _, gr = s.eval_grad_many(y)
        inside = leaf >= 0
        assert st in (0, pkg.capi.GSL_EDOM) and inside.sum() >= 300 and st_g == 0 and 0 < it < 1000
        if what.startswith("L"):
            notch = (y[:, 0] > 0.55) & (y[:, 1] > 0.55)
            assert notch.sum() > 50 and not inside[notch].any()
        mine, mine_g, _ = restatement(pts, tri, nbr, f, g, leaf[inside], y[inside])
        err = np.abs(v[inside] - mine).max() / np.abs(f).max()
        err_g = np.abs(gr[inside] - mine_g).max() / np.abs(mine_g).max()
        print(f"cubic, {what}: {inside.sum()} targets, value {err:.2e} max|f|, gradient {err_g:.2e} max|grad s| (bound {TOL:.0e})")
        assert err <= TOL and err_g <= TOL


# ------------------------------------------------------------------------------------------------- tree-built type, checkpoints
def test_cubic_simplex_and_checkpoints(pkg, orc, cases, tmp_path):
    n = 500
    x = orc.synth_centres(n, 2) * [40.0, 0.25] + [5.0, -1.0]            # anisotropic: the tree standardises per axis
    f = response(x / [40.0, 0.25])
    y = np.ascontiguousarray(orc.synth_targets(0, 3000, 2) * [40.0, 0.25] + [5.0, -1.0])
    s = pkg.Sinterp("cubic_simplex", 2, n, 0)
    assert s.set_tree_options(0, pkg.capi.Rng(0)) == 0 and s.init(x, f) == 0
    with pkg.capi.ErrorCalls():
        st, v, leaf = s.eval_many(y, want_leaf=True)
        _, _, gr = s.eval_grad_many(y)
    tree = pkg.SimplexTree(2, n)
    assert tree.init(x, flags=0, rng=pkg.capi.Rng(0)) == 0
    mesh = pkg.SimplexMesh.from_tree(tree)
    tri, nbr = mesh.triangles(), mesh.neighbours()
    st_g, g, it, res = s.get_gradients()
    inside = leaf >= 0
    assert st_g == 0 and 0 < it < 1000 and inside.sum() > 2400 and st == (0 if inside.all() else pkg.capi.GSL_EDOM)
    mine, mine_g, _ = restatement(x, tri, nbr, f, g, leaf[inside], y[inside])
    err = np.abs(v[inside] - mine).max() / np.abs(f).max()
    err_g = np.abs(gr[inside] - mine_g).max() / np.abs(mine_g).max()
    print(f"cubic_simplex, anisotropic N = 500 ({it} iterations, residual {res:.2e}): value {err:.2e} max|f|, gradient {err_g:.2e} "
          f"max|grad s| (bound {TOL:.0e})")
    assert err <= TOL and err_g <= TOL
    stg, grid = s.eval_grid(x.min(axis=0) + 0.3 * np.ptp(x, axis=0), x.min(axis=0) + 0.7 * np.ptp(x, axis=0), 16, 16)
    assert stg == 0 and np.isfinite(grid).all()
    c = cases["uniform 60"]
    m = make(pkg, "cubic_mesh", c["x"], c["f"], c["tri"], c["nbr"])
    for kind, src, yy in (("cubic_simplex", s, y), ("cubic_mesh", m, c["y"])):
        size = len(x) if kind == "cubic_simplex" else len(c["x"])
        with pkg.capi.ErrorCalls():
            st0, v0, g0 = src.eval_grad_many(yy)
        _, gs, its, _ = src.get_gradients()
        path = tmp_path / (kind + ".bin")
        assert src.fwrite(path) == 0 and its > 0
        r = pkg.Sinterp(kind, 2, size, 0)
        assert r.fread(path) == 0
        str_, gr_, itr, _ = r.get_gradients()
        assert str_ == 0 and itr == 0 and np.array_equal(bits(gr_), bits(gs))            # restored, not estimated again
        with pkg.capi.ErrorCalls():
            st1, v1, g1 = r.eval_grad_many(yy)
        ok = np.isfinite(v0)
        assert st1 == st0 and np.array_equal(bits(v1[ok]), bits(v0[ok])) and np.array_equal(bits(g1[ok]), bits(g0[ok]))
        assert np.isnan(v1[~ok]).all()
        other = "cubic_mesh" if kind == "cubic_simplex" else "cubic_simplex"
        with pkg.capi.ErrorCalls():
            assert pkg.Sinterp(other, 2, size, 0).fread(path) == pkg.capi.GSL_EBADLEN
            assert pkg.Sinterp("linear_mesh", 2, size, 0).fread(path) == pkg.capi.GSL_EBADLEN
    # what the Clough-Tocher types do not offer, and the device entries' refusals
    EUNSUP = pkg.capi.GSL_EUNSUP
    with pkg.capi.ErrorCalls():
        assert pkg.lib().gsl_sinterp_eval_variance_resident(s._p, None, 0, 2, None) == EUNSUP
        assert s.set_neighbours(4) == EUNSUP
        grp_s = pkg.Sinterp("cubic_simplex", 2, n, 0)
        assert grp_s.set_device_list([0, 0]) == 0 and grp_s.init(x, f) == EUNSUP
        grp = mesh.device_alloc_multi([0, 0])
        assert grp.set_response(f) == 0 and grp.eval_cubic_many(y[:10])[0] == EUNSUP
        from scipy.spatial import Delaunay
        x3 = np.random.default_rng(5).random((50, 3))
        d3 = pkg.SimplexMesh.from_arrays(x3, Delaunay(x3).simplices.astype(np.int32)).device_alloc(0)
        assert d3.set_response(x3[:, 0]) == 0 and d3.gradients()[0] == EUNSUP
    # the mirror: rebinding a response drops gradients and records; the linear path is untouched
    dev = mesh.device_alloc(0)
    assert dev.set_response(f) == 0
    _, lin0, t0 = dev.eval_many(y)
    with pkg.capi.ErrorCalls():
        std, vd, gd, td = dev.eval_cubic_many(y, want_grad=True)
        _, lin1, t1 = dev.eval_many(y)
    assert np.array_equal(td, leaf) and np.array_equal(bits(vd[inside]), bits(v[inside])) and np.array_equal(bits(gd[inside]), bits(gr[inside]))
    assert np.array_equal(t0, t1) and np.array_equal(bits(lin0[inside]), bits(lin1[inside]))
    assert dev.set_response(2.0 * f) == 0
    with pkg.capi.ErrorCalls():
        _, v2, _, _ = dev.eval_cubic_many(y)
    assert np.abs(v2[inside] - 2.0 * v[inside]).max() <= 1e-10 * np.abs(f).max() and dev.gradients()[2] > 0


# ------------------------------------------------------------------------------------------------- raw entries, edge cases
def test_raw_entries_skipped_edges_unused_vertices_and_flat_triangles(pkg):
    import torch
    capi = pkg.capi
    ctx = capi.HipContext(0)
    cu = lambda a, t: torch.from_numpy(np.ascontiguousarray(a, dtype=t)).cuda()
    # the unit square cut along 1-2; vertex 4 duplicates vertex 3 (an edge of length 0 is its only one), vertex 5 has no
    # edge at all; vertex 6 is collinear with 0 and 1, vertex 7 sits 2^-50 above the midpoint of 0-1
    x = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0], [1.0, 1.0], [5.0, 5.0], [2.0, 0.0], [0.5, 2.0 ** -50]])
    f = 2.0 * x[:, 0] + 3.0 * x[:, 1] + np.array([0.0, 0.0, 0.0, 0.5, 0.0, 0.0, 0.0, 0.0])
    # rows: a self-edge in row 0, an id out of range in row 1, the zero-length edge 3-4 in rows 3 and 4; rows 5, 6, 7 empty
    rows = [[0, 1, 2], [0, 2, 3, 99], [0, 1, 3], [1, 2, 4], [3], [], [], []]
    off = np.cumsum([0] + [len(r) for r in rows])
    adj = np.concatenate([np.array(r, dtype=np.int64) for r in rows])
    d_off, d_adj, d_x, d_f = cu(off, np.int32), cu(adj, np.int32), cu(x, np.float64), cu(f, np.float64)
    d_g = torch.full((8, 2), np.nan, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    st, it, res = ctx.mesh_cubic_gradients(8, d_off.data_ptr(), d_adj.data_ptr(), len(adj), d_x.data_ptr(), d_f.data_ptr(), d_g.data_ptr())
    g = d_g.cpu().numpy()
    A, r = dense_gradient_system(x[:4], np.array([[0, 1, 2], [1, 3, 2]]), f[:4])
    g_dense = np.linalg.solve(A, r).reshape(-1, 2)
    err, cond = np.linalg.norm(g[:4] - g_dense) / np.linalg.norm(g_dense), np.linalg.cond(A)
    print(f"cubic raw gradients, 4 used vertices of 8: {it} iterations, residual {res:.2e}, error {err:.2e} (bound {cond * 1e-12:.2e})")
    assert st == 0 and 0 < it < 1000 and res <= 1e-12 and err <= cond * 1e-12
    assert (g[4:] == 0.0).all()                                                      # left out of the system
    # records: two proper triangles, an exactly flat one (no plane), a sliver under the flat tolerance (a plane: 2, 3)
    tri = np.array([[0, 1, 2], [1, 3, 2], [0, 1, 6], [0, 1, 7]])
    nbr = np.array([[1, -1, -1], [-1, 0, -1], [-1, -1, -1], [-1, -1, -1]])
    d_rec = torch.zeros(4 * capi.CUBIC_RECORD_BYTES // 8, dtype=torch.float64, device="cuda")
    d_tri, d_nbr = cu(tri, np.int32), cu(nbr, np.int32)
    ctx.mesh_cubic_pack(4, d_tri.data_ptr(), d_nbr.data_ptr(), 8, d_x.data_ptr(), d_f.data_ptr(), d_g.data_ptr(), d_rec.data_ptr())
    y = np.array([[0.5, 0.0], [0.5, 0.0], [0.25, 0.25], [0.25, 0.25], [0.7, 0.6]])
    located = np.array([2, 3, 0, -1, 1])
    lin = np.array([7.0, 8.0, -1.0, -1.0, -1.0])
    d_y, d_loc, d_lin = cu(y, np.float64), cu(located, np.int32), cu(lin, np.float64)
    d_v = torch.zeros(5, dtype=torch.float64, device="cuda")
    d_gr = torch.zeros((5, 3), dtype=torch.float64, device="cuda")                 # gtda = 3: the padding column stays 0
    d_v0 = torch.zeros(5, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ctx.mesh_cubic_eval(4, d_rec.data_ptr(), d_loc.data_ptr(), d_lin.data_ptr(), d_y.data_ptr(), 5, 2, d_v.data_ptr(), d_gr.data_ptr(), 3)
    ctx.mesh_cubic_eval(4, d_rec.data_ptr(), d_loc.data_ptr(), d_lin.data_ptr(), d_y.data_ptr(), 5, 2, d_v0.data_ptr())
    ctx.sync()
    v, gr, v0 = d_v.cpu().numpy(), d_gr.cpu().numpy(), d_v0.cpu().numpy()
    assert v[0] == 7.0 and np.isnan(gr[0, :2]).all()                               # flat, no plane: linear value, NaN gradient
    assert v[1] == 8.0 and gr[1, 0] == 2.0 and gr[1, 1] == 3.0                     # flat with a plane: its gradient
    assert np.isnan(v[3]) and np.isnan(gr[3, :2]).all()                            # not located
    assert (gr[:, 2] == 0.0).all()
    mine, mine_g, _ = restatement(x, tri, nbr, f, g, np.array([0, 1]), y[[2, 4]])
    assert np.abs(v[[2, 4]] - mine).max() <= TOL * np.abs(f).max() and np.abs(gr[[2, 4], :2] - mine_g).max() <= TOL * np.abs(mine_g).max()
    assert np.array_equal(bits(v0[[0, 1, 2, 4]]), bits(v[[0, 1, 2, 4]])) and np.isnan(v0[3])
