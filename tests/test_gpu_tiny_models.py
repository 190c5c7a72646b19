"""-m gpu: every interpolant type at its smallest sizes, through pkg.Sinterp only, against tests/tiny_ref.py.

Sizes.  SMALL = the type's true minimum and the four sizes above it, and 8 (tiny_ref.small_cases); EDGE = 31 .. 129 around
the 32-column and 128-column boundaries of the factorisation for the Cholesky-route features (tiny_ref.edge_cases, fp64
numpy reference).  Inputs: tiny_ref.cloud -- seeded sites in the unit box, nine smooth responses, and 70 targets (the
sites, points inside, ten points up to 10 % outside the box, one NaN row).  Every model runs at its type's DEFAULT shape:
no set_shape anywhere.  tests/test_tiny_ref.py proves on the CPU that every system matrix used here has an fp64 condition
number <= 1e4 and that no k = N - 1 neighbourhood is a near-tie, so 1e-10 is attainable and no target is left out.

Tolerances are those of the entries' existing tests:
    values                        max |got - want| <= 1e-10 max|f|
    variances                     1e-10 absolute (the sill is 1)
    weights, tail coefficients    1e-10 relative to max|want|; only where the exact weights vanish identically (kriging on one
                                  site, universal kriging on N = q sites: the device's are the rounding residue
                                  cond * 2^-52 * max|f| ~ 2e-12) relative to max|f|: with phi <= 1 a weight error d moves
                                  a value by at most N d
    gradients                     test_gpu_rbf_grad.relerr < 1e-10 (where the exact gradient vanishes identically -- kriging
                                  on one site -- 1e-10 max|f| absolute: the box has unit length)
    leave-one-out                 test_gpu_loo.res_err < 1e-10, variances 1e-10 absolute
    scores                        test_gpu_fit: |ML - want| <= 1e-10 N, |LOO - want| <= 1e-10 want"""
import numpy as np
import pytest

import tiny_ref as T
import ukrige_ref
from gpu_util import bits, dev, ptr

pytestmark = pytest.mark.gpu
TOL = 1e-10
SMALL, EDGE_CASES, LOCAL = T.small_cases(), T.edge_cases(), T.local_cases()
GLOBAL = SMALL + EDGE_CASES
idents = lambda cases: ["-".join(str(v) for v in c) for c in cases]


def relerr(got, want):
    """test_gpu_rbf_grad.relerr"""
    return float(np.abs(got - want).max() / np.abs(want).max())


def res_err(got, want):
    """test_gpu_loo.res_err"""
    return float((np.abs(got - want).max(axis=0) / np.abs(want).max(axis=0)).max())


def coef_err(got, want, fmax):
    """relative to max|want|; where the exact coefficients vanish (kriging on one site, universal kriging on q sites: the
    reference holds 0 or 1e-50) relative to max|f|"""
    scale = np.abs(want).max()
    return float(np.abs(got - want).max() / (scale if scale > 1e-30 * fmax else fmax))


# ------------------------------------------------------------------------------------------------- references, once
_refs = {}


def reference(typ, dim, n, drift):
    """the model of all nine fields (extended precision up to 14 sites, fp64 beyond), with its values at the finite
    targets: computed once, shared, left unchanged"""
    key = (typ, dim, n, drift)
    if key not in _refs:
        x, F, y = T.cloud(dim, n)
        m = (T.fit if n < T.EDGE[0] else T.np_fit)(typ, dim, x, F, nugget=T.nugget_of(typ), drift=drift)
        vals = m.values(y[:-1])
        vals.setflags(write=False)
        _refs[key] = (m, vals)
    return _refs[key]


_loo = {}


def loo_reference(typ, dim, n, drift, nf):
    key = (typ, dim, n, drift)
    if key not in _loo:
        x, F, _ = T.cloud(dim, n)
        _loo[key] = (T.loo_by_deletion if n < T.EDGE[0] else T.np_loo_by_deletion)(typ, dim, x, F[:, :5], nugget=T.nugget_of(typ), drift=drift)
    E, v = _loo[key]
    return E[:, :nf], v


def make(pkg, typ, dim, n, drift=0, variance=False, loo=False, neighbours=0):
    s = pkg.Sinterp(typ, dim, n, 0)
    if T.TYPES[typ][1]:
        assert s.set_nugget(T.nugget_of(typ)) == 0
        if drift:
            assert s.set_drift(drift) == 0
        if variance:
            assert s.set_variance(1) == 0
        if neighbours:
            assert s.set_neighbours(neighbours) == 0
    if loo:
        assert s.set_loo(1) == 0
    return s


def loo_defined(typ, dim, n, drift):
    if typ not in T.PD_TYPES:
        return False
    if not T.TYPES[typ][1]:
        return True
    return n > (ukrige_ref.n_terms(dim, drift) if drift else 1)


def route_of(typ, drift):
    return 12 if drift else 7 if T.TYPES[typ][1] else None


# ------------------------------------------------------------------------------------------------- 1. values, every entry
@pytest.mark.parametrize("typ,dim,n,drift", GLOBAL, ids=idents(GLOBAL))
def test_weights_values_and_every_scalar_entry(pkg, tmp_path, typ, dim, n, drift):
    import torch
    x, F, y = T.cloud(dim, n)
    f = np.array(F[:, 0])
    fmax = np.abs(f).max()
    m, want = reference(typ, dim, n, drift)
    kind, krige, affine = T.TYPES[typ]
    s = make(pkg, typ, dim, n, drift)
    with pkg.capi.ErrorCalls() as calls:
        assert s.init(x, f) == 0 and calls == []
    if route_of(typ, drift):
        assert s.route() == route_of(typ, drift)
    st, w = s.weights()
    ew = coef_err(w, m.w[:, 0], fmax)
    assert st == 0 and np.isfinite(w).all()
    ec = 0.0
    if drift:
        st, c, shift, scale = s.drift_coefficients()
        ec = coef_err(c, m.c[:, 0], fmax)
        gs, gc = ukrige_ref.geometry(x)
        assert st == 0 and np.abs(shift - gs).max() <= 1e-15 and np.abs(scale - gc).max() <= 1e-15 * np.abs(gc).max()
        assert s.mean()[0] == pkg.capi.GSL_EUNSUP
    elif krige:
        st, mu = s.mean()
        ec = coef_err(np.array([mu]), m.c[:, 0], fmax)
        assert st == 0
    elif affine:
        st, c = s.poly()
        ec = coef_err(c, m.c[:, 0], fmax)
        assert st == 0
    st, got, _ = s.eval_many(y)
    ev = np.abs(got[:-1] - want[:, 0]).max() / fmax
    print(f"{typ} dim {dim} n {n} drift {drift}: weights {ew:.3e}, tail {ec:.3e}, values {ev:.3e} max|f|")
    assert st == 0 and np.isnan(got[-1]) and np.isfinite(got[:-1]).all()
    assert ew <= TOL and ec <= TOL and ev <= TOL
    if not (krige and T.nugget_of(typ) > 0.0):
        assert np.abs(got[:n] - f).max() <= TOL * fmax               # an interpolant: the data at the sites
    # one target at a time, and resident: the same bits
    for k in range(len(y)) if n < T.EDGE[0] else (0, n - 1, n, len(y) - 2, len(y) - 1):
        st, v = s.eval_e(y[k])
        assert st == 0 and bits(np.array([v]))[0] == bits(got)[k], k
    d_y, d_s = dev(y), torch.zeros(len(y), dtype=torch.float64, device="cuda")
    assert s.eval_resident(ptr(d_y), len(y), dim, ptr(d_s)) == 0
    torch.cuda.synchronize()
    assert (bits(d_s.cpu().numpy()) == bits(got)).all()
    # checkpoint round trip: the same bits from another object
    path = str(tmp_path / "tiny.bin")
    assert s.fwrite(path) == 0
    r = make(pkg, typ, dim, n)
    assert r.fread(path) == 0
    st, again, _ = r.eval_many(y)
    assert st == 0 and (bits(again) == bits(got)).all()


# ------------------------------------------------------------------------------------------------- 2. gradients
@pytest.mark.parametrize("typ,dim,n,drift", SMALL, ids=idents(SMALL))
def test_gradients(pkg, typ, dim, n, drift):
    x, F, y = T.cloud(dim, n)
    f = np.array(F[:, 0])
    m, _ = reference(typ, dim, n, drift)
    want = m.gradient(y[:-1])[:, 0, :]
    s = make(pkg, typ, dim, n, drift)
    assert s.init(x, f) == 0
    st, val, g = s.eval_grad_many(y)
    st2, plain, _ = s.eval_many(y)
    assert st == 0 and st2 == 0 and (bits(val) == bits(plain)).all()
    assert np.isnan(g[-1]).all() and np.isfinite(g[:-1]).all()
    if np.abs(want).max() == 0.0:                                   # kriging on one site: s = f everywhere
        err = np.abs(g[:-1]).max() / np.abs(f).max()
    else:
        err = relerr(g[:-1], want)
    print(f"{typ} dim {dim} n {n} drift {drift}: gradient {err:.3e}, max|want| {np.abs(want).max():.3e}")
    assert err < TOL
    st, none, g_only = s.eval_grad_many(y, want_value=False)
    assert st == 0 and none is None and (bits(g_only) == bits(g)).all()
    for k in (0, n, len(y) - 2):
        st, v0, g0 = s.eval_grad_e(y[k])
        assert st == 0 and bits(np.array([v0]))[0] == bits(val)[k] and (bits(g0) == bits(g[k])).all()


# ------------------------------------------------------------------------------------------------- 3. K fields
@pytest.mark.parametrize("nf", [1, 5, 9])
@pytest.mark.parametrize("typ,dim,n,drift", GLOBAL, ids=idents(GLOBAL))
def test_fields(pkg, typ, dim, n, drift, nf):
    x, F, y = T.cloud(dim, n)
    Fk = np.ascontiguousarray(F[:, :nf])
    fmax = np.abs(Fk).max(axis=0)
    m, want = reference(typ, dim, n, drift)
    loo = nf == 5 and loo_defined(typ, dim, n, drift)
    s = make(pkg, typ, dim, n, drift, loo=loo)
    assert s.init_fields(x, Fk) == 0 and s.n_fields() == nf
    st, S = s.eval_fields_many(y)
    err = (np.abs(S[:-1] - want[:, :nf]).max(axis=0) / fmax).max()
    assert st == 0 and S.shape == (len(y), nf) and np.isnan(S[-1]).all() and np.isfinite(S[:-1]).all()
    ew = 0.0
    for q in range(nf):
        st, w = s.field_weights(q)
        assert st == 0
        ew = max(ew, coef_err(w, m.w[:, q], fmax[q]))
        if drift:
            st, c, _, _ = s.drift_coefficients(q)
            assert st == 0
            ew = max(ew, coef_err(c, m.c[:, q], fmax[q]))
        elif T.TYPES[typ][1]:
            st, mu = s.field_mean(q)
            assert st == 0
            ew = max(ew, coef_err(np.array([mu]), m.c[:, q], fmax[q]))
        elif T.TYPES[typ][2]:
            st, c = s.field_poly(q)
            assert st == 0
            ew = max(ew, coef_err(c, m.c[:, q], fmax[q]))
    print(f"{typ} dim {dim} n {n} drift {drift} K {nf}: worst column {err:.3e}, weights and tails {ew:.3e}")
    assert err <= TOL and ew <= TOL
    st, first, _ = s.eval_many(y)                                    # the scalar entries evaluate field 0: the same bits
    assert st == 0 and (bits(first) == bits(S[:, 0])).all()
    st, one = s.eval_fields_e(y[n])
    assert st == 0 and (bits(one) == bits(S[n])).all()
    if loo:                                                          # the fields share the leave-one-out diagonal
        E, v = loo_reference(typ, dim, n, drift, nf)
        st, gotE = s.loo_residuals()
        st2, gotv = s.loo_variance()
        assert st == 0 and st2 == 0 and res_err(gotE, E) < TOL and np.abs(gotv - v).max() < TOL


# ------------------------------------------------------------------------------------------------- 4. kriging variance
KRIGED = [c for c in GLOBAL if c[0] in T.KRIGE_TYPES]


@pytest.mark.parametrize("typ,dim,n,drift", KRIGED, ids=idents(KRIGED))
def test_kriging_variance(pkg, typ, dim, n, drift):
    x, F, y = T.cloud(dim, n)
    m, _ = reference(typ, dim, n, drift)
    want = np.maximum(m.variance(y[:-1]), 0.0)
    s = make(pkg, typ, dim, n, drift, variance=True)
    assert s.init(x, np.array(F[:, 0])) == 0 and s.route() == route_of(typ, drift)
    st, var = s.eval_variance_many(y)
    err = np.abs(var[:-1] - want).max()
    print(f"{typ} dim {dim} n {n} drift {drift}: variance {err:.3e}, max {want.max():.3e}")
    assert st == 0 and np.isnan(var[-1]) and (var[:-1] >= 0.0).all()
    assert err <= TOL
    if T.nugget_of(typ) == 0.0:
        assert var[:n].max() <= TOL                                  # no uncertainty at the data
    for k in (0, n, len(y) - 2):
        st, v = s.eval_variance_e(y[k])
        assert st == 0 and bits(np.array([v]))[0] == bits(var)[k]


# ------------------------------------------------------------------------------------------------- 5. leave-one-out
WITH_LOO = [c for c in GLOBAL if loo_defined(*c)]


@pytest.mark.parametrize("typ,dim,n,drift", WITH_LOO, ids=idents(WITH_LOO))
def test_leave_one_out(pkg, typ, dim, n, drift):
    x, F, _ = T.cloud(dim, n)
    E, v = loo_reference(typ, dim, n, drift, 1)
    for variance in ((False, True) if T.TYPES[typ][1] else (False,)):   # b / B from a temporary, or kept with the factor
        s = make(pkg, typ, dim, n, drift, loo=True, variance=variance)
        assert s.init(x, np.array(F[:, 0])) == 0
        st, gotE = s.loo_residuals()
        st2, gotv = s.loo_variance()
        assert st == 0 and st2 == 0 and gotE.shape == (n, 1)
        er, ev = res_err(gotE, E), np.abs(gotv - v).max()
        print(f"{typ} dim {dim} n {n} drift {drift} variance {variance}: residuals {er:.3e} of {np.abs(E).max():.3e}, variances {ev:.3e}")
        assert np.isfinite(gotE).all() and (gotv > 0.0).all()
        assert er < TOL and ev < TOL


# ------------------------------------------------------------------------------------------------- 6. the fit criteria
SCORED = [c for c in SMALL if c[0] in T.PD_TYPES and c[3] == 0 and c[2] >= 2]


@pytest.mark.parametrize("typ,dim,n,drift", SCORED, ids=idents(SCORED))
def test_scores(pkg, typ, dim, n, drift):
    x, F, _ = T.cloud(dim, n)
    f = np.array(F[:, 0])
    eps, nugget = T.default_eps(T.TYPES[typ][0], n, dim), T.nugget_of(typ)
    ml, loo = T.scores(typ, dim, x, f, eps, nugget=nugget)
    s = pkg.Sinterp(typ, dim, n, 0)
    fit = s.fit_workspace(x, f)
    with pkg.capi.ErrorCalls() as calls:
        st, got_ml = fit.score(pkg.FIT_ML, eps, nugget)
        st2, got_loo = fit.score(pkg.FIT_LOO, eps, nugget)
    print(f"{typ} dim {dim} n {n}: ML {got_ml:.12g} (want {ml:.12g}), LOO {got_loo:.12g} (want {loo:.12g})")
    assert st == 0 and st2 == 0 and calls == []
    assert abs(got_ml - ml) <= TOL * n
    assert abs(got_loo - loo) <= TOL * loo
    fit.close()


# ------------------------------------------------------------------------------------------------- 7. the local route
@pytest.mark.parametrize("typ,dim,n,k,drift", LOCAL, ids=idents(LOCAL))
def test_local_route(pkg, typ, dim, n, k, drift):
    x, F, y = T.cloud(dim, n)
    f = np.array(F[:, 0])
    fmax = np.abs(f).max()
    idx, _ = T.neighbour_sets(x, y, k)
    want_s, want_v = T.local_krige(typ, dim, x, f, y, idx, drift=drift)
    s = make(pkg, typ, dim, n, drift, neighbours=k)
    assert s.init(x, f) == 0 and s.route() == 11
    st, ls, lv, li = s.eval_local_many(y)
    ok = slice(0, len(y) - 1)
    es, ev = np.abs(ls[ok] - want_s[ok]).max() / fmax, np.abs(lv[ok] - np.maximum(want_v[ok], 0.0)).max()
    print(f"{typ} dim {dim} n {n} k {k} drift {drift}: values {es:.3e} max|f|, variances {ev:.3e}")
    assert st == 0 and (li == idx).all()
    assert np.isnan(ls[-1]) and np.isnan(lv[-1]) and np.isfinite(ls[ok]).all() and (lv[ok] >= 0.0).all()
    assert es <= TOL and ev <= TOL
    st1, s1, _ = s.eval_many(y)
    st2, v2 = s.eval_variance_many(y)
    assert st1 == 0 and st2 == 0 and (bits(s1) == bits(ls)).all() and (bits(v2) == bits(lv)).all()
    for j in (0, n, len(y) - 2):
        st4, s4 = s.eval_e(y[j])
        st5, v5 = s.eval_variance_e(y[j])
        assert st4 == 0 and st5 == 0 and s4 == ls[j] and v5 == lv[j]
    if k == n:                                                       # every neighbourhood is the cloud: the global model
        m, want = reference(typ, dim, n, drift)
        assert np.abs(ls[ok] - want[:, 0]).max() <= TOL * fmax


# ------------------------------------------------------------------------------------------------- 8. meshes of a few simplices
MESHES = [(dim, n) for dim in (2, 3) for n in T.MESH_SIZES[dim]]
MESHES_2D = [(2, n) for n in T.MESH_SIZES[2]]
STRICT = 1e-9                                           # a target this far inside a simplex (barycentric) is nobody's tie
_mesh_refs = {}


def mesh_reference(dim, n):
    """piecewise-linear values, gradients, simplex and margin of every target of the scene, in extended precision"""
    if (dim, n) not in _mesh_refs:
        x, F, simp, nbr, y, tags = T.mesh_scene(dim, n)
        _mesh_refs[(dim, n)] = T.simplex_linear(x, F, simp.tolist(), y)
    return _mesh_refs[(dim, n)]


def check_located(pkg, st, leaf, vals, margin, tags):
    """what the existing tests of the mesh types document: a target outside the mesh (or NaN) has leaf -1 and NaN, and the
    call then reports GSL_EDOM once, with everything else stored; a target on the hull may round to either side"""
    inside, outside = margin > STRICT, ~(margin >= -STRICT)          # NaN rows are outside
    assert (leaf[inside] >= 0).all() and (leaf[outside] == -1).all()
    assert np.isnan(vals[leaf < 0]).all() and np.isfinite(vals[leaf >= 0]).all()
    assert st == (pkg.capi.GSL_EDOM if (leaf < 0).any() else 0)
    assert (leaf[tags == "vertex"] >= 0).all() and (leaf[tags == "interior"] >= 0).all() and (leaf[tags == "centroid"] >= 0).all()
    return inside


def imported(pkg, kind, dim, n):
    x, F, simp, nbr, y, tags = T.mesh_scene(dim, n)
    s = pkg.Sinterp(kind, dim, n, 0)
    assert s.set_triangulation(simp, nbr) == 0
    return s


@pytest.mark.parametrize("dim,n", MESHES, ids=idents(MESHES))
def test_linear_mesh(pkg, tmp_path, dim, n):
    import torch
    x, F, simp, nbr, y, tags = T.mesh_scene(dim, n)
    S, G, where, margin = mesh_reference(dim, n)
    fmax = np.abs(F).max(axis=0)
    s = imported(pkg, "linear_mesh", dim, n)
    assert s.init(x, np.array(F[:, 0])) == 0
    with pkg.capi.ErrorCalls() as calls:
        st, v, leaf = s.eval_many(y, want_leaf=True)
    inside = check_located(pkg, st, leaf, v, margin, tags)
    assert [c[1] for c in calls] == [pkg.capi.GSL_EDOM]
    got = leaf >= 0
    known = got & (margin >= 0)                                      # hull targets the device kept but the reference rounds out: below
    err = np.abs(v[known] - S[known, 0]).max() / fmax[0]
    print(f"linear_mesh dim {dim} n {n}: {len(simp)} simplices, {got.sum()} of {len(y)} targets located, values {err:.3e} max|f|")
    assert err <= TOL and (leaf[inside] == where[inside]).all()
    assert np.abs(v[tags == "vertex"] - F[:, 0]).max() <= 1e-12 * fmax[0]   # a vertex returns its datum (the skeleton bound of test_gpu_mesh3.py)
    # K = 3 fields and the per-simplex gradients from one locate
    k = pkg.Sinterp("linear_mesh", dim, n, 0)
    assert k.set_triangulation(simp, nbr) == 0 and k.linear_init_fields(x, F) == 0 and k.n_fields() == 3
    with pkg.capi.ErrorCalls():
        stk, Sk, Gk, leafk = k.linear_eval_fields_many(y, want_grad=True, want_leaf=True)
        st1, s1, g1 = k.linear_eval_fields_e(y[n], want_grad=True)
        st2, v2 = s.eval_e(y[n])
    assert stk == st and np.array_equal(leafk, leaf) and np.array_equal(bits(Sk[got, 0]), bits(v[got])) and np.isnan(Sk[~got]).all()
    es = (np.abs(Sk[known] - S[known]).max(axis=0) / fmax).max()
    Gk = Gk.reshape(len(y), 3, dim)
    eg = np.abs(Gk[inside] - G[inside]).max() / np.abs(G[inside]).max()
    print(f"   fields {es:.3e}, gradients {eg:.3e} of max|g| = {np.abs(G[inside]).max():.3e}")
    assert es <= TOL and eg <= TOL and np.isnan(Gk[~got]).all()
    assert st1 == 0 and np.array_equal(bits(s1), bits(Sk[n])) and np.array_equal(bits(g1.reshape(-1)), bits(Gk[n].reshape(-1)))
    assert st2 == 0 and bits(np.array([v2]))[0] == bits(v)[n]
    for j in np.flatnonzero(got & ~(margin >= 0)):                   # kept hull targets: the face's own interpolation, to rounding
        assert abs(margin[j]) <= 1e-12
    d_y, d_s = dev(y), torch.zeros(len(y), dtype=torch.float64, device="cuda")
    with pkg.capi.ErrorCalls():
        assert s.eval_resident(ptr(d_y), len(y), dim, ptr(d_s)) in (0, pkg.capi.GSL_EDOM)
    torch.cuda.synchronize()
    r = d_s.cpu().numpy()
    assert np.array_equal(bits(r[got]), bits(v[got])) and np.isnan(r[~got]).all()
    path = str(tmp_path / "mesh.bin")
    assert s.fwrite(path) == 0
    back = pkg.Sinterp("linear_mesh", dim, n, 0)
    assert back.fread(path) == 0
    with pkg.capi.ErrorCalls():
        stb, vb, leafb = back.eval_many(y, want_leaf=True)
    assert stb == st and np.array_equal(leafb, leaf) and np.array_equal(bits(vb[got]), bits(v[got]))


def tree_mesh(pkg, x):
    """the triangulation the types with a tree of their own build (Delaunay in the tree's per-axis standardised metric, which
    need not be scipy's at 8 sites): triangles, neighbours, and the (shift, scale) of the metric its natural neighbours use"""
    tree = pkg.SimplexTree(2, len(x))
    assert tree.init(x, flags=0, rng=pkg.capi.Rng(0)) == 0
    mesh = pkg.SimplexMesh.from_tree(tree)
    metric = mesh.delaunay_metric()                       # 1: Delaunay as given (what the natural neighbours then use), 2: standardised
    assert metric in (1, 2)
    shift, scale = mesh.geometry() if metric == 2 else (np.zeros(2), np.ones(2))
    return mesh.triangles(), mesh.neighbours(), (shift, scale)


@pytest.mark.parametrize("dim,n", MESHES_2D, ids=idents(MESHES_2D))
def test_linear_simplex(pkg, orc, dim, n):
    """the type that builds its own tree (2-D): the CPU oracle's bits at every finite target (the cage's leaves included),
    and the extended-precision barycentric value strictly inside the tree's triangulation of the sites"""
    x, F, _, _, y, tags = T.mesh_scene(dim, n)
    f = np.array(F[:, 0])
    s = pkg.Sinterp("linear_simplex", dim, n, 0)
    assert s.set_tree_options(0, pkg.capi.Rng(0)) == 0 and s.init(x, f) == 0
    ot = orc.Tree(dim, n)
    assert ot.init(x, flags=0, seed=0) == 0
    fin = np.ascontiguousarray(y[:-1])
    ovals, oleaf = ot.eval_many(x, f, fin)
    with pkg.capi.ErrorCalls():
        st, v, leaf = s.eval_many(y, want_leaf=True)
    assert st in (0, pkg.capi.GSL_EDOM) and np.array_equal(leaf[:-1], oleaf) and np.array_equal(bits(v[:-1]), bits(ovals))
    assert np.isnan(v[-1]) and (leaf[:-1] >= 0).all()                 # the unit box lies inside the cage
    tri, nbr, _ = tree_mesh(pkg, x)
    assert len(tri) == len(T.mesh_scene(dim, n)[2]) and (n > 3 or sorted(tri[0]) == [0, 1, 2])
    S, G, where, margin = T.simplex_linear(x, F, tri.tolist(), y)
    inside = margin > STRICT
    err = np.abs(v[inside] - S[inside, 0]).max() / np.abs(f).max()
    print(f"linear_simplex n {n}: {len(tri)} triangles, {inside.sum()} targets strictly inside, values {err:.3e} max|f|")
    assert err <= TOL and inside.sum() >= 4 * len(tri)
    k = pkg.Sinterp("linear_simplex", dim, n, 0)
    assert k.set_tree_options(0, pkg.capi.Rng(0)) == 0 and k.linear_init_fields(x, F) == 0
    with pkg.capi.ErrorCalls():
        stk, Sk, Gk, leafk = k.linear_eval_fields_many(y, want_grad=True, want_leaf=True)
    assert stk == st and np.array_equal(leafk, leaf) and np.array_equal(bits(Sk[:-1, 0]), bits(v[:-1]))
    Gk = Gk.reshape(len(y), 3, dim)
    es = (np.abs(Sk[inside] - S[inside]).max(axis=0) / np.abs(F).max(axis=0)).max()
    eg = np.abs(Gk[inside] - G[inside]).max() / np.abs(G[inside]).max()
    print(f"   fields {es:.3e}, gradients {eg:.3e}")
    assert es <= TOL and eg <= TOL


@pytest.mark.parametrize("dim,n", MESHES_2D, ids=idents(MESHES_2D))
def test_natural_neighbours(pkg, dim, n):
    from test_gpu_natural import sibson_oracle
    x, F, simp, nbr, y, tags = T.mesh_scene(dim, n)
    S, G, where, margin = mesh_reference(dim, n)
    f = np.array(F[:, 0])
    fmax = np.abs(f).max()
    s = imported(pkg, "natural_mesh", dim, n)
    assert s.init(x, f) == 0
    with pkg.capi.ErrorCalls() as calls:
        st, v, leaf = s.eval_many(y, want_leaf=True)
    inside = check_located(pkg, st, leaf, v, margin, tags)
    assert [c[1] for c in calls] == [pkg.capi.GSL_EDOM]
    assert np.array_equal(bits(v[tags == "vertex"]), bits(f))         # every site returns its datum, bit for bit
    # the oracle takes every located target: strictly inside a triangle, on an interior edge, near the hull -- all but the
    # sites (bits, above) and the points ON the hull, whose Voronoi cell is unbounded (the edge's own interpolation, below)
    cmp = (leaf >= 0) & ~np.isin(tags, ["vertex", "hull"])
    assert (cmp >= inside & (tags != "vertex")).all() and cmp[tags == "interior"].all()
    worst = defect = 0.0
    for j in np.flatnonzero(cmp):
        lam, lp = sibson_oracle(x, y[j])
        defect, worst = max(defect, lp), max(worst, abs(v[j] - lam @ f))
    on_hull = (leaf >= 0) & (tags == "hull")                          # a hull edge: the edge's own linear interpolation
    hull = np.abs(v[on_hull] - S[on_hull, 0]).max() / fmax if (on_hull & (margin >= 0)).any() else 0.0
    print(f"natural_mesh n {n}: {cmp.sum()} targets against the oracle ({(tags == 'interior').sum()} on interior edges), |value - oracle| {worst / fmax:.3e} max|f| (oracle defect {defect:.2e}), "
          f"{on_hull.sum()} hull targets located")
    assert defect <= 1e-12 and worst <= TOL * fmax
    for j in np.flatnonzero(on_hull & (margin >= 0)):
        assert abs(v[j] - S[j, 0]) <= 1e-9 * fmax
    if n == 3:                                                        # one triangle: Sibson's coordinates are the barycentric ones
        assert np.abs(v[inside] - S[inside, 0]).max() <= TOL * fmax
    # the type with a tree of its own: the bits of the imported type on the tree's exported mesh, and the oracle in the
    # metric that mesh is Delaunay in (as given where it is; otherwise the tree's per-axis standardised coordinates)
    t = pkg.Sinterp("natural_simplex", dim, n, 0)
    assert t.set_tree_options(0, pkg.capi.Rng(0)) == 0 and t.init(x, f) == 0
    with pkg.capi.ErrorCalls():
        stt, vt, leaft = t.eval_many(y, want_leaf=True)
    tri, tnbr, (shift, scale) = tree_mesh(pkg, x)
    twin = pkg.Sinterp("natural_mesh", dim, n, 0)
    assert twin.set_triangulation(tri, tnbr) == 0 and twin.init(x, f) == 0
    with pkg.capi.ErrorCalls():
        stw, vw, leafw = twin.eval_many(y, want_leaf=True)
    gt = leaft >= 0
    assert stt == stw and np.array_equal(leaft, leafw) and np.array_equal(bits(vt[gt]), bits(vw[gt])) and np.isnan(vt[~gt]).all()
    assert (leaft[inside] >= 0).all() and np.array_equal(bits(vt[tags == "vertex"]), bits(f))
    xs, worst = (x - shift) * scale, 0.0
    # as above: every located target but the sites and the points on the hull (the convex hull is any triangulation's)
    cmp = gt & ~np.isin(tags, ["vertex", "hull"])
    assert cmp[inside & (tags != "vertex")].all() and cmp[tags == "interior"].all()
    for j in np.flatnonzero(gt & (tags == "hull") & (margin >= 0)):
        assert abs(vt[j] - S[j, 0]) <= 1e-9 * fmax
    for j in np.flatnonzero(cmp):
        lam, lp = sibson_oracle(xs, (y[j] - shift) * scale)
        assert lp <= 1e-12
        worst = max(worst, abs(vt[j] - lam @ f))
    print(f"   natural_simplex: |value - oracle in the tree's metric| {worst / fmax:.3e} max|f|")
    assert worst <= TOL * fmax


@pytest.mark.parametrize("dim,n", MESHES_2D, ids=idents(MESHES_2D))
def test_clough_tocher(pkg, dim, n):
    from scipy.interpolate import CloughTocher2DInterpolator
    from scipy.spatial import Delaunay
    from test_gpu_cubic import GRAD_TOL, dense_gradient_system, restatement
    x, F, simp, nbr, y, tags = T.mesh_scene(dim, n)
    _, _, where, margin = mesh_reference(dim, n)
    f = np.array(F[:, 0])
    fmax = np.abs(f).max()
    d = Delaunay(np.array(x))
    assert sorted(sorted(r) for r in d.simplices.tolist()) == sorted(sorted(r) for r in simp.tolist())
    ct = CloughTocher2DInterpolator(d, f, tol=1e-15, maxiter=100000)
    g = np.ascontiguousarray(ct.grad[:, 0, :])
    s = imported(pkg, "cubic_mesh", dim, n)
    assert s.set_gradients(g) == 0 and s.init(x, f) == 0
    with pkg.capi.ErrorCalls() as calls:
        st, v, leaf = s.eval_many(y, want_leaf=True)
        stg, vg, gr = s.eval_grad_many(y)
    inside = check_located(pkg, st, leaf, v, margin, tags)
    assert stg == st and [c[1] for c in calls] == [pkg.capi.GSL_EDOM] * 2
    got = leaf >= 0
    assert np.array_equal(bits(v[got]), bits(vg[got])) and np.isnan(gr[~got]).all() and np.isfinite(gr[got]).all()
    # every located target but the vertices (below): strictly inside, on interior edges (C1: either triangle's cubic gives
    # the value and the gradient) and on the hull; scipy wherever scipy itself locates the point
    cmp = got & (tags != "vertex")
    assert cmp[inside].all() and cmp[tags == "interior"].all()
    ref = ct(y[cmp])
    fin = np.isfinite(ref)
    assert fin[(inside | (tags == "interior"))[cmp]].all()
    mine, gmine, _ = restatement(np.array(x), np.array(simp), np.array(nbr), f, g, leaf[cmp], y[cmp])
    err, err_r = np.abs(v[cmp][fin] - ref[fin]).max() / fmax, np.abs(v[cmp] - mine).max() / fmax
    eg = np.abs(gr[cmp] - gmine).max() / np.abs(gmine).max()
    print(f"cubic_mesh n {n}: {cmp.sum()} targets ({(tags == 'interior').sum()} on interior edges, {(cmp & (tags == 'hull')).sum()} on the hull), values against scipy {err:.3e}, the restatement {err_r:.3e} max|f|; gradient {eg:.3e} max|grad s|")
    assert err <= TOL and err_r <= TOL and eg <= GRAD_TOL
    assert np.abs(v[tags == "vertex"] - f).max() <= TOL * fmax and np.abs(gr[tags == "vertex"] - g).max() <= GRAD_TOL * np.abs(g).max()
    # the estimated gradients: conjugate gradients on n vertices against the dense solve, as test_gpu_cubic.py bounds it
    e = imported(pkg, "cubic_mesh", dim, n)
    assert e.init(x, f) == 0
    stq, ge, it, res = e.get_gradients()
    A, r = dense_gradient_system(np.array(x), np.array(simp), f)
    g_dense, cond = np.linalg.solve(A, r).reshape(-1, 2), np.linalg.cond(A)
    errg = np.linalg.norm(ge - g_dense) / np.linalg.norm(g_dense)
    print(f"   estimated gradients: {it} iterations, residual {res:.2e}, |g - g_dense| / |g_dense| = {errg:.2e} (cond {cond:.2e})")
    assert stq == 0 and 0 < it < 1000 and res <= 1e-12 and errg <= cond * 1e-12
    # the type with a tree of its own: gradients estimated on ITS triangles, values and gradients by the restatement
    t = pkg.Sinterp("cubic_simplex", dim, n, 0)
    assert t.set_tree_options(0, pkg.capi.Rng(0)) == 0 and t.init(x, f) == 0
    tri, tnbr, _ = tree_mesh(pkg, x)
    stt, gt, itt, rest = t.get_gradients()
    A, r = dense_gradient_system(np.array(x), tri, f)
    g_dense, cond = np.linalg.solve(A, r).reshape(-1, 2), np.linalg.cond(A)
    assert stt == 0 and 0 < itt < 1000 and np.linalg.norm(gt - g_dense) / np.linalg.norm(g_dense) <= cond * 1e-12
    with pkg.capi.ErrorCalls():
        stt, vt, leaft = t.eval_many(y, want_leaf=True)
        _, _, grt = t.eval_grad_many(y)
    assert (leaft[inside] >= 0).all() and stt == (pkg.capi.GSL_EDOM if (leaft < 0).any() else 0)
    cmp = (leaft >= 0) & (tags != "vertex")                           # interior edges and hull points of ITS mesh included
    assert cmp[inside].all() and np.abs(vt[tags == "vertex"] - f).max() <= TOL * fmax
    mine, gmine, _ = restatement(np.array(x), tri, tnbr, f, gt, leaft[cmp], y[cmp])
    err, eg = np.abs(vt[cmp] - mine).max() / fmax, np.abs(grt[cmp] - gmine).max() / np.abs(gmine).max()
    print(f"   cubic_simplex: {len(tri)} triangles, values {err:.3e} max|f|, gradient {eg:.3e} max|grad s|")
    assert err <= TOL and eg <= GRAD_TOL


# ------------------------------------------------------------------------------------------------- 9. modified Shepard
SHEPARD = T.shepard_cases()


@pytest.mark.parametrize("dim,n", SHEPARD, ids=idents(SHEPARD))
def test_shepard_at_its_true_minimum(pkg, dim, n):
    import shepard_ref
    nq = T.SHEPARD_MIN[dim][0]
    x, F, y = T.cloud(dim, n, T.SHEPARD_SALT)
    f = np.array(F[:, 0])
    model = shepard_ref.fit(x, f, nq, nq)
    shepard_ref.self_check(model, y[:-1])
    s_ref, g_ref, leaf_ref = shepard_ref.evaluate(model, y)
    assert not model["coincident"] and np.isfinite(s_ref[:-1]).all() and (model["mode"] == 2).all()
    si = pkg.Sinterp("shepard", dim, n, 0)
    assert si.set_shepard(nq, nq) == 0 and si.init(x, f) == 0
    with pkg.capi.ErrorCalls() as calls:
        st, s, leaf = si.eval_many(y, want_leaf=True)
        st2, s2, g = si.eval_grad_many(y)
    ok = slice(0, len(y) - 1)
    ds, dg = np.abs(s[ok] - s_ref[ok]).max() / np.abs(f).max(), np.abs(g[ok] - g_ref[ok]).max() / np.abs(g_ref[ok]).max()
    print(f"shepard dim {dim} n {n} nq = nw = {nq}: value defect {ds:.3g}, gradient defect {dg:.3g}, leaf {leaf[ok].min()}..{leaf[ok].max()}")
    assert st == 0 and st2 == 0 and calls == []                      # a NaN coordinate: NaN and no error; the box is covered
    assert np.isnan(s[-1]) and np.isnan(g[-1]).all() and leaf[-1] == -1
    assert ds <= TOL and dg <= TOL and (leaf == leaf_ref).all()
    assert (bits(s[ok]) == bits(s2[ok])).all() and np.array_equal(bits(s[:n]), bits(f))
    stt = si.shepard_stats()
    assert stt[:3] == (0, 0, 0) and stt[3] == pytest.approx(model["rw"].max(), rel=1e-13)
    stg, gn, _, _ = si.get_gradients()                               # the nodal gradients: the linear coefficients over Rq
    want = model["coef"][:, :dim] / model["rq"][:, None]
    assert stg == 0 and np.abs(gn - want).max() <= TOL * np.abs(want).max()
    if n == T.SHEPARD_MIN[dim][1]:                                   # every node's neighbourhood is the whole cloud
        assert (leaf[n:-1] >= 1).all() and np.isfinite(model["rw"]).all()


# ------------------------------------------------------------------------------------------------- 10. impossible models
# The contract: the init, or the first entry that cannot answer, returns a nonzero status through the error handler; no
# entry returns success with a non-finite (or meaningless) weight or value; a later init of the same object on good data
# works and gives the bits of a fresh object.
def refused(pkg, call, status):
    with pkg.capi.ErrorCalls() as calls:
        got = call()
    got = got[0] if isinstance(got, tuple) else got
    assert got == status and calls and calls[-1][1] == status, (got, calls)


def nothing_evaluates(pkg, s, y):
    E = pkg.capi
    with E.ErrorCalls() as calls:
        assert s.eval_many(y)[0] == E.GSL_EINVAL and s.eval_e(y[0])[0] == E.GSL_EINVAL and s.weights()[0] == E.GSL_EINVAL
        assert s.eval_grad_many(y)[0] == E.GSL_EINVAL and s.fwrite("/dev/null") == E.GSL_EINVAL
    assert len(calls) == 5 and all(c[1] == E.GSL_EINVAL for c in calls)


def same_bits_as_fresh(pkg, s, fresh, x, f, y):
    assert s.init(x, f) == 0 and fresh.init(x, f) == 0
    (st, a, _), (st2, b, _) = s.eval_many(y), fresh.eval_many(y)
    assert st == 0 and st2 == 0 and np.isfinite(a[:-1]).all() and (bits(a) == bits(b)).all()
    assert (bits(s.weights()[1]) == bits(fresh.weights()[1])).all()


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_thin_plate_spline_on_one_site_is_refused(pkg, dim):
    """Phi = [0]: GSL_EDOM from the init whatever the solver (the shifted route cannot factor, the pivoted LU meets a zero
    pivot), and the object stays uninitialised.  Pinned as found; what changed is that nothing evaluates afterwards."""
    x, F, y = T.cloud(dim, 1)
    for solver in (None, 3):                                          # the Cholesky-type solvers 1 and 2 are not offered to this type
        s = pkg.Sinterp("tps", dim, 1, 0)
        if solver is not None:
            with pkg.capi.ErrorCalls():
                assert s.set_solver(1) == pkg.GSL_EINVAL and s.set_solver(2) == pkg.GSL_EINVAL
            assert s.set_solver(solver) == 0
        refused(pkg, lambda: s.init(x, np.array(F[:, 0])), pkg.GSL_EDOM)
        nothing_evaluates(pkg, s, y)


@pytest.mark.parametrize("n", [3, 4])
def test_thin_plate_splines_on_collinear_centres(pkg, n):
    """2-D centres on a line.  The plain thin-plate matrix stays regular there (cond asserted), so that type must either
    refuse or be right: it is right, through whichever route the cascade ends on.  The affine tail [1, x, y] is NOT
    determined on a line: GSL_EDOM from the init, nothing evaluates, and good data afterwards gives a fresh object's bits."""
    t = np.linspace(0.1, 0.9, n)
    line = np.ascontiguousarray(np.column_stack([t, 0.25 + 0.5 * t]))
    f = np.sin(3.0 * t) + 2.0
    _, _, y = T.cloud(2, n)
    assert np.linalg.cond(T.system_matrix("tps", 2, line)) <= T.COND_CAP
    m = T.fit("tps", 2, line, f)
    s = pkg.Sinterp("tps", 2, n, 0)
    with pkg.capi.ErrorCalls() as calls:
        assert s.init(line, f) == 0 and calls == []
    (st, w), (st2, got, _) = s.weights(), s.eval_many(y)
    assert st == 0 and st2 == 0 and coef_err(w, m.w[:, 0], np.abs(f).max()) <= TOL
    assert np.abs(got[:-1] - m.values(y[:-1])[:, 0]).max() <= TOL * np.abs(f).max() and np.isnan(got[-1])
    a = pkg.Sinterp("tps_affine", 2, n, 0)
    refused(pkg, lambda: a.init(line, f), pkg.GSL_EDOM)
    refused(pkg, lambda: a.init_fields(line, np.column_stack([f, f * f])), pkg.GSL_EDOM)
    nothing_evaluates(pkg, a, y)
    assert a.poly()[0] == pkg.GSL_EINVAL
    x, F, _ = T.cloud(2, n)
    same_bits_as_fresh(pkg, a, pkg.Sinterp("tps_affine", 2, n, 0), x, np.array(F[:, 0]), y)


def test_affine_thin_plate_spline_on_coplanar_centres(pkg):
    rng = np.random.default_rng(T.SEED)
    uv = rng.random((6, 2))
    plane = np.ascontiguousarray(np.column_stack([uv[:, 0], uv[:, 1], 0.2 + 0.3 * uv[:, 0] + 0.4 * uv[:, 1]]))
    a = pkg.Sinterp("tps_affine", 3, 6, 0)
    refused(pkg, lambda: a.init(plane, np.cos(uv[:, 0])), pkg.GSL_EDOM)
    x, F, y = T.cloud(3, 6)
    nothing_evaluates(pkg, a, y)
    three = pkg.Sinterp("tps_affine", 3, 3, 0)                         # min_size 3 is accepted, but three sites are always coplanar
    refused(pkg, lambda: three.init(np.ascontiguousarray(x[:3]), np.array(F[:3, 0])), pkg.GSL_EDOM)
    same_bits_as_fresh(pkg, a, pkg.Sinterp("tps_affine", 3, 6, 0), x, np.array(F[:, 0]), y)


@pytest.mark.parametrize("typ", T.KRIGE_TYPES)
@pytest.mark.parametrize("dim,drift", [(1, 0), (2, 0), (3, 0), (1, 1), (2, 1), (2, 2), (3, 1)])
def test_kriging_leave_one_out_needs_more_sites_than_terms(pkg, typ, dim, drift):
    """N = 1 (ordinary kriging) and N = q (universal kriging): the model exists and evaluates, the model WITHOUT a site does
    not -- Dubrule's diagonal is 0 / 0.  The accessors answer GSL_EDOM and store nothing (they used to return NaN, +-inf
    and 1e15 with GSL_SUCCESS)."""
    n = ukrige_ref.n_terms(dim, drift) if drift else 1
    x, F, y = T.cloud(dim, n)
    f = np.array(F[:, 0])
    for variance in (False, True):
        s = make(pkg, typ, dim, n, drift, loo=True, variance=variance)
        with pkg.capi.ErrorCalls() as calls:
            assert s.init(x, f) == 0 and calls == []
        E0, v0 = np.full((n, 1), 7.0), np.full(n, 7.0)
        refused(pkg, lambda: s.loo_residuals(out=E0), pkg.GSL_EDOM)
        refused(pkg, lambda: s.loo_variance(out=v0), pkg.GSL_EDOM)
        assert (E0 == 7.0).all() and (v0 == 7.0).all()
        st, got, _ = s.eval_many(y)                                   # the model itself is fine
        _, want = reference(typ, dim, n, drift)
        assert st == 0 and np.abs(got[:-1] - want[:, 0]).max() <= TOL * np.abs(f).max()
    K5 = make(pkg, typ, dim, n, drift, loo=True)
    assert K5.init_fields(x, np.ascontiguousarray(F[:, :5])) == 0
    refused(pkg, lambda: K5.loo_residuals(out=np.zeros((n, 5))), pkg.GSL_EDOM)
    plain = make(pkg, typ, dim, n, drift)                             # not asked for: the older status, unchanged
    assert plain.init(x, f) == 0
    refused(pkg, lambda: plain.loo_variance(), pkg.GSL_EINVAL)


@pytest.mark.parametrize("typ", T.KRIGE_TYPES)
@pytest.mark.parametrize("dim,drift", [(1, 1), (2, 1), (3, 1), (1, 2), (2, 2), (3, 2)])
def test_a_drift_needs_as_many_sites_as_terms(pkg, typ, dim, drift):
    """N = q - 1: GSL_EINVAL from the init (pinned as found), nothing evaluates; without the drift the same object works"""
    n = ukrige_ref.n_terms(dim, drift) - 1
    x, F, y = T.cloud(dim, n)
    f = np.array(F[:, 0])
    s = make(pkg, typ, dim, n, drift)
    refused(pkg, lambda: s.init(x, f), pkg.GSL_EINVAL)
    refused(pkg, lambda: s.init_fields(x, np.ascontiguousarray(F[:, :5])), pkg.GSL_EINVAL)
    nothing_evaluates(pkg, s, y)
    assert s.drift_coefficients()[0] == pkg.GSL_EINVAL
    assert s.set_drift(0) == 0
    same_bits_as_fresh(pkg, s, make(pkg, typ, dim, n), x, f, y)


@pytest.mark.parametrize("kind", ["linear_mesh", "natural_mesh", "cubic_mesh"])
def test_an_imported_mesh_whose_only_triangle_is_flat(pkg, kind):
    """Pinned as found: the triangulation is accepted and initialised (a flat triangle contains nothing), and the first
    entry that cannot answer says so -- every target is outside: GSL_EDOM, NaN, triangle -1.  A good triangle afterwards
    gives a fresh object's bits."""
    flat = np.array([[0.1, 0.1], [0.5, 0.5], [0.9, 0.9]])
    tri = np.array([[0, 1, 2]], dtype=np.int32)
    f = np.array([1.0, 2.0, 3.0])
    y = np.array([[0.2, 0.3], [0.7, 0.1], [0.4, 0.2], [np.nan, 0.1]])   # off the triangle's own line
    s = pkg.Sinterp(kind, 2, 3, 0)
    with pkg.capi.ErrorCalls() as calls:
        assert s.set_triangulation(tri) == 0 and s.init(flat, f) == 0 and calls == []
    with pkg.capi.ErrorCalls() as calls:
        st, v, leaf = s.eval_many(y, want_leaf=True)
    assert st == pkg.capi.GSL_EDOM and [c[1] for c in calls] == [pkg.capi.GSL_EDOM]
    with pkg.capi.ErrorCalls() as calls:                              # one target: by status (the handler is the type's own matter)
        st1, v1 = s.eval_e(y[0])
    assert st1 == pkg.capi.GSL_EDOM and all(c[1] == pkg.capi.GSL_EDOM for c in calls)
    assert np.isnan(v).all() and np.isnan(v1) and (leaf == -1).all()
    if kind == "cubic_mesh":
        with pkg.capi.ErrorCalls():
            stg, vg, g = s.eval_grad_many(y)
        assert stg == pkg.capi.GSL_EDOM and np.isnan(vg).all() and np.isnan(g).all()
    x, F, simp, nbr, yy, _ = T.mesh_scene(2, 3)
    fresh = pkg.Sinterp(kind, 2, 3, 0)
    assert s.set_triangulation(simp, nbr) == 0 and fresh.set_triangulation(simp, nbr) == 0
    assert s.init(x, np.array(F[:, 0])) == 0 and fresh.init(x, np.array(F[:, 0])) == 0
    with pkg.capi.ErrorCalls():
        (sa, a, la), (sb, b, lb) = s.eval_many(yy, want_leaf=True), fresh.eval_many(yy, want_leaf=True)
    assert sa == sb and np.array_equal(la, lb) and (la >= 0).sum() >= 8 and np.array_equal(bits(a[la >= 0]), bits(b[la >= 0]))


@pytest.mark.parametrize("dim", [2, 3])
def test_shepard_below_max_nq_nw_plus_two(pkg, dim):
    """size = max(nq, nw) + 1: GSL_EINVAL from the init (pinned as found), nothing evaluates; with the counts lowered to the
    size's own minimum (2-D) / on a cloud of its own size (3-D) the object works.  Below the type's min_size of 7 there is
    no object at all."""
    E = pkg.capi
    with pytest.raises(E.GslError):
        pkg.Sinterp("shepard", dim, 6, 0)
    nq, n = T.SHEPARD_MIN[dim]
    x, F, y = T.cloud(dim, n, T.SHEPARD_SALT)
    f = np.array(F[:, 0])
    s = pkg.Sinterp("shepard", dim, n, 0)
    assert s.set_shepard(nq + 1, nq) == 0
    refused(pkg, lambda: s.init(x, f), E.GSL_EINVAL)
    with E.ErrorCalls() as calls:
        assert s.eval_many(y)[0] == E.GSL_EINVAL and s.eval_grad_many(y)[0] == E.GSL_EINVAL and s.shepard_stats()[0] != 0
    assert len(calls) == 3
    d = pkg.Sinterp("shepard", dim, n, 0)                              # Renka's defaults need 21 / 34 sites
    refused(pkg, lambda: d.init(x, f), E.GSL_EINVAL)
    fresh = pkg.Sinterp("shepard", dim, n, 0)
    assert s.set_shepard(nq, nq) == 0 and fresh.set_shepard(nq, nq) == 0 and s.init(x, f) == 0 and fresh.init(x, f) == 0
    (st, a, _), (st2, b, _) = s.eval_many(y), fresh.eval_many(y)
    assert st == 0 and st2 == 0 and np.isfinite(a[:-1]).all() and (bits(a) == bits(b)).all()
