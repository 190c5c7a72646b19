"""-m gpu: K responses and per-simplex gradients of the piecewise-linear types from one locate
(csrc/hip/linear_fields.hip; DESIGN.md 4, "Several responses on a mesh"; CPU part: tests/test_linear_fields_api.py).

Three routes: the history DAG of a SimplexTree over N = 200 random sites of the unit square, the QHull triangulation of
the same sites imported as a 2-D mesh, and the QHull tetrahedralisation of N = 150 random sites of the unit cube.

Values are compared BIT FOR BIT with the scalar entry bound to one column at a time.

Gradient tolerance.  The reference is the gradient of the plane through the located simplex's vertex data, from the raw
vertex coordinates in np.longdouble (Cramer's rule); the bound per simplex is  C_GRAD u kappa_2(E) |g_ref|_2,  u = 2^-53,
E = the raw edge matrix, kappa_2 by np.linalg.cond.  C_GRAD is not a guess: it is 16 x the worst ratio to u kappa_2 |g| that
numpy's own float64 solve of the same systems (every simplex a target can be located in x the 64 fields of this file)
shows against the longdouble result, per route, rounded down.  Measured on the CPU by numpy_solve_ratio() below, which
test_gradients prints again:
    tree (401 leaves, the 20 cage leaves included)   3.245   ->  C_GRAD = 51
    2-D mesh (QHull triangles)                       2.586   ->  C_GRAD = 41
    3-D mesh (QHull tetrahedra)                      3.912   ->  C_GRAD = 62"""
import os

import numpy as np
import pytest
import torch

from gpu_util import CANARY, Canaried, bits
from test_mesh3_api import qhull

pytestmark = pytest.mark.gpu

N2, N3, KMAX = 200, 150, 64
KS = (1, 3, 8, 64)
U = 2.0 ** -53
C_GRAD = {"tree": 51.0, "mesh2": 41.0, "mesh3": 62.0}      # 16 x numpy_solve_ratio, rounded down (module docstring)
LD = np.longdouble
AFFINE = {2: (0.25, np.array([1.25, -0.75])), 3: (0.25, np.array([1.25, -0.75, 0.5]))}


def sites(dim):
    """random sites on the 2^-26 grid of the unit box: with AFFINE's few-bit coefficients a + b . x is then exact in fp64, so
    that the affine check below measures the sweep and not the rounding of its own data"""
    r = np.random.default_rng(10 + dim).random((N2 if dim == 2 else N3, dim))
    return np.ascontiguousarray(np.floor(r * 2.0 ** 26) / 2.0 ** 26)


def responses(x):
    """n x 64: column 0 is affine in the coordinates (exactly), the others are noise (nothing a smooth field would hide)"""
    F = np.random.default_rng(20 + x.shape[1]).standard_normal((len(x), KMAX))
    a, b = AFFINE[x.shape[1]]
    F[:, 0] = a + x @ b
    return np.ascontiguousarray(F)


def sort_threshold(pkg):
    """the smallest batch the located sweeps reorder, from the route helper (monotone in m)"""
    want = pkg.lib().gsl_sinterp_hip_sort_wanted
    assert not want(1) and want(1 << 24)
    lo, hi = 1, 1 << 24
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if want(mid) else (mid, hi)
    return hi


_scenes = {}


def scene(pkg, route):
    """one route: mirror, the raw vertex coordinates V [n, d + 1, d] and data rows ROW [n, d + 1] (-1 = cage vertex) of
    every simplex (DAG node), cand = the ones a target can be located in (the leaves), the target pool, and the scalar
    reference of every column"""
    if route in _scenes:
        return _scenes[route]
    dim = 3 if route == "mesh3" else 2
    x = sites(dim)
    F = responses(x)
    sc = {"dim": dim, "x": x, "F": F, "route": route}
    if route == "tree":
        tree = pkg.SimplexTree(2, len(x))
        assert tree.init(x, flags=0, rng=pkg.capi.Rng(0)) == 0
        _, pidx, _ = tree.arrays()
        pidx = pidx.reshape(-1, 3)
        seed = tree.geom()[:6].reshape(3, 2)
        row = np.where(pidx >= 0, tree.shuffle().astype(np.int64)[np.clip(pidx, 0, None)], -1)
        V = np.where((pidx >= 0)[:, :, None], x[np.clip(row, 0, None)], seed[np.clip(-pidx - 1, 0, 2)])
        sc.update(keep=tree, dev=tree.device_alloc(0), far=100.0 * np.abs(seed).max(), cand=np.nonzero(tree.arrays()[0] == 0)[0])
    else:
        _, simp, nbr = qhull(x)
        mesh = pkg.SimplexMesh.from_arrays(x, simp, nbr)
        row, V = simp.astype(np.int64), x[simp]
        sc.update(keep=mesh, dev=mesh.device_alloc(0), far=1e3, simp=simp, nbr=nbr, cand=np.arange(len(simp)))
    sc.update(ROW=row, V=np.ascontiguousarray(V, dtype=np.float64))
    # the pool: an interior point first (a batch of one succeeds), then far outside, sites, edge midpoints, points outside
    # the data hull (inside the cage of the tree route), then uniform points of the slightly enlarged bounding box
    thr = sort_threshold(pkg)
    rng = np.random.default_rng(30 + dim)
    data = sc["cand"][(row[sc["cand"]] >= 0).all(axis=1)]
    t = data[rng.integers(0, len(data), 20)]
    mid = 0.5 * (V[t, 0] + V[t, 1])
    ring = 0.5 + (0.6 + 0.3 * rng.random((20, 1))) * np.where(rng.random((20, dim)) < 0.5, -1.0, 1.0)
    y = np.concatenate([x.mean(axis=0, keepdims=True), np.full((3, dim), sc["far"]) * [[1], [-1], [1]], x[:20], mid, ring,
                        -0.05 + 1.1 * rng.random((thr, dim))])
    y[2, 0] = np.nan                                                          # a NaN coordinate: whatever the locate stores
    sc["y"] = np.ascontiguousarray(y)
    sc["batches"] = (1, 65, thr - 1, thr)
    # scalar reference: every column bound in turn, every batch size
    ref = {m: (np.empty((m, KMAX)), None, None) for m in sc["batches"]}
    for q in range(KMAX):
        assert sc["dev"].set_response(np.ascontiguousarray(F[:, q])) == 0
        for m in sc["batches"]:
            st, v, leaf = sc["dev"].eval_many(np.ascontiguousarray(sc["y"][:m]))
            ref[m][0][:, q] = v
            if q == 0:
                ref[m] = (ref[m][0], leaf.copy(), st)
            assert np.array_equal(leaf, ref[m][1]) and st == ref[m][2]
    sc["ref"] = ref
    _scenes[route] = sc
    return sc


def reference_gradients(V, fv):
    """the plane through the vertex data, in longdouble: V [t, d + 1, d] raw coordinates, fv [t, d + 1, K] -> g [t, K, d];
    also the float64 edge matrix A (rows = edges v_i - v_last)"""
    Vl, fl = V.astype(LD), fv.astype(LD)
    d = V.shape[2]
    A = Vl[:, :d, :] - Vl[:, d:, :]
    df = fl[:, :d, :] - fl[:, d:, :]
    if d == 2:
        det = A[:, 0, 0] * A[:, 1, 1] - A[:, 0, 1] * A[:, 1, 0]
        inv = np.empty_like(A)
        inv[:, 0, 0], inv[:, 0, 1], inv[:, 1, 0], inv[:, 1, 1] = A[:, 1, 1], -A[:, 0, 1], -A[:, 1, 0], A[:, 0, 0]
    else:
        c = [np.cross(A[:, 1], A[:, 2]), np.cross(A[:, 2], A[:, 0]), np.cross(A[:, 0], A[:, 1])]
        det = (A[:, 0] * c[0]).sum(axis=1)
        inv = np.stack(c, axis=2)
    return np.einsum("tai,tik->tka", inv / det[:, None, None], df), V[:, :d, :] - V[:, d:, :]


def vertex_data(sc, F):
    return np.where((sc["ROW"] >= 0)[:, :, None], F[np.clip(sc["ROW"], 0, None)], 0.0)


def numpy_solve_ratio(sc):
    """worst |g_numpy64 - g_longdouble| / (u kappa_2 |g|) over every simplex and field of the route: what C_GRAD is 16 x"""
    fv = vertex_data(sc, sc["F"])[sc["cand"]]
    g, A = reference_gradients(sc["V"][sc["cand"]], fv)
    d = sc["dim"]
    g64 = np.transpose(np.linalg.solve(A, fv[:, :d, :] - fv[:, d:, :]), (0, 2, 1))
    err = np.sqrt(((g64.astype(LD) - g) ** 2).sum(axis=2)).astype(np.float64)
    gn = np.sqrt((g ** 2).sum(axis=2)).astype(np.float64)
    return (err / (U * np.linalg.cond(A)[:, None] * gn)).max()


ROUTES = ("tree", "mesh2", "mesh3")


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("route", ROUTES)
def test_values_are_the_scalar_bits(pkg, route, K):
    sc = scene(pkg, route)
    dev, thr = sc["dev"], sc["batches"][-1]
    assert dev.set_responses(sc["F"][:, :K]) == 0 and dev.n_responses() == K      # a view: F->tda = 64
    for m in sc["batches"]:
        y = np.ascontiguousarray(sc["y"][:m])
        want, leaf_ref, st_ref = sc["ref"][m]
        with pkg.capi.ErrorCalls() as calls:
            st, S, _, leaf = dev.eval_fields_many(y)
        assert st == st_ref == (0 if m == 1 else pkg.capi.GSL_EDOM) and len(calls) == (st != 0)
        assert np.array_equal(leaf, leaf_ref)
        assert np.array_equal(bits(S), bits(want[:, :K])), (route, K, m)        # NaN rows included: one quiet NaN
        out = leaf < 0
        assert np.isnan(S[out]).all() and np.isfinite(S[~out & ~np.isnan(y).any(axis=1)]).all()
        if m >= 65:
            # far outside; sites and midpoints inside.  Row 2 has a NaN coordinate: whatever the locate stored (the DAG walk
            # leaves it in a leaf with a NaN value, the mesh walks call it outside), the bits above are the scalar entry's
            assert out[1] and out[3] and np.isnan(S[2]).all() and not out[4:44].any()
            if route == "tree":                                                  # outside the hull, inside the cage: masked leaves
                assert not out[44:64].any() and (sc["ROW"][leaf[44:64]] < 0).any()
            else:
                assert out[44:64].all()
    assert sc["batches"] == (1, 65, thr - 1, thr) and not pkg.lib().gsl_sinterp_hip_sort_wanted(thr - 1)


@pytest.mark.parametrize("route", ROUTES)
def test_layouts_and_resident_entry(pkg, route):
    sc = scene(pkg, route)
    dev, dim, K, m = sc["dev"], sc["dim"], 3, 65
    Fwide = np.full((len(sc["x"]), K + 2), np.nan)
    Fwide[:, :K] = sc["F"][:, 5:5 + K]
    assert dev.set_responses(Fwide[:, :K]) == 0                                   # F->tda = K + 2, NaN in the padding
    ywide = np.full((m, dim + 3), np.nan)
    ywide[:, :dim] = sc["y"][:m]
    sentinel = np.frombuffer(np.uint64(CANARY).tobytes(), dtype=np.float64)[0]
    Sw, Gw = np.full((m, K + 1), sentinel), np.full((m, K * dim + 5), sentinel)
    st, S, G, leaf = dev.eval_fields_many(ywide[:, :dim], want_grad=True, out=(Sw[:, :K], Gw[:, :K * dim]))
    assert st == pkg.capi.GSL_EDOM
    assert (bits(Sw[:, K:]) == CANARY).all() and (bits(Gw[:, K * dim:]) == CANARY).all()
    st0, S0, G0, leaf0 = dev.eval_fields_many(np.ascontiguousarray(sc["y"][:m]), want_grad=True)
    assert np.array_equal(bits(S), bits(S0)) and np.array_equal(bits(G), bits(G0)) and np.array_equal(leaf, leaf0)
    assert np.array_equal(bits(S0), bits(sc["ref"][m][0][:, 5:5 + K]))
    # resident: ttda, stda and gtda above the minimum, 8-byte aligned bases, nothing read back
    Y, Sd, Gd = Canaried(sc["y"][:m], ld=dim + 1, off=1), Canaried(np.zeros((m, K)), ld=K + 2, off=1), Canaried(np.zeros((m, K * dim)), ld=K * dim + 3, off=1)
    tl = torch.full((m,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with pkg.capi.ErrorCalls() as calls:
        assert dev.eval_fields_resident(Y.ptr, m, dim + 1, Sd.ptr, K + 2, Gd.ptr, K * dim + 3, tl.data_ptr()) == 0
        assert dev.eval_fields_resident(Y.ptr, 0, dim + 1, Sd.ptr, K + 2, Gd.ptr, K * dim + 3, tl.data_ptr()) == 0
    torch.cuda.synchronize()
    assert not calls
    assert np.array_equal(bits(Sd.get()), bits(S0)) and np.array_equal(bits(Gd.get()), bits(G0)) and np.array_equal(tl.cpu().numpy(), leaf0)
    assert Y.padding_intact() and Sd.padding_intact() and Gd.padding_intact()
    # no index array, no gradient: the same value bits
    S2 = Canaried(np.zeros((m, K)), ld=K)
    torch.cuda.synchronize()
    assert dev.eval_fields_resident(Y.ptr, m, dim + 1, S2.ptr, K) == 0
    torch.cuda.synchronize()
    assert np.array_equal(bits(S2.get()), bits(S0)) and S2.padding_intact()
    # statuses of the mirror entries, each one handler call
    E = pkg.capi
    for args, want in (((Y.ptr, m, dim + 1, Sd.ptr, K - 1), E.GSL_EINVAL), ((Y.ptr, m, dim + 1, Sd.ptr, K, Gd.ptr, K * dim - 1), E.GSL_EINVAL),
                       ((Y.ptr, m, dim - 1, Sd.ptr, K), E.GSL_EBADLEN), ((None, m, dim, Sd.ptr, K), E.GSL_EFAULT)):
        with pkg.capi.ErrorCalls() as calls:
            assert dev.eval_fields_resident(*args) == want
        assert len(calls) == 1
    with pkg.capi.ErrorCalls() as calls:
        assert dev.set_responses(np.zeros((len(sc["x"]), KMAX + 1))) == E.GSL_EINVAL
        assert dev.set_responses(np.zeros((len(sc["x"]) - 1, 2))) == E.GSL_EBADLEN
        assert dev.eval_fields_many(np.zeros((2, dim + 1)))[0] == E.GSL_EBADLEN
    assert len(calls) == 3 and dev.n_responses() == K


@pytest.mark.parametrize("route", ROUTES)
def test_gradients(pkg, route):
    sc = scene(pkg, route)
    dev, dim, K = sc["dev"], sc["dim"], 8
    m = sc["batches"][-1]
    y = np.ascontiguousarray(sc["y"][:m])
    ratio = numpy_solve_ratio(sc)
    print(f"{route}: numpy float64 solve, worst ratio to u kappa_2 |g|: {ratio:.3f} (C_GRAD = {C_GRAD[route]})")
    assert dev.set_responses(sc["F"][:, :K]) == 0
    st, S, G, leaf = dev.eval_fields_many(y, want_grad=True)
    st1, S1, _, leaf1 = dev.eval_fields_many(y)
    assert st == st1 == pkg.capi.GSL_EDOM and np.array_equal(leaf, leaf1)
    assert np.array_equal(bits(S), bits(S1))                                     # the value bits do not depend on G
    assert np.array_equal(bits(S), bits(sc["ref"][m][0][:, :K]))
    out = leaf < 0
    assert out.any() and np.isnan(G[out]).all() and np.isnan(S[out]).all() and np.isfinite(G[~out]).all()   # G: no function of the target
    G = G.reshape(m, K, dim)
    # constant per simplex: every target of a simplex carries the bits of the first one
    ids, first, count = np.unique(leaf[~out], return_index=True, return_counts=True)
    rows = np.nonzero(~out)[0]
    assert count.max() >= 2
    assert np.array_equal(bits(G[~out]), bits(G[rows[first]][np.searchsorted(ids, leaf[~out])]))
    # against the longdouble plane of every simplex hit
    g_ref, A = reference_gradients(sc["V"][ids], vertex_data(sc, sc["F"][:, :K])[ids])
    kappa = np.linalg.cond(A)
    got = G[rows[first]]
    err = np.sqrt(((got.astype(LD) - g_ref) ** 2).sum(axis=2)).astype(np.float64)
    gn = np.sqrt((g_ref ** 2).sum(axis=2)).astype(np.float64)
    worst = (err / (U * kappa[:, None] * gn)).max()
    print(f"{route}: {len(ids)} simplices hit, kappa_2 up to {kappa.max():.3g}, worst gradient error / (u kappa_2 |g_ref|) = {worst:.3f}")
    assert (err <= C_GRAD[route] * U * kappa[:, None] * gn).all()
    # the affine column returns its slope wherever all vertices carry data
    whole = (sc["ROW"][ids] >= 0).all(axis=1)
    b = AFFINE[dim][1]
    eb = np.sqrt(((got[whole, 0, :] - b) ** 2).sum(axis=1))
    print(f"{route}: affine field, worst |g - b| / (u kappa_2 |b|) = {(eb / (U * kappa[whole] * np.linalg.norm(b))).max():.3f}")
    assert whole.sum() > 50 and (eb <= C_GRAD[route] * U * kappa[whole] * np.linalg.norm(b)).all()
    if route == "tree":
        assert (~whole).any()                                                    # cage leaves took part: their vertices carry 0


def test_raw_entry_strided_fields_and_statuses(pkg):
    """gsl_sinterp_hip_bary_fields_eval on raw arrays: ftda > nf with an 8-byte aligned base, odd nf, and the statuses that
    are decided before anything touches the device"""
    sc = scene(pkg, "tree")
    tree, x, m = sc["keep"], sc["x"], 65
    types, pidx, links = tree.arrays()
    n, geom, shuffle = tree.n_nodes, tree.geom(), tree.shuffle()
    ctx = pkg.HipContext.on_torch_stream(0)
    dv = lambda a, t: torch.from_numpy(np.ascontiguousarray(a)).to(t).cuda()
    d_type, d_pidx, d_links, d_pts = dv(types, torch.int32), dv(pidx, torch.int32), dv(links, torch.int32), dv(x[shuffle], torch.float64)
    rec = torch.empty(n * 8 + 8, dtype=torch.float64, device="cuda")
    rec_ptr = (rec.data_ptr() + 63) // 64 * 64
    tab = torch.zeros(n * 4, dtype=torch.float64, device="cuda")
    ctx.tree_pack(n, d_type.data_ptr(), d_pidx.data_ptr(), d_links.data_ptr(), len(x), d_pts.data_ptr(), geom, rec_ptr)
    d_y = dv(sc["y"][:m], torch.float64)
    vals = torch.empty(m, dtype=torch.float64, device="cuda")
    loc = torch.empty(m, dtype=torch.int32, device="cuda")
    ctx.bary_eval(n, rec_ptr, tab.data_ptr(), geom[8:10], d_y.data_ptr(), m, 2, vals.data_ptr(), loc.data_ptr())
    ctx.sync()
    assert np.array_equal(loc.cpu().numpy(), sc["ref"][m][1])
    L, scale = pkg.lib(), np.ascontiguousarray(geom[8:10])
    sp = scale.ctypes.data_as(pkg.capi._pd)
    for nf, ftda in ((1, 1), (3, 4), (5, 7), (64, 65)):
        Fd = Canaried(sc["F"][shuffle][:, :nf], ld=ftda, off=1)
        S, G = Canaried(np.zeros((m, nf)), ld=nf + 1, off=1), Canaried(np.zeros((m, 2 * nf)), ld=2 * nf + 1)
        torch.cuda.synchronize()
        assert L.gsl_sinterp_hip_bary_fields_eval(ctx._h, n, rec_ptr, d_pidx.data_ptr(), len(x), Fd.ptr, nf, ftda, sp, loc.data_ptr(),
                                                  d_y.data_ptr(), m, 2, S.ptr, nf + 1, G.ptr, 2 * nf + 1) == 0
        ctx.sync()
        assert np.array_equal(bits(S.get()), bits(sc["ref"][m][0][:, :nf])), nf
        assert Fd.padding_intact() and S.padding_intact() and G.padding_intact()
    E = pkg.capi
    ok = dict(nf=3, ftda=3, ttda=2, stda=3, g=G.ptr, gtda=6, rec=rec_ptr, loc=loc.data_ptr(), m=m)
    for change, want in ((dict(nf=0), E.GSL_EINVAL), (dict(nf=65, ftda=65, stda=65, gtda=130), E.GSL_EINVAL), (dict(ftda=2), E.GSL_EINVAL),
                         (dict(stda=2), E.GSL_EINVAL), (dict(gtda=5), E.GSL_EINVAL), (dict(ttda=1), E.GSL_EINVAL), (dict(rec=None), E.GSL_EFAULT),
                         (dict(loc=None), E.GSL_EFAULT), (dict(m=0, loc=None), 0), (dict(g=None, gtda=0), 0)):
        a = dict(ok, **change)
        st = L.gsl_sinterp_hip_bary_fields_eval(ctx._h, n, a["rec"], d_pidx.data_ptr(), len(x), Fd.ptr, a["nf"], a["ftda"], sp, a["loc"],
                                                d_y.data_ptr(), a["m"], a["ttda"], S.ptr, a["stda"], a["g"], a["gtda"])
        assert st == want, (change, st)
    assert L.gsl_sinterp_hip_bary_fields_eval(None, n, rec_ptr, d_pidx.data_ptr(), len(x), Fd.ptr, 3, 3, sp, loc.data_ptr(), d_y.data_ptr(), m, 2,
                                              S.ptr, 3, None, 0) == E.GSL_EFAULT
    ctx.sync()


def reseed(pkg, s, kind):
    """the tree of the scene: same flags, a generator in the same state (every init draws from it)"""
    if kind == "linear_simplex":
        assert s.set_tree_options(0, pkg.capi.Rng(0)) == 0


def facade(pkg, sc, kind):
    s = pkg.Sinterp(kind, sc["dim"], len(sc["x"]), 0)
    reseed(pkg, s, kind)
    if kind == "linear_mesh":
        assert s.set_triangulation(sc["simp"], sc["nbr"]) == 0
    return s


@pytest.mark.parametrize("route,kind", [("tree", "linear_simplex"), ("mesh2", "linear_mesh"), ("mesh3", "linear_mesh")])
def test_facade(pkg, route, kind, tmp_path):
    sc = scene(pkg, route)
    x, F, dim, m, K = sc["x"], sc["F"], sc["dim"], 65, 3
    y = np.ascontiguousarray(sc["y"][:m])
    want, leaf_ref, _ = sc["ref"][m]
    E = pkg.capi
    s = facade(pkg, sc, kind)
    assert s.n_fields() == 0 and s.linear_init_fields(x, F[:, :K]) == 0 and s.n_fields() == K
    st, S, G, leaf = s.linear_eval_fields_many(y, want_grad=True, want_leaf=True)
    assert st == E.GSL_EDOM and np.array_equal(bits(S), bits(want[:, :K])) and np.array_equal(leaf, leaf_ref)
    # to every other entry the interpolant is field 0's: the bits of a scalar interpolant initialised with column 0
    one = facade(pkg, sc, kind)
    assert one.init(x, np.ascontiguousarray(F[:, 0])) == 0 and one.n_fields() == 1
    st_a, v_a, leaf_a = s.eval_many(y, want_leaf=True)
    st_b, v_b, leaf_b = one.eval_many(y, want_leaf=True)
    assert st_a == st_b == E.GSL_EDOM and np.array_equal(bits(v_a), bits(v_b)) and np.array_equal(bits(v_a), bits(S[:, 0]))
    assert np.array_equal(leaf_a, leaf_b) and np.array_equal(leaf_a, leaf)
    # a plain init answers with K = 1: the linear gradient entry
    st1, S1, G1, leaf1 = one.linear_eval_fields_many(y, want_grad=True, want_leaf=True)
    assert st1 == E.GSL_EDOM and S1.shape == (m, 1) and np.array_equal(bits(S1[:, 0]), bits(S[:, 0])) and np.array_equal(leaf1, leaf)
    assert np.array_equal(bits(G1), bits(G[:, :dim]))
    se, s_e, g_e = s.linear_eval_fields_e(y[0], want_grad=True)
    assert se == 0 and np.array_equal(bits(s_e), bits(S[0])) and np.array_equal(bits(g_e.reshape(-1)), bits(G[0]))
    se, s_e, g_e = s.linear_eval_fields_e(y[1], want_grad=True)
    assert se == E.GSL_EDOM and np.isnan(s_e).all() and np.isnan(g_e).all()
    # resident entry of the facade
    ty = torch.from_numpy(y).cuda()
    tS, tG = torch.empty((m, K), dtype=torch.float64, device="cuda"), torch.empty((m, K * dim), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    assert s.linear_eval_fields_resident(ty.data_ptr(), m, dim, tS.data_ptr(), K, tG.data_ptr(), K * dim) == 0
    assert s.linear_eval_fields_resident(ty.data_ptr(), m, dim, tS.data_ptr(), K - 1) == E.GSL_EINVAL
    assert s.linear_eval_fields_resident(ty.data_ptr(), m, dim, tS.data_ptr(), K, tG.data_ptr(), K * dim - 1) == E.GSL_EINVAL
    torch.cuda.synchronize()
    assert np.array_equal(bits(tS.cpu().numpy()), bits(S)) and np.array_equal(bits(tG.cpu().numpy()), bits(G))
    # checkpoints: one field travels, several are refused and nothing is written
    path, empty = str(tmp_path / "one.bin"), str(tmp_path / "three.bin")
    assert s.fwrite(empty) == E.GSL_EUNSUP and os.path.getsize(empty) == 0
    assert one.fwrite(path) == 0
    back = pkg.Sinterp(kind, dim, len(x), 0)
    assert back.fread(path) == 0 and back.n_fields() == 1
    st2, S2, G2, leaf2 = back.linear_eval_fields_many(y, want_grad=True, want_leaf=True)
    assert st2 == E.GSL_EDOM and np.array_equal(bits(S2), bits(S1)) and np.array_equal(bits(G2), bits(G1)) and np.array_equal(leaf2, leaf)
    # shapes of the many entry
    assert s.linear_eval_fields_many(y, out=(np.empty((m, K + 1)), None))[0] == E.GSL_EBADLEN
    assert s.linear_eval_fields_many(y, want_grad=True, out=(np.empty((m, K)), np.empty((m, K * dim + 1))))[0] == E.GSL_EBADLEN
    # back to one field, then another K
    reseed(pkg, s, kind)
    assert s.init(x, np.ascontiguousarray(F[:, 1])) == 0 and s.n_fields() == 1
    st3, S3, _, _ = s.linear_eval_fields_many(y)
    assert S3.shape == (m, 1) and np.array_equal(bits(S3[:, 0]), bits(want[:, 1])) and s.fwrite(empty) == 0
    reseed(pkg, s, kind)
    assert s.linear_init_fields(x, F[:, :8]) == 0 and s.n_fields() == 8
    st4, S4, _, _ = s.linear_eval_fields_many(y)
    assert np.array_equal(bits(S4), bits(want[:, :8]))
    for h in (s, one, back):
        h.close()


@pytest.mark.parametrize("route", ROUTES)
def test_the_two_bindings_do_not_disturb_each_other(pkg, route):
    sc = scene(pkg, route)
    x, F, m, K = sc["x"], sc["F"], 65, 3
    y = np.ascontiguousarray(sc["y"][:m])
    want = sc["ref"][m][0]
    fresh = sc["keep"].device_alloc(0)                                           # no set_response yet
    assert fresh.set_responses(F[:, :K]) == 0
    assert fresh.eval_many(y)[0] == pkg.capi.GSL_EINVAL                          # the scalar entries still ask for set_response
    S = fresh.eval_fields_many(y)[1]
    assert np.array_equal(bits(S), bits(want[:, :K]))
    assert fresh.set_response(np.ascontiguousarray(F[:, 9])) == 0
    v = fresh.eval_many(y)[1]
    assert np.array_equal(bits(v), bits(want[:, 9]))
    assert np.array_equal(bits(fresh.eval_fields_many(y)[1]), bits(S))           # set_response left the K columns alone
    assert fresh.set_responses(F[:, 20:22]) == 0                                 # ... and set_responses the scalar binding
    assert np.array_equal(bits(fresh.eval_many(y)[1]), bits(v))
    assert np.array_equal(bits(fresh.eval_fields_many(y)[1]), bits(want[:, 20:22]))
    fresh.close()
