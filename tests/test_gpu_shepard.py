"""-m gpu: modified quadratic Shepard interpolation (csrc/hip/shepard.hip) through the raw entries and the facade type
gsl_sinterp_shepard.

Reference: tests/shepard_ref.py (numpy fp64: brute-force neighbour search, np.linalg.qr with the library's rank rule, analytic
gradient), used only after its own two cross-checks passed (lstsq against QR to 1e-11, analytic gradient against Richardson
differences).  Every parity test first asserts on the reference that rho(nc) >= 1e-3 at every node, far from the rank
rule's threshold.  Tolerances: values 1e-10 max|f| (the project's), gradients 1e-10 max|grad s_ref|, fit outputs: radii
1e-13 relative (a square root of a sum of at most three squares, with or without FMA), coefficients 1e-10 max|c|
(Householder QR is backward stable and the scaled matrices have condition <= 200, asserted).  Quadratic data: 1e-12 max|f|
in value and gradient."""
import functools

import numpy as np
import pytest
import torch

import shepard_ref as ref
from gpu_util import Canaried, bits, dev, ptr

pytestmark = pytest.mark.gpu
TOL = 1e-10
SEED = 20261019
M = 2000


def response(x):
    f = np.sin(3.0 * x[:, 0]) * np.cos(2.0 * x[:, 1]) + 0.5 * x[:, 0] ** 2
    if x.shape[1] == 3:
        f = f + np.exp(-x[:, 2]) * x[:, 1]
    return f


def cloud(name):
    rng = np.random.default_rng(SEED + sum(map(ord, name)))
    if name == "random2":
        x = rng.random((400, 2))
    elif name == "random3":
        x = rng.random((600, 3))
    elif name == "clustered":
        x = np.concatenate([0.5 + 0.05 * rng.standard_normal((200, 2)), rng.random((200, 2))])
    elif name == "lattice":
        g = np.arange(20) / 19.0
        x = np.stack(np.meshgrid(g, g, indexing="ij"), axis=2).reshape(-1, 2)
    else:
        raise KeyError(name)
    return np.ascontiguousarray(x), np.ascontiguousarray(rng.random((M, x.shape[1])))


@functools.lru_cache(maxsize=None)
def case(name, nq=0, nw=0):
    """(x, f, y, model, s, g, leaf) of the reference, computed once per session and never modified"""
    x, y = cloud(name)
    f = response(x)
    model = ref.fit(x, f, nq, nw)
    assert not model["coincident"]
    ref.self_check(model, y)
    assert model["rho"].min() >= 1e-3 and model["cond"].max() <= 200.0
    s, g, leaf = ref.evaluate(model, y)
    assert np.isfinite(s).all()                            # the unit box is covered
    for a in (x, f, y, s, g, leaf):
        a.setflags(write=False)
    return x, f, y, model, s, g, leaf


def make(pkg, x, f, nq=0, nw=0):
    n, dim = x.shape
    si = pkg.Sinterp("shepard", dim, n, 0)
    assert si.set_shepard(nq, nw) == 0
    assert si.init(x, f) == 0
    return si


def raw_fit(pkg, x, f, nq, nw, xtda=None):
    """(status, counts, rq, rw, coef) of gsl_sinterp_hip_shepard_fit on a fresh context"""
    n, dim = x.shape
    nc = ref.n_coef(dim)
    ctx = pkg.HipContext.on_torch_stream(0)
    xs = Canaried(np.array(x), ld=xtda or dim)
    d_f = dev(np.array(f))
    rq, rw, coef = Canaried(np.zeros(n)), Canaried(np.zeros(n)), Canaried(np.zeros((n, nc)))
    st, counts = ctx.shepard_fit(xs.ptr, n, dim, xs.ld, ptr(d_f), nq, nw, rq.ptr, rw.ptr, coef.ptr)
    torch.cuda.synchronize()
    assert rq.padding_intact() and rw.padding_intact() and coef.padding_intact() and xs.padding_intact()
    fits = ctx.shepard_fit_count()
    ctx.close()
    return st, counts, rq.get(), rw.get(), coef.get(), fits


CLOUDS = ["random2", "random3", "clustered", "lattice"]


# ---- 1. parity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nq,nw", [(c, 0, 0) for c in CLOUDS] + [("random2", 8, 10), ("random2", 62, 62), ("lattice", 8, 10)])
def test_parity_values_gradients_leaf(pkg, name, nq, nw):
    x, f, y, model, s_ref, g_ref, leaf_ref = case(name, nq, nw)
    si = make(pkg, x, f, nq, nw)
    st, s, leaf = si.eval_many(y, want_leaf=True)
    st2, s2, g = si.eval_grad_many(y)
    ds, dg = np.abs(s - s_ref).max() / np.abs(f).max(), np.abs(g - g_ref).max() / np.abs(g_ref).max()
    print(f"{name} nq={nq} nw={nw}: value defect {ds:.3g}, gradient defect {dg:.3g}, leaf {leaf.min()}..{leaf.max()}")
    assert st == 0 and st2 == 0
    assert ds <= TOL and dg <= TOL
    assert (leaf == leaf_ref).all()
    assert (bits(s) == bits(s2)).all()                     # the value bits do not depend on the gradient output
    stt = si.shepard_stats()
    assert stt[:3] == (0, 0, 0) and stt[3] == pytest.approx(model["rw"].max(), rel=1e-13)


@pytest.mark.parametrize("name,nq,nw", [("random2", 13, 19), ("random3", 17, 32), ("clustered", 13, 19), ("lattice", 13, 19),
                                        ("random2", 8, 10), ("random2", 62, 62)])
def test_raw_fit_against_the_reference(pkg, name, nq, nw):
    x, f, y, model, *_ = case(name, 0 if (nq, nw) in ((13, 19), (17, 32)) else nq, 0 if (nq, nw) in ((13, 19), (17, 32)) else nw)
    st, counts, rq, rw, coef, fits = raw_fit(pkg, x, f, nq, nw, xtda=x.shape[1] + 2)
    drq, drw = np.abs(rq / model["rq"] - 1.0).max(), np.abs(rw / model["rw"] - 1.0).max()
    dc = np.abs(coef - model["coef"]).max() / np.abs(model["coef"]).max()
    print(f"{name} nq={nq} nw={nw}: Rq {drq:.3g}, Rw {drw:.3g}, coefficients {dc:.3g}")
    assert st == 0 and counts == (0, 0, 0) and fits == 1
    assert drq <= 1e-13 and drw <= 1e-13 and dc <= TOL


# ---- 2. properties -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["random2", "random3"])
def test_quadratics_are_reproduced(pkg, name):
    x, y = cloud(name)
    dim = x.shape[1]
    lin, sq = np.arange(1.0, dim + 1.0), np.arange(2.0, dim + 2.0)
    quad = lambda p: 1.0 + p @ lin + (p * p) @ sq + p[:, 0] * p[:, 1] - 0.5 * p[:, -1] * p[:, 0]
    f = quad(x)
    want_g = lin + 2.0 * y * sq
    want_g[:, 0] += y[:, 1] - 0.5 * y[:, -1]
    want_g[:, 1] += y[:, 0]
    want_g[:, -1] -= 0.5 * y[:, 0]
    si = make(pkg, x, f)
    st, s, g = si.eval_grad_many(y)
    ds, dg = np.abs(s - quad(y)).max() / np.abs(f).max(), np.abs(g - want_g).max() / np.abs(f).max()
    print(f"{name}: quadratic value defect {ds:.3g}, gradient defect {dg:.3g}")
    assert st == 0 and ds <= 1e-12 and dg <= 1e-12


@pytest.mark.parametrize("name", ["random2", "random3", "lattice"])
def test_sites_are_reproduced_bit_for_bit(pkg, name):
    x, f, *_ = case(name)
    si = make(pkg, x, f)
    st, s, leaf = si.eval_many(x, want_leaf=True)
    st2, s2, g = si.eval_grad_many(x)
    st3, nodal, iters, resid = si.get_gradients()
    assert st == 0 and st2 == 0 and st3 == 0 and iters == 0 and resid == 0.0
    assert (bits(s) == bits(f)).all() and (bits(s2) == bits(f)).all() and (leaf == 1).all()
    assert nodal.shape == x.shape and (bits(g) == bits(nodal)).all()
    st4, v = si.eval_e(x[7])
    assert st4 == 0 and bits(np.array([v]))[0] == bits(f[7:8])[0]


@pytest.mark.parametrize("name", ["random2", "random3"])
def test_gradient_is_the_derivative_of_the_values(pkg, name):
    """central differences of the library's own values, step h, against its gradient.  The reference shows the defect
    D_ref of the same differences at the same step; the library's values are within tau = 1e-10 max|f| of the reference's
    (the parity bound) and its gradients within 1e-10 max|grad|, so the library's defect is at most
    D_ref + tau / h + 1e-10 max|grad|."""
    x, f, y, model, s_ref, g_ref, _ = case(name)
    dim, h = x.shape[1], 1e-4
    yy = np.ascontiguousarray(y[:300])
    si = make(pkg, x, f)
    g = si.eval_grad_many(yy)[2]
    worst_lib = worst_ref = 0.0
    for a in range(dim):
        e = np.zeros(dim)
        e[a] = h
        cd = (si.eval_many(yy + e)[1] - si.eval_many(yy - e)[1]) / (2.0 * h)
        cd_ref = (ref.evaluate(model, yy + e)[0] - ref.evaluate(model, yy - e)[0]) / (2.0 * h)
        worst_lib = max(worst_lib, np.abs(cd - g[:, a]).max())
        worst_ref = max(worst_ref, np.abs(cd_ref - g_ref[:300, a]).max())
    bound = worst_ref + TOL * np.abs(f).max() / h + TOL * np.abs(g_ref).max()
    print(f"{name}: central-difference defect {worst_lib:.3g} (reference {worst_ref:.3g}, bound {bound:.3g})")
    assert worst_lib <= bound


# ---- 3. edges ----------------------------------------------------------------------------------------------------------
def test_uncovered_and_nan_targets(pkg):
    x, f, y, model, s_ref, *_ = case("random2")
    si = make(pkg, x, f)
    yy = np.array(y[:50])
    yy[3] = [7.0, -3.0]
    yy[17] = [1.0 + 2.0 * model["rw"].max(), 0.5]
    with pkg.capi.ErrorCalls() as calls:
        st, s, leaf = si.eval_many(yy, want_leaf=True)
        st2, s2, g = si.eval_grad_many(yy)
        st3, v = si.eval_e(yy[3])
    assert st == st2 == st3 == pkg.GSL_EDOM and [c[1] for c in calls] == [pkg.GSL_EDOM] * 2     # eval_e: by status only
    out = np.zeros(50, dtype=bool)
    out[[3, 17]] = True
    assert np.isnan(s[out]).all() and np.isnan(g[out]).all() and (leaf[out] == -1).all() and np.isnan(v)
    assert np.abs(s[~out] - s_ref[:50][~out]).max() <= TOL * np.abs(f).max() and np.isfinite(g[~out]).all() and (leaf[~out] > 0).all()
    # a NaN coordinate: NaN and no error
    yy = np.array(y[:50])
    yy[5, 1] = np.nan
    with pkg.capi.ErrorCalls() as calls:
        st, s, leaf = si.eval_many(yy, want_leaf=True)
        st2, s2, g = si.eval_grad_many(yy)
    assert st == 0 and st2 == 0 and calls == []
    assert np.isnan(s[5]) and np.isnan(g[5]).all() and leaf[5] == -1 and np.isfinite(np.delete(s, 5)).all()
    # eval_grid reports uncovered nodes the mesh types' way
    with pkg.capi.ErrorCalls() as calls:
        st, grid = si.eval_grid([0.0, 0.0], [4.0, 4.0], 4, 4)
    assert st == pkg.GSL_EDOM and np.isnan(grid[3, 3]) and np.isfinite(grid[0, 0])


def test_target_at_1e_200_from_a_site(pkg):
    x, f, *_ = case("random2")
    x = np.array(x)
    x[11] = [0.0, 0.0]                                     # where 1e-200 is representable next to the site
    f = response(x)
    si = make(pkg, x, f)
    yy = np.array([[1e-200, 0.0], [0.0, -1e-200], [1e-200, 1e-200]])
    st, s, leaf = si.eval_many(yy, want_leaf=True)
    st2, s2, g = si.eval_grad_many(yy)
    nodal = si.get_gradients()[1]
    assert st == 0 and st2 == 0 and (bits(s) == bits(f[11])).all() and (bits(s2) == bits(f[11])).all()
    assert (bits(g) == bits(np.tile(nodal[11], (3, 1)))).all() and (leaf >= 1).all()


def test_coincident_sites_fail_init(pkg):
    x, f, y, *_ = case("random2")
    x = np.array(x)
    x[200] = x[31]
    si = pkg.Sinterp("shepard", 2, 400, 0)
    with pkg.capi.ErrorCalls() as calls:
        assert si.init(x, f) == pkg.GSL_EDOM
        assert si.eval_many(y[:4])[0] == pkg.GSL_EINVAL   # stays uninitialised
    assert [c[1] for c in calls] == [pkg.GSL_EDOM, pkg.GSL_EINVAL]
    st, counts, *_ = raw_fit(pkg, x, f, 13, 19)
    assert st == pkg.GSL_EDOM and counts[2] == 2


def test_collinear_cloud_takes_the_constant_fallback(pkg):
    n = 60
    t = np.sort(np.random.default_rng(SEED + 5).random(n))
    x = np.ascontiguousarray(np.stack([t, t], axis=1))     # the diagonal: both linear columns are the same
    f = np.sin(4.0 * t)
    si = make(pkg, x, f)
    st, n_lin, n_const, rw_max = si.shepard_stats()
    assert st == 0 and (n_lin, n_const) == (0, n) and rw_max > 0.0
    mid = np.ascontiguousarray(0.5 * (x[1:] + x[:-1]))
    st, s, g = si.eval_grad_many(mid)
    assert st == 0 and np.isfinite(s).all() and np.isfinite(g).all()
    assert s.min() >= f.min() - 1e-12 and s.max() <= f.max() + 1e-12      # constant nodal functions: a convex combination of the data
    assert (bits(si.eval_many(x)[1]) == bits(f)).all()
    assert (si.get_gradients()[1] == 0.0).all()


def test_planar_cloud_in_3d_takes_fallbacks(pkg):
    n = 300
    p = np.random.default_rng(SEED + 6).random((n, 2))
    x = np.ascontiguousarray(np.stack([p[:, 0], p[:, 1], 0.25 + 0.5 * p[:, 0]], axis=1))     # a tilted plane
    f = response(x)
    si = make(pkg, x, f)
    st, n_lin, n_const, _ = si.shepard_stats()
    assert st == 0 and n_lin + n_const == n               # no neighbourhood has rank 9
    yy = np.ascontiguousarray(x[:100] + 1e-3)
    st, s, g = si.eval_grad_many(yy)
    assert st == 0 and np.isfinite(s).all() and np.isfinite(g).all()
    assert (bits(si.eval_many(x)[1]) == bits(f)).all()


# ---- 4. bits -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["random2", "random3"])
def test_same_bits_alone_in_a_batch_and_past_the_cell_order_threshold(pkg, name):
    x, f, y, *_ = case(name)
    dim = x.shape[1]
    big = np.ascontiguousarray(np.random.default_rng(SEED + 7).random((5000, dim)))
    big[1234] = y[0]
    si = make(pkg, x, f)
    one_s, one_g = si.eval_grad_many(np.ascontiguousarray(y[:1]))[1:]
    h_s, h_g = si.eval_grad_many(np.ascontiguousarray(y[:100]))[1:]
    b_s, b_g = si.eval_grad_many(big)[1:]
    assert bits(one_s)[0] == bits(h_s)[0] == bits(b_s)[1234] and (bits(one_g[0]) == bits(h_g[0])).all() and (bits(one_g[0]) == bits(b_g[1234])).all()
    assert (bits(si.eval_many(big)[1]) == bits(b_s)).all()                  # with and without the gradient, cell-ordered batch
    assert (bits(si.eval_many(np.ascontiguousarray(big[:100]))[1]) == bits(b_s[:100])).all()
    assert (bits(si.eval_grad_many(big)[1]) == bits(b_s)).all()             # run to run
    # one pack for all of it
    assert si.shepard_counters() == (1, 1)


def test_two_fits_give_identical_coefficients(pkg):
    x, f, *_ = case("random3")
    a = raw_fit(pkg, x, f, 17, 32)
    b = raw_fit(pkg, x, f, 17, 32)
    assert a[0] == 0 and b[0] == 0
    for u, v in zip(a[2:5], b[2:5]):
        assert (bits(u) == bits(v)).all()


@pytest.mark.parametrize("name", ["random2", "random3"])
def test_checkpoint_round_trip(pkg, name, tmp_path):
    x, f, y, *_ = case(name)
    n, dim = x.shape
    si = make(pkg, x, f, 0 if dim == 2 else 12, 0)
    path = str(tmp_path / "shepard.bin")
    assert si.fwrite(path) == 0
    back = pkg.Sinterp("shepard", dim, n, 0)
    assert back.fread(path) == 0
    assert back.shepard_counters() == (0, 0)               # nothing was searched or fitted
    assert back.shepard_stats() == si.shepard_stats()
    st, s, g = back.eval_grad_many(y)
    st0, s0, g0 = si.eval_grad_many(y)
    assert st == 0 and (bits(s) == bits(s0)).all() and (bits(g) == bits(g0)).all()
    assert (bits(back.get_gradients()[1]) == bits(si.get_gradients()[1])).all()
    assert back.shepard_counters() == (0, 1)
    path2 = str(tmp_path / "again.bin")
    assert back.fwrite(path2) == 0 and open(path, "rb").read() == open(path2, "rb").read()
    with pkg.capi.ErrorCalls():
        assert pkg.Sinterp("shepard", dim, n + 1, 0).fread(path) == pkg.capi.GSL_EBADLEN
        assert pkg.Sinterp("gaussian", dim, n, 0).fread(path) == pkg.capi.GSL_EBADLEN


# ---- 5. size -----------------------------------------------------------------------------------------------------------
def test_twenty_thousand_sites_in_3d(pkg):
    n = m = 20000
    rng = np.random.default_rng(SEED + 8)
    x, y = np.ascontiguousarray(rng.random((n, 3))), np.ascontiguousarray(rng.random((m, 3)))
    f = response(x)
    si = make(pkg, x, f)
    st, s, g = si.eval_grad_many(y)
    st2, s2, leaf = si.eval_many(y, want_leaf=True)
    assert st == 0 and st2 == 0 and (bits(s) == bits(s2)).all() and (leaf > 0).all()
    spot = rng.choice(m, 500, replace=False)
    model = ref.fit(x, f)                                   # candidate neighbours from the kd-tree ...
    some = rng.choice(n, 1000, replace=False)
    brute = ref.fit(x, f, rows=some, kdtree=False)          # ... which the brute-force pass confirms on 1000 rows
    assert all((bits(brute[k][some]) == bits(model[k][some])).all() for k in ("rq", "rw", "coef"))
    assert model["rho"].min() >= 1e-3
    s_ref, g_ref, leaf_ref = ref.evaluate(model, y[spot])
    ds, dg = np.abs(s[spot] - s_ref).max() / np.abs(f).max(), np.abs(g[spot] - g_ref).max() / np.abs(g_ref).max()
    print(f"N = 20000: value defect {ds:.3g}, gradient defect {dg:.3g}, leaf up to {leaf.max()}")
    assert ds <= TOL and dg <= TOL and (leaf[spot] == leaf_ref).all()
    assert si.shepard_stats()[3] == pytest.approx(model["rw"].max(), rel=1e-13)


# ---- 6. canaries, strides, the resident entries --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["random2", "random3"])
def test_raw_eval_strides_and_canaries(pkg, name):
    x, f, y, model, s_ref, g_ref, leaf_ref = case(name)
    n, dim = x.shape
    nq, nw = ref.DEFAULTS[dim]
    ctx = pkg.HipContext.on_torch_stream(0)
    xs, ys = Canaried(np.array(x), ld=dim + 1, off=1), Canaried(np.array(y), ld=dim + 3)
    d_f = dev(np.array(f))
    rq, rw, coef = Canaried(np.zeros(n)), Canaried(np.zeros(n)), Canaried(np.zeros((n, ref.n_coef(dim))))
    st, counts = ctx.shepard_fit(xs.ptr, n, dim, xs.ld, ptr(d_f), nq, nw, rq.ptr, rw.ptr, coef.ptr)
    assert st == 0 and counts == (0, 0, 0)
    s, g = Canaried(np.zeros(M)), Canaried(np.zeros((M, dim)), ld=dim + 2, off=1)
    leaf = torch.full((M + 64,), -7, dtype=torch.int32, device="cuda")
    for rep in range(2):
        st, outside = ctx.shepard_eval(xs.ptr, n, dim, xs.ld, ptr(d_f), rq.ptr, rw.ptr, coef.ptr, ys.ptr, M, ys.ld, s.ptr, g.ptr, g.ld, ptr(leaf), 77)
        assert st == 0 and outside == 0 and ctx.shepard_pack_count() == 1
    torch.cuda.synchronize()
    for c in (xs, ys, rq, rw, coef, s, g):
        assert c.padding_intact()
    hl = leaf.cpu().numpy()
    assert (hl[M:] == -7).all() and (hl[:M] == leaf_ref).all()
    assert np.abs(s.get() - s_ref).max() <= TOL * np.abs(f).max() and np.abs(g.get() - g_ref).max() <= TOL * np.abs(g_ref).max()
    # values only, gradient only, leaf only: the same bits; model_id 0 packs again
    s2 = Canaried(np.zeros(M))
    st, _ = ctx.shepard_eval(xs.ptr, n, dim, xs.ld, ptr(d_f), rq.ptr, rw.ptr, coef.ptr, ys.ptr, M, ys.ld, s2.ptr, None, 0, None, 0)
    g2 = Canaried(np.zeros((M, dim)))
    st2, _ = ctx.shepard_eval(xs.ptr, n, dim, xs.ld, ptr(d_f), rq.ptr, rw.ptr, coef.ptr, ys.ptr, M, ys.ld, None, g2.ptr, dim, None, 77)
    assert st == 0 and st2 == 0 and ctx.shepard_pack_count() == 3
    assert (bits(s2.get()) == bits(s.get())).all() and (bits(g2.get()) == bits(g.get())).all() and s2.padding_intact() and g2.padding_intact()
    # the facade computes the same bits from the same data
    si = make(pkg, x, f)
    assert (bits(si.eval_many(y)[1]) == bits(s.get())).all()
    ctx.close()


def test_facade_resident_grid_and_single_target_entries(pkg):
    x, f, y, model, s_ref, g_ref, leaf_ref = case("random2")
    si = make(pkg, x, f)
    st, s, leaf = si.eval_many(y, want_leaf=True)
    g = si.eval_grad_many(y)[2]
    ys = Canaried(np.array(y), ld=4)
    d_s, d_g = Canaried(np.zeros(M)), Canaried(np.zeros((M, 2)), ld=3)
    d_leaf = torch.full((M + 16,), -7, dtype=torch.int32, device="cuda")
    assert si.eval_resident(ys.ptr, M, 4, d_s.ptr, ptr(d_leaf)) == 0
    assert (bits(d_s.get()) == bits(s)).all() and (d_leaf.cpu().numpy()[:M] == leaf).all() and (d_leaf.cpu().numpy()[M:] == -7).all()
    d_s.set(np.zeros(M))
    assert si.eval_grad_resident(ys.ptr, M, 4, d_s.ptr, d_g.ptr, 3) == 0
    assert (bits(d_s.get()) == bits(s)).all() and (bits(d_g.get()) == bits(g)).all() and d_s.padding_intact() and d_g.padding_intact()
    assert si.eval_grad_resident(ys.ptr, M, 4, None, d_g.ptr, 3) == 0 and (bits(d_g.get()) == bits(g)).all()
    st, v, gv = si.eval_grad_e(y[9])
    assert st == 0 and bits(np.array([v]))[0] == bits(s)[9] and (bits(gv) == bits(g[9])).all()
    st, grid = si.eval_grid([0.0, 0.0], [1.0, 1.0], 6, 5)
    gy = np.ascontiguousarray(np.stack(np.meshgrid((1.0 / 6) * np.arange(6), (1.0 / 5) * np.arange(5), indexing="ij"), axis=2).reshape(-1, 2))
    assert st == 0 and (bits(grid.ravel()) == bits(si.eval_many(gy)[1])).all()
    # a strided host batch and a strided gradient matrix
    wide = np.full((M, 5), np.nan)
    wide[:, :2] = y
    gw = np.full((M, 4), 7.0)
    st, s3, g3 = si.eval_grad_many(wide[:, :2], out=(np.zeros(M), gw[:, :2]))
    assert st == 0 and (bits(s3) == bits(s)).all() and (bits(gw[:, :2]) == bits(g)).all() and (gw[:, 2:] == 7.0).all()
    # re-initialised with other data: a new model, a new pack
    assert si.init(x, 2.0 * f) == 0 and si.shepard_counters()[0] == 2
    assert np.abs(si.eval_many(y)[1] - 2.0 * s_ref).max() <= 2.0 * TOL * np.abs(f).max()
