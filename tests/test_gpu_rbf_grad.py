"""-m gpu: value + gradient of the RBF-family interpolants from the fused sweeps (csrc/hip/rbf.hip: rbf_grad_kernel and
rbf_grad_cull_kernel, the GRAD instances of the bodies rbf_sweep / rbf_sweep_cull that rbf_eval_kernel and
rbf_eval_gauss_cull_kernel share).

The oracle has no gradient.  The reference is the formula in numpy fp64,
    grad s(y) = sum_j w_j psi(r_j^2) (y - x_j) [+ c_1 .. c_dim],   psi = phi'(r) / r
    Gaussian -2 eps^2 exp(-eps^2 r^2);  Wendland -20 eps^2 (1 - eps r)_+^3;  thin-plate ln r^2 + 1,
summed with the LIBRARY's weights (Sinterp.weights(), poly() for the affine type), so the sweep is tested and not the
conditioning of the solve.  That reference is within 1e-14 relative of its 80-bit evaluation on these shapes, so the
bound is the project's TOL = 1e-10 on relerr = max|got - want| / max|want| over the whole m x dim array.  The reference
takes every term; the sweeps drop Gaussian terms below 2^-72 of the kernel maximum (< N max|w| eps 3e-21 in all).

Targets are synth_targets(0, m, dim) followed by the first 20 centres, so r = 0 terms occur.  Values are compared
BITWISE with eval_many's.

Non-finite targets: "an infinite coordinate takes no term" is a statement about the kinds that have a take-criterion
(Gaussian, Wendland); a thin-plate term at infinite distance is not finite and nothing is asserted about it."""
import numpy as np
import pytest
import torch

from gpu_util import Canaried, bits, dev, ptr

pytestmark = pytest.mark.gpu
TOL = 1e-10
GAUSSIAN, TPS, WENDLAND = 0, 1, 2
KIND = {"gaussian": GAUSSIAN, "kriging": GAUSSIAN, "tps": TPS, "tps_affine": TPS, "wendland": WENDLAND}
N_SITES = 20


def relerr(got, want):
    return np.abs(got - want).max() / np.abs(want).max()


def reference_gradient(kind, eps, x, w, y, tail=None):
    """the formula in fp64, every term"""
    out = np.empty((len(y), x.shape[1]))
    block = max(1, 2_000_000 // len(x))                              # rows per pass: bounded temporaries at large n
    for k0 in range(0, len(y), block):
        d = y[k0:k0 + block, None, :] - x[None, :, :]
        r2 = (d * d).sum(axis=2)
        if kind == GAUSSIAN:
            psi = -2.0 * eps * eps * np.exp(-(eps * eps) * r2)
        elif kind == WENDLAND:
            t = eps * np.sqrt(r2)
            psi = -20.0 * eps * eps * np.where(t < 1.0, (1.0 - t) ** 3, 0.0)
        else:
            psi = np.log(np.where(r2 > 0.0, r2, 1.0)) + 1.0          # r = 0: finite times (y - x) = 0
        out[k0:k0 + block] = np.einsum("kj,kjc->kc", psi * w[None, :], d)
    if tail is not None:
        out += np.asarray(tail)[1:1 + x.shape[1]][None, :]
    return out


_models = {}


def model(pkg, orc, typ, dim, n, response=None):
    """an initialised interpolant of one shape with its centres, weights, eps and tail: built once, shared, left unchanged"""
    key = (typ, dim, n, response)
    if key not in _models:
        x = orc.synth_centres(n, dim)
        f = orc.synth_response(x) if response is None else 3.0 + 2.0 * x[:, 0] - 5.0 * x[:, 1]
        s = pkg.Sinterp(typ, dim, n, 0)
        if typ == "wendland":
            eps = 0.125 * n ** (1.0 / dim)                           # the facade default
        else:
            eps = orc.gaussian_eps(n, dim)
            assert s.set_shape(eps) == 0
        if typ == "kriging":
            assert s.set_nugget(1e-3) == 0
        assert s.init(x, f) == 0
        st, w = s.weights()
        assert st == 0
        tail = None
        if typ == "tps_affine":
            st, tail = s.poly()
            assert st == 0
        for a in (x, f, w):
            a.setflags(write=False)
        _models[key] = (s, x, w, eps, tail)
    return _models[key]


def targets(orc, x, m):
    """m rows in all: synthetic targets followed by the first 20 centres"""
    y = np.ascontiguousarray(np.vstack([orc.synth_targets(0, m - N_SITES, x.shape[1]), x[:N_SITES]]))
    y.setflags(write=False)
    return y


PLAIN = [("gaussian", 2, 513), ("gaussian", 1, 130), ("gaussian", 3, 700), ("tps", 2, 513), ("tps", 3, 333), ("tps", 1, 130),
         ("tps_affine", 2, 600), ("wendland", 2, 513), ("kriging", 2, 513)]
CULLED = [("gaussian", 2, 1100), ("gaussian", 3, 1200), ("wendland", 2, 1100), ("wendland", 3, 1200), ("kriging", 2, 1100),
          ("gaussian", 1, 1100), ("wendland", 1, 1100)]        # the 1-D culled kernel (DIM = 1, tiles of 32)


@pytest.mark.parametrize("typ,dim,n", PLAIN + CULLED)
def test_facade_matches_the_formula(pkg, orc, typ, dim, n):
    s, x, w, eps, tail = model(pkg, orc, typ, dim, n)
    y = targets(orc, x, 300 + N_SITES)
    st, val, g = s.eval_grad_many(y)
    assert st == 0
    want = reference_gradient(KIND[typ], eps, x, w, y, tail)
    err = relerr(g, want)
    print(f"{typ} dim {dim} n {n}: gradient relerr {err:.3e}, max|want| {np.abs(want).max():.3e}")
    assert err < TOL
    st, plain, _ = s.eval_many(y)
    assert st == 0 and np.array_equal(bits(val), bits(plain))
    st, v0, g0 = s.eval_grad_e(y[0])
    assert st == 0 and np.array_equal(bits(np.array([v0])), bits(val[:1])) and np.array_equal(bits(g0), bits(g[0]))
    st, none, g_only = s.eval_grad_many(y, want_value=False)
    assert st == 0 and none is None and np.array_equal(bits(g_only), bits(g))


def test_affine_exactness(pkg, orc):
    s, x, w, eps, tail = model(pkg, orc, "tps_affine", 2, 600, response="linear")
    y = targets(orc, x, 300 + N_SITES)
    st, val, g = s.eval_grad_many(y)
    assert st == 0
    err = np.abs(g - np.array([2.0, -5.0])[None, :]).max()
    print(f"affine exactness: max |g - (2, -5)| = {err:.3e}")
    assert err < 1e-9


@pytest.mark.parametrize("typ,n,m", [("gaussian", 1100, 5000), ("gaussian", 1100, 131077), ("gaussian", 1100, 262147),
                                     ("tps", 100, 262147), ("wendland", 1100, 131077)])
def test_sorted_route_and_two_targets_per_lane(pkg, orc, typ, n, m):
    dim = 2
    s, x, w, eps, tail = model(pkg, orc, typ, dim, n)
    y = targets(orc, x, m)
    st, val, g = s.eval_grad_many(y)
    assert st == 0
    rows = np.unique(np.concatenate([np.arange(0, m, 131), np.arange(m - 25, m)]))
    err = relerr(g[rows], reference_gradient(KIND[typ], eps, x, w, y[rows], tail))
    print(f"{typ} n {n} m {m}: gradient relerr on {len(rows)} rows {err:.3e}")
    assert err < TOL
    st, plain, _ = s.eval_many(y)
    assert st == 0 and np.array_equal(bits(val), bits(plain))
    # a target's bits do not depend on where it sits in the batch
    order = np.random.default_rng(m).permutation(m)
    st, val2, g2 = s.eval_grad_many(np.ascontiguousarray(y[order]))
    assert st == 0 and np.array_equal(bits(val2), bits(val[order])) and np.array_equal(bits(g2), bits(g[order]))


@pytest.mark.parametrize("kind,n,tail,want_value", [
    (GAUSSIAN, 65600, None, True),             # tile size 16
    (GAUSSIAN, 131080, None, True),            # tile size 32
    (GAUSSIAN, 262150, None, True),            # beyond CULL_MAX_TILES: the plain sweep
    (WENDLAND, 1100, (0.5, 1.0, -2.0), True),
    (GAUSSIAN, 1100, None, False),             # d_s = NULL
])
def test_raw_entry_layouts_and_tile_sizes(pkg, orc, kind, n, tail, want_value):
    dim, xtda, ytda, gtda, m = 2, 3, 4, 5, 64 + 1
    x = orc.synth_centres(n, dim)
    w = np.random.default_rng(n).standard_normal(n)
    eps = orc.gaussian_eps(n, dim) if kind == GAUSSIAN else 0.125 * n ** (1.0 / dim)
    y = targets(orc, x, m)
    want = reference_gradient(kind, eps, x, w, y, tail)
    ctx = pkg.HipContext.on_torch_stream(0)
    d_x, d_y, d_w = Canaried(x, ld=xtda), Canaried(y, ld=ytda), Canaried(w)

    def call(model_id, value_first=False):
        d_s, d_g = Canaried(np.zeros(m)), Canaried(np.zeros((m, dim)), ld=gtda)
        if value_first:                                              # into a buffer of its own: d_s stays the gradient call's
            ctx.rbf_eval(kind, eps, d_x.ptr, n, dim, xtda, d_w.ptr, d_y.ptr, m, ytda, Canaried(np.zeros(m)).ptr, model_id=model_id)
        st = ctx.rbf_eval_grad(kind, eps, d_x.ptr, n, dim, xtda, d_w.ptr, d_y.ptr, m, ytda, d_s.ptr if want_value else None, d_g.ptr, gtda,
                               tail=tail, model_id=model_id)
        ctx.sync()
        assert st == 0
        assert d_s.padding_intact() and d_g.padding_intact()
        return d_s.get(), d_g.get()

    val, g = call(0)
    err = relerr(g, want)
    print(f"raw kind {kind} n {n}: gradient relerr {err:.3e}")
    assert err < TOL
    if want_value:
        d_v = Canaried(np.zeros(m))
        if tail is None:
            ctx.rbf_eval(kind, eps, d_x.ptr, n, dim, xtda, d_w.ptr, d_y.ptr, m, ytda, d_v.ptr)
        else:
            ctx.rbf_eval_affine(kind, eps, tail, d_x.ptr, n, dim, xtda, d_w.ptr, d_y.ptr, m, ytda, d_v.ptr)
        ctx.sync()
        assert np.array_equal(bits(val), bits(d_v.get()))
    else:
        assert (val == 0.0).all()                                    # the value buffer was not given: nothing wrote one
    # the packed-centre cache: filled by a gradient call, reused by the next; filled by a VALUE call, reused by a gradient call
    v1, g1 = call(7)
    v2, g2 = call(7)
    v3, g3 = call(9, value_first=True)
    for vv, gg in ((v1, g1), (v2, g2), (v3, g3)):
        assert np.array_equal(bits(gg), bits(g)) and np.array_equal(bits(vv), bits(val))
    assert d_x.padding_intact() and d_y.padding_intact() and d_w.padding_intact()
    # m = 0 succeeds and touches nothing; a row pitch below dim is refused
    p = d_y.ptr
    assert ctx.rbf_eval_grad(kind, eps, d_x.ptr, n, dim, xtda, d_w.ptr, None, 0, ytda, None, None, gtda) == 0
    assert ctx.rbf_eval_grad(kind, eps, d_x.ptr, n, dim, xtda, d_w.ptr, p, m, ytda, None, p, 1) == pkg.GSL_EINVAL
    assert ctx.rbf_eval_grad(kind, eps, d_x.ptr, n, 4, xtda, d_w.ptr, p, m, ytda, None, p, gtda) == pkg.GSL_EINVAL
    assert ctx.rbf_eval_grad(7, eps, d_x.ptr, n, dim, xtda, d_w.ptr, p, m, ytda, None, p, gtda) == pkg.GSL_EINVAL
    assert ctx.rbf_eval_grad(kind, eps, d_x.ptr, n, dim, xtda, d_w.ptr, p, m, ytda, None, None, gtda) == pkg.capi.GSL_EFAULT
    ctx.close()


@pytest.mark.parametrize("typ", ["gaussian", "tps", "wendland"])
def test_nan_inf_and_far_targets(pkg, orc, typ):
    dim, n = 2, 513
    s, x, w, eps, tail = model(pkg, orc, typ, dim, n)
    y = np.array(targets(orc, x, 64 + N_SITES))
    y[3, 0] = np.nan
    y[70, 1] = np.nan
    local = typ != "tps"
    if local:
        y[5] = 50.0
        y[9, 1] = np.inf
        y[11, 0] = -np.inf
    st, val, g = s.eval_grad_many(y)
    assert st == 0
    for k in (3, 70):
        assert np.isnan(val[k]) and np.isnan(g[k]).all()
    if local:
        for k in (5, 9, 11):
            assert (g[k] == 0.0).all() and val[k] == 0.0
    ok = np.isfinite(y).all(axis=1)
    assert relerr(g[ok], reference_gradient(KIND[typ], eps, x, w, y[ok], tail)) < TOL
    st, plain, _ = s.eval_many(y)
    assert st == 0 and np.array_equal(np.isnan(plain), np.isnan(val)) and np.array_equal(bits(plain[ok]), bits(val[ok]))


def test_checkpoint(pkg, orc, tmp_path):
    dim, n = 2, 513
    s, x, w, eps, tail = model(pkg, orc, "kriging", dim, n)
    y = targets(orc, x, 300 + N_SITES)
    st, val, g = s.eval_grad_many(y)
    assert st == 0
    path = tmp_path / "krige_grad.bin"
    assert s.fwrite(str(path)) == 0
    r = pkg.Sinterp("kriging", dim, n, 0)
    assert r.fread(str(path)) == 0
    st, val2, g2 = r.eval_grad_many(y)
    assert st == 0 and np.array_equal(bits(val2), bits(val)) and np.array_equal(bits(g2), bits(g))


def test_device_list(pkg, orc):
    dim, n = 2, 1100
    s, x, w, eps, tail = model(pkg, orc, "gaussian", dim, n)
    y = targets(orc, x, 300 + N_SITES)
    st, val, g = s.eval_grad_many(y)
    assert st == 0
    grp = pkg.Sinterp("gaussian", dim, n, 0)
    assert grp.set_device_list([0, 0]) == 0 and grp.set_shape(eps) == 0
    assert grp.init(x, orc.synth_response(x)) == 0
    st, val2, g2 = grp.eval_grad_many(y)
    assert st == 0 and np.array_equal(bits(val2), bits(val)) and np.array_equal(bits(g2), bits(g))
    d_y, d_s, d_g = dev(y), dev(np.zeros(len(y))), dev(np.zeros((len(y), dim)))
    assert grp.eval_grad_resident(ptr(d_y), len(y), dim, ptr(d_s), ptr(d_g), dim) == 0
    torch.cuda.synchronize()                                         # the group's members run on streams of their own
    assert np.array_equal(bits(d_g.cpu().numpy()), bits(g)) and np.array_equal(bits(d_s.cpu().numpy()), bits(val))
