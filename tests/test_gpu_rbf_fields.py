"""-m gpu: several fields on one set of centres (csrc/hip/rbf.hip: rbf_fields_kernel and rbf_fields_cull_kernel, the fields
instances of the bodies rbf_sweep / rbf_sweep_cull; solve.hip: rbf_solve_fields / krige_solve_fields; the facade's
init_fields / eval_fields entries).

The central contract is bitwise: field q of a fields sweep has the bits of gsl_sinterp_hip_rbf_eval_model called with
d_w = column q.  The solves are compared with the oracle per column at the project's TOL = 1e-10 on
relerr = max|got - want| / max|want| (tests/test_gpu_rbf.py): columns solved in different groups of right-hand sides agree
to rounding only, so nothing bitwise is asserted across columns there.

Targets are synth_targets followed by the first 20 centres, so r = 0 terms occur."""
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


def shape_eps(orc, kind, n, dim):
    return orc.gaussian_eps(n, dim) if kind == GAUSSIAN else 0.125 * n ** (1.0 / dim)


def targets(orc, x, m):
    """m rows in all: synthetic targets followed by the first 20 centres"""
    return np.ascontiguousarray(np.vstack([orc.synth_targets(0, m - N_SITES, x.shape[1]), x[:N_SITES]]))


def field_counts(pkg):
    nf, small = pkg.HipContext.rbf_fields_block(), pkg.HipContext.rbf_fields_block_small()
    # a full block, a ragged block, several passes; and the same for the small instance that takes the last <= small fields
    return sorted({1, 2, 3, nf, nf + 1, 2 * nf + 3, small, small + 1, nf + small})


def responses(orc, x, k):
    """k smooth, different responses on the centres: synth_response composed with a map per field"""
    f = orc.synth_response(x)
    maps = [lambda v: v, np.sin, lambda v: v * v + 0.5 * v, np.cos, lambda v: np.exp(0.3 * v), lambda v: 1.0 / (2.0 + v * v)]
    return np.ascontiguousarray(np.stack([maps[q % len(maps)]((1.0 + q // len(maps)) * f) for q in range(k)], axis=1))


def scalar_columns(ctx, kind, eps, d_x, n, dim, xtda, W, d_y, m, ytda, model_id=0):
    """the reference of the bit rule: rbf_eval_model on a contiguous copy of every column"""
    out = np.empty((m, W.shape[0]))
    for q in range(W.shape[0]):
        d_w, d_s = dev(W[q]), dev(np.zeros(m))
        ctx.rbf_eval(kind, eps, d_x.ptr, n, dim, xtda, ptr(d_w), d_y.ptr, m, ytda, ptr(d_s), model_id=model_id)
        ctx.sync()
        out[:, q] = d_s.cpu().numpy()
    return out


# ---------------------------------------------------------------------------------------------- 1. the sweep, bitwise
@pytest.mark.parametrize("n", [513, 1100])          # the plain kernel, one centre past its tiles; the culled kernel (N >= 1024)
@pytest.mark.parametrize("dim", [1, 2, 3])
@pytest.mark.parametrize("kind", [GAUSSIAN, TPS, WENDLAND])
def test_sweep_is_bitwise_the_scalar_sweep_per_column(pkg, orc, kind, dim, n):
    ks = field_counts(pkg)
    kmax, xtda, ytda = ks[-1], dim + 1, dim + 2
    x = orc.synth_centres(n, dim)
    eps = shape_eps(orc, kind, n, dim)
    W = np.random.default_rng(1000 * kind + 10 * n + dim).standard_normal((kmax, n))
    ctx = pkg.HipContext.on_torch_stream(0)
    d_x = Canaried(x, ld=xtda)
    for m in (320, 5000):                            # 5000: the target sort
        y = targets(orc, x, m)
        if kind != TPS:
            y[7, dim - 1] = np.nan
        d_y = Canaried(y, ld=ytda)
        want = scalar_columns(ctx, kind, eps, d_x, n, dim, xtda, W, d_y, m, ytda)
        if kind != TPS:
            assert np.isnan(want[7]).all()
        for k in ks:
            ldw, stda = n + 3, k + 2
            d_w, d_s = Canaried(W[:k], ld=ldw, off=1), Canaried(np.zeros((m, k)), ld=stda, off=1)
            st = ctx.rbf_eval_fields(kind, eps, d_x.ptr, n, dim, xtda, d_w.ptr, ldw, k, d_y.ptr, m, ytda, d_s.ptr, stda)
            ctx.sync()
            assert st == 0
            got = d_s.get()
            if kind != TPS:
                assert np.isnan(got[7]).all()        # a NaN coordinate: NaN in all k outputs of the row
            for q in range(k):
                assert np.array_equal(bits(got[:, q]), bits(want[:, q])), (kind, dim, n, m, k, q)
            assert d_w.padding_intact() and d_s.padding_intact()
        assert d_y.padding_intact()
    assert d_x.padding_intact()
    ctx.close()


@pytest.mark.parametrize("kind", [GAUSSIAN, TPS, WENDLAND])
def test_sweep_large_batch(pkg, orc, kind):
    dim, n, m = 2, 1100, 131077
    k = pkg.HipContext.rbf_fields_block() + 1
    x = orc.synth_centres(n, dim)
    eps = shape_eps(orc, kind, n, dim)
    W = np.random.default_rng(kind).standard_normal((k, n))
    y = targets(orc, x, m)
    ctx = pkg.HipContext.on_torch_stream(0)
    d_x, d_y = Canaried(x), Canaried(y)
    want = scalar_columns(ctx, kind, eps, d_x, n, dim, dim, W, d_y, m, dim)
    d_w, d_s = Canaried(W, ld=n + 1), Canaried(np.zeros((m, k)), ld=k + 1)
    assert ctx.rbf_eval_fields(kind, eps, d_x.ptr, n, dim, dim, d_w.ptr, n + 1, k, d_y.ptr, m, dim, d_s.ptr, k + 1) == 0
    ctx.sync()
    assert np.array_equal(bits(d_s.get()), bits(want))
    assert d_s.padding_intact() and d_w.padding_intact()
    ctx.close()


def test_raw_entry_arguments_and_tail(pkg, orc):
    dim, n, m, k = 2, 513, 64 + N_SITES, 3
    x = orc.synth_centres(n, dim)
    eps = shape_eps(orc, WENDLAND, n, dim)
    W = np.random.default_rng(5).standard_normal((k, n))
    y = targets(orc, x, m)
    ctx = pkg.HipContext.on_torch_stream(0)
    d_x, d_y, d_w = Canaried(x), Canaried(y), Canaried(W)
    # the tail: field q has the bits of rbf_eval_affine / krige_eval on column q
    tail = np.array([[0.5, 1.0, -2.0], [3.0, 0.0, 0.0], [0.0, 0.0, 0.25]])
    d_s = Canaried(np.zeros((m, k)))
    assert ctx.rbf_eval_fields(WENDLAND, eps, d_x.ptr, n, dim, dim, d_w.ptr, n, k, d_y.ptr, m, dim, d_s.ptr, k, tail=tail) == 0
    ctx.sync()
    got = d_s.get()
    for q in range(k):
        d_c, d_v = dev(W[q]), dev(np.zeros(m))
        if q == 1:
            ctx.krige_eval(WENDLAND, eps, tail[q, 0], d_x.ptr, n, dim, dim, ptr(d_c), d_y.ptr, m, dim, ptr(d_v))
        else:
            ctx.rbf_eval_affine(WENDLAND, eps, tail[q], d_x.ptr, n, dim, dim, ptr(d_c), d_y.ptr, m, dim, ptr(d_v))
        ctx.sync()
        assert np.array_equal(bits(got[:, q]), bits(d_v.cpu().numpy())), q
    # m = 0 succeeds and touches nothing; bad arguments
    p = d_y.ptr
    ev = lambda **o: ctx.rbf_eval_fields(o.get("kind", WENDLAND), eps, d_x.ptr, n, o.get("dim", dim), dim, o.get("w", d_w.ptr), o.get("ldw", n),
                                         o.get("k", k), o.get("y", p), o.get("m", m), dim, o.get("s", d_s.ptr), o.get("stda", k))
    assert ev(m=0, y=None, s=None) == 0
    assert ev(stda=k - 1) == pkg.GSL_EINVAL and ev(ldw=n - 1) == pkg.GSL_EINVAL
    assert ev(k=0) == pkg.GSL_EINVAL and ev(k=65, stda=65) == pkg.GSL_EINVAL
    assert ev(dim=4) == pkg.GSL_EINVAL and ev(kind=7) == pkg.GSL_EINVAL
    assert ev(s=None) == pkg.capi.GSL_EFAULT and ev(y=None) == pkg.capi.GSL_EFAULT and ev(w=None) == pkg.capi.GSL_EFAULT
    d_phi = torch.empty((n, n), dtype=torch.float64, device="cuda")
    assert ctx.rbf_solve_fields(TPS, 0.0, d_x.ptr, n, dim, dim, ptr(d_phi), n, d_w.ptr, n, k)[0] == pkg.GSL_EINVAL
    assert ctx.krige_solve_fields(TPS, 0.0, 0.0, d_x.ptr, n, dim, dim, ptr(d_phi), n, d_w.ptr, n, k)[0] == pkg.GSL_EINVAL
    assert ctx.rbf_solve_fields(GAUSSIAN, eps, d_x.ptr, n, dim, dim, ptr(d_phi), n, d_w.ptr, n, 65)[0] == pkg.GSL_EINVAL
    assert ctx.rbf_solve_fields(GAUSSIAN, eps, d_x.ptr, n, dim, dim, ptr(d_phi), n, d_w.ptr, n - 1, k)[0] == pkg.GSL_EINVAL
    assert ctx.rbf_solve_fields(GAUSSIAN, eps, d_x.ptr, n, dim, dim, None, n, d_w.ptr, n, k)[0] == pkg.capi.GSL_EFAULT
    ctx.close()


# ---------------------------------------------------------------------------------------------- 2. the packed-centre cache
def test_cache_scalar_and_fields_calls_on_one_model_id(pkg, orc):
    dim, n, m = 2, 1100, 320
    k = pkg.HipContext.rbf_fields_block() + 1
    x = orc.synth_centres(n, dim)
    eps = shape_eps(orc, GAUSSIAN, n, dim)
    rng = np.random.default_rng(11)
    W, other = rng.standard_normal((k, n)), rng.standard_normal(n)
    y = targets(orc, x, m)
    ctx = pkg.HipContext.on_torch_stream(0)
    d_x, d_y, d_w, d_o = dev(x), dev(y), dev(W), dev(other)

    def fields(model_id):
        d_s = dev(np.zeros((m, k)))
        assert ctx.rbf_eval_fields(GAUSSIAN, eps, ptr(d_x), n, dim, dim, ptr(d_w), n, k, ptr(d_y), m, dim, ptr(d_s), k, model_id=model_id) == 0
        ctx.sync()
        return d_s.cpu().numpy()

    def scalar(d_col, model_id):
        d_s = dev(np.zeros(m))
        ctx.rbf_eval(GAUSSIAN, eps, ptr(d_x), n, dim, dim, ptr(d_col), ptr(d_y), m, dim, ptr(d_s), model_id=model_id)
        ctx.sync()
        return d_s.cpu().numpy()

    want_f, want_0, want_o = fields(0), scalar(d_w, 0), scalar(d_o, 0)       # d_w points at column 0
    assert np.array_equal(bits(want_f[:, 0]), bits(want_0))
    mid = 77
    assert np.array_equal(bits(fields(mid)), bits(want_f))
    assert np.array_equal(bits(scalar(d_w, mid)), bits(want_0))
    assert np.array_equal(bits(fields(mid)), bits(want_f))
    assert np.array_equal(bits(scalar(d_o, mid)), bits(want_o))
    assert np.array_equal(bits(fields(mid)), bits(want_f))
    ctx.close()


# ---------------------------------------------------------------------------------------------- 3. the solves
@pytest.mark.parametrize("n", [256, 300])           # a multiple of 128: the folded forward substitution; else the two sweeps
@pytest.mark.parametrize("kind", [GAUSSIAN, WENDLAND])
def test_rbf_solve_fields(pkg, orc, kind, n):
    dim, m, ldw = 2, 200 + N_SITES, n + 4
    x = orc.synth_centres(n, dim)
    eps = shape_eps(orc, kind, n, dim)
    y = targets(orc, x, m)
    F = responses(orc, x, 11)
    want = np.stack([orc.rbf_eval(kind, eps, x, orc.rbf_solve(kind, eps, x, np.ascontiguousarray(F[:, q])), y) for q in range(11)], axis=1)
    ctx = pkg.HipContext.on_torch_stream(0)
    d_x, d_y = dev(x), dev(y)
    for k in (1, 5, 6, 11):                          # across the groups of 5 right-hand sides
        d_phi = torch.empty((n, n), dtype=torch.float64, device="cuda")
        d_w, d_s = Canaried(F[:, :k].T, ld=ldw), dev(np.zeros((m, k)))
        st, route = ctx.rbf_solve_fields(kind, eps, ptr(d_x), n, dim, dim, ptr(d_phi), n, d_w.ptr, ldw, k)
        assert st == 0 and route == 1
        assert ctx.rbf_eval_fields(kind, eps, ptr(d_x), n, dim, dim, d_w.ptr, ldw, k, ptr(d_y), m, dim, ptr(d_s), k) == 0
        ctx.sync()
        got = d_s.cpu().numpy()
        for q in range(k):
            err = relerr(got[:, q], want[:, q])
            print(f"kind {kind} n {n} k {k} field {q}: relerr {err:.3e}")
            assert err < TOL
        assert d_w.padding_intact()
    ctx.close()


@pytest.mark.parametrize("n", [256, 300])
def test_krige_solve_fields(pkg, orc, n):
    dim, m, k, nugget, ldw = 2, 200 + N_SITES, 5, 1e-3, n + 2          # six right-hand sides
    x = orc.synth_centres(n, dim)
    eps = shape_eps(orc, GAUSSIAN, n, dim)
    y = targets(orc, x, m)
    F = responses(orc, x, k)
    ctx = pkg.HipContext.on_torch_stream(0)
    d_x, d_y = dev(x), dev(y)
    d_phi = torch.empty((n, n), dtype=torch.float64, device="cuda")
    d_w, d_s = Canaried(F.T, ld=ldw), dev(np.zeros((m, k)))
    st, route, means = ctx.krige_solve_fields(GAUSSIAN, eps, nugget, ptr(d_x), n, dim, dim, ptr(d_phi), n, d_w.ptr, ldw, k)
    assert st == 0 and route == 7
    tail = np.zeros((k, dim + 1))
    tail[:, 0] = means
    assert ctx.rbf_eval_fields(GAUSSIAN, eps, ptr(d_x), n, dim, dim, d_w.ptr, ldw, k, ptr(d_y), m, dim, ptr(d_s), k, tail=tail) == 0
    ctx.sync()
    got = d_s.cpu().numpy()
    for q in range(k):
        w, mu = orc.krige_solve(GAUSSIAN, eps, nugget, x, np.ascontiguousarray(F[:, q]))
        err = relerr(got[:, q], orc.krige_eval(GAUSSIAN, eps, mu, x, w, y))
        print(f"kriging n {n} field {q}: mean {means[q]:.6e} vs {mu:.6e}, relerr {err:.3e}")
        assert abs(means[q] - mu) <= TOL * abs(mu) and err < TOL
    assert d_w.padding_intact()
    ctx.close()


# ---------------------------------------------------------------------------------------------- 4. the facade
def facade_model(pkg, orc, typ, n, k=3):
    dim = 2
    x = orc.synth_centres(n, dim)
    F = responses(orc, x, k)
    s = pkg.Sinterp(typ, dim, n, 0)
    eps = shape_eps(orc, KIND[typ], n, dim)
    if typ != "wendland":
        assert s.set_shape(eps) == 0
    if typ == "kriging":
        assert s.set_nugget(1e-3) == 0
    return s, x, F, eps


def oracle_field(orc, typ, eps, x, f, y):
    f = np.ascontiguousarray(f)
    if typ == "kriging":
        w, mu = orc.krige_solve(GAUSSIAN, eps, 1e-3, x, f)
        return orc.krige_eval(GAUSSIAN, eps, mu, x, w, y), mu, None
    if typ == "tps_affine":
        w, c = orc.rbf_solve_affine(TPS, 0.0, x, f)
        return orc.rbf_eval_affine(TPS, 0.0, c, x, w, y), None, c
    w = orc.rbf_solve(KIND[typ], eps, x, f)
    return orc.rbf_eval(KIND[typ], eps, x, w, y), None, None


@pytest.mark.parametrize("typ", ["gaussian", "tps", "tps_affine", "wendland", "kriging"])
def test_facade(pkg, orc, typ):
    n, k = (600 if typ == "tps_affine" else 513), 3
    s, x, F, eps = facade_model(pkg, orc, typ, n, k)
    y = targets(orc, x, 300 + N_SITES)
    assert s.n_fields() == 0
    assert s.init_fields(x, F) == 0 and s.n_fields() == k
    assert s.route() in {"gaussian": (1,), "wendland": (1,), "kriging": (7,), "tps": (2, 3), "tps_affine": (9, 10)}[typ]   # shared: 1 / 7
    S = np.full((len(y), k + 2), -7.0)              # a wider matrix: the row stride is honoured, the padding untouched
    st, _ = s.eval_fields_many(y, out=S[:, :k])
    assert st == 0 and (S[:, k:] == -7.0).all()
    for q in range(k):
        want, mu, c = oracle_field(orc, typ, eps, x, F[:, q], y)
        err = relerr(S[:, q], want)
        print(f"{typ} field {q}: relerr {err:.3e}")
        assert err < TOL
        if mu is not None:
            st, got_mu = s.field_mean(q)
            assert st == 0 and abs(got_mu - mu) <= TOL * abs(mu)
        else:
            assert s.field_mean(q)[0] == pkg.GSL_EINVAL
        if c is not None:
            st, got_c = s.field_poly(q)
            assert st == 0 and np.abs(got_c - c).max() <= 1e-8 * max(1.0, np.abs(c).max())
        else:
            assert s.field_poly(q)[0] == pkg.GSL_EINVAL
    # to every existing entry the interpolant is field 0's
    st, v0, _ = s.eval_many(y)
    assert st == 0 and np.array_equal(bits(v0), bits(S[:, 0]))
    st, row0 = s.eval_fields_e(y[0])
    assert st == 0 and np.array_equal(bits(row0), bits(S[0, :k]))
    st, w0 = s.field_weights(0)
    st2, w = s.weights()
    assert st == 0 and st2 == 0 and np.array_equal(bits(w0), bits(w))
    assert s.field_weights(k)[0] == pkg.capi.GSL_EBADLEN and s.field_weights(k - 1)[0] == 0
    if typ == "kriging":
        assert s.mean()[1] == s.field_mean(0)[1]
    if typ == "tps_affine":
        assert np.array_equal(s.poly()[1], s.field_poly(0)[1])
    # resident, with a row pitch
    d_y, d_s = dev(y), Canaried(np.zeros((len(y), k)), ld=k + 1)
    assert s.eval_fields_resident(ptr(d_y), len(y), 2, d_s.ptr, k + 1) == 0
    torch.cuda.synchronize()
    assert np.array_equal(bits(d_s.get()), bits(S[:, :k])) and d_s.padding_intact()
    assert s.eval_fields_resident(ptr(d_y), len(y), 2, d_s.ptr, k - 1) == pkg.GSL_EINVAL
    assert s.eval_fields_many(y, out=np.zeros((len(y), k + 1)))[0] == pkg.capi.GSL_EBADLEN
    # re-initialisation: one field again, then another field count
    assert s.init(x, np.ascontiguousarray(F[:, 1])) == 0 and s.n_fields() == 1
    st, one = s.eval_fields_many(y)
    st2, plain, _ = s.eval_many(y)
    assert st == 0 and st2 == 0 and one.shape == (len(y), 1) and np.array_equal(bits(one[:, 0]), bits(plain))
    assert relerr(plain, oracle_field(orc, typ, eps, x, F[:, 1], y)[0]) < TOL
    assert s.init_fields(x, np.ascontiguousarray(F[:, 1:])) == 0 and s.n_fields() == 2
    st, two = s.eval_fields_many(y)
    assert st == 0 and relerr(two[:, 1], oracle_field(orc, typ, eps, x, F[:, 2], y)[0]) < TOL
    assert relerr(two[:, 0], plain) < TOL


def test_affine_exactness_per_field(pkg, orc):
    n, dim = 600, 2
    x = orc.synth_centres(n, dim)
    coef = np.array([[3.0, 2.0, -5.0], [-1.0, 0.5, 0.25], [0.0, -4.0, 1.5]])
    F = np.ascontiguousarray(coef[:, 0][None, :] + x @ coef[:, 1:].T)
    s = pkg.Sinterp("tps_affine", dim, n, 0)
    assert s.init_fields(x, F) == 0
    y = targets(orc, x, 300 + N_SITES)
    st, S = s.eval_fields_many(y)
    assert st == 0
    want = coef[:, 0][None, :] + y @ coef[:, 1:].T
    for q in range(3):
        err = relerr(S[:, q], want[:, q])
        print(f"affine exactness field {q}: relerr {err:.3e}")
        assert err < TOL


def test_kriging_variance_after_init_fields(pkg, orc):
    n = 513
    s, x, F, eps = facade_model(pkg, orc, "kriging", n)
    y = targets(orc, x, 200 + N_SITES)
    assert s.set_variance(True) == 0 and s.init_fields(x, F) == 0 and s.route() == 7
    st, var_fields = s.eval_variance_many(y)
    assert st == 0
    one, _, _, _ = facade_model(pkg, orc, "kriging", n)
    assert one.set_variance(True) == 0 and one.init(x, np.ascontiguousarray(F[:, 0])) == 0
    st, var_one = one.eval_variance_many(y)
    assert st == 0 and np.abs(var_fields - var_one).max() < TOL        # absolute: the sill is 1 (tests/test_gpu_krige_variance.py)


def test_checkpoint_of_several_fields_is_refused(pkg, orc, tmp_path):
    s, x, F, eps = facade_model(pkg, orc, "gaussian", 513)
    assert s.init_fields(x, F) == 0
    path = tmp_path / "fields.bin"
    assert s.fwrite(str(path)) == pkg.GSL_EUNSUP
    assert path.stat().st_size == 0
    assert s.init_fields(x, np.ascontiguousarray(F[:, :1])) == 0 and s.fwrite(str(path)) == 0 and path.stat().st_size > 0


def test_device_list(pkg, orc):
    s, x, F, eps = facade_model(pkg, orc, "gaussian", 1100)
    y = targets(orc, x, 300 + N_SITES)
    assert s.init_fields(x, F) == 0
    st, S = s.eval_fields_many(y)
    assert st == 0
    grp, _, _, _ = facade_model(pkg, orc, "gaussian", 1100)
    assert grp.set_device_list([0, 0]) == 0 and grp.init_fields(x, F) == 0
    st, S2 = grp.eval_fields_many(y)
    assert st == 0 and np.array_equal(bits(S2), bits(S))
    st, v0, _ = grp.eval_many(y)                     # the sharded scalar path reads column 0 of every member's model
    assert st == 0 and np.array_equal(bits(v0), bits(S[:, 0]))


@pytest.mark.parametrize("how", ["cholesky2", "rcond"])
def test_per_column_route(pkg, orc, how):
    s, x, F, eps = facade_model(pkg, orc, "gaussian", 513)
    y = targets(orc, x, 300 + N_SITES)
    if how == "cholesky2":
        assert s.set_solver(pkg.capi.SOLVER_CHOLESKY2) == 0
    assert s.set_rcond(True) == 0
    assert s.init_fields(x, F) == 0 and s.route() == (4 if how == "cholesky2" else 1)
    st, rc = s.rcond()
    assert st == 0 and np.isfinite(rc) and 0.0 < rc < 1.0
    st, S = s.eval_fields_many(y)
    assert st == 0
    for q in range(F.shape[1]):
        assert relerr(S[:, q], oracle_field(orc, "gaussian", eps, x, F[:, q], y)[0]) < TOL


# ---------------------------------------------------------------------------------------------- 5. the existing path is untouched
def test_existing_path_before_and_after_a_fields_evaluation(pkg, orc):
    s, x, F, eps = facade_model(pkg, orc, "gaussian", 1100)
    y = targets(orc, x, 5000)
    assert s.init_fields(x, F) == 0
    st, before, _ = s.eval_many(y)
    assert st == 0
    st, S = s.eval_fields_many(y)
    assert st == 0
    st, after, _ = s.eval_many(y)
    assert st == 0 and np.array_equal(bits(before), bits(after)) and np.array_equal(bits(S[:, 0]), bits(before))
