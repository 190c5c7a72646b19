"""-m gpu: the raw device API (include/gsl_sinterp_hip.h) at every stride and alignment the header allows.

Every device array sits in a larger buffer whose padding (columns beyond the row length, the word before an offset
base, a tail) holds a NaN bit pattern (gpu_util.CANARY): a kernel that READS padding turns its result into NaN, a kernel
that WRITES outside its array changes the pattern.  Results are compared with the CPU oracle at the tolerances of the
dense tests, and -- where only a stride changes and the kernel route cannot -- with the dense call on a fresh context,
bit for bit.  The cases are chosen to reach each route once (odd lda and 8-byte aligned bases select the 32-wide
Cholesky path, the folded forward substitution needs n % 128 == 0, an even lda and a 16-byte aligned matrix)."""
import numpy as np
import pytest
import torch

from gpu_util import CANARY, Canaried, bits, dev, ptr

pytestmark = pytest.mark.gpu
TOL = 1e-10


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def spd(n, seed):
    rng = np.random.default_rng(seed)
    m = rng.random((n, n))
    return np.tril(m) + np.tril(m, -1).T + 10.0 * n * np.eye(n)


def strided(x, ld, off=0):
    """x (rows x dim) as a canaried device array with row stride ld"""
    return Canaried(x, ld=ld, off=off)


def rbf_eps(kind, n, dim, orc):
    if kind == 0:
        return orc.gaussian_eps(n, dim)
    if kind == 2:
        return 0.125 * n ** (1.0 / dim)          # Wendland: support radius 1 / eps
    return 0.0


# ------------------------------------------------------------------ Cholesky
@pytest.mark.parametrize("n,lda,off", [(256, 257, 0), (256, 258, 1), (384, 390, 0), (1000, 1001, 0), (1152, 1152, 1)])
def test_cholesky_decomp1_svx_strided(pkg, orc, n, lda, off):
    """odd lda / 8-byte aligned base: the 32-wide path of the default build; lda > n on the 128-wide path"""
    a = spd(n, n + lda)
    b = np.cos(np.arange(n) + 0.5)
    ctx = pkg.HipContext.on_torch_stream(0)
    A = Canaried(a, ld=lda, off=off)
    st, info = ctx.cholesky_decomp1(n, A.ptr, lda)
    assert st == 0 and info == 0
    got = A.get()
    st_o, want = orc.cholesky_decomp1(a)
    assert np.abs(np.tril(got) - np.tril(want)).max() <= 1e-12 * np.abs(np.tril(want)).max()
    assert np.array_equal(np.triu(got, 1), np.triu(a, 1))
    X = Canaried(b, off=off)
    ctx.cholesky_svx(n, A.ptr, lda, X.ptr)
    ctx.sync()
    xo = orc.cholesky_solve(want, b)
    assert np.abs(X.get() - xo).max() <= 1e-11 * np.abs(xo).max()
    assert A.padding_intact() and X.padding_intact()


@pytest.mark.parametrize("n,lda", [(256, 256), (640, 642), (300, 301)])
@pytest.mark.parametrize("extra", [0, 3])
@pytest.mark.parametrize("xoff", [0, 1])
def test_cholesky_factor_solve_layouts(pkg, orc, n, lda, extra, xoff):
    """gsl_sinterp_hip_cholesky_factor_solve: n = 256 / 640 take the folded forward substitution (fb 16- or only
    8-byte aligned, ldx = n or n + 3, 1..5 right-hand sides); n = 300 (odd lda) the factorisation + two sweeps."""
    ldx = n + extra
    a = spd(n, 7 * n)
    st_o, want = orc.cholesky_decomp1(a)
    ctx = pkg.HipContext.on_torch_stream(0)
    A = Canaried(a, ld=lda)
    rng = np.random.default_rng(n + extra + xoff)
    for nrhs in range(1, 6):
        B = rng.standard_normal((nrhs, n))
        A.set(a)
        X = Canaried(B, ld=ldx, off=xoff)
        st, info = ctx.cholesky_factor_solve(n, A.ptr, lda, X.ptr, ldx, nrhs)
        assert st == 0 and info == 0
        got = A.get()
        assert np.abs(np.tril(got) - np.tril(want)).max() <= 1e-12 * np.abs(np.tril(want)).max()
        assert np.array_equal(np.triu(got, 1), np.triu(a, 1))
        x = X.get()
        for q in range(nrhs):
            xo = orc.cholesky_solve(want, B[q])
            assert np.abs(x[q] - xo).max() <= 1e-11 * np.abs(xo).max(), (nrhs, q)
        assert A.padding_intact() and X.padding_intact(), nrhs


def test_cholesky_factor_solve_reports_edom_and_bad_arguments(pkg):
    n = 256
    a = spd(n, 1)
    a[200, 200] = -1.0
    ctx = pkg.HipContext.on_torch_stream(0)
    A, X = Canaried(a), Canaried(np.ones((2, n)))
    st, info = ctx.cholesky_factor_solve(n, A.ptr, n, X.ptr, n, 2)
    assert st == pkg.capi.GSL_EDOM and info == 201
    for ldx, nrhs in ((n - 1, 1), (n, 0), (n, 6)):
        st, _ = ctx.cholesky_factor_solve(n, A.ptr, n, X.ptr, ldx, nrhs)
        assert st == pkg.capi.GSL_EINVAL


# ------------------------------------------------------------------ RBF fill
@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_rbf_fill_centre_stride(pkg, orc, kind, dim):
    n, lda = 300, 301
    x = orc.synth_centres(n, dim)
    eps = rbf_eps(kind, n, dim, orc)
    dense_ctx = pkg.HipContext.on_torch_stream(0)
    d_x, phi = dev(x), torch.empty((n, n), dtype=torch.float64, device="cuda")
    dense_ctx.rbf_fill(kind, eps, ptr(d_x), n, dim, dim, ptr(phi), n)
    dense = phi.cpu().numpy()
    want = orc.rbf_fill(kind, eps, x)
    assert np.abs(dense - want).max() <= 2e-15 * max(1.0, np.abs(want).max())
    for xtda in sorted({dim + 1, 4}):
        ctx = pkg.HipContext.on_torch_stream(0)
        X = strided(x, xtda)
        P = Canaried(np.zeros((n, n)), ld=lda)
        ctx.rbf_fill(kind, eps, X.ptr, n, dim, xtda, P.ptr, lda)
        ctx.sync()
        assert np.array_equal(bits(P.get()), bits(dense)), xtda
        assert X.padding_intact() and P.padding_intact(), xtda


# ------------------------------------------------------------------ RBF solve
@pytest.mark.parametrize("kind,n,extra,phi_off,force_lu,route", [
    (0, 512, 2, 0, "0", 1),     # fold on (n % 128 == 0, even lda, aligned)
    (0, 512, 2, 1, "0", 1),     # 8-byte aligned matrix: 32-wide path, sweeps after the factorisation
    (0, 700, 1, 0, "0", 1),
    (1, 512, 1, 0, "0", 2),     # shifted-SPD thin-plate spline + Woodbury
    (1, 700, 2, 1, "0", 2),
    (1, 512, 2, 0, "1", 3),     # pivoted LU
    (2, 700, 1, 0, "0", 1),     # Wendland
])
def test_rbf_solve_strided(pkg, orc, monkeypatch, kind, n, extra, phi_off, force_lu, route):
    dim, m = 2, 3000
    monkeypatch.setenv("GSL_SINTERP_FORCE_LU", force_lu)
    x = orc.synth_centres(n, dim)
    f = orc.synth_response(x)
    y = orc.synth_targets(0, m, dim)
    eps = rbf_eps(kind, n, dim, orc)
    lda = n + extra
    ctx = pkg.HipContext.on_torch_stream(0)
    X = strided(x, dim + 1)
    P = Canaried(np.zeros((n, n)), ld=lda, off=phi_off)
    W = Canaried(f, off=1)
    st, r = ctx.rbf_solve(kind, eps, X.ptr, n, dim, dim + 1, P.ptr, lda, W.ptr)
    assert st == 0 and r == route
    w_o = orc.rbf_solve(kind, eps, x, f)
    if kind != 1:
        assert relerr(W.get(), w_o) < TOL
    Y, S = strided(y, dim + 1), Canaried(np.zeros(m), off=1)
    ctx.rbf_eval(kind, eps, X.ptr, n, dim, dim + 1, W.ptr, Y.ptr, m, dim + 1, S.ptr)
    ctx.sync()
    assert relerr(S.get(), orc.rbf_eval(kind, eps, x, w_o, y)) < TOL
    assert X.padding_intact() and P.padding_intact() and W.padding_intact() and Y.padding_intact() and S.padding_intact()


@pytest.mark.parametrize("solver,route", [(0, 1), (1, 4), (2, 5), (3, 6)])
def test_rbf_solve_ex_strided(pkg, orc, solver, route):
    """each explicit solver once, with rcond (DEFAULT + rcond keeps the original above the diagonal)"""
    n, dim, m = 512, 2, 3000
    x = orc.synth_centres(n, dim)
    f = orc.synth_response(x)
    y = orc.synth_targets(0, m, dim)
    eps = orc.gaussian_eps(n, dim)
    lda = n + 1
    ctx = pkg.HipContext.on_torch_stream(0)
    X = strided(x, 3)
    P = Canaried(np.zeros((n, n)), ld=lda, off=1)
    W = Canaried(f, off=1)
    st, r, rc = ctx.rbf_solve_ex(0, eps, X.ptr, n, dim, 3, P.ptr, lda, W.ptr, solver, want_rcond=True)
    assert st == 0 and r == route
    w_o = orc.rbf_solve(0, eps, x, f)
    Y, S = strided(y, 3), Canaried(np.zeros(m))
    ctx.rbf_eval(0, eps, X.ptr, n, dim, 3, W.ptr, Y.ptr, m, 3, S.ptr)
    ctx.sync()
    want = orc.rbf_eval(0, eps, x, w_o, y)
    assert np.abs(S.get() - want).max() <= 1e-10 * np.abs(want).max()
    if route in (1, 4):
        phi = orc.rbf_fill(0, eps, x)
        llt = orc.cholesky_decomp1(phi)[1] if route == 1 else orc.cholesky_decomp2(phi)[1]
        r_o = orc.cholesky_rcond(llt)
        assert abs(rc - r_o) <= 1e-6 * r_o
    else:
        assert np.isnan(rc)
    assert X.padding_intact() and P.padding_intact() and W.padding_intact() and Y.padding_intact() and S.padding_intact()


# ------------------------------------------------------------------ thin-plate spline with its affine tail
@pytest.mark.parametrize("dim,n", [(1, 300), (2, 512), (3, 640)])
@pytest.mark.parametrize("force_lu,route", [("0", 9), ("1", 10)])
def test_rbf_solve_affine_poly_buffer_and_layouts(pkg, orc, monkeypatch, dim, n, force_lu, route):
    """h_poly holds dim + 1 doubles (the header's size): nothing behind h_poly[dim] is written by the solve or read by
    the evaluation.  Route 10 factors the (n + dim + 1)-row augmented matrix at lda = n + dim + 1 exactly."""
    monkeypatch.setenv("GSL_SINTERP_FORCE_LU", force_lu)
    m, k = 2500, dim + 1
    x = orc.synth_centres(n, dim) * 2.0 - 0.5
    f = orc.synth_response(orc.synth_centres(n, dim)) + 1.5
    y = orc.synth_targets(0, m, dim) * 2.0 - 0.5
    lda = n + k
    rows = n + k if route == 10 else n
    ctx = pkg.HipContext.on_torch_stream(0)
    X = strided(x, dim + 1)
    P = Canaried(np.zeros((rows, rows)), ld=lda, tail=3 * lda)
    W = Canaried(f, off=1)
    h_poly = np.full(8, CANARY, dtype=np.uint64).view(np.float64)
    st, r = ctx.rbf_solve_affine(1, 0.0, X.ptr, n, dim, dim + 1, P.ptr, lda, W.ptr, h_poly)
    assert st == 0 and r == route
    assert (h_poly[k:].view(np.uint64) == CANARY).all()
    w_o, c_o = orc.rbf_solve_affine(1, 0.0, x, f)
    assert np.abs(h_poly[:k] - c_o).max() <= 1e-7 * max(1.0, np.abs(c_o).max())
    Y, S = strided(y, dim + 2), Canaried(np.zeros(m), off=1)
    ctx.rbf_eval_affine(1, 0.0, h_poly, X.ptr, n, dim, dim + 1, W.ptr, Y.ptr, m, dim + 2, S.ptr)
    ctx.sync()
    got = S.get()
    assert np.isfinite(got).all()
    assert relerr(got, orc.rbf_eval_affine(1, 0.0, c_o, x, w_o, y)) < TOL
    assert X.padding_intact() and P.padding_intact() and W.padding_intact() and Y.padding_intact() and S.padding_intact()


# ------------------------------------------------------------------ kriging
@pytest.mark.parametrize("dim,nugget,extra", [(2, 0.0, 1), (2, 1e-3, 2), (3, 0.0, 2), (3, 1e-3, 1)])
def test_krige_solve_eval_strided(pkg, orc, dim, nugget, extra):
    n, m = 600, 3000
    x = orc.synth_centres(n, dim)
    f = orc.synth_response(x) + 3.0
    y = orc.synth_targets(0, m, dim)
    eps = orc.gaussian_eps(n, dim)
    ctx = pkg.HipContext.on_torch_stream(0)
    X = strided(x, dim + 1)
    P = Canaried(np.zeros((n, n)), ld=n + extra)
    W = Canaried(f, off=1)
    st, route, mean = ctx.krige_solve(0, eps, nugget, X.ptr, n, dim, dim + 1, P.ptr, n + extra, W.ptr)
    assert st == 0 and route == 7
    w_o, mu = orc.krige_solve(0, eps, nugget, x, f)
    assert abs(mean - mu) <= TOL * abs(mu) and relerr(W.get(), w_o) < 1e-8
    Y, S = strided(y, dim + 2), Canaried(np.zeros(m))
    ctx.krige_eval(0, eps, mean, X.ptr, n, dim, dim + 1, W.ptr, Y.ptr, m, dim + 2, S.ptr)
    ctx.sync()
    assert relerr(S.get(), orc.krige_eval(0, eps, mu, x, w_o, y)) < TOL
    assert X.padding_intact() and P.padding_intact() and W.padding_intact() and Y.padding_intact() and S.padding_intact()


def test_krige_pivoted_route_strided_is_bit_identical_to_dense(pkg, orc):
    """a flat covariance (numerically semi-definite) takes the pivoted LDL^T route 8, whose factorisation is
    reference-order and independent of the layout: strided centres and matrix give the bits of the dense call"""
    n, dim, m = 300, 2, 2000
    x = orc.synth_centres(n, dim)
    f = orc.synth_response(x)
    y = orc.synth_targets(0, m, dim)

    def solve(eps, xtda, lda, off):
        ctx = pkg.HipContext.on_torch_stream(0)
        X = strided(x, xtda)
        P = Canaried(np.zeros((n, n)), ld=lda, off=off)
        W = Canaried(f, off=off)
        st, route, mean = ctx.krige_solve(0, eps, 0.0, X.ptr, n, dim, xtda, P.ptr, lda, W.ptr)
        if st != 0 or route != 8:
            return st, route, None
        S = Canaried(np.zeros(m))
        Y = strided(y, xtda)
        ctx.krige_eval(0, eps, mean, X.ptr, n, dim, xtda, W.ptr, Y.ptr, m, xtda, S.ptr)
        ctx.sync()
        assert X.padding_intact() and P.padding_intact() and W.padding_intact() and S.padding_intact()
        return st, route, (mean, W.get(), S.get())
    for factor in (0.05, 0.02, 0.01):
        eps = factor * orc.gaussian_eps(n, dim)
        st, route, dense = solve(eps, dim, n, 0)
        assert st == 0 and route in (7, 8)
        if route == 8:
            break
    assert route == 8
    st, route, wide = solve(eps, dim + 1, n + 1, 1)
    assert st == 0 and route == 8
    assert np.array_equal(bits(np.array([wide[0]])), bits(np.array([dense[0]])))
    assert np.array_equal(bits(wide[1]), bits(dense[1])) and np.array_equal(bits(wide[2]), bits(dense[2]))
    assert np.isfinite(dense[2]).all()


# ------------------------------------------------------------------ evaluation sweep
@pytest.mark.parametrize("kind,n", [(0, 700), (0, 3000), (1, 700), (2, 3000)])
@pytest.mark.parametrize("m", [3000, 9000])
def test_rbf_eval_strides_bit_identical_to_dense(pkg, orc, kind, n, m):
    """plain (small model) and culled Gaussian sweeps, thin-plate spline, Wendland; below and above the 4096-target sort"""
    dim = 2
    x = orc.synth_centres(n, dim)
    eps = rbf_eps(kind, n, dim, orc)
    w = np.random.default_rng(n + m).standard_normal(n)
    y = orc.synth_targets(0, m, dim)
    y[-20:] += 30.0
    dctx = pkg.HipContext.on_torch_stream(0)
    d_x, d_w, d_y = dev(x), dev(w), dev(y)
    d_s = torch.empty(m, dtype=torch.float64, device="cuda")
    dctx.rbf_eval(kind, eps, ptr(d_x), n, dim, dim, ptr(d_w), ptr(d_y), m, dim, ptr(d_s))
    dctx.sync()
    dense = d_s.cpu().numpy()
    idx = np.arange(0, m, 3)
    assert relerr(dense[idx], orc.rbf_eval(kind, eps, x, w, np.ascontiguousarray(y[idx]))) < TOL
    ctx = pkg.HipContext.on_torch_stream(0)
    X, W, Y, S = strided(x, dim + 2), Canaried(w, off=1), strided(y, dim + 1, off=1), Canaried(np.zeros(m), off=1)
    ctx.rbf_eval(kind, eps, X.ptr, n, dim, dim + 2, W.ptr, Y.ptr, m, dim + 1, S.ptr)
    ctx.sync()
    assert np.array_equal(bits(S.get()), bits(dense))
    assert X.padding_intact() and W.padding_intact() and Y.padding_intact() and S.padding_intact()


# ------------------------------------------------------------------ solver breadth at lda = n + 1
def test_solver_breadth_padded_lda(pkg, orc):
    n = 200
    lda = n + 1
    ctx = pkg.HipContext.on_torch_stream(0)
    a = spd(n, 11) * np.outer(np.linspace(1.0, 30.0, n), np.linspace(1.0, 30.0, n))
    b = np.arange(1.0, n + 1.0)
    # decomp2 / svx2 / rcond
    st_o, v_o, s_o = orc.cholesky_decomp2(a)
    A, S = Canaried(a, ld=lda), Canaried(np.zeros(n), off=1)
    st, info = ctx.cholesky_decomp2(n, A.ptr, lda, S.ptr)
    assert st == 0 and info == 0
    ctx.sync()
    got = A.get()
    assert np.array_equal(S.get(), s_o)
    assert np.abs(np.tril(got) - np.tril(v_o)).max() <= 1e-12
    assert np.array_equal(np.triu(got, 1), np.triu(v_o, 1))
    X = Canaried(b, off=1)
    ctx.cholesky_svx2(n, A.ptr, lda, S.ptr, X.ptr)
    ctx.sync()
    x_o = orc.cholesky_solve2(v_o, s_o, b)
    assert np.abs(X.get() - x_o).max() <= 1e-10 * np.abs(x_o).max()
    r, r_o = ctx.cholesky_rcond(n, A.ptr, lda), orc.cholesky_rcond(v_o)
    assert abs(r - r_o) <= 1e-6 * r_o
    assert A.padding_intact() and S.padding_intact() and X.padding_intact()
    # pivoted LDL^T: the oracle's bits
    st_o, ldlt_o, perm_o = orc.pcholesky_decomp(a)
    A = Canaried(a, ld=lda)
    d_p = torch.empty(n, dtype=torch.int32, device="cuda")
    ctx.pcholesky_decomp(n, A.ptr, lda, ptr(d_p))
    ctx.sync()
    assert np.array_equal(d_p.cpu().numpy().astype(np.uintp), perm_o)
    assert np.array_equal(bits(A.get()), bits(ldlt_o))
    X = Canaried(b, off=1)
    ctx.pcholesky_svx(n, A.ptr, lda, ptr(d_p), X.ptr)
    ctx.sync()
    x_o = orc.pcholesky_solve(ldlt_o, perm_o, b)
    assert np.abs(X.get() - x_o).max() <= 1e-10 * max(1.0, np.abs(x_o).max())
    r, r_o = ctx.pcholesky_rcond(n, A.ptr, lda, ptr(d_p)), orc.pcholesky_rcond(ldlt_o, perm_o)
    assert abs(r - r_o) <= 1e-6 * r_o
    assert A.padding_intact() and X.padding_intact()
    st_o, ldlt2_o, perm2_o, s2_o = orc.pcholesky_decomp2(a)
    A, S = Canaried(a, ld=lda), Canaried(np.zeros(n), off=1)
    ctx.pcholesky_decomp2(n, A.ptr, lda, ptr(d_p), S.ptr)
    ctx.sync()
    assert np.array_equal(S.get(), s2_o) and np.array_equal(d_p.cpu().numpy().astype(np.uintp), perm2_o)
    assert np.array_equal(bits(A.get()), bits(ldlt2_o))
    X = Canaried(b, off=1)
    ctx.pcholesky_svx2(n, A.ptr, lda, ptr(d_p), S.ptr, X.ptr)
    ctx.sync()
    x_o = orc.pcholesky_solve2(ldlt2_o, perm2_o, s2_o, b)
    assert np.abs(X.get() - x_o).max() <= 1e-10 * np.abs(x_o).max()
    assert A.padding_intact() and S.padding_intact() and X.padding_intact()


@pytest.mark.parametrize("n", [100, 700])
def test_lu_refine_with_distinct_strides(pkg, orc, n):
    """A at lda = n + 1, its LU at ldlu = n + 3 (lu_refine reads both with their own stride)"""
    lda, ldlu = n + 1, n + 3
    rng = np.random.default_rng(n)
    a = rng.standard_normal((n, n)) + np.diag(np.linspace(1, 1e6, n))
    b = np.arange(1.0, n + 1.0)
    lu_o, perm_o, _ = orc.lu_decomp(a)
    st, x_o = orc.lu_solve(lu_o, perm_o, b)
    x0 = x_o * (1 + 1e-7 * np.cos(np.arange(n)))
    st, xr_o = orc.lu_refine(a, lu_o, perm_o, b, x0)
    ctx = pkg.HipContext.on_torch_stream(0)
    A, LU = Canaried(a, ld=lda), Canaried(a, ld=ldlu, off=1)
    d_perm = torch.empty(n, dtype=torch.int32, device="cuda")
    ctx.lu_decomp(n, LU.ptr, ldlu, ptr(d_perm))
    ctx.sync()
    assert np.array_equal(d_perm.cpu().numpy().astype(np.uintp), perm_o)
    assert np.abs(LU.get() - lu_o).max() <= 1e-9 * np.abs(lu_o).max()
    X, B, WK = Canaried(x0, off=1), Canaried(b, off=1), Canaried(np.zeros(n), off=1)
    assert ctx.lu_refine(n, A.ptr, lda, LU.ptr, ldlu, ptr(d_perm), B.ptr, X.ptr, WK.ptr) == 0
    ctx.sync()
    assert np.abs(X.get() - xr_o).max() <= 1e-10 * np.abs(xr_o).max()
    X2 = Canaried(b, off=1)
    assert ctx.lu_svx(n, LU.ptr, ldlu, ptr(d_perm), X2.ptr) == 0
    ctx.sync()
    assert np.abs(X2.get() - x_o).max() <= 1e-7 * np.abs(x_o).max()
    for c in (A, LU, X, B, WK, X2):
        assert c.padding_intact()
