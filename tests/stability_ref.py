"""Ill-conditioned test matrices, error measures and a numpy model of the blocked solver, for tests/test_stability_ref.py
(CPU) and tests/test_gpu_stability.py (GPU).  Pure numpy / scipy: nothing here touches the library.

ZOO      seeded generators of exactly symmetric float64 matrices whose condition numbers are those of the library's real
         inputs (Gaussian kernel matrices with a small nugget, prescribed spectra, graded and 2^+-900 scaled matrices,
         numerically semi-definite ones).
MEASURES backward and forward errors with the residuals taken beyond float64: products of two float64 matrices are
         formed from 20-bit integer slices of their rows (every slice product is exact in a float64 GEMM) and summed in
         np.longdouble, so a residual of a few eps is measured, not drowned in the rounding of its own evaluation.
MODEL    a short restatement of the documented algorithm -- right-looking blocked Cholesky whose row solve MULTIPLIES by
         the inverted 32 x 32 diagonal block, sweeps that multiply by inverted 64 x 64 blocks.  It is not a bound: it shows
         that a correct implementation of this design meets the bounds the GPU tests derive from LAPACK."""
import zlib

import numpy as np
import scipy.linalg as sla

EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble
MARGIN = 16.0            # 16 x the float64 reference's own figure, the rule of C_GRAD in tests/test_gpu_linear_fields.py

PD = ["spec_1e6", "spec_1e10", "gauss2d_a", "gauss2d_b", "gauss3d", "graded", "scaled_up", "scaled_down"]
SEMIDEF = ["semidef_gram", "semidef_gauss"]
SIZES = [96, 424, 1024, 2176]
AT_2176 = ["spec_1e10", "gauss2d_a", "graded"]


def sizes_of(name):
    return SIZES if name in AT_2176 else SIZES[:-1]


# ---------------------------------------------------------------- zoo
def _rng(tag, n):
    return np.random.default_rng([zlib.crc32(tag.encode()), n])


def _sym(a):
    return np.tril(a) + np.tril(a, -1).T


def spectrum(n, kappa, tag="spec"):
    """Q diag(lambda) Q^T, lambda_i = kappa^(-i / (n - 1)), Q from the QR of a standard normal matrix"""
    q, _ = np.linalg.qr(_rng(tag, n).standard_normal((n, n)))
    lam = kappa ** (-np.arange(n) / (n - 1.0))
    a = (q * lam) @ q.T
    return _sym((a + a.T) / 2)


def gauss_points(n, dim, tag):
    return _rng(tag, n).random((n, dim))


def gauss(n, dim, factor, nu, tag):
    """exp(-eps^2 r^2) + nu I on uniform random points, eps = factor * 2 * n^(1/dim): a flat Gaussian with a nugget"""
    x = gauss_points(n, dim, tag)
    eps = factor * 2.0 * n ** (1.0 / dim)
    r2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(axis=2)
    return _sym(np.exp(-eps * eps * r2) + nu * np.eye(n))


def zoo(name, n):
    if name.startswith("spec_"):
        return spectrum(n, float(name[5:]))
    if name == "gauss2d_a":
        return gauss(n, 2, 0.25, 1e-8, "g2")
    if name == "gauss2d_b":
        return gauss(n, 2, 0.05, 1e-4, "g2")
    if name == "gauss3d":
        return gauss(n, 3, 0.25, 1e-8, "g3")
    if name == "graded":
        d = np.logspace(0.0, -4.0, n)                  # with 1e-6 the last pivots fall below 16 n eps max a_ii
        return _sym(d[:, None] * spectrum(n, 1e4) * d[None, :])
    if name == "scaled_up":
        return np.ldexp(spectrum(n, 1e4), 900)
    if name == "scaled_down":
        return np.ldexp(spectrum(n, 1e4), -900)
    if name == "semidef_gram":
        g = _rng("gram", n).standard_normal((n, n // 2))
        return _sym(g @ g.T)
    if name == "semidef_gauss":
        return gauss(n, 2, 0.05, 0.0, "g2")
    raise KeyError(name)


def shifted(a):
    """A + 16 n eps max a_ii I: the nearest matrix LAPACK is sure to factor, the yardstick of the semi-definite cases"""
    n = len(a)
    return a + 16.0 * n * EPS * np.diag(a).max() * np.eye(n)


def rhs(a, name, nrhs=5):
    """nrhs right-hand sides b = A x*, x* standard normal, as rows"""
    xs = _rng("rhs_" + name, len(a)).standard_normal((nrhs, len(a)))
    return np.ascontiguousarray((a @ xs.T).T)


# ---------------------------------------------------------------- measures
_BITS, _SLICES = 20, 4


def _slices(m):
    """m = sum_s ints[s] * 2^(e - 20 (s + 1)) row by row, up to 2^-80 of the row's largest entry; ints[s] hold integers of
    at most 2^20, so dot products of up to 2^12 of them are exact in float64"""
    _, e = np.frexp(np.abs(m).max(axis=1))
    e = e.astype(np.int64)
    rem, out = np.array(m, dtype=np.float64), []
    for s in range(_SLICES):
        sh = _BITS * (s + 1) - e
        q = np.round(np.ldexp(rem, sh[:, None]))
        out.append(q)
        rem = rem - np.ldexp(q, -sh[:, None])         # exact
    return out, e


def product_ld(x, y, y_slices=None):
    """x @ y.T in np.longdouble for float64 x, y with at most 4096 columns; error <= 2^-68 of (row max of x)(row max of y).
    y_slices: _slices(y), when the caller multiplies by the same y more than once"""
    assert x.shape[1] == y.shape[1] and x.shape[1] <= 4096
    xs, ex = _slices(x)
    ys, ey = (xs, ex) if y is x else (y_slices or _slices(y))
    ee = (ex[:, None] + ey[None, :]).astype(np.int64)
    acc = np.zeros((len(x), len(y)), dtype=LD)
    for lvl in range(_SLICES - 1, -1, -1):             # smallest terms first
        part = np.zeros((len(x), len(y)), dtype=LD)
        for s in range(lvl + 1):
            t = lvl - s
            if y is x and s > t:
                continue                              # x x^T: the pair (t, s) is the transpose of (s, t)
            p = xs[s] @ ys[t].T                       # integers below 2^53: exact whatever the order of the sum
            part += p
            if y is x and s < t:
                part += p.T
        acc += np.ldexp(part, ee - _BITS * (lvl + 2))
    return acc


def factor_resid(a, l):
    """|A - L L^T| (lower triangle of L is used) in np.longdouble"""
    l = np.tril(l)
    return np.abs(a.astype(LD) - product_ld(l, l))


def factor_be(a, l):
    return float(factor_resid(a, l).max() / np.abs(a).max())


def factor_figures(a, l):
    """(factor_be, componentwise max |A - L L^T| / (|L| |L^T|) in eps) from one residual.  The componentwise figure is
    reported, never asserted, and taken over the entries whose |L| |L^T| is at least 2^-12 of the product of the two
    rows' largest |L|: product_ld is exact to 2^-68 of that product, so only there is a ratio of a few eps resolved
    (the far-apart pairs of a Gaussian matrix, entries like 1e-90, are left out)."""
    r = factor_resid(a, l)
    la = np.abs(np.tril(l))
    e = np.frexp(la.max())[1]
    la = np.ldexp(la, -e)                              # |L| |L^T| in float64 is plenty for a denominator
    den = la @ la.T
    rm = la.max(axis=1)
    keep = den >= 2.0 ** -12 * rm[:, None] * rm[None, :]
    cw = (np.ldexp(r[keep], -2 * e) / den[keep]).max() / EPS
    return float(r.max() / np.abs(a).max()), float(cw)


def norm_inf(a):
    return float(np.abs(a).sum(axis=1).max())


def solve_be(a, x, b):
    """||A x - b||_inf / (||A||_inf ||x||_inf + ||b||_inf), the residual in np.longdouble (a may be given as longdouble)"""
    r = np.abs(a.astype(LD, copy=False) @ np.asarray(x, dtype=LD) - np.asarray(b, dtype=LD)).max()
    return float(r / (LD(norm_inf(a)) * LD(np.abs(x).max()) + LD(np.abs(b).max())))


def resid_inf(a, x, b):
    return np.abs(a.astype(LD, copy=False) @ np.asarray(x, dtype=LD) - np.asarray(b, dtype=LD)).max()


def x_ref(a, b):
    """A^-1 b (b: one right-hand side, or several as rows) to far below float64's reach: LAPACK's Cholesky solution,
    refined with residuals from product_ld (x split into two float64 parts) until the correction of a row stops halving.
    Asserts that the corrections shrank to 2^-8 of the first one, which is LAPACK's own forward error."""
    bb = np.atleast_2d(np.asarray(b, dtype=np.float64))
    c = sla.cho_factor(a, lower=True)
    a_slices = _slices(a)
    x = sla.cho_solve(c, bb.T).T.astype(LD)
    first, last, active = None, np.full(len(bb), np.inf), np.ones(len(bb), dtype=bool)
    for _ in range(40):
        xh = x.astype(np.float64)
        xl = (x - xh).astype(np.float64)
        r = bb.astype(LD) - (product_ld(xh, a, a_slices) + product_ld(xl, a, a_slices))       # A symmetric: (x A)^T = A x
        d = sla.cho_solve(c, r.astype(np.float64).T).T
        size = np.abs(d).max(axis=1) / np.abs(x).max(axis=1).astype(np.float64)
        first = size if first is None else first
        active = active & (size < 0.5 * last)
        if not active.any():
            break
        x[active] += d[active]
        last[active] = size[active]
    assert (last <= 2.0 ** -8 * np.maximum(first, EPS)).all(), ("x_ref did not converge", first, last)
    return x if np.ndim(b) == 2 else x[0]


def forward_err(x, xr):
    return float(np.abs(np.asarray(x, dtype=LD) - xr).max() / np.abs(xr).max())


def lu_be(a, lu, perm):
    """max |A[perm] - L U| / max |A| in np.longdouble"""
    l = np.tril(lu, -1) + np.eye(len(a))
    return float(np.abs(a[perm].astype(LD) - product_ld(l, np.ascontiguousarray(np.triu(lu).T))).max() / np.abs(a).max())


def refine_step(lu_piv, a, x0, b):
    """one step of iterative refinement as LAPACK users write it, all in float64: x0 - (LU)^-1 (A x0 - b) with scipy's
    lu_factor of a.  The yardstick of lu_refine, which forms its residual in float64 too."""
    return x0 - sla.lu_solve(lu_piv, a @ x0 - b)


# ---------------------------------------------------------------- model
NB, TS = 32, 64


def model_cholesky(a):
    """right-looking, 32 wide; the rows below a diagonal block are MULTIPLIED by its forward-substituted inverse"""
    a, n = np.array(a), len(a)
    for j in range(0, n, NB):
        k = min(j + NB, n)
        d = np.linalg.cholesky(a[j:k, j:k])
        a[j:k, j:k] = d
        dinv = sla.solve_triangular(d, np.eye(k - j), lower=True)
        a[k:, j:k] = a[k:, j:k] @ dinv.T
        a[k:, k:] -= a[k:, j:k] @ a[k:, j:k].T
    return np.tril(a)


def model_solve(l, b):
    """L y = b, L^T x = y by 64-wide blocks; the diagonal systems are multiplied by the inverted block once n > 64"""
    n, x = len(l), np.array(b, dtype=np.float64)
    blocks = [(j, min(j + TS, n)) for j in range(0, n, TS)]

    def diag(d, v, trans):
        if n <= TS:
            return sla.solve_triangular(d, v, lower=True, trans=trans)
        w = sla.solve_triangular(d, np.eye(len(d)), lower=True)
        return (w.T if trans else w) @ v
    for j, k in blocks:
        x[j:k] = diag(l[j:k, j:k], x[j:k], 0)
        x[k:] -= l[k:, j:k] @ x[j:k]
    for j, k in reversed(blocks):
        x[j:k] = diag(l[j:k, j:k], x[j:k], 1)
        x[:j] -= l[j:k, :j].T @ x[j:k]
    return x


# ---------------------------------------------------------------- LU inputs
LU_SIZES = [33, 700, 1100]
LU_KINDS = ["svd_1e6", "svd_1e12", "tps", "rowgraded"]


def lu_matrix(kind, n):
    rng = _rng("lu_" + kind, n)
    if kind.startswith("svd_"):
        u, _ = np.linalg.qr(rng.standard_normal((n, n)))
        v, _ = np.linalg.qr(rng.standard_normal((n, n)))
        return (u * float(kind[4:]) ** (-np.arange(n) / (n - 1.0))) @ v.T
    if kind == "tps":
        x = rng.random((n, 2))
        r2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(axis=2)
        return 0.5 * r2 * np.log(np.where(r2 > 0, r2, 1.0))          # r^2 log r, zero diagonal: indefinite
    if kind == "rowgraded":
        return np.logspace(0.0, -8.0, n)[:, None] * rng.standard_normal((n, n))
    raise KeyError(kind)


# ---------------------------------------------------------------- the two consumers of the inverse
def cholesky_ld(k):
    """lower Cholesky factor in np.longdouble (left-looking, one matrix-vector product per column)"""
    l = np.tril(np.asarray(k, dtype=LD))
    for j in range(len(l)):
        l[j:, j] -= l[j:, :j] @ l[j, :j]
        l[j, j] = np.sqrt(l[j, j])
        l[j + 1:, j] /= l[j, j]
    return l


def kriging_formulas(k, kt, f, ld):
    """(variance at the targets, leave-one-out residuals, leave-one-out variances) of ordinary kriging with sill 1 from a
    Cholesky factor of K: kt = the covariances k(x_i, y_j) (n x m, without the nugget), f the responses.
        sigma^2 = 1 - k^T K^-1 k + (1 - b^T k)^2 / (1^T b), b = K^-1 1         (tests/test_gpu_krige_variance.py)
        e = w / d, v = 1 / d, w = K^-1 f - b (1^T K^-1 f) / (1^T b), d = diag(K^-1) - b^2 / (1^T b)   (tests/test_gpu_loo.py)
    ld: in np.longdouble throughout; otherwise float64 with LAPACK's factor and triangular solves"""
    n = len(k)
    r = np.column_stack([kt, np.ones(n), f])
    if ld:
        l = cholesky_ld(k)
        li, y = np.zeros((n, n), dtype=LD), r.astype(LD)
        for j in range(n):
            li[j, :j] = -(l[j, :j] @ li[:j, :j]) / l[j, j]
            li[j, j] = 1 / l[j, j]
            y[j] = (y[j] - l[j, :j] @ y[:j]) / l[j, j]
    else:
        l = np.linalg.cholesky(k)
        li = sla.solve_triangular(l, np.eye(n), lower=True)
        y = sla.solve_triangular(l, r, lower=True)
    yk, y1, yf = y[:, :-2], y[:, -2], y[:, -1]
    g, b, w0 = (li * li).sum(axis=0), li.T @ y1, li.T @ yf
    sb = b.sum()
    var = 1 - (yk * yk).sum(axis=0) + (1 - y1 @ yk) ** 2 / sb
    d = g - b * b / sb
    return var, (w0 - b * (w0.sum() / sb)) / d, 1 / d
