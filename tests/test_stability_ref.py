"""CPU: the checks that keep the bounds of tests/test_gpu_stability.py honest.  For every positive-definite zoo entry, at
every size the GPU tests use it:
  - LAPACK factors it, and its smallest squared pivot is >= 16 n eps max a_ii (the reference is in control of the input);
  - x_ref converges;
  - the numpy model of the documented algorithm (inverted 32 x 32 blocks in the row solve, inverted 64 x 64 blocks in the
    sweeps) has factor_be and solve_be <= 8 x LAPACK's on the same matrix -- so the GPU bound of 16 x LAPACK is one that
    a correct implementation of this design meets with room to spare.
If an entry fails one of these, the entry changes, not the condition."""
import numpy as np
import pytest
import scipy.linalg as sla

import stability_ref as sr

CASES = [(name, n) for name in sr.PD + ["spec_1e4"] for n in sr.sizes_of(name)]


def test_measures_see_one_ulp():
    """the sliced products are exact: a residual built by hand is returned to the last bit, at every scale"""
    rng = np.random.default_rng(1)
    for scale in (0, 450, -450):
        l = np.ldexp(np.tril(rng.standard_normal((130, 130))), scale)
        exact = sr.product_ld(l, l)
        a = exact.astype(np.float64)                               # L L^T rounded to float64: residual <= half an ulp
        assert sr.factor_be(a, l) <= 0.5 * sr.EPS
        a2 = a.copy()
        a2[7, 3] = np.nextafter(a2[7, 3], np.inf) if a2[7, 3] > 0 else np.nextafter(a2[7, 3], -np.inf)
        got = sr.factor_resid(a2, l)[7, 3]
        want = np.abs(a2[7, 3].astype(sr.LD) - exact[7, 3])
        assert got == want and got >= 0.5 * np.spacing(np.abs(a[7, 3]))
    # against plain longdouble arithmetic on a small product
    x, y = rng.standard_normal((9, 40)), rng.standard_normal((7, 40)) * np.logspace(0, -30, 7)[:, None]
    plain = x.astype(sr.LD) @ y.astype(sr.LD).T
    scale = np.abs(x).max(axis=1)[:, None] * np.abs(y).max(axis=1)[None, :]
    assert (np.abs(sr.product_ld(x, y) - plain) <= 40 * 2.0 ** -62 * scale).all()


@pytest.mark.parametrize("name", sr.PD + sr.SEMIDEF + ["spec_1e4"])
def test_zoo_is_symmetric_and_seeded(name):
    a = sr.zoo(name, 96)
    assert a.dtype == np.float64 and np.array_equal(a, a.T) and np.isfinite(a).all()
    assert np.array_equal(a, sr.zoo(name, 96))
    tiny = np.finfo(np.float64).tiny
    assert np.abs(a[a != 0]).min() >= tiny                          # no subnormal entries, the scaled ones included


@pytest.mark.parametrize("name,n", CASES, ids=["%s-%d" % c for c in CASES])
def test_reference_controls_the_entry_and_model_meets_the_bound(name, n):
    a = sr.zoo(name, n)
    l = np.linalg.cholesky(a)                                       # raises if LAPACK fails
    piv = float((np.diag(l) ** 2).min())
    floor = 16.0 * n * sr.EPS * float(np.diag(a).max())
    b = sr.rhs(a, name, 1)[0]
    xr = sr.x_ref(a, b)                                             # asserts its own convergence
    x_lap = sla.cho_solve((l, True), b)
    lm = sr.model_cholesky(a)
    x_mod = sr.model_solve(lm, b)
    (f_lap, c_lap), (f_mod, c_mod) = sr.factor_figures(a, l), sr.factor_figures(a, lm)
    lam = np.linalg.eigvalsh(a) if n <= 1024 else np.array([np.nan, np.nan])       # printed only
    s_lap, s_mod = sr.solve_be(a, x_lap, b), sr.solve_be(a, x_mod, b)
    print(f"{name} n {n}: cond {lam[-1] / lam[0]:.2e}, min pivot^2 / floor {piv / floor:.2e}; factor_be LAPACK {f_lap / sr.EPS:.2f} eps, "
          f"model {f_mod / sr.EPS:.2f} eps (x{f_mod / f_lap:.2f}); solve_be LAPACK {s_lap / sr.EPS:.3f} eps, model {s_mod / sr.EPS:.3f} eps "
          f"(x{s_mod / s_lap:.2f}); forward LAPACK {sr.forward_err(x_lap, xr):.2e}, model {sr.forward_err(x_mod, xr):.2e}; "
          f"componentwise LAPACK {c_lap:.1f} eps, model {c_mod:.1f} eps")
    assert piv >= floor
    assert np.isfinite(lm).all()
    assert f_mod <= 8.0 * f_lap
    assert s_mod <= 8.0 * s_lap


@pytest.mark.parametrize("name", sr.SEMIDEF)
@pytest.mark.parametrize("n", sr.SIZES[:-1])
def test_semidefinite_entries_have_a_controlled_neighbour(name, n):
    """the semi-definite entries are what they claim (smallest eigenvalue within rounding of 0), and the shifted
    matrix that sets their bound is one LAPACK factors with pivots above the floor"""
    a = sr.zoo(name, n)
    lam = np.linalg.eigvalsh(a)
    assert lam[0] <= 4.0 * n * sr.EPS * lam[-1]
    s = sr.shifted(a)
    l = np.linalg.cholesky(s)
    assert np.isfinite(l).all() and sr.factor_be(s, l) <= 8.0 * n * sr.EPS


@pytest.mark.parametrize("kind", sr.LU_KINDS)
@pytest.mark.parametrize("n", sr.LU_SIZES)
def test_lu_reference(kind, n):
    """scipy's LU of the LU inputs: finite, |L| <= 1, and lu_be agrees with a plain longdouble residual"""
    a = sr.lu_matrix(kind, n)
    lu, piv = sla.lu_factor(a)
    perm = np.arange(n)
    for i, p in enumerate(piv):
        perm[[i, p]] = perm[[p, i]]
    assert np.isfinite(lu).all() and np.abs(np.tril(lu, -1)).max() <= 1.0
    be = sr.lu_be(a, lu, perm)
    print(f"{kind} n {n}: cond {np.linalg.cond(a):.2e}, lu_be {be / sr.EPS:.2f} eps")
    assert be <= n * sr.EPS
    if n == 33:
        ld = sr.LD
        plain = np.abs(a[perm].astype(ld) - (np.tril(lu, -1) + np.eye(n)).astype(ld) @ np.triu(lu).astype(ld)).max() / np.abs(a).max()
        assert abs(be - float(plain)) <= 2.0 ** -60
