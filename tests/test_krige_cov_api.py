"""The joint-covariance and simulation entries (gsl_sinterp_eval_covariance_*, gsl_sinterp_simulate_*) where they answer
without a GPU: the symbols, every refusal that needs no initialised model with one call to the error handler each, the
`neighbours > 0` refusal, the work-size functions, the C prototypes, and the numpy reference of tests/krige_cov_ref.py
against itself (its two routes, its diagonal against the variance formula, the simulation identity)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import krige_cov_ref as kc
import ukrige_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KRIGING = ("kriging", "kriging_matern32", "kriging_matern52")
NEW_SYMBOLS = ("gsl_sinterp_eval_covariance_many", "gsl_sinterp_eval_covariance_resident", "gsl_sinterp_simulate_many",
               "gsl_sinterp_simulate_resident", "gsl_sinterp_hip_krige_covariance_work", "gsl_sinterp_hip_krige_covariance",
               "gsl_sinterp_hip_krige_simulate_work", "gsl_sinterp_hip_krige_simulate")


def fake_device_pointer():
    """a non-NULL address for arguments that the entry must reject before it looks at them"""
    return C.addressof(C.create_string_buffer(64))


def one_call(pkg, fn, status):
    """fn() answers `status` and calls the handler exactly once with it"""
    with pkg.capi.ErrorCalls() as calls:
        r = fn()
    st = int(r[0] if isinstance(r, tuple) else r)
    assert st == status and [c[1] for c in calls] == [status], (st, calls)
    return r


def entries(pkg, s, dim=2, m=5, S=3):
    """the four facade entries on well-shaped host arguments / non-NULL fake device pointers"""
    y, zn, p = np.zeros((m, dim)), np.zeros((m, S)), fake_device_pointer()
    return (lambda: s.eval_covariance_many(y), lambda: s.eval_covariance_many(y[:2], y),
            lambda: s.eval_covariance_resident(p, m, dim, None, 0, 0, p, m), lambda: s.simulate_many(y, 1.0, 0.0, zn),
            lambda: s.simulate_resident(p, m, dim, 1.0, 0.0, p, S, S, p, S))


def test_symbols_and_methods_exist(pkg):
    L = pkg.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in pkg.capi.SIGNATURES, name
    for name in ("eval_covariance_many", "eval_covariance_resident", "simulate_many", "simulate_resident"):
        assert callable(getattr(pkg.Sinterp, name)), name
    for name in ("krige_covariance", "krige_covariance_work", "krige_simulate", "krige_simulate_work"):
        assert callable(getattr(pkg.HipContext, name)), name


def test_state_refusals_are_those_of_the_variance_entries(pkg):
    """same status and same reason as eval_variance_many on the same interpolant, one handler call each"""
    y = np.zeros((5, 2))
    for kind in pkg.Sinterp.TYPES:
        s = pkg.Sinterp(kind, 2, 10)
        with pkg.capi.ErrorCalls() as want:
            st = s.eval_variance_many(y)[0]
        assert st != 0 and len(want) == 1
        if kind in KRIGING:
            assert st == pkg.GSL_EINVAL                                # not initialised
        for fn in entries(pkg, s):
            with pkg.capi.ErrorCalls() as calls:
                got = fn()
            got = int(got[0] if isinstance(got, tuple) else got)
            assert got == st and list(calls) == list(want), (kind, got, calls, want)
        s.close()


@pytest.mark.parametrize("kind", KRIGING)
def test_neighbours_refuse_before_the_device(pkg, kind):
    s = pkg.Sinterp(kind, 2, 50)
    assert s.set_variance(1) == 0 and s.set_neighbours(8) == 0
    for fn in entries(pkg, s):
        one_call(pkg, fn, pkg.capi.GSL_EUNSUP)
    assert s.set_neighbours(0) == 0
    for fn in entries(pkg, s):
        one_call(pkg, fn, pkg.GSL_EINVAL)                              # back to "not initialised"


def test_null_arguments_and_shapes(pkg):
    L, cap = pkg.lib(), pkg.capi
    EFAULT, EBADLEN = cap.GSL_EFAULT, cap.GSL_EBADLEN
    s = pkg.Sinterp("kriging", 2, 10)
    M = lambda a: C.byref(cap.as_matrix(a))
    y, y3, cov, zn, out = np.zeros((5, 2)), np.zeros((5, 3)), np.zeros((5, 5)), np.zeros((5, 3)), np.zeros((5, 3))
    p = fake_device_pointer()
    one_call(pkg, lambda: L.gsl_sinterp_eval_covariance_many(None, M(y), None, M(cov)), EFAULT)
    one_call(pkg, lambda: L.gsl_sinterp_eval_covariance_many(s._p, None, None, M(cov)), EFAULT)
    one_call(pkg, lambda: L.gsl_sinterp_eval_covariance_many(s._p, M(y), None, None), EFAULT)
    one_call(pkg, lambda: L.gsl_sinterp_eval_covariance_resident(None, p, 5, 2, None, 0, 0, p, 5), EFAULT)
    one_call(pkg, lambda: L.gsl_sinterp_simulate_many(None, M(y), 1.0, 0.0, M(zn), M(out)), EFAULT)
    one_call(pkg, lambda: L.gsl_sinterp_simulate_many(s._p, None, 1.0, 0.0, M(zn), M(out)), EFAULT)
    one_call(pkg, lambda: L.gsl_sinterp_simulate_many(s._p, M(y), 1.0, 0.0, None, M(out)), EFAULT)
    one_call(pkg, lambda: L.gsl_sinterp_simulate_many(s._p, M(y), 1.0, 0.0, M(zn), None), EFAULT)
    one_call(pkg, lambda: L.gsl_sinterp_simulate_resident(None, p, 5, 2, 1.0, 0.0, p, 3, 3, p, 3), EFAULT)
    # shapes: decided before the state is looked at, as in eval_variance_many
    one_call(pkg, lambda: s.eval_covariance_many(y3), EBADLEN)                          # ya without dim columns
    one_call(pkg, lambda: s.eval_covariance_many(y, y3), EBADLEN)                       # yb without dim columns
    one_call(pkg, lambda: s.eval_covariance_many(y, out=np.zeros((5, 4))), EBADLEN)     # Cov not ma x ma
    one_call(pkg, lambda: s.eval_covariance_many(y[:2], y, out=np.zeros((5, 2))), EBADLEN)   # Cov not ma x mb
    one_call(pkg, lambda: s.simulate_many(y3, 1.0, 0.0, zn), EBADLEN)
    one_call(pkg, lambda: s.simulate_many(y, 1.0, 0.0, zn[:4]), EBADLEN)                # Zn not m x S
    one_call(pkg, lambda: s.simulate_many(y, 1.0, 0.0, zn, out=np.zeros((5, 2))), EBADLEN)
    one_call(pkg, lambda: s.simulate_many(y, 1.0, 0.0, np.zeros((5, 0)), out=np.zeros((5, 0))), EBADLEN)     # S >= 1


def test_raw_entries_and_work_sizes(pkg):
    L, EFAULT = pkg.lib(), pkg.capi.GSL_EFAULT
    H = pkg.HipContext
    assert L.gsl_sinterp_hip_krige_covariance(None, 0, 1.0, 0, None, None, None, 8, 2, 2, None, 8, None, 8, None, None, None, 4, 2, None, 0, 0,
                                              None, 4, None) == EFAULT
    assert L.gsl_sinterp_hip_krige_simulate(None, 0, 1.0, 0, None, None, None, 8, 2, 2, None, 8, None, 8, None, None, None, 4, 2, None, 1.0, 0.0,
                                            None, 1, 1, None, 1, None) == EFAULT
    up = lambda v, to: (v + to - 1) // to * to
    for n, ma, mb, q in ((700, 65, 130, 3), (129, 1, 0, 1), (384, 130, 3, 6), (100, 200, 200, 10), (1200, 85, 0, 4)):
        rows = up(ma, 128) + (up(mb, 128) if mb else 0)
        work = H.krige_covariance_work(n, ma, mb, q)
        assert work >= rows * n + rows + (ma + mb) * q, (n, ma, mb, q)       # (ma_pad + mb_pad) N, the row norms, T
        assert work >= rows * up(n, 128)                                      # ... at the pitch the substitution takes
        assert work <= rows * (up(n, 128) + 1) + (ma + mb) * q + 16           # and nothing of another order
        assert H.krige_simulate_work(n, ma, 16, q) >= H.krige_covariance_work(n, ma, 0, q) + ma * ma + 16 * ma


def test_c_program_references_the_prototypes(pkg, tmp_path):
    libdir = os.path.dirname(pkg.library_path())
    exe = str(tmp_path / "krige_cov_prototypes")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if os.environ.get("GSL_SINTERP_ASAN") else []
    libname = os.path.basename(pkg.library_path())[3:-3]
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Werror", *san, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "krige_cov_prototypes.c"), "-o", exe,
                           "-L", libdir, "-l" + libname, "-lm", "-Wl,-rpath," + libdir])
    assert "ok" in subprocess.check_output([exe], text=True)


# ---- the reference against itself, on one shape: the figures every GPU test leans on ----
def test_reference_self_checks(orc):
    kind, dim, n, m, nugget, order = ref.MATERN52, 2, 300, 65, 0.0, 1
    x = orc.synth_centres(n, dim)
    f = orc.synth_response(x) + 3.0
    y = np.ascontiguousarray(np.vstack([orc.synth_targets(0, m, dim), x[:20]]))
    eps = ref.default_eps(kind, n, dim)
    M = kc.CovModel(kind, eps, nugget, order, x, f)
    e, d = M.check(y)                                                 # the two routes, the diagonal: asserts REF_TOL
    ex, _ = M.check(y[:3], y)
    U = ref.Model(kind, eps, nugget, order, x, f)
    dv = np.abs(np.diag(M.covariance(y)) - U.variance(y)).max()      # ... and against the reference the variance tests use
    vv = np.abs(M.values(y) - U.values(y)[:, 0]).max() / np.abs(f).max()
    print(f"routes {e:.2e} (cross {ex:.2e}), diagonal against variance {d:.2e}, against ukrige_ref {dv:.2e}, values {vv:.2e}")
    assert dv < kc.REF_TOL and vv < kc.REF_TOL
    S = M.covariance(y)
    assert np.abs(S - S.T).max() < kc.REF_TOL
    assert np.abs(M.covariance(y[:3], y) - S[:3]).max() < kc.REF_TOL and np.abs(M.covariance(y, y[:3]) - S[:, :3]).max() < kc.REF_TOL
    assert np.abs(S[-20:, :]).max() < kc.REF_TOL                      # nugget 0: the field is known at the data sites
    # ordinary kriging is the case q = 1 of the same formulas
    O = kc.CovModel(ref.GAUSSIAN, ref.default_eps(ref.GAUSSIAN, n, dim), 1e-3, 0, x, f)
    O.check(y)
    k = O.cross(y)
    b = np.linalg.solve(O.K, np.ones(n))
    want = 1.0 - (k * np.linalg.solve(O.K, k)).sum(axis=0) + (1.0 - b @ k) ** 2 / b.sum()
    assert np.abs(np.diag(O.covariance(y)) - want).max() < kc.REF_TOL
    # a draw: zeros return the mean; A A^T = Sigma; value i depends on the normals 0 .. i only
    T = M.covariance(y[:m])
    zn = np.column_stack([np.zeros(m), np.linspace(-1.0, 1.0, m)])
    out = M.simulate(y[:m], 2.5, 0.0, zn, cov=T)
    assert np.array_equal(out[:, 0], M.values(y[:m]))
    A = (M.simulate(y[:m], 2.5, 0.0, np.eye(m), cov=T) - M.values(y[:m])[:, None]) / np.sqrt(2.5)
    assert np.abs(np.triu(A, 1)).max() == 0.0 and np.abs(A @ A.T - T).max() < kc.REF_TOL
