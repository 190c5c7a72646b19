"""The model-selection entry points where they answer without a GPU: the types fit_alloc accepts, its argument errors (the
status of an entry that returns a pointer arrives through the GSL error handler), the search settings, the raw reduction's
NULL context, the bindings and the C prototypes."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PD_KINDS = ("gaussian", "wendland", "matern32", "matern52", "imq", "kriging", "kriging_matern32", "kriging_matern52")


def alloc_status(pkg, interp, x, f):
    """status with which gsl_sinterp_fit_alloc refuses (it must refuse: none of these calls may reach a device)"""
    with pytest.raises(pkg.capi.GslError) as err:
        pkg.SinterpFit(interp, x, f)
    return err.value.status


@pytest.mark.parametrize("kind", ("tps", "tps_affine", "linear_simplex", "linear_mesh"))
def test_fit_alloc_is_for_the_positive_definite_types(pkg, kind):
    s = pkg.Sinterp(kind, 2, 8)
    assert alloc_status(pkg, s, np.zeros((8, 2)), np.zeros(8)) == pkg.GSL_EINVAL
    with pytest.raises(pkg.capi.GslError):
        s.fit_workspace(np.zeros((8, 2)), np.zeros(8))


@pytest.mark.parametrize("kind", PD_KINDS)
def test_fit_alloc_argument_errors(pkg, kind):
    s = pkg.Sinterp(kind, 2, 8)
    x, f = np.zeros((8, 2)), np.zeros(8)
    assert alloc_status(pkg, s, np.zeros((8, 3)), f) == pkg.capi.GSL_EBADLEN
    assert alloc_status(pkg, s, np.zeros((7, 2)), f) == pkg.capi.GSL_EBADLEN
    assert alloc_status(pkg, s, x, np.zeros(9)) == pkg.capi.GSL_EBADLEN
    assert alloc_status(pkg, s, None, f) == pkg.capi.GSL_EFAULT
    assert alloc_status(pkg, s, x, None) == pkg.capi.GSL_EFAULT
    assert alloc_status(pkg, None, x, f) == pkg.capi.GSL_EFAULT
    assert s._p.contents.shape == 0.0 and s.n_fields() == 0      # the interpolant is not touched


def test_the_handler_is_restored_after_fit_alloc(pkg):
    with pkg.capi.ErrorCalls() as outer:
        alloc_status(pkg, pkg.Sinterp("tps", 2, 8), np.zeros((8, 2)), np.zeros(8))
        assert outer == []                                       # the inner recorder took the call ...
        assert pkg.lib().gsl_sinterp_set_loo(None, 1) == pkg.capi.GSL_EFAULT
        assert [c[1] for c in outer] == [pkg.capi.GSL_EFAULT]    # ... and handed the handler back


def test_search_settings_and_null_workspaces(pkg):
    L = pkg.lib()
    EINVAL, EFAULT = pkg.GSL_EINVAL, pkg.capi.GSL_EFAULT
    # the numbers are judged before the workspace pointer
    assert L.gsl_sinterp_fit_set_search(None, 2, 1e-2, 40) == EINVAL
    assert L.gsl_sinterp_fit_set_search(None, 9, 0.0, 40) == EINVAL
    assert L.gsl_sinterp_fit_set_search(None, 9, -1e-2, 40) == EINVAL
    assert L.gsl_sinterp_fit_set_search(None, 9, float("nan"), 40) == EINVAL
    assert L.gsl_sinterp_fit_set_search(None, 9, 1e-2, 8) == EINVAL
    assert L.gsl_sinterp_fit_set_search(None, 9, 1e-2, 40) == EFAULT
    import ctypes as C
    v, p = C.c_double(0), C.c_double(0)
    assert L.gsl_sinterp_fit_score(None, pkg.FIT_ML, 1.0, 0.0, C.byref(v)) == EFAULT and np.isnan(v.value)
    assert L.gsl_sinterp_fit_shape(None, pkg.FIT_ML, 0.0, 1.0, 2.0, C.byref(p), C.byref(v)) == EFAULT and np.isnan(p.value)
    assert L.gsl_sinterp_fit_nugget(None, pkg.FIT_LOO, 1.0, 1e-4, 1.0, C.byref(p), C.byref(v)) == EFAULT
    assert L.gsl_sinterp_fit_n_eval(None) == 0
    assert L.gsl_sinterp_fit_trace(None, None, None) == EFAULT
    assert L.gsl_sinterp_fit_sigma2(None, C.byref(v)) == EFAULT
    L.gsl_sinterp_fit_free(None)                                 # a no-op


def test_raw_reduction_rejects_a_null_context(pkg):
    assert pkg.lib().gsl_sinterp_hip_score_reduce(None, 8, None, 8, None, None, None, None, 1.0, None) == pkg.capi.GSL_EFAULT
    assert callable(pkg.HipContext.score_reduce)


def test_bindings_exist(pkg):
    assert pkg.FIT_LOO == 0 and pkg.FIT_ML == 1 and pkg.SinterpFit.LOO == 0 and pkg.SinterpFit.ML == 1
    for name in ("score", "fit_shape", "fit_nugget", "set_search", "n_eval", "trace", "sigma2", "close"):
        assert callable(getattr(pkg.SinterpFit, name)), name
    assert callable(pkg.Sinterp.fit_workspace)
    for name in ("alloc", "free", "score", "shape", "nugget", "set_search", "n_eval", "trace", "sigma2"):
        assert "gsl_sinterp_fit_" + name in pkg.capi.SIGNATURES and hasattr(pkg.lib(), "gsl_sinterp_fit_" + name)


def test_c_program_references_the_prototypes(pkg, tmp_path):
    libdir = os.path.dirname(pkg.library_path())
    exe = str(tmp_path / "fit_prototypes")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if os.environ.get("GSL_SINTERP_ASAN") else []
    libname = os.path.basename(pkg.library_path())[3:-3]
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Werror", *san, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "fit_prototypes.c"), "-o", exe,
                           "-L", libdir, "-l" + libname, "-lm", "-Wl,-rpath," + libdir])
    assert "ok" in subprocess.check_output([exe], text=True)
