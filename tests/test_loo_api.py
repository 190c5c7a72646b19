"""The leave-one-out entry points where they answer without a GPU: the switch per type, state errors, the workspace size and
the C prototypes."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("kind", ("gaussian", "wendland", "kriging"))
def test_set_loo_toggles_the_flag(pkg, kind):
    s = pkg.Sinterp(kind, 2, 8)
    assert s._p.contents.want_loo == 0                          # the default
    assert s.set_loo(1) == 0 and s._p.contents.want_loo == 1
    assert s.set_loo(0) == 0 and s._p.contents.want_loo == 0
    assert pkg.lib().gsl_sinterp_set_loo(None, 1) == pkg.capi.GSL_EFAULT


@pytest.mark.parametrize("kind", ("tps", "tps_affine", "linear_simplex", "linear_mesh"))
def test_set_loo_is_for_the_positive_definite_types(pkg, kind):
    s = pkg.Sinterp(kind, 2, 8)
    assert s.set_loo(1) == pkg.GSL_EINVAL and s._p.contents.want_loo == 0
    assert s.loo_residuals(out=np.zeros((8, 1)))[0] == pkg.GSL_EINVAL
    assert s.loo_variance()[0] == pkg.GSL_EINVAL


@pytest.mark.parametrize("kind", ("gaussian", "wendland", "kriging"))
def test_accessors_of_an_uninitialised_interpolant(pkg, kind):
    s = pkg.Sinterp(kind, 2, 8)
    assert s.set_loo(1) == 0
    E = np.full((8, 1), 7.0)
    st, _ = s.loo_residuals(out=E)
    assert st == pkg.GSL_EINVAL and (E == 7.0).all()            # nothing written
    st, v = s.loo_variance(out=np.full(8, 7.0))
    assert st == pkg.GSL_EINVAL and (v == 7.0).all()
    L = pkg.lib()
    assert L.gsl_sinterp_loo_residuals(s._p, None) == pkg.capi.GSL_EFAULT
    assert L.gsl_sinterp_loo_variance(None, None) == pkg.capi.GSL_EFAULT


def test_workspace_covers_the_work_matrix(pkg):
    work = pkg.HipContext.chol_inv_diag_work
    r128 = lambda v: (v + 127) // 128 * 128
    for n, chunk in ((1, 1), (100, 65), (129, 128), (700, 256), (16384, 2048)):
        assert work(n, chunk) >= r128(chunk) * r128(n) + n
    assert work(700, 1 << 20) == work(700, 768)                 # a pass never has more rows than n rounded up to 128


def test_raw_entries_reject_a_null_context(pkg):
    L = pkg.lib()
    assert L.gsl_sinterp_hip_chol_inv_diag(None, 8, None, 8, None, None, 128) == pkg.capi.GSL_EFAULT
    assert L.gsl_sinterp_hip_loo_combine(None, 8, 1, None, None, 1.0, None, 8, None, 8, None) == pkg.capi.GSL_EFAULT
    for name in ("chol_inv_diag", "chol_inv_diag_work", "loo_combine"):
        assert callable(getattr(pkg.HipContext, name)), name


def test_c_program_references_the_prototypes(pkg, tmp_path):
    libdir = os.path.dirname(pkg.library_path())
    exe = str(tmp_path / "loo_prototypes")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if os.environ.get("GSL_SINTERP_ASAN") else []
    libname = os.path.basename(pkg.library_path())[3:-3]
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Werror", *san, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "loo_prototypes.c"), "-o", exe,
                           "-L", libdir, "-l" + libname, "-lm", "-Wl,-rpath," + libdir])
    assert "ok" in subprocess.check_output([exe], text=True)
