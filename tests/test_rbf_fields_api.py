"""The fields entry points (several responses on one set of centres) where they answer without a GPU: the symbols, state,
type, shape and NULL-argument errors, and the C prototypes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RBF_TYPES = ("gaussian", "tps", "tps_affine", "wendland", "kriging")
NEW_SYMBOLS = ("gsl_sinterp_init_fields", "gsl_sinterp_n_fields", "gsl_sinterp_eval_fields_e", "gsl_sinterp_eval_fields_many",
               "gsl_sinterp_eval_fields_resident", "gsl_sinterp_get_field_weights", "gsl_sinterp_field_mean", "gsl_sinterp_field_poly",
               "gsl_sinterp_hip_rbf_eval_fields", "gsl_sinterp_hip_rbf_fields_block", "gsl_sinterp_hip_rbf_fields_block_small", "gsl_sinterp_hip_rbf_solve_fields",
               "gsl_sinterp_hip_krige_solve_fields")


def fake_device_pointer():
    """a non-NULL address for arguments that the entry must reject before it looks at them"""
    return C.addressof(C.create_string_buffer(64))


def test_symbols_and_methods_exist(pkg):
    L = pkg.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in pkg.capi.SIGNATURES, name
    for name in ("init_fields", "n_fields", "eval_fields_e", "eval_fields_many", "eval_fields_resident", "field_weights", "field_mean",
                 "field_poly"):
        assert callable(getattr(pkg.Sinterp, name)), name
    for name in ("rbf_eval_fields", "rbf_solve_fields", "krige_solve_fields", "rbf_fields_block"):
        assert callable(getattr(pkg.HipContext, name)), name
    assert 1 <= pkg.HipContext.rbf_fields_block_small() <= pkg.HipContext.rbf_fields_block() <= 64


@pytest.mark.parametrize("kind", RBF_TYPES)
@pytest.mark.parametrize("dim", (1, 2, 3))
def test_uninitialised_interpolant(pkg, kind, dim):
    s = pkg.Sinterp(kind, dim, 8)
    assert s.n_fields() == 0
    y = np.zeros((5, dim))
    assert s.eval_fields_many(y, out=np.zeros((5, 3)))[0] == pkg.GSL_EINVAL
    st, val = s.eval_fields_e(y[0])
    assert st == pkg.GSL_EINVAL and np.isnan(val).all()
    p = fake_device_pointer()
    assert s.eval_fields_resident(p, 5, dim, p, 3) == pkg.GSL_EINVAL
    assert s.eval_fields_resident(None, 0, dim, None, 3) == pkg.GSL_EINVAL
    assert s.field_weights(0)[0] == pkg.GSL_EINVAL
    assert s.field_mean(0)[0] == pkg.GSL_EINVAL
    assert s.field_poly(0)[0] == pkg.GSL_EINVAL


@pytest.mark.parametrize("kind", ("linear_simplex", "linear_mesh"))
def test_linear_types_are_unsupported(pkg, kind):
    s = pkg.Sinterp(kind, 2, 8)
    y = np.zeros((5, 2))
    assert s.n_fields() == 0
    assert s.init_fields(np.zeros((8, 2)), np.zeros((8, 3))) == pkg.GSL_EUNSUP
    assert s.eval_fields_many(y, out=np.zeros((5, 3)))[0] == pkg.GSL_EUNSUP
    st, val = s.eval_fields_e(y[0])
    assert st == pkg.GSL_EUNSUP and np.isnan(val).all()
    p = fake_device_pointer()
    assert s.eval_fields_resident(p, 5, 2, p, 3) == pkg.GSL_EUNSUP
    assert s.field_weights(0)[0] == pkg.GSL_EUNSUP
    assert s.field_mean(0)[0] == pkg.GSL_EUNSUP
    assert s.field_poly(0)[0] == pkg.GSL_EUNSUP


def test_wrong_shapes(pkg):
    cap = pkg.capi
    s = pkg.Sinterp("gaussian", 2, 8)
    x = np.zeros((8, 2))
    assert s.init_fields(x, np.zeros((7, 3))) == cap.GSL_EBADLEN         # F->size1 != size
    assert s.init_fields(np.zeros((8, 3)), np.zeros((8, 3))) == cap.GSL_EBADLEN
    assert s.init_fields(np.zeros((7, 2)), np.zeros((8, 3))) == cap.GSL_EBADLEN
    assert s.init_fields(x, np.zeros((8, 0))) == cap.GSL_EINVAL          # K = 0
    assert s.init_fields(x, np.zeros((8, 65))) == cap.GSL_EINVAL         # K > GSL_SINTERP_MAX_FIELDS
    y = np.zeros((5, 2))
    assert s.eval_fields_many(y, out=np.zeros((5, 3)))[0] == cap.GSL_EINVAL      # right shapes: only the state is wrong
    assert s.eval_fields_many(np.zeros((5, 3)), out=np.zeros((5, 3)))[0] == cap.GSL_EBADLEN   # y->size2 != dim
    assert s.eval_fields_many(y, out=np.zeros((4, 3)))[0] == cap.GSL_EBADLEN     # S->size1 != m
    L = pkg.lib()
    sv = np.zeros(3)
    assert L.gsl_sinterp_eval_fields_e(s._p, C.byref(cap.as_vector(np.zeros(3))), C.byref(cap.as_vector(sv))) == cap.GSL_EBADLEN
    assert np.isnan(sv).all()


def test_null_arguments(pkg):
    L, cap = pkg.lib(), pkg.capi
    s = pkg.Sinterp("tps", 2, 8)
    x, F = cap.as_matrix(np.zeros((8, 2))), cap.as_matrix(np.zeros((8, 3)))
    y, S, yv, sv, out = cap.as_matrix(np.zeros((5, 2))), cap.as_matrix(np.zeros((5, 3))), cap.as_vector(np.zeros(2)), cap.as_vector(np.zeros(3)), C.c_double(0)
    assert L.gsl_sinterp_init_fields(None, C.byref(x), C.byref(F)) == cap.GSL_EFAULT
    assert L.gsl_sinterp_init_fields(s._p, None, C.byref(F)) == cap.GSL_EFAULT
    assert L.gsl_sinterp_init_fields(s._p, C.byref(x), None) == cap.GSL_EFAULT
    assert L.gsl_sinterp_n_fields(None) == 0
    assert L.gsl_sinterp_eval_fields_many(None, C.byref(y), C.byref(S)) == cap.GSL_EFAULT
    assert L.gsl_sinterp_eval_fields_many(s._p, None, C.byref(S)) == cap.GSL_EFAULT
    assert L.gsl_sinterp_eval_fields_many(s._p, C.byref(y), None) == cap.GSL_EFAULT
    assert L.gsl_sinterp_eval_fields_e(None, C.byref(yv), C.byref(sv)) == cap.GSL_EFAULT
    assert L.gsl_sinterp_eval_fields_e(s._p, None, C.byref(sv)) == cap.GSL_EFAULT
    assert L.gsl_sinterp_eval_fields_e(s._p, C.byref(yv), None) == cap.GSL_EFAULT
    p = fake_device_pointer()
    assert L.gsl_sinterp_eval_fields_resident(None, p, 5, 2, p, 3) == cap.GSL_EFAULT
    assert s.eval_fields_resident(None, 5, 2, p, 3) == cap.GSL_EFAULT
    assert s.eval_fields_resident(p, 5, 2, None, 3) == cap.GSL_EFAULT
    assert L.gsl_sinterp_get_field_weights(None, 0, C.byref(sv)) == cap.GSL_EFAULT
    assert L.gsl_sinterp_get_field_weights(s._p, 0, None) == cap.GSL_EFAULT
    assert L.gsl_sinterp_field_mean(s._p, 0, None) == cap.GSL_EFAULT
    assert L.gsl_sinterp_field_mean(None, 0, C.byref(out)) == cap.GSL_EFAULT
    assert L.gsl_sinterp_field_poly(s._p, 0, None) == cap.GSL_EFAULT
    assert L.gsl_sinterp_hip_rbf_eval_fields(None, 0, 1.0, None, p, 8, 2, 2, p, 8, 3, p, 5, 2, p, 3, 0) == cap.GSL_EFAULT
    assert L.gsl_sinterp_hip_rbf_solve_fields(None, 0, 1.0, p, 8, 2, 2, p, 8, p, 8, 3, None) == cap.GSL_EFAULT
    assert L.gsl_sinterp_hip_krige_solve_fields(None, 0, 1.0, 0.0, p, 8, 2, 2, p, 8, p, 8, 3, C.byref(out), None) == cap.GSL_EFAULT


def test_c_program_references_the_prototypes(pkg, tmp_path):
    libdir = os.path.dirname(pkg.library_path())
    exe = str(tmp_path / "rbf_fields_prototypes")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if os.environ.get("GSL_SINTERP_ASAN") else []
    libname = os.path.basename(pkg.library_path())[3:-3]
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Werror", *san, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "rbf_fields_prototypes.c"), "-o", exe,
                           "-L", libdir, "-l" + libname, "-lm", "-Wl,-rpath," + libdir])
    assert "ok" in subprocess.check_output([exe], text=True)
