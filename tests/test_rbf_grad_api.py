"""The value + gradient entry points where they answer without a GPU: state, type, shape and NULL-argument errors, and
the C prototypes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RBF_TYPES = ("gaussian", "tps", "tps_affine", "wendland", "kriging")


def fake_device_pointer():
    """a non-NULL address for arguments that the entry must reject before it looks at them"""
    return C.addressof(C.create_string_buffer(64))


@pytest.mark.parametrize("kind", RBF_TYPES)
@pytest.mark.parametrize("dim", (1, 2, 3))
def test_uninitialised_interpolant(pkg, kind, dim):
    s = pkg.Sinterp(kind, dim, 8)
    y = np.zeros((5, dim))
    st, val, g = s.eval_grad_many(y)
    assert st == pkg.GSL_EINVAL
    assert s.eval_grad_many(y, want_value=False)[0] == pkg.GSL_EINVAL
    st, val, g = s.eval_grad_e(y[0])
    assert st == pkg.GSL_EINVAL and val != val and g.shape == (dim,) and np.isnan(g).all()
    p = fake_device_pointer()
    assert s.eval_grad_resident(p, 5, dim, p, p, dim) == pkg.GSL_EINVAL
    assert s.eval_grad_resident(p, 5, dim, None, p, dim) == pkg.GSL_EINVAL
    assert s.eval_grad_resident(None, 0, dim, None, None, dim) == pkg.GSL_EINVAL


@pytest.mark.parametrize("kind", ("linear_simplex", "linear_mesh"))
def test_linear_types_are_unsupported(pkg, kind):
    s = pkg.Sinterp(kind, 2, 8)
    y = np.zeros((5, 2))
    assert s.eval_grad_many(y)[0] == pkg.GSL_EUNSUP
    st, val, g = s.eval_grad_e(y[0])
    assert st == pkg.GSL_EUNSUP and val != val and np.isnan(g).all()
    p = fake_device_pointer()
    assert s.eval_grad_resident(p, 5, 2, p, p, 2) == pkg.GSL_EUNSUP


def test_wrong_shapes(pkg):
    L, cap = pkg.lib(), pkg.capi
    s = pkg.Sinterp("gaussian", 2, 8)
    many = lambda y, sv, g: L.gsl_sinterp_eval_grad_many(s._p, C.byref(cap.as_matrix(y)), C.byref(cap.as_vector(sv)) if sv is not None else None,
                                                         C.byref(cap.as_matrix(g)))
    y, sv, g = np.zeros((5, 2)), np.zeros(5), np.zeros((5, 2))
    assert many(y, sv, g) == pkg.GSL_EINVAL                          # right shapes: only the state is wrong
    assert many(np.zeros((5, 3)), sv, np.zeros((5, 3))) == cap.GSL_EBADLEN     # y->size2 != dim
    assert many(y, sv, np.zeros((4, 2))) == cap.GSL_EBADLEN          # g->size1 != m
    assert many(y, sv, np.zeros((5, 3))) == cap.GSL_EBADLEN          # g->size2 != dim
    assert many(y, np.zeros(6), g) == cap.GSL_EBADLEN                # s->size != m
    assert many(y, None, np.zeros((6, 2))) == cap.GSL_EBADLEN
    one = lambda yv, gv: L.gsl_sinterp_eval_grad_e(s._p, C.byref(cap.as_vector(yv)), C.byref(C.c_double(0)), C.byref(cap.as_vector(gv)))
    assert one(np.zeros(3), np.zeros(2)) == cap.GSL_EBADLEN
    gv = np.zeros(3)
    assert one(np.zeros(2), gv) == cap.GSL_EBADLEN and np.isnan(gv).all()


def test_null_arguments(pkg):
    L, cap = pkg.lib(), pkg.capi
    s = pkg.Sinterp("tps", 2, 8)
    y, g, yv, gv, out = cap.as_matrix(np.zeros((5, 2))), cap.as_matrix(np.zeros((5, 2))), cap.as_vector(np.zeros(2)), cap.as_vector(np.zeros(2)), C.c_double(0)
    assert L.gsl_sinterp_eval_grad_many(None, C.byref(y), None, C.byref(g)) == cap.GSL_EFAULT
    assert L.gsl_sinterp_eval_grad_many(s._p, None, None, C.byref(g)) == cap.GSL_EFAULT
    assert L.gsl_sinterp_eval_grad_many(s._p, C.byref(y), None, None) == cap.GSL_EFAULT
    assert L.gsl_sinterp_eval_grad_e(None, C.byref(yv), C.byref(out), C.byref(gv)) == cap.GSL_EFAULT
    assert L.gsl_sinterp_eval_grad_e(s._p, None, C.byref(out), C.byref(gv)) == cap.GSL_EFAULT
    assert L.gsl_sinterp_eval_grad_e(s._p, C.byref(yv), None, C.byref(gv)) == cap.GSL_EFAULT
    assert L.gsl_sinterp_eval_grad_e(s._p, C.byref(yv), C.byref(out), None) == cap.GSL_EFAULT
    p = fake_device_pointer()
    assert L.gsl_sinterp_eval_grad_resident(None, p, 5, 2, p, p, 2) == cap.GSL_EFAULT
    assert s.eval_grad_resident(None, 5, 2, p, p, 2) == cap.GSL_EFAULT
    assert s.eval_grad_resident(p, 5, 2, p, None, 2) == cap.GSL_EFAULT
    assert L.gsl_sinterp_hip_rbf_eval_grad(None, 0, 1.0, None, p, 8, 2, 2, p, p, 5, 2, p, p, 2, 0) == cap.GSL_EFAULT


def test_c_program_references_the_prototypes(pkg, tmp_path):
    libdir = os.path.dirname(pkg.library_path())
    exe = str(tmp_path / "rbf_grad_prototypes")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if os.environ.get("GSL_SINTERP_ASAN") else []
    libname = os.path.basename(pkg.library_path())[3:-3]
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Werror", *san, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "rbf_grad_prototypes.c"), "-o", exe,
                           "-L", libdir, "-l" + libname, "-lm", "-Wl,-rpath," + libdir])
    assert "ok" in subprocess.check_output([exe], text=True)
