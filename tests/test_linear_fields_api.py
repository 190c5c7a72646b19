"""The linear fields entries (K responses and per-simplex gradients of the piecewise-linear types) where they answer
without a GPU: the symbols, the refusals of every type on never-initialised interpolants -- status and a single call to the
error handler each, before any device work -- and the C prototypes.  Nothing tests/test_facade_status_matrix.py pins is
asserted again.  GPU part: tests/test_gpu_linear_fields.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINEAR = ("linear_simplex", "linear_mesh")
NEW_SYMBOLS = ("gsl_sinterp_linear_init_fields", "gsl_sinterp_linear_eval_fields_e", "gsl_sinterp_linear_eval_fields_many",
               "gsl_sinterp_linear_eval_fields_resident", "simplex_tree_device_set_responses", "simplex_tree_device_n_responses",
               "simplex_tree_device_eval_fields_many", "simplex_tree_device_eval_fields_resident", "simplex_mesh_device_set_responses",
               "simplex_mesh_device_n_responses", "simplex_mesh_device_eval_fields_many", "simplex_mesh_device_eval_fields_resident",
               "gsl_sinterp_hip_bary_fields_eval", "gsl_sinterp_hip_mesh3_fields_eval", "gsl_sinterp_hip_sort_wanted")


def all_kinds(pkg):
    return list(pkg.Sinterp.TYPES) + list(pkg.Sinterp.MORE_TYPES)


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


def test_symbols_and_methods_exist(pkg):
    L = pkg.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in pkg.capi.SIGNATURES, name
    for name in ("linear_init_fields", "linear_eval_fields_e", "linear_eval_fields_many", "linear_eval_fields_resident"):
        assert callable(getattr(pkg.Sinterp, name)), name
    for cls in (pkg.capi.DeviceTree, pkg.capi.DeviceMesh):
        for name in ("set_responses", "n_responses", "eval_fields_many", "eval_fields_resident"):
            assert callable(getattr(cls, name)), (cls, name)
    assert L.gsl_sinterp_hip_sort_wanted(1) == 0 and L.gsl_sinterp_hip_sort_wanted(1 << 24) == 1


def test_every_other_type_is_refused_with_one_message(pkg):
    messages = set()
    p = fake_device_pointer()
    for kind in all_kinds(pkg):
        if kind in LINEAR:
            continue
        s = pkg.Sinterp(kind, 2, 10, 0)
        x, y = np.zeros((10, 2)), np.zeros((3, 2))
        with pkg.capi.ErrorCalls() as calls:
            got = [s.linear_init_fields(x, np.zeros((10, 3))),
                   s.linear_init_fields(np.zeros((9, 2)), np.zeros((9, 70))),               # wrong in every other way as well
                   s.linear_eval_fields_many(y)[0], s.linear_eval_fields_many(np.zeros((3, 5)), want_grad=True, want_leaf=True)[0],
                   s.linear_eval_fields_resident(p, 3, 2, p, 1, p, 2, p), s.linear_eval_fields_resident(None, 0, 2, None, 0)]
            st, val, g = s.linear_eval_fields_e(y[0], want_grad=True)
        assert got == [pkg.GSL_EUNSUP] * 6 and st == pkg.GSL_EUNSUP and np.isnan(val).all() and np.isnan(g).all(), kind
        assert [c[1] for c in calls] == [pkg.GSL_EUNSUP] * 7, (kind, calls)
        messages |= {c[0] for c in calls}
        assert s.n_fields() == 0
        s.close()
    assert len(messages) == 1 and "gsl_sinterp_linear_simplex" in next(iter(messages))


@pytest.mark.parametrize("kind,dim", [("linear_simplex", 2), ("linear_mesh", 2), ("linear_mesh", 3)])
def test_linear_types_never_initialised(pkg, kind, dim):
    cap = pkg.capi
    s = pkg.Sinterp(kind, dim, 10, 0)
    x, y, p = np.zeros((10, dim)), np.zeros((3, dim)), fake_device_pointer()
    # shapes and K of init, before anything is built
    one_call(pkg, lambda: s.linear_init_fields(x, np.zeros((9, 3))), cap.GSL_EBADLEN)
    one_call(pkg, lambda: s.linear_init_fields(np.zeros((10, dim + 1)), np.zeros((10, 3))), cap.GSL_EBADLEN)
    one_call(pkg, lambda: s.linear_init_fields(np.zeros((9, dim)), np.zeros((10, 3))), cap.GSL_EBADLEN)
    one_call(pkg, lambda: s.linear_init_fields(x, np.zeros((10, 0))), cap.GSL_EINVAL)
    one_call(pkg, lambda: s.linear_init_fields(x, np.zeros((10, 65))), cap.GSL_EINVAL)
    if kind == "linear_mesh":                                                        # as gsl_sinterp_init: no triangulation set
        one_call(pkg, lambda: s.linear_init_fields(x, np.zeros((10, 3))), cap.GSL_EINVAL)
    assert s.n_fields() == 0
    # not initialised
    one_call(pkg, lambda: s.linear_eval_fields_many(y), cap.GSL_EINVAL)
    one_call(pkg, lambda: s.linear_eval_fields_many(y, want_grad=True, want_leaf=True), cap.GSL_EINVAL)
    one_call(pkg, lambda: s.linear_eval_fields_resident(p, 3, dim, p, 1, p, dim, p), cap.GSL_EINVAL)
    one_call(pkg, lambda: s.linear_eval_fields_resident(None, 0, dim, None, 1), cap.GSL_EINVAL)
    st, val, g = one_call(pkg, lambda: s.linear_eval_fields_e(y[0], want_grad=True), cap.GSL_EINVAL)
    assert np.isnan(val).all() and np.isnan(g).all()
    # shapes of the evaluation entries
    one_call(pkg, lambda: s.linear_eval_fields_many(np.zeros((3, dim + 1))), cap.GSL_EBADLEN)
    one_call(pkg, lambda: s.linear_eval_fields_many(y, out=(np.zeros((4, 1)), None)), cap.GSL_EBADLEN)
    one_call(pkg, lambda: s.linear_eval_fields_e(np.zeros(dim + 1)), cap.GSL_EBADLEN)
    # NULL
    L = pkg.lib()
    X, F, Y, S = (cap.as_matrix(a) for a in (x, np.zeros((10, 3)), y, np.zeros((3, 1))))
    yv, sv = cap.as_vector(np.zeros(dim)), cap.as_vector(np.zeros(1))
    for fn in (lambda: L.gsl_sinterp_linear_init_fields(None, C.byref(X), C.byref(F)), lambda: L.gsl_sinterp_linear_init_fields(s._p, None, C.byref(F)),
               lambda: L.gsl_sinterp_linear_init_fields(s._p, C.byref(X), None),
               lambda: L.gsl_sinterp_linear_eval_fields_many(None, C.byref(Y), C.byref(S), None, None),
               lambda: L.gsl_sinterp_linear_eval_fields_many(s._p, None, C.byref(S), None, None),
               lambda: L.gsl_sinterp_linear_eval_fields_many(s._p, C.byref(Y), None, None, None),
               lambda: L.gsl_sinterp_linear_eval_fields_e(None, C.byref(yv), C.byref(sv), None),
               lambda: L.gsl_sinterp_linear_eval_fields_e(s._p, None, C.byref(sv), None),
               lambda: L.gsl_sinterp_linear_eval_fields_e(s._p, C.byref(yv), None, None),
               lambda: L.gsl_sinterp_linear_eval_fields_resident(None, p, 3, dim, p, 1, None, 0, None),
               lambda: s.linear_eval_fields_resident(None, 3, dim, p, 1), lambda: s.linear_eval_fields_resident(p, 3, dim, None, 1)):
        one_call(pkg, fn, cap.GSL_EFAULT)
    s.close()


def test_mirror_and_raw_entries_refuse_null(pkg):
    L, cap = pkg.lib(), pkg.capi
    F, Y, S = (cap.as_matrix(a) for a in (np.zeros((10, 3)), np.zeros((3, 2)), np.zeros((3, 3))))
    p = fake_device_pointer()
    for pre in ("simplex_tree_device", "simplex_mesh_device"):
        one_call(pkg, lambda: getattr(L, pre + "_set_responses")(None, C.byref(F)), cap.GSL_EFAULT)
        one_call(pkg, lambda: getattr(L, pre + "_eval_fields_many")(None, C.byref(Y), C.byref(S), None, None), cap.GSL_EFAULT)
        one_call(pkg, lambda: getattr(L, pre + "_eval_fields_resident")(None, p, 3, 2, p, 3, None, 0, None), cap.GSL_EFAULT)
        assert getattr(L, pre + "_n_responses")(None) == 0
    g = np.zeros(12).ctypes.data_as(cap._pd)
    assert L.gsl_sinterp_hip_bary_fields_eval(None, 1, p, p, 3, p, 1, 1, g, p, p, 1, 2, p, 1, None, 0) == cap.GSL_EFAULT
    assert L.gsl_sinterp_hip_mesh3_fields_eval(None, 1, p, p, 4, p, 1, 1, g, p, p, 1, 3, p, 1, None, 0) == cap.GSL_EFAULT


def test_c_program_references_the_prototypes(pkg, tmp_path):
    libdir = os.path.dirname(pkg.library_path())
    exe = str(tmp_path / "linear_fields_prototypes")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if os.environ.get("GSL_SINTERP_ASAN") else []
    libname = os.path.basename(pkg.library_path())[3:-3]
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Werror", *san, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "linear_fields_prototypes.c"), "-o", exe,
                           "-L", libdir, "-l" + libname, "-lm", "-Wl,-rpath," + libdir])
    assert "ok" in subprocess.check_output([exe], text=True)
