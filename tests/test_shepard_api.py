"""Modified quadratic Shepard interpolation, CPU part: the type and its name, the facade's allocation rules, the bounds of
gsl_sinterp_set_shepard, the status of every entry the type refuses, the argument checks of the raw entries (all answered
before anything touches a device), the bindings' type registry, and a C program against the headers.
-m gpu part: tests/test_gpu_shepard.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_name_and_type_registry(pkg):
    capi = pkg.capi
    assert "gsl_sinterp_shepard" in capi.DATA_SYMBOLS
    s = pkg.Sinterp("shepard", 2, 50, 0)
    assert s.name() == "modified-quadratic-shepard"
    assert pkg.lib().gsl_sinterp_min_size(s._p) == 7
    # the registry the status matrix pins stays as it is; the new type lives beside it
    assert len(pkg.Sinterp.TYPES) == 16 and "shepard" not in pkg.Sinterp.TYPES
    assert pkg.Sinterp.MORE_TYPES == {"shepard": "gsl_sinterp_shepard"}
    ptrs = {capi._ptr(sym) for sym in list(pkg.Sinterp.TYPES.values()) + list(pkg.Sinterp.MORE_TYPES.values())}
    assert len(ptrs) == 17 and None not in ptrs and 0 not in ptrs
    for name in ("gsl_sinterp_hip_shepard_fit", "gsl_sinterp_hip_shepard_eval", "gsl_sinterp_hip_shepard_pack_count",
                 "gsl_sinterp_hip_shepard_fit_count", "gsl_sinterp_set_shepard", "gsl_sinterp_shepard_stats", "gsl_sinterp_shepard_ctx"):
        assert name in capi.SIGNATURES and hasattr(pkg.lib(), name)


@pytest.mark.parametrize("dim,status", [(1, "GSL_EUNIMPL"), (2, None), (3, None), (4, "GSL_EUNIMPL")])
def test_alloc_by_dimension(pkg, dim, status):
    capi = pkg.capi
    with capi.ErrorCalls() as calls:
        if status is None:
            assert pkg.Sinterp("shepard", dim, 100, 0).name() == "modified-quadratic-shepard"
        else:
            with pytest.raises(capi.GslError):
                pkg.Sinterp("shepard", dim, 100, 0)
    assert [s for _, s in calls] == ([] if status is None else [getattr(capi, status)])


def test_alloc_below_min_size(pkg):
    capi = pkg.capi
    with capi.ErrorCalls() as calls:
        with pytest.raises(capi.GslError):
            pkg.Sinterp("shepard", 2, 6, 0)
    assert [s for _, s in calls] == [capi.GSL_EINVAL]


def test_set_shepard_bounds(pkg):
    capi = pkg.capi
    s2, s3 = pkg.Sinterp("shepard", 2, 100, 0), pkg.Sinterp("shepard", 3, 100, 0)
    assert s2.set_shepard(0, 0) == 0 and s2.set_shepard(5, 1) == 0 and s2.set_shepard(62, 62) == 0 and s2.set_shepard(8, 10) == 0
    assert s3.set_shepard(9, 1) == 0 and s3.set_shepard(0, 40) == 0
    with capi.ErrorCalls() as calls:
        assert s2.set_shepard(4, 10) == capi.GSL_EINVAL            # fewer neighbours than monomials
        assert s3.set_shepard(8, 10) == capi.GSL_EINVAL
        assert s2.set_shepard(63, 10) == capi.GSL_EINVAL           # k = max + 2 > 64
        assert s2.set_shepard(10, 63) == capi.GSL_EINVAL
        assert pkg.Sinterp("gaussian", 2, 100, 0).set_shepard(0, 0) == capi.GSL_EINVAL
        assert pkg.Sinterp("cubic_simplex", 2, 100, 0).set_shepard(0, 0) == capi.GSL_EINVAL
        assert pkg.lib().gsl_sinterp_set_shepard(None, 0, 0) == capi.GSL_EFAULT
    assert len(calls) == 7


def test_init_refusals_before_any_device(pkg):
    capi = pkg.capi
    x, f = np.random.default_rng(0).random((20, 2)), np.zeros(20)
    s = pkg.Sinterp("shepard", 2, 20, 0)                            # default nw = 19 needs 21 sites
    with capi.ErrorCalls() as calls:
        assert s.init(x, f) == capi.GSL_EINVAL
        assert s.set_shepard(13, 18) == 0 and s.set_devices(2) == 0
        assert s.init(x, f) == capi.GSL_EUNSUP                      # one device only
    assert [st for _, st in calls] == [capi.GSL_EINVAL, capi.GSL_EUNSUP]


def test_unsupported_entries(pkg):
    capi = pkg.capi
    L = pkg.lib()
    x, f = np.random.default_rng(0).random((30, 2)), np.zeros(30)
    s = pkg.Sinterp("shepard", 2, 30, 0)
    with capi.ErrorCalls() as calls:
        assert s.set_neighbours(3) == capi.GSL_EUNSUP
        assert L.gsl_sinterp_eval_variance_resident(s._p, None, 0, 2, None) == capi.GSL_EUNSUP
        assert s.init_fields(x, np.zeros((30, 2))) == capi.GSL_EUNSUP
        assert s.eval_fields_many(x)[0] == capi.GSL_EUNSUP
        assert s.loo_variance()[0] == capi.GSL_EUNSUP
        assert s.loo_residuals()[0] == capi.GSL_EUNSUP
        assert not L.gsl_sinterp_fit_alloc(s._p, C.byref(capi.as_matrix(x)), C.byref(capi.as_vector(f)))
    assert [st for _, st in calls] == [capi.GSL_EUNSUP] * 7
    with capi.ErrorCalls() as calls:
        assert s.set_solver(1) == capi.GSL_EINVAL
        assert s.weights()[0] == capi.GSL_EINVAL
        assert s.mean()[0] == capi.GSL_EINVAL
        assert s.poly()[0] == capi.GSL_EINVAL
        assert s.set_nugget(0.1) == capi.GSL_EINVAL
        assert s.set_variance(True) == capi.GSL_EINVAL
        assert s.set_loo(True) == capi.GSL_EINVAL
        assert s.set_triangulation(np.array([[0, 1, 2]], dtype=np.int32)) == capi.GSL_EINVAL
        assert s.set_gradients(np.zeros((30, 2))) == capi.GSL_EINVAL
        assert s.eval_local_many(x)[0] == capi.GSL_EINVAL
    assert [st for _, st in calls] == [capi.GSL_EINVAL] * 10
    # supported entries of an interpolant that is not initialised say so
    with capi.ErrorCalls() as calls:
        assert s.eval_many(x)[0] == capi.GSL_EINVAL
        assert L.gsl_sinterp_eval_resident(s._p, None, 0, 2, None, None) == capi.GSL_EINVAL
        assert s.eval_grad_many(x)[0] == capi.GSL_EINVAL
        assert L.gsl_sinterp_eval_grad_resident(s._p, None, 0, 2, None, None, 2) == capi.GSL_EINVAL
        assert s.get_gradients()[0] == capi.GSL_EINVAL
        assert s.shepard_stats()[0] == capi.GSL_EINVAL
        assert s.eval_grid([0, 0], [1, 1], 4, 4)[0] == capi.GSL_EINVAL
    assert [st for _, st in calls] == [capi.GSL_EINVAL] * 7
    assert s.shepard_counters() == (0, 0)


def test_fwrite_of_an_uninitialised_interpolant(pkg, tmp_path):
    capi = pkg.capi
    s = pkg.Sinterp("shepard", 3, 40, 0)
    with capi.ErrorCalls() as calls:
        assert s.fwrite(str(tmp_path / "m.bin")) == capi.GSL_EINVAL
    assert [st for _, st in calls] == [capi.GSL_EINVAL]


def test_raw_argument_checks(pkg):
    capi = pkg.capi
    L = pkg.lib()
    buf = np.zeros(64)
    p = buf.ctypes.data
    counts = (C.c_size_t * 3)(9, 9, 9)
    fit = lambda ctx, n, dim, xtda, nq, nw, ptr=p: L.gsl_sinterp_hip_shepard_fit(ctx, ptr, n, dim, xtda, p, nq, nw, p, p, p, counts)
    assert fit(None, 100, 1, 1, 13, 19) == capi.GSL_EINVAL                 # dim
    assert fit(None, 100, 4, 4, 13, 19) == capi.GSL_EINVAL
    assert fit(None, 100, 2, 2, 4, 19) == capi.GSL_EINVAL                  # nq < nc
    assert fit(None, 100, 3, 3, 8, 19) == capi.GSL_EINVAL
    assert fit(None, 100, 2, 2, 13, 0) == capi.GSL_EINVAL                  # nw < 1
    assert fit(None, 100, 2, 2, 63, 19) == capi.GSL_EINVAL                 # k > 64
    assert fit(None, 100, 2, 2, 13, 63) == capi.GSL_EINVAL
    assert fit(None, 20, 2, 2, 13, 19) == capi.GSL_EINVAL                  # k > n
    assert fit(None, 100, 3, 2, 17, 32) == capi.GSL_EINVAL                 # tda < dim
    assert fit(None, 100, 2, 2, 13, 19) == capi.GSL_EFAULT                 # the numbers are fine: the NULL context
    assert list(counts) == [0, 0, 0]
    outside = C.c_size_t(9)
    ev = lambda dim, xtda, ytda, gtda, g=None: L.gsl_sinterp_hip_shepard_eval(None, p, 100, dim, xtda, p, p, p, p, p, 1, ytda, p, g, gtda, None,
                                                                             C.byref(outside), 0)
    assert ev(1, 1, 1, 0) == capi.GSL_EINVAL and ev(4, 4, 4, 0) == capi.GSL_EINVAL
    assert ev(2, 1, 2, 0) == capi.GSL_EINVAL and ev(2, 2, 1, 0) == capi.GSL_EINVAL and ev(3, 3, 3, 2, p) == capi.GSL_EINVAL
    assert ev(2, 2, 2, 0) == capi.GSL_EFAULT and outside.value == 0
    assert L.gsl_sinterp_hip_shepard_pack_count(None) == 0 and L.gsl_sinterp_hip_shepard_fit_count(None) == 0


def test_c_program_references_the_shepard_prototypes(pkg, tmp_path):
    libdir = os.path.dirname(pkg.library_path())
    exe = str(tmp_path / "shepard_prototypes")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if os.environ.get("GSL_SINTERP_ASAN") else []
    libname = os.path.basename(pkg.library_path())[3:-3]
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Werror", *san, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "shepard_prototypes.c"), "-o", exe,
                           "-L", libdir, "-l" + libname, "-lm", "-Wl,-rpath," + libdir])
    assert "ok" in subprocess.check_output([exe], text=True)
