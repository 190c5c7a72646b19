"""The Matern 3/2, Matern 5/2 and inverse multiquadric types where they answer without a GPU: the type symbols and their
names, the kind constants and TYPES keys of the bindings, the switches per type, state errors, and the C prototypes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"matern32": ("gsl_sinterp_rbf_matern32", "rbf-matern-3/2"),
         "matern52": ("gsl_sinterp_rbf_matern52", "rbf-matern-5/2"),
         "imq": ("gsl_sinterp_rbf_imq", "rbf-inverse-multiquadric"),
         "kriging_matern32": ("gsl_sinterp_kriging_matern32", "ordinary-kriging-matern-3/2"),
         "kriging_matern52": ("gsl_sinterp_kriging_matern52", "ordinary-kriging-matern-5/2")}
RBF = ("matern32", "matern52", "imq")
KRIGE = ("kriging_matern32", "kriging_matern52")


def test_constants_and_types_keys(pkg):
    cap = pkg.capi
    assert (cap.RBF_MATERN32, cap.RBF_MATERN52, cap.RBF_IMQ) == (3, 4, 5)
    assert (cap.RBF_GAUSSIAN, cap.RBF_TPS, cap.RBF_WENDLAND) == (0, 1, 2)        # the older kinds keep their values
    for key, (symbol, _) in NAMES.items():
        assert pkg.Sinterp.TYPES[key] == symbol
        assert symbol in cap.DATA_SYMBOLS


@pytest.mark.parametrize("kind", RBF + KRIGE)
def test_type_symbols_names_and_min_size(pkg, kind):
    symbol, name = NAMES[kind]
    L = pkg.lib()
    assert pkg.capi._ptr(symbol)                                                 # an exported, non-NULL `const gsl_sinterp_type *`
    for dim in (1, 2, 3):
        s = pkg.Sinterp(kind, dim, 1)                                            # min_size 1
        assert s.name() == name
        assert L.gsl_sinterp_min_size(s._p) == 1
    with pytest.raises(pkg.capi.GslError):
        pkg.Sinterp(kind, 2, 0)
    # five distinct types, none of them an older one
    ptrs = {pkg.capi._ptr(sym) for sym in pkg.Sinterp.TYPES.values()}
    assert len(ptrs) == len(pkg.Sinterp.TYPES)


@pytest.mark.parametrize("kind", RBF + KRIGE)
def test_switches_per_type(pkg, kind):
    cap = pkg.capi
    krige = kind in KRIGE
    s = pkg.Sinterp(kind, 2, 8)
    assert s.set_loo(1) == 0 and s._p.contents.want_loo == 1
    assert s.set_loo(0) == 0 and s._p.contents.want_loo == 0
    assert s.set_shape(4.0) == 0
    assert s.set_devices(2) == 0 and s.n_devices() == 2
    assert s.set_device_list([0, 0, 0]) == 0 and s.n_devices() == 3
    assert s.set_nugget(1e-3) == (0 if krige else pkg.GSL_EINVAL)
    assert s.set_variance(1) == (0 if krige else pkg.GSL_EINVAL)
    assert s._p.contents.want_variance == int(krige)
    # kriging chooses its own route; the plain types take every solver the Gaussian takes
    for solver in (cap.SOLVER_CHOLESKY2, cap.SOLVER_PCHOLESKY, cap.SOLVER_LU_REFINE):
        assert s.set_solver(solver) == (pkg.GSL_EINVAL if krige else 0)
    assert s.set_solver(cap.SOLVER_DEFAULT) == 0
    assert s.set_rcond(1) == (pkg.GSL_EINVAL if krige else 0)


@pytest.mark.parametrize("kind", RBF + KRIGE)
def test_uninitialised_interpolant(pkg, kind):
    krige = kind in KRIGE
    dim, n = 2, 8
    s = pkg.Sinterp(kind, dim, n)
    y = np.zeros((5, dim))
    assert s.n_fields() == 0 and s.route() == 0
    assert s.eval_many(y)[0] != 0 and s.eval_e(y[0])[0] != 0
    st, val, g = s.eval_grad_e(y[0])
    assert st == pkg.GSL_EINVAL and np.isnan(val) and np.isnan(g).all()
    assert s.eval_grad_many(y)[0] == pkg.GSL_EINVAL
    assert s.eval_fields_many(y, out=np.zeros((5, 3)))[0] == pkg.GSL_EINVAL
    assert s.field_weights(0)[0] == pkg.GSL_EINVAL and s.field_mean(0)[0] == pkg.GSL_EINVAL
    assert s.weights()[0] != 0
    assert s.mean()[0] == pkg.GSL_EINVAL
    assert s.poly()[0] == pkg.GSL_EINVAL and s.field_poly(0)[0] == pkg.GSL_EINVAL       # no affine tail on these types
    assert s.eval_variance_many(y)[0] == pkg.GSL_EINVAL
    assert s.set_loo(1) == 0
    E = np.full((n, 1), 7.0)
    assert s.loo_residuals(out=E)[0] == pkg.GSL_EINVAL and (E == 7.0).all()
    assert s.loo_variance(out=np.full(n, 7.0))[0] == pkg.GSL_EINVAL
    if krige:
        assert s.set_nugget(-1.0) == pkg.capi.GSL_EDOM


@pytest.mark.parametrize("kind", RBF + KRIGE)
def test_init_without_a_device_fails_cleanly(pkg, kind, tmp_path):
    """no device: the init reports a status (no abort, no fall-back) and the interpolant stays uninitialised, as for the
    older types; with a device there is nothing to check here (tests/test_gpu_kernels_matern_imq.py does)"""
    if pkg.lib().gsl_sinterp_hip_device_count() > 0:
        return
    rng = np.random.default_rng(3)
    x, f = rng.random((8, 2)), rng.random(8)
    for k in (kind, "gaussian"):
        s = pkg.Sinterp(k, 2, 8)
        assert s.init(x, f) != 0
        assert s.init_fields(x, np.column_stack([f, f])) != 0
        assert s.eval_many(x)[0] != 0 and s.n_fields() == 0
        assert s.fwrite(str(tmp_path / "none.bin")) == pkg.GSL_EINVAL                    # nothing to write


def test_raw_entries_reject_a_null_context_for_every_kind(pkg):
    L = pkg.lib()
    for kind in (3, 4, 5, 6, 7):
        assert L.gsl_sinterp_hip_rbf_fill(None, kind, 1.0, None, 0, 2, 2, None, 0) == pkg.capi.GSL_EFAULT
        assert L.gsl_sinterp_hip_rbf_eval_model(None, kind, 1.0, None, 0, 2, 2, None, None, 0, 2, None, 0) == pkg.capi.GSL_EFAULT


def test_c_program_references_the_prototypes(pkg, tmp_path):
    libdir = os.path.dirname(pkg.library_path())
    exe = str(tmp_path / "kernel_types_prototypes")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if os.environ.get("GSL_SINTERP_ASAN") else []
    libname = os.path.basename(pkg.library_path())[3:-3]
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Werror", *san, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "kernel_types_prototypes.c"), "-o", exe,
                           "-L", libdir, "-l" + libname, "-lm", "-Wl,-rpath," + libdir])
    assert "ok" in subprocess.check_output([exe], text=True)
