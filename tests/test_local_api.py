"""Local kriging (gsl_sinterp_set_neighbours, gsl_sinterp_hip_knn / _local_krige) where it answers without a GPU: which
types take the switch, argument errors of the switch and of the raw entries (checked before anything touches the device),
the GSL_EUNSUP answers of the entries that need a global model, the struct field in the bindings, the C prototypes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KRIGING = ("kriging", "kriging_matern32", "kriging_matern52")
OTHERS = ("gaussian", "wendland", "matern32", "matern52", "imq", "tps", "tps_affine", "linear_simplex", "linear_mesh")
GAUSSIAN, TPS, WENDLAND, MATERN32, MATERN52, IMQ = 0, 1, 2, 3, 4, 5


@pytest.mark.parametrize("kind", KRIGING)
def test_set_neighbours_sets_the_field(pkg, kind):
    s = pkg.Sinterp(kind, 2, 100)
    assert s._p.contents.neighbours == 0                           # the default: the global model
    for k in (1, 16, 64):
        assert s.set_neighbours(k) == 0 and s._p.contents.neighbours == k
    assert s.set_neighbours(0) == 0 and s._p.contents.neighbours == 0
    assert s.route() == 0                                           # nothing initialised yet


@pytest.mark.parametrize("kind", OTHERS)
def test_set_neighbours_is_for_the_kriging_types(pkg, kind):
    s = pkg.Sinterp(kind, 2, 100)
    assert s.set_neighbours(16) == pkg.GSL_EINVAL and s._p.contents.neighbours == 0
    assert s.set_neighbours(0) == pkg.GSL_EINVAL


def test_set_neighbours_argument_errors(pkg):
    s = pkg.Sinterp("kriging_matern52", 2, 40)
    assert s.set_neighbours(65) == pkg.GSL_EINVAL                   # k > 64
    assert s.set_neighbours(41) == pkg.GSL_EINVAL                   # k > size
    assert s._p.contents.neighbours == 0
    assert s.set_neighbours(40) == 0 and s._p.contents.neighbours == 40
    assert pkg.lib().gsl_sinterp_set_neighbours(None, 4) == pkg.capi.GSL_EFAULT


def test_struct_field_is_last_and_a_size_t(pkg):
    name, ctype = pkg.capi.gsl_sinterp._fields_[-1]
    assert name == "neighbours" and ctype is C.c_size_t
    assert pkg.capi.gsl_sinterp._fields_[-2][0] == "want_loo"       # nothing moved in front of it
    s = pkg.Sinterp("kriging", 3, 10)
    assert s.set_nugget(0.25) == 0 and s.set_loo(1) == 0 and s.set_neighbours(7) == 0
    c = s._p.contents
    assert (c.dim, c.size, c.nugget, c.want_loo, c.neighbours) == (3, 10, 0.25, 1, 7)


def knn(pkg, ctx=None, n=100, dim=2, xtda=None, ytda=None, k=8, m=1):
    xtda = dim if xtda is None else xtda
    ytda = dim if ytda is None else ytda
    return pkg.lib().gsl_sinterp_hip_knn(ctx, None, n, dim, xtda, None, m, ytda, k, None, None, 0)


def krige(pkg, kind=MATERN52, eps=1.0, nugget=0.0, n=100, dim=2, k=8, m=1):
    return pkg.lib().gsl_sinterp_hip_local_krige(None, kind, eps, nugget, None, n, dim, dim, None, None, m, dim, k, None, None, None, None, 0)


def test_raw_entries_check_their_arguments_before_the_device(pkg):
    EINVAL, EFAULT = pkg.GSL_EINVAL, pkg.capi.GSL_EFAULT
    assert knn(pkg) == EFAULT and krige(pkg) == EFAULT              # good arguments, NULL context
    for k in (0, 65, 101):                                          # k < 1, k > 64, k > n
        assert knn(pkg, k=k, n=100 if k != 65 else 1000) == EINVAL
        assert krige(pkg, k=k, n=100 if k != 65 else 1000) == EINVAL
    for dim in (0, 4):
        assert knn(pkg, dim=dim, xtda=4, ytda=4) == EINVAL and krige(pkg, dim=dim) == EINVAL
    assert knn(pkg, xtda=1) == EINVAL and knn(pkg, ytda=1) == EINVAL
    assert krige(pkg, kind=TPS) == EINVAL and krige(pkg, kind=6) == EINVAL and krige(pkg, kind=-1) == EINVAL
    for kind in (GAUSSIAN, WENDLAND, MATERN32, MATERN52, IMQ):
        assert krige(pkg, kind=kind) == EFAULT                      # every positive definite kind gets as far as the context
    for nugget in (-1e-300, -1.0, np.inf, np.nan):
        assert krige(pkg, nugget=nugget) == EINVAL
    for eps in (0.0, -1.0, np.inf, np.nan):
        assert krige(pkg, eps=eps) == EINVAL
    assert pkg.lib().gsl_sinterp_hip_local_pack(None, None, 100, 2, 2, None, 0) == EFAULT
    assert pkg.lib().gsl_sinterp_hip_local_pack(None, None, 100, 4, 4, None, 0) == EINVAL
    assert pkg.lib().gsl_sinterp_hip_local_pack_count(None) == 0
    for name in ("knn", "local_krige", "local_pack", "local_pack_count"):
        assert callable(getattr(pkg.HipContext, name)), name


@pytest.mark.parametrize("kind", KRIGING)
def test_entries_that_need_a_global_model_answer_eunsup(pkg, kind, tmp_path):
    n, dim = 50, 2
    s = pkg.Sinterp(kind, dim, n)
    assert s.set_neighbours(16) == 0
    EUNSUP = pkg.capi.GSL_EUNSUP
    y = np.full((3, dim), 0.5)
    x = np.random.default_rng(1).random((n, dim))
    assert s.eval_grad_many(y)[0] == EUNSUP
    assert s.eval_grad_e(y[0])[0] == EUNSUP
    assert s.eval_grad_resident(None, 0, dim, None, None, dim) == EUNSUP
    assert s.init_fields(x, np.zeros((n, 2))) == EUNSUP
    assert s.eval_fields_many(y)[0] == EUNSUP
    assert s.eval_fields_e(y[0])[0] == EUNSUP
    assert s.eval_fields_resident(None, 0, dim, None, 1) == EUNSUP
    assert s.field_weights(0)[0] == EUNSUP and s.field_mean(0)[0] == EUNSUP
    assert s.weights()[0] == EUNSUP
    assert s.mean()[0] == EUNSUP
    path = str(tmp_path / "local.bin")
    assert s.fwrite(path) == EUNSUP and os.path.getsize(path) == 0  # nothing written
    assert s.set_loo(1) == 0
    assert s.loo_residuals(out=np.zeros((n, 1)))[0] == EUNSUP and s.loo_variance()[0] == EUNSUP
    # not initialised: the local entry and the variance say so, they are not unsupported
    assert s.eval_local_many(y)[0] == pkg.GSL_EINVAL
    assert s.eval_variance_many(y)[0] == pkg.GSL_EINVAL
    # back to the global model: the old answers
    assert s.set_neighbours(0) == 0
    assert s.mean()[0] == pkg.GSL_EINVAL and s.weights()[0] == pkg.GSL_EINVAL
    assert s.eval_grad_many(y)[0] == pkg.GSL_EINVAL


def test_eval_local_many_argument_errors(pkg):
    L = pkg.lib()
    assert L.gsl_sinterp_eval_local_many(None, None, None, None, None) == pkg.capi.GSL_EFAULT
    g = pkg.Sinterp("gaussian", 2, 50)
    assert g.eval_local_many(np.zeros((1, 2)))[0] == pkg.GSL_EINVAL  # not a kriging interpolant


def test_c_program_references_the_prototypes(pkg, tmp_path):
    libdir = os.path.dirname(pkg.library_path())
    exe = str(tmp_path / "local_prototypes")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if os.environ.get("GSL_SINTERP_ASAN") else []
    libname = os.path.basename(pkg.library_path())[3:-3]
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Werror", *san, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "local_prototypes.c"), "-o", exe,
                           "-L", libdir, "-l" + libname, "-lm", "-Wl,-rpath," + libdir])
    assert "ok" in subprocess.check_output([exe], text=True)
