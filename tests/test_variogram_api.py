"""The variogram entry points where they answer without a GPU: every argument and state error (none may reach a device), the
bindings, the C prototypes, and gsl_sinterp_variogram_fit_model against the Python reference of tests/variogram_ref.py on
synthetic, exact variograms."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import variogram_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = {"gaussian": ref.GAUSSIAN, "matern32": ref.MATERN32, "matern52": ref.MATERN52}
NEW_SYMBOLS = ("gsl_sinterp_hip_variogram", "gsl_sinterp_hip_variogram_pairs_tested", "gsl_sinterp_hip_bbox", "gsl_sinterp_variogram_alloc",
               "gsl_sinterp_variogram_set_device", "gsl_sinterp_variogram_compute", "gsl_sinterp_variogram_compute_resident",
               "gsl_sinterp_variogram_get", "gsl_sinterp_variogram_h_max", "gsl_sinterp_variogram_fit", "gsl_sinterp_variogram_apply",
               "gsl_sinterp_variogram_free", "gsl_sinterp_variogram_fit_model", "gsl_sinterp_variogram_fit_model_n_eval",
               "gsl_sinterp_variogram_fit_model_trace")


def synthetic(kind, eps, c0=0.2, c=1.7, n_bins=15, h_max=0.5):
    lag = (np.arange(n_bins) + 0.5) * h_max / n_bins
    gamma = ref.model(kind, eps, c0, c, lag)
    count = 50.0 * (np.arange(n_bins) + 1.0)              # as many pairs as an annulus holds
    return lag, gamma, count


def test_symbols_bindings_and_constants(pkg):
    capi, L = pkg.capi, pkg.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in capi.SIGNATURES, name
    for name in ("compute", "compute_resident", "get", "fit", "apply", "close", "h_max", "set_device"):
        assert callable(getattr(pkg.Variogram, name)), name
    for name in ("variogram", "variogram_pairs_tested", "bbox"):
        assert callable(getattr(pkg.HipContext, name)), name
    assert (capi.VARIOGRAM_MATHERON, capi.VARIOGRAM_CRESSIE) == (0, 1) == (pkg.Variogram.MATHERON, pkg.Variogram.CRESSIE)
    assert (capi.VARIOGRAM_W_COUNT, capi.VARIOGRAM_W_COUNT_H2, capi.VARIOGRAM_W_NONE) == (0, 1, 2)
    hdr = open(os.path.join(ROOT, "include", "gsl_sinterp.h")).read()
    for name, val in (("MATHERON", 0), ("CRESSIE", 1), ("W_COUNT", 0), ("W_COUNT_H2", 1), ("W_NONE", 2)):
        assert any(line.split()[:3] == ["#define", "GSL_SINTERP_VARIOGRAM_" + name, str(val)] for line in hdr.splitlines()), name
    assert (ref.GAUSSIAN, ref.MATERN32, ref.MATERN52) == (pkg.RBF_GAUSSIAN, pkg.RBF_MATERN32, pkg.RBF_MATERN52)


@pytest.mark.parametrize("dim,n_bins", [(0, 15), (4, 15), (2, 0), (2, 257)])
def test_alloc_refuses_through_the_handler(pkg, dim, n_bins):
    with pkg.capi.ErrorCalls() as calls:
        assert not pkg.lib().gsl_sinterp_variogram_alloc(dim, n_bins)
    assert [c[1] for c in calls] == [pkg.GSL_EINVAL]
    with pytest.raises(pkg.capi.GslError) as err:
        pkg.Variogram(dim, n_bins)
    assert err.value.status == pkg.GSL_EINVAL


def test_facade_statuses_before_any_device(pkg):
    capi = pkg.capi
    EFAULT, EBADLEN, EINVAL, EUNSUP = capi.GSL_EFAULT, capi.GSL_EBADLEN, capi.GSL_EINVAL, capi.GSL_EUNSUP
    L = pkg.lib()
    for dim in (1, 2, 3):
        for nb in (1, 256):
            pkg.Variogram(dim, nb).close()
    v = pkg.Variogram(2, 15)
    x, f = np.zeros((8, 2)), np.zeros(8)
    with capi.ErrorCalls() as calls:
        assert v.compute(None, f, 1.0) == EFAULT and v.compute(x, None, 1.0) == EFAULT
        assert L.gsl_sinterp_variogram_compute(None, C.byref(capi.as_matrix(x)), C.byref(capi.as_vector(f)), 1.0) == EFAULT
        assert v.compute(np.zeros((8, 3)), f, 1.0) == EBADLEN and v.compute(x, np.zeros(7), 1.0) == EBADLEN
        assert v.compute(x, f, float("nan")) == EINVAL and v.compute(x, f, float("inf")) == EINVAL
        p = C.addressof(C.create_string_buffer(256))
        assert v.compute_resident(None, 8, 2, p, 1.0) == EFAULT and v.compute_resident(p, 8, 2, None, 1.0) == EFAULT
        assert L.gsl_sinterp_variogram_compute_resident(None, p, 8, 2, p, 1.0) == EFAULT
        assert v.compute_resident(p, 8, 1, p, 1.0) == EBADLEN
        assert v.compute_resident(p, 8, 2, p, float("nan")) == EINVAL and v.compute_resident(p, 1 << 31, 2, p, 1.0) == EINVAL
        assert len(calls) == 13 and all(c[1] != 0 for c in calls)        # every one through the handler
    assert np.isnan(v.h_max()) and np.isnan(L.gsl_sinterp_variogram_h_max(None))
    st, lag, gamma, count = v.get()
    assert st == EINVAL                                                   # no variogram
    assert L.gsl_sinterp_variogram_get(None, 0, None, None, None) == EFAULT
    assert L.gsl_sinterp_variogram_get(v._h, 2, None, None, None) == EINVAL
    assert v.set_device(-1) == EINVAL and v.set_device(0) == 0 and L.gsl_sinterp_variogram_set_device(None, 0) == EFAULT
    # fit: the type is judged before the state
    assert v.fit("gaussian")[0] == EINVAL and v.fit("matern32")[0] == EINVAL and v.fit("tps")[0] == EINVAL and v.fit("imq")[0] == EINVAL
    for kind in ("linear_mesh", "linear_simplex", "natural_mesh", "cubic_simplex", "shepard"):
        assert v.fit(kind)[0] == EUNSUP, kind
    for kind in ("kriging", "kriging_matern32", "kriging_matern52"):
        st, eps, nug, s2, wss = v.fit(kind)
        assert st == EINVAL and all(np.isnan(t) for t in (eps, nug, s2, wss))  # no variogram
        assert v.fit(kind, estimator=2)[0] == EINVAL and v.fit(kind, weights=3)[0] == EINVAL
    assert v.fit(None)[0] == EFAULT
    out = C.c_double(0)
    assert L.gsl_sinterp_variogram_fit(None, capi._ptr("gsl_sinterp_kriging"), 0, 1, 0.0, 0.0, C.byref(out), C.byref(out), C.byref(out), None) == EFAULT
    assert L.gsl_sinterp_variogram_fit(v._h, capi._ptr("gsl_sinterp_kriging"), 0, 1, 0.0, 0.0, None, C.byref(out), C.byref(out), None) == EFAULT
    s = pkg.Sinterp("kriging_matern32", 2, 8)
    assert v.apply(s) == EINVAL and v.apply(None) == EFAULT and L.gsl_sinterp_variogram_apply(None, s._p) == EFAULT
    assert s._p.contents.shape == 0.0 and s._p.contents.nugget == 0.0
    L.gsl_sinterp_variogram_free(None)
    v.close()


def test_raw_entry_statuses_without_a_context(pkg):
    L = pkg.lib()
    EFAULT, EINVAL = pkg.capi.GSL_EFAULT, pkg.GSL_EINVAL
    acc = (C.c_uint64 * 7)()
    shift = (C.c_int * 3)()
    p = C.addressof(C.create_string_buffer(256))
    call = lambda dim, xtda, h, nb, n=4, a=acc, s=shift: L.gsl_sinterp_hip_variogram(None, p, n, dim, xtda, p, h, nb, a, s)
    for dim in (0, 4, -1):
        assert call(dim, 4, 1.0, 15) == EINVAL
    for nb in (0, 257, -3):
        assert call(2, 2, 1.0, nb) == EINVAL
    for h in (0.0, -1.0, float("inf"), float("nan")):
        assert call(2, 2, h, 1) == EINVAL
    assert call(2, 1, 1.0, 1) == EINVAL and call(2, 2, 1.0, 1, n=1 << 31) == EINVAL
    assert call(2, 2, 1.0, 1) == EFAULT                                   # the NULL context, after the numbers
    assert L.gsl_sinterp_hip_variogram_pairs_tested(None) == 0
    assert L.gsl_sinterp_hip_bbox(None, p, 4, 2, 2, None) == EFAULT and L.gsl_sinterp_hip_bbox(None, p, 0, 2, 2, None) == EINVAL


def test_c_program_references_the_prototypes(pkg, tmp_path):
    libdir = os.path.dirname(pkg.library_path())
    exe = str(tmp_path / "variogram_prototypes")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if os.environ.get("GSL_SINTERP_ASAN") else []
    libname = os.path.basename(pkg.library_path())[3:-3]
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Werror", *san, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "variogram_prototypes.c"), "-o", exe,
                           "-L", libdir, "-l" + libname, "-lm", "-Wl,-rpath," + libdir])
    assert "ok" in subprocess.check_output([exe], text=True)


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("eps", [3.0, 8.0, 20.0])
def test_fit_model_recovers_an_exact_variogram(pkg, kind, eps):
    """15 bins, lags (b + 1/2) 0.5 / 15, c0 = 0.2, c = 1.7, weights N_b / h^2, bracket 0.5 .. 200, tol 1e-8, max_eval 200: eps to 1e-6
    relative, c0 and c to 1e-5 relative (a numpy prototype of the rule reaches 1e-9 in 51 evaluations)."""
    capi = pkg.capi
    lag, gamma, count = synthetic(KINDS[kind], eps)
    st, e, c0, c, wss = capi.variogram_fit_model(KINDS[kind], capi.VARIOGRAM_W_COUNT_H2, lag, gamma, count, 0.5, 200.0, 9, 1e-8, 200)
    n_eval = int(pkg.lib().gsl_sinterp_variogram_fit_model_n_eval())
    r_e, r_c0, r_c, r_wss, trace = ref.fit_model(KINDS[kind], ref.W_COUNT_H2, lag, gamma, count, 0.5, 200.0, 9, 1e-8, 200)
    print(f"{kind} eps {eps}: {n_eval} evaluations, eps off {abs(e / eps - 1):.2e}, c0 off {abs(c0 / 0.2 - 1):.2e}, c off {abs(c / 1.7 - 1):.2e}, "
          f"wss {wss:.2e}; reference eps off {abs(r_e / eps - 1):.2e} in {len(trace)}")
    assert st == 0 and n_eval <= 200
    assert abs(e / eps - 1) <= 1e-6 and abs(c0 / 0.2 - 1) <= 1e-5 and abs(c / 1.7 - 1) <= 1e-5
    assert abs(r_e / eps - 1) <= 1e-6 and wss >= 0.0


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("eps", [3.0, 8.0, 20.0])
@pytest.mark.parametrize("weights", [0, 1, 2])
def test_default_search_agrees_with_the_reference(pkg, kind, eps, weights):
    """the defaults (9, 1e-2, 40), passed as zeros: the same number of evaluations, eps to 1e-12 relative, the same trace"""
    capi = pkg.capi
    lag, gamma, count = synthetic(KINDS[kind], eps)
    gamma = gamma * (1.0 + 0.05 * np.cos(7.0 * np.arange(15)))             # not an exact model: the sum of squares stays away from 0
    st, e, c0, c, wss = capi.variogram_fit_model(KINDS[kind], weights, lag, gamma, count, 0.5, 200.0)
    r_e, r_c0, r_c, r_wss, trace = ref.fit_model(KINDS[kind], weights, lag, gamma, count, 0.5, 200.0)
    st_t, t_eps, t_wss = capi.variogram_fit_model_trace()
    assert st == 0 and st_t == 0 and len(t_eps) == len(trace) <= 40
    assert abs(e / r_e - 1) <= 1e-12 and abs(c0 - r_c0) <= 1e-10 * (r_c0 + r_c) and abs(c - r_c) <= 1e-10 * (r_c0 + r_c)
    assert np.allclose(t_eps, [t[0] for t in trace], rtol=1e-12, atol=0) and np.allclose(t_wss, [t[1] for t in trace], rtol=1e-9, atol=0)
    assert wss == t_wss.min() and e == t_eps[np.argmin(t_wss)] and t_eps[0] == 0.5 and t_eps[8] == 200.0


def test_search_settings_and_argument_errors(pkg):
    capi = pkg.capi
    EINVAL, EFAULT = pkg.GSL_EINVAL, capi.GSL_EFAULT
    lag, gamma, count = synthetic(ref.MATERN32, 8.0)
    fm = lambda *a, **k: capi.variogram_fit_model(*a, **k)[0]
    for kind in (capi.RBF_TPS, capi.RBF_WENDLAND, capi.RBF_IMQ, -1, 6):
        assert fm(kind, 1, lag, gamma, count, 0.5, 200.0) == EINVAL
    assert fm(ref.MATERN32, 3, lag, gamma, count, 0.5, 200.0) == EINVAL and fm(ref.MATERN32, -1, lag, gamma, count, 0.5, 200.0) == EINVAL
    assert fm(ref.MATERN32, 1, lag, gamma, count, 0.5, 200.0, n_grid=2) == EINVAL
    assert fm(ref.MATERN32, 1, lag, gamma, count, 0.5, 200.0, tol=-1e-2) == EINVAL
    assert fm(ref.MATERN32, 1, lag, gamma, count, 0.5, 200.0, tol=float("nan")) == EINVAL
    assert fm(ref.MATERN32, 1, lag, gamma, count, 0.5, 200.0, max_eval=8) == EINVAL
    assert fm(ref.MATERN32, 1, lag, gamma, count, 0.5, 200.0, n_grid=41) == EINVAL        # above the default max_eval
    for lo, hi in ((0.0, 1.0), (-1.0, 1.0), (2.0, 2.0), (2.0, 1.0), (1.0, float("inf")), (float("nan"), 1.0)):
        assert fm(ref.MATERN32, 1, lag, gamma, count, lo, hi) == EINVAL
    assert fm(ref.MATERN32, 1, None, gamma, count, 0.5, 200.0) == EFAULT
    assert fm(ref.MATERN32, 7, None, gamma, count, 0.5, 200.0) == EINVAL                  # the numbers before the pointers
    st, e, c0, c, wss = capi.variogram_fit_model(ref.MATERN32, 7, lag, gamma, count, 0.5, 200.0)
    assert all(np.isnan(t) for t in (e, c0, c, wss))
    with capi.ErrorCalls() as calls:
        fm(ref.MATERN32, 1, lag, gamma, count, 0.5, 200.0, n_grid=2)
        assert [c[1] for c in calls] == [EINVAL]


def test_degenerate_fits(pkg):
    capi = pkg.capi
    lag, gamma, count = synthetic(ref.MATERN32, 8.0)
    # fewer than 3 usable bins
    few = count.copy()
    few[2:] = 0.0
    st, e, c0, c, wss = capi.variogram_fit_model(ref.MATERN32, 1, lag, gamma, few, 0.5, 200.0)
    assert st == pkg.GSL_EDOM and all(np.isnan(t) for t in (e, c0, c, wss))
    assert ref.fit_model(ref.MATERN32, 1, lag, gamma, few, 0.5, 200.0) is None
    bad = gamma.copy()
    bad[:13] = np.nan
    assert capi.variogram_fit_model(ref.MATERN32, 1, lag, bad, count, 0.5, 200.0)[0] == pkg.GSL_EDOM
    # a constant gamma is a pure nugget: c = 0 exactly, no error from fit_model
    for weights in (0, 1, 2):
        st, e, c0, c, wss = capi.variogram_fit_model(ref.MATERN32, weights, lag, np.full(15, 2.0), count, 0.5, 200.0)
        assert st == 0 and c == 0.0 and c0 == 2.0 and wss == 0.0 and e == 0.5          # the first point evaluated already has wss 0
    # an empty bin in the middle (NaN lag and gamma, count 0, as gsl_sinterp_variogram_get reports it) is skipped
    lag2, gamma2, count2 = lag.copy(), gamma.copy(), count.copy()
    lag2[7], gamma2[7], count2[7] = np.nan, np.nan, 0.0
    st, e, c0, c, wss = capi.variogram_fit_model(ref.MATERN32, 1, lag2, gamma2, count2, 0.5, 200.0, 9, 1e-8, 200)
    keep = np.arange(15) != 7
    st3, e3, c03, c3, wss3 = capi.variogram_fit_model(ref.MATERN32, 1, lag[keep], gamma[keep], count[keep], 0.5, 200.0, 9, 1e-8, 200)
    assert st == 0 and st3 == 0 and (e, c0, c, wss) == (e3, c03, c3, wss3) and abs(e / 8.0 - 1) <= 1e-6
    r = ref.fit_model(ref.MATERN32, 1, lag2, gamma2, count2, 0.5, 200.0, 9, 1e-8, 200)
    assert abs(r[0] / 8.0 - 1) <= 1e-6
    # a bin of coincident sites (lag 0) has no finite N / h^2: skipped under W_COUNT_H2, kept under the other weights
    lag0 = lag.copy()
    lag0[0] = 0.0
    g0 = ref.model(ref.MATERN32, 8.0, 0.2, 1.7, lag0)
    assert abs(capi.variogram_fit_model(ref.MATERN32, 1, lag0, g0, count, 0.5, 200.0, 9, 1e-8, 200)[1] / 8.0 - 1) <= 1e-6
    assert abs(capi.variogram_fit_model(ref.MATERN32, 0, lag0, g0, count, 0.5, 200.0, 9, 1e-8, 200)[1] / 8.0 - 1) <= 1e-6
