"""-m gpu: backward and forward errors of every factorisation and solve route on ill-conditioned matrices.

The other Cholesky tests use one matrix family with condition number ~1 (spd(n) = random + 10 n I).  Here the inputs are
the zoo of tests/stability_ref.py (prescribed spectra up to 1e10, flat Gaussian kernel matrices with a nugget, a graded
matrix, 2^+-900 scalings, numerically semi-definite matrices) and the bounds come from LAPACK ON THE SAME MATRIX:

    figure(gpu) <= 16 x figure(LAPACK),      residuals taken beyond float64 (stability_ref.product_ld, np.longdouble)

16 is the rule tests/test_gpu_linear_fields.py uses for C_GRAD: room for another valid summation order and for the
row solve that multiplies by inverted 32 x 32 blocks (tests/test_stability_ref.py shows a numpy model of that design
within 8 x LAPACK on every entry), orders of magnitude below a dropped K-slice or a short 1/sqrt(d) correction chain.
It is never measured on the code under test.

The switches are read once per process, so every route is one child interpreter (this file run as a script) that runs
all its cases once and writes a JSON of figures; the children run one after another, each under a timeout, and the first
one that fails stops the rest.  The residual of a factor is keyed by the factor's bits, so routes that return the same
bits (packed / strided, rider on / off) cost one residual.  With GSL_SINTERP_STABILITY_RECORD=path in the environment
every measured ratio is also written to that file (profiles/stability_ratios.json was made that way): factor, solve,
forward, componentwise and scale figures, the outcome of every semi-definite case, the lu_refine residuals beside
scipy's, what each child's switch left behind, and the kriging-variance and leave-one-out errors of (f).

Sizes: 96 (base kernel, three 32-wide leaves, two sweep blocks), 424 (128-wide leaves with the side-buffer write-back),
1024 (all-128, riders, folded substitution), 2176 (17 panels, uneven splits, stream-K; three entries only).
LU sizes: 33, 700, 1100 (more than 1024 rows: the cooperative panels)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import stability_ref as sr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = sr.MARGIN

SWITCHES = ["GSL_SINTERP_TRSM_RF", "GSL_SINTERP_NO_DIAG_RIDER", "GSL_SINTERP_NO_PANEL128", "GSL_SINTERP_NO_FOLD",
            "GSL_SINTERP_NO_DATAFLOW_TRSV", "GSL_SINTERP_GEMM_CFG", "GSL_SINTERP_GEMM_RULE_R4"]
ROUTES = {
    "default": {},
    "trsm_rf64": {"GSL_SINTERP_TRSM_RF": "64"},               # strip row solve
    "no_rider": {"GSL_SINTERP_NO_DIAG_RIDER": "1"},
    "no_panel128": {"GSL_SINTERP_NO_PANEL128": "1"},          # 32-wide recursion at every size
    "no_fold": {"GSL_SINTERP_NO_FOLD": "1"},
    "no_dataflow_trsv": {"GSL_SINTERP_NO_DATAFLOW_TRSV": "1"},   # one launch per block of the sweeps
    "gemm_cfg0": {"GSL_SINTERP_GEMM_CFG": "0"},               # 256 x 128 tile: meaningful at n = 2176 only
}
LU_ROUTES = ["default", "no_dataflow_trsv"]                   # the sweeps are shared with lu.hip
FOLLOW = {96: "spec_1e6", 424: "spec_1e6", 1024: "spec_1e6", 2176: "spec_1e10"}   # the good matrix after a semi-definite one
SEMIDEF_CASES = [(name, n) for name in sr.SEMIDEF for n in sr.SIZES[:-1]] + [("semidef_gram", 2176)]
N_RHS = 5
CANARY = -7.25                                                # fills the doubles around a matrix; no zoo entry holds it
N_KRIGE, M_KRIGE = 1024, 500


def layouts(n):
    """(name, lda, offset in doubles): packed, and lda > n behind a 16-byte offset (tests/test_gpu_chol_rider.py)"""
    return [("packed", n, 0), ("strided", n + 6, 2)]


def pd_cases(route):
    names = sr.PD + ["spec_1e4"]
    cases = [(name, n) for name in names for n in sr.sizes_of(name)]
    return [c for c in cases if c[1] == 2176] if route == "gemm_cfg0" else cases


def semidef_cases(route):
    return [c for c in SEMIDEF_CASES if c[1] == 2176] if route == "gemm_cfg0" else SEMIDEF_CASES


def route_names(names, cases_of):
    """(route, name) pairs that have at least one case"""
    return [(r, nm) for r in ROUTES for nm in names if any(c[0] == nm for c in cases_of(r))]


def key(name, n):
    return "%s_%d" % (name, n)


def lu_rhs(a, kind):
    xs = np.random.default_rng(len(a)).standard_normal(len(a))
    return a @ xs


# ---------------------------------------------------------------- the child: one route, every case once
class Residuals:
    """factor_figures keyed by (matrix, bits of the factor), shared by the children through a file"""

    def __init__(self, path):
        self.path, self.d = path, {}
        if os.path.exists(path):
            with open(path) as f:
                self.d = json.load(f)

    def figures(self, tag, a, l):
        k = tag + ":" + hashlib.sha1(np.ascontiguousarray(l).tobytes()).hexdigest()
        if k not in self.d:
            self.d[k] = list(sr.factor_figures(a, l))
        return self.d[k]

    def save(self):
        with open(self.path, "w") as f:
            json.dump(self.d, f)


def _child(route, zoo_dir, out_path):
    sys.path.insert(0, ROOT)
    import torch
    import __graft_entry__ as g
    from gpu_util import dev, ptr
    pkg = g.load_package()
    ctx = pkg.HipContext.on_torch_stream(0)
    cache = Residuals(os.path.join(zoo_dir, "residuals.json"))
    load = lambda what, name, n: np.load(os.path.join(zoo_dir, "%s_%s_%d.npy" % (what, name, n)))
    res = {"factor": {}, "solve": {}, "scale": {}, "semidef": {}, "lu": {}, "route": {}}

    def stage(a, lda, off):
        """a in the given layout, every double around it (in front of the offset, right of column n) holding CANARY"""
        n = len(a)
        buf = torch.full((off + n * lda,), CANARY, dtype=torch.float64, device="cuda")
        view = buf[off:].view(n, lda)
        view[:, :n] = torch.from_numpy(a).cuda()
        return buf, view

    def around_same(buf, view, n, off):
        return bool((buf[:off] == CANARY).all().item() and (view[:, n:] == CANARY).all().item())

    def factor(a, lda, off):
        """cholesky_decomp1 of a in the given layout: (st, info, the n x n window, the padding still holds CANARY)"""
        n = len(a)
        buf, view = stage(a, lda, off)
        st, info = ctx.cholesky_decomp1(n, buf.data_ptr() + 8 * off, lda)
        ctx.sync()
        return st, info, view.cpu().numpy()[:, :n].copy(), buf, around_same(buf, view, n, off)

    def factor_record(tag, a, lda, off):
        st, info, got, buf, around = factor(a, lda, off)
        l = np.tril(got)
        rec = dict(st=int(st), info=int(info), finite=bool(np.isfinite(l).all()), around_same=around,
                   upper_same=bool(np.array_equal(np.triu(got, 1), np.triu(a, 1))))
        if st == 0 and rec["finite"]:
            rec["be"], rec["cw"] = cache.figures(tag, a, l)
        return rec, l, buf

    kept = {}                                                  # (name, n, layout) -> L, for the scale test
    for name, n in pd_cases(route):
        a, b, xr = load("A", name, n), load("B", name, n), load("XR", name, n)
        ald = a.astype(sr.LD)
        sol = lambda x, q: dict(be=sr.solve_be(ald, x, b[q]), fwd=sr.forward_err(x, xr[q]), finite=bool(np.isfinite(x).all()))
        for lay, lda, off in layouts(n):
            rec, l, buf = factor_record(key(name, n), a, lda, off)
            res["factor"][key(name, n) + "_" + lay] = rec
            if n == 1024 and "riders_1024" not in res["route"]:     # riders of the cholesky_decomp1 just made (test_routes_differ)
                res["route"]["riders_1024"] = int(pkg.lib().gsl_sinterp_hip_debug_chol_riders())
            if name in ("spec_1e4", "scaled_up", "scaled_down"):
                kept[(name, n, lay)] = l
            if rec["st"] == 0:
                d_x = dev(b[0])                                # cholesky_svx on the GPU's own factor
                ctx.cholesky_svx(n, buf.data_ptr() + 8 * off, lda, ptr(d_x))
                ctx.sync()
                res["solve"][key(name, n) + "_" + lay + "_svx"] = [sol(d_x.cpu().numpy(), 0)]
            for nrhs in (1, N_RHS):
                buf, view = stage(a, lda, off)
                d_x = dev(b[:nrhs])
                st, info = ctx.cholesky_factor_solve(n, buf.data_ptr() + 8 * off, lda, ptr(d_x), n, nrhs)
                ctx.sync()
                x = d_x.cpu().numpy()
                res["solve"][key(name, n) + "_" + lay + "_fs%d" % nrhs] = (
                    [dict(st=int(st), info=int(info), around_same=around_same(buf, view, n, off))]
                    + ([sol(x[q], q) for q in range(nrhs)] if st == 0 else []))
        print(route, name, n, "done", flush=True)
    for (name, n, lay), l in kept.items():
        if name != "spec_1e4":
            want = np.ldexp(kept[("spec_1e4", n, lay)], 450 if name == "scaled_up" else -450)
            res["scale"][key(name, n) + "_" + lay] = float(np.abs(l - want).max() / np.abs(want).max())
    for name, n in semidef_cases(route):
        a, good = load("A", name, n), load("A", FOLLOW[n], n)
        for lay, lda, off in layouts(n):
            rec, _, _ = factor_record(key(name, n), a, lda, off)
            rec["follow"], _, _ = factor_record(key(FOLLOW[n], n), good, lda, off)   # same context: flags and abort word reset
            res["semidef"][key(name, n) + "_" + lay] = rec
        print(route, name, n, "done", flush=True)
    if route in LU_ROUTES:
        for kind in sr.LU_KINDS:
            for n in sr.LU_SIZES:
                a = load("LU", kind, n)
                b = lu_rhs(a, kind)
                d_a, d_lu, d_b = dev(a), dev(a), dev(b)
                d_perm = torch.empty(n, dtype=torch.int32, device="cuda")
                ctx.lu_decomp(n, ptr(d_lu), n, ptr(d_perm))
                ctx.sync()
                lu, perm = d_lu.cpu().numpy(), d_perm.cpu().numpy().astype(np.int64)
                rec = dict(finite=bool(np.isfinite(lu).all()), is_perm=bool(np.array_equal(np.sort(perm), np.arange(n))))
                if rec["finite"] and rec["is_perm"]:
                    rec["max_l"] = float(np.abs(np.tril(lu, -1)).max())
                    rec["be"] = sr.lu_be(a, lu, perm)
                    d_x = dev(b)
                    rec["svx_st"] = int(ctx.lu_svx(n, ptr(d_lu), n, ptr(d_perm), ptr(d_x)))
                    ctx.sync()
                    x = d_x.cpu().numpy()
                    rec["solve_be"] = sr.solve_be(a, x, b)
                    # one refinement step from the solution disturbed in its 8th digit, and from the solution itself;
                    # the parent takes a float64 scipy step from the same starts (X0_*.npy) as the yardstick
                    for tag, x0 in (("far", x * (1.0 + 1e-7 * np.cos(np.arange(n)))), ("near", x)):
                        np.save(os.path.join(zoo_dir, "X0_%s_%s_%d_%s.npy" % (route, kind, n, tag)), x0)
                        d_x0, d_work = dev(x0), dev(np.zeros(n))
                        rec["refine_st_" + tag] = int(ctx.lu_refine(n, ptr(d_a), n, ptr(d_lu), n, ptr(d_perm), ptr(d_b), ptr(d_x0), ptr(d_work)))
                        ctx.sync()
                        rec["r0_" + tag] = float(sr.resid_inf(a, x0, b))
                        rec["r1_" + tag] = float(sr.resid_inf(a, d_x0.cpu().numpy(), b))
                res["lu"][key(kind, n)] = rec
            print(route, kind, "done", flush=True)
    # which tile a 512 x 256 x 64 lower update takes in this process (a case of tests/test_gpu_gemm_c256.py): 0 = the
    # 256 x 128 tile, which the dispatch rule does not pick at this size unless GSL_SINTERP_GEMM_CFG=0 reached the library
    d_pa, d_pb, d_pc = dev(np.zeros((512, 64))), dev(np.zeros((256, 64))), dev(np.zeros((512, 256)))
    ctx.gemm_minus(512, 256, 64, ptr(d_pa), 64, ptr(d_pb), 64, 0, ptr(d_pc), 256, 1)
    ctx.sync()
    res["route"]["gemm_probe_cfg"] = int(pkg.lib().gsl_sinterp_hip_debug_gemm_last_cfg())
    cache.save()
    with open(out_path, "w") as f:
        json.dump(res, f)


# ---------------------------------------------------------------- the parent: zoo, LAPACK's figures, the children
def _reference(zoo_dir):
    """writes the zoo as .npy and returns LAPACK's / scipy's figures on the same matrices"""
    import scipy.linalg as sla
    ref = {"factor": {}, "solve": {}, "semidef": {}, "lu": {}, "lu_factor": {}}
    for name, n in pd_cases("default"):
        a = sr.zoo(name, n)
        b = sr.rhs(a, name, N_RHS)
        l = np.linalg.cholesky(a)
        ald = a.astype(sr.LD)
        xr = sr.x_ref(a, b)
        x = sla.cho_solve((l, True), b.T).T
        ref["factor"][key(name, n)] = list(sr.factor_figures(a, l))
        ref["solve"][key(name, n)] = [dict(be=sr.solve_be(ald, x[q], b[q]), fwd=sr.forward_err(x[q], xr[q])) for q in range(N_RHS)]
        for what, arr in (("A", a), ("B", b), ("XR", xr)):
            np.save(os.path.join(zoo_dir, "%s_%s_%d.npy" % (what, name, n)), arr)
    for name, n in SEMIDEF_CASES:
        a = sr.zoo(name, n)
        s = sr.shifted(a)
        ref["semidef"][key(name, n)] = sr.factor_be(s, np.linalg.cholesky(s))
        np.save(os.path.join(zoo_dir, "A_%s_%d.npy" % (name, n)), a)
    for kind in sr.LU_KINDS:
        for n in sr.LU_SIZES:
            a = sr.lu_matrix(kind, n)
            b = lu_rhs(a, kind)
            lu, piv = sla.lu_factor(a)
            perm = np.arange(n)
            for i, p in enumerate(piv):
                perm[[i, p]] = perm[[p, i]]
            ref["lu"][key(kind, n)] = dict(be=sr.lu_be(a, lu, perm), solve_be=sr.solve_be(a, sla.lu_solve((lu, piv), b), b))
            ref["lu_factor"][key(kind, n)] = (a, b, (lu, piv))
            np.save(os.path.join(zoo_dir, "LU_%s_%d.npy" % (kind, n)), a)
    return ref


def _refine_reference(zoo_dir, ref):
    """the long-double residual after ONE float64 scipy refinement step (stability_ref.refine_step) from the very starts
    the children refined from: ref["refine"][route][kind_n] = dict(far=, near=)"""
    ref["refine"] = {}
    for route in LU_ROUTES:
        ref["refine"][route] = {}
        for k, (a, b, lu_piv) in ref["lu_factor"].items():
            paths = {tag: os.path.join(zoo_dir, "X0_%s_%s_%s.npy" % (route, k, tag)) for tag in ("far", "near")}
            if all(os.path.exists(p) for p in paths.values()):  # absent: the factor was not finite, test_lu says so
                ref["refine"][route][k] = {tag: float(sr.resid_inf(a, sr.refine_step(lu_piv, a, np.load(p), b), b))
                                           for tag, p in paths.items()}


def _ratios(ref, fig):
    """every measured figure over LAPACK's, for the record (profiles/stability_ratios.json)"""
    out = {}
    for route, res in fig.items():
        o = out[route] = {"factor_be": {}, "componentwise_eps": {}, "solve_be": {}, "forward": {}, "scale": res["scale"], "lu": {},
                          "semidef": {}, "route": res["route"]}
        for k, rec in res["semidef"].items():
            base = k.rsplit("_", 1)[0]
            n = int(base.rsplit("_", 1)[1])
            fol = rec["follow"]
            o["semidef"][k] = dict(st=rec["st"], info=rec["info"], finite=rec["finite"],
                                   be_over_shifted=rec["be"] / ref["semidef"][base] if "be" in rec else None,
                                   follow=dict(st=fol["st"], info=fol["info"],
                                               factor_be=fol["be"] / ref["factor"][key(FOLLOW[n], n)][0] if "be" in fol else None))
        for k, rec in res["factor"].items():
            base = k.rsplit("_", 1)[0]
            if "be" in rec:
                o["factor_be"][k] = rec["be"] / ref["factor"][base][0]
                o["componentwise_eps"][k] = dict(gpu=rec["cw"], lapack=ref["factor"][base][1])
        for k, recs in res["solve"].items():
            base = k.rsplit("_", 2)[0]
            sols = recs if k.endswith("svx") else recs[1:]
            o["solve_be"][k] = max([s["be"] / ref["solve"][base][q]["be"] for q, s in enumerate(sols)], default=None)
            o["forward"][k] = max([s["fwd"] / max(ref["solve"][base][q]["fwd"], sr.EPS) for q, s in enumerate(sols)], default=None)
        for k, rec in res["lu"].items():
            if "be" in rec:
                yard = ref["refine"][route][k]
                o["lu"][k] = dict(be=rec["be"] / ref["lu"][k]["be"], solve_be=rec["solve_be"] / ref["lu"][k]["solve_be"], max_l=rec["max_l"],
                                  refine={tag: dict(r0=rec["r0_" + tag], r1=rec["r1_" + tag], scipy_r1=yard[tag],
                                                    r1_over_r0=rec["r1_" + tag] / rec["r0_" + tag] if rec["r0_" + tag] else None,
                                                    r1_over_scipy=rec["r1_" + tag] / yard[tag] if yard[tag] else None)
                                          for tag in ("far", "near")})
    return out


def _record(update):
    """with GSL_SINTERP_STABILITY_RECORD=path: adds the top-level entries of `update` to that JSON file"""
    path = os.environ.get("GSL_SINTERP_STABILITY_RECORD")
    if path:
        old = {}
        if os.path.exists(path):
            with open(path) as f:
                old = json.load(f)
        old.update(update)
        with open(path, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    zoo_dir = str(tmp_path_factory.mktemp("stability"))
    ref = _reference(zoo_dir)
    fig = {}
    for route, switch in ROUTES.items():
        env = dict(os.environ)
        for s in SWITCHES:
            env.pop(s, None)
        env.update(switch)
        out = os.path.join(zoo_dir, route + ".json")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", route, zoo_dir, out], cwd=ROOT, env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        assert r.returncode == 0, route + ":\n" + r.stdout[-3000:]     # a child that failed: none is started after it
        with open(out) as f:
            fig[route] = json.load(f)
    _refine_reference(zoo_dir, ref)
    _record(_ratios(ref, fig))
    return ref, fig


def _factor_ok(rec, lapack_be, what):
    assert rec["st"] == 0 and rec["info"] == 0, (what, rec)
    assert rec["finite"], what
    assert rec["upper_same"], what                              # the strict upper triangle still holds the input
    assert rec["around_same"], what                             # and so do the doubles in front of it and right of column n
    print(f"{what}: factor_be {rec['be'] / sr.EPS:.2f} eps = {rec['be'] / lapack_be:.2f} x LAPACK; componentwise {rec['cw']:.1f} eps")
    assert rec["be"] <= M * lapack_be, (what, rec["be"], lapack_be)


@pytest.mark.parametrize("route,name", route_names(sr.PD, pd_cases))
def test_factor(runs, route, name):
    """(a) and the factor half of (c): status 0, finite, input kept above the diagonal, factor_be <= 16 x LAPACK's"""
    ref, fig = runs
    todo = [c for c in pd_cases(route) if c[0] == name]
    for _, n in todo:
        for lay, _, _ in layouts(n):
            _factor_ok(fig[route]["factor"][key(name, n) + "_" + lay], ref["factor"][key(name, n)][0], f"{route} {name} n {n} {lay}")


@pytest.mark.parametrize("route,name", route_names(sr.PD, pd_cases))
def test_solves(runs, route, name):
    """(b) cholesky_svx on the GPU's factor, cholesky_factor_solve with 1 and 5 right-hand sides b = A x*:
    solve_be <= 16 x scipy cho_solve's, forward error <= 16 x max(LAPACK's, eps), both against x_ref"""
    ref, fig = runs
    for _, n in [c for c in pd_cases(route) if c[0] == name]:
        want = ref["solve"][key(name, n)]
        for lay, _, _ in layouts(n):
            for call, nrhs in (("svx", 1), ("fs1", 1), ("fs%d" % N_RHS, N_RHS)):
                recs = fig[route]["solve"][key(name, n) + "_" + lay + "_" + call]
                if call != "svx":
                    assert recs[0] == dict(st=0, info=0, around_same=True), (route, name, n, lay, call, recs[0])
                    recs = recs[1:]
                assert len(recs) == nrhs
                for q, s in enumerate(recs):
                    what = f"{route} {name} n {n} {lay} {call} rhs {q}"
                    print(f"{what}: solve_be {s['be'] / want[q]['be']:.2f} x, forward {s['fwd'] / max(want[q]['fwd'], sr.EPS):.2f} x "
                          f"({s['fwd']:.2e})")
                    assert s["finite"], what
                    assert s["be"] <= M * want[q]["be"], (what, s["be"], want[q]["be"])
                    assert s["fwd"] <= M * max(want[q]["fwd"], sr.EPS), (what, s["fwd"], want[q]["fwd"])


@pytest.mark.parametrize("route", list(ROUTES)[:-1])
def test_scale(runs, route):
    """(c) the factor of 2^+-900 A is 2^+-450 x the GPU's own factor of A to 1e-13: power-of-two scaling is exact away from
    over- and underflow; a few ulp are allowed should the rsq seed not be scale-exact"""
    _, fig = runs
    got = fig[route]["scale"]
    assert len(got) == 2 * 2 * len(sr.SIZES[:-1])
    for k, rel in got.items():
        print(route, k, rel)
        assert rel <= 1e-13, (route, k, rel)


@pytest.mark.parametrize("route,name", route_names(sr.SEMIDEF, semidef_cases))
def test_semidefinite(runs, route, name, pkg):
    """(d) exactly one of: GSL_EDOM with 1 <= info <= n; or status 0 with a finite factor whose factor_be is within
    16 x LAPACK's on A + 16 n eps max a_ii I.  Never status 0 with NaN or Inf in L.  The good matrix factored next on the
    same context passes (a)."""
    ref, fig = runs
    for _, n in [c for c in semidef_cases(route) if c[0] == name]:
        for lay, _, _ in layouts(n):
            rec = fig[route]["semidef"][key(name, n) + "_" + lay]
            what = f"{route} {name} n {n} {lay}"
            print(what, {k: v for k, v in rec.items() if k != "follow"})
            assert rec["around_same"], what
            if rec["st"] == 0:
                assert rec["finite"], what
                assert rec["info"] == 0, what
                assert rec["be"] <= M * ref["semidef"][key(name, n)], (what, rec["be"], ref["semidef"][key(name, n)])
            else:
                assert rec["st"] == pkg.capi.GSL_EDOM and 1 <= rec["info"] <= n, (what, rec)
            _factor_ok(rec["follow"], ref["factor"][key(FOLLOW[n], n)][0], what + " then " + FOLLOW[n])


@pytest.mark.parametrize("kind", sr.LU_KINDS)
@pytest.mark.parametrize("route", LU_ROUTES)
def test_lu(runs, route, kind):
    """(e) permutations are not compared (near-ties may fall either way): perm is a permutation, max |L_ij| <= 1 (the
    partial-pivoting invariant), max |A[perm] - L U| / max |A| and solve_be <= 16 x scipy's.

    lu_refine, one step from two starts, each held to 16 x the long-double residual that ONE float64 scipy refinement
    step (stability_ref.refine_step: the same formula on scipy's lu_factor) leaves from the very same start:
      far   lu_svx's solution disturbed in its 8th digit (far above the rounding floor): the step must not
            increase the residual AND must reach the rounding floor, which is where the scipy step lands;
      near  lu_svx's own solution.  Here "does not increase" is no property of a correct step: lu_refine forms A x - b
            in float64 (linalg_extra.hip), so at the floor the new residual is set by the rounding of the last solve,
            for LAPACK as well -- a float64 scipy step from scipy's own solution grows the residual 1.21 x on svd_1e12
            at n = 33.  So the yardstick is the scipy step from this start, not the start's own residual."""
    ref, fig = runs
    for n in sr.LU_SIZES:
        rec, want, what = fig[route]["lu"][key(kind, n)], ref["lu"][key(kind, n)], f"{route} {kind} n {n}"
        assert rec["finite"] and rec["is_perm"], what
        yard = ref["refine"][route][key(kind, n)]
        print(f"{what}: max|L| {rec['max_l']}, lu_be {rec['be'] / want['be']:.2f} x, solve_be {rec['solve_be'] / want['solve_be']:.2f} x, "
              f"refine far {rec['r0_far']:.2e} -> {rec['r1_far']:.2e} (scipy {yard['far']:.2e}), "
              f"near {rec['r0_near']:.2e} -> {rec['r1_near']:.2e} (scipy {yard['near']:.2e})")
        assert rec["max_l"] <= 1.0, (what, rec["max_l"])
        assert rec["be"] <= M * want["be"], (what, rec["be"], want["be"])
        assert rec["svx_st"] == 0 and rec["solve_be"] <= M * want["solve_be"], (what, rec["solve_be"], want["solve_be"])
        assert rec["refine_st_far"] == 0 and rec["refine_st_near"] == 0
        assert rec["r1_far"] <= rec["r0_far"], (what, rec["r0_far"], rec["r1_far"])
        assert rec["r1_far"] <= M * yard["far"], (what, rec["r1_far"], yard["far"])
        assert rec["r1_near"] <= M * yard["near"], (what, rec["r1_near"], yard["near"])


@pytest.mark.parametrize("route", list(ROUTES))
def test_routes_differ(runs, route):
    """the switches that leave a trace did reach the library in their child, and in no other: a 512 x 256 x 64 lower
    update takes the 256 x 128 tile (gsl_sinterp_hip_debug_gemm_last_cfg() == 0) under GSL_SINTERP_GEMM_CFG=0 only; the
    first cholesky_decomp1 at n = 1024 has n / 128 - 1 riders by default and none with NO_DIAG_RIDER or NO_PANEL128
    (tests/test_gpu_chol_rider.py).  TRSM_RF, NO_FOLD and NO_DATAFLOW_TRSV leave no counter to read."""
    _, fig = runs
    got = fig[route]["route"]
    print(route, got)
    assert (got["gemm_probe_cfg"] == 0) == (route == "gemm_cfg0"), got
    if route == "default":
        assert got["riders_1024"] == 1024 // 128 - 1, got
    if route in ("no_rider", "no_panel128"):
        assert got["riders_1024"] == 0, got


# ---------------------------------------------------------------- (f) two consumers of the inverse
@pytest.fixture(scope="module")
def krige_reference():
    return _krige_reference()


def _krige_reference():
    n = N_KRIGE
    x = sr.gauss_points(n, 2, "g2")                            # gauss2d_a: its points, shape and nugget
    eps, nugget = 0.25 * 2.0 * n ** 0.5, 1e-8
    y = np.random.default_rng(7).random((M_KRIGE, 2))
    f = np.sin(3.0 * x[:, 0]) + np.cos(2.0 * x[:, 1]) + x[:, 0] * x[:, 1]
    cov = lambda p, q: np.exp(-eps * eps * ((p[:, None, :] - q[None, :, :]) ** 2).sum(axis=2))
    k, kt = cov(x, x) + nugget * np.eye(n), cov(x, y)
    exact = sr.kriging_formulas(k, kt, f, True)
    fp64 = sr.kriging_formulas(k, kt, f, False)
    return x, y, f, eps, nugget, exact, fp64


def _rel(got, want):
    return float(np.abs(np.asarray(got, dtype=sr.LD) - want).max() / np.abs(want).max())


def _krige(pkg, ref, loo, variance):
    x, y, f, eps, nugget = ref[:5]
    s = pkg.Sinterp("kriging", 2, len(x), 0)
    assert s.set_nugget(nugget) == 0 and s.set_shape(eps) == 0
    if variance:
        assert s.set_variance(1) == 0
    if loo:
        assert s.set_loo(1) == 0
    assert s.init(np.ascontiguousarray(x), f.copy()) == 0 and s.route() == 7
    return s


def test_kriging_variance_at_1e9(pkg, krige_reference):
    """eval_variance_many at 500 targets, cond(K) ~ 1e9: the error against the longdouble evaluation of the formula is
    within 16 x that of its float64 LAPACK evaluation; variances finite and >= 0.  Absolute errors: the sill is 1."""
    x, y, f, eps, nugget, exact, fp64 = krige_reference
    s = _krige(pkg, krige_reference, loo=False, variance=True)
    st, got = s.eval_variance_many(np.ascontiguousarray(y))
    assert st == 0 and got.shape == (M_KRIGE,)
    err, yard = float(np.abs(got.astype(sr.LD) - exact[0]).max()), float(np.abs(fp64[0].astype(sr.LD) - exact[0]).max())
    print(f"variance: gpu {err:.3e}, float64 LAPACK {yard:.3e}, min {got.min():.3e}, exact min {float(exact[0].min()):.3e}")
    _record({"kriging_variance": dict(gpu_err=err, lapack_err=yard, ratio=err / yard, gpu_min=float(got.min()))})
    assert np.isfinite(got).all() and (got >= 0.0).all()
    assert err <= M * yard


def test_loo_at_1e9(pkg, krige_reference):
    """loo_residuals / loo_variance on the same model: errors relative to the largest exact value, within 16 x those of
    the float64 LAPACK evaluation"""
    x, y, f, eps, nugget, exact, fp64 = krige_reference
    s = _krige(pkg, krige_reference, loo=True, variance=False)
    st, e = s.loo_residuals()
    st2, v = s.loo_variance()
    assert st == 0 and st2 == 0
    e = np.asarray(e).reshape(-1)
    for what, got, i in (("residuals", e, 1), ("variances", v, 2)):
        err, yard = _rel(got, exact[i]), _rel(fp64[i], exact[i])
        print(f"loo {what}: gpu {err:.3e}, float64 LAPACK {yard:.3e}")
        _record({"loo_" + what: dict(gpu_err=err, lapack_err=yard, ratio=err / yard, gpu_min=float(np.min(got)))})
        assert np.isfinite(got).all()
        assert err <= M * yard, (what, err, yard)
    assert (v >= 0.0).all()


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1] == "child":
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        _child(sys.argv[2], sys.argv[3], sys.argv[4])
