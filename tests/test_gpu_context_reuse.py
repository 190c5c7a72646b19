"""-m gpu: one context, interleaved calls.  The factorisations and sweeps are captured into hipGraphs and replayed when
a slot's key matches (four slots per context), and some state is kept per context or per device (workspaces, the
barycentric jump table and leaf-walk locator, the exclusive-section chain).  Each step below changes ONE argument that
shares a slot or a cache with the step before it; every result must equal the oracle at the dense tests' tolerance and
the bits of the same call made alone on a fresh context."""
import numpy as np
import pytest
import torch

from gpu_util import CANARY, Canaried, bits, dev, ptr

pytestmark = pytest.mark.gpu
TOL = 1e-10


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def spd(n, seed):
    rng = np.random.default_rng(seed)
    m = rng.random((n, n))
    return np.tril(m) + np.tril(m, -1).T + 10.0 * n * np.eye(n)


def test_factor_solve_graph_key_separates_rhs_pointer_count_and_stride(pkg, orc):
    """Slot 0 with the forward substitution folded in: the right-hand sides' pointer, count and stride are baked into
    the captured kernels.  (R, 5 columns) then (R + 1 element, 1 column), ... on one matrix buffer: every step is a
    different graph.  The buffer of R has room for 5 columns at R + 1, so even a wrong replay stays inside it."""
    n = 256
    a = spd(n, 5)
    st_o, want = orc.cholesky_decomp1(a)
    ctx = pkg.HipContext.on_torch_stream(0)
    A = Canaried(a)
    rng = np.random.default_rng(17)
    for ldx in (256, 260):
        R = Canaried(np.zeros((5, ldx)), ld=ldx, off=0, tail=ldx + 64)     # R + 1 element .. + 5 ldx fits
        for off, nrhs in ((0, 5), (1, 1), (0, 1), (1, 5)):
            B = rng.standard_normal((nrhs, n))
            A.set(a)
            R.buf.fill_(CANARY)
            view = R.buf.view(torch.float64)[off:off + nrhs * ldx].view(nrhs, ldx)
            view[:, :n].copy_(torch.from_numpy(B))
            st, info = ctx.cholesky_factor_solve(n, A.ptr, n, R.ptr + 8 * off, ldx, nrhs)
            assert st == 0 and info == 0
            h = R.buf.cpu().numpy()
            x = h.view(np.float64)[off:off + nrhs * ldx].reshape(nrhs, ldx)[:, :n]
            mask = np.ones(h.size, dtype=bool)
            mask[(off + np.arange(nrhs)[:, None] * ldx + np.arange(n)[None, :]).ravel()] = False
            assert (h[mask] == CANARY).all(), (ldx, off, nrhs)          # nothing written outside this call's columns
            for q in range(nrhs):
                xo = orc.cholesky_solve(want, B[q])
                assert np.abs(x[q] - xo).max() <= 1e-11 * np.abs(xo).max(), (ldx, off, nrhs, q)
            # the same call alone on a fresh context: the same bits
            fctx = pkg.HipContext.on_torch_stream(0)
            FA, FX = Canaried(a), Canaried(B, ld=ldx, off=off)
            st, info = fctx.cholesky_factor_solve(n, FA.ptr, n, FX.ptr, ldx, nrhs)
            assert st == 0 and np.array_equal(bits(FX.get().reshape(nrhs, n)), bits(x)), (ldx, off, nrhs)
            fctx.close()


def test_slot0_shared_by_decomp1_and_gaussian_solve(pkg, orc):
    """cholesky_decomp1 and the Gaussian rbf_solve factor on slot 0 with the same buffer and n (they differ in the
    symmetric-input bit and the folded right-hand side); then n = 2048 -> 512 -> 2048 regrows and reuses the workspace"""
    dim = 2

    def problem(n):
        x = orc.synth_centres(n, dim)
        return x, orc.synth_response(x), orc.gaussian_eps(n, dim)

    def decomp(ctx, buf, a, n):
        buf[: n * n].copy_(torch.from_numpy(a.ravel()))
        st, info = ctx.cholesky_decomp1(n, ptr(buf), n)
        assert st == 0 and info == 0
        ctx.sync()
        return buf[: n * n].cpu().numpy().reshape(n, n)

    def solve(ctx, buf, x, f, eps, n):
        d_x, d_w = dev(x), dev(f)
        st, route = ctx.rbf_solve(0, eps, ptr(d_x), n, dim, dim, ptr(buf), n, ptr(d_w))
        assert st == 0 and route == 1
        return d_w.cpu().numpy()

    alone = {}
    for n in (512, 2048):
        x, f, eps = problem(n)
        a = spd(n, n)
        c = pkg.HipContext.on_torch_stream(0)
        b1 = torch.empty(n * n, dtype=torch.float64, device="cuda")
        alone[("decomp", n)] = decomp(c, b1, a, n)
        c.close()
        c = pkg.HipContext.on_torch_stream(0)
        b2 = torch.empty(n * n, dtype=torch.float64, device="cuda")
        alone[("solve", n)] = solve(c, b2, x, f, eps, n)
        c.close()
    x, f, eps = problem(512)
    st_o, llt_o = orc.cholesky_decomp1(spd(512, 512))
    assert np.abs(np.tril(alone[("decomp", 512)]) - np.tril(llt_o)).max() <= 1e-12 * np.abs(np.tril(llt_o)).max()
    assert relerr(alone[("solve", 512)], orc.rbf_solve(0, eps, x, f)) < TOL
    x2, f2, eps2 = problem(2048)
    phi = torch.from_numpy(orc.rbf_fill(0, eps2, x2)).cuda()
    w2 = torch.from_numpy(alone[("solve", 2048)]).cuda()
    assert float((phi @ w2 - torch.from_numpy(f2).cuda()).abs().max()) < 1e-9 * np.abs(f2).max()

    ctx = pkg.HipContext.on_torch_stream(0)
    buf = torch.empty(2048 * 2048, dtype=torch.float64, device="cuda")
    for n in (512, 512, 2048, 512, 2048):
        x, f, eps = problem(n)
        a = spd(n, n)
        for what in ("decomp", "solve", "decomp", "solve"):
            got = decomp(ctx, buf, a, n) if what == "decomp" else solve(ctx, buf, x, f, eps, n)
            assert np.array_equal(bits(got), bits(alone[(what, n)])), (n, what)


def test_sweep_slots_shared_across_solvers(pkg, orc):
    """Slots 2 / 3 (forward / backward sweeps) are used by cholesky_svx, lu_svx and pcholesky_svx at the same n, with
    different matrices, unit flags, modes and right-hand-side buffers"""
    n = 512
    a = spd(n, 9)
    b = np.sin(np.arange(n) * 0.37) + 2.0

    def factors(ctx):
        llt, lu, ldlt = dev(a), dev(a), dev(a)
        p_lu = torch.empty(n, dtype=torch.int32, device="cuda")
        p_ld = torch.empty(n, dtype=torch.int32, device="cuda")
        st, info = ctx.cholesky_decomp1(n, ptr(llt), n)
        assert st == 0
        ctx.lu_decomp(n, ptr(lu), n, ptr(p_lu))
        ctx.pcholesky_decomp(n, ptr(ldlt), n, ptr(p_ld))
        ctx.sync()
        return llt, lu, p_lu, ldlt, p_ld

    def run(ctx, F, which, d_x):
        llt, lu, p_lu, ldlt, p_ld = F
        d_x.copy_(torch.from_numpy(b))
        if which == "chol":
            ctx.cholesky_svx(n, ptr(llt), n, ptr(d_x))
        elif which == "lu":
            assert ctx.lu_svx(n, ptr(lu), n, ptr(p_lu), ptr(d_x)) == 0
        else:
            ctx.pcholesky_svx(n, ptr(ldlt), n, ptr(p_ld), ptr(d_x))
        ctx.sync()
        return d_x.cpu().numpy()

    alone = {}
    for which in ("chol", "lu", "pchol"):
        c = pkg.HipContext.on_torch_stream(0)
        alone[which] = run(c, factors(c), which, torch.empty(n, dtype=torch.float64, device="cuda"))
        c.close()
    want = {"chol": orc.cholesky_solve(orc.cholesky_decomp1(a)[1], b)}
    lu_o, perm_o, _ = orc.lu_decomp(a)
    want["lu"] = orc.lu_solve(lu_o, perm_o, b)[1]
    _, ldlt_o, pp_o = orc.pcholesky_decomp(a)
    want["pchol"] = orc.pcholesky_solve(ldlt_o, pp_o, b)
    tol = {"chol": 1e-11, "lu": 1e-7, "pchol": 1e-10}
    for which in alone:
        assert np.abs(alone[which] - want[which]).max() <= tol[which] * np.abs(want[which]).max(), which

    ctx = pkg.HipContext.on_torch_stream(0)
    F = factors(ctx)
    X = [torch.empty(n, dtype=torch.float64, device="cuda") for _ in range(2)]
    seq = [("chol", 0), ("lu", 0), ("pchol", 1), ("chol", 1), ("lu", 1), ("pchol", 0), ("chol", 0), ("lu", 0), ("chol", 1)]
    for which, k in seq:
        got = run(ctx, F, which, X[k])
        assert np.array_equal(bits(got), bits(alone[which])), (which, k)


def test_lu_slot_with_two_permutation_buffers_and_strides(pkg, orc):
    """Slot 1: the LU graph bakes the matrix, its stride and the pivot buffer"""
    n = 384
    rng = np.random.default_rng(n)
    a = rng.standard_normal((n, n)) + np.diag(np.linspace(1, 10, n))
    b = np.arange(1.0, n + 1.0)
    lu_o, perm_o, _ = orc.lu_decomp(a)
    x_o = orc.lu_solve(lu_o, perm_o, b)[1]

    def one(ctx, A, lda, d_perm):
        A.set(a)
        ctx.lu_decomp(n, A.ptr, lda, ptr(d_perm))
        X = Canaried(b)
        assert ctx.lu_svx(n, A.ptr, lda, ptr(d_perm), X.ptr) == 0
        ctx.sync()
        return A.get(), d_perm.cpu().numpy().copy(), X.get()

    ref = {}
    for lda in (n, n + 1):                                       # the same call alone on a fresh context, per stride
        c = pkg.HipContext.on_torch_stream(0)
        ref[lda] = one(c, Canaried(a, ld=lda), lda, torch.empty(n, dtype=torch.int32, device="cuda"))
        c.close()
        assert np.array_equal(ref[lda][1].astype(np.uintp), perm_o)
        assert np.abs(ref[lda][0] - lu_o).max() <= 1e-9 * np.abs(lu_o).max()
        assert np.abs(ref[lda][2] - x_o).max() <= 1e-7 * np.abs(x_o).max()

    ctx = pkg.HipContext.on_torch_stream(0)
    A = {n: Canaried(a), n + 1: Canaried(a, ld=n + 1)}
    P = [torch.full((n,), -1, dtype=torch.int32, device="cuda") for _ in range(2)]
    for lda, k in ((n, 0), (n, 1), (n + 1, 1), (n + 1, 0), (n, 0), (n + 1, 1)):
        P[1 - k].fill_(-1)                                       # the other pivot buffer must not be written
        got = one(ctx, A[lda], lda, P[k])
        assert np.array_equal(bits(got[0]), bits(ref[lda][0])), (lda, k)
        assert np.array_equal(got[1], ref[lda][1]) and np.array_equal(bits(got[2]), bits(ref[lda][2])), (lda, k)
        assert (P[1 - k].cpu().numpy() == -1).all() and A[lda].padding_intact()


def test_facade_objects_interleaved_on_one_device(pkg, orc):
    """Gaussian RBF, affine thin-plate spline and kriging objects (each with its own context) interleaved: the state
    shared per device (exclusive-section chain, kernel attributes) must not change a bit"""
    n, dim, m = 512, 2, 5000
    x = orc.synth_centres(n, dim)
    f = orc.synth_response(x) + 1.0
    y = orc.synth_targets(0, m, dim)
    kinds = ("gaussian", "tps_affine", "kriging")

    def make(kind):
        s = pkg.Sinterp(kind, dim, n, 0)
        if kind == "kriging":
            assert s.set_nugget(1e-3) == 0
        return s

    alone = {}
    for kind in kinds:
        s = make(kind)
        assert s.init(x, f) == 0
        st, v, _ = s.eval_many(y)
        assert st == 0
        alone[kind] = v
        s.close()
    eps = orc.gaussian_eps(n, dim)
    assert relerr(alone["gaussian"], orc.rbf_eval(0, eps, x, orc.rbf_solve(0, eps, x, f), y)) < TOL
    w, c = orc.rbf_solve_affine(1, 0.0, x, f)
    assert relerr(alone["tps_affine"], orc.rbf_eval_affine(1, 0.0, c, x, w, y)) < TOL
    w, mu = orc.krige_solve(0, eps, 1e-3, x, f)
    assert relerr(alone["kriging"], orc.krige_eval(0, eps, mu, x, w, y)) < TOL

    objs = {k: make(k) for k in kinds}
    steps = [("init", "gaussian"), ("init", "tps_affine"), ("eval", "gaussian"), ("init", "kriging"), ("eval", "tps_affine"),
             ("eval", "kriging"), ("init", "gaussian"), ("eval", "kriging"), ("eval", "gaussian"), ("init", "tps_affine"),
             ("eval", "tps_affine")]
    for what, kind in steps:
        s = objs[kind]
        if what == "init":
            assert s.init(x, f) == 0
        else:
            st, v, _ = s.eval_many(y)
            assert st == 0 and np.array_equal(bits(v), bits(alone[kind])), kind


def test_two_simplex_trees_packed_on_one_context(pkg, orc):
    """The jump table and the leaf-walk locator of a context belong to the LAST tree packed on it: batches that
    alternate between two packed trees must still give the oracle's leaves and bits"""
    ctx = pkg.HipContext.on_torch_stream(0)
    trees = []
    for n, scale, off in ((1500, np.array([1.0, 1.0]), np.array([0.0, 0.0])), (2200, np.array([3.0, 0.5]), np.array([-1.0, 10.0]))):
        x = orc.synth_centres(n, 2) * scale + off
        f = orc.synth_response(x)
        t = pkg.SimplexTree(2, n)
        assert t.init(x, flags=0, rng=pkg.capi.Rng(0)) == 0
        o = orc.Tree(2, n)
        assert o.init(x, flags=0, seed=0) == 0
        types, pidx, links = t.arrays()
        sh = t.shuffle()
        nn = t.n_nodes
        assert nn >= 2048
        d = dict(t=t, o=o, x=x, f=f, nn=nn, geom=t.geom(), scale=scale, off=off,
                 arrays=(dev(types), dev(pidx), dev(links), dev(x[sh]), dev(f[sh])),
                 rec=torch.empty(nn * 64, dtype=torch.uint8, device="cuda"),
                 tab=torch.empty(nn * 32, dtype=torch.uint8, device="cuda"))
        d_type, d_pidx, d_links, d_pts, d_resp = d["arrays"]
        ctx.tree_pack(nn, ptr(d_type), ptr(d_pidx), ptr(d_links), n, ptr(d_pts), d["geom"], ptr(d["rec"]))
        ctx.tree_bind(nn, ptr(d_pidx), n, ptr(d_resp), ptr(d["tab"]))
        trees.append(d)
    for step, (k, m) in enumerate(((0, 8192), (1, 6000), (0, 5000), (1, 9000), (0, 4096), (1, 300))):
        d = trees[k]
        y = orc.synth_targets(step, m, 2) * d["scale"] + d["off"]
        d_y = dev(y)
        d_v = torch.empty(m, dtype=torch.float64, device="cuda")
        d_l = torch.empty(m, dtype=torch.int32, device="cuda")
        outside = ctx.bary_eval(d["nn"], ptr(d["rec"]), ptr(d["tab"]), d["geom"][8:10], ptr(d_y), m, 2, ptr(d_v), ptr(d_l),
                                count_outside=True)
        ovals, oleaf = d["o"].eval_many(d["x"], d["f"], y)
        assert outside == 0
        assert np.array_equal(d_l.cpu().numpy(), oleaf), (step, k)
        assert np.array_equal(bits(d_v.cpu().numpy()), bits(ovals)), (step, k)
