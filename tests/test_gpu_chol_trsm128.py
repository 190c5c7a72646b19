"""-m gpu: chol_trsm128_kernel, the 64-row strip row solve below a 128-wide diagonal block, at the smallest shapes.

By default the strip kernel serves only panels with more than 4096 rows below them, so only the full-size tests reach it.
The developer override GSL_SINTERP_TRSM_RF=64 forces it for every 128-wide leaf; it is read once per process, so the
forced route runs in a child interpreter (this file, run as a script, is that child) and the parent runs the same cases
on the default route, chol_trsm16_kernel<1> at these sizes.  Both solve the same rows against the same diagonal block, so
they must agree to rounding."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from test_gpu_chol_rider import layouts, spd

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# rows below the 128-wide leaves: 384 -> 256, 128, 0 (whole workgroups of 64 rows); 424 -> 296, 168, 40 (partial last
# workgroups: the load clamp and the store guard, one launch of a single, partly filled workgroup; 424 is no multiple of
# 128, so the leaves write their diagonal blocks back through the side buffer)
DECOMP_SIZES = [384, 424]
SOLVE_N = 384                      # a multiple of 128: the forward substitution folds into the row solves
SOLVE_NRHS = [1, 5]                # one and all three load passes of the staged right-hand sides


def rhs(nrhs):
    return np.random.default_rng(100 * SOLVE_N + nrhs).random((nrhs, SOLVE_N))


def device_matrix(a, lda, off):
    n = a.shape[0]
    buf = torch.zeros(off + n * lda, dtype=torch.float64, device="cuda")
    view = buf[off:].view(n, lda)
    view[:, :n] = torch.from_numpy(a).cuda()
    return buf, view


def run_cases(pkg, out):
    """every case on the route this process was started with; the whole matrices and the solutions as .npy files in `out`"""
    ctx = pkg.HipContext.on_torch_stream(0)
    for n in DECOMP_SIZES:
        a = spd(n, n)
        for name, lda, off in layouts(n):
            buf, view = device_matrix(a, lda, off)
            st, info = ctx.cholesky_decomp1(n, buf.data_ptr() + 8 * off, lda)
            assert st == 0 and info == 0, (n, name, st, info)
            np.save(os.path.join(out, f"A_{n}_{name}.npy"), view.cpu().numpy()[:, :n])
    a = spd(SOLVE_N, SOLVE_N)
    for nrhs, (name, lda, off) in zip(SOLVE_NRHS, layouts(SOLVE_N)):
        buf, view = device_matrix(a, lda, off)
        d_x = torch.from_numpy(rhs(nrhs)).cuda()
        st, info = ctx.cholesky_factor_solve(SOLVE_N, buf.data_ptr() + 8 * off, lda, d_x.data_ptr(), SOLVE_N, nrhs)
        assert st == 0 and info == 0, (nrhs, st, info)
        np.save(os.path.join(out, f"FA_{nrhs}.npy"), view.cpu().numpy()[:, :SOLVE_N])
        np.save(os.path.join(out, f"FX_{nrhs}.npy"), d_x.cpu().numpy())


def forced_child(out):
    env = dict(os.environ)
    env["GSL_SINTERP_TRSM_RF"] = "64"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]


@pytest.fixture(scope="module")
def routes(pkg):
    """directories of results: the default route, and the forced strip kernel twice"""
    with tempfile.TemporaryDirectory() as tmp:
        dirs = [os.path.join(tmp, d) for d in ("default", "strip", "strip_again")]
        for d in dirs:
            os.makedirs(d)
        assert not os.environ.get("GSL_SINTERP_TRSM_RF"), "this module runs the default route in the parent"
        run_cases(pkg, dirs[0])
        forced_child(dirs[1])
        forced_child(dirs[2])
        yield dirs


def matrices():
    """(file stem, input matrix) of every factorisation of run_cases"""
    return [(f"A_{n}_{name}", spd(n, n)) for n in DECOMP_SIZES for name, _, _ in layouts(n)] + \
           [(f"FA_{nrhs}", spd(SOLVE_N, SOLVE_N)) for nrhs in SOLVE_NRHS]


def test_strip_kernel_factor_agrees_with_default_route(routes, orc):
    """lower triangles of the strip kernel and of the default route within 1e-13 max|L| of each other and both within
    1e-12 max|L| of the oracle (the tolerances of test_gpu_chol_rider.py for two routes of one factorisation); the strict
    upper triangle is the input, bit for bit (cholesky.c:103)"""
    default, strip, _ = routes
    want = {}
    for nm, a in matrices():
        n = a.shape[0]
        if n not in want:
            st, llt = orc.cholesky_decomp1(a)
            assert st == 0
            want[n] = np.tril(llt)
        got_d, got_s = np.load(os.path.join(default, nm + ".npy")), np.load(os.path.join(strip, nm + ".npy"))
        for got in (got_d, got_s):
            assert np.array_equal(np.triu(got, 1), np.triu(a, 1)), nm
        l_d, l_s = np.tril(got_d), np.tril(got_s)
        scale = np.abs(l_d).max()
        d = np.abs(l_s - l_d).max()
        e_d, e_s = np.abs(l_d - want[n]).max(), np.abs(l_s - want[n]).max()
        print(f"{nm}: strip vs default {d / scale:.3e}, vs oracle {e_s / scale:.3e} (default {e_d / scale:.3e})")
        assert d <= 1e-13 * scale, nm
        assert e_d <= 1e-12 * np.abs(want[n]).max(), nm
        assert e_s <= 1e-12 * np.abs(want[n]).max(), nm


def test_strip_kernel_folded_solve_agrees(routes, orc):
    """the forward substitution folded into the strip kernel (f -= X y while X is in LDS): solutions within 1e-12 of the
    default route's, relative to the largest entry, and within 1e-11 of the oracle's"""
    default, strip, _ = routes
    st, llt = orc.cholesky_decomp1(spd(SOLVE_N, SOLVE_N))
    assert st == 0
    for nrhs in SOLVE_NRHS:
        x_d, x_s = np.load(os.path.join(default, f"FX_{nrhs}.npy")), np.load(os.path.join(strip, f"FX_{nrhs}.npy"))
        d = np.abs(x_s - x_d).max() / np.abs(x_d).max()
        print(f"nrhs {nrhs}: strip vs default {d:.3e}")
        assert d <= 1e-12, nrhs
        b = rhs(nrhs)
        for q in range(nrhs):
            xo = orc.cholesky_solve(llt, b[q])
            for x in (x_d, x_s):
                assert np.abs(x[q] - xo).max() <= 1e-11 * np.abs(xo).max(), (nrhs, q)


def test_strip_kernel_is_deterministic(routes):
    """two processes on the forced route give the same bits: every file, factors and solutions"""
    _, strip, again = routes
    names = sorted(os.listdir(strip))
    assert names == sorted(os.listdir(again)) and len(names) == len(matrices()) + len(SOLVE_NRHS)
    for nm in names:
        assert np.array_equal(np.load(os.path.join(strip, nm)), np.load(os.path.join(again, nm))), nm


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import __graft_entry__ as g
    run_cases(g.load_package(), sys.argv[1])
