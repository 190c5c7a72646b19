"""-m gpu: the diagonal-block rider of the Cholesky trailing updates.

The update in front of a 128-wide leaf carries one extra workgroup that factors the leaf's diagonal block as soon as the
tiles covering it are stored; GSL_SINTERP_NO_DIAG_RIDER=1 restores the launch per diagonal block.  Both routes run the
same device function on the same block, so they must agree; the switch is read once per process, so the "off" route runs
in a child interpreter (this file, run as a script, is that child)."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [256, 384, 1024, 2176, 4096]
EDOM_CASES = [(1024, 3 * 128 + 17), (1024, 17)]       # a column inside a rider-factored block, and one in panel 0


def spd(n, seed):
    rng = np.random.default_rng(seed)
    m = rng.random((n, n))
    return np.tril(m) + np.tril(m, -1).T + 10.0 * n * np.eye(n)      # linalg/test_common.c:68-88


def layouts(n):
    """(name, lda, offset in doubles): packed, and lda > n behind a 16-byte offset"""
    return [("packed", n, 0), ("strided", n + 6, 2)]


def run_cases(pkg, out):
    """every case of the agreement test on the route this process was started with; results as .npy files in `out`"""
    import torch
    ctx = pkg.HipContext.on_torch_stream(0)
    riders = {}
    for n in SIZES:
        a = spd(n, n)
        for name, lda, off in layouts(n):
            buf = torch.zeros(off + n * lda, dtype=torch.float64, device="cuda")
            view = buf[off:].view(n, lda)
            view[:, :n] = torch.from_numpy(a).cuda()
            st, info = ctx.cholesky_decomp1(n, buf.data_ptr() + 8 * off, lda)
            assert st == 0 and info == 0, (n, name, st, info)
            riders[(n, name)] = pkg.lib().gsl_sinterp_hip_debug_chol_riders()
            got = view.cpu().numpy()[:, :n]
            assert np.array_equal(np.triu(got, 1), np.triu(a, 1))     # cholesky.c:103: original kept above the diagonal
            np.save(os.path.join(out, f"L_{n}_{name}.npy"), np.tril(got))
        for nrhs in range(1, 6):
            name, lda, off = layouts(n)[nrhs % 2]
            buf = torch.zeros(off + n * lda, dtype=torch.float64, device="cuda")
            view = buf[off:].view(n, lda)
            view[:, :n] = torch.from_numpy(a).cuda()
            b = np.random.default_rng(100 * n + nrhs).random((nrhs, n))
            d_x = torch.from_numpy(b).cuda()
            st, info = ctx.cholesky_factor_solve(n, buf.data_ptr() + 8 * off, lda, d_x.data_ptr(), n, nrhs)
            assert st == 0 and info == 0, (n, nrhs, st, info)
            np.save(os.path.join(out, f"FL_{n}_{nrhs}.npy"), np.tril(view.cpu().numpy()[:, :n]))
            np.save(os.path.join(out, f"FX_{n}_{nrhs}.npy"), d_x.cpu().numpy())
    for n, col in EDOM_CASES:
        a = spd(n, 7)
        a[col, col] = -1.0
        d_a = torch.from_numpy(a).cuda()
        st, info = ctx.cholesky_decomp1(n, d_a.data_ptr(), n)
        np.save(os.path.join(out, f"EDOM_{n}_{col}.npy"), np.array([st, info]))
    np.save(os.path.join(out, "riders.npy"), np.array([[n, 0 if name == "packed" else 1, r] for (n, name), r in riders.items()]))


def child(switch_value, out):
    env = dict(os.environ)
    env["GSL_SINTERP_NO_DIAG_RIDER"] = switch_value
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]


@pytest.fixture(scope="module")
def both_routes(pkg):
    with tempfile.TemporaryDirectory() as tmp:
        on, off = os.path.join(tmp, "on"), os.path.join(tmp, "off")
        os.makedirs(on)
        os.makedirs(off)
        assert os.environ.get("GSL_SINTERP_NO_DIAG_RIDER", "0") != "1", "this module tests the default route"
        run_cases(pkg, on)
        child("1", off)
        yield on, off


def test_factor_agreement_rider_on_and_off(both_routes, orc):
    """lower triangles of both routes within 1e-13 max|L| of each other (packed and lda > n behind a 16-byte offset,
    decomp1 and factor_solve with 1..5 right-hand sides); both within the suite's 1e-12 of the oracle at n <= 1024"""
    on, off = both_routes
    for n in SIZES:
        a = spd(n, n)
        llt = orc.cholesky_decomp1(a)[1] if n <= 1024 else None
        want = np.tril(llt) if n <= 1024 else None
        names = [f"L_{n}_{name}" for name, _, _ in layouts(n)] + [f"FL_{n}_{nrhs}" for nrhs in range(1, 6)]
        for nm in names:
            l_on, l_off = np.load(os.path.join(on, nm + ".npy")), np.load(os.path.join(off, nm + ".npy"))
            scale = np.abs(l_off).max()
            d = np.abs(l_on - l_off).max()
            print(f"{nm}: on vs off {d / scale:.3e} (bit-identical {np.array_equal(l_on, l_off)})")
            assert d <= 1e-13 * scale, nm
            if want is not None:
                assert np.abs(l_on - want).max() <= 1e-12 * np.abs(want).max(), nm
                assert np.abs(l_off - want).max() <= 1e-12 * np.abs(want).max(), nm
        for nrhs in range(1, 6):
            x_on, x_off = np.load(os.path.join(on, f"FX_{n}_{nrhs}.npy")), np.load(os.path.join(off, f"FX_{n}_{nrhs}.npy"))
            # the matrices are strongly diagonally dominant (condition number of order 1): the solutions inherit the factors' agreement
            assert np.abs(x_on - x_off).max() <= 1e-12 * np.abs(x_off).max(), (n, nrhs)
            if want is not None:
                b = np.random.default_rng(100 * n + nrhs).random((nrhs, n))
                for q in range(nrhs):
                    xo = orc.cholesky_solve(llt, b[q])
                    assert np.abs(x_on[q] - xo).max() <= 1e-11 * np.abs(xo).max(), (n, nrhs, q)


def test_edom_is_reported_alike(both_routes, orc, pkg):
    """cholesky.c:120-123: the failing column, in a block the rider factors and in panel 0: same status and column on
    both routes, the column the reference stops at"""
    on, off = both_routes
    for n, col in EDOM_CASES:
        r_on, r_off = np.load(os.path.join(on, f"EDOM_{n}_{col}.npy")), np.load(os.path.join(off, f"EDOM_{n}_{col}.npy"))
        a = spd(n, 7)
        a[col, col] = -1.0
        st_o, part = orc.cholesky_decomp1(a)
        assert st_o != 0
        # the oracle scales a column only after its pivot passed: the first column whose diagonal is still <= 0
        stopped = int(np.argmax(np.diag(part) <= 0.0))
        assert stopped == col
        assert list(r_on) == [pkg.capi.GSL_EDOM, stopped + 1], (n, col, r_on)
        assert list(r_off) == list(r_on), (n, col, r_off)


def test_rider_count(both_routes, pkg):
    """every leaf but the first is factored by a rider when all panels are 128 wide; none when they are not, none when off.
    n / 128 - 1 holds for the sizes here (n <= 4096 on a 256-CU device): the 256 x 128 tile has no rider variant, so from
    n = 8192 on the leaves behind the top-level updates that take that tile keep their own launch (61 of 63 riders at
    n = 8192, 121 of 127 at 16384)."""
    import torch
    on, off = both_routes
    got = {(int(n), int(s)): int(r) for n, s, r in np.load(os.path.join(on, "riders.npy"))}
    for n in SIZES:
        assert got[(n, 0)] == (n // 128 - 1 if n % 128 == 0 else 0), (n, got)
        assert got[(n, 1)] == got[(n, 0)], (n, got)
    assert all(int(r) == 0 for _, _, r in np.load(os.path.join(off, "riders.npy")))
    ctx = pkg.HipContext.on_torch_stream(0)
    d_a = torch.from_numpy(spd(1000, 3)).cuda()
    st, info = ctx.cholesky_decomp1(1000, d_a.data_ptr(), 1000)
    assert st == 0 and info == 0
    assert pkg.lib().gsl_sinterp_hip_debug_chol_riders() == 0


@pytest.mark.parametrize("n", [1024, 2176])
def test_repeated_calls_are_bit_identical(pkg, n):
    """five calls on one context (the first records the graph, the others replay it): counters and flags are reset by
    every call, the partial sums are added in a fixed order"""
    import torch
    ctx = pkg.HipContext.on_torch_stream(0)
    d0 = torch.from_numpy(spd(n, 11)).cuda()
    d = d0.clone()
    b0 = torch.from_numpy(np.random.default_rng(5).random((2, n))).cuda()
    first = None
    for rep in range(5):
        d.copy_(d0)
        x = b0.clone()
        st, info = ctx.cholesky_factor_solve(n, d.data_ptr(), n, x.data_ptr(), n, 2)
        assert st == 0 and info == 0
        got = (d.cpu().numpy(), x.cpu().numpy())
        if first is None:
            first = got
        else:
            assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1]), rep


LINALG = ["tests/test_gpu_linalg.py", "-k", "cholesky or gemm or graph_replays or single_launch"]
RBF_INIT = ["tests/test_gpu_rbf.py", "-k", "repeated_init or tps_solver_routes or facade_rbf"]


@pytest.mark.parametrize("selection", [LINALG, RBF_INIT], ids=["linalg", "rbf"])
def test_switch_passes_parity(selection):
    """the launch-per-diagonal route behind the switch passes the existing parity tests (as tests/test_gpu_switches.py does)"""
    env = dict(os.environ)
    env["GSL_SINTERP_NO_DIAG_RIDER"] = "1"
    cmd = [sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider"] + selection
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, "GSL_SINTERP_NO_DIAG_RIDER=1: " + " ".join(selection) + "\n" + r.stdout[-3000:]


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import __graft_entry__ as g
    run_cases(g.load_package(), sys.argv[1])
