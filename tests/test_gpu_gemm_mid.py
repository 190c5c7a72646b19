"""-m gpu: the stream-K trailing update (gsl_sinterp_hip_gemm_minus) under each tile configuration and split policy
of its dispatcher (csrc/hip/gemm.hip), forced through GSL_SINTERP_GEMM_CFG in a child interpreter (read once per
process), and the Cholesky factorisation under the current dispatch rule and the round-4 rule
(GSL_SINTERP_GEMM_RULE_R4=1)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gpu_util import dev, ptr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.2204460492503131e-16

# (m, n, k, lower): every shape is a whole number of 128-tiles with k % 16 == 0, so it takes the stream-K path
SHAPES = [
    (1024, 1024, 256, 1),     # lower square
    (1024, 512, 512, 0),      # full
    (2048, 512, 256, 1),      # lower trapezoid
    (1152, 384, 128, 1),      # rows not a multiple of 256
    (8192, 2048, 64, 1),      # more than two rounds of tiles: whole-tile rounds, then a split remainder
    (512, 512, 2048, 0),      # few tiles, deep K: pure stream-K, every tile split
    (512, 256, 1024, 1),      # the same, lower
]
# tile configuration [+ "w": whole tiles only]; "" = the dispatch rule
VARIANTS = ["", "0", "1", "2", "5", "6", "5w", "6w", "1w"]
RULE_CFGS = (0, 5, 6)      # what the dispatch rule picks from


def _expected_cfg(m, n, lower):
    """(cfg, whole) the forced GSL_SINTERP_GEMM_CFG of this process must launch, or None where the shape does not
    allow it (the 256-row tile needs m % 256 == 0 and, lower, an even count of 128-columns) and the rule applies."""
    v = os.environ.get("GSL_SINTERP_GEMM_CFG")
    if not v:
        return None
    cfg = int(v.rstrip("w"))
    tn = min(n // 128, m // 128) if lower else n // 128
    if cfg == 0 and (m % 256 or tn % 2):
        return None
    return cfg, v.endswith("w")


@pytest.mark.parametrize("m,n,k,lower", SHAPES)
def test_gemm_mid_shapes(pkg, m, n, k, lower):
    """C -= A B^T against numpy under whatever configuration this process was started with."""
    rng = np.random.default_rng(m + 3 * n + 7 * k + lower)
    A = rng.standard_normal((m, k)); B = rng.standard_normal((n, k)); Cm = rng.standard_normal((m, n))
    ctx = pkg.HipContext.on_torch_stream(0)
    dA, dB = dev(A), dev(B)
    outs = []
    for _ in range(3):
        dC = dev(Cm)
        ctx.gemm_minus(m, n, k, ptr(dA), k, ptr(dB), k, 0, ptr(dC), n, lower)
        ctx.sync()
        outs.append(dC.cpu().numpy())
    ran = pkg.lib().gsl_sinterp_hip_debug_gemm_last_cfg()
    want_cfg = _expected_cfg(m, n, lower)
    if want_cfg is None:
        assert ran >= 0 and ran // 2 in RULE_CFGS and ran % 2 == 0, ran
    else:
        assert (ran // 2, bool(ran % 2)) == want_cfg, (ran, want_cfg)
    got = outs[0]
    want = Cm - A @ B.T
    if lower:
        rows, cols = np.indices((m, n))
        mask = cols <= rows
        assert np.abs(got - want)[mask].max() <= 1e-12 * k
        assert np.array_equal(got[~mask], Cm[~mask])          # strict upper part untouched
    else:
        assert np.abs(got - want).max() <= 1e-12 * k
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])   # repeated launches: same bits


@pytest.mark.parametrize("variant", VARIANTS, ids=[v or "rule" for v in VARIANTS])
def test_every_configuration_passes(variant):
    env = dict(os.environ)
    env.pop("GSL_SINTERP_GEMM_CFG", None)
    if variant:
        env["GSL_SINTERP_GEMM_CFG"] = variant
    cmd = [sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider",
           "tests/test_gpu_gemm_mid.py", "-k", "test_gemm_mid_shapes"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, f"GSL_SINTERP_GEMM_CFG={variant}\n" + r.stdout[-3000:]


def _spd(n, seed):
    rng = np.random.default_rng(seed)
    m = rng.random((n, n))
    return np.tril(m) + np.tril(m, -1).T + 10.0 * n * np.eye(n)


def _factor_solve(pkg, a, b):
    n = a.shape[0]
    ctx = pkg.HipContext.on_torch_stream(0)
    d_a = dev(a)
    st, info = ctx.cholesky_decomp1(n, ptr(d_a), n)
    assert st == 0 and info == 0
    d_x = dev(b)
    ctx.cholesky_svx(n, ptr(d_a), n, ptr(d_x))
    ctx.sync()
    return d_a.cpu().numpy(), d_x.cpu().numpy()


# child half of the round-4 comparison: factor and solve in a fresh interpreter, save the results
_CHILD = """
import sys, numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import __graft_entry__ as g
from test_gpu_gemm_mid import _spd, _factor_solve
n = {n}
L, x = _factor_solve(g.load_package(), _spd(n, n), np.arange(1, n + 1, dtype=np.float64))
np.save({out!r} + "_L.npy", L); np.save({out!r} + "_x.npy", x)
"""


def test_cholesky_new_and_round4_dispatch(pkg, orc, tmp_path):
    n = 4096
    a = _spd(n, n)
    b = np.arange(1, n + 1, dtype=np.float64)
    got_new = _factor_solve(pkg, a, b)
    env = dict(os.environ)
    env.pop("GSL_SINTERP_GEMM_CFG", None)
    env["GSL_SINTERP_GEMM_RULE_R4"] = "1"
    code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), n=n, out=str(tmp_path / "r4"))
    cmd = [sys.executable, "-c", code]
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    got_r4 = (np.load(str(tmp_path / "r4_L.npy")), np.load(str(tmp_path / "r4_x.npy")))
    st_o, want = orc.cholesky_decomp1(a)
    Lo = np.tril(want)
    xo = orc.cholesky_solve(want, b)
    for got, x in (got_new, got_r4):
        L = np.tril(got)
        assert np.abs(L - Lo).max() <= 1e-12 * np.abs(Lo).max()
        assert np.array_equal(np.triu(got, 1), np.triu(a, 1))
        assert np.abs(L @ L.T - a).max() <= (10.0 + n / 20.0) * EPS * np.abs(a).max()
        assert np.abs(x - xo).max() <= 1e-11 * np.abs(xo).max()
