"""-m gpu: the 256x128 tile of the stream-K trailing update (csrc/hip/gemm.hip), whose owner segments start their
accumulators from the C tile and end in a store-only epilogue.  The tile is forced with the developer override
GSL_SINTERP_GEMM_CFG=0 in ONE child interpreter that runs every case below and saves its figures; the tests assert on
them.  The shapes are the smallest that reach each path of the kernel:
  a few whole tiles (one owner segment each); two tiles cut over ~32 workgroups (the owner starts from C and adds 15
  partials); 1056 tiles = three whole-tile rounds plus a K-split remainder (a workgroup ends one segment as non-owner
  and opens the next as owner); five K-steps per tile on a rectangular full update.
Bounds: |got - (C - A B^T)| <= 1e-12 k, the bound of tests/test_gpu_gemm_mid.py (operands N(0,1));
the factor within 1e-12 max|L| of numpy's, the bound of tests/test_gpu_chol_rider.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (name, m, n, k, lower, scale of A): scale 1e-6 / sqrt(k) makes the entries of C ~1e6 times the product's -- a wrong sign
# of the product or a dropped C is far outside the (absolute) bound, which stays the one of N(0,1) operands
CASES = [
    ("whole_lower", 512, 256, 64, 1, 1.0),
    ("whole_full", 512, 256, 64, 0, 1.0),
    ("whole_lower_large_c", 512, 256, 64, 1, 1e-6 / 8.0),
    ("deep_k_split", 256, 256, 4096, 1, 1.0),
    ("rounds_then_split", 8192, 8192, 64, 1, 1.0),
    ("five_steps_full", 8192, 4096, 80, 0, 1.0),
]
CHOL_N = [2176, 4096]


def _spd(n):
    rng = np.random.default_rng(n)
    m = rng.random((n, n))
    return np.tril(m) + np.tril(m, -1).T + 10.0 * n * np.eye(n)


def _child(out_path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import __graft_entry__ as g
    from gpu_util import dev, ptr
    pkg = g.load_package()
    ctx = pkg.HipContext.on_torch_stream(0)
    res = {}
    for name, m, n, k, lower, scale in CASES:
        rng = np.random.default_rng(m + 3 * n + 7 * k + lower)
        A = rng.standard_normal((m, k)) * scale
        B = rng.standard_normal((n, k))
        Cm = rng.standard_normal((m, n))
        dA, dB = dev(A), dev(B)
        got, repeat_same = None, True
        for _ in range(3):
            dC = dev(Cm)                                      # a fresh copy of C for every launch
            ctx.gemm_minus(m, n, k, ptr(dA), k, ptr(dB), k, 0, ptr(dC), n, lower)
            ctx.sync()
            out = dC.cpu().numpy()
            del dC
            if got is None:
                got = out
            else:
                repeat_same = repeat_same and bool(np.array_equal(got, out))
        ran = int(pkg.lib().gsl_sinterp_hip_debug_gemm_last_cfg())
        err = np.abs(got - (Cm - A @ B.T))
        if lower:
            upper_same = bool(np.array_equal(np.triu(got, 1), np.triu(Cm, 1)))   # m >= n: the strict upper part
            err = np.tril(err)
        else:
            upper_same = True
        res[name] = dict(ran=ran, err=float(err.max()), upper_same=upper_same, repeat_same=repeat_same,
                         finite=bool(np.isfinite(got).all()))
    for n in CHOL_N:
        a = _spd(n)
        gots = []
        for _ in range(2):
            d = dev(a)
            st, info = ctx.cholesky_decomp1(n, ptr(d), n)
            ctx.sync()
            gots.append(d.cpu().numpy())
        ref = np.linalg.cholesky(a)
        res["chol_%d" % n] = dict(st=int(st), info=int(info),
                                  rel=float(np.abs(np.tril(gots[0]) - ref).max() / np.abs(ref).max()),
                                  upper_same=bool(np.array_equal(np.triu(gots[0], 1), np.triu(a, 1))),
                                  repeat_same=bool(np.array_equal(gots[0], gots[1])))
    with open(out_path, "w") as f:
        json.dump(res, f)


@pytest.fixture(scope="module")
def figures(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("c256") / "figures.json")
    env = dict(os.environ)
    env["GSL_SINTERP_GEMM_CFG"] = "0"
    env.pop("GSL_SINTERP_GEMM_RULE_R4", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", out], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    with open(out) as f:
        return json.load(f)


@pytest.mark.parametrize("name,m,n,k,lower,scale", CASES, ids=[c[0] for c in CASES])
def test_c256_update(figures, name, m, n, k, lower, scale):
    f = figures[name]
    print(name, f)
    assert f["ran"] == 0, f["ran"]                 # 2 * cfg + whole: the 256x128 tile with the K split
    assert f["finite"]
    assert f["err"] <= 1e-12 * k, f["err"]
    assert f["upper_same"]                         # the strict upper part of C is untouched
    assert f["repeat_same"]                        # three launches on fresh copies of C: the same bits


@pytest.mark.parametrize("n", CHOL_N)
def test_c256_cholesky(figures, n):
    f = figures["chol_%d" % n]
    print(n, f)
    assert f["st"] == 0 and f["info"] == 0
    assert f["rel"] <= 1e-12, f["rel"]
    assert f["upper_same"]
    assert f["repeat_same"]                        # two calls: bit-identical factors


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "child":
        _child(sys.argv[2])
