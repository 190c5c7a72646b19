"""-m gpu: the meshless local routes (csrc/hip/local.hip, csrc/hip/shepard.hip) produce the BYTES the parent of the
"one neighbourhood body, one grid binning" refactor produced: k nearest neighbours, local ordinary and universal kriging,
the modified Shepard fit and sweep, through the raw capi entries only.

tests/golden/local_bits_parent.json was written by `python tests/test_gpu_local_bits.py` on the parent's build (twice:
the two files were identical, as the file headers of local.hip and shepard.hip argue they must be -- neighbour sets and
sums are functions of (model, target) alone).  Per case it holds the returned status and count and, per output buffer,
the SHA-256 of its bytes and its first four values (doubles as hex floats) so that a mismatch can be read.  The test fails
when the file is missing.

Cases: seeded numpy clouds in the unit box, the smallest shapes that reach every template instance and branch.
  local_krige / local_ukrige   Gaussian (the exp2-table kind) and Matern 5/2, dim 1..3, n = 300, m = 64, nugget 1e-3,
                               k on both sides of every KMAX boundary (and k = dim + 2, the least a linear drift takes);
                               dim 2, m = 4096, k = 8: the cell-ordered target route (LK_SORT_MIN)
  *_fail                       two coincident sites, nugget 0, one NaN target: failed pivots, their count, NaN outputs
  knn                          dim 3, k = 64
  shepard                      dim 2 and 3, n = 400, m = 256 and 4096 (cell-ordered), Renka's nq / nw; target 5 lies outside
                               every radius (counted, leaf -1), target 7 is NaN (not counted)"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

from gpu_util import dev, ptr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "local_bits_parent.json")
GAUSSIAN, MATERN52 = 0, 4
KINDS = {"gaussian": GAUSSIAN, "matern52": MATERN52}
SEED = 20261021
N_KRIGE, N_SHEPARD = 300, 400


def _cases():
    out = []
    for route in ("local_krige", "local_ukrige"):
        for kind in KINDS:
            for dim in (1, 2, 3):
                for k in ((5, 16, 17, 33, 64) if route == "local_krige" else (dim + 2, 16, 17, 64)):
                    out.append(dict(id=f"{route}-{kind}-d{dim}-k{k}", route=route, kind=kind, dim=dim, m=64, k=k, nugget=1e-3, fail=False))
            out.append(dict(id=f"{route}-{kind}-d2-k8-m4096", route=route, kind=kind, dim=2, m=4096, k=8, nugget=1e-3, fail=False))
        out.append(dict(id=f"{route}-fail", route=route, kind="matern52", dim=2, m=64, k=8, nugget=0.0, fail=True))
    out.append(dict(id="knn-d3-k64", route="knn", dim=3, m=64, k=64))
    for dim in (2, 3):
        for m in (256, 4096):
            out.append(dict(id=f"shepard-d{dim}-m{m}", route="shepard", dim=dim, m=m))
    return out


CASES = _cases()


def _cloud(n, dim, m, salt):
    """sites, responses (a polynomial: no libm in the inputs) and targets in the unit box"""
    rng = np.random.default_rng(SEED + 1000 * dim + salt)
    x = rng.random((n, dim))
    f = 1.0 + x[:, 0] - 0.5 * x[:, -1] ** 2 + x[:, 0] * x[:, dim // 2]
    y = rng.random((m, dim))
    return x, f, y


def _entry(bufs, status, count):
    rec = {"status": int(status), "count": int(count), "buffers": {}}
    for name, t in bufs.items():
        a = np.ascontiguousarray(t.cpu().numpy())
        head = a.ravel()[:4]
        rec["buffers"][name] = {"sha256": hashlib.sha256(a.tobytes()).hexdigest(),
                                "head": [float(v).hex() if a.dtype == np.float64 else int(v) for v in head]}
    return rec


def run_case(pkg, case):
    ctx = pkg.HipContext.on_torch_stream(0)
    dim, m = case["dim"], case["m"]
    f64 = lambda *shape: torch.full(shape, -7.0, dtype=torch.float64, device="cuda")
    i32 = lambda *shape: torch.full(shape, -7, dtype=torch.int32, device="cuda")
    if case["route"] == "shepard":
        n, nc = N_SHEPARD, 5 if dim == 2 else 9
        nq, nw = (13, 19) if dim == 2 else (17, 32)
        x, f, y = _cloud(n, dim, m, 1)
        y[5], y[7] = 10.0, np.nan
        d_x, d_f, d_y = dev(x), dev(f), dev(y)
        rq, rw, coef = f64(n), f64(n), f64(n, nc)
        st, counts = ctx.shepard_fit(ptr(d_x), n, dim, dim, ptr(d_f), nq, nw, ptr(rq), ptr(rw), ptr(coef))
        assert st == 0 and counts[2] == 0
        s, g, leaf, s_only = f64(m), f64(m, dim), i32(m), f64(m)
        st, outside = ctx.shepard_eval(ptr(d_x), n, dim, dim, ptr(d_f), ptr(rq), ptr(rw), ptr(coef), ptr(d_y), m, dim, ptr(s), ptr(g), dim,
                                       ptr(leaf))
        st2, outside2 = ctx.shepard_eval(ptr(d_x), n, dim, dim, ptr(d_f), ptr(rq), ptr(rw), ptr(coef), ptr(d_y), m, dim, ptr(s_only))
        assert (st2, outside2) == (st, outside)
        rec = _entry(dict(rq=rq, rw=rw, coef=coef, s=s, g=g, leaf=leaf, s_only=s_only), st, outside)
        rec["fit_counts"] = [int(c) for c in counts]
        return rec
    n, k = N_KRIGE, case["k"]
    x, f, y = _cloud(n, dim, m, 2)
    d_idx = i32(m, k)
    if case["route"] == "knn":
        d_x, d_y, r2 = dev(x), dev(y), f64(m, k)
        st = ctx.knn(ptr(d_x), n, dim, dim, ptr(d_y), m, dim, k, ptr(d_idx), ptr(r2))
        return _entry(dict(idx=d_idx, r2=r2), st, 0)
    if case["fail"]:
        x[1] = x[0]
        y[0] = x[0] + 1e-3                         # both coincident sites are among its neighbours
        y[3] = np.nan
    d_x, d_f, d_y = dev(x), dev(f), dev(y)
    eps = 0.5 * n ** (1.0 / dim)
    s, var = f64(m), f64(m)
    entry = ctx.local_krige if case["route"] == "local_krige" else ctx.local_ukrige
    st, failed = entry(KINDS[case["kind"]], eps, case["nugget"], ptr(d_x), n, dim, dim, ptr(d_f), ptr(d_y), m, dim, k, ptr(s), ptr(var),
                       ptr(d_idx))
    return _entry(dict(s=s, var=var, idx=d_idx), st, failed)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_bytes_equal_the_parent(pkg, case):
    want = json.load(open(GOLDEN))[case["id"]]
    got = run_case(pkg, case)
    for name, b in got["buffers"].items():
        print(f"{case['id']} {name}: head {b['head']} (parent {want['buffers'][name]['head']})")
    assert got == want


def test_the_fixture_reaches_the_branches():
    """what the cases are there for, read from the recorded parent: failed pivots and an outside target are counted"""
    gold = json.load(open(GOLDEN))
    assert sorted(gold) == sorted(c["id"] for c in CASES)
    for c in CASES:
        e = gold[c["id"]]
        if c["route"] == "shepard":
            assert (e["status"], e["count"]) == (1, 1) and e["fit_counts"][2] == 0
        elif c.get("fail"):
            assert e["status"] == 1 and e["count"] >= 1
        else:
            assert (e["status"], e["count"]) == (0, 0)


if __name__ == "__main__":                                            # record with the loaded build
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    p = g.load_package()
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    gold = {c["id"]: run_case(p, c) for c in CASES}
    with open(path, "w") as fh:
        json.dump(gold, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"{len(gold)} cases -> {path}")
