"""Developer tool: time natural-neighbour interpolation (csrc/hip/natural.hip) next to the linear 2-D mesh path.

N = 10^5 uniform points, M = 10^7 uniform targets in the points' bounding box, resident buffers.  The triangulation comes
from scipy.spatial.Delaunay (QHull) and is built, like the host import and the device mirror, OUTSIDE the timed regions;
the natural-neighbour records are packed by the first (warm-up) evaluation.  Timed with the context's device events
(gsl_sinterp_hip_timer_start / _stop around the entry), 2 warm-up + 7 timed runs each, median [min - max]:
  * linear:  simplex_mesh_device_eval_resident (reorder, walk, scan, un-sort) -- the yardstick;
  * natural: simplex_mesh_device_eval_natural_resident (the same locate, then the cavity sweep and its scan).
One JSON line per measurement, appended to --out (default profiles/natural_time.jsonl).
usage: python tools/natural_time.py [--out FILE] [--n POINTS] [--m TARGETS]"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM, REPS = 2, 7


def stats(ms):
    s = sorted(ms)
    return {"ms_median": s[len(s) // 2], "ms_min": s[0], "ms_max": s[-1], "ms_all": ms}


def main():
    args = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "natural_time.jsonl")
    n, m = 10 ** 5, 10 ** 7
    if "--out" in args:
        i = args.index("--out"); out = args[i + 1]; del args[i:i + 2]
    if "--n" in args:
        i = args.index("--n"); n = int(args[i + 1]); del args[i:i + 2]
    if "--m" in args:
        i = args.index("--m"); m = int(args[i + 1]); del args[i:i + 2]
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from scipy.spatial import Delaunay
    import __graft_entry__ as g
    pkg = g.load_package()
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to fall back to"
    L = pkg.lib()
    lines = []

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    rng = np.random.default_rng(20261019)
    x = rng.random((n, 2))
    f = 2.0 + np.sin(3.0 * x[:, 0]) + np.cos(2.0 * x[:, 1])
    d = Delaunay(x)
    mesh = pkg.SimplexMesh.from_arrays(x, d.simplices, d.neighbors)
    base = {"n": n, "m": m, "triangles": int(mesh.n_triangles), "metric": mesh.delaunay_metric()}
    dev = mesh.device_alloc(0)
    assert dev.set_response(f) == 0
    h = dev.ctx_handle()
    y = torch.from_numpy(rng.random((m, 2))).cuda()
    d_s = torch.empty(m, dtype=torch.float64, device="cuda")
    d_t = torch.empty(m, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    med = {}
    for what, fn in (("linear", dev.eval_resident), ("natural", dev.eval_natural_resident)):
        ms = []
        for r in range(WARM + REPS):
            assert L.gsl_sinterp_hip_timer_start(h) == 0
            assert fn(y.data_ptr(), m, 2, d_s.data_ptr(), d_t.data_ptr()) == 0
            t = C.c_float(0)
            assert L.gsl_sinterp_hip_timer_stop(h, C.byref(t)) == 0
            if r >= WARM:
                ms.append(float(t.value))
        rec = stats(ms)
        med[what] = rec["ms_median"]
        located = int((d_t >= 0).sum().item())
        finite = int(torch.isfinite(d_s).sum().item())
        emit({"what": what, **base, **rec, "targets_per_s": m / (rec["ms_median"] * 1e-3), "located": located, "finite": finite})
    emit({"what": "ratio", **base, "natural_over_linear": med["natural"] / med["linear"]})
    dev.close()
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as fp:
        for rec in lines:
            fp.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
