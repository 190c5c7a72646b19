"""Developer tool: time the imported tetrahedral mesh path (csrc/hip/mesh3.hip) next to the 2-D imported mesh path.

N = 10^5 uniform points, M = 10^7 uniform targets in the points' bounding box, resident buffers, for dim = 3 and, as the
yardstick, dim = 2 at the same N and M.  The triangulation comes from scipy.spatial.Delaunay (QHull) and is built, like
the host import, OUTSIDE the timed regions.  Timed, 2 warm-up + 5 timed runs each, wall clock ended by a device
synchronise, median and spread:
  * pack: simplex_mesh_device_alloc (upload of the raw arrays, records, seed grid) + set_response (response table);
  * eval: simplex_mesh_device_eval_resident over the M targets (reorder, walk, scan, un-sort), with targets/s.
One JSON line per measurement, appended to --out (default profiles/mesh3_time.jsonl).
usage: python tools/mesh3_time.py [--out FILE] [--n POINTS] [--m TARGETS]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM, REPS = 2, 5


def stats(ms):
    s = sorted(ms)
    return {"ms_median": s[len(s) // 2], "ms_min": s[0], "ms_max": s[-1], "ms_all": ms}


def main():
    args = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "mesh3_time.jsonl")
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
    lines = []

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    rng = np.random.default_rng(20261019)
    for dim in (3, 2):
        x = rng.random((n, dim))
        f = 2.0 + np.sin(3.0 * x[:, 0]) + np.cos(2.0 * x[:, 1])
        t0 = time.perf_counter()
        d = Delaunay(x)
        t1 = time.perf_counter()
        mesh = pkg.SimplexMesh.from_arrays(x, d.simplices, d.neighbors)
        t2 = time.perf_counter()
        base = {"dim": dim, "n": n, "m": m, "simplices": int(mesh.n_triangles), "convex": bool(mesh.convex())}
        emit({"what": "host_untimed", **base, "qhull_s": t1 - t0, "import_s": t2 - t1})
        y = torch.from_numpy(rng.random((m, dim))).cuda()
        d_s = torch.empty(m, dtype=torch.float64, device="cuda")
        d_t = torch.empty(m, dtype=torch.int32, device="cuda")
        ms, dev = [], None
        for r in range(WARM + REPS):
            if dev is not None:
                dev.close()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dev = mesh.device_alloc(0)
            assert dev.set_response(f) == 0
            assert pkg.lib().gsl_sinterp_hip_sync(dev.ctx_handle()) == 0
            if r >= WARM:
                ms.append((time.perf_counter() - t0) * 1e3)
        emit({"what": "pack", **base, **stats(ms)})
        ms = []
        for r in range(WARM + REPS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            assert dev.eval_resident(y.data_ptr(), m, dim, d_s.data_ptr(), d_t.data_ptr()) == 0
            assert pkg.lib().gsl_sinterp_hip_sync(dev.ctx_handle()) == 0
            if r >= WARM:
                ms.append((time.perf_counter() - t0) * 1e3)
        rec = stats(ms)
        located = int((d_t >= 0).sum().item())
        emit({"what": "eval", **base, **rec, "targets_per_s": m / (rec["ms_median"] * 1e-3), "located": located})
        dev.close()
        del y, d_s, d_t
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as fp:
        for rec in lines:
            fp.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
