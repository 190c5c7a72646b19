"""Developer tool: time Clough-Tocher interpolation (csrc/hip/cubic.hip) next to the linear 2-D mesh path and natural
neighbours.

N = 10^5 uniform points, M = 10^7 uniform targets in the points' bounding box, resident buffers.  The triangulation comes
from scipy.spatial.Delaunay (QHull) and is built, like the host import, the vertex adjacency and the device mirror,
OUTSIDE the timed regions.  Timed with the context's device events (gsl_sinterp_hip_timer_start / _stop around the
entry), 2 warm-up + 7 timed runs each, median [min - max]:
  * gradients:   gsl_sinterp_hip_mesh_cubic_gradients on resident arrays (set-up, the PCG iterations with their host
                 looks at the stopping verdict, to rtol = 1e-12);
  * pack:        gsl_sinterp_hip_mesh_cubic_pack (one record per triangle);
  * linear:      simplex_mesh_device_eval_resident (reorder, walk, scan, un-sort) -- the yardstick;
  * natural:     simplex_mesh_device_eval_natural_resident -- the second yardstick;
  * cubic:       simplex_mesh_device_eval_cubic_resident, values only (the same locate, then the cubic sweep);
  * cubic_grad:  the same with the gradient output.
One JSON line per measurement, appended to --out (default profiles/cubic_time.jsonl).
usage: python tools/cubic_time.py [--out FILE] [--n POINTS] [--m TARGETS]"""
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
    out = os.path.join(ROOT, "profiles", "cubic_time.jsonl")
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

    def timed(h, call):
        ms = []
        for r in range(WARM + REPS):
            assert L.gsl_sinterp_hip_timer_start(h) == 0
            call()
            t = C.c_float(0)
            assert L.gsl_sinterp_hip_timer_stop(h, C.byref(t)) == 0
            if r >= WARM:
                ms.append(float(t.value))
        return stats(ms)

    rng = np.random.default_rng(20261019)
    x = rng.random((n, 2))
    f = 2.0 + np.sin(3.0 * x[:, 0]) + np.cos(2.0 * x[:, 1])
    d = Delaunay(x)
    mesh = pkg.SimplexMesh.from_arrays(x, d.simplices, d.neighbors)
    n_tri = int(mesh.n_triangles)
    base = {"n": n, "m": m, "triangles": n_tri}
    dev = mesh.device_alloc(0)
    assert dev.set_response(f) == 0
    h = dev.ctx_handle()

    # the two preparation steps through the raw entries, on resident arrays
    off, adj = mesh.vertex_adjacency()
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    t_off, t_adj, t_x, t_f = cu(off), cu(adj), cu(x), cu(f)
    t_tri, t_nbr = cu(mesh.triangles()), cu(mesh.neighbours())
    t_g = torch.empty((n, 2), dtype=torch.float64, device="cuda")
    t_rec = torch.empty(n_tri * pkg.capi.CUBIC_RECORD_BYTES // 8, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    info = {}

    def solve():
        it, res = C.c_int(0), C.c_double(0.0)
        assert L.gsl_sinterp_hip_mesh_cubic_gradients(h, n, t_off.data_ptr(), t_adj.data_ptr(), len(adj), t_x.data_ptr(), t_f.data_ptr(),
                                                      1e-12, 1000, t_g.data_ptr(), C.byref(it), C.byref(res)) == 0
        info.update(iterations=it.value, residual=res.value)

    rec = timed(h, solve)
    emit({"what": "gradients", **base, **rec, **info, "edges": len(adj) // 2})

    def pack():
        assert L.gsl_sinterp_hip_mesh_cubic_pack(h, n_tri, t_tri.data_ptr(), t_nbr.data_ptr(), n, t_x.data_ptr(), t_f.data_ptr(),
                                                 t_g.data_ptr(), t_rec.data_ptr()) == 0

    emit({"what": "pack", **base, **timed(h, pack), "record_bytes": pkg.capi.CUBIC_RECORD_BYTES})

    # the sweeps through the mirror (its first cubic call estimates and packs: a warm-up run)
    y = torch.from_numpy(rng.random((m, 2))).cuda()
    d_s = torch.empty(m, dtype=torch.float64, device="cuda")
    d_g = torch.empty((m, 2), dtype=torch.float64, device="cuda")
    d_t = torch.empty(m, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    yp, sp, gp, tp = y.data_ptr(), d_s.data_ptr(), d_g.data_ptr(), d_t.data_ptr()
    med = {}
    for what, fn in (("linear", lambda: dev.eval_resident(yp, m, 2, sp, tp)),
                     ("natural", lambda: dev.eval_natural_resident(yp, m, 2, sp, tp)),
                     ("cubic", lambda: dev.eval_cubic_resident(yp, m, 2, sp, None, 2, tp)),
                     ("cubic_grad", lambda: dev.eval_cubic_resident(yp, m, 2, sp, gp, 2, tp))):
        def call():
            assert fn() == 0
        rec = timed(h, call)
        med[what] = rec["ms_median"]
        located = int((d_t >= 0).sum().item())
        finite = int(torch.isfinite(d_s).sum().item())
        emit({"what": what, **base, **rec, "targets_per_s": m / (rec["ms_median"] * 1e-3), "located": located, "finite": finite})
    emit({"what": "ratio", **base, "cubic_over_linear": med["cubic"] / med["linear"], "cubic_grad_over_linear": med["cubic_grad"] / med["linear"],
          "cubic_over_natural": med["cubic"] / med["natural"]})
    dev.close()
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as fp:
        for rec in lines:
            fp.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
