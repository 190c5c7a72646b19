"""Developer tool: time modified quadratic Shepard interpolation (csrc/hip/shepard.hip) next to the linear 2-D mesh path and
local kriging.

Uniform clouds in the unit box, default parameters (nq / nw = 13 / 19 in 2-D, 17 / 32 in 3-D), M = 10^7 uniform resident
targets.  Timed with the context's device events, 2 warm-up + 7 timed runs each (the N = 10^6 fit: 1 + 3), median
[min - max]:
  * fit:        gsl_sinterp_hip_shepard_fit on resident arrays (neighbour search in chunks + one wave per node), N = 10^5
                in 2-D and 3-D and N = 10^6 in 3-D;
  * pack:       a sweep of 64 targets with model id 0, which packs every time: the pack plus one small launch;
  * value:      gsl_sinterp_hip_shepard_eval, values only, on the packed model;
  * value_grad: the same with the gradient output;
  * linear:     simplex_mesh_device_eval_resident on the QHull triangulation of the same 2-D cloud (built outside the
                timed region) -- the yardstick of the mesh methods;
  * local_k32:  gsl_sinterp_hip_local_krige, Matern 5/2 at eps = sqrt(N), nugget 1e-3, k = 32, value only, on 10^6 of the
                targets (one wave per target: its rate is what is compared, not its time).
One JSON line per measurement, appended to --out (default profiles/shepard_time.jsonl).
usage: python tools/shepard_time.py [--out FILE] [--m TARGETS] [--skip-million]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM, REPS = 2, 7
DEFAULTS = {2: (13, 19), 3: (17, 32)}
MATERN52 = 4


def stats(ms):
    s = sorted(ms)
    return {"ms_median": s[len(s) // 2], "ms_min": s[0], "ms_max": s[-1], "ms_all": ms}


def main():
    args = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "shepard_time.jsonl")
    m, million = 10 ** 7, True
    if "--out" in args:
        i = args.index("--out"); out = args[i + 1]; del args[i:i + 2]
    if "--m" in args:
        i = args.index("--m"); m = int(args[i + 1]); del args[i:i + 2]
    if "--skip-million" in args:
        args.remove("--skip-million"); million = False
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import __graft_entry__ as g
    pkg = g.load_package()
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to fall back to"
    lines = []

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    def timed(ctx, call, warm=WARM, reps=REPS):
        ms = []
        for r in range(warm + reps):
            ctx.timer_start()
            call()
            t = ctx.timer_stop()
            if r >= warm:
                ms.append(float(t))
        return stats(ms)

    rng = np.random.default_rng(20261019)
    for dim, n in ((2, 10 ** 5), (3, 10 ** 5)) + (((3, 10 ** 6),) if million else ()):
        nq, nw = DEFAULTS[dim]
        nc = dim + dim * (dim + 1) // 2
        xh = rng.random((n, dim))
        fh = 2.0 + np.sin(3.0 * xh[:, 0]) + np.cos(2.0 * xh[:, 1]) + (xh[:, 2] ** 2 if dim == 3 else 0.0)
        x, f = torch.from_numpy(xh).cuda(), torch.from_numpy(fh).cuda()
        rq = torch.empty(n, dtype=torch.float64, device="cuda")
        rw = torch.empty(n, dtype=torch.float64, device="cuda")
        coef = torch.empty((n, nc), dtype=torch.float64, device="cuda")
        y = torch.from_numpy(rng.random((m, dim))).cuda()
        d_s = torch.empty(m, dtype=torch.float64, device="cuda")
        d_g = torch.empty((m, dim), dtype=torch.float64, device="cuda")
        d_l = torch.empty(m, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        base = {"n": n, "m": m, "dim": dim, "nq": nq, "nw": nw}
        ctx = pkg.HipContext.on_torch_stream(0)
        info = {}

        def fit():
            st, counts = ctx.shepard_fit(x.data_ptr(), n, dim, dim, f.data_ptr(), nq, nw, rq.data_ptr(), rw.data_ptr(), coef.data_ptr())
            assert st == 0
            info.update(linear_fallbacks=counts[0], constant_fallbacks=counts[1])

        big = n >= 10 ** 6
        emit({"what": "fit", **base, **timed(ctx, fit, 1 if big else WARM, 3 if big else REPS), **info, "rw_max": float(rw.max().item())})

        def sweep(count, grad, leaf, model_id):
            st, outside = ctx.shepard_eval(x.data_ptr(), n, dim, dim, f.data_ptr(), rq.data_ptr(), rw.data_ptr(), coef.data_ptr(), y.data_ptr(),
                                           count, dim, d_s.data_ptr(), d_g.data_ptr() if grad else None, dim, d_l.data_ptr() if leaf else None,
                                           model_id)
            assert st in (0, pkg.GSL_EDOM)
            info["outside"] = outside

        emit({"what": "pack", **base, **timed(ctx, lambda: sweep(64, False, False, 0)), "record_bytes": 80 if dim == 2 else 128})
        med = {}
        for what, grad in (("value", False), ("value_grad", True)):
            rec = timed(ctx, lambda: sweep(m, grad, True, 1))
            med[what] = rec["ms_median"]
            emit({"what": what, **base, **rec, "targets_per_s": m / (rec["ms_median"] * 1e-3), "outside": info["outside"],
                  "mean_leaf": float(d_l[d_l > 0].double().mean().item()), "max_leaf": int(d_l.max().item())})
        if dim == 2:
            from scipy.spatial import Delaunay
            d = Delaunay(xh)
            mesh = pkg.SimplexMesh.from_arrays(xh, d.simplices, d.neighbors)
            dev = mesh.device_alloc(0)
            assert dev.set_response(fh) == 0
            L = pkg.lib()
            import ctypes as C
            ms = []
            for r in range(WARM + REPS):
                assert L.gsl_sinterp_hip_timer_start(dev.ctx_handle()) == 0
                assert dev.eval_resident(y.data_ptr(), m, 2, d_s.data_ptr(), d_l.data_ptr()) in (0, pkg.GSL_EDOM)
                t = C.c_float(0)
                assert L.gsl_sinterp_hip_timer_stop(dev.ctx_handle(), C.byref(t)) == 0
                if r >= WARM:
                    ms.append(float(t.value))
            rec = stats(ms)
            emit({"what": "linear", **base, **rec, "targets_per_s": m / (rec["ms_median"] * 1e-3), "triangles": int(mesh.n_triangles)})
            emit({"what": "ratio", **base, "value_over_linear": med["value"] / rec["ms_median"],
                  "value_grad_over_linear": med["value_grad"] / rec["ms_median"]})
            dev.close()
            ml = min(m, 10 ** 6)
            eps = float(n) ** 0.5

            def local():
                st, failed = ctx.local_krige(MATERN52, eps, 1e-3, x.data_ptr(), n, 2, 2, f.data_ptr(), y.data_ptr(), ml, 2, 32, d_s.data_ptr(),
                                             None, None, 2)
                assert st == 0

            rec = timed(ctx, local)
            emit({"what": "local_k32", **base, "m": ml, **rec, "targets_per_s": ml / (rec["ms_median"] * 1e-3)})
        ctx.close()
        del x, f, rq, rw, coef, y, d_s, d_g, d_l
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as fp:
        for rec in lines:
            fp.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
