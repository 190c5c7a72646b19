"""Developer tool: time K responses (and their gradients) from one locate (csrc/hip/linear_fields.hip) next to the scalar
linear path called K times.

N = 10^5 uniform points, M = 10^7 uniform targets in the points' bounding box, resident buffers, for a 2-D and a 3-D
imported mesh (scipy.spatial.Delaunay, built like the host import and the device mirror OUTSIDE the timed regions).
Timed with the context's device events (gsl_sinterp_hip_timer_start / _stop around the entry), 2 warm-up + 7 timed rounds;
every round runs the scalar entry and then the six field configurations once, so that all of them see the same machine:
  * scalar:  simplex_mesh_device_eval_resident (reorder, walk, scan, un-sort) -- one response per call;
  * fields:  simplex_mesh_device_eval_fields_resident at K = 1, 3, 8, without and with gradients (the same locate once,
             then the fields sweep).
One JSON line per measurement, appended to --out (default profiles/linear_fields_time.jsonl): median [min - max] in ms,
next to each fields line the scalar median of the same run, K times that figure, and fields / (K x scalar).
usage: python tools/linear_fields_time.py [--out FILE] [--n POINTS] [--m TARGETS]"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM, REPS = 2, 7
KS = (1, 3, 8)


def stats(ms):
    s = sorted(ms)
    return {"ms_median": s[len(s) // 2], "ms_min": s[0], "ms_max": s[-1], "ms_all": ms}


def main():
    args = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "linear_fields_time.jsonl")
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
    for dim in (2, 3):
        x = rng.random((n, dim))
        F = np.ascontiguousarray(np.stack([2.0 + np.sin((3.0 + q) * x[:, 0]) + np.cos((2.0 + q) * x[:, 1]) for q in range(max(KS))], axis=1))
        d = Delaunay(x)
        mesh = pkg.SimplexMesh.from_arrays(x, d.simplices, d.neighbors)
        base = {"dim": dim, "n": n, "m": m, "simplices": int(mesh.n_triangles)}
        # one mirror per K (a binding is per mirror): the timed rounds then only evaluate
        devs = {}
        for K in KS:
            devs[K] = mesh.device_alloc(0)
            assert devs[K].set_response(np.ascontiguousarray(F[:, 0])) == 0 and devs[K].set_responses(F[:, :K]) == 0
        y = torch.from_numpy(rng.random((m, dim))).cuda()
        d_s = torch.empty(m, dtype=torch.float64, device="cuda")
        d_t = torch.empty(m, dtype=torch.int32, device="cuda")
        d_S = torch.empty(m * max(KS), dtype=torch.float64, device="cuda")
        d_G = torch.empty(m * max(KS) * dim, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()

        def timed(dev, call):
            h = dev.ctx_handle()
            assert L.gsl_sinterp_hip_timer_start(h) == 0
            assert call() == 0
            t = C.c_float(0)
            assert L.gsl_sinterp_hip_timer_stop(h, C.byref(t)) == 0
            return float(t.value)

        configs = [(K, grad) for K in KS for grad in (False, True)]
        ms = {c: [] for c in configs + ["scalar"]}
        for r in range(WARM + REPS):
            t = timed(devs[1], lambda: devs[1].eval_resident(y.data_ptr(), m, dim, d_s.data_ptr(), d_t.data_ptr()))
            if r >= WARM:
                ms["scalar"].append(t)
            for K, grad in configs:
                t = timed(devs[K], lambda: devs[K].eval_fields_resident(y.data_ptr(), m, dim, d_S.data_ptr(), K, d_G.data_ptr() if grad else None,
                                                                         K * dim, d_t.data_ptr()))
                if r >= WARM:
                    ms[(K, grad)].append(t)
        scalar = stats(ms["scalar"])
        located = int((d_t >= 0).sum().item())
        emit({"what": "scalar", **base, **scalar, "targets_per_s": m / (scalar["ms_median"] * 1e-3), "located": located})
        for K, grad in configs:
            rec = stats(ms[(K, grad)])
            emit({"what": "fields", **base, "K": K, "gradients": grad, **rec, "scalar_ms_median": scalar["ms_median"],
                  "K_scalar_calls_ms": K * scalar["ms_median"], "fields_over_K_scalar_calls": rec["ms_median"] / (K * scalar["ms_median"]),
                  "values_per_s": m * K / (rec["ms_median"] * 1e-3)})
        # what was timed is what the scalar entry returns: column 0 of the last K = 8 run against the scalar values
        assert devs[8].eval_fields_resident(y.data_ptr(), m, dim, d_S.data_ptr(), 8, None, 0, d_t.data_ptr()) == 0
        assert devs[1].eval_resident(y.data_ptr(), m, dim, d_s.data_ptr(), d_t.data_ptr()) == 0
        torch.cuda.synchronize()
        same = bool(torch.equal(d_S.view(m, 8)[:, 0].contiguous().view(torch.int64), d_s.view(torch.int64)))
        emit({"what": "check", **base, "column0_bits_equal_scalar": same})
        for dev in devs.values():
            dev.close()
        del y, d_s, d_t, d_S, d_G
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as fp:
        for rec in lines:
            fp.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
