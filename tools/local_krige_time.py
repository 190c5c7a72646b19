"""Developer tool: time local kriging (gsl_sinterp_hip_local_krige) and, where a dense model still fits, the global kriging
it stands beside.

2-D, Matern 5/2 covariance at the type's default shape sqrt(N), nugget 1e-3, uniform clouds, M = 10^6 uniform targets,
k in {16, 32, 64}; 2 warm-up + 7 timed runs, median and spread.  Resident buffers everywhere.
  * local, N = 16384 and N = 10^6: device-event time of one gsl_sinterp_hip_local_krige call (value + variance; the entry
    synchronises) on a packed model, and of gsl_sinterp_hip_local_pack (model id 0: packs every time);
  * global, N = 16384 only (a dense matrix at N = 10^6 is 8 TB): wall clock of gsl_sinterp_init with set_variance and of
    gsl_sinterp_eval_resident over the same 10^6 targets, each ended by a device synchronise.  The variance of the global
    model costs M N^2 flops and is timed on 16384 targets only.
One JSON line per measurement, appended to --out (default profiles/local_krige_time.jsonl).
usage: python tools/local_krige_time.py [--out FILE] [--m TARGETS] [--skip-global] [N ...]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM, REPS, DIM, NUGGET, KIND, MATERN52 = 2, 7, 2, 1e-3, "kriging_matern52", 4


def stats(ms):
    s = sorted(ms)
    return {"ms_median": s[len(s) // 2], "ms_min": s[0], "ms_max": s[-1], "ms_all": ms}


def main():
    args = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "local_krige_time.jsonl")
    m, skip_global = 10 ** 6, False
    if "--out" in args:
        i = args.index("--out"); out = args[i + 1]; del args[i:i + 2]
    if "--m" in args:
        i = args.index("--m"); m = int(args[i + 1]); del args[i:i + 2]
    if "--skip-global" in args:
        args.remove("--skip-global"); skip_global = True
    sizes = [int(a) for a in args] or [16384, 10 ** 6]
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

    rng = np.random.default_rng(20261019)
    y = torch.from_numpy(rng.random((m, DIM))).cuda()
    d_s = torch.empty(m, dtype=torch.float64, device="cuda")
    d_v = torch.empty(m, dtype=torch.float64, device="cuda")
    for n in sizes:
        xh = rng.random((n, DIM))
        fh = 2.0 + np.sin(3.0 * xh[:, 0]) + np.cos(2.0 * xh[:, 1])
        x, f = torch.from_numpy(xh).cuda(), torch.from_numpy(fh).cuda()
        eps = n ** (1.0 / DIM)
        base = {"n": n, "m": m, "dim": DIM, "kind": KIND, "nugget": NUGGET, "eps": eps}
        ctx = pkg.HipContext.on_torch_stream(0)
        ms = []
        for r in range(WARM + REPS):
            ctx.timer_start()
            assert ctx.local_pack(x.data_ptr(), n, DIM, DIM, f.data_ptr(), 0) == 0
            t = ctx.timer_stop()
            if r >= WARM:
                ms.append(t)
        emit({"what": "local_pack", **base, **stats(ms)})
        for k in (16, 32, 64):
            ms = []
            for r in range(WARM + REPS):
                ctx.timer_start()
                st, failed = ctx.local_krige(MATERN52, eps, NUGGET, x.data_ptr(), n, DIM, DIM, f.data_ptr(), y.data_ptr(), m, DIM, k,
                                             d_s.data_ptr(), d_v.data_ptr(), None, n)
                t = ctx.timer_stop()
                assert st == 0 and failed == 0
                if r >= WARM:
                    ms.append(t)
            rec = stats(ms)
            emit({"what": "local_krige", "k": k, **base, **rec, "targets_per_s": m / (rec["ms_median"] * 1e-3), "packs": ctx.local_pack_count()})
        ctx.close()
        if n <= 16384 and not skip_global:
            si = pkg.Sinterp(KIND, DIM, n, 0)
            assert si.set_nugget(NUGGET) == 0 and si.set_variance(1) == 0

            def wall(fn):
                v = []
                for r in range(WARM + REPS):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    assert fn() == 0
                    torch.cuda.synchronize()
                    if r >= WARM:
                        v.append((time.perf_counter() - t0) * 1e3)
                return stats(v)

            emit({"what": "global_init_with_variance", **base, **wall(lambda: si.init(xh, fh))})
            rec = wall(lambda: si.eval_resident(y.data_ptr(), m, DIM, d_s.data_ptr()))
            emit({"what": "global_eval", **base, **rec, "targets_per_s": m / (rec["ms_median"] * 1e-3)})
            mv = min(m, 16384)
            rec = wall(lambda: si.eval_variance_resident(y.data_ptr(), mv, DIM, d_v.data_ptr()))
            emit({"what": "global_variance", **base, "m": mv, **rec, "targets_per_s": mv / (rec["ms_median"] * 1e-3)})
            si.close()
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as fp:
        for rec in lines:
            fp.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
