"""Developer tool: what a polynomial drift (gsl_sinterp_set_drift) costs next to ordinary kriging, measured in the same run.

2-D, Matern 5/2 covariance at the type's default shape sqrt(N), nugget 1e-3, uniform clouds, resident buffers; 2 warm-up +
5 timed runs, median and spread; wall clock ended by a device synchronise, except the local route (device events around
the entry, which synchronises itself).
  * init at N = 4096 and 16384 for order 0, 1 and 2 (without set_variance);
  * 10^6 resident targets at N = 4096: value (gsl_sinterp_eval_resident) and value + gradient (eval_grad_resident), order
    0, 1, 2;
  * variance of 10^4 targets at N = 4096 (set_variance), order 0, 1, 2;
  * local route: N = 10^6, k = 32, 10^6 targets, order 0 (gsl_sinterp_hip_local_krige) against order 1 (_local_ukrige).
One JSON line per measurement, appended to --out (default profiles/ukrige_time.jsonl); every line of order > 0 carries
"ratio_to_ordinary", its median over the median of the order-0 line of the same measurement.
usage: python tools/ukrige_time.py [--out FILE] [--m TARGETS] [--skip-local]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM, REPS, DIM, NUGGET, KIND, MATERN52 = 2, 5, 2, 1e-3, "kriging_matern52", 4


def stats(ms):
    s = sorted(ms)
    return {"ms_median": s[len(s) // 2], "ms_min": s[0], "ms_max": s[-1], "ms_all": ms}


def main():
    args = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "ukrige_time.jsonl")
    m, skip_local = 10 ** 6, False
    if "--out" in args:
        i = args.index("--out"); out = args[i + 1]; del args[i:i + 2]
    if "--m" in args:
        i = args.index("--m"); m = int(args[i + 1]); del args[i:i + 2]
    if "--skip-local" in args:
        args.remove("--skip-local"); skip_local = True
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import __graft_entry__ as g
    pkg = g.load_package()
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to fall back to"
    lines, ordinary = [], {}

    def emit(what, order, base, rec):
        rec = {"what": what, "order": order, **base, **rec}
        key = (what, base["n"])
        if order == 0:
            ordinary[key] = rec["ms_median"]
        else:
            rec["ratio_to_ordinary"] = rec["ms_median"] / ordinary[key]
        lines.append(rec)
        print(json.dumps(rec), flush=True)

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

    rng = np.random.default_rng(20261020)
    y = torch.from_numpy(rng.random((m, DIM))).cuda()
    d_s = torch.empty(m, dtype=torch.float64, device="cuda")
    d_v = torch.empty(m, dtype=torch.float64, device="cuda")
    d_g = torch.empty((m, DIM), dtype=torch.float64, device="cuda")
    for n in (4096, 16384):
        xh = rng.random((n, DIM))
        fh = 2.0 + np.sin(3.0 * xh[:, 0]) + np.cos(2.0 * xh[:, 1]) + xh[:, 0] - 2.0 * xh[:, 1]
        base = {"n": n, "dim": DIM, "kind": KIND, "nugget": NUGGET, "eps": n ** (1.0 / DIM)}
        for order in (0, 1, 2):
            si = pkg.Sinterp(KIND, DIM, n, 0)
            assert si.set_nugget(NUGGET) == 0 and si.set_drift(order) == 0
            emit("init", order, base, wall(lambda: si.init(xh, fh)))
            if n == 4096:
                emit("eval_value", order, {**base, "m": m}, wall(lambda: si.eval_resident(y.data_ptr(), m, DIM, d_s.data_ptr())))
                emit("eval_value_gradient", order, {**base, "m": m},
                     wall(lambda: si.eval_grad_resident(y.data_ptr(), m, DIM, d_s.data_ptr(), d_g.data_ptr(), DIM)))
                assert si.set_variance(1) == 0 and si.init(xh, fh) == 0
                mv = min(m, 10 ** 4)
                emit("variance", order, {**base, "m": mv}, wall(lambda: si.eval_variance_resident(y.data_ptr(), mv, DIM, d_v.data_ptr())))
            si.close()
    if not skip_local:
        n, k = 10 ** 6, 32
        xh = rng.random((n, DIM))
        fh = 2.0 + np.sin(3.0 * xh[:, 0]) + np.cos(2.0 * xh[:, 1])
        x, f = torch.from_numpy(xh).cuda(), torch.from_numpy(fh).cuda()
        eps = n ** (1.0 / DIM)
        base = {"n": n, "m": m, "k": k, "dim": DIM, "kind": KIND, "nugget": NUGGET, "eps": eps}
        ctx = pkg.HipContext.on_torch_stream(0)
        for order, entry in ((0, ctx.local_krige), (1, ctx.local_ukrige)):
            ms = []
            for r in range(WARM + REPS):
                ctx.timer_start()
                st, failed = entry(MATERN52, eps, NUGGET, x.data_ptr(), n, DIM, DIM, f.data_ptr(), y.data_ptr(), m, DIM, k, d_s.data_ptr(),
                                   d_v.data_ptr(), None, n)
                t = ctx.timer_stop()
                assert st in (0, pkg.GSL_EDOM)            # a neighbourhood that does not determine the drift is a count, not a stop
                if r >= WARM:
                    ms.append(t)
            emit("local", order, {**base, "failed": failed}, stats(ms))
        ctx.close()
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as fp:
        for rec in lines:
            fp.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
