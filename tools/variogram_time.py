"""Developer tool: time the empirical variogram (gsl_sinterp_hip_variogram) and the host-side model fit.

2-D uniform clouds in the unit square, 15 bins, f = a smooth function plus noise; resident buffers; 2 warm-up + 7 timed runs,
median and spread.
  * device-event time of one gsl_sinterp_hip_variogram call (range pass, binning, pair kernel, 840 bytes back; the entry
    synchronises), the pairs it tested and the pairs it binned, hence pairs tested per second:
      N = 16384 with the default cut-off (a third of the box diagonal), N = 10^6 with h_max = 0.02 and 0.1 of the box side;
  * wall clock of gsl_sinterp_variogram_fit (Matheron, N_b / h^2, default bracket and search) on the variogram just computed:
    host arithmetic on 15 numbers.
One JSON line per measurement, appended to --out (default profiles/variogram_time.jsonl).
usage: python tools/variogram_time.py [--out FILE] [--bins B]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM, REPS, DIM = 2, 7, 2
CONFIGS = [(16384, None), (10 ** 6, 0.02), (10 ** 6, 0.1)]      # (N, h_max; None = the facade's default)


def stats(ms):
    s = sorted(ms)
    return {"ms_median": s[len(s) // 2], "ms_min": s[0], "ms_max": s[-1], "ms_all": ms}


def main():
    args = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "variogram_time.jsonl")
    n_bins = 15
    if "--out" in args:
        i = args.index("--out"); out = args[i + 1]; del args[i:i + 2]
    if "--bins" in args:
        i = args.index("--bins"); n_bins = int(args[i + 1]); del args[i:i + 2]
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

    rng = np.random.default_rng(20261021)
    for n, h_max in CONFIGS:
        xh = rng.random((n, DIM))
        fh = 2.0 + np.sin(3.0 * xh[:, 0]) + np.cos(2.0 * xh[:, 1]) + 0.1 * rng.standard_normal(n)
        x, f = torch.from_numpy(xh).cuda(), torch.from_numpy(fh).cuda()
        v = pkg.Variogram(DIM, n_bins, device=0)
        assert v.compute_resident(x.data_ptr(), n, DIM, f.data_ptr(), h_max or 0.0) == 0
        h = v.h_max()
        base = {"n": n, "dim": DIM, "n_bins": n_bins, "h_max": h, "h_max_default": h_max is None}
        ctx = pkg.HipContext.on_torch_stream(0)
        ms, acc = [], None
        for r in range(WARM + REPS):
            ctx.timer_start()
            st, acc, _ = ctx.variogram(x.data_ptr(), n, DIM, DIM, f.data_ptr(), h, n_bins)
            t = ctx.timer_stop()
            assert st == 0
            if r >= WARM:
                ms.append(t)
        rec = stats(ms)
        tested, binned = ctx.variogram_pairs_tested(), int(acc[:, 0].sum())
        emit({"what": "variogram", **base, **rec, "pairs_tested": tested, "pairs_binned": binned, "pairs_all": n * (n - 1) // 2,
              "pairs_tested_per_s": tested / (rec["ms_median"] * 1e-3), "pairs_binned_per_s": binned / (rec["ms_median"] * 1e-3)})
        ctx.close()
        ws, res = [], None
        for r in range(WARM + REPS):
            t0 = time.perf_counter()
            res = v.fit("kriging_matern32", pkg.Variogram.MATHERON, pkg.Variogram.W_COUNT_H2)
            if r >= WARM:
                ws.append((time.perf_counter() - t0) * 1e3)
        emit({"what": "variogram_fit_host", **base, **stats(ws), "status": res[0], "eps": res[1], "nugget": res[2], "sigma2": res[3],
              "n_eval": int(pkg.lib().gsl_sinterp_variogram_fit_model_n_eval())})
        v.close()
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as fp:
        for rec in lines:
            fp.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
