"""Developer tool: time the model-selection entries (gsl_sinterp_fit_score / gsl_sinterp_fit_shape) against the loop over
gsl_sinterp_set_shape + gsl_sinterp_init that they replace.

Ordinary kriging with the Matern 5/2 covariance in 2-D, nugget 1e-3, the noisy response of tests/test_gpu_fit.py, at the
type's default shape e0 = sqrt(N).  For every N -- default 4096 and 16384 -- one child process (its own time limit; the
parent stops at the first child that fails) reports, as JSON lines, wall clock (every entry synchronises), 2 warm-up + 7
timed runs, the median:
  * (a) one FIT_ML evaluation and (b) one FIT_LOO evaluation on a resident workspace;
  * (c) the whole default search gsl_sinterp_fit_shape over [e0 / 8, 4 e0], for both criteria (one run each after one
    warm-up run), with its number of evaluations;
  * (d) gsl_sinterp_init at the same shape without and (e) with gsl_sinterp_set_loo: what a host-side loop pays per trial.
--init-only measures (d) and (e) alone and needs nothing this tool's commit added, so that --root DIR can point it at a
built checkout of an EARLIER commit (its package, oracle and libraries are then the ones loaded); --label tags the lines.
usage: python tools/fit_time.py [--out FILE] [--label TEXT] [--root DIR] [--init-only] [N ...]
       python tools/fit_time.py --child N [--init-only] [--label TEXT] [--root DIR]     one size, JSON lines on stdout"""
import json
import os
import sys
import time

WARM, REPS, DIM, NUGGET, KIND = 2, 7, 2, 1e-3, "kriging_matern52"
CHILD_LIMIT = {4096: 240, 16384: 540}                       # seconds per child


def take(args, flag, has_value):
    """remove `flag` (and its value) from args; returns the value, True, or None"""
    if flag not in args:
        return None
    i = args.index(flag)
    v = args[i + 1] if has_value else True
    del args[i:i + (2 if has_value else 1)]
    return v


def median(v):
    return sorted(v)[len(v) // 2]


def wall(fn, warm=WARM, reps=REPS):
    ms = []
    for r in range(warm + reps):
        t0 = time.perf_counter()
        fn()
        if r >= warm:
            ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def child(n, root, label, init_only):
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    import numpy as np
    import __graft_entry__ as g
    import oracle_lib as orc
    pkg = g.load_package()
    xs = orc.synth_centres(n, DIM)
    i = np.arange(n)
    fs = np.sin(3.0 * np.pi * xs[:, 0]) * np.cos(2.0 * np.pi * xs[:, 1]) + 0.35 * (((i + 1) * 0.6180339887498949) % 1.0 - 0.5)
    e0 = n ** (1.0 / DIM)
    base = {"n": n, "kind": KIND, "nugget": NUGGET, "eps": e0, "label": label}
    if not init_only:
        s = pkg.Sinterp(KIND, DIM, n, 0)
        fit = s.fit_workspace(xs, fs)
        for name, crit in (("ml", pkg.FIT_ML), ("loo", pkg.FIT_LOO)):
            def call():
                st, v = fit.score(crit, e0, NUGGET)
                assert st == 0 and np.isfinite(v), (st, v)
            ms = wall(call)
            print(json.dumps({"what": "fit_score", "criterion": name, **base, "ms_median": median(ms), "ms_all": ms}), flush=True)
        for name, crit in (("ml", pkg.FIT_ML), ("loo", pkg.FIT_LOO)):
            def search():
                st, best, v = fit.fit_shape(crit, e0 / 8, 4 * e0, NUGGET)
                assert st == 0, st
                return best, v
            ms = wall(search, warm=1, reps=1)
            best, v = search()
            st, _, scores = fit.trace()
            print(json.dumps({"what": "fit_shape", "criterion": name, **base, "lo": e0 / 8, "hi": 4 * e0, "ms": ms[0], "n_eval": fit.n_eval(),
                              "n_infinite": int(np.isinf(scores).sum()), "eps_best": best, "score_best": v}), flush=True)
        fit.close()
        s.close()
    res = {}
    for loo in (0, 1):
        s = pkg.Sinterp(KIND, DIM, n, 0)
        assert s.set_nugget(NUGGET) == 0 and s.set_shape(e0) == 0 and s.set_loo(loo) == 0

        def init():
            assert s.init(xs, fs) == 0

        res[loo] = wall(init)
        assert s.route() == 7
        s.close()
    print(json.dumps({"what": "init", **base, "ms_without": median(res[0]), "ms_with_loo": median(res[1]), "ms_all_without": res[0],
                      "ms_all_with_loo": res[1]}), flush=True)


args = sys.argv[1:]
root_ = os.path.abspath(take(args, "--root", True) or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
label_ = take(args, "--label", True) or ""
init_only_ = bool(take(args, "--init-only", False))
out_path = take(args, "--out", True)
child_n = take(args, "--child", True)
if child_n is not None:
    child(int(child_n), root_, label_, init_only_)
else:
    import subprocess
    for n_ in [int(a) for a in args] or [4096, 16384]:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(n_), "--root", root_, "--label", label_]
        r = subprocess.run(cmd + (["--init-only"] if init_only_ else []), stdout=subprocess.PIPE, text=True, timeout=CHILD_LIMIT.get(n_, 540))
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if out_path:
            with open(out_path, "a") as fp:
                fp.write(r.stdout)
        if r.returncode != 0:                               # nothing more is started on the GPU after a failure
            sys.exit(r.returncode if r.returncode > 0 else 1)
