"""Developer tool: time the leave-one-out diagonal (gsl_sinterp_hip_chol_inv_diag) and what it adds to an init.

For every N -- default 4096 and 16384 -- one child process (its own time limit; the parent stops at the first child that
fails) reports, as JSON lines, 2 warm-up + 7 timed runs each, the median:
  * chol_inv_diag alone on a resident factor for chunk in {1024, 2048, 4096, 8192, N}: event time, and (N^3 / 3) / time;
  * gsl_sinterp_hip_krige_variance with the N sites as targets (M = N, chunk 8192) in the same process: the existing
    M N^2 route to the same diagonal, N^3 flops;
  * gsl_sinterp_init with and without gsl_sinterp_set_loo for the Gaussian and the kriging type (wall clock: the init
    synchronises), and the add-on as a multiple of the init without it;
  * at N <= 4096 the largest deviation of g from diag(inv(K)) in numpy, relative to max g, for every chunk.
usage: python tools/loo_time.py [--out FILE] [N ...]
       python tools/loo_time.py --child N        one size, JSON lines on stdout"""
import json
import os
import sys
import time

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _R)
sys.path.insert(0, os.path.join(_R, "tests"))

WARM, REPS, DIM, NUGGET, VAR_CHUNK = 2, 7, 2, 1e-3, 8192
CHILD_LIMIT = {4096: 240, 16384: 540}                       # seconds per child


def median(v):
    return sorted(v)[len(v) // 2]


def child(n):
    import numpy as np
    import torch
    import __graft_entry__ as g
    import oracle_lib as orc
    pkg = g.load_package()
    ctx = pkg.HipContext.on_torch_stream(0)

    def timed(fn):
        for _ in range(WARM):
            fn()
        ms = []
        for _ in range(REPS):
            ctx.timer_start()
            fn()
            ms.append(ctx.timer_stop())
        return ms

    xs = orc.synth_centres(n, DIM)
    fs = orc.synth_response(xs)
    eps = 2.0 * n ** (1.0 / DIM)
    x, w = torch.from_numpy(xs).cuda(), torch.from_numpy(fs).cuda()
    phi = torch.empty((n, n), dtype=torch.float64, device="cuda")
    st, route, _ = ctx.krige_solve(0, eps, NUGGET, x.data_ptr(), n, DIM, DIM, phi.data_ptr(), n, w.data_ptr())
    assert st == 0 and route == 7, (st, route)
    want = None
    if n <= 4096:
        d2 = ((xs[:, None, :] - xs[None, :, :]) ** 2).sum(axis=2)
        want = np.diag(np.linalg.inv(np.exp(-eps * eps * d2) + NUGGET * np.eye(n)))
    gd = torch.empty(n, dtype=torch.float64, device="cuda")
    diag_ms = {}
    for chunk in sorted({1024, 2048, 4096, 8192, n}):
        if chunk > n:
            continue
        work = torch.empty(pkg.HipContext.chol_inv_diag_work(n, chunk), dtype=torch.float64, device="cuda")

        def call():
            assert ctx.chol_inv_diag(n, phi.data_ptr(), n, gd.data_ptr(), work.data_ptr(), chunk) == 0

        ms = timed(call)
        out = {"what": "chol_inv_diag", "n": n, "chunk": chunk, "ms_median": median(ms), "ms_all": ms,
               "gflops": n ** 3 / 3.0 / median(ms) / 1e6}
        if want is not None:
            ctx.sync()
            out["max_rel_err"] = float(np.abs(gd.cpu().numpy() - want).max() / want.max())
        diag_ms[chunk] = median(ms)
        print(json.dumps(out), flush=True)
        del work
    # the existing route to the same diagonal: the variance entry with the sites as targets
    b = torch.empty(n, dtype=torch.float64, device="cuda")
    dinv = torch.empty((n + 31) // 32 * 1024, dtype=torch.float64, device="cuda")
    st, denom = ctx.krige_variance_prepare(n, phi.data_ptr(), n, b.data_ptr(), dinv.data_ptr())
    assert st == 0
    work = torch.empty(pkg.HipContext.krige_variance_work(n, VAR_CHUNK), dtype=torch.float64, device="cuda")
    var = torch.empty(n, dtype=torch.float64, device="cuda")

    def call_var():
        assert ctx.krige_variance(0, eps, x.data_ptr(), n, DIM, DIM, phi.data_ptr(), n, b.data_ptr(), dinv.data_ptr(), denom,
                                  x.data_ptr(), n, DIM, var.data_ptr(), work.data_ptr(), VAR_CHUNK) == 0

    ms = timed(call_var)
    print(json.dumps({"what": "krige_variance_M=N", "n": n, "chunk": VAR_CHUNK, "ms_median": median(ms), "ms_all": ms,
                      "gflops": float(n) ** 3 / median(ms) / 1e6,
                      "over_chol_inv_diag": {str(c): median(ms) / t for c, t in diag_ms.items()}}), flush=True)
    del work, var, phi, b, dinv
    ctx.close()
    # the init with and without the switch
    for kind in ("gaussian", "kriging"):
        res = {}
        for loo in (0, 1):
            s = pkg.Sinterp(kind, DIM, n, 0)
            if kind == "kriging":
                assert s.set_nugget(NUGGET) == 0
            assert s.set_loo(loo) == 0
            ms = []
            for r in range(WARM + REPS):
                t0 = time.perf_counter()
                assert s.init(xs, fs) == 0
                if r >= WARM:
                    ms.append((time.perf_counter() - t0) * 1e3)
            assert s.route() in (1, 7)
            res[loo] = median(ms)
            s.close()
        print(json.dumps({"what": "init", "kind": kind, "n": n, "ms_without": res[0], "ms_with_loo": res[1],
                          "addon_over_init": (res[1] - res[0]) / res[0]}), flush=True)


if len(sys.argv) > 2 and sys.argv[1] == "--child":
    child(int(sys.argv[2]))
else:
    import subprocess
    args = sys.argv[1:]
    out_path = None
    if args and args[0] == "--out":
        out_path, args = args[1], args[2:]
    for n_ in [int(a) for a in args] or [4096, 16384]:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n_)], stdout=subprocess.PIPE, text=True,
                           timeout=CHILD_LIMIT.get(n_, 540))
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if out_path:
            with open(out_path, "a") as fp:
                fp.write(r.stdout)
        if r.returncode != 0:                               # nothing more is started on the GPU after a failure
            sys.exit(r.returncode if r.returncode > 0 else 1)
