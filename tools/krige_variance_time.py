"""Developer tool: time the kriging variance (gsl_sinterp_hip_krige_variance) with the context's event timer.

For every (N, M) -- default 4096 x 65536 and 16384 x 16384, chunk = 8192 -- it reports
  * the whole call: ms and M N^2 / time in GFLOP/s, 1 warm-up + REPS timed calls, for the left-looking width-128 recursion
    (the default) and for wider panels.  GSL_SINTERP_KRIGE_PANEL is read once per process, so every variant runs in a
    fresh child process, the default first and again last (the spread between those two is the noise);
  * the isolated GEMM of the same shape class, gemm_minus at m = chunk, n = 128, k = N / 2, for comparison with the
    update kernels' rate (tools/krige_variance_split.py gives their time from a kernel trace);
  * at N <= 4096 the largest deviation from the numpy formula on 256 targets, for every variant (faster and different
    is not faster).
usage: python tools/krige_variance_time.py [N:M ...]
       python tools/krige_variance_time.py --child N:M     one variant (the environment's), one JSON line
       rocprofv3 --kernel-trace -d DIR -o t --output-format csv -- python tools/krige_variance_time.py --trace N:M
           two calls and nothing else, then: python tools/krige_variance_split.py DIR N:M"""
import json
import os
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _R)
sys.path.insert(0, os.path.join(_R, "tests"))
import numpy as np
import torch
import __graft_entry__ as g

pkg = g.load_package()
ctx = None                                                 # the children open the GPU, the parent does not
CHUNK, REPS, DIM, NUGGET = 8192, 3, 2, 1e-3


def timed(fn, reps):
    fn()                                                   # warm-up: code objects, workspaces, cached graphs
    ms = []
    for _ in range(reps):
        ctx.timer_start()
        fn()
        ms.append(ctx.timer_stop())
    return ms


def run(n, m, trace_only=False):
    gen = torch.Generator(device="cuda").manual_seed(n)
    x = torch.rand((n, DIM), dtype=torch.float64, device="cuda", generator=gen)
    y = torch.rand((m, DIM), dtype=torch.float64, device="cuda", generator=gen)
    w = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen)
    eps = 2.0 * n ** (1.0 / DIM)
    phi = torch.empty((n, n), dtype=torch.float64, device="cuda")
    st, route, _ = ctx.krige_solve(0, eps, NUGGET, x.data_ptr(), n, DIM, DIM, phi.data_ptr(), n, w.data_ptr())
    assert st == 0 and route == 7, (st, route)
    b = torch.empty(n, dtype=torch.float64, device="cuda")
    dinv = torch.empty((n + 31) // 32 * 1024, dtype=torch.float64, device="cuda")
    st, denom = ctx.krige_variance_prepare(n, phi.data_ptr(), n, b.data_ptr(), dinv.data_ptr())
    assert st == 0
    work = torch.empty(pkg.HipContext.krige_variance_work(n, CHUNK), dtype=torch.float64, device="cuda")
    var = torch.empty(m, dtype=torch.float64, device="cuda")

    def call():
        st = ctx.krige_variance(0, eps, x.data_ptr(), n, DIM, DIM, phi.data_ptr(), n, b.data_ptr(), dinv.data_ptr(), denom,
                                y.data_ptr(), m, DIM, var.data_ptr(), work.data_ptr(), CHUNK)
        assert st == 0, st

    want = None
    if n <= 4096:
        xs, ys = x.cpu().numpy(), y[:256].cpu().numpy()
        d2 = lambda a, c: ((a[:, None, :] - c[None, :, :]) ** 2).sum(axis=2)
        K = np.exp(-eps * eps * d2(xs, xs)) + NUGGET * np.eye(n)
        k = np.exp(-eps * eps * d2(ys, xs)).T
        bb = np.linalg.solve(K, np.ones(n))
        want = 1.0 - (k * np.linalg.solve(K, k)).sum(axis=0) + (1.0 - bb @ k) ** 2 / bb.sum()

    if trace_only:
        call(); call()
        ctx.sync()
        return
    flops = float(m) * n * n
    out = {"n": n, "m": m, "chunk": CHUNK, "panel": os.environ.get("GSL_SINTERP_KRIGE_PANEL", "128")}
    call()
    ctx.sync()
    if want is not None:
        out["max_abs_err_256"] = float(np.abs(var[:256].cpu().numpy() - want).max())
    ms = sorted(timed(call, REPS))
    out.update({"ms_min": ms[0], "ms_median": ms[len(ms) // 2], "ms_all": ms, "gflops": flops / ms[0] / 1e6})
    # the isolated update of the middle of the recursion: m = chunk rows, one 128-column block, K = N / 2
    kk = n // 2
    a = torch.randn((CHUNK, kk), dtype=torch.float64, device="cuda", generator=gen)
    bm = torch.randn((128, kk), dtype=torch.float64, device="cuda", generator=gen)
    c = torch.randn((CHUNK, 128), dtype=torch.float64, device="cuda", generator=gen)
    one = min(timed(lambda: ctx.gemm_minus(CHUNK, 128, kk, a.data_ptr(), kk, bm.data_ptr(), kk, 0, c.data_ptr(), 128, 0), 5))
    out["gemm_one"] = {"m": CHUNK, "n": 128, "k": kk, "ms": one, "gflops": 2.0 * CHUNK * 128 * kk / one / 1e6}
    print(json.dumps(out), flush=True)


if len(sys.argv) > 2 and sys.argv[1] in ("--child", "--trace"):
    n_, m_ = (int(v) for v in sys.argv[2].split(":"))
    ctx = pkg.HipContext.on_torch_stream(0)
    run(n_, m_, sys.argv[1] == "--trace")
    ctx.close()
else:
    import subprocess
    for spec in sys.argv[1:] or ["4096:65536", "16384:16384"]:
        n_ = int(spec.split(":")[0])
        for panel in ("128", "1024", str(n_), "128"):
            env = dict(os.environ)
            env.pop("GSL_SINTERP_KRIGE_PANEL", None)
            if panel != "128":
                env["GSL_SINTERP_KRIGE_PANEL"] = panel
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", spec], env=env, check=True, timeout=300)
