"""Developer tool: time the joint covariance and the conditional simulation of kriging against the pointwise variance,
through the facade's resident entries (one Gaussian ordinary-kriging model per N, nugget 1e-3, 2-D).

For every N (default 4096 and 16384) and every M (default 1024 and 4096) it reports, as one JSON line per (N, M) appended
to profiles/krige_covariance_time.jsonl:
  * gsl_sinterp_eval_covariance_resident, one target set (M x M, symmetric), and gsl_sinterp_eval_variance_resident for the
    same M targets: ms (1 warm-up + REPS timed calls, host clock around a device synchronise; minimum and all), and the
    rates: M N^2 flops (the triangular substitution both share) over the variance's time, M N^2 + M^2 N (the lower half of
    the product added) over the covariance's;
  * gsl_sinterp_simulate_resident with 16 draws at jitter 1e-10 (covariance + Cholesky of the M x M matrix + the product);
  * the largest deviation of the covariance's diagonal from the variance entry on the same targets, and the largest
    asymmetry (0: the mirror), at the sizes timed.
usage: python tools/krige_covariance_time.py [--out FILE] [N:M ...]"""
import json
import os
import sys
import time

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _R)
sys.path.insert(0, os.path.join(_R, "tests"))
import numpy as np
import torch
import __graft_entry__ as g

pkg = g.load_package()
REPS, DIM, NUGGET, DRAWS, JITTER = 3, 2, 1e-3, 16, 1e-10


def timed(fn, reps):
    fn()                                                   # warm-up: code objects, workspaces, cached graphs
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return sorted(ms)


def run(n, sizes, out_path):
    rng = np.random.default_rng(n)
    x = rng.random((n, DIM))
    f = np.sin(3.0 * x[:, 0]) + np.cos(2.0 * x[:, 1]) + 2.0
    s = pkg.Sinterp("kriging", DIM, n, 0)
    assert s.set_nugget(NUGGET) == 0 and s.set_variance(1) == 0
    assert s.init(x, f) == 0 and s.route() == 7, s.route()
    for m in sizes:
        gen = torch.Generator(device="cuda").manual_seed(n + m)
        y = torch.rand((m, DIM), dtype=torch.float64, device="cuda", generator=gen)
        zn = torch.randn((m, DRAWS), dtype=torch.float64, device="cuda", generator=gen)
        cov = torch.empty((m, m), dtype=torch.float64, device="cuda")
        var = torch.empty(m, dtype=torch.float64, device="cuda")
        draws = torch.empty((m, DRAWS), dtype=torch.float64, device="cuda")

        def call_cov():
            assert s.eval_covariance_resident(y.data_ptr(), m, DIM, None, 0, 0, cov.data_ptr(), m) == 0

        def call_var():
            assert s.eval_variance_resident(y.data_ptr(), m, DIM, var.data_ptr()) == 0

        def call_sim():
            assert s.simulate_resident(y.data_ptr(), m, DIM, 1.0, JITTER, zn.data_ptr(), DRAWS, DRAWS, draws.data_ptr(), DRAWS) == 0

        t_var, t_cov, t_sim = timed(call_var, REPS), timed(call_cov, REPS), timed(call_sim, REPS)
        c, v = cov.cpu().numpy(), var.cpu().numpy()
        sub, prod = float(m) * n * n, float(m) * m * n
        out = {"n": n, "m": m, "draws": DRAWS, "jitter": JITTER, "nugget": NUGGET,
               "variance_ms_min": t_var[0], "variance_ms_all": t_var, "covariance_ms_min": t_cov[0], "covariance_ms_all": t_cov,
               "simulate_ms_min": t_sim[0], "simulate_ms_all": t_sim,
               "covariance_over_variance": t_cov[0] / t_var[0],
               "variance_gflops": sub / t_var[0] / 1e6, "covariance_gflops": (sub + prod) / t_cov[0] / 1e6,
               "product_over_substitution_flops": prod / sub,
               "max_abs_diag_minus_variance": float(np.abs(np.diag(c) - v).max()), "max_asymmetry": float(np.abs(c - c.T).max()),
               "draws_finite": bool(torch.isfinite(draws).all().item())}
        line = json.dumps(out)
        print(line, flush=True)
        with open(out_path, "a") as fp:
            fp.write(line + "\n")
    s.close()


if __name__ == "__main__":
    args = sys.argv[1:]
    out_path = os.path.join(_R, "profiles", "krige_covariance_time.jsonl")
    if args and args[0] == "--out":
        out_path, args = args[1], args[2:]
    specs = [tuple(int(v) for v in a.split(":")) for a in args] or [(4096, 1024), (4096, 4096), (16384, 1024), (16384, 4096)]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    for n_ in sorted({n for n, _ in specs}):
        run(n_, [m for n, m in specs if n == n_], out_path)
