"""Developer tool: what a further field costs.  Times, on resident buffers with the context's event timer,
  * one fields sweep (gsl_sinterp_hip_rbf_eval_fields) against K calls of the scalar sweep (gsl_sinterp_hip_rbf_eval_model)
    on the K columns, at the benchmark's C2 shape (thin-plate, 2-D, N = 4096, M = 10^6) and C4 shape (Gaussian, 2-D,
    N = 8192, M = 10^7) for K in 2, 4, 8, 16, and
  * gsl_sinterp_init_fields against K calls of gsl_sinterp_init at N = 4096 (Gaussian: the shared factorisation; thin-plate:
    the per-field route), host wall clock around the whole entry,
and prints one JSON line per measurement with the ratio fields / K scalar.  The expectation from the instruction count (a
further field is one FMA and one select per pair next to ~22 VALU instructions of distance, take test and phi) is a ratio
far below 1; a ratio >= 1 for some K is a finding to act on in rbf_sweep_dispatch.

Each call is a whole entry (target sort + sweep; the packed centres are cached by model_id after the warm-up).  WARMUP
untimed calls, then REPS timed ones; min, median and max are reported (the median is the number to quote).  Centres,
weights and targets are uniform random: a timing run, the tests check the numbers.
usage: python tools/rbf_fields_time.py [kind:N:M ...] [init]     kind = gaussian | tps | wendland; default: both shapes + init"""
import json
import os
import sys
import time

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _R)
import numpy as np
import torch
import __graft_entry__ as g

pkg = g.load_package()
KINDS = {"gaussian": 0, "tps": 1, "wendland": 2}
DIM, WARMUP, REPS, KS = 2, 2, 7, (2, 4, 8, 16)


def stats(ms):
    ms = sorted(ms)
    return {"min": ms[0], "median": ms[len(ms) // 2], "max": ms[-1]}


def timed(ctx, fn):
    for _ in range(WARMUP):
        fn()
    ctx.sync()
    ms = []
    for _ in range(REPS):
        ctx.timer_start()
        fn()
        ms.append(ctx.timer_stop())
    return stats(ms)


def sweep(ctx, name, n, m):
    kind = KINDS[name]
    gen = torch.Generator(device="cuda").manual_seed(n)
    x = torch.rand((n, DIM), dtype=torch.float64, device="cuda", generator=gen)
    y = torch.rand((m, DIM), dtype=torch.float64, device="cuda", generator=gen)
    eps = (0.125 if kind == 2 else 2.0) * n ** (1.0 / DIM)
    for k in KS:
        w = torch.randn((k, n), dtype=torch.float64, device="cuda", generator=gen)
        s1 = torch.empty(m, dtype=torch.float64, device="cuda")
        sk = torch.empty((m, k), dtype=torch.float64, device="cuda")

        def scalar_k():                                              # ids 1 .. k: every column's packed centres stay one call long
            for q in range(k):
                ctx.rbf_eval(kind, eps, x.data_ptr(), n, DIM, DIM, w.data_ptr() + 8 * q * n, y.data_ptr(), m, DIM, s1.data_ptr(), model_id=1 + q)

        def fields():
            st = ctx.rbf_eval_fields(kind, eps, x.data_ptr(), n, DIM, DIM, w.data_ptr(), n, k, y.data_ptr(), m, DIM, sk.data_ptr(), k,
                                     model_id=100 + k)
            assert st == 0, st

        out = {"what": "sweep", "kind": name, "n": n, "m": m, "dim": DIM, "k": k, "nf_block": pkg.HipContext.rbf_fields_block(),
               "warmup": WARMUP, "reps": REPS, "scalar_k_ms": timed(ctx, scalar_k), "fields_ms": timed(ctx, fields)}
        out["scalar_1_ms_median"] = out["scalar_k_ms"]["median"] / k
        out["ratio_fields_over_k_scalar"] = out["fields_ms"]["median"] / out["scalar_k_ms"]["median"]
        out["fields_in_scalar_sweeps"] = out["fields_ms"]["median"] / out["scalar_1_ms_median"]
        print(json.dumps(out), flush=True)


def init(name, n):
    rng = np.random.default_rng(n)
    x = rng.random((n, DIM))
    for k in KS:
        F = np.ascontiguousarray(rng.standard_normal((n, k)))
        cols = [np.ascontiguousarray(F[:, q]) for q in range(k)]
        s = pkg.Sinterp(name, DIM, n, 0)

        def wall(fn):
            ms = []
            for i in range(WARMUP + REPS):
                t0 = time.perf_counter()
                fn()
                if i >= WARMUP:
                    ms.append(1e3 * (time.perf_counter() - t0))
            return stats(ms)

        def k_inits():
            for q in range(k):
                assert s.init(x, cols[q]) == 0

        def one_init_fields():
            assert s.init_fields(x, F) == 0

        out = {"what": "init", "kind": name, "n": n, "dim": DIM, "k": k, "warmup": WARMUP, "reps": REPS,
               "k_inits_ms": wall(k_inits), "init_fields_ms": wall(one_init_fields), "route": s.route()}
        out["ratio_fields_over_k_inits"] = out["init_fields_ms"]["median"] / out["k_inits_ms"]["median"]
        print(json.dumps(out), flush=True)
        s.close()


if __name__ == "__main__":
    args = sys.argv[1:] or ["tps:4096:1000000", "gaussian:8192:10000000", "init"]
    ctx = pkg.HipContext.on_torch_stream(0)
    for spec in args:
        if spec == "init":
            init("gaussian", 4096)
            init("tps", 4096)
        else:
            name, n_, m_ = spec.split(":")
            sweep(ctx, name, int(n_), int(m_))
    ctx.close()
