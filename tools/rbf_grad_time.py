"""Developer tool: what the gradient costs.  Times, on resident buffers with the context's event timer,
  * the value sweep (gsl_sinterp_hip_rbf_eval_model) and
  * the fused value + gradient sweep (gsl_sinterp_hip_rbf_eval_grad), with and without the value output,
at the benchmark's C2 shape (thin-plate, 2-D, N = 4096, M = 10^6) and C4 shape (Gaussian, 2-D, N = 8192, M = 10^7), and
prints one JSON line per shape with the ratio grad / value.  A gradient built from the value sweep alone (central
differences) costs 2 dim more sweeps, an analytic one at least dim + 1 sweeps' worth of kernel evaluations: the fused sweep
has to stay below dim + 1.

Each call is a whole entry (target sort + sweep; the packed centres are cached by model_id after the warm-up).  WARMUP
untimed calls, then REPS timed ones; min and median are reported (the median is the number to quote, the spread
min .. max is the noise).  Centres, weights and targets are uniform random: a timing run, the tests check the numbers.
usage: python tools/rbf_grad_time.py [kind:N:M ...]      kind = gaussian | tps | wendland, default tps:4096:1000000
                                                         gaussian:8192:10000000"""
import json
import os
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _R)
import torch
import __graft_entry__ as g

pkg = g.load_package()
KINDS = {"gaussian": 0, "tps": 1, "wendland": 2}
DIM, WARMUP, REPS = 2, 2, 7


def timed(ctx, fn):
    for _ in range(WARMUP):
        fn()
    ctx.sync()
    ms = []
    for _ in range(REPS):
        ctx.timer_start()
        fn()
        ms.append(ctx.timer_stop())
    ms.sort()
    return {"min": ms[0], "median": ms[len(ms) // 2], "max": ms[-1]}


def run(ctx, name, n, m):
    kind = KINDS[name]
    gen = torch.Generator(device="cuda").manual_seed(n)
    x = torch.rand((n, DIM), dtype=torch.float64, device="cuda", generator=gen)
    y = torch.rand((m, DIM), dtype=torch.float64, device="cuda", generator=gen)
    w = torch.randn(n, dtype=torch.float64, device="cuda", generator=gen)
    s = torch.empty(m, dtype=torch.float64, device="cuda")
    grad = torch.empty((m, DIM), dtype=torch.float64, device="cuda")
    eps = (0.125 if kind == 2 else 2.0) * n ** (1.0 / DIM)

    def value():
        ctx.rbf_eval(kind, eps, x.data_ptr(), n, DIM, DIM, w.data_ptr(), y.data_ptr(), m, DIM, s.data_ptr(), model_id=1)

    def value_grad(d_s):
        st = ctx.rbf_eval_grad(kind, eps, x.data_ptr(), n, DIM, DIM, w.data_ptr(), y.data_ptr(), m, DIM, d_s, grad.data_ptr(), DIM,
                               model_id=1)
        assert st == 0, st

    out = {"kind": name, "n": n, "m": m, "dim": DIM, "warmup": WARMUP, "reps": REPS,
           "value_ms": timed(ctx, value),
           "value_grad_ms": timed(ctx, lambda: value_grad(s.data_ptr())),
           "grad_only_ms": timed(ctx, lambda: value_grad(None)),
           "value_again_ms": timed(ctx, value)}                      # the first measurement repeated: drift of the session
    out["ratio_median"] = out["value_grad_ms"]["median"] / out["value_ms"]["median"]
    out["floor_dim_plus_1"] = DIM + 1
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ctx = pkg.HipContext.on_torch_stream(0)
    for spec in sys.argv[1:] or ["tps:4096:1000000", "gaussian:8192:10000000"]:
        name, n_, m_ = spec.split(":")
        run(ctx, name, int(n_), int(m_))
    ctx.close()
