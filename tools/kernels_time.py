"""Developer tool: time the plain sweep and the fill of the Matern 3/2, Matern 5/2 and inverse multiquadric kinds beside the
thin-plate plain sweep -- the yardstick: the same kernel body, every centre for every target, with log_tbl where the new
kinds have sqrt + exp2_tbl (Matern) or sqrt + a division (inverse multiquadric).

For every N -- default 4096, the C2 shape: 2-D, M = 10^6 targets -- one child process (its own time limit; the parent stops
at the first child that fails) reports, as JSON lines, 2 warm-up + 7 timed runs each, event time on resident buffers, the
median:
  * gsl_sinterp_hip_rbf_eval (value sweep, two targets per lane at this M) per kind, in ms, in picoseconds per
    (target, centre) pair over the whole device, and as a multiple of the thin-plate sweep;
  * gsl_sinterp_hip_rbf_eval_grad (value + gradient) the same way;
  * gsl_sinterp_hip_rbf_fill (both triangles) per kind, in ms and in GB/s of matrix written.
The weights are random: a sweep's time does not depend on them.
usage: python tools/kernels_time.py [--out FILE] [--targets M] [N ...]
       python tools/kernels_time.py --child N M      one size, JSON lines on stdout"""
import json
import os
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _R)
sys.path.insert(0, os.path.join(_R, "tests"))

WARM, REPS, DIM = 2, 7, 2
KINDS = {"thin-plate": 1, "matern32": 3, "matern52": 4, "imq": 5}            # the plain-sweep kinds
FILL_KINDS = {"gaussian": 0, "thin-plate": 1, "wendland": 2, "matern32": 3, "matern52": 4, "imq": 5}
CHILD_LIMIT = 300                                                          # seconds per child


def median(v):
    return sorted(v)[len(v) // 2]


def child(n, m):
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

    eps = n ** (1.0 / DIM)
    x = torch.from_numpy(orc.synth_centres(n, DIM)).cuda()
    y = torch.from_numpy(orc.synth_targets(0, m, DIM)).cuda()
    w = torch.from_numpy(np.random.default_rng(1).standard_normal(n)).cuda()
    s = torch.empty(m, dtype=torch.float64, device="cuda")
    gr = torch.empty((m, DIM), dtype=torch.float64, device="cuda")
    base = {}
    for what in ("sweep", "sweep_grad"):
        for name, kind in KINDS.items():
            if what == "sweep":
                def call():
                    ctx.rbf_eval(kind, eps, x.data_ptr(), n, DIM, DIM, w.data_ptr(), y.data_ptr(), m, DIM, s.data_ptr())
            else:
                def call():
                    assert ctx.rbf_eval_grad(kind, eps, x.data_ptr(), n, DIM, DIM, w.data_ptr(), y.data_ptr(), m, DIM, s.data_ptr(),
                                             gr.data_ptr(), DIM) == 0
            ms = timed(call)
            ctx.sync()
            assert bool(torch.isfinite(s).all())
            base.setdefault(what, median(ms))                              # thin-plate comes first
            print(json.dumps({"what": what, "kind": name, "n": n, "m": m, "dim": DIM, "eps": eps, "ms_median": median(ms), "ms_all": ms,
                              "ps_per_pair": median(ms) * 1e9 / (float(n) * m), "over_thin_plate": median(ms) / base[what]}), flush=True)
    phi = torch.empty((n, n), dtype=torch.float64, device="cuda")
    for name, kind in FILL_KINDS.items():
        e = {0: 2.0 * eps, 2: eps / 8.0}.get(kind, eps)                    # each kind at its default shape

        def call():
            ctx.rbf_fill(kind, e, x.data_ptr(), n, DIM, DIM, phi.data_ptr(), n)

        ms = timed(call)
        print(json.dumps({"what": "fill", "kind": name, "n": n, "dim": DIM, "eps": e, "ms_median": median(ms), "ms_all": ms,
                          "gb_per_s": 8.0 * n * n / median(ms) / 1e6}), flush=True)
    ctx.close()


if len(sys.argv) > 3 and sys.argv[1] == "--child":
    child(int(sys.argv[2]), int(sys.argv[3]))
else:
    import subprocess
    args = sys.argv[1:]
    out_path, m_ = None, 1000000
    while args and args[0] in ("--out", "--targets"):
        if args[0] == "--out":
            out_path = args[1]
        else:
            m_ = int(args[1])
        args = args[2:]
    for n_ in [int(a) for a in args] or [4096]:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n_), str(m_)], stdout=subprocess.PIPE, text=True,
                           timeout=CHILD_LIMIT)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if out_path:
            with open(out_path, "a") as fp:
                fp.write(r.stdout)
        if r.returncode != 0:                               # nothing more is started on the GPU after a failure
            sys.exit(r.returncode if r.returncode > 0 else 1)
