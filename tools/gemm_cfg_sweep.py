"""Developer tool: every trailing-update shape of the recursive Cholesky at N = 4096, 8192 and 16384 (the launches
chol_panel in csrc/hip/chol.hip issues) under each tile configuration and split policy the dispatcher can be forced
into (GSL_SINTERP_GEMM_CFG, csrc/hip/gemm.hip): 0 = 256x128 (8 waves), 1 = 128x128 (4 waves), 2 = 64x64 (4 waves),
5 = 128x128 (8 waves), 6 = 64x64 (8 waves, 4-step groups); suffix "w" = whole tiles only (no K split), none = the
hybrid split.  Prints one line per (variant, shape) and, per N and K level, the time of
the default rule, of the round-4 rule and of the best variant of every shape.
usage: python tools/gemm_cfg_sweep.py [N ...]"""
import json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PB = 128
VARIANTS = ["0", "0w", "1", "1w", "2", "2w", "5", "5w", "6", "6w"]


def shapes_of(N):
    def split(w):
        unit = PB if w > PB else 32
        w1 = ((w // 2 + unit - 1) // unit) * unit
        return w1 if w1 < w else w - unit
    out = []
    def panel(j0, w):
        if w <= PB:
            return
        w1 = split(w)
        panel(j0, w1)
        r0, w2 = j0 + w1, w - w1
        out.append((N - r0, w2, w1))
        panel(r0, w2)
    panel(0, N)
    return out


def allowed(cfg, m, n):
    if cfg == "0":                          # 256-row tiles: rows split evenly, even count of 128-columns in the lower case
        tn = min(n // 128, m // 128)
        return m % 256 == 0 and tn % 2 == 0
    return True


if len(sys.argv) > 1 and sys.argv[1] == "child":
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import __graft_entry__ as g
    pkg = g.load_package()
    ctx = pkg.HipContext.on_torch_stream(0)
    var = sys.argv[2]
    for N in [int(v) for v in sys.argv[3:]]:
        a = torch.randn((N, N), dtype=torch.float64, device="cuda")
        seen = {}
        for (m, n, k) in shapes_of(N):
            if var not in ("rule", "r4") and not allowed(var.rstrip("w"), m, n):
                continue
            if (m, n, k) in seen:
                continue
            pa = a.data_ptr() + ((N - m) * N) * 8
            pc = pa + k * 8
            ctx.gemm_minus(m, n, k, pa, N, pa, N, 0, pc, N, 1)
            reps = 2 if k >= 2048 else 5
            ctx.timer_start()
            for _ in range(reps):
                ctx.gemm_minus(m, n, k, pa, N, pa, N, 0, pc, N, 1)
            seen[(m, n, k)] = ctx.timer_stop() / reps
        for (m, n, k), ms in seen.items():
            print(json.dumps({"var": var, "N": N, "m": m, "n": n, "k": k, "us": ms * 1e3}))
        del a
        torch.cuda.empty_cache()
else:
    Ns = [int(v) for v in sys.argv[1:]] or [4096, 8192, 16384]
    rows = []
    for var in ["rule", "r4"] + VARIANTS:
        env = dict(os.environ)
        env.pop("GSL_SINTERP_GEMM_CFG", None); env.pop("GSL_SINTERP_GEMM_RULE_R4", None)
        if var == "r4":
            env["GSL_SINTERP_GEMM_RULE_R4"] = "1"
        elif var != "rule":
            env["GSL_SINTERP_GEMM_CFG"] = var
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", var] + [str(v) for v in Ns], env=env, cwd=ROOT,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        if r.returncode != 0:
            print(f"variant {var}: exit {r.returncode}\n{r.stdout[-2000:]}")
            sys.exit(1)
        for line in r.stdout.splitlines():
            if line.startswith("{"):
                rows.append(json.loads(line))
                d = rows[-1]
                print(f"{d['var']:>4} N={d['N']:5d} m={d['m']:6d} n={d['n']:5d} k={d['k']:5d} {d['us']:9.1f} us")
        sys.stdout.flush()
    by = {}
    for d in rows:
        by.setdefault((d["N"], d["m"], d["n"], d["k"]), {})[d["var"]] = d["us"]
    print("\nper shape: best variant (us), default rule, round-4 rule")
    for N in Ns:
        lev = {}
        for (NN, m, n, k), v in sorted(by.items(), key=lambda t: (t[0][0], -t[0][3], -t[0][1])):
            if NN != N:
                continue
            cand = {kk: vv for kk, vv in v.items() if kk not in ("rule", "r4")}
            best = min(cand, key=cand.get)
            print(f"N={N:5d} m={m:6d} n={n:5d} k={k:5d}  best {best:>3} {cand[best]:9.1f}  rule {v['rule']:9.1f}  r4 {v['r4']:9.1f}  "
                  + " ".join(f"{kk}:{cand[kk]:.1f}" for kk in VARIANTS if kk in cand))
        # level totals over the recursion's launches (repeated shapes counted as often as they occur)
        for (m, n, k) in shapes_of(N):
            v = by[(N, m, n, k)]
            cand = {kk: vv for kk, vv in v.items() if kk not in ("rule", "r4")}
            t = lev.setdefault(k, [0.0, 0.0, 0.0])
            t[0] += v["rule"]; t[1] += v["r4"]; t[2] += min(cand.values())
        print(f"N={N}: per level (ms)  rule / round-4 rule / best per shape")
        for k in sorted(lev, reverse=True):
            t = lev[k]
            print(f"  K={k:5d}  {t[0] / 1e3:8.3f}  {t[1] / 1e3:8.3f}  {t[2] / 1e3:8.3f}")
        print("  all    %8.3f  %8.3f  %8.3f" % tuple(sum(t[i] for t in lev.values()) / 1e3 for i in range(3)))
