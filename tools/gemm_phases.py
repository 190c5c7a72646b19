"""Developer tool: phase cycle stamps of gemm_minus_streamk_kernel (libgsl_sinterp_prof.so, `make prof`) at trailing-update
shapes of the recursive Cholesky, operands laid out as tools/gemm_cfg_sweep.py lays them out (N = 16384).  Per launch:
the workgroups' mean time in each phase -- prologue (segment start to the first MFMA: ring fill, C prefetch), K loop,
exchange (non-owner: partial publish; owner: fix-up wait + partial reads), C epilogue -- and, from the 100 MHz clock,
the spread of start times and the mean time a workgroup sits finished while others still run (tail).
usage: python tools/gemm_phases.py [variant ...]   (variant: rule, r4, or a GSL_SINTERP_GEMM_CFG value)"""
import ctypes as C, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(8192, 128, 128), (16128, 256, 256), (8192, 512, 512), (8192, 1024, 1024), (12288, 2048, 2048)]
# the seven launches of the 256x128 tile in the N = 16384 recursion (K = 8192, 4096, 2048; tools/chol_levels.py)
SHAPES += [(8192, 8192, 8192), (12288, 4096, 4096), (4096, 4096, 4096),
           (14336, 2048, 2048), (10240, 2048, 2048), (6144, 2048, 2048), (2048, 2048, 2048)]

if len(sys.argv) > 1 and sys.argv[1] == "child":
    os.environ.setdefault("GSL_SINTERP_LIBRARY", os.path.join(ROOT, "gsl-scattered-interpolation_amd", "libgsl_sinterp_prof.so"))
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np, torch
    import __graft_entry__ as g
    pkg = g.load_package()
    lib = pkg.capi.lib()
    ctx = pkg.HipContext.on_torch_stream(0)
    var = sys.argv[2]
    N = 16384
    a = torch.randn((N, N), dtype=torch.float64, device="cuda")
    buf = (C.c_ulonglong * (1024 * 8))()
    for (m, n, k) in SHAPES:
        pa = a.data_ptr() + ((N - m) * N) * 8
        pc = pa + k * 8
        for _ in range(3):
            ctx.gemm_minus(m, n, k, pa, N, pa, N, 0, pc, N, 1)
        ctx.sync()
        assert lib.gsl_sinterp_hip_debug_gemm_ts_clear() == 0
        ctx.gemm_minus(m, n, k, pa, N, pa, N, 0, pc, N, 1)
        ctx.sync()
        assert lib.gsl_sinterp_hip_debug_gemm_ts(buf) == 0
        v = np.frombuffer(buf, dtype=np.uint64).reshape(1024, 8).astype(np.float64)
        v = v[v[:, 1] > 0]
        span = v[:, 1] - v[:, 0]
        rspan = (v[:, 7] - v[:, 6]) * 1e-2                       # us (100 MHz)
        ghz = np.median(span / (v[:, 7] - v[:, 6]) * 0.1)       # shader clock of the stamps
        us = lambda c: c / (ghz * 1e3)
        ph = [us(v[:, 2 + i]).mean() for i in range(4)]
        tail = (v[:, 7].max() - v[:, 7]).mean() * 1e-2
        skew = (v[:, 6].max() - v[:, 6].min()) * 1e-2
        print(f"{var:>4} m={m:6d} n={n:5d} k={k:5d}  G={len(v):3d}  span {rspan.mean():7.1f} us (max {rspan.max():7.1f})  "
              f"prologue {ph[0]:6.1f}  kloop {ph[1]:7.1f}  exchange {ph[2]:6.1f}  epilogue {ph[3]:6.1f}  "
              f"start skew {skew:5.1f}  tail {tail:6.1f}  ({ghz:.2f} GHz)")
        sys.stdout.flush()
else:
    for var in sys.argv[1:] or ["rule", "r4"]:
        env = dict(os.environ)
        env.pop("GSL_SINTERP_GEMM_CFG", None); env.pop("GSL_SINTERP_GEMM_RULE_R4", None)
        if var == "r4":
            env["GSL_SINTERP_GEMM_RULE_R4"] = "1"
        elif var != "rule":
            env["GSL_SINTERP_GEMM_CFG"] = var
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", var], env=env, cwd=ROOT,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        print(r.stdout[-6000:])
        if r.returncode != 0:
            print(f"variant {var}: exit {r.returncode}")
            sys.exit(1)
