#!/usr/bin/env python3
"""Developer tool: where the time of one kriging-variance call goes, from a rocprofv3 --kernel-trace CSV of
`tools/krige_variance_time.py --trace N:M` (see there): the kernels of the LAST call, grouped into fill, GEMM updates,
diagonal steps and the rest (sweep with its target sort, combine), with the launch gaps and the update kernels' rate.
usage: python tools/krige_variance_split.py <dir-with-*_kernel_trace.csv> N:M [chunk]"""
import csv, glob, json, sys
from collections import defaultdict

f = sorted(glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True))[-1]
n, m = (int(v) for v in sys.argv[2].split(":"))
chunk = int(sys.argv[3]) if len(sys.argv) > 3 else 8192
passes = (m + chunk - 1) // chunk
rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
comb = [i for i, r in enumerate(rows) if "krige_combine" in r["Kernel_Name"]]
assert len(comb) >= 2 * passes, "the trace must hold two calls"
last = rows[comb[-passes - 1] + 1:comb[-1] + 1]             # after the previous call's last combine, through this call's
tot, cnt = defaultdict(float), defaultdict(int)
for r in last:
    nm = r["Kernel_Name"]
    key = "fill" if "krige_cross_fill" in nm else "gemm" if "gemm_minus" in nm else "diag" if "krige_trsm128" in nm else "sweep_combine"
    tot[key] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
    cnt[key] += 1
span = (int(last[-1]["End_Timestamp"]) - int(last[0]["Start_Timestamp"])) / 1e6
gemm_flops = sum(2.0 * m * min(128, n - j) * j for j in range(0, n, 128))
print(json.dumps({"n": n, "m": m, "chunk": chunk, "span_ms": span, "kernel_ms": dict(tot), "launches": dict(cnt),
                  "gaps_ms": span - sum(tot.values()), "gemm_gflops": gemm_flops / tot["gemm"] / 1e6 if tot["gemm"] else None}))
