"""Developer tool: are the kernels of two builds of one .hip file the same code?  Takes two device assembly listings
(hipcc <the Makefile's HIPFLAGS> --cuda-device-only -S file.hip -o file.s) and compares, kernel by kernel,
  * the instruction count and the opcode histogram (first token of every instruction line), and
  * the resources the kernel descriptor declares (VGPRs, SGPRs, LDS bytes, scratch bytes).
Operands, label numbers and instruction order are not compared: two listings that pass hold the same instructions per kernel,
possibly scheduled or register-allocated differently.  Prints the kernels that differ (with the differing opcodes) and one
summary line; exit status 1 when anything differs.
usage: python tools/asm_kernel_diff.py before.s after.s"""
import collections
import re
import sys

RESOURCES = (".amdhsa_next_free_vgpr", ".amdhsa_next_free_sgpr", ".amdhsa_group_segment_fixed_size",
             ".amdhsa_private_segment_fixed_size")


def kernels(path):
    """{kernel symbol: (opcode histogram, {resource: value})}"""
    lines = open(path).read().split("\n")
    res = {}
    name = None
    for ln in lines:
        tok = ln.split()
        if len(tok) == 2 and tok[0] == ".amdhsa_kernel":
            name = tok[1]
            res[name] = {}
        elif tok and tok[0] == ".end_amdhsa_kernel":
            name = None
        elif name and len(tok) >= 2 and tok[0] in RESOURCES:
            res[name][tok[0]] = tok[1]
    hist = {}
    name = None
    for ln in lines:
        code = ln.split(";")[0].rstrip()
        if not code:
            continue
        if not code[0].isspace():                                    # a label
            label = code.rstrip(":")
            if label in res:
                name = label
                hist[name] = collections.Counter()
            elif re.match(r"\.Lfunc_end\d+$", label):
                name = None
            continue
        op = code.split()[0]
        if name and not op.startswith("."):                          # directives are not instructions
            hist[name][op] += 1
    return {k: (hist.get(k, collections.Counter()), res[k]) for k in res}


def main(before, after):
    a, b = kernels(before), kernels(after)
    differing = 0
    for k in sorted(set(a) ^ set(b)):
        differing += 1
        print(f"only in {before if k in a else after}: {k}")
    for k in sorted(set(a) & set(b)):
        (ha, ra), (hb, rb) = a[k], b[k]
        if ha == hb and ra == rb:
            continue
        differing += 1
        print(f"differs: {k}")
        print(f"  instructions {sum(ha.values())} -> {sum(hb.values())}")
        for op in sorted(set(ha) | set(hb)):
            if ha[op] != hb[op]:
                print(f"  {op}: {ha[op]} -> {hb[op]}")
        for r in RESOURCES:
            if ra.get(r) != rb.get(r):
                print(f"  {r}: {ra.get(r)} -> {rb.get(r)}")
    common = len(set(a) & set(b))
    print(f"{len(a)} kernels before, {len(b)} after, {common} in both: {differing} differ in instruction count, opcode histogram or "
          f"resources (instructions in all: {sum(sum(h.values()) for h, _ in a.values())} -> "
          f"{sum(sum(h.values()) for h, _ in b.values())})")
    return 1 if differing else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
