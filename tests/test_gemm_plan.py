"""The dispatch rule of the trailing update (csrc/hip/gemm_plan.h) against the decisions sinterp_gemm_minus made before
the rule was moved out of it (tests/golden/gemm_plan_parent.json), field for field, and the invariants the stream-K kernel
relies on.  No GPU: the rule is host integer arithmetic, tests/c/gemm_plan_dump.cpp prints its plans."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SK_PRI_SLOTS = 32
FAMILIES = {"smallk32", "smallk64", "sk_nt", "dma256", "dma128", "sk_kn256", "sk_kn128", "plain"}
SWITCHES = ["no_dma", "no_w8", "rule_r4", "no_t64", "no_group", "no_pipe", "no_hybrid", "no_kn", "rider_slices", "cfg_override", "cfg_whole"]
DEFAULTS = {s: 0 for s in SWITCHES}
DEFAULTS["cfg_override"] = -1


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "gemm_plan_parent.json")) as f:
        doc = json.load(f)
    assert doc["in_columns"][9:] == SWITCHES
    return doc


@pytest.fixture(scope="module")
def plans(golden, tmp_path_factory):
    """the plans of the header for the golden inputs, as [family, int, ...] rows in golden order"""
    exe = str(tmp_path_factory.mktemp("gemm_plan") / "gemm_plan_dump")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if os.environ.get("GSL_SINTERP_ASAN") else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", *san,
                           "-I", os.path.join(ROOT, "gsl-scattered-interpolation_amd", "csrc", "hip"),
                           os.path.join(ROOT, "tests", "c", "gemm_plan_dump.cpp"), "-o", exe])
    text = "".join(" ".join(str(v) for v in r["in"]) + "\n" for r in golden["records"])
    out = subprocess.run([exe], input=text, stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
    assert len(out) == len(golden["records"])
    return [[f[0]] + [int(v) for v in f[1:]] for f in (line.split() for line in out)]


def test_plans_equal_the_parent_commit(golden, plans):
    cols = golden["plan_columns"]
    for rec, got in zip(golden["records"], plans):
        want = rec["plan"]
        assert len(got) == len(want) == len(cols)
        diff = {c: (w, g) for c, w, g in zip(cols, want, got) if w != g}
        assert not diff, (rec["tag"], dict(zip(golden["in_columns"], rec["in"])), diff)


def test_golden_covers_every_family_and_cu_count(golden):
    recs = golden["records"]
    assert {r["plan"][0] for r in recs} == FAMILIES
    cus = golden["in_columns"].index("cus")
    assert {256, 8, 1, 0} <= {r["in"][cus] for r in recs}
    for n in (256, 384, 1024, 1152, 4096, 8192, 16384, 1000):
        assert {256, 8, 1} <= {r["in"][cus] for r in recs if r["tag"] == f"chol N={n}"}


def test_every_switch_changes_a_plan(golden, plans):
    """a switch that the rule silently ignores fails here: for each one there is a pair of records that differ in that
    switch alone (every other switch at its default; cfg_whole: under the same cfg_override) and whose plans differ"""
    icol = golden["in_columns"]
    by_in = {tuple(r["in"]): p for r, p in zip(golden["records"], plans)}
    for sw in SWITCHES:
        at = icol.index(sw)
        others = [icol.index(s) for s in SWITCHES if s != sw and not (sw == "cfg_whole" and s == "cfg_override")]
        changed = 0
        for key, plan in by_in.items():
            if key[at] == DEFAULTS[sw] or any(key[i] != DEFAULTS[icol[i]] for i in others):
                continue
            off = list(key)
            off[at] = DEFAULTS[sw]
            base = by_in.get(tuple(off))
            changed += base is not None and base != plan
        assert changed, sw


def _tiles(rec_in, p):
    """tiles of the plan's configuration, counted the way decode_tile (gemm.hip) enumerates them"""
    lower = rec_in["lower_only"]
    tm, tn = p["tiles_m"], p["tiles_n"]
    if not lower:
        return tm * tn
    if p["family"] == "sk_nt" and p["cfg"] == 0:          # 256x128: two column tiles per tile row on the diagonal
        fr = tn // 2
        return fr * (fr + 1) + (tm - fr) * tn
    return tn * (tn + 1) // 2 + (tm - tn) * tn


def test_stream_k_invariants(golden, plans):
    seen_pri = seen_dp = 0
    for rec, row in zip(golden["records"], plans):
        p = dict(zip(golden["plan_columns"], row))
        i = dict(zip(golden["in_columns"], rec["in"]))
        if i["cus"] == 1:
            assert not p["ride"], i                          # no CU can be left to a rider
        if p["ride"]:
            assert p["family"] == "sk_nt" and i["rider_offered"] and i["c_aligned"] and i["lower_only"]
            assert p["grid"] == p["G"] + 1 and p["need"] == (3 if p["cfg"] == 6 else 1)
        if not p["family"].startswith("sk_"):
            continue
        tiles = _tiles(i, p)
        assert 1 <= p["G"] <= i["cus"] - (1 if p["ride"] else 0), (i, p)
        assert p["dp_rounds"] * p["G"] <= tiles, (i, p)
        if not p["whole"] and p["pri_tiles"] == 0:
            assert p["total"] == p["G"] * p["base"] + p["rem"], (i, p)
            assert p["total"] == (tiles - p["dp_rounds"] * p["G"]) * p["steps"], (i, p)
        seen_dp += p["dp_rounds"] > 0
        if p["pri_tiles"] > 0:
            seen_pri += 1
            assert p["ride"] and p["pri_tiles"] == p["need"]
            assert p["dp_rounds"] == 0
            assert p["pri_sl"] * p["pri_nsl"] == p["steps"]
            assert p["pri_tiles"] * p["pri_nsl"] <= min(p["G"], SK_PRI_SLOTS)
            assert p["base"] == (p["total"] + p["pri_tiles"] * p["steps"]) // p["G"]     # base counts the slices too
            assert 2 * p["pri_sl"] <= p["base"]
            assert p["pri_tiles"] < tiles
            assert p["pri_base"] == i["cus"]
    assert seen_pri and seen_dp
