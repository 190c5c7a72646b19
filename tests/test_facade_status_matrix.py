"""The facade's answers that need no device, for every type x every entry: the return value and every (reason, status) call
to the GSL error handler, compared field for field with tests/golden/facade_status_parent.json.

The golden file's "recorded" block is the output of collect() below on a build of the commit before the type table
(`python tests/test_facade_status_matrix.py OUT.json` with GSL_SINTERP_LIBRARY naming that build's library).  Its
"by_hand" block holds the cells that commit could not be asked for, because it read a mesh_state as an rbf_state there or
took a wild pointer: eval_grid, get_weights and set_solver on the five mesh-state types, and gsl_sinterp_alloc with a type
that is not one of the sixteen.  Those are written from the table of what changes, not recorded.

Every entry runs on a fresh interpolant of dim 2, size 10 that was never initialised (or on none), so that no cell depends
on an earlier one and none reaches the device.  Two entries are shaped for that: `init` hands right-sized data to the
imported types (no triangulation set: refused before the device) and wrong-sized data to the others; `init_fields` and
`fit_alloc` get arrays of the wrong shape, which every type that passes its type checks refuses next."""
import ctypes as C
import json
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "facade_status_parent.json")
MESH_STATE = ("linear_mesh", "natural_mesh", "natural_simplex", "cubic_mesh", "cubic_simplex")
IMPORTED = ("linear_mesh", "natural_mesh", "cubic_mesh")
SOLVERS = (0, 1, 2, 3)
# the checkpoint ids, to write "a well-formed header of another type id"
TYPE_ID = {"gaussian": 0, "tps": 1, "linear_simplex": 2, "wendland": 3, "kriging": 4, "tps_affine": 5, "linear_mesh": 6, "matern32": 7,
           "matern52": 8, "imq": 9, "kriging_matern32": 10, "kriging_matern52": 11, "natural_mesh": 12, "natural_simplex": 13,
           "cubic_mesh": 14, "cubic_simplex": 15}
BY_HAND = ("eval_grid",) + tuple(f"set_solver_{k}" for k in SOLVERS) + ("get_weights",)


def _st(r):
    """the status of a wrapper's answer: the int itself, or the first entry of its tuple"""
    return int(r[0] if isinstance(r, tuple) else r)


def _entries(pkg, kind, tmp):
    capi, L = pkg.capi, pkg.lib()
    x = np.zeros((10, 2))
    f = np.zeros(10)
    y = np.zeros((3, 2))
    M, V = (lambda a: C.byref(capi.as_matrix(a))), (lambda a: C.byref(capi.as_vector(a)))

    def alloc(dim, size):
        p = L.gsl_sinterp_alloc(capi._ptr(pkg.Sinterp.TYPES[kind]), dim, size)
        if p:
            L.gsl_sinterp_free(p)
        return "interpolant" if p else "NULL"

    def fit_alloc(s):
        w = L.gsl_sinterp_fit_alloc(s._p, M(np.zeros((9, 2))), V(f))
        if w:
            L.gsl_sinterp_fit_free(w)
        return "workspace" if w else "NULL"

    def fwrite(s):
        return s.fwrite(os.path.join(tmp, "w.bin"))

    def fread(s, blob):
        path = os.path.join(tmp, "r.bin")
        with open(path, "wb") as fp:
            fp.write(blob)
        return s.fread(path)

    other = (TYPE_ID[kind] + 1) % 16
    header = lambda magic, tid: magic + struct.pack("<QQQdq", tid, 2, 10, 0.0, 0)
    min_size = 3 if kind in MESH_STATE + ("linear_simplex", "tps_affine") else 1
    E = {
        "alloc_dim1": None, "alloc_dim2": None, "alloc_dim3": None, "alloc_dim4": None, "alloc_size0": None, "alloc_below_min_size": None,
        "name": lambda s: s.name(),
        "min_size": lambda s: int(L.gsl_sinterp_min_size(s._p)),
        "set_neighbours_3": lambda s: s.set_neighbours(3),
        "set_neighbours_65": lambda s: s.set_neighbours(65),
        "set_nugget_0.1": lambda s: s.set_nugget(0.1),
        "set_nugget_-1": lambda s: s.set_nugget(-1.0),
        "set_variance_1": lambda s: s.set_variance(True),
        "set_loo_1": lambda s: s.set_loo(True),
        **{f"set_solver_{k}": (lambda s, k=k: s.set_solver(k)) for k in SOLVERS},
        "set_rcond_1": lambda s: s.set_rcond(True),
        "rcond": lambda s: _st(s.rcond()),
        "route": lambda s: s.route(),
        "mean": lambda s: _st(s.mean()),
        "poly": lambda s: _st(s.poly()),
        "get_weights": lambda s: _st(s.weights()),
        "n_fields": lambda s: s.n_fields(),
        "get_field_weights_0": lambda s: _st(s.field_weights(0)),
        "field_mean_0": lambda s: _st(s.field_mean(0)),
        "field_poly_0": lambda s: _st(s.field_poly(0)),
        "loo_residuals": lambda s: _st(s.loo_residuals()),
        "loo_variance": lambda s: _st(s.loo_variance()),
        "fit_alloc": fit_alloc,
        "eval_many": lambda s: _st(s.eval_many(y)),
        "eval_resident": lambda s: s.eval_resident(None, 0, 2, None, None),
        "eval_e": lambda s: _st(s.eval_e(np.zeros(2))),
        "eval_e_wrong_length": lambda s: _st(s.eval_e(np.zeros(3))),
        "eval_variance_many": lambda s: _st(s.eval_variance_many(y)),
        "eval_variance_resident_m0": lambda s: s.eval_variance_resident(None, 0, 2, None),
        "eval_variance_e": lambda s: _st(s.eval_variance_e(np.zeros(2))),
        "eval_grad_many": lambda s: _st(s.eval_grad_many(y)),
        "eval_grad_resident_m0": lambda s: s.eval_grad_resident(None, 0, 2, None, None, 2),
        "eval_grad_e": lambda s: _st(s.eval_grad_e(np.zeros(2))),
        "init_fields": lambda s: s.init_fields(x, np.zeros((9, 2))),
        "eval_fields_many": lambda s: _st(s.eval_fields_many(y)),
        "eval_fields_resident_m0": lambda s: s.eval_fields_resident(None, 0, 2, None, 1),
        "eval_fields_e": lambda s: _st(s.eval_fields_e(np.zeros(2))),
        "eval_local_many": lambda s: _st(s.eval_local_many(y)),
        "eval_grid": lambda s: _st(s.eval_grid([0.0, 0.0], [1.0, 1.0], 4, 4)),
        "set_triangulation": lambda s: s.set_triangulation(np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)),
        "set_gradients_10x2": lambda s: s.set_gradients(np.zeros((10, 2))),
        "set_gradients_10x3": lambda s: s.set_gradients(np.zeros((10, 3))),
        "set_gradient_options_1e-10_10": lambda s: s.set_gradient_options(1e-10, 10),
        "set_gradient_options_0_10": lambda s: s.set_gradient_options(0.0, 10),
        "get_gradients": lambda s: _st(s.get_gradients()),
        "init": lambda s: s.init(x, f) if kind in IMPORTED else s.init(np.zeros((9, 2)), np.zeros(9)),
        "fwrite": fwrite,
        "fread_wrong_magic": lambda s: fread(s, header(b"NOTACKPT", TYPE_ID[kind])),
        "fread_other_type_id": lambda s: fread(s, header(b"GSLSINT1", other)),
    }
    A = {"alloc_dim1": (1, 10), "alloc_dim2": (2, 10), "alloc_dim3": (3, 10), "alloc_dim4": (4, 10), "alloc_size0": (2, 0),
         "alloc_below_min_size": (2, min_size - 1)}
    for k, (dim, size) in A.items():
        E[k] = (lambda s, dim=dim, size=size: alloc(dim, size))
    return E


def collect(pkg, skip=lambda kind, entry: False):
    """{type: {entry: {"returns": value, "handler": [[reason, status], ..]}}}"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for kind in pkg.Sinterp.TYPES:
            out[kind] = {}
            for name, fn in _entries(pkg, kind, tmp).items():
                if skip(kind, name):
                    continue
                s = pkg.Sinterp(kind, 2, 10, 0)
                with pkg.capi.ErrorCalls() as calls:
                    ret = fn(s)
                out[kind][name] = {"returns": ret, "handler": [[r, st] for r, st in calls]}
                s.close()
    return out


def foreign_alloc(pkg):
    """gsl_sinterp_alloc with a well-formed gsl_sinterp_type that is not a row of the table"""
    class Type(C.Structure):
        _fields_ = [("name", C.c_char_p), ("min_size", C.c_uint)] + [(n, C.c_void_p) for n in ("alloc", "init", "eval_many", "eval_resident", "free")]
    T = Type(b"foreign", 1, None, None, None, None, None)
    with pkg.capi.ErrorCalls() as calls:
        p = pkg.lib().gsl_sinterp_alloc(C.cast(C.pointer(T), C.c_void_p), 2, 10)
    assert not p
    return {"returns": "NULL", "handler_statuses": [st for _, st in calls]}


def test_status_matrix_equals_the_parent(pkg):
    with open(GOLDEN) as fp:
        golden = json.load(fp)
    want = golden["recorded"]
    for kind, cells in golden["by_hand"]["cells"].items():
        assert not set(cells) & set(want[kind])
        want[kind].update(cells)
    got = collect(pkg)
    assert len(got) == 16 and sorted(got) == sorted(want)
    n_entries = {len(c) for c in got.values()}
    assert n_entries == {57}, n_entries                                      # sixteen types x the full entry list, no skips
    for kind in got:
        assert sorted(got[kind]) == sorted(want[kind]), kind
        for entry in got[kind]:
            assert got[kind][entry] == want[kind][entry], (kind, entry, got[kind][entry], want[kind][entry])
    assert foreign_alloc(pkg) == golden["by_hand"]["foreign_type_alloc"]


def test_c_program_walks_the_sixteen_types(pkg, tmp_path):
    libdir = os.path.dirname(pkg.library_path())
    exe = str(tmp_path / "facade_refusals")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if os.environ.get("GSL_SINTERP_ASAN") else []
    libname = os.path.basename(pkg.library_path())[3:-3]
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Werror", *san, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "facade_refusals.c"), "-o", exe,
                           "-L", libdir, "-l" + libname, "-lm", "-Wl,-rpath," + libdir])
    assert "ok" in subprocess.check_output([exe], text=True)


if __name__ == "__main__":                                                   # record the parent's cells
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    p = g.load_package()
    rec = collect(p, skip=lambda kind, entry: kind in MESH_STATE and entry in BY_HAND)
    with open(sys.argv[1], "w") as fp:
        json.dump(rec, fp, indent=1, sort_keys=True)
