"""-m gpu: the facade's host code (csrc/host/sinterp.c) where the type table, the single mesh-type path and the host
staging helper can go wrong: the grid entry on an imported triangulation, strided host batches through every one-shot
`_many` entry, and the bytes of a checkpoint of each of the sixteen types against files written before the table
(tests/golden/checkpoints_parent/, written by `python tests/test_gpu_facade.py DIR` on that build)."""
import os
import sys

import numpy as np
import pytest

from gpu_util import bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKPOINTS = os.path.join(ROOT, "tests", "golden", "checkpoints_parent")
SENTINEL = -12345.0


# ---------------------------------------------------------------- 1. grid on a linear mesh
def grid_nodes(lo, hi, n0, n1):
    xs, ys = (hi[0] - lo[0]) / n0, (hi[1] - lo[1]) / n1
    return np.array([[lo[0] + xs * i, lo[1] + ys * j] for i in range(n0) for j in range(n1)])


def test_grid_on_a_linear_mesh(pkg, tmp_path):
    from scipy.spatial import Delaunay
    rng = np.random.default_rng(5)
    x = rng.random((50, 2))
    f = np.sin(3.0 * x[:, 0]) + x[:, 1] ** 2
    d = Delaunay(x)
    s = pkg.Sinterp("linear_mesh", 2, 50, 0)
    with pkg.capi.ErrorCalls() as calls:
        assert s.eval_grid([0.0, 0.0], [1.0, 1.0], 4, 4)[0] == pkg.capi.GSL_EINVAL
    assert calls == [("gsl_sinterp_eval_grid: interpolant not initialised", pkg.capi.GSL_EINVAL)]
    assert s.set_triangulation(d.simplices.astype(np.int32), d.neighbors.astype(np.int32)) == 0 and s.init(x, f) == 0
    # strictly inside the hull: the box around the centroid that the hull's inscribed circle contains
    c = x.mean(axis=0)
    cross = lambda u, v: u[0] * v[1] - u[1] * v[0]
    r = min(abs(cross(x[b] - x[a], c - x[a])) / np.linalg.norm(x[b] - x[a]) for a, b in d.convex_hull)
    lo, hi = c - 0.5 * r, c + 0.5 * r
    st, grid = s.eval_grid(lo, hi, 8, 8)
    st2, direct, tri = s.eval_many(grid_nodes(lo, hi, 8, 8), want_leaf=True)
    assert st == 0 and st2 == 0 and (tri >= 0).all()
    assert np.array_equal(bits(grid.reshape(-1)), bits(direct))
    # past the hull: EDOM, NaN exactly where eval_many finds no triangle
    lo2, hi2 = x.min(axis=0) - 0.25, x.max(axis=0) + 0.25
    with pkg.capi.ErrorCalls() as calls:
        st, wide = s.eval_grid(lo2, hi2, 8, 8)
    assert st == pkg.capi.GSL_EDOM and calls == [("gsl_sinterp_eval_grid: grid node(s) outside the triangulation", pkg.capi.GSL_EDOM)]
    with pkg.capi.ErrorCalls():
        st2, direct2, tri2 = s.eval_many(grid_nodes(lo2, hi2, 8, 8), want_leaf=True)
    assert st2 == pkg.capi.GSL_EDOM and (tri2 < 0).any() and (tri2 >= 0).any()
    assert np.array_equal(np.isnan(wide.reshape(-1)), tri2 == -1)
    assert np.array_equal(bits(wide.reshape(-1))[tri2 >= 0], bits(direct2)[tri2 >= 0])
    # a checkpoint round trip keeps the grid's bits
    path = tmp_path / "mesh.bin"
    assert s.fwrite(path) == 0
    r2 = pkg.Sinterp("linear_mesh", 2, 50, 0)
    assert r2.fread(path) == 0
    st, again = r2.eval_grid(lo, hi, 8, 8)
    assert st == 0 and np.array_equal(bits(again), bits(grid))


# ---------------------------------------------------------------- 2. strided host batches
N, M = 40, 7


def strided(a, width=5):
    """the rows of `a` as the first columns of a wider array full of SENTINEL; (view, holder)"""
    w = np.full((a.shape[0], width), SENTINEL)
    w[:, :a.shape[1]] = a
    return w[:, :a.shape[1]], w


def every_second(m):
    h = np.full(2 * m, SENTINEL)
    return h[::2], h


def untouched(holder, view_cols=None):
    """every SENTINEL outside the view is still there"""
    if holder.ndim == 1:
        return bool((holder[1::2] == SENTINEL).all())
    return bool((holder[:, view_cols:] == SENTINEL).all())


def _data(dim, seed=3):
    rng = np.random.default_rng(seed)
    x = rng.random((N, dim))
    f = np.cos(2.0 * x[:, 0]) + x[:, -1]
    y = 0.1 + 0.8 * rng.random((M, dim))
    return x, f, y


def test_strided_variance_batch(pkg):
    x, f, y = _data(2)
    s = pkg.Sinterp("kriging", 2, N, 0)
    assert s.set_variance(True) == 0 and s.init(x, f) == 0
    st, want = s.eval_variance_many(y)
    yv, yh = strided(y)
    ov, oh = every_second(M)
    st2, got = s.eval_variance_many(yv, out=ov)
    assert st == 0 and st2 == 0 and np.array_equal(bits(got), bits(want)) and untouched(oh) and untouched(yh, 2)
    with pkg.capi.ErrorCalls() as calls:
        assert s.eval_variance_many(np.zeros((0, 2)))[0] == 0
    assert calls == []


@pytest.mark.parametrize("dim", [2, 3])
def test_strided_gradient_batch(pkg, dim):
    x, f, y = _data(dim)
    s = pkg.Sinterp("gaussian", dim, N, 0)
    assert s.init(x, f) == 0
    st, sv, g = s.eval_grad_many(y)
    assert st == 0
    yv, yh = strided(y)
    for want_value in (True, False):
        ov, oh = every_second(M)
        gv, gh = strided(np.full((M, dim), SENTINEL))
        st2, s2, g2 = s.eval_grad_many(yv, want_value=want_value, out=(ov if want_value else None, gv))
        assert st2 == 0 and np.array_equal(bits(g2), bits(g)) and untouched(gh, dim) and untouched(yh, dim)
        if want_value:
            assert np.array_equal(bits(s2), bits(sv)) and untouched(oh)
        else:
            assert s2 is None
            stc, _, gc = s.eval_grad_many(y, want_value=False)
            assert stc == 0 and np.array_equal(bits(gc), bits(g))
    with pkg.capi.ErrorCalls() as calls:
        assert s.eval_grad_many(np.zeros((0, dim)))[0] == 0
        assert s.eval_grad_many(np.zeros((0, dim)), want_value=False)[0] == 0
    assert calls == []


def test_strided_fields_batch(pkg):
    x, f, y = _data(2)
    F = np.ascontiguousarray(np.stack([f, f ** 2, np.sin(f)], axis=1))
    s = pkg.Sinterp("gaussian", 2, N, 0)
    assert s.init_fields(x, F) == 0 and s.n_fields() == 3
    st, want = s.eval_fields_many(y)
    yv, yh = strided(y)
    Sv, Sh = strided(np.full((M, 3), SENTINEL))
    st2, got = s.eval_fields_many(yv, out=Sv)
    assert st == 0 and st2 == 0 and np.array_equal(bits(got), bits(want)) and untouched(Sh, 3) and untouched(yh, 2)
    with pkg.capi.ErrorCalls() as calls:
        assert s.eval_fields_many(np.zeros((0, 2)))[0] == 0
    assert calls == []


def test_strided_local_batch(pkg):
    import ctypes as C
    capi, L = pkg.capi, pkg.lib()
    x, f, y = _data(2)
    s = pkg.Sinterp("kriging", 2, N, 0)
    assert s.set_neighbours(4) == 0 and s.init(x, f) == 0
    st, sv, var, idx = s.eval_local_many(y)
    assert st == 0 and idx.shape == (M, 4) and (idx >= 0).all()
    yv, yh = strided(y)
    (o1, h1), (o2, h2) = every_second(M), every_second(M)
    i2 = np.full((M, 4), -7, dtype=np.int32)
    st2 = L.gsl_sinterp_eval_local_many(s._p, C.byref(capi.as_matrix(yv)), C.byref(capi.as_vector(o1)), C.byref(capi.as_vector(o2)),
                                        i2.ctypes.data_as(C.POINTER(C.c_int)))
    assert st2 == 0 and np.array_equal(bits(o1), bits(sv)) and np.array_equal(bits(o2), bits(var)) and np.array_equal(i2, idx)
    assert untouched(h1) and untouched(h2) and untouched(yh, 2)
    # one output at a time: the others are neither allocated nor touched
    o3, h3 = every_second(M)
    assert L.gsl_sinterp_eval_local_many(s._p, C.byref(capi.as_matrix(yv)), None, C.byref(capi.as_vector(o3)), None) == 0
    assert np.array_equal(bits(o3), bits(var)) and untouched(h3)
    with capi.ErrorCalls() as calls:
        assert s.eval_local_many(np.zeros((0, 2)))[0] == 0
    assert calls == []


def test_strided_cubic_gradient_batch(pkg):
    from scipy.spatial import Delaunay
    x, f, y = _data(2)
    d = Delaunay(x)
    s = pkg.Sinterp("cubic_mesh", 2, N, 0)
    assert s.set_triangulation(d.simplices.astype(np.int32), d.neighbors.astype(np.int32)) == 0 and s.init(x, f) == 0
    y = x.mean(axis=0) + 0.2 * (y - 0.5)                              # well inside the hull
    st, sv, g = s.eval_grad_many(y)
    assert st == 0 and np.isfinite(g).all()
    yv, yh = strided(y)
    ov, oh = every_second(M)
    gv, gh = strided(np.full((M, 2), SENTINEL))
    st2, s2, g2 = s.eval_grad_many(yv, out=(ov, gv))
    assert st2 == 0 and np.array_equal(bits(s2), bits(sv)) and np.array_equal(bits(g2), bits(g))
    assert untouched(oh) and untouched(gh, 2) and untouched(yh, 2)
    st3, _, g3 = s.eval_grad_many(yv, want_value=False, out=(None, gv))
    assert st3 == 0 and np.array_equal(bits(g3), bits(g)) and untouched(gh, 2)
    # a target outside the triangulation: everything is stored (NaN there), then GSL_EDOM is reported once
    yo = y.copy(); yo[2] = [9.0, 9.0]
    with pkg.capi.ErrorCalls() as calls:
        st4, s4, g4 = s.eval_grad_many(yo)
    assert st4 == pkg.capi.GSL_EDOM and [c[1] for c in calls] == [pkg.capi.GSL_EDOM]
    assert np.isnan(s4[2]) and np.array_equal(bits(np.delete(s4, 2)), bits(np.delete(sv, 2)))
    with pkg.capi.ErrorCalls() as calls:
        assert s.eval_grad_many(np.zeros((0, 2)))[0] == 0
    assert calls == []


# ---------------------------------------------------------------- 3. checkpoint bytes
KINDS = ("gaussian", "tps", "linear_simplex", "wendland", "kriging", "tps_affine", "linear_mesh", "matern32", "matern52", "imq",
         "kriging_matern32", "kriging_matern52", "natural_mesh", "natural_simplex", "cubic_mesh", "cubic_simplex")   # index = type id
HOST_PAYLOAD = (2, 6, 12, 13, 14, 15)                                 # tree / mesh / response / gradients: all made on the host
RBF_PREFIX = 8 + 3 * 8 + 8 + 8 + 8 * 2 * 8                            # magic, head, eps, flags word, the 8 x 2 centres
# two rows of four points, the upper shifted by half a cell: six triangles, strictly Delaunay, a convex parallelogram
LATTICE = np.array([[0.0, 0.0], [1.0, 0.0], [2.0, 0.0], [3.0, 0.0], [0.5, 0.75], [1.5, 0.75], [2.5, 0.75], [3.5, 0.75]])
LATTICE_TRI = np.array([[0, 1, 4], [1, 5, 4], [1, 2, 5], [2, 6, 5], [2, 3, 6], [3, 7, 6]], dtype=np.int32)


def checkpoint_model(pkg, kind):
    """(interpolant, x, f): N = 8, dim 2, seed 2024; the imported types on the lattice, the others on random sites"""
    rng = np.random.default_rng(2024)
    x = rng.random((8, 2))
    grad = rng.random((8, 2))
    s = pkg.Sinterp(kind, 2, 8, 0)
    if kind.endswith("_mesh"):
        x = LATTICE.copy()
        assert s.set_triangulation(LATTICE_TRI) == 0
    if kind.endswith("_simplex"):
        assert s.set_tree_options(0, pkg.capi.Rng(0)) == 0
    if kind.startswith("cubic"):
        assert s.set_gradients(grad) == 0                            # supplied: nothing is estimated
    f = 1.0 + x[:, 0] - 0.5 * x[:, 1] ** 2
    assert s.init(x, f) == 0, kind
    return s, x, f


@pytest.mark.parametrize("tid", range(16))
def test_checkpoint_bytes_equal_the_parent(pkg, tmp_path, tid):
    kind = KINDS[tid]
    golden = os.path.join(CHECKPOINTS, f"{tid:02d}_{kind}.bin")
    want = open(golden, "rb").read()
    assert len(want) < 2048
    s, x, f = checkpoint_model(pkg, kind)
    path = tmp_path / "new.bin"
    assert s.fwrite(path) == 0
    got = path.read_bytes()
    assert len(got) == len(want)
    if tid in HOST_PAYLOAD:
        assert got == want
    else:
        assert got[:RBF_PREFIX] == want[:RBF_PREFIX]                  # weight bits are not pinned across builds
    r = pkg.Sinterp(kind, 2, 8, 0)
    assert r.fread(golden) == 0
    st, v, _ = r.eval_many(np.ascontiguousarray(x))
    # At the data sites.  Linear / natural / cubic: a vertex has barycentric coordinates (1, 0, 0) up to rounding in the
    # (for the tree: standardised) coordinates, a few hundred ulp at worst, so the value is f_i to well under 1e-12 |f|
    # (measured: 4.4e-13 for linear_simplex, <= 2.3e-16 for the others).  RBF and kriging (nugget 0) interpolate: the residual of the
    # solve is cond(A) eps, and for 8 sites at these widths cond(A) < 1e5: 1e-9 leaves two digits.
    tol = 1e-12 if tid in HOST_PAYLOAD else 1e-9
    print(f"{kind}: max |s(x_i) - f_i| = {np.abs(v - f).max():.3e}")
    assert st == 0 and np.abs(v - f).max() <= tol * np.abs(f).max()


if __name__ == "__main__":                                            # write the sixteen files with the loaded build
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    p = g.load_package()
    os.makedirs(sys.argv[1], exist_ok=True)
    for tid, kind in enumerate(KINDS):
        s, _, _ = checkpoint_model(p, kind)
        assert s.fwrite(os.path.join(sys.argv[1], f"{tid:02d}_{kind}.bin")) == 0
        print(kind, os.path.getsize(os.path.join(sys.argv[1], f"{tid:02d}_{kind}.bin")))
