"""Natural-neighbour (Sibson) interpolation, CPU part: simplex_mesh_delaunay_metric (which metric makes an imported mesh
Delaunay), the facade's allocation rules and the status answers that need no device.  The reference lists "Voronoi"
interpolation as future work only: PARITY UNPINNED.  scipy.spatial.Delaunay is the QHull import.
-m gpu part: tests/test_gpu_natural.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def qhull(points):
    from scipy.spatial import Delaunay
    d = Delaunay(points)
    return np.ascontiguousarray(d.simplices, dtype=np.int32), np.ascontiguousarray(d.neighbors, dtype=np.int32)


def flip_one_interior_edge(x, tri, nbr):
    """the triangle array with the shared edge of one strictly convex pair of triangles exchanged for the other diagonal"""
    def cross(a, b, c):
        return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
    for t in range(len(tri)):
        for k in range(3):
            u = nbr[t, k]
            if u < 0:
                continue
            a, b, c = tri[t, k], tri[t, (k + 1) % 3], tri[t, (k + 2) % 3]      # the edge b-c is shared; a is opposite
            d = [v for v in tri[u] if v != b and v != c][0]
            # strictly convex quadrilateral a, b, d, c, and clearly so: the new diagonal a-d separates b from c
            s1, s2 = cross(x[a], x[d], x[b]), cross(x[a], x[d], x[c])
            area = abs(cross(x[a], x[b], x[c])) + abs(cross(x[d], x[b], x[c]))
            if s1 * s2 < 0 and min(abs(s1), abs(s2)) > 0.2 * area:
                out = tri.copy()
                out[t] = [a, b, d]
                out[u] = [a, d, c]
                return out
    raise AssertionError("no flippable edge")


def test_delaunay_metric(pkg):
    rng = np.random.default_rng(0)
    x = rng.random((200, 2))
    tri, nbr = qhull(x)
    assert pkg.SimplexMesh.from_arrays(x, tri, nbr).delaunay_metric() == 1
    assert pkg.SimplexMesh.from_arrays(x, tri).delaunay_metric() == 1                       # derived links
    wide = x * [1000.0, 1.0]
    wt, wn = qhull(wide)
    assert pkg.SimplexMesh.from_arrays(wide, wt, wn).delaunay_metric() == 1                  # triangulated as given
    # triangulated in the standardised coordinates (centre of the bounding box, 1 / extent), imported with the raw points
    lo, hi = wide.min(axis=0), wide.max(axis=0)
    st, sn = qhull((wide - (lo + hi) / 2.0) / (hi - lo))
    assert pkg.SimplexMesh.from_arrays(wide, st, sn).delaunay_metric() == 2
    flipped = flip_one_interior_edge(x, tri, nbr)
    m = pkg.SimplexMesh.from_arrays(x, flipped)
    assert m.n_triangles == len(tri) and m.convex()
    assert m.delaunay_metric() == 0
    x3 = rng.random((40, 3))
    from scipy.spatial import Delaunay
    assert pkg.SimplexMesh.from_arrays(x3, Delaunay(x3).simplices.astype(np.int32)).delaunay_metric() == 0
    # everything cocircular / flat triangles skipped: a lattice passes
    g = np.stack(np.meshgrid(np.arange(7.0), np.arange(7.0), indexing="ij"), axis=-1).reshape(-1, 2)
    gt, gn = qhull(g)
    assert pkg.SimplexMesh.from_arrays(g, gt, gn).delaunay_metric() == 1


def test_a_tree_export_is_delaunay_in_the_standardised_metric(pkg, orc):
    x = orc.synth_centres(300, 2) * [50.0, 0.2] + [3.0, -1.0]
    t = pkg.SimplexTree(2, 300)
    assert t.init(x, flags=0, rng=pkg.capi.Rng(0)) == 0
    assert pkg.SimplexMesh.from_tree(t).delaunay_metric() == 2


def test_facade_allocation_and_statuses_without_a_device(pkg):
    capi = pkg.capi
    for kind in ("natural_mesh", "natural_simplex"):
        with capi.ErrorCalls() as calls:
            with pytest.raises(capi.GslError):
                pkg.Sinterp(kind, 3, 10, 0)
        assert [s for _, s in calls] == [capi.GSL_EUNIMPL]
        s = pkg.Sinterp(kind, 2, 10, 0)
        assert s.name() == {"natural_mesh": "natural-neighbour-imported-triangulation", "natural_simplex": "natural-neighbour-simplex"}[kind]
        with capi.ErrorCalls() as calls:
            assert s.set_neighbours(3) == capi.GSL_EUNSUP
            assert pkg.lib().gsl_sinterp_eval_grad_resident(s._p, None, 0, 2, None, None, 2) == capi.GSL_EUNSUP
            assert pkg.lib().gsl_sinterp_eval_variance_resident(s._p, None, 0, 2, None) == capi.GSL_EUNSUP
        assert [st for _, st in calls] == [capi.GSL_EUNSUP] * 3
    x = np.array([[0.0, 0.0], [2.0, -1.5], [3.0, 0.0], [2.0, 1.5]])
    f = np.zeros(4)
    s = pkg.Sinterp("natural_mesh", 2, 4, 0)
    assert s.init(x, f) == capi.GSL_EINVAL                                                   # no triangulation set
    assert s.set_triangulation(np.array([[0, 1, 3], [1, 2, 3]], dtype=np.int32)) == 0
    assert s.init(x, f) == capi.GSL_EINVAL                                                   # the wrong diagonal: not Delaunay
    assert pkg.Sinterp("natural_simplex", 2, 4, 0).set_triangulation(np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)) == capi.GSL_EINVAL
    # device entries: a NULL mirror / context is GSL_EFAULT before anything else
    L = pkg.lib()
    v = np.zeros(4)
    assert L.simplex_mesh_device_eval_natural_many(None, C.byref(capi.as_matrix(x)), C.byref(capi.as_vector(v)), None) == capi.GSL_EFAULT
    assert L.simplex_mesh_device_eval_natural_resident(None, None, 0, 2, None, None) == capi.GSL_EFAULT
    assert L.gsl_sinterp_hip_mesh_natural_pack(None, 2, None, None, 4, None, None, None) == capi.GSL_EFAULT
    assert L.gsl_sinterp_hip_mesh_natural_eval(None, 2, None, None, None, None, None, 0, 2, 0, None, None) == capi.GSL_EFAULT


def test_c_program_references_the_natural_prototypes(pkg, tmp_path):
    libdir = os.path.dirname(pkg.library_path())
    exe = str(tmp_path / "natural_prototypes")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if os.environ.get("GSL_SINTERP_ASAN") else []
    libname = os.path.basename(pkg.library_path())[3:-3]
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Werror", *san, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "natural_prototypes.c"), "-o", exe,
                           "-L", libdir, "-l" + libname, "-lm", "-Wl,-rpath," + libdir])
    assert "ok" in subprocess.check_output([exe], text=True)
