"""Clough-Tocher C1 cubic interpolation, CPU part: simplex_mesh_vertex_adjacency (the rows of the gradient system), the
facade's allocation rules and the status answers that need no device.  The reference has no cubic mesh method: PARITY
UNPINNED.  scipy.spatial.Delaunay is the QHull import and the oracle of the adjacency.
-m gpu part: tests/test_gpu_cubic.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_vertex_adjacency_matches_qhull(pkg):
    from scipy.spatial import Delaunay
    x = np.random.default_rng(0).random((60, 2))
    d = Delaunay(x)
    mesh = pkg.SimplexMesh.from_arrays(x, np.ascontiguousarray(d.simplices, dtype=np.int32), np.ascontiguousarray(d.neighbors, dtype=np.int32))
    off, adj = mesh.vertex_adjacency()
    indptr, indices = d.vertex_neighbor_vertices
    assert off[0] == 0 and off[-1] == len(adj) == len(indices)
    for i in range(60):
        row = adj[off[i]:off[i + 1]]
        assert list(row) == sorted(set(row.tolist()))                       # ascending, every edge once
        assert set(row.tolist()) == set(indices[indptr[i]:indptr[i + 1]].tolist())
    # every undirected edge once per endpoint
    pairs = {(i, int(j)) for i in range(60) for j in adj[off[i]:off[i + 1]]}
    assert all((j, i) in pairs for i, j in pairs) and len(pairs) == len(adj)
    # derived links give the same rows; a 3-D mesh has none
    off2, adj2 = pkg.SimplexMesh.from_arrays(x, np.ascontiguousarray(d.simplices, dtype=np.int32)).vertex_adjacency()
    assert np.array_equal(off, off2) and np.array_equal(adj, adj2)
    x3 = np.random.default_rng(1).random((30, 3))
    m3 = pkg.SimplexMesh.from_arrays(x3, Delaunay(x3).simplices.astype(np.int32))
    with pkg.capi.ErrorCalls() as calls:
        with pytest.raises(pkg.capi.GslError):
            m3.vertex_adjacency()
    assert [s for _, s in calls] == [pkg.capi.GSL_EUNSUP]


def test_facade_allocation_and_statuses_without_a_device(pkg):
    capi = pkg.capi
    L = pkg.lib()
    x = np.array([[0.0, 0.0], [2.0, -1.5], [3.0, 0.0], [2.0, 1.5]])
    f = np.zeros(4)
    names = {"cubic_mesh": "clough-tocher-imported-triangulation", "cubic_simplex": "clough-tocher-simplex"}
    for kind in ("cubic_mesh", "cubic_simplex"):
        with capi.ErrorCalls() as calls:
            with pytest.raises(capi.GslError):
                pkg.Sinterp(kind, 3, 10, 0)
        assert [s for _, s in calls] == [capi.GSL_EUNIMPL]
        s = pkg.Sinterp(kind, 2, 4, 0)
        assert s.name() == names[kind]
        # fields, variance, leave-one-out, fit and set_neighbours: not for these types
        with capi.ErrorCalls() as calls:
            assert s.set_neighbours(3) == capi.GSL_EUNSUP
            assert L.gsl_sinterp_eval_variance_resident(s._p, None, 0, 2, None) == capi.GSL_EUNSUP
            assert s.init_fields(x, np.zeros((4, 2))) == capi.GSL_EUNSUP
            assert s.loo_variance()[0] == capi.GSL_EUNSUP
            assert s.loo_residuals()[0] == capi.GSL_EUNSUP
            assert not L.gsl_sinterp_fit_alloc(s._p, C.byref(capi.as_matrix(x)), C.byref(capi.as_vector(f)))
        assert [st for _, st in calls] == [capi.GSL_EUNSUP] * 6
        # gradients are supported: an interpolant that is not initialised says so
        with capi.ErrorCalls() as calls:
            assert L.gsl_sinterp_eval_grad_resident(s._p, None, 0, 2, None, None, 2) == capi.GSL_EINVAL
            assert s.eval_grad_many(x)[0] == capi.GSL_EINVAL
            assert s.get_gradients()[0] == capi.GSL_EINVAL
            # set_gradients: size x 2 only
            assert s.set_gradients(np.zeros((4, 3))) == capi.GSL_EBADLEN
            assert s.set_gradients(np.zeros((5, 2))) == capi.GSL_EBADLEN
            assert s.set_gradient_options(0.0, 10) == capi.GSL_EINVAL and s.set_gradient_options(1e-10, 0) == capi.GSL_EINVAL
        assert s.set_gradients(np.zeros((4, 2))) == 0 and s.set_gradients(None) == 0
        assert s.set_gradient_options(1e-10, 10) == 0
    s = pkg.Sinterp("cubic_mesh", 2, 4, 0)
    with capi.ErrorCalls():
        assert s.init(x, f) == capi.GSL_EINVAL                                               # no triangulation set
        assert pkg.Sinterp("cubic_simplex", 2, 4, 0).set_triangulation(np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)) == capi.GSL_EINVAL
        # the other types have no gradients to set
        lin = pkg.Sinterp("linear_mesh", 2, 4, 0)
        assert lin.set_gradients(np.zeros((4, 2))) == capi.GSL_EINVAL and lin.set_gradient_options(1e-10, 10) == capi.GSL_EINVAL
        assert lin.get_gradients()[0] == capi.GSL_EINVAL
    # the wrong diagonal of the kite is no obstacle for this method: accepted
    assert s.set_triangulation(np.array([[0, 1, 3], [1, 2, 3]], dtype=np.int32)) == 0


def test_null_interpolant_mirror_or_context_is_efault(pkg):
    capi = pkg.capi
    L = pkg.lib()
    x = np.zeros((4, 2))
    v = np.zeros(4)
    M, V = C.byref(capi.as_matrix(x)), C.byref(capi.as_vector(v))
    with capi.ErrorCalls():
        assert L.gsl_sinterp_set_gradients(None, M) == capi.GSL_EFAULT
        assert L.gsl_sinterp_set_gradient_options(None, 1e-10, 10) == capi.GSL_EFAULT
        assert L.gsl_sinterp_get_gradients(None, M, None, None) == capi.GSL_EFAULT
        assert L.simplex_mesh_device_bind_gradients(None, M) == capi.GSL_EFAULT
        assert L.simplex_mesh_device_set_gradient_options(None, 1e-10, 10) == capi.GSL_EFAULT
        assert L.simplex_mesh_device_gradients(None, M, None, None) == capi.GSL_EFAULT
        assert L.simplex_mesh_device_eval_cubic_many(None, M, V, None, None) == capi.GSL_EFAULT
        assert L.simplex_mesh_device_eval_cubic_resident(None, None, 0, 2, None, None, 2, None) == capi.GSL_EFAULT
        assert L.simplex_mesh_vertex_adjacency(None, None, None, 0, None) == capi.GSL_EFAULT
    assert L.gsl_sinterp_hip_mesh_cubic_gradients(None, 4, None, None, 0, None, None, 1e-12, 10, None, None, None) == capi.GSL_EFAULT
    assert L.gsl_sinterp_hip_mesh_cubic_pack(None, 2, None, None, 4, None, None, None, None) == capi.GSL_EFAULT
    assert L.gsl_sinterp_hip_mesh_cubic_eval(None, 2, None, None, None, None, 0, 2, None, None, 2) == capi.GSL_EFAULT


def test_existing_types_still_refuse_gradients(pkg):
    capi = pkg.capi
    for kind in ("linear_mesh", "natural_mesh", "natural_simplex", "linear_simplex"):
        s = pkg.Sinterp(kind, 2, 10, 0)
        with capi.ErrorCalls():
            assert pkg.lib().gsl_sinterp_eval_grad_resident(s._p, None, 0, 2, None, None, 2) == capi.GSL_EUNSUP


def test_c_program_references_the_cubic_prototypes(pkg, tmp_path):
    libdir = os.path.dirname(pkg.library_path())
    exe = str(tmp_path / "cubic_prototypes")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if os.environ.get("GSL_SINTERP_ASAN") else []
    libname = os.path.basename(pkg.library_path())[3:-3]
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Werror", *san, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "cubic_prototypes.c"), "-o", exe,
                           "-L", libdir, "-l" + libname, "-lm", "-Wl,-rpath," + libdir])
    assert "ok" in subprocess.check_output([exe], text=True)
