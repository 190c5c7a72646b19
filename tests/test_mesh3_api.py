"""Imported tetrahedral meshes, CPU part: simplex_mesh_import_nd (validation, neighbour links by face matching,
standardisation, convexity from the boundary faces), the two checkpoint layouts and the facade's argument handling.
The reference has no 3-D path (its flip logic aborts in 3-D) and no import at all: PARITY UNPINNED.
scipy.spatial.Delaunay is the QHull import; its arrays use the same convention (neighbour k opposite vertex k, -1 on the
hull), so derived links are compared for exact equality.  -m gpu part: tests/test_gpu_mesh3.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def box_points(n, seed=0):
    """the anisotropic box"""
    return np.random.default_rng(seed).random((n, 3)) * [3.0, 0.5, 20.0] + [10.0, -2.0, 100.0]


def qhull(points):
    from scipy.spatial import Delaunay
    d = Delaunay(points)
    return d, np.ascontiguousarray(d.simplices, dtype=np.int32), np.ascontiguousarray(d.neighbors, dtype=np.int32)


def cavity_and_dent(x, tet):
    """the two non-convex meshes of the convexity test: a cavity around the box centre, a dent at one hull vertex"""
    from scipy.spatial import ConvexHull
    lo, hi = x.min(axis=0), x.max(axis=0)
    z = (x - (lo + hi) / 2.0) / (hi - lo)                                       # standardised units
    cen = z[tet].mean(axis=1)
    cavity = np.ascontiguousarray(tet[np.sqrt((cen ** 2).sum(axis=1)) >= 0.25])
    v = int(ConvexHull(x).vertices[0])
    dent = np.ascontiguousarray(tet[~(tet == v).any(axis=1)])
    return cavity, dent, v


@pytest.fixture(scope="module")
def mesh400():
    x = box_points(400)
    d, tet, nbr = qhull(x)
    return x, d, tet, nbr


def import_status(pkg, x, dim, tet, nbr):
    """(handle, statuses reported to the error handler) of a raw simplex_mesh_import_nd call"""
    tet = np.ascontiguousarray(tet, dtype=np.int32)
    nbr = None if nbr is None else np.ascontiguousarray(nbr, dtype=np.int32)
    with pkg.capi.ErrorCalls() as calls:
        h = pkg.lib().simplex_mesh_import_nd(C.byref(pkg.capi.as_matrix(x)), dim, tet.ctypes.data_as(C.POINTER(C.c_int)),
                                             nbr.ctypes.data_as(C.POINTER(C.c_int)) if nbr is not None else None, len(tet))
    return h, [s for _, s in calls]


def test_import_of_a_qhull_tetrahedralisation(pkg, mesh400):
    x, d, tet, nbr = mesh400
    m = pkg.SimplexMesh.from_arrays(x, tet)                                     # neighbours == NULL: face matching
    assert m.dim() == 3 and m.n_triangles == len(tet)
    assert pkg.lib().simplex_mesh_n_points(m._h) == 400 and m.tree_nodes() is None
    assert m.triangles().shape == (len(tet), 4) and np.array_equal(m.triangles(), tet)
    assert np.array_equal(m.neighbours(), nbr)
    shift, scale = m.geometry()
    lo, hi = m.bbox()
    assert np.array_equal(lo, x.min(axis=0)) and np.array_equal(hi, x.max(axis=0))
    assert np.array_equal(shift, (lo + hi) / 2.0) and np.array_equal(scale, 1.0 / (hi - lo))
    assert m.convex()
    g = pkg.SimplexMesh.from_arrays(x, tet, nbr)                                # the links given
    assert np.array_equal(g.neighbours(), nbr) and g.convex() and g.dim() == 3
    # a zero extent gives scale 1: four points in the plane z = 5 still import (one flat tetrahedron)
    flat = np.array([[0.0, 0, 5], [1, 0, 5], [0, 1, 5], [1, 1, 5]])
    f = pkg.SimplexMesh.from_arrays(flat, np.array([[0, 1, 2, 3]], dtype=np.int32))
    assert np.array_equal(f.geometry()[1], [1.0, 1.0, 1.0]) and np.array_equal(f.geometry()[0], [0.5, 0.5, 5.0])
    assert not f.convex()                                                       # a flat boundary tetrahedron: doubt answers 0


def test_import_rejections(pkg, mesh400):
    x, d, tet, nbr = mesh400
    EINVAL, EUNIMPL = pkg.capi.GSL_EINVAL, pkg.capi.GSL_EUNIMPL
    t0 = int(np.nonzero((nbr >= 0).all(axis=1))[0][0])                          # an interior tetrahedron
    bad_vertex = tet.copy(); bad_vertex[5, 2] = 400
    repeated = tet.copy(); repeated[5, 1] = repeated[5, 0]
    one_sided = nbr.copy(); one_sided[t0, 0] = -1                               # the neighbour still points back
    wrong_face = nbr.copy(); wrong_face[t0, [0, 1]] = wrong_face[t0, [1, 0]]    # mutual, but across the wrong faces
    own = nbr.copy(); own[t0, 0] = t0
    three = np.vstack([tet, tet[:1], tet[:1]])                                  # every face of tet 0 now in three tetrahedra
    for what, (ti, ni) in {"vertex id out of range": (bad_vertex, nbr), "repeated vertex": (repeated, nbr),
                           "non-mutual link": (tet, one_sided), "link across the wrong face": (tet, wrong_face),
                           "self-neighbour": (tet, own), "face shared by three": (three, None)}.items():
        h, st = import_status(pkg, x, 3, ti, ni)
        assert not h and st == [EINVAL], what
    h, st = import_status(pkg, np.random.default_rng(1).random((50, 4)), 4, np.arange(5, dtype=np.int32)[None, :], None)
    assert not h and st == [EUNIMPL]
    h, st = import_status(pkg, x[:, :2].copy(), 3, tet, None)                   # points->size2 < dim
    assert not h and st == [EINVAL]
    h, st = import_status(pkg, x[:3].copy(), 3, np.array([[0, 1, 2, 0]], dtype=np.int32), None)   # fewer than dim + 1 points
    assert not h and st == [EINVAL]
    with pytest.raises(pkg.capi.GslError):
        pkg.SimplexMesh.from_arrays(x, bad_vertex, nbr)


def test_dim2_import_nd_is_the_2d_import(pkg, orc, tmp_path):
    x = orc.synth_centres(300, 2)
    from scipy.spatial import Delaunay
    d = Delaunay(x)
    tri, nbr = d.simplices.astype(np.int32), d.neighbors.astype(np.int32)
    for links in (nbr, None):
        a = pkg.SimplexMesh.from_arrays(x, tri, links)                          # simplex_mesh_import
        h, st = import_status(pkg, x, 2, tri, links)
        assert h and st == []
        b = pkg.SimplexMesh(h)
        assert a.dim() == 2 and b.dim() == 2
        assert np.array_equal(a.triangles(), b.triangles()) and np.array_equal(a.neighbours(), b.neighbours())
        assert a.convex() == b.convex() and a.n_triangles == b.n_triangles
        assert all(np.array_equal(p, q) for p, q in zip(a.geometry() + a.bbox(), b.geometry() + b.bbox()))
        assert a.fwrite(tmp_path / "a.bin") == 0 and b.fwrite(tmp_path / "b.bin") == 0
        blob = (tmp_path / "a.bin").read_bytes()
        assert blob == (tmp_path / "b.bin").read_bytes() and blob[:8] == b"GSLSMSH1"
        # the layout of the 2-D checkpoint, spelled out: header of four int64, 3-wide arrays, 2-wide points, 8 doubles
        assert len(blob) == 8 + 32 + 2 * 12 * len(tri) + 16 * len(x) + 64


def test_3d_checkpoint_round_trip_and_validation(pkg, mesh400, tmp_path):
    x, d, tet, nbr = mesh400
    m = pkg.SimplexMesh.from_arrays(x, tet, nbr)
    m.set_convex(False)                                                         # the flag travels, whatever was detected
    path = tmp_path / "mesh3.bin"
    assert m.fwrite(path) == 0
    blob = path.read_bytes()
    assert blob[:8] == b"GSLSMSH2" and blob[:8] != b"GSLSMSH1"
    assert len(blob) == 8 + 40 + 2 * 16 * len(tet) + 24 * len(x) + 96
    assert int.from_bytes(blob[40:48], "little") == 3                           # the header carries dim
    r = pkg.SimplexMesh.fread(path)
    assert r is not None and r.dim() == 3 and r.n_triangles == len(tet) and not r.convex()
    assert np.array_equal(r.triangles(), tet) and np.array_equal(r.neighbours(), nbr)
    assert all(np.array_equal(p, q) for p, q in zip(m.geometry() + m.bbox(), r.geometry() + r.bbox()))
    assert np.array_equal(r.points(), x)

    def load(b):
        p = tmp_path / "bad3.bin"
        p.write_bytes(bytes(b))
        with pkg.capi.ErrorCalls() as calls:
            with pkg.capi.CFile(p, "rb") as fp:
                h = pkg.lib().simplex_mesh_fread(fp)
        if h:
            pkg.lib().simplex_mesh_free(C.c_void_p(h))
        return h, [s for _, s in calls]
    EFAILED = pkg.capi.GSL_EFAILED
    assert load(blob)[0]
    for cut in (len(blob) // 2, len(blob) - 8, 30):
        h, st = load(blob[:cut])
        assert not h and st == [EFAILED]
    off_nbr = 8 + 40 + 16 * len(tet)
    t0 = int(np.nonzero((nbr >= 0).all(axis=1))[0][0])
    first = int(nbr[t0, 0])
    other = next(t for t in range(len(tet)) if t != t0 and t not in nbr[t0])
    assert int.from_bytes(blob[off_nbr + 16 * t0:off_nbr + 16 * t0 + 4], "little", signed=True) == first
    bad = bytearray(blob)
    bad[off_nbr + 16 * t0:off_nbr + 16 * t0 + 4] = other.to_bytes(4, "little", signed=True)   # a link nobody answers
    h, st = load(bad)
    assert not h and st == [EFAILED]
    bad = bytearray(blob)
    bad[8 + 40:8 + 44] = (10 ** 6).to_bytes(4, "little")                        # vertex id out of range
    assert not load(bad)[0]
    bad = bytearray(blob)
    bad[40:48] = (4).to_bytes(8, "little")                                      # a dim the format does not hold
    assert not load(bad)[0]


def test_convexity_from_the_boundary_faces(pkg, mesh400):
    x, d, tet, nbr = mesh400
    cavity, dent, _ = cavity_and_dent(x, tet)
    assert 0 < len(cavity) < len(tet) and 0 < len(dent) < len(tet)
    for part in (cavity, dent):
        m = pkg.SimplexMesh.from_arrays(x, part)
        assert not m.convex()
        m.set_convex(True)
        assert m.convex()
    m = pkg.SimplexMesh.from_arrays(x, tet)
    assert m.convex()
    m.set_convex(False)
    assert not m.convex()
    # coplanar hull faces are not reflex edges: a cube cut into five tetrahedra
    cube = np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], dtype=np.float64)
    five = np.array([[0, 3, 5, 6], [0, 1, 3, 5], [0, 2, 3, 6], [0, 4, 5, 6], [3, 5, 6, 7]], dtype=np.int32)
    assert pkg.SimplexMesh.from_arrays(cube, five).convex()
    assert not pkg.SimplexMesh.from_arrays(cube, five[[1, 2, 3, 4]]).convex()   # the core removed: four corners touching at edges


def test_facade_accepts_dim_3(pkg, mesh400):
    x, d, tet, nbr = mesh400
    f = np.ascontiguousarray(x[:, 0])
    s = pkg.Sinterp("linear_mesh", 3, 400)
    assert s.name() == "linear-imported-triangulation"
    with pytest.raises(pkg.capi.GslError):
        pkg.Sinterp("linear_mesh", 4, 400)
    with pytest.raises(pkg.capi.GslError):
        pkg.Sinterp("linear_mesh", 1, 400)
    assert s.init(x, f) == pkg.GSL_EINVAL                                       # no triangulation yet
    assert s.set_triangulation(tet, nbr) == 0                                   # 4 ids per simplex are read
    y = np.zeros((2, 3))
    assert s.eval_grad_many(y)[0] == pkg.capi.GSL_EUNSUP
    assert s.init_fields(x, np.ascontiguousarray(np.stack([f, f], axis=1))) == pkg.capi.GSL_EUNSUP
    assert pkg.Sinterp("linear_mesh", 2, 400) is not None                       # the 2-D type is where it was


def test_c_program_references_the_mesh3_prototypes(pkg, tmp_path):
    libdir = os.path.dirname(pkg.library_path())
    exe = str(tmp_path / "mesh3_prototypes")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if os.environ.get("GSL_SINTERP_ASAN") else []
    libname = os.path.basename(pkg.library_path())[3:-3]
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Werror", *san, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "mesh3_prototypes.c"), "-o", exe,
                           "-L", libdir, "-l" + libname, "-lm", "-Wl,-rpath," + libdir])
    assert "ok" in subprocess.check_output([exe], text=True)
