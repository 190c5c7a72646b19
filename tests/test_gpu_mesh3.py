"""-m gpu: imported tetrahedral meshes -- grid seed + walk over the face links (csrc/hip/mesh3.hip).
PARITY UNPINNED: the reference has no 3-D path (its flip logic aborts in 3-D) and no import, so
there is no oracle.  The references are scipy (Delaunay = the QHull import, find_simplex, LinearNDInterpolator) and plain
numpy fp64: barycentric coordinates by np.linalg.solve in the mesh's standardised coordinates.  Tolerances: 1e-9 is
MESH_GAP, the project's acceptance of a least violating simplex; 1e-10 max|f| is the project's value tolerance (the numpy
formula alone reproduces a linear response to ~4e-16 on these meshes).  CPU part: tests/test_mesh3_api.py."""
import numpy as np
import pytest

from gpu_util import bits
from test_mesh3_api import box_points, cavity_and_dent, qhull

pytestmark = pytest.mark.gpu

GAP = 1e-9


def linear(p):
    return 1.3 * p[:, 0] - 0.7 * p[:, 1] + 0.05 * p[:, 2] + 2.0


def standardise(mesh, p):
    shift, scale = mesh.geometry()
    return scale * (p - shift)


def coords_in(z, tet, ids, zy):
    """numpy barycentric coordinates [k, 4] of the standardised targets zy[k] in the tetrahedra tet[ids[k]]"""
    v = z[tet[ids]]                                             # [k, 4, 3]
    M = np.transpose(v[:, :3, :] - v[:, 3:4, :], (0, 2, 1))     # columns = edges
    c = np.linalg.solve(M, (zy - v[:, 3, :])[:, :, None])[:, :, 0]
    return np.concatenate([c, 1.0 - c.sum(axis=1, keepdims=True)], axis=1)


def violation(c):
    return np.maximum(np.maximum(-c, c - 1.0).max(axis=-1), 0.0)


def flat_mask(z, tet):
    """the singular rule of the pack: |det| <= 1e-12 x the product of the three standardised edge lengths"""
    e = z[tet[:, :3]] - z[tet[:, 3:4]]
    return ~(np.abs(np.linalg.det(e)) > 1e-12 * np.linalg.norm(e, axis=2).prod(axis=1))


def brute_force(z, tet, zy):
    """(least violation, its tetrahedron) over all non-flat tetrahedra, for every standardised target"""
    ok = np.nonzero(~flat_mask(z, tet))[0]
    v = z[tet[ok]]
    Minv = np.linalg.inv(np.transpose(v[:, :3, :] - v[:, 3:4, :], (0, 2, 1)))     # [t, 3, 3]
    best = np.full(len(zy), np.inf)
    arg = np.full(len(zy), -1)
    for s in range(0, len(zy), 256):
        b = zy[s:s + 256, None, :] - v[None, :, 3, :]                              # [k, t, 3]
        c = np.einsum("tij,ktj->kti", Minv, b)
        c = np.concatenate([c, 1.0 - c.sum(axis=2, keepdims=True)], axis=2)
        vi = violation(c)
        a = vi.argmin(axis=1)
        best[s:s + 256] = vi[np.arange(len(a)), a]
        arg[s:s + 256] = ok[a]
    return best, arg


_cache = {}


def scene(pkg, n):
    """points of the anisotropic box, their QHull tetrahedralisation, the mesh and its device mirror: built once per n"""
    if n not in _cache:
        x = box_points(n)
        d, tet, nbr = qhull(x)
        mesh = pkg.SimplexMesh.from_arrays(x, tet, nbr)
        _cache[n] = (x, d, tet, nbr, mesh, mesh.device_alloc(0))
    return _cache[n]


def smooth(orc, mesh, x):
    return orc.synth_response(np.ascontiguousarray(standardise(mesh, x)))


@pytest.mark.parametrize("n,m", [(60, 5000), (3000, 20000)])
def test_qhull_import_through_scipy(pkg, orc, n, m):
    from scipy.interpolate import LinearNDInterpolator
    x, d, tet, nbr, mesh, dev = scene(pkg, n)
    assert mesh.convex() and mesh.dim() == 3
    z = standardise(mesh, x)
    f = smooth(orc, mesh, x)
    rng = np.random.default_rng(7)
    lo, hi = mesh.bbox()
    y = np.ascontiguousarray(lo + rng.random((m, 3)) * (hi - lo))
    y[-20:] += 100.0                                            # far outside
    assert dev.set_response(f) == 0
    st, vals, idx = dev.eval_many(y)
    assert st == pkg.GSL_EDOM and (idx[-20:] == -1).all() and np.isnan(vals[-20:]).all()
    assert ((idx >= -1) & (idx < len(tet))).all()
    inside = idx >= 0
    assert np.isnan(vals[~inside]).all() and np.isfinite(vals[inside]).all()
    sfind = d.find_simplex(y)
    differ = np.nonzero(inside != (sfind >= 0))[0]
    zy = standardise(mesh, y)
    print(f"n={n}: {inside.sum()} of {m} inside, {len(differ)} differ from find_simplex")
    assert len(differ) <= 3                                     # hull-face rounding
    if len(differ):
        least, _ = brute_force(z, tet, zy[differ])
        print("least violations of the exceptions:", least)
        assert (least <= GAP).all()
    c = coords_in(z, tet, idx[inside], zy[inside])
    print("min coordinate in the returned tetrahedra:", c.min())
    assert c.min() >= -GAP
    ref = LinearNDInterpolator(d, f)(y)
    both = inside & (sfind >= 0)
    err = np.abs(vals[both] - ref[both]).max()
    print("value error against LinearNDInterpolator:", err, "of", np.abs(f).max())
    assert err <= 1e-10 * np.abs(f).max()
    # batch independence: a shuffled half (5000 -> 2500 leaves the sorted route) gives the same indices and bits
    p = rng.permutation(m)[: m // 2]
    st2, vals2, idx2 = dev.eval_many(np.ascontiguousarray(y[p]))
    assert np.array_equal(idx2, idx[p]) and np.array_equal(bits(vals2), bits(vals[p]))
    # a linear response is reproduced
    fl = linear(x)
    assert dev.set_response(fl) == 0
    st3, vl, il = dev.eval_many(y)
    assert st3 == pkg.GSL_EDOM and np.array_equal(il, idx)
    errl = np.abs(vl[inside] - linear(y[inside])).max()
    print("linear reproduction error:", errl, "of", np.abs(fl).max())
    assert errl <= 1e-10 * np.abs(fl).max()


def test_one_tetrahedron(pkg):
    """The smallest mesh.  The vertices are chosen so that the standardised edge matrix and its inverse are small
    integers: then the coordinates of a vertex are exactly a unit vector and "a vertex returns its datum" can be asked
    with ==.  (For a general tetrahedron the inverse is rounded and the skeleton test's 1e-12 max|f| applies; the last
    vertex, the origin of the frame, is exact in any tetrahedron.)"""
    x = np.array([[0.0, 0, 0], [4, 0, 0], [4, 4, 0], [0, 0, 4]])
    f = np.array([0.1, -2.7, 3.3, 1000.0 + 1.0 / 3.0])
    mesh = pkg.SimplexMesh.from_arrays(x, np.array([[0, 1, 2, 3]], dtype=np.int32))
    assert mesh.convex() and np.array_equal(mesh.neighbours(), [[-1, -1, -1, -1]])
    dev = mesh.device_alloc(0)
    assert dev.set_response(f) == 0
    cen = x.mean(axis=0)
    st, vals, idx = dev.eval_many(np.ascontiguousarray(np.vstack([cen, x])))
    assert st == pkg.GSL_SUCCESS and (idx == 0).all()
    assert np.array_equal(vals[1:], f)                          # exactly
    assert abs(vals[0] - f.mean()) <= 4e-16 * np.abs(f).max()
    mirrored = []
    for k in range(4):                                          # the centroid reflected through the face opposite vertex k
        a, b, c = x[[i for i in range(4) if i != k]]
        nrm = np.cross(b - a, c - a)
        mirrored.append(cen - 2.0 * np.dot(cen - a, nrm) / np.dot(nrm, nrm) * nrm)
    st, vals, idx = dev.eval_many(np.ascontiguousarray(np.array(mirrored)))
    assert st == pkg.GSL_EDOM and (idx == -1).all() and np.isnan(vals).all()
    st, vals, idx = dev.eval_many(np.array([[1.0, np.nan, 1.0]]))
    assert st == pkg.GSL_EDOM and idx[0] == -1 and np.isnan(vals[0])            # a NaN coordinate: outside
    assert dev.eval_many(np.zeros((3, 2)))[0] == pkg.capi.GSL_EBADLEN           # M x 3 targets for a 3-D mesh


def test_targets_on_the_mesh_skeleton(pkg, orc):
    """Data points, edge midpoints and face centroids lie on the boundary of several tetrahedra; within rounding of an
    edge or a vertex the closed test can fail in all of them and the walk circles: it must still return one of them."""
    x, d, tet, nbr, mesh, dev = scene(pkg, 400)
    z = standardise(mesh, x)
    f = smooth(orc, mesh, x)
    rng = np.random.default_rng(11)
    verts = rng.choice(400, 200, replace=False)
    te = rng.choice(len(tet), 300)
    ea, eb = rng.integers(0, 4, 300), rng.integers(1, 4, 300)
    mids = 0.5 * (x[tet[te, ea]] + x[tet[te, (ea + eb) % 4]])
    tf = rng.choice(len(tet), 300)
    drop = rng.integers(0, 4, 300)
    faces = np.array([np.delete(tet[t], k) for t, k in zip(tf, drop)])
    cents = x[faces].sum(axis=1) / 3.0
    y = np.ascontiguousarray(np.vstack([x[verts], mids, cents]))
    assert dev.set_response(f) == 0
    st, vals, idx = dev.eval_many(y)
    assert st == pkg.GSL_SUCCESS and (idx >= 0).all()
    viol = violation(coords_in(z, tet, idx, standardise(mesh, y)))
    print("worst violation in the returned tetrahedra:", viol.max(), "; not contained under the closed rule:", (viol > 0).sum())
    assert viol.max() <= GAP
    assert np.abs(vals[:200] - f[verts]).max() <= 1e-12 * np.abs(f).max()
    fl = linear(x)
    assert dev.set_response(fl) == 0
    st, vl, il = dev.eval_many(y)
    assert st == pkg.GSL_SUCCESS and np.array_equal(il, idx)
    assert np.abs(vl - linear(y)).max() <= 1e-10 * np.abs(fl).max()


def test_lattice_with_flat_tetrahedra(pkg):
    """QHull returns exactly flat tetrahedra for cospherical input (a cube's eight corners); after standardisation their
    determinant is rounding residue.  They carry the singular flag and never contain a target."""
    g = np.arange(6, dtype=np.float64)
    x = np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3))
    d, tet, nbr = qhull(x)
    mesh = pkg.SimplexMesh.from_arrays(x, tet, nbr)
    z = standardise(mesh, x)
    flat = flat_mask(z, tet)
    print(f"{flat.sum()} of {len(tet)} tetrahedra are flat; convex detected: {mesh.convex()}")
    assert flat.sum() > 0.05 * len(tet)
    fl = linear(x)
    dev = mesh.device_alloc(0)
    assert dev.set_response(fl) == 0
    y = np.ascontiguousarray(1e-6 + np.random.default_rng(13).random((1000, 3)) * (5.0 - 2e-6))
    st, vals, idx = dev.eval_many(y)
    assert st == pkg.GSL_SUCCESS and (idx >= 0).all()
    assert not flat[idx].any()
    assert violation(coords_in(z, tet, idx, standardise(mesh, y))).max() <= GAP
    assert np.abs(vals - linear(y)).max() <= 1e-10 * np.abs(fl).max()


def test_cavity_mesh_uses_the_scan(pkg):
    """The n = 400 mesh with a cavity around the box centre (CPU test: convex == 0 detected).  A walk that runs into the
    cavity's wall proves nothing: such targets go to the exhaustive scan, which finds the targets behind the cavity
    (seed cells inside it are filled from one side, so many walks start across it) and rejects those inside it."""
    x, d, tet, nbr, _, _ = scene(pkg, 400)
    cavity, _, _ = cavity_and_dent(x, tet)
    mesh = pkg.SimplexMesh.from_arrays(x, cavity)
    assert not mesh.convex()
    z = standardise(mesh, x)
    fl = linear(x)
    dev = mesh.device_alloc(0)
    assert dev.set_response(fl) == 0
    rng = np.random.default_rng(17)
    u = rng.normal(size=(1500, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    zy = u * rng.uniform(0.02, 0.42, size=(1500, 1))            # standardised: inside the cavity and all around it
    shift, scale = mesh.geometry()
    y = np.ascontiguousarray(zy / scale + shift)
    st, vals, idx = dev.eval_many(y)
    least, arg = brute_force(z, cavity, standardise(mesh, y))
    must_in, must_out = least == 0.0, least > 1e-6
    print(f"{must_in.sum()} targets in the mesh, {must_out.sum()} outside it or in the cavity")
    assert must_in.sum() > 300 and must_out.sum() > 100 and st == pkg.GSL_EDOM
    assert (idx[must_out] == -1).all() and np.isnan(vals[must_out]).all()
    assert (idx[must_in] >= 0).all()
    assert violation(coords_in(z, cavity, idx[must_in], standardise(mesh, y[must_in]))).max() <= GAP
    assert np.abs(vals[must_in] - linear(y[must_in])).max() <= 1e-10 * np.abs(fl).max()
    inside_cavity = np.linalg.norm(zy, axis=1) < 0.1           # well inside: every removed centroid lay within 0.25
    assert inside_cavity.sum() > 10 and (idx[inside_cavity] == -1).all()
    # declared convex, the same walls would be taken for the hull: the override is honoured (no scan, cavity targets still outside)
    mesh.set_convex(True)
    dev2 = mesh.device_alloc(0)
    assert dev2.set_response(fl) == 0
    st2, v2, i2 = dev2.eval_many(y)
    assert (i2[inside_cavity] == -1).all() and (i2[i2 >= 0] == idx[i2 >= 0]).all()


def test_large_batch_two_level_reorder(pkg, orc):
    """m = 300 000 >= 2^18 takes the two-level reorder in 3-D; chunks of 1000 take the unsorted route: same indices, same bits."""
    x, d, tet, nbr, mesh, dev = scene(pkg, 3000)
    f = smooth(orc, mesh, x)
    assert dev.set_response(f) == 0
    lo, hi = mesh.bbox()
    m = 300_000
    y = np.ascontiguousarray(lo + np.random.default_rng(19).random((m, 3)) * (hi - lo))
    st, vals, idx = dev.eval_many(y)
    assert st in (pkg.GSL_SUCCESS, pkg.GSL_EDOM) and (idx >= 0).sum() > 0.5 * m
    v = np.empty(m)
    i = np.empty(m, dtype=np.int32)
    for s in range(0, m, 1000):
        assert dev.eval_many(np.ascontiguousarray(y[s:s + 1000]), out=(v[s:s + 1000], i[s:s + 1000]))[0] in (pkg.GSL_SUCCESS, pkg.GSL_EDOM)
    assert np.array_equal(i, idx) and np.array_equal(bits(v), bits(vals))


@pytest.mark.parametrize("m", [1000, 6000])
def test_resident_entry_with_padded_rows(pkg, orc, m):
    import torch
    x, d, tet, nbr, mesh, dev = scene(pkg, 400)
    f = smooth(orc, mesh, x)
    assert dev.set_response(f) == 0
    lo, hi = mesh.bbox()
    y = np.ascontiguousarray(lo + np.random.default_rng(23).random((m, 3)) * (hi - lo))
    st, vals, idx = dev.eval_many(y)
    pad = np.full((m, 5), 7.0)
    pad[:, :3] = y
    ty = torch.from_numpy(pad).cuda()
    tv = torch.empty(m, dtype=torch.float64, device="cuda")
    ti = torch.empty(m, dtype=torch.int32, device="cuda")
    assert dev.eval_resident(ty.data_ptr(), m, 5, tv.data_ptr(), ti.data_ptr()) == 0
    assert pkg.lib().gsl_sinterp_hip_sync(dev.ctx_handle()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(ti.cpu().numpy(), idx) and np.array_equal(bits(tv.cpu().numpy()), bits(vals))
    assert dev.eval_resident(ty.data_ptr(), m, 2, tv.data_ptr(), ti.data_ptr()) == pkg.capi.GSL_EBADLEN


def test_facade_type_in_3d(pkg, orc, tmp_path):
    n, m = 3000, 20000
    x, d, tet, nbr, mesh, dev = scene(pkg, n)
    f = smooth(orc, mesh, x)
    assert dev.set_response(f) == 0
    lo, hi = mesh.bbox()
    y = np.ascontiguousarray(lo + np.random.default_rng(29).random((m, 3)) * (hi - lo))
    st0, v0, t0 = dev.eval_many(y)
    s = pkg.Sinterp("linear_mesh", 3, n, 0)
    assert s.init(x, f) == pkg.GSL_EINVAL                      # no triangulation yet
    assert s.set_triangulation(tet) == 0 and s.init(x, f) == 0
    st1, v1, t1 = s.eval_many(y, want_leaf=True)
    assert st1 == st0 and np.array_equal(bits(v1), bits(v0)) and np.array_equal(t1, t0)
    for k in range(12):
        st, val = s.eval_e(y[k])
        assert st == (pkg.GSL_SUCCESS if t0[k] >= 0 else pkg.GSL_EDOM)
        assert bits(np.array([val]))[0] == bits(v0[k:k + 1])[0]
    assert s.eval_grad_many(y[:4])[0] == pkg.capi.GSL_EUNSUP
    path = tmp_path / "mesh3_interp.bin"
    assert s.fwrite(path) == 0
    r = pkg.Sinterp("linear_mesh", 3, n, 0)
    assert r.fread(path) == 0
    st2, v2, t2 = r.eval_many(y, want_leaf=True)
    assert st2 == st0 and np.array_equal(bits(v2), bits(v0)) and np.array_equal(t2, t0)
    assert pkg.Sinterp("linear_mesh", 2, n, 0).fread(path) == pkg.capi.GSL_EBADLEN
    g = pkg.Sinterp("linear_mesh", 3, n, 0)
    assert g.set_device_list([0, 0]) == 0 and g.set_triangulation(tet, nbr) == 0 and g.init(x, f) == 0
    assert g.n_devices() == 2
    st3, v3, t3 = g.eval_many(y, want_leaf=True)
    assert st3 == st0 and np.array_equal(bits(v3), bits(v0)) and np.array_equal(t3, t0)
