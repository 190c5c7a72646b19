"""-m gpu: natural-neighbour (Sibson) interpolation on 2-D Delaunay meshes (csrc/hip/natural.hip).  PARITY UNPINNED: the
reference lists "Voronoi" interpolation as future work only.  The reference here is a CLIPPING ORACLE written below in
plain Python floats: the Voronoi cell of the target y is a box around y clipped by the N half-planes "closer to y than
to x_j"; the part of it stolen from site i is that cell clipped by the half-planes "closer to x_i than to x_j"; lambda_i
= area_i / area.  It shares nothing with the kernel's cavity formula.  Values are compared at the project's value
tolerance, 1e-10 max|f|; the oracle's own linear-precision defect |sum lambda_i x_i - y| is asserted <= 1e-12 for every
target it is used on.

Observed on one MI355X (max |value - oracle| / max|f|; printed by every test):
    random N = 12: 2.6e-15   random N = 60: 4.4e-16   on / near interior edges: 4.6e-15   7 x 7 lattice: 8.6e-15
    clustered cloud: 6.6e-16   96 cocircular sites: 5.2e-16   (oracle's own linear-precision defect <= 7.2e-15)
    linear precision, N = 2000, M = 20000: 5.5e-16;  walk against scan at depth_cap = 1: 5.5e-16 (220 of 300 targets of
    the N = 60 cloud and all 30 of the circle take the scan there; none does at the default cap)
    smallest depth_cap without a scanned target: 3 (N = 60), 2 (circle);  natural_simplex near its hull, linear f: 6.1e-16
"""
import ctypes as C

import numpy as np
import pytest

from gpu_util import bits

pytestmark = pytest.mark.gpu

TOL = 1e-10


# ---------------------------------------------------------------------------------------------- the clipping oracle
def _clip(poly, nx, ny, c):
    """the part of the convex polygon (list of (x, y)) with nx x + ny y <= c"""
    out = []
    k = len(poly)
    for a in range(k):
        px, py = poly[a]
        qx, qy = poly[(a + 1) % k]
        dp, dq = nx * px + ny * py - c, nx * qx + ny * qy - c
        if dp <= 0.0:
            out.append((px, py))
        if (dp < 0.0 < dq) or (dq < 0.0 < dp):
            t = dp / (dp - dq)
            out.append((px + (qx - px) * t, py + (qy - py) * t))
    return out


def _area(poly):
    s = 0.0
    for a in range(len(poly)):
        px, py = poly[a]
        qx, qy = poly[(a + 1) % len(poly)]
        s += px * qy - py * qx
    return 0.5 * s


def _cell(p, box):
    lo0, lo1, hi0, hi1 = box
    cell = [(lo0, lo1), (hi0, lo1), (hi0, hi1), (lo0, hi1)]
    for px, py in p:
        cell = _clip(cell, px, py, 0.5 * (px * px + py * py))        # closer to 0 (= y) than to p_j
    return cell


def sibson_oracle(x, y):
    """(lambda [N], linear-precision defect) of the target y, in coordinates relative to y"""
    p = [(float(a - y[0]), float(b - y[1])) for a, b in x]
    b = 4.0
    while True:                                                       # a box the cell does not touch
        cell = _cell(p, (-b, -b, b, b))
        if max(max(abs(vx), abs(vy)) for vx, vy in cell) < b or b > 1e6:
            break
        b *= 4.0
    xs, ys = [v[0] for v in cell], [v[1] for v in cell]
    w, h = max(xs) - min(xs), max(ys) - min(ys)                       # again from a tight box: vertex errors ~ eps * cell size
    cell = _cell(p, (min(xs) - 0.25 * w, min(ys) - 0.25 * h, max(xs) + 0.25 * w, max(ys) + 0.25 * h))
    tot = _area(cell)
    lam = np.zeros(len(p))
    for i, (ax, ay) in enumerate(p):
        a2 = ax * ax + ay * ay
        part = cell
        for j, (bx, by) in enumerate(p):
            if j == i:
                continue
            part = _clip(part, bx - ax, by - ay, 0.5 * ((bx * bx + by * by) - a2))    # closer to p_i than to p_j
            if len(part) < 3:
                break
        if len(part) >= 3:
            lam[i] = _area(part)
    lam /= tot
    return lam, float(np.abs(lam @ x - y).max())


def response(x):
    return np.sin(3.0 * x[:, 0]) + np.cos(2.0 * x[:, 1]) + x[:, 0] * x[:, 1]


def qhull_mesh(pkg, x):
    from scipy.spatial import Delaunay
    d = Delaunay(x)
    tri, nbr = np.ascontiguousarray(d.simplices, dtype=np.int32), np.ascontiguousarray(d.neighbors, dtype=np.int32)
    mesh = pkg.SimplexMesh.from_arrays(x, tri, nbr)
    assert mesh.delaunay_metric() == 1 and mesh.convex()
    return d, tri, nbr, mesh


def compare_with_oracle(pkg, x, y, what, min_inside=1):
    """natural values of the cloud x at the targets y against the oracle; returns (values, triangles)"""
    f = response(x)
    d, tri, nbr, mesh = qhull_mesh(pkg, x)
    dev = mesh.device_alloc(0)
    assert dev.set_response(f) == 0
    y = np.ascontiguousarray(y)
    st, v, t = dev.eval_natural_many(y)
    inside = t >= 0
    assert st == (pkg.GSL_SUCCESS if inside.all() else pkg.GSL_EDOM)
    assert np.isnan(v[~inside]).all() and np.isfinite(v[inside]).all() and inside.sum() >= min_inside
    worst = defect = 0.0
    for k in np.nonzero(inside)[0]:
        lam, lp = sibson_oracle(x, y[k])
        defect = max(defect, lp)
        worst = max(worst, abs(v[k] - lam @ f))
    fmax = np.abs(f).max()
    print(f"{what}: {inside.sum()} of {len(y)} targets inside, max |value - oracle| = {worst / fmax:.2e} max|f|, "
          f"oracle linear-precision defect {defect:.2e}")
    assert defect <= 1e-12
    assert worst <= TOL * fmax
    return v, t


# ---------------------------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("n", [12, 60])
def test_random_clouds_match_the_clipping_oracle(pkg, n):
    rng = np.random.default_rng(100 + n)
    x = rng.random((n, 2))
    y = 0.02 + 0.96 * rng.random((300, 2))
    compare_with_oracle(pkg, x, y, f"random N = {n}", min_inside=100)


def test_targets_on_and_near_interior_edges(pkg):
    rng = np.random.default_rng(160)
    x = rng.random((60, 2))
    from scipy.spatial import Delaunay
    d = Delaunay(x)
    edges = [(d.simplices[t, (k + 1) % 3], d.simplices[t, (k + 2) % 3]) for t in range(len(d.simplices)) for k in range(3)
             if d.neighbors[t, k] > t]
    pick = rng.choice(len(edges), 100, replace=False)
    ys = []
    for e in pick:
        a, b = x[edges[e][0]], x[edges[e][1]]
        on = a + rng.uniform(0.2, 0.8) * (b - a)
        nrm = np.array([-(b - a)[1], (b - a)[0]]) / np.hypot(*(b - a))
        ys += [on + off * nrm for off in (0.0, 1e-14, 1e-10, 1e-6)]
    v, t = compare_with_oracle(pkg, x, np.array(ys), "N = 60, on and 1e-14 / 1e-10 / 1e-6 off interior edges", min_inside=400)


def test_lattice_everything_cocircular(pkg):
    g = np.stack(np.meshgrid(np.arange(7.0), np.arange(7.0), indexing="ij"), axis=-1).reshape(-1, 2) / 6.0
    rng = np.random.default_rng(7)
    inner = g[((g > 0.1) & (g < 0.9)).all(axis=1)]
    cells = (inner[:, None, :] + np.array([[0.5, 0.5], [0.5, 0.0], [0.0, 0.5]]) / 6.0).reshape(-1, 2)     # centres and edge midpoints
    cells = cells[((cells > 0.1) & (cells < 0.9)).all(axis=1)]
    y = np.vstack([0.1 + 0.8 * rng.random((60, 2)), inner + 1e-13, cells])
    compare_with_oracle(pkg, g, y, "7 x 7 lattice", min_inside=len(y))


def test_clustered_cloud_across_the_cluster_boundary(pkg):
    rng = np.random.default_rng(40)
    x = np.vstack([rng.random((40, 2)), 0.495 + 0.01 * rng.random((40, 2))])
    ang, r = rng.uniform(0, 2 * np.pi, 100), rng.uniform(0.0, 0.03, 100)
    y = 0.5 + np.stack([r * np.cos(ang), r * np.sin(ang)], axis=1)
    compare_with_oracle(pkg, x, y, "40 uniform + 40 clustered", min_inside=100)


def circle_cloud():
    a = 2.0 * np.pi * np.arange(96) / 96.0
    return np.stack([np.cos(a), np.sin(a)], axis=1)


def test_cocircular_sites_every_cavity_is_the_whole_mesh(pkg):
    x = circle_cloud()
    rng = np.random.default_rng(96)
    a, r = rng.uniform(0, 2 * np.pi, 30), 0.5 * np.sqrt(rng.random(30))
    y = np.stack([r * np.cos(a), r * np.sin(a)], axis=1)
    compare_with_oracle(pkg, x, y, "96 cocircular sites", min_inside=30)


# ---------------------------------------------------------------------------------------------- the raw entries
class RawMesh:
    """the raw device route: mesh_pack + tree_bind + mesh_eval (locate, linear value), natural_pack + natural_eval"""

    def __init__(self, pkg, x, tri, nbr, f):
        import torch
        self.pkg, self.torch = pkg, torch
        self.ctx = pkg.capi.HipContext(0)
        self.nt, self.npts = len(tri), len(x)
        dev = "cuda"
        self.d_tri = torch.from_numpy(np.ascontiguousarray(tri, dtype=np.int32)).to(dev)
        self.d_nbr = torch.from_numpy(np.ascontiguousarray(nbr, dtype=np.int32)).to(dev)
        self.d_pts = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)
        self.d_f = torch.from_numpy(np.ascontiguousarray(f, dtype=np.float64)).to(dev)
        lo, hi = x.min(axis=0), x.max(axis=0)
        self.geom = np.concatenate([(lo + hi) / 2.0, 1.0 / (hi - lo), lo, hi])
        self.G = max(1, int(np.ceil(np.sqrt(self.nt / 2.0))))
        self.d_rec = torch.zeros(self.nt * 64 // 8 + 8, dtype=torch.float64, device=dev)
        self.d_tab = torch.zeros(self.nt * 32 // 8, dtype=torch.float64, device=dev)
        self.d_seed = torch.zeros(2 * self.G * self.G, dtype=torch.int32, device=dev)
        self.d_nn = torch.zeros((self.nt + 1) * pkg.capi.NATURAL_RECORD_BYTES // 8, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        L, h = pkg.lib(), self.ctx._h
        self.rec_ptr = (self.d_rec.data_ptr() + 63) // 64 * 64
        g = self.geom.ctypes.data_as(C.POINTER(C.c_double))
        assert L.gsl_sinterp_hip_mesh_pack(h, self.nt, self.d_tri.data_ptr(), self.d_nbr.data_ptr(), self.npts, self.d_pts.data_ptr(), g,
                                           self.G, self.rec_ptr, self.d_seed.data_ptr()) == 0
        self.ctx.tree_bind(self.nt, self.d_tri.data_ptr(), self.npts, self.d_f.data_ptr(), self.d_tab.data_ptr())
        self.ctx.mesh_natural_pack(self.nt, self.d_tri.data_ptr(), self.d_nbr.data_ptr(), self.npts, self.d_pts.data_ptr(), [1.0, 1.0],
                                   self.d_nn.data_ptr())
        self.ctx.sync()

    def natural(self, y, depth_cap):
        """(values, triangles, number of targets that took the scan)"""
        torch, L, h = self.torch, self.pkg.lib(), self.ctx._h
        m = len(y)
        d_y = torch.from_numpy(np.ascontiguousarray(y)).to("cuda")
        d_lin = torch.empty(m, dtype=torch.float64, device="cuda")
        d_out = torch.empty(m, dtype=torch.float64, device="cuda")
        d_loc = torch.empty(m, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        g = self.geom.ctypes.data_as(C.POINTER(C.c_double))
        st = L.gsl_sinterp_hip_mesh_eval(h, self.nt, self.rec_ptr, self.d_tab.data_ptr(), self.d_seed.data_ptr(), self.G, g, 1, d_y.data_ptr(),
                                         m, 2, d_lin.data_ptr(), d_loc.data_ptr(), None)
        assert st == 0
        scanned = self.ctx.mesh_natural_eval(self.nt, self.d_nn.data_ptr(), self.d_tab.data_ptr(), d_loc.data_ptr(), d_lin.data_ptr(),
                                             d_y.data_ptr(), m, 2, d_out.data_ptr(), depth_cap)
        self.ctx.sync()
        return d_out.cpu().numpy(), d_loc.cpu().numpy(), scanned


def test_depth_cap_drives_the_scan_and_it_agrees_with_the_walk(pkg):
    from scipy.spatial import Delaunay
    rng = np.random.default_rng(160)
    clouds = {"N = 60": (rng.random((60, 2)), 0.2 + 0.6 * rng.random((300, 2)))}
    a, r = rng.uniform(0, 2 * np.pi, 30), 0.5 * np.sqrt(rng.random(30))
    clouds["circle"] = (circle_cloud(), np.stack([r * np.cos(a), r * np.sin(a)], axis=1))
    for name, (x, y) in clouds.items():
        f = response(x)
        d = Delaunay(x)
        raw = RawMesh(pkg, x, d.simplices, d.neighbors, f)
        v0, t0, s0 = raw.natural(y, 0)
        v1, t1, s1 = raw.natural(y, 1)
        inside = t0 >= 0
        assert inside.sum() >= {"N = 60": 300, "circle": 30}[name] and np.array_equal(t0, t1)
        diff = np.abs(v0[inside] - v1[inside]).max() / np.abs(f).max()
        print(f"{name}: default cap {s0} scanned, depth_cap = 1 {s1} scanned of {len(y)}; max |walk - scan| = {diff:.2e} max|f|")
        assert s1 > 0
        assert diff <= 1e-12
        assert s0 == 0                                                 # the default cap holds every cavity of these clouds
        need = next(c for c in range(1, pkg.capi.NATURAL_STACK + 1) if raw.natural(y, c)[2] == 0)
        print(f"{name}: smallest depth_cap without a scanned target = {need} (pending triangles a lane holds at most)")
        # the raw route and the mirror are the same computation
        mesh = pkg.SimplexMesh.from_arrays(x, d.simplices.astype(np.int32), d.neighbors.astype(np.int32))
        dev = mesh.device_alloc(0)
        assert dev.set_response(f) == 0
        st, v, t = dev.eval_natural_many(np.ascontiguousarray(y))
        assert np.array_equal(t, t0) and np.array_equal(bits(v[inside]), bits(v0[inside]))


# ---------------------------------------------------------------------------------------------- properties
@pytest.fixture(scope="module")
def cloud2000(pkg):
    rng = np.random.default_rng(2000)
    x = rng.random((2000, 2))
    f = 2.0 * x[:, 0] - 3.0 * x[:, 1] + 0.5
    d, tri, nbr, mesh = qhull_mesh(pkg, x)
    dev = mesh.device_alloc(0)
    assert dev.set_response(f) == 0
    return x, f, d, mesh, dev


def test_linear_precision_and_the_sorted_route(pkg, cloud2000):
    from scipy.spatial import ConvexHull
    x, f, d, mesh, dev = cloud2000
    rng = np.random.default_rng(1)
    hull = x[ConvexHull(x).vertices]
    c = hull.mean(axis=0)
    shrunk = c + 0.99 * (hull - c)                                   # the hull shrunk by 1 %
    ys = []
    while sum(len(a) for a in ys) < 20000:
        cand = rng.random((30000, 2))
        e0, e1 = shrunk, np.roll(shrunk, -1, axis=0)                   # counter-clockwise: inside = left of every edge
        left = ((e1 - e0)[None, :, 0] * (cand[:, None, 1] - e0[None, :, 1]) - (e1 - e0)[None, :, 1] * (cand[:, None, 0] - e0[None, :, 0])) > 0
        ys.append(cand[left.all(axis=1)])
    y = np.ascontiguousarray(np.vstack(ys)[:20000])
    st, v, t = dev.eval_natural_many(y)                               # >= 4096: located through the sorted route
    assert st == 0 and (t >= 0).all()
    want = 2.0 * y[:, 0] - 3.0 * y[:, 1] + 0.5
    err = np.abs(v - want).max() / np.abs(f).max()
    print(f"linear precision, N = 2000, M = 20000: max |s - f(y)| = {err:.2e} max|f|")
    assert err <= 1e-12
    # alone, in a batch of 100, in the batch of 20000: the same bits
    pick = rng.choice(20000, 100, replace=False)
    st, v100, t100 = dev.eval_natural_many(np.ascontiguousarray(y[pick]))
    assert st == 0 and np.array_equal(bits(v100), bits(v[pick])) and np.array_equal(t100, t[pick])
    for k in range(100):
        st, v1, t1 = dev.eval_natural_many(np.ascontiguousarray(y[pick[k]:pick[k] + 1]))
        assert st == 0 and bits(v1)[0] == bits(v[pick[k]:pick[k] + 1])[0] and t1[0] == t[pick[k]]


def test_sites_hull_edges_and_outside_targets(pkg, cloud2000):
    import torch
    from scipy.spatial import ConvexHull
    x, _, d, mesh, dev = cloud2000
    f = response(x)
    assert dev.set_response(f) == 0
    try:
        st, v, t = dev.eval_natural_many(x)                            # every site returns its datum, bit for bit
        assert st == 0 and (t >= 0).all() and np.array_equal(bits(v), bits(f))
        hv = ConvexHull(x).vertices
        a, b = hv, np.roll(hv, -1)
        s = np.random.default_rng(2).uniform(0.1, 0.9, len(hv))
        y = np.ascontiguousarray(x[a] + s[:, None] * (x[b] - x[a]))    # on hull edges, to rounding
        st, v, t = dev.eval_natural_many(y)
        on = t >= 0                                                     # rounding may put a point a hair outside
        print(f"{on.sum()} of {len(y)} hull-edge targets located")
        assert st in (0, pkg.GSL_EDOM) and on.sum() >= 0.75 * len(y) and np.isfinite(v[on]).all()
        want = f[a] + s * (f[b] - f[a])
        assert np.abs(v[on] - want[on]).max() <= 1e-9 * np.abs(f).max()
        y = np.ascontiguousarray(np.vstack([x[:5] * 0.5 + 0.25, [[50.0, 50.0], [-3.0, 0.5], [np.nan, 0.5], [0.5, np.nan]], x[5:8] * 0.5 + 0.25]))
        st, v, t = dev.eval_natural_many(y)
        assert st == pkg.GSL_EDOM and (t[5:9] == -1).all() and np.isnan(v[5:9]).all()
        assert (t[:5] >= 0).all() and (t[9:] >= 0).all() and np.isfinite(v[:5]).all() and np.isfinite(v[9:]).all()    # all others stored
        # the resident entry, without a triangle buffer
        ty = torch.from_numpy(y).cuda()
        tv = torch.empty(len(y), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        assert dev.eval_natural_resident(ty.data_ptr(), len(y), 2, tv.data_ptr(), None) == 0
        assert pkg.lib().gsl_sinterp_hip_sync(dev.ctx_handle()) == 0
        assert np.array_equal(bits(tv.cpu().numpy()), bits(v))
    finally:
        assert dev.set_response(2.0 * x[:, 0] - 3.0 * x[:, 1] + 0.5) == 0


def test_linear_path_on_the_same_mirror_is_unchanged(pkg, cloud2000):
    x, f, d, mesh, dev = cloud2000
    y = np.random.default_rng(3).random((6000, 2))
    fresh = mesh.device_alloc(0)                                       # a mirror that never evaluates natural neighbours
    assert fresh.set_response(f) == 0
    st0, v0, t0 = fresh.eval_many(y)
    st1, v1, t1 = dev.eval_many(y)
    dev.eval_natural_many(y)
    st2, v2, t2 = dev.eval_many(y)
    assert st0 == st1 == st2
    for v, t in ((v1, t1), (v2, t2)):
        assert np.array_equal(t, t0) and np.array_equal(bits(v[t0 >= 0]), bits(v0[t0 >= 0])) and np.isnan(v[t0 < 0]).all()


# ---------------------------------------------------------------------------------------------- the facade
def test_facade_types_checkpoint_and_statuses(pkg, orc, tmp_path):
    n = 500
    x = orc.synth_centres(n, 2) * [40.0, 0.25] + [5.0, -1.0]            # anisotropic: the tree standardises per axis
    f = response(x / [40.0, 0.25])
    y = np.ascontiguousarray(orc.synth_targets(0, 5000, 2) * [40.0, 0.25] + [5.0, -1.0])
    s = pkg.Sinterp("natural_simplex", 2, n, 0)
    assert s.set_tree_options(0, pkg.capi.Rng(0)) == 0 and s.init(x, f) == 0
    st, v, leaf = s.eval_many(y, want_leaf=True)
    tree = pkg.SimplexTree(2, n)
    assert tree.init(x, flags=0, rng=pkg.capi.Rng(0)) == 0
    mesh = pkg.SimplexMesh.from_tree(tree)
    assert mesh.delaunay_metric() == 2
    m = pkg.Sinterp("natural_mesh", 2, n, 0)
    assert m.set_triangulation(mesh.triangles(), mesh.neighbours()) == 0 and m.init(x, f) == 0
    stm, vm, leafm = m.eval_many(y, want_leaf=True)
    inside = leaf >= 0
    assert inside.sum() > 4000 and st == stm == (0 if inside.all() else pkg.GSL_EDOM)
    assert np.array_equal(leaf, leafm) and np.array_equal(bits(v[inside]), bits(vm[inside])) and np.isnan(v[~inside]).all()
    # ... and the mirror of that mesh gives the same again
    dev = mesh.device_alloc(0)
    assert dev.set_response(f) == 0
    _, vd, td = dev.eval_natural_many(y)
    assert np.array_equal(td, leaf) and np.array_equal(bits(vd[inside]), bits(v[inside]))
    # natural neighbours differ from the linear interpolant, and reproduce the data at the sites
    lin = pkg.Sinterp("linear_simplex", 2, n, 0)
    assert lin.set_tree_options(0, pkg.capi.Rng(0)) == 0 and lin.init(x, f) == 0
    _, vl, _ = lin.eval_many(y)
    assert np.abs(v[inside] - vl[inside]).max() > 1e-4
    sts, vs, _ = s.eval_many(x)
    assert sts == 0 and np.array_equal(bits(vs), bits(f))
    st1, one = s.eval_e(y[inside][0])
    assert st1 == 0 and bits(np.array([one]))[0] == bits(v[inside][:1])[0]
    lo, ext = x.min(axis=0), x.max(axis=0) - x.min(axis=0)
    stg, grid = s.eval_grid(lo + 0.3 * ext, lo + 0.7 * ext, 16, 16)
    assert stg == 0 and np.isfinite(grid).all()
    # the tree-built mesh near its hull: a linear function is reproduced on targets up to 0.1 % inside the hull
    from scipy.spatial import ConvexHull
    hull = x[ConvexHull(x).vertices]
    c = hull.mean(axis=0)
    rng = np.random.default_rng(11)
    k = rng.integers(0, len(hull), 2000)
    w = rng.random(2000)[:, None]
    edge = hull[k] + w * (hull[(k + 1) % len(hull)] - hull[k])
    depth = rng.choice([0.999, 0.99, 0.9], 2000)[:, None]
    yh = np.ascontiguousarray(c + depth * (edge - c))
    lin_f = 2.0 * x[:, 0] / 40.0 - 3.0 * x[:, 1] / 0.25 + 0.5
    sl = pkg.Sinterp("natural_simplex", 2, n, 0)
    assert sl.set_tree_options(0, pkg.capi.Rng(0)) == 0 and sl.init(x, lin_f) == 0
    sth, vh, th = sl.eval_many(yh, want_leaf=True)
    errh = np.abs(vh - (2.0 * yh[:, 0] / 40.0 - 3.0 * yh[:, 1] / 0.25 + 0.5)).max() / np.abs(lin_f).max()
    print(f"natural_simplex, 2000 targets 0.1 % .. 10 % inside the hull: max |s - f(y)| = {errh:.2e} max|f|")
    assert sth == 0 and (th >= 0).all() and errh <= 1e-12
    # checkpoints: new type ids, the mesh payload; the bits survive
    for kind, src in (("natural_simplex", s), ("natural_mesh", m)):
        path = tmp_path / (kind + ".bin")
        assert src.fwrite(path) == 0
        r = pkg.Sinterp(kind, 2, n, 0)
        assert r.fread(path) == 0
        str_, vr, leafr = r.eval_many(y, want_leaf=True)
        assert str_ == st and np.array_equal(leafr, leaf) and np.array_equal(bits(vr[inside]), bits(v[inside]))
        other = "natural_mesh" if kind == "natural_simplex" else "natural_simplex"
        assert pkg.Sinterp(other, 2, n, 0).fread(path) == pkg.capi.GSL_EBADLEN
        assert pkg.Sinterp("linear_mesh", 2, n, 0).fread(path) == pkg.capi.GSL_EBADLEN
    # what natural neighbours do not offer
    EUNSUP = pkg.capi.GSL_EUNSUP
    with pkg.capi.ErrorCalls():
        assert pkg.lib().gsl_sinterp_eval_grad_resident(s._p, None, 0, 2, None, None, 2) == EUNSUP
        assert pkg.lib().gsl_sinterp_eval_variance_resident(s._p, None, 0, 2, None) == EUNSUP
        assert s.set_neighbours(4) == EUNSUP
        g = pkg.Sinterp("natural_simplex", 2, n, 0)
        assert g.set_device_list([0, 0]) == 0 and g.init(x, f) == EUNSUP                       # no sharding
        # the device entries: a group, a non-convex mesh, a 3-D mesh, a non-Delaunay mesh
        grp = mesh.device_alloc_multi([0, 0])
        assert grp.set_response(f) == 0 and grp.eval_natural_many(y[:10])[0] == EUNSUP
        mesh.set_convex(0)
        nc = mesh.device_alloc(0)
        mesh.set_convex(1)
        assert nc.set_response(f) == 0 and nc.eval_natural_many(y[:10])[0] == EUNSUP
        from scipy.spatial import Delaunay
        x3 = np.random.default_rng(5).random((50, 3))
        d3 = pkg.SimplexMesh.from_arrays(x3, Delaunay(x3).simplices.astype(np.int32)).device_alloc(0)
        assert d3.set_response(x3[:, 0]) == 0 and d3.eval_natural_many(x3[:4])[0] == EUNSUP
        kite = np.array([[0.0, 0.0], [2.0, -1.5], [3.0, 0.0], [2.0, 1.5]])
        bad = pkg.SimplexMesh.from_arrays(kite, np.array([[0, 1, 3], [1, 2, 3]], dtype=np.int32))
        assert bad.delaunay_metric() == 0
        bd = bad.device_alloc(0)
        assert bd.set_response(np.zeros(4)) == 0 and bd.eval_natural_many(np.array([[1.5, 0.0]]))[0] == pkg.capi.GSL_EINVAL
