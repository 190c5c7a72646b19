"""-m gpu: the sorted-target routes of the located sweeps on ONE context whose batch size keeps changing.

The sort buffer and the walk buffer of a context are grow-only and laid out per batch; the routes switch at m = 4096
(unsorted -> one-level reorder, exact kernel -> certified walks) and at m = 2^18 (one-level -> two-level reorder).  The
sequence below visits each switch-over size and its predecessor, large before small and back, with and without a leaf
output.  DAG path: bit for bit against the CPU oracle.  Imported meshes (2-D, 3-D): bit for bit against the same batch
on a fresh context -- a mesh result is a function of (mesh, target) only."""
import ctypes
import os

import numpy as np
import pytest
import torch

from gpu_util import bits, dev, ptr
from test_gpu_bary import build_pair
from test_gpu_mesh3 import scene, smooth

pytestmark = pytest.mark.gpu

SIZES = [262_144, 4096, 100, 262_143, 4095, 262_144]
M = max(SIZES)
N = 3000                                                   # ~27 000 nodes >= 2048: leaf-walk data and jump table exist

_tree = {}


def tree_scene(pkg, orc):
    """the tree of N synthetic centres, its oracle twin, the targets and the oracle's answers on the checked subset"""
    if not _tree:
        x = orc.synth_centres(N, 2)
        f = orc.synth_response(x)
        t, o = build_pair(pkg, orc, x)
        assert t.n_nodes >= 2048
        y = orc.synth_targets(0, M, 2) * 1.1 - 0.05          # a few outside the hull, in the cage leaves
        idx = np.unique(np.concatenate([checked(m) for m in SIZES]))
        ov, ol = o.eval_many(x, f, np.ascontiguousarray(y[idx]))
        _tree.update(x=x, f=f, t=t, y=y, idx=idx, ov=ov, ol=ol)
    return _tree


def checked(m):
    """stride-41 subset plus the last 3000 targets of a batch of m"""
    return np.unique(np.concatenate([np.arange(0, m, 41), np.arange(max(0, m - 3000), m)]))


class Out:
    """device outputs, refilled with a sentinel before every call so that a stale result cannot pass"""

    def __init__(self):
        self.v = torch.empty(M, dtype=torch.float64, device="cuda")
        self.l = torch.empty(M, dtype=torch.int32, device="cuda")

    def reset(self):
        self.v.fill_(-7.0)
        self.l.fill_(-7)
        torch.cuda.synchronize()

    def get(self, m, sync):
        sync()
        torch.cuda.synchronize()
        return self.v[:m].cpu().numpy(), self.l[:m].cpu().numpy()


def check_against_oracle(s, m, v, l):
    sel = checked(m)
    pos = np.searchsorted(s["idx"], sel)
    ov, ol = s["ov"][pos], s["ol"][pos]
    ok = ol >= 0
    assert ok.sum() > 0.5 * len(sel)
    if l is not None:
        assert np.array_equal(l[sel], ol)
    assert np.array_equal(bits(v[sel][ok]), bits(ov[ok]))


def last_route(pkg, ctx_handle):
    q, lw = ctypes.c_uint(0), ctypes.c_int(0)
    assert pkg.lib().gsl_sinterp_hip_bary_last_queue(ctx_handle, ctypes.byref(q), ctypes.byref(lw)) == 0
    return lw.value


def test_dag_batches_of_changing_size_on_the_packing_context(pkg, orc):
    """records packed by tree_pack on this context: pack-time jump table, certified leaf walk from 4096 targets"""
    s = tree_scene(pkg, orc)
    d = s["t"].device_alloc(0)
    assert d.set_response(s["f"]) == 0
    ctx = pkg.lib().simplex_tree_device_ctx(d._h)
    plain = not any(os.environ.get(k) == "1" for k in ("GSL_SINTERP_NO_SORT", "GSL_SINTERP_NO_LEAFWALK", "GSL_SINTERP_NO_FASTDIV"))
    d_y, out = dev(s["y"]), Out()
    for m in SIZES:
        for want_leaf in (True, False):
            out.reset()
            assert d.eval_resident(ptr(d_y), m, 2, ptr(out.v), ptr(out.l) if want_leaf else None) == 0
            v, l = out.get(m, lambda: pkg.lib().gsl_sinterp_hip_sync(ctx))
            assert last_route(pkg, ctx) == (1 if plain and m >= 4096 else 0), m
            check_against_oracle(s, m, v, l if want_leaf else None)
            assert want_leaf or (l == -7).all()


def test_dag_batches_of_changing_size_on_a_foreign_context(pkg, orc):
    """records packed on ANOTHER context (the broadcast situation), through the raw entry: per-batch jump table and the
    certified DAG walk from 4096 targets, never the leaf walk"""
    s = tree_scene(pkg, orc)
    t = s["t"]
    types, pidx, links = t.arrays()
    sh = t.shuffle()
    nn = t.n_nodes
    ctx_pack, ctx_eval = pkg.HipContext.on_torch_stream(0), pkg.HipContext.on_torch_stream(0)
    d_type, d_pidx, d_links = dev(types), dev(pidx), dev(links)
    d_pts, d_resp = dev(s["x"][sh]), dev(s["f"][sh])
    rec = torch.empty(nn * 64, dtype=torch.uint8, device="cuda")
    tab = torch.empty(nn * 32, dtype=torch.uint8, device="cuda")
    geom = t.geom()
    ctx_pack.tree_pack(nn, ptr(d_type), ptr(d_pidx), ptr(d_links), N, ptr(d_pts), geom, ptr(rec))
    ctx_pack.tree_bind(nn, ptr(d_pidx), N, ptr(d_resp), ptr(tab))
    ctx_pack.sync()
    d_y, out = dev(s["y"]), Out()
    for m in SIZES:
        for want_leaf in (True, False):
            out.reset()
            ctx_eval.bary_eval(nn, ptr(rec), ptr(tab), geom[8:10], ptr(d_y), m, 2, ptr(out.v), ptr(out.l) if want_leaf else None)
            v, l = out.get(m, ctx_eval.sync)
            assert last_route(pkg, ctx_eval.handle) == 0, m
            check_against_oracle(s, m, v, l if want_leaf else None)
            assert want_leaf or (l == -7).all()


def mesh_sequence(pkg, mesh, f, y, shared):
    """every batch of SIZES on the shared mirror == the same batch on a fresh mirror (a context of its own)"""
    dim = y.shape[1]
    d_y, out = dev(y), Out()
    fresh = {}
    for m in sorted(set(SIZES)):
        one = mesh.device_alloc(0)
        assert one.set_response(f) == 0
        out.reset()
        assert one.eval_resident(ptr(d_y), m, dim, ptr(out.v), ptr(out.l)) == 0
        fresh[m] = out.get(m, lambda: pkg.lib().gsl_sinterp_hip_sync(one.ctx_handle()))
        assert (fresh[m][1] >= 0).sum() > 0.5 * m and (fresh[m][1] >= -1).all()
        one.close()
    for m in SIZES:
        for want_leaf in (True, False):
            out.reset()
            assert shared.eval_resident(ptr(d_y), m, dim, ptr(out.v), ptr(out.l) if want_leaf else None) == 0
            v, l = out.get(m, lambda: pkg.lib().gsl_sinterp_hip_sync(shared.ctx_handle()))
            assert np.array_equal(bits(v), bits(fresh[m][0])), (m, want_leaf)
            assert np.array_equal(l, fresh[m][1]) if want_leaf else (l == -7).all(), (m, want_leaf)


def test_exported_2d_mesh_batches_of_changing_size(pkg, orc):
    s = tree_scene(pkg, orc)
    mesh = pkg.SimplexMesh.from_tree(s["t"])
    shared = mesh.device_alloc(0)
    assert shared.set_response(s["f"]) == 0
    mesh_sequence(pkg, mesh, s["f"], s["y"], shared)


def test_3d_mesh_batches_of_changing_size(pkg, orc):
    x, d, tet, nbr, mesh, shared = scene(pkg, 400)
    f = smooth(orc, mesh, x)
    assert shared.set_response(f) == 0
    lo, hi = mesh.bbox()
    y = np.ascontiguousarray(lo + np.random.default_rng(29).random((M, 3)) * (hi - lo))
    mesh_sequence(pkg, mesh, f, y, shared)
