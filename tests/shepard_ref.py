"""numpy fp64 reference of the modified quadratic Shepard method (include/gsl_sinterp_hip.h, gsl_sinterp_hip_shepard_fit):
brute-force neighbour search, np.linalg.qr of the column-scaled weighted matrix with the library's rank rule, the analytic
gradient.  Two internal cross-checks (self_check) must hold before a test may use it: the coefficients against
np.linalg.lstsq, and the analytic gradient against Richardson differences of the reference's own values."""
import numpy as np

SQRT_EPS = 1.4901161193847656e-08          # GSL_SQRT_DBL_EPSILON
DEFAULTS = {2: (13, 19), 3: (17, 32)}      # Renka's nq, nw


def n_coef(dim):
    return dim + dim * (dim + 1) // 2


def monomials(u):
    """u [..., d] -> m(u) [..., nc]: the d linear monomials, then u_a u_b for a <= b in row-major order"""
    d = u.shape[-1]
    cols = [u[..., a] for a in range(d)]
    cols += [u[..., a] * u[..., b] for a in range(d) for b in range(a, d)]
    return np.stack(cols, axis=-1)


def d_monomials(u):
    """dm/du [..., nc, d]"""
    d = u.shape[-1]
    out = np.zeros(u.shape[:-1] + (n_coef(d), d))
    for a in range(d):
        out[..., a, a] = 1.0
    q = d
    for a in range(d):
        for b in range(a, d):
            out[..., q, a] += u[..., b]
            out[..., q, b] += u[..., a]
            q += 1
    return out


def _rho(diag):
    a = np.abs(diag)
    with np.errstate(invalid="ignore", divide="ignore"):
        return a.min(axis=-1) / a.max(axis=-1)


def fit(x, f, nq=0, nw=0, rows=None, chunk=1024, kdtree=None):
    """The model of nodes `rows` (default: all): dict with rq, rw [n], coef [n, nc], rho [n] = rho(nc), rho_lin [n], mode [n]
    (2 quadratic, 1 linear, 0 constant), cond [n] of the scaled matrix, coincident (bool); nodes outside `rows` hold NaN.
    The K + 8 candidate neighbours of a node come from a brute-force pass over all sites; kdtree = True (default for more than
    2048 sites, where the n x n pass takes seconds) takes them from scipy's cKDTree instead.  Either way the distances that
    enter the model are recomputed from the coordinate differences; the size test compares the two routes on a subset of rows."""
    x = np.asarray(x, dtype=np.float64)
    f = np.asarray(f, dtype=np.float64)
    n, d = x.shape
    nc = n_coef(d)
    nq = nq or DEFAULTS[d][0]
    nw = nw or DEFAULTS[d][1]
    K = max(nq, nw) + 1                                   # nearest OTHER sites needed
    KC = min(K + 8, n - 1)
    sq = (x * x).sum(axis=1)
    rows = np.arange(n) if rows is None else np.asarray(rows)
    tree = None
    if kdtree if kdtree is not None else n > 2048:
        from scipy.spatial import cKDTree
        tree = cKDTree(x)
    out = {"nq": nq, "nw": nw, "x": x, "f": f, "rq": np.full(n, np.nan), "rw": np.full(n, np.nan), "coef": np.full((n, nc), np.nan),
           "rho": np.full(n, np.nan), "rho_lin": np.full(n, np.nan), "mode": np.full(n, -1), "cond": np.full(n, np.nan),
           "coincident": False, "A": {}, "b": {}}
    for c0 in range(0, len(rows), chunk):
        ii = rows[c0:c0 + chunk]
        # candidates by |a|^2 + |b|^2 - 2 a.b (one matrix product; its rounding can only reorder near-ties, hence the
        # margin of 8), then the distances of the candidates from the coordinate differences themselves
        if tree is None:
            approx = sq[ii][:, None] + sq[None, :] - 2.0 * (x[ii] @ x.T)
            approx[np.arange(len(ii)), ii] = np.inf        # the node itself
            cand = np.argpartition(approx, KC - 1, axis=1)[:, :KC]
        else:
            cand = tree.query(x[ii], KC + 1)[1]
            keep = np.argsort(cand == ii[:, None], axis=1, kind="stable")      # the node itself to the end
            cand = np.take_along_axis(cand, keep, axis=1)[:, :KC]
        diff = x[cand] - x[ii][:, None, :]
        r2 = (diff * diff).sum(axis=2)
        near = np.take_along_axis(cand, np.argpartition(r2, K - 1, axis=1)[:, :K], axis=1)
        rn = np.sqrt(((x[near] - x[ii][:, None, :]) ** 2).sum(axis=2))
        order = np.argsort(rn, axis=1, kind="stable")
        near = np.take_along_axis(near, order, axis=1)
        rn = np.take_along_axis(rn, order, axis=1)
        if (rn[:, 0] == 0.0).any():
            out["coincident"] = True
            return out
        rq, rw = rn[:, nq], rn[:, nw]                      # the (nq + 1)-th / (nw + 1)-th nearest other site
        w = np.where(rn < rq[:, None], (rq[:, None] - rn) / (rq[:, None] * rn), 0.0)
        u = (x[near] - x[ii][:, None, :]) / rq[:, None, None]
        A = w[:, :, None] * monomials(u)
        b = w * (f[near] - f[ii][:, None])
        nrm = np.sqrt((A * A).sum(axis=1))
        As = A / np.where(nrm > 0.0, nrm, 1.0)[:, None, :]
        Q, R = np.linalg.qr(As)
        diag = np.diagonal(R, axis1=1, axis2=2)
        rho, rho_lin = _rho(diag), _rho(diag[:, :d])
        mode = np.where(rho >= SQRT_EPS, 2, np.where(rho_lin >= SQRT_EPS, 1, 0))
        qtb = np.einsum("nkc,nk->nc", Q, b)
        coef = np.zeros((len(ii), nc))
        for t in range(len(ii)):
            k = nc if mode[t] == 2 else (d if mode[t] == 1 else 0)
            if k:
                coef[t, :k] = np.linalg.solve(R[t, :k, :k], qtb[t, :k]) / nrm[t, :k]
        out["rq"][ii], out["rw"][ii], out["coef"][ii] = rq, rw, coef
        out["rho"][ii], out["rho_lin"][ii], out["mode"][ii] = rho, rho_lin, mode
        with np.errstate(invalid="ignore", divide="ignore"):
            sv = np.linalg.svd(As, compute_uv=False)
            out["cond"][ii] = sv[:, 0] / sv[:, -1]
        if len(rows) <= 2048:                               # kept for the lstsq cross-check of small clouds
            for t, i in enumerate(ii):
                out["A"][int(i)], out["b"][int(i)] = A[t], b[t]
    return out


def evaluate(model, y, chunk=128):
    """(s [m], g [m, d], leaf [m]) by brute force over every node; NaN / -1 where no node covers the target or a
    coordinate is NaN; at r2 = 0 the smallest such row's value, its nodal gradient and leaf 1"""
    x, f, rq, rw, coef = model["x"], model["f"], model["rq"], model["rw"], model["coef"]
    y = np.asarray(y, dtype=np.float64)
    m, d = y.shape
    s, g, leaf = np.full(m, np.nan), np.full((m, d), np.nan), np.full(m, -1)
    known = np.isfinite(rw)                                # a partial model: the other nodes must not be in reach
    for c0 in range(0, m, chunk):
        yy = y[c0:c0 + chunk]
        diff = yy[:, None, :] - x[None, :, :]
        r2 = (diff * diff).sum(axis=2)
        r = np.sqrt(r2)
        for t in range(len(yy)):
            if not np.isfinite(yy[t]).all():
                continue
            hit = np.flatnonzero(r2[t] == 0.0)
            if len(hit):
                i = hit[0]
                s[c0 + t], g[c0 + t], leaf[c0 + t] = f[i], coef[i, :d] / rq[i], 1
                continue
            sel = np.flatnonzero(known & (r[t] < rw))
            if not len(sel):
                continue
            rr, dd = r[t, sel], diff[t, sel]
            wv = (rw[sel] - rr) / (rw[sel] * rr)
            W = wv * wv
            sel, rr, dd, wv, W = sel[W > 0], rr[W > 0], dd[W > 0], wv[W > 0], W[W > 0]
            if not len(sel):
                continue
            u = dd / rq[sel, None]
            Q = f[sel] + (coef[sel] * monomials(u)).sum(axis=1)
            gQ = np.einsum("nc,ncd->nd", coef[sel], d_monomials(u)) / rq[sel, None]
            gW = (-2.0 * wv / (rr * rr * rr))[:, None] * dd      # w = 1/r - 1/Rw, grad w = -(y - x) / r^3
            sw = W.sum()
            sv = (W * Q).sum() / sw
            s[c0 + t] = sv
            g[c0 + t] = (W[:, None] * gQ + (Q - sv)[:, None] * gW).sum(axis=0) / sw
            leaf[c0 + t] = len(sel)
    return s, g, leaf


def self_check(model, y):
    """the two cross-checks; raises AssertionError when the reference disagrees with itself"""
    d = model["x"].shape[1]
    # 1. QR coefficients against lstsq of the same weighted system (full-rank nodes)
    worst = 0.0
    for i, A in model["A"].items():
        if model["mode"][i] != 2:
            continue
        nrm = np.sqrt((A * A).sum(axis=0))
        c = np.linalg.lstsq(A / nrm, model["b"][i], rcond=None)[0] / nrm
        worst = max(worst, np.abs(c - model["coef"][i]).max() / max(1.0, np.abs(c).max()))
    assert worst <= 1e-11, f"reference: lstsq and QR coefficients differ by {worst:g}"
    # 2. analytic gradient against Richardson differences of the reference's own values
    yy = np.asarray(y, dtype=np.float64)[:40]
    s0, g0, leaf0 = evaluate(model, yy)
    ok = leaf0 > 1
    yy, g0 = yy[ok], g0[ok]
    h = 1e-4
    num = np.zeros_like(g0)
    for a in range(d):
        e = np.zeros(d)
        e[a] = h
        d1 = (evaluate(model, yy + e)[0] - evaluate(model, yy - e)[0]) / (2 * h)
        d2 = (evaluate(model, yy + e / 2)[0] - evaluate(model, yy - e / 2)[0]) / h
        num[:, a] = (4.0 * d2 - d1) / 3.0
    defect = np.nanmax(np.abs(num - g0)) / np.abs(g0).max()
    assert defect <= 1e-6, f"reference: analytic gradient and Richardson differences differ by {defect:g}"
    return worst, defect
