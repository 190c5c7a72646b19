"""Extended-precision references for the smallest models (tests/test_tiny_ref.py, tests/test_gpu_tiny_models.py).

Plain mpmath at 50 digits: no GPU, no project code, no identity that the device code also uses.  Every system is the
textbook one, solved through the explicit inverse of a matrix of at most two dozen rows:

    RBF            Phi w = f                                        s(y) = sum_j w_j phi(|y - x_j|)
    affine TPS     [Phi P; P^T 0] [w; c] = [f; 0],  P = [1, x]      s(y) = ... + c_0 + sum_a c_a y_a     (raw coordinates)
    kriging        [K P; P^T 0] [w; c] = [f; 0],    K = Phi + nugget I,  P = the drift basis of ukrige_ref.basis in the
                   standardised coordinates of ukrige_ref.geometry (order 0: P = 1, c = the mean)
                   sigma^2(y) = phi(0) - k^T lambda - p^T mu,  [K P; P^T 0] [lambda; mu] = [k; p]
    leave-one-out  by deletion: N refits without one site each
    scores         as tests/test_gpu_fit.py::scores defines them, with the leave-one-out residuals by deletion

Kernels (eps = the shape parameter, t as given):
    Gaussian      exp(-(eps r)^2)                                       phi'/r = -2 eps^2 phi
    thin plate    r^2 ln r, 0 at r = 0 (no shape parameter)             phi'/r = 2 ln r + 1   (the term vanishes at r = 0)
    Wendland C2   (1 - t)_+^4 (4 t + 1),            t = eps r           phi'/r = -20 eps^2 (1 - t)_+^3
    Matern 3/2    (1 + t) exp(-t),                  t = sqrt(3) eps r   phi'/r = -3 eps^2 exp(-t)
    Matern 5/2    (1 + t + t^2 / 3) exp(-t),        t = sqrt(5) eps r   phi'/r = -(5 eps^2 / 3) (1 + t) exp(-t)
    inv. multiq.  1 / sqrt(1 + (eps r)^2)                               phi'/r = -eps^2 phi^3

Arrays come in and go out as numpy fp64 (inputs are taken exactly, outputs are the 50-digit results rounded once)."""
import mpmath as mp
import numpy as np

import ukrige_ref

mp.mp.dps = 50
GAUSSIAN, TPS, WENDLAND, MATERN32, MATERN52, IMQ = 0, 1, 2, 3, 4, 5
# facade type -> (kind, kriging, affine tail)
TYPES = {"gaussian": (GAUSSIAN, False, False), "tps": (TPS, False, False), "tps_affine": (TPS, False, True),
         "wendland": (WENDLAND, False, False), "matern32": (MATERN32, False, False), "matern52": (MATERN52, False, False),
         "imq": (IMQ, False, False), "kriging": (GAUSSIAN, True, False), "kriging_matern32": (MATERN32, True, False),
         "kriging_matern52": (MATERN52, True, False)}


def default_eps(kind, n, dim):
    """the types' default shape (orc.gaussian_eps, ukrige_ref.default_eps, test_gpu_fit.default_eps away from 1-D)"""
    return (0.125 if kind == WENDLAND else 2.0 if kind == GAUSSIAN else 1.0) * n ** (1.0 / dim)


# ------------------------------------------------------------------------------------------------- kernels
def phi(kind, eps, r):
    r, eps = mp.mpf(r), mp.mpf(eps)
    if kind == GAUSSIAN:
        return mp.exp(-(eps * r) ** 2)
    if kind == TPS:
        return r * r * mp.log(r) if r > 0 else mp.mpf(0)
    if kind == WENDLAND:
        t = eps * r
        return (1 - t) ** 4 * (4 * t + 1) if t < 1 else mp.mpf(0)
    if kind == MATERN32:
        t = mp.sqrt(3) * eps * r
        return (1 + t) * mp.exp(-t)
    if kind == MATERN52:
        t = mp.sqrt(5) * eps * r
        return (1 + t + t * t / 3) * mp.exp(-t)
    assert kind == IMQ
    return 1 / mp.sqrt(1 + (eps * r) ** 2)


def psi(kind, eps, r):
    """phi'(r) / r, so that grad_y phi(|y - x|) = psi (y - x); thin plate at r = 0: 0 (the product with y - x = 0 is)"""
    r, eps = mp.mpf(r), mp.mpf(eps)
    if kind == GAUSSIAN:
        return -2 * eps * eps * mp.exp(-(eps * r) ** 2)
    if kind == TPS:
        return 2 * mp.log(r) + 1 if r > 0 else mp.mpf(0)
    if kind == WENDLAND:
        t = eps * r
        return -20 * eps * eps * (1 - t) ** 3 if t < 1 else mp.mpf(0)
    if kind == MATERN32:
        return -3 * eps * eps * mp.exp(-mp.sqrt(3) * eps * r)
    if kind == MATERN52:
        t = mp.sqrt(5) * eps * r
        return -(5 * eps * eps / 3) * (1 + t) * mp.exp(-t)
    assert kind == IMQ
    return -eps * eps * phi(IMQ, eps, r) ** 3


# ------------------------------------------------------------------------------------------------- plumbing
def _mat(a):
    """numpy (1-D or 2-D) -> mp.matrix with the exact fp64 values"""
    a = np.asarray(a, dtype=np.float64)
    a = a.reshape(len(a), -1)
    return mp.matrix([[mp.mpf(float(v)) for v in row] for row in a])


def _np(M):
    return np.array([[float(M[i, j]) for j in range(M.cols)] for i in range(M.rows)], dtype=np.float64).reshape(M.rows, M.cols)


def _dist(a, i, b, j):
    return mp.sqrt(mp.fsum((a[i, c] - b[j, c]) ** 2 for c in range(a.cols)))


def kernel_matrix(kind, eps, a, b):
    """phi(|a_i - b_j|), rows of a x rows of b (mp.matrix in, mp.matrix out)"""
    return mp.matrix([[phi(kind, eps, _dist(a, i, b, j)) for j in range(b.rows)] for i in range(a.rows)])


def _stack(K, P):
    """[K P; P^T 0]"""
    n, q = K.rows, P.cols
    A = mp.zeros(n + q, n + q)
    for i in range(n):
        for j in range(n):
            A[i, j] = K[i, j]
        for a in range(q):
            A[i, n + a] = A[n + a, i] = P[i, a]
    return A


def _rows(M, lo, hi):
    return mp.matrix([[M[i, j] for j in range(M.cols)] for i in range(lo, hi)])


def _basis(y, shift, scale, order):
    """ukrige_ref.basis in extended precision: (P rows x q, dP rows x q x dim) as nested lists; order 0: the constant"""
    shift, scale = [mp.mpf(float(v)) for v in shift], [mp.mpf(float(v)) for v in scale]
    d = y.cols
    P, D = [], []
    for i in range(y.rows):
        u = [(y[i, a] - shift[a]) * scale[a] for a in range(d)]
        row, grad = [mp.mpf(1)], [[mp.mpf(0)] * d]
        if order >= 1:
            for a in range(d):
                row.append(u[a])
                grad.append([scale[a] if c == a else mp.mpf(0) for c in range(d)])
        if order == 2:
            for a in range(d):
                for b in range(a, d):
                    row.append(u[a] * u[b])
                    g = [mp.mpf(0)] * d
                    g[a] += u[b] * scale[a]
                    g[b] += u[a] * scale[b]
                    grad.append(g)
        P.append(row)
        D.append(grad)
    return mp.matrix(P), D


def _raw_affine(y):
    """P = [1, y] and its gradient in raw coordinates (the affine thin-plate tail)"""
    d = y.cols
    P = mp.matrix([[mp.mpf(1)] + [y[i, a] for a in range(d)] for i in range(y.rows)])
    D = [[[mp.mpf(0)] * d] + [[mp.mpf(1) if c == a else mp.mpf(0) for c in range(d)] for a in range(d)] for _ in range(y.rows)]
    return P, D


class Model:
    """One fitted model of K fields.  kind: the kernel; tail: None (plain RBF), "affine" (thin-plate spline with [1, x] in
    raw coordinates) or a drift order 0 / 1 / 2 (kriging; 0 = ordinary).  w (n x K) and c (q x K) are numpy fp64."""

    def __init__(self, kind, eps, x, F, tail=None, nugget=0.0, geometry=None):
        self.kind, self.eps, self.tail = kind, eps, tail
        self.x = _mat(x)
        self.F = _mat(F)
        n = self.n = self.x.rows
        self.Phi = kernel_matrix(kind, eps, self.x, self.x)
        self.K = self.Phi.copy()
        for i in range(n):
            self.K[i, i] += mp.mpf(float(nugget))
        self.nugget = mp.mpf(float(nugget))
        if tail is None:
            self.P, self.q = None, 0
            self.A = self.K
        else:
            if tail == "affine":
                self.P, _ = _raw_affine(self.x)
            else:
                self.shift, self.scale = geometry if geometry is not None else ukrige_ref.geometry(np.asarray(x, dtype=np.float64))
                self.P, _ = _basis(self.x, self.shift, self.scale, tail)
            self.q = self.P.cols
            self.A = _stack(self.K, self.P)
        self.Ainv = mp.inverse(self.A)
        rhs = mp.zeros(n + self.q, self.F.cols)
        for i in range(n):
            for k in range(self.F.cols):
                rhs[i, k] = self.F[i, k]
        sol = self.Ainv * rhs
        self.W, self.C = _rows(sol, 0, n), (_rows(sol, n, n + self.q) if self.q else None)
        self.w, self.c = _np(self.W), (_np(self.C) if self.q else None)

    def _tail(self, Y):
        if self.tail == "affine":
            return _raw_affine(Y)
        return _basis(Y, self.shift, self.scale, self.tail)

    def values(self, y):
        """m x K"""
        Y = _mat(y)
        S = kernel_matrix(self.kind, self.eps, Y, self.x) * self.W
        if self.q:
            S += self._tail(Y)[0] * self.C
        return _np(S)

    def gradient(self, y, fields=(0,)):
        """m x len(fields) x dim"""
        Y = _mat(y)
        m, d = Y.rows, Y.cols
        D = self._tail(Y)[1] if self.q else None
        out = np.zeros((m, len(fields), d))
        for i in range(m):
            ps = [psi(self.kind, self.eps, _dist(Y, i, self.x, j)) for j in range(self.n)]
            for slot, k in enumerate(fields):
                for c in range(d):
                    g = mp.fsum(ps[j] * self.W[j, k] * (Y[i, c] - self.x[j, c]) for j in range(self.n))
                    if self.q:
                        g += mp.fsum(D[i][a][c] * self.C[a, k] for a in range(self.q))
                    out[i, slot, c] = float(g)
        return out

    def variance(self, y):
        """kriging variance at the rows of y (the bordered system; the plain positive definite RBF gives the power function)"""
        Y = _mat(y)
        m = Y.rows
        kv = kernel_matrix(self.kind, self.eps, Y, self.x)               # m x n
        p = self._tail(Y)[0] if self.q else None
        rhs = mp.zeros(self.n + self.q, m)
        for i in range(m):
            for j in range(self.n):
                rhs[j, i] = kv[i, j]
            for a in range(self.q):
                rhs[self.n + a, i] = p[i, a]
        lam = self.Ainv * rhs
        return np.array([float(phi(self.kind, self.eps, 0) - mp.fsum(rhs[j, i] * lam[j, i] for j in range(self.n + self.q)))
                         for i in range(m)])


def fit(typ, dim, x, F, eps=None, nugget=0.0, drift=0):
    """the model of a facade type at its default shape"""
    kind, krige, affine = TYPES[typ]
    x = np.asarray(x, dtype=np.float64).reshape(-1, dim)
    eps = default_eps(kind, len(x), dim) if eps is None else eps
    return Model(kind, eps, x, F, tail=(drift if krige else "affine" if affine else None), nugget=nugget if krige else 0.0)


def loo_by_deletion(typ, dim, x, F, eps=None, nugget=0.0, drift=0):
    """(E n x K, v n): refit without site i, predict at x_i; v_i = the variance of the prediction error of the observation
    f_i (sigma^2 of the model without i at x_i, plus the nugget).  The shape and the drift's standardisation stay those of
    the full cloud.  Kriging needs n - 1 >= the number of drift terms (1 without a drift)."""
    kind, krige, affine = TYPES[typ]
    assert not affine and kind != TPS
    x = np.asarray(x, dtype=np.float64).reshape(-1, dim)
    F = np.asarray(F, dtype=np.float64).reshape(len(x), -1)
    n = len(x)
    eps = default_eps(kind, n, dim) if eps is None else eps
    geometry = ukrige_ref.geometry(x)
    if n == 1 and not krige:                                # nothing is left: the empty model predicts 0 with variance phi(0)
        return F.copy(), np.ones(1)
    E, v = np.zeros(F.shape), np.zeros(n)
    for i in range(n):
        keep = np.arange(n) != i
        m = Model(kind, eps, x[keep], F[keep], tail=(drift if krige else None), nugget=nugget if krige else 0.0, geometry=geometry)
        E[i] = F[i] - m.values(x[i:i + 1])[0]
        v[i] = m.variance(x[i:i + 1])[0] + (nugget if krige else 0.0)
    return E, v


def scores(typ, dim, x, f, eps, nugget=0.0):
    """(ML, LOO) of tests/test_gpu_fit.py::scores: ML = (n ln(2 pi s2) + ln det K + n) / 2 with s2 = f.w / n and w the model's
    weights; LOO = the mean squared leave-one-out residual, here by deletion"""
    kind, krige, _ = TYPES[typ]
    x = np.asarray(x, dtype=np.float64).reshape(-1, dim)
    n = len(x)
    m = Model(kind, eps, x, f, tail=(0 if krige else None), nugget=nugget if krige else 0.0)
    s2 = mp.fsum(m.F[i, 0] * m.W[i, 0] for i in range(n)) / n
    ml = (n * mp.log(2 * mp.pi * s2) + mp.log(mp.det(m.K)) + n) / 2
    E, _ = loo_by_deletion(typ, dim, x, f, eps=eps, nugget=nugget)
    return float(ml), float(np.mean(E[:, 0] ** 2))


# ------------------------------------------------------------------------------------------------- one and two simplices
def barycentric(verts, y):
    """the barycentric coordinates (dim + 1) of y in the simplex with the given vertex rows, in extended precision"""
    V, d = _mat(verts), len(y)
    A = mp.matrix(d + 1, d + 1)
    for j in range(d + 1):
        A[0, j] = 1
        for c in range(d):
            A[1 + c, j] = V[j, c]
    b = mp.matrix([mp.mpf(1)] + [mp.mpf(float(v)) for v in y])
    return mp.lu_solve(A, b)


def simplex_linear(x, F, simplices, y):
    """(values m x K, gradients m x K x dim, simplex m, margin m) of the piecewise-linear interpolant on the listed simplices.
    A target belongs to the simplex in which its smallest barycentric coordinate is largest (the first such); margin is
    that coordinate: > 0 strictly inside a simplex, ~ 0 on the skeleton, < 0 outside the mesh, where the values are NaN and
    the simplex is -1.  NaN targets: NaN, -1, margin NaN."""
    x = np.asarray(x, dtype=np.float64)
    F = np.asarray(F, dtype=np.float64).reshape(len(x), -1)
    m, d, nf = len(y), x.shape[1], F.shape[1]
    S, G, T = np.full((m, nf), np.nan), np.full((m, nf, d), np.nan), np.full(m, -1, dtype=np.int64)
    margin = np.full(m, np.nan)
    grads = []
    for t in simplices:
        A = mp.matrix(d + 1, d + 1)
        for j in range(d + 1):
            A[j, 0] = 1
            for c in range(d):
                A[j, 1 + c] = mp.mpf(float(x[t[j], c]))
        grads.append(mp.inverse(A) * _mat(F[list(t)]))                   # row 0: constant, rows 1..d: the gradient
    for i in range(m):
        if np.isnan(y[i]).any():
            continue
        best = None
        for ti, t in enumerate(simplices):
            lam = barycentric(x[list(t)], y[i])
            if best is None or min(lam) > best[0]:
                best = (min(lam), ti, lam)
        margin[i] = float(best[0])
        if best[0] >= 0:
            ti, lam = best[1], best[2]
            t = simplices[ti]
            for k in range(nf):
                S[i, k] = float(mp.fsum(lam[j] * mp.mpf(float(F[t[j], k])) for j in range(d + 1)))
                for c in range(d):
                    G[i, k, c] = float(grads[ti][1 + c, k])
            T[i] = ti
    return S, G, T, margin


# ------------------------------------------------------------------------------------------------- fp64 twins (numpy)
def np_phi(kind, eps, r):
    with np.errstate(divide="ignore", invalid="ignore"):
        if kind == GAUSSIAN:
            return np.exp(-(eps * r) ** 2)
        if kind == TPS:
            return np.where(r > 0.0, r * r * np.log(np.where(r > 0.0, r, 1.0)), 0.0)
        if kind == WENDLAND:
            t = eps * r
            return np.where(t < 1.0, (1.0 - t) ** 4 * (4.0 * t + 1.0), 0.0)
        if kind == MATERN32:
            t = np.sqrt(3.0) * eps * r
            return (1.0 + t) * np.exp(-t)
        if kind == MATERN52:
            t = np.sqrt(5.0) * eps * r
            return (1.0 + t + t * t / 3.0) * np.exp(-t)
        assert kind == IMQ
        return 1.0 / np.sqrt(1.0 + (eps * r) ** 2)


def np_basis(y, tail, geometry):
    """the columns of the tail at the rows of y: [1, y] raw (affine), or ukrige_ref.basis cut to the order (0: the constant)"""
    if tail == "affine":
        return np.column_stack([np.ones(len(y)), y])
    if tail == 0:
        return np.ones((len(y), 1))
    return ukrige_ref.basis(y, geometry[0], geometry[1], tail)[0]


def system_matrix(typ, dim, x, eps=None, nugget=0.0, drift=0):
    """the fp64 matrix the model of a facade type solves with: Phi, or the bordered [K P; P^T 0]"""
    kind, krige, affine = TYPES[typ]
    n = len(x)
    eps = default_eps(kind, n, dim) if eps is None else eps
    K = np_phi(kind, eps, ukrige_ref.dist(x, x)) + (nugget if krige else 0.0) * np.eye(n)
    tail = drift if krige else "affine" if affine else None
    if tail is None:
        return K
    P = np_basis(x, tail, ukrige_ref.geometry(x))
    return np.block([[K, P], [P.T, np.zeros((P.shape[1], P.shape[1]))]])


class NpModel:
    """Model in numpy fp64, for the sizes past extended precision's reach (31 .. 129); same fields, same methods"""

    def __init__(self, kind, eps, x, F, tail=None, nugget=0.0, geometry=None):
        self.kind, self.eps, self.tail, self.x = kind, eps, tail, x
        F = np.asarray(F, dtype=np.float64).reshape(len(x), -1)
        n = self.n = len(x)
        self.geometry = geometry if geometry is not None else ukrige_ref.geometry(x)
        K = np_phi(kind, eps, ukrige_ref.dist(x, x)) + nugget * np.eye(n)
        if tail is None:
            self.q, self.A = 0, K
        else:
            P = np_basis(x, tail, self.geometry)
            self.q = P.shape[1]
            self.A = np.block([[K, P], [P.T, np.zeros((self.q, self.q))]])
        sol = np.linalg.solve(self.A, np.vstack([F, np.zeros((self.q, F.shape[1]))]))
        self.w, self.c = sol[:n], (sol[n:] if self.q else None)

    def values(self, y):
        s = np_phi(self.kind, self.eps, ukrige_ref.dist(y, self.x)) @ self.w
        return s + np_basis(y, self.tail, self.geometry) @ self.c if self.q else s

    def variance(self, y):
        k = np_phi(self.kind, self.eps, ukrige_ref.dist(y, self.x)).T
        rhs = np.vstack([k, np_basis(y, self.tail, self.geometry).T]) if self.q else k
        return 1.0 - (rhs * np.linalg.solve(self.A, rhs)).sum(axis=0)


def np_fit(typ, dim, x, F, eps=None, nugget=0.0, drift=0):
    kind, krige, affine = TYPES[typ]
    eps = default_eps(kind, len(x), dim) if eps is None else eps
    return NpModel(kind, eps, x, F, tail=(drift if krige else "affine" if affine else None), nugget=nugget if krige else 0.0)


def np_loo_by_deletion(typ, dim, x, F, eps=None, nugget=0.0, drift=0):
    """loo_by_deletion in fp64"""
    kind, krige, _ = TYPES[typ]
    F = np.asarray(F, dtype=np.float64).reshape(len(x), -1)
    n = len(x)
    eps = default_eps(kind, n, dim) if eps is None else eps
    geometry = ukrige_ref.geometry(x)
    E, v = np.zeros(F.shape), np.zeros(n)
    for i in range(n):
        keep = np.arange(n) != i
        m = NpModel(kind, eps, x[keep], F[keep], tail=(drift if krige else None), nugget=nugget if krige else 0.0, geometry=geometry)
        E[i] = F[i] - m.values(x[i:i + 1])[0]
        v[i] = m.variance(x[i:i + 1])[0] + (nugget if krige else 0.0)
    return E, v


# ------------------------------------------------------------------------------------------------- inputs
SEED = 20261021
EDGE = (31, 32, 33, 63, 64, 65, 127, 128, 129)
M_TARGETS = 70
# (dim, n) / (dim, n, salt) -> how often the cloud's seed was moved on.  The rule is unfit() below, a CPU rule and nothing
# else: every entry is the SMALLEST count at which unfit() has no objection, and every cloud without an entry passes at 0
# (tests/test_tiny_ref.py asserts both, so no seed can have been moved for any other reason)
RESEED = {(1, 5): 1, (1, 6): 1, (1, 7): 1, (1, 8): 10, (2, 8): 1,
          (3, 13, 1): 1, (3, 14, 1): 1, (3, 15, 1): 1}                        # (dim, n, salt): the modified Shepard clouds


def small_sizes(lo):
    """lo .. lo + 4, and 8 where that lies above"""
    return [lo + i for i in range(5)] + ([8] if 8 > lo + 4 else [])


def response(x):
    """smooth, O(1), no symmetry (test_gpu_local.response)"""
    return 2.0 + np.sin(3.0 * x[:, 0]) + (np.cos(2.0 * x[:, 1]) if x.shape[1] > 1 else 0.0) + (0.5 * x[:, 2] if x.shape[1] > 2 else 0.0)


def fields(x, k):
    """k smooth, different responses on the centres; column 0 is response(x)"""
    f = response(x)
    maps = [lambda v: v, np.sin, lambda v: v * v + 0.5 * v, np.cos, lambda v: np.exp(0.3 * v), lambda v: 1.0 / (2.0 + v * v)]
    return np.ascontiguousarray(np.stack([maps[q % len(maps)]((1.0 + q // len(maps)) * f) for q in range(k)], axis=1))


_clouds = {}


def cloud(dim, n, salt=0, reseed=None):
    """(x, F n x 9, y): a seeded cloud in the unit box, nine responses, and the targets -- the sites, points inside, ten
    points up to 10 % outside the box, one NaN row last; 70 rows where n leaves room, n + 51 otherwise.  salt: another
    stream of the same kind (the modified Shepard cases have seeds of their own).  reseed: the cloud another count of
    RESEED would give (for the rule's own checks).  Read-only."""
    key = (dim, n, salt) if salt else (dim, n)
    if reseed is not None and reseed != RESEED.get(key, 0):
        key = key + ("reseed", reseed)
    if key not in _clouds:
        rng = np.random.default_rng(SEED + 1000 * dim + n + 100000 * (RESEED.get(key, 0) if reseed is None else reseed) + 10000000 * salt)
        if n < EDGE[0]:
            x = rng.random((n, dim))
        else:                                               # spacing: one site per cell of a lattice, jittered by 30 % of the cell
            g = int(np.ceil(n ** (1.0 / dim)))
            cells = rng.permutation(g ** dim)[:n]
            ijk = np.stack([(cells // g ** a) % g for a in range(dim)], axis=1)
            x = (ijk + 0.5 + 0.6 * (rng.random((n, dim)) - 0.5)) / g
        inside = rng.random((max(M_TARGETS - n - 11, 40), dim))
        out = rng.random((10, dim))
        axis, side, depth = rng.integers(0, dim, 10), rng.integers(0, 2, 10), 0.1 * rng.random(10)
        out[np.arange(10), axis] = np.where(side == 1, 1.0 + depth, -depth)
        y = np.ascontiguousarray(np.vstack([x, inside, out, np.full((1, dim), np.nan)]))
        F = fields(x, 9)
        for a in (x, F, y):
            a.setflags(write=False)
        _clouds[key] = (x, F, y)
    return _clouds[key]


RBF_TYPES = ("gaussian", "tps", "wendland", "matern32", "matern52", "imq")
KRIGE_TYPES = ("kriging", "kriging_matern32", "kriging_matern52")
PD_TYPES = tuple(t for t in RBF_TYPES if t != "tps") + KRIGE_TYPES            # leave-one-out and the fit criteria
NUGGET = {"kriging": 0.0, "kriging_matern32": 0.0, "kriging_matern52": 1e-3}  # as tests/test_gpu_local.py pairs them
EDGE_TYPES = ("matern52", "wendland", "kriging_matern52")
COND_CAP = 1e4


def true_minimum(typ, dim, drift=0):
    """the smallest size at which the type has an interpolant on points in general position"""
    if typ == "tps":
        return 2                                            # N = 1: the matrix is [0]
    if typ == "tps_affine":
        return max(3, dim + 1)
    if drift:
        return ukrige_ref.n_terms(dim, drift)
    return 1


def small_cases():
    """(typ, dim, n, drift) of every global model of the smallest sizes"""
    out = []
    for typ in RBF_TYPES + ("tps_affine",) + KRIGE_TYPES:
        for dim in (1, 2, 3):
            for drift in ((0, 1, 2) if typ in KRIGE_TYPES else (0,)):
                out += [(typ, dim, n, drift) for n in small_sizes(true_minimum(typ, dim, drift))]
    return out


def edge_cases():
    """(typ, dim, n, drift) at the factorisation's block boundaries: 2-D, and a linear drift for the kriging type"""
    return [(typ, 2, n, drift) for typ in EDGE_TYPES for n in EDGE for drift in ((0, 1) if typ in KRIGE_TYPES else (0,))]


def nugget_of(typ):
    return NUGGET.get(typ, 0.0)


def local_cases():
    """(typ, dim, n, k, drift) of the local route: k = N and k = N - 1; with a linear drift from k = dim + 2 = N up"""
    out = []
    for typ in KRIGE_TYPES:
        for dim in (1, 2, 3):
            for n in small_sizes(1):
                out += [(typ, dim, n, k, 0) for k in (n, n - 1) if k >= 1]
            for n in small_sizes(dim + 2):
                out += [(typ, dim, n, k, 1) for k in (n, n - 1) if k >= dim + 2]
    return out


def neighbour_sets(x, y, k):
    """(idx m x k nearest first with ties to the smaller index, relative gap of r^2 between the k-th and the (k+1)-th
    neighbour per target: inf where k = n) in extended precision; a NaN target: -1 and inf"""
    X, n = _mat(x), len(x)
    idx, gap = np.full((len(y), k), -1, dtype=np.int32), np.full(len(y), np.inf)
    for i, row in enumerate(y):
        if np.isnan(row).any():
            continue
        Y = _mat(row.reshape(1, -1))
        r2 = [mp.fsum((Y[0, c] - X[j, c]) ** 2 for c in range(X.cols)) for j in range(n)]
        order = sorted(range(n), key=lambda j: (r2[j], j))
        idx[i] = order[:k]
        if k < n and r2[order[k]] > 0:
            gap[i] = float((r2[order[k]] - r2[order[k - 1]]) / r2[order[k]])
    return idx, gap


def local_krige(typ, dim, x, f, y, idx, drift=0):
    """(s, var) of local kriging at the finite targets from their neighbour rows: one Model per distinct neighbourhood, with
    the shape of the WHOLE cloud.  A linear drift spans the same functions in any affine coordinates, so the model's own
    standardisation serves for the device's target-centred one.  NaN rows of y stay NaN."""
    kind, _, _ = TYPES[typ]
    eps = default_eps(kind, len(x), dim)
    s, v, models = np.full(len(y), np.nan), np.full(len(y), np.nan), {}
    for i in range(len(y)):
        if idx[i, 0] < 0:
            continue
        key = tuple(sorted(int(j) for j in idx[i]))
        if key not in models:
            models[key] = Model(kind, eps, x[list(key)], f[list(key)], tail=drift, nugget=nugget_of(typ))
        s[i], v[i] = models[key].values(y[i:i + 1])[0, 0], models[key].variance(y[i:i + 1])[0]
    return s, v


# ------------------------------------------------------------------------------------------------- meshes of a few simplices
# by hand: one triangle, two triangles (the Delaunay diagonal of a convex quadrilateral), one tetrahedron, two tetrahedra
# on either side of a shared face.  Simplex k's neighbour j lies opposite its vertex j (-1: the hull), as QHull writes them.
HAND = {
    (2, 3): (np.array([[0.125, 0.1875], [0.875, 0.125], [0.375, 0.875]]), [[0, 1, 2]], [[-1, -1, -1]]),
    (2, 4): (np.array([[0.125, 0.1875], [0.875, 0.125], [0.8125, 0.75], [0.25, 0.875]]), [[0, 1, 2], [0, 2, 3]], [[-1, 1, -1], [-1, -1, 0]]),
    (3, 4): (np.array([[0.125, 0.125, 0.25], [0.875, 0.1875, 0.3125], [0.3125, 0.875, 0.375], [0.375, 0.3125, 0.9375]]),
             [[0, 1, 2, 3]], [[-1, -1, -1, -1]]),
    (3, 5): (np.array([[0.125, 0.125, 0.25], [0.875, 0.1875, 0.3125], [0.3125, 0.875, 0.375], [0.375, 0.3125, 0.9375],
                       [0.5, 0.4375, 0.0625]]), [[0, 1, 2, 3], [0, 1, 2, 4]], [[-1, -1, -1, 1], [-1, -1, -1, 0]]),
}
MESH_SIZES = {2: (3, 4, 5, 6, 7, 8), 3: (4, 5, 6, 7, 8)}
_meshes = {}


def mesh_scene(dim, n):
    """(x, F n x 3, simplices, neighbours, y, tag): the hand-built mesh of HAND, or scipy's Delaunay triangulation of
    tiny_ref.cloud(dim, n).  Targets: the vertices ("vertex"); the centroid of every simplex ("centroid"); two points on
    every interior edge (2-D) / face (3-D) ("interior"); the midpoint of every hull edge / centroid of every hull face
    ("hull"); four points well inside every simplex ("inner"); the cloud's remaining targets, inside or outside the mesh as they fall ("free"); one NaN row.  Read-only."""
    if (dim, n) not in _meshes:
        from scipy.spatial import Delaunay
        if (dim, n) in HAND:
            x, simp, nbr = HAND[(dim, n)]
            simp, nbr = np.array(simp, dtype=np.int32), np.array(nbr, dtype=np.int32)
        else:
            x = np.array(cloud(dim, n)[0])
            d = Delaunay(x)
            simp, nbr = np.ascontiguousarray(d.simplices, dtype=np.int32), np.ascontiguousarray(d.neighbors, dtype=np.int32)
        free = cloud(dim, n)[2][n:-1]
        rows, tags = [x], ["vertex"] * n
        rows.append(x[simp].mean(axis=1)); tags += ["centroid"] * len(simp)
        for t in range(len(simp)):
            for j in range(dim + 1):
                face = x[np.delete(simp[t], j)]                          # opposite vertex j
                if nbr[t, j] < 0:
                    rows.append(face.mean(axis=0)[None, :]); tags.append("hull")
                elif nbr[t, j] > t:
                    w = np.array([0.5, 0.3, 0.2])[:dim] if dim == 3 else np.array([0.25, 0.75])
                    rows.append((w @ face)[None, :]); rows.append((w[::-1] @ face)[None, :]); tags += ["interior"] * 2
        rng = np.random.default_rng(SEED + 7 * dim + n)
        for t in range(len(simp)):                               # four points well inside every simplex
            w = 0.1 + rng.random((4, dim + 1))
            rows.append((w / w.sum(axis=1, keepdims=True)) @ x[simp[t]]); tags += ["inner"] * 4
        rows.append(free); tags += ["free"] * len(free)
        rows.append(np.full((1, dim), np.nan)); tags.append("nan")
        y = np.ascontiguousarray(np.vstack(rows))
        F = fields(x, 3)
        for a in (x, F, simp, nbr, y):
            a.setflags(write=False)
        _meshes[(dim, n)] = (x, F, simp, nbr, y, np.array(tags))
    return _meshes[(dim, n)]


# ------------------------------------------------------------------------------------------------- modified Shepard
SHEPARD_MIN = {2: (5, 7), 3: (9, 11)}                      # dim -> (nq = nw, the smallest size: max(nq, nw) + 2)


SHEPARD_SALT = 1


def shepard_cases():
    """(dim, n): the true minimum with the smallest neighbour counts the kernel takes, and the four sizes above it"""
    return [(dim, SHEPARD_MIN[dim][1] + i) for dim in (2, 3) for i in range(5)]


# ------------------------------------------------------------------------------------------------- the rule behind RESEED
SHEPARD_RHO_MIN = 1e-3                                     # the rank margin tests/test_gpu_shepard.py asks of its clouds


def unfit(dim, n, salt=0, reseed=None):
    """None when the cloud (dim, n, salt) at that reseed count may be used, else the first objection as text.  fp64 / mpmath
    on the CPU only.  salt 0 (the RBF, kriging and local cases of that shape): every system matrix of small_cases() /
    edge_cases() has a condition number <= COND_CAP; every k = N - 1 neighbourhood of local_cases() is decided by a relative
    r^2 gap > 1e-9 and its system matrix is under the cap too.  SHEPARD_SALT: the reference model of shepard_ref at the
    smallest neighbour counts has no coincident sites, every nodal fit quadratic (mode 2) with rho >= SHEPARD_RHO_MIN and a
    scaled-matrix condition number <= COND_CAP, and covers every finite target."""
    x, F, y = cloud(dim, n, salt, reseed)
    if salt == SHEPARD_SALT:
        import shepard_ref
        nq = SHEPARD_MIN[dim][0]
        m = shepard_ref.fit(x, F[:, 0], nq, nq)
        if m["coincident"] or not (m["mode"] == 2).all():
            return "a nodal fit is not quadratic"
        if m["rho"].min() < SHEPARD_RHO_MIN or m["cond"].max() > COND_CAP:
            return f"nodal fit: rho {m['rho'].min():.2e}, cond {m['cond'].max():.2e}"
        if not np.isfinite(shepard_ref.evaluate(m, y[:-1])[0]).all():
            return "a target is covered by no node"
        return None
    for typ, d, nn, drift in small_cases() + edge_cases():
        if (d, nn) == (dim, n):
            c = np.linalg.cond(system_matrix(typ, dim, x, nugget=nugget_of(typ), drift=drift))
            if not c <= COND_CAP:
                return f"{typ} drift {drift}: cond {c:.2e}"
    for typ, d, nn, k, drift in local_cases():
        if (d, nn) == (dim, n) and k < n and typ == KRIGE_TYPES[0]:      # the neighbourhoods do not depend on the type
            idx, gap = neighbour_sets(x, y, k)
            if not (gap > 1e-9).all():
                return f"k = {k}: neighbour gap {gap.min():.2e}"
            for t in KRIGE_TYPES:
                for key in {tuple(sorted(row)) for row in idx[:-1].tolist()}:
                    c = np.linalg.cond(system_matrix(t, dim, x[list(key)], eps=default_eps(TYPES[t][0], n, dim), nugget=nugget_of(t), drift=drift))
                    if not c <= COND_CAP:
                        return f"{t} k = {k} drift {drift}: local cond {c:.2e}"
    return None


def cloud_shapes():
    """every (dim, n, salt) the GPU file draws from cloud()"""
    out = {(d, n, 0) for _, d, n, _ in small_cases() + edge_cases()} | {(d, n, 0) for _, d, n, _, _ in local_cases()}
    return sorted(out | {(d, n, SHEPARD_SALT) for d, n in shepard_cases()})
