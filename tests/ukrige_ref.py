"""numpy fp64 reference of universal kriging (kriging with a polynomial drift), shared by test_ukrige_api.py and
test_gpu_ukrige.py.

    s(y) = p(u(y))^T c + sum_j w_j phi(|y - x_j|),   [K P; P^T 0] [w; c] = [f; 0],   K = Phi + nugget I,
    sigma^2(y) = phi(0) - k^T K^-1 k + r^T S^-1 r,   r = p(u(y)) - B^T k(y),   B = K^-1 P,   S = P^T B,

with the basis in standardised coordinates u_a = (y_a - shift_a) scale_a (shift = centre of the sites' bounding box, scale
= 1 / half-extent), term order 1; u_1 .. u_d; u_a u_b for a <= b.

Two independent routes, which must agree to REF_TOL before either is used (Model.check):
  bordered   np.linalg.solve of the (n + q) saddle system, for the weights and for the variance multipliers
             ([K P; P^T 0] [lambda; mu] = [k; p], sigma^2 = 1 - k^T lambda - p^T mu);
  schur      Cholesky of K and the Schur complement S, the way the device code is organised.
The oracle library has no kriging; the formulas are the textbook ones (Chiles & Delfiner 3.4; Dubrule 1983 for the
leave-one-out rule with a drift)."""
import numpy as np

TOL = 1e-10
REF_TOL = 1e-11
GAUSSIAN, MATERN32, MATERN52 = 0, 3, 4
KIND = {"kriging": GAUSSIAN, "kriging_matern32": MATERN32, "kriging_matern52": MATERN52}


def default_eps(kind, n, dim):
    return (2.0 if kind == GAUSSIAN else 1.0) * n ** (1.0 / dim)


def phi(kind, eps, r):
    if kind == GAUSSIAN:
        return np.exp(-(eps * r) ** 2)
    if kind == MATERN32:
        t = np.sqrt(3.0) * eps * r
        return (1.0 + t) * np.exp(-t)
    t = np.sqrt(5.0) * eps * r
    return (1.0 + t + t * t / 3.0) * np.exp(-t)


def psi(kind, eps, r):
    """phi'(r) / r"""
    if kind == GAUSSIAN:
        return -2.0 * eps * eps * np.exp(-(eps * r) ** 2)
    if kind == MATERN32:
        return -3.0 * eps * eps * np.exp(-np.sqrt(3.0) * eps * r)
    t = np.sqrt(5.0) * eps * r
    return -(5.0 * eps * eps / 3.0) * (1.0 + t) * np.exp(-t)


def dist(a, b):
    return np.sqrt(((a[:, None, :] - b[None, :, :]) ** 2).sum(axis=2))


def n_terms(dim, order):
    return 1 if order == 0 else dim + 1 if order == 1 else (dim + 1) * (dim + 2) // 2


def geometry(x):
    lo, hi = x.min(axis=0), x.max(axis=0)
    half = 0.5 * (hi - lo)
    return lo + half, np.where(half > 0.0, 1.0 / np.where(half > 0.0, half, 1.0), 1.0)


def basis(y, shift, scale, order):
    """P (rows of y x q) and dP/dy (rows x q x dim, raw coordinates)"""
    u = (y - shift) * scale
    m, d = u.shape
    cols, grads = [np.ones(m)], [np.zeros((m, d))]
    for a in range(d):
        g = np.zeros((m, d))
        g[:, a] = scale[a]
        cols.append(u[:, a])
        grads.append(g)
    if order == 2:
        for a in range(d):
            for b in range(a, d):
                g = np.zeros((m, d))
                g[:, a] += u[:, b] * scale[a]
                g[:, b] += u[:, a] * scale[b]
                cols.append(u[:, a] * u[:, b])
                grads.append(g)
    return np.stack(cols, axis=1), np.stack(grads, axis=1)


class Model:
    """one universal-kriging model of nf fields (F: n x nf) in numpy, both routes"""

    def __init__(self, kind, eps, nugget, order, x, F):
        self.kind, self.eps, self.order, self.x = kind, eps, order, x
        F = F.reshape(len(x), -1)
        n = len(x)
        self.shift, self.scale = geometry(x)
        self.P, _ = basis(x, self.shift, self.scale, order)
        self.q = self.P.shape[1]
        self.K = phi(kind, eps, dist(x, x)) + nugget * np.eye(n)
        # bordered
        self.A = np.block([[self.K, self.P], [self.P.T, np.zeros((self.q, self.q))]])
        sol = np.linalg.solve(self.A, np.vstack([F, np.zeros((self.q, F.shape[1]))]))
        self.w, self.c = sol[:n], sol[n:]
        # Cholesky + Schur complement
        self.L = np.linalg.cholesky(self.K)
        Kinv = lambda R: np.linalg.solve(self.L.T, np.linalg.solve(self.L, R))
        self.B = Kinv(self.P)
        Af = Kinv(F)
        self.S = self.P.T @ self.B
        self.c2 = np.linalg.solve(self.S, self.P.T @ Af)
        self.w2 = Af - self.B @ self.c2

    def values(self, y, schur=False):
        k = phi(self.kind, self.eps, dist(y, self.x))
        p, _ = basis(y, self.shift, self.scale, self.order)
        return (k @ self.w2 + p @ self.c2) if schur else (k @ self.w + p @ self.c)

    def gradient(self, y, field=0):
        r = dist(y, self.x)
        diff = y[:, None, :] - self.x[None, :, :]
        g = ((psi(self.kind, self.eps, r) * self.w[:, field][None, :])[:, :, None] * diff).sum(axis=1)
        _, dp = basis(y, self.shift, self.scale, self.order)
        return g + np.einsum("mqd,q->md", dp, self.c[:, field])

    def variance(self, y, schur=False):
        k = phi(self.kind, self.eps, dist(y, self.x)).T                   # n x m
        p, _ = basis(y, self.shift, self.scale, self.order)
        if not schur:
            lam = np.linalg.solve(self.A, np.vstack([k, p.T]))
            return 1.0 - (k * lam[:len(self.x)]).sum(axis=0) - (p.T * lam[len(self.x):]).sum(axis=0)
        z = np.linalg.solve(self.L, k)
        r = p.T - self.B.T @ k
        return 1.0 - (z * z).sum(axis=0) + (r * np.linalg.solve(self.S, r)).sum(axis=0)

    def far_variance(self, y):
        """where every covariance vanishes: 1 + p^T S^-1 p"""
        p, _ = basis(y, self.shift, self.scale, self.order)
        return 1.0 + (p.T * np.linalg.solve(self.S, p.T)).sum(axis=0)

    def check(self, y, fmax):
        """the two routes against each other: (value error relative to fmax, variance error scaled by max(1, |want|))"""
        ev = np.abs(self.values(y) - self.values(y, schur=True)).max() / fmax
        a, b = self.variance(y), self.variance(y, schur=True)
        es = (np.abs(a - b) / np.maximum(1.0, np.abs(a))).max()
        assert ev < REF_TOL and es < REF_TOL, (ev, es)
        return ev, es


def loo_by_deletion(kind, eps, nugget, order, x, F, shift=None, scale=None):
    """(E n x nf, v n): refit without site i by the bordered system, predict at x_i; v = the variance of the prediction
    error of the OBSERVATION f_i (sigma^2 of the model without i at x_i, plus the nugget).  The basis keeps the
    standardisation of the full cloud, as the identity does (the span of the drift does not depend on it)."""
    F = F.reshape(len(x), -1)
    n = len(x)
    if shift is None:
        shift, scale = geometry(x)
    P, _ = basis(x, shift, scale, order)
    q = P.shape[1]
    Phi = phi(kind, eps, dist(x, x))
    K = Phi + nugget * np.eye(n)
    E, v = np.zeros(F.shape), np.zeros(n)
    for i in range(n):
        keep = np.arange(n) != i
        A = np.block([[K[np.ix_(keep, keep)], P[keep]], [P[keep].T, np.zeros((q, q))]])
        rhs = np.concatenate([Phi[keep, i], P[i]])
        lam = np.linalg.solve(A, np.column_stack([np.vstack([F[keep], np.zeros((q, F.shape[1]))]), rhs]))
        sol, mult = lam[:, :-1], lam[:, -1]
        E[i] = F[i] - (Phi[i, keep] @ sol[:n - 1] + P[i] @ sol[n - 1:])
        v[i] = 1.0 - Phi[keep, i] @ mult[:n - 1] - P[i] @ mult[n - 1:] + nugget
    return E, v


def loo_by_identity(kind, eps, nugget, order, x, F):
    """Dubrule with a drift: diag_i = (K^-1)_ii - B_i S^-1 B_i^T, e_i = w_i / diag_i, v_i = 1 / diag_i"""
    F = F.reshape(len(x), -1)
    m = Model(kind, eps, nugget, order, x, F)
    Kinv = np.linalg.inv(m.K)
    d = np.diag(Kinv) - (m.B * np.linalg.solve(m.S, m.B.T).T).sum(axis=1)
    return m.w2 / d[:, None], 1.0 / d


def local_ukrige(kind, eps, nugget, x, f, y, idx, check=True):
    """(s, var) of local universal kriging with a LINEAR drift at the targets from their neighbour rows idx (m x k, nearest
    first), in the local basis u = (x_i - y) / h, h the distance of the k-th neighbour, by the two routes; asserts that
    they agree to REF_TOL (values relative to max|f|, variances scaled by max(1, |want|)).  Returns (s, var, value
    disagreement per target, variance disagreement per target); check=False leaves the judgement to the caller, who may
    drop the targets whose neighbourhood is too close to collinear for fp64 to pin the answer down"""
    m, k = idx.shape
    xs, fs = x[idx], f[idx]                                                     # m x k x d, m x k
    d = x.shape[1]
    r = lambda a: np.sqrt((a ** 2).sum(axis=-1))
    K = phi(kind, eps, r(xs[:, :, None, :] - xs[:, None, :, :])) + nugget * np.eye(k)
    kv = phi(kind, eps, r(y[:, None, :] - xs))                                  # m x k
    h = r(xs[:, k - 1, :] - y)
    P = np.concatenate([np.ones((m, k, 1)), (xs - y[:, None, :]) / h[:, None, None]], axis=2)    # m x k x (d + 1)
    q = d + 1
    e0 = np.zeros((m, q))
    e0[:, 0] = 1.0
    # route 1: the bordered (k + q) system, for the weights of the data and for the variance multipliers
    A = np.zeros((m, k + q, k + q))
    A[:, :k, :k], A[:, :k, k:], A[:, k:, :k] = K, P, np.transpose(P, (0, 2, 1))
    lam = np.linalg.solve(A, np.concatenate([kv, e0], axis=1)[:, :, None])[:, :, 0]
    s1 = (lam[:, :k] * fs).sum(axis=1)
    v1 = 1.0 - (lam[:, :k] * kv).sum(axis=1) - lam[:, k]
    # route 2: Cholesky and the Schur complement, the way the kernel is organised
    L = np.linalg.cholesky(K)
    Li = np.linalg.inv(L)
    V, g, u = Li @ P, (Li @ fs[:, :, None])[:, :, 0], (Li @ kv[:, :, None])[:, :, 0]
    S = np.transpose(V, (0, 2, 1)) @ V
    c = np.linalg.solve(S, (np.transpose(V, (0, 2, 1)) @ g[:, :, None]))[:, :, 0]
    s2 = c[:, 0] + (u * (g - (V @ c[:, :, None])[:, :, 0])).sum(axis=1)
    rr = e0 - (np.transpose(V, (0, 2, 1)) @ u[:, :, None])[:, :, 0]
    v2 = 1.0 - (u * u).sum(axis=1) + (rr * np.linalg.solve(S, rr[:, :, None])[:, :, 0]).sum(axis=1)
    es = np.abs(s1 - s2) / np.abs(f).max()
    ev = np.abs(v1 - v2) / np.maximum(1.0, np.abs(v1))
    assert not check or (es.max() < REF_TOL and ev.max() < REF_TOL), (es.max(), ev.max())
    return s1, v1, es, ev
