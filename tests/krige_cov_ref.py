"""numpy fp64 reference of the joint posterior covariance of kriging and of conditional simulation, shared by
test_krige_cov_api.py and test_gpu_krige_cov.py.  Ordinary kriging (order 0) or a drift of order 1 / 2, sill 1, the nugget
measurement noise:

    Sigma_ab = C(|ya_i - yb_j|) - [k_a; p_a]^T [K P; P^T 0]^-1 [k_b; p_b]
             = C(|ya_i - yb_j|) - k_a^T K^-1 k_b + r_a^T S^-1 r_b,      r = p(u(y)) - B^T k(y),  B = K^-1 P,  S = P^T B,

with k(y)_j = C(|y - x_j|), K = C + nugget I and the basis p of tests/ukrige_ref.py (order 0: p = 1).  Two independent
routes, which must agree to REF_TOL before either is used (CovModel.check):
  bordered   np.linalg.solve of the (n + q) saddle system with the right-hand sides [k_b; p_b];
  schur      Cholesky of K and of the Schur complement S, the way the device code is organised (Z = L^-1 k, T = Ls^-1 r).
A conditional draw is mean + sqrt(sigma2) chol(Sigma + jitter I) z with numpy's lower Cholesky factor, in target order."""
import numpy as np

import ukrige_ref as ref

TOL = ref.TOL
REF_TOL = ref.REF_TOL


class CovModel:
    """one kriging model (order 0, 1 or 2) of one field in numpy, both routes"""

    def __init__(self, kind, eps, nugget, order, x, f):
        self.kind, self.eps, self.order, self.x = kind, eps, order, x
        n = len(x)
        self.shift, self.scale = ref.geometry(x)
        self.P = self.basis(x)
        self.q = self.P.shape[1]
        self.K = ref.phi(kind, eps, ref.dist(x, x)) + nugget * np.eye(n)
        self.A = np.block([[self.K, self.P], [self.P.T, np.zeros((self.q, self.q))]])
        sol = np.linalg.solve(self.A, np.concatenate([f, np.zeros(self.q)]))
        self.w, self.c = sol[:n], sol[n:]
        self.L = np.linalg.cholesky(self.K)
        self.B = np.linalg.solve(self.L.T, np.linalg.solve(self.L, self.P))
        self.S = self.P.T @ self.B
        self.Ls = np.linalg.cholesky(self.S)

    def basis(self, y):
        return np.ones((len(y), 1)) if self.order == 0 else ref.basis(y, self.shift, self.scale, self.order)[0]

    def cross(self, y):
        """k(Y), n x m"""
        return ref.phi(self.kind, self.eps, ref.dist(y, self.x)).T

    def values(self, y):
        return self.cross(y).T @ self.w + self.basis(y) @ self.c

    def covariance(self, ya, yb=None, schur=False):
        yb = ya if yb is None else yb
        ka, kb, pa, pb = self.cross(ya), self.cross(yb), self.basis(ya), self.basis(yb)
        C = ref.phi(self.kind, self.eps, ref.dist(ya, yb))
        n = len(self.x)
        if not schur:
            lam = np.linalg.solve(self.A, np.vstack([kb, pb.T]))
            return C - ka.T @ lam[:n] - pa @ lam[n:]
        za, zb = np.linalg.solve(self.L, ka), np.linalg.solve(self.L, kb)
        ta, tb = np.linalg.solve(self.Ls, pa.T - self.B.T @ ka), np.linalg.solve(self.Ls, pb.T - self.B.T @ kb)
        return C - za.T @ zb + ta.T @ tb

    def variance(self, y):
        """the pointwise kriging variance by the formula of the variance entries, not through covariance()"""
        k, p = self.cross(y), self.basis(y)
        r = p.T - self.B.T @ k
        return 1.0 - (k * np.linalg.solve(self.K, k)).sum(axis=0) + (r * np.linalg.solve(self.S, r)).sum(axis=0)

    def check(self, ya, yb=None):
        """(the two routes against each other, the diagonal against variance()), absolute; asserts REF_TOL"""
        a, b = self.covariance(ya, yb), self.covariance(ya, yb, schur=True)
        e = np.abs(a - b).max()
        d = np.abs(np.diag(self.covariance(ya)) - self.variance(ya)).max()
        assert e < REF_TOL and d < REF_TOL, (e, d)
        return e, d

    def simulate(self, y, sigma2, jitter, zn, cov=None):
        """mean + sqrt(sigma2) chol(Sigma + jitter I) zn (np.linalg.LinAlgError when that is not positive definite)"""
        cov = self.covariance(y) if cov is None else cov
        A = np.linalg.cholesky(0.5 * (cov + cov.T) + jitter * np.eye(len(y)))
        return self.values(y)[:, None] + np.sqrt(sigma2) * (A @ zn)
