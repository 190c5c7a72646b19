"""numpy / Python reference of the empirical variogram (include/gsl_sinterp_hip.h, "BIN RULE") and of the model fit.

The words are Python integers: r2 = ((dx*dx) + (dy*dy)) + (dz*dz) and (f_i - f_j)^2 are formed with the same IEEE operations
the device performs, every term is quantised as rint(ldexp(t, shift)) and summed exactly.  The doubles of `get` come from
exact rationals.  The fit repeats the C search operation by operation.
"""
import math
from fractions import Fraction

import numpy as np

MATHERON, CRESSIE = 0, 1
W_COUNT, W_COUNT_H2, W_NONE = 0, 1, 2
GAUSSIAN, MATERN32, MATERN52 = 0, 3, 4


def edges2(h_max, n_bins):
    w = np.float64(h_max) / np.float64(n_bins)
    e = np.arange(n_bins + 1, dtype=np.float64) * w
    e2 = e * e
    e2[n_bins] = np.float64(h_max) * np.float64(h_max)
    return e2


def shifts(f, h_max):
    """shift[k] = 62 - frexp exponent of the bound of term k; a constant (or absent) response gives 0 for the f terms"""
    s = [0, 62 - math.frexp(float(h_max))[1], 0]
    f = np.asarray(f, dtype=np.float64)
    if f.size >= 2:
        spread = float(np.max(f) - np.min(f))
        if spread > 0.0:
            s[0] = 62 - math.frexp(spread * spread)[1]
            s[2] = 62 - math.frexp(math.sqrt(spread))[1]
    return s


def _r2(xi, xj):
    """xi [a, dim], xj [b, dim] -> [a, b], left to right over the axes"""
    d = xi[:, None, 0] - xj[None, :, 0]
    r2 = d * d
    for c in range(1, xi.shape[1]):
        d = xi[:, None, c] - xj[None, :, c]
        r2 = r2 + d * d
    return r2


def _quantise(t, shift):
    return np.rint(np.ldexp(t, shift)).astype(np.uint64)


def pair_terms(x, f, h_max, n_bins, chunk=512):
    """every pair i < j with r2 < h_max^2: (bin, r2, df) as flat arrays"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    f = np.ascontiguousarray(f, dtype=np.float64)
    n = x.shape[0]
    e2 = edges2(h_max, n_bins)
    bins, r2s, dfs = [], [], []
    for i0 in range(0, n, chunk):
        i1 = min(n, i0 + chunk)
        r2 = _r2(x[i0:i1], x[i0:])
        ii, jj = np.nonzero(r2 < e2[n_bins])
        keep = jj + i0 > ii + i0                       # column index is j - i0
        ii, jj = ii[keep], jj[keep]
        v = r2[ii, jj]
        bins.append(np.searchsorted(e2, v, side="right") - 1)
        r2s.append(v)
        dfs.append(f[i0 + ii] - f[i0 + jj])
    if not bins:
        return np.zeros(0, dtype=np.int64), np.zeros(0), np.zeros(0)
    return np.concatenate(bins), np.concatenate(r2s), np.concatenate(dfs)


def _sum_u64(q, bins, n_bins):
    """exact per-bin sums of uint64 terms as Python integers"""
    lo = np.zeros(n_bins, dtype=np.uint64)
    hi = np.zeros(n_bins, dtype=np.uint64)
    np.add.at(lo, bins, q & np.uint64(0xFFFFFFFF))
    np.add.at(hi, bins, q >> np.uint64(32))
    return [int(l) + (int(h) << 32) for l, h in zip(lo, hi)]


def counts(x, h_max, n_bins, chunk=512):
    """pair count per bin alone (any n that fits a row chunk of the distance matrix)"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    e2 = edges2(h_max, n_bins)
    out = np.zeros(n_bins, dtype=np.int64)
    within = 0
    for i0 in range(0, x.shape[0], chunk):
        i1 = min(x.shape[0], i0 + chunk)
        r2 = _r2(x[i0:i1], x[i0:])
        ii, jj = np.nonzero(r2 < e2[n_bins])
        keep = jj > ii
        v = r2[ii[keep], jj[keep]]
        within += v.size
        out += np.bincount(np.searchsorted(e2, v, side="right") - 1, minlength=n_bins)[:n_bins]
    return out, within


class Reference:
    """words[b] = [count, sum0, sum1, sum2] as Python integers (sum_k already lo + 2^64 hi), the shifts, and for the two sums
    that carry a sqrt their exact values as rationals of the HOST's correctly rounded sqrt"""

    def __init__(self, x, f, h_max, n_bins):
        x = np.ascontiguousarray(x, dtype=np.float64)
        f = np.ascontiguousarray(f, dtype=np.float64)
        self.n_bins, self.h_max = n_bins, float(h_max)
        self.shift = shifts(f, h_max)
        n = x.shape[0]
        self.count = [0] * n_bins
        self.s = [[0] * n_bins for _ in range(3)]
        self.bins = np.zeros(0, dtype=np.int64)
        if n < 2:
            return
        bins, r2, df = pair_terms(x, f, h_max, n_bins)
        self.bins, self.r2, self.df = bins, r2, df
        self.count = [int(c) for c in np.bincount(bins, minlength=n_bins)[:n_bins]]
        terms = (df * df, np.sqrt(r2), np.sqrt(np.abs(df)))
        self.terms = terms
        for k in range(3):
            self.s[k] = _sum_u64(_quantise(terms[k], self.shift[k]), bins, n_bins)

    def acc(self):
        """the 7 words per bin as the device lays them out"""
        out = np.zeros((self.n_bins, 7), dtype=np.uint64)
        for b in range(self.n_bins):
            out[b, 0] = self.count[b]
            for k in range(3):
                out[b, 1 + 2 * k] = self.s[k][b] & 0xFFFFFFFFFFFFFFFF
                out[b, 2 + 2 * k] = self.s[k][b] >> 64
        return out

    def value(self, k, b):
        """sum k of bin b as an exact rational of the quantised words"""
        return Fraction(self.s[k][b], 1 << self.shift[k]) if self.shift[k] >= 0 else Fraction(self.s[k][b] * (1 << -self.shift[k]))

    def exact(self, k, b):
        """sum k of bin b as the exact rational sum of the unquantised host terms"""
        t = self.terms[k][self.bins == b]
        return sum((Fraction(float(v)) for v in t), Fraction(0))

    def get(self, estimator, exact=True):
        """(lag, gamma, count) as correctly rounded doubles of exact rationals: of the unquantised host terms (exact=True) or of
        the quantised words"""
        lag, gam, cnt = (np.full(self.n_bins, np.nan) for _ in range(3))
        src = self.exact if exact else self.value
        for b in range(self.n_bins):
            nb = self.count[b]
            cnt[b] = nb
            if nb == 0:
                continue
            lag[b] = float(src(1, b) / nb)
            if estimator == MATHERON:
                gam[b] = float(src(0, b) / (2 * nb))
            else:
                m = src(2, b) / nb
                gam[b] = float(Fraction(1, 2) * m ** 4 / (Fraction(457, 1000) + Fraction(494, 1000) / nb))
        return lag, gam, cnt


def words_to_value(lo, hi, shift):
    return Fraction((int(hi) << 64) + int(lo), 1 << shift) if shift >= 0 else Fraction(((int(hi) << 64) + int(lo)) * (1 << -shift))


# ---------------------------------------------------------------------------- the fit
def rise(kind, eps, h):
    if kind == GAUSSIAN:
        t = eps * h
        return 1.0 - math.exp(-(t * t))
    if kind == MATERN32:
        t = math.sqrt(3.0) * eps * h
        return 1.0 - (1.0 + t) * math.exp(-t)
    t = math.sqrt(5.0) * eps * h
    return 1.0 - (1.0 + t + t * t / 3.0) * math.exp(-t)


def model(kind, eps, c0, c, h):
    return np.array([c0 + c * rise(kind, eps, float(v)) for v in np.atleast_1d(h)])


def _wss(kind, h, y, w, eps, c0, c):
    s = 0.0
    for hb, yb, wb in zip(h, y, w):
        r = yb - c0 - c * rise(kind, eps, hb)
        s += wb * r * r
    return s


def wls(kind, h, y, w, eps):
    sw = sg = sgg = sy = sgy = 0.0
    for hb, yb, wb in zip(h, y, w):
        g = rise(kind, eps, hb)
        sw += wb
        sg += wb * g
        sgg += wb * g * g
        sy += wb * yb
        sgy += wb * g * yb
    det = sw * sgg - sg * sg
    if det > 0.0:
        c = (sw * sgy - sg * sy) / det
        c0 = (sy - c * sg) / sw
        if c0 >= 0.0 and c >= 0.0:
            return _wss(kind, h, y, w, eps, c0, c), c0, c
    a0 = sy / sw
    a1 = sgy / sgg if sgg > 0.0 else 0.0
    a0 = a0 if a0 > 0.0 else 0.0
    a1 = a1 if a1 > 0.0 else 0.0
    w0, w1 = _wss(kind, h, y, w, eps, a0, 0.0), _wss(kind, h, y, w, eps, 0.0, a1)
    if w1 < w0:
        return w1, 0.0, a1
    return w0, a0, 0.0


def usable(weights, lag, gamma, count):
    h, y, w = [], [], []
    for lb, gb, nb in zip(lag, gamma, count):
        if not (nb > 0.0) or not math.isfinite(nb) or not math.isfinite(gb) or not math.isfinite(lb) or lb < 0.0:
            continue
        if weights == W_COUNT_H2 and not lb > 0.0:
            continue
        h.append(float(lb))
        y.append(float(gb))
        w.append(float(nb) if weights == W_COUNT else float(nb) / (float(lb) * float(lb)) if weights == W_COUNT_H2 else 1.0)
    return h, y, w


def fit_model(kind, weights, lag, gamma, count, eps_lo, eps_hi, n_grid=9, tol=1e-2, max_eval=40):
    """(eps, c0, c, wss, trace) by the fixed rule: grid in t = log eps, golden section around the first smallest grid value,
    the best point ever evaluated; None when fewer than 3 bins are usable"""
    h, y, w = usable(weights, lag, gamma, count)
    if len(h) < 3:
        return None
    trace = []
    best = [math.inf, math.nan, math.nan, math.nan]

    def ev(t, p=0.0):
        if len(trace) >= max_eval:
            return math.inf
        e = p if p != 0.0 else math.exp(t)
        v, c0, c = wls(kind, h, y, w, e)
        trace.append((e, v))
        if v < best[0]:
            best[:] = [v, e, c0, c]
        return v

    tlo, thi = math.log(eps_lo), math.log(eps_hi)
    k, g_best = 0, math.inf
    for j in range(n_grid):
        t = tlo + (thi - tlo) * (float(j) / float(n_grid - 1))
        v = ev(t, eps_lo if j == 0 else eps_hi if j == n_grid - 1 else 0.0)
        if v < g_best:
            g_best, k = v, j
    if math.isfinite(g_best):
        ka, kb = (k - 1 if k > 0 else 0), (k + 1 if k + 1 < n_grid else k)
        a = tlo + (thi - tlo) * (float(ka) / float(n_grid - 1))
        b = tlo + (thi - tlo) * (float(kb) / float(n_grid - 1))
        r = 0.6180339887498949
        cpt, dpt = b - r * (b - a), a + r * (b - a)
        fc = ev(cpt)
        fd = ev(dpt)
        while b - a > tol and len(trace) < max_eval:
            if fc <= fd:
                b, dpt, fd = dpt, cpt, fc
                cpt = b - r * (b - a)
                if b - a > tol:
                    fc = ev(cpt)
            else:
                a, cpt, fc = cpt, dpt, fd
                dpt = a + r * (b - a)
                if b - a > tol:
                    fd = ev(dpt)
    return best[1], best[2], best[3], best[0], trace
