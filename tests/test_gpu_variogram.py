"""-m gpu: the empirical variogram (csrc/hip/variogram.hip) against the integer reference of tests/variogram_ref.py.

The pair count and the words of sum (f_i - f_j)^2 are a pure function of the input under IEEE arithmetic: they are compared for
EQUALITY, with the three shifts.  The sums of h and of sqrt|f_i - f_j| contain one device sqrt per term whose last bit is not
pinned: they are compared as values, to a relative (P_b + 8) 2^-52 with P_b the count of the bin -- one rounding per term plus
the quantisation.
"""
from fractions import Fraction

import numpy as np
import pytest

import variogram_ref as ref
from gpu_util import dev, ptr

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 2, 63, 64, 65, 257)
BINS = (1, 15, 256)
_cache = {}


def cloud(n, dim, seed=0):
    """random sites in the unit box, f = a smooth function plus noise"""
    rng = np.random.default_rng(1000 * seed + 10 * n + dim)
    x = rng.random((n, dim))
    f = np.sin(3.0 * x[:, 0]) + 0.5 * np.cos(5.0 * x.sum(axis=1)) + 0.1 * rng.standard_normal(n) if n else np.zeros(0)
    return x, f


def reference(x, f, h_max, n_bins, key=None):
    if key is None:
        return ref.Reference(x, f, h_max, n_bins)
    if key not in _cache:
        _cache[key] = ref.Reference(x, f, h_max, n_bins)
    return _cache[key]


def run(ctx, x, f, h_max, n_bins, pad=0):
    """the raw entry on device copies of (x, f); pad > 0 stores x with a row pitch of dim + pad"""
    n, dim = x.shape
    xs = np.full((max(n, 1), dim + pad), np.nan)
    xs[:n, :dim] = x
    d_x, d_f = dev(xs), dev(f if n else np.zeros(1))
    st, acc, shift = ctx.variogram(ptr(d_x), n, dim, dim + pad, ptr(d_f), h_max, n_bins)
    return st, acc, shift


def compare(acc, shift, r, what):
    """equality of the count, the (df)^2 words and the shifts; the two sqrt sums as values.  Returns the largest value error in
    units of (P_b + 8) 2^-52."""
    want = r.acc()
    assert shift == r.shift, (what, shift, r.shift)
    assert np.array_equal(acc[:, :3], want[:, :3]), what
    worst = 0.0
    for b in range(r.n_bins):
        nb = r.count[b]
        if nb == 0:
            assert not acc[b].any(), (what, b)
            continue
        for k in (1, 2):
            got = ref.words_to_value(acc[b, 1 + 2 * k], acc[b, 2 + 2 * k], shift[k])
            exact = r.exact(k, b)
            bound = Fraction(nb + 8, 1 << 52) * exact
            assert abs(got - exact) <= bound, (what, b, k, float(got), float(exact))
            if exact:
                worst = max(worst, float(abs(got - exact) / bound))
    return worst


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_words_equal_the_reference_at_the_smallest_shapes(pkg, dim):
    ctx = pkg.HipContext.on_torch_stream(0)
    h_max = {1: 0.2, 2: 0.35, 3: 0.5}[dim]
    worst = 0.0
    for n in SIZES:
        x, f = cloud(n, dim)
        for n_bins in BINS:
            st, acc, shift = run(ctx, x, f, h_max, n_bins)
            assert st == 0, (n, n_bins)
            r = reference(x, f, h_max, n_bins, key=("small", n, dim, n_bins))
            if n < 2:
                assert not acc.any() and shift == [0, r.shift[1], 0] and ctx.variogram_pairs_tested() == 0
            worst = max(worst, compare(acc, shift, r, (n, dim, n_bins)))
            assert int(acc[:, 0].sum()) <= ctx.variogram_pairs_tested() <= n * (n - 1) // 2 or n < 2
    print(f"dim {dim}: largest error of the sqrt sums {worst:.3f} of the bound (P_b + 8) 2^-52")
    ctx.close()


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_non_unit_row_pitch(pkg, dim):
    ctx = pkg.HipContext.on_torch_stream(0)
    x, f = cloud(257, dim)
    h_max = {1: 0.2, 2: 0.35, 3: 0.5}[dim]
    st, acc, shift = run(ctx, x, f, h_max, 15, pad=2)                      # the padding columns hold NaN: they must not be read
    assert st == 0
    compare(acc, shift, reference(x, f, h_max, 15, key=("small", 257, dim, 15)), ("pitch", dim))
    ctx.close()


@pytest.mark.parametrize("shape", [(17, 17), (6, 6, 6)])
def test_integer_lattice_pairs_on_the_bin_edges(pkg, shape):
    """h_max = 4, 4 bins: the edges are r2 = 0, 1, 4, 9, 16 and many pairs sit exactly on one.  A pair at r2 = b^2 belongs to bin b;
    the pairs at r2 = 16 are excluded."""
    ctx = pkg.HipContext.on_torch_stream(0)
    g = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), axis=-1).reshape(-1, len(shape))
    x = g.astype(np.float64)
    f = np.cos(0.7 * x.sum(axis=1))
    st, acc, shift = run(ctx, x, f, 4.0, 4)
    assert st == 0
    d = g[:, None, :] - g[None, :, :]
    r2 = (d * d).sum(axis=-1)[np.triu_indices(len(g), 1)]                # integers: no rounding anywhere
    want = [int(((r2 >= b * b) & (r2 < (b + 1) * (b + 1))).sum()) for b in range(4)]
    assert (r2 == 16).sum() > 0 and [int(c) for c in acc[:, 0]] == want
    compare(acc, shift, reference(x, f, 4.0, 4), ("lattice", shape))
    ctx.close()


def test_duplicated_sites_land_in_bin_zero(pkg):
    ctx = pkg.HipContext.on_torch_stream(0)
    x0, f0 = cloud(40, 2, seed=3)
    x, f = np.repeat(x0, 3, axis=0), np.repeat(f0, 3) + np.tile([0.0, 0.25, -0.5], 40)
    st, acc, shift = run(ctx, x, f, 1e-3, 15)                              # nothing but the coincident pairs is this close
    assert st == 0 and int(acc[0, 0]) == 40 * 3 and not acc[1:].any()
    assert acc[0, 3] == 0 and acc[0, 4] == 0                             # sum h = 0
    compare(acc, shift, reference(x, f, 1e-3, 15), "duplicates")
    st, acc, shift = run(ctx, x, f, 0.3, 15)
    assert st == 0 and int(acc[0, 0]) >= 40 * 3
    compare(acc, shift, reference(x, f, 0.3, 15), "duplicates in a cloud")
    ctx.close()


def test_row_order_and_repetition_do_not_change_a_word(pkg):
    ctx = pkg.HipContext.on_torch_stream(0)
    x, f = cloud(2000, 2, seed=5)
    st, acc, shift = run(ctx, x, f, 0.15, 15)
    st2, acc2, shift2 = run(ctx, x, f, 0.15, 15)
    perm = np.random.default_rng(9).permutation(len(x))
    st3, acc3, shift3 = run(ctx, x[perm], f[perm], 0.15, 15)
    other = pkg.HipContext.on_torch_stream(0)
    st4, acc4, shift4 = run(other, x, f, 0.15, 15)
    assert st == st2 == st3 == st4 == 0
    assert np.array_equal(acc, acc2) and np.array_equal(acc, acc3) and np.array_equal(acc, acc4) and shift == shift2 == shift3 == shift4
    assert acc[:, 0].min() > 0
    other.close()
    ctx.close()


def test_utm_sized_coordinates(pkg):
    ctx = pkg.HipContext.on_torch_stream(0)
    x, f = cloud(257, 2, seed=7)
    x = x * 1000.0 + 5.0e5
    st, acc, shift = run(ctx, x, f, 350.0, 15)
    assert st == 0
    compare(acc, shift, reference(x, f, 350.0, 15), "utm")
    ctx.close()


@pytest.mark.parametrize("where", ["x", "f"])
@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_non_finite_input_is_edom_with_zeroed_words(pkg, where, value):
    ctx = pkg.HipContext.on_torch_stream(0)
    x, f = cloud(257, 2)
    if where == "x":
        x[100, 1] = value
    else:
        f[200] = value
    st, acc, shift = run(ctx, x, f, 0.35, 15)
    assert st == pkg.GSL_EDOM and not acc.any() and ctx.variogram_pairs_tested() == 0
    x, f = cloud(257, 2)
    st, acc, shift = run(ctx, x, f, 0.35, 15)                              # the context is as usable as before
    assert st == 0
    compare(acc, shift, reference(x, f, 0.35, 15, key=("small", 257, 2, 15)), "after EDOM")
    ctx.close()


def test_facade_get_against_exact_rationals(pkg):
    x, f = cloud(257, 2)
    v = pkg.Variogram(2, 15)
    assert v.compute(x, f, 0.35) == 0 and v.h_max() == 0.35
    r = reference(x, f, 0.35, 15, key=("small", 257, 2, 15))
    worst = [0.0, 0.0, 0.0]
    for est in (ref.MATHERON, ref.CRESSIE):
        st, lag, gamma, count = v.get(est)
        want_lag, want_gamma, want_count = r.get(est, exact=True)
        assert st == 0 and np.array_equal(count, want_count) and count.min() > 0
        for b in range(15):
            nb = int(count[b])
            e_lag = abs(lag[b] / want_lag[b] - 1)
            e_gam = abs(gamma[b] / want_gamma[b] - 1)
            assert e_lag <= 4 * 2.0 ** -53, (est, b, e_lag)
            if est == ref.MATHERON:
                assert e_gam <= 4 * 2.0 ** -53, (b, e_gam)
                worst[1] = max(worst[1], e_gam / 2.0 ** -53)
            else:
                assert e_gam <= 4 * (nb + 8) * 2.0 ** -52, (b, e_gam)
                worst[2] = max(worst[2], e_gam / (4 * (nb + 8) * 2.0 ** -52))
            worst[0] = max(worst[0], e_lag / 2.0 ** -53)
    print(f"get: lag off by {worst[0]:.2f} x 2^-53, Matheron gamma by {worst[1]:.2f} x 2^-53, Cressie gamma by {worst[2]:.3f} of its bound")
    v.close()


def test_facade_lag_of_exact_distances(pkg):
    """sites on a line at dyadic spacings: every h is exact, so the lag itself is held to 4 x 2^-53"""
    x = (np.arange(65, dtype=np.float64) * 0.125).reshape(-1, 1)
    f = np.sin(x[:, 0])
    v = pkg.Variogram(1, 4)
    assert v.compute(x, f, 2.0) == 0
    st, lag, gamma, count = v.get(ref.MATHERON)
    want_lag, want_gamma, want_count = ref.Reference(x, f, 2.0, 4).get(ref.MATHERON, exact=True)
    assert st == 0 and np.array_equal(count, want_count)
    assert np.max(np.abs(lag / want_lag - 1)) <= 4 * 2.0 ** -53 and np.max(np.abs(gamma / want_gamma - 1)) <= 4 * 2.0 ** -53
    v.close()


def test_facade_empty_bins_and_default_h_max(pkg):
    rng = np.random.default_rng(11)
    x = np.concatenate([rng.random((20, 2)) * 0.05, rng.random((20, 2)) * 0.05 + [0.8, 0.0]])
    f = rng.standard_normal(40)
    v = pkg.Variogram(2, 15)
    assert v.compute(x, f, 1.0) == 0
    st, lag, gamma, count = v.get()
    r = ref.Reference(x, f, 1.0, 15)
    assert st == 0 and [int(c) for c in count] == r.count and 0 in r.count
    empty = count == 0
    assert np.isnan(lag[empty]).all() and np.isnan(gamma[empty]).all() and np.isfinite(lag[~empty]).all() and np.isfinite(gamma[~empty]).all()
    st, lag2, gamma2, _ = v.get(ref.CRESSIE)
    assert st == 0 and np.isnan(gamma2[empty]).all() and np.isfinite(gamma2[~empty]).all()
    # outputs may be NULL
    assert pkg.lib().gsl_sinterp_variogram_get(v._h, 0, None, None, None) == 0
    # h_max <= 0: a third of the diagonal of the bounding box
    for h in (0.0, -1.0):
        assert v.compute(x, f, h) == 0
        ext = x.max(axis=0) - x.min(axis=0)
        want = np.sqrt(ext[0] * ext[0] + ext[1] * ext[1]) / 3.0
        assert abs(v.h_max() - want) <= 2 * np.spacing(want)
    # a failed compute leaves no variogram behind
    f[3] = np.nan
    assert v.compute(x, f, 1.0) == pkg.GSL_EDOM and np.isnan(v.h_max()) and v.get()[0] == pkg.GSL_EINVAL
    # a constant response is a pure nugget of 0: the relative nugget does not exist
    assert v.compute(x, np.full(40, 3.0), 1.0) == 0
    st, eps, nug, s2, wss = v.fit("kriging_matern32")
    assert st == pkg.GSL_EDOM and all(np.isnan(t) for t in (eps, nug, s2, wss))
    assert v.apply(pkg.Sinterp("kriging_matern32", 2, 40)) == pkg.GSL_EINVAL
    v.close()


def test_pruning_is_a_condition(pkg):
    """n = 8192 uniform in the unit square, h_max = 0.02: cells between h_max and 2 h_max on a side make a 3 x 3 block cover at most
    36 h_max^2 = 1.4 % of the square, so 10 % of all pairs leaves a factor of seven"""
    import torch
    ctx = pkg.HipContext.on_torch_stream(0)
    n = 8192
    x = np.random.default_rng(21).random((n, 2))
    f = np.sin(4.0 * x[:, 0]) * np.cos(3.0 * x[:, 1])
    st, acc, shift = run(ctx, x, f, 0.02, 15)
    torch.cuda.synchronize()
    want, within = ref.counts(x, 0.02, 15)
    tested = ctx.variogram_pairs_tested()
    print(f"pairs tested {tested} = {tested / (n * (n - 1) / 2):.4%} of all, {within} within h_max")
    assert st == 0 and np.array_equal(acc[:, 0].astype(np.int64), want)
    assert within <= tested <= 0.10 * n * (n - 1) / 2
    ctx.close()


def matern_field(n, seed, eps=6.0, sill=4.0, nugget=0.05, mean=10.0):
    rng = np.random.default_rng(seed)
    x = rng.random((n, 2))
    d = x[:, None, :] - x[None, :, :]
    t = np.sqrt(3.0) * eps * np.sqrt((d * d).sum(axis=-1))
    cov = sill * ((1.0 + t) * np.exp(-t) + nugget * np.eye(n))
    f = mean + np.linalg.cholesky(cov) @ rng.standard_normal(n)
    return x, f


def reference_pipeline(x, f, kind=ref.MATERN32):
    ext = x.max(axis=0) - x.min(axis=0)
    h_max = float(np.sqrt(ext[0] * ext[0] + ext[1] * ext[1]) / 3.0)
    r = ref.Reference(x, f, h_max, 15)
    lag, gamma, count = r.get(ref.MATHERON, exact=False)
    eps, c0, c, wss, _ = ref.fit_model(kind, ref.W_COUNT_H2, lag, gamma, count, 0.1 / h_max, 100.0 / h_max)
    return h_max, eps, c0 / c, c


def test_end_to_end_variogram_to_local_kriging(pkg):
    n = 1500
    x, f = matern_field(n, seed=2024)
    h_max, r_eps, r_nug, r_s2 = reference_pipeline(x, f)
    print(f"reference pipeline: h_max {h_max:.4f}, eps {r_eps:.4f}, nugget {r_nug:.4f}, sigma2 {r_s2:.4f}")
    assert 3.0 <= r_eps <= 12.0                                          # the data were drawn with eps = 6
    v = pkg.Variogram(2, 15)
    assert v.compute(x, f) == 0 and abs(v.h_max() - h_max) <= 2 * np.spacing(h_max)
    st, eps, nug, s2, wss = v.fit("kriging_matern32", pkg.Variogram.MATHERON, pkg.Variogram.W_COUNT_H2)
    print(f"device pipeline: eps off {abs(eps / r_eps - 1):.2e}, nugget off {abs(nug / r_nug - 1):.2e}, sigma2 off {abs(s2 / r_s2 - 1):.2e}")
    assert st == 0 and wss >= 0.0
    assert abs(eps / r_eps - 1) <= 1e-9 and abs(nug / r_nug - 1) <= 1e-9 and abs(s2 / r_s2 - 1) <= 1e-9
    g = pkg.Sinterp("kriging", 2, n)
    assert v.apply(g) == pkg.GSL_EINVAL                                  # another type than the one fitted
    s = pkg.Sinterp("kriging_matern32", 2, n)
    assert v.apply(s) == 0 and s._p.contents.shape == eps and s._p.contents.nugget == nug
    assert s.set_neighbours(32) == 0 and s.init(x, f) == 0
    y = np.random.default_rng(5).random((100, 2))
    st, vals, _ = s.eval_many(y)
    assert st == 0 and np.isfinite(vals).all() and abs(vals.mean() - f.mean()) < 3.0 * np.sqrt(s2)
    v.close()
