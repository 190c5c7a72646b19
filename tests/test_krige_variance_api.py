"""The kriging-variance entry points that answer without a GPU: argument and state errors, workspace size."""


def test_set_variance_is_for_kriging_only(pkg):
    for kind in ("gaussian", "tps", "wendland"):
        s = pkg.Sinterp(kind, 2, 8)
        assert s.set_variance(1) == pkg.GSL_EINVAL
    k = pkg.Sinterp("kriging", 2, 8)
    assert k.set_variance(1) == 0 and k._p.contents.want_variance == 1
    assert k.set_variance(0) == 0 and k._p.contents.want_variance == 0


def test_variance_of_an_uninitialised_interpolant(pkg):
    import numpy as np
    y = np.zeros((5, 2))
    k = pkg.Sinterp("kriging", 2, 8)
    assert k.set_variance(1) == 0
    assert k.eval_variance_many(y)[0] == pkg.GSL_EINVAL
    st, v = k.eval_variance_e(y[0])
    assert st == pkg.GSL_EINVAL and v != v
    assert k.eval_variance_resident(None, 0, 2, None) == pkg.GSL_EINVAL
    g = pkg.Sinterp("gaussian", 2, 8)
    assert g.eval_variance_many(y)[0] == pkg.GSL_EINVAL


def test_workspace_covers_the_work_matrix(pkg):
    work = pkg.HipContext.krige_variance_work
    for n, chunk in ((1, 1), (100, 65), (129, 1), (700, 64), (4096, 8192), (16384, 8192)):
        assert work(n, chunk) >= n * chunk
