"""The products of an ensemble chain on the device (nfa_ensemble_histogram, _covariance, _moments): marginal
histograms against numpy exactly, covariances against their longdouble twin, the moments of the model spectra against the
host route of `predict_moments` bit for bit, and all of them through `sample_pixels` and `sample_cube`."""
import numpy as np
import pytest

from nestfit_amd import ensemble
from test_ensemble import NOISE, _data, _runner, _stack
from test_sibling_models import MODES, mode_guard          # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu
LD = np.longdouble
U = 2.0 ** -53
FIELDS = ('mean', 'std', 'peak_mean', 'peak_std', 'total_mean', 'total_std')

# (cube pixels, pix, W, ncomp, masked, thin) after 12 steps with n_burn 5: N = 48, less than a wave; N = 1120, no multiple of
# a workgroup; two components with two slots left out, the cube's pixels out of order
CASES = {'48': (3, [0, 1, 2], 16, 1, False, 2), '1120': (2, [0, 1], 160, 1, False, 1), 'masked': (3, [2, 0], 32, 2, True, 1)}


def _ensemble(engine, mode, case, **options):
    """(runner, device ensemble after its run, free mask or None) of a case."""
    n_cube, pix, W, ncomp, masked, thin = CASES[case]
    runner = _runner(engine, ncomp, n_cube, **options)
    runner.set_exp_mode(mode)
    mask = runner.utrans.free_mask(ncomp) if masked else None
    pix = np.asarray(pix, dtype=np.int32)
    dev = ensemble.DeviceEnsemble(runner, pix, W, ensemble.starts(runner, pix, W, n_init=256, seed=3), mask)
    dev.run(12, 5, thin, 2.0, 1)
    return runner, dev, mask


def _edges(X, n_bins):
    """edges[ndim, n_bins + 1] from the samples X[P, N, ndim] themselves: the first pixel's sorted distinct values, so that
    samples lie on the first, on inner and on the last edge; column 0 cut by two values at either end, so that samples lie
    outside on both sides; n_bins = 1024: linspace over the column's range.  A constant column: +-1 around its value."""
    ndim = X.shape[2]
    edges = np.empty((ndim, n_bins + 1))
    for c in range(ndim):
        s = np.unique(X[0, :, c])
        if s.size == 1:
            edges[c] = np.linspace(s[0] - 1.0, s[0] + 1.0, n_bins + 1)
            continue
        assert s.size >= 12, (c, s.size)
        if c == 0:
            s = s[2:-2]
        if n_bins == 1024:
            lo, hi = (s[0], s[-1]) if c == 0 else (X[:, :, c].min(), X[:, :, c].max())
            edges[c] = np.linspace(lo, hi, n_bins + 1)
        else:
            edges[c] = s[np.round(np.linspace(0, s.size - 1, n_bins + 1)).astype(int)]
    return edges


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', list(CASES))
def test_histogram_equals_numpy(engine, mode, case):
    runner, dev, mask = _ensemble(engine, mode, case)
    theta, _ = dev.chain()
    P, n_keep, W, ndim = theta.shape
    N = n_keep * W
    assert N == {'48': 48, '1120': 1120, 'masked': 224}[case]
    X = theta.reshape(P, N, ndim)
    for n_bins in (1, 7, 1024):
        edges = _edges(X, n_bins)
        counts, outside = dev.histogram(edges)
        assert counts.shape == (P, ndim, n_bins) and counts.dtype == np.int64 and outside.shape == (P, ndim)
        for p in range(P):
            for c in range(ndim):
                assert np.array_equal(counts[p, c], np.histogram(X[p, :, c], bins=edges[c])[0]), (n_bins, p, c)
        assert np.array_equal(outside, N - counts.sum(axis=2))
        t_counts, t_outside = ensemble.pdf_counts(theta, edges)
        assert np.array_equal(counts, t_counts) and np.array_equal(outside, t_outside)
        # the construction did what it is for: samples outside on both sides of column 0, and on the edges of column 1
        assert (X[0, :, 0] < edges[0, 0]).sum() >= 2 and (X[0, :, 0] > edges[0, -1]).sum() >= 2 and outside[0, 0] >= 4
        if n_bins < 1024:
            assert (X[0, :, 1] == edges[1, 0]).any() and (X[0, :, 1] == edges[1, -1]).any() and outside[0, 1] == 0
        if n_bins == 7:
            assert (X[0, :, 1] == edges[1, 3]).any()
        const = np.flatnonzero((X == X[:, :1]).all(axis=(0, 1)))
        assert mask is None or set(np.flatnonzero(mask == 0)) <= set(const)
        for c in const:                                        # a slot that is not sampled: its N samples in one bin
            assert (counts[:, c].max(axis=1) == N).all() and (outside[:, c] == 0).all()
    dev.close()


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', list(CASES))
def test_covariance(engine, mode, case):
    runner, dev, mask = _ensemble(engine, mode, case)
    theta, lnL = dev.chain()
    P, n_keep, W, ndim = theta.shape
    N = n_keep * W
    cov = dev.covariance()
    assert cov.shape == (P, ndim, ndim)
    ref = ensemble.covariance_of(theta, lnL, LD)
    _, std, best, _, _ = dev.summary(())
    dmax = np.abs(theta.reshape(P, N, ndim).astype(LD) - best[:, None, :].astype(LD)).max(axis=1)
    bound = 8 * N * U * dmax[:, :, None] * dmax[:, None, :]
    err = np.abs(cov.astype(LD) - ref)
    live = bound > 0
    print(f'covariance {mode} {case} N={N}: off by {float(np.max((err / np.where(live, bound, 1))[live])):.3f} of its bound')
    assert np.all(err <= bound)
    assert np.array_equal(cov, np.swapaxes(cov, 1, 2))
    k = np.arange(ndim)
    assert np.array_equal(cov[:, k, k] > 0, dmax > 0) and (cov[:, k, k] >= 0).all()
    # the diagonal is the summary's variance, each within the summary's tolerance of the exact one
    assert np.all(np.abs(cov[:, k, k].astype(LD) - std.astype(LD) ** 2) <= 2 * 8 * N * U * dmax ** 2)
    const = np.flatnonzero((dmax == 0).all(axis=0))             # a slot that is not sampled: an exact zero row and column
    assert const.size >= (0 if mask is None else int(np.count_nonzero(mask == 0)))
    assert mask is None or set(np.flatnonzero(mask == 0)) <= set(const)
    for c in const:
        assert (cov[:, c, :] == 0).all() and (cov[:, :, c] == 0).all()
    dev.close()


def _same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and np.array_equal(a, b, equal_nan=True))


def _check_moments(runner, dev, chunks):
    """`dev.moments` against the host route over the fetched chain; the chain and the runner's likelihood are left as they were."""
    rng = np.random.default_rng(2)
    theta, lnL = dev.chain()
    P, n_keep, W, ndim = theta.shape
    N = n_keep * W
    rows = theta.reshape(P * N, ndim)
    probe = rng.uniform(size=(40, ndim))
    probe_pix = np.resize(dev.pix, 40) if dev.pix is not None else None
    loglike = lambda: runner.loglikelihood_batch(probe.copy()) if probe_pix is None else runner.loglikelihood_batch(probe_pix, probe.copy())
    before = loglike()
    for chunk in chunks:
        got = dev.moments(chunk_rows=chunk)
        if dev.pix is None:
            want = runner.predict_moments(rows)
        else:
            want = runner.predict_moments(dev.pix, np.arange(P + 1, dtype=np.int64) * N, rows, chunk_rows=chunk)
        for name in FIELDS:
            assert _same(getattr(got, name), getattr(want, name)), (chunk, name)
        assert got.mean.shape == (P, runner._ss.chan_tot) and np.isfinite(got.mean).all() and (got.std > 0).any()
        lean = dev.moments(chunk_rows=chunk, want_spectra=False)
        assert lean.mean is None and lean.std is None
        assert all(_same(getattr(lean, name), getattr(got, name)) for name in FIELDS[2:])
    after_theta, after_lnL = dev.chain()
    assert np.array_equal(after_theta, theta) and np.array_equal(after_lnL, lnL)
    assert np.array_equal(loglike(), before)


@pytest.mark.parametrize('mode', MODES)
def test_moments_equal_the_host_route(engine, mode):
    runner, dev, _ = _ensemble(engine, mode, '1120')           # segments of 1120 rows straddle the chunks of 64 and of 4096
    assert dev.n_keep == 7
    _check_moments(runner, dev, (64, None))
    dev.close()


@pytest.mark.parametrize('options', [{}, dict(layered=True)], ids=['plain', 'layered'])
def test_moments_of_two_components_with_pixels_out_of_order(engine, options):
    runner, dev, _ = _ensemble(engine, 'table', 'masked', **options)
    _check_moments(runner, dev, (64, None))
    dev.close()


def test_moments_of_a_one_pixel_runner(engine):
    axes, data, ut = _data(engine, 1, 1, seed=4)
    n = axes[0].size
    runner = engine.AmmoniaRunner.from_data([[axes[k], data[0, k * n:(k + 1) * n], NOISE, k + 1] for k in range(2)], ut, ncomp=1)
    dev = ensemble.DeviceEnsemble(runner, None, 16, ensemble.starts(runner, None, 16, n_init=256, seed=3))
    dev.run(12, 5, 1, 2.0, 1)
    _check_moments(runner, dev, (None,))
    dev.close()


@pytest.mark.parametrize('mode', MODES)
def test_same_arguments_same_bits(engine, mode):
    runner, dev, _ = _ensemble(engine, mode, '1120')
    theta, _ = dev.chain()
    edges = _edges(theta.reshape(2, -1, 6), 7)
    for call in (lambda: dev.histogram(edges), lambda: (dev.covariance(),), lambda: tuple(dev.moments(chunk_rows=64))):
        a, b = call(), call()
        assert len(a) == len(b) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))
    dev.close()


def test_errors_leave_runner_and_ensemble_usable(engine):
    runner = _runner(engine, 1, 2)
    pix = np.arange(2, dtype=np.int32)
    dev = ensemble.DeviceEnsemble(runner, pix, 16, ensemble.starts(runner, pix, 16, n_init=256, seed=3))
    E = engine.EngineError
    good = np.stack([np.linspace(-100.0, 100.0, 8)] * 6)
    for call in (lambda: dev.histogram(good), dev.covariance, dev.moments):
        with pytest.raises(E, match='no run yet'):
            call()
    dev.run(12, 5, 1, 2.0, 1)
    first = dev.summary((0.5,))
    with pytest.raises(E, match='NFA_ENS_MAX_BINS'):
        dev.histogram(np.zeros((6, 1)))                        # 0 bins
    with pytest.raises(E, match='NFA_ENS_MAX_BINS'):
        dev.histogram(np.stack([np.linspace(0.0, 1.0, 1026)] * 6))
    for k, value in ((3, good[2, 2]), (3, good[2, 1]), (7, np.nan), (0, -np.inf)):
        bad = good.copy()
        bad[2, k] = value
        with pytest.raises(E, match='increase strictly' if np.isfinite(value) else 'not finite'):
            dev.histogram(bad)
    with pytest.raises(ValueError):
        dev.histogram(good[:5])
    with pytest.raises(E, match='multiple of 64'):
        dev.moments(chunk_rows=100)
    again = dev.summary((0.5,))
    assert all(np.array_equal(x, y) for x, y in zip(first, again))
    counts, outside = dev.histogram(good)
    assert np.array_equal(counts.sum(axis=2) + outside, np.full((2, 6), 7 * 16))
    dev.run(6, 0, 1, 2.0, 2)                                   # a second run, and its products
    assert dev.chain()[0].shape == (2, 6, 16, 6) and dev.covariance().shape == (2, 6, 6) and dev.moments().mean.shape == (2, 192)
    dev.close()


def test_sample_pixels_and_sample_cube(engine, mode_guard):
    axes, data, ut = _data(engine, 1, 4, seed=4)
    data[1, 10] = np.nan                                       # pixel 1 = lon 0, lat 1 is not good
    engine.set_exp_mode('table')
    n_bins, W, n_keep = 9, 16, 8
    kw = dict(n_walkers=W, n_steps=40, n_burn=8, thin=4, seed=2, n_init=256, free_mask=ut.free_mask(1))
    products = dict(par_bins=n_bins, covariance=True, moments=True)
    one = ensemble.sample_cube(_stack(axes, data, 2, NOISE), ut, engine.AmmoniaRunner, 1, **products, **kw)
    lib = engine._ffi.load()
    per_pixel = lib.nfa_ensemble_bytes(1, W, 6, 5, 40, n_keep) + lib.nfa_ensemble_moments_bytes(1, 192, 2)
    two = ensemble.sample_cube(_stack(axes, data, 2, NOISE), ut, engine.AmmoniaRunner, 1, memory_budget=2 * per_pixel + 1, **products, **kw)
    assert one.n_groups == 1 and two.n_groups == 2
    shapes = dict(pdf_counts=(6, n_bins, 2, 2), pdf_outside=(6, 2, 2), cov=(6, 6, 2, 2), spec_mean=(192, 2, 2), spec_std=(192, 2, 2),
                  peak_mean=(2, 2, 2), peak_std=(2, 2, 2), total_mean=(2, 2, 2), total_std=(2, 2, 2), mean=(6, 2, 2))
    bad = np.zeros((2, 2), dtype=bool)
    bad[1, 0] = True
    for name, shape in shapes.items():
        a, b = getattr(one, name), getattr(two, name)
        assert a.shape == shape, name
        assert np.array_equal(a, b, equal_nan=True), name      # a pixel's products do not depend on its group
        if name.startswith('pdf'):
            assert a.dtype == np.int64 and (a[..., bad] == -1).all() and (a[..., ~bad] >= 0).all()
        else:
            assert np.isnan(a[..., bad]).all() and np.isfinite(a[..., ~bad]).all(), name
    assert one.pdf_bins.shape == (6, n_bins) and np.array_equal(one.pdf_bins, two.pdf_bins)
    edges = ensemble.bin_edges(ut, 1, n_bins)
    assert np.array_equal(one.pdf_bins, 0.5 * (edges[:, :-1] + edges[:, 1:]))
    total = one.pdf_counts.sum(axis=1) + one.pdf_outside
    assert (total[:, ~bad] == n_keep * W).all()
    # without the products the maps are what they were, and the new ones are absent
    plain = ensemble.sample_cube(_stack(axes, data, 2, NOISE), ut, engine.AmmoniaRunner, 1, **kw)
    assert np.array_equal(plain.mean, one.mean, equal_nan=True) and not hasattr(plain, 'cov') and not hasattr(plain, 'pdf_counts')

    # sample_pixels: the products outlive close(); the model is the host route's over the kept chain
    runner = _runner(engine, 1, 3)
    pix = np.array([2, 0], dtype=np.int32)
    res = runner.sample_posterior(pix, keep_chain=True, par_bins=n_bins, utrans=ut, covariance=True, moments=True, **kw)
    open_route = res.moments(runner, chunk_rows=64)
    res.close()
    assert res.pdf_counts.shape == (2, 6, n_bins) and res.pdf_outside.shape == (2, 6) and res.cov.shape == (2, 6, 6)
    assert np.array_equal(res.pdf_counts.sum(axis=2) + res.pdf_outside, np.full((2, 6), n_keep * W))
    t_counts, t_outside = ensemble.pdf_counts(res.theta, edges)
    assert np.array_equal(res.pdf_counts, t_counts) and np.array_equal(res.pdf_outside, t_outside)
    host = res.moments(runner)
    assert all(_same(getattr(res.model, name), getattr(host, name)) for name in FIELDS)
    host64 = res.moments(runner, chunk_rows=64)
    assert all(_same(getattr(open_route, name), getattr(host64, name)) for name in FIELDS)
    bare = runner.sample_posterior(pix, **kw)
    assert bare.pdf_counts is None and bare.pdf_outside is None and bare.pdf_bins is None and bare.cov is None and bare.model is None
    bare.close()
