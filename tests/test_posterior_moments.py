"""Weighted posterior moments of model spectra on the device (nfa_runner_predict_moments, nfa_runner_row_statistics;
DESIGN 4.21), in both numerical modes.

The reference of every comparison is longdouble numpy on the spectra the existing `predict_batch` returns for the same
rows (that code is pinned to the oracle elsewhere).  Tolerances are derived, not tuned.  With n rows in a segment,
u = 2^-53 and d_i = p_i - p_i* the rows about the segment's row of largest weight:

    |mean - ref|  <= 8 n u max_i |d_i[j]|  +  u |ref|
    |std^2 - ref| <= 8 n u max_i d_i[j]^2
    total within 8 n_chan u sum |p| of the NaN-ignoring sum;  peak bit for bit (a maximum rounds nothing)

The first term of the mean's bound is the error of S1 / S0 (n products and sums, each within u); the second is the
rounding of the result itself, p_i* + S1 / S0 stored as a double, which no f64 output can be without and which is the
larger one wherever the posterior is tight.  The moments of the totals carry the totals' own error e = max_i 8 n_chan u
sum |p_i| as well: 2 e on every d, so 2 e on the mean and 4 e max |d| + 4 e^2 on std^2."""
import numpy as np
import pytest

from test_sibling_models import MODES, n2hp_axis

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
LD = np.longdouble
SIZES = (1, 2, 63, 64, 65, 200, 0, 5)               # the last segment: all weights 0
OFFSETS = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)


def _reference(x, w, off):
    """Per segment (mean, var, max |d|, n) of the columns of x in longdouble, None where NaN is due.  Two passes over d, the
    rows about the row of largest weight (d is exact in longdouble, so one row gives var = 0 exactly)."""
    out = []
    for g in range(len(off) - 1):
        xs, ws = np.asarray(x[off[g]:off[g + 1]], dtype=LD), np.asarray(w[off[g]:off[g + 1]], dtype=LD)
        if xs.shape[0] == 0 or not ws.sum() > 0:
            out.append(None)
            continue
        top = xs[np.argmax(ws)]
        d = xs - top
        m1 = (ws[:, None] * d).sum(axis=0) / ws.sum()
        var = (ws[:, None] * (d - m1) ** 2).sum(axis=0) / ws.sum()
        out.append((top + m1, var, np.abs(d).max(axis=0), xs.shape[0]))
    return out


def _check(mean, std, x, w, off, err=0.0):
    """mean, std [n_seg, n_col] of the device against the columns of x within the bounds above; err: the error every entry
    of x may carry itself (the totals')."""
    for g, ref in enumerate(_reference(x, w, off)):
        if ref is None:
            assert np.isnan(mean[g]).all() and np.isnan(std[g]).all(), g
            continue
        rmean, rvar, d, n = ref
        dm = np.abs(mean[g].astype(LD) - rmean)
        tol = 8 * n * U * d + U * np.abs(rmean) + 2 * err
        assert np.all(dm <= tol), (g, float(np.max(dm / np.maximum(tol, LD(1e-300)))))
        dv = np.abs(std[g].astype(LD) ** 2 - rvar)
        tol = 8 * n * U * d * d + 4 * err * d + 4 * err * err
        assert np.all(dv <= tol), (g, float(np.max(dv / np.maximum(tol, LD(1e-300)))))
        assert np.all(std[g] >= 0)


def _check_all(res, spec, w, off, spec_off, signed=False):
    """A `PosteriorMoments` record against `predict_batch`'s spectra of the same rows."""
    from nestfit_amd._model import signed_peak
    w = np.ones(spec.shape[0]) if w is None else w
    _check(res.mean, res.std, spec, w, off)
    top = signed_peak if signed else np.nanmax
    n_spec = len(spec_off) - 1
    peak = np.stack([top(spec[:, spec_off[k]:spec_off[k + 1]], axis=1) for k in range(n_spec)], axis=1)
    total = np.stack([np.nansum(spec[:, spec_off[k]:spec_off[k + 1]].astype(LD), axis=1) for k in range(n_spec)], axis=1)
    _check(res.peak_mean, res.peak_std, peak, w, off)
    err = max(8 * (spec_off[k + 1] - spec_off[k]) * U * np.abs(spec[:, spec_off[k]:spec_off[k + 1]]).sum(axis=1).max() for k in range(n_spec))
    _check(res.total_mean, res.total_std, total, w, off, err=err)


def _same_bits(a, b):
    return all((x is None and y is None) or np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def _jitter(rng, truth, rows, scale):
    return np.ascontiguousarray(truth * (1.0 + scale * rng.normal(size=(rows, truth.size))))


@pytest.fixture(scope='module')
def shapes(engine):
    """Ammonia, two spectra of 70 and 129 channels (chan_tot = 199), two components, three pixels; the rows of SIZES."""
    from nestfit_amd.cube import CubeRunner
    from nestfit_amd.synth import TRUTH_2COMP, freq_axis
    rng = np.random.default_rng(21)
    axes = [freq_axis(1, 70, 20.0), freq_axis(2, 129, 20.0)]
    runner = CubeRunner(axes, (1, 2), rng.normal(0, 0.2, (3, 199)), np.full((3, 2), 0.2), None, ncomp=2)
    rows = int(OFFSETS[-1])
    theta = _jitter(rng, TRUTH_2COMP, rows, 0.03)
    w = rng.uniform(0.0, 1.0, rows)
    w[rng.uniform(size=rows) < 0.15] = 0.0
    w[0] = 0.7                                                         # the one-row segment keeps a weight
    w[OFFSETS[-2]:] = 0.0
    seg_pix = (np.arange(len(SIZES)) % 3).astype(np.int32)
    return runner, seg_pix, theta, w


@pytest.mark.parametrize('mode', MODES)
def test_shapes(shapes, mode):
    runner, seg_pix, theta, w = shapes
    runner.set_exp_mode(mode)
    assert runner.n_chan_tot == 199 and np.sum(w == 0) > 10
    spec, _ = runner.predict_batch(np.repeat(seg_pix, np.diff(OFFSETS)), theta)
    res = runner.predict_moments(seg_pix, OFFSETS, theta, w, chunk_rows=64)
    assert res.mean.shape == res.std.shape == (8, 199) and res.peak_mean.shape == res.total_std.shape == (8, 2)
    _check_all(res, spec, w, OFFSETS, [0, 70, 199])
    for g in (6, 7):                                                   # the empty and the all-zero-weight segments, and no other
        assert all(np.isnan(a[g]).all() for a in res)
    assert all(np.isfinite(a[:6]).all() for a in res)
    assert np.all(res.std[0] == 0) and np.all(res.peak_std[0] == 0) and np.all(res.total_std[0] == 0)       # one row
    assert np.array_equal(res.mean[0], spec[0])
    assert _same_bits(res, runner.predict_moments(seg_pix, OFFSETS, theta, w, chunk_rows=64))
    _check_all(runner.predict_moments(seg_pix, OFFSETS, theta, w, chunk_rows=4096), spec, w, OFFSETS, [0, 70, 199])
    _check_all(runner.predict_moments(seg_pix, OFFSETS, theta, w), spec, w, OFFSETS, [0, 70, 199])
    ones = runner.predict_moments(seg_pix, OFFSETS, theta, None, chunk_rows=64)
    assert _same_bits(ones, runner.predict_moments(seg_pix, OFFSETS, theta, np.ones(theta.shape[0]), chunk_rows=64))
    _check_all(ones, spec, None, OFFSETS, [0, 70, 199])
    only_stats = runner.predict_moments(seg_pix, OFFSETS, theta, w, chunk_rows=64, want_spectra=False)
    assert only_stats.mean is None and _same_bits(only_stats[2:], res[2:])
    none = runner.predict_moments(np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros((0, 12)))
    assert none.mean.shape == (0, 199)                                 # n_seg = 0: a no-op


@pytest.mark.parametrize('mode', MODES)
def test_tight_posterior(shapes, mode):
    """Rows whose spectra differ by about 1e-7 relative: the bound in d holds and std has 1e-6 relative, where raw second
    moments in float64 would have no digit."""
    from nestfit_amd.synth import TRUTH_2COMP
    runner = shapes[0]
    runner.set_exp_mode(mode)
    rng = np.random.default_rng(8)
    theta = _jitter(rng, TRUTH_2COMP, 150, 1e-7)
    w = rng.uniform(0.1, 1.0, 150)
    off = np.array([0, 150], dtype=np.int64)
    pix = np.zeros(1, np.int32)
    spec, _ = runner.predict_batch(np.zeros(150, np.int32), theta)
    res = runner.predict_moments(pix, off, theta, w, chunk_rows=64)
    _check_all(res, spec, w, off, [0, 70, 199])
    _, rvar, _, _ = _reference(spec, w, off)[0]
    rstd = np.sqrt(rvar).astype(np.float64)
    big = rstd > 1e-9 * np.abs(spec[0]).max()                          # channels where the line is
    assert big.sum() > 20
    assert np.max(np.abs(res.std[0][big] / rstd[big] - 1.0)) <= 1e-6
    assert np.max(rstd[big] / np.abs(spec[0])[big]) < 1e-5             # tight it is


def _small_case(runner, rng, truth, n_pix, scale=0.03, signed=False, spec_off=None):
    sizes = (3, 70, 0, 9)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    theta = _jitter(rng, truth, int(off[-1]), scale)
    w = rng.uniform(0.0, 1.0, int(off[-1]))
    w[::5] = 0.0
    seg_pix = (np.array([1, 0, 0, 2]) % n_pix).astype(np.int32)
    spec, _ = runner.predict_batch(np.repeat(seg_pix, np.diff(off)), theta)
    res = runner.predict_moments(seg_pix, off, theta, w, chunk_rows=64)
    _check_all(res, spec, w, off, spec_off, signed=signed)
    assert np.isnan(res.mean[2]).all() and np.isfinite(res.mean[[0, 1, 3]]).all()
    return res, spec, seg_pix, off, theta, w


@pytest.mark.parametrize('mode', MODES)
def test_set_forms(engine, mode):
    """A channel response, layered N2H+ and a continuum that differs from pixel to pixel: the moments are those of
    `predict_batch`'s spectra of the same set."""
    from nestfit_amd import HANNING_RESPONSE
    from nestfit_amd._model import signed_peak
    from nestfit_amd.cube import CubeRunner
    from nestfit_amd.synth import TRUTH_2COMP, freq_axis
    rng = np.random.default_rng(33)
    axes = [freq_axis(1, 70, 20.0), freq_axis(2, 129, 20.0)]
    data, noise = rng.normal(0, 0.2, (2, 199)), np.full((2, 2), 0.2)
    plain = CubeRunner(axes, (1, 2), data, noise, None, ncomp=2)
    smooth = CubeRunner(axes, (1, 2), data, noise, None, ncomp=2, response=HANNING_RESPONSE)
    for r in (plain, smooth):
        r.set_exp_mode(mode)
    res, spec, seg_pix, off, theta, w = _small_case(smooth, np.random.default_rng(1), TRUTH_2COMP, 2, spec_off=[0, 70, 199])
    assert not np.array_equal(spec, plain.predict_batch(np.repeat(seg_pix, np.diff(off)), theta)[0])     # the filtered form it is

    n2hp = np.array([-1.0, 1.2, 9.0, 6.0, 0.6, 1.2, 0.4, 0.5])         # voff, tex, ltau, sigm of two layers, the front one over the back
    layered = CubeRunner([n2hp_axis(1, 150)], (1,), rng.normal(0, 0.2, (2, 150)), np.full((2, 1), 0.2), None, ncomp=2, model=1,
                         layered=True)
    summed = CubeRunner([n2hp_axis(1, 150)], (1,), rng.normal(0, 0.2, (2, 150)), np.full((2, 1), 0.2), None, ncomp=2, model=1)
    for r in (layered, summed):
        r.set_exp_mode(mode)
    res, spec, seg_pix, off, theta, w = _small_case(layered, np.random.default_rng(2), n2hp, 2, spec_off=[0, 150])
    assert not np.array_equal(spec, summed.predict_batch(np.repeat(seg_pix, np.diff(off)), theta)[0])

    tc = np.array([[30.0, 28.0], [0.0, 0.0], [3.0, 12.5]])             # a row per pixel; pixel 0 absorbs
    cont = CubeRunner(axes, (1, 2), rng.normal(0, 0.2, (3, 199)), np.full((3, 2), 0.2), None, ncomp=2, continuum=tc)
    cont.set_exp_mode(mode)
    res, spec, seg_pix, off, theta, w = _small_case(cont, np.random.default_rng(3), TRUTH_2COMP, 3, signed=True, spec_off=[0, 70, 199])
    pix = np.repeat(seg_pix, np.diff(off))
    peak, total = cont.row_statistics(pix, theta)
    want = np.stack([signed_peak(spec[:, :70], axis=1), signed_peak(spec[:, 70:], axis=1)], axis=1)
    assert np.array_equal(peak, want) and np.any(peak < 0) and np.any(peak > 0)          # the signed peak, bit for bit
    other = cont.predict_moments(np.roll(seg_pix, 1), off, theta, w, chunk_rows=64)      # seg_pix matters
    assert not np.array_equal(other.mean[1], res.mean[1])


def test_against_the_oracle(engine, nfo):
    """One segment of 32 rows of TRUTH_2COMP jittered by 1 %: the mean against longdouble moments of the oracle's spectra,
    within what test_postprocess.py::test_postprocess_on_device allows device spectra in table mode."""
    from nestfit_amd.cube import CubeRunner
    from nestfit_amd.synth import TRUTH_2COMP, freq_axis
    rng = np.random.default_rng(17)
    axes = [freq_axis(1, 96, 20.0), freq_axis(2, 96, 20.0)]
    runner = CubeRunner(axes, (1, 2), np.zeros((1, 192)), np.ones((1, 2)), None, ncomp=2)
    runner.set_exp_mode('table')
    theta = _jitter(rng, TRUTH_2COMP, 32, 0.01)
    w = rng.uniform(0.1, 1.0, 32)
    oracle = []
    for th in theta:
        row = []
        for x, t in zip(axes, (1, 2)):
            s = nfo.AmmoniaSpectrum(x, np.zeros(96), 1.0, t)
            nfo.amm_predict(s, np.ascontiguousarray(th))
            row.append(s.get_spec())
        oracle.append(np.concatenate(row))
    rmean, rvar, _, _ = _reference(np.array(oracle), w, [0, 32])[0]
    res = runner.predict_moments(np.zeros(1, np.int32), np.array([0, 32]), theta, w)
    np.testing.assert_allclose(res.mean[0], rmean.astype(np.float64), rtol=2e-7, atol=1e-30)
    np.testing.assert_allclose(res.std[0], np.sqrt(rvar).astype(np.float64), rtol=2e-7, atol=1e-30)
    one = engine.AmmoniaRunner.from_data([[x, np.zeros(96), 1.0, t] for x, t in zip(axes, (1, 2))], None, ncomp=2)
    one.set_exp_mode('table')
    single = one.predict_moments(theta, w)                             # the single-pixel runner: the same segment
    assert _same_bits(single, res)
    peak, total = one.row_statistics(theta)
    assert np.array_equal(peak, runner.row_statistics(np.zeros(32, np.int32), theta)[0])


@pytest.mark.parametrize('mode', MODES)
def test_row_statistics_and_refused_requests(shapes, engine, mode):
    runner, seg_pix, theta, w = shapes
    runner.set_exp_mode(mode)
    th = theta[:130]
    pix = (np.arange(130) % 3).astype(np.int32)
    peak, total = runner.row_statistics(pix, th)
    want_peak, want_total = runner.peak_and_integrated(pix, th)
    spec, _ = runner.predict_batch(pix, th)
    assert np.array_equal(peak, want_peak)
    for k, sl in enumerate((slice(0, 70), slice(70, 199))):
        ref = np.nansum(spec[:, sl].astype(LD), axis=1)
        bound = 8 * (sl.stop - sl.start) * U * np.abs(spec[:, sl]).sum(axis=1)
        assert np.all(np.abs(total[:, k].astype(LD) - ref) <= bound)
        assert np.all(np.abs(total[:, k] - want_total[:, k]) <= 2 * bound)

    def refused(words, *args, **kw):
        with pytest.raises(engine.EngineError) as e:
            runner.predict_moments(*args, **kw)
        assert words in str(e.value), str(e.value)
    off = np.array([0, 5, 10], dtype=np.int64)
    two = np.zeros(2, np.int32)
    bad_w = np.ones(10); bad_w[3] = -0.5
    refused('weight', two, off, theta[:10], bad_w)
    bad_w[3] = np.inf
    refused('weight', two, off, theta[:10], bad_w)
    refused('decrease', np.zeros(3, np.int32), np.array([0, 7, 5, 10]), theta[:10])
    refused('multiple of 64', two, off, theta[:10], chunk_rows=100)
    refused('pixel', np.array([0, 3], np.int32), off, theta[:10])
    with pytest.raises(engine.EngineError) as e:
        runner.row_statistics(np.full(4, -1, np.int32), theta[:4])
    assert 'pixel' in str(e.value)
    from nestfit_amd import _ffi
    rc = _ffi.load().nfa_runner_predict_moments(runner._run.handle, 2, None, off.ctypes.data_as(_ffi._lp), _ffi.dptr(theta), None, 0,
                                                None, None, None, None)
    assert rc != 0 and b'outputs' in _ffi.load().nfa_last_error()
    res = runner.predict_moments(two, off, theta[:10])                 # and the runner is as good as before
    assert np.isfinite(res.mean).all()


def test_whole_store_on_the_device(engine, tmp_path):
    """`generate_posterior_profiles` on the `fitted` store of test_postprocess.py: the device route equals the
    `predict_backend` route (the oracle's spectra, the numpy twin's moments) within the tolerance of
    test_against_the_oracle."""
    from nestfit_amd import postprocess as pp
    from nestfit_amd.store import HdfStore
    from test_fitter_cpu import _fitter, _stack
    from test_posterior_profiles_cpu import NEW, OracleBackend
    stack = _stack(n_lon=4, n_lat=2, seed=4)
    path = str(tmp_path / 'run')
    _fitter(stack).fit_cube(path, nproc=2)

    def read(store):
        prod = store.hdf['/products']
        out = {k: np.array(prod[k][...]) for k in NEW[2:]}
        for kind in ('mean', 'std'):
            for t in (1, 2):
                out[f'{kind}{t}'] = np.array(prod[f'model_spec_{kind}'][f'trans{t}'][...])
        return out
    with HdfStore(path) as store:
        pp.aggregate_run_attributes(store); pp.convolve_evidence(store, 0.6); pp.aggregate_run_products(store)
        pp.generate_posterior_profiles(store, stack)
        dev = read(store)
        pp.generate_posterior_profiles(store, stack, predict_backend=OracleBackend(stack))
        cpu = read(store)
    assert np.isfinite(dev['mean1']).sum() >= 2 * 96 and np.isfinite(dev['peak_intensity_std']).sum() >= 4
    for k in dev:
        np.testing.assert_allclose(dev[k], cpu[k], rtol=2e-7, atol=1e-30, equal_nan=True, err_msg=k)
