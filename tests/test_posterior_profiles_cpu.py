"""`postprocess.generate_posterior_profiles` without a GPU: the store of test_postprocess.py's `fitted`
recipe, the oracle predictor as `predict_backend`, so the moments are formed by the numpy twin (nestfit_amd/moments.py).
Every product is compared with a plain per-pixel longdouble loop over the stored posteriors."""
import numpy as np
import pytest

from nestfit_amd import postprocess as pp
from nestfit_amd.store import HdfStore

from test_fitter_cpu import N_CHAN, _fitter, _stack

NEW = ('model_spec_mean', 'model_spec_std', 'peak_intensity_mean', 'peak_intensity_std', 'integrated_intensity_mean',
       'integrated_intensity_std')
N_LON, N_LAT, N_MAX = 4, 2, 2


class OracleBackend:
    """predict_backend of the oracle: theta[B, 6 n] (parameter-major) -> spectra, or peak and total per cube."""

    def __init__(self, stack):
        from oracle import nfo
        self.nfo, self.stack = nfo, stack
        self.spectra = [nfo.AmmoniaSpectrum(dc.xarr, np.zeros(dc.nchan), 1.0, dc.trans_id) for dc in stack.cubes]

    def row(self, th):
        out = []
        for s in self.spectra:
            self.nfo.amm_predict(s, np.ascontiguousarray(th, dtype=np.float64))
            out.append(s.get_spec())
        return out

    def __call__(self, lon, lat, theta, want_spectra):
        rows = [self.row(th) for th in theta]
        if want_spectra:
            return np.array([np.concatenate(r) for r in rows]).reshape(len(rows), -1), None, None
        peak = np.array([[np.nanmax(c) for c in r] for r in rows]).reshape(len(rows), -1)
        tot = np.array([[np.nansum(c) for c in r] for r in rows]).reshape(len(rows), -1)
        return None, peak, tot


def _ld_moments(x, w):
    """Weighted mean and std of the rows of x in longdouble, two passes."""
    x, w = np.asarray(x, dtype=np.longdouble), np.asarray(w, dtype=np.longdouble)
    mean = (w[:, None] * x).sum(axis=0) / w.sum()
    var = (w[:, None] * (x - mean) ** 2).sum(axis=0) / w.sum()
    return mean, np.sqrt(var)


@pytest.fixture(scope='module')
def products(tmp_path_factory):
    stack = _stack(n_lon=N_LON, n_lat=N_LAT, seed=4)
    path = str(tmp_path_factory.mktemp('postprof') / 'run')
    _fitter(stack).fit_cube(path, nproc=2)
    backend = OracleBackend(stack)
    with HdfStore(path) as store:
        pp.postprocess_run(store, stack, evid_kernel=0.6, post_kernel=pp.gaussian_kernel(0.6), predict_backend=backend)
        before = sorted(store.hdf['/products'])
        pp.generate_posterior_profiles(store, stack, predict_backend=backend)
        prod = store.hdf['/products']
        out = {k: np.array(prod[k][...]) for k in NEW[2:]}
        for kind in ('mean', 'std'):
            out[f'model_spec_{kind}'] = [np.array(prod[f'model_spec_{kind}'][f'trans{t}'][...]) for t in (1, 2)]
        out['conv_nbest'] = np.array(prod['conv_nbest'][...])
        out['posteriors'] = {}
        for g in store.iter_pix_groups():
            l, b = int(g.attrs['i_lon']), int(g.attrs['i_lat'])
            n = int(out['conv_nbest'][b, l])
            if n > 0:
                out['posteriors'][(l, b)] = (n, np.asarray(g[f'{n}']['posteriors'][...], dtype=np.float64))
        pp.generate_posterior_profiles(store, stack, thin=1.0, predict_backend=backend)
        out['thin'] = {kind: [np.array(prod[f'model_spec_{kind}'][f'trans{t}'][...]) for t in (1, 2)] for kind in ('mean', 'std')}
        out['thin_stats'] = {k: np.array(prod[k][...]) for k in NEW[2:]}
    return stack, backend, before, out


def test_postprocess_run_without_the_keyword_writes_none_of_them(products):
    _, _, before, _ = products
    assert 'model_spec' in before and 'peak_intensity' in before
    assert not set(before) & set(NEW)


def test_all_six_products_in_their_shapes(products):
    _, _, _, out = products
    for kind in ('mean', 'std'):
        assert all(c.shape == (N_CHAN, N_LAT, N_LON) and c.dtype == np.float32 for c in out[f'model_spec_{kind}'])
    for k in NEW[2:]:
        assert out[k].shape == (2, N_MAX, N_LAT, N_LON) and out[k].dtype == np.float64
    assert len(out['posteriors']) >= 2


def test_products_equal_a_longdouble_loop_over_the_posteriors(products):
    stack, backend, _, out = products
    dv = [dc.dv for dc in stack.cubes]
    seen_two = 0
    for b in range(N_LAT):
        for l in range(N_LON):
            if (l, b) not in out['posteriors']:                       # a pixel without components (or without data)
                for kind in ('mean', 'std'):
                    assert all(np.isnan(c[:, b, l]).all() for c in out[f'model_spec_{kind}'])
                assert all(np.isnan(out[k][:, :, b, l]).all() for k in NEW[2:])
                continue
            n, post = out['posteriors'][(l, b)]
            seen_two += n == 2
            w = post[:, -1]
            keep = w > 0
            theta, w = post[keep, :-2], w[keep]
            whole = [backend.row(th) for th in theta]
            for t in range(2):
                mean, std = _ld_moments([r[t] for r in whole], w)
                np.testing.assert_allclose(out['model_spec_mean'][t][:, b, l], mean.astype(np.float64), rtol=1e-6, atol=1e-30)
                np.testing.assert_allclose(out['model_spec_std'][t][:, b, l], std.astype(np.float64), rtol=1e-6, atol=1e-30)
            for c in range(n):
                alone = [backend.row(th[c::n]) for th in theta]
                for t in range(2):
                    pm, ps = _ld_moments([[np.max(r[t])] for r in alone], w)
                    tm, ts = _ld_moments([[np.sum(r[t].astype(np.longdouble))] for r in alone], w)
                    got = [out[k][t, c, b, l] for k in NEW[2:]]
                    want = [pm[0], ps[0], tm[0] * dv[t], ts[0] * abs(dv[t])]
                    np.testing.assert_allclose(got, np.array(want, dtype=np.float64), rtol=1e-10)
            assert all(np.isnan(out[k][:, n:, b, l]).all() for k in NEW[2:])
    assert seen_two >= 1 or N_MAX == 1 or all(n == 1 for n, _ in out['posteriors'].values())


def test_thin_of_one_leaves_the_row_of_largest_weight(products):
    stack, backend, _, out = products
    for (l, b), (n, post) in out['posteriors'].items():
        top = post[np.argmax(post[:, -1])]
        assert np.sum(post[:, -1] == top[-1]) == 1                    # (no tie for the largest weight in this store)
        spec = backend.row(top[:-2])
        for t in range(2):
            assert np.array_equal(out['thin']['mean'][t][:, b, l], spec[t].astype(np.float32))
            assert np.all(out['thin']['std'][t][:, b, l] == 0)
        for c in range(n):
            alone = backend.row(top[:-2][c::n])
            for t in range(2):
                assert out['thin_stats']['peak_intensity_mean'][t, c, b, l] == np.max(alone[t])
                assert out['thin_stats']['peak_intensity_std'][t, c, b, l] == 0
                assert out['thin_stats']['integrated_intensity_std'][t, c, b, l] == 0


def test_twin_keeps_the_std_of_a_tight_posterior():
    """Rows whose spectra differ by 1e-7 relative: the std of the twin agrees with longdouble to 1e-6 relative, where raw
    second moments (sum w p^2 / S0 - mean^2 in float64) have no correct digit."""
    from nestfit_amd.moments import moments_of
    rng = np.random.default_rng(11)
    base = rng.uniform(0.5, 3.0, size=37)
    x = base * (1.0 + 1e-7 * rng.normal(size=(50, 37)))
    w = rng.uniform(0.0, 1.0, size=50)
    w[::7] = 0.0
    off = np.array([0, 50])
    mean, std = moments_of(x, w, off)
    ref_mean, ref_std = _ld_moments(x, w)
    assert np.max(np.abs(std[0] / ref_std.astype(np.float64) - 1.0)) <= 1e-6
    assert np.max(np.abs(mean[0] / ref_mean.astype(np.float64) - 1.0)) <= 4e-16
    raw = np.sqrt(np.maximum((w[:, None] * x * x).sum(axis=0) / w.sum() - ((w[:, None] * x).sum(axis=0) / w.sum()) ** 2, 0))
    assert np.max(np.abs(raw / ref_std.astype(np.float64) - 1.0)) > 1e-3          # what the rule is for


def test_twin_edges_and_row_statistics():
    from nestfit_amd._model import signed_peak
    from nestfit_amd.moments import moments_of, posterior_moments_of, row_statistics_of
    rng = np.random.default_rng(2)
    x = rng.normal(size=(10, 9))
    w = rng.uniform(0.1, 1.0, size=10)
    w[4:7] = 0.0                                                       # segment 2: all weights 0
    off = np.array([0, 1, 4, 7, 7, 10])                                # 1, 3, 3 (weightless), 0 and 3 rows
    mean, std = moments_of(x, w, off)
    assert np.array_equal(mean[0], x[0]) and np.all(std[0] == 0)       # one row
    assert np.isnan(mean[2]).all() and np.isnan(std[2]).all() and np.isnan(mean[3]).all() and np.isnan(std[3]).all()
    for g in (1, 4):
        rm, rs = _ld_moments(x[off[g]:off[g + 1]], w[off[g]:off[g + 1]])
        np.testing.assert_allclose(mean[g], rm.astype(np.float64), rtol=1e-14)
        np.testing.assert_allclose(std[g], rs.astype(np.float64), rtol=1e-13)
    m1, s1 = moments_of(x, None, off)
    m2, s2 = moments_of(x, np.ones(10), off)
    assert np.array_equal(m1, m2, equal_nan=True) and np.array_equal(s1, s2, equal_nan=True)
    x[0, 2] = np.nan
    peak, tot = row_statistics_of(x, [0, 4, 9])
    assert peak.shape == (10, 2) and peak[0, 0] == np.nanmax(x[0, :4]) and tot[3, 1] == np.nansum(x[3, 4:])
    speak, _ = row_statistics_of(x, [0, 4, 9], signed=True)
    assert np.array_equal(speak[:, 1], signed_peak(x[:, 4:], axis=1)) and np.any(speak < 0)
    rec = posterior_moments_of(x[1:], w[1:], off[1:] - 1, [0, 4, 9], want_spectra=False)
    assert rec.mean is None and rec.peak_mean.shape == (4, 2) and rec.total_std.shape == (4, 2)
    with pytest.raises(ValueError):
        moments_of(x, -w, off)
    with pytest.raises(ValueError):
        moments_of(x, w, [0, 5, 3, 10])
