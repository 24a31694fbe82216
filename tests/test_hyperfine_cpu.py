"""The hyperfine model of caller-supplied line tables (nestfit_amd/hyperfine.py) without a GPU: the numpy restatement the
GPU tests compare against (tests/hf_restatement.py) pinned to the oracle, `LineTable`, the module's metadata, and the cube
driver, the store and the map products with stand-ins for the device (the way tests/test_fitter_cpu.py does it)."""
import json
from pathlib import Path

import numpy as np
import pytest

import hf_restatement as hfr

LITERALS = Path(__file__).resolve().parent / 'golden' / 'reference_literals.json'
N2HP_NU = {1: 93173.7637e6, 2: 186344.8420e6, 3: 279511.8325e6}


def n2hp_axis(trans, n, vhalf=20.0):
    v = np.linspace(vhalf, -vhalf, n)
    return N2HP_NU[trans] * (1.0 - v / hfr.CKMS)


def draw_params(rng, ncomp):
    """The ranges tests/test_sibling_models.py draws N2H+ parameters from."""
    return np.concatenate([rng.uniform(-8, 8, ncomp), rng.uniform(2.8, 25, ncomp),
                           rng.uniform(-2, 1.5, ncomp), 10 ** rng.uniform(-1.3, 0.3, ncomp)])


def test_restatement_equals_the_oracle_on_the_n2hp_tables(nfo):
    """3 transitions x 256 / 1024 channels x 40 draws of 1-3 components: 240 of 240 bit for bit, none left out."""
    ref = json.loads(LITERALS.read_text())['n2hp']
    rng = np.random.default_rng(20)
    n_cases = 0
    for trans in (1, 2, 3):
        table = (ref['NU'][trans - 1], np.array(ref['VOFF'][trans - 1]), np.array(ref['TAU_WTS'][trans - 1]))
        for n in (256, 1024):
            x = n2hp_axis(trans, n)
            sc = nfo.DiazenyliumSpectrum(x, np.zeros(n), 0.1, trans)
            tbg = hfr.tbg_of(nfo, x)
            assert np.array_equal(tbg, sc.tbg_arr)
            for _ in range(40):
                th = draw_params(rng, int(rng.integers(1, 4)))
                nfo.nnhp_predict(sc, th)
                got = hfr.hf_predict(nfo, x, tbg, table, th)
                assert np.array_equal(got, sc.get_spec()), (trans, n, th)
                lo, hi = hfr.hf_windows(x, table, th[0], th[-1])
                clo, chi = sc.hf_windows(th[0], th[-1])
                assert np.array_equal(lo, clo) and np.array_equal(hi, chi)
                n_cases += 1
    assert n_cases == 240


# ---------------------------------------------------------------------------- LineTable
BAD_TABLES = [
    ('no line', dict(nu=1e11, voff=[], tau_wts=[]), '1..50 lines'),
    ('51 lines', dict(nu=1e11, voff=np.linspace(-5, 5, 51), tau_wts=np.ones(51)), '1..50 lines'),
    ('lengths differ', dict(nu=1e11, voff=[0.0, 1.0], tau_wts=[1.0]), 'one length'),
    ('nu zero', dict(nu=0.0, voff=[0.0], tau_wts=[1.0]), 'rest frequency'),
    ('nu negative', dict(nu=-1e11, voff=[0.0], tau_wts=[1.0]), 'rest frequency'),
    ('nu inf', dict(nu=np.inf, voff=[0.0], tau_wts=[1.0]), 'rest frequency'),
    ('nu nan', dict(nu=np.nan, voff=[0.0], tau_wts=[1.0]), 'rest frequency'),
    ('offset nan', dict(nu=1e11, voff=[0.0, np.nan], tau_wts=[1.0, 1.0]), 'velocity offset'),
    ('offset inf', dict(nu=1e11, voff=[np.inf], tau_wts=[1.0]), 'velocity offset'),
    ('offset c', dict(nu=1e11, voff=[hfr.CKMS], tau_wts=[1.0]), 'velocity offset'),
    ('offset -c', dict(nu=1e11, voff=[-hfr.CKMS], tau_wts=[1.0]), 'velocity offset'),
    ('weight negative', dict(nu=1e11, voff=[0.0, 1.0], tau_wts=[1.0, -0.1]), 'weight'),
    ('weight nan', dict(nu=1e11, voff=[0.0], tau_wts=[np.nan]), 'weight'),
    ('weight inf', dict(nu=1e11, voff=[0.0], tau_wts=[np.inf]), 'weight'),
    ('weights zero', dict(nu=1e11, voff=[0.0, 1.0], tau_wts=[0.0, 0.0]), 'all zero'),
]


@pytest.mark.parametrize('what,kw,msg', BAD_TABLES, ids=[b[0] for b in BAD_TABLES])
def test_line_table_rejects(what, kw, msg, monkeypatch):
    """ValueError on the host, before any device call: the engine's loader is made to fail the test if it is reached."""
    from nestfit_amd import _ffi, hyperfine

    def no_device():
        raise AssertionError('a device call before the table was checked')
    monkeypatch.setattr(_ffi, 'engine', no_device)
    with pytest.raises(ValueError, match=msg):
        hyperfine.LineTable(**kw)
    # ... and through the classes that take a table: the table is built first
    x = np.linspace(1e11, 1.0001e11, 64)
    with pytest.raises(ValueError, match=msg):
        hyperfine.HyperfineSpectrum(x, np.zeros(64), 0.1, hyperfine.LineTable(**kw))
    with pytest.raises(ValueError, match='must be a LineTable'):
        hyperfine.HyperfineSpectrum(x, np.zeros(64), 0.1, (1e11, [0.0], [1.0]))


def test_line_table_is_immutable_and_compares_by_value():
    from nestfit_amd import LineTable
    t = LineTable(1e11, [0.5, -0.5, 0.0], [0.2, 0.3, 0.5], name='x')
    assert (t.nu, t.n, len(t), t.name) == (1e11, 3, 3, 'x')
    with pytest.raises(AttributeError):
        t.nu = 2e11
    with pytest.raises(ValueError):
        t.voff[0] = 1.0
    with pytest.raises(ValueError):
        t.tau_wts[0] = 1.0
    src = np.array([0.5, -0.5, 0.0])
    t2 = LineTable(1e11, src, [0.2, 0.3, 0.5])
    src[0] = 9.0                                             # the table keeps its own copy
    assert t2 == t and hash(t2) == hash(t) and t2.voff[0] == 0.5
    assert t != LineTable(1e11, [0.5, -0.5, 0.0], [0.2, 0.3, 0.6])
    assert t != LineTable(1e11, [-0.5, 0.5, 0.0], [0.3, 0.2, 0.5])      # the same lines in another order: another table
    # weights are used as given: not normalised
    assert LineTable(1e11, [0.0], [7.0]).tau_wts[0] == 7.0
    # one line of weight zero among others is fine
    assert LineTable(1e11, [0.0, 1.0], [0.0, 1.0]).n == 2


def test_builtin_tables_against_the_reference_literals():
    from nestfit_amd import LineTable
    ref = json.loads(LITERALS.read_text())
    for model, key, n_trans in (('diazenylium', 'n2hp', 3), ('ammonia', 'nh3', 9)):
        for t in range(1, n_trans + 1):
            tab = LineTable.builtin(model, t)
            assert tab.n == ref[key]['NHF'][t - 1] and tab.nu == ref[key]['NU'][t - 1]
            assert tab.voff.tolist() == ref[key]['VOFF'][t - 1][:tab.n]
            assert tab.tau_wts.tolist() == ref[key]['TAU_WTS'][t - 1][:tab.n]
            assert tab.name == f'{model}:{t}'
    for model, t in (('diazenylium', 0), ('diazenylium', 4), ('ammonia', 10), ('gaussian', 1)):
        with pytest.raises(ValueError):
            LineTable.builtin(model, t)


def test_module_metadata():
    import nestfit_amd as na
    h, d = na.hyperfine, na.diazenylium
    assert (h.NAME, h.N, h.IX_VCEN, h.IX_SIGM) == ('hyperfine', 4, 0, 3)
    assert h.PAR_NAMES == d.PAR_NAMES == ['voff', 'tex', 'ltau', 'sigm']
    assert h.PAR_NAMES_SHORT == d.PAR_NAMES_SHORT and h.TEX_LABELS == d.TEX_LABELS
    assert h.TEX_LABELS_WITH_UNITS == d.TEX_LABELS_WITH_UNITS
    assert h.get_par_names(2) == ['v1', 'v2', 'Tx1', 'Tx2', 'lt1', 'lt2', 's1', 's2'] and h.get_par_names() == ['v', 'Tx', 'lt', 's']
    assert h.ModelRunner is na.HyperfineRunner is h.HyperfineRunner and h.model_predict is h.hf_predict
    assert h.ModelSpectrum is h.HyperfineSpectrum and na.LineTable is h.LineTable
    assert 'hyperfine' not in na.MODELS                      # the registry stays the reference's three
    assert na.model_module('hyperfine') is h and na.model_module('diazenylium') is d and na.model_module('nope') is None
    from nestfit_amd import fitter, postprocess
    assert fitter._MODEL_ID['hyperfine'] == postprocess._MODEL_ID['hyperfine'] == 3


# ---------------------------------------------------------------------------- the cube driver, the store, the map products
N_CHAN, NOISE, NU0 = 96, 0.1, 88.6318e9
TRUTH = np.array([0.4, 9.0, 0.3, 0.6])


def _three_lines(scale=1.0):
    from nestfit_amd import LineTable
    return LineTable(NU0, [-7.1, 0.0, 4.9], [0.2 * scale, 0.5, 0.3], name='three')


def _axis():
    return NU0 * (1.0 - np.linspace(14.0, -14.0, N_CHAN) / hfr.CKMS)


def _stack(nfo, lines, n=3, seed=0):
    """A 3 x 3 cube of the three-line species: a line in the pixels of even i_lon, noise only elsewhere."""
    from nestfit_amd.cubeio import CubeStack, DataCube, SimpleCube
    rng = np.random.default_rng(seed)
    x = _axis()
    model = hfr.hf_predict(nfo, x, hfr.tbg_of(nfo, x), hfr.table_of(lines), TRUTH)
    data = rng.normal(0, NOISE, (N_CHAN, n, n))
    for i in range(0, n, 2):
        data[:, :, i] += model[:, None]
    hdr = {'SIMPLE': True, 'BITPIX': -64, 'NAXIS': 3, 'NAXIS1': n, 'NAXIS2': n, 'NAXIS3': N_CHAN,
           'BUNIT': 'K', 'CTYPE1': 'RA---SIN', 'CTYPE2': 'DEC--SIN', 'CTYPE3': 'FREQ', 'CUNIT3': 'Hz',
           'CRVAL3': float(x[0]), 'CDELT3': float(x[1] - x[0]), 'CRPIX3': 1.0, 'RESTFRQ': NU0}
    return CubeStack([DataCube(SimpleCube(hdr, data), NOISE, lines=lines)])


def _priors():
    import nestfit_amd as na
    from scipy import stats
    x = np.linspace(0, 1, 200)
    ranges = [(-4, 4), (3.0, 20), (-1.0, 1.0), (0.2, 1.5)]
    return na.PriorTransformer([
        na.Prior(na.Distribution(lo + x * (hi - lo), stats.uniform(lo, hi - lo).pdf(lo + x * (hi - lo))), k)
        for k, (lo, hi) in enumerate(ranges)])


def _restatement_backend(fitter, lon, lat, ncomp, nlive, kw):
    """The numpy twin of the sampler, its likelihood the restatement on the stack's own tables."""
    from oracle import nfo
    from nestfit_amd import sampler
    ps = nfo.PriorSet(fitter.utrans.lower())
    pixels = []
    for i, j in zip(lon, lat):
        rows, has_nans = fitter.stack.get_spec_data(i, j)
        assert not has_nans
        pixels.append([(x, d, noise, hfr.tbg_of(nfo, x), hfr.table_of(dc.lines))
                       for (x, d, noise, _), dc in zip(rows, fitter.stack.cubes)])

    def loglike(pix, U):
        out = np.empty(U.shape[0])
        for k in range(U.shape[0]):
            th = U[k].copy()
            ps.transform(th, ncomp)
            U[k] = th
            out[k] = sum(hfr.loglike(d, hfr.hf_predict(nfo, x, tbg, tab, th), noise) for x, d, noise, tbg, tab in pixels[pix[k]])
        return out
    res = sampler.run_nested(loglike, 4 * ncomp, len(pixels), nlive=nlive, batch_target=64, **kw)
    null = np.array([sum(-np.sum(d ** 2) / (2 * noise ** 2) for _, d, noise, _, _ in p) for p in pixels])
    return res, null, N_CHAN


def _restatement_predictor(stack):
    from oracle import nfo

    def predict(lon, lat, theta, want_spectra):
        spec = np.empty((theta.shape[0], sum(dc.nchan for dc in stack.cubes)))
        for k, th in enumerate(theta):
            spec[k] = np.concatenate([hfr.hf_predict(nfo, dc.xarr, hfr.tbg_of(nfo, dc.xarr), hfr.table_of(dc.lines), th)
                                      for dc in stack.cubes])
        edges = np.concatenate([[0], np.cumsum([dc.nchan for dc in stack.cubes])])
        peak = np.stack([spec[:, a:b].max(axis=1) for a, b in zip(edges[:-1], edges[1:])], axis=1)
        tot = np.stack([spec[:, a:b].sum(axis=1) for a, b in zip(edges[:-1], edges[1:])], axis=1)
        return (spec, None, None) if want_spectra else (None, peak, tot)
    return predict


def test_cube_driver_store_and_products_without_a_gpu(nfo, tmp_path):
    import nestfit_amd as na
    from nestfit_amd import postprocess as pp
    from nestfit_amd.fitter import CubeFitter
    from nestfit_amd.store import HdfStore
    lines = _three_lines()
    stack = _stack(nfo, lines)
    fitter = CubeFitter(stack, _priors(), na.HyperfineRunner, lnZ_thresh=11, ncomp_max=1,
                        mn_kwargs={'nlive': 24, 'tol': 1.0, 'seed': 3, 'maxiter': 250}, nlive_snr_fact=0,
                        fit_backend=_restatement_backend)
    assert (fitter.model_id, fitter.n_model, fitter.runner_kwargs) == (3, 4, {})
    path = str(tmp_path / 'run')
    fitter.fit_cube(path, nproc=1)
    with HdfStore(path) as store:
        assert store.hdf.attrs['model_name'] == 'hyperfine' and store.model is na.hyperfine
        assert store.hdf.attrs['n_params'] == 4 and list(store.hdf.attrs['par_names']) == ['voff', 'tex', 'ltau', 'sigm']
        groups = {(g.attrs['i_lon'], g.attrs['i_lat']): g for g in store.iter_pix_groups()}
        assert sorted(groups) == [(i, j) for i in range(3) for j in range(3)]
        for (i, _), g in groups.items():
            assert g.attrs['nbest'] == (1 if i % 2 == 0 else 0), (i, g.attrs['nbest'])
            assert g['1'].attrs['n_params'] == 4 and g['1'].attrs['n_chan_tot'] == N_CHAN
        back = store.read_model_lines()
        assert back == [lines] and back[0].name == 'three' and back[0].nu == NU0
        assert np.array_equal(back[0].voff, lines.voff) and np.array_equal(back[0].tau_wts, lines.tau_wts)
    # a reopened store returns them; the map products through a stand-in for the device
    with HdfStore(path) as store:
        assert store.read_model_lines() == [lines]
        pp.postprocess_run(store, stack, evid_kernel=0.6, post_kernel=pp.gaussian_kernel(0.6),
                           predict_backend=_restatement_predictor(stack))
        peak = np.asarray(store.hdf[f'{store.dpath}/peak_intensity'])             # (t, m, b, l)
        spec = np.asarray(store.hdf[f'{store.dpath}/model_spec/spec0'])            # (m, S, b, l)
        pmap = np.asarray(store.hdf[f'{store.dpath}/nbest_MAP'])                   # (m, p, b, l)
        assert peak.shape == (1, 1, 3, 3) and spec.shape == (1, N_CHAN, 3, 3)
        x = stack.cubes[0].xarr                                                    # (the axis as the header gives it)
        for l in range(3):
            for b in range(3):
                if not np.isfinite(pmap[0, :, b, l]).all():                         # no MAP row: no products
                    assert np.isnan(peak[0, 0, b, l]) and np.isnan(spec[0, :, b, l]).all()
                    continue
                want = hfr.hf_predict(nfo, x, hfr.tbg_of(nfo, x), hfr.table_of(lines), pmap[0, :, b, l])
                np.testing.assert_allclose(spec[0, :, b, l], want.astype(np.float32), rtol=0, atol=0)
                assert peak[0, 0, b, l] == want.max()
                if l % 2 == 0:
                    assert abs(pmap[0, 0, b, l] - TRUTH[0]) < 0.5                  # the fit found the line
    # a stack whose table differs from the store's is refused
    other = _stack(nfo, _three_lines(scale=1.5))
    with HdfStore(path) as store:
        with pytest.raises(ValueError, match='line tables differ'):
            pp.postprocess_run(store, other, predict_backend=_restatement_predictor(other))
        with pytest.raises(ValueError, match='line tables differ'):
            pp.check_model_lines(store, other)
    # ... and a cube takes a trans_id or a table, not both
    from nestfit_amd.cubeio import DataCube
    with pytest.raises(ValueError, match='not both'):
        DataCube(stack.cubes[0], NOISE, trans_id=1, lines=lines)
