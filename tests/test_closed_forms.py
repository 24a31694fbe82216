"""Pins that do not go through the oracle's own code path: independent closed forms derived
from the reference text for the parts no reference output exists for.

  * every `Prior` kind of nestfit/core/core.pyx:169-435 against numpy forms built from the `Distribution` tables alone
    (tests/prior_closed_forms.py) -- oracle on CPU, device under -m gpu;
  * `cold` (Swift et al. 2005 eq. A6, ammonia.pyx:280-286) and `lte` (ammonia.pyx:346) as identities of `amm_predict`:
    cold = the same call with trot replaced by swift(trot), lte = the same call with tex replaced by trot;
  * the eight known-answer spectra of the survey, channel by channel (tests/golden/kat_spectra.npz).
"""
import json
import math
from pathlib import Path

import numpy as np
import pytest

from nestfit_amd.synth import freq_axis

import prior_closed_forms as pcf

GOLD = Path(__file__).parent / 'golden'


def _prior_sets(na):
    from scipy import stats
    u = np.linspace(0, 1, 300)
    d_v = na.Distribution(8 * u - 4, stats.beta(5, 5).pdf(u))
    d_sep = na.Distribution(3 * u + 0.7, stats.beta(1.5, 3.5).pdf(u))
    d_s = na.Distribution(2 * u + 0.067, stats.beta(1.5, 5).pdf(u))
    d_t = na.Distribution(23 * u + 7, stats.beta(3, 6.7).pdf(u))
    d_vw = na.Distribution(80 * u - 40, stats.beta(5, 5).pdf(u))
    rest = [na.DuplicatePrior(d_t, 1, 2), na.Prior(d_t, 3), na.ConstantPrior(0.25, 5)]
    return {
        'ordered': [na.OrderedPrior(d_v, 0), na.Prior(d_s, 4)] + rest,
        'spaced': [na.SpacedPrior(na.Prior(d_v, 0), na.Prior(d_sep, 0)), na.Prior(d_s, 4)] + rest,
        'censep': [na.CenSepPrior(na.Prior(d_v, 0), na.Prior(d_sep, 0)), na.Prior(d_s, 4)] + rest,
        'rcensep': [na.ResolvedCenSepPrior(na.Prior(d_v, 0), na.Prior(d_sep, 0), na.Prior(d_s, 4))] + rest,
        'rplace': [na.ResolvedPlacementPrior(na.Prior(d_v, 0), na.Prior(d_s, 4), scale=1.2)] + rest,
        'rplace_wide': [na.ResolvedPlacementPrior(na.Prior(d_v, 0), na.Prior(d_s, 4), scale=6.0)] + rest,
        'irdc': list(na.get_irdc_priors(size=500).priors),
        'synth': list(na.get_synth_priors(size=500).priors),
        # up to ten components (MAXCOMP): the minimum separations of the sets above overflow the 8 km/s axis in most
        # draws at high counts (Degenerate), so these place them on +-40 km/s, with sigma <= 1 km/s for the irdc shape
        'rplace_wide_axis': [na.ResolvedPlacementPrior(na.Prior(d_vw, 0), na.Prior(d_s, 4), scale=1.2)] + rest,
        'irdc_wide_axis': irdc_wide_axis(na, size=500),
    }


def irdc_wide_axis(na, size=500, vhalf=40.0, sigm_hi=1.0):
    """get_irdc_priors' five priors and table size on a velocity axis of +-vhalf km/s and sigma in [0.067, sigm_hi]:
    its draws are never degenerate up to ten components while 9 * 1.2 * FWHM * sigm_hi < 2 * vhalf."""
    from scipy import stats
    u = np.linspace(0, 1, size)
    d_voff = na.Distribution(2 * vhalf * u - vhalf, stats.beta(5.0, 5.0).pdf(u))
    d_sigm = na.Distribution((sigm_hi - 0.067) * u + 0.067, stats.beta(1.5, 5.0).pdf(u))
    return [na.ResolvedPlacementPrior(na.Prior(d_voff, 0), na.Prior(d_sigm, 4), scale=1.2),
            na.Prior(na.Distribution(23.00 * u + 7.00, stats.beta(3.0, 6.7).pdf(u)), 1),
            na.Prior(na.Distribution(9.26 * u + 2.80, stats.beta(1.0, 2.5).pdf(u)), 2),
            na.Prior(na.Distribution(4.00 * u + 12.50, stats.beta(10.0, 8.5).pdf(u)), 3),
            na.ConstantPrior(0, 5)]


def _ncomps(name):
    if name in ('censep', 'rcensep', 'synth'):
        return (1, 2)                                # n <= 2: core.pyx:316-318, 364-366
    if name in ('rplace', 'rplace_wide', 'irdc'):
        return (1, 2, 3, 4)                          # beyond: mostly Degenerate on their 8 km/s axis (the *_wide_axis sets)
    return tuple(range(1, 11))                       # up to MAXCOMP


def test_oracle_prior_transforms_against_closed_forms(nfo):
    import nestfit_amd as na
    rng = np.random.default_rng(77)
    worst, n_checked, n_degenerate = 0.0, 0, 0
    for name, priors in _prior_sets(na).items():
        ps = nfo.PriorSet(na.PriorTransformer(np.array(priors, dtype=object)).lower())
        for ncomp in _ncomps(name):
            for u in rng.uniform(size=(150, 6 * ncomp)):
                try:
                    want = pcf.transform(priors, u, ncomp)
                except pcf.Degenerate:
                    n_degenerate += 1
                    continue
                got = u.copy()
                ps.transform(got, ncomp)
                err = np.max(np.abs(got - want) / (1e-3 + np.abs(want)))
                worst = max(worst, err)
                n_checked += 1
                assert err < 1e-11, (name, ncomp, u, got, want)
    print(f'oracle vs closed forms: {n_checked} draws, worst relative deviation {worst:.2e}; {n_degenerate} degenerate draws skipped')
    assert n_checked > 10 * n_degenerate


@pytest.mark.gpu
def test_device_prior_transforms_against_closed_forms(engine):
    rng = np.random.default_rng(78)
    for name, priors in _prior_sets(engine).items():
        ut = engine.PriorTransformer(np.array(priors, dtype=object))
        for ncomp in _ncomps(name):
            U = rng.uniform(size=(150, 6 * ncomp))
            keep, want = [], []
            for k, u in enumerate(U):
                try:
                    want.append(pcf.transform(priors, u, ncomp))
                    keep.append(k)
                except pcf.Degenerate:
                    pass
            if not keep:                                 # (scale 6 with four components: every draw overflows the interval)
                continue
            got = U.copy()
            ut.transform_batch(got, ncomp)
            got, want = got[keep], np.array(want)
            # (the device's placement CDF comes from prefix moments: <= ~1e-10 km/s on the centroids)
            np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-10, err_msg=f'{name} ncomp={ncomp}')


def _swift(tkin):                                    # Swift et al. 2005 eq. A6 (ammonia.pyx:280-286)
    return tkin / (1.0 + (tkin / 41.18) * math.log(1.0 + 0.6 * math.exp(-15.7 / tkin)))


def test_swift_and_the_cold_lte_identities_on_the_oracle(nfo):
    for tkin in (5.0, 9.3, 15.0, 22.5, 41.18, 80.0):
        assert nfo.swift_convert(tkin) == pytest.approx(_swift(tkin), rel=1e-15)
    assert _swift(15.0) == pytest.approx(14.023487575888257, abs=1e-8)           # the reference's own known answer
    _cold_lte_identities(lambda s, p, **kw: nfo.amm_predict(s, p, **kw), nfo.AmmoniaSpectrum, 0.0)


def _cold_lte_identities(predict, spectrum_cls, tol):
    rng = np.random.default_rng(9)
    for trans in (1, 2, 3, 4, 7, 9):
        x = freq_axis(trans, 512)
        for ncomp in (1, 2):
            for _ in range(3):
                p = np.concatenate([rng.uniform(-3, 3, ncomp), rng.uniform(8, 28, ncomp), rng.uniform(3, 9, ncomp),
                                    rng.uniform(13.8, 15.2, ncomp), rng.uniform(0.15, 1.2, ncomp), rng.uniform(0.1, 0.9, ncomp)])
                def spec(params, **kw):
                    s = spectrum_cls(x, np.zeros(512), 0.1, trans)
                    predict(s, np.ascontiguousarray(params), **kw)
                    return np.array(s.get_spec())
                warm = p.copy()
                warm[ncomp:2 * ncomp] = [_swift(t) for t in p[ncomp:2 * ncomp]]
                a, b = spec(p, cold=True), spec(warm)
                np.testing.assert_allclose(a, b, rtol=max(tol, 2e-13), atol=0)       # swift(trot) by libm here and there
                assert np.array_equal(a != 0, b != 0)
                eq = p.copy()
                eq[2 * ncomp:3 * ncomp] = p[ncomp:2 * ncomp]
                a, b = spec(p, lte=True), spec(eq)
                np.testing.assert_allclose(a, b, rtol=tol, atol=0)                   # tex := trot, nothing else
                both = warm.copy()
                both[2 * ncomp:3 * ncomp] = warm[ncomp:2 * ncomp]
                np.testing.assert_allclose(spec(p, cold=True, lte=True), spec(both), rtol=max(tol, 2e-13), atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['table', 'fast'])
def test_cold_lte_identities_on_the_device(engine, mode):
    engine.set_exp_mode(mode)
    try:
        _cold_lte_identities(lambda s, p, **kw: engine.amm_predict(s, p, **kw), engine.AmmoniaSpectrum,
                             1e-13 if mode == 'table' else 2e-6)
    finally:
        engine.set_exp_mode('fast')


def _kat_cases():
    kat = json.loads((GOLD / 'survey_kat.json').read_text())['spectra']
    gold = np.load(GOLD / 'kat_spectra.npz')
    return [(c, gold[f'pred_{k}']) for k, c in enumerate(kat)]


def test_oracle_reproduces_the_committed_kat_spectra(nfo):
    for c, want in _kat_cases():
        x = freq_axis(c['trans_id'], c['n_chan'], c['vhalf'])
        s = nfo.AmmoniaSpectrum(x, np.zeros(c['n_chan']), c['noise'], c['trans_id'])
        nfo.amm_predict(s, np.array(c['params'], dtype=float))
        got = s.get_spec()
        assert np.array_equal(got != 0, want != 0)
        np.testing.assert_allclose(got, want, rtol=1e-13, atol=0)
        # ... whose summaries are the reference's recorded outputs
        assert int((want != 0).sum()) == c['nnz'] and want.max() == pytest.approx(c['max'], rel=1e-12)


@pytest.mark.gpu
def test_device_table_mode_reproduces_the_kat_spectra_channel_by_channel(engine):
    """GPU table mode against (i) the committed per-channel vectors and (ii) the reference's recorded max / sum / support /
    lnL directly, to 1e-12 (the reference's own build-flag noise is 1e-11)."""
    engine.set_exp_mode('table')
    try:
        for c, want in _kat_cases():
            x = freq_axis(c['trans_id'], c['n_chan'], c['vhalf'])
            s = engine.AmmoniaSpectrum(x, np.zeros(c['n_chan']), c['noise'], c['trans_id'])
            engine.amm_predict(s, np.array(c['params'], dtype=float))
            got = s.get_spec()
            assert np.array_equal(got != 0, want != 0) and int((got != 0).sum()) == c['nnz'] and got[-1] == 0.0
            np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
            assert s.max_spec == pytest.approx(c['max'], rel=1e-12)
            if 'sum' in c:
                assert s.sum_spec == pytest.approx(c['sum'], rel=1e-12)
            assert s.loglikelihood == pytest.approx(c['lnL'], rel=1e-12)
    finally:
        engine.set_exp_mode('fast')
