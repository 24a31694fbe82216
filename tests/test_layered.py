"""Layered radiative transfer on the device (nfa_specset_set_layered, `layered=True`): component 0 is the farthest
from the observer and every component absorbs those behind it, pred <- pred + (g_c - pred) a_c in component order.

The reference is tests/layer_restatement.py at the sizes of the sibling tests (300 channels: four full rows of 64 and one of
44; 200 parameter rows), in both modes.  TIGHT, LNL_RTOL and the per-channel rule are the sibling tests', but deviations are
measured against S = sum_c |g_c a_c|, the summed model term by term, not against the layered value: a layered channel can
be a small difference of large terms.  Every stage's error is at most eps a_c max(g_c, pred) with eps the mode's relative
error on one component's term, so over ncomp stages |got - want| <= ncomp TIGHT[mode] S, plus the helper's floor.  The zero
pattern is S's, exactly.

Measured on an MI355X, the worst |got - want| / S over every row and channel of a case (the bound is ncomp x 1e-11 in the
table mode, ncomp x 5e-7 in the fast mode):

    ammonia (1,1)+(2,2), 1..4 layers    table 2.6e-15, 2.1e-15, 2.5e-15, 3.2e-15    fast 2.9e-7, 3.7e-7, 3.3e-7, 3.2e-7
    N2H+ 2-1 (wide), 2 layers           table 7.4e-16                              fast 2.3e-7
    a line table, 3 layers              table 9.0e-16                              fast 2.9e-7
    an LTE blend, 2 layers              table 9.0e-16                              fast 2.6e-7
    a filled mix, 1..4 layers           table 1.2e-15, 1.0e-15, 8.7e-16, 9.5e-16    fast 2.7e-7, 2.7e-7, 3.0e-7, 2.6e-7

lnL within 1.8e-15 (table) and 9.1e-8 (fast) of the restatement's.  The sampler run: the layered two-component fit's best lnL
-142.8 (lnZ -199.4 +- 0.5) against the summed fit's -48323.0 on the same data.
"""
import functools
import os

import numpy as np
import pytest

import hf_restatement as hfr
import layer_restatement as lay
import mix_restatement as mr
from test_hyperfine import _through_a_broker
from test_lte import _routes
from test_lte_bands_cpu import N_CHAN, band_axis
from test_lte_mix import N_ROWS, NOISE
from test_sibling_models import LNL_RTOL, MODES, TB_ATOL_K, TIGHT, _simple_priors, n2hp_axis

pytestmark = pytest.mark.gpu


@pytest.fixture
def mode_guard(engine):
    from nestfit_amd import _ffi
    yield
    _ffi.set_option('coalesce', 8)
    _ffi.set_option('lnl_split', 0)
    engine.set_exp_mode('fast')


def _check_layered(got, want, S, mode, ncomp, tex):
    """The zero pattern is S's; every channel within ncomp TIGHT[mode] S plus the floor of tests/test_lte_mix.py's helper
    (fast mode: 2^-53 of the components' tex, 4e-15 K at the least); returns the worst |got - want| / S of the channels above 1e-6 K."""
    assert np.array_equal(got == 0, S == 0)
    floor = max(TB_ATOL_K[mode], 2.0 ** -53 * float(np.sum(tex))) if mode == 'fast' else TB_ATOL_K[mode]
    dev = np.abs(got - want)
    big = S > 1e-6
    worst = float(np.max(dev[big] / S[big])) if big.any() else 0.0
    assert (dev <= ncomp * TIGHT[mode] * S + floor).all(), (worst, float(np.max(dev - ncomp * TIGHT[mode] * S)))
    return worst


# ---------------------------------------------------------------------------- the models
#   name: parameters per component, the rows of (tex, depth), the depth parameter from thin to opaque, its thick band
LINES3 = (88.6318e9, [-7.1, 0.0, 4.9], [0.2, 0.5, 0.3])
MODELS = {
    'ammonia': dict(n=6, tex_row=2, depth_row=3, depth=(11.3, 16.6), thick=(14.6, 15.3), tex=(3.5, 9.0), sigm_row=4),
    'n2hp':    dict(n=4, tex_row=1, depth_row=2, depth=(-3.0, 2.7), thick=(1.0, 1.8), tex=(3.5, 20.0), sigm_row=3),
    'lines':   dict(n=4, tex_row=1, depth_row=2, depth=(-3.5, 2.2), thick=(0.5, 1.3), tex=(3.5, 20.0), sigm_row=3),
    'mix':     dict(n=5, tex_row=1, depth_row=2, depth=(11.0, 17.0), thick=(15.2, 15.8), tex=(8.0, 55.0), sigm_row=3),
    'filled':  dict(n=6, tex_row=1, depth_row=2, depth=(11.0, 17.0), thick=(15.2, 15.8), tex=(8.0, 55.0), sigm_row=3),
}


@functools.lru_cache(maxsize=None)
def _species():
    """mix_restatement.test_species, once: its partition tables are direct sums."""
    import nestfit_amd as na
    return mr.test_species(na)


def draw_layers(rng, name, ncomp, row):
    """Parameter-major theta of `ncomp` layers.  Even rows: the layers on top of one another -- within 0.4 of the narrowest
    width in velocity, every one thick (the model's `thick` band of its depth parameter), the hottest at the back so that
    what the front ones absorb is a large part of the row.  Odd rows: anywhere within +-5 km/s, the depth parameter over its
    whole range from tau < 1e-3 to tau > 32, widths over 0.2..1.26 km/s."""
    m = MODELS[name]
    if row % 2 == 0:
        sigm = rng.uniform(0.4, 1.0, ncomp)
        voff = rng.uniform(-3, 3) + rng.uniform(-0.4, 0.4, ncomp) * sigm.min()
        tex = np.sort(rng.uniform(*m['tex'], ncomp))[::-1]
        depth = rng.uniform(*m['thick'], ncomp)
    else:
        sigm = 10 ** rng.uniform(-0.7, 0.1, ncomp)
        voff = rng.uniform(-5, 5, ncomp)
        tex = rng.uniform(*m['tex'], ncomp)
        depth = rng.uniform(*m['depth'], ncomp)
    rows = {0: voff, m['tex_row']: tex, m['depth_row']: depth, m['sigm_row']: sigm}
    if name == 'ammonia':
        rows[1], rows[5] = tex + rng.uniform(2.0, 12.0, ncomp), rng.uniform(0.0, 0.5, ncomp)     # trot above tex; orth
    if name in ('mix', 'filled'):
        rows[4] = depth - rng.uniform(0.5, 2.0, ncomp)                                          # the isotopologue's column
    if name == 'filled':
        # lnff, the layers of a row in the ncomp equal parts of the range in an order drawn per row: over -0.2..0 where the
        # layers are stacked (f > 0.63: a = f (1 - e^-tau) can pass 0.5), over -1..0 elsewhere
        rows[5] = (-0.2 if row % 2 == 0 else -1.0) * (1.0 - (rng.permutation(ncomp) + rng.uniform(0.05, 0.95, ncomp)) / ncomp)
    return np.concatenate([rows[k] for k in range(m['n'])])


def _spectra(name, na):
    """[(axis, what the restatement and the runner need of the spectrum)] of the model's test set."""
    from nestfit_amd.synth import freq_axis
    if name == 'ammonia':
        return [(freq_axis(1, N_CHAN, 20.0), 1), (freq_axis(2, N_CHAN, 20.0), 2)]          # (1,1) + (2,2)
    if name == 'n2hp':
        return [(n2hp_axis(2, N_CHAN), 2)]                                                # 2-1: 40 lines, the WIDE instances
    if name == 'lines':
        t = na.LineTable(*LINES3, name='three')
        return [(LINES3[0] * (1.0 - np.linspace(20.0, -20.0, N_CHAN) / hfr.CKMS), t)]
    mol, ks, iso, isos = _species()
    return [(band_axis(ks[0].nu), na.LteBlend(ks + isos)), (band_axis(ks[0].nu), isos[1])]


def _data_rows(name, na, seed):
    rng = np.random.default_rng(seed)
    return [[x, rng.normal(0, NOISE, N_CHAN), NOISE, what] for x, what in _spectra(name, na)]


def _runner(engine, name, rows, ut, ncomp, **kw):
    if name == 'ammonia':
        return engine.AmmoniaRunner.from_data(rows, ut, ncomp=ncomp, **kw)
    if name == 'n2hp':
        return engine.DiazenyliumRunner.from_data(rows, ut, ncomp=ncomp, **kw)
    if name == 'lines':
        return engine.HyperfineRunner.from_data(rows, ut, ncomp=ncomp, **kw)
    mol, ks, iso, isos = _species()
    return engine.LteMix((mol, iso), fill=name == 'filled').Runner.from_data(rows, ut, ncomp=ncomp, **kw)


def restated(nfo, na, name, rows, theta, tbgs=None, terms=None):
    """(layered spectra of the rows concatenated, S likewise, lnL) of one parameter vector; `terms`: a list that receives
    the (tau, g, a) of every layer of the FIRST spectrum."""
    out = []
    for k, (x, _, _, what) in enumerate(rows):
        t = terms if k == 0 else None
        if name == 'ammonia':
            out.append(lay.amm_layered(nfo, x, what, theta, t))
        elif name == 'n2hp':
            out.append(lay.nnhp_layered(nfo, x, what, theta, t))
        elif name == 'lines':
            out.append(lay.hf_layered(nfo, x, tbgs[k] if tbgs else hfr.tbg_of(nfo, x), hfr.table_of(what), theta, t))
        else:
            mol, ks, iso, isos = _species()
            out.append(lay.mix_layered(nfo, x, tbgs[k] if tbgs else hfr.tbg_of(nfo, x), what, (mol, iso), theta, fill=name == 'filled', terms=t))
    lnl = sum(hfr.loglike(d, p, noise) for (_, d, noise, _), (p, _) in zip(rows, out))
    return np.concatenate([p for p, _ in out]), np.concatenate([s for _, s in out]), lnl


def _tex_of(name, theta, ncomp):
    r = MODELS[name]['tex_row']
    return theta[r * ncomp:(r + 1) * ncomp]


@functools.lru_cache(maxsize=None)
def _reference(name, ncomp):
    """(rows, thetas, layered spectra, S, lnL, what the draws contain) of the restatement, computed once for both modes."""
    import nestfit_amd as na
    from oracle import nfo
    rows = _data_rows(name, na, seed=100 + ncomp)
    rng = np.random.default_rng(9000 + 10 * len(name) + ncomp)
    thetas = np.stack([draw_layers(rng, name, ncomp, k) for k in range(N_ROWS)])
    tbgs = [hfr.tbg_of(nfo, x) for x, *_ in rows]
    spec, S, lnl, tau_peak, stacked, absorbed = [], [], [], [], 0, []
    m = MODELS[name]
    for th in thetas:
        terms = []
        p, s, l = restated(nfo, na, name, rows, th, tbgs, terms)
        spec.append(p), S.append(s), lnl.append(l)
        tau_peak += [t[0].max() for t in terms]
        voff, sigm = th[:ncomp], th[m['sigm_row'] * ncomp:(m['sigm_row'] + 1) * ncomp]
        # two layers within one line width of each other, a > 0.5 in both in one channel: what the layers are for
        pairs = [(c, d) for c in range(ncomp) for d in range(c + 1, ncomp)
                 if abs(voff[c] - voff[d]) < min(sigm[c], sigm[d]) and np.minimum(terms[c][2], terms[d][2]).max() > 0.5]
        if pairs:
            stacked += 1
            summed = sum(t[1] * t[2] for t in terms)                                  # (of the first spectrum, like `terms`)
            absorbed.append(np.abs(p[:N_CHAN] - summed).max() / np.abs(s[:N_CHAN]).max())
    spec, S, lnl = np.stack(spec), np.stack(S), np.array(lnl)
    for a in (spec, S, lnl, thetas):
        a.setflags(write=False)
    return rows, thetas, spec, S, lnl, dict(tau_peak=np.array(tau_peak), stacked=stacked, absorbed=np.array(absorbed))


def _against_the_restatement(engine, name, ncomp, mode):
    engine.set_exp_mode(mode)
    rows, thetas, want, S, want_lnl, draws = _reference(name, ncomp)
    # the draws contain what they are meant to contain
    if ncomp > 1:
        assert draws['stacked'] >= N_ROWS // 4 and draws['absorbed'].min() > 0.1, (draws['stacked'], draws['absorbed'].min())
    assert draws['tau_peak'].min() < 1e-3 and draws['tau_peak'].max() > 32.0
    assert S.max() > 1.0
    run = _runner(engine, name, rows, None, ncomp, layered=True)
    assert run.layered is True and run.ndim == MODELS[name]['n'] * ncomp
    spec, lnl = run.predict_batch(np.array(thetas))
    worst, worst_lnl = 0.0, 0.0
    for sp, ll, ws, s, wl, th in zip(spec, lnl, want, S, want_lnl, thetas):           # every row, every channel
        worst = max(worst, _check_layered(sp, ws, s, mode, ncomp, _tex_of(name, th, ncomp)))
        worst_lnl = max(worst_lnl, abs(ll - wl) / abs(wl))
    print(f'layered {name} {mode} ncomp={ncomp}: worst |got - want| / S {worst:.2e} (bound {ncomp * TIGHT[mode]:.1e}), lnL {worst_lnl:.2e}')
    np.testing.assert_allclose(lnl, want_lnl, rtol=LNL_RTOL[mode])
    return run, rows, thetas, spec, lnl


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('ncomp', [1, 2, 3, 4])
def test_ammonia_against_the_restatement(engine, ncomp, mode, mode_guard):
    """NH3 (1,1) + (2,2): the oracle's one-component predictions through the layers."""
    _against_the_restatement(engine, 'ammonia', ncomp, mode)


@pytest.mark.parametrize('mode', MODES)
def test_diazenylium_wide_against_the_restatement(engine, mode, mode_guard):
    """N2H+ 2-1, 40 lines: the WIDE instances."""
    _against_the_restatement(engine, 'n2hp', 2, mode)


@pytest.mark.parametrize('mode', MODES)
def test_a_line_table_against_the_restatement(engine, mode, mode_guard):
    _against_the_restatement(engine, 'lines', 3, mode)


@pytest.mark.parametrize('mode', MODES)
def test_an_lte_blend_against_the_restatement(engine, mode, mode_guard):
    _against_the_restatement(engine, 'mix', 2, mode)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('ncomp', [1, 2, 3, 4])
def test_a_filled_mix_against_the_restatement(engine, ncomp, mode, mode_guard):
    """a_c = f_c (1 - e^-tau_c), lnff differing between the layers of every row: a component-index slip shows."""
    run, rows, thetas, spec, lnl = _against_the_restatement(engine, 'filled', ncomp, mode)
    lnff = thetas[:, 5 * ncomp:]
    assert ncomp == 1 or np.abs(np.diff(np.sort(lnff, axis=1), axis=1)).min() > 0.019 / ncomp
    # ... and `predict` of a layered runner: the runner's own set, spectrum by spectrum
    run.predict(np.array(thetas[2]))
    assert np.array_equal(np.concatenate([s.get_spec() for s in run.spectra]), spec[2])
    assert sum(s.loglikelihood for s in run.spectra) == pytest.approx(lnl[2], rel=1e-12)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', ['ammonia', 'n2hp', 'lines', 'mix', 'filled'])
def test_one_layer_is_the_summed_runner(engine, name, mode, mode_guard):
    """g - 0 = g: the summed runner's spectra and lnL to TIGHT (another instance of the kernel: whether the bits are the
    same is reported, not promised)."""
    engine.set_exp_mode(mode)
    rows, thetas, _, S, _, _ = _reference(name, 1)
    spec, lnl = _runner(engine, name, rows, None, 1, layered=True).predict_batch(np.array(thetas))
    summed = _runner(engine, name, rows, None, 1)
    assert summed.layered is False
    want, want_lnl = summed.predict_batch(np.array(thetas))
    worst = max(_check_layered(sp, ws, s, mode, 1, _tex_of(name, th, 1)) for sp, ws, s, th in zip(spec, want, S, thetas))
    print(f'layered {name} {mode}: one layer against the summed runner: worst {worst:.2e}, same bits: {np.array_equal(spec, want)}')
    np.testing.assert_allclose(lnl, want_lnl, rtol=LNL_RTOL[mode])


@pytest.mark.parametrize('mode', MODES)
def test_the_order_of_the_components_is_the_order_along_the_line_of_sight(engine, nfo, mode, mode_guard):
    """theta with the two front components swapped: the restatement of the swapped vector, not of the original."""
    engine.set_exp_mode(mode)
    for name, ncomp in (('ammonia', 2), ('filled', 3)):
        rows, thetas, want, S, _, _ = _reference(name, ncomp)
        n = MODELS[name]['n']
        order = list(range(ncomp - 2)) + [ncomp - 1, ncomp - 2]
        swapped = np.ascontiguousarray(thetas[:40].reshape(40, n, ncomp)[:, :, order].reshape(40, -1))
        spec, _ = _runner(engine, name, rows, None, ncomp, layered=True).predict_batch(swapped)
        differ = 0
        for sp, th, orig, s in zip(spec, swapped, want[:40], S[:40]):
            ws, s2, _ = restated(nfo, engine, name, rows, th)
            _check_layered(sp, ws, s2, mode, ncomp, _tex_of(name, th, ncomp))
            differ += int(np.abs(sp - orig).max() > 0.1 * s.max())
        assert differ >= 8                                                     # (stacked rows of unlike tex: a tenth of the peak and more)


# ---------------------------------------------------------------------------- routes
def _ranges(name):
    m = MODELS[name]
    r = {0: (-5, 5), m['tex_row']: m['tex'], m['depth_row']: (m['thick'][0] - 1.5, m['thick'][1]), m['sigm_row']: (0.2, 1.2)}
    if name == 'ammonia':
        r[1], r[5] = (10.0, 25.0), (0.0, 0.5)
    if name in ('mix', 'filled'):
        r[4] = (12.5, 14.5)
    if name == 'filled':
        r[5] = (-1.0, 0.0)
    return [r[k] for k in range(m['n'])]


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', ['ammonia', 'filled'])
def test_the_same_bits_on_every_route(engine, nfo, name, mode, mode_guard):
    from nestfit_amd import _ffi
    engine.set_exp_mode(mode)
    rng = np.random.default_rng(83)
    ut = _simple_priors(engine, _ranges(name))
    rows = _data_rows(name, engine, seed=3)
    tbgs = [hfr.tbg_of(nfo, x) for x, *_ in rows]
    run = _runner(engine, name, rows, ut, 2, layered=True)
    summed = _runner(engine, name, rows, ut, 2)
    # host and device batches, coalescing 8 and 1, single points and a handful
    U, theta, lnl = _routes(engine, run, rng)
    for k in (0, 100, 512):
        assert lnl[k] == pytest.approx(restated(nfo, engine, name, rows, theta[k], tbgs)[2], rel=LNL_RTOL[mode])
    assert not np.array_equal(summed.loglikelihood_batch(U.copy()), lnl)
    for split in (4, 1):                                                        # ... whatever the row split of a small launch
        _ffi.set_option('lnl_split', split)
        run_s = _runner(engine, name, rows, ut, 2, layered=True)                # (a runner reads the option when it is made)
        for k in (0, 7, 150):
            u = U[k].copy()
            assert run_s.loglikelihood(u) == lnl[k] and np.array_equal(u, theta[k]), split
        few = U[20:31].copy()
        assert np.array_equal(run_s.loglikelihood_batch(few), lnl[20:31]), split
    _ffi.set_option('lnl_split', 0)
    lb, tb = _through_a_broker(engine, run, U[:64].reshape(8, 8, -1))
    assert np.array_equal(lb.ravel(), lnl[:64]) and np.array_equal(tb.reshape(64, -1), theta[:64])
    # predict_batch: whatever the batch
    spec, pl = run.predict_batch(theta[:40])
    for k in (0, 13, 39):
        s1, l1 = run.predict_batch(theta[k:k + 1])
        assert np.array_equal(s1[0], spec[k]) and l1[0] == pl[k]
    np.testing.assert_allclose(pl, lnl[:40], rtol=LNL_RTOL[mode])
    ws, s, _ = restated(nfo, engine, name, rows, theta[3], tbgs)
    _check_layered(spec[3], ws, s, mode, 2, _tex_of(name, theta[3], 2))
    # a noise per channel, with masked channels
    chan = [rng.uniform(0.1, 0.3, N_CHAN) for _ in rows]
    for c in chan:
        c[rng.integers(0, N_CHAN, 5)] = np.inf
    rows_c = [[x, d, c, t] for (x, d, _, t), c in zip(rows, chan)]
    run_c = _runner(engine, name, rows_c, ut, 2, layered=True)
    _, theta_c, lnl_c = _routes(engine, run_c, rng, n_rows=256)
    for k in (0, 100, 255):
        pred = restated(nfo, engine, name, rows, theta_c[k], tbgs)[0]
        want = sum(-np.sum(((d - pred[i * N_CHAN:(i + 1) * N_CHAN]) / c)[np.isfinite(c)] ** 2) / 2 for i, (_, d, c, _) in enumerate(rows_c))
        assert lnl_c[k] == pytest.approx(want, rel=LNL_RTOL[mode])
    # a baseline of order 1: the same bits on every route, never a worse fit than without one, and the layered model's
    run_b = _runner(engine, name, rows, ut, 2, layered=True, baseline_order=1)
    Ub, theta_b, lnl_b = _routes(engine, run_b, rng, n_rows=256)
    plain = run.loglikelihood_batch(Ub.copy())
    assert (lnl_b >= plain - 1e-9 * np.abs(plain)).all() and (lnl_b > plain).any()
    from nestfit_amd._model import baseline_fit
    for k in (0, 255):
        pred = restated(nfo, engine, name, rows, theta_b[k], tbgs)[0]
        want = 0.0
        for i, (_, d, noise, _) in enumerate(rows):
            resid = d - pred[i * N_CHAN:(i + 1) * N_CHAN]
            want += -np.sum((resid - baseline_fit(resid, np.ones(N_CHAN), 1)) ** 2) / (2 * noise * noise)
        assert lnl_b[k] == pytest.approx(want, rel=10 * LNL_RTOL[mode])        # (chi^2 less what the baseline takes away: a difference)


@pytest.mark.parametrize('mode', MODES)
def test_every_batch_of_a_coalesced_group_reads_its_own_theta(engine, mode, mode_guard):
    """Device batches of ONE shape, held and launched together at coalesce 8 and one by one at 1, each in another part of
    the prior: every batch against the host call on the same rows, theta and lnL bit for bit."""
    from nestfit_amd import _ffi
    from test_device_batches import _run_on_device
    engine.set_exp_mode(mode)
    rng = np.random.default_rng(62)
    for name, ncomp, each, n_batch in (('filled', 2, 256, 5), ('ammonia', 3, 128, 3)):
        ut = _simple_priors(engine, _ranges(name))
        run = _runner(engine, name, _data_rows(name, engine, seed=61), ut, ncomp, layered=True)
        batches = []
        for k in range(n_batch):
            U = rng.uniform(size=(each, run.ndim))
            U[:, ncomp:2 * ncomp] = (k + rng.uniform(size=(each, ncomp))) / n_batch      # the second parameter row: its k-th part
            batches.append((None, U))
        want = []
        for _, U in batches:
            theta = U.copy()
            want.append((theta, run.loglikelihood_batch(theta)))
        assert len({w[1].tobytes() for w in want}) == n_batch and all(np.isfinite(w[1]).all() for w in want)
        for coalesce in (8, 1):
            _ffi.set_option('coalesce', coalesce)
            got = _run_on_device(_ffi, run._run.handle, batches)
            for k, ((theta, lnl), (want_theta, want_lnl)) in enumerate(zip(got, want)):
                assert np.array_equal(theta, want_theta) and np.array_equal(lnl, want_lnl), (name, coalesce, k)
        _ffi.set_option('coalesce', 8)


@pytest.mark.parametrize('mode', MODES)
def test_the_setter_on_a_live_runner(engine, nfo, mode, mode_guard):
    """nfa_specset_set_layered on a runner in use: on gives the layered restatement, off the summed runner's bits -- also
    after a single point was served, whose captured graph holds the kernel of the moment."""
    from nestfit_amd import _ffi
    engine.set_exp_mode(mode)
    lib = _ffi.load()
    name, ncomp = 'ammonia', 2
    rows, thetas, want, S, want_lnl, _ = _reference(name, ncomp)
    ut = _simple_priors(engine, _ranges(name))
    run = _runner(engine, name, rows, ut, ncomp)
    fresh = _runner(engine, name, rows, ut, ncomp)
    handle = run._ss.handle
    assert lib.nfa_specset_layered(handle) == 0 and lib.nfa_specset_layered(None) == 0
    summed_spec, summed_lnl = fresh.predict_batch(np.array(thetas[:64]))
    u = np.full(run.ndim, 0.37)
    point_summed = run.loglikelihood(u.copy())                                  # a single point: the graph is captured
    assert point_summed == run.loglikelihood(u.copy())
    for turn in range(2):
        _ffi.check(lib.nfa_specset_set_layered(handle, 1))
        assert lib.nfa_specset_layered(handle) == 1
        spec, lnl = run.predict_batch(np.array(thetas[:64]))
        for sp, ws, s, th in zip(spec, want, S, thetas):
            _check_layered(sp, ws, s, mode, ncomp, _tex_of(name, th, ncomp))
        np.testing.assert_allclose(lnl, want_lnl[:64], rtol=LNL_RTOL[mode])
        theta = u.copy()
        point_layered = run.loglikelihood(theta)
        assert point_layered != point_summed and point_layered == run.loglikelihood(u.copy())
        assert point_layered == pytest.approx(restated(nfo, engine, name, rows, theta)[2], rel=LNL_RTOL[mode])
        assert point_layered == run.loglikelihood_batch(np.tile(u, (70, 1)))[69]
        _ffi.check(lib.nfa_specset_set_layered(handle, 0))
        assert lib.nfa_specset_layered(handle) == 0
        spec, lnl = run.predict_batch(np.array(thetas[:64]))
        assert np.array_equal(spec, summed_spec) and np.array_equal(lnl, summed_lnl), turn
        assert run.loglikelihood(u.copy()) == point_summed
    # the Gaussian model is refused with a message, and stays what it was
    x = rows[0][0]
    g = engine.GaussianRunner.from_data([x, rows[0][1], NOISE, float(x[N_CHAN // 2])], None, ncomp=2)
    with pytest.raises(engine.EngineError, match='no optical depth'):
        _ffi.check(lib.nfa_specset_set_layered(g._ss.handle, 1))
    assert lib.nfa_specset_layered(g._ss.handle) == 0
    with pytest.raises(engine.EngineError, match='null argument'):
        _ffi.check(lib.nfa_specset_set_layered(None, 1))


def test_the_resident_kernel_refuses_a_layered_runner(engine, mode_guard):
    from nestfit_amd.ring import RingServer
    for name in ('ammonia', 'lines', 'filled'):
        run = _runner(engine, name, _data_rows(name, engine, seed=2), _simple_priors(engine, _ranges(name)), 1, layered=True)
        with RingServer(f'nfa_test_ring_layer_{os.getpid()}', n_slots=1, runner=run) as server:
            with pytest.raises(engine.EngineError, match='no form for layered transfer: use nfa_ring_serve'):
                server.serve_device(lifetime_ms=20, idle_ms=100)
        u = np.full(run.ndim, 0.5)                                        # ... and a single point takes the batch path
        assert np.isfinite(run.loglikelihood(u))


@pytest.mark.parametrize('mode', MODES)
def test_nan_and_minus_infinity_behave_as_in_the_summed_set(engine, mode, mode_guard):
    """A NaN parameter: NaN lnL in the rows where the summed runner gives NaN, the other rows untouched.  lnff = -inf in front: the layer
    neither adds nor absorbs -- the back layer alone, exactly."""
    engine.set_exp_mode(mode)
    rows, thetas, _, _, _, _ = _reference('ammonia', 2)
    run, summed = _runner(engine, 'ammonia', rows, None, 2, layered=True), _runner(engine, 'ammonia', rows, None, 2)
    good, lnl_good = run.predict_batch(np.array(thetas[:64]))
    bad = np.array(thetas[:64])
    bad[(5, 17, 40, 63), (0, 5, 6, 9)] = np.nan                           # voff, tex, ntot, sigm of one layer or the other
    spec, lnl = run.predict_batch(bad)
    _, lnl_s = summed.predict_batch(bad)
    assert np.array_equal(np.isnan(lnl), np.isnan(lnl_s)) and np.isnan(lnl).any()     # (a NaN voff: no window, the layer is skipped)
    keep = ~np.isin(np.arange(64), (5, 17, 40, 63))
    assert np.array_equal(lnl[keep], lnl_good[keep]) and np.array_equal(spec[keep], good[keep]) and np.isfinite(lnl_good).all()
    rows, thetas, _, _, _, _ = _reference('filled', 2)
    two, one = _runner(engine, 'filled', rows, None, 2, layered=True), _runner(engine, 'filled', rows, None, 1, layered=True)
    gone = np.array(thetas[:64])
    gone[:, 11] = -np.inf                                                 # the front layer fills nothing
    spec, lnl = two.predict_batch(gone)
    want_spec, want_lnl = one.predict_batch(np.ascontiguousarray(gone[:, 0::2]))
    assert np.array_equal(spec, want_spec) and np.abs(want_spec).max() > 0.05
    np.testing.assert_allclose(lnl, want_lnl, rtol=LNL_RTOL[mode])
    assert not np.array_equal(two.predict_batch(np.array(thetas[:64]))[0], want_spec)


# ---------------------------------------------------------------------------- sampling
#   voff, tex, ltau, sigm of the back layer (warm, broad, thick) and of the front one (cold, narrow) at the same velocity
TRUTH_BACK, TRUTH_FRONT = (0.3, 14.0, 0.7, 1.1), (0.3, 4.0, 0.3, 0.35)
TRUTH_FIT = np.array([v for pair in zip(TRUTH_BACK, TRUTH_FRONT) for v in pair])
FIT_RANGES = [(-2, 2), (2.8, 25.0), (-1.0, 1.5), (0.15, 1.8)]


def test_run_multinest_fits_a_self_absorbed_line(engine, nfo, mode_guard):
    """One spectrum of one single line: a warm broad thick layer behind a cold narrow one at the same velocity, noise 0.02 K.
    The layered two-component fit recovers both tex within its posterior widths; the summed two-component fit of the same
    data cannot make the dip, and its best lnL is far below the layered one's."""
    from nestfit_amd import sampler
    table = engine.LineTable(72.4e9, [0.0], [1.0], name='one')
    x = table.nu * (1.0 - np.linspace(12.0, -12.0, N_CHAN) / hfr.CKMS)
    tbg = hfr.tbg_of(nfo, x)
    clean, S = lay.hf_layered(nfo, x, tbg, hfr.table_of(table), TRUTH_FIT)
    centre = np.argmax(S)
    assert clean[centre] < 0.6 * clean.max() and clean.min() >= 0                      # self-absorbed: a dip between two horns
    noise = 0.02
    data = clean + np.random.default_rng(17).normal(0, noise, N_CHAN)
    ut = _simple_priors(engine, FIT_RANGES)
    best = {}
    for layered in (True, False):
        run = engine.HyperfineRunner.from_data([[x, data, noise, table]], ut, ncomp=2, layered=layered)
        res = sampler.run_multinest(run, sampler.Dumper(sampler.MemoryGroup()), nlive=200, seed=5)
        best[layered] = (res.max_loglike, res)
    (lnl_lay, res), (lnl_sum, res_sum) = best[True], best[False]
    mean, std = res.param_constr[0], res.param_constr[1]
    print(f'layered: best lnL {lnl_lay:.1f}, lnZ {res.lnZ:.1f} +- {res.lnZ_err:.2f}; summed: best lnL {lnl_sum:.1f}, lnZ {res_sum.lnZ:.1f} +- '
          f'{res_sum.lnZ_err:.2f}; layered mean {mean}, std {std}, truth {TRUTH_FIT}')
    for k in (2, 3):                                                                   # tex of the back and of the front layer
        assert abs(mean[k] - TRUTH_FIT[k]) < 5 * std[k], (k, mean[k], std[k])
    assert std[2] < 3.0 and std[3] < 1.0                                               # constrained, not the prior's width
    assert lnl_lay - lnl_sum > 100 * max(res.lnZ_err, res_sum.lnZ_err) and lnl_lay - lnl_sum > 50


# ---------------------------------------------------------------------------- the cube route
def test_cube_route_on_the_device(engine, nfo, tmp_path, mode_guard):
    """A 4 x 4 cube of self-absorbed lines through CubeFitter(runner_kwargs={'layered': True}): the store carries `layered`,
    postprocess_run writes model_spec_total, and that is predict_batch of a layered runner at the MAP parameters."""
    from nestfit_amd import hyperfine
    from nestfit_amd import postprocess as pp
    from nestfit_amd.cubeio import CubeStack, DataCube, SimpleCube
    from nestfit_amd.fitter import CubeFitter
    from nestfit_amd.store import HdfStore
    table = engine.LineTable(72.4e9, [0.0], [1.0], name='one')
    n_chan, n_side, noise = 128, 4, 0.02
    x = table.nu * (1.0 - np.linspace(8.0, -8.0, n_chan) / hfr.CKMS)
    tbg = hfr.tbg_of(nfo, x)
    rng = np.random.default_rng(31)
    data = np.random.default_rng(1).normal(0, noise, (n_chan, n_side, n_side))
    for k in range(16):
        truth = TRUTH_FIT + np.concatenate([np.repeat(rng.uniform(-0.3, 0.3), 2), rng.uniform(-0.5, 0.5, 2), rng.uniform(-0.1, 0.1, 2), [0, 0]])
        data[:, k // n_side, k % n_side] += lay.hf_layered(nfo, x, tbg, hfr.table_of(table), truth)[0]
    hdr = {'SIMPLE': True, 'BITPIX': -64, 'NAXIS': 3, 'NAXIS1': n_side, 'NAXIS2': n_side, 'NAXIS3': n_chan,
           'BUNIT': 'K', 'CTYPE1': 'RA---SIN', 'CTYPE2': 'DEC--SIN', 'CTYPE3': 'FREQ', 'CUNIT3': 'Hz',
           'CRVAL3': float(x[0]), 'CDELT3': float(x[1] - x[0]), 'CRPIX3': 1.0, 'RESTFRQ': table.nu}
    stack = CubeStack([DataCube(SimpleCube(hdr, data), noise, lines=table)])
    fitter = CubeFitter(stack, _simple_priors(engine, FIT_RANGES), hyperfine.HyperfineRunner, runner_kwargs={'layered': True},
                        lnZ_thresh=11, ncomp_max=2, mn_kwargs={'nlive': 100, 'tol': 1.0, 'seed': 5}, nlive_snr_fact=0)
    assert fitter.layered is True
    runner, _, _ = stack.to_device(None, ncomp=2, model=3, layered=True)
    assert runner.layered is True and runner.ndim == 8
    path = str(tmp_path / 'run')
    fitter.fit_cube(path, nproc=1)
    with HdfStore(path) as store:
        assert bool(store.hdf.attrs['layered']) is True and store.read_model_layered() is True
        groups = list(store.iter_pix_groups())
        assert len(groups) == 16 and sum(g.attrs['nbest'] == 2 for g in groups) >= 12      # the dip asks for the second layer
        with pytest.raises(ValueError, match='fitted with layered components'):         # before any product is written
            pp.postprocess_run(store, stack, runner=stack.to_device(None, ncomp=1, model=3)[0])
        pp.postprocess_run(store, stack, evid_kernel=0.6, post_kernel=pp.gaussian_kernel(0.6))
        pmap = np.asarray(store.hdf[f'{store.dpath}/nbest_MAP'])                         # (m, p, b, l)
        per_layer = np.asarray(store.hdf[f'{store.dpath}/model_spec/spec0'])            # (m, S, b, l)
        total = np.asarray(store.hdf[f'{store.dpath}/model_spec_total/spec0'])          # (S, b, l)
        assert per_layer.shape == (2, n_chan, 4, 4) and total.shape == (n_chan, 4, 4) and total.dtype == np.float32
        xs = stack.cubes[0].xarr
        dips = 0
        for b in range(4):
            for l in range(4):
                n = int(np.all(np.isfinite(pmap[:, :, b, l]), axis=1).sum())
                assert n >= 1
                theta = np.ascontiguousarray(pmap[:n, :, b, l].T.reshape(1, -1))         # parameter-major
                one = stack.to_device(None, ncomp=n, model=3, lon=np.array([l]), lat=np.array([b]), layered=True)[0]
                one.set_exp_mode('table')
                got, _ = one.predict_batch(np.zeros(1, dtype=np.int32), theta)
                assert np.array_equal(total[:, b, l], got[0].astype(np.float32))
                ws, s = lay.hf_layered(nfo, xs, hfr.tbg_of(nfo, xs), hfr.table_of(table), theta[0])
                _check_layered(got[0], ws, s, 'table', n, theta[0][n:2 * n])
                # the cubes of the single layers are each layer seen alone: they no longer add up to the model
                if n == 2:
                    alone = per_layer[:, :, b, l].sum(axis=0)
                    dips += int(np.abs(alone - total[:, b, l]).max() > 0.1 * total[:, b, l].max())
        assert dips >= 12
