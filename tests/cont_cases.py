"""The model cases of tests/test_continuum.py, so that tests/test_continuum_cpu.py can hold the restatement's own spectra to
what the GPU test says of its draws: at Tc = 35 K every row with a non-zero channel is negative there; at the model's low
Tc each sign occurs in at least a tenth of the rows.

The draws are tests/test_layered.py's (`draw_layers`: stacked thick layers in the even rows, anything from tau < 1e-3 to
tau > 32 in the odd ones), 200 rows of 300 channels.  Every case has TWO spectra, so that a spectrum with Tc = 0 stands beside
one with a continuum: N2H+ 2-1 beside 1-0 (the set is WIDE by the 40 lines of 2-1), the three-line table twice.  The filled
mix draws tex over 8..30 K, not test_layered's 8..55 K: the high continuum, 35 K, is to lie above the model's whole tex range.

The low Tc per model, from J(tex) - J(Tcmb) over the model's tex range at its frequency: NH3 at 23.7 GHz, tex 3.5..9 K, is
0.8..6.3 K: Tc = 3 K; N2H+ 2-1 at 186 GHz, tex 3.5..20 K, is 0.4..15.5 K: 3 K absorbs in about a fifth of the components;
the three lines at 88.6 GHz likewise; the mix, tex 8..30 K: 12 K."""
import functools

import numpy as np

import cont_restatement as cr
import hf_restatement as hfr

TC_HIGH = 35.0
TC_LOW = {'ammonia': 3.0, 'n2hp': 3.0, 'lines': 3.0, 'filled': 12.0}
FILLED_TEX = (8.0, 30.0)
CASES = [('ammonia', 1), ('ammonia', 2), ('ammonia', 3), ('ammonia', 4), ('n2hp', 2), ('lines', 3), ('filled', 2)]


def pairs(name):
    """The two continuum rows [n_spec = 2] of a case: 35 K beside 0, and the model's low Tc on both spectra (0.8 of it on the
    second, so that a slip between the spectra shows)."""
    return {'high': (TC_HIGH, 0.0), 'low': (TC_LOW[name], 0.8 * TC_LOW[name])}


def spectra(name, na):
    """[(axis, what the restatement and the runner need of the spectrum)]: two spectra per case."""
    import test_layered as tl
    from test_sibling_models import n2hp_axis
    if name == 'n2hp':
        return [(n2hp_axis(2, tl.N_CHAN), 2), (n2hp_axis(1, tl.N_CHAN), 1)]
    if name == 'lines':
        return tl._spectra(name, na) * 2
    return tl._spectra(name, na)


def data_rows(name, na, seed, chan=False):
    """The rows [axis, data, noise, what]: noise of 0.2 K about zero; chan: a noise per channel with masked channels astride
    the first seam (tmpl_cases.channel_noise)."""
    import tmpl_cases as tcs
    from test_lte_mix import NOISE
    rng = np.random.default_rng(seed)
    rows = []
    for k, (x, what) in enumerate(spectra(name, na)):
        noise = tcs.channel_noise(x.size, 31 + k, base=NOISE) if chan else NOISE
        scatter = np.where(np.isfinite(noise), noise, 0.0) * np.ones(x.size)
        rows.append([x, rng.normal(0, 1, x.size) * scatter, noise, what])
    return rows


def draw(rng, name, ncomp, row):
    import test_layered as tl
    theta = tl.draw_layers(rng, name, ncomp, row)
    if name == 'filled':                                      # tex from 8..55 K to 8..30 K, linearly
        lo, hi = tl.MODELS[name]['tex']
        r = tl.MODELS[name]['tex_row']
        theta[r * ncomp:(r + 1) * ncomp] = FILLED_TEX[0] + (theta[r * ncomp:(r + 1) * ncomp] - lo) * (FILLED_TEX[1] - FILLED_TEX[0]) / (hi - lo)
    return theta


def components(nfo, na, name, axes, theta):
    """What `evaluate` needs of one parameter vector, per spectrum: the oracle's terms, or the layers and the background."""
    import test_layered as tl
    out = []
    for x, what in axes:
        if name == 'ammonia':
            out.append(('oracle', cr.amm_terms(nfo, x, what, theta)[0]))
        elif name == 'n2hp':
            out.append(('oracle', cr.nnhp_terms(nfo, x, what, theta)[0]))
        elif name == 'lines':
            out.append(('layers', cr.hf_layers(nfo, x, hfr.table_of(what), theta), x, hfr.tbg_of(nfo, x)))
        else:
            mol, ks, iso, isos = tl._species()
            out.append(('layers', cr.mix_layers(nfo, x, what, (mol, iso), theta, fill=name == 'filled'), x, hfr.tbg_of(nfo, x)))
    return out


def put_before(nfo, comps, tcs, layered):
    """(spectra concatenated, S likewise) of `components`' result before the continuum row `tcs`."""
    out = []
    for c, tc in zip(comps, tcs):
        out.append(cr.through_oracle(c[1], tc, layered) if c[0] == 'oracle' else cr.through(nfo, c[2], c[3], c[1], tc, layered))
    return np.concatenate([p for p, _ in out]), np.concatenate([s for _, s in out])


@functools.lru_cache(maxsize=None)
def reference(name, ncomp):
    """(axes, thetas[200, ndim], the components of every row), computed once."""
    import nestfit_amd as na
    from oracle import nfo
    from test_lte_mix import N_ROWS
    axes = spectra(name, na)
    rng = np.random.default_rng(9100 + 10 * len(name) + ncomp)
    thetas = np.stack([draw(rng, name, ncomp, k) for k in range(N_ROWS)])
    thetas.setflags(write=False)
    return axes, thetas, [components(nfo, na, name, axes, th) for th in thetas]


@functools.lru_cache(maxsize=None)
def evaluate(name, ncomp, which, layered):
    """(spectra[200, chan_tot], S) of the restatement for the case's continuum row `which` ('high' / 'low'), read-only."""
    from oracle import nfo
    _, _, comps = reference(name, ncomp)
    out = [put_before(nfo, c, pairs(name)[which], layered) for c in comps]
    spec, S = np.stack([p for p, _ in out]), np.stack([s for _, s in out])
    spec.setflags(write=False), S.setflags(write=False)
    return spec, S


def check_draws(name, ncomp, which, layered):
    """What the draws exercise, asserted of the restatement's own spectra (the first spectrum, whose Tc is not 0): returns
    (rows that absorb, rows that emit)."""
    spec, S = evaluate(name, ncomp, which, layered)
    n = spec.shape[1] // 2
    p, s = spec[:, :n], S[:, :n]
    assert S.max() > 1.0
    if which == 'high':
        live = s != 0
        assert live.any(axis=1).sum() > 0.9 * len(p) and (p[live] < 0).all()           # negative wherever a component has optical depth
        assert (spec[:, n:] >= 0).all() and spec[:, n:].max() > 0.05                  # ... and the spectrum beside it, Tc = 0, emits
        return int(live.any(axis=1).sum()), 0
    absorb = int((p.min(axis=1) < -1e-3).sum())
    emit = int((p.max(axis=1) > 1e-3).sum())
    assert absorb >= len(p) // 10 and emit >= len(p) // 10, (name, ncomp, absorb, emit)
    return absorb, emit
