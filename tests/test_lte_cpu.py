"""The LTE model's host side (nestfit_amd/lte.py) without a GPU: `Molecule`, `LteLines`, the module's metadata and the
store round trip of the tables.  The test species is a rigid linear rotor made from closed forms (tests/lte_restatement.py)."""
import math

import numpy as np
import pytest

import hf_restatement as hfr
import lte_restatement as lr

B_ROT, MU = 46.5e9, 3.4e-18            # Hz, esu cm: 1-0 at 93 GHz


def rotor_species(na, n_q=32, t_lo=5.0, t_hi=40.0, B=B_ROT, mu=MU, name='rotor'):
    """(molecule, 1-0 with a made-up three-line structure, 2-1 as one line, 3-2 as two lines)."""
    temps = np.geomspace(t_lo, t_hi, n_q)
    mol = na.Molecule(name, temps, lr.rotor_partition(B, temps))
    t10 = mol.transition(*lr.rotor_transition(B, mu, 0), voff=[-7.1, 0.0, 4.9], tau_wts=[0.2, 0.5, 0.3], name='1-0')
    t21 = mol.transition(*lr.rotor_transition(B, mu, 1), name='2-1')
    t32 = mol.transition(*lr.rotor_transition(B, mu, 2), voff=[-2.2, 1.3], tau_wts=[0.4, 0.6], name='3-2')
    return mol, t10, t21, t32


def _trans(t):
    return t.nu, t.e_up, t.g_up, t.a_ul


def test_tau_main_equals_the_restatement():
    import nestfit_amd as na
    rng = np.random.default_rng(1)
    mol, t10, t21, t32 = rotor_species(na)
    worst = 0.0
    for t in (t10, t21, t32):
        for _ in range(200):
            tex, lncol, sigm = 10 ** rng.uniform(0.4, 1.9), rng.uniform(11, 15), 10 ** rng.uniform(-1.3, 0.5)
            want = lr.tau_main(_trans(t), mol.q_temp, mol.q_val, tex, lncol, sigm)
            got = float(t.tau_main(tex, lncol, sigm))
            worst = max(worst, abs(got - want) / want)
    print(f'tau_main: worst relative difference {worst:.2e}')
    assert worst < 1e-14
    # broadcasting, and what is not an ordinary positive number gives NaN
    grid = t10.tau_main(np.array([5.0, 10.0])[:, None], 13.0, np.array([0.3, 0.6, 0.9])[None, :])
    assert grid.shape == (2, 3) and grid[1, 2] == pytest.approx(lr.tau_main(_trans(t10), mol.q_temp, mol.q_val, 10.0, 13.0, 0.9), rel=1e-14)
    with np.errstate(all='ignore'):
        assert np.isnan(t10.tau_main(-3.0, 13.0, 0.5)) and np.isnan(t10.tau_main(np.nan, 13.0, 0.5))
        assert np.isnan(t10.tau_main(10.0, 13.0, np.nan))


def test_line_ratio_is_the_rotors_boltzmann_expression():
    """tau(2-1) / tau(1-0) of a rigid rotor, everything but the level populations and the stimulated-emission factors
    cancelling: nu^3 (J+1)/(2J+3) in A, g_u, 1/nu^3 in fracterm * widthterm leave
        [2 exp(-6 hB/kT) expm1(4 hB/kT)] / [exp(-2 hB/kT) expm1(2 hB/kT)]."""
    import nestfit_amd as na
    _, t10, t21, _ = rotor_species(na)
    for tex in (3.0, 5.0, 7.77, 12.0, 35.0, 80.0):
        x = lr.H * B_ROT / (lr.KB * tex)
        want = 2.0 * math.exp(-6 * x) * math.expm1(4 * x) / (math.exp(-2 * x) * math.expm1(2 * x))
        got = float(t21.tau_main(tex, 13.3, 0.45) / t10.tau_main(tex, 13.3, 0.45))
        assert got == pytest.approx(want, rel=1e-13)


def test_partition_is_the_log_log_interpolation():
    import nestfit_amd as na
    mol, *_ = rotor_species(na)
    ln_t, ln_q = np.log(mol.q_temp), np.log(mol.q_val)
    # at the nodes: the table itself
    np.testing.assert_allclose(mol.partition(mol.q_temp), mol.q_val, rtol=4e-16)
    # between them: numpy.interp on the logarithms
    inside = np.random.default_rng(2).uniform(mol.q_temp[0], mol.q_temp[-1], 300)
    np.testing.assert_allclose(mol.partition(inside), np.exp(np.interp(np.log(inside), ln_t, ln_q)), rtol=1e-14)
    # outside: the end segments' lines continued
    lo, hi = np.array([0.5, 2.0, 4.99]), np.array([40.01, 75.0, 900.0])
    s_lo = (ln_q[1] - ln_q[0]) / (ln_t[1] - ln_t[0])
    s_hi = (ln_q[-1] - ln_q[-2]) / (ln_t[-1] - ln_t[-2])
    np.testing.assert_allclose(mol.partition(lo), np.exp(ln_q[0] + s_lo * (np.log(lo) - ln_t[0])), rtol=1e-14)
    np.testing.assert_allclose(mol.partition(hi), np.exp(ln_q[-2] + s_hi * (np.log(hi) - ln_t[-2])), rtol=1e-14)
    assert mol.partition(900.0) > mol.q_val[-1] and mol.partition(0.5) < mol.q_val[0]
    # ... and the restatement's own look-up is the same function
    for t in np.concatenate([lo, hi, inside[:20], mol.q_temp[[0, 7, 31]]]):
        assert float(mol.ln_partition(t)) == pytest.approx(lr.ln_partition(mol.q_temp, mol.q_val, float(t)), rel=1e-14, abs=1e-15)
    two = na.Molecule('two', [5.0, 40.0], [2.0, 17.0])
    assert float(two.partition(1.0)) == pytest.approx(2.0 * (1.0 / 5.0) ** (math.log(8.5) / math.log(8.0)), rel=1e-14)
    # a high-temperature rotor: Q ~ kT / hB, the table reproduces the direct sum to the interpolation's error
    direct = lr.rotor_partition(B_ROT, [17.3])[0]
    assert float(mol.partition(17.3)) == pytest.approx(direct, rel=2e-4)


def test_every_value_error():
    import nestfit_amd as na
    M = na.Molecule
    for temps, qs in (([10.0], [3.0]), (np.linspace(1, 70, 65), np.linspace(1, 70, 65)),       # n_q outside 2..64
                      ([10.0, 10.0], [1.0, 2.0]), ([20.0, 10.0], [1.0, 2.0]),                    # not strictly ascending
                      ([0.0, 10.0], [1.0, 2.0]), ([-1.0, 10.0], [1.0, 2.0]),                     # not positive
                      ([np.nan, 10.0], [1.0, 2.0]), ([5.0, np.inf], [1.0, 2.0]),
                      ([5.0, 10.0], [0.0, 2.0]), ([5.0, 10.0], [1.0, -2.0]),                     # Q not finite and positive
                      ([5.0, 10.0], [1.0, np.nan]), ([5.0, 10.0], [np.inf, 2.0]),
                      ([5.0, 10.0], [1.0, 2.0, 3.0]), ([[5.0, 10.0]], [[1.0, 2.0]]), (['a', 'b'], [1.0, 2.0])):
        with pytest.raises(ValueError):
            M('bad', temps, qs)
    assert M('edge', np.linspace(1, 64, 64), np.linspace(1, 64, 64)).n == 64 and M('edge', [1, 2], [1, 2]).n == 2
    mol = M('ok', [5.0, 10.0, 20.0], [2.0, 4.0, 9.0])
    good = dict(nu=1e11, e_up=4.0, g_up=3.0, a_ul=1e-5)
    assert mol.transition(**good).n == 1
    for key, bad in (('e_up', -0.1), ('e_up', np.nan), ('e_up', np.inf), ('g_up', 0.0), ('g_up', -1.0), ('g_up', np.nan),
                     ('g_up', np.inf), ('a_ul', 0.0), ('a_ul', -1e-5), ('a_ul', np.nan), ('a_ul', np.inf), ('a_ul', 'x'),
                     ('nu', 0.0), ('nu', np.inf)):
        with pytest.raises(ValueError):
            mol.transition(**{**good, key: bad})
    assert mol.transition(**{**good, 'e_up': 0.0}).e_up == 0.0
    # weights: a sum of 1 within 1e-6, or normalise=True
    for wts in ([0.5, 0.4], [0.5, 0.5 + 3e-6], [2.0, 3.0]):
        with pytest.raises(ValueError, match='sum to 1'):
            mol.transition(**good, voff=[0.0, 1.0], tau_wts=wts)
    assert mol.transition(**good, voff=[0.0, 1.0], tau_wts=[0.5, 0.5 + 5e-7]).n == 2
    t = mol.transition(**good, voff=[0.0, 1.0], tau_wts=[2.0, 3.0], normalise=True)
    assert np.array_equal(t.tau_wts, np.array([2.0, 3.0]) / 5.0)
    # ... and everything a LineTable refuses
    for kw in (dict(voff=[0.0, 1.0], tau_wts=[1.0]), dict(voff=[np.nan], tau_wts=[1.0]), dict(voff=[0.0], tau_wts=[-1.0]),
               dict(voff=np.zeros(51), tau_wts=np.full(51, 1 / 51)), dict(voff=[0.0, 1.0], tau_wts=[0.0, 0.0], normalise=True)):
        with pytest.raises(ValueError):
            mol.transition(**good, **kw)
    with pytest.raises(ValueError, match='Molecule'):
        na.LteLines('ok', 1e11, 4.0, 3.0, 1e-5)
    # a runner's rows name one molecule; spectra take LteLines (checked before any device call)
    other = M('other', [5.0, 10.0, 20.0], [2.0, 4.0, 9.5])
    x = lr.axis(1e11, 64, 10.0)
    rows = [[x, np.zeros(64), 0.1, mol.transition(**good)], [x, np.zeros(64), 0.1, other.transition(**good)]]
    with pytest.raises(ValueError, match='one Molecule'):
        na.LteRunner.from_data(rows, None)
    with pytest.raises(ValueError, match='LteLines'):
        na.LteRunner.from_data([[x, np.zeros(64), 0.1, na.LineTable(1e11, [0.0], [1.0])]], None)
    with pytest.raises(ValueError, match='baseline_order'):
        na.LteRunner.from_data(rows[:1], None, baseline_order=7)


def test_immutable_and_compared_by_value():
    import nestfit_amd as na
    mol, t10, t21, _ = rotor_species(na)
    again, u10, u21, _ = rotor_species(na)
    assert mol == again and hash(mol) == hash(again) and mol is not again
    assert t10 == u10 and hash(t10) == hash(u10) and t21 == u21 and t10 != t21
    assert len({mol, again}) == 1 and len({t10, u10, t21}) == 2
    assert mol != na.Molecule('rotor', mol.q_temp, mol.q_val * 1.01) and mol != na.Molecule('other', mol.q_temp, mol.q_val)
    assert mol != na.Molecule('rotor', mol.q_temp[:-1], mol.q_val[:-1])
    kw = dict(voff=t10.voff, tau_wts=t10.tau_wts)
    nu, e, g, a = _trans(t10)
    assert t10 == mol.transition(nu, e, g, a, name='a label', **kw)                       # the name is a label
    for diff in (mol.transition(nu, e * 1.1, g, a, **kw), mol.transition(nu, e, g + 1, a, **kw), mol.transition(nu, e, g, a * 2, **kw),
                 mol.transition(nu * 1.01, e, g, a, **kw), na.Molecule('rotor', mol.q_temp, mol.q_val * 1.01).transition(nu, e, g, a, **kw)):
        assert t10 != diff
    plain = na.LineTable(nu, t10.voff, t10.tau_wts)
    assert isinstance(t10, na.LineTable) and t10 != plain and plain != t10                # a table alone is no transition
    for obj, key in ((mol, 'name'), (mol, '_q_val'), (t10, 'e_up'), (t10, '_nu'), (t10, 'molecule')):
        with pytest.raises(AttributeError):
            setattr(obj, key, 1.0)
        with pytest.raises(AttributeError):
            delattr(obj, key)
    for arr in (mol.q_temp, mol.q_val, t10.voff, t10.tau_wts):
        with pytest.raises(ValueError):
            arr[0] = 1.0
    assert (t10.molecule is mol) and (t10.n, t21.n) == (3, 1) and t10.name == '1-0'


def test_module_metadata():
    import nestfit_amd as na
    from nestfit_amd import fitter, postprocess
    m, h = na.lte, na.hyperfine
    assert (m.NAME, m.N, m.IX_VCEN, m.IX_SIGM) == ('lte', 4, 0, 3)
    assert m.PAR_NAMES == ['voff', 'tex', 'lncol', 'sigm'] and len(m.PAR_NAMES_SHORT) == 4
    assert len(m.TEX_LABELS) == len(m.TEX_LABELS_WITH_UNITS) == 4
    assert m.TEX_LABELS[0] == h.TEX_LABELS[0] and m.TEX_LABELS[2] != h.TEX_LABELS[2]
    assert m.get_par_names() == m.PAR_NAMES_SHORT and m.get_par_names(2) == [f'{p}{k}' for p in m.PAR_NAMES_SHORT for k in (1, 2)]
    assert m.ModelRunner is na.LteRunner is m.LteRunner and m.ModelSpectrum is na.LteSpectrum and m.model_predict is na.lte_predict
    assert na.Molecule is m.Molecule and na.LteLines is m.LteLines
    assert na.model_module('lte') is m and na.model_module('hyperfine') is h and na.model_module('nope') is None
    assert set(na.MODELS) == {'ammonia', 'diazenylium', 'gaussian'}                     # the registry stays the reference's three
    assert fitter._MODEL_ID['lte'] == postprocess._MODEL_ID['lte'] == 4
    for name in ('lte', 'Molecule', 'LteLines', 'LteSpectrum', 'LteRunner', 'lte_predict'):
        assert name in na.__all__
    from nestfit_amd import _ffi
    assert 'nfa_specset_create_lte' in _ffi.SIGNATURES and hasattr(_ffi.load(), 'nfa_specset_create_lte')


# ---------------------------------------------------------------------------- the cube driver and the store
N_CHAN, NOISE = 64, 0.1


def _stack(na, tables, n=3, seed=0):
    from nestfit_amd.cubeio import CubeStack, DataCube, SimpleCube
    rng = np.random.default_rng(seed)
    cubes = []
    for t in tables:
        x = lr.axis(t.nu, N_CHAN, 14.0)
        hdr = {'SIMPLE': True, 'BITPIX': -64, 'NAXIS': 3, 'NAXIS1': n, 'NAXIS2': n, 'NAXIS3': N_CHAN,
               'BUNIT': 'K', 'CTYPE1': 'RA---SIN', 'CTYPE2': 'DEC--SIN', 'CTYPE3': 'FREQ', 'CUNIT3': 'Hz',
               'CRVAL3': float(x[0]), 'CDELT3': float(x[1] - x[0]), 'CRPIX3': 1.0, 'RESTFRQ': t.nu}
        cubes.append(DataCube(SimpleCube(hdr, rng.normal(0, NOISE, (N_CHAN, n, n))), NOISE, lines=t))
    return CubeStack(cubes)


def _priors(na):
    from scipy import stats
    x = np.linspace(0, 1, 200)
    ranges = [(-4, 4), (3.0, 20), (12.0, 14.5), (0.2, 1.5)]
    return na.PriorTransformer([
        na.Prior(na.Distribution(lo + x * (hi - lo), stats.uniform(lo, hi - lo).pdf(lo + x * (hi - lo))), k)
        for k, (lo, hi) in enumerate(ranges)])


def _stub_backend(fitter, lon, lat, ncomp, nlive, kw):
    """A stand-in for the device: the numpy twin of the sampler on a Gaussian in the unit cube (the store's tables do not
    depend on what was fitted)."""
    from nestfit_amd import sampler

    def loglike(pix, U):
        return -0.5 * np.sum((U - 0.5) ** 2, axis=1) / 0.2 ** 2
    res = sampler.run_nested(loglike, 4 * ncomp, lon.size, nlive=nlive, batch_target=64, **kw)
    return res, np.full(lon.size, -40.0), 2 * N_CHAN


def test_store_round_trip_of_the_tables(tmp_path):
    import nestfit_amd as na
    from nestfit_amd import postprocess as pp
    from nestfit_amd.fitter import CubeFitter
    from nestfit_amd.store import HdfStore
    mol, t10, t21, _ = rotor_species(na)
    stack = _stack(na, [t10, t21])
    fitter = CubeFitter(stack, _priors(na), na.LteRunner, lnZ_thresh=11, ncomp_max=1,
                        mn_kwargs={'nlive': 20, 'tol': 1.0, 'seed': 3, 'maxiter': 120}, nlive_snr_fact=0, fit_backend=_stub_backend)
    assert (fitter.model_id, fitter.n_model, fitter.runner_kwargs) == (4, 4, {})
    path = str(tmp_path / 'run')
    fitter.fit_cube(path, nproc=1)
    with HdfStore(path) as store:
        assert store.hdf.attrs['model_name'] == 'lte' and store.model is na.lte
        assert store.hdf.attrs['n_params'] == 4 and list(store.hdf.attrs['par_names']) == ['voff', 'tex', 'lncol', 'sigm']
        part = store.hdf['/model_partition']
        assert part.attrs['name'] == 'rotor'
        assert np.array_equal(np.asarray(part['temp'][...]), mol.q_temp) and np.array_equal(np.asarray(part['q'][...]), mol.q_val)
        for k, t in enumerate((t10, t21)):
            g = store.hdf[f'/model_lines/spec{k}']
            assert (g.attrs['nu'], g.attrs['e_up'], g.attrs['g_up'], g.attrs['a_ul']) == (t.nu, t.e_up, t.g_up, t.a_ul)
            assert g.attrs['name'] == t.name
            assert np.array_equal(np.asarray(g['voff'][...]), t.voff) and np.array_equal(np.asarray(g['tau_wts'][...]), t.tau_wts)
        back = store.read_model_lines()
        assert back == [t10, t21] and all(isinstance(t, na.LteLines) for t in back)
        assert back[0].molecule == mol and [t.name for t in back] == ['1-0', '2-1']
        assert len(list(store.iter_pix_groups())) == 9
    with HdfStore(path) as store:                                  # reopened
        assert pp.check_model_lines(store, stack) == [t10, t21]
        # another e_up, another partition table, a plain LineTable, another order: refused
        nu, e, g, a = _trans(t21)
        hotter = mol.transition(nu, e * 1.01, g, a, name='2-1')
        mol2, u10, u21, _ = rotor_species(na, t_hi=41.0)
        plain = na.LineTable(t21.nu, t21.voff, t21.tau_wts)
        for tables in ([t10, hotter], [u10, u21], [t10, plain], [t21, t10], [t10]):
            other = _stack(na, tables)
            with pytest.raises(ValueError, match='line tables differ'):
                pp.check_model_lines(store, other)
            with pytest.raises(ValueError, match='line tables differ'):
                pp.postprocess_run(store, other, predict_backend=lambda *a: None)
    # two molecules in one stack: nothing is written
    with pytest.raises(ValueError, match='one Molecule'):
        CubeFitter(_stack(na, [t10, u21]), _priors(na), na.LteRunner, fit_backend=_stub_backend).fit_cube(str(tmp_path / 'two'), nproc=1)
