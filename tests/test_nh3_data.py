"""Cross-checks the line-data header against the literals in the reference text, recorded as numbers in
tests/golden/reference_literals.json (tests/golden/make_reference_literals.py reads them from the reference's text)."""
import json
import re
from pathlib import Path

import pytest

GOLDEN = Path(__file__).resolve().parent / 'golden' / 'reference_literals.json'


@pytest.fixture(scope='module')
def literals():
    return json.loads(GOLDEN.read_text())


def test_line_data_matches_reference_text(nfo, literals):
    ref = literals['nh3']
    lib = nfo.lib()
    nhf = ref['NHF']
    assert nhf == [lib.nfo_trans_nhf(t) for t in range(1, 10)]
    assert ref['NU'] == [lib.nfo_trans_nu(t) for t in range(1, 10)]
    assert ref['EA'][:9] == [lib.nfo_trans_ea(t) for t in range(1, 10)]
    for t in range(1, 10):
        v = ref['VOFF'][t - 1]
        w = ref['TAU_WTS'][t - 1]
        assert len(v) == len(w) == nhf[t - 1]
        assert v == [lib.nfo_trans_voff(t, i) for i in range(nhf[t - 1])]
        assert w == [lib.nfo_trans_tau_wt(t, i) for i in range(nhf[t - 1])]


def test_weights_are_normalised(nfo):
    lib = nfo.lib()
    for t in range(1, 10):
        n = lib.nfo_trans_nhf(t)
        tot = sum(lib.nfo_trans_tau_wt(t, i) for i in range(n))
        assert tot == pytest.approx(1.0, abs=2e-3)


def test_constants_match_reference_text(nfo, literals):
    """The physical and spectroscopic constants of csrc/nh3_data.h (shared by the engine and the oracle: a wrong literal
    would be common to both) against the reference's own text: model_includes.pxi:27-36, ammonia.pyx:14-30,
    hyperfine.pyx:10-16, core.pyx:20."""
    ref = literals['constants']
    hdr = (Path(__file__).resolve().parent.parent / 'nestfit_amd' / 'csrc' / 'nh3_data.h').read_text()

    def mine(name, new_const=True):
        ms = re.findall(rf'#define {name}\s+([-+0-9.eE]+)', hdr)
        assert ms, name
        return float(ms[-1] if new_const and len(ms) > 1 else ms[0])
    assert literals['flags'] == {'__NEW_CONST': True, '__APPROX': True}      # the constant set the reference ships
    for ref_name, my_name in (('CKMS', 'NFA_CKMS'), ('CCMS', 'NFA_CCMS'), ('H', 'NFA_H'), ('KB', 'NFA_KB')):
        assert mine(my_name) == ref[ref_name]
    assert mine('NFA_TCMB') == ref['TCMB']
    assert mine('NFA_BROT') == ref['BROT']
    assert mine('NFA_CROT') == ref['CROT']
    assert mine('NFA_NPART') == ref['NPART'] and mine('NFA_N_LEVELS') == ref['N_LEVELS']
    assert mine('NFA_N_PARAMS') == ref['N_PARAMS']
    assert mine('NFA_MAX_HF_N') == ref['MAX_HF_N']
    # the 1/(e^x - 1) table: 1000 points between (h 23 GHz / k) / 8 K and (h 28 GHz / k) / 2.7 K
    t0 = literals['t0_table']
    assert ref['T0_SIZE'] == 1000 and (t0['lo_hz'], t0['hi_hz']) == (23.0e9, 28.0e9)
    assert (t0['lo_tex'], t0['hi_tex']) == (8.0, 2.7)
    lib = nfo.lib()
    assert lib.nfo_t0_xmin() == ref['H'] * t0['lo_hz'] / ref['KB'] / t0['lo_tex']
    assert lib.nfo_t0_xmax() == ref['H'] * t0['hi_hz'] / ref['KB'] / t0['hi_tex']
    assert ref['FWHM'] == 2.3548200450309493
    # Swift et al. 2005 eq. A6 literals and the (J, K) ladder of the partition sum
    assert literals['swift_a6'] == {'a': 41.18, 'b': 15.7, 'c': 0.6}
