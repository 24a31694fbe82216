"""Which likelihoods a spectra set takes beside the ones it has is one table, csrc/nfa_set_rules.h: plain C++17 that g++
compiles alone.  Before the table each nfa_specset_set_* call carried its own chain of `if`s; this test holds set_refusal to
those eight chains, transcribed below with their messages, for every set (512 masks of the nine features) and every
request, on a machine without a GPU.  The engine's part is the word it forms from a set (specset_has) and the condition
under which a setter asks (a request that switches the feature on); the GPU tests of each feature go through both."""
import ctypes as C
import itertools
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
MASK, BASELINE, CALIB, NMARG, CORR, RESP, TMPL, CONT, ROBUST = (1 << i for i in range(9))
T_BASELINE, T_CALIB, T_NMARG, T_CORR, T_RESP, T_TMPL, T_CONT, T_ROBUST = range(8)
# the feature a request switches on
GIVES = {T_BASELINE: BASELINE, T_CALIB: CALIB, T_NMARG: NMARG, T_CORR: CORR, T_RESP: RESP, T_TMPL: TMPL, T_CONT: CONT, T_ROBUST: ROBUST}

NMARG_CALIB = "a set takes a calibration uncertainty or a noise uncertainty, not both: a calibrated set's part is no chi^2"
CONT_CALIB = 'a set with a calibration uncertainty takes no continuum background'
CONT_CORR = 'a set with correlated channel noise takes no continuum background'
CONT_RESP = 'a set with a channel response takes no continuum background'
CONT_TMPL = 'a set with nuisance templates takes no continuum background'
rob_refuses = 'a set with a robust likelihood takes no {}'.format
rob_refused = 'a set with {} takes no robust likelihood'.format


def chain(has, takes):
    """The setters' chains as they stood, one `if` per line in their order: the first that applies is the refusal."""
    if takes == T_BASELINE:                     # nfa_specset_set_baseline, order >= 0
        if has & RESP: return 'a set with a channel response takes no baseline'
        if has & CORR: return 'a set with correlated channel noise takes no baseline'
        if has & ROBUST: return rob_refuses('baseline')
    if takes == T_CALIB:                        # nfa_specset_set_calibration, some s > 0
        if has & RESP: return 'a set with a channel response takes no calibration uncertainty'
        if has & CORR: return 'a set with correlated channel noise takes no calibration uncertainty'
        if has & TMPL: return 'a set with nuisance templates takes no calibration uncertainty'
        if has & NMARG: return NMARG_CALIB
        if has & CONT: return CONT_CALIB
        if has & ROBUST: return rob_refuses('calibration uncertainty')
    if takes == T_NMARG:                        # nfa_specset_set_noise_uncertainty, some f > 0
        if has & CALIB: return NMARG_CALIB
        if has & ROBUST: return rob_refuses('noise uncertainty')
    if takes == T_CORR:                         # nfa_specset_set_correlation, some rho != 0
        if has & MASK: return 'a set with a masked channel takes no noise correlation'
        if has & BASELINE: return 'a set with a baseline takes no noise correlation'
        if has & CALIB: return 'a set with a calibration uncertainty takes no noise correlation'
        if has & TMPL: return 'a set with nuisance templates takes no noise correlation'
        if has & CONT: return CONT_CORR
        if has & ROBUST: return rob_refuses('noise correlation')
    if takes == T_RESP:                         # nfa_specset_set_response, some taps not the identity
        if has & MASK: return 'a set with a masked channel takes no channel response'
        if has & BASELINE: return 'a set with a baseline takes no channel response'
        if has & CALIB: return 'a set with a calibration uncertainty takes no channel response'
        if has & TMPL: return 'a set with nuisance templates takes no channel response'
        if has & CONT: return CONT_RESP
        if has & ROBUST: return rob_refuses('channel response')
    if takes == T_TMPL:                         # nfa_specset_set_templates, some spectrum with templates
        if has & RESP: return 'a set with a channel response takes no nuisance templates'
        if has & CORR: return 'a set with correlated channel noise takes no nuisance templates'
        if has & CALIB: return 'a set with a calibration uncertainty takes no nuisance templates'
        if has & CONT: return CONT_TMPL
        if has & ROBUST: return rob_refuses('nuisance templates')
    if takes == T_CONT:                         # nfa_specset_set_continuum, some Tc > 0
        if has & RESP: return CONT_RESP
        if has & CORR: return CONT_CORR
        if has & CALIB: return CONT_CALIB
        if has & TMPL: return CONT_TMPL
        if has & ROBUST: return rob_refuses('continuum background')
    if takes == T_ROBUST:                       # nfa_specset_set_robust, some nu > 0
        if has & BASELINE: return rob_refused('a baseline')
        if has & TMPL: return rob_refused('nuisance templates')
        if has & CALIB: return rob_refused('a calibration uncertainty')
        if has & RESP: return rob_refused('a channel response')
        if has & CORR: return rob_refused('correlated channel noise')
        if has & NMARG: return rob_refused('a noise uncertainty')
        if has & CONT: return rob_refused('a continuum background')
    return None


SHIM = r'''
#include "nfa_set_rules.h"
extern "C" {
const char *refusal(unsigned has, int takes) { return set_refusal(has, takes); }
int constants(int i) {
    const int c[] = {SET_HAS_MASK, SET_HAS_BASELINE, SET_HAS_CALIB, SET_HAS_NMARG, SET_HAS_CORR, SET_HAS_RESP, SET_HAS_TMPL, SET_HAS_CONT,
                     SET_HAS_ROBUST, SET_HAS_ALL, SET_TAKES_BASELINE, SET_TAKES_CALIB, SET_TAKES_NMARG, SET_TAKES_CORR, SET_TAKES_RESP,
                     SET_TAKES_TMPL, SET_TAKES_CONT, SET_TAKES_ROBUST, SET_TAKES_N};
    return c[i];
}
}
'''


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('set_rules')
    src = tmp / 'rules.cpp'
    src.write_text(SHIM)
    so = tmp / 'librules.so'
    res = subprocess.run(['g++', '-std=c++17', '-Wall', '-Werror', '-O1', '-shared', '-fPIC', f'-I{ROOT / "nestfit_amd" / "csrc"}',
                          str(src), '-o', str(so)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    lib = C.CDLL(str(so))
    lib.refusal.restype = C.c_char_p
    lib.refusal.argtypes = [C.c_uint, C.c_int]
    assert [lib.constants(i) for i in range(19)] == [MASK, BASELINE, CALIB, NMARG, CORR, RESP, TMPL, CONT, ROBUST, 511] + list(range(8)) + [8]
    return lib


def refusal(lib, has, takes):
    why = lib.refusal(has, takes)
    return None if why is None else why.decode()


def test_every_set_and_every_request_is_refused_as_the_setters_chains_refused_it(lib):
    """All 512 sets x 8 requests: the same message byte for byte, the first of the chain where several features refuse, and
    null exactly where the chain ran through."""
    n_refused = 0
    for has, takes in itertools.product(range(512), range(8)):
        want = chain(has, takes)
        assert refusal(lib, has, takes) == want, (has, takes)
        n_refused += want is not None
    assert 0 < n_refused < 512 * 8
    # a set with nothing takes everything; a request the table does not know is refused nothing
    assert all(refusal(lib, 0, takes) is None for takes in range(8))
    assert all(refusal(lib, has, 8) is None and refusal(lib, has, -1) is None for has in range(512))


def test_an_incompatible_pair_is_refused_in_either_order(lib):
    """Whichever of two incompatible likelihoods comes second, its setter refuses.  (A masked channel comes with the set's
    creation: no setter gives it, so it is asked about from one side only.)"""
    pairs = 0
    for a, b in itertools.permutations(range(8), 2):
        if refusal(lib, GIVES[a], b) is None:
            continue
        assert refusal(lib, GIVES[b], a) is not None, (a, b)
        pairs += 1
    # 19 pairs, each counted from both sides: a robust likelihood with the other seven; a calibration with the other six
    # but a baseline; a baseline with a correlation and a response; a correlation and a response each with templates and a
    # continuum; templates with a continuum
    assert pairs == 2 * (7 + 5 + 2 + 4 + 1)
    # the groups that say it in the same words from either setter
    assert refusal(lib, NMARG, T_CALIB) == refusal(lib, CALIB, T_NMARG) == NMARG_CALIB
    for other, t_other, why in ((CALIB, T_CALIB, CONT_CALIB), (CORR, T_CORR, CONT_CORR), (RESP, T_RESP, CONT_RESP), (TMPL, T_TMPL, CONT_TMPL)):
        assert refusal(lib, other, T_CONT) == refusal(lib, CONT, t_other) == why
    # no feature refuses itself: a setter replaces what its own call gave
    assert all(refusal(lib, GIVES[t], t) is None for t in range(8))
