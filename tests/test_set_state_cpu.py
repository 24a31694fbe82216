"""What a spectra set's options ask of the device is one header, csrc/nfa_set_state.h: plain C++17 that g++ compiles alone.
Before it every nfa_specset_set_* call allocated, pointed and formed for itself, through an apply function per option in
nfa_engine.hip; this test holds set_layout and the stage selection to those functions, transcribed below, for every
set (512 masks of the nine features) on a scalar noise and on a noise per channel, on a machine without a GPU.  The engine's
part is specset_realise, which allocates, forms and frees what the header names; tests/test_set_state.py goes through both."""
import ctypes as C
import itertools
import subprocess
from pathlib import Path

import pytest

from test_set_rules_cpu import BASELINE, CALIB, CONT, CORR, GIVES, MASK, NMARG, RESP, ROBUST, TMPL, chain

ROOT = Path(__file__).resolve().parent.parent
OPTIONS = (BASELINE, CALIB, NMARG, CORR, RESP, TMPL, CONT, ROBUST)
# SB_*: the buffers, and SetChanW
W, WDATA, BL, TP, CAL2, NMARG_B, Q0, Q1, Q2, COEF, RESP_B, TMPL_B, CONT_B, RG, RGD, ROB_B = (1 << i for i in range(16))
QS = Q0 | Q1 | Q2 | COEF
NONE, OWN, Q, ROB_G = range(4)
# UP_*, ST_*
UP_CAL2, UP_CORR, UP_RESP, UP_TMPL, UP_CONT = (1 << i for i in range(5))
ST_ONES, ST_CHAN_WEIGHT, ST_CORR, ST_FORM_Q, ST_ROWSQ, ST_ROB, ST_BL, ST_BL_BASIS, ST_TP, ST_TP_BASIS, ST_NMARG = (1 << i for i in range(8, 19))
STAGES = {'UP_CAL2': UP_CAL2, 'UP_CORR': UP_CORR, 'UP_RESP': UP_RESP, 'UP_TMPL': UP_TMPL, 'UP_CONT': UP_CONT, 'ST_ONES': ST_ONES,
          'ST_CHAN_WEIGHT': ST_CHAN_WEIGHT, 'ST_CORR': ST_CORR, 'ST_FORM_Q': ST_FORM_Q, 'ST_ROWSQ': ST_ROWSQ, 'ST_ROB': ST_ROB,
          'ST_BL': ST_BL, 'ST_BL_BASIS': ST_BL_BASIS, 'ST_TP': ST_TP, 'ST_TP_BASIS': ST_TP_BASIS, 'ST_NMARG': ST_NMARG}


# The options a copy or a stage reads, from the kernels' code (csrc/nfa_device.h) and the comments beside the stages in the
# header -- directly, or through a buffer whose presence or content the option decides: the set's own weights of a scalar noise
# exist for a baseline, a calibration, a continuum, templates, a correlation or a response (NEEDS_W); d_wdata holds Q d under a
# correlation or a response and w d otherwise; totsq is a robust set's k C; the templates' launch reads the baseline order.
NEEDS_W = BASELINE | CALIB | CONT | TMPL | CORR | RESP
READS = {UP_CAL2: CALIB, UP_CORR: CORR | RESP, UP_RESP: RESP, UP_TMPL: TMPL, UP_CONT: CONT, ST_ONES: NEEDS_W, ST_CHAN_WEIGHT: NEEDS_W,
         ST_CORR: CORR | RESP, ST_FORM_Q: CORR | RESP, ST_ROWSQ: CORR | RESP | ROBUST, ST_ROB: ROBUST, ST_BL: BASELINE | CALIB | CONT,
         ST_BL_BASIS: BASELINE | CALIB | CONT, ST_TP: TMPL | BASELINE, ST_TP_BASIS: TMPL | BASELINE, ST_NMARG: NMARG}


def parent_layout(has, chan):
    """(buffers, ones, chan_w source) as the setters of the parent left a set with the features `has`."""
    want_bl = bool(has & (BASELINE | CALIB | CONT))            # the records' function: d.bl_order >= 0 || d.cal2 || d.cont
    want_tp = bool(has & TMPL)                                 # ... d.tmpl != nullptr
    q = bool(has & (CORR | RESP))                              # a correlation or a response, either: Q's arrays
    ones_for_records = not chan and (want_bl or want_tp)       # the records' function: if (!d.chan_w) { ... its ownership flag
    ones_for_q = not chan and q                                # the correlation's: if (!ss->d_w) { ... its own flag
    ones = ones_for_records or ones_for_q
    bufs = 0
    if chan or ones: bufs |= W | WDATA
    if want_bl: bufs |= BL
    if want_tp: bufs |= TMPL_B | TP
    if has & CALIB: bufs |= CAL2
    if has & NMARG: bufs |= NMARG_B
    if q: bufs |= QS
    if has & RESP: bufs |= RESP_B
    if has & CONT: bufs |= CONT_B
    if has & ROBUST: bufs |= RG | RGD | ROB_B
    # the robust setter last: d.chan_w = ss->d_rg; the correlation's: ss->d_q0; the records' function and both removals: ss->d_w
    src = ROB_G if has & ROBUST else Q if q else OWN if chan or ones else NONE
    return bufs, ones, src


def parent_set_data(has, chan):
    """The launches of the parent's nfa_specset_set_data, its if-chain over SpecDev's pointers."""
    bufs, _, src = parent_layout(has, chan)
    if has & ROBUST:                                           # if (ss->dev.rob): the set's own w d and sums, then rob_setup_kernel
        return (ST_CHAN_WEIGHT if bufs & W else 0) | ST_ROWSQ | ST_ROB
    st = ST_CORR if bufs & Q1 else ST_CHAN_WEIGHT if src != NONE else 0    # if (corr_q1) ... else if (chan_w) ...
    st |= ST_ROWSQ
    if bufs & BL: st |= ST_BL
    if bufs & TP: st |= ST_TP
    return st


SHIM = r'''
#include "nfa_set_state.h"
// a set with the features `has` (SET_HAS_* without the mask) at its first (v = 1) or second value
static SetOptions options(unsigned has, int v) {
    SetOptions o;
    if (has & SET_HAS_BASELINE) o.bl_order = v;
    if (has & SET_HAS_CALIB) { o.cal_on = true; o.cal[0] = 0.1 * v; }
    if (has & SET_HAS_NMARG) { o.nunc_on = true; o.nunc[1] = 0.1 * v; }
    if (has & SET_HAS_CORR) { o.corr_on = true; o.rho[0][0] = 0.2 * v; o.rho[0][1] = 0.1; }
    if (has & SET_HAS_RESP) { o.resp_on = true; for (int s = 0; s < 2; ++s) { o.resp[s][1] = o.resp[s][3] = 0.125 * v; o.resp[s][2] = 1.0 - 0.25 * v; } }
    if (has & SET_HAS_TMPL) { o.tmpl_on = true; o.ntmpl[0] = v; }
    if (has & SET_HAS_CONT) o.cont_on = true;
    if (has & SET_HAS_ROBUST) { o.rob_on = true; o.rob[0] = 4.0 * v; }
    return o;
}
extern "C" {
void layout(unsigned has, int chan, unsigned *bufs, int *ones, int *chan_w) {
    const SetLayout L = set_layout(options(has, 1), chan != 0);
    *bufs = L.bufs; *ones = L.ones; *chan_w = (int)L.chan_w;
}
unsigned has_word(unsigned has, int masked) { return set_has(options(has, 1), masked != 0); }
unsigned stages_all(unsigned has, int chan) { return set_stages_all(set_layout(options(has, 1), chan != 0)); }
unsigned stages_data(unsigned has, int chan) { return set_stages_data(set_layout(options(has, 1), chan != 0)); }
unsigned stages_change(unsigned has_a, int va, unsigned has_b, int vb, int chan) {
    const SetOptions a = options(has_a, va), b = options(has_b, vb);
    const bool tmpl = (has_a | has_b) & SET_HAS_TMPL && ((has_a ^ has_b) & SET_HAS_TMPL || va != vb);
    const bool cont = (has_a | has_b) & SET_HAS_CONT && ((has_a ^ has_b) & SET_HAS_CONT || va != vb);
    return set_stages_change(a, set_layout(a, chan != 0), b, set_layout(b, chan != 0), tmpl, cont);
}
int equal(unsigned has_a, int va, unsigned has_b, int vb) { return set_options_equal(options(has_a, va), options(has_b, vb)); }
unsigned constants(int i) {
    const unsigned c[] = {SB_W, SB_WDATA, SB_BL, SB_TP, SB_CAL2, SB_NMARG, SB_Q0, SB_Q1, SB_Q2, SB_CORR, SB_RESP, SB_TMPL, SB_CONT, SB_RG, SB_RGD,
                          SB_ROB, SB_N, CHAN_W_NONE, CHAN_W_OWN, CHAN_W_Q, CHAN_W_ROBUST, UP_CAL2, UP_CORR, UP_RESP, UP_TMPL, UP_CONT, ST_ONES,
                          ST_CHAN_WEIGHT, ST_CORR, ST_FORM_Q, ST_ROWSQ, ST_ROB, ST_BL, ST_BL_BASIS, ST_TP, ST_TP_BASIS, ST_NMARG};
    return c[i];
}
}
'''


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('set_state')
    src = tmp / 'state.cpp'
    src.write_text(SHIM)
    so = tmp / 'libstate.so'
    res = subprocess.run(['g++', '-std=c++17', '-Wall', '-Werror', '-O1', '-shared', '-fPIC', f'-I{ROOT / "nestfit_amd" / "csrc"}',
                          str(src), '-o', str(so)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    lib = C.CDLL(str(so))
    for name in ('has_word', 'stages_all', 'stages_data', 'stages_change', 'constants'):
        getattr(lib, name).restype = C.c_uint
    want = ([1 << i for i in range(16)] + [16, NONE, OWN, Q, ROB_G] + list(STAGES.values()))
    assert [lib.constants(i) for i in range(len(want))] == want
    return lib


def layout(lib, has, chan):
    bufs, ones, src = C.c_uint(), C.c_int(), C.c_int()
    lib.layout(has, int(chan), C.byref(bufs), C.byref(ones), C.byref(src))
    return bufs.value, bool(ones.value), src.value


def exists(has):
    """Whether the rules table lets a set with the features `has` come to be: every feature of it is taken beside the others."""
    takes = {v: k for k, v in GIVES.items()}
    return all(chain(has & ~f, takes[f]) is None for f in OPTIONS if has & f)


def test_every_set_has_the_layout_the_setters_left(lib):
    for has, chan in itertools.product(range(512), (False, True)):
        assert layout(lib, has & ~MASK, chan) == parent_layout(has, chan), (has, chan)
        assert lib.has_word(has & ~MASK, has & MASK) == has | (CORR if has & RESP else 0), has      # a response has the coefficients


def test_the_sets_that_exist(lib):
    n = 0
    for has, chan in itertools.product(range(0, 512, 2), (False, True)):
        if not exists(has):
            continue
        n += 1
        bufs, ones, src = layout(lib, has, chan)
        # exactly one chan_w source, and the one its buffers stand for
        assert src == (ROB_G if bufs & RG else Q if bufs & Q0 else OWN if bufs & W else NONE)
        assert bool(bufs & RG) + bool(bufs & Q0) <= 1
        assert bool(bufs & W) == bool(bufs & WDATA) and bool(bufs & RG) == bool(bufs & RGD) == bool(bufs & ROB_B)
        assert not (ones and chan) and (not ones or bufs & W)
        assert bool(bufs & W) == (chan or ones)
        assert bool(bufs & TP) == bool(has & TMPL) == bool(bufs & TMPL_B)
        assert bool(bufs & Q0) == bool(has & (CORR | RESP)) and all(bool(bufs & b) == bool(bufs & Q0) for b in (Q1, Q2, COEF))
        # the weighted forms read chan_w and wdata: who has records has weights
        assert not bufs & (BL | TP) or src == OWN
    assert n >= 2 * (1 + 8 + 9)         # the set with nothing, with one of the eight, with one of the 28 - 19 pairs that go together, ...


def test_new_data_run_the_stages_of_the_set_data_chain(lib):
    for has, chan in itertools.product(range(0, 512, 2), (False, True)):
        if exists(has):
            assert lib.stages_data(has, chan) == parent_set_data(has, chan), (has, chan)
            assert lib.stages_data(has, chan) & ~lib.stages_all(has, chan) == 0


def test_a_change_runs_what_reads_it_and_nothing_else(lib):
    reads = READS
    assert sorted(reads) == sorted(STAGES.values())
    checked = 0
    for has, chan in itertools.product(range(0, 512, 2), (False, True)):
        if not exists(has):
            continue
        # equal options: nothing
        assert lib.equal(has, 1, has, 1) and lib.stages_change(has, 1, has, 1, chan) == 0
        for f in OPTIONS:
            # on and off beside the rest, and a second value in the place of the first
            if has & f:
                moves = [(has & ~f, 1, has, 1), (has, 1, has & ~f, 1)]
            else:
                continue
            for a, va, b, vb in moves:
                st = lib.stages_change(a, va, b, vb, chan)
                assert not lib.equal(a, va, b, vb)
                for bit, what in reads.items():
                    assert not st & bit or what & f, (a, b, chan, hex(st), hex(bit))
                assert st & ~lib.stages_all(b, chan) == 0
                checked += 1
        # from nothing the set's own option alone: everything it has but the stages whose result the scalar sums already are
        if has and not has & (has - 1):
            st, every = lib.stages_change(0, 1, has, 1, chan), lib.stages_all(has, chan)
            keeps = ST_ROWSQ if has & (BASELINE | CALIB | CONT | TMPL | NMARG) else 0
            keeps |= ST_CHAN_WEIGHT if chan and not has & (CORR | RESP) else 0
            assert st == every & ~keeps, (has, chan, hex(st), hex(every))
    assert checked > 100
    # a second value: the buffers stay, what reads the value runs
    for chan in (False, True):
        assert lib.stages_change(BASELINE, 1, BASELINE, 2, chan) == ST_BL | ST_BL_BASIS
        assert lib.stages_change(BASELINE | TMPL, 1, BASELINE | TMPL, 2, chan) == UP_TMPL | ST_BL | ST_BL_BASIS | ST_TP | ST_TP_BASIS
        assert lib.stages_change(CALIB, 1, CALIB, 2, chan) == UP_CAL2
        assert lib.stages_change(NMARG, 1, NMARG, 2, chan) == ST_NMARG
        assert lib.stages_change(CORR, 1, CORR, 2, chan) == UP_CORR | ST_CORR | ST_FORM_Q | ST_ROWSQ
        assert lib.stages_change(CORR | RESP, 1, CORR | RESP, 2, chan) == UP_CORR | UP_RESP | ST_CORR | ST_FORM_Q | ST_ROWSQ
        assert lib.stages_change(CORR, 1, CORR | RESP, 1, chan) == UP_RESP             # Q is there: the taps alone
        assert lib.stages_change(CONT, 1, CONT, 2, chan) == UP_CONT
        assert lib.stages_change(ROBUST, 1, ROBUST, 2, chan) == ST_ROWSQ | ST_ROB
        # off: the set's own weights behind chan_w again, and its sums
        assert lib.stages_change(CORR, 1, 0, 1, chan) == (ST_CHAN_WEIGHT if chan else 0) | ST_ROWSQ
        assert lib.stages_change(ROBUST, 1, 0, 1, chan) == ST_ROWSQ
        assert lib.stages_change(BASELINE, 1, 0, 1, chan) == 0
