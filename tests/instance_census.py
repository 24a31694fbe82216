"""The census of the likelihood kernel's instances: one case for every (instance, launch form) that lnl_instance_exists
(csrc/nfa_launch_plan.h) admits, 208 of them.  A plain module: tests/test_launch_plan.py holds the table to the rule without a
GPU (the set of pairs the cases name is the set the rule admits, and plan_lnl gives every case its pair), and
tests/instance_census_worker.py launches every case on the device for tests/test_instance_census.py.

A case names its model set, the numerical mode, whether spectra come out, the number of components, the flags of the set
(a noise per channel, a baseline order, filled, layered, a calibration uncertainty), the size of the launch, and the
(instance index, form) it must land on.  Nothing here computes a model of its own: the sets, the parameter draws and the data
are the sibling tests' (test_layered._spectra and draw_layers, test_calibration._data and CAL, test_lte_bands.wide_band), the
wanted spectra are layer_restatement's, the wanted lnL calib_restatement's.

    narrow sets       NH3 (1,1) + (2,2), 300 channels                               kinds without the filled bit
    narrow, filled    the filled mix of test_layered ('filled': 7 lines + 1)         kinds with it
    wide sets         N2H+ 2-1, 40 lines                                            kinds without the filled bit
    wide, filled      the filled mix on wide_band + the isotopologue (33 lines + 1)  kinds with it
    the queue form    NH3 (1,1) + (2,2), 512 channels, the 72 rows tiled to the smallest launch the plan queues, plus 17

Kinds 0, 1 and 3 have the unrolled component forms: 1, 2, 3 and 4 components (NCOMP 1, 2, 3 and the general form).  Every
kind with the filled, layered or calibrated bit has the general form alone: 2 components.  Every launch is of 72 rows: one
set-up group of 64 and one of 8; every spectrum of 300 channels ends in a row of 44 of 64 lanes.
"""
import functools
from collections import namedtuple

import numpy as np

K_WEIGHTED, K_BASELINE, K_FILL, K_LAYER, K_CALIB = 1, 2, 4, 8, 16
PLAIN, W8, QUEUE, WEIGHTED, BASELINE = range(5)
N_ROWS = 72                     # one set-up group of 64 rows and one of 8
ORDER = 3                       # the baseline order of every case with the baseline bit
QUEUE_CHAN = 512                # the queue form asks for units of eight rows and more
QUEUE_EXTRA = 17                # rows above the smallest queued launch: not a whole number of 16-unit chunks
MODES = ('table', 'fast')
SEED_BASE = 7020                # of the parameter draws: chosen on the CPU so that check_draws holds for every set
# every set of the five bits the rule admits: plain, weighted, baseline; filled; layered; calibrated
KINDS = (0, 1, 3, 4, 5, 7, 8, 9, 11, 12, 13, 15, 19, 23, 27, 31)
UNROLLED_KINDS = (0, 1, 3)

# name: the model of test_layered.MODELS its parameters are drawn for, the channels of its spectra, the most lines of a
# spectrum (LpShape.nhf_max: more than 26 are the wide forms), whether the set is filled
SETS = {
    'ammonia':     dict(model='ammonia', sizes=(300, 300), nhf_max=21, filled=False),
    'filled':      dict(model='filled', sizes=(300, 300), nhf_max=7, filled=True),
    'n2hp':        dict(model='n2hp', sizes=(300,), nhf_max=40, filled=False),
    'wide_filled': dict(model='filled', sizes=(300, 300), nhf_max=33, filled=True),
    'ammonia512':  dict(model='ammonia', sizes=(QUEUE_CHAN, QUEUE_CHAN), nhf_max=21, filled=False),
}
SET_OF = {(False, False): 'ammonia', (False, True): 'filled', (True, False): 'n2hp', (True, True): 'wide_filled'}

# set: the name in SETS; mode: 'table' / 'fast'; spectra: spectra out; ncomp: components of the runner; chan: a noise per
# channel; order: the baseline order or None; filled, layered: the set's; cal: whether the set has a calibration uncertainty
# (test_calibration.CAL of the set's model); rows: the launch's rows, None: the queue's (queue_rows of the device);
# index, form: lnl_inst_index and LnlForm of the instance the launch must land on; group: the child process that runs it
Case = namedtuple('Case', 'set mode spectra ncomp chan order filled layered cal rows index form group')


def wide_of(set_name):
    return SETS[set_name]['nhf_max'] > 26


def inst_index(mode, spectra, wide, ncomp_inst, kind):
    """lnl_inst_index: bits 0-1 NCOMP, 2 wide, 3 spectra out, 4 fast mode, 5-9 kind."""
    return (kind << 5) | (16 if mode == 'fast' else 0) | (8 if spectra else 0) | (4 if wide else 0) | ncomp_inst


def kind_of(case):
    return ((K_WEIGHTED if case.chan or case.order is not None or case.cal else 0) | (K_BASELINE if case.order is not None or case.cal else 0)
            | (K_FILL if case.filled else 0) | (K_LAYER if case.layered else 0) | (K_CALIB if case.cal else 0))


def _cases():
    out = []
    for mode in MODES:
        for wide in (False, True):
            for kind in KINDS:
                general_only = bool(kind & (K_FILL | K_LAYER | K_CALIB))
                assert general_only == (kind not in UNROLLED_KINDS)
                for ncomp in ((2,) if general_only else (1, 2, 3, 4)):
                    for spectra in (False, True):
                        form = (BASELINE if kind & K_BASELINE else WEIGHTED if kind & K_WEIGHTED
                                else W8 if kind == 0 and mode == 'table' and spectra else PLAIN)     # (w8: the plain set's alone)
                        filled = bool(kind & K_FILL)
                        out.append(Case(set=SET_OF[wide, filled], mode=mode, spectra=spectra, ncomp=ncomp, chan=bool(kind & K_WEIGHTED),
                                        order=ORDER if kind & K_BASELINE else None, filled=filled, layered=bool(kind & K_LAYER),
                                        cal=bool(kind & K_CALIB), rows=N_ROWS,
                                        index=inst_index(mode, spectra, wide, 0 if general_only or ncomp > 3 else ncomp, kind), form=form,
                                        group=f'{mode}-{"wide" if wide else "narrow"}-{"general" if general_only else "unrolled"}'))
    # the queue form: the table mode, narrow, kind 0
    for ncomp in (1, 2, 3, 4):
        for spectra in (False, True):
            out.append(Case(set='ammonia512', mode='table', spectra=spectra, ncomp=ncomp, chan=False, order=None, filled=False,
                            layered=False, cal=False, rows=None, index=inst_index('table', spectra, False, 0 if ncomp > 3 else ncomp, 0), form=QUEUE,
                            group='queue'))
    return tuple(out)


CASES = _cases()
GROUPS = tuple(dict.fromkeys(c.group for c in CASES))
assert all(kind_of(c) == c.index >> 5 for c in CASES)


def small_form(case):
    """The form of a queue case's first launch, too small for the queue: w8 with spectra out, else plain."""
    return W8 if case.spectra else PLAIN


def table_workgroup(ncomp, nhf_max):
    """(waves per workgroup, workgroups per CU) of a table-mode launch with one wave per unit, as DESIGN 4.2 states them: of 4,
    6, ..., 16 waves the count that keeps the most of a CU's 32 wave slots filled beside the 6656 doubles of tables each
    workgroup stages in 160 KiB of LDS, then the most workgroups, then the fewest waves; with the queue's 16 bytes."""
    tables, lds = 256 + 2 * 10 * 256 + 10 * 128, 160 * 1024
    wave_doubles = (ncomp * nhf_max * 5 + 1) // 2 * 2

    def per_cu(w, extra):
        return lds // (8 * (tables + wave_doubles * w) + extra)
    w = max(range(4, 17, 2), key=lambda w: (min(32, per_cu(w, 0) * w), per_cu(w, 0), -w))
    return w, max(1, min(per_cu(w, 16), 32 // w))


def queue_rows(n_cu, ncomp, set_name='ammonia512'):
    """The smallest launch of the set that plan_lnl sends to the queue on a device of n_cu compute units: two units and more
    per wave of the workgroups resident at once."""
    waves, per_cu = table_workgroup(ncomp, SETS[set_name]['nhf_max'])
    n_spec = len(SETS[set_name]['sizes'])
    return -(-2 * n_cu * per_cu * waves // n_spec)


def rows_of(case, n_cu):
    return case.rows if case.rows is not None else queue_rows(n_cu, case.ncomp, case.set) + QUEUE_EXTRA


# ---------------------------------------------------------------------------- sets, draws, data (the sibling tests')
def spectra_of(set_name, na):
    """[(axis, what the restatement and the runner need of the spectrum)]."""
    import test_layered as tl
    if set_name == 'ammonia512':
        from nestfit_amd.synth import freq_axis
        return [(freq_axis(1, QUEUE_CHAN, 20.0), 1), (freq_axis(2, QUEUE_CHAN, 20.0), 2)]
    if set_name == 'wide_filled':
        from test_lte_bands import wide_band
        mol, ks, iso, isos = tl._species()
        (x0, _), second = tl._spectra('filled', na)
        wide = na.LteBlend(list(wide_band(mol, ks)) + isos)
        assert wide.n_lines == SETS[set_name]['nhf_max']
        return [(x0, wide), second]
    return tl._spectra(set_name, na)


def make_runner(na, case, rows):
    import test_calibration as tc
    import test_layered as tl
    kw = dict(baseline_order=case.order, layered=case.layered, calibration=tc.CAL[SETS[case.set]['model']] if case.cal else None)
    if case.set == 'wide_filled':
        mol, ks, iso, isos = tl._species()
        return na.LteMix((mol, iso), fill=True).Runner.from_data(rows, None, ncomp=case.ncomp, **kw)
    return tl._runner(na, SETS[case.set]['model'], rows, None, case.ncomp, **kw)


@functools.lru_cache(maxsize=None)
def data_rows(set_name, ncomp, order, chan):
    """The rows [axis, data, noise, what] of a set: test_calibration._data -- the truth times the gains, its ramp where a baseline
    is fitted, with `chan` a noise per channel that masks a stretch on the line.  The wide filled set has the narrow one's
    data (the axes are the same) beside its own transitions; the queue's set of 512 channels has noise alone, as
    test_layered._data_rows."""
    import nestfit_amd as na
    import test_calibration as tc
    from test_lte_mix import NOISE
    if set_name == 'ammonia512':
        assert order is None and not chan
        rng = np.random.default_rng(512 + ncomp)
        return [[x, rng.normal(0, NOISE, QUEUE_CHAN), NOISE, what] for x, what in spectra_of(set_name, na)]
    if set_name == 'wide_filled':
        return [[x, d, noise, what] for (x, d, noise, _), (_, what) in zip(tc._data('filled', ncomp, order, chan), spectra_of(set_name, na))]
    return tc._data(set_name, ncomp, order, chan)


@functools.lru_cache(maxsize=None)
def reference(set_name, ncomp):
    """(thetas[N_ROWS], layered spectra, summed spectra, S, what the draws hold) of layer_restatement on the set's spectra,
    concatenated per row; the summed spectrum is sum_c g_c a_c of the restatement's own terms."""
    import hf_restatement as hfr
    import layer_restatement as lay
    import nestfit_amd as na
    import test_layered as tl
    from oracle import nfo
    model = SETS[set_name]['model']
    m = tl.MODELS[model]
    axes = spectra_of(set_name, na)
    rng = np.random.default_rng(SEED_BASE + 100 * sorted(SETS).index(set_name) + ncomp)
    thetas = np.stack([tl.draw_layers(rng, model, ncomp, k) for k in range(N_ROWS)])
    tbgs = [hfr.tbg_of(nfo, x) for x, _ in axes]
    layered, summed, S, tau_peak, stacked = [], [], [], [], 0
    for th in thetas:
        row = [], [], []
        for k, ((x, what), tbg) in enumerate(zip(axes, tbgs)):
            terms = []
            if model == 'ammonia':
                p, s = lay.amm_layered(nfo, x, what, th, terms)
            elif model == 'n2hp':
                p, s = lay.nnhp_layered(nfo, x, what, th, terms)
            else:
                mol, ks, iso, isos = tl._species()
                p, s = lay.mix_layered(nfo, x, tbg, what, (mol, iso), th, fill=True, terms=terms)
            row[0].append(p), row[1].append(sum(g * a for _, g, a in terms)), row[2].append(s)
            if k == 0:
                tau_peak += [t[0].max() for t in terms]
                voff, sigm = th[:ncomp], th[m['sigm_row'] * ncomp:(m['sigm_row'] + 1) * ncomp]
                # two layers within one line width of each other, a > 0.5 in both in one channel (test_layered._reference)
                stacked += any(abs(voff[c] - voff[d]) < min(sigm[c], sigm[d]) and np.minimum(terms[c][2], terms[d][2]).max() > 0.5
                               for c in range(ncomp) for d in range(c + 1, ncomp))
        layered.append(np.concatenate(row[0])), summed.append(np.concatenate(row[1])), S.append(np.concatenate(row[2]))
    layered, summed, S = np.stack(layered), np.stack(summed), np.stack(S)
    for a in (thetas, layered, summed, S):
        a.setflags(write=False)
    return thetas, layered, summed, S, dict(tau_peak=np.array(tau_peak), stacked=stacked)


def check_draws(set_name, ncomp, layered):
    """The draws hold what makes the checks bite: optical depths from thin to opaque, lines far above the noise, and for a
    layered case layers on top of one another in a quarter of the rows and more."""
    _, _, _, S, draws = reference(set_name, ncomp)
    assert draws['tau_peak'].min() < 1e-3 and draws['tau_peak'].max() > 32.0, (set_name, ncomp, draws['tau_peak'].min(), draws['tau_peak'].max())
    assert S.max() > 1.0, (set_name, ncomp, S.max())
    if layered:
        assert ncomp > 1 and draws['stacked'] >= N_ROWS // 4, (set_name, ncomp, draws['stacked'])


@functools.lru_cache(maxsize=None)
def wanted(set_name, ncomp, layered, chan, order, cal):
    """(rows, thetas, wanted spectra, S, wanted lnL, M): lnL and M of calib_restatement in longdouble on the restatement's
    spectra -- cal = 0, order = None and a scalar noise reduce marginal_lnl to the plain chi^2."""
    import calib_restatement as cr
    import test_calibration as tc
    thetas, lay_spec, sum_spec, S, _ = reference(set_name, ncomp)
    spec = lay_spec if layered else sum_spec
    rows = data_rows(set_name, ncomp, order, chan)
    cals = tc.CAL[SETS[set_name]['model']] if cal else (0.0,) * len(rows)
    at = np.concatenate([[0], np.cumsum([len(r[0]) for r in rows])])
    lnl, M = np.zeros(N_ROWS), np.zeros(N_ROWS)
    for i, pred in enumerate(spec):
        for k, (_, d, noise, _) in enumerate(rows):
            p = pred[at[k]:at[k + 1]]
            lnl[i] += float(cr.marginal_lnl(d, p, noise, cals[k], order))
            M[i] += float(cr.magnitude(d, p, noise, cals[k], order))
    lnl.setflags(write=False), M.setflags(write=False)
    return rows, thetas, spec, S, lnl, M


def wanted_of(case):
    return wanted(case.set, case.ncomp, case.layered, case.chan, case.order, case.cal)
