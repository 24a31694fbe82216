"""Every launch of a runner's kernels is planned by csrc/nfa_launch_plan.h: the kernel instance, the workgroups, the
waves and the dynamic LDS.  The header is plain C++17, g++ compiles it alone, and this test checks the plans on a machine
without a GPU against statements written down independently: the table of launch forms in DESIGN 4.2, the LDS carve-up
in the comments of lnl_body / lnl_kernel_queue / setup_body / point_kernel / ring_serve_kernel, and the figures DESIGN
records.  (A profiler's trace does not show a launch's dynamic LDS; reads past it return nothing and fault nothing.)"""
import ctypes as C
import itertools
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
LDS_PER_CU = 160 * 1024
TABLES = 256 + 2 * 10 * 256 + 10 * 128      # doubles of the table mode's staged tables: 2^(i/256), FastExp's C, B and A
TAIL = 768                                  # doubles that must lie behind them (nfa_device.h: SM_TABLE_TAIL)
PROG_BYTES, LINE_REC_BYTES = 3624, 32       # sizeof(PriorProg), sizeof(LineRec): the engine asserts them
PLAIN, W8, QUEUE, WEIGHTED, BASELINE = range(5)


class LpShape(C.Structure):
    _fields_ = [('n_spec', C.c_int), ('size', C.c_int * 16), ('nhf_max', C.c_int), ('ncomp', C.c_int), ('ndim', C.c_int),
                ('model', C.c_int), ('n_stage', C.c_int), ('stage_doubles', C.c_int), ('wpb', C.c_int), ('wpb_table', C.c_int),
                ('lnl_cap', C.c_int), ('lnl_split', C.c_int), ('prog_bytes', C.c_int), ('line_rec_bytes', C.c_int)]


class LpLaunch(C.Structure):
    _fields_ = [('B', C.c_int64), ('mode', C.c_int), ('group_n', C.c_int), ('group_each', C.c_int64), ('write_spec', C.c_bool),
                ('has_prior', C.c_bool), ('baseline', C.c_bool), ('weighted', C.c_bool), ('has_queue', C.c_bool)]


class LpKnobs(C.Structure):
    _fields_ = [(k, C.c_int) for k in ('n_cu', 'setup_ti', 'setup_threads', 'setup_sub', 'lnl_queue', 'lnl_queue_wg',
                                       'coalesce', 'ablate')]


class LnlGeom(C.Structure):
    _fields_ = [('nhf_max', C.c_int), ('wave_doubles', C.c_int), ('inv_nspec', C.c_uint), ('inv_nhf', C.c_uint),
                ('split', C.c_int), ('queue', C.c_void_p), ('ablate', C.c_int)]


class LnlPlan(C.Structure):
    _fields_ = [('form', C.c_int), ('wide', C.c_bool), ('G', LnlGeom), ('waves', C.c_int), ('lds', C.c_size_t),
                ('blocks', C.c_int64), ('error', C.c_char_p)]


class SetupPlan(C.Structure):
    _fields_ = [('inst', C.c_int), ('ti', C.c_int), ('nsub', C.c_int), ('threads', C.c_int), ('blocks', C.c_uint),
                ('lds', C.c_size_t), ('staged', C.c_bool), ('error', C.c_char_p)]


class FusedPlan(C.Structure):
    _fields_ = [('refusal', C.c_char_p), ('ring_error', C.c_char_p), ('G', LnlGeom), ('n_blocks', C.c_int), ('ctl_double', C.c_int),
                ('staged', C.c_bool), ('lds_point', C.c_size_t), ('lds_ring', C.c_size_t)]


MIRRORS = [LpShape, LpLaunch, LpKnobs, LnlGeom, LnlPlan, SetupPlan, FusedPlan]
# one row of lnl_many's input / output (int64 columns)
IN = ['mode', 'nhf_max', 'size0', 'size_rest', 'n_spec', 'ncomp', 'B', 'write_spec', 'baseline', 'weighted', 'lnl_queue',
      'has_queue', 'lnl_split', 'wpb', 'lnl_cap', 'n_cu']
OUT = ['error', 'form', 'wide', 'split', 'wave_doubles', 'waves', 'lds', 'blocks', 'inv_nspec', 'inv_nhf']
SHIM = r'''
#include "nfa_launch_plan.h"
#include <cstring>
extern "C" {
void lnl(const LpShape *s, const LpKnobs *k, const LpLaunch *L, LnlPlan *out) { *out = plan_lnl(*s, *k, *L); }
void setup(const LpShape *s, const LpKnobs *k, const LpLaunch *L, SetupPlan *out) { *out = plan_setup(*s, *k, *L); }
void fused(const LpShape *s, const LpKnobs *k, int mode, int bl, int wt, FusedPlan *out) { *out = plan_fused(*s, *k, mode, bl != 0, wt != 0); }
int lanes(const LpShape *s, const LpKnobs *k, long long B) { return lp_lanes(*s, *k, B); }
int may_hold(const LpShape *s, const LpKnobs *k, long long B, int profiling) { return lp_may_hold(*s, *k, B, profiling != 0); }
int group_full(const LpShape *s, const LpKnobs *k, int n, long long B) { return lp_group_full(*s, *k, n, B); }
int t_waves(const LpShape *s) { return table_waves(*s); }
int t_wg_per_cu(const LpShape *s, int waves) { return table_wg_per_cu(*s, waves); }
// n likelihood plans of ammonia sets without priors: rows of IN -> rows of OUT (the error as its address)
void lnl_many(long long n, const long long *in, long long *out) {
    for (long long i = 0; i < n; ++i, in += 16, out += 10) {
        LpShape s = {};
        s.nhf_max = (int)in[1]; s.n_spec = (int)in[4]; s.ncomp = (int)in[5]; s.ndim = 6 * s.ncomp; s.model = NFA_MODEL_AMMONIA;
        for (int q = 0; q < s.n_spec; ++q) s.size[q] = (int)(q ? in[3] : in[2]);
        s.lnl_split = (int)in[12]; s.wpb = (int)in[13]; s.lnl_cap = (int)in[14]; s.prog_bytes = 3624; s.line_rec_bytes = 32;
        LpKnobs k = {};
        k.lnl_queue = (int)in[10]; k.n_cu = (int)in[15]; k.coalesce = NFA_GROUP_MAX;
        LpLaunch L = {};
        L.B = in[6]; L.mode = (int)in[0]; L.group_n = 1; L.group_each = in[6];
        L.write_spec = in[7]; L.baseline = in[8]; L.weighted = in[9]; L.has_queue = in[11];
        const LnlPlan P = plan_lnl(s, k, L);
        out[0] = (long long)(size_t)P.error; out[1] = P.form; out[2] = P.wide; out[3] = P.G.split; out[4] = P.G.wave_doubles;
        out[5] = P.waves; out[6] = (long long)P.lds; out[7] = P.blocks; out[8] = P.G.inv_nspec; out[9] = P.G.inv_nhf;
    }
}
// the instance rule (lnl_instance_exists) and, for a plan of a launch with the three set flags, {error, form, wide, kind, ncomp}
int inst_exists(int form, int mode, int ws, int wide, int ncomp_inst, unsigned kind) {
    return lnl_instance_exists((LnlForm)form, mode, ws != 0, wide != 0, ncomp_inst, kind);
}
void plan_inst(const LpShape *s, const LpKnobs *k, const LpLaunch *L, int filled, int layered, int calibrated, int *out) {
    LpLaunch l = *L;
    l.filled = filled != 0; l.layered = layered != 0; l.calibrated = calibrated != 0;
    const LnlPlan P = plan_lnl(*s, *k, l);
    out[0] = P.error != nullptr; out[1] = P.form; out[2] = P.wide; out[3] = (int)lnl_plan_kind(P); out[4] = lnl_plan_ncomp(P, s->ncomp);
}
// the side family (lnl_kernel_side): a side's flag word and plan form, an instance's index and its inverse, the side of a set
unsigned side_flags(int side) { return lnl_side_flags((LnlSide)side); }
int side_form(int side) { return lnl_side_form((LnlSide)side); }
int side_index(int mode, int ws, int wide, int filled, int layered) { return lnl_side_index(mode, ws != 0, wide != 0, filled != 0, layered != 0); }
void side_at(int i, int *out) {
    const LnlSideInst a = lnl_side_at(i);
    out[0] = a.mode; out[1] = a.write_spec; out[2] = a.wide; out[3] = a.filled; out[4] = a.layered;
}
int side_of(int corr, int resp, int tmpl, int cont, int rob) { return lnl_side_of(corr != 0, resp != 0, tmpl != 0, cont != 0, rob != 0); }
int sizes(int i) {
    const int s[] = {sizeof(LpShape), sizeof(LpLaunch), sizeof(LpKnobs), sizeof(LnlGeom), sizeof(LnlPlan), sizeof(SetupPlan), sizeof(FusedPlan),
                     SM_TABLE_DOUBLES, SM_TABLE_TAIL, (int)LDS_PER_CU, LNL_PARTS, NFA_BL_NB, SETUP_TI, QREC, POINT_WAVES, NFA_POINT_MAXDIM, NFA_GROUP_MAX};
    return s[i];
}
}
'''


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('launch_plan')
    src = tmp / 'plan.cpp'
    src.write_text(SHIM)
    so = tmp / 'libplan.so'
    res = subprocess.run(['g++', '-std=c++17', '-Wall', '-Werror', '-O1', '-shared', '-fPIC', f'-I{ROOT / "nestfit_amd" / "csrc"}',
                          str(src), '-o', str(so)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    lib = C.CDLL(str(so))
    for i, m in enumerate(MIRRORS):
        assert lib.sizes(i) == C.sizeof(m), m.__name__
    assert [lib.sizes(i) for i in range(7, 17)] == [TABLES, TAIL, LDS_PER_CU, 4, 4, 64, 12, 8, 24, 8]
    lib.lnl_many.argtypes = [C.c_longlong, C.c_void_p, C.c_void_p]
    lib.lanes.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong]
    lib.may_hold.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int]
    lib.group_full.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_longlong]
    return lib


def shape(n_spec=2, size=1024, nhf_max=21, ncomp=2, model=0, n_stage=10, stage_doubles=5000, ndim=None, **kw):
    """A runner; by default the benchmark's: NH3 (1,1) + (2,2) (21 lines at most) of 1024 channels, two components, the
    ten 500-point tables that get_irdc_priors stages."""
    sizes = list(size) if isinstance(size, (list, tuple)) else [size] * n_spec
    s = LpShape(n_spec=n_spec, nhf_max=nhf_max, ncomp=ncomp, ndim=6 * ncomp if ndim is None else ndim, model=model,
                n_stage=n_stage, stage_doubles=stage_doubles, prog_bytes=PROG_BYTES, line_rec_bytes=LINE_REC_BYTES, **{'wpb': 1, **kw})
    s.size[:n_spec] = sizes
    return s


def knobs(**kw):
    return LpKnobs(**{**dict(n_cu=256, lnl_queue=1, coalesce=8), **kw})


def launch(B, mode, n=1, each=None, **kw):
    return LpLaunch(B=B, mode=mode, group_n=n, group_each=B // n if each is None else each,
                    **{**dict(has_prior=True, has_queue=True), **kw})


# ---- the likelihood launch ----------------------------------------------------------------------------------------
def wave_doubles(ncomp, nhf_max):
    """lnl_body: per unit a line table of ncomp * nhf_max 32-byte records, then a window of two ints per line; an even
    number of doubles."""
    return (ncomp * nhf_max * (4 + 1) + 1) // 2 * 2


def table_workgroup(ncomp, nhf_max):
    """Waves per workgroup of a table-mode launch with one wave per unit: of 4, 6, ..., 16 the count that keeps the most
    waves (of a CU's 32) resident beside the 52 KB of tables each workgroup stages, then the most workgroups, then the
    smallest; and how many such workgroups a CU holds, with the queue's 16 bytes."""
    def per_cu(w, extra):
        return LDS_PER_CU // (8 * (TABLES + wave_doubles(ncomp, nhf_max) * w) + extra)
    w = max(range(4, 17, 2), key=lambda w: (min(32, per_cu(w, 0) * w), per_cu(w, 0), -w))
    return w, max(1, min(per_cu(w, 16), 32 // w))


def expected_lnl(c, tw):
    """Columns of IN (arrays) -> columns of OUT, from DESIGN 4.2 and the kernels' comments; tw[ncomp, nhf_max] =
    table_workgroup."""
    table = c['mode'] == 0
    units = c['B'] * c['n_spec']
    several = c['n_spec'] > 1
    min_size = np.where(several, np.minimum(c['size0'], c['size_rest']), c['size0'])
    max_size = np.where(several, np.maximum(c['size0'], c['size_rest']), c['size0'])
    slots = 32 * c['n_cu']
    # waves per unit: as asked, or two / four while the launch leaves half / three quarters of the wave slots empty;
    # never more than the shortest spectrum has rows of 64 channels
    asked = np.where(c['lnl_split'] > 0, c['lnl_split'], np.where(4 * units <= slots, 4, np.where(2 * units <= slots, 2, 1)))
    rows = (min_size + 63) // 64
    split = np.select([(asked >= 4) & (rows >= 4), (asked >= 2) & (rows >= 2)], [4, 2], 1)
    wd = (c['ncomp'] * c['nhf_max'] * 5 + 1) // 2 * 2
    w_fast = np.clip(c['wpb'], 1, 16)
    w_fast = np.maximum(w_fast, split) // split * split
    w_tab, wg_tab = tw[c['ncomp'], c['nhf_max'], 0], tw[c['ncomp'], c['nhf_max'], 1]
    waves = np.where(table, np.where(split > 1, 8, w_tab), w_fast)
    upw = waves // split
    wide = (c['nhf_max'] > 26) | (max_size > 2 ** 22)
    # DESIGN 4.2, the first row that applies
    resident = c['n_cu'] * wg_tab                                   # workgroups resident at once (queue: split 1, so w_tab waves)
    form = np.select([c['baseline'] != 0,
                      c['weighted'] != 0,
                      table & ~wide & (split == 1) & (c['lnl_queue'] != 0) & (min_size >= 512) & (units >= 2 * resident * w_tab)
                      & (c['has_queue'] != 0),
                      table & (c['write_spec'] != 0)],
                     [BASELINE, WEIGHTED, QUEUE, W8], PLAIN)
    # LDS: [table mode: the tables][per unit of the workgroup: its line table][split > 1, per unit: 4 parts x 64 lanes,
    # with a baseline 1 + 4 of them][queue: 16 bytes]; table mode: at least tables + tail
    per_unit = wd + np.where(split > 1, 4 * 64 * np.where(form == BASELINE, 5, 1), 0)
    lds = 8 * (np.where(table, TABLES, 0) + per_unit * upw) + np.where(form == QUEUE, 16, 0)
    lds = np.where(table, np.maximum(lds, 8 * (TABLES + TAIL)), lds)
    too_big = lds > LDS_PER_CU
    # the residency pad (fast mode, option lnl_cap): at most `cap` workgroups per CU
    cap = np.maximum(c['lnl_cap'], 1)
    lds = np.where(~table & (c['lnl_cap'] > 0) & (waves * c['lnl_cap'] < 32), np.maximum(lds, LDS_PER_CU // cap // 16 * 16), lds)
    blocks = np.where(form == QUEUE, resident, (units + upw - 1) // upw)
    inv = lambda n: np.where(n == 1, 0, 2 ** 32 // n + 1)
    return dict(too_big=too_big, form=form, wide=wide, split=split, wave_doubles=wd, waves=waves, lds=lds, blocks=blocks,
                inv_nspec=inv(c['n_spec']), inv_nhf=inv(c['nhf_max']))


def test_likelihood_plans_follow_the_form_table_and_the_kernels_layout(lib):
    n_cu = 256
    tw = np.zeros((11, 51, 2), dtype=np.int64)
    for ncomp in range(1, 11):
        for nhf in range(1, 51):
            tw[ncomp, nhf] = table_workgroup(ncomp, nhf)
            s = shape(ncomp=ncomp, nhf_max=nhf)
            assert (lib.t_waves(C.byref(s)), lib.t_wg_per_cu(C.byref(s), int(tw[ncomp, nhf, 0]))) == tuple(tw[ncomp, nhf]), (ncomp, nhf)
    assert tuple(tw[2, 21]) == (16, 2)                                  # the benchmark's set: two workgroups of sixteen waves
    s = shape(wpb_table=8)
    assert lib.t_waves(C.byref(s)) == 8                                 # option wpb_table
    n, forms, errors, splits = 0, set(), set(), set()
    fixed_B = np.array([1, 2, 63, 300, 513, 4096, 32768, 0, 0])
    blw = np.array([(0, 0), (0, 1), (1, 1)])                            # neither, a noise per channel, a baseline (weighted too)
    for mode, nhf, size in itertools.product((0, 2), (1, 18, 26, 27, 40, 50), (128, 256, 511, 512, 1024, 2 ** 22 + 64)):
        blocks = []
        # spectra of one size at every B; sets of several also with a first spectrum of `size` before others of 1024 channels
        for size_rest, b_ix in ((size, range(9)), (1024, (0, 5, 8))):
            n_spec, ncomp, ws, w_ix, queue, counters, split, wpb, cap, b = [m.ravel() for m in np.meshgrid(
                (1, 2, 3, 16), (1, 2, 3, 4, 10), (0, 1), (0, 1, 2), (0, 1), (0, 1), (0, 1, 2, 4), (1, 4, 16), (0, 2), b_ix, indexing='ij')]
            # the two edges of "fills the resident workgroups twice": the last B that does not, the first that does
            edge = -(-2 * n_cu * tw[ncomp, nhf, 1] * tw[ncomp, nhf, 0] // n_spec)
            B = np.where(b < 7, fixed_B[b], edge - (b == 7))
            one = np.ones_like(B)
            blocks.append(np.stack([mode * one, nhf * one, size * one, size_rest * one, n_spec, ncomp, B, ws, blw[w_ix, 0], blw[w_ix, 1],
                                    queue, counters, split, wpb, cap, n_cu * one], axis=1)[(n_spec > 1) | (size_rest == size)])
        rows = np.concatenate(blocks)
        a = np.ascontiguousarray(rows, dtype=np.int64)
        out = np.zeros((len(a), len(OUT)), dtype=np.int64)
        lib.lnl_many(len(a), a.ctypes.data, out.ctypes.data)
        c = {k: a[:, i] for i, k in enumerate(IN)}
        got = {k: out[:, i] for i, k in enumerate(OUT)}
        want = expected_lnl(c, tw)
        texts = {p: C.string_at(int(p)) for p in np.unique(got['error']) if p}
        assert set(texts.values()) <= {b'ncomp too large for the LDS line table'}, texts
        failed = got['error'] != 0
        assert np.array_equal(failed, want['too_big']), (mode, nhf, size)
        ok = ~failed
        for f in ('form', 'wide', 'split', 'wave_doubles', 'waves', 'lds', 'blocks', 'inv_nspec', 'inv_nhf'):
            bad = np.flatnonzero(ok & (got[f] != want[f]))
            assert bad.size == 0, (f, dict(zip(IN, a[bad[0]])), got[f][bad[0]], want[f][bad[0]])
        # what every launch must satisfy whatever the form: the grid covers the units, a workgroup has 1..16 whole waves
        # per unit, and its LDS fits a CU
        upw = got['waves'] // np.maximum(got['split'], 1)
        assert np.all((got['form'] == QUEUE)[ok] | (got['blocks'] * upw >= c['B'] * c['n_spec'])[ok])
        assert np.all((got['waves'] >= 1)[ok] & (got['waves'] <= 16)[ok] & (got['waves'] % got['split'] == 0)[ok])
        assert np.all(got['lds'][ok] <= LDS_PER_CU)
        n += len(a)
        forms |= set(np.unique(got['form'][ok])); splits |= set(np.unique(got['split'][ok])); errors |= set(texts.values())
    assert forms == {PLAIN, W8, QUEUE, WEIGHTED, BASELINE} and splits == {1, 2, 4} and len(errors) == 1
    print(f'{n} likelihood plans checked')


# ---- the instances of the likelihood kernel ------------------------------------------------------------------------
K_WEIGHTED, K_BASELINE, K_FILL, K_LAYER, K_CALIB = 1, 2, 4, 8, 16


def test_the_instance_rule_gives_the_documented_families(lib):
    """lnl_instance_exists over every (form, mode, spectra out, wide, NCOMP 0..3, kind 0..31) against the counts DESIGN
    states: 4.2 (plain, weighted and baseline: 32 each over mode, spectra out, wide, NCOMP; w8: the table mode with spectra
    out; queue: the table mode, narrow), 4.10 (filled: plain, weighted, baseline over mode, spectra out, wide), 4.11
    (layered: those over filled as well), 4.12 (calibrated: the baseline form over filled and layered)."""
    count = dict.fromkeys(('plain', 'w8', 'queue', 'weighted', 'baseline', 'filled', 'layered', 'calibrated'), 0)
    for form, mode, ws, wide, ncomp, kind in itertools.product(range(5), (0, 2), (0, 1), (0, 1), range(4), range(32)):
        if not lib.inst_exists(form, mode, ws, wide, ncomp, kind):
            continue
        if kind == 0:
            family = {PLAIN: 'plain', W8: 'w8', QUEUE: 'queue'}[form]          # (no other form without a kind)
        else:
            family = ('calibrated' if kind & K_CALIB else 'layered' if kind & K_LAYER else 'filled' if kind & K_FILL
                      else 'baseline' if kind & K_BASELINE else 'weighted')
        count[family] += 1
    assert count == dict(plain=24, w8=8, queue=8, weighted=32, baseline=32, filled=24, layered=48, calibrated=32)
    assert sum(count.values()) == 208
    # the plain form of kind 0: everything but the table mode with spectra out, which is w8's or the queue's
    for mode, ws, wide, ncomp in itertools.product((0, 2), (0, 1), (0, 1), range(4)):
        assert bool(lib.inst_exists(PLAIN, mode, ws, wide, ncomp, 0)) == (not (mode == 0 and ws))
    # outside the enumeration there is nothing: the polynomial mode, NCOMP 4, a kind of six bits
    assert not any(lib.inst_exists(PLAIN, *a) for a in ((1, 0, 0, 0, 0), (0, 0, 0, 4, 0), (0, 0, 0, -1, 0), (0, 0, 0, 0, 32)))


def test_every_plan_has_its_instance(lib):
    """The sweep of tests/test_calibration_cpu.py crossed with filled, layered and calibrated: every plan names an instance
    that exists, and its kind and NCOMP are what the rule says in words: weighted for the weighted and the baseline form,
    baseline for the baseline form, the three flags as the launch has them; NCOMP 1..3 unrolled, else and for every filled,
    layered or calibrated set the general form."""
    out = (C.c_int * 5)()
    n, kinds = 0, set()
    for mode, B, (nhf_max, size, model), ncomp, write_spec in itertools.product(
            (0, 2), (1, 11, 64, 4096, 32768), ((9, 300, 4), (21, 1024, 0), (33, 1024, 1)), (1, 2, 3, 4, 8), (False, True)):
        s, k = shape(n_spec=2, size=size, nhf_max=nhf_max, ncomp=ncomp, model=model), knobs()
        for baseline, weighted, has_queue, filled, layered, calibrated in itertools.product((False, True), repeat=6):
            L = LpLaunch(B=B, mode=mode, group_n=1, group_each=B, write_spec=write_spec, has_prior=True, baseline=baseline,
                         weighted=weighted, has_queue=has_queue)
            lib.plan_inst(C.byref(s), C.byref(k), C.byref(L), filled, layered, calibrated, out)
            error, form, wide, kind, ncomp_inst = out
            assert not error, (mode, B, nhf_max, ncomp)               # (none of these shapes is refused: no plan is left out)
            want_kind = ((K_WEIGHTED if form in (WEIGHTED, BASELINE) else 0) | (K_BASELINE if form == BASELINE else 0)
                         | (K_FILL if filled else 0) | (K_LAYER if layered else 0) | (K_CALIB if calibrated else 0))
            want_ncomp = 0 if filled or layered or calibrated or ncomp > 3 else ncomp
            assert (kind, ncomp_inst) == (want_kind, want_ncomp)
            assert lib.inst_exists(form, mode, write_spec, wide, ncomp_inst, kind), (form, mode, write_spec, wide, ncomp_inst, kind)
            n += 1
            kinds.add(kind)
    assert n == 2 * 5 * 3 * 5 * 2 * 64
    # every kind the rule admits is planned by some launch: 1 + weighted, baseline + 3 filled + 6 layered + 4 calibrated
    assert len(kinds) == 16 and kinds == {kd for kd in range(32) if lib.inst_exists(
        BASELINE if kd & K_BASELINE else WEIGHTED if kd & K_WEIGHTED else PLAIN, 2, 0, 0, 0, kd)}


def admitted(lib):
    """{(lnl_inst_index, form)} of everything lnl_instance_exists admits."""
    return {((kind << 5) | (16 if mode else 0) | (8 if ws else 0) | (4 if wide else 0) | ncomp, form)
            for form, mode, ws, wide, ncomp, kind in itertools.product(range(5), (0, 2), (0, 1), (0, 1), range(4), range(32))
            if lib.inst_exists(form, mode, ws, wide, ncomp, kind)}


def planned(lib, s, k, L, filled, layered, calibrated, out=None):
    """(lnl_inst_index, form) of the plan of a launch; it has no error and names an instance that exists."""
    out = (C.c_int * 5)() if out is None else out
    lib.plan_inst(C.byref(s), C.byref(k), C.byref(L), filled, layered, calibrated, out)
    error, form, wide, kind, ncomp_inst = out
    assert not error
    return (kind << 5) | (16 if L.mode else 0) | (8 if L.write_spec else 0) | (4 if wide else 0) | ncomp_inst, form


def test_every_instance_is_the_plan_of_some_launch(lib):
    """The converse of test_every_plan_has_its_instance: everything the rule admits -- everything the engine compiles -- is
    what plan_lnl names for some runner, launch and options.  One and two spectra of 128 and 1024 channels, 21 and 40 lines, 1
    to 4 components, lnl_split 0 and 1, from one row to 40000, both modes, spectra out or not, the lane's counters there or
    not, every set of the five flags."""
    want = admitted(lib)
    assert len(want) == 208
    got, out, k = set(), (C.c_int * 5)(), knobs()
    for n_spec, size, nhf_max, ncomp, split in itertools.product((1, 2), (128, 1024), (21, 40), (1, 2, 3, 4), (0, 1)):
        s = shape(n_spec=n_spec, size=size, nhf_max=nhf_max, ncomp=ncomp, lnl_split=split)
        for mode, B, write_spec, has_queue, baseline, weighted in itertools.product((0, 2), (1, 4096, 40000), (False, True), (False, True),
                                                                                   (False, True), (False, True)):
            L = LpLaunch(B=B, mode=mode, group_n=1, group_each=B, write_spec=write_spec, has_prior=False, baseline=baseline,
                         weighted=weighted, has_queue=has_queue)
            for filled, layered, calibrated in itertools.product((0, 1), repeat=3):
                got.add(planned(lib, s, k, L, filled, layered, calibrated, out))
    assert got == want, (sorted(want - got), sorted(got - want))


def test_the_census_names_every_instance_and_every_case_plans_its_own(lib):
    """tests/instance_census.py: the (instance, form) pairs its cases name are the pairs the rule admits, one case each, and
    at 256 compute units plan_lnl gives every case exactly its pair, at lnl_split 0 and 1 -- what tests/test_instance_census.py
    then finds in the launch counters of the device."""
    import instance_census as ic
    assert (ic.PLAIN, ic.W8, ic.QUEUE, ic.WEIGHTED, ic.BASELINE) == (PLAIN, W8, QUEUE, WEIGHTED, BASELINE)
    named = [(c.index, c.form) for c in ic.CASES]
    assert len(named) == len(set(named)) == 208 and set(named) == admitted(lib)
    assert len(ic.GROUPS) == 9 and all(c.group in ic.GROUPS for c in ic.CASES)
    k = knobs(n_cu=256)

    def plan(c, B, split):
        st = ic.SETS[c.set]
        s = shape(n_spec=len(st['sizes']), size=list(st['sizes']), nhf_max=st['nhf_max'], ncomp=c.ncomp, lnl_split=split)
        L = LpLaunch(B=B, mode={'table': 0, 'fast': 2}[c.mode], group_n=1, group_each=B, write_spec=c.spectra, has_prior=False,
                     baseline=c.order is not None, weighted=c.chan, has_queue=True)
        assert st['filled'] == c.filled and ic.wide_of(c.set) == bool(c.index & 4)
        return planned(lib, s, k, L, c.filled, c.layered, c.cal)
    for c in ic.CASES:
        for split in (0, 1):
            assert plan(c, ic.rows_of(c, 256), split) == (c.index, c.form), c
        if c.form == QUEUE:
            # the queue's launches are the smallest the plan queues, and 17 rows; one row fewer than the smallest is not
            # queued, nor is the cases' first launch: both land on the plain or w8 instance of the same NCOMP
            smallest = ic.queue_rows(256, c.ncomp, c.set)
            assert ic.rows_of(c, 256) == smallest + 17 and (2 * (smallest + 17)) % 16 != 0
            assert plan(c, smallest, 0) == (c.index, QUEUE)
            for B in (smallest - 1, ic.N_ROWS):
                assert plan(c, B, 0) == (c.index, ic.small_form(c)), (c, B)


def one_lnl(lib, s, k, L):
    out = LnlPlan()
    lib.lnl(C.byref(s), C.byref(k), C.byref(L), C.byref(out))
    return out


def test_launches_too_large_are_refused(lib):
    # units * 8 must stay below 2^28 (the kernels divide by multiplying); 2^25 units are the first too many
    assert one_lnl(lib, shape(), knobs(), launch(2 ** 24 - 1, 2)).error is None
    assert one_lnl(lib, shape(), knobs(), launch(2 ** 24, 2)).error == b'batch too large for one launch'
    assert one_lnl(lib, shape(ncomp=10, nhf_max=50, wpb=16), knobs(), launch(4096, 2)).error == b'ncomp too large for the LDS line table'


def test_the_shapes_design_records(lib):
    """the benchmark coalesces 8 batches of 4096 rows x 2 spectra of 1024 channels (NH3 (1,1) + (2,2), two
    components) into one table-mode launch: the queue form, 2 n_cu workgroups of sixteen waves.  A lone batch is the
    plain form; with spectra out and the queue off, w8."""
    s, k = shape(), knobs()
    p = one_lnl(lib, s, k, launch(8 * 4096, 0, n=8))
    assert (p.error, p.form, p.blocks, p.waves, p.G.split) == (None, QUEUE, 2 * 256, 16, 1)
    assert p.lds == 8 * (TABLES + 16 * wave_doubles(2, 21)) + 16
    p = one_lnl(lib, s, k, launch(4096, 0))
    assert (p.error, p.form, p.blocks, p.waves) == (None, PLAIN, 4096 * 2 // 16, 16)
    p = one_lnl(lib, s, knobs(lnl_queue=0), launch(8 * 4096, 0, n=8, write_spec=True))
    assert (p.error, p.form, p.blocks, p.waves) == (None, W8, 8 * 4096 * 2 // 16, 16)
    # option lnl_queue_wg: one workgroup per CU; the knob `ablate` travels in the geometry
    p = one_lnl(lib, s, knobs(lnl_queue_wg=1, ablate=5), launch(8 * 4096, 0, n=8))
    assert (p.form, p.blocks, p.G.ablate, p.G.queue) == (QUEUE, 256, 5, None)


# ---- the set-up launch --------------------------------------------------------------------------------------------
TABLE_2, TABLE, FAST, POLY = range(4)        # setup_kernel<0, false, 2>, <0, false>, <1, true>, <1, false>


def setup_lds(ncomp, ndim, tables, nsub, staged_doubles):
    """setup_body: [exponential tables][per group of items: theta, ndim x 64; partition records, 64 x ncomp x 12]
    [the prior program, and one double][its staged tables]"""
    return 8 * ((TABLES if tables else 256) + nsub * (64 * ndim + 64 * ncomp * 12) + PROG_BYTES // 8 + 1 + staged_doubles)


def one_setup(lib, s, k, L):
    out = SetupPlan()
    lib.setup(C.byref(s), C.byref(k), C.byref(L), C.byref(out))
    return out


def test_setup_plans(lib):
    k = knobs()
    assert setup_lds(7, 42, True, 1, 5000) == 161392 and setup_lds(8, 48, True, 1, 5000) == 170608
    p = one_setup(lib, shape(ncomp=7), k, launch(300, 0))
    assert (p.error, p.inst, p.nsub, p.threads, p.blocks, p.lds, p.staged, p.ti) == (None, TABLE, 1, 512, 5, 161392, True, 64)
    p = one_setup(lib, shape(ncomp=8), k, launch(300, 0))                 # the program that reads its tables from global memory
    assert (p.error, p.inst, p.nsub, p.threads, p.blocks, p.lds, p.staged) == (None, TABLE, 1, 512, 5, 170608 - 8 * 5000, False)
    p = one_setup(lib, shape(ncomp=8), k, launch(300, 0, has_prior=False))   # predict: no program at all
    assert (p.lds, p.staged) == (170608 - 8 * 5000, False)
    # two groups per workgroup: whole workgroups, more items than ti * n_cu, no override, a staged layout that fits
    two = (None, TABLE_2, 2, 1024, 256, setup_lds(2, 12, True, 2, 5000), True)
    got = lambda p: (p.error, p.inst, p.nsub, p.threads, p.blocks, p.lds, p.staged)
    assert two[5] == 133744
    assert got(one_setup(lib, shape(), k, launch(32768, 0, n=8))) == two
    assert got(one_setup(lib, shape(), k, launch(32768, 0))) == two
    p = one_setup(lib, shape(), k, launch(32700, 0))                       # one batch may have any size
    assert (p.inst, p.blocks) == (TABLE_2, 256)
    one = lambda B, threads=512, ti=64: (None, TABLE, 1, threads, -(-B // ti), setup_lds(2, 12, True, 1, 5000), True)
    assert got(one_setup(lib, shape(), k, launch(64 * 256, 0, n=4))) == one(64 * 256)              # not more than ti * n_cu
    assert got(one_setup(lib, shape(), k, launch(64 * 256 + 1, 0))) == two[:4] + (129,) + two[5:]
    assert got(one_setup(lib, shape(), k, launch(2 * 8320, 0, n=2))) == two[:4] + (130,) + two[5:]
    assert got(one_setup(lib, shape(), k, launch(8 * 4160, 0, n=8))) == one(8 * 4160)              # batches of 65 workgroups
    assert got(one_setup(lib, shape(), knobs(setup_threads=384), launch(32768, 0))) == one(32768, threads=384)
    assert got(one_setup(lib, shape(), knobs(setup_sub=1), launch(32768, 0))) == one(32768)
    assert got(one_setup(lib, shape(), knobs(setup_ti=32), launch(32768, 0))) == one(32768, ti=32)
    assert one_setup(lib, shape(), knobs(setup_ti=32), launch(32768, 0)).ti == 32
    assert setup_lds(5, 30, True, 2, 5000) > LDS_PER_CU >= setup_lds(5, 30, True, 1, 5000)         # two groups would not fit staged
    p = one_setup(lib, shape(ncomp=5), k, launch(32768, 0))
    assert got(p) == (None, TABLE, 1, 512, 512, setup_lds(5, 30, True, 1, 5000), True)
    p = one_setup(lib, shape(ncomp=5, n_stage=0, stage_doubles=0), k, launch(32768, 0))            # priors with nothing staged: two fit
    assert got(p) == (None, TABLE_2, 2, 1024, 256, setup_lds(5, 30, True, 2, 0), False)
    # the fast mode, and a model without partition sums in the table mode: the polynomial's table, four waves
    p = one_setup(lib, shape(), k, launch(32768, 2))
    assert got(p) == (None, FAST, 1, 256, 512, setup_lds(2, 12, False, 1, 5000), True)
    for model in (1, 2, 3, 4):
        p = one_setup(lib, shape(model=model, ndim=8), k, launch(32768, 0))
        assert got(p) == (None, POLY, 1, 256, 512, setup_lds(2, 8, False, 1, 5000), True)
        assert one_setup(lib, shape(model=model, ndim=8), k, launch(32768, 2)).inst == FAST
    p = one_setup(lib, shape(ncomp=10, ndim=200), k, launch(300, 0))
    assert p.error == b'too many parameters for the set-up kernel'


# ---- the fused kernels ----------------------------------------------------------------------------------------------
def one_fused(lib, s, mode, bl=0, wt=0, k=None):
    out = FusedPlan()
    lib.fused(C.byref(s), C.byref(k or knobs()), mode, bl, wt, C.byref(out))
    return out


def fused_expected(s, mode, split, staged=True):
    """point_kernel: [exponential tables][the set-up stage | table mode: behind the tables, fast mode: from the start: the
    line tables and split parts of the 8 / split units of a pass].  ring_serve_kernel: [exponential tables][the set-up
    stage, its prior tables staged once][line tables and parts][16 bytes of control words, 16-byte aligned]; table mode:
    the tail behind the tables at least."""
    setup = setup_lds(s.ncomp, s.ndim, mode == 0, 1, s.stage_doubles if staged else 0)
    units = 8 * (wave_doubles(s.ncomp, s.nhf_max) + (256 if split > 1 else 0)) * (8 // split)
    tables = 8 * TABLES if mode == 0 else 0
    ring = setup + units
    if mode == 0:
        ring = max(ring, 8 * (TABLES + TAIL))
    ring = (ring + 15) // 16 * 16
    return max(setup, tables + units), ring + 16, ring // 8


def test_fused_plans(lib):
    batch = b"this runner's points go through the batch kernels: use nfa_ring_serve"
    for s, bl, wt, why in ((shape(ncomp=5), 0, 0, batch), (shape(nhf_max=40), 0, 0, batch), (shape(size=2 ** 22 + 64), 0, 0, batch),
                           (shape(), 1, 1, b'the resident kernel has no form for a baseline: use nfa_ring_serve'),
                           (shape(), 0, 1, b'the resident kernel has no form for a noise per channel: use nfa_ring_serve'),
                           (shape(lnl_split=16), 0, 0, b"spectra too short for the point kernel's split")):
        for mode in (0, 2):
            p = one_fused(lib, s, mode, bl, wt)
            assert p.refusal == why and p.ring_error == why
    # (5001 staged doubles: an odd count in front of the resident kernel's control words, which lie on 16 bytes)
    for mode, n_spec, split, ncomp, staged in itertools.product((0, 2), (1, 2, 3, 16), (1, 2, 4), (1, 2, 4), (5000, 5001)):
        s = shape(n_spec=n_spec, ncomp=ncomp, lnl_split=split, stage_doubles=staged)
        p = one_fused(lib, s, mode)
        want = fused_expected(s, mode, split)
        where = (mode, n_spec, split, ncomp, staged)
        assert p.refusal is None and p.G.split == split and p.staged, where
        assert p.n_blocks == -(-n_spec // (8 // split)), where
        assert (p.lds_point, p.lds_ring, p.ctl_double) == want, where
        assert p.ring_error is None and p.lds_ring <= LDS_PER_CU and p.lds_ring == 8 * p.ctl_double + 16 and p.ctl_double % 2 == 0, where
    # a launch of one item splits by itself: 2 units on 8192 wave slots
    assert one_fused(lib, shape(), 0).G.split == 4 and one_fused(lib, shape(size=128), 0).G.split == 2
    assert one_fused(lib, shape(), 0).lds_ring == 8 * (TABLES + 2304 + 454 + 5000) + 8 * 2 * (210 + 256) + 16 == 122784
    # the fast mode's small layouts still hold the control words behind everything else
    s = shape(n_spec=1, ncomp=1, nhf_max=1, n_stage=0, stage_doubles=0)
    assert one_fused(lib, s, 2).lds_ring == fused_expected(s, 2, 4)[1]
    # sixteen spectra of 26 lines, four components, one wave per unit: the resident kernel's line tables do not fit
    s = shape(n_spec=16, ncomp=4, nhf_max=26, lnl_split=1)
    p = one_fused(lib, s, 0)
    assert p.refusal is None and p.ring_error == b'too many parameters for the resident kernel'
    assert (p.lds_point, p.lds_ring) == fused_expected(s, 0, 1)[:2] and p.lds_point <= LDS_PER_CU < p.lds_ring
    # whether the prior tables are staged is asked of the set-up stage behind the polynomial's table in either mode: with
    # 9000 doubles of them and four components the table mode's point launch does not fit, and takes the batch path
    s = shape(ncomp=4, stage_doubles=9000)
    p = one_fused(lib, s, 0)
    assert p.staged and p.lds_point == setup_lds(4, 24, True, 1, 9000) == 165744 and p.lds_point > LDS_PER_CU
    s = shape(ncomp=4, stage_doubles=16000)
    p = one_fused(lib, s, 2)
    assert not p.staged and p.lds_point == setup_lds(4, 24, False, 1, 0)


# ---- lanes and coalescing -------------------------------------------------------------------------------------------
def test_lanes_and_coalescing_at_their_edges(lib):
    s, k = shape(), knobs()                                               # 2 spectra, 256 CUs: 8192 wave slots
    lanes = lambda B, s=s: lib.lanes(C.byref(s), C.byref(k), B)
    # six lanes for batches of three quarters to one and a half units per wave slot, else four
    assert [lanes(B) for B in (1, 3071, 3072, 4096, 6144, 6145, 32768)] == [4, 4, 6, 6, 6, 4, 4]
    assert [lanes(B, shape(n_spec=3)) for B in (2047, 2048, 4096, 4097)] == [4, 6, 6, 4]
    hold = lambda B, k=k, prof=0: bool(lib.may_hold(C.byref(s), C.byref(k), B, prof))
    # held: whole set-up workgroups, at most four units per wave slot, not while profiling, not with option coalesce 1
    assert [hold(B) for B in (64, 4096, 4097, 16384, 16448)] == [True, True, False, True, False]
    assert not hold(4096, prof=1) and not hold(4096, k=knobs(coalesce=1)) and hold(4096, k=knobs(coalesce=2))
    assert hold(4128, k=knobs(setup_ti=32)) and not hold(4128)
    full = lambda n, B, k=k: bool(lib.group_full(C.byref(s), C.byref(k), n, B))
    # full: `coalesce` batches, or one more would make more than eight units per wave slot
    assert [full(n, 4096) for n in (1, 7, 8)] == [False, False, True]
    assert [full(n, 4096, knobs(coalesce=2)) for n in (1, 2)] == [False, True]
    assert [full(n, 8192) for n in (2, 3, 4)] == [False, False, True]
    assert [full(n, 16384) for n in (1, 2)] == [False, True]


# ---- the side family ------------------------------------------------------------------------------------------------
F_CORR, F_RESP, F_TMPL, F_CONT, F_ROBUST = 32, 64, 128, 256, 512
SIDE_NONE, SIDE_CORR, SIDE_RESP, SIDE_TMPL, SIDE_CONT, SIDE_ROBUST = range(6)
# a side's kernels: the flags of lnl_body they switch on, and the form whose plan they are launched with
SIDES = {SIDE_CORR: (K_WEIGHTED | F_CORR, WEIGHTED), SIDE_RESP: (K_WEIGHTED | F_CORR | F_RESP, WEIGHTED),
         SIDE_TMPL: (K_WEIGHTED | K_BASELINE | F_TMPL, BASELINE), SIDE_CONT: (K_WEIGHTED | K_BASELINE | F_CONT, BASELINE),
         SIDE_ROBUST: (K_WEIGHTED | F_ROBUST, WEIGHTED)}


def test_the_side_family_is_the_five_words_their_forms_one_layout_and_one_precedence(lib):
    """lnl_kernel_side's host side against a table written here: the flag word of each side (none: the plain set's 0), the
    plan form it runs under (the weighted form for a correlation, a response and a robust likelihood, the baseline form for
    templates and a continuum), the index of an instance -- bit 0 wide, 1 spectra out, 2 fast mode, 3 filled, 4 layered, so
    exactly the values 0..31, each once, and lnl_side_at its inverse -- and the side of a set: a robust likelihood before a
    continuum before templates before a response before a correlation."""
    lib.side_flags.restype = C.c_uint
    assert lib.side_flags(SIDE_NONE) == 0 and lib.side_form(SIDE_NONE) == PLAIN
    for side, (flags, form) in SIDES.items():
        assert (lib.side_flags(side), lib.side_form(side)) == (flags, form), side
    assert len({flags for flags, _ in SIDES.values()}) == 5
    seen, out = {}, (C.c_int * 5)()
    for layered, filled, mode, ws, wide in itertools.product((0, 1), (0, 1), (0, 2), (0, 1), (0, 1)):
        i = lib.side_index(mode, ws, wide, filled, layered)
        assert i == 16 * layered + 8 * filled + (4 if mode == 2 else 0) + 2 * ws + wide
        lib.side_at(i, out)
        assert list(out) == [mode, ws, wide, filled, layered]
        seen[i] = (mode, ws, wide, filled, layered)
    assert sorted(seen) == list(range(32))
    for corr, resp, tmpl, cont, rob in itertools.product((0, 1), repeat=5):
        want = (SIDE_ROBUST if rob else SIDE_CONT if cont else SIDE_TMPL if tmpl else SIDE_RESP if resp else SIDE_CORR if corr
                else SIDE_NONE)
        assert lib.side_of(corr, resp, tmpl, cont, rob) == want, (corr, resp, tmpl, cont, rob)
