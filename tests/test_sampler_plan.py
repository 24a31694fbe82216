"""The form of a device-sampler run is decided by `ns_plan` (csrc/nfa_sampler_plan.h) and, for the numpy twin
(nestfit_amd/nested.py), by `nested._plan`.  Every GPU sampler test rests on the two taking the same decisions, and on
the twin's stages (`_refit`, `_propose`, `_update_reject`, `_walk_step`, `_chunk_kr`) working with the kernels' constants;
this one checks the decisions themselves and every shared constant, the header's NS_X against the twin's _NS_X, on a
machine without a GPU: the header is plain C++17, g++ compiles it alone."""
import ctypes as C
import itertools
import subprocess
from pathlib import Path

import numpy as np
import pytest

from nestfit_amd import nested

ROOT = Path(__file__).resolve().parent.parent
UNSET = -2 ** 31                                    # NS_UNSET

INT_KNOBS = ['ellipsoids', 'frames', 'walkers', 'walk_factor', 'k_target', 'refit_every', 'ratio_max', 'kmax']
DBL_KNOBS = ['margin', 'shear', 'pairs']
INT_FIELDS = ['max_ell', 'stage_live', 'multi', 'shear', 'sh_M', 'boxes', 'n_frames', 'pairs', 'walk_factor', 'k_target',
              'refit_every', 'w_fixed', 'w_stride', 'ratio_max', 'kmax', 'refit_threads']
DBL_FIELDS = ['shear_enlarge', 'margin_c', 'pairs_enlarge']
SHARED = [f for f in INT_FIELDS + DBL_FIELDS if f != 'refit_threads']      # (the twin launches nothing)
# every constant of the header the twin mirrors, by the type it has there
INT_CONSTS = ['NS_ME', 'NS_ME_MAXD', 'NS_STAGE_BYTES', 'NS_FRAMES', 'NS_RATIO_MAX', 'NS_KMAX', 'NS_SHEAR_MMAX', 'NS_KP_START',
              'NS_K_TARGET', 'NS_REFIT_EVERY', 'NS_WALK_LOWD', 'NS_WALK_FACTOR_LOWD', 'NS_WALK_FACTOR']
DBL_CONSTS = ['NS_MARGIN_C', 'NS_SHEAR_ENLARGE', 'NS_PAIRS_ENLARGE', 'NS_WALK_TARGET', 'NS_ME_GAIN', 'NS_MARGIN_A',
              'NS_MARGIN_FLOOR', 'NS_SHEAR_RIDGE', 'NS_SHEAR_PIVOT']
U64_CONSTS = ['NS_TAG_LIVE', 'NS_B_RADIUS', 'NS_B_START', 'NS_B_ELL', 'NS_B_KEEP', 'NS_FRAME_SEED']


class NsKnobs(C.Structure):
    _fields_ = [(k, C.c_int) for k in INT_KNOBS] + [(k, C.c_double) for k in DBL_KNOBS]


class NsPlan(C.Structure):
    _fields_ = ([(f, C.c_int) for f in INT_FIELDS] + [(f, C.c_double) for f in DBL_FIELDS]
                + [('lds_update', C.c_size_t), ('lds_refit', C.c_size_t), ('error', C.c_char_p)])


@pytest.fixture(scope='module')
def plan_lib(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('ns_plan')
    src = tmp / 'plan.cpp'
    src.write_text('#include "nfa_sampler_plan.h"\n'
                   'extern "C" void plan(int D, int DT, int N, const int *fm, const NsKnobs *k, NsPlan *out) { *out = ns_plan(D, DT, N, fm, *k); }\n'
                   'extern "C" void merge(const NsKnobs *a, const NsKnobs *b, NsKnobs *out) { *out = ns_merge(*a, *b); }\n'
                   'extern "C" int sizes(int i) { const int s[] = {sizeof(NsKnobs), sizeof(NsPlan), NS_SHEAR_MMAX, NS_STAGE_BYTES}; return s[i]; }\n'
                   'extern "C" int const_int(int i) { const int v[] = {%s}; return v[i]; }\n'
                   'extern "C" double const_dbl(int i) { const double v[] = {%s}; return v[i]; }\n'
                   'extern "C" unsigned long long const_u64(int i) { const unsigned long long v[] = {%s}; return v[i]; }\n'
                   % (', '.join(INT_CONSTS), ', '.join(DBL_CONSTS), ', '.join(U64_CONSTS)))
    so = tmp / 'libplan.so'
    res = subprocess.run(['g++', '-std=c++17', '-Wall', '-Werror', '-shared', '-fPIC', f'-I{ROOT / "nestfit_amd" / "csrc"}',
                          str(src), '-o', str(so)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    lib = C.CDLL(str(so))
    assert lib.sizes(0) == C.sizeof(NsKnobs) and lib.sizes(1) == C.sizeof(NsPlan)
    lib.const_dbl.restype, lib.const_u64.restype = C.c_double, C.c_ulonglong
    return lib


def shapes():
    """(ndim, slots of the sampled dimensions): a theta row holds six parameters of 1..4 components, parameter-major
    (slot = parameter * ncomp + component)."""
    out = []
    for nc in (1, 2, 3, 4):
        out.append((6 * nc, list(range(6 * nc))))                            # all free: D = 6, 12, 18, 24
        out.append((6 * nc, list(range(5 * nc))))                            # five of six parameters: 5, 10, 15, 20
        out.append((6 * nc, list(range(4 * nc))))                            # four of six: 4, 8, 12, 16
        out.append((6 * nc, list(range(1, 6 * nc, 2))))                      # the odd slots: 3, 6, 9, 12
    out += [(6, [2]), (6, [0, 3]), (12, list(range(7)))]                     # D = 1, 2, 7
    out.append((12, list(range(8)) + [10, 11]))                              # D = 10, another map that keeps slot % 2 = dimension % 2
    out.append((12, list(range(8)) + [9, 10]))                               # ... one that breaks it
    out.append((12, [0, 1, 2, 3, 4, 5, 6, 7, 8, 11]))                        # ... (only the last dimension's slot moved: still kept)
    out.append((18, list(range(14)) + [15]))                                 # D = 15, broken
    out.append((18, list(range(10))))                                        # D = 10 in a row of three components
    out.append((10, list(range(10))))                                        # D = 10, no sixth parameter
    return out


def nlives(ndim, D):
    edge = nested._NS_STAGE_BYTES // (8 * D)                               # the most live points that are staged
    return sorted({n for n in (ndim + 2, 100, 383, 384, 400, 768, 1000, 8192, edge, edge + 1) if ndim + 2 <= n <= 8192})


CHAIN = list(itertools.product([None, 1, 2, 4],             # ellipsoids: unset, off, two values
                               [None, -1, 0, 8, 32],        # frames: unset, no boxes, axis boxes only, two values
                               [None, 0.0, 2.5, 4.0],       # shear: unset, off, two values
                               [None, 0.0, 1.75, 2.5]))     # pairs
# the knobs the chain does not read (walkers, walk_factor, k_target, refit_every, ratio_max, kmax, margin)
FREE = [(None, None, None, None, None, None, None), (0, None, 0, None, None, None, 1.5),
        (64, 1, 4, 1, 8, 64, 3.5), (256, 32, 64, 16, 64, 262144, None)]


def cases():
    for ndim, fm in shapes():
        for n in nlives(ndim, len(fm)):
            for (ell, fr, sh, pr), (wk, wf, kt, re_, rm, km, mg) in itertools.product(CHAIN, FREE):
                yield ndim, fm, n, dict(ellipsoids=ell, frames=fr, walkers=wk, walk_factor=wf, k_target=kt, refit_every=re_,
                                        ratio_max=rm, kmax=km, margin=mg, shear=sh, pairs=pr)


def lds_update_expected(N):
    """ns_update_kernel: [live lnL: N doubles, an even count][a segment's survivors: lnL][their proposal, compact row, rank:
    ints][valid / surviving counts: 32 ints][threshold, done flag]; a segment = 4 x 256 proposals."""
    seg = 4 * 256
    return 8 * ((N + 1) // 2 * 2) + 8 * seg + 3 * 4 * seg + 4 * 32 + 8 * 2


def lds_refit_expected(N, D, p):
    """ns_refit_kernel: [8 doubles: reductions][A: D*D][c: D, an even count][live points: N*D, where staged][NS_ME + 2 fit
    slots of D + 2 D*D + 4 doubles, a label per live point (ints, a multiple of four) | the shear's scratch: Gram matrix
    M*M, coefficients D*M, mu and sigma 2 D, the constant one, one of padding]."""
    b = 8 * (8 + D * D + (D + 1) // 2 * 2)
    if p.stage_live:
        b += 8 * N * D
    if p.multi:
        b += 8 * (4 + 2) * (D + 2 * D * D + 4) + 4 * ((N + 3) // 4 * 4)
    if p.shear:
        b += 8 * (p.sh_M * p.sh_M + D * p.sh_M + 2 * D + 1 + 1)
    return b


def test_device_plan_equals_the_twins(plan_lib):
    n = 0
    seen = {f: set() for f in SHARED}
    largest = (0, None)
    kn, out = NsKnobs(), NsPlan()
    for ndim, fm, N, knobs in cases():
        D = len(fm)
        for k in INT_KNOBS:
            setattr(kn, k, UNSET if knobs[k] is None else knobs[k])
        for k in DBL_KNOBS:
            setattr(kn, k, float(UNSET) if knobs[k] is None else knobs[k])
        plan_lib.plan(D, ndim, N, (C.c_int * D)(*fm), C.byref(kn), C.byref(out))
        tw = nested._plan(D, ndim, N, np.array(fm), **knobs)
        where = (ndim, fm, N, knobs)
        assert out.error is None and tw.error is None, where
        for f in SHARED:
            a, b = getattr(out, f), getattr(tw, f)
            assert type(a) is type(b) and a == b, (f, a, b, where)
            seen[f].add(a)
        assert out.refit_threads == (64 if out.multi else 512), where
        assert out.lds_update == lds_update_expected(N), where
        assert out.lds_refit == lds_refit_expected(N, D, out), where
        if out.stage_live:
            assert N * D * 8 <= plan_lib.sizes(3), where
            assert out.lds_refit <= 160 * 1024, (out.lds_refit, where)
            largest = max(largest, (out.lds_refit, where), key=lambda t: t[0])
        assert out.lds_update <= 160 * 1024, where
        assert out.sh_M <= plan_lib.sizes(2), where
        if out.pairs:                               # the pair ellipses are fitted in the shear's scratch, four doubles a pair
            assert out.shear and out.boxes and 4 * (D * (D - 1) // 2) <= out.sh_M * out.sh_M, where
        n += 1
    assert n >= 115200
    # every form of the bound occurred, and every on / off field took both values
    for f in ('stage_live', 'multi', 'shear', 'boxes', 'pairs'):
        assert seen[f] == {0, 1}, f
    assert seen['sh_M'] >= {0, 36, 56} and max(seen['sh_M']) == 56
    print(f'{n} plans compared; largest lds_refit of a staged shape {largest[0]} bytes at {largest[1]}')


def test_a_default_changed_on_one_side_is_caught(plan_lib, monkeypatch):
    """The comparison is not vacuous: with another _NS_MARGIN_C in the twin alone the plans of a default run differ."""
    kn, out = NsKnobs(), NsPlan()
    for k in INT_KNOBS:
        setattr(kn, k, UNSET)
    for k in DBL_KNOBS:
        setattr(kn, k, float(UNSET))
    plan_lib.plan(5, 6, 400, (C.c_int * 5)(*range(5)), C.byref(kn), C.byref(out))
    assert out.margin_c == nested._plan(5, 6, 400, np.arange(5)).margin_c
    monkeypatch.setattr(nested, '_NS_MARGIN_C', 1.75)
    assert out.margin_c != nested._plan(5, 6, 400, np.arange(5)).margin_c


def test_shared_constants_equal_the_twins(plan_lib):
    """Every NS_X of the header that the twin holds as _NS_X has the same value there, exactly and in the same kind of
    number -- the stream slots and the frame seed as 64-bit integers -- and the twin holds no _NS_ name the header lacks."""
    for names, get, kind in ((INT_CONSTS, plan_lib.const_int, int), (DBL_CONSTS, plan_lib.const_dbl, float),
                             (U64_CONSTS, plan_lib.const_u64, np.uint64)):
        for i, name in enumerate(names):
            twin = getattr(nested, '_' + name)
            assert type(twin) is kind and twin == kind(get(i)), (name, twin, get(i))
    assert {n for n in vars(nested) if n.startswith('_NS_')} == {'_' + n for n in INT_CONSTS + DBL_CONSTS + U64_CONSTS}
    assert int(nested._NS_TAG_LIVE) == 1 << 62 and plan_lib.const_u64(U64_CONSTS.index('NS_TAG_LIVE')) == 1 << 62     # (no 32-bit wrap)


def test_setter_before_option_before_constant(plan_lib):
    """ns_merge: knob by knob, the first argument's value where it is set, else the second's."""
    a, b, m = NsKnobs(), NsKnobs(), NsKnobs()
    for i, k in enumerate(INT_KNOBS + DBL_KNOBS):
        setattr(a, k, (UNSET if i % 2 else 3))
        setattr(b, k, (UNSET if i % 3 == 0 else 7))
    plan_lib.merge(C.byref(a), C.byref(b), C.byref(m))
    for i, k in enumerate(INT_KNOBS + DBL_KNOBS):
        assert getattr(m, k) == (3 if i % 2 == 0 else UNSET if i % 3 == 0 else 7), k
