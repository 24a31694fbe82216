"""The setters of a spectra set's likelihood options (the nfa_specset_set_* calls) hold one contract (include/nestfit_amd.h):
a call leaves the set as one made that way, to the bit, whatever it was before; a refused or failed call leaves it as it was;
and nfa_specset_set_data keeps the options.  One piece of the engine holds it, specset_realise over csrc/nfa_set_state.h.

test_the_walk: one live two-pixel set per noise kind walks a fixed list of setter calls -- every option on, replaced, off
(None, and the all-zero / identity value); every pair the rules table accepts, on in both orders and off in both orders; the
triples that run together -- and after every step equals a fresh set constructed with exactly the options now on: the bytes
of predict_batch's spectra and lnL, null_lnZ, a single point of pixel 1, two single points on the captured-graph route
(`_state`) and every getter.  Between the steps one request the table refuses changes nothing, and new data in pixel 1 give a fresh set made with those data.  Nothing here is a tolerance.

test_a_failed_allocation_leaves_the_set_as_it_was: the test library's option "fail_alloc" fails the k-th allocation of a
change for every k the change has (the count set_layout gives, before and after)."""
import ctypes as C
import gc

import numpy as np
import pytest

import cont_cases as cc
from nestfit_amd import _options
from test_layered import _ranges
from test_lte_mix import NOISE
from test_set_rules_cpu import BASELINE, CALIB, CONT, CORR, MASK, NMARG, RESP, ROBUST, TMPL, chain
from test_set_state_cpu import layout, lib as state_header          # noqa: F401 (a fixture: the compiled csrc/nfa_set_state.h)
from test_sibling_models import MODES, _simple_priors

pytestmark = pytest.mark.gpu

NCOMP, N_THETA = 2, 96
NAMES = ('baseline_order', 'calibration', 'noise_uncertainty', 'correlation', 'response', 'templates', 'continuum', 'robust')
BIT = dict(zip(NAMES, (BASELINE, CALIB, NMARG, CORR, RESP, TMPL, CONT, ROBUST)))
TAKES = {name: k for k, name in enumerate(NAMES)}                    # SET_TAKES_* of csrc/nfa_set_rules.h
KINDS = ('scalar', 'channel', 'masked')


def _axes(engine):
    return [x for x, _ in cc.spectra('ammonia', engine)]


def _values(n):
    """Two values of every option, [n_spec = 2] (the continuum's second: per pixel), and its all-zero / identity value."""
    j = np.arange(n)
    t1, t2 = np.sin(j / 7.0), np.cos(j / 23.0)
    return {
        'baseline_order': (1, 2, -1),
        'calibration': ([0.1, 0.0], [0.05, 0.2], [0.0, 0.0]),
        'noise_uncertainty': ([0.2, 0.0], [0.1, 0.1], [0.0, 0.0]),
        'correlation': ([[0.5, 0.25], [0.0, 0.0]], [[0.3, 0.1], [0.2, 0.05]], [[0.0, 0.0], [0.0, 0.0]]),
        'response': ([[0.0, 0.25, 0.5, 0.25, 0.0]] * 2, [[0.05, 0.2, 0.5, 0.2, 0.05], [0.0, 0.0, 1.0, 0.0, 0.0]], [[0.0, 0.0, 1.0, 0.0, 0.0]] * 2),
        'templates': ([t1[None], None], [np.stack([t1, t2]), t2[None]], [None, None]),
        'continuum': ([30.0, 0.0], np.array([[2.0, 5.5], [7.0, 1.0]]), [0.0, 0.0]),
        'robust': ([4.0, 0.0], [8.0, 3.0], [0.0, 0.0]),
    }


def _data(engine, kind):
    """(data[2, chan_tot], other data of pixel 1, noise): two pixels of the ammonia rows -- 300 channels a spectrum, four rows of
    64 and one of 44."""
    rows = [cc.data_rows('ammonia', engine, seed=s, chan=kind != 'scalar') for s in (5, 7, 6)]
    data = np.stack([np.concatenate([r[1] for r in rs]) for rs in rows])
    if kind == 'scalar':
        return data[:2].copy(), data[2].copy(), np.array([[NOISE, NOISE], [1.5 * NOISE, 0.8 * NOISE]])
    noise = np.stack([np.concatenate([r[2] for r in rs]) for rs in rows[:2]])
    noise[~np.isfinite(noise)] = 3.0 * NOISE                          # no channel is masked ...
    noise[1] *= 1.25
    if kind == 'masked':
        noise[1, 70] = np.inf                                         # ... but this one
    return data[:2].copy(), data[2].copy(), noise


def _cube(engine, ut, data, noise, options):
    from nestfit_amd.cube import CubeRunner
    return CubeRunner(_axes(engine), (1, 2), data, noise, ut, ncomp=NCOMP, **options)


def _engine_set(ss, name, value):
    """The engine's setter of option `name` with `value`, past the Python side's own table: the return code."""
    from nestfit_amd import _ffi
    about = {'model': ss.model, 'n_pix': ss.n_pix} if name == 'continuum' else {}
    value = _options.normalise(name, value, ss.n_spec, ss.sizes, **about)
    args = {'templates': ss._packed_templates, 'baseline_order': lambda v: (-1 if v is None else v,)}.get(name)
    call = getattr(_ffi.load(), 'nfa_specset_set_' + name.replace('_order', ''))
    return call(ss.handle, *(args(value) if args else (None if value is None else _ffi.dptr(value),)))


def _getters(ss):
    """Every getter's return and values: the seven options' and `layered` (the baseline order has no getter in the C ABI: the
    bits and null_lnZ hold it)."""
    from nestfit_amd import _ffi
    lib = _ffi.load()
    out = []
    for name, shape in (('calibration', 2), ('noise_uncertainty', 2), ('correlation', (2, 2)), ('response', (2, 5)), ('continuum', (ss.n_pix, 2)),
                        ('robust', 2)):
        a = np.zeros(shape)
        out.append((getattr(lib, 'nfa_specset_' + name)(ss.handle, _ffi.dptr(a)), a.tobytes()))
    t, n = np.zeros((4, ss.chan_tot)), np.zeros(2, dtype=np.int32)
    out.append((lib.nfa_specset_templates(ss.handle, _ffi.dptr(t), n.ctypes.data_as(_ffi._ip)), t.tobytes(), n.tobytes()))
    out.append(lib.nfa_specset_layered(ss.handle))
    return tuple(out)


def _state(run, thetas, pix, u):
    """(bytes of the spectra and lnL of predict_batch, null_lnZ, a single point of pixel 1, two single points without a pixel
    array, the getters).  The last two points are MultiNest's call (B = 1, pix NULL: pixel 0): where the point kernel has no
    form for the set (plan_fused of csrc/nfa_launch_plan.h refuses it: a calibration, a continuum, ...) and the mode is the fast one, a runner's second
    such call captures the batch launches as a graph, which holds SpecDev by value, and every later one replays it -- so after
    the first state of a live runner the graph is in play at every setter (which drops it) and every nfa_specset_set_data
    (which does not).  The plain sets and the table mode take the point kernel or the batch path there."""
    from nestfit_amd import _ffi
    spec, lnl = run.predict_batch(pix, thetas)
    point = run.loglikelihood_batch(np.array([1], dtype=np.int32), u.copy()[None])
    single = []
    for _ in range(2):
        U, one = u.copy(), np.empty(1)
        _ffi.check(_ffi.load().nfa_runner_loglike_batch(run._run.handle, None, _ffi.dptr(U), _ffi.dptr(one), 1))
        single.append(U.tobytes() + one.tobytes())
    return spec.tobytes() + lnl.tobytes(), run._ss.null_lnZ().tobytes(), point.tobytes(), tuple(single), _getters(run._ss)


def _thetas():
    rng = np.random.default_rng(9133)
    thetas = np.stack([cc.draw(rng, 'ammonia', NCOMP, k) for k in range(N_THETA)])
    return thetas, (np.arange(N_THETA) % 2).astype(np.int32), np.full(6 * NCOMP, 0.41)


def _walk(masked):
    """The steps (option, which value: 0, 1, None or 'zero'), a fixed list."""
    names = [n for n in NAMES if _options.refusal(n, {'masked'} if masked else set()) is None]
    steps = []
    for n in names:                                                   # on, replaced, off with None; on, off with zeros
        steps += [(n, 0), (n, 1), (n, None), (n, 0), (n, 'zero')]
    pairs = [(a, b) for i, a in enumerate(names) for b in names[i + 1:]
             if _options.refusal(a, {b}) is None and _options.refusal(b, {a}) is None]
    for a, b in pairs:                                                # on in both orders, off in both orders
        steps += [(a, 0), (b, 0), (a, None), (b, None), (b, 1), (a, 1), (b, None), (a, None)]
    for triple in (('baseline_order', 'templates', 'noise_uncertainty'), ('correlation', 'response', 'noise_uncertainty'),
                   ('continuum', 'baseline_order', 'noise_uncertainty')):
        if all(n in names for n in triple):
            steps += [(n, 0) for n in triple] + [(n, None) for n in triple]
    return steps, len(pairs)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('mode', MODES)
def test_the_walk(engine, mode, kind):
    from nestfit_amd import _ffi
    lib = _ffi.load()
    try:
        engine.set_exp_mode(mode)
        ut = _simple_priors(engine, _ranges('ammonia'))
        data, other, noise = _data(engine, kind)
        values = _values(data.shape[1] // 2)
        thetas, pix, u = _thetas()
        changed = data.copy()
        changed[1] = other
        fresh = {}

        def want(on, d):
            """The state of a fresh set made with the options `on` ({name: which value}) and the data `d`, once per such set."""
            key = (tuple(sorted(on.items())), d is changed)
            if key not in fresh:
                fresh[key] = _state(_cube(engine, ut, d, noise, {n: values[n][v] for n, v in on.items()}), thetas, pix, u)
            return fresh[key]

        live = _cube(engine, ut, data, noise, {})
        on = {}
        steps, n_pairs = _walk(kind == 'masked')
        # 28 pairs of eight options less the table's 19; a masked set has no correlation and no response: less those two with a
        # noise uncertainty and with each other
        assert n_pairs == (9 if kind != 'masked' else 6)
        n_refused = 0
        for at, (name, which) in enumerate(steps):
            getattr(live._ss, 'set_' + name.replace('_order', ''))(None if which is None else values[name][2 if which == 'zero' else which])
            if which in (0, 1):
                on[name] = which
            else:
                on.pop(name, None)
            assert _state(live, thetas, pix, u) == want(on, data), (at, name, which, dict(on))
            # the first request the table refuses this set: its sentence, and nothing changes
            has = {*on, 'masked'} if kind == 'masked' else set(on)
            no = next((n for n in NAMES if _options.refusal(n, has) is not None), None)
            if no is not None:
                word = sum(BIT[n] for n in on) | (CORR if 'response' in on else 0) | (MASK if kind == 'masked' else 0)
                assert _engine_set(live._ss, no, values[no][0]) == 1          # NFA_ERR_ARG
                assert lib.nfa_last_error().decode() == chain(word, TAKES[no]), (at, no, dict(on))
                assert _state(live, thetas, pix, u) == want(on, data), (at, 'refused', no, dict(on))
                n_refused += 1
            # new data in pixel 1: a set made with them; and the old again
            if on:
                _ffi.check(lib.nfa_specset_set_data(live._ss.handle, 1, _ffi.dptr(other)))
                assert _state(live, thetas, pix, u) == want(on, changed), (at, 'set_data', dict(on))
                _ffi.check(lib.nfa_specset_set_data(live._ss.handle, 1, _ffi.dptr(np.ascontiguousarray(data[1]))))
                assert _state(live, thetas, pix, u) == want(on, data), (at, 'data back', dict(on))
        assert not on and n_refused > len(steps) // 2
        # the states are not all one: an option changes the bits
        assert len({v[0] for v in fresh.values()}) == len(fresh)
    finally:
        engine.set_exp_mode('fast')


# ------------------------------------------------------------------------------------------------ a failed allocation
@pytest.fixture
def test_library(engine):
    """The Python side over the test library (include/nestfit_amd_test.h) while the test lasts: what it makes, it destroys."""
    from nestfit_amd import _ffi
    gc.collect()
    saved, _ffi._lib = _ffi._lib, _ffi.test_engine()
    try:
        yield _ffi._lib
    finally:
        _ffi._lib.nfa_set_option(b'fail_alloc', 0)
        gc.collect()
        _ffi._lib = saved


def test_a_failed_allocation_leaves_the_set_as_it_was(engine, test_library, state_header):
    lib = test_library
    ut = _simple_priors(engine, _ranges('ammonia'))
    data, _, noise = _data(engine, 'scalar')
    values = _values(data.shape[1] // 2)
    thetas, pix, u = _thetas()
    fired = 0
    for name, base in (('baseline_order', {}), ('correlation', {}), ('templates', {}), ('continuum', {}), ('robust', {}),
                       ('response', {'correlation': values['correlation'][0]})):
        live = _cube(engine, ut, data, noise, base)
        before = _state(live, thetas, pix, u)
        want = _state(_cube(engine, ut, data, noise, {**base, name: values[name][0]}), thetas, pix, u)
        assert want != before
        # the buffers the change adds, as csrc/nfa_set_state.h lays the two sets out
        has = sum(BIT[n] for n in base)
        adds = layout(state_header, has | BIT[name], False)[0] & ~layout(state_header, has, False)[0]
        n_adds = bin(adds).count('1')
        assert n_adds == {'baseline_order': 3, 'correlation': 6, 'templates': 4, 'continuum': 4, 'robust': 3, 'response': 1}[name]
        for k in range(1, n_adds + 1):
            assert lib.nfa_set_option(b'fail_alloc', k) == 0
            assert _engine_set(live._ss, name, values[name][0]) == 2, (name, k)          # NFA_ERR_DEVICE
            assert lib.nfa_last_error().decode().startswith('out of device memory for '), (name, k)
            fired += 1
            assert _state(live, thetas, pix, u) == before, (name, k)
            assert _engine_set(live._ss, name, values[name][0]) == 0                       # unarmed: it succeeds
            assert _state(live, thetas, pix, u) == want, (name, k)
            assert _engine_set(live._ss, name, None) == 0
            assert _state(live, thetas, pix, u) == before, (name, k)
        lib.nfa_set_option(b'fail_alloc', n_adds + 1)                                                # one more than the change has: it never fires
        assert _engine_set(live._ss, name, values[name][0]) == 0
        lib.nfa_set_option(b'fail_alloc', 0)
        assert _state(live, thetas, pix, u) == want
        del live
        gc.collect()
    assert fired == 3 + 6 + 4 + 4 + 3 + 1
    del ut
