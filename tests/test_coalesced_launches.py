"""The benchmark's launches: device-pointer batches at the shapes of bench.WORKLOADS ('C2', 'C4') that the engine holds
and sends as one launch (BatchGroup, n > 1) -- the two-group set-up kernel and the unit queue (lnl_kernel_queue), where
every workgroup and every unit finds its own batch through group_of.  Every batch has its own unit-cube rows, pixel
array and lnL array (and spectra), all of one kind inside ONE allocation between guard bands that must come back bit
for bit unchanged; every batch must give the host-pointer call's bits (that call runs each batch alone) and the CPU
oracle's values to the parity tolerances (test_gpu_parity.py).

The paths named in the comments are those of a 256-CU MI355X (nfa_launch_plan.h: plan_lnl, plan_setup);
test_the_queue_kernel_runs_for_every_batch_of_the_group proves the queue ones with the test library's trace."""
import contextlib
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import bench
from device_buffers import DeviceArrays, GuardedArrays
from nestfit_amd import synth
from nestfit_amd.synth import freq_axis

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
MODES = ['table', 'fast']
LNL_RTOL = {'table': 1e-9, 'fast': 1e-6}             # test_gpu_parity.LNL_RTOL
TB_RTOL, TB_ATOL_K = 1e-6, {'table': 0.0, 'fast': 4e-15}     # test_gpu_parity.test_amm_predict_grid
N_PIX = 6
# guard bands: NaN where the kernels only write; where they read, a value they can read (a stray read then takes the
# ordinary path and shows in the results, a stray write in the band)
U_SENTINEL = 0.4375
PIX_SENTINEL = N_PIX - 1
DEFAULTS = {'coalesce': 8, 'lnl_queue': 1, 'setup_ti': 0, 'setup_sub': 0}


@contextlib.contextmanager
def engine_state(engine, mode, **options):
    """Exp mode `mode` and engine options set for the block; the mode before it and the options' defaults restored."""
    from nestfit_amd import _ffi
    before = _ffi.load().nfa_get_exp_mode()
    try:
        engine.set_exp_mode(mode)
        for key, value in options.items():
            _ffi.set_option(key, value)
        yield
    finally:
        for key, value in DEFAULTS.items():
            _ffi.set_option(key, value)
        engine.set_exp_mode(before)


class Workload:
    """bench.WORKLOADS[name] on a cube of N_PIX pixels whose data and noise are known here: the engine's CubeRunner and
    one oracle runner per pixel."""

    def __init__(self, engine, nfo, name):
        from nestfit_amd.cube import CubeRunner
        trans, n_chan, vhalf, ncomp, truth_key, rows = bench.WORKLOADS[name]
        self.name, self.trans, self.n_chan, self.ncomp, self.rows = name, trans, n_chan, ncomp, rows
        self.ndim, self.n_spec, self.chan_tot = 6 * ncomp, len(trans), len(trans) * n_chan
        axes = [freq_axis(t, n_chan, vhalf) for t in trans]
        rng = np.random.default_rng(2024 + ncomp)
        self.noise = rng.uniform(0.15, 0.3, (N_PIX, self.n_spec))
        self.data = np.empty((N_PIX, self.chan_tot))
        truth = getattr(synth, truth_key)
        for p in range(N_PIX):
            th = truth.copy()
            th[:ncomp] += 0.4 * p                                       # every pixel its own velocities
            for s, (t, x) in enumerate(zip(trans, axes)):
                sc = nfo.AmmoniaSpectrum(x, np.zeros(n_chan), 1.0, t)
                nfo.amm_predict(sc, th)
                self.data[p, s * n_chan:(s + 1) * n_chan] = sc.get_spec() + rng.normal(0, self.noise[p, s], n_chan)
        ut = engine.get_irdc_priors(size=500, vsys=0.0)
        self.cube = CubeRunner(axes, trans, self.data, self.noise, ut, ncomp=ncomp)
        prior = nfo.PriorSet(ut.lower())
        self.oracle = [nfo.AmmoniaRunner([nfo.AmmoniaSpectrum(x, self.data[p, s * n_chan:(s + 1) * n_chan], self.noise[p, s], t)
                                          for s, (t, x) in enumerate(zip(trans, axes))], prior, ncomp=ncomp)
                       for p in range(N_PIX)]
        self._oracle_cache = {}

    def draw(self, n, seed, pattern, rows=None):
        """n batches [(pix, U)]: pattern 'pixel' one pixel per batch (the bench's walk), 'row' a pixel per row (its
        pixels_per_step B), 'mixed' the two in turn."""
        rows = rows or self.rows
        rng = np.random.default_rng(seed)
        out = []
        for k in range(n):
            per_row = pattern == 'row' or (pattern == 'mixed' and k % 2)
            pix = rng.integers(0, N_PIX, rows) if per_row else np.full(rows, k % N_PIX)
            out.append((np.ascontiguousarray(pix, dtype=np.int32), rng.uniform(size=(rows, self.ndim))))
        return out

    def host(self, batches):
        """[(theta, lnL)] of every batch alone through the host-pointer call."""
        want = []
        for pix, U in batches:
            theta = U.copy()
            want.append((theta, self.cube.loglikelihood_batch(pix, theta)))
        return want

    def oracle_loglike(self, key, pix, U, sel):
        """(theta, lnL) of rows `sel` from the oracle runners of their pixels (cached under `key`: mode-independent)."""
        if key not in self._oracle_cache:
            theta, lnl = U[sel].copy(), np.empty(len(sel))
            ps = pix[sel]
            for p in np.unique(ps):
                m = ps == p
                t = np.ascontiguousarray(theta[m])
                lnl[m] = self.oracle[p].loglikelihood_batch(t)
                theta[m] = t
            self._oracle_cache[key] = (theta, lnl)
        return self._oracle_cache[key]


_WORKLOADS = {}


@pytest.fixture(scope='module')
def workload(engine, nfo):
    def get(name):
        if name not in _WORKLOADS:
            _WORKLOADS[name] = Workload(engine, nfo, name)
        return _WORKLOADS[name]
    yield get
    _WORKLOADS.clear()


def run_loglike(wl, batches, passes=1, between=None):
    """The batches through nfa_runner_loglike_batch_dev, one after the other, then one synchronise; `between(k)` runs
    before batch k is enqueued and (k = n) before the synchronise.  Returns per pass [(theta, lnL)]; the guard bands
    are checked after every pass."""
    from nestfit_amd import _ffi
    lib = _ffi.load()
    h = wl.cube._run.handle
    n, rows = len(batches), batches[0][1].shape[0]
    dev = DeviceArrays(lib, _ffi.check)
    try:
        g_u = GuardedArrays(dev, n, (rows, wl.ndim), np.float64, U_SENTINEL)
        g_p = GuardedArrays(dev, n, (rows,), np.int32, PIX_SENTINEL)
        g_l = GuardedArrays(dev, n, (rows,), np.float64, np.nan)
        for k, (pix, U) in enumerate(batches):
            g_p.put(k, pix)
        out = []
        for _ in range(passes):
            for k, (pix, U) in enumerate(batches):
                g_u.put(k, U)
                g_l.put(k, np.full(rows, np.nan))
            for k in range(n):
                if between:
                    between(k)
                _ffi.check(lib.nfa_runner_loglike_batch_dev(h, g_p.ptr(k), g_u.ptr(k), g_l.ptr(k), rows))
            if between:
                between(n)
            _ffi.check(lib.nfa_runner_synchronize(h))
            assert g_u.bands_intact(), 'unit-cube guard band changed'
            assert g_p.bands_intact(), 'pixel guard band changed'
            assert g_l.bands_intact(), 'lnL guard band changed'
            out.append([(g_u.get(k), g_l.get(k)) for k in range(n)])
        return out
    finally:
        dev.free()


def assert_same_bits(got, want, what):
    for k, ((th, ln), (wt, wl_)) in enumerate(zip(got, want)):
        assert np.array_equal(th, wt, equal_nan=True), f'{what}: theta of batch {k}'
        assert np.array_equal(ln, wl_, equal_nan=True), f'{what}: lnL of batch {k}'


def assert_oracle(wl, mode, got, batches, tag, sel):
    for k, ((th, ln), (pix, U)) in enumerate(zip(got, batches)):
        tc, lc = wl.oracle_loglike((tag, k), pix, U, sel)
        # (the prior transform's bar of test_gpu_parity: over every row of the batches the device's theta sits up to
        # ~1e-10 from the oracle's, above the 1e-11 a 64-row sample of test_full_size_configs meets)
        np.testing.assert_allclose(th[sel], tc, rtol=1e-9, atol=1e-10, err_msg=f'{tag} theta, batch {k}')
        np.testing.assert_allclose(ln[sel], lc, rtol=LNL_RTOL[mode], err_msg=f'{tag} lnL, batch {k}')


@pytest.mark.parametrize('pattern', ['pixel', 'row'])
@pytest.mark.parametrize('mode', MODES)
def test_headline_groups_of_eight(engine, workload, mode, pattern):
    """Case 1: eight 4096-row C2 batches as one group -- table mode: two-group set-up (B = 32768 > 64 n_cu) and
    lnl_kernel_queue<false, 2>; against the host call of each batch alone (one wave per unit: another kernel) bit for
    bit, every row against the oracle, and with the queue off the same bits again."""
    wl = workload('C2')
    batches = wl.draw(8, seed=11, pattern=pattern)
    with engine_state(engine, mode, coalesce=8):
        want = wl.host(batches)
        got = run_loglike(wl, batches)[0]
        assert_same_bits(got, want, f'{mode} {pattern}')
        assert_oracle(wl, mode, got, batches, ('headline', pattern), np.arange(wl.rows))
        if mode == 'table':
            from nestfit_amd import _ffi
            _ffi.set_option('lnl_queue', 0)                  # the same group, every wave one unit (lnl_kernel)
            assert_same_bits(run_loglike(wl, batches)[0], want, 'lnl_queue 0')


# (coalesce, batches, rows): the path each group takes on a 256-CU part -- the queue from two units per resident wave
# (16384 units: two C2 batches of 4096 rows), the two-group set-up from B > 64 n_cu = 16384 rows with every batch a
# multiple of 128 rows
THRESHOLDS = [
    (8, 1, 4096),    # one batch alone: 8192 units, below the queue (lnl_kernel), one-group set-up
    (2, 2, 4096),    # 16384 units: exactly on the queue threshold (queue); B = 8192: one-group set-up
    (3, 3, 4096),    # queue; one-group set-up
    (4, 4, 4096),    # queue; B = 16384 = 64 n_cu, not above it: one-group set-up
    (5, 5, 4096),    # queue; B = 20480: two-group set-up
    (8, 11, 4096),   # a group of eight (queue, two-group set-up) and a rest of three (queue, one-group set-up)
    (8, 8, 4032),    # 4032 = 63 x 64 is no multiple of 128: one-group set-up at B = 32256; queue
]


@pytest.mark.parametrize('coalesce,n,rows', THRESHOLDS, ids=[f'g{c}-n{n}-r{r}' for c, n, r in THRESHOLDS])
@pytest.mark.parametrize('mode', MODES)
def test_group_sizes_around_the_thresholds(engine, workload, mode, coalesce, n, rows):
    """Case 2: group sizes on both sides of the queue and two-group set-up thresholds; pixels per batch and per row
    in turn."""
    wl = workload('C2')
    batches = wl.draw(n, seed=100 + 10 * n + coalesce + rows, pattern='mixed', rows=rows)
    with engine_state(engine, mode, coalesce=coalesce):
        want = wl.host(batches)
        got = run_loglike(wl, batches)[0]
        assert_same_bits(got, want, f'{mode} coalesce {coalesce} x {n} of {rows}')
        assert_oracle(wl, mode, got, batches, ('thresholds', coalesce, n, rows), np.arange(0, rows, 16))


@pytest.mark.parametrize('mode', MODES)
def test_three_groups_in_flight_twice(engine, workload, mode):
    """Case 3: 24 batches before one synchronise -- three groups of eight on three stream lanes, each with its own
    queue counters -- and the whole sequence again: the same bits, so every launch left its counters at zero."""
    wl = workload('C2')
    batches = wl.draw(24, seed=31, pattern='mixed')
    with engine_state(engine, mode, coalesce=8):
        want = wl.host(batches)
        first, second = run_loglike(wl, batches, passes=2)
        assert_same_bits(first, want, f'{mode} first pass')
        assert_same_bits(second, first, f'{mode} second pass')
        assert_oracle(wl, mode, first, batches, ('in_flight',), np.arange(0, wl.rows, 64))


@pytest.mark.parametrize('mode', MODES)
def test_predict_groups_of_eight(engine, nfo, workload, mode):
    """Case 4: eight 4096-row C2 nfa_runner_predict_batch_dev calls, every batch its own spectra and lnL arrays
    (table mode: lnl_kernel_queue<true, 2> with a group): the host call's spectra and lnL bit for bit, theta untouched,
    a sample against the oracle's amm_predict."""
    from nestfit_amd import _ffi
    wl = workload('C2')
    n, rows = 8, wl.rows
    draws = wl.draw(n, seed=41, pattern='mixed')
    # physical parameters: the oracle's prior transform of unit-cube rows
    batches = [(pix, wl.oracle_loglike(('predict', k), pix, U, np.arange(rows))[0]) for k, (pix, U) in enumerate(draws)]
    lib = _ffi.load()
    h = wl.cube._run.handle
    dev = DeviceArrays(lib, _ffi.check)
    with engine_state(engine, mode, coalesce=8):
        try:
            g_t = GuardedArrays(dev, n, (rows, wl.ndim), np.float64, synth.TRUTH_2COMP)
            g_p = GuardedArrays(dev, n, (rows,), np.int32, PIX_SENTINEL)
            g_s = GuardedArrays(dev, n, (rows, wl.chan_tot), np.float64, np.nan)
            g_l = GuardedArrays(dev, n, (rows,), np.float64, np.nan)
            nan_spec = np.full((rows, wl.chan_tot), np.nan)
            for k, (pix, theta) in enumerate(batches):
                g_t.put(k, theta)
                g_p.put(k, pix)
                g_s.put(k, nan_spec)
                g_l.put(k, np.full(rows, np.nan))
            for k in range(n):
                _ffi.check(lib.nfa_runner_predict_batch_dev(h, g_p.ptr(k), g_t.ptr(k), rows, g_s.ptr(k), g_l.ptr(k)))
            _ffi.check(lib.nfa_runner_synchronize(h))
            assert g_t.bands_intact() and g_p.bands_intact() and g_s.bands_intact() and g_l.bands_intact()
            sel = np.arange(0, rows, 512)
            for k, (pix, theta) in enumerate(batches):
                want_spec, want_lnl = wl.cube.predict_batch(pix, theta)
                spec, lnl = g_s.get(k), g_l.get(k)
                assert np.array_equal(spec, want_spec, equal_nan=True), f'{mode}: spectra of batch {k}'
                assert np.array_equal(lnl, want_lnl, equal_nan=True), f'{mode}: lnL of batch {k}'
                assert np.array_equal(g_t.get(k), theta), f'theta of batch {k} changed'
                for b in sel:
                    runner = wl.oracle[pix[b]]
                    tot = 0.0
                    for s, sc in enumerate(runner.spectra):
                        nfo.amm_predict(sc, theta[b])
                        pc, pg = sc.get_spec(), spec[b, s * wl.n_chan:(s + 1) * wl.n_chan]
                        assert np.array_equal(pg == 0, pc == 0), (mode, k, b, s)
                        assert (np.abs(pg - pc) <= TB_RTOL * np.abs(pc) + TB_ATOL_K[mode]).all(), (mode, k, b, s)
                        tot += sc.loglikelihood
                    assert lnl[b] == pytest.approx(tot, rel=LNL_RTOL[mode]), (mode, k, b)
        finally:
            dev.free()


@pytest.mark.parametrize('mode', MODES)
def test_c4_groups_of_five(engine, workload, mode):
    """Case 5: seven 4096-row C4 batches (3 spectra x 2048 channels, three components): a group of five -- the most
    below eight waves per wave slot; table mode lnl_kernel_queue<false, 3> -- and a rest of two."""
    wl = workload('C4')
    batches = wl.draw(7, seed=51, pattern='mixed')
    with engine_state(engine, mode, coalesce=8):
        want = wl.host(batches)
        got = run_loglike(wl, batches)[0]
        assert_same_bits(got, want, f'{mode} C4')
        assert_oracle(wl, mode, got, batches, ('c4',), np.arange(0, wl.rows, 16))


# (option, value set before the batches, value set while they are held, batches, rows, index of the batch before which
# the option changes (n: after the last one, before the synchronise))
MID_HOLD = [
    ('setup_ti', 32, 64, 3, 96, 3),      # held as multiples of 32 rows; a flush under 64 would map workgroups to batches wrongly
    ('lnl_queue', 1, 0, 6, 4096, 3),
    ('setup_sub', 0, 1, 8, 4096, 5),
    ('coalesce', 8, 2, 8, 4096, 5),
]


@pytest.mark.parametrize('option,before,after,n,rows,at', MID_HOLD, ids=[m[0] for m in MID_HOLD])
@pytest.mark.parametrize('mode', MODES)
def test_options_changed_while_batches_are_held(engine, workload, mode, option, before, after, n, rows, at):
    """Case 6: an option changed while batches are held launches them first (nfa_set_option), under the options
    they were accepted with: the host call's bits, the guard bands intact."""
    from nestfit_amd import _ffi
    wl = workload('C2')
    batches = wl.draw(n, seed=61, pattern='mixed', rows=rows)
    with engine_state(engine, mode):
        want = wl.host(batches)
        _ffi.set_option(option, before)

        def between(k):
            if k == at:
                _ffi.set_option(option, after)
        got = run_loglike(wl, batches, between=between)[0]
        assert_same_bits(got, want, f'{mode}: {option} {before} -> {after}')


def test_the_queue_kernel_runs_for_every_batch_of_the_group(engine):
    """Case 7: the groups of cases 1, 4 and 5 reach lnl_kernel_queue, and every batch of the group has units in it
    (the test library's trace of the last launch, in a child process of its own)."""
    lib_path = ROOT / 'nestfit_amd' / 'lib' / 'libnestfit_amd_test.so'
    assert lib_path.exists()
    env = dict(os.environ, NFA_ENGINE_LIB=str(lib_path))
    res = subprocess.run([sys.executable, str(ROOT / 'tests' / 'queue_trace_worker.py')], env=env, cwd=str(ROOT),
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    out = json.loads(res.stdout.strip().splitlines()[-1])
    for case in ('C2 n=8', 'C2 n=2', 'C2 spectra n=8', 'C4 n=5'):
        r = out[case]
        assert r['queue'], (case, r)
        assert r['batches'] == list(range(r['n'])), (case, r)
    if out['n_cu'] == 256:
        assert not out['C2 n=1']['queue'], out['C2 n=1']       # one batch alone: one wave per unit
