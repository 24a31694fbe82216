"""The table mode's likelihood kernels outside their line blocks -- the unit prologue (line set-up, windows) and the head
of every row (lane values, hit masks, run set-up, the odd line of a run, the dispatch before the Tb pass, the chi^2 pair):
lnL and theta of the queue form at its smallest launch must keep the bits recorded from the commit before that code was
shortened (tests/golden/row_heads_*.npy, written by `python tests/test_row_heads.py --write-golden` on a GPU with that
commit's build), equal the one-unit-per-wave form bit for bit, and agree with the CPU oracle.

The launch: the queue kernel runs from 16384 units and 512 channels (nfa_launch_plan.h: plan_lnl), so 8192 rows x 2 spectra,
sent through nfa_runner_loglike_batch_dev as two batches of 4096 that the engine coalesces (BatchGroup.n = 2).

The draws come from a prior set far wider than the benchmark's -- voff uniform over +-45 km/s on a band of +-30 km/s, sigm
over [0.02, 8.02] km/s -- and the first rows of each batch are set by hand (DRAW_* below), so that the cases do not hang on
the seed:
  * voff at and near both ends of its range: the hyperfine lines of NH3 (1,1) span +-19.5 km/s about voff, so at
    |voff| = 45 most of a component's lines lie beyond the band's edge (empty windows) and the rest are cut by it (clipped);
  * sigm = 0.02 km/s: a window of 5 sigm = 0.1 km/s either side is 3 to 5 channels at 1024 channels (0.059 km/s each), narrower
    than the 0.3 km/s and more between the lines of the outer satellite groups: rows that hold ONE line (runs of 1, the odd-line
    block alone), and lines whose window holds no channel centre at all at 512 channels;
  * sigm above 6.5 km/s (u = 0.9999 of its prior): windows of +-32 km/s and more, wider than the band: every row holds all 18 (or 21) lines of the transition (runs of
    18 and 21: nine and ten pair blocks, with and without an odd line in front).
A centre or a width that is not finite cannot be sent in: the entry point takes unit-cube rows, and theta is the prior set's.
"""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / 'tests' / 'golden'
ROWS, N_BATCH = 4096, 2
TRANS = (1, 2)
CASES = [(n, ncomp) for ncomp in (2, 3) for n in (512, 577, 1024)]
LNL_RTOL_TABLE = 1e-9                     # test_gpu_parity.LNL_RTOL['table']
DRAW_VOFF_U = (0.0, 0.03, 0.17, 0.5, 0.83, 0.97, 0.9999)
DRAW_SIGM_U = (0.0, 0.004, 0.05, 0.9999)


def wide_priors():
    """Independent priors per parameter (core.Prior): voff uniform over [-45, 45] km/s, sigm Beta(1.5, 5) over [0.02, 8.02]."""
    from scipy import stats
    from nestfit_amd.core import ConstantPrior, Distribution, Prior, PriorTransformer
    u = np.linspace(0, 1, 500)
    flat = np.ones_like(u) / u.size
    return PriorTransformer(np.array([
        Prior(Distribution(90.0 * u - 45.0, flat.copy()), 0),
        Prior(Distribution(23.0 * u + 7.0, stats.beta(3.0, 6.7).pdf(u)), 1),
        Prior(Distribution(9.26 * u + 2.8, stats.beta(1.0, 2.5).pdf(u)), 2),
        Prior(Distribution(4.0 * u + 12.5, stats.beta(10.0, 8.5).pdf(u)), 3),
        Prior(Distribution(8.0 * u + 0.02, stats.beta(1.5, 5.0).pdf(u)), 4),
        ConstantPrior(0, 5),
    ]))


def draws(ncomp):
    """Unit-cube rows [N_BATCH * ROWS, 6 ncomp] (parameter p of component c in column p * ncomp + c): random rows, and at
    the head of each batch the 28 (voff, sigm) pairs of DRAW_* for component 0, with component 1 at the mirrored voff and the
    next sigm of the list (a narrow component beside a broad one, both ends of the band in one row)."""
    U = np.random.default_rng(1000 + ncomp).uniform(size=(N_BATCH * ROWS, 6 * ncomp))
    pairs = [(v, s) for v in DRAW_VOFF_U for s in DRAW_SIGM_U]
    for k in range(N_BATCH):
        for i, (v, s) in enumerate(pairs):
            r = k * ROWS + i
            U[r, 0], U[r, 4 * ncomp] = v, s
            U[r, 1], U[r, 4 * ncomp + 1] = min(1.0 - v, 0.9999), DRAW_SIGM_U[(DRAW_SIGM_U.index(s) + 1 + k) % len(DRAW_SIGM_U)]
    return U


def spec_data(n):
    from nestfit_amd.synth import freq_axis
    rng = np.random.default_rng(77 + n)
    return [[freq_axis(t, n), rng.normal(0, 0.2, n), 0.2, t] for t in TRANS]


def theta_digest(theta):
    """One 64-bit word per row from the bits of its doubles (wrapping sum of the words times odd constants): equal digests
    for equal bits, and a changed bit of any parameter changes the row's word."""
    bits = np.ascontiguousarray(theta, dtype=np.float64).view(np.uint64)
    mult = np.array([((2 * k + 1) * 0x9E3779B97F4A7C15) % (1 << 64) for k in range(bits.shape[1])], dtype=np.uint64)
    with np.errstate(over='ignore'):
        return (bits * mult[None, :]).sum(axis=1, dtype=np.uint64)


def run_on_device(run, U):
    """U as N_BATCH batches of ROWS through nfa_runner_loglike_batch_dev, one after the other, then one synchronise:
    (theta, lnL) of all rows."""
    from device_buffers import DeviceArrays
    from nestfit_amd import _ffi
    lib = _ffi.load()
    dev = DeviceArrays(lib, _ffi.check)
    try:
        slots = []
        for k in range(N_BATCH):
            Uk = np.ascontiguousarray(U[k * ROWS:(k + 1) * ROWS])
            slots.append((dev.upload(Uk), dev.empty(8 * ROWS), Uk))
        for d_u, d_l, Uk in slots:
            _ffi.check(lib.nfa_runner_loglike_batch_dev(run._run.handle, None, d_u, d_l, ROWS))
        _ffi.check(lib.nfa_runner_synchronize(run._run.handle))
        theta = np.concatenate([dev.download(d_u, Uk) for d_u, d_l, Uk in slots])
        lnl = np.concatenate([dev.download(d_l, np.empty(ROWS)) for d_u, d_l, Uk in slots])
        return theta, lnl
    finally:
        dev.free()


def evaluate(engine, n, ncomp, queue):
    from nestfit_amd import _ffi
    engine.set_exp_mode('table')
    try:
        _ffi.set_option('lnl_queue', queue)
        run = engine.AmmoniaRunner.from_data(spec_data(n), wide_priors(), ncomp=ncomp)
        return run_on_device(run, draws(ncomp))
    finally:
        _ffi.set_option('lnl_queue', 1)
        engine.set_exp_mode('fast')


def golden_paths(n, ncomp):
    return GOLDEN / f'row_heads_lnl_n{n}_c{ncomp}.npy', GOLDEN / f'row_heads_theta_c{ncomp}.npy'


@pytest.mark.gpu
@pytest.mark.parametrize('n,ncomp', CASES)
def test_row_heads_keep_the_bits(engine, nfo, n, ncomp):
    theta, lnl = evaluate(engine, n, ncomp, 1)
    ndim = 6 * ncomp
    # the draws are what the docstring says: both ends of voff's range, the narrowest and the broadest sigm
    voff, sigm = theta[:, :ncomp], theta[:, 4 * ncomp:5 * ncomp]
    assert voff.min() < -44.9 and voff.max() > 44.9 and sigm.min() < 0.021 and sigm.max() > 6.5
    assert theta.shape == (N_BATCH * ROWS, ndim) and np.all(np.isfinite(lnl))
    # 1. the bits of the commit before the row heads changed
    p_lnl, p_theta = golden_paths(n, ncomp)
    want_lnl, want_theta = np.load(p_lnl), np.load(p_theta)
    assert np.array_equal(theta_digest(theta), want_theta), 'theta'
    diff = np.flatnonzero(lnl.view(np.uint64) != want_lnl.view(np.uint64))
    assert diff.size == 0, f'lnL differs in {diff.size} rows, first {diff[:8]}: {lnl[diff[:8]]} against {want_lnl[diff[:8]]}'
    # 2. one unit per wave (lnl_kernel) gives the queue form's bits
    theta0, lnl0 = evaluate(engine, n, ncomp, 0)
    assert np.array_equal(theta0, theta) and np.array_equal(lnl0.view(np.uint64), lnl.view(np.uint64))
    # 3. 200 rows against the CPU oracle: the hand-set rows of the first batch and a random sample
    U = draws(ncomp)
    pick = np.concatenate([np.arange(len(DRAW_VOFF_U) * len(DRAW_SIGM_U)),
                           np.random.default_rng(3).choice(np.arange(64, N_BATCH * ROWS), 200 - 28, replace=False)])
    cpu = nfo.AmmoniaRunner([nfo.AmmoniaSpectrum(*sd) for sd in spec_data(n)], nfo.PriorSet(wide_priors().lower()), ncomp=ncomp)
    Uc = U[pick].copy()
    want = cpu.loglikelihood_batch(Uc)
    np.testing.assert_allclose(theta[pick], Uc, rtol=1e-9, atol=1e-10)
    np.testing.assert_allclose(lnl[pick], want, rtol=LNL_RTOL_TABLE)


# ---- the cut-off's short form (csrc/nfa_line_window.h) on the host: no GPU ----------------------------------------------
CUTOFF_SHIM = r"""
#include "nfa_line_window.h"
extern "C" void windows(long n, const double *a, const double *w, double nu_chan, double r_chan,
                        double *f_ref, double *f_short, int *same) {
    for (long i = 0; i < n; ++i) {
        double ql, qh;
        nf_window_quot_ref(a[i], 0.5 / (w[i] * w[i]), nu_chan, r_chan, ql, qh);      // hf_idenom as nf_line forms it
        f_ref[2 * i] = floor(ql); f_ref[2 * i + 1] = floor(qh);
        same[i] = nf_window_quot_short(a[i], w[i], nu_chan, r_chan, ql, qh);
        f_short[2 * i] = floor(ql); f_short[2 * i + 1] = floor(qh);
    }
}
"""


@pytest.fixture(scope='module')
def cutoff_lib(tmp_path_factory):
    import subprocess
    tmp = tmp_path_factory.mktemp('line_window')
    src, so = tmp / 'w.cpp', tmp / 'libw.so'
    src.write_text(CUTOFF_SHIM)
    res = subprocess.run(['g++', '-std=c++17', '-Wall', '-Werror', '-O2', '-ffp-contract=off', '-shared', '-fPIC',
                          f'-I{ROOT / "nestfit_amd" / "csrc"}', str(src), '-o', str(so)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    lib = C.CDLL(str(so))
    lib.windows.argtypes = [C.c_long] + [C.c_void_p] * 2 + [C.c_double] * 2 + [C.c_void_p] * 3
    return lib


def window_floors(lib, a, w, nu_chan, r_chan):
    a, w = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(w, dtype=np.float64)
    f_ref, f_short, same = np.empty((a.size, 2)), np.empty((a.size, 2)), np.empty(a.size, dtype=np.int32)
    lib.windows(a.size, a.ctypes.data, w.ctypes.data, nu_chan, r_chan, f_ref.ctypes.data, f_short.ctypes.data, same.ctypes.data)
    return f_ref, f_short, same.astype(bool)


def clipped(f, n):
    """lo, hi of nf_line from the two floors (hyperfine.pyx:78-86)."""
    empty = (f[:, 1] < 0) | (f[:, 0] > n - 1) | ~np.isfinite(f).all(axis=1)
    return np.where(empty, 0, np.clip(f[:, 0], 0, n - 1)), np.where(empty, 0, np.clip(f[:, 1], 0, n - 1))


NU0, CKMS, N_CHAN = 23.6944955e9, 299792.458, 1024
NU_CHAN = NU0 * (60.0 / (N_CHAN - 1)) / CKMS              # the channel width of freq_axis(1, 1024): 4.6 kHz


@pytest.mark.parametrize('r_chan', [1.0 / NU_CHAN, 0.0], ids=['markstein', 'division'])
def test_cutoff_short_form_random_lines(cutoff_lib, r_chan):
    """1e6 random lines, centres from before the band to behind it, sigm 0.02 .. 8 km/s (and a few far outside the range the short
    form accepts): wherever the short form says "same", both floors are the reference sequence's; and it says so nearly always."""
    rng = np.random.default_rng(5)
    n = 1_000_000
    a = rng.uniform(-0.3, 1.3, n) * N_CHAN * NU_CHAN
    w = 10 ** rng.uniform(np.log10(0.02), np.log10(8.0), n) / CKMS * NU0
    w[:2000] = 10 ** rng.uniform(-320, 300, 2000)             # subnormal, tiny, huge, overflowing w^2
    w[2000:2010] = [0.0, -0.0, np.inf, -np.inf, np.nan, -1e4, 1e-100, 1e100, 5e-324, 1.7e308]
    f_ref, f_short, same = window_floors(cutoff_lib, a, w, NU_CHAN, r_chan)
    assert np.array_equal(f_short[same], f_ref[same])
    lo_r, hi_r = clipped(f_ref, N_CHAN)
    lo_s, hi_s = clipped(np.where(same[:, None], f_short, f_ref), N_CHAN)         # the kernel: the reference's where not "same"
    assert np.array_equal(lo_s, lo_r) and np.array_equal(hi_s, hi_r)
    aw = np.abs(w[:2010])
    assert not same[:2010][(aw < 1e-100) | (aw > 1e100) | ~np.isfinite(aw)].any()
    assert same[2010:].mean() > 1 - 1e-5, same[2010:].mean()


def test_cutoff_short_form_near_integers(cutoff_lib):
    """Centres placed so that a quotient falls within a few ulps of an integer, on either side of it: a = k nu_chan +- 5 w stepped
    through +-48 neighbouring doubles, for both ends, 2000 (k, w) pairs.  There the two sequences' cut-offs, which differ in the
    last bits, can put the quotient on different sides of k: the short form must not say "same" for any such line, and the
    windows that result must be the reference's for all of them."""
    rng = np.random.default_rng(6)
    k = rng.integers(-50, N_CHAN + 50, 2000).astype(np.float64)
    w = 10 ** rng.uniform(np.log10(0.02), np.log10(8.0), 2000) / CKMS * NU0
    a_parts = []
    for sign in (+1.0, -1.0):                                  # the lower end (a - c) and the upper end (a + c) at k nu_chan
        base = k * NU_CHAN + sign * 5.0 * w
        for step in range(-48, 49):
            b = base.copy()
            for _ in range(abs(step)):
                b = np.nextafter(b, np.inf if step > 0 else -np.inf)
            a_parts.append(b)
    a = np.concatenate(a_parts)
    ww = np.tile(w, len(a_parts))
    for r_chan in (1.0 / NU_CHAN, 0.0):
        f_ref, f_short, same = window_floors(cutoff_lib, a, ww, NU_CHAN, r_chan)
        differ = (f_ref != f_short).any(axis=1)
        print(f'r_chan {r_chan:.3g}: {a.size} lines, {int((~same).sum())} sent to the reference sequence, {int(differ.sum())} whose floors differ')
        assert not (same & differ).any()
        assert np.array_equal(f_short[same], f_ref[same])
        lo_r, hi_r = clipped(f_ref, N_CHAN)
        lo_s, hi_s = clipped(np.where(same[:, None], f_short, f_ref), N_CHAN)
        assert np.array_equal(lo_s, lo_r) and np.array_equal(hi_s, hi_r)
        # the placement works: at zero steps the quotient is within the guard of k (nearly all lines are caught there)
        assert (~same).mean() > 0.25


if __name__ == '__main__':
    if sys.argv[1:] != ['--write-golden']:
        sys.exit('usage: python tests/test_row_heads.py --write-golden   (on a GPU, with the build whose bits are to be kept)')
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / 'tests'))
    import nestfit_amd
    from nestfit_amd import _ffi
    _ffi.engine()
    for n, ncomp in CASES:
        theta, lnl = evaluate(nestfit_amd, n, ncomp, 1)
        p_lnl, p_theta = golden_paths(n, ncomp)
        np.save(p_lnl, lnl)
        d = theta_digest(theta)
        if p_theta.exists():
            assert np.array_equal(np.load(p_theta), d), 'theta depends on the channel count?'
        np.save(p_theta, d)
        print(n, ncomp, 'written', float(lnl.min()), float(lnl.max()))
