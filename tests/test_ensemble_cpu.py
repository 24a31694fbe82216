"""The ensemble sampler without a GPU: the plan header (csrc/nfa_ensemble_plan.h, plain C++17, compiled alone by g++) and
the numpy twin (nestfit_amd/ensemble.py) on likelihoods with known answers."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from nestfit_amd import ensemble
from nestfit_amd.nested import LOG_ZERO

ROOT = Path(__file__).resolve().parent.parent

SHIM = r'''
#include "nfa_ensemble_plan.h"
extern "C" {
long long consts(int i) {
    const long long v[] = {NFA_ENS_MAX_WALKERS, NFA_ENS_MAX_Q, NFA_ENS_MAX_SORT, (long long)NFA_ENS_TAG, (long long)ENS_A_MAX,
                           ENS_PIECE_ROWS, ENS_RED_DOUBLES};
    return v[i];
}
const char *check_walkers(int W, int D) { return ens_check_walkers(W, D); }
const char *check_run(long long n_steps, long long n_burn, long long thin, double a) { return ens_check_run(n_steps, n_burn, thin, a); }
const char *check_levels(const double *q, int nq, long long n) { return ens_check_levels(q, nq, n); }
long long n_keep(long long n_steps, long long n_burn, long long thin) { return ens_n_keep(n_steps, n_burn, thin); }
int keeps(long long s, long long n_burn, long long thin) { return ens_keeps(s, n_burn, thin) ? 1 : 0; }
long long keep_slot(long long s, long long n_burn, long long thin) { return ens_keep_slot(s, n_burn, thin); }
void bytes(long long P, int W, int ndim, int D, long long n_steps, long long n_keep, long long *out) {
    const EnsBytes B = ens_bytes(P, W, ndim, D, n_steps, n_keep);
    out[0] = B.state; out[1] = B.chain; out[2] = B.trace; out[3] = B.total;
}
void geom(int which, long long P, int W, int ndim, long long n, int nq, long long *out) {
    const EnsGeom G = which == 0 ? ens_walk_geom(P, W) : which == 1 ? ens_trace_geom(P) : which == 2 ? ens_keep_geom(P, W, ndim)
                                                                                       : ens_summary_geom(P, n, nq);
    out[0] = G.grid; out[1] = G.threads; out[2] = (long long)G.lds;
}
long long sort_len(long long n, int nq) { return ens_sort_len(n, nq); }
}
'''


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('ens_plan')
    src = tmp / 'plan.cpp'
    src.write_text(SHIM)
    so = tmp / 'libensplan.so'
    res = subprocess.run(['g++', '-std=c++17', '-Wall', '-Werror', '-O1', '-shared', '-fPIC', f'-I{ROOT / "nestfit_amd" / "csrc"}',
                          str(src), '-o', str(so)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    lib = C.CDLL(str(so))
    LL = C.c_longlong
    for name in ('consts', 'n_keep', 'keep_slot', 'sort_len'):
        getattr(lib, name).restype = LL
    for name in ('check_walkers', 'check_run', 'check_levels'):
        getattr(lib, name).restype = C.c_char_p
    lib.check_walkers.argtypes = [C.c_int, C.c_int]
    lib.check_run.argtypes = [LL, LL, LL, C.c_double]
    lib.check_levels.argtypes = [C.c_void_p, C.c_int, LL]
    lib.n_keep.argtypes = lib.keeps.argtypes = lib.keep_slot.argtypes = [LL, LL, LL]
    lib.bytes.argtypes = [LL, C.c_int, C.c_int, C.c_int, LL, LL, C.c_void_p]
    lib.geom.argtypes = [C.c_int, LL, C.c_int, C.c_int, LL, C.c_int, C.c_void_p]
    lib.sort_len.argtypes = [LL, C.c_int]
    return lib


# ---- the plan header --------------------------------------------------------------------------------------------------
def test_constants_are_the_twins(lib):
    assert [lib.consts(i) for i in range(7)] == [512, 8, 8192, 1 << 61, 16, 1 << 20, 64]
    assert (ensemble.MAX_WALKERS, ensemble.MAX_Q, ensemble.MAX_SORT, ensemble.ENS_TAG, ensemble.A_MAX) == (512, 8, 8192, 1 << 61, 16.0)
    # clear of the nested sampler's stream tags: proposal counts below, NS_TAG_LIVE = 2^62 above
    assert 1 << 40 < ensemble.ENS_TAG and ensemble.ENS_TAG + 2 * (1 << 40) + 1 < 1 << 62


def test_every_check_has_its_sentence(lib):
    assert lib.check_walkers(16, 6) is None and lib.check_walkers(14, 6) is None and lib.check_walkers(512, 60) is None
    assert b'even' in lib.check_walkers(15, 3)
    assert b'sampled dimensions + 1' in lib.check_walkers(12, 6)
    assert b'NFA_ENS_MAX_WALKERS' in lib.check_walkers(514, 3) and b'NFA_ENS_MAX_WALKERS' in lib.check_walkers(0, 0)
    assert lib.check_run(30, 6, 4, 2.0) is None and lib.check_run(10, 9, 1, 16.0) is None
    for a in (1.0, 0.5, 16.5, float('nan')):
        assert b'stretch scale' in lib.check_run(30, 6, 4, a)
    assert b'thin' in lib.check_run(30, 6, 0, 2.0)
    assert b'n_burn' in lib.check_run(10, 10, 1, 2.0) and b'n_burn' in lib.check_run(10, 12, 1, 2.0) and b'n_burn' in lib.check_run(10, -1, 1, 2.0)
    assert b'no step is kept' in lib.check_run(10, 5, 6, 2.0)
    assert b'n_steps' in lib.check_run(0, 0, 1, 2.0)
    q = (C.c_double * 9)(0.0, 0.16, 0.5, 0.84, 1.0, 0.1, 0.2, 0.3, 0.4)
    assert lib.check_levels(q, 8, 8192) is None and lib.check_levels(None, 0, 1 << 30) is None
    assert b'NFA_ENS_MAX_Q' in lib.check_levels(q, 9, 100)
    assert b'NFA_ENS_MAX_SORT' in lib.check_levels(q, 3, 8193)
    for bad in (-1e-9, 1.0000001, float('nan')):
        q[1] = bad
        assert b'outside [0, 1]' in lib.check_levels(q, 3, 100)


def test_which_steps_are_kept(lib):
    for n_steps, n_burn, thin, kept in ((24, 5, 4, [9, 13, 17, 21]), (10, 9, 1, [10]), (10, 0, 3, [3, 6, 9])):
        assert lib.n_keep(n_steps, n_burn, thin) == len(kept) == ensemble.n_keep_of(n_steps, n_burn, thin)
        steps = [s for s in range(1, n_steps + 1) if lib.keeps(s, n_burn, thin)]
        assert steps == kept == [s for s in range(1, n_steps + 1) if ensemble.keeps(s, n_burn, thin)]
        assert [lib.keep_slot(s, n_burn, thin) for s in kept] == list(range(len(kept)))


def test_byte_counts(lib):
    out = (C.c_longlong * 4)()
    for P, W, ndim, D, n_steps, n_keep in ((1, 16, 6, 6, 30, 6), (1024, 64, 12, 10, 2000, 128), (3, 512, 60, 60, 10, 10)):
        lib.bytes(P, W, ndim, D, n_steps, n_keep, out)
        state, chain, trace, total = out[0], out[1], out[2], out[3]
        assert chain == 8 * P * n_keep * W * (ndim + 1) and trace == 8 * P * n_steps * (D + 1)
        walkers, rows = P * W, P * W // 2
        assert state == (8 * walkers * (D + ndim + 1) + 4 * walkers + 8 * rows * (ndim + D + 1) + 8 * rows + 8 * 3 * P + 4 * P + 4 * D
                         + 8 * P * (2 * ndim + ndim + 1 + 8 * ndim) + 64)
        assert total == state + chain + trace
    lib.bytes(2, 16, 6, 6, 30, 6, out)
    two = out[3]
    lib.bytes(1, 16, 6, 6, 30, 6, out)
    assert two <= 2 * out[3]                                   # a group of n pixels fits n times the bytes of one
    assert ensemble.pixel_groups(9, 100, 350) == [(0, 3), (3, 6), (6, 9)] and ensemble.pixel_groups(4, 100, 10) == [(0, 1), (1, 2), (2, 3), (3, 4)]
    assert ensemble.pixel_groups(5, 100, 1 << 30) == [(0, 5)]


def test_geometry(lib):
    out = (C.c_longlong * 3)()
    for W, threads in ((2, 64), (16, 64), (128, 64), (130, 128), (160, 128), (384, 192), (512, 256)):
        lib.geom(0, 7, W, 6, 0, 0, out)
        assert (out[0], out[1], out[2]) == (7, threads, 0) and W // 2 <= threads <= 256
    lib.geom(1, 5, 16, 6, 0, 0, out)
    assert (out[0], out[1]) == (5, 64)
    lib.geom(2, 3, 16, 6, 0, 0, out)
    assert (out[0], out[1]) == (-(-3 * 16 * 7 // 256), 256)
    for n, nq, threads, srt in ((96, 3, 64, 128), (1, 3, 64, 2), (8192, 8, 1024, 8192), (8192, 0, 1024, 0), (100000, 0, 1024, 0),
                                (1000, 1, 512, 1024)):
        lib.geom(3, 4, 0, 0, n, nq, out)
        assert lib.sort_len(n, nq) == srt
        assert (out[0], out[1], out[2]) == (4, threads, 8 * (64 + srt))
        assert out[2] % 16 == 0 and out[2] <= 160 * 1024
    lib.geom(3, 4, 0, 0, 8192, 8, out)
    assert out[2] == 64 * 1024 + 512                           # the cap: 64 KB of samples behind the waves' partial results


# ---- the twin ---------------------------------------------------------------------------------------------------------
def _start(P, W, ndim, seed, lo=0.0, hi=1.0):
    return np.random.default_rng(seed).uniform(lo, hi, size=(P, W, ndim))


def _ks_uniform(x):
    """Kolmogorov-Smirnov statistic against the uniform law and its asymptotic p-value."""
    x = np.sort(x)
    n = x.size
    d = max(np.max(np.arange(1, n + 1) / n - x), np.max(x - np.arange(n) / n))
    t = (np.sqrt(n) + 0.12 + 0.11 / np.sqrt(n)) * d
    k = np.arange(1, 101)
    return d, float(2 * np.sum((-1.0) ** (k - 1) * np.exp(-2 * k * k * t * t)))


def test_constant_likelihood_keeps_the_flat_target():
    """The stretch move with outside-rejection keeps the uniform law.  Eight walkers in three dimensions decorrelate in
    about 90 steps (Sokal's estimate per walker), so samples 50 steps apart are not independent and the p-values lean low:
    of the seeds 1 .. 12, eleven pass at 1e-3 in every coordinate (smallest 0.004) and seed 11 gives 7e-4 in one; over all
    twelve the pooled mean is 0.494 .. 0.521 and the variance 0.081 .. 0.085 (1 / 12 = 0.0833)."""
    D, W, n_steps = 3, 8, 4000
    res = ensemble.run_twin(lambda pix, T: np.zeros(T.shape[0]), D, 1, W, _start(1, W, D, 3), n_steps, 0, 1, seed=1)
    assert res.outside[0] > 0 and res.evaluated[0] == n_steps * W and 0 < res.accepted[0] < n_steps * W
    u = res.chain_theta[0]                                     # (the likelihood leaves u in the row: theta = u)
    assert u.shape == (n_steps, W, D) and ((u > 0) & (u < 1)).all()
    for d in range(D):
        stat, pval = _ks_uniform(u[49::50, :, d].ravel())
        assert pval > 1e-3, (d, stat, pval)


def test_gaussian_means_and_variances():
    sigma = np.array([0.02, 0.05, 0.1, 0.03])
    D, W, n_steps = 4, 32, 3000
    n_burn = n_steps // 2

    def loglike(pix, T):
        return -0.5 * (((T - 0.5) / sigma) ** 2).sum(axis=1)
    res = ensemble.run_twin(loglike, D, 1, W, _start(1, W, D, 5, 0.4, 0.6), n_steps, n_burn, 1, seed=2)
    x = res.chain_theta[0]                                     # [n_keep, W, D]
    step_mean = x.mean(axis=1)                                 # per-step ensemble means
    step_var = ((x - 0.5) ** 2).mean(axis=1)                   # ... of the squared distance from the known centre
    for series, truth in ((step_mean, np.full(D, 0.5)), (step_var, sigma ** 2)):
        batches = series.reshape(20, -1, D).mean(axis=1)
        est, se = batches.mean(axis=0), batches.std(axis=0, ddof=1) / np.sqrt(20)
        assert np.all(np.abs(est - truth) < 5 * se), (est, truth, se)
        assert np.all(se < 0.2 * np.where(truth == 0.5, sigma, truth))      # and the test has teeth


def test_free_mask_samples_only_the_free_slots():
    ndim, mask, W = 5, [1, 0, 1, 1, 0], 10
    seen = []

    def loglike(pix, T):
        assert (T[:, 1] == 0.5).all() and (T[:, 4] == 0.5).all()
        seen.append(T.shape[0])
        return -0.5 * (((T[:, [0, 2, 3]] - 0.5) / 0.1) ** 2).sum(axis=1)
    u0 = _start(2, W, ndim, 8)
    res = ensemble.run_twin(loglike, ndim, 2, W, u0, 40, 0, 1, seed=4, free_mask=mask)
    assert res.trace.shape == (2, 40, 4) and res.state.D == 3
    assert (res.u[:, :, [1, 4]] == 0.5).all() and seen[0] == 2 * W and set(seen[1:]) == {W}
    with pytest.raises(ValueError):                            # W / 2 >= D + 1 counts the sampled slots: 3 pass, 5 do not
        ensemble.run_twin(loglike, ndim, 2, W, u0, 40, 0, 1, seed=4)
    # (D - 1) of the acceptance is the sampled count: the same problem written in three dimensions takes the same decisions
    res3 = ensemble.run_twin(lambda pix, T: -0.5 * (((T - 0.5) / 0.1) ** 2).sum(axis=1), 3, 2, W, u0[:, :, [0, 2, 3]], 40, 0, 1, seed=4)
    assert np.array_equal(res3.u, res.u[:, :, [0, 2, 3]]) and np.array_equal(res3.accepted, res.accepted)
    assert np.array_equal(res3.trace, res.trace)


def test_same_arguments_same_bits_and_how_a_run_continues():
    D, W = 3, 8
    f = lambda pix, T: -0.5 * (((T - 0.4) / 0.1) ** 2).sum(axis=1)
    u0 = np.repeat(_start(1, W, D, 1), 2, axis=0)              # two pixels, the same start
    a = ensemble.run_twin(f, D, 2, W, u0, 20, 4, 2, seed=7)
    b = ensemble.run_twin(f, D, 2, W, u0, 20, 4, 2, seed=7)
    for name in ('u', 'theta', 'lnL', 'chain_theta', 'chain_lnL', 'trace', 'accepted', 'outside', 'evaluated'):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert a.margin == b.margin and np.isfinite(a.margin)
    assert not np.array_equal(a.u[0], a.u[1])                  # the pixel is in the stream
    # the cube pixel, not the position in the run: pixel 1 alone takes the steps it takes beside pixel 0
    alone = ensemble.run_twin(f, D, 1, W, u0[1:], 20, 4, 2, seed=7, pix=[1])
    assert np.array_equal(alone.u[0], a.u[1]) and np.array_equal(alone.chain_theta[0], a.chain_theta[1])
    # a run numbers its steps from 1: two runs of 10 with one seed repeat the random numbers and are not the run of 20 ...
    first = ensemble.run_twin(f, D, 2, W, u0, 10, 0, 1, seed=7)
    assert np.array_equal(first.trace, ensemble.run_twin(f, D, 2, W, u0, 20, 0, 1, seed=7).trace[:, :10])
    again = ensemble.run_twin(f, D, 2, W, None, 10, 0, 1, seed=7, state=first.state)
    assert not np.array_equal(again.u, a.u)
    # ... a continuation takes a seed of its own, and is then the run from that state with that seed
    first = ensemble.run_twin(f, D, 2, W, u0, 10, 0, 1, seed=7)
    cont = ensemble.run_twin(f, D, 2, W, None, 10, 0, 1, seed=8, state=first.state)
    fresh = ensemble.run_twin(f, D, 2, W, first.u, 10, 0, 1, seed=8)
    assert np.array_equal(cont.u, fresh.u) and np.array_equal(cont.trace, fresh.trace) and cont.evaluated.tolist() == [80, 80]


@pytest.mark.parametrize('phi', [0.5, 0.9])
def test_autocorrelation_time_of_an_ar1_series(phi):
    rng = np.random.default_rng(17)
    n = 200000
    e = rng.normal(size=n)
    x = np.empty(n)
    x[0] = e[0] / np.sqrt(1 - phi * phi)
    for i in range(1, n):
        x[i] = phi * x[i - 1] + e[i]
    truth = (1 + phi) / (1 - phi)
    assert abs(ensemble.autocorr_time(x) - truth) < 0.1 * truth
    assert np.isnan(ensemble.autocorr_time(np.ones(50)))


def test_quantile_formula():
    rng = np.random.default_rng(23)
    for N in (1, 2, 7, 96, 8192):
        s = np.sort(rng.normal(3.0, 2.0, size=N))
        for q in (0.0, 0.16, 0.5, 0.84, 0.999, 1.0):
            h = float(N - 1) * q
            i = int(np.floor(h))
            mine = s[i] + (s[min(i + 1, N - 1)] - s[i]) * (h - i)
            got = ensemble.quantile(s, q)
            assert got == mine
            ref = np.quantile(s, q)
            assert abs(got - ref) <= 2 * np.spacing(abs(ref)), (N, q, got, ref)
    # the summary's twin: best row the first of the largest, quantiles by the same formula
    theta, lnL = rng.normal(size=(2, 5, 4, 3)), rng.normal(size=(2, 5, 4))
    lnL[0, 1, 2] = lnL[0, 3, 0] = 9.0
    mean, std, best, best_lnL, quant = ensemble.summarize(theta, lnL, (0.25, 0.5))
    assert np.array_equal(best[0], theta[0, 1, 2]) and best_lnL[0] == 9.0 and quant.shape == (2, 3, 2)
    flat = theta.reshape(2, 20, 3)
    np.testing.assert_allclose(mean, flat.mean(axis=1), rtol=1e-13)
    np.testing.assert_allclose(std, flat.std(axis=1), rtol=1e-12)
    assert quant[1, 2, 1] == ensemble.quantile(np.sort(flat[1, :, 2]), 0.5)
    assert np.array_equal(ensemble.summarize(theta[:, :1, :1], lnL[:, :1, :1])[1], np.zeros((2, 3)))      # one sample: std 0


def test_log_zero():
    D, W = 2, 6
    u0 = _start(1, W, D, 31, 0.3, 0.7)
    bad_start = u0[0, 0].copy()

    def nan_at_start(pix, T):                                  # walker 0 starts where the likelihood is NaN
        out = -0.5 * (((T - 0.5) / 0.2) ** 2).sum(axis=1)
        out[(T == bad_start).all(axis=1)] = np.nan
        return out
    res = ensemble.run_twin(nan_at_start, D, 1, W, u0, 1, 0, 1, seed=3)
    # its lnL became log_zero, so its first inside proposal of finite lnL is accepted whatever r_2
    assert res.state.D == 2 and res.outside[0] == 0 and np.isfinite(res.lnL).all() and res.lnL[0, 0] > -10
    assert not np.array_equal(res.u[0, 0], bad_start)
    still = ensemble.run_twin(nan_at_start, D, 1, W, u0, 1, 0, 1, seed=3, log_zero=-123.0)
    assert np.array_equal(still.u, res.u)
    # a NaN (or infinite) proposal is rejected: with NaN everywhere but the start nothing ever moves
    def nan_elsewhere(pix, T):
        start = (T[:, None, :] == u0[0][None]).all(axis=2).any(axis=1)
        return np.where(start, 0.0, np.nan)
    res = ensemble.run_twin(nan_elsewhere, D, 1, W, u0, 25, 0, 1, seed=3)
    assert res.accepted[0] == 0 and np.array_equal(res.u, u0) and res.evaluated[0] == 25 * W
    assert np.isinf(res.margin)                                # no decision was taken on a finite lnL
    assert LOG_ZERO == -1e100
