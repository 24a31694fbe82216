"""Tempered ensembles without a GPU: what the plan header (csrc/nfa_ensemble_plan.h, compiled alone by g++) adds
for them, the numpy twin's rungs and swaps on targets with known answers, and the evidence reduction's twin."""
import ctypes as C
import functools
import subprocess
import warnings
from pathlib import Path

import numpy as np
import pytest

from nestfit_amd import ensemble

ROOT = Path(__file__).resolve().parent.parent
LD = np.longdouble
U = 2.0 ** -53

SHIM = r'''
#include "nfa_ensemble_plan.h"
extern "C" {
unsigned long long consts(int i) {
    const unsigned long long v[] = {NFA_ENS_MAX_TEMPS, NFA_ENS_MAX_BLOCKS, ENS_RUNG_SHIFT, NFA_ENS_SWAP_TAG, ENS_SWAP_THREADS_MAX,
                                    ENS_EVID_THREADS, NFA_ENS_TAG, (unsigned long long)ENS_STEPS_MAX, NFA_ENS_MAX_WALKERS};
    return v[i];
}
const char *check_betas(const double *b, int n) { return ens_check_betas(b, n); }
const char *check_swap_every(long long n) { return ens_check_swap_every(n); }
const char *check_blocks(int B, long long n_keep) { return ens_check_blocks(B, n_keep); }
int swaps(long long s, long long every) { return ens_swaps(s, every) ? 1 : 0; }
int parity(long long sweep) { return ens_swap_parity(sweep); }
int pairs(int T, int parity) { return ens_swap_pairs(T, parity); }
unsigned long long move_tag(int t, long long s, int h) { return ens_move_tag(t, s, h); }
unsigned long long swap_tag(int t, long long s) { return ens_swap_tag(t, s); }
long long set_steps(long long n_keep, int B, int j) { return ens_set_steps(n_keep, B, j); }
long long set_first(long long n_keep, int B, int j) { return ens_set_first(n_keep, B, j); }
void bytes(long long P, int W, int T, int ndim, int D, long long n_steps, long long n_keep, long long *out) {
    const EnsBytes B = ens_tempered_bytes(P, W, T, ndim, D, n_steps, n_keep);
    out[0] = B.state; out[1] = B.chain; out[2] = B.trace; out[3] = B.total;
}
void geom(int which, long long P, int W, int T, int parity, long long *out) {
    const EnsGeom G = which == 0 ? ens_swap_geom(P, W, T, parity) : ens_evidence_geom(P, T);
    out[0] = G.grid; out[1] = G.threads; out[2] = (long long)G.lds;
}
}
'''

MAIN = r'''
#include <cmath>
#include <cstdio>
#include <vector>
int main() {
    int bad = 0;
    for (int T = 0; T <= 34; ++T) {
        std::vector<double> b((size_t)(T > 0 ? T : 1), 0.0);       // exactly T doubles: a read past them is the sanitizer's to find
        for (int t = 0; t < T; ++t) b[(size_t)t] = t == T - 1 ? 0.0 : std::pow(0.5, t);
        const char *why = check_betas(b.data(), T);
        bad += (why == nullptr) != (T >= 2 && T <= 32);
        if (T >= 2) { b[(size_t)(T - 1)] = NAN; bad += check_betas(b.data(), T) == nullptr; }
        for (int par = 0; par < 2; ++par) {
            long long g[3];
            geom(0, 3, 130, T < 2 ? 2 : T > 32 ? 32 : T, par, g);
            bad += g[1] != 192;
            geom(1, 3, 130, T < 2 ? 2 : T, par, g);
            bad += g[1] != 256;
        }
    }
    bad += check_betas(nullptr, 4) == nullptr;
    bad += move_tag(31, 1ll << 40, 1) >= swap_tag(0, 1) || swap_tag(31, 1ll << 40) >= (1ull << 62);
    for (int B = 1; B <= 16; ++B) for (int j = 0; j <= B; ++j) bad += set_first(1000, B, j) + set_steps(1000, B, j) > 1000;
    long long out[4];
    bytes(1ll << 24, 512, 32, 60, 60, 1ll << 20, 1ll << 10, out);     // (the sum stays inside 64 bits)
    bad += out[3] <= 0;
    std::printf("%d\n", bad);
    return bad;
}
'''


def _compile(tmp, name, source, *flags):
    src, out = tmp / f'{name}.cpp', tmp / name
    src.write_text(source)
    res = subprocess.run(['g++', '-std=c++17', '-Wall', '-Werror', '-O1', f'-I{ROOT / "nestfit_amd" / "csrc"}', *flags, str(src),
                          '-o', str(out)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return out


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    so = _compile(tmp_path_factory.mktemp('ens_tempered_plan'), 'libensplan.so', SHIM, '-shared', '-fPIC')
    lib = C.CDLL(str(so))
    LL, ULL = C.c_longlong, C.c_ulonglong
    for name in ('consts', 'move_tag', 'swap_tag'):
        getattr(lib, name).restype = ULL
    for name in ('set_steps', 'set_first'):
        getattr(lib, name).restype = LL
        getattr(lib, name).argtypes = [LL, C.c_int, C.c_int]
    for name in ('check_betas', 'check_swap_every', 'check_blocks'):
        getattr(lib, name).restype = C.c_char_p
    lib.check_betas.argtypes = [C.c_void_p, C.c_int]
    lib.check_swap_every.argtypes = [LL]
    lib.check_blocks.argtypes = [C.c_int, LL]
    lib.swaps.argtypes = [LL, LL]
    lib.parity.argtypes = [LL]
    lib.pairs.argtypes = [C.c_int, C.c_int]
    lib.move_tag.argtypes = [C.c_int, LL, C.c_int]
    lib.swap_tag.argtypes = [C.c_int, LL]
    lib.bytes.argtypes = [LL, C.c_int, C.c_int, C.c_int, C.c_int, LL, LL, C.c_void_p]
    lib.geom.argtypes = [C.c_int, LL, C.c_int, C.c_int, C.c_int, C.c_void_p]
    return lib


# ---- the plan header --------------------------------------------------------------------------------------------------
def test_constants_are_the_twins(lib):
    assert [lib.consts(i) for i in range(9)] == [32, 16, 48, (1 << 61) + (1 << 60), 512, 256, 1 << 61, 1 << 40, 512]
    assert (ensemble.MAX_TEMPS, ensemble.MAX_BLOCKS, ensemble.RUNG_SHIFT, ensemble.ENS_SWAP_TAG) == (32, 16, 48, (1 << 61) + (1 << 60))
    header = (ROOT / 'include' / 'nestfit_amd.h').read_text()
    assert '#define NFA_ENS_MAX_TEMPS  32' in header and '#define NFA_ENS_MAX_BLOCKS 16' in header


def _betas(*b):
    return (C.c_double * len(b))(*b)


def test_every_ladder_refusal_has_its_sentence(lib):
    assert lib.check_betas(_betas(1.0, 0.0), 2) is None and lib.check_betas(_betas(1.0, 0.5, 0.25), 3) is None
    full = ensemble.ladder(32)
    assert lib.check_betas(_betas(*full), 32) is None
    assert b'NFA_ENS_MAX_TEMPS' in lib.check_betas(_betas(1.0), 1)
    assert b'NFA_ENS_MAX_TEMPS' in lib.check_betas(_betas(*ensemble.ladder(33)), 33)
    assert b'betas[0] must be 1' in lib.check_betas(_betas(0.9, 0.5, 0.0), 3)
    assert b'decrease strictly' in lib.check_betas(_betas(1.0, 0.5, 0.5, 0.0), 4)          # a tie
    assert b'decrease strictly' in lib.check_betas(_betas(1.0, 0.5, 0.6, 0.0), 4)          # an increase
    assert b'must not be negative' in lib.check_betas(_betas(1.0, 0.5, -1e-9), 3)
    assert b'not finite' in lib.check_betas(_betas(1.0, float('nan'), 0.0), 3)
    assert b'not finite' in lib.check_betas(_betas(1.0, 0.5, float('-inf')), 3)
    assert b'not given' in lib.check_betas(None, 3)
    assert lib.check_swap_every(0) is None and lib.check_swap_every(7) is None and b'swap_every' in lib.check_swap_every(-1)
    assert lib.check_blocks(1, 1) is None and lib.check_blocks(16, 16) is None and lib.check_blocks(8, 1000) is None
    assert b'NFA_ENS_MAX_BLOCKS' in lib.check_blocks(0, 10) and b'NFA_ENS_MAX_BLOCKS' in lib.check_blocks(17, 100)
    assert b'no more blocks than kept steps' in lib.check_blocks(8, 7)
    for bad in ([1.0], [0.9, 0.0], [1.0, 0.5, 0.5], [1.0, -0.1], [1.0, np.nan, 0.0], ensemble.ladder(33)):
        with pytest.raises(ValueError):
            ensemble.check_betas(bad)


def test_tags_and_swap_parity(lib):
    top = 1 << 40
    # the largest move tag lies below the smallest swap tag, the largest swap tag below 2^62, everything at 2^61 or above
    assert lib.move_tag(31, top, 1) == (1 << 61) + (31 << 48) + 2 * top + 1 < lib.swap_tag(0, 1) == (1 << 61) + (1 << 60) + 1
    assert lib.swap_tag(31, top) == (1 << 61) + (1 << 60) + (31 << 48) + top < 1 << 62
    assert lib.move_tag(0, 1, 0) == ensemble.ENS_TAG + 2                   # rung 0 moves on the untempered tags
    assert lib.move_tag(3, top, 1) < lib.move_tag(4, 1, 0)                 # the rungs' tags do not meet
    assert lib.swap_tag(5, 9) == ensemble.ENS_SWAP_TAG + (5 << ensemble.RUNG_SHIFT) + 9
    assert [lib.swaps(s, 3) for s in range(1, 8)] == [0, 0, 1, 0, 0, 1, 0] and not any(lib.swaps(s, 0) for s in range(1, 8))
    assert [lib.parity(n) for n in range(5)] == [0, 1, 0, 1, 0] == [ensemble.swap_parity(n) for n in range(5)]
    for T in range(2, 33):
        for parity in (0, 1):
            assert lib.pairs(T, parity) == len(range(parity, T - 1, 2))
    assert lib.pairs(2, 0) == 1 and lib.pairs(2, 1) == 0                   # one pair, active on the even sweeps only


def test_byte_counts(lib):
    out = (C.c_longlong * 4)()
    for P, W, T, ndim, D, n_steps, n_keep in ((1, 16, 2, 6, 6, 30, 6), (64, 64, 16, 12, 10, 2000, 128), (3, 512, 32, 60, 60, 10, 10)):
        lib.bytes(P, W, T, ndim, D, n_steps, n_keep, out)
        state, chain, trace, total = out[0], out[1], out[2], out[3]
        units = P * T
        walkers, rows = units * W, units * W // 2
        assert chain == 8 * P * n_keep * W * (ndim + 1) + 8 * units * n_keep * W      # the cold chain, and lnL of every rung
        assert trace == 8 * units * n_steps * (D + 1)
        assert state == (8 * walkers * (D + ndim + 1) + 4 * walkers + 8 * rows * (ndim + D + 1) + 8 * rows + 8 * 3 * units + 4 * units
                         + 4 * D + 8 * P * (2 * ndim + ndim + 1 + 8 * ndim) + 64 + 8 * T + 16 * P * (T - 1) + 8 * units * 17 * 3)
        assert total == state + chain + trace
        lib.bytes(2 * P, W, T, ndim, D, n_steps, n_keep, out)
        assert out[3] <= 2 * total                                # a group of n pixels fits n times the bytes of one


def test_geometry(lib):
    out = (C.c_longlong * 3)()
    for W, threads in ((2, 64), (16, 64), (64, 64), (66, 128), (130, 192), (512, 512)):
        for T, parity, pairs in ((2, 0, 1), (2, 1, 0), (3, 0, 1), (3, 1, 1), (5, 0, 2), (5, 1, 2), (16, 0, 8), (16, 1, 7)):
            lib.geom(0, 7, W, T, parity, out)
            assert (out[0], out[1], out[2]) == (7 * pairs, threads, 0) and W <= threads <= 512
    lib.geom(1, 5, 16, 7, 0, out)
    assert (out[0], out[1], out[2]) == (35, 256, 0)
    for n_keep, B in ((1000, 8), (7, 3), (16, 16), (5, 1)):
        blk = n_keep // B
        assert (lib.set_first(n_keep, B, 0), lib.set_steps(n_keep, B, 0)) == (0, n_keep)
        assert [(lib.set_first(n_keep, B, j), lib.set_steps(n_keep, B, j)) for j in range(1, B + 1)] == [((j - 1) * blk, blk) for j in range(1, B + 1)]


def test_checks_and_geometries_under_the_sanitizers(tmp_path):
    """Host code only: the new checks and geometries in a program of their own, built with -fsanitize=address,undefined."""
    exe = _compile(tmp_path, 'plan_main', SHIM + MAIN, '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-g')
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.strip() == '0', (res.stdout, res.stderr)
    assert 'runtime error' not in res.stderr and 'AddressSanitizer' not in res.stderr


# ---- the twin ---------------------------------------------------------------------------------------------------------
COLD = ('u', 'theta', 'lnL', 'chain_theta', 'chain_lnL', 'trace', 'accepted', 'outside', 'evaluated')
RUNGS = ('rung_u', 'rung_theta', 'rung_lnL_state', 'rung_lnL', 'rung_trace', 'rung_accepted', 'rung_outside', 'rung_evaluated',
         'swaps_accepted', 'swaps_proposed')


def _quad(pix, T):
    return -0.5 * (((T - 0.4) / 0.1) ** 2).sum(axis=1)


def test_rung_0_of_a_run_without_swaps_is_the_untempered_run():
    D, W = 3, 8
    u0 = np.random.default_rng(1).uniform(size=(2, W, D))
    cold = ensemble.run_twin(_quad, D, 2, W, u0, 20, 4, 2, seed=7, pix=[3, 1])
    hot = ensemble.run_twin(_quad, D, 2, W, u0, 20, 4, 2, seed=7, pix=[3, 1], betas=[1.0, 0.3, 0.0], swap_every=0)
    for name in COLD:
        assert np.array_equal(getattr(cold, name), getattr(hot, name)), name
    assert hot.margin <= cold.margin and np.isinf(hot.swap_margin) and not hot.swaps_proposed.any()
    assert hot.rung_lnL.shape == (2, 3, 8, W) and hot.rung_trace.shape == (2, 3, 20, D + 1) and hot.rung_u.shape == (2, 3, W, D)
    assert hot.rung_evaluated.tolist() == [[20 * W] * 3] * 2
    # the rungs start alike and part: each has a stream of its own
    assert not np.array_equal(hot.rung_u[:, 0], hot.rung_u[:, 1]) and not np.array_equal(hot.rung_u[:, 1], hot.rung_u[:, 2])
    # with swaps the cold chain is another one, and every sweep proposes W swaps per active pair: 20 sweeps, 10 of each parity
    swapped = ensemble.run_twin(_quad, D, 2, W, u0, 20, 4, 2, seed=7, pix=[3, 1], betas=[1.0, 0.3, 0.0], swap_every=1)
    assert not np.array_equal(swapped.chain_theta, cold.chain_theta) and np.isfinite(swapped.swap_margin)
    assert swapped.swaps_proposed.tolist() == [[10 * W, 10 * W]] * 2 and (swapped.swaps_accepted > 0).all()
    two = ensemble.run_twin(_quad, D, 2, W, u0, 20, 4, 2, seed=7, pix=[3, 1], betas=[1.0, 0.0], swap_every=3)
    assert two.swaps_proposed.tolist() == [[3 * W]] * 2           # sweeps at steps 3 .. 18: six, the pair active on the even ones


def test_same_arguments_same_bits_and_how_a_run_continues():
    D, W, betas = 3, 8, ensemble.ladder(4, 1e-2)
    u0 = np.random.default_rng(2).uniform(size=(2, W, D))
    kw = dict(betas=betas, swap_every=2)
    a = ensemble.run_twin(_quad, D, 2, W, u0, 20, 4, 2, seed=7, **kw)
    b = ensemble.run_twin(_quad, D, 2, W, u0, 20, 4, 2, seed=7, **kw)
    for name in COLD + RUNGS:
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert a.margin == b.margin and a.swap_margin == b.swap_margin
    # u0[P, W, D] went to every rung; the same start spelt out per rung is the same run
    c = ensemble.run_twin(_quad, D, 2, W, np.repeat(u0[:, None], 4, axis=1), 20, 4, 2, seed=7, **kw)
    assert np.array_equal(c.rung_u, a.rung_u)
    # a continuation from the rung state with another seed is the run from that state, and is not the second half of one long run
    first = ensemble.run_twin(_quad, D, 2, W, u0, 10, 0, 1, seed=7, **kw)
    cont = ensemble.run_twin(_quad, D, 2, W, None, 10, 0, 1, seed=8, state=first.state)
    fresh = ensemble.run_twin(_quad, D, 2, W, first.rung_u, 10, 0, 1, seed=8, **kw)
    again = ensemble.run_twin(_quad, D, 2, W, first.rung_u, 10, 0, 1, seed=8, **kw)
    long = ensemble.run_twin(_quad, D, 2, W, u0, 20, 0, 1, seed=7, **kw)
    for name in COLD + RUNGS:
        assert np.array_equal(getattr(cont, name), getattr(fresh, name)), name
        assert np.array_equal(getattr(again, name), getattr(fresh, name)), name
    assert not np.array_equal(cont.rung_u, long.rung_u) and np.array_equal(first.rung_trace, long.rung_trace[:, :, :10])


# ---- evidence and modes: one twin run per seed, pixel 0 the Gaussian, pixel 1 the two modes ---------------------------
SIGMA, CENTRE = 0.02, np.array([0.4, 0.5, 0.6])
LNZ_EXACT = 1.5 * np.log(2 * np.pi) + 3 * np.log(SIGMA)        # -8.979: the unit cube cuts the Gaussian 20 sigma out
W_T, N_STEPS, N_BURN = 16, 1500, 500
LNZ_BOUND = 0.2


def _targets(pix, T):
    g = -0.5 * (((T - CENTRE) / SIGMA) ** 2).sum(axis=1)
    two = np.logaddexp(-0.5 * (((T - 0.2) / SIGMA) ** 2).sum(axis=1), -0.5 * (((T - 0.8) / SIGMA) ** 2).sum(axis=1))
    return np.where(pix == 0, g, two)


def _starts(seed):
    rng = np.random.default_rng(100 + seed)
    return np.stack([CENTRE + rng.uniform(-0.05, 0.05, (W_T, 3)), 0.2 + rng.uniform(-0.01, 0.01, (W_T, 3))])


@functools.lru_cache(maxsize=None)
def _tempered(seed):
    return ensemble.run_twin(_targets, 3, 2, W_T, _starts(seed), N_STEPS, N_BURN, 1, seed=seed, betas=ensemble.ladder(16, 1e-4))


@pytest.mark.parametrize('seed', [1, 2, 3, 4, 5])
def test_evidence_of_a_gaussian(seed):
    """The stepping-stone lnZ of the twin against the exact one.  Observed, seeds 1 .. 5: lnZ - exact = +0.036, -0.019, -0.068,
    -0.013, -0.014; lnZ_err 0.037 .. 0.050; lnZ_ti - exact -0.48 .. -0.57; swap rates 0.59 .. 0.99.  The bound is
    three times the worst observed, 0.068, and inside the 0.25 the nested sampler's error bar has."""
    res = _tempered(seed)
    ev = ensemble.evidence_of(res.rung_lnL[:1], ensemble.ladder(16, 1e-4), 8)
    print(f'seed {seed}: lnZ - exact {ev.lnZ[0] - LNZ_EXACT:+.4f}, lnZ_err {ev.lnZ_err[0]:.4f}, lnZ_ti - exact {ev.lnZ_ti[0] - LNZ_EXACT:+.4f}, '
          f'swap rates {np.round((res.swaps_accepted / res.swaps_proposed)[0], 2)}')
    assert abs(ev.lnZ[0] - LNZ_EXACT) <= LNZ_BOUND
    assert 0 < ev.lnZ_err[0] < 0.25
    assert ev.lnZ_ti[0] - LNZ_EXACT < -0.2                     # the trapezoid over these rungs is a diagnostic, not the product
    assert ev.mean_lnL.shape == (1, 16) and np.all(np.diff(ev.mean_lnL[0]) < 0)       # hotter rungs sit lower


@pytest.mark.parametrize('seed', [1, 2, 3, 4, 5])
def test_swaps_carry_the_cold_chain_across_the_modes(seed):
    res = _tempered(seed)
    share = float((res.chain_theta[1, :, :, 0] > 0.5).mean())
    print(f'seed {seed}: {share:.3f} of the kept cold samples in the second mode')
    assert 0.25 <= share <= 0.75
    cold = ensemble.run_twin(_targets, 3, 2, W_T, _starts(seed), N_STEPS, N_BURN, 1, seed=seed)
    assert float((cold.chain_theta[1, :, :, 0] > 0.5).mean()) == 0.0


# ---- evidence_of ------------------------------------------------------------------------------------------------------
def test_evidence_of_against_longdouble():
    rng = np.random.default_rng(3)
    P, T, n_keep, W = 2, 5, 70, 16
    betas = ensemble.ladder(T, 1e-3)
    x = -50.0 + 30.0 * rng.standard_normal((P, T, n_keep, W)) * betas[None, :, None, None] - 1e3 * (1 - betas)[None, :, None, None]
    for B in (1, 8, 16, 3):
        got, ref = ensemble.evidence_sets(x, betas, B), ensemble.evidence_sets(x, betas, B, dtype=LD)
        assert got.shape == (P, T, B + 1, 3) and got.dtype == np.float64 and ref.dtype == LD
        blk = n_keep // B
        for j in range(B + 1):
            first, steps = (0, n_keep) if j == 0 else ((j - 1) * blk, blk)
            v = x[:, :, first:first + steps].reshape(P, T, -1).astype(LD)
            n = v.shape[2]
            d = np.abs(v - v[:, :, :1]).max(axis=2)
            assert np.all(np.abs(got[:, :, j, 0] - ref[:, :, j, 0]) <= 8 * n * U * d + U * np.abs(ref[:, :, j, 0]))
            assert np.all(np.abs(got[:, :, j, 1] - ref[:, :, j, 1]) <= 8 * n * U * d * d)
            assert np.all(np.abs(got[:, :, j, 2] - ref[:, :, j, 2]) <= 8 * n * U + 2 * U * np.abs(ref[:, :, j, 2]))
            # the block sets drop the remainder of n_keep / B: set j is that of the block alone
            if j > 0:
                alone = ensemble.evidence_sets(x[:, :, first:first + steps], betas, 1)
                assert np.array_equal(alone[:, :, 0], got[:, :, j])
        assert (got[:, 0, :, 2] == 0).all()
    ev = ensemble.evidence_of(x, betas, 3)                      # 70 = 3 x 23 + 1: the last kept step is in set 0 only
    assert np.array_equal(ev.sets[:, :, 3], ensemble.evidence_sets(x[:, :, 46:69], betas, 1)[:, :, 0])
    assert np.array_equal(ev.lnZ, ev.sets[:, :, 0, 2].sum(axis=1))
    blocks = ev.sets[:, :, 1:, 2].sum(axis=1)
    assert np.allclose(ev.lnZ_err, blocks.std(axis=1, ddof=1) / np.sqrt(3), rtol=1e-14)
    assert np.allclose(ev.lnZ_ti, [float(sum(LD(0.5) * (LD(ev.mean_lnL[p, t]) + LD(ev.mean_lnL[p, t + 1])) * (LD(betas[t]) - LD(betas[t + 1])) for t in range(T - 1)))
                                    for p in range(P)], rtol=1e-12)
    with pytest.raises(ValueError):
        ensemble.evidence_sets(x, betas, 71)
    with pytest.raises(ValueError):
        ensemble.evidence_sets(x, betas, 17)
    # a constant likelihood: Z = exp(c) exactly, whatever the ladder
    flat = ensemble.evidence_of(np.full((1, 4, 10, 8), -3.0), ensemble.ladder(4), 2)
    assert abs(flat.lnZ[0] + 3.0) < 1e-14 and flat.lnZ_err[0] < 1e-14 and (flat.sets[..., 1] == 0).all()


def test_a_ladder_that_does_not_end_at_0_gives_no_evidence():
    x = np.random.default_rng(4).normal(-5.0, 1.0, (1, 3, 10, 8))
    with pytest.warns(RuntimeWarning, match='does not end at beta = 0'):
        ev = ensemble.evidence_of(x, [1.0, 0.5, 0.25], 2)
    assert np.isnan(ev.lnZ).all() and np.isfinite(ev.lnZ_ti).all() and np.isfinite(ev.mean_lnL).all()
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert np.isfinite(ensemble.evidence_of(x, [1.0, 0.5, 0.0], 2).lnZ).all()
    assert ensemble.ladder(16)[0] == 1.0 and ensemble.ladder(16)[-1] == 0.0 and ensemble.ladder(16)[-2] == 1e-4
    assert np.allclose(ensemble.ladder(4, 1e-3), [1.0, 10 ** -1.5, 1e-3, 0.0], rtol=1e-14)


# ---- the rule of compare_ncomp ----------------------------------------------------------------------------------------
def test_the_component_count_follows_the_fitters_rule():
    nan = np.nan
    #                null   N = 1   N = 2   N = 3
    lnZ = np.array([[-100., -100., -100., -100., -100., nan],
                    [-80.0, -89.0, -95.0, -89.0, nan, -50.],
                    [-60.0, -70.0, -60.0, -78.0, -10., -20.],
                    [-49.0, -40.0, -10.0, -67.0, 0.0, 0.0]])
    # gains: (20, 20, 11) -> 3; (11, 19, 30) -> 3; (5, ..) stops at 0 though N = 2 would gain 35; (11, 11, 11) -> 3; NaN stops
    assert ensemble.nbest_of(lnZ, 11).tolist() == [3, 3, 0, 3, 0, 0]
    assert ensemble.nbest_of(lnZ, 20).tolist() == [2, 0, 0, 0, 0, 0]
    assert ensemble.nbest_of(lnZ[:2], 11).tolist() == [1, 1, 0, 1, 0, 0]
    maps = ensemble.nbest_of(lnZ.reshape(4, 2, 3), 11)
    assert maps.shape == (2, 3) and maps.dtype == np.int64 and maps.tolist() == [[3, 3, 0], [3, 0, 0]]
