"""The products of an ensemble chain without a GPU: the plan header's part for them (csrc/nfa_ensemble_plan.h,
compiled alone by g++) and the numpy twins `pdf_counts`, `covariance_of` and `bin_edges` of nestfit_amd/ensemble.py."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from nestfit_amd import ensemble

ROOT = Path(__file__).resolve().parent.parent

SHIM = r'''
#include "nfa_ensemble_plan.h"
extern "C" {
long long consts(int i) {
    const long long v[] = {NFA_ENS_MAX_BINS, ENS_SLAB_BYTES, ENS_SAMPLES_MAX};
    return v[i];
}
const char *check_edges(const double *edges, int ndim, int n_bins, long long n) { return ens_check_edges(edges, ndim, n_bins, n); }
void geom(int which, long long P, int ndim, long long n, int n_bins, long long *out) {
    const EnsGeom G = which == 0 ? ens_hist_geom(P, ndim, n, n_bins) : ens_cov_geom(P, n);
    out[0] = G.grid; out[1] = G.threads; out[2] = (long long)G.lds;
}
long long hist_lds(int n_bins) { return (long long)ens_hist_lds(n_bins); }
long long slab_pixels(long long bytes) { return ens_slab_pixels(bytes); }
long long hist_pixel_bytes(int ndim, int n_bins) { return ens_hist_pixel_bytes(ndim, n_bins); }
long long cov_pixel_bytes(int ndim) { return ens_cov_pixel_bytes(ndim); }
long long moments_bytes(long long P, long long chan_tot, int n_spec) { return ens_moments_bytes(P, chan_tot, n_spec); }
}
'''


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('ens_products_plan')
    src = tmp / 'plan.cpp'
    src.write_text(SHIM)
    so = tmp / 'libensproducts.so'
    res = subprocess.run(['g++', '-std=c++17', '-Wall', '-Werror', '-O1', '-shared', '-fPIC', f'-I{ROOT / "nestfit_amd" / "csrc"}',
                          str(src), '-o', str(so)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    lib = C.CDLL(str(so))
    LL = C.c_longlong
    for name in ('consts', 'hist_lds', 'slab_pixels', 'hist_pixel_bytes', 'cov_pixel_bytes', 'moments_bytes'):
        getattr(lib, name).restype = LL
    lib.check_edges.restype = C.c_char_p
    lib.check_edges.argtypes = [C.c_void_p, C.c_int, C.c_int, LL]
    lib.geom.argtypes = [C.c_int, LL, C.c_int, LL, C.c_int, C.c_void_p]
    lib.slab_pixels.argtypes = [LL]
    lib.moments_bytes.argtypes = [LL, LL, C.c_int]
    return lib


def _check(lib, edges, n_bins, n=100):
    edges = np.ascontiguousarray(edges, dtype=np.float64)
    return lib.check_edges(edges.ctypes.data, edges.shape[0], n_bins, n)


# ---- the plan header --------------------------------------------------------------------------------------------------
def test_constants_are_the_twins(lib):
    assert [lib.consts(i) for i in range(3)] == [1024, 8 << 20, 1 << 32]
    assert ensemble.MAX_BINS == lib.consts(0)
    header = (ROOT / 'include' / 'nestfit_amd.h').read_text()
    assert '#define NFA_ENS_MAX_BINS 1024' in header


def test_every_refusal_of_the_edges_has_its_sentence(lib):
    good = np.stack([np.linspace(0.0, 1.0, 8), np.linspace(-3.0, 5.0, 8)])
    assert _check(lib, good, 7) is None
    assert _check(lib, np.array([[0.0, 1.0]]), 1) is None
    assert _check(lib, np.stack([np.linspace(0, 1, 1025)] * 2), 1024) is None
    assert b'NFA_ENS_MAX_BINS' in _check(lib, good, 0)
    assert b'NFA_ENS_MAX_BINS' in _check(lib, np.stack([np.linspace(0, 1, 1026)] * 2), 1025)
    assert b'not given' in lib.check_edges(None, 2, 7, 100)
    for value, word in ((good[1, 2], b'increase strictly'), (good[1, 1], b'increase strictly'), (np.nan, b'not finite'),
                        (np.inf, b'not finite'), (-np.inf, b'not finite')):
        bad = good.copy()
        bad[1, 3] = value                                      # an edge repeated, a decreasing one, NaN, +-inf: in the second column
        assert word in _check(lib, bad, 7), value
    bad = good.copy()
    bad[0, 7] = np.inf                                         # ... and in the last edge of the first
    assert b'not finite' in _check(lib, bad, 7)
    assert _check(lib, good, 7, (1 << 32) - 1) is None and b'2^32' in _check(lib, good, 7, 1 << 32)


def test_geometry_and_lds(lib):
    out = (C.c_longlong * 3)()
    for n_bins in (1, 7, 1024):
        assert lib.hist_lds(n_bins) == 12 * (n_bins + 1)       # f64 edges and 32-bit counters, one more of each than bins
        for P, ndim, n, threads in ((3, 6, 48, 64), (2, 6, 1120, 256), (2, 12, 192, 192), (1, 1, 1, 64), (5, 60, 8192, 256)):
            lib.geom(0, P, ndim, n, n_bins, out)
            assert list(out) == [P * ndim, threads, 12 * (n_bins + 1)]
            lib.geom(1, P, ndim, n, n_bins, out)
            assert list(out) == [P, threads, 0]
    assert lib.hist_lds(1024) <= 8 * 1024 + 4 * 1024 + 12      # the issue's 8 KB + 4 KB at the cap, and the outside counter
    # the pixels of a call go through a fixed scratch: whole pixels, one at least
    assert lib.hist_pixel_bytes(12, 1024) == 12 * 1025 * 8 and lib.cov_pixel_bytes(12) == 12 * 12 * 8
    assert lib.slab_pixels(lib.hist_pixel_bytes(12, 1024)) == (8 << 20) // (12 * 1025 * 8)
    assert lib.slab_pixels(8) == 1 << 20 and lib.slab_pixels(8 << 20) == 1 and lib.slab_pixels(1 << 30) == 1
    # what the moments hold per pixel in the runner's scratch: reference rows, two planes of accumulators, S0
    assert lib.moments_bytes(1, 2048, 2) == 8 * (3 * (2048 + 4) + 1) and lib.moments_bytes(7, 192, 2) == 7 * lib.moments_bytes(1, 192, 2)


# ---- the twins --------------------------------------------------------------------------------------------------------
def _loop_counts(x, edges):
    """Bins and outside of the samples x on the edges, sample by sample."""
    n_bins = len(edges) - 1
    counts, outside = [0] * n_bins, 0
    for v in x:
        if not (edges[0] <= v <= edges[-1]):                   # a NaN too
            outside += 1
            continue
        b = n_bins - 1
        for k in range(n_bins):
            if edges[k] <= v < edges[k + 1]:
                b = k
        counts[b] += 1
    return counts, outside


def test_pdf_counts_against_a_plain_loop():
    rng = np.random.default_rng(3)
    P, n_keep, W, ndim = 2, 3, 8, 3
    chain = rng.normal(size=(P, n_keep, W, ndim))
    edges = np.stack([np.linspace(-1.0, 1.0, 6), np.array([-2.0, -0.5, -0.25, 0.0, 0.7, 3.0]), np.linspace(-4.0, 4.0, 6)])
    chain[0, 0, 0, 0], chain[0, 0, 1, 0], chain[0, 0, 2, 0] = edges[0, 0], edges[0, 2], edges[0, 5]      # on the first, an inner, the last edge
    chain[1, 2, 7, 1], chain[1, 1, 1, 1], chain[1, 0, 0, 1] = edges[1, 0], edges[1, 3], edges[1, 5]
    chain[0, 1, 1, 2] = np.nan
    counts, outside = ensemble.pdf_counts(chain, edges)
    assert counts.shape == (P, ndim, 5) and counts.dtype == np.int64 and outside.shape == (P, ndim)
    N = n_keep * W
    for p in range(P):
        for c in range(ndim):
            ref_counts, ref_out = _loop_counts(chain[p, :, :, c].ravel(), edges[c])
            assert counts[p, c].tolist() == ref_counts and outside[p, c] == ref_out
            # numpy's own rule: searchsorted from the right, less one, the last edge folded into the last bin
            x = chain[p, :, :, c].ravel()
            ok = (x >= edges[c, 0]) & (x <= edges[c, -1])
            b = np.minimum(np.searchsorted(edges[c], x[ok], 'right') - 1, 4)
            assert np.array_equal(np.bincount(b, minlength=5), counts[p, c])
    assert np.array_equal(counts.sum(axis=2) + outside, np.full((P, ndim), N))
    assert outside[0, 2] >= 1 and outside[:, 0].min() > 0      # the NaN; a normal sample beyond +-1
    with pytest.raises(ValueError):
        ensemble.pdf_counts(chain, edges[:2])


def test_covariance_of_against_numpy():
    rng = np.random.default_rng(5)
    P, n_keep, W, ndim = 3, 5, 16, 4
    A = rng.normal(size=(ndim, ndim))
    chain = rng.normal(size=(P, n_keep, W, ndim)) @ A + np.array([3.0, -1.0, 0.5, 10.0])
    chain[..., 2] = 0.75                                       # a constant column
    lnL = rng.normal(size=(P, n_keep, W))
    lnL[1, 2, 3] = lnL[1, 4, 1] = 9.0                          # a tie: the first in (keep, walker) order is the reference row
    cov = ensemble.covariance_of(chain, lnL)
    assert cov.shape == (P, ndim, ndim) and cov.dtype == np.float64
    for p in range(P):
        ref = np.cov(chain[p].reshape(-1, ndim), rowvar=False, bias=True)
        live = [0, 1, 3]
        np.testing.assert_allclose(cov[p][np.ix_(live, live)], ref[np.ix_(live, live)], rtol=1e-12, atol=0)
    assert (cov[:, 2, :] == 0).all() and (cov[:, :, 2] == 0).all()
    assert np.array_equal(cov, np.swapaxes(cov, 1, 2))
    assert (cov[:, np.arange(ndim), np.arange(ndim)] >= 0).all()
    wide = ensemble.covariance_of(chain, lnL, np.longdouble)
    assert wide.dtype == np.longdouble
    np.testing.assert_allclose(cov, wide.astype(np.float64), rtol=1e-12, atol=1e-15)
    # a covariance does not depend on the row it is taken about, up to rounding: the tie's other row gives the same
    lnL2 = lnL.copy()
    lnL2[1, 2, 3] = 8.0
    np.testing.assert_allclose(ensemble.covariance_of(chain, lnL2)[1], cov[1], rtol=1e-11, atol=1e-14)


class _BoxPriors:
    """Two parameters per component, laid out parameter-major as a theta row is: (a1, a2, b1, b2) for ncomp = 2."""
    n_param = 2

    def transform(self, u, ncomp):
        for k in range(ncomp):
            u[k] = -10.0 + 20.0 * u[k] + k                     # a_k in [-10 + k, 10 + k]
            u[ncomp + k] = 2.5                                 # b_k: a constant


def test_bin_edges_follow_the_theta_layout():
    from nestfit_amd import lsq
    edges = ensemble.bin_edges(_BoxPriors(), 2, 7)
    lower, upper = lsq.prior_box(_BoxPriors(), 2)
    assert edges.shape == (4, 8) and edges.flags.c_contiguous
    assert np.array_equal(edges[:2], np.linspace(lower[:2], upper[:2], 8, axis=1))
    assert -10.0 <= edges[0, 0] < -9.9 and 10.9 < edges[1, -1] <= 11.0      # column 1 is the second component's a
    assert np.array_equal(edges[2], np.linspace(2.0, 3.0, 8)) and np.array_equal(edges[3], edges[2])     # a point: width 1 around it
    assert (np.diff(edges, axis=1) > 0).all()
