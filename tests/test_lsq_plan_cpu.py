"""The normal equations (nfa_runner_normal_equations) are planned by csrc/nfa_lsq_plan.h: the rows of a point, the points of
a chunk, the order of the Gram entries, the geometry of the Gram launch and the sets the call refuses.  The header is
plain C++17; g++ compiles it alone and it is checked here without a GPU."""
import ctypes as C
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
MAX_DIM, TILE = 24, 128
MASK, BASELINE, CALIB, NMARG, CORR, RESP, TMPL, CONT, ROBUST = (1 << k for k in range(9))

SHIM = r'''
#include "nfa_lsq_plan.h"
extern "C" {
int consts(int i) { const int v[] = {NFA_LSQ_MAX_DIM, LSQ_CHUNK_ROWS, LSQ_TILE, LSQ_STRIDE}; return v[i]; }
int rows_per_point(int ndim) { return lsq_rows_per_point(ndim); }
long long points_per_chunk(long long chunk_rows, int ndim) { return lsq_points_per_chunk(chunk_rows, ndim); }
long long n_chunks(long long points, long long chunk_rows, int ndim) { return lsq_n_chunks(points, chunk_rows, ndim); }
int chunk_refused(long long chunk_rows, int ndim) { return lsq_check_chunk_rows(chunk_rows, ndim) != nullptr; }
int ndim_refused(int ndim) { return lsq_check_ndim(ndim) != nullptr; }
int n_pairs(int ndim) { return lsq_n_pairs(ndim); }
int pair_index(int k, int l) { return lsq_pair_index(k, l); }
int pair_k(int index) { int k, l; lsq_pair_of(index, &k, &l); return k; }
int pair_l(int index) { int k, l; lsq_pair_of(index, &k, &l); return l; }
void geom(int ndim, long long points, long long *out) {
    const LsqGeom G = lsq_geom(ndim, points);
    out[0] = G.grid; out[1] = G.threads; out[2] = G.ept; out[3] = (long long)G.lds;
}
long long probe_blocks(long long points, int ndim) { return lsq_probe_blocks(points, ndim); }
void scratch(long long B, int ndim, long long *out) {
    const LsqScratchPlan P = lsq_scratch(B, ndim);
    const size_t v[] = {P.theta, P.inv_d, P.chi2, P.grad, P.curv, P.step, P.lower, P.upper, P.total};
    for (int i = 0; i < 9; ++i) out[i] = (long long)v[i];
}
const char *refusal(unsigned has) { return lsq_refusal(has); }
}
'''


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('lsq_plan')
    src = tmp / 'plan.cpp'
    src.write_text(SHIM)
    so = tmp / 'liblsqplan.so'
    res = subprocess.run(['g++', '-std=c++17', '-Wall', '-Werror', '-O1', '-shared', '-fPIC', f'-I{ROOT / "nestfit_amd" / "csrc"}',
                          str(src), '-o', str(so)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    lib = C.CDLL(str(so))
    for name in ('points_per_chunk', 'n_chunks', 'probe_blocks'):
        getattr(lib, name).restype = C.c_longlong
    lib.points_per_chunk.argtypes = lib.chunk_refused.argtypes = [C.c_longlong, C.c_int]
    lib.n_chunks.argtypes = [C.c_longlong, C.c_longlong, C.c_int]
    lib.geom.argtypes = [C.c_int, C.c_longlong, C.c_void_p]
    lib.probe_blocks.argtypes = [C.c_longlong, C.c_int]
    lib.scratch.argtypes = [C.c_longlong, C.c_int, C.c_void_p]
    lib.refusal.argtypes = [C.c_uint]
    lib.refusal.restype = C.c_char_p
    assert [lib.consts(i) for i in range(4)] == [MAX_DIM, 4096, TILE, TILE + 1]
    return lib


def test_rows_and_points(lib):
    assert [lib.rows_per_point(n) for n in (0, 1, 6, 12, 24)] == [1, 3, 13, 25, 49]
    assert lib.points_per_chunk(64, 6) == 4 and lib.points_per_chunk(64, 12) == 2 and lib.points_per_chunk(64, 24) == 1
    assert lib.points_per_chunk(0, 12) == 4096 // 25 and lib.points_per_chunk(0, 0) == 4096 and lib.points_per_chunk(128, 0) == 128
    # a point's rows never straddle chunks: whole points only, and every point has a chunk
    for chunk in (64, 128, 4096):
        for n in (0, 1, 6, 12, 24):
            per = lib.points_per_chunk(chunk, n)
            assert per >= 1 and per * lib.rows_per_point(n) <= chunk < (per + 1) * lib.rows_per_point(n)
            for points in (1, per, per + 1, 9, 4096):
                assert lib.n_chunks(points, chunk, n) == -(-points // per)


def test_refused_chunks_and_dimensions(lib):
    for ok in (0, 64, 128, 4096, 1 << 20):
        assert not lib.chunk_refused(ok, 12)
    for bad in (63, 65, -64, 100, (1 << 20) + 64):
        assert lib.chunk_refused(bad, 6)
    assert lib.chunk_refused(64, 32)                                  # 65 rows do not fit 64
    assert not lib.chunk_refused(64, 24) and not lib.chunk_refused(128, 32)
    assert not lib.chunk_refused(64, 0)                               # chi^2 alone: one row per point
    assert not lib.ndim_refused(24) and lib.ndim_refused(25) and lib.ndim_refused(0) and not lib.ndim_refused(1)


def test_pair_index_is_a_bijection(lib):
    for n in range(MAX_DIM + 1):
        m = n + 1
        assert lib.n_pairs(n) == m * (m + 1) // 2
        seen = set()
        for l in range(m):
            for k in range(l + 1):
                i = lib.pair_index(k, l)
                assert lib.pair_index(l, k) == i                      # symmetric
                assert (lib.pair_k(i), lib.pair_l(i)) == (k, l)       # and the inverse gives k <= l back
                seen.add(i)
        assert seen == set(range(lib.n_pairs(n)))


def test_geometry_stays_inside_the_device(lib):
    out = (C.c_longlong * 4)()
    for n in range(MAX_DIM + 1):
        for points in (1, 2, 163, 4096):
            lib.geom(n, points, out)
            grid, threads, ept, lds = out[0], out[1], out[2], out[3]
            assert grid == points                                     # a workgroup per point
            assert ept == (2 if n + 1 <= 16 else 4)
            assert lib.n_pairs(n) <= threads <= 1024 and threads % 64 == 0            # a thread per Gram entry ...
            assert (n + 1) * TILE <= threads * ept < (n + 1) * TILE + 64 * ept       # ... and one per ept elements of a tile
            assert lds == 8 * 2 * (n + 1) * (TILE + 1) <= 160 * 1024
    assert (TILE + 1) % 2 == 1                                        # rows k = 0 .. 31 start in different bank pairs
    assert len({(2 * k * (TILE + 1)) % 64 for k in range(MAX_DIM + 1)}) == MAX_DIM + 1
    assert lib.probe_blocks(4, 6) == 1 and lib.probe_blocks(163, 12) == -(-163 * 25 // 256) and lib.probe_blocks(257, 0) == 2


def test_scratch_is_laid_out_without_overlap(lib):
    out = (C.c_longlong * 9)()
    for B, n in ((1, 1), (9, 12), (4096, 24)):
        lib.scratch(B, n, out)
        sizes = [B * n, B * n, B, B * n, B * n * n, n, n, n]
        assert out[0] == 0
        for i, size in enumerate(sizes):
            assert out[i + 1] == out[i] + size
        assert out[8] == sum(sizes)


def test_refusal_serves_masks_and_continua_alone(lib):
    words = {BASELINE: b'baseline', TMPL: b'templates', CALIB: b'calibration', CORR: b'correlated', RESP: b'response',
             NMARG: b'noise uncertainty', ROBUST: b'robust'}
    for has in range(512):
        why = lib.refusal(has)
        if has & ~(MASK | CONT) == 0:
            assert why is None, has
        else:
            assert why is not None and why.startswith(b'a set with ') and why.endswith(b'takes no normal equations'), has
    for bit, word in words.items():
        assert word in lib.refusal(bit) and word in lib.refusal(bit | MASK | CONT)
    assert b'response' in lib.refusal(RESP | CORR)                    # a response brings the correlated coefficients along
    assert lib.refusal(1 << 9) is not None                            # a bit this header does not know
