"""The posterior moments (nfa_runner_predict_moments) are planned by csrc/nfa_moments_plan.h: how a call's rows are cut
into chunks and pieces, and the geometry of the reduction launches.  The header is plain C++17; g++ compiles it alone and
the cut and the geometry are checked here without a GPU."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
RMAX, TILE, WAVE_ROWS, WAVES_PER_CU = 16, 64, 8, 32

SHIM = r'''
#include "nfa_moments_plan.h"
extern "C" {
int consts(int i) { const int v[] = {MOM_CHUNK_ROWS, MOM_TILE, MOM_RMAX, MOM_WAVE_ROWS, MOM_WAVES_PER_CU, (int)sizeof(MomPiece)}; return v[i]; }
int chunk_refused(long long chunk_rows) { return mom_check_chunk_rows(chunk_rows) != nullptr; }
long long chunk_rows(long long c) { return mom_chunk_rows(c); }
long long n_chunks(long long rows, long long chunk) { return mom_n_chunks(rows, chunk); }
// every chunk's pieces in turn, the cursor carried: rows of out are (chunk, seg, row0, n); returns their number
long long cut_all(const long long *seg_off, long long n_seg, long long chunk, long long *out) {
    static MomPiece buf[1 << 16];
    int64_t cursor = 0;
    long long total = 0;
    const long long nc = mom_n_chunks(seg_off[n_seg], chunk);
    for (long long c = 0; c < nc; ++c) {
        const int64_t n = mom_cut((const int64_t *)seg_off, n_seg, chunk, c, &cursor, buf);
        for (int64_t k = 0; k < n; ++k, ++total) {
            out[4 * total] = c; out[4 * total + 1] = buf[k].seg; out[4 * total + 2] = buf[k].row0; out[4 * total + 3] = buf[k].n;
        }
    }
    return total;
}
void geom(long long n_pieces, long long ncol, long long max_rows, int n_cu, long long *out) {
    const MomGeom G = mom_geom(n_pieces, ncol, max_rows, n_cu);
    out[0] = G.R; out[1] = G.grid_x; out[2] = G.grid_y; out[3] = G.threads; out[4] = (long long)G.lds;
}
long long stat_blocks(long long rows, int n_spec) { return mom_stat_blocks(rows, n_spec); }
long long sizes(int which, long long n, long long ncol) {
    return which == 0 ? (long long)mom_acc_doubles(n, ncol) : which == 1 ? (long long)mom_ref_doubles(n, ncol) : (long long)mom_stat_doubles(n, (int)ncol);
}
}
'''


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('moments_plan')
    src = tmp / 'plan.cpp'
    src.write_text(SHIM)
    so = tmp / 'libmomplan.so'
    res = subprocess.run(['g++', '-std=c++17', '-Wall', '-Werror', '-O1', '-shared', '-fPIC', f'-I{ROOT / "nestfit_amd" / "csrc"}',
                          str(src), '-o', str(so)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    lib = C.CDLL(str(so))
    for name in ('chunk_rows', 'n_chunks', 'cut_all', 'stat_blocks', 'sizes'):
        getattr(lib, name).restype = C.c_longlong
    lib.chunk_refused.argtypes = lib.chunk_rows.argtypes = [C.c_longlong]
    lib.n_chunks.argtypes = [C.c_longlong, C.c_longlong]
    lib.cut_all.argtypes = [C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p]
    lib.geom.argtypes = [C.c_longlong, C.c_longlong, C.c_longlong, C.c_int, C.c_void_p]
    lib.stat_blocks.argtypes = [C.c_longlong, C.c_int]
    lib.sizes.argtypes = [C.c_int, C.c_longlong, C.c_longlong]
    assert [lib.consts(i) for i in range(6)] == [4096, TILE, RMAX, WAVE_ROWS, WAVES_PER_CU, 16]
    return lib


def _cut(lib, offsets, chunk):
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    out = np.zeros((int(off[-1]) + 1, 4), dtype=np.int64)
    n = lib.cut_all(off.ctypes.data, off.size - 1, chunk, out.ctypes.data)
    return out[:n]


def _geom(lib, n_pieces, ncol, max_rows, n_cu=256):
    out = np.zeros(5, dtype=np.int64)
    lib.geom(n_pieces, ncol, max_rows, n_cu, out.ctypes.data)
    return dict(zip(('R', 'grid_x', 'grid_y', 'threads', 'lds'), (int(v) for v in out)))


OFFSETS = (0, 1, 3, 66, 130, 195, 395, 395)          # segments of 1, 2, 63, 64, 65, 200 and 0 rows


def test_every_row_is_in_exactly_one_piece(lib):
    pieces = _cut(lib, OFFSETS, 64)
    seen = np.zeros(OFFSETS[-1], dtype=int)
    owner = np.full(OFFSETS[-1], -1)
    for c, seg, row0, n in pieces:
        assert n > 0 and 0 <= row0 and row0 + n <= 64                 # inside its chunk
        a = c * 64 + row0
        assert OFFSETS[seg] <= a and a + n <= OFFSETS[seg + 1]        # inside its segment
        seen[a:a + n] += 1
        owner[a:a + n] = seg
    assert np.all(seen == 1)
    want = np.repeat(np.arange(len(OFFSETS) - 1), np.diff(OFFSETS))
    assert np.array_equal(owner, want)
    assert 6 not in pieces[:, 1]                                      # the empty segment has no piece
    # a chunk holds at most one piece per segment (one writer per segment and column in a launch), in ascending order
    for c in np.unique(pieces[:, 0]):
        segs = pieces[pieces[:, 0] == c, 1]
        assert np.all(np.diff(segs) > 0)
    # the segment of 200 rows from row 195 straddles chunks 3 .. 6
    assert sorted(pieces[pieces[:, 1] == 5, 0]) == [3, 4, 5, 6]


def test_cut_of_other_shapes(lib):
    rng = np.random.default_rng(5)
    for chunk in (64, 128, 4096):
        sizes = rng.integers(0, 300, size=40)
        sizes[rng.uniform(size=40) < 0.2] = 0
        off = np.concatenate([[0], np.cumsum(sizes)])
        pieces = _cut(lib, off, chunk)
        seen = np.zeros(off[-1], dtype=int)
        for c, seg, row0, n in pieces:
            a = c * chunk + row0
            assert n > 0 and row0 + n <= chunk and off[seg] <= a and a + n <= off[seg + 1]
            seen[a:a + n] += 1
        assert np.all(seen == 1)
    assert _cut(lib, (0, 0, 0), 64).shape[0] == 0                     # nothing but empty segments
    assert lib.n_chunks(395, 64) == 7 and lib.n_chunks(0, 64) == 0 and lib.n_chunks(64, 64) == 1


def test_chunk_rows_is_a_multiple_of_64(lib):
    assert lib.chunk_rows(0) == 4096 and lib.chunk_rows(64) == 64
    for ok in (0, 64, 128, 4096, 1 << 20):
        assert not lib.chunk_refused(ok)
    for bad in (100, 1, 63, 65, -64, (1 << 20) + 64):
        assert lib.chunk_refused(bad)


def test_geometry_stays_inside_its_bounds(lib):
    slots = 256 * WAVES_PER_CU
    # one segment of 4096 rows x 2048 columns: 32 column tiles alone would be 32 waves; the rows go over 16 waves each
    g = _geom(lib, 1, 2048, 4096)
    assert g == {'R': 16, 'grid_x': 1, 'grid_y': 32, 'threads': 16 * 64, 'lds': 16 * 2 * 64 * 8}
    # 4096 segments of one row x 6 columns (the row statistics of three spectra): one wave per piece
    g = _geom(lib, 4096, 6, 1)
    assert g == {'R': 1, 'grid_x': 4096, 'grid_y': 1, 'threads': 64, 'lds': 2 * 64 * 8}
    for n_pieces in (1, 2, 7, 64, 1000, 4096):
        for ncol in (1, 6, 63, 64, 65, 199, 2048, 4100):
            for max_rows in (1, 7, 8, 15, 16, 64, 200, 4096):
                g = _geom(lib, n_pieces, ncol, max_rows)
                R = g['R']
                assert 1 <= R <= RMAX and R & (R - 1) == 0
                assert g['grid_x'] == n_pieces and g['grid_y'] == -(-ncol // TILE) and g['grid_y'] * TILE >= ncol
                assert g['threads'] == R * 64 <= 1024 and g['lds'] == R * 2 * TILE * 8 <= 64 * 1024
                if R > 1:
                    assert R * WAVE_ROWS <= max_rows                       # no wave for fewer than 8 rows
                    assert n_pieces * g['grid_y'] * R <= slots             # never more waves than fill the device once
                if R < RMAX:                                               # ... and as many as those two allow
                    assert 2 * R * WAVE_ROWS > max_rows or n_pieces * g['grid_y'] * 2 * R > slots
    assert _geom(lib, 1, 2048, 4096, n_cu=8)['R'] == 8                     # from the shape and the device alone
    assert lib.stat_blocks(130, 3) == 98 and lib.stat_blocks(1, 1) == 1
    assert lib.sizes(0, 7, 199) == 2 * 7 * 199 and lib.sizes(1, 7, 199) == 7 * 199 and lib.sizes(2, 64, 3) == 64 * 6
