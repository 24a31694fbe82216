// nfa_moments_plan.h -- the weighted posterior moments of model spectra (nfa_runner_predict_moments), planned on the host:
// how the rows of a call are cut into chunks and pieces, the geometry of the reduction launches, the scratch sizes.
//
// Standard C++17 without a HIP include: a host compiler builds this header alone, so the cut and the geometry can be
// tested on a machine without a GPU (tests/test_moments_plan_cpu.py).  Arithmetic only: no lock, no allocation, no call
// into the runtime.  Errors travel as `const char *`, in the words the engine fails with.
//
// A call describes n_seg segments: segment g is the rows seg_off[g] .. seg_off[g + 1] - 1.  The rows are predicted chunk
// by chunk (chunk c: rows c * chunk_rows .. ), and a chunk's spectra are reduced before the next chunk overwrites them.
// A piece is the part of one segment inside one chunk: a segment has one piece per chunk it touches, a chunk at most one
// piece per segment -- so a reduction launch over a chunk's pieces has one writer per (segment, column).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

#define MOM_CHUNK_ROWS   4096           // rows per chunk where the caller says 0
#define MOM_CHUNK_MAX    (1 << 20)      // ... and the most a caller may ask for (a piece's rows are 32-bit)
#define MOM_TILE         64             // columns of a wave: lane = column, a row is read as 512 contiguous bytes
#define MOM_RMAX         16             // waves of a workgroup at most: the rows of a piece are split over them
#define MOM_WAVE_ROWS    8              // a wave is not added for fewer rows than this
#define MOM_STAT_WAVES   4              // waves per workgroup of the row-statistics kernel, one per (row, spectrum)
#define MOM_WAVES_PER_CU 32             // wave slots of a compute unit as the plan counts them

// rows [row0, row0 + n) of the chunk (counted from the chunk's first row) belong to segment seg
struct MomPiece { int32_t seg, row0, n, pad_; };

// the caller's chunk_rows: null, or why it is refused
inline const char *mom_check_chunk_rows(int64_t chunk_rows) {
    if (chunk_rows < 0 || chunk_rows % 64 != 0) return "chunk_rows must be 0 (4096) or a multiple of 64";
    if (chunk_rows > MOM_CHUNK_MAX) return "chunk_rows must be 1048576 at most";
    return nullptr;
}
inline int64_t mom_chunk_rows(int64_t chunk_rows) { return chunk_rows == 0 ? MOM_CHUNK_ROWS : chunk_rows; }
inline int64_t mom_n_chunks(int64_t rows, int64_t chunk_rows) { return (rows + chunk_rows - 1) / chunk_rows; }

// The pieces of chunk c, in the segments' order, into out[] (room for min(chunk_rows, n_seg) of them); returns their
// number.  *cursor: the first segment that can still reach into this chunk -- 0 before chunk 0, carried from chunk to
// chunk by a caller who takes the chunks in ascending order (so the whole cut is one walk over seg_off).  Empty segments
// yield nothing.  seg_off is non-decreasing with seg_off[0] = 0 (the caller has checked).
inline int64_t mom_cut(const int64_t *seg_off, int64_t n_seg, int64_t chunk_rows, int64_t c, int64_t *cursor, MomPiece *out) {
    const int64_t a = c * chunk_rows, b = std::min(a + chunk_rows, seg_off[n_seg]);
    int64_t g = *cursor, n = 0;
    while (g < n_seg && seg_off[g + 1] <= a) ++g;             // segments that ended before this chunk, empty ones too
    while (g < n_seg && seg_off[g] < b) {
        const int64_t lo = std::max(seg_off[g], a), hi = std::min(seg_off[g + 1], b);
        if (hi > lo) out[n++] = MomPiece{(int32_t)g, (int32_t)(lo - a), (int32_t)(hi - lo), 0};
        if (seg_off[g + 1] > b) break;                        // goes on in the next chunk
        ++g;
    }
    *cursor = g;
    return n;
}

// One accumulate launch: workgroup (x = piece, y = column tile) of R waves; wave r takes the piece's rows r, r + R, ...
// and the R partial sums meet through LDS in the order r = 0 .. R - 1.  R is a power of two from the shape alone: as
// many waves as fill the device's wave slots once (pieces x tiles x R), never more than MOM_RMAX and never so many that
// a wave of the longest piece gets fewer than MOM_WAVE_ROWS rows.
struct MomGeom { int R; unsigned grid_x, grid_y, threads; size_t lds; };
inline MomGeom mom_geom(int64_t n_pieces, int64_t ncol, int64_t max_piece_rows, int n_cu) {
    const int64_t tiles = (ncol + MOM_TILE - 1) / MOM_TILE;
    const int64_t slots = (int64_t)std::max(n_cu, 1) * MOM_WAVES_PER_CU, units = std::max<int64_t>(n_pieces * tiles, 1);
    int R = 1;
    while (R < MOM_RMAX && units * (2 * R) <= slots && (int64_t)(2 * R) * MOM_WAVE_ROWS <= max_piece_rows) R *= 2;
    return MomGeom{R, (unsigned)n_pieces, (unsigned)tiles, (unsigned)(R * MOM_TILE), sizeof(double) * 2 * R * MOM_TILE};
}
// workgroups of the row-statistics launch over `rows` rows of n_spec spectra
inline int64_t mom_stat_blocks(int64_t rows, int n_spec) { return (rows * n_spec + MOM_STAT_WAVES - 1) / MOM_STAT_WAVES; }

// Scratch (doubles).  The accumulators of a matrix of ncol columns are two planes [2][n_seg][ncol], S1 then S2; the
// finish kernel turns them into mean and std in place, so each plane goes back to the host as one contiguous copy.
inline size_t mom_acc_doubles(int64_t n_seg, int64_t ncol) { return (size_t)2 * (size_t)n_seg * (size_t)ncol; }
inline size_t mom_ref_doubles(int64_t n_seg, int64_t ncol) { return (size_t)n_seg * (size_t)ncol; }
inline size_t mom_stat_doubles(int64_t chunk_rows, int n_spec) { return (size_t)chunk_rows * 2 * (size_t)n_spec; }
