// nfa_lsq_plan.h -- the normal equations of a least-squares fit (nfa_runner_normal_equations), planned on the host: the
// rows a point takes, how the points of a call are cut into chunks, the order of the Gram entries, the geometry and LDS
// of the Gram launch, the scratch sizes, and which sets the call refuses.
//
// Standard C++17 without a HIP include, like nfa_moments_plan.h: a host compiler builds this header alone, and
// tests/test_lsq_plan_cpu.py checks it without a GPU.  Arithmetic only.  Errors travel as `const char *`, in the words
// the engine fails with.
//
// A point is one (pixel, theta).  With gradients it takes R = 1 + 2 ndim rows of a predict launch: the base row, then
// theta+ and theta- of parameter 0, then of 1 .. ndim - 1; for chi^2 alone it takes the base row (the plan is then asked
// with ndim = 0 probed parameters).  A chunk of chunk_rows rows holds floor(chunk_rows / R) whole points: a point's rows
// never straddle chunks.  The Gram matrix of a point is [J r]^T W [J r] over the ndim + 1 columns J_0 .. J_(ndim-1), r:
// symmetric, so (ndim + 1)(ndim + 2) / 2 entries (k <= l), one per thread of the point's workgroup.
#pragma once

#include <cstddef>
#include <cstdint>

#include "nfa_set_rules.h"     // SET_HAS_*

#define NFA_LSQ_MAX_DIM  24             // include/nestfit_amd.h says the same: four ammonia or eight Gaussian components
#define LSQ_CHUNK_ROWS   4096           // rows per chunk where the caller says 0
#define LSQ_CHUNK_MAX    (1 << 20)      // ... and the most a caller may ask for
#define LSQ_TILE         128            // channels of an LDS tile
#define LSQ_EPT_COLS     16             // columns up to which a thread holds two elements of a tile (16 x 64 = 1024 threads), four above
#define LSQ_STRIDE       (LSQ_TILE + 1) // doubles between the tile's rows: odd, so the rows k = 0 .. 31 that the lanes of a
                                        // wave read at one channel start in 32 different pairs of the 64 four-byte banks

inline int lsq_rows_per_point(int ndim) { return 1 + 2 * ndim; }
inline int64_t lsq_chunk_rows(int64_t chunk_rows) { return chunk_rows == 0 ? LSQ_CHUNK_ROWS : chunk_rows; }
inline int64_t lsq_points_per_chunk(int64_t chunk_rows, int ndim) { return lsq_chunk_rows(chunk_rows) / lsq_rows_per_point(ndim); }
inline int64_t lsq_n_chunks(int64_t points, int64_t chunk_rows, int ndim) {
    const int64_t per = lsq_points_per_chunk(chunk_rows, ndim);
    return (points + per - 1) / per;
}

// the runner's ndim: null, or why it is refused
inline const char *lsq_check_ndim(int ndim) {
    if (ndim < 1) return "normal_equations: the runner has no parameters";
    if (ndim > NFA_LSQ_MAX_DIM) return "normal_equations: more than NFA_LSQ_MAX_DIM = 24 parameters";
    return nullptr;
}
// the caller's chunk_rows for points of `ndim` probed parameters (0: chi^2 alone): null, or why it is refused
inline const char *lsq_check_chunk_rows(int64_t chunk_rows, int ndim) {
    if (chunk_rows < 0 || chunk_rows % 64 != 0) return "chunk_rows must be 0 (4096) or a multiple of 64";
    if (chunk_rows > LSQ_CHUNK_MAX) return "chunk_rows must be 1048576 at most";
    if (lsq_chunk_rows(chunk_rows) < lsq_rows_per_point(ndim)) return "chunk_rows must hold the 1 + 2 ndim rows of a point";
    return nullptr;
}

// Entry (k, l), k <= l, of a symmetric matrix: the upper triangle column by column, whatever the matrix's size --
// consecutive entries share l and walk k, so the lanes of a wave read one row of the tile together and neighbouring rows
// of the weighted tile.  (k > l: the same entry.)
inline int lsq_n_pairs(int ndim) { return (ndim + 1) * (ndim + 2) / 2; }
inline int lsq_pair_index(int k, int l) { return k <= l ? l * (l + 1) / 2 + k : k * (k + 1) / 2 + l; }
inline void lsq_pair_of(int index, int *k, int *l) {
    int c = 0;
    while ((c + 1) * (c + 2) / 2 <= index) ++c;
    *l = c; *k = index - c * (c + 1) / 2;
}

// The Gram launch: one workgroup per point.  The elements (column, channel) of a tile belong to the threads two apiece, or
// (above LSQ_EPT_COLS columns) four, so that the tile's loads are all in flight at once; the first
// (ndim + 1)(ndim + 2) / 2 threads own a Gram entry each.  LDS: the tile T[ndim + 1][LSQ_STRIDE] and the weighted tile w T.
struct LsqGeom { unsigned grid, threads; int ept; size_t lds; };
inline size_t lsq_lds_bytes(int ndim) { return sizeof(double) * 2 * (size_t)(ndim + 1) * LSQ_STRIDE; }
inline LsqGeom lsq_geom(int ndim, int64_t points) {
    const int ncol = ndim + 1, ept = ncol <= LSQ_EPT_COLS ? 2 : 4;
    const unsigned threads = (unsigned)((ncol * LSQ_TILE / ept + 63) / 64 * 64);
    return LsqGeom{(unsigned)points, threads, ept, lsq_lds_bytes(ndim)};
}
// the probe launch: a thread per row of the chunk
inline unsigned lsq_probe_blocks(int64_t points, int ndim) { return (unsigned)((points * lsq_rows_per_point(ndim) + 255) / 256); }

// Scratch of a call of B points (doubles), in this order: theta [B][ndim], 1 / (theta+ - theta-) [B][ndim], chi2 [B],
// grad [B][ndim], curv [B][ndim][ndim], then step, lower, upper [ndim] each
struct LsqScratchPlan { size_t theta, inv_d, chi2, grad, curv, step, lower, upper, total; };
inline LsqScratchPlan lsq_scratch(int64_t B, int ndim) {
    const size_t b = (size_t)B, n = (size_t)ndim;
    LsqScratchPlan P;
    P.theta = 0; P.inv_d = P.theta + b * n; P.chi2 = P.inv_d + b * n; P.grad = P.chi2 + b; P.curv = P.grad + b * n;
    P.step = P.curv + b * n * n; P.lower = P.step + n; P.upper = P.lower + n; P.total = P.upper + n;
    return P;
}

// A set the call serves has a likelihood that is -chi^2 / 2 of white noise: masked channels, a noise per channel and a
// continuum leave it so.  Null, or the sentence the call refuses the set with (the first of the set's features, in this
// order; a response before the correlation it brings along).
inline const char *lsq_refusal(unsigned has) {
    if (has & SET_HAS_BASELINE) return "a set with a baseline takes no normal equations";
    if (has & SET_HAS_TMPL) return "a set with nuisance templates takes no normal equations";
    if (has & SET_HAS_CALIB) return "a set with a calibration uncertainty takes no normal equations";
    if (has & SET_HAS_RESP) return "a set with a channel response takes no normal equations";
    if (has & SET_HAS_CORR) return "a set with correlated channel noise takes no normal equations";
    if (has & SET_HAS_NMARG) return "a set with a noise uncertainty takes no normal equations";
    if (has & SET_HAS_ROBUST) return "a set with a robust likelihood takes no normal equations";
    if (has & ~(unsigned)(SET_HAS_MASK | SET_HAS_CONT)) return "a set with an unknown likelihood option takes no normal equations";
    return nullptr;
}
