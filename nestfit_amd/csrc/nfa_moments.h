// nfa_moments.h -- reduction kernels behind nfa_runner_predict_moments and nfa_runner_row_statistics (gfx950, wave64):
// the spectra of a predict launch are reduced where they lie, in the runner's spectra scratch, and never cross the bus.
// f64 throughout; no floating-point atomics and no order that depends on scheduling: every sum has a fixed shape
// (lane-strided, then a butterfly over the lanes; rows r, r + R, ... per wave, then r = 0 .. R - 1 through LDS), so
// two calls with the same arguments give the same bits.  Geometry and the cut into pieces: nfa_moments_plan.h.
#pragma once

#include "nfa_moments_plan.h"

struct MomSpecs { int n_spec, size[MAXSPEC], off[MAXSPEC]; };

// Peak and total of every (row, spectrum) of spec[rows][chan_tot]: one wave each, lane l reads channels l, l + 64, ...
// peak: the NaN-ignoring maximum, or (signed != 0: a set with a continuum, the line may absorb) the signed value of
// largest magnitude, the first such channel on ties -- `signed_peak` of the Python side; NaN where every channel is.
// total: the NaN-ignoring sum.  They go to peak[(row * n_spec + s) * step] and total[(row * n_spec + s) * step]
// (step 2 with total = peak + 1: the interleaved matrix [rows][n_spec][2] the moments are taken of; step 1: two arrays).
__global__ __launch_bounds__(MOM_STAT_WAVES * 64)
void row_stats_kernel(const double *__restrict__ spec, long rows, long chan_tot, MomSpecs S, int is_signed,
                      double *__restrict__ peak, double *__restrict__ total, int step) {
    const int lane = threadIdx.x & 63;
    const long unit = (long)blockIdx.x * MOM_STAT_WAVES + (threadIdx.x >> 6);
    if (unit >= rows * S.n_spec) return;                       // (whole waves leave: no barrier below)
    const long row = unit / S.n_spec;
    const int s = (int)(unit - row * S.n_spec);
    const double *p = spec + row * chan_tot + S.off[s];
    const int n = S.size[s];
    double sum = 0.0, best = 0.0;
    int at = -1;                                               // the channel `best` came from; -1: none yet
    for (int j = lane; j < n; j += 64) {
        const double v = p[j];
        if (v != v) continue;
        sum += v;
        if (at < 0 || (is_signed ? fabs(v) > fabs(best) : v > best)) { best = v; at = j; }
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const double o_sum = __shfl_xor(sum, d, 64), o_best = __shfl_xor(best, d, 64);
        const int o_at = __shfl_xor(at, d, 64);
        sum += o_sum;
        const double a = is_signed ? fabs(o_best) : o_best, b = is_signed ? fabs(best) : best;
        if (o_at >= 0 && (at < 0 || a > b || (a == b && o_at < at))) { best = o_best; at = o_at; }
    }
    if (lane == 0) {
        const long k = (row * S.n_spec + s) * step;
        peak[k] = at < 0 ? (double)NAN : best;
        total[k] = sum;
    }
}

// S1, S2 of this chunk's rows added to the running accumulators.  x[rows][ld] is the chunk's matrix (the spectra, or the
// row statistics), ncol of its columns are reduced; ref[n_seg][ncol] the segments' reference rows; acc two planes
// [2][n_seg][ncol].  Workgroup (x = piece, y = column tile) of R waves, lane = column.  With d = x - ref of the piece's
// segment, wave r forms sum w d and sum w d^2 over the rows r, r + R, ... of the piece (rows of weight 0 are left out:
// they contribute nothing, whatever their spectrum holds); wave 0 adds the R partial sums in the order r = 0 .. R - 1
// and then to the accumulator, of which it is the only writer in this launch.  w == nullptr: all ones.
__global__ __launch_bounds__(MOM_RMAX * MOM_TILE)
void moments_accumulate_kernel(const double *__restrict__ x, long ld, long ncol, const double *__restrict__ w,
                               const MomPiece *__restrict__ pieces, const double *__restrict__ ref,
                               double *__restrict__ acc, long n_seg, int R) {
    extern __shared__ double mom_sm[];                         // [R][2][MOM_TILE]
    const int lane = threadIdx.x & 63, r = threadIdx.x >> 6;
    const MomPiece P = pieces[blockIdx.x];
    const long col = (long)blockIdx.y * MOM_TILE + lane;
    const bool live = col < ncol;
    double s1 = 0.0, s2 = 0.0;
    if (live) {
        const double base = ref[(long)P.seg * ncol + col];
        const double *px = x + (long)P.row0 * ld + col;
        const double *pw = w ? w + P.row0 : nullptr;
        int i = r;
        for (; i + 3 * R < P.n; i += 4 * R) {                  // four rows in flight per lane
            const double v0 = px[(long)i * ld], v1 = px[(long)(i + R) * ld], v2 = px[(long)(i + 2 * R) * ld], v3 = px[(long)(i + 3 * R) * ld];
            const double w0 = pw ? pw[i] : 1.0, w1 = pw ? pw[i + R] : 1.0, w2 = pw ? pw[i + 2 * R] : 1.0, w3 = pw ? pw[i + 3 * R] : 1.0;
            const double d0 = v0 - base, d1 = v1 - base, d2 = v2 - base, d3 = v3 - base;
            if (w0 != 0.0) { const double t = w0 * d0; s1 += t; s2 += t * d0; }
            if (w1 != 0.0) { const double t = w1 * d1; s1 += t; s2 += t * d1; }
            if (w2 != 0.0) { const double t = w2 * d2; s1 += t; s2 += t * d2; }
            if (w3 != 0.0) { const double t = w3 * d3; s1 += t; s2 += t * d3; }
        }
        for (; i < P.n; i += R) {
            const double wi = pw ? pw[i] : 1.0, d = px[(long)i * ld] - base;
            if (wi != 0.0) { const double t = wi * d; s1 += t; s2 += t * d; }
        }
    }
    if (R > 1) {
        mom_sm[(r * 2 + 0) * MOM_TILE + lane] = s1;
        mom_sm[(r * 2 + 1) * MOM_TILE + lane] = s2;
        __syncthreads();
        if (r != 0) return;
        s1 = mom_sm[lane]; s2 = mom_sm[MOM_TILE + lane];
        for (int q = 1; q < R; ++q) { s1 += mom_sm[(q * 2 + 0) * MOM_TILE + lane]; s2 += mom_sm[(q * 2 + 1) * MOM_TILE + lane]; }
    }
    if (live) {
        acc[(long)P.seg * ncol + col] += s1;
        acc[(n_seg + P.seg) * ncol + col] += s2;
    }
}

// Mean and std from the accumulators, in place: plane 0 becomes ref + S1 / S0, plane 1 sqrt(max(S2 / S0 - (S1 / S0)^2, 0));
// NaN in both for a segment whose weights sum to 0 (s0[seg], the host's sum; an empty segment has 0).
__global__ __launch_bounds__(256)
void moments_finish_kernel(double *__restrict__ acc, const double *__restrict__ ref, const double *__restrict__ s0,
                           long n_seg, long ncol) {
    const long k = (long)blockIdx.x * 256 + threadIdx.x;
    if (k >= n_seg * ncol) return;
    const double S0 = s0[k / ncol];
    if (!(S0 > 0.0)) { acc[k] = (double)NAN; acc[n_seg * ncol + k] = (double)NAN; return; }
    const double m1 = acc[k] / S0, var = acc[n_seg * ncol + k] / S0 - m1 * m1;
    acc[k] = ref[k] + m1;
    acc[n_seg * ncol + k] = var < 0.0 ? 0.0 : sqrt(var);
}

// Row g of out[n][ndim] = the first row of segment first + g of theta[.][ndim] on the device, whose segments are seg_rows
// rows each: the reference rows where the rows of a call lie in HBM with equal weights (a segment's row of largest weight
// is then its first).  A thread per double.
__global__ __launch_bounds__(256)
void moments_first_rows_kernel(const double *__restrict__ theta, long seg_rows, long first, long n, int ndim, double *__restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n * ndim) return;
    const long g = i / ndim, k = i - g * ndim;
    out[i] = theta[(first + g) * seg_rows * ndim + k];
}
