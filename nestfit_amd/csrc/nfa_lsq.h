// nfa_lsq.h -- the kernels behind nfa_runner_normal_equations (gfx950, wave64): the probe rows of a chunk of points are
// written on the device, predicted by an ordinary predict launch into the runner's spectra scratch and reduced there to
// chi^2, J^T W r and J^T W J per point; the spectra never cross the bus.  f64 throughout, plain products and sums (the
// build has -ffp-contract=off); no atomics and no order that depends on scheduling: every entry is one thread's sum over
// the channels in channel order, so two calls with the same arguments give the same bits.  Rows, entries, geometry and
// LDS: nfa_lsq_plan.h.  (Included after nfa_device.h: SpecDev.)
#pragma once

#include "nfa_lsq_plan.h"

// The rows of points [0, points) of a chunk into U[points * R][ndim], R = 1 + 2 nj, and their pixel into row_pix: the
// base row theta, then for k = 0 .. nj - 1 theta with theta_k + step_k and with theta_k - step_k, each clipped into
// [lower_k, upper_k] where those are given.  The thread of a theta+ row writes inv_d[point][k] = 1 / (theta+_k - theta-_k)
// of the two doubles as the rows hold them, 0 where they are equal: a fixed parameter.  nj = 0: the base rows alone
// (step, lower, upper and inv_d are not read).  pix: the points' pixels, or null: pixel 0.
__device__ __forceinline__ double lsq_probe(double th, double h, const double *lower, const double *upper, int k) {
    double v = th + h;
    if (lower && v < lower[k]) v = lower[k];
    if (upper && v > upper[k]) v = upper[k];
    return v;
}
__global__ __launch_bounds__(256)
void lsq_probe_kernel(const double *__restrict__ theta, const int *__restrict__ pix, long points, int ndim, int nj,
                      const double *__restrict__ step, const double *__restrict__ lower, const double *__restrict__ upper,
                      double *__restrict__ U, int *__restrict__ row_pix, double *__restrict__ inv_d) {
    const long row = (long)blockIdx.x * 256 + threadIdx.x;
    const int R = 1 + 2 * nj;
    if (row >= points * R) return;
    const long p = row / R;
    const int q = (int)(row - p * R);
    const double *th = theta + p * ndim;
    double *u = U + row * ndim;
    for (int j = 0; j < ndim; ++j) u[j] = th[j];
    row_pix[row] = pix ? pix[p] : 0;
    if (q == 0) return;
    const int k = (q - 1) >> 1;
    const double plus = lsq_probe(th[k], step[k], lower, upper, k), minus = lsq_probe(th[k], -step[k], lower, upper, k);
    if (q & 1) {
        u[k] = plus;
        inv_d[p * ndim + k] = plus == minus ? 0.0 : 1.0 / (plus - minus);
    } else {
        u[k] = minus;
    }
}

// The augmented Gram matrix [J r]^T W [J r] of every point of a chunk.  spec[points * R][chan_tot] are the chunk's model
// spectra in the probe kernel's row order; workgroup = point (point0 + blockIdx.x of the call), thread t < (nj + 1)(nj + 2) / 2
// owns entry (k, l) = lsq_pair_of(t).  The channels go by spectrum and within a spectrum by tiles of LSQ_TILE.  The elements
// (column, channel) of a tile T[nj + 1][tile], numbered column * LSQ_TILE + channel, belong to the threads EPT apiece: t, t +
// blockDim, ... (EPT = 2, or 4 above 16 columns; a wave reads 512 contiguous bytes of a row): J_k = (p(theta+) - p(theta-)) * inv_d_k
// (0 for a fixed parameter), and r = d - p(theta) as the last column; w T goes beside it, w the channel's chan_w (1 without); a
// channel of weight 0 holds zeros whatever the model or the data hold there.  The values of the next tile are loaded into
// registers before the entries of the tile in LDS are summed, so the loads are in flight meanwhile; they go to LDS between
// two barriers.  Each owner adds (w T_k)[c] * T_l[c] over the tile in channel order.  A spectrum's sum is scaled by its
// 1 / sigma_ref^2 as the spectrum ends and added to the point's.  A model value that is not finite at a channel of positive
// weight makes the point's outputs NaN.  chi2[point] = (r, r), grad[point][k] = (J_k, r), curv[point][k][l] = curv[point][l][k]
// = (J_k, J_l); grad and curv are not touched for nj = 0.
template <int EPT>
__global__ __launch_bounds__(1024)
void lsq_gram_kernel(const double *__restrict__ spec, SpecDev S, const int *__restrict__ pix, const double *__restrict__ inv_d,
                     long point0, int nj, double *__restrict__ chi2, double *__restrict__ grad, double *__restrict__ curv) {
    extern __shared__ double lsq_sm[];                         // T[nj + 1][LSQ_STRIDE], w T likewise
    const int ncol = nj + 1, R = 1 + 2 * nj, t = (int)threadIdx.x, nt = (int)blockDim.x;
    double *T = lsq_sm, *WT = lsq_sm + ncol * LSQ_STRIDE;
    const long point = point0 + blockIdx.x, ct = S.chan_tot;
    const long px = pix ? pix[point] : 0;
    const double *rows = spec + (long)blockIdx.x * R * ct;
    const double *data = S.data + px * ct;
    const double *cw = S.chan_w ? S.chan_w + px * ct : nullptr;
    const double *inv = inv_d + point * nj;
    int k = 0, l = 0;
    const bool owner = t < ncol * (ncol + 1) / 2;
    if (owner) { while ((l + 1) * (l + 2) / 2 <= t) ++l; k = t - l * (l + 1) / 2; }
    double v[EPT], wv[EPT];
    int bad = 0;
    // this thread's elements of the tile at channels c0 .. of spectrum s, into v and wv
    auto load = [&](int s, int c0) {
        const int len = S.size[s] - c0 < LSQ_TILE ? S.size[s] - c0 : LSQ_TILE, base = S.off[s] + c0;
#pragma unroll
        for (int i = 0; i < EPT; ++i) {
            const int e = t + i * nt, col = e / LSQ_TILE, c = e - col * LSQ_TILE;
            v[i] = 0.0; wv[i] = 0.0;
            if (col < ncol && c < len) {
                const int ch = base + c;
                const bool res = col == nj;
                const double m = res ? 1.0 : inv[col];         // (r = (d - p) * 1 exactly)
                const double *pa = res ? data + ch : rows + (long)(1 + 2 * col) * ct + ch;
                const double *pb = res ? rows + ch : rows + (long)(2 + 2 * col) * ct + ch;
                const double a = *pa, b = *pb, w = cw ? cw[ch] : 1.0;
                if (w > 0.0 && m != 0.0) {
                    const double d = (a - b) * m;
                    if (!isfinite(d)) bad = 1;
                    v[i] = d; wv[i] = w * d;
                }
            }
        }
    };
    int s = 0, c0 = 0;
    while (s < S.n_spec && S.size[s] <= 0) ++s;
    if (s < S.n_spec) load(s, c0);
    double total = 0.0, acc = 0.0;
    while (s < S.n_spec) {
        const int len = S.size[s] - c0 < LSQ_TILE ? S.size[s] - c0 : LSQ_TILE;
        __syncthreads();                                       // the readers of the tile before are done
#pragma unroll
        for (int i = 0; i < EPT; ++i) {
            const int e = t + i * nt, col = e / LSQ_TILE, c = e - col * LSQ_TILE;
            if (col < ncol) { T[col * LSQ_STRIDE + c] = v[i]; WT[col * LSQ_STRIDE + c] = wv[i]; }
        }
        __syncthreads();
        int ns = s, nc0 = c0 + LSQ_TILE;
        if (nc0 >= S.size[s]) { nc0 = 0; ++ns; while (ns < S.n_spec && S.size[ns] <= 0) ++ns; }
        if (ns < S.n_spec) load(ns, nc0);                      // in flight while the entries are summed
        if (owner) {
            const double *a = WT + k * LSQ_STRIDE, *b = T + l * LSQ_STRIDE;
#pragma unroll 8
            for (int c = 0; c < len; ++c) acc += a[c] * b[c];
        }
        if (ns != s) {
            const double sigma = S.noise[px * S.n_spec + s];
            total += acc * (1.0 / (sigma * sigma));
            acc = 0.0;
        }
        s = ns; c0 = nc0;
    }
    bad = __syncthreads_or(bad);
    if (!owner) return;
    if (bad) total = (double)NAN;
    if (l == nj) {
        if (k == nj) chi2[point] = total;
        else grad[point * nj + k] = total;
    } else {
        curv[(point * nj + k) * nj + l] = total;
        curv[(point * nj + l) * nj + k] = total;
    }
}
