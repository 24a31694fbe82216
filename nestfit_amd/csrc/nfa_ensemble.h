// nfa_ensemble.h -- the kernels behind nfa_ensemble_* (gfx950, wave64): an affine-invariant ensemble sampler (the stretch
// move of Goodman & Weare 2010) of many pixels in lock-step, in the sampled slots of the unit cube, around the engine's
// likelihood batch.  The contract is the head of nfa_ensemble_plan.h.  f64 throughout, plain products and sums (the build
// has -ffp-contract=off), the nested sampler's counter-based random numbers; no atomics and no order that depends on
// scheduling: the same arguments give the same bits.  One half-step is ens_propose_kernel, the likelihood launches over
// its P W/2 rows, ens_accept_kernel; a step ends with ens_trace_kernel and, where it is kept, ens_keep_kernel.  The chain
// is reduced where it lies: ens_summary_kernel, ens_hist_kernel (whose integer counts alone meet in LDS adds: the same in
// any order), ens_cov_kernel, and the moments of its model spectra through the engine's mom_reduce.
// A tempered ensemble runs T rungs per pixel through the same kernels, a (pixel, rung) unit in the place of a
// pixel; ens_swap_kernel exchanges walkers between neighbouring rungs after the half-steps of a step, and
// ens_evidence_kernel reduces the rungs' kept lnL to the terms of the stepping-stone evidence.
// (Included after nfa_sampler.h: ns_stream, ns_uniform_of.)
#pragma once

#include "nfa_ensemble_plan.h"

struct EnsDev {
    int     P, W, D, DT;                // units, walkers per unit, SAMPLED dimensions, length of a theta row
    int     T;                          // rungs per pixel: unit p is rung p % T of pixel p / T.  Untempered: T = 1, a unit is a pixel
    const double *betas;                // [T] the ladder (untempered: null, beta = 1)
    const int *fmap;                    // [D] slot of every sampled dimension; the others stay at u = 0.5
    const int *pix;                     // [P] cube pixel of every unit of the run: in the random stream and in the rows
    double *u, *theta, *lnL;            // the walkers: [P][W][D], [P][W][DT], [P][W]
    double *rows, *row_lnL, *y;         // a half-step's batch: [P W/2][DT] (u in, theta out), [P W/2], and the proposals [P W/2][D]
    int    *row_pix, *inside;           // [P W/2] each
    long   *counts;                     // [P][3]: accepted, outside, evaluated
    long   *swaps;                      // [P / T][T - 1][2]: swaps accepted, proposed, of the pair (t, t + 1)
};

__device__ __forceinline__ double ens_stretch(double a, double r1) {
    const double t = (a - 1.0) * r1 + 1.0;
    return t * t / a;
}
__device__ __forceinline__ uint64_t ens_stream(const EnsDev &E, uint64_t seed, int p, long step, int h) {
    return ns_stream(seed, (uint64_t)E.pix[p], ens_move_tag(p % E.T, step, h));
}
__device__ __forceinline__ double ens_beta(const EnsDev &E, int p) { return E.T > 1 ? E.betas[p % E.T] : 1.0; }

// Workgroup = pixel, thread m < W/2 = walker k = h W/2 + m of the moving half.  Writes the proposal y, whether it is
// inside, and the batch row: y through fmap where it is inside, the walker's own u where it is not (every half-step has
// the same P W/2 rows: no compaction, no count read back), 0.5 in the slots that are not sampled.
__global__ __launch_bounds__(256)
void ens_propose_kernel(EnsDev E, long step, int h, double a, uint64_t seed) {
    const int p = (int)blockIdx.x, m = (int)threadIdx.x, half = E.W >> 1;
    if (m >= half) return;
    const int k = h * half + m, other = (1 - h) * half;
    const uint64_t strm = ens_stream(E, seed, p, step, h);
    const double r0 = ns_uniform_of(strm, 3ull * (uint64_t)k), r1 = ns_uniform_of(strm, 3ull * (uint64_t)k + 1ull);
    const int j = other + min((int)(r0 * (double)half), half - 1);
    const double z = ens_stretch(a, r1);
    const long row = (long)p * half + m;
    const double *uk = E.u + ((long)p * E.W + k) * E.D, *uj = E.u + ((long)p * E.W + j) * E.D;
    double *y = E.y + row * E.D, *t = E.rows + row * E.DT;
    int in = 1;
    for (int d = 0; d < E.D; ++d) {
        const double v = uj[d] + z * (uk[d] - uj[d]);
        y[d] = v;
        if (!(v > 0.0 && v < 1.0)) in = 0;
    }
    for (int c = 0; c < E.DT; ++c) t[c] = 0.5;
    for (int d = 0; d < E.D; ++d) t[E.fmap[d]] = in ? y[d] : uk[d];
    E.row_pix[row] = E.pix[p];
    E.inside[row] = in;
}

// Same geometry, after the likelihood of the rows.  An accepted walker takes y, the row's theta and its lnL.  The pixel's
// counters: every wave counts its lanes with a ballot, the waves' counts meet in LDS and thread 0 adds them in wave order
// (one workgroup per pixel: one writer).
__global__ __launch_bounds__(256)
void ens_accept_kernel(EnsDev E, long step, int h, double a, uint64_t seed) {
    __shared__ int s_acc[4], s_out[4];
    const int p = (int)blockIdx.x, m = (int)threadIdx.x, half = E.W >> 1;
    int acc = 0, out = 0;
    if (m < half) {
        const int k = h * half + m;
        const long row = (long)p * half + m, w = (long)p * E.W + k;
        const uint64_t strm = ens_stream(E, seed, p, step, h);
        const double r1 = ns_uniform_of(strm, 3ull * (uint64_t)k + 1ull), r2 = ns_uniform_of(strm, 3ull * (uint64_t)k + 2ull);
        const double z = ens_stretch(a, r1), Ly = E.row_lnL[row], Lk = E.lnL[w];
        out = E.inside[row] ? 0 : 1;
        if (!out && isfinite(Ly)) {
            const double rhs = (double)(E.D - 1) * log(z) + ens_beta(E, p) * (Ly - Lk);       // (beta = 1 multiplies exactly)
            acc = log(r2) < rhs ? 1 : 0;
        }
        if (acc) {
            const double *y = E.y + row * E.D, *t = E.rows + row * E.DT;
            double *uk = E.u + w * E.D, *tk = E.theta + w * E.DT;
            for (int d = 0; d < E.D; ++d) uk[d] = y[d];
            for (int c = 0; c < E.DT; ++c) tk[c] = t[c];
            E.lnL[w] = Ly;
        }
    }
    const int wave = (int)threadIdx.x >> 6, nw = (int)blockDim.x >> 6;
    const int wa = __popcll(__ballot(acc)), wo = __popcll(__ballot(out));
    if ((threadIdx.x & 63) == 0) { s_acc[wave] = wa; s_out[wave] = wo; }
    __syncthreads();
    if (threadIdx.x == 0) {
        long ta = 0, to = 0;
        for (int v = 0; v < nw; ++v) { ta += s_acc[v]; to += s_out[v]; }
        long *c = E.counts + (long)p * 3;
        c[0] += ta; c[1] += to; c[2] += half;
    }
}

// One wave per pixel: trace[p][step - 1][0 .. D] = the mean over the walkers of every sampled u and of lnL.  Lane l adds
// walkers l, l + 64, ... in that order, then a butterfly over the lanes (32, 16, .. 1): a fixed shape, the same bits.
__global__ __launch_bounds__(64)
void ens_trace_kernel(EnsDev E, long step, long n_steps, double *__restrict__ trace) {
    const int p = (int)blockIdx.x, lane = (int)threadIdx.x;
    double *out = trace + ((long)p * n_steps + (step - 1)) * (E.D + 1);
    for (int q = 0; q <= E.D; ++q) {
        double v = 0.0;
        for (int w = lane; w < E.W; w += 64) v += q < E.D ? E.u[((long)p * E.W + w) * E.D + q] : E.lnL[(long)p * E.W + w];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if (lane == 0) out[q] = v / (double)E.W;
    }
}

// The state into slot `slot` of the chain; a thread per double of the state's theta and lnL.  Rung 0 of pixel q goes to the
// cold chain, chain_theta[P / T][n_keep][W][DT] and chain_lnL[P / T][n_keep][W]; lnL of every unit p to rung_lnL[P][n_keep][W]
// where that is given (a tempered ensemble).
__global__ __launch_bounds__(256)
void ens_keep_kernel(EnsDev E, long slot, long n_keep, double *__restrict__ chain_theta, double *__restrict__ chain_lnL,
                     double *__restrict__ rung_lnL) {
    const long nt = (long)E.W * E.DT, per = nt + E.W, i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)E.P * per) return;
    const long p = i / per, e = i - p * per, q = p / E.T;
    const bool cold = p - q * E.T == 0;
    if (e < nt) {
        if (cold) chain_theta[(q * n_keep + slot) * nt + e] = E.theta[p * nt + e];
    } else {
        const double v = E.lnL[p * E.W + (e - nt)];
        if (cold) chain_lnL[(q * n_keep + slot) * E.W + (e - nt)] = v;
        if (rung_lnL) rung_lnL[(p * n_keep + slot) * E.W + (e - nt)] = v;
    }
}

// ---- a tempered ensemble: swaps and the evidence -------------------------------------------------------------------
// Workgroup = (pixel q, active pair i of the sweep) = blockIdx.x / n_pairs, blockIdx.x % n_pairs: the rungs t = parity + 2 i
// and t + 1 of the pixel; the pairs of a sweep are disjoint, so no workgroup reads what another writes.  Thread k < W
// exchanges walker k of the two rungs -- u, theta and lnL, D + DT + 1 doubles -- iff log(r) < (beta_t - beta_t+1)(lnL_t+1,k -
// lnL_t,k).  The pair's counters as ens_accept_kernel counts: a ballot per wave, the waves through LDS, thread 0 adds in
// wave order.  (lnL of a walker is finite: the run has made it so and accepts nothing else.)
__global__ __launch_bounds__(ENS_SWAP_THREADS_MAX)
void ens_swap_kernel(EnsDev E, long step, int parity, int n_pairs, uint64_t seed) {
    __shared__ int s_acc[ENS_SWAP_THREADS_MAX / 64];
    const int q = (int)blockIdx.x / n_pairs, t = parity + 2 * ((int)blockIdx.x - q * n_pairs), k = (int)threadIdx.x;
    const long a = (long)q * E.T + t, b = a + 1;
    int acc = 0;
    if (k < E.W) {
        const long wa = a * E.W + k, wb = b * E.W + k;
        const double r = ns_uniform_of(ns_stream(seed, (uint64_t)E.pix[a], ens_swap_tag(t, step)), (uint64_t)k);
        const double La = E.lnL[wa], Lb = E.lnL[wb];
        const double rhs = (E.betas[t] - E.betas[t + 1]) * (Lb - La);
        acc = log(r) < rhs ? 1 : 0;
        if (acc) {
            double *ua = E.u + wa * E.D, *ub = E.u + wb * E.D, *ta = E.theta + wa * E.DT, *tb = E.theta + wb * E.DT;
            for (int d = 0; d < E.D; ++d) { const double v = ua[d]; ua[d] = ub[d]; ub[d] = v; }
            for (int c = 0; c < E.DT; ++c) { const double v = ta[c]; ta[c] = tb[c]; tb[c] = v; }
            E.lnL[wa] = Lb; E.lnL[wb] = La;
        }
    }
    const int wave = (int)threadIdx.x >> 6, nw = (int)blockDim.x >> 6;
    const int n = __popcll(__ballot(acc));
    if ((threadIdx.x & 63) == 0) s_acc[wave] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        long ta = 0;
        for (int v = 0; v < nw; ++v) ta += s_acc[v];
        long *c = E.swaps + ((long)q * (E.T - 1) + t) * 2;
        c[0] += ta; c[1] += E.W;
    }
}

// the largest of v over the workgroup, known to every thread (a maximum does not depend on the order it is taken in)
__device__ __forceinline__ double ens_block_max(double v, double *red) {
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    const int nw = (int)blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = red[0];
    for (int w = 1; w < nw; ++w) t = fmax(t, red[w]);
    return t;
}

// ---- the summary of a chain --------------------------------------------------------------------------------------
// Sums over the workgroup in a fixed shape: a butterfly inside every wave, the waves' results through red[] in wave order.
__device__ __forceinline__ double ens_block_sum(double v, double *red) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    const int nw = (int)blockDim.x >> 6;
    __syncthreads();                                           // the readers of the sum before are done
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    for (int w = 0; w < nw; ++w) t += red[w];
    return t;
}
// (value, index) a before b: the larger value, the smaller index on ties
__device__ __forceinline__ bool ens_before(double va, long ia, double vb, long ib) { return va > vb || (va == vb && ia < ib); }

// The row of largest lnL among L[0 .. N), the first on ties (row 0 where every lnL is NaN), known to every thread of the
// workgroup: a strided scan, a butterfly inside every wave, the waves' candidates through redv[], redi[] in wave order.
__device__ __forceinline__ long ens_best_row(const double *__restrict__ L, long N, double *redv, long *redi) {
    const int t = (int)threadIdx.x, T = (int)blockDim.x, lane = t & 63, wave = t >> 6, nw = T >> 6;
    double bv = -INFINITY; long bi = N;
    for (long i = t; i < N; i += T) { const double v = L[i]; if (ens_before(v, i, bv, bi)) { bv = v; bi = i; } }
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(bv, off); const long oi = __shfl_xor(bi, off);
        if (ens_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) { redv[wave] = bv; redi[wave] = bi; }
    __syncthreads();
    bv = redv[0]; bi = redi[0];
    for (int w = 1; w < nw; ++w) if (ens_before(redv[w], redi[w], bv, bi)) { bv = redv[w]; bi = redi[w]; }
    return bi >= N ? 0 : bi;
}

// Workgroup = pixel; N = n_keep W kept samples in (keep, walker) order.  best[p][0 .. DT] = theta and lnL of the row of
// largest lnL, the first on ties.  Per parameter c, with d_i = x_i - best_c: summary[p][c] = (best_c + S1 / N,
// sqrt(max(S2 / N - (S1 / N)^2, 0))) -- moments of differences, for the reason DESIGN 4.21 gives; one sample: std 0.  With
// nq > 0 levels (N <= NFA_ENS_MAX_SORT) the parameter's samples are sorted in LDS, padded with +inf to npow2 (bitonic: a
// thread per compare-exchange), and quant[p][c][l] = s[i] + (s[i + 1] - s[i]) g with h = (N - 1) q_l, i = floor(h), g = h - i.
// Dynamic LDS: red[ENS_RED_DOUBLES], then s[npow2].
__global__ __launch_bounds__(1024)
void ens_summary_kernel(const double *__restrict__ chain_theta, const double *__restrict__ chain_lnL, long N, int DT,
                        const double *__restrict__ levels, int nq, long npow2,
                        double *__restrict__ summary, double *__restrict__ best, double *__restrict__ quant) {
    extern __shared__ __attribute__((aligned(16))) double ens_sm[];
    double *red = ens_sm, *redv = ens_sm + 16, *s = ens_sm + ENS_RED_DOUBLES;
    long *redi = (long *)(ens_sm + 32);
    const long p = blockIdx.x;
    const int t = (int)threadIdx.x, T = (int)blockDim.x;
    const double *X = chain_theta + p * N * DT, *L = chain_lnL + p * N;
    const long bi = ens_best_row(L, N, redv, redi);
    if (t <= DT) best[p * (DT + 1) + t] = t < DT ? X[bi * DT + t] : L[bi];
    const double inv_n = 1.0 / (double)N;
    for (int c = 0; c < DT; ++c) {
        const double ref = X[bi * DT + c];
        double s1 = 0.0, s2 = 0.0;
        for (long i = t; i < N; i += T) { const double d = X[i * DT + c] - ref; s1 += d; s2 += d * d; }
        s1 = ens_block_sum(s1, red);
        s2 = ens_block_sum(s2, red);
        if (t == 0) {
            const double m = s1 * inv_n, var = s2 * inv_n - m * m;
            summary[(p * DT + c) * 2] = ref + m;
            summary[(p * DT + c) * 2 + 1] = var > 0.0 ? sqrt(var) : 0.0;
        }
        if (nq <= 0) continue;
        __syncthreads();                                       // the quantiles of the parameter before are read
        for (long i = t; i < npow2; i += T) s[i] = i < N ? X[i * DT + c] : (double)INFINITY;
        __syncthreads();
        for (long k = 2; k <= npow2; k <<= 1) {
            for (long j = k >> 1; j > 0; j >>= 1) {
                for (long i = t; i < npow2; i += T) {
                    const long o = i ^ j;
                    if (o > i) {
                        const double x = s[i], y = s[o];
                        if ((i & k) == 0 ? x > y : x < y) { s[i] = y; s[o] = x; }
                    }
                }
                __syncthreads();
            }
        }
        if (t < nq) {
            const double hq = (double)(N - 1) * levels[t];
            const long i = (long)hq, i1 = i + 1 < N ? i + 1 : N - 1;
            const double g = hq - (double)i;
            quant[(p * DT + c) * nq + t] = s[i] + (s[i1] - s[i]) * g;
        }
    }
}

// ---- the products of a chain -------------------------------------------------------------------------------------
// Workgroup = (pixel p, parameter c) = blockIdx.x / DT, blockIdx.x % DT of a slab of pixels whose chain starts at chain_theta.
// The parameter's nb + 1 edges and nb + 1 32-bit counters (the last: outside) sit in LDS.  A thread takes the samples t,
// t + T, ... of the pixel's N (stride DT doubles, as the summary reads them); a sample inside [e_0, e_nb] finds the last
// edge not above it among e_0 .. e_nb-1 by a binary search without a branch on the data -- so x == e_nb lands in the last
// bin, as np.histogram puts it -- and counts there with an integer LDS add: integer counts are the same in any order.  The
// workgroup is the one writer of its nb counts, widened to 64 bits; no global atomics.  (The host has checked N < 2^32.)
__global__ __launch_bounds__(256)
void ens_hist_kernel(const double *__restrict__ chain_theta, long N, int DT, const double *__restrict__ edges, int nb,
                     long *__restrict__ counts, long *__restrict__ outside) {
    extern __shared__ __attribute__((aligned(16))) double ens_hist_sm[];
    double *ed = ens_hist_sm;
    unsigned *cnt = (unsigned *)(ens_hist_sm + nb + 1);
    const long p = blockIdx.x / (unsigned)DT;
    const int c = (int)(blockIdx.x - (unsigned)p * (unsigned)DT), t = (int)threadIdx.x, T = (int)blockDim.x;
    for (int b = t; b <= nb; b += T) { ed[b] = edges[(long)c * (nb + 1) + b]; cnt[b] = 0u; }
    __syncthreads();
    const double *X = chain_theta + p * N * DT + c;
    const double lo = ed[0], hi = ed[nb];
    unsigned out = 0u;
    for (long i = t; i < N; i += T) {
        const double x = X[i * DT];
        if (!(x >= lo && x <= hi)) { out += 1u; continue; }   // (a NaN too)
        int b = 0, n = nb;                                     // the last edge <= x lies in [b, b + n)
        while (n > 1) {
            const int half = n >> 1;
            b = ed[b + half] <= x ? b + half : b;
            n -= half;
        }
        atomicAdd(&cnt[b], 1u);
    }
    if (out) atomicAdd(&cnt[nb], out);
    __syncthreads();
    const long o = p * DT + c;
    for (int b = t; b < nb; b += T) counts[o * nb + b] = (long)cnt[b];
    if (t == 0) outside[o] = (long)cnt[nb];
}

// Workgroup = pixel of a slab whose chain starts at chain_theta, chain_lnL; cov[p][DT][DT].  About the best row (ens_best_row,
// the summary's): first every parameter's S_a and S_aa -> its mean of differences m_a = S_a / N into LDS and the diagonal
// max(S_aa / N - m_a^2, 0); then every pair a < b: cov_ab = S_ab / N - m_a m_b, written at [a][b] and [b][a].  Every sum is
// a strided scan and ens_block_sum: a fixed shape, no atomics.  A parameter that is constant has d = 0 throughout: an exact
// zero row and column.
__global__ __launch_bounds__(256)
void ens_cov_kernel(const double *__restrict__ chain_theta, const double *__restrict__ chain_lnL, long N, int DT, double *__restrict__ cov) {
    __shared__ double red[4], redv[4], m[NS_MAXD];
    __shared__ long redi[4];
    const long p = blockIdx.x;
    const int t = (int)threadIdx.x, T = (int)blockDim.x;
    const double *X = chain_theta + p * N * DT, *L = chain_lnL + p * N;
    double *C = cov + p * DT * DT;
    const double *R = X + ens_best_row(L, N, redv, redi) * DT;
    const double n = (double)N;
    for (int a = 0; a < DT; ++a) {
        const double ra = R[a];
        double s1 = 0.0, s2 = 0.0;
        for (long i = t; i < N; i += T) { const double d = X[i * DT + a] - ra; s1 += d; s2 += d * d; }
        s1 = ens_block_sum(s1, red);
        s2 = ens_block_sum(s2, red);
        if (t == 0) {
            const double ma = s1 / n, var = s2 / n - ma * ma;
            m[a] = ma;
            C[a * DT + a] = var > 0.0 ? var : 0.0;
        }
    }
    __syncthreads();
    for (int a = 0; a < DT; ++a)
        for (int b = a + 1; b < DT; ++b) {
            const double ra = R[a], rb = R[b];
            double s = 0.0;
            for (long i = t; i < N; i += T) s += (X[i * DT + a] - ra) * (X[i * DT + b] - rb);
            s = ens_block_sum(s, red);
            if (t == 0) {
                const double v = s / n - m[a] * m[b];
                C[a * DT + b] = v;
                C[b * DT + a] = v;
            }
        }
}

// Workgroup = unit (pixel, rung t) of a tempered ensemble; x = rung_lnL of the unit, n_keep W doubles on end, so a set is a
// contiguous run of them and the strided reads of a wave are coalesced.  For the sets j = 0 .. n_blocks (ens_set_first,
// ens_set_steps) two passes: the maximum M, then S1 = sum d_i, S2 = sum d_i^2 with d_i = x_i - x_first and Se = sum exp(delta
// (x_i - M)), each a strided scan and ens_block_sum: a fixed shape.  out[unit][j] = (x_first + S1 / n, max(S2 / n - (S1 / n)^2,
// 0), delta M + log(Se / n)); rung 0 has r = 0.  The largest term of Se is exp(0) = 1, so Se >= 1 and the log is finite.
__global__ __launch_bounds__(ENS_EVID_THREADS)
void ens_evidence_kernel(const double *__restrict__ rung_lnL, const double *__restrict__ betas, int T, long n_keep, int W, int n_blocks,
                         double *__restrict__ out) {
    __shared__ double red[ENS_EVID_THREADS / 64];
    const long unit = blockIdx.x;
    const int t = (int)(unit % T), tid = (int)threadIdx.x, nt = (int)blockDim.x;
    const double delta = t > 0 ? betas[t - 1] - betas[t] : 0.0;
    for (int j = 0; j <= n_blocks; ++j) {
        const long n = ens_set_steps(n_keep, n_blocks, j) * W;
        const double *x = rung_lnL + unit * n_keep * W + ens_set_first(n_keep, n_blocks, j) * W;
        double m = -INFINITY;
        for (long i = tid; i < n; i += nt) m = fmax(m, x[i]);
        m = ens_block_max(m, red);
        const double x0 = x[0];
        double s1 = 0.0, s2 = 0.0, se = 0.0;
        for (long i = tid; i < n; i += nt) {
            const double v = x[i], d = v - x0;
            s1 += d; s2 += d * d;
            se += exp(delta * (v - m));
        }
        s1 = ens_block_sum(s1, red);
        s2 = ens_block_sum(s2, red);
        se = ens_block_sum(se, red);
        if (tid == 0) {
            const double nn = (double)n, mean = s1 / nn, var = s2 / nn - mean * mean;
            double *o = out + (unit * (n_blocks + 1) + j) * 3;
            o[0] = x0 + mean;
            o[1] = var > 0.0 ? var : 0.0;
            o[2] = t > 0 ? delta * m + log(se / nn) : 0.0;
        }
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------
// Everything an ensemble holds on the device belongs to it: `bufs` lives as long as the ensemble, `run_bufs` (chain and
// trace) as long as the last run.  The likelihood batch works on the ensemble's own rows, as the nested sampler's does on
// its candidates: run_batch on lane 0, nothing of the runner's staging.
struct nfa_ensemble {
    nfa_runner *r = nullptr;
    EnsDev d = {};
    std::vector<int> fm;                 // sampled slots
    int64_t n_pix = 0;                   // pixels: d.P = n_pix d.T units
    std::vector<int32_t> h_pix;          // [n_pix] the cube pixels (d.pix holds the one of every unit)
    bool has_pix = false;
    int *d_start_pix = nullptr;          // [P][W] cube pixel of every start row
    std::vector<void *> bufs, run_bufs;
    double *chain_theta = nullptr, *chain_lnL = nullptr, *trace = nullptr;      // the cold chain; the trace of every unit
    double *d_summary = nullptr, *d_best = nullptr, *d_quant = nullptr, *d_levels = nullptr;
    int64_t n_keep = 0, n_steps = 0;
    // a tempered ensemble (d.T > 1)
    std::vector<double> h_betas;
    int64_t swap_every = 0;
    double *rung_lnL = nullptr;          // [P][n_keep][W] of the last run
    double *d_evid = nullptr;            // [P][NFA_ENS_MAX_BLOCKS + 1][3] at most
};
static bool ens_tempered(const nfa_ensemble *e) { return e->d.T > 1; }

template <typename T>
static int ens_alloc(std::vector<void *> &owner, T **out, size_t count) {
    void *p = nullptr;
    HIP_TRY(hipMalloc(&p, sizeof(T) * std::max<size_t>(count, 1)));
    owner.push_back(p);
    *out = (T *)p;
    return NFA_OK;
}
static void ens_free(std::vector<void *> &owner) {
    for (void *p : owner) (void)hipFree(p);
    owner.clear();
}
// the likelihood of `rows` rows on lane 0, in pieces of ENS_PIECE_ROWS at most
static int ens_evaluate(nfa_runner *r, const int *d_pix, double *d_rows, double *d_lnL, int64_t rows) {
    for (int64_t a = 0; a < rows; a += ENS_PIECE_ROWS) {
        const int64_t n = std::min<int64_t>(ENS_PIECE_ROWS, rows - a);
        int rc = run_batch(r, d_pix + a, d_rows + a * r->ndim, d_lnL + a, nullptr, n, true, 0);
        if (rc) return rc;
    }
    return NFA_OK;
}
// after a failure on lane 0: whatever was enqueued is waited for, so that the runner is usable and buffers may go
static int ens_abandon(nfa_runner *r, int rc) {
    const std::string why = g_err;
    (void)hipStreamSynchronize(r->lanes[0]);
    (void)hipGetLastError();
    r->lane_busy &= ~1u;
    g_err = why;
    return rc;
}

static int ens_create_on_device(nfa_ensemble *e, const int32_t *pix, const std::vector<double> &u, const std::vector<double> &rows) {
    nfa_runner *r = e->r;
    EnsDev &d = e->d;
    const size_t P = (size_t)d.P, W = (size_t)d.W, D = (size_t)d.D, DT = (size_t)d.DT, half = W / 2, T = (size_t)d.T, NP = (size_t)e->n_pix;
    int rc;
    int *fmap = nullptr, *dpix = nullptr;
    if (T > 1) {
        double *betas = nullptr;
        if ((rc = ens_alloc(e->bufs, &betas, T)) || (rc = ens_alloc(e->bufs, &d.swaps, NP * (T - 1) * 2)) ||
            (rc = ens_alloc(e->bufs, &e->d_evid, P * (NFA_ENS_MAX_BLOCKS + 1) * 3)))
            return rc;
        d.betas = betas;
        HIP_TRY(hipMemcpy(betas, e->h_betas.data(), sizeof(double) * T, hipMemcpyHostToDevice));
        HIP_TRY(hipMemset(d.swaps, 0, sizeof(long) * NP * (T - 1) * 2));
    }
    if ((rc = ens_alloc(e->bufs, &fmap, D)) || (rc = ens_alloc(e->bufs, &dpix, P)) ||
        (rc = ens_alloc(e->bufs, &d.u, P * W * D)) || (rc = ens_alloc(e->bufs, &d.theta, P * W * DT)) ||
        (rc = ens_alloc(e->bufs, &d.lnL, P * W)) || (rc = ens_alloc(e->bufs, &e->d_start_pix, P * W)) ||
        (rc = ens_alloc(e->bufs, &d.rows, P * half * DT)) || (rc = ens_alloc(e->bufs, &d.row_lnL, P * half)) ||
        (rc = ens_alloc(e->bufs, &d.y, P * half * D)) || (rc = ens_alloc(e->bufs, &d.row_pix, P * half)) ||
        (rc = ens_alloc(e->bufs, &d.inside, P * half)) || (rc = ens_alloc(e->bufs, &d.counts, P * 3)) ||
        (rc = ens_alloc(e->bufs, &e->d_summary, NP * DT * 2)) || (rc = ens_alloc(e->bufs, &e->d_best, NP * (DT + 1))) ||
        (rc = ens_alloc(e->bufs, &e->d_quant, NP * DT * NFA_ENS_MAX_Q)) || (rc = ens_alloc(e->bufs, &e->d_levels, (size_t)NFA_ENS_MAX_Q)))
        return rc;
    d.fmap = fmap; d.pix = dpix;
    std::vector<int32_t> &h_pix = e->h_pix;
    std::vector<int32_t> h_unit(P, 0);
    std::vector<int> h_start(P * W, 0);
    h_pix.assign(NP, 0);
    for (size_t q = 0; q < NP; ++q) h_pix[q] = pix ? pix[q] : 0;
    for (size_t p = 0; p < P; ++p) {
        h_unit[p] = h_pix[p / T];
        for (size_t w = 0; w < W; ++w) h_start[p * W + w] = h_unit[p];
    }
    HIP_TRY(hipMemcpy(fmap, e->fm.data(), sizeof(int) * D, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dpix, h_unit.data(), sizeof(int) * P, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->d_start_pix, h_start.data(), sizeof(int) * P * W, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d.u, u.data(), sizeof(double) * P * W * D, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d.theta, rows.data(), sizeof(double) * P * W * DT, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(d.counts, 0, sizeof(long) * P * 3));
    // the start rows, once: theta and lnL of every walker, straight into the state
    rc = ens_evaluate(r, e->d_start_pix, d.theta, d.lnL, (int64_t)(P * W));
    if (rc) return ens_abandon(r, rc);
    hipError_t err = hipStreamSynchronize(r->lanes[0]);
    r->lane_busy &= ~1u;
    if (err != hipSuccess) return fail(NFA_ERR_DEVICE, std::string("ensemble start rows: ") + hipGetErrorString(err));
    return NFA_OK;
}

// count blocks of `per` doubles (or longs), every stride-th of those at src: the units of an ensemble, or rung 0 of every pixel
template <typename V>
static int ens_fetch(V *dst, const V *src, size_t per, size_t count, size_t stride) {
    if (stride == 1) HIP_TRY(hipMemcpy(dst, src, sizeof(V) * per * count, hipMemcpyDeviceToHost));
    else HIP_TRY(hipMemcpy2D(dst, sizeof(V) * per, src, sizeof(V) * per * stride, sizeof(V) * per, count, hipMemcpyDeviceToHost));
    return NFA_OK;
}
// the three fetches of the state, of every unit (rungs) or of the cold rung of every pixel
static int ens_get_counts(nfa_ensemble *e, bool rungs, int64_t *accepted, int64_t *outside, int64_t *evaluated) {
    const size_t n = rungs ? (size_t)e->d.P : (size_t)e->n_pix;
    std::vector<long> h(n * 3);
    int rc = ens_fetch(h.data(), (const long *)e->d.counts, 3, n, rungs ? 1 : (size_t)e->d.T); if (rc) return rc;
    for (size_t p = 0; p < n; ++p) { accepted[p] = h[3 * p]; outside[p] = h[3 * p + 1]; evaluated[p] = h[3 * p + 2]; }
    return NFA_OK;
}
static int ens_get_state(nfa_ensemble *e, bool rungs, double *u, double *theta, double *lnL) {
    const EnsDev &d = e->d;
    const size_t units = rungs ? (size_t)d.P : (size_t)e->n_pix, stride = rungs ? 1 : (size_t)d.T, W = (size_t)d.W, n = units * W;
    int rc;
    if (u) {
        std::vector<double> h(n * d.D);
        if ((rc = ens_fetch(h.data(), (const double *)d.u, W * d.D, units, stride))) return rc;
        for (size_t i = 0; i < n; ++i) {
            for (int c = 0; c < d.DT; ++c) u[i * d.DT + c] = 0.5;
            for (int k = 0; k < d.D; ++k) u[i * d.DT + e->fm[k]] = h[i * d.D + k];
        }
    }
    if (theta && (rc = ens_fetch(theta, (const double *)d.theta, W * d.DT, units, stride))) return rc;
    if (lnL && (rc = ens_fetch(lnL, (const double *)d.lnL, W, units, stride))) return rc;
    return NFA_OK;
}
static int ens_get_trace(nfa_ensemble *e, bool rungs, double *trace) {
    return ens_fetch(trace, (const double *)e->trace, (size_t)e->n_steps * (e->d.D + 1), rungs ? (size_t)e->d.P : (size_t)e->n_pix,
                     rungs ? 1 : (size_t)e->d.T);
}
extern "C" {

int nfa_ensemble_destroy(nfa_ensemble *e) {
    if (!e) return NFA_OK;
    ens_free(e->run_bufs);
    ens_free(e->bufs);
    delete e;
    return NFA_OK;
}

int64_t nfa_ensemble_bytes(int64_t n_pix, int n_walkers, int ndim, int n_sampled, int64_t n_steps, int64_t n_keep) {
    if (n_pix < 0 || n_walkers < 0 || ndim < 0 || n_sampled < 0 || n_steps < 0 || n_keep < 0) return -1;
    return ens_bytes(n_pix, n_walkers, ndim, n_sampled, n_steps, n_keep).total;
}

// behind both creators: n_temps = 1 and no betas for an untempered ensemble, whose units are its pixels
static int ens_create(nfa_ensemble **out, nfa_runner *r, const int32_t *pix, int64_t n_pix, int n_walkers, const double *betas,
                      int n_temps, int64_t swap_every, const int32_t *free_mask, const double *u0) {
    if (!out || !r || !u0) return fail(NFA_ERR_ARG, "null argument");
    if (!r->pr) return fail(NFA_ERR_STATE, "runner has no priors (predict-only)");
    if (n_pix < 1 || n_pix > (1 << 24)) return fail(NFA_ERR_ARG, "n_pix out of range");
    if (r->ndim > NS_MAXD) return fail(NFA_ERR_ARG, "too many dimensions");
    int rc = check_pix(r, pix, n_pix); if (rc) return rc;
    std::vector<int> fm;
    for (int j = 0; j < r->ndim; ++j) if (!free_mask || free_mask[j]) fm.push_back(j);
    if (fm.empty()) return fail(NFA_ERR_ARG, "no free dimension to sample");
    const int D = (int)fm.size(), DT = r->ndim, W = n_walkers;
    if (const char *why = ens_check_walkers(W, D)) return fail(NFA_ERR_ARG, why);
    // the start: u of the sampled slots, and the full rows with 0.5 elsewhere
    const size_t n = (size_t)n_pix * (size_t)n_temps * (size_t)W;
    std::vector<double> u(n * D), rows(n * DT, 0.5);
    for (size_t i = 0; i < n; ++i)
        for (int d = 0; d < D; ++d) {
            const double v = u0[i * DT + fm[d]];
            if (!(v > 0.0 && v < 1.0)) return fail(NFA_ERR_ARG, "ensemble: u0 must lie inside (0, 1) at every sampled slot");
            u[i * D + d] = v; rows[i * DT + fm[d]] = v;
        }
    rc = engine_init(); if (rc) return rc;
    nfa_ensemble *e = new nfa_ensemble();
    e->r = r; e->fm = fm; e->has_pix = pix != nullptr;
    e->n_pix = n_pix; e->d.T = n_temps; e->swap_every = swap_every;
    if (betas) e->h_betas.assign(betas, betas + n_temps);
    e->d.P = (int)(n_pix * n_temps); e->d.W = W; e->d.D = D; e->d.DT = DT;
    {
        RUNNER_LOCK(r);
        rc = sync_all_lanes(r);
        if (!rc) rc = ens_create_on_device(e, pix, u, rows);
    }
    if (rc) { const std::string why = g_err; nfa_ensemble_destroy(e); g_err = why; return rc; }
    *out = e;
    return NFA_OK;
}

int nfa_ensemble_create(nfa_ensemble **out, nfa_runner *r, const int32_t *pix, int64_t n_pix, int n_walkers,
                        const int32_t *free_mask, const double *u0) {
    return ens_create(out, r, pix, n_pix, n_walkers, nullptr, 1, 0, free_mask, u0);
}

int nfa_ensemble_create_tempered(nfa_ensemble **out, nfa_runner *r, const int32_t *pix, int64_t n_pix, int n_walkers,
                                 const double *betas, int n_temps, int64_t swap_every, const int32_t *free_mask, const double *u0) {
    if (const char *why = ens_check_betas(betas, n_temps)) return fail(NFA_ERR_ARG, why);
    if (const char *why = ens_check_swap_every(swap_every)) return fail(NFA_ERR_ARG, why);
    return ens_create(out, r, pix, n_pix, n_walkers, betas, n_temps, swap_every, free_mask, u0);
}

int64_t nfa_ensemble_tempered_bytes(int64_t n_pix, int n_walkers, int n_temps, int ndim, int n_sampled, int64_t n_steps, int64_t n_keep) {
    if (n_pix < 0 || n_walkers < 0 || n_temps < 1 || ndim < 0 || n_sampled < 0 || n_steps < 0 || n_keep < 0) return -1;
    return ens_tempered_bytes(n_pix, n_walkers, n_temps, ndim, n_sampled, n_steps, n_keep).total;
}

int nfa_ensemble_run(nfa_ensemble *e, int64_t n_steps, int64_t n_burn, int64_t thin, double a, int64_t seed, double log_zero) {
    if (!e) return fail(NFA_ERR_ARG, "null ensemble");
    if (const char *why = ens_check_run(n_steps, n_burn, thin, a)) return fail(NFA_ERR_ARG, why);
    nfa_runner *r = e->r;
    EnsDev &d = e->d;
    const int64_t P = d.P, NP = e->n_pix, W = d.W, half = W / 2, n_keep = ens_n_keep(n_steps, n_burn, thin);
    const bool tempered = ens_tempered(e);
    RUNNER_LOCK(r);
    int rc = sync_all_lanes(r); if (rc) return rc;
    // chain and trace of the run before go, this run's come: the cold chain of the pixels, the trace (and lnL) of every unit
    ens_free(e->run_bufs);
    e->chain_theta = e->chain_lnL = e->trace = e->rung_lnL = nullptr; e->n_keep = e->n_steps = 0;
    if ((rc = ens_alloc(e->run_bufs, &e->chain_theta, (size_t)(NP * n_keep * W * d.DT))) ||
        (rc = ens_alloc(e->run_bufs, &e->chain_lnL, (size_t)(NP * n_keep * W))) ||
        (rc = ens_alloc(e->run_bufs, &e->trace, (size_t)(P * n_steps * (d.D + 1)))) ||
        (tempered && (rc = ens_alloc(e->run_bufs, &e->rung_lnL, (size_t)(P * n_keep * W))))) {
        const std::string why = g_err; ens_free(e->run_bufs); e->chain_theta = e->chain_lnL = e->trace = e->rung_lnL = nullptr; g_err = why;
        return rc;
    }
    hipStream_t st = r->lanes[0];
    const EnsGeom Gw = ens_walk_geom(P, (int)W), Gt = ens_trace_geom(P), Gk = ens_keep_geom(P, (int)W, d.DT);
    auto steps = [&]() -> int {
        HIP_TRY(hipMemsetAsync(d.counts, 0, sizeof(long) * P * 3, st));
        if (tempered) HIP_TRY(hipMemsetAsync(d.swaps, 0, sizeof(long) * NP * (d.T - 1) * 2, st));
        int64_t sweep = 0;
        hipLaunchKernelGGL(ns_sanitize_kernel, dim3((unsigned)((P * W + 255) / 256)), dim3(256), 0, st, d.lnL, (long)(P * W), log_zero);
        HIP_TRY(hipGetLastError());
        for (int64_t s = 1; s <= n_steps; ++s) {
            for (int h = 0; h < 2; ++h) {
                hipLaunchKernelGGL(ens_propose_kernel, dim3(Gw.grid), dim3(Gw.threads), 0, st, d, (long)s, h, a, (uint64_t)seed);
                HIP_TRY(hipGetLastError());
                int rcb = ens_evaluate(r, d.row_pix, d.rows, d.row_lnL, P * half);
                if (rcb) return rcb;
                hipLaunchKernelGGL(ens_accept_kernel, dim3(Gw.grid), dim3(Gw.threads), 0, st, d, (long)s, h, a, (uint64_t)seed);
                HIP_TRY(hipGetLastError());
            }
            if (tempered && ens_swaps(s, e->swap_every)) {
                const int parity = ens_swap_parity(sweep++);
                const EnsGeom Gs = ens_swap_geom(NP, (int)W, d.T, parity);
                if (Gs.grid > 0) {
                    hipLaunchKernelGGL(ens_swap_kernel, dim3(Gs.grid), dim3(Gs.threads), 0, st, d, (long)s, parity, ens_swap_pairs(d.T, parity),
                                       (uint64_t)seed);
                    HIP_TRY(hipGetLastError());
                }
            }
            hipLaunchKernelGGL(ens_trace_kernel, dim3(Gt.grid), dim3(Gt.threads), 0, st, d, (long)s, (long)n_steps, e->trace);
            HIP_TRY(hipGetLastError());
            if (ens_keeps(s, n_burn, thin)) {
                hipLaunchKernelGGL(ens_keep_kernel, dim3(Gk.grid), dim3(Gk.threads), 0, st, d, (long)ens_keep_slot(s, n_burn, thin),
                                   (long)n_keep, e->chain_theta, e->chain_lnL, e->rung_lnL);
                HIP_TRY(hipGetLastError());
            }
        }
        HIP_TRY(hipStreamSynchronize(st));
        return NFA_OK;
    };
    rc = steps();
    if (rc) return ens_abandon(r, rc);
    r->lane_busy &= ~1u;
    e->n_keep = n_keep; e->n_steps = n_steps;
    return NFA_OK;
}

#define ENS_NEED_TEMPERED(e) do { if (!ens_tempered(e)) return fail(NFA_ERR_ARG, "ensemble: not a tempered ensemble"); } while (0)

int nfa_ensemble_counts(nfa_ensemble *e, int64_t *accepted, int64_t *outside, int64_t *evaluated) {
    if (!e || !accepted || !outside || !evaluated) return fail(NFA_ERR_ARG, "null argument");
    RUNNER_LOCK(e->r);
    return ens_get_counts(e, false, accepted, outside, evaluated);
}

int nfa_ensemble_rung_counts(nfa_ensemble *e, int64_t *accepted, int64_t *outside, int64_t *evaluated, int64_t *swaps_accepted,
                             int64_t *swaps_proposed) {
    if (!e || !accepted || !outside || !evaluated || !swaps_accepted || !swaps_proposed) return fail(NFA_ERR_ARG, "null argument");
    ENS_NEED_TEMPERED(e);
    RUNNER_LOCK(e->r);
    int rc = ens_get_counts(e, true, accepted, outside, evaluated); if (rc) return rc;
    const size_t n = (size_t)e->n_pix * (e->d.T - 1);
    std::vector<long> h(n * 2);
    HIP_TRY(hipMemcpy(h.data(), e->d.swaps, sizeof(long) * h.size(), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) { swaps_accepted[i] = h[2 * i]; swaps_proposed[i] = h[2 * i + 1]; }
    return NFA_OK;
}

int nfa_ensemble_state(nfa_ensemble *e, double *u, double *theta, double *lnL) {
    if (!e) return fail(NFA_ERR_ARG, "null ensemble");
    RUNNER_LOCK(e->r);
    return ens_get_state(e, false, u, theta, lnL);
}

int nfa_ensemble_rung_state(nfa_ensemble *e, double *u, double *theta, double *lnL) {
    if (!e) return fail(NFA_ERR_ARG, "null ensemble");
    ENS_NEED_TEMPERED(e);
    RUNNER_LOCK(e->r);
    return ens_get_state(e, true, u, theta, lnL);
}

int nfa_ensemble_trace(nfa_ensemble *e, double *trace) {
    if (!e || !trace) return fail(NFA_ERR_ARG, "null argument");
    if (!e->trace) return fail(NFA_ERR_STATE, "ensemble: no run yet");
    RUNNER_LOCK(e->r);
    return ens_get_trace(e, false, trace);
}

int nfa_ensemble_rung_trace(nfa_ensemble *e, double *trace) {
    if (!e || !trace) return fail(NFA_ERR_ARG, "null argument");
    ENS_NEED_TEMPERED(e);
    if (!e->trace) return fail(NFA_ERR_STATE, "ensemble: no run yet");
    RUNNER_LOCK(e->r);
    return ens_get_trace(e, true, trace);
}

int nfa_ensemble_rung_lnl(nfa_ensemble *e, double *lnL) {
    if (!e || !lnL) return fail(NFA_ERR_ARG, "null argument");
    ENS_NEED_TEMPERED(e);
    if (!e->rung_lnL) return fail(NFA_ERR_STATE, "ensemble: no run yet");
    RUNNER_LOCK(e->r);
    HIP_TRY(hipMemcpy(lnL, e->rung_lnL, sizeof(double) * (size_t)e->d.P * e->n_keep * e->d.W, hipMemcpyDeviceToHost));
    return NFA_OK;
}

// The evidence reduction of the head of nfa_ensemble_plan.h over the last run's rung lnL: out[n_pix][T][n_blocks + 1][3].
int nfa_ensemble_evidence(nfa_ensemble *e, int n_blocks, double *out) {
    if (!e || !out) return fail(NFA_ERR_ARG, "null argument");
    ENS_NEED_TEMPERED(e);
    if (!e->rung_lnL) return fail(NFA_ERR_STATE, "ensemble: no run yet");
    if (const char *why = ens_check_blocks(n_blocks, e->n_keep)) return fail(NFA_ERR_ARG, why);
    const EnsDev &d = e->d;
    nfa_runner *r = e->r;
    RUNNER_LOCK(r);
    int rc = sync_all_lanes(r); if (rc) return rc;
    hipStream_t st = r->lanes[0];
    const EnsGeom G = ens_evidence_geom(e->n_pix, d.T);
    auto work = [&]() -> int {
        hipLaunchKernelGGL(ens_evidence_kernel, dim3(G.grid), dim3(G.threads), 0, st, (const double *)e->rung_lnL, d.betas, d.T,
                           (long)e->n_keep, d.W, n_blocks, e->d_evid);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out, e->d_evid, sizeof(double) * (size_t)d.P * (n_blocks + 1) * 3, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return NFA_OK;
    };
    rc = work();
    if (rc) return ens_abandon(r, rc);
    return NFA_OK;
}

int nfa_ensemble_chain(nfa_ensemble *e, double *theta, double *lnL) {
    if (!e) return fail(NFA_ERR_ARG, "null ensemble");
    if (!e->chain_theta) return fail(NFA_ERR_STATE, "ensemble: no run yet");
    RUNNER_LOCK(e->r);
    const size_t n = (size_t)e->n_pix * e->n_keep * e->d.W;
    if (theta) HIP_TRY(hipMemcpy(theta, e->chain_theta, sizeof(double) * n * e->d.DT, hipMemcpyDeviceToHost));
    if (lnL) HIP_TRY(hipMemcpy(lnL, e->chain_lnL, sizeof(double) * n, hipMemcpyDeviceToHost));
    return NFA_OK;
}

int nfa_ensemble_chain_dev(nfa_ensemble *e, const double **d_theta, const double **d_lnL, int64_t *n_keep) {
    if (!e) return fail(NFA_ERR_ARG, "null ensemble");
    if (!e->chain_theta) return fail(NFA_ERR_STATE, "ensemble: no run yet");
    if (d_theta) *d_theta = e->chain_theta;
    if (d_lnL) *d_lnL = e->chain_lnL;
    if (n_keep) *n_keep = e->n_keep;
    return NFA_OK;
}

int nfa_ensemble_summary(nfa_ensemble *e, const double *levels, int n_levels, double *summary, double *best, double *quant) {
    if (!e) return fail(NFA_ERR_ARG, "null ensemble");
    if (!e->chain_theta) return fail(NFA_ERR_STATE, "ensemble: no run yet");
    const EnsDev &d = e->d;
    const int64_t N = e->n_keep * d.W;
    if (const char *why = ens_check_levels(levels, n_levels, N)) return fail(NFA_ERR_ARG, why);
    if (n_levels > 0 && !quant) return fail(NFA_ERR_ARG, "ensemble: quantile levels without a place for the quantiles");
    nfa_runner *r = e->r;
    RUNNER_LOCK(r);
    int rc = sync_all_lanes(r); if (rc) return rc;
    hipStream_t st = r->lanes[0];
    const EnsGeom G = ens_summary_geom(e->n_pix, N, n_levels);
    rc = ensure_dynamic_lds((const void *)ens_summary_kernel, G.lds); if (rc) return rc;
    auto work = [&]() -> int {
        if (n_levels > 0) HIP_TRY(hipMemcpyAsync(e->d_levels, levels, sizeof(double) * n_levels, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(ens_summary_kernel, dim3(G.grid), dim3(G.threads), G.lds, st, (const double *)e->chain_theta,
                           (const double *)e->chain_lnL, (long)N, d.DT, (const double *)e->d_levels, n_levels,
                           (long)ens_sort_len(N, n_levels), e->d_summary, e->d_best, e->d_quant);
        HIP_TRY(hipGetLastError());
        const size_t P = (size_t)e->n_pix, DT = (size_t)d.DT;
        if (summary) HIP_TRY(hipMemcpyAsync(summary, e->d_summary, sizeof(double) * P * DT * 2, hipMemcpyDeviceToHost, st));
        if (best) HIP_TRY(hipMemcpyAsync(best, e->d_best, sizeof(double) * P * (DT + 1), hipMemcpyDeviceToHost, st));
        if (n_levels > 0) HIP_TRY(hipMemcpyAsync(quant, e->d_quant, sizeof(double) * P * DT * n_levels, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return NFA_OK;
    };
    rc = work();
    if (rc) return ens_abandon(r, rc);
    return NFA_OK;
}

int nfa_ensemble_histogram(nfa_ensemble *e, const double *edges, int n_bins, int64_t *counts, int64_t *outside) {
    if (!e || !counts) return fail(NFA_ERR_ARG, "null argument");
    if (!e->chain_theta) return fail(NFA_ERR_STATE, "ensemble: no run yet");
    const EnsDev &d = e->d;
    const int64_t N = e->n_keep * d.W, P = e->n_pix, DT = d.DT;
    if (const char *why = ens_check_edges(edges, d.DT, n_bins, N)) return fail(NFA_ERR_ARG, why);
    nfa_runner *r = e->r;
    RUNNER_LOCK(r);
    int rc = sync_all_lanes(r); if (rc) return ens_abandon(r, rc);
    hipStream_t st = r->lanes[0];
    const int64_t slab = std::min(P, ens_slab_pixels(ens_hist_pixel_bytes(d.DT, n_bins)));
    std::vector<void *> took;
    double *d_edges = nullptr;
    long *d_counts = nullptr, *d_out = nullptr;
    std::vector<int64_t> h_out(outside ? 0 : (size_t)(slab * DT));        // (the copy out needs a place either way)
    auto work = [&]() -> int {
        int rcw;
        if ((rcw = ens_alloc(took, &d_edges, (size_t)(DT * (n_bins + 1)))) || (rcw = ens_alloc(took, &d_counts, (size_t)(slab * DT * n_bins))) ||
            (rcw = ens_alloc(took, &d_out, (size_t)(slab * DT))))
            return rcw;
        HIP_TRY(hipMemcpyAsync(d_edges, edges, sizeof(double) * DT * (n_bins + 1), hipMemcpyHostToDevice, st));
        for (int64_t p0 = 0; p0 < P; p0 += slab) {
            const int64_t np = std::min(slab, P - p0);
            const EnsGeom G = ens_hist_geom(np, d.DT, N, n_bins);
            hipLaunchKernelGGL(ens_hist_kernel, dim3(G.grid), dim3(G.threads), G.lds, st, (const double *)e->chain_theta + p0 * N * DT, (long)N,
                               d.DT, (const double *)d_edges, n_bins, d_counts, d_out);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(counts + p0 * DT * n_bins, d_counts, sizeof(long) * np * DT * n_bins, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(outside ? outside + p0 * DT : h_out.data(), d_out, sizeof(long) * np * DT, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));                 // the slab's scratch is free for the next one
        }
        return NFA_OK;
    };
    rc = work();
    if (rc) rc = ens_abandon(r, rc);
    ens_free(took);
    return rc;
}

int nfa_ensemble_covariance(nfa_ensemble *e, double *cov) {
    if (!e || !cov) return fail(NFA_ERR_ARG, "null argument");
    if (!e->chain_theta) return fail(NFA_ERR_STATE, "ensemble: no run yet");
    const EnsDev &d = e->d;
    const int64_t N = e->n_keep * d.W, P = e->n_pix, DT = d.DT;
    nfa_runner *r = e->r;
    RUNNER_LOCK(r);
    int rc = sync_all_lanes(r); if (rc) return ens_abandon(r, rc);
    hipStream_t st = r->lanes[0];
    const int64_t slab = std::min(P, ens_slab_pixels(ens_cov_pixel_bytes(d.DT)));
    std::vector<void *> took;
    double *d_cov = nullptr;
    auto work = [&]() -> int {
        int rcw = ens_alloc(took, &d_cov, (size_t)(slab * DT * DT)); if (rcw) return rcw;
        for (int64_t p0 = 0; p0 < P; p0 += slab) {
            const int64_t np = std::min(slab, P - p0);
            const EnsGeom G = ens_cov_geom(np, N);
            hipLaunchKernelGGL(ens_cov_kernel, dim3(G.grid), dim3(G.threads), 0, st, (const double *)e->chain_theta + p0 * N * DT,
                               (const double *)e->chain_lnL + p0 * N, (long)N, d.DT, d_cov);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(cov + p0 * DT * DT, d_cov, sizeof(double) * np * DT * DT, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        return NFA_OK;
    };
    rc = work();
    if (rc) rc = ens_abandon(r, rc);
    ens_free(took);
    return rc;
}

int nfa_ensemble_moments(nfa_ensemble *e, int64_t chunk_rows, double *spec_mean, double *spec_std, double *stat_mean, double *stat_std) {
    if (!e) return fail(NFA_ERR_ARG, "null ensemble");
    if (!e->chain_theta) return fail(NFA_ERR_STATE, "ensemble: no run yet");
    if (!spec_mean && !spec_std && !stat_mean && !stat_std) return fail(NFA_ERR_ARG, "predict_moments: all four outputs are null");
    if (const char *why = mom_check_chunk_rows(chunk_rows)) return fail(NFA_ERR_ARG, why);
    const int64_t N = e->n_keep * e->d.W, P = e->n_pix;
    // nfa_runner_predict_moments' arguments: a segment of N rows per pixel, equal weights, so S0 = N
    std::vector<int64_t> seg_off((size_t)P + 1);
    for (int64_t g = 0; g <= P; ++g) seg_off[(size_t)g] = g * N;
    const std::vector<double> s0((size_t)P, (double)N);
    nfa_runner *r = e->r;
    RUNNER_LOCK(r);
    int rc = sync_all_lanes(r);
    if (!rc) rc = mom_reduce(r, P, e->has_pix ? e->h_pix.data() : nullptr, seg_off.data(), MomRows{nullptr, e->chain_theta, nullptr}, nullptr,
                             s0.data(), mom_chunk_rows(chunk_rows), spec_mean, spec_std, stat_mean, stat_std);
    if (rc) return ens_abandon(r, rc);
    return NFA_OK;
}

int64_t nfa_ensemble_moments_bytes(int64_t n_pix, int64_t chan_tot, int n_spec) {
    if (n_pix < 0 || chan_tot < 0 || n_spec < 0) return -1;
    return ens_moments_bytes(n_pix, chan_tot, n_spec);
}

}  // extern "C"
