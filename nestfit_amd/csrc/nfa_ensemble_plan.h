// nfa_ensemble_plan.h -- the ensemble sampler (nfa_ensemble_*, nfa_ensemble.h), planned on the host: its limits and the
// tag of its random streams, the checks of its arguments, which steps are kept, the bytes a run holds on the device, the
// launch geometries and the LDS of the summary, and the same for the products of a chain (histogram, covariance, moments).
//
// Standard C++17 without a HIP include, like nfa_lsq_plan.h and nfa_moments_plan.h: a host compiler builds this header
// alone, and tests/test_ensemble_cpu.py checks it without a GPU.  Arithmetic only.  Errors travel as `const char *`, in
// the words the engine fails with.
//
// The contract (include/nestfit_amd.h and DESIGN 4.24 say the same).  A run holds P pixels with W walkers each, W even,
// W / 2 >= D + 1, in the D sampled slots of the unit cube.  One step is two half-steps h = 0, 1; in half-step h the
// walkers k of [h W/2, (h+1) W/2) move against the other half as it stands.  With p the pixel's cube index, s the step
// (from 1 in every run) and r_i = ns_uniform_of(ns_stream(seed, p, NFA_ENS_TAG + 2 s + h), 3 k + i):
//     partner  j = other half's base + min(floor(r_0 W/2), W/2 - 1)
//     stretch  z = ((a - 1) r_1 + 1)^2 / a
//     proposal y_d = u_j,d + z (u_k,d - u_j,d)                     (inside: every y_d in (0, 1))
//     accept   inside, lnL_y finite, and log(r_2) < (D - 1) log(z) + (lnL_y - lnL_k)
// The state after step s is kept iff s > n_burn and (s - n_burn) % thin == 0.
//
// The products of the last run's chain; a pixel has N = n_keep W samples in (keep, walker) order.
//     histogram   column c on edges[c][0 .. n_bins], strictly increasing and finite: bin b counts edges[b] <= x < edges[b + 1],
//                 the last bin x == edges[n_bins] too; a NaN and an x beyond the edges count as outside and in no bin
//                 (np.histogram of an edge array)
//     covariance  about the best row b of the summary: d_i,a = x_i,a - x_b,a, S_a = sum d_i,a, S_ab = sum d_i,a d_i,b,
//                 cov_ab = S_ab / N - (S_a / N)(S_b / N) for a <= b, mirrored; the diagonal not below 0
//     moments     nfa_runner_predict_moments over the chain where it lies: a segment per pixel, equal weights
//
// A tempered ensemble holds T = n_temps rungs per pixel, 2 <= T <= NFA_ENS_MAX_TEMPS, at inverse temperatures
// 1 = beta_0 > beta_1 > .. > beta_T-1 >= 0, W walkers each.  A (pixel, rung) unit moves like a pixel above with two changes:
//     stream   ns_stream(seed, p, NFA_ENS_TAG + t 2^48 + 2 s + h)
//     accept   log(r_2) < (D - 1) log(z) + beta_t (lnL_y - lnL_k), the product formed last; beta_0 = 1 multiplies exactly, so
//              rung 0 of a run that never swaps has the bits of the untempered run (which is T = 1, beta = 1)
// Outside proposals and a lnL_y that is not finite are rejected at every beta, 0 included.  After the two half-steps of step
// s, if swap_every > 0 and s % swap_every == 0, with n the number of swap sweeps before in this run: the pairs (t, t + 1) with
// t % 2 == n % 2 exchange walker k for walker k (u, theta, lnL) iff
//     log(r) < (beta_t - beta_t+1) (lnL_t+1,k - lnL_t,k),   r = ns_uniform_of(ns_stream(seed, p, NFA_ENS_SWAP_TAG + t 2^48 + s), k)
// before the trace and the keep of the step.  Kept: the theta chain of rung 0 in the layout above (summary, histogram,
// covariance, moments, chain, counts, state and trace describe the cold chain), lnL of every rung [P][T][n_keep][W], the trace
// of every rung [P][T][n_steps][D + 1]; counters per (pixel, rung) and per (pixel, pair): swaps accepted, proposed.
// The evidence reduction, per (pixel, rung t, set j) over the kept lnL x_i: set 0 is all n_keep kept steps, sets 1 .. B are
// contiguous blocks of floor(n_keep / B) kept steps, 1 <= B <= NFA_ENS_MAX_BLOCKS, B <= n_keep.  With d_i = x_i - x_first:
//     mean = x_first + S1 / n,  var = max(S2 / n - (S1 / n)^2, 0),
//     r    = delta M + log(sum exp(delta (x_i - M)) / n),  delta = beta_t-1 - beta_t, M = max x_i     (t = 0: r = 0)
// out[P][T][B + 1][3]; with beta_T-1 = 0 the sum over t of r is ln Z (stepping stones: Z_beta_t-1 / Z_beta_t = E_beta_t[L^delta]).
#pragma once

#include <cstddef>
#include <cstdint>

#ifdef __HIP__
#define ENS_HD __host__ __device__          // what the kernels of nfa_ensemble.h call too
#else
#define ENS_HD
#endif

#define NFA_ENS_MAX_WALKERS 512          // include/nestfit_amd.h says the same for these three
#define NFA_ENS_MAX_Q       8            // quantile levels of a summary
#define NFA_ENS_MAX_SORT    8192         // kept samples per pixel a summary sorts: 64 KB of LDS
#define NFA_ENS_MAX_BINS    1024         // bins of a histogram: its edges and counts are 8 KB + 4 KB of LDS
// The streams of a run: ns_stream(seed, pixel, NFA_ENS_TAG + 2 step + half).  The nested sampler's third stream argument
// is a count of proposals (below 2^61), NS_FRAME_SEED (2^31) or NS_TAG_LIVE + live point (2^62 ..); a run of 2^59 steps
// stays inside [2^61, 2^62).
#define NFA_ENS_TAG         (1ull << 61)
#define ENS_A_MAX           16.0         // the stretch scale: 1 < a <= 16
#define ENS_PIECE_ROWS      (1 << 20)    // rows of one likelihood launch at most; a larger half-step is cut into pieces
#define ENS_STEPS_MAX       (1ll << 40)
#define ENS_RED_DOUBLES     64           // head of the summary's LDS: the partial results of up to 16 waves, three arrays
#define ENS_SLAB_BYTES      (8 << 20)    // device scratch of a histogram or covariance call: the pixels go through it in slabs
#define ENS_SAMPLES_MAX     (1ll << 32)  // kept samples per pixel a histogram counts: its LDS counters are 32 bits wide
// A tempered ensemble.  Rung t moves on the tags NFA_ENS_TAG + t 2^48 + 2 s + h and swaps with rung t + 1 on NFA_ENS_SWAP_TAG
// + t 2^48 + s.  With s <= ENS_STEPS_MAX = 2^40 and t < 32 = 2^5: 2 s + h <= 2^41 + 1 < 2^48, so the rungs' tags do not meet,
// and t 2^48 + 2 s + h < 2^53 + 2^42; the largest move tag lies below 2^61 + 2^54 < 2^61 + 2^60, the smallest swap tag, and
// the largest swap tag below 2^61 + 2^60 + 2^54 < 2^62: all inside [2^61, 2^62), moves and swaps apart.
#define NFA_ENS_MAX_TEMPS   32           // include/nestfit_amd.h says the same for these two
#define NFA_ENS_MAX_BLOCKS  16           // blocks of an evidence's batch means
#define ENS_RUNG_SHIFT      48
#define NFA_ENS_SWAP_TAG    (NFA_ENS_TAG + (1ull << 60))
#define ENS_SWAP_THREADS_MAX 512         // = NFA_ENS_MAX_WALKERS: a thread per walker
#define ENS_EVID_THREADS    256

// ---- argument checks: null, or why the argument is refused
inline const char *ens_check_walkers(int n_walkers, int n_sampled) {
    if (n_walkers < 2 || n_walkers > NFA_ENS_MAX_WALKERS) return "ensemble: n_walkers must be in 2 .. NFA_ENS_MAX_WALKERS = 512";
    if (n_walkers % 2 != 0) return "ensemble: n_walkers must be even: each half moves against the other";
    if (n_walkers / 2 < n_sampled + 1) return "ensemble: half the walkers must number the sampled dimensions + 1 at least";
    return nullptr;
}
inline int64_t ens_n_keep(int64_t n_steps, int64_t n_burn, int64_t thin) { return thin < 1 ? 0 : (n_steps - n_burn) / thin; }
inline bool ens_keeps(int64_t step, int64_t n_burn, int64_t thin) { return step > n_burn && (step - n_burn) % thin == 0; }
inline int64_t ens_keep_slot(int64_t step, int64_t n_burn, int64_t thin) { return (step - n_burn) / thin - 1; }
inline const char *ens_check_run(int64_t n_steps, int64_t n_burn, int64_t thin, double a) {
    if (!(a > 1.0 && a <= ENS_A_MAX)) return "ensemble: the stretch scale a must lie in (1, 16]";
    if (thin < 1) return "ensemble: thin must be 1 at least";
    if (n_steps < 1 || n_steps > ENS_STEPS_MAX) return "ensemble: n_steps is out of range";
    if (n_burn < 0 || n_burn >= n_steps) return "ensemble: n_burn must lie in 0 .. n_steps - 1";
    if (ens_n_keep(n_steps, n_burn, thin) < 1) return "ensemble: no step is kept: (n_steps - n_burn) / thin is 0";
    return nullptr;
}
// the quantile levels of a summary over n_samples = n_keep W kept samples per pixel
inline const char *ens_check_levels(const double *levels, int n_levels, int64_t n_samples) {
    if (n_levels < 0 || n_levels > NFA_ENS_MAX_Q) return "ensemble: a summary takes NFA_ENS_MAX_Q = 8 quantile levels at most";
    if (n_levels > 0 && !levels) return "ensemble: quantile levels are counted but not given";
    for (int i = 0; i < n_levels; ++i)
        if (!(levels[i] >= 0.0 && levels[i] <= 1.0)) return "ensemble: a quantile level lies outside [0, 1]";
    if (n_levels > 0 && n_samples > NFA_ENS_MAX_SORT) return "ensemble: quantiles take NFA_ENS_MAX_SORT = 8192 kept samples per pixel at most";
    return nullptr;
}
// the edges[ndim][n_bins + 1] of a histogram over n_samples kept samples per pixel
inline const char *ens_check_edges(const double *edges, int ndim, int n_bins, int64_t n_samples = 0) {
    if (n_bins < 1 || n_bins > NFA_ENS_MAX_BINS) return "ensemble: a histogram takes 1 .. NFA_ENS_MAX_BINS = 1024 bins";
    if (!edges) return "ensemble: bins are counted but their edges are not given";
    for (int c = 0; c < ndim; ++c) {
        const double *e = edges + (size_t)c * (size_t)(n_bins + 1);
        for (int b = 0; b <= n_bins; ++b) {
            if (!(e[b] - e[b] == 0.0)) return "ensemble: a bin edge is not finite";
            if (b > 0 && !(e[b] > e[b - 1])) return "ensemble: the bin edges of a parameter must increase strictly";
        }
    }
    if (n_samples >= ENS_SAMPLES_MAX) return "ensemble: a histogram counts fewer than 2^32 kept samples per pixel";
    return nullptr;
}
// the ladder betas[n_temps] of a tempered ensemble
inline const char *ens_check_betas(const double *betas, int n_temps) {
    if (n_temps < 2 || n_temps > NFA_ENS_MAX_TEMPS) return "ensemble: a tempered ensemble takes 2 .. NFA_ENS_MAX_TEMPS = 32 rungs";
    if (!betas) return "ensemble: rungs are counted but their betas are not given";
    for (int t = 0; t < n_temps; ++t)
        if (!(betas[t] - betas[t] == 0.0)) return "ensemble: a beta is not finite";
    if (betas[0] != 1.0) return "ensemble: betas[0] must be 1: rung 0 is the cold chain";
    for (int t = 1; t < n_temps; ++t)
        if (!(betas[t] < betas[t - 1])) return "ensemble: the betas must decrease strictly";
    if (betas[n_temps - 1] < 0.0) return "ensemble: the last beta must not be negative";
    return nullptr;
}
inline const char *ens_check_swap_every(int64_t swap_every) {
    return swap_every < 0 ? "ensemble: swap_every must be 0 (never) or a number of steps" : nullptr;
}
// the blocks of an evidence over n_keep kept steps
inline const char *ens_check_blocks(int n_blocks, int64_t n_keep) {
    if (n_blocks < 1 || n_blocks > NFA_ENS_MAX_BLOCKS) return "ensemble: an evidence takes 1 .. NFA_ENS_MAX_BLOCKS = 16 blocks";
    if (n_blocks > n_keep) return "ensemble: an evidence takes no more blocks than kept steps";
    return nullptr;
}
// ---- swaps: whether step s ends with a sweep; sweep n (from 0 in every run) exchanges the pairs (t, t + 1) with t % 2 == n % 2
inline bool ens_swaps(int64_t step, int64_t swap_every) { return swap_every > 0 && step % swap_every == 0; }
inline int ens_swap_parity(int64_t sweep) { return (int)(sweep & 1); }
inline int ens_swap_pairs(int n_temps, int parity) { return (n_temps - parity) / 2; }      // t = parity, parity + 2, .. <= T - 2
ENS_HD inline uint64_t ens_move_tag(int rung, int64_t step, int h) { return NFA_ENS_TAG + ((uint64_t)rung << ENS_RUNG_SHIFT) + 2ull * (uint64_t)step + (uint64_t)h; }
ENS_HD inline uint64_t ens_swap_tag(int rung, int64_t step) { return NFA_ENS_SWAP_TAG + ((uint64_t)rung << ENS_RUNG_SHIFT) + (uint64_t)step; }
// ---- evidence: the kept steps [first, first + count) of set j of n_blocks blocks (set 0: all of them)
ENS_HD inline int64_t ens_set_steps(int64_t n_keep, int n_blocks, int j) { return j == 0 ? n_keep : n_keep / n_blocks; }
ENS_HD inline int64_t ens_set_first(int64_t n_keep, int n_blocks, int j) { return j == 0 ? 0 : (int64_t)(j - 1) * (n_keep / n_blocks); }

// ---- device bytes of an ensemble of P pixels: what create allocates (state: the walkers, a half-step's proposal rows,
// the counters and the summary's outputs), and what a run of n_steps steps with n_keep kept adds (chain, trace)
struct EnsBytes { int64_t state, chain, trace, total; };
inline EnsBytes ens_bytes(int64_t P, int W, int ndim, int D, int64_t n_steps, int64_t n_keep) {
    const int64_t d = 8, i = 4, walkers = P * W, rows = P * (W / 2);
    EnsBytes B;
    B.state = walkers * (D + ndim + 1) * d + walkers * i           // u, theta, lnL; the pixel of every start row
            + rows * (ndim + D + 1) * d + rows * 2 * i             // a half-step: rows, y, lnL; pixel and inside flag
            + P * 3 * d + P * i + (int64_t)D * i                   // counters, pix, fmap
            + P * ((int64_t)ndim * 2 + (ndim + 1) + (int64_t)ndim * NFA_ENS_MAX_Q) * d + NFA_ENS_MAX_Q * d;    // summary, best, quant, levels
    B.chain = P * n_keep * W * (ndim + 1) * d;
    B.trace = P * n_steps * (D + 1) * d;
    B.total = B.state + B.chain + B.trace;
    return B;
}
// A tempered ensemble of P pixels and T rungs: the walkers, the half-step rows and the (pixel, rung) counters of P T units;
// the summary's outputs of P pixels; the ladder, the swap counters of P (T - 1) pairs and the evidence's output at its
// largest; the cold chain (theta and lnL of rung 0, the layout of an untempered chain) and lnL of every rung; the trace of
// every rung.
inline EnsBytes ens_tempered_bytes(int64_t P, int W, int T, int ndim, int D, int64_t n_steps, int64_t n_keep) {
    const int64_t d = 8, i = 4, units = P * T, walkers = units * W, rows = units * (W / 2);
    EnsBytes B;
    B.state = walkers * (D + ndim + 1) * d + walkers * i
            + rows * (ndim + D + 1) * d + rows * 2 * i
            + units * 3 * d + units * i + (int64_t)D * i
            + P * ((int64_t)ndim * 2 + (ndim + 1) + (int64_t)ndim * NFA_ENS_MAX_Q) * d + NFA_ENS_MAX_Q * d
            + T * d + P * (T - 1) * 2 * d + units * (NFA_ENS_MAX_BLOCKS + 1) * 3 * d;      // betas, swap counters, evidence
    B.chain = P * n_keep * W * (ndim + 1) * d + units * n_keep * W * d;
    B.trace = units * n_steps * (D + 1) * d;
    B.total = B.state + B.chain + B.trace;
    return B;
}
// A histogram and a covariance hold ENS_SLAB_BYTES of device scratch whatever the number of pixels (a lone pixel whose
// outputs are larger: that pixel's), for the length of the call: pixels [p0, p0 + ens_slab_pixels) go through it at a time.
// So ens_bytes has nothing to add for them.  The moments use the runner's scratch of nfa_runner_predict_moments, which
// does grow with the pixels: reference rows and two accumulator planes of chan_tot + 2 n_spec columns, and S0.
inline int64_t ens_slab_pixels(int64_t bytes_per_pixel) { return bytes_per_pixel >= ENS_SLAB_BYTES ? 1 : ENS_SLAB_BYTES / bytes_per_pixel; }
inline int64_t ens_hist_pixel_bytes(int ndim, int n_bins) { return (int64_t)ndim * (n_bins + 1) * 8; }     // counts and outside
inline int64_t ens_cov_pixel_bytes(int ndim) { return (int64_t)ndim * ndim * 8; }
inline int64_t ens_moments_bytes(int64_t P, int64_t chan_tot, int n_spec) { return P * (3 * (chan_tot + 2 * (int64_t)n_spec) + 1) * 8; }

// ---- launch geometries
struct EnsGeom { unsigned grid, threads; size_t lds; };
// propose and accept: a workgroup per pixel, a thread per walker of the moving half (whole waves: 64 .. 256 threads)
inline EnsGeom ens_walk_geom(int64_t P, int W) { return EnsGeom{(unsigned)P, (unsigned)((W / 2 + 63) / 64 * 64), 0}; }
// trace: one wave per pixel
inline EnsGeom ens_trace_geom(int64_t P) { return EnsGeom{(unsigned)P, 64u, 0}; }
// keep: a thread per double of the state's theta and lnL
inline EnsGeom ens_keep_geom(int64_t P, int W, int ndim) { return EnsGeom{(unsigned)((P * W * (ndim + 1) + 255) / 256), 256u, 0}; }
// summary: a workgroup per pixel.  With quantiles the n_samples of a parameter are sorted in LDS, padded to a power of two
// (bitonic); the head of the LDS holds the waves' partial results.
inline int64_t ens_pow2(int64_t n) { int64_t m = 1; while (m < n) m <<= 1; return m; }
inline int64_t ens_sort_len(int64_t n_samples, int n_levels) { return n_levels > 0 ? (ens_pow2(n_samples) < 2 ? 2 : ens_pow2(n_samples)) : 0; }
inline size_t ens_summary_lds(int64_t n_samples, int n_levels) {
    return sizeof(double) * (size_t)(ENS_RED_DOUBLES + ens_sort_len(n_samples, n_levels));
}
inline EnsGeom ens_summary_geom(int64_t P, int64_t n_samples, int n_levels) {
    int64_t t = ens_pow2(n_samples) / 2;                   // a thread per compare-exchange of a sorting stage, up to 1024
    t = t < 64 ? 64 : t > 1024 ? 1024 : t;
    return EnsGeom{(unsigned)P, (unsigned)t, ens_summary_lds(n_samples, n_levels)};
}
// histogram: a workgroup per (pixel, parameter), pixel-major; a thread per strided sample, whole waves up to four.  LDS:
// the parameter's n_bins + 1 edges, then n_bins + 1 32-bit counters (the last one counts outside).
inline unsigned ens_scan_threads(int64_t n_samples) {
    const int64_t t = (n_samples + 63) / 64 * 64;
    return (unsigned)(t < 64 ? 64 : t > 256 ? 256 : t);
}
inline size_t ens_hist_lds(int n_bins) { return (sizeof(double) + sizeof(uint32_t)) * (size_t)(n_bins + 1); }
inline EnsGeom ens_hist_geom(int64_t P, int ndim, int64_t n_samples, int n_bins) {
    return EnsGeom{(unsigned)(P * ndim), ens_scan_threads(n_samples), ens_hist_lds(n_bins)};
}
// covariance: a workgroup per pixel, the same threads; its LDS is static
inline EnsGeom ens_cov_geom(int64_t P, int64_t n_samples) { return EnsGeom{(unsigned)P, ens_scan_threads(n_samples), 0}; }
// A tempered ensemble's propose, accept, trace and keep take its P T units where the functions above take P pixels.
// swap: a workgroup per (pixel, active pair of the sweep), a thread per walker (whole waves: 64 .. 512 threads); grid 0 where
// the sweep has no pair (T = 2, an odd sweep): nothing is launched
inline EnsGeom ens_swap_geom(int64_t P, int W, int n_temps, int parity) {
    return EnsGeom{(unsigned)(P * ens_swap_pairs(n_temps, parity)), (unsigned)((W + 63) / 64 * 64), 0};
}
// evidence: a workgroup per (pixel, rung); its LDS is static
inline EnsGeom ens_evidence_geom(int64_t P, int n_temps) { return EnsGeom{(unsigned)(P * n_temps), (unsigned)ENS_EVID_THREADS, 0}; }
