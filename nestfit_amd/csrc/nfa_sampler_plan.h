// nfa_sampler_plan.h -- what form a run of the device sampler takes, decided once on the host.
//
// Standard C++17 without a HIP include: a host compiler builds this header alone, so the decision can be tested on a
// machine without a GPU against the numpy twin's `_plan` (nestfit_amd/nested.py), which holds the same chain under the
// same field names.  It holds the policy defaults and limits the plan uses, the constants the kernels share with the
// twin, the knobs in one convention, and ns_plan.
#pragma once

#include <climits>
#include <cstddef>
#include <vector>

#ifdef __HIP__
#define NS_HD __host__ __device__
#else
#define NS_HD
#endif

// Several bounding ellipsoids per pixel (MultiNest's `mmodal` bound in its simplest form): up to NS_ME of them where at
// most NS_ME_MAXD dimensions are sampled.
#define NS_ME 4
#ifndef NS_ME_MAXD
#define NS_ME_MAXD 6
#endif
#define NS_STAGE_BYTES (96 * 1024) // a refit stages the centred live points in LDS when they fit in this much of it
#define NS_FRAMES 32               // rotated frames a caller gets who asks for boxes without naming a number
#define NS_FRAMES_MAX 64
#define NS_MARGIN_C 2.5            // (round 4: 1.75, sampler.py precision='speed')
#define NS_RATIO_MAX 32            // proposals drawn per round: at most this multiple of the evaluations aimed for
#ifndef NS_KMAX
#define NS_KMAX 65536              // most proposals one pixel gets in a round
#endif
#define NS_SHEAR_ENLARGE 3.0       // safety factor on the enclosing volume of the sheared ellipsoid (round 4: 2.5, sampler.py precision='speed')
#define NS_SHEAR_MMAX 64           // monomials at most
#define NS_REFIT_THREADS 512       // of the workgroup that fits a one-ellipsoid bound
#define NS_PAIRS_ENLARGE 2.0       // safety factor on the area of a pair ellipse (round 4: 1.75, sampler.py precision='speed')
// (a pixel starts with a small share and doubles it while its rounds accept little: started at the round's Kr, a run of
// two pixels drew 65 k proposals per pixel in its first round, where every second one is accepted, and halved from there)
#define NS_KP_START 256            // a pixel's share of proposals in its first rejection round
#define NS_K_TARGET 16             // replacements per pixel and rejection round the per-pixel share of proposals aims at
#define NS_REFIT_EVERY 4           // rejection-mode pixels refit in rounds that are multiples of this
// When does a pixel give up rejection sampling for constrained walks?  Measured on config 5 (profiles/r03/
// sweep_walk_factor.txt): with ten sampled dimensions the walks win from an acceptance of ~1 in 2 n_steps down (the
// run takes 7.0-7.2 s for factors 1..4, 8.6 s at 32, 10.9 s at 64); with five they hardly ever do -- a rejection
// round is one large batch, a walk cycle n_steps small ones, and the run goes from 1.16 s (factor 2) to 0.84 s (64;
// rejection only: 0.79 s).  The walks stay as the way out of a bound that has become hopeless.
#define NS_WALK_LOWD 6             // up to this many sampled dimensions ...
#define NS_WALK_FACTOR_LOWD 64     // ... the switch to walks waits for an acceptance below 1 / (64 n_steps)
#define NS_WALK_FACTOR 2           // above: 1 / (2 n_steps)

// What the kernels share with the numpy twin beside the plan (nestfit_amd/nested.py holds every NS_X below as _NS_X;
// tests/test_sampler_plan.py compares them): the random stream's slots, the walk's target, the bound-fitting constants.
#define NS_TAG_LIVE  (1ull << 62)
#define NS_B_RADIUS  255ull
#define NS_B_START   250ull      // stream index of a walker's starting live point
#define NS_WALK_TARGET 0.5     // acceptance the walk scale is tuned to
// Several ellipsoids: a cluster of live points is cut in two across its principal axis at its
// centre; the cut is kept when the two halves' ellipsoids together have less than NS_ME_GAIN of the parent's volume.
#define NS_ME_GAIN 0.7
#define NS_B_ELL 253ull            // random-stream slots of a proposal: which ellipsoid, and the 1 / (number that hold it) test
#define NS_B_KEEP 254ull
// Free rejections of a one-ellipsoid bound: a proposal outside the bounding box of the live points -- in the unit cube's
// axes, in the ellipsoid's own (Cholesky) frame, or in one of NS_FRAMES fixed rotations of that frame -- is dropped before
// its likelihood is evaluated.  Every box holds the live region, so what passes is uniform over the intersection.  A face
// lies beyond the extreme live point by c max(0.1 s, extreme - mean - 1.5 s), s = the spread along the face's direction:
// small where the marginal ends abruptly (a flat direction), large where it thins out (the projection of a round body).
// scripts/proto_intersection.py measured what each family of bounds cuts off the true region and what it saves; the
// numpy twin's _fit_boxes / _box_veto hold the same arithmetic.
#define NS_MARGIN_A 1.5
#define NS_MARGIN_FLOOR 0.1
#define NS_FRAME_SEED 0x5EEDF00Dull
// A volume-preserving shear in front of the one-ellipsoid bound (the twin's _fit_shear): every sampled coordinate minus a
// quadratic function of the earlier ones -- the curved tex / ntot ridges of faint pixels come out straight, and an
// ellipsoid around straight things is small
#define NS_SHEAR_RIDGE 1e-6        // on the Gram matrix's diagonal, times the live points
#define NS_SHEAR_PIVOT 1e-9        // a Cholesky pivot below this fraction of its diagonal entry: the monomial is dropped

// Walkers of a pixel with n live points: a cycle's walkers are harvested against a threshold that rises with every
// replacement, so many more than a third of n mostly harvest each other's leftovers (of k walkers n ln(1 + k / n) pass);
// 64 of them are a small batch once the pixels are few -- 128 from 384 live points, 256 from 768.
NS_HD inline int ns_walkers_for(int n) { return n >= 768 ? 256 : n >= 384 ? 128 : 64; }

// One fit slot of the several-ellipsoids refit in LDS: [c: D][L: D*D, lower][cov: D*D, lower][r2, lnv, n, final]
NS_HD inline int ns_me_slot(int D) { return D + 2 * D * D + 4; }

#define NS_UPD_THREADS 256
#define NS_UPD_SEG (4 * NS_UPD_THREADS)
NS_HD inline size_t ns_upd_lds(int N) {   // doubles: live lnL | survivors' lnL | their k, row, rank (ints) | counts | control
    return (size_t)((N + 1) & ~1) + NS_UPD_SEG + (3 * NS_UPD_SEG) / 2 + 16 + 2;
}

// The monomials of the shear (the twin's _shear_monomials): [1], then per coordinate j its own z_j, z_j^2 and
// z_k z_j for the earlier coordinates k of the same velocity component (k % nc == j % nc).
inline void ns_shear_monomials(int D, int nc, std::vector<int> &mono, std::vector<int> &start) {
    mono.assign({-1, -1});
    start.clear();
    for (int j = 0; j < D; ++j) {
        start.push_back((int)mono.size() / 2);
        mono.push_back(j); mono.push_back(-1);
        mono.push_back(j); mono.push_back(j);
        for (int k = 0; k < j; ++k)
            if (k % nc == j % nc) { mono.push_back(k); mono.push_back(j); }
    }
    mono.resize((size_t)(start.back() + 1) * 2);      // the last coordinate is nobody's feature
}

// Every knob in one convention: NS_UNSET or a value.  The sentinels and hundredths of the C API and of the process
// options are translated where they enter (nfa_sampler_set_*, ns_engine_knobs), not here.
#define NS_UNSET INT_MIN
struct NsKnobs {
    int    ellipsoids  = NS_UNSET;  // bounding ellipsoids per pixel at most: 1..NS_ME
    int    frames      = NS_UNSET;  // rotated box frames of a one-ellipsoid bound: 0..NS_FRAMES_MAX, -1 = no boxes
    int    walkers     = NS_UNSET;  // walkers per pixel of a walk cycle: 64, 128, 192, 256; 0 = by the live points
    int    walk_factor = NS_UNSET;  // to walks below an acceptance of 1 / (walk_factor n_steps): >= 1
    int    k_target    = NS_UNSET;  // replacements per pixel and rejection round its share aims at; 0 = everybody the round's Kr
    int    refit_every = NS_UNSET;  // >= 1
    int    ratio_max   = NS_UNSET;  // >= 1
    int    kmax        = NS_UNSET;  // >= 1
    double margin      = NS_UNSET;  // the boxes' margin factor c
    double shear       = NS_UNSET;  // safety factor on the sheared ellipsoid's volume, >= 1; 0 = no shear
    double pairs       = NS_UNSET;  // safety factor on a pair ellipse's area, >= 1; 0 = no pair ellipses
};
// a if it is set, else b: the caller's setter before the process option (ns_merge), the result before the constant (ns_plan)
template <class T> inline T ns_pick(T a, T b) { return a != (T)NS_UNSET ? a : b; }
inline NsKnobs ns_merge(const NsKnobs &a, const NsKnobs &b) {
    NsKnobs k;
    k.ellipsoids = ns_pick(a.ellipsoids, b.ellipsoids); k.frames = ns_pick(a.frames, b.frames);
    k.walkers = ns_pick(a.walkers, b.walkers); k.walk_factor = ns_pick(a.walk_factor, b.walk_factor);
    k.k_target = ns_pick(a.k_target, b.k_target); k.refit_every = ns_pick(a.refit_every, b.refit_every);
    k.ratio_max = ns_pick(a.ratio_max, b.ratio_max); k.kmax = ns_pick(a.kmax, b.kmax);
    k.margin = ns_pick(a.margin, b.margin); k.shear = ns_pick(a.shear, b.shear); k.pairs = ns_pick(a.pairs, b.pairs);
    return k;
}

struct NsPlan {
    int    max_ell;             // ellipsoids per pixel at most
    int    stage_live;          // the refit stages the centred live points in LDS
    int    multi;               // the bound may be split into several ellipsoids
    int    shear, sh_M;         // the shear in front of a one-ellipsoid bound; its monomials
    int    boxes, n_frames;     // free rejections by boxes; rotated frames beside the unit cube's axes and the ellipsoid's own
    int    pairs;               // pair ellipses
    int    walk_factor, k_target, refit_every;
    int    w_fixed, w_stride;   // walkers per pixel whatever the live points (0: ns_walkers_for); walker slots per pixel
    int    ratio_max, kmax;     // proposals per round: at most this multiple of the evaluations aimed for; per pixel at most
    int    refit_threads;       // workgroup of ns_refit_kernel
    double shear_enlarge, margin_c, pairs_enlarge;
    size_t lds_update, lds_refit;   // dynamic LDS of ns_update_kernel / ns_refit_kernel, bytes
    const char *error;          // null, or why there is no plan
};

// D sampled dimensions of a theta row of DT slots, fm[D] = slot of every sampled dimension, N = the stride of the live
// arrays (the largest number of live points of a pixel).  One chain in dependency order; every later line may read the
// earlier ones, never the other way round.
inline NsPlan ns_plan(int D, int DT, int N, const int *fm, const NsKnobs &k) {
    NsPlan p = {};
    // 0. what does not depend on the bound's form
    p.ratio_max = ns_pick(k.ratio_max, NS_RATIO_MAX);
    p.kmax = ns_pick(k.kmax, NS_KMAX);
    p.w_fixed = ns_pick(k.walkers, 0);
    p.w_stride = p.w_fixed > 0 ? p.w_fixed : ns_walkers_for(N);      // (a pixel's own count can only be smaller than N)
    p.walk_factor = ns_pick(k.walk_factor, D <= NS_WALK_LOWD ? NS_WALK_FACTOR_LOWD : NS_WALK_FACTOR);
    p.k_target = ns_pick(k.k_target, NS_K_TARGET);
    p.refit_every = ns_pick(k.refit_every, NS_REFIT_EVERY);
    // 1. staging: every refined bound below works on the live points in LDS
    p.stage_live = (size_t)N * D * sizeof(double) <= NS_STAGE_BYTES ? 1 : 0;
    // 2. several ellipsoids: few dimensions, staged, and not turned off (ellipsoids = 1)
    p.max_ell = ns_pick(k.ellipsoids, NS_ME);
    p.multi = (p.stage_live && D <= NS_ME_MAXD && p.max_ell > 1) ? 1 : 0;
    p.refit_threads = p.multi ? 64 : NS_REFIT_THREADS;               // one wave splits clusters, a full workgroup fits one ellipsoid
    // 3. the shear: one-ellipsoid bounds of all five free parameters of two or three components, dimension j of
    //    component j % nc in a slot of the same component
    p.shear_enlarge = ns_pick(k.shear, NS_SHEAR_ENLARGE);
    const int nc = D / 5;
    bool shape = (D == 10 || D == 15) && DT == 6 * nc;
    for (int j = 0; shape && j < D; ++j) shape = (fm[j] % nc) == (j % nc);
    p.shear = (p.shear_enlarge >= 1.0 && shape && !p.multi && p.stage_live) ? 1 : 0;
    if (p.shear) {
        std::vector<int> mono, start;
        ns_shear_monomials(D, nc, mono, start);
        p.sh_M = (int)mono.size() / 2;
        if (p.sh_M > NS_SHEAR_MMAX) { p.error = "shear: too many monomials"; return p; }
    }
    // 4. free rejections by boxes: one-ellipsoid bounds whose live points are staged.  By default NS_FRAMES frames where
    //    the bound is sheared -- there the pair halves the evaluations of config 5's two-component runs in less time
    //    than the walks take -- and none elsewhere: on BASELINE config 5 the boxes alone save a quarter of the
    //    evaluations of the two-component runs and cost more than that in longer rounds
    const int nf = ns_pick(k.frames, p.shear ? NS_FRAMES : -1);
    p.boxes = (!p.multi && p.stage_live && nf >= 0) ? 1 : 0;
    p.n_frames = p.boxes ? nf : 0;
    p.margin_c = ns_pick(k.margin, NS_MARGIN_C);
    // 5. pair ellipses: with the shear and the boxes; they are fitted in the shear's scratch, four doubles a pair (no
    //    shape the shear admits has more pairs than fit, but the condition is the kernel's and stays)
    p.pairs_enlarge = ns_pick(k.pairs, NS_PAIRS_ENLARGE);
    p.pairs = (p.shear && p.boxes && p.pairs_enlarge >= 1.0 && (size_t)(D * (D - 1) / 2) * 4 <= (size_t)p.sh_M * p.sh_M) ? 1 : 0;
    // 6. LDS.  The update workgroup: the live log-likelihoods, a segment's survivors.  The refit workgroup, in the order
    //    of ns_refit_kernel's carve-up:
    p.lds_update = sizeof(double) * ns_upd_lds(N);
    p.lds_refit = sizeof(double) * 8                                                             // reductions
                + sizeof(double) * ((size_t)D * D + (size_t)((D + 1) & ~1))                        // A, c
                + (p.stage_live ? sizeof(double) * (size_t)N * D : 0)                              // the live points
                + (p.multi ? sizeof(double) * (size_t)((NS_ME + 2) * ns_me_slot(D))                // fit slots ...
                             + sizeof(int) * (size_t)((N + 3) & ~3) : 0)                           // ... and labels, or
                + (p.shear ? sizeof(double) * ((size_t)p.sh_M * p.sh_M + (size_t)D * p.sh_M        // the shear's scratch: Gram matrix,
                                               + 2 * (size_t)D + 2) : 0);                          // coefficients, mu, sg, the constant 1 (+ 1: even)
    return p;
}
