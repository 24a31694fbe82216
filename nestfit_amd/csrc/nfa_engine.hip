// nfa_engine.hip -- host side (C ABI of include/nestfit_amd.h) of the MI355X
// NH3 log-likelihood engine; the kernels live in nfa_device.h.
//
// Build: hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -shared (see
// nestfit_amd/build.py).  One process per GPU; every runner owns a HIP stream.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/nestfit_amd.h"

#define NFA_DATA_QUAL static const
#include "nh3_data.h"
#include "n2hp_data.h"
#include "nfa_device.h"
#include "nfa_lsq.h"
#include "nfa_moments.h"
#include "nfa_set_decl.h"
#include "nfa_set_rules.h"
#include "nfa_set_state.h"

// ---------------------------------------------------------------------------
//  error plumbing
// ---------------------------------------------------------------------------
static thread_local std::string g_err;
static int fail(int code, const std::string &msg) { g_err = msg; return code; }
#define HIP_TRY(expr)                                                              \
    do {                                                                           \
        hipError_t e_ = (expr);                                                    \
        if (e_ != hipSuccess)                                                      \
            return fail(NFA_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// ---------------------------------------------------------------------------
//  host side
// ---------------------------------------------------------------------------
struct Engine {
    bool   init = false;
    int    device = 0;
    int    n_cu = 256;
    int    exp_mode = 2;             // "fast": see include/nestfit_amd.h, nfa_set_exp_mode
    int    wpb = 1;                  // waves per workgroup of the likelihood kernel (fast / poly mode): one -- a workgroup
                                     // retires, and its slot is refilled, wave by wave (4: -1.5 %, 8: -9 %, profiles/r02/sweep_lanes.txt)
    int    wpb_table = 0;            // the same in table mode; 0 = chosen per spectra set (nfa_launch_plan.h: table_waves)
    int    lnl_split = 0;            // waves per (item, spectrum) unit of the likelihood kernel: 1, 2, 4, or
                                     // 0 = by launch size (resolve_split).  The chi^2 of a unit is a sum of LNL_PARTS
                                     // row blocks in a fixed order whatever the split, so every evaluation is bitwise
                                     // independent of it and of the batch it travels in (the sampler twin relies on that)
    int    lnl_queue = 1;            // table mode: launches of two and more units per wave slot run as resident workgroups
                                     // whose waves draw the units from a queue (lnl_kernel_queue); 0 = one unit per wave always
    unsigned long long *d_trace = nullptr;   // test library: the queue kernel's per-wave records (nfa_test_queue_trace)
    int    lnl_queue_wg = 0;         // A/B: workgroups per CU of a queue launch (0 = 2)
    int    lnl_cap = 0;              // fast / poly mode: workgroups of the likelihood kernel resident per CU at most
                                     // (LDS padding; 0 = no cap).  A/B knob: leaving one slot per CU to the set-up
                                     // kernels of the next batch paid off (+7 %) until those kernels got a raised wave
                                     // priority of their own; with it the cap only costs occupancy (-6 %).
    int    ablate = 0;
    int    streams = 0;              // stream lanes of new runners; 0 = six, of which a batch uses four or six (run_batch)
    int    sampler_parts = 3;        // groups of pixels the device sampler pipelines over the lanes
    int    sampler_refit_every = 4;  // rejection-mode pixels refit their bound in every n-th round (A/B knob)
    int    sampler_walkers = 0;      // walkers per pixel of a walk cycle (A/B knob: 64, 128, 192, 256); 0 = by the live points
    int    sampler_ellipsoids = 0;   // 1: one bounding ellipsoid per pixel whatever the dimension (A/B knob; 0: several where it pays)
    int    sampler_frames = -2;      // rotated box frames of a one-ellipsoid bound: -2 = by the sampled dimensions, -1 = no boxes, 0..64
    int    sampler_margin_pct = 0;   // the boxes' margin factor c in hundredths (0 = NS_MARGIN_C)
    int    profile_skip = 0;         // nfa_runner_get_profile leaves the first calls out (warm-up launches behind an idle gap)
    int    sampler_ktarget = -1;     // replacements per pixel and rejection round its share of proposals aims at (-1 = NS_K_TARGET, 0 = everybody the round's Kr)
    int    sampler_pairs_pct = -1;   // the pair ellipses' safety factor in hundredths (-1 = NS_PAIRS_ENLARGE where the bound is sheared and boxed, 0 = off)
    int    sampler_ratio_max = 0;    // proposals drawn per round: at most this multiple of the evaluations aimed for (0 = NS_RATIO_MAX)
    int    sampler_kmax = 0;         // most proposals one pixel gets in a round (0 = NS_KMAX)
    int    sampler_shear_pct = -1;   // the shear's safety factor in hundredths (-1 = the default, NS_SHEAR_ENLARGE where the shape allows; 0 = no shear)
    int    sampler_walk_factor = 0;  // a pixel turns to walks when rejection accepts fewer than 1 in factor * n_steps; 0 = by the
                                     // number of sampled dimensions (nfa_sampler_begin)
    int    graph = -1;               // single-point graph replay: -1 = decide at first use, 0 off, 1 on
    int    coalesce = NFA_GROUP_MAX; // device-pointer batches of one shape enqueued back to back travel as one launch, up to
                                     // this many (1 = every batch its own launches)
    int    prior_stage = 1;          // prior tables staged in LDS by the set-up kernel (priors created afterwards)
    int    setup_ti = 0, setup_threads = 0;   // set-up kernel: items and threads per workgroup (0 = 64 / 256)
    int    setup_overlap = 1;                 // set-up stage: a resolved prior's velocities beside the sums and records (0: in sequence, A/B)
    int    setup_sub = 0;                     // table mode: 1 = one group of items per set-up workgroup (0 = two where the batch allows)
    int    point = 1;                // single points: 1 = the one-launch point kernel, 0 = the batch kernels (graph replay)
    bool   have_t0 = false;
    double *d_tabs = nullptr;                      // SM_END_TABLE doubles
    double t0_xmin = 0, t0_xmax = 0, t0_inv_dx = 0;
};
static Engine g_eng;
struct nfa_runner;
static int flush_pending(nfa_runner *r);
static int flush_all_runners();
static std::mutex g_runners_m;
static std::vector<nfa_runner *> g_runners;         // live runners: nfa_device_synchronize / nfa_set_exp_mode flush them all

// The HIP runtime multiplexes a process's streams over GPU_MAX_HW_QUEUES hardware queues (default 4);
// streams that share a queue run in order with each other.  A runner's stream lanes only overlap when
// every lane has a queue of its own, so ask for 8 -- before the runtime reads the variable, i.e. when this
// library is loaded, and only if the user has not set it.
__attribute__((constructor)) static void nfa_hw_queues() { setenv("GPU_MAX_HW_QUEUES", "8", 0); }

static int engine_init_once();
// HIP's current device is per host thread (default 0): every public entry point that allocates or
// launches binds the calling thread to the engine's device first (broker threads, sampler threads
// of a host application, MultiNest's own thread).
static int engine_init() {
    if (!g_eng.init) { int rc = engine_init_once(); if (rc) return rc; }
    static thread_local int bound = -1;
    if (bound != g_eng.device) {
        HIP_TRY(hipSetDevice(g_eng.device));
        bound = g_eng.device;
    }
    return NFA_OK;
}
static int engine_init_once() {
    static std::mutex mu;
    std::lock_guard<std::mutex> lock(mu);
    if (g_eng.init) return NFA_OK;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(NFA_ERR_DEVICE, "no HIP device available (the engine has no CPU fallback)");
    HIP_TRY(hipSetDevice(g_eng.device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, g_eng.device));
    g_eng.n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    {   // what belongs to a transition beyond its lines (nfa_device.h); the lines are per spectra set (set_plan, nfa_set_decl.h)
        static double h_nu[NFA_T_ALL];
        for (int t = 0; t < NFA_N_LEVELS; ++t) h_nu[t] = nfa_nu[t];
        for (int t = 0; t < NFA_N2HP_LEVELS; ++t) h_nu[NFA_T_N2HP + t] = nfa_n2hp_nu[t];
        h_nu[NFA_T_GAUSS] = 0.0; h_nu[NFA_T_LINES] = 0.0;
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(c_nu), h_nu, sizeof(h_nu)));
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(c_ea), nfa_ea, sizeof(nfa_ea)));
    }
    std::vector<double> tabs(SM_END_TABLE, 0.0);
    // 2^(i/256)
    for (int i = 0; i < NFA_EXP2_N; ++i) tabs[SM_EXP2 + i] = (double)exp2l((long double)i / (long double)NFA_EXP2_N);
    // FastExp product tables: host libm exp() of exactly representable
    // arguments, as the reference fills them (fastexp.c:203-226)
    for (int l = 0; l < 10; ++l) {
        for (int j = 0; j < 128; ++j) tabs[SM_FEA + l * 128 + j] = exp(-ldexp((double)(128 + j), l - 12));
        for (int j = 0; j < 256; ++j) {
            tabs[SM_FEB + l * 256 + j] = exp(-ldexp((double)j, l - 20));
            tabs[SM_FEC + l * 256 + j] = exp(-ldexp((double)j, l - 28));
        }
    }
    HIP_TRY(hipMalloc(&g_eng.d_tabs, sizeof(double) * SM_END_TABLE));
    HIP_TRY(hipMemcpy(g_eng.d_tabs, tabs.data(), sizeof(double) * SM_END_TABLE, hipMemcpyHostToDevice));
    g_eng.init = true;
    return NFA_OK;
}

// A set's likelihood options: the per-spectrum part (nfa_set_state.h) and the two large arrays, empty where the option is off
struct SetRecord {
    SetOptions o;
    std::vector<double> tmpl;                       // the caller's templates [NFA_TMPL_MAX][chan_tot], unused slots zero
    std::vector<double> cont;                       // the caller's continuum [n_pix][n_spec]
};
static_assert(SET_RESP_NT == NFA_RESP_NT, "nfa_set_state.h keeps the taps of a response");

struct nfa_specset {
    SpecDev dev{};
    int64_t n_pix = 0;
    int     nhf_max = 0;
    double *d_xarr = nullptr, *d_t0 = nullptr, *d_tbg = nullptr, *d_data = nullptr, *d_noise = nullptr;
    double *d_t0tbg = nullptr, *d_rowsq = nullptr, *d_totsq = nullptr;
    double *d_w = nullptr, *d_wdata = nullptr;     // a noise per channel: SpecDev.chan_w, .wdata (null otherwise)
    double *d_bl = nullptr;                         // a baseline: SpecDev.bl (nfa_specset_set_baseline)
    LineRow *d_lines = nullptr;                     // the line rows of the spectra: SpecDev.lines
    LteRec  *d_lte = nullptr;                       // the LTE model's record: SpecDev.lte_rec (null for the other models)
    BandRec *d_band = nullptr;                      // LTE bands: SpecDev.band (null for a set without a banded spectrum)
    MixRec  *d_mix = nullptr;                       // LTE mixes: SpecDev.mix (null for a set of one species)
    GridRec *d_grid = nullptr;                      // the excitation-grid model's record: SpecDev.grid (null for the other models) ...
    double  *d_grid_tex = nullptr, *d_grid_ltau = nullptr;     // ... and its tables [n_spec][nt][nn][nc], which the record points at
    int     h_nhf[MAXSPEC] = {};                    // lines of every spectrum
    bool    filled = false;                         // an LTE set with a beam filling factor per component: the last parameter
    bool    layered = false;                        // layered transfer: a component absorbs those behind it (nfa_specset_set_layered)
    bool    chan_noise = false;                     // a noise per channel: d_w and d_wdata are the set's from its creation
    bool    masked = false;                         // ... with a masked channel (w = 0) somewhere
    // The likelihood options as the caller gave them (the nfa_specset_set_* calls): "is option X on" is a question to this
    // record.  The buffers below are what set_layout (nfa_set_state.h) makes of it, kept so by specset_realise alone.
    SetRecord opt;
    double *d_cal2 = nullptr;                       // a calibration uncertainty: SpecDev.cal2
    // correlated channel noise or a channel response: Q's diagonal (SpecDev.chan_w while it lasts; d_w keeps u^2) and
    // off-diagonals, the entries of R^-1 per spectrum (white without a correlation); SpecDev.resp
    double *d_q0 = nullptr, *d_q1 = nullptr, *d_q2 = nullptr, *d_corr = nullptr, *d_resp = nullptr;
    double *d_tmpl = nullptr, *d_tp = nullptr;      // nuisance templates: SpecDev.tmpl (scaled) and .tp
    double *d_nmarg = nullptr;                      // an uncertain noise level: SpecDev.nmarg
    double *d_cont = nullptr;                       // a continuum background: SpecDev.cont
    // a robust likelihood: g and g d (SpecDev.chan_w and .wdata while it lasts; d_w and d_wdata keep the set's own), SpecDev.rob
    double *d_rg = nullptr, *d_rgd = nullptr, *d_rob = nullptr;
};
// The option-dependent buffers of a set: specset_realise allocates and frees through this list, nfa_specset_destroy frees
// through it.  (Doubles all of them; the message is what a failed allocation says.)
static const char OOM_WEIGHTS[] = "out of device memory for the channel weights";
struct SetBuf { unsigned bit; double *nfa_specset::*p; const char *oom; };
static const SetBuf SET_BUFS[SB_N] = {
    {SB_W, &nfa_specset::d_w, OOM_WEIGHTS}, {SB_WDATA, &nfa_specset::d_wdata, OOM_WEIGHTS},
    {SB_BL, &nfa_specset::d_bl, "out of device memory for the baseline records"},
    {SB_TP, &nfa_specset::d_tp, "out of device memory for the templates' records"},
    {SB_CAL2, &nfa_specset::d_cal2, "out of device memory for the calibration uncertainties"},
    {SB_NMARG, &nfa_specset::d_nmarg, "out of device memory for the noise uncertainties' records"},
    {SB_Q0, &nfa_specset::d_q0, "out of device memory for the correlated weights"},
    {SB_Q1, &nfa_specset::d_q1, "out of device memory for the correlated weights"},
    {SB_Q2, &nfa_specset::d_q2, "out of device memory for the correlated weights"},
    {SB_CORR, &nfa_specset::d_corr, "out of device memory for the correlation's coefficients"},
    {SB_RESP, &nfa_specset::d_resp, "out of device memory for the channel response"},
    {SB_TMPL, &nfa_specset::d_tmpl, "out of device memory for the templates"},
    {SB_CONT, &nfa_specset::d_cont, "out of device memory for the continuum"},
    {SB_RG, &nfa_specset::d_rg, "out of device memory for the robust weights"},
    {SB_RGD, &nfa_specset::d_rgd, "out of device memory for the robust weights"},
    {SB_ROB, &nfa_specset::d_rob, "out of device memory for the robust records"},
};
static size_t set_buf_doubles(const nfa_specset *ss, unsigned bit) {
    const SpecDev &d = ss->dev;
    const size_t spec = (size_t)(ss->n_pix * d.n_spec);
    switch (bit) {
    case SB_BL: return NFA_BL_REC * spec;
    case SB_TP: return NFA_TP_REC * spec;
    case SB_CAL2: return (size_t)d.n_spec;
    case SB_NMARG: case SB_ROB: return 2 * spec;
    case SB_CORR: return NFA_CORR_NC * MAXSPEC;
    case SB_RESP: return NFA_RESP_NT * MAXSPEC;
    case SB_TMPL: return NFA_TMPL_MAX * (size_t)d.chan_tot;
    case SB_CONT: return spec;
    default: return (size_t)(ss->n_pix * d.chan_tot);      // per channel, like the data
    }
}

struct nfa_priors {
    PriorProg prog{};
    PriorProg *d_prog = nullptr;       // device copy handed to the kernels
    PriorProg *d_prog_global = nullptr;    // the same program with n_stage = 0 (its tables read from global memory: the same
                                           // values) for a set-up launch whose staged layout does not fit; d_prog if nothing is staged
    std::vector<double *> d_arrays;
};

// Scratch of the posterior moments (nfa_moments.h), owned by a runner and grown on demand.  Per segment: the reference
// rows' spectra and row statistics, the accumulator planes of both matrices, S0.  Per chunk: the rows' statistics and
// weights and the chunk's pieces; two pinned staging slots (a chunk's pixel per row, then its pieces) that the host fills
// for chunk c + 1 while the device works on chunk c -- a slot's event stands behind the copies out of it.
struct MomScratch {
    double *d_ref = nullptr, *d_acc = nullptr, *d_sref = nullptr, *d_sacc = nullptr, *d_s0 = nullptr;
    int64_t cap_seg = 0;
    double *d_stat = nullptr, *d_w = nullptr;
    MomPiece *d_pieces = nullptr;
    int64_t cap_rows = 0;
    char *h_stage[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
};

// Scratch of the normal equations (nfa_lsq.h), owned by a runner and grown on demand: one slab of doubles in the order of
// lsq_scratch (nfa_lsq_plan.h) and the points' pixels.
struct LsqScratch {
    double *d_buf = nullptr;
    int    *d_pix = nullptr;
    int64_t cap_B = 0;
};

#define NFA_MAX_LANES 8
struct nfa_runner {
    nfa_specset *ss = nullptr;
    nfa_priors  *pr = nullptr;
    int ncomp = 1, cold = 0, lte = 0, ndim = 6;
    // numerical mode: -1 = the process default at call time (nfa_set_exp_mode), 0..2 = pinned to
    // this runner (nfa_runner_set_exp_mode): runners of different modes may then work side by side
    int exp_mode = -1;
    LpShape shape = {};              // what the launch plans read of all that, and the launch geometry (nfa_launch_plan.h)
    // Stream lanes: consecutive batches go to different HIP streams (round robin), so the
    // tail of one batch (few workgroups left, SIMDs draining) overlaps the start of the
    // next; inside a lane the set-up kernel and the likelihood kernel run in order and own
    // the lane's derived-parameter records.
    int         n_lanes = 1;
    bool        lanes_auto = false;      // four lanes, six once batches of about one wave per slot have come by (run_batch)
    hipStream_t lanes[NFA_MAX_LANES] = {};
    double     *d_D[NFA_MAX_LANES] = {};
    double     *d_band[NFA_MAX_LANES] = {};  // LTE bands: tau_main per (item, component, spectrum, transition) (lte_band_kernel)
    double     *d_part[NFA_MAX_LANES] = {};  // per (item, spectrum) log-likelihood terms
    unsigned   *d_queue[NFA_MAX_LANES] = {}; // unit counters of the lane's table-mode launches (lnl_kernel_queue), zero between launches
    int64_t     cap_D[NFA_MAX_LANES] = {};
    hipStream_t stream = nullptr;            // lane 0: also the stream of the host-pointer entry points
    uint64_t    n_calls = 0;
    unsigned    lane_busy = 0;               // lanes with work enqueued and not yet synchronised
    double *d_U = nullptr, *d_lnL = nullptr, *d_spec = nullptr;
    int    *d_pix = nullptr;
    int64_t cap_B = 0, cap_spec = 0;
    // single-point calls (MultiNest's LogLike): the whole H2D -> 5 kernels -> D2H sequence as one
    // captured graph, replayed per call (built on the third single-point call in a given mode)
    hipGraphExec_t g1 = nullptr;
    int     g1_mode = -1;
    double *h_pin = nullptr;         // pinned staging: ndim + 1 doubles
    uint64_t n_single = 0;
    bool    part_only = false;       // a batch leaves the per-spectrum chi^2 parts; whoever set this sums them (the device sampler's update)
    double *h_point = nullptr;       // mapped host buffer of the point kernel: theta[ndim], lnL, sequence number
    double *d_point = nullptr;       // the same buffer as the device sees it
    unsigned *d_point_done = nullptr; // workgroups of a point launch that have finished
    uint64_t pt_seq = 0;
    // optional per-kernel timing (HIP events on the runner's stream)
    bool profiling = false;
    std::vector<hipEvent_t> ev;      // per call: start and stop of the set-up kernel's dispatch, start and stop of lnl_kernel's
    size_t ev_used = 0;
    hipEvent_t *ev_cur = nullptr;        // profiling: [set-up start, stop, likelihood start, stop] of the call under way
    BatchGroup  cur_group = {};          // the batches of the launches being enqueued (run_group)
    BatchGroup  pending = {};            // device-pointer batches accepted but not yet launched (coalescing)
    MomScratch  mom;                     // nfa_runner_predict_moments, nfa_runner_row_statistics: reference rows, accumulators, staging
    LsqScratch  lsq;                     // nfa_runner_normal_equations: the points, their probe steps and the outputs
    bool        pending_prior = true;    // ... loglike batches (unit cube, prior transform) or predict batches (physical parameters)
    // One in-flight call per runner is the contract (include/nestfit_amd.h); the process-wide calls
    // (nfa_device_synchronize, nfa_set_exp_mode) walk every live runner from whatever thread makes them, so the state a
    // launch touches -- pending, cur_group, n_calls, lane_busy, the lanes themselves -- is guarded: every public entry
    // point of a runner and the global flush take this lock (recursive: entry points call each other).
    std::recursive_mutex mu;
};
#define RUNNER_LOCK(r) std::lock_guard<std::recursive_mutex> runner_lock_((r)->mu)
// numerical mode of a runner's launches: its own, or the process default at call time
static int runner_mode(const nfa_runner *r) { return r->exp_mode >= 0 ? r->exp_mode : g_eng.exp_mode; }
// the inputs of the launch plans: the options as they stand now, and a launch of B items of the runner's set as it is now
static LpKnobs plan_knobs() { return {g_eng.n_cu, g_eng.setup_ti, g_eng.setup_threads, g_eng.setup_sub, g_eng.lnl_queue, g_eng.lnl_queue_wg, g_eng.coalesce, g_eng.ablate}; }
static LpLaunch plan_launch(const nfa_runner *r, int64_t B, int mode, bool write_spec, bool has_prior, int slot) {
    return LpLaunch{B, mode, r->cur_group.n, r->cur_group.each, write_spec, has_prior, r->ss->dev.bl_order >= 0 || r->ss->dev.cont != nullptr || r->ss->dev.grid != nullptr,
                    r->ss->dev.chan_w != nullptr, r->d_queue[slot] != nullptr, r->ss->filled, r->ss->layered, r->ss->dev.cal2 != nullptr};
}
#ifdef NFA_TEST_HOOKS
// nfa_testhooks.h: the test library's option "fail_alloc" arms set_alloc's k-th call from now to fail, once
static void test_fail_alloc(int k);
static bool test_alloc_fails();
#endif

extern "C" {

const char *nfa_last_error(void) { return g_err.c_str(); }
int nfa_version(void) { return 100; }

int nfa_device_count(int *count) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; return fail(NFA_ERR_DEVICE, hipGetErrorString(e)); }
    *count = n;
    return NFA_OK;
}

int nfa_set_device(int device) {
    if (g_eng.init && device != g_eng.device)
        return fail(NFA_ERR_STATE, "nfa_set_device must be called before any other engine call");
    g_eng.device = device;
    return engine_init();
}

int nfa_device_synchronize(void) {
    int rc = flush_all_runners(); if (rc) return rc;          // batches held for coalescing are launched first
    HIP_TRY(hipDeviceSynchronize());
    return NFA_OK;
}

int nfa_device_name(char *buf, int buflen) {
    int rc = engine_init(); if (rc) return rc;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, g_eng.device));
    snprintf(buf, buflen, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
    return NFA_OK;
}

int nfa_device_uuid(char *buf, int buflen) {
    if (!buf || buflen < 33) return fail(NFA_ERR_ARG, "buffer too small for a UUID (33 bytes)");
    int rc = engine_init(); if (rc) return rc;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, g_eng.device));
    for (int k = 0; k < 16; ++k) snprintf(buf + 2 * k, 3, "%02x", (unsigned)(unsigned char)prop.uuid.bytes[k]);
    return NFA_OK;
}

int nfa_set_exp_mode(int mode) {
    if (mode != 0 && mode != 2) return fail(NFA_ERR_ARG, "exp mode must be 0 (table) or 2 (fast)");
    { int rc = flush_all_runners(); if (rc) return rc; }       // what is held was enqueued under the old mode
    g_eng.exp_mode = mode;
    return NFA_OK;
}
int nfa_get_exp_mode(void) { return g_eng.exp_mode; }

int nfa_set_option(const char *key, int value) {
    // what is held was accepted under the old options (enqueue_dev: B % setup_ti; launch_setup reads it at the flush)
    { int rc = flush_all_runners(); if (rc) return rc; }
    if (key && !strcmp(key, "lnl_cap") && value >= 0 && value <= 8) { g_eng.lnl_cap = value; return NFA_OK; }
    if (key && !strcmp(key, "lnl_queue_wg") && value >= 0 && value <= 2) { g_eng.lnl_queue_wg = value; return NFA_OK; }
    if (key && !strcmp(key, "lnl_queue") && (value == 0 || value == 1)) { g_eng.lnl_queue = value; return NFA_OK; }
    if (key && !strcmp(key, "lnl_split") && (value == 0 || value == 1 || value == 2 || value == 4)) { g_eng.lnl_split = value; return NFA_OK; }
    if (key && !strcmp(key, "graph") && (value == 0 || value == 1)) { g_eng.graph = value; return NFA_OK; }
    if (key && !strcmp(key, "point") && (value == 0 || value == 1)) { g_eng.point = value; return NFA_OK; }
    if (key && !strcmp(key, "coalesce") && value >= 1 && value <= NFA_GROUP_MAX) { g_eng.coalesce = value; return NFA_OK; }
    if (key && !strcmp(key, "prior_stage") && (value == 0 || value == 1)) { g_eng.prior_stage = value; return NFA_OK; }
    if (key && !strcmp(key, "setup_ti") && (value == 0 || value == 8 || value == 16 || value == 32 || value == 64)) { g_eng.setup_ti = value; return NFA_OK; }
    if (key && !strcmp(key, "setup_overlap") && (value == 0 || value == 1)) { g_eng.setup_overlap = value; return NFA_OK; }
    if (key && !strcmp(key, "setup_sub") && (value == 0 || value == 1)) { g_eng.setup_sub = value; return NFA_OK; }
    if (key && !strcmp(key, "setup_threads") && (value == 0 || value == 256 || value == 320 || value == 384 || value == 448 || value == 512)) { g_eng.setup_threads = value; return NFA_OK; }
    if (key && !strcmp(key, "sampler_parts") && value >= 1 && value <= 4) { g_eng.sampler_parts = value; return NFA_OK; }
    if (key && !strcmp(key, "sampler_refit_every") && value >= 1 && value <= 16) { g_eng.sampler_refit_every = value; return NFA_OK; }
    if (key && !strcmp(key, "sampler_walkers") && value >= 0 && value <= 256 && value % 64 == 0) { g_eng.sampler_walkers = value; return NFA_OK; }
    if (key && !strcmp(key, "sampler_ellipsoids") && value >= 0 && value <= 1) { g_eng.sampler_ellipsoids = value; return NFA_OK; }
    if (key && !strcmp(key, "sampler_walk_factor") && value >= 0 && value <= 1024) { g_eng.sampler_walk_factor = value; return NFA_OK; }
    if (key && !strcmp(key, "sampler_frames") && value >= -2 && value <= 64) { g_eng.sampler_frames = value; return NFA_OK; }
    if (key && !strcmp(key, "sampler_margin_pct") && value >= 0 && value <= 1000) { g_eng.sampler_margin_pct = value; return NFA_OK; }
    if (key && !strcmp(key, "profile_skip") && value >= 0 && value <= 100000) { g_eng.profile_skip = value; return NFA_OK; }
    if (key && !strcmp(key, "sampler_ktarget") && value >= -1 && value <= 4096) { g_eng.sampler_ktarget = value; return NFA_OK; }
    if (key && !strcmp(key, "sampler_pairs_pct") && (value == -1 || value == 0 || (value >= 100 && value <= 100000))) { g_eng.sampler_pairs_pct = value; return NFA_OK; }
    if (key && !strcmp(key, "sampler_ratio_max") && value >= 0 && value <= 64) { g_eng.sampler_ratio_max = value; return NFA_OK; }
    if (key && !strcmp(key, "sampler_kmax") && (value == 0 || (value >= 64 && value <= 262144))) { g_eng.sampler_kmax = value; return NFA_OK; }
    if (key && !strcmp(key, "sampler_shear_pct") && (value == -1 || value == 0 || (value >= 100 && value <= 100000))) { g_eng.sampler_shear_pct = value; return NFA_OK; }
    if (key && !strcmp(key, "wpb_table") && value >= 0 && value <= 16) { g_eng.wpb_table = value; return NFA_OK; }
    if (key && !strcmp(key, "wpb") && value >= 1 && value <= 16) { g_eng.wpb = value; return NFA_OK; }
#ifdef NFA_ABLATE
    if (key && !strcmp(key, "ablate") && value >= 0 && value <= 127) { g_eng.ablate = value; return NFA_OK; }
#endif
#ifdef NFA_TEST_HOOKS
    if (key && !strcmp(key, "fail_alloc") && value >= 0) { test_fail_alloc(value); return NFA_OK; }
#endif
    if (key && !strcmp(key, "streams") && value >= 0 && value <= NFA_MAX_LANES) { g_eng.streams = value; return NFA_OK; }
    return fail(NFA_ERR_ARG, "unknown option, or value out of range");
}

int nfa_set_iemtex_table(const double *t0_x, const double *t0_y, int64_t n) {
    if (n != T0_SIZE || !t0_x || !t0_y) return fail(NFA_ERR_ARG, "iemtex table must have 1000 points");
    int rc = engine_init(); if (rc) return rc;
    HIP_TRY(hipMemcpy(g_eng.d_tabs + SM_T0X, t0_x, sizeof(double) * T0_SIZE, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(g_eng.d_tabs + SM_T0Y, t0_y, sizeof(double) * T0_SIZE, hipMemcpyHostToDevice));
    g_eng.t0_xmin = (NFA_H * 23.0e9 / NFA_KB) / 8.0;           // hyperfine.pyx:13-16
    g_eng.t0_xmax = (NFA_H * 28.0e9 / NFA_KB) / 2.7;
    g_eng.t0_inv_dx = 1.0 / (t0_x[1] - t0_x[0]);               // hyperfine.pyx:20
    g_eng.have_t0 = true;
    return NFA_OK;
}

// ---- spectra ---------------------------------------------------------------
// sums of data^2 per row of 64 channels (chi^2 of the rows without a line window) of pixels
// [pix0, pix0 + n)
static int launch_rowsq(nfa_specset *ss, int64_t pix0, int64_t n) {
    const int64_t waves = n * ss->dev.rows_tot;
    hipLaunchKernelGGL(ss->dev.chan_w ? rowsq_w_kernel : rowsq_kernel, dim3((unsigned)((waves * 64 + 255) / 256)), dim3(256), 0, 0,
                       ss->dev, (long)pix0, (long)n, ss->d_rowsq);
    hipLaunchKernelGGL(totsq_kernel, dim3((unsigned)((n * ss->dev.n_spec + 255) / 256)), dim3(256), 0, 0, ss->dev,
                       (long)pix0, (long)n, (const double *)ss->d_rowsq, ss->d_totsq);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return NFA_OK;
}

// weighted sets: chan_w and the masked, weighted data of pixels [pix0, pix0 + n) (form_w: chan_w from the channel noise
// that d_w holds)
static int launch_chan_weight(nfa_specset *ss, int64_t pix0, int64_t n, bool form_w) {
    const int64_t items = n * ss->dev.chan_tot;
    hipLaunchKernelGGL(chan_weight_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, 0, ss->dev,
                       (long)pix0, (long)n, ss->d_w, ss->d_data, ss->d_wdata, (int)form_w);
    HIP_TRY(hipGetLastError());
    return NFA_OK;
}

// correlated channel noise: wdata = Q d of pixels [pix0, pix0 + n) (form_q: Q's bands too) from the set's own weights in d_w
static int launch_corr_setup(nfa_specset *ss, int64_t pix0, int64_t n, bool form_q) {
    const int64_t items = n * ss->dev.chan_tot;
    hipLaunchKernelGGL(corr_setup_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, 0, ss->dev,
                       (long)pix0, (long)n, (const double *)ss->d_w, ss->d_q0, ss->d_q1, ss->d_q2, ss->d_wdata, (int)form_q);
    HIP_TRY(hipGetLastError());
    return NFA_OK;
}

// baseline records of pixels [pix0, pix0 + n) (form_basis: the Gram matrix and L^-1 too, not only m(d))
static int launch_bl_setup(nfa_specset *ss, int64_t pix0, int64_t n, bool form_basis) {
    const int64_t waves = n * ss->dev.n_spec;
    hipLaunchKernelGGL(bl_setup_kernel, dim3((unsigned)((waves * 64 + 255) / 256)), dim3(256), 0, 0, ss->dev,
                       (long)pix0, (long)n, ss->d_bl, (int)form_basis);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return NFA_OK;
}

// records of a set with templates of pixels [pix0, pix0 + n) (form_basis: the Gram matrix and L^-1 too, not only m(d))
static int launch_tmpl_setup(nfa_specset *ss, int64_t pix0, int64_t n, bool form_basis) {
    const int64_t waves = n * ss->dev.n_spec;
    hipLaunchKernelGGL(tmpl_setup_kernel, dim3((unsigned)((waves * 64 + 255) / 256)), dim3(256), 0, 0, ss->dev,
                       (long)pix0, (long)n, ss->d_tp, (int)form_basis);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return NFA_OK;
}

// The creators of include/nestfit_amd.h: each fills its prefix of the declaration (SetDecl, nfa_set_decl.h) with what it was
// given, and specset_build, behind specset_realise below, makes the set of it.
static int specset_build(nfa_specset **out, const SetDecl &decl);

int nfa_specset_create_model(nfa_specset **out, int model, int n_spec, const int64_t *sizes,
                             const int32_t *trans_ids, const double *rest_freqs,
                             const double *const *xarr, int64_t n_pix, const double *data,
                             const double *noise) {
    return specset_build(out, SetDecl{DECL_MODEL, out, model, n_spec, sizes, xarr, n_pix, data, noise, nullptr, rest_freqs, trans_ids});
}
int nfa_specset_create(nfa_specset **out, int n_spec, const int64_t *sizes,
                       const int32_t *trans_ids, const double *const *xarr,
                       int64_t n_pix, const double *data, const double *noise) {
    return specset_build(out, SetDecl{DECL_MODEL, out, NFA_MODEL_AMMONIA, n_spec, sizes, xarr, n_pix, data, noise, nullptr, nullptr, trans_ids});
}
int nfa_specset_create_channel_noise(nfa_specset **out, int model, int n_spec, const int64_t *sizes,
                                     const int32_t *trans_ids, const double *rest_freqs,
                                     const double *const *xarr, int64_t n_pix, const double *data,
                                     const double *chan_noise) {
    return specset_build(out, SetDecl{DECL_CHANNEL_NOISE, out, model, n_spec, sizes, xarr, n_pix, data, nullptr, chan_noise, rest_freqs, trans_ids});
}

int nfa_specset_create_lines(nfa_specset **out, int n_spec, const int64_t *sizes, const int32_t *n_lines,
                             const double *rest_freqs, const double *voff, const double *tau_wts,
                             const double *const *xarr, int64_t n_pix, const double *data, const double *noise,
                             const double *chan_noise) {
    return specset_build(out, SetDecl{DECL_LINES, out, NFA_MODEL_HYPERFINE, n_spec, sizes, xarr, n_pix, data, noise, chan_noise, rest_freqs, nullptr,
                                      n_lines, voff, tau_wts});
}

// nfa_specset_create_lines with an excitation grid: the declaration is the lines creator's, the grid rides beside it
int nfa_specset_create_grid(nfa_specset **out, int n_spec, const int64_t *sizes, const int32_t *n_lines,
                            const double *rest_freqs, const double *voff, const double *tau_wts,
                            int nt, const double *tkin, int nn, const double *lnden, int nc, const double *lncd,
                            const double *tex, const double *ltau,
                            const double *const *xarr, int64_t n_pix, const double *data, const double *noise,
                            const double *chan_noise) {
    SetDecl d{DECL_LINES, out, NFA_MODEL_GRID, n_spec, sizes, xarr, n_pix, data, noise, chan_noise, rest_freqs, nullptr, n_lines, voff, tau_wts};
    d.grid = true;
    d.g_nt = nt; d.g_nn = nn; d.g_nc = nc;
    d.g_tkin = tkin; d.g_lnden = lnden; d.g_lncd = lncd; d.g_tex = tex; d.g_ltau = ltau;
    return specset_build(out, d);
}

int nfa_specset_create_lte(nfa_specset **out, int n_spec, const int64_t *sizes, const int32_t *n_lines,
                           const double *rest_freqs, const double *voff, const double *tau_wts,
                           const double *e_up, const double *g_up, const double *a_ul,
                           int n_q, const double *q_temp, const double *q_val,
                           const double *const *xarr, int64_t n_pix, const double *data, const double *noise,
                           const double *chan_noise) {
    const int32_t nq = n_q;
    return specset_build(out, SetDecl{DECL_LTE, out, NFA_MODEL_LTE, n_spec, sizes, xarr, n_pix, data, noise, chan_noise, rest_freqs, nullptr,
                                      n_lines, voff, tau_wts, e_up, g_up, a_ul, &nq, q_temp, q_val});
}

int nfa_specset_create_lte_bands(nfa_specset **out, int n_spec, const int64_t *sizes, const int32_t *n_trans,
                                 const int32_t *n_lines, const double *trans_freqs, const double *voff, const double *tau_wts,
                                 const double *e_up, const double *g_up, const double *a_ul,
                                 int n_q, const double *q_temp, const double *q_val,
                                 const double *const *xarr, int64_t n_pix, const double *data, const double *noise,
                                 const double *chan_noise) {
    const int32_t nq = n_q;
    return specset_build(out, SetDecl{DECL_BANDS, out, NFA_MODEL_LTE, n_spec, sizes, xarr, n_pix, data, noise, chan_noise, trans_freqs, nullptr,
                                      n_lines, voff, tau_wts, e_up, g_up, a_ul, &nq, q_temp, q_val, n_trans});
}

int nfa_specset_create_lte_mix(nfa_specset **out, int n_spec, const int64_t *sizes, const int32_t *n_trans,
                               const int32_t *n_lines, const double *trans_freqs, const double *voff, const double *tau_wts,
                               const double *e_up, const double *g_up, const double *a_ul,
                               int n_species, const int32_t *species, const int32_t *n_q, const double *q_temp, const double *q_val,
                               const double *const *xarr, int64_t n_pix, const double *data, const double *noise,
                               const double *chan_noise) {
    return specset_build(out, SetDecl{DECL_MIX, out, NFA_MODEL_LTE, n_spec, sizes, xarr, n_pix, data, noise, chan_noise, trans_freqs, nullptr,
                                      n_lines, voff, tau_wts, e_up, g_up, a_ul, n_q, q_temp, q_val, n_trans, n_species, species});
}

// nfa_specset_create_lte_mix with one more parameter per component.  A filled set owns its band and mix records whatever it
// holds -- one species, a transition per spectrum -- so that launch_band runs for it (SetKind, nfa_set_decl.h).
int nfa_specset_create_lte_filled(nfa_specset **out, int n_spec, const int64_t *sizes, const int32_t *n_trans,
                                  const int32_t *n_lines, const double *trans_freqs, const double *voff, const double *tau_wts,
                                  const double *e_up, const double *g_up, const double *a_ul,
                                  int n_species, const int32_t *species, const int32_t *n_q, const double *q_temp, const double *q_val,
                                  const double *const *xarr, int64_t n_pix, const double *data, const double *noise,
                                  const double *chan_noise) {
    return specset_build(out, SetDecl{DECL_FILLED, out, NFA_MODEL_LTE, n_spec, sizes, xarr, n_pix, data, noise, chan_noise, trans_freqs, nullptr,
                                      n_lines, voff, tau_wts, e_up, g_up, a_ul, n_q, q_temp, q_val, n_trans, n_species, species});
}

int nfa_builtin_lines(int model, int trans_id, double *nu, double *voff, double *tau_wts, int *n) {
    if (!nu || !voff || !tau_wts || !n) return fail(NFA_ERR_ARG, "null argument");
    int tg;
    if (model == NFA_MODEL_AMMONIA && trans_id >= 1 && trans_id <= NFA_N_LEVELS) tg = trans_id - 1;
    else if (model == NFA_MODEL_DIAZENYLIUM && trans_id >= 1 && trans_id <= NFA_N2HP_LEVELS) tg = NFA_T_N2HP + trans_id - 1;
    else return fail(NFA_ERR_ARG, "no shipped line table for this model and trans_id (ammonia 1..9, N2H+ 1..3)");
    const double *v, *w;
    *n = builtin_table(tg, nu, &v, &w);
    memcpy(voff, v, sizeof(double) * NFA_MAX_HF_N);
    memcpy(tau_wts, w, sizeof(double) * NFA_MAX_HF_N);
    return NFA_OK;
}

int nfa_specset_destroy(nfa_specset *ss) {
    if (!ss) return NFA_OK;
    (void)hipFree(ss->d_xarr); (void)hipFree(ss->d_t0); (void)hipFree(ss->d_tbg); (void)hipFree(ss->d_data); (void)hipFree(ss->d_noise);
    (void)hipFree(ss->d_t0tbg); (void)hipFree(ss->d_rowsq); (void)hipFree(ss->d_totsq); (void)hipFree(ss->d_lines);
    for (const SetBuf &b : SET_BUFS) (void)hipFree(ss->*b.p);
    (void)hipFree(ss->d_lte); (void)hipFree(ss->d_band); (void)hipFree(ss->d_mix);
    (void)hipFree(ss->d_grid); (void)hipFree(ss->d_grid_tex); (void)hipFree(ss->d_grid_ltau);
    delete ss;
    return NFA_OK;
}

// What the nfa_specset_set_* calls do before they change a set: held batches were accepted for the old likelihood, launches
// in flight read the buffers changed there, and a runner's captured single-point graph holds the old SpecDev
static int specset_quiesce(nfa_specset *ss) {
    int rc = flush_all_runners(); if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    std::lock_guard<std::mutex> lk(g_runners_m);
    for (nfa_runner *r : g_runners)
        if (r->ss == ss) { RUNNER_LOCK(r); if (r->g1) { (void)hipGraphExecDestroy(r->g1); r->g1 = nullptr; } }
    return NFA_OK;
}

// The entries of R^-1 (NFA_CORR_NC of them) of the unit-variance AR(2) process with autocorrelations (r1, r2) by Yule-Walker;
// false if the pair is outside the domain, `why` then says how
static bool corr_coef(double r1, double r2, double *c, const char **why) {
    if (!std::isfinite(r1) || !std::isfinite(r2)) { *why = "a noise correlation is a pair of finite numbers (rho_1, rho_2) per spectrum"; return false; }
    if (!(std::fabs(r1) < 1.0)) { *why = "a noise correlation needs |rho_1| < 1"; return false; }
    if (!(r2 > 2.0 * r1 * r1 - 1.0 && r2 < 1.0)) { *why = "a noise correlation needs 2 rho_1^2 - 1 < rho_2 < 1 (a positive definite correlation matrix)"; return false; }
    const double den = 1.0 - r1 * r1;
    const double f1 = r1 * (1.0 - r2) / den, f2 = (r2 - r1 * r1) / den;
    const double v = 1.0 - f1 * r1 - f2 * r2;
    if (!(v >= 0.01)) { *why = "a noise correlation needs an innovations variance v >= 0.01: the noise is nearly determined by its neighbours"; return false; }
    c[0] = 1.0 / v; c[1] = (1.0 + f1 * f1) / v; c[2] = (1.0 + f1 * f1 + f2 * f2) / v;
    c[3] = -f1 / v; c[4] = -f1 * (1.0 - f2) / v; c[5] = -f2 / v;
    return true;
}

// The one allocation of an option's buffer
static int set_alloc(double **p, size_t doubles, const char *oom) {
#ifdef NFA_TEST_HOOKS
    if (test_alloc_fails()) return fail(NFA_ERR_DEVICE, oom);
#endif
    if (hipMalloc(p, sizeof(double) * doubles) != hipSuccess) { (void)hipGetLastError(); *p = nullptr; return fail(NFA_ERR_DEVICE, oom); }
    return NFA_OK;
}

// SpecDev's pointers as layout L of options o names them.  base: chan_w and wdata of a robust set at what lies beneath g, the
// set's own weights (a scalar noise: none) -- the state launch_rowsq forms its sums from before rob_setup_kernel turns them into k C.
static void specset_point(nfa_specset *ss, const SetOptions &o, const SetLayout &L, bool base) {
    SpecDev &d = ss->dev;
    const bool own = L.chan_w == CHAN_W_OWN || (L.chan_w == CHAN_W_ROBUST && (base && L.has(SB_W)));
    const bool rob = L.chan_w == CHAN_W_ROBUST && !base;
    d.chan_w = L.chan_w == CHAN_W_Q ? ss->d_q0 : own ? ss->d_w : rob ? ss->d_rg : nullptr;
    d.wdata = L.chan_w == CHAN_W_Q || own ? ss->d_wdata : rob ? ss->d_rgd : nullptr;
    d.bl = L.has(SB_BL) ? ss->d_bl : nullptr;
    d.bl_order = o.bl_order;
    d.tmpl = L.has(SB_TMPL) ? ss->d_tmpl : nullptr;
    d.tp = L.has(SB_TP) ? ss->d_tp : nullptr;
    d.cal2 = L.has(SB_CAL2) ? ss->d_cal2 : nullptr;
    d.nmarg = L.has(SB_NMARG) ? ss->d_nmarg : nullptr;
    d.corr_q1 = L.has(SB_Q1) ? ss->d_q1 : nullptr;
    d.corr_q2 = L.has(SB_Q2) ? ss->d_q2 : nullptr;
    d.corr_coef = L.has(SB_CORR) ? ss->d_corr : nullptr;
    d.resp = L.has(SB_RESP) ? ss->d_resp : nullptr;
    d.cont = L.has(SB_CONT) ? ss->d_cont : nullptr;
    d.rob = rob ? ss->d_rob : nullptr;
}

// The device state of record `next`, whatever the set holds now, for pixels [pix0, pix0 + n): `work` is the copies and
// forming stages to run (set_stages_*, nfa_set_state.h).  Three phases.  1. Allocate every buffer the layout needs that is not
// there; a failure frees what this call allocated and returns with nothing the kernels read touched.  2. Copy the small
// arrays up, point SpecDev at the layout's buffers and run the stages in their order; *touched says this phase began.
// 3. Free what the layout does not need.  A call turns one option on or off, so its peak memory is max(before, after).
// `sigmas`: the caller's noise per channel [n_pix][chan_tot] for ST_FORM_W, the stage of a set's creation.
static int specset_realise(nfa_specset *ss, const SetRecord &next, int64_t pix0, int64_t n, unsigned work, bool *touched = nullptr,
                           const double *sigmas = nullptr) {
    SpecDev &d = ss->dev;
    const SetOptions &o = next.o;
    const SetLayout L = set_layout(o, ss->chan_noise);
    double *made[SB_N] = {};
    for (int i = 0; i < SB_N; ++i) {
        const SetBuf &b = SET_BUFS[i];
        if (!L.has(b.bit) || ss->*b.p) continue;
        const int rc = set_alloc(&made[i], set_buf_doubles(ss, b.bit), b.oom);
        if (rc) { for (double *m : made) (void)hipFree(m); return rc; }
    }
    for (int i = 0; i < SB_N; ++i) if (made[i]) ss->*SET_BUFS[i].p = made[i];

    if (touched) *touched = true;
    const size_t chan = (size_t)d.chan_tot, all = (size_t)(ss->n_pix * d.chan_tot);
    if (work & UP_CAL2) {
        double s2[MAXSPEC];
        for (int s = 0; s < d.n_spec; ++s) s2[s] = o.cal[s] * o.cal[s];
        HIP_TRY(hipMemcpy(ss->d_cal2, s2, sizeof(double) * d.n_spec, hipMemcpyHostToDevice));
    }
    if (work & UP_CORR) {             // white noise in a spectrum (and everywhere under a response alone): R = 1
        double coef[MAXSPEC][NFA_CORR_NC];
        for (int s = 0; s < d.n_spec; ++s) {
            const char *why = nullptr;
            if ((o.rho[s][0] == 0.0 && o.rho[s][1] == 0.0) || !corr_coef(o.rho[s][0], o.rho[s][1], coef[s], &why)) {
                coef[s][0] = coef[s][1] = coef[s][2] = 1.0; coef[s][3] = coef[s][4] = coef[s][5] = 0.0;
            }
        }
        HIP_TRY(hipMemcpy(ss->d_corr, coef, sizeof(double) * NFA_CORR_NC * d.n_spec, hipMemcpyHostToDevice));
    }
    if (work & UP_RESP) HIP_TRY(hipMemcpy(ss->d_resp, o.resp, sizeof(double) * NFA_RESP_NT * d.n_spec, hipMemcpyHostToDevice));
    if (work & UP_TMPL) {             // each template goes up scaled to max |t| = 1 over its spectrum
        std::vector<double> scaled(NFA_TMPL_MAX * chan, 0.0);
        for (int s = 0; s < d.n_spec; ++s)
            for (int k = 0; k < o.ntmpl[s]; ++k) {
                const double *t = next.tmpl.data() + k * chan + d.off[s];
                double top = 0.0;
                for (int j = 0; j < d.size[s]; ++j) top = std::max(top, std::fabs(t[j]));
                for (int j = 0; j < d.size[s]; ++j) scaled[k * chan + d.off[s] + j] = t[j] / top;
            }
        HIP_TRY(hipMemcpy(ss->d_tmpl, scaled.data(), sizeof(double) * scaled.size(), hipMemcpyHostToDevice));
    }
    if (work & UP_CONT) HIP_TRY(hipMemcpy(ss->d_cont, next.cont.data(), sizeof(double) * next.cont.size(), hipMemcpyHostToDevice));
    specset_point(ss, o, L, true);
    int rc = NFA_OK;
    if (work & ST_ONES) {             // a scalar noise runs as the weighted form with w == 1: its bits
        std::vector<double> one(all, 1.0);
        HIP_TRY(hipMemcpy(ss->d_w, one.data(), sizeof(double) * all, hipMemcpyHostToDevice));
    }
    if (work & ST_FORM_W) HIP_TRY(hipMemcpy(ss->d_w, sigmas, sizeof(double) * all, hipMemcpyHostToDevice));       // creation alone
    if (work & ST_CHAN_WEIGHT) { rc = launch_chan_weight(ss, pix0, n, (work & ST_FORM_W) != 0); if (rc) return rc; }      // (otherwise the mask stays)
    if (work & ST_CORR) { rc = launch_corr_setup(ss, pix0, n, (work & ST_FORM_Q) != 0); if (rc) return rc; }
    if (work & ST_ROWSQ) { rc = launch_rowsq(ss, pix0, n); if (rc) return rc; }
    if (work & ST_ROB) {              // g, g d, totsq = k C and the records; the spectra with nu = 0 keep the sums beneath
        // (the kernel reads the set's data, noise, sizes and offsets and its own arguments, neither S.chan_w nor S.wdata:
        // that `d` still points at the base here is nothing to it)
        RobNu nu_of = {};
        for (int s = 0; s < d.n_spec; ++s) nu_of.nu[s] = o.rob[s];
        hipLaunchKernelGGL(rob_setup_kernel, dim3((unsigned)((n * d.n_spec * 64 + 255) / 256)), dim3(256), 0, 0, d, (long)pix0, (long)n,
                           (const double *)ss->d_w, nu_of, ss->d_rg, ss->d_rgd, ss->d_totsq, ss->d_rob);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
    }
    specset_point(ss, o, L, false);
    if (work & ST_BL) { rc = launch_bl_setup(ss, pix0, n, (work & ST_BL_BASIS) != 0); if (rc) return rc; }
    if (work & ST_TP) { rc = launch_tmpl_setup(ss, pix0, n, (work & ST_TP_BASIS) != 0); if (rc) return rc; }
    if (work & ST_NMARG) {            // {a, a + nu / 2} of every (pixel, spectrum), nu the channels whose own weight is > 0
        NmargA a_of = {};
        for (int s = 0; s < d.n_spec; ++s) a_of.a[s] = o.nunc[s] > 0.0 ? 1.0 / (4.0 * o.nunc[s] * o.nunc[s]) : 0.0;
        const int64_t spec = ss->n_pix * d.n_spec;
        hipLaunchKernelGGL(nmarg_setup_kernel, dim3((unsigned)((spec * 64 + 255) / 256)), dim3(256), 0, 0, d, (long)ss->n_pix,
                           (const double *)ss->d_w, a_of, ss->d_nmarg);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
    }

    for (const SetBuf &b : SET_BUFS)
        if (!L.has(b.bit) && ss->*b.p) { (void)hipFree(ss->*b.p); ss->*b.p = nullptr; }
    return NFA_OK;
}

static int upload(void *dst, const void *src, size_t bytes) {          // dst: where the device pointer goes
    HIP_TRY(hipMalloc((void **)dst, bytes));
    HIP_TRY(hipMemcpy(*(void **)dst, src, bytes, hipMemcpyHostToDevice));
    return NFA_OK;
}
// A set from its declaration.  The header's part first (nfa_set_decl.h: every check and every host-side record, no device
// call), then the device: the base arrays go up, and the rest is specset_realise of the empty options record with every stage
// -- for a noise per channel the weights' buffers, w from the sigmas and w d, for every set the sums.
static int specset_upload(nfa_specset *ss, const SetDecl &decl, const SetPlan &p) {
    SpecDev &d = ss->dev;
    d.n_spec = p.n_spec; d.model = p.model; d.npar = p.npar; d.chan_tot = p.chan_tot; d.rows_tot = p.rows_tot;
    memcpy(d.rest, p.rest, sizeof d.rest); memcpy(d.size, p.size, sizeof d.size); memcpy(d.trans, p.trans, sizeof d.trans);
    memcpy(d.off, p.off, sizeof d.off); memcpy(d.row_off, p.row_off, sizeof d.row_off); memcpy(d.nu_min, p.nu_min, sizeof d.nu_min);
    memcpy(d.nu_chan, p.nu_chan, sizeof d.nu_chan); memcpy(d.r_chan, p.r_chan, sizeof d.r_chan);
    ss->n_pix = p.n_pix; ss->nhf_max = p.nhf_max; memcpy(ss->h_nhf, p.h_nhf, sizeof ss->h_nhf);
    ss->filled = p.filled; ss->chan_noise = p.chan_noise; ss->masked = p.masked;
    const int64_t tot = p.chan_tot, spec = p.n_pix * p.n_spec;
    std::vector<double> xcat(tot);
    for (int s = 0; s < p.n_spec; ++s) memcpy(xcat.data() + p.off[s], decl.xarr[s], sizeof(double) * p.size[s]);
    // (the allocations in the order they always had: where the buffers lie relative to each other is part of the likelihood's speed)
    for (double **b : {&ss->d_xarr, &ss->d_t0, &ss->d_tbg, &ss->d_t0tbg}) HIP_TRY(hipMalloc(b, sizeof(double) * tot));
    HIP_TRY(hipMalloc(&ss->d_data, sizeof(double) * tot * p.n_pix));
    HIP_TRY(hipMalloc(&ss->d_noise, sizeof(double) * spec));
    HIP_TRY(hipMalloc(&ss->d_rowsq, sizeof(double) * p.rows_tot * p.n_pix));
    HIP_TRY(hipMalloc(&ss->d_totsq, sizeof(double) * spec));
    HIP_TRY(hipMemcpy(ss->d_xarr, xcat.data(), sizeof(double) * tot, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ss->d_data, decl.data, sizeof(double) * tot * p.n_pix, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ss->d_noise, p.chan_noise ? p.sigma_ref.data() : decl.noise, sizeof(double) * spec, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(prep_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, 0,
                       ss->d_xarr, ss->d_t0, ss->d_tbg, ss->d_t0tbg, (long)tot);
    HIP_TRY(hipGetLastError());
    d.xarr = ss->d_xarr; d.t0 = ss->d_t0; d.tbg = ss->d_tbg; d.data = ss->d_data; d.noise = ss->d_noise;
    d.t0tbg = ss->d_t0tbg; d.rowsq = ss->d_rowsq; d.totsq = ss->d_totsq;
    int rc = upload(&ss->d_lines, p.lines, sizeof(LineRow) * p.n_spec); if (rc) return rc;
    d.lines = ss->d_lines;
    if (p.kind >= SET_LTE) { rc = upload(&ss->d_lte, &p.lte, sizeof p.lte); if (rc) return rc; d.lte_rec = ss->d_lte; }
    if (p.kind >= SET_BANDS) { rc = upload(&ss->d_band, &p.band, sizeof p.band); if (rc) return rc; d.band = ss->d_band; }
    if (p.kind == SET_MIX) { rc = upload(&ss->d_mix, &p.mix, sizeof p.mix); if (rc) return rc; d.mix = ss->d_mix; }
    if (p.grid) {                 // the tables, then the record that points at them; the set's kernels are the baseline form's
        const size_t bytes = sizeof(double) * (size_t)p.grid_rec.nt * p.grid_rec.nn * p.grid_rec.nc * p.n_spec;
        rc = upload(&ss->d_grid_tex, decl.g_tex, bytes); if (rc) return rc;
        rc = upload(&ss->d_grid_ltau, decl.g_ltau, bytes); if (rc) return rc;
        GridRec rec = p.grid_rec;
        rec.tex = ss->d_grid_tex; rec.ltau = ss->d_grid_ltau;
        rc = upload(&ss->d_grid, &rec, sizeof rec); if (rc) return rc;
        d.grid = ss->d_grid;
        ss->opt.o.grid_on = true;
    }
    return specset_realise(ss, ss->opt, 0, p.n_pix, set_stages_create(set_layout(ss->opt.o, p.chan_noise)), nullptr, decl.chan_noise);
}
static int specset_build(nfa_specset **out, const SetDecl &decl) {
    SetPlan p; std::string why;
    int rc = set_plan(decl, p, why); if (rc) return fail(rc, why);
    rc = engine_init(); if (rc) return rc;
    nfa_specset *ss = new nfa_specset();
    rc = specset_upload(ss, decl, p);
    if (rc) { nfa_specset_destroy(ss); return rc; }          // frees whatever was allocated
    *out = ss;
    return NFA_OK;
}

// The shared body of the setters, after a setter's value checks and the table's refusal: the set becomes `next`, or stays as
// it was -- a failed allocation touches nothing, and after a failed copy or launch the old record is realised once more with
// every stage (the first error's text stays).
static int specset_change(nfa_specset *ss, SetRecord &next) {
    int rc = engine_init(); if (rc) return rc;
    rc = specset_quiesce(ss); if (rc) return rc;
    const auto differ = [](const std::vector<double> &a, const std::vector<double> &b) {      // bit for bit, like set_options_equal
        return a.size() != b.size() || (!a.empty() && memcmp(a.data(), b.data(), sizeof(double) * a.size()) != 0);
    };
    const bool tmpl_changed = differ(next.tmpl, ss->opt.tmpl), cont_changed = differ(next.cont, ss->opt.cont);
    if (set_options_equal(next.o, ss->opt.o) && !tmpl_changed && !cont_changed) return NFA_OK;
    const SetLayout la = set_layout(ss->opt.o, ss->chan_noise), lb = set_layout(next.o, ss->chan_noise);
    bool touched = false;
    rc = specset_realise(ss, next, 0, ss->n_pix, set_stages_change(ss->opt.o, la, next.o, lb, tmpl_changed, cont_changed), &touched);
    if (rc == NFA_OK) { ss->opt = std::move(next); return NFA_OK; }
    if (touched) {
        const std::string why = g_err;
        (void)specset_realise(ss, ss->opt, 0, ss->n_pix, set_stages_all(la));
        g_err = why;
    }
    return rc;
}

int nfa_specset_set_data(nfa_specset *ss, int64_t pix, const double *data) {
    if (!ss || !data || pix < 0 || pix >= ss->n_pix) return fail(NFA_ERR_ARG, "bad pixel index");
    int rc = engine_init(); if (rc) return rc;
    HIP_TRY(hipMemcpy(ss->d_data + pix * ss->dev.chan_tot, data, sizeof(double) * ss->dev.chan_tot,
                      hipMemcpyHostToDevice));
    return specset_realise(ss, ss->opt, pix, 1, set_stages_data(set_layout(ss->opt.o, ss->chan_noise)));
}

// What the set has, as set_refusal (nfa_set_rules.h) asks: which of the likelihoods a setter may not put beside its own
static unsigned specset_has(const nfa_specset *ss) { return set_has(ss->opt.o, ss->masked); }
// A set of the excitation-grid model runs a side of its own (LNL_SIDE_TEXS) and a side is exclusive: the setters of the other
// sides' options, and of a calibration, refuse it by its model, as nfa_specset_set_layered refuses the Gaussian model
// (`what`: "nuisance templates", ...).  nfa_set_rules.h stays the table of option pairs.
static bool grid_refuses(const nfa_specset *ss, const char *what) {
    if (ss->dev.model != NFA_MODEL_GRID) return false;
    fail(NFA_ERR_ARG, std::string("a set of the excitation-grid model takes no ") + what);
    return true;
}

// A setter: null check, its value check (`any`: the request switches the option on), the table's refusal, a copy of the
// record with its one field edited, specset_change.
int nfa_specset_set_baseline(nfa_specset *ss, int order) {
    if (!ss) return fail(NFA_ERR_ARG, "null argument");
    if (order < -1 || order > NFA_BASELINE_MAX) return fail(NFA_ERR_ARG, "baseline order must be in -1..3 (-1: none)");
    if (const char *why = order >= 0 ? set_refusal(specset_has(ss), SET_TAKES_BASELINE) : nullptr) return fail(NFA_ERR_ARG, why);
    SetRecord next = ss->opt;
    next.o.bl_order = order;
    return specset_change(ss, next);
}

// the per-spectrum values of a request into their field of the record: vals[n_spec][width] if `any`, zeros otherwise
static void set_field(double *field, size_t bytes, bool *has, bool any, const double *vals, int n) {
    memset(field, 0, bytes);
    if (any) memcpy(field, vals, sizeof(double) * n);
    *has = any;
}

int nfa_specset_set_calibration(nfa_specset *ss, const double *cal) {
    if (!ss) return fail(NFA_ERR_ARG, "null argument");
    bool any = false;
    for (int s = 0; cal && s < ss->dev.n_spec; ++s) {
        if (!(cal[s] >= 0.0 && cal[s] <= 1.0))                // (NaN fails both)
            return fail(NFA_ERR_ARG, "a calibration uncertainty is a finite fraction in [0, 1] per spectrum");
        any = any || cal[s] > 0.0;
    }
    if (any && grid_refuses(ss, "calibration uncertainty")) return NFA_ERR_ARG;
    if (const char *why = any ? set_refusal(specset_has(ss), SET_TAKES_CALIB) : nullptr) return fail(NFA_ERR_ARG, why);
    SetRecord next = ss->opt;                                 // (null, or all zeros: the set's former kernels and bits)
    set_field(next.o.cal, sizeof next.o.cal, &next.o.cal_on, any, cal, ss->dev.n_spec);
    return specset_change(ss, next);
}

int nfa_specset_calibration(const nfa_specset *ss, double *out) {
    if (!ss || !ss->opt.o.cal_on) return 0;
    for (int s = 0; out && s < ss->dev.n_spec; ++s) out[s] = ss->opt.o.cal[s];
    return 1;
}

int nfa_specset_set_noise_uncertainty(nfa_specset *ss, const double *f) {
    if (!ss) return fail(NFA_ERR_ARG, "null argument");
    bool any = false;
    for (int s = 0; f && s < ss->dev.n_spec; ++s) {
        if (!(f[s] >= 0.0 && f[s] <= 0.5))                    // (NaN fails both)
            return fail(NFA_ERR_ARG, "a noise uncertainty is a finite fraction in [0, 0.5] per spectrum");
        any = any || f[s] > 0.0;
    }
    if (const char *why = any ? set_refusal(specset_has(ss), SET_TAKES_NMARG) : nullptr) return fail(NFA_ERR_ARG, why);
    SetRecord next = ss->opt;                                 // (null, or all zeros: the set's former arithmetic and bits)
    set_field(next.o.nunc, sizeof next.o.nunc, &next.o.nunc_on, any, f, ss->dev.n_spec);
    return specset_change(ss, next);
}

int nfa_specset_noise_uncertainty(const nfa_specset *ss, double *out) {
    if (!ss || !ss->opt.o.nunc_on) return 0;
    for (int s = 0; out && s < ss->dev.n_spec; ++s) out[s] = ss->opt.o.nunc[s];
    return 1;
}

int nfa_specset_set_correlation(nfa_specset *ss, const double *rho) {
    if (!ss) return fail(NFA_ERR_ARG, "null argument");
    const SpecDev &d = ss->dev;
    double coef[NFA_CORR_NC];
    bool any = false;
    for (int s = 0; rho && s < d.n_spec; ++s) {
        const double r1 = rho[2 * s], r2 = rho[2 * s + 1];
        if (r1 == 0.0 && r2 == 0.0) continue;                 // white noise in this spectrum: R = 1
        const char *why = nullptr;
        if (!corr_coef(r1, r2, coef, &why)) return fail(NFA_ERR_ARG, why);
        any = true;
    }
    if (any) {
        for (int s = 0; s < d.n_spec; ++s)
            if (d.size[s] < 4) return fail(NFA_ERR_ARG, "a noise correlation needs spectra of 4 channels and more");
        if (grid_refuses(ss, "noise correlation")) return NFA_ERR_ARG;
        if (const char *why = set_refusal(specset_has(ss), SET_TAKES_CORR)) return fail(NFA_ERR_ARG, why);
    }
    SetRecord next = ss->opt;         // (null, or all zeros: the set's former kernels and bits, or a response's over white noise)
    set_field(&next.o.rho[0][0], sizeof next.o.rho, &next.o.corr_on, any, rho, 2 * d.n_spec);
    return specset_change(ss, next);
}

int nfa_specset_correlation(const nfa_specset *ss, double *out) {
    if (!ss || !ss->opt.o.corr_on) return 0;
    if (out) memcpy(out, ss->opt.o.rho, sizeof(double) * 2 * ss->dev.n_spec);
    return 1;
}

int nfa_specset_set_response(nfa_specset *ss, const double *taps) {
    if (!ss) return fail(NFA_ERR_ARG, "null argument");
    const SpecDev &d = ss->dev;
    bool any = false;
    for (int s = 0; taps && s < d.n_spec; ++s) {
        const double *h = taps + s * NFA_RESP_NT;
        double sum = 0.0;
        for (int k = 0; k < NFA_RESP_NT; ++k) {
            if (!std::isfinite(h[k])) return fail(NFA_ERR_ARG, "a channel response is five finite taps per spectrum");
            sum += h[k];
        }
        if (!(std::fabs(sum - 1.0) <= 1e-9)) return fail(NFA_ERR_ARG, "the taps of a channel response sum to 1 (within 1e-9): it conserves the integrated intensity");
        if (!(h[2] > 0.0)) return fail(NFA_ERR_ARG, "a channel response needs a central tap > 0");
        any = any || !(h[0] == 0.0 && h[1] == 0.0 && h[2] == 1.0 && h[3] == 0.0 && h[4] == 0.0);
    }
    if (any) {
        for (int s = 0; s < d.n_spec; ++s)
            if (d.size[s] < 4) return fail(NFA_ERR_ARG, "a channel response needs spectra of 4 channels and more");
        if (grid_refuses(ss, "channel response")) return NFA_ERR_ARG;
        if (const char *why = set_refusal(specset_has(ss), SET_TAKES_RESP)) return fail(NFA_ERR_ARG, why);
    }
    SetRecord next = ss->opt;         // (null, or the identity everywhere: the correlated set's kernels and bits, or the set's former ones)
    set_field(&next.o.resp[0][0], sizeof next.o.resp, &next.o.resp_on, any, taps, NFA_RESP_NT * d.n_spec);
    return specset_change(ss, next);
}

int nfa_specset_response(const nfa_specset *ss, double *out) {
    if (!ss || !ss->opt.o.resp_on) return 0;
    if (out) memcpy(out, ss->opt.o.resp, sizeof(double) * NFA_RESP_NT * ss->dev.n_spec);
    return 1;
}

int nfa_specset_set_templates(nfa_specset *ss, const double *t, const int *n_tmpl) {
    if (!ss) return fail(NFA_ERR_ARG, "null argument");
    const SpecDev &d = ss->dev;
    const size_t n = (size_t)d.chan_tot;
    bool any = false;
    for (int s = 0; t && n_tmpl && s < d.n_spec; ++s) {
        if (n_tmpl[s] < 0 || n_tmpl[s] > NFA_TMPL_MAX) return fail(NFA_ERR_ARG, "nuisance templates: 0..4 templates per spectrum");
        any = any || n_tmpl[s] > 0;
    }
    std::vector<double> vals;
    if (any) {
        vals.assign(NFA_TMPL_MAX * n, 0.0);                   // the slots in use alone are read
        for (int s = 0; s < d.n_spec; ++s)
            for (int k = 0; k < n_tmpl[s]; ++k) {
                const double *v = t + k * n + d.off[s];
                bool zero = true;
                for (int j = 0; j < d.size[s]; ++j) {
                    if (!std::isfinite(v[j])) return fail(NFA_ERR_ARG, "nuisance templates: every value is finite");
                    zero = zero && v[j] == 0.0;
                    vals[k * n + d.off[s] + j] = v[j];
                }
                if (zero) return fail(NFA_ERR_ARG, "nuisance templates: a template is zero over its whole spectrum");
            }
        if (grid_refuses(ss, "nuisance templates")) return NFA_ERR_ARG;
        if (const char *why = set_refusal(specset_has(ss), SET_TAKES_TMPL)) return fail(NFA_ERR_ARG, why);
    }
    SetRecord next = ss->opt;
    next.o.tmpl_on = any;
    for (int s = 0; s < MAXSPEC; ++s) next.o.ntmpl[s] = any && s < d.n_spec ? n_tmpl[s] : 0;
    next.tmpl.swap(vals);
    return specset_change(ss, next);
}

int nfa_specset_templates(const nfa_specset *ss, double *out_t, int *out_n) {
    if (!ss || !ss->opt.o.tmpl_on) return 0;
    if (out_t) memcpy(out_t, ss->opt.tmpl.data(), sizeof(double) * ss->opt.tmpl.size());
    for (int s = 0; out_n && s < ss->dev.n_spec; ++s) out_n[s] = ss->opt.o.ntmpl[s];
    return 1;
}

int nfa_specset_set_continuum(nfa_specset *ss, const double *tc) {
    if (!ss) return fail(NFA_ERR_ARG, "null argument");
    const int64_t n = ss->n_pix * ss->dev.n_spec;
    bool any = false;
    for (int64_t i = 0; tc && i < n; ++i) {
        if (!(tc[i] >= 0.0 && tc[i] < INFINITY))              // (NaN fails both)
            return fail(NFA_ERR_ARG, "a continuum background is a finite brightness temperature >= 0 K per (pixel, spectrum)");
        any = any || tc[i] > 0.0;
    }
    if (any) {
        if (ss->dev.model == NFA_MODEL_GAUSSIAN)
            return fail(NFA_ERR_ARG, "the Gaussian model has no optical depth: its components cannot absorb a continuum background");
        if (grid_refuses(ss, "continuum background")) return NFA_ERR_ARG;
        if (const char *why = set_refusal(specset_has(ss), SET_TAKES_CONT)) return fail(NFA_ERR_ARG, why);
    }
    SetRecord next = ss->opt;
    next.o.cont_on = any;
    if (any) next.cont.assign(tc, tc + n); else next.cont.clear();
    return specset_change(ss, next);
}

int nfa_specset_continuum(const nfa_specset *ss, double *out) {
    if (!ss || !ss->opt.o.cont_on) return 0;
    if (out) memcpy(out, ss->opt.cont.data(), sizeof(double) * ss->opt.cont.size());
    return 1;
}

int nfa_specset_set_robust(nfa_specset *ss, const double *nu) {
    if (!ss) return fail(NFA_ERR_ARG, "null argument");
    bool any = false;
    for (int s = 0; nu && s < ss->dev.n_spec; ++s) {
        if (!(nu[s] == 0.0 || (nu[s] >= 1.0 && nu[s] <= 1e6)))   // (NaN fails all)
            return fail(NFA_ERR_ARG, "a robust likelihood takes finite degrees of freedom per spectrum, 0 (Gaussian) or in [1, 1e6]");
        any = any || nu[s] > 0.0;
    }
    if (any && grid_refuses(ss, "robust likelihood")) return NFA_ERR_ARG;
    if (const char *why = any ? set_refusal(specset_has(ss), SET_TAKES_ROBUST) : nullptr) return fail(NFA_ERR_ARG, why);
    SetRecord next = ss->opt;                                 // (null, or all zeros: the set's former kernels and bits)
    set_field(next.o.rob, sizeof next.o.rob, &next.o.rob_on, any, nu, ss->dev.n_spec);
    return specset_change(ss, next);
}

int nfa_specset_robust(const nfa_specset *ss, double *out) {
    if (!ss || !ss->opt.o.rob_on) return 0;
    for (int s = 0; out && s < ss->dev.n_spec; ++s) out[s] = ss->opt.o.rob[s];
    return 1;
}

int nfa_specset_set_layered(nfa_specset *ss, int on) {
    if (!ss) return fail(NFA_ERR_ARG, "null argument");
    if (ss->dev.model == NFA_MODEL_GAUSSIAN)
        return fail(NFA_ERR_ARG, "the Gaussian model has no optical depth: its components cannot absorb one another (no layered transfer)");
    int rc = engine_init(); if (rc) return rc;
    // as nfa_specset_set_baseline: held batches were accepted for the old likelihood, launches in flight were planned for
    // it, and a runner's captured single-point graph holds the old kernel
    rc = specset_quiesce(ss); if (rc) return rc;
    ss->layered = on != 0;
    return NFA_OK;
}

int nfa_specset_layered(const nfa_specset *ss) { return ss && ss->layered ? 1 : 0; }

int nfa_specset_null_lnz(const nfa_specset *ss, double *out) {
    if (!ss || !out) return fail(NFA_ERR_ARG, "null argument");
    const int64_t n = ss->n_pix * ss->dev.n_spec;
    double *d_out = nullptr;
    HIP_TRY(hipMalloc(&d_out, sizeof(double) * n));
    const SetOptions &o = ss->opt.o;
    if (o.rob_on)                                            // the likelihood kernel's own value at p = 0
        hipLaunchKernelGGL(null_lnz_rob_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, ss->dev, (long)ss->n_pix, d_out);
    else if (o.tmpl_on)                                      // the model of baseline and templates alone
        hipLaunchKernelGGL(null_lnz_tmpl_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, ss->dev, (long)ss->n_pix, d_out);
    else if (o.bl_order >= 0)                                 // the baseline-only model (a calibrated set's zeroed record is no baseline)
        hipLaunchKernelGGL(null_lnz_bl_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, ss->dev, (long)ss->n_pix, d_out);
    else
        hipLaunchKernelGGL(set_layout(o, ss->chan_noise).chan_w != CHAN_W_NONE ? null_lnz_w_kernel : null_lnz_kernel,
                           dim3((unsigned)((n * 64 + 255) / 256)), dim3(256), 0, 0, ss->dev, (long)ss->n_pix, d_out);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && o.nunc_on) {                      // an uncertain noise level: lnl_of_item's term of the same h
        hipLaunchKernelGGL(null_lnz_nmarg_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, ss->dev.nmarg, (long)n, d_out);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out, d_out, sizeof(double) * n, hipMemcpyDeviceToHost);
    (void)hipFree(d_out);                                     // on every path
    if (e != hipSuccess) return fail(NFA_ERR_DEVICE, std::string("nfa_specset_null_lnz: ") + hipGetErrorString(e));
    return NFA_OK;
}

int nfa_specset_tbg(const nfa_specset *ss, double *out) {
    if (!ss || !out) return fail(NFA_ERR_ARG, "null argument");
    HIP_TRY(hipMemcpy(out, ss->d_tbg, sizeof(double) * ss->dev.chan_tot, hipMemcpyDeviceToHost));
    return NFA_OK;
}

int64_t nfa_specset_chan_tot(const nfa_specset *ss) { return ss ? ss->dev.chan_tot : 0; }

// ---- priors ----------------------------------------------------------------
static int priors_fill(nfa_priors *p, const nfa_prior_desc *priors, int n_prior, const nfa_dist_desc *dists,
                       int n_dist, int n_param) {
    PriorProg &g = p->prog;
    g.n_prior = n_prior; g.n_dist = n_dist; g.n_param = n_param; g.max_size = 2;
    for (int k = 0; k < n_prior; ++k) {
        g.pr[k] = priors[k];
        const int dd[3] = {priors[k].dist0, priors[k].dist1, priors[k].dist2};
        for (int q = 0; q < 3; ++q)
            if (dd[q] >= n_dist) return fail(NFA_ERR_ARG, "distribution index out of range");
        if (priors[k].p_ix < 0) return fail(NFA_ERR_ARG, "p_ix must be >= 0");   // core.pyx:186
    }
    auto upload = [&](const double *src, int64_t n, const double **dst) -> int {
        double *dp = nullptr;
        HIP_TRY(hipMalloc(&dp, sizeof(double) * n));
        p->d_arrays.push_back(dp);                 // owned from here on: nfa_priors_destroy frees it
        HIP_TRY(hipMemcpy(dp, src, sizeof(double) * n, hipMemcpyHostToDevice));
        *dst = dp;
        return NFA_OK;
    };
    std::vector<std::array<std::vector<double>, 3>> moments;      // host copies, for the staging image below
    for (int k = 0; k < n_dist; ++k) {
        const nfa_dist_desc &s = dists[k];
        if (s.size < 2 || s.size > 65536) return fail(NFA_ERR_ARG, "distribution size out of range");
        DistDev &d = g.ds[k];
        d.size = (int)s.size; d.du = s.du; d.dx = s.dx; d.xmin = s.xmin; d.xmax = s.xmax;
        const double *src[4] = {s.xax, s.pdf, s.cdf, s.ppf};
        const double **dst[4] = {&d.xax, &d.pdf, &d.cdf, &d.ppf};
        for (int q = 0; q < 4; ++q) { int rc = upload(src[q], s.size, dst[q]); if (rc) return rc; }
        // prefix moments of the trapezoid terms (long double accumulation, one rounding each)
        std::vector<double> m0(s.size), m1(s.size), m2(s.size);
        long double a0 = 0, a1 = 0, a2 = 0;
        m0[0] = m1[0] = m2[0] = 0.0;
        for (int64_t i = 1; i < s.size; ++i) {
            const long double ti = 0.5L * ((long double)s.pdf[i] + (long double)s.pdf[i - 1]);
            const long double ic = (long double)(i - s.size / 2);
            a0 += ti; a1 += ti * ic; a2 += ti * ic * ic;
            m0[i] = (double)a0; m1[i] = (double)a1; m2[i] = (double)a2;
        }
        const double *msrc[3] = {m0.data(), m1.data(), m2.data()};
        const double **mdst[3] = {&d.m0, &d.m1, &d.m2};
        for (int q = 0; q < 3; ++q) { int rc = upload(msrc[q], s.size, mdst[q]); if (rc) return rc; }
        g.max_size = std::max(g.max_size, (int)s.size);
        moments.push_back({std::move(m0), std::move(m1), std::move(m2)});
    }
    // tables the set-up kernel keeps in LDS: ppf of every distribution a prior interpolates, and the
    // abscissa + prefix moments (+ pdf, for more than three components) of a placement prior's distribution
    {
        bool need[MAXDIST][6] = {};
        for (int k = 0; k < n_prior; ++k) {
            const nfa_prior_desc &q = priors[k];
            const bool composite = q.kind == NFA_PRIOR_RESOLVED_CENSEP || q.kind == NFA_PRIOR_RESOLVED_PLACEMENT;
            if (q.kind != NFA_PRIOR_CONSTANT && q.dist0 >= 0) need[q.dist0][ST_PPF] = true;
            if ((q.kind == NFA_PRIOR_SPACED || q.kind == NFA_PRIOR_CENSEP || q.kind == NFA_PRIOR_RESOLVED_CENSEP) && q.dist1 >= 0)
                need[q.dist1][ST_PPF] = true;
            if (composite && q.sub_kind != NFA_PRIOR_CONSTANT && q.dist2 >= 0) need[q.dist2][ST_PPF] = true;
            if (q.kind == NFA_PRIOR_RESOLVED_PLACEMENT && q.dist0 >= 0)
                for (int f : {ST_XAX, ST_PDF, ST_M0, ST_M1, ST_M2}) need[q.dist0][f] = true;
        }
        int n = 0, off = 0;
        for (int d = 0; d < n_dist; ++d)
            for (int f = 0; f < 6; ++f)
                if (need[d][f] && n < MAXSTAGE) { g.stage[n++] = StageItem{d, f, g.ds[d].size, off}; off += g.ds[d].size; }
        g.n_stage = n; g.stage_doubles = off;
        if (off * sizeof(double) > 72 * 1024 || !g_eng.prior_stage) { g.n_stage = 0; g.stage_doubles = 0; }     // too big (or option prior_stage 0): stay in global memory
        // one contiguous image of the staged tables, in LDS order: staging is a flat copy (every load of a
        // workgroup in flight at once) instead of a walk over the table list
        g.stage_image = nullptr;
        if (g.n_stage > 0) {
            std::vector<double> image((size_t)g.stage_doubles);
            for (int q = 0; q < g.n_stage; ++q) {
                const StageItem &it = g.stage[q];
                const nfa_dist_desc &s = dists[it.dist];
                const double *src = it.field == ST_XAX ? s.xax : it.field == ST_PDF ? s.pdf : it.field == ST_PPF ? s.ppf
                                  : moments[it.dist][it.field - ST_M0].data();
                std::copy(src, src + it.n, image.begin() + it.off);
            }
            int rc = upload(image.data(), (int64_t)image.size(), &g.stage_image); if (rc) return rc;
        }
    }
    // Priors that write disjoint parameter slots can be interpreted side by side (one wave each): the
    // reference applies them one after the other (core.pyx:459-476), which only matters if two of them share a slot.
    {
        unsigned seen = 0;
        g.parallel = 1;
        for (int k = 0; k < n_prior; ++k) {
            const nfa_prior_desc &q = priors[k];
            unsigned mine = 1u << (q.p_ix & 31);
            const bool two = q.kind == NFA_PRIOR_DUPLICATE || q.kind == NFA_PRIOR_RESOLVED_CENSEP || q.kind == NFA_PRIOR_RESOLVED_PLACEMENT;
            if (two && q.p_ix2 >= 0) mine |= 1u << (q.p_ix2 & 31);
            if ((seen & mine) || q.p_ix >= 32 || (two && q.p_ix2 >= 32)) g.parallel = 0;
            seen |= mine;
        }
    }
    // The set-up stage may run ONE resolved prior's part B (its velocities: prior_apply_lane) beside the partition sums and
    // the derived records, if those read nothing that part B writes: the program is parallel, the prior's main slot is 0
    // (the velocity, which enters a record only as d[2], written last) and its sub-prior's is not.  Parallel leaves no
    // second prior on slot 0, so every other slot is complete before part B starts.  Anything else: the phases in sequence.
    {
        int n_b = 0, k_b = -1;
        bool ok = g.parallel != 0;
        for (int k = 0; k < n_prior; ++k) {
            const nfa_prior_desc &q = priors[k];
            if (q.kind != NFA_PRIOR_RESOLVED_CENSEP && q.kind != NFA_PRIOR_RESOLVED_PLACEMENT) continue;
            n_b += 1; k_b = k;
            if (q.p_ix != 0 || q.p_ix2 <= 0) ok = false;
        }
        g.overlap_k = ok && n_b == 1 ? k_b + 1 : 0;
    }
    HIP_TRY(hipMalloc(&p->d_prog, sizeof(PriorProg)));
    HIP_TRY(hipMemcpy(p->d_prog, &p->prog, sizeof(PriorProg), hipMemcpyHostToDevice));
    if (g.n_stage == 0) { p->d_prog_global = p->d_prog; return NFA_OK; }
    PriorProg flat = g;
    flat.n_stage = 0; flat.stage_doubles = 0; flat.stage_image = nullptr;
    HIP_TRY(hipMalloc(&p->d_prog_global, sizeof(PriorProg)));
    HIP_TRY(hipMemcpy(p->d_prog_global, &flat, sizeof(PriorProg), hipMemcpyHostToDevice));
    return NFA_OK;
}

int nfa_priors_create(nfa_priors **out, const nfa_prior_desc *priors, int n_prior,
                      const nfa_dist_desc *dists, int n_dist, int n_param) {
    if (!out || !priors || n_prior < 1 || n_prior > MAXPRIOR || n_dist < 0 || n_dist > MAXDIST)
        return fail(NFA_ERR_ARG, "prior program out of range (<=16 priors, <=16 distributions)");
    int rc = engine_init(); if (rc) return rc;
    nfa_priors *p = new nfa_priors();
    rc = priors_fill(p, priors, n_prior, dists, n_dist, n_param);
    if (rc) { nfa_priors_destroy(p); return rc; }            // frees whatever was uploaded
    *out = p;
    return NFA_OK;
}

int nfa_priors_destroy(nfa_priors *p) {
    if (!p) return NFA_OK;
    if (p->d_prog_global != p->d_prog) (void)hipFree(p->d_prog_global);
    (void)hipFree(p->d_prog);
    for (double *d : p->d_arrays) (void)hipFree(d);
    delete p;
    return NFA_OK;
}

static int launch_priors(const nfa_priors *p, double *d_U, int64_t B, int ncomp, hipStream_t st) {
    const int ndim = p->prog.n_param * ncomp;
    const size_t lds = sizeof(double) * 64 * (size_t)ndim;          // theta transposed, one lane per item
    if (lds > 64 * 1024) return fail(NFA_ERR_ARG, "too many parameters for the prior kernel");
    hipLaunchKernelGGL(prior_items_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), lds, st,
                       (const PriorProg *)p->d_prog, d_U, (long)B, ncomp);
    HIP_TRY(hipGetLastError());
    return NFA_OK;
}

int nfa_priors_transform_batch(const nfa_priors *p, double *U, int64_t B, int ncomp, int ndim) {
    if (!p || !U) return fail(NFA_ERR_ARG, "null argument");
    if (ncomp < 1 || p->prog.n_param * ncomp != ndim) {                 // core.pyx:479-483
        char msg[96];
        snprintf(msg, sizeof msg, "Invalid shape for ncomp=%d: %d", ncomp, ndim);
        return fail(NFA_ERR_ARG, msg);
    }
    if (B <= 0) return NFA_OK;
    double *d_U = nullptr;
    HIP_TRY(hipMalloc(&d_U, sizeof(double) * B * ndim));
    HIP_TRY(hipMemcpy(d_U, U, sizeof(double) * B * ndim, hipMemcpyHostToDevice));
    int rc = launch_priors(p, d_U, B, ncomp, 0);
    if (rc) { (void)hipFree(d_U); return rc; }
    HIP_TRY(hipMemcpy(U, d_U, sizeof(double) * B * ndim, hipMemcpyDeviceToHost));
    (void)hipFree(d_U);
    return NFA_OK;
}

// ---- runner ----------------------------------------------------------------
int nfa_runner_create(nfa_runner **out, nfa_specset *ss, nfa_priors *priors, int ncomp,
                      int cold, int lte) {
    if (!out || !ss) return fail(NFA_ERR_ARG, "null argument");
    if (ncomp < 1 || ncomp > MAXCOMP) return fail(NFA_ERR_ARG, "ncomp must be in 1..10");   // ammonia.pyx:401
    if (priors && priors->prog.n_param != ss->dev.npar)
        return fail(NFA_ERR_ARG, "prior program must cover the model's parameters (6 NH3, 4 N2H+, hyperfine and LTE, 3 Gaussian, 3 + the species of an LTE mix, one more with a filling factor, 5 excitation grid)");
    int rc = engine_init(); if (rc) return rc;
    nfa_runner *r = new nfa_runner();
    r->ss = ss; r->pr = priors; r->ncomp = ncomp; r->cold = cold ? 1 : 0; r->lte = lte ? 1 : 0;
    r->ndim = ss->dev.npar * ncomp;
    r->lanes_auto = g_eng.streams == 0;
    r->n_lanes = r->lanes_auto ? 4 : std::max(1, std::min(g_eng.streams, NFA_MAX_LANES));     // automatic: two more on demand (run_batch)
    static_assert(sizeof(PriorProg) == 3624 && sizeof(LineRec) == 32, "LDS layouts of nfa_launch_plan.h (and of its test)");
    r->shape = LpShape{ss->dev.n_spec, {}, ss->nhf_max, ncomp, r->ndim, ss->dev.model, priors ? priors->prog.n_stage : 0,
                       priors ? priors->prog.stage_doubles : 0, g_eng.wpb, g_eng.wpb_table, g_eng.lnl_cap, g_eng.lnl_split,
                       (int)sizeof(PriorProg), (int)sizeof(LineRec)};
    std::copy(ss->dev.size, ss->dev.size + MAXSPEC, r->shape.size);
    for (int k = 0; k < r->n_lanes; ++k) HIP_TRY(hipStreamCreateWithFlags(&r->lanes[k], hipStreamNonBlocking));
    r->stream = r->lanes[0];
    { std::lock_guard<std::mutex> lk(g_runners_m); g_runners.push_back(r); }
    *out = r;
    return NFA_OK;
}

int nfa_runner_destroy(nfa_runner *r) {
    if (!r) return NFA_OK;
    // out of the list first: from here on no global call walks this runner
    { std::lock_guard<std::mutex> lk(g_runners_m); g_runners.erase(std::remove(g_runners.begin(), g_runners.end(), r), g_runners.end()); }
    // batches still held for coalescing are dropped, not launched: their buffers are the caller's, who may have freed
    // them already (whoever wants the results synchronises, and that launches what is held)
    { RUNNER_LOCK(r); r->pending.n = 0; }
    for (int k = 0; k < r->n_lanes; ++k) (void)hipStreamSynchronize(r->lanes[k]);
    (void)hipFree(r->d_U); (void)hipFree(r->d_lnL); (void)hipFree(r->d_pix); (void)hipFree(r->d_spec);
    for (int k = 0; k < r->n_lanes; ++k) { (void)hipFree(r->d_D[k]); (void)hipFree(r->d_part[k]); (void)hipFree(r->d_queue[k]); (void)hipFree(r->d_band[k]); }
    if (r->g1) (void)hipGraphExecDestroy(r->g1);
    if (r->h_pin) (void)hipHostFree(r->h_pin);
    if (r->h_point) (void)hipHostFree(r->h_point);
    {
        MomScratch &m = r->mom;
        (void)hipFree(m.d_ref); (void)hipFree(m.d_acc); (void)hipFree(m.d_sref); (void)hipFree(m.d_sacc); (void)hipFree(m.d_s0);
        (void)hipFree(m.d_stat); (void)hipFree(m.d_w); (void)hipFree(m.d_pieces);
        for (int k = 0; k < 2; ++k) { if (m.h_stage[k]) (void)hipHostFree(m.h_stage[k]); if (m.ev[k]) (void)hipEventDestroy(m.ev[k]); }
    }
    (void)hipFree(r->lsq.d_buf); (void)hipFree(r->lsq.d_pix);
    if (r->d_point_done) (void)hipFree(r->d_point_done);
    for (hipEvent_t x : r->ev) (void)hipEventDestroy(x);
    for (int k = 0; k < r->n_lanes; ++k) (void)hipStreamDestroy(r->lanes[k]);
    delete r;
    return NFA_OK;
}

int nfa_runner_ndim(const nfa_runner *r) { return r ? r->ndim : 0; }

int nfa_runner_set_exp_mode(nfa_runner *r, int mode) {
    if (!r) return fail(NFA_ERR_ARG, "null runner");
    RUNNER_LOCK(r);
    if (mode != -1 && mode != 0 && mode != 2) return fail(NFA_ERR_ARG, "exp mode must be -1 (process default), 0 (table) or 2 (fast)");
    { int rc = flush_pending(r); if (rc) return rc; }
    r->exp_mode = mode;
    return NFA_OK;
}
int nfa_runner_get_exp_mode(const nfa_runner *r) { return !r ? -1 : runner_mode(r); }

static int runner_reserve(nfa_runner *r, int64_t B, bool spec) {
    if (B > r->cap_B) {
        if (r->g1) { (void)hipGraphExecDestroy(r->g1); r->g1 = nullptr; }
        (void)hipFree(r->d_U); (void)hipFree(r->d_lnL); (void)hipFree(r->d_pix);
        r->d_U = nullptr; r->d_lnL = nullptr; r->d_pix = nullptr; r->cap_B = 0;
        const int64_t cap = std::max<int64_t>(B, 64);
        HIP_TRY(hipMalloc(&r->d_U, sizeof(double) * cap * r->ndim));
        HIP_TRY(hipMalloc(&r->d_lnL, sizeof(double) * cap));
        HIP_TRY(hipMalloc(&r->d_pix, sizeof(int) * cap));
        r->cap_B = cap;
    }
    if (spec && B > r->cap_spec) {
        (void)hipFree(r->d_spec); r->d_spec = nullptr; r->cap_spec = 0;
        HIP_TRY(hipMalloc(&r->d_spec, sizeof(double) * B * r->ss->dev.chan_tot));
        r->cap_spec = B;
    }
    return NFA_OK;
}

}  // extern "C" (templates need C++ linkage)

static SpecDev runner_specdev(const nfa_runner *r) {
    SpecDev S = r->ss->dev;
    S.ncomp = r->ncomp; S.cold = r->cold; S.lte = r->lte;
    S.t0_xmin = g_eng.t0_xmin; S.t0_xmax = g_eng.t0_xmax; S.t0_inv_dx = g_eng.t0_inv_dx;
    return S;
}
// the plan of the fused kernels for a runner's points (S: runner_specdev(r)): what its set is right now, said once
static FusedPlan runner_fused_plan(const nfa_runner *r, int mode, const SpecDev &S) {
    return plan_fused(r->shape, plan_knobs(), mode, S.bl_order >= 0, S.chan_w != nullptr, S.band != nullptr, r->ss->filled, r->ss->layered,
                      S.cal2 != nullptr, S.corr_q1 != nullptr, S.resp != nullptr, S.tmpl != nullptr, S.cont != nullptr, S.rob != nullptr,
                      S.grid != nullptr);
}

// A kernel that wants more than 64 KB of dynamic LDS has to be told so -- once per kernel and size, not on every
// launch (the attribute call is a trip into the runtime: 1-2 us of the ~10 the host spends on enqueueing a step).
static int ensure_dynamic_lds(const void *kernel, size_t lds) {
    if (lds <= 64 * 1024) return NFA_OK;
    struct Grant { const void *kernel; int device; size_t lds; };        // the attribute belongs to a kernel on a device
    static std::mutex m;
    static std::vector<Grant> granted;
    std::lock_guard<std::mutex> lk(m);
    for (auto &g : granted)
        if (g.kernel == kernel && g.device == g_eng.device) {
            if (g.lds >= lds) return NFA_OK;
            HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            g.lds = lds;
            return NFA_OK;
        }
    HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    granted.push_back(Grant{kernel, g_eng.device, lds});
    return NFA_OK;
}

// derived records and chi^2 parts of stream lane `slot` for B items
static int reserve_lane(nfa_runner *r, int slot, int64_t B) {
    if (B <= r->cap_D[slot]) return NFA_OK;  // grown outside any timed loop
    const int n_spec = r->ss->dev.n_spec;
    if (slot == 0 && r->g1) { (void)hipGraphExecDestroy(r->g1); r->g1 = nullptr; }
    HIP_TRY(hipStreamSynchronize(r->lanes[slot]));
    (void)hipFree(r->d_D[slot]); (void)hipFree(r->d_part[slot]); (void)hipFree(r->d_band[slot]);
    r->d_D[slot] = nullptr; r->d_part[slot] = nullptr; r->d_band[slot] = nullptr; r->cap_D[slot] = 0;
    const int64_t cap = std::max<int64_t>(B, 4096);
    // (the record as the plan header counts it, which tests/test_grid_cpu.py holds to the kernels' layout: an excitation-grid
    // set's is the larger one)
    HIP_TRY(hipMalloc(&r->d_D[slot], sizeof(double) * cap * lnl_drec_doubles(r->ncomp, n_spec, r->ss->dev.grid != nullptr)));
    if (r->ss->dev.band) HIP_TRY(hipMalloc(&r->d_band[slot], sizeof(double) * cap * r->ncomp * n_spec * NFA_BAND_MAXT));
    HIP_TRY(hipMalloc(&r->d_part[slot], sizeof(double) * cap * n_spec));
    if (!r->d_queue[slot]) {
        HIP_TRY(hipMalloc(&r->d_queue[slot], sizeof(unsigned) * NFA_QUEUE_WORDS));
        // on the lane itself: the lanes are non-blocking streams, so a null-stream memset is not ordered before the lane's
        // first queue launch, which could then start from whatever the fresh allocation held
        HIP_TRY(hipMemsetAsync(r->d_queue[slot], 0, sizeof(unsigned) * NFA_QUEUE_WORDS, r->lanes[slot]));
    }
    r->cap_D[slot] = cap;
    return NFA_OK;
}

// Set-up stage of a batch (the arrays travel in r->cur_group) on stream lane `slot`: [unit cube -> theta in place] ->
// partition sums -> derived records r->d_D[slot], one launch (setup_kernel, nfa_setup.h)
static int launch_setup(nfa_runner *r, int64_t B, bool has_prior, int slot, int mode) {
    const SpecDev S = runner_specdev(r);
    hipStream_t st = r->lanes[slot];
    int rc = reserve_lane(r, slot, B); if (rc) return rc;
    if (has_prior && !r->pr) return fail(NFA_ERR_STATE, "runner has no priors (predict-only)");
    const SetupPlan P = plan_setup(r->shape, plan_knobs(), plan_launch(r, B, mode, false, has_prior, slot));
    if (P.error) return fail(NFA_ERR_ARG, P.error);
    const PriorProg *prog = !has_prior ? nullptr : P.staged ? r->pr->d_prog : r->pr->d_prog_global;
    const auto kern = P.inst == SETUP_TABLE_2 ? setup_kernel<0, false, 2> : P.inst == SETUP_TABLE ? setup_kernel<0, false>
                    : P.inst == SETUP_FAST ? setup_kernel<1, true> : setup_kernel<1, false>;
    { int rc2 = ensure_dynamic_lds((const void *)kern, P.lds); if (rc2) return rc2; }
    if (r->ev_cur)      // profiling: the events ride on the dispatch itself -- its own start and stop, as a tracer sees them
        hipExtLaunchKernelGGL(kern, dim3(P.blocks), dim3(P.threads), P.lds, st, r->ev_cur[0], r->ev_cur[1], 0, prog, S, r->cur_group, r->d_D[slot], (long)B,
                              has_prior ? 1 : 0, (const double *)g_eng.d_tabs, g_eng.ablate, P.ti, g_eng.setup_overlap);
    else
        hipLaunchKernelGGL(kern, dim3(P.blocks), dim3(P.threads), P.lds, st, prog, S, r->cur_group, r->d_D[slot], (long)B,
                           has_prior ? 1 : 0, (const double *)g_eng.d_tabs, g_eng.ablate, P.ti, g_eng.setup_overlap);
    HIP_TRY(hipGetLastError());
    return NFA_OK;
}

// LTE bands: tau_main of every (item, component, spectrum, transition) of the B items whose records the set-up stage has
// just written on this lane (lte_band_kernel, nfa_setup.h), one small launch between the two stages
// An LTE mix: lte_mix_kernel in its place, which also reads the column densities of the further species from the theta
// of the batches in r->cur_group (written back by the set-up launch before it on this lane)
static int launch_band(nfa_runner *r, int slot, int64_t B) {
    const int n_spec = r->ss->dev.n_spec;
    const int64_t lanes = B * r->ncomp * n_spec * NFA_BAND_MAXT;
    if (r->ss->dev.mix) {
        hipLaunchKernelGGL(lte_mix_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, r->lanes[slot],
                           (const BandRec *)r->ss->d_band, (const MixRec *)r->ss->d_mix, (const LteRec *)r->ss->d_lte,
                           (const double *)r->d_D[slot], r->d_band[slot], r->cur_group, (long)B, r->ncomp, n_spec, r->ss->dev.npar);
        HIP_TRY(hipGetLastError());
        // a filled set: the components' filling factors from the same theta into the records (lte_fill_kernel)
        if (r->ss->filled) {
            const int64_t recs = B * r->ncomp * n_spec;
            hipLaunchKernelGGL(lte_fill_kernel, dim3((unsigned)((recs + 255) / 256)), dim3(256), 0, r->lanes[slot],
                               r->d_D[slot], r->cur_group, (long)B, r->ncomp, n_spec, r->ss->dev.npar);
            HIP_TRY(hipGetLastError());
        }
        return NFA_OK;
    }
    hipLaunchKernelGGL(lte_band_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, r->lanes[slot],
                       (const BandRec *)r->ss->d_band, (const double *)r->d_D[slot], r->d_band[slot], (long)B, r->ncomp, n_spec);
    HIP_TRY(hipGetLastError());
    return NFA_OK;
}

// The excitation-grid model: the records of every (item, component, spectrum) of the B items whose theta the set-up stage
// has just left in the batches of r->cur_group on this lane (grid_derive_kernel, nfa_setup.h), one launch between the two
// stages; the fast mode's records where the set-up stage would have written those
static int launch_grid(nfa_runner *r, int slot, int64_t B, int mode) {
    const SpecDev S = runner_specdev(r);
    const int64_t recs = B * r->ncomp * S.n_spec;
    const auto kern = mode == 2 ? grid_derive_kernel<true> : grid_derive_kernel<false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)((recs + 255) / 256)), dim3(256), 0, r->lanes[slot], S, r->d_D[slot], r->cur_group,
                       (long)B, (const double *)g_eng.d_tabs);
    HIP_TRY(hipGetLastError());
    return NFA_OK;
}

// The kernel of a plan.  Naming an instance compiles it, so entry I of the table names its instance only where
// lnl_instance_exists (nfa_launch_plan.h) says there is one: that predicate is what keeps the instance count where it is
// (208: the plain form of the table mode with spectra out is not among them, no plan of plan_lnl names it).
typedef void (*LnlKernel)(SpecDev, BatchGroup, const double *, double *, double *, long, LnlGeom, const double *);
template <int I>     // I: lnl_inst_index
static LnlKernel lnl_kernel_inst(LnlForm form) {
    constexpr LnlInst N = lnl_inst_at(I);
    if constexpr (N.kind != 0) {
        // (a kind has one form, lnl_kind_form: the predicate is asked about that one, and so decides on the bits and NCOMP alone)
        if constexpr (lnl_instance_exists(lnl_kind_form(N.kind), N.mode, N.write_spec, N.wide, N.ncomp, N.kind))
            if (form == lnl_kind_form(N.kind)) return lnl_kernel_kind<N.mode, N.write_spec, N.wide, N.ncomp, N.kind>;
    } else {
        if constexpr (lnl_instance_exists(LNL_QUEUE, N.mode, N.write_spec, N.wide, N.ncomp, 0))
            if (form == LNL_QUEUE) return lnl_kernel_queue<N.write_spec, N.ncomp>;
        if constexpr (lnl_instance_exists(LNL_W8, N.mode, N.write_spec, N.wide, N.ncomp, 0))
            if (form == LNL_W8) return lnl_kernel_w8<N.mode, N.write_spec, N.wide, N.ncomp>;
        if constexpr (lnl_instance_exists(LNL_PLAIN, N.mode, N.write_spec, N.wide, N.ncomp, 0))
            if (form == LNL_PLAIN) return lnl_kernel<N.mode, N.write_spec, N.wide, N.ncomp>;
    }
    return nullptr;                                           // (null: no instance of this form here)
}
template <size_t... I>
static LnlKernel lnl_kernel_at(int i, LnlForm form, std::index_sequence<I...>) {
    static constexpr LnlKernel (*inst[])(LnlForm) = {lnl_kernel_inst<(int)I>...};
    return inst[i](form);
}
static LnlKernel lnl_kernel_of(int mode, bool write_spec, int ncomp, const LnlPlan &P) {
    return lnl_kernel_at(lnl_inst_index({mode, write_spec, P.wide, lnl_plan_ncomp(P, ncomp), lnl_plan_kind(P)}), P.form,
                         std::make_index_sequence<LNL_INSTANCES>());
}
// The kernel of a set of a side (LnlSide): lnl_kernel_side over (side, lnl_side_index), beside the table (its launches are
// on no entry of it, so count_lnl_launch counts none of them).  Null unless the plan has the side's form.
template <int I>     // I: 32 (side - 1) + lnl_side_index
static LnlKernel lnl_kernel_side_inst() {
    constexpr LnlSideInst N = lnl_side_at(I % LNL_SIDE_INSTANCES);
    return lnl_kernel_side<N.mode, N.write_spec, N.wide, N.filled, N.layered, I / LNL_SIDE_INSTANCES + 1>;
}
template <size_t... I>
static LnlKernel lnl_kernel_side_at(int i, std::index_sequence<I...>) {
    static constexpr LnlKernel (*inst[])() = {lnl_kernel_side_inst<(int)I>...};
    return inst[i]();
}
static LnlKernel lnl_kernel_side_of(LnlSide side, int mode, bool write_spec, const LnlPlan &P) {
    if (P.form != lnl_side_form(side)) return nullptr;
    return lnl_kernel_side_at(LNL_SIDE_INSTANCES * (side - 1) + lnl_side_index(mode, write_spec, P.wide, P.filled, P.layered),
                              std::make_index_sequence<LNL_SIDES * LNL_SIDE_INSTANCES>());
}
#ifdef NFA_TEST_HOOKS
#include <atomic>
// Likelihood launches by (lnl_inst_index, LnlForm) since the last reset (nfa_test_lnl_launches): host side, counted where
// the launch is made; atomic, a broker's runners launch from several threads.  A launch is counted on the entry of the
// table that holds the kernel it was given -- found by the kernel's address, not by the index lnl_kernel_of formed -- so a
// slip in that index shows as a launch on another instance (every instance is a function of its own: one entry per address).
static std::atomic<int64_t> g_lnl_launches[LNL_INSTANCES][LNL_BASELINE + 1];
static void count_lnl_launch(LnlKernel kern) {
    static thread_local LnlKernel last = nullptr;             // (a thread's launches are mostly of one kernel: the table is
    static thread_local std::atomic<int64_t> *slot = nullptr; //  searched when the kernel changes)
    if (kern != last) {
        last = kern, slot = nullptr;
        for (int i = 0; i < LNL_INSTANCES && !slot; ++i)
            for (int f = 0; f <= LNL_BASELINE && !slot; ++f)
                if (lnl_kernel_at(i, (LnlForm)f, std::make_index_sequence<LNL_INSTANCES>()) == kern) slot = &g_lnl_launches[i][f];
    }
    if (slot) slot->fetch_add(1, std::memory_order_relaxed);
}
#endif

// Likelihood stage of the batch in r->cur_group on stream lane `slot`: chi^2 parts of the units (and spectra out), then
// -- want_lnl, and nobody else sums the parts -- lnL of the items (lnl_sum_kernel)
static int launch_lnl(nfa_runner *r, int slot, bool want_lnl, double *d_spec, int64_t B, int mode) {
    SpecDev S = runner_specdev(r);
    S.band_tau = r->d_band[slot];                             // (null unless the set is banded)
    LnlPlan P = plan_lnl(r->shape, plan_knobs(), plan_launch(r, B, mode, d_spec != nullptr, false, slot), S.tmpl != nullptr, S.grid != nullptr);
    if (P.error) return fail(NFA_ERR_ARG, P.error);
    if (P.form == LNL_QUEUE) P.G.queue = r->d_queue[slot];
#ifdef NFA_TEST_HOOKS
    P.G.trace = g_eng.d_trace;
#endif
    const LnlSide side = lnl_side_of(S.corr_q1 != nullptr, S.resp != nullptr, S.tmpl != nullptr, S.cont != nullptr, S.rob != nullptr, S.grid != nullptr);
    const LnlKernel kern = side != LNL_SIDE_NONE ? lnl_kernel_side_of(side, mode, d_spec != nullptr, P) : lnl_kernel_of(mode, d_spec != nullptr, r->ncomp, P);
    if (!kern) return fail(NFA_ERR_STATE, "no likelihood kernel of the planned form");
#ifdef NFA_TEST_HOOKS
    count_lnl_launch(kern);
#endif
    int rc = ensure_dynamic_lds((const void *)kern, P.lds); if (rc) return rc;
    hipStream_t st = r->lanes[slot];
    double *part = want_lnl ? r->d_part[slot] : nullptr;
    if (r->ev_cur) {
        hipExtLaunchKernelGGL(kern, dim3((unsigned)P.blocks), dim3(64 * P.waves), P.lds, st, r->ev_cur[2], r->ev_cur[3], 0, S, r->cur_group,
                              (const double *)r->d_D[slot], part, d_spec, (long)B, P.G, (const double *)g_eng.d_tabs);
        r->ev_cur = nullptr;
    } else
        hipLaunchKernelGGL(kern, dim3((unsigned)P.blocks), dim3(64 * P.waves), P.lds, st, S, r->cur_group,
                           (const double *)r->d_D[slot], part, d_spec, (long)B, P.G, (const double *)g_eng.d_tabs);
    HIP_TRY(hipGetLastError());
    if (want_lnl && !r->part_only) {
        if (S.nmarg)
            hipLaunchKernelGGL(lnl_sum_nmarg_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st,
                               (const double *)r->d_part[slot], S.noise, S.nmarg, r->cur_group, (long)B, S.n_spec);
        else
            hipLaunchKernelGGL(lnl_sum_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st,
                               (const double *)r->d_part[slot], S.noise, r->cur_group, (long)B, S.n_spec);
        HIP_TRY(hipGetLastError());
    }
    return NFA_OK;
}

// The batches of `grp` (one, or several of the same shape coalesced) as one set of launches on the next stream lane
// (force_lane >= 0: on that one): set-up kernel, then likelihood kernel.
static int run_group(nfa_runner *r, const BatchGroup &grp, double *d_spec, bool has_prior, int force_lane) {
    const int64_t B = (int64_t)grp.each * grp.n;
    int rc0 = engine_init(); if (rc0) return rc0;            // binds the calling thread to the device
    if (!g_eng.have_t0) return fail(NFA_ERR_STATE, "nfa_set_iemtex_table has not been called");
    int n_use = r->n_lanes;
    if (r->lanes_auto) {
        n_use = lp_lanes(r->shape, plan_knobs(), B);
        // The fifth and sixth stream exist only once a batch of that size has come by: idle streams are not free --
        // with six streams mapped the small launches of a sampler round trip 25 % slower even on the three they use
        // (config 5, one component: 1.25 -> 1.56 s).
        while (r->n_lanes < n_use && force_lane < 0) {
            HIP_TRY(hipStreamCreateWithFlags(&r->lanes[r->n_lanes], hipStreamNonBlocking));
            r->n_lanes += 1;
        }
        n_use = std::min(n_use, r->n_lanes);
    }
    const int slot = force_lane >= 0 ? force_lane : (int)(r->n_calls % (uint64_t)n_use);
    if (r->profiling) {
        if (r->ev_used + 4 > r->ev.size()) {
            for (int k = 0; k < 4; ++k) { hipEvent_t x; HIP_TRY(hipEventCreate(&x)); r->ev.push_back(x); }
        }
        r->ev_cur = &r->ev[r->ev_used];                       // (launch_lnl takes the last pair and clears it)
        r->ev_used += 4;
    }
    const int mode = runner_mode(r);                          // read once per batch
    r->cur_group = grp;
    int rc = launch_setup(r, B, has_prior, slot, mode);
    if (rc) return rc;
    if (r->ss->dev.band) { rc = launch_band(r, slot, B); if (rc) return rc; }
    if (r->ss->dev.grid) { rc = launch_grid(r, slot, B, mode); if (rc) return rc; }
    rc = launch_lnl(r, slot, grp.lnL[0] != nullptr, d_spec, B, mode);
    if (rc) return rc;
    r->n_calls++;
    r->lane_busy |= 1u << slot;
    return NFA_OK;
}
static int run_batch(nfa_runner *r, const int *d_pix, double *d_U, double *d_lnL, double *d_spec,
                     int64_t B, bool has_prior, int force_lane) {
    BatchGroup g = {};
    g.pix[0] = d_pix; g.U[0] = d_U; g.lnL[0] = d_lnL; g.each = (long)B; g.n = 1;
    return run_group(r, g, d_spec, has_prior, force_lane);
}

// Coalescing of device-pointer batches.  nfa_runner_loglike_batch_dev returns before anything runs anyway; batches
// of one shape that arrive back to back are held (at most `coalesce` of them) and launched together: a launch of
// four times 4096 rows keeps the vector ALUs busy 94 % of the time, four launches of 4096 rows overlapping on
// their lanes 79 %.  Everything that looks at results, changes how launches are made or uses the lanes
// itself launches what is held first (flush_pending).
static int flush_pending(nfa_runner *r) {
    if (r->pending.n == 0) return NFA_OK;
    const BatchGroup g = r->pending;
    r->pending.n = 0;
    return run_group(r, g, g.spec[0], r->pending_prior, -1);
}
static int flush_all_runners() {
    std::lock_guard<std::mutex> lk(g_runners_m);
    for (nfa_runner *r : g_runners) {
        RUNNER_LOCK(r);
        int rc = flush_pending(r); if (rc) return rc;
    }
    return NFA_OK;
}

static int sync_all_lanes(nfa_runner *r) {
    { int rc = flush_pending(r); if (rc) return rc; }
    // only lanes that had work enqueued since their last synchronisation (a synchronise call on an
    // idle stream still costs a couple of microseconds, and single-point callers pay it per point)
    for (int k = 0; k < r->n_lanes; ++k)
        if (r->lane_busy & (1u << k)) HIP_TRY(hipStreamSynchronize(r->lanes[k]));
    r->lane_busy = 0;
    return NFA_OK;
}

static int check_pix(const nfa_runner *r, const int32_t *pix, int64_t B) {
    if (!pix) return NFA_OK;
    for (int64_t b = 0; b < B; ++b)
        if (pix[b] < 0 || pix[b] >= r->ss->n_pix) return fail(NFA_ERR_ARG, "pixel index out of range");
    return NFA_OK;
}

extern "C" {

// a device-pointer batch: launched with its neighbours of the same kind and shape, or on its own
static int enqueue_dev(nfa_runner *r, const int32_t *d_pix, double *d_U, double *d_lnL, double *d_spec, int64_t B, bool has_prior) {
    BatchGroup &p = r->pending;
    const LpKnobs knobs = plan_knobs();                // read per call: knobs, not part of a runner's identity
    const bool fits = lp_may_hold(r->shape, knobs, B, r->profiling);
    if (p.n > 0 && (!fits || p.each != (long)B || r->pending_prior != has_prior || (p.pix[0] == nullptr) != (d_pix == nullptr) ||
                    (p.lnL[0] == nullptr) != (d_lnL == nullptr) || (p.spec[0] == nullptr) != (d_spec == nullptr) ||
                    lp_group_full(r->shape, knobs, p.n, B))) {
        int rc = flush_pending(r); if (rc) return rc;
    }
    if (!fits) return run_batch(r, d_pix, d_U, d_lnL, d_spec, B, has_prior, -1);
    p.pix[p.n] = d_pix; p.U[p.n] = d_U; p.lnL[p.n] = d_lnL; p.spec[p.n] = d_spec; p.each = (long)B; p.n += 1;
    r->pending_prior = has_prior;
    if (lp_group_full(r->shape, knobs, p.n, B)) return flush_pending(r);
    return NFA_OK;
}

int nfa_runner_loglike_batch_dev(nfa_runner *r, const int32_t *d_pix, double *d_U, double *d_lnL,
                                 int64_t B) {
    if (!r || !d_U || !d_lnL) return fail(NFA_ERR_ARG, "null argument");
    if (!r->pr) return fail(NFA_ERR_STATE, "runner has no priors (predict-only)");
    if (B <= 0) return NFA_OK;
    RUNNER_LOCK(r);
    return enqueue_dev(r, d_pix, d_U, d_lnL, nullptr, B, true);
}

int nfa_runner_set_profiling(nfa_runner *r, int on) {
    if (!r) return fail(NFA_ERR_ARG, "null runner");
    RUNNER_LOCK(r);
    int rc = sync_all_lanes(r); if (rc) return rc;
    r->profiling = on != 0;
    r->ev_used = 0;
    return NFA_OK;
}

// length of the union of intervals [a_k, b_k] (milliseconds)
static double union_length(std::vector<std::pair<double, double>> iv) {
    std::sort(iv.begin(), iv.end());
    double tot = 0, cur_a = 0, cur_b = -1;
    for (auto &p : iv) {
        if (cur_b < cur_a || p.first > cur_b) {
            if (cur_b >= cur_a) tot += cur_b - cur_a;
            cur_a = p.first; cur_b = p.second;
        } else if (p.second > cur_b) cur_b = p.second;
    }
    if (cur_b >= cur_a) tot += cur_b - cur_a;
    return tot;
}

int nfa_runner_get_profile(nfa_runner *r, double *out, int64_t *calls) {
    if (!r || !out || !calls) return fail(NFA_ERR_ARG, "null argument");
    RUNNER_LOCK(r);
    int rc = sync_all_lanes(r); if (rc) return rc;
    double a = 0, b = 0;
    std::vector<std::pair<double, double>> iv_setup, iv_lnl;
    const size_t n = std::min(r->ev_used, r->ev.size()) / 4;
    // (the first profile_skip calls are left out: launches behind an idle gap run at the clocks the chip had idled at, a
    // few milliseconds of load later the same launch is 10 % shorter -- a timed block is long, a probe of 15 launches is not)
    const size_t k0 = std::min<size_t>(n, (size_t)std::max(0, g_eng.profile_skip));
    for (size_t k = k0; k < n; ++k) {
        float t0 = 0, t1 = 0, t2 = 0, t3 = 0;  // times since the first recorded event
        HIP_TRY(hipEventElapsedTime(&t0, r->ev[0], r->ev[4 * k]));
        HIP_TRY(hipEventElapsedTime(&t1, r->ev[0], r->ev[4 * k + 1]));
        HIP_TRY(hipEventElapsedTime(&t2, r->ev[0], r->ev[4 * k + 2]));
        HIP_TRY(hipEventElapsedTime(&t3, r->ev[0], r->ev[4 * k + 3]));
        a += t1 - t0; b += t3 - t2;
        iv_setup.emplace_back(t0, t1);
        iv_lnl.emplace_back(t2, t3);
    }
    out[0] = a;                          // sum of set-up kernel durations
    out[1] = b;                          // sum of lnl_kernel durations (lnl_sum_kernel not included)
    out[2] = union_length(iv_setup);     // time during which >= 1 set-up kernel was running
    out[3] = union_length(iv_lnl);       // time during which >= 1 likelihood kernel was running
    *calls = (int64_t)(n - k0);
    r->ev_used = 0;
    return NFA_OK;
}

int nfa_runner_synchronize(nfa_runner *r) {
    if (!r) return fail(NFA_ERR_ARG, "null runner");
    RUNNER_LOCK(r);
    return sync_all_lanes(r);
}

}  // extern "C"

// One point, or the few a broker gathered, through the point kernel (nfa_setup.h); returns 1 when the call
// was served, 0 when another path has to do it, a negative value on a device error.
#define POINT_HOST_DOUBLES (NFA_POINT_MAXB * (2 * NFA_POINT_MAXDIM + 2) + 8)
template <int MODE>    // the instance of a component count: 1..3 with the component loop unrolled, anything else the general form
static decltype(&point_kernel<MODE, 0>) point_kernel_of(int ncomp) {
    switch (ncomp) {
    case 1: return point_kernel<MODE, 1>;
    case 2: return point_kernel<MODE, 2>;
    case 3: return point_kernel<MODE, 3>;
    default: return point_kernel<MODE, 0>;
    }
}

static int few_points_kernel(nfa_runner *r, const int32_t *pix, double *U, double *lnL, int64_t B) {
    const int ndim = r->ndim;
    if (!g_eng.point || r->profiling || B > NFA_POINT_MAXB) return 0;
    const int mode = runner_mode(r);
    const SpecDev S = runner_specdev(r);
    const FusedPlan P = runner_fused_plan(r, mode, S);
    if (P.refusal || P.lds_point > LDS_PER_CU) return 0;
    if (reserve_lane(r, 0, B) != NFA_OK) return -1;
    if (!r->h_point) {
        bool ok = hipHostMalloc((void **)&r->h_point, sizeof(double) * POINT_HOST_DOUBLES, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess
                  && hipHostGetDevicePointer((void **)&r->d_point, r->h_point, 0) == hipSuccess
                  && hipMalloc((void **)&r->d_point_done, sizeof(unsigned)) == hipSuccess
                  && hipMemset(r->d_point_done, 0, sizeof(unsigned)) == hipSuccess
                  && hipDeviceSynchronize() == hipSuccess;        // (a null-stream memset is not ordered before the lanes' work)
        if (!ok) {
            (void)hipGetLastError();
            if (r->h_point) (void)hipHostFree(r->h_point);
            if (r->d_point_done) (void)hipFree(r->d_point_done);
            r->h_point = nullptr; r->d_point_done = nullptr;
            g_eng.point = 0;
            return 0;
        }
        memset(r->h_point, 0, sizeof(double) * POINT_HOST_DOUBLES);
    }
    PointIn in;
    memset(&in, 0, sizeof in);
    in.seq = ++r->pt_seq;
    in.n = (int)B;
    in.n_blocks = P.n_blocks;
    in.overlap = g_eng.setup_overlap;
    if (B == 1) {
        memcpy(in.u, U, sizeof(double) * ndim);
        in.pix = pix ? pix[0] : -1;
    } else {                                                     // the unit cubes travel through the mapped buffer
        double *in_u = r->h_point + B * (ndim + 1) + 1;
        memcpy(in_u, U, sizeof(double) * B * ndim);
        if (pix) memcpy(in_u + B * ndim, pix, sizeof(int32_t) * B);
        in.pix = pix ? 0 : -1;
    }
    volatile unsigned long long *flag = (volatile unsigned long long *)(r->h_point + B * (ndim + 1));
    *flag = 0;                                                   // the slot holds other data when B changes
    __atomic_thread_fence(__ATOMIC_SEQ_CST);
    const auto kern = mode == 0 ? point_kernel_of<0>(r->ncomp) : point_kernel_of<2>(r->ncomp);
    (void)ensure_dynamic_lds((const void *)kern, P.lds_point);
    hipLaunchKernelGGL(kern, dim3((unsigned)in.n), dim3(POINT_THREADS), P.lds_point, r->lanes[0],
                       (const PriorProg *)(P.staged ? r->pr->d_prog : r->pr->d_prog_global), S, in,
                       r->d_pix, r->d_U, r->d_D[0], r->d_part[0], r->d_point, r->d_point_done, P.G,
                       (const double *)g_eng.d_tabs);
    if (hipGetLastError() != hipSuccess) { fail(NFA_ERR_DEVICE, "point kernel launch failed"); return -1; }
    // the kernel's last store is the sequence number; the host reads it straight from the mapped buffer
    const auto t_start = std::chrono::steady_clock::now();
    for (uint64_t spins = 0;; ++spins) {
        if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == in.seq) break;
        if ((spins & 0xffff) == 0xffff
            && std::chrono::steady_clock::now() - t_start > std::chrono::seconds(2)) {
            // nothing came back: let the runtime say why (a fault surfaces here), or finish a very slow kernel
            if (hipStreamSynchronize(r->lanes[0]) != hipSuccess) { fail(NFA_ERR_DEVICE, "point kernel failed"); return -1; }
        }
    }
    memcpy(U, r->h_point, sizeof(double) * B * ndim);
    memcpy(lnL, r->h_point + B * ndim, sizeof(double) * B);
    return 1;
}

// One point through a captured graph; returns 1 when the call was served, 0 when the plain path
// has to do it (first calls, table mode whose launch sets a function attribute, profiling on).
static int single_point_graph(nfa_runner *r, double *U, double *lnL) {
    if (g_eng.graph < 0) {
        // Stream capture under the rocprofiler-sdk tool library (rocprofv3) has crashed the process
        // here: with a profiler attached single points take the plain path unless asked otherwise.
        bool profiled = false;
        for (const char *name : {"ROCP_TOOL_LIBRARIES", "ROCP_TOOL_LIB", "HSA_TOOLS_LIB"}) {
            const char *v = getenv(name);
            profiled = profiled || (v && *v);
        }
        const char *pre = getenv("LD_PRELOAD");
        profiled = profiled || (pre && (strstr(pre, "rocprof") || strstr(pre, "roctracer")));
        g_eng.graph = profiled ? 0 : 1;
    }
    const int mode = runner_mode(r);
    if (!g_eng.graph || r->profiling || mode == 0 || r->cap_B < 1 || r->cap_D[0] < 1 || r->n_single < 2) return 0;
    const int ndim = r->ndim;
    hipStream_t st = r->lanes[0];
    if (!r->h_pin && hipHostMalloc((void **)&r->h_pin, sizeof(double) * (ndim + 1)) != hipSuccess) return 0;
    if (r->g1 && r->g1_mode != mode) { (void)hipGraphExecDestroy(r->g1); r->g1 = nullptr; }
    if (!r->g1) {
        hipGraph_t graph = nullptr;
        if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) != hipSuccess) return 0;
        bool ok = hipMemcpyAsync(r->d_U, r->h_pin, sizeof(double) * ndim, hipMemcpyHostToDevice, st) == hipSuccess;
        ok = ok && run_batch(r, nullptr, r->d_U, r->d_lnL, nullptr, 1, true, 0) == NFA_OK;
        ok = ok && hipMemcpyAsync(r->h_pin, r->d_U, sizeof(double) * ndim, hipMemcpyDeviceToHost, st) == hipSuccess;
        ok = ok && hipMemcpyAsync(r->h_pin + ndim, r->d_lnL, sizeof(double), hipMemcpyDeviceToHost, st) == hipSuccess;
        const bool ended = hipStreamEndCapture(st, &graph) == hipSuccess && graph;
        if (!ok || !ended || hipGraphInstantiate(&r->g1, graph, nullptr, nullptr, 0) != hipSuccess) {
            if (graph) (void)hipGraphDestroy(graph);
            r->g1 = nullptr;
            (void)hipGetLastError();
            r->n_single = 0;                         // do not try again right away
            return 0;
        }
        (void)hipGraphDestroy(graph);
        r->g1_mode = mode;
    }
    memcpy(r->h_pin, U, sizeof(double) * ndim);
    if (hipGraphLaunch(r->g1, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return 0;
    r->lane_busy &= ~1u;
    memcpy(U, r->h_pin, sizeof(double) * ndim);
    *lnL = r->h_pin[ndim];
    return 1;
}

extern "C" {

// The device's view of host memory it can address (pinned and mapped: nfa_host_alloc, hipHostMalloc,
// hipHostRegister), nullptr for ordinary pageable memory.
static void *mapped_view(const void *host) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, host) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if (a.type != hipMemoryTypeHost || !a.devicePointer) return nullptr;
    return a.devicePointer;
}

// Pinned, device-addressable host memory for the buffers of the host-pointer entry points.
int nfa_host_alloc(void **out, size_t bytes) {
    if (!out || bytes == 0) return fail(NFA_ERR_ARG, "null argument");
    int rc = engine_init(); if (rc) return rc;
    HIP_TRY(hipHostMalloc(out, bytes, hipHostMallocMapped | hipHostMallocPortable));
    return NFA_OK;
}
int nfa_host_free(void *p) {
    if (!p) return NFA_OK;
    HIP_TRY(hipHostFree(p));
    return NFA_OK;
}

int nfa_runner_loglike_batch(nfa_runner *r, const int32_t *pix, double *U, double *lnL, int64_t B) {
    if (!r || !U || !lnL) return fail(NFA_ERR_ARG, "null argument");
    if (B <= 0) return NFA_OK;
    int rc = check_pix(r, pix, B); if (rc) return rc;
    if (!r->pr) return fail(NFA_ERR_STATE, "runner has no priors (predict-only)");
    RUNNER_LOCK(r);
    rc = sync_all_lanes(r); if (rc) return rc;           // the staging buffers are shared
    rc = runner_reserve(r, B, false); if (rc) return rc;
    if (B <= NFA_POINT_MAXB) {                           // MultiNest-style single points, a broker's handful: one launch, no copies
        const int served = few_points_kernel(r, pix, U, lnL, B);
        if (served < 0) return NFA_ERR_DEVICE;
        if (served) return NFA_OK;
    }
    if (B == 1 && !pix) {                                // ... or the batch kernels replayed as a graph
        r->n_single += 1;
        if (single_point_graph(r, U, lnL)) return NFA_OK;
    }
    // Large batches go through the stream lanes in chunks: the kernels of chunk c run while the
    // host copies chunk c+1 in, and the results of chunk c come back while c+1 computes.  (Every
    // per-item result is independent of the batch it travels in.)
    // A buffer the device can address itself (nfa_host_alloc, or memory the caller registered with the
    // runtime) is not copied at all: the set-up kernel reads the unit cube over the bus and writes theta back
    // in place, the sum kernel writes lnL there.
    double *vU = (double *)mapped_view(U), *vL = (double *)mapped_view(lnL);
    const int32_t *vP = pix ? (const int32_t *)mapped_view(pix) : nullptr;
    const int n_chunks = (B >= 16384 && r->n_lanes > 1) ? (int)std::min<int64_t>(r->lanes_auto ? 4 : r->n_lanes, B / 4096) : 1;
    const int64_t per = ((B + n_chunks - 1) / n_chunks + 63) / 64 * 64;
    const int ndim = r->ndim;
    for (int c = 0; c < n_chunks; ++c) {
        const int64_t b0 = c * per, nb = std::min<int64_t>(per, B - b0);
        if (nb <= 0) break;
        hipStream_t st = r->lanes[c];
        if (!vU) HIP_TRY(hipMemcpyAsync(r->d_U + b0 * ndim, U + b0 * ndim, sizeof(double) * nb * ndim, hipMemcpyHostToDevice, st));
        if (pix && !vP) HIP_TRY(hipMemcpyAsync(r->d_pix + b0, pix + b0, sizeof(int) * nb, hipMemcpyHostToDevice, st));
        rc = run_batch(r, pix ? (vP ? vP + b0 : r->d_pix + b0) : nullptr, vU ? vU + b0 * ndim : r->d_U + b0 * ndim,
                       vL ? vL + b0 : r->d_lnL + b0, nullptr, nb, true, c);
        if (rc) return rc;
    }
    for (int c = 0; c < n_chunks; ++c) {
        const int64_t b0 = c * per, nb = std::min<int64_t>(per, B - b0);
        if (nb <= 0) break;
        hipStream_t st = r->lanes[c];
        if (!vU) HIP_TRY(hipMemcpyAsync(U + b0 * ndim, r->d_U + b0 * ndim, sizeof(double) * nb * ndim, hipMemcpyDeviceToHost, st));
        if (!vL) HIP_TRY(hipMemcpyAsync(lnL + b0, r->d_lnL + b0, sizeof(double) * nb, hipMemcpyDeviceToHost, st));
    }
    for (int c = 0; c < n_chunks; ++c) HIP_TRY(hipStreamSynchronize(r->lanes[c]));
    r->lane_busy &= ~((1u << n_chunks) - 1u);
    return NFA_OK;
}

int nfa_runner_predict_batch(nfa_runner *r, const int32_t *pix, const double *theta, int64_t B,
                             double *spectra_out, double *lnL_out) {
    if (!r || !theta) return fail(NFA_ERR_ARG, "null argument");
    if (B <= 0) return NFA_OK;
    int rc = check_pix(r, pix, B); if (rc) return rc;
    RUNNER_LOCK(r);
    rc = sync_all_lanes(r); if (rc) return rc;
    // output buffers the device can address (nfa_host_alloc) are written by the kernels themselves: the spectra
    // -- B x chan_tot doubles, the bulk of this call's traffic -- then cross the bus once, without a staging copy
    double *vS = spectra_out ? (double *)mapped_view(spectra_out) : nullptr;
    double *vL = lnL_out ? (double *)mapped_view(lnL_out) : nullptr;
    rc = runner_reserve(r, B, spectra_out != nullptr && !vS); if (rc) return rc;
    hipStream_t st = r->lanes[0];
    HIP_TRY(hipMemcpyAsync(r->d_U, theta, sizeof(double) * B * r->ndim, hipMemcpyHostToDevice, st));
    if (pix) HIP_TRY(hipMemcpyAsync(r->d_pix, pix, sizeof(int) * B, hipMemcpyHostToDevice, st));
    rc = run_batch(r, pix ? r->d_pix : nullptr, r->d_U, vL ? vL : r->d_lnL, spectra_out ? (vS ? vS : r->d_spec) : nullptr, B,
                   false, 0);
    if (rc) return rc;
    if (spectra_out && !vS)
        HIP_TRY(hipMemcpyAsync(spectra_out, r->d_spec, sizeof(double) * B * r->ss->dev.chan_tot,
                               hipMemcpyDeviceToHost, st));
    if (lnL_out && !vL)
        HIP_TRY(hipMemcpyAsync(lnL_out, r->d_lnL, sizeof(double) * B, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    r->lane_busy &= ~1u;
    return NFA_OK;
}

// The spectra-out call for a caller whose buffers live in HBM: theta in, model spectra (and, where asked for, lnL)
// out, nothing copied, nothing waited for -- what deblend_hf_intensity / generate_predicted_profiles
// (nestfit/main.py:1106-1113, 1182-1188) become when the MAP cube and the profile cube stay on the device.
// Consecutive calls rotate over the runner's stream lanes like nfa_runner_loglike_batch_dev's.
int nfa_runner_predict_batch_dev(nfa_runner *r, const int32_t *d_pix, const double *d_theta, int64_t B,
                                 double *d_spectra, double *d_lnL) {
    if (!r || !d_theta || (!d_spectra && !d_lnL)) return fail(NFA_ERR_ARG, "null argument");
    if (B <= 0) return NFA_OK;
    RUNNER_LOCK(r);
    // (coalesced like the likelihood's batches: a launch of one 4096-row batch is one wave per wave slot and as long as its
    // longest wave, 37.8 us against 26 per batch in a launch of eight)
    return enqueue_dev(r, d_pix, const_cast<double *>(d_theta), d_lnL, d_spectra, B, false);
}

}  // extern "C"

// ---- posterior moments of model spectra (nfa_moments.h, nfa_moments_plan.h) -------------------------------------
static int mom_reserve_rows(nfa_runner *r, int64_t rows) {
    MomScratch &m = r->mom;
    if (rows <= m.cap_rows) return NFA_OK;
    (void)hipFree(m.d_stat); (void)hipFree(m.d_w); (void)hipFree(m.d_pieces);
    for (int k = 0; k < 2; ++k) { if (m.h_stage[k]) (void)hipHostFree(m.h_stage[k]); m.h_stage[k] = nullptr; }
    m.d_stat = nullptr; m.d_w = nullptr; m.d_pieces = nullptr; m.cap_rows = 0;
    HIP_TRY(hipMalloc(&m.d_stat, sizeof(double) * mom_stat_doubles(rows, r->ss->dev.n_spec)));
    HIP_TRY(hipMalloc(&m.d_w, sizeof(double) * rows));
    HIP_TRY(hipMalloc(&m.d_pieces, sizeof(MomPiece) * rows));
    for (int k = 0; k < 2; ++k) {
        HIP_TRY(hipHostMalloc((void **)&m.h_stage[k], (sizeof(int32_t) + sizeof(MomPiece)) * rows, hipHostMallocDefault));
        if (!m.ev[k]) HIP_TRY(hipEventCreateWithFlags(&m.ev[k], hipEventDisableTiming));
    }
    m.cap_rows = rows;
    return NFA_OK;
}
static int mom_reserve_segs(nfa_runner *r, int64_t n_seg) {
    MomScratch &m = r->mom;
    if (n_seg <= m.cap_seg) return NFA_OK;
    (void)hipFree(m.d_ref); (void)hipFree(m.d_acc); (void)hipFree(m.d_sref); (void)hipFree(m.d_sacc); (void)hipFree(m.d_s0);
    m.d_ref = m.d_acc = m.d_sref = m.d_sacc = m.d_s0 = nullptr; m.cap_seg = 0;
    const int64_t chan_tot = r->ss->dev.chan_tot, nstat = 2 * r->ss->dev.n_spec;
    HIP_TRY(hipMalloc(&m.d_ref, sizeof(double) * mom_ref_doubles(n_seg, chan_tot)));
    HIP_TRY(hipMalloc(&m.d_acc, sizeof(double) * mom_acc_doubles(n_seg, chan_tot)));
    HIP_TRY(hipMalloc(&m.d_sref, sizeof(double) * mom_ref_doubles(n_seg, nstat)));
    HIP_TRY(hipMalloc(&m.d_sacc, sizeof(double) * mom_acc_doubles(n_seg, nstat)));
    HIP_TRY(hipMalloc(&m.d_s0, sizeof(double) * n_seg));
    m.cap_seg = n_seg;
    return NFA_OK;
}
static MomSpecs mom_specs(const nfa_runner *r) {
    MomSpecs S = {};
    S.n_spec = r->ss->dev.n_spec;
    for (int s = 0; s < S.n_spec; ++s) { S.size[s] = r->ss->dev.size[s]; S.off[s] = r->ss->dev.off[s]; }
    return S;
}
// peak and total of `rows` rows of spec[rows][chan_tot] on the runner's stream (step: see row_stats_kernel)
static int launch_row_stats(nfa_runner *r, const double *d_spec, int64_t rows, double *d_peak, double *d_total, int step) {
    hipLaunchKernelGGL(row_stats_kernel, dim3((unsigned)mom_stat_blocks(rows, r->ss->dev.n_spec)), dim3(MOM_STAT_WAVES * 64), 0, r->lanes[0],
                       d_spec, (long)rows, (long)r->ss->dev.chan_tot, mom_specs(r), r->ss->dev.cont != nullptr ? 1 : 0, d_peak, d_total, step);
    HIP_TRY(hipGetLastError());
    return NFA_OK;
}
static int launch_accumulate(nfa_runner *r, const double *d_x, int64_t ld, int64_t ncol, const double *d_w, int64_t n_pieces,
                             int64_t max_rows, const double *d_ref, double *d_acc, int64_t n_seg) {
    const MomGeom G = mom_geom(n_pieces, ncol, max_rows, g_eng.n_cu);
    hipLaunchKernelGGL(moments_accumulate_kernel, dim3(G.grid_x, G.grid_y), dim3(G.threads), G.lds, r->lanes[0],
                       d_x, (long)ld, (long)ncol, d_w, (const MomPiece *)r->mom.d_pieces, d_ref, d_acc, (long)n_seg, G.R);
    HIP_TRY(hipGetLastError());
    return NFA_OK;
}

// The moments of nfa_runner_predict_moments once its arguments are checked, S0 of every segment is summed and the lanes
// are idle (the caller holds the runner's lock): scratch, reference rows, the chunk loop, the finish and the copies out.
// The rows are the host's (T.host, with the segments' reference rows in T.ref: copied into the staging chunk by chunk) or
// lie on the device with equal weights and segments of seg_off[1] rows each (T.dev: the batch reads a chunk's rows where
// they are -- run_batch without a prior writes none of its rows -- and the reference rows are gathered on the device).
struct MomRows { const double *host, *dev, *ref; };
static int mom_reduce(nfa_runner *r, int64_t n_seg, const int32_t *seg_pix, const int64_t *seg_off, MomRows T, const double *weight,
                      const double *s0, int64_t chunk, double *spec_mean, double *spec_std, double *stat_mean, double *stat_std) {
    const int ndim = r->ndim;
    const int64_t chan_tot = r->ss->dev.chan_tot, nstat = 2 * r->ss->dev.n_spec, rows = seg_off[n_seg];
    const bool want_spec = spec_mean || spec_std, want_stat = stat_mean || stat_std;
    int rc = runner_reserve(r, chunk, true); if (rc) return rc;
    rc = mom_reserve_rows(r, chunk); if (rc) return rc;
    rc = mom_reserve_segs(r, n_seg); if (rc) return rc;
    MomScratch &m = r->mom;
    hipStream_t st = r->lanes[0];
    HIP_TRY(hipMemcpyAsync(m.d_s0, s0, sizeof(double) * n_seg, hipMemcpyHostToDevice, st));
    if (want_spec) HIP_TRY(hipMemsetAsync(m.d_acc, 0, sizeof(double) * mom_acc_doubles(n_seg, chan_tot), st));
    if (want_stat) HIP_TRY(hipMemsetAsync(m.d_sacc, 0, sizeof(double) * mom_acc_doubles(n_seg, nstat), st));
    // the reference rows: ordinary predict launches of n_seg rows into ref[n_seg][chan_tot], their statistics taken there
    for (int64_t b0 = 0; b0 < n_seg; b0 += r->cap_B) {
        const int64_t nb = std::min<int64_t>(r->cap_B, n_seg - b0);
        if (T.dev) {
            hipLaunchKernelGGL(moments_first_rows_kernel, dim3((unsigned)((nb * ndim + 255) / 256)), dim3(256), 0, st, T.dev, (long)seg_off[1],
                               (long)b0, (long)nb, ndim, r->d_U);
            HIP_TRY(hipGetLastError());
        } else
            HIP_TRY(hipMemcpyAsync(r->d_U, T.ref + b0 * ndim, sizeof(double) * nb * ndim, hipMemcpyHostToDevice, st));
        if (seg_pix) HIP_TRY(hipMemcpyAsync(r->d_pix, seg_pix + b0, sizeof(int) * nb, hipMemcpyHostToDevice, st));
        rc = run_batch(r, seg_pix ? r->d_pix : nullptr, r->d_U, r->d_lnL, m.d_ref + b0 * chan_tot, nb, false, 0);
        if (rc) return rc;
    }
    if (want_stat) { rc = launch_row_stats(r, m.d_ref, n_seg, m.d_sref, m.d_sref + 1, 2); if (rc) return rc; }
    // chunk by chunk: predict into the spectra scratch, reduce there
    const int64_t n_chunks = mom_n_chunks(rows, chunk);
    int64_t cursor = 0;
    for (int64_t c = 0; c < n_chunks; ++c) {
        const int64_t a = c * chunk, nb = std::min(chunk, rows - a);
        const int slot = (int)(c & 1);
        if (c >= 2) HIP_TRY(hipEventSynchronize(m.ev[slot]));          // the copies out of this slot two chunks ago
        int32_t *h_pix = (int32_t *)m.h_stage[slot];
        MomPiece *h_pieces = (MomPiece *)(m.h_stage[slot] + sizeof(int32_t) * m.cap_rows);
        const int64_t n_pieces = mom_cut(seg_off, n_seg, chunk, c, &cursor, h_pieces);
        int64_t max_rows = 0;
        for (int64_t k = 0; k < n_pieces; ++k) {
            max_rows = std::max<int64_t>(max_rows, h_pieces[k].n);
            if (seg_pix) std::fill(h_pix + h_pieces[k].row0, h_pix + h_pieces[k].row0 + h_pieces[k].n, seg_pix[h_pieces[k].seg]);
        }
        if (T.host) HIP_TRY(hipMemcpyAsync(r->d_U, T.host + a * ndim, sizeof(double) * nb * ndim, hipMemcpyHostToDevice, st));
        if (weight) HIP_TRY(hipMemcpyAsync(m.d_w, weight + a, sizeof(double) * nb, hipMemcpyHostToDevice, st));
        if (seg_pix) HIP_TRY(hipMemcpyAsync(r->d_pix, h_pix, sizeof(int32_t) * nb, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(m.d_pieces, h_pieces, sizeof(MomPiece) * n_pieces, hipMemcpyHostToDevice, st));
        HIP_TRY(hipEventRecord(m.ev[slot], st));
        double *d_rows = T.host ? r->d_U : const_cast<double *>(T.dev) + a * ndim;
        rc = run_batch(r, seg_pix ? r->d_pix : nullptr, d_rows, r->d_lnL, r->d_spec, nb, false, 0);
        if (rc) return rc;
        const double *d_w = weight ? m.d_w : nullptr;
        if (want_spec) {
            rc = launch_accumulate(r, r->d_spec, chan_tot, chan_tot, d_w, n_pieces, max_rows, m.d_ref, m.d_acc, n_seg);
            if (rc) return rc;
        }
        if (want_stat) {
            rc = launch_row_stats(r, r->d_spec, nb, m.d_stat, m.d_stat + 1, 2); if (rc) return rc;
            rc = launch_accumulate(r, m.d_stat, nstat, nstat, d_w, n_pieces, max_rows, m.d_sref, m.d_sacc, n_seg);
            if (rc) return rc;
        }
    }
    if (want_spec) {
        const int64_t n = n_seg * chan_tot;
        hipLaunchKernelGGL(moments_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, m.d_acc, (const double *)m.d_ref,
                           (const double *)m.d_s0, (long)n_seg, (long)chan_tot);
        HIP_TRY(hipGetLastError());
        if (spec_mean) HIP_TRY(hipMemcpyAsync(spec_mean, m.d_acc, sizeof(double) * n, hipMemcpyDeviceToHost, st));
        if (spec_std) HIP_TRY(hipMemcpyAsync(spec_std, m.d_acc + n, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    }
    if (want_stat) {
        const int64_t n = n_seg * nstat;
        hipLaunchKernelGGL(moments_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, m.d_sacc, (const double *)m.d_sref,
                           (const double *)m.d_s0, (long)n_seg, (long)nstat);
        HIP_TRY(hipGetLastError());
        if (stat_mean) HIP_TRY(hipMemcpyAsync(stat_mean, m.d_sacc, sizeof(double) * n, hipMemcpyDeviceToHost, st));
        if (stat_std) HIP_TRY(hipMemcpyAsync(stat_std, m.d_sacc + n, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    r->lane_busy &= ~1u;
    return NFA_OK;
}

extern "C" {

int nfa_runner_predict_moments(nfa_runner *r, int64_t n_seg, const int32_t *seg_pix, const int64_t *seg_off, const double *theta,
                               const double *weight, int64_t chunk_rows, double *spec_mean, double *spec_std,
                               double *stat_mean, double *stat_std) {
    if (!r) return fail(NFA_ERR_ARG, "null runner");
    if (n_seg < 0 || n_seg > INT32_MAX) return fail(NFA_ERR_ARG, "the number of segments is out of range");
    if (!spec_mean && !spec_std && !stat_mean && !stat_std) return fail(NFA_ERR_ARG, "predict_moments: all four outputs are null");
    if (const char *why = mom_check_chunk_rows(chunk_rows)) return fail(NFA_ERR_ARG, why);
    if (n_seg == 0) return NFA_OK;
    if (!seg_off) return fail(NFA_ERR_ARG, "null argument");
    if (seg_off[0] != 0) return fail(NFA_ERR_ARG, "segment offsets start at 0");
    for (int64_t g = 0; g < n_seg; ++g)
        if (seg_off[g + 1] < seg_off[g]) return fail(NFA_ERR_ARG, "segment offsets must not decrease");
    const int64_t rows = seg_off[n_seg];
    if (rows > 0 && !theta) return fail(NFA_ERR_ARG, "null argument");
    int rc = check_pix(r, seg_pix, n_seg); if (rc) return rc;
    if (weight)
        for (int64_t i = 0; i < rows; ++i)
            if (!(weight[i] >= 0.0) || !std::isfinite(weight[i])) return fail(NFA_ERR_ARG, "a weight is finite and >= 0");
    const int64_t chan_tot = r->ss->dev.chan_tot, nstat = 2 * r->ss->dev.n_spec, chunk = mom_chunk_rows(chunk_rows);
    if (rows == 0) {                                         // nothing to predict: every segment is empty
        for (double *out : {spec_mean, spec_std}) if (out) std::fill(out, out + n_seg * chan_tot, (double)NAN);
        for (double *out : {stat_mean, stat_std}) if (out) std::fill(out, out + n_seg * nstat, (double)NAN);
        return NFA_OK;
    }
    // S0 and the reference row of every segment: the row of largest weight, the first on ties (an empty segment borrows
    // a row: its S0 = 0 makes every output NaN whatever that row's spectrum is)
    const int ndim = r->ndim;
    std::vector<double> s0((size_t)n_seg), ref_theta((size_t)n_seg * ndim);
    for (int64_t g = 0; g < n_seg; ++g) {
        int64_t best = std::min(seg_off[g], rows - 1);
        double sum = 0.0;
        for (int64_t i = seg_off[g]; i < seg_off[g + 1]; ++i) {
            const double w = weight ? weight[i] : 1.0;
            sum += w;
            if (w > (weight ? weight[best] : 1.0)) best = i;
        }
        s0[(size_t)g] = sum;
        std::copy(theta + best * ndim, theta + (best + 1) * ndim, ref_theta.begin() + (size_t)g * ndim);
    }
    RUNNER_LOCK(r);
    rc = sync_all_lanes(r); if (rc) return rc;
    return mom_reduce(r, n_seg, seg_pix, seg_off, MomRows{theta, nullptr, ref_theta.data()}, weight, s0.data(), chunk,
                      spec_mean, spec_std, stat_mean, stat_std);
}

int nfa_runner_row_statistics(nfa_runner *r, const int32_t *pix, const double *theta, int64_t B, double *peak, double *total) {
    if (!r || !theta || !peak || !total) return fail(NFA_ERR_ARG, "null argument");
    if (B <= 0) return NFA_OK;
    int rc = check_pix(r, pix, B); if (rc) return rc;
    RUNNER_LOCK(r);
    rc = sync_all_lanes(r); if (rc) return rc;
    const int64_t chunk = std::min<int64_t>(MOM_CHUNK_ROWS, (B + 63) / 64 * 64);
    rc = runner_reserve(r, chunk, true); if (rc) return rc;
    rc = mom_reserve_rows(r, chunk); if (rc) return rc;
    MomScratch &m = r->mom;
    hipStream_t st = r->lanes[0];
    const int n_spec = r->ss->dev.n_spec, ndim = r->ndim;
    double *d_peak = m.d_stat, *d_total = m.d_stat + m.cap_rows * n_spec;
    for (int64_t a = 0; a < B; a += chunk) {
        const int64_t nb = std::min(chunk, B - a);
        HIP_TRY(hipMemcpyAsync(r->d_U, theta + a * ndim, sizeof(double) * nb * ndim, hipMemcpyHostToDevice, st));
        if (pix) HIP_TRY(hipMemcpyAsync(r->d_pix, pix + a, sizeof(int) * nb, hipMemcpyHostToDevice, st));
        rc = run_batch(r, pix ? r->d_pix : nullptr, r->d_U, r->d_lnL, r->d_spec, nb, false, 0);
        if (rc) return rc;
        rc = launch_row_stats(r, r->d_spec, nb, d_peak, d_total, 1); if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(peak + a * n_spec, d_peak, sizeof(double) * nb * n_spec, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(total + a * n_spec, d_total, sizeof(double) * nb * n_spec, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    r->lane_busy &= ~1u;
    return NFA_OK;
}

}  // extern "C"

// ---- normal equations of a least-squares fit (nfa_lsq.h, nfa_lsq_plan.h) ------------------------------------------
static int lsq_reserve(nfa_runner *r, int64_t B) {
    LsqScratch &q = r->lsq;
    if (B <= q.cap_B) return NFA_OK;
    (void)hipFree(q.d_buf); (void)hipFree(q.d_pix);
    q.d_buf = nullptr; q.d_pix = nullptr; q.cap_B = 0;
    HIP_TRY(hipMalloc(&q.d_buf, sizeof(double) * lsq_scratch(B, r->ndim).total));
    HIP_TRY(hipMalloc(&q.d_pix, sizeof(int) * B));
    q.cap_B = B;
    return NFA_OK;
}

extern "C" {

int nfa_runner_normal_equations(nfa_runner *r, const int32_t *pix, const double *theta, int64_t B, const double *step,
                                const double *lower, const double *upper, int64_t chunk_rows, double *chi2, double *grad, double *curv) {
    if (!r) return fail(NFA_ERR_ARG, "null runner");
    if (B < 0 || B > INT32_MAX) return fail(NFA_ERR_ARG, "the number of points is out of range");
    const int ndim = r->ndim;
    if (const char *why = lsq_check_ndim(ndim)) return fail(NFA_ERR_ARG, why);
    const int nj = grad || curv ? ndim : 0;                  // probed parameters: none for chi^2 alone
    if (const char *why = lsq_check_chunk_rows(chunk_rows, nj)) return fail(NFA_ERR_ARG, why);
    if (nj && !step) return fail(NFA_ERR_ARG, "normal_equations: grad or curv without step");
    if (nj) {
        for (int k = 0; k < ndim; ++k) {
            if (!(step[k] > 0.0) || !std::isfinite(step[k])) return fail(NFA_ERR_ARG, "a step is finite and > 0");
            if (lower && upper && lower[k] > upper[k]) return fail(NFA_ERR_ARG, "a lower bound lies above its upper bound");
            if ((lower && lower[k] != lower[k]) || (upper && upper[k] != upper[k])) return fail(NFA_ERR_ARG, "a bound is NaN");
        }
    }
    if (const char *why = lsq_refusal(specset_has(r->ss))) return fail(NFA_ERR_STATE, why);
    if (B == 0) return NFA_OK;
    if (!theta || !chi2) return fail(NFA_ERR_ARG, "null argument");
    int rc = check_pix(r, pix, B); if (rc) return rc;
    const int R = lsq_rows_per_point(nj);
    const int64_t chunk = lsq_chunk_rows(chunk_rows), per = lsq_points_per_chunk(chunk_rows, nj);
    RUNNER_LOCK(r);
    rc = sync_all_lanes(r); if (rc) return rc;
    rc = runner_reserve(r, chunk, true); if (rc) return rc;
    rc = lsq_reserve(r, B); if (rc) return rc;
    const LsqScratchPlan P = lsq_scratch(r->lsq.cap_B, ndim);
    double *buf = r->lsq.d_buf;
    hipStream_t st = r->lanes[0];
    HIP_TRY(hipMemcpyAsync(buf + P.theta, theta, sizeof(double) * B * ndim, hipMemcpyHostToDevice, st));
    if (pix) HIP_TRY(hipMemcpyAsync(r->lsq.d_pix, pix, sizeof(int) * B, hipMemcpyHostToDevice, st));
    if (nj) {
        HIP_TRY(hipMemcpyAsync(buf + P.step, step, sizeof(double) * ndim, hipMemcpyHostToDevice, st));
        if (lower) HIP_TRY(hipMemcpyAsync(buf + P.lower, lower, sizeof(double) * ndim, hipMemcpyHostToDevice, st));
        if (upper) HIP_TRY(hipMemcpyAsync(buf + P.upper, upper, sizeof(double) * ndim, hipMemcpyHostToDevice, st));
    }
    const int *d_ppix = pix ? r->lsq.d_pix : nullptr;
    const SpecDev S = runner_specdev(r);
    for (int64_t a = 0; a < B; a += per) {                   // chunk by chunk: probe rows, predict, reduce
        const int64_t np = std::min(per, B - a);
        hipLaunchKernelGGL(lsq_probe_kernel, dim3(lsq_probe_blocks(np, nj)), dim3(256), 0, st, (const double *)(buf + P.theta + a * ndim),
                           d_ppix ? d_ppix + a : nullptr, (long)np, ndim, nj, (const double *)(buf + P.step),
                           lower ? (const double *)(buf + P.lower) : nullptr, upper ? (const double *)(buf + P.upper) : nullptr,
                           r->d_U, r->d_pix, buf + P.inv_d + a * ndim);
        HIP_TRY(hipGetLastError());
        rc = run_batch(r, pix ? r->d_pix : nullptr, r->d_U, r->d_lnL, r->d_spec, np * R, false, 0);
        if (rc) return rc;
        const LsqGeom G = lsq_geom(nj, np);
        hipLaunchKernelGGL(G.ept == 2 ? lsq_gram_kernel<2> : lsq_gram_kernel<4>, dim3(G.grid), dim3(G.threads), G.lds, st,
                           (const double *)r->d_spec, S, d_ppix, (const double *)(buf + P.inv_d), (long)a, nj, buf + P.chi2, buf + P.grad,
                           buf + P.curv);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(chi2, buf + P.chi2, sizeof(double) * B, hipMemcpyDeviceToHost, st));
    if (grad) HIP_TRY(hipMemcpyAsync(grad, buf + P.grad, sizeof(double) * B * ndim, hipMemcpyDeviceToHost, st));
    if (curv) HIP_TRY(hipMemcpyAsync(curv, buf + P.curv, sizeof(double) * B * ndim * ndim, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    r->lane_busy &= ~1u;
    return NFA_OK;
}

}  // extern "C"

extern "C" {

void nfa_loglike_callback(double *Cube, int *ndim, int *npars, double *lnew, void *ctx) {
    (void)npars;
    nfa_runner *r = (nfa_runner *)ctx;
    if (!r || !Cube || !lnew || !ndim || *ndim != r->ndim) {
        if (lnew) *lnew = NAN;
        return;
    }
    if (nfa_runner_loglike_batch(r, nullptr, Cube, lnew, 1) != NFA_OK) *lnew = NAN;
}

// ---- device memory + events -------------------------------------------------
int nfa_malloc(void **dptr, int64_t bytes) {
    int rc = engine_init(); if (rc) return rc;
    HIP_TRY(hipMalloc(dptr, (size_t)bytes));
    return NFA_OK;
}
int nfa_free(void *dptr) { HIP_TRY(hipFree(dptr)); return NFA_OK; }
int nfa_memcpy_h2d(void *dst, const void *src, int64_t bytes) {
    HIP_TRY(hipMemcpy(dst, src, (size_t)bytes, hipMemcpyHostToDevice)); return NFA_OK;
}
int nfa_memcpy_d2h(void *dst, const void *src, int64_t bytes) {
    HIP_TRY(hipMemcpy(dst, src, (size_t)bytes, hipMemcpyDeviceToHost)); return NFA_OK;
}
int nfa_memcpy_d2d(void *dst, const void *src, int64_t bytes) {
    HIP_TRY(hipMemcpy(dst, src, (size_t)bytes, hipMemcpyDeviceToDevice)); return NFA_OK;
}
int nfa_event_create(void **ev) {
    int rc = engine_init(); if (rc) return rc;
    hipEvent_t e; HIP_TRY(hipEventCreate(&e)); *ev = (void *)e; return NFA_OK;
}
int nfa_event_destroy(void *ev) { HIP_TRY(hipEventDestroy((hipEvent_t)ev)); return NFA_OK; }
int nfa_event_record(void *ev, nfa_runner *r) {
    if (r) {                 // batches held for coalescing are launched first: the event stands behind everything enqueued so far
        RUNNER_LOCK(r);
        int rc = flush_pending(r); if (rc) return rc;
        HIP_TRY(hipEventRecord((hipEvent_t)ev, r->stream));
        return NFA_OK;
    }
    HIP_TRY(hipEventRecord((hipEvent_t)ev, 0)); return NFA_OK;
}
int nfa_event_synchronize(void *ev) { HIP_TRY(hipEventSynchronize((hipEvent_t)ev)); return NFA_OK; }
int nfa_event_elapsed_ms(void *start, void *stop, float *ms) {
    HIP_TRY(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop)); return NFA_OK;
}

}  // extern "C"

#include "nfa_broker.h"
#include "nfa_ring.h"
#include "nfa_ring_serve.h"
#include "nfa_sampler.h"
#include "nfa_ensemble.h"
#include "nfa_comm.h"
#ifdef NFA_TEST_HOOKS
#include "nfa_testhooks.h"      // libnestfit_amd_test.so only
#endif
