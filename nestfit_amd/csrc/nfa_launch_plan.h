// nfa_launch_plan.h -- every launch of a runner's kernels, decided on the host: which kernel instance, how many
// workgroups and waves, how much dynamic LDS.
//
// Standard C++17 without a HIP include: a host compiler builds this header alone, so every decision can be tested on a
// machine without a GPU (tests/test_launch_plan.py).  It holds the layout constants the kernels and the plans share (one
// definition each: nfa_device.h and nfa_setup.h include this file), the plain inputs -- LpShape: a runner, filled once
// at its creation; LpLaunch: one launch; LpKnobs: the process options, filled per call -- and one chain of functions in
// dependency order.  Arithmetic only: no lock, no allocation, no call into the runtime; the plans live on the caller's
// stack.  Errors travel as `const char *error`, in the words the engine fails with.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include "../../include/nestfit_amd.h"

#define MAXSPEC   16
#define T0_SIZE   1000
// table layout inside g_tabs (doubles); the LDS copy starts at SM_EXP2
#define SM_T0X    0
#define SM_T0Y    1000
#define NFA_EXP2_N 256        // entries of the polynomial mode's table
#define SM_EXP2   2000        // 2^(i/256), i = 0..255        (poly)
// (table; C first, A last: a lane outside the tables' range -- it is given its value by the branch for such
// arguments -- still forms an address from its exponent bits, up to row 15 of a 10-row table: behind C lies B,
// behind B lies A, behind A at least SM_TABLE_TAIL doubles of whatever the kernel keeps there)
#define SM_FEC    (SM_EXP2 + NFA_EXP2_N)   // exp(-j 2^(l-28)) [10][256]
#define SM_FEB    (SM_FEC + 2560)   // exp(-j 2^(l-20)) [10][256]
#define SM_FEA    (SM_FEB + 2560)   // exp(-(128+j) 2^(l-12)) [10][128]
#define SM_END_TABLE  (SM_FEA + 1280)   // 8432 doubles
#define SM_TABLE_TAIL 768               // doubles that must follow the staged tables in LDS (row 15 of A ends there)
#define SM_TABLE_DOUBLES (SM_END_TABLE - SM_EXP2)   // the table mode's staged tables: 6656 doubles, 52 KB
#define NFA_BL_NB  4            // moments every baseline form accumulates: P_0..P_3, whatever the order
#define NFA_TP_NB  (NFA_BL_NB + NFA_TMPL_MAX)   // ... and every form with nuisance templates: those and t_1..t_4, whatever their number
#define LNL_PARTS 4      // row parts of a unit: the fixed shape of its chi^2 sum
// (eight since round 5, four before: a table-mode launch spends its tail with fewer and fewer waves per SIMD, and eight
// batches in a launch halve that share: profiles/r05/queue_timeline.txt, 86.3 -> 87.8 M evaluations/s on the metric shape)
#ifndef NFA_GROUP_MAX
#define NFA_GROUP_MAX 8
#endif
#define QREC 12                 // doubles of an (item, component) partition record of the set-up stage
#define SETUP_TI 64
#define SETUP_THREADS 256
#define NFA_POINT_MAXDIM 24
#define POINT_THREADS 512
#define POINT_WAVES (POINT_THREADS / 64)
static const size_t LDS_PER_CU = 160 * 1024;      // LDS of a compute unit (gfx950), the most one workgroup can ask for
#define LP_WAVES_PER_CU 32      // wave slots of a compute unit as the plans count them
struct LnlGeom {
    int nhf_max;       // lines per component slot in the LDS line table
    int wave_doubles;  // LDS doubles per wave
    unsigned inv_nspec; // floor(2^32 / nspec) + 1: unit / nspec = mulhi(unit, inv_nspec) for unit < 2^28; 0: nspec == 1
    unsigned inv_nhf;   // floor(2^32 / nhf_max) + 1: p / nhf_max = mulhi(p, inv_nhf) for the few hundred (component, line) slots; 0: nhf_max == 1
    int split;          // waves that share one (item, spectrum) unit (1, 2, 4), each taking LNL_PARTS / split row parts
#ifdef NFA_TEST_HOOKS
    unsigned long long *trace;   // measurement (test library): per wave of the queue kernel 8 records {start, end, unit, position} in 10 ns ticks
#endif
    unsigned *queue;    // table mode, split == 1, launches of several units per wave slot (lnl_kernel_queue): the launch's
                        // chunk counter and, a 128-byte line behind it, its count of workgroups that have left
                        // (NFA_QUEUE_WORDS words, zero between launches); nullptr: one unit per wave (lnl_kernel)
    int ablate;        // timing experiments only: 1 skip Tb, 2 skip the line loop, 4 skip rows, 8 skip line set-up
};

// A runner: what does not change between its launches (the launch geometry: from the process options at its creation;
// prog_bytes, line_rec_bytes: sizeof(PriorProg) and sizeof(LineRec), which enter the LDS layouts)
struct LpShape {
    int n_spec, size[MAXSPEC], nhf_max, ncomp, ndim, model;
    int n_stage, stage_doubles;              // prior tables the set-up stage keeps in LDS (0, 0: none, or no priors)
    int wpb, wpb_table, lnl_cap, lnl_split, prog_bytes, line_rec_bytes;
};
// One launch: B items in `mode` (0 table, 2 fast), of a group of `group_n` batches of `group_each` rows; what the
// spectra set is right now (nfa_specset_set_baseline changes it) and whether the lane has its queue counters; filled: an
// LTE set with a beam filling factor per component (nfa_specset_create_lte_filled; in the struct's tail padding); layered:
// a set whose components absorb those behind them (nfa_specset_set_layered; the next byte of that padding, zero = summed);
// calibrated: a set with a calibration uncertainty per spectrum (nfa_specset_set_calibration; the last byte of that
// padding, zero = none)
struct LpLaunch { int64_t B; int mode, group_n; int64_t group_each; bool write_spec, has_prior, baseline, weighted, has_queue, filled, layered, calibrated; };
// The process options the decisions read, as they stand at the call (nfa_set_option)
struct LpKnobs { int n_cu, setup_ti, setup_threads, setup_sub, lnl_queue, lnl_queue_wg, coalesce, ablate; };

// items per workgroup (per group of a two-group workgroup) of the set-up kernel: option setup_ti, an A/B knob
inline int lp_setup_ti(const LpKnobs &k) { return k.setup_ti > 0 ? k.setup_ti : SETUP_TI; }
inline int64_t lp_wave_slots(const LpKnobs &k) { return (int64_t)k.n_cu * LP_WAVES_PER_CU; }
// Lanes a sequence of batches rotates over.  Four overlap the draining tail of one batch with the next; a batch of
// about one wave per wave slot (the metric's 4096 rows x 2 spectra) leaves the longest tail and gains another 3 % from
// six, smaller and larger ones lose with more than four (profiles/r02/sweep_lanes.txt).
inline int lp_lanes(const LpShape &s, const LpKnobs &k, int64_t B) {
    const int64_t units = B * s.n_spec, slots = lp_wave_slots(k);
    return (4 * units >= 3 * slots && 2 * units <= 3 * slots) ? 6 : 4;
}
// Coalescing of device-pointer batches of B rows: whether one may be held for its neighbours (whole set-up workgroups;
// a group stays below NFA_GROUP_MAX waves per slot), and whether a group of n of them takes no more
inline bool lp_may_hold(const LpShape &s, const LpKnobs &k, int64_t B, bool profiling) {
    return k.coalesce > 1 && !profiling && B % lp_setup_ti(k) == 0 && 2 * B * s.n_spec <= NFA_GROUP_MAX * lp_wave_slots(k);
}
inline bool lp_group_full(const LpShape &s, const LpKnobs &k, int n, int64_t B) {
    return n >= k.coalesce || (n + 1) * B * s.n_spec > NFA_GROUP_MAX * lp_wave_slots(k);
}

// the fast mode's narrow form (FastRec records, fp32 window test): at most 26 lines per transition (a 32-bit line
// mask per component) and channel indices that fp32 holds to the half (nfa_device.h: FastRec)
inline bool lnl_wide(const LpShape &s) {
    int max_size = 0;
    for (int k = 0; k < s.n_spec; ++k) max_size = std::max(max_size, s.size[k]);
    return s.nhf_max > 26 || max_size > (1 << 22);
}
// LDS doubles per (item, spectrum) unit: the line table (32-byte records, nhf_max per component) followed by the
// windows (two ints per line)
inline int lnl_wave_doubles(const LpShape &s) {
    const int per_line = s.line_rec_bytes / (int)sizeof(double) + 1;
    return (s.ncomp * s.nhf_max * per_line + 1) & ~1;                // 16-byte records: an even number of doubles
}
// LDS of a table-mode workgroup of `waves` waves with one wave per unit: the tables, the waves' line tables, the queue's words
inline size_t lnl_table_lds(const LpShape &s, int waves, int queue_bytes) {
    return sizeof(double) * ((size_t)SM_TABLE_DOUBLES + (size_t)lnl_wave_doubles(s) * waves) + queue_bytes;
}
// waves per workgroup of a table-mode launch with one wave per unit: the workgroup stages 51 KB of product tables, so it
// is made as fat as keeps the most waves resident per CU (ties: more workgroups, so that one stages while another computes)
inline int table_waves(const LpShape &s) {
    if (s.wpb_table > 0) return s.wpb_table;
    int best = -1, best_blocks = 0, waves = 16;
    for (int w = 4; w <= 16; w += 2) {
        const int blocks = (int)(LDS_PER_CU / lnl_table_lds(s, w, 0));
        const int resident = std::min(LP_WAVES_PER_CU, blocks * w);
        if (resident > best || (resident == best && blocks > best_blocks)) { best = resident; best_blocks = blocks; waves = w; }
    }
    return waves;
}
// workgroups of `waves` waves of the table mode that a CU holds at once
inline int table_wg_per_cu(const LpShape &s, int waves) {
    return std::max(1, std::min((int)(LDS_PER_CU / lnl_table_lds(s, waves, 16)), LP_WAVES_PER_CU / waves));
}
// waves per unit of a launch of B items (runner option lnl_split; 0 = by the size of the launch).  A launch with fewer
// units than a few per wave slot is latency bound: its waves are placed once and every SIMD waits for its own longest;
// splitting the rows of a unit over 2 or 4 waves gives the hardware shorter waves to place as slots free up (a single
// point: 2 units -> 8 waves).
inline int resolve_split(const LpShape &s, const LpKnobs &k, int64_t B) {
    int split = s.lnl_split;
    if (split == 0) {
        split = 1;
        while (split < LNL_PARTS && B * s.n_spec * split * 2 <= lp_wave_slots(k)) split *= 2;
    }
    int min_rows = 1 << 30;
    for (int i = 0; i < s.n_spec; ++i) min_rows = std::min(min_rows, (s.size[i] + 63) / 64);
    while (split > 1 && split > min_rows) split /= 2;
    return split;
}
// What of LnlGeom the runner and the size of the launch (B items) decide.  The queue and the test library's trace stay
// null: the engine sets them for a batch launch, the fused kernels have none.
inline LnlGeom lnl_geom(const LpShape &s, const LpKnobs &k, int64_t B) {
    LnlGeom G = {};
    G.nhf_max = s.nhf_max;
    G.inv_nspec = s.n_spec == 1 ? 0u : (unsigned)(0x100000000ull / (unsigned)s.n_spec) + 1u;
    G.inv_nhf = G.nhf_max == 1 ? 0u : (unsigned)(0x100000000ull / (unsigned)G.nhf_max) + 1u;
    G.split = resolve_split(s, k, B);
    G.wave_doubles = lnl_wave_doubles(s);
    return G;
}

// per-lane sums a part of a unit leaves in LDS when several waves share the unit: chi^2's, a baseline's NFA_BL_NB moments
// (with nuisance templates: NFA_TP_NB), a calibrated set's sum w p^2
inline int lnl_part_slots(bool baseline, bool calibrated, bool templates = false) {
    return 1 + (templates ? NFA_TP_NB : baseline ? NFA_BL_NB : 0) + (calibrated ? 1 : 0);
}
// Waves per workgroup of a launch with `split` waves per unit: option wpb, made a multiple of the split.  Table mode stages
// 51 KB of product tables per workgroup, so the workgroup is made as fat as keeps the most waves resident per CU
// (table_waves); its split launches take eight.
inline int lnl_waves(const LpShape &s, bool table, int split) {
    int waves = std::max(1, std::min(s.wpb, 16));
    waves = std::max(waves, split);
    waves -= waves % split;
    if (table) waves = split > 1 ? std::max(8, split) : table_waves(s);
    return waves;
}
// LDS in bytes of the units of a workgroup: per unit the line table and, split > 1, `slots` sums per part and lane
inline size_t lnl_units_lds(const LpShape &s, bool table, int split, int waves, int slots) {
    const size_t part_doubles = split > 1 ? (size_t)LNL_PARTS * 64 * slots : 0;
    return sizeof(double) * ((size_t)(table ? SM_TABLE_DOUBLES : 0) + ((size_t)lnl_wave_doubles(s) + part_doubles) * (waves / split));
}

// doubles of an item's derived record (nfa_device.h: drec_size): a leading block of four per component -- texs, a set of the
// excitation-grid model: per (component, spectrum) -- and DREC_CS = 16 per (component, spectrum)
constexpr int LP_DREC_CS = 16;
constexpr int lnl_drec_doubles(int ncomp, int nspec, bool texs = false) {
    return 4 * ncomp * (texs ? nspec : 1) + ncomp * nspec * LP_DREC_CS;
}
enum LnlForm { LNL_PLAIN, LNL_W8, LNL_QUEUE, LNL_WEIGHTED, LNL_BASELINE };
// waves per workgroup, its dynamic LDS in bytes, workgroups; error: null, or why there is no plan.  filled, layered,
// calibrated: the launch's (in the padding behind `wide`).  Which kernel instance a plan names: lnl_instance_exists below.
struct LnlPlan { LnlForm form; bool wide, filled, layered, calibrated; LnlGeom G; int waves; size_t lds; int64_t blocks; const char *error; };

// The kind of a spectra set: which of lnl_body's WEIGHTED, BASELINE, FILL, LAYER, CALIB flags its kernel switches on
// (lnl_kernel_kind<..., KIND>, nfa_device.h).  Kind 0 is the plain set: lnl_kernel, lnl_kernel_w8, lnl_kernel_queue.
// Behind the five kind bits, in the same word, the flags of lnl_body that no kind has: the side family's (LnlSide below).
enum : unsigned { LNL_K_WEIGHTED = 1, LNL_K_BASELINE = 2, LNL_K_FILL = 4, LNL_K_LAYER = 8, LNL_K_CALIB = 16,
                  LNL_F_CORR = 32, LNL_F_RESP = 64, LNL_F_TMPL = 128, LNL_F_CONT = 256, LNL_F_ROBUST = 512, LNL_F_TEXS = 1024 };
constexpr unsigned LNL_KINDS = 32;      // kinds 0 .. 31: every set of the five bits
constexpr unsigned lnl_plan_kind(const LnlPlan &P) {
    return (P.form == LNL_WEIGHTED || P.form == LNL_BASELINE ? LNL_K_WEIGHTED : 0u) | (P.form == LNL_BASELINE ? LNL_K_BASELINE : 0u) |
           (P.filled ? LNL_K_FILL : 0u) | (P.layered ? LNL_K_LAYER : 0u) | (P.calibrated ? LNL_K_CALIB : 0u);
}
// NCOMP of a plan's instance for a runner of `ncomp` components: 1..3, the component loop unrolled; 0, the general form
constexpr int lnl_plan_ncomp(const LnlPlan &P, int ncomp) {
    return P.filled || P.layered || P.calibrated || ncomp < 1 || ncomp > 3 ? 0 : ncomp;
}
// the form of a set of kind != 0: what its weighted and baseline bits say
constexpr LnlForm lnl_kind_form(unsigned kind) {
    return (kind & LNL_K_BASELINE) ? LNL_BASELINE : (kind & LNL_K_WEIGHTED) ? LNL_WEIGHTED : LNL_PLAIN;
}
// The rule: whether the engine has the likelihood kernel of `form` for (mode 0 table / 2 fast, spectra out, wide,
// NCOMP 0..3, kind).  The engine instantiates exactly the instances this admits (nfa_engine.hip: lnl_kernel_inst) and
// tests/test_launch_plan.py holds every plan of plan_lnl to it; DESIGN 4.2 counts them.
constexpr bool lnl_instance_exists(LnlForm form, int mode, bool write_spec, bool wide, int ncomp_inst, unsigned kind) {
    if ((mode != 0 && mode != 2) || ncomp_inst < 0 || ncomp_inst > 3 || kind >= LNL_KINDS) return false;
    if (kind == 0)               // a plain set: the table mode with spectra out is w8's (plan_lnl sends no such launch to the plain
                                 // form), every other instance plain; the queue for the table mode's narrow sets
        return (form == LNL_PLAIN && !(mode == 0 && write_spec)) || (form == LNL_W8 && mode == 0 && write_spec) ||
               (form == LNL_QUEUE && mode == 0 && !wide);
    if ((kind & LNL_K_BASELINE) && !(kind & LNL_K_WEIGHTED)) return false;       // a baseline is profiled out of weighted sums
    if ((kind & LNL_K_CALIB) && !(kind & LNL_K_BASELINE)) return false;          // the gain is marginalised in the baseline form
    if ((kind & (LNL_K_FILL | LNL_K_LAYER | LNL_K_CALIB)) && ncomp_inst != 0) return false;     // the general component form only
    return form == lnl_kind_form(kind);         // never w8 or the queue: the units give the same bits whatever the form
}
// An entry of the engine's table of instances and its index: bits 0-1 NCOMP, 2 wide, 3 spectra out, 4 fast mode, 5-9 kind
struct LnlInst { int mode; bool write_spec, wide; int ncomp; unsigned kind; };
constexpr int LNL_INSTANCES = 32 * LNL_KINDS;
constexpr int lnl_inst_index(const LnlInst &i) {
    return (int)(i.kind << 5) | (i.mode == 0 ? 0 : 16) | (i.write_spec ? 8 : 0) | (i.wide ? 4 : 0) | i.ncomp;
}
constexpr LnlInst lnl_inst_at(int i) { return {(i & 16) ? 2 : 0, (i & 8) != 0, (i & 4) != 0, i & 3, (unsigned)i >> 5}; }
constexpr bool lnl_inst_round_trip() {
    for (int i = 0; i < LNL_INSTANCES; ++i) {
        const LnlInst a = lnl_inst_at(i);
        if (lnl_inst_index(a) != i || a.ncomp > 3 || a.kind >= LNL_KINDS || (a.mode != 0 && a.mode != 2)) return false;
    }
    return true;
}
static_assert(lnl_inst_round_trip(), "lnl_inst_at must invert lnl_inst_index over the whole table");

// The side family, lnl_kernel_side<MODE, WRITE_SPEC, WIDE, FILL, LAYER, SIDE> (nfa_device.h): the kernels of a set with
// correlated channel noise, a channel response, nuisance templates, a continuum background or a robust likelihood, and of a
// set of the excitation-grid model (an excitation temperature per (component, spectrum): LNL_F_TEXS).  They stand
// beside the table of kinds, in the general component form only (NCOMP 0), 32 instances per side; a side says which flags
// of lnl_body its kernels switch on and, through them, under which plan form they run.
enum LnlSide { LNL_SIDE_NONE, LNL_SIDE_CORR, LNL_SIDE_RESP, LNL_SIDE_TMPL, LNL_SIDE_CONT, LNL_SIDE_ROBUST, LNL_SIDE_TEXS };
constexpr int LNL_SIDES = 6, LNL_SIDE_INSTANCES = 32;
constexpr unsigned lnl_side_flags(LnlSide side) {
    return side == LNL_SIDE_CORR ? LNL_K_WEIGHTED | LNL_F_CORR : side == LNL_SIDE_RESP ? LNL_K_WEIGHTED | LNL_F_CORR | LNL_F_RESP :
           side == LNL_SIDE_TMPL ? LNL_K_WEIGHTED | LNL_K_BASELINE | LNL_F_TMPL :
           side == LNL_SIDE_CONT ? LNL_K_WEIGHTED | LNL_K_BASELINE | LNL_F_CONT : side == LNL_SIDE_ROBUST ? LNL_K_WEIGHTED | LNL_F_ROBUST :
           side == LNL_SIDE_TEXS ? LNL_K_WEIGHTED | LNL_K_BASELINE | LNL_F_TEXS : 0u;
}
// the plan form a side's kernels run under: the weighted form's waves, LDS and workgroups, or the baseline form's
constexpr LnlForm lnl_side_form(LnlSide side) { return lnl_kind_form(lnl_side_flags(side)); }
// the side of a set: an excitation per spectrum first (the model's own side: such a set takes none of the others), then a
// robust likelihood, a continuum, templates, a response (which is correlated too), a correlation
constexpr LnlSide lnl_side_of(bool corr, bool resp, bool tmpl, bool cont, bool rob, bool texs = false) {
    return texs ? LNL_SIDE_TEXS : rob ? LNL_SIDE_ROBUST : cont ? LNL_SIDE_CONT : tmpl ? LNL_SIDE_TMPL : resp ? LNL_SIDE_RESP : corr ? LNL_SIDE_CORR : LNL_SIDE_NONE;
}
// An instance of a side and its index: bit 0 wide, 1 spectra out, 2 fast mode, 3 filled, 4 layered
struct LnlSideInst { int mode; bool write_spec, wide, filled, layered; };
constexpr int lnl_side_index(int mode, bool write_spec, bool wide, bool filled, bool layered) {
    return (layered ? 16 : 0) | (filled ? 8 : 0) | (mode == 0 ? 0 : 4) | (write_spec ? 2 : 0) | (wide ? 1 : 0);
}
constexpr LnlSideInst lnl_side_at(int i) { return {(i & 4) ? 2 : 0, (i & 2) != 0, (i & 1) != 0, (i & 8) != 0, (i & 16) != 0}; }
constexpr bool lnl_side_round_trip() {
    for (int i = 0; i < LNL_SIDE_INSTANCES; ++i) {
        const LnlSideInst a = lnl_side_at(i);
        if (lnl_side_index(a.mode, a.write_spec, a.wide, a.filled, a.layered) != i || (a.mode != 0 && a.mode != 2)) return false;
    }
    return true;
}
static_assert(lnl_side_round_trip(), "lnl_side_at must invert lnl_side_index over a side's 32 instances");
// Plans the likelihood launch of L.B items (the table of forms in DESIGN 4.2 is tested against this chain).
// templates: the set has nuisance templates (nfa_specset_set_templates): the baseline form's plan over nine
// sums per part, for lnl_kernel_side's templates side (beside the table: the plan names no instance of it).
// texs: the set is of the excitation-grid model: the baseline form whatever the set's options, for
// lnl_kernel_side's excitation side, whose item records are the larger ones (lnl_drec_doubles) -- in global memory, so the
// plan's LDS is the baseline form's, slot for slot.
inline LnlPlan plan_lnl(const LpShape &s, const LpKnobs &k, const LpLaunch &L, bool templates = false, bool texs = false) {
    LnlPlan P = {};
    const int64_t units = L.B * s.n_spec;
    if (units * 8 >= (1LL << 28)) { P.error = "batch too large for one launch"; return P; }
    const bool table = L.mode == 0;
    // table mode: more than 26 lines in a transition (N2H+ 2-1, 3-2): 64-bit line masks, a mask per component;
    // fast mode: more lines than any NH3 transition (or 2^22 channels): fp64 running sum of tau
    P.wide = lnl_wide(s);
    P.G = lnl_geom(s, k, L.B);
    P.G.ablate = k.ablate;
    P.filled = L.filled;
    P.layered = L.layered;
    P.calibrated = L.calibrated;
    int waves = lnl_waves(s, table, P.G.split);
    // A calibrated set keeps one more sum per part than a baseline set.  Where that sixth slot is what does not fit, the
    // workgroup takes one unit (waves = split): less LDS than any baseline workgroup of two units and more; and should a
    // baseline workgroup of ONE unit have fitted where this one does not, half the split, down to one wave per unit, which
    // keeps no sums in LDS at all.  So whatever plans with a baseline plans calibrated.  The bits depend on neither.
    // (G.split is lowered after lnl_geom filled G: of LnlGeom only `split` itself depends on the split -- nhf_max,
    // wave_doubles, inv_nspec and inv_nhf are the runner's -- and waves, LDS and workgroups are computed below from the
    // lowered value.  The GPU suite launches the waves = split case; the halving is held to its arithmetic without a GPU only.)
    // A set with templates keeps nine sums per part, and plans by the same rule.
    const int slots_most = lnl_part_slots(true, L.calibrated, templates);
    if ((L.calibrated || templates) && lnl_units_lds(s, table, P.G.split, waves, slots_most) > LDS_PER_CU) {
        waves = P.G.split;
        while (P.G.split > 1 && lnl_units_lds(s, table, P.G.split, waves, slots_most) > LDS_PER_CU) waves = P.G.split /= 2;
    }
    const int split = P.G.split;
    P.waves = waves;
    const int upw = waves / split;                               // units per workgroup
    // What the queue form asks of the launch's size: units of eight rows and more (short units -- config 1's 256 channels
    // are four rows -- finish before the draw has paid: 348 M evaluations/s one unit per wave against 335 M through the
    // queue), and two units and more per wave of the workgroups that are resident at once.
    bool long_units = true;
    for (int i = 0; i < s.n_spec; ++i) if (s.size[i] < 512) long_units = false;
    const int wg_per_cu = table_wg_per_cu(s, waves);
    const bool fills_twice = units >= 2 * ((int64_t)k.n_cu * wg_per_cu) * waves;
    // The form: the first line that applies.
    P.form = LNL_PLAIN;
    if (L.calibrated || templates || texs) P.form = LNL_BASELINE;      // a calibration uncertainty, templates, an excitation per spectrum: the baseline form (whatever the order)
    else if (L.baseline) P.form = LNL_BASELINE;      // every mode, wide, spectra out; such a set is weighted too
    else if (L.weighted) P.form = LNL_WEIGHTED;      // every mode, wide, spectra out: no queue or w8 form of its own (the
                                                     // units give the same bits whatever the form, so none is instantiated)
    else if (L.filled || L.layered) P.form = LNL_PLAIN;   // a filling factor, layered transfer: baseline, weighted or plain,
                                                     // never the queue or w8 form
    else if (table && !P.wide && split == 1          // the queue kernel is table mode, narrow, one wave per unit ...
             && k.lnl_queue != 0                     // ... unless switched off (option lnl_queue) ...
             && long_units && fills_twice            // ... pays for launches like these only ...
             && L.has_queue)                         // ... and needs the lane's counters (reserve_lane)
        P.form = LNL_QUEUE;
    else if (table && L.write_spec) P.form = LNL_W8; // table mode with spectra out asks for 66 registers left alone
    const bool queue = P.form == LNL_QUEUE;
    // LDS: [table mode: the product tables][per unit of the workgroup: the line table; split > 1: the parts' sums
    // (a baseline: and those of the moments of the unit; calibrated: and that of sum w p^2)][queue: the workgroup's queue word and count]
    const int n_shared = table ? SM_TABLE_DOUBLES : 0;
    P.lds = lnl_units_lds(s, table, split, waves, lnl_part_slots(P.form == LNL_BASELINE, L.calibrated, templates)) + (queue ? 16 : 0);
    if (table) P.lds = std::max(P.lds, sizeof(double) * (size_t)(n_shared + SM_TABLE_TAIL));
    if (P.lds > LDS_PER_CU) { P.error = "ncomp too large for the LDS line table"; return P; }
    if (!table && s.lnl_cap > 0 && waves * s.lnl_cap < LP_WAVES_PER_CU)      // residency cap: see Engine::lnl_cap
        P.lds = std::max(P.lds, (LDS_PER_CU / s.lnl_cap) & ~(size_t)15);
    // the queue form: as many workgroups as are resident at once (option lnl_queue_wg: A/B); else one per upw units
    P.blocks = queue ? (int64_t)k.n_cu * (k.lnl_queue_wg > 0 ? k.lnl_queue_wg : wg_per_cu) : (units + upw - 1) / upw;
    if (P.blocks > 0x7fffffffLL) P.error = "batch too large for one launch";
    return P;
}

// LDS of the set-up stage (setup_body) in bytes: `n_exp` doubles of exponential tables, then per group of items theta
// and the partition records, the prior program and `stage_doubles` of its tables
inline size_t setup_lds_layout(const LpShape &s, int n_exp, int nsub, int stage_doubles) {
    const size_t work = (size_t)nsub * ((size_t)64 * s.ndim + (size_t)SETUP_TI * s.ncomp * QREC) + s.prog_bytes / sizeof(double) + 1
                        + (size_t)stage_doubles;
    return sizeof(double) * ((size_t)n_exp + work);
}
// Whether a launch stages the prior tables the priors were created with (`want` doubles: setup_want).  Whether they
// fit is only known here: in the table mode, 500-point irdc tables (10 of them staged) and 8 or more components need more
// than 160 KiB.  Such a launch takes the copy of the program that reads the tables from global memory
// (nfa_priors::d_prog_global): the same values, so the same bits, as priors created under option prior_stage 0.
inline int setup_want(const LpShape &s, bool has_prior) { return has_prior && s.n_stage > 0 ? s.stage_doubles : 0; }
inline bool setup_fits(const LpShape &s, int n_exp, int nsub, int want) { return setup_lds_layout(s, n_exp, nsub, want) <= LDS_PER_CU; }

enum SetupInst { SETUP_TABLE_2, SETUP_TABLE, SETUP_FAST, SETUP_POLY };   // setup_kernel<0, false, 2>, <0, false>, <1, true>, <1, false>
// items per group, groups and threads per workgroup, workgroups, LDS; staged: the launch takes d_prog, not d_prog_global
struct SetupPlan { SetupInst inst; int ti, nsub, threads; unsigned blocks; size_t lds; bool staged; const char *error; };
inline SetupPlan plan_setup(const LpShape &s, const LpKnobs &k, const LpLaunch &L) {
    SetupPlan P = {};
    P.ti = lp_setup_ti(k);
    const bool tables = L.mode == 0 && s.model == NFA_MODEL_AMMONIA;     // FastExp's product tables too: the partition sums go through them
    const int n_exp = tables ? SM_TABLE_DOUBLES : NFA_EXP2_N;
    // Eight waves per workgroup where the partition sums go through FastExp's tables (52 KB of LDS per workgroup: two per
    // CU whatever their size; 88.4 -> 90.5 M evaluations/s on the metric shape); the polynomial's set-up (fast mode) is
    // faster with four (156.5 against 149.8 M): its workgroups are many per CU (scripts/gpu_setup_shape.sh).
    P.threads = k.setup_threads > 0 ? k.setup_threads : tables ? 2 * SETUP_THREADS : SETUP_THREADS;
    // ... and two such groups per workgroup behind one copy of the tables (115 KB of LDS for one group: two rounds of
    // workgroups for 32768 items; 133 KB for two: one round, profiles/r05/ab_table_linestep.txt).  Every batch of a group
    // must hold whole workgroups; a launch of ONE batch may have any size (the last workgroup's second group then has fewer
    // items, or none).  Small launches keep one group: they are latency, not rounds.  Two groups only with all staged that
    // the priors were created to stage.
    const bool whole = L.group_n <= 1 || (L.B % (2 * P.ti) == 0 && L.group_each % (2 * P.ti) == 0);
    const bool two = tables && k.setup_threads == 0 && k.setup_sub != 1 && P.ti == SETUP_TI && whole && L.B > (int64_t)P.ti * k.n_cu;
    const int want = setup_want(s, L.has_prior);
    bool fits = two && setup_fits(s, n_exp, 2, want);
    P.nsub = fits ? 2 : 1;
    if (P.nsub == 2) P.threads = 1024;
    else fits = setup_fits(s, n_exp, 1, want);
    P.staged = want > 0 && fits;
    P.blocks = (unsigned)((L.B + (int64_t)P.ti * P.nsub - 1) / ((int64_t)P.ti * P.nsub));
    P.lds = setup_lds_layout(s, n_exp, P.nsub, P.staged ? want : 0);
    if (P.lds > LDS_PER_CU) P.error = "too many parameters for the set-up kernel";
    P.inst = P.nsub == 2 ? SETUP_TABLE_2 : tables ? SETUP_TABLE : L.mode == 2 ? SETUP_FAST : SETUP_POLY;
    return P;
}

// The fused kernels, point_kernel (nfa_setup.h) and ring_serve_kernel (nfa_ring_serve.h): both run setup_body and
// lnl_body<MODE, false, false, NCOMP> (narrow, unweighted) on one item in one workgroup of POINT_WAVES waves.
// refusal: why they cannot serve the runner's points (null: they can), in the words nfa_ring_serve_device fails with
// (few_points_kernel takes the batch path instead); ring_error: that, or that the resident kernel's LDS does not fit.
// G: of a launch of one item; n_blocks: passes of the workgroup over the units; staged: d_prog, not d_prog_global;
// lds_point: more than LDS_PER_CU sends the points the batch path; ctl_double: the resident kernel's control words
struct FusedPlan { const char *refusal, *ring_error; LnlGeom G; int n_blocks, ctl_double; bool staged; size_t lds_point, lds_ring; };
// banded: an LTE set with several transitions inside a spectrum (lte_band_kernel runs between the stages of a batch);
// filled: one with a beam filling factor per component (lte_fill_kernel runs there, and only the batch kernels have the form);
// layered: a set whose components absorb those behind them (nfa_specset_set_layered: the batch kernels only, and the first
// refusal of all -- whatever else the set is, its points must not reach a kernel that sums)
// calibrated: a set with a calibration uncertainty per spectrum (nfa_specset_set_calibration: the batch kernels only)
// correlated: a set whose channel noise is correlated along the spectrum (nfa_specset_set_correlation: the batch kernels
// only -- such a set is weighted too, and the weighted sum alone would leave out the products of neighbouring channels)
// response: a set with a channel response (nfa_specset_set_response: the batch kernels only, and refused before everything
// else -- such a set is "correlated" to its kernels even over white noise, and the reason must be its own)
// templates: a set with nuisance templates (nfa_specset_set_templates: the batch kernels only -- such a set is weighted too,
// and the reason must be its own)
// continuum: a set with a continuum background (nfa_specset_set_continuum: the batch kernels only -- such a set is weighted and
// runs the baseline form, and the reason must be its own)
// robust: a set with a robust likelihood (nfa_specset_set_robust: the batch kernels only, and refused first of all -- such a
// set is weighted to its kernels, whose weighted sum would be no likelihood of it)
inline FusedPlan plan_fused(const LpShape &s, const LpKnobs &k, int mode, bool baseline, bool weighted, bool banded = false,
                            bool filled = false, bool layered = false, bool calibrated = false, bool correlated = false,
                            bool response = false, bool templates = false, bool continuum = false, bool robust = false,
                            bool texs = false) {
    FusedPlan P = {};
    P.G = lnl_geom(s, k, 1);
    // texs: a set of the excitation-grid model (nfa_specset_create_grid: the batch kernels only, and refused first of all --
    // the fused kernels read one excitation temperature per component from a record that has none)
    if (texs) P.refusal = "the resident kernel has no form for an excitation per spectrum: use nfa_ring_serve";
    else if (robust) P.refusal = "the resident kernel has no form for a robust likelihood: use nfa_ring_serve";
    else if (response) P.refusal = "the resident kernel has no form for a channel response: use nfa_ring_serve";
    else if (correlated) P.refusal = "the resident kernel has no form for correlated channel noise: use nfa_ring_serve";
    else if (calibrated) P.refusal = "the resident kernel has no form for a calibration uncertainty: use nfa_ring_serve";
    else if (layered) P.refusal = "the resident kernel has no form for layered transfer: use nfa_ring_serve";
    else if (continuum) P.refusal = "the resident kernel has no form for a continuum background: use nfa_ring_serve";
    else if (templates) P.refusal = "the resident kernel has no form for nuisance templates: use nfa_ring_serve";
    else if (s.ndim > NFA_POINT_MAXDIM || lnl_wide(s)) P.refusal = "this runner's points go through the batch kernels: use nfa_ring_serve";
    else if (filled) P.refusal = "the resident kernel has no form for a filling factor: use nfa_ring_serve";
    // (weighted sets, baseline sets among them: the fused kernels run the unweighted body, which would compute the unweighted sum.)
    else if (baseline) P.refusal = "the resident kernel has no form for a baseline: use nfa_ring_serve";
    else if (weighted) P.refusal = "the resident kernel has no form for a noise per channel: use nfa_ring_serve";
    else if (banded) P.refusal = "the resident kernel has no form for LTE bands: use nfa_ring_serve";
    else if (P.G.split > POINT_WAVES) P.refusal = "spectra too short for the point kernel's split";
    if ((P.ring_error = P.refusal)) return P;
    const int upw = POINT_WAVES / P.G.split;                     // units per pass of the workgroup
    P.n_blocks = (s.n_spec + upw - 1) / upw;
    // The kernels stage the exponential tables themselves (table mode: FastExp's product tables whatever the model), so
    // whether the prior tables are staged is asked of the set-up stage's own layout, behind the polynomial's table.
    const int want = setup_want(s, true);
    P.staged = want > 0 && setup_fits(s, NFA_EXP2_N, 1, want);
    const size_t tables = sizeof(double) * (mode == 0 ? SM_TABLE_DOUBLES : 0);                // the likelihood's
    const size_t setup = setup_lds_layout(s, mode == 0 ? SM_TABLE_DOUBLES : NFA_EXP2_N, 1, P.staged ? want : 0);
    const size_t units = sizeof(double) * (((size_t)P.G.wave_doubles + (P.G.split > 1 ? LNL_PARTS * 64 : 0)) * upw);   // line tables, split parts of a pass
    // point kernel: the set-up stage and the likelihood waves use the same LDS one after the other, behind the staged tables
    P.lds_point = std::max(setup, tables + units);
    // resident kernel: [exponential tables][theta, partition records][prior program + tables][line tables][control words]
    size_t lds = setup + units;
    if (mode == 0) lds = std::max(lds, tables + sizeof(double) * SM_TABLE_TAIL);
    lds = (lds + 15) & ~(size_t)15;
    P.ctl_double = (int)(lds / sizeof(double));
    P.lds_ring = lds + 16;
    if (P.lds_ring > LDS_PER_CU) P.ring_error = "too many parameters for the resident kernel";
    return P;
}
