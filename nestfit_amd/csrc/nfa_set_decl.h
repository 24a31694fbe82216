// nfa_set_decl.h -- how a spectra set is declared: the plain records the kernels read (LineRow, LteRec, BandRec, MixRec),
// everything a creator of include/nestfit_amd.h can be given (SetDecl), and the one function that turns a declaration into
// a refusal or into what the engine uploads (set_plan -> SetPlan).
//
// Standard C++17 without a HIP include, like nfa_launch_plan.h, nfa_set_rules.h and nfa_set_state.h: a host compiler builds
// this header alone, and tests/test_set_decl_cpu.py holds every refusal and every record to it without a GPU.  The engine's
// part is specset_build (nfa_engine.hip), which allocates, copies and forms what the plan names.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/nestfit_amd.h"   // NFA_MODEL_*, NFA_ERR_ARG
#include "n2hp_data.h"                   // the shipped tables (and nh3_data.h: NFA_MAX_HF_N, the constants)
#include "nfa_launch_plan.h"             // MAXSPEC
#include "nfa_grid_decl.h"               // the excitation-grid model's record and checks (GridRec, grid_fill)

// Transition indices of every model in one index space: 0..8 NH3 (1,1)..(9,9), 9..11 N2H+ 1-0, 2-1, 3-2, 12 the
// Gaussian model's single "line" (offset 0, weight 1, rest frequency from the spectrum), 13 a spectrum of the
// hyperfine model or of the LTE model, whose lines the caller supplies (nfa_specset_create_lines, _create_lte).
// SpecDev.trans holds index + 1.
// The index selects what belongs to a transition beyond its lines (c_nu and c_ea: ammonia only; the Gaussian
// model's line centre, nf_line); the lines themselves are per spectrum, in device memory (SpecDev.lines).
#define NFA_T_N2HP   NFA_N_LEVELS
#define NFA_T_GAUSS  (NFA_N_LEVELS + NFA_N2HP_LEVELS)
#define NFA_T_LINES  (NFA_T_GAUSS + 1)
#define NFA_T_ALL    (NFA_T_LINES + 1)

// The lines of one spectrum as the kernels read them (line_row_fill below; the shipped tables for ammonia,
// N2H+ and the Gaussian model, the caller's for the hyperfine model): hf_freq = (1 - voff / CKMS) * nu of every line
// (hyperfine.pyx:71), its weight, the number of lines, and the position of every line when the lines are ordered by
// their velocity offset (stable): in that order the lines whose windows touch a row of channels form ONE run of
// neighbours (fast mode's line table, lnl_body).
struct LineRow {
    double        hfreq[NFA_MAX_HF_N];
    double        tauw[NFA_MAX_HF_N];
    int           nhf;
    unsigned char rank[NFA_MAX_HF_N];
};

// What the LTE model (NFA_MODEL_LTE, nfa_specset_create_lte) needs beyond the lines, one record per spectra set in
// device memory: the upper level and the Einstein coefficient of every spectrum's transition, and the species'
// partition function as ln Q over ln T with the slope of every segment (slope[k]: entries k, k + 1).  Only the set-up
// stage's derive_lte_lane reads it (nfa_setup.h).
#define NFA_LTE_MAXQ 64
struct LteRec {
    double e_up[MAXSPEC], g_up[MAXSPEC], a_ul[MAXSPEC];      // K, statistical weight, 1/s
    int    n_q, pad;
    double ln_t[NFA_LTE_MAXQ], ln_q[NFA_LTE_MAXQ], slope[NFA_LTE_MAXQ];
};

// LTE bands (nfa_specset_create_lte_bands): a spectrum that covers several transitions g of the species, each
// with lines of its own.  One record per banded spectra set in device memory (null for every other set): the number of
// transitions of every spectrum and the transition of every line, and per (spectrum, transition), formed on the host in
// doubles against the spectrum's reference transition 0 (the one of the lowest lower-level energy, whose numbers
// SpecDev.rest and LteRec hold):  t0 = h nu_g / k,  de = (E_g - t0_g) - (E_0 - t0_0) >= 0,
// k = (g_g A_g / nu_g^3) / (g_0 A_0 / nu_0^3).  lte_band_kernel (nfa_setup.h) reads the numbers, lnl_body grp.
#define NFA_BAND_MAXT 8
struct BandRec {
    int           n_trans[MAXSPEC];
    unsigned char grp[MAXSPEC][NFA_MAX_HF_N];
    double        t0[MAXSPEC][NFA_BAND_MAXT], de[MAXSPEC][NFA_BAND_MAXT], k[MAXSPEC][NFA_BAND_MAXT];
};

// LTE mixes (nfa_specset_create_lte_mix): a set whose transitions belong to K = 2..4 species that share voff,
// tex and sigm, each with a column density (parameter 3 + k of a component for species k >= 1; species 0's stays
// parameter 2) and a partition table of its own.  One record per such set in device memory (null for every other set)
// beside a BandRec, which a mix set always owns: the species of every (spectrum, transition) in the band's order, and the
// partition tables of species 1..K-1 as LteRec holds species 0's (entry k - 1: species k).  Only lte_mix_kernel
// (nfa_setup.h) reads it.
#define NFA_LTE_MAXSP 4
struct MixRec {
    int           n_species, pad;
    unsigned char species[MAXSPEC][NFA_BAND_MAXT];
    int           n_q[NFA_LTE_MAXSP - 1], pad2;
    double        ln_t[NFA_LTE_MAXSP - 1][NFA_LTE_MAXQ], ln_q[NFA_LTE_MAXSP - 1][NFA_LTE_MAXQ], slope[NFA_LTE_MAXSP - 1][NFA_LTE_MAXQ];
};
// the kernels read these in device memory: layout and field order are theirs
static_assert(sizeof(LineRow) == 856 && sizeof(LteRec) == 1928 && sizeof(BandRec) == 3936 && sizeof(MixRec) == 4760,
              "the records' layout is the kernels'");

// Who is asking: the entry points of include/nestfit_amd.h in the order they were added, each with the arguments of the one
// before and more.  (nfa_specset_create is DECL_MODEL with the ammonia model; nfa_specset_create_lte_filled has the mix
// creator's arguments.)
enum SetCreator { DECL_MODEL, DECL_CHANNEL_NOISE, DECL_LINES, DECL_LTE, DECL_BANDS, DECL_MIX, DECL_FILLED };

// Everything a creator can be given, null where it has no such argument; in the order in which the creators grew, so that each
// fills a prefix (nfa_engine.hip)
struct SetDecl {
    SetCreator who = DECL_MODEL;
    const void *out = nullptr;                      // where the set goes: only whether it is null
    int model = NFA_MODEL_AMMONIA, n_spec = 0;
    const int64_t *sizes = nullptr;
    const double *const *xarr = nullptr;
    int64_t n_pix = 0;
    const double *data = nullptr, *noise = nullptr, *chan_noise = nullptr;
    const double  *rest_freqs = nullptr;            // per spectrum; from DECL_BANDS on per transition (trans_freqs)
    const int32_t *trans_ids = nullptr;             // DECL_MODEL, DECL_CHANNEL_NOISE
    const int32_t *n_lines = nullptr;               // the line tables, from DECL_LINES on: per spectrum (from DECL_BANDS on: per transition)
    const double  *voff = nullptr, *tau_wts = nullptr;
    const double  *e_up = nullptr, *g_up = nullptr, *a_ul = nullptr;      // from DECL_LTE on: per transition
    const int32_t *n_q = nullptr;                   // ... and the length of every species' partition table
    const double  *q_temp = nullptr, *q_val = nullptr;
    const int32_t *n_trans = nullptr;               // from DECL_BANDS on: transitions per spectrum
    int n_species = 1;                              // from DECL_MIX on
    const int32_t *species = nullptr;               // ... per transition
    // nfa_specset_create_grid: a DECL_LINES declaration with an excitation grid (`grid` says so: the pointers may be null)
    bool grid = false;
    int g_nt = 0, g_nn = 0, g_nc = 0;               // nodes of the three axes
    const double *g_tkin = nullptr, *g_lnden = nullptr, *g_lncd = nullptr;
    const double *g_tex = nullptr, *g_ltau = nullptr;     // [n_spec][nt * nn * nc]
};

// What kind of set a declaration makes.  Each kind owns the records of the one before: SET_LTE an LteRec, SET_BANDS a BandRec
// too, SET_MIX a MixRec too.  A mix declaration of one species is a SET_BANDS (or less), a bands declaration with a
// transition per spectrum a SET_LTE; a filled set is a SET_MIX whatever it holds, so that launch_band runs for it.
enum SetKind { SET_BUILTIN, SET_LINES, SET_LTE, SET_BANDS, SET_MIX };

struct SetPlan {
    SetKind kind = SET_BUILTIN;
    bool    filled = false;                         // a beam filling factor per component: the last parameter
    bool    chan_noise = false, masked = false;     // a noise per channel; with a masked channel somewhere
    // SpecDev's geometry
    int     model = 0, n_spec = 0, npar = 0;
    double  rest[MAXSPEC] = {};
    int     size[MAXSPEC] = {}, trans[MAXSPEC] = {}, off[MAXSPEC] = {}, row_off[MAXSPEC] = {};
    double  nu_min[MAXSPEC] = {}, nu_chan[MAXSPEC] = {}, r_chan[MAXSPEC] = {};
    int64_t chan_tot = 0, rows_tot = 0, n_pix = 0;
    int     nhf_max = 0, h_nhf[MAXSPEC] = {};       // lines of every spectrum
    LineRow lines[MAXSPEC];                         // zeroed by set_plan, padding included
    LteRec  lte;                                    // kind >= SET_LTE
    BandRec band;                                   // kind >= SET_BANDS
    MixRec  mix;                                    // kind == SET_MIX
    bool    grid = false;                           // the excitation-grid model: a SET_LINES set with ...
    GridRec grid_rec;                               // ... its axes (the tables' pointers are the engine's to fill)
    std::vector<double> sigma_ref;                  // chan_noise: the smallest finite sigma_c of every (pixel, spectrum)
};

inline int decl_refuse(std::string &why, const std::string &msg) { why = msg; return NFA_ERR_ARG; }

// The line row of one spectrum from a table of n lines: hf_freq of every line with one rounding per operation
// (hyperfine.pyx:71) and the rank of every line (stable).  A plain row (nu_step 0) has one rest frequency, nu[0], and ranks
// by descending velocity offset; a banded row (nu_step 1, nfa_specset_create_lte_bands) takes every line against the rest
// frequency of its own transition, nu[i], and ranks by ascending hf_freq -- for one transition the permutation the descending
// offsets give, but not the same order: rounding can tie hf_freq where the offsets differ.  The slots behind the last line
// hold hf_freq of a zero offset (against nu[0]), weight 0 and their own index.
inline void line_row_fill(LineRow &row, int n, const double *nu, int nu_step, const double *voff, const double *tauw) {
    row.nhf = n;
    for (int i = 0; i < NFA_MAX_HF_N; ++i) {
        volatile double q = (i < n ? voff[i] : 0.0) / NFA_CKMS;       // hyperfine.pyx:71, one rounding per operation
        volatile double f = 1.0 - q;
        row.hfreq[i] = f * nu[i < n ? i * nu_step : 0];
        row.tauw[i] = i < n ? tauw[i] : 0.0;
        row.rank[i] = (unsigned char)i;
    }
    std::vector<int> order(n);
    for (int i = 0; i < n; ++i) order[i] = i;
    if (nu_step) std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return row.hfreq[a] < row.hfreq[b]; });
    else std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return voff[a] > voff[b]; });
    for (int k = 0; k < n; ++k) row.rank[order[k]] = (unsigned char)k;
}
// The shipped table of global transition index tg (NFA_T_*): the line count, the rest frequency, offsets and weights
inline int builtin_table(int tg, double *nu, const double **voff, const double **tauw) {
    static const double gauss_voff[NFA_MAX_HF_N] = {0.0}, gauss_w[NFA_MAX_HF_N] = {1.0};
    if (tg < NFA_T_N2HP) { *nu = nfa_nu[tg]; *voff = nfa_voff[tg]; *tauw = nfa_tau_wts[tg]; return nfa_nhf[tg]; }
    if (tg < NFA_T_GAUSS) {
        const int t = tg - NFA_T_N2HP;
        *nu = nfa_n2hp_nu[t]; *voff = nfa_n2hp_voff[t]; *tauw = nfa_n2hp_tau_wts[t]; return nfa_n2hp_nhf[t];
    }
    *nu = 0.0; *voff = gauss_voff; *tauw = gauss_w; return 1;
}

// the checks of nfa_specset_create_lines on one table of n lines (`at`: where, for the message)
inline int check_one_table(std::string &why, int n, double nu, const double *voff, const double *tau_wts, const std::string &at) {
    if (n < 1 || n > NFA_MAX_HF_N) return decl_refuse(why, "a line table must have 1..50 lines" + at);
    if (!(std::isfinite(nu) && nu > 0)) return decl_refuse(why, "a rest frequency must be finite and positive" + at);
    bool any = false;
    for (int i = 0; i < n; ++i) {
        const double v = voff[i], w = tau_wts[i];
        if (!(std::isfinite(v) && std::fabs(v) < NFA_CKMS)) return decl_refuse(why, "a velocity offset must be finite and below the speed of light" + at);
        if (!(std::isfinite(w) && w >= 0)) return decl_refuse(why, "a line weight must be finite and not negative" + at);
        any = any || w > 0;
    }
    if (!any) return decl_refuse(why, "the weights of a line table are all zero" + at);
    return NFA_OK;
}
// the checks of nfa_specset_create_lte on one transition beyond its line table's
inline int check_one_transition(std::string &why, double e_up, double g_up, double a_ul, int n, const double *tau_wts, const std::string &at) {
    if (!(std::isfinite(e_up) && e_up >= 0)) return decl_refuse(why, "an upper-level energy must be finite and not negative (K)" + at);
    if (!(std::isfinite(g_up) && g_up > 0)) return decl_refuse(why, "an upper-level weight must be finite and positive" + at);
    if (!(std::isfinite(a_ul) && a_ul > 0)) return decl_refuse(why, "an Einstein coefficient must be finite and positive (1/s)" + at);
    double sum = 0.0;
    for (int i = 0; i < n; ++i) sum += tau_wts[i];
    if (!(std::fabs(sum - 1.0) <= 1e-6)) return decl_refuse(why, "the weights of a transition must sum to 1 within 1e-6" + at);
    return NFA_OK;
}
// ... and on a partition function, which it leaves as ln Q over ln T with the segments' slopes (`at`: which species')
inline int lte_partition_fill(std::string &why, int &n_out, double *ln_t, double *ln_q, double *slope, int n_q,
                              const double *q_temp, const double *q_val, const std::string &at) {
    static const char ascending[] = "the temperatures of a partition table must be finite, positive and strictly ascending";
    if (n_q < 2 || n_q > NFA_LTE_MAXQ) return decl_refuse(why, "a partition table must have 2..64 entries" + at);
    for (int k = 0; k < n_q; ++k) {
        if (!(std::isfinite(q_temp[k]) && q_temp[k] > 0 && (k == 0 || q_temp[k] > q_temp[k - 1]))) return decl_refuse(why, ascending + at);
        if (!(std::isfinite(q_val[k]) && q_val[k] > 0)) return decl_refuse(why, "a partition function value must be finite and positive" + at);
        ln_t[k] = log(q_temp[k]);
        ln_q[k] = log(q_val[k]);
    }
    for (int k = 0; k + 1 < n_q; ++k) {
        if (!(ln_t[k + 1] > ln_t[k])) return decl_refuse(why, ascending + at);
        slope[k] = (ln_q[k + 1] - ln_q[k]) / (ln_t[k + 1] - ln_t[k]);
    }
    n_out = n_q;
    return NFA_OK;
}

// The line tables of the spectra, one after the other, as the rows are formed from them: the caller's own arrays, or a banded
// set's in the engine's order (band_layout) with the rest frequency of every line's transition beside them
struct SetTables {
    const int32_t *n_lines = nullptr;
    const double  *rest = nullptr, *voff = nullptr, *tau_wts = nullptr, *line_nu = nullptr;     // line_nu: banded rows only
    std::vector<int32_t> s_lines;
    std::vector<double>  s_rest, l_voff, l_wts, l_nu;
};
// What the bands creator and the mix creator share: the checks per transition, and the spectra's transitions in the engine's
// order with their lines one after the other -- the band record, the reference transitions' numbers for the set-up stage
// (p.lte, T.s_rest) and the flattened line arrays.  `species` (null: one species): the species of every transition, which goes
// into the mix record in the band's order; the same transition twice is then refused within a species.
inline int band_layout(std::string &why, const SetDecl &d, const int32_t *species, SetPlan &p, SetTables &T) {
    const int32_t *n_lines = d.n_lines;
    const double *trans_freqs = d.rest_freqs, *voff = d.voff, *tau_wts = d.tau_wts, *e_up = d.e_up, *g_up = d.g_up, *a_ul = d.a_ul;
    // the spectra's transitions in the engine's order -- ascending lower-level energy, then rest frequency, then the caller's
    // order -- and their lines one after the other: what the caller's order of a spectrum's transitions cannot change
    T.s_lines.assign((size_t)d.n_spec, 0);
    T.s_rest.assign((size_t)d.n_spec, 0.0);
    int64_t tr0 = 0, l0 = 0;
    for (int s = 0; s < d.n_spec; ++s) {
        const int nt = d.n_trans[s];
        std::vector<int64_t> first((size_t)nt);                     // the first line of every transition
        std::vector<double> e_low((size_t)nt);
        int total = 0;
        for (int j = 0; j < nt; ++j) {
            const int64_t t = tr0 + j;
            const std::string at = " (spectrum " + std::to_string(s) + ", transition " + std::to_string(j) + ")";
            first[j] = l0;
            if (n_lines[t] >= 1 && n_lines[t] <= NFA_MAX_HF_N && total + n_lines[t] > NFA_MAX_HF_N)
                return decl_refuse(why, "the transitions of a spectrum must have at most 50 lines together (spectrum " + std::to_string(s) + ")");
            int rc = check_one_table(why, n_lines[t], trans_freqs[t], voff + l0, tau_wts + l0, at); if (rc) return rc;
            rc = check_one_transition(why, e_up[t], g_up[t], a_ul[t], n_lines[t], tau_wts + l0, at); if (rc) return rc;
            for (int i = 0; i < j; ++i)
                if ((!species || species[tr0 + i] == species[t]) && trans_freqs[tr0 + i] == trans_freqs[t] && e_up[tr0 + i] == e_up[t] &&
                    g_up[tr0 + i] == g_up[t] && a_ul[tr0 + i] == a_ul[t])
                    return decl_refuse(why, (species ? "a spectrum lists the same transition of a species twice" : "a spectrum lists the same transition twice") + at);
            e_low[j] = e_up[t] - NFA_H * trans_freqs[t] / NFA_KB;
            total += n_lines[t];
            l0 += n_lines[t];
        }
        std::vector<int> order((size_t)nt);
        for (int j = 0; j < nt; ++j) order[j] = j;
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
            return e_low[a] != e_low[b] ? e_low[a] < e_low[b] : trans_freqs[tr0 + a] < trans_freqs[tr0 + b];
        });
        const int64_t r = tr0 + order[0];                           // the reference transition
        const double ref_t0 = NFA_H * trans_freqs[r] / NFA_KB;
        const double ref_k = g_up[r] * a_ul[r] / (trans_freqs[r] * trans_freqs[r] * trans_freqs[r]);
        T.s_rest[s] = trans_freqs[r];
        p.lte.e_up[s] = e_up[r]; p.lte.g_up[s] = g_up[r]; p.lte.a_ul[s] = a_ul[r];
        p.band.n_trans[s] = nt;
        int line = 0;
        for (int g = 0; g < nt; ++g) {
            const int64_t t = tr0 + order[g];
            const double nu = trans_freqs[t], tg = NFA_H * nu / NFA_KB;
            p.band.t0[s][g] = tg;
            p.band.de[s][g] = (e_up[t] - tg) - (e_up[r] - ref_t0);
            p.band.k[s][g] = (g_up[t] * a_ul[t] / (nu * nu * nu)) / ref_k;
            if (species) p.mix.species[s][g] = (unsigned char)species[t];
            for (int i = 0; i < n_lines[t]; ++i, ++line) {
                p.band.grp[s][line] = (unsigned char)g;
                T.l_voff.push_back(voff[first[order[g]] + i]);
                T.l_wts.push_back(tau_wts[first[order[g]] + i]);
                T.l_nu.push_back(nu);
            }
        }
        T.s_lines[s] = line;
        tr0 += nt;
    }
    T.n_lines = T.s_lines.data(); T.rest = T.s_rest.data(); T.voff = T.l_voff.data(); T.tau_wts = T.l_wts.data(); T.line_nu = T.l_nu.data();
    return NFA_OK;
}

// A declaration into a plan, or a refusal: NFA_ERR_ARG with its message in `why`.  No device call.
//
// THE ORDER OF THE CHECKS IS FROZEN.  An input that is wrong in two ways gets the message of the check that comes first
// below, and callers have seen those messages since the creators were separate functions calling each other: the model
// creator asks about the model before n_spec, the channel-noise creator after the noise values; a noise per channel is
// checked before trans_ids and the axis, a scalar noise after them; the mix creator's species before anything per
// transition; a bands declaration with a transition per spectrum checks every table and then every transition, like the LTE
// creator, a banded one transition by transition.  tests/test_set_decl_cpu.py lists one doubly wrong input per adjacent pair.
inline int set_plan(const SetDecl &d, SetPlan &p, std::string &why) {
    p = SetPlan{};
    memset(p.lines, 0, sizeof p.lines); memset(&p.lte, 0, sizeof p.lte); memset(&p.band, 0, sizeof p.band); memset(&p.mix, 0, sizeof p.mix);
    memset(&p.grid_rec, 0, sizeof p.grid_rec);
    const SetCreator who = d.who;
    const bool chan = who == DECL_CHANNEL_NOISE || (who >= DECL_LINES && d.chan_noise);
    const auto n_spec_range = [&] { return d.n_spec < 1 || d.n_spec > MAXSPEC ? decl_refuse(why, "n_spec must be in 1..16") : NFA_OK; };
    const auto n_pix_range = [&] { return d.n_pix < 1 ? decl_refuse(why, "n_pix must be >= 1") : NFA_OK; };
    const auto size_range = [&](int s) { return d.sizes[s] < 2 || d.sizes[s] > (1 << 24) ? decl_refuse(why, "spectrum size out of range") : NFA_OK; };
    int rc;

    // 1. the arguments every route of the creator reads
    if (!d.out || !d.sizes || !d.xarr || !d.data || (who == DECL_MODEL && !d.noise) || (who == DECL_CHANNEL_NOISE && !d.chan_noise) ||
        (who >= DECL_LINES && (!d.n_lines || !d.rest_freqs || !d.voff || !d.tau_wts)) || (who >= DECL_BANDS && !d.n_trans) ||
        (who >= DECL_MIX && (!d.species || !d.n_q)) || (d.grid && (!d.g_tkin || !d.g_lnden || !d.g_lncd || !d.g_tex || !d.g_ltau)))
        return decl_refuse(why, "null argument");
    if (who >= DECL_MIX && (d.n_species < 1 || d.n_species > NFA_LTE_MAXSP)) return decl_refuse(why, "n_species must be in 1..4");
    if (who >= DECL_LINES && (d.noise != nullptr) == (d.chan_noise != nullptr))
        return decl_refuse(why, "exactly one of noise and chan_noise must be given");
    if (who != DECL_MODEL) { rc = n_spec_range(); if (rc) return rc; }
    // 2. what kind of set: the transitions per spectrum and the species say whether it has a band and a mix record
    p.kind = who == DECL_LINES ? SET_LINES : who == DECL_LTE ? SET_LTE : who >= DECL_BANDS ? SET_BANDS : SET_BUILTIN;
    if (who >= DECL_BANDS) {
        bool banded = false;
        for (int s = 0; s < d.n_spec; ++s) {
            if (d.n_trans[s] < 1 || d.n_trans[s] > NFA_BAND_MAXT)
                return decl_refuse(why, "a spectrum must have 1..8 transitions (spectrum " + std::to_string(s) + ")");
            banded = banded || d.n_trans[s] > 1;
        }
        if (who >= DECL_MIX) {
            int64_t n_all = 0;
            for (int s = 0; s < d.n_spec; ++s) n_all += d.n_trans[s];
            bool seen[NFA_LTE_MAXSP] = {};
            for (int64_t t = 0; t < n_all; ++t) {
                if (d.species[t] < 0 || d.species[t] >= d.n_species)
                    return decl_refuse(why, "a species index must be in 0..n_species - 1 (transition " + std::to_string(t) + ")");
                seen[d.species[t]] = true;
            }
            for (int k = 0; k < d.n_species; ++k)
                if (!seen[k])
                    return decl_refuse(why, "a species without a transition in any spectrum: its column density would be unconstrained (species "
                                            + std::to_string(k) + ")");
        }
        p.filled = who == DECL_FILLED;
        // one species: the bands creator's set; a transition per spectrum: nfa_specset_create_lte's -- bit for bit
        p.kind = p.filled || d.n_species > 1 ? SET_MIX : banded ? SET_BANDS : SET_LTE;
    }
    // 3. the line tables and what belongs to the transitions
    SetTables T;
    T.n_lines = d.n_lines; T.rest = d.rest_freqs; T.voff = d.voff; T.tau_wts = d.tau_wts;
    if (p.kind == SET_LINES || p.kind == SET_LTE) {             // every table, then every transition
        int64_t l0 = 0;
        for (int s = 0; s < d.n_spec; ++s) {
            rc = check_one_table(why, d.n_lines[s], d.rest_freqs[s], d.voff + l0, d.tau_wts + l0, " (spectrum " + std::to_string(s) + ")");
            if (rc) return rc;
            l0 += d.n_lines[s];
        }
    }
    if (d.grid && who == DECL_LINES) {                          // the grid creator: every transition's weights, then the grid
        rc = grid_check_weights(why, d.n_spec, d.n_lines, d.tau_wts); if (rc) return rc;
        rc = grid_fill(why, p.grid_rec, GridDecl{d.g_nt, d.g_nn, d.g_nc, d.g_tkin, d.g_lnden, d.g_lncd, d.g_tex, d.g_ltau}, d.n_spec);
        if (rc) return rc;
        p.grid = true;
    }
    if (p.kind >= SET_LTE && (!d.e_up || !d.g_up || !d.a_ul || !d.q_temp || !d.q_val)) return decl_refuse(why, "null argument");
    if (p.kind == SET_LTE) {
        int64_t l0 = 0;
        for (int s = 0; s < d.n_spec; ++s) {
            rc = check_one_transition(why, d.e_up[s], d.g_up[s], d.a_ul[s], d.n_lines[s], d.tau_wts + l0, " (spectrum " + std::to_string(s) + ")");
            if (rc) return rc;
            l0 += d.n_lines[s];
            p.lte.e_up[s] = d.e_up[s]; p.lte.g_up[s] = d.g_up[s]; p.lte.a_ul[s] = d.a_ul[s];
        }
    }
    if (p.kind >= SET_BANDS) {                                  // transition by transition
        if (p.kind == SET_MIX) p.mix.n_species = d.n_species;
        rc = band_layout(why, d, p.kind == SET_MIX ? d.species : nullptr, p, T); if (rc) return rc;
    }
    // the partition tables: species 0's where the set-up stage reads it, the others' in the mix record
    const int n_tables = p.kind == SET_MIX ? d.n_species : p.kind >= SET_LTE ? 1 : 0;
    int64_t q0 = 0;
    for (int k = 0; k < n_tables; ++k) {
        const std::string at = p.kind == SET_MIX ? " (species " + std::to_string(k) + ")" : "";
        rc = k == 0 ? lte_partition_fill(why, p.lte.n_q, p.lte.ln_t, p.lte.ln_q, p.lte.slope, d.n_q[0], d.q_temp, d.q_val, at)
                    : lte_partition_fill(why, p.mix.n_q[k - 1], p.mix.ln_t[k - 1], p.mix.ln_q[k - 1], p.mix.slope[k - 1], d.n_q[k],
                                         d.q_temp + q0, d.q_val + q0, at);
        if (rc) return rc;
        q0 += d.n_q[k];
    }
    // 4. a noise per channel: sigma_ref of every (pixel, spectrum) -- the smallest finite sigma_c -- after its checks
    if (chan) {
        rc = n_pix_range(); if (rc) return rc;
        int64_t tot = 0;
        for (int s = 0; s < d.n_spec; ++s) { rc = size_range(s); if (rc) return rc; tot += d.sizes[s]; }
        p.sigma_ref.resize((size_t)(d.n_pix * d.n_spec));
        for (int64_t pix = 0; pix < d.n_pix; ++pix) {
            int64_t c = pix * tot;
            for (int s = 0; s < d.n_spec; ++s) {
                double lo = INFINITY;
                for (int64_t j = 0; j < d.sizes[s]; ++j, ++c) {
                    const double sg = d.chan_noise[c];
                    if (!(sg > 0)) return decl_refuse(why, "channel noise must be > 0 (NaN is not allowed; inf masks the channel)");
                    if (sg == INFINITY) { p.masked = true; continue; }
                    if (std::isnan(d.data[c])) return decl_refuse(why, "NaN data in a channel that is not masked (channel noise inf masks it)");
                    lo = std::min(lo, sg);
                }
                if (lo == INFINITY) return decl_refuse(why, "every channel of a spectrum is masked (channel noise inf)");
                p.sigma_ref[(size_t)(pix * d.n_spec + s)] = lo;
            }
        }
        p.chan_noise = true;
    }
    // 5. the model of the two creators that take one
    p.model = who >= DECL_LTE ? NFA_MODEL_LTE : who == DECL_LINES ? (p.grid ? NFA_MODEL_GRID : NFA_MODEL_HYPERFINE) : d.model;
    if (who < DECL_LINES) {
        if (d.model == NFA_MODEL_HYPERFINE) return decl_refuse(why, "the hyperfine model takes its line tables through nfa_specset_create_lines");
        if (d.model == NFA_MODEL_LTE)
            return decl_refuse(why, "unknown model to this creator: the LTE model takes its line tables and partition function "
                                    "through nfa_specset_create_lte");
        if (d.model == NFA_MODEL_GRID) return decl_refuse(why, grid_model_refusal());
        if (d.model < NFA_MODEL_AMMONIA || d.model > NFA_MODEL_LTE) return decl_refuse(why, "unknown model");
        if (d.model != NFA_MODEL_GAUSSIAN && !d.trans_ids) return decl_refuse(why, "null argument");
        if (d.model == NFA_MODEL_GAUSSIAN && d.n_spec != 1) return decl_refuse(why, "the Gaussian model takes one spectrum");     // gaussian.pyx:57-89
        rc = n_spec_range(); if (rc) return rc;
    }
    if (!chan) { rc = n_pix_range(); if (rc) return rc; }
    // 6. the geometry, spectrum by spectrum: its size, its transition, its axis
    const int model = p.model;
    const bool tabled = p.kind >= SET_LINES;                                    // the caller's line tables
    p.n_spec = d.n_spec;
    p.n_pix = d.n_pix;
    p.npar = model == NFA_MODEL_DIAZENYLIUM || tabled ? NFA_N2HP_PARAMS
           : model == NFA_MODEL_GAUSSIAN ? NFA_GAUSS_PARAMS : NFA_N_PARAMS;
    if (p.kind == SET_MIX) p.npar = 3 + d.n_species + (p.filled ? 1 : 0);
    if (p.grid) p.npar = NFA_GRID_PARAMS;
    int64_t tot = 0, rows = 0, line0 = 0;
    for (int s = 0; s < d.n_spec; ++s) {
        rc = size_range(s); if (rc) return rc;
        int tglob;                                                      // index into the device tables
        if (model == NFA_MODEL_AMMONIA) {
            if (d.trans_ids[s] < 1 || d.trans_ids[s] > NFA_N_LEVELS) return decl_refuse(why, "trans_id must be in 1..9");         // ammonia.pyx:268
            tglob = d.trans_ids[s] - 1;
            p.rest[s] = nfa_nu[tglob];
        } else if (model == NFA_MODEL_DIAZENYLIUM) {
            if (d.trans_ids[s] < 1 || d.trans_ids[s] > NFA_N2HP_LEVELS) return decl_refuse(why, "trans_id must be in 1..3");      // diazenylium.pyx:128
            tglob = NFA_T_N2HP + d.trans_ids[s] - 1;
            p.rest[s] = nfa_n2hp_nu[d.trans_ids[s] - 1];
        } else if (model == NFA_MODEL_GAUSSIAN) {
            tglob = NFA_T_GAUSS;
            p.rest[s] = d.rest_freqs ? d.rest_freqs[s] : 0.0;           // core.pyx:510
        } else {
            tglob = NFA_T_LINES;
            p.rest[s] = T.rest[s];
        }
        {
            double nu; const double *voff, *tauw;
            int n;
            if (tabled) {
                n = T.n_lines[s]; voff = T.voff + line0; tauw = T.tau_wts + line0;
                if (T.line_nu) line_row_fill(p.lines[s], n, T.line_nu + line0, 1, voff, tauw);
                else line_row_fill(p.lines[s], n, T.rest + s, 0, voff, tauw);
                line0 += n;
            } else {
                n = builtin_table(tglob, &nu, &voff, &tauw);
                line_row_fill(p.lines[s], n, &nu, 0, voff, tauw);
            }
            p.h_nhf[s] = n;
            p.nhf_max = std::max(p.nhf_max, n);
        }
        const double nu_chan = d.xarr[s][1] - d.xarr[s][0];
        if (!(nu_chan > 0)) return decl_refuse(why, "frequency axis must be ascending");   // core.pyx:503-504
        p.size[s] = (int)d.sizes[s];
        p.trans[s] = tglob + 1;
        p.off[s] = (int)tot;
        p.row_off[s] = (int)rows;
        p.nu_min[s] = d.xarr[s][0];
        p.nu_chan[s] = nu_chan;
        {   // the reciprocal nf_line divides with (0: a width that is not an ordinary number, or whose mantissa is all ones)
            uint64_t bits; memcpy(&bits, &nu_chan, sizeof bits);
            const bool ordinary = std::isnormal(nu_chan) && nu_chan > 1e-100 && nu_chan < 1e100;
            p.r_chan[s] = ordinary && (bits & 0xfffffffffffffull) != 0xfffffffffffffull ? 1.0 / nu_chan : 0.0;
        }
        tot += d.sizes[s];
        rows += (d.sizes[s] + 63) / 64;
    }
    p.chan_tot = tot;
    p.rows_tot = rows;
    // 7. a scalar noise
    for (int64_t i = 0; !chan && i < d.n_pix * d.n_spec; ++i)
        if (!(d.noise[i] > 0)) return decl_refuse(why, "noise must be > 0");                // core.pyx:502
    return NFA_OK;
}
