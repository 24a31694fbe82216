// nfa_set_state.h -- what a spectra set's likelihood options ask of the device: the record of the options (SetOptions), the
// buffers and pointers that record stands for (set_layout) and the forming work a change of it needs (set_stages_*).
//
// Standard C++17 without a HIP include, like nfa_launch_plan.h and nfa_set_rules.h: a host compiler builds this header
// alone, and tests/test_set_state_cpu.py holds it to the setters it replaced without a GPU.  The engine's part is
// specset_realise (nfa_engine.hip), which allocates, forms and frees what this header names.
#pragma once
#include <cstring>

#include "nfa_launch_plan.h"   // MAXSPEC
#include "nfa_set_rules.h"     // SET_HAS_*

#define SET_RESP_NT 5          // NFA_RESP_NT (nfa_device.h)

// What the caller asked for, per spectrum; an option that is off holds zeros (bl_order: -1).  The two large arrays, the
// templates' values and the continuum, stay with the engine: here they are presence (and the templates' counts).
struct SetOptions {
    int    bl_order = -1;                       // nfa_specset_set_baseline
    bool   cal_on = false, nunc_on = false, corr_on = false, resp_on = false, tmpl_on = false, cont_on = false, rob_on = false;
    double cal[MAXSPEC] = {};                   // nfa_specset_set_calibration: fractional 1-sigma values
    double nunc[MAXSPEC] = {};                  // nfa_specset_set_noise_uncertainty: fractional 1-sigma values
    double rho[MAXSPEC][2] = {};                // nfa_specset_set_correlation: (rho_1, rho_2)
    double resp[MAXSPEC][SET_RESP_NT] = {};     // nfa_specset_set_response: the taps
    int    ntmpl[MAXSPEC] = {};                 // nfa_specset_set_templates: templates per spectrum
    double rob[MAXSPEC] = {};                   // nfa_specset_set_robust: degrees of freedom
    bool   grid_on = false;                     // no request: a set of the excitation-grid model, from its creation on (its
                                                // kernels are the baseline form's: set_layout)
};
// bit for bit: -0.0 is another request than 0.0 (a getter hands it back)
#define SET_SAME(f) (memcmp(a.f, b.f, sizeof a.f) == 0)
inline bool set_options_equal(const SetOptions &a, const SetOptions &b) {
    return a.bl_order == b.bl_order && a.cal_on == b.cal_on && a.nunc_on == b.nunc_on && a.corr_on == b.corr_on &&
           a.resp_on == b.resp_on && a.tmpl_on == b.tmpl_on && a.cont_on == b.cont_on && a.rob_on == b.rob_on && a.grid_on == b.grid_on &&
           SET_SAME(cal) && SET_SAME(nunc) && SET_SAME(rho) && SET_SAME(resp) && SET_SAME(ntmpl) && SET_SAME(rob);
}
// the word set_refusal (nfa_set_rules.h) asks about.  ("correlated" is the coefficients of the correlated kernels, which a
// response over white noise has too.)
inline unsigned set_has(const SetOptions &o, bool masked) {
    return (masked ? SET_HAS_MASK : 0u) | (o.bl_order >= 0 ? SET_HAS_BASELINE : 0u) | (o.cal_on ? SET_HAS_CALIB : 0u) |
           (o.nunc_on ? SET_HAS_NMARG : 0u) | (o.corr_on || o.resp_on ? SET_HAS_CORR : 0u) | (o.resp_on ? SET_HAS_RESP : 0u) |
           (o.tmpl_on ? SET_HAS_TMPL : 0u) | (o.cont_on ? SET_HAS_CONT : 0u) | (o.rob_on ? SET_HAS_ROBUST : 0u);
}

// The device buffers that depend on the options, one bit each
enum : unsigned {
    SB_W = 1u << 0, SB_WDATA = 1u << 1,                 // the set's own weights u^2 and w d: a noise per channel, or ones
    SB_BL = 1u << 2, SB_TP = 1u << 3,                   // baseline and template records
    SB_CAL2 = 1u << 4, SB_NMARG = 1u << 5,
    SB_Q0 = 1u << 6, SB_Q1 = 1u << 7, SB_Q2 = 1u << 8, SB_CORR = 1u << 9,     // Q's bands and the entries of R^-1
    SB_RESP = 1u << 10, SB_TMPL = 1u << 11, SB_CONT = 1u << 12,
    SB_RG = 1u << 13, SB_RGD = 1u << 14, SB_ROB = 1u << 15,                   // robust g, g d and the records
    SB_N = 16
};
// what SpecDev.chan_w and .wdata point at
enum SetChanW { CHAN_W_NONE,      // nothing: a scalar noise and no option that runs a weighted form
                CHAN_W_OWN,       // d_w, d_wdata = w d
                CHAN_W_Q,         // d_q0, d_wdata = Q d
                CHAN_W_ROBUST };  // d_rg, d_rgd; d_w and d_wdata (if any) keep the set's own beneath

// option -> buffers, chan_w source, records:
//   baseline order >= 0   ones*, bl                         own
//   calibration           ones*, bl (zeroed without a baseline), cal2      own
//   continuum             ones*, bl (likewise), cont        own
//   (excitation-grid set) ones*, bl (likewise)              own
//   templates             ones*, tmpl, tp                   own
//   noise uncertainty     nmarg                             (as it was)
//   correlation           ones*, q0 q1 q2 corr              Q
//   response              ones*, q0 q1 q2 corr (white without a correlation), resp     Q
//   robust                rg rgd rob                        robust g
// (* on a scalar noise: d_w == 1 and d_wdata, one flag and one allocation)
struct SetLayout {
    unsigned bufs = 0;            // SB_*: the buffers that exist
    bool     ones = false;        // a scalar noise whose d_w is all ones
    SetChanW chan_w = CHAN_W_NONE;
    bool has(unsigned b) const { return (bufs & b) != 0; }
};
inline SetLayout set_layout(const SetOptions &o, bool has_channel_noise) {
    SetLayout L;
    const bool q = o.corr_on || o.resp_on;
    // a calibration or a continuum alone, a set of the excitation-grid model: the zeroed record
    const bool bl = o.bl_order >= 0 || o.cal_on || o.cont_on || o.grid_on;
    L.ones = !has_channel_noise && (bl || o.tmpl_on || q);
    if (has_channel_noise || L.ones) L.bufs |= SB_W | SB_WDATA;
    if (bl) L.bufs |= SB_BL;
    if (o.tmpl_on) L.bufs |= SB_TMPL | SB_TP;
    if (o.cal_on) L.bufs |= SB_CAL2;
    if (o.nunc_on) L.bufs |= SB_NMARG;
    if (q) L.bufs |= SB_Q0 | SB_Q1 | SB_Q2 | SB_CORR;
    if (o.resp_on) L.bufs |= SB_RESP;
    if (o.cont_on) L.bufs |= SB_CONT;
    if (o.rob_on) L.bufs |= SB_RG | SB_RGD | SB_ROB;
    L.chan_w = o.rob_on ? CHAN_W_ROBUST : q ? CHAN_W_Q : L.has(SB_W) ? CHAN_W_OWN : CHAN_W_NONE;
    return L;
}

// The work of specset_realise's second phase, in the order it runs.  The forming stages are the engine's launches; next to
// each, what it reads -- a stage runs when something it reads changed or when a buffer it writes is new.
enum : unsigned {
    UP_CAL2 = 1u << 0, UP_CORR = 1u << 1, UP_RESP = 1u << 2, UP_TMPL = 1u << 3, UP_CONT = 1u << 4,     // host -> device copies
    ST_ONES = 1u << 8,            // d_w = 1                                     reads: nothing
    ST_CHAN_WEIGHT = 1u << 9,     // launch_chan_weight: d_wdata = w d            reads: d_w, data
    ST_CORR = 1u << 10,           // launch_corr_setup: d_wdata = Q d             reads: d_w, data, Q's bands
    ST_FORM_Q = 1u << 11,         // ... with form_q: Q's bands too               reads: d_w, R^-1 of the correlation
    ST_ROWSQ = 1u << 12,          // launch_rowsq under the set's own weights or Q (a robust set: its base)   reads: data, d_wdata
    ST_ROB = 1u << 13,            // rob_setup_kernel over that base              reads: d_w, data, totsq, the degrees of freedom
    ST_BL = 1u << 14,             // launch_bl_setup: m(d)                        reads: d_wdata
    ST_BL_BASIS = 1u << 15,       // ... with form_basis                          reads: d_w, the baseline order
    ST_TP = 1u << 16,             // launch_tmpl_setup: m(d)                      reads: d_wdata, the templates
    ST_TP_BASIS = 1u << 17,       // ... with form_basis                          reads: d_w, the templates, the baseline order
    ST_NMARG = 1u << 18,          // nmarg_setup_kernel                           reads: d_w, the noise uncertainties
    ST_FORM_W = 1u << 19,         // beside ST_CHAN_WEIGHT, with form_w: w too, from the caller's sigmas, which go into d_w first
    ST_DATA = ST_CHAN_WEIGHT | ST_CORR | ST_ROWSQ | ST_ROB | ST_BL | ST_TP     // the stages that read the data (or what they make of them)
};
// (Through the buffers a stage reads the options that decide their presence or content: the set's own weights of a scalar noise
// exist for a baseline, a calibration, a continuum, templates, a correlation or a response; d_wdata holds Q d under a correlation
// or a response and w d otherwise; totsq is a robust set's k C.  tests/test_set_state_cpu.py holds the selection to that table.)

// every copy and every stage a layout has: a set formed from nothing
inline unsigned set_stages_all(const SetLayout &L) {
    unsigned st = 0;
    if (L.has(SB_CAL2)) st |= UP_CAL2;
    if (L.has(SB_CORR)) st |= UP_CORR | ST_CORR | ST_FORM_Q;
    if (L.has(SB_RESP)) st |= UP_RESP;
    if (L.has(SB_TMPL)) st |= UP_TMPL;
    if (L.has(SB_CONT)) st |= UP_CONT;
    if (L.ones) st |= ST_ONES;
    if (L.has(SB_W) && L.chan_w != CHAN_W_Q) st |= ST_CHAN_WEIGHT;
    st |= ST_ROWSQ;
    if (L.has(SB_ROB)) st |= ST_ROB;
    if (L.has(SB_BL)) st |= ST_BL | ST_BL_BASIS;
    if (L.has(SB_TP)) st |= ST_TP | ST_TP_BASIS;
    if (L.has(SB_NMARG)) st |= ST_NMARG;
    return st;
}
// a set's creation (specset_build): the empty record's stages, and a noise per channel becomes the weights
// (a set of the excitation-grid model over a scalar noise is created with the ones: no sigmas to form weights from)
inline unsigned set_stages_create(const SetLayout &L) { return set_stages_all(L) | (L.has(SB_W) && !L.ones ? ST_FORM_W : 0u); }
// new data in a pixel (nfa_specset_set_data): Q, the mask, the baseline basis and the templates' stay
inline unsigned set_stages_data(const SetLayout &L) { return set_stages_all(L) & ST_DATA; }
// from options a (layout la) to options b (layout lb), which differ in one option; tmpl_changed, cont_changed: the values of
// the large arrays differ.  Replacing a value with one of the same kind reuses the buffers and runs what reads the value.
inline unsigned set_stages_change(const SetOptions &a, const SetLayout &la, const SetOptions &b, const SetLayout &lb,
                                  bool tmpl_changed, bool cont_changed) {
    const unsigned born = lb.bufs & ~la.bufs;
    const bool coef = (born & SB_CORR) || !SET_SAME(rho);                     // R^-1 as Q's bands hold it
    const bool rob = (born & SB_ROB) || !SET_SAME(rob);
    const bool order = a.bl_order != b.bl_order;
    unsigned st = 0;
    if ((born & SB_CAL2) || !SET_SAME(cal)) st |= UP_CAL2;
    if (coef) st |= UP_CORR | ST_CORR | ST_FORM_Q;
    if ((born & SB_RESP) || !SET_SAME(resp)) st |= UP_RESP;
    if ((born & SB_TMPL) || tmpl_changed) st |= UP_TMPL;
    if ((born & SB_CONT) || cont_changed) st |= UP_CONT;
    if (lb.ones && !la.ones) st |= ST_ONES;
    if ((born & SB_WDATA) || la.chan_w == CHAN_W_Q) st |= ST_CHAN_WEIGHT;     // w d is new, or was Q d
    // (w == 1 gives the sums of the scalar noise to the bit: ones that come or go leave rowsq and totsq as they are)
    if (coef || (la.chan_w == CHAN_W_Q) != (lb.chan_w == CHAN_W_Q) || rob || la.has(SB_ROB) != lb.has(SB_ROB)) st |= ST_ROWSQ;
    if (rob) st |= ST_ROB;
    if ((born & SB_BL) || order) st |= ST_BL | ST_BL_BASIS;
    if ((born & SB_TP) || tmpl_changed || order) st |= ST_TP | ST_TP_BASIS;
    if ((born & SB_NMARG) || !SET_SAME(nunc)) st |= ST_NMARG;
    return st & set_stages_all(lb);
}
#undef SET_SAME
