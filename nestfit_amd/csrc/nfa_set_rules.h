// nfa_set_rules.h -- which likelihoods a spectra set takes beside the ones it has: every "a set with X takes no Y" of the
// nfa_specset_set_* calls, in one table.
//
// Standard C++17 without a HIP include, like nfa_launch_plan.h: a host compiler builds this header alone, and
// tests/test_set_rules_cpu.py holds every cell of it to the sentences without a GPU.  The checks of a setter's own values
// (ranges, "4 channels and more", the Gaussian model) stay with the setter.
#pragma once

// what a set has (the engine forms the word from the set: specset_has)
enum : unsigned {
    SET_HAS_MASK = 1,        // a noise per channel with a masked channel somewhere
    SET_HAS_BASELINE = 2, SET_HAS_CALIB = 4, SET_HAS_NMARG = 8,
    SET_HAS_CORR = 16,       // the correlated kernels' coefficients: a set with a response has them too, over white noise
    SET_HAS_RESP = 32, SET_HAS_TMPL = 64, SET_HAS_CONT = 128, SET_HAS_ROBUST = 256,
    SET_HAS_ALL = 511
};
// what a setter asks it to take
enum SetTakes { SET_TAKES_BASELINE, SET_TAKES_CALIB, SET_TAKES_NMARG, SET_TAKES_CORR, SET_TAKES_RESP, SET_TAKES_TMPL, SET_TAKES_CONT,
                SET_TAKES_ROBUST, SET_TAKES_N };

// The rows of a request in the order they are asked: a set with several of the features is refused for the first.
// An incompatible pair is refused from either setter.  Three groups say it in the same words whichever comes second: a
// calibration uncertainty and a noise uncertainty (a calibrated set's part is chi^2 plus sigma^2 log1p(s^2 A / sigma^2), DESIGN
// 4.12: no chi^2 whose noise scale integrates out in closed form); a continuum background (one kernel family, the
// baseline form's) with a calibration, a correlation, a response or templates; and a robust likelihood (no linear
// nuisance has a closed form under Student-t noise and a part is no chi^2), whose two sentences mirror each other.
struct SetRule { int takes; unsigned has; const char *why; };
static const SetRule SET_RULES[] = {
    {SET_TAKES_BASELINE, SET_HAS_RESP, "a set with a channel response takes no baseline"},
    {SET_TAKES_BASELINE, SET_HAS_CORR, "a set with correlated channel noise takes no baseline"},
    {SET_TAKES_BASELINE, SET_HAS_ROBUST, "a set with a robust likelihood takes no baseline"},
    {SET_TAKES_CALIB, SET_HAS_RESP, "a set with a channel response takes no calibration uncertainty"},
    {SET_TAKES_CALIB, SET_HAS_CORR, "a set with correlated channel noise takes no calibration uncertainty"},
    {SET_TAKES_CALIB, SET_HAS_TMPL, "a set with nuisance templates takes no calibration uncertainty"},
    {SET_TAKES_CALIB, SET_HAS_NMARG, "a set takes a calibration uncertainty or a noise uncertainty, not both: a calibrated set's part is no chi^2"},
    {SET_TAKES_CALIB, SET_HAS_CONT, "a set with a calibration uncertainty takes no continuum background"},
    {SET_TAKES_CALIB, SET_HAS_ROBUST, "a set with a robust likelihood takes no calibration uncertainty"},
    {SET_TAKES_NMARG, SET_HAS_CALIB, "a set takes a calibration uncertainty or a noise uncertainty, not both: a calibrated set's part is no chi^2"},
    {SET_TAKES_NMARG, SET_HAS_ROBUST, "a set with a robust likelihood takes no noise uncertainty"},
    {SET_TAKES_CORR, SET_HAS_MASK, "a set with a masked channel takes no noise correlation"},
    {SET_TAKES_CORR, SET_HAS_BASELINE, "a set with a baseline takes no noise correlation"},
    {SET_TAKES_CORR, SET_HAS_CALIB, "a set with a calibration uncertainty takes no noise correlation"},
    {SET_TAKES_CORR, SET_HAS_TMPL, "a set with nuisance templates takes no noise correlation"},
    {SET_TAKES_CORR, SET_HAS_CONT, "a set with correlated channel noise takes no continuum background"},
    {SET_TAKES_CORR, SET_HAS_ROBUST, "a set with a robust likelihood takes no noise correlation"},
    {SET_TAKES_RESP, SET_HAS_MASK, "a set with a masked channel takes no channel response"},
    {SET_TAKES_RESP, SET_HAS_BASELINE, "a set with a baseline takes no channel response"},
    {SET_TAKES_RESP, SET_HAS_CALIB, "a set with a calibration uncertainty takes no channel response"},
    {SET_TAKES_RESP, SET_HAS_TMPL, "a set with nuisance templates takes no channel response"},
    {SET_TAKES_RESP, SET_HAS_CONT, "a set with a channel response takes no continuum background"},
    {SET_TAKES_RESP, SET_HAS_ROBUST, "a set with a robust likelihood takes no channel response"},
    {SET_TAKES_TMPL, SET_HAS_RESP, "a set with a channel response takes no nuisance templates"},
    {SET_TAKES_TMPL, SET_HAS_CORR, "a set with correlated channel noise takes no nuisance templates"},
    {SET_TAKES_TMPL, SET_HAS_CALIB, "a set with a calibration uncertainty takes no nuisance templates"},
    {SET_TAKES_TMPL, SET_HAS_CONT, "a set with nuisance templates takes no continuum background"},
    {SET_TAKES_TMPL, SET_HAS_ROBUST, "a set with a robust likelihood takes no nuisance templates"},
    {SET_TAKES_CONT, SET_HAS_RESP, "a set with a channel response takes no continuum background"},
    {SET_TAKES_CONT, SET_HAS_CORR, "a set with correlated channel noise takes no continuum background"},
    {SET_TAKES_CONT, SET_HAS_CALIB, "a set with a calibration uncertainty takes no continuum background"},
    {SET_TAKES_CONT, SET_HAS_TMPL, "a set with nuisance templates takes no continuum background"},
    {SET_TAKES_CONT, SET_HAS_ROBUST, "a set with a robust likelihood takes no continuum background"},
    {SET_TAKES_ROBUST, SET_HAS_BASELINE, "a set with a baseline takes no robust likelihood"},
    {SET_TAKES_ROBUST, SET_HAS_TMPL, "a set with nuisance templates takes no robust likelihood"},
    {SET_TAKES_ROBUST, SET_HAS_CALIB, "a set with a calibration uncertainty takes no robust likelihood"},
    {SET_TAKES_ROBUST, SET_HAS_RESP, "a set with a channel response takes no robust likelihood"},
    {SET_TAKES_ROBUST, SET_HAS_CORR, "a set with correlated channel noise takes no robust likelihood"},
    {SET_TAKES_ROBUST, SET_HAS_NMARG, "a set with a noise uncertainty takes no robust likelihood"},
    {SET_TAKES_ROBUST, SET_HAS_CONT, "a set with a continuum background takes no robust likelihood"},
};
// why a set that has `has` does not take `takes` (null: it does)
inline const char *set_refusal(unsigned has, int takes) {
    for (const SetRule &r : SET_RULES)
        if (r.takes == takes && (has & r.has)) return r.why;
    return nullptr;
}
