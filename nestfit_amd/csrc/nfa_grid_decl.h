// nfa_grid_decl.h -- the excitation-grid model's part of a set's declaration (NFA_MODEL_GRID, nfa_specset_create_grid, DESIGN
// 4.23): the record the derive kernel reads (GridRec) and the checks of the creator's grid arguments (grid_fill), which
// set_plan (nfa_set_decl.h) calls behind the line tables' checks.
//
// Standard C++17 without a HIP include, like nfa_set_decl.h: a host compiler builds it alone, and tests/test_grid_cpu.py holds
// every refusal to it without a GPU.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/nestfit_amd.h"   // NFA_GRID_MAXN, NFA_GRID_MAXCELLS, NFA_ERR_ARG

// One record per set of the model in device memory (null for every other set): the three axes shared by the spectra --
// kinetic temperature, log10 of the H2 density, log10 of the column density per unit line width -- with their node counts,
// and the two tables of every spectrum over them, [n_spec][nt][nn][nc] doubles each in device memory of their own (up to
// 8.4 MB each: they live in L2, not in LDS): the excitation temperature and log10 of the peak optical depth.  Only
// grid_derive_kernel reads it (nfa_setup.h).
struct GridRec {
    int           nt, nn, nc, pad;
    double        tkin[NFA_GRID_MAXN], lnden[NFA_GRID_MAXN], lncd[NFA_GRID_MAXN];
    const double *tex, *ltau;
};
static_assert(sizeof(GridRec) == 1568, "the record's layout is the kernel's");

// the grid arguments of the creator: the node counts, the axes, the tables [n_spec][nt * nn * nc]
struct GridDecl {
    int nt, nn, nc;
    const double *tkin, *lnden, *lncd, *tex, *ltau;
};

inline int grid_refuse(std::string &why, const std::string &msg) { why = msg; return NFA_ERR_ARG; }

// what the other creators say to the model
inline const char *grid_model_refusal() {
    return "unknown model to this creator: the excitation-grid model takes its line tables and its grid through nfa_specset_create_grid";
}

// a transition's weights sum to 1 (nfa_specset_create_lte's check and words): the tables hold the depth summed over the lines
inline int grid_check_weights(std::string &why, int n_spec, const int32_t *n_lines, const double *tau_wts) {
    int64_t l0 = 0;
    for (int s = 0; s < n_spec; ++s) {
        double sum = 0.0;
        for (int i = 0; i < n_lines[s]; ++i) sum += tau_wts[l0 + i];
        if (!(std::fabs(sum - 1.0) <= 1e-6))
            return grid_refuse(why, "the weights of a transition must sum to 1 within 1e-6 (spectrum " + std::to_string(s) + ")");
        l0 += n_lines[s];
    }
    return 0;
}

// The checks on the grid, which they leave as the record's axes (the tables stay the caller's arrays until the engine
// uploads them).  In order: the node counts, their product, the axes, every tex, every ltau.
inline int grid_fill(std::string &why, GridRec &g, const GridDecl &d, int n_spec) {
    const struct { const char *name; int n; const double *a; double *to; } axes[3] = {
        {"tkin", d.nt, d.tkin, g.tkin}, {"lnden", d.nn, d.lnden, g.lnden}, {"lncd", d.nc, d.lncd, g.lncd}};
    for (const auto &ax : axes)
        if (ax.n < 1 || ax.n > NFA_GRID_MAXN)
            return grid_refuse(why, std::string("an axis of an excitation grid must have 1..64 nodes (") + ax.name + ")");
    const int64_t cells = (int64_t)d.nt * d.nn * d.nc;
    if (cells > NFA_GRID_MAXCELLS) return grid_refuse(why, "an excitation grid must have at most 65536 nodes (nt * nn * nc)");
    for (const auto &ax : axes)
        for (int i = 0; i < ax.n; ++i) {
            if (!(std::isfinite(ax.a[i]) && (i == 0 || ax.a[i] > ax.a[i - 1])))
                return grid_refuse(why, std::string("an axis of an excitation grid must be finite and strictly ascending (") + ax.name + ")");
            ax.to[i] = ax.a[i];
        }
    const auto at = [&](int64_t i) { return " (spectrum " + std::to_string(i / cells) + ", node " + std::to_string(i % cells) + ")"; };
    for (int64_t i = 0; i < cells * n_spec; ++i)
        if (!(std::isfinite(d.tex[i]) && d.tex[i] > 0))
            return grid_refuse(why, "an excitation temperature of a grid must be finite and positive: cut the grid where the "
                                    "populations invert or the solver did not converge" + at(i));
    for (int64_t i = 0; i < cells * n_spec; ++i)
        if (!std::isfinite(d.ltau[i])) return grid_refuse(why, "a log10 optical depth of a grid must be finite: cut the grid where it is not" + at(i));
    g.nt = d.nt; g.nn = d.nn; g.nc = d.nc;
    return 0;
}
