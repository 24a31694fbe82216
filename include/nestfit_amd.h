/* nestfit_amd.h -- C ABI of the MI355X-native NH3 log-likelihood engine.
 *
 * Drop-in boundary for the hot path of autocorr/nestfit v0.2: everything that
 * runs inside `AmmoniaRunner.c_loglikelihood` (prior transform -> model spectra
 * -> chi^2), batched over live points and map pixels on one gfx950 device.
 * Plain pointers and sizes only; no torch / numpy types.  All functions return
 * 0 on success and a non-zero code on failure (text via nfa_last_error());
 * the one exception is nfa_loglike_callback, which has MultiNest's `LogLike`
 * signature and therefore no error channel (it writes NaN into *lnew).
 *
 * Each entry point names the reference interface it replaces (file:line in
 * /root/reference).  INTEGRATION.md shows the ctypes / Cython stubs a
 * maintainer of the reference would add to bind them.
 */
#ifndef NESTFIT_AMD_H
#define NESTFIT_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NFA_OK            0
#define NFA_ERR_ARG       1   /* invalid argument (reference: assert / ValueError) */
#define NFA_ERR_DEVICE    2   /* HIP runtime error, or no gfx950 device            */
#define NFA_ERR_STATE     3   /* call order / missing table                        */

typedef struct nfa_specset nfa_specset;  /* device-resident spectra of 1..n_pix pixels */
typedef struct nfa_priors  nfa_priors;   /* device-resident prior program              */
typedef struct nfa_runner  nfa_runner;   /* (specset, priors, ncomp, cold, lte) bundle */

/* ---- process / device ---------------------------------------------------- */
const char *nfa_last_error(void);
int nfa_version(void);
int nfa_device_count(int *count);
int nfa_set_device(int device);              /* one process per GPU: call first */
int nfa_device_synchronize(void);
int nfa_device_name(char *buf, int buflen);
/* the 16-byte UUID of the engine's device as 32 hex digits (two ranks that report the same one share a GPU) */
int nfa_device_uuid(char *buf, int buflen);

/* Numerical mode of the FastExp replacement (process default, 2 unless set; a runner can pin
 * its own with nfa_runner_set_exp_mode):
 *   0 = "table": the reference's three-table product held in LDS
 *       (nestfit/core/fastexp.c:234-283), bit-identical table indices;
 *   (1, an fp64 polynomial form of the same exponential, was a likelihood mode until round 3:
 *       slower than the table mode and less faithful, it is refused now);
 *   2 = "fast" : window / table indices and the float-narrowed FastExp argument
 *       in fp64 exactly as above, exponentials in fp32 with split exponents;
 *       <= 1e-6 relative on brightness temperature (the metric's tolerance). */
int nfa_set_exp_mode(int mode);
int nfa_get_exp_mode(void);
/* Engine tuning knobs for A/B measurements (key, value):
 *   "wpb"           waves per workgroup of the likelihood kernel (1..16, default 1), and
 *   "wpb_table"     the same in table mode (0 = chosen per spectra set, the default): both are
 *                   taken over by runners created afterwards;
 *   "lnl_split"     waves that share one (item, spectrum) unit of the likelihood kernel: 1, 2, 4, or 0 = chosen per
 *                   launch (the default: 4 for single points and small batches, 1 for batches that fill the
 *                   GPU's wave slots).  More, shorter waves balance a small launch better at a few per cent more
 *                   instructions.  The chi^2 of a unit is always the sum of four interleaved row parts (rows h,
 *                   h + 4, ...) taken in order, whoever computed them, so log-likelihoods are bitwise independent
 *                   of this option and of the batch an evaluation travels in;
 *   "lnl_queue"     1 (default) / 0: table mode, launches of two and more (item, spectrum) units per wave slot of the
 *                   device (the coalesced steps of nfa_runner_loglike_batch_dev; spectra of 512 channels and more) run as
 *                   resident workgroups whose waves draw their units from a queue, or every wave owns one unit.
 *                   Bitwise the same results; "lnl_queue_wg" 1 / 2 (0 = as many as fit): workgroups per CU of such a
 *                   launch (A/B knob);
 *   "lnl_cap"       workgroups of the likelihood kernel resident per CU at most (fast and poly mode,
 *                   0 = no cap, the default; 1..8): A/B knob, see DESIGN.md;
 *   "streams"       number of HIP streams ("lanes", 1..8) that runners created afterwards spread consecutive
 *                   nfa_runner_loglike_batch_dev calls over; 0 (default) = six streams of which a batch of
 *                   about one wavefront per wave slot of the GPU uses all six and any other batch four;
 *   "sampler_parts" groups of pixels the device sampler pipelines over the lanes (1..4, default 3);
 *   "coalesce"      1..8 (default 8; 4 until round 5): nfa_runner_loglike_batch_dev calls of one shape (same number of rows, a
 *                   multiple of 64; pixels given or not) that follow each other are held and launched together,
 *                   at most this many (1 = every call its own launches).  Results are bitwise the same; anything
 *                   that looks at them or changes the way launches are made (nfa_runner_synchronize,
 *                   nfa_device_synchronize, the host-pointer calls, a mode change, nfa_set_option, the sampler) launches what is
 *                   held first.  Read at every call;
 *   "prior_stage"   1 / 0: the set-up kernel stages the prior tables in LDS (default) or reads them from global
 *                   memory; taken over by priors created afterwards (A/B knob: no measurable difference in the
 *                   pipelined rates, the staged form is 5 us shorter when the stage runs alone);
 *   "setup_ti", "setup_threads"  items (8..64, default 64) and threads (256 .. 512 in steps of 64; default 256, 512 in the table mode) per workgroup of
 *                   the set-up kernel: A/B knobs, see DESIGN.md;
 *   "setup_sub"     1: one group of 64 items per set-up workgroup in the table mode; 0 (default): two groups behind one
 *                   copy of the tables where every batch of the launch is a multiple of 128 rows;
 *   "setup_overlap" 1 (default) / 0: the set-up stage runs a resolved prior's velocities (placement, centre and
 *                   separation) beside the partition sums and the derived records where the prior program allows it,
 *                   or every phase after the other; the same bits either way (A/B knob, read when a launch is made);
 *   "point"         1 / 0: single points and small batches (nfa_runner_loglike_batch with B <= 128,
 *                   nfa_loglike_callback) go through the one-launch point kernel (default: one workgroup per
 *                   point, the result written to a mapped host buffer) or through the batch kernels;
 *   "graph"         1 / 0: with "point" 0, replay single-point calls as one captured hipGraph or not (default:
 *                   on, off when the rocprofiler tool library is attached: capture crashed under it);
 *   "sampler_parts"       1..4 (default 3): groups of pixels the device sampler pipelines over the stream lanes;
 *   "sampler_ellipsoids"  1: one bounding ellipsoid per pixel whatever the dimension; 0 (default): up to four where at
 *                   most six dimensions are sampled (per sampler: nfa_sampler_set_ellipsoids);
 *   "sampler_walk_factor" a pixel turns from rejection rounds to constrained walks when a round accepts fewer than
 *                   1 in factor * n_steps candidates (and back above 8 times that); 0 (default): 64 up to six sampled
 *                   dimensions, 2 above (the numpy twin takes `walk_factor=`: the two must agree to run alike);
 *   "sampler_walkers"     walkers per pixel of a walk cycle, 64 / 128 / 192 / 256; 0 (default): by the live points
 *                   (128 from 384, 256 from 768);
 *   "sampler_frames"      rotated box frames of a one-ellipsoid bound (nfa_sampler_set_boxes): -2 (default) and -1
 *                   none, 0..64; "sampler_margin_pct": the boxes' margin factor in hundredths (0 = 250);
 *   "sampler_shear_pct"   the shear in front of one-ellipsoid bounds (nfa_sampler_set_shear): its safety factor in
 *                   hundredths, -1 (default) = 300 where the shape allows, 0 = off, 100..100000;
 *   "sampler_pairs_pct"   the pair ellipses of a sheared and boxed bound (nfa_sampler_set_pairs): their safety factor in
 *                   hundredths, -1 (default) = 200, 0 = off, 100..100000 (the host side names sets of these three:
 *                   nestfit_amd.sampler.PRECISION, 'speed' = 250 / 175 / 175, round 4's defaults);
 *   "sampler_ktarget"     replacements per pixel and rejection round a pixel's own share of the round's proposals aims
 *                   at: halved after a round with more than twice as many, doubled after one with fewer than half
 *                   (-1 = the default, 16; 0 = every pixel the round's number); "sampler_ratio_max": proposals drawn
 *                   per round with vetoes on, at most this multiple of the evaluations aimed for (0 = the default,
 *                   32; the candidate buffers are sized by it when a sampler is created); "sampler_kmax": most
 *                   proposals a pixel gets in a round (0 = 65536).  The twin: `k_target=`, `ratio_max=`, `kmax=`;
 *   "sampler_refit_every" rejection-mode pixels refit their bound in rounds that are multiples of this (default 4);
 *                   the sampler_* keys are read when a sampler is created / begun, A/B knobs like the rest;
 *   "ablate"        only in builds with -DNFA_ABLATE (timing experiments, results invalid; the
 *                   shipped library rejects the key): bit mask, 1 skip the Tb pass, 2 skip the
 *                   hyperfine-line loop, 4 skip the rows, 8 skip the line set-up.
 * Unknown keys and values out of range return NFA_ERR_ARG. */
int nfa_set_option(const char *key, int value);

/* 1/(e^x-1) interpolation table.  The reference builds T0_X, T0_Y with numpy at
 * import (nestfit/models/hyperfine.pyx:12-20); the host passes the same
 * arrays so device and reference index identical numbers.  n must be 1000. */
int nfa_set_iemtex_table(const double *t0_x, const double *t0_y, int64_t n);

/* ---- spectra --------------------------------------------------------------
 * Replaces AmmoniaSpectrum.__init__ / Spectrum.__init__
 * (nestfit/models/ammonia.pyx:244-277, nestfit/core/core.pyx:486-520) for all
 * spectra of one pixel or of a whole cube.  Inputs are copied to the device;
 * the caller keeps ownership of its arrays.
 *   sizes[n_spec], trans_ids[n_spec] (1..9), xarr[s] -> sizes[s] doubles
 *   (ascending Hz, shared by all pixels), data[n_pix][sum(sizes)] channel-
 *   contiguous per pixel with spectra concatenated in order, noise[n_pix][n_spec].
 */
int nfa_specset_create(nfa_specset **out, int n_spec, const int64_t *sizes,
                       const int32_t *trans_ids, const double *const *xarr,
                       int64_t n_pix, const double *data, const double *noise);
/* The same for the sibling models on the same kernels:
 *   model 0 = ammonia (as above);
 *   model 1 = N2H+, DiazenyliumSpectrum.__init__ (nestfit/models/diazenylium.pyx:108-136),
 *             trans_ids 1..3 = J 1-0, 2-1, 3-2; parameters per component voff, tex, ltau, sigm
 *             (c_nnhp_predict, diazenylium.pyx:138-154);
 *   model 2 = Gaussian on a plain Spectrum (nestfit/core/core.pyx:486-520 with rest_freq;
 *             c_gauss_predict, nestfit/models/gaussian.pyx:17-50): n_spec must be 1,
 *             trans_ids is ignored, rest_freqs[0] = Spectrum.rest_freq in Hz (NULL = 0 like
 *             the reference's default); parameters per component voff, sigm, peak. */
#define NFA_MODEL_AMMONIA      0
#define NFA_MODEL_DIAZENYLIUM  1
#define NFA_MODEL_GAUSSIAN     2
#define NFA_MODEL_HYPERFINE    3   /* nfa_specset_create_lines below; this function returns NFA_ERR_ARG for it */
#define NFA_MODEL_LTE          4   /* nfa_specset_create_lte below; this function returns NFA_ERR_ARG for it */
#define NFA_MODEL_GRID         5   /* nfa_specset_create_grid below; this function returns NFA_ERR_ARG for it */
#define NFA_GRID_PARAMS        5   /* voff, tkin, lnden, lncol, sigm */
#define NFA_GRID_MAXN          64      /* nodes of an axis of an excitation grid */
#define NFA_GRID_MAXCELLS      65536   /* ... and of the three axes together: nt * nn * nc */
int nfa_specset_create_model(nfa_specset **out, int model, int n_spec, const int64_t *sizes,
                             const int32_t *trans_ids, const double *rest_freqs,
                             const double *const *xarr, int64_t n_pix, const double *data,
                             const double *noise);
/* A noise per channel instead of one per spectrum: chan_noise[n_pix][sum(sizes)], laid out like data.
 * sigma_c > 0 is the noise of channel c; sigma_c = +inf masks the channel: it adds nothing to chi^2 or
 * to null_lnZ and its data value is ignored (it may be NaN).  The log-likelihood is
 *     lnL = -sum_s sum_c (d_c - p_c)^2 / (2 sigma_c^2)      (no normalisation term, like core.pyx:530)
 * Returns NFA_ERR_ARG for a NaN or non-positive sigma_c, for NaN data in a channel that is not masked, and
 * for a (pixel, spectrum) none of whose channels has a finite sigma_c.  Everything else is as for
 * nfa_specset_create_model; a channel noise that is one constant per (pixel, spectrum) gives that
 * function's log-likelihoods and null_lnZ bit for bit.  nfa_specset_set_data keeps the set's mask (the
 * new data of masked channels are ignored); nfa_specset_null_lnz returns -sum_unmasked d^2/(2 sigma_c^2).
 * Single points of such a set go through the batch kernels, and nfa_ring_serve_device refuses its runners
 * (NFA_ERR_ARG; nfa_ring_serve serves them). */
int nfa_specset_create_channel_noise(nfa_specset **out, int model, int n_spec, const int64_t *sizes,
                                     const int32_t *trans_ids, const double *rest_freqs,
                                     const double *const *xarr, int64_t n_pix, const double *data,
                                     const double *chan_noise);
/* model 3 = any species whose spectrum is a set of hyperfine lines sharing one excitation temperature: c_hf_predict
 * (nestfit/models/hyperfine.pyx:52-118) on a line table of the caller's, with the parameters of N2H+ per component
 * (voff, tex, ltau, sigm; parameter-major).  Spectrum s has n_lines[s] lines (1..50) at the rest frequency
 * rest_freqs[s] (Hz); voff (km/s) and tau_wts hold the tables of the spectra one after the other, sum(n_lines) values
 * each.  The optical depth of line i of a component is 10^ltau * tau_wts[i]: the weights are used as given, not
 * normalised, and ltau is shared by the spectra of a pixel (like c_nnhp_predict), so relative optical depths between
 * transitions are folded into the weights.  The order of a table's lines does not matter.
 * Exactly one of noise[n_pix][n_spec] and chan_noise[n_pix][sum(sizes)] is non-NULL (the latter as for
 * nfa_specset_create_channel_noise).  Returns NFA_ERR_ARG, with a message, for a line count outside 1..50, a rest
 * frequency that is not finite and positive, an offset that is not finite or not below the speed of light, a weight
 * that is not finite or is negative, and a table whose weights are all zero; every check of the other creators
 * applies as well. */
int nfa_specset_create_lines(nfa_specset **out, int n_spec, const int64_t *sizes, const int32_t *n_lines,
                             const double *rest_freqs, const double *voff, const double *tau_wts,
                             const double *const *xarr, int64_t n_pix, const double *data, const double *noise,
                             const double *chan_noise);
/* model 4 = one species in LTE across several rotational transitions: column density, excitation temperature and a
 * partition function give every transition its own optical depth.  Parameters per component, parameter-major: voff (km/s),
 * tex (K), lncol = log10 of the total column density (cm^-2), sigm (km/s).  Spectrum s covers ONE transition, with any
 * hyperfine structure inside it: n_lines, rest_freqs, voff and tau_wts as for nfa_specset_create_lines, but the weights
 * of a transition sum to 1; e_up[n_spec] (K) and g_up[n_spec] are its upper level's energy and statistical weight,
 * a_ul[n_spec] (1/s) its Einstein coefficient.  All spectra share the partition function Q, given at n_q (2..64)
 * temperatures q_temp (K, strictly ascending) as q_val.  In cgs units, with T0 = h nu / k:
 *     ln Q(T)  linear in ln T between the bracketing entries of the table; outside it the end segment's line is continued
 *     N_u      = 10^lncol g_up exp(-e_up / tex) / Q(tex)
 *     tau_main = N_u c^2 a_ul / (8 pi nu^2) expm1(T0 / tex) CKMS / (sigm nu sqrt(2 pi))
 * tau_main is the transition's peak optical depth summed over its lines; line i gets tau_main * tau_wts[i], and the
 * spectrum follows as for model 3 (c_hf_predict with tex).  A tex or sigm that is not an ordinary positive number gives
 * NaN.  Returns NFA_ERR_ARG, with a message, for everything nfa_specset_create_lines refuses and for an e_up that is not
 * finite or is negative, a g_up or a_ul that is not finite and positive, a transition whose weights do not sum to 1
 * within 1e-6, n_q outside 2..64, temperatures that are not positive and strictly ascending, and a Q that is not finite
 * and positive. */
int nfa_specset_create_lte(nfa_specset **out, int n_spec, const int64_t *sizes, const int32_t *n_lines,
                           const double *rest_freqs, const double *voff, const double *tau_wts,
                           const double *e_up, const double *g_up, const double *a_ul,
                           int n_q, const double *q_temp, const double *q_val,
                           const double *const *xarr, int64_t n_pix, const double *data, const double *noise,
                           const double *chan_noise);
/* LTE bands: nfa_specset_create_lte with SEVERAL transitions of the species inside one spectrum (the K components of a
 * symmetric top in one window).  Spectrum s covers n_trans[s] (1..8) transitions; the arrays n_lines, trans_freqs, e_up, g_up
 * and a_ul have one entry per transition (sum of n_trans in all), voff and tau_wts one per line, the transitions of a
 * spectrum and the spectra one after the other.  The offsets of a transition's lines are in km/s from its own rest frequency,
 * its weights sum to 1, and the transitions of a spectrum have at most 50 lines together.  Line i of transition g:
 *     hf_freq_i = (1 - voff_i / CKMS) nu_g
 *     tau_i     = tau_main_g(tex, lncol, sigm) tau_wts_i          (tau_main_g: the formula above with nu_g, e_up_g, g_up_g, a_ul_g)
 * and the spectrum follows as for model 3 from all its lines.  The model stays NFA_MODEL_LTE and the parameters voff, tex,
 * lncol, sigm.  The order in which a spectrum's transitions are listed does not change the result.  If every n_trans is 1
 * this is nfa_specset_create_lte, bit for bit.  A set with a banded spectrum is served by the batch entry points, the
 * broker and the callback; nfa_ring_serve_device refuses it.  Returns NFA_ERR_ARG, with a message, for everything
 * nfa_specset_create_lte refuses (per transition) and for an n_trans outside 1..8, more than 50 lines in a spectrum, and
 * a spectrum that lists the same transition (equal frequency, e_up, g_up and a_ul) twice. */
int nfa_specset_create_lte_bands(nfa_specset **out, int n_spec, const int64_t *sizes, const int32_t *n_trans,
                                 const int32_t *n_lines, const double *trans_freqs, const double *voff, const double *tau_wts,
                                 const double *e_up, const double *g_up, const double *a_ul,
                                 int n_q, const double *q_temp, const double *q_val,
                                 const double *const *xarr, int64_t n_pix, const double *data, const double *noise,
                                 const double *chan_noise);
/* LTE mixes: nfa_specset_create_lte_bands with the transitions belonging to n_species (1..4) SPECIES that share a velocity,
 * a width and an excitation temperature along the line of sight -- a molecule and its isotopologue, the A and E species of
 * one -- each with a column density and a partition function of its own.  species[t] (0..n_species - 1) is the species of
 * transition t, one entry per transition like n_lines; n_q[k] the length of species k's partition table, and q_temp and
 * q_val hold the tables one after the other (sum of n_q entries).  The model stays NFA_MODEL_LTE; the parameters of a
 * component are 3 + n_species, parameter-major:
 *     voff, tex, lncol_0, sigm, lncol_1, ..., lncol_{n_species - 1}
 * and transition g of species k has tau_main of the formula above with nu_g, e_up_g, g_up_g, a_ul_g, lncol_k and Q_k(tex).
 * Lines and spectrum follow as for a band, all the species' lines in one optical depth.  A prior program for such a set
 * covers 3 + n_species parameters.  With n_species == 1 this is nfa_specset_create_lte_bands, bit for bit, on its routes.
 * A set of several species is served like a banded one: the batch entry points, the broker and the callback;
 * nfa_ring_serve_device refuses it.  Returns NFA_ERR_ARG, with a message, for everything nfa_specset_create_lte_bands
 * refuses (the same transition twice: within a species), for n_species outside 1..4, a species index outside 0..n_species - 1,
 * a species without a transition in any spectrum, and a bad partition table, naming the species. */
int nfa_specset_create_lte_mix(nfa_specset **out, int n_spec, const int64_t *sizes, const int32_t *n_trans,
                               const int32_t *n_lines, const double *trans_freqs, const double *voff, const double *tau_wts,
                               const double *e_up, const double *g_up, const double *a_ul,
                               int n_species, const int32_t *species, const int32_t *n_q, const double *q_temp, const double *q_val,
                               const double *const *xarr, int64_t n_pix, const double *data, const double *noise,
                               const double *chan_noise);
/* LTE with a beam filling factor: nfa_specset_create_lte_mix, argument for argument and check for check (n_species == 1 is
 * allowed and the common case), whose components have one more parameter, the LAST one: lnff = log10 f, the fraction of the
 * beam the component's gas fills (decadic like lncol).  4 + n_species parameters per component, parameter-major:
 *     voff, tex, lncol_0, sigm, lncol_1, ..., lncol_{n_species - 1}, lnff
 * and the model spectrum is
 *     sum over components c of  10^lnff_c . T0 (y(T0 / tex_c) - tbg) (1 - e^{-tau_c})
 * with tau_c exactly as nfa_specset_create_lte_mix forms it: a thick line reads f (J(tex) - J(Tbg)), not J(tex) - J(Tbg).
 * Nothing bounds f here (a prior does; f > 1 is arithmetic like any other); lnff = -inf gives a component that adds
 * nothing, a NaN lnff NaN spectra and lnL.  The model stays NFA_MODEL_LTE, and a prior program for such a set covers
 * 4 + n_species parameters.
 * DEGENERACY: where every line of a component is optically thin, 1 - e^{-tau} = tau and the spectrum depends on f and the
 * column densities only through f N_k: lnff and the lncol_k are then not separately constrained.  A thick line (which
 * measures f J(tex)) beside thin ones (whose ratios measure tex, whose intensities f N) lifts it; a prior must otherwise.
 * Served by the batch entry points (host and device pointers, predict), single points and a broker's handful (through
 * the batch kernels), the broker, the callback and the device sampler up to 60 dimensions; nfa_ring_serve_device refuses
 * such a set ("the resident kernel has no form for a filling factor: use nfa_ring_serve").  Errors as
 * nfa_specset_create_lte_mix. */
int nfa_specset_create_lte_filled(nfa_specset **out, int n_spec, const int64_t *sizes, const int32_t *n_trans,
                                  const int32_t *n_lines, const double *trans_freqs, const double *voff, const double *tau_wts,
                                  const double *e_up, const double *g_up, const double *a_ul,
                                  int n_species, const int32_t *species, const int32_t *n_q, const double *q_temp, const double *q_val,
                                  const double *const *xarr, int64_t n_pix, const double *data, const double *noise,
                                  const double *chan_noise);
/* model 5 = non-LTE excitation from a grid of the caller's: every transition of a species has an excitation temperature
 * and an optical depth of its own, read from radiative-transfer tables (RADEX, LVG) over kinetic temperature, H2 density
 * and column density per line width.  No molecular data ship: the caller brings the tables, as with line tables and
 * partition functions.  NFA_GRID_PARAMS = 5 parameters per component, parameter-major:
 *     voff (km/s), tkin (K), lnden = log10 n(H2)/cm^-3, lncol = log10 N/cm^-2, sigm (km/s)
 * Spectrum s covers ONE transition with any hyperfine structure inside it: n_lines, rest_freqs, voff and tau_wts as for
 * nfa_specset_create_lte (the weights of a transition sum to 1).  The three axes are shared by all spectra: tkin[nt],
 * lnden[nn] and lncd[nc], each strictly ascending and finite with 1..64 nodes (one node: the axis has no effect),
 * nt nn nc <= 65536; lncd is log10 of the column density per unit line width, N / (cm^-2 (km/s)^-1), the width as FWHM.
 * tex[n_spec][nt][nn][nc] (K) and ltau[n_spec][nt][nn][nc] hold for each spectrum the excitation temperature and log10
 * of the line's peak optical depth summed over its hyperfine lines.  For component c and spectrum s:
 *     x = (tkin_c, lnden_c, lncol_c - log10(sqrt(8 ln 2) sigm_c))
 *     per axis a with nodes a_0 < ... < a_{n-1}:
 *         k = #{ i in 1..n-2 : x >= a_i }                     (n = 1: k = 0)
 *         f = clamp((x - a_k) / (a_{k+1} - a_k), 0, 1)        (n = 1: f = 0) -- outside the grid the edge value holds
 *     v(x) = trilinear over the eight corners, each step v0 + f (v1 - v0), lncd innermost, then lnden, then tkin
 *     tex_{c,s} = tex_s(x)      tau_main_{c,s} = 10^ltau_s(x)
 * and the spectrum follows as for model 3: c_hf_predict with (voff_c, tex_{c,s}, tau_main_{c,s}, sigm_c) on spectrum s,
 * line i with tau_main_{c,s} tau_wts[i].  A tkin, lnden or lncol that is not finite, or a sigm that is not an ordinary
 * positive number, gives a NaN tau_main (model 4's rule).  CLAMPING is deliberate: a prior that leaves the grid sees a
 * flat likelihood in that direction; nothing is extrapolated.
 * A set of this model takes a noise per channel, masked channels, a baseline (nfa_specset_set_baseline), layered
 * transfer and a noise uncertainty; the setters of templates, a continuum, a correlation, a response, a calibration and a
 * robust likelihood refuse it ("a set of the excitation-grid model takes no ...") and leave it as it was.  Served by the
 * batch entry points (host and device pointers, predict), single points and a broker's handful (through the batch
 * kernels), the broker, the callback and nfa_ring_serve; nfa_ring_serve_device refuses it ("the resident kernel has no
 * form for an excitation per spectrum: use nfa_ring_serve").
 * Returns NFA_ERR_ARG, with a message, for everything nfa_specset_create_lines refuses, a transition whose weights do
 * not sum to 1 within 1e-6, a node count outside 1..64, nt nn nc above 65536, an axis that is not finite and strictly
 * ascending, a tex that is not finite and positive (a population inversion: cut the grid) and an ltau that is not
 * finite. */
int nfa_specset_create_grid(nfa_specset **out, int n_spec, const int64_t *sizes, const int32_t *n_lines,
                            const double *rest_freqs, const double *voff, const double *tau_wts,
                            int nt, const double *tkin, int nn, const double *lnden, int nc, const double *lncd,
                            const double *tex, const double *ltau,
                            const double *const *xarr, int64_t n_pix, const double *data, const double *noise,
                            const double *chan_noise);
/* A shipped line table, as a template for nfa_specset_create_lines: model 0 (trans_id 1..9) or 1 (trans_id 1..3);
 * voff and tau_wts take 50 doubles each (zero behind the *n lines), *nu the rest frequency in Hz.  Needs no device. */
int nfa_builtin_lines(int model, int trans_id, double *nu, double *voff, double *tau_wts, int *n);
int nfa_specset_destroy(nfa_specset *ss);
int nfa_specset_set_data(nfa_specset *ss, int64_t pix, const double *data);
/* null_lnZ[n_pix][n_spec] = -sum(data^2)/(2 noise^2)   (core.pyx:517-520); with a baseline, the baseline-only model:
 * -chi2_min(p = 0) / (2 sigma_ref^2) (nfa_specset_set_baseline) */
int nfa_specset_null_lnz(const nfa_specset *ss, double *out);
/* A polynomial baseline of degree <= order per (pixel, spectrum), profiled out of the likelihood in closed form (no sampler
 * dimension).  With weights w_c (1 for a scalar noise, (sigma_ref / sigma_c)^2 for a channel noise, 0 where masked),
 * residual r = d - p(theta) and V_K the polynomials of degree <= K in the channel index of the spectrum:
 *     chi2_min,s = min_{b in V_K} sum_c w_c (r_c - b_c)^2,    lnL = -sum_s chi2_min,s / (2 sigma_ref,s^2)
 * That is the marginal likelihood under a flat prior on the baseline's coefficients up to a factor that depends only on the
 * pixel, its weights and K -- the same for nfa_specset_null_lnz, which then returns the baseline-only model, and for every
 * ncomp: differences of lnZ are Bayes factors of baseline-marginalised models.  A spectrum with n <= K unmasked channels
 * gets degree n - 1 (its chi2_min is 0).
 * order = -1 removes the baseline (the set's former results bit for bit), 0..NFA_BASELINE_MAX sets it; anything else
 * returns NFA_ERR_ARG.  Batches held for coalescing are launched first (as by nfa_set_option) and the device is
 * synchronised: call it between batches, not while one of this set's runners is in flight.  nfa_specset_set_data keeps
 * the order.  Spectra out are unchanged: the model without the baseline.  Single points of such a set go through the
 * batch kernels, and nfa_ring_serve_device refuses its runners (NFA_ERR_ARG; nfa_ring_serve serves them). */
#define NFA_BASELINE_MAX 3
int nfa_specset_set_baseline(nfa_specset *ss, int order);
/* Layered radiative transfer: the components of a parameter vector are layers along the line of sight, component 0 the
 * FARTHEST from the observer and the last the nearest, and each absorbs what lies behind it.  The model spectrum, measured
 * against the background like the summed one, is built in component order,
 *     pred <- pred + (g_c - pred) a_c        g_c = T0 (y(T0 / tex_c) - tbg),  a_c = 1 - e^{-tau_c}
 * (a filled LTE set: a_c = 10^lnff_c (1 - e^{-tau_c}), exact where the layers in front fill the beam, a random-covering
 * approximation where they cover it partly), where the summed model is sum_c g_c a_c (hyperfine.pyx:104-118).  A component
 * with tau_c = 0 in a channel leaves it as it is; one component is the summed model; components that do not overlap in
 * velocity are too.  The layout of the parameter vector does not change, but the component labels are no longer
 * exchangeable: an ordered-velocity prior now ties the order along the line of sight to the order in velocity.
 * on != 0 sets, 0 clears (a new set is summed).  Every set kind takes it -- ammonia, N2H+, line tables, LTE, bands, mixes,
 * filled sets, with a channel noise and a baseline or without -- but the Gaussian model, which has no optical depth:
 * NFA_ERR_ARG.  Like nfa_specset_set_baseline it launches held batches first, synchronises the device and drops the
 * runners' captured single-point graphs: call it between batches.  Layered sets go through the batch kernels (the general
 * component form); single points and a broker's handful too, and nfa_ring_serve_device refuses their runners ("the resident
 * kernel has no form for layered transfer: use nfa_ring_serve"). */
int nfa_specset_set_layered(nfa_specset *ss, int on);
/* 1 for a layered set, 0 for a summed one (and for null) */
int nfa_specset_layered(const nfa_specset *ss);
/* A calibration uncertainty per spectrum, integrated out of the likelihood in closed form (no sampler dimension).  The data
 * of spectrum s are d = g p(theta) + baseline + noise with a gain g ~ N(1, cal[s]^2): cal[n_spec] are the fractional 1-sigma
 * uncertainties of the spectra's intensity scales, shared by all pixels, each finite and in [0, 1].  With the weighted
 * products <x,y> = sum_c w_c x_c y_c (the baseline, if any, projected out of both), A = <p,p>, B = <d,p> and chi2_1 the value
 * at g = 1 (what the set computes without a calibration):
 *     lnL_s = -[chi2_1 - s^2 (B - A)^2 / (sigma^2 + s^2 A)] / (2 sigma^2) - log1p(s^2 A / sigma^2) / 2
 * The last term depends on theta and belongs to the marginal; nfa_specset_null_lnz (p = 0) is unchanged, so lnZ - null_lnZ
 * stays a Bayes factor.  A spectrum with cal[s] = 0 keeps chi2_1 to the bit.  The gain is a marginalised nuisance with a
 * proper prior, independent per (pixel, spectrum): it is no parameter of an information criterion.
 * cal = NULL or all zeros removes the calibration (the set's former kernels and results bit for bit); a value that is not
 * finite or lies outside [0, 1] returns NFA_ERR_ARG and leaves the set as it was.  Every set kind and model takes it, with
 * a channel noise, a baseline or layering or without; it commutes with nfa_specset_set_baseline.  Like that call it
 * launches held batches first, synchronises the device and drops the runners' captured single-point graphs: call it
 * between batches.  nfa_specset_set_data keeps it.  Spectra out are unchanged: the model at g = 1.  Calibrated sets go
 * through the batch kernels (the general component form); single points and a broker's handful too, and
 * nfa_ring_serve_device refuses their runners ("the resident kernel has no form for a calibration uncertainty: use
 * nfa_ring_serve"). */
int nfa_specset_set_calibration(nfa_specset *ss, const double *cal);
/* 1 and out[n_spec] = the values set (out may be null), or 0 for a set without a calibration uncertainty (and for null) */
int nfa_specset_calibration(const nfa_specset *ss, double *out);
/* Channel noise correlated along the spectral axis (Hanning smoothing, regridding, an oversampling correlator).  The noise
 * of spectrum s is n_c = sigma_c eps_c, sigma_c the set's scalar or per-channel noise and eps the zero-mean, unit-variance
 * stationary Gaussian AR(2) process whose first two autocorrelations are rho[s][0], rho[s][1] (the maximum-entropy process
 * with those two; AR(1) is rho_2 = rho_1^2).  Yule-Walker: phi_1 = rho_1 (1 - rho_2) / (1 - rho_1^2), phi_2 = (rho_2 -
 * rho_1^2) / (1 - rho_1^2), v = 1 - phi_1 rho_1 - phi_2 rho_2; the inverse of the correlation matrix R is pentadiagonal
 * in closed form, and with u_c = sigma_ref / sigma_c, Q = diag(u) R^-1 diag(u):
 *     lnL_s = -(d - p)^T Q (d - p) / (2 sigma_ref^2)
 * without a normalisation term, like every likelihood here (-ln det R / 2, ln det R = (N - 2) ln v + ln(1 - rho_1^2), is
 * a constant of the data).  nfa_specset_null_lnz is the same expression at p = 0.
 * rho[n_spec][2], shared by all pixels.  rho = NULL or all zeros removes the correlation (the set's former kernels and
 * results bit for bit); a spectrum whose pair is (0, 0) beside correlated ones keeps white noise.  NFA_ERR_ARG, the set
 * left as it was: a value that is not finite, |rho_1| >= 1, rho_2 outside (2 rho_1^2 - 1, 1), v < 0.01 (the noise nearly
 * determined by its neighbours: Q ill-conditioned), a spectrum of fewer than 4 channels; a set with a masked channel
 * (channel noise inf), a baseline or a calibration uncertainty -- and nfa_specset_set_baseline (order >= 0) and
 * nfa_specset_set_calibration (a value > 0) refuse a correlated set likewise.  Every model, filled and layered sets too.
 * Like nfa_specset_set_baseline it launches held batches first, synchronises the device and drops the runners' captured
 * single-point graphs: call it between batches.  nfa_specset_set_data keeps it.  Spectra out are the model, unchanged.
 * Correlated sets go through the batch kernels (the general component form); single points and a broker's handful too, and
 * nfa_ring_serve_device refuses their runners ("the resident kernel has no form for correlated channel noise: use
 * nfa_ring_serve"). */
int nfa_specset_set_correlation(nfa_specset *ss, const double *rho);
/* 1 and out[n_spec][2] = the pairs set (out may be null), or 0 for a set without a noise correlation (and for null) */
int nfa_specset_correlation(const nfa_specset *ss, double *out);
/* The channel response of the spectrometer (Hanning smoothing, regridding): the operation that correlates the noise also
 * convolves the signal.  taps[n_spec][5] = (h_-2, h_-1, h_0, h_1, h_2) per spectrum in units of channels, shared by all
 * pixels; a response of three taps has zero ends.  The model that enters the likelihood is then
 *     p~_j = sum_{k = -2..2} h_k p_{j+k},    p_i := 0 for i < 0 and i >= N,
 * p the model spectrum at the channel centres, and everything downstream takes p~ for p: lnL = -(d - p~)^T Q (d - p~) /
 * (2 sigma_ref^2) with nfa_specset_set_correlation's Q, or diag(w) or 1 without a correlation; spectra out (predict_batch)
 * are p~.  nfa_specset_null_lnz does not change (p = 0 gives p~ = 0).  A line within two channels of a band end loses the
 * part of the response that reaches beyond it.
 * taps = NULL or the identity (0, 0, 1, 0, 0) in every spectrum removes the response (the set's former kernels and results
 * bit for bit); the identity beside real responses is an unfiltered spectrum.  NFA_ERR_ARG, the set left as it was: a tap
 * that is not finite, |sum h - 1| > 1e-9 (a response conserves the integrated intensity), h_0 <= 0, a spectrum of fewer than
 * 4 channels; a set with a masked channel (channel noise inf), a baseline or a calibration uncertainty -- and
 * nfa_specset_set_baseline (order >= 0) and nfa_specset_set_calibration (a value > 0) refuse a set with a response likewise.
 * It goes with and without nfa_specset_set_correlation, in either order.  Every model, filled and layered sets too.
 * Like nfa_specset_set_correlation it launches held batches first, synchronises the device and drops the runners' captured
 * single-point graphs: call it between batches.  nfa_specset_set_data keeps it.  Such sets go through the batch kernels (the
 * general component form); single points and a broker's handful too, and nfa_ring_serve_device refuses their runners ("the
 * resident kernel has no form for a channel response: use nfa_ring_serve"). */
int nfa_specset_set_response(nfa_specset *ss, const double *taps);
/* 1 and out[n_spec][5] = the taps set (out may be null), or 0 for a set without a channel response (and for null) */
int nfa_specset_response(const nfa_specset *ss, double *out);
/* Nuisance templates: fixed shapes on the channel grid that the caller knows up to an amplitude -- a standing wave of known
 * period (its sine and cosine), a bandpass residual, an atmospheric feature, an RFI comb -- profiled out of the likelihood
 * together with the polynomial baseline, in closed form and without a sampler dimension.  With nfa_specset_set_baseline's
 * weights w_c and polynomial basis P_0..P_K (K = -1: none) and the templates t_1..t_T of spectrum s:
 *     V = span{P_0..P_K, t_1..t_T},   chi2_min,s = min_{b in V} sum_c w_c (r_c - b_c)^2,   lnL = -sum_s chi2_min,s / (2 sigma_ref,s^2)
 * nfa_specset_null_lnz is the same expression at p = 0, and the Bayes-factor argument of nfa_specset_set_baseline holds
 * unchanged.  A direction of V that the others already span (a constant template beside order 0, a template given twice, a
 * spectrum with fewer unmasked channels than basis functions) is dropped by that call's rank rule.
 * t[NFA_TMPL_MAX][sum(sizes)]: slot k of every spectrum, the spectra concatenated like `data`; n_tmpl[n_spec] in
 * 0..NFA_TMPL_MAX says how many slots of spectrum s are used (the others are not read).  The templates are shared by all
 * pixels.  The engine scales each to max |t| = 1; nfa_specset_templates returns the caller's values.
 * t = NULL, n_tmpl = NULL or all counts zero removes the templates (the set's former kernels and results bit for bit).
 * NFA_ERR_ARG, the set left as it was: a count outside 0..NFA_TMPL_MAX, a value that is not finite, a template that is zero
 * over its whole spectrum; a set with a calibration uncertainty, correlated channel noise or a channel response ("... takes
 * no nuisance templates") -- and nfa_specset_set_calibration, nfa_specset_set_correlation and nfa_specset_set_response
 * refuse a set with templates likewise.  With masked channels, a noise per channel, filled and layered sets: yes.  It
 * commutes with nfa_specset_set_baseline.  Like that call it launches held batches first, synchronises the device and
 * drops the runners' captured single-point graphs: call it between batches.  nfa_specset_set_data keeps the templates.
 * Spectra out are unchanged: the model without nuisance terms.  Such sets go through the batch kernels (the general
 * component form); single points and a broker's handful too, and nfa_ring_serve_device refuses their runners ("the resident
 * kernel has no form for nuisance templates: use nfa_ring_serve"). */
#define NFA_TMPL_MAX 4
int nfa_specset_set_templates(nfa_specset *ss, const double *t, const int *n_tmpl);
/* 1, out_t[NFA_TMPL_MAX][sum(sizes)] = the values set (unused slots zero) and out_n[n_spec] = the counts (either may be
 * null), or 0 for a set without templates (and for null) */
int nfa_specset_templates(const nfa_specset *ss, double *out_t, int *out_n);
/* An uncertain noise level per spectrum, integrated out of the likelihood in closed form (no sampler dimension, DESIGN
 * 4.16).  The true noise of spectrum s is t sigma_c, sigma_c the set's scalar or per-channel noise and t one unknown scale
 * for all its channels; the precision tau = 1 / t^2 has a Gamma prior of shape a and rate a (mean 1), a = 1 / (4 f^2) for the
 * fractional 1-sigma uncertainty f[s] of the noise level (std(tau) = 2 f to first order).  With nu the unmasked channels of
 * the (pixel, spectrum) and X = chi2_s / sigma_ref^2 whatever the set's kind makes of it (baseline, templates, correlation
 * and response included):
 *     lnL = sum_s -(a_s + nu_s / 2) log1p( (chi2_s / (2 sigma_s^2)) / a_s )
 * constants dropped as everywhere.  f -> 0 gives -chi2 / (2 sigma^2); a spectrum with f[s] = 0 keeps that expression to the
 * bit.  nfa_specset_null_lnz is the same function of the set's own null value (what it returns without the uncertainty): the
 * likelihood at p = 0 to rounding, and to the bit where the two already agree to the bit (spectra of 64 channels and less).  A
 * row with a NaN parameter or NaN data is NaN, as in every set.  nu counts channels only (the profile
 * convention): it does not subtract the rank of a baseline or of templates, depends on the masks alone, and the call
 * commutes with nfa_specset_set_baseline, _set_templates, _set_correlation and _set_response.
 * f[n_spec], shared by all pixels; f = NULL or all zeros removes it (the set's former results bit for bit).  NFA_ERR_ARG,
 * the set left as it was, before any device call: a value that is not finite or lies outside [0, 0.5] ("a noise
 * uncertainty is ...": above 0.5 the first-order relation between f and a means nothing); a set with a calibration
 * uncertainty, whose part is no chi^2 -- and nfa_specset_set_calibration refuses a set with a noise uncertainty in the
 * same words.  No likelihood kernel changes: every set kind, launch form, single points, a broker, nfa_ring_serve,
 * nfa_ring_serve_device and the device sampler serve such a set.  Like nfa_specset_set_calibration it launches held
 * batches first, synchronises the device and drops the runners' captured single-point graphs: call it between batches.
 * nfa_specset_set_data keeps it.  Spectra out are unchanged. */
int nfa_specset_set_noise_uncertainty(nfa_specset *ss, const double *f);
/* 1 and out[n_spec] = the values set (out may be null), or 0 for a set without a noise uncertainty (and for null) */
int nfa_specset_noise_uncertainty(const nfa_specset *ss, double *out);
/* A continuum background: a source of brightness temperature Tc >= 0 (K, on the data's scale) behind all components of a
 * (pixel, spectrum) -- an H II region, a dust peak, a quasar -- whose level was subtracted from the data, so that a line goes
 * NEGATIVE wherever J(tex) < J(Tcmb) + Tc.  With g_c = T0 (y(T0 / tex_c) - tbg) and a_c = 1 - FastExp(tau_c) (a filled set:
 * f_c times that):
 *     summed:   pred = sum_c (g_c - Tc) a_c          layered:   pred <- pred + (g_c - Tc - pred) a_c
 * Tc is DATA, not a parameter: it comes from the continuum map that was subtracted (the subtracted cube cannot give it back),
 * and the sampler's dimensions, the optical depths and nfa_specset_null_lnz (the null model has no absorber) do not change.
 * With nfa_specset_set_baseline(ss, 0) the same likelihood fits data whose continuum was NOT subtracted: the offset is
 * profiled out, the depth still needs Tc.  On a filled set the form is exact where the layer covers the source.
 * tc[n_pix][n_spec].  tc = NULL or all zeros removes the continuum (the set's former kernels and results bit for bit).
 * NFA_ERR_ARG, the set left as it was: a value that is negative or not finite; the Gaussian model (no optical depth); a set with
 * a calibration uncertainty, correlated channel noise, a channel response or nuisance templates ("... takes no continuum
 * background") -- and nfa_specset_set_calibration, nfa_specset_set_correlation, nfa_specset_set_response and
 * nfa_specset_set_templates refuse a set with a continuum in the same words.  With a scalar noise and a noise per channel,
 * masked channels, a baseline (the two calls commute), layered and filled sets, every hyperfine and LTE model and
 * nfa_specset_set_noise_uncertainty: yes.  Like nfa_specset_set_baseline it launches held batches first, synchronises the
 * device and drops the runners' captured single-point graphs: call it between batches.  nfa_specset_set_data keeps the
 * continuum.  Spectra out are the model against the off-line level, negative in absorption.  Such sets go through the batch
 * kernels (the general component form); single points and a broker's handful too, and nfa_ring_serve_device refuses their
 * runners ("the resident kernel has no form for a continuum background: use nfa_ring_serve"). */
int nfa_specset_set_continuum(nfa_specset *ss, const double *tc);
/* 1 and out[n_pix][n_spec] = the values set (out may be null), or 0 for a set without a continuum (and for null) */
int nfa_specset_continuum(const nfa_specset *ss, double *out);
/* A robust likelihood: each channel's noise is Student-t with nu degrees of freedom and scale sigma_j instead of Gaussian
 * -- a Gaussian whose precision per CHANNEL is Gamma(nu / 2, nu / 2)-distributed and integrated out in closed form -- so that
 * an interference spike or a bad channel nobody flagged costs the logarithm of its residual, not its square.  With the
 * weights w_j of a noise per channel (1 for a scalar noise, 0 where masked) and a_j = w_j / (nu sigma_ref^2),
 *     lnL_s = -(nu + 1) / 2 sum_j log1p(a_j (d_j - p_j)^2)
 * without the normalisation, as everywhere; Gaussian in the limit of large nu.  It adds no sampler dimension.
 * nfa_specset_null_lnz is the same expression at p = 0, bit for bit the likelihood kernel's value there.
 * nu[n_spec]: 0 keeps that spectrum Gaussian beside robust ones.  nu = NULL or all zeros removes it (the set's former kernels
 * and results bit for bit).  NFA_ERR_ARG, the set left as it was: a value that is not finite, or neither 0 nor in [1, 1e6]
 * (beyond 1e6 the value is the Gaussian one within 1e-6: leave it out); a set with a baseline, nuisance templates, a
 * calibration uncertainty, a channel response, correlated channel noise, a noise uncertainty or a continuum background
 * ("a set with ... takes no robust likelihood": under a t likelihood no linear nuisance has a closed form and a part is no
 * chi^2) -- and those setters refuse a robust set ("a set with a robust likelihood takes no ...").  With a scalar noise
 * and a noise per channel, masked channels, layered and filled sets, every model: yes.  Like nfa_specset_set_baseline it
 * launches held batches first, synchronises the device and drops the runners' captured single-point graphs: call it between
 * batches.  nfa_specset_set_data keeps it.  Spectra out do not change.  Such sets go through the batch kernels (the general
 * component form); single points and a broker's handful too, and nfa_ring_serve_device refuses their runners ("the resident
 * kernel has no form for a robust likelihood: use nfa_ring_serve"). */
int nfa_specset_set_robust(nfa_specset *ss, const double *nu);
/* 1 and out[n_spec] = the values set (out may be null), or 0 for a set without a robust likelihood (and for null) */
int nfa_specset_robust(const nfa_specset *ss, double *out);
/* tbg[sum(sizes)] = 1/expm1(h nu / (k TCMB))           (ammonia.pyx:273-277) */
int nfa_specset_tbg(const nfa_specset *ss, double *out);
int64_t nfa_specset_chan_tot(const nfa_specset *ss);

/* ---- priors ---------------------------------------------------------------
 * Replaces PriorTransformer + the Prior family (nestfit/core/core.pyx:169-476).
 * A prior program is the ordered list of priors (executed in order, in place,
 * like c_transform, core.pyx:459-476) plus the Distribution tables
 * (core.pyx:23-45: xax, pdf, cdf, ppf of `size` doubles each).
 */
enum {
    NFA_PRIOR_SIMPLE = 0,             /* Prior                  core.pyx:169-197 */
    NFA_PRIOR_DUPLICATE = 1,          /* DuplicatePrior         core.pyx:200-221 */
    NFA_PRIOR_CONSTANT = 2,           /* ConstantPrior          core.pyx:224-238 */
    NFA_PRIOR_ORDERED = 3,            /* OrderedPrior           core.pyx:241-258 */
    NFA_PRIOR_SPACED = 4,             /* SpacedPrior            core.pyx:261-292 */
    NFA_PRIOR_CENSEP = 5,             /* CenSepPrior            core.pyx:295-318 */
    NFA_PRIOR_RESOLVED_CENSEP = 6,    /* ResolvedCenSepPrior    core.pyx:321-366 */
    NFA_PRIOR_RESOLVED_PLACEMENT = 7  /* ResolvedPlacementPrior core.pyx:369-435 */
};

typedef struct {
    int64_t size;
    double  du, dx, xmin, xmax;
    const double *xax, *pdf, *cdf, *ppf;
} nfa_dist_desc;

typedef struct {
    int32_t kind;
    int32_t p_ix;      /* parameter slot (vcen slot for the composite kinds) */
    int32_t p_ix2;     /* duplicate slot / sigm slot                         */
    int32_t dist0;     /* main / vcen / independent distribution             */
    int32_t dist1;     /* vsep / dependent distribution                      */
    int32_t dist2;     /* sigm distribution                                  */
    int32_t sub_kind;  /* kind of the sigm sub-prior (SIMPLE/CONSTANT/ORDERED) */
    int32_t pad_;
    double  value;     /* constant value                                     */
    double  sep_scale; /* FWHM * scale                                       */
} nfa_prior_desc;

int nfa_priors_create(nfa_priors **out, const nfa_prior_desc *priors, int n_prior,
                      const nfa_dist_desc *dists, int n_dist, int n_param);
int nfa_priors_destroy(nfa_priors *p);
/* PriorTransformer.transform (core.pyx:478-483) over B rows of U[B][n_param*ncomp],
 * host memory, in place.  NFA_ERR_ARG when ndim != n_param*ncomp. */
int nfa_priors_transform_batch(const nfa_priors *p, double *U, int64_t B,
                               int ncomp, int ndim);

/* ---- runner ---------------------------------------------------------------
 * Replaces AmmoniaRunner (nestfit/models/ammonia.pyx:369-447).  `priors` may be
 * NULL for predict-only use (amm_predict, ammonia.pyx:364-366).
 */
int nfa_runner_create(nfa_runner **out, nfa_specset *ss, nfa_priors *priors,
                      int ncomp, int cold, int lte);
int nfa_runner_destroy(nfa_runner *r);
int nfa_runner_ndim(const nfa_runner *r);
/* Numerical mode of this runner: -1 (default) = whatever nfa_set_exp_mode says when a batch is
 * launched; 0..2 = pinned, so that runners of different modes can work side by side (threads of a
 * broker, a table-mode checker next to a fast-mode sampler). */
int nfa_runner_set_exp_mode(nfa_runner *r, int mode);
int nfa_runner_get_exp_mode(const nfa_runner *r);

/* AmmoniaRunner.c_loglikelihood (ammonia.pyx:423-432) for B unit-cube rows of
 * pixel `pix[b]` (pix == NULL: pixel 0).  U[B][ndim] host memory, overwritten
 * in place with the physical parameters exactly like the reference mutates
 * `utheta`; lnL[B] out.  Synchronous.  Up to 128 rows take one launch (point kernel), more go through
 * the batch kernels with copies in and out; the values do not depend on the route. */
int nfa_runner_loglike_batch(nfa_runner *r, const int32_t *pix, double *U,
                             double *lnL, int64_t B);
/* Host buffers the device can address (pinned and mapped).  A U / lnL / pix buffer of
 * nfa_runner_loglike_batch that lies in such memory (from here, or registered with the HIP runtime by the
 * caller) is not copied: the kernels read the unit cube over the bus and write theta and lnL in place
 * (no reference counterpart: the reference's arrays never leave the host). */
int nfa_host_alloc(void **out, size_t bytes);
int nfa_host_free(void *p);

/* AmmoniaRunner.predict / amm_predict (ammonia.pyx:437-447, 364-366) for B
 * parameter rows theta[B][ndim] (no priors).  spectra_out[B][chan_tot] and/or
 * lnL_out[B] may be NULL; output buffers from nfa_host_alloc are written by the kernels themselves. */
int nfa_runner_predict_batch(nfa_runner *r, const int32_t *pix, const double *theta,
                             int64_t B, double *spectra_out, double *lnL_out);

/* Weighted posterior moments of model spectra; host pointers, synchronous.  Segment g is the rows seg_off[g] ..
 * seg_off[g + 1] - 1 of theta (physical parameters, as for nfa_runner_predict_batch), all of pixel seg_pix[g], with
 * weights w_i >= 0.  p_i is the model spectrum nfa_runner_predict_batch returns for row i (the runner's numerical mode;
 * the filtered, layered, filled and continuum forms where the set has them).  The moments are taken about the segment's
 * row of largest weight i* (the first on ties), d_i = p_i - p_i*: with S0 = sum w_i, S1 = sum w_i d_i, S2 = sum w_i d_i^2
 *     mean = p_i* + S1 / S0,    std = sqrt(max(S2 / S0 - (S1 / S0)^2, 0))
 * per channel -- raw second moments cancel where the posterior is tight.  The row statistics are the peak (the
 * NaN-ignoring maximum; for a set with a continuum the signed value of largest magnitude) and the total (the NaN-ignoring
 * sum) of every (row, spectrum); their weighted mean and std over a segment are the same moments.  A segment without
 * rows or with S0 = 0 gives NaN, a segment of one row std = 0.  The rows are predicted chunk_rows at a time and reduced
 * on the device; no sum depends on scheduling: the same arguments give the same bits.
 * NFA_ERR_ARG: a negative or non-finite weight, a decreasing seg_off, a chunk_rows that is no multiple of 64, all four
 * outputs null, a pixel out of range.  n_seg = 0 is a no-op. */
int nfa_runner_predict_moments(nfa_runner *r, int64_t n_seg, const int32_t *seg_pix /* NULL: pixel 0 */,
        const int64_t *seg_off /* [n_seg+1], seg_off[0] = 0, non-decreasing */,
        const double *theta /* [seg_off[n_seg]][ndim] */, const double *weight /* or NULL */,
        int64_t chunk_rows /* 0: 4096; else a multiple of 64 */,
        double *spec_mean /* [n_seg][chan_tot] or NULL */, double *spec_std /* or NULL */,
        double *stat_mean /* [n_seg][n_spec][2]: peak, total; or NULL */, double *stat_std /* or NULL */);
/* peak and total of every spectrum of B rows: peak_and_integrated without the spectra crossing the bus */
int nfa_runner_row_statistics(nfa_runner *r, const int32_t *pix, const double *theta, int64_t B,
        double *peak /* [B][n_spec] */, double *total /* [B][n_spec] */);

/* The normal equations of a least-squares fit at B points (pixel, theta); host pointers, synchronous.
 * p(theta) is the model spectrum nfa_runner_predict_batch returns for the point (the runner's numerical mode; the layered,
 * filled and continuum forms where the set has them).  The probes of parameter k are theta+ = theta + step_k e_k and theta- =
 * theta - step_k e_k, each clipped into [lower_k, upper_k] where those are given, and
 *     J_k = (p(theta+) - p(theta-)) / (theta+_k - theta-_k)
 * with the difference of the two doubles as they are; a parameter with theta+_k == theta-_k is fixed and has J_k = 0.  The
 * weight of channel j is W_j = 1 / sigma^2 for a scalar noise and chan_w_j / sigma_ref^2 for a noise per channel; a channel of
 * weight 0 (masked) is left out whatever the model or the data hold there, and a model value that is not finite at a channel
 * of positive weight makes the point's outputs NaN.  With r_j = d_j - p_j(theta):
 *     chi2 = sum_j W_j r_j^2,   grad_k = sum_j W_j J_kj r_j (= -1/2 d chi2 / d theta_k),   curv_kl = sum_j W_j J_kj J_lj
 * (full and symmetric, both triangles written): the entries of one augmented Gram matrix [J r]^T W [J r].  With grad and curv
 * both null the call predicts one row per point and returns chi2 alone, the same bits as the full call's; step may then be
 * null.  Otherwise a point takes R = 1 + 2 ndim rows, a chunk holds floor(chunk_rows / R) points, and the spectra are reduced
 * on the device as each chunk is predicted; no sum depends on scheduling: the same arguments give the same bits.
 * NFA_ERR_ARG: a null theta or chi2, grad or curv without step, a step that is not finite and > 0, lower_k > upper_k, a
 * chunk_rows that is no multiple of 64 or smaller than R, ndim > NFA_LSQ_MAX_DIM, a pixel out of range.  NFA_ERR_STATE, with a
 * sentence: a set whose likelihood is not -chi^2 / 2 of white noise -- a baseline, templates, a calibration uncertainty, a noise
 * correlation, a channel response, a noise uncertainty, a robust likelihood.  B = 0 is a no-op. */
#define NFA_LSQ_MAX_DIM  24
int nfa_runner_normal_equations(nfa_runner *r, const int32_t *pix /* [B] or NULL: pixel 0 */,
        const double *theta /* [B][ndim], physical parameters as for nfa_runner_predict_batch */, int64_t B,
        const double *step /* [ndim], > 0 */, const double *lower /* [ndim] or NULL */, const double *upper /* [ndim] or NULL */,
        int64_t chunk_rows /* 0: 4096; else a multiple of 64 and >= 1 + 2 ndim */,
        double *chi2 /* [B] */, double *grad /* [B][ndim] or NULL */, double *curv /* [B][ndim][ndim] or NULL */);

/* Same as nfa_runner_loglike_batch with every buffer already resident in device
 * memory (from nfa_malloc); enqueued, returns without synchronising.  d_pix may be
 * NULL.  Consecutive calls of one shape may be launched together (option "coalesce");
 * consecutive launches go to different HIP streams of the runner (round robin) and may
 * overlap on the device: the buffers of calls that are in flight together must not
 * alias, and the caller's buffers must stay valid until nfa_runner_synchronize (or
 * nfa_device_synchronize), which launches what is still held and waits for all of it. */
int nfa_runner_loglike_batch_dev(nfa_runner *r, const int32_t *d_pix, double *d_U,
                                 double *d_lnL, int64_t B);
/* Spectra-out with device pointers (what AmmoniaRunner.predict is to deblend_hf_intensity /
 * generate_predicted_profiles, nestfit/main.py:1106-1113, 1182-1188, for a caller whose MAP cube and
 * profile cube stay in HBM): d_theta [B x ndim] physical parameters (read only), d_spectra
 * [B x chan_tot] or NULL, d_lnL [B] or NULL (not both NULL).  Asynchronous and rotating over the
 * runner's streams like nfa_runner_loglike_batch_dev, and like its batches consecutive calls of one
 * shape (same B, a multiple of 64; the same of d_pix / d_spectra / d_lnL given) travel as one launch,
 * every batch writing its own arrays (option "coalesce"; since round 5: a launch of one 4096-row batch is
 * as long as its longest wave); same results as nfa_runner_predict_batch. */
int nfa_runner_predict_batch_dev(nfa_runner *r, const int32_t *d_pix, const double *d_theta, int64_t B,
                                 double *d_spectra, double *d_lnL);
int nfa_runner_synchronize(nfa_runner *r);
/* Per-kernel timing of nfa_runner_loglike_batch_dev with HIP events recorded on
 * the stream each kernel is launched on, over the calls made since profiling was
 * switched on.  out[0], out[1]: summed milliseconds of the set-up kernel and of the
 * likelihood kernel (lnl_kernel alone: the interval rocprofv3 reports for it when the
 * runner has one stream lane); out[2], out[3]: milliseconds during which at least one set-up /
 * likelihood kernel was running (union of the launch intervals: with several stream
 * lanes launches overlap and the plain sum counts that time more than once). */
int nfa_runner_set_profiling(nfa_runner *r, int on);
int nfa_runner_get_profile(nfa_runner *r, double *out, int64_t *calls);

/* MultiNest `LogLike` (nestfit/core/cmultinest.pxd:27-28; the reference's
 * trampoline is mn_loglikelihood, nestfit/core/core.pyx:622-624).  Pass the
 * nfa_runner* as MultiNest's `context`. */
void nfa_loglike_callback(double *Cube, int *ndim, int *npars, double *lnew, void *ctx);

/* ---- callback-coalescing broker -------------------------------
 * MultiNest evaluates one point per LogLike call (cmultinest.pxd:27-28); the broker
 * gathers concurrent calls of many sampler threads into GPU batches.
 * nfa_broker_loglike blocks the calling thread until its batch has run: `cube` (ndim
 * doubles in the unit cube) is overwritten with the physical parameters and *lnew set,
 * exactly like mn_loglikelihood -> c_loglikelihood (core.pyx:622-624,
 * ammonia.pyx:423-432); pix < 0 = the runner's only pixel.  A generation's first caller
 * leads it: it launches when n_clients requests (0 = unknown) or max_batch are queued, or
 * after max_wait_us.  Results are bitwise those of nfa_runner_loglike_batch.
 * nfa_broker_callback has MultiNest's LogLike signature; its context is an
 * nfa_broker_client (broker + pixel).  The runner must not be used directly while a
 * broker serves it. */
typedef struct nfa_broker nfa_broker;
typedef struct { nfa_broker *broker; int32_t pix; } nfa_broker_client;
int  nfa_broker_create(nfa_broker **out, nfa_runner *r, int max_batch, int64_t max_wait_us, int n_clients);
int  nfa_broker_destroy(nfa_broker *b);
int  nfa_broker_set_clients(nfa_broker *b, int n_clients);
int  nfa_broker_loglike(nfa_broker *b, int32_t pix, double *cube, double *lnew);
void nfa_broker_callback(double *Cube, int *ndim, int *npars, double *lnew, void *ctx);
/* out[0] batches launched, out[1] evaluations served, out[2] largest batch */
int  nfa_broker_stats(nfa_broker *b, int64_t *out);

/* ---- cross-process transport for the broker --------------------
 * The reference runs one process per stripe (nestfit/main.py:516-523), each with its own
 * MultiNest (one instance per process) calling LogLike point by point
 * (cmultinest.pxd:27-28).  With a ring those processes never touch the GPU: each attaches to a
 * POSIX shared-memory ring (`name`), owns one slot, and nfa_ring_loglike / nfa_ring_callback
 * (MultiNest's LogLike signature; context = nfa_ring_client) post the point there and sleep
 * until the ONE serving process has evaluated it together with the other processes' points:
 * nfa_ring_serve = nfa_ring_poll -> nfa_runner_loglike_batch (up to 128 points: one launch;
 * up to 1024 through the batch kernels) -> nfa_ring_complete, until nfa_ring_stop, max_batches
 * (> 0) or idle_ms without a post.  A request that names a pixel the runner does not have fails
 * alone (NFA_ERR_ARG to its client); a device error stops the ring.
 * Results are bitwise those of nfa_runner_loglike_batch.  poll / complete are public so that a
 * server can put its own evaluator between them.  All entry points except nfa_ring_serve are
 * also exported by libnestfit_amd_ring.so, which has no HIP in it: the one library a sampler
 * process loads. */
typedef struct nfa_ring nfa_ring;
typedef struct { nfa_ring *ring; int32_t pix; } nfa_ring_client;
int  nfa_ring_create(nfa_ring **out, const char *name, int n_slots, int ndim);      /* server; one point per slot */
/* slots that hold up to max_points (<= 64) points each: for samplers that post several points per call */
int  nfa_ring_create_multi(nfa_ring **out, const char *name, int n_slots, int ndim, int max_points);
int  nfa_ring_attach(nfa_ring **out, const char *name, int wait_ms);                /* client: takes a slot */
int  nfa_ring_close(nfa_ring *r);            /* client: gives the slot back; server: removes the ring */
int  nfa_ring_stop(nfa_ring *r);             /* everybody leaves: blocked clients get NFA_ERR_STATE */
int  nfa_ring_ndim(const nfa_ring *r);
int  nfa_ring_slot(const nfa_ring *r);
int  nfa_ring_max_points(const nfa_ring *r);
/* blocking; NFA_ERR_STATE when the ring was stopped, its creator is gone, or no serving loop has been on it for 5 s */
int  nfa_ring_loglike(nfa_ring *r, int32_t pix, double *cube, double *lnew);
/* k points in one call (k <= max_points, all against pixel pix): cubes[k][ndim] in: unit cube, out: theta; lnew[k].
 * MultiNest asks for one point per call; a sampler whose next k proposals do not depend on each other's
 * likelihoods (uniform draws from the current bounding ellipsoid) posts them together and uses them in order */
int  nfa_ring_loglike_many(nfa_ring *r, int32_t pix, double *cubes, double *lnew, int k);
void nfa_ring_callback(double *Cube, int *ndim, int *npars, double *lnew, void *ctx);
/* slots[k], pix[k], U[k*ndim..]: row k of the *n gathered points (at most max_batch; the points of one
 * request are neighbouring rows with the same slot); returns when every attached client has posted, or
 * max_wait_us after the first post; *n = 0 after idle_ms without a post or when the ring was stopped
 * (*stopped).  nfa_ring_complete takes whole requests back, in one call or several. */
int  nfa_ring_poll(nfa_ring *r, int max_batch, int64_t max_wait_us, int idle_ms, int32_t *slots,
                   int32_t *pix, double *U, int *n, int *stopped);
int  nfa_ring_complete(nfa_ring *r, int n, const int32_t *slots, const double *U, const double *lnL, int rc);
int  nfa_ring_serve(nfa_ring *r, nfa_runner *run, int64_t max_wait_us, int64_t max_batches, int idle_ms);
/* The same service from a RESIDENT kernel (engine library only; one point per slot: rings made with nfa_ring_create).
 * The ring's mapping is registered with the runtime; the kernel's workgroups poll the slots themselves, claim a posted
 * point, run the point kernel's path and write theta, lnL and the DONE state into the slot the client spins on: a
 * LogLike call (mn_loglikelihood, nestfit/core/core.pyx:622-624) costs the path itself, no launch and no host thread.
 * Every kernel instance ends after lifetime_ms (0 = 20) or when the ring is stopped, and is launched again while there is
 * work; the call returns when the ring was stopped or nothing was served for idle_ms.  Bitwise nfa_runner_loglike_batch. */
int  nfa_ring_serve_device(nfa_ring *r, nfa_runner *run, int lifetime_ms, int idle_ms);
/* out[0] batches served, out[1] evaluations served, out[2] largest batch, out[3] clients attached */
int  nfa_ring_stats(nfa_ring *r, int64_t *out);
/* ---- device-resident batched nested sampler --------------------
 * Stand-in for one serial MultiNest run per pixel (run_multinest, nestfit/core/core.pyx:727-823,
 * pixel loop nestfit/main.py:452-469) when libmultinest is absent: all pixels' runs advance in
 * lock-step rounds with their state in HBM; a round = n_cand candidates per active pixel from
 * its bounding ellipsoid, one likelihood batch over all of them, one wave per pixel doing the
 * replace / evidence / stop / refit step.  pix[n_pix]: cube pixel of each run.  n_cand: candidates
 * per pixel and round at least; the number is raised (up to 16384) so that a round proposes about
 * batch_target candidates however few pixels are still running; only the proposals inside the
 * unit cube (the prior's support) are compacted and sent to the likelihood.  cap_iter: dead
 * point slots per pixel (a run stops when they are full).  free_mask[ndim] (NULL = all ones): unit-cube
 * slots the likelihood depends on; the others (constant or duplicated parameters) are not sampled --
 * integrating a uniform dummy dimension out exactly -- and stay at u = 0.5.  tol, efr, seed, maxiter as
 * run_multinest; upd = replacements between ellipsoid refits; log_zero replaces non-finite
 * likelihoods; check_every = rounds between two compactions of the active-pixel list.
 * Outputs are the raw material of what mn_dump stores (core.pyx:627-687): dead points with
 * their ln-weights, the final live points, iteration and evaluation counts; nestfit_amd/sampler.py
 * assembles the results from them and nestfit_amd/nested.py holds the bit-compatible host twin of the algorithm. */
typedef struct nfa_sampler nfa_sampler;
int nfa_sampler_create(nfa_sampler **out, nfa_runner *r, const int32_t *pix, int64_t n_pix, int nlive,
                       int n_cand, int64_t batch_target, int64_t cap_iter, const int32_t *free_mask);
int nfa_sampler_destroy(nfa_sampler *s);
/* Optional, between create and begin: pixels with numbers of live points of their own (the cube driver gives every
 * pixel nlive + int(5 SNR), nestfit/main.py:445-447) in ONE lock-step group: nlive[p] <= the nlive of
 * nfa_sampler_create (which is then the stride of the live arrays nfa_sampler_live returns: pixel p's points are
 * the first nlive[p] of its slice), cap[p] <= cap_iter dead-point slots, upd[p] replacements between refits. */
int nfa_sampler_set_pixel_nlive(nfa_sampler *s, const int32_t *nlive, const int64_t *cap, const int32_t *upd);
/* Optional, between create and begin: bounding ellipsoids per pixel at most -- MultiNest's `mmodal` / `maxModes`
 * (nestfit/core/core.pyx:727-760) as far as this sampler has them: 1 = one ellipsoid around all live points
 * (mmodal = False), 2..4 = clusters of live points get ellipsoids of their own where at most six dimensions are
 * sampled, 0 = the default (4 there, 1 above). */
int nfa_sampler_set_ellipsoids(nfa_sampler *s, int max_ellipsoids);
/* Free rejections of a one-ellipsoid bound (between create and begin).  Above six sampled dimensions no ellipsoid bounds
 * the live region of a fit well; but every superset of the region may veto a proposal before its likelihood is evaluated:
 * the bounding boxes of the live points in the unit cube's axes, in the ellipsoid's own frame and in n_frames fixed
 * rotations of it (-2: the default = 32 where the bound is sheared, none elsewhere; -1: none; 0..64).  margin: a face lies
 * beyond the extreme live point by margin * max(0.1 s, extreme - mean - 1.5 s), s the spread along its direction
 * (0: the default, 2.5).  MultiNest has no counterpart; `efr` keeps its meaning for the ellipsoid the proposals are drawn
 * from (nestfit/core/core.pyx:727-732). */
int nfa_sampler_set_boxes(nfa_sampler *s, int n_frames, double margin);
/* A volume-preserving shear in front of a one-ellipsoid bound (between create and begin).  The live region of a faint
 * pixel is a curved ridge (tex against ntot) that an ellipsoid holds badly.  The bound is therefore fitted AFTER the map
 * w_j = z_j - q_j(z_0 .. z_j-1), z = (u - mean) / spread, q_j the least-squares quadratic of the live points (squares and,
 * inside one velocity component, products of the earlier coordinates): an additive triangular map has a unit Jacobian, so
 * a point drawn uniformly in the w-ellipsoid and mapped back is uniform over its curved image in the unit cube.  Boxes, if
 * on, are fitted and tested in the w frame.  enlarge: the safety factor on the sheared ellipsoid's enclosing volume (>= 1;
 * 3 is the measured choice), 0 = off, < 0 = the default (engine option "sampler_shear_pct": 3 unless changed).  Applies
 * where all five free parameters of two or three components are sampled (10 or 15 dimensions); accepted and without effect
 * elsewhere.  MultiNest has no counterpart (its answer to curved regions is more ellipsoids: nestfit/core/core.pyx:727-760). */
int nfa_sampler_set_shear(nfa_sampler *s, double enlarge);
/* With the shear and the boxes on: every pair (i, j) of the sheared coordinates has the bounding ellipse of the live points'
 * projection onto (w_i, w_j) -- the covariance ellipse scaled to enclose them, its area times `enlarge` -- as one more free
 * veto: the region lies inside the cylinder over each of its projections.  enlarge >= 1 (2 is the measured choice), 0 = off,
 * < 0 = the default (engine option "sampler_pairs_pct", hundredths).  Between create and begin. */
int nfa_sampler_set_pairs(nfa_sampler *s, double enlarge);
/* After a run: every pixel's table of posterior samples in one copy (what MultiNest leaves in its post files and mn_dump
 * reads back, nestfit/core/core.pyx:627-687) -- rows [offsets[p], offsets[p+1]) of out[offsets[P]][ndim + 2] are pixel p's
 * dead points (min(n_iter[p], cap) of them) followed by its live points; a row = theta[ndim], -2 lnL, ln(prior mass x
 * likelihood): lnw + lnL of a dead point, lnL + live_off[p] of a live one (live_off[p] = -n_iter / nlive - ln nlive, given by
 * the caller, who normalises the last column into weights) -- or, with stats[P][6 + 4 ndim] given, the device does: the
 * last column comes back as weights exp(. - lnZ) and stats[p] = lnZ, lnZ of the dead points alone, information H, largest
 * lnL, largest lnL of the live points, sum of the weights, then weighted mean[ndim], weighted raw second moment[ndim],
 * theta of the largest likelihood[ndim], theta of the largest weight[ndim] (what mn_dump derives from MultiNest's files). */
int nfa_sampler_posterior_packed(nfa_sampler *s, const int64_t *offsets, const double *live_off, double *out, double *stats);
int nfa_sampler_run(nfa_sampler *s, double tol, double efr, int64_t seed, int64_t maxiter, int upd,
                    double log_zero, int check_every);
/* method: how a pixel finds its next point above the threshold.  0 = rejection sampling in the
 * bounding ellipsoid only; 1 = a pixel whose rejection round accepted fewer than 1 in 2 n_steps of
 * the evaluated candidates switches to constrained random walks: 64 walkers start from random live
 * points and take n_steps Metropolis steps inside {L > threshold}; a step is a scaled difference of
 * two random live points (differential evolution, ter Braak 2006), the scale tuned to an acceptance
 * of one half;
 * 2 = walks from the first round.  nfa_sampler_run uses method 1, n_steps 10 x sampled dimensions
 * (walks that are too short bias lnZ upwards: +0.13 with 40 steps in 10 dimensions, +0.014 with 120).
 * (nfa_sampler_run uses enlarge = 1.5: safety factor on the volume of the ellipsoid that just
 * encloses the live points, before MultiNest's floor X / efr is applied)
 * the same in two steps: begin = live points + first ellipsoids; advance = up to max_chunks groups
 * of check_every rounds (0 = to the end); *n_active = pixels still running (progress, time limits).
 * A pixel stops when its live points could add less than tol to lnZ, at maxiter iterations, when its dead-point slots
 * are full -- and when all its live points carry one lnL (a constant likelihood, or every draw non-finite and hence
 * log_zero): nothing can be proposed above such a threshold and the rest of the evidence is exactly L + ln X.  Such
 * a pixel is done before its first round (n_iter = 0) or after the replacement that made it so. */
int nfa_sampler_begin(nfa_sampler *s, double tol, double efr, int64_t seed, int64_t maxiter, int upd,
                      double log_zero, int check_every, double enlarge, int method, int n_steps);
int nfa_sampler_advance(nfa_sampler *s, int64_t max_chunks, int64_t *n_active);
int nfa_sampler_counts(nfa_sampler *s, int64_t *n_iter, int64_t *n_evals, int64_t *rounds);
/* The first n dead points of pixel p, in the order they died: theta[n][ndim], lnL[n], lnw[n] (ln of the prior mass each
 * carries), n <= min(n_iter[p], the pixel's dead-point slots).  Asking for more than a pixel holds is NFA_ERR_ARG here,
 * in nfa_sampler_dead_packed and in nfa_sampler_posterior_packed: the slots behind were never written. */
int nfa_sampler_dead(nfa_sampler *s, int64_t p, int64_t n, double *theta, double *lnL, double *lnw);
/* The same for all pixels in one call: offsets[P + 1] with offsets[0] = 0 and offsets[p + 1] - offsets[p] the
 * number of dead points wanted of pixel p (at most min(n_iter[p], cap_iter)); rows offsets[p] .. offsets[p + 1]
 * of theta[.][ndim], lnL[.], lnw[.] are pixel p's. */
int nfa_sampler_dead_packed(nfa_sampler *s, const int64_t *offsets, double *theta, double *lnL, double *lnw);
int nfa_sampler_live(nfa_sampler *s, double *theta, double *lnL);

/* ---- ensemble MCMC on the device: posteriors at a fixed component count -------------
 * The affine-invariant stretch move (Goodman & Weare 2010) of n_pix pixels in lock-step, in the unit cube, where the prior
 * is flat by construction: the target is L(theta(u)) on (0, 1)^D under every prior kind, model and likelihood option.
 *
 * Setting.  pix[n_pix] = cube pixel of each (NULL: all pixel 0, a one-pixel runner).  Each pixel has W = n_walkers walkers, W
 * even, W / 2 >= D + 1, W <= NFA_ENS_MAX_WALKERS, in the D sampled unit-cube slots (free_mask[ndim] as in nfa_sampler_create;
 * the other slots stay at u = 0.5).  A walker holds u[D], theta[ndim] (what the likelihood batch leaves in its row) and lnL;
 * nfa_ensemble_run turns a lnL that is not finite into log_zero.
 * One step is two half-steps, h = 0 then h = 1; in half-step h the walkers k of [h W/2, (h+1) W/2) move against the other half
 * as it stands.  For walker k in step s (from 1 in every nfa_ensemble_run call) of the pixel with cube index p, with
 * stream = ns_stream(seed, p, NFA_ENS_TAG + 2 s + h) and r_i = ns_uniform_of(stream, 3 k + i), the nested sampler's generator:
 *     partner   j = the other half's first walker + min(floor(r_0 W/2), W/2 - 1)
 *     stretch   z = ((a - 1) r_1 + 1)^2 / a                       (1 < a <= 16)
 *     proposal  y_d = u_j,d + z (u_k,d - u_j,d) for every sampled d  (f64, plain products and sums in that association)
 *     outside   any y_d not in (0, 1): rejected whatever its likelihood; its batch row carries the walker's own u, so every
 *               half-step evaluates the same n_pix W/2 rows and nothing between the launches of a run waits for the host
 *     accept    iff inside, lnL_y finite and log(r_2) < (D - 1) log(z) + (lnL_y - lnL_k), in that order: the walker takes y,
 *               the row's theta and its lnL.
 * Every lnL is bitwise what nfa_runner_loglike_batch returns for that (pixel, u).  Because the cube pixel is in the stream, a
 * pixel's run does not depend on the pixels it travels with.  Counters per pixel, of the last run: accepted, outside,
 * evaluated (W/2 per half-step, outside rows included: what was launched).
 * The state after step s is kept iff s > n_burn and (s - n_burn) % thin == 0; n_keep = (n_steps - n_burn) / thin; layout
 * chain_theta[n_pix][n_keep][W][ndim], chain_lnL[n_pix][n_keep][W], on the device until fetched.  After every step
 * trace[n_pix][n_steps][D + 1] holds the mean over the walkers of every sampled u and of lnL (lane l of a wave adds walkers
 * l, l + 64, ... in order, then a butterfly over the lanes: the same arguments give the same bits).
 *
 * nfa_ensemble_create evaluates the start rows u0 once (NFA_ERR_ARG: a u0 outside (0, 1) at a sampled slot, W odd, W / 2 <
 * D + 1, a pixel out of range).  nfa_ensemble_run may be called again and continues from the state; it numbers its steps from
 * 1, so a continuation needs another seed (20 steps are not two runs of 10 with one seed), and it replaces chain, trace and
 * counters.  NFA_ERR_ARG: a outside (1, 16], thin < 1, n_burn >= n_steps, n_keep < 1.  nfa_ensemble_state returns u as
 * [n_pix][W][ndim], 0.5 in the slots that are not sampled: a u0.  nfa_ensemble_summary reduces the chain on the device, per
 * parameter of theta over the N = n_keep W kept samples of a pixel: summary[n_pix][ndim][2] = mean and standard deviation
 * (divisor N) as moments of the differences from the pixel's best row, best[n_pix][ndim + 1] = theta and lnL of the row of
 * largest lnL (the first in (keep, walker) order on ties), quant[n_pix][ndim][n_levels] = s[i] + (s[i+1] - s[i]) g of the
 * sorted samples with h = (N - 1) q, i = floor(h), g = h - i (NFA_ERR_ARG: more than NFA_ENS_MAX_Q levels, a level outside
 * [0, 1], N > NFA_ENS_MAX_SORT with n_levels > 0; NFA_ERR_STATE before the first run).  nfa_ensemble_bytes: the device
 * bytes of an ensemble and its run (a caller cuts a cube into groups of pixels with it).  All buffers belong to the
 * nfa_ensemble and go with it; it uses its runner, which must outlive it, one call at a time. */
#define NFA_ENS_MAX_WALKERS 512
#define NFA_ENS_MAX_Q       8
#define NFA_ENS_MAX_SORT    8192
typedef struct nfa_ensemble nfa_ensemble;
int nfa_ensemble_create(nfa_ensemble **out, nfa_runner *r, const int32_t *pix, int64_t n_pix, int n_walkers,
                        const int32_t *free_mask /* [ndim] or NULL */, const double *u0 /* [n_pix][n_walkers][ndim], in (0,1) */);
int nfa_ensemble_destroy(nfa_ensemble *e);
int nfa_ensemble_run(nfa_ensemble *e, int64_t n_steps, int64_t n_burn, int64_t thin, double a, int64_t seed, double log_zero);
int nfa_ensemble_counts(nfa_ensemble *e, int64_t *accepted, int64_t *outside, int64_t *evaluated);   /* [n_pix] each */
int nfa_ensemble_state(nfa_ensemble *e, double *u, double *theta, double *lnL);                        /* the walkers as they stand */
int nfa_ensemble_trace(nfa_ensemble *e, double *trace);
int nfa_ensemble_chain(nfa_ensemble *e, double *theta, double *lnL);                                   /* either may be NULL */
int nfa_ensemble_chain_dev(nfa_ensemble *e, const double **d_theta, const double **d_lnL, int64_t *n_keep);
int nfa_ensemble_summary(nfa_ensemble *e, const double *levels, int n_levels, double *summary, double *best, double *quant);
int64_t nfa_ensemble_bytes(int64_t n_pix, int n_walkers, int ndim, int n_sampled, int64_t n_steps, int64_t n_keep);

/* The products of the last run's chain, reduced where it lies; N = n_keep W samples per pixel in (keep,
 * walker) order.  Each takes the runner's lock, waits for its lanes and works on lane 0 like nfa_ensemble_summary; NFA_ERR_STATE
 * before the first run; a failure leaves runner and ensemble usable; the same arguments give the same bits.
 * nfa_ensemble_histogram bins column c of every pixel on edges[c][0 .. n_bins], strictly increasing and finite, 1 <= n_bins <=
 * NFA_ENS_MAX_BINS (else NFA_ERR_ARG): bin b counts edges[b] <= x < edges[b + 1], the last bin x == edges[n_bins] too; a NaN,
 * an x < edges[0] and an x > edges[n_bins] are counted in outside[p][c] and in no bin -- np.histogram(x, bins=edges[c])[0].
 * nfa_ensemble_covariance: about the pixel's best row b (nfa_ensemble_summary's), d_i,a = x_i,a - x_b,a, S_a = sum d_i,a,
 * S_ab = sum d_i,a d_i,b: cov_ab = S_ab / N - (S_a / N)(S_b / N), the diagonal not below 0, computed for a <= b and mirrored; a
 * slot that is not sampled has an exact zero row and column.
 * nfa_ensemble_moments is nfa_runner_predict_moments with n_seg = n_pix, seg_pix the ensemble's pixels, seg_off[g] = g N, theta
 * the chain and no weights, bit for bit (one function behind both), the chain read where it lies and left as it is.
 * nfa_ensemble_moments_bytes: the runner scratch that call holds per pixel, beside nfa_ensemble_bytes; histogram and
 * covariance hold a fixed scratch for the length of the call, whatever n_pix. */
#define NFA_ENS_MAX_BINS 1024
int nfa_ensemble_histogram(nfa_ensemble *e, const double *edges /* [ndim][n_bins + 1] */, int n_bins,
                           int64_t *counts /* [n_pix][ndim][n_bins] */, int64_t *outside /* [n_pix][ndim] or NULL */);
int nfa_ensemble_covariance(nfa_ensemble *e, double *cov /* [n_pix][ndim][ndim] */);
int nfa_ensemble_moments(nfa_ensemble *e, int64_t chunk_rows /* as nfa_runner_predict_moments */,
                         double *spec_mean, double *spec_std, double *stat_mean, double *stat_std);
int64_t nfa_ensemble_moments_bytes(int64_t n_pix, int64_t chan_tot, int n_spec);

/* ---- tempered ensembles: evidences and multimodal posteriors --------------------------
 * A tempered ensemble is an nfa_ensemble with n_temps = T rungs per pixel, 2 <= T <= NFA_ENS_MAX_TEMPS, at the inverse
 * temperatures betas[T]: betas[0] == 1, strictly decreasing, finite, betas[T - 1] >= 0 (else NFA_ERR_ARG); every (pixel, rung)
 * has W walkers under the rules above; u0 is [n_pix][T][W][ndim].  Rung t moves by the move above against L^beta_t:
 *     stream   ns_stream(seed, p, NFA_ENS_TAG + t 2^48 + 2 s + h)
 *     accept   iff inside, lnL_y finite and log(r_2) < (D - 1) log(z) + beta_t (lnL_y - lnL_k), the product formed last in plain
 *              f64; beta_0 = 1 multiplies exactly, so rung 0 of a run that never swaps has the bits of the untempered run with
 *              the same arguments.  Outside proposals and a lnL_y that is not finite are rejected at every beta, 0 included.
 * After the two half-steps of step s, if swap_every > 0 and s % swap_every == 0, with n the number of swap sweeps before in
 * this run, the pairs (t, t + 1) with t % 2 == n % 2 exchange: walker k of rung t and walker k of rung t + 1 swap u, theta and
 * lnL iff log(r) < (beta_t - beta_t+1)(lnL_t+1,k - lnL_t,k), r = ns_uniform_of(ns_stream(seed, p, NFA_ENS_TAG + 2^60 + t 2^48 +
 * s), k).  With n_steps <= 2^40 and t < 32 every tag lies in [2^61, 2^62) and the move tags below the swap tags.  Swaps come
 * before the trace and the keep of the step.
 * Kept: the theta chain of rung 0 only, in the layout above, so nfa_ensemble_summary, _histogram, _covariance, _moments, _chain,
 * _chain_dev, _counts, _state and _trace of a tempered ensemble describe the cold chain with the shapes of an untempered one;
 * lnL of every rung, [n_pix][T][n_keep][W]; the trace of every rung, [n_pix][T][n_steps][D + 1]; counters of the last run per
 * (pixel, rung) and per (pixel, pair (t, t + 1)): swaps accepted, swaps proposed (W per sweep the pair is active in).
 * nfa_ensemble_rung_state returns u as [n_pix][T][W][ndim]: a u0.
 * nfa_ensemble_evidence reduces the kept lnL on the device per (pixel, rung t, set j): set 0 is all n_keep kept steps, sets
 * 1 .. n_blocks are contiguous blocks of floor(n_keep / n_blocks) kept steps, 1 <= n_blocks <= NFA_ENS_MAX_BLOCKS, n_blocks <=
 * n_keep (else NFA_ERR_ARG).  With x_i the n values of the set: out[n_pix][T][n_blocks + 1][3] =
 *     mean = x_first + S1 / n,  var = max(S2 / n - (S1 / n)^2, 0)        (S1, S2: sums of x_i - x_first and of its square)
 *     r    = delta M + log(sum exp(delta (x_i - M)) / n),  delta = beta_t-1 - beta_t,  M = max x_i;  r = 0 for t = 0
 * the sums in a fixed shape (strided per thread, a butterfly per wave, the waves in order): the same arguments give the same
 * bits.  With betas[T - 1] == 0 the sum over t of r is ln Z, by the stepping-stone identity Z_beta_t-1 / Z_beta_t =
 * E_beta_t[L^delta] and Z(0) = 1 in the unit cube.  NFA_ERR_STATE before a run; NFA_ERR_ARG on an untempered ensemble, as for
 * every nfa_ensemble_rung_* call.  A failure leaves runner and ensemble usable. */
#define NFA_ENS_MAX_TEMPS  32
#define NFA_ENS_MAX_BLOCKS 16
int nfa_ensemble_create_tempered(nfa_ensemble **out, nfa_runner *r, const int32_t *pix, int64_t n_pix, int n_walkers,
                                 const double *betas /* [n_temps] */, int n_temps, int64_t swap_every /* 0: never */,
                                 const int32_t *free_mask, const double *u0 /* [n_pix][n_temps][n_walkers][ndim] */);
int nfa_ensemble_rung_counts(nfa_ensemble *e, int64_t *accepted, int64_t *outside, int64_t *evaluated /* [n_pix][T] each */,
                             int64_t *swaps_accepted, int64_t *swaps_proposed /* [n_pix][T - 1] each */);
int nfa_ensemble_rung_state(nfa_ensemble *e, double *u, double *theta, double *lnL);                   /* any may be NULL */
int nfa_ensemble_rung_trace(nfa_ensemble *e, double *trace);
int nfa_ensemble_rung_lnl(nfa_ensemble *e, double *lnL);
int nfa_ensemble_evidence(nfa_ensemble *e, int n_blocks, double *out /* [n_pix][T][n_blocks + 1][3] */);
int64_t nfa_ensemble_tempered_bytes(int64_t n_pix, int n_walkers, int n_temps, int ndim, int n_sampled, int64_t n_steps,
                                    int64_t n_keep);

/* ---- the exchange step of a sharded cube fit ---------------------
 * The reference stripes pixels over processes, (lon_ix[i::nproc], lat_ix[i::nproc])
 * (nestfit/main.py:565-571), and exchanges nothing while sampling; its processes meet through chunk
 * files (main.py:516-523, docs/store_spec.rst:12-32).  One process per GPU here; these entry points
 * are the end-of-run exchange: RCCL over xGMI (librccl.so, opened at run time).  Rank 0 calls
 * nfa_comm_unique_id and the host carries the 128 bytes to the other ranks; every rank then calls
 * nfa_comm_create (after nfa_set_device).  All buffers are host memory; calls are blocking.
 * op: 0 sum, 2 max, 3 min. */
typedef struct nfa_comm nfa_comm;
int nfa_comm_unique_id(unsigned char *id128);
int nfa_comm_create(nfa_comm **out, const unsigned char *id128, int rank, int world);
int nfa_comm_destroy(nfa_comm *c);
int nfa_comm_rank(const nfa_comm *c);
int nfa_comm_world(const nfa_comm *c);
int nfa_comm_allgather(nfa_comm *c, const double *send, int64_t count, double *recv /* [world][count] */);
int nfa_comm_allreduce(nfa_comm *c, double *values, int64_t count, int op);
int nfa_comm_barrier(nfa_comm *c);

/* ---- device memory + events (for harnesses that keep inputs in HBM) ------- */
int nfa_malloc(void **dptr, int64_t bytes);
int nfa_free(void *dptr);
int nfa_memcpy_h2d(void *dst, const void *src, int64_t bytes);
int nfa_memcpy_d2h(void *dst, const void *src, int64_t bytes);
int nfa_memcpy_d2d(void *dst, const void *src, int64_t bytes);
int nfa_event_create(void **ev);
int nfa_event_destroy(void *ev);
int nfa_event_record(void *ev, nfa_runner *r);       /* on the runner's stream */
int nfa_event_synchronize(void *ev);
int nfa_event_elapsed_ms(void *start, void *stop, float *ms);

#ifdef __cplusplus
}
#endif
#endif /* NESTFIT_AMD_H */
