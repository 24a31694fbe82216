// nfa_line_window.h -- the two quotients whose floor() are the ends of a hyperfine line's channel window
// (reference: nestfit/models/hyperfine.pyx:75-79), in the reference's sequence and in a short form that the table mode's
// line set-up takes where it can prove the same integers.  Plain C++ for host and device: the likelihood kernels include it
// (nfa_device.h: nf_line), and tests/test_row_heads.py compiles it alone, on a machine without a GPU.
// Compile with -ffp-contract=off: every operation below rounds once, as written.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define NFA_HD __host__ __device__ __forceinline__
#else
#define NFA_HD inline
#endif

// RN(a / nu_chan) for both ends: with r = RN(1 / nu_chan), q = a r, e = a - nu_chan q (exact, fused), q + e r is the correctly
// rounded quotient (Markstein's final step; r_chan == 0: the host found nu_chan's mantissa all ones, take the division)
NFA_HD void nf_window_quot(double nu_lo, double nu_hi, double nu_chan, double r_chan, double &q_lo, double &q_hi) {
    if (r_chan != 0.0) {
        const double ql = nu_lo * r_chan, qh = nu_hi * r_chan;
        q_lo = __builtin_fma(__builtin_fma(-nu_chan, ql, nu_lo), r_chan, ql);
        q_hi = __builtin_fma(__builtin_fma(-nu_chan, qh, nu_hi), r_chan, qh);
    } else {
        q_lo = nu_lo / nu_chan;
        q_hi = nu_hi / nu_chan;
    }
}

// The reference's sequence: nu_cutoff = sqrt(12.5 / hf_idenom) (hyperfine.pyx:76), a = hf_nucen - nu_min
NFA_HD void nf_window_quot_ref(double a, double hf_idenom, double nu_chan, double r_chan, double &q_lo, double &q_hi) {
    const double nu_cutoff = sqrt(12.5 / hf_idenom);
    nf_window_quot(a - nu_cutoff, a + nu_cutoff, nu_chan, r_chan, q_lo, q_hi);
}

// The short form: the cut-off is 5 |w| in exact arithmetic (hf_idenom = 0.5 / w^2, w = hf_width), so c = RN(5 |w|) stands in
// for the reference's division and square root -- and the caller may use floor() of these quotients only where this returns
// true, which says that the reference's quotients have the same floor()s.  Why, with u = 2^-53 and every |e| <= u:
//   reference  p = w^2 (1 + e1),  i = 0.5 / p (1 + e2),  12.5 / i (1 + e3) = 25 w^2 (1 + e1)(1 + e3) / (1 + e2),  and its root
//              c_r = 5 |w| sqrt((1 + e1)(1 + e3) / (1 + e2)) (1 + e4) = 5 |w| (1 + d_r),  |d_r| < 2.6 u
//              (w in [1e-100, 1e100]: no intermediate leaves the normal range; any other w returns false);
//   here       c = 5 |w| (1 + d_c), |d_c| <= u, so |c_r - c| < 3.7 u c;
//   the ends   RN(a -+ c_r) and RN(a -+ c) differ by at most |c_r - c| + u (|one| + |other|);
//   quotients  Q = RN(end / nu_chan), correctly rounded in both sequences: |Q_r - Q| <= |end_r - end| / nu_chan + u (|Q_r| + |Q|).
// With m >= max(|Q_lo|, |Q_hi|) of THIS sequence (the code takes |Q_lo| + |Q_hi|): c / nu_chan = (end_hi - end_lo) / (2 nu_chan) <= m (1 + 3 u) and |end| / nu_chan
// <= m (1 + u), hence |Q_r - Q| < (3.7 + 2 + 2) u m + O(u^2 m) < 8 u m.  The guard is G = 2^-49 (m + 1) = 16 u (m + 1): twice the
// bound, plus an absolute 16 u for the roundings of the fraction below (f = Q - floor(Q) is exact for Q >= 0 and off by at most
// u for Q < 0; f - 0.5 by at most u / 4).  If G < f < 1 - G for both quotients, Q_r lies strictly inside (floor(Q), floor(Q) + 1)
// like Q: the same floor().  A quotient that is not finite, or so large that G >= 0.5, fails the test (NaN compares false).
// About 2 m 2^-48 of all lines fail it -- m < 2^13: one in 10^10.
NFA_HD bool nf_window_quot_short(double a, double hf_width, double nu_chan, double r_chan, double &q_lo, double &q_hi) {
    const double aw = fabs(hf_width), c = 5.0 * aw;
    nf_window_quot(a - c, a + c, nu_chan, r_chan, q_lo, q_hi);
    const double m1 = (fabs(q_lo) + fabs(q_hi)) + 1.0;                   // (the sum for the larger of the two: two additions)
    const double t = __builtin_fma(m1, -0x1p-49, 0.5);                   // 0.5 - G
    const double f_lo = q_lo - floor(q_lo), f_hi = q_hi - floor(q_hi);
    // (no short-circuit: four compares and three ANDs of lane masks, not a branch per condition)
    return (bool)((int)(fabs(f_lo - 0.5) < t) & (int)(fabs(f_hi - 0.5) < t) & (int)(aw > 1e-100) & (int)(aw < 1e100));
}
