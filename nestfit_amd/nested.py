"""The numpy twin of the device sampler (csrc/nfa_sampler.h): the same algorithm on the host for any likelihood callable,
the same counter-based random stream and the same decisions, so that the same seed gives the same run.  It is the
device's specification: the GPU sampler tests assert "device = twin, decision for decision".  One state (`TwinState`,
fields named like `NsDev`'s) and one function per stage of the device: `_begin` (nfa_sampler_begin + ns_init_live_kernel),
`_refit` (ns_refit / ns_refit_multi / ns_shear_fit), `_propose` (ns_propose_one), `_update_reject`, `_walk_step` and
`_replace` (the scan branch, the walk branch and the replacement of ns_update_kernel), `_plateau` (ns_plateau_kernel and the same test after a replacement), `_chunk_kr` (ns_chunk_kr);
`run_nested` is the loop over rounds around them.  `nestfit_amd.sampler` imports from here, never the other way round."""
import math
import types

import numpy as np

LOG_ZERO = -1e100

# ---- the constants shared with the device: csrc/nfa_sampler_plan.h's NS_X is _NS_X here (tests/test_sampler_plan.py
# compares every one of them with the header's, exactly)
_U64 = np.uint64
_NS_TAG_LIVE = _U64(1 << 62)                                    # the stream of the first live points
# stream slots of a proposal: a walker's starting live point, which ellipsoid, the 1 / (number that hold it) test, the radius
_NS_B_START, _NS_B_ELL, _NS_B_KEEP, _NS_B_RADIUS = _U64(250), _U64(253), _U64(254), _U64(255)
_NS_FRAME_SEED = _U64(0x5EEDF00D)
_NS_WALK_TARGET = 0.5                                           # acceptance the walk scale is tuned to
_NS_ME_GAIN = 0.7                                               # a cut stays when the halves have less than this of the volume
_NS_MARGIN_A, _NS_MARGIN_FLOOR = 1.5, 0.1                       # a box face beyond the extreme live point (`_fit_boxes`)
_NS_SHEAR_RIDGE, _NS_SHEAR_PIVOT = 1e-6, 1e-9                   # `_fit_shear`: on the Gram diagonal; a pivot that is dropped
# the policy defaults and limits of `_plan`
_NS_ME, _NS_ME_MAXD, _NS_STAGE_BYTES = 4, 6, 96 * 1024
_NS_FRAMES, _NS_MARGIN_C = 32, 2.5                                  # (margin, round 4: 1.75 = precision='speed')
_NS_SHEAR_ENLARGE, _NS_SHEAR_MMAX, _NS_PAIRS_ENLARGE = 3.0, 64, 2.0     # (round 4: 2.5 and 1.75 = precision='speed')
_NS_RATIO_MAX, _NS_KMAX, _NS_KP_START, _NS_K_TARGET, _NS_REFIT_EVERY = 32, 65536, 256, 16, 4
_NS_WALK_LOWD, _NS_WALK_FACTOR_LOWD, _NS_WALK_FACTOR = 6, 64, 2
# literals the kernels hold inline (no NS_ name on the device): the stream slots of a walk step's two partners, the
# differential-evolution scale 2.38 / sqrt(2 D), the largest share of proposals a pixel asks for, and how far above the
# switch to walks (1 in walk_factor n_steps) a bound must promise before a pixel goes back to rejection
_B_PARTNER_A, _B_PARTNER_B = _U64(251), _U64(252)
_DE_GAMMA, _KP_MAX, _WALK_BACK = 2.38, 1 << 20, 8.0


class NestedResult:
    """Per-pixel outcome, named like the quantities MultiNest hands to ``mn_dump``."""

    def __init__(self, posterior, lnZ, lnZ_err, max_loglike, n_live, n_evals, n_iter, information):
        self.posterior = posterior                  # (n_samples, n_params + 2)
        self.n_samples = int(posterior.shape[0])
        self.n_params = int(posterior.shape[1] - 2)
        self.lnZ = float(lnZ)
        self.lnZ_err = float(lnZ_err)
        self.max_loglike = float(max_loglike)
        self.n_live = int(n_live)
        self.n_evals = int(n_evals)
        self.n_iter = int(n_iter)
        self.information = float(information)
        # True when the run was stopped by its iteration / dead-point cap before the evidence tolerance was
        # met: lnZ is then the evidence collected so far plus the live points' share, a lower-quality
        # estimate (set by run_nested / run_nested_device)
        self.truncated = False
        w = posterior[:, -1]
        th = posterior[:, :-2]
        best = th[np.argmin(posterior[:, -2])]      # max likelihood
        mapp = th[np.argmax(w)]                     # largest posterior mass
        # the weighted moments about the row of the largest weight, a point inside the posterior's bulk (raw second moments
        # cancel where |mean| >> sigma); one (n_samples, n_params) temporary, like the device's ns_finish_kernel
        d = th - mapp
        m1 = w @ d
        d *= d
        mean = m1 + mapp * w.sum()
        self.param_constr = np.stack([mean, np.sqrt(_var_about(w @ d, mean, mapp, w.sum())), best, mapp])    # (4, n_params)

    @classmethod
    def from_stats(cls, posterior, stats, n_live, n_evals, n_iter):
        """The same result from what the device has already formed of the table (nfa_sampler_posterior_packed with `stats`:
        lnZ, lnZ of the dead points, H, largest lnL, largest live lnL, sum of the weights, mean, second moment about the row of
        the largest weight, theta of the largest likelihood, theta of the largest weight): no pass over the table on the host."""
        self = cls.__new__(cls)
        nd = int(posterior.shape[1] - 2)
        self.posterior = posterior
        self.n_samples = int(posterior.shape[0])
        self.n_params = nd
        self.lnZ = float(stats[0])
        self.information = float(stats[2])
        self.lnZ_err = float(np.sqrt(max(self.information, 0.0) / n_live))
        self.max_loglike = float(stats[3])
        self.n_live, self.n_evals, self.n_iter = int(n_live), int(n_evals), int(n_iter)
        self.truncated = False
        mean, m2, mapp = stats[6:6 + nd], stats[6 + nd:6 + 2 * nd], stats[6 + 3 * nd:6 + 4 * nd]      # (m2: about the row of the largest weight)
        self.param_constr = np.stack([mean, np.sqrt(_var_about(m2, mean, mapp, stats[5])), stats[6 + 2 * nd:6 + 3 * nd], mapp])
        return self


def _var_about(s2, mean, c, wsum):
    """sum w (t - mean)^2 from s2 = sum w (t - c)^2, mean = sum w t and wsum = sum w (the weights add up to one to rounding)."""
    delta = mean - c
    return np.maximum(s2 - 2.0 * delta * (mean - c * wsum) + delta * delta * wsum, 0.0)


# ---- counter-based random numbers, shared bit for bit with csrc/nfa_sampler.h -------------
def _mix(x):
    """splitmix64 finaliser on uint64 arrays (wrap-around arithmetic)."""
    with np.errstate(over='ignore'):
        x = x + _U64(0x9E3779B97F4A7C15)
        z = x
        z = (z ^ (z >> _U64(30))) * _U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U64(27))) * _U64(0x94D049BB133111EB)
        return z ^ (z >> _U64(31))


def _uniform(seed, p, a, b):
    """Uniform in (0, 1): a pure function of (seed, pixel, a, b) (ns_uniform on the device)."""
    with np.errstate(over='ignore'):
        h = _mix(_mix(_mix(_mix(np.asarray(seed, dtype=_U64)) + np.asarray(p, dtype=_U64))
                      + np.asarray(a, dtype=_U64)) + np.asarray(b, dtype=_U64))
    return ((h >> _U64(11)).astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)


def _walkers_for(n):
    """Walkers of a pixel with n live points (ns_walkers_for): 64, 128 from 384 live points, 256 from 768."""
    return 256 if n >= 768 else 128 if n >= 384 else 64


def _ball_points(seed, p, a, D):
    """Uniform points of the unit D-ball for stream indices a[K] of pixel p (the Box-Muller and
    radius draws of ns_propose_one)."""
    a = np.asarray(a, dtype=_U64)
    z = np.empty((a.size, D))
    for m in range(0, D, 2):
        u1 = _uniform(seed, p, a, _U64(m))
        u2 = _uniform(seed, p, a, _U64(m + 1))
        r = np.sqrt(-2.0 * np.log(u1))
        ang = 6.283185307179586 * u2
        z[:, m] = r * np.cos(ang)
        if m + 1 < D:
            z[:, m + 1] = r * np.sin(ang)
    ur = _uniform(seed, p, a, _NS_B_RADIUS)
    return z * (np.exp(np.log(ur) / D) / np.sqrt((z * z).sum(axis=1)))[:, None]


def _fit_ellipsoids(U, efr, ln_x, enlarge=1.0):
    """Bounding ellipsoid of one pixel's live points U[nlive, ndim] (ns_refit): centre c and lower-triangular
    A with {c + A z : |z| <= 1}: the covariance ellipsoid scaled until it encloses every live point,
    its volume times the safety factor `enlarge`, and, MultiNest's rule (Feroz et al. 2009, sec. 5.1.1), enlarged until its volume is at least
    the expected prior volume over the target efficiency, X / efr, with ln X = ln_x.  Returns c, A, use_cube, ln volume."""
    nlive, ndim = U.shape
    c = U.sum(axis=0) / nlive
    d = U - c
    cov = np.einsum('ni,nj->ij', d, d) / (nlive - 1)
    cov = cov + (1e-12 * np.maximum(np.trace(cov), 1e-30)) * np.eye(ndim)
    L = np.linalg.cholesky(cov)
    y = np.linalg.solve(L, d.T)                                # (ndim, nlive)
    r2 = np.max(np.sum(y * y, axis=0))                         # largest Mahalanobis distance^2
    ln_vball = 0.5 * ndim * np.log(np.pi) - math.lgamma(0.5 * ndim + 1.0)
    lnv = ln_vball + 0.5 * ndim * np.log(r2) + np.log(np.diagonal(L)).sum() + math.log(enlarge)
    grow = np.maximum((ln_x - np.log(efr)) - lnv, 0.0)
    scale = np.sqrt(r2) * np.exp((grow + math.log(enlarge)) / ndim)
    lnv = lnv + grow
    # ln volume against ln 1 of the unit cube: a larger ellipsoid is no better than the prior itself
    return c, L * scale, lnv >= 0.0, lnv


# ---- several ellipsoids per pixel (ns_refit_multi / the several-ellipsoids draw of ns_propose_one) ----------

def _me_fit(Y, enlarge):
    """Mean, Cholesky factor, covariance, largest Mahalanobis distance^2, ln volume (safety factor included) and size
    of a cluster of live points Y[n, d] (ns_me_fit)."""
    n, d = Y.shape
    c = Y.sum(axis=0) / n
    dl = Y - c
    cov = dl.T @ dl / (n - 1)
    Lc = np.linalg.cholesky(cov + 1e-12 * max(float(np.trace(cov)), 1e-30) * np.eye(d))
    y = np.linalg.solve(Lc, dl.T)
    r2 = float(np.max(np.sum(y * y, axis=0)))
    ln_vball = 0.5 * d * math.log(math.pi) - math.lgamma(0.5 * d + 1.0)
    lnv = ln_vball + 0.5 * d * math.log(r2) + float(np.log(np.diag(Lc)).sum()) + math.log(enlarge)
    return c, Lc, cov, r2, lnv, n


def _fit_multi(U, efr, ln_x, enlarge=1.0, max_ell=4):
    """The bound of one pixel's live points U[nlive, d] as up to four ellipsoids (ns_refit_multi): the cluster with the
    largest ellipsoid is cut across its principal axis at its centre; the cut stays when the halves' ellipsoids together
    have less than 0.7 of its volume, else the cluster is final.  Then MultiNest's rule on the summed volume.
    Returns centres [4, d], axes [4, d, d], ln volumes [4], the number in use, ln of the summed volume, use_cube."""
    n, d = U.shape
    minp = 2 * (d + 2)
    lab = np.zeros(n, dtype=np.int64)
    fits, final = [_me_fit(U, enlarge)], [False]
    while len(fits) < max_ell:
        best = -1
        for k, f in enumerate(fits):
            if not final[k] and f[5] >= 2 * minp and (best < 0 or f[4] > fits[best][4]):
                best = k
        if best < 0:
            break
        c, _, cov, _, lnv, _ = fits[best]
        v = np.ones(d)
        for _ in range(20):                                      # power iteration from (1, ..., 1)
            w = cov @ v
            v = w * (1.0 / math.sqrt(float((w * w).sum())))
        idx = np.flatnonzero(lab == best)
        side = ((U[idx] - c) @ v) >= 0.0
        ia, ib = idx[~side], idx[side]
        if ia.size < minp or ib.size < minp:
            final[best] = True
            continue
        fa, fb = _me_fit(U[ia], enlarge), _me_fit(U[ib], enlarge)
        if np.logaddexp(fa[4], fb[4]) < lnv + math.log(_NS_ME_GAIN):
            lab[ib] = len(fits)
            fits[best] = fa
            fits.append(fb)
            final[best] = False
            final.append(False)
        else:
            final[best] = True
    tot = -np.inf
    for f in fits:
        tot = np.logaddexp(tot, f[4])
    grow = max((ln_x - math.log(efr)) - tot, 0.0)
    cs, As, lv = np.zeros((_NS_ME, d)), np.zeros((_NS_ME, d, d)), np.full(_NS_ME, -np.inf)
    for k, (c, Lc, _, r2, lnv, _) in enumerate(fits):
        cs[k], As[k], lv[k] = c, Lc * (math.sqrt(r2) * math.exp((grow + math.log(enlarge)) / d)), lnv + grow
    return cs, As, lv, len(fits), tot + grow, (tot + grow) >= 0.0


def _candidates_multi(seed, p, a, cs, As, lv, ne, lnvol):
    """The candidates of stream indices a[K] of pixel p, uniform over the union of its `ne` ellipsoids: one is drawn by
    volume, and a point that lies in q of them is kept with probability 1 / q.  Returns the points and the keep flags."""
    usel = _uniform(seed, p, a, _NS_B_ELL)
    cum = np.cumsum(np.exp(lv[:ne - 1] - lnvol))
    ke = np.searchsorted(cum, usel, side='right')
    z = _ball_points(seed, p, a, cs.shape[1])
    cand = cs[ke] + np.einsum('kji,ki->kj', As[ke], z)
    q = np.ones(a.size, dtype=np.int64)
    for k in range(ne):
        y = np.linalg.solve(As[k], (cand - cs[k]).T)
        q += ((np.sum(y * y, axis=0) <= 1.0) & (ke != k)).astype(np.int64)
    keep = (q == 1) | (_uniform(seed, p, a, _NS_B_KEEP) * q < 1.0)
    return cand, keep


# ---- free rejections: boxes around the live points in several frames (ns_refit / ns_propose_kernel) ---------------
# Above six sampled dimensions no ellipsoid bounds the live region well (a two-component fit: its ten-dimensional live set
# is box-like in some directions, curved in others), and a proposal uniform in the bounding ellipsoid is rarely inside
# the region.  But every superset of the region may veto a proposal BEFORE its likelihood is evaluated, and what is left
# is still uniform over the intersection: the axis-aligned bounding box of the live points in the unit cube, their
# bounding box in the ellipsoid's own (Cholesky) frame, and their bounding boxes in `n_frames` fixed rotations of that
# frame.  A face sits beyond the extreme live point by c max(0.1 s, extreme - mean - 1.5 s), s the standard deviation
# along that direction: a marginal that ends abruptly (a flat, box-like direction: extreme near 1.7 s) gets a margin of
# a quarter of s, one that thins out (the projection of a round body: extreme near 2.9 s) one and a half s -- what the
# spacing of the extreme order statistics would give (scripts/proto_intersection.py: the fraction of the true region a
# bound cuts off, and the evaluations per iteration it saves).
def _frames(D, K):
    """K fixed orthogonal D x D matrices (ns_make_frames): entries 2 u - 1 from the counter-based stream, columns
    orthonormalised one after the other (modified Gram-Schmidt).  Column b of frame k is the direction of coordinate b."""
    Q = np.zeros((K, D, D))
    for k in range(K):
        M = 2.0 * _uniform(_NS_FRAME_SEED,_U64(k + 1), np.arange(D, dtype=_U64)[:, None], np.arange(D, dtype=_U64)[None, :]) - 1.0
        for b in range(D):
            v = M[:, b].copy()
            for q in range(b):
                dot = 0.0
                for a in range(D):
                    dot += Q[k, a, q] * v[a]
                v -= dot * Q[k, :, q]
            n2 = 0.0
            for a in range(D):
                n2 += v[a] * v[a]
            Q[k, :, b] = v / math.sqrt(n2)
    return Q


def _fit_boxes(U, c, A, frames, margin_c):
    """The boxes of one pixel (ns_refit's last part): `ubox` [D, 2] around U[n, D] in the unit cube's own axes, `fbox`
    [K + 1, D, 2] around zz = A^-1 (u - c) in the Cholesky frame (k = 0) and in frame k's rotation of it."""
    n, D = U.shape
    d = U - c
    cov_diag = np.einsum('ni,ni->i', d, d) / (n - 1)
    sg = np.sqrt(cov_diag)
    lo, hi = d.min(axis=0), d.max(axis=0)
    ubox = np.stack([c + lo - margin_c * np.maximum(_NS_MARGIN_FLOOR * sg, -lo - _NS_MARGIN_A * sg),
                     c + hi + margin_c * np.maximum(_NS_MARGIN_FLOOR * sg, hi - _NS_MARGIN_A * sg)], axis=1)
    zz = np.linalg.solve(A, d.T).T                                     # [n, D]; every direction of it has the same spread:
    sz = math.sqrt(float((zz * zz).sum()) / ((n - 1) * D))              # sqrt(trace of its covariance / D)
    K = frames.shape[0]
    fbox = np.empty((K + 1, D, 2))
    for k in range(K + 1):
        W = zz if k == 0 else zz @ frames[k - 1]
        wlo, whi = W.min(axis=0), W.max(axis=0)
        fbox[k, :, 0] = wlo - margin_c * np.maximum(_NS_MARGIN_FLOOR * sz, -wlo - _NS_MARGIN_A * sz)
        fbox[k, :, 1] = whi + margin_c * np.maximum(_NS_MARGIN_FLOOR * sz, whi - _NS_MARGIN_A * sz)
    return ubox, fbox


def _box_veto(cand, zz, ubox, fbox, frames):
    """Flags of the proposals cand[K, D] (zz[K, D] = their coordinates in the Cholesky frame) that lie inside every box."""
    ok = np.all((cand >= ubox[:, 0]) & (cand <= ubox[:, 1]), axis=1)
    for k in range(fbox.shape[0]):
        W = zz if k == 0 else zz @ frames[k - 1]
        ok &= np.all((W >= fbox[k, :, 0]) & (W <= fbox[k, :, 1]), axis=1)
    return ok


# ---- a volume-preserving shear in front of the one-ellipsoid bound (ns_shear_fit / ns_shear_inv on the device) --------
def _shear_monomials(comp):
    """The monomials (a, b) -> z_a z_b (-1 = the factor 1) of the shear of sampled dimensions with velocity components
    comp[D], ordered by their largest coordinate: [1], then per coordinate j its own z_j, z_j^2 and z_k z_j for the earlier
    coordinates k of the same component.  start[j] = monomials before coordinate j's own = the features z_j is regressed
    on; mono[start[j]] is z_j itself.  (ns_shear_monomials on the host side of the device sampler.)"""
    D = len(comp)
    mono, start = [(-1, -1)], []
    for j in range(D):
        start.append(len(mono))
        mono.append((j, -1))
        mono.append((j, j))
        for k in range(j):
            if comp[k] == comp[j]:
                mono.append((k, j))
    return np.array(mono[:start[-1] + 1], dtype=np.int32), np.array(start, dtype=np.int32)


def _shear_phi(Z, mono, n):
    """The first n monomials of rows Z[K, D]."""
    F = np.ones((Z.shape[0], n))
    for m in range(1, n):
        a, b = mono[m]
        F[:, m] = Z[:, a] if b < 0 else Z[:, a] * Z[:, b]
    return F


def _fit_shear(U, mono, start):
    """The shear of one pixel's live points U[n, D]: standardise, z = (u - mu) / sg, then regress every coordinate on
    the monomials of the earlier ones (`_shear_monomials`): w_j = z_j - phi_j(z_<j) . beta_j.  An additive triangular map
    has a unit Jacobian: a point uniform in a w-ellipsoid is uniform in u over the ellipsoid's curved image, whose volume
    is the ellipsoid's times prod sg.  One Gram matrix of all monomials and ONE Cholesky factorisation of it serve every
    coordinate: the factor of a leading block is the leading block of the factor, and row start[j] of the factor is the
    forward substitution of coordinate j's normal equations.  Returns mu[D], sg[D], beta[D, M] (row j: start[j] numbers)."""
    n, D = U.shape
    M = mono.shape[0]
    mu = U.sum(axis=0) / n
    d = U - mu
    sg = np.sqrt(np.einsum('ni,ni->i', d, d) / (n - 1))
    sg = np.maximum(sg, 1e-300)
    Z = d / sg
    F = _shear_phi(Z, mono, M)
    G = F.T @ F
    G[np.diag_indices(M)] += _NS_SHEAR_RIDGE * n
    # Cholesky, column by column; a monomial whose pivot has drowned in rounding is dropped (ns_shear_fit): pivot = its own
    # norm, nothing below it, so that its coefficient comes out as zero
    Lc = np.zeros((M, M))
    for j in range(M):
        d = G[j, j] - Lc[j, :j] @ Lc[j, :j]
        keep = d > _NS_SHEAR_PIVOT * G[j, j]
        Lc[j, j] = math.sqrt(d) if keep else math.sqrt(max(G[j, j], 1e-300))
        if keep and j + 1 < M:
            Lc[j + 1:, j] = (G[j + 1:, j] - Lc[j + 1:, :j] @ Lc[j, :j]) / Lc[j, j]
    beta = np.zeros((D, M))
    for j in range(1, D):
        pj = int(start[j])
        y = Lc[pj, :pj]
        b = np.zeros(pj)
        for r in range(pj - 1, -1, -1):                                         # back substitution with the block's transpose
            b[r] = (y[r] - Lc[r + 1:pj, r] @ b[r + 1:]) / Lc[r, r]
        beta[j, :pj] = b
    return mu, sg, beta


def _shear_fwd(X, mu, sg, beta, mono, start):
    """w of rows X[K, D] of the unit cube."""
    Z = (X - mu) / sg
    W = Z.copy()
    for j in range(1, Z.shape[1]):
        pj = int(start[j])
        W[:, j] = Z[:, j] - _shear_phi(Z, mono, pj) @ beta[j, :pj]
    return W


def _shear_inv(W, mu, sg, beta, mono, start):
    """Unit-cube rows of rows W[K, D]: coordinate by coordinate, each from the ones before it."""
    Z = W.copy()
    # (a draw from the far end of an ellipsoid whose coefficients are large can run away through the products: it ends as
    # inf or nan, fails the unit cube's test like any other point outside, and is dropped -- on the device as here)
    with np.errstate(over='ignore', invalid='ignore'):
        for j in range(1, W.shape[1]):
            pj = int(start[j])
            Z[:, j] = W[:, j] + _shear_phi(Z, mono, pj) @ beta[j, :pj]
        return mu + sg * Z


def _fit_pairs(W, enlarge):
    """The pair ellipses of one pixel (ns_refit): for every pair i < j of the sheared coordinates the ellipse around the live
    points' projection onto (w_i, w_j) -- covariance ellipse scaled to enclose every point, its area times `enlarge`.  The
    region lies inside the cylinder over every one of its projections: D (D - 1) / 2 more free vetoes, five numbers each:
    rows [c_i, c_j, 1 / L00, L10, 1 / L11] with {c + L y : |y| <= 1}."""
    n, D = W.shape
    c = W.sum(axis=0) / n
    d = W - c
    cov = (d.T @ d) / (n - 1)
    out = np.empty((D * (D - 1) // 2, 5))
    e = 0
    for j in range(1, D):
        for i in range(j):
            l00 = math.sqrt(max(cov[i, i], 1e-300))
            l10 = cov[j, i] / l00
            l11 = math.sqrt(max(cov[j, j] - l10 * l10, 1e-300))
            y0 = d[:, i] / l00
            y1 = (d[:, j] - l10 * y0) / l11
            s = math.sqrt(float(np.max(y0 * y0 + y1 * y1)) * enlarge)
            out[e] = (c[i], c[j], 1.0 / (l00 * s), l10 * s, 1.0 / (l11 * s))
            e += 1
    return out


def _pair_veto(W, pairs):
    """Flags of the rows W[K, D] (sheared coordinates) inside every pair ellipse."""
    D = W.shape[1]
    ok = np.ones(W.shape[0], dtype=bool)
    e = 0
    for j in range(1, D):
        for i in range(j):
            ci, cj, r00, l10, r11 = pairs[e]
            y0 = (W[:, i] - ci) * r00
            y1 = ((W[:, j] - cj) - l10 * y0) * r11
            ok &= (y0 * y0 + y1 * y1) <= 1.0
            e += 1
    return ok


def _assemble(ndim, nlive, n_iter, n_evals, dead, Tlive, Llive, tol=None):
    """NestedResult per pixel from dead points (theta, lnL, lnw per pixel) and final live points:
    every live point carries the mass X_final / nlive.  `nlive`: one number, or one per pixel (a pixel's live
    points are then the first nlive[p] of its slice of `Tlive` / `Llive`).  With `tol` given a run whose live
    points could still add more than `tol` to lnZ (the stop test it did not meet) is marked `truncated`."""
    nl_all = np.broadcast_to(np.asarray(nlive, dtype=np.int64), (len(n_iter),))
    def log_sum_exp(x):
        """ln sum exp(x) about the largest term (a sequential logaddexp.reduce costs five times as much: this
        loop runs once per pixel of a map)."""
        if x.size == 0:
            return -np.inf
        m = x.max()
        return m if not np.isfinite(m) else m + math.log(np.exp(x - m).sum())

    results = []
    for p in range(len(n_iter)):
        nlive = int(nl_all[p])
        ln_nlive = math.log(nlive)
        dT, dL, dlnw = dead[p]
        n_dead = dL.shape[0]
        post = np.empty((n_dead + nlive, ndim + 2))
        post[:n_dead, :ndim] = dT
        post[n_dead:, :ndim] = Tlive[p][:nlive]
        L = np.empty(n_dead + nlive)
        L[:n_dead] = dL
        L[n_dead:] = Llive[p][:nlive]
        lw = np.empty(n_dead + nlive)                           # ln(prior mass x likelihood)
        np.add(dlnw, dL, out=lw[:n_dead])
        np.add(Llive[p][:nlive], -n_iter[p] / nlive - ln_nlive, out=lw[n_dead:])
        lnZ_dead = log_sum_exp(lw[:n_dead])
        lnZ_tot = np.logaddexp(lnZ_dead, log_sum_exp(lw[n_dead:]))
        wt = np.exp(lw - lnZ_tot)
        # information H = sum w (lnL - lnZ), for the error estimate sqrt(H / nlive)
        with np.errstate(invalid='ignore'):
            Hp = float(np.sum(np.where(wt > 0, wt * (L - lnZ_tot), 0.0)))
        np.multiply(L, -2.0, out=post[:, ndim])
        post[:, ndim + 1] = wt
        results.append(NestedResult(post, lnZ_tot, np.sqrt(max(Hp, 0.0) / nlive), L.max(), nlive,
                                    n_evals[p], n_iter[p], Hp))
        if tol is not None:
            remain = Llive[p][:nlive].max() - n_iter[p] / nlive
            # (a plateau -- every live point at one lnL, `_plateau` -- is a finished run: what is left is exactly L + ln X)
            results[-1].truncated = bool(not (np.logaddexp(lnZ_dead, remain) - lnZ_dead < tol) and not _plateau(Llive[p][:nlive]))
    return results


def _plateau(Llive):
    """The stop rule beside `tol`, `maxiter` and the dead-point cap: live points that all carry one lnL.  No proposal can
    be above the threshold of such a pixel (a replacement needs L > min), so its run would never end; and nothing is
    left to find -- the rest of its evidence is exactly L + ln X, which the live points' share of `_assemble` adds.  (A
    pixel whose every draw is non-finite is all log_zero; lines narrower than a channel predict exactly zero.)  The
    device tests the same where it tests the others: ns_plateau_kernel before the first round, ns_update_kernel after
    every replacement."""
    return bool(Llive.max() == Llive.min())


def _resolve_seed(seed):
    if seed is None or seed < 0:                                # like MultiNest: from the system
        return int(np.random.SeedSequence().generate_state(1, dtype=np.uint64)[0] >> np.uint64(1))
    return int(seed)


def default_cap_iter(nlive):
    """Dead-point slots per pixel when the caller names none: 60 nlive iterations reach ln X = -60, far
    past where any fit of this kind has collected its evidence; a run that does hit the cap is flagged
    `truncated`.  The same default on the host twin and on the device."""
    return 60 * int(nlive)


# Named settings of a sheared one-ellipsoid bound (two and three components) and its free rejections: the safety factor on
# the ellipsoid's volume and the margins of the boxes and the pair ellipses trade evaluations for a cut of prior mass that
# shows in the evidence.  Measured on 256 pixels of the two-component test cube against bound-free rejection
# (tests/test_sampler_bias.py pins them; tests/golden/sampler_bias_reference.json, scripts/sampler_bias_reference.py;
# a pixel's own lnZ_err is 0.25; profiles/r05/sampler_bias.txt):
#   'speed'     shear 2.5, margin 1.75, pairs 1.75 (round 4's default)         +0.075 in lnZ, 408 k evaluations per pixel
#   'default'   shear 3,   margin 2.5,  pairs 2.0                              +0.031, 699 k
#   'evidence'  shear 4,   margin 3.5,  pairs 2.5, rejection only (no walks)   +0.018, 1180 k
# (the sheared ellipsoid alone at 2.5, no boxes, no pairs: +0.029 at 5.6 M -- the factor on its volume, not the margins,
# carries the last 0.03)
PRECISION = {'speed': {'shear': 2.5, 'margin': 1.75, 'pairs': 1.75}, 'default': {},
             'evidence': {'shear': 4.0, 'margin': 3.5, 'pairs': 2.5, 'method': 'reject'}}


def resolve_precision(precision, margin=None, pairs=None, method='auto', shear=None):
    """(margin, pairs, method, shear) of the named setting `precision` (None = 'default'); values given explicitly win."""
    knobs = PRECISION[precision or 'default']
    return (knobs.get('margin') if margin is None else margin, knobs.get('pairs') if pairs is None else pairs,
            knobs.get('method', method) if method == 'auto' else method, knobs.get('shear') if shear is None else shear)


# ---- the run's form, decided once: ns_plan of csrc/nfa_sampler_plan.h, the same chain under the same field names
# (tests/test_sampler_plan.py compares the two plans field by field)
def _plan(nd, ndim, nlive, fmap, ellipsoids=None, frames=None, walkers=None, walk_factor=None, k_target=None,
          refit_every=None, ratio_max=None, kmax=None, margin=None, shear=None, pairs=None):
    """What bound a run gets: `nd` sampled dimensions of `ndim` slots (fmap[nd] = their slots), `nlive` = the largest
    number of live points of a pixel, every knob None (unset) or a value.  In dependency order, like ns_plan."""
    def pick(v, default):
        return default if v is None else v
    p = types.SimpleNamespace(error=None)
    p.ratio_max, p.kmax = int(pick(ratio_max, _NS_RATIO_MAX)), int(pick(kmax, _NS_KMAX))
    p.w_fixed = int(pick(walkers, 0))                           # (A/B knob; 0: by the live points)
    p.w_stride = p.w_fixed if p.w_fixed > 0 else _walkers_for(nlive)
    # to walks below an acceptance of 1 in walk_factor * n_steps: 2 from seven sampled dimensions on, 64 below -- there a
    # rejection round, one large batch, beats a walk cycle of n_steps small ones down to very low acceptances
    p.walk_factor = int(pick(walk_factor, _NS_WALK_FACTOR_LOWD if nd <= _NS_WALK_LOWD else _NS_WALK_FACTOR))
    p.k_target, p.refit_every = int(pick(k_target, _NS_K_TARGET)), int(pick(refit_every, _NS_REFIT_EVERY))
    p.stage_live = int(nlive * nd * 8 <= _NS_STAGE_BYTES)       # the device's refit holds the live points in LDS
    p.max_ell = int(pick(ellipsoids, _NS_ME))
    p.multi = int(bool(p.stage_live) and nd <= _NS_ME_MAXD and p.max_ell > 1)
    # the shear: all five free parameters of two or three components, slot % ncomp = dimension % ncomp
    p.shear_enlarge = float(pick(shear, _NS_SHEAR_ENLARGE))
    nc = nd // 5
    shape = nd in (10, 15) and ndim == 6 * nc and bool(np.all(np.asarray(fmap) % nc == np.arange(nd) % nc))
    p.shear = int(p.shear_enlarge >= 1.0 and shape and not p.multi and bool(p.stage_live))
    p.sh_M = int(_shear_monomials(np.arange(nd) % nc)[0].shape[0]) if p.shear else 0
    if p.sh_M > _NS_SHEAR_MMAX:
        p.error = 'shear: too many monomials'
        return p
    # boxes: one-ellipsoid bounds with staged live points; by default _NS_FRAMES frames where the bound is sheared, none elsewhere
    nf = int(pick(frames, _NS_FRAMES if p.shear else -1))
    p.boxes = int(not p.multi and bool(p.stage_live) and nf >= 0)
    p.n_frames = nf if p.boxes else 0
    p.margin_c = float(pick(margin, _NS_MARGIN_C))
    # the pair ellipses: with the shear and the boxes (the device fits them in the shear's scratch, four doubles a pair)
    p.pairs_enlarge = float(pick(pairs, _NS_PAIRS_ENLARGE))
    p.pairs = int(bool(p.shear) and bool(p.boxes) and p.pairs_enlarge >= 1.0 and (nd * (nd - 1) // 2) * 4 <= p.sh_M * p.sh_M)
    return p


# ---- the twin: one state, and one function per stage of the device sampler (csrc/nfa_sampler.h) ---------------------
def _conventions(n_pix, ndim, nlive, efr, n_cand, upd_frac, seed, method, n_steps, free_mask, precision, margin, pairs, shear):
    """What `run_nested` and `sampler.run_nested_device` settle in the same way before either starts.  `nl`: live points
    per pixel -- one number for everybody, or one per pixel (arrays are then laid out for the largest, `nlive`, and a pixel
    uses the first nl[p] slots, like the device sampler after nfa_sampler_set_pixel_nlive); `K` proposals per pixel and
    round at least; the seed; the named precision (`margin`, `pairs`, `shear`, the method); the method's code; `n_steps`;
    the sampled slots `fmap` and their number `nd`; `updp` replacements of a pixel between two refits."""
    cv = types.SimpleNamespace()
    cv.nl = np.broadcast_to(np.asarray(nlive, dtype=np.int64), (int(n_pix),)).copy()
    cv.nlive = int(cv.nl.max())
    assert cv.nl.min() > ndim + 1 and 0 < efr <= 1
    cv.margin, cv.pairs, method, cv.shear = resolve_precision(precision, margin, pairs, method, shear)
    cv.seed = _resolve_seed(seed)
    cv.K = int(n_cand) if n_cand else int(np.ceil(2.0 / efr))
    cv.method = {'reject': 0, 'auto': 1, 'walk': 2}[method] if isinstance(method, str) else int(method)
    cv.fmap = np.arange(ndim) if free_mask is None else np.flatnonzero(np.asarray(free_mask))
    cv.nd = int(cv.fmap.size)                                   # sampled dimensions
    cv.n_steps = int(n_steps) if n_steps else 10 * cv.nd
    cv.updp = np.maximum(1, (upd_frac * cv.nl).astype(np.int64))
    return cv


class TwinState(types.SimpleNamespace):
    """Everything a run of the twin holds, under `NsDev`'s field names where NsDev has the field (csrc/nfa_sampler.h):
    the scalars P, N, D, DT, K, fmap, seed, tol, maxiter, method, n_steps, log_zero and the per-pixel nlive, capp, updp;
    the live points Ulive, Tlive, Llive; the bound centre, axes, elnv, nell, use_cube, lnvol with ubox, fbox, frames,
    pair_tab and sh_mu, sh_sg, sh_beta, sh_mono, sh_start; the counters n_iter, n_evals, cand_base, lnZ, active,
    since_fit; the walks' walk, wstep, wW, wscale, wLthr, wacc_sum, wtot_sum, wU, wT, wL, wnacc; the rejection rounds'
    rj_scan, rj_acc, rj_raw, rj_val, ln_pass, Kp.  Beside them the plan `pl` (`_plan`), the dead points (`dead`: theta,
    lnL and ln w of each, per pixel in the order they died), the round `rnd` with its `Kr`, `n_chunk`, `raw_sum` and
    `val_sum` (`_chunk_kr`), and what only the host has: `loglike`, `chunk`, `efr`, `enlarge`, `ln_shrink`, `b_target`."""


def _expand(S, U):
    """Rows of the full unit cube from rows of the sampled dimensions."""
    T = np.full(U.shape[:-1] + (S.DT,), 0.5)
    T[..., S.fmap] = U
    return T


def _evaluate(S, pix, T):
    """lnL of rows T of pixels pix, `chunk` rows a call; what is not finite becomes log_zero.  T comes back as theta."""
    out = np.empty(T.shape[0])
    for a in range(0, T.shape[0], S.chunk):
        out[a:a + S.chunk] = S.loglike(pix[a:a + S.chunk], T[a:a + S.chunk])
    return np.where(np.isfinite(out), out, S.log_zero)


def _begin(loglike, ndim, cv, tol, efr, maxiter, log_zero, chunk, cap_iter, batch_target, enlarge, **knobs):
    """nfa_sampler_begin + ns_init_live_kernel: the state of a run with the conventions `cv` (`_conventions`) and the
    plan's `knobs` (`_plan`) -- its form, the first live points, zeroed counters, the first bound of every pixel."""
    P, N, D = int(cv.nl.size), cv.nlive, cv.nd
    assert cv.fmap.size > 0 and cv.fmap.max() < ndim
    S = TwinState(P=P, N=N, D=D, DT=int(ndim), K=cv.K, fmap=cv.fmap, seed=cv.seed, tol=tol, maxiter=maxiter, method=cv.method,
                  n_steps=cv.n_steps, nlive=cv.nl, updp=cv.updp, log_zero=log_zero, loglike=loglike, chunk=chunk, efr=efr,
                  enlarge=enlarge, ln_shrink=np.log1p(-np.exp(-1.0 / cv.nl)))       # ln(X_i - X_{i+1}) - ln X_i, per pixel
    # dead-point slots per pixel, never more than maxiter: the twin keeps lists and a run of maxiter = 0 has none (the
    # device allocates them, needs at least one and takes a given cap_iter as it is: run_nested_device)
    if cap_iter is None:
        S.capp = np.array([min(maxiter, default_cap_iter(int(n))) for n in cv.nl], dtype=np.int64)
    else:
        S.capp = np.full(P, min(cap_iter, maxiter) if maxiter > 0 else cap_iter, dtype=np.int64)
    S.pl = _plan(D, ndim, N, cv.fmap, margin=cv.margin, shear=cv.shear, pairs=cv.pairs, **knobs)
    assert S.pl.error is None and (S.pl.shear_enlarge == 0.0 or S.pl.shear_enlarge >= 1.0)
    # live points: unit-cube positions, physical parameters, log-likelihoods
    all_pix = np.arange(P, dtype=np.int32)
    S.Ulive = _uniform(S.seed, all_pix[:, None, None], _NS_TAG_LIVE + np.arange(N, dtype=_U64)[None, :, None],
                       np.arange(D, dtype=_U64)[None, None, :])
    T = _expand(S, S.Ulive).reshape(-1, S.DT)
    S.Llive = _evaluate(S, np.repeat(all_pix, N), T).reshape(P, N)
    S.Tlive = T.reshape(P, N, S.DT)
    S.n_evals, S.n_iter, S.cand_base = cv.nl.copy(), np.zeros(P, dtype=np.int64), np.zeros(P, dtype=np.int64)
    S.lnZ, S.active, S.since_fit = np.full(P, -np.inf), np.full(P, maxiter > 0), np.zeros(P, dtype=np.int64)
    for p in range(P):                                          # (ns_plateau_kernel: such a pixel never enters a round)
        S.active[p] &= not _plateau(S.Llive[p, :int(cv.nl[p])])
    S.dead = [[] for _ in range(P)]                             # per pixel: theta, lnL, ln w of its dead points
    S.rnd, S.Kr, S.n_chunk, S.b_target = 0, S.K, P, max(P * S.K, int(batch_target))
    S.raw_sum = S.val_sum = 0                                   # proposals drawn / evaluated since the last `_chunk_kr`
    _begin_bound(S)
    _begin_walks(S)
    for p in range(P):
        _refit(S, p, 0.0)
    return S


def _begin_bound(S):
    """The bound's arrays, [pixel][ellipsoid]; the free rejections of a one-ellipsoid bound: boxes in the unit cube's
    axes, the ellipsoid's frame and n_frames rotations, the pair ellipses (`_fit_pairs`) with the shear and the boxes."""
    P, D, pl = S.P, S.D, S.pl
    S.centre, S.axes = np.zeros((P, _NS_ME, D)), np.zeros((P, _NS_ME, D, D))
    S.elnv, S.nell = np.full((P, _NS_ME), -np.inf), np.ones(P, dtype=np.int64)
    S.use_cube, S.lnvol = np.empty(P, dtype=bool), np.empty(P)
    S.frames = _frames(D, pl.n_frames) if pl.boxes else None
    S.ubox, S.fbox = np.zeros((P, D, 2)), np.zeros((P, pl.n_frames + 1, D, 2))
    S.pair_tab = np.zeros((P, D * (D - 1) // 2, 5)) if pl.pairs else None
    if pl.shear:
        S.sh_mono, S.sh_start = _shear_monomials(S.fmap % (D // 5))
        S.sh_mu, S.sh_sg, S.sh_beta = np.zeros((P, D)), np.ones((P, D)), np.zeros((P, D, S.sh_mono.shape[0]))


def _begin_walks(S):
    """The state of the constrained random walks, per pixel and per walker, and of the rejection rounds' decisions."""
    P, W = S.P, S.pl.w_stride
    S.walk, S.wstep, S.wW = np.zeros(P, dtype=bool), np.zeros(P, dtype=np.int64), np.zeros(P, dtype=np.int64)
    S.wscale, S.wLthr = np.ones(P), np.zeros(P)
    S.wacc_sum, S.wtot_sum = np.zeros(P, dtype=np.int64), np.zeros(P, dtype=np.int64)
    S.wU, S.wT, S.wL = np.zeros((P, W, S.D)), np.zeros((P, W, S.DT)), np.zeros((P, W))
    S.wnacc = np.zeros((P, W), dtype=np.int64)
    # what a pixel's rejection rounds did since the last decision point (every n_steps rounds): candidates scanned and
    # accepted, proposals drawn and evaluated; ln of the last window's evaluated / drawn (the boxes' share of the
    # ellipsoid: what the way back from the walks counts the bound's volume with)
    S.rj_scan, S.rj_acc = np.zeros(P, dtype=np.int64), np.zeros(P, dtype=np.int64)
    S.rj_raw, S.rj_val = np.zeros(P, dtype=np.int64), np.zeros(P, dtype=np.int64)
    S.ln_pass = np.zeros(P)
    # a pixel's own share of a rejection round's proposals (NS_K_TARGET): halved after a round with more than twice
    # k_target replacements, doubled after one with fewer than half of it; 0 = the round's Kr
    S.Kp = np.full(P, _NS_KP_START, dtype=np.int64)             # (a small share first, doubled while little is accepted)


def _refit(S, p, ln_x):
    """ns_refit / ns_refit_multi / ns_shear_fit: the bound of pixel p's live points at ln X = ln_x -- several ellipsoids,
    or one (behind the shear where the plan has it) with its boxes and pair ellipses."""
    pl, U = S.pl, S.Ulive[p, :int(S.nlive[p])]
    if pl.multi:
        S.centre[p], S.axes[p], S.elnv[p], S.nell[p], S.lnvol[p], S.use_cube[p] = _fit_multi(U, S.efr, ln_x, S.enlarge, pl.max_ell)
        return
    ln_jac, enlarge = 0.0, S.enlarge
    if pl.shear:
        S.sh_mu[p], S.sh_sg[p], S.sh_beta[p] = _fit_shear(U, S.sh_mono, S.sh_start)
        U = _shear_fwd(U, S.sh_mu[p], S.sh_sg[p], S.sh_beta[p], S.sh_mono, S.sh_start)     # the bound, `ubox` included, is fitted in w
        ln_jac = float(np.log(S.sh_sg[p]).sum())                # ln |du / dw|: volumes in w units are smaller by this
        enlarge = pl.shear_enlarge
    c, A, _, lnv = _fit_ellipsoids(U, S.efr, ln_x - ln_jac, enlarge)
    S.centre[p, 0], S.axes[p, 0], S.lnvol[p], S.nell[p] = c, A, lnv + ln_jac, 1
    S.use_cube[p], S.elnv[p, 0] = S.lnvol[p] >= 0.0, S.lnvol[p]
    if pl.boxes:
        S.ubox[p], S.fbox[p] = _fit_boxes(U, c, A, S.frames, pl.margin_c)
    if pl.pairs:
        S.pair_tab[p] = _fit_pairs(U, pl.pairs_enlarge)


def _propose(S, p, k):
    """ns_propose_one, k times: the next k proposals of pixel p's stream -- uniform in its ellipsoid(s), or in the unit
    cube while that is the smaller bound, mapped back through the shear -- and which of them are valid: inside every
    box and pair ellipse, kept by the several-ellipsoids test, inside the unit cube (outside = outside the prior)."""
    pl, keep = S.pl, True
    a = _U64(S.cand_base[p]) + np.arange(k, dtype=_U64)
    if S.nell[p] > 1 and not S.use_cube[p]:
        cand, keep = _candidates_multi(S.seed, p, a, S.centre[p], S.axes[p], S.elnv[p], int(S.nell[p]), S.lnvol[p])
    else:
        c, A, zz = S.centre[p, 0], S.axes[p, 0], None
        if S.use_cube[p]:
            cand = _uniform(S.seed, p, a[:, None], np.arange(S.D, dtype=_U64)[None, :])
        else:
            zz = _ball_points(S.seed, p, a, S.D)
            cand = c + np.einsum('ji,ki->kj', A, zz)
        wc = cand
        if pl.shear:
            # the ellipsoid lives in the sheared frame: its draws are w, the unit cube's draws are u
            if S.use_cube[p]:
                wc = _shear_fwd(cand, S.sh_mu[p], S.sh_sg[p], S.sh_beta[p], S.sh_mono, S.sh_start)
            else:
                cand = _shear_inv(wc, S.sh_mu[p], S.sh_sg[p], S.sh_beta[p], S.sh_mono, S.sh_start)
        if pl.boxes:
            # the proposal's coordinates in the ellipsoid's frame: the unit-ball point it was made from, or (drawn from the
            # unit cube) A^-1 (w - c)
            if zz is None:
                zz = np.linalg.solve(A, (wc - c).T).T
            keep = _box_veto(wc, zz, S.ubox[p], S.fbox[p], S.frames)
            if pl.pairs:
                keep &= _pair_veto(wc, S.pair_tab[p])
    return cand, np.all((cand >= 0.0) & (cand < 1.0), axis=1) & keep


def _evaluate_valid(S, p, cand, valid):
    """The round's likelihood batch, pixel p's rows of it: the valid proposals compacted, expanded to theta rows and
    evaluated.  Returns their indices into `cand`, theta and lnL."""
    vi = np.flatnonzero(valid)
    S.val_sum += int(vi.size)
    T = _expand(S, cand[vi])
    return vi, T, _evaluate(S, np.full(vi.size, p, dtype=np.int32), T)


def _replace(S, p, cU, cT, Lk):
    """The replacement in ns_update_kernel: the worst live point of pixel p dies, the candidate takes its slot (Skilling's
    bookkeeping: dead point, ln w, running lnZ); True when p is done."""
    nlive, cap = int(S.nlive[p]), int(S.capp[p])
    Llive = S.Llive[p, :nlive]
    w = int(np.argmin(Llive))
    Lmin = Llive[w]
    lnw = -S.n_iter[p] / nlive + S.ln_shrink[p]
    S.lnZ[p] = np.logaddexp(S.lnZ[p], lnw + Lmin)
    if S.n_iter[p] < cap:
        S.dead[p].append((S.Tlive[p, w].copy(), Lmin, lnw))
    S.Ulive[p, w], S.Tlive[p, w], Llive[w] = cU, cT, Lk
    S.n_iter[p] += 1
    S.since_fit[p] += 1
    remain = Llive.max() - S.n_iter[p] / nlive
    return bool((np.logaddexp(S.lnZ[p], remain) - S.lnZ[p] < S.tol) or S.n_iter[p] >= S.maxiter or S.n_iter[p] >= cap
                or _plateau(Llive))


def _scan(S, p, cU, cT, cL):
    """The update wave's sequential scan: the candidates in order, every one above the pixel's threshold of the moment
    replaces its worst live point, until the pixel is done.  Returns how many were scanned and accepted, and done."""
    Llive = S.Llive[p, :int(S.nlive[p])]
    accepted = 0
    for j in range(cL.shape[0]):
        if cL[j] > Llive.min():
            accepted += 1
            if _replace(S, p, cU[j].copy(), cT[j].copy(), cL[j]):
                return j + 1, accepted, True
    return cL.shape[0], accepted, False


def _update_reject(S, p, Kr):
    """The scan branch of ns_update_kernel, with the proposals and likelihoods the round's earlier launches hand it: scan,
    the pixel's share `Kp` of the next round's proposals, and at a round that is a multiple of n_steps the decision to
    walk.  True when p is done."""
    k_target = S.pl.k_target
    k_used = int(min(S.Kp[p], Kr)) if (k_target > 0 and S.Kp[p] > 0) else Kr      # what the pixel's random stream advances by
    cand, valid = _propose(S, p, k_used)
    vi, T, L = _evaluate_valid(S, p, cand, valid)
    scanned, accepted, done = _scan(S, p, cand[vi], T, L)
    S.n_evals[p] += scanned
    S.rj_scan[p] += scanned; S.rj_acc[p] += accepted; S.rj_raw[p] += k_used; S.rj_val[p] += int(vi.size)
    if k_target > 0:
        if accepted > 2 * k_target:
            S.Kp[p] = max(k_used // 2, S.K)
        elif 2 * accepted < k_target:
            S.Kp[p] = min(k_used * 2, _KP_MAX)
        else:
            S.Kp[p] = k_used
    # walk cycles of all pixels stay in phase: they start at rounds that are multiples of n_steps.  The decision looks at all
    # rejection rounds since the last one: to walks below 1 accepted in walk_factor * n_steps (profiles/r03/sweep_walk_factor.txt)
    if (S.rnd + 1) % S.n_steps == 0:
        few = S.pl.walk_factor * S.rj_acc[p] * S.n_steps < S.rj_scan[p] if S.rj_scan[p] >= 64 else S.rj_raw[p] >= 4096
        if not done and (S.method == 2 or (S.method == 1 and few)):
            S.walk[p], S.wstep[p], S.wscale[p], S.wacc_sum[p], S.wtot_sum[p] = True, 0, 1.0, 0, 0
            S.ln_pass[p] = math.log(max(int(S.rj_val[p]), 1) / max(int(S.rj_raw[p]), 1)) if S.pl.boxes else 0.0
        S.rj_scan[p] = S.rj_acc[p] = S.rj_raw[p] = S.rj_val[p] = 0
    S.cand_base[p] += k_used
    return done


def _walk_step(S, p, Kr):
    """The walk branch of ns_update_kernel: one Metropolis step of every walker of pixel p inside {L > the threshold frozen
    at the cycle's start}; the first step of a cycle starts the walkers from random live points, the last one hands them
    to the scan as the candidates, tunes the scale and decides on the way back to rejection.  True when p is done."""
    nlive, step, done = int(S.nlive[p]), int(S.wstep[p]), False
    W = min(S.pl.w_stride, S.pl.w_fixed or _walkers_for(nlive), Kr) if step == 0 else int(S.wW[p])
    a = _U64(S.cand_base[p]) + np.arange(W, dtype=_U64)
    wU, wT, wL, wnacc, Ulive = S.wU[p, :W], S.wT[p, :W], S.wL[p, :W], S.wnacc[p, :W], S.Ulive[p]
    if step == 0:
        start = np.minimum(nlive - 1, (_uniform(S.seed, p, a, _NS_B_START) * nlive).astype(np.int64))
        wU[:], wT[:], wL[:], wnacc[:] = Ulive[start], S.Tlive[p, start], S.Llive[p, start], 0
        S.wLthr[p] = S.Llive[p, :nlive].min()
        S.wW[p] = W
    # differential-evolution move: a scaled difference of two random live points
    ia = np.minimum(nlive - 1, (_uniform(S.seed, p, a, _B_PARTNER_A) * nlive).astype(np.int64))
    ib = np.minimum(nlive - 2, (_uniform(S.seed, p, a, _B_PARTNER_B) * (nlive - 1)).astype(np.int64))
    ib = ib + (ib >= ia)
    gam = S.wscale[p] * _DE_GAMMA / math.sqrt(2.0 * S.D)
    cand = wU + gam * (Ulive[ia] - Ulive[ib])
    vi, T, L = _evaluate_valid(S, p, cand, np.all((cand >= 0.0) & (cand < 1.0), axis=1))
    inside = L > S.wLthr[p]
    ok = vi[inside]
    wU[ok], wT[ok], wL[ok] = cand[ok], T[inside], L[inside]
    wnacc[ok] += 1
    S.n_evals[p] += vi.size
    S.wacc_sum[p] += ok.size
    S.wtot_sum[p] += vi.size
    S.wstep[p] = step + 1
    if S.wstep[p] >= S.n_steps:                                 # cycle end: the walkers that moved are the candidates
        k = np.flatnonzero(wnacc > 0)
        _, _, done = _scan(S, p, wU[k], wT[k], wL[k])
        if S.wtot_sum[p] > 0:                                   # acceptance near one half
            S.wscale[p] = min(1.0, S.wscale[p] * math.exp((S.wacc_sum[p] / S.wtot_sum[p] - _NS_WALK_TARGET) / (0.5 * math.sqrt(S.D))))
        S.wacc_sum[p] = S.wtot_sum[p] = S.wstep[p] = 0
        # back to rejection once the bound promises clearly more than a walk delivers: _WALK_BACK times what sent it to walks
        if S.method == 1 and (-S.n_iter[p] / nlive - min(S.lnvol[p] + S.ln_pass[p], 0.0)) > math.log(_WALK_BACK / (S.pl.walk_factor * S.n_steps)):
            S.walk[p] = False
    S.cand_base[p] += Kr
    return done


def _chunk_kr(S):
    """ns_chunk_kr, where the device compacts its pixel list: the proposals per pixel of the next rounds.  With boxes most
    proposals are vetoed for free: draw so many more that a round still evaluates ~b_target."""
    ratio = min(S.pl.ratio_max, max(1, (S.raw_sum + S.val_sum // 2) // max(S.val_sum, 1))) if S.pl.boxes and S.raw_sum else 1
    S.n_chunk = int(S.active.sum())                             # the pixels the device's list holds until the next look
    S.Kr = int(min(S.pl.kmax, max(S.K, (S.b_target * ratio) // S.n_chunk)))
    S.raw_sum = S.val_sum = 0


def _finish(S):
    """A `NestedResult` per pixel from its dead points, in the order they died, and its final live points."""
    dead = [(np.array([d[0] for d in dp]).reshape(-1, S.DT), np.array([d[1] for d in dp], dtype=np.float64),
             np.array([d[2] for d in dp], dtype=np.float64)) for dp in S.dead]
    res = _assemble(S.DT, S.nlive, S.n_iter, S.n_evals, dead, S.Tlive, S.Llive, S.tol)
    for r in res:
        r.rounds = S.rnd
    return res


def run_nested(loglike, ndim, n_pix, nlive=400, tol=0.5, efr=0.3, seed=-1, maxiter=int(1e6),
               n_cand=None, upd_frac=0.1, log_zero=LOG_ZERO, chunk=1 << 18, cap_iter=None,
               check_every=32, batch_target=262144, enlarge=1.5, method='auto', n_steps=None, free_mask=None, walk_factor=None, ellipsoids=None, walkers=None,
               progress=None, frames=None, margin=None, refit_every=4, shear=None, kmax=None, k_target=None, ratio_max=None, pairs=None,
               precision=None):
    """Nested sampling of `n_pix` independent problems in lock-step: the host twin of the
    device-resident sampler (csrc/nfa_sampler.h), same random numbers, same decisions.

    Parameters
    ----------
    loglike : callable(pix[B] int32, U[B, ndim] float64) -> lnL[B]
        Evaluates unit-cube rows against pixels; must overwrite U with the physical parameters
        (the convention of Runner.loglikelihood, core.pyx:558-561).
    nlive, tol, efr, seed, maxiter : as in ``run_multinest`` (core.pyx:727-744): live points,
        evidence tolerance, target sampling efficiency (the bounding ellipsoid is enlarged until its
        volume reaches X / efr), RNG seed (-1 = from the OS), iteration cap per pixel.
    n_cand : candidates per pixel and round (default ceil(2 / efr)), at least: every
        `check_every` rounds the number is raised so that the round's batch stays near
        max(n_pix * n_cand, batch_target) proposals however few pixels are still running (at most
        65536 per pixel); only proposals inside the unit cube are evaluated.
        They are scanned in order and every one above the pixel's current threshold replaces its
        worst live point.
    upd_frac : the ellipsoids are refitted at the end of a round once this fraction of nlive
        replacements has accumulated.
    cap_iter : dead-point slots per pixel (default: min(maxiter, 60 nlive), `default_cap_iter`); a pixel
        that fills them before meeting `tol` is returned with `truncated = True`.
    method, n_steps : 'reject' = rejection sampling in the bounding ellipsoid only; 'auto' = a pixel
        whose rejection round accepted fewer than 1 in 2 `n_steps` of the evaluated candidates
        switches to constrained random walks (64 walkers from random live points, `n_steps`
        Metropolis steps inside {L > threshold}; a step is a scaled difference of two random live
        points -- differential evolution, ter Braak 2006 -- with the scale tuned to an acceptance
        of one half); 'walk' = walks from the start.  n_steps defaults to 10 x sampled dimensions:
        scripts/sampler_bias_check.py measures the lnZ bias of walks that are too short (10
        dimensions: +0.13 with 40 steps, +0.03 with 80, +0.014 with 120; the error per run is 0.25).
    free_mask : ndim flags, 0 for unit-cube slots the likelihood does not depend on (constant or
        duplicated parameters: `PriorTransformer.free_mask`).  They are not sampled -- a uniform dummy
        dimension integrates to one -- and stay at u = 0.5: fewer dimensions for the same evidence.
    precision : 'speed' / 'default' / 'evidence': named settings of `shear`, `margin`, `pairs` and `method` (`PRECISION`).
    frames, margin : the free rejections of a one-ellipsoid bound (`_fit_boxes`): `frames` rotated frames beside the unit
        cube's axes and the ellipsoid's own (-1: no boxes; None: 32 where the bound is sheared, none elsewhere), `margin` the factor c of a face's distance beyond the extreme live point (2.5).
        With boxes the proposals per round are scaled by the last rounds' ratio of drawn to evaluated proposals (at most 8).
    shear : 0 = off; a number >= 1 = the one-ellipsoid bound is fitted to the live points AFTER a volume-preserving
        polynomial shear (`_fit_shear`: every coordinate minus a quadratic function of the earlier ones, which straightens
        the curved tex / ntot ridges), with this safety factor on the enclosing volume instead of `enlarge`; None = the
        default, 3.  Proposals are drawn in the sheared frame and mapped back; boxes, if on, live in that frame.  Only
        where all five free parameters of two or three components are sampled (10 or 15 dimensions): elsewhere ignored.
    refit_every : rejection-mode pixels refit their bound in rounds that are multiples of this (the device's engine option
        `sampler_refit_every`).
    enlarge : safety factor on the volume of the ellipsoid that just encloses the live points
        (scripts/sampler_bias_check.py: 1.0 biases lnZ by +0.020, 1.25 by +0.011, 2.0 by nothing measurable; the error is 0.18).

    Returns a list of `NestedResult`, one per pixel.
    """
    assert ndim > 0 and tol > 0 and maxiter >= 0
    cv = _conventions(n_pix, ndim, nlive, efr, n_cand, upd_frac, seed, method, n_steps, free_mask, precision, margin, pairs, shear)
    # (`ellipsoids`, `walkers`, `walk_factor`, `ratio_max`, `kmax`: None / 0 = the plan's default)
    S = _begin(loglike, ndim, cv, tol, efr, maxiter, log_zero, chunk, cap_iter, batch_target, enlarge,
               ellipsoids=ellipsoids or None, frames=frames, walkers=walkers or None, walk_factor=walk_factor or None,
               k_target=k_target, refit_every=refit_every, ratio_max=ratio_max or None, kmax=kmax or None)
    while S.active.any():
        if S.rnd % check_every == 0:
            _chunk_kr(S)
        S.raw_sum += S.Kr * S.n_chunk
        for p in np.flatnonzero(S.active):                      # one workgroup per pixel on the device
            p = int(p)
            was_walking = bool(S.walk[p])
            done = _walk_step(S, p, S.Kr) if was_walking else _update_reject(S, p, S.Kr)
            if done:
                S.active[p] = False
            elif S.since_fit[p] >= S.updp[p] and (was_walking or (S.rnd + 1) % S.pl.refit_every == 0):
                # (rejection-mode pixels refit only in every fourth round: on the device a refit makes the
                # whole launch wait, so they are taken together)
                _refit(S, p, -S.n_iter[p] / int(S.nlive[p]))
                S.since_fit[p] = 0
        S.rnd += 1
        if progress is not None:
            progress(int(S.active.sum()), int(S.n_iter.max()))
            if hasattr(progress, 'detail'):                     # (debugging aid: the round's state)
                progress.detail(dict(rnd=S.rnd, n_iter=S.n_iter, n_evals=S.n_evals, walk=S.walk, use_cube=S.use_cube, lnvol=S.lnvol, nell=S.nell,
                                     Kr=S.Kr, rj=(S.rj_scan, S.rj_acc, S.rj_raw, S.rj_val), ln_pass=S.ln_pass, Llive=S.Llive,
                                     Ulive=S.Ulive))
    return _finish(S)
