"""The likelihood of one spectrum under channel noise correlated along the spectral axis, restated with numpy.

The noise is n_c = sigma_c eps_c with eps the stationary unit-variance AR(2) process whose first two autocorrelations are
(rho_1, rho_2).  Here the correlation matrix R is the Toeplitz matrix of the autocorrelation sequence -- rho_0 = 1, rho_1,
rho_2, then the recursion rho_k = phi_1 rho_{k-1} + phi_2 rho_{k-2} -- and

    chi^2 = r^T (S R S)^-1 r,        r = d - p,  S = diag(sigma_c),        lnL = -chi^2 / 2

comes from a dense solve.  The engine computes it from the closed-form pentadiagonal inverse of R; nothing of that is shared
here.  `pred` comes from the other restatements and the oracle, never from the device.
"""
import numpy as np


def autocorrelation(rho1, rho2, n):
    """rho_0 .. rho_{n-1} of the AR(2) process with the given first two autocorrelations."""
    den = 1.0 - rho1 * rho1
    phi1, phi2 = rho1 * (1.0 - rho2) / den, (rho2 - rho1 * rho1) / den
    rho = np.empty(max(n, 3))
    rho[:3] = 1.0, rho1, rho2
    for k in range(3, n):
        rho[k] = phi1 * rho[k - 1] + phi2 * rho[k - 2]
    return rho[:n]


def corr_matrix(rho, n):
    """R [n, n]; rho = (rho_1, rho_2), (0, 0) for white noise."""
    seq = autocorrelation(float(rho[0]), float(rho[1]), n)
    idx = np.abs(np.arange(n)[:, None] - np.arange(n)[None, :])
    return seq[idx]


def sigmas(noise, size):
    return np.full(size, float(noise)) if np.ndim(noise) == 0 else np.asarray(noise, dtype=np.float64)


def covariance(noise, rho, size):
    s = sigmas(noise, size)
    return s[:, None] * corr_matrix(rho, size) * s[None, :]


def chi2(data, pred, noise, rho):
    r = np.asarray(data, dtype=np.float64) - np.asarray(pred, dtype=np.float64)
    return float(r @ np.linalg.solve(covariance(noise, rho, r.size), r))


def lnl(data, pred, noise, rho):
    """lnL of one spectrum, without the normalisation term (like every likelihood of the engine)."""
    return -0.5 * chi2(data, pred, noise, rho)


def magnitude(data, pred, noise, rho):
    """M of tests/test_correlation.py: the size of the terms lnL is a sum of, (|d|^T |Q| |d| + 2 |d|^T |Q| |p| + |p|^T |Q| |p|) / 2
    with |Q| the absolute values of the dense inverse covariance."""
    d, p = np.abs(np.asarray(data, dtype=np.float64)), np.abs(np.asarray(pred, dtype=np.float64))
    A = np.abs(np.linalg.inv(covariance(noise, rho, d.size)))
    return float(d @ A @ d + 2.0 * (d @ A @ p) + p @ A @ p) / 2.0


def ar2_noise(rng, rho, shape):
    """Unit-variance stationary Gaussian AR(2) noise along the last axis of `shape`: white noise through the Cholesky factor of R."""
    L = np.linalg.cholesky(corr_matrix(rho, shape[-1]))
    return rng.normal(size=shape) @ L.T


def bartlett_se(rho, k, n_pairs):
    """Standard error of the sample autocorrelation at lag k from n_pairs products, by Bartlett's formula from the TRUE
    autocorrelations: var = sum_j (rho_{j+k}^2 + rho_{j-k} rho_{j+k} - 4 rho_k rho_j rho_{j-k} + 2 rho_k^2 rho_j^2) / n."""
    m = 400
    seq = autocorrelation(float(rho[0]), float(rho[1]), m + k + 1)
    r = lambda j: seq[abs(j)]
    tot = sum(r(j + k) ** 2 + r(j - k) * r(j + k) - 4 * r(k) * r(j) * r(j - k) + 2 * r(k) ** 2 * r(j) ** 2 for j in range(-m, m + 1))
    return float(np.sqrt(tot / n_pairs))


# the calibration of the likelihood (tests/test_correlation.py, test_correlation_cpu.py): 512 pixels of true AR(2) noise
CAL_PIX, CAL_N, CAL_SIGMA, CAL_SEED = 512, 256, 0.2, 61


def calibration_pixels(rho):
    out = CAL_SIGMA * ar2_noise(np.random.default_rng(CAL_SEED), rho, (CAL_PIX, CAL_N))
    out.setflags(write=False)
    return out


def calibration_figures(x2):
    """(mean, its distance from N in standard errors, variance / 2N) of -2 sigma^2 lnL at p = 0 over the pixels."""
    x2 = np.asarray(x2)
    mean = float(x2.mean())
    return mean, (mean - CAL_N) / np.sqrt(2.0 * CAL_N / x2.size), float(x2.var(ddof=1)) / (2.0 * CAL_N)
