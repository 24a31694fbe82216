"""The template sets and noise rows of tests/test_templates.py, numpy only, so that tests/test_templates_cpu.py can hold every
one of them to the condition the GPU bound assumes: a normalised Gram matrix, over the directions the rank rule keeps, of
condition number <= 1e3 (the moment form loses about cond x 2e-16 against the QR of tests/tmpl_restatement.py).

Periods are chosen with 1.5 cycles and more across the spectrum and are no integer: beside a cubic, fewer cycles are nearly a
polynomial."""
import numpy as np

BOUNDARY_SIZES = (4, 63, 64, 65, 127, 128, 129, 300)
ORDERS = (-1, 0, 1, 3)
COUNTS = (1, 2, 4)
N_CHAN = 300                      # test_lte_bands_cpu.N_CHAN: the channels of a spectrum of the model cases
COND_MAX = 1e3
SCI_N, SCI_PERIOD, SCI_PHASE, SCI_AMP, SCI_SIGMA = 256, 37.3, 0.9, 0.5, 0.1      # 7. the science: the ripple is 0.5 sigma


def ripple(n, period, phase=None):
    """nestfit_amd.ripple, restated (the CPU test holds the two together)."""
    arg = 2.0 * np.pi * np.arange(n) / period
    return np.stack([np.sin(arg), np.cos(arg)]) if phase is None else np.sin(arg + phase)[None, :]


def templates(n, count):
    """1: a ripple of known phase, 2.3 cycles across the spectrum; 2: its sine and cosine; 4: and those of 3.7 cycles.  In
    the caller's scaling: amplitudes of 0.3 and 25, which the engine must not see."""
    if count == 1:
        return 0.3 * ripple(n, n / 2.3, 0.7)
    if count == 2:
        return 25.0 * ripple(n, n / 2.3)
    return np.concatenate([25.0 * ripple(n, n / 2.3), 0.3 * ripple(n, n / 3.7)])


def channel_noise(n, seed, base=0.1):
    """A noise per channel over base .. 3 base with masked channels (inf): three at random and, from 70 channels on, the four
    astride the first 64-channel seam but one (62, 63 and 65, 66), so that a row's last and first lanes hold weight 0."""
    rng = np.random.default_rng(seed)
    noise = base * rng.uniform(1.0, 3.0, n)
    if n >= 8:
        noise[rng.choice(n, 3, replace=False)] = np.inf
    if n >= 70:
        noise[[62, 63, 65, 66]] = np.inf
    return noise


# the model cases: templates per spectrum for the sets of two spectra (ammonia, the filled mix) and of one (N2H+ 2-1)
def model_templates(n_spec, which):
    """'mixed': four on the first spectrum and none (T = 0) on the second; 'both': two and one; one spectrum: `which` counts."""
    if n_spec == 1:
        return [templates(N_CHAN, 4 if which == 'mixed' else 2)]
    if which == 'mixed':
        return [templates(N_CHAN, 4), None]
    return [templates(N_CHAN, 2), 0.5 * ripple(N_CHAN, 37.3, 0.2)]


def every_set():
    """(label, n, noise, order, templates of ONE spectrum) of everything the GPU tests give the engine, rank tests aside (those
    are degenerate on purpose and say so)."""
    for n in BOUNDARY_SIZES:
        for chan in (False, True):
            for order in ORDERS:
                for count in COUNTS:
                    yield f'boundary n={n} chan={chan} K={order} T={count}', n, channel_noise(n, 7 * n) if chan else 0.1, order, templates(n, count)
    for order in ORDERS:
        for which in ('mixed', 'both'):
            for k, t in enumerate(model_templates(2, which)):
                if t is not None:
                    for chan in (False, True):
                        yield f'model {which} spectrum {k} chan={chan} K={order}', N_CHAN, channel_noise(N_CHAN, 31 + k) if chan else 0.2, order, t
    yield 'science', SCI_N, SCI_SIGMA, 1, ripple(SCI_N, SCI_PERIOD)
