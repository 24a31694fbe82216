"""What every entry point that checks the likelihood options before its first device call says to every pair of options and
to each option's invalid values: one line per input and outcome -- the exception's type and message or `passed the checks` --
with the entry points that gave it (the runners' `from_data` by their models' names; `all`: every entry point, which is the
rule).  Runs without a GPU: the engine's loader is replaced by one that raises, and reaching it is what passing the checks
means.  The output of two commits is compared with diff (profiles/likelihood_options/).

    python scripts/likelihood_option_cases.py > cases.txt
"""
import itertools
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import nestfit_amd as na                                     # noqa: E402
from nestfit_amd import _ffi                                 # noqa: E402
from nestfit_amd.cube import CubeRunner                      # noqa: E402
from nestfit_amd.cubeio import CubeStack, DataCube, SimpleCube  # noqa: E402
from nestfit_amd.fitter import CubeFitter                    # noqa: E402

N = 32
X = np.linspace(1.0e11, 1.0001e11, N)


class Device(Exception):
    """The first device call."""


def _no_device(*args, **kwargs):
    raise Device()


_ffi.engine = _ffi.load = _no_device


def valid(n_spec):
    """The smallest valid value that switches each option on, for `n_spec` spectra of N channels."""
    return {'baseline_order': 1, 'layered': True, 'calibration': 0.1, 'noise_uncertainty': 0.1, 'correlation': na.HANNING,
            'response': na.HANNING_RESPONSE, 'templates': [na.ripple(N, 9.3)] + [None] * (n_spec - 1), 'continuum': 3.0,
            'robust': 4}


# each option's invalid values, as the CPU tests of the options give them (for two spectra where the length matters)
INVALID = {
    'baseline_order': (True, 4, -2, 1.5, 'one'),
    'layered': (None, 1, 'yes'),
    'calibration': (-0.1, 1.5, float('nan'), [0.1, 0.1, 0.1], 'ten percent', True, []),
    'noise_uncertainty': (0.6, -0.1, float('nan'), [0.1, 0.1, 0.1], 'some', True, []),
    'correlation': ((1.0, 0.5), (0.5, -0.9), (0.5,), (0.5, float('nan')), 'hanning', np.full((3, 2), 0.1), (0.999, 0.998)),
    'response': ((0.5, 0.5, 0.5), (0.25, 0.75), (1.0, -1.0, 1.0), (0.25, float('inf'), 0.25), 'hanning', np.full((3, 3), 1.0 / 3.0)),
    'templates': ('ripple', [], [np.zeros((1, N)), None, None], [np.ones((5, N)), None], [np.ones((1, N - 1)), None],
                  [np.full((1, N), np.nan), None], [np.zeros((1, N)), None]),
    'continuum': (-1.0, float('nan'), [1.0, 2.0, 3.0], True, 'bright', np.ones((2, 2, 2))),
    'robust': (0.5, -4, 1e6 + 1, float('nan'), [4.0, 4.0, 4.0], 'heavy', True, []),
}


def _noise(masked):
    if not masked:
        return 0.1
    noise = np.full(N, 0.1)
    noise[5] = np.inf
    return noise


def _stack(continuum):
    cubes = []
    for trans in (1, 2):
        hdr = {'SIMPLE': True, 'BITPIX': -64, 'NAXIS': 3, 'NAXIS1': 3, 'NAXIS2': 3, 'NAXIS3': N, 'BUNIT': 'K',
               'CTYPE1': 'RA---SIN', 'CTYPE2': 'DEC--SIN', 'CTYPE3': 'FREQ', 'CUNIT3': 'Hz', 'CRVAL3': float(X[0]),
               'CDELT3': float(X[1] - X[0]), 'CRPIX3': 1.0, 'RESTFRQ': float(X[N // 2])}
        cubes.append(DataCube(SimpleCube(hdr, np.zeros((N, 3, 3))), 0.1, trans_id=trans, continuum=continuum if trans == 1 else None))
    return CubeStack(cubes)


MOL, ISO = na.Molecule('mol', [5.0, 10.0, 20.0], [1.0, 2.0, 4.0]), na.Molecule('iso', [5.0, 10.0, 20.0], [1.5, 3.0, 6.0])
MIX = na.LteMix([MOL, ISO])


def entry_points():
    """(name, n_spec, call(masked, **options)): each runner's from_data, CubeRunner and CubeFitter as the CPU tests build them."""
    rows = lambda masked, *last: [[X, np.zeros(N), _noise(masked), v] for v in last]
    table = na.LineTable(1e11, [0.0], [1.0])
    lines = [MOL.transition(1.00005e11, 10.0, 3.0, 1e-6), MOL.transition(1.00006e11, 20.0, 5.0, 2e-6)]
    blend = [lines[0], ISO.transition(1.00004e11, 10.0, 3.0, 1e-6)]
    yield 'Ammonia', 2, lambda masked, **kw: na.AmmoniaRunner.from_data(rows(masked, 1, 2), None, **kw)
    yield 'Diazenylium', 2, lambda masked, **kw: na.DiazenyliumRunner.from_data(rows(masked, 1, 2), None, **kw)
    yield 'Gaussian', 1, lambda masked, **kw: na.GaussianRunner.from_data(rows(masked, 1.00005e11)[0], None, **kw)
    yield 'Hyperfine', 2, lambda masked, **kw: na.HyperfineRunner.from_data(rows(masked, table, table), None, **kw)
    yield 'Lte', 2, lambda masked, **kw: na.LteRunner.from_data(rows(masked, *lines), None, **kw)
    yield 'LteMix', 2, lambda masked, **kw: MIX.Runner.from_data(rows(masked, *blend), None, **kw)

    def cube(masked, **kw):
        noise = np.tile(_noise(True), (1, 2)) if masked else np.full((1, 2), 0.1)
        return CubeRunner([X, X], (1, 2), np.zeros((1, 2 * N)), noise, None, **kw)
    yield 'CubeRunner', 2, cube

    def fitter(masked, **kw):                                # (its continuum comes from the stack's maps; it asks no mask)
        tc = kw.pop('continuum', None)
        return CubeFitter(_stack(tc), None, na.AmmoniaRunner, runner_kwargs=kw)
    yield 'CubeFitter', 2, fitter
    yield 'CubeFitter(kwargs)', 2, lambda masked, **kw: CubeFitter(_stack(None), None, na.AmmoniaRunner, runner_kwargs=kw)


def outcome(call, masked, kw):
    try:
        call(masked, **kw)
    except Device:
        return 'passed the checks'
    except (ValueError, TypeError) as e:
        return f'{type(e).__name__}: {e}'
    except Exception as e:                                   # nothing else is expected before the device
        return f'passed the checks ({type(e).__name__})'
    return 'passed the checks'


def show(v):
    return ' '.join(repr(v).split())


def cases(n_spec):
    """(label, masked, keywords) of every input: nothing, each option alone, every pair, each invalid value."""
    on = valid(n_spec)
    yield 'nothing', False, {}
    yield 'masked', True, {}
    for a in on:
        yield a, False, {a: on[a]}
        yield f'masked + {a}', True, {a: on[a]}
    for a, b in itertools.combinations(on, 2):
        yield f'{a} + {b}', False, {a: on[a], b: on[b]}
    for a, values in INVALID.items():
        for v in values:
            yield f'{a}={show(v)}', False, {a: v}


def main():
    """One line per input and distinct outcome, with the entry points that gave it (`all`: the nine of them)."""
    said = {}                                                # label -> outcome -> the entry points that gave it
    names = []
    for name, n_spec, call in entry_points():
        names.append(name)
        for label, masked, kw in cases(n_spec):
            said.setdefault(label, {}).setdefault(outcome(call, masked, kw), []).append(name)
    for label, outcomes in said.items():
        for what, who in outcomes.items():
            print(f'{label} | {"all" if who == names else ", ".join(who)} | {what}')


if __name__ == '__main__':
    main()
