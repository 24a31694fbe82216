"""usage: python scripts/measure_continuum.py [--ncomp 2,4] [--steps N] [--warmup W] [--reps R] [--out FILE]

lnL evaluations/s at the metric shape -- 4096-row batches, two spectra of 1024 channels, a noise per channel -- of spectra sets
on the same data: the weighted set, the set with a baseline of order 1 (the baseline kind), the same set layered (the baseline
kind in the general component form, which is the form lnl_kernel_side (cont) has), and the sets with a continuum background of 30 K
per (pixel, spectrum) behind them (`continuum=`, lnl_kernel_side (cont): one more add per visited row and lane), with the baseline
and without one (a zeroed record), summed and layered.  At four components every set runs the general component form and
`time_vs_baseline` of the set 'continuum' is the feature's own cost; at two the baseline set is the UNROLLED form (NCOMP = 2,
packed windows) and that ratio is the form's cost -- `time_vs_general`, against the layered baseline set, leaves it out.
Table and fast mode, the sets timed in turn, R times each, the median of each reported: the set-up, the timing loop and the
record of scripts/measure_correlation.py.  One JSON line per (mode, set)."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'scripts'))

import nestfit_amd as na                        # noqa: E402
from nestfit_amd import _ffi                    # noqa: E402
import measure_correlation as mc                # noqa: E402

TC = 30.0


def make_sets(NCOMP):
    """measure_correlation's weighted set, and the same data behind a baseline, a layered baseline and a continuum."""
    sets = {'weighted': mc.make_sets(NCOMP)['weighted']}
    base = sets['weighted']
    make = lambda **kw: mc.CubeRunner(base._ss.xarrs, mc.TRANS, base._data, base._noise, base.utrans, ncomp=NCOMP, **kw)
    tc = np.full((mc.N_PIX, len(mc.TRANS)), TC)
    tc[::4, 1] = 0.0                                # (a spectrum with Tc = 0 beside one with a continuum)
    sets['baseline'] = make(baseline_order=1)
    sets['baseline_general'] = make(baseline_order=1, layered=True)
    sets['continuum'] = make(baseline_order=1, continuum=tc)
    sets['continuum_layered'] = make(baseline_order=1, layered=True, continuum=tc)
    sets['continuum_no_baseline'] = make(continuum=tc)
    return sets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ncomp', default='2,4')
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if na.device_count() < 1:
        sys.exit('measure_continuum: no GPU')
    lib = _ffi.load()
    lines = []
    for NCOMP in (int(v) for v in args.ncomp.split(',')):
        at = len(lines)
        mc.measure(lib, make_sets(NCOMP), NCOMP, args, lines)
        for mode in ('table', 'fast'):
            recs = [r for r in lines[at:] if r['mode'] == mode]
            bl = next(r for r in recs if r['set'] == 'baseline')
            gen = next(r for r in recs if r['set'] == 'baseline_general')
            for r in recs:
                r['time_vs_baseline'] = bl['evals_per_s'] / r['evals_per_s']
                r['time_vs_general'] = gen['evals_per_s'] / r['evals_per_s']
                print(json.dumps({k: r[k] for k in ('mode', 'ncomp', 'set', 'evals_per_s', 'time_vs_weighted', 'time_vs_baseline', 'time_vs_general')}),
                      flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(''.join(json.dumps(x) + '\n' for x in lines))


if __name__ == '__main__':
    main()
