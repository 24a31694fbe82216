"""usage: python scripts/measure_response.py [--ncomp 2,4] [--steps N] [--warmup W] [--reps R] [--out FILE]

lnL evaluations/s at the metric shape -- 4096-row batches, two spectra of 1024 channels, a noise per channel -- of three
spectra sets on the same data: the weighted set, the set with correlated channel noise (`correlation=HANNING`,
lnl_kernel_side (corr): rows of 62 channels) and the set with a channel response as well (`**na.smoothed(na.HANNING_RESPONSE)`,
lnl_kernel_side (resp): rows of 58 channels, four more wave shifts and five multiply-adds per visited row), and the response alone
(over white coefficients).  Table and fast mode, the sets timed in turn, R times each, the median of each reported: the
set-up, the timing loop and the record of scripts/measure_correlation.py, whose `time_vs_weighted` is kept and
`time_vs_correlated` added.  --ncomp 4: every set takes the general component form; --ncomp 2: the weighted side is the
unrolled form (see measure_correlation.py).  One JSON line per (mode, set)."""
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


def make_sets(NCOMP):
    """measure_correlation's two sets, and the same data behind a response: with the correlation that goes with it, and alone."""
    sets = mc.make_sets(NCOMP)
    base = sets['weighted']
    make = lambda **kw: mc.CubeRunner(base._ss.xarrs, mc.TRANS, base._data, base._noise, base.utrans, ncomp=NCOMP, **kw)
    sets['response'] = make(**na.smoothed(na.HANNING_RESPONSE))
    sets['response_only'] = make(response=na.HANNING_RESPONSE)
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
        sys.exit('measure_response: no GPU')
    lib = _ffi.load()
    lines = []
    for NCOMP in (int(v) for v in args.ncomp.split(',')):
        at = len(lines)
        mc.measure(lib, make_sets(NCOMP), NCOMP, args, lines)
        for mode in ('table', 'fast'):
            recs = [r for r in lines[at:] if r['mode'] == mode]
            corr = next(r for r in recs if r['set'] == 'correlated')
            for r in recs:
                r['time_vs_correlated'] = corr['evals_per_s'] / r['evals_per_s']
                print(json.dumps({k: r[k] for k in ('mode', 'ncomp', 'set', 'evals_per_s', 'time_vs_weighted', 'time_vs_correlated')}), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(''.join(json.dumps(x) + '\n' for x in lines))


if __name__ == '__main__':
    main()
