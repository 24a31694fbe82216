"""usage: python scripts/measure_noise_uncertainty.py [--ncomp 2] [--steps N] [--warmup W] [--reps R] [--side S] [--out FILE]

What an uncertain noise level (`noise_uncertainty=0.2`) costs.  No likelihood kernel changes: the difference is
lnl_sum_nmarg_kernel's log1p and division per (item, spectrum) in place of lnl_sum_kernel's division, and in the device sampler
that kernel's launch per round, which the update kernel's own summing of the parts saves for every other set.

1. lnL evaluations/s at the metric shape -- 4096-row batches, two spectra of 1024 channels, ammonia (1,1) + (2,2) -- of the
   scalar-noise set (the headline's kind) and of scripts/measure_correlation.py's weighted set, each against the same set with
   the uncertainty, in the table and the fast mode: device-pointer batches like bench.py, the sets timed in turn, R times each,
   the median reported; the scalar set stands twice, first and last in the rotation (the place alone is worth 3 to 5 %).  One
   JSON line per (mode, set).
2. One config-5-style run of the device sampler: the S x S pixels (default 8 x 8) of `synth.c5_stack` -- two-component truths,
   1024 channels, 0.2 K -- fitted with two components, 400 live points, tol 0.5, efr 0.3, seed 5, with and without the
   uncertainty: seconds, evaluations and iterations per pixel, mean lnZ - null_lnZ.  One JSON line per run."""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'scripts'))

import nestfit_amd as na                        # noqa: E402
from nestfit_amd import _ffi, sampler           # noqa: E402
import measure_correlation as mc                # noqa: E402

F = 0.2


def make_sets(NCOMP):
    weighted = mc.make_sets(NCOMP)['weighted']
    scalar_noise = np.ascontiguousarray(weighted._noise[:, ::mc.N_CHAN])          # (constant over each spectrum)
    make = lambda noise, **kw: mc.CubeRunner(weighted._ss.xarrs, mc.TRANS, weighted._data, noise, weighted.utrans, ncomp=NCOMP, **kw)
    # (the scalar set stands twice, first and last in the rotation: what the place in the rotation alone is worth)
    return {'scalar': make(scalar_noise), 'scalar + uncertainty': make(scalar_noise, noise_uncertainty=F),
            'weighted': weighted, 'weighted + uncertainty': make(weighted._noise, noise_uncertainty=F),
            'scalar + nothing, last': make(scalar_noise)}


def measure(lib, sets, NCOMP, args, lines):
    n = args.steps + args.warmup
    rng = np.random.default_rng(3)
    U_all = np.ascontiguousarray(rng.uniform(size=(n, mc.ROWS, 6 * NCOMP)))
    pix = np.ascontiguousarray(rng.integers(0, mc.N_PIX, (n, mc.ROWS)).astype(np.int32))
    d_pix, d_u, d_l = C.c_void_p(), C.c_void_p(), C.c_void_p()
    _ffi.check(lib.nfa_malloc(C.byref(d_pix), pix.nbytes))
    _ffi.check(lib.nfa_malloc(C.byref(d_u), U_all.nbytes))
    _ffi.check(lib.nfa_malloc(C.byref(d_l), n * mc.ROWS * 8))
    _ffi.check(lib.nfa_memcpy_h2d(d_pix, pix.ctypes.data_as(C.c_void_p), pix.nbytes))
    try:
        for mode in ('table', 'fast'):
            for r in sets.values():
                r.set_exp_mode(mode)
            secs = {name: [] for name in sets}
            for _ in range(args.reps):
                for name, r in sets.items():
                    secs[name].append(mc.time_steps(lib, r, d_pix, d_u, d_l, U_all, args.steps, args.warmup))
            for name, s in secs.items():
                med = float(np.median(s))
                base = float(np.median(secs[name.split(' + ')[0]]))
                rec = {'what': 'batches', 'mode': mode, 'set': name, 'rows': mc.ROWS, 'spectra': len(mc.TRANS), 'channels': mc.N_CHAN,
                       'ncomp': NCOMP, 'steps': args.steps, 'reps': args.reps, 'evals_per_s': mc.ROWS * args.steps / med,
                       'evals_per_s_spread': [mc.ROWS * args.steps / max(s), mc.ROWS * args.steps / min(s)], 'time_vs_plain': med / base}
                lines.append(rec)
                print(json.dumps(rec), flush=True)
    finally:
        for p in (d_pix, d_u, d_l):
            lib.nfa_free(p)


def sampler_run(side, lines):
    from nestfit_amd.synth import c5_stack
    stack, truths, model, data, axes, ut = c5_stack(side, 1024, 0.2)
    na.set_exp_mode('fast')
    for f in (None, F, None, F):                                # (the first pair brings code objects and buffers up)
        cube, lon, lat = stack.to_device(ut, ncomp=2, noise_uncertainty=f)
        _ffi.check(_ffi.load().nfa_device_synchronize())
        t0 = time.perf_counter()
        res = sampler.fit_pixels(cube, np.arange(cube.n_pix), nlive=400, tol=0.5, efr=0.3, seed=5)
        seconds = time.perf_counter() - t0
        rec = {'what': 'sampler', 'mode': 'fast', 'noise_uncertainty': f, 'pixels': cube.n_pix, 'ncomp': 2, 'nlive': 400, 'seconds': seconds,
               'evals_per_pixel': float(np.mean([r.n_evals for r in res])), 'iterations_per_pixel': float(np.mean([r.n_iter for r in res])),
               'evals_per_s': float(sum(r.n_evals for r in res)) / seconds,
               'mean_lnZ_minus_null': float(np.mean([r.lnZ for r in res] - cube.null_lnZ))}
        lines.append(rec)
        print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ncomp', default='2')
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--side', type=int, default=8)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if na.device_count() < 1:
        sys.exit('measure_noise_uncertainty: no GPU')
    lib = _ffi.load()
    lines = []
    for NCOMP in (int(v) for v in args.ncomp.split(',')):
        measure(lib, make_sets(NCOMP), NCOMP, args, lines)
    if args.side > 0:
        sampler_run(args.side, lines)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(''.join(json.dumps(x) + '\n' for x in lines))


if __name__ == '__main__':
    main()
