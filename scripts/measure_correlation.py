"""usage: python scripts/measure_correlation.py [--ncomp 2,4] [--steps N] [--warmup W] [--reps R] [--out FILE]

lnL evaluations/s at the metric shape -- 4096-row batches, two spectra of 1024 channels -- of one weighted spectra set (a
noise per channel, constant over each spectrum) against the same data with correlated channel noise (`correlation=HANNING`,
nfa_specset_set_correlation: lnl_kernel_side (corr), the weighted form in the general component form with rows of 62 channels and
two more loads and a neighbour product per row), in the table mode (the unit queue off, which weighted sets skip anyway) and
the fast mode.  --ncomp 4: both sets take the general component form, so the kernels differ by the correlation alone (34
rows of 62 channels against 32 of 64, the halo lanes' model values, two DPP shifts and a fused multiply-add chain per row).
--ncomp 2: the weighted side is the UNROLLED form (NCOMP = 2, packed windows), the correlated side the general form; the
general form alone costs about 1.2 x, and the two are not timed apart here.  The data are the model plus
Hanning-smoothed white noise.  Device-pointer batches (nfa_runner_loglike_batch_dev) like bench.py; the sets are timed in
turn, R times each, and the median of each is reported.  One JSON line per (mode, set)."""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import nestfit_amd as na                        # noqa: E402
from nestfit_amd import _ffi                    # noqa: E402
from nestfit_amd.cube import CubeRunner         # noqa: E402
from nestfit_amd.synth import TRUTH_2COMP, freq_axis      # noqa: E402

ROWS, N_CHAN, N_PIX, TRANS = 4096, 1024, 16, (1, 2)


def make_sets(NCOMP):
    rng = np.random.default_rng(17)
    axes = [freq_axis(t, N_CHAN) for t in TRANS]
    ut = na.get_irdc_priors(size=500, vsys=0.0)
    noise = rng.uniform(0.15, 0.3, (N_PIX, len(TRANS)))
    zero = CubeRunner(axes, TRANS, np.zeros((N_PIX, 2 * N_CHAN)), noise, ut, ncomp=NCOMP)
    # (four components: the truth's two, and the two again 4 km/s further on)
    truth = TRUTH_2COMP if NCOMP == 2 else np.concatenate([TRUTH_2COMP.reshape(6, 2), TRUTH_2COMP.reshape(6, 2) + np.eye(6)[:, :1] * 4.0], axis=1).ravel()
    theta = np.repeat(truth[None, :], N_PIX, axis=0)
    theta[:, :NCOMP] += 0.3 * np.arange(N_PIX)[:, None]
    spec, _ = zero.predict_batch(np.arange(N_PIX, dtype=np.int32), theta)
    flat = np.repeat(noise, N_CHAN, axis=1)
    white = rng.normal(0, 1, (N_PIX, 2 * N_CHAN + 2))
    smooth = (0.25 * white[:, :-2] + 0.5 * white[:, 1:-1] + 0.25 * white[:, 2:]) / np.sqrt(0.375)      # unit variance, rho = HANNING
    data = spec + smooth * flat
    make = lambda **kw: CubeRunner(axes, TRANS, data, flat, ut, ncomp=NCOMP, **kw)
    return {'weighted': make(), 'correlated': make(correlation=na.HANNING)}


def time_steps(lib, runner, d_pix, d_u, d_l, U_all, steps, warmup):
    step_bytes = ROWS * runner.ndim * 8
    _ffi.check(lib.nfa_memcpy_h2d(d_u, U_all.ctypes.data_as(C.c_void_p), U_all.nbytes))
    _ffi.check(lib.nfa_device_synchronize())
    h = runner._run.handle

    def step(k):
        _ffi.check(lib.nfa_runner_loglike_batch_dev(h, C.c_void_p(d_pix.value + k * ROWS * 4),
                                                    C.c_void_p(d_u.value + k * step_bytes),
                                                    C.c_void_p(d_l.value + k * ROWS * 8), ROWS))
    for k in range(warmup):
        step(k)
    _ffi.check(lib.nfa_runner_synchronize(h))
    _ffi.check(lib.nfa_device_synchronize())
    t0 = time.perf_counter()
    for k in range(warmup, warmup + steps):
        step(k)
    _ffi.check(lib.nfa_runner_synchronize(h))
    _ffi.check(lib.nfa_device_synchronize())
    return time.perf_counter() - t0


def measure(lib, sets, NCOMP, args, lines):
    n = args.steps + args.warmup
    ndim = 6 * NCOMP
    rng = np.random.default_rng(3)
    U_all = np.ascontiguousarray(rng.uniform(size=(n, ROWS, ndim)))
    pix = np.ascontiguousarray(rng.integers(0, N_PIX, (n, ROWS)).astype(np.int32))
    d_pix, d_u, d_l = C.c_void_p(), C.c_void_p(), C.c_void_p()
    _ffi.check(lib.nfa_malloc(C.byref(d_pix), pix.nbytes))
    _ffi.check(lib.nfa_malloc(C.byref(d_u), U_all.nbytes))
    _ffi.check(lib.nfa_malloc(C.byref(d_l), n * ROWS * 8))
    _ffi.check(lib.nfa_memcpy_h2d(d_pix, pix.ctypes.data_as(C.c_void_p), pix.nbytes))
    try:
        for mode in ('table', 'fast'):
            _ffi.set_option('lnl_queue', 0)                 # (weighted sets never take the queue form)
            for r in sets.values():
                r.set_exp_mode(mode)
            secs = {name: [] for name in sets}
            for _ in range(args.reps):
                for name, r in sets.items():
                    secs[name].append(time_steps(lib, r, d_pix, d_u, d_l, U_all, args.steps, args.warmup))
            base = np.median(secs['weighted'])
            for name, s in secs.items():
                med = float(np.median(s))
                rec = {'mode': mode, 'set': name, 'rows': ROWS, 'spectra': len(TRANS), 'channels': N_CHAN, 'ncomp': NCOMP,
                       'steps': args.steps, 'reps': args.reps, 'evals_per_s': ROWS * args.steps / med,
                       'evals_per_s_spread': [ROWS * args.steps / max(s), ROWS * args.steps / min(s)],
                       'time_vs_weighted': med / base}
                lines.append(rec)
                print(json.dumps(rec), flush=True)
    finally:
        _ffi.set_option('lnl_queue', 1)
        for p in (d_pix, d_u, d_l):
            lib.nfa_free(p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ncomp', default='2,4')
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if na.device_count() < 1:
        sys.exit('measure_correlation: no GPU')
    lib = _ffi.load()
    lines = []
    for NCOMP in (int(v) for v in args.ncomp.split(',')):
        measure(lib, make_sets(NCOMP), NCOMP, args, lines)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(''.join(json.dumps(x) + '\n' for x in lines))


if __name__ == '__main__':
    main()
