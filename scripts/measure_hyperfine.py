"""usage: python scripts/measure_hyperfine.py [--steps N] [--warmup W] [--reps R] [--out FILE]

lnL evaluations/s of the N2H+ model on its shipped tables (DiazenyliumRunner's route: nfa_specset_create_model) against
the hyperfine model on copies of the same tables handed in by the caller (LineTable.builtin -> nfa_specset_create_lines):
4096-row batches, two spectra of 1024 channels, two components, in the table mode and the fast mode, at two shapes:
"wide" (J = 1-0 and 2-1: 15 and 40 lines, the WIDE kernel forms) and "narrow" (J = 1-0 twice: at most 26 lines, the forms
the headline benchmark and most tables of one's own take).
Both routes fill the same per-spectrum line rows and run the same kernel instance on the same numbers, so the expectation
is equality.  Device-pointer batches (nfa_runner_loglike_batch_dev) like bench.py; the two sets alternate in one process,
R times each, and the median of each is reported.  One JSON line per (shape, mode, set)."""
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

ROWS, N_CHAN, NCOMP, N_PIX = 4096, 1024, 2, 16
SHAPES = {'wide': (1, 2), 'narrow': (1, 1)}
CKMS = 299792.458
RANGES = [(-6.0, 6.0), (2.8, 20.0), (-1.5, 1.0), (0.1, 1.5)]          # voff, tex, ltau, sigm
TRUTH = np.array([-1.0, 2.0, 8.0, 5.0, 0.3, -0.2, 0.4, 0.7])


def uniform_priors(size=500):
    u = np.linspace(0, 1, size)
    return na.PriorTransformer([na.Prior(na.Distribution(lo + u * (hi - lo), np.full(size, 1.0 / (hi - lo))), k)
                                for k, (lo, hi) in enumerate(RANGES)])


def make_sets(TRANS):
    rng = np.random.default_rng(17)
    tables = [na.LineTable.builtin('diazenylium', t) for t in TRANS]
    axes = [tab.nu * (1.0 - np.linspace(20.0, -20.0, N_CHAN) / CKMS) for tab in tables]
    ut = uniform_priors()
    noise = rng.uniform(0.15, 0.3, (N_PIX, len(TRANS)))
    zero = CubeRunner(axes, TRANS, np.zeros((N_PIX, 2 * N_CHAN)), noise, ut, ncomp=NCOMP, model=1)
    theta = np.repeat(TRUTH[None, :], N_PIX, axis=0)
    theta[:, :NCOMP] += 0.2 * np.arange(N_PIX)[:, None]
    spec, _ = zero.predict_batch(np.arange(N_PIX, dtype=np.int32), theta)
    data = spec + rng.normal(0, 1, spec.shape) * np.repeat(noise, N_CHAN, axis=1)
    return {'diazenylium': CubeRunner(axes, TRANS, data, noise, ut, ncomp=NCOMP, model=1),
            'hyperfine': CubeRunner(axes, None, data, noise, ut, ncomp=NCOMP, model=3, lines=tables)}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=60)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if na.device_count() < 1:
        sys.exit('measure_hyperfine: no GPU')
    lib = _ffi.load()
    n = args.steps + args.warmup
    ndim = 4 * NCOMP
    rng = np.random.default_rng(3)
    U_all = np.ascontiguousarray(rng.uniform(size=(n, ROWS, ndim)))
    pix = np.ascontiguousarray(rng.integers(0, N_PIX, (n, ROWS)).astype(np.int32))
    d_pix, d_u, d_l = C.c_void_p(), C.c_void_p(), C.c_void_p()
    _ffi.check(lib.nfa_malloc(C.byref(d_pix), pix.nbytes))
    _ffi.check(lib.nfa_malloc(C.byref(d_u), U_all.nbytes))
    _ffi.check(lib.nfa_malloc(C.byref(d_l), n * ROWS * 8))
    _ffi.check(lib.nfa_memcpy_h2d(d_pix, pix.ctypes.data_as(C.c_void_p), pix.nbytes))
    lines = []
    try:
        for shape, mode in ((s, m) for s in SHAPES for m in ('table', 'fast')):
            TRANS = SHAPES[shape]
            sets = make_sets(TRANS)
            for r in sets.values():
                r.set_exp_mode(mode)
            secs = {name: [] for name in sets}
            lnl = {}
            for _ in range(args.reps):
                for name, r in sets.items():
                    secs[name].append(time_steps(lib, r, d_pix, d_u, d_l, U_all, args.steps, args.warmup))
                    out = np.empty(n * ROWS)
                    _ffi.check(lib.nfa_memcpy_d2h(out.ctypes.data_as(C.c_void_p), d_l, out.nbytes))
                    lnl[name] = out
            same = bool(np.array_equal(lnl['diazenylium'], lnl['hyperfine'], equal_nan=True))
            base = np.median(secs['diazenylium'])
            for name, s in secs.items():
                med = float(np.median(s))
                rec = {'shape': shape, 'lines': [15 if t == 1 else 40 for t in TRANS], 'mode': mode, 'set': name, 'rows': ROWS, 'spectra': len(TRANS), 'channels': N_CHAN, 'ncomp': NCOMP,
                       'steps': args.steps, 'reps': args.reps, 'evals_per_s': ROWS * args.steps / med,
                       'evals_per_s_spread': [ROWS * args.steps / max(s), ROWS * args.steps / min(s)],
                       'time_vs_diazenylium': med / base, 'lnl_bits_equal': same}
                lines.append(rec)
                print(json.dumps(rec), flush=True)
    finally:
        for p in (d_pix, d_u, d_l):
            lib.nfa_free(p)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(''.join(json.dumps(x) + '\n' for x in lines))


if __name__ == '__main__':
    main()
