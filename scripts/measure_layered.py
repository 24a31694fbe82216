"""usage: python scripts/measure_layered.py [--steps N] [--warmup W] [--reps R] [--ncomp 2 4] [--out FILE]

lnL evaluations/s of a LAYERED spectra set (CubeRunner(..., layered=True): nfa_specset_set_layered) against the
summed set on the same tables, data and priors at the metric shape: 4096-row batches, two spectra of 1024 channels, in the
table mode and the fast mode -- the LTE mix of scripts/measure_lte_mix.py, two species, five parameters per component.
Measured at TWO and at FOUR components:

  * at four both runners take the general component form of the likelihood kernel, so the ratio is the price of the
    layered update itself: one subtraction per (channel, component) at the sites that add to the model;
  * at two the summed set takes the unrolled form (NCOMP = 2; in the table mode the queue form) and the layered one the
    general form, so the ratio also holds the general form against the unrolled one.

In the table mode the summed set's large launches take the queue form, which a layered set never takes; there a third
route, the summed set with option lnl_queue 0 (the plain form, like the layered set's), is timed as well.

Device-pointer batches (nfa_runner_loglike_batch_dev) like bench.py; the routes alternate in one process, R times each, and
the median of each is reported.  One JSON line per (ncomp, mode, set); time_vs_summed is against the summed set as it runs
by default, time_vs_summed_plain (table mode) against the summed set without the queue."""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'scripts'))

import nestfit_amd as na                        # noqa: E402
from nestfit_amd import _ffi                    # noqa: E402
from nestfit_amd.cube import CubeRunner         # noqa: E402
from nestfit_amd.lte import CKMS                # noqa: E402
import measure_lte_mix as mm                    # noqa: E402  (the species, the priors and the timed loop)

ROWS, N_CHAN, N_PIX = mm.ROWS, mm.N_CHAN, mm.N_PIX
RANGES = mm.RANGES['mix']


def make_sets(ncomp):
    """The summed and the layered runner of `ncomp` components on one set of tables, axes, data and noise."""
    rng = np.random.default_rng(17)
    bands = mm.top_bands()
    axes = [b.nu * (1.0 - np.linspace(36.0, -14.0, N_CHAN) / CKMS) for b in bands]
    noise = rng.uniform(0.15, 0.3, (N_PIX, 2))
    zero = CubeRunner(axes, None, np.zeros((N_PIX, 2 * N_CHAN)), noise, None, ncomp=mm.NCOMP, model=4, lines=bands)
    theta = np.repeat(mm.TRUTH[None, :], N_PIX, axis=0)
    theta[:, :mm.NCOMP] += 0.2 * np.arange(N_PIX)[:, None]
    spec, _ = zero.predict_batch(np.arange(N_PIX, dtype=np.int32), theta)
    data = spec + rng.normal(0, 1, spec.shape) * np.repeat(noise, N_CHAN, axis=1)
    species, blends = mm.as_mix(bands)
    return {name: CubeRunner(axes, None, data, noise, mm.uniform_priors(RANGES), ncomp=ncomp, model=4, lines=blends,
                             species=species, layered=name == 'layered') for name in ('summed', 'layered')}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=60)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--ncomp', type=int, nargs='+', default=[2, 4])
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if na.device_count() < 1:
        sys.exit('measure_layered: no GPU')
    lib = _ffi.load()
    n = args.steps + args.warmup
    rng = np.random.default_rng(3)
    U_all = np.ascontiguousarray(rng.uniform(size=(n, ROWS, 5 * max(args.ncomp))))
    pix = np.ascontiguousarray(rng.integers(0, N_PIX, (n, ROWS)).astype(np.int32))
    d_pix, d_u, d_l = C.c_void_p(), C.c_void_p(), C.c_void_p()
    _ffi.check(lib.nfa_malloc(C.byref(d_pix), pix.nbytes))
    _ffi.check(lib.nfa_malloc(C.byref(d_u), U_all.nbytes))
    _ffi.check(lib.nfa_malloc(C.byref(d_l), n * ROWS * 8))
    _ffi.check(lib.nfa_memcpy_h2d(d_pix, pix.ctypes.data_as(C.c_void_p), pix.nbytes))
    lines = []
    try:
        for ncomp in args.ncomp:
            for mode in ('table', 'fast'):
                sets = make_sets(ncomp)
                for r in sets.values():
                    r.set_exp_mode(mode)
                routes = [('summed', 'summed', None), ('layered', 'layered', None)] + ([('summed lnl_queue=0', 'summed', 0)] if mode == 'table' else [])
                secs = {name: [] for name, _, _ in routes}
                finite = {}
                for _ in range(args.reps):
                    for name, which, queue in routes:
                        r = sets[which]
                        if queue is not None:
                            _ffi.set_option('lnl_queue', queue)
                        try:
                            secs[name].append(mm.time_steps(lib, r, d_pix, d_u, d_l, U_all, args.steps, args.warmup))
                        finally:
                            if queue is not None:
                                _ffi.set_option('lnl_queue', 1)
                        out = np.empty(n * ROWS)
                        _ffi.check(lib.nfa_memcpy_d2h(out.ctypes.data_as(C.c_void_p), d_l, out.nbytes))
                        finite[name] = bool(np.isfinite(out).all())
                base = float(np.median(secs['summed']))
                plain = float(np.median(secs['summed lnl_queue=0'])) if mode == 'table' else None
                for name, s in secs.items():
                    med = float(np.median(s))
                    rec = {'ncomp': ncomp, 'mode': mode, 'set': name, 'rows': ROWS, 'spectra': 2, 'channels': N_CHAN,
                           'npar': sets[name.split()[0]].n_model,
                           'steps': args.steps, 'reps': args.reps, 'evals_per_s': ROWS * args.steps / med,
                           'evals_per_s_spread': [ROWS * args.steps / max(s), ROWS * args.steps / min(s)],
                           'time_vs_summed': med / base, 'time_vs_summed_plain': med / plain if plain else None,
                           'lnl_all_finite': finite[name]}
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
