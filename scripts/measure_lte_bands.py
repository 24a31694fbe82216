"""usage: python scripts/measure_lte_bands.py [--steps N] [--warmup W] [--reps R] [--out FILE] [--no-trace]

lnL evaluations/s of LTE bands (CubeRunner model 4 on LteBands: nfa_specset_create_lte_bands) against the
hyperfine model on the same lines as constant tables (model 3: nfa_specset_create_lines) at the metric shape: 4096-row
batches, two spectra of 1024 channels, two components, in the table mode and the fast mode.  The species is a symmetric
top made here from closed forms; each spectrum is a band of four transitions (K = 0..3 of one J) of a single line each,
and the hyperfine set has the same eight lines with their optical-depth ratios at 20 K as weights.  The likelihood
kernels are shared; what differs is one extra launch per group, lte_band_kernel: one exp and two expm1 per (item,
component, spectrum, transition).  Device-pointer batches (nfa_runner_loglike_batch_dev) like bench.py; the two sets
alternate in one process, R times each, and the median of each is reported.  Then, unless --no-trace, one run of the
banded set under `rocprofv3 --kernel-trace --stats` (a fresh child process, no counters) gives the mean time per launch
of lte_band_kernel and of the set-up kernel.  One JSON line per (mode, set)."""
import argparse
import csv
import ctypes as C
import json
import math
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import nestfit_amd as na                        # noqa: E402
from nestfit_amd import _ffi                    # noqa: E402
from nestfit_amd.cube import CubeRunner         # noqa: E402
from nestfit_amd.lte import CCMS, CKMS, H_CGS, KB_CGS   # noqa: E402

ROWS, N_CHAN, NCOMP, N_PIX = 4096, 1024, 2, 16
A_ROT, B_ROT, D_JK, MU = 200e9, 4.0e9, 33.4e3, 3.9e-18
RANGES = {'bands': [(-6.0, 6.0), (6.0, 60.0), (13.0, 15.0), (0.1, 1.5)],         # voff, tex, lncol, sigm
          'hyperfine': [(-6.0, 6.0), (6.0, 60.0), (-1.5, 1.0), (0.1, 1.5)]}      # voff, tex, ltau, sigm
TRUTH = np.array([-1.0, 2.0, 20.0, 35.0, 14.5, 14.2, 0.4, 0.7])
T_WEIGHTS = 20.0                                # K: the temperature the constant tables' weights are right at


def spin_weight(K):
    return 1.0 if K == 0 else 4.0 if K % 3 == 0 else 2.0


def top_bands():
    """The bands of J = 5-4 and 6-5, K = 0..3 each, of a symmetric top with its partition function on 32 temperatures."""
    temps = np.geomspace(5.0, 80.0, 32)
    q = [sum((2 * J + 1) * spin_weight(K) * math.exp(-H_CGS * (B_ROT * J * (J + 1) + (A_ROT - B_ROT) * K * K) / (KB_CGS * T))
             for J in range(200) for K in range(J + 1)) for T in temps]
    mol = na.Molecule('top', temps, q)

    def trans(J, K):
        Jp = J + 1
        nu = 2.0 * Jp * (B_ROT - D_JK * K * K)
        a_ul = 64.0 * math.pi ** 4 * nu ** 3 * MU ** 2 * (Jp * Jp - K * K) / (3.0 * H_CGS * CCMS ** 3 * Jp * (2 * Jp + 1))
        return mol.transition(nu, H_CGS * (B_ROT * Jp * (Jp + 1) + (A_ROT - B_ROT) * K * K) / KB_CGS, (2 * Jp + 1) * spin_weight(K), a_ul)
    return [mol.band([trans(J, K) for K in range(4)]) for J in (4, 5)]


def constant_tables(bands):
    """The bands' lines as LineTables about each band's first transition, weighted by tau_main at T_WEIGHTS relative to
    the first band's first transition."""
    ref = float(bands[0][0].tau_main(T_WEIGHTS, 14.0, 0.5))
    return [na.LineTable(b.nu, [(1.0 - t.nu / b.nu) * CKMS for t in b], [float(t.tau_main(T_WEIGHTS, 14.0, 0.5)) / ref for t in b])
            for b in bands]


def uniform_priors(ranges, size=500):
    u = np.linspace(0, 1, size)
    return na.PriorTransformer([na.Prior(na.Distribution(lo + u * (hi - lo), np.full(size, 1.0 / (hi - lo))), k)
                                for k, (lo, hi) in enumerate(ranges)])


def make_sets(only=None):
    rng = np.random.default_rng(17)
    bands = top_bands()
    axes = [b.nu * (1.0 - np.linspace(36.0, -14.0, N_CHAN) / CKMS) for b in bands]
    noise = rng.uniform(0.15, 0.3, (N_PIX, 2))
    zero = CubeRunner(axes, None, np.zeros((N_PIX, 2 * N_CHAN)), noise, None, ncomp=NCOMP, model=4, lines=bands)
    theta = np.repeat(TRUTH[None, :], N_PIX, axis=0)
    theta[:, :NCOMP] += 0.2 * np.arange(N_PIX)[:, None]
    spec, _ = zero.predict_batch(np.arange(N_PIX, dtype=np.int32), theta)
    data = spec + rng.normal(0, 1, spec.shape) * np.repeat(noise, N_CHAN, axis=1)
    plain = constant_tables(bands)
    make = {'hyperfine': lambda: CubeRunner(axes, None, data, noise, uniform_priors(RANGES['hyperfine']), ncomp=NCOMP, model=3, lines=plain),
            'bands': lambda: CubeRunner(axes, None, data, noise, uniform_priors(RANGES['bands']), ncomp=NCOMP, model=4, lines=bands)}
    return {name: f() for name, f in make.items() if only in (None, name)}


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


def kernel_times(mode, steps, warmup):
    """Mean time per launch of lte_band_kernel and of the set-up kernel of the banded set, from a child of this script
    under rocprofv3 (kernel trace and statistics only); None (and a message on stderr) where the profiler is missing or
    its output is not understood."""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', tmp, '--', sys.executable, __file__,
               '--trace-set', 'bands', '--mode', mode, '--steps', str(steps), '--warmup', str(warmup), '--reps', '1', '--no-trace']
        try:
            subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=240)
        except (OSError, subprocess.SubprocessError) as e:
            print(f'measure_lte_bands: no kernel trace of {mode}: {e}', file=sys.stderr)
            return None
        found = {}
        for path in Path(tmp).rglob('*kernel_stats.csv'):
            with open(path) as f:
                for row in csv.DictReader(f):
                    for key in ('lte_band_kernel', 'setup_kernel'):
                        if key in row.get('Name', ''):
                            found[key] = {'kernel': row['Name'].split('(')[0], 'calls': int(row['Calls']), 'mean_us': float(row['AverageNs']) / 1e3}
    if 'lte_band_kernel' not in found:
        print(f'measure_lte_bands: no lte_band_kernel in the trace of {mode}', file=sys.stderr)
        return None
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=60)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-trace', action='store_true')
    ap.add_argument('--trace-set', default=None, help='run this set alone (the child under the profiler)')
    ap.add_argument('--mode', default=None, help='table or fast alone')
    args = ap.parse_args()
    if na.device_count() < 1:
        sys.exit('measure_lte_bands: no GPU')
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
        for mode in ((args.mode,) if args.mode else ('table', 'fast')):
            sets = make_sets(args.trace_set)
            for r in sets.values():
                r.set_exp_mode(mode)
            secs = {name: [] for name in sets}
            finite = {}
            for _ in range(args.reps):
                for name, r in sets.items():
                    secs[name].append(time_steps(lib, r, d_pix, d_u, d_l, U_all, args.steps, args.warmup))
                    out = np.empty(n * ROWS)
                    _ffi.check(lib.nfa_memcpy_d2h(out.ctypes.data_as(C.c_void_p), d_l, out.nbytes))
                    finite[name] = bool(np.isfinite(out).all())
            base = np.median(secs['hyperfine']) if 'hyperfine' in secs else None
            for name, s in secs.items():
                med = float(np.median(s))
                rec = {'mode': mode, 'set': name, 'lines': [4, 4], 'rows': ROWS, 'spectra': 2, 'channels': N_CHAN, 'ncomp': NCOMP,
                       'steps': args.steps, 'reps': args.reps, 'evals_per_s': ROWS * args.steps / med,
                       'evals_per_s_spread': [ROWS * args.steps / max(s), ROWS * args.steps / min(s)],
                       'time_vs_hyperfine': med / base if base else None, 'lnl_all_finite': finite[name]}
                if not args.no_trace and name == 'bands':
                    rec['kernels'] = kernel_times(mode, args.steps, args.warmup)
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
