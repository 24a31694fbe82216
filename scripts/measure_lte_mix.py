"""usage: python scripts/measure_lte_mix.py [--steps N] [--warmup W] [--reps R] [--out FILE] [--no-trace]

lnL evaluations/s of an LTE mix (CubeRunner model 4 on two species: nfa_specset_create_lte_mix) against the
single-species band on the same lines (nfa_specset_create_lte_bands) at the metric shape: 4096-row batches, two spectra of
1024 channels, two components, in the table mode and the fast mode.  The species is a symmetric top made here from closed
forms; each spectrum is a band of four transitions (K = 0..3 of one J) of a single line each.  In the mix, K = 2 and 3
belong to a second molecule with a partition table of its own (the same numbers on another grid) and a column density of
its own: five parameters per component against four.  The likelihood kernels are shared; what differs is the small launch
between the stages -- lte_mix_kernel in lte_band_kernel's place: a log, an exp and an exp10 more per lane of the second
species, and two table scans -- and a fifth parameter per component in the set-up stage.  Device-pointer batches
(nfa_runner_loglike_batch_dev) like bench.py; the two sets alternate in one process, R times each, and the median of each
is reported.  Then, unless --no-trace, one run of the mix under `rocprofv3 --kernel-trace --stats` (a fresh child process,
no counters) gives the mean time per launch of lte_mix_kernel and of the set-up kernel.  One JSON line per (mode, set)."""
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
          'mix': [(-6.0, 6.0), (6.0, 60.0), (13.0, 15.0), (0.1, 1.5), (13.0, 15.0)]}        # ... and lncol2
TRUTH = np.array([-1.0, 2.0, 20.0, 35.0, 14.5, 14.2, 0.4, 0.7])


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


def as_mix(bands):
    """(species, blends): the bands with K = 2, 3 given to a second molecule -- the same partition function on 24
    temperatures of its own."""
    mol = bands[0].molecule
    temps = np.geomspace(4.0, 90.0, 24)
    other = na.Molecule('top-b', temps, mol.partition(temps))
    blends = [na.LteBlend(list(b[:2]) + [other.transition(t.nu, t.e_up, t.g_up, t.a_ul) for t in b[2:]]) for b in bands]
    return (mol, other), blends


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
    species, blends = as_mix(bands)
    make = {'bands': lambda: CubeRunner(axes, None, data, noise, uniform_priors(RANGES['bands']), ncomp=NCOMP, model=4, lines=bands),
            'mix': lambda: CubeRunner(axes, None, data, noise, uniform_priors(RANGES['mix']), ncomp=NCOMP, model=4, lines=blends,
                                      species=species)}
    return {name: f() for name, f in make.items() if only in (None, name)}


def time_steps(lib, runner, d_pix, d_u, d_l, U_all, steps, warmup):
    step_bytes = ROWS * runner.ndim * 8
    U_all = np.ascontiguousarray(U_all[:, :, :runner.ndim])          # (the band has four parameters per component, the mix five)
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
    """Mean time per launch of lte_mix_kernel and of the set-up kernel of the mix, from a child of this script
    under rocprofv3 (kernel trace and statistics only); None (and a message on stderr) where the profiler is missing or
    its output is not understood."""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', tmp, '--', sys.executable, __file__,
               '--trace-set', 'mix', '--mode', mode, '--steps', str(steps), '--warmup', str(warmup), '--reps', '1', '--no-trace']
        try:
            res = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=240)
        except OSError as e:                                  # no profiler on this machine: nothing ran
            print(f'measure_lte_mix: no kernel trace of {mode}: {e}', file=sys.stderr)
            return None
        # a child that was killed by a signal, ran out of time (TimeoutExpired, not caught) or failed has left the device in
        # an unknown state: nothing more is started on it
        if res.returncode != 0:
            sys.exit(f'measure_lte_mix: the traced run of {mode} ended with status {res.returncode}; stopping\n'
                     + res.stderr.decode(errors='replace')[-2000:])
        found = {}
        for path in Path(tmp).rglob('*kernel_stats.csv'):
            with open(path) as f:
                for row in csv.DictReader(f):
                    for key in ('lte_mix_kernel', 'setup_kernel'):
                        if key in row.get('Name', ''):
                            found[key] = {'kernel': row['Name'].split('(')[0], 'calls': int(row['Calls']), 'mean_us': float(row['AverageNs']) / 1e3}
    if 'lte_mix_kernel' not in found:
        print(f'measure_lte_mix: no lte_mix_kernel in the trace of {mode}', file=sys.stderr)
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
        sys.exit('measure_lte_mix: no GPU')
    lib = _ffi.load()
    n = args.steps + args.warmup
    ndim = 5 * NCOMP
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
            base = np.median(secs['bands']) if 'bands' in secs else None
            for name, s in secs.items():
                med = float(np.median(s))
                rec = {'mode': mode, 'set': name, 'lines': [4, 4], 'rows': ROWS, 'spectra': 2, 'channels': N_CHAN, 'ncomp': NCOMP,
                       'steps': args.steps, 'reps': args.reps, 'evals_per_s': ROWS * args.steps / med,
                       'evals_per_s_spread': [ROWS * args.steps / max(s), ROWS * args.steps / min(s)],
                       'time_vs_bands': med / base if base else None, 'lnl_all_finite': finite[name]}
                if not args.no_trace and name == 'mix':
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
