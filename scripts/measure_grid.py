"""usage: python scripts/measure_grid.py [--steps N] [--warmup W] [--reps R] [--out FILE] [--no-trace]

lnL evaluations/s of the excitation-grid model (CubeRunner model 5: nfa_specset_create_grid) against the
hyperfine model on copies of the same line tables (model 3: nfa_specset_create_lines) at the metric shape: 4096-row batches,
two spectra of 1024 channels, two components, in the table mode and the fast mode.  The species is a rigid linear rotor made
here from closed forms (1-0 with a three-line structure, 3-2 as one line: the narrow kernel forms), the grid the two-level
formula tex = tkin / (1 + (tkin / T0) ln(1 + ncrit / n)) on 12 x 10 x 9 nodes with the LTE optical depth at that tex.  The
hyperfine set runs model 3's unrolled kernels; the grid set runs the general-form baseline side (lnl_kernel_side, texs) and
one more launch between the stages, grid_derive_kernel.  The expectation to test is the cost of that side against the
unrolled kernels, which DESIGN 4.15 measured at about 1.3 for the templates side, plus the derive kernel's own time.
Device-pointer batches (nfa_runner_loglike_batch_dev) like bench.py; the two sets alternate in one process, R times
each, and the median of each is reported.  Then, unless --no-trace, one run of each set under `rocprofv3 --kernel-trace
--stats` (a fresh child process each) gives the mean time per launch of the set-up kernel and, for the grid set, of the
derive kernel.  One JSON line per (mode, set)."""
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
from nestfit_amd.excitation import FWHM       # noqa: E402
from nestfit_amd.lte import CCMS, CKMS, H_CGS, KB_CGS   # noqa: E402

ROWS, N_CHAN, NCOMP, N_PIX = 4096, 1024, 2, 16
B_ROT, MU = 46.5e9, 3.4e-18
RANGES = {'grid': [(-6.0, 6.0), (10.0, 55.0), (4.8, 6.8), (12.2, 14.2), (0.1, 1.5)],      # voff, tkin, lnden, lncol, sigm
          'hyperfine': [(-6.0, 6.0), (2.8, 20.0), (-1.5, 1.0), (0.1, 1.5)]}                # voff, tex, ltau, sigm
NPAR = {'grid': 5, 'hyperfine': 4}
TRUTH = np.array([-1.0, 2.0, 25.0, 18.0, 6.0, 5.6, 13.3, 13.0, 0.4, 0.7])
AXES = (np.linspace(8.0, 60.0, 12), np.linspace(4.5, 7.0, 10), np.linspace(11.0, 15.0, 9))
NCRIT = (1e4, 1e6)                             # of 1-0 and 3-2


def rotor_tables():
    temps = np.geomspace(2.5, 80.0, 32)
    q = [sum((2 * J + 1) * math.exp(-H_CGS * B_ROT * J * (J + 1) / (KB_CGS * T)) for J in range(400)) for T in temps]
    mol = na.Molecule('rotor', temps, q)

    def trans(J, **kw):
        nu = 2.0 * B_ROT * (J + 1)
        a_ul = 64.0 * math.pi ** 4 * nu ** 3 * MU ** 2 * (J + 1) / (3.0 * H_CGS * CCMS ** 3 * (2 * J + 3))
        return mol.transition(nu, H_CGS * B_ROT * (J + 1) * (J + 2) / KB_CGS, 2 * J + 3, a_ul, **kw)
    return [trans(0, voff=[-7.1, 0.0, 4.9], tau_wts=[0.2, 0.5, 0.3]), trans(2)]


def grid_tables(tables):
    """The `GridLines` of the LTE transitions `tables` on AXES: the two-level tex, the LTE depth at that tex for an FWHM of 1 km/s."""
    grid = na.ExcitationGrid(*AXES, name='two-level rotor')
    tk, nd, cd = np.meshgrid(*AXES, indexing='ij')
    out = []
    for t, ncrit in zip(tables, NCRIT):
        t0 = H_CGS * t.nu / KB_CGS
        tex = tk / (1.0 + (tk / t0) * np.log1p(ncrit / 10.0 ** nd))
        out.append(grid.transition(t.nu, tex, np.log10(t.tau_main(tex, cd, 1.0 / FWHM)), voff=t.voff, tau_wts=t.tau_wts, name=t.name))
    return out


def uniform_priors(ranges, size=500):
    u = np.linspace(0, 1, size)
    return na.PriorTransformer([na.Prior(na.Distribution(lo + u * (hi - lo), np.full(size, 1.0 / (hi - lo))), k)
                                for k, (lo, hi) in enumerate(ranges)])


def make_sets(only=None):
    rng = np.random.default_rng(17)
    tables = rotor_tables()
    axes = [t.nu * (1.0 - np.linspace(20.0, -20.0, N_CHAN) / CKMS) for t in tables]
    noise = rng.uniform(0.15, 0.3, (N_PIX, 2))
    on_grid = grid_tables(tables)
    zero = CubeRunner(axes, None, np.zeros((N_PIX, 2 * N_CHAN)), noise, None, ncomp=NCOMP, model=5, lines=on_grid)
    theta = np.repeat(TRUTH[None, :], N_PIX, axis=0)
    theta[:, :NCOMP] += 0.2 * np.arange(N_PIX)[:, None]
    spec, _ = zero.predict_batch(np.arange(N_PIX, dtype=np.int32), theta)
    data = spec + rng.normal(0, 1, spec.shape) * np.repeat(noise, N_CHAN, axis=1)
    plain = [na.LineTable(t.nu, t.voff, t.tau_wts) for t in tables]
    make = {'hyperfine': lambda: CubeRunner(axes, None, data, noise, uniform_priors(RANGES['hyperfine']), ncomp=NCOMP, model=3, lines=plain),
            'grid': lambda: CubeRunner(axes, None, data, noise, uniform_priors(RANGES['grid']), ncomp=NCOMP, model=5, lines=on_grid)}
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


def setup_kernel_time(name, mode, steps, warmup):
    """Mean time per launch of the set-up kernel (and of grid_derive_kernel, where it ran) of set `name`, from a child of this
    script under rocprofv3; None (and a message on stderr) where the profiler is missing or its output is not understood."""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', tmp, '--', sys.executable, __file__,
               '--trace-set', name, '--mode', mode, '--steps', str(steps), '--warmup', str(warmup), '--reps', '1', '--no-trace']
        try:
            subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=240)
        except OSError as e:                                 # no profiler on this machine: the rates stand without the trace
            print(f'measure_grid: no kernel trace of {name} / {mode}: {e}', file=sys.stderr)
            return None
        except subprocess.SubprocessError as e:              # the child hung or died on the device: nothing more is started there
            sys.exit(f'measure_grid: the traced run of {name} / {mode} failed, stopping: {e}')
        found = []
        for path in Path(tmp).rglob('*kernel_stats.csv'):
            with open(path) as f:
                for row in csv.DictReader(f):
                    if 'setup_kernel' in row.get('Name', '') or 'grid_derive_kernel' in row.get('Name', ''):
                        found.append({'kernel': row['Name'].split('(')[0], 'calls': int(row['Calls']), 'mean_us': float(row['AverageNs']) / 1e3})
        if found:
            return found
    print(f'measure_grid: no set-up kernel in the trace of {name} / {mode}', file=sys.stderr)
    return None


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
        sys.exit('measure_grid: no GPU')
    lib = _ffi.load()
    n = args.steps + args.warmup
    rng = np.random.default_rng(3)
    U_of = {name: np.ascontiguousarray(rng.uniform(size=(n, ROWS, k * NCOMP))) for name, k in NPAR.items()}
    pix = np.ascontiguousarray(rng.integers(0, N_PIX, (n, ROWS)).astype(np.int32))
    d_pix, d_u, d_l = C.c_void_p(), C.c_void_p(), C.c_void_p()
    _ffi.check(lib.nfa_malloc(C.byref(d_pix), pix.nbytes))
    _ffi.check(lib.nfa_malloc(C.byref(d_u), U_of['grid'].nbytes))
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
                    secs[name].append(time_steps(lib, r, d_pix, d_u, d_l, U_of[name], args.steps, args.warmup))
                    out = np.empty(n * ROWS)
                    _ffi.check(lib.nfa_memcpy_d2h(out.ctypes.data_as(C.c_void_p), d_l, out.nbytes))
                    finite[name] = bool(np.isfinite(out).all())
            base = np.median(secs['hyperfine']) if 'hyperfine' in secs else None
            for name, s in secs.items():
                med = float(np.median(s))
                rec = {'mode': mode, 'set': name, 'lines': [3, 1], 'rows': ROWS, 'spectra': 2, 'channels': N_CHAN, 'ncomp': NCOMP,
                       'steps': args.steps, 'reps': args.reps, 'evals_per_s': ROWS * args.steps / med,
                       'evals_per_s_spread': [ROWS * args.steps / max(s), ROWS * args.steps / min(s)],
                       'time_vs_hyperfine': med / base if base else None, 'lnl_all_finite': finite[name]}
                if not args.no_trace:
                    rec['setup_kernels'] = setup_kernel_time(name, mode, args.steps, args.warmup)
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
