"""What the normal equations cost on the device: `CubeRunner.normal_equations` against the route to the same
numbers without it, `lsq.PredictBackend`: `predict_batch` of the probe rows to the host plus the numpy twin.

Shape: 4096 points on two spectra of 1024 channels, two ammonia components (ndim 12, 25 rows per point, 163 points per chunk
of 4096 rows), both numerical modes.  A host clock around the calls, which are synchronous; after warm-up, the median of
REPEATS repeats (of HOST_REPEATS for the host route, which takes seconds).  The Gram kernel alone is not visible from outside
the call; its time comes from a kernel trace of this script in a run of its own (`--trace`: three calls per mode and nothing
else).  `--fit-cube`: `lsq.fit_cube` of the 32 x 32 cube of config 5 (synth.c5_stack) with two components, timed whole, and the
share of pixels that end 'converged'.  The script fails if the new call is not faster than the host route.

    python scripts/measure_lsq.py [--out profiles/lsq.txt] [--points 4096] [--trace | --fit-cube]
"""
import argparse
import ctypes as C
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

REPEATS, HOST_REPEATS = 20, 3
HOST_BLOCK = 160                    # points per predict_batch of the host route: 4000 rows, 65 MB of spectra


def fit_cube(args, lines):
    import nestfit_amd as na
    from nestfit_amd import lsq
    from nestfit_amd.synth import c5_stack
    stack, truths, _, _, _, ut = c5_stack(side=args.side, n=args.chan)
    for mode in ('table', 'fast'):
        na.set_exp_mode(mode)
        lsq.fit_cube(stack, ut, na.AmmoniaRunner, ncomp=2, n_draws=64, n_starts=1, max_iter=2)      # warm-up: the kernels load
        t0 = time.perf_counter()
        fit = lsq.fit_cube(stack, ut, na.AmmoniaRunner, ncomp=2)
        dt = time.perf_counter() - t0
        n_pix = fit.status.size
        share = {s: float(np.mean(fit.status == s)) for s in ('converged', 'max_iter', 'stalled', 'invalid')}
        truth = truths.T.reshape(12, args.side, args.side).transpose(0, 2, 1)
        swap = np.arange(12).reshape(6, 2)[:, ::-1].ravel()             # the two components in the other order
        with np.errstate(divide='ignore', invalid='ignore'):
            near = [np.all((np.abs(fit.params - t) / fit.errors)[:10] <= 5, axis=0) for t in (truth, truth[swap])]
        ok = (fit.status == 'converged') & (near[0] | near[1])
        lines += [f'fit_cube, mode {mode}: {args.side} x {args.side} pixels, 2 x {args.chan} channels, ncomp 2, 2048 draws and 4 starts per pixel',
                  f'  whole call                     {dt:10.2f} s   ({dt / n_pix * 1e3:.2f} ms per pixel)',
                  '  status                         ' + ', '.join(f'{k} {v:.3f}' for k, v in share.items()),
                  f'  converged with every parameter within 5 error bars of the truth (the components in either order): {float(np.mean(ok)):.3f}',
                  f'  median chi2 {float(np.median(fit.chi2)):.1f} on {2 * args.chan} channels', '']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'lsq.txt'))
    ap.add_argument('--points', type=int, default=4096)
    ap.add_argument('--chan', type=int, default=1024)
    ap.add_argument('--side', type=int, default=32)
    ap.add_argument('--repeats', type=int, default=REPEATS)
    ap.add_argument('--trace', action='store_true', help='three normal_equations calls per mode and nothing else (for a kernel trace)')
    ap.add_argument('--fit-cube', action='store_true', help='time lsq.fit_cube on the cube of config 5')
    args = ap.parse_args()

    import nestfit_amd as na
    from nestfit_amd import _ffi, lsq
    from nestfit_amd.cube import CubeRunner
    from nestfit_amd.synth import TRUTH_2COMP, freq_axis
    lib = _ffi.engine()
    assert na.device_count() > 0, 'no GPU visible'
    name = C.create_string_buffer(256)
    _ffi.check(lib.nfa_device_name(name, 256))
    lines = [f'least-squares normal equations, {name.value.decode()}', '']
    if args.fit_cube:
        fit_cube(args, lines)
        text = '\n'.join(lines)
        print(text)
        Path(args.out).write_text(text + '\n')
        return 0

    rng = np.random.default_rng(3)
    B, n_chan = args.points, args.chan
    chan_tot = 2 * n_chan
    axes = [freq_axis(1, n_chan, 30.0), freq_axis(2, n_chan, 30.0)]
    n_pix = 64
    probe = CubeRunner(axes, (1, 2), np.zeros((1, chan_tot)), np.full((1, 2), 0.2), None, ncomp=2)
    model, _ = probe.predict_batch(np.zeros(n_pix, np.int32), np.repeat(TRUTH_2COMP[None], n_pix, axis=0))
    runner = CubeRunner(axes, (1, 2), model + rng.normal(0, 0.2, model.shape), np.full((n_pix, 2), 0.2), None, ncomp=2)
    theta = np.ascontiguousarray(TRUTH_2COMP * (1.0 + 0.02 * rng.normal(size=(B, 12))))
    pix = (np.arange(B) % n_pix).astype(np.int32)
    lower, upper = TRUTH_2COMP - np.maximum(np.abs(TRUTH_2COMP), 1.0), TRUTH_2COMP + np.maximum(np.abs(TRUTH_2COMP), 1.0)
    step = 1e-3 * (upper - lower)
    host = lsq.PredictBackend(runner)

    def host_route():
        parts = [host.normal_equations(pix[a:a + HOST_BLOCK], theta[a:a + HOST_BLOCK], step, lower, upper) for a in range(0, B, HOST_BLOCK)]
        return lsq.NormalEquations(*(np.concatenate(x) for x in zip(*parts)))

    lines[1:1] = [f'{B} points, 2 x {n_chan} channels, ncomp 2 (ndim 12: 25 rows per point, 163 points per chunk of 4096 rows); '
                  f'median of {args.repeats} repeats after warm-up ({HOST_REPEATS} of the host route)']
    ok = True
    med = statistics.median
    for mode in ('table', 'fast'):
        runner.set_exp_mode(mode)
        if args.trace:
            for _ in range(3):
                runner.normal_equations(pix, theta, step, lower, upper)
            continue
        for _ in range(2):
            ne = runner.normal_equations(pix, theta, step, lower, upper)
            runner.chi_squared(pix, theta)
        whole, only = [], []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            ne = runner.normal_equations(pix, theta, step, lower, upper)
            whole.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            chi2 = runner.chi_squared(pix, theta)
            only.append((time.perf_counter() - t0) * 1e3)
        assert np.array_equal(chi2, ne.chi2)
        ref = host_route()
        scale = np.sqrt(np.einsum('bkk,bll->bkl', ref.curv, ref.curv))
        assert np.all(np.abs(ne.curv - ref.curv) <= 1e-10 * scale + 1e-300) and np.allclose(ne.chi2, ref.chi2, rtol=1e-10), 'the two routes disagree'
        today = []
        for _ in range(HOST_REPEATS):
            t0 = time.perf_counter()
            host_route()
            today.append((time.perf_counter() - t0) * 1e3)
        n_chunks = -(-B // (4096 // 25))
        lines += [f'mode {mode}',
                  f'  whole normal_equations call    {med(whole):10.2f} ms host clock (min {min(whole):.2f}, max {max(whole):.2f}); '
                  f'{n_chunks} chunks: {med(whole) / n_chunks * 1e3:.1f} us per chunk',
                  f'  chi_squared (one row a point)  {med(only):10.2f} ms host clock (min {min(only):.2f}, max {max(only):.2f})',
                  f'  host: predict_batch + numpy    {med(today):10.2f} ms host clock (min {min(today):.2f}, max {max(today):.2f})',
                  f'  new call / host route          {med(whole) / med(today):10.5f}',
                  f'  spectra that stay on the device {B * 25 * chan_tot * 8 / 1e9:9.2f} GB per call; {B * 12 * 8 / 1e3:.0f} kB of theta go in, '
                  f'{B * (1 + 12 + 144) * 8 / 1e6:.1f} MB come out', '']
        ok = ok and med(whole) < med(today)
    if args.trace:
        print('trace run done')
        return 0
    text = '\n'.join(lines)
    print(text)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text + '\n')
    if not ok:
        print('FAIL: normal_equations is not faster than predict_batch + numpy')
        return 1
    return 0


if __name__ == '__main__':
    sys.exit(main())
