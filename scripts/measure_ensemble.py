"""What the ensemble sampler costs on the device.

1. Wall time per step: P = 1024 pixels, W = 64 walkers, two spectra of 1024 channels, two ammonia components (ten sampled
   dimensions), both numerical modes; a host clock around `nfa_ensemble_run` (synchronous), the median of REPEATS runs of
   200 steps after warm-up.  The split by kernel comes from a kernel trace of this script in a run of its own (`--trace`:
   one run of 50 steps per mode and nothing else).
2. The summary on the device against the host route: `nfa_ensemble_summary` against fetching the chain and `ensemble.summarize`
   (the same reductions in numpy), same shape, 8192 kept samples per pixel.
3. `--cube`: evaluations per pixel on the 32 x 32 cube of config 5 (synth.c5_stack), two components, until n_eff >= 1000 in
   every sampled dimension: runs of doubling length, the share of pixels that got there and of pixels whose tau is not yet
   trustworthy (n_steps - n_burn < 50 tau), reported, not dropped.
4. `--products`: the products of a chain by the device route against the host route of the same tree, P = 256,
   W = 64, n_keep = 128, two spectra of 1024 channels, two components, both modes, the median of REPEATS: `moments` against
   fetching the chain and `predict_moments`; `histogram` (64 bins over the priors' box) and `covariance` against fetching
   the chain and the numpy twins.  Default --out: profiles/ensemble_products.txt.
5. `--tempered`: tempered ensembles, P = 64, W = 64, T = 16 (`ladder(16)`), two spectra of 1024 channels, two
   components, both modes: the wall time per step against the untempered step of P T = 1024 pixels of the same runner -- the
   same number of rows a half-step -- as in 1; `nfa_ensemble_evidence` against fetching the rung lnL and `ensemble.evidence_of`,
   as in 4.  With `--trace` one tempered run of 50 steps per mode and nothing else (for the swap kernel's share in a kernel
   trace); with `--cube` the config-5 cube, two components: lnZ_err per pixel after runs of `--steps` steps, next to the
   evaluations per pixel they took, all rungs counted.  Default --out: profiles/ensemble_tempered.txt.

    python scripts/measure_ensemble.py [--out profiles/ensemble.txt] [--pixels 1024] [--trace | --cube | --products | --tempered]
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

REPEATS = 20


def cube(args, lines):
    import nestfit_amd as na
    from nestfit_amd import ensemble
    from nestfit_amd.synth import c5_stack
    stack, _, _, _, _, ut = c5_stack(side=args.side, n=args.chan)
    na.set_exp_mode('table')
    mask = ut.free_mask(2)
    for n_steps in args.steps:
        t0 = time.perf_counter()
        maps = ensemble.sample_cube(stack, ut, na.AmmoniaRunner, 2, n_walkers=64, n_steps=n_steps, free_mask=mask, levels=())
        dt = time.perf_counter() - t0
        n_eff = np.nanmin(np.where(np.isfinite(maps.n_eff), maps.n_eff, 0.0), axis=0).ravel()
        tau = np.nanmax(np.where(np.isfinite(maps.tau), maps.tau, np.inf), axis=0).ravel()
        young = (n_steps - n_steps // 2) < 50 * tau
        evals = maps.n_evals.ravel() + 2048                     # the start draws included
        lines += [f'sample_cube, table mode: {args.side} x {args.side} pixels, 2 x {args.chan} channels, ncomp 2, W = 64, {n_steps} steps, half burned',
                  f'  whole call {dt:8.2f} s; evaluations per pixel {int(np.median(evals))} (nested run, DESIGN 6: 1.10 M)',
                  f'  pixels with n_eff >= 1000 in every sampled dimension: {float(np.mean(n_eff >= 1000)):.3f}; median of the smallest n_eff {float(np.median(n_eff)):.0f}',
                  f'  pixels whose tau is not yet trustworthy (n_steps - n_burn < 50 tau): {float(np.mean(young)):.3f}; median of the largest tau {float(np.median(tau)):.1f} steps',
                  f'  acceptance {float(np.nanmedian(maps.acceptance)):.3f}, outside {float(np.nanmedian(maps.outside)):.3f}', '']


def products(args, lines):
    import nestfit_amd as na
    from nestfit_amd import ensemble
    from nestfit_amd.cube import CubeRunner
    from nestfit_amd.synth import TRUTH_2COMP, freq_axis
    P, W, n, n_keep, n_bins = 256, 64, args.chan, 128, 64
    rng = np.random.default_rng(1)
    axes = [freq_axis(1, n), freq_axis(2, n)]
    ut = na.get_irdc_priors(size=500, vsys=0.0)
    na.set_exp_mode('table')
    probe = CubeRunner(axes, (1, 2), np.zeros((1, 2 * n)), np.full((1, 2), 0.2), ut, ncomp=2)
    model, _ = probe.predict_batch(np.zeros(P, np.int32), np.repeat(TRUTH_2COMP[None], P, axis=0))
    runner = CubeRunner(axes, (1, 2), model + rng.normal(0, 0.2, model.shape), np.full((P, 2), 0.2), ut, ncomp=2)
    pix = np.arange(P, dtype=np.int32)
    edges = ensemble.bin_edges(ut, 2, n_bins)
    offsets = np.arange(P + 1, dtype=np.int64) * (n_keep * W)
    u0 = ensemble.starts(runner, pix, W, n_init=256, seed=1)

    def median_ms(call):
        call()
        times = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            out = call()
            times.append(time.perf_counter() - t0)
        return statistics.median(times) * 1e3, out

    for mode in ('table', 'fast'):
        runner.set_exp_mode(mode)
        ens = ensemble.DeviceEnsemble(runner, pix, W, u0, ut.free_mask(2))
        ens.run(2 * n_keep, n_keep, 1, 2.0, 1)

        def host_moments():
            theta, _ = ens.chain()
            return runner.predict_moments(pix, offsets, theta.reshape(-1, ens.ndim))

        def host_histogram():
            return ensemble.pdf_counts(ens.chain()[0], edges)

        def host_covariance():
            return ensemble.covariance_of(*ens.chain())
        lines.append(f'mode {mode}: P = {P}, W = {W}, n_keep = {n_keep} ({n_keep * W} samples per pixel), 2 x {n} channels, ncomp 2, '
                     f'chain {P * n_keep * W * (ens.ndim + 1) * 8 / 1e6:.0f} MB; median of {args.repeats}')
        for what, dev_call, host_call in (('moments', ens.moments, host_moments), (f'histogram, {n_bins} bins', lambda: ens.histogram(edges), host_histogram),
                                          ('covariance', ens.covariance, host_covariance)):
            t_dev, dev = median_ms(dev_call)
            t_host, host = median_ms(host_call)
            if what != 'covariance':
                assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(dev, host)), what
            lines.append(f'  {what:22s} device {t_dev:10.2f} ms   chain to the host + host route {t_host:10.2f} ms')
        lines.append('')
        ens.close()


def tempered_cube(args, lines):
    import nestfit_amd as na
    from nestfit_amd import ensemble
    from nestfit_amd.synth import c5_stack
    stack, _, _, _, _, ut = c5_stack(side=args.side, n=args.chan)
    na.set_exp_mode('table')
    betas, W = ensemble.ladder(16), 64
    for n_steps in args.steps:
        t0 = time.perf_counter()
        maps = ensemble.sample_cube(stack, ut, na.AmmoniaRunner, 2, n_walkers=W, n_steps=n_steps, free_mask=ut.free_mask(2), levels=(),
                                    betas=betas)
        dt = time.perf_counter() - t0
        err = maps.lnZ_err[np.isfinite(maps.lnZ_err)]
        evals = betas.size * (n_steps * W + W) + 2048          # every rung's steps and start rows, and the start draws
        lines += [f'sample_cube, table mode, ladder(16): {args.side} x {args.side} pixels, 2 x {args.chan} channels, ncomp 2, W = {W}, {n_steps} steps, half burned',
                  f'  whole call {dt:8.2f} s; evaluations per pixel {evals} (nested run, DESIGN 6: 1.10 M, lnZ_err 0.25)',
                  f'  lnZ_err (8 blocks): median {float(np.median(err)):.3f}, largest {float(err.max()):.3f}; pixels below 0.25: {float(np.mean(err < 0.25)):.3f}',
                  f'  smallest swap rate {float(np.nanmin(maps.swap_rate)):.3f}, median {float(np.nanmedian(maps.swap_rate)):.3f}; cold acceptance {float(np.nanmedian(maps.acceptance)):.3f}', '']


def tempered(args, lines):
    import nestfit_amd as na
    from nestfit_amd import ensemble
    from nestfit_amd.cube import CubeRunner
    from nestfit_amd.synth import TRUTH_2COMP, freq_axis
    P, W, T, n = 64, 64, 16, args.chan
    betas = ensemble.ladder(T)
    rng = np.random.default_rng(1)
    axes = [freq_axis(1, n), freq_axis(2, n)]
    ut = na.get_irdc_priors(size=500, vsys=0.0)
    na.set_exp_mode('table')
    probe = CubeRunner(axes, (1, 2), np.zeros((1, 2 * n)), np.full((1, 2), 0.2), ut, ncomp=2)
    model, _ = probe.predict_batch(np.zeros(P * T, np.int32), np.repeat(TRUTH_2COMP[None], P * T, axis=0))
    runner = CubeRunner(axes, (1, 2), model + rng.normal(0, 0.2, model.shape), np.full((P * T, 2), 0.2), ut, ncomp=2)
    pix = np.arange(P * T, dtype=np.int32)
    mask = ut.free_mask(2)
    u0 = ensemble.starts(runner, pix, W, n_init=256, seed=1)

    def per_step(ens):
        ens.run(20, 0, 1, 2.0, 1)                                  # warm-up
        times = []
        for k in range(args.repeats):
            t0 = time.perf_counter()
            ens.run(200, 100, 1, 2.0, 2 + k)
            times.append(time.perf_counter() - t0)
        return statistics.median(times) / 200, min(times) / 200, max(times) / 200

    for mode in ('table', 'fast'):
        runner.set_exp_mode(mode)
        hot = ensemble.DeviceEnsemble(runner, pix[:P], W, u0[:P], mask, betas=betas, swap_every=1)
        if args.trace:
            hot.run(50, 0, 1, 2.0, 1)
            hot.close()
            continue
        t_hot = per_step(hot)
        cold = ensemble.DeviceEnsemble(runner, pix, W, u0, mask)
        t_cold = per_step(cold)
        cold.close()
        lines += [f'mode {mode}: P = {P}, W = {W}, T = {T}, 2 x {n} channels, ncomp 2 (D = {hot.D} of {hot.ndim}); {P * T * W // 2} rows per half-step; '
                  f'runs of 200 steps, median of {args.repeats}',
                  f'  tempered, a swap sweep every step      {t_hot[0] * 1e6:10.1f} us per step  ({t_hot[1] * 1e6:.1f} .. {t_hot[2] * 1e6:.1f})',
                  f'  untempered, {P * T} pixels              {t_cold[0] * 1e6:10.1f} us per step  ({t_cold[1] * 1e6:.1f} .. {t_cold[2] * 1e6:.1f})']
        hot.run(256, 128, 1, 2.0, 99)                              # 128 kept steps x 64 walkers = 8192 values per (pixel, rung)
        hot.evidence(8)
        t_dev, t_host = [], []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            dev = hot.evidence(8)
            t_dev.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            host = ensemble.evidence_of(hot.rung_lnL(), betas, 8)
            t_host.append(time.perf_counter() - t0)
        assert np.allclose(dev.lnZ, host.lnZ, rtol=0, atol=1e-9)
        lines += [f'  evidence of {P} x {T} x 8192 kept lnL, 8 blocks:',
                  f'    nfa_ensemble_evidence               {statistics.median(t_dev) * 1e3:10.2f} ms',
                  f'    rung lnL to the host + evidence_of  {statistics.median(t_host) * 1e3:10.2f} ms  (the rung lnL is {P * T * 8192 * 8 / 1e6:.0f} MB)',
                  f'  lnZ_err of the {P} pixels: median {float(np.median(dev.lnZ_err)):.3f}; smallest swap rate '
                  f'{float((hot.rung_counts()[3] / hot.rung_counts()[4]).min()):.3f}', '']
        hot.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    ap.add_argument('--pixels', type=int, default=1024)
    ap.add_argument('--chan', type=int, default=1024)
    ap.add_argument('--side', type=int, default=32)
    ap.add_argument('--steps', type=int, nargs='+', default=[1000, 4000])
    ap.add_argument('--repeats', type=int, default=REPEATS)
    ap.add_argument('--trace', action='store_true', help='one run of 50 steps per mode and nothing else (for a kernel trace)')
    ap.add_argument('--cube', action='store_true', help='evaluations per pixel on the cube of config 5')
    ap.add_argument('--products', action='store_true', help='histogram, covariance and moments: device route against host route')
    ap.add_argument('--tempered', action='store_true', help='tempered ensembles: step time, evidence call; with --cube the evidences of config 5')
    args = ap.parse_args()
    args.out = args.out or str(ROOT / 'profiles' / ('ensemble_tempered.txt' if args.tempered else 'ensemble_products.txt' if args.products
                                                    else 'ensemble.txt'))

    import nestfit_amd as na
    from nestfit_amd import _ffi, ensemble
    from nestfit_amd.cube import CubeRunner
    from nestfit_amd.synth import TRUTH_2COMP, freq_axis
    lib = _ffi.engine()
    assert na.device_count() > 0, 'no GPU visible'
    name = C.create_string_buffer(256)
    _ffi.check(lib.nfa_device_name(name, 256))
    lines = [f'ensemble sampler, {name.value.decode()}', '']
    if args.cube or args.products or args.tempered:
        if args.tempered:
            tempered(args, lines)
            if args.trace:
                return 0
            if args.cube:
                tempered_cube(args, lines)
        else:
            (cube if args.cube else products)(args, lines)
        text = '\n'.join(lines)
        print(text)
        Path(args.out).write_text(text + '\n')
        return 0

    P, W, n = args.pixels, 64, args.chan
    rng = np.random.default_rng(1)
    axes = [freq_axis(1, n), freq_axis(2, n)]
    ut = na.get_irdc_priors(size=500, vsys=0.0)
    na.set_exp_mode('table')
    probe = CubeRunner(axes, (1, 2), np.zeros((1, 2 * n)), np.full((1, 2), 0.2), ut, ncomp=2)
    model, _ = probe.predict_batch(np.zeros(P, np.int32), np.repeat(TRUTH_2COMP[None], P, axis=0))
    runner = CubeRunner(axes, (1, 2), model + rng.normal(0, 0.2, model.shape), np.full((P, 2), 0.2), ut, ncomp=2)
    pix = np.arange(P, dtype=np.int32)
    mask = ut.free_mask(2)
    u0 = ensemble.starts(runner, pix, W, n_init=256, seed=1)
    for mode in ('table', 'fast'):
        runner.set_exp_mode(mode)
        ens = ensemble.DeviceEnsemble(runner, pix, W, u0, mask)
        if args.trace:
            ens.run(50, 0, 1, 2.0, 1)
            ens.close()
            continue
        ens.run(20, 0, 1, 2.0, 1)                                  # warm-up: the kernels load, the lanes' workspaces come
        times = []
        for k in range(args.repeats):
            t0 = time.perf_counter()
            ens.run(200, 100, 1, 2.0, 2 + k)
            times.append(time.perf_counter() - t0)
        per_step = statistics.median(times) / 200
        lines += [f'mode {mode}: P = {P}, W = {W}, 2 x {n} channels, ncomp 2 (D = {ens.D} of {ens.ndim}); {P * W // 2} rows per half-step',
                  f'  run of 200 steps, median of {args.repeats}   {statistics.median(times) * 1e3:10.2f} ms  ({min(times) * 1e3:.2f} .. {max(times) * 1e3:.2f})',
                  f'  per step                          {per_step * 1e6:10.1f} us  = {P * W / per_step / 1e6:.1f} M evaluations/s']
        # the summary: 128 kept steps x 64 walkers = 8192 samples per pixel
        ens.run(256, 128, 1, 2.0, 99)
        levels = (0.16, 0.5, 0.84)
        ens.summary(levels)
        t_dev, t_host = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            dev = ens.summary(levels)
            t_dev.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            theta, lnL = ens.chain()
            host = ensemble.summarize(theta, lnL, levels)
            t_host.append(time.perf_counter() - t0)
        assert np.array_equal(dev[2], host[2]) and np.array_equal(dev[4], host[4])
        lines += [f'  summary of {P} x 8192 samples x {ens.ndim} parameters, three quantiles:',
                  f'    nfa_ensemble_summary            {statistics.median(t_dev) * 1e3:10.2f} ms',
                  f'    chain to the host + numpy       {statistics.median(t_host) * 1e3:10.2f} ms  (the chain is {theta.nbytes / 1e6:.0f} MB)', '']
        ens.close()
    if args.trace:
        return 0
    text = '\n'.join(lines)
    print(text)
    Path(args.out).write_text(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
