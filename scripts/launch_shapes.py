"""usage: python scripts/launch_shapes.py            one launch of every kind through the public API (one MI355X)
       python scripts/launch_shapes.py --reduce kernel_trace.csv [...]   the trace of such a run as a list of launches
       python scripts/launch_shapes.py --shapes kernel_trace.csv [...]   that list's checksum and its distinct launches

The first form sends one launch through every branch of the host's launch planning (nfa_launch_plan.h: plan_lnl,
plan_setup, plan_fused) and prints a checksum of every result array.  It is deterministic -- fixed seeds, one
process, no timing, a synchronisation after every launch -- so that two builds of the engine can be compared: run it
under `rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/launch_shapes.py` with each, reduce the
two traces with the second form to (kernel, grid, workgroup, LDS) in dispatch order, and diff the two lists and the two
outputs (profiles/launch_plan/README.md, profiles/set_kinds/README.md, profiles/side_family/README.md).  The resident ring kernel needs a client process: tests/test_ring.py."""
import csv
import ctypes as C
import hashlib
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np

MODES = ('table', 'fast')


def reduce_traces(paths, shapes_only):
    rows = []
    for path in paths:
        with open(path) as f:
            for r in csv.DictReader(f):
                dims = lambda key: 'x'.join(r[f'{key}_{a}'] for a in 'XYZ') if f'{key}_X' in r else r[key]
                name = r['Kernel_Name'].split('(')[0].replace('void ', '')          # the argument list says nothing here
                rows.append((int(r['Dispatch_Id']), name, dims('Grid_Size'), dims('Workgroup_Size'), r['LDS_Block_Size']))
    lines = [f'{name}\tgrid {grid}\tworkgroup {wg}\tlds {lds}' for _, name, grid, wg, lds in sorted(rows)]
    if not shapes_only:
        print('\n'.join(lines))
        return
    # the list is thousands of lines: its checksum, and per kernel every distinct launch once with the times it came by
    print(f'{len(lines)} dispatches in order: sha1 {hashlib.sha1(chr(10).join(lines).encode()).hexdigest()}')
    count = {}
    for _, name, grid, wg, lds in sorted(rows):
        shape = f'grid {grid.replace("x1x1", "")} workgroup {wg.replace("x1x1", "")} lds {lds}'
        count.setdefault(name, {}).setdefault(shape, 0)
        count[name][shape] += 1
    for name, shapes in count.items():
        print(f'{name}: ' + '; '.join(f'{n} x {shape}' for shape, n in shapes.items()))


if len(sys.argv) > 1 and sys.argv[1] in ('--reduce', '--shapes'):
    reduce_traces(sys.argv[2:], sys.argv[1] == '--shapes')
    sys.exit(0)

import nestfit_amd as na
from nestfit_amd import _ffi
from nestfit_amd.cube import CubeRunner
from nestfit_amd.synth import CKMS, TRUTH_2COMP, freq_axis

lib = _ffi.load()
N2HP_NU = {1: 93173.7637e6, 2: 186344.8420e6, 3: 279511.8325e6}
N_PIX = 4


def emit(tag, *arrays):
    h = hashlib.sha1()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    print(f'{tag}: {h.hexdigest()[:16]}', flush=True)


def ammonia_spectra(n_chan, seed, noise=0.2):
    """[x, data, noise, trans] of NH3 (1,1) and (2,2): the two-component truth plus noise."""
    rng = np.random.default_rng(seed)
    out = []
    for t in (1, 2):
        x = freq_axis(t, n_chan)
        s = na.AmmoniaSpectrum(x, np.zeros(n_chan), noise, t)
        na.amm_predict(s, TRUTH_2COMP)
        out.append([x, s.get_spec() + rng.normal(0, noise, n_chan), noise, t])
    return out


def uniform_priors(ranges, size=200):
    x = np.linspace(0, 1, size)
    return na.PriorTransformer([na.Prior(na.Distribution(lo + x * (hi - lo), np.full(size, 1.0 / (hi - lo))), k)
                                for k, (lo, hi) in enumerate(ranges)])


def host_calls(tag, run, sizes, seed, spectra_rows=0):
    """loglikelihood_batch of `sizes` rows each; then predict_batch (spectra out) of theta rows one of them left."""
    rng = np.random.default_rng(seed)
    theta = None
    for B in sizes:
        U = rng.uniform(size=(B, run.ndim))
        lnl = run.loglikelihood_batch(U)
        emit(f'{tag} loglike B={B}', U, lnl)
        if theta is None and B >= spectra_rows:
            theta = U
    if spectra_rows:
        spec, lnl = run.predict_batch(theta[:spectra_rows])
        emit(f'{tag} predict B={spectra_rows}', spec, lnl)


class DeviceBuffer:
    def __init__(self, a):
        self.like, self.p = np.ascontiguousarray(a), C.c_void_p()
        _ffi.check(lib.nfa_malloc(C.byref(self.p), self.like.nbytes))
        _ffi.check(lib.nfa_memcpy_h2d(self.p, self.like.ctypes.data_as(C.c_void_p), self.like.nbytes))

    def get(self):
        out = np.empty_like(self.like)
        _ffi.check(lib.nfa_memcpy_d2h(out.ctypes.data_as(C.c_void_p), self.p, out.nbytes))
        _ffi.check(lib.nfa_free(self.p))
        return out


def device_group(tag, cube, n_batches, rows, seed, spectra=False):
    """n_batches device-pointer batches of `rows` rows enqueued back to back (the engine holds them and launches them
    as one group), then one synchronise; spectra: and then as many predict batches with spectra out."""
    rng = np.random.default_rng(seed)
    h = cube._run.handle
    bufs = [(DeviceBuffer(rng.integers(0, cube.n_pix, rows).astype(np.int32)), DeviceBuffer(rng.uniform(size=(rows, cube.ndim))),
             DeviceBuffer(np.full(rows, np.nan))) for _ in range(n_batches)]
    for pix, u, lnl in bufs:
        _ffi.check(lib.nfa_runner_loglike_batch_dev(h, pix.p, u.p, lnl.p, rows))
    _ffi.check(lib.nfa_runner_synchronize(h))
    specs = []
    if spectra:                                              # theta: what the loglike batches left in U
        for pix, u, lnl in bufs:
            specs.append(DeviceBuffer(np.full((rows, cube.n_chan_tot), np.nan)))
            _ffi.check(lib.nfa_runner_predict_batch_dev(h, pix.p, u.p, rows, specs[-1].p, lnl.p))
        _ffi.check(lib.nfa_runner_synchronize(h))
    emit(f'{tag} {"predict" if spectra else "loglike"}_dev {n_batches} x {rows}', *[b.get() for t in bufs for b in t], *[a.get() for a in specs])


def make_cube(n_chan, seed, ncomp=2, chan_noise=False, baseline_order=None):
    rng = np.random.default_rng(seed)
    spectra = ammonia_spectra(n_chan, seed)
    axes = [s[0] for s in spectra]
    data = np.stack([np.concatenate([s[1] for s in spectra]) + 0.05 * p + rng.normal(0, 0.1, 2 * n_chan) for p in range(N_PIX)])
    if chan_noise:
        noise = rng.uniform(0.15, 0.3, (N_PIX, 2 * n_chan))
        noise[:, ::97] = np.inf                               # masked channels
    else:
        noise = rng.uniform(0.15, 0.3, (N_PIX, 2))
    return CubeRunner(axes, [1, 2], data, noise, na.get_irdc_priors(size=500, vsys=0.0), ncomp=ncomp, baseline_order=baseline_order)


def cube_host(tag, cube, sizes, seed):
    rng = np.random.default_rng(seed)
    for B in sizes:
        pix, U = rng.integers(0, N_PIX, B), rng.uniform(size=(B, cube.ndim))
        lnl = cube.loglikelihood_batch(pix, U)
        emit(f'{tag} loglike B={B}', U, lnl)
        if B == 300:
            spec, lnl = cube.predict_batch(pix, U)
            emit(f'{tag} predict B={B}', spec, lnl)


def main():
    assert na.device_count() > 0, 'no GPU visible'
    for mode in MODES:
        na.set_exp_mode(mode)
        # component counts, log-likelihood and spectra out (8 components, 500-point irdc priors, table mode: the set-up
        # launch takes the prior program that reads its tables from global memory)
        for ncomp in (1, 2, 3, 4, 8):
            run = na.AmmoniaRunner.from_data(ammonia_spectra(1024, 3), na.get_irdc_priors(size=500), ncomp=ncomp)
            host_calls(f'{mode} ncomp={ncomp}', run, (300,), 10 + ncomp, spectra_rows=300)
        # launch sizes through the host call: automatic split 4, 2, 1; just above the point kernel's limit; chunks
        run = na.AmmoniaRunner.from_data(ammonia_spectra(1024, 3), na.get_irdc_priors(size=500), ncomp=2)
        host_calls(f'{mode} sizes', run, (300, 1500, 4096, 129, 65536), 20, spectra_rows=4096)
        host_calls(f'{mode} sizes spectra', run, (1500,), 21, spectra_rows=1500)
        # groups of device-pointer batches: 2 x 1024 channels (table mode: the queue form, two-group set-up), 2 x 256
        for n_chan in (1024, 256):
            cube = make_cube(n_chan, 30)
            for n in (1, 2, 8):
                device_group(f'{mode} {n_chan} channels', cube, n, 4096, 31 + n)
            for n in (1, 2):
                device_group(f'{mode} {n_chan} channels', cube, n, 4096, 41 + n, spectra=True)
        # the other models: N2H+ with the 2-1 transition (wide), one Gaussian spectrum
        rng = np.random.default_rng(50)
        ut = uniform_priors([(-6, 6), (2.8, 20), (-1.5, 1.0), (0.1, 1.5)])
        args = []
        for trans, n in ((1, 700), (2, 1024)):
            x = N2HP_NU[trans] * (1.0 - np.linspace(20, -20, n) / CKMS)
            s = na.DiazenyliumSpectrum(x, np.zeros(n), 0.15, trans)
            na.nnhp_predict(s, np.array([-1.0, 2.0, 8.0, 5.0, 0.3, -0.2, 0.4, 0.7]))
            args.append([x, s.get_spec() + rng.normal(0, 0.15, n), 0.15, trans])
        host_calls(f'{mode} n2hp', na.DiazenyliumRunner.from_data(args, ut, ncomp=2), (1, 16, 300, 4096), 51, spectra_rows=300)
        nu0 = 110.201354e9
        x = nu0 * (1.0 - np.linspace(30, -30, 1500) / CKMS)
        utg = uniform_priors([(-20, 20), (0.2, 3.0), (0.0, 5.0)])
        gauss = na.GaussianRunner.from_data([x, rng.normal(0, 0.3, 1500), 0.3, nu0], utg, ncomp=3)
        host_calls(f'{mode} gaussian', gauss, (1, 16, 300, 4096), 52, spectra_rows=300)
        # caller-supplied line tables: a hyperfine set of one line, one of 40 lines (the wide forms), an LTE set of two
        # transitions -- batches, spectra out and single points each
        axis = lambda nu, n, v: nu * (1.0 - np.linspace(v, -v, n) / CKMS)
        rows = lambda tables, n, v: [[axis(t.nu, n, v), rng.normal(0, 0.2, n), 0.2, t] for t in tables]
        one_line = na.LineTable(115.271202e9, [0.0], [1.0])
        forty = na.LineTable(N2HP_NU[2], np.linspace(-19.5, 19.5, 40), np.linspace(0.5, 1.5, 40) / 40)
        mol = na.Molecule('rotor', [5.0, 10.0, 20.0, 40.0, 80.0], [2.2, 4.1, 7.9, 15.5, 30.7])
        lte = [na.LteLines(mol, 110.201354e9, 5.29, 3, 6.3e-8), na.LteLines(mol, 220.398684e9, 15.87, 5, 6.0e-7, voff=[-0.8, 0.0, 0.9], tau_wts=[0.2, 0.5, 0.3])]
        utl = uniform_priors([(-6, 6), (2.8, 20), (12.0, 14.0), (0.1, 1.5)])
        host_calls(f'{mode} hyperfine 1 line', na.HyperfineRunner.from_data(rows([one_line], 700, 20), ut, ncomp=2), (1, 16, 300, 4096), 53, spectra_rows=300)
        host_calls(f'{mode} hyperfine 40 lines', na.HyperfineRunner.from_data(rows([forty], 1024, 45), ut, ncomp=2), (1, 16, 300, 4096), 54, spectra_rows=300)
        host_calls(f'{mode} lte 2 transitions', na.LteRunner.from_data(rows(lte, 800, 20), utl, ncomp=2), (1, 16, 300, 4096), 55, spectra_rows=300)
        # the set kinds of the general component form, on short spectra: a filled LTE mix; layered sets (ammonia, the filled
        # mix); calibrated sets (ammonia without and with a baseline, the filled layered mix)
        iso = na.Molecule('rotor-iso', [5.0, 10.0, 20.0, 40.0, 80.0], [2.3, 4.3, 8.3, 16.3, 32.3])
        mix_rows = rows([lte[0], na.LteLines(iso, 109.782176e9, 5.27, 3, 6.2e-8)], 300, 20)
        utm = uniform_priors([(-6, 6), (2.8, 20), (12.0, 14.0), (0.1, 1.5), (11.0, 13.0), (-1.0, 0.0)])
        filled = lambda **kw: na.LteMix((mol, iso), fill=True).Runner.from_data(mix_rows, utm, ncomp=2, **kw)
        ammonia = lambda **kw: na.AmmoniaRunner.from_data(ammonia_spectra(320, 3), na.get_irdc_priors(size=500), ncomp=2, **kw)
        for seed, (what, make, kw) in enumerate((('filled mix', filled, {}), ('ammonia layered', ammonia, dict(layered=True)),
                                                 ('filled mix layered', filled, dict(layered=True)),
                                                 ('ammonia calibrated', ammonia, dict(calibration=0.1)),
                                                 ('ammonia calibrated, baseline 3', ammonia, dict(calibration=0.1, baseline_order=3)),
                                                 ('filled mix layered calibrated', filled, dict(layered=True, calibration=0.1)))):
            host_calls(f'{mode} {what}', make(**kw), (1, 16, 300, 4096), 56 + seed, spectra_rows=300)
        # the side family (lnl_kernel_side), one small set per side: ammonia of 2 x 300 channels, the same layered, and the
        # filled mix -- a correlation, a response with its correlation, templates beside a baseline, a continuum, a robust likelihood
        short = lambda **kw: na.AmmoniaRunner.from_data(ammonia_spectra(300, 3), na.get_irdc_priors(size=500), ncomp=2, **kw)
        ripples = [na.ripple(300, 137.3)] * 2
        for seed, (side, kw) in enumerate((('correlation', dict(correlation=na.HANNING)), ('response', na.smoothed(na.HANNING_RESPONSE)),
                                           ('templates', dict(templates=ripples, baseline_order=1)), ('continuum', dict(continuum=30.0)),
                                           ('robust', dict(robust=4)))):
            for what, make, more in (('ammonia', short, {}), ('ammonia layered', short, dict(layered=True)), ('filled mix', filled, {})):
                host_calls(f'{mode} {side} {what}', make(**kw, **more), (1, 16, 300), 90 + seed, spectra_rows=300)
        # weighted sets and baselines: the split parts' LDS differs with a baseline
        for what, kw in (('channel noise', dict(chan_noise=True)), ('baseline 1', dict(baseline_order=1)),
                         ('channel noise, baseline 3', dict(chan_noise=True, baseline_order=3))):
            cube = make_cube(1024, 60, **kw)
            cube_host(f'{mode} {what}', cube, (1, 300, 1500), 61)
            device_group(f'{mode} {what}', cube, 2, 4096, 62)
            device_group(f'{mode} {what}', cube, 1, 4096, 63, spectra=True)
        # single points and a handful: the point kernel and (option point 0) the batch kernels; ndim 12 and, above
        # NFA_POINT_MAXDIM, 30
        for ncomp in (2, 5):
            run = na.AmmoniaRunner.from_data(ammonia_spectra(1024, 3), na.get_irdc_priors(size=500), ncomp=ncomp)
            for point in (1, 0):
                _ffi.set_option('point', point)
                host_calls(f'{mode} ndim={6 * ncomp} point={point}', run, (1, 1, 1, 1, 16, 128), 70 + ncomp)
            _ffi.set_option('point', 1)
    # every knob off its default, one at a time (the runner takes its launch geometry from the options at creation, the
    # priors their staging)
    knobs = [('lnl_split', 1), ('lnl_split', 2), ('lnl_split', 4), ('lnl_queue', 0), ('lnl_queue_wg', 1), ('wpb', 4),
             ('wpb_table', 8), ('lnl_cap', 2), ('prior_stage', 0), ('setup_ti', 32), ('setup_threads', 384),
             ('setup_sub', 1), ('streams', 1)]
    for key, value in knobs:
        _ffi.set_option(key, value)
        cube = make_cube(1024, 80)
        for mode in MODES:
            na.set_exp_mode(mode)
            cube_host(f'{key}={value} {mode}', cube, (1, 300, 1500, 4096), 81)
            device_group(f'{key}={value} {mode}', cube, 2, 4096, 82)
            device_group(f'{key}={value} {mode}', cube, 8, 4096, 83)
        del cube
        _ffi.set_option(key, {'lnl_queue': 1, 'wpb': 1, 'prior_stage': 1}.get(key, 0))
    print('launch_shapes done')


main()
