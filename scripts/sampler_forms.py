"""usage: python scripts/sampler_forms.py        the device sampler once per form of its plan (one MI355X)
       python scripts/sampler_forms.py --rate   rounds per second of one-pixel runs: the host's work per round

One short run of `run_nested_device` for every form `ns_plan` (csrc/nfa_sampler_plan.h) can give a run -- several
ellipsoids, one ellipsoid, the sheared ellipsoid with boxes and pair ellipses and each of them turned off, walks, live
points per pixel, live points that are not staged, the sibling models, every `sampler_*` process option off its
default -- and a checksum of n_iter, n_evals, rounds and the posterior tables of each.  It is deterministic (fixed
seeds, one process), so two builds of the engine can be compared: run it under
`rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/sampler_forms.py` with each, reduce the traces with
`scripts/launch_shapes.py --shapes`, and diff the two lists and the two outputs (profiles/sampler_plan/README.md)."""
import hashlib
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np

import nestfit_amd as na
from nestfit_amd import _ffi, sampler
from nestfit_amd.cube import CubeRunner
from nestfit_amd.synth import CKMS, freq_axis

TRUTH = {1: [-0.5, 14.0, 6.0, 14.5, 0.5, 0.0],
         2: [-0.5, 1.0, 12.0, 15.0, 5.0, 6.0, 14.4, 14.6, 0.4, 0.4, 0.0, 0.0],
         3: [-1.5, 0.0, 1.6, 12.0, 14.0, 15.0, 5.0, 5.5, 6.0, 14.4, 14.5, 14.6, 0.35, 0.4, 0.35, 0.0, 0.0, 0.0]}
# (key, a value off its default, the default)
OPTIONS = [('sampler_parts', 2, 3), ('sampler_refit_every', 2, 4), ('sampler_walkers', 64, 0), ('sampler_ellipsoids', 1, 0),
           ('sampler_walk_factor', 8, 0), ('sampler_frames', 8, -2), ('sampler_margin_pct', 150, 0), ('sampler_ktarget', 0, -1),
           ('sampler_pairs_pct', 0, -1), ('sampler_ratio_max', 8, 0), ('sampler_kmax', 1024, 0), ('sampler_shear_pct', 250, -1)]


def run(tag, cube, n_pix, **kw):
    res = sampler.fit_pixels(cube, np.arange(n_pix), tol=0.5, efr=0.3, **kw)
    h = hashlib.sha1()
    for r in res:
        h.update(np.array([r.n_iter, r.n_evals, r.rounds], dtype=np.int64).tobytes())
        h.update(np.ascontiguousarray(r.posterior).tobytes())
    print(f'{tag}: n_iter {[r.n_iter for r in res]} n_evals {[r.n_evals for r in res]} rounds {res[0].rounds} sha1 {h.hexdigest()[:16]}', flush=True)


def ammonia_cube(ncomp, n_pix, seed, n=128, noise=0.1):
    rng = np.random.default_rng(seed)
    axes = [freq_axis(1, n), freq_axis(2, n)]
    ut = na.get_irdc_priors(size=500, vsys=0.0)
    truths = np.tile(np.array(TRUTH[ncomp]), (n_pix, 1))
    truths[:, 3 * ncomp] += 0.2 * np.arange(n_pix)                     # (ntot of the first component)
    probe = CubeRunner(axes, (1, 2), np.zeros((1, 2 * n)), np.full((1, 2), noise), ut, ncomp=ncomp)
    model, _ = probe.predict_batch(np.zeros(n_pix, dtype=np.int32), truths)
    return CubeRunner(axes, (1, 2), model + rng.normal(0, noise, model.shape), np.full((n_pix, 2), noise), ut, ncomp=ncomp)


def sibling_cube(model, n_pix, seed, n=256, noise=0.1):
    x = np.linspace(0, 1, 200)
    ranges = [(-4, 4), (2.8, 20), (-1.5, 1.0), (0.1, 1.5)] if model == 1 else [(-15, 15), (0.2, 3.0), (0.0, 5.0)]
    ut = na.PriorTransformer([na.Prior(na.Distribution(lo + x * (hi - lo), np.full(x.size, 1.0 / (hi - lo))), k)
                              for k, (lo, hi) in enumerate(ranges)])
    nu0 = 93173.7637e6 if model == 1 else 110.201354e9
    f = nu0 * (1.0 - np.linspace(15, -15, n) / CKMS)
    truth = np.array([0.5, 7.0, 0.3, 0.4] if model == 1 else [-2.0, 1.2, 1.5])
    kw = dict(model=1) if model == 1 else dict(model=2, rest_freqs=[nu0])
    probe = CubeRunner([f], [1], np.zeros((1, n)), np.full((1, 1), noise), ut, ncomp=1, **kw)
    spec, _ = probe.predict_batch(np.zeros(n_pix, dtype=np.int32), np.tile(truth, (n_pix, 1)))
    return CubeRunner([f], [1], spec + np.random.default_rng(seed).normal(0, noise, spec.shape), np.full((n_pix, 1), noise), ut, ncomp=1, **kw)


def rate():
    """One pixel: the GPU work of a round is at its smallest, what is left is the host's share (launches, the wait for
    the row count).  The second run of each cube is the one to read: the first loads the code objects."""
    for ncomp, cube in ((1, ammonia_cube(1, 1, 21)), (2, ammonia_cube(2, 1, 3))):
        for _ in range(2):
            r = sampler.fit_pixels(cube, np.arange(1), nlive=400, tol=0.5, efr=0.3, seed=5, maxiter=4000)[0]
        print(f'one pixel, {ncomp} comp: {r.rounds} rounds in {r.timings["rounds"]:.3f} s = {r.rounds / r.timings["rounds"]:.0f} rounds/s '
              f'(n_iter {r.n_iter}, n_evals {r.n_evals})', flush=True)


def main():
    assert na.device_count() > 0, 'no GPU visible'
    na.set_exp_mode('table')
    if '--rate' in sys.argv:
        return rate()
    one, two, three = ammonia_cube(1, 3, 21), ammonia_cube(2, 3, 3), ammonia_cube(3, 2, 4)
    k1 = dict(nlive=60, seed=33)
    k2 = dict(nlive=150, seed=7, batch_target=2048, maxiter=900)
    # five sampled dimensions: several ellipsoids, one, one with boxes; the three methods; live points per pixel; not staged
    run('1 comp', one, 3, **k1)
    run('1 comp ellipsoids=1', one, 3, ellipsoids=1, **k1)
    run('1 comp ellipsoids=2', one, 3, ellipsoids=2, **k1)
    run('1 comp ellipsoids=1 frames=8 margin=1.5', one, 3, ellipsoids=1, frames=8, margin=1.5, **k1)
    run('1 comp ellipsoids=1 frames=0', one, 3, ellipsoids=1, frames=0, **k1)
    run('1 comp reject', one, 3, method='reject', **k1)
    run('1 comp walk', one, 3, method='walk', n_steps=7, maxiter=400, **k1)
    run('1 comp walk nlive=400', one, 3, method='walk', n_steps=5, maxiter=500, nlive=400, seed=33)
    run('1 comp nlive per pixel', one, 3, nlive=np.array([60, 71, 83]), seed=33)
    run('1 comp nlive per pixel walk', one, 3, nlive=np.array([60, 71, 83]), seed=33, method='walk', n_steps=7, maxiter=500)
    for nlive in (1500, 2600):                              # 60 KB staged / 104 KB not
        run(f'1 comp nlive={nlive}', one, 1, nlive=nlive, seed=12, maxiter=nlive // 2, batch_target=4096)
    # ten: the sheared ellipsoid with boxes and pair ellipses, and each of them turned off or set
    run('2 comp', two, 3, **k2)
    for extra in (dict(shear=0), dict(frames=-1), dict(frames=8, margin=1.5), dict(pairs=0), dict(shear=0, frames=32), dict(shear=4.0, pairs=2.5),
                  dict(precision='speed'), dict(precision='default'), dict(precision='evidence'),
                  dict(method='reject'), dict(method='auto', n_steps=20), dict(method='walk', n_steps=20, maxiter=300)):
        run(f'2 comp {extra}', two, 3, **{**k2, **extra})
    run('2 comp nlive=1300', two, 2, nlive=1300, seed=3, maxiter=2000, batch_target=4096, method='reject')
    run('2 comp nlive per pixel', two, 3, **{**k2, 'nlive': np.array([150, 160, 171])})
    # fifteen
    run('3 comp', three, 2, nlive=200, seed=11, batch_target=2048, method='reject', maxiter=1200)
    run('3 comp pairs=0', three, 2, nlive=200, seed=11, batch_target=2048, maxiter=800, pairs=0)
    # the sibling models: four and three sampled dimensions
    run('n2hp', sibling_cube(1, 3, 4), 3, nlive=80, seed=6)
    run('gaussian', sibling_cube(2, 3, 5), 3, nlive=80, seed=7)
    # every process option off its default, one at a time
    for key, value, default in OPTIONS:
        _ffi.set_option(key, value)
        run(f'{key}={value} 1 comp', one, 3, **k1)
        run(f'{key}={value} 2 comp', two, 3, **k2)
        _ffi.set_option(key, default)
    print('sampler_forms done')


main()
