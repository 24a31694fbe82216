"""Digests of the numpy twin's results (`sampler.run_nested`): one SHA-256 per case over everything a run returns, so
that two trees can be compared bit for bit.  The cases execute every statement of `run_nested`: several ellipsoids, one
ellipsoid, walks, the automatic switch there and back, a free mask, the caps, a NaN likelihood, boxes, the shear, the
pair ellipses and the named precisions.

    python scripts/twin_digest.py [--only SUBSTRING]

prints per case the digest, every pixel's n_iter and n_evals, the rounds and the seconds, and the total time last."""
import argparse
import hashlib
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from nestfit_amd import sampler                                  # noqa: E402


def gauss(centres, sigma):
    centres = np.atleast_2d(np.asarray(centres, dtype=np.float64))

    def loglike(pix, U):
        d2 = ((U[:, None, :] - centres[None]) ** 2).sum(axis=2)
        return np.logaddexp.reduce(-0.5 * d2 / sigma ** 2, axis=1)
    return loglike


def like5(pix, U):                                               # depends on slots 0, 2, 3 only
    assert (U[:, 1] == 0.5).all() and (U[:, 4] == 0.5).all()
    return -0.5 * ((U[:, [0, 2, 3]] - 0.5) ** 2).sum(axis=1) / 0.05 ** 2


def nan_loglike(pix, U):
    out = gauss([.5] * 2, 0.1)(pix, U)
    out[U[:, 0] < 0.2] = np.nan
    return out


def cube_like(pix, U):
    d = np.maximum(np.abs(U - 0.5).max(axis=1) - 0.11, 0.0)
    return -0.5 * (d / 0.004) ** 2 - 0.5 * (((U - 0.5) / 0.2) ** 2).sum(axis=1)


def ridge(pix, T):
    U = T[:, :10] - 0.5
    d = U.copy()
    d[:, 6] -= 3.0 * U[:, 4] ** 2 - 0.05
    d[:, 7] += 3.0 * U[:, 5] ** 2 - 0.05
    s = np.full(10, 0.08)
    s[[6, 7]] = 0.01
    return -0.5 * ((d / s) ** 2).sum(axis=1)


def there_and_back(pix, U):
    return np.logaddexp(-0.5 * (((U - .25) / .02) ** 2).sum(axis=1), -20.0 - 0.5 * (((U - .75) / .05) ** 2).sum(axis=1))


class Transitions:
    """A `progress` with `detail`: the rounds after which pixel 0 turned to walks and back to rejection."""

    def __init__(self):
        self.walking, self.to_walk, self.back = False, [], []

    def __call__(self, n_active, n_iter):
        pass

    def detail(self, d):
        now = bool(d['walk'][0])
        if now != self.walking:
            (self.to_walk if now else self.back).append(int(d['rnd']))
        self.walking = now


FM = np.array([1] * 10 + [0, 0])
TWO = gauss([[.25] * 5, [.75] * 5], 0.01)
BOX = dict(nlive=200, tol=.5, efr=.3, seed=11, method='reject', batch_target=1024, frames=16)
RIDGE = dict(nlive=200, tol=.5, efr=.3, seed=3, batch_target=512, free_mask=FM)
AUTO = dict(nlive=100, tol=.5, seed=4, batch_target=512)
# name, likelihood, unit-cube slots, pixels, keywords
CASES = [
    ('several ellipsoids', gauss([.4] * 3, .1), 3, 3, dict(nlive=60, seed=7)),
    ('live points per pixel', gauss([.4] * 3, .1), 3, 4, dict(nlive=np.array([60, 75, 90, 75]), seed=7)),
    ('one ellipsoid', gauss([.5] * 5, .05), 5, 2, dict(nlive=100, seed=2, ellipsoids=1)),
    ('walks from the start', gauss([.5] * 6, .04), 6, 2, dict(nlive=150, tol=.1, efr=.5, seed=21, method='walk', n_steps=20,
                                                             batch_target=512)),
    ('auto -> walks', TWO, 5, 1, dict(n_steps=20, walk_factor=2, ellipsoids=1, **AUTO)),
    ('auto, several ellipsoids', TWO, 5, 1, dict(AUTO)),
    ('free mask', like5, 5, 3, dict(nlive=150, tol=.1, efr=.5, seed=9, free_mask=[1, 0, 1, 1, 0])),
    ('maxiter=30', gauss([.5] * 2, .1), 2, 2, dict(nlive=50, seed=1, maxiter=30)),
    ('maxiter=0', gauss([.5] * 2, .1), 2, 1, dict(nlive=50, seed=1, maxiter=0)),
    ('cap_iter=40', gauss([.5] * 2, .1), 2, 2, dict(nlive=50, seed=1, cap_iter=40)),
    ('NaN likelihood', nan_loglike, 2, 1, dict(nlive=80, seed=3)),
    ('boxes', cube_like, 8, 2, dict(BOX)),
    ('boxes, k_target=0', gauss([.5] * 8, .05), 8, 1, dict(k_target=0, **BOX)),
    ('shear + boxes + pairs', ridge, 12, 1, dict(method='reject', **RIDGE)),
    ('shear alone', ridge, 12, 1, dict(method='reject', shear=4.0, frames=-1, **RIDGE)),
    ("precision='speed', auto", ridge, 12, 2, dict(precision='speed', **RIDGE)),
    ("precision='evidence'", ridge, 12, 1, dict(RIDGE, seed=5, precision='evidence')),
    ('to walks and back', there_and_back, 7, 1, dict(nlive=150, tol=.5, efr=.5, seed=3, method='auto', n_steps=20, walk_factor=2,
                                                     ellipsoids=1, batch_target=512)),
]


def digest(results):
    h = hashlib.sha256()
    for r in results:
        h.update(np.ascontiguousarray(r.posterior, dtype=np.float64).tobytes())
        h.update(np.ascontiguousarray(r.param_constr, dtype=np.float64).tobytes())
        h.update(np.array([r.lnZ, r.lnZ_err, r.max_loglike, r.information], dtype=np.float64).tobytes())
        h.update(np.array([r.n_live, r.n_evals, r.n_iter, r.n_samples, int(r.truncated), r.rounds], dtype=np.int64).tobytes())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--only', default='', help='run the cases whose name contains this')
    args = ap.parse_args()
    total = 0.0
    for name, like, ndim, n_pix, kw in CASES:
        if args.only not in name:
            continue
        watch = Transitions() if name == 'to walks and back' else None
        t0 = time.perf_counter()
        res = sampler.run_nested(like, ndim, n_pix, progress=watch, **kw)
        dt = time.perf_counter() - t0
        total += dt
        print(f'{name:26s} {digest(res)}  n_iter {[r.n_iter for r in res]}  n_evals {[r.n_evals for r in res]}  '
              f'rounds {res[0].rounds}  {dt:.2f} s', flush=True)
        if watch is not None:
            assert watch.to_walk and watch.back and watch.to_walk[0] < watch.back[0], (watch.to_walk, watch.back)
            print(f'{"":26s} to walks after round {watch.to_walk}, back after round {watch.back}')
    print(f'total {total:.2f} s')


if __name__ == '__main__':
    main()
