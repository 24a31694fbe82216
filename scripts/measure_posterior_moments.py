"""What the posterior moments cost on the device: `CubeRunner.predict_moments` against today's route to the
same numbers, `predict_batch` into a pinned buffer plus the numpy twin.

Shape: 256 segments x 512 rows, two spectra of 1024 channels, two components, both numerical modes.  HIP events through
nfa_event_* around the device work, a host clock around calls that end in a synchronise; after warm-up, the median of
REPEATS repeats.  Times taken:

  whole      the whole predict_moments call (host clock: it is synchronous; and the events around its device work)
  predict    its predict launches alone: nfa_runner_predict_batch_dev with spectra, chunk by chunk into one device buffer
  today      predict_batch into a pinned buffer, 4096 rows at a time, and `moments.posterior_moments_of` on each batch

The accumulate kernel alone is not visible to events from outside the call; its time comes from a kernel trace of this
script in a run of its own (`--trace`: a few calls and nothing else), and the bytes it reads per launch are printed here.
The script fails if the new call is not faster than today's route.

    python scripts/measure_posterior_moments.py [--out profiles/posterior_moments.txt] [--segments 256] [--rows 512]
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
CHUNK = 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'posterior_moments.txt'))
    ap.add_argument('--segments', type=int, default=256)
    ap.add_argument('--rows', type=int, default=512)
    ap.add_argument('--chan', type=int, default=1024)
    ap.add_argument('--repeats', type=int, default=REPEATS)
    ap.add_argument('--trace', action='store_true', help='three predict_moments calls per mode and nothing else (for a kernel trace)')
    args = ap.parse_args()

    import nestfit_amd as na
    from nestfit_amd import _ffi, moments
    from nestfit_amd.cube import CubeRunner
    from nestfit_amd.synth import TRUTH_2COMP, freq_axis
    lib = _ffi.engine()
    assert na.device_count() > 0, 'no GPU visible'
    name = C.create_string_buffer(256)
    _ffi.check(lib.nfa_device_name(name, 256))

    rng = np.random.default_rng(3)
    n_seg, per, n_chan = args.segments, args.rows, args.chan
    rows, chan_tot = n_seg * per, 2 * n_chan
    axes = [freq_axis(1, n_chan, 30.0), freq_axis(2, n_chan, 30.0)]
    runner = CubeRunner(axes, (1, 2), np.zeros((1, chan_tot)), np.ones((1, 2)), None, ncomp=2)
    theta = np.ascontiguousarray(TRUTH_2COMP * (1.0 + 0.02 * rng.normal(size=(rows, 12))))
    w = rng.uniform(0.0, 1.0, rows)
    off = (np.arange(n_seg + 1) * per).astype(np.int64)
    seg_pix = np.zeros(n_seg, np.int32)
    row_pix = np.zeros(rows, np.int32)
    spec_off = [0, n_chan, chan_tot]
    handle = runner._run.handle

    def events():
        a, b = C.c_void_p(), C.c_void_p()
        _ffi.check(lib.nfa_event_create(C.byref(a))); _ffi.check(lib.nfa_event_create(C.byref(b)))
        return a, b

    def elapsed(a, b):
        ms = C.c_float()
        _ffi.check(lib.nfa_event_synchronize(b)); _ffi.check(lib.nfa_event_elapsed_ms(a, b, C.byref(ms)))
        return ms.value

    ev = events()
    lines = [f'posterior moments, {name.value.decode()}', f'{n_seg} segments x {per} rows = {rows} rows, 2 x {n_chan} channels, ncomp 2; '
             f'chunks of {CHUNK} rows; median of {args.repeats} repeats after warm-up', '']
    ok = True
    for mode in ('table', 'fast'):
        runner.set_exp_mode(mode)
        if args.trace:
            for _ in range(3):
                runner.predict_moments(seg_pix, off, theta, w)
            continue
        # the whole call
        for _ in range(2):
            res = runner.predict_moments(seg_pix, off, theta, w)
        whole_host, whole_dev = [], []
        for _ in range(args.repeats):
            _ffi.check(lib.nfa_event_record(ev[0], handle))
            t0 = time.perf_counter()
            res = runner.predict_moments(seg_pix, off, theta, w)
            whole_host.append((time.perf_counter() - t0) * 1e3)
            _ffi.check(lib.nfa_event_record(ev[1], handle))
            whole_dev.append(elapsed(*ev))
        # its predict launches alone, device pointers
        d_theta, d_spec = C.c_void_p(), C.c_void_p()
        _ffi.check(lib.nfa_malloc(C.byref(d_theta), theta.nbytes))
        _ffi.check(lib.nfa_malloc(C.byref(d_spec), 8 * CHUNK * chan_tot * 8))      # a buffer per launch in flight
        _ffi.check(lib.nfa_memcpy_h2d(d_theta, theta.ctypes.data_as(C.c_void_p), theta.nbytes))
        _ffi.set_option('coalesce', 1)                   # one launch per chunk, as inside the call

        def predict_alone():
            for k, a in enumerate(range(0, rows, CHUNK)):
                nb = min(CHUNK, rows - a)
                _ffi.check(lib.nfa_runner_predict_batch_dev(handle, None, C.c_void_p(d_theta.value + a * 12 * 8), nb,
                                                            C.c_void_p(d_spec.value + (k % 8) * CHUNK * chan_tot * 8), None))
            _ffi.check(lib.nfa_runner_synchronize(handle))
        # (the launches rotate over the runner's stream lanes: the host clock around launch .. synchronise is the figure)
        pred = []
        for k in range(2 + args.repeats):
            t0 = time.perf_counter()
            predict_alone()
            if k >= 2:
                pred.append((time.perf_counter() - t0) * 1e3)
        _ffi.set_option('coalesce', 8)
        _ffi.check(lib.nfa_free(d_theta)); _ffi.check(lib.nfa_free(d_spec))
        # today's route
        pinned = _ffi.pinned_empty((CHUNK, chan_tot))

        def today():
            out = []
            for a in range(0, rows, CHUNK):
                nb = min(CHUNK, rows - a)
                spec, _ = runner.predict_batch(row_pix[a:a + nb], theta[a:a + nb], out=pinned[:nb])
                g0, g1 = a // per, (a + nb) // per
                out.append(moments.posterior_moments_of(spec, w[a:a + nb], off[g0:g1 + 1] - a, spec_off))
            return out
        assert CHUNK % per == 0, 'today\'s route takes whole segments per batch'
        ref = today()
        got = np.concatenate([r.mean for r in ref])
        scale = np.abs(got).max()
        assert np.max(np.abs(res.mean - got)) <= 1e-12 * scale, 'the two routes disagree'
        assert np.allclose(res.std, np.concatenate([r.std for r in ref]), rtol=1e-9, atol=1e-12 * scale)
        host = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            today()
            host.append((time.perf_counter() - t0) * 1e3)
        med = statistics.median
        n_chunks = -(-rows // CHUNK)
        acc_bytes = CHUNK * chan_tot * 8
        lines += [f'mode {mode}',
                  f'  whole predict_moments call     {med(whole_host):10.2f} ms host clock   {med(whole_dev):10.2f} ms between events '
                  f'(min {min(whole_host):.2f}, max {max(whole_host):.2f})',
                  f'  its {n_chunks} predict launches alone {med(pred):10.2f} ms host clock, launch .. synchronise '
                  f'({med(pred) / n_chunks * 1e3:.1f} us per chunk of {CHUNK} rows; min {min(pred):.2f}, max {max(pred):.2f})',
                  f'  today: predict_batch + numpy   {med(host):10.2f} ms host clock (min {min(host):.2f}, max {max(host):.2f})',
                  f'  new call / today               {med(whole_host) / med(host):10.4f}',
                  f'  accumulate launch reads        {acc_bytes / 1e6:10.1f} MB per chunk ({n_chunks} launches per call): its time is in the kernel trace',
                  '']
        ok = ok and med(whole_host) < med(host)
    if args.trace:
        print('trace run done')
        return 0
    text = '\n'.join(lines)
    print(text)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text + '\n')
    if not ok:
        print('FAIL: predict_moments is not faster than predict_batch + numpy')
        return 1
    return 0


if __name__ == '__main__':
    sys.exit(main())
