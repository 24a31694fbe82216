"""Child of tests/test_coalesced_launches.py (case 7), run with NFA_ENGINE_LIB = the test library: one group of each of
the benchmark's coalesced launches with the queue kernel's trace attached (nfa_test_queue_trace: the last launch's
units, per wave), and which batches of the group had units drawn.  Prints one JSON line."""
import ctypes as C
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'tests'))
assert 'libnestfit_amd_test' in os.environ.get('NFA_ENGINE_LIB', ''), 'run with NFA_ENGINE_LIB = the test library'

import numpy as np  # noqa: E402

import bench  # noqa: E402
import nestfit_amd as na  # noqa: E402
from device_buffers import DeviceArrays  # noqa: E402
from nestfit_amd import _ffi  # noqa: E402
from nestfit_amd.cube import CubeRunner  # noqa: E402
from nestfit_amd.synth import freq_axis  # noqa: E402

TRACE_WAVES = 8192                       # NFA_TRACE_WAVES: waves x 8 records x {start, end, unit, position}

lib = _ffi.engine()
name = C.create_string_buffer(256)
_ffi.check(lib.nfa_device_name(name, 256))
n_cu = int(name.value.decode().split(',')[-1].split()[0])
rng = np.random.default_rng(3)


def cube_of(workload):
    trans, n_chan, vhalf, ncomp, _, rows = bench.WORKLOADS[workload]
    axes = [freq_axis(t, n_chan, vhalf) for t in trans]
    data = rng.normal(0, 0.2, (2, len(trans) * n_chan))
    return CubeRunner(axes, trans, data, np.full((2, len(trans)), 0.2), na.get_irdc_priors(size=500, vsys=0.0),
                      ncomp=ncomp), rows


def traced(cube, n, rows, predict=False):
    """n batches of `rows` sent back to back and synchronised once; which batches the queue kernel drew units of."""
    h = cube._run.handle
    dev = DeviceArrays(lib, _ffi.check)
    try:
        calls = []
        for k in range(n):
            U = rng.uniform(size=(rows, cube.ndim))
            pix = np.full(rows, k % 2, dtype=np.int32)
            if predict:
                cube.loglikelihood_batch(pix, U)                      # U -> physical parameters
            calls.append((dev.upload(pix), dev.upload(U), dev.empty(8 * rows),
                          dev.empty(8 * rows * cube.n_chan_tot) if predict else None))
        _ffi.check(lib.nfa_device_synchronize())
        _ffi.check(lib.nfa_test_queue_trace(1))                       # cleared
        _ffi.check(lib.nfa_device_synchronize())
        for d_p, d_u, d_l, d_s in calls:
            if predict:
                _ffi.check(lib.nfa_runner_predict_batch_dev(h, d_p, d_u, rows, d_s, d_l))
            else:
                _ffi.check(lib.nfa_runner_loglike_batch_dev(h, d_p, d_u, d_l, rows))
        _ffi.check(lib.nfa_runner_synchronize(h))
        buf = np.zeros(TRACE_WAVES * 8 * 4, dtype=np.uint64)
        _ffi.check(lib.nfa_test_queue_trace_read(buf.ctypes.data_as(C.POINTER(C.c_ulonglong))))
    finally:
        dev.free()
    rec = buf.reshape(TRACE_WAVES, 8, 4).astype(np.int64)
    used = rec[:, :, 1] > 0                                           # a record has an end time
    units = rec[:, :, 2][used]
    batches = sorted({int(b) for b in np.unique(units // cube.n_spec // rows)})
    return {'n': n, 'rows': rows, 'queue': bool(used.any()), 'units_recorded': int(used.sum()),
            'waves': int(used.any(1).sum()), 'batches': batches}


na.set_exp_mode('table')
_ffi.set_option('coalesce', 8)
c2, rows2 = cube_of('C2')
c4, rows4 = cube_of('C4')
out = {'n_cu': n_cu}
out['C2 n=8'] = traced(c2, 8, rows2)
out['C2 n=2'] = traced(c2, 2, rows2)
out['C2 n=1'] = traced(c2, 1, rows2)
out['C2 spectra n=8'] = traced(c2, 8, rows2, predict=True)
out['C4 n=5'] = traced(c4, 5, rows4)
_ffi.check(lib.nfa_test_queue_trace(0))
na.set_exp_mode('fast')
print(json.dumps(out))
