"""Child of tests/test_component_counts.py, run with NFA_ENGINE_LIB = the test library: the launches of
test_unit_queue_matches_one_unit_per_wave (table mode, lnl_queue 1) at 4, 7 and 10 components with the queue kernel's
trace attached (nfa_test_queue_trace: the last launch's units, per wave).  Prints one JSON line."""
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

import nestfit_amd as na  # noqa: E402
from nestfit_amd import _ffi  # noqa: E402
from nestfit_amd.synth import freq_axis  # noqa: E402
from test_component_counts import _tiled, _wide, usable_rows  # noqa: E402

TRACE_WAVES = 8192                       # NFA_TRACE_WAVES: waves x 8 records x {start, end, unit, position}

lib = _ffi.engine()
rng = np.random.default_rng(3)
trans, n = (1, 2), 512
spec_data = [[freq_axis(t, n), rng.normal(0, 0.2, n), 0.2, t] for t in trans]
B = 16384 // len(trans) + 16 * 40 + 1
na.set_exp_mode('table')
_ffi.set_option('lnl_queue', 1)
out = {}
for ncomp in (4, 7, 10):
    ut = _wide(na)
    run = na.AmmoniaRunner.from_data(spec_data, ut, ncomp=ncomp)
    U = _tiled(usable_rows(ut, ncomp, 1024, seed=30 + ncomp), B)
    _ffi.check(lib.nfa_device_synchronize())
    _ffi.check(lib.nfa_test_queue_trace(1))                           # cleared
    _ffi.check(lib.nfa_device_synchronize())
    lnl = run.loglikelihood_batch(U)
    buf = np.zeros(TRACE_WAVES * 8 * 4, dtype=np.uint64)
    _ffi.check(lib.nfa_test_queue_trace_read(buf.ctypes.data_as(C.POINTER(C.c_ulonglong))))
    rec = buf.reshape(TRACE_WAVES, 8, 4).astype(np.int64)
    used = rec[:, :, 1] > 0                                           # a record has an end time
    out[str(ncomp)] = {'queue': bool(used.any()), 'units_recorded': int(used.sum()), 'waves': int(used.any(1).sum()),
                       'finite': bool(np.isfinite(lnl).all())}
_ffi.check(lib.nfa_test_queue_trace(0))
na.set_exp_mode('fast')
print(json.dumps(out))
