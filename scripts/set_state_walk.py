"""usage: python scripts/set_state_walk.py  -- the setter walk of tests/test_set_state.py without its comparisons: every step
of the fixed list on one live two-pixel set per noise kind (scalar, per channel, per channel with a masked channel), and new
data in pixel 1 and back in every state with an option on.  The walk's list, data and values are those of
tests/test_set_state.py, which it imports (to run it on an earlier commit, copy that file and tests/test_set_state_cpu.py there); the package has no public set_data, so that call goes through `_ffi`; the
setters are the set's own (`runner._ss`), for a CubeRunner has no set_calibration.  No likelihood launch: under a kernel
trace with statistics the run counts the dispatches of the set-up kernels (chan_weight_kernel, corr_setup_kernel, rowsq*,
totsq_kernel, bl_setup_kernel, tmpl_setup_kernel, nmarg_setup_kernel, rob_setup_kernel) that the setters and
nfa_specset_set_data make, for comparison between two commits (profiles/set_state/README.md)."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / 'tests')]

import nestfit_amd as engine                                 # noqa: E402
from nestfit_amd import _ffi                                 # noqa: E402
import test_set_state as walk                                # noqa: E402
from test_layered import _ranges                             # noqa: E402
from test_sibling_models import _simple_priors               # noqa: E402

lib = _ffi.engine()
ut = _simple_priors(engine, _ranges('ammonia'))
n_steps = n_data = 0
for kind in walk.KINDS:
    data, other, noise = walk._data(engine, kind)
    values = walk._values(data.shape[1] // 2)
    live = walk._cube(engine, ut, data, noise, {})
    on = set()
    for name, which in walk._walk(kind == 'masked')[0]:
        getattr(live._ss, 'set_' + name.replace('_order', ''))(None if which is None else values[name][2 if which == 'zero' else which])
        (on.add if which in (0, 1) else on.discard)(name)
        n_steps += 1
        if on:
            _ffi.check(lib.nfa_specset_set_data(live._ss.handle, 1, _ffi.dptr(other)))
            _ffi.check(lib.nfa_specset_set_data(live._ss.handle, 1, _ffi.dptr(np.ascontiguousarray(data[1]))))
            n_data += 2
    assert not on
    del live
_ffi.check(lib.nfa_device_synchronize())
print(f'{n_steps} setter calls, {n_data} nfa_specset_set_data calls')
