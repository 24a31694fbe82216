"""Child of tests/test_instance_census.py, run with NFA_ENGINE_LIB = the test library and the name of a group of
tests/instance_census.py's cases: every case of the group is launched through predict_batch at lnl_split 0 and 1, the test
library's launch counters (nfa_test_lnl_launches) must show the case's (instance, form) and nothing else, and lnL and the
spectra are held to the restatements at the sibling tests' bounds.  A failed check is recorded and the next case runs; an
engine error ends the child.  Prints one JSON line."""
import ctypes as C
import json
import os
import re
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'tests'))
assert 'libnestfit_amd_test' in os.environ.get('NFA_ENGINE_LIB', ''), 'run with NFA_ENGINE_LIB = the test library'

import numpy as np  # noqa: E402

import instance_census as ic  # noqa: E402
import nestfit_amd as na  # noqa: E402
from nestfit_amd import _ffi  # noqa: E402
from test_calibration import K_BOUND  # noqa: E402
from test_layered import MODELS, _check_layered  # noqa: E402
from test_sibling_models import LNL_RTOL, TIGHT  # noqa: E402

t_start = time.time()
group = sys.argv[1]
cases = [c for c in ic.CASES if c.group == group]
assert cases, group
lib = _ffi.engine()
hook = lib.nfa_test_lnl_launches
hook.restype, hook.argtypes = _ffi.TEST_SIGNATURES['nfa_test_lnl_launches']


def launches():
    """{(instance index, form): launches} since the last call; the counters are cleared."""
    out = np.zeros((1024, 5), dtype=np.int64)
    _ffi.check(hook(out.ctypes.data_as(C.POINTER(C.c_int64)), 1))
    return {(int(i), int(f)): int(out[i, f]) for i, f in zip(*np.nonzero(out))}


def compute_units():
    buf = C.create_string_buffer(256)
    _ffi.check(lib.nfa_device_name(buf, 256))
    return int(re.search(r'(\d+) CUs', buf.value.decode()).group(1))


N_CU = compute_units()
launched = {}


def predict(case, rows, theta, split):
    _ffi.set_option('lnl_split', split)                    # (a runner reads the option when it is made)
    try:
        run = ic.make_runner(na, case, rows)
    finally:
        _ffi.set_option('lnl_split', 0)
    spec, lnl = run.predict_batch(theta.copy(), want_spectra=case.spectra)
    assert np.isfinite(lnl).all() and (spec is None) == (not case.spectra)
    return spec, lnl


def same_bits(a, b):
    return np.array_equal(a[1], b[1]) and (a[0] is None or np.array_equal(a[0], b[0]))


def check(case):
    """-> (worst |got - want| / S of the spectra or None, worst relative lnL deviation or None, worst |got - want| / M or None)"""
    mode, ncomp = case.mode, case.ncomp
    rows, thetas, want_spec, S, want_lnl, M = ic.wanted_of(case)
    ic.check_draws(case.set, ncomp, case.layered)
    na.set_exp_mode(mode)
    launches()
    n = ic.rows_of(case, N_CU)
    theta = np.ascontiguousarray(np.resize(thetas, (n, thetas.shape[1])))
    if case.form == ic.QUEUE:
        # a first launch too small for the queue: the plain or w8 instance of the same NCOMP, and the same bits
        small = predict(case, rows, theta[:ic.N_ROWS], 0)
        seen = launches()
        assert seen == {(case.index, ic.small_form(case)): 1}, f'the small launch was counted as {seen}'
        launched[(case.index, ic.small_form(case))] = launched.get((case.index, ic.small_form(case)), 0) + 1
    got = predict(case, rows, theta, 0)
    other = predict(case, rows, theta, 1)
    seen = launches()
    for key, count in seen.items():
        launched[key] = launched.get(key, 0) + count
    assert seen == {(case.index, case.form): 2}, f'counted {seen}, the case names {(case.index, case.form)}'
    assert same_bits(got, other), 'lnl_split 0 and 1 differ'
    spec, lnl = got
    if n > ic.N_ROWS:                                       # tiled rows: every copy of a reference row, the same bits
        copy_of = np.arange(n) % ic.N_ROWS
        assert np.array_equal(lnl, lnl[:ic.N_ROWS][copy_of]) and (spec is None or np.array_equal(spec, spec[:ic.N_ROWS][copy_of]))
        assert same_bits(small, (None if spec is None else spec[:ic.N_ROWS], lnl[:ic.N_ROWS])), 'the queue and the small launch differ'
        lnl = lnl[:ic.N_ROWS]
        spec = None if spec is None else spec[:ic.N_ROWS]
    dev = np.abs(lnl - want_lnl)
    worst_rel, worst_m = None, None
    if ic.kind_of(case) & ic.K_BASELINE:
        worst_m = float((dev / M).max())
        assert (dev <= K_BOUND * LNL_RTOL[mode] * M).all(), f'lnL: worst |got - want| / M {worst_m:.3e}'
    else:
        worst_rel = float((dev / np.abs(want_lnl)).max())
        np.testing.assert_allclose(lnl, want_lnl, rtol=LNL_RTOL[mode])
    worst_spec = None
    if case.spectra:
        tex_row = MODELS[ic.SETS[case.set]['model']]['tex_row']
        worst_spec = 0.0
        for sp, ws, s, th in zip(spec, want_spec, S, thetas):              # every row, every channel
            worst_spec = max(worst_spec, _check_layered(sp, ws, s, mode, ncomp, th[tex_row * ncomp:(tex_row + 1) * ncomp]))
    return worst_spec, worst_rel, worst_m


failures, worst = [], {'spec_over_S': 0.0, 'spec_over_bound': 0.0, 'lnl_rel': 0.0, 'lnl_over_M': 0.0}
for case in cases:
    try:
        ws, wr, wm = check(case)
    except AssertionError as e:
        failures.append({'case': case._asdict(), 'error': str(e)[:600]})
        continue
    if ws is not None:
        worst['spec_over_S'] = max(worst['spec_over_S'], ws)
        worst['spec_over_bound'] = max(worst['spec_over_bound'], ws / (case.ncomp * TIGHT[case.mode]))
    if wr is not None:
        worst['lnl_rel'] = max(worst['lnl_rel'], wr)
    if wm is not None:
        worst['lnl_over_M'] = max(worst['lnl_over_M'], wm)
na.set_exp_mode('fast')
print(json.dumps({'group': group, 'n_cu': N_CU, 'cases': len(cases), 'failures': failures, 'worst': worst,
                  'launched': sorted([i, f, n] for (i, f), n in launched.items()), 'seconds': round(time.time() - t_start, 1)}))
