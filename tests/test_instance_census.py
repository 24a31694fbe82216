"""Every instance of the likelihood kernel, launched once and held to a restatement (208 (instance, form) pairs).

tests/instance_census.py has one case per pair that lnl_instance_exists admits; tests/test_launch_plan.py holds that table to
the rule without a GPU.  Here every case runs on the device, in child processes on the test library
(tests/instance_census_worker.py): predict_batch at lnl_split 0 and 1 gives the same bits; the test library's launch
counters (nfa_test_lnl_launches: launch_lnl counts every launch on the entry of the engine's table of instances that holds
the kernel it launched, found by the kernel's address) show the case's instance and form and no other;
lnL agrees with calib_restatement.marginal_lnl in longdouble on the spectra of layer_restatement -- rtol LNL_RTOL[mode] for
the kinds without the baseline bit, |got - want| <= K_BOUND LNL_RTOL[mode] M for those with it (test_calibration.py's bound);
and for the spectra-out cases every channel is within ncomp TIGHT[mode] S plus the floor of test_layered._check_layered, the
zero pattern S's.  The queue cases also run a launch too small for the queue (the plain or w8 instance of the same NCOMP, the
same bits) and every tiled copy of a reference row gives the same bits.  The bounds are the sibling tests'; none is new.

Measured on an MI355X, the worst deviation over the cases of a group (spectra: |got - want| / S against ncomp x 1e-11 in the
table mode, ncomp x 5e-7 in the fast mode; lnL: relative against 1e-9 / 1e-6, and |got - want| / M against the same):

    group (cases)                  spectra / S    lnL, relative    lnL / M
    table, narrow, unrolled (24)   2.4e-15        4.0e-15          8.1e-16
    table, narrow, general (26)    2.2e-15        1.6e-15          7.1e-16
    table, wide, unrolled (24)     7.6e-16        1.2e-14          7.8e-16
    table, wide, general (26)      7.4e-16        7.8e-16          9.1e-16
    fast, narrow, unrolled (24)    3.0e-7         6.2e-8           3.5e-8
    fast, narrow, general (26)     2.8e-7         5.1e-8           4.3e-8
    fast, wide, unrolled (24)      2.7e-7         5.2e-8           1.2e-8
    fast, wide, general (26)       2.3e-7         6.5e-8           3.3e-8
    queue (8)                      2.8e-15        1.5e-15          (no baseline)

The spectra come closest to their bound in the fast mode at one component: 0.54 of it.  Every child takes 1 to 2 s on the
device and 2 to 4 s in all.
"""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

import instance_census as ic

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize('group', ic.GROUPS)
def test_every_instance_of_the_group_is_launched_and_right(engine, group):
    from nestfit_amd import _ffi
    env = dict(os.environ, NFA_ENGINE_LIB=str(_ffi.TEST_LIB_PATH))
    res = subprocess.run([sys.executable, str(ROOT / 'tests' / 'instance_census_worker.py'), group], env=env, cwd=str(ROOT),
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    out = json.loads(res.stdout.strip().splitlines()[-1])
    print(f'census {group}: {out["cases"]} cases in {out["seconds"]} s on {out["n_cu"]} CUs; worst {out["worst"]}')
    cases = [c for c in ic.CASES if c.group == group]
    assert out['cases'] == len(cases) and not out['failures'], out['failures']
    # every case's pair was counted, twice (lnl_split 0 and 1); beside them only the queue cases' small launches
    want = {(c.index, c.form): 2 for c in cases}
    want.update({(c.index, ic.small_form(c)): 1 for c in cases if c.form == ic.QUEUE})
    assert {(i, f): n for i, f, n in out['launched']} == want
