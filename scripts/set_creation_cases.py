"""What the seven creators of include/nestfit_amd.h make and refuse, for comparing two builds of the engine
with diff (profiles/set_creation/): for every creator, a scalar noise, the same noise per channel and a varying noise per
channel with a masked channel, one and two components, both numerical modes -- a digest of predict_batch's spectra, of its
lnL and of null_lnZ; then every (rc, message) the refusal table of tests/set_decl_cases.py gets, with the number and a digest
of the inputs (entry point and label) that got it: 1167 inputs, a line each would say the same at ten times the length.  Deterministic, one
process, needs a GPU.  NFA_ENGINE_LIB selects the library (nestfit_amd/_ffi.py).

    python scripts/set_creation_cases.py > cases.txt
"""
import ctypes as C
import hashlib
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / 'tests')]
import set_decl_cases as sd                                  # noqa: E402
from nestfit_amd import _ffi                                 # noqa: E402


def digest(a):
    return hashlib.sha256(a.tobytes()).hexdigest()[:16]


def main():
    lib = _ffi.engine()
    for mode in (0, 2):
        _ffi.check(lib.nfa_set_exp_mode(mode))
        for name in sd.NAMES:
            scalar = sd.full(name, lib)
            for kind, d in (('scalar', scalar), ('channel', sd.per_channel(scalar)), ('masked', sd.per_channel(scalar, masked=True))):
                runs = [sd.evaluate(lib, d, name, ncomp) for ncomp in (1, 2)]
                said = ' | '.join(f'ncomp {k + 1}: spectra {digest(spec)} lnL {digest(lnl)}' for k, (spec, lnl, _) in enumerate(runs))
                print(f'{name} | {kind} | mode {mode} | {said} | null_lnZ {digest(runs[0][2])}')
    _ffi.check(lib.nfa_set_exp_mode(2))
    said = {}                                                # (rc, message) -> the inputs that got it, in the table's order
    for k, (label, d, _, _) in enumerate(sd.REFUSALS):
        rc, msg, h = sd.call_creator(lib, d, handle=C.c_void_p())
        said.setdefault((rc, msg), []).append(f'{k} {d["entry"]} {label}')
        if rc == 0:
            lib.nfa_specset_destroy(h)
    for (rc, msg), inputs in said.items():
        print(f'{rc} | {msg} | {len(inputs)} inputs {digest(np.array(inputs))}')


if __name__ == '__main__':
    main()
