#!/usr/bin/env python3
"""What tests/test_oracle_pin.py holds the oracle's FastExp against where the reference's own build is absent:
the reference's nestfit/core/fastexp.c compiled as it lies by oracle/Makefile into oracle/_ref/ (tables
calcExpTableEntries(3, 8) like includes/model_includes.pxi:12), run on the seeded inputs of the two tests.

  strict_sha256, strict_n   SHA-256 of the float64 outputs (little-endian bytes) of the strict build
                            (libfastexp_ref.so) on the 500k inputs of the bit-for-bit test: equal bits, equal digest
  fast_math_y               the outputs of the build with the reference's flags (libfastexp_ref_fm.so,
                            -O3 -ffast-math) on the 50k inputs of the flag-noise test

    python tests/golden/make_fastexp_pins.py      ->  tests/golden/fastexp_pins.npz

Needs oracle/_ref (built from the reference tree); the fixture it writes does not."""
import ctypes as C
import hashlib
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parents[1]))
sys.path.insert(0, str(HERE.parent))


def main():
    from oracle import nfo
    from test_oracle_pin import bit_for_bit_inputs, flag_noise_inputs
    strict, fm = nfo.ref_fastexp_lib(), nfo.ref_fastexp_lib(fast_math=True)
    if strict is None or fm is None:
        raise SystemExit('oracle/_ref is not built: the reference tree is needed to make this fixture')
    x = bit_for_bit_inputs()
    y = np.array([strict.FastExp(C.c_float(float(v))) for v in x], dtype='<f8')
    xf = flag_noise_inputs()
    yf = np.array([fm.FastExp(C.c_float(float(v))) for v in xf], dtype=np.float64)
    out = HERE / 'fastexp_pins.npz'
    np.savez_compressed(out, strict_sha256=np.array(hashlib.sha256(y.tobytes()).hexdigest()), strict_n=np.array(x.size),
                        fast_math_y=yf)
    print(out, x.size, 'strict outputs,', xf.size, 'fast-math outputs')


if __name__ == '__main__':
    main()
