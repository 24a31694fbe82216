"""The seven creators of include/nestfit_amd.h on the device.  Each fills one declaration record and specset_build
(nfa_engine.hip) makes the set: csrc/nfa_set_decl.h checks and derives on the host, the base arrays go up, and
specset_realise forms the rest as it does for every other state of a set.

test_the_library_refuses_what_the_header_refuses: the refusal table of tests/test_set_decl_cpu.py through the real entry
points -- the same code and message, *out untouched, and a valid creation afterwards.
test_a_constant_channel_noise_is_the_scalar_set: for every creator, a noise per channel that is one constant per (pixel,
spectrum) gives the scalar set's spectra, lnL and null_lnZ to the bit (the contract of nfa_specset_create_channel_noise, which
tests/test_channel_noise.py holds for ammonia), for one and two components in both numerical modes.
test_a_failed_allocation_creates_no_set: the test library's option "fail_alloc" fails each allocation that creation routes
through set_alloc, the two of a noise per channel.  Host side only: no kernel runs on memory that is not there.
Shapes: two pixels, two spectra of 64 and 130 channels (130 crosses a row of 64), up to three transitions in a spectrum, two
species, 16 parameter rows.  Nothing here is a tolerance."""
import ctypes as C

import numpy as np
import pytest

import set_decl_cases as sd
from test_set_decl_cpu import REFUSALS
from test_sibling_models import MODES, mode_guard          # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu

SENTINEL = 0x5e7dec1
OOM = 'out of device memory for the channel weights'


def _bytes(result):
    return tuple(a.tobytes() for a in result)


def test_the_library_refuses_what_the_header_refuses(engine):
    from nestfit_amd import _ffi
    lib = _ffi.engine()
    valid = {}
    for _, d in sd.VALID:
        valid.setdefault(d['entry'], d)
    assert len(valid) == 8 and len(REFUSALS) > 600
    for label, d, code, message in REFUSALS:
        h = C.c_void_p(SENTINEL)
        rc, msg, _ = sd.call_creator(lib, d, handle=h)
        assert (rc, msg) == (code, message), label
        assert h.value == SENTINEL, label
        rc, msg, h = sd.call_creator(lib, valid[d['entry']])
        assert rc == 0 and h.value not in (None, SENTINEL), (label, msg)
        assert lib.nfa_specset_destroy(h) == 0


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', sd.NAMES)
def test_a_constant_channel_noise_is_the_scalar_set(engine, name, mode, mode_guard):
    from nestfit_amd import _ffi
    lib = _ffi.engine()
    engine.set_exp_mode(mode)
    scalar = sd.full(name, lib)
    channel = sd.per_channel(scalar)
    assert channel['noise'] is None and channel['chan_noise'].shape == scalar['data'].shape
    for ncomp in (1, 2):
        want = sd.evaluate(lib, scalar, name, ncomp)
        assert np.isfinite(want[1]).all() and np.isfinite(want[2]).all() and np.abs(want[0]).max() > 1e-3, (name, ncomp)
        assert _bytes(sd.evaluate(lib, channel, name, ncomp)) == _bytes(want), (name, ncomp)


@pytest.fixture
def test_lib():
    from nestfit_amd import _ffi
    lib = _ffi.test_engine()
    try:
        yield lib
    finally:
        lib.nfa_set_option(b'fail_alloc', 0)


@pytest.mark.parametrize('name', sd.NAMES)
def test_a_failed_allocation_creates_no_set(engine, test_lib, name):
    lib = test_lib
    scalar = sd.full(name, lib)
    channel = sd.per_channel(scalar, masked=True)
    before = _bytes(sd.evaluate(lib, channel, name, 2)), _bytes(sd.evaluate(lib, scalar, name, 2))      # the hook untouched
    n_alloc = 2                                                 # SB_W and SB_WDATA: set_layout of the empty record on a noise per channel
    for k in range(1, n_alloc + 1):
        assert lib.nfa_set_option(b'fail_alloc', k) == 0
        h = C.c_void_p(SENTINEL)
        rc, msg, _ = sd.call_creator(lib, channel, handle=h)
        assert (rc, msg, h.value) == (2, OOM, SENTINEL), (name, k)                                    # NFA_ERR_DEVICE, and no set
        assert _bytes(sd.evaluate(lib, channel, name, 2)) == before[0], (name, k)                      # the same call, unarmed
    assert lib.nfa_set_option(b'fail_alloc', n_alloc + 1) == 0                                         # one beyond: it never fires
    assert _bytes(sd.evaluate(lib, channel, name, 2)) == before[0]
    assert lib.nfa_set_option(b'fail_alloc', 1) == 0                                                   # a scalar noise allocates none of them
    assert _bytes(sd.evaluate(lib, scalar, name, 2)) == before[1]
    assert lib.nfa_set_option(b'fail_alloc', 0) == 0
