"""Device buffers for the tests of the device-pointer entry points (nfa_runner_loglike_batch_dev,
nfa_runner_predict_batch_dev): plain arrays (DeviceArrays), and the arrays of several batches inside ONE allocation
between guard bands of a sentinel (GuardedArrays), so that a kernel that reads or writes past its batch stays inside
the test's own memory and is seen: the bands must come back bit for bit unchanged."""
import ctypes as C

import numpy as np


class DeviceArrays:
    def __init__(self, lib, check):
        self.lib, self.check, self.ptrs = lib, check, []

    def upload(self, a):
        a = np.ascontiguousarray(a)
        p = C.c_void_p()
        self.check(self.lib.nfa_malloc(C.byref(p), a.nbytes))
        self.check(self.lib.nfa_memcpy_h2d(p, a.ctypes.data_as(C.c_void_p), a.nbytes))
        self.ptrs.append(p)
        return p

    def empty(self, nbytes):
        p = C.c_void_p()
        self.check(self.lib.nfa_malloc(C.byref(p), nbytes))
        self.ptrs.append(p)
        return p

    def download(self, p, like):
        out = np.empty_like(like)
        self.check(self.lib.nfa_memcpy_d2h(out.ctypes.data_as(C.c_void_p), p, out.nbytes))
        return out

    def free(self):
        for p in self.ptrs:
            self.lib.nfa_free(p)
        self.ptrs = []


class GuardedArrays:
    """`n` arrays of shape `shape` (rows first) and type `dtype` in one device allocation laid out as
    [guard][array 0][guard][array 1] ... [array n-1][guard], every guard `guard` rows of `sentinel`."""

    def __init__(self, dev, n, shape, dtype, sentinel, guard=64):
        self.dev, self.n, self.guard = dev, n, guard
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.row_bytes = int(np.prod(self.shape[1:], dtype=np.int64)) * self.dtype.itemsize
        self.stride = (self.shape[0] + guard) * self.row_bytes            # from one array to the next
        self.band = np.full((guard,) + self.shape[1:], sentinel, dtype=self.dtype)
        self.base = dev.empty(n * self.stride + guard * self.row_bytes)
        for k in range(n + 1):
            self._put(self._band_offset(k), self.band)

    def _band_offset(self, k):
        return k * self.stride

    def _put(self, offset, a):
        a = np.ascontiguousarray(a, dtype=self.dtype)
        self.dev.check(self.dev.lib.nfa_memcpy_h2d(C.c_void_p(self.base.value + offset), a.ctypes.data_as(C.c_void_p), a.nbytes))

    def _get(self, offset, shape):
        out = np.empty(shape, dtype=self.dtype)
        self.dev.check(self.dev.lib.nfa_memcpy_d2h(out.ctypes.data_as(C.c_void_p), C.c_void_p(self.base.value + offset), out.nbytes))
        return out

    def ptr(self, k):
        assert 0 <= k < self.n
        return C.c_void_p(self.base.value + self._band_offset(k) + self.guard * self.row_bytes)

    def put(self, k, a):
        assert a.shape == self.shape, (a.shape, self.shape)
        self._put(self._band_offset(k) + self.guard * self.row_bytes, a)

    def get(self, k):
        return self._get(self._band_offset(k) + self.guard * self.row_bytes, self.shape)

    def bands_intact(self):
        """Whether every guard band still holds its sentinel, bit for bit (NaN sentinels included)."""
        want = self.band.view(np.uint8)
        return all(np.array_equal(self._get(self._band_offset(k), self.band.shape).view(np.uint8), want)
                   for k in range(self.n + 1))
