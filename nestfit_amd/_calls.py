"""What the one-pixel runners (`_model.EngineRunner`) and `cube.CubeRunner` do alike before and around an engine call: the
checks of their array arguments, each written once with its message, and the three chunked host calls of a runner handle."""
import numpy as np

from . import _ffi
from .core import _as_inplace_matrix


def shape_error(runner, got):
    """The ValueError of parameters that are not `runner.ndim` wide; `got`: the shape, or the length, as the caller words it."""
    return ValueError(f'Invalid shape for ncomp={runner.ncomp}: {got}')


def parameter_rows(runner, theta):
    """Physical parameter rows theta[B, ndim] as a contiguous float64 array."""
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    if theta.ndim != 2 or theta.shape[1] != runner.ndim:
        raise shape_error(runner, theta.shape)
    return theta


def unit_rows(runner, U):
    """Unit-cube rows U[B, ndim] that the engine overwrites: the caller's own array, never a copy."""
    U = _as_inplace_matrix(U)
    if U.shape[1] != runner.ndim:
        raise shape_error(runner, U.shape[1])
    return U


def pixel_indices(pix, n, per='row'):
    """pix[n] as a contiguous int32 array: one pixel index per row of parameters, or per segment of rows."""
    pix = np.ascontiguousarray(pix, dtype=np.int32)
    if pix.shape != (n,):
        raise ValueError(f'one pixel index per {per} is required')
    return pix


def out_array(out, shape, what):
    """The caller's `out`, a contiguous float64 array of `shape` (in the message: `what`), or a new one for None."""
    out = np.empty(shape) if out is None else out
    if out.shape != shape or out.dtype != np.float64 or not out.flags.c_contiguous:
        raise ValueError(f'out must be a contiguous float64 array {what}')
    return out


def _sample_posterior(runner, pix, **kw):
    """`ensemble.sample_pixels` of a runner's pixels (pix: None for the pixel of a one-pixel runner): the ensemble sampler's
    arguments are checked once, by the engine -- the ladder `betas=` of a tempered ensemble among them."""
    from .ensemble import sample_pixels
    return sample_pixels(runner, pix, **kw)


def _row_statistics(handle, pix, theta, n_spec):
    """nfa_runner_row_statistics on checked arrays (pix: int32[B] or None)."""
    B = theta.shape[0]
    peak, total = np.empty((B, n_spec)), np.empty((B, n_spec))
    _ffi.check(_ffi.load().nfa_runner_row_statistics(handle, None if pix is None else pix.ctypes.data_as(_ffi._ip),
                                                     _ffi.dptr(theta), B, _ffi.dptr(peak), _ffi.dptr(total)))
    return peak, total


def _normal_equations(handle, pix, theta, step, lower, upper, chunk_rows, want_curvature, want_grad=True):
    """nfa_runner_normal_equations on checked points (pix: int32[B] or None; theta: float64[B, ndim]) -> `NormalEquations`."""
    from .lsq import NormalEquations
    B, ndim = theta.shape

    def vector(a, name):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.shape != (ndim,):
            raise ValueError(f'{name} must hold one value per parameter')
        return a
    step, lower, upper = vector(step, 'step'), vector(lower, 'lower'), vector(upper, 'upper')
    chi2 = np.empty(B)
    grad = np.empty((B, ndim)) if want_grad else None
    curv = np.empty((B, ndim, ndim)) if want_curvature else None
    opt = lambda a: None if a is None else _ffi.dptr(a)
    _ffi.check(_ffi.load().nfa_runner_normal_equations(
        handle, None if pix is None else pix.ctypes.data_as(_ffi._ip), _ffi.dptr(theta), B, opt(step), opt(lower), opt(upper),
        0 if chunk_rows is None else int(chunk_rows), _ffi.dptr(chi2), opt(grad), opt(curv)))
    return NormalEquations(chi2, grad, curv)


def _predict_moments(handle, pix, offsets, theta, weights, chunk_rows, want_spectra, n_chan_tot, n_spec):
    """nfa_runner_predict_moments on checked arrays (pix: int32[n_seg] or None) -> `PosteriorMoments`."""
    from .moments import PosteriorMoments
    n_seg = offsets.size - 1
    if weights is not None:
        weights = np.ascontiguousarray(weights, dtype=np.float64)
        if weights.shape != (theta.shape[0],):
            raise ValueError('one weight per row is required')
    mean = np.empty((n_seg, n_chan_tot)) if want_spectra else None
    std = np.empty((n_seg, n_chan_tot)) if want_spectra else None
    smean, sstd = np.empty((n_seg, n_spec, 2)), np.empty((n_seg, n_spec, 2))
    opt = lambda a: None if a is None else _ffi.dptr(a)
    _ffi.check(_ffi.load().nfa_runner_predict_moments(
        handle, n_seg, None if pix is None else pix.ctypes.data_as(_ffi._ip), offsets.ctypes.data_as(_ffi._lp),
        _ffi.dptr(theta), opt(weights), 0 if chunk_rows is None else int(chunk_rows), opt(mean), opt(std),
        _ffi.dptr(smean), _ffi.dptr(sstd)))
    return PosteriorMoments(mean, std, smean[:, :, 0].copy(), sstd[:, :, 0].copy(), smean[:, :, 1].copy(), sstd[:, :, 1].copy())
