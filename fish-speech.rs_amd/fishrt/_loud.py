"""Device loudness measurement and normalisation without a codec handle (fishrt.h fs_loudness_normalize): the integrated loudness of
ITU-R BS.1770-4 for one channel at 8 .. 48 kHz (K-weighting, 400 ms blocks every 100 ms, absolute gate at -70 LUFS, relative gate 10 LU
under the gated mean), the sample peak, and one gain per row: min(what reaches the target, max_gain_db, what keeps the peak at peak_db)."""
import ctypes as C

import numpy as np

from . import _ffi

PEAK_DB, MAX_GAIN_DB = -1.0, 30.0  # the defaults of the definition


def _record(r):
    return dict(lufs=float(r.lufs), peak=float(np.float32(r.peak)), gain=float(np.float32(r.gain)), blocks_total=int(r.blocks_total),
                blocks_kept=int(r.blocks_kept))


def _rows(pcm, lengths, what):
    x = np.ascontiguousarray(pcm, np.float32)
    one = x.ndim == 1
    if one:
        x = x.reshape(1, -1)
    if x.ndim != 2:
        raise ValueError(f"{what}: pcm must have shape (n,) or (b, n)")
    b, n = x.shape
    if one and lengths is not None:
        raise ValueError("lengths go with a (b, n) array")
    ns = np.array([n] * b if lengths is None else [int(v) for v in lengths], np.int64)
    if ns.shape != (b,) or (ns < 0).any() or (ns > n).any():
        raise ValueError("lengths must hold one sample count in [0, n] per row")
    if n == 0:
        x = np.zeros((b, 1), np.float32)
    return x, one, b, ns


def _call(x, b, ns, rate, device, params, out):
    res = (_ffi.LoudResult * b)()
    _ffi.check(_ffi.lib().fs_loudness_normalize(int(device), x.ctypes.data_as(C.POINTER(C.c_float)), int(b),
                                                C.c_size_t(x.shape[1]), ns.ctypes.data_as(C.POINTER(C.c_int64)), int(rate),
                                                C.byref(params) if params is not None else None,
                                                out.ctypes.data_as(C.POINTER(C.c_float)) if out is not None else None,
                                                C.c_size_t(out.shape[1] if out is not None else 0), res))
    return [_record(r) for r in res]


def loudness(pcm, rate, lengths=None, device=0, details=False):
    """pcm f32 (n,) -> LUFS, or (b, n) -> a list of b values (lengths: one sample count <= n per row, every row measured on its own in one
    call).  -inf for a row without loudness (under 400 ms, or nothing above the gates).  details: the whole record per row instead --
    dict(lufs, peak, gain = 1, blocks_total, blocks_kept)."""
    x, one, b, ns = _rows(pcm, lengths, "loudness")
    recs = _call(x, b, ns, rate, device, None, None)
    vals = recs if details else [r["lufs"] for r in recs]
    return vals[0] if one else vals


def loudness_normalize(pcm, rate, target, peak_db=PEAK_DB, max_gain_db=MAX_GAIN_DB, lengths=None, device=0, return_info=False):
    """pcm f32 (n,) -> (n,), or (b, n) -> (b, n); with lengths -> a list of b arrays.  Every row is multiplied by its own gain.  target: LUFS
    in -40 .. -5; peak_db <= 0: the gain never lifts the sample peak above it; max_gain_db in 0 .. 60.  return_info: also the record(s)
    dict(lufs, peak, gain, blocks_total, blocks_kept) -- lufs is the loudness MEASURED, before the gain."""
    x, one, b, ns = _rows(pcm, lengths, "loudness_normalize")
    params = _ffi.LoudParams(float(target), float(peak_db), float(max_gain_db))
    out = np.zeros_like(x)
    recs = _call(x, b, ns, rate, device, params, out)
    if lengths is not None:
        y = [out[i, : ns[i]].copy() for i in range(b)]
    else:
        y = out[:, : ns[0]]
        y = y[0].copy() if one else np.ascontiguousarray(y)
    if not return_info:
        return y
    return y, (recs[0] if one else recs)
