"""Device sample-rate conversion without a codec handle (fishrt.h fs_resample / fs_resample_out_len): "linear" is the reference's
audio/functional.rs::resample bit for bit, "sinc" a Hann-windowed sinc polyphase filter (W = 6, rolloff 0.99); dtype "s16" fuses
wav.pcm_to_i16 into the kernel's store."""
import ctypes as C

import numpy as np

from . import _ffi


def resample_out_len(n, from_rate, to_rate, mode="linear"):
    """samples that n input samples become"""
    if mode not in _ffi.RESAMPLE_MODES:
        raise ValueError(f"resample mode must be one of {sorted(_ffi.RESAMPLE_MODES)}")
    out = C.c_int64(0)
    _ffi.check(_ffi.lib().fs_resample_out_len(int(from_rate), int(to_rate), _ffi.RESAMPLE_MODES[mode], int(n), C.byref(out)))
    return int(out.value)


def resample(pcm, from_rate, to_rate, mode="linear", dtype="f32", lengths=None, device=0):
    """pcm f32 (n,) -> (out_len,), or (b, n) -> (b, out_len); with lengths (one sample count <= n per row, 0 allowed) -> a list of b arrays,
    every row converted on its own in one launch.  Rows are independent: no row reads another row's samples."""
    spec = _ffi.pcm_spec(to_rate, mode, dtype)
    x = np.ascontiguousarray(pcm, np.float32)
    one = x.ndim == 1
    if one:
        x = x.reshape(1, -1)
    if x.ndim != 2:
        raise ValueError("resample: pcm must have shape (n,) or (b, n)")
    b, n = x.shape
    ns = np.array([n] * b if lengths is None else [int(v) for v in lengths], np.int64)
    if ns.shape != (b,) or (ns < 0).any() or (ns > n).any():
        raise ValueError("lengths must hold one sample count in [0, n] per row")
    if one and lengths is not None:
        raise ValueError("lengths go with a (b, n) array")
    stride = max(1, max(resample_out_len(int(v), from_rate, to_rate, mode) for v in ns))
    out = np.zeros((b, stride), _ffi.PCM_DTYPES[dtype])
    got = (C.c_int64 * b)()
    if n == 0:
        x = np.zeros((b, 1), np.float32)
    _ffi.check(_ffi.lib().fs_resample(int(device), x.ctypes.data_as(C.POINTER(C.c_float)), int(b), C.c_size_t(x.shape[1]),
                                      ns.ctypes.data_as(C.POINTER(C.c_int64)), int(from_rate), C.byref(spec), out.ctypes.data_as(C.c_void_p),
                                      C.c_size_t(stride), got))
    if lengths is not None:
        return [out[i, : got[i]].copy() for i in range(b)]
    assert all(got[i] == got[0] for i in range(b))
    out = out[:, : got[0]]
    return out[0].copy() if one else np.ascontiguousarray(out)
