"""Device time-stretch without a codec handle (fishrt.h fs_time_stretch / fs_time_stretch_out_len): WSOLA with a squared-difference measure,
frame 1024, hop 512, search radius 512 unless frame= / radius= say otherwise.  speed > 1 is faster (fewer samples), the pitch stays."""
import ctypes as C

import numpy as np

from . import _ffi

FRAME, RADIUS = 1024, 512  # the defaults of the definition


def time_stretch_out_len(n, speed):
    """samples that n input samples become at `speed` (0.25 .. 4.0): floor(n / speed + 0.5)"""
    out = C.c_int64(0)
    _ffi.check(_ffi.lib().fs_time_stretch_out_len(int(n), C.c_double(float(speed)), C.byref(out)))
    return int(out.value)


def time_stretch(pcm, speed, return_positions=False, lengths=None, frame=None, radius=None, device=0):
    """pcm f32 (n,) -> (out_len,), or (b, n) -> (b, out_len); with lengths (one sample count <= n per row, 0 allowed) -> a list of b arrays,
    every row stretched on its own in one call.  return_positions: also the frame positions p_k, int64 -- (K,), (b, K) or a list of b arrays
    -- the hook the tests referee through.  frame / radius: N and D of the definition (None: the defaults)."""
    params = None
    if frame is not None or radius is not None:
        params = _ffi.TsmParams(FRAME if frame is None else int(frame), RADIUS if radius is None else int(radius))
    hs = (FRAME if frame is None else int(frame)) // 2
    x = np.ascontiguousarray(pcm, np.float32)
    one = x.ndim == 1
    if one:
        x = x.reshape(1, -1)
    if x.ndim != 2:
        raise ValueError("time_stretch: pcm must have shape (n,) or (b, n)")
    b, n = x.shape
    ns = np.array([n] * b if lengths is None else [int(v) for v in lengths], np.int64)
    if ns.shape != (b,) or (ns < 0).any() or (ns > n).any():
        raise ValueError("lengths must hold one sample count in [0, n] per row")
    if one and lengths is not None:
        raise ValueError("lengths go with a (b, n) array")
    stride = max(1, max(time_stretch_out_len(int(v), speed) for v in ns))
    out = np.zeros((b, stride), np.float32)
    got = (C.c_int64 * b)()
    pstride = max(1, -(-stride // max(hs, 1)))
    pos = np.zeros((b, pstride), np.int64) if return_positions else None
    if n == 0:
        x = np.zeros((b, 1), np.float32)
    _ffi.check(_ffi.lib().fs_time_stretch(int(device), x.ctypes.data_as(C.POINTER(C.c_float)), int(b), C.c_size_t(x.shape[1]),
                                          ns.ctypes.data_as(C.POINTER(C.c_int64)), C.c_double(float(speed)),
                                          C.byref(params) if params is not None else None, out.ctypes.data_as(C.POINTER(C.c_float)),
                                          C.c_size_t(stride), got, pos.ctypes.data_as(C.POINTER(C.c_int64)) if return_positions else None,
                                          C.c_size_t(pstride)))
    frames = [-(-int(got[i]) // hs) for i in range(b)]
    if lengths is not None:
        ys = [out[i, : got[i]].copy() for i in range(b)]
        return (ys, [pos[i, : frames[i]].copy() for i in range(b)]) if return_positions else ys
    assert all(got[i] == got[0] for i in range(b))
    y = out[:, : got[0]]
    y = y[0].copy() if one else np.ascontiguousarray(y)
    if not return_positions:
        return y
    p = pos[:, : frames[0]]
    return y, (p[0].copy() if one else np.ascontiguousarray(p))


def time_stretch_chunks(pcm, chunk_lens, speed, frame=None, radius=None, device=0):
    """the test hook of the chunked stretch (fishrt.h fs_selftest_tsm_chunks): pcm f32 (n,) cut into consecutive chunks of chunk_lens samples
    (they add up to n; the last one is the final item and may be 0), one plan step and one launch pair per chunk, the state a speed stream
    keeps carried between them -> (y f32 (out_len,), emitted int64 (len(chunk_lens),), positions int64 (K,))"""
    params = None
    if frame is not None or radius is not None:
        params = _ffi.TsmParams(FRAME if frame is None else int(frame), RADIUS if radius is None else int(radius))
    hs = (FRAME if frame is None else int(frame)) // 2
    x = np.ascontiguousarray(pcm, np.float32).reshape(-1)
    lens = np.ascontiguousarray(np.asarray(chunk_lens, np.int64).reshape(-1))
    cap = max(1, time_stretch_out_len(x.shape[0], speed))
    pcap = max(1, -(-cap // max(hs, 1)))
    out, emitted, pos = np.zeros(cap, np.float32), np.zeros(max(1, lens.shape[0]), np.int64), np.zeros(pcap, np.int64)
    n_out, n_pos = C.c_int64(0), C.c_int64(0)
    xs = x if x.shape[0] else np.zeros(1, np.float32)
    _ffi.check(_ffi.lib().fs_selftest_tsm_chunks(int(device), xs.ctypes.data_as(C.POINTER(C.c_float)), C.c_int64(x.shape[0]),
                                                 lens.ctypes.data_as(C.POINTER(C.c_int64)), int(lens.shape[0]), C.c_double(float(speed)),
                                                 C.byref(params) if params is not None else None, out.ctypes.data_as(C.POINTER(C.c_float)),
                                                 C.c_size_t(cap), C.byref(n_out), emitted.ctypes.data_as(C.POINTER(C.c_int64)),
                                                 pos.ctypes.data_as(C.POINTER(C.c_int64)), C.c_size_t(pcap), C.byref(n_pos)))
    return out[: n_out.value].copy(), emitted[: lens.shape[0]].copy(), pos[: n_pos.value].copy()
