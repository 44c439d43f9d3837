"""fish_speech_python `FireflyCodec` (codec.rs:18-115) over the C ABI: decode(u32[b,8,T]) -> f32[b,1,2048*T], encode(f32[1,1,n]) -> u32[1,8,L]."""
import ctypes as C

import numpy as np

from . import _ffi


class FireflyCodec:
    PRECISIONS = {"f32": 0, "bf16x3": 1, "f16": 2}

    def __init__(self, device=0, channel_div=1, precision="f16"):
        """precision: arithmetic of the decode path's convs -- "f16" (default: single f16 operands on the matrix cores, f32 accumulation
        and f32 residual stream; PCM 1.6e-5 RMS from the f32 reference at signal rms 0.031, bound 1e-4), "bf16x3" (split-bf16 matrix
        products, 3e-7 RMS) or "f32" (exact f32 products); the encoder always runs exact f32 (fishrt.h: fs_codec_set_precision)"""
        h = C.c_void_p()
        _ffi.check(_ffi.lib().fs_codec_create(int(device), int(channel_div), C.byref(h)))
        self._h = h
        _ffi.check(_ffi.lib().fs_codec_set_precision(self._h, self.PRECISIONS[precision]))
        self.precision = precision

    def _dtypes(self):
        """stream id -> "f32" | "s16" of the streams opened with a PCM spec"""
        return self.__dict__.setdefault("_stream_dtype", {})

    def close(self):
        if getattr(self, "_h", None) and _ffi is not None and getattr(_ffi, "lib", None):  # (module globals are gone at interpreter exit)
            _ffi.lib().fs_codec_destroy(self._h)
            self._h = None

    __del__ = close

    def load_synthetic(self, seed):
        _ffi.check(_ffi.lib().fs_codec_load_synthetic(self._h, C.c_uint64(seed)))
        return self

    def load_safetensors(self, path):
        _ffi.check(_ffi.lib().fs_codec_load_safetensors(self._h, str(path).encode()))
        return self

    @property
    def sample_rate(self):
        return _ffi.lib().fs_codec_sample_rate(self._h)

    def _spec(self, sample_rate, resample, dtype):
        """None when the arguments ask for what the plain calls return (codec rate, f32), else the fs_pcm_spec"""
        if sample_rate is None and dtype == "f32":
            return None
        return _ffi.pcm_spec(self.sample_rate if sample_rate is None else sample_rate, resample, dtype)

    last_loudness = None  # the per-row records of the last decode(loudness=) call

    def decode(self, codes, sample_rate=None, resample="linear", dtype="f32", speed=None, loudness=None, peak_db=None, max_gain_db=None):
        """sample_rate / dtype: convert every PCM row on the device before it is copied to the host (fishrt.h fs_codec_decode_pcm) ->
        (b, 1, out_len) f32 or int16; resample: "linear" (the reference's resample, bit for bit) or "sinc" (band-limited).
        speed (0.25 .. 4.0; None = no stretch stage): every row time-stretched on the device first (fishrt.h fs_codec_decode_speed: WSOLA,
        the pitch stays) -- 2048 T / speed samples per row, before sample_rate / dtype apply.
        loudness (LUFS, -40 .. -5; None = no loudness stage): every row measured (BS.1770 integrated loudness) and multiplied by its own gain
        on the device, in front of the stretch stage (fishrt.h fs_codec_decode_loud); peak_db (default -1) bounds the sample peak the gain may
        produce, max_gain_db (default 30) the gain.  Returns what it returns without; the rows' records -- dict(lufs, peak, gain,
        blocks_total, blocks_kept), lufs as measured before the gain -- are in self.last_loudness"""
        if not isinstance(codes, np.ndarray) or not codes.flags["C_CONTIGUOUS"]:
            raise ValueError("Input array must be contiguous")  # codec.rs:97-101
        if codes.ndim != 3 or codes.shape[1] != 8:
            raise ValueError("codes must have shape (b, 8, T)")
        codes = codes.astype(np.uint32, copy=False)
        b, _, T = codes.shape
        if loudness is not None:
            from . import _loud
            from ._resample import resample_out_len
            from ._tsm import time_stretch_out_len
            spec = _ffi.pcm_spec(self.sample_rate if sample_rate is None else sample_rate, resample, dtype)
            params = _ffi.LoudParams(float(loudness), _loud.PEAK_DB if peak_db is None else float(peak_db),
                                     _loud.MAX_GAIN_DB if max_gain_db is None else float(max_gain_db))
            speed = 1.0 if speed is None else float(speed)
            n = time_stretch_out_len(2048 * T, speed) if speed != 1.0 else 2048 * T  # (refuses a speed outside 0.25 .. 4.0)
            if spec.rate != self.sample_rate:
                n = resample_out_len(n, self.sample_rate, spec.rate, resample)
            out = np.empty((b, 1, max(n, 1)), _ffi.PCM_DTYPES[dtype])
            got, res = (C.c_int64 * b)(), (_ffi.LoudResult * b)()
            _ffi.check(_ffi.lib().fs_codec_decode_loud(self._h, codes.ctypes.data_as(C.POINTER(C.c_uint32)), b, T, C.byref(params),
                                                       C.c_double(speed), C.byref(spec), out.ctypes.data_as(C.c_void_p),
                                                       C.c_size_t(out.shape[2]), got, res))
            assert all(got[i] == n for i in range(b))
            self.last_loudness = [_loud._record(r) for r in res]
            return out[:, :, :n]
        if peak_db is not None or max_gain_db is not None:
            raise ValueError("peak_db / max_gain_db go with loudness=")
        if speed is not None:
            from ._resample import resample_out_len
            from ._tsm import time_stretch_out_len
            spec = _ffi.pcm_spec(self.sample_rate if sample_rate is None else sample_rate, resample, dtype)
            n = time_stretch_out_len(2048 * T, speed)  # (refuses a speed outside 0.25 .. 4.0)
            if spec.rate != self.sample_rate:
                n = resample_out_len(n, self.sample_rate, spec.rate, resample)
            out = np.empty((b, 1, max(n, 1)), _ffi.PCM_DTYPES[dtype])
            got = (C.c_int64 * b)()
            _ffi.check(_ffi.lib().fs_codec_decode_speed(self._h, codes.ctypes.data_as(C.POINTER(C.c_uint32)), b, T, C.c_double(float(speed)),
                                                        C.byref(spec), out.ctypes.data_as(C.c_void_p), C.c_size_t(out.shape[2]), got))
            assert all(got[i] == n for i in range(b))
            return out[:, :, :n]
        spec = self._spec(sample_rate, resample, dtype)
        if spec is not None:
            from ._resample import resample_out_len
            n = resample_out_len(2048 * T, self.sample_rate, spec.rate, resample) if spec.rate != self.sample_rate else 2048 * T
            out = np.empty((b, 1, max(n, 1)), _ffi.PCM_DTYPES[dtype])
            got = (C.c_int64 * b)()
            _ffi.check(_ffi.lib().fs_codec_decode_pcm(self._h, codes.ctypes.data_as(C.POINTER(C.c_uint32)), b, T, C.byref(spec),
                                                      out.ctypes.data_as(C.c_void_p), C.c_size_t(out.shape[2]), got))
            assert all(got[i] == n for i in range(b))
            return out[:, :, :n]
        pcm = np.empty((b, 1, 2048 * T), np.float32)
        _ffi.check(_ffi.lib().fs_codec_decode(self._h, codes.ctypes.data_as(C.POINTER(C.c_uint32)), b, T,
                                              pcm.ctypes.data_as(C.POINTER(C.c_float))))
        return pcm

    # ---- f16 range guard (fishrt.h fs_codec_set_range_check / fs_codec_range_stats): diagnostic for validating a new checkpoint
    def set_range_check(self, on=True):
        _ffi.check(_ffi.lib().fs_codec_set_range_check(self._h, 1 if on else 0))
        return self

    def range_stats(self):
        out, rms = (C.c_uint64 * 5)(), C.c_double(0.0)
        _ffi.check(_ffi.lib().fs_codec_range_stats(self._h, out, C.byref(rms)))
        return dict(act_saturated=int(out[0]), act_flushed=int(out[1]), weights_saturated=int(out[2]), weights_flushed=int(out[3]),
                    fallbacks=int(out[4]), last_pcm_rms_diff=float(rms.value))

    # ---- stateful streaming (fishrt.h fs_codec_stream_*): chunks of ONE code sequence, left context kept on the device
    STREAM_MIN_FRAMES = 16

    def stream_begin(self):
        _ffi.check(_ffi.lib().fs_codec_stream_begin(self._h))
        return self

    def stream_decode(self, codes):
        """codes u32 (8, T) or (1, 8, T), T >= 16: the next chunk of the stream -> f32 (2048 T,) PCM.  Concatenated over a stream the result
        is bit-identical to decode() of the whole sequence; no frame is decoded twice."""
        codes = np.ascontiguousarray(codes, np.uint32)
        if codes.ndim == 3 and codes.shape[0] == 1:
            codes = codes[0]
        if codes.ndim != 2 or codes.shape[0] != 8:
            raise ValueError("a streamed chunk must have shape (8, T)")
        T = codes.shape[1]
        pcm = np.empty(2048 * T, np.float32)
        _ffi.check(_ffi.lib().fs_codec_stream_decode(self._h, codes.ctypes.data_as(C.POINTER(C.c_uint32)), T, pcm.ctypes.data_as(C.POINTER(C.c_float))))
        return pcm

    def stream_end(self):
        _ffi.check(_ffi.lib().fs_codec_stream_end(self._h))

    # ---- many concurrent streams on one handle (fishrt.h fs_codec_streams_*): one launch sequence advances n streams by T frames each
    STREAMS_MAX = 64

    def streams_open(self, sample_rate=None, resample="linear", dtype="f32", speed=None):
        """-> stream id: a new stream from zero left context, in the handle's current precision mode.  sample_rate / dtype: its PCM leaves
        converted on the device (fishrt.h fs_codec_streams_open_pcm); such a stream is decoded by streams_decode_ragged only.
        speed (0.25 .. 4.0; None = no stretch stage): its PCM is time-stretched on the device first, chunk by chunk (fishrt.h
        fs_codec_streams_open_speed), before sample_rate / dtype apply; decoded by streams_decode_ragged only, with a final flag on its last
        item.  Its pieces concatenated equal decode(..., speed=) of the whole sequence bit for bit."""
        sid = C.c_int(-1)
        spec = self._spec(sample_rate, resample, dtype)
        if speed is not None:
            _ffi.check(_ffi.lib().fs_codec_streams_open_speed(self._h, C.c_double(float(speed)), C.byref(spec) if spec is not None else None,
                                                              C.byref(sid)))
        elif spec is None:
            _ffi.check(_ffi.lib().fs_codec_streams_open(self._h, C.byref(sid)))
        else:
            _ffi.check(_ffi.lib().fs_codec_streams_open_pcm(self._h, C.byref(spec), C.byref(sid)))
        self._dtypes().pop(int(sid.value), None)
        if spec is not None or speed is not None:  # (a speed stream goes through fs_codec_streams_decode_pcm whatever its dtype)
            self._dtypes()[int(sid.value)] = dtype
        return int(sid.value)

    def streams_close(self, stream_id):
        _ffi.check(_ffi.lib().fs_codec_streams_close(self._h, int(stream_id)))
        self._dtypes().pop(int(stream_id), None)

    def streams_pending(self, stream_id, T, final=False):
        """samples the next streams_decode_ragged item of T frames (final or not) would emit for this stream"""
        n = C.c_int64(0)
        _ffi.check(_ffi.lib().fs_codec_streams_pending(self._h, int(stream_id), int(T), 1 if final else 0, C.byref(n)))
        return int(n.value)

    def streams_decode(self, ids, codes):
        """ids: n distinct open stream ids; codes u32 (n, 8, T), T >= 16: item i is the next chunk of stream ids[i] -> f32 (n, 2048 T) PCM.
        Per stream, the chunks' PCM concatenated is bit-identical to decode() of its whole sequence."""
        ids = np.ascontiguousarray(np.asarray(ids, np.int32).reshape(-1))
        codes = np.ascontiguousarray(codes, np.uint32)
        if codes.ndim != 3 or codes.shape[1] != 8 or codes.shape[0] != ids.shape[0]:
            raise ValueError("streams_decode: codes must have shape (n, 8, T) with one item per stream id")
        n, _, T = codes.shape
        pcm = np.empty((n, 2048 * T), np.float32)
        _ffi.check(_ffi.lib().fs_codec_streams_decode(self._h, int(n), ids.ctypes.data_as(C.POINTER(C.c_int)),
                                                      codes.ctypes.data_as(C.POINTER(C.c_uint32)), int(T),
                                                      pcm.ctypes.data_as(C.POINTER(C.c_float))))
        return pcm

    def _streams_decode_pcm(self, ids, chunks, final):
        n = len(chunks)
        final = np.zeros(n, np.uint8) if final is None else np.ascontiguousarray(np.asarray(final).reshape(-1) != 0, np.uint8)
        if final.shape != (n,):
            raise ValueError("streams_decode_ragged: one final flag per item")
        T = np.array([c.shape[1] for c in chunks], np.int32)
        codes = np.concatenate([c.reshape(-1) for c in chunks] + [np.zeros(1, np.uint32)])
        dts = [self._dtypes().get(int(i), "f32") for i in ids]
        counts = [self.streams_pending(int(i), int(t), bool(f)) for i, t, f in zip(ids, T, final)]
        sizes = [c * np.dtype(_ffi.PCM_DTYPES[d]).itemsize for c, d in zip(counts, dts)]
        buf = np.zeros(max(1, sum(sizes)), np.uint8)
        got = (C.c_int64 * n)()
        _ffi.check(_ffi.lib().fs_codec_streams_decode_pcm(self._h, int(n), ids.ctypes.data_as(C.POINTER(C.c_int)), T.ctypes.data_as(C.POINTER(C.c_int)),
                                                          final.ctypes.data_as(C.POINTER(C.c_uint8)), codes.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                          buf.ctypes.data_as(C.c_void_p), C.c_size_t(sum(sizes)), got))
        out, at = [], 0
        for i in range(n):
            assert got[i] == counts[i]
            out.append(np.frombuffer(buf[at:at + sizes[i]].tobytes(), _ffi.PCM_DTYPES[dts[i]]))  # (a copy: an f32 item may start at an odd offset)
            at += sizes[i]
        return out

    def streams_decode_ragged(self, ids, chunks, final=None):
        """ids: n distinct open stream ids; chunks: n arrays u32 (8, T_i), T_i >= 1 and different per item: item i is the next chunk of stream
        ids[i] -> list of n f32 (2048 T_i,) PCM arrays.  Per stream, the chunks' PCM concatenated (through this call and streams_decode in
        any interleaving) is bit-identical to decode() of its whole sequence.  The items run at the stride of the longest one."""
        ids = np.ascontiguousarray(np.asarray(ids, np.int32).reshape(-1))
        chunks = [np.ascontiguousarray(c, np.uint32) for c in chunks]
        if len(chunks) != ids.shape[0]:
            raise ValueError("streams_decode_ragged: one chunk per stream id")
        if not 1 <= len(chunks) <= self.STREAMS_MAX:
            raise ValueError(f"streams_decode_ragged: 1 .. {self.STREAMS_MAX} streams per call")
        if final is not None or any(int(i) in self._dtypes() for i in ids):
            # fishrt.h fs_codec_streams_decode_pcm: a final flag per item (an (8, 0) chunk with final set is a pure flush), every item's PCM
            # in its stream's rate and dtype; a stream emits the samples whose input exists and the rest on its final item
            for c in chunks:
                if c.ndim != 2 or c.shape[0] != 8:
                    raise ValueError("streams_decode_ragged: every chunk must have shape (8, T)")
            return self._streams_decode_pcm(ids, chunks, final)
        for c in chunks:
            if c.ndim != 2 or c.shape[0] != 8 or c.shape[1] < 1:
                raise ValueError("streams_decode_ragged: every chunk must have shape (8, T) with T >= 1")
        T = np.array([c.shape[1] for c in chunks], np.int32)
        codes = np.concatenate([c.reshape(-1) for c in chunks])
        pcm = np.empty(2048 * int(T.sum()), np.float32)
        _ffi.check(_ffi.lib().fs_codec_streams_decode_ragged(self._h, int(len(chunks)), ids.ctypes.data_as(C.POINTER(C.c_int)),
                                                             T.ctypes.data_as(C.POINTER(C.c_int)), codes.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                             pcm.ctypes.data_as(C.POINTER(C.c_float))))
        ends = 2048 * np.cumsum(T)
        return [pcm[e - 2048 * t:e] for e, t in zip(ends, T)]

    def encode_stage(self, pcm, stage):
        """fishrt.h fs_selftest_codec_encode_stage: encode() of one mono clip at the codec rate with ONE intermediate tensor copied out -> f32,
        channel-first, flat (the log-mel as (160, frames)): stage -1 the log-mel, 0..3 after each backbone stage, 4 after the final LayerNorm, 5 / 6 after each downsample block;
        stage -2 (pcm ignored): the handle's mel filterbank (1025, 160).  Diagnostics / parity tests."""
        if stage == -2:
            out, n = np.empty(1025 * 160, np.float32), C.c_size_t(0)
            _ffi.check(_ffi.lib().fs_selftest_codec_encode_stage(self._h, None, 0, -2, out.ctypes.data_as(C.POINTER(C.c_float)), C.c_size_t(out.size),
                                                                 C.byref(n)))
            return out[: n.value].reshape(1025, 160)
        pcm = np.ascontiguousarray(pcm, np.float32).reshape(-1)
        frames = pcm.size // 512 + 8
        out, n = np.empty(1025 * frames, np.float32), C.c_size_t(0)
        _ffi.check(_ffi.lib().fs_selftest_codec_encode_stage(self._h, pcm.ctypes.data_as(C.POINTER(C.c_float)), int(pcm.size), int(stage),
                                                             out.ctypes.data_as(C.POINTER(C.c_float)), C.c_size_t(out.size), C.byref(n)))
        rows = 160 if stage == -1 else None
        got = out[: n.value].copy()
        return got.reshape(rows, -1) if rows else got  # stages 0..6: flat (channels * frames); the caller knows the stage's width

    def _encode_pcm(self, pcm_data, lengths, sample_rate, resample):
        if resample not in _ffi.RESAMPLE_MODES:
            raise ValueError(f"resample mode must be one of {sorted(_ffi.RESAMPLE_MODES)}")
        if pcm_data.ndim != 3:
            raise ValueError("pcm_data must be a 3-D array (b, channels, n)")
        b, ch, n_max = pcm_data.shape
        ns = [n_max] * b if lengths is None else [int(v) for v in lengths]
        if len(ns) != b or any(v <= 0 or v > n_max for v in ns):
            raise ValueError("lengths must hold one sample count in (0, n] per clip")
        out = []
        for i in range(b):
            inter = np.ascontiguousarray(pcm_data[i, :, : ns[i]].astype(np.float32, copy=False).T)  # [frames][channels]
            cap = int(ns[i] * (self.sample_rate / float(sample_rate))) // 2048 + 8
            codes = np.zeros((8, cap), np.uint32)
            nf = C.c_size_t(0)
            _ffi.check(_ffi.lib().fs_codec_encode_pcm(self._h, inter.ctypes.data_as(C.POINTER(C.c_float)), int(ch), int(ns[i]), int(sample_rate),
                                                      _ffi.RESAMPLE_MODES[resample], codes.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                      C.c_size_t(cap), C.byref(nf)))
            out.append(codes[:, : nf.value].copy())
        if lengths is not None:
            return out
        assert len(set(c.shape[1] for c in out)) == 1
        return np.stack(out)

    def encode(self, pcm_data, lengths=None, sample_rate=None, resample="linear"):
        """codec.rs:73-94 / firefly.rs:36-39: f32 (b, 1, n) mono 44.1 kHz PCM -> u32 (b, 8, L).  Every clip is encoded on its own
        (fishrt.h fs_codec_encode_batch; the reference's front-end would glue a batch into one signal, spectrogram.rs:33).  lengths: optional
        per-clip sample counts <= n (ragged clips, zero-padded rows) -> list of (8, L_i) instead of one array."""
        if not isinstance(pcm_data, np.ndarray) or not pcm_data.flags["C_CONTIGUOUS"]:
            raise ValueError("Data must be a contiguous array")
        if sample_rate is not None:
            # fishrt.h fs_codec_encode_pcm: (b, channels, n) at sample_rate Hz -> downmix, resample to the codec rate and encode on the device
            return self._encode_pcm(pcm_data, lengths, sample_rate, resample)
        if pcm_data.ndim != 3 or pcm_data.shape[1] != 1:
            raise ValueError("pcm_data must be a 3-D array (b, 1, n)")
        b, _, n_max = pcm_data.shape
        pcm = np.ascontiguousarray(pcm_data.astype(np.float32, copy=False).reshape(b, n_max))
        ns = np.array([n_max] * b if lengths is None else [int(v) for v in lengths], np.int32)
        if ns.shape != (b,) or (ns <= 0).any() or (ns > n_max).any():
            raise ValueError("lengths must hold one sample count in (0, n] per clip")
        cap = n_max // 2048 + 4
        codes = np.zeros((b, 8, cap), np.uint32)
        nf = (C.c_size_t * b)()
        _ffi.check(_ffi.lib().fs_codec_encode_batch(self._h, pcm.ctypes.data_as(C.POINTER(C.c_float)), int(b), C.c_size_t(n_max),
                                                    ns.ctypes.data_as(C.POINTER(C.c_int)), codes.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                    C.c_size_t(cap), nf))
        if lengths is not None:
            return [codes[i, :, : nf[i]].copy() for i in range(b)]
        assert len(set(nf[i] for i in range(b))) == 1
        return codes[:, :, : nf[0]].copy()

