"""fishrt: MI355X-native Fish-Speech hot path (dual-AR decode + Firefly vocoder) behind the C ABI of include/fishrt.h.
Python here is only the host-side mirror of the reference's PyO3 surface; all compute is hand-written HIP in libfishrt.so."""
from . import config
from ._ffi import LIB_PATH, SYMBOLS, lib
from .codec import FireflyCodec
from .lm import LM, DualARTransformer, prefix_blob_info
from ._resample import resample, resample_out_len
from ._tsm import time_stretch, time_stretch_out_len
from ._loud import loudness, loudness_normalize
from .stream import SessionStreamer, StreamingSynth, decode_chunk

__all__ = ["config", "lib", "LIB_PATH", "SYMBOLS", "DualARTransformer", "LM", "prefix_blob_info", "FireflyCodec", "StreamingSynth", "SessionStreamer", "decode_chunk",
           "resample", "resample_out_len", "time_stretch", "time_stretch_out_len", "loudness", "loudness_normalize"]
