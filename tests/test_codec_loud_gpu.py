"""GPU: fs_codec_decode_loud on synthetic codec weights against the composition of the stand-alone calls it is defined by --
fs_resample(fs_time_stretch(fs_loudness_normalize(fs_codec_decode))) -- bit for bit, with the same gain; without loudness parameters it is
fs_codec_decode_speed; a refused call (a bad target, a cap too small) leaves the handle usable."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import fishrt
from fishrt import _ffi

B, T = 2, 24
TARGET = -23.0


@pytest.fixture(scope="module")
def codec():
    c = fishrt.FireflyCodec(0).load_synthetic(0xC0DEC)
    yield c
    c.close()


@pytest.fixture(scope="module")
def codes():
    return np.random.RandomState(24).randint(0, 1000, (B, 8, T)).astype(np.uint32)


@pytest.fixture(scope="module")
def scaled(codec, codes):
    """the vocoder's rows through the stand-alone call: (rows * gain, records)"""
    pcm = codec.decode(codes)[:, 0]
    y, infos = fishrt.loudness_normalize(pcm, 44100, TARGET, return_info=True)
    print("vocoder rows:", infos)
    assert all(i["blocks_total"] == 2048 * T // 4410 - 3 and i["blocks_kept"] > 0 and i["gain"] != 1.0 for i in infos)  # (the stage has work to do)
    for i in range(B):
        assert np.array_equal(y[i], pcm[i] * np.float32(infos[i]["gain"]))
    return y, infos


@pytest.mark.parametrize("speed", [1.0, 1.25])
@pytest.mark.parametrize("spec", [dict(), dict(sample_rate=24000, resample="sinc", dtype="s16")], ids=["codec-rate-f32", "24k-sinc-s16"])
def test_decode_loud_is_the_composition_of_the_stand_alone_calls(codec, codes, scaled, speed, spec):
    y, infos = scaled
    got = codec.decode(codes, loudness=TARGET, speed=speed, **spec)
    assert codec.last_loudness == infos  # the same L, peak, gain and counts as the stand-alone call on the same rows
    st = fishrt.time_stretch(y, speed) if speed != 1.0 else y
    if spec:
        ref = fishrt.resample(st, 44100, 24000, mode="sinc", dtype="s16")
    else:  # the codec's own rate: the format stage alone, f32 to f32
        ref = fishrt.resample(st, 44100, 44100, mode="linear", dtype="f32")
        assert np.array_equal(ref, st)
    assert got.dtype == ref.dtype and got.shape == (B, 1, ref.shape[1]) and np.array_equal(got[:, 0], ref)
    # speed=None is speed 1.0
    if speed == 1.0:
        assert np.array_equal(codec.decode(codes, loudness=TARGET, **spec), got)


def _raw(codec, codes, loud, speed, spec, cap, res=True):
    out = np.zeros((B, max(cap, 1)), _ffi.PCM_DTYPES["s16" if spec.format else "f32"])
    got, rec = (C.c_int64 * B)(), (_ffi.LoudResult * B)()
    rc = _ffi.lib().fs_codec_decode_loud(codec._h, codes.ctypes.data_as(C.POINTER(C.c_uint32)), B, T, C.byref(loud) if loud is not None else None,
                                         C.c_double(speed), C.byref(spec), out.ctypes.data_as(C.c_void_p), C.c_size_t(cap), got, rec if res else None)
    return rc, _ffi.lib().fs_last_error().decode(), out, list(got), rec


def test_without_loudness_parameters_it_is_decode_speed(codec, codes):
    for speed, kw in ((1.25, dict(sample_rate=24000, resample="sinc", dtype="s16")), (1.0, dict(dtype="f32")), (0.8, dict(dtype="f32"))):
        want = codec.decode(codes, speed=speed, **kw)[:, 0]
        spec = _ffi.pcm_spec(kw.get("sample_rate", 44100), kw.get("resample", "linear"), kw["dtype"])
        rc, msg, out, got, rec = _raw(codec, codes, None, speed, spec, want.shape[1])
        assert rc == 0 and got == [want.shape[1]] * B and np.array_equal(out, want), msg
        assert all(r.blocks_total == 0 and r.gain == 0.0 for r in rec)  # (untouched)


def test_a_refused_call_leaves_the_handle_usable(codec, codes, scaled):
    spec = _ffi.pcm_spec(24000, "sinc", "s16")
    n = fishrt.resample_out_len(fishrt.time_stretch_out_len(2048 * T, 1.25), 44100, 24000, "sinc")
    ok = _ffi.LoudParams(TARGET, -1.0, 30.0)
    want = codec.decode(codes, loudness=TARGET, speed=1.25, sample_rate=24000, resample="sinc", dtype="s16")[:, 0]
    for loud, word in ((_ffi.LoudParams(-41.0, -1.0, 30.0), "target_lufs"), (_ffi.LoudParams(TARGET, 1.0, 30.0), "peak_db"),
                       (_ffi.LoudParams(TARGET, -1.0, 70.0), "max_gain_db")):
        rc, msg, out, got, rec = _raw(codec, codes, loud, 1.25, spec, n)
        assert rc != 0 and word in msg and not out.any(), msg
    rc, msg, out, got, rec = _raw(codec, codes, ok, 1.25, spec, n - 1)
    assert rc != 0 and "fs_codec_decode_loud" in msg and "cap" in msg and not out.any(), msg
    rc, msg, out, got, rec = _raw(codec, codes, ok, 5.0, spec, n)
    assert rc != 0 and "speed" in msg, msg
    rc, msg, out, got, rec = _raw(codec, codes, ok, 1.25, spec, n)
    assert rc == 0 and got == [n] * B and np.array_equal(out, want), msg
    assert [fishrt._loud._record(r) for r in rec] == scaled[1]
    rc, msg, out, got, rec = _raw(codec, codes, ok, 1.25, spec, n, res=False)  # the records are optional
    assert rc == 0 and np.array_equal(out, want)
    with pytest.raises(RuntimeError, match="target_lufs"):
        codec.decode(codes, loudness=-3.0)
    with pytest.raises(ValueError):
        codec.decode(codes, peak_db=-3.0)
    assert np.array_equal(codec.decode(codes, loudness=TARGET, speed=1.25, sample_rate=24000, resample="sinc", dtype="s16")[:, 0], want)
