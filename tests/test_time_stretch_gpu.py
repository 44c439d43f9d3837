"""GPU: device time-stretch (fs_time_stretch, fs_time_stretch_out_len, fs_codec_decode_speed; csrc/codec_tsm.hip) against the numpy referee
of tests/tsm_refs.py.  Exact tier: the f64 chain has no near-tie frame, so the positions must equal it, and the PCM is the float32
overlap-add of those positions bit for bit -- each case as one ragged b = 3 call beside two short rows (1, 511, 512, 513, 1537 samples:
no frame, one frame to the sample, one sample into the second, three).  Refereed tier: the f64 errors are replayed along the device's own
positions; every pick must pass the derived admission test, may differ from the f64 winner only in a near-tie frame, and in at most
max(1, 5 %) of the frames.  Crafted: speed 1, a bit-for-bit periodic signal (the tie rule decides), digital silence, other parameters, and
every validation error.  Codec: fs_codec_decode_speed is fs_resample of fs_time_stretch of fs_codec_decode, bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import fishrt
from fishrt import _ffi

import tsm_refs as R

C = _ffi.C
SHORT = [1, 511, 512, 513, 1537]


def _ragged(x, speed, shorts):
    """x beside two of its own prefixes in one call -> the rows, (pcm, positions) per row"""
    rows = np.zeros((3, len(x)), np.float32)
    lens = [shorts[0], shorts[1], len(x)]
    for i, n in enumerate(lens):
        rows[i, :n] = x[:n]
        rows[i, n:] = 7.0  # (samples behind a row's length are not the row's: they must not be read)
    ys, ps = fishrt.time_stretch(rows, speed, return_positions=True, lengths=lens)
    return lens, ys, ps


@pytest.mark.parametrize("idx", range(len(R.EXACT)), ids=["%s-%d-%d-%g" % c for c in R.EXACT])
def test_exact_tier_positions_and_pcm_are_bitwise(idx):
    kind, n, seed, speed = R.EXACT[idx]
    x = R.signal(kind, n, seed)
    shorts = [SHORT[idx % 5], SHORT[(idx + 2) % 5]]
    lens, ys, ps = _ragged(x, speed, shorts)
    for i, ln in enumerate(lens):
        xi = x[:ln]
        want = R.chain_of(kind, n, seed, speed)[0] if ln == n else R.chain64(xi, speed)[0]
        out_len, K, _ = R.plan(ln, speed)
        assert len(ys[i]) == out_len == fishrt.time_stretch_out_len(ln, speed) and len(ps[i]) == K, (ln, speed)
        assert np.array_equal(ps[i], want), (ln, speed, np.flatnonzero(ps[i] != want)[:4].tolist())
        assert np.array_equal(ys[i], R.ola_f32(xi, ps[i], speed)), (ln, speed)


@pytest.mark.parametrize("case", R.REFEREED, ids=lambda c: "%s-%d-%d-%g" % c)
def test_refereed_tier_picks_are_admitted_and_differ_only_in_near_ties(case):
    kind, n, seed, speed = case
    x = R.signal(kind, n, seed)
    y, pos = fishrt.time_stretch(x, speed, return_positions=True)
    r = R.replay(x, speed, pos)
    print("refereed", case, r)
    assert r["admitted"] and r["stray"] == 0 and r["differ"] <= R.cap_of(r["frames"]), r
    assert np.array_equal(y, R.ola_f32(x, pos, speed))


def test_speed_one_is_identity_positions():
    x = R.signal("voiced", 9000, 3)
    y, pos = fishrt.time_stretch(x, 1.0, return_positions=True)
    assert pos.tolist() == [512 * k for k in range(18)]
    assert np.array_equal(y, R.ola_f32(x, pos, 1.0)) and np.array_equal(y[:512], x[:512])
    assert np.all(np.abs(y - x) <= 2.4e-7 * np.abs(x))


@pytest.mark.parametrize("case", R.CRAFTED, ids=lambda c: "%s-%d-%d-%g" % c)
def test_periodic_and_silence_are_bitwise_against_the_f64_chain(case):
    kind, n, seed, speed = case
    x = R.signal(kind, n, seed)
    y, pos = fishrt.time_stretch(x, speed, return_positions=True)
    want = R.chain_of(kind, n, seed, speed)[0]
    assert np.array_equal(pos, want), np.flatnonzero(pos != want)[:4].tolist()
    assert np.array_equal(y, R.ola_f32(x, pos, speed))


@pytest.mark.parametrize("frame,radius", [(256, 64), (1024, 0), (66, 3), (2048, 1024)])
def test_other_parameters(frame, radius):
    # noise: its search has one sharp minimum per frame (checked: no near-tie frame under the f64 chain at these parameters)
    x = R.signal("noise", 6000 if frame < 2048 else 9000, 9)
    for speed in (0.8, 1.25):
        want, ties = R.chain64(x, speed, N=frame, D=radius)
        assert not ties.any()
        y, pos = fishrt.time_stretch(x, speed, return_positions=True, frame=frame, radius=radius)
        assert np.array_equal(pos, want), (speed, np.flatnonzero(pos != want)[:4].tolist())
        assert np.array_equal(y, R.ola_f32(x, pos, speed, N=frame))
        if radius == 0:
            assert np.array_equal(pos, R.plan(len(x), speed, frame)[2])


def test_empty_rows_and_lengths():
    ys, ps = fishrt.time_stretch(np.zeros((2, 4), np.float32), 4.0, return_positions=True, lengths=[0, 1])
    assert [len(y) for y in ys] == [0, 0] and [len(p) for p in ps] == [0, 0]  # 1 / 4 + 0.5 rounds to no sample
    assert fishrt.time_stretch_out_len(1280, 1.25) == 1024 and fishrt.time_stretch_out_len(0, 0.25) == 0
    y = fishrt.time_stretch(np.arange(100, dtype=np.float32), 0.5)  # n < Hs: the row, then zeros
    assert y.tolist() == list(range(100)) + [0.0] * 100


def _call(x, speed, params=None, out_stride=None, pos_stride=None, b=1):
    x = np.ascontiguousarray(x, np.float32).reshape(1, -1)
    ns = np.array([x.shape[1]], np.int64)
    out = np.zeros((1, out_stride if out_stride is not None else 4 * x.shape[1] + 8), np.float32)
    pos = np.zeros((1, pos_stride if pos_stride is not None else 64), np.int64)
    got = (C.c_int64 * 1)()
    rc = _ffi.lib().fs_time_stretch(0, x.ctypes.data_as(C.POINTER(C.c_float)), b, C.c_size_t(x.shape[1]), ns.ctypes.data_as(C.POINTER(C.c_int64)),
                                    C.c_double(speed), C.byref(params) if params is not None else None, out.ctypes.data_as(C.POINTER(C.c_float)),
                                    C.c_size_t(out.shape[1]), got, pos.ctypes.data_as(C.POINTER(C.c_int64)), C.c_size_t(pos.shape[1]))
    return rc, _ffi.lib().fs_last_error().decode()


def test_every_validation_error_names_its_argument():
    x = R.signal("noise", 3000, 1)
    for speed in (0.2, 4.5, 0.0, -1.0, float("nan"), float("inf")):
        rc, msg = _call(x, speed)
        assert rc != 0 and "speed" in msg and "0.25 .. 4.0" in msg, (speed, msg)
        n = C.c_int64(0)
        assert _ffi.lib().fs_time_stretch_out_len(100, C.c_double(speed), C.byref(n)) != 0 and "speed" in _ffi.lib().fs_last_error().decode()
        with pytest.raises(RuntimeError, match="speed"):
            fishrt.time_stretch(x, speed)
    for frame, radius, word in ((62, 0, "frame"), (2050, 0, "frame"), (1023, 0, "frame"), (1024, -1, "radius"), (1024, 1025, "radius")):
        rc, msg = _call(x, 1.25, _ffi.TsmParams(frame, radius))
        assert rc != 0 and "fs_tsm_params" in msg and word in msg, (frame, radius, msg)
    rc, msg = _call(x, 1.25, out_stride=2399)  # 3000 / 1.25 = 2400 samples
    assert rc != 0 and "out_stride" in msg, msg
    rc, msg = _call(x, 1.25, pos_stride=4)  # 5 frames
    assert rc != 0 and "pos_stride" in msg, msg
    rc, msg = _call(x, 1.25, b=0)
    assert rc != 0 and "rows" in msg, msg
    assert _call(x, 1.25, out_stride=2400, pos_stride=5)[0] == 0
    with pytest.raises(ValueError):
        fishrt.time_stretch(np.zeros((2, 2, 2), np.float32), 1.25)


# ---- behind the codec
@pytest.fixture(scope="module")
def codec():
    c = fishrt.FireflyCodec(0).load_synthetic(0xC0DEC)
    yield c
    c.close()


@pytest.mark.parametrize("T", [8, 33])
def test_codec_decode_speed_is_resample_of_stretch_of_decode(codec, T):
    codes = np.random.RandomState(T).randint(0, 1000, (2, 8, T)).astype(np.uint32)
    pcm = codec.decode(codes)[:, 0]
    for speed in (1.25, 0.77):
        st = fishrt.time_stretch(pcm, speed)
        assert st.shape == (2, fishrt.time_stretch_out_len(2048 * T, speed))
        for dtype in ("f32", "s16"):
            for mode in ("linear", "sinc"):
                # the codec's own rate: a format conversion only, whatever the mode (fs_resample "linear" at equal rates is that conversion)
                got = codec.decode(codes, dtype=dtype, resample=mode, speed=speed)
                ref = fishrt.resample(st, 44100, 44100, mode="linear", dtype=dtype)
                assert got.dtype == ref.dtype and np.array_equal(got[:, 0], ref), (speed, dtype, mode, "codec rate")
                got = codec.decode(codes, sample_rate=24000, dtype=dtype, resample=mode, speed=speed)
                ref = fishrt.resample(st, 44100, 24000, mode=mode, dtype=dtype)
                assert got.shape == (2, 1, ref.shape[1]) and np.array_equal(got[:, 0], ref), (speed, dtype, mode, 24000)
    # speed 1.0: no stretch stage -- fs_codec_decode_pcm
    for kw in (dict(dtype="s16"), dict(sample_rate=24000, resample="sinc", dtype="f32"), dict()):
        assert np.array_equal(codec.decode(codes, speed=1.0, **kw), codec.decode(codes, **kw)), kw


def test_codec_decode_speed_validates_before_it_launches(codec):
    codes = np.zeros((1, 8, 8), np.uint32)
    with pytest.raises(RuntimeError, match="speed"):
        codec.decode(codes, speed=5.0)
    spec = _ffi.pcm_spec(24000, "sinc", "s16")
    n = fishrt.resample_out_len(fishrt.time_stretch_out_len(2048 * 8, 1.25), 44100, 24000, "sinc")
    out, got = np.zeros(n, np.int16), (C.c_int64 * 1)()
    args = (codec._h, codes.ctypes.data_as(C.POINTER(C.c_uint32)), 1, 8, C.c_double(1.25), C.byref(spec), out.ctypes.data_as(C.c_void_p))
    assert _ffi.lib().fs_codec_decode_speed(*args, C.c_size_t(n - 1), got) != 0
    msg = _ffi.lib().fs_last_error().decode()
    assert "fs_codec_decode_speed" in msg and "cap" in msg, msg
    assert _ffi.lib().fs_codec_decode_speed(*args, C.c_size_t(n), got) == 0 and got[0] == n
    bad = _ffi.pcm_spec(24000, "sinc", "s16")
    bad.format = 9
    assert _ffi.lib().fs_codec_decode_speed(*args[:5], C.byref(bad), args[6], C.c_size_t(n), got) != 0 and "format" in _ffi.lib().fs_last_error().decode()
