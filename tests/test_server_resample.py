"""CPU: the serving shim's device sample-rate conversion options (fishrt/server.py AppState(device_resample=, opus_rate=)).  The LM and the
codec are stand-ins that record how they are driven, as in tests/test_server_shim.py: what is checked is which codec calls the routes make
and what the answers carry -- the `sample_rate` field accepted or rejected by the option, the WAV header's rate, the `pcm` byte count per
chunk (fishrt.resample_out_len), the arguments the Opus hook gets, and the encoding route going through the codec or through scipy."""
import io
import struct

import numpy as np
import pytest

import fishrt
from fishrt import server

from test_server_shim import FakeLM, Tok
from fishrt import prompt as fprompt


class RecordingCodec:
    sample_rate = 44100

    def __init__(self):
        self.decodes, self.encodes = [], []

    def decode(self, codes, sample_rate=None, resample="linear", dtype="f32"):
        b, _, t = codes.shape
        self.decodes.append(dict(frames=t, sample_rate=sample_rate, resample=resample, dtype=dtype))
        n = 2048 * t if sample_rate in (None, 44100) else fishrt.resample_out_len(2048 * t, 44100, sample_rate, resample)
        return np.full((b, 1, n), 0.25 if dtype == "f32" else 8191, np.float32 if dtype == "f32" else np.int16)

    def encode(self, pcm, lengths=None, sample_rate=None, resample="linear"):
        self.encodes.append(dict(shape=pcm.shape, sample_rate=sample_rate, resample=resample))
        return np.full((1, 8, 5), 7, np.uint32)


def _state(**kw):
    tok = Tok()
    enc = fprompt.PromptEncoder(tok, 8, fprompt.FISH_1_5)
    default = enc.encode_conditioning_prompt("hello there", np.full((8, 4), 3, np.uint32))
    lm = FakeLM()
    ls = server.LMState(lm, tok, {"default": default}, default, max_new_tokens=lm.M, max_batch=1)
    codec = RecordingCodec()
    return server.AppState(ls, codec, batch_window_s=0.05, **kw), codec


def _client(state):
    from fastapi.testclient import TestClient
    return TestClient(server.make_app(state))


TEXT = "First sentence is here and it is long enough to stand alone as a chunk of text for the model to speak aloud, yes it is. " * 2 + \
       "Second one follows, also long enough to be its own chunk because the combine threshold is one hundred and fifty characters. " * 2


def test_sample_rate_is_rejected_without_the_option_and_nothing_else_changes():
    state, codec = _state()
    c = _client(state)
    r = c.post("/v1/audio/speech", json=dict(model="tts-1", voice="default", input=TEXT, sample_rate=24000))
    assert r.status_code == 422 and "device_resample" in r.json()["detail"] and not codec.decodes
    r = c.post("/v1/audio/speech", json=dict(model="tts-1", voice="default", input=TEXT))
    assert r.status_code == 200 and struct.unpack("<I", r.content[24:28])[0] == 44100
    assert codec.decodes and all(d["sample_rate"] is None and d["dtype"] == "f32" for d in codec.decodes)
    with pytest.raises(ValueError):
        _state(device_resample="cubic")


def test_wav_carries_the_requested_rate_and_pcm_the_resampled_byte_count():
    state, codec = _state(device_resample="sinc")
    c = _client(state)
    r = c.post("/v1/audio/speech", json=dict(model="tts-1", voice="default", input=TEXT, sample_rate=24000))
    assert r.status_code == 200 and r.headers["content-type"] == "audio/wav"
    rate, byte_rate = struct.unpack("<II", r.content[24:32])
    assert rate == 24000 and byte_rate == 48000
    assert len(codec.decodes) >= 2 and all(d == dict(frames=d["frames"], sample_rate=24000, resample="sinc", dtype="s16") for d in codec.decodes)
    want = sum(fishrt.resample_out_len(2048 * d["frames"], 44100, 24000, "sinc") for d in codec.decodes)
    assert struct.unpack("<I", r.content[40:44])[0] == 2 * want and np.frombuffer(r.content[44:], "<i2").tolist() == [8191] * want
    first = list(codec.decodes)
    del codec.decodes[:]
    r = c.post("/v1/audio/speech", json=dict(model="tts-1", voice="default", input=TEXT, sample_rate=16000, response_format="pcm"))
    assert r.status_code == 200 and r.headers["content-type"].startswith("audio/pcm")
    assert [d["frames"] for d in codec.decodes] == [d["frames"] for d in first]
    assert len(r.content) == sum(2 * fishrt.resample_out_len(2048 * d["frames"], 44100, 16000, "sinc") for d in codec.decodes)
    # without the field the option changes nothing: f32 from the codec at its own rate, converted on the host as ever
    del codec.decodes[:]
    r = c.post("/v1/audio/speech", json=dict(model="tts-1", voice="default", input=TEXT, response_format="pcm"))
    assert r.status_code == 200 and len(r.content) == sum(2 * 2048 * d["frames"] for d in codec.decodes)
    assert all(d["sample_rate"] is None and d["dtype"] == "f32" for d in codec.decodes)
    for bad in (0, "24000", 2.5, True):
        r = c.post("/v1/audio/speech", json=dict(model="tts-1", voice="default", input=TEXT, sample_rate=bad))
        assert r.status_code == 422, bad


def test_the_opus_hook_gets_pcm_at_opus_rate_when_set():
    got = []

    def hook(pcm, rate):
        got.append((pcm.dtype, pcm.shape[0], rate))
        return [b"x"]

    state, codec = _state(opus_encoder=hook, opus_rate=24000, device_resample="linear")
    r = _client(state).post("/v1/audio/speech", json=dict(model="tts-1", voice="default", input=TEXT, response_format="opus"))
    assert r.status_code == 200 and r.content == b"x" * len(codec.decodes)
    assert all(d["sample_rate"] == 24000 and d["resample"] == "linear" and d["dtype"] == "f32" for d in codec.decodes)
    assert got == [(np.dtype(np.float32), fishrt.resample_out_len(2048 * d["frames"], 44100, 24000, "linear"), 24000) for d in codec.decodes]
    # today's arguments without opus_rate: f32 at the codec rate
    del got[:]
    state, codec = _state(opus_encoder=hook)
    r = _client(state).post("/v1/audio/speech", json=dict(model="tts-1", voice="default", input=TEXT, response_format="opus"))
    assert r.status_code == 200
    assert got == [(np.dtype(np.float32), 2048 * d["frames"], 44100) for d in codec.decodes] and all(d["sample_rate"] is None for d in codec.decodes)


def _wav(x, sr):  # (channels, n) f32 -> float32 WAV bytes
    data = np.ascontiguousarray(x.T, "<f4").tobytes()
    ch = x.shape[0]
    return (b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVE" + b"fmt " + struct.pack("<IHHIIHH", 16, 3, ch, sr, sr * 4 * ch, 4 * ch, 32)
            + b"data" + struct.pack("<I", len(data)) + data)


def test_the_encoding_route_goes_through_the_codec_only_with_the_option():
    x = np.random.RandomState(0).uniform(-0.5, 0.5, (2, 22050)).astype(np.float32)
    state, codec = _state(device_resample="linear")
    r = _client(state).post("/v1/audio/encoding", files=dict(file=("a.wav", io.BytesIO(_wav(x, 22050)), "audio/wav")))
    assert r.status_code == 200
    assert codec.encodes == [dict(shape=(1, 2, 22050), sample_rate=22050, resample="linear")]
    state, codec = _state()
    r = _client(state).post("/v1/audio/encoding", files=dict(file=("a.wav", io.BytesIO(_wav(x, 22050)), "audio/wav")))
    assert r.status_code == 200
    assert codec.encodes == [dict(shape=(1, 1, 44100), sample_rate=None, resample="linear")]  # downmixed and resampled on the host, as before
