"""CPU: the serving shim's `speed` field (fishrt/server.py AppState(device_speed=)).  The LM and the codec are stand-ins that record how they
are driven, as in tests/test_server_resample.py.  With the option off the field is ignored and the answer's bytes are those of a request
without it; with it on the value reaches codec.decode(speed=) for the WAV, `pcm` and Opus-hook answers, before resampling and formatting,
and a value that is not a number in 0.25 .. 4.0 answers 422 with a message."""
import struct

import numpy as np

import fishrt
from fishrt import server

from test_server_shim import FakeLM, Tok
from fishrt import prompt as fprompt


def _stretched(n, speed):  # fishrt.time_stretch_out_len without the library's help: floor(n / speed + 0.5)
    return int(np.floor(n / speed + 0.5))


class RecordingCodec:
    sample_rate = 44100

    def __init__(self):
        self.decodes = []

    def decode(self, codes, **kw):
        b, _, t = codes.shape
        self.decodes.append(dict(frames=t, **kw))
        sample_rate, resample, dtype, speed = kw.get("sample_rate"), kw.get("resample", "linear"), kw.get("dtype", "f32"), kw.get("speed")
        n = 2048 * t if speed is None else _stretched(2048 * t, speed)
        if sample_rate not in (None, 44100):
            n = fishrt.resample_out_len(n, 44100, sample_rate, resample)
        return np.full((b, 1, n), 0.25 if dtype == "f32" else 8191, np.float32 if dtype == "f32" else np.int16)


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
REQ = dict(model="tts-1", voice="default", input=TEXT)


def test_speed_is_ignored_without_the_option_and_the_bytes_do_not_change():
    state, codec = _state()
    c = _client(state)
    plain = c.post("/v1/audio/speech", json=REQ)
    calls = list(codec.decodes)
    del codec.decodes[:]
    for speed in (1.25, "fast", 9, None):  # (not even looked at)
        r = c.post("/v1/audio/speech", json=dict(REQ, speed=speed))
        assert r.status_code == 200 and r.content == plain.content
    assert codec.decodes == calls * 4 and all("speed" not in d for d in codec.decodes)
    # the option on, a request without the field: the codec calls of before
    state, codec = _state(device_speed=True)
    r = _client(state).post("/v1/audio/speech", json=REQ)
    assert r.status_code == 200 and r.content == plain.content and codec.decodes == calls
    r = _client(state).post("/v1/audio/speech", json=dict(REQ, speed=None))
    assert r.status_code == 200 and r.content == plain.content


def test_speed_reaches_the_codec_for_wav_pcm_and_opus():
    got = []

    def hook(pcm, rate):
        got.append((pcm.dtype, pcm.shape[0], rate))
        return [b"x"]

    state, codec = _state(device_speed=True, device_resample="sinc", opus_encoder=hook, opus_rate=24000)
    c = _client(state)
    # WAV at the codec's rate: f32 from the codec, stretched
    r = c.post("/v1/audio/speech", json=dict(REQ, speed=1.25))
    assert r.status_code == 200 and r.headers["content-type"] == "audio/wav" and struct.unpack("<I", r.content[24:28])[0] == 44100
    assert len(codec.decodes) >= 2 and all(d == dict(frames=d["frames"], speed=1.25) for d in codec.decodes)
    assert struct.unpack("<I", r.content[40:44])[0] == 2 * sum(_stretched(2048 * d["frames"], 1.25) for d in codec.decodes)
    frames = [d["frames"] for d in codec.decodes]
    # WAV with sample_rate: stretched, then resampled and packed on the device
    del codec.decodes[:]
    r = c.post("/v1/audio/speech", json=dict(REQ, speed=0.5, sample_rate=24000))
    assert r.status_code == 200 and struct.unpack("<I", r.content[24:28])[0] == 24000
    assert codec.decodes == [dict(frames=f, sample_rate=24000, resample="sinc", dtype="s16", speed=0.5) for f in frames]
    want = sum(fishrt.resample_out_len(_stretched(2048 * f, 0.5), 44100, 24000, "sinc") for f in frames)
    assert struct.unpack("<I", r.content[40:44])[0] == 2 * want
    # pcm, with and without sample_rate; an integer speed is a number too
    del codec.decodes[:]
    r = c.post("/v1/audio/speech", json=dict(REQ, speed=2, response_format="pcm"))
    assert r.status_code == 200 and len(r.content) == 2 * sum(_stretched(2048 * f, 2.0) for f in frames)
    assert codec.decodes == [dict(frames=f, speed=2.0) for f in frames]
    del codec.decodes[:]
    r = c.post("/v1/audio/speech", json=dict(REQ, speed=4.0, response_format="pcm", sample_rate=16000))
    assert r.status_code == 200 and codec.decodes == [dict(frames=f, sample_rate=16000, resample="sinc", dtype="s16", speed=4.0) for f in frames]
    assert len(r.content) == 2 * sum(fishrt.resample_out_len(_stretched(2048 * f, 4.0), 44100, 16000, "sinc") for f in frames)
    # the Opus hook: stretched PCM at opus_rate
    del codec.decodes[:]
    r = c.post("/v1/audio/speech", json=dict(REQ, speed=0.25, response_format="opus"))
    assert r.status_code == 200 and r.content == b"x" * len(frames)
    assert codec.decodes == [dict(frames=f, sample_rate=24000, resample="sinc", dtype="f32", speed=0.25) for f in frames]
    assert got == [(np.dtype(np.float32), fishrt.resample_out_len(_stretched(2048 * f, 0.25), 44100, 24000, "sinc"), 24000) for f in frames]
    # ... and without opus_rate, at the codec's
    del got[:]
    state, codec = _state(device_speed=True, opus_encoder=hook)
    r = _client(state).post("/v1/audio/speech", json=dict(REQ, speed=1.5, response_format="opus"))
    assert r.status_code == 200 and got == [(np.dtype(np.float32), _stretched(2048 * f, 1.5), 44100) for f in frames]
    assert codec.decodes == [dict(frames=f, speed=1.5) for f in frames]


def test_bad_speed_values_answer_422_with_a_message():
    state, codec = _state(device_speed=True)
    c = _client(state)
    for bad in (0.2, 4.01, 0, -1, "1.25", True, [1.25], {"x": 1}):
        r = c.post("/v1/audio/speech", json=dict(REQ, speed=bad))
        assert r.status_code == 422 and "speed" in r.json()["detail"] and "0.25 .. 4.0" in r.json()["detail"], bad
    assert not codec.decodes
    status, _, body = server.generate_speech(state, dict(REQ, speed=float("nan")))  # (JSON has no NaN; a caller of the core may pass one)
    assert status == 422 and b"speed" in body
    for ok in (0.25, 1, 1.0, 4):
        assert c.post("/v1/audio/speech", json=dict(REQ, speed=ok)).status_code == 200, ok
