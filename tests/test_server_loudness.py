"""CPU: the serving shim's `loudness` field (fishrt/server.py AppState(device_loudness=)).  The LM and the codec are stand-ins that record how
they are driven, as in tests/test_server_speed.py.  With the option on, a WAV request with `loudness` vocodes its chunks in ONE
codec.decode(loudness=) call over their codes in order, with `speed` and `sample_rate` passed on; a value that is not a number in -40 .. -5
answers 422 with a message; the `pcm` and Opus answers, which stream chunk by chunk, refuse the field with a 422 that says why; with the
option off the field answers 422 too.  A request without the field makes the calls it made before, option on or off."""
import struct

import numpy as np

import fishrt
from fishrt import server

from test_server_speed import REQ, RecordingCodec, _client, _stretched
from test_server_shim import FakeLM, Tok
from fishrt import prompt as fprompt


class LoudCodec(RecordingCodec):
    def decode(self, codes, loudness=None, **kw):
        n_before = len(self.decodes)
        pcm = super().decode(codes, **kw)
        if loudness is not None:
            self.decodes[n_before]["loudness"] = loudness
        return pcm


def _state(**kw):
    tok = Tok()
    enc = fprompt.PromptEncoder(tok, 8, fprompt.FISH_1_5)
    default = enc.encode_conditioning_prompt("hello there", np.full((8, 4), 3, np.uint32))
    lm = FakeLM()
    ls = server.LMState(lm, tok, {"default": default}, default, max_new_tokens=lm.M, max_batch=1)
    codec = LoudCodec()
    return server.AppState(ls, codec, batch_window_s=0.05, **kw), codec


def test_a_request_without_the_field_makes_the_calls_it_made():
    state, codec = _state()
    plain = _client(state).post("/v1/audio/speech", json=REQ)
    calls = list(codec.decodes)
    assert plain.status_code == 200 and len(calls) >= 2 and all("loudness" not in d for d in calls)
    for kw in (dict(device_loudness=True), dict(device_loudness=True, device_speed=True, device_resample="sinc")):
        state, codec = _state(**kw)
        c = _client(state)
        r = c.post("/v1/audio/speech", json=REQ)
        assert r.status_code == 200 and r.content == plain.content and codec.decodes == calls
        r = c.post("/v1/audio/speech", json=dict(REQ, loudness=None))
        assert r.status_code == 200 and r.content == plain.content and codec.decodes == calls * 2
        del codec.decodes[:]
        assert c.post("/v1/audio/speech", json=dict(REQ, response_format="pcm")).status_code == 200 and codec.decodes == calls


def test_loudness_reaches_the_codec_in_one_call_over_the_whole_answer():
    state, codec = _state()
    _client(state).post("/v1/audio/speech", json=REQ)
    frames = [d["frames"] for d in codec.decodes]
    state, codec = _state(device_loudness=True, device_speed=True, device_resample="sinc")
    c = _client(state)
    # WAV at the codec's rate
    r = c.post("/v1/audio/speech", json=dict(REQ, loudness=-16))
    assert r.status_code == 200 and r.headers["content-type"] == "audio/wav" and struct.unpack("<I", r.content[24:28])[0] == 44100
    assert codec.decodes == [dict(frames=sum(frames), loudness=-16.0)] and isinstance(codec.decodes[0]["loudness"], float)
    assert struct.unpack("<I", r.content[40:44])[0] == 2 * 2048 * sum(frames)
    # ... with speed and sample_rate: measured and scaled, then stretched, then resampled and packed, all in that call
    del codec.decodes[:]
    r = c.post("/v1/audio/speech", json=dict(REQ, loudness=-23.5, speed=1.25, sample_rate=24000))
    assert r.status_code == 200 and struct.unpack("<I", r.content[24:28])[0] == 24000
    assert codec.decodes == [dict(frames=sum(frames), sample_rate=24000, resample="sinc", dtype="s16", speed=1.25, loudness=-23.5)]
    want = fishrt.resample_out_len(_stretched(2048 * sum(frames), 1.25), 44100, 24000, "sinc")
    assert struct.unpack("<I", r.content[40:44])[0] == 2 * want
    # the ends of the range
    for ok in (-40, -5, -5.0, -39.99):
        assert c.post("/v1/audio/speech", json=dict(REQ, loudness=ok)).status_code == 200, ok


def test_bad_values_answer_422_with_a_message():
    state, codec = _state(device_loudness=True)
    c = _client(state)
    for bad in (-40.5, -4.9, 0, 3, "-16", True, [-16], {"x": 1}):
        r = c.post("/v1/audio/speech", json=dict(REQ, loudness=bad))
        assert r.status_code == 422 and "loudness" in r.json()["detail"] and "-40 .. -5" in r.json()["detail"], bad
    status, _, body = server.generate_speech(state, dict(REQ, loudness=float("nan")))  # (JSON has no NaN; a caller of the core may pass one)
    assert status == 422 and b"loudness" in body
    assert not codec.decodes


def test_streaming_answers_refuse_the_field_and_say_why():
    state, codec = _state(device_loudness=True, opus_encoder=lambda pcm, rate: [b"x"])
    c = _client(state)
    for fmt in ("pcm", "opus"):
        r = c.post("/v1/audio/speech", json=dict(REQ, loudness=-16, response_format=fmt))
        assert r.status_code == 422 and "loudness" in r.json()["detail"] and "whole signal" in r.json()["detail"] and fmt in r.json()["detail"]
    assert not codec.decodes
    assert c.post("/v1/audio/speech", json=dict(REQ, loudness=-16)).status_code == 200


def test_the_field_needs_the_option():
    state, codec = _state()
    r = _client(state).post("/v1/audio/speech", json=dict(REQ, loudness=-16))
    assert r.status_code == 422 and "device_loudness" in r.json()["detail"] and not codec.decodes
    state, codec = _state(device_speed=True)
    assert _client(state).post("/v1/audio/speech", json=dict(REQ, loudness="x")).status_code == 422 and not codec.decodes
