"""CPU: the hidden-states request of the serving shim (fishrt/server.py generate_hidden_states; server/lib/handlers/send_hidden_states.rs)
-- response archive, scheduling of collecting jobs in and outside a session, and that a lock-step batch never carries one.  Stand-in LM /
codec handles in the style of tests/test_server_shim.py (the real ones need an MI355X)."""
import io
import json
import struct
import threading
import zipfile

import numpy as np

from fishrt import prompt as fprompt
from fishrt import server

from test_server_shim import FakeCodec, FakeLM, FakeSession, Tok

DIM = 16


def _hidden(prompt, codes, extra):
    """rows of a generation: one per frame, plus `extra` (the terminating iteration); row r = r + the request's marker"""
    n = codes.shape[1] + extra
    return np.arange(n, dtype=np.float32)[:, None] + np.full((1, DIM), float(int(prompt[0, -5]) % 1000), np.float32)


class HiddenSession(FakeSession):
    def __init__(self, lm, kw):
        super().__init__(lm, kw)
        self.hid = {}

    def add(self, prompt, max_new_tokens, collect_hidden=False):
        slot = super().add(prompt, max_new_tokens)
        if slot is not None:
            self.hid[slot] = _hidden(prompt, self.slots[slot][0], self.lm.extra_for(prompt)) if collect_hidden else None
            self.lm.calls.append(("add_hidden" if collect_hidden else "add_plain", prompt.shape[1]))
        return slot

    def poll_hidden(self, slot, first=0):
        full, n = self.slots[slot]
        if self.hid[slot] is None:
            raise RuntimeError("the slot does not collect hidden states")
        assert n == full.shape[1], "the shim reads the rows of a finished slot"
        return self.hid[slot][first:].copy()


class HiddenLM(FakeLM):
    def __init__(self, **kw):
        super().__init__(**kw)
        self.cfg = dict(num_codebooks=8, dim=DIM)
        self.extra_for = lambda prompt: int(prompt[0, -5]) % 2  # some generations end on <|im_end|>: one row more than frames

    def generate_blocking_with_hidden(self, prompt, max_new_tokens, collect_hidden_states=True, **kw):
        assert collect_hidden_states
        codes = self.generate_blocking(prompt, max_new_tokens, **kw)
        self.calls[-1] = ("single_hidden",) + self.calls[-1][1:]
        return codes, _hidden(prompt, codes, self.extra_for(prompt))[:, None, :]  # (iterations, 1, dim) like fishrt.lm

    def session(self, **kw):
        return HiddenSession(self, kw)


def _state(max_batch=1, continuous=True, auto_batch=False, **lm_kw):
    tok = Tok()
    enc = fprompt.PromptEncoder(tok, 8, fprompt.FISH_1_5)
    default = enc.encode_conditioning_prompt("hello there", np.full((8, 4), 3, np.uint32))
    alice = enc.encode_conditioning_prompt("i am alice", np.full((8, 6), 9, np.uint32))
    lm = HiddenLM(**lm_kw)
    ls = server.LMState(lm, tok, {"default": default, "alice": alice}, default, max_new_tokens=lm.M, max_batch=max_batch)
    return server.AppState(ls, FakeCodec(), batch_window_s=0.05, continuous=continuous, auto_batch=auto_batch), lm


def _client(state):
    from fastapi.testclient import TestClient
    return TestClient(server.make_app(state))


TEXT = "First sentence is here and it is long enough to stand alone as a chunk of text for the model to speak aloud, yes it is. " * 2 + \
       "Second one follows, also long enough to be its own chunk because the combine threshold is one hundred and fifty characters. " * 2


def _open(r):
    assert r.status_code == 200 and r.headers["content-type"] == "application/zip", r.content[:200]
    z = zipfile.ZipFile(io.BytesIO(r.content))
    assert all(i.compress_type == zipfile.ZIP_STORED for i in z.infolist())  # FileOptions ... CompressionMethod::Stored
    return z


def _calls(lm, kind):
    return [k for k in lm.calls if k[0] == kind]


def test_hidden_states_archive_without_and_with_audio():
    state, lm = _state()
    c = _client(state)
    z = _open(c.post("/v1/audio/hidden_states", json=dict(text=TEXT, speaker_id="alice", return_audio=False)))
    assert z.namelist() == ["hidden_states.npy", "metadata.json"]
    hs = np.lib.format.read_array(io.BytesIO(z.read("hidden_states.npy")))
    chunks = state.preprocess(TEXT)
    assert len(chunks) >= 2 and len(_calls(lm, "single_hidden")) == len(chunks) and not _calls(lm, "single")
    # rows per chunk: the stand-in's frames (3 + last prompt token % 5) + its extra row; concatenated in chunk order
    enc = fprompt.PromptEncoder(Tok(), 8, fprompt.FISH_1_5)
    assistant = enc.encode_vq(None)
    bodies = [np.concatenate([enc.encode_text("user", ch), assistant], 1) for ch in chunks]
    frames = [lm._gen(b).shape[1] for b in bodies]
    rows = [f + lm.extra_for(b) for f, b in zip(frames, bodies)]
    assert rows != frames, "no chunk of the fixture ends on the extra row"
    want = np.concatenate([_hidden(b, lm._gen(b), lm.extra_for(b)) for b in bodies], 0)
    assert hs.dtype == np.float32 and hs.shape == (sum(rows), DIM)  # the sum of the chunks' row counts
    assert np.array_equal(hs, want)
    meta = json.loads(z.read("metadata.json"))
    assert meta == {"frame_count": hs.shape[0], "frame_rate": 21.535, "hidden_dim": DIM}
    # the chunks of one request reuse the conditioning prefix like a speech request's (speech.rs:40)
    assert state.scheduler.stats["prefix_hits"] == len(chunks) - 1
    # server default sampling (send_hidden_states.rs:60)
    kw = dict(_calls(lm, "single_hidden")[0][3])
    assert kw.pop("seed") in range(2**64) and kw == dict(temp=0.7, top_p=0.8, top_k=256, repetition_penalty=1.4)

    z = _open(c.post("/v1/audio/hidden_states", json=dict(text=TEXT, speaker_id="nobody", return_audio=True)))
    assert z.namelist() == ["hidden_states.npy", "audio.wav", "metadata.json"]
    wav = z.read("audio.wav")
    assert wav[:4] == b"RIFF" and wav[8:12] == b"WAVE" and struct.unpack("<I", wav[24:28])[0] == 44100
    hs2 = np.lib.format.read_array(io.BytesIO(z.read("hidden_states.npy")))
    assert struct.unpack("<I", wav[40:44])[0] // 2 == 2048 * sum(frames)  # the audio of the emitted frames; the rows may count one more per chunk
    assert hs2.shape == hs.shape and json.loads(z.read("metadata.json"))["frame_count"] == hs2.shape[0]
    # malformed bodies / no text
    assert c.post("/v1/audio/hidden_states", json=dict(text="Hi.", speaker_id="alice")).status_code == 422
    r = c.post("/v1/audio/hidden_states", json=dict(text="", speaker_id="alice", return_audio=False))
    assert r.status_code == 500 and b"Something went wrong" in r.content
    # the speech route is untouched by the new one
    r = c.post("/v1/audio/speech", json=dict(model="x", voice="alice", input="Hi."))
    assert r.status_code == 200 and r.headers["content-type"] == "audio/wav" and lm.calls[-1][0] == "single"
    state.scheduler.close()


def test_collecting_jobs_join_a_session_next_to_speech_jobs():
    """max_batch > 1, auto_batch: hidden-state chunks and speech chunks in flight together are slots of ONE session; the collecting ones are
    admitted with collect_hidden=True and read through poll_hidden, the others exactly as before"""
    state, lm = _state(max_batch=8, slow=0.02, auto_batch=True)
    lm.frames_for = lambda prompt: 20 + int(prompt[0, -5]) % 30
    c = _client(state)
    results = {}

    def go(i):
        if i % 2:
            results[i] = c.post("/v1/audio/hidden_states", json=dict(text=f"Request number {i}.", speaker_id="alice", return_audio=bool(i % 4 == 1)))
        else:
            results[i] = c.post("/v1/audio/speech", json=dict(model="x", voice="default", input=f"Request number {i}."))

    ths = [threading.Thread(target=go, args=(i,)) for i in range(6)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert all(r.status_code == 200 for r in results.values()), {i: r.content[:120] for i, r in results.items()}
    kinds = [k[0] for k in lm.calls]
    assert "add_hidden" in kinds and kinds.count("session") == kinds.count("session_end") >= 1
    in_session = kinds.count("add_hidden") + kinds.count("add_plain")
    assert in_session == state.scheduler.stats["batched_rows"] and in_session + state.scheduler.stats["single"] == 6
    assert kinds.count("add_hidden") + kinds.count("single_hidden") == 3 and "batch" not in kinds
    for i in (1, 3, 5):
        z = _open(results[i])
        hs = np.lib.format.read_array(io.BytesIO(z.read("hidden_states.npy")))
        assert hs.shape[1] == DIM and hs.shape[0] >= 20 and ("audio.wav" in z.namelist()) == (i % 4 == 1)
        assert np.array_equal(hs[:, 0] - hs[0, 0], np.arange(hs.shape[0], dtype=np.float32))  # one generation's rows, in order
    for i in (0, 2, 4):
        assert results[i].headers["content-type"] == "audio/wav"
    state.scheduler.close()


def test_a_lock_step_batch_never_carries_collect_hidden():
    """Scheduler(continuous=False): jobs waiting together go through one generate_static_batch call -- except the collecting ones, which
    run alone through generate_blocking_with_hidden (the reference's static batch returns no hidden states)"""
    state, lm = _state(max_batch=8, continuous=False)
    sch = state.scheduler
    seen = []
    batched = sch._batched
    sch._batched = lambda jobs: (seen.append([j.collect_hidden for j in jobs]), batched(jobs))[1]
    enc = fprompt.PromptEncoder(Tok(), 8, fprompt.FISH_1_5)
    bodies = [np.concatenate([enc.encode_text("user", f"Job {i}."), enc.encode_vq(None)], 1) for i in range(5)]
    gate = threading.Event()
    gen = lm.generate_blocking
    lm.generate_blocking = lambda *a, **k: (gate.wait(5), gen(*a, **k))[1]  # hold the worker on a first job while the others queue up
    first = sch.submit(None, bodies[0], 0, False)
    futs = [sch.submit(None, b, 0, True, collect_hidden=i in (1, 3)) for i, b in enumerate(bodies)]
    gate.set()
    first.result(timeout=10)
    outs = [f.result(timeout=10) for f in futs]
    assert seen and all(not any(flags) for flags in seen), seen
    batch_calls = [k for k in lm.calls if k[0] == "batch"]
    assert len(batch_calls) == 1 and len(batch_calls[0][1]) == 3
    assert [k[0] for k in lm.calls].count("single_hidden") == 2
    for i, o in enumerate(outs):
        if i in (1, 3):
            codes, hid = o
            assert codes.shape[0] == 8 and hid.shape == (codes.shape[1] + lm.extra_for(bodies[i]), DIM)
        else:
            assert isinstance(o, np.ndarray) and o.shape[0] == 8
    # and the assertion inside _batched itself
    j = server._Job(None, bodies[0], 0, True, collect_hidden=True)
    try:
        batched([j, j])
    except AssertionError as e:
        assert "lock-step" in str(e)
    else:
        raise AssertionError("_batched accepted a collecting job")
    sch.close()
