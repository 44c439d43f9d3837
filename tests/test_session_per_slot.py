"""CPU: FS_SESSION_PER_SLOT / fs_lm_session_add_ex through the layers that need no GPU -- header, exported symbols and the ctypes table
agree; Session.add validates its arguments before any call reaches the library; the scheduler's routing with a stand-in LM (default off:
nothing changes; on: per-slot session, per-job seed and settings, request-level settings never reach a lock-step sampler)."""
import ctypes as C
import os
import re
import threading

import numpy as np
import pytest

import fishrt
from fishrt import _ffi, lm as flm, prompt as fprompt, server, stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "fishrt.h")).read()


def test_header_exports_and_ffi_table_agree():
    assert re.search(r"#define\s+FS_SESSION_PER_SLOT\s+16u", HEADER)
    assert _ffi.FS_SESSION_PER_SLOT == 16 and _ffi.FS_SESSION_ROWS == 8 and _ffi.FS_GEN_IGNORE_EOS == 1
    m = re.search(r"int\s+fs_lm_session_add_ex\(([^;]*)\);", HEADER)
    assert m, "fs_lm_session_add_ex is not declared"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 8 and args[1] == "int prefix_id" and "fs_sampling*" in args[5] and "uint64_t*" in args[6] and args[7] == "int* slot"
    assert "fs_lm_session_add_ex" in fishrt.SYMBOLS
    getattr(fishrt.lib(), "fs_lm_session_add_ex")  # exported by the built library


class _RecLib:
    """records the session calls a fishrt.lm.Session makes instead of running them"""

    def __init__(self):
        self.calls = []

    def fs_lm_session_begin(self, h, s, seed, flags):
        self.calls.append(("begin", s._obj.temp, s._obj.top_k, round(s._obj.repetition_penalty, 3), int(flags)))
        return 0

    def fs_lm_session_end(self, h):
        return 0

    def fs_lm_session_add(self, h, p, L, mnt, slot):
        self.calls.append(("add", L, mnt))
        slot._obj.value = 0
        return 0

    def fs_lm_session_add_prefixed(self, h, pid, p, L, mnt, slot):
        self.calls.append(("add_prefixed", pid, L, mnt))
        slot._obj.value = 1
        return 0

    def fs_lm_session_add_ex(self, h, pid, p, L, mnt, sp, sd, slot):
        s = None if sp is None else (sp._obj.temp, sp._obj.top_p, sp._obj.top_k, round(sp._obj.repetition_penalty, 3))
        self.calls.append(("add_ex", pid, L, mnt, s, None if sd is None else int(sd._obj.value)))
        slot._obj.value = 2
        return 0


class _H:
    cfg = dict(num_codebooks=8)
    _h = None


@pytest.fixture
def rec(monkeypatch):
    r = _RecLib()
    monkeypatch.setattr(_ffi, "lib", lambda: r)
    return r


def test_session_flags_and_add_arguments(rec):
    p = np.zeros((9, 5), np.uint32)
    s = flm.Session(_H(), 0.7, 0.8, 256, 1, True, per_slot=True, repetition_penalty=1.4)
    assert rec.calls[-1] == ("begin", 0.7, 256, 1.4, 1 | 16)
    assert s.add(p, 20) == 0 and rec.calls[-1] == ("add", 5, 20)                       # no settings: the plain entry points
    assert s.add(p, 20, prefix=3) == 1 and rec.calls[-1] == ("add_prefixed", 3, 5, 20)
    assert s.add(p, 20, seed=9) == 2 and rec.calls[-1] == ("add_ex", -1, 5, 20, None, 9)
    s.add(p, 20, prefix=3, sampling=dict(temp=0.0))                                      # missing entries: the session's
    assert rec.calls[-1] == ("add_ex", 3, 5, 20, (0.0, 0.8, 256, 1.4), None)
    s.add(p, 20, sampling=server.SamplingArgs(0.9, 0.5, 50, 1.2), seed=2**64 - 1)       # a SamplingArgs-like object
    assert rec.calls[-1] == ("add_ex", -1, 5, 20, (0.9, 0.5, 50, 1.2), 2**64 - 1)
    n = len(rec.calls)
    for bad in (dict(sampling=dict(temperature=0.7)), dict(sampling=dict(temp=-1.0)), dict(sampling=dict(top_k=-1)), dict(sampling=7),
                dict(seed=-1), dict(seed=2**64)):
        with pytest.raises(ValueError):
            s.add(p, 20, **bad)
    with pytest.raises(ValueError):
        s.add(np.zeros((8, 5), np.uint32), 20, seed=1)
    assert len(rec.calls) == n, "a refused add must not reach the library"
    plain = flm.Session(_H(), 0.7, 0.8, 256, 1, False)
    assert rec.calls[-1] == ("begin", 0.7, 256, 1.0, 0)
    with pytest.raises(ValueError, match="per_slot=True"):
        plain.add(p, 20, seed=1)
    with pytest.raises(ValueError, match="exclude"):
        flm.Session(_H(), 0.7, 0.8, 256, 1, False, rows=True, per_slot=True)
    rows = flm.Session(_H(), 0.7, 0.8, 256, 1, False, rows=True)
    assert rows.add(p, 20, seed=4) == 2


def test_session_streamer_passes_sampling_and_seed_through():
    class S:
        def __init__(self):
            self.adds = []

        def add(self, prompt, mnt, **kw):
            self.adds.append(kw)
            return len(self.adds) - 1

    class Cd:
        STREAM_MIN_FRAMES = 16

        def streams_open(self):
            return 0

        def streams_close(self, sid):
            pass

    s = S()
    st = stream.SessionStreamer(s, Cd())
    st.add(np.zeros((9, 4), np.uint32), 30)
    st.add(np.zeros((9, 4), np.uint32), 30, prefix=2, sampling=dict(temp=0.0), seed=5)
    assert s.adds == [{}, dict(prefix=2, sampling=dict(temp=0.0), seed=5)]


# ---- scheduler routing with a stand-in LM (style of tests/test_server_shim.py)
class Tok:
    def encode(self, text):
        return list(text.encode())

    def token_to_id(self, token):
        return {"<|semantic:0|>": 1000, "<|semantic|>": 5}.get(token)


class FakeLM:
    def __init__(self, max_batch, per_slot_ok=True):
        self.cfg, self.max_batch, self.calls, self.per_slot_ok = dict(num_codebooks=8), max_batch, [], per_slot_ok
        self.gate = threading.Event()  # cleared: generate_blocking waits (holds the worker while a test queues its requests)
        self.gate.set()

    def clear_slow_layer_caches(self):
        pass

    def clear_slow_caches_until(self, pos):
        pass

    def curr_kv_size(self):
        return 0

    def generate_blocking(self, prompt, max_new_tokens, **kw):
        assert self.gate.wait(30)
        self.calls.append(("single", dict(kw)))
        return np.full((8, 4), 1, np.uint32)

    def generate_static_batch(self, prompts, max_new_tokens, **kw):
        self.calls.append(("batch", len(prompts)))
        return [np.full((8, 4), 2, np.uint32) for _ in prompts]

    def session(self, **kw):
        if kw.get("per_slot") and not self.per_slot_ok:
            raise RuntimeError("sessions need the MFMA row path")
        self.calls.append(("session", dict(kw)))
        return FakeSession(self)


class FakeSession:
    def __init__(self, lm):
        self.lm, self.slots = lm, {}

    def close(self):
        self.lm.calls.append(("session_end",))

    def add(self, prompt, max_new_tokens, **kw):
        free = [i for i in range(self.lm.max_batch) if i not in self.slots]
        if not free:
            return None
        self.slots[free[0]] = 0
        self.lm.calls.append(("add", dict(kw)))
        return free[0]

    def step(self, n):
        for k in self.slots:
            self.slots[k] += n
        return sum(v < 16 for v in self.slots.values())

    def poll(self, slot, codes=True):
        n = min(self.slots[slot], 16)
        return (np.full((8, n), 3, np.uint32), n == 16) if codes else (n, n == 16)

    def release(self, slot):
        del self.slots[slot]


class FakeCodec:
    def decode(self, codes):
        return np.full((codes.shape[0], 1, 2048 * codes.shape[2]), 0.25, np.float32)


def _state(per_slot_sampling, max_batch=16, continuous=True, **lm_kw):
    tok = Tok()
    enc = fprompt.PromptEncoder(tok, 8, fprompt.FISH_1_5)
    default = enc.encode_conditioning_prompt("hello there", np.full((8, 4), 3, np.uint32))
    lm = FakeLM(max_batch, **lm_kw)
    seeds = iter(range(100, 10000))
    ls = server.LMState(lm, tok, {"default": default}, default, max_new_tokens=64, max_batch=max_batch, seed_source=lambda: next(seeds))
    kw = dict(per_slot_sampling=True) if per_slot_sampling else {}
    return server.AppState(ls, FakeCodec(), batch_window_s=0.05, continuous=continuous, **kw), lm


def _post(state, **extra):
    status, ctype, body = server.generate_speech(state, dict(model="tts-1", voice="default", input="Some words to say.", **extra))
    return status, body


def _fire(state, reqs):
    """all requests queued before the worker looks at the first of them (it is held in a batch-1 call meanwhile): no request is
    'alone on the server' by an accident of thread timing"""
    import time
    lm = state.lm.lm
    lm.gate.clear()
    blocker = state.scheduler.submit(None, np.zeros((9, 6), np.uint32), 0, False)
    t0 = time.time()
    while state.scheduler.q.qsize() > 0 and time.time() - t0 < 10:  # the worker has taken the blocker
        time.sleep(0.005)
    out = [None] * len(reqs)

    def one(i):
        out[i] = _post(state, **reqs[i])

    ths = [threading.Thread(target=one, args=(i,)) for i in range(len(reqs))]
    for t in ths:
        t.start()
    t0 = time.time()
    while state.scheduler.q.qsize() < len(reqs) and time.time() - t0 < 10:
        time.sleep(0.005)
    lm.gate.set()
    for t in ths:
        t.join()
    blocker.result(timeout=30)
    return out


def test_default_off_nothing_changes():
    state, lm = _state(False)
    try:
        assert state.scheduler.per_slot_sampling is False and "per_slot_sessions" not in state.scheduler.stats
        # request-level fields are not read, chunks do not batch without batch_size: the batch-1 path with the server's settings
        assert _post(state, seed=5, temperature=0.1)[0] == 200
        assert [c[0] for c in lm.calls] == ["single"] and lm.calls[0][1]["temp"] == 0.7 and lm.calls[0][1]["seed"] == 100
        res = _fire(state, [dict(batch_size=2)] * 4)
        assert all(r[0] == 200 for r in res)
        sess = [c for c in lm.calls if c[0] == "session"]
        assert sess and all("per_slot" not in c[1] for c in sess)
        assert all(c[1] == {} for c in lm.calls if c[0] == "add")
    finally:
        state.scheduler.close()


def test_on_opens_a_per_slot_session_and_passes_seed_and_settings_per_job():
    state, lm = _state(True)
    try:
        res = _fire(state, [dict(), dict(seed=77, temperature=0.3), dict(top_k=40), dict()])
        assert all(r[0] == 200 for r in res), res
        sess = [c for c in lm.calls if c[0] == "session"]
        assert sess and all(c[1].get("per_slot") is True and c[1]["repetition_penalty"] == 1.4 for c in sess)
        assert state.scheduler.stats["per_slot_sessions"] == len(sess) >= 1
        adds = [c[1] for c in lm.calls if c[0] == "add"]
        assert all("seed" in a and a["sampling"]["repetition_penalty"] == 1.4 for a in adds)
        own = [a for a in adds if a["seed"] == 77]
        assert len(own) == 1 and own[0]["sampling"]["temp"] == 0.3 and own[0]["sampling"]["top_k"] == 256
        assert any(a["sampling"]["top_k"] == 40 and a["sampling"]["temp"] == 0.7 for a in adds)
        assert len({a["seed"] for a in adds}) == len(adds), "every job draws its own seed"
        assert not any(c[0] == "batch" for c in lm.calls)
        # a seeded request runs in the session even when it is alone: same kernels, same audio, whatever the load
        n = len(lm.calls)
        assert _post(state, seed=77, temperature=0.3)[0] == 200
        after = [c for c in lm.calls[n:] if c[0] in ("session", "add", "single")]  # (the idle worker may close the earlier session only now)
        assert [c[0] for c in after] == ["session", "add"] and after[1][1]["seed"] == 77
        # settings outside the per-slot samplers: alone on the batch-1 path, with the request's settings
        n = len(lm.calls)
        assert _post(state, top_k=0, seed=3)[0] == 200
        single = [c for c in lm.calls[n:] if c[0] == "single"]
        assert len(single) == 1 and single[0][1]["top_k"] == 0 and single[0][1]["seed"] == 3
        assert not any(c[0] == "add" for c in lm.calls[n:])
        assert _post(state, seed=-1)[0] == 500 and _post(state, temperature=-2)[0] == 500
    finally:
        state.scheduler.close()


def test_request_level_settings_never_reach_a_lock_step_sampler():
    # a handle that cannot open a per-slot session: the job runs alone instead of joining a lock-step session
    state, lm = _state(True, per_slot_ok=False)
    try:
        res = _fire(state, [dict(seed=5), dict(temperature=0.2), dict()])
        assert all(r[0] == 200 for r in res)
        assert not any(c[0] in ("session", "add", "batch") for c in lm.calls) and sum(c[0] == "single" for c in lm.calls) == 3 + 1  # (+ _fire's blocker)
    finally:
        state.scheduler.close()
    # the lock-step scheduler variant: jobs with their own settings are taken out of the batch (_batched never sees them)
    state, lm = _state(True, continuous=False)
    try:
        sch = state.scheduler
        seen = []
        orig = sch._batched
        sch._batched = lambda jobs: (seen.extend(jobs), orig(jobs))[1]
        res = _fire(state, [dict(seed=5), dict(), dict(), dict(temperature=0.2)])
        assert all(r[0] == 200 for r in res)
        assert all(j.sampling is None and j.seed is None for j in seen)
        own = [c for c in lm.calls if c[0] == "single" and (c[1]["seed"] == 5 or c[1]["temp"] == 0.2)]
        assert len(own) == 2
    finally:
        state.scheduler.close()
    # Scheduler.submit with settings on a scheduler without per-slot sampling: alone, never the plain session
    state, lm = _state(False)
    try:
        p = np.zeros((9, 6), np.uint32)
        futs = [state.scheduler.submit(None, p, 0, True, sampling=server.SamplingArgs(temp=0.1), seed=1)] + [state.scheduler.submit(None, p, 0, True) for _ in range(3)]
        for f in futs:
            f.result(timeout=30)
        assert all(c[1] == {} for c in lm.calls if c[0] == "add")
        assert any(c[0] == "single" and c[1]["temp"] == 0.1 and c[1]["seed"] == 1 for c in lm.calls)
    finally:
        state.scheduler.close()
