"""CPU: Fish <= 1.4 handles in per-slot sessions through the layers that need no GPU -- the Python Session passes FS_SESSION_PER_SLOT for
a legacy handle unchanged (the C side decides, not the wrapper); the scheduler opens a per-slot session for a Fish-1.4 LMState when
per_slot_sampling is on -- without trying the row kernels first -- and never otherwise; results keep the codes - 1 shift and the "code 0"
error; the header and the documents state which session kind takes which token layout."""
import os
import threading

import numpy as np
import pytest

from fishrt import _ffi, config as fcfg, lm as flm, prompt as fprompt, server
from test_session_per_slot import FakeCodec, FakeSession, Tok, _fire, _post, _RecLib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _LegacyHandle:
    cfg = dict(fcfg.FISH_1_4)
    token_cfg = dict(fcfg.FISH_1_4_TOKENS)
    _h = None


def test_session_passes_per_slot_flags_for_a_legacy_handle_unchanged(monkeypatch):
    rec = _RecLib()
    monkeypatch.setattr(_ffi, "lib", lambda: rec)
    s = flm.Session(_LegacyHandle(), 0.7, 0.8, 256, 1, True, per_slot=True, repetition_penalty=1.2)
    assert rec.calls[-1] == ("begin", 0.7, 256, 1.2, 1 | 16)
    assert s.add(np.zeros((9, 5), np.uint32), 20, sampling=dict(temp=0.0), seed=7) == 2
    assert rec.calls[-1] == ("add_ex", -1, 5, 20, (0.0, 0.8, 256, 1.2), 7)
    flm.Session(_LegacyHandle(), 0.7, 0.8, 256, 1, False)  # a plain session reaches the library too: the refusal is the C side's
    assert rec.calls[-1] == ("begin", 0.7, 256, 1.0, 0)


class LegacyFakeLM:
    """stand-in for a Fish <= 1.4 handle with 8 slots: only per_slot sessions open (the C side's rule); generate_multi would serve it, so
    rows_supported says yes -- exactly what made the scheduler try a row session first"""

    def __init__(self, code=3):
        self.cfg, self.max_batch, self.calls, self.code = dict(num_codebooks=8), 8, [], code
        self.gate = threading.Event()
        self.gate.set()

    def clear_slow_layer_caches(self):
        pass

    def clear_slow_caches_until(self, pos):
        pass

    def curr_kv_size(self):
        return 0

    def rows_supported(self, n, **kw):
        self.calls.append(("rows_supported", n))
        return True

    def generate_blocking(self, prompt, max_new_tokens, **kw):
        assert self.gate.wait(30)
        self.calls.append(("single", dict(kw)))
        return np.full((8, 4), 3, np.uint32)  # (`code` is what the SESSION's slots return)

    def session(self, **kw):
        self.calls.append(("session", dict(kw)))
        if not kw.get("per_slot"):
            raise RuntimeError("plain and FS_SESSION_ROWS sessions need the Fish 1.5 token layout; Fish <= 1.4 handles take FS_SESSION_PER_SLOT")
        fs = FakeSession(self)
        poll = fs.poll
        fs.poll = lambda slot, codes=True: ((np.full_like(poll(slot)[0], self.code), poll(slot)[1]) if codes else poll(slot, False))
        return fs


def _state(per_slot_sampling, **lm_kw):
    tok = Tok()
    enc = fprompt.PromptEncoder(tok, 8, fprompt.FISH_1_4)
    default = enc.encode_conditioning_prompt("hello there", np.full((8, 4), 3, np.uint32))
    lm = LegacyFakeLM(**lm_kw)
    seeds = iter(range(100, 10000))
    ls = server.LMState(lm, tok, {"default": default}, default, model_type=fprompt.FISH_1_4, max_new_tokens=64, max_batch=8,
                        seed_source=lambda: next(seeds))
    kw = dict(per_slot_sampling=True) if per_slot_sampling else {}
    return server.AppState(ls, FakeCodec(), batch_window_s=0.05, **kw), lm


def test_scheduler_opens_a_per_slot_session_for_fish14_when_asked():
    state, lm = _state(True)
    try:
        res = _fire(state, [dict(), dict(seed=77, temperature=0.0), dict(top_k=40), dict()])
        assert all(r[0] == 200 for r in res), res
        sess = [c[1] for c in lm.calls if c[0] == "session"]
        assert sess and all(k.get("per_slot") is True and not k.get("rows") and k["repetition_penalty"] == 1.2 for k in sess), sess
        assert not any(c[0] == "rows_supported" for c in lm.calls), "a Fish <= 1.4 handle has no row sessions to ask for"
        assert state.scheduler.stats["per_slot_sessions"] == len(sess) >= 1 and "row_sessions" not in state.scheduler.stats
        adds = [c[1] for c in lm.calls if c[0] == "add"]
        assert len(adds) == 4 and all("seed" in a and a["sampling"]["repetition_penalty"] == 1.2 for a in adds)
        # a greedy request joins the session of a sampled server default: per-slot sessions mix both, also at 8 slots
        own = [a for a in adds if a["seed"] == 77]
        assert len(own) == 1 and own[0]["sampling"]["temp"] == 0.0
    finally:
        state.scheduler.close()


def test_scheduler_never_opens_one_otherwise():
    state, lm = _state(False)
    try:
        res = _fire(state, [dict(), dict(seed=5), dict()])
        assert all(r[0] == 200 for r in res), res
        assert not any(c[0] == "session" and c[1].get("per_slot") for c in lm.calls)
        assert sum(c[0] == "single" for c in lm.calls) == 3 + 1  # (+ _fire's blocker): one after the other, as before
        assert "per_slot_sessions" not in state.scheduler.stats
    finally:
        state.scheduler.close()


def test_result_applies_the_shift_and_raises_on_code_zero():
    state, lm = _state(True)
    try:
        sch = state.scheduler
        j = server._Job(None, np.zeros((9, 6), np.uint32), 0, True)
        codes = np.arange(1, 17, dtype=np.uint32).reshape(8, 2)
        assert np.array_equal(sch._result(j, codes, None), codes - 1)
        jh = server._Job(None, np.zeros((9, 6), np.uint32), 0, True, collect_hidden=True)
        out, hid = sch._result(jh, codes, np.ones((3, 1, 4), np.float32))
        assert np.array_equal(out, codes - 1) and hid.shape == (3, 4)
        with pytest.raises(RuntimeError, match="code 0"):
            sch._result(j, np.zeros((8, 1), np.uint32), None)
    finally:
        state.scheduler.close()
    # through the session path: a slot whose codes hold a 0 fails its request with that message, the others are served
    state, lm = _state(True, code=0)
    try:
        res = _fire(state, [dict(), dict()])
        assert all(r[0] == 500 and b"code 0" in r[1] for r in res), res
    finally:
        state.scheduler.close()


def test_header_and_documents_state_the_token_layout_rule():
    header = open(os.path.join(ROOT, "include", "fishrt.h")).read()
    block = header[header.index("continuous batching"):header.index("int fs_lm_session_begin")]
    assert "Fish <= 1.4" in block and "FS_SESSION_PER_SLOT sessions only" in block
    assert "ONE stream word per live frame" in block and "greedy" in block
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "Fish <= 1.4" in integ[integ.index("### Per-request sampling from C / Rust"):integ.index("### Hidden states of session slots")]
    src = open(os.path.join(ROOT, "fish-speech.rs_amd", "csrc", "lm_engine.hip")).read()
    assert "Fish <= 1.4 handles take FS_SESSION_PER_SLOT" in src
