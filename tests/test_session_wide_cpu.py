"""CPU: FS_SESSION_WIDE_SAMPLER through the layers that need no GPU -- header, ctypes table and Session flags agree; the scheduler's
routing with the stand-in LM of tests/test_session_per_slot.py: with wide_sampling a nucleus-only (top_k = 0) and a top_k = 512 request
join the per-slot session, which was begun with the wide flag; without it both run alone, as before; a server whose DEFAULT settings are
nucleus-only gets a (wide) per-slot session instead of serving every request alone."""
import os
import re

import numpy as np
import pytest

from fishrt import _ffi, lm as flm, server
from test_session_per_slot import FakeCodec, FakeLM, Tok, _fire, _H, _post, _RecLib

from fishrt import prompt as fprompt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "fishrt.h")).read()


def test_header_and_ffi_table_agree():
    assert re.search(r"#define\s+FS_SESSION_WIDE_SAMPLER\s+32u", HEADER)
    assert _ffi.FS_SESSION_WIDE_SAMPLER == 32 and _ffi.FS_SESSION_PER_SLOT == 16
    m = re.search(r"int\s+fs_selftest_sample_slots\(([^;]*)\);", HEADER)
    assert m, "fs_selftest_sample_slots is not declared"
    args = [a.strip() for a in m.group(1).split(",")]
    assert args == ["int device_id", "const float* logits", "int S", "int R", "int n", "const fs_sampling* samplings", "const uint64_t* seeds",
                    "uint32_t* out", "uint64_t* words_used"]
    assert "fs_selftest_sample_slots" in _ffi.SYMBOLS


def test_session_wide_flag(monkeypatch):
    rec = _RecLib()
    monkeypatch.setattr(_ffi, "lib", lambda: rec)
    s = flm.Session(_H(), 0.7, 0.8, 0, 1, False, per_slot=True, repetition_penalty=1.4, wide=True)
    assert rec.calls[-1] == ("begin", 0.7, 0, 1.4, 16 | 32) and s.wide is True and s.per_slot is True
    s = flm.Session(_H(), 0.7, 0.8, 256, 1, True, per_slot=True, repetition_penalty=1.4)
    assert rec.calls[-1] == ("begin", 0.7, 256, 1.4, 1 | 16) and s.wide is False
    n = len(rec.calls)
    for kw in (dict(), dict(rows=True)):
        with pytest.raises(ValueError, match="per_slot=True"):
            flm.Session(_H(), 0.7, 0.8, 0, 1, False, wide=True, **kw)
    assert len(rec.calls) == n, "a refused session must not reach the library"


def _state(default=None, max_batch=16, **sched_kw):
    tok = Tok()
    enc = fprompt.PromptEncoder(tok, 8, fprompt.FISH_1_5)
    voice = enc.encode_conditioning_prompt("hello there", np.full((8, 4), 3, np.uint32))
    lm = FakeLM(max_batch)
    seeds = iter(range(100, 10000))
    ls = server.LMState(lm, tok, {"default": voice}, voice, max_new_tokens=64, max_batch=max_batch, seed_source=lambda: next(seeds),
                        default_sampling_args=default)
    return server.AppState(ls, FakeCodec(), batch_window_s=0.05, **sched_kw), lm


def test_wide_requests_join_the_per_slot_session():
    state, lm = _state(per_slot_sampling=True, wide_sampling=True)
    try:
        assert state.scheduler.wide_sampling is True and state.scheduler.stats["wide_sessions"] == 0
        res = _fire(state, [dict(), dict(top_k=0, seed=11), dict(top_k=512, seed=12, temperature=1.1), dict()])
        assert all(r[0] == 200 for r in res), res
        sess = [c[1] for c in lm.calls if c[0] == "session"]
        assert sess and all(k.get("per_slot") is True and k.get("wide") is True for k in sess), sess
        assert state.scheduler.stats["wide_sessions"] == state.scheduler.stats["per_slot_sessions"] == len(sess)
        adds = {a["seed"]: a["sampling"] for a in (c[1] for c in lm.calls if c[0] == "add")}
        assert adds[11]["top_k"] == 0 and adds[11]["temp"] == 0.7
        assert adds[12]["top_k"] == 512 and adds[12]["temp"] == 1.1
        single = [c for c in lm.calls if c[0] == "single"]
        assert len(single) == 1, "only _fire's blocker takes the batch-1 path"  # (it is submitted with allow_batch off)
        assert _post(state, temperature=-2)[0] == 500 and _post(state, top_k=-1)[0] == 500
    finally:
        state.scheduler.close()


def test_without_the_option_wide_requests_run_single():
    state, lm = _state(per_slot_sampling=True)
    try:
        assert state.scheduler.wide_sampling is False and "wide_sessions" not in state.scheduler.stats
        res = _fire(state, [dict(), dict(top_k=0, seed=11), dict(top_k=512, seed=12), dict()])
        assert all(r[0] == 200 for r in res), res
        sess = [c[1] for c in lm.calls if c[0] == "session"]
        assert sess and all("wide" not in k for k in sess)
        single = {c[1]["seed"]: c[1] for c in lm.calls if c[0] == "single"}
        assert single[11]["top_k"] == 0 and single[12]["top_k"] == 512
        assert not any(c[0] == "add" and c[1].get("seed") in (11, 12) for c in lm.calls)
    finally:
        state.scheduler.close()


def test_wide_sampling_needs_per_slot_sampling():
    tok = Tok()
    ls = server.LMState(FakeLM(16), tok, {}, None, max_batch=16)
    with pytest.raises(ValueError, match="per_slot_sampling"):
        server.Scheduler(ls, wide_sampling=True)
    with pytest.raises(ValueError, match="per_slot_sampling"):
        server.AppState(ls, FakeCodec(), wide_sampling=True)


def test_row_session_handles_keep_their_limit():
    """max_batch 2 / 4 / 8 on Fish 1.5: the handle's sessions are row sessions; a job outside the row kernels' samplers still runs alone"""
    state, lm = _state(per_slot_sampling=True, wide_sampling=True, max_batch=4)
    lm.rows_supported = lambda n, **kw: True
    try:
        res = _fire(state, [dict(), dict(top_k=0, seed=11), dict()])
        assert all(r[0] == 200 for r in res), res
        assert any(c[0] == "single" and c[1]["seed"] == 11 and c[1]["top_k"] == 0 for c in lm.calls)
        assert not any(c[0] == "add" and c[1].get("seed") == 11 for c in lm.calls)
        sess = [c[1] for c in lm.calls if c[0] == "session"]
        assert sess and all(k.get("rows") is True and "wide" not in k for k in sess)
    finally:
        state.scheduler.close()


def test_nucleus_only_server_defaults_open_a_wide_per_slot_session():
    default = server.SamplingArgs(temp=0.7, top_p=0.8, top_k=0, repetition_penalty=1.2)  # upstream Fish-Speech: no top-k at all

    class StrictLM(FakeLM):  # a per-slot session refuses settings outside its samplers unless it is a wide one, like the library
        def session(self, **kw):
            if kw.get("per_slot") and not kw.get("wide") and not (kw["temp"] == 0 or 0 < kw["top_k"] <= 256):
                raise RuntimeError("FS_SESSION_PER_SLOT: ... 0 < top_k <= 256 ...")
            return FakeLM.session(self, **kw)

    for wide in (True, False):
        state, lm = _state(default=default, per_slot_sampling=True, **(dict(wide_sampling=True) if wide else {}))
        lm.__class__ = StrictLM
        try:
            res = _fire(state, [dict(), dict(), dict(seed=5)])
            assert all(r[0] == 200 for r in res), res
            sess = [c[1] for c in lm.calls if c[0] == "session"]
            adds = [c[1] for c in lm.calls if c[0] == "add"]
            single = [c for c in lm.calls if c[0] == "single"]
            if wide:
                assert sess and all(k.get("wide") is True and k["top_k"] == 0 for k in sess)
                assert len(adds) == 3 and all(a["sampling"]["top_k"] == 0 for a in adds) and len(single) == 1  # (the blocker)
            else:  # today's behaviour: no session can be opened, every request is served alone
                assert not sess and not adds and len(single) == 3 + 1
        finally:
            state.scheduler.close()
