"""CPU: prefixes from a slot's history (fs_lm_session_prefix_from_slot) without a GPU -- the page book under the promotion's operations
(tools/kv_history_check.cpp: scripted cases and a random walk against a naive model, built with the host compiler and run; no sanitizer
flags here, the ASan / UBSan build is the command in the program's header, run by hand as a stand-alone program), the argument checks of
Session.prefix_from_slot / continue_from and DualARTransformer.generate_turns, and the server's chunk_history option driven through
stand-ins that record how they are called (admission order, body columns, budget arithmetic, fallback, releases)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from fishrt import lm as flm
from fishrt import prompt as fprompt
from fishrt import server
from test_server_shim import FakeCodec, Tok

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kv_history_host_check(tmp_path):
    cxx = shutil.which("c++") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "kv_history_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tools", "kv_history_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout
    assert r.stdout.splitlines()[-1:] == ["kv_history_check ok"], r.stdout


class _NoHandle:
    cfg = dict(num_codebooks=8, max_seq_len=256)
    _h = None


def _session(rows=False):
    s = object.__new__(flm.Session)  # no handle: reaching the C call would fail with something other than ValueError
    s.lm, s.rows, s.per_slot, s._open = _NoHandle(), rows, not rows, False
    return s


def test_session_argument_checks():
    s = _session()
    for bad in (0, -1, -5, 1.5, True, "3"):
        with pytest.raises((ValueError, TypeError)):
            s.prefix_from_slot(0, bad)
    with pytest.raises(ValueError, match="FS_SESSION_ROWS"):
        _session(rows=True).prefix_from_slot(0)
    with pytest.raises(ValueError, match="no prefix argument"):
        s.continue_from(0, np.zeros((9, 2), np.uint32), 10, prefix=1)
    for body in (np.zeros((8, 2), np.uint32), np.zeros(9, np.uint32)):
        with pytest.raises(ValueError, match="body must be u32"):
            s.continue_from(0, body, 10)


def test_generate_turns_argument_checks():
    lm = object.__new__(flm.DualARTransformer)
    lm.cfg, lm._h = dict(num_codebooks=8, max_seq_len=256), None
    ok = np.zeros((9, 4), np.uint32)
    with pytest.raises(ValueError, match=r"bodies\[1\]"):
        lm.generate_turns(ok, [ok, np.zeros((9, 0), np.uint32)], 10)
    with pytest.raises(ValueError, match="cond"):
        lm.generate_turns(np.zeros((8, 4), np.uint32), [ok], 10)
    with pytest.raises(ValueError, match="between"):
        lm.generate_turns(ok, [ok], 10, between=np.zeros(3, np.uint32))
    with pytest.raises(ValueError, match="max_new_tokens"):
        lm.generate_turns(ok, [ok], 0)


# ---- the server's chunk_history option
class TurnLM:
    """stand-in handle: batch-1 calls and per-slot sessions, every call recorded"""

    def __init__(self, max_new_tokens=40, max_seq_len=4096):
        self.cfg = dict(num_codebooks=8, max_seq_len=max_seq_len)
        self.calls, self.M = [], max_new_tokens

    def frames(self, prompt):  # 3 .. 7 frames, a function of the request
        return 3 + prompt.shape[1] % 5

    def clear_slow_layer_caches(self):
        pass

    def clear_slow_caches_until(self, pos):
        pass

    def curr_kv_size(self):
        return 0

    def generate_blocking(self, prompt, max_new_tokens, **kw):
        self.calls.append(("single", prompt.copy(), max_new_tokens))
        return np.full((8, self.frames(prompt)), 7, np.uint32)

    def session(self, **kw):
        self.calls.append(("session", dict(kw)))
        return TurnSession(self)


class TurnSession:
    """stand-in for fishrt.lm.Session with Session.continue_from's contract: the whole history of a DONE slot becomes a prefix, the new
    slot's body is [last frame's column, body...], and the session's reference on the prefix is dropped once the add is queued"""

    def __init__(self, lm):
        self.lm, self.slots, self.prefixes, self.n_prefixes = lm, {}, set(), 0

    def close(self):
        self.lm.calls.append(("session_end", len(self.slots), len(self.prefixes)))

    def _admit(self, total_len, n_frames, tag):
        free = [i for i in range(4) if i not in self.slots]
        if not free:
            return None
        # [frames, emitted so far, total prompt length]; frame k of the slot holds 100 * slot tag + k in every codebook
        self.slots[free[0]] = [np.full((8, n_frames), 0, np.uint32) + np.arange(n_frames, dtype=np.uint32)[None] + np.uint32(100 * tag), 0, total_len]
        return free[0]

    def add(self, prompt, max_new_tokens, prefix=None, sampling=None, seed=None, collect_hidden=False):
        assert prefix is None and sampling is not None and seed is not None
        slot = self._admit(prompt.shape[1], self.lm.frames(prompt), len(self.lm.calls))
        self.lm.calls.append(("add", slot, prompt.copy(), max_new_tokens))
        return slot

    def last_frame(self, slot):
        full, n, _ = self.slots[slot]
        assert n >= 1
        return np.concatenate([[np.uint32(2000) + full[0, n - 1]], full[:, n - 1]]).astype(np.uint32)

    def continue_from(self, slot, body, max_new_tokens, **kw):
        full, n, L = self.slots[slot]
        assert n == full.shape[1], "the next turn was admitted before the slot was done"
        assert kw.get("sampling") is not None and kw.get("seed") is not None
        pid = self.n_prefixes
        self.n_prefixes += 1
        self.prefixes.add(pid)
        whole = np.concatenate([self.last_frame(slot)[:, None], body], 1)
        hist = L + n - 1
        new = self._admit(hist + whole.shape[1], self.lm.frames(whole), len(self.lm.calls))
        self.prefixes.discard(pid)  # (dropped once the add is queued)
        self.lm.calls.append(("continue", slot, new, whole.copy(), max_new_tokens, hist))
        return (new, pid) if new is not None else (None, None)

    def step(self, n):
        live = 0
        for v in self.slots.values():
            v[1] = min(v[0].shape[1], v[1] + n)
            live += v[1] < v[0].shape[1]
        return live

    def poll(self, slot, codes=True):
        full, n, _ = self.slots[slot]
        return (full[:, :n].copy(), n == full.shape[1]) if codes else (n, n == full.shape[1])

    def release(self, slot):
        self.lm.calls.append(("release", slot))
        del self.slots[slot]


TEXT = "The first chunk of the request.|And the second one follows it, a little longer.|A third one closes it."  # (chunks: split at |)


def _turn_state(**lm_kw):
    tok = Tok()
    enc = fprompt.PromptEncoder(tok, 8, fprompt.FISH_1_5)
    default = enc.encode_conditioning_prompt("hello there", np.full((8, 4), 3, np.uint32))
    lm = TurnLM(**lm_kw)
    seeds = iter(range(1000, 2000))
    ls = server.LMState(lm, tok, {"default": default}, default, max_new_tokens=lm.M, max_batch=8, seed_source=lambda: next(seeds))
    return server.AppState(ls, FakeCodec(), per_slot_sampling=True, chunk_history=True, preprocess=lambda t: t.split("|")), lm, enc


def _parts(state, enc):
    """the request's chunks as the server encodes them: (conditioning columns, [body per chunk], the columns that close a turn)"""
    n_cond, cond, bodies = server._prompts_for_request(state, dict(voice="default", input=TEXT))
    assert len(bodies) == 3 and n_cond == cond.shape[1]
    return cond, bodies, enc.tokenize_text("<|im_end|>")


def test_chunk_history_needs_the_per_slot_continuous_scheduler():
    ls = server.LMState(TurnLM(), Tok(), {}, None, max_batch=8)
    with pytest.raises(ValueError, match="chunk_history"):
        server.AppState(ls, FakeCodec(), chunk_history=True)
    with pytest.raises(ValueError, match="chunk_history"):
        server.AppState(ls, FakeCodec(), chunk_history=True, per_slot_sampling=True, continuous=False)


def test_chunks_run_as_turns_on_the_history_of_the_chunk_before():
    state, lm, enc = _turn_state()
    cond, bodies, sep = _parts(state, enc)
    status, ctype, body = server.generate_speech(state, dict(model="x", voice="default", input=TEXT))
    state.scheduler.close()
    assert status == 200 and ctype == "audio/wav"
    M = lm.M
    adds = [k for k in lm.calls if k[0] == "add"]
    turns = [k for k in lm.calls if k[0] == "continue"]
    assert len(adds) == 1 and len(turns) == 2 and not [k for k in lm.calls if k[0] == "single"]
    # chunk 0: the conditioning and its body, the server's budget
    assert np.array_equal(adds[0][2], np.concatenate([cond, bodies[0]], 1)) and adds[0][3] == M
    L_prev, src = adds[0][2].shape[1], adds[0][1]
    for i, (_, slot, new, whole, mnt, hist) in enumerate(turns, 1):
        n_prev = lm.frames(adds[0][2]) if i == 1 else lm.frames(turns[i - 2][3])
        # admitted on the slot of the chunk before it (TurnSession asserts that slot was done), on all of its history
        assert slot == src and hist == L_prev + n_prev - 1
        # the body: the last frame's column, <|im_end|>, the user turn, the assistant's opening
        last = whole[:, 0]
        assert last[0] == 2000 + last[1] and last[1] % 100 == n_prev - 1
        assert np.array_equal(whole[:, 1:], np.concatenate([sep, enc.encode_text("user", state.preprocess(TEXT)[i]), enc.encode_vq(None)], 1))
        assert np.array_equal(whole[:, 1 + sep.shape[1]:], bodies[i])
        # the budget: the frames the chunk would have had on the conditioning alone
        L_turn, L_plain = hist + whole.shape[1], cond.shape[1] + bodies[i].shape[1]
        assert mnt == M + (L_turn - L_plain)
        assert 1 + max(0, mnt - L_turn + 1) == 1 + max(0, M - L_plain + 1)
        L_prev, src = L_turn, new
    # the old slot goes right after its turn has been queued; every slot and prefix is released at the end
    order = [k[0] for k in lm.calls if k[0] in ("add", "continue", "release")]
    assert order == ["add", "continue", "release", "continue", "release", "release"]
    ends = [k for k in lm.calls if k[0] == "session_end"]
    assert len(ends) == 1 and ends[0][1:] == (0, 0)
    st = state.scheduler.stats
    assert st["history_turns"] == 2 and st["history_fallbacks"] == 0 and st["jobs"] == 3
    # the audio: three chunks, in order
    n_frames = lm.frames(adds[0][2]) + sum(lm.frames(t[3]) for t in turns)
    assert len(body) == 44 + 2 * 2048 * n_frames


def test_a_turn_that_does_not_fit_falls_back_to_the_conditioning_alone():
    probe_state, probe_lm, enc = _turn_state()
    cond, bodies, sep = _parts(probe_state, enc)
    probe_state.scheduler.close()
    M = probe_lm.M
    L0 = cond.shape[1] + bodies[0].shape[1]
    hist1 = L0 + probe_lm.frames(np.concatenate([cond, bodies[0]], 1)) - 1
    L1 = hist1 + 1 + sep.shape[1] + bodies[1].shape[1]
    need1 = L1 + max(0, M - (cond.shape[1] + bodies[1].shape[1]) + 1)
    # max_seq_len holds turn 1 exactly; turn 2 would sit on a longer history and does not fit
    state, lm, enc = _turn_state(max_seq_len=need1)
    status, _, _ = server.generate_speech(state, dict(model="x", voice="default", input=TEXT))
    state.scheduler.close()
    assert status == 200
    turns = [k for k in lm.calls if k[0] == "continue"]
    assert len(turns) == 1 and turns[0][5] == hist1
    # the third chunk ran on the conditioning alone (a lone job: the batch-1 path), with the plain budget
    singles = [k for k in lm.calls if k[0] == "single"]
    assert len(singles) == 1 and np.array_equal(singles[0][1], np.concatenate([cond, bodies[2]], 1)) and singles[0][2] == M
    st = state.scheduler.stats
    assert st["history_turns"] == 1 and st["history_fallbacks"] == 1
    assert all(k[1:] == (0, 0) for k in lm.calls if k[0] == "session_end")


def test_requests_share_the_session_and_a_refused_turn_falls_back():
    """two requests of three chunks each in flight together: their turns are slots of one session; when the stand-in has no free slot for a
    turn (4 slots, held by other requests' chunks) the chunk falls back instead of waiting on its history"""
    import threading
    state, lm, enc = _turn_state()
    out = {}

    def go(i):
        out[i] = server.generate_speech(state, dict(model="x", voice="default", input=TEXT))

    ths = [threading.Thread(target=go, args=(i,)) for i in range(3)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    state.scheduler.close()
    assert all(v[0] == 200 for v in out.values())
    st = state.scheduler.stats
    assert st["jobs"] == 9 and st["history_turns"] + st["history_fallbacks"] == 6, st
    assert all(k[1:] == (0, 0) for k in lm.calls if k[0] == "session_end")
    # every turn was admitted on a slot that was done, and released afterwards
    for i, k in enumerate(lm.calls):
        if k[0] == "continue":
            assert ("release", k[1]) in [c[:2] for c in lm.calls[i + 1:]]
