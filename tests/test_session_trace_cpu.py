"""CPU: FS_SESSION_TRACE through the layers that need no GPU -- the header defines the flag and both prototypes, the ctypes table agrees,
and fishrt.lm.Session raises its flag, shape and argument errors before the library is called (a recording stand-in for the library, as
tests/test_session_score_cpu.py uses)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from fishrt import _ffi, lm as flm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "fishrt.h")).read()


def _args(name):
    m = re.search(r"int\s+" + name + r"\(([^;]*)\);", HEADER)
    assert m, f"{name} is not declared"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_and_ffi_table_agree():
    assert re.search(r"#define\s+FS_SESSION_TRACE\s+128u", HEADER)
    assert _ffi.FS_SESSION_TRACE == 128 and _ffi.FS_SESSION_SCORE == 64 and _ffi.FS_SESSION_PER_SLOT == 16
    protos = {
        "fs_lm_session_add_traced": ["fs_lm_t* lm", "int prefix_id", "const uint32_t* prompt", "int L", "int max_new_tokens",
                                     "const fs_sampling* sampling", "const uint64_t* seed", "int collect_hidden", "int* slot"],
        "fs_lm_session_poll_trace": ["fs_lm_t* lm", "int slot", "size_t first_row", "uint32_t* tokens", "float* logprob", "float* top_logprob",
                                     "uint32_t* top", "float* eos_logprob", "int* n_decisions", "size_t cap_rows", "size_t* n_rows"],
    }
    ctype_of = {"int": C.c_int, "size_t": C.c_size_t, "fs_lm_t*": C.c_void_p, "const uint32_t*": C.POINTER(C.c_uint32),
                "uint32_t*": C.POINTER(C.c_uint32), "float*": C.POINTER(C.c_float), "int*": C.POINTER(C.c_int),
                "size_t*": C.POINTER(C.c_size_t), "const fs_sampling*": C.c_void_p, "const uint64_t*": C.POINTER(C.c_uint64)}
    for name, want in protos.items():
        assert _args(name) == want, name
        assert name in _ffi.SYMBOLS
        assert _ffi.TRACE_PROTOTYPES[name] == [ctype_of[a.rsplit(" ", 1)[0]] for a in want], name
    assert "FS_SESSION_TRACE" in _args("fs_lm_session_begin")[-1], "the flag list of fs_lm_session_begin names the new flag"


class _RecLib:
    """records the calls a fishrt.lm.Session makes instead of running them"""

    def __init__(self):
        self.calls = []

    def fs_lm_session_begin(self, h, s, seed, flags):
        self.calls.append(("begin", int(flags)))
        return 0

    def fs_lm_session_end(self, h):
        return 0

    def fs_lm_session_add_traced(self, h, pid, p, L, max_new, samp, seed, hid, slot):
        self.calls.append(("add_traced", pid, L, max_new, None if samp is None else round(float(samp._obj.temp), 3),
                           None if seed is None else int(seed._obj.value), hid))
        slot._obj.value = 5
        return 0

    def fs_lm_session_add_ex(self, h, pid, p, L, max_new, samp, seed, slot):
        self.calls.append(("add_ex", pid, L, max_new))
        slot._obj.value = 6
        return 0

    def fs_lm_session_poll_trace(self, h, slot, first, tok, lp, tlp, top, eos, nd, cap, n):
        self.calls.append(("poll_trace", slot, int(first.value), int(cap.value), tok is None))
        n._obj.value = 4
        return 0


class _H:
    cfg = dict(num_codebooks=8, dim=1024)
    _h = None


def test_session_trace_flag(monkeypatch):
    rec = _RecLib()
    monkeypatch.setattr(_ffi, "lib", lambda: rec)
    s = flm.Session(_H(), 0.0, 1.0, 0, 1, False, per_slot=True, score=True, trace=True)
    assert rec.calls[-1] == ("begin", 16 | 64 | 128) and s.trace is True and s.score is True
    s = flm.Session(_H(), 0.7, 0.8, 0, 1, True, per_slot=True, wide=True, score=True, trace=True)
    assert rec.calls[-1] == ("begin", 1 | 16 | 32 | 64 | 128)
    s = flm.Session(_H(), 0.7, 0.8, 256, 1, False, per_slot=True, score=True)
    assert rec.calls[-1] == ("begin", 16 | 64) and s.trace is False, "a score session without the flag keeps its flags"
    n = len(rec.calls)
    for kw in (dict(), dict(per_slot=True), dict(rows=True), dict(per_slot=True, wide=True)):
        with pytest.raises(ValueError, match="per_slot=True and score=True"):
            flm.Session(_H(), 0.7, 0.8, 0, 1, False, trace=True, **kw)
    with pytest.raises(ValueError, match="per_slot=True"):  # (score without per_slot is refused as before)
        flm.Session(_H(), 0.7, 0.8, 0, 1, False, score=True, trace=True)
    assert len(rec.calls) == n, "a refused session must not reach the library"


def test_add_and_poll_errors_never_reach_the_library(monkeypatch):
    rec = _RecLib()
    monkeypatch.setattr(_ffi, "lib", lambda: rec)
    s = flm.Session(_H(), 0.7, 0.8, 256, 1, False, per_slot=True, score=True, trace=True)
    p = np.zeros((9, 5), np.uint32)
    assert s.add(p, 11, trace=True) == 5 and rec.calls[-1] == ("add_traced", -1, 5, 11, None, None, 0)
    assert s.add(p[:, :2], 7, prefix=3, sampling=dict(temp=0.0), seed=9, collect_hidden=True, trace=True) == 5
    assert rec.calls[-1] == ("add_traced", 3, 2, 7, 0.0, 9, 1)
    assert s.add(p, 11, seed=2) == 6 and rec.calls[-1][0] == "add_ex", "an add without trace=True takes the entry point it always took"
    r = s.poll_trace(5, first=1)
    assert rec.calls[-2:] == [("poll_trace", 5, 0, 0, True), ("poll_trace", 5, 1, 3, False)]
    assert r["tokens"].shape == r["logprob"].shape == r["top_logprob"].shape == r["top"].shape == (3, 9)
    assert r["eos_logprob"].shape == r["n_decisions"].shape == (3,)
    assert r["tokens"].dtype == r["top"].dtype == np.uint32 and r["logprob"].dtype == np.float32 and r["n_decisions"].dtype == np.int32
    n = len(rec.calls)
    with pytest.raises(ValueError, match="prompt"):
        s.add(np.zeros((8, 5), np.uint32), 11, trace=True)
    with pytest.raises(ValueError, match="unknown sampling"):
        s.add(p, 11, sampling=dict(temperature=1.0), trace=True)
    with pytest.raises(ValueError, match="seed"):
        s.add(p, 11, seed=-1, trace=True)
    with pytest.raises(ValueError, match="first"):
        s.poll_trace(5, first=-1)
    for kw in (dict(per_slot=True, score=True), dict(per_slot=True), dict()):
        other = flm.Session(_H(), 0.7, 0.8, 256, 1, False, **kw)
        m = len(rec.calls)
        with pytest.raises(ValueError, match="trace=True"):
            other.add(p, 11, trace=True)
        with pytest.raises(ValueError, match="trace=True"):
            other.poll_trace(0)
        assert len(rec.calls) == m, "a refused call must not reach the library"
    assert len(rec.calls) == n + 3  # (the three sessions begun above)


def test_generate_traced_checks_its_lists_before_it_opens_a_session(monkeypatch):
    rec = _RecLib()
    monkeypatch.setattr(_ffi, "lib", lambda: rec)
    p = np.zeros((9, 5), np.uint32)
    with pytest.raises(ValueError, match="2 prompts"):
        flm.DualARTransformer.generate_traced(_H(), [p, p], [8, 8, 8])
    with pytest.raises(ValueError, match="2 prompts"):
        flm.DualARTransformer.generate_traced(_H(), [p, p], 8, seeds=[1])
    assert rec.calls == []
