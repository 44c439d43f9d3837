"""CPU: FS_SESSION_SCORE through the layers that need no GPU -- header, ctypes table and Session flags agree; Session.add_scored's shape
errors never reach the library; and the f64 referee the GPU tests hold the score node to (ref_scores: log-softmax of a row at its target
and at its maximum, the LAST maximal index) agrees with torch.log_softmax in f64."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from fishrt import _ffi, lm as flm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "fishrt.h")).read()


def ref_scores(row, target, exclude0=False):
    """numpy f64 referee of one decision -> (logprob, top_logprob, top, eos_logprob): log-softmax of `row` at `target` and at its maximum,
    the LAST index holding the maximum (-0 == +0), log-softmax at candidate 0; exclude0: candidate 0 takes no part (-inf)"""
    x = np.asarray(row, np.float64).copy()
    if exclude0:
        x[0] = -np.inf
    m = x.max()
    top = int(np.nonzero(x == m)[0][-1])
    ls = np.log(np.exp(x - m).sum())
    return float((x[target] - m) - ls), float(-ls), top, float((x[0] - m) - ls)


def _args(name):
    m = re.search(r"int\s+" + name + r"\(([^;]*)\);", HEADER)
    assert m, f"{name} is not declared"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_and_ffi_table_agree():
    assert re.search(r"#define\s+FS_SESSION_SCORE\s+64u", HEADER)
    assert _ffi.FS_SESSION_SCORE == 64 and _ffi.FS_SESSION_PER_SLOT == 16
    protos = {
        "fs_lm_session_add_scored": ["fs_lm_t* lm", "int prefix_id", "const uint32_t* prompt", "int L", "const uint32_t* frames", "int N",
                                     "int collect_hidden", "int* slot"],
        "fs_lm_session_poll_scores": ["fs_lm_t* lm", "int slot", "size_t first_row", "float* logprob", "float* top_logprob", "uint32_t* top",
                                      "float* eos_logprob", "size_t cap_rows", "size_t* n_rows"],
        "fs_selftest_score_rows": ["int device_id", "const float* logits", "int S", "int n", "const uint32_t* targets", "int exclude0",
                                   "float* logprob_out", "float* top_logprob_out", "uint32_t* top_out", "float* row_out"],
    }
    ctype_of = {"int": C.c_int, "size_t": C.c_size_t, "fs_lm_t*": C.c_void_p, "const uint32_t*": C.POINTER(C.c_uint32),
                "uint32_t*": C.POINTER(C.c_uint32), "const float*": C.POINTER(C.c_float), "float*": C.POINTER(C.c_float),
                "int*": C.POINTER(C.c_int), "size_t*": C.POINTER(C.c_size_t)}
    for name, want in protos.items():
        assert _args(name) == want, name
        assert name in _ffi.SYMBOLS
        assert _ffi.SCORE_PROTOTYPES[name] == [ctype_of[a.rsplit(" ", 1)[0]] for a in want], name


class _RecLib:
    """records the calls a fishrt.lm.Session makes instead of running them"""

    def __init__(self):
        self.calls = []

    def fs_lm_session_begin(self, h, s, seed, flags):
        self.calls.append(("begin", int(flags)))
        return 0

    def fs_lm_session_end(self, h):
        return 0

    def fs_lm_session_add_scored(self, h, pid, p, L, f, N, hid, slot):
        self.calls.append(("add_scored", pid, L, N, hid))
        slot._obj.value = 3
        return 0


class _H:
    cfg = dict(num_codebooks=8, dim=1024)
    _h = None


def test_session_score_flag(monkeypatch):
    rec = _RecLib()
    monkeypatch.setattr(_ffi, "lib", lambda: rec)
    s = flm.Session(_H(), 0.0, 1.0, 0, 1, False, per_slot=True, score=True)
    assert rec.calls[-1] == ("begin", 16 | 64) and s.score is True and s.per_slot is True
    s = flm.Session(_H(), 0.7, 0.8, 0, 1, True, per_slot=True, wide=True, score=True)
    assert rec.calls[-1] == ("begin", 1 | 16 | 32 | 64)
    s = flm.Session(_H(), 0.7, 0.8, 256, 1, False, per_slot=True)
    assert rec.calls[-1] == ("begin", 16) and s.score is False
    n = len(rec.calls)
    for kw in (dict(), dict(rows=True)):
        with pytest.raises(ValueError, match="per_slot=True"):
            flm.Session(_H(), 0.7, 0.8, 0, 1, False, score=True, **kw)
    assert len(rec.calls) == n, "a refused session must not reach the library"


def test_add_scored_shape_errors_never_reach_the_library(monkeypatch):
    rec = _RecLib()
    monkeypatch.setattr(_ffi, "lib", lambda: rec)
    s = flm.Session(_H(), 0.0, 1.0, 0, 1, False, per_slot=True, score=True)
    p, f = np.zeros((9, 5), np.uint32), np.zeros((9, 7), np.uint32)
    assert s.add_scored(p, f) == 3 and rec.calls[-1] == ("add_scored", -1, 5, 7, 0)
    assert s.add_scored(p[:, :2], f[:, :1], prefix=4, collect_hidden=True) == 3 and rec.calls[-1] == ("add_scored", 4, 2, 1, 1)
    n = len(rec.calls)
    bad_frames = [np.zeros((8, 7), np.uint32), np.zeros((9, 0), np.uint32), np.zeros((9, 7), np.int64), np.zeros((9, 7), np.float32),
                  np.zeros(63, np.uint32), np.zeros((1, 9, 7), np.uint32), [[0] * 7] * 9]
    for bad in bad_frames:
        with pytest.raises(ValueError, match="frames"):
            s.add_scored(p, bad)
    with pytest.raises(ValueError, match="prompt"):
        s.add_scored(np.zeros((8, 5), np.uint32), f)
    plain = flm.Session(_H(), 0.0, 1.0, 0, 1, False, per_slot=True)
    m = len(rec.calls)
    with pytest.raises(ValueError, match="score=True"):
        plain.add_scored(p, f)
    with pytest.raises(ValueError, match="first"):
        s.poll_scores(0, first=-1)
    assert len(rec.calls) == m == n + 1, "a refused add must not reach the library"


def test_referee_agrees_with_torch_log_softmax_in_f64():
    import torch
    rng = np.random.RandomState(5)
    rows = [rng.randn(n).astype(np.float32) * 3 for n in (2, 63, 64, 65, 1024, 2037, 2048)]
    crafted = np.arange(40, dtype=np.float32) * np.float32(0.01)
    tie = crafted.copy(); tie[[3, 17, 39]] = 1.0                     # the maximum three times, the last at n - 1
    zeros = -np.abs(crafted) - 1; zeros[5] = 0.0; zeros[9] = -0.0    # -0 == +0: the later index wins
    ninf = crafted.copy(); ninf[[0, 7, 20]] = -np.inf
    big = crafted.copy() * 100 - 80; big[11] = 80.0
    rows += [crafted, tie, zeros.astype(np.float32), ninf, big, np.full(33, 1.25, np.float32)]
    for row in rows:
        n = len(row)
        for ex in (False, True):
            x = torch.tensor(row, dtype=torch.float64)
            if ex:
                x[0] = -float("inf")
            ls = torch.log_softmax(x, dim=0).numpy()
            top = int(np.nonzero(ls == ls.max())[0][-1])
            for t in sorted({0, n - 1, top, n // 2}):
                lp, tlp, tp, eos = ref_scores(row, t, ex)
                assert tp == top, (n, ex)
                for got, want in ((lp, ls[t]), (tlp, ls[top]), (eos, ls[0])):
                    assert got == want or abs(got - want) <= 1e-12, (n, ex, t, got, want)
    assert ref_scores(tie, 0)[2] == 39 and ref_scores(zeros, 0)[2] == 9 and ref_scores(ninf, 3, True)[3] == -np.inf
