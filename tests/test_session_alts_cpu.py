"""CPU: FS_SESSION_ALTS through the layers that need no GPU -- the header defines the flag, the N field and both prototypes, the ctypes
table agrees, fishrt.lm.Session sends the flags and raises its errors before the library is called (a recording stand-in for the library,
as tests/test_session_score_cpu.py uses), the f64 referee of the GPU tests (ref_alts) agrees with torch on rows of distinct values, and the
collector book hands out no buffer pooled under a shorter row size (a small host program against csrc/fs_slot_book.h)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from fishrt import _ffi, lm as flm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "fishrt.h")).read()
PAD = 0xFFFFFFFF


def ref_alts(row, n_alts, exclude0=False):
    """The referee of the alternatives: row f32 [n] -> (alt_index u32 [n_alts], alt_logprob f64 [n_alts], entropy f64).  Candidates: every
    index, without 0 when exclude0.  Order: value descending with -0 == +0, among equal values the HIGHER index first; -inf last.
    log-prob = exact log-softmax over the candidates (f64); entropy = log(s) - sum_i exp(x_i - m) (x_i - m) / s over the finite ones;
    padding 0xFFFFFFFF / NaN behind the last candidate."""
    x = np.asarray(row, np.float32).astype(np.float64) + 0.0  # (-0 -> +0)
    cand = np.arange(1 if exclude0 else 0, x.size)
    xc = x[cand]
    order = np.lexsort((-cand, -xc))  # primary: value descending; secondary: index descending
    m = xc.max()
    fin = np.isfinite(xc)
    d = xc[fin] - m
    e = np.exp(d)
    s = e.sum()
    idx = np.full(n_alts, PAD, np.uint32)
    lp = np.full(n_alts, np.nan, np.float64)
    k = min(n_alts, cand.size)
    idx[:k] = cand[order[:k]]
    lp[:k] = (xc[order[:k]] - m) - np.log(s)
    return idx, lp, float(np.log(s) - (e * d).sum() / s)


def _args(name):
    m = re.search(r"int\s+" + name + r"\(([^;]*)\);", HEADER)
    assert m, f"{name} is not declared"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_and_ffi_table_agree():
    assert re.search(r"#define\s+FS_SESSION_ALTS\s+256u", HEADER)
    assert re.search(r"#define\s+FS_SESSION_ALTS_N\(n\)\s+\(\(uint32_t\)\(n\)\s*<<\s*16\)", HEADER)
    assert re.search(r"#define\s+FS_ALTS_MAX\s+16u?", HEADER)
    assert _ffi.FS_SESSION_ALTS == 256 and _ffi.FS_ALTS_MAX == 16 and _ffi.FS_SESSION_TRACE == 128 and _ffi.FS_SESSION_SCORE == 64
    # the flag arithmetic: the N field is 5 bits at 16, clear of every flag bit
    assert _ffi.FS_SESSION_ALTS | _ffi.FS_SESSION_ALTS_N(16) == 256 | (16 << 16) == 0x100100
    every_flag = 1 | 8 | 16 | 32 | 64 | 128 | 256
    assert _ffi.FS_SESSION_ALTS_N(31) & every_flag == 0 and (_ffi.FS_SESSION_ALTS_N(31) >> 16) == 31 and _ffi.FS_SESSION_ALTS_N(0) == 0
    protos = {
        "fs_lm_session_poll_alts": ["fs_lm_t* lm", "int slot", "size_t first_row", "uint32_t* alt_index", "float* alt_logprob", "float* entropy",
                                    "size_t cap_rows", "size_t* n_rows", "int* n_alts"],
        "fs_selftest_alt_rows": ["int device_id", "const float* logits", "int S", "int n", "int exclude0", "int n_alts", "uint32_t* alt_index_out",
                                 "float* alt_logprob_out", "float* entropy_out"],
    }
    ctype_of = {"int": C.c_int, "size_t": C.c_size_t, "fs_lm_t*": C.c_void_p, "uint32_t*": C.POINTER(C.c_uint32), "float*": C.POINTER(C.c_float),
                "const float*": C.POINTER(C.c_float), "int*": C.POINTER(C.c_int), "size_t*": C.POINTER(C.c_size_t)}
    for name, want in protos.items():
        assert _args(name) == want, name
        assert name in _ffi.SYMBOLS
        assert _ffi.ALTS_PROTOTYPES[name] == [ctype_of[a.rsplit(" ", 1)[0]] for a in want], name


class _RecLib:
    """records the calls a fishrt.lm.Session makes instead of running them"""

    def __init__(self):
        self.calls = []

    def fs_lm_session_begin(self, h, s, seed, flags):
        self.calls.append(("begin", int(flags)))
        return 0

    def fs_lm_session_end(self, h):
        return 0

    def fs_lm_session_poll_alts(self, h, slot, first, idx, lp, ent, cap, n, na):
        self.calls.append(("poll_alts", slot, int(first.value), int(cap.value), idx is None))
        n._obj.value = 4
        na._obj.value = 8
        return 0


class _H:
    cfg = dict(num_codebooks=8, dim=1024)
    _h = None


def test_session_sends_the_flags_and_raises_before_any_call(monkeypatch):
    rec = _RecLib()
    monkeypatch.setattr(_ffi, "lib", lambda: rec)
    s = flm.Session(_H(), 0.0, 1.0, 0, 1, False, per_slot=True, score=True, alts=8)
    assert rec.calls[-1] == ("begin", 16 | 64 | 256 | (8 << 16)) and s.alts == 8
    s = flm.Session(_H(), 0.7, 0.8, 0, 1, True, per_slot=True, wide=True, score=True, trace=True, alts=16)
    assert rec.calls[-1] == ("begin", 1 | 16 | 32 | 64 | 128 | 256 | (16 << 16))
    s = flm.Session(_H(), 0.7, 0.8, 0, 1, False, per_slot=True, score=True, alts=1)
    assert rec.calls[-1] == ("begin", 16 | 64 | 256 | (1 << 16))
    s0 = flm.Session(_H(), 0.7, 0.8, 256, 1, False, per_slot=True, score=True, trace=True)
    assert rec.calls[-1] == ("begin", 16 | 64 | 128) and s0.alts == 0, "a session without alts keeps its flags"
    s0 = flm.Session(_H(), 0.7, 0.8, 256, 1, False, per_slot=True, score=True, alts=0)
    assert rec.calls[-1] == ("begin", 16 | 64)
    n = len(rec.calls)
    for kw in (dict(), dict(per_slot=True), dict(per_slot=True, wide=True)):
        with pytest.raises(ValueError, match="per_slot=True and score=True"):  # alts without score
            flm.Session(_H(), 0.7, 0.8, 0, 1, False, alts=8, **kw)
    with pytest.raises(ValueError, match="rows"):  # alts with rows
        flm.Session(_H(), 0.7, 0.8, 0, 1, False, rows=True, alts=8)
    for bad in (17, 32, -1, 2.5, True):
        with pytest.raises(ValueError, match="0 .. 16"):
            flm.Session(_H(), 0.7, 0.8, 0, 1, False, per_slot=True, score=True, alts=bad)
    with pytest.raises(ValueError, match="alts=N"):
        s0.poll_alts(0)
    with pytest.raises(ValueError, match="first"):
        s.poll_alts(0, first=-1)
    assert len(rec.calls) == n, "a refused call must not reach the library"
    r = s.poll_alts(3, first=1)
    assert rec.calls[-2:] == [("poll_alts", 3, 0, 0, True), ("poll_alts", 3, 1, 3, False)]
    assert r["alt_index"].shape == r["alt_logprob"].shape == (3, 9, 8) and r["entropy"].shape == (3, 9)
    assert r["alt_index"].dtype == np.uint32 and r["alt_logprob"].dtype == r["entropy"].dtype == np.float32


def test_score_and_generate_traced_check_top_n_before_they_open_a_session(monkeypatch):
    rec = _RecLib()
    monkeypatch.setattr(_ffi, "lib", lambda: rec)
    p, f = np.zeros((9, 5), np.uint32), np.zeros((9, 3), np.uint32)
    for bad in (17, -2):
        with pytest.raises(ValueError, match="top_n"):
            flm.DualARTransformer.score(_H(), [p], [f], top_n=bad)
        with pytest.raises(ValueError, match="top_n"):
            flm.DualARTransformer.generate_traced(_H(), [p], 8, top_n=bad)
    assert rec.calls == []


def test_referee_agrees_with_torch_on_distinct_rows():
    import torch
    rng = np.random.default_rng(7)
    for n, n_alts, ex0 in ((2, 1, False), (17, 8, False), (65, 16, True), (1024, 16, False), (2037, 8, True), (2048, 16, False)):
        row = (rng.permutation(n).astype(np.float32) - n / 2) * np.float32(0.01) + rng.uniform(-1e-3, 1e-3, n).astype(np.float32)
        assert np.unique(row).size == n
        idx, lp, ent = ref_alts(row, n_alts, ex0)
        t = torch.from_numpy(row.astype(np.float64))[1 if ex0 else 0:]
        ls = torch.log_softmax(t, dim=0)
        k = min(n_alts, t.numel())
        v, i = torch.topk(ls, k)
        assert np.array_equal(idx[:k], i.numpy().astype(np.uint32) + (1 if ex0 else 0)), (n, n_alts)
        assert np.abs(lp[:k] - v.numpy()).max() < 1e-12
        assert np.all(idx[k:] == PAD) and np.all(np.isnan(lp[k:]))
        assert abs(ent - float(-(ls.exp() * ls).sum())) < 1e-10


def test_referee_order_rule():
    ninf = -np.inf
    # equal values: the HIGHER index first; -0 == +0; -inf last with log-prob -inf and no share in the entropy; padding behind the candidates
    idx, lp, ent = ref_alts(np.array([1.0, 3.0, 3.0, -0.0, 0.0, ninf, 3.0], np.float32), 8)
    assert idx.tolist() == [6, 2, 1, 0, 4, 3, 5, PAD]
    assert lp[0] == lp[1] == lp[2] and lp[4] == lp[5] and lp[6] == ninf and np.isnan(lp[7]) and np.isfinite(ent)
    idx, lp, ent = ref_alts(np.array([9.0, 1.0], np.float32), 4, exclude0=True)  # one candidate
    assert idx.tolist() == [1, PAD, PAD, PAD] and lp[0] == 0.0 and ent == 0.0
    idx, lp, ent = ref_alts(np.zeros(5, np.float32), 2)
    assert idx.tolist() == [4, 3] and abs(ent - np.log(5)) < 1e-12


_BOOK_PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "fs_slot_book.h"
static size_t g_last = 0; static int g_live = 0;
static void* al(size_t n) { g_last = n; ++g_live; return std::malloc(n); }
static void fr(void* p) { --g_live; std::free(p); }
int main(int argc, char** argv) {
    const size_t a = std::strtoul(argv[1], nullptr, 10), b = std::strtoul(argv[2], nullptr, 10);
    const int cap = std::atoi(argv[3]);
    {
        fs::SlotBook<fs::ScoreSlot> book(al, fr);
        book.begin(4, a);
        fs::SlotBuf s = book.take(cap);
        book.put(s);
        std::printf("pooled_a %zu alloc_a %zu\n", book.pooled(), g_last);
        book.begin(4, a);
        std::printf("pooled_same %zu\n", book.pooled());
        book.begin(4, b);
        g_last = 0;
        fs::SlotBuf l = book.take(cap);
        std::printf("pooled_b %zu alloc_b %zu cap_b %d live %d\n", book.pooled(), g_last, l.cap, g_live);
        char* p = static_cast<char*>(l.p);
        for (size_t i = 0; i < b * (size_t)cap; ++i) p[i] = 1;
    }
    std::printf("live_end %d\n", g_live);
    return 0;
}
"""


def test_slot_book_frees_its_pool_when_the_row_size_changes(tmp_path):
    """begin with row size a, take and put back a buffer; begin with row size b > a, take the same cap: a fresh allocation of b * cap bytes"""
    cxx = shutil.which("c++") or "/opt/rocm/bin/hipcc"
    src, exe = tmp_path / "book.cpp", str(tmp_path / "book")
    src.write_text(_BOOK_PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "fish-speech.rs_amd", "csrc"), str(src), "-o", exe], check=True)
    a, cap = 128 + 4 * 9, 12
    b = a + 9 * (8 * 16 + 4)
    r = subprocess.run([exe, str(a), str(b), str(cap)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout
    got = dict(zip(r.stdout.split()[::2], map(int, r.stdout.split()[1::2])))
    assert got["pooled_a"] == 1 and got["alloc_a"] == a * cap
    assert got["pooled_same"] == 1, "the same row size keeps the pool"
    assert got["pooled_b"] == 0 and got["alloc_b"] >= b * cap and got["cap_b"] == cap and got["live"] == 1, got
    assert got["live_end"] == 0
