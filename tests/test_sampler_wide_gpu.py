"""The per-slot sampler of a FS_SESSION_PER_SLOT | FS_SESSION_WIDE_SAMPLER session (include/fishrt.h) through its test hook,
fs_selftest_sample_slots: every stream is one slot -- its own StdRng stream, its own settings -- making R decisions in order on given
rows.  The referee is the oracle's LogitsProcessor (orc_sampler_create / orc_sampler_sample), one per stream.
 (1) token-exact in volume: 48 streams x 64 rows at n = 300 / 1024 / 2037 / 2048 with nucleus-only, wide top-k, narrow and greedy settings mixed;
 (2) crafted rows: all-equal, ties across the top-k boundary and across the top-p cut, -inf entries, one-hot, a running sum that reaches
     top_p = 1.0 before the last entry;
 (3) CPU, the oracle alone: the settings above cannot be served by clamping top_k to 256 or by dropping top-p -- every wide stream's
     oracle picks differ from the picks with top_k = 256 (and, nucleus-only with top_p < 1, from those with top_p = 1)."""
import ctypes as C
import functools

import numpy as np
import pytest

from fishrt import _ffi
from oracle import oracle as orc

S, R = 48, 64
NS = (300, 1024, 2037, 2048)
TEMPS = (0.02, 0.7, 1.0, 1.5)
TOP_PS = (0.0, 0.5, 0.8, 1.0)
NARROW = (dict(temp=0.7, top_p=0.8, top_k=256), dict(temp=1.0, top_p=0.9, top_k=50), dict(temp=0.02, top_p=0.8, top_k=256),
          dict(temp=0.7, top_p=1.0, top_k=128), dict(temp=1.5, top_p=0.5, top_k=200), dict(temp=0.7, top_p=0.0, top_k=1))
GREEDY_STREAM = 5


def _top_ks(n):
    return (0, 257, 300, n - 1, n, n + 5, 1000)


def is_wide(kw, n):
    """the decisions FS_SESSION_PER_SLOT alone refuses: sampled with no top-k, or a top-k outside the block-parallel sampler"""
    return kw["temp"] > 0 and (kw["top_k"] == 0 or kw["top_k"] > 256 or kw["top_k"] >= n)


def volume_settings(n):
    """48 streams: every 8th inside the narrow limit, one greedy, the other 41 wide -- top_k cycles through 7 values, top_p through 4 (all
    28 pairs occur), temp through 4.
    n = 300 is the exception: its wide streams take top_p from {0.0, 1.0} only.  The 256 largest of 300 probabilities hold at least
    256 / 300 of the mass whatever the row, so a nucleus of 0.5 or 0.8 lies inside them and top_k = 256 provably gives the same picks:
    test (3) cannot hold for such a stream, and a stream it cannot hold for shows nothing about the wide path."""
    top_ps = TOP_PS if n >= 1024 else (0.0, 1.0)
    out, w = [], 0
    for s in range(S):
        if s == GREEDY_STREAM:
            out.append(dict(temp=0.0, top_p=1.0, top_k=0))
        elif s % 8 == 7:
            out.append(dict(NARROW[(s // 8) % len(NARROW)]))
        else:
            out.append(dict(temp=TEMPS[(w // 3) % 4], top_p=top_ps[w % len(top_ps)], top_k=_top_ks(n)[w % 7]))
            w += 1
    return out


def volume_case(n):
    """logits [S][R][n], settings, seeds.  A stream's rows are N(0, 1) x its temperature x a per-row scale in {0.4, 1, 2.5, 6}: after the
    division by the temperature every stream sees flat, middling and peaked rows alike (also the temp = 0.02 ones), so that what lies
    outside the 256 largest candidates carries weight in every stream -- see test (3)"""
    rs = np.random.RandomState(1000 + n)
    settings = volume_settings(n)
    scale = np.array([0.4, 1.0, 2.5, 6.0], np.float32)[rs.randint(0, 4, (S, R))]
    temps = np.array([kw["temp"] if kw["temp"] > 0 else 1.0 for kw in settings], np.float32)
    logits = rs.randn(S, R, n).astype(np.float32) * scale[:, :, None] * temps[:, None, None]
    seeds = [0x5EED0000 + 7919 * s + n for s in range(S)]
    return np.ascontiguousarray(logits), settings, seeds


def gpu_slots(logits, settings, seeds):
    """fs_selftest_sample_slots -> (picks [S][R], words_used [S])"""
    s_, r_, n = logits.shape
    ss = (_ffi.Sampling * s_)(*[_ffi.Sampling(float(kw["temp"]), float(kw["top_p"]), int(kw["top_k"]), 1.0) for kw in settings])
    sd = (C.c_uint64 * s_)(*[int(v) for v in seeds])
    out = np.zeros((s_, r_), np.uint32)
    used = np.zeros(s_, np.uint64)
    logits = np.ascontiguousarray(logits, np.float32)
    _ffi.check(_ffi.lib().fs_selftest_sample_slots(0, logits.ctypes.data_as(C.POINTER(C.c_float)), s_, r_, n, ss, sd,
                                                   out.ctypes.data_as(C.POINTER(C.c_uint32)), used.ctypes.data_as(C.POINTER(C.c_uint64))))
    return out, used


def orc_stream(rows, kw, seed):
    """one oracle LogitsProcessor over the rows [R][n] in order -> picks [R]"""
    L = orc.lib()
    rows = np.ascontiguousarray(rows, np.float32)
    n = rows.shape[1]
    s = L.orc_sampler_create(C.c_uint64(seed), C.c_double(kw["temp"]), C.c_double(kw["top_p"]), C.c_uint64(kw["top_k"]))
    try:
        return np.array([L.orc_sampler_sample(C.c_void_p(s), rows[r].ctypes.data_as(C.POINTER(C.c_float)), C.c_uint64(n)) for r in range(rows.shape[0])],
                        np.uint32)
    finally:
        L.orc_sampler_destroy(C.c_void_p(s))


def orc_words_used(rows, kw, picks):
    """stream words the oracle's R decisions consumed: a sampled decision draws one word unless every weight is zero -- which for a
    softmax row happens exactly when the nucleus cut zeroes the first entry already, top_p <= 0 without a top-k (the pick is then 0)"""
    if kw["temp"] == 0:
        return 0
    n = rows.shape[1]
    nucleus = kw["top_k"] == 0 or kw["top_k"] >= n
    if nucleus and np.float32(kw["top_p"]) <= 0:
        assert not picks.any()
        return 0
    return rows.shape[0]


@functools.lru_cache(maxsize=None)
def volume_reference(n):
    logits, settings, seeds = volume_case(n)
    return np.stack([orc_stream(logits[s], settings[s], seeds[s]) for s in range(S)])


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
def test_streams_token_exact_in_volume(n):
    logits, settings, seeds = volume_case(n)
    assert {kw["top_k"] for kw in settings} >= set(_top_ks(n)) and {kw["top_p"] for kw in settings if is_wide(kw, n)} == set(TOP_PS if n >= 1024 else (0.0, 1.0))
    assert {kw["temp"] for kw in settings} >= set(TEMPS) | {0.0}
    assert sum(is_wide(kw, n) for kw in settings) == 41 and sum(kw["temp"] > 0 and not is_wide(kw, n) for kw in settings) == 6
    exp = volume_reference(n)
    got, used = gpu_slots(logits, settings, seeds)
    bad = np.argwhere(got != exp)
    print(f"n={n}: {S * R - len(bad)}/{S * R} decisions identical to the oracle")
    assert bad.size == 0, f"first (stream, row) {bad[0]}: gpu {got[tuple(bad[0])]} oracle {exp[tuple(bad[0])]} settings {settings[bad[0][0]]}"
    exp_used = [orc_words_used(logits[s], settings[s], exp[s]) for s in range(S)]
    assert used.tolist() == exp_used, [(s, settings[s], int(used[s]), exp_used[s]) for s in range(S) if int(used[s]) != exp_used[s]][:4]


def test_the_volume_settings_are_not_served_by_a_clamped_top_k_or_a_dropped_top_p():
    """CPU, the oracle alone (check 3): for every wide stream of test (1) the oracle's picks with the stream's top_k differ from its picks
    with top_k = 256 in at least one decision; nucleus-only streams with top_p < 1 also differ from top_p = 1"""
    for n in NS:
        logits, settings, seeds = volume_case(n)
        exp = volume_reference(n)
        for s, kw in enumerate(settings):
            if not is_wide(kw, n):
                continue
            clamped = orc_stream(logits[s], dict(kw, top_k=256), seeds[s])
            assert (clamped != exp[s]).any(), f"n={n} stream {s} {kw}: top_k = 256 gives the same {R} picks"
            if (kw["top_k"] == 0 or kw["top_k"] >= n) and kw["top_p"] < 1:
                no_cut = orc_stream(logits[s], dict(kw, top_p=1.0), seeds[s])
                assert (no_cut != exp[s]).any(), f"n={n} stream {s} {kw}: top_p = 1 gives the same {R} picks"


# ---- crafted rows.  Every case is one stream of RC rows built by the same recipe (another permutation / another random part per row), so
# that the draws land on different sides of the edge the case is about.
RC = 32


def _crafted(n):
    rs = np.random.RandomState(77 + n)
    cases = []  # (name, rows [RC][n], settings)

    def add(name, rows, **kw):
        rows = np.ascontiguousarray(rows, np.float32)
        assert rows.shape == (RC, n)
        cases.append((name, rows, kw))

    # all-equal: n equal weights; the cumulative chain over all of them must round like the oracle's (1 / 2037 is not a power of two)
    for top_p in (1.0, 0.8):
        add(f"all-equal top_p={top_p}", np.full((RC, n), 0.25), temp=0.7, top_p=top_p, top_k=0)
    add("all-equal top_k=300", np.full((RC, n), -1.5), temp=1.0, top_p=0.9, top_k=300)
    # exact ties across the top-k boundary: 280 distinct larger values, then 60 equal ones of which top_k = 300 keeps the 20 of lowest index
    rows = np.empty((RC, n), np.float32)
    for r in range(RC):
        v = np.concatenate([np.linspace(0.5, 0.2, 280), np.full(60, 0.1), -0.5 - rs.rand(n - 340)]).astype(np.float32)
        rows[r] = v[rs.permutation(n)]
    add("ties across top_k", rows, temp=1.0, top_p=1.0, top_k=300)
    add("ties across top_k, top-p cut inside them", rows, temp=1.0, top_p=0.97, top_k=300)
    # ties across the top-p cut: a few levels only, hundreds of equal candidates per level
    rows = (np.round(rs.randn(RC, n) * 1.5) / 1.5).astype(np.float32)
    add("ties across top_p, nucleus-only", rows, temp=1.0, top_p=0.5, top_k=0)
    add("ties across top_p, top_k=1000", rows, temp=0.7, top_p=0.8, top_k=1000)
    # -inf entries, index 0 among them; with top_k = 1000 of n = 1024 fewer finite candidates than top_k: zero-weight entries are kept
    rows = rs.randn(RC, n).astype(np.float32)
    rows[rs.rand(RC, n) < 0.35] = -np.inf
    rows[:, 0] = -np.inf
    rows[:, n - 1] = -np.inf
    rows[:, 17] = 0.5
    add("-inf entries, nucleus-only", rows, temp=0.7, top_p=0.8, top_k=0)
    add("-inf entries, top_k=1000", rows, temp=1.0, top_p=1.0, top_k=1000)
    add("-inf entries, top_k=n-1", rows, temp=1.0, top_p=0.9, top_k=n - 1)
    # one-hot: a single finite candidate / a single candidate far above the rest
    rows = np.full((RC, n), -np.inf, np.float32)
    hot = rs.randint(0, n, RC)
    rows[np.arange(RC), hot] = 3.0
    add("one-hot (-inf elsewhere)", rows, temp=0.7, top_p=0.8, top_k=0)
    add("one-hot (-inf elsewhere), top_k=257", rows, temp=0.7, top_p=1.0, top_k=257)
    rows = rs.randn(RC, n).astype(np.float32)
    rows[np.arange(RC), hot] = 60.0
    add("one-hot (60 above the rest)", rows, temp=1.0, top_p=1.0, top_k=0)
    # the descending running sum reaches top_p = 1.0 before the last entry: one candidate holds 1 - (n - 1) q, the others q = e^-17 ~ 4.1e-8
    # each -- more than half an ulp of the running sum (5.96e-8 just below 1), so every addition rounds UP by a whole ulp and the f32 sum
    # passes 1.0 after about two thirds of the entries; the rest is zeroed (asserted on the f32 chain below)
    rows = np.zeros((RC, n), np.float32)
    rows[np.arange(RC), hot] = 17.0
    add("running sum reaches top_p=1.0 early", rows, temp=1.0, top_p=1.0, top_k=0)
    p = np.exp(np.float32(-17.0) * np.ones(n, np.float32)); p[0] = 1.0
    p = (p / np.float32(p.astype(np.float64).sum())).astype(np.float32)
    run = np.cumsum(p, dtype=np.float32)
    assert run[n // 2] < 1.0 <= run[n - 8], "the crafted row does not reach 1.0 before its last entries"
    return cases


@functools.lru_cache(maxsize=None)
def crafted_case(n):
    cases = _crafted(n)
    logits = np.stack([c[1] for c in cases])
    settings = [c[2] for c in cases]
    seeds = [0xC0FFEE + 31 * i + n for i in range(len(cases))]
    exp = np.stack([orc_stream(logits[i], settings[i], seeds[i]) for i in range(len(cases))])
    return [c[0] for c in cases], logits, settings, seeds, exp


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1024, 2037, 2048])
def test_crafted_rows(n):
    names, logits, settings, seeds, exp = crafted_case(n)
    got, used = gpu_slots(logits, settings, seeds)
    for i, name in enumerate(names):
        bad = np.nonzero(got[i] != exp[i])[0]
        assert bad.size == 0, f"n={n} {name} {settings[i]}: rows {bad[:6]} gpu {got[i][bad[:6]]} oracle {exp[i][bad[:6]]}"
        assert int(used[i]) == orc_words_used(logits[i], settings[i], exp[i]), (name, int(used[i]))
    # the crafted edges are really hit: kept ties are the lowest indices, -inf entries are never picked
    i = names.index("ties across top_k")
    for r in range(RC):
        tied = np.nonzero(logits[i][r] == np.float32(0.1))[0]
        assert exp[i][r] not in tied[20:], "the oracle picked a tied candidate of higher index than the 20 kept"
    assert any(exp[i][r] in np.nonzero(logits[i][r] == np.float32(0.1))[0][:20] for r in range(RC)), "no draw landed on a kept tie"
    i = names.index("-inf entries, top_k=1000")
    assert np.isfinite(logits[i][np.arange(RC), exp[i]]).all()


@pytest.mark.gpu
def test_hook_refuses_bad_arguments():
    L = _ffi.lib()
    logits = np.zeros((1, 1, 4096), np.float32)
    ss = (_ffi.Sampling * 1)(_ffi.Sampling(0.7, 0.8, 0, 1.0))
    sd = (C.c_uint64 * 1)(1)
    out, used = np.zeros(1, np.uint32), np.zeros(1, np.uint64)
    args = (out.ctypes.data_as(C.POINTER(C.c_uint32)), used.ctypes.data_as(C.POINTER(C.c_uint64)))
    assert L.fs_selftest_sample_slots(0, logits.ctypes.data_as(C.POINTER(C.c_float)), 1, 1, 2049, ss, sd, *args) != 0
    assert b"2048" in L.fs_last_error()
    bad = (_ffi.Sampling * 1)(_ffi.Sampling(-0.5, 0.8, 0, 1.0))
    assert L.fs_selftest_sample_slots(0, logits.ctypes.data_as(C.POINTER(C.c_float)), 1, 1, 100, bad, sd, *args) != 0
    assert b"temp" in L.fs_last_error()
