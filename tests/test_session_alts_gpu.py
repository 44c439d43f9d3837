"""GPU: FS_SESSION_ALTS -- the N most likely candidates and the entropy of every decision of a scoring or traced slot (include/fishrt.h:
fs_lm_session_poll_alts; the second instantiation of the score node, csrc/lm_sample.hip: each wave extracts its own top N from the
registers, one wave merges the 4 N keys).

Bounds.  Indices are compared EXACTLY: kernel and referee (tests/test_session_alts_cpu.py: ref_alts) order the same f32 bits by the same
rule, so a near tie cannot excuse a mismatch.  Log-probs: LP_TOL = 2e-4 absolute against the f64 referee, the score node's derived bound
(tests/test_session_score_gpu.py: an f32 sum of <= 2048 non-negative terms is within 2047 * 2^-24 = 1.2e-4 relative, which is the
absolute error of its log; the rest covers a few ulp of expf, logf and x - m).  Entropy: ENT_TOL = 2.5e-3 absolute: both sums
(sum e_i and sum e_i (x_i - m)) have same-signed terms, so each is within 1.2e-4 relative; their ratio is at most log 2048 = 7.63 in size,
hence 7.63 * 2.44e-4 + 1.2e-4 (the log) = 1.98e-3, and the rest covers a few ulp of expf, logf and the products.  Everything else is
compared bit for bit.  Fish-1.5 shapes, synthetic weights, max_batch 16; at most 7 slots and 13 iterations per slot."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import fishrt
from fishrt import _ffi
from fishrt import config as fcfg
from test_session_alts_cpu import PAD, ref_alts
from test_session_per_slot_gpu import PENALTIES, SETTINGS
from test_rows_gpu import EOS_BOOST, EOS_CFG, EOS_TOK, _eos_prompt

SEED = 0xF15E5EED
CFG, TOK = fcfg.FISH_1_5, fcfg.FISH_1_5_TOKENS
IM_END, SEM0 = TOK["im_end_id"], TOK["semantic_start_id"]
AUDIO_BASE = SEM0 - 1
N_AUDIO = CFG["vocab_size"] - IM_END
LP_TOL, ENT_TOL = 2e-4, 2.5e-3  # (derivations above)
KEYS = ("logprob", "top_logprob", "top", "eos_logprob")
AKEYS = ("alt_index", "alt_logprob", "entropy")


def _prompt(L, seed):
    p = np.zeros((9, L), np.uint32)
    p[0] = np.random.RandomState(seed).randint(0, IM_END, L)
    return p


def _frames(N, seed):
    rng = np.random.RandomState(seed)
    f = np.zeros((9, N), np.uint32)
    f[0] = SEM0 + rng.randint(0, CFG["vocab_size"] - SEM0, N)
    f[1:] = rng.randint(0, 1024, (8, N))
    return f


def _run_all(s, n_frames=8):
    while s.step(n_frames):
        pass


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    diff = np.nonzero(_bits(a) != _bits(b))
    assert diff[0].size == 0, f"{what}: differs at {[d[:5].tolist() for d in diff]}"


@pytest.fixture(scope="module")
def lm16():
    lm = fishrt.DualARTransformer(CFG, TOK, 0, "bf16", max_batch=16).load_synthetic(SEED)
    yield lm
    lm.close()


def _check_row(tag, row, exclude0, idx, lp, ent, n_alts):
    """one decision against the referee on its raw row -> (worst |dlogprob|, |dentropy|)"""
    ridx, rlp, rent = ref_alts(row, n_alts, exclude0)
    assert np.array_equal(idx, ridx), (tag, idx.tolist(), ridx.tolist())
    n_cand = row.size - (1 if exclude0 else 0)
    assert np.array_equal(idx == PAD, np.arange(n_alts) >= n_cand), (tag, "padding exactly behind the last candidate")
    assert np.array_equal(np.isnan(lp), idx == PAD) and np.array_equal(np.isneginf(lp), np.isneginf(rlp)), (tag, lp.tolist(), rlp.tolist())
    fin = np.isfinite(rlp)
    dlp = float(np.abs(lp[fin].astype(np.float64) - rlp[fin]).max()) if fin.any() else 0.0
    dent = abs(float(ent) - rent)
    assert dlp <= LP_TOL, (tag, dlp, lp.tolist(), rlp.tolist())
    assert dent <= ENT_TOL, (tag, float(ent), rent)
    return dlp, dent


# ------------------------------------------------------------------------------------------------------------------ 1. the hook alone
def _owned(t, n):
    """the candidates thread t of the node owns: 4 t .. 4 t + 3 and 1024 + 4 t .. + 3, below n"""
    return [i for i in list(range(4 * t, 4 * t + 4)) + list(range(1024 + 4 * t, 1024 + 4 * t + 4)) if i < n]


def _hook_rows(n, N, rng):
    """the rows that break a per-wave-then-merge selection, for n candidates and N alternatives -> (names, f32 [S][n])"""
    rows, names = [], []

    def add(name, r):
        names.append(name)
        rows.append(np.asarray(r, np.float32))

    base = lambda: rng.normal(0.0, 1.0, n).astype(np.float32)
    add("random N(0, 3)", rng.normal(0.0, 3.0, n))
    # the N largest in ONE thread's entries (N > its entries: the next thread's too -- the same wave)
    t = int(rng.randint(0, (min(n, 1024) + 3) // 4))
    own = (_owned(t, n) + _owned(t + 1, n) + _owned(max(t - 1, 0), n))
    own = list(dict.fromkeys(own))[:N]
    r = base()
    r[own] = 20.0 + rng.permutation(len(own)).astype(np.float32)
    add(f"the largest in thread {t}'s entries", r)
    # all in one wave (wave w owns 256 w .. 256 w + 255 and 1024 + 256 w .. + 255)
    w = int(rng.randint(0, (min(n, 1024) + 255) // 256))
    wave = [i for i in list(range(256 * w, 256 * w + 256)) + list(range(1024 + 256 * w, 1024 + 256 * w + 256)) if i < n]
    pick = rng.choice(wave, min(N, len(wave)), replace=False)
    r = base()
    r[pick] = 20.0 + rng.permutation(len(pick)).astype(np.float32)
    add(f"the largest all in wave {w}", r)
    # exactly one per wave
    r = base()
    for k, w2 in enumerate(range((min(n, 1024) + 255) // 256)):
        lo, hi = 256 * w2, min(256 * w2 + 256, n)
        r[int(rng.randint(lo, hi))] = 30.0 + k
    add("one winner per wave", r)
    # the maximum repeated N + 1 times: tie order, and alternative N - 1 is still a maximum
    r = base()
    r[rng.choice(n, min(N + 1, n), replace=False)] = 7.5
    add("the maximum N + 1 times", r)
    # -0 / +0 pairs on top of a negative row
    r = -np.abs(base()) - 1.0
    z = rng.choice(n, min(N + 2, n), replace=False)
    r[z] = np.where(rng.randint(0, 2, z.size) == 1, np.float32(-0.0), np.float32(0.0))
    add("-0 / +0 on top", r)
    # fewer than N finite entries, -inf elsewhere (one finite entry at an index >= 1, so that leaving candidate 0 out keeps one)
    r = np.full(n, -np.inf, np.float32)
    k = max(1, min(n - 1, N // 2))
    fin = 1 + rng.choice(n - 1, k, replace=False)
    r[fin] = rng.normal(0.0, 3.0, k)
    add(f"{k} finite entries", r)
    add("all entries equal", np.full(n, -1.25, np.float32))
    # winners at index 0, n - 1, 1023 and 1024
    r = base()
    for k, i in enumerate(i for i in (0, n - 1, 1023, 1024) if i < n):
        r[i] = 15.0 + 0.5 * k
    add("winners at 0, n - 1, 1023, 1024", r)
    add("|x| up to 80", rng.uniform(-80.0, 80.0, n))
    return names, np.ascontiguousarray(np.stack(rows))


def _alt_rows(rows, exclude0, N):
    S, n = rows.shape
    idx, lp, ent = np.zeros((S, N), np.uint32), np.zeros((S, N), np.float32), np.zeros(S, np.float32)
    fp = C.POINTER(C.c_float)
    _ffi.check(fishrt.lib().fs_selftest_alt_rows(0, rows.ctypes.data_as(fp), S, n, 1 if exclude0 else 0, N, idx.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                 lp.ctypes.data_as(fp), ent.ctypes.data_as(fp)))
    return idx, lp, ent


@pytest.mark.parametrize("N", [1, 8, 16])
def test_the_hook_alone(N):
    worst_lp, worst_ent = 0.0, 0.0
    for n in (2, 3, 15, 16, 17, 63, 64, 65, 512, 513, 1024, 2037, 2048):
        names, rows = _hook_rows(n, N, np.random.RandomState(1000 * N + n))
        for exclude0 in (False, True):
            idx, lp, ent = _alt_rows(rows, exclude0, N)
            for s, name in enumerate(names):
                dlp, dent = _check_row(f"n={n} N={N} exclude0={exclude0} row '{name}'", rows[s], exclude0, idx[s], lp[s], ent[s], N)
                worst_lp, worst_ent = max(worst_lp, dlp), max(worst_ent, dent)
            if exclude0:
                assert not (idx == 0).any(), (n, N, "candidate 0 is left out and never appears")
        if n == 2:  # with exclude0 there is one candidate
            assert idx[:, 0].tolist() == [1] * len(names) and (idx[:, 1:] == PAD).all()
    print(f"hook N={N}: worst |dlogprob| {worst_lp:.2e} (bound {LP_TOL:.0e}), worst |dentropy| {worst_ent:.2e} (bound {ENT_TOL:.1e})")


def test_the_hook_agrees_with_the_score_hook_bit_for_bit():
    """alternative 0 is the score node's top / top_logprob, and an alternative's log-prob is the score node's log-prob of that target"""
    n, N, rng = 2037, 8, np.random.RandomState(5)
    rows = np.ascontiguousarray(rng.normal(0.0, 3.0, (6, n)).astype(np.float32))
    idx, lp, ent = _alt_rows(rows, False, N)
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    for j in (0, 3, N - 1):
        tgt = np.ascontiguousarray(idx[:, j])
        slp, stlp, stop = np.zeros(6, np.float32), np.zeros(6, np.float32), np.zeros(6, np.uint32)
        _ffi.check(fishrt.lib().fs_selftest_score_rows(0, rows.ctypes.data_as(fp), 6, n, tgt.ctypes.data_as(up), 0, slp.ctypes.data_as(fp),
                                                       stlp.ctypes.data_as(fp), stop.ctypes.data_as(up), None))
        _same_bits(lp[:, j], slp, f"alt_logprob[{j}] vs the score hook's logprob of that target")
        assert np.array_equal(stop, idx[:, 0])
        _same_bits(lp[:, 0], stlp, "alt_logprob[0] vs top_logprob")


# ------------------------------------------------------------------------------------------------- 2. scoring slots in a session
def _check_slot_against_capture(tag, al, rec, targets, cap, ignore_eos, N):
    """al: poll_alts, rec: the slot's existing record (poll_scores / poll_trace), targets [n][9]: candidate index per decision (or -1)"""
    n = rec["logprob"].shape[0]
    assert al["alt_index"].shape == al["alt_logprob"].shape == (n, 9, N) and al["entropy"].shape == (n, 9), tag
    worst_lp, worst_ent = 0.0, 0.0
    for i in range(n):
        for d in range(9):
            if targets[i, d] < 0:
                continue
            row = cap[i, 0, :N_AUDIO] if d == 0 else cap[i, d, :1024]
            dlp, dent = _check_row(f"{tag} row {i} decision {d}", row, ignore_eos and d == 0, al["alt_index"][i, d], al["alt_logprob"][i, d],
                                   al["entropy"][i, d], N)
            worst_lp, worst_ent = max(worst_lp, dlp), max(worst_ent, dent)
            hit = np.nonzero(al["alt_index"][i, d] == targets[i, d])[0]
            if hit.size:  # the forced / picked token is among the alternatives: the very expression of logprob
                assert _bits(al["alt_logprob"][i, d, hit[:1]])[0] == _bits(rec["logprob"][i, d:d + 1])[0], (tag, i, d)
    ok = targets >= 0
    assert np.array_equal(al["alt_index"][..., 0][ok], rec["top"][ok]), (tag, "alt_index[..., 0] == top")
    _same_bits(al["alt_logprob"][..., 0][ok], rec["top_logprob"][ok], f"{tag}: alt_logprob[..., 0] vs top_logprob")
    if ignore_eos:
        assert not (al["alt_index"][:, 0] == 0).any(), (tag, "candidate 0 of the slow decision never appears under FS_GEN_IGNORE_EOS")
    return worst_lp, worst_ent


@pytest.mark.parametrize("dtype,ignore_eos,N", [("bf16", False, 8), ("bf16", True, 16), ("fp8", False, 5)])
def test_scoring_slots_against_the_captured_rows(dtype, ignore_eos, N, lm16):
    F, S = 13, 7
    lm = lm16 if dtype == "bf16" else fishrt.DualARTransformer(CFG, TOK, 0, dtype, max_batch=16).load_synthetic(SEED)
    seqs = [(_prompt(11 + 6 * i, 3100 + i), _frames(F, 3200 + i)) for i in range(S)]
    kw = dict(temp=0.0, top_p=1.0, top_k=0, seed=0, repetition_penalty=1.0, ignore_eos=ignore_eos, per_slot=True, score=True)

    def run(alts):
        with lm.session(alts=alts, **kw) as s:
            slots = []
            for i, (p, f) in enumerate(seqs):  # (three together, then one join per step: the slots sit at different iterations of a step)
                slots.append(s.add_scored(p, f))
                if i >= 2:
                    s.step(1)
            assert None not in slots
            _run_all(s)
            return slots, [s.poll_scores(sl) for sl in slots], [s.poll_alts(sl) for sl in slots] if alts else None

    try:
        lm.debug_capture(F)
        try:
            slots, recs, alts = run(N)
            caps = [lm.debug_read_row(sl, F) for sl in slots]
        finally:
            lm.debug_capture(0)
        _, recs0, _ = run(0)
        worst_lp, worst_ent = 0.0, 0.0
        for i, ((p, f), sl, rec, rec0, al, cap) in enumerate(zip(seqs, slots, recs, recs0, alts, caps)):
            for k in KEYS:
                _same_bits(rec[k], rec0[k], f"{dtype} sequence {i} {k}: the existing record in the session with the flag vs without")
            targets = np.concatenate([f[:1].astype(np.int64) - AUDIO_BASE, f[1:].astype(np.int64)]).T
            a, b = _check_slot_against_capture(f"{dtype} ignore_eos={ignore_eos} N={N} sequence {i}", al, rec, targets, cap, ignore_eos, N)
            worst_lp, worst_ent = max(worst_lp, a), max(worst_ent, b)
        print(f"{dtype} ignore_eos={ignore_eos} N={N}: {S} x {F} iterations, worst |dlogprob| {worst_lp:.2e} (bound {LP_TOL:.0e}), "
              f"worst |dentropy| {worst_ent:.2e} (bound {ENT_TOL:.1e})")
    finally:
        if lm is not lm16:
            lm.close()


# -------------------------------------------------------------------------------------------------------------------- 3. traced slots
@pytest.mark.parametrize("wide", [False, True])
def test_traced_slots_equal_add_scored_of_their_picks(lm16, wide):
    F, N = 10, 8
    reqs = [dict(kw=dict(temp=0.0, top_p=1.0, top_k=0), amt=1.0),  # greedy
            dict(kw=dict(temp=0.7, top_p=0.8, top_k=256), amt=1.2),  # narrow
            dict(kw=dict(temp=0.9, top_p=0.9, top_k=0) if wide else SETTINGS[1], amt=1.2),  # (wide: nucleus only)
            dict(kw=dict(temp=0.0, top_p=1.0, top_k=0), amt=1.4)]  # greedy behind the penalty: the pick may leave the argmax
    for i, r in enumerate(reqs):
        r["p"], r["seed"] = _prompt(13 + 7 * i, 4100 + i), 700 + 31 * i
    kw = dict(temp=0.7, top_p=0.8, top_k=256, seed=3, ignore_eos=True, per_slot=True, score=True, alts=N)
    with lm16.session(trace=True, wide=wide, **kw) as s:
        slots = [s.add(r["p"], r["p"].shape[1] + F - 2, sampling=dict(r["kw"], repetition_penalty=r["amt"]), seed=r["seed"], trace=True) for r in reqs]
        assert None not in slots
        _run_all(s)
        traced = [(s.poll_trace(sl), s.poll_alts(sl)) for sl in slots]
    with lm16.session(**kw) as s:  # (no trace flag: scoring slots only)
        slots = [s.add_scored(r["p"], np.ascontiguousarray(tr["tokens"].T)) for r, (tr, _) in zip(reqs, traced)]
        assert None not in slots
        _run_all(s)
        scored = [(s.poll_scores(sl), s.poll_alts(sl)) for sl in slots]
    for i, ((tr, ta), (sc, sa)) in enumerate(zip(traced, scored)):
        assert (tr["n_decisions"] == 9).all() and ta["alt_index"].shape == (F, 9, N)
        for k in KEYS:
            _same_bits(tr[k], sc[k], f"wide={wide} request {i} {k}: traced vs scored")
        for k in AKEYS:
            _same_bits(ta[k], sa[k], f"wide={wide} request {i} {k}: traced vs scored")
        assert np.array_equal(ta["alt_index"][..., 0], tr["top"]) and np.isfinite(ta["entropy"]).all() and (ta["entropy"] > 0).all()
        _same_bits(ta["alt_logprob"][..., 0], tr["top_logprob"], "alt_logprob[..., 0] vs top_logprob")
        pick = np.concatenate([tr["tokens"][:, :1].astype(np.int64) - AUDIO_BASE, tr["tokens"][:, 1:].astype(np.int64)], axis=1)
        hit = ta["alt_index"].astype(np.int64) == pick[..., None]
        assert hit.any(), "no pick among the alternatives: the bitwise rule is untested"
        want = np.broadcast_to(tr["logprob"][..., None], hit.shape)
        assert np.array_equal(_bits(ta["alt_logprob"])[hit], _bits(np.ascontiguousarray(want))[hit]), (i, "alt_logprob == logprob where the pick is an alternative")


def test_the_im_end_iteration_holds_the_fill(tmp_path):
    """The EOS-heavy checkpoint of tests/test_rows_gpu.py, without ignore_eos: the codebook decisions an <|im_end|> iteration skips hold
    0xFFFFFFFF / NaN / NaN, its slow decision is recorded, and every other row is complete."""
    import test_safetensors_gpu as tsf
    t = tsf._lm_tensors(EOS_CFG, bf16=True)
    t["output.weight"][EOS_TOK["im_end_id"]] *= np.float32(EOS_BOOST)
    t["output.weight"] = (t["output.weight"].view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    path = str(tmp_path / "model.safetensors")
    tsf._save(t, path, True)
    lm = fishrt.DualARTransformer(EOS_CFG, EOS_TOK, 0, "bf16", max_batch=8).load_safetensors(path)
    os.remove(path)
    N = 8
    try:
        prompts = [_eos_prompt(12 + (i % 5), 4000 + i) for i in range(8)]
        iters = [13, 13, 13, 13, 13, 13, 2, 3]
        kws = [dict(temp=0.0, top_p=1.0, top_k=0), dict(temp=1.0, top_p=0.95, top_k=256)]
        with lm.session(temp=0.7, top_p=0.8, top_k=256, seed=21, per_slot=True, score=True, trace=True, alts=N) as s:
            slots = [s.add(p, p.shape[1] + n - 2, sampling=dict(kws[i % 2], repetition_penalty=1.2), seed=40 + i, trace=True)
                     for i, (p, n) in enumerate(zip(prompts, iters))]
            assert sorted(slots) == list(range(8))
            _run_all(s, 3)
            got = [(s.poll_trace(sl), s.poll_alts(sl)) for sl in slots]
        by_eos = 0
        for i, (tr, al) in enumerate(got):
            n = tr["tokens"].shape[0]
            assert al["alt_index"].shape == (n, 9, N) and al["entropy"].shape == (n, 9), i
            full = tr["n_decisions"] == 9
            assert (al["alt_index"][full] < 2048).all() and np.isfinite(al["alt_logprob"][full]).all() and np.isfinite(al["entropy"][full]).all(), i
            assert np.array_equal(al["alt_index"][full][..., 0], tr["top"][full]), i
            for r in np.nonzero(~full)[0]:
                by_eos += 1
                assert r == n - 1 and tr["tokens"][r, 0] == EOS_TOK["im_end_id"], (i, r)
                assert (al["alt_index"][r, 1:] == PAD).all() and np.isnan(al["alt_logprob"][r, 1:]).all() and np.isnan(al["entropy"][r, 1:]).all(), (i, r)
                assert al["alt_index"][r, 0, 0] == tr["top"][r, 0] and np.isfinite(al["alt_logprob"][r, 0]).all() and np.isfinite(al["entropy"][r, 0]), (i, r)
                assert _bits(al["alt_logprob"][r, 0, :1])[0] == _bits(tr["top_logprob"][r, :1])[0], (i, r)
        assert by_eos >= 1, "no traced slot reached <|im_end|>: the fill is untested"
    finally:
        lm.close()


# ------------------------------------------------------------------------------------------------------------- 4. non-interference
def test_nothing_else_moves_and_the_graph_cache_and_pool_tell_sessions_apart(lm16):
    F = 8
    gen = [dict(p=_prompt(14 + 9 * i, 1300 + i), kw=SETTINGS[i % len(SETTINGS)], amt=PENALTIES[i % 3], seed=9000 + 17 * i) for i in range(5)]
    sp, sf = _prompt(16, 91), _frames(F, 92)

    def run(alts):
        with lm16.session(temp=0.7, top_p=0.8, top_k=256, seed=3, ignore_eos=True, per_slot=True, score=True, trace=True, repetition_penalty=1.4,
                          alts=alts) as s:
            add = lambda r, **kw: s.add(r["p"], r["p"].shape[1] + F - 2, sampling=dict(r["kw"], repetition_penalty=r["amt"]), seed=r["seed"], **kw)
            plain = [add(gen[0]), add(gen[1])]
            traced = [add(gen[2], trace=True)]
            s.step(2)
            scored = s.add_scored(sp, sf, collect_hidden=True)
            hid = add(gen[3], collect_hidden=True)
            traced.append(add(gen[4], trace=True))
            assert None not in plain + traced + [scored, hid]
            _run_all(s)
            out = dict(codes=[s.poll(sl)[0] for sl in plain + traced + [scored, hid]], scored=s.poll_scores(scored),
                       hidden=[s.poll_hidden(scored), s.poll_hidden(hid)], trace=[s.poll_trace(sl) for sl in traced])
            if alts:
                out["alts"] = [s.poll_alts(sl) for sl in traced + [scored]]
                with pytest.raises(RuntimeError, match="neither a scoring nor a traced slot"):
                    s.poll_alts(plain[0])
                with pytest.raises(RuntimeError, match="neither a scoring nor a traced slot"):
                    s.poll_alts(hid)
            return out

    # without the flag, with it, without it AFTER an ALTS session, and with another N after that (the step-graph cache, the buffer pool)
    runs = [run(0), run(8), run(0), run(16), run(8)]
    a = runs[0]
    for j, b in enumerate(runs[1:], 1):
        for i, (x, y) in enumerate(zip(a["codes"], b["codes"])):
            assert x.shape == (8, F) and np.array_equal(x, y), f"run {j} slot {i}: codes differ"
        for k in KEYS:
            _same_bits(a["scored"][k], b["scored"][k], f"run {j} scoring slot {k}")
            for i, (x, y) in enumerate(zip(a["trace"], b["trace"])):
                _same_bits(x[k], y[k], f"run {j} traced slot {i} {k}")
        for i, (x, y) in enumerate(zip(a["trace"], b["trace"])):
            assert np.array_equal(x["tokens"], y["tokens"]) and np.array_equal(x["n_decisions"], y["n_decisions"]), (j, i)
        for x, y in zip(a["hidden"], b["hidden"]):
            _same_bits(x, y, f"run {j} hidden rows")
    for x, y, z in zip(runs[1]["alts"], runs[3]["alts"], runs[4]["alts"]):
        assert x["alt_index"].shape == (F, 9, 8) and y["alt_index"].shape == (F, 9, 16)
        _same_bits(x["alt_index"], y["alt_index"][..., :8], "the 8 alternatives are the first 8 of the 16")
        _same_bits(x["alt_logprob"], y["alt_logprob"][..., :8], "the 8 alternatives are the first 8 of the 16")
        _same_bits(x["entropy"], y["entropy"], "entropy at N = 8 and N = 16")
        for k in AKEYS:
            _same_bits(x[k], z[k], f"{k}: N = 8 again after N = 16")


# --------------------------------------------------------------------------------------------------------- 5. flag and poll errors
def test_flag_and_poll_errors_name_their_cause(lm16):
    L = fishrt.lib()
    samp = _ffi.Sampling(0.0, 1.0, 0, 1.0)
    A, AN = _ffi.FS_SESSION_ALTS, _ffi.FS_SESSION_ALTS_N
    for flags, words in ((A, (b"FS_SESSION_ALTS", b"not alone")), (A | 64, (b"not alone",)), (A | 8, (b"FS_SESSION_ALTS", b"FS_SESSION_ROWS")),
                         (A | 16 | 64 | 8, (b"FS_SESSION_ROWS",)), (A | 16, (b"FS_SESSION_ALTS", b"without FS_SESSION_SCORE")),
                         (A | 16 | 32 | 128, (b"without FS_SESSION_SCORE",)), (A | 16 | 64 | AN(17), (b"FS_SESSION_ALTS_N(17)", b"16")),
                         (A | 16 | 64 | AN(31), (b"FS_SESSION_ALTS_N(31)",)), (16 | 64 | AN(4), (b"FS_SESSION_ALTS_N(4)", b"without FS_SESSION_ALTS")),
                         (16 | 64 | 128 | AN(16), (b"without FS_SESSION_ALTS",))):
        assert L.fs_lm_session_begin(lm16._h, C.byref(samp), C.c_uint64(1), flags) != 0, hex(flags)
        for w in words:
            assert w in L.fs_last_error(), (hex(flags), L.fs_last_error())
    p = np.ascontiguousarray(_prompt(12, 3))
    n, na = C.c_size_t(0), C.c_int(0)
    with lm16.session(temp=0.0, top_p=1.0, top_k=0, seed=1, per_slot=True, score=True) as s:  # the handle is usable; no flag: the poll refuses
        sc = s.add_scored(p, _frames(3, 5))
        assert L.fs_lm_session_poll_alts(lm16._h, sc, 0, None, None, None, 0, C.byref(n), C.byref(na)) != 0
        assert b"needs FS_SESSION_ALTS" in L.fs_last_error()
        _run_all(s)
        assert s.poll_scores(sc)["logprob"].shape == (3, 9)
    # the N field 0 is the default of 8; a plain slot of an ALTS session has no alternatives
    assert L.fs_lm_session_begin(lm16._h, C.byref(samp), C.c_uint64(1), 16 | 64 | A) == 0, L.fs_last_error()
    try:
        slot = C.c_int(-1)
        assert L.fs_lm_session_add(lm16._h, p.ctypes.data_as(C.POINTER(C.c_uint32)), 12, 14, C.byref(slot)) == 0 and slot.value >= 0
        act = C.c_int(0)
        assert L.fs_lm_session_step(lm16._h, 2, C.byref(act)) == 0
        assert L.fs_lm_session_poll_alts(lm16._h, slot.value, 0, None, None, None, 0, C.byref(n), C.byref(na)) != 0
        assert b"neither a scoring nor a traced slot" in L.fs_last_error(), L.fs_last_error()
        f = _frames(3, 6)
        sc = C.c_int(-1)
        assert L.fs_lm_session_add_scored(lm16._h, -1, p.ctypes.data_as(C.POINTER(C.c_uint32)), 12, f.ctypes.data_as(C.POINTER(C.c_uint32)), 3, 0,
                                          C.byref(sc)) == 0 and sc.value >= 0
        assert L.fs_lm_session_poll_alts(lm16._h, sc.value, 0, None, None, None, 0, C.byref(n), C.byref(na)) == 0, L.fs_last_error()
        assert (n.value, na.value) == (0, 8), "a prefilling slot has no rows; N field 0 = 8 alternatives"
        assert L.fs_lm_session_step(lm16._h, 8, C.byref(act)) == 0
        assert L.fs_lm_session_poll_alts(lm16._h, sc.value, 0, None, None, None, 0, C.byref(n), C.byref(na)) == 0 and n.value == 3
    finally:
        assert L.fs_lm_session_end(lm16._h) == 0
    lm14 = fishrt.DualARTransformer(dict(fcfg.FISH_1_4, n_layer=3), fcfg.FISH_1_4_TOKENS, 0, "bf16", max_batch=4).load_synthetic(SEED)
    try:
        assert L.fs_lm_session_begin(lm14._h, C.byref(samp), C.c_uint64(1), 16 | 64 | A) != 0
        assert b"Fish <= 1.4" in L.fs_last_error(), L.fs_last_error()
    finally:
        lm14.close()


# --------------------------------------------------------------------------------------------------------------- 6. the Python calls
def test_score_and_generate_traced_with_top_n(lm16):
    F, N = 6, 8
    prompts = [_prompt(11 + 5 * i, 300 + i) for i in range(3)]
    frames = [_frames(F - i, 400 + i) for i in range(3)]
    out = lm16.score(prompts, frames, top_n=N)
    plain = lm16.score(prompts, frames)
    with lm16.session(temp=0.0, top_p=1.0, top_k=0, seed=0, repetition_penalty=1.0, per_slot=True, score=True, alts=N) as s:
        slots = [s.add_scored(p, f) for p, f in zip(prompts, frames)]
        _run_all(s)
        ref = [(s.poll_scores(sl), s.poll_alts(sl)) for sl in slots]
    for i, (r, r0, (sc, al)) in enumerate(zip(out, plain, ref)):
        assert set(r) == set(r0) | set(AKEYS) and not set(r0) & set(AKEYS)
        assert r["alt_index"].shape == r["alt_logprob"].shape == (F - i, 9, N) and r["entropy"].shape == (F - i, 9)
        for k in KEYS:
            _same_bits(r[k], sc[k], f"score sequence {i} {k}")
            _same_bits(r[k], r0[k], f"score sequence {i} {k} with and without top_n")
        for k in AKEYS:
            _same_bits(r[k], al[k], f"score sequence {i} {k}")
    samplings = [dict(temp=0.0, repetition_penalty=1.0), None, dict(temp=0.7, top_p=0.8, top_k=256)]
    seeds = [1, 2, 3]
    budgets = [p.shape[1] + F - 2 for p in prompts]
    out = lm16.generate_traced(prompts, budgets, samplings=samplings, seeds=seeds, top_n=N)
    plain = lm16.generate_traced(prompts, budgets, samplings=samplings, seeds=seeds)
    with lm16.session(per_slot=True, score=True, trace=True, alts=N) as s:
        slots = [s.add(p, b, sampling=sp, seed=sd, trace=True) for p, b, sp, sd in zip(prompts, budgets, samplings, seeds)]
        _run_all(s)
        ref = [(s.poll(sl)[0], s.poll_trace(sl), s.poll_alts(sl)) for sl in slots]
    for i, (r, r0, (codes, tr, al)) in enumerate(zip(out, plain, ref)):
        n = r["tokens"].shape[0]
        assert set(r) == set(r0) | set(AKEYS) and np.array_equal(r["codes"], codes) and np.array_equal(r0["codes"], codes)
        assert r["alt_index"].shape == r["alt_logprob"].shape == (n, 9, N) and r["entropy"].shape == (n, 9)
        for k in KEYS + ("tokens", "n_decisions"):
            _same_bits(r[k], tr[k], f"generate_traced request {i} {k}")
        for k in AKEYS:
            _same_bits(r[k], al[k], f"generate_traced request {i} {k}")
