"""GPU: FS_SESSION_TRACE -- traced slots of a per-slot score session (include/fishrt.h: fs_lm_session_add_traced /
fs_lm_session_poll_trace).  A traced slot generates like any slot and leaves the scoring slots' record for the tokens it PICKED: the score
node in front of each sampler keeps the raw row, its maximum and log-sum (k_score_slots, second path), one tail node behind the frame's
last sampler reads the picks and closes the row (k_trace_commit).

Bounds.  Against the f64 referee on the captured raw row (test 1): TOL = 2e-4 absolute, the score node's derived bound
(tests/test_session_score_gpu.py: an f32 sum of <= 2048 non-negative terms is within 2047 * 2^-24 = 1.2e-4 relative, the absolute error
of its log; the rest covers a few ulp of expf, logf and x - m at |x| <= 100) -- it is the same arithmetic.  Everything else is compared
bit for bit: picks, `top`, the round trip through fs_lm_session_add_scored, and what the other slot kinds of the session produce.
Fish-1.5 shapes, synthetic weights; at most 8 slots and 13 iterations per slot."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import fishrt
from fishrt import config as fcfg
from test_session_score_cpu import ref_scores
from test_session_per_slot_gpu import PENALTIES, SETTINGS
from test_rows_gpu import EOS_BOOST, EOS_CFG, EOS_TOK, _eos_prompt

SEED = 0xF15E5EED
CFG, TOK = fcfg.FISH_1_5, fcfg.FISH_1_5_TOKENS
IM_END, SEM0 = TOK["im_end_id"], TOK["semantic_start_id"]
AUDIO_BASE = SEM0 - 1
N_AUDIO = CFG["vocab_size"] - IM_END
TOL = 2e-4  # traced record vs the f64 referee on the same row: the score node's bound (derivation above)
KEYS = ("logprob", "top_logprob", "top", "eos_logprob")
NOPICK = np.uint32(0xFFFFFFFF)


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


@pytest.fixture(scope="module")
def lm16():
    lm = fishrt.DualARTransformer(CFG, TOK, 0, "bf16", max_batch=16).load_synthetic(SEED)
    yield lm
    lm.close()


def _check_shapes(tr, n):
    assert tr["tokens"].shape == tr["logprob"].shape == tr["top_logprob"].shape == tr["top"].shape == (n, 9)
    assert tr["eos_logprob"].shape == tr["n_decisions"].shape == (n,)


def _check_skipped(tag, tr, i, im_end):
    """row i is an iteration whose slow pick was <|im_end|>: one decision, and its log-prob is the row's <|im_end|> log-prob"""
    assert tr["n_decisions"][i] == 1 and tr["tokens"][i, 0] == im_end, (tag, i)
    assert _bits(tr["logprob"][i, :1])[0] == _bits(tr["eos_logprob"][i:i + 1])[0], (tag, i, "logprob[0] is eos_logprob on the terminating row")
    assert np.isnan(tr["logprob"][i, 1:]).all() and np.isnan(tr["top_logprob"][i, 1:]).all(), (tag, i)
    assert (tr["top"][i, 1:] == NOPICK).all() and (tr["tokens"][i, 1:] == 0).all(), (tag, i)
    assert np.isfinite(tr["top_logprob"][i, 0]) and tr["top"][i, 0] < N_AUDIO, (tag, i)


# ------------------------------------------------------------------------------------------------------ 1. the record is the row's
def _check_against_capture(tag, tr, codes, cap, ignore_eos, greedy_raw):
    n = tr["tokens"].shape[0]
    _check_shapes(tr, n)
    made = tr["n_decisions"] == 9
    n_frames = codes.shape[1]
    assert n in (n_frames, n_frames + 1) and made[: n - 1].all(), (tag, n, n_frames)
    worst = 0.0
    for i in range(n):
        if not made[i]:  # (the capture of a frozen slot's last iteration is rewritten by the steps that follow: tests 4 covers this row)
            _check_skipped(tag, tr, i, IM_END)
            continue
        assert np.array_equal(tr["tokens"][i, 1:], codes[:, i]), (tag, i, "tokens[1:] are the polled codes")
        assert np.array_equal(cap[i, 1:, 1024].astype(np.int64), tr["tokens"][i, 1:].astype(np.int64)), (tag, i, "captured codebook picks")
        if i + 1 == n or made[i + 1]:  # (a slot that freezes rewrites the slow pick of the frame before in the capture record)
            assert int(cap[i, 0, 2047]) == int(tr["tokens"][i, 0]) - AUDIO_BASE, (tag, i, "captured slow pick")
        for d in range(9):
            row = cap[i, 0, :N_AUDIO] if d == 0 else cap[i, d, :1024]
            pick = int(tr["tokens"][i, 0]) - AUDIO_BASE if d == 0 else int(tr["tokens"][i, d])
            lp, tlp, top, eos = ref_scores(row, pick, ignore_eos and d == 0)
            assert tr["top"][i, d] == top, (tag, i, d, int(tr["top"][i, d]), top)
            for got, want in ((tr["logprob"][i, d], lp), (tr["top_logprob"][i, d], tlp)):
                print(f"{tag} row {i} decision {d}: {float(got):.6f} referee {want:.6f}")
                worst = max(worst, abs(float(got) - want))
                assert abs(float(got) - want) <= TOL, (tag, i, d, float(got), want)
            if d == 0 and ignore_eos:
                assert np.isneginf(tr["eos_logprob"][i]) and np.isneginf(row[0]), (tag, i)
            elif d == 0:
                worst = max(worst, abs(float(tr["eos_logprob"][i]) - eos))
                assert abs(float(tr["eos_logprob"][i]) - eos) <= TOL, (tag, i, float(tr["eos_logprob"][i]), eos)
    if greedy_raw:  # greedy on the raw row (no penalty): the pick IS the argmax
        want_top = np.concatenate([tr["tokens"][:, :1].astype(np.int64) - AUDIO_BASE, tr["tokens"][:, 1:].astype(np.int64)], axis=1)
        assert made.all() and np.array_equal(tr["top"].astype(np.int64), want_top), (tag, "a greedy slot without penalty picks the argmax")
        assert np.array_equal(_bits(tr["logprob"]), _bits(tr["top_logprob"])), (tag, "... and its log-prob is the top log-prob, bit for bit")
    return worst


@pytest.mark.parametrize("wide,ignore_eos", [(False, True), (False, False), (True, False)])
def test_the_record_is_the_rows(lm16, wide, ignore_eos):
    F = 10
    reqs = [dict(kw=dict(temp=0.0, top_p=1.0, top_k=0), amt=1.0),       # greedy on the raw row
            dict(kw=dict(temp=0.7, top_p=0.8, top_k=256), amt=1.2),
            dict(kw=SETTINGS[1], amt=PENALTIES[2]),
            dict(kw=dict(temp=0.0, top_p=1.0, top_k=0), amt=1.4),       # greedy behind the penalty: the pick may leave the argmax
            dict(kw=SETTINGS[2], amt=PENALTIES[0]),
            dict(kw=dict(temp=0.9, top_p=0.9, top_k=0) if wide else SETTINGS[3], amt=1.2),    # (wide: nucleus only)
            dict(kw=dict(temp=1.1, top_p=0.95, top_k=600) if wide else SETTINGS[0], amt=1.0)]  # (wide: top_k > 256)
    for i, r in enumerate(reqs):
        r["p"], r["seed"] = _prompt(13 + 7 * i, 2100 + i), 500 + 31 * i
    lm16.debug_capture(F)
    try:
        with lm16.session(temp=0.7, top_p=0.8, top_k=256, seed=3, ignore_eos=ignore_eos, per_slot=True, score=True, trace=True, wide=wide) as s:
            slots = []
            for i, r in enumerate(reqs):  # three together, then one join per round: the slots sit at different iterations of one step
                slots.append(s.add(r["p"], r["p"].shape[1] + F - 2, sampling=dict(r["kw"], repetition_penalty=r["amt"]), seed=r["seed"], trace=True))
                if i >= 2:
                    s.step(1)
            assert None not in slots and len(set(slots)) == len(reqs)
            _run_all(s)
            got = [(s.poll(sl), s.poll_trace(sl)) for sl in slots]
        caps = [lm16.debug_read_row(sl, F) for sl in slots]
    finally:
        lm16.debug_capture(0)
    for i, (r, sl, ((codes, done), tr), cap) in enumerate(zip(reqs, slots, got, caps)):
        assert done
        worst = _check_against_capture(f"wide={wide} ignore_eos={ignore_eos} slot {sl}", tr, codes, cap, ignore_eos, greedy_raw=(i == 0))
        print(f"wide={wide} ignore_eos={ignore_eos} slot {sl} {r['kw']}: {tr['tokens'].shape[0]} rows, max |dlogprob| vs the referee on the captured row {worst:.2e} (bound {TOL:.0e})")


# ------------------------------------------------------------------------------------------------------------------ 2. round trip
@pytest.mark.parametrize("dtype,max_batch", [("bf16", 16), ("fp8", 12)])
def test_feeding_the_traced_tokens_back_scores_the_same_records(dtype, max_batch, lm16):
    F, L = 10, 23
    lm = lm16 if dtype == "bf16" else fishrt.DualARTransformer(CFG, TOK, 0, dtype, max_batch=max_batch).load_synthetic(SEED)
    p = _prompt(L, 77)
    kw = dict(temp=0.7, top_p=0.8, top_k=256, seed=11, ignore_eos=True, per_slot=True, score=True, repetition_penalty=1.2)
    try:
        with lm.session(trace=True, **kw) as s:
            sl = s.add(p, L + F - 2, seed=1234, trace=True)
            _run_all(s)
            tr, codes = s.poll_trace(sl), s.poll(sl)[0]
        assert tr["tokens"].shape == (F, 9) and (tr["n_decisions"] == 9).all() and np.array_equal(tr["tokens"][:, 1:].T, codes)
        frames = np.ascontiguousarray(tr["tokens"].T)
        with lm.session(**kw) as s:  # (a score session without the trace flag: the graphs it always replayed)
            sl2 = s.add_scored(p, frames)
            _run_all(s)
            sc = s.poll_scores(sl2)
        for k in KEYS:
            diff = np.nonzero(_bits(sc[k]) != _bits(tr[k]))
            assert diff[0].size == 0, f"{dtype} {k}: scored != traced at rows {diff[0][:5]}, decisions {diff[1][:5] if len(diff) > 1 else ''}"
    finally:
        if lm is not lm16:
            lm.close()


# ------------------------------------------------------------------------------------------------------------ 3. nothing else moves
def test_other_slot_kinds_are_bit_identical_next_to_traced_slots(lm16):
    F = 8
    gen = [dict(p=_prompt(14 + 9 * i, 1300 + i), kw=SETTINGS[i % len(SETTINGS)], amt=PENALTIES[i % 3], seed=9000 + 17 * i) for i in range(6)]
    sp, sf = _prompt(16, 91), _frames(F, 92)

    def run(trace):
        with lm16.session(temp=0.7, top_p=0.8, top_k=256, seed=3, ignore_eos=True, per_slot=True, score=True, repetition_penalty=1.4,
                          **(dict(trace=True) if trace else {})) as s:
            add = lambda r, **kw: s.add(r["p"], r["p"].shape[1] + F - 2, sampling=dict(r["kw"], repetition_penalty=r["amt"]), seed=r["seed"], **kw)
            plain = [add(gen[0]), add(gen[1])]
            traced = [add(gen[2], trace=trace)]
            s.step(2)
            scored = s.add_scored(sp, sf, collect_hidden=True)
            hid = add(gen[3], collect_hidden=True)
            traced.append(add(gen[4], trace=trace))
            s.step(1)
            traced.append(add(gen[5], trace=trace, collect_hidden=True))
            assert None not in plain + traced + [scored, hid]
            _run_all(s)
            out = dict(plain=[s.poll(sl)[0] for sl in plain], traced=[s.poll(sl)[0] for sl in traced], scored=s.poll_scores(scored),
                       scored_codes=s.poll(scored)[0], scored_hid=s.poll_hidden(scored), hid=s.poll_hidden(hid), hid_codes=s.poll(hid)[0],
                       traced_hid=s.poll_hidden(traced[2]))
            if trace:
                out["trace"] = [s.poll_trace(sl) for sl in traced]
                with pytest.raises(RuntimeError, match="not a traced slot"):
                    s.poll_trace(plain[0])
                with pytest.raises(RuntimeError, match="not a traced slot"):
                    s.poll_trace(scored)
                with pytest.raises(RuntimeError, match="not a scoring slot"):
                    s.poll_scores(traced[0])
            return out

    a, b = run(False), run(True)
    for k in ("plain", "traced"):
        for i, (x, y) in enumerate(zip(a[k], b[k])):
            assert x.shape == (8, F) and np.array_equal(x, y), f"{k} request {i}: codes differ in the trace session"
    assert np.array_equal(a["scored_codes"], b["scored_codes"]) and np.array_equal(a["hid_codes"], b["hid_codes"])
    for k in KEYS:
        assert np.array_equal(_bits(a["scored"][k]), _bits(b["scored"][k])), f"scoring slot {k}: differs in the trace session"
    for k in ("scored_hid", "hid", "traced_hid"):
        assert a[k].shape == (F, CFG["dim"]) and np.array_equal(_bits(a[k]), _bits(b[k])), f"{k}: hidden rows differ in the trace session"
    for tr, codes in zip(b["trace"], b["traced"]):
        _check_shapes(tr, F)
        assert (tr["n_decisions"] == 9).all() and np.array_equal(tr["tokens"][:, 1:].T, codes)


# ---------------------------------------------------------------------------------------------------------------- 4. EOS and budget
def test_eos_closes_the_last_row_once_and_budget_ends_need_no_extra_row(tmp_path):
    """The EOS-heavy checkpoint of tests/test_rows_gpu.py, without ignore_eos: a slot that draws <|im_end|> is `done` from its slow
    sampler on, yet its row is closed (one decision), exactly once; a slot that ends by budget has only full rows."""
    import test_safetensors_gpu as tsf
    t = tsf._lm_tensors(EOS_CFG, bf16=True)
    t["output.weight"][EOS_TOK["im_end_id"]] *= np.float32(EOS_BOOST)
    t["output.weight"] = (t["output.weight"].view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    path = str(tmp_path / "model.safetensors")
    tsf._save(t, path, True)
    lm = fishrt.DualARTransformer(EOS_CFG, EOS_TOK, 0, "bf16", max_batch=8).load_safetensors(path)
    os.remove(path)
    try:
        prompts = [_eos_prompt(12 + (i % 5), 4000 + i) for i in range(8)]
        iters = [13, 13, 13, 13, 13, 13, 2, 3]
        kws = [dict(temp=0.0, top_p=1.0, top_k=0), dict(temp=1.0, top_p=0.95, top_k=256)]
        with lm.session(temp=0.7, top_p=0.8, top_k=256, seed=21, per_slot=True, score=True, trace=True) as s:
            slots = [s.add(p, p.shape[1] + n - 2, sampling=dict(kws[i % 2], repetition_penalty=1.2), seed=40 + i, collect_hidden=True, trace=True)
                     for i, (p, n) in enumerate(zip(prompts, iters))]
            assert sorted(slots) == list(range(8))
            _run_all(s, 3)  # (the short-budget and the terminated slots ride the others' steps to the end: they must add no row)
            got = [(s.poll(sl), s.poll_trace(sl), s.poll_hidden(sl).shape[0]) for sl in slots]
        by_eos, by_budget = 0, 0
        for i, ((codes, done), tr, n_hid) in enumerate(got):
            n, n_frames = tr["tokens"].shape[0], codes.shape[1]
            assert done and 1 <= n <= iters[i] and n == n_hid, (i, n, n_hid, "one row per iteration the slot ran == poll_hidden's count")
            _check_shapes(tr, n)
            assert (tr["n_decisions"][: n - 1] == 9).all(), (i, "only the last row can be the terminating one")
            full = tr["n_decisions"] == 9
            assert np.isfinite(tr["logprob"][full]).all() and (tr["tokens"][full][:, 0] >= EOS_TOK["semantic_start_id"]).all(), i
            if tr["n_decisions"][-1] == 1:
                by_eos += 1
                _check_skipped(f"slot {i}", tr, n - 1, EOS_TOK["im_end_id"])
                assert n == (n_frames + 1 if n > 1 else n_frames), (i, n, n_frames, "the terminating iteration emits no frame (but frame 0)")
                assert np.array_equal(tr["tokens"][: n - 1, 1:].T, codes[:, : n - 1]), i
            else:
                by_budget += 1
                assert n == iters[i] == n_frames and np.array_equal(tr["tokens"][:, 1:].T, codes), (i, n, n_frames)
        print(f"EOS-heavy checkpoint: {by_eos} traced slots ended by <|im_end|> (rows {[g[1]['tokens'].shape[0] for g in got]}), {by_budget} by budget")
        assert by_eos >= 1, "no traced slot reached <|im_end|>: the early-exit path is untested"
        assert by_budget >= 1, "no traced slot ended by budget"
    finally:
        lm.close()


# ------------------------------------------------------------------------------------------------------------------- 5. life cycle
def test_life_cycle(lm16):
    F, L = 8, 19
    p = _prompt(L, 7)
    kw = dict(temp=0.7, top_p=0.8, top_k=256, seed=1, ignore_eos=True, per_slot=True, score=True, trace=True)
    with lm16.session(**kw) as s:
        a = s.add(p, L + F - 2, seed=5, trace=True)
        assert s.poll_trace(a)["tokens"].shape == (0, 9), "a slot that is still prefilling has no rows"
        s.step(3)
        assert s.poll_trace(a)["tokens"].shape == (3, 9)
        _run_all(s)
        full = s.poll_trace(a)
        assert full["tokens"].shape == (F, 9) and s.poll(a, codes=False) == (F, True)
        s.step(2)
        assert s.poll_trace(a)["tokens"].shape == (F, 9), "a finished slot adds no row"
        tail = s.poll_trace(a, first=3)  # paging
        for k in KEYS + ("tokens", "n_decisions"):
            assert np.array_equal(_bits(tail[k]), _bits(full[k][3:])), k
        assert s.poll_trace(a, first=F)["tokens"].shape == (0, 9) and s.poll_trace(a, first=50)["n_decisions"].shape == (0,)
        # a released and re-admitted slot starts again at row 0, and the same request leaves the same records
        s.release(a)
        b = s.add(p, L + 3 - 2, seed=5, trace=True)
        g = s.add(p, L + 3 - 2, seed=5)
        sc = s.add_scored(p, np.ascontiguousarray(full["tokens"][:2].T))
        assert b == a and s.poll_trace(b)["tokens"].shape == (0, 9)
        _run_all(s)
        again = s.poll_trace(b)
        assert again["tokens"].shape == (3, 9)
        for k in KEYS + ("tokens", "n_decisions"):
            assert np.array_equal(_bits(again[k]), _bits(full[k][:3])), f"{k}: the re-admitted slot's rows differ from the first run's"
        assert np.array_equal(s.poll(g)[0], s.poll(b)[0]), "a traced slot's codes are those of the same fs_lm_session_add_ex request"
        with pytest.raises(RuntimeError, match="not a traced slot"):
            s.poll_trace(g)
        with pytest.raises(RuntimeError, match="not a traced slot"):
            s.poll_trace(sc)
        with pytest.raises(RuntimeError, match="not a scoring slot"):
            s.poll_scores(b)
        assert s.poll_scores(sc)["logprob"].shape == (2, 9)
        # a traced add still pending when the session ends: its buffer goes back with it ...
        assert s.add(p, L + F - 2, seed=6, trace=True) is not None
    with lm16.session(**kw) as s:  # ... and the next session on the handle runs as the first did
        a = s.add(p, L + F - 2, seed=5, trace=True)
        _run_all(s)
        fresh = s.poll_trace(a)
    for k in KEYS + ("tokens", "n_decisions"):
        assert np.array_equal(_bits(fresh[k]), _bits(full[k])), k


def test_errors_say_which_flag_is_missing(lm16):
    L = fishrt.lib()
    samp = fishrt._ffi.Sampling(0.0, 1.0, 0, 1.0)
    for flags, word in ((128, b"not alone"), (128 | 16, b"without FS_SESSION_SCORE"), (128 | 64, b"not alone"), (128 | 8, b"FS_SESSION_ROWS"),
                        (128 | 64 | 16 | 8, b"FS_SESSION_ROWS")):
        assert L.fs_lm_session_begin(lm16._h, C.byref(samp), C.c_uint64(1), flags) != 0, flags
        assert word in L.fs_last_error() and (b"FS_SESSION_TRACE" in L.fs_last_error() or b"FS_SESSION_SCORE" in L.fs_last_error()), (flags, L.fs_last_error())
    p = np.ascontiguousarray(_prompt(12, 3))
    with lm16.session(temp=0.0, top_p=1.0, top_k=0, seed=1, per_slot=True, score=True) as s:  # no flag: both entry points refuse
        slot, n = C.c_int(-1), C.c_size_t(0)
        g = s.add(p, 12 + 2)
        assert L.fs_lm_session_add_traced(lm16._h, -1, p.ctypes.data_as(C.POINTER(C.c_uint32)), 12, 14, None, None, 0, C.byref(slot)) != 0
        assert b"needs FS_SESSION_TRACE" in L.fs_last_error()
        assert L.fs_lm_session_poll_trace(lm16._h, g, 0, None, None, None, None, None, None, 0, C.byref(n)) != 0
        assert b"needs FS_SESSION_TRACE" in L.fs_last_error()
        _run_all(s)
        assert s.poll(g)[0].shape == (8, 4)
    with lm16.session(temp=0.7, top_p=0.8, top_k=256, seed=1, per_slot=True, score=True, trace=True) as s:  # a narrow session refuses a wide setting
        with pytest.raises(RuntimeError, match="top_k"):
            s.add(p, 14, sampling=dict(temp=0.7, top_k=0), trace=True)
        a = s.add(p, 14, trace=True)
        _run_all(s)
        assert s.poll_trace(a)["tokens"].shape == (4, 9)
    lm14 = fishrt.DualARTransformer(dict(fcfg.FISH_1_4, n_layer=3), fcfg.FISH_1_4_TOKENS, 0, "bf16", max_batch=4).load_synthetic(SEED)
    try:
        assert L.fs_lm_session_begin(lm14._h, C.byref(samp), C.c_uint64(1), 16 | 64 | 128) != 0
        assert b"Fish <= 1.4" in L.fs_last_error(), L.fs_last_error()
    finally:
        lm14.close()


def test_generate_traced_is_the_session_done_by_hand(lm16):
    F = 6
    prompts = [_prompt(11 + 5 * i, 300 + i) for i in range(3)]
    samplings = [dict(temp=0.0, repetition_penalty=1.0), None, dict(temp=0.7, top_p=0.8, top_k=256)]
    seeds = [1, 2, 3]
    out = lm16.generate_traced(prompts, [p.shape[1] + F - 2 for p in prompts], samplings=samplings, seeds=seeds, collect_hidden=True)
    with lm16.session(per_slot=True, score=True, trace=True) as s:
        slots = [s.add(p, p.shape[1] + F - 2, sampling=sp, seed=sd, trace=True) for p, sp, sd in zip(prompts, samplings, seeds)]
        _run_all(s)
        ref = [(s.poll(sl)[0], s.poll_trace(sl)) for sl in slots]
    for r, (codes, tr) in zip(out, ref):
        assert r["hidden"].shape[0] == r["tokens"].shape[0] and np.array_equal(r["codes"], codes)
        for k in KEYS + ("tokens", "n_decisions"):
            assert np.array_equal(_bits(r[k]), _bits(tr[k])), k
        assert abs(r["total"] - float(np.nansum(tr["logprob"], dtype=np.float64))) == 0.0
