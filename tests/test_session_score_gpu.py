"""GPU: FS_SESSION_SCORE -- scoring slots of a per-slot session (include/fishrt.h: fs_lm_session_add_scored / fs_lm_session_poll_scores).
A scoring slot is forced along a given code sequence by a small node (k_score_slots) in front of each of the step's 9 per-slot sampler
nodes, which records the f32 log-softmax of the raw row at the forced token and at its maximum, and the greedy pick.

Bounds.  Score node against the f64 referee on the SAME row (tests 1, 2): 2e-4 absolute -- an f32 sum of at most 2048 non-negative terms
in any order is within 2047 * 2^-24 = 1.2e-4 relative, which is the absolute error of its log; the rest covers a few ulp of expf, logf and
x_t - m at |x| <= 100.  `top` and the forced rows are compared exactly.  Against the teacher-forced CPU oracle (test 5): 2e-2 = twice the
project's unforced bf16 logit bound BF16_TOL = 1e-2 (tests/test_timed_workloads_gpu.py) -- a log-softmax entry moves at most twice the
largest logit error.  Fish-1.5 shapes, synthetic weights."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import fishrt
from fishrt import config as fcfg
from oracle import oracle as orc
from test_session_score_cpu import ref_scores
from test_session_per_slot_gpu import PENALTIES, SETTINGS

SEED = 0xF15E5EED
CFG, TOK = fcfg.FISH_1_5, fcfg.FISH_1_5_TOKENS
IM_END, SEM0 = TOK["im_end_id"], TOK["semantic_start_id"]
AUDIO_BASE = SEM0 - 1
N_AUDIO = CFG["vocab_size"] - IM_END
TOL = 2e-4          # score node vs the f64 referee on the same row (derivation above)
ORACLE_TOL = 2e-2   # vs the teacher-forced oracle: 2 x BF16_TOL
FP = C.POINTER(C.c_float)
UP = C.POINTER(C.c_uint32)


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


@pytest.fixture(scope="module")
def lm16():
    lm = fishrt.DualARTransformer(CFG, TOK, 0, "bf16", max_batch=16).load_synthetic(SEED)
    yield lm
    lm.close()


# ---------------------------------------------------------------------------------------------------------------- 1. the kernel alone
def _score_rows(rows, targets, exclude0):
    rows = np.ascontiguousarray(rows, np.float32)
    S, n = rows.shape
    t = np.ascontiguousarray(targets, np.uint32)
    lp, tlp, top, out = np.zeros(S, np.float32), np.zeros(S, np.float32), np.zeros(S, np.uint32), np.zeros((S, n), np.float32)
    fishrt._ffi.check(fishrt.lib().fs_selftest_score_rows(0, rows.ctypes.data_as(FP), S, n, t.ctypes.data_as(UP), int(exclude0),
                                                          lp.ctypes.data_as(FP), tlp.ctypes.data_as(FP), top.ctypes.data_as(UP), out.ctypes.data_as(FP)))
    return lp, tlp, top, out


def _crafted_rows(n, rng):
    """(row, [targets]) pairs; crafted logits are spaced by >= 0.01, so a wrong target is far outside the tolerance"""
    grid = (rng.permutation(n).astype(np.float32) - np.float32(n // 2)) * np.float32(0.01)  # distinct, 0.01 apart
    am = int(np.argmax(grid))
    ends = [0, n - 1, am]
    rows = [(rng.randn(n).astype(np.float32) * 3, ends), (rng.randn(n).astype(np.float32) * 3, ends), (grid.copy(), ends)]
    rep = grid.copy(); rep[[0, n // 2, n - 1]] = grid.max() + np.float32(1)          # the maximum three times, the last at n - 1
    rows.append((rep, [0, n - 1, n // 2]))
    rep2 = grid.copy(); rep2[[0, n // 3]] = grid.max() + np.float32(1)               # ... and with the last one inside the row
    rows.append((rep2, [0, n - 1, n // 3]))
    z = -np.abs(grid) - np.float32(1); z[n // 2] = np.float32(0.0); z[n - 1] = np.float32(-0.0); z[0] = np.float32(-0.0)  # -0 == +0
    rows.append((z, [0, n - 1, n // 2]))
    z2 = z.copy(); z2[n - 1] = np.float32(-3)                                         # (+0 behind -0: still the later index)
    rows.append((z2, [0, n - 1, n // 2]))
    ni = grid.copy(); ni[rng.rand(n) < 0.3] = -np.inf; ni[n // 2] = np.float32(2)     # -inf entries (never all of them)
    rows.append((ni, [0, n - 1, n // 2]))
    big = np.clip(grid * 100, -80, 80).astype(np.float32); big[n // 2] = np.float32(80); big[0] = np.float32(-80)
    rows.append((big, [0, n - 1, n // 2]))
    rows.append((-big, [0, n - 1, n // 2]))
    rows.append((np.full(n, 1.25, np.float32), [0, n - 1, n // 2]))                   # all equal: the last index, logprob -log(n)
    return rows


@pytest.mark.parametrize("n", [2, 63, 64, 65, 1024, 2037, 2048])
def test_score_node_on_caller_rows(n):
    rng = np.random.RandomState(100 + n)
    rows, targets = [], []
    for row, ts in _crafted_rows(n, rng):
        for t in sorted(set(ts)):
            rows.append(row)
            targets.append(t)
    rows = np.stack(rows)
    worst = 0.0
    for ex in (0, 1):
        lp, tlp, top, out = _score_rows(rows, targets, ex)
        for i, (row, t) in enumerate(zip(rows, targets)):
            rlp, rtlp, rtop, _ = ref_scores(row, t, bool(ex))
            assert top[i] == rtop, (n, ex, i, t, int(top[i]), rtop)
            for got, want in ((lp[i], rlp), (tlp[i], rtlp)):
                if np.isinf(want):
                    assert got == want, (n, ex, i, t, got, want)
                else:
                    worst = max(worst, abs(float(got) - want))
                    assert abs(float(got) - want) <= TOL, (n, ex, i, t, float(got), want)
            exp = row.copy(); exp[t] = np.inf
            assert np.array_equal(out[i].view(np.uint32), exp.view(np.uint32)), (n, ex, i, t, "the row must come back unchanged but for +inf at the target")
    print(f"score node, n = {n}: {len(targets)} rows x exclude0 off/on, max |dlogprob| vs the f64 referee {worst:.2e} (bound {TOL:.0e})")


# ------------------------------------------------------------------------------------- 2. forced means forced; the record is the row's
def _check_slot(tag, frames, codes, sc, cap, ignore_eos):
    N = frames.shape[1]
    assert codes.shape == (8, N) and np.array_equal(codes, frames[1:]), f"{tag}: the polled codes are not frames[1:]"
    assert sc["logprob"].shape == sc["top_logprob"].shape == sc["top"].shape == (N, 9) and sc["eos_logprob"].shape == (N,)
    assert np.array_equal(cap[:N, 0, 2047].astype(np.int64), frames[0].astype(np.int64) - AUDIO_BASE), f"{tag}: captured slow picks"
    assert np.array_equal(cap[:N, 1:, 1024].astype(np.int64), frames[1:].T.astype(np.int64)), f"{tag}: captured codebook picks"
    worst = 0.0
    for i in range(N):
        for d in range(9):
            row = cap[i, 0, :N_AUDIO] if d == 0 else cap[i, d, :1024]
            t = int(frames[0, i]) - AUDIO_BASE if d == 0 else int(frames[d, i])
            lp, tlp, top, eos = ref_scores(row, t, ignore_eos and d == 0)
            assert sc["top"][i, d] == top, (tag, i, d, int(sc["top"][i, d]), top)
            for got, want in ((sc["logprob"][i, d], lp), (sc["top_logprob"][i, d], tlp)):
                worst = max(worst, abs(float(got) - want))
                assert abs(float(got) - want) <= TOL, (tag, i, d, float(got), want)
            if d == 0:
                if ignore_eos:
                    assert np.isneginf(sc["eos_logprob"][i]) and np.isneginf(row[0]), (tag, i)
                else:
                    worst = max(worst, abs(float(sc["eos_logprob"][i]) - eos))
                    assert abs(float(sc["eos_logprob"][i]) - eos) <= TOL, (tag, i, float(sc["eos_logprob"][i]), eos)
    return worst


@pytest.mark.parametrize("dtype,max_batch", [("bf16", 16), ("fp8", 12)])
def test_forced_slots_emit_their_targets_and_record_their_rows(dtype, max_batch, lm16):
    F = 12
    lm = lm16 if dtype == "bf16" else fishrt.DualARTransformer(CFG, TOK, 0, dtype, max_batch=max_batch).load_synthetic(SEED)
    pre = _prompt(37 + 9, 700)
    plan = [dict(p=pre[:, 37:], f=_frames(12, 1), prefix=True), dict(p=_prompt(21, 701), f=_frames(9, 2)), dict(p=_prompt(30, 702), f=_frames(12, 3)),
            dict(p=_prompt(17, 703), f=_frames(5, 4))]
    try:
        for ignore_eos in (True, False):
            lm.debug_capture(F)
            try:
                with lm.session(temp=0.7, top_p=0.8, top_k=256, seed=3, ignore_eos=ignore_eos, per_slot=True, score=True) as s:
                    pid = s.add_prefix(pre[:, :37])
                    slots = [s.add_scored(plan[0]["p"], plan[0]["f"], prefix=pid)]
                    slots += [s.add_scored(r["p"], r["f"]) for r in plan[1:3]]  # two admitted together
                    s.step(3)
                    slots.append(s.add_scored(plan[3]["p"], plan[3]["f"]))      # one joining mid-flight
                    assert None not in slots and len(set(slots)) == 4
                    _run_all(s)
                    got = [(s.poll(sl), s.poll_scores(sl)) for sl in slots]
                caps = [lm.debug_read_row(sl, F) for sl in slots]
            finally:
                lm.debug_capture(0)
            for r, sl, ((codes, done), sc), cap in zip(plan, slots, got, caps):
                assert done
                worst = _check_slot(f"{dtype} ignore_eos={ignore_eos} slot {sl}", r["f"], codes, sc, cap, ignore_eos)
                print(f"{dtype} ignore_eos={ignore_eos} slot {sl}: {r['f'].shape[1]} x 9 records, max |dlogprob| vs the referee on the captured row {worst:.2e}")
    finally:
        if lm is not lm16:
            lm.close()


# ------------------------------------------------------------------------------------------------------------- 3. self-consistency
def test_scoring_a_greedy_sequence_reproduces_its_run(lm16):
    F, L = 12, 26
    p = _prompt(L, 41)
    kw = dict(temp=0.0, top_p=1.0, top_k=0, seed=5, ignore_eos=True, per_slot=True, repetition_penalty=1.0)
    lm16.debug_capture(F)
    try:
        with lm16.session(**kw) as s:
            sl = s.add(p, L + F - 2, collect_hidden=True)
            _run_all(s)
            codes, hid = s.poll(sl)[0], s.poll_hidden(sl)
        cap_gen = lm16.debug_read_row(sl, F)
        assert codes.shape == (8, F) and hid.shape == (F, CFG["dim"])
        frames = np.concatenate([(cap_gen[:, 0, 2047].astype(np.int64) + AUDIO_BASE)[None], codes.astype(np.int64)]).astype(np.uint32)
        lm16.debug_capture(F)  # (a fresh, zeroed record for the second run)
        with lm16.session(score=True, **kw) as s:
            sl2 = s.add_scored(p, frames, collect_hidden=True)
            _run_all(s)
            sc, codes2, hid2 = s.poll_scores(sl2), s.poll(sl2)[0], s.poll_hidden(sl2)
        cap_sc = lm16.debug_read_row(sl2, F)
    finally:
        lm16.debug_capture(0)
    assert np.array_equal(codes2, codes)
    want_top = np.concatenate([frames[:1].astype(np.int64) - AUDIO_BASE, frames[1:].astype(np.int64)]).T
    assert np.array_equal(sc["top"].astype(np.int64), want_top), "the model's own greedy sequence must be the argmax at all F x 9 decisions"
    assert np.array_equal(sc["top_logprob"].view(np.uint32), sc["logprob"].view(np.uint32))
    assert np.array_equal(cap_gen.view(np.uint32), cap_sc.view(np.uint32)), "the scoring run saw other rows than the generating run"
    assert np.array_equal(hid.view(np.uint32), hid2.view(np.uint32)), "hidden rows of the scoring slot differ from the generating slot's"


# ------------------------------------------------------------------------------------------------------------ 4. nothing else moves
def test_generating_slots_are_bit_identical_with_the_flag_and_next_to_scoring_slots(lm16):
    F, n = 10, 7
    reqs = [dict(p=_prompt(14 + 9 * i, 1300 + i), kw=SETTINGS[i % len(SETTINGS)], amt=PENALTIES[i % 3], seed=9000 + 17 * i) for i in range(n)]

    def run(score, scoring):
        with lm16.session(temp=0.7, top_p=0.8, top_k=256, seed=3, ignore_eos=True, per_slot=True, repetition_penalty=1.4,
                          **(dict(score=True) if score else {})) as s:
            slots, extra, k = [], [], 0
            for r in reqs:  # one join per round: each request meets the others mid-flight
                slots.append(s.add(r["p"], r["p"].shape[1] + F - 2, sampling=dict(r["kw"], repetition_penalty=r["amt"]), seed=r["seed"]))
                assert slots[-1] is not None
                if scoring:  # scoring slots join between the steps, and leave again as soon as they are done
                    extra.append(s.add_scored(_prompt(11 + k, 50 + k), _frames(2 + k % 3, 60 + k)))
                    assert extra[-1] is not None
                    k += 1
                s.step(2)
                for e in [e for e in extra if s.poll(e, codes=False)[1]]:
                    assert s.poll_scores(e)["logprob"].shape[0] == s.poll(e, codes=False)[0]
                    s.release(e)
                    extra.remove(e)
            _run_all(s)
            return [s.poll(sl)[0] for sl in slots]

    a, b, c = run(False, False), run(True, False), run(True, True)
    for i in range(n):
        assert a[i].shape == (8, F)
        assert np.array_equal(a[i], b[i]), f"request {i}: the flag alone changed a generating slot's codes"
        assert np.array_equal(a[i], c[i]), f"request {i}: scoring slots next to it changed a generating slot's codes"


# ------------------------------------------------------------------------------------------------- 5. against the oracle, end to end
def test_scores_against_the_teacher_forced_oracle(lm16):
    F, L = 12, 16
    p, frames = _prompt(L, 88), _frames(F, 89)
    with lm16.session(temp=0.0, top_p=1.0, top_k=0, seed=1, per_slot=True, score=True) as s:
        sl = s.add_scored(p, frames)
        _run_all(s)
        sc = s.poll_scores(sl)
    o = orc.OracleLM(orc.FISH15).load_synthetic(SEED, bf16=True)
    o.set_kv_round_bf16(True)
    femb = o.fast_embeddings()
    cur, pos = p, 0
    worst = 0.0
    for f in range(F):
        lg, hd = o.forward_generate(cur, pos, full_head=False)
        lp, _, _, eos = ref_scores(lg[0, IM_END:], int(frames[0, f]) - AUDIO_BASE)
        d = max(abs(float(sc["logprob"][f, 0]) - lp), abs(float(sc["eos_logprob"][f]) - eos))
        o.clear_fast()
        x = hd[0]
        for c in range(8):
            fg = o.forward_generate_fast(x, c)[0]
            d = max(d, abs(float(sc["logprob"][f, 1 + c]) - ref_scores(fg, int(frames[1 + c, f]))[0]))
            x = femb[int(frames[1 + c, f])]
        worst = max(worst, d)
        pos += cur.shape[1]
        cur = frames[:, f].reshape(9, 1)
    line = f"session score, bf16, {L}-position prompt, {F} forced frames: max |dlogprob| vs the teacher-forced oracle {worst:.2e} over {F * 9} decisions (bound {ORACLE_TOL:.0e})"
    print(line)
    path = os.environ.get("FISHRT_PARITY_LOG")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")
    assert worst <= ORACLE_TOL


# --------------------------------------------------------------------------------------------------------- 6. bookkeeping and errors
def test_bookkeeping(lm16):
    p, f = _prompt(19, 7), _frames(8, 8)
    with lm16.session(temp=0.0, top_p=1.0, top_k=0, seed=1, per_slot=True, score=True) as s:
        a = s.add_scored(p, f)
        assert s.poll_scores(a)["logprob"].shape == (0, 9), "a slot that is still prefilling has no rows"
        s.step(3)
        assert s.poll_scores(a)["logprob"].shape == (3, 9)
        _run_all(s)
        full = s.poll_scores(a)
        assert full["logprob"].shape == (8, 9) and s.poll(a, codes=False) == (8, True)
        tail = s.poll_scores(a, first=3)
        for k in ("logprob", "top_logprob", "top", "eos_logprob"):
            assert np.array_equal(tail[k].view(np.uint32), full[k][3:].view(np.uint32)), k
        assert s.poll_scores(a, first=8)["logprob"].shape == (0, 9) and s.poll_scores(a, first=50)["eos_logprob"].shape == (0,)
        # a released and re-admitted slot starts at row 0; N = 1 works
        s.release(a)
        b = s.add_scored(p, f[:, :1])
        assert b == a and s.poll_scores(b)["logprob"].shape == (0, 9)
        _run_all(s)
        one = s.poll_scores(b)
        assert one["logprob"].shape == (1, 9) and np.array_equal(one["logprob"].view(np.uint32), full["logprob"][:1].view(np.uint32))
        assert np.array_equal(s.poll(b)[0], f[1:, :1])
        # *slot = -1 when every slot is taken
        others = [s.add_scored(_prompt(4 + i, 20 + i), _frames(1, 30 + i)) for i in range(15)]
        assert None not in others and len(set(others + [b])) == 16
        assert s.add_scored(p, f) is None
        _run_all(s)
        assert all(s.poll_scores(sl)["logprob"].shape == (1, 9) for sl in others)


def test_collector_kinds_swap_slots_and_reuse_each_others_buffers(lm16):
    """A hidden-state collector and a scoring slot leave, and each kind is re-admitted into the slot the OTHER kind held: both tables
    and the two buffer pools meet here.  Reuse against fresh on the same handle: bit-equal, no tolerance."""
    L, N = 5, 3
    pa, pb, fb = _prompt(L, 61), _prompt(L, 62), _frames(N, 63)
    kw = dict(temp=0.0, top_p=1.0, top_k=0, seed=5, ignore_eos=True, per_slot=True, score=True, repetition_penalty=1.0)

    def second_round(s):  # B' (scored, collecting) first, then A': slots are handed out lowest-first
        b2 = s.add_scored(pb, fb, collect_hidden=True)
        a2 = s.add(pa, L + N - 2, seed=77, collect_hidden=True)
        rows0 = (s.poll_hidden(a2).shape[0], s.poll_hidden(b2).shape[0], s.poll_scores(b2)["logprob"].shape[0])
        _run_all(s)
        return a2, b2, rows0, s.poll(a2)[0], s.poll_hidden(a2), s.poll_scores(b2), s.poll_hidden(b2)

    with lm16.session(**kw) as s:  # the fresh run
        _, _, _, _, _, sc_ref, hid_b_ref = second_round(s)
    with lm16.session(**kw) as s:
        a = s.add(pa, L + N - 2, seed=77, collect_hidden=True)
        b = s.add_scored(pb, fb)
        assert (a, b) == (0, 1)
        _run_all(s)
        codes_a, hid_a, sc_b = s.poll(a)[0], s.poll_hidden(a), s.poll_scores(b)
        s.release(a)
        s.release(b)
        a2, b2, rows0, codes_a2, hid_a2, sc_b2, hid_b2 = second_round(s)
    assert (b2, a2) == (a, b), "each kind must land in the slot the other kind left"
    assert rows0 == (0, 0, 0), "a re-admitted slot of either kind starts at row 0"
    assert codes_a.shape == (8, N) and hid_a.shape == (N, CFG["dim"]) and sc_b["logprob"].shape == (N, 9)
    assert hid_a2.shape == hid_a.shape and hid_b2.shape == (N, CFG["dim"]) and sc_b2["logprob"].shape == (N, 9)
    assert np.array_equal(codes_a2, codes_a) and np.array_equal(hid_a2.view(np.uint32), hid_a.view(np.uint32)), "A' differs from A"
    for k in ("logprob", "top_logprob", "top", "eos_logprob"):
        assert np.array_equal(sc_b2[k].view(np.uint32), sc_ref[k].view(np.uint32)), f"B' {k}: reuse differs from fresh"
    assert np.array_equal(hid_b2[:N].view(np.uint32), hid_b_ref[:N].view(np.uint32)), "B' hidden rows: reuse differs from fresh"


def test_errors_name_their_field_and_leave_the_session_as_it_was(lm16):
    L = fishrt.lib()
    p, f = _prompt(19, 7), _frames(6, 8)
    samp = fishrt._ffi.Sampling(0.0, 1.0, 0, 1.0)
    for flags, word in ((64, b"not alone"), (64 | 8, b"FS_SESSION_ROWS"), (64 | 16 | 8, b"FS_SESSION_ROWS")):
        assert L.fs_lm_session_begin(lm16._h, C.byref(samp), C.c_uint64(1), flags) != 0
        assert b"FS_SESSION_SCORE" in L.fs_last_error() and word in L.fs_last_error(), L.fs_last_error()
    pp, ff = np.ascontiguousarray(p), np.ascontiguousarray(f)
    with lm16.session(temp=0.0, top_p=1.0, top_k=0, seed=1, per_slot=True) as s:  # no flag: both entry points refuse (C ABI: Python refuses earlier)
        slot, n = C.c_int(-1), C.c_size_t(0)
        g = s.add(p, 19 + 4)
        assert L.fs_lm_session_add_scored(lm16._h, -1, pp.ctypes.data_as(UP), 19, ff.ctypes.data_as(UP), 6, 0, C.byref(slot)) != 0
        assert b"needs FS_SESSION_SCORE" in L.fs_last_error()
        assert L.fs_lm_session_poll_scores(lm16._h, g, 0, None, None, None, None, 0, C.byref(n)) != 0
        assert b"needs FS_SESSION_SCORE" in L.fs_last_error()
        _run_all(s)
        assert s.poll(g)[0].shape == (8, 6)
    with lm16.session(temp=0.0, top_p=1.0, top_k=0, seed=1, per_slot=True, score=True) as s:
        pid = s.add_prefix(_prompt(37, 3))
        g = s.add(p, 19 + 4)
        sc = s.add_scored(p, f)
        s.step(1)  # (everything admitted so far is live: the pool only moves with what follows)
        free = s.info()["free_pages"]
        with pytest.raises(RuntimeError, match="not a scoring slot"):
            s.poll_scores(g)
        bad = {}
        bad["frames[0][2]"] = f.copy(); bad["frames[0][2]"][0, 2] = IM_END
        bad["frames[0][5]"] = f.copy(); bad["frames[0][5]"][0, 5] = SEM0 - 2
        bad["frames[0][0]"] = f.copy(); bad["frames[0][0]"][0, 0] = CFG["vocab_size"]
        bad["frames[3][1]"] = f.copy(); bad["frames[3][1]"][3, 1] = 1024
        for field, fr in bad.items():
            with pytest.raises(RuntimeError) as e:
                s.add_scored(p, fr)
            assert field in str(e.value) and ("codebook_size" if field == "frames[3][1]" else "semantic_start_id") in str(e.value), str(e.value)
        long = _frames(CFG["max_seq_len"] - 19 + 2, 9)  # L + N - 1 == max_seq_len + 1
        with pytest.raises(RuntimeError, match="max_seq_len"):
            s.add_scored(p, long)
        with pytest.raises(RuntimeError, match="max_seq_len"):  # (L counts the prefix)
            s.add_scored(p, _frames(CFG["max_seq_len"] - 19 - 37 + 2, 9), prefix=pid)
        with pytest.raises(RuntimeError, match="prefix"):
            s.add_scored(p, f, prefix=pid + 5)
        assert s.info()["free_pages"] == free, "a refused add must leave the page pool as it was"
        _run_all(s)
        assert s.poll(g)[0].shape == (8, 6) and s.poll_scores(sc)["logprob"].shape == (6, 9) and np.array_equal(s.poll(sc)[0], f[1:])
    # a Fish <= 1.4 handle (has_semantic_end == 0) has no slow-token distribution to score
    lm14 = fishrt.DualARTransformer(dict(fcfg.FISH_1_4, n_layer=3), fcfg.FISH_1_4_TOKENS, 0, "bf16", max_batch=4).load_synthetic(SEED)
    try:
        assert L.fs_lm_session_begin(lm14._h, C.byref(samp), C.c_uint64(1), 16 | 64) != 0
        assert b"FS_SESSION_SCORE" in L.fs_last_error() and b"Fish <= 1.4" in L.fs_last_error(), L.fs_last_error()
        with lm14.session(temp=0.0, top_p=1.0, top_k=0, seed=1, per_slot=True) as s:  # (the handle still takes its own session kind)
            pass
    finally:
        lm14.close()
