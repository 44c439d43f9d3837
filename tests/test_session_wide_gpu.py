"""GPU: FS_SESSION_PER_SLOT | FS_SESSION_WIDE_SAMPLER (include/fishrt.h) -- a per-slot session whose slots may also sample nucleus-only
(top_k == 0) or with 256 < top_k.  Every decision of every slot is refereed by the oracle's LogitsProcessor on the slot's captured rows
(the scheme of tests/test_session_per_slot_gpu.py); settings inside the narrow limit give the same codes with and without the flag; a wide
slot does not depend on its neighbours; the flag's errors; sessions without the flag are what they were; Fish <= 1.4 handles keep their
2-way slow draw.  Fish-1.5 / Fish-1.4 shapes, synthetic weights."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import fishrt
from fishrt import config as fcfg
from test_session_per_slot_gpu import SEED, TOK, _picks, _prompt, _replay, _run_all

F = 12  # refereed frames per slot

# the seven slots of the heterogeneous test: (temp, top_p, top_k, penalty); on Fish 1.5 the slow decision has n = 2037 candidates and a
# codebook 1024, so top_k = 1500 is a top-k decision on the slow token and nucleus-only on the codebooks
SLOTS = [dict(temp=0.7, top_p=0.8, top_k=0, amt=1.4), dict(temp=1.0, top_p=1.0, top_k=0, amt=1.0), dict(temp=0.7, top_p=0.9, top_k=300, amt=1.0),
         dict(temp=1.0, top_p=0.8, top_k=1500, amt=1.0), dict(temp=0.7, top_p=0.8, top_k=256, amt=1.0), dict(temp=0.7, top_p=0.9, top_k=50, amt=1.0),
         dict(temp=0.0, top_p=1.0, top_k=0, amt=1.0)]


def _kw(d):
    return dict(temp=d["temp"], top_p=d["top_p"], top_k=d["top_k"])


def _is_wide(d):
    return d["temp"] > 0 and (d["top_k"] == 0 or d["top_k"] > 256)


@pytest.fixture(scope="module")
def lm16():
    lm = fishrt.DualARTransformer(fcfg.FISH_1_5, TOK, 0, "bf16", max_batch=16).load_synthetic(SEED)
    yield lm
    lm.close()


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_every_decision_of_heterogeneous_wide_slots_is_refereed_by_the_oracle(dtype):
    """7 requests join one per round -- two nucleus-only, two with a wide top-k, two inside the narrow limit, one greedy -- and run F + 1
    frames with the decision capture armed.  For every slot: the captured picks are the returned codes, and its raw rows replayed through
    the oracle's repetition penalty and ONE LogitsProcessor stream reproduce all (F + 1) x 9 picks.  The 9 decisions of frame F draw from
    the stream position the first F frames left behind, so their equality is the check that the position after F x 9 decisions is the
    oracle's (the hook test compares the word count itself).
    Not served by a clamped top-k: for at least one wide slot the oracle replay of the captured rows with top_k = 256 gives other picks.
    Temperature used for that: the table's own values (0.7 / 1.0).  The synthetic heads give flat rows (tests/test_sampler_gpu.py models
    them as unit-variance logits), on which the candidates outside the 256 largest carry about half of the weight at these temperatures;
    the test prints the number of differing picks per wide slot."""
    n = len(SLOTS)
    lm = fishrt.DualARTransformer(fcfg.FISH_1_5, TOK, 0, dtype, max_batch=16).load_synthetic(SEED)
    reqs = [dict(p=_prompt(14 + 9 * i, 2300 + i), d=SLOTS[i], seed=7000 + 13 * i) for i in range(n)]
    lm.debug_capture(F + 1)
    try:
        with lm.session(temp=0.7, top_p=0.8, top_k=0, seed=3, ignore_eos=True, per_slot=True, wide=True, repetition_penalty=1.4) as s:
            assert s.wide
            slots = []
            for r in reqs:  # one join per round: each request meets the others mid-flight
                slots.append(s.add(r["p"], r["p"].shape[1] + F + 1 - 2, sampling=dict(_kw(r["d"]), repetition_penalty=r["d"]["amt"]), seed=r["seed"]))
                assert slots[-1] is not None
                s.step(2)
            _run_all(s)
            outs = [s.poll(sl)[0] for sl in slots]
        caps = [lm.debug_read_row(sl, F + 1) for sl in slots]
    finally:
        lm.debug_capture(0)
        lm.close()
    assert len(set(slots)) == n
    clamp_differs = []
    for r, sl, codes, cap in zip(reqs, slots, outs, caps):
        d = r["d"]
        assert codes.shape == (8, F + 1), (sl, codes.shape)
        got = _picks(cap)
        assert np.array_equal(got[:, 1:].T, codes.astype(np.int64)), f"slot {sl}: captured picks are not the returned codes"
        assert np.isneginf(cap[:, 0, 0]).all(), "ignore_eos must mask the <|im_end|> logit"
        exp, moved = _replay(cap, r["seed"], _kw(d), d["amt"])
        bad = np.argwhere(got != exp)
        print(f"{dtype} slot {sl} {d}: {(F + 1) * 9 - len(bad)}/{(F + 1) * 9} decisions identical to the oracle replay")
        assert bad.size == 0, f"slot {sl} {d}: {len(bad)} of {(F + 1) * 9} decisions differ from the oracle, first (frame, decision) {bad[0]}: gpu {got[tuple(bad[0])]} oracle {exp[tuple(bad[0])]}"
        if d["amt"] != 1.0:
            assert moved, "a penalised entry of frame 1 must differ from the raw logit"
        if _is_wide(d):
            clamped = _replay(cap, r["seed"], dict(_kw(d), top_k=256), d["amt"])[0]
            clamp_differs.append(int((clamped != exp).sum()))
            print(f"   oracle replay with top_k = 256 instead: {clamp_differs[-1]} of {(F + 1) * 9} picks differ")
    assert len(clamp_differs) == 4 and max(clamp_differs) > 0, "no wide slot's picks depend on its top_k: a clamped top-k would pass this test"


NARROW3 = [dict(temp=0.7, top_p=0.8, top_k=256, repetition_penalty=1.4), dict(temp=1.0, top_p=0.9, top_k=50, repetition_penalty=1.2),
           dict(temp=0.0, top_p=1.0, top_k=0, repetition_penalty=1.2)]


def _three_narrow(lm, **sess_kw):
    with lm.session(temp=0.7, top_p=0.8, top_k=256, seed=21, ignore_eos=True, per_slot=True, repetition_penalty=1.4, **sess_kw) as s:
        slots = []
        for i, kw in enumerate(NARROW3):
            p = _prompt(17 + 6 * i, 3100 + i)
            slots.append(s.add(p, p.shape[1] + F - 2, sampling=kw, seed=600 + i))
            s.step(1)
        _run_all(s)
        return [s.poll(sl)[0] for sl in slots]


def test_narrow_settings_give_the_same_codes_with_and_without_the_flag(lm16):
    a = _three_narrow(lm16)
    b = _three_narrow(lm16, wide=True)
    for x, y in zip(a, b):
        assert x.shape == y.shape == (8, F)
        assert np.array_equal(x, y), f"first differing frame {int(np.argmax((x != y).any(0)))}"
    assert not np.array_equal(a[0], a[1])


def test_a_wide_slot_does_not_depend_on_its_neighbours_or_its_slot(lm16):
    FR = 20
    p, kw, seed = _prompt(33, 78), dict(temp=0.8, top_p=0.85, top_k=0, repetition_penalty=1.4), 515151
    with lm16.session(seed=1, ignore_eos=True, per_slot=True, wide=True) as s:
        sl = s.add(p, 33 + FR - 2, sampling=kw, seed=seed)
        assert sl == 0
        _run_all(s)
        alone = s.poll(sl)[0]
    others = [dict(p=_prompt(10 + 7 * i, 900 + i), F=6 + 4 * i, kw=dict(_kw(SLOTS[i]), repetition_penalty=SLOTS[i]["amt"])) for i in range(7)]
    with lm16.session(temp=1.0, top_p=0.9, top_k=700, seed=99, ignore_eos=True, per_slot=True, wide=True) as s:
        for o in others[:3]:
            assert s.add(o["p"], o["p"].shape[1] + o["F"] - 2, sampling=o["kw"], seed=o["F"]) is not None
            s.step(1)
        sl = s.add(p, 33 + FR - 2, sampling=kw, seed=seed)
        assert sl == 3
        for o in others[3:]:
            s.step(2)
            assert s.add(o["p"], o["p"].shape[1] + o["F"] - 2, sampling=o["kw"], seed=o["F"]) is not None
        _run_all(s, 5)
        among = s.poll(sl)[0]
    assert alone.shape == among.shape == (8, FR)
    assert np.array_equal(alone, among), f"first differing frame {int(np.argmax((alone != among).any(0)))}"


def test_errors_and_sessions_without_the_flag_stay_as_they_were(lm16):
    L = fishrt.lib()
    p0 = _prompt(20, 31)
    narrow = dict(temp=0.7, top_p=0.8, top_k=256)

    def narrow_session_codes():
        """a session WITHOUT the flag: refuses top_k = 0 / 257 by the name of its limit, and a fixed request's codes"""
        with lm16.session(seed=4, ignore_eos=True, per_slot=True, **narrow) as s:
            for bad in (dict(temp=0.7, top_p=0.8, top_k=0), dict(temp=0.7, top_p=0.8, top_k=257)):
                with pytest.raises(RuntimeError, match="top_k <= 256"):
                    s.add(p0, 20 + F - 2, sampling=bad)
            sl = s.add(p0, 20 + F - 2, sampling=dict(narrow, repetition_penalty=1.4), seed=111)
            _run_all(s)
            return s.poll(sl)[0]

    before = narrow_session_codes()
    with lm16.session(temp=0.9, top_p=0.7, top_k=0, seed=4, ignore_eos=True, per_slot=True, wide=True) as s:
        a = s.add(p0, 20 + F - 2, sampling=dict(temp=0.7, top_p=0.8, top_k=257, repetition_penalty=1.4), seed=111)
        b = s.add(p0, 20 + F - 2)  # the session's own nucleus-only setting
        with pytest.raises(RuntimeError, match="top_p"):
            s.add(p0, 20 + F - 2, sampling=dict(temp=0.7, top_p=float("nan"), top_k=0))
        with pytest.raises(RuntimeError, match="temp"):
            s.add(p0, 20 + F - 2, sampling=dict(temp=float("inf"), top_p=0.8, top_k=0))
        # (a negative temp through the C ABI: Session.add refuses it before the call)
        slot, neg = C.c_int(-1), fishrt._ffi.Sampling(-0.5, 0.8, 0, 1.2)
        pp = np.ascontiguousarray(p0)
        assert L.fs_lm_session_add_ex(lm16._h, -1, pp.ctypes.data_as(C.POINTER(C.c_uint32)), 20, 20 + F - 2, C.byref(neg), None, C.byref(slot)) != 0
        assert b"temp" in L.fs_last_error()
        _run_all(s)
        wide_codes = s.poll(a)[0]
        assert wide_codes.shape == s.poll(b)[0].shape == (8, F)
    after = narrow_session_codes()
    assert np.array_equal(before, after), "a wide session leaked into the narrow session that follows it (or its step graph was reused)"
    assert not np.array_equal(wide_codes, before)
    ok = fishrt._ffi.Sampling(0.7, 0.8, 0, 1.4)
    for flags, msg in ((32, b"only together with FS_SESSION_PER_SLOT"), (32 | 8, b"only together with FS_SESSION_PER_SLOT"),
                       (32 | 16 | 8, b"FS_SESSION_ROWS")):
        assert L.fs_lm_session_begin(lm16._h, C.byref(ok), C.c_uint64(1), flags) != 0
        assert msg in L.fs_last_error(), L.fs_last_error()
    for bad, msg in ((fishrt._ffi.Sampling(-1.0, 0.8, 0, 1.4), b"temp"), (fishrt._ffi.Sampling(0.7, float("nan"), 0, 1.4), b"top_p")):
        assert L.fs_lm_session_begin(lm16._h, C.byref(bad), C.c_uint64(1), 16 | 32) != 0
        assert msg in L.fs_last_error(), L.fs_last_error()
    assert L.fs_lm_session_begin(lm16._h, C.byref(ok), C.c_uint64(1), 16) != 0 and b"top_k <= 256" in L.fs_last_error()
    assert np.array_equal(narrow_session_codes(), before)  # no refused begin left a session open or the handle changed


def test_legacy_handle_wide_slot_keeps_the_two_way_slow_draw():
    """Fish <= 1.4 tokens: a nucleus-only slot takes ONE stream word per frame for the 2-way {pad, im_end} slow draw (u is checked against
    the stream's word at the slot's position), and its 8 codebook decisions per frame replay exactly through the oracle's nucleus sampler"""
    from test_session_legacy_gpu import F as FL, _check_slot, _lm, _prompt as _lprompt
    kw = dict(temp=0.9, top_p=0.8, top_k=0)
    lm = _lm("bf16")
    p = _lprompt(20, 31)
    lm.debug_capture(FL)
    try:
        with lm.session(temp=0.7, top_p=0.8, top_k=256, seed=4, ignore_eos=True, per_slot=True, wide=True) as s:
            a = s.add(p, 20 + FL - 2, sampling=dict(kw, repetition_penalty=1.3), seed=333)
            b = s.add(p, 20 + FL - 2, sampling=dict(temp=0.7, top_p=0.9, top_k=600, repetition_penalty=1.0), seed=334)
            _run_all(s)
            codes_a, codes_b = s.poll(a)[0], s.poll(b)[0]
        cap_a, cap_b = lm.debug_read_row(a, FL), lm.debug_read_row(b, FL)
    finally:
        lm.debug_capture(0)
        lm.close()
    assert _check_slot(cap_a, codes_a, 333, kw, 1.3, FL, ignore_eos=True) is None
    assert _check_slot(cap_b, codes_b, 334, dict(temp=0.7, top_p=0.9, top_k=600), 1.0, FL, ignore_eos=True) is None
    assert len(set(cap_a[:, 0, 2].tolist())) > FL // 2, "the recorded draws do not move along the stream"
