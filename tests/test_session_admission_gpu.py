"""GPU: admission to a continuous-batching session (fs_lm_session_add / _add_prefixed / _add_ex, include/fishrt.h).  A plain add IS a prefixed
add with an empty prefix: the two must give codes of the same shape, reserve the same pages beyond the prefix's full ones and generate the
same codes (parting only where the plain slot's own recorded logits hold a near-tie); a refused add (no free slot, KV page pool short)
returns None and leaves the page pool as it was; a slot whose budget passes max_seq_len stops there, where generate_blocking raises;
argument errors keep their messages; and every admission kind (plain, prefixed, own settings, hidden-state, scored, traced) refuses
without moving anything and admits the same slot whatever was refused before it."""
import ctypes as C
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import fishrt
from fishrt import _ffi
from fishrt import config as fcfg
from test_session_prefix_gpu import NEAR_TIE, SEED, _pages, _prompt

N_AUDIO = fcfg.TINY["vocab_size"] - fcfg.TINY_TOKENS["im_end_id"]
GREEDY = dict(temp=0.0, top_p=1.0, top_k=0, seed=42, ignore_eos=True)
U32P = C.POINTER(C.c_uint32)


def _tiny(**over):
    return fishrt.DualARTransformer(dict(fcfg.TINY, **over), fcfg.TINY_TOKENS, 0, "bf16", max_batch=2).load_synthetic(SEED)


@pytest.fixture(scope="module")
def lm():
    h = _tiny()
    yield h
    h.close()


def _run(s, slot):
    while not s.poll(slot, codes=False)[1]:
        s.step(8)
    return s.poll(slot)[0]


def _near_tie_gap(cap, a, b):
    """cap = the plain slot's recorded decisions [F][9][2048], a = its codes, b = the prefixed slot's: the smallest gap that can explain the
    first difference -- the two picks of that codebook decision, or the top two of the slow-token decision of that frame or the one before"""
    f = int(np.argmax((a != b).any(0)))
    c = int(np.argmax(a[:, f] != b[:, f]))
    lg = cap[f, 1 + c, : fcfg.TINY["codebook_size"]]
    gaps = [float(abs(lg[a[c, f]] - lg[b[c, f]]))]
    for g in (f, f - 1):
        if g >= 0:
            sl = np.sort(cap[g, 0, :N_AUDIO][np.isfinite(cap[g, 0, :N_AUDIO])])
            gaps.append(float(sl[-1] - sl[-2]))
    return f, c, min(gaps)


def test_a_plain_add_is_a_prefixed_add_of_the_same_columns(lm):
    rng = np.random.RandomState(11)
    F = 8
    lm.debug_capture(F)
    try:
        for P in (1, 63, 64, 65):
            for Lb in (1, 7):
                pre, body = _prompt(rng, P), _prompt(rng, Lb)
                full = np.concatenate([pre, body], 1)
                L = P + Lb
                m = L + F - 2
                shape = (8, 1 + max(0, m - L + 1))
                end = L + shape[1] - 1  # positions whose K/V the slot keeps
                with lm.session(**GREEDY) as s:
                    free0 = s.info()["free_pages"]
                    slot = s.add(full, m)
                    plain_pages = free0 - s.info()["free_pages"]
                    plain = _run(s, slot)
                cap = lm.debug_read_row(slot, F)
                with lm.session(**GREEDY) as s:
                    pid = s.add_prefix(pre)
                    free0 = s.info()["free_pages"]
                    slot = s.add(body, m, prefix=pid)
                    info = s.info()
                    prefixed_pages = free0 - info["free_pages"]
                    prefixed = _run(s, slot)
                assert plain.shape == prefixed.shape == shape, (P, Lb, plain.shape, prefixed.shape)
                # private pages: everything beyond the prefix's full pages (which the prefixed slot shares instead of taking)
                assert plain_pages == _pages(end), (P, Lb, plain_pages)
                assert plain_pages - P // 64 == prefixed_pages == _pages(end) - P // 64, (P, Lb, plain_pages, prefixed_pages)
                assert info["shared_pages"] == _pages(P), (P, Lb, info)  # (a partly filled last page is held until it has been copied)
                if np.array_equal(plain, prefixed):
                    print(f"P {P} body {Lb}: identical")
                    continue
                f, c, gap = _near_tie_gap(cap, plain.astype(np.int64), prefixed.astype(np.int64))
                print(f"P {P} body {Lb}: parts at frame {f} codebook {c} on a gap of {gap:.2e}")
                assert gap < NEAR_TIE, (P, Lb, f, c, gap)
    finally:
        lm.debug_capture(0)


def test_a_full_session_refuses_without_touching_the_pool(lm):
    rng = np.random.RandomState(12)
    pre, body = _prompt(rng, 70), _prompt(rng, 9)
    with lm.session(**GREEDY) as s:
        pid = s.add_prefix(pre)
        assert s.add(body, 40) == 0 and s.add(body, 70 + 9 + 20, prefix=pid) == 1
        before = s.info()
        assert before["shared_pages"] == 2  # the prefix's full page and, until it has been copied, its partly filled one
        assert s.add(body, 40) is None
        assert s.add(body, 70 + 9 + 20, prefix=pid) is None
        assert s.info() == before
        s.step(1)
        before = s.info()
        assert before["shared_pages"] == 1
        assert s.add(body, 40) is None
        assert s.add(body, 70 + 9 + 20, prefix=pid) is None
        assert s.info() == before


def test_a_short_pool_refuses_until_pages_come_back(lm):
    rng = np.random.RandomState(13)
    msl = fcfg.TINY["max_seq_len"]
    pre, body, long_p = _prompt(rng, 10), _prompt(rng, 6), _prompt(rng, 16)
    m = msl - 5  # L = 16 either way: the slot keeps K/V up to position L + (1 + m - L + 1) - 1 = m + 1
    need = _pages(m + 1)
    with lm.session(**GREEDY) as s:
        pid = s.add_prefix(pre)
        first = s.add(long_p, m)
        assert first == 0
        free = s.info()["free_pages"]
        assert 0 < free < need, (free, need)  # the second slot is free, the pages are not
        assert s.add(long_p, m) is None
        assert s.add(body, m, prefix=pid) is None
        assert s.info()["free_pages"] == free
        s.release(first)
        assert s.info()["free_pages"] == free + need
        again = s.add(long_p, m)
        assert again is not None and s.info()["free_pages"] == free
        s.release(again)
        again = s.add(body, m, prefix=pid)
        assert again is not None and s.info()["free_pages"] == free


def test_a_slot_stops_at_max_seq_len_where_generate_blocking_raises():
    msl, L = 128, 10
    h = _tiny(max_seq_len=msl)
    p = _prompt(np.random.RandomState(14), L)
    try:
        with h.session(**GREEDY) as s:
            slot = s.add(p, L + 3 * msl)
            codes = _run(s, slot)
            assert s.poll(slot, codes=False) == (msl - L + 1, True)
        assert codes.shape == (8, msl - L + 1)
        with pytest.raises(RuntimeError, match=re.escape("generation ran past max_seq_len without <|im_end|> (the reference fails at dual_ar.rs:623-624)")):
            h.generate_blocking(p, L + 3 * msl, temp=0.0, top_p=1.0, top_k=0, ignore_eos=True)
    finally:
        h.close()


def test_argument_errors_keep_their_messages(lm):
    rng = np.random.RandomState(15)
    msl = fcfg.TINY["max_seq_len"]
    L = _ffi.lib()
    pre, body = _prompt(rng, 40), _prompt(rng, 8)
    out = C.c_int(-7)

    def raises(msg):
        return pytest.raises(RuntimeError, match="^" + re.escape(msg) + "$")

    with lm.session(**GREEDY) as s:
        pid = s.add_prefix(pre)
        before = s.info()
        with raises("empty prompt"):
            _ffi.check(L.fs_lm_session_add(lm._h, body.ctypes.data_as(U32P), 0, 50, C.byref(out)))
        with raises("empty body (a prefixed add needs its last prompt column)"):
            _ffi.check(L.fs_lm_session_add_prefixed(lm._h, pid, body.ctypes.data_as(U32P), 0, 50, C.byref(out)))
        with raises("prompt exceeds max_seq_len (dual_ar.rs:623-624)"):
            s.add(_prompt(rng, msl + 1), msl + 10)
        with raises("prompt exceeds max_seq_len (dual_ar.rs:623-624)"):
            s.add(_prompt(rng, msl - 40 + 1), msl + 10, prefix=pid)
        with raises("unknown or released prefix id"):
            s.add(body, 50, prefix=pid + 5)
        with raises("per-slot sampling / seed need a session begun with FS_SESSION_PER_SLOT or FS_SESSION_ROWS (the lock-step sampler has one "
                    "setting and one stream per session)"):
            sa = _ffi.Sampling(0.7, 0.8, 50, 1.2)
            _ffi.check(L.fs_lm_session_add_ex(lm._h, -1, body.ctypes.data_as(U32P), 8, 50, C.byref(sa), None, C.byref(out)))
        assert s.info() == before and out.value == -7
        assert s.add(body, 50) == 0  # nothing above took a slot


# ------------------------------------------------------------------------------------------------ every admission kind, one path
# One request record and one admission function serve all six entry points: a refused add of ANY kind must leave the session exactly as
# it was (page pool, counters, slot order, what the live slots generate), and an admitted one must not depend on what was refused before it.
F15, TOK15 = fcfg.FISH_1_5, fcfg.FISH_1_5_TOKENS
KINDS = ("plain", "prefixed", "sampled", "hidden", "scored", "scored_hidden", "traced", "traced_hidden")
ON_PREFIX = ("prefixed", "scored_hidden", "traced_hidden")  # the valid add of these kinds is a body on the 37-column prefix
P37, N_SC = 37, 3  # 37 % 64 != 0: the prefix's partly filled last page is referenced until it has been copied
TOP_K_TEXT = "FS_SESSION_PER_SLOT: a slot samples greedy (temp == 0) or with temp > 0 and 0 < top_k <= 256 (the in-launch samplers' limit)"


@pytest.fixture(scope="module")
def lm16():
    h = fishrt.DualARTransformer(F15, TOK15, 0, "bf16", max_batch=16).load_synthetic(SEED)
    yield h
    h.close()


def _p15(L, seed):
    p = np.zeros((9, L), np.uint32)
    p[0] = np.random.RandomState(seed).randint(0, TOK15["im_end_id"], L)
    return p


def _f15(seed):
    rng = np.random.RandomState(seed)
    f = np.zeros((9, N_SC), np.uint32)
    f[0] = TOK15["semantic_start_id"] + rng.randint(0, F15["vocab_size"] - TOK15["semantic_start_id"], N_SC)
    f[1:] = rng.randint(0, F15["codebook_size"], (8, N_SC))
    return f


def _admit(s, kind, p, prefix=None, P=0, sampling=None, frames=None):
    """one add of `kind`: max_new_tokens = L + 2 (L counts the prefix), or the N_SC frames of a scoring slot"""
    hidden = kind.endswith("hidden")
    if kind.startswith("scored"):
        return s.add_scored(p, frames, prefix=prefix, collect_hidden=hidden)
    kw = dict(sampling=dict(temp=0.9, top_p=0.7, top_k=40), seed=77) if kind == "sampled" else {}
    if sampling is not None:
        kw["sampling"] = sampling
    return s.add(p, P + p.shape[1] + 2, prefix=prefix, collect_hidden=hidden, trace=kind.startswith("traced"), **kw)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _all_kinds(lm, refuse):
    """the session with (refuse=True) or without the refused adds; everything else -- the live slot, the probe after each refusal, one valid add
    per kind, the slots that fill the session -- is the same in both -> (codes of the live slot, {kind: what its slot left})"""
    msl = F15["max_seq_len"]
    pre, frames = _p15(P37, 1), _f15(2)
    bad = frames.copy()
    bad[3, 1] = F15["codebook_size"]

    def refused(s, kind, what, **kw):
        """one refusal, then: nothing moved, and the lowest free slot is still the next one handed out"""
        before, low = s.info(), min(set(range(16)) - set(taken))
        if refuse:
            with pytest.raises(RuntimeError, match="^" + re.escape(what) + "$"):
                _admit(s, kind, **kw)
            assert s.info() == before, (kind, what)
        probe = s.add(_p15(5, 3), 5 + 2)
        assert probe == low, (kind, what, probe, low)
        s.release(probe)
        assert s.info()["free_pages"] == before["free_pages"], (kind, what)

    with lm.session(temp=0.7, top_p=0.8, top_k=256, seed=3, ignore_eos=True, per_slot=True, score=True, trace=True) as s:
        pid = s.add_prefix(pre)
        taken = [s.add(_p15(19, 4), 19 + 2)]
        assert taken == [0] and s.step(1) == 1  # one generating slot is live
        for i, kind in enumerate(KINDS):
            on = kind in ON_PREFIX
            p = _p15(5 + 2 * i, 10 + i)  # 5 .. 19 columns
            ok = dict(p=p, prefix=pid if on else None, P=P37 if on else 0, frames=frames)
            scored = kind.startswith("scored")
            if kind != "plain":
                refused(s, kind, "unknown or released prefix id", **dict(ok, prefix=pid + 5))
            if kind in ("sampled", "hidden", "traced", "traced_hidden"):
                refused(s, kind, TOP_K_TEXT, **dict(ok, sampling=dict(top_k=300)))
            L_long = msl + 1 - ok["P"]
            refused(s, kind, f"L + N - 1 = {msl + N_SC} exceeds max_seq_len (L counts the prefix; a scored sequence is never clipped)" if scored
                    else "prompt exceeds max_seq_len (dual_ar.rs:623-624)", **dict(ok, p=_p15(L_long, 5)))
            if scored:
                refused(s, kind, f"frames[3][1] = {F15['codebook_size']}: a code must be < codebook_size", **dict(ok, frames=bad))
            taken.append(_admit(s, kind, **ok))
            assert taken[-1] == 1 + i, (kind, taken)
        fill = [s.add(_p15(6, 20 + j), 6 + 2) for j in range(16 - len(taken))]
        assert fill == list(range(len(taken), 16))
        taken += fill
        if refuse:  # all slots taken: every kind answers None, and nothing moves
            for i, kind in enumerate(KINDS):
                on = kind in ON_PREFIX
                before = s.info()
                assert _admit(s, kind, p=_p15(5 + 2 * i, 10 + i), prefix=pid if on else None, P=P37 if on else 0, frames=frames) is None, kind
                assert s.info() == before, kind
        for b in fill:
            s.release(b)
            taken.remove(b)
        probe = s.add(_p15(5, 3), 5 + 2)  # the session has free slots again: the lowest one first
        assert probe == len(taken)
        s.release(probe)
        while s.step(8):
            pass
        out = {}
        for i, kind in enumerate(KINDS):
            b = 1 + i
            got = dict(codes=s.poll(b)[0])
            assert s.poll(b, codes=False) == (N_SC if kind.startswith("scored") else 4, True), kind
            if kind.endswith("hidden"):
                got["hidden"] = s.poll_hidden(b)
                assert got["hidden"].shape == (got["codes"].shape[1], F15["dim"]), kind
            if kind.startswith("scored"):
                got.update(s.poll_scores(b))
                assert np.array_equal(got["codes"], frames[1:]) and got["logprob"].shape == (N_SC, 9), kind
            if kind.startswith("traced"):
                got.update(s.poll_trace(b))
                assert np.array_equal(got["tokens"][:, 1:].T, got["codes"]), kind
            out[kind] = got
        return s.poll(0)[0], out


def test_every_admission_kind_refuses_cleanly_and_admits_the_same(lm16):
    live_a, kinds_a = _all_kinds(lm16, refuse=True)
    live_b, kinds_b = _all_kinds(lm16, refuse=False)  # the fresh session: the same adds, nothing refused
    assert live_a.shape == (8, 4) and np.array_equal(live_a, live_b)
    for kind in KINDS:
        assert kinds_a[kind].keys() == kinds_b[kind].keys(), kind
        for key, a in kinds_a[kind].items():
            b = kinds_b[kind][key]
            assert a.shape == b.shape and a.size > 0 and np.array_equal(_bits(a), _bits(b)), (kind, key)
