"""GPU: session prefixes made from a slot's history (fs_lm_session_prefix_from_slot / fs_lm_session_last_frame, include/fishrt.h).
The K/V rows of the promoted prefix must be the slot's own rows, bit for bit; a fork admitted on it with the slot's last frame must
continue the slot bit for bit; finished sources (budget, <|im_end|>) must never write a page the prefix shares; a real body prefilled over
decode-written history must agree with the oracle's one-prompt run of the concatenated tokens; the prefix is an ordinary one (export /
import / release / session end / chains of turns); pages are accounted exactly; every error has its message; and the other slots of a
session with a promotion are untouched.  TINY (head_dim 32) and MID (head_dim 64) configurations: max_seq_len 256, 64-token pages."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import fishrt
from fishrt import _ffi
from fishrt import config as fcfg
from oracle import oracle as orc

SEED = 0xF15E5EED
NEAR_TIE = 5e-3  # the constant of tests/test_session_prefix_gpu.py
MID = dict(fcfg.TINY, dim=256, n_head=4, n_local_heads=2, head_dim=64, intermediate_size=1024)
SEM0 = fcfg.TINY_TOKENS["semantic_start_id"]
GREEDY = dict(temp=0.0, top_p=1.0, top_k=0, seed=42, ignore_eos=True)
HANDLES = {"hd32": (fcfg.TINY, "bf16"), "hd64": (MID, "bf16"), "hd64-fp8": (MID, "fp8")}
COUNTERS = ("free_pages", "shared_pages", "live_prefixes", "prefill_passes", "tokens_prefilled", "prefix_tokens_reused", "tail_pages_copied")
_handles = {}


def _handle(name):
    """one 8-slot handle per configuration for the whole module (pool: 32 pages, one of them the session's scratch page)"""
    if name not in _handles:
        cfg, dtype = HANDLES[name]
        _handles[name] = fishrt.DualARTransformer(cfg, fcfg.TINY_TOKENS, 0, dtype, max_batch=8).load_synthetic(SEED)
    return _handles[name]


def _prompt(rng, L):
    p = np.zeros((9, L), np.uint32)
    p[0] = rng.randint(0, 400, L)
    k = min(L - 1, 5)
    if k > 0:  # a VQ span so that codebook embeddings take part
        p[0, 1 : 1 + k] = SEM0 + rng.randint(0, 64, k)
        p[1:, 1 : 1 + k] = rng.randint(0, 64, (8, k))
    return p


def _frames(rng, N):
    f = np.zeros((9, N), np.uint32)
    f[0] = SEM0 + rng.randint(0, 64, N)
    f[1:] = rng.randint(0, 64, (8, N))
    return f


def _rows(lm, slot, n):
    """K / V rows [0, n) of every slow layer of a slot"""
    return [lm.debug_read_kv(layer, 0, n, slot=slot) for layer in range(lm.cfg["n_layer"])]


def _same_rows(got, ref, P):
    return all(np.array_equal(gk[:P], rk[:P]) and np.array_equal(gv[:P], rv[:P]) for (gk, gv), (rk, rv) in zip(got, ref))


def _live(s, slot):
    """step until the slot has left its prefill (it has emitted a frame)"""
    for _ in range(8):
        if s.poll(slot, codes=False)[0] > 0:
            return
        s.step(1)
    raise AssertionError("the slot did not go live")


def _drain(s, live, results):
    while live:
        s.step(8)
        for slot in list(live):
            if s.poll(slot, codes=False)[1]:
                results[live.pop(slot)] = s.poll(slot)[0]
                s.release(slot)


def _info(s):
    i = s.info()
    return {k: i[k] for k in COUNTERS}


# ---- 1. the rows are the slot's rows
@pytest.mark.parametrize("name", ["hd32", "hd64", "hd64-fp8"])
def test_promoted_rows_are_the_slots_rows(name):
    """a joiner on the promoted prefix reads, at rows [0, P) of every layer, the bytes the source held before the call: histories that end
    one short of a page, on a page and one past it, cuts inside the prompt, on a page boundary and inside a page of a longer history"""
    lm = _handle(name)
    rng = np.random.RandomState(41)
    L = 40
    with lm.session(**GREEDY) as s:
        for T, cuts in ((63, (None,)), (64, (None,)), (65, (None,)), (100, (None, 37, 64, 70)), (128, (None,))):
            n = T - L + 1
            src = s.add(_prompt(rng, L), L + n + 40)
            s.step(n)
            assert s.poll(src, codes=False) == (n, False)
            ref = _rows(lm, src, T)  # (before the call)
            col = s.last_frame(src)
            assert np.array_equal(col[1:], s.poll(src)[0][:, n - 1]) and col[0] >= SEM0
            for cut in cuts:
                pid, P = s.prefix_from_slot(src, cut)
                assert pid is not None and P == (T if cut is None else cut), (T, cut, pid, P)
                j = s.add(col[:, None] if cut is None else _prompt(rng, 1), P + 1 + 4, prefix=pid)
                assert j is not None
                _live(s, j)  # (the source steps on underneath: it writes rows >= T only)
                assert _same_rows(_rows(lm, j, P), ref, P), (name, T, cut)
                s.release(j)
                s.release_prefix(pid)
            assert _same_rows(_rows(lm, src, T), ref, T), (name, T)
            s.release(src)
        info = s.info()
        assert info["live_prefixes"] == 0 and info["shared_pages"] == 0


# ---- 2. a fork continues its source bit for bit
@pytest.mark.parametrize("T", [64, 100])
@pytest.mark.parametrize("per_slot", [False, True], ids=["plain", "per-slot"])
@pytest.mark.parametrize("name", ["hd32", "hd64"])
def test_a_fork_continues_its_source_bit_for_bit(name, per_slot, T):
    lm = _handle(name)
    rng = np.random.RandomState(100 + T)
    L, m = 30, 12
    n = T - L + 1
    p = _prompt(rng, L)
    kw = dict(GREEDY, per_slot=True, repetition_penalty=1.0) if per_slot else GREEDY
    ref, got = {}, {}
    with lm.session(**kw) as s:  # the same request in a session without the promotion
        _drain(s, {s.add(p, L + (n + m) - 2): "A"}, ref)
    assert ref["A"].shape == (8, n + m)
    with lm.session(**kw) as s:
        a = s.add(p, L + (n + m) - 2)
        s.step(n)
        assert s.poll(a, codes=False) == (n, False)
        pid, P = s.prefix_from_slot(a)
        assert pid is not None and P == T
        col = s.last_frame(a)
        live = {a: "A"}
        for tag in ("B1", "B2"):  # two forks on one prefix
            b = s.add(col[:, None], (T + 1) + m - 2, prefix=pid)
            assert b is not None
            live[b] = tag
        _drain(s, live, got)
    assert np.array_equal(got["A"], ref["A"]), "the source's own codes changed"
    for tag in ("B1", "B2"):
        assert got[tag].shape == (8, m)
        assert np.array_equal(got[tag], ref["A"][:, n : n + m]), (tag, np.argwhere(got[tag] != ref["A"][:, n : n + m])[:3])


# ---- 3. frozen sources do not touch shared pages
def _frozen_source_keeps_off_shared_pages(lm, s, src, T, step_others):
    """src is finished with T % 64 == 0 history positions: promote it, let the session run 70 more steps, release it -- the rows read
    through joined slots stay the rows read at promotion"""
    n, done = s.poll(src, codes=False)
    assert done and T % 64 == 0
    ref = _rows(lm, src, T)
    before = s.info()
    pid, P = s.prefix_from_slot(src)
    assert pid is not None and P == T
    after = s.info()
    assert after["free_pages"] == before["free_pages"] and after["tail_pages_copied"] == before["tail_pages_copied"]  # aligned: no page taken
    col = s.last_frame(src)
    j = s.add(col[:, None], T + 1 + 100, prefix=pid)
    _live(s, j)
    assert _same_rows(_rows(lm, j, P), ref, P)
    step_others(70)  # (the source is not released: a frozen slot rides every replay of the step graph)
    assert _same_rows(_rows(lm, j, P), ref, P), "a frozen source wrote into a page its prefix shares"
    s.release(src)
    j2 = s.add(col[:, None], T + 1 + 4, prefix=pid)
    _live(s, j2)
    step_others(2)
    assert _same_rows(_rows(lm, j, P), ref, P) and _same_rows(_rows(lm, j2, P), ref, P)


@pytest.mark.parametrize("name", ["hd32", "hd64"])
def test_a_budget_finished_source_keeps_off_the_shared_pages(name):
    lm = _handle(name)
    rng = np.random.RandomState(7)
    L, N = 30, 35  # T = L + N - 1 = 64: the slot's whole allocation is shared
    with lm.session(**GREEDY) as s:
        src = s.add(_prompt(rng, L), L + N - 2)
        x = s.add(_prompt(rng, 20), 20 + 160)  # another live slot
        s.step(N + 3)
        assert s.poll(src, codes=False) == (N, True)

        def step_others(k):
            s.step(k)
            assert not s.poll(x, codes=False)[1]

        _frozen_source_keeps_off_shared_pages(lm, s, src, L + N - 1, step_others)


# (prompt length, prompt seed) of requests that end on <|im_end|> after n frames with (L + n - 1) % 64 == 0 on the EOS-boosted checkpoint
# below (greedy per-slot, repetition penalty 1.0); found by running candidates, and asserted again by the test
EOS_SOURCES = ((93, 0), (122, 2))  # 36 and 7 frames: T = 128


def _eos_lm(tmp_path):
    import test_safetensors_gpu as tsf
    from test_rows_gpu import EOS_BOOST, EOS_CFG, EOS_TOK
    t = tsf._lm_tensors(EOS_CFG, bf16=True)
    t["output.weight"][EOS_TOK["im_end_id"]] *= np.float32(EOS_BOOST)
    t["output.weight"] = (t["output.weight"].view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    path = str(tmp_path / "model.safetensors")
    tsf._save(t, path, True)
    lm = fishrt.DualARTransformer(EOS_CFG, EOS_TOK, 0, "bf16", max_batch=4).load_safetensors(path)
    os.remove(path)
    return lm


def test_an_im_end_finished_source_keeps_off_the_shared_pages(tmp_path):
    """the EOS-boosted checkpoint of tests/test_session_per_slot_gpu.py::test_eos_ends_a_slot_like_its_own_generate_call: the source ends on
    <|im_end|> (asserted) with its frozen write target on row T = 64 k, the first row of the page behind the shared ones"""
    from test_rows_gpu import EOS_TOK, _eos_prompt
    lm = _eos_lm(tmp_path)
    try:
        L, seed = EOS_SOURCES[0]
        M = 80
        rng = np.random.RandomState(3)
        with lm.session(temp=0.0, top_p=1.0, top_k=0, seed=42, per_slot=True, score=True, repetition_penalty=1.0) as s:
            src = s.add(_eos_prompt(L, seed), L + M)
            # another live slot that cannot end early: a scoring slot forced along 200 frames
            fr = np.zeros((9, 200), np.uint32)
            fr[0] = EOS_TOK["semantic_start_id"] + rng.randint(0, 1024, 200)
            fr[1:] = rng.randint(0, 1024, (8, 200))
            x = s.add_scored(_eos_prompt(12, 999), fr)
            s.step(M + 2)
            n, done = s.poll(src, codes=False)
            assert done and 2 <= n <= M, f"the source did not end on <|im_end|> ({n} frames of a budget of {M + 2})"
            assert (L + n - 1) % 64 == 0, (L, n)

            def step_others(k):
                s.step(k)
                assert not s.poll(x, codes=False)[1]

            _frozen_source_keeps_off_shared_pages(lm, s, src, L + n - 1, step_others)
    finally:
        lm.close()


# ---- 4. a real body on decode-written history agrees with the oracle
# (P, body columns, seed): the six requests.  Seeds scanned with the oracle on the CPU for a smallest top-2 margin >= NEAR_TIE over all
# frames of the oracle's run (the test asserts it again before it looks at the engine's codes)
ORACLE_FRAMES = 8
ORACLE_REQUESTS = ((70, 2, 6), (70, 17, 8), (70, 40, 9), (128, 2, 5), (128, 17, 6), (128, 40, 2))
ORACLE_L = 30


def _oracle_request(P, Lb, seed):
    """-> (source prompt [9, 30], forced frames [9, N] with 30 + N - 1 == P, body [9, Lb]); the history is prompt + frames[:, :N - 1]"""
    rng = np.random.RandomState(5000 + 1000 * seed + 10 * P + Lb)
    N = P - ORACLE_L + 1
    return _prompt(rng, ORACLE_L), _frames(rng, N), _prompt(rng, Lb)


def _oracle_mid():
    o = orc.OracleLM(orc.TINY | {k: MID[k] for k in ("dim", "n_head", "n_local_heads", "head_dim", "intermediate_size")})
    o.load_synthetic(SEED, bf16=True)
    o.set_kv_round_bf16(True)
    return o


def test_a_body_on_decode_written_history_agrees_with_the_oracle():
    """the source is a scoring slot forced along chosen frames, so every history token is known; the continuing slot is per-slot greedy
    (penalty 1.0) with a body of 2 / 17 / 40 columns prefilled over the promoted pages from a mid-page (P = 70) and a page-aligned
    (P = 128) start; the reference is the oracle's one-prompt run of concat(history, body) with bf16-rounded K/V"""
    lm, o = _handle("hd64"), _oracle_mid()
    reqs = [_oracle_request(*r) for r in ORACLE_REQUESTS]
    full, exp = [], []
    for (P, Lb, seed), (p, fr, body) in zip(ORACLE_REQUESTS, reqs):
        f = np.concatenate([p, fr[:, : fr.shape[1] - 1], body], 1)
        assert f.shape[1] == P + Lb
        full.append(f)
        exp.append(o.generate_batch([f], f.shape[1] + ORACLE_FRAMES - 2, seed=42, temp=0.0, top_p=1.0, top_k=0, ignore_eos=True)[0])
        margin = float(o.last_batch_margins[:, 0].min())
        print(f"P {P} body {Lb} seed {seed}: smallest oracle margin {margin:.3e}")
        assert exp[-1].shape == (8, ORACLE_FRAMES) and margin >= NEAR_TIE, (P, Lb, seed, margin)
    got = {}
    with lm.session(**dict(GREEDY, per_slot=True, score=True, repetition_penalty=1.0)) as s:
        srcs = [s.add_scored(p, fr) for p, fr, _ in reqs]
        assert None not in srcs
        while s.step(8):
            pass
        pids = []
        for (P, _, _), src, (_, fr, _) in zip(ORACLE_REQUESTS, srcs, reqs):
            assert s.poll(src, codes=False) == (fr.shape[1], True)
            pid, got_P = s.prefix_from_slot(src)
            assert pid is not None and got_P == P
            pids.append(pid)
            s.release(src)
        live = {}
        for i, ((P, Lb, _), (_, _, body)) in enumerate(zip(ORACLE_REQUESTS, reqs)):
            live[s.add(body, P + Lb + ORACLE_FRAMES - 2, prefix=pids[i], seed=i)] = i  # (a seed of its own: a pass of its own)
        assert None not in live
        _drain(s, live, got)
    bad = [(ORACLE_REQUESTS[i], int(np.argmax((got[i] != exp[i]).any(0)))) for i in range(len(reqs)) if not np.array_equal(got[i], exp[i])]
    assert not bad, f"(request, first differing frame): {bad}"


# ---- 5. it is an ordinary prefix
def test_a_promoted_prefix_exports_imports_and_outlives_its_uses():
    lm = _handle("hd64")
    lm2 = fishrt.DualARTransformer(MID, fcfg.TINY_TOKENS, 0, "bf16", max_batch=8).load_synthetic(SEED)
    rng = np.random.RandomState(55)
    kw = dict(temp=0.7, top_p=0.8, top_k=50, seed=5, ignore_eos=True, per_slot=True)
    L, T = 30, 70
    p, tail = _prompt(rng, L), _prompt(rng, 9)
    got = {}
    with lm.session(**kw) as s:
        free0 = s.info()["free_pages"]
        src = s.add(p, L + 100, seed=7)
        s.step(T - L + 1)
        pid, P = s.prefix_from_slot(src)
        assert P == T
        blob = s.export_prefix(pid)
        assert fishrt.prefix_blob_info(blob)["P"] == T
        body = np.concatenate([s.last_frame(src)[:, None], tail], 1)
        b = s.add(body, T + 10 + 19, prefix=pid, seed=99)
        s.step(1)
        s.release_prefix(pid)  # while a slot uses it (and the source still shares its page)
        assert s.info()["live_prefixes"] == 0
        s.release(src)
        _drain(s, {b: "own"}, got)
        assert s.info()["free_pages"] == free0 and s.info()["shared_pages"] == 0
        # session end with a promoted prefix live and a slot on it
        src = s.add(p, L + 100, seed=7)
        s.step(T - L + 1)
        pid, _ = s.prefix_from_slot(src)
        assert s.add(body, T + 10 + 19, prefix=pid, seed=99) is not None
    with lm.session(**kw) as s:
        info = s.info()
        assert info["free_pages"] == free0 and info["shared_pages"] == 0 and info["live_prefixes"] == 0, info
    with lm2.session(**kw) as s:  # a second handle with the same weights
        pid = s.import_prefix(blob)
        assert pid is not None
        _drain(s, {s.add(body, T + 10 + 19, prefix=pid, seed=99): "imported"}, got)
    lm2.close()
    assert got["own"].shape == (8, 21) and np.array_equal(got["own"], got["imported"])


@pytest.mark.parametrize("name", ["hd32", "hd64"])
def test_a_chain_of_three_turns_through_continue_from(name):
    """three turns of 10 frames with empty bodies are one slot of 30 frames, bit for bit (per-slot greedy, penalty 1.0); turns with a
    real body keep the rows of the turns before them; and every page comes back"""
    lm = _handle(name)
    rng = np.random.RandomState(77)
    L, F = 30, 10
    p = _prompt(rng, L)
    kw = dict(GREEDY, per_slot=True, repetition_penalty=1.0)
    empty = np.zeros((9, 0), np.uint32)
    ref, got = {}, {}
    with lm.session(**kw) as s:
        free0 = s.info()["free_pages"]
        _drain(s, {s.add(p, L + 3 * F - 2): "R"}, ref)
        t, Lt = s.add(p, L + F - 2), L
        for turn in range(3):
            while s.step(8):
                pass
            assert s.poll(t, codes=False) == (F, True)
            got[turn] = s.poll(t)[0]
            if turn == 2:
                break
            Lt = Lt + F  # history Lt + F - 1, and the last frame's column in front of the (empty) body
            nxt, pid = s.continue_from(t, empty, Lt + F - 2)
            assert nxt is not None and s.info()["live_prefixes"] == 0
            s.release(t)
            t = nxt
        s.release(t)
        assert np.array_equal(np.concatenate([got[0], got[1], got[2]], 1), ref["R"])
        assert _info(s)["free_pages"] == free0 and s.info()["shared_pages"] == 0
        # turns with bodies: 22-frame turns, 5-column bodies; turn k + 1 holds turn k's rows
        t, Lt, F2 = s.add(p, L + 22 - 2, seed=3), L, 22
        for turn in range(2):
            while s.step(8):
                pass
            T = Lt + F2 - 1
            rows = _rows(lm, t, T)
            Lt = T + 1 + 5
            nxt, _ = s.continue_from(t, _prompt(rng, 5), Lt + F2 - 2, seed=4 + turn)
            assert nxt is not None
            s.release(t)
            _live(s, nxt)
            assert _same_rows(_rows(lm, nxt, T), rows, T), turn
            t = nxt
        s.release(t)
        info = s.info()
        assert info["free_pages"] == free0 and info["shared_pages"] == 0 and info["live_prefixes"] == 0, info


# ---- 6. exact page accounting
def test_page_accounting_is_exact():
    lm = _handle("hd64")
    rng = np.random.RandomState(9)
    L = 30
    with lm.session(**GREEDY) as s:
        i0 = _info(s)
        free0 = i0["free_pages"]

        def moved(before, **delta):
            exp = dict(before)
            for k, v in delta.items():
                exp[k] += v
            now = _info(s)
            assert now == exp, (now, exp)
            return now

        src = s.add(_prompt(rng, L), L + 130)  # L + n_iter - 1 = 161 positions: 3 pages
        s.step(41)  # T = 70
        i1 = moved(i0, free_pages=-3, prefill_passes=1, tokens_prefilled=L - 1)
        # P % 64 != 0: page 0 shared, one page taken, one tail copy; no pass, no token
        pa, P = s.prefix_from_slot(src)
        assert P == 70
        i2 = moved(i1, free_pages=-1, shared_pages=1, live_prefixes=1, tail_pages_copied=1)
        # P % 64 == 0: no page taken (page 0 only gains a reference)
        pb, P = s.prefix_from_slot(src, 64)
        assert P == 64
        i3 = moved(i2, live_prefixes=1)
        s.step(58)  # T = 128
        pc, P = s.prefix_from_slot(src)
        assert P == 128
        i4 = moved(i3, shared_pages=1, live_prefixes=1)
        # a slot that sits on another prefix: its shared page simply gains a reference, its private page becomes shared at the second cut
        j = s.add(_prompt(rng, 5), 70 + 5 + 80, prefix=pa)  # 70 + 5 + 81 - 1 = 155 positions: page 0 shared, 2 private
        _live(s, j)
        s.step(30)  # T_j >= 74 + 30
        i5 = moved(i4, free_pages=-2, prefill_passes=1, tokens_prefilled=4, prefix_tokens_reused=70, tail_pages_copied=1)
        pd, P = s.prefix_from_slot(j, 100)
        assert P == 100
        i6 = moved(i5, free_pages=-1, live_prefixes=1, tail_pages_copied=1)
        s.step(30)  # T_j >= 134
        pe, P = s.prefix_from_slot(j, 128)
        i7 = moved(i6, shared_pages=1, live_prefixes=1)
        for pid in (pa, pb, pc, pd, pe):
            s.release_prefix(pid)
        s.release(src)
        s.release(j)
        i8 = _info(s)
        assert i8["free_pages"] == free0 and i8["shared_pages"] == 0 and i8["live_prefixes"] == 0, i8
        # source, joiner and prefix released in every order
        for P, order in itertools.product((100, 128), itertools.permutations(["source", "joiner", "prefix"])):
            src = s.add(_prompt(rng, L), L + 130)
            s.step(P - L + 1)
            pid, got_P = s.prefix_from_slot(src)
            assert got_P == P
            slots = {"source": src, "joiner": s.add(s.last_frame(src)[:, None], P + 1 + 30, prefix=pid)}
            _live(s, slots["joiner"])  # (its hold on the prefix's partly filled page ends with its activation)
            info = s.info()
            assert info["shared_pages"] == P // 64 and info["live_prefixes"] == 1
            for what in order:
                if what == "prefix":
                    s.release_prefix(pid)
                else:
                    s.release(slots[what])
            info = s.info()
            assert info["free_pages"] == free0 and info["shared_pages"] == 0 and info["live_prefixes"] == 0, (P, order, info)
        # the refused promotion: no free page and a cut inside a page -> (None, P), every counter unchanged; an aligned cut still goes through
        slots = [s.add(_prompt(rng, L), 10000) for _ in range(7)]  # clipped at max_seq_len: 4 pages each
        slots.append(s.add(_prompt(rng, L), L + 130))                # 3 pages
        assert None not in slots
        s.step(41)
        before = _info(s)
        assert before["free_pages"] == 0
        assert s.prefix_from_slot(slots[0]) == (None, 70) and s.prefix_from_slot(slots[7], 1) == (None, 1)
        assert _info(s) == before
        pid, P = s.prefix_from_slot(slots[0], 64)
        assert pid is not None and P == 64
        moved(before, shared_pages=1, live_prefixes=1)


# ---- 7. the error contract
def test_error_contract():
    lm = _handle("hd64")
    rng = np.random.RandomState(1)
    Lib = _ffi.lib()
    pid, P = C.c_int(-7), C.c_int(-7)
    col = np.zeros(9, np.uint32)

    def promote(slot, n):
        _ffi.check(Lib.fs_lm_session_prefix_from_slot(lm._h, slot, n, C.byref(pid), C.byref(P)))

    with pytest.raises(RuntimeError, match="no open session"):
        promote(0, -1)
    with pytest.raises(RuntimeError, match="no open session"):
        _ffi.check(Lib.fs_lm_session_last_frame(lm._h, 0, col.ctypes.data_as(C.POINTER(C.c_uint32))))
    with lm.session(**GREEDY) as s:
        free0 = _info(s)
        for bad in (-1, 3, 8, 100):
            with pytest.raises(RuntimeError, match="not a live session slot"):
                promote(bad, -1)
        with pytest.raises(RuntimeError, match="not a live session slot"):
            s.last_frame(3)
        # a one-column prompt before its first step: T = 0
        one = s.add(_prompt(rng, 1), 20)
        with pytest.raises(RuntimeError, match="T = 0"):
            s.prefix_from_slot(one)
        with pytest.raises(RuntimeError, match="not emitted a frame"):
            s.last_frame(one)
        s.release(one)
        # a slot still prefilling is waited for: its history is its prompt but the last column
        a = s.add(_prompt(rng, 30), 30 + 100)
        with pytest.raises(RuntimeError, match="not emitted a frame"):
            s.last_frame(a)
        got_pid, got_P = s.prefix_from_slot(a)
        assert got_pid is not None and got_P == 29
        s.release_prefix(got_pid)
        s.step(5)  # T = 34
        before = _info(s)
        for bad in (0, -2, 35, 1000):
            with pytest.raises(RuntimeError, match=r"n_positions = -?\d+ outside \[1, T = 34\]"):
                promote(a, bad)
        with pytest.raises(ValueError, match="n_positions"):
            s.prefix_from_slot(a, 0)
        assert _info(s) == before
        s.release(a)
        # P >= max_seq_len: a slot that ran into max_seq_len has T == max_seq_len
        b = s.add(_prompt(rng, 250), 10000)
        s.step(10)
        assert s.poll(b, codes=False) == (7, True)
        before = _info(s)
        with pytest.raises(RuntimeError, match="P = 256 >= max_seq_len"):
            s.prefix_from_slot(b)
        assert _info(s) == before
        got_pid, got_P = s.prefix_from_slot(b, 255)
        assert got_pid is not None and got_P == 255
        s.release_prefix(got_pid)
        s.release(b)
        assert _info(s)["free_pages"] == free0["free_pages"]


def test_a_rows_session_refuses():
    """the one full-size case (FS_SESSION_ROWS needs the Fish 1.5 shapes); nothing is generated"""
    lm = fishrt.DualARTransformer(fcfg.FISH_1_5, fcfg.FISH_1_5_TOKENS, 0, "bf16", max_batch=2).load_synthetic(SEED)
    try:
        p = np.zeros((9, 12), np.uint32)
        p[0] = np.random.RandomState(2).randint(0, 1000, 12)
        pid, P = C.c_int(-7), C.c_int(-7)
        with lm.session(temp=0.0, top_p=1.0, top_k=0, seed=1, ignore_eos=True, rows=True) as s:
            slot = s.add(p, 40)
            assert slot is not None
            with pytest.raises(ValueError, match="FS_SESSION_ROWS"):
                s.prefix_from_slot(slot)
            with pytest.raises(RuntimeError, match="FS_SESSION_ROWS sessions are not supported"):
                _ffi.check(_ffi.lib().fs_lm_session_prefix_from_slot(lm._h, slot, -1, C.byref(pid), C.byref(P)))
            assert s.info()["live_prefixes"] == 0
    finally:
        lm.close()


# ---- 8. untouched paths
def test_the_other_slots_of_a_session_with_a_promotion_are_untouched():
    lm = _handle("hd64")
    rng = np.random.RandomState(88)
    prompts = [_prompt(rng, L) for L in (30, 21, 17, 26)]
    frames = _frames(rng, 40)
    kw = dict(temp=0.7, top_p=0.8, top_k=50, seed=5, ignore_eos=True, per_slot=True, score=True, trace=True)

    def run(promote):
        out = {}
        with lm.session(**kw) as s:
            plain = s.add(prompts[0], 30 + 60, seed=11)
            hid = s.add(prompts[1], 21 + 50, seed=12, collect_hidden=True)
            sc = s.add_scored(prompts[2], frames)
            tr = s.add(prompts[3], 26 + 45, seed=13, trace=True)
            s.step(41)  # the plain slot has T = 70
            if promote:
                pid, P = s.prefix_from_slot(plain)  # a cut inside a page: the copy runs on the decode stream
                assert pid is not None and P == 70
            while s.step(8):
                pass
            for tag, slot in (("plain", plain), ("hid", hid), ("sc", sc), ("tr", tr)):
                out[tag] = s.poll(slot)[0]
            out["hidden"] = s.poll_hidden(hid)
            out.update({"sc." + k: v for k, v in s.poll_scores(sc).items()})
            out.update({"tr." + k: v for k, v in s.poll_trace(tr).items()})
        return out

    a, b = run(False), run(True)
    assert a.keys() == b.keys() and a["plain"].shape[1] == 62 and a["hidden"].shape[0] == 52
    for k in a:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


def test_generate_turns_keeps_the_budget_and_falls_back_when_the_history_no_longer_fits():
    """six turns of 30 frames behind a 40-column conditioning (per-slot greedy, penalty 1.0): every turn gets the frames it would have had
    on the conditioning alone; turn 0 IS the plain add, turn 1 is continue_from of it, and turn 5, whose history + body + budget would
    pass max_seq_len = 256, starts over on the conditioning alone"""
    lm = _handle("hd64")
    rng = np.random.RandomState(61)
    F = 30
    cond, bodies = _prompt(rng, 40), [_prompt(rng, 12) for _ in range(6)]
    between = np.zeros((9, 1), np.uint32)
    between[0, 0] = fcfg.TINY_TOKENS["im_end_id"]
    mnt = 40 + 12 + F - 2
    kw = dict(temp=0.0, top_p=1.0, top_k=0, repetition_penalty=1.0, seed=42, ignore_eos=True)
    turns = lm.generate_turns(cond, bodies, mnt, between=between, **kw)
    assert [t.shape for t in turns] == [(8, F)] * 6
    ref = {}
    with lm.session(per_slot=True, **kw) as s:
        a = s.add(np.concatenate([cond, bodies[0]], 1), mnt)
        _drain(s, {s.add(np.concatenate([cond, bodies[5]], 1), mnt): "alone"}, ref)
        assert s.poll(a, codes=False) == (F, True)
        ref["turn0"] = s.poll(a)[0]
        hist = 52 + F - 1
        b, _ = s.continue_from(a, np.concatenate([between, bodies[1]], 1), mnt + (hist + 1 + 13 - 52))
        s.release(a)
        _drain(s, {b: "turn1"}, ref)
        assert s.info()["live_prefixes"] == 0 and s.info()["shared_pages"] == 0
    assert np.array_equal(turns[0], ref["turn0"]) and np.array_equal(turns[1], ref["turn1"])
    assert np.array_equal(turns[5], ref["alone"])
