"""GPU: FS_SESSION_PER_SLOT -- a session slot on the static-batch step is its own generate_blocking call for every sampling decision
(include/fishrt.h): own settings, own StdRng stream, repetition penalty, batch-1 greedy / top-p / <|im_end|> rules, at max_batch values
and handle types outside FS_SESSION_ROWS.  Fish-1.5 shapes, synthetic weights."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import fishrt
from fishrt import config as fcfg, prompt as fprompt, server
from oracle import oracle as orc
from test_rows_gpu import EOS_BOOST, EOS_CFG, EOS_TOK, _eos_prompt, _referee

SEED = 0xF15E5EED
TOK = fcfg.FISH_1_5_TOKENS
IM_END = TOK["im_end_id"]
N_AUDIO = fcfg.FISH_1_5["vocab_size"] - IM_END

# the settings tests/test_persist_sampled_gpu.py uses: the server default, a narrower top-k, two peaked ones, one greedy
SETTINGS = [dict(temp=0.7, top_p=0.8, top_k=256), dict(temp=0.7, top_p=0.9, top_k=50), dict(temp=0.0875, top_p=0.8, top_k=256),
            dict(temp=0.02, top_p=0.8, top_k=256), dict(temp=0.0, top_p=1.0, top_k=0)]
PENALTIES = [1.0, 1.2, 1.4]


def _prompt(L, seed):
    p = np.zeros((9, L), np.uint32)
    p[0] = np.random.RandomState(seed).randint(0, IM_END, L)
    return p


@pytest.fixture(scope="module")
def lm16():
    lm = fishrt.DualARTransformer(fcfg.FISH_1_5, TOK, 0, "bf16", max_batch=16).load_synthetic(SEED)
    yield lm
    lm.close()


def _picks(cap):
    return np.concatenate([cap[:, :1, 2047], cap[:, 1:, 1024]], axis=1).astype(np.int64)  # [F][9]


def _replay(cap, seed, kw, amt):
    """the slot's RAW captured rows through the oracle: one RepPen(1024, 16, amt) per codebook from frame 1 on (last_token = that codebook's
    previous pick), then ONE LogitsProcessor stream in decision order -> (picks [F][9], a penalised entry really moved)"""
    L = orc.lib()
    L.orc_reppen_create.argtypes = [C.c_int, C.c_int, C.c_float]
    s = L.orc_sampler_create(C.c_uint64(seed), C.c_double(kw["temp"]), C.c_double(kw["top_p"]), C.c_uint64(kw["top_k"]))
    rps = [L.orc_reppen_create(1024, 16, C.c_float(amt)) for _ in range(8)]
    F = cap.shape[0]
    out = np.zeros((F, 9), np.int64)
    moved = False
    try:
        for f in range(F):
            row = np.ascontiguousarray(cap[f, 0, :N_AUDIO])
            out[f, 0] = L.orc_sampler_sample(C.c_void_p(s), row.ctypes.data_as(C.POINTER(C.c_float)), C.c_uint64(N_AUDIO))
            for c in range(8):
                raw = np.ascontiguousarray(cap[f, 1 + c, :1024])
                row = raw.copy()
                if f >= 1:
                    last = int(out[f - 1, 1 + c])
                    assert L.orc_reppen_apply(C.c_void_p(rps[c]), row.ctypes.data_as(C.POINTER(C.c_float)), 1024, last) == 0
                    if f == 1 and row[last] != raw[last]:
                        moved = True
                out[f, 1 + c] = L.orc_sampler_sample(C.c_void_p(s), row.ctypes.data_as(C.POINTER(C.c_float)), C.c_uint64(1024))
    finally:
        L.orc_sampler_destroy(C.c_void_p(s))
        for r in rps:
            L.orc_reppen_destroy(C.c_void_p(r))
    return out, moved


def _run_all(s, n_frames=8):
    while s.step(n_frames):
        pass


@pytest.mark.parametrize("dtype,max_batch", [("bf16", 16), ("fp8", 12)])
def test_every_decision_of_heterogeneous_slots_is_refereed_by_the_oracle(dtype, max_batch):
    """7 requests join one per round, each with its own settings, penalty and seed; for every slot the recorded picks are the returned
    codes, and replaying its raw captured rows through the oracle's repetition penalty and ONE sampler stream reproduces all F x 9 picks"""
    F, n = 20, 7
    lm = fishrt.DualARTransformer(fcfg.FISH_1_5, TOK, 0, dtype, max_batch=max_batch).load_synthetic(SEED)
    reqs = [dict(p=_prompt(14 + 9 * i, 1300 + i), kw=SETTINGS[i % len(SETTINGS)], amt=PENALTIES[i % 3], seed=9000 + 17 * i) for i in range(n)]
    lm.debug_capture(F)
    try:
        with lm.session(temp=0.7, top_p=0.8, top_k=256, seed=3, ignore_eos=True, per_slot=True, repetition_penalty=1.4) as s:
            slots = []
            for r in reqs:  # one join per round: each request meets the others mid-flight
                slots.append(s.add(r["p"], r["p"].shape[1] + F - 2, sampling=dict(r["kw"], repetition_penalty=r["amt"]), seed=r["seed"]))
                assert slots[-1] is not None
                s.step(2)
            _run_all(s)
            outs = [s.poll(sl)[0] for sl in slots]
        caps = [lm.debug_read_row(sl, F) for sl in slots]
    finally:
        lm.debug_capture(0)
        lm.close()
    assert len(set(slots)) == n
    penalty_mattered = False
    for r, sl, codes, cap in zip(reqs, slots, outs, caps):
        assert codes.shape == (8, F), (sl, codes.shape)
        got = _picks(cap)
        assert np.array_equal(got[:, 1:].T, codes.astype(np.int64)), f"slot {sl}: captured picks are not the returned codes"
        assert np.isneginf(cap[:, 0, 0]).all(), "ignore_eos must mask the <|im_end|> logit"
        exp, moved = _replay(cap, r["seed"], r["kw"], r["amt"])
        bad = np.argwhere(got != exp)
        print(f"{dtype} slot {sl} {r['kw']} penalty {r['amt']}: {F * 9 - len(bad)}/{F * 9} decisions identical to the oracle replay")
        assert bad.size == 0, f"slot {sl}: {len(bad)} of {F * 9} decisions differ from the oracle, first (frame, decision) {bad[0]}: gpu {got[tuple(bad[0])]} oracle {exp[tuple(bad[0])]}"
        if r["amt"] != 1.0:
            assert moved, "a penalised entry of frame 1 must differ from the raw logit"
            penalty_mattered |= not np.array_equal(_replay(cap, r["seed"], r["kw"], 1.0)[0], exp)
    assert penalty_mattered, "no slot's picks depend on its repetition penalty: the check above would not see a dropped penalty"


def test_a_request_does_not_depend_on_its_neighbours_or_its_slot(lm16):
    """One sampled request with an explicit seed, alone in the 16-slot session and admitted fifth among seven other requests with other
    settings that join and leave: identical codes.  (In a plain session the same request gets different codes in slot 0 and in slot 4:
    the lock-step sampler numbers its child streams by slot and max_batch.)"""
    F = 28
    p, kw, seed = _prompt(33, 77), dict(temp=0.7, top_p=0.8, top_k=256, repetition_penalty=1.4), 424242
    with lm16.session(seed=1, ignore_eos=True, per_slot=True) as s:
        sl = s.add(p, 33 + F - 2, sampling=kw, seed=seed)
        assert sl == 0
        _run_all(s)
        alone = s.poll(sl)[0]
    others = [dict(p=_prompt(10 + 7 * i, 500 + i), F=6 + 5 * i, kw=dict(SETTINGS[i % len(SETTINGS)], repetition_penalty=PENALTIES[i % 3])) for i in range(7)]
    with lm16.session(seed=99, ignore_eos=True, per_slot=True) as s:
        live = {}
        for o in others[:4]:
            live[s.add(o["p"], o["p"].shape[1] + o["F"] - 2, sampling=o["kw"], seed=o["F"])] = o
            s.step(1)
        sl = s.add(p, 33 + F - 2, sampling=kw, seed=seed)
        assert sl == 4
        left = 0
        for o in others[4:]:
            s.step(3)
            for k in list(live):  # the finished ones leave, the next one takes the freed slot
                if s.poll(k, codes=False)[1]:
                    s.release(k)
                    del live[k]
                    left += 1
            live[s.add(o["p"], o["p"].shape[1] + o["F"] - 2, sampling=o["kw"], seed=o["F"])] = o
        assert left >= 1
        _run_all(s, 5)
        among = s.poll(sl)[0]
    assert alone.shape == among.shape == (8, F)
    assert np.array_equal(alone, among), f"first differing frame {int(np.argmax((alone != among).any(0)))}"


def _through_session(lm, prompts, budgets, ignore_eos, rp):
    out = {}
    with lm.session(temp=0.0, top_p=1.0, top_k=0, seed=5, ignore_eos=ignore_eos, per_slot=True, repetition_penalty=rp) as s:
        slots = {}
        for i, (p, b) in enumerate(zip(prompts, budgets)):
            slots[s.add(p, b)] = i
            s.step(2)
        _run_all(s)
        for sl, i in slots.items():
            codes, done = s.poll(sl)
            assert done
            out[i] = codes
    return out


def test_greedy_slots_equal_their_own_generate_call(lm16):
    """greedy, penalty 1.2, ignore-eos: 9 requests through the per-slot session == generate_blocking of the same prompt, or parted at a
    refereed near-tie (at most 5 of 9, the share tests/test_rows_gpu.py grants its row-session twin)"""
    rp = 1.2
    rng = np.random.RandomState(11)
    lens = [int(v) for v in rng.randint(10, 90, 9)]
    frames = [int(v) for v in rng.randint(6, 40, 9)]
    prompts = [_prompt(L, 400 + i) for i, L in enumerate(lens)]
    budgets = [L + F - 2 for L, F in zip(lens, frames)]
    got = _through_session(lm16, prompts, budgets, True, rp)
    parted = 0
    for i in range(9):
        lm16.clear_slow_layer_caches()
        ref = lm16.generate_blocking(prompts[i], budgets[i], temp=0.0, top_p=1.0, top_k=0, repetition_penalty=rp, ignore_eos=True)
        assert got[i].shape == ref.shape == (8, frames[i]), (i, got[i].shape, ref.shape)
        if not np.array_equal(got[i], ref):
            parted += 1
            f, c, gap = _referee(lm16, prompts[i], budgets[i], got[i], ref, rp)
            print(f"request {i}: parts from its batch-1 call at frame {f} decision {c}: near-tie, gap {gap:.2e}")
    print(f"per-slot session: {9 - parted} of 9 requests identical to their own fs_lm_generate call")
    assert parted <= 5


def test_eos_ends_a_slot_like_its_own_generate_call(tmp_path):
    """without ignore-eos on the EOS-heavy checkpoint of tests/test_rows_gpu.py: a slot that samples <|im_end|> stops where its own
    generate_blocking call stops (zero frame 0 included), or parts from it at a refereed near-tie (at most 5 of 9)"""
    import test_safetensors_gpu as tsf
    rp, M = 1.2, 40
    t = tsf._lm_tensors(EOS_CFG, bf16=True)
    t["output.weight"][EOS_TOK["im_end_id"]] *= np.float32(EOS_BOOST)
    t["output.weight"] = (t["output.weight"].view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    path = str(tmp_path / "model.safetensors")
    tsf._save(t, path, True)
    lm = fishrt.DualARTransformer(EOS_CFG, EOS_TOK, 0, "bf16", max_batch=16).load_safetensors(path)
    os.remove(path)
    try:
        prompts = [_eos_prompt(12 + (s % 5), 4000 + s) for s in range(9)]
        budgets = [p.shape[1] + M for p in prompts]
        ref = []
        for p, b in zip(prompts, budgets):
            lm.clear_slow_layer_caches()
            ref.append(lm.generate_blocking(p, b, temp=0.0, top_p=1.0, top_k=0, repetition_penalty=rp))
        early = [i for i, r in enumerate(ref) if r.shape[1] < M + 2]
        assert early, "no fixture request reaches <|im_end|>: EOS path untested"
        got = _through_session(lm, prompts, budgets, False, rp)
        parted = 0
        for i in range(9):
            a, b = got[i], ref[i]
            if a.shape == b.shape and np.array_equal(a, b):
                continue
            parted += 1
            f, c, gap = _referee(lm, prompts[i], budgets[i], a, b, rp, ignore_eos=False)
            print(f"request {i}: parts from its batch-1 call at frame {f} decision {c}: near-tie, gap {gap:.2e}")
        print(f"per-slot session without ignore_eos: {9 - parted} of 9 identical; early stops on the batch-1 path: {[(i, ref[i].shape[1]) for i in early]}")
        assert parted <= 5
    finally:
        lm.close()


def test_lifecycle_reuse_prefix_errors_and_nothing_leaks(lm16):
    F = 12
    kw = dict(temp=0.7, top_p=0.8, top_k=256)
    p0, p1 = _prompt(20, 31), _prompt(27, 32)
    plain_kw = dict(temp=0.7, top_p=0.8, top_k=256, seed=8, ignore_eos=True)

    def plain_codes():
        with lm16.session(**plain_kw) as s:
            sl = s.add(p0, 20 + F - 2)
            _run_all(s)
            return s.poll(sl)[0]

    before = plain_codes()
    lm16.debug_capture(F)
    try:
        with lm16.session(seed=4, ignore_eos=True, per_slot=True, **kw) as s:
            # a slot released and re-admitted with another seed and penalty starts from word 0 and an empty window
            a = s.add(p0, 20 + F - 2, sampling=dict(kw, repetition_penalty=1.4), seed=111)
            _run_all(s)
            s.release(a)
            b = s.add(p1, 27 + F - 2, sampling=dict(kw, repetition_penalty=1.2), seed=222)
            assert b == a
            _run_all(s)
            codes_b = s.poll(b)[0]
            cap = lm16.debug_read_row(b, F)
            exp, _ = _replay(cap, 222, kw, 1.2)
            assert np.array_equal(_picks(cap), exp), "a re-admitted slot does not replay from a clean RNG / penalty state"
            assert np.array_equal(exp[:, 1:].T, codes_b.astype(np.int64))
            # prefixed admission == plain admission of the concatenated prompt (same settings, same seed)
            pid = s.add_prefix(p1[:, :19])
            c = s.add(p1[:, 19:], 27 + F - 2, prefix=pid, sampling=dict(kw, repetition_penalty=1.2), seed=222)
            _run_all(s)
            assert np.array_equal(s.poll(c)[0], codes_b)
            # add / add_prefixed without settings keep working: the session's settings, seed + admission number
            d = s.add(p0, 20 + F - 2)
            _run_all(s)
            assert s.poll(d)[0].shape == (8, F)
            # settings outside the per-slot samplers are refused, by name of the limit
            for bad in (dict(temp=0.7, top_p=0.8, top_k=0), dict(temp=0.7, top_p=0.8, top_k=257)):
                with pytest.raises(RuntimeError, match="top_k <= 256"):
                    s.add(p0, 20 + F - 2, sampling=bad)
    finally:
        lm16.debug_capture(0)
    L = fishrt.lib()
    samp = fishrt._ffi.Sampling(0.7, 0.8, 256, 1.4)
    assert L.fs_lm_session_begin(lm16._h, C.byref(samp), C.c_uint64(1), 16 | 8) != 0  # PER_SLOT | ROWS
    assert b"exclude" in L.fs_last_error()
    bad = fishrt._ffi.Sampling(0.7, 0.8, 0, 1.4)
    assert L.fs_lm_session_begin(lm16._h, C.byref(bad), C.c_uint64(1), 16) != 0
    assert b"top_k <= 256" in L.fs_last_error()
    with lm16.session(**plain_kw) as s:  # a plain session refuses per-slot settings and seeds (C ABI: the Python layer refuses earlier)
        slot, sd = C.c_int(-1), C.c_uint64(5)
        pp = np.ascontiguousarray(p0)
        args = (lm16._h, -1, pp.ctypes.data_as(C.POINTER(C.c_uint32)), 20, 20 + F - 2)
        assert L.fs_lm_session_add_ex(*args, C.byref(samp), None, C.byref(slot)) != 0 and b"FS_SESSION_PER_SLOT" in L.fs_last_error()
        assert L.fs_lm_session_add_ex(*args, None, C.byref(sd), C.byref(slot)) != 0
        assert L.fs_lm_session_add_ex(*args, None, None, C.byref(slot)) == 0 and slot.value == 0  # == fs_lm_session_add
    assert np.array_equal(plain_codes(), before), "a per-slot session leaked into the plain session that follows it"


def test_rows_session_takes_per_slot_settings_inside_its_instantiation():
    """FS_SESSION_ROWS + add_ex: own seed and settings per row, as long as all rows stay sampled (or all greedy)"""
    F, kw = 10, dict(temp=0.7, top_p=0.8, top_k=256)
    lm = fishrt.DualARTransformer(fcfg.FISH_1_5, TOK, 0, "bf16", max_batch=4).load_synthetic(SEED)
    p = _prompt(21, 5)
    lm.debug_capture(F)
    try:
        with lm.session(seed=1, ignore_eos=True, rows=True, repetition_penalty=1.2, **kw) as s:
            a = s.add(p, 21 + F - 2, sampling=dict(temp=0.7, top_p=0.9, top_k=50, repetition_penalty=1.4), seed=555)
            b = s.add(p, 21 + F - 2)
            with pytest.raises(RuntimeError, match="greedy or every slot sampled"):
                s.add(p, 21 + F - 2, sampling=dict(temp=0.0, top_p=1.0, top_k=0))
            _run_all(s)
            codes = s.poll(a)[0]
            assert s.poll(b)[0].shape == (8, F)
        cap = lm.debug_read_row(a, F)
    finally:
        lm.debug_capture(0)
        lm.close()
    # (the row kernels record the logits AFTER the penalty: the sampler stream alone replays them)
    from test_persist_sampled_gpu import _oracle_picks
    exp = _oracle_picks(cap, 555, 0.7, 0.9, 50)
    assert np.array_equal(_picks(cap), exp) and np.array_equal(exp[:, 1:].T, codes.astype(np.int64))


class Tok:  # ids = utf-8 bytes (all < im_end); <|semantic:0|> as in the Fish-1.5 token config
    def encode(self, text):
        return list(text.encode())

    def token_to_id(self, token):
        return {"<|semantic:0|>": TOK["semantic_start_id"]}.get(token)


class _FoldedCodec:
    """the synthetic LM draws codes over all 1024 codebook entries, the codec's FSQ has 1000 levels (a trained model never emits the rest):
    fold them, so that the WAV is a deterministic function of the generated codes instead of an out-of-range error"""

    def __init__(self, codec):
        self.codec = codec

    def decode(self, codes):
        return self.codec.decode(np.ascontiguousarray(codes % np.uint32(1000)))


def test_server_request_with_seed_sounds_the_same_alone_and_among_seven_others(lm16):
    from fastapi.testclient import TestClient
    codec = fishrt.FireflyCodec(0).load_synthetic(0xC0DEC)
    tok = Tok()
    enc = fprompt.PromptEncoder(tok, 8, fprompt.FISH_1_5)
    rng = np.random.RandomState(3)
    voices = {n: enc.encode_conditioning_prompt(f"reference text of {n}", rng.randint(0, 1000, (8, 40)).astype(np.uint32)) for n in ("default", "alice")}
    seeds = iter(range(1000, 100000))
    lock = threading.Lock()

    def seed_source():
        with lock:
            return next(seeds)

    # (prompts are 270-290 tokens: budgets of 20-40 frames, far below max_new_tokens frames, which the re-roll rule takes for a failed generation)
    ls = server.LMState(lm16, tok, voices, voices["default"], max_new_tokens=310, max_batch=16,
                        default_sampling_args=server.SamplingArgs(temp=0.7, top_p=0.8, top_k=256, repetition_penalty=1.4), seed_source=seed_source)
    st = server.AppState(ls, _FoldedCodec(codec), batch_window_s=0.05, per_slot_sampling=True)
    try:
        c = TestClient(server.make_app(st))
        req = dict(model="tts-1", voice="alice", input="The same words every time.", seed=31337, temperature=0.9)
        alone = c.post("/v1/audio/speech", json=req)
        assert alone.status_code == 200 or b"second time" in alone.content, alone.content[:200]
        res = [None] * 8

        def one(i):
            body = req if i == 3 else dict(model="tts-1", voice="default" if i % 2 else "alice", input=f"Other request number {i}, with other words.")
            res[i] = c.post("/v1/audio/speech", json=body)

        ths = [threading.Thread(target=one, args=(i,)) for i in range(8)]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        assert st.scheduler.stats["per_slot_sessions"] >= 1, st.scheduler.stats
        assert res[3].status_code == alone.status_code
        assert res[3].content == alone.content, "the seeded request's audio depends on the server's load"
        assert alone.status_code == 200, "the fixture must produce audio for the comparison to mean anything"
    finally:
        st.scheduler.close()
        codec.close()
