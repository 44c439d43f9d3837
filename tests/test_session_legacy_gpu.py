"""GPU: FS_SESSION_PER_SLOT sessions on Fish <= 1.4 handles (has_semantic_end == 0; include/fishrt.h).  Every slot is that request's own
fs_lm_generate call: the slow token is the legacy 2-way {pad, im_end} draw -- p_pad = softmax([pad, eos])[0] in f32, u = (word >> 8) * 2^-24
from the slot's own StdRng stream, ONE word per live frame at every temperature (greedy included) -- and the codebook decisions, penalty
windows, embedding, paging, prefixes, hidden states, server and streamer work as on Fish 1.5 handles.  Fish-1.4 shapes, synthetic weights."""
import ctypes as C
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import fishrt
from fishrt import config as fcfg, prompt as fprompt, server
from oracle import oracle as orc
from test_rows_gpu import NEAR_TIE
from test_session_per_slot_gpu import PENALTIES, SETTINGS

SEED = 0xF15E5EED
CFG, TOK = fcfg.FISH_1_4, fcfg.FISH_1_4_TOKENS
PAD, IM_END = TOK["pad_id"], TOK["im_end_id"]
F = 16  # iterations of a request that never samples <|im_end|>

# Sampler seeds and iteration budgets of the six refereed requests (the same for both handle dtypes).  The synthetic model's P(pad) is low
# on most prompts, so most seeds draw <|im_end|> within the first iterations; these were picked from a scan of candidate seeds on an
# MI355X (the end of a request is a function of its prompt, settings and seed alone: a seeded slot is prefilled in a pass of its own) so
# that both ways a slot can finish occur: requests 0, 1, 2, 4 draw <|im_end|> in iterations 0 - 2 of a 16-iteration budget, request 3
# runs out its 4 iterations and request 5 all 16 (its penalty windows fill up).  The test asserts both counts.
SEEDS = [9000, 9017, 9034, 14051, 10068, 14085]
BUDGETS = [16, 16, 16, 4, 16, 16]


def _prompt(L, seed):
    p = np.zeros((9, L), np.uint32)
    p[0] = np.random.RandomState(seed).randint(6, 400, L)
    p[0, 3:6] = PAD  # a VQ span: codebook embeddings are added under the <|semantic|> token only
    p[1:, 3:6] = np.random.RandomState(seed + 1).randint(1, 1024, (8, 3))
    return p


def _lm(dtype, max_batch=8):
    return fishrt.DualARTransformer(CFG, TOK, 0, dtype, max_batch=max_batch).load_synthetic(SEED)


@pytest.fixture(scope="module")
def lm14():
    lm = _lm("bf16")
    yield lm
    lm.close()


def _run_all(s, n_frames=8):
    while s.step(n_frames):
        pass


def _words(seed, n):
    out = (C.c_uint32 * n)()
    orc.lib().orc_rng_stream(C.c_uint64(seed), n, out, 0, None)
    return np.array(out, np.uint32)


def _u_of(word):
    return np.float32(int(word) >> 8) * np.float32(1.0 / 16777216.0)


def _p_pad(pad, eos):
    pad, eos = np.float32(pad), np.float32(eos)
    m = max(pad, eos)
    e_pad, e_eos = np.exp(np.float32(pad - m)), np.exp(np.float32(eos - m))
    return np.float32(e_pad / np.float32(e_pad + e_eos))


def _replay(cap, seed, kw, amt, n_iter, ignore_eos=False):
    """One legacy slot's capture record through the oracle: the slow decision recomputed from the two recorded logits and u (which must be
    the stream's word at the slot's position: one word per live frame for the slow draw, as the oracle's own legacy generate takes it
    from the request's stream, plus one per sampled codebook decision), the codebook decisions through RepPen(1024, 16, amt) from frame 1
    on and ONE sampler stream.  -> (picks [iterations run][9], iteration that drew <|im_end|> or None, penalised rows [f][c][1024])"""
    L = orc.lib()
    L.orc_reppen_create.argtypes = [C.c_int, C.c_int, C.c_float]
    sampled = kw["temp"] != 0.0
    s = L.orc_sampler_create(C.c_uint64(seed), C.c_double(kw["temp"]), C.c_double(kw["top_p"]), C.c_uint64(kw["top_k"]))
    rps = [L.orc_reppen_create(1024, 16, C.c_float(amt)) for _ in range(8)]
    words = _words(seed, 9 * n_iter + 9)
    two = np.zeros(2, np.float32)
    picks, rows, pos, ended = [], [], 0, None
    try:
        for f in range(n_iter):
            pad, eos, u = cap[f, 0, 0], cap[f, 0, 1], cap[f, 0, 2]
            assert np.isfinite(pad) and np.isfinite(eos), "the legacy record keeps both raw logits (ignore_eos masks nothing)"
            assert u == _u_of(words[pos]), f"frame {f}: recorded u {u!r} is not the stream's word {pos}"
            pos += 1
            if sampled:  # the oracle sampler's stream moves past the slow draw's word (a 2-candidate draw takes exactly one)
                L.orc_sampler_sample(C.c_void_p(s), two.ctypes.data_as(C.POINTER(C.c_float)), C.c_uint64(2))
            slow = 0 if (u < _p_pad(pad, eos) or ignore_eos) else 1
            frame = [slow]
            if slow == 1:
                ended = f
                picks.append(frame + [0] * 8)
                break
            prow = []
            for c in range(8):
                row = np.ascontiguousarray(cap[f, 1 + c, :1024]).copy()
                if f >= 1:
                    assert L.orc_reppen_apply(C.c_void_p(rps[c]), row.ctypes.data_as(C.POINTER(C.c_float)), 1024, int(picks[f - 1][1 + c])) == 0
                frame.append(int(L.orc_sampler_sample(C.c_void_p(s), row.ctypes.data_as(C.POINTER(C.c_float)), C.c_uint64(1024))))
                prow.append(row)
                pos += 1 if sampled else 0
            picks.append(frame)
            rows.append(prow)
    finally:
        L.orc_sampler_destroy(C.c_void_p(s))
        for r in rps:
            L.orc_reppen_destroy(C.c_void_p(r))
    return np.array(picks, np.int64), ended, rows


def _picks(cap, n):
    return np.concatenate([cap[:n, :1, 2047], cap[:n, 1:, 1024]], axis=1).astype(np.int64)


def _check_slot(cap, codes, seed, kw, amt, n_iter, ignore_eos=False):
    """captured picks == returned codes; every decision == the oracle replay -> iteration that drew <|im_end|> or None"""
    exp, ended, _ = _replay(cap, seed, kw, amt, n_iter, ignore_eos)
    n = exp.shape[0]
    got = _picks(cap, n)
    if ended is not None:  # the terminating iteration: no codebook decision was taken or recorded, and nothing beyond it
        assert not cap[ended, 1:].any(), "a slot that drew <|im_end|> still recorded codebook decisions in that iteration"
        assert not cap[ended + 1:].any(), "a finished slot went on recording"
        got[ended, 1:] = 0
    bad = np.argwhere(got != exp)
    assert bad.size == 0, f"{len(bad)} of {n * 9} decisions differ from the oracle, first (frame, decision) {bad[0]}: gpu {got[tuple(bad[0])]} oracle {exp[tuple(bad[0])]}"
    n_frames = n_iter if ended is None else max(ended, 1)  # frame 0 is emitted unconditionally, the terminating iteration's codes are not
    assert codes.shape == (8, n_frames), (codes.shape, n_frames, ended)
    assert np.array_equal(exp[:n_frames, 1:].T, codes.astype(np.int64)), "captured picks are not the returned codes"
    return ended


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_per_slot_session_opens_on_a_legacy_handle(dtype):
    lm = _lm(dtype)
    try:
        p = _prompt(12, 1)
        with lm.session(temp=0.7, top_p=0.8, top_k=256, seed=3, per_slot=True, ignore_eos=True) as s:
            sl = s.add(p, 12 + 4 - 2)
            assert sl == 0
            _run_all(s)
            codes, done = s.poll(sl)
        assert done and codes.shape == (8, 4) and codes.max() < 1024
    finally:
        lm.close()


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_every_decision_of_heterogeneous_legacy_slots_is_refereed(dtype):
    """six requests join one per round with their own settings, penalty and seed, ignore_eos off: the slow decision recomputed from the
    recorded logits and u, u checked against the stream word, all codebook decisions replayed; both endings occur"""
    n = 6
    lm = _lm(dtype)
    reqs = [dict(p=_prompt(14 + 9 * i, 1300 + i), kw=SETTINGS[i % len(SETTINGS)], amt=PENALTIES[i % 3], seed=SEEDS[i], F=BUDGETS[i]) for i in range(n)]
    lm.debug_capture(F)
    try:
        with lm.session(temp=0.7, top_p=0.8, top_k=256, seed=3, per_slot=True, repetition_penalty=1.4) as s:
            slots = []
            for r in reqs:
                slots.append(s.add(r["p"], r["p"].shape[1] + r["F"] - 2, sampling=dict(r["kw"], repetition_penalty=r["amt"]), seed=r["seed"]))
                assert slots[-1] is not None
                s.step(2)
            _run_all(s)
            outs = [s.poll(sl) for sl in slots]
        caps = [lm.debug_read_row(sl, F) for sl in slots]
    finally:
        lm.debug_capture(0)
        lm.close()
    assert len(set(slots)) == n
    ends = []
    for r, sl, (codes, done), cap in zip(reqs, slots, outs, caps):
        assert done
        ends.append(_check_slot(cap, codes, r["seed"], r["kw"], r["amt"], r["F"]))
        print(f"{dtype} slot {sl} {r['kw']} penalty {r['amt']} seed {r['seed']}: {codes.shape[1]} frames, <|im_end|> at iteration {ends[-1]}; every decision identical to the oracle replay")
    early = [e for e, r in zip(ends, reqs) if e is not None and e < r["F"] - 1]
    assert len(early) >= 2, f"fewer than two slots ended by <|im_end|> before their budget: {ends}"
    assert sum(e is None for e in ends) >= 2, f"fewer than two slots ran their budget out: {ends}"


def test_a_greedy_legacy_slot_takes_one_word_per_frame_and_a_readmission_starts_fresh(lm14):
    greedy, kw = dict(temp=0.0, top_p=1.0, top_k=0), dict(temp=0.7, top_p=0.8, top_k=256)
    p0, p1 = _prompt(20, 31), _prompt(27, 32)
    lm14.debug_capture(F)
    try:
        with lm14.session(seed=4, ignore_eos=True, per_slot=True, **kw) as s:
            a = s.add(p0, 20 + F - 2, sampling=dict(greedy, repetition_penalty=1.2), seed=111)
            _run_all(s)
            codes_a = s.poll(a)[0]
            cap = lm14.debug_read_row(a, F)
            # (the replay checks u of frame f against word f of the stream of seed 111: greedy codebook decisions draw nothing)
            assert _check_slot(cap, codes_a, 111, greedy, 1.2, F, ignore_eos=True) is None
            assert len(set(cap[:, 0, 2].tolist())) > F // 2, "the recorded draws do not move along the stream"
            s.release(a)
            b = s.add(p1, 27 + F - 2, sampling=dict(kw, repetition_penalty=1.4), seed=222)
            assert b == a
            _run_all(s)
            codes_b = s.poll(b)[0]
            cap = lm14.debug_read_row(b, F)
            assert _check_slot(cap, codes_b, 222, kw, 1.4, F, ignore_eos=True) is None  # replay from consumed = 0, empty windows
    finally:
        lm14.debug_capture(0)


@pytest.mark.parametrize("kw", [dict(temp=0.0, top_p=1.0, top_k=0, repetition_penalty=1.2), dict(temp=0.7, top_p=0.8, top_k=256, repetition_penalty=1.4)],
                         ids=["greedy", "sampled"])
def test_a_legacy_request_does_not_depend_on_its_neighbours_or_its_slot(lm14, kw):
    p, seed = _prompt(33, 77), 424242
    with lm14.session(seed=1, per_slot=True, ignore_eos=True) as s:
        sl = s.add(p, 33 + F - 2, sampling=kw, seed=seed)
        assert sl == 0
        _run_all(s)
        alone = s.poll(sl)[0]
    others = [dict(p=_prompt(10 + 7 * i, 500 + i), F=5 + 3 * i, kw=dict(SETTINGS[i % len(SETTINGS)], repetition_penalty=PENALTIES[i % 3])) for i in range(5)]
    with lm14.session(seed=99, per_slot=True, ignore_eos=True) as s:
        for o in others[:3]:
            assert s.add(o["p"], o["p"].shape[1] + o["F"] - 2, sampling=o["kw"], seed=o["F"]) is not None
            s.step(1)
        sl = s.add(p, 33 + F - 2, sampling=kw, seed=seed)
        assert sl == 3
        for o in others[3:]:
            s.step(2)
            assert s.add(o["p"], o["p"].shape[1] + o["F"] - 2, sampling=o["kw"], seed=o["F"]) is not None
        _run_all(s, 5)
        among = s.poll(sl)[0]
    assert alone.shape == among.shape == (8, F)
    assert np.array_equal(alone, among), f"first differing frame {int(np.argmax((alone != among).any(0)))}"


def test_greedy_legacy_slots_equal_their_own_generate_call(lm14):
    """greedy, penalty 1.2, ignore-eos: 8 requests through the per-slot session == fs_lm_generate(FS_GEN_NO_PERSIST) of the same prompt, or
    parted at a near-tie of the session's own penalised logits (at most 4 of 8: the 5-of-9 share of the Fish-1.5 twin)"""
    rp, n = 1.2, 8
    greedy = dict(temp=0.0, top_p=1.0, top_k=0)
    rng = np.random.RandomState(11)
    lens = [int(v) for v in rng.randint(10, 90, n)]
    frames = [int(v) for v in rng.randint(6, 20, n)]
    prompts = [_prompt(L, 400 + i) for i, L in enumerate(lens)]
    budgets = [L + Fi - 2 for L, Fi in zip(lens, frames)]
    lm14.debug_capture(20)
    try:
        with lm14.session(seed=5, ignore_eos=True, per_slot=True, repetition_penalty=rp, **greedy) as s:
            slots = []
            for p, b in zip(prompts, budgets):
                slots.append(s.add(p, b))
                s.step(2)
            _run_all(s)
            got = [s.poll(sl)[0] for sl in slots]
        caps = [lm14.debug_read_row(sl, 20) for sl in slots]
    finally:
        lm14.debug_capture(0)
    parted = 0
    for i in range(n):
        lm14.clear_slow_layer_caches()
        ref = lm14.generate_blocking(prompts[i], budgets[i], repetition_penalty=rp, ignore_eos=True, persistent=False, **greedy)
        assert got[i].shape == ref.shape == (8, frames[i]), (i, got[i].shape, ref.shape)
        if not np.array_equal(got[i], ref):
            parted += 1
            f = int(np.argmax((got[i] != ref).any(0)))
            c = int(np.argmax(got[i][:, f] != ref[:, f]))
            rows = _replay(caps[i], 5 + i, greedy, rp, frames[i], ignore_eos=True)[2]
            gap = float(abs(rows[f][c][got[i][c, f]] - rows[f][c][ref[c, f]]))
            print(f"request {i}: parts from its batch-1 call at frame {f} codebook {c}: near-tie, gap {gap:.2e}")
            assert gap < NEAR_TIE, (i, f, c, gap)
    print(f"legacy per-slot session: {n - parted} of {n} requests identical to their own fs_lm_generate call")
    assert parted <= 4


def test_legacy_surface_prefix_hidden_pages_and_errors(lm14):
    kw = dict(temp=0.7, top_p=0.8, top_k=256)
    p1 = _prompt(27, 32)
    with lm14.session(seed=4, ignore_eos=True, per_slot=True, **kw) as s:
        free0 = s.info()["free_pages"]
        a = s.add(p1, 27 + F - 2, sampling=dict(kw, repetition_penalty=1.2), seed=222)
        _run_all(s)
        full = s.poll(a)[0]
        pid = s.add_prefix(p1[:, :19])
        b = s.add(p1[:, 19:], 27 + F - 2, prefix=pid, sampling=dict(kw, repetition_penalty=1.2), seed=222)
        h = s.add(p1, 27 + F - 2, sampling=dict(kw, repetition_penalty=1.2), seed=222, collect_hidden=True)
        _run_all(s)
        assert np.array_equal(s.poll(b)[0], full), "a prefixed add differs from the full-prompt add"
        assert np.array_equal(s.poll(h)[0], full), "collecting hidden states changed a slot's codes"
        hid = s.poll_hidden(h)
        assert hid.shape[0] in (full.shape[1], full.shape[1] + 1) and hid.shape[1] == CFG["dim"] and np.isfinite(hid).all() and np.abs(hid).max() > 0
        for sl in (a, b, h):
            s.release(sl)
        s.release_prefix(pid)
        info = s.info()
        assert info["free_pages"] == free0 and info["shared_pages"] == 0 and info["live_prefixes"] == 0, info
    # without ignore_eos a collecting slot that draws <|im_end|> has one row more than frames (unless it ended in iteration 0)
    with lm14.session(seed=4, per_slot=True, **kw) as s:
        h = s.add(p1, 27 + F - 2, seed=SEEDS[1], collect_hidden=True)
        _run_all(s)
        n = s.poll(h)[0].shape[1]
        assert s.poll_hidden(h).shape[0] in (n, n + 1)
    for bad in (dict(), dict(rows=True)):
        with pytest.raises(RuntimeError, match="FS_SESSION_PER_SLOT"):
            lm14.session(seed=1, **kw, **bad)
    with lm14.session(seed=1, per_slot=True, **kw) as s:  # the handle is fine after the refusals
        assert s.add(p1, 27 + 2) == 0


class Tok:  # ids = utf-8 bytes + 6 (clear of the control ids); <|semantic|> as in the Fish-1.4 token config
    def encode(self, text):
        return [6 + b for b in text.encode()]

    def token_to_id(self, token):
        return {"<|semantic|>": PAD}.get(token)


class _SpyLM:
    """the handle, with every finished slot's polled codes recorded (and those of a job that ran alone on the batch-1 path)"""

    def __init__(self, lm):
        self._lm, self.polled = lm, []

    def __getattr__(self, k):
        return getattr(self._lm, k)

    def generate_blocking(self, *a, **kw):
        codes = self._lm.generate_blocking(*a, **kw)
        self.polled.append(codes.copy())
        return codes

    def session(self, **kw):
        s, spy = self._lm.session(**kw), self
        poll = s.poll

        def spy_poll(slot, codes=True):
            r = poll(slot, codes)
            if codes and r[1]:
                spy.polled.append(r[0].copy())
            return r

        s.poll = spy_poll
        return s


class _RecCodec:
    def __init__(self, codec):
        self.codec, self.seen, self.lock = codec, [], threading.Lock()

    def decode(self, codes):
        with self.lock:
            self.seen.append(np.array(codes[0], np.uint32))
        return self.codec.decode(np.ascontiguousarray(codes % np.uint32(1000)))


def test_server_legacy_jobs_join_a_per_slot_session(lm14):
    codec = fishrt.FireflyCodec(0).load_synthetic(0xC0DEC)
    tok, spy = Tok(), _SpyLM(lm14)
    enc = fprompt.PromptEncoder(tok, 8, fprompt.FISH_1_4)
    rng = np.random.RandomState(3)
    voices = {n: enc.encode_conditioning_prompt(f"reference text of {n}", rng.randint(0, 1000, (8, 20)).astype(np.uint32)) for n in ("default", "alice")}
    seeds = iter(range(1000, 100000))
    lock = threading.Lock()

    def seed_source():
        with lock:
            return next(seeds)

    texts = ["The same words every time."] + [f"Other request number {i}, with other words." for i in range(3)]
    longest = max(enc.encode_sequence([t], None, v)[1][0].shape[1] for t in texts for v in voices.values())
    # (budgets of about 20 frames, far below max_new_tokens frames, which the re-roll rule takes for a failed generation)
    ls = server.LMState(spy, tok, voices, voices["default"], model_type=fprompt.FISH_1_4, max_new_tokens=longest + 20, max_batch=8,
                        default_sampling_args=server.SamplingArgs(temp=0.7, top_p=0.8, top_k=256, repetition_penalty=1.2), seed_source=seed_source)
    rec = _RecCodec(codec)
    st = server.AppState(ls, rec, batch_window_s=0.05, per_slot_sampling=True)
    try:
        # fixture: a seed whose generation yields audio (the synthetic model can draw <|im_end|> in iteration 0 or a code 0, which the
        # Fish <= 1.4 shift refuses by design)
        req = alone = None
        for seed in range(31337, 31337 + 12):
            req = dict(model="tts-1", voice="alice", input="The same words every time.", seed=seed, temperature=0.9)
            alone = server.generate_speech(st, req)
            if alone[0] == 200:
                break
            assert b"code 0" in (alone[2] if isinstance(alone[2], bytes) else str(alone[2]).encode()), alone
        assert alone[0] == 200, "no candidate seed produces audio"
        res = [None] * 4

        def one(i):
            body = req if i == 3 else dict(model="tts-1", voice="default" if i % 2 else "alice", input=texts[1 + i])
            res[i] = server.generate_speech(st, body)

        ths = [threading.Thread(target=one, args=(i,)) for i in range(4)]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        assert st.scheduler.stats["per_slot_sessions"] >= 1, st.scheduler.stats
        assert st.scheduler.stats.get("row_sessions", 0) == 0, st.scheduler.stats
        assert res[3][0] == 200 and res[3][2] == alone[2], "the seeded request's audio depends on the server's load"
        for r in res:
            assert r[0] == 200 or "code 0" in str(r[2]), r
        # every code array the vocoder was given is a finished slot's codes minus one
        assert rec.seen and len(rec.seen) <= len(spy.polled)
        for got in rec.seen:
            assert any(p.shape == got.shape and p.min() >= 1 and np.array_equal(p - np.uint32(1), got) for p in spy.polled)
    finally:
        st.scheduler.close()
        codec.close()


class _Shifted:
    """a legacy session's codes as the vocoder takes them: minus one (Fish <= 1.4), folded into the synthetic codec's 1000 FSQ levels"""

    def __init__(self, s):
        self.s = s

    def add(self, p, n):
        return self.s.add(p, n)

    def step(self, k):
        return self.s.step(k)

    def release(self, slot):
        return self.s.release(slot)

    def poll(self, slot, codes=True):
        r = self.s.poll(slot, codes)
        return ((r[0] + np.uint32(999)) % np.uint32(1000), r[1]) if codes else r


def test_ragged_session_streamer_over_legacy_slots():
    lm = _lm("bf16", max_batch=4)
    codec = fishrt.FireflyCodec(0).load_synthetic(0xC0DEC)
    lens, frames, joins = (12, 7, 20, 9), (20, 13, 17, 3), (0, 0, 1, 2)
    prompts = [_prompt(L, 60 + i) for i, L in enumerate(lens)]
    out, pcm, finals = {}, {i: [] for i in range(4)}, []
    try:
        with lm.session(temp=0.7, top_p=0.8, top_k=256, seed=42, ignore_eos=True, per_slot=True) as raw:
            ss = fishrt.SessionStreamer(_Shifted(raw), codec, chunk=8, first_chunk=4, ragged=True,
                                        on_audio=lambda tag, p, final: (pcm[tag].append(p.copy()), final and finals.append(tag)))
            live, step = {}, 0
            while len(out) < 4:
                for i in range(4):
                    if joins[i] <= step and i not in out and i not in live.values():
                        slot = ss.add(prompts[i], lens[i] + frames[i] - 2, tag=i)
                        assert slot is not None
                        live[slot] = i
                ss.step(4)
                for slot, i in list(live.items()):
                    if i in ss.results:
                        out[i] = ss.results[i]
                        del live[slot]
                step += 1
                assert step < 100
        assert sorted(finals) == [0, 1, 2, 3]
        for i in range(4):
            assert out[i].shape == (8, frames[i])
            ref = codec.decode(np.ascontiguousarray(out[i][None]))[0, 0]
            streamed = np.concatenate(pcm[i])
            assert streamed.shape == ref.shape and np.array_equal(streamed, ref), (i, float(np.abs(streamed - ref).max()))
    finally:
        codec.close()
        lm.close()
