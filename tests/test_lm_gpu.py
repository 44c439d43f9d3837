"""GPU parity tests of the dual-AR LM hot path: HIP (through the C ABI) vs the CPU oracle and the committed goldens.

Tolerances.  f32 mode (f32 weights + f32 KV): only summation order differs from the oracle -> logits within 2e-4 rel /
5e-5 abs, greedy tokens bit-identical.  bf16 mode (bf16 weights + bf16 KV, f32 activations) is compared with the oracle
run on the SAME bf16-rounded weights with its KV rounded to bf16: logits within 2e-3 abs, greedy tokens identical
wherever the oracle's top-2 margin exceeds that tolerance (SURVEY.md §7 "hard parts")."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import fishrt
from fishrt import config as fcfg
from oracle import oracle as orc

G = os.path.join(os.path.dirname(__file__), "golden")
LMG = np.load(os.path.join(G, "lm_tiny.npz"))
SEED = int(LMG["seed"])
TOL32 = dict(rtol=2e-4, atol=5e-5)
TOLBF = dict(rtol=2e-3, atol=2e-3)
NEAR_TIE = 5e-3  # bf16 handles: logits within TOLBF of the oracle's, so a greedy decision can flip only where the oracle's top-2 margin is ~2 x that


def _rows_leave_oracle_only_at_near_ties(got, exp, o, what=""):
    """Greedy static batch vs the oracle's generate_static_batch restatement: row b may leave the oracle's token stream only at a frame
    whose smallest top-2 logit margin over the row's 9 decisions (oracle.last_batch_margins[frame, row]) is below NEAR_TIE -- a kernel
    bug (wrong row / position / panel mapping) diverges on ordinary margins.  Returns the number of rows that flipped."""
    flips = 0
    m = o.last_batch_margins
    for b, (g, e) in enumerate(zip(got, exp)):
        assert g.shape == e.shape, (what, b, g.shape, e.shape)
        if np.array_equal(g, e):
            continue
        f = int(np.argmax((g != e).any(0)))
        # the slow token is not part of the output: a flipped slow token of iteration f - 1 first shows in frame f (through the next input)
        mf = float(min(m[f, b], m[f - 1, b])) if f > 0 else float(m[f, b])
        assert mf < NEAR_TIE, f"{what} row {b} left the oracle's stream at frame {f} on a margin of {mf:.2e}"
        flips += 1
    return flips


def _tiny(dtype, max_batch=1):
    return fishrt.DualARTransformer(fcfg.TINY, fcfg.TINY_TOKENS, 0, dtype, max_batch).load_synthetic(SEED)


@pytest.fixture(scope="module")
def tiny32():
    return _tiny("f32", 2)


@pytest.fixture(scope="module")
def tinybf():
    return _tiny("bf16", 2)


def test_synthetic_weights_match_oracle_spec(tiny32, tinybf):
    ids = np.array([0, 11, 50, 63], np.uint32)
    for lm, bf in ((tiny32, False), (tinybf, True)):
        exp = orc.synth("fast_embeddings.weight", 64 * 128, SEED, 0.0, 0.02, bf).reshape(64, 128)[ids]
        assert np.array_equal(lm.fast_embeddings(ids), exp)


def test_tiny_f32_teacher_forced_vs_golden(tiny32):
    lm = tiny32
    lm.clear_slow_layer_caches()
    logits, hidden = lm.forward_generate(LMG["prompt"], 0)
    np.testing.assert_allclose(logits, LMG["f32w_prefill_logits"], **TOL32)
    np.testing.assert_allclose(hidden, LMG["f32w_prefill_hidden"], **TOL32)
    assert lm.curr_kv_size() == LMG["prompt"].shape[1]
    l2, h2 = lm.forward_generate(LMG["decode_step_tokens"], lm.curr_kv_size())
    np.testing.assert_allclose(l2, LMG["f32w_decode_logits"], **TOL32)
    np.testing.assert_allclose(h2, LMG["f32w_decode_hidden"], **TOL32)
    lm.clear_fast_layer_caches()
    fe = lm.fast_embeddings([11, 50])
    f0 = lm.forward_generate_fast(h2, 0)
    f1 = lm.forward_generate_fast(fe[0], 1)
    f2 = lm.forward_generate_fast(fe[1], 2)
    np.testing.assert_allclose(np.concatenate([f0, f1, f2]), LMG["f32w_fast_logits"], **TOL32)


def test_tiny_chunked_prefill_and_truncate(tiny32):
    lm = tiny32
    p = LMG["prompt"]
    lm.clear_slow_layer_caches()
    lm.forward_generate(p[:, :5], 0)
    l3, _ = lm.forward_generate(p[:, 5:], 5)
    np.testing.assert_allclose(l3, LMG["f32w_chunked_logits"], **TOL32)
    lm.clear_slow_caches_until(5)  # NOT inclusive (dual_ar.rs:391-404)
    assert lm.curr_kv_size() == 5
    l4, _ = lm.forward_generate(p[:, 5:], 5)
    np.testing.assert_array_equal(l3, l4)
    lm.clear_slow_caches_until(1000)
    assert lm.curr_kv_size() == p.shape[1]


def test_tiny_batched_prefill_pad_mask_ignored(tiny32):
    lm = tiny32
    lm.clear_slow_layer_caches()
    lb, hb = lm.forward_generate(LMG["batch2_prompt"], 0)
    np.testing.assert_allclose(lb, LMG["f32w_batch2_logits"], **TOL32)
    np.testing.assert_allclose(hb, LMG["f32w_batch2_hidden"], **TOL32)


@pytest.mark.parametrize("rp", [1.0, 1.2])
def test_tiny_f32_greedy_rollout_bit_identical(tiny32, rp):
    lm = tiny32
    lm.clear_slow_layer_caches()
    p = LMG["prompt"]
    out = lm.generate_blocking(p, 24 + p.shape[1] - 2, temp=0.0, top_p=1.0, top_k=0, repetition_penalty=rp, ignore_eos=True)
    assert out.shape == (8, 24)
    assert np.array_equal(out, LMG[f"f32w_rollout_rp{int(rp * 10)}"])
    assert lm.curr_kv_size() == p.shape[1] + 23
    # run-to-run determinism and oracle agreement on a second prompt with a cached prefix (speech.rs:40 pattern)
    o = orc.OracleLM(orc.TINY).load_synthetic(SEED)
    o.forward_generate(p[:, :6], 0)
    exp = o.generate(p[:, 6:], 20, temp=0.0, repetition_penalty=rp, ignore_eos=True)
    lm.clear_slow_caches_until(6)
    got = lm.generate_blocking(p[:, 6:], 20, temp=0.0, top_p=1.0, top_k=0, repetition_penalty=rp, ignore_eos=True)
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("rp", [1.0, 1.2])
def test_tiny_bf16_vs_oracle_same_rounding(tinybf, rp):
    lm = tinybf
    p = LMG["prompt"]
    o = orc.OracleLM(orc.TINY).load_synthetic(SEED, bf16=True)
    o.set_kv_round_bf16(True)
    lm.clear_slow_layer_caches()
    lg, hg = lm.forward_generate(p, 0)
    lo, ho = o.forward_generate(p, 0)
    np.testing.assert_allclose(lg, lo, **TOLBF)
    np.testing.assert_allclose(hg, ho, **TOLBF)
    lm.clear_slow_layer_caches()
    o.clear_slow()
    M = 24 + p.shape[1] - 2
    got = lm.generate_blocking(p, M, temp=0.0, top_p=1.0, top_k=0, repetition_penalty=rp, ignore_eos=True)
    exp = o.generate(p, M, temp=0.0, repetition_penalty=rp, ignore_eos=True)
    assert got.shape == exp.shape == (8, 24)
    assert np.array_equal(got, exp)


def test_eos_semantics_and_budget(tiny32):
    """single_batch.rs:61,77,153-156,199-204,250,264-266: budget counts prompt tokens; an <|im_end|> frame is dropped
    unless it is the first; the oracle is the judge for where EOS falls."""
    lm = tiny32
    o = orc.OracleLM(orc.TINY).load_synthetic(SEED)
    rng = np.random.RandomState(5)
    hit_eos = 0
    for trial in range(6):
        L = int(rng.randint(1, 9))
        p = np.zeros((9, L), np.uint32)
        p[0] = rng.randint(0, 400, L)
        lm.clear_slow_layer_caches(); o.clear_slow()
        M = 120
        got = lm.generate_blocking(p, M, temp=0.0, top_p=1.0, top_k=0, repetition_penalty=1.1)
        exp = o.generate(p, M, temp=0.0, repetition_penalty=1.1)
        assert np.array_equal(got, exp)
        assert lm.curr_kv_size() == o.kv_len()
        hit_eos += exp.shape[1] < M - L + 2
    # error behaviour: prompt row count / out-of-range ids
    with pytest.raises(ValueError):
        lm.generate_blocking(np.zeros((8, 4), np.uint32), 10)
    with pytest.raises(RuntimeError):
        lm.forward_generate(np.full((9, 2), 600, np.uint32), lm.curr_kv_size())


def test_generate_blocking_with_hidden_vs_oracle(tiny32):
    """single_batch.rs:217-306: codes + the slow transformer's hidden state of every generator iteration (the terminating <|im_end|>
    iteration included, :264-266); collect_hidden_states = false returns None; Fish-1.5 shapes in bf16 below."""
    lm = tiny32
    o = orc.OracleLM(orc.TINY).load_synthetic(SEED)
    rng = np.random.RandomState(5)
    n_plus_one = 0
    for trial in range(6):
        L = int(rng.randint(1, 9))
        p = np.zeros((9, L), np.uint32)
        p[0] = rng.randint(0, 400, L)
        lm.clear_slow_layer_caches(); o.clear_slow()
        codes, hid = lm.generate_blocking_with_hidden(p, 120, True, temp=0.0, top_p=1.0, top_k=0, repetition_penalty=1.1)
        ec, eh = o.generate(p, 120, temp=0.0, repetition_penalty=1.1, collect_hidden=True)
        assert np.array_equal(codes, ec)
        assert hid.shape == (eh.shape[0], 1, eh.shape[1]) and hid.shape[0] in (codes.shape[1], codes.shape[1] + 1)
        np.testing.assert_allclose(hid[:, 0], eh, rtol=2e-4, atol=2e-5)
        n_plus_one += hid.shape[0] == codes.shape[1] + 1
        # the rows are what forward_generate returns as `hidden` for the same position
        lm.clear_slow_layer_caches()
        _, h0 = lm.forward_generate(p, 0)
        np.testing.assert_allclose(hid[0, 0], h0.reshape(-1), rtol=1e-5, atol=1e-6)
    assert n_plus_one >= 1, "no run ended on <|im_end|>: the extra hidden row of the terminating iteration went untested"
    lm.clear_slow_layer_caches()
    codes2, none = lm.generate_blocking_with_hidden(p, 120, False, temp=0.0, top_p=1.0, top_k=0, repetition_penalty=1.1)
    assert none is None and np.array_equal(codes2, codes)


def test_generate_blocking_with_hidden_fish15_bf16():
    lm = fishrt.DualARTransformer(fcfg.FISH_1_5, fcfg.FISH_1_5_TOKENS, 0, "bf16").load_synthetic(SEED)
    rng = np.random.RandomState(8)
    p = np.zeros((9, 20), np.uint32)
    p[0] = rng.randint(0, 100000, 20)
    for persistent in (True, False):
        lm.clear_slow_layer_caches()
        codes, hid = lm.generate_blocking_with_hidden(p, 20 + 10, True, temp=0.0, top_p=1.0, top_k=0, repetition_penalty=1.2, ignore_eos=True,
                                                      persistent=persistent)
        assert codes.shape == (8, 12) and hid.shape == (12, 1, 1024) and np.isfinite(hid).all()
        lm.clear_slow_layer_caches()
        _, h0 = lm.forward_generate(p, 0)
        # (generate runs the last prompt token through the GEMV decode kernels, forward_generate runs all of them as one MFMA pass)
        np.testing.assert_allclose(hid[0, 0], h0.reshape(-1), rtol=2e-3, atol=1e-3)
        assert np.abs(hid[1, 0] - hid[0, 0]).max() > 1e-2
    lm.close()


def test_streaming_callback_matches_blocking(tiny32):
    lm = tiny32
    p = LMG["prompt"]
    lm.clear_slow_layer_caches()
    frames = []
    out = lm.generate_blocking(p, 40, temp=0.0, top_p=1.0, top_k=0, repetition_penalty=1.2, ignore_eos=True,
                               on_frame=lambda i, c: frames.append((i, list(c))) and False)
    assert [f[0] for f in frames] == list(range(out.shape[1]))
    assert np.array_equal(np.array([f[1] for f in frames], np.uint32).T, out)


def test_static_batch_greedy_rows_match_padded_single(tiny32):
    """static_batch.rs:68-111: left padding with <|im_end|>/0 is NOT masked -> row i == single generation of the padded prompt."""
    lm = tiny32
    rng = np.random.RandomState(9)
    prompts = []
    for L in (5, 9, 7):
        p = np.zeros((9, L), np.uint32)
        p[0] = rng.randint(0, 400, L)
        prompts.append(p)
    outs = lm.generate_static_batch(prompts, 30, temp=0.0, top_p=1.0, top_k=0, repetition_penalty=1.3, ignore_eos=True)
    o = orc.OracleLM(orc.TINY).load_synthetic(SEED)
    for p, got in zip(prompts, outs):
        pad = 9 - p.shape[1]
        pp = np.concatenate([np.zeros((9, pad), np.uint32), p], 1)
        pp[0, :pad] = 400
        o.clear_slow()
        exp = o.generate(pp, 30, temp=0.0, repetition_penalty=1.0, ignore_eos=True)  # batch rep-pen is a no-op (static_batch.rs:204-206)
        assert np.array_equal(got, exp)


@pytest.mark.parametrize("kw", [dict(temp=0.7, top_p=0.8, top_k=32), dict(temp=1.0, top_p=0.95, top_k=16), dict(temp=1e-8, top_p=1.0, top_k=16)])
def test_static_batch_on_f32_handle_follows_the_batch_sampler(tiny32, kw):
    """f32 handles generate a static batch row by row on the single-sequence kernels (no MFMA row path), but with
    BatchedLogitsProcessor semantics (sampling/mod.rs:77-109): temp <= 1e-7 -> FIRST-max argmax, else row b draws call c of its request
    from the child StdRng seeded with the master's u64 number c * B + b -- so the rows equal the oracle's lock-step generate_static_batch
    token for token (f32 logits; ADVICE r1: the fallback used the single-sequence tie rule and an ad-hoc per-row seed)."""
    lm = tiny32
    o = orc.OracleLM(orc.TINY).load_synthetic(SEED)
    rng = np.random.RandomState(19)
    prompts = []
    for L in (5, 9, 7, 3):
        p = np.zeros((9, L), np.uint32)
        p[0] = rng.randint(0, 400, L)
        prompts.append(p)
    outs = lm.generate_static_batch(prompts, 30, seed=42, ignore_eos=True, **kw)
    exps = o.generate_batch(prompts, 30, seed=42, ignore_eos=True, **kw)
    for b, (g, e) in enumerate(zip(outs, exps)):
        assert g.shape == e.shape and np.array_equal(g, e), (b, int(np.argmax((g != e).any(0))) if g.shape == e.shape else (g.shape, e.shape))


@pytest.mark.parametrize("temp,top_p,top_k", [(0.7, 0.8, 0), (0.7, 0.8, 16), (1.0, 1.0, 0), (0.5, 0.9, 50)])
def test_sampled_decode_matches_oracle_stream(tiny32, temp, top_p, top_k):
    """temp > 0: softmax(logits/temp) -> top-k -> top-p -> WeightedIndex draw from the StdRng (ChaCha12) stream seeded by
    `seed` (sampling/mod.rs:51-132; candle LogitsProcessor::TopKThenTopP).  Device sampler and oracle share the RNG stream
    and the decision procedure, so the sampled tokens are expected to be identical (expf differs by <= 1 ulp between the
    two, which can move a cumulative-probability boundary across the uniform draw only with probability ~1e-6/sample)."""
    lm = tiny32
    o = orc.OracleLM(orc.TINY).load_synthetic(SEED)
    p = LMG["prompt"]
    agree, total = 0, 0
    for seed in (1, 42, 12345):
        lm.clear_slow_layer_caches(); o.clear_slow()
        M = 30 + p.shape[1] - 2
        got = lm.generate_blocking(p, M, temp=temp, top_p=top_p, top_k=top_k, repetition_penalty=1.2, seed=seed, ignore_eos=True)
        exp = o.generate(p, M, temp=temp, top_p=top_p, top_k=top_k, repetition_penalty=1.2, seed=seed, ignore_eos=True)
        assert got.shape == exp.shape == (8, 30)
        same = (got == exp).all(0)
        first_bad = int(np.argmin(same)) if not same.all() else 30
        agree += first_bad; total += 30
        assert first_bad >= 10, (seed, first_bad, got[:, :first_bad + 1], exp[:, :first_bad + 1])
    print(f"sampled (temp={temp}, top_p={top_p}, top_k={top_k}): identical prefix {agree}/{total} frames")
    # different seeds give different streams; same seed is reproducible
    lm.clear_slow_layer_caches()
    a = lm.generate_blocking(p, 30, temp=temp, top_p=top_p, top_k=top_k, seed=7, ignore_eos=True)
    lm.clear_slow_layer_caches()
    b = lm.generate_blocking(p, 30, temp=temp, top_p=top_p, top_k=top_k, seed=7, ignore_eos=True)
    lm.clear_slow_layer_caches()
    c = lm.generate_blocking(p, 30, temp=temp, top_p=top_p, top_k=top_k, seed=8, ignore_eos=True)
    assert np.array_equal(a, b) and not np.array_equal(a, c)


def _batch_prompts(seed, lens):
    rng = np.random.RandomState(seed)
    out = []
    for L in lens:
        p = np.zeros((9, L), np.uint32)
        p[0] = rng.randint(0, 400, L)
        if L >= 6:  # a VQ span so that codebook embeddings are exercised
            codes = rng.randint(0, 64, (8, 3))
            p[0, 2:5] = 401 + codes[0]
            p[1:, 2:5] = codes
        out.append(p)
    return out


@pytest.mark.parametrize("sampling", [dict(temp=0.0, top_p=1.0, top_k=0), dict(temp=0.7, top_p=0.8, top_k=32)])
def test_static_batch_mfma_rows_vs_oracle(sampling):
    """generate_static_batch on the MFMA row path (bf16 handle; rows = sequences, weights streamed once per step) vs the
    oracle's restatement of static_batch.rs on the same bf16-rounded weights with bf16-rounded K/V: ragged prompts,
    left padding, per-row EOS, child-RNG sampling (seed 42 like static_batch.rs:63)."""
    lm = _tiny("bf16", 8)
    o = orc.OracleLM(orc.TINY).load_synthetic(SEED, bf16=True)
    o.set_kv_round_bf16(True)
    prompts = _batch_prompts(5, (5, 11, 8, 3, 7))
    M = 40
    lm.debug_capture(M - 11 + 2)
    got = lm.generate_static_batch(prompts, M, seed=42, repetition_penalty=1.3, ignore_eos=True, **sampling)
    # every decision of every row == the oracle batch sampler on the logits the decision saw (fs_lm_debug_capture on the row path): no
    # near-tie / CDF-boundary excuse -- the comparison is on the GPU's own logits
    from test_batch_capture_gpu import replay_batch_decisions
    replay_batch_decisions(lm, 5, M - 11 + 2, sampling, 42, got, n_audio=fcfg.TINY["vocab_size"] - fcfg.TINY_TOKENS["im_end_id"], cb_size=fcfg.TINY["codebook_size"])
    lm.debug_capture(0)
    exp = o.generate_batch(prompts, M, seed=42, ignore_eos=True, **sampling)
    assert [g.shape for g in got] == [e.shape for e in exp] == [(8, M - 11 + 2)] * 5
    agree = [int(np.argmin((g == e).all(0))) if not (g == e).all() else g.shape[1] for g, e in zip(got, exp)]
    print("static batch", sampling, "identical frame prefix per row:", agree, "of", got[0].shape[1])
    if sampling["temp"] == 0.0:
        _rows_leave_oracle_only_at_near_ties(got, exp, o, "B=5")
    else:
        assert min(agree) >= 8, agree  # tripwire next to the decision replay above: a CDF boundary within the bf16 logit noise of a draw moves the stream
    # EOS path: rows finish at different frames; dead rows are stepped but not recorded (static_batch.rs:160-173,328-331)
    got = lm.generate_static_batch(prompts, 150, seed=42, **sampling)
    exp = o.generate_batch(prompts, 150, seed=42, **sampling)
    for g, e in zip(got, exp):
        n = min(g.shape[1], e.shape[1], 8)
        assert np.array_equal(g[:, :n], e[:, :n])
    assert lm.last_stats()["frames"] == sum(g.shape[1] for g in got)


def test_fish14_legacy_slow_sampler_vs_oracle():
    """Fish <= 1.4 (single_batch.rs:104-124, sampling/mod.rs:8-26): the slow token is a 2-way {pad, <|im_end|>} draw that
    ignores the temperature; codebook embeddings are added only where the slow token == <|semantic|> (dual_ar.rs:558).
    Device and oracle draw the uniform from the same seeded StdRng stream, so token streams (incl. where EOS falls) agree."""
    tok14 = fcfg.TINY_1_4_TOKENS
    lm = fishrt.DualARTransformer(fcfg.TINY, tok14, 0, "f32").load_synthetic(SEED)
    o = orc.OracleLM(orc.TINY | tok14).load_synthetic(SEED)
    rng = np.random.RandomState(2)
    p = np.zeros((9, 9), np.uint32)
    p[0] = rng.randint(6, 400, 9)
    p[0, 3:6] = 5                                # a VQ span: slow token == <|semantic|>
    p[1:, 3:6] = rng.randint(0, 64, (8, 3))
    lg, hg = lm.forward_generate(p, 0)
    lo, ho = o.forward_generate(p, 0)
    np.testing.assert_allclose(hg, ho, **TOL32)
    n_eos = 0
    for seed in range(6):
        for kw in (dict(temp=0.0, top_p=1.0, top_k=0), dict(temp=0.8, top_p=0.9, top_k=16)):
            lm.clear_slow_layer_caches(); o.clear_slow()
            got = lm.generate_blocking(p, 60, repetition_penalty=1.2, seed=seed, **kw)
            exp = o.generate(p, 60, repetition_penalty=1.2, seed=seed, **kw)
            assert np.array_equal(got, exp), (seed, kw)
            assert lm.curr_kv_size() == o.kv_len()
            n_eos += exp.shape[1] < 60 - 9 + 2
    assert n_eos > 0, "the fixture never hit <|im_end|>: EOS path untested"
    lm.clear_slow_layer_caches(); o.clear_slow()
    got = lm.generate_blocking(p, 40, temp=0.0, top_p=1.0, top_k=0, repetition_penalty=1.0, seed=3, ignore_eos=True)
    assert got.shape == (8, 40 - 9 + 2)
    assert np.array_equal(got, o.generate(p, 40, temp=0.0, repetition_penalty=1.0, seed=3, ignore_eos=True))


def test_static_batch_more_rows_than_one_mfma_panel():
    """B = 40 > 32 rows: the static-batch GEMMs loop over two 32-row panels; every row must still equal the oracle's
    static_batch restatement (greedy; same-rounding bf16 weights and KV)."""
    lm = _tiny("bf16", 40)
    o = orc.OracleLM(orc.TINY).load_synthetic(SEED, bf16=True)
    o.set_kv_round_bf16(True)
    lens = [3 + (7 * i) % 11 for i in range(40)]
    prompts = _batch_prompts(40, lens)
    M = 30
    got = lm.generate_static_batch(prompts, M, seed=42, temp=0.0, top_p=1.0, top_k=0, ignore_eos=True)
    exp = o.generate_batch(prompts, M, seed=42, temp=0.0, top_p=1.0, top_k=0, ignore_eos=True)
    assert [g.shape for g in got] == [e.shape for e in exp]
    flips = _rows_leave_oracle_only_at_near_ties(got, exp, o, "B=40")
    print(f"B=40: {40 - flips}/40 rows identical to the oracle over {got[0].shape[1]} frames, {flips} left it at a near-tie")
    # sampled: per-row child RNG streams are indexed by (call, row) with B = 40 -- every decision of the 40 rows replayed through the oracle
    # batch sampler on the captured logits
    Fr = got[0].shape[1]
    lm.debug_capture(Fr)
    got = lm.generate_static_batch(prompts, M, seed=42, temp=0.7, top_p=0.8, top_k=32, ignore_eos=True)
    from test_batch_capture_gpu import replay_batch_decisions
    replay_batch_decisions(lm, 40, Fr, dict(temp=0.7, top_p=0.8, top_k=32), 42, got, n_audio=fcfg.TINY["vocab_size"] - fcfg.TINY_TOKENS["im_end_id"],
                           cb_size=fcfg.TINY["codebook_size"])
    lm.debug_capture(0)
    exp = o.generate_batch(prompts, M, seed=42, temp=0.7, top_p=0.8, top_k=32, ignore_eos=True)
    agree = [int(np.argmin((g == e).all(0))) if not (g == e).all() else g.shape[1] for g, e in zip(got, exp)]
    assert min(agree) >= 4 and np.mean(agree) >= 8, agree  # (tripwire; the replay above is the check)
    lm.close()


@pytest.fixture(scope="module")
def ofish3():
    o = orc.OracleLM(dict(orc.FISH15, n_layer=3)).load_synthetic(SEED, bf16=True)
    o.set_kv_round_bf16(True)
    return o


@pytest.mark.parametrize("B", [33, 40])
def test_fish_width_static_batch_beyond_32_rows_vs_oracle(B, ofish3):
    """Fish-1.5 width (16 heads of 64 dims over 2 kv heads, 3 slow layers) with more rows than one MFMA panel: the decode steps take
    k_attn_rows<bf16, 64, 4> (the 8 query heads of a kv head over two blocks), which no TINY / MID batch reaches.  B = 33: 2 * 2 * 33 = 132
    blocks, not a multiple of 16 -> the plain block mapping; B = 40: 160 blocks -> the XCD-aware mapping.  Greedy rows vs the oracle's
    static_batch restatement on the same bf16-rounded weights and K/V, near-tie referee as for the TINY B = 40 test."""
    lm = fishrt.DualARTransformer(dict(fcfg.FISH_1_5, n_layer=3), fcfg.FISH_1_5_TOKENS, 0, "bf16", B).load_synthetic(SEED)
    sem = fcfg.FISH_1_5_TOKENS["semantic_start_id"]
    rng = np.random.RandomState(1500 + B)
    prompts = []
    for i in range(B):
        L = 3 + (7 * i) % 11
        p = np.zeros((9, L), np.uint32)
        p[0] = rng.randint(0, 100000, L)
        if L >= 6:  # a VQ span so that codebook embeddings are exercised
            codes = rng.randint(0, 1024, (8, 3))
            p[0, 2:5] = sem + codes[0]
            p[1:, 2:5] = codes
        prompts.append(p)
    M = 13 + 6 - 2  # longest prompt 13 columns -> 6 frames
    got = lm.generate_static_batch(prompts, M, seed=42, temp=0.0, top_p=1.0, top_k=0, ignore_eos=True)
    lm.close()
    exp = ofish3.generate_batch(prompts, M, seed=42, temp=0.0, top_p=1.0, top_k=0, ignore_eos=True)
    assert [g.shape for g in got] == [e.shape for e in exp] == [(8, 6)] * B
    flips = _rows_leave_oracle_only_at_near_ties(got, exp, ofish3, f"fish B={B}")
    print(f"fish B={B}: {B - flips}/{B} rows identical to the oracle over 6 frames, {flips} left it at a near-tie")


# head_dim 64 at a small width: the configuration that takes the causal flash-attention prefill kernel and the group prefill of
# static batches (the TINY config has head_dim 32 and keeps the chunked row attention)
MID = dict(fcfg.TINY, dim=256, n_head=4, n_local_heads=2, head_dim=64, intermediate_size=1024)


def _mid(dtype, max_batch=1):
    return fishrt.DualARTransformer(MID, fcfg.TINY_TOKENS, 0, dtype, max_batch).load_synthetic(SEED)


def _omid():
    o = orc.OracleLM(dict(orc.TINY, dim=256, n_head=4, n_local_heads=2, head_dim=64, intermediate_size=1024)).load_synthetic(SEED, bf16=True)
    o.set_kv_round_bf16(True)
    return o


def test_mid_flash_prefill_vs_oracle():
    """forward_generate over 45 prompt tokens (one MFMA pass + causal flash attention, then a cached-prefix continuation of 20
    more) against the oracle on the same bf16-rounded weights / KV."""
    lm, o = _mid("bf16"), _omid()
    p = _batch_prompts(3, [65])[0]
    lg, hg = lm.forward_generate(np.ascontiguousarray(p[:, :45]), 0)
    lo, ho = o.forward_generate(np.ascontiguousarray(p[:, :45]), 0)
    np.testing.assert_allclose(hg, ho, **TOLBF)
    np.testing.assert_allclose(lg, lo, **TOLBF)
    lg, hg = lm.forward_generate(np.ascontiguousarray(p[:, 45:]), 45)
    lo, ho = o.forward_generate(np.ascontiguousarray(p[:, 45:]), 45)
    np.testing.assert_allclose(hg, ho, **TOLBF)
    np.testing.assert_allclose(lg, lo, **TOLBF)
    assert lm.curr_kv_size() == 65
    lm.close()


@pytest.mark.parametrize("B,span", [(5, 17), (37, 67)])  # (37, 67): 37 x 68 prompt rows > 2048 -> two group passes
def test_mid_static_batch_group_prefill_vs_oracle(B, span, monkeypatch):
    """Static batch whose prompts are prefilled as ONE group pass (rows = sequences x tokens) -- against the oracle, and
    bit-identical to the one-sequence-per-pass prefill (row results do not depend on where a row sits in a pass)."""
    lm, o = _mid("bf16", B), _omid()
    lens = [3 + (5 * i) % span for i in range(B)]
    prompts = _batch_prompts(11, lens)
    M = max(lens) + 14
    kw = dict(seed=42, temp=0.0, top_p=1.0, top_k=0, ignore_eos=True)
    got = lm.generate_static_batch(prompts, M, **kw)
    exp = o.generate_batch(prompts, M, **kw)
    assert [g.shape for g in got] == [e.shape for e in exp]
    flips = _rows_leave_oracle_only_at_near_ties(got, exp, o, f"B={B} group prefill")
    print(f"B={B} group prefill: {B - flips}/{B} rows identical to the oracle over {got[0].shape[1]} frames")
    monkeypatch.setenv("FISHRT_NO_GROUP_PREFILL", "1")
    seq = lm.generate_static_batch(prompts, M, **kw)
    monkeypatch.delenv("FISHRT_NO_GROUP_PREFILL")
    assert all(np.array_equal(a, b) for a, b in zip(got, seq))
    lm.close()


@pytest.mark.parametrize("which", ["tiny", "mid"])
def test_random_chunked_prefill_schedules_vs_oracle(which):
    """24 random prompts (1..90 tokens, random VQ columns) fed as random chunk schedules (single tokens, short and long chunks,
    i.e. decode kernels, small-M and multi-panel MFMA passes over growing cached prefixes; head_dim 32 -> chunked row attention,
    head_dim 64 -> flash prefill) -- the last chunk's logits / hidden state and the KV length against the oracle."""
    if which == "tiny":
        lm = _tiny("bf16")
        o = orc.OracleLM(orc.TINY).load_synthetic(SEED, bf16=True); o.set_kv_round_bf16(True)
    else:
        lm, o = _mid("bf16"), _omid()
    rng = np.random.RandomState(1234)
    worst = 0.0
    for case in range(24):
        L = int(rng.randint(1, 91))
        p = np.zeros((9, L), np.uint32)
        p[0] = rng.randint(0, 400, L)
        for col in np.nonzero(rng.rand(L) < 0.2)[0]:
            p[0, col] = 401 + rng.randint(0, 64)
            p[1:, col] = rng.randint(0, 64, 8)
        cuts = sorted(set([0, L] + [int(c) for c in rng.randint(0, L + 1, rng.randint(0, 5))]))
        lm.clear_slow_layer_caches(); o.clear_slow()
        for a, b in zip(cuts[:-1], cuts[1:]):
            chunk = np.ascontiguousarray(p[:, a:b])
            lg, hg = lm.forward_generate(chunk, a)
            lo, ho = o.forward_generate(chunk, a)
        assert lm.curr_kv_size() == L
        np.testing.assert_allclose(hg, ho, **TOLBF, err_msg=f"case {case}: L={L} cuts={cuts}")
        np.testing.assert_allclose(lg, lo, **TOLBF, err_msg=f"case {case}: L={L} cuts={cuts}")
        worst = max(worst, float(np.abs(lg - lo).max()))
    print(f"{which}: 24 random chunk schedules, worst |dlogit| {worst:.2e}")
    lm.close()


@pytest.mark.parametrize("which", ["tiny", "mid"])
def test_static_batch_sizes_around_panel_boundaries_vs_oracle(which):
    """Static batches of 1, 2, 15, 16, 17, 33 and 64 rows (half-panel GEMM variant up to 16 rows, one / two / several 32-row panels,
    fused row attention with and without the head split) with ragged prompts -- every row against the oracle's static_batch."""
    if which == "tiny":
        lm = _tiny("bf16", 64)
        o = orc.OracleLM(orc.TINY).load_synthetic(SEED, bf16=True); o.set_kv_round_bf16(True)
    else:
        lm, o = _mid("bf16", 64), _omid()
    rng = np.random.RandomState(77)
    kw = dict(seed=42, temp=0.0, top_p=1.0, top_k=0, ignore_eos=True)
    for B in (1, 2, 15, 16, 17, 33, 64):
        lens = [int(x) for x in rng.randint(2, 40, B)]
        prompts = _batch_prompts(1000 + B, lens)
        M = max(lens) + 12
        got = lm.generate_static_batch(prompts, M, **kw)
        exp = o.generate_batch(prompts, M, **kw)
        assert [g.shape for g in got] == [e.shape for e in exp]
        # bf16 near-ties (flat logits of random weights) flip a few rows somewhere in a 14-frame free run; every flip must sit on a
        # near-tie of the oracle (a wrong row / position / panel mapping breaks rows on ordinary margins, at frame 0)
        flips = _rows_leave_oracle_only_at_near_ties(got, exp, o, f"{which} B={B}")  # (asserts the near-tie for every row that left)
        print(f"{which} B={B}: {B - flips}/{B} rows identical to the oracle, {flips} left it on a near-tie the oracle reports")
    lm.close()


def test_static_batch_single_token_prompts_and_max_rows():
    """Edge cases of the static-batch row path: prompts of ONE token (no prefill pass at all: Lmax - 1 == 0), mixed 1 / 2-token
    prompts, and the maximum of 256 rows -- against the oracle's static_batch restatement."""
    o = _omid()
    kw = dict(seed=42, temp=0.0, top_p=1.0, top_k=0, ignore_eos=True)
    lm = _mid("bf16", 256)
    for lens in ([1, 1, 1], [1, 2], [2]):
        prompts = _batch_prompts(5 + len(lens), lens)
        got = lm.generate_static_batch(prompts, max(lens) + 6, **kw)
        exp = o.generate_batch(prompts, max(lens) + 6, **kw)
        assert [g.shape for g in got] == [e.shape for e in exp]
        _rows_leave_oracle_only_at_near_ties(got, exp, o, f"lens {lens}")
    lens = [2 + (i * 7) % 13 for i in range(256)]
    prompts = _batch_prompts(99, lens)
    got = lm.generate_static_batch(prompts, max(lens) + 4, **kw)
    exp = o.generate_batch(prompts, max(lens) + 4, **kw)
    assert len(got) == 256 and [g.shape for g in got] == [e.shape for e in exp]
    flips = _rows_leave_oracle_only_at_near_ties(got, exp, o, "256 rows")
    print(f"256 rows: {256 - flips} identical to the oracle over all 6 frames, {flips} left it at a near-tie")
    lm.close()
    # more prompts than the handle's max_batch: rows are generated one after another on KV slot 0 (same tokens under greedy decoding)
    small = fishrt.DualARTransformer(MID, fcfg.TINY_TOKENS, 0, "bf16", 4).load_synthetic(SEED)
    seq = small.generate_static_batch(prompts[:5], max(lens[:5]) + 4, **kw)
    exp5 = o.generate_batch(prompts[:5], max(lens[:5]) + 4, **kw)
    assert [g.shape for g in seq] == [e.shape for e in exp5] and all(np.array_equal(g[:, 0], e[:, 0]) for g, e in zip(seq, exp5))
    small.close()
