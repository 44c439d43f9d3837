"""CPU: the frame-by-frame sampler definitions of tests/sample_refs.py are pinned against independent code -- the window machine against
the oracle's RepPen (orc_reppen_*), the ArgMax rules and the RNG numbering against the oracle's entry points, the whole single-sequence
and static-batch machines against OracleLM.generate / generate_batch on the TINY config with teacher-forced logits -- every mutation of
the machines changes the expected trace of the cases listed for it, the case list reaches every production sampler kernel, and the hook
refuses the rejected cases before any device call."""
import ctypes as C

import numpy as np
import pytest

import sample_refs as sr
from oracle import oracle as orc

F32, U32, I32 = np.float32, np.uint32, np.int32


# ---------------------------------------------------------------------------------------------------------------- the window
def _orc_window(vocab, amt, toks, rows):
    L = orc.lib()
    r = C.c_void_p(L.orc_reppen_create(vocab, 16, C.c_float(amt)))
    out = []
    for t, row in zip(toks, rows):
        lg = np.array(row, F32)
        assert L.orc_reppen_apply(r, lg.ctypes.data_as(C.POINTER(C.c_float)), vocab, int(t)) == 0
        m = np.zeros(vocab, F32)
        L.orc_reppen_mask(r, m.ctypes.data_as(C.POINTER(C.c_float)))
        out.append((lg, m))
    L.orc_reppen_destroy(r)
    return out


def _window_sequences():
    seqs = [[ev[1] if ev[0] == "pick" else (ev[1] if ev[0] == "probe" else 63) for ev in s] for s in sr.window_scripts(40)]
    r = np.random.RandomState(3)
    seqs += [r.randint(0, 6, 60).tolist(), r.randint(0, 20, 80).tolist(), [7] * 40, r.randint(0, 64, 200).tolist()]
    return seqs


@pytest.mark.parametrize("amt", [1.0, 1.2, 1.5])
def test_window_machine_matches_oracle_reppen(amt):
    r = np.random.RandomState(1)
    for toks in _window_sequences():
        rows = (r.standard_normal((len(toks), 64)) * 2).astype(F32)
        w = sr.PenWindow(64, amt)
        for (lg, m), t, row in zip(_orc_window(64, amt, toks, rows), toks, rows):
            w.push(t)
            assert np.array_equal(w.mask.view(U32), m.view(U32))
            assert np.array_equal(w.apply(row).view(U32), lg.view(U32))
            # the ring the device keeps is the same deque: newest first from `head`, len saturating at 16
            assert [int(w.ring_[(w.head + i) % 17]) for i in range(w.len)] == w.ctx[: w.len]
            if amt == 1.0:
                assert (w.mask == 1.0).all()


# ---------------------------------------------------------------------------------------------------------------- ArgMax rules, RNG numbering
def test_total_key_is_the_oracle_host_argmax():
    r = np.random.RandomState(2)
    s = sr.Stream(1, 0.0, 1.0, 0)
    for row in sr.tie_rows(r, 2037, 1) + sr.tie_rows(r, 64, 2) + [np.array([-0.0, 0.0, -0.0], F32), np.array([0.0, -0.0, 0.0, -1.0], F32)]:
        k = sr.total_key(row)
        assert s.sample(row) == len(k) - 1 - int(np.argmax(k[::-1]))


def test_batch_argmax_is_first_max_ieee():
    r = np.random.RandomState(2)
    for row in sr.tie_rows(r, 64, 1):
        assert sr.batched_pick(1, 0.0, 1.0, 0, row[None], 5)[0] == int(np.argmax(row))


def test_child_words_and_call_numbering():
    # the word table's numbers ARE the children orc_batched_sample draws with: picks of call c on B rows == picks of the same rows as
    # one-row batches at call index c * B + b
    r = np.random.RandomState(4)
    for B in (1, 3, 9):
        rows = (r.standard_normal((B, 64)) * 2).astype(F32)
        for call in (0, 1, 7):
            full = sr.batched_pick(42, 0.8, 0.9, 16, rows, call)
            one = [sr.batched_pick(42, 0.8, 0.9, 16, rows[b][None], call * B + b)[0] for b in range(B)]
            assert full.tolist() == one
    u = sr.stream_u64(42, 8)
    w = sr.stream_words(42, 16)
    assert [int(u[i]) for i in range(8)] == [int(w[2 * i]) | (int(w[2 * i + 1]) << 32) for i in range(8)]
    assert sr.child_word(42, 5) == int(sr.stream_words(int(u[5]), 1)[0])


def test_nodraw_stream_returns_zero():
    s = sr.Stream(9, 0.9, 0.0, 0)
    r = np.random.RandomState(5)
    assert all(s.sample((r.standard_normal(64) * 2).astype(F32)) == 0 for _ in range(8))


# ---------------------------------------------------------------------------------------------------------------- whole machines vs the generators
TINY = orc.TINY
SEED = 0xF15E5EED


def _teacher_forced(lm, prompt, frames_tokens):
    """logits of every decision of a run whose iteration i produced frames_tokens[i] = [slow, c0..]: forward_generate / forward_generate_fast"""
    Cb, V = TINY["num_codebooks"], TINY["vocab_size"]
    lm.clear_slow()
    cur, pos = np.asarray(prompt, U32), 0
    out = []
    for toks in frames_tokens:
        logits, hidden = lm.forward_generate(cur, pos)
        pos += cur.shape[-1]
        lm.clear_fast()
        x = hidden[0]
        fast = []
        for ci in range(Cb):
            fast.append(lm.forward_generate_fast(x, ci)[0].copy())
            x = lm.fast_embeddings()[int(toks[ci + 1])]
        out.append((logits[0, TINY["im_end_id"]:].copy(), np.stack(fast)))
        cur = np.asarray(toks, U32).reshape(Cb + 1, 1)
    return out


def _run_single(lm, prompt, n_frames, cfg, ignore_eos):
    """drive the single-sequence machine with the oracle model in the loop: each launch's logits come from the model, fed the machine's own
    picks; returns the machine's emitted codes"""
    Cb = TINY["num_codebooks"]
    tokens = dict(im_end_id=TINY["im_end_id"], pad_id=TINY["pad_id"], semantic_start_id=TINY["semantic_start_id"],
                  semantic_end_id=TINY["semantic_end_id"], has_semantic_end=1)
    n_slow = TINY["vocab_size"] - TINY["im_end_id"]
    logits = [(np.zeros((1, n_slow), F32), np.zeros((Cb, 1, TINY["codebook_size"]), F32)) for _ in range(n_frames)]
    case = sr.Case("pin/single", "single", [dict(cfg, ignore_eos=int(ignore_eos))], logits, B=1, n_cb=Cb, cb_size=TINY["codebook_size"], n_slow=n_slow,
                   dim=TINY["dim"], tokens=tokens, out_cap=n_frames + 2, wt="f32")
    m = sr.Machine(case)
    m.fast = lm.fast_embeddings()  # (the picks do not depend on the tables; XF does, and is not looked at here)
    lm.clear_slow()
    cur, pos = np.asarray(prompt, U32), 0
    for f in range(n_frames):
        if m.st[0][sr.DONE]:
            break
        lg, hidden = lm.forward_generate(cur, pos)
        pos += cur.shape[-1]
        logits[f][0][0] = lg[0, TINY["im_end_id"]:]
        m.single_slow(f)
        lm.clear_fast()
        x = hidden[0]
        for ci in range(Cb):
            if m.st[0][sr.CUR] != TINY["im_end_id"]:
                logits[f][1][ci][0] = lm.forward_generate_fast(x, ci)[0]
            m.single_fast(f, ci)
            x = lm.fast_embeddings()[int(m.st[0][sr.CUR + ci + 1])]
        cur = m.st[0][sr.CUR: sr.CUR + Cb + 1].astype(U32).reshape(Cb + 1, 1)
    n = int(m.st[0][sr.NOUT])
    return m.codes[0][:, :n].copy(), m


@pytest.fixture(scope="module")
def tiny_lm():
    return orc.OracleLM(TINY).load_synthetic(SEED)


def _prompt(L=6):
    p = np.zeros((9, L), U32)
    p[0] = np.random.RandomState(0).randint(0, 400, L)
    return p


@pytest.mark.parametrize("cfg", [dict(temp=0.0, top_p=1.0, top_k=0, rep_pen=1.2, seed=3), dict(temp=0.7, top_p=0.8, top_k=16, rep_pen=1.2, seed=3),
                                 dict(temp=0.9, top_p=0.9, top_k=0, rep_pen=1.5, seed=11)])
def test_single_machine_matches_oracle_generate(tiny_lm, cfg):
    prompt = _prompt()
    n = 24
    tiny_lm.clear_slow()
    exp = tiny_lm.generate(prompt, prompt.shape[1] + n - 2, temp=cfg["temp"], top_p=cfg["top_p"], top_k=cfg["top_k"], repetition_penalty=cfg["rep_pen"],
                           seed=cfg["seed"], ignore_eos=True)
    got, _ = _run_single(tiny_lm, prompt, n, cfg, True)
    assert exp.shape[1] == n - 1 or exp.shape[1] == n
    assert np.array_equal(got[:, : exp.shape[1]], exp)


def test_single_machine_ends_on_im_end(tiny_lm):
    # without ignore_eos: find a sampled run that ends on <|im_end|> by itself (hot sampling over the whole audio range), then compare
    prompt = _prompt()
    for seed in range(40):
        cfg = dict(temp=3.0, top_p=1.0, top_k=0, rep_pen=1.2, seed=seed)
        tiny_lm.clear_slow()
        exp = tiny_lm.generate(prompt, prompt.shape[1] + 60, temp=cfg["temp"], top_p=cfg["top_p"], top_k=cfg["top_k"], repetition_penalty=cfg["rep_pen"],
                               seed=seed, ignore_eos=False)
        if 2 <= exp.shape[1] < 50:
            got, m = _run_single(tiny_lm, prompt, 62, cfg, False)
            assert m.st[0][sr.DONE] == 2 and np.array_equal(got, exp)
            return
    pytest.fail("no seed ended on <|im_end|>")


@pytest.mark.parametrize("temp", [0.0, 0.8])
def test_batch_machine_matches_oracle_generate_batch(tiny_lm, temp):
    Cb, B, n = TINY["num_codebooks"], 3, 6
    prompts = [_prompt(5) for _ in range(B)]
    for b in range(B):
        prompts[b][0] = np.random.RandomState(10 + b).randint(0, 400, 5)
    cfg = dict(temp=temp, top_p=0.9, top_k=16, seed=42)
    tiny_lm.clear_slow()
    exp = tiny_lm.generate_batch(prompts, 5 + n - 2, temp=temp, top_p=0.9, top_k=16, seed=42, ignore_eos=True)
    tokens = dict(im_end_id=TINY["im_end_id"], pad_id=TINY["pad_id"], semantic_start_id=TINY["semantic_start_id"],
                  semantic_end_id=TINY["semantic_end_id"], has_semantic_end=1)
    n_slow = TINY["vocab_size"] - TINY["im_end_id"]
    nf = exp[0].shape[1]
    logits = [(np.zeros((B, n_slow), F32), np.zeros((Cb, B, TINY["codebook_size"]), F32)) for _ in range(nf)]
    case = sr.Case("pin/rows", "rows", [dict(cfg, ignore_eos=1)], logits, B=B, n_cb=Cb, cb_size=TINY["codebook_size"], n_slow=n_slow, dim=TINY["dim"],
                   tokens=tokens, out_cap=nf + 2, wt="f32")
    m = sr.Machine(case)
    m.fast = tiny_lm.fast_embeddings()
    tiny_lm.clear_slow()
    cur, pos = np.stack(prompts), 0
    for f in range(nf):
        lg, hidden = tiny_lm.forward_generate(cur, pos)
        pos += cur.shape[-1]
        logits[f][0][:] = lg[:, TINY["im_end_id"]:]
        m.rows_slow(f)
        tiny_lm.clear_fast()
        x = hidden
        for ci in range(Cb):
            logits[f][1][ci][:] = tiny_lm.forward_generate_fast(x, ci)
            m.rows_fast(f, ci)
            x = tiny_lm.fast_embeddings()[m.st[:, sr.CUR + ci + 1].astype(int)]
        cur = m.st[:, sr.CUR: sr.CUR + Cb + 1].astype(U32).reshape(B, Cb + 1, 1)
    for b in range(B):
        assert np.array_equal(m.codes[b][:, :nf], exp[b])


# ---------------------------------------------------------------------------------------------------------------- cases, mutations, validation
def test_case_table_reaches_every_production_kernel():
    reached = set()
    for c in sr.all_cases():
        reached |= set(c.kernels())
    assert reached == set(sr.PRODUCTION_KERNELS)
    assert set(sr.FAMILY_KERNELS) == set(sr.FAMILIES)
    for fam in sr.FAMILIES:  # ... and every family with both table types
        assert {c.wt for c in sr.all_cases() if c.family == fam} >= {"bf16"}
    assert {c.wt for c in sr.all_cases()} == {"bf16", "f32"}


def test_scripts_make_their_events_happen():
    ref = sr.reference(sr.case_by_name("window/single/1.2"))
    F, Lf = 24, 9
    picks = ref["STATES"].view(I32)[:, 0, sr.CUR + 1: sr.CUR + 9]
    at = lambda f, cb: int(picks[f * Lf + 1 + cb, cb])
    assert at(15, 0) == sr.Bq and at(16, 1) == sr.Bq and at(17, 2) == sr.A      # ages 15, 16 penalised; 17 not
    assert at(17, 3) == sr.A and at(22, 4) == sr.A and at(17, 5) == sr.A        # the reference quirk, last == dropped
    assert at(16, 6) == sr.A and at(17, 7) == sr.Bq                              # the division raises a penalised negative logit
    assert at(2, 0) == 63                                                        # the tie the division creates: the later index
    ref1 = sr.reference(sr.case_by_name("window/single/1.0"))
    assert (ref1["MASK"].view(F32) == 1.0).all()


@pytest.mark.parametrize("mut", sorted(sr.MUTATIONS))
def test_mutation_changes_a_listed_case(mut):
    assert len(sr.MUTATIONS) >= 12
    for name in sr.MUTATIONS[mut]:
        case = sr.case_by_name(name)
        assert sr.traces_differ(sr.reference(case), sr.reference(case, mut)), (mut, name)


@pytest.mark.parametrize("label,case,over,msg", sr.rejected_cases(), ids=[r[0] for r in sr.rejected_cases()])
def test_hook_rejects_before_any_device_call(label, case, over, msg):
    rc, err = sr.call_rejected(case, over)
    assert rc != 0 and msg in err, err


def test_hook_plan_only_needs_no_device():
    from fishrt import _ffi
    case = sr.case_by_name("rng/rows_par/B3")
    c, keep = case.ffi(plan_only=True)
    o = _ffi.SampleOut()
    _ffi.check(_ffi.lib().fs_selftest_sample_frames(0, C.byref(c), C.byref(o)))
    assert o.n_launches == case.F * case.Lf == 3 * 4
    assert o.need[_ffi.SAMPLE_OUTS.index("STATES")] == o.n_launches * case.B * 160
    assert o.need[_ffi.SAMPLE_OUTS.index("WORDS")] == o.n_launches * case.B * 64
    assert C.sizeof(_ffi.SampleCase) == 28 * 4 + 10 * 8 and C.sizeof(_ffi.SampleOut) == 3 * 13 * 8 + 8
