"""GPU: hidden states of session slots (fs_lm_session_add_hidden / fs_lm_session_poll_hidden; Session.add(collect_hidden=True) /
Session.poll_hidden).  Fish-1.5 shapes, synthetic bf16 weights, prompts of 20-40 positions, 8 frames per slot, greedy unless stated.

Where row 0 comes from: a slot's prefill pass runs its first L - 1 prompt positions only; the LAST prompt position -- the iteration whose
frame is emitted unconditionally -- is the slot's first decode step, in every session kind and for solo, group and prefixed admissions
alike.  So every row, row 0 included, is stored by the step's k_hidden_rows node and is a decode-path row."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import fishrt
from fishrt import config as fcfg

SEED = 0xF15E5EED
TOK = fcfg.FISH_1_5_TOKENS
IM_END = TOK["im_end_id"]
DIM = fcfg.FISH_1_5["dim"]
F = 8
MODES = ["plain", "per_slot", "rows"]
# the EOS-heavy synthetic checkpoint of tests/test_session_per_slot_gpu.py::test_eos_ends_a_slot_like_its_own_generate_call
EOS_CFG = dict(fcfg.FISH_1_5, n_layer=4, vocab_size=4096, max_seq_len=2048)
EOS_TOK = dict(im_end_id=2059, pad_id=5, semantic_start_id=2060, semantic_end_id=3083, has_semantic_end=1)
EOS_BOOST = 6.0


def _prompt(L, seed, hi=IM_END):
    p = np.zeros((9, L), np.uint32)
    p[0] = np.random.RandomState(seed).randint(0, hi, L)
    return p


@pytest.fixture(scope="module")
def lm8():
    lm = fishrt.DualARTransformer(fcfg.FISH_1_5, TOK, 0, "bf16", max_batch=8).load_synthetic(SEED)
    yield lm
    lm.close()


@pytest.fixture(scope="module")
def lm4():
    lm = fishrt.DualARTransformer(fcfg.FISH_1_5, TOK, 0, "bf16", max_batch=4).load_synthetic(SEED)
    yield lm
    lm.close()


@pytest.fixture(scope="module")
def lm_eos(tmp_path_factory):
    import test_safetensors_gpu as tsf
    t = tsf._lm_tensors(EOS_CFG, bf16=True)
    t["output.weight"][EOS_TOK["im_end_id"]] *= np.float32(EOS_BOOST)
    t["output.weight"] = (t["output.weight"].view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    path = str(tmp_path_factory.mktemp("eos_hidden") / "model.safetensors")
    tsf._save(t, path, True)
    lm = fishrt.DualARTransformer(EOS_CFG, EOS_TOK, 0, "bf16", max_batch=8).load_safetensors(path)
    os.remove(path)
    yield lm
    lm.close()


def _session(lm, mode, ignore_eos=True, **kw):
    kw = dict(dict(temp=0.0, top_p=1.0, top_k=0, seed=5, repetition_penalty=1.2), **kw)
    return lm.session(ignore_eos=ignore_eos, rows=mode == "rows", per_slot=mode == "per_slot", **kw)


def _run_all(s):
    while s.step(F):
        pass


def _budget(p, frames=F):
    return p.shape[1] + frames - 2  # 1 + max(0, max_new_tokens - L + 1) == frames iterations


def _handle(mode, lm8, lm4):
    return lm4 if mode == "rows" else lm8


def _collect_run(lm, mode, prompts, collect):
    """all prompts admitted at once, run to the end -> ([codes], {index: rows})"""
    with _session(lm, mode) as s:
        slots = [s.add(p, _budget(p), collect_hidden=i in collect) for i, p in enumerate(prompts)]
        assert None not in slots and len(set(slots)) == len(prompts)
        _run_all(s)
        codes = [s.poll(sl)[0] for sl in slots]
        rows = {i: s.poll_hidden(slots[i]) for i in collect}
    return codes, rows


@pytest.mark.parametrize("mode", MODES)
def test_collection_changes_nothing_else(mode, lm8, lm4):
    """the same session with slots {0, 2} collecting, with none, with {0, 2} again and with all four: every slot's codes are bit-identical
    in all runs; a collecting slot's rows are bit-identical between the two identical runs and when its neighbours collect too"""
    lm = _handle(mode, lm8, lm4)
    prompts = [_prompt(L, 100 + i) for i, L in enumerate((23, 40, 31, 20))]
    c_some, r_some = _collect_run(lm, mode, prompts, {0, 2})
    c_none, r_none = _collect_run(lm, mode, prompts, set())
    c_again, r_again = _collect_run(lm, mode, prompts, {0, 2})
    c_all, r_all = _collect_run(lm, mode, prompts, {0, 1, 2, 3})
    assert r_none == {}
    for i in range(4):
        assert c_some[i].shape == (8, F)
        for other in (c_none, c_again, c_all):
            assert np.array_equal(c_some[i], other[i]), (mode, i)
    for i in (0, 2):
        assert r_some[i].shape == (F, DIM) and r_some[i].dtype == np.float32 and np.isfinite(r_some[i]).all()
        assert np.array_equal(r_some[i], r_again[i]), (mode, i)
        assert np.array_equal(r_some[i], r_all[i]), (mode, i)
        assert (np.abs(np.diff(r_some[i], axis=0)).max(axis=1) > 1e-2).all(), "consecutive rows repeat"
    assert not np.array_equal(r_some[0], r_some[2])


@pytest.mark.parametrize("mode", MODES)
def test_row_count_tail_readmission_and_errors(mode, lm8, lm4):
    """ignore_eos: n_rows == n_frames; poll_hidden(first > 0) is the tail; a slot still prefilling has no rows; a non-collecting slot
    raises; a slot released and re-admitted starts again at row 0 (its rows are those of the new request, not appended to the old)"""
    lm = _handle(mode, lm8, lm4)
    pa, pb, pc = _prompt(26, 200), _prompt(33, 201), _prompt(21, 202)
    with _session(lm, mode) as s:
        a = s.add(pa, _budget(pa), collect_hidden=True)
        b = s.add(pb, _budget(pb))
        assert s.poll_hidden(a).shape == (0, DIM)  # (queued: nothing ran yet)
        with pytest.raises(RuntimeError, match="does not collect"):
            s.poll_hidden(b)
        s.step(3)
        assert s.poll(a, codes=False)[0] == 3 and s.poll_hidden(a).shape == (3, DIM)
        _run_all(s)
        codes_a, done = s.poll(a)
        rows_a = s.poll_hidden(a)
        assert done and codes_a.shape == (8, F) and rows_a.shape == (F, DIM)
        assert np.array_equal(s.poll_hidden(a, first=5), rows_a[5:])
        assert s.poll_hidden(a, first=F).shape == (0, DIM) and s.poll_hidden(a, first=F + 3).shape == (0, DIM)
        s.release(a)
        with pytest.raises(RuntimeError, match="not a live session slot"):
            s.poll_hidden(a)
        a2 = s.add(pc, _budget(pc, 5), collect_hidden=True)
        assert a2 == a, "the lowest free slot is handed out first"
        _run_all(s)
        rows_c = s.poll_hidden(a2)
        assert s.poll(a2)[0].shape == (8, 5) and rows_c.shape == (5, DIM)
        assert np.abs(rows_c[0] - rows_a[0]).max() > 1e-2
        s.release(a2)
        a3 = s.add(pa, _budget(pa))  # the same slot again, now without collection
        assert a3 == a
        with pytest.raises(RuntimeError, match="does not collect"):
            s.poll_hidden(a3)
        _run_all(s)
        assert s.poll(a3)[0].shape == codes_a.shape
    # the re-admitted slot's row 0 is the row of ITS prompt's last position
    lm.clear_slow_layer_caches()
    _, h0 = lm.forward_generate(pc, 0)
    lm.clear_slow_layer_caches()
    np.testing.assert_allclose(rows_c[0], h0.reshape(-1), rtol=2e-3, atol=1e-3)


@pytest.mark.parametrize("mode", MODES)
def test_terminating_iteration_adds_a_row(mode, lm_eos):
    """without ignore_eos on the EOS-heavy checkpoint: a slot has one row per iteration it ran -- n_frames rows when it ran out of budget or
    sampled <|im_end|> in its very first iteration (that frame is emitted unconditionally), n_frames + 1 when a later iteration sampled
    <|im_end|> (its frame is not emitted).  Two rounds of 8 slots, the second re-using the slots of the first."""
    lm = lm_eos
    plus_one, seen = 0, []
    with _session(lm, mode, ignore_eos=False) as s:
        for rnd in range(2):
            prompts = [_prompt(20 + (7 * i + rnd) % 21, 4000 + 8 * rnd + i, EOS_TOK["im_end_id"]) for i in range(8)]
            slots = [s.add(p, _budget(p), collect_hidden=True) for p in prompts]
            assert sorted(slots) == list(range(8))
            _run_all(s)
            for sl in slots:
                codes, done = s.poll(sl)
                rows = s.poll_hidden(sl)
                n, r = codes.shape[1], rows.shape[0]
                seen.append((n, r))
                assert done and 1 <= n <= F and r in (n, n + 1), (mode, sl, n, r)
                if n == F:
                    assert r == F  # the budget ended it
                elif n > 1:
                    assert r == n + 1  # <|im_end|> in iteration n >= 1: a row, no frame
                # (n == 1 < F: <|im_end|> in iteration 0, r == 1, or in iteration 1, r == 2)
                assert np.isfinite(rows).all()
                plus_one += r == n + 1
                s.release(sl)
    print(f"{mode}: (frames, rows) per slot: {seen}")
    assert plus_one >= 1, "no slot ended on <|im_end|> after its first frame: the terminating iteration's row went untested"


def _teacher_forced(lm, prompt, codes, slow_picks, n_rows):
    """`hidden` of forward_generate(prompt ++ the slot's own frames [:, :L + i], 0) for i < n_rows, on cleared caches"""
    L = prompt.shape[1]
    n = codes.shape[1]
    frames = np.zeros((9, n), np.uint32)
    frames[0] = IM_END + slow_picks[:n]
    frames[1:] = codes
    mat = np.ascontiguousarray(np.concatenate([prompt, frames], 1))
    out = np.zeros((n_rows, DIM), np.float32)
    for i in range(n_rows):
        lm.clear_slow_layer_caches()
        _, h = lm.forward_generate(np.ascontiguousarray(mat[:, : L + i]), 0)
        out[i] = h.reshape(-1)
    lm.clear_slow_layer_caches()
    return out


@pytest.mark.parametrize("mode", MODES)
def test_values_against_teacher_forced_prefill(mode, lm8, lm4):
    """Every row i of every collecting slot against forward_generate(prompt ++ the slot's own first i frames, 0).hidden -- a decode-path
    row against the one-pass MFMA prefill, the comparison of tests/test_lm_gpu.py:210 and its bound (rtol 2e-3, atol 1e-3); consecutive
    rows differ by more than 1e-2 somewhere (:211).  One session holds: a slot joined on a shared prefix of 37 positions (partly filled
    last page), two slots prefilled together in a group pass, and a slot that joins while the others are mid-generation (prefilled alone
    on the second stream).  The frames' slow tokens come from the decision capture (the codes do not carry them).

    Row 0 of the solo-prefilled slot: the session's prefill pass covers positions [0, L - 1) only and the last prompt position is the
    slot's first DECODE step (module docstring), so it is not a one-pass prefill on both sides and the one-pass class's bound (rtol 1e-5,
    atol 1e-6, tests/test_lm_gpu.py:190) does not apply; its distance is printed and it keeps the decode-path bound."""
    lm = _handle(mode, lm8, lm4)
    prefix, body = _prompt(37, 300), _prompt(3, 301)
    reqs = [np.ascontiguousarray(np.concatenate([prefix, body], 1)), _prompt(24, 302), _prompt(31, 303), _prompt(29, 304)]
    lm.debug_capture(F)
    try:
        with _session(lm, mode) as s:
            pid = s.add_prefix(prefix)
            slots = [s.add(body, _budget(reqs[0]), prefix=pid, collect_hidden=True)]
            slots += [s.add(p, _budget(p), collect_hidden=True) for p in reqs[1:3]]
            s.step(3)
            info = s.info()
            assert info["prefill_passes"] == 2 and info["tail_pages_copied"] == 1, info  # the prefix's pass + ONE group pass of three
            assert [s.poll(sl, codes=False)[0] for sl in slots] == [3, 3, 3]
            slots.append(s.add(reqs[3], _budget(reqs[3]), collect_hidden=True))  # joins mid-generation
            _run_all(s)
            assert s.info()["prefill_passes"] == 3
            codes = [s.poll(sl)[0] for sl in slots]
            rows = [s.poll_hidden(sl) for sl in slots]
        picks = [lm.debug_read_row(sl, F)[:, 0, 2047].astype(np.int64) for sl in slots]
    finally:
        lm.debug_capture(0)
    for i, (p, c, r, pk) in enumerate(zip(reqs, codes, rows, picks)):
        assert c.shape == (8, F) and r.shape == (F, DIM)
        assert (pk >= 1).all(), "ignore_eos: no <|im_end|> pick"
        ref = _teacher_forced(lm, p, c, pk, F)
        err = np.abs(r - ref)
        print(f"{mode} slot {slots[i]} (L {p.shape[1]}): max |row - teacher-forced| per row {np.round(err.max(1), 6).tolist()}")
        np.testing.assert_allclose(r, ref, rtol=2e-3, atol=1e-3)
        assert (np.abs(np.diff(r, axis=0)).max(axis=1) > 1e-2).all(), "consecutive rows repeat"
    lm.clear_slow_layer_caches()
    _, h0 = lm.forward_generate(reqs[3], 0)
    lm.clear_slow_layer_caches()
    print(f"{mode} solo-prefilled slot, row 0 vs forward_generate(prompt, 0): max abs {np.abs(rows[3][0] - h0.reshape(-1)).max():.3e}")
    np.testing.assert_allclose(rows[3][0], h0.reshape(-1), rtol=2e-3, atol=1e-3)


def _mixed_run(lm, collect):
    """sampled per-slot session, slots admitted and released across steps -> ({request: codes}, {request: rows}, graph launches)"""
    sampling = dict(temp=0.7, top_p=0.8, top_k=256, repetition_penalty=1.4)
    prompts = [_prompt(20 + (5 * i) % 21, 500 + i) for i in range(12)]
    codes, rows, live, nxt = {}, {}, {}, 0
    with _session(lm, "per_slot", seed=3, **sampling) as s:
        while nxt < len(prompts) or live:
            while nxt < len(prompts) and len(live) < 6:  # admissions trickle in: one or two per round, at most 6 slots live
                sl = s.add(prompts[nxt], _budget(prompts[nxt]), seed=7000 + nxt, collect_hidden=nxt in collect)
                assert sl is not None
                live[sl] = nxt
                nxt += 1
                if len(live) % 2 == 0:
                    break
            s.step(3)
            for sl in list(live):
                n, done = s.poll(sl, codes=False)
                if done:
                    i = live.pop(sl)
                    codes[i] = s.poll(sl)[0]
                    if i in collect:
                        rows[i] = s.poll_hidden(sl)
                    s.release(sl)
        launches = lm.last_stats()["graph_launches"]
    return codes, rows, launches


def test_mixed_sampled_session_admits_and_releases_collectors(lm8):
    """sampled per-slot session (0.7 / 0.8 / 256, penalty 1.4), 12 requests through at most 6 live slots of the 8, every third one collecting, admitted and
    released across steps.  The session exposes no count of graph CAPTURES (fs_lm_last_stats.graph_launches counts replays), so the
    one-graph property is checked through what it guarantees: every request's codes are bit-identical to a run without any collector
    and to a run where all collect (a step graph that depended on the collectors would have to differ between these), with the same
    number of replays; rows are identical between the mixed and the all-collecting run."""
    some = {i for i in range(12) if i % 3 == 0}
    c_some, r_some, n_some = _mixed_run(lm8, some)
    c_none, r_none, n_none = _mixed_run(lm8, set())
    c_all, r_all, n_all = _mixed_run(lm8, set(range(12)))
    assert n_some == n_none == n_all and n_some > 0
    assert r_none == {} and set(r_some) == some and set(r_all) == set(range(12))
    for i in range(12):
        assert c_some[i].shape == (8, F)
        assert np.array_equal(c_some[i], c_none[i]) and np.array_equal(c_some[i], c_all[i]), i
    for i in some:
        assert r_some[i].shape == (F, DIM) and np.array_equal(r_some[i], r_all[i]), i
    assert len({r.tobytes() for r in r_all.values()}) == 12
