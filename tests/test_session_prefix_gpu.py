"""GPU: shared conditioning prefixes of a continuous-batching session (fs_lm_session_prefix_create / _release / fs_lm_session_add_prefixed /
fs_lm_session_info, include/fishrt.h).  A slot admitted on a prefix must generate what a plain add of concat(prefix, body) generates:
the oracle's one-prompt generate_batch (or its own generate_blocking call on a FS_SESSION_ROWS session), parting only at a near-tie.
Its KV rows must be the prefix's (shared full pages + the copied tail page), pages must be accounted exactly, and one group pass must
take members that start at different positions.  Full size: an FS_SESSION_ROWS session (greedy against generate_blocking, sampled against
the oracle sampler per admission number) and a 32-slot static-batch session of 32 prefixed joins against the oracle."""
import ctypes as C
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import fishrt
from fishrt import _ffi
from fishrt import config as fcfg
from oracle import oracle as orc

SEED = 0xF15E5EED
NEAR_TIE = 5e-3
MID = dict(fcfg.TINY, dim=256, n_head=4, n_local_heads=2, head_dim=64, intermediate_size=1024)
TOK15 = fcfg.FISH_1_5_TOKENS
IM_END = TOK15["im_end_id"]
N_AUDIO = fcfg.FISH_1_5["vocab_size"] - IM_END


def _prompt(rng, L):
    p = np.zeros((9, L), np.uint32)
    p[0] = rng.randint(0, 400, L)
    k = min(L - 1, 5)
    if k > 0:  # a VQ span so that codebook embeddings take part
        p[0, 1 : 1 + k] = fcfg.TINY_TOKENS["semantic_start_id"] + rng.randint(0, 64, k)
        p[1:, 1 : 1 + k] = rng.randint(0, 64, (8, k))
    return p


def _check_vs_oracle(o, prompt, max_new, got, what, **kw):
    exp = o.generate_batch([prompt], max_new, seed=42, temp=0.0, top_p=1.0, top_k=0, **kw)[0]
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    if np.array_equal(got, exp):
        return 0
    m = o.last_batch_margins
    f = int(np.argmax((got != exp).any(0)))
    mf = float(min(m[f, 0], m[f - 1, 0])) if f > 0 else float(m[f, 0])
    assert mf < NEAR_TIE, f"{what} left the oracle's stream at frame {f} on a margin of {mf:.2e}"
    return 1


def _lm_and_oracle(cfg, dtype, max_batch=4):
    lm = fishrt.DualARTransformer(cfg, fcfg.TINY_TOKENS, 0, dtype, max_batch=max_batch).load_synthetic(SEED)
    o = orc.OracleLM(orc.TINY | {k: cfg[k] for k in ("dim", "n_head", "n_local_heads", "head_dim", "intermediate_size")})
    o.load_synthetic(SEED, bf16=dtype == "bf16", fp8=dtype == "fp8")
    o.set_kv_round_bf16(True)
    return lm, o


def _drain(s, live, results, rng=None):
    """step until every live slot is done; results[tag] = codes"""
    while live:
        s.step(int(rng.randint(1, 9)) if rng is not None else 8)
        for slot in list(live):
            if s.poll(slot, codes=False)[1]:
                results[live.pop(slot)] = s.poll(slot)[0]
                s.release(slot)


@pytest.mark.parametrize("cfg,dtype", [(fcfg.TINY, "bf16"), (MID, "bf16"), (MID, "fp8")], ids=["hd32", "hd64", "hd64-fp8"])
def test_prefixed_slots_equal_one_prompt_static_batches_of_the_concatenation(cfg, dtype):
    lm, o = _lm_and_oracle(cfg, dtype)
    rng = np.random.RandomState(17)
    prefixes = {P: _prompt(rng, P) for P in (64, 37, 100)}  # aligned, and two with a partly filled last page
    # (prefix length or None for a plain add, body length): bodies of 1 column prefill nothing of their own
    reqs = [(37, 12), (None, 30), (100, 1), (64, 9), (37, 1), (100, 25), (None, 7), (64, 40), (37, 20), (100, 6), (64, 1), (37, 33)]
    bodies = [_prompt(rng, Lb) for _, Lb in reqs]
    full = [b if P is None else np.concatenate([prefixes[P], b], 1) for (P, _), b in zip(reqs, bodies)]
    budgets = [f.shape[1] + int(rng.randint(10, 50)) for f in full]
    results = {}
    with lm.session(temp=0.0, top_p=1.0, top_k=0, seed=42, ignore_eos=True) as s:
        ids = {P: s.add_prefix(p) for P, p in prefixes.items()}
        assert all(v is not None for v in ids.values())
        pending, live, steps, released = list(range(len(reqs))), {}, 0, False
        while pending or live:
            while pending:
                i = pending[0]
                P = reqs[i][0]
                if P is not None and ids[P] is None:  # its prefix was released: add it again (release and re-add)
                    ids[P] = s.add_prefix(prefixes[P])
                slot = s.add(bodies[i], budgets[i], prefix=None if P is None else ids[P])
                if slot is None:
                    assert len(live) == 4
                    break
                live[slot] = pending.pop(0)
            s.step(int(rng.randint(1, 9)))
            steps += 1
            if not released and steps == 3:  # the 37 prefix is released while slots still use it
                s.release_prefix(ids[37])
                ids[37], released = None, True
            for slot in list(live):
                if s.poll(slot, codes=False)[1]:
                    results[live.pop(slot)] = s.poll(slot)[0]
                    s.release(slot)
        info = s.info()
        assert info["tail_pages_copied"] > 0 and info["prefix_tokens_reused"] > 0
    flips = 0
    for i, f in enumerate(full):
        assert results[i].shape == (8, 1 + max(0, budgets[i] - f.shape[1] + 1)), i
        flips += _check_vs_oracle(o, f, budgets[i], results[i], f"request {i}", ignore_eos=True)
    print(f"prefixed session: {len(reqs) - flips}/{len(reqs)} requests identical to their one-prompt static batch")
    assert flips <= 3
    lm.clear_slow_layer_caches()
    lm.generate_blocking(full[0], 20)


def test_prefixed_kv_rows_equal_the_plain_slot_of_the_concatenation():
    lm = fishrt.DualARTransformer(MID, fcfg.TINY_TOKENS, 0, "bf16", max_batch=4).load_synthetic(SEED)
    rng = np.random.RandomState(3)
    P = 100
    pre = _prompt(rng, P)
    bodies = [_prompt(rng, 21), _prompt(rng, 14)]
    with lm.session(temp=0.0, top_p=1.0, top_k=0, seed=42, ignore_eos=True) as s:
        pid = s.add_prefix(pre)
        sa = s.add(bodies[0], P + 21 + 30, prefix=pid)
        sb = s.add(bodies[1], P + 14 + 30, prefix=pid)
        sp = s.add(np.concatenate([pre, bodies[0]], 1), P + 21 + 30)
        s.step(1)
        for layer in range(MID["n_layer"]):
            ka, va = lm.debug_read_kv(layer, 0, P + 21 - 1, slot=sa)
            kb, vb = lm.debug_read_kv(layer, 0, P, slot=sb)
            kp, vp = lm.debug_read_kv(layer, 0, P + 21 - 1, slot=sp)
            # rows [0, P): the shared pages and the copied tail are the same bytes in every prefixed slot
            assert np.array_equal(ka[:P], kb) and np.array_equal(va[:P], vb), layer
            for got, ref in ((ka, kp), (va, vp)):
                tol = 2e-4 * float(np.abs(ref).max())
                err = float(np.abs(got - ref).max())
                assert err <= tol, (layer, err, tol)


def test_members_with_different_starts_share_one_group_pass():
    lm, o = _lm_and_oracle(MID, "bf16")
    rng = np.random.RandomState(5)
    prefixes = {P: _prompt(rng, P) for P in (37, 64, 100)}
    members = [(None, 30), (37, 25), (64, 30), (100, 18)]  # starts 0 / 37 / 64 / 100
    bodies = [_prompt(rng, Lb) for _, Lb in members]
    full = [b if P is None else np.concatenate([prefixes[P], b], 1) for (P, _), b in zip(members, bodies)]
    budgets = [f.shape[1] + 20 for f in full]
    results = {}
    with lm.session(temp=0.0, top_p=1.0, top_k=0, seed=42, ignore_eos=True) as s:
        ids = {P: s.add_prefix(p) for P, p in prefixes.items()}
        s.step(1)  # nothing live: the prefixes' own pass runs and is activated
        before = s.info()
        live = {}
        for i, (P, _) in enumerate(members):
            live[s.add(bodies[i], budgets[i], prefix=None if P is None else ids[P])] = i
        s.step(1)
        after = s.info()
        assert after["prefill_passes"] - before["prefill_passes"] == 1, (before, after)
        rows = sum((f.shape[1] - 1) if P is None else (Lb - 1) for (P, Lb), f in zip(members, full))
        assert after["tokens_prefilled"] - before["tokens_prefilled"] == rows
        assert after["prefix_tokens_reused"] - before["prefix_tokens_reused"] == 37 + 64 + 100
        assert after["tail_pages_copied"] - before["tail_pages_copied"] == 2  # 37 and 100; 64 is page-aligned
        _drain(s, live, results)
    flips = sum(_check_vs_oracle(o, f, budgets[i], results[i], f"member {i}", ignore_eos=True) for i, f in enumerate(full))
    assert flips <= 1


def test_one_session_runs_every_kind_of_prefill_pass():
    """The kinds of pass a session's queue is taken apart into (csrc/fs_prefill_plan.h), in ONE per-slot session of a max_batch = 2 handle
    (MID: the TINY handle with head_dim 64 -- the group pass needs the flash kernel): an imported prefix of 65 positions, a created one of
    63, unseeded prefixed adds with bodies of 1 and 7 columns, a seeded plain add of 2 columns.  Of those only ONE member is unseeded
    and has a row to run, so they make an import pass, single passes and a pass without rows; two more unseeded prefixed adds (bodies of
    5 and 3 columns, once the slots are free again) make the group pass.  The four counters after each stage are computed here from the
    rules, and every slot's codes are those of a plain add of the concatenation (parting only at an oracle near-tie)."""
    lm, o = _lm_and_oracle(MID, "bf16", max_batch=2)
    rng = np.random.RandomState(23)
    Pi, Pc = 65, 63
    pre_i, pre_c = _prompt(rng, Pi), _prompt(rng, Pc)
    # (tag, prefix or None, body columns, seed)
    reqs = [("one", "i", 1, None), ("seven", "c", 7, None), ("seeded", None, 2, 1234), ("five", "i", 5, None), ("three", "c", 3, None)]
    pre = {"i": pre_i, "c": pre_c, None: np.zeros((9, 0), np.uint32)}
    bodies = {tag: _prompt(rng, Lb) for tag, _, Lb, _ in reqs}
    full = {tag: np.concatenate([pre[k], bodies[tag]], 1) for tag, k, _, _ in reqs}
    budget = {tag: f.shape[1] + 10 for tag, f in full.items()}
    kw = dict(temp=0.0, top_p=1.0, top_k=0, seed=42, ignore_eos=True, per_slot=True, repetition_penalty=1.0)
    counters = ("prefill_passes", "tokens_prefilled", "prefix_tokens_reused", "tail_pages_copied")
    with lm.session(**kw) as s:
        blob = s.export_prefix(s.add_prefix(pre_i))
    got, plain = {}, {}
    with lm.session(**kw) as s:
        def add(tag):
            _, k, _, seed = next(r for r in reqs if r[0] == tag)
            slot = s.add(bodies[tag], budget[tag], prefix=ids[k] if k else None, seed=seed)
            assert slot is not None, tag
            return slot
        ids = {"i": s.import_prefix(blob), "c": s.add_prefix(pre_c)}
        live = {add("one"): "one", add("seven"): "seven"}
        s.step(1)  # nothing live: the whole queue is taken apart, pass after pass
        # the import (no transformer pass, no counter) | the creation alone, 63 rows | "seven" alone (6 rows from position 63; "one" has
        # no row to run and cannot join) | "one" without a pass.  Both prefixes end inside a page: one tail copy per add.
        info = s.info()
        assert [info[k] for k in counters] == [2, Pc + 6, Pc + Pi, 2], info
        _drain(s, live, got)
        live = {add("seeded"): "seeded"}  # a seed of its own: alone by rule, 1 row
        s.step(1)
        info = s.info()
        assert [info[k] for k in counters] == [3, Pc + 6 + 1, Pc + Pi, 2], info
        _drain(s, live, got)
        live = {add("five"): "five", add("three"): "three"}  # ONE group pass of 2 x 4 rows, starts 65 and 63: 4 + 2 rows are tokens
        s.step(1)
        info = s.info()
        assert [info[k] for k in counters] == [4, Pc + 6 + 1 + 4 + 2, 2 * (Pc + Pi), 4], info
        _drain(s, live, got)
    with lm.session(**kw) as s:  # the plain adds of the concatenations, each in a pass of its own
        for tag, _, _, seed in reqs:
            _drain(s, {s.add(full[tag], budget[tag], seed=seed): tag}, plain)
    flips = 0
    for tag, _, _, _ in reqs:
        assert got[tag].shape == plain[tag].shape == (8, budget[tag] - full[tag].shape[1] + 2), tag
        if not np.array_equal(got[tag], plain[tag]):  # both sides of a parting sit at a near-tie of the oracle's stream
            flips += 1
            _check_vs_oracle(o, full[tag], budget[tag], got[tag], f"{tag}", ignore_eos=True)
            _check_vs_oracle(o, full[tag], budget[tag], plain[tag], f"{tag} (plain)", ignore_eos=True)
    assert flips <= 1


def _pages(n):
    return (n + 63) // 64


def test_page_accounting_is_exact():
    lm = fishrt.DualARTransformer(MID, fcfg.TINY_TOKENS, 0, "bf16", max_batch=4).load_synthetic(SEED)
    rng = np.random.RandomState(9)
    P, Lb = 100, 20
    pre, body = _prompt(rng, P), _prompt(rng, Lb)
    mnt = P + Lb + 40
    n_iter = 1 + max(0, mnt - (P + Lb) + 1)
    private = _pages(P + Lb + n_iter - 1) - P // 64
    with lm.session(temp=0.0, top_p=1.0, top_k=0, seed=42, ignore_eos=True) as s:
        free0 = s.info()["free_pages"]
        for k in (1, 2, 3):
            pid = s.add_prefix(pre)
            slots = [s.add(body, mnt, prefix=pid) for _ in range(k)]
            s.step(1)
            info = s.info()
            assert info["free_pages"] == free0 - _pages(P) - k * private, (k, info)
            assert info["shared_pages"] == P // 64 and info["live_prefixes"] == 1, (k, info)
            for sl in slots:
                s.release(sl)
            s.release_prefix(pid)
            assert s.info()["free_pages"] == free0
        for order in itertools.permutations(["a", "b", "prefix"]):  # every release order returns every page
            pid = s.add_prefix(pre)
            slots = {"a": s.add(body, mnt, prefix=pid), "b": s.add(body, mnt, prefix=pid)}
            s.step(2)
            for what in order:
                if what == "prefix":
                    s.release_prefix(pid)
                else:
                    s.release(slots[what])
            info = s.info()
            assert info["free_pages"] == free0 and info["shared_pages"] == 0 and info["live_prefixes"] == 0, (order, info)
        # session_end with live prefixes (one still being prefilled) and slots on them frees everything
        pid = s.add_prefix(pre)
        s.add(body, mnt, prefix=pid)
        s.step(1)
        s.add_prefix(_prompt(rng, 70))
    with lm.session(temp=0.0, top_p=1.0, top_k=0, seed=42, ignore_eos=True) as s:
        info = s.info()
        assert info["free_pages"] == free0 and info["shared_pages"] == 0 and info["live_prefixes"] == 0, info


def test_error_contract():
    lm = fishrt.DualARTransformer(MID, fcfg.TINY_TOKENS, 0, "bf16", max_batch=2).load_synthetic(SEED)
    rng = np.random.RandomState(1)
    msl = MID["max_seq_len"]
    L = _ffi.lib()
    u32p = C.POINTER(C.c_uint32)
    pre, body = _prompt(rng, 40), _prompt(rng, 8)
    out = C.c_int(-7)
    with pytest.raises(RuntimeError):  # no session
        _ffi.check(L.fs_lm_session_prefix_create(lm._h, pre.ctypes.data_as(u32p), 40, C.byref(out)))
    with pytest.raises(RuntimeError):
        _ffi.check(L.fs_lm_session_add_prefixed(lm._h, 0, body.ctypes.data_as(u32p), 8, 50, C.byref(out)))
    with pytest.raises(RuntimeError):
        _ffi.check(L.fs_lm_session_prefix_release(lm._h, 0))
    with lm.session(temp=0.0, top_p=1.0, top_k=0, seed=42, ignore_eos=True) as s:
        pid = s.add_prefix(pre)
        with pytest.raises(RuntimeError):  # unknown id
            s.add(body, 50, prefix=pid + 5)
        with pytest.raises(RuntimeError):
            s.release_prefix(-1)
        with pytest.raises(RuntimeError):  # L_body = 0
            _ffi.check(L.fs_lm_session_add_prefixed(lm._h, pid, body.ctypes.data_as(u32p), 0, 50, C.byref(out)))
        with pytest.raises(RuntimeError):  # P + L_body > max_seq_len
            s.add(_prompt(rng, msl - 40 + 1), msl + 10, prefix=pid)
        s.release_prefix(pid)
        with pytest.raises(RuntimeError):  # released id
            s.add(body, 50, prefix=pid)
        with pytest.raises(RuntimeError):
            s.release_prefix(pid)
        # a pool too small for a prefix: -1 (None), not an error
        big = _prompt(rng, msl - 1)
        ids, none_seen = [], False
        for _ in range(4):
            r = s.add_prefix(big)
            if r is None:
                none_seen = True
                break
            ids.append(r)
        assert none_seen and ids
        free = s.info()["free_pages"]
        assert free < _pages(msl - 1)
        s.step(1)
    # the handle works normally after the session
    p = _prompt(rng, 12)
    a = lm.generate_blocking(p, 20, temp=0.0, top_p=1.0, top_k=0, ignore_eos=True)
    lm.clear_slow_layer_caches()
    b = lm.generate_blocking(p, 20, temp=0.0, top_p=1.0, top_k=0, ignore_eos=True)
    assert np.array_equal(a, b)


def _prompt15(L, seed):
    p = np.zeros((9, L), np.uint32)
    p[0] = np.random.RandomState(seed).randint(0, IM_END, L)
    return p


def _referee(lm, p, mnt, a, b, rp, ignore_eos=True):
    """a = the session's codes, b = the batch-1 path's: where they part, the batch-1 path's recorded logits of that decision must hold
    the two choices within NEAR_TIE of each other (a codebook decision, or the slow-token decision of that frame or the one before)"""
    n = min(a.shape[1], b.shape[1])
    neq = (a[:, :n] != b[:, :n]).any(0)
    f = int(np.argmax(neq)) if neq.any() else n
    lm.debug_capture(f + 1)
    try:
        lm.clear_slow_layer_caches()
        again = lm.generate_blocking(p, mnt, temp=0.0, top_p=1.0, top_k=0, repetition_penalty=rp, ignore_eos=ignore_eos)
        cap = lm.debug_read(f + 1)
    finally:
        lm.debug_capture(0)
    assert np.array_equal(again, b), "the batch-1 path is not deterministic"
    if not neq.any():
        assert not ignore_eos and a.shape[1] != b.shape[1]
        sl = cap[f, 0, :N_AUDIO]
        gap, c = float(abs(sl[0] - sl[1:].max())), -1
    else:
        c = int(np.argmax(a[:, f] != b[:, f]))
        if a.shape[1] > f and b.shape[1] > f and not (a[:, f].any() and b[:, f].any()):
            sl = cap[f, 0, :N_AUDIO]
            gap, c = float(abs(sl[0] - sl[1:].max())), -1
        else:
            lg = cap[f, 1 + c, :1024]
            gap = float(abs(lg[a[c, f]] - lg[b[c, f]]))
            if gap >= NEAR_TIE:
                for g in (f, f - 1):
                    if g >= 0:
                        sl = np.sort(cap[g, 0, :N_AUDIO][np.isfinite(cap[g, 0, :N_AUDIO])])
                        if float(sl[-1] - sl[-2]) < gap:
                            gap, c = float(sl[-1] - sl[-2]), -2
    assert gap < NEAR_TIE, (f, c, gap)
    return f, c, gap


def test_fullsize_rows_session_prefixed_requests_are_their_own_generate_call():
    """Fish-1.5 shapes, bf16, FS_SESSION_ROWS, greedy, repetition penalty 1.2: 10 requests through 4 slots over 2 prefixes of ~340
    positions; each request == generate_blocking(concat(prefix, body)) on the same handle, or parts at a refereed near-tie"""
    rp = 1.2
    lm = fishrt.DualARTransformer(fcfg.FISH_1_5, TOK15, 0, "bf16", max_batch=4).load_synthetic(SEED)
    rng = np.random.RandomState(21)
    prefixes = [_prompt15(340, 900), _prompt15(333, 901)]
    reqs = [(i % 2, int(rng.randint(24, 49))) for i in range(10)]
    bodies = [_prompt15(Lb, 910 + i) for i, (_, Lb) in enumerate(reqs)]
    frames = [int(v) for v in rng.randint(6, 30, 10)]
    full = [np.concatenate([prefixes[k], b], 1) for (k, _), b in zip(reqs, bodies)]
    budgets = [f.shape[1] + F - 2 for f, F in zip(full, frames)]
    results, pending, live = {}, list(range(10)), {}
    with lm.session(temp=0.0, top_p=1.0, top_k=0, seed=5, ignore_eos=True, rows=True, repetition_penalty=rp) as s:
        ids = [s.add_prefix(p) for p in prefixes]
        steps = 0
        while pending or live:
            while pending:
                i = pending[0]
                slot = s.add(bodies[i], budgets[i], prefix=ids[reqs[i][0]])
                if slot is None:
                    assert len(live) == 4
                    break
                live[slot] = pending.pop(0)
            s.step(int(rng.randint(1, 9)))
            steps += 1
            for slot in list(live):
                if s.poll(slot, codes=False)[1]:
                    results[live.pop(slot)] = s.poll(slot)[0]
                    s.release(slot)
        info = s.info()
        assert info["prefix_tokens_reused"] == sum(prefixes[k].shape[1] for k, _ in reqs)
    parted = 0
    for i in range(10):
        lm.clear_slow_layer_caches()
        ref = lm.generate_blocking(full[i], budgets[i], temp=0.0, top_p=1.0, top_k=0, repetition_penalty=rp, ignore_eos=True)
        assert results[i].shape == ref.shape == (8, frames[i]), (i, results[i].shape, ref.shape)
        if not np.array_equal(results[i], ref):
            parted += 1
            _referee(lm, full[i], budgets[i], results[i], ref, rp)
    print(f"prefixed rows session: {10 - parted} of 10 requests identical to their own generate call")
    assert parted <= 5
    lm.close()


def _oracle_picks(cap, seed, temp, top_p, top_k):
    L = orc.lib()
    s = L.orc_sampler_create(C.c_uint64(seed), C.c_double(temp), C.c_double(top_p), C.c_uint64(top_k))
    picks = np.zeros((cap.shape[0], 9), np.int64)
    try:
        for f in range(cap.shape[0]):
            for r in range(9):
                n = N_AUDIO if r == 0 else 1024
                row = np.ascontiguousarray(cap[f, r, :n])
                picks[f, r] = L.orc_sampler_sample(C.c_void_p(s), row.ctypes.data_as(C.POINTER(C.c_float)), C.c_uint64(n))
    finally:
        L.orc_sampler_destroy(C.c_void_p(s))
    return picks


def test_fullsize_rows_session_sampled_prefixed_slots_every_decision():
    """sampled FS_SESSION_ROWS slots on prefixes: the k-th ADMISSION (plain or prefixed; creating a prefix is no admission) draws from
    StdRng(seed + k), and every captured decision == the oracle sampler on the captured logits"""
    F, rp, seed = 24, 1.2, 77
    kw = dict(temp=0.7, top_p=0.8, top_k=256)
    lm = fishrt.DualARTransformer(fcfg.FISH_1_5, TOK15, 0, "bf16", max_batch=4).load_synthetic(SEED)
    lm.debug_capture(F)
    prefixes = [_prompt15(340, 920), _prompt15(333, 921)]
    outs, order = {}, []
    with lm.session(seed=seed, ignore_eos=True, rows=True, repetition_penalty=rp, **kw) as s:
        pa = s.add_prefix(prefixes[0])
        order.append(s.add(_prompt15(30, 930), 30 + F - 2))                    # admission 0: plain
        pb = s.add_prefix(prefixes[1])                                          # (no admission number)
        s.step(3)
        order.append(s.add(_prompt15(25, 931), 340 + 25 + F - 2, prefix=pa))   # admission 1
        s.step(3)
        order.append(s.add(_prompt15(41, 932), 333 + 41 + F - 2, prefix=pb))   # admission 2
        s.step(2)
        order.append(s.add(_prompt15(1, 933), 340 + 1 + F - 2, prefix=pa))     # admission 3: a body of one column
        while s.step(8):
            pass
        for k, sl in enumerate(order):
            outs[k] = s.poll(sl)[0]
    for k, sl in enumerate(order):
        cap = lm.debug_read_row(sl, F)
        assert outs[k].shape == (8, F)
        picks = np.concatenate([cap[:, :1, 2047], cap[:, 1:, 1024]], axis=1).astype(np.int64)
        assert np.array_equal(picks[:, 1:].T, outs[k].astype(np.int64))
        exp = _oracle_picks(cap, seed + k, kw["temp"], kw["top_p"], kw["top_k"])
        bad = np.argwhere(picks != exp)
        assert bad.size == 0, f"admission {k} (slot {sl}): {len(bad)} of {F * 9} decisions differ from the oracle sampler, first {bad[0]}"
    lm.debug_capture(0)
    lm.close()


def test_fullsize_static_batch_session_32_prefixed_joins_vs_oracle():
    """Fish-1.5 shapes, bf16, a max_batch = 32 static-batch session: 32 requests on one 340-position prefix (bodies U{24..48}) are
    admitted in ONE group pass whose members start at position 340; rows of a subset == the oracle's one-prompt generate_static_batch of
    concat(prefix, body), except at oracle near-ties"""
    lm = fishrt.DualARTransformer(fcfg.FISH_1_5, TOK15, 0, "bf16", max_batch=32).load_synthetic(SEED)
    rng = np.random.RandomState(31)
    sem0 = TOK15["semantic_start_id"]
    pre = _prompt15(340, 940)
    pre[0, 300:330] = sem0 + rng.randint(0, 1024, 30)  # a VQ span in the prefix, as a voice prompt has
    pre[1:, 300:330] = rng.randint(0, 1024, (8, 30))
    bodies = [_prompt15(int(rng.randint(24, 49)), 950 + i) for i in range(32)]
    frames = 8
    budgets = [340 + b.shape[1] + frames - 2 for b in bodies]
    got = {}
    with lm.session(temp=0.0, top_p=1.0, top_k=0, ignore_eos=True) as s:
        pid = s.add_prefix(pre)
        s.step(1)  # the prefix's own pass
        before = s.info()
        live = {s.add(b, budgets[i], prefix=pid): i for i, b in enumerate(bodies)}
        assert len(live) == 32
        s.step(1)
        after = s.info()
        assert after["prefill_passes"] - before["prefill_passes"] == 1, (before, after)
        assert after["tail_pages_copied"] - before["tail_pages_copied"] == 32
        assert after["shared_pages"] == 340 // 64
        _drain(s, live, got)
    o = orc.OracleLM(orc.FISH15).load_synthetic(SEED, bf16=True)
    o.set_kv_round_bf16(True)
    flips = 0
    rows = (0, 6, 13, 19, 25, 31)
    for i in rows:
        assert got[i].shape == (8, frames), (i, got[i].shape)
        flips += _check_vs_oracle(o, np.concatenate([pre, bodies[i]], 1), budgets[i], got[i], f"join {i}", ignore_eos=True)
    # (every parting is asserted to sit at an oracle near-tie above; the synthetic weights' flat 1024-way codebook logits make those
    # common at full size -- test_session_gpu.py's full-size session allows 2 of 5)
    print(f"32 prefixed joins: {len(rows) - flips}/{len(rows)} checked rows identical to the oracle's one-prompt static batch")
    assert flips <= len(rows) // 2
    lm.close()
