"""CPU: the float64 attention definitions of tests/attn_refs.py are pinned against torch's scaled_dot_product_attention in float64; splitting
at arbitrary chunks and merging equals the whole; every case of test_attn_paths_gpu.py is planned (fs_selftest_attn, plan_only: no device) and
its plan name compared with the case table; the hook refuses bad cases by validation alone; and the cases have TEETH without a GPU: for every
planted case, the reference mutated in each way a kernel goes wrong (one token dropped, the first stale row read, the neighbouring kv head,
the row's last 16-token wave tile counted twice; for the prefill rows the first two are the causal offset -1 / +1) moves at least one element by >= 10 x that
element's tolerance."""
import functools

import numpy as np
import pytest
import torch

import attn_refs as R
from attn_refs import F32, F64

MUTATIONS = ("drop", "extra", "g+1", "g-1", "dup")


@functools.lru_cache(maxsize=None)
def cases():
    return {c.id: c for c in R.all_cases()}


def test_case_ids_are_unique():
    ids = [c.id for c in R.all_cases()]
    assert len(ids) == len(set(ids))


def test_bf16_rne_is_torch_bfloat16():
    rng = np.random.RandomState(1)
    x = np.concatenate([rng.randn(4096).astype(F32) * 10.0 ** rng.randint(-20, 20, 4096), np.float32([0, -0.0, 1, 1.00390625, 1.01171875, 2.0 ** 100,
                        -2.0 ** 100, 3.3895314e38])]).astype(F32)
    ref = torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()
    assert np.array_equal(R.bf16_rne(x).view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(R.bf16_rne(np.float32([1.00390625, 1.01171875])), np.float32([1.0, 1.015625]))  # ties go to even


def _torch_sdpa(case, m_rows):
    """rows m_rows of one sequence against torch in float64: GQA by repeat_interleave, a boolean mask for the rows' lengths"""
    s = case.rows[m_rows[0]][0]
    L = max(case.rows[m][1] for m in m_rows)
    k = np.stack([R.gather(case.k_ref, case.table[s], L, g) for g in range(case.Hk)]).astype(F64)
    v = np.stack([R.gather(case.v_ref, case.table[s], L, g) for g in range(case.Hk)]).astype(F64)
    kt = torch.from_numpy(k).repeat_interleave(case.n_rep, 0)
    vt = torch.from_numpy(v).repeat_interleave(case.n_rep, 0)
    q = torch.from_numpy(np.stack([case.q_ref[m] for m in m_rows], 1))  # [H][rows][Dh]
    mask = torch.tensor([[t < case.rows[m][1] for t in range(L)] for m in m_rows])
    return torch.nn.functional.scaled_dot_product_attention(q, kt, vt, attn_mask=mask).numpy().transpose(1, 0, 2)


@pytest.mark.parametrize("cid", ["decode-FISH-bf16-T129-planted", "decode-TINY-f32-T65-planted", "prefill-MID-pos5-M65", "prefill-group-MID",
                                 "rows-MID-M4-random", "rows-FISH-M4-step0", "tbl-FISH-pos0-7", "chunked-TINY-M129", "small-TINY-ident0"])
def test_reference_is_torch_sdpa(cid):
    case = cases()[cid]
    o, tol, _ = case.reference()
    by_seq = {}
    for m, (s, _) in enumerate(case.rows):
        by_seq.setdefault(s, []).append(m)
    for s, ms in by_seq.items():
        t = _torch_sdpa(case, ms)
        assert np.abs(t - o[ms]).max() <= 1e-12 * max(1.0, np.abs(o[ms]).max()), cid
    assert (tol >= 0).all() and np.isfinite(tol).all()  # (0 only where the output is an exact 0: one token whose v is 0)


def test_causal_offsets_of_the_prefill_layout():
    case = cases()["prefill-MID-pos130-M65"]
    assert case.rows[0] == (0, 131) and case.rows[64] == (0, 195) and case.M == 65
    g = cases()["prefill-group-MID"]
    assert [g.rows[i] for i in (0, 16, 17, 50)] == [(0, 1), (0, 17), (1, 71), (2, 147)]


@pytest.mark.parametrize("seed", range(4))
def test_split_at_arbitrary_chunks_then_merge_equals_the_whole(seed):
    rng = np.random.RandomState(seed)
    T, Dh = int(rng.randint(2, 700)), (32, 64)[seed % 2]
    q, k, v = rng.randn(Dh) * 3, rng.randn(T, Dh), rng.randn(T, Dh)
    k[rng.randint(0, T)] *= 8  # one dominant token: the partial maxima differ by tens
    whole, _, _ = R.attend(q, k, v)
    cuts = [0] + sorted(set(int(c) for c in rng.randint(1, T, int(rng.randint(1, 9))))) + [T]
    parts = [R.partial(q, k[a:b], v[a:b]) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
    assert np.abs(R.merge(parts) - whole).max() <= 1e-13 * max(1.0, np.abs(whole).max())
    one = R.partial(q, k, v)
    assert np.allclose(R.merge([one]), whole, rtol=1e-15, atol=0)


def test_rope_i_rotates_interleaved_pairs():
    x = np.arange(8.0)
    c, s = np.array([1.0, 0.0, 0.5, -1.0]), np.array([0.0, 1.0, 0.5, 0.0])
    assert np.array_equal(R.rope_i(x, c, s), [0, 1, -3, 2, 4 * .5 - 5 * .5, 4 * .5 + 5 * .5, -6, -7])


# ---------------------------------------------------------------------------------------------------------------------- plans, without a device
def test_plan_names_of_every_gpu_case():
    seen = set()
    for c in cases().values():
        name = c.plan_name()
        assert name == c.expect, (c.id, name, c.expect)
        seen.add(name.split("+")[0])
    assert seen == set(R.PLAN_TABLE), seen ^ set(R.PLAN_TABLE)


def test_hsplit_bounds_are_the_launchers():
    """the M at which k_attn_rows changes its head split, read off the launcher's own ternary: Hk * M <= 64 -> 4, < 256 -> 2, else 1 (Hk = 2)"""
    def name(M):
        return R.Case(f"hs-{M}", "rows", "bf16", "FISH", "random", "", [1] * M, pos_step=0).plan_name()
    assert name(32).startswith("rows/bf16/64/2/hs4") and name(33).startswith("rows/bf16/64/4/hs2")
    assert name(127).startswith("rows/bf16/64/4/hs2") and name(128) == "rows/bf16/64/8"


def test_rejected_cases_are_validation_errors():
    """refused on the host, with or without a device: the message is the validation's, never a launch's or 'no HIP device'"""
    for label, c, text in R.rejected_cases():
        rc, msg = R.call_rejected(c)
        assert rc != 0, label
        assert text in msg and "no HIP device" not in msg and "hip" not in msg.split(":")[0].lower(), (label, msg)


# ---------------------------------------------------------------------------------------------------------------------- teeth
def _moved(base, tol, mut):
    both = ~np.isnan(base) & ~np.isnan(mut)
    ratio = np.zeros(base.shape)
    d = np.abs(mut[both] - base[both])
    ratio[both] = np.where(d > 0, d / np.maximum(tol[both], 1e-300), 0.0)
    ratio[np.isnan(base) != np.isnan(mut)] = np.inf
    ratio[~np.isfinite(mut) & ~np.isnan(mut)] = np.inf
    return ratio.max()


def _planted():
    return [c for c in cases().values() if c.tier == "planted"]


def test_planted_tokens_carry_the_weight():
    for c in _planted():
        _, _, w = c.reference()
        assert w.min() >= 0.99, (c.id, float(w.min()))
        ts = set(int(t) for t in c.tstar.reshape(-1))
        if c.kind in ("decode", "decode_wo"):
            assert {0, c.Ts[0] - 1} <= ts, (c.id, ts)


def test_every_mutation_moves_every_planted_case():
    worst = {}
    for c in _planted():
        if c.kind == "decode":
            base, tol = c.reference_partials(_tpb(c))
            ref = lambda mut: c.reference_partials(_tpb(c), mut)[0]
        elif c.kind in ("decode_wo", "fused"):
            base, tol = c.reference_x()
            ref = lambda mut: c.reference_x(mut)[0]
        else:
            base, tol, _ = c.reference()
            ref = lambda mut: c.reference(mut)[0]
        for mut in MUTATIONS:
            if mut == "dup" and c.kind != "decode" and max(T for _, T in c.rows) <= 16:
                continue  # all of a row's tokens twice is the same normalised output: not a mutation there
            if mut == "drop" and c.kind != "decode" and max(T for _, T in c.rows) == 1:
                continue  # no token left: not an attention
            with np.errstate(all="ignore"):
                r = _moved(base, tol, ref(mut))
            assert r >= 10.0, (c.id, mut, r)
            worst[mut] = min(worst.get(mut, np.inf), r)
    print("weakest planted case per mutation, |moved| / tol:", {k: f"{v:.3g}" for k, v in worst.items()})


def _tpb(c):
    return int(c.expect.split("tpb")[1]) if "tpb" in c.expect else 1
