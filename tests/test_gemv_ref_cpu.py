"""CPU: the float64 definitions of tests/gemv_refs.py are pinned against torch in float64 and bfloat16 (RMSNorm + GEMV, the interleaved RoPE,
SwiGLU, the one rounding of the cache rows, the embedding sum); the Tier A exactness arithmetic holds for every Tier A case; every case of
test_gemv_paths_gpu.py is planned (fs_selftest_gemv, plan_only: no device) and its plan name and grid compared with the case table -- the
launchers' dispatch written out in gemv_refs.Case.expect; the hook refuses bad cases by validation alone; and the cases have TEETH without a
GPU: the reference mutated in each way these kernels go wrong (gemv_refs.MUTATIONS) moves every applicable Tier A case by at least one grid
step and every applicable Tier B case by >= 10 x the moved element's own tolerance.  What a mutation is waived for is recomputed here and must
equal the written-out table gemv_refs.WAIVED."""
import numpy as np
import pytest
import torch

import gemv_refs as R
from gemv_refs import F32, F64

CASES = {c.id: c for c in R.all_cases()}


def test_case_ids_are_unique_and_cover_the_shapes():
    assert len(CASES) == len(R.all_cases())
    by = lambda op: [c for c in R.all_cases() if c.op == op]
    for op, widths in (("qkv", (128, 256, 1024, 4096)), ("up", (128, 256, 1024, 4096)), ("down", (128, 256, 1024, 4096)),
                       ("head", (128, 256, 1024, 4096)), ("wo", (128, 256, 1024))):
        for wt in R.WTS:
            for K in widths:
                tiers = {c.tier for c in by(op) if c.wt == wt and c.K == K}
                assert tiers == {"A", "B"} or (op == "qkv" and K == 4096 and tiers), (op, wt, K, tiers)
        if op in R.FLAG_OPS:
            assert {c.resident for c in by(op)} == {False, True}
    assert {c.rows for c in by("up")} == {6, 130} and {c.rows for c in by("head")} == {1, 5, 2037}
    assert any(c.K == 128 and c.fp8 for c in by("down"))   # K / KS = 32 with fp8: two lanes hold data
    q = by("qkv")
    assert {c.pos for c in q} == set(R.POSITIONS) and {c.rope_off for c in q} == {0, 7} and {c.use_state for c in q} == {False, True}
    assert {c.geom for c in q} >= {"TINY", "MID", "FISH"}
    assert {c.xs for c in R.all_cases() if c.tier == "B" and c.op in R.NORM_OPS} == {0.0, 1e-3, 1.0, 30.0}
    assert max(c.n_weights for c in R.all_cases() if c.op not in ("embed", "fast_embed") and c.geom != "BIG") < 8.5e6
    e = by("embed")
    assert {(c.kw["source"], c.kw["t0"]) for c in e} >= {(s, t) for s in ("prompt", "cur") for t in (9, 10, 30, 31)}
    assert all(c.build().step > 0 and c.prompt_L > 1 for c in e if c.kw["source"] == "prompt")


# ---------------------------------------------------------------------------------------------------------------------- the definitions
def _torch_gemv(case):
    x, g = torch.from_numpy(case.x).double(), None
    if case.op in R.NORM_OPS:
        g = torch.from_numpy(case.g).double()
        x = x * torch.rsqrt((x * x).mean() + case.eps) * g
    y = torch.from_numpy(case.w).double() @ x
    if case.fp8:
        y = y * torch.from_numpy(case.wscale).double()
    return y


def _close(a, b, rel=1e-12):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    return (np.abs(a - b) <= rel * (np.abs(a) + np.abs(b)) + 1e-300).all()


@pytest.mark.parametrize("cid", ["head-K128-f32-n1-A", "head-K1024-bf16-n2037-tail-B", "down-K128-fp8-dim5-nt-A", "wo-MID-fp8-nt-B",
                                 "up-K256-bf16-inter130-nt-B", "qkv-TINY-bf16-pos200-ro7-state-res-B", "qkv-FISH-f32-pos63-ro0-static-nt-B"])
def test_definitions_against_torch(cid):
    case = CASES[cid].build()
    ref = R.reference(case)
    y = _torch_gemv(case)
    if case.op == "head":
        assert _close(ref["Y"][0], y.numpy())
    elif case.op in ("down", "wo"):
        assert _close(ref["Y"][0], (torch.from_numpy(case.y0).double() + y).numpy())
    elif case.op == "up":
        assert _close(ref["Y"][0], (torch.nn.functional.silu(y[0::2]) * y[1::2]).numpy(), 1e-9)
    else:
        H, Hk, Dh, half = case.H, case.Hk, case.Dh, case.Dh // 2
        row = case.pos + case.rope_off
        cs, sn = torch.from_numpy(case.cos_t).double()[row], torch.from_numpy(case.sin_t).double()[row]
        qk = y[:(H + Hk) * Dh].reshape(H + Hk, half, 2)
        rot = torch.stack([qk[..., 0] * cs - qk[..., 1] * sn, qk[..., 0] * sn + qk[..., 1] * cs], -1).reshape(H + Hk, Dh)
        assert _close(ref["Y"][0], rot[:H].reshape(-1).numpy())
        page, slot = int(case.table[case.pos >> 6]), case.pos & 63
        assert page != case.pos >> 6
        for name, val in (("K", rot[H:]), ("V", y[(H + Hk) * Dh:].reshape(Hk, Dh))):
            pool = ref[name][0]
            base = getattr(case, name.lower() + "0").astype(F64)
            addr = ((page * Hk + np.arange(Hk)[:, None]) * 64 + slot) * Dh + np.arange(Dh)[None, :]   # the store address of the issue
            assert _close(pool.reshape(-1)[addr], val.numpy())
            rest = np.ones(pool.size, bool)
            rest[addr.reshape(-1)] = False
            assert np.array_equal(pool.reshape(-1)[rest], base.reshape(-1)[rest]) and rest.sum() == pool.size - Hk * Dh


def test_cache_rows_are_rounded_once_like_torch_bfloat16():
    x = np.random.RandomState(3).randn(4096) * 10.0 ** np.random.RandomState(4).randint(-10, 10, 4096)
    t = torch.from_numpy(x).float().to(torch.bfloat16).double().numpy()
    assert np.array_equal(R.kv_round(x, "bf16"), t) and np.array_equal(R.kv_round(x, "fp8"), t)
    assert np.array_equal(R.kv_round(x, "f32"), x.astype(F32).astype(F64))
    case = CASES["qkv-MID-bf16-pos0-ro0-static-nt-A"] if "qkv-MID-bf16-pos0-ro0-static-nt-A" in CASES else next(
        c for c in R.all_cases() if c.op == "qkv" and c.tier == "A" and c.wt != "f32")
    ref = R.reference(case.build())
    for name in ("K", "V"):
        p = ref[name][0]
        assert np.array_equal(torch.from_numpy(p).float().to(torch.bfloat16).double().numpy(), p)


@pytest.mark.parametrize("cid", [c.id for c in R.all_cases() if c.op in ("embed", "fast_embed")])
def test_embed_definition_against_torch(cid):
    case = CASES[cid].build()
    y = R.reference(case)["Y"][0]
    dt = torch.float32 if case.kvt == "f32" else torch.bfloat16
    tok = torch.from_numpy(case.tok).to(dt)
    assert torch.equal(tok.float(), torch.from_numpy(case.tok))   # the tables are values of their type
    if case.op == "fast_embed":
        assert np.array_equal(y, tok.float()[torch.from_numpy(case.ids.astype(np.int64))].double().numpy())
        return
    cb = torch.from_numpy(case.cb).to(dt).float()
    col = case.tokens.reshape(case.n_cb + 1, -1)[:, case.step] if case.prompt else case.tokens
    t0 = int(col[0])
    acc = torch.zeros(case.dim) + tok.float()[t0]
    if case.sem_lo <= t0 <= case.sem_hi:
        for c in range(case.n_cb):
            acc = acc + cb[c * case.cb_size + int(col[c + 1])]   # f32 additions, in order
    assert np.array_equal(y, acc.double().numpy())
    assert (case.kw["t0"] in (10, 30)) == bool(case.sem_lo <= t0 <= case.sem_hi)


def test_tier_b_bound_constants():
    assert R.U == 2.0 ** -23 and R.SILU_C_BOUND == 4.0 * 1.588   # the row path's allowance, not a new one
    assert R.nx_of(128, "fp8") == 16 and R.nx_of(4096, "f32") == 64 and R.nx_of(1024, "bf16") == 16
    assert R.c_ops("head", 128, "fp8") == 8 + 9 and R.c_ops("wo", 1024, "bf16") == 8 and R.c_ops("down", 4096, "f32") == 12
    up = CASES["up-K1024-bf16-inter130-nt-B"] if "up-K1024-bf16-inter130-nt-B" in CASES else next(
        c for c in R.all_cases() if c.op == "up" and c.tier == "B" and c.rows == 130 and c.xs > 0)
    a, _ = R.reference(up.build())["_ab"]
    assert abs(a[1] - 90) < 9 and abs(a[2] + 90) < 9 and abs(a[3] + 87.3) < 9   # rows with a near +-90
    for c in R.all_cases():
        if c.tier == "B" and c.fp8 and c.op not in ("embed", "fast_embed"):
            c.build()
            if c.n_weights <= (1 << 20):
                assert np.isin(c.w.astype(F64), R.e4m3_values()).all(), c.id   # W in the weight type
            e = np.log2(c.wscale.astype(F64))
            assert (np.abs(e - np.round(e)) > 1e-6).mean() > 0.9 and (c.op == "up" or c.w_rows < 2 or (e.min() < -5.4 and e.max() > 2.5)), c.id


@pytest.mark.parametrize("case", [c for c in R.all_cases() if c.tier == "A"], ids=repr)
def test_tier_a_arithmetic_is_exact(case):
    R.check_tier_a(case)


# ---------------------------------------------------------------------------------------------------------------------- plans, without a device
def test_plan_names_and_grids_of_every_gpu_case():
    seen = set()
    for c in R.all_cases():
        name, grid, _ = c.plan()
        want, wgrid = c.expect
        assert name == want and grid == wgrid, (c.id, name, grid, want, wgrid)
        seen.add(name)
    for op, widths in (("qkv", (128, 256, 1024, 4096)), ("up", (128, 256, 1024, 4096)), ("head", (128, 256, 1024, 4096)),
                       ("down", (128, 256, 1024, 4096))):
        for wt in R.WTS:
            for K in widths:
                assert any(n.startswith(f"{op}/{wt}/K{K}/") for n in seen), (op, wt, K)
    assert {"qkv/bf16/K1024/w2/nt", "qkv/bf16/K1024/w2/res"} & seen and "head/f32/K128/w4" in seen
    print(f"{len(seen)} plan names over {len(R.all_cases())} cases")


def test_rejected_cases_are_validation_errors():
    """refused on the host, with or without a device: the message is the validation's, never a launch's or 'no HIP device'"""
    for label, c, over, text in R.rejected_cases():
        rc, msg = R.call_rejected(c, over)
        assert rc != 0, label
        assert text in msg and "no HIP device" not in msg and "hip" not in msg.split(":")[0].lower(), (label, msg)


# ---------------------------------------------------------------------------------------------------------------------- teeth
def _moved(base, mutd):
    """how far the mutation moves the reference: max over outputs and elements of |moved| / (10 tol) where the element has a tolerance, of
    |moved| / one grid step where it is exact; a NaN pattern change counts as infinite"""
    worst = 0.0
    for name, (ref, tol) in base.items():
        if name.startswith("_"):
            continue
        mut = mutd[name][0]
        if (np.isnan(ref) != np.isnan(mut)).any():
            return np.inf
        d = np.abs(np.nan_to_num(mut) - np.nan_to_num(ref))
        unit = np.where(tol > 0, 10.0 * tol, R.GRID_A)
        worst = max(worst, float((d / unit).max()))
    return worst


def test_every_mutation_moves_every_applicable_case():
    caught, weakest, waived = {}, {}, {}
    for c in R.all_cases():
        base = None
        for mut, ops in R.MUTATIONS.items():
            if c.op not in ops:
                continue
            why = R.waived(c, mut)
            if why is not None:
                waived[(mut, why)] = waived.get((mut, why), 0) + 1
                continue
            if base is None:
                base = R.reference(c)
            with np.errstate(all="ignore"):
                r = _moved(base, R.reference(c, mut))
            assert r >= 1.0, (c.id, mut, r)
            caught[(mut, c.tier)] = caught.get((mut, c.tier), 0) + 1
            weakest[mut] = min(weakest.get(mut, np.inf), r)
    for mut in R.MUTATIONS:
        assert caught.get((mut, "A"), 0) >= 1, f"no Tier A case for {mut}"
        if not mut.startswith("embed"):
            assert caught.get((mut, "B"), 0) >= 1, f"no Tier B case for {mut}"
    print("cases caught per (mutation, tier):", caught)
    print("weakest |moved| / (10 tol or one grid step):", {k: f"{v:.3g}" for k, v in weakest.items()})
    print("waived:", waived)
    assert waived == R.WAIVED, (waived, R.WAIVED)   # the cap: nothing is waived beyond the written-out table
