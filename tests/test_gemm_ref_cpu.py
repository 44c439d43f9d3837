"""CPU: the number formats of tests/gemm_refs.py are pinned against torch (bf16 RNE, the e4m3fn value set) and the fragment layout's mirror
round-trips; the Tier A exactness arithmetic holds for every Tier A case; every case of test_gemm_paths_gpu.py is planned (fs_selftest_gemm,
plan_only: no device), its plan name and grid compared with the case table, and the table of listed variants -- the dispatch written out
branch for branch -- equals the set of names the cases reach; the hook refuses bad cases by validation alone; and the cases have TEETH
without a GPU: the reference mutated in each way these kernels go wrong (gemm_refs.MUTATIONS) moves every applicable Tier A case by at least
one grid step, and every applicable Tier B case by >= 10 x the moved element's own tolerance (the two lo-plane mutations: Tier B at depth
128 only)."""
import numpy as np
import pytest
import torch

import gemm_refs as R
from gemm_refs import F32, F64

CASES = {c.id: c for c in R.all_cases()}
SMALL = [c for c in R.all_cases() if c.op == "prep" or c.M * c.N * c.K <= (1 << 23)]  # the references the CPU tests compute


def test_case_ids_are_unique():
    assert len(CASES) == len(R.all_cases())


def test_bf16_rne_and_split_are_torch_bfloat16():
    rng = np.random.RandomState(1)
    x = np.concatenate([rng.randn(4096).astype(F32) * 10.0 ** rng.randint(-20, 20, 4096),
                        np.float32([0, -0.0, 1, 1.00390625, 1.01171875, 2.0 ** 100, -2.0 ** 100])]).astype(F32)
    t = torch.from_numpy(x)
    hi_t = t.to(torch.bfloat16).to(torch.float32)
    lo_t = (t - hi_t).to(torch.bfloat16).to(torch.float32)
    hi, lo = R.split(x)
    assert np.array_equal(hi.view(np.uint32), hi_t.numpy().view(np.uint32)) and np.array_equal(lo.view(np.uint32), lo_t.numpy().view(np.uint32))
    assert np.array_equal(R.bf16_rne(np.float32([1.00390625, 1.01171875])), np.float32([1.0, 1.015625]))  # ties go to even
    ok = np.abs(x) < 1e30
    assert (np.abs(hi.astype(F64) + lo.astype(F64) - x)[ok] <= 2.0 ** -17 * np.abs(x[ok])).all()  # the file header's claim about the split


def test_e4m3_value_set_is_torch_float8_e4m3fn():
    b = np.arange(256, dtype=np.uint8)
    v = torch.from_numpy(b).view(torch.float8_e4m3fn).to(torch.float32).numpy().astype(F64)
    finite = v[np.isfinite(v)]
    assert np.array_equal(np.unique(finite), R.e4m3_values()) and len(R.e4m3_values()) == 253  # 254 bytes, +0 == -0
    x = np.random.RandomState(2).randn(4096) * 50
    q = R.e4m3_nearest(x)
    assert np.isin(q.astype(F64), R.e4m3_values()).all()
    qt = torch.from_numpy(x.astype(F32)).to(torch.float8_e4m3fn).to(torch.float32).numpy()
    assert (np.abs(q - x) <= np.abs(qt - x) + 1e-12).all()


def test_frag_off_mirror_round_trips():
    for rows, K in ((32, 128), (96, 256), (64, 1280)):
        m, k = np.meshgrid(np.arange(rows), np.arange(K), indexing="ij")
        off = np.concatenate([R.frag_off(m, k, part, K).reshape(-1) for part in (0, 1)])
        assert np.array_equal(np.sort(off), np.arange(2 * rows * K))  # a bijection onto [0, 2 rows K)
        # the layout the kernels' operand loads assume: lane = (k / 8 % 4) * 16 + m % 16 reads 8 consecutive k; tiles 512, parts 1024 apart
        assert R.frag_off(17, 40, 1, K) == ((((0 * (K >> 5) + 1) * 2 + 1) * 2 + 1) * 64 + (1 * 16 + 1)) * 8
        assert R.frag_off(0, 0, 1, K) == 1024 and R.frag_off(16, 0, 0, K) == 512 and R.frag_off(0, 32, 0, K) == 2048


@pytest.mark.parametrize("case", [c for c in SMALL if c.tier == "A"], ids=repr)
def test_tier_a_arithmetic_is_exact(case):
    R.check_tier_a(case)


def test_tier_a_arithmetic_of_the_large_cases_inputs():
    """the large Tier A cases: the input grids and the S bound (their references are computed once, on the GPU side)"""
    for c in R.all_cases():
        if c.tier == "A" and c not in SMALL:
            c.build()
            S = np.abs(c.x.astype(F64)) @ np.abs(c.w.astype(F64)).T
            assert S.max() < 2 ** 24 * R.GRID_A and c.K <= 4096, c.id


# ---------------------------------------------------------------------------------------------------------------------- plans, without a device
def test_plan_names_and_grids_of_every_gpu_case():
    seen = set()
    for c in R.all_cases():
        name, grid = c.plan()
        assert name == c.expect, (c.id, name, c.expect)
        if c.grid is not None:
            assert grid == c.grid, (c.id, grid, c.grid)
        seen.add(name)
    listed = R.listed_variants()
    assert seen <= listed, sorted(seen - listed)       # no case reaches an unlisted variant
    assert listed <= seen, sorted(listed - seen)       # every listed variant is reached
    print(f"{len(listed)} listed variants, {len(R.all_cases())} cases")


def test_panel_loop_cases_run_it_twice():
    """gridDim.z < panels: the first_panel = false path (k_gemm3) and the cross-panel prefetch (k_gemm_big)"""
    for cid in ("g3-STORE-panels-N6400-A", "g3-RESIDUAL-panels-N6400-B", "big-RESIDUAL-M289-N4096-xpanel-A", "g3-QKV-panels-pre-M416-A",
                "g3-QKV_RMS-panels-pre-M416-B", "g3-SWIGLU_RMS-panels-N6400-A", "g3-STORE_RMS-panels-N6400-B"):
        c = CASES[cid]
        _, grid = c.plan()
        assert grid[2] < -(-c.M // 32), (cid, grid)


def test_big_min_m_moves_shapes_between_kernels_for_one_call():
    c = R.Case("t", "rows", "A", "", 64, 64, 1024, epi="STORE", big_min_m=16)
    assert c.plan()[0] == "big/STORE/bf16"
    assert R.Case("t", "rows", "A", "", 64, 64, 1024, epi="STORE").plan()[0] == "gemm3/STORE/nks8/rt1/bf16"
    # the production thresholds: 4 x 128 rows, or 128 rows with >= 64 (tile, K range) blocks
    name = lambda M, N: R.Case("t", "rows", "A", "", M, N, 1024, epi="STORE").plan()[0]
    assert name(511, 64).startswith("gemm3") and name(512, 64).startswith("big")
    assert name(128, 4096).startswith("big") and name(127, 4096).startswith("gemm3") and name(128, 4032).startswith("gemm3")


def test_rejected_cases_are_validation_errors():
    """refused on the host, with or without a device: the message is the validation's, never a launch's or 'no HIP device'"""
    for label, c, over, text in R.rejected_cases():
        rc, msg = R.call_rejected(c, over)
        assert rc != 0, label
        assert text in msg and "no HIP device" not in msg and "hip" not in msg.split(":")[0].lower(), (label, msg)


# ---------------------------------------------------------------------------------------------------------------------- teeth
def _moved(case, base, mutd):
    """how far the mutation moves the reference: max over outputs and elements of |moved| / tol where the element has a tolerance, of
    |moved| / one grid step where it is exact; a NaN pattern change counts as infinite"""
    worst = 0.0
    for name, (ref, tol) in base.items():
        if name.startswith("_") or name == "Y_unsplit":
            continue
        mut = mutd[name][0]
        if (np.isnan(ref) != np.isnan(mut)).any():
            return np.inf
        d = np.abs(np.nan_to_num(mut) - np.nan_to_num(ref))
        unit = np.where(tol > 0, 10.0 * tol, R.GRID_A)
        worst = max(worst, float((d / unit).max()))
    return worst


def test_every_mutation_moves_every_applicable_case():
    caught, weakest = {}, {}
    for c in SMALL:
        c.build()
        deep = c.op != "prep" and c.tier == "B" and c.K // c.ksplit != 128
        base = None
        for mut in R.MUTATIONS:
            if not R.mutation_applies(c, mut):
                continue
            if deep and mut in ("lo_drop", "lo_kstep"):
                continue  # (module docstring of gemm_refs: the n u S of a deep Tier B case is too loose for a lo-plane error; its Tier A twin is not)
            if base is None:
                base = R.reference(c)
            with np.errstate(all="ignore"):
                r = _moved(c, base, R.reference(c, mut))
            assert r >= 1.0, (c.id, mut, r)
            caught[(mut, c.tier)] = caught.get((mut, c.tier), 0) + 1
            weakest[mut] = min(weakest.get(mut, np.inf), r)
    for mut in R.MUTATIONS:
        assert caught.get((mut, "A"), 0) >= 1, f"no Tier A case for {mut}"
    for mut in ("lo_drop", "lo_kstep", "tile_swap", "k_quarter", "scale_shift", "rope_norot", "kpos-1", "pt_neighbor", "slab_missing"):
        assert caught.get((mut, "B"), 0) >= 1, f"no Tier B case for {mut}"
    print("cases caught per (mutation, tier):", caught)
    print("weakest |moved| / (10 tol or one grid step):", {k: f"{v:.3g}" for k, v in weakest.items()})
