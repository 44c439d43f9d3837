"""Every launch variant of the row-path GEMM family (csrc/lm_gemm.hip: k_prep, k_gemm3, k_gemm_big, k_gemm_down), one launcher call at a time,
against the float64 definitions of tests/gemm_refs.py (pinned on the CPU by test_gemm_ref_cpu.py, which also plans every case, holds the
table of listed variants against the names reached, and proves the teeth of these cases).

One entry point, fs_selftest_gemm (include/fishrt.h), runs ONE k_prep / launch_gemm3 / launch_gemm_down call on host data.  EVERY element of
EVERY output of EVERY case is compared, and every case also asserts (_check): the plan name the launcher dispatched through (and the grid
where the case names one); every guard intact; no NaN in a live output -- the fragment rows [M, Mcap) of the GEMM input are NaN, so a live
element that depends on a row that does not exist fails here; NaN (the poison) in everything the launch must not write: rows >= M, columns
>= N of a padded row stride, pool rows of other tokens keep their bits; and the tier's comparison, naming the worst (output, index).

Tiers (derivations: gemm_refs module docstring).  A: inputs on dyadic grids, every partial sum exact in f32 in any order -- the f32 outputs
equal the float64 reference, the bf16 outputs equal it rounded once, the hi / lo planes equal the mirrored split, at every element, zero
tolerance.  B: normal data, |y - ref| <= n u S (n = 2 K_range + 4 operations, u = 2^-23, S = sum |w x|) against the split operand, + 2^-17 S
against the unsplit x, plus the epilogue terms from their operation counts.  C: bit identities (HALF == full, another gridDim.z, the `pre`
path of a first panel == the same rows in the block's later panel for RESIDUAL and for QKV / QKV_RMS with lock-step rows, k_gemm_big ==
k_gemm3 on Tier A).  k_prep without a norm is mirrored exactly (slab sums in order, then the split) on
normal data too.
The one measured quantity is the SwiGLU device function a / (1 + __expf(-a)): SILU_C = max (|hi + lo - ref| - 2^-8 |lo|) / ((|a| + 1) 2^-24
|ref|) over the Tier A SwiGLU cases (test_swiglu_allowance prints it).  Measured on an MI355X: 1.588 at a = -0.0190 (gemm_refs.
SILU_C_MEASURED); asserted: 4 x = 6.352 (SILU_C_BOUND).
Worst |err| / tol measured on an MI355X (profiles/gemm_paths_parity.txt; each test prints its own): k_gemm3 Y 0.0114 (0.0475 against the
unsplit x), k_gemm_big Y 0.0005 (0.0023), k_gemm_down X 0.0029; ss partials 0.066 / 0.016 / 0.075; bf16 cache rows 0.962 and hi + lo planes
0.925 (half-ulp bounds of the format); k_prep with a norm 0.84; every Tier A comparison exact.  No kernel had to change."""
import copy
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import gemm_refs as R
from gemm_refs import F32, F64

CASES = {c.id: c for c in R.all_cases()}
WORST = {}   # (op, output) -> worst |err| / tol seen


def _report(line):
    print(line)
    path = os.environ.get("FISHRT_PARITY_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _where(shape, idx):
    return tuple(int(p) for p in np.unravel_index(int(idx), shape))


def _compare(case, what, got, ref, tol):
    """NaN exactly where the reference has NaN (never written); elsewhere inside the bound, bit-exact where the bound is 0"""
    got = np.asarray(got, F64)
    assert got.shape == ref.shape, (case.id, what, got.shape, ref.shape)
    dead = np.isnan(ref)
    leaked = np.isnan(got) & ~dead
    assert not leaked.any(), f"{case.id}: NaN in live {what} at {_where(ref.shape, np.flatnonzero(leaked)[0])} (poison left, or a row that does not exist was read)"
    wrote = ~np.isnan(got) & dead
    assert not wrote.any(), f"{case.id}: {what} written at {_where(ref.shape, np.flatnonzero(wrote)[0])}, which the launch must not touch"
    err = np.where(dead, 0.0, np.abs(np.where(dead, 0.0, got) - np.where(dead, 0.0, ref)))
    bad = err > tol
    ratio = np.where(tol > 0, err / np.maximum(tol, 1e-300), np.where(err > 0, np.inf, 0.0))
    i = int(ratio.argmax()) if ratio.size else 0
    assert not bad.any(), (f"{case.id}: {int(bad.sum())} of {bad.size} elements of {what} outside the bound; worst |err| / tol = {ratio.reshape(-1)[i]:.3g} at "
                           f"{_where(ref.shape, i)}: got {got.reshape(-1)[i]!r}, want {ref.reshape(-1)[i]!r} +- {tol.reshape(-1)[i]:.3g}")
    w = float(np.where(tol > 0, ratio, 0.0).max()) if ratio.size else 0.0
    key = (case.op if case.op != "rows" else case.expect.split("/")[0], what)
    WORST[key] = max(WORST.get(key, 0.0), w)
    return w


def _check(case):
    res = case.run()
    assert res["name"] == case.expect, (case.id, res["name"], case.expect)
    if case.grid is not None:
        assert res["grid"] == case.grid, (case.id, res["grid"], case.grid)
    assert res["guard_ok"], f"{case.id}: a guard around a buffer the launch writes was written"
    ref = R.reference(case)
    worst = {}
    for what, (want, tol) in ref.items():
        if what.startswith("_"):
            continue
        got = {"sum": lambda: res["hi"].astype(F64) + res["lo"].astype(F64), "Y_unsplit": lambda: res["Y"]}.get(what, lambda: res[what])()
        worst[what] = _compare(case, what, got, want, tol)
    if "hi" in res and "hi" not in ref and "sum" not in ref:
        raise AssertionError(f"{case.id}: planes returned that the reference does not describe")
    if "sum" in ref:  # lo is the residual of hi
        live = ~np.isnan(ref["sum"][0])
        assert (np.abs(res["lo"][live]) <= 2.0 ** -8 * np.abs(res["hi"][live]) + 1e-38).all(), f"{case.id}: lo is not the residual of hi"
    if case.op == "down":
        assert (res["epoch1"] == 0).all(), f"{case.id}: an owner wave gave up on an exchange unit (epoch[1] = {res['epoch1'].tolist()})"
    _report(f"{case.id} [{res['name']}, grid {res['grid']}]: " + ("exact" if not any(worst.values()) else
                                                                 "worst |err| / tol " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items() if v)))
    return res


def _ids(pred):
    return [i for i, c in CASES.items() if pred(c)]


@pytest.mark.parametrize("cid", _ids(lambda c: c.op == "prep"))
def test_prep(cid):
    _check(CASES[cid])


@pytest.mark.parametrize("cid", _ids(lambda c: c.op == "rows" and c.expect.startswith("gemm3")))
def test_gemm3(cid):
    _check(CASES[cid])


@pytest.mark.parametrize("cid", _ids(lambda c: c.op == "rows" and c.expect.startswith("big")))
def test_gemm_big(cid):
    _check(CASES[cid])


@pytest.mark.parametrize("cid", _ids(lambda c: c.op == "down"))
def test_gemm_down(cid):
    """n_launches = 2: the exchange buffer still holds the previous node's units (and started as NaN partials under the previous node's tag);
    the second launch must equal its own oracle, and no owner wave may have given up"""
    _check(CASES[cid])


def test_swiglu_allowance():
    """the device's a / (1 + __expf(-a)) on exact a, b (Tier A) against the float64 expression: SILU_C (gemm_refs module docstring)"""
    c_max, at = 0.0, None
    for cid in _ids(lambda c: c.tier == "A" and c.epi in ("SWIGLU", "SWIGLU_RMS")):
        case = CASES[cid]
        res = case.run()
        ref = R.reference(case)
        a, b = ref["_swiglu_ab"]
        v = R.silu64(a) * b
        hi, lo = res["hi"][:case.M, :v.shape[1]].astype(F64), res["lo"][:case.M, :v.shape[1]].astype(F64)
        excess = np.maximum(np.abs(hi + lo - v) - 2.0 ** -8 * np.abs(lo), 0.0)
        ok = np.abs(v) > 2.0 ** -100
        c = np.where(ok, excess / ((np.abs(a) + 1) * 2.0 ** -24 * np.maximum(np.abs(v), 1e-300)), 0.0)
        if c.max() > c_max:
            i = _where(c.shape, c.argmax())
            c_max, at = float(c.max()), (cid, i, float(a[i]), float(b[i]))
    _report(f"SwiGLU device function: SILU_C measured = {c_max:.4g} at {at}; recorded SILU_C_MEASURED = {R.SILU_C_MEASURED}, asserted bound = {R.SILU_C_BOUND}")
    assert c_max <= R.SILU_C_BOUND, "the recorded allowance (4 x measured) no longer covers the device function"


# ---------------------------------------------------------------------------------------------------------------------- tier C: bit identities
def _clone(case, cid, M=None, **attrs):
    """a case of its own with the same parameters (and another M), built, then given `attrs` as its input arrays"""
    c = copy.copy(case)
    c.id, c._built = cid, False
    if M is not None:
        c.M, c.Mcap = M, -(-M // 32) * 32
    c.build()
    for k, v in attrs.items():
        setattr(c, k, v)
    return c


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.mark.parametrize("cid", ["g3-STORE-nks2-bf16-M17-B", "g3-RESIDUAL_NORM-nks2-fp8-M17-B", "g3-SWIGLU-nks8-fp8-M17-B"])
def test_half_variant_equals_the_full_variant(cid):
    """HALF at M = 16 == the full variant at M = 17 on the 16 common rows"""
    full = CASES[cid].build()
    assert full.M == 17 and not full.expect.endswith("/half")
    half = _clone(full, cid + "-half16", M=16, x=full.x[:16].copy(), w=full.w, wscale=full.wscale, y0=full.y0[:16].copy(), g=full.g)
    half.expect = full.expect + "/half"
    rf, rh = full.run(), half.run()
    assert rh["name"] == half.expect and rf["name"] == full.expect
    for what in ("Y", "hi", "lo", "ss"):
        if what in rf:
            assert np.array_equal(_bits(rf[what][..., :16, :]), _bits(rh[what][..., :16, :])), (cid, what)


def test_another_grid_z_gives_the_same_rows():
    """N = 6400 runs the panel loop twice per block (gridDim.z = 2 < 4 panels); the same weight rows in a launch with gridDim.z = 4 give the
    same output rows bit for bit"""
    wide = CASES["g3-STORE-panels-N6400-B"].build()
    narrow = _clone(wide, "narrow", x=wide.x, w=None)
    narrow.N, narrow.ldy, narrow.grid = 48, 48, (3, 1, 4)
    narrow.w = wide.w[:48].copy()
    rw, rn = wide.run(), narrow.run()
    assert rw["grid"] == (400, 1, 2) and rn["grid"] == (3, 1, 4)
    assert np.array_equal(_bits(rw["Y"][:, :wide.M, :48]), _bits(rn["Y"][:, :wide.M, :48]))


def test_pre_path_equals_a_later_panel():
    """RESIDUAL, gridDim.z = 2 < 4 panels: rows 0..31 take the residual through the `pre` slot requested at kernel entry; the same data in
    rows 64..95 (the block's second panel: `pre` must not be used) give the same values"""
    base = CASES["g3-RESIDUAL-panels-N6400-B"].build()
    x, y0 = base.x.copy(), base.y0.copy()
    x[64:96], y0[64:96] = base.x[:32], base.y0[:32]
    moved = _clone(base, "moved", x=x, y0=y0, w=base.w, g=base.g)
    rb, rm = base.run(), moved.run()
    assert rb["grid"] == (400, 1, 2)
    assert np.array_equal(_bits(rb["Y"][:32]), _bits(rm["Y"][64:96]))
    assert np.array_equal(_bits(rb["Y"][32:64]), _bits(rm["Y"][32:64]))


@pytest.mark.parametrize("cid", ["g3-QKV-panels-pre-M416-A", "g3-QKV_RMS-panels-pre-M416-A", "g3-QKV-panels-pre-M416-B", "g3-QKV_RMS-panels-pre-M416-B"])
def test_qkv_pre_path_equals_a_later_panel(cid):
    """QKV / QKV_RMS with lock-step rows (pos_step 0), gridDim.z = 12 < 13 panels: block z = 0 computes rows 0..31 with the RoPE factors of its
    `pre` slot (requested at kernel entry) and rows 384..415 in its second panel, where `pre` must not be used and s_rms is rewritten behind
    the panel barrier.  The same data in both row ranges give the same q rows and the same cached K / V rows, bit for bit"""
    base = CASES[cid].build()
    x = base.x.copy()
    x[384:416] = base.x[:32]
    attrs = dict(x=x, w=base.w, wscale=base.wscale, cos_t=base.cos_t, sin_t=base.sin_t, k0=base.k0, v0=base.v0, table=base.table)
    if base.rms:
        ss = base.ss.copy()
        ss[384:416] = base.ss[:32]
        attrs["ss"] = ss
    twin = _clone(base, cid + "-twin", **attrs)
    r = twin.run()
    assert r["name"] == base.expect and r["grid"] == (80, 1, 12) and r["guard_ok"]
    assert not np.isnan(r["Y"][:416, :base.qdim]).any()
    assert np.array_equal(_bits(r["Y"][:32]), _bits(r["Y"][384:416]))
    slot = base.pos % R.KV_PAGE
    for what in ("K", "V"):
        first = np.stack([r[what][base.page_of(m, base.pos), :, slot] for m in range(32)])
        later = np.stack([r[what][base.page_of(m, base.pos), :, slot] for m in range(384, 416)])
        assert np.array_equal(_bits(first), _bits(later)), (cid, what)


@pytest.mark.parametrize("epi,N", [("STORE", 72), ("RESIDUAL_NORM", 512), ("SWIGLU_RMS", 128), ("QKV", 0)])
def test_gemm_big_equals_gemm3_on_tier_a(epi, N):
    kw = dict(geom="MID", pos_step=1, pos=30, rope_off=1) if epi == "QKV" else {}
    big = R.Case(f"c-big-{epi}", "rows", "A", f"big/{epi}/bf16", 65, N, 1024, epi=epi, big_min_m=16, **kw).build()
    small = _clone(big, f"c-g3-{epi}")
    small.big_min_m, small.expect = 0, f"gemm3/{epi}/nks8/rt{R.EPI_RT[epi]}/bf16"
    for k in ("x", "w", "y0", "g", "ss", "cos_t", "sin_t", "k0", "v0", "table"):
        if hasattr(big, k):
            setattr(small, k, getattr(big, k))
    rb, rs = big.run(), small.run()
    assert rb["name"] == big.expect and rs["name"] == small.expect
    for what in ("Y", "hi", "lo", "K", "V"):
        if rb.get(what) is not None:
            assert np.array_equal(_bits(rb[what]), _bits(rs[what])), (epi, what)
    if epi == "RESIDUAL_NORM":  # 64-row blocks against 16-row blocks: four of the small kernel's partials make one of the big kernel's (not bitwise)
        a, b = rb["ss"][:65].astype(F64), rs["ss"][:65].astype(F64).reshape(65, -1, 4).sum(2)
        assert (np.abs(a - b) <= 66 * R.U * np.abs(a)).all()


def test_rejected_cases_launch_nothing():
    for label, c, over, text in R.rejected_cases():
        rc, msg = R.call_rejected(c, over)
        assert rc != 0 and text in msg, (label, msg)


def test_worst_ratios():
    """the summary line of a whole run of this module (measured maxima per kernel and output)"""
    _report("worst |err| / tol per (kernel, output): " + ", ".join(f"{k[0]}/{k[1]} {v:.3g}" for k, v in sorted(WORST.items())))
