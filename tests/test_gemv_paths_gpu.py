"""Every launch variant of the batch-1 node kernels (csrc/lm_kernels.hip: k_qkv, k_ffn_up, k_ffn_down, k_head, the GEMV body of k_wo, k_embed,
k_fast_embed), one launcher call at a time, against the float64 definitions of tests/gemv_refs.py (pinned on the CPU by test_gemv_ref_cpu.py,
which also plans every case and proves the teeth of these cases).

One entry point, fs_selftest_gemv (include/fishrt.h), runs ONE LmKernels launcher call on host data.  EVERY element of EVERY output of EVERY
case is compared, and every case also asserts (_check): the plan name and grid the launcher dispatched through; every guard intact; no NaN
(the poison) left in an output; for QKV the whole of both pools -- the 2 Hk Dh written elements against the reference, every other element
bit-identical to its input; and the tier's comparison, naming the worst (output, index).

Tiers (derivations: gemv_refs module docstring).  A: inputs on dyadic grids with mean(x^2) + eps an exact power of 4, every partial sum exact
in f32 in any order -- the f32 outputs equal the float64 reference, the bf16 cache rows equal it rounded once, zero tolerance (SwiGLU outputs:
the device-function allowance on exact a, b).  B: normal data, |y - ref| <= (K + c) u S plus the epilogue terms.  C: bit identities
(cache_resident true == false, state == static position source, HEAD 2037 == the first 2037 rows of 2040, QKV leaves the rest of the pools
alone).  The embedding sum is mirrored exactly.  WO_BODY relies on __expf(0) == 1 (merge weight exactly 1), asserted here.
The last test prints the worst |err| / tol per (op, weight type) of a whole run and appends it to the file named by FISHRT_PARITY_LOG
(profiles/gemv_paths_parity.txt is such a run)."""
import copy
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import attn_refs
import gemv_refs as R
from gemv_refs import F32, F64

CASES = {c.id: c for c in R.all_cases()}
WORST = {}   # (op, wt, output) -> worst |err| / tol seen
EXACT = {}   # (op, wt) -> Tier A comparisons that were exact


def _report(line):
    print(line)
    path = os.environ.get("FISHRT_PARITY_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _where(shape, idx):
    return tuple(int(p) for p in np.unravel_index(int(idx), shape))


def _compare(case, what, got, ref, tol):
    """no NaN anywhere (the poison, or a value that does not exist); inside the bound, equal where the bound is 0"""
    got = np.asarray(got, F64)
    assert got.shape == ref.shape, (case.id, what, got.shape, ref.shape)
    bad_nan = np.isnan(got)
    assert not bad_nan.any(), f"{case.id}: NaN in {what} at {_where(ref.shape, np.flatnonzero(bad_nan)[0])} (poison left: an element the launch did not write)"
    err = np.abs(got - ref)
    bad = err > tol
    ratio = np.where(tol > 0, err / np.maximum(tol, 1e-300), np.where(err > 0, np.inf, 0.0))
    i = int(ratio.argmax()) if ratio.size else 0
    assert not bad.any(), (f"{case.id}: {int(bad.sum())} of {bad.size} elements of {what} outside the bound; worst |err| / tol = {ratio.reshape(-1)[i]:.3g} at "
                           f"{_where(ref.shape, i)}: got {got.reshape(-1)[i]!r}, want {ref.reshape(-1)[i]!r} +- {tol.reshape(-1)[i]:.3g}")
    w = float(np.where(tol > 0, ratio, 0.0).max()) if ratio.size else 0.0
    key = (case.op, case.wt, what)
    WORST[key] = max(WORST.get(key, 0.0), w)
    return w


def _check(case):
    res = case.run()
    name, grid = case.expect
    assert res["name"] == name and res["grid"] == grid, (case.id, res["name"], res["grid"], name, grid)
    assert res["guard_ok"], f"{case.id}: a guard around a buffer the launch writes was written"
    ref = R.reference(case)
    worst = {}
    for what, (want, tol) in ref.items():
        if what.startswith("_"):
            continue
        if case.tier == "A" and not (case.op == "up" and what == "Y"):
            assert (tol == 0).all(), (case.id, what)   # Tier A is a zero-tolerance comparison
        worst[what] = _compare(case, what, res[what], want, tol)
    if case.op == "qkv":  # Tier C: everything outside the 2 Hk Dh written elements keeps its bits
        for what, base in (("K", case.k0), ("V", case.v0)):
            changed = res[what].view(np.uint32) != np.ascontiguousarray(base, F32).view(np.uint32)
            page, slot = int(case.table[case.pos >> 6]), case.pos & 63
            changed[page, :, slot] = False
            assert not changed.any(), f"{case.id}: {what} pool element {_where(changed.shape, np.flatnonzero(changed)[0])} outside the written row changed"
    if case.tier == "A" and not any(worst.values()):
        EXACT[(case.op, case.wt)] = EXACT.get((case.op, case.wt), 0) + 1
    _report(f"{case.id} [{res['name']}, grid {res['grid']}]: " + ("exact" if not any(worst.values()) else
                                                                 "worst |err| / tol " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items() if v)))
    return res


def _ids(op):
    return [i for i, c in CASES.items() if c.op == op]


def test_expf_of_zero_is_one():
    """WO_BODY's partials {o = a, m = 0, l = 1}: the merge weight __expf(0) / (1 * __expf(0)) is exactly 1 iff the device's __expf(0) is"""
    got = attn_refs.run_expf(np.float32([0.0, -0.0]))
    assert np.array_equal(got, np.float32([1.0, 1.0])), got


@pytest.mark.parametrize("cid", _ids("qkv"))
def test_qkv(cid):
    _check(CASES[cid])


@pytest.mark.parametrize("cid", _ids("up"))
def test_ffn_up(cid):
    _check(CASES[cid])


@pytest.mark.parametrize("cid", _ids("down"))
def test_ffn_down(cid):
    _check(CASES[cid])


@pytest.mark.parametrize("cid", _ids("head"))
def test_head(cid):
    _check(CASES[cid])


@pytest.mark.parametrize("cid", _ids("wo"))
def test_wo_body(cid):
    _check(CASES[cid])


@pytest.mark.parametrize("cid", _ids("embed"))
def test_embed(cid):
    _check(CASES[cid])


@pytest.mark.parametrize("cid", _ids("fast_embed"))
def test_fast_embed(cid):
    _check(CASES[cid])


# ---------------------------------------------------------------------------------------------------------------------- tier C: bit identities
def _twin(case, **attrs):
    """the same built inputs in a case of its own, with other attributes"""
    c = copy.copy(case.build())
    for k, v in attrs.items():
        setattr(c, k, v)
    return c


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _same(ra, rb, cid):
    for what in ("Y", "K", "V"):
        if ra.get(what) is not None:
            assert np.array_equal(_bits(ra[what]), _bits(rb[what])), (cid, what)


@pytest.mark.parametrize("cid", ["qkv-TINY-fp8-pos63-ro0-state-nt-B", "qkv-FISH-bf16-pos200-ro7-state-nt-B", "qkv-MID-f32-pos64-ro7-static-res-A",
                                 "wo-TINY-f32-res-B", "wo-FISH-fp8-res-B", "wo-MID-bf16-res-A", "up-K128-fp8-inter130-nt-B", "up-K4096-bf16-inter130-nt-B",
                                 "up-K256-f32-inter6-res-B", "down-K128-fp8-dim5-res-B", "down-K4096-f32-dim131-nt-B", "down-K1024-bf16-dim131-nt-B"])
def test_cache_resident_equals_streamed(cid):
    """the load policy (non-temporal or default weight loads) is the only difference between the two instantiations"""
    a = CASES[cid]
    b = _twin(a, resident=not a.resident)
    ra, rb = a.run(), b.run()
    assert ra["name"] != rb["name"] and {ra["name"].rsplit("/", 1)[1], rb["name"].rsplit("/", 1)[1]} == {"nt", "res"}
    _same(ra, rb, cid)


@pytest.mark.parametrize("cid", ["qkv-TINY-bf16-pos200-ro7-state-res-B", "qkv-MID-fp8-pos64-ro7-state-nt-A", "qkv-FISH-f32-pos63-ro0-static-nt-B",
                                 "qkv-FISH-bf16-pos64-ro7-static-res-A"])
def test_state_source_equals_static_source(cid):
    """SeqState {pos, rope_off} (the slow path) against pos_static / rope_static with a null state (the fast decoder), same position"""
    a = CASES[cid]
    b = _twin(a, use_state=not a.use_state)
    ra, rb = a.run(), b.run()
    assert ra["name"] == rb["name"]
    _same(ra, rb, cid)


@pytest.mark.parametrize("wt", R.WTS)
def test_head_2037_rows_equal_the_first_rows_of_2040(wt):
    """n_rows = 2037 ends in a block with one live wave; the same rows in a launch of 2040 (whole blocks) are bit-identical"""
    tail = CASES[f"head-K1024-{wt}-n2037-tail-B"].build()
    full = R.Case(f"head-K1024-{wt}-n2040-B", "head", wt, "B", K=1024, rows=2040, xs=1.0).build()
    full.x, full.g = tail.x, tail.g
    full.w[:2037] = tail.w
    if tail.fp8:
        full.wscale[:2037] = tail.wscale
    rt, rf = tail.run(), full.run()
    assert rt["grid"] == (510, 1, 1) and rf["grid"] == (510, 1, 1) and rt["Y"].size == 2037 and rf["Y"].size == 2040
    assert np.array_equal(_bits(rt["Y"]), _bits(rf["Y"][:2037]))


def test_qkv_touches_exactly_the_written_elements():
    """a stale pool full of one bit pattern: after the call exactly 2 Hk Dh elements may differ, and they are the row of pos in its page"""
    a = CASES["qkv-MID-bf16-pos63-ro0-state-res-B"]
    fill = np.full(a.build().k0.shape, -7.0, F32)
    r = _twin(a, k0=fill, v0=fill).run()
    page, slot = int(a.table[a.pos >> 6]), a.pos & 63
    for what in ("K", "V"):
        diff = r[what] != -7.0
        assert diff.sum() <= a.Hk * a.Dh and diff[page, :, slot].sum() == diff.sum() and diff.sum() > a.Hk * a.Dh // 2, (what, int(diff.sum()))


def test_rejected_cases_launch_nothing():
    for label, c, over, text in R.rejected_cases():
        rc, msg = R.call_rejected(c, over)
        assert rc != 0 and text in msg, (label, msg)


def test_worst_ratios():
    """the summary of a whole run of this module: worst |err| / tol per (op, weight type, output), and the exact Tier A comparisons"""
    for op in R.OPS:
        for wt in R.WTS:
            keys = sorted(k for k in WORST if k[0] == op and k[1] == wt)
            if keys:
                _report(f"worst |err| / tol {op}/{wt}: " + ", ".join(f"{k[2]} {WORST[k]:.3g}" for k in keys) + f"; Tier A cases exact: {EXACT.get((op, wt), 0)}")
    assert all(v <= 1.0 for v in WORST.values())
