"""Every launch path of the attention kernels (csrc/lm_attn.hip) and of k_wo's chunk-merge prologues, one launcher call at a time, against the
float64 definitions of tests/attn_refs.py (pinned on the CPU by test_attn_ref_cpu.py, which also proves the teeth of these cases).

One entry point, fs_selftest_attn (include/fishrt.h), runs ONE AttnKernels::decode / AttnKernels::rows / LmKernels::wo call on host data.
EVERY element of EVERY case is compared, and every case also asserts (_check): no poison left in the logical output; rows >= M and partial
slots the launch does not produce still poison (NaN); all guards intact; both pools bit-identical after the launch -- except the row the
qkv-table kernel appends, which must equal bf16_rne(rope_i(table row)) bit for bit; and the plan name the launcher dispatched through.

Inputs (attn_refs.Case): K, V and the qkv table pre-rounded to the KV type.  Tiers: random N(0, 1); equal (every score equal, V dyadic: the
output is the exact mean, a miscount shows as 1 / T); planted (query head h aligned with its own token t*_h, >= 0.99 of the weight, t*
spread over 0, T - 1 and both sides of the nearest 16 / 64 / CH / 8 CH edge); range_first / range_last (the maximum in the first / last
chunk, every other score 60..80 lower: rescale factors of e^-60 and below).  Everything the kernels' comments call stale is +-2^100 (finite):
pool rows >= T, whole pages behind the slots of launched-but-empty chunks, DECODE_WO's partials buffer; the first stale row's K is aligned
with q, so an unmasked read takes the output over.  Page tables are permuted, and sequences 0 and 1 of a batch share their first page.

Bound, per element (derivation: attn_refs module docstring), with u = 2^-24, A_t = scale sum_i |q_i k_ti|, R_t = max s - s_t,
B_d = sum_t w_t |v_td|, delta = (Dh + 2) eps_q max_t A_t, eps_exp(x) = 4 c (|x| + 1) u:
    tol_d = 2 sum_t w_t (2 delta + eps_exp(R_t) + eps_p) |v_td| + (T + 64) u B_d + eps_out |o_d|
eps_q = eps_p = u on the VALU paths, 2^-16 on the MFMA prefill; eps_out = 2^-17 for hi + lo outputs, u for f32.  Through Wo:
|Wo| tol + (dim + 2) u |Wo| |a| + u (|x| + |x0|).
c is the one measured quantity: max |rel err| / ((|x| + 1) u) of the device's __expf against float64 exp (test_expf_constant prints it).
Measured on an MI355X over 2.08 M values of [-88, 0]: c = 1.203 (at x = -44.63) wherever e^x is a normal float, i.e. x >= ln 2^-126 =
-87.3365; below that the true value is subnormal and the device returns 0 -- all 15 859 such values, an absolute error below 2^-126, which
the test asserts as such (no case here has a score more than 80 below its maximum, so the flush enters no bound).  attn_refs.EXPF_C = 1.203;
asserted = 4 x measured; a measurement above 8 is a finding, not something to adopt.
Worst |err| / tol measured over all cases (MI355X; each test prints its own): decode partials 0.041, decode + k_wo merge 0.011, fused k_wo
0.022, k_attn_rows and chunked + combine 0.14, small rows 0.144, small rows from the qkv table 0.084, MFMA prefill 0.0011 (group 0.0006: its
bound is dominated by delta at eps_q = 2^-16, which the kernel's hi + lo operands stay far inside).  No kernel or launcher had to change."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import attn_refs as R
from attn_refs import F64, U

CASES = {c.id: c for c in R.all_cases()}
REACHED = {}   # case id -> plan name the launcher reported
WORST = {}     # kind -> worst |err| / tol seen


def _where(shape, idx, names):
    pos = np.unravel_index(int(idx), shape)
    return ", ".join(f"{n} {int(p)}" for n, p in zip(names, pos))


def _close(case, got, ref, tol, names):
    """every element inside its bound; the message names the worst offender"""
    err = np.abs(got.astype(F64) - ref)
    ratio = np.where(err > 0, err / np.maximum(tol, 1e-300), 0.0)
    worst = float(ratio.max()) if ratio.size else 0.0
    bad = err > tol
    assert not bad.any(), (f"{case.id}: {int(bad.sum())} of {bad.size} elements outside the bound; worst |err| / tol = {worst:.3g} at "
                           f"({_where(ratio.shape, ratio.argmax(), names)}): got {got.reshape(-1)[ratio.argmax()]!r}, want {ref.reshape(-1)[ratio.argmax()]!r}")
    WORST[case.kind] = max(WORST.get(case.kind, 0.0), worst)
    print(f"{case.id}: worst |err| / tol = {worst:.3g} (worst so far for {case.kind}: {WORST[case.kind]:.3g})")


def _check(case):
    out, ka, va, name, ok = case.run()
    REACHED[case.id] = name
    assert name == case.expect, (case.id, name, case.expect)
    assert ok, f"{case.id}: a guard around an output or a pool was written"
    # pools: untouched, bit for bit -- for the qkv-table kernel except the appended rows, which are in k_ref / v_ref
    for what, after, want in (("K", ka, case.k_ref), ("V", va, case.v_ref)):
        diff = after.view(np.uint32) != np.ascontiguousarray(want, np.float32).view(np.uint32)
        assert not diff.any(), f"{case.id}: {what} pool changed at (page, kv head, row, dim) {tuple(int(i[0]) for i in np.nonzero(diff))}"
    if case.kind == "decode":
        tpb = int(case.expect.split("tpb")[1]) if "tpb" in case.expect else 1
        ref, tol = case.reference_partials(tpb)
        got = out.reshape(ref.shape)
        written = ~np.isnan(ref)
        assert not np.isnan(got[written]).any(), f"{case.id}: poison left in a partial the launch must produce"
        assert np.isnan(got[~written]).all(), f"{case.id}: a partial slot >= nc was written"
        _close(case, np.where(written, got, 0.0), np.where(written, ref, 0.0), tol, ("head", "chunk", "element"))
    elif case.kind in ("decode_wo", "fused"):
        ref, tol = case.reference_x()
        assert np.isfinite(out).all(), f"{case.id}: x is not finite (a stale partial or row leaked in)"
        _close(case, out, ref, tol, ("row",))
    else:
        Mcap = out.size // (2 * case.K)
        hi, lo = out[:Mcap * case.K].reshape(Mcap, case.K), out[Mcap * case.K:].reshape(Mcap, case.K)
        assert np.isnan(hi[case.M:]).all() and np.isnan(lo[case.M:]).all(), f"{case.id}: a row >= M was written"
        assert not np.isnan(hi[:case.M]).any() and not np.isnan(lo[:case.M]).any(), f"{case.id}: poison left in rows < M"
        assert (np.abs(lo[:case.M]) <= 2.0 ** -8 * np.abs(hi[:case.M]) + 1e-38).all(), f"{case.id}: lo is not the residual of hi"
        ref, tol, _ = case.reference()
        got = hi[:case.M].astype(F64) + lo[:case.M].astype(F64)
        _close(case, got.reshape(ref.shape), ref, tol, ("row", "head", "dim"))


def _ids(kinds):
    return [i for i, c in CASES.items() if c.kind in kinds]


@pytest.mark.parametrize("cid", _ids(("decode",)))
def test_decode_partials(cid):
    _check(CASES[cid])


@pytest.mark.parametrize("cid", _ids(("decode_wo",)))
def test_decode_then_wo_merge(cid):
    _check(CASES[cid])


@pytest.mark.parametrize("cid", _ids(("fused",)))
def test_wo_fused_attention(cid):
    _check(CASES[cid])


@pytest.mark.parametrize("cid", _ids(("rows", "small", "tbl", "prefill", "group")))
def test_rows(cid):
    _check(CASES[cid])


def test_equal_scores_give_the_exact_mean():
    """equal tier, stated without the reference: every score of a head is equal, so the output is mean_t v_t -- V is dyadic, the mean of T
    values is off by one token's share (1 / T) for any miscount, against a bound of a few u"""
    case = CASES["rows-MID-M3-step0"]
    out = case.run()[0]
    Mcap = out.size // (2 * case.K)
    got = (out[:Mcap * case.K].astype(F64) + out[Mcap * case.K:].astype(F64)).reshape(Mcap, case.H, case.Dh)[:case.M]
    for m, (s, T) in enumerate(case.rows):
        for h in range(case.H):
            mean = R.gather(case.v, case.table[s], T, h // case.n_rep).astype(F64).mean(0)
            assert np.abs(got[m, h] - mean).max() <= (T + 64) * U * 2.0 + 2.0 ** -17 * 2.0 < 0.1 / T, (m, h)


def test_expf_constant():
    """the device's __expf against float64 exp over [-88, 0]: c = max |rel err| / ((|x| + 1) u) wherever e^x is a normal float; below that
    (x < ln 2^-126 = -87.3365) the subnormal result is flushed to 0, an absolute error below 2^-126"""
    rng = np.random.RandomState(5)
    x = np.concatenate([np.linspace(-88.0, 0.0, 1 << 20), -88.0 * rng.rand(1 << 20), -np.arange(0, 89.0), -2.0 ** -np.arange(1, 30.0)]).astype(np.float32)
    y = R.run_expf(x).astype(F64)
    ref = np.exp(x.astype(F64))
    normal = x.astype(F64) >= R.EXPF_NORMAL_MIN
    c_all = np.abs(y / ref - 1.0) / ((np.abs(x.astype(F64)) + 1.0) * U)
    c = float(c_all[normal].max())
    i = int(np.where(normal, c_all, 0).argmax())
    print(f"__expf: c = {c:.4g} at x = {x[i]!r} (got {y[i]!r}, exp {ref[i]!r}) over {int(normal.sum())} values with a normal e^x; "
          f"{int((y[~normal] == 0).sum())} of the {int((~normal).sum())} subnormal results are flushed to 0; recorded EXPF_C = {R.EXPF_C}")
    assert (y[x == 0.0] == 1.0).all()
    assert (np.abs(y[~normal] - ref[~normal]) <= 2.0 ** -126).all(), "a subnormal result is off by more than the flush"
    assert c <= R.EXPF_FINDING, "a finding: __expf is further off than 8 (|x| + 1) u"
    assert c <= 4.0 * R.EXPF_C, "the recorded constant no longer covers the device function"


def test_rejected_cases_launch_nothing():
    for label, c, text in R.rejected_cases():
        rc, msg = R.call_rejected(c)
        assert rc != 0 and text in msg, (label, msg)


def test_plan_table_equals_the_paths_reached():
    """the names the launchers reported over all cases == the table of every plan lm_attn.hip can produce (attn_refs.PLAN_TABLE)"""
    for cid, c in CASES.items():
        if cid not in REACHED:  # (a partial run of this module)
            REACHED[cid] = c.run()[3]
    reached = set(n.split("+")[0] for n in REACHED.values())
    assert reached == set(R.PLAN_TABLE), reached ^ set(R.PLAN_TABLE)
    assert {"+wo/reg", "+wo/lds"} == set("+" + n.split("+")[1] for n in REACHED.values() if "+" in n)
    print("worst |err| / tol per op:", {k: f"{v:.3g}" for k, v in WORST.items()})
