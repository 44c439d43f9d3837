"""GPU: the PREFILL pass (forward_generate over L > 1 rows: k_embed_rows, k_prep, k_gemm3 with every EPI_* epilogue and its M <= 16 half-panel
variant, k_gemm_big, the split-K down projection, k_attn_prefill_mfma / k_attn_decode + k_attn_combine on prefill rows, the RoPE + paged K/V
scatter) against the CPU oracle under the K/V-forced protocol of tests/test_kv_forced_gpu.py, at EVERY row of EVERY layer.

tests/test_kv_forced_gpu.py leaves the prefill pass with the bf16 protocol (1e-2, last row only), and the other prefill tests look at the last
row only at 2e-3 .. 1e-2: a kernel that is wrong in row 37 of a 200-row pass, in one 16-row tile or in the first token past a page boundary
moves the last row's logits by its share of the softmax weight over hundreds of keys -- far inside 1e-2.

Protocol (_forced_prefill).  For every chunk [a, b) of a schedule the GPU runs forward_generate(chunk, a); the K/V rows [a, b) it cached are
read back for every layer (fs_lm_debug_read_kv) and the oracle's pass over the same chunk is armed with them (OracleLM.force_kv_rows; the
existing single-row force_kv for one-token chunks): layer l of the oracle attends over, and caches, bit for bit the rows the kernel cached, so
layer l + 1 of both sees the same inputs up to the summation order of ONE layer.  Before they are replaced, the oracle's own rows are compared
with the forced ones, per entry: excess = max(0, |own value before its bf16 rounding - forced| - half a bf16 ulp of the forced value) -- ~0 for
a correctly rounded neighbour of any magnitude, absolute f32 error otherwise.  Layer l's K/V rows are a function of every row of layer l - 1's
GEMMs and attention, so all rows of all layers check every row of every prefill kernel except the last layer's tail, which is checked at the
last row of every chunk through the hidden state and the logits.

Bounds (the ones of tests/test_kv_forced_gpu.py: same quantities, same protocol): last-row max |dlogit| over [im_end:] <= SLOW_TOL = 2e-4,
last-row max |dh| / rms(h) <= 2e-4, per-entry K/V excess <= 1.2e-4 = 16 x 2^-17 (one-token chunks go through force_kv and keep its own
measure: <= 16 units).  A failure names the worst (layer, row, K or V): that localises a bug to a stage, a row tile or a page.  Every measured
maximum goes to stdout and, when FISHRT_PARITY_LOG names a file, into it (profiles/prefill_forced_parity.txt).

Shapes: Fish-1.5 widths with 3 layers (dim 1024 / intermediate 4096 are what k_gemm_big needs: K / ksplit == 1024; three layers put layer 0's
output through a checked layer twice; the oracle pass costs 1/8 of the 24-layer one), plus MID (dim 256, head_dim 64) and TINY (head_dim 32:
chunked row attention + k_attn_combine) of tests/test_lm_gpu.py.  Synthetic weights, forward_generate only: no persistent kernel is involved.
tests/test_oracle_force_rows.py runs this file's comparison code on the CPU with a second oracle in the GPU's place and a planted error."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import fishrt
from fishrt import config as fcfg
from oracle import oracle as orc

SEED = 0xF15E5EED
SLOW_TOL = 2e-4      # last-row logits (tests/test_kv_forced_gpu.py)
HIDDEN_TOL = 2e-4    # last-row max |dh| / rms(h)
EXCESS_TOL = 1.2e-4  # per-entry K/V excess: 16 x 2^-17, "the same bound as SLOW_TOL" (tests/test_kv_forced_gpu.py)
UNITS_TOL = 16.0     # one-token chunks (force_kv): bf16 ulps of the forced value, floored at 2^-17 (tests/test_kv_forced_gpu.py)

FISH3 = dict(fcfg.FISH_1_5, n_layer=3)
OFISH3 = dict(orc.FISH15, n_layer=3)
MID = dict(fcfg.TINY, dim=256, n_head=4, n_local_heads=2, head_dim=64, intermediate_size=1024)   # = test_lm_gpu.MID
OMID = dict(orc.TINY, dim=256, n_head=4, n_local_heads=2, head_dim=64, intermediate_size=1024)

# one-pass lengths: edges of the code, not workload sizes.  2 / 16 / 17: the M <= 16 GEMM variant and its boundary, one vs two 16-row attention
# tiles; 32 / 33: the PF_M panel; 64 / 65: KV_PAGE, first row past a page; 127 / 128 / 129: GB_MIN_M (W13 and W2 switch to k_gemm_big);
# 256 / 257: four pages (every wave of k_attn_prefill_mfma owns exactly one), then a fifth; 511 / 512 / 513: Wqkv and Wo switch to k_gemm_big
# and nblk_o of the fused sum-of-squares changes
FISH_LENS = [2, 16, 17, 32, 33, 64, 65, 127, 128, 129, 256, 257, 511, 512, 513]
SMALL_LENS = [2, 16, 17, 33, 64, 65, 129]
FP8_LENS = [17, 65, 129, 513]
# cached-prefix schedules (attention pos0 != 0, page tables start mid-page): a big-GEMM chunk starting mid-page, then the 3-row variant; ...
SCHEDULES = [[0, 70, 200, 203], [0, 1, 66], [0, 64, 65, 193], [0, 130, 131, 140]]


def prompt(L, seed, text_ids, sem_start, cb_size):
    """a random text row plus a few VQ columns (k_embed_rows sums the 8 codebook embeddings there) -- always one at row 0 and one at the last row"""
    rng = np.random.RandomState(seed)
    p = np.zeros((9, L), np.uint32)
    p[0] = rng.randint(0, text_ids, L)
    cols = set([0, L - 1] + [int(c) for c in rng.randint(0, L, 1 + L // 8)])
    for c in sorted(cols):
        codes = rng.randint(0, cb_size, 8)
        p[0, c] = sem_start + codes[0]
        p[1:, c] = codes
    return p


def _forced_prefill(lm, o, p, cuts):
    """Runs the chunk schedule `cuts` of prompt `p` on `lm` (the GPU handle: forward_generate, debug_read_kv, clear_slow_layer_caches, cfg) and,
    K/V-forced on the rows lm cached, on the oracle `o`.  Returns the record _check judges:
    excess (n_layer, L, 2) [K | V] (NaN on rows of one-token chunks), units (n_layer, L), dlogit / dhidden: worst over the chunks' last rows"""
    n_layer, L, im_end = lm.cfg["n_layer"], p.shape[1], o.cfg["im_end_id"]
    assert cuts[0] == 0 and cuts[-1] == L
    excess = np.full((n_layer, L, 2), np.nan, np.float32)
    units = np.zeros((n_layer, L), np.float32)
    dlogit = dhidden = 0.0
    lm.clear_slow_layer_caches(); o.clear_slow()
    for a, b in zip(cuts[:-1], cuts[1:]):
        chunk = np.ascontiguousarray(p[:, a:b])
        lg, hg = lm.forward_generate(chunk, a)
        kv = [lm.debug_read_kv(l, a, b - a) for l in range(n_layer)]
        for l in range(n_layer):
            if b - a == 1:
                o.force_kv(l, kv[l][0][0], kv[l][1][0])
            else:
                o.force_kv_rows(l, kv[l][0], kv[l][1])
        lo, ho = o.forward_generate(chunk, a, full_head=False)
        for l in range(n_layer):
            if b - a == 1:
                units[l, a] = o.force_kv_diff(l)
            else:
                excess[l, a:b] = o.force_kv_row_excess(l, split=True).T
                units[l, a:b] = o.force_kv_row_units(l)
        dlogit = max(dlogit, float(np.abs(lg[0, im_end:] - lo[0, im_end:]).max()))
        dhidden = max(dhidden, float(np.abs(hg[0] - ho[0]).max() / np.sqrt(np.mean(np.square(ho[0], dtype=np.float64)))))
    return dict(excess=excess, units=units, dlogit=dlogit, dhidden=dhidden, cuts=list(cuts))


def _worst(rec):
    """(excess, layer, row, 'K' | 'V') of the worst multi-row entry (0.0 when every chunk had one token)"""
    ex = np.nan_to_num(rec["excess"], nan=-1.0)
    l, r, w = np.unravel_index(int(np.argmax(ex)), ex.shape)
    return max(float(ex[l, r, w]), 0.0), int(l), int(r), "KV"[w]


def _line(what, rec):
    x, l, r, w = _worst(rec)
    ul, ur = np.unravel_index(int(np.argmax(rec["units"])), rec["units"].shape)
    per_layer = " ".join(f"{max(float(np.nan_to_num(rec['excess'][i], nan=0.0).max()), 0.0):.1e}" for i in range(rec["excess"].shape[0]))
    return (f"{what}: chunks {rec['cuts']}: K/V excess {x:.2e} (layer {l}, row {r}, {w}; per layer {per_layer}), {float(rec['units'].max()):.1f} units "
            f"(layer {ul}, row {ur}); last rows: max |dlogit| {rec['dlogit']:.2e}, max |dh| / rms(h) {rec['dhidden']:.2e}  "
            f"[bounds {EXCESS_TOL:.1e} / {SLOW_TOL:.0e} / {HIDDEN_TOL:.0e}]")


def _report(line):
    print(line)
    path = os.environ.get("FISHRT_PARITY_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _check(what, rec):
    """the bounds of this file on one _forced_prefill record; reports the measured maxima first"""
    _report(_line(what, rec))
    x, l, r, w = _worst(rec)
    assert x <= EXCESS_TOL, (f"{what}: the {w} row the prefill pass cached at layer {l}, row {r} is {x:.2e} (beyond half a bf16 ulp) from the oracle's "
                             f"on identical inputs [bound {EXCESS_TOL:.1e}]; rows over the bound per layer: "
                             f"{[np.nonzero(np.nan_to_num(rec['excess'][i]).max(1) > EXCESS_TOL)[0].tolist()[:24] for i in range(rec['excess'].shape[0])]}")
    one = np.isnan(rec["excess"][:, :, 0])  # rows of one-token chunks: force_kv's own measure
    if one.any():
        u = np.where(one, rec["units"], 0.0)
        ul, ur = np.unravel_index(int(np.argmax(u)), u.shape)
        assert u.max() <= UNITS_TOL, f"{what}: the K/V row of the one-token step at layer {ul}, row {ur} is {u.max():.1f} units from the oracle's"
    assert rec["dhidden"] <= HIDDEN_TOL, f"{what}: last-row hidden state max |dh| / rms(h) {rec['dhidden']:.2e} > {HIDDEN_TOL:.0e}"
    assert rec["dlogit"] <= SLOW_TOL, f"{what}: last-row logits max |dlogit| {rec['dlogit']:.2e} > {SLOW_TOL:.0e}"


# ---------------------------------------------------------------- handles (one per shape and dtype for the module)
def _pair(cfg, ocfg, tok, dtype):
    lm = fishrt.DualARTransformer(cfg, tok, 0, dtype).load_synthetic(SEED)
    o = orc.OracleLM(ocfg).load_synthetic(SEED, bf16=(dtype == "bf16"), fp8=(dtype == "fp8"))
    o.set_kv_round_bf16(True)
    return lm, o


@pytest.fixture(scope="module")
def fish_bf16():
    lm, o = _pair(FISH3, OFISH3, fcfg.FISH_1_5_TOKENS, "bf16")
    yield lm, o
    lm.close()


@pytest.fixture(scope="module")
def fish_fp8():
    lm, o = _pair(FISH3, OFISH3, fcfg.FISH_1_5_TOKENS, "fp8")
    yield lm, o
    lm.close()


@pytest.fixture(scope="module")
def mid_bf16():
    lm, o = _pair(MID, OMID, fcfg.TINY_TOKENS, "bf16")
    yield lm, o
    lm.close()


@pytest.fixture(scope="module")
def tiny_bf16():
    lm, o = _pair(fcfg.TINY, orc.TINY, fcfg.TINY_TOKENS, "bf16")
    yield lm, o
    lm.close()


def _fish_prompt(L):
    return prompt(L, 7000 + L, 100000, fcfg.FISH_1_5_TOKENS["semantic_start_id"], 1024)


def _small_prompt(L):
    return prompt(L, 7000 + L, 400, fcfg.TINY_TOKENS["semantic_start_id"], 64)


# ---------------------------------------------------------------- one pass
@pytest.mark.parametrize("L", FISH_LENS)
def test_fish_width_one_pass_every_row_kv_forced(fish_bf16, L):
    """Fish-1.5 widths, 3 layers, bf16: ONE prefill pass of L rows, every K/V row of every layer + the last row's hidden state and logits"""
    lm, o = fish_bf16
    _check(f"fish-1.5 x 3 layers bf16, one pass of {L}", _forced_prefill(lm, o, _fish_prompt(L), [0, L]))


@pytest.mark.parametrize("L", FP8_LENS)
def test_fish_width_one_pass_every_row_kv_forced_fp8(fish_fp8, L):
    """the e4m3 images (`wscale` kernel twins) against the fp8-mode oracle (same integer quantiser, computes on the dequantised values)"""
    lm, o = fish_fp8
    _check(f"fish-1.5 x 3 layers fp8, one pass of {L}", _forced_prefill(lm, o, _fish_prompt(L), [0, L]))


@pytest.mark.parametrize("L", SMALL_LENS)
def test_mid_one_pass_every_row_kv_forced(mid_bf16, L):
    """dim 256, head_dim 64 (flash prefill; k_gemm3 at every M: k_gemm_big needs K / ksplit == 1024)"""
    lm, o = mid_bf16
    _check(f"MID bf16, one pass of {L}", _forced_prefill(lm, o, _small_prompt(L), [0, L]))


@pytest.mark.parametrize("L", SMALL_LENS)
def test_tiny_one_pass_every_row_kv_forced(tiny_bf16, L):
    """head_dim 32: the chunked row attention (k_attn_decode on prefill rows + k_attn_combine)"""
    lm, o = tiny_bf16
    _check(f"TINY bf16, one pass of {L}", _forced_prefill(lm, o, _small_prompt(L), [0, L]))


# ---------------------------------------------------------------- cached-prefix schedules
@pytest.mark.parametrize("cuts", SCHEDULES, ids=["-".join(map(str, c)) for c in SCHEDULES])
def test_fish_width_cached_prefix_schedules_kv_forced(fish_bf16, cuts):
    """chunks over a cached prefix: attention pos0 != 0, page tables start mid-page, one-token chunks between passes (decode kernels)"""
    lm, o = fish_bf16
    _check("fish-1.5 x 3 layers bf16, schedule", _forced_prefill(lm, o, _fish_prompt(cuts[-1]), cuts))


def test_fish_width_cached_prefix_schedule_kv_forced_fp8(fish_fp8):
    lm, o = fish_fp8
    cuts = SCHEDULES[0]
    _check("fish-1.5 x 3 layers fp8, schedule", _forced_prefill(lm, o, _fish_prompt(cuts[-1]), cuts))


@pytest.mark.parametrize("which", ["mid", "tiny"])
@pytest.mark.parametrize("cuts", SCHEDULES, ids=["-".join(map(str, c)) for c in SCHEDULES])
def test_small_cached_prefix_schedules_kv_forced(which, cuts, request):
    lm, o = request.getfixturevalue(f"{which}_bf16")
    _check(f"{which.upper()} bf16, schedule", _forced_prefill(lm, o, _small_prompt(cuts[-1]), cuts))


# ---------------------------------------------------------------- group prefill
def test_mid_group_prefill_rows_bit_identical_to_solo_pass(mid_bf16):
    """Group prefill of a static batch (EPI_QKV_SEQ, blockIdx.y sequences of k_attn_prefill_mfma; the ragged B = 5 lengths of
    test_lm_gpu.test_mid_static_batch_group_prefill_vs_oracle): for every slot, the K/V rows the group pass cached, in every layer, are
    BIT-identical to the rows a solo forward_generate of the same tokens leaves in slot 0 of a batch-1 handle.  test_lm_gpu claims this
    independence on greedy tokens only.  The solo pass itself is held to the oracle by the forced cases above.

    A static batch left-pads every prompt to Lmax columns (static_batch.rs:68-111; the pad is not masked) and the group pass runs the first
    Lmax - 1 columns of every slot, so `the prompt` of slot b is its padded form and the rows compared are [0, Lmax - 1) -- for the longest
    prompt, rows [0, len - 1) of the prompt itself.  MID never takes k_gemm_big (K / ksplit is 256), so the kernel choice does not depend on M
    there (85 rows in the group pass, 17 in a solo one, both above the M <= 16 variant): bit identity is the expectation, not a tolerance."""
    solo, _ = mid_bf16
    B, span = 5, 17
    lens = [3 + (5 * i) % span for i in range(B)]
    prompts = [_small_prompt(L) for L in lens]
    Lmax = max(lens)
    lm = fishrt.DualARTransformer(MID, fcfg.TINY_TOKENS, 0, "bf16", B).load_synthetic(SEED)
    lm.generate_static_batch(prompts, Lmax + 1, seed=42, temp=0.0, top_p=1.0, top_k=0, ignore_eos=True)
    n_layer, im_end = MID["n_layer"], fcfg.TINY_TOKENS["im_end_id"]
    bad = []
    for b in range(B):
        padded = np.zeros((9, Lmax), np.uint32)
        padded[0, : Lmax - lens[b]] = im_end
        padded[:, Lmax - lens[b]:] = prompts[b]
        solo.clear_slow_layer_caches()
        solo.forward_generate(np.ascontiguousarray(padded[:, : Lmax - 1]), 0)
        for l in range(n_layer):
            gk, gv = lm.debug_read_kv(l, 0, Lmax - 1, slot=b)
            sk, sv = solo.debug_read_kv(l, 0, Lmax - 1)
            for name, g, s in (("K", gk, sk), ("V", gv, sv)):
                rows = np.nonzero((g.view(np.uint32) != s.view(np.uint32)).any((1, 2)))[0]
                if rows.size:
                    bad.append((b, l, name, rows.tolist(), float(np.abs(g - s).max())))
    lm.close()
    _report(f"MID group prefill, lens {lens}: {B} slots x {n_layer} layers x {Lmax - 1} rows of K and V vs the solo pass: "
            f"{'bit-identical' if not bad else f'{len(bad)} (slot, layer, K|V) differ'}")
    assert not bad, f"(slot, layer, K|V, rows, max |d|) where the group pass's cached rows differ from the solo pass's: {bad}"
