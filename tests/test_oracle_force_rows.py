"""CPU: the oracle's multi-row K/V force hook (OracleLM.force_kv_rows / force_kv_row_excess, oracle_lm.cpp LM::block_forward) and the comparison
code of tests/test_prefill_forced_gpu.py with a second oracle standing in for the GPU -- the forced-prefill protocol must be transparent on
identical inputs and must FAIL, naming the place, on a planted error."""
import numpy as np
import pytest

from oracle import oracle as orc
import test_prefill_forced_gpu as pf

SEED = 0xF15E5EED
NL, HK, DH = orc.TINY["n_layer"], orc.TINY["n_local_heads"], orc.TINY["head_dim"]


def _oracle(round_kv=True, acc64=False):
    o = orc.OracleLM(orc.TINY).load_synthetic(SEED, bf16=True)
    o.set_kv_round_bf16(round_kv)
    o.set_acc64(acc64)
    return o


def _p(L):
    return pf.prompt(L, 7000 + L, 400, orc.TINY["semantic_start_id"], 64)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("round_kv", [True, False], ids=["bf16-kv", "f32-kv"])
@pytest.mark.parametrize("cuts", [[0, 40], [0, 13, 40], [0, 1, 2, 38, 40]], ids=["one-pass", "cached-prefix", "with-single-rows"])
def test_forcing_own_rows_changes_nothing(round_kv, cuts):
    """a pass forced on the oracle's OWN rows (read back from the cache of an unforced run) is the unforced pass bit for bit -- logits, hidden
    state, every cached row -- and reports excess 0 and 0 units at every row (a value is within half an ulp of its own rounding)"""
    p = _p(cuts[-1])
    a, b = _oracle(round_kv), _oracle(round_kv)
    for s, e in zip(cuts[:-1], cuts[1:]):
        chunk = np.ascontiguousarray(p[:, s:e])
        la, ha = a.forward_generate(chunk, s)
        for l in range(NL):
            k, v = a.get_kv(l, s, e - s)
            assert k.shape == (e - s, HK, DH)
            if e - s == 1:
                b.force_kv(l, k[0], v[0])
            else:
                b.force_kv_rows(l, k, v)
        lb, hb = b.forward_generate(chunk, s)
        assert np.array_equal(_bits(la), _bits(lb)) and np.array_equal(_bits(ha), _bits(hb))
        for l in range(NL):
            assert b.force_kv_diff(l) == 0.0
            if e - s > 1:
                x = b.force_kv_row_excess(l, split=True)
                assert x.shape == (2, e - s) and not x.any()
                assert not b.force_kv_row_excess(l).any() and not b.force_kv_row_units(l).any()
            ka, va = a.get_kv(l, 0, e)
            kb, vb = b.get_kv(l, 0, e)
            assert np.array_equal(_bits(ka), _bits(kb)) and np.array_equal(_bits(va), _bits(vb))
    # one-shot: the next pass runs on the oracle's own rows again
    assert a.kv_len() == b.kv_len() == cuts[-1]


@pytest.mark.parametrize("which", ["K", "V"])
@pytest.mark.parametrize("layer,row,head,dim,delta", [(0, 0, 0, 0, 3e-3), (1, 22, 1, 31, -1e-2), (1, 39, 0, 7, 5e-3)])
def test_known_perturbation_is_reported_at_its_row(which, layer, row, head, dim, delta):
    """rows perturbed by a known amount in ONE (layer, row, head, dim): the record holds exactly max(0, |own - forced| - ulp(forced) / 2) at that
    row, in the K or the V half, and 0 everywhere else in that layer and in the layers before it.  f32 K/V: the oracle's own entry is the cached
    one, so `own` is known exactly.  (The head / dim -> row mapping is what the (n, Hkv, D) <-> (Hkv, L, D) transpose could get wrong.)"""
    L = 40
    p = _p(L)
    a, b = _oracle(False), _oracle(False)
    a.forward_generate(p, 0)
    own = None
    for l in range(NL):
        k, v = a.get_kv(l, 0, L)
        if l == layer:
            t = k if which == "K" else v
            own = float(t[row, head, dim])
            t[row, head, dim] = np.float32(own + delta)
            forced = float(t[row, head, dim])
        b.force_kv_rows(l, k, v)
    b.forward_generate(p, 0)
    u = 2.0 ** (np.floor(np.log2(abs(forced))) - 7)
    exp = max(0.0, abs(np.float32(np.float32(own) - np.float32(forced))) - 0.5 * u)
    assert exp > 0  # (the deltas are chosen above half an ulp of entries of this model's size, < 1)
    for l in range(layer + 1):
        x = b.force_kv_row_excess(l, split=True)
        want = np.zeros((2, L), np.float32)
        if l == layer:
            want[0 if which == "K" else 1, row] = exp
        np.testing.assert_allclose(x, want, rtol=1e-6, atol=0)
        assert np.array_equal(b.force_kv_row_excess(l), x.max(0))
    # the pass attended over the forced rows and cached them
    k, v = b.get_kv(layer, row, 1)
    assert float((k if which == "K" else v)[0, head, dim]) == forced
    if layer + 1 < NL:  # causal: the rows before the perturbed one saw nothing of it in the layers behind
        assert not b.force_kv_row_excess(layer + 1)[:row].any()


def test_excess_takes_half_an_ulp_off_whatever_the_magnitude():
    """bf16 K/V: the forced rows are the oracle's own ROUNDED rows moved by one bf16 ulp -- the units of force_kv_diff say ~1 for every entry,
    the excess says what is beyond half an ulp: between 0 and 1 ulp of the entry, i.e. it scales with the entry, unlike the floored unit"""
    L = 24
    p = _p(L)
    a, b = _oracle(True), _oracle(True)
    a.forward_generate(p, 0)
    k, v = a.get_kv(0, 0, L)
    ulp = np.exp2(np.floor(np.log2(np.maximum(np.abs(k), 1e-30))) - 7).astype(np.float32)
    b.force_kv_rows(0, k + ulp, v)
    for l in range(1, NL):
        b.force_kv_rows(l, *a.get_kv(l, 0, L))
    b.forward_generate(p, 0)
    x = b.force_kv_row_excess(0, split=True)
    assert not x[1].any()
    row_max_ulp = ulp.reshape(L, -1).max(1)
    assert (x[0] > 0).all() and (x[0] <= 1.0001 * row_max_ulp).all()
    assert b.force_kv_diff(0) >= 1.0


def test_wrong_row_count_raises_and_disarms():
    p = _p(12)
    a, b = _oracle(), _oracle()
    la, _ = a.forward_generate(p, 0)
    k, v = a.get_kv(0, 0, 12)
    b.force_kv_rows(0, k[:11], v[:11])
    with pytest.raises(RuntimeError, match="force_kv_rows"):
        b.forward_generate(p, 0)
    b.clear_slow()
    lb, _ = b.forward_generate(p, 0)  # disarmed by the refusal
    assert np.array_equal(_bits(la), _bits(lb))
    b.force_kv_rows(0, k, v)
    with pytest.raises(RuntimeError, match="force_kv_rows"):  # a single-token step is no 12-row pass either
        b.forward_generate(np.ascontiguousarray(p[:, :1]), 12)
    with pytest.raises(RuntimeError):
        b.force_kv_rows(NL, k, v)
    b.force_kv(0, k[0], v[0])  # the single-row hook still refuses a multi-row pass
    b.clear_slow()
    with pytest.raises(RuntimeError, match="single-token"):
        b.forward_generate(p, 0)


def test_acc64_oracle_is_the_f32_oracle_up_to_summation_noise():
    p = _p(33)
    lf, hf = _oracle().forward_generate(p, 0)
    ld, hd = _oracle(acc64=True).forward_generate(p, 0)
    assert not np.array_equal(lf, ld)
    # bf16 K/V without forcing: rounding-boundary flips compound, so this is the loose bf16 protocol, not a noise measurement
    np.testing.assert_allclose(lf, ld, rtol=0, atol=2e-3)
    np.testing.assert_allclose(hf, hd, rtol=0, atol=2e-3)


# ---------------------------------------------------------------- tests/test_prefill_forced_gpu.py's comparison code, an oracle in the GPU's place
class _OracleAsGpu:
    """what _forced_prefill needs of the GPU handle, served by a second oracle with a bf16-rounded cache; `plant` = (layer, row, head, dim, K|V,
    delta) corrupts that cached entry as the rows are read back"""
    def __init__(self, plant=None):
        self.o, self.cfg, self.plant = _oracle(), dict(orc.TINY), plant

    def clear_slow_layer_caches(self):
        self.o.clear_slow()

    def forward_generate(self, chunk, pos):
        return self.o.forward_generate(chunk, pos, full_head=False)

    def debug_read_kv(self, layer, t0, n):
        k, v = self.o.get_kv(layer, t0, n)
        if self.plant and self.plant[0] == layer and t0 <= self.plant[1] < t0 + n:
            _, row, head, dim, which, delta = self.plant
            (k if which == "K" else v)[row - t0, head, dim] += np.float32(delta)
        return k, v


@pytest.mark.parametrize("cuts", [[0, 65], [0, 30, 31, 65]], ids=["one-pass", "schedule"])
def test_forced_prefill_comparison_is_transparent_on_identical_inputs(cuts):
    rec = pf._forced_prefill(_OracleAsGpu(), _oracle(), _p(65), cuts)
    assert rec["excess"].shape == (NL, 65, 2)
    assert np.nan_to_num(rec["excess"]).max() == 0.0 and rec["units"].max() == 0.0 and rec["dlogit"] == 0.0 and rec["dhidden"] == 0.0
    assert np.isnan(rec["excess"]).any() == (cuts != [0, 65])  # one-token chunks carry no excess record, only units
    pf._check("oracle in the GPU's place", rec)


@pytest.mark.parametrize("which", ["K", "V"])
@pytest.mark.parametrize("cuts", [[0, 65], [0, 30, 31, 65]], ids=["one-pass", "schedule"])
def test_forced_prefill_comparison_fails_on_a_planted_error_and_names_it(which, cuts):
    """one cached entry of (layer 1, row 37) off by 1e-3: the check fails and its message names layer, row and K / V.  The entry is the row's
    smallest in magnitude: half a bf16 ulp of the entry comes off the distance, and for an entry of 0.5 that is 1e-3 itself -- a bf16 cache
    cannot tell such an error from a rounding (the last-row bounds are what is left for those)"""
    L = 65
    p = _p(L)
    probe = _oracle()
    probe.forward_generate(p, 0)
    k, v = probe.get_kv(1, 37, 1)
    t = np.abs((k if which == "K" else v)[0])
    head, dim = np.unravel_index(int(np.argmin(t)), t.shape)
    assert t[head, dim] < 0.03  # half an ulp <= 6.2e-5, of the entry and of the entry + 1e-3
    rec = pf._forced_prefill(_OracleAsGpu((1, 37, int(head), int(dim), which, 1e-3)), _oracle(), p, cuts)
    x, l, r, w = pf._worst(rec)
    assert (l, r, w) == (1, 37, which) and 1e-3 - 2 * 6.2e-5 <= x <= 1e-3 + 6.2e-5
    assert np.nan_to_num(rec["excess"][0]).max() == 0.0
    with pytest.raises(AssertionError, match=f"the {which} row the prefill pass cached at layer 1, row 37 "):
        pf._check("planted", rec)
