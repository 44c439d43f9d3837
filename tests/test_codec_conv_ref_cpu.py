"""CPU anchor of tests/test_codec_conv_variants_gpu.py: its float64 reference (causal conv with left zero pad (K-1)*dil, transposed conv
with right trim K - stride, the per-sample sum of |w x|, the plane-format rounding) against torch.nn.functional in float64.
Bound: two float64 sums of n = Cin*K terms taken in different orders differ by at most 2 * n * 2^-53 * sum|w x| (each partial sum is below
sum|w x| and each addition rounds once); the comparison allows exactly that."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_codec_conv_variants_gpu import bf16_rne, f16_rne, plane_round, ref_conv, ref_tconv

KS, DILS, STRIDES = (1, 2, 3, 7, 11, 13), (1, 3, 5), (2, 8)


def _close(a, b, S, n):
    assert a.shape == b.shape
    return bool(np.all(np.abs(a - b) <= 2 * n * 2.0 ** -53 * S + 1e-300))


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("dil", DILS)
def test_causal_conv_reference_vs_torch(K, dil):
    rng = np.random.RandomState(100 * K + dil)
    for B, Cin, Cout, T in ((1, 5, 7, 1), (3, 24, 20, (K - 1) * dil + 1), (2, 16, 33, 301)):
        x, w = rng.standard_normal((B, Cin, T)), rng.standard_normal((Cout, Cin, K))
        y, S = ref_conv(x, w, dil)
        halo = (K - 1) * dil
        t = F.conv1d(F.pad(torch.from_numpy(x), (halo, 0)), torch.from_numpy(w), dilation=dil).numpy()
        ts = F.conv1d(F.pad(torch.from_numpy(np.abs(x)), (halo, 0)), torch.from_numpy(np.abs(w)), dilation=dil).numpy()
        assert _close(y, t, S, Cin * K) and _close(S, ts, S, Cin * K)
        # causal: sample t does not see x behind t, and the first sample sees only the last tap
        assert _close(y[:, :, 0], np.einsum("oi,bi->bo", w[:, :, K - 1], x[:, :, 0]), S[:, :, 0], Cin * K)
        if T > 1:
            y2, _ = ref_conv(x[:, :, :T - 1], w, dil)
            assert _close(y2, y[:, :, :T - 1], S[:, :, :T - 1], Cin * K)


@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("taps", (1, 2, 3, 7, 11))
def test_transposed_conv_reference_vs_torch(stride, taps):
    K = taps * stride  # the kernels' polyphase form needs K % stride == 0
    rng = np.random.RandomState(1000 * stride + taps)
    for B, Cin, Cout, T in ((1, 3, 2, 1), (3, 16, 5, 37)):
        x, w = rng.standard_normal((B, Cin, T)), rng.standard_normal((Cin, Cout, K))
        y, S = ref_tconv(x, w, stride)
        t = F.conv_transpose1d(torch.from_numpy(x), torch.from_numpy(w), stride=stride).numpy()
        assert t.shape[2] == (T - 1) * stride + K and y.shape == (B, Cout, T * stride)
        assert _close(y, t[:, :, :T * stride], S, Cin * taps)  # right trim K - stride (utils/mod.rs:110-122)


@pytest.mark.parametrize("K", (13, 16))
def test_transposed_conv_reference_any_kernel_size(K):
    rng = np.random.RandomState(K)
    x, w = rng.standard_normal((2, 4, 9)), rng.standard_normal((4, 3, K))
    y, S = ref_tconv(x, w, 8)
    t = F.conv_transpose1d(torch.from_numpy(x), torch.from_numpy(w), stride=8).numpy()
    assert _close(y, t[:, :, :72], S, 4 * K)


def test_plane_format_rounding():
    rng = np.random.RandomState(3)
    v = np.concatenate([rng.standard_normal(4000) * 10.0 ** rng.randint(-6, 5, 4000), [0.0, 65504.0, 65520.0, 7e4, -1e9, 2.0 ** -24, 2.0 ** -25, 3e-8]]).astype(np.float32)
    assert np.array_equal(bf16_rne(v), torch.from_numpy(v).to(torch.bfloat16).to(torch.float32).numpy())
    tf16 = torch.from_numpy(v).clamp(-65504.0, 65504.0).to(torch.float16).to(torch.float32).numpy()
    assert np.array_equal(plane_round(v, 2), tf16) and np.array_equal(f16_rne(v), tf16.astype(np.float64))
    p = plane_round(v, 1).astype(np.float64)
    assert np.all(np.abs(p - v) <= 2.0 ** -17 * np.abs(v))  # hi + lo keeps 16 bits
