"""GPU: the stand-alone device resampler (fs_resample, csrc/codec_resample.hip), no codec.  The referees are numpy restatements of the two
definitions of include/fishrt.h written here: linear in the reference's exact dtype sequence (audio/functional.rs:3-37) and compared with
np.array_equal; sinc with f64 taps and f64 sums, compared per output sample against
    |y - ref| <= (K + 3) * 2^-24 * sum_k |h[j][k] * x_k| + 1e-30
which bounds the f32 accumulation of K terms (K * 2^-24 relative to the sum of magnitudes) plus the f32 rounding of each tap, of each
product's use in the FMA chain and of the output -- derived, not tuned.  Measured on an MI355X (printed by the test, per rate pair): the
worst sample sits at 0.26 of that bound for the 15-tap pairs, at 0.01 .. 0.05 for the others.  s16 output is fishrt.wav.pcm_to_i16 of the same call's f32 output, exactly."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import fishrt
from fishrt.wav import pcm_to_i16

PAIRS = [(44100, 24000), (44100, 48000), (44100, 16000), (22050, 44100), (48000, 44100), (8000, 44100), (44100, 44100)]
LENGTHS = [1, 2, 147, 148, 4096, 44100 + 7]
W, ROLLOFF = 6, 0.99


def _noise(n, seed=5):
    return np.random.RandomState(seed).uniform(-1.0, 1.0, n).astype(np.float32)


def _tone(n, rate):
    return np.sin(2.0 * np.pi * 19845.0 * np.arange(n, dtype=np.float64) / rate).astype(np.float32)


def linear_ref(x, frm, to):
    n = x.shape[0]
    ratio = np.float64(to) / np.float64(frm)
    out_len = int(np.ceil(np.float64(n) * ratio))
    idx = np.arange(out_len, dtype=np.float64) / ratio
    fl = np.floor(idx)
    # f64 rounding can make the last floor index n (n = 147 at 44.1 -> 24 kHz: out_len = ceil(80.00000000000001) = 81 and idx(80) = 147.0).
    # The reference's gather is out of range there and it returns an error; fishrt.h clamps the floor index like the ceil index, t stays
    # idx - floor(idx) = 0, so the extra sample repeats x[n - 1]
    f = np.minimum(fl.astype(np.int64), n - 1)
    c = np.minimum(np.ceil(idx).astype(np.int64), n - 1)
    t = (idx - fl).astype(np.float32)
    u = np.float32(1.0) - t
    return x[f] * u + x[c] * t  # f32 arrays: two products rounded separately, one add


def sinc_params(frm, to):
    g = math.gcd(frm, to)
    o, p = frm // g, to // g
    base = min(o, p) * ROLLOFF
    width = int(math.ceil(W * o / base))
    return o, p, base, width, 2 * width + o


def sinc_taps64(frm, to):
    o, p, base, width, K = sinc_params(frm, to)
    j = np.arange(p, dtype=np.float64)[:, None]
    k = np.arange(K, dtype=np.float64)[None, :]
    t = np.clip((-j / p + (k - width) / o) * base, -W, W)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(t == 0.0, 1.0, np.sin(np.pi * t) / (np.pi * t))
    return s * np.cos(np.pi * t / (2 * W)) ** 2 * (base / o)


def sinc_ref(x, frm, to):
    """-> (f64 output, per-sample sum_k |h x|)"""
    o, p, _, width, K = sinc_params(frm, to)
    n = x.shape[0]
    out_len = (p * n + o - 1) // o
    h = sinc_taps64(frm, to)
    xp = np.concatenate([np.zeros(width), x.astype(np.float64), np.zeros(K + o)])
    y, mag = np.empty(out_len), np.empty(out_len)
    ar = np.arange(K)
    for lo in range(0, out_len, 8192):
        q = np.arange(lo, min(out_len, lo + 8192))
        win = xp[(q // p)[:, None] * o + ar[None, :]]
        prod = h[q % p] * win
        y[lo:lo + q.shape[0]] = prod.sum(axis=1)
        mag[lo:lo + q.shape[0]] = np.abs(prod).sum(axis=1)
    return y, mag


def _rows(frm):
    """the six lengths x {noise, tone} as four calls of b = 3 rows of different lengths"""
    sig = {"noise": lambda n: _noise(n, 5 + n % 7), "tone": lambda n: _tone(n, frm)}
    calls = []
    for kinds, lens in ((("noise", "tone", "noise"), (1, 147, 44107)), (("tone", "noise", "tone"), (2, 148, 4096)),
                        (("tone", "noise", "tone"), (44107, 1, 147)), (("noise", "tone", "noise"), (4096, 2, 148))):
        calls.append([sig[k](n) for k, n in zip(kinds, lens)])
    assert sorted({r.shape[0] for c in calls for r in c}) == LENGTHS
    return calls


def _call(rows, frm, to, mode, dtype="f32"):
    n = max(r.shape[0] for r in rows)
    x = np.zeros((len(rows), n), np.float32)
    for i, r in enumerate(rows):
        x[i, : r.shape[0]] = r
    return fishrt.resample(x, frm, to, mode=mode, dtype=dtype, lengths=[r.shape[0] for r in rows])


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_linear_equals_the_reference_arithmetic_bit_for_bit(pair):
    frm, to = pair
    for rows in _rows(frm):
        got = _call(rows, frm, to, "linear")
        for r, y in zip(rows, got):
            ref = linear_ref(r, frm, to)
            assert y.dtype == np.float32 and y.shape == ref.shape, (pair, r.shape, y.shape, ref.shape)
            assert fishrt.resample_out_len(r.shape[0], frm, to, "linear") == ref.shape[0]
            assert np.array_equal(y, ref), (pair, r.shape[0], float(np.abs(y - ref).max()))
            if frm == to:
                assert np.array_equal(y, r)


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_sinc_is_within_the_f32_accumulation_bound_of_the_f64_definition(pair):
    frm, to = pair
    K = sinc_params(frm, to)[4]
    worst = 0.0
    for rows in _rows(frm):
        got = _call(rows, frm, to, "sinc")
        for r, y in zip(rows, got):
            ref, mag = sinc_ref(r, frm, to)
            assert y.dtype == np.float32 and y.shape == ref.shape, (pair, r.shape, y.shape, ref.shape)
            assert fishrt.resample_out_len(r.shape[0], frm, to, "sinc") == ref.shape[0]
            bound = (K + 3) * 2.0 ** -24 * mag + 1e-30
            err = np.abs(y.astype(np.float64) - ref)
            worst = max(worst, float((err / bound).max()))
            bad = int(np.argmax(err - bound))
            assert (err <= bound).all(), (pair, r.shape[0], bad, float(err[bad]), float(bound[bad]))
    print(f"sinc {frm} -> {to}: K = {K}, worst |y - ref| / bound = {worst:.4f}")


@pytest.mark.parametrize("case", [(44100, 24000, "sinc"), (44100, 44100, "linear"), (22050, 44100, "linear"), (44100, 16000, "linear")],
                         ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}")
def test_s16_is_pcm_to_i16_of_the_f32_output(case):
    frm, to, mode = case
    x = _noise(5000, 11) * np.float32(1.6)  # a good part outside [-1, 1]
    x[100:104] = [1.0, -1.0, 1.0, -1.0]
    x[200:204] = np.nan  # (a run: a 2.76 : 1 linear downsampling steps over single samples)
    x[210:212] = [3.5, -7.0]
    x[300:310] = 1.0  # a run, so that the interpolated outputs hit +-1 exactly too
    x[320:330] = -1.0
    f = fishrt.resample(x, frm, to, mode=mode, dtype="f32")
    s = fishrt.resample(x, frm, to, mode=mode, dtype="s16")
    assert s.dtype == np.int16 and s.shape == f.shape
    nan = np.isnan(f)
    assert nan.any() and (s[nan] == 0).all()
    assert np.array_equal(s, pcm_to_i16(np.where(nan, np.float32(0.0), f)))
    assert (np.abs(f[~nan]) > 1.0).any() and (s == 32767).any() and (s == -32767).any()
    if mode == "linear" and to % frm == 0:  # t is 0 or 0.5 here: the interpolation inside a run of +-1 is exact
        assert (f == 1.0).any() and (f == -1.0).any()


def test_sinc_removes_the_alias_the_linear_mode_keeps():
    frm, to = 44100, 24000
    x = _tone(44107, frm)  # 19 845 Hz: above the 12 kHz the output can carry
    ys, yl = fishrt.resample(x, frm, to, mode="sinc"), fishrt.resample(x, frm, to, mode="linear")
    ref, _ = sinc_ref(x, frm, to)
    rms = lambda v: float(np.sqrt(np.mean(np.asarray(v, np.float64)[200:-200] ** 2)))
    print(f"19845 Hz tone 44.1 -> 24 kHz: sinc RMS {rms(ys):.3e} (f64 referee {rms(ref):.3e}), linear RMS {rms(yl):.3f}")
    assert rms(ys) <= 2.0 * rms(ref)
    assert np.array_equal(yl, linear_ref(x, frm, to))


def test_an_empty_row_and_single_rows():
    frm, to = 44100, 24000
    a, b = _noise(300, 2), _noise(159, 3)
    for mode in ("linear", "sinc"):
        got = _call([a, np.zeros(0, np.float32), b], frm, to, mode)
        assert got[1].shape == (0,)
        assert np.array_equal(got[0], fishrt.resample(a, frm, to, mode=mode))
        assert np.array_equal(got[2], fishrt.resample(b, frm, to, mode=mode))


def test_an_oversize_rate_pair_is_refused():
    with pytest.raises(RuntimeError, match="44100 -> 44101"):
        fishrt.resample(_noise(64), 44100, 44101, mode="sinc")
    assert fishrt.resample(_noise(64), 44100, 44101, mode="linear").shape == (65,)
    with pytest.raises(ValueError):
        fishrt.resample(_noise(64), 44100, 24000, mode="cubic")
