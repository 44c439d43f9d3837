"""FireflyCodec::encode on the device, stage by stage, against the CPU oracle -- and bit for bit on clips where the oracle alone decides.

fs_selftest_codec_encode_stage (include/fishrt.h) runs the encoder as fs_codec_encode does and copies ONE intermediate tensor out: the
log-mel (stage -1) or the activation where the oracle records stage 0..6 (after each of the four backbone stages, after the final LayerNorm,
after each of the two downsample blocks).  All distances are max |a - b| over the tensor.

Log-mel against oracle.log_mel: both use the same table (test_codec_encoder_ops_gpu.py holds the two tables to one ulp), an f64 FFT and the
same ascending f32 chain; what differs is the f64 transform's rounding seen through one f32 store and the two logf.
    bound = 4 x measured, never above the suite's 5e-5:   measured 4.768e-07 (worst of the four tiny clips; full size the same), asserted 1.91e-06

Stages 0..6 against oracle.encode_mel(oracle.log_mel(pcm), stage = i): the bound of stage i is 4 x d_i, d_i = the distance between the f32
oracle and the independent float64-accumulating restatement committed in tests/golden/codec_enc_tiny.npz at that stage (two references of
the same tensor: their distance is what f32 evaluation order alone does to it), never above 4 x the suite's 2e-5.  d_i is computed on the
CPU (test_codec_encoder_ref_cpu.py recomputes it and holds it under the value written here):
    stage          0         1         2         3         4         5         6
    d_i            3.34e-06  2.57e-06  2.61e-06  3.19e-06  3.22e-06  2.21e-06  2.75e-06      (max |activation| 2.7 .. 3.6)
    bound 4 d_i    1.34e-05  1.03e-05  1.05e-05  1.28e-05  1.29e-05  8.9e-06   1.10e-05
    GPU measured   2.15e-06  2.38e-06  2.98e-06  3.11e-06  3.52e-06  2.26e-06  2.22e-06      (MI355X, worst of the four tiny clips; printed
                                                                                        by test_tiny_stages_vs_oracle)
The full-size handle (0.5 s clip; log-mel, stages 0, 4, 6) has no second reference; its bound is the cap itself, 4 x 2e-5 (channel sums 8 x
longer than the tiny codec's, on activations of the same magnitude).  Measured on an MI355X: 3.46e-06, 4.29e-06, 5.13e-06.

Strict clips: codec_enc_refs.STRICT_CLIPS lists _clip seeds found by a CPU search whose oracle rounding margin (encode_mel stage 7) is >=
1e-3 at EVERY index -- 250 x the largest stage distance above, so the oracle alone decides every index and the GPU must produce exactly the
oracle's codes: one-clip, batched and ragged calls, no exemption."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import fishrt
from oracle import oracle as orc

import codec_enc_refs as R
from test_codec_encode import G, SEED, _clip

D_I = R.STAGE_D
STAGE_CAP = 4 * 2e-5
STAGE_BOUND = tuple(min(4 * d, STAGE_CAP) for d in D_I)
LOGMEL_CAP = 5e-5
LOGMEL_MEASURED = 4.768e-07   # MI355X
LOGMEL_BOUND = min(4 * LOGMEL_MEASURED, LOGMEL_CAP)
TINY_DIMS = (16, 32, 48, 64, 64, 64, 64)
FULL_DIMS = (128, 256, 384, 512, 512, 512, 512)


@pytest.fixture(scope="module")
def otiny():
    return orc.OracleCodec(tiny=True).load_synthetic(SEED)


@pytest.fixture(scope="module")
def gtiny():
    return fishrt.FireflyCodec(0, channel_div=8).load_synthetic(SEED)


def _stage_frames(F, i):
    return F if i <= 4 else F // 2 if i == 5 else F // 4


def _oracle_stage(o, mel, i, dims):
    n = dims[i] * _stage_frames(mel.shape[1], i)
    return o.encode_mel(mel, stage=i, stage_size=n)[1]


def test_tiny_stages_vs_oracle(otiny, gtiny):
    clips = [("golden", G["pcm"])] + [(f"clip{n}", _clip(n, seed)) for n, seed in ((768 * 3, 1), (512 * 37 + 11, 2), (44100, 3))]
    worst_mel, worst = 0.0, [0.0] * 7
    for name, pcm in clips:
        mel = otiny.log_mel(pcm)
        gmel = gtiny.encode_stage(pcm, -1)
        assert gmel.shape == mel.shape == (160, R.n_frames(pcm.size)), name
        worst_mel = max(worst_mel, float(np.abs(gmel - mel).max()))
        for i in range(7):
            exp = _oracle_stage(otiny, mel, i, TINY_DIMS)
            got = gtiny.encode_stage(pcm, i)
            assert got.shape == exp.shape and np.isfinite(got).all(), (name, i)
            worst[i] = max(worst[i], float(np.abs(got - exp).max()))
    print(f"tiny log-mel: GPU - oracle {worst_mel:.3e} (bound {LOGMEL_BOUND:.3e})")
    print("tiny stages: GPU - oracle " + "  ".join(f"{v:.2e}" for v in worst) + " | bound " + "  ".join(f"{v:.2e}" for v in STAGE_BOUND))
    assert worst_mel <= LOGMEL_BOUND <= LOGMEL_CAP
    for i in range(7):
        assert worst[i] <= STAGE_BOUND[i], (i, worst[i], STAGE_BOUND[i])


def test_fullsize_stages_vs_oracle():
    o = orc.OracleCodec(tiny=False).load_synthetic(SEED)
    c = fishrt.FireflyCodec(0).load_synthetic(SEED)
    pcm = _clip(22050, 5)
    mel = o.log_mel(pcm)
    gmel = c.encode_stage(pcm, -1)
    dm = float(np.abs(gmel - mel).max())
    out = []
    for i in (0, 4, 6):
        exp = _oracle_stage(o, mel, i, FULL_DIMS)
        got = c.encode_stage(pcm, i)
        assert got.shape == exp.shape
        out.append(float(np.abs(got - exp).max()))
    print(f"full size: log-mel {dm:.3e} (bound {LOGMEL_BOUND:.3e}); stages 0, 4, 6: " + "  ".join(f"{v:.2e}" for v in out) + f" (bound {STAGE_CAP:.1e})")
    assert dm <= LOGMEL_BOUND
    assert max(out) <= STAGE_CAP


def test_tap_is_inert(gtiny):
    pcm = _clip(9000, 7)
    before = gtiny.encode(pcm[None, None])
    for stage in (-2, -1, 0, 3, 4, 5, 6):
        gtiny.encode_stage(pcm, stage)
        assert np.array_equal(gtiny.encode(pcm[None, None]), before), stage  # between tapped calls
    with pytest.raises(RuntimeError):
        gtiny.encode_stage(pcm, 7)
    with pytest.raises(RuntimeError):
        gtiny.encode_stage(np.zeros(100, np.float32), 0)  # a failed tapped call disarms the tap too
    assert np.array_equal(gtiny.encode(pcm[None, None]), before)
    assert np.array_equal(gtiny.encode_stage(pcm, 4), gtiny.encode_stage(pcm, 4))


def test_strict_clips_equal_the_oracle_everywhere(otiny, gtiny):
    assert len(R.STRICT_CLIPS) >= 4
    whole = [R.clip(9000, seed) for seed, _ in R.STRICT_CLIPS]
    assert np.array_equal(whole[0], _clip(9000, R.STRICT_CLIPS[0][0]))  # the encode suite's clip generator
    exp_whole = [otiny.encode(p) for p in whole]
    exp_prefix = [otiny.encode(p[:n]) for p, (_, n) in zip(whole, R.STRICT_CLIPS)]
    # one clip per call
    for p, e, (seed, n), ep in zip(whole, exp_whole, R.STRICT_CLIPS, exp_prefix):
        assert np.array_equal(gtiny.encode(p[None, None])[0], e), seed
        assert np.array_equal(gtiny.encode(np.ascontiguousarray(p[None, None, :n]))[0], ep), (seed, n)
    # batched
    batch = np.ascontiguousarray(np.stack(whole)[:, None, :])
    got = gtiny.encode(batch)
    for i, e in enumerate(exp_whole):
        assert np.array_equal(got[i], e), i
    # ragged: zero-padded rows with lengths=
    rag = gtiny.encode(batch, lengths=[n for _, n in R.STRICT_CLIPS])
    for i, e in enumerate(exp_prefix):
        assert np.array_equal(rag[i], e), i
