"""GPU: device sample-rate conversion behind the codec (fs_codec_decode_pcm, fs_codec_streams_open_pcm / _pending / _decode_pcm,
fs_codec_encode_pcm) on a full-size synthetic codec, in both matrix-core precision modes.  One-shot: decode(sample_rate=) is
fishrt.resample of decode(), bit for bit.  Streams: per stream, the outputs of all its calls concatenated equal the one-shot result with
np.array_equal -- in both modes and both formats, whatever the chunk lengths, the other items of a call or their order, and after
rejected calls.  Encode: encode(sample_rate=) gives the codes of encode() on the resampled, downmixed clip.  End to end:
fishrt.SessionStreamer(ragged=True, sample_rate=24000, pcm_dtype="s16")."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import fishrt
from fishrt import _ffi
from fishrt import config as fcfg

G = os.path.join(os.path.dirname(__file__), "golden")
C = _ffi.C

SPECS = [dict(sample_rate=24000, resample="sinc", dtype="s16"), dict(sample_rate=48000, resample="sinc", dtype="f32"),
         dict(sample_rate=16000, resample="linear", dtype="f32"), dict(sample_rate=44100, resample="linear", dtype="s16"), None]
LENGTHS = [1, 13, 40, 77, 120]


def _voice():
    return np.ascontiguousarray(np.load(os.path.join(G, "default_voice_codes.npy")).astype(np.uint32))  # (8, 274)


def _one_shot(c, seq, spec):
    return c.decode(seq[None], **spec)[0, 0] if spec else c.decode(seq[None])[0, 0]


@pytest.fixture(scope="module", params=["f16", "bf16x3"])
def codec(request):
    c = fishrt.FireflyCodec(0, precision=request.param).load_synthetic(0xC0DEC)
    yield c
    c.close()


def test_one_shot_decode_equals_resample_of_decode(codec):
    rng = np.random.RandomState(2)
    codes = np.stack([np.ascontiguousarray(_voice()[:, 50:71]), rng.randint(0, 1000, (8, 21)).astype(np.uint32)])
    pcm = codec.decode(codes)
    for mode in ("linear", "sinc"):
        for dtype in ("f32", "s16"):
            got = codec.decode(codes, sample_rate=24000, resample=mode, dtype=dtype)
            ref = fishrt.resample(pcm[:, 0], 44100, 24000, mode=mode, dtype=dtype)
            assert got.shape == (2, 1, ref.shape[1]) and got.dtype == ref.dtype
            assert np.array_equal(got[:, 0], ref), (mode, dtype)
    same = codec.decode(codes, sample_rate=44100, dtype="s16")  # the codec's own rate: a format conversion only
    assert np.array_equal(same[:, 0], fishrt.wav.pcm_to_i16(pcm[:, 0]))


def _cut(rng, total, lo, hi):
    out = []
    while total > 0:
        t = min(int(rng.randint(lo, hi + 1)), total)
        out.append(t)
        total -= t
    return out


def test_streams_equal_one_shot_bit_for_bit(codec):
    c = codec
    rng, voice = np.random.RandomState(17), _voice()
    seqs = [rng.randint(0, 1000, (8, L)).astype(np.uint32) for L in LENGTHS]
    seqs[3] = np.ascontiguousarray(voice[:, 100:177])
    refs = [_one_shot(c, s, spec) for s, spec in zip(seqs, SPECS)]
    # stream 0: one frame at a time (a single one); stream 1: only 1 .. 3 frame chunks; stream 2: flushed by a T = 0 final item
    chunks = [[1], _cut(rng, 13, 1, 3), _cut(rng, 40, 1, 30), _cut(rng, 77, 1, 40), [1] * 120]
    # (stream 4, plain, takes the one-frame-at-a-time role over 120 frames as well)
    flush_alone = [False, False, True, False, True]
    sid = [c.streams_open(**spec) if spec else c.streams_open() for spec in SPECS]
    nxt, pos, parts, done = [0] * 5, [0] * 5, [[] for _ in seqs], [False] * 5
    calls = 0
    while not all(done):
        live = [i for i in range(5) if not done[i]]
        pick = [i for i in live if rng.rand() < 0.6] or live[:1]
        rng.shuffle(pick)
        items, final = [], []
        for i in pick:
            if nxt[i] == len(chunks[i]):  # all frames fed: the pure flush
                T, fin = 0, True
            else:
                T = chunks[i][nxt[i]]
                fin = nxt[i] == len(chunks[i]) - 1 and not flush_alone[i]
            items.append(np.ascontiguousarray(seqs[i][:, pos[i]:pos[i] + T]))
            final.append(fin)
        want = [c.streams_pending(sid[i], it.shape[1], f) for i, it, f in zip(pick, items, final)]
        out = c.streams_decode_ragged([sid[i] for i in pick], items, final=final)
        calls += 1
        for k, i in enumerate(pick):
            assert out[k].shape == (want[k],), (i, out[k].shape, want[k])
            parts[i].append(out[k])
            pos[i] += items[k].shape[1]
            nxt[i] += items[k].shape[1] > 0
            done[i] = final[k]
        assert calls < 1000
    for i, ref in enumerate(refs):
        got = np.concatenate(parts[i])
        assert got.dtype == ref.dtype and got.shape == ref.shape, (i, got.shape, ref.shape)
        assert np.array_equal(got, ref), (i, SPECS[i], int(np.argmax(got != ref)))
    # sinc pieces vary in length: whole blocks of p outputs only, until the flush
    assert len({p.shape[0] for p in parts[1]}) > 1 and all(p.shape[0] % 80 == 0 for p in parts[0][:-1] + parts[1][:-1])
    for s in sid:
        c.streams_close(s)


def _raw_pcm(c, ids, T, final, codes, cap_bytes):
    ids, T, final = np.asarray(ids, np.int32), np.asarray(T, np.int32), np.asarray(final, np.uint8)
    codes = np.ascontiguousarray(np.concatenate([np.asarray(codes, np.uint32).reshape(-1), np.zeros(1, np.uint32)]))
    buf = np.zeros(max(cap_bytes, 8), np.uint8)
    n_out = (C.c_int64 * len(ids))()
    return _ffi.lib().fs_codec_streams_decode_pcm(c._h, len(ids), ids.ctypes.data_as(C.POINTER(C.c_int)), T.ctypes.data_as(C.POINTER(C.c_int)),
                                                  final.ctypes.data_as(C.POINTER(C.c_uint8)), codes.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                  buf.ctypes.data_as(C.c_void_p), C.c_size_t(cap_bytes), n_out)


def test_rejected_calls_leave_every_stream_untouched(codec):
    c = codec
    voice = np.ascontiguousarray(_voice()[:, :40])
    other = np.random.RandomState(9).randint(0, 1000, (8, 40)).astype(np.uint32)
    sv, so = dict(sample_rate=24000, resample="sinc", dtype="s16"), dict(sample_rate=16000, resample="linear", dtype="f32")
    ref_v, ref_o = _one_shot(c, voice, sv), _one_shot(c, other, so)
    s, t = c.streams_open(**sv), c.streams_open(**so)
    gone = c.streams_open(**sv)
    pv, po, at = [], [], [0, 0]

    def good(nv, no, fv=False, fo=False):
        out = c.streams_decode_ragged([t, s], [other[:, at[1]:at[1] + no], voice[:, at[0]:at[0] + nv]], final=[fo, fv])
        po.append(out[0])
        pv.append(out[1])
        at[0] += nv
        at[1] += no

    good(3, 11)
    c.streams_decode_ragged([gone], [voice[:, :2]], final=[True])  # `gone` is flushed now
    two = np.concatenate([voice[:, 3:8].reshape(-1), other[:, 11:20].reshape(-1)])
    need = 2 * c.streams_pending(s, 5) + 4 * c.streams_pending(t, 9)
    assert need > 8
    last_err = lambda: _ffi.lib().fs_last_error().decode()
    for ids, T, final, codes, cap, msg in (([s, t], [5, 9], [0, 0], two, need - 1, "cap_bytes"),
                                           ([s, gone], [5, 9], [0, 0], two, 1 << 22, "already flushed"),
                                           ([s, t], [5, 0], [0, 0], two, 1 << 22, "must be final"),
                                           ([s, s], [5, 9], [0, 0], two, 1 << 22, "twice")):
        assert _raw_pcm(c, ids, T, final, codes, cap) != 0, msg
        assert msg in last_err(), (msg, last_err())
    with pytest.raises(RuntimeError, match="fs_codec_streams_decode_pcm"):  # a spec stream in the old ragged call
        c._stream_dtype.pop(s)  # (the wrapper would route the call to the new one: go through the old one as an old client would)
        try:
            c.streams_decode_ragged([s], [voice[:, 3:8]])
        finally:
            c._stream_dtype[s] = "s16"
    with pytest.raises(RuntimeError, match="fs_codec_streams_decode_pcm"):
        c.streams_decode([s], np.ascontiguousarray(voice[None, :, 3:19]))
    good(5, 9)
    good(1, 20, fo=True)
    good_rest = c.streams_decode_ragged([s], [voice[:, at[0]:]], final=[True])
    pv.append(good_rest[0])
    assert np.array_equal(np.concatenate(pv), ref_v) and np.array_equal(np.concatenate(po), ref_o)
    for i in (s, t, gone):
        c.streams_close(i)


def test_plain_streams_through_the_old_calls_stay_bit_identical(codec):
    c = codec
    seq = np.ascontiguousarray(_voice()[:, 10:70])
    ref = c.decode(seq[None])[0, 0]
    a, b = c.streams_open(), c.streams_open()
    pa = [c.streams_decode_ragged([a], [seq[:, lo:hi]])[0].copy() for lo, hi in ((0, 1), (1, 20), (20, 60))]
    pb = [c.streams_decode([b], np.ascontiguousarray(seq[None, :, lo:hi]))[0].copy() for lo, hi in ((0, 16), (16, 60))]
    assert np.array_equal(np.concatenate(pa), ref) and np.array_equal(np.concatenate(pb), ref)
    c.streams_close(a)
    c.streams_close(b)


# numpy restatements of the reference's downmix (encode_speech.rs:51-53) and resample (audio/functional.rs:3-37)
def _downmix_ref(x):  # (channels, n) -> (n,)
    s = x[0].copy()
    for ch in x[1:]:
        s = s + ch
    return s / np.float32(x.shape[0])


def _linear_ref(x, frm, to):
    n = x.shape[0]
    ratio = np.float64(to) / np.float64(frm)
    out_len = int(np.ceil(np.float64(n) * ratio))
    idx = np.arange(out_len, dtype=np.float64) / ratio
    fl = np.floor(idx)
    c = np.minimum(np.ceil(idx).astype(np.int64), n - 1)
    t = (idx - fl).astype(np.float32)
    f = np.minimum(fl.astype(np.int64), n - 1)  # (fishrt.h: the floor index is clamped like the ceil index)
    return x[f] * (np.float32(1.0) - t) + x[c] * t


def test_encode_from_another_rate_and_channel_count():
    c = fishrt.FireflyCodec(0).load_synthetic(0xC0DEC)
    rng = np.random.RandomState(12)
    t = np.arange(22050, dtype=np.float64) / 22050.0
    stereo = np.stack([0.4 * np.sin(2 * np.pi * 220.0 * t) + 0.05 * rng.randn(22050), 0.3 * np.sin(2 * np.pi * 331.0 * t) + 0.05 * rng.randn(22050)])
    stereo = np.ascontiguousarray(stereo.astype(np.float32))
    t = np.arange(47000, dtype=np.float64) / 48000.0
    mono = np.ascontiguousarray((0.5 * np.sin(2 * np.pi * 440.0 * t * (1 + t)) + 0.02 * rng.randn(47000)).astype(np.float32))[None]
    for clip, sr in ((stereo, 22050), (mono, 48000)):
        mixed = _downmix_ref(clip)
        lin = np.ascontiguousarray(_linear_ref(mixed, sr, 44100))
        got = c.encode(clip[None], sample_rate=sr, resample="linear")
        ref = c.encode(lin[None, None])
        assert got.shape == ref.shape and got.shape[1] == 8 and got.shape[2] >= 18, (sr, got.shape, ref.shape)
        assert np.array_equal(got, ref), (sr, "linear", int((got != ref).sum()))
        snc = fishrt.resample(mixed, sr, 44100, mode="sinc")
        got = c.encode(clip[None], sample_rate=sr, resample="sinc")
        ref = c.encode(np.ascontiguousarray(snc[None, None]))
        assert np.array_equal(got, ref), (sr, "sinc", int((got != ref).sum()))
    c.close()


class _CodesBelow1000:
    """the synthetic LM samples from its 1024 codebook entries, the codec's FSQ has 1000: fold its codes into range"""

    def __init__(self, s):
        self.s = s

    def add(self, p, n):
        return self.s.add(p, n)

    def step(self, k):
        return self.s.step(k)

    def release(self, slot):
        return self.s.release(slot)

    def poll(self, slot, codes=True):
        r = self.s.poll(slot, codes)
        return (r[0] % 1000, r[1]) if codes else r


def test_session_streamer_delivers_24k_s16():
    cfg, tok = fcfg.TINY, fcfg.TINY_TOKENS
    lm = fishrt.DualARTransformer(cfg, tok, 0, "bf16", max_batch=3).load_synthetic(0xF15E5EED)
    rng = np.random.RandomState(3)
    Ls, Fs = (12, 7, 9), (37, 16, 1)  # the second finishes on a chunk boundary (1 + 5 + 5 + 5): its flush item has no frames left
    prompts = []
    for L in Ls:
        p = np.zeros((9, L), np.uint32)
        p[0] = rng.randint(0, min(tok["semantic_start_id"], 400), L)
        prompts.append(p)
    codec = fishrt.FireflyCodec(0).load_synthetic(0xC0DEC)
    pcm, finals = {i: [] for i in range(3)}, []
    with lm.session(temp=0.0, top_p=1.0, top_k=0, seed=42, ignore_eos=True) as raw:
        ss = fishrt.SessionStreamer(_CodesBelow1000(raw), codec, chunk=5, first_chunk=1, ragged=True, sample_rate=24000, pcm_dtype="s16",
                                    on_audio=lambda tag, p, final: (pcm[tag].append(p.copy()), final and finals.append(tag)))
        for i in range(3):
            assert ss.add(prompts[i], Ls[i] + Fs[i], tag=i) is not None
        step = 0
        while len(ss.results) < 3:
            ss.step(5)
            step += 1
            assert step < 200
    assert sorted(finals) == [0, 1, 2]
    for i in range(3):
        ref = codec.decode(np.ascontiguousarray(ss.results[i][None]), sample_rate=24000, resample="sinc", dtype="s16")[0, 0]
        got = np.concatenate(pcm[i])
        assert got.dtype == np.int16 and got.shape == ref.shape, (i, got.shape, ref.shape)
        assert np.array_equal(got, ref), i
        assert ss.stats[i]["samples"] == ref.shape[0] and ss.stats[i]["frames"] == ss.results[i].shape[1]
    assert len({p.shape[0] for p in pcm[0]}) > 2  # pieces vary in length
    codec.close()
