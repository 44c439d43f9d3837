"""GPU: the `speed` of a request in codec multi-streams (fs_codec_streams_open_speed; the stretch stage of fs_codec_streams_decode_pcm) on
a full-size synthetic codec.  Per stream, the outputs of all its calls concatenated equal fs_codec_decode_speed of the whole sequence at
b = 1 with np.array_equal -- for every split of 33 frames listed below, three speeds and three PCM specs, beside streams of other speeds and
kinds in either item order, and after a rejected call.  fs_codec_streams_pending counts through both stages; speed 1.0 is a PCM stream;
the old multi-stream calls refuse a speed stream.  End to end: fishrt.SessionStreamer(ragged=True) with a speed per request."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import fishrt
from fishrt import _ffi
from fishrt import config as fcfg

C = _ffi.C
T_TOTAL = 33
SPLITS = [[33], [16, 17], [1, 1, 2, 5, 8, 16], [8, 8, 8, 9, 0]]  # (the last one ends in a pure flush)
SPEEDS = (0.5, 1.25, 4.0)
SPECS = [None, dict(sample_rate=24000, resample="sinc", dtype="s16"), dict(sample_rate=16000, resample="linear", dtype="f32")]


@pytest.fixture(scope="module")
def codec():
    c = fishrt.FireflyCodec(0).load_synthetic(0xC0DEC)
    yield c
    c.close()


@pytest.fixture(scope="module")
def seq():
    return np.random.RandomState(33).randint(0, 1000, (8, T_TOTAL)).astype(np.uint32)


_refs = {}


def _ref(c, s, speed, spec):
    """fs_codec_decode_speed (speed None: fs_codec_decode_pcm / fs_codec_decode) of the whole sequence, computed once per key"""
    key = (s.tobytes(), speed, None if spec is None else tuple(sorted(spec.items())))
    if key not in _refs:
        kw = dict(spec or {})
        if speed is not None:
            kw["speed"] = speed
        _refs[key] = c.decode(np.ascontiguousarray(s[None]), **kw)[0, 0].copy()
    return _refs[key]


def _feed(c, sid, s, split):
    """one stream through streams_decode_ragged, item by item -> its pieces; every piece has the length streams_pending announced"""
    parts, at = [], 0
    for i, T in enumerate(split):
        fin = i + 1 == len(split)
        want = c.streams_pending(sid, T, fin)
        out = c.streams_decode_ragged([sid], [np.ascontiguousarray(s[:, at:at + T])], final=[fin])[0]
        assert out.shape == (want,), (split, i, out.shape, want)
        parts.append(out)
        at += T
    return parts


@pytest.mark.parametrize("spec", SPECS, ids=["codec-rate-f32", "24k-sinc-s16", "16k-linear-f32"])
def test_every_split_equals_one_shot_decode_speed(codec, seq, spec):
    c = codec
    for speed in SPEEDS:
        ref = _ref(c, seq, speed, spec)
        for split in SPLITS:
            sid = c.streams_open(speed=speed, **(spec or {}))
            got = np.concatenate(_feed(c, sid, seq, split))
            c.streams_close(sid)
            assert got.dtype == ref.dtype and got.shape == ref.shape, (speed, split, got.shape, ref.shape)
            assert np.array_equal(got, ref), (speed, split, int(np.argmax(got != ref)))


@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_streams_of_different_speeds_and_kinds_share_a_call(codec, seq, order):
    c = codec
    rng = np.random.RandomState(5)
    seqs = [seq, np.ascontiguousarray(seq[:, ::-1]), rng.randint(0, 1000, (8, 21)).astype(np.uint32), np.ascontiguousarray(seq[:, 3:30]),
            rng.randint(0, 1000, (8, 26)).astype(np.uint32)]
    kinds = [(0.5, SPECS[1]), (1.25, None), (4.0, SPECS[2]), (None, SPECS[1]), (None, None)]  # three speed streams, a PCM stream, a plain one
    splits = [[16, 17, 0], [1, 1, 2, 5, 8, 16], [8, 13], [5, 9, 13], [13, 13]]
    sids = [c.streams_open(**dict(spec or {}, **({} if speed is None else dict(speed=speed)))) for speed, spec in kinds]
    parts, at, nxt = [[] for _ in seqs], [0] * 5, [0] * 5
    while any(nxt[i] < len(splits[i]) for i in range(5)):
        live = [i for i in range(5) if nxt[i] < len(splits[i])]
        if order == "reversed":
            live = live[::-1]
        items = [np.ascontiguousarray(seqs[i][:, at[i]:at[i] + splits[i][nxt[i]]]) for i in live]
        final = [nxt[i] + 1 == len(splits[i]) for i in live]
        want = [c.streams_pending(sids[i], it.shape[1], f) for i, it, f in zip(live, items, final)]
        out = c.streams_decode_ragged([sids[i] for i in live], items, final=final)
        for j, i in enumerate(live):
            assert out[j].shape == (want[j],), (i, out[j].shape, want[j])
            parts[i].append(out[j])
            at[i] += items[j].shape[1]
            nxt[i] += 1
    for i, (speed, spec) in enumerate(kinds):
        ref, got = _ref(c, seqs[i], speed, spec), np.concatenate(parts[i])
        assert got.dtype == ref.dtype and np.array_equal(got, ref), (order, i, got.shape, ref.shape)
    for s in sids:
        c.streams_close(s)


def test_speed_one_is_a_pcm_stream(codec, seq):
    c = codec
    for spec in SPECS:
        a, b = c.streams_open(speed=1.0, **(spec or {})), c.streams_open(**(spec or {}))
        pa, pb = _feed(c, a, seq, SPLITS[2]), _feed(c, b, seq, SPLITS[2])
        assert len(pa) == len(pb) and all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(pa, pb)), spec
        c.streams_close(a)
        c.streams_close(b)
    # ... and at the codec's rate in f32 it is a plain stream, which the old calls take
    a = c.streams_open(speed=1.0)
    c._dtypes().pop(a)
    assert np.array_equal(c.streams_decode_ragged([a], [seq])[0], c.decode(seq[None])[0, 0])
    c.streams_close(a)


def _raw_pcm(c, ids, T, final, codes, cap_bytes):
    ids, T, final = np.asarray(ids, np.int32), np.asarray(T, np.int32), np.asarray(final, np.uint8)
    codes = np.ascontiguousarray(np.concatenate([np.asarray(codes, np.uint32).reshape(-1), np.zeros(1, np.uint32)]))
    buf = np.zeros(max(cap_bytes, 8), np.uint8)
    n_out = (C.c_int64 * len(ids))()
    return _ffi.lib().fs_codec_streams_decode_pcm(c._h, len(ids), ids.ctypes.data_as(C.POINTER(C.c_int)), T.ctypes.data_as(C.POINTER(C.c_int)),
                                                  final.ctypes.data_as(C.POINTER(C.c_uint8)), codes.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                  buf.ctypes.data_as(C.c_void_p), C.c_size_t(cap_bytes), n_out)


def test_rejected_calls_leave_a_speed_stream_untouched(codec, seq):
    c = codec
    spec = SPECS[1]
    ref = _ref(c, seq, 1.25, spec)
    s = c.streams_open(speed=1.25, **spec)
    last_err = lambda: _ffi.lib().fs_last_error().decode()
    parts, at = [], 0
    for T, fin in ((8, False), (8, False), (8, False), (9, True)):
        need = 2 * c.streams_pending(s, T, fin)
        assert need > 2
        # one sample short: refused, names cap_bytes, and the retried call yields the bits of an undisturbed run
        assert _raw_pcm(c, [s], [T], [fin], seq[:, at:at + T], need - 2) != 0
        assert "cap_bytes" in last_err(), last_err()
        assert c.streams_pending(s, T, fin) * 2 == need
        parts.append(c.streams_decode_ragged([s], [np.ascontiguousarray(seq[:, at:at + T])], final=[fin])[0])
        at += T
    assert np.array_equal(np.concatenate(parts), ref)
    # an item after the final item
    assert _raw_pcm(c, [s], [4], [0], seq[:, :4], 1 << 22) != 0 and "already flushed" in last_err(), last_err()
    with pytest.raises(RuntimeError, match="already flushed"):
        c.streams_pending(s, 4)
    c.streams_close(s)


def test_old_calls_refuse_a_speed_stream_and_open_refuses_a_bad_speed(codec, seq):
    c = codec
    s = c.streams_open(speed=0.5)
    c._dtypes().pop(s)  # (the wrapper would route the call to fs_codec_streams_decode_pcm: go through the old calls as an old client would)
    with pytest.raises(RuntimeError, match="fs_codec_streams_open_speed.*fs_codec_streams_decode_pcm"):
        c.streams_decode_ragged([s], [seq[:, :5]])
    with pytest.raises(RuntimeError, match="fs_codec_streams_open_speed.*fs_codec_streams_decode_pcm"):
        c.streams_decode([s], np.ascontiguousarray(seq[None, :, :16]))
    c._dtypes()[s] = "f32"
    got = np.concatenate(_feed(c, s, seq, SPLITS[1]))  # the refused calls changed nothing
    assert np.array_equal(got, _ref(c, seq, 0.5, None))
    c.streams_close(s)
    for bad in (0.2, 4.5, 0.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="speed"):
            c.streams_open(speed=bad)
    bad_spec = _ffi.pcm_spec(24000, "sinc", "s16")
    bad_spec.format = 9
    sid = C.c_int(-1)
    assert _ffi.lib().fs_codec_streams_open_speed(c._h, C.c_double(1.25), C.byref(bad_spec), C.byref(sid)) != 0
    assert "format" in _ffi.lib().fs_last_error().decode()
    # none of the refused opens took a stream id
    ids = [c.streams_open() for _ in range(3)]
    assert s in ids
    for i in ids:
        c.streams_close(i)


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


def test_session_streamer_with_a_speed_per_request(codec):
    cfg, tok = fcfg.TINY, fcfg.TINY_TOKENS
    lm = fishrt.DualARTransformer(cfg, tok, 0, "bf16", max_batch=3).load_synthetic(0xF15E5EED)
    rng = np.random.RandomState(3)
    Ls, Fs, speeds = (12, 7, 9), (37, 20, 9), (None, 0.8, 1.5)  # the second finishes on a chunk boundary (4 + 8 + 8): a flush with no frames
    prompts = []
    for L in Ls:
        p = np.zeros((9, L), np.uint32)
        p[0] = rng.randint(0, min(tok["semantic_start_id"], 400), L)
        prompts.append(p)
    pcm, finals = {i: [] for i in range(3)}, []
    with lm.session(temp=0.0, top_p=1.0, top_k=0, seed=42, ignore_eos=True) as raw:
        ss = fishrt.SessionStreamer(_CodesBelow1000(raw), codec, chunk=8, first_chunk=4, ragged=True,
                                    on_audio=lambda tag, p, final: (pcm[tag].append(p.copy()), final and finals.append(tag)))
        for i in range(3):
            assert ss.add(prompts[i], Ls[i] + Fs[i], tag=i, speed=speeds[i]) is not None
        step = 0
        while len(ss.results) < 3:
            ss.step(4)
            step += 1
            assert step < 200
    assert sorted(finals) == [0, 1, 2]
    for i in range(3):
        kw = {} if speeds[i] is None else dict(speed=speeds[i])
        ref = codec.decode(np.ascontiguousarray(ss.results[i][None]), **kw)[0, 0]
        got = np.concatenate(pcm[i])
        assert got.dtype == ref.dtype and got.shape == ref.shape, (i, got.shape, ref.shape)
        assert np.array_equal(got, ref), i
        assert ss.stats[i]["samples"] == ref.shape[0] and ss.stats[i]["frames"] == ss.results[i].shape[1]
    assert len(pcm[1]) > 2 and sum(len(p) > 0 for p in pcm[1][:-1]) >= 1  # the speed request streamed: audio before its final piece
