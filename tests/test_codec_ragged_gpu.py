"""GPU: the ragged multi-stream vocoder call (fs_codec_streams_decode_ragged).  Every item of a call advances its stream by its own number
of frames, from 1 up; per stream, the PCM of all its chunks concatenated must equal fs_codec_decode of its whole sequence at b = 1, bit for
bit (np.array_equal), in both matrix-core precision modes -- whatever the chunk lengths, the other items of a call, their order, and after
rejected calls.  End to end: fishrt.SessionStreamer(ragged=True) makes at most one vocoder call per step."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import fishrt
from fishrt import _ffi
from fishrt import config as fcfg

G = os.path.join(os.path.dirname(__file__), "golden")
FORCED = [1, 2, 3, 4, 7, 8, 15, 16, 17]


def _voice():
    return np.ascontiguousarray(np.load(os.path.join(G, "default_voice_codes.npy")).astype(np.uint32))  # (8, 274)


def _cut(rng, total, lo, hi):
    out = []
    while total > 0:
        t = min(int(rng.randint(lo, hi + 1)), total)
        out.append(t)
        total -= t
    return out


def _schedule(seed):
    """-> (sequences, chunk lengths per stream): 7 streams of 1 .. ~200 frames; stream 0 is fed one frame at a time, stream 1 only in chunks
    below 16 frames, stream 2 starts with every forced length, stream 3 is a single frame, the others are cut into chunks of 1 .. 80"""
    rng, voice = np.random.RandomState(seed), _voice()
    lengths = [13, 90, sum(FORCED) + 60, 1, 200, 149, 77]
    seqs = [rng.randint(0, 1000, (8, L)).astype(np.uint32) for L in lengths]
    seqs[4] = np.ascontiguousarray(voice[:, :200])
    seqs[6] = np.ascontiguousarray(voice[:, 120:197])
    forced = list(FORCED)
    rng.shuffle(forced)
    chunks = [[1] * 13, _cut(rng, 90, 1, 15), forced + _cut(rng, 60, 1, 80), [1], _cut(rng, 200, 1, 80), _cut(rng, 149, 1, 80),
              _cut(rng, 77, 1, 80)]
    assert all(sum(c) == s.shape[1] for c, s in zip(chunks, seqs))
    assert all(t < 16 for t in chunks[1]) and set(FORCED) <= set(chunks[2])
    return seqs, chunks


@pytest.mark.parametrize("precision", ["f16", "bf16x3"])
def test_random_ragged_schedules_equal_one_shot_bit_for_bit(precision):
    c = fishrt.FireflyCodec(0, precision=precision).load_synthetic(0xC0DEC)
    seqs, chunks = _schedule(23)
    refs = [c.decode(s[None])[0, 0] for s in seqs]
    rng = np.random.RandomState(31)
    sid = [c.streams_open() for _ in seqs]
    pos, nxt, parts = [0] * len(seqs), [0] * len(seqs), [[] for _ in seqs]
    calls, seen = 0, set()
    while any(nxt[i] < len(chunks[i]) for i in range(len(seqs))):
        live = [i for i in range(len(seqs)) if nxt[i] < len(chunks[i])]
        pick = [i for i in live if rng.rand() < 0.6] or live[:1]
        rng.shuffle(pick)
        items = [np.ascontiguousarray(seqs[i][:, pos[i]:pos[i] + chunks[i][nxt[i]]]) for i in pick]
        pcm = c.streams_decode_ragged([sid[i] for i in pick], items)
        calls += 1
        assert len(pcm) == len(pick)
        for k, i in enumerate(pick):
            T = chunks[i][nxt[i]]
            assert pcm[k].shape == (2048 * T,)
            parts[i].append(pcm[k].copy())
            seen.add(T)
            pos[i] += T
            nxt[i] += 1
        assert calls < 1000
    assert set(FORCED) <= seen and calls > 10
    for i, ref in enumerate(refs):
        got = np.concatenate(parts[i])
        assert got.shape == ref.shape, (precision, i)
        assert np.array_equal(got, ref), (precision, i, chunks[i], float(np.abs(got - ref).max()))
    for s in sid:
        c.streams_close(s)
    c.close()


@pytest.mark.parametrize("precision", ["f16", "bf16x3"])
def test_uniform_lengths_equal_the_uniform_call_and_the_calls_interleave(precision):
    c = fishrt.FireflyCodec(0, precision=precision).load_synthetic(0xC0DEC)
    rng = np.random.RandomState(4)
    seqs = [rng.randint(0, 1000, (8, 112)).astype(np.uint32), np.ascontiguousarray(_voice()[:, 30:142]), rng.randint(0, 1000, (8, 112)).astype(np.uint32)]
    refs = [c.decode(s[None])[0, 0] for s in seqs]
    cuts = [(0, 16), (16, 48), (48, 65), (65, 112)]  # all >= 16 frames
    a = [c.streams_open() for _ in seqs]  # fed through the uniform call only
    b = [c.streams_open() for _ in seqs]  # fed through the ragged call only
    d = [c.streams_open() for _ in seqs]  # alternating
    pa, pb, pd = [[] for _ in seqs], [[] for _ in seqs], [[] for _ in seqs]
    for k, (lo, hi) in enumerate(cuts):
        items = [np.ascontiguousarray(s[:, lo:hi]) for s in seqs]
        u = c.streams_decode(a, np.stack(items))
        r = c.streams_decode_ragged(b, items)
        m = c.streams_decode(d, np.stack(items)) if k % 2 == 0 else c.streams_decode_ragged(d, items)
        for i in range(len(seqs)):
            assert np.array_equal(u[i], r[i]), (precision, k, i)
            pa[i].append(u[i])
            pb[i].append(r[i].copy())
            pd[i].append(np.array(m[i]))
    for i, ref in enumerate(refs):
        for parts in (pa, pb, pd):
            assert np.array_equal(np.concatenate(parts[i]), ref), (precision, i)
    c.close()


def test_order_and_company_do_not_change_a_chunk():
    c = fishrt.FireflyCodec(0).load_synthetic(0xC0DEC)
    rng = np.random.RandomState(8)
    seq = np.ascontiguousarray(_voice()[:, 40:80])
    others = [rng.randint(0, 1000, (8, 120)).astype(np.uint32) for _ in range(3)]
    ref = c.decode(seq[None])[0, 0]
    for first, T in ((21, 5), (9, 1), (0, 1)):  # the chunk under test: frames [first, first + T) of `seq`, after one earlier chunk (or none)
        chunk = np.ascontiguousarray(seq[:, first:first + T])
        got = {}
        for name, where, company in (("alone", 0, []), ("first", 0, [7, 3]), ("last", 2, [3, 7]), ("next to 80x longer", 1, [80 * T])):
            s = c.streams_open()
            o = [c.streams_open() for _ in company]
            if first:
                c.streams_decode_ragged([s], [np.ascontiguousarray(seq[:, :first])])
            ids, items = [o[k] for k in range(len(company))], [np.ascontiguousarray(others[k][:, :n]) for k, n in enumerate(company)]
            ids.insert(where, s)
            items.insert(where, chunk)
            got[name] = c.streams_decode_ragged(ids, items)[where].copy()
            for i in [s] + o:
                c.streams_close(i)
        for name, pcm in got.items():
            assert np.array_equal(pcm, ref[2048 * first:2048 * (first + T)]), (first, T, name)
    c.close()


def _raw_ragged(c, n, ids, T, codes):
    ids, T, codes = np.asarray(ids, np.int32), np.asarray(T, np.int32), np.ascontiguousarray(codes, np.uint32)
    pcm = np.zeros(2048 * max(1, int(np.clip(T, 0, None).sum())), np.float32)
    return _ffi.lib().fs_codec_streams_decode_ragged(c._h, int(n), ids.ctypes.data_as(_ffi.C.POINTER(_ffi.C.c_int)),
                                                     T.ctypes.data_as(_ffi.C.POINTER(_ffi.C.c_int)),
                                                     codes.ctypes.data_as(_ffi.C.POINTER(_ffi.C.c_uint32)),
                                                     pcm.ctypes.data_as(_ffi.C.POINTER(_ffi.C.c_float)))


def test_rejected_calls_leave_every_stream_untouched():
    c = fishrt.FireflyCodec(0).load_synthetic(0xC0DEC)
    voice = np.ascontiguousarray(_voice()[:, :60])
    other = np.random.RandomState(9).randint(0, 1000, (8, 60)).astype(np.uint32)
    ref_v, ref_o = c.decode(voice[None])[0, 0], c.decode(other[None])[0, 0]
    s, t = c.streams_open(), c.streams_open()
    pv, po = [], []
    at = [0, 0]

    def good(nv, no):
        pcm = c.streams_decode_ragged([t, s], [other[:, at[1]:at[1] + no], voice[:, at[0]:at[0] + nv]])
        po.append(pcm[0].copy())
        pv.append(pcm[1].copy())
        at[0] += nv
        at[1] += no

    good(3, 21)  # an odd number of chunks so far: the parity of both streams is 1
    gone = c.streams_open()
    c.streams_close(gone)
    two = np.concatenate([voice[:, 3:8].reshape(-1), other[:, 21:30].reshape(-1)])
    bad = two.copy()
    bad[-1] = 1000  # in the last item
    last_err = lambda: _ffi.lib().fs_last_error().decode()
    for n, ids, T, codes, msg in ((2, [s, t], [5, 0], two, ">= 1 frame"),
                                  (2, [s, t], [5, -3], two, ">= 1 frame"),
                                  (2, [s, s], [5, 9], two, "twice"),
                                  (2, [s, gone], [5, 9], two, "not an open stream"),
                                  (2, [s, t], [5, 9], bad, "FSQ index"),
                                  (0, [s, t], [5, 9], two, "1 .. 64"),
                                  (65, list(range(65)), [1] * 65, np.zeros(65 * 8, np.uint32), "1 .. 64")):
        assert _raw_ragged(c, n, ids, T, codes) != 0, msg
        assert msg in last_err(), (msg, last_err())
    good(5, 9)
    _ffi.check(_ffi.lib().fs_codec_set_precision(c._h, 1))  # the streams were opened in f16 mode
    with pytest.raises(RuntimeError, match="precision mode changed"):
        c.streams_decode_ragged([s], [voice[:, 8:10]])
    _ffi.check(_ffi.lib().fs_codec_set_precision(c._h, 2))
    good(1, 30)
    pcm = c.streams_decode_ragged([s], [voice[:, at[0]:]])
    pv.append(pcm[0].copy())
    assert np.array_equal(np.concatenate(pv), ref_v) and np.array_equal(np.concatenate(po), ref_o)
    c.close()
    for kw in (dict(precision="f32"), dict(channel_div=8)):
        h = fishrt.FireflyCodec(0, **kw).load_synthetic(1)
        with pytest.raises(RuntimeError, match="plane data flow"):
            h.streams_open()
        h.close()


class _CodesBelow1000:
    """the synthetic Fish-1.5 LM samples from its 1024 codebook entries, the codec's FSQ has 1000: fold its codes into range (both runs
    of the test see the same mapping)"""

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


def _prompt(rng, L, start):
    p = np.zeros((9, L), np.uint32)
    p[0] = rng.randint(0, min(start, 400), L)
    return p


@pytest.mark.parametrize("rows", [False, True], ids=["static-step", "rows"])
def test_ragged_session_streamer_end_to_end(rows):
    if rows:
        cfg, tok = fcfg.FISH_1_5, fcfg.FISH_1_5_TOKENS
    else:
        cfg, tok = fcfg.TINY, fcfg.TINY_TOKENS
    lm = fishrt.DualARTransformer(cfg, tok, 0, "bf16", max_batch=4).load_synthetic(0xF15E5EED)
    if rows and not lm.rows_supported(4):
        pytest.skip("fs_lm_rows_supported says no for a max_batch 4 bf16 Fish-1.5 handle on this device")
    rng = np.random.RandomState(3)
    prompts = [_prompt(rng, L, tok["semantic_start_id"]) for L in (12, 7, 20, 9)]
    budgets = [L + F for L, F in zip((12, 7, 20, 9), (90, 61, 123, 3))]  # tails of 14, 9, 23 frames; one request shorter than first_chunk
    joins = [0, 0, 3, 7]
    kw = dict(temp=0.0, top_p=1.0, top_k=0, seed=42, ignore_eos=True, rows=rows)
    codec = fishrt.FireflyCodec(0).load_synthetic(0xC0DEC)
    out, pcm, finals = {}, {i: [] for i in range(4)}, []
    with lm.session(**kw) as raw:
        s = _CodesBelow1000(raw)
        ss = fishrt.SessionStreamer(s, codec, chunk=24, first_chunk=4, ragged=True,
                                    on_audio=lambda tag, p, final: (pcm[tag].append(p.copy()), final and finals.append(tag)))
        live, step = {}, 0
        while len(out) < 4:
            for i in range(4):
                if joins[i] <= step and i not in out and i not in live.values():
                    slot = ss.add(prompts[i], budgets[i], tag=i)
                    assert slot is not None
                    live[slot] = i
            ss.step(8)
            for slot, i in list(live.items()):
                if i in ss.results:
                    out[i] = ss.results[i]
                    del live[slot]
            step += 1
            assert step < 500
    assert sorted(finals) == [0, 1, 2, 3]
    for i in range(4):
        ref = codec.decode(np.ascontiguousarray(out[i][None]))[0, 0]
        streamed = np.concatenate(pcm[i])
        assert streamed.shape == ref.shape and np.array_equal(streamed, ref), (i, float(np.abs(streamed - ref).max()))
        assert ss.stats[i]["frames"] == out[i].shape[1] and ss.stats[i]["first_audio_s"] is not None
    quanta = [q for q, _, _, _ in ss.calls]
    assert len(quanta) == len(set(quanta)), ss.calls  # at most one vocoder call per step
    assert {kind for _, kind, _, _ in ss.calls} == {"ragged"}
    assert any(n > 1 for _, _, n, _ in ss.calls)
    for sid in range(codec.STREAMS_MAX):  # every stream id is closed again
        with pytest.raises(RuntimeError, match="not an open stream"):
            codec.streams_close(sid)
    codec.close()
