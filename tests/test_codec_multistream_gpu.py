"""GPU: many concurrent vocoder streams on one codec handle (fs_codec_streams_*).  Every call advances a subset of the open streams by a
common T in one launch sequence; per stream, the PCM of its chunks concatenated must equal decoding its whole sequence at b = 1, bit for
bit, in both matrix-core precision modes -- whatever the other streams in the call are, in which order the ids come, and after rejected
calls.  End to end: fishrt.SessionStreamer streams every request of a continuous-batching session through it."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import fishrt
from fishrt import _ffi
from fishrt import config as fcfg

G = os.path.join(os.path.dirname(__file__), "golden")


def _voice():
    return np.ascontiguousarray(np.load(os.path.join(G, "default_voice_codes.npy")).astype(np.uint32))  # (8, 274)


def _sequences():
    voice, rng = _voice(), np.random.RandomState(5)
    return [voice, np.ascontiguousarray(voice[:, 60:210]), rng.randint(0, 1000, (8, 300)).astype(np.uint32),
            rng.randint(0, 1000, (8, 97)).astype(np.uint32), rng.randint(0, 1000, (8, 50)).astype(np.uint32)]


@pytest.mark.parametrize("precision", ["f16", "bf16x3"])
def test_interleaved_streams_equal_one_shot_bit_for_bit(precision):
    c = fishrt.FireflyCodec(0, precision=precision).load_synthetic(0xC0DEC)
    seqs = _sequences()
    refs = [c.decode(s[None])[0, 0] for s in seqs]
    rng = np.random.RandomState(17)
    # the single-stream API on the same handle runs alongside and is independent of the multi-streams
    c.stream_begin()
    single, single_at = [], 0
    start_round = [0, 0, 2, 5, None]  # the fifth sequence opens once a stream has closed: it must get the freed id and start clean
    sid, pos, parts, closed_ids = {}, [0] * 5, [[] for _ in seqs], []
    calls, rnd = 0, 0
    while True:
        for i, r in enumerate(start_round):
            if i not in sid and pos[i] == 0 and ((r is not None and rnd >= r) or (r is None and closed_ids)):
                sid[i] = c.streams_open()
                if r is None:
                    assert sid[i] in closed_ids, (sid[i], closed_ids)
        live = [i for i in sid if seqs[i].shape[1] - pos[i] >= 16]
        if live:
            T = int(rng.choice([16, 17, 32, 64, 100]))
            cand = [i for i in live if seqs[i].shape[1] - pos[i] >= T] or live
            if cand is live:
                T = min(seqs[i].shape[1] - pos[i] for i in live)
            pick = [i for i in cand if rng.rand() < 0.75] or cand[:1]
            rng.shuffle(pick)
            pcm = c.streams_decode([sid[i] for i in pick], np.stack([seqs[i][:, pos[i]:pos[i] + T] for i in pick]))
            calls += 1
            for k, i in enumerate(pick):
                parts[i].append(pcm[k])
                pos[i] += T
        for i in list(sid):
            left = seqs[i].shape[1] - pos[i]
            if 0 < left < 16:  # a short tail: stateless decode with a halo, then the stream closes
                parts[i].append(fishrt.decode_chunk(c, seqs[i], pos[i], seqs[i].shape[1]))
                pos[i] = seqs[i].shape[1]
            if pos[i] == seqs[i].shape[1]:
                c.streams_close(sid[i])
                closed_ids.append(sid.pop(i))
        if single_at < 274:
            n = min(40, 274 - single_at)
            single.append(c.stream_decode(seqs[0][:, single_at:single_at + n]) if n >= 16 else fishrt.decode_chunk(c, seqs[0], single_at, 274))
            single_at += n
        rnd += 1
        if all(p == s.shape[1] for p, s in zip(pos, seqs)):
            break
        assert rnd < 200
    c.stream_end()
    assert calls > 10
    for i, ref in enumerate(refs):
        got = np.concatenate(parts[i])
        assert got.shape == ref.shape and np.array_equal(got, ref), (precision, i, float(np.abs(got - ref).max()))
    assert np.array_equal(np.concatenate(single), refs[0])
    c.close()


def test_id_order_does_not_matter():
    c = fishrt.FireflyCodec(0).load_synthetic(0xC0DEC)
    seqs = [np.ascontiguousarray(s[:, :80]) for s in _sequences()[:4]]
    out = []
    for orders in (([0, 1, 2, 3], [3, 1, 0, 2]), ([2, 0, 3, 1], [1, 2, 3, 0])):
        ids = [c.streams_open() for _ in seqs]
        got = [[] for _ in seqs]
        for a, b, order in ((0, 48, orders[0]), (48, 80, orders[1])):
            pcm = c.streams_decode([ids[i] for i in order], np.stack([seqs[i][:, a:b] for i in order]))
            for k, i in enumerate(order):
                got[i].append(pcm[k])
        for i in ids:
            c.streams_close(i)
        out.append([np.concatenate(g) for g in got])
    for i, s in enumerate(seqs):
        ref = c.decode(s[None])[0, 0]
        assert np.array_equal(out[0][i], ref) and np.array_equal(out[1][i], ref), i
    c.close()


def test_rejected_calls_leave_every_context_untouched():
    c = fishrt.FireflyCodec(0).load_synthetic(0xC0DEC)
    voice = _voice()
    other = np.random.RandomState(9).randint(0, 1000, (8, 96)).astype(np.uint32)
    ref_v, ref_o = c.decode(np.ascontiguousarray(voice[None, :, :96]))[0, 0], c.decode(other[None])[0, 0]
    s, t = c.streams_open(), c.streams_open()
    pv, po = [], []

    def good(a, b):
        pcm = c.streams_decode([s, t], np.stack([voice[:, a:b], other[:, a:b]]))
        pv.append(pcm[0])
        po.append(pcm[1])

    good(0, 32)
    gone = c.streams_open()
    c.streams_close(gone)
    bad_code = np.stack([voice[:, 32:64], other[:, 32:64]])
    bad_code[1, 3, 7] = 1000
    for ids, codes, msg in (([s, s], np.stack([voice[:, 32:64]] * 2), "twice"),
                            ([s, gone], np.stack([voice[:, 32:64], other[:, 32:64]]), "not an open stream"),
                            ([s, 63], np.stack([voice[:, 32:64], other[:, 32:64]]), "not an open stream"),
                            ([s, t], np.stack([voice[:, 32:40], other[:, 32:40]]), "16 frames"),
                            ([s, t], bad_code, "FSQ index")):
        with pytest.raises(RuntimeError, match=msg):
            c.streams_decode(ids, codes)
    good(32, 64)
    _ffi.check(_ffi.lib().fs_codec_set_precision(c._h, 1))  # the streams were opened in f16 mode
    with pytest.raises(RuntimeError, match="precision mode changed"):
        c.streams_decode([t, s], np.stack([other[:, 64:96], voice[:, 64:96]]))
    _ffi.check(_ffi.lib().fs_codec_set_precision(c._h, 2))
    good(64, 96)
    assert np.array_equal(np.concatenate(pv), ref_v) and np.array_equal(np.concatenate(po), ref_o)
    with pytest.raises(RuntimeError, match="not an open stream"):
        c.streams_close(gone)
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
def test_session_streamer_end_to_end(rows):
    if rows:
        cfg, tok = fcfg.FISH_1_5, fcfg.FISH_1_5_TOKENS
    else:
        cfg, tok = fcfg.TINY, fcfg.TINY_TOKENS
    lm = fishrt.DualARTransformer(cfg, tok, 0, "bf16", max_batch=4).load_synthetic(0xF15E5EED)
    if rows and not lm.rows_supported(4):
        pytest.skip("fs_lm_rows_supported says no for a max_batch 4 bf16 Fish-1.5 handle on this device")
    rng = np.random.RandomState(3)
    prompts = [_prompt(rng, L, tok["semantic_start_id"]) for L in (12, 7, 20, 9)]
    budgets = [L + F for L, F in zip((12, 7, 20, 9), (90, 61, 120, 40))]
    joins = [0, 0, 3, 7]  # requests join at different steps
    kw = dict(temp=0.0, top_p=1.0, top_k=0, seed=42, ignore_eos=True, rows=rows)

    def run(stream):
        codec = fishrt.FireflyCodec(0).load_synthetic(0xC0DEC) if stream else None
        out, pcm = {}, {i: [] for i in range(4)}
        with lm.session(**kw) as raw:
            s = _CodesBelow1000(raw)
            ss = fishrt.SessionStreamer(s, codec, chunk=32, first_chunk=16,
                                        on_audio=lambda tag, p, final: pcm[tag].append(p)) if stream else None
            live, step = {}, 0
            while len(out) < 4:
                for i in range(4):
                    if joins[i] <= step and i not in out and i not in live.values():
                        slot = ss.add(prompts[i], budgets[i], tag=i) if stream else s.add(prompts[i], budgets[i])
                        assert slot is not None
                        live[slot] = i
                if stream:
                    ss.step(8)
                    for slot, i in list(live.items()):
                        if i in ss.results:  # finished: flushed, its stream closed and its slot released by the streamer
                            out[i] = ss.results[i]
                            del live[slot]
                else:
                    s.step(8)
                    for slot in list(live):
                        codes, done = s.poll(slot)
                        if done:
                            out[live.pop(slot)] = codes
                            s.release(slot)
                step += 1
                assert step < 500
        return out, pcm, (ss, codec)

    plain, _, _ = run(False)
    got, pcm, (ss, codec) = run(True)
    for i in range(4):
        assert np.array_equal(got[i], plain[i]), i
        ref = codec.decode(np.ascontiguousarray(got[i][None]))[0, 0]
        streamed = np.concatenate(pcm[i])
        assert streamed.shape == ref.shape and np.array_equal(streamed, ref), (i, float(np.abs(streamed - ref).max()))
        assert ss.stats[i]["frames"] == got[i].shape[1] and ss.stats[i]["first_audio_s"] is not None
    per_q = {}
    for q, kind, n, T in ss.calls:
        if kind == "chunk":
            per_q.setdefault(q, []).append(T)
    assert all(len(Ts) == len(set(Ts)) for Ts in per_q.values()), per_q  # <= 1 vocoder call per distinct T per step
    assert any(n > 1 for _, kind, n, _ in ss.calls if kind == "chunk")
    codec.close()
