"""CPU: the ragged multi-stream vocoder call without a GPU -- the header declares fs_codec_streams_decode_ragged, the library exports it and
fishrt._ffi lists it; FireflyCodec.streams_decode_ragged checks its arguments before any C call; the context rule the kernels implement
("last PAD slots of old context ++ new data") restated in numpy; and fishrt.SessionStreamer(ragged=True)'s scheduling against a fake
session and a fake codec: at most one vocoder call per step, tails of any length in that call, any chunk size >= 1 -- while ragged=False
keeps the call sequence it had."""
import ctypes
import os
import re

import numpy as np
import pytest

from fishrt import _ffi
from fishrt.codec import FireflyCodec
from fishrt.stream import SessionStreamer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPF = 4  # samples per frame of the fake codec


def test_header_library_and_ffi_agree_on_the_entry_point():
    header = open(os.path.join(ROOT, "include", "fishrt.h")).read()
    m = re.search(r"int\s+fs_codec_streams_decode_ragged\s*\(([^;]*)\);", header)
    assert m, "include/fishrt.h does not declare fs_codec_streams_decode_ragged"
    args = " ".join(m.group(1).split())
    assert args == "fs_codec_t* c, int n, const int* stream_ids, const int* T, const uint32_t* codes, float* pcm_out"
    assert "fs_codec_streams_decode_ragged" in _ffi.SYMBOLS
    assert hasattr(ctypes.CDLL(_ffi.LIB_PATH), "fs_codec_streams_decode_ragged")
    assert "fs_codec_streams_decode_ragged" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_argument_checks_come_before_the_c_call():
    c = object.__new__(FireflyCodec)  # no handle: reaching the C call would fail with something other than ValueError
    c._h = None
    ok = np.zeros((8, 3), np.uint32)
    for ids, chunks in (([0, 1], [ok]),                          # one chunk per id
                        ([0], [ok, ok]),
                        ([], []),                                # empty call
                        ([0], [np.zeros((8, 0), np.uint32)]),    # empty chunk
                        ([0], [np.zeros((7, 3), np.uint32)]),    # wrong number of codebooks
                        ([0], [np.zeros((1, 8, 3), np.uint32)]),  # wrong rank
                        ([0, 1], [ok, np.zeros(24, np.uint32)]),
                        (list(range(65)), [ok] * 65)):
        with pytest.raises(ValueError, match="streams_decode_ragged"):
            c.streams_decode_ragged(ids, chunks)


def test_context_rule_last_pad_of_old_plus_new():
    """what the kernels do per tensor, per item: slot j of the new context is slot Te - PAD + j of the item's own data where that index is
    >= 0, else slot j + Te of the old context.  Feeding a signal in chunks of any lengths must leave the last PAD slots of the zero-padded
    signal, the same as one chunk would."""
    PAD = 64
    rng = np.random.RandomState(0)
    for per in (4, 8, 64):  # slots per frame at different stages
        x = rng.randint(1, 1 << 16, 300 * per)
        for lengths in ([1] * 40, [1, 2, 3, 4, 7, 8, 15, 16, 17], [80, 1, 1, 30], [16] * 5):
            ctx, at = np.zeros(PAD, x.dtype), 0
            for T in lengths:
                Te = T * per
                new, data = np.empty(PAD, x.dtype), x[at:at + Te]
                for j in range(PAD):
                    new[j] = data[Te - PAD + j] if Te - PAD + j >= 0 else ctx[j + Te]
                assert np.array_equal(new, np.concatenate([ctx, data])[-PAD:])
                ctx, at = new, at + Te
            assert np.array_equal(ctx, np.concatenate([np.zeros(PAD, x.dtype), x[:at]])[-PAD:])


# ---- the scheduling, against fakes (the pattern of tests/test_session_streamer_cpu.py)
def _pcm_of(codes):
    return (codes[0].astype(np.float32)[:, None] + np.arange(SPF, dtype=np.float32)[None] / SPF).reshape(-1)


class FakeCodec:
    STREAM_MIN_FRAMES = 16

    def __init__(self):
        self.open, self.next_id, self.calls, self.ragged_calls, self.decode_calls, self.fail_next = {}, 0, [], [], [], None

    def streams_open(self):
        sid = self.next_id
        self.next_id += 1
        self.open[sid] = 0
        return sid

    def streams_close(self, sid):
        del self.open[sid]

    def streams_decode(self, ids, codes):
        codes = np.asarray(codes)
        assert codes.ndim == 3 and codes.shape[0] == len(ids) and codes.shape[2] >= self.STREAM_MIN_FRAMES
        assert len(set(ids)) == len(ids) and all(i in self.open for i in ids)
        self.calls.append((list(ids), codes.shape[2]))
        for i in ids:
            self.open[i] += codes.shape[2]
        return np.stack([_pcm_of(c) for c in codes])

    def streams_decode_ragged(self, ids, chunks):
        if self.fail_next:
            e, self.fail_next = self.fail_next, None
            raise e
        assert len(chunks) == len(ids) >= 1 and len(set(ids)) == len(ids) and all(i in self.open for i in ids)
        assert all(c.ndim == 2 and c.shape[0] == 8 and c.shape[1] >= 1 for c in chunks)
        self.ragged_calls.append((list(ids), [c.shape[1] for c in chunks]))
        for i, c in zip(ids, chunks):
            self.open[i] += c.shape[1]
        return [_pcm_of(c) for c in chunks]

    def decode(self, codes):  # the halo path (stream.decode_chunk)
        self.decode_calls.append(codes.shape)
        return _pcm_of(codes[0])[None, None]


class FakeSession:
    def __init__(self, seqs, max_batch=4):
        self.seqs, self.max_batch, self.slots, self.released = seqs, max_batch, {}, []

    def add(self, prompt, max_new_tokens):
        free = [s for s in range(self.max_batch) if s not in self.slots]
        if not free:
            return None
        self.slots[free[0]] = [int(prompt), 0]
        return free[0]

    def step(self, k):
        for st in self.slots.values():
            st[1] = min(st[1] + k, self.seqs[st[0]].shape[1])
        return sum(st[1] < self.seqs[st[0]].shape[1] for st in self.slots.values())

    def poll(self, slot, codes=True):
        i, n = self.slots[slot]
        done = n == self.seqs[i].shape[1]
        return (self.seqs[i][:, :n].copy(), done) if codes else (n, done)

    def release(self, slot):
        del self.slots[slot]
        self.released.append(slot)


def _seqs(lengths, seed=0):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 1000, (8, L)).astype(np.uint32) for L in lengths]


def _drive(lengths, joins, k, max_batch=4, **kw):
    seqs = _seqs(lengths)
    sess, codec, pieces = FakeSession(seqs, max_batch), FakeCodec(), {i: [] for i in range(len(lengths))}
    finals = []
    ss = SessionStreamer(sess, codec, on_audio=lambda tag, pcm, final: (pieces[tag].append(pcm), final and finals.append(tag)), **kw)
    step, pending = 0, list(range(len(lengths)))
    while pending or ss.live:
        for i in [i for i in pending if joins[i] <= step]:
            if ss.add(i, 0, tag=i) is not None:
                pending.remove(i)
        ss.step(k)
        step += 1
        assert step < 1000
    assert sorted(finals) == list(range(len(lengths))), finals  # exactly one final signal per request
    return ss, codec, seqs, pieces


def test_ragged_one_call_per_step_tails_included():
    lengths, joins = [200, 75, 16, 9, 130, 47, 4, 28], [0, 0, 2, 3, 5, 9, 11, 12]
    ss, codec, seqs, pieces = _drive(lengths, joins, k=8, chunk=24, first_chunk=4, ragged=True)
    quanta = [q for q, _, _, _ in ss.calls]
    assert len(quanta) == len(set(quanta)), ss.calls                    # at most one vocoder call per step
    assert {kind for _, kind, _, _ in ss.calls} == {"ragged"}           # no "chunk", "tail" or "halo"
    assert codec.calls == [] and codec.decode_calls == []               # nothing went through the uniform call or the one-shot decode
    assert len(codec.ragged_calls) == len(ss.calls)
    assert any(len(set(Ts)) > 1 for _, Ts in codec.ragged_calls)        # first pieces, steady pieces and tails share calls
    assert any(min(Ts) < 16 for _, Ts in codec.ragged_calls)
    for (_, _, n, T), (ids, Ts) in zip(ss.calls, codec.ragged_calls):
        assert n == len(ids) and T == max(Ts)
    for i, seq in enumerate(seqs):
        assert np.array_equal(np.concatenate(pieces[i]), _pcm_of(seq)), i
        assert np.array_equal(ss.results[i], seq)
        sizes = [len(p) // SPF for p in pieces[i] if len(p)]
        assert sum(sizes) == seq.shape[1]
        if seq.shape[1] > 4:  # first piece = first_chunk, then chunk-sized pieces, then whatever remains
            assert sizes[0] == 4 and all(s == 24 for s in sizes[1:-1]) and sizes[-1] <= 24 + 8, (i, sizes)
        st = ss.stats[i]
        assert st["frames"] == seq.shape[1] and st["chunks"] == len(sizes) and st["first_audio_s"] is not None
    assert codec.open == {} and ss.live == {}
    assert len(ss.session.released) == len(lengths)


def test_ragged_any_chunk_size_from_one():
    ss, codec, seqs, pieces = _drive([7, 3, 12], [0, 0, 1], k=1, chunk=1, first_chunk=1, ragged=True)
    assert all(max(Ts) == 1 for _, Ts in codec.ragged_calls)
    for i, seq in enumerate(seqs):
        assert np.array_equal(np.concatenate(pieces[i]), _pcm_of(seq))
    with pytest.raises(ValueError):
        SessionStreamer(FakeSession([]), FakeCodec(), chunk=0, ragged=True)
    with pytest.raises(ValueError):
        SessionStreamer(FakeSession([]), FakeCodec(), chunk=8, first_chunk=0, ragged=True)
    with pytest.raises(ValueError):
        SessionStreamer(FakeSession([]), FakeCodec(), chunk=8)  # ragged=False keeps the 16-frame minimum


def test_ragged_finished_request_with_nothing_left_still_signals_final():
    # two requests whose first pieces share the first call; both finish with their tails in a call, streams closed, slots released
    ss, codec, seqs, pieces = _drive([28, 4], [0, 0], k=4, chunk=24, first_chunk=4, ragged=True)
    assert [Ts for _, Ts in codec.ragged_calls][0] == [4, 4]
    assert codec.open == {} and len(ss.session.released) == 2
    # a request whose frames are all vocoded before it is seen finished: the session reports done one step late
    class LateDone(FakeSession):
        seen = None

        def poll(self, slot, codes=True):
            i, n = self.slots[slot]
            full = n == self.seqs[i].shape[1]
            done = full and self.seen == slot
            if full:
                self.seen = slot
            return (self.seqs[i][:, :n].copy(), done) if codes else (n, done)

    seqs = _seqs([8])
    sess, codec, got = LateDone(seqs), FakeCodec(), []
    ss = SessionStreamer(sess, codec, chunk=4, first_chunk=4, ragged=True, on_audio=lambda tag, pcm, final: got.append((len(pcm) // SPF, final)))
    ss.add(0, 0, tag="a")
    while ss.live:
        ss.step(4)
    assert got == [(4, False), (4, False), (0, True)], got
    assert len(codec.ragged_calls) == 2 and codec.open == {} and sess.released == [0]


def test_ragged_errors_surface_and_finished_streams_close():
    sess, codec = FakeSession(_seqs([6, 100])), FakeCodec()
    ss = SessionStreamer(sess, codec, chunk=24, first_chunk=4, ragged=True)
    ss.add(0, 0)
    ss.add(1, 0)
    codec.fail_next = RuntimeError("vocoder failed")
    with pytest.raises(RuntimeError, match="vocoder failed"):
        ss.step(8)  # request 0 finished in this step (6 frames), request 1 has its first 4 due: the failing call raises out of step()
    assert list(ss.live) == [1] and sess.released == [0] and list(codec.open) == [1]
    ss.close()
    assert codec.open == {}


def test_ragged_false_keeps_the_call_sequence():
    """the default scheduling is untouched: same script, same `calls`, as recorded from the scheduling before the ragged call existed"""
    ss, codec, _, _ = _drive([16 + 32 + 5, 9, 40, 100], [0, 0, 0, 2], k=8, chunk=32, first_chunk=16)
    ss2, codec2, _, _ = _drive([16 + 32 + 5, 9, 40, 100], [0, 0, 0, 2], k=8, chunk=32, first_chunk=16, ragged=False)
    assert ss.calls == ss2.calls and codec.calls == codec2.calls
    assert codec.ragged_calls == []
    assert ss.calls == [(2, "chunk", 2, 16), (2, "halo", 1, 9), (4, "chunk", 1, 16), (5, "tail", 1, 24), (6, "chunk", 1, 32),
                        (7, "halo", 1, 5), (8, "chunk", 1, 32), (12, "chunk", 1, 32), (15, "tail", 1, 20)], ss.calls
