"""CPU: fishrt.SessionStreamer's scheduling against a fake session and a fake codec (no GPU): chunk boundaries and the first-chunk size,
one vocoder call per distinct chunk length per step with a uniform T, short tails through the halo path, streams closed and slots released
when a request finishes, errors surfacing to the caller -- and every request's pieces concatenated equal a one-shot decode of its codes."""
import numpy as np
import pytest

from fishrt.stream import SessionStreamer

SPF = 4  # samples per frame of the fake codec (the real one has 2048; the scheduling does not depend on it)


def _pcm_of(codes):
    """fake vocoder: frame t's samples are code[0, t] + (0, 0.25, 0.5, 0.75) -- a one-shot decode is just this map"""
    return (codes[0].astype(np.float32)[:, None] + np.arange(SPF, dtype=np.float32)[None] / SPF).reshape(-1)


class FakeCodec:
    STREAM_MIN_FRAMES = 16

    def __init__(self):
        self.open, self.next_id, self.calls, self.decode_calls, self.fail_next = {}, 0, [], [], None

    def streams_open(self):
        sid = self.next_id
        self.next_id += 1
        self.open[sid] = 0
        return sid

    def streams_close(self, sid):
        del self.open[sid]

    def streams_decode(self, ids, codes):
        if self.fail_next:
            e, self.fail_next = self.fail_next, None
            raise e
        codes = np.asarray(codes)
        assert codes.ndim == 3 and codes.shape[0] == len(ids) and codes.shape[2] >= self.STREAM_MIN_FRAMES
        assert len(set(ids)) == len(ids) and all(i in self.open for i in ids)
        self.calls.append((list(ids), codes.shape[2]))
        for i in ids:
            self.open[i] += codes.shape[2]
        return np.stack([_pcm_of(c) for c in codes])

    def decode(self, codes):  # the halo path (stream.decode_chunk)
        self.decode_calls.append(codes.shape)
        return _pcm_of(codes[0])[None, None]


class FakeSession:
    """slots generate their predetermined code sequences, one frame per slot per step frame"""

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


def _drive(lengths, joins, k, chunk=32, first_chunk=16):
    """joins[i] = the step before which request i is added; returns (streamer, codec, pieces per request, calls per step)"""
    seqs = _seqs(lengths)
    sess, codec, pieces = FakeSession(seqs), FakeCodec(), {i: [] for i in range(len(lengths))}
    finals = []
    ss = SessionStreamer(sess, codec, chunk=chunk, first_chunk=first_chunk,
                         on_audio=lambda tag, pcm, final: (pieces[tag].append(pcm), final and finals.append(tag)))
    step, pending = 0, list(range(len(lengths)))
    while pending or ss.live:
        for i in [i for i in pending if joins[i] <= step]:
            if ss.add(i, 0, tag=i) is not None:
                pending.remove(i)
        ss.step(k)
        step += 1
        assert step < 1000
    assert sorted(finals) == list(range(len(lengths)))
    return ss, codec, seqs, pieces


def test_pieces_concatenate_to_one_shot_decode_and_chunk_boundaries():
    lengths, joins = [200, 75, 16, 9, 130, 47], [0, 0, 2, 3, 5, 9]
    ss, codec, seqs, pieces = _drive(lengths, joins, k=8)
    for i, seq in enumerate(seqs):
        got = np.concatenate(pieces[i])
        assert np.array_equal(got, _pcm_of(seq)), i
        assert np.array_equal(ss.results[i], seq)
        sizes = [len(p) // SPF for p in pieces[i]]
        assert sum(sizes) == seq.shape[1]
        # first piece = first_chunk, then chunk-sized pieces, then the tail (whatever remains when the request finishes)
        if seq.shape[1] > 16:
            assert sizes[0] == 16, (i, sizes)
            assert all(s == 32 for s in sizes[1:-1]), (i, sizes)
        st = ss.stats[i]
        assert st["frames"] == seq.shape[1] and st["chunks"] == len(sizes) and st["first_audio_s"] is not None


def test_uniform_T_and_one_call_per_distinct_T_per_step():
    ss, codec, _, _ = _drive([300, 280, 260, 90, 64], [0, 0, 1, 4, 7], k=16)
    per_step = {}
    for q, kind, n, T in ss.calls:
        if kind == "chunk":
            per_step.setdefault(q, []).append(T)
    assert per_step and all(len(Ts) == len(set(Ts)) for Ts in per_step.values()), per_step
    assert any(n > 1 for _, kind, n, _ in ss.calls if kind == "chunk")  # requests share vocoder calls
    for ids, T in codec.calls:  # every call: one T for all items (the fake codec's array is (n, 8, T))
        assert T >= 16
    assert all(n == 1 for _, kind, n, _ in ss.calls if kind != "chunk")


def test_short_tails_take_the_halo_path_and_streams_close():
    ss, codec, seqs, pieces = _drive([16 + 32 + 5, 9, 40], [0, 0, 0], k=8)
    kinds = {(kind, T) for _, kind, _, T in ss.calls}
    assert ("halo", 5) in kinds and ("halo", 9) in kinds  # < 16 frames left at the end: stateless decode with a halo
    assert ("tail", 24) in kinds                          # >= 16 left: one more stateful chunk of n = 1
    assert len(codec.decode_calls) == 2
    assert codec.open == {}  # every stream closed on finish
    assert sorted(ss.session.released) == [0, 1, 2] and ss.live == {}


def test_full_session_opens_nothing():
    sess, codec = FakeSession(_seqs([40] * 3), max_batch=2), FakeCodec()
    ss = SessionStreamer(sess, codec, chunk=32, first_chunk=16)
    assert ss.add(0, 0) == 0 and ss.add(1, 0) == 1
    assert ss.add(2, 0) is None
    assert len(codec.open) == 2
    ss.close()
    assert codec.open == {}


def test_errors_surface_to_the_caller():
    with pytest.raises(ValueError):
        SessionStreamer(FakeSession([]), FakeCodec(), chunk=8)
    sess, codec = FakeSession(_seqs([100, 100])), FakeCodec()
    ss = SessionStreamer(sess, codec, chunk=32, first_chunk=16)
    ss.add(0, 0)
    ss.add(1, 0)
    ss.step(8)
    codec.fail_next = RuntimeError("vocoder failed")
    with pytest.raises(RuntimeError, match="vocoder failed"):
        ss.step(8)  # 16 frames due for both: the failing call raises out of step()
    with pytest.raises(ValueError, match="already in use"):
        ss.add(1, 0, tag=0)
    ss.close()
    assert codec.open == {}
