"""GPU: the chunked time stretch through its test hook (fs_selftest_tsm_chunks: one row, one plan step and one launch pair per chunk, the
carry rows and the position word of a speed stream carried between them; csrc/codec_tsm.hip).  Against the one-shot device call
(fs_time_stretch): positions and PCM np.array_equal, for every signal of tests/tsm_refs.py, six speeds and seven chunkings -- one chunk, all
2048, all 300 (below Hs: calls that only carry), a cut exactly at an emission threshold q_k + D + N and one sample before it, a seeded ragged
list, a trailing empty final chunk -- on the edge lengths 0, 1, 511, 512, 513 and at other (N, D); the samples every chunk emits equal the
numpy rule of tests/tsm_stream_refs.py.  Against the numpy referee: on the exact and crafted tiers the hook's positions equal the float64
chain and its PCM the float32 overlap-add, which anchors the comparison to something other than the one-shot kernel."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import fishrt
from fishrt._tsm import time_stretch_chunks

import tsm_refs as R
import tsm_stream_refs as S

SPEEDS = (0.25, 0.5, 0.8, 1.25, 2.0, 4.0)
SIGNALS = (("voiced", 20000, 1), ("noise", 12000, 5), ("periodic", 8000, 2), ("silence_gap", 12000, 4))


@functools.lru_cache(maxsize=None)
def _one_shot(kind, n, seed, speed, N=R.FRAME, D=R.RADIUS):
    y, pos = fishrt.time_stretch(R.signal(kind, n, seed), speed, return_positions=True, frame=N, radius=D)
    y.setflags(write=False)
    pos.setflags(write=False)
    return y, pos


def _check(x, chunks, speed, want_y, want_pos, N=R.FRAME, D=R.RADIUS, tag=None):
    y, emitted, pos = time_stretch_chunks(x, chunks, speed, frame=N, radius=D)
    assert emitted.tolist() == S.emitted(chunks, speed, N, D), (tag, "emitted")
    assert np.array_equal(pos, want_pos), (tag, "positions", np.flatnonzero(pos != want_pos)[:4].tolist() if pos.shape == want_pos.shape else pos.shape)
    assert y.shape == want_y.shape and np.array_equal(y, want_y), (tag, "pcm")
    return emitted


@pytest.mark.parametrize("speed", SPEEDS)
@pytest.mark.parametrize("sig", SIGNALS, ids=lambda s: s[0])
def test_chunked_equals_one_shot(sig, speed):
    kind, n, seed = sig
    x = R.signal(kind, n, seed)
    want_y, want_pos = _one_shot(kind, n, seed, speed)
    cuts = S.chunkings(n, speed, seed=seed)
    assert {"one", "2048", "300", "ragged", "ragged+flush", "threshold-0", "threshold-1"} <= set(cuts)
    for name, chunks in cuts.items():
        emitted = _check(x, chunks, speed, want_y, want_pos, tag=(kind, speed, name))
        if name == "300":
            assert (emitted[:-1] == 0).any()  # calls that only carry
        if name == "ragged+flush":
            assert chunks[-1] == 0
    # q_k + D + N is the binding clause of frame k for 1 <= speed <= 3 at the defaults: below 1 the template clause hi_{k-1} + Hs + N lies
    # above it (q_k - q_{k-1} < Hs), above 3 the out_len clause does (Hs * speed > D + N).  Where it binds, the cut at it lets one more frame
    # out of the first call than the cut one sample before it
    a, b = S.emitted(cuts["threshold-0"], speed), S.emitted(cuts["threshold-1"], speed)
    assert a[0] - b[0] == (512 if 1.0 <= speed <= 3.0 else a[0] - b[0]) and a[0] - b[0] in (0, 512), (speed, a, b)


@pytest.mark.parametrize("n", [0, 1, 511, 512, 513])
def test_edge_lengths(n):
    x = R.noise(max(n, 1), 11)[:n]
    for speed in SPEEDS:
        want_y, want_pos = fishrt.time_stretch(x, speed, return_positions=True) if n else (np.zeros(0, np.float32), np.zeros(0, np.int64))
        assert len(want_y) == S.out_len(n, speed)
        for chunks in ([n], [n, 0], [n // 2, n - n // 2], [1, n - 1] if n else [0, 0], [n - n // 3, n // 3, 0]):
            _check(x, chunks, speed, want_y, want_pos, tag=(n, speed, chunks))


@pytest.mark.parametrize("N,D", [(64, 0), (66, 3), (2048, 1024)])
def test_other_parameters(N, D):
    kind, n, seed = "noise", 12000, 5
    x = R.signal(kind, n, seed)
    for speed in (0.5, 1.25, 4.0):
        want_y, want_pos = _one_shot(kind, n, seed, speed, N, D)
        cuts = S.chunkings(n, speed, N, D, seed=7)
        for name in ("300", "ragged", "ragged+flush", "threshold-0", "threshold-1"):
            _check(x, cuts[name], speed, want_y, want_pos, N, D, tag=(N, D, speed, name))
        # chunks of a few samples around every threshold of the small frames
        if N <= 66:
            _check(x[:1500], S.ragged(1500, 9, 1, 7), speed, *fishrt.time_stretch(x[:1500], speed, return_positions=True, frame=N, radius=D), N, D,
                   tag=(N, D, speed, "tiny chunks"))


@pytest.mark.parametrize("case", R.EXACT + R.CRAFTED, ids=lambda c: "%s-%d-%d-%g" % c)
def test_hook_equals_the_numpy_referee(case):
    kind, n, seed, speed = case
    x = R.signal(kind, n, seed)
    want_pos = R.chain_of(kind, n, seed, speed)[0]  # float64 chain; these tiers have no near-tie frame (tests/test_tsm_ref_cpu.py)
    _check(x, S.ragged(n, seed + 40, 1, 2500), speed, R.ola_f32(x, want_pos, speed), want_pos, tag=case)


def test_hook_validates_its_arguments():
    x = R.signal("noise", 12000, 5)[:3000]
    with pytest.raises(RuntimeError, match="add up"):
        time_stretch_chunks(x, [1000, 1000], 1.25)
    with pytest.raises(RuntimeError, match="speed"):
        time_stretch_chunks(x, [3000], 5.0)
    with pytest.raises(RuntimeError, match="frame"):
        time_stretch_chunks(x, [3000], 1.25, frame=65)
