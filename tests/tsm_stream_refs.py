"""The referee of the chunked time-stretch tests (tests/test_tsm_stream_plan_cpu.py, tests/test_tsm_stream_gpu.py,
tests/test_codec_speed_stream_gpu.py): the emission rule of include/fishrt.h ("Streams") restated in numpy / plain Python on top of
tests/tsm_refs.py -- when a frame may be emitted, where the carry starts, how long it can get -- and the chunkings the GPU tests cut their
signals into.  Nothing here touches the library.

The rule is a function of counters alone: n, the input samples a stream has seen.  With q_k = floor(k Hs speed + 0.5) (f64), hi_k = lo_k = 0
for k == 0, else hi_k = q_k + D, lo_k = q_k - D, frame k is emittable at n before the final item iff
    (k + 1) Hs <= out_len(n);   k == 0: Hs <= n;   k >= 1: q_k + D + N <= n and hi_{k-1} + Hs + N <= n
and a call emits the longest prefix of frames not yet emitted.  The final item emits all frames up to ceil(out_len(n) / Hs), the last one cut
at out_len(n).  The carry of a stream whose next frame is k starts at max(0, min(lo_k, lo_{k-1} + Hs)) (k == 0: 0)."""
import math

import numpy as np

import tsm_refs as R

SPEEDS = (0.25, 0.5, 0.77, 1.0, 1.25, 2.0, 3.0, 4.0)
PARAMS = ((1024, 512), (64, 0), (66, 3), (256, 64), (2048, 1024))


def out_len(n, speed):
    return int(np.floor(np.float64(n) / np.float64(speed) + 0.5)) if n > 0 else 0


def q_of(k, speed, N=R.FRAME):
    return int(np.floor(np.float64(k * (N // 2)) * np.float64(speed) + 0.5))


def hi_of(k, speed, N=R.FRAME, D=R.RADIUS):
    return 0 if k <= 0 else q_of(k, speed, N) + D


def lo_of(k, speed, N=R.FRAME, D=R.RADIUS):
    return 0 if k <= 0 else q_of(k, speed, N) - D


def emittable(k, n, speed, N=R.FRAME, D=R.RADIUS):
    hs = N // 2
    if (k + 1) * hs > out_len(n, speed):
        return False
    if k == 0:
        return hs <= n
    return q_of(k, speed, N) + D + N <= n and hi_of(k - 1, speed, N, D) + hs + N <= n


def carry_start(k, speed, N=R.FRAME, D=R.RADIUS):
    if k <= 0:
        return 0
    return max(0, min(lo_of(k, speed, N, D), lo_of(k - 1, speed, N, D) + N // 2))


def carry_bound(speed, N=R.FRAME, D=R.RADIUS):
    """the bound derived in csrc/fs_tsm_plan.h: carry < max(g + 0.5, D + N, D + N + Hs - g + 1) + max(D, g + 1 + D - Hs), g = Hs * speed,
    both terms rounded up (the first from g + 1)"""
    hs = N // 2
    g = hs * float(speed)
    return math.ceil(max(g + 1.0, D + N, D + N + hs - g + 1.0)) + math.ceil(max(float(D), g + 1.0 + D - hs))


def reads(k, speed, N=R.FRAME, D=R.RADIUS):
    """[lo, hi) of the input indices frame k can read, p_{k-1} unknown (negative indices read zero and are left out)"""
    hs = N // 2
    if k == 0:
        return 0, hs
    q = q_of(k, speed, N)
    return max(0, min(q - D, lo_of(k - 1, speed, N, D) + hs)), max(q + D + N, hi_of(k - 1, speed, N, D) + hs + N)


def walk(chunks, speed, N=R.FRAME, D=R.RADIUS):
    """the books of a stream fed `chunks` (sample counts; the last one is the final item) -> one dict per chunk: n (after it), k0, k1,
    n_emit, carry_start (after it; n on the final item)"""
    hs, n, k, emitted, out = N // 2, 0, 0, 0, []
    for c, n_new in enumerate(chunks):
        n += int(n_new)
        k0 = k
        if c + 1 == len(chunks):
            ol = out_len(n, speed)
            k = max(k0, -(-ol // hs))
            n_emit, cs = max(0, ol - emitted), n
        else:
            while emittable(k, n, speed, N, D):
                k += 1
            n_emit, cs = (k - k0) * hs, min(n, carry_start(k, speed, N, D))
        emitted += n_emit
        out.append(dict(n=n, k0=k0, k1=k, n_emit=n_emit, carry_start=cs))
    return out


def emitted(chunks, speed, N=R.FRAME, D=R.RADIUS):
    return [s["n_emit"] for s in walk(chunks, speed, N, D)]


# ---- chunkings of an n-sample signal (sample counts; the last chunk is the final item)
def even(n, size):
    return [size] * (n // size) + ([n % size] if n % size else []) or [0]


def ragged(n, seed, lo=1, hi=3000):
    rng, out, left = np.random.RandomState(seed), [], n
    while left > 0:
        t = min(int(rng.randint(lo, hi + 1)), left)
        out.append(t)
        left -= t
    return out or [0]


def threshold_cut(n, speed, N=R.FRAME, D=R.RADIUS, before=0):
    """two chunks, the cut at q_k + D + N - before for the middle frame k whose region threshold lies inside the signal; None if there is none"""
    K = -(-out_len(n, speed) // (N // 2))
    ks = [k for k in range(1, K) if 1 < q_of(k, speed, N) + D + N < n]
    if not ks:
        return None
    t = q_of(ks[len(ks) // 2], speed, N) + D + N - before
    return [t, n - t]


def chunkings(n, speed, N=R.FRAME, D=R.RADIUS, seed=0):
    """name -> chunk list: one chunk; all 2048; all 300 (below Hs at the defaults: calls that only carry); a cut exactly at an emission
    threshold q_k + D + N and one sample before it; a seeded ragged list; the same with a trailing empty final chunk"""
    out = {"one": [n], "2048": even(n, 2048), "300": even(n, 300), "ragged": ragged(n, seed + 1)}
    out["ragged+flush"] = [c for c in ragged(n, seed + 2) if c] + [0]
    for before in (0, 1):
        cut = threshold_cut(n, speed, N, D, before)
        if cut is not None:
            out["threshold-%d" % before] = cut
    return out
