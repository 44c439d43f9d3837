"""The referee of the time-stretch tests (tests/test_tsm_ref_cpu.py, tests/test_time_stretch_gpu.py): the definition in include/fishrt.h
(WSOLA with a squared-difference measure) restated in numpy, the test signals and the case table.  Nothing here touches the library.

plan / ola_f32 are exact restatements: lengths and nominal positions in f64, the overlap-add in numpy float32 (two products rounded
separately, one add), which the device must match bit for bit.  The search is refereed in float64: errors64 gives every lag's error of a
frame, chain64 the whole chain with the tie rule.  The device accumulates N non-negative f32 terms per lag, each the square of a rounded
difference, so a computed error lies within (N + 3) * 2^-24 of its value, relatively; two lags can therefore swap only when
    e64[pick] <= e64[best] + tol,  tol = 2 * (N + 3) * 2^-24 * e64[pick]
and that is the admission test of `replay` -- derived, not tuned.  A frame is a NEAR-TIE frame when a lag other than the f64 winner passes
that test while the winner's error is positive (an exact 0 is exact in f32 as well); only there may the device differ from chain64.

Signals (44.1 kHz, float32):
  voiced(n, seed)    11 harmonics with 1/h amplitudes and random phases on a fundamental gliding from 110 Hz to about 190 Hz over the clip
                     with a 0.7 Hz wobble of 4 Hz depth, a 3 Hz amplitude envelope (0.6 + 0.4 sin), overall gain 0.2, plus N(0, 0.005) noise
  noise(n, seed)     uniform(-1, 1)
  periodic(n, seed)  a 147-sample random pattern repeated bit for bit
  silence_gap(n, seed)  voiced with 3000 exact zeros in the middle"""
import functools

import numpy as np

FRAME, RADIUS = 1024, 512
RATE = 44100
U = 2.0 ** -24


# ---- signals
def voiced(n, seed):
    rng = np.random.RandomState(seed)
    t = np.arange(n) / RATE
    f0 = 110.0 + 80.0 * t / max(n / RATE, 1e-9) + 4.0 * np.sin(2 * np.pi * 0.7 * t)
    phase = 2 * np.pi * np.cumsum(f0) / RATE
    phis = rng.uniform(0, 2 * np.pi, 11)
    s = sum(np.sin(h * phase + phis[h - 1]) / h for h in range(1, 12))
    env = 0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t)
    return (0.2 * env * s + rng.normal(0.0, 0.005, n)).astype(np.float32)


def noise(n, seed):
    return np.random.RandomState(seed).uniform(-1, 1, n).astype(np.float32)


def periodic(n, seed):
    pat = np.random.RandomState(seed).uniform(-1, 1, 147).astype(np.float32)
    return np.ascontiguousarray(np.tile(pat, n // 147 + 1)[:n])


def silence_gap(n, seed):
    x = voiced(n, seed)
    x[n // 2 - 1500:n // 2 + 1500] = 0.0
    return x


SIGNALS = dict(voiced=voiced, noise=noise, periodic=periodic, silence_gap=silence_gap)

# (signal, n, seed, speed).  EXACT: chain64 has no near-tie frame, so the device's positions must equal it.  REFEREED: it has some (one
# frame in 29 .. 46 here).  tests/test_tsm_ref_cpu.py asserts the tier of every case; with this file's `voiced` the two voiced cases at the
# end of EXACT have no near-tie frame, so they sit in that tier.
EXACT = ([("voiced", 20000, 1, s) for s in (0.5, 0.77, 0.8, 1.25, 2.0)] + [("noise", 12000, 5, s) for s in (0.77, 1.25, 2.0, 3.0)]
         + [("voiced", 20000, 1, 3.0), ("voiced", 9000, 3, 1.25)])
REFEREED = [("noise", 12000, 5, 0.5), ("noise", 12000, 5, 0.8)]
CRAFTED = [("periodic", 8000, 2, 1.25), ("periodic", 8000, 2, 0.8), ("silence_gap", 12000, 4, 1.25), ("silence_gap", 12000, 4, 0.77)]


@functools.lru_cache(maxsize=None)
def signal(kind, n, seed):
    x = SIGNALS[kind](n, seed)
    x.setflags(write=False)
    return x


# ---- the definition
def plan(n, speed, N=FRAME):
    """-> (out_len, K, q int64 [K])"""
    hs = N // 2
    out_len = int(np.floor(np.float64(n) / np.float64(speed) + 0.5)) if n > 0 else 0
    K = -(-out_len // hs)
    q = np.floor((np.arange(K, dtype=np.int64) * hs).astype(np.float64) * np.float64(speed) + 0.5).astype(np.int64)
    return out_len, K, q


def window(N=FRAME):
    return (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N, dtype=np.float64) / N)).astype(np.float32)


_LEFT, _RIGHT = 4096, 12288  # zeros around x: every index a frame can read lies inside (q_k < n + 4 * 1024 + 2, plus D + N)


def _padded(x, dtype):
    return np.concatenate([np.zeros(_LEFT, dtype), np.asarray(x, dtype), np.zeros(_RIGHT, dtype)])


def errors64(x, p_prev, q, N=FRAME, D=RADIUS, _xp=None):
    """e[d] for d = -D .. D (index d + D) of the frame whose predecessor sits at p_prev and whose nominal position is q, in float64"""
    xp = _padded(x, np.float64) if _xp is None else _xp
    t = xp[_LEFT + p_prev + N // 2:_LEFT + p_prev + N // 2 + N]
    reg = xp[_LEFT + q - D:_LEFT + q + D + N]
    win = np.lib.stride_tricks.sliding_window_view(reg, N)
    df = win - t
    return np.einsum("ij,ij->i", df, df)


def pick64(e, D=RADIUS):
    """the tie rule on exact values: smallest e, then smallest |d|, then the negative lag"""
    d = np.flatnonzero(e == e.min()) - D
    a = np.abs(d)
    d = d[a == a.min()]
    return int(d.min())


def tol_of(e, N=FRAME):
    return 2.0 * (N + 3) * U * e


def near_tie(e, D=RADIUS, N=FRAME):
    best = e.min()
    if not best > 0:
        return False
    ok = e <= best + tol_of(e, N)
    ok[pick64(e, D) + D] = False
    return bool(ok.any())


def chain64(x, speed, N=FRAME, D=RADIUS, pick=pick64):
    """-> (positions int64 [K], near-tie flags bool [K])"""
    _, K, q = plan(len(x), speed, N)
    xp = _padded(x, np.float64)
    pos, ties = np.zeros(K, np.int64), np.zeros(K, bool)
    for k in range(1, K):
        e = errors64(x, int(pos[k - 1]), int(q[k]), N, D, xp)
        pos[k] = q[k] + pick(e, D)
        ties[k] = near_tie(e, D, N)
    return pos, ties


@functools.lru_cache(maxsize=None)
def chain_of(kind, n, seed, speed):
    pos, ties = chain64(signal(kind, n, seed), speed)
    pos.setflags(write=False)
    return pos, ties


def replay(x, speed, positions, N=FRAME, D=RADIUS):
    """the f64 errors along GIVEN positions -> dict(admitted: every pick passes the admission test, differ: frames whose pick is not the f64
    winner, stray: such frames that are not near-tie frames, worst: the largest (e64[pick] - best) / tol)"""
    _, K, q = plan(len(x), speed, N)
    assert len(positions) == K and (K == 0 or positions[0] == 0)
    xp = _padded(x, np.float64)
    out = dict(admitted=True, differ=0, stray=0, worst=0.0, frames=max(K - 1, 0))
    for k in range(1, K):
        d = int(positions[k] - q[k])
        if abs(d) > D:
            out["admitted"] = False
            continue
        e = errors64(x, int(positions[k - 1]), int(q[k]), N, D, xp)
        best, mine = e.min(), e[d + D]
        tol = tol_of(mine, N)
        if not mine <= best + tol:
            out["admitted"] = False
        if mine > best:
            out["worst"] = max(out["worst"], float((mine - best) / tol))
        if d != pick64(e, D):
            out["differ"] += 1
            out["stray"] += not near_tie(e, D, N)
    return out


def cap_of(frames):
    """frames of a refereed case that may differ from the f64 winner: max(1, 5 %)"""
    return max(1, int(0.05 * frames))


def _gather(x, idx):
    ok = (idx >= 0) & (idx < len(x))
    return np.where(ok, x[np.clip(idx, 0, max(len(x) - 1, 0))] if len(x) else 0, 0).astype(x.dtype)


def ola_f32(x, p, speed, N=FRAME, fused=False):
    """the output along positions p, numpy float32: the two products rounded separately, then one add.  fused=True contracts the first
    product into the add (one rounding less), what a build without the explicit roundings would compute"""
    x = np.asarray(x, np.float32)
    out_len, K, _ = plan(len(x), speed, N)
    assert len(p) == K
    hs, w = N // 2, window(N)
    m = np.arange(out_len, dtype=np.int64)
    k, i = m // hs, m % hs
    y = _gather(x, m)
    late = k >= 1
    kk, ii = k[late], i[late]
    pv = np.asarray(p, np.int64)
    a, b = _gather(x, pv[kk - 1] + hs + ii), _gather(x, pv[kk] + ii)
    if fused:
        second = (w[ii] * b).astype(np.float64)
        y[late] = (w[ii + hs].astype(np.float64) * a.astype(np.float64) + second).astype(np.float32)
    else:
        y[late] = w[ii + hs] * a + w[ii] * b
    return y


def first_min(e, D=RADIUS):
    """a wrong tie rule for the teeth test: the first minimum in ascending d"""
    return int(np.argmin(e)) - D
