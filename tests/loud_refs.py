"""The numpy / float64 referee of the loudness definition (include/fishrt.h "Device loudness normalisation"), written from that text and not
from csrc/fs_loud_plan.h: coefficients, a serial filter, hops, blocks, both gates, peak and gain; the case table of the GPU tests; and the
bound the device's hop energies are held to, derived below (hop_bound) from the f64 unit round-off, the filter's noise gain and the chunked
evaluation order -- not from anything a device returned."""
import functools
import math

import numpy as np
from scipy.signal import fftconvolve, lfilter
from scipy.ndimage import maximum_filter1d

U = 2.0 ** -53  # unit round-off of f64
CHUNK, WG = 32, 256  # samples a lane filters and lanes of a workgroup (csrc/fs_loud_plan.h): only the bound and the case lengths use them
SPAN = CHUNK * WG
PEAK_DB, MAX_GAIN_DB = -1.0, 30.0


def coefs(rate):
    """((b0, b1, b2, a1, a2) of the shelf, (d1, d2) of the high-pass whose numerator is 1, -2, 1)"""
    K = math.tan(math.pi * 1681.974450955533 / rate)
    Vh = 10.0 ** (3.999843853973347 / 20.0)
    Vb = Vh ** 0.4996667741545416
    Q = 0.7071752369554196
    a0 = 1.0 + K / Q + K * K
    shelf = ((Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0, 2.0 * (K * K - 1.0) / a0,
             (1.0 - K / Q + K * K) / a0)
    K = math.tan(math.pi * 38.13547087602444 / rate)
    Q = 0.5003270373238773
    a0 = 1.0 + K / Q + K * K
    return shelf, (2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0)


def hop(rate):
    return (rate + 5) // 10


def kweight(x, rate, amp=False):
    """z of the definition, sample by sample in Python floats (f64, no fma).  amp: also A_n, the sum of the absolute values of every term
    the step at sample n rounds (hop_bound)"""
    (b0, b1, b2, a1, a2), (d1, d2) = coefs(rate)
    s0 = s1 = s2 = s3 = 0.0
    xs = np.asarray(x, np.float32).astype(np.float64).tolist()
    z_out = [0.0] * len(xs)
    a_out = [0.0] * len(xs) if amp else None
    for i, v in enumerate(xs):
        y = b0 * v + s0
        if amp:
            zz = y + s2
            a_out[i] = (abs(b0 * v) + abs(s0) + abs(b1 * v) + abs(a1 * y) + abs(s1) + abs(b2 * v) + abs(a2 * y) + 4.0 * abs(y) + abs(s2) + abs(d1 * zz)
                        + abs(s3) + abs(d2 * zz))
        s0 = b1 * v - a1 * y + s1
        s1 = b2 * v - a2 * y
        z = y + s2
        s2 = -2.0 * y - d1 * z + s3
        s3 = y - d2 * z
        z_out[i] = z
    z = np.array(z_out, np.float64)
    return (z, np.array(a_out, np.float64)) if amp else z


def hop_sums(z, rate):
    h = hop(rate)
    nb = len(z) // h
    return np.array([math.fsum((z[i * h:(i + 1) * h] ** 2).tolist()) for i in range(nb)], np.float64)  # (fsum: the sum itself adds no error)


def lufs_of(m):
    with np.errstate(divide="ignore", invalid="ignore"):
        return -0.691 + 10.0 * np.log10(m)


def gate(s, rate, absolute=True, relative=True):
    """dict(lufs, blocks_total, blocks_kept, l, gamma) from the hop energies; absolute / relative = False disables that gate (the teeth)"""
    h, nb = hop(rate), len(s)
    out = dict(lufs=-math.inf, blocks_total=max(nb - 3, 0), blocks_kept=0, l=np.zeros(0), gamma=math.nan)
    if nb < 4:
        return out
    m = (s[:-3] + s[1:-2] + s[2:-1] + s[3:]) / (4.0 * h)
    l = lufs_of(m)
    out["l"] = l
    k1 = (l > -70.0) if absolute else ~np.isnan(l)
    if not k1.any():
        return out
    gamma = float(lufs_of(np.mean(m[k1]))) - 10.0
    out["gamma"] = gamma
    k2 = k1 & (l > gamma) if relative else k1
    if not k2.any():
        return out
    out["blocks_kept"] = int(k2.sum())
    out["lufs"] = float(lufs_of(np.mean(m[k2])))
    return out


def peak(x):
    a = np.abs(np.asarray(x, np.float32))
    a = a[~np.isnan(a)]
    return np.float32(a.max()) if a.size else np.float32(0.0)


def gain(lufs, pk, target, peak_db=PEAK_DB, max_gain_db=MAX_GAIN_DB):
    if not lufs > -math.inf:
        return np.float32(1.0)
    g = min(10.0 ** ((target - lufs) / 20.0), 10.0 ** (max_gain_db / 20.0))
    if pk > 0:
        g = min(g, 10.0 ** (peak_db / 20.0) / float(pk))
    return np.float32(g)


def measure(x, rate, **gates):
    s = hop_sums(kweight(x, rate), rate)
    r = gate(s, rate, **gates)
    r["s"], r["peak"] = s, peak(x)
    return r


# ---- the bound on a hop energy.  The device and this referee evaluate the same recurrence; they differ by rounding alone.
#
# (1) One step.  A step of the cascade rounds at most 4 times in any one of its six expressions, each rounding at most U times the sum of the
#     absolute values of that expression's terms; y and z, rounded in the same step, enter the state updates through |a1|, |a2|, |d1|, |d2| < 2
#     and the constant 2.  With A_n the sum of the absolute values of ALL terms of step n (kweight(amp=True)), no state component is left
#     more than C1 U A_n from the exact step, C1 = 16 (4 roundings of its own + 2 x 2 + 2 x 1 + 2 x 1 passed on from y and z, rounded up to a
#     power of two).  An fma removes roundings, never adds one.
# (2) Noise gain.  An error e in state component j at step n moves z at step n + k by G_j[k] e, G_j the zero-input response.  The poles of the
#     high-pass have radius rho = sqrt(d2), within 6e-3 of the unit circle at every rate up to 48 kHz, and nearly coincide (Q = 0.5003), so
#     |G_j[k]| <= Cg (k + 1) rho^k, the response of a double pole at rho; Cg = max over j and k of |G_j[k]| / ((k + 1) rho^k) is computed from
#     the coefficients (noise_gain), not assumed, and the four components add: the error of z at step t from the steps alone is at most
#         E1[t] = sum_n 4 Cg (t - n + 1) rho^(t - n) C1 U A_n,
#     which is A filtered by 1 / (1 - rho z^-1)^2.  Sum_k (k + 1) rho^k = 1 / (1 - rho)^2, about 4e4 at 48 kHz: that is the noise gain.
# (3) Chunked order.  The device enters every chunk of 32 samples with a state it composed from partial states: M^(2^k) s' + s over 8 scan
#     steps, one table product M^l s_wg, one product per workgroup on the way.  Every s', s there is the zero-state response to a sub-range of
#     the input, so each of its components is bounded by B[t] = sum_n Habs[t - n] |x_n|, Habs[k] the largest state component k steps after a
#     unit input sample (computed from the coefficients; its sum is about 5, not the 1 / (1 - rho)^2 of (2): the numerator 1, -2, 1 keeps the
#     input out of the slow mode).  A composition is four 4-term dot products plus one addition: 8 roundings of at most U (4 Pmax B' + B),
#     Pmax the largest entry of any power of the transition matrix (computed) and B' the bound at the earlier time, inside the same workgroup
#     span; the table entries are computed in extended precision and rounded once, within U Pmax each: 4 U Pmax B' more.  With D = 10 levels
#     and B over the span's window taken as its maximum, a chunk entry is off by at most 9 D U (4 Pmax + 1) max(B[t - SPAN .. t]) on top of
#     (1), injected at every chunk boundary and carried on by (2).
# (4) A hop.  With E = 2 E1 + E2 (this referee makes the errors of (1) too; E2 is (3) carried by (2)):
#         |s_dev - s_ref| <= sum over the hop of (2 |z| E + E^2)  +  (h + 64) U s_i,
#     the last term for the two summation orders (fsum here; on the device 32 serial additions, 3 partials, a 6-level butterfly, h / 2048 strided).
# The result is a bound per hop, relative to that hop's own energy through |z|: in a silent gap E decays with the state it is relative to.
C1, LEVELS = 16.0, 10.0


@functools.lru_cache(None)
def noise_gain(rate):
    """(rho, Cg, Pmax, Habs) of (2) and (3), from the coefficients"""
    (b0, b1, b2, a1, a2), (d1, d2) = coefs(rate)
    A = np.array([[-a1, 1, 0, 0], [-a2, 0, 0, 0], [-2.0 - d1, 0, -d1, 1], [1.0 - d2, 0, -d2, 0]], np.float64)
    rho = math.sqrt(d2)
    S = np.eye(4)
    cg = pmax = 0.0
    v = np.array([b1 - a1 * b0, b2 - a2 * b0, -2.0 * b0 - d1 * b0, b0 - d2 * b0])  # the state one unit input sample leaves
    habs = []
    for k in range(60000):
        env = (k + 1) * rho ** k
        if env < 1e-18:
            break
        habs.append(float(np.max(np.abs(S @ v))))
        # z at step n + k from a unit error in component j at step n: (1, 0, 1, 0) . A^k e_j  (z = y + s2, y = s0 with zero input)
        cg = max(cg, float(np.max(np.abs(S[0] + S[2])) / env))
        if k:
            pmax = max(pmax, float(np.max(np.abs(S))))
        S = A @ S
    return rho, cg, pmax, np.array(habs)


def hop_bound(x, rate):
    """absolute bound on |s_dev - s_ref| per whole hop, (1) .. (4) above"""
    (b0, b1, b2, a1, a2), _ = coefs(rate)
    z, A = kweight(x, rate, amp=True)
    ok = np.isfinite(z)
    z, A = np.where(ok, z, 0.0), np.where(ok, A, 0.0)  # (a NaN row: its hops from the NaN on are NaN on both sides and compared as such)
    rho, cg, pmax, habs = noise_gain(rate)
    den = [1.0, -2.0 * rho, rho * rho]
    E1 = lfilter([4.0 * cg * C1 * U], den, A)
    xa = np.abs(np.nan_to_num(np.asarray(x, np.float32).astype(np.float64)))
    B = np.abs(fftconvolve(xa, habs)[:len(xa)]) * (1.0 + 1e-9) + 1e-12 * (xa.max() if len(xa) else 0.0)  # (the FFT's own rounding)
    Bw = maximum_filter1d(B, size=2 * SPAN + 1, mode="constant")  # (centred window: covers [t - SPAN, t])
    inj = np.zeros_like(B)
    inj[::CHUNK] = 9.0 * LEVELS * U * (4.0 * pmax + 1.0) * Bw[::CHUNK]
    E2 = lfilter([4.0 * cg], den, inj)
    E = 2.0 * E1 + E2
    h = hop(rate)
    nb = len(z) // h
    s = hop_sums(z, rate)
    return np.array([np.sum(2.0 * np.abs(z[i * h:(i + 1) * h]) * E[i * h:(i + 1) * h] + E[i * h:(i + 1) * h] ** 2) for i in range(nb)]) + (h + 64) * U * s


# ---- signals and the case table
def signal(kind, n, rate, seed=0):
    rng = np.random.RandomState(seed)
    t = np.arange(n, dtype=np.float64) / rate
    sine = np.sin(2.0 * np.pi * 997.0 * t)
    noise = rng.uniform(-1.0, 1.0, n)
    if kind == "sine":
        x = sine
    elif kind == "mix":
        x = 0.3 * sine + 0.1 * noise
    elif kind == "gap":  # 5 hops of noise, 12 hops of digital silence, a burst 16.7 dB down: the 9 silent blocks fall to the absolute gate,
        # which lifts the relative gate over the second burst; without the absolute gate that burst is kept (test_loud_ref_cpu.py)
        h = hop(rate)
        x = 0.05 * 10.0 ** (-17.3 / 20.0) * noise
        x[5 * h:17 * h] = 0.0
        x[17 * h:] *= 10.0 ** (-16.67 / 20.0)
    elif kind == "quiet":  # a loud passage, then one 15 LU quieter: it falls to the relative gate
        x = 0.25 * noise
        x[n // 2:] *= 10.0 ** (-15.0 / 20.0)
    elif kind == "spike":  # quiet, one full-scale sample: the peak clause decides the gain
        x = 0.002 * noise
        x[n // 3] = 1.0
    elif kind == "under":  # 50 LU under a target of -18: max_gain_db decides
        x = 10.0 ** ((-68.0 + 3.0075) / 20.0) * sine
    elif kind == "nan":
        x = 0.3 * sine + 0.1 * noise
        x[int(0.83 * n)] = np.nan
    else:
        raise ValueError(kind)
    return x.astype(np.float32)


def edge_lengths(rate):
    h = hop(rate)
    return [4 * h - 1, 4 * h, 4 * h + 1, 5 * h - 1, SPAN + 4 * h + 1237]  # the last: no multiple of CHUNK or SPAN, two workgroups


RATES = (8000, 24000, 44100, 48000)
LONG = 66157  # 1.5 s at 44.1 kHz: nine workgroups, the last one partial
TARGET = -18.0
# (kind, n, rate, seed)
EDGES = [("mix", n, rate, 1) for rate in RATES for n in edge_lengths(rate)]
SIGNALS = [("sine", LONG, 44100, 0), ("mix", LONG, 44100, 2), ("gap", 25 * 4410 + 100, 44100, 3), ("quiet", LONG, 44100, 4), ("spike", LONG, 44100, 5),
           ("under", LONG, 44100, 0), ("nan", LONG, 44100, 6), ("mix", 72000, 48000, 7), ("mix", 3 * SPAN + 7, 8000, 8)]
CASES = EDGES + SIGNALS
GAP, QUIET = SIGNALS[2], SIGNALS[3]


@functools.lru_cache(None)
def reference(case):
    """the referee's record of a case, computed once and shared: dict(x, s, bound, lufs, blocks_total, blocks_kept, l, gamma, peak)"""
    kind, n, rate, seed = case
    x = signal(kind, n, rate, seed)
    r = measure(x, rate)
    r["x"], r["bound"] = x, hop_bound(x, rate)
    for v in (r["x"], r["s"], r["bound"]):
        v.setflags(write=False)
    return r


def case_id(case):
    return "%s-%d-%d-%d" % case
