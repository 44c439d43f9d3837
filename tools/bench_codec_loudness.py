"""One vocoder call to s16 at 24 kHz in host memory with loudness=-18: what the device stage costs, what the host path it replaces costs,
and whether the calls without the stage still cost what they did (profiles/codec_loudness.json).

Per call shape -- 8 rows x 32 frames and 32 rows x 16 frames -- the wall time of one FireflyCodec.decode call:
  (a) loud     decode(codes, sample_rate=24000, resample="sinc", dtype="s16", loudness=-18)   (fs_codec_decode_loud)
  (b) plain    the same call without loudness=                                                 (fs_codec_decode_pcm)
  (c) host     decode(codes) -- f32 at full length to the host -- then the definition on the host: the two K-weighting biquads as serial
               f64 IIR passes (scipy.signal.lfilter), hop sums, blocks and both gates in numpy, the gain multiply.  The resample and the
               s16 pack that (a) and (b) include are NOT in this figure: it is the round trip and the measurement alone.
With --parent-lib (a libfishrt.so built from the parent commit) the calls this change does not mean to touch, build against build:
  (d) pcm      decode(codes, sample_rate=24000, resample="sinc", dtype="s16")                  this build / the parent build
  (e) speed    the same with speed=1.25 (fs_codec_decode_speed)                                this build / the parent build
Every mode runs in a process of its own and the modes alternate, --reps rounds; the figure of a mode is the median over rounds of the
per-process median over its timed calls after its warm-up calls, given with its smallest and largest round.

usage: bench_codec_loudness.py [--reps 5] [--calls 30] [--warmup 5] [--parent-lib path] [--out profiles/codec_loudness.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(8, 32), (32, 16)]
TARGET, RATE = -18.0, 44100
SPEC = dict(sample_rate=24000, resample="sinc", dtype="s16")


def loudness_host(x, rate):
    """L of one row by the definition of include/fishrt.h, on the host"""
    import math
    import numpy as np
    from scipy.signal import lfilter

    def biquad(f0, Q, shelf_db=None):
        K = math.tan(math.pi * f0 / rate)
        a0 = 1.0 + K / Q + K * K
        a = [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
        if shelf_db is None:
            return [1.0, -2.0, 1.0], a
        Vh = 10.0 ** (shelf_db / 20.0)
        Vb = Vh ** 0.4996667741545416
        return [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0], a

    z = lfilter(*biquad(1681.974450955533, 0.7071752369554196, 3.999843853973347), x.astype(np.float64))
    z = lfilter(*biquad(38.13547087602444, 0.5003270373238773), z)
    h = (rate + 5) // 10
    nb = len(z) // h
    if nb < 4:
        return -math.inf
    s = (z[:nb * h] ** 2).reshape(nb, h).sum(1)
    m = (s[:-3] + s[1:-2] + s[2:-1] + s[3:]) / (4.0 * h)
    with np.errstate(divide="ignore"):
        l = -0.691 + 10.0 * np.log10(m)
    keep = l > -70.0
    if not keep.any():
        return -math.inf
    keep &= l > -0.691 + 10.0 * math.log10(m[keep].mean()) - 10.0
    return -0.691 + 10.0 * math.log10(m[keep].mean()) if keep.any() else -math.inf


def child(mode, calls, warmup, lib):
    sys.path.insert(0, os.path.join(ROOT, "fish-speech.rs_amd"))
    import numpy as np
    from fishrt import _ffi
    if lib:
        _ffi.LIB_PATH = os.path.abspath(lib)
    import fishrt
    codec = fishrt.FireflyCodec(0).load_synthetic(0xC0DEC)
    rng = np.random.RandomState(1)
    out = {}
    for b, T in SHAPES:
        times, d2h = [], 0
        for k in range(warmup + calls):
            codes = rng.randint(0, 1000, (b, 8, T)).astype(np.uint32)
            t0 = time.perf_counter()
            if mode == "loud":
                pcm = codec.decode(codes, loudness=TARGET, **SPEC)
            elif mode in ("plain", "pcm"):
                pcm = codec.decode(codes, **SPEC)
            elif mode == "speed":
                pcm = codec.decode(codes, speed=1.25, **SPEC)
            else:
                pcm = codec.decode(codes)
                for i in range(b):
                    row = pcm[i, 0]
                    L = loudness_host(row, RATE)
                    pk = float(np.abs(row).max())
                    g = 1.0 if L == -np.inf else min(10.0 ** ((TARGET - L) / 20.0), 10.0 ** 1.5, 10.0 ** (-1.0 / 20.0) / pk if pk > 0 else np.inf)
                    row *= np.float32(g)
            t1 = time.perf_counter()
            d2h = pcm.nbytes
            if k >= warmup:
                times.append((t1 - t0) * 1e3)
        out[f"{b}x{T}"] = dict(ms=statistics.median(times), d2h_bytes=int(d2h))
    codec.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "codec_loudness.json"))
    ap.add_argument("--child", default=None)
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.calls, a.warmup, a.lib)
    modes = [("loud", "loud", None), ("plain", "plain", None), ("host", "host", None)]
    if a.parent_lib:
        modes += [("pcm_this", "pcm", None), ("pcm_parent", "pcm", a.parent_lib), ("speed_this", "speed", None), ("speed_parent", "speed", a.parent_lib)]
    runs = {name: [] for name, _, _ in modes}
    for _ in range(a.reps):
        for name, mode, lib in modes:  # alternating processes
            cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--calls", str(a.calls), "--warmup", str(a.warmup)]
            if lib:
                cmd += ["--lib", lib]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True, timeout=600, check=True)
            runs[name].append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    res = dict(protocol=f"{a.reps} rounds of alternating processes, median of {a.calls} calls after {a.warmup}; loudness {TARGET} LUFS, s16 at 24 kHz "
                        "(sinc); ms = median over rounds, ms_min / ms_max = smallest / largest round", shapes={})
    if not a.parent_lib:
        res["against_the_parent_build"] = "not measured yet"
    for b, T in SHAPES:
        key, row = f"{b}x{T}", {}
        for name, _, _ in modes:
            vals = [r[key]["ms"] for r in runs[name]]
            row[name] = dict(ms=statistics.median(vals), ms_min=min(vals), ms_max=max(vals), d2h_bytes=runs[name][0][key]["d2h_bytes"])
        res["shapes"][key] = row
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
