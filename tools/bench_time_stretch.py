"""One vocoder call to s16 host memory at speed 1.25: the device path against the host path it replaces (profiles/codec_speed.json).

Per call shape -- 8 rows x 32 frames and 32 rows x 16 frames -- the wall time of one FireflyCodec.decode call that ends with s16 PCM at
the codec's rate in host memory, and the bytes its D2H copy moves:
  (a) device   decode(codes, dtype="s16", speed=1.25)   (fs_codec_decode_speed: vocoder -> stretch -> s16, one D2H of the stretched s16)
  (b) host     decode(codes) -- f32 at full length to the host -- then a vectorised numpy restatement of the same definition (float32 error
               sums over the six segments, the tie rule, the float32 overlap-add) and pcm_to_i16
  (c) plain    decode(codes, dtype="s16")               (fs_codec_decode_pcm: the call without a stretch stage, for scale)
Every mode runs in a process of its own and the modes alternate, --reps rounds; the figure of a mode is the median over rounds of the
per-process median over its timed calls after its warm-up calls (the host mode takes --host-calls calls after one: a call is seconds).
The chain is serial over the frames of a row (about 86 per second of output), so the device figure grows with the row length, not with the
number of rows, until the rows outnumber the compute units.

usage: bench_time_stretch.py [--reps 3] [--calls 20] [--warmup 5] [--host-calls 3] [--out profiles/codec_speed.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(8, 32), (32, 16)]
MODES = ["device", "host", "plain"]
SPEED = 1.25
N, HS, D, SEGS = 1024, 512, 512, 6


def stretch_numpy(x, speed):
    """the definition of include/fishrt.h in float32 numpy, one row"""
    import numpy as np
    n = len(x)
    out_len = int(np.floor(np.float64(n) / np.float64(speed) + 0.5))
    K = -(-out_len // HS)
    q = np.floor((np.arange(K, dtype=np.int64) * HS).astype(np.float64) * np.float64(speed) + 0.5).astype(np.int64)
    left = 2048
    xp = np.concatenate([np.zeros(left, np.float32), x, np.zeros(8192, np.float32)])
    seg = -(-N // SEGS)
    lags = np.arange(-D, D + 1)
    order = np.lexsort((lags, np.abs(lags)))  # smallest |d| first, of +-d the negative: the first minimum in this order is the tie rule
    pos = np.zeros(K, np.int64)
    for k in range(1, K):
        t = xp[left + pos[k - 1] + HS:left + pos[k - 1] + HS + N]
        win = np.lib.stride_tricks.sliding_window_view(xp[left + q[k] - D:left + q[k] + D + N], N)
        df = win - t
        e = np.zeros(2 * D + 1, np.float32)
        for s in range(SEGS):
            part = df[:, s * seg:min(N, (s + 1) * seg)]
            e = e + np.einsum("ij,ij->i", part, part)
        pos[k] = q[k] + lags[order[np.argmin(e[order])]]
    w = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N, dtype=np.float64) / N)).astype(np.float32)
    m = np.arange(out_len, dtype=np.int64)
    kk, ii = m // HS, m % HS
    y = xp[left + m].copy()
    late = kk >= 1
    kk, ii = kk[late], ii[late]
    y[late] = w[ii + HS] * xp[left + pos[kk - 1] + HS + ii] + w[ii] * xp[left + pos[kk] + ii]
    return y


def child(mode, calls, warmup):
    sys.path.insert(0, os.path.join(ROOT, "fish-speech.rs_amd"))
    import numpy as np
    import fishrt
    from fishrt.wav import pcm_to_i16
    codec = fishrt.FireflyCodec(0).load_synthetic(0xC0DEC)
    rng = np.random.RandomState(1)
    out = {}
    for b, T in SHAPES:
        times, d2h = [], 0
        for k in range(warmup + calls):
            codes = rng.randint(0, 1000, (b, 8, T)).astype(np.uint32)
            t0 = time.perf_counter()
            if mode == "device":
                pcm = codec.decode(codes, dtype="s16", speed=SPEED)
                d2h = pcm.nbytes
            elif mode == "plain":
                pcm = codec.decode(codes, dtype="s16")
                d2h = pcm.nbytes
            else:
                f32 = codec.decode(codes)
                d2h = f32.nbytes
                pcm = [pcm_to_i16(stretch_numpy(f32[i, 0], SPEED)) for i in range(b)]
            t1 = time.perf_counter()
            if k >= warmup:
                times.append((t1 - t0) * 1e3)
        out[f"{b}x{T}"] = dict(ms=statistics.median(times), d2h_bytes=int(d2h))
    codec.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-calls", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "codec_speed.json"))
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.calls, a.warmup)
    runs = {m: [] for m in MODES}
    for _ in range(a.reps):
        for m in MODES:  # alternating processes
            calls, warmup = (a.host_calls, 1) if m == "host" else (a.calls, a.warmup)
            cmd = [sys.executable, os.path.abspath(__file__), "--child", m, "--calls", str(calls), "--warmup", str(warmup)]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True, timeout=600, check=True)
            runs[m].append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    res = dict(protocol=f"{a.reps} rounds of alternating processes, median of {a.calls} calls after {a.warmup} (host: {a.host_calls} after 1); "
                        f"speed {SPEED}, s16 at the codec's rate", shapes={})
    for b, T in SHAPES:
        key, row = f"{b}x{T}", {}
        for m in MODES:
            vals = [r[key]["ms"] for r in runs[m]]
            row[m] = dict(ms=statistics.median(vals), ms_min=min(vals), ms_max=max(vals), d2h_bytes=runs[m][0][key]["d2h_bytes"])
        res["shapes"][key] = row
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
