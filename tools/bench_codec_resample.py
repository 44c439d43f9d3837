"""Vocoder streams to 24 kHz s16: the device path against the two host paths it replaces (profiles/codec_resample.json).

Per call shape -- 8 streams x 32 frames and 32 streams x 16 frames -- the wall time of one vocoder call that ends with s16 PCM at 24 kHz
in host memory, and the bytes its D2H copy moves:
  (a) device    streams opened with {24000, sinc, s16}, FireflyCodec.streams_decode_ragged(..., final=) (fs_codec_streams_decode_pcm)
  (b) linear    plain streams, f32 at 44.1 kHz to the host, then the numpy restatement of the reference's linear resample + pcm_to_i16
  (c) scipy     the same followed by scipy.signal.resample_poly(x, 80, 147) + pcm_to_i16
and, in (b), the plain streams_decode_ragged call alone ("plain_ms": the launches a handle without spec streams makes; compare it with the
same figure of a parent build through --lib).  Every mode runs in a process of its own and the modes alternate, --reps rounds; the figure
of a mode is the median over rounds of the per-process median over --calls timed calls after --warmup.  The first-audio latency of a
32-slot SessionStreamer is not taken here.

usage: bench_codec_resample.py [--reps 5] [--calls 20] [--warmup 5] [--lib OTHER.so] [--out profiles/codec_resample.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(8, 32), (32, 16)]
MODES = ["device", "linear", "scipy"]


def _linear_24k(x):
    import numpy as np
    n = x.shape[0]
    ratio = np.float64(24000) / np.float64(44100)
    out_len = int(np.ceil(np.float64(n) * ratio))
    idx = np.arange(out_len, dtype=np.float64) / ratio
    fl = np.floor(idx)
    f, c = np.minimum(fl.astype(np.int64), n - 1), np.minimum(np.ceil(idx).astype(np.int64), n - 1)
    t = (idx - fl).astype(np.float32)
    return x[f] * (np.float32(1.0) - t) + x[c] * t


def child(mode, calls, warmup, lib):
    sys.path.insert(0, os.path.join(ROOT, "fish-speech.rs_amd"))
    import numpy as np
    if lib:
        from fishrt import _ffi
        _ffi.LIB_PATH = lib
    import fishrt
    from fishrt.wav import pcm_to_i16
    if mode == "scipy":
        from scipy.signal import resample_poly
    codec = fishrt.FireflyCodec(0).load_synthetic(0xC0DEC)
    rng = np.random.RandomState(1)
    out = {}
    for n, T in SHAPES:
        spec = dict(sample_rate=24000, resample="sinc", dtype="s16") if mode == "device" else {}
        ids = [codec.streams_open(**spec) for _ in range(n)]
        times, plain, d2h = [], [], 0
        for k in range(warmup + calls):
            chunks = [rng.randint(0, 1000, (8, T)).astype(np.uint32) for _ in range(n)]
            t0 = time.perf_counter()
            if mode == "device":
                pcm = codec.streams_decode_ragged(ids, chunks, final=[False] * n)
                d2h = sum(p.nbytes for p in pcm)
                t1 = time.perf_counter()
            else:
                pcm = codec.streams_decode_ragged(ids, chunks)
                t1 = time.perf_counter()
                d2h = sum(p.nbytes for p in pcm)
                if mode == "linear":
                    pcm = [pcm_to_i16(_linear_24k(p)) for p in pcm]
                else:
                    pcm = [pcm_to_i16(resample_poly(p, 80, 147).astype(np.float32)) for p in pcm]
            t2 = time.perf_counter()
            if k >= warmup:
                times.append((t2 - t0) * 1e3)
                plain.append((t1 - t0) * 1e3)
        for i in ids:
            codec.streams_close(i)
        rec = dict(ms=statistics.median(times), d2h_bytes=int(d2h))
        if mode != "device":
            rec["plain_ms"] = statistics.median(plain)
        out[f"{n}x{T}"] = rec
    codec.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "codec_resample.json"))
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.calls, a.warmup, a.lib)
    runs = {m: [] for m in MODES}
    for _ in range(a.reps):
        for m in MODES:  # alternating processes
            cmd = [sys.executable, os.path.abspath(__file__), "--child", m, "--calls", str(a.calls), "--warmup", str(a.warmup)]
            if a.lib:
                cmd += ["--lib", a.lib]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True, timeout=300, check=True)
            runs[m].append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    res = dict(protocol=f"{a.reps} rounds of alternating processes, median of {a.calls} calls after {a.warmup}; to 24 kHz s16", lib=a.lib, shapes={})
    for n, T in SHAPES:
        key, row = f"{n}x{T}", {}
        for m in MODES:
            vals = [r[key]["ms"] for r in runs[m]]
            row[m] = dict(ms=statistics.median(vals), ms_min=min(vals), ms_max=max(vals), d2h_bytes=runs[m][0][key]["d2h_bytes"])
            if m != "device":
                pv = [r[key]["plain_ms"] for r in runs[m]]
                row[m].update(plain_ms=statistics.median(pv), plain_ms_min=min(pv), plain_ms_max=max(pv))
        res["shapes"][key] = row
    res["first_audio_32_slots"] = None  # not measured by this tool
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
