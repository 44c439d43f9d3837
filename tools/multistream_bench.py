"""Multi-stream vocoder (fs_codec_streams_decode): one call that advances n streams by T frames each vs n separate n = 1 calls, for
n in {1, 2, 4, 8, 16, 32} x T in {16, 32, 64}.  Full-size codec, synthetic weights, f16 precision (argv[1] = precision).  Every call ends
with a stream synchronisation (the PCM is on the host when it returns), so wall time around a call is HIP-synchronised time.  Per point: 3
warm-up rounds, then the best of 7 of each variant.  --profile: only n = 8, T = 32 (20 batched calls then 20 x 8 single calls) for a
rocprofv3 --kernel-trace --stats run.  usage: multistream_bench.py [precision] [--profile]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fish-speech.rs_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (rocprofv3 needs torch's HIP runtime loaded first)

import fishrt  # noqa: E402


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    prec = args[0] if args else "f16"
    profile = "--profile" in sys.argv
    c = fishrt.FireflyCodec(0, precision=prec).load_synthetic(0xC0DEC)
    rng = np.random.RandomState(0)
    points = [(8, 32)] if profile else [(n, T) for n in (1, 2, 4, 8, 16, 32) for T in (16, 32, 64)]
    rows = []
    for n, T in points:
        ids = [c.streams_open() for _ in range(n)]
        codes = rng.randint(0, 1000, (n, 8, T)).astype(np.uint32)

        def batched():
            c.streams_decode(ids, codes)

        def single():
            for i in range(n):
                c.streams_decode(ids[i:i + 1], codes[i:i + 1])

        def best(fn, reps):
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                fn()
                ts.append(time.perf_counter() - t0)
            return min(ts)

        if profile:
            for _ in range(20):
                batched()
            for _ in range(20):
                single()
            print(f"profile run: n={n} T={T}, 20 batched calls + 20 x {n} single calls")
        else:
            best(batched, 3)
            best(single, 3)
            tb, ts = best(batched, 7), best(single, 7)
            r = dict(precision=prec, n=n, T=T, batched_ms=round(tb * 1e3, 3), separate_ms=round(ts * 1e3, 3), speedup=round(ts / tb, 3),
                     batched_frames_per_s=round(n * T / tb, 1))
            rows.append(r)
            print(json.dumps(r), flush=True)
        for i in ids:
            c.streams_close(i)
    if rows:
        print(f"\n{'n':>3} {'T':>3} {'batched ms':>11} {'n x 1 ms':>9} {'speed-up':>9} {'frames/s':>10}")
        for r in rows:
            print(f"{r['n']:>3} {r['T']:>3} {r['batched_ms']:>11.3f} {r['separate_ms']:>9.3f} {r['speedup']:>9.2f} {r['batched_frames_per_s']:>10.0f}")


if __name__ == "__main__":
    main()
