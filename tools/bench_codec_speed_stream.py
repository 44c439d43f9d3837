"""The `speed` of a request in codec multi-streams (fs_codec_streams_open_speed): what the chunked stretch stage costs per ragged call, what
it buys in first audio, and whether the one-shot path kept its speed (profiles/codec_speed_stream.json).  Full-size codec, synthetic
weights, f16 mode; every timed call ends with its PCM in host memory, so wall time around a call is synchronised time.

  call         one ragged vocoder call of 8 x 32 and 32 x 16 frames to s16 at 24 kHz (sinc), repeated on the same open streams:
                 stream    streams opened with speed 1.25 (vocoder -> stretch stage -> resample / format stage)
                 plain     the same call on streams without a stretch stage (fs_codec_streams_open_pcm)
                 oneshot   fs_codec_decode_speed of the same shape (b rows of T frames, nothing carried)
               chain_frames_per_call: the stretch frames one stream emits per call in steady state (2048 T / speed / 512); the chain kernel
               walks them one after the other, all streams side by side, so stream - plain is about that many serial frame searches.
  one_shot     fs_time_stretch (b rows of 2048 T samples, host to host) and fs_codec_decode_speed on this build and on a build of the parent
               commit (--parent-lib, default tools/_ab/libparent.so; left out when the file is missing).
  first_audio  a 32-slot Fish-1.5 bf16 session (synthetic weights), every request at speed 1.25 to s16 at 24 kHz, 4 frames per step:
                 streamed  SessionStreamer(ragged=True, speed=1.25, first_chunk=4, chunk=64): add() to the first non-empty piece
                 waiting   what the parent commit can do: step until the request has finished, then decode(speed=) of all its frames

The modes of `call` and `one_shot` run in a process each and alternate, --reps rounds; a mode's figure is the median over rounds of the
per-process median over --calls timed calls after --warmup, with the smallest and largest round next to it (the spread).  first_audio loads
the LM once and alternates the two ways inside one process, --fa-reps times after one warm-up each.

usage: bench_codec_speed_stream.py [--reps 3] [--calls 20] [--warmup 5] [--fa-reps 3] [--parts call,one_shot,first_audio] [--parent-lib F] [--out F]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(8, 32), (32, 16)]
SPEED = 1.25
SPEC = dict(sample_rate=24000, resample="sinc", dtype="s16")


def _fishrt(lib=None):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "fish-speech.rs_amd")]
    import fishrt
    if lib:
        fishrt._ffi.LIB_PATH = os.path.abspath(lib)  # (before the first call loads the library)
    return fishrt


def _median_ms(fn, calls, warmup):
    ts = []
    for k in range(warmup + calls):
        t0 = time.perf_counter()
        fn()
        if k >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def child(mode, calls, warmup, lib):
    import numpy as np
    fishrt = _fishrt(lib)
    codec = fishrt.FireflyCodec(0).load_synthetic(0xC0DEC)
    rng = np.random.RandomState(1)
    out = {}
    for b, T in SHAPES:
        key = f"{b}x{T}"
        codes = rng.randint(0, 1000, (b, 8, T)).astype(np.uint32)
        if mode in ("stream", "plain"):
            kw = dict(SPEC, speed=SPEED) if mode == "stream" else SPEC
            ids = [codec.streams_open(**kw) for _ in range(b)]
            chunks = [np.ascontiguousarray(codes[i]) for i in range(b)]
            out[key] = dict(ms=_median_ms(lambda: codec.streams_decode_ragged(ids, chunks, final=[False] * b), calls, warmup))
            for i in ids:
                codec.streams_close(i)
        else:  # "this" / "parent": the one-shot calls
            x = rng.uniform(-0.5, 0.5, (b, 2048 * T)).astype(np.float32)
            out[key] = dict(decode_speed_ms=_median_ms(lambda: codec.decode(codes, speed=SPEED, **SPEC), calls, warmup),
                            time_stretch_ms=_median_ms(lambda: fishrt.time_stretch(x, SPEED), calls, warmup))
    codec.close()
    print("RESULT " + json.dumps(out))


class _CodesBelow1000:
    """the synthetic LM samples from 1024 codebook entries, the codec's FSQ has 1000: fold the codes into range"""

    def __init__(self, s):
        self.s = s

    def add(self, p, n):
        return self.s.add(p, n)

    def step(self, k):
        return self.s.step(k)

    def release(self, slot):
        return self.s.release(slot)

    def poll(self, slot, codes=True):
        r = self.s.poll(slot, codes)
        return (r[0] % 1000, r[1]) if codes else r


def first_audio(reps, slots=32, k=4):
    import numpy as np
    fishrt = _fishrt()
    from fishrt import config as fcfg
    lm = fishrt.DualARTransformer(fcfg.FISH_1_5, fcfg.FISH_1_5_TOKENS, 0, "bf16", max_batch=slots).load_synthetic(0xF15E5EED)
    rows = bool(lm.rows_supported(slots))
    codec = fishrt.FireflyCodec(0, precision="f16").load_synthetic(0xC0DEC)
    rng = np.random.RandomState(2)
    prompts = []
    for i in range(slots):
        p = np.zeros((9, 24 + i % 9), np.uint32)
        p[0] = rng.randint(0, 400, p.shape[1])
        prompts.append(p)
    frames = [96 + (29 * i) % 131 for i in range(slots)]

    def streamed():
        first = {}
        t0 = time.perf_counter()
        with lm.session(temp=0.0, top_p=1.0, top_k=0, seed=1, ignore_eos=True, rows=rows) as raw:
            t_add = {}

            def on_audio(tag, pcm, final):
                if len(pcm) and tag not in first:
                    first[tag] = time.perf_counter() - t_add[tag]

            ss = fishrt.SessionStreamer(_CodesBelow1000(raw), codec, chunk=64, first_chunk=4, ragged=True, speed=SPEED, sample_rate=SPEC["sample_rate"],
                                        resample=SPEC["resample"], pcm_dtype=SPEC["dtype"], on_audio=on_audio)
            for i in range(slots):
                t_add[i] = time.perf_counter()
                assert ss.add(prompts[i], prompts[i].shape[1] + frames[i], tag=i) is not None
            while ss.live:
                ss.step(k)
        return first, time.perf_counter() - t0, len(ss.calls)

    def waiting():
        first = {}
        t0 = time.perf_counter()
        with lm.session(temp=0.0, top_p=1.0, top_k=0, seed=1, ignore_eos=True, rows=rows) as raw:
            s = _CodesBelow1000(raw)
            live, calls = {}, 0
            for i in range(slots):
                t = time.perf_counter()
                live[s.add(prompts[i], prompts[i].shape[1] + frames[i])] = (i, t)
            while live:
                s.step(k)
                for slot in [sl for sl in live if s.poll(sl, codes=False)[1]]:
                    i, t = live.pop(slot)
                    codec.decode(np.ascontiguousarray(s.poll(slot)[0][None]), speed=SPEED, **SPEC)
                    first[i] = time.perf_counter() - t
                    calls += 1
                    s.release(slot)
        return first, time.perf_counter() - t0, calls

    def summary(rs):
        fa = [np.array([r[0][i] for i in range(slots)]) * 1e3 for r in rs]
        med, worst, wall = [float(np.median(a)) for a in fa], [float(a.max()) for a in fa], [r[1] * 1e3 for r in rs]
        return dict(first_audio_median_ms=round(statistics.median(med), 3), first_audio_median_ms_all=[round(v, 3) for v in med],
                    first_audio_worst_ms=round(statistics.median(worst), 3), wall_ms=round(statistics.median(wall), 1),
                    wall_ms_all=[round(v, 1) for v in wall], vocoder_calls=rs[0][2])

    streamed(), waiting()  # warm-up
    a, b = [], []
    for _ in range(reps):
        a.append(streamed())
        b.append(waiting())
    codec.close()
    print("RESULT " + json.dumps(dict(slots=slots, rows_session=rows, frames_per_step=k, first_chunk=4, chunk=64, reps=reps, speed=SPEED, spec=SPEC,
                                      requests_frames=[min(frames), max(frames)], streamed=summary(a), waiting_for_the_finished_request=summary(b))))


def _spawn(args, timeout=900):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, stdout=subprocess.PIPE, universal_newlines=True, timeout=timeout, check=True)
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def _spread(vals):
    return dict(ms=round(statistics.median(vals), 4), ms_min=round(min(vals), 4), ms_max=round(max(vals), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--fa-reps", type=int, default=3)
    ap.add_argument("--parts", default="call,one_shot,first_audio")
    ap.add_argument("--parent-lib", default=os.path.join(ROOT, "tools", "_ab", "libparent.so"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "codec_speed_stream.json"))
    ap.add_argument("--child", default=None)
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    if a.child == "first_audio":
        return first_audio(a.fa_reps)
    if a.child:
        return child(a.child, a.calls, a.warmup, a.lib)
    parts = a.parts.split(",")
    have_parent = os.path.exists(a.parent_lib)
    modes = (["stream", "plain"] if "call" in parts else []) + (["this"] + (["parent"] if have_parent else []) if "one_shot" in parts or "call" in parts else [])
    runs = {m: [] for m in modes}
    for _ in range(a.reps):
        for m in modes:  # alternating processes
            extra = ["--lib", a.parent_lib] if m == "parent" else []
            runs[m].append(_spawn(["--child", m, "--calls", str(a.calls), "--warmup", str(a.warmup)] + extra))
    res = dict(tool="tools/bench_codec_speed_stream.py",
               protocol=f"{a.reps} rounds of alternating processes, median of {a.calls} calls after {a.warmup}; speed {SPEED}, s16 at 24 kHz (sinc); "
                        "ms = median over rounds, ms_min / ms_max = the smallest and largest round")
    if "call" in parts:
        res["call"] = {}
        for b, T in SHAPES:
            key = f"{b}x{T}"
            row = dict(stream=_spread([r[key]["ms"] for r in runs["stream"]]), plain=_spread([r[key]["ms"] for r in runs["plain"]]),
                       oneshot=_spread([r[key]["decode_speed_ms"] for r in runs["this"]]))
            row["chain_frames_per_call"] = round(2048 * T / SPEED / 512, 1)
            row["stretch_stage_ms"] = round(row["stream"]["ms"] - row["plain"]["ms"], 4)
            row["stretch_stage_us_per_chain_frame"] = round(1e3 * row["stretch_stage_ms"] / row["chain_frames_per_call"], 2)
            res["call"][key] = row
    if "one_shot" in parts:
        res["one_shot"] = {}
        for b, T in SHAPES:
            key = f"{b}x{T}"
            row = {}
            for name in ("decode_speed_ms", "time_stretch_ms"):
                row[name] = dict(this_build=_spread([r[key][name] for r in runs["this"]]),
                                 parent_build=_spread([r[key][name] for r in runs["parent"]]) if have_parent else "not measured yet")
            res["one_shot"][key] = row
    res["first_audio"] = _spawn(["--child", "first_audio", "--fa-reps", str(a.fa_reps)], timeout=1500) if "first_audio" in parts else "not measured yet"
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
