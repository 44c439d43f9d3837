"""Ragged multi-stream vocoder call (fs_codec_streams_decode_ragged): three measurements on one MI355X, f16 mode, full-size codec with
synthetic weights.  Every vocoder call ends with a stream synchronisation (the PCM is on the host when it returns), so wall time around a
call is HIP-synchronised time.  Each part prints ONE JSON line.

  --part existing [--pkg DIR] [--label L]
      the entry points that existed before: fs_codec_decode at 256 frames, fs_codec_streams_decode at n = 8, T = 32 and n = 32, T = 16
      (the points of profiles/multistream_bench.txt).  Per point 10 warm-up calls, then 50 timed calls: median, min, 10th / 90th percentile.
      --pkg: directory holding the `fishrt` package and its libfishrt.so (default: this tree) -- point it at a build of the parent commit
      to get the bar; run parent, this build, parent again to see the run-to-run spread.
  --part replay
      the vocoder workload of a 32-slot session, two ways.  A scripted session (every live slot gains `k` frames per step; 96 requests
      of staggered lengths, a new one admitted whenever a slot is free) is driven through SessionStreamer(first_chunk=32, chunk=64) with
      ragged=False -- the call sequence without the ragged call: one uniform call per distinct T per step, n = 1 tails, halo decodes --
      and with ragged=True: one call per step.  Same requests, same codes, same steps; only the time inside the codec calls is counted.
      One warm-up run of each, then --reps runs of each, alternating.
  --part first_audio
      SessionStreamer on a real 32-slot Fish-1.5 bf16 session (synthetic weights), first_chunk = 32 / ragged=False against first_chunk = 4 /
      ragged=True (chunk = 64, 4 frames per step for both): median and worst first_audio_s over the requests and the session's wall time.
  --collect FILE...   merge the JSON lines of earlier runs into one document (--out)

    python tools/bench_codec_ragged.py --part replay [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _import(pkg):
    sys.path[:0] = [ROOT, pkg or os.path.join(ROOT, "fish-speech.rs_amd")]
    import fishrt
    return fishrt


def _stats(ts):
    a = np.sort(np.asarray(ts)) * 1e3
    return dict(median_ms=round(float(np.median(a)), 4), min_ms=round(float(a[0]), 4), p10_ms=round(float(np.percentile(a, 10)), 4),
                p90_ms=round(float(np.percentile(a, 90)), 4), reps=len(a))


def _timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return _stats(ts)


def part_existing(fishrt, label):
    c = fishrt.FireflyCodec(0, precision="f16").load_synthetic(0xC0DEC)
    rng = np.random.RandomState(0)
    out = dict(part="existing", label=label, lib=fishrt._ffi.LIB_PATH)
    one = rng.randint(0, 1000, (1, 8, 256)).astype(np.uint32)
    out["decode_T256"] = _timed(lambda: c.decode(one), 10, 50)
    for n, T in ((8, 32), (32, 16)):
        ids = [c.streams_open() for _ in range(n)]
        codes = rng.randint(0, 1000, (n, 8, T)).astype(np.uint32)
        out[f"streams_decode_n{n}_T{T}"] = _timed(lambda: c.streams_decode(ids, codes), 10, 50)
        for i in ids:
            c.streams_close(i)
    c.close()
    return out


class ScriptedSession:
    """stands in for lm.Session: slot s of request i holds a fixed code sequence and gains k frames per step(k)"""

    def __init__(self, seqs, max_batch):
        self.seqs, self.max_batch, self.slots = seqs, max_batch, {}

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
        return (self.seqs[i][:, :n], done) if codes else (n, done)

    def release(self, slot):
        del self.slots[slot]


class TimedCodec:
    """forwards to the codec and sums the wall time spent inside its decode calls"""

    def __init__(self, codec):
        self.c, self.t, self.n = codec, 0.0, 0
        self.STREAM_MIN_FRAMES = codec.STREAM_MIN_FRAMES

    def streams_open(self):
        return self.c.streams_open()

    def streams_close(self, sid):
        return self.c.streams_close(sid)

    def _timed(self, fn, *a):
        t0 = time.perf_counter()
        r = fn(*a)
        self.t += time.perf_counter() - t0
        self.n += 1
        return r

    def streams_decode(self, ids, codes):
        return self._timed(self.c.streams_decode, ids, codes)

    def streams_decode_ragged(self, ids, chunks):
        return self._timed(self.c.streams_decode_ragged, ids, chunks)

    def decode(self, codes):
        return self._timed(self.c.decode, codes)


def part_replay(fishrt, reps, slots=32, requests=96, k=8):
    codec = fishrt.FireflyCodec(0, precision="f16").load_synthetic(0xC0DEC)
    rng = np.random.RandomState(1)
    lengths = [150 + (37 * i) % 311 for i in range(requests)]  # staggered: tails of every length occur
    seqs = [rng.randint(0, 1000, (8, L)).astype(np.uint32) for L in lengths]

    def run(ragged):
        sess, tc = ScriptedSession(seqs, slots), TimedCodec(codec)
        ss = fishrt.SessionStreamer(sess, tc, chunk=64, first_chunk=32, ragged=ragged)
        pending, samples = list(range(requests)), 0
        while pending or ss.live:
            while pending and ss.add(pending[0], 0, tag=pending[0]) is not None:
                pending.pop(0)
            for _, pcm, _ in ss.step(k):
                samples += len(pcm)
        assert samples == 2048 * sum(lengths)
        kinds = {}
        for _, kind, _, _ in ss.calls:
            kinds[kind] = kinds.get(kind, 0) + 1
        steps_with_calls = len({q for q, _, _, _ in ss.calls})
        return dict(vocoder_s=tc.t, calls=tc.n, steps=ss.quantum, steps_with_calls=steps_with_calls, kinds=kinds,
                    max_calls_in_a_step=max(sum(1 for c in ss.calls if c[0] == q) for q in {c[0] for c in ss.calls}))

    run(False), run(True)  # warm-up: every shape of both sequences
    a, b = [], []
    for _ in range(reps):
        a.append(run(False))
        b.append(run(True))

    def summary(rs):
        ts = np.array([r["vocoder_s"] for r in rs])
        return dict(vocoder_ms_median=round(float(np.median(ts)) * 1e3, 2), vocoder_ms_min=round(float(ts.min()) * 1e3, 2),
                    vocoder_ms_max=round(float(ts.max()) * 1e3, 2), calls=rs[0]["calls"], steps=rs[0]["steps"],
                    calls_per_step=round(rs[0]["calls"] / rs[0]["steps"], 3), max_calls_in_a_step=rs[0]["max_calls_in_a_step"], kinds=rs[0]["kinds"])

    sa, sb = summary(a), summary(b)
    codec.close()
    return dict(part="replay", slots=slots, requests=requests, frames=int(sum(lengths)), frames_per_step=k, reps=reps, first_chunk=32, chunk=64,
                uniform_tail_halo_sequence=sa, one_ragged_call_per_step=sb,
                ragged_over_sequence_time=round(sb["vocoder_ms_median"] / sa["vocoder_ms_median"], 4))


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


def part_first_audio(fishrt, reps, slots=32, k=4):
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

    def run(first_chunk, ragged):
        t0 = time.perf_counter()
        with lm.session(temp=0.0, top_p=1.0, top_k=0, seed=1, ignore_eos=True, rows=rows) as raw:
            ss = fishrt.SessionStreamer(_CodesBelow1000(raw), codec, chunk=64, first_chunk=first_chunk, ragged=ragged)
            for i in range(slots):
                assert ss.add(prompts[i], prompts[i].shape[1] + frames[i], tag=i) is not None
            while ss.live:
                ss.step(k)
        wall = time.perf_counter() - t0
        fa = np.array([ss.stats[i]["first_audio_s"] for i in range(slots)])
        return dict(first_audio_median_ms=float(np.median(fa)) * 1e3, first_audio_worst_ms=float(fa.max()) * 1e3, wall_ms=wall * 1e3,
                    vocoder_calls=len(ss.calls), steps=ss.quantum)

    run(32, False), run(4, True)  # warm-up
    a, b = [], []
    for _ in range(reps):
        a.append(run(32, False))
        b.append(run(4, True))

    def summary(rs):
        out = {key: round(float(np.median([r[key] for r in rs])), 3) for key in ("first_audio_median_ms", "first_audio_worst_ms", "wall_ms")}
        out["wall_ms_all"] = [round(r["wall_ms"], 1) for r in rs]
        out["vocoder_calls"], out["steps"] = rs[0]["vocoder_calls"], rs[0]["steps"]
        return out

    codec.close()
    return dict(part="first_audio", slots=slots, rows_session=rows, frames_per_step=k, chunk=64, reps=reps, requests_frames=[min(frames), max(frames)],
                first_chunk_32_uniform=summary(a), first_chunk_4_ragged=summary(b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["existing", "replay", "first_audio"])
    ap.add_argument("--pkg", default=None)
    ap.add_argument("--label", default="this build")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--collect", nargs="*")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.collect is not None:
        doc = dict(tool="tools/bench_codec_ragged.py", results=[])
        try:
            doc["commit"] = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip() + " + this change"
        except Exception:
            pass
        for f in a.collect:
            for line in open(f):
                if line.startswith("{"):
                    doc["results"].append(json.loads(line))
        text = json.dumps(doc, indent=1)
    else:
        fishrt = _import(a.pkg)
        r = part_existing(fishrt, a.label) if a.part == "existing" else part_replay(fishrt, a.reps) if a.part == "replay" else part_first_audio(fishrt, a.reps)
        text = json.dumps(r)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
