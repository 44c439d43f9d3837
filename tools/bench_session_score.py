"""What FS_SESSION_SCORE costs and what DualARTransformer.score() delivers.  The protocol of tools/bench_session_hidden.py, in ONE process:

    python tools/bench_session_score.py --out profiles/session_score.json

1. Step time of a SAMPLED per-slot session of 16 and of 32 live slots (--slots), begun without the flag ("flag_off") and with it but no
   scoring slot ("flag_on_no_scoring_slot": the 9 score nodes are in the step graph and every block of them exits at once).  Ignore-eos,
   sampling 0.7 / 0.8 / 256 with repetition penalty 1.4, Fish-1.5 shapes, synthetic bf16 weights.  A round opens a session, admits the
   slots, warms up, then steps until --seconds of decode time have passed; the step time is the handle's own HIP-event time around the
   session_step launches (last_stats()["decode_ms"]) divided by the frames launched.  Rounds of the two modes alternate, each mode is
   warmed up by an untimed round first, every round starts from the same prompts.  Per mode: every round's figure, the median and the
   run-to-run spread (max - min) / median; "flag_on_over_off" = the ratio of the medians - 1.
2. Sequences per second of score() at --score-slots x --score-frames (32 x 256): wall time of the whole call -- session, prefill of every
   prompt, the forced steps, the polls -- after one untimed call; the median of --rounds calls.

No threshold is built in: the tool reports."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fish-speech.rs_amd")]

MODES = ("flag_off", "flag_on_no_scoring_slot")


def step_times(args, slots):
    import numpy as np
    import fishrt
    from fishrt import config as fcfg
    tok = fcfg.FISH_1_5_TOKENS
    lm = fishrt.DualARTransformer(fcfg.FISH_1_5, tok, 0, "bf16", max_batch=slots).load_synthetic(0xF15E5EED)
    rs = np.random.RandomState(1)
    prompts = []
    for _ in range(slots):
        p = np.zeros((9, args.prompt_len), np.uint32)
        p[0] = rs.randint(0, tok["im_end_id"], args.prompt_len)
        prompts.append(p)
    kw = dict(temp=0.7, top_p=0.8, top_k=256, seed=42, ignore_eos=True, per_slot=True, repetition_penalty=1.4)
    budget = args.prompt_len + args.max_frames
    res = {m: [] for m in MODES}

    def one_round(mode):
        with lm.session(score=(mode != "flag_off"), **kw) as s:
            for p in prompts:
                assert s.add(p, budget) is not None
            assert s.step(args.warmup) == slots
            st0 = lm.last_stats()
            while True:
                live = s.step(8)
                st = lm.last_stats()
                if st["decode_ms"] - st0["decode_ms"] >= args.seconds * 1000.0 or live < slots:
                    break
            assert live == slots, "slots finished inside the timed window: raise --max-frames"
            return (st["decode_ms"] - st0["decode_ms"]) * 1000.0 / (st["graph_launches"] - st0["graph_launches"])

    for m in MODES:  # untimed: graph capture, allocations
        one_round(m)
    for r in range(args.rounds):
        for m in MODES:
            res[m].append(one_round(m))
            print(f"{slots} slots, round {r} {m}: {res[m][-1]:.1f} us / step", flush=True)
    lm.close()
    out = {}
    for m in MODES:
        med = statistics.median(res[m])
        out[m] = dict(us_per_step=res[m], median_us=med, spread=(max(res[m]) - min(res[m])) / med)
    out["flag_on_over_off"] = out[MODES[1]]["median_us"] / out[MODES[0]]["median_us"] - 1.0
    return out


def score_rate(args):
    import numpy as np
    import fishrt
    from fishrt import config as fcfg
    cfg, tok = fcfg.FISH_1_5, fcfg.FISH_1_5_TOKENS
    n, N = args.score_slots, args.score_frames
    lm = fishrt.DualARTransformer(cfg, tok, 0, "bf16", max_batch=n).load_synthetic(0xF15E5EED)
    rs = np.random.RandomState(2)
    prompts, frames = [], []
    for _ in range(n):
        p = np.zeros((9, args.prompt_len), np.uint32)
        p[0] = rs.randint(0, tok["im_end_id"], args.prompt_len)
        f = np.zeros((9, N), np.uint32)
        f[0] = tok["semantic_start_id"] + rs.randint(0, cfg["vocab_size"] - tok["semantic_start_id"], N)
        f[1:] = rs.randint(0, cfg["codebook_size"], (8, N))
        prompts.append(p)
        frames.append(f)
    lm.score(prompts, frames)  # untimed: graph capture, allocations
    secs = []
    for r in range(args.rounds):
        t0 = time.perf_counter()
        out = lm.score(prompts, frames)
        secs.append(time.perf_counter() - t0)
        assert len(out) == n and all(o["logprob"].shape == (N, 9) and np.isfinite(o["total"]) for o in out)
        print(f"score() round {r}: {n} sequences x {N} frames in {secs[-1]:.3f} s", flush=True)
    lm.close()
    med = statistics.median(secs)
    return dict(sequences=n, frames=N, prompt_len=args.prompt_len, seconds=secs, median_s=med, sequences_per_s=n / med, frames_per_s=n * N / med)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--slots", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--prompt-len", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=0.35, help="timed decode time per round and mode")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--max-frames", type=int, default=600)
    ap.add_argument("--score-slots", type=int, default=32)
    ap.add_argument("--score-frames", type=int, default=256)
    ap.add_argument("--out")
    a = ap.parse_args()
    import fishrt
    out = dict(version=fishrt.lib().fs_version().decode(), prompt_len=a.prompt_len, seconds_per_round=a.seconds, rounds=a.rounds,
               sampling=dict(temp=0.7, top_p=0.8, top_k=256, repetition_penalty=1.4), step={})
    for slots in a.slots:
        out["step"][str(slots)] = step_times(a, slots)
    out["score"] = score_rate(a)
    text = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    print(json.dumps(dict(step={k: dict(off_us=v[MODES[0]]["median_us"], on_us=v[MODES[1]]["median_us"], on_over_off=v["flag_on_over_off"])
                                for k, v in out["step"].items()},
                          score=dict(sequences_per_s=out["score"]["sequences_per_s"], frames_per_s=out["score"]["frames_per_s"]))))


if __name__ == "__main__":
    main()
