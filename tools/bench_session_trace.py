"""What FS_SESSION_TRACE costs and what DualARTransformer.generate_traced() saves.  The protocol of tools/bench_session_score.py:

    python tools/bench_session_trace.py --out profiles/session_trace.json

1. Step time of a SAMPLED per-slot session of 16 and of 32 live slots (--slots) in three modes (--modes): "score" = begun with
   FS_SESSION_SCORE only (the graphs such a session always replayed), "trace_no_traced_slot" = FS_SESSION_TRACE with plain slots (the tail
   node is in the graph and every block of it exits at once), "trace_all_traced" = the same session with every slot traced (every score
   node keeps its row, the tail node closes every row).  Ignore-eos, sampling 0.7 / 0.8 / 256 with repetition penalty 1.4, Fish-1.5
   shapes, synthetic bf16 weights.  A round opens a session, admits the slots, warms up, then steps until --seconds of decode time have
   passed; the step time is the handle's own HIP-event time around the session_step launches divided by the frames launched.  Rounds
   of the modes alternate, each mode is warmed up by an untimed round first.  Per mode: every round's figure, the median, the spread
   (max - min) / median; the ratios of the medians over "score".
2. --lib PATH runs on another build of the library (an earlier commit's, for the "score" mode and the two-pass figure: alternate
   processes of the two builds and compare their medians).
3. Wall time of generate_traced() at --gen-slots x --gen-frames (32 x 256) against the two passes it replaces: generating the same
   requests in a per-slot session, then score() of as many sequences of the same length (the log-probs of given tokens; recovering the
   slow tokens of the first pass is not counted).  One untimed call each, then the median of --rounds calls.

No threshold is built in: the tool reports."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fish-speech.rs_amd")]

MODES = ("score", "trace_no_traced_slot", "trace_all_traced")
KW = dict(temp=0.7, top_p=0.8, top_k=256, seed=42, ignore_eos=True, per_slot=True, score=True, repetition_penalty=1.4)


def _prompts(n, L, seed, tok):
    import numpy as np
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        p = np.zeros((9, L), np.uint32)
        p[0] = rs.randint(0, tok["im_end_id"], L)
        out.append(p)
    return out


def step_times(args, slots):
    import fishrt
    from fishrt import config as fcfg
    tok = fcfg.FISH_1_5_TOKENS
    lm = fishrt.DualARTransformer(fcfg.FISH_1_5, tok, 0, "bf16", max_batch=slots).load_synthetic(0xF15E5EED)
    prompts = _prompts(slots, args.prompt_len, 1, tok)
    budget = args.prompt_len + args.max_frames
    res = {m: [] for m in args.modes}

    def one_round(mode):
        with lm.session(**(KW if mode == "score" else dict(KW, trace=True))) as s:
            for i, p in enumerate(prompts):  # (a seed of its own in every mode: the same prefill passes, the same streams)
                assert s.add(p, budget, seed=1000 + i, **(dict(trace=True) if mode == "trace_all_traced" else {})) is not None
            assert s.step(args.warmup) == slots
            st0 = lm.last_stats()
            while True:
                live = s.step(8)
                st = lm.last_stats()
                if st["decode_ms"] - st0["decode_ms"] >= args.seconds * 1000.0 or live < slots:
                    break
            assert live == slots, "slots finished inside the timed window: raise --max-frames"
            if mode == "trace_all_traced":
                assert s.poll_trace(0)["tokens"].shape[0] == s.poll(0, codes=False)[0]
            return (st["decode_ms"] - st0["decode_ms"]) * 1000.0 / (st["graph_launches"] - st0["graph_launches"])

    for m in args.modes:  # untimed: graph capture, allocations
        one_round(m)
    for r in range(args.rounds):
        for m in args.modes:
            res[m].append(one_round(m))
            print(f"{slots} slots, round {r} {m}: {res[m][-1]:.1f} us / step", flush=True)
    lm.close()
    out = {}
    for m in args.modes:
        med = statistics.median(res[m])
        out[m] = dict(us_per_step=res[m], median_us=med, spread=(max(res[m]) - min(res[m])) / med)
    if "score" in out:
        for m in args.modes[1:] if args.modes[0] == "score" else ():
            out[m + "_over_score"] = out[m]["median_us"] / out["score"]["median_us"] - 1.0
    return out


def generate_rates(args):
    import numpy as np
    import fishrt
    from fishrt import config as fcfg
    cfg, tok = fcfg.FISH_1_5, fcfg.FISH_1_5_TOKENS
    n, N, L = args.gen_slots, args.gen_frames, args.prompt_len
    lm = fishrt.DualARTransformer(cfg, tok, 0, "bf16", max_batch=n).load_synthetic(0xF15E5EED)
    prompts = _prompts(n, L, 2, tok)
    rs = np.random.RandomState(3)
    frames = []
    for _ in range(n):
        f = np.zeros((9, N), np.uint32)
        f[0] = tok["semantic_start_id"] + rs.randint(0, cfg["vocab_size"] - tok["semantic_start_id"], N)
        f[1:] = rs.randint(0, cfg["codebook_size"], (8, N))
        frames.append(f)
    sampling = {k: KW[k] for k in ("temp", "top_p", "top_k", "repetition_penalty")}

    def two_pass():
        with lm.session(**dict(KW, score=False)) as s:
            slots = [s.add(p, L + N - 2, seed=7 + i) for i, p in enumerate(prompts)]
            assert None not in slots
            while s.step(8):
                pass
            codes = [s.poll(sl)[0] for sl in slots]
        assert all(c.shape == (8, N) for c in codes)
        out = lm.score(prompts, frames)
        assert len(out) == n and all(o["logprob"].shape == (N, 9) for o in out)

    def traced():
        # (the session of generate_traced with this bench's settings: ignore-eos, so that every request runs its N iterations)
        with lm.session(**dict(KW, trace=True)) as s:
            slots = [s.add(p, L + N - 2, seed=7 + i, trace=True) for i, p in enumerate(prompts)]
            assert None not in slots
            while s.step(8):
                pass
            out = [(s.poll(sl)[0], s.poll_trace(sl)) for sl in slots]
        assert all(c.shape == (8, N) and t["logprob"].shape == (N, 9) and np.isfinite(t["logprob"]).all() for c, t in out)

    res = {}
    for name, fn in (("generate_then_score", two_pass),) + ((("generate_traced", traced),) if not args.lib else ()):
        fn()  # untimed: graph capture, allocations
        res[name] = []
    for r in range(args.rounds):
        for name, fn in (("generate_then_score", two_pass), ("generate_traced", traced)):
            if name not in res:
                continue
            t0 = time.perf_counter()
            fn()
            res[name].append(time.perf_counter() - t0)
            print(f"{name} round {r}: {n} requests x {N} frames in {res[name][-1]:.3f} s", flush=True)
    lm.close()
    out = dict(requests=n, frames=N, prompt_len=L, sampling=sampling)
    for name, secs in res.items():
        out[name] = dict(seconds=secs, median_s=statistics.median(secs))
    if "generate_traced" in out:
        out["traced_over_two_pass"] = out["generate_traced"]["median_s"] / out["generate_then_score"]["median_s"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--slots", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--modes", nargs="+", default=list(MODES), choices=MODES)
    ap.add_argument("--lib", help="another build of libfishrt.so (an earlier commit's: --modes score only)")
    ap.add_argument("--prompt-len", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=0.35, help="timed decode time per round and mode")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--max-frames", type=int, default=600)
    ap.add_argument("--gen-slots", type=int, default=32)
    ap.add_argument("--gen-frames", type=int, default=256)
    ap.add_argument("--no-generate", action="store_true", help="step times only")
    ap.add_argument("--out")
    a = ap.parse_args()
    import fishrt
    if a.lib:
        if a.modes != ["score"]:
            ap.error("--lib runs a build without the flag: --modes score")
        fishrt._ffi.LIB_PATH = os.path.abspath(a.lib)
        fishrt._ffi.TRACE_PROTOTYPES = {}  # (that build does not export the traced-slot entry points)
    out = dict(version=fishrt.lib().fs_version().decode(), lib=a.lib or "this build", prompt_len=a.prompt_len, seconds_per_round=a.seconds,
               rounds=a.rounds, sampling={k: KW[k] for k in ("temp", "top_p", "top_k", "repetition_penalty")}, step={})
    for slots in a.slots:
        out["step"][str(slots)] = step_times(a, slots)
    if not a.no_generate:
        out["generate"] = generate_rates(a)
    text = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    print(json.dumps(dict(step={k: {m: v[m]["median_us"] for m in a.modes} for k, v in out["step"].items()},
                          generate={k: v["median_s"] for k, v in out.get("generate", {}).items() if isinstance(v, dict) and "median_s" in v})))


if __name__ == "__main__":
    main()
