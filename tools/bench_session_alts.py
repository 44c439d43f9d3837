"""What FS_SESSION_ALTS costs.  The protocol of tools/bench_session_trace.py:

    python tools/bench_session_alts.py --out profiles/session_alts.json

1. Step time of a SAMPLED per-slot session of 16 and of 32 live slots (--slots) in these modes (--modes):
     "trace"               FS_SESSION_PER_SLOT | SCORE | TRACE with plain slots: the graphs such a session always replayed
     "alts_no_slot"        the same session with FS_SESSION_ALTS (N = 8) and no scoring or traced slot: the second instantiation of the
                           score nodes is in the graph and every block of it exits at once
     "trace_all_traced"    the first session with every slot traced (the figure the next three are read against)
     "alts1_all_traced", "alts8_all_traced", "alts16_all_traced"   every slot traced, N = 1, 8, 16: every score node selects
   Ignore-eos, sampling 0.7 / 0.8 / 256 with repetition penalty 1.4, Fish-1.5 shapes, synthetic bf16 weights.  A round opens a session,
   admits the slots, warms up, then steps until --seconds of decode time have passed; the step time is the handle's own HIP-event time
   around the session_step launches divided by the frames launched.  Rounds of the modes alternate, each mode is warmed up by an untimed
   round first.  Per mode: every round's figure, the median, the spread (max - min) / median; the ratios of the medians over "trace" and
   over "trace_all_traced".
2. Wall time of score() of --score-seqs x --score-frames (32 x 256) with top_n 0, 8 and 16: one untimed call each, then the median of
   --rounds calls, alternating.
3. --lib PATH runs on another build of the library (an earlier commit's, for the "trace" and "trace_all_traced" modes and score() without
   top_n: alternate processes of the two builds and compare their medians).
4. The node's arithmetic against an f64 computation on --parity-rows random rows of 2037 and 1024 candidates (fs_selftest_alt_rows,
   N = 16): the worst |log-prob error| and |entropy error|, next to the bounds the tests hold (2e-4, 2.5e-3).

No threshold is built in: the tool reports."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fish-speech.rs_amd")]

# mode -> (alts N, every slot traced)
MODES = {"trace": (0, False), "alts_no_slot": (8, False), "trace_all_traced": (0, True), "alts1_all_traced": (1, True),
         "alts8_all_traced": (8, True), "alts16_all_traced": (16, True)}
KW = dict(temp=0.7, top_p=0.8, top_k=256, seed=42, ignore_eos=True, per_slot=True, score=True, trace=True, repetition_penalty=1.4)


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
        n_alts, traced = MODES[mode]
        with lm.session(**(dict(KW, alts=n_alts) if n_alts else KW)) as s:
            for i, p in enumerate(prompts):  # (a seed of its own in every mode: the same prefill passes, the same streams)
                assert s.add(p, budget, seed=1000 + i, **(dict(trace=True) if traced else {})) is not None
            assert s.step(args.warmup) == slots
            st0 = lm.last_stats()
            while True:
                live = s.step(8)
                st = lm.last_stats()
                if st["decode_ms"] - st0["decode_ms"] >= args.seconds * 1000.0 or live < slots:
                    break
            assert live == slots, "slots finished inside the timed window: raise --max-frames"
            if traced:
                rows = s.poll(0, codes=False)[0]
                assert s.poll_trace(0)["tokens"].shape[0] == rows
                if n_alts:
                    al = s.poll_alts(0)
                    assert al["alt_index"].shape == (rows, 9, n_alts) and (al["alt_index"][..., 0] == s.poll_trace(0)["top"]).all()
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
    for base in ("trace", "trace_all_traced"):
        for m in args.modes:
            if base in out and m != base and MODES[m][1] == MODES[base][1]:
                out[f"{m}_over_{base}"] = out[m]["median_us"] / out[base]["median_us"] - 1.0
    return out


def score_rates(args):
    import numpy as np
    import fishrt
    from fishrt import config as fcfg
    cfg, tok = fcfg.FISH_1_5, fcfg.FISH_1_5_TOKENS
    n, N, L = args.score_seqs, args.score_frames, args.prompt_len
    lm = fishrt.DualARTransformer(cfg, tok, 0, "bf16", max_batch=n).load_synthetic(0xF15E5EED)
    prompts = _prompts(n, L, 2, tok)
    rs = np.random.RandomState(3)
    frames = []
    for _ in range(n):
        f = np.zeros((9, N), np.uint32)
        f[0] = tok["semantic_start_id"] + rs.randint(0, cfg["vocab_size"] - tok["semantic_start_id"], N)
        f[1:] = rs.randint(0, cfg["codebook_size"], (8, N))
        frames.append(f)
    tops = (0,) if args.lib else (0, 8, 16)
    res = {t: [] for t in tops}

    def run(top_n):
        out = lm.score(prompts, frames, top_n=top_n) if top_n else lm.score(prompts, frames)
        assert len(out) == n and all(o["logprob"].shape == (N, 9) for o in out)
        assert not top_n or all(o["alt_index"].shape == (N, 9, top_n) and np.isfinite(o["entropy"]).all() for o in out)

    for t in tops:
        run(t)  # untimed: graph capture, allocations
    for r in range(args.rounds):
        for t in tops:
            t0 = time.perf_counter()
            run(t)
            res[t].append(time.perf_counter() - t0)
            print(f"score top_n={t} round {r}: {n} sequences x {N} frames in {res[t][-1]:.3f} s", flush=True)
    lm.close()
    out = dict(sequences=n, frames=N, prompt_len=L)
    for t in tops:
        med = statistics.median(res[t])
        out[f"top_n_{t}"] = dict(seconds=res[t], median_s=med, frames_per_s=n * N / med)
    for t in tops[1:]:
        out[f"top_n_{t}_over_0"] = out[f"top_n_{t}"]["median_s"] / out["top_n_0"]["median_s"] - 1.0
    return out


def parity(args):
    import numpy as np
    import fishrt
    out = {}
    for n in (2037, 1024):
        rows = np.ascontiguousarray(np.random.RandomState(n).normal(0.0, 3.0, (args.parity_rows, n)).astype(np.float32))
        S, N = rows.shape[0], 16
        idx, lp, ent = np.zeros((S, N), np.uint32), np.zeros((S, N), np.float32), np.zeros(S, np.float32)
        fp = C.POINTER(C.c_float)
        fishrt._ffi.check(fishrt.lib().fs_selftest_alt_rows(0, rows.ctypes.data_as(fp), S, n, 0, N, idx.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                            lp.ctypes.data_as(fp), ent.ctypes.data_as(fp)))
        x = rows.astype(np.float64)
        d = x - x.max(axis=1, keepdims=True)
        ls = np.log(np.exp(d).sum(axis=1, keepdims=True))
        want_lp = np.take_along_axis(d - ls, idx.astype(np.int64), axis=1)
        p = np.exp(d - ls)
        want_ent = -(p * (d - ls)).sum(axis=1)
        order = np.argsort(-x, axis=1, kind="stable")[:, :N]
        out[str(n)] = dict(rows=S, n_alts=N, indices_equal=bool((np.take_along_axis(x, order, 1) == np.take_along_axis(x, idx.astype(np.int64), 1)).all()),
                           worst_logprob_err=float(np.abs(lp - want_lp).max()), worst_entropy_err=float(np.abs(ent - want_ent).max()))
    out["bounds"] = dict(logprob=2e-4, entropy=2.5e-3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--slots", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--modes", nargs="+", default=list(MODES), choices=list(MODES))
    ap.add_argument("--prompt-len", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=0.35, help="timed decode time per round and mode")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--max-frames", type=int, default=600)
    ap.add_argument("--score-seqs", type=int, default=32)
    ap.add_argument("--score-frames", type=int, default=256)
    ap.add_argument("--parity-rows", type=int, default=512)
    ap.add_argument("--no-score", action="store_true", help="step times only")
    ap.add_argument("--lib", help="another build of libfishrt.so (an earlier commit's: --modes trace trace_all_traced only)")
    ap.add_argument("--out")
    a = ap.parse_args()
    import fishrt
    if a.lib:
        if any(MODES[m][0] for m in a.modes):
            ap.error("--lib runs a build without the flag: --modes trace trace_all_traced")
        fishrt._ffi.LIB_PATH = os.path.abspath(a.lib)
        fishrt._ffi.ALTS_PROTOTYPES = {}  # (that build does not export the alternatives' entry points)
    out = dict(version=fishrt.lib().fs_version().decode(), lib=a.lib or "this build", prompt_len=a.prompt_len, seconds_per_round=a.seconds, rounds=a.rounds,
               sampling={k: KW[k] for k in ("temp", "top_p", "top_k", "repetition_penalty")}, step={})
    for slots in a.slots:
        out["step"][str(slots)] = step_times(a, slots)
    if not a.no_score:
        out["score"] = score_rates(a)
    if not a.lib:
        out["parity"] = parity(a)
    text = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    print(json.dumps(dict(step={k: {m: round(v[m]["median_us"], 1) for m in a.modes} for k, v in out["step"].items()},
                          score={k: round(v["median_s"], 3) for k, v in out.get("score", {}).items() if isinstance(v, dict)}, parity=out.get("parity"))))


if __name__ == "__main__":
    main()
