"""Step time of a FS_SESSION_PER_SLOT session whose slots collect hidden states (fs_lm_session_add_hidden) against the same step of a
parent build.  The protocol of tools/bench_session_per_slot.py:

    python tools/bench_session_hidden.py --lib /path/libfishrt.so --out parent.json   # a parent build (no fs_lm_session_add_hidden): per-slot step only
    python tools/bench_session_hidden.py --out new.json                               # this build: no slot collecting / all collecting, alternated
    python tools/bench_session_hidden.py --merge parent.json [parent2.json ...] new.json --out profiles/session_hidden_step.json

32 live slots (--slots), ignore-eos, sampling 0.7 / 0.8 / 256 with repetition penalty 1.4, Fish-1.5 shapes, synthetic bf16 weights.  A
round opens a session, admits the slots, warms up, then steps until --seconds of decode time have passed; the step time is the handle's
own HIP-event time around the session_step launches (last_stats()["decode_ms"]) divided by the frames launched.  Rounds of the modes
alternate, every round starts from the same prompts, so all modes walk the same KV lengths.  Per mode: every round's figure, the median
and the run-to-run spread (max - min) / median.  --merge states the two checks: with no slot collecting the step lies inside the
PARENT's own run-to-run spread (over all rounds of all the parent runs given: run the parent before AND after the new build, a
process-to-process shift is larger than the spread inside one process), and with every slot collecting it stays within 5 % of the
parent's median."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fish-speech.rs_amd")]


def measure(args):
    import numpy as np
    from fishrt import _ffi
    if args.lib:
        _ffi.LIB_PATH = os.path.abspath(args.lib)
    import fishrt
    from fishrt import config as fcfg
    has_hidden = hasattr(fishrt.lib(), "fs_lm_session_add_hidden")
    tok = fcfg.FISH_1_5_TOKENS
    lm = fishrt.DualARTransformer(fcfg.FISH_1_5, tok, 0, "bf16", max_batch=args.slots).load_synthetic(0xF15E5EED)
    rs = np.random.RandomState(1)
    prompts = []
    for _ in range(args.slots):
        p = np.zeros((9, args.prompt_len), np.uint32)
        p[0] = rs.randint(0, tok["im_end_id"], args.prompt_len)
        prompts.append(p)
    kw = dict(temp=0.7, top_p=0.8, top_k=256, seed=42, ignore_eos=True)
    modes = ["none_collecting"] + (["all_collecting"] if has_hidden else [])
    res = {m: [] for m in modes}
    budget = args.prompt_len + args.max_frames

    def one_round(mode):
        add_kw = dict(collect_hidden=True) if mode == "all_collecting" else {}
        with lm.session(per_slot=True, repetition_penalty=1.4, **kw) as s:
            for p in prompts:
                assert s.add(p, budget, **add_kw) is not None
            assert s.step(args.warmup) == args.slots
            st0 = lm.last_stats()
            while True:
                live = s.step(8)
                st = lm.last_stats()
                if st["decode_ms"] - st0["decode_ms"] >= args.seconds * 1000.0 or live < args.slots:
                    break
            assert live == args.slots, "slots finished inside the timed window: raise --max-frames"
            if add_kw:  # every slot really stored a row per step
                n = s.poll(0, codes=False)[0]
                assert s.poll_hidden(0, first=n - 1).shape[0] == 1 and s.poll_hidden(args.slots - 1, first=n - 1).shape[0] == 1
            return (st["decode_ms"] - st0["decode_ms"]) * 1000.0 / (st["graph_launches"] - st0["graph_launches"])

    for m in modes:  # untimed: graph capture, allocations
        one_round(m)
    for r in range(args.rounds):
        for m in modes:
            res[m].append(one_round(m))
            print(f"round {r} {m}: {res[m][-1]:.1f} us / step", flush=True)
    lm.close()
    out = dict(lib=args.lib or "in-tree", version=fishrt.lib().fs_version().decode(), slots=args.slots, prompt_len=args.prompt_len,
               seconds_per_round=args.seconds, rounds=args.rounds, sampling=dict(temp=0.7, top_p=0.8, top_k=256, repetition_penalty=1.4))
    for m in modes:
        med = statistics.median(res[m])
        out[m] = dict(us_per_step=res[m], median_us=med, spread=(max(res[m]) - min(res[m])) / med)
    return out


def merge(parents, new):
    """parents: one or more runs (processes) of the parent build; its run-to-run spread is taken over all their rounds"""
    rounds = [x for p in parents for x in p["none_collecting"]["us_per_step"]]
    base = statistics.median(rounds)
    out = dict(parent_runs=parents, new=new)
    out["parent_per_slot_us"] = dict(median=base, min=min(rounds), max=max(rounds), spread=(max(rounds) - min(rounds)) / base,
                                     run_medians=[p["none_collecting"]["median_us"] for p in parents])
    out["none_collecting_over_parent"] = new["none_collecting"]["median_us"] / base - 1.0
    out["none_collecting_inside_parent_spread"] = min(rounds) <= new["none_collecting"]["median_us"] <= max(rounds)
    out["all_collecting_over_parent"] = new["all_collecting"]["median_us"] / base - 1.0
    out["all_collecting_within_5_percent"] = out["all_collecting_over_parent"] <= 0.05
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", help="libfishrt.so to measure (default: the in-tree build); one without fs_lm_session_add_hidden measures the plain per-slot step only")
    ap.add_argument("--slots", type=int, default=32)
    ap.add_argument("--prompt-len", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=0.35, help="timed decode time per round and mode")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--max-frames", type=int, default=600)
    ap.add_argument("--merge", nargs="+", metavar="JSON", help="PARENT_JSON [PARENT_JSON ...] NEW_JSON")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.merge and len(a.merge) < 2:
        ap.error("--merge needs at least one parent run and the new run")
    out = merge([json.load(open(f)) for f in a.merge[:-1]], json.load(open(a.merge[-1]))) if a.merge else measure(a)
    text = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    print(text if a.merge else json.dumps({k: (v if not isinstance(v, dict) or "median_us" not in v else dict(median_us=v["median_us"], spread=v["spread"])) for k, v in out.items()}))


if __name__ == "__main__":
    main()
