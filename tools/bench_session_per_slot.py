"""Step time of a FS_SESSION_PER_SLOT session against the lock-step session step (include/fishrt.h).

    python tools/bench_session_per_slot.py --out new.json                      # this build: both modes, alternated in one process
    python tools/bench_session_per_slot.py --lib /path/libfishrt.so --out parent.json   # another build (a parent commit; lock-step only if it lacks the mode)
    python tools/bench_session_per_slot.py --merge parent.json [parent2.json ...] new.json --out profiles/session_per_slot_step.json

32 live slots (--slots), ignore-eos, sampling 0.7 / 0.8 / 256 with repetition penalty 1.4, Fish-1.5 shapes, synthetic bf16 weights.  A
round opens a session, admits the slots, warms up, then steps until --seconds of decode time have passed; the step time is the handle's
own HIP-event time around the session_step launches (last_stats()["decode_ms"]) divided by the frames launched.  Rounds of the two modes
alternate, every round starts from the same prompts, so both modes walk the same KV lengths.  Per mode: every round's figure, the median
and the run-to-run spread (max - min) / median.  --merge states the two checks: the per-slot step within 5 % of the PARENT's lock-step
step, and this build's lock-step step inside the parent's own run-to-run spread (over all rounds of all the parent runs given: run the
parent before AND after the new build, a process-to-process shift is larger than the spread inside one process).  Where the parent runs
have the per-slot mode too, the same spread check is stated for per-slot against the parent's per-slot."""
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
    has_per_slot = hasattr(fishrt.lib(), "fs_lm_session_add_ex")
    tok = fcfg.FISH_1_5_TOKENS
    lm = fishrt.DualARTransformer(fcfg.FISH_1_5, tok, 0, "bf16", max_batch=args.slots).load_synthetic(0xF15E5EED)
    rs = np.random.RandomState(1)
    prompts = []
    for _ in range(args.slots):
        p = np.zeros((9, args.prompt_len), np.uint32)
        p[0] = rs.randint(0, tok["im_end_id"], args.prompt_len)
        prompts.append(p)
    kw = dict(temp=0.7, top_p=0.8, top_k=256, seed=42, ignore_eos=True)
    modes = ["lock_step"] + (["per_slot"] if has_per_slot else [])
    res = {m: [] for m in modes}
    budget = args.prompt_len + args.max_frames

    def one_round(mode):
        s = lm.session(per_slot=True, repetition_penalty=1.4, **kw) if mode == "per_slot" else lm.session(**kw)
        with s:
            for p in prompts:
                assert s.add(p, budget) is not None
            assert s.step(args.warmup) == args.slots
            st0 = lm.last_stats()
            while True:
                live = s.step(8)
                st = lm.last_stats()
                if st["decode_ms"] - st0["decode_ms"] >= args.seconds * 1000.0 or live < args.slots:
                    break
            assert live == args.slots, "slots finished inside the timed window: raise --max-frames"
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
    rounds = [x for p in parents for x in p["lock_step"]["us_per_step"]]
    base = statistics.median(rounds)
    out = dict(parent_runs=parents, new=new)
    out["parent_lock_step_us"] = dict(median=base, min=min(rounds), max=max(rounds), spread=(max(rounds) - min(rounds)) / base,
                                      run_medians=[p["lock_step"]["median_us"] for p in parents])
    out["per_slot_over_parent_lock_step"] = new["per_slot"]["median_us"] / base - 1.0
    out["per_slot_within_5_percent"] = out["per_slot_over_parent_lock_step"] <= 0.05
    out["lock_step_new_over_parent"] = new["lock_step"]["median_us"] / base - 1.0
    out["lock_step_inside_parent_spread"] = min(rounds) <= new["lock_step"]["median_us"] <= max(rounds)
    if all("per_slot" in p for p in parents):  # a parent that has the mode: the same spread check, per-slot against per-slot
        ps = [x for p in parents for x in p["per_slot"]["us_per_step"]]
        pbase = statistics.median(ps)
        out["parent_per_slot_us"] = dict(median=pbase, min=min(ps), max=max(ps), spread=(max(ps) - min(ps)) / pbase,
                                         run_medians=[p["per_slot"]["median_us"] for p in parents])
        out["per_slot_new_over_parent"] = new["per_slot"]["median_us"] / pbase - 1.0
        out["per_slot_inside_parent_spread"] = min(ps) <= new["per_slot"]["median_us"] <= max(ps)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", help="libfishrt.so to measure (default: the in-tree build); one without fs_lm_session_add_ex runs lock-step only")
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
