"""Prefixes from a slot's history (fs_lm_session_prefix_from_slot): what a second turn costs, and what a promotion costs the slots that
are generating.  Full-size Fish-1.5 bf16 with synthetic weights, the default voice's prompt (bench.default_voice_prompt: 367 positions), a
per-slot session.  Prints ONE JSON line.

(a) turn 2: a slot has generated H = 64 / 256 frames behind the default voice; the next turn has a body of 30 columns (the last frame's
    column + 29).  Time from the call to the new slot's first frame -- the call, the prefill of what has to be prefilled, one decode step --
    through Session.continue_from (the history's rows are shared / copied, the body is prefilled) against a plain add of the concatenated
    tokens (everything is prefilled).  The two alternate, --reps each, in one process; fs_lm_session_info's prefill-stream time alongside.
(b) step time: 16 sampled slots generate; wall time per decode step over 256 steps in step(8) calls while ONE slot is promoted every 8
    steps (the prefix is released at once), against the same session without promotions.  Same build, alternating PROCESSES, --reps each.

The parent process never opens the GPU: every measurement runs in a child of its own.

    python tools/bench_session_history.py [--reps 5] [--out profiles/session_history.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fish-speech.rs_amd")]

SEED = 0xF15E5EED
BODY = 30
GREEDY = dict(temp=0.0, top_p=1.0, top_k=0, seed=1, ignore_eos=True, per_slot=True, repetition_penalty=1.0)
SAMPLED = dict(temp=0.7, top_p=0.8, top_k=50, seed=1, ignore_eos=True, per_slot=True, repetition_penalty=1.2)


def _handle():
    import fishrt
    from fishrt import config as fcfg
    return fishrt.DualARTransformer(fcfg.FISH_1_5, fcfg.FISH_1_5_TOKENS, 0, "bf16", max_batch=16).load_synthetic(SEED)


def _first_frame(s, slot):
    while s.poll(slot, codes=False)[0] < 1:
        s.step(1)


def turn2(lm, prompt, body, H, how):
    from fishrt import config as fcfg
    L = prompt.shape[1]
    with lm.session(**GREEDY) as s:
        a = s.add(prompt, L + H - 2)
        while s.step(8):
            pass
        codes, done = s.poll(a)
        assert done and codes.shape[1] == H
        col = s.last_frame(a)
        if how == "plain":  # the tokens of the concatenation (timing only: the slow tokens of the history are stood in for by code 0's)
            hist = np.concatenate([(fcfg.FISH_1_5_TOKENS["semantic_start_id"] + codes[:1]).astype(np.uint32), codes], 0)
            full = np.ascontiguousarray(np.concatenate([prompt, hist[:, : H - 1], col[:, None], body], 1))
        before = s.info()
        t0 = time.perf_counter()
        if how == "continue":
            new, _ = s.continue_from(a, body, L + H + BODY + 40)
        else:
            new = s.add(full, L + H + BODY + 40)
        t1 = time.perf_counter()
        assert new is not None
        _first_frame(s, new)
        t2 = time.perf_counter()
        info = s.info()
    return dict(call_ms=(t1 - t0) * 1e3, to_first_frame_ms=(t2 - t0) * 1e3, prefill_stream_ms=(info["prefill_us"] - before["prefill_us"]) / 1e3,
                tokens_prefilled=info["tokens_prefilled"] - before["tokens_prefilled"], tail_pages_copied=info["tail_pages_copied"] - before["tail_pages_copied"])


def child_turn2(reps):
    import bench
    from fishrt import config as fcfg
    lm = _handle()
    prompt = bench.default_voice_prompt(fcfg.FISH_1_5_TOKENS)
    body = np.ascontiguousarray(prompt[:, -(BODY - 1):])
    out = {}
    for H in (64, 256):
        for how in ("continue", "plain"):
            turn2(lm, prompt, body, H, how)  # warm-up: buffers, step and prefill graphs of these shapes
        runs = {"continue": [], "plain": []}
        for _ in range(reps):
            for how in runs:
                runs[how].append(turn2(lm, prompt, body, H, how))
        out[str(H)] = dict(runs=runs, median={v: {k: float(np.median([r[k] for r in rs])) for k in rs[0]} for v, rs in runs.items()})
    lm.close()
    return dict(prompt_len=int(prompt.shape[1]), body_len=BODY, history=out)


def child_steps(promote, steps=256, every=8, slots=16):
    import bench
    from fishrt import config as fcfg
    lm = _handle()
    prompt = bench.default_voice_prompt(fcfg.FISH_1_5_TOKENS)
    with lm.session(**SAMPLED) as s:
        live = [s.add(prompt, prompt.shape[1] + steps + 200, seed=100 + i) for i in range(slots)]
        assert None not in live
        s.step(32)  # warm-up: every slot is live, the step graph of this bucket is captured
        n_promoted = 0
        t0 = time.perf_counter()
        for i in range(steps // every):
            s.step(every)
            if promote:
                pid, _ = s.prefix_from_slot(live[i % slots])
                assert pid is not None
                s.release_prefix(pid)
                n_promoted += 1
        wall = time.perf_counter() - t0
        info = s.info()
    lm.close()
    return dict(ms_per_step=wall * 1e3 / steps, promotions=n_promoted, tail_pages_copied=info["tail_pages_copied"])


def _child(args):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + args, stdout=subprocess.PIPE, universal_newlines=True, check=True)
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs="+", default=None)
    a = ap.parse_args()
    if a.child:
        what = a.child[0]
        res = child_turn2(int(a.child[1])) if what == "turn2" else child_steps(what == "promote")
        print(json.dumps(res))
        return
    res = dict(workload="session_history", reps=a.reps)
    res["a"] = _child(["turn2", str(a.reps)])
    runs = {"none": [], "promote": []}
    for _ in range(a.reps):  # alternating processes of the same build
        for how in runs:
            runs[how].append(_child([how]))
    med = {v: float(np.median([r["ms_per_step"] for r in rs])) for v, rs in runs.items()}
    res["b"] = dict(steps=256, promote_every=8, live_slots=16, runs=runs, median_ms_per_step=med,
                    spread_ms_per_step={v: [float(min(r["ms_per_step"] for r in rs)), float(max(r["ms_per_step"] for r in rs))] for v, rs in runs.items()})
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
