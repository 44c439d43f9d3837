"""Prefix KV blobs: importing a voice's conditioning K/V against prefilling it, full-size Fish-1.5 bf16 with synthetic weights and the default
voice's conditioning (system + user text + the voice's VQ span + <|im_end|>: 339 positions).  The create path of the same build is the
yardstick.  Prints ONE JSON line.

(a) activate: time from the call (Session.add_prefix / Session.import_prefix) to an activated prefix in an idle session -- the call plus
    the step() that waits for its pass -- and the prefill-stream time of that pass (fs_lm_session_info).  The two alternate, --reps each.
(b) join: 16 slots of a max_batch = 32 session are generating; wall time of 64 single-frame step() calls during which one cold voice joins
    (the prefix by create or by import, plus a request on it, both issued before the first of the 64 steps), against the same 64 steps
    with no join; and the step at which the joining slot has its first frame.

    python tools/bench_prefix_import.py [--reps 5] [--out profiles/prefix_import.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fish-speech.rs_amd")]

import bench  # noqa: E402
import fishrt  # noqa: E402
from fishrt import config as fcfg  # noqa: E402

SEED = 0xF15E5EED
TOK = fcfg.FISH_1_5_TOKENS
P_COND = 12 + 48 + 4 + 274 + 1  # bench.default_voice_prompt: [sys][user][assistant][VQ span][im_end] | [user 24][assistant 4]
KW = dict(temp=0.0, top_p=1.0, top_k=0, seed=1, ignore_eos=True)


def activate(lm, cond, blob):
    with lm.session(**KW) as s:
        t0 = time.perf_counter()
        pid = s.add_prefix(cond) if blob is None else s.import_prefix(blob)
        t1 = time.perf_counter()
        s.step(1)  # nothing live: the queued pass runs and is activated
        t2 = time.perf_counter()
        info = s.info()
        assert pid is not None and info["live_prefixes"] == 1
    return dict(call_ms=(t1 - t0) * 1e3, total_ms=(t2 - t0) * 1e3, prefill_stream_ms=info["prefill_us"] / 1e3, passes=info["prefill_passes"])


def join(lm, prompt, cond, body, blob, how, steps=64, others=16):
    with lm.session(**KW) as s:
        slots = [s.add(prompt, prompt.shape[1] + 400) for _ in range(others)]
        assert None not in slots
        s.step(4)
        t0 = time.perf_counter()
        slot, first = None, None
        if how != "none":
            pid = s.add_prefix(cond) if how == "create" else s.import_prefix(blob)
            slot = s.add(body, cond.shape[1] + body.shape[1] + 200, prefix=pid)
            assert pid is not None and slot is not None
        for i in range(steps):
            s.step(1)
            if slot is not None and first is None and s.poll(slot, codes=False)[0] >= 1:
                first = i + 1
        wall = time.perf_counter() - t0
        info = s.info()
    return dict(wall_ms=wall * 1e3, first_frame_step=first or 0, prefill_stream_ms=info["prefill_us"] / 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    prompt = bench.default_voice_prompt(TOK)
    cond, body = np.ascontiguousarray(prompt[:, :P_COND]), np.ascontiguousarray(prompt[:, P_COND:])
    lm = fishrt.DualARTransformer(fcfg.FISH_1_5, TOK, 0, "bf16", max_batch=32).load_synthetic(SEED)
    with lm.session(**KW) as s:
        blob = s.export_prefix(s.add_prefix(cond))
    res = dict(workload="prefix_import", prefix_len=int(cond.shape[1]), body_len=int(body.shape[1]), blob_bytes=len(blob), reps=a.reps)
    activate(lm, cond, None), activate(lm, cond, blob)  # warm-up (buffers, the staging buffer)
    runs = {"create": [], "import": []}
    for _ in range(a.reps):
        runs["create"].append(activate(lm, cond, None))
        runs["import"].append(activate(lm, cond, blob))
    med = {v: {k: float(np.median([r[k] for r in rs])) for k in rs[0]} for v, rs in runs.items()}
    res["a"] = dict(runs=runs, median=med)
    join(lm, prompt, cond, body, blob, "import", steps=8)  # warm-up (step graphs)
    runs = {"none": [], "create": [], "import": []}
    for _ in range(a.reps):
        for how in runs:
            runs[how].append(join(lm, prompt, cond, body, blob, how))
    med = {v: {k: float(np.median([r[k] for r in rs])) for k in rs[0]} for v, rs in runs.items()}
    res["b"] = dict(steps=64, live_slots=16, runs=runs, median=med)
    lm.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
