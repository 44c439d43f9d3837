"""Shared session prefixes on the device, plain adds vs prefixed adds, full-size Fish-1.5 bf16 with synthetic weights.  Prints ONE JSON line.

(a) burst: 32 requests sharing a 340-position conditioning prefix (bodies U{24..48}) into an idle max_batch = 32 static-batch session;
    per variant: prefill-stream time (fs_lm_session_info), prefill passes, KV pages in use once all are admitted, whole-job wall time.
    The two variants alternate, --reps times each.
(b) join: one request joins an 8-slot FS_SESSION_ROWS session whose other 7 slots are generating; time from the add to the joining
    slot's first frame, the prefill-stream time of the join, and the decode-stream time of the other slots over that interval (HIP
    events of session_step, fs_lm_last_stats decode_ms; per frame) next to the wall time per step call (host activation and polling
    included).

    python tools/bench_session_prefix.py [--reps 3] [--frames 16] [--out profiles/session_prefix.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fish-speech.rs_amd")]

import fishrt  # noqa: E402
from fishrt import config as fcfg  # noqa: E402

SEED = 0xF15E5EED
TOK = fcfg.FISH_1_5_TOKENS


def _prompt(L, seed):
    p = np.zeros((9, L), np.uint32)
    p[0] = np.random.RandomState(seed).randint(0, TOK["im_end_id"], L)
    return p


def burst(lm, prefix, bodies, frames, prefixed):
    t0 = time.perf_counter()
    with lm.session(temp=0.0, top_p=1.0, top_k=0, seed=1, ignore_eos=True) as s:
        free0 = s.info()["free_pages"]
        pid = s.add_prefix(prefix) if prefixed else None
        live = {}
        for i, b in enumerate(bodies):
            L = b.shape[1] + prefix.shape[1]
            slot = s.add(b, L + frames - 2, prefix=pid) if prefixed else s.add(np.concatenate([prefix, b], 1), L + frames - 2)
            assert slot is not None, "session full"
            live[slot] = i
        s.step(1)  # idle session: every queued request is admitted (group pass after group pass), then one frame
        info = s.info()
        while live:
            s.step(8)
            for slot in list(live):
                if s.poll(slot, codes=False)[1]:
                    s.release(slot)
                    live.pop(slot)
    wall = time.perf_counter() - t0
    return dict(prefill_ms=info["prefill_us"] / 1e3, passes=info["prefill_passes"], pages_in_use=free0 - info["free_pages"],
                tokens_prefilled=info["tokens_prefilled"], shared_pages=info["shared_pages"], wall_ms=wall * 1e3)


def join(lm, prefix, body, prefixed):
    with lm.session(temp=0.0, top_p=1.0, top_k=0, seed=1, ignore_eos=True, rows=True, repetition_penalty=1.2) as s:
        pid = s.add_prefix(prefix) if prefixed else None
        others = [s.add(_prompt(prefix.shape[1] + 30, 50 + k), prefix.shape[1] + 30 + 400) for k in range(7)]
        s.step(4)  # the 7 are live and generating (and the prefix, if any, is prefilled)
        before = s.info()
        n0 = sum(s.poll(o, codes=False)[0] for o in others)
        d0 = lm.last_stats()["decode_ms"]  # (HIP-event time of the decode stream, summed over session_step calls)
        t0 = time.perf_counter()
        L = prefix.shape[1] + body.shape[1]
        slot = s.add(body, L + 40, prefix=pid) if prefixed else s.add(np.concatenate([prefix, body], 1), L + 40)
        steps = 0
        while s.poll(slot, codes=False)[0] < 1:
            s.step(1)
            steps += 1
        dt = time.perf_counter() - t0
        decode_ms = lm.last_stats()["decode_ms"] - d0
        n1 = sum(s.poll(o, codes=False)[0] for o in others)
        after = s.info()
    return dict(first_frame_ms=dt * 1e3, join_prefill_ms=(after["prefill_us"] - before["prefill_us"]) / 1e3, steps=steps,
                others_frames=int(n1 - n0), others_decode_ms=decode_ms, others_decode_ms_per_frame=decode_ms / max(1, steps),
                wall_ms_per_step=dt * 1e3 / max(1, steps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--part", choices=["a", "b", "ab"], default="ab")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.RandomState(0)
    prefix = _prompt(340, 7)
    bodies = [_prompt(int(rng.randint(24, 49)), 100 + i) for i in range(32)]
    res = dict(workload="session_prefix", prefix_len=340, body_lens=[b.shape[1] for b in bodies], frames=a.frames)
    if "a" in a.part:
        lm = fishrt.DualARTransformer(fcfg.FISH_1_5, TOK, 0, "bf16", max_batch=32).load_synthetic(SEED)
        burst(lm, prefix, bodies[:4], 4, True)  # warm-up (buffers, graphs)
        runs = {"plain": [], "prefixed": []}
        for _ in range(a.reps):
            for v in ("plain", "prefixed"):
                runs[v].append(burst(lm, prefix, bodies, a.frames, v == "prefixed"))
        lm.close()
        med = {v: {k: float(np.median([r[k] for r in rs])) for k in rs[0]} for v, rs in runs.items()}
        res["a"] = dict(runs=runs, median=med, prefill_speedup=med["plain"]["prefill_ms"] / max(1e-9, med["prefixed"]["prefill_ms"]),
                        pages_saved=med["plain"]["pages_in_use"] - med["prefixed"]["pages_in_use"])
    if "b" in a.part:
        lm = fishrt.DualARTransformer(fcfg.FISH_1_5, TOK, 0, "bf16", max_batch=8).load_synthetic(SEED)
        join(lm, prefix, bodies[0], True)  # warm-up
        runs = {"plain": [], "prefixed": []}
        for r in range(a.reps):
            for v in ("plain", "prefixed"):
                runs[v].append(join(lm, prefix, bodies[1 + r], v == "prefixed"))
        lm.close()
        med = {v: {k: float(np.median([x[k] for x in rs])) for k in rs[0]} for v, rs in runs.items()}
        res["b"] = dict(runs=runs, median=med)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
