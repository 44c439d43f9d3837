"""FS_SESSION_WIDE_SAMPLER: what the flag costs slots that do not need it, and what it buys slots that do.

    python tools/bench_session_wide.py --out profiles/session_wide.json

Fish-1.5 shapes, bf16, synthetic weights, ignore-eos (every slot stays live for the whole window), prompts of --prompt-len tokens.
Step time = the handle's own HIP-event time around the session_step launches (last_stats()["decode_ms"]) / frames launched.
 (a) narrow settings (the server default 0.7 / 0.8 / 256, penalty 1.4) at 16 and 32 slots: per-slot sessions without and with the flag,
     alternating in ONE process, --rounds times each.  The unflagged session runs the instantiations a build without the flag has, so
     its rounds are the baseline AND give the run-to-run spread the difference is judged by.
 (b) wide settings (nucleus-only: top_k = 0 with top_p = 0.8, and with top_p = 1.0 -- the longest sequential chains) at 4 / 16 / 32
     slots, all slots wide: step time and frames/s, against the same requests one after the other through fs_lm_generate (what a server
     does with such requests without the flag: the batch-1 path, persistent kernels, its general sampler)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fish-speech.rs_amd")]


def _commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        return os.environ.get("FISHRT_COMMIT", "unknown")


def _prompts(n, L, hi, seed=1):
    import numpy as np
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        p = np.zeros((9, L), np.uint32)
        p[0] = rs.randint(6, hi, L)
        out.append(p)
    return out


def _session_step_us(lm, prompts, budget, frames, warmup, wide, **kw):
    n = len(prompts)
    with lm.session(per_slot=True, wide=wide, ignore_eos=True, seed=42, **kw) as s:
        for p in prompts:
            assert s.add(p, budget) is not None
        assert s.step(warmup) == n
        st0 = lm.last_stats()
        live, done = n, 0
        while done < frames:
            live = s.step(8)
            done += 8
        st = lm.last_stats()
        assert live == n, "slots finished inside the timed window"
        return (st["decode_ms"] - st0["decode_ms"]) * 1000.0 / (st["graph_launches"] - st0["graph_launches"])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--narrow-slots", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--wide-slots", type=int, nargs="+", default=[4, 16, 32])
    ap.add_argument("--prompt-len", type=int, default=64)
    ap.add_argument("--frames", type=int, default=96, help="timed frames per round")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--out")
    a = ap.parse_args()

    import fishrt
    from fishrt import config as fcfg
    tok = fcfg.FISH_1_5_TOKENS
    budget = a.prompt_len + a.warmup + a.frames + 64
    narrow = dict(temp=0.7, top_p=0.8, top_k=256, repetition_penalty=1.4)
    wides = {"top_k=0 top_p=0.8": dict(temp=0.7, top_p=0.8, top_k=0, repetition_penalty=1.4),
             "top_k=0 top_p=1.0": dict(temp=0.7, top_p=1.0, top_k=0, repetition_penalty=1.4)}
    out = dict(commit=_commit(), version=fishrt.lib().fs_version().decode(), model="Fish-1.5 shapes, bf16, synthetic weights", prompt_len=a.prompt_len,
               frames=a.frames, rounds=a.rounds, narrow_settings=narrow, flag_on_narrow={}, wide={})
    for n in sorted(set(a.narrow_slots) | set(a.wide_slots)):
        lm = fishrt.DualARTransformer(fcfg.FISH_1_5, tok, 0, "bf16", max_batch=n).load_synthetic(0xF15E5EED)
        prompts = _prompts(n, a.prompt_len, tok["im_end_id"])
        if n in a.narrow_slots:
            for w in (False, True):  # untimed: graph capture of both instantiations, allocations
                _session_step_us(lm, prompts, budget, 16, a.warmup, w, **narrow)
            off, on = [], []
            for _ in range(a.rounds):  # alternating
                off.append(_session_step_us(lm, prompts, budget, a.frames, a.warmup, False, **narrow))
                on.append(_session_step_us(lm, prompts, budget, a.frames, a.warmup, True, **narrow))
            mo, mn = statistics.median(off), statistics.median(on)
            spread = (max(off) - min(off)) / mo
            delta = mn / mo - 1.0
            out["flag_on_narrow"][str(n)] = dict(unflagged_us_per_step=off, flagged_us_per_step=on, unflagged_median_us=mo, flagged_median_us=mn,
                                                 unflagged_run_to_run_spread=spread, flagged_over_unflagged=delta,
                                                 inside_unflagged_spread=bool(min(off) <= mn <= max(off) or abs(delta) <= spread))
            print(f"{n} slots, narrow settings: unflagged {mo:.1f} us/step (spread {spread * 100:.2f}%), flagged {mn:.1f} us/step ({delta * 100:+.2f}%)", flush=True)
        if n in a.wide_slots:
            for name, kw in wides.items():
                _session_step_us(lm, prompts, budget, 16, a.warmup, True, **kw)  # untimed
                rounds = [_session_step_us(lm, prompts, budget, a.frames, a.warmup, True, **kw) for _ in range(a.rounds)]
                med = statistics.median(rounds)
                # the same requests one after the other (ignore-eos: a.frames + 2 frames each)
                mnt = a.prompt_len + a.frames
                lm.clear_slow_layer_caches()
                lm.generate_blocking(prompts[0], mnt, seed=1, ignore_eos=True, **kw)  # untimed
                t0, nf = time.perf_counter(), 0
                for i, p in enumerate(prompts):
                    lm.clear_slow_layer_caches()
                    nf += lm.generate_blocking(p, mnt, seed=100 + i, ignore_eos=True, **kw).shape[1]
                dt = time.perf_counter() - t0
                fps = n * 1e6 / med
                out["wide"].setdefault(str(n), {})[name] = dict(us_per_step=rounds, median_us=med, frames_per_s=fps,
                                                                sequential=dict(requests=n, frames=nf, seconds=dt, frames_per_s=nf / dt, ms_per_frame=dt * 1000.0 / nf),
                                                                speedup_over_sequential=fps / (nf / dt))
                print(f"{n} slots, {name}: step {med:.1f} us, {fps:.0f} frames/s; sequential {nf / dt:.0f} frames/s ({fps / (nf / dt):.2f}x)", flush=True)
        lm.close()
    text = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
