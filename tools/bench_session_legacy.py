"""Per-slot sessions on a Fish <= 1.4 handle against the only path such a deployment had: one fs_lm_generate call after the other.

    python tools/bench_session_legacy.py --out legacy.json                       # Fish-1.4 shapes, fp8: sessions of 4 / 16 / 32 live slots + sequential
    python tools/bench_session_legacy.py --fish15-step [--lib /path/libfishrt.so] --out run.json   # 16-slot Fish-1.5 per-slot step of one build
    python tools/bench_session_legacy.py --merge legacy.json --new n1.json n2.json n3.json --parent p1.json p2.json p3.json \\
        --out profiles/session_legacy.json

Legacy part: synthetic fp8 weights, sampling 0.7 / 0.8 / 256 with repetition penalty 1.2, ignore-eos (every slot stays live for the whole
window).  Per slot count N: a session with N live slots, warmed up, stepped for --frames frames; step time = the handle's own HIP-event
time around the session_step launches (last_stats()["decode_ms"]) / frames launched; frames/s = N / step time.  Sequential: the same N
requests one after the other through fs_lm_generate (persistent kernels, what the server's batch-1 path runs), wall time per request
from submit to return; frames/s = frames generated / total time.
--fish15-step: step time of a 16-slot Fish-1.5 bf16 per-slot session at default settings (the 1.5 path must not pay for the legacy
branch of k_sample_slow_slots): run three processes of this build and three of the parent build, alternating; --merge states whether
this build's median lies inside the parent's run-to-run range or within its spread of it."""
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


def _session_step_us(lm, prompts, budget, frames, warmup, **kw):
    n = len(prompts)
    with lm.session(per_slot=True, ignore_eos=True, seed=42, **kw) as s:
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


def measure_legacy(a):
    import fishrt
    from fishrt import config as fcfg
    kw = dict(temp=0.7, top_p=0.8, top_k=256, repetition_penalty=1.2)
    out = dict(commit=_commit(), version=fishrt.lib().fs_version().decode(), model="Fish-1.4 shapes, fp8, synthetic weights", prompt_len=a.prompt_len,
               frames=a.frames, sampling=kw, sessions={}, sequential={})
    budget = a.prompt_len + a.warmup + a.frames + 64
    for n in a.slots:
        lm = fishrt.DualARTransformer(fcfg.FISH_1_4, fcfg.FISH_1_4_TOKENS, 0, "fp8", max_batch=n).load_synthetic(0xF15E5EED)
        prompts = _prompts(n, a.prompt_len, 400)
        _session_step_us(lm, prompts, budget, 16, a.warmup, **kw)  # untimed: graph capture, allocations
        rounds = [_session_step_us(lm, prompts, budget, a.frames, a.warmup, **kw) for _ in range(a.rounds)]
        med = statistics.median(rounds)
        out["sessions"][str(n)] = dict(us_per_step=rounds, median_us=med, frames_per_s=n * 1e6 / med)
        # the same requests one after the other (ignore-eos: a.frames + 2 frames each)
        mnt = a.prompt_len + a.frames
        lm.clear_slow_layer_caches()
        lm.generate_blocking(prompts[0], mnt, seed=1, ignore_eos=True, **kw)  # untimed
        t0, nf = time.perf_counter(), 0
        for i, p in enumerate(prompts):
            lm.clear_slow_layer_caches()
            nf += lm.generate_blocking(p, mnt, seed=100 + i, ignore_eos=True, **kw).shape[1]
        dt = time.perf_counter() - t0
        out["sequential"][str(n)] = dict(requests=n, frames=nf, seconds=dt, frames_per_s=nf / dt, ms_per_frame=dt * 1000.0 / nf)
        out["sessions"][str(n)]["speedup_over_sequential"] = out["sessions"][str(n)]["frames_per_s"] / (nf / dt)
        print(f"{n} slots: step {med:.1f} us, {n * 1e6 / med:.0f} frames/s; sequential {nf / dt:.0f} frames/s", flush=True)
        lm.close()
    return out


def measure_fish15(a):
    from fishrt import _ffi
    if a.lib:
        _ffi.LIB_PATH = os.path.abspath(a.lib)
    import fishrt
    from fishrt import config as fcfg
    lm = fishrt.DualARTransformer(fcfg.FISH_1_5, fcfg.FISH_1_5_TOKENS, 0, "bf16", max_batch=16).load_synthetic(0xF15E5EED)
    prompts = _prompts(16, a.prompt_len, fcfg.FISH_1_5_TOKENS["im_end_id"])
    budget = a.prompt_len + a.warmup + a.frames + 64
    _session_step_us(lm, prompts, budget, 16, a.warmup)  # (default settings: lm.session()'s own)
    rounds = [_session_step_us(lm, prompts, budget, a.frames, a.warmup) for _ in range(a.rounds)]
    lm.close()
    return dict(lib=a.lib or "in-tree", version=fishrt.lib().fs_version().decode(), slots=16, us_per_step=rounds, median_us=statistics.median(rounds))


def merge(a):
    out = json.load(open(a.merge))
    new, parent = [json.load(open(f)) for f in a.new], [json.load(open(f)) for f in a.parent]
    nm, pm = [r["median_us"] for r in new], [r["median_us"] for r in parent]
    spread = (max(pm) - min(pm)) / statistics.median(pm)
    delta = statistics.median(nm) / statistics.median(pm) - 1.0
    out["fish15_per_slot_step_16_slots"] = dict(new_runs_us=nm, parent_runs_us=pm, new_median_us=statistics.median(nm), parent_median_us=statistics.median(pm),
                                                parent_run_to_run_spread=spread, new_over_parent=delta,
                                                inside_parent_spread=bool(min(pm) <= statistics.median(nm) <= max(pm) or abs(delta) <= spread))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--slots", type=int, nargs="+", default=[4, 16, 32])
    ap.add_argument("--prompt-len", type=int, default=64)
    ap.add_argument("--frames", type=int, default=128, help="timed frames per round")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--fish15-step", action="store_true")
    ap.add_argument("--lib", help="libfishrt.so to measure with --fish15-step (default: the in-tree build)")
    ap.add_argument("--merge", metavar="LEGACY_JSON")
    ap.add_argument("--new", nargs="+", default=[])
    ap.add_argument("--parent", nargs="+", default=[])
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.merge and not (a.new and a.parent):
        ap.error("--merge needs --new and --parent runs")
    out = merge(a) if a.merge else (measure_fish15(a) if a.fish15_step else measure_legacy(a))
    text = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
