"""Outputs of a fixed list of small synthetic cases that between them launch the GEMM kernels of the MFMA row path (csrc/lm_gemm.hip) that the
engine reaches at TINY, MID and Fish-1.5 widths,
as .npy files (logits, hidden states, codes, cached K / V rows) -- for a byte-for-byte comparison of two builds (a refactor of the row-path
GEMMs must not move one bit):
    python tools/rows_paths_dump.py --out DIR                      # the in-tree build
    python tools/rows_paths_dump.py --lib /path/libfishrt.so --out DIR2   # another build (a parent commit); then: cmp every file of DIR and DIR2
One process per library; the FISHRT_ROWS_NO_FOLD=1 cases run first, in a child process of their own (the switch is read once per process), which
has ended before this process opens the GPU.  --cases runs a subset.  Cases and the row-path kernels each launches: CASES below."""
import argparse, os, subprocess, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fish-speech.rs_amd")]
SEED = 0xF15E5EED
GREEDY = dict(temp=0.0, top_p=1.0, top_k=0, ignore_eos=True)

CASES = """tiny_pf     TINY bf16: passes of 1, 17, 33, 129 rows (the 1-row pass takes the batch-1 kernels)    k_embed_rows, k_prep; k_gemm3 NKS 1 full panels: QKV, RESIDUAL_NORM, SWIGLU_RMS (RT 2); STORE NKS 2 (W2 slabs)
mid_pf      MID bf16: the same passes                                           the same at NKS 2; STORE NKS 8 (W2 as one 1024-deep range)
fish_pf129  Fish x 3 layers {bf16, fp8}: one pass of 129 rows                   k_gemm_big<SWIGLU_RMS>, k_gemm_big<STORE> (W13, W2); k_gemm3<QKV / RESIDUAL_NORM, NKS 8> for Wqkv, Wo
fish_pf513  ... 513 rows (one pass of 512, then a batch-1 step)                 k_gemm_big<QKV>, k_gemm_big<RESIDUAL_NORM> too: no k_gemm3
fish_b5     ... static batch B = 5, 3 frames                                    group prefill (plain QKV with seq_rows, full panels, STORE slabs); fold step on HALF panels: k_gemm3<QKV / QKV_RMS / STORE_RMS / RESIDUAL_NORM / SWIGLU_RMS, HALF>, k_gemm_down<8>
fish_b17    ... B = 17                                                          group prefill on k_gemm_big<SWIGLU_RMS / STORE>; the fold step on full panels
fish_b32    ... B = 32                                                          the same at the panel limit
fish_b40    ... B = 40                                                          > 32 rows: k_gemm3<QKV / RESIDUAL_NORM / SWIGLU_RMS / STORE> + k_prep every layer, two panels
fish_b32_nofold   B = 32 with FISHRT_ROWS_NO_FOLD=1 (child process)             the kernels of fish_b40 at one full panel
fish_sess   ... 4-slot session, prompts of 9 / 1 / 40 / 17 tokens queued together   one plain group pass; pos_step < 0 (every row at its own position) through the HALF fold step
fish_pfx    ... 6-slot session: members on shared prefixes, starts 0 / 37 / 70 / 70 in one group pass, then 37 / 70 in a 10-row one   k_gemm3<QKV_SEQ, NKS 8> full and HALF; tail-page copies; the HALF fold step
mid_pfx     MID {bf16, fp8}: the same                                           k_gemm3<QKV_SEQ, NKS 2> full and HALF, k_gemm_down<2>
mid_b       MID {bf16, fp8}: static batches B = 5 and 17, 3 frames              the fold step at NKS 2, HALF and full: QKV_RMS, STORE_RMS, RESIDUAL_NORM, SWIGLU_RMS, k_gemm_down<2>
small_nofold  Fish B = 5, MID B = 5 and 17 with FISHRT_ROWS_NO_FOLD=1 (child)   k_gemm3<STORE, NKS 2 and 8> HALF and full, with QKV / RESIDUAL_NORM / SWIGLU_RMS beside them"""
# Kernel lists: rocprofv3 --kernel-trace --stats of every case on an MI355X.  Together: 59 k_gemm3 (every NKS 2 and NKS 8 instantiation of the
# seven epilogues above, bf16 / fp8, full / HALF; NKS 1 for QKV, RESIDUAL_NORM, SWIGLU_RMS), 8 k_gemm_big, 4 k_gemm_down.  Not launched: the
# un-fused EPI_RESIDUAL / EPI_SWIGLU (the engine's row contexts always carry A2 / ss), the other NKS 1 kernels and k_gemm_down<1> (TINY static
# batches), k_gemm_big with QKV_RMS / STORE_RMS / QKV_SEQ (fold steps and group passes of >= 128 rows).

CASE_NAMES = [l.split()[0] for l in CASES.splitlines()]


def prompt(L, seed, text_ids, sem_start, cb_size):
    """a random text row plus a few VQ columns (the codebook embeddings are summed there)"""
    rng = np.random.RandomState(seed)
    p = np.zeros((9, L), np.uint32)
    p[0] = rng.randint(0, text_ids, L)
    for c in sorted(set([0, L - 1] + [int(c) for c in rng.randint(0, L, 1 + L // 8)])):
        codes = rng.randint(0, cb_size, 8)
        p[0, c] = sem_start + codes[0]
        p[1:, c] = codes
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", help="libfishrt.so to run (default: the in-tree build)")
    ap.add_argument("--out", required=True)
    ap.add_argument("--cases", help="comma-separated subset of the case names (default: all)")
    ap.add_argument("--nofold-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    want = args.cases.split(",") if args.cases else list(CASE_NAMES)
    unknown = set(want) - set(CASE_NAMES)
    if unknown:
        ap.error(f"unknown cases {sorted(unknown)} (known: {', '.join(CASE_NAMES)})")
    NOFOLD = ("fish_b32_nofold", "small_nofold")
    if set(NOFOLD) & set(want) and not args.nofold_child:  # before this process touches the GPU
        cmd = [sys.executable, os.path.abspath(__file__), "--out", args.out, "--nofold-child", "--cases", ",".join(c for c in want if c in NOFOLD)]
        cmd += ["--lib", args.lib] if args.lib else []
        subprocess.run(cmd, env=dict(os.environ, FISHRT_ROWS_NO_FOLD="1"), check=True, timeout=600)
    from fishrt import _ffi
    if args.lib:
        _ffi.LIB_PATH = os.path.abspath(args.lib)
    import fishrt
    from fishrt import config as fcfg
    print("lib:", _ffi.LIB_PATH, fishrt.lib().fs_version().decode(), "(FISHRT_ROWS_NO_FOLD=1)" if args.nofold_child else "", flush=True)

    def save(name, a):
        np.save(os.path.join(args.out, name + ".npy"), np.ascontiguousarray(a))

    def save_kv(lm, name, n, slots=(0,)):
        for b in slots:
            for l in range(lm.cfg["n_layer"]):
                k, v = lm.debug_read_kv(l, 0, n, slot=b)
                save(f"{name}_s{b}_l{l}_k", k); save(f"{name}_s{b}_l{l}_v", v)

    def passes(lm, name, p, cuts):
        lm.clear_slow_layer_caches()
        for i in range(len(cuts) - 1):
            lg, hd = lm.forward_generate(p[:, cuts[i]:cuts[i + 1]], cuts[i])
            save(f"{name}_logits{i}", lg); save(f"{name}_hidden{i}", hd)
        save_kv(lm, name, cuts[-1])

    def batch(lm, name, prompts, frames):
        Lmax = max(p.shape[1] for p in prompts)
        got = lm.generate_static_batch(prompts, Lmax + frames - 2, seed=42, **GREEDY)
        save(name + "_codes", np.stack(got))
        save_kv(lm, name, Lmax + frames - 2, slots=(0, len(prompts) - 1))

    def drain(s, name, slots):
        while s.step(3):
            pass
        for i, slot in enumerate(slots):
            save(f"{name}_codes{i}", s.poll(slot)[0])

    def prefixed(lm, name, mk):
        """members that start at 0 / 37 / 70 / 70 queued together: ONE group pass with per-sequence positions"""
        pre = {P: mk(P, 900 + P) for P in (37, 70)}
        members = [(None, 12), (37, 9), (70, 20), (70, 5)]
        late = [(37, 4), (70, 6)]  # a second group pass of 2 x 5 rows: the M <= 16 half-panel kernels
        with lm.session(seed=42, **GREEDY) as s:
            ids = {P: s.add_prefix(p) for P, p in pre.items()}
            s.step(1)  # nothing live: the prefixes' own pass runs and is activated
            before = s.info()
            slots = [s.add(mk(Lb, 950 + i), (P or 0) + Lb + 4, prefix=None if P is None else ids[P]) for i, (P, Lb) in enumerate(members)]
            s.step(1)
            after = s.info()
            save(name + "_info", np.array([after[k] - before[k] for k in ("prefill_passes", "tokens_prefilled", "prefix_tokens_reused", "tail_pages_copied")]))
            for slot, (P, Lb) in zip(slots, members):
                for l in range(lm.cfg["n_layer"]):
                    k, v = lm.debug_read_kv(l, 0, (P or 0) + Lb - 1, slot=slot)
                    save(f"{name}_s{slot}_l{l}_k", k); save(f"{name}_s{slot}_l{l}_v", v)
            before = s.info()
            slots += [s.add(mk(Lb, 970 + i), P + Lb + 4, prefix=ids[P]) for i, (P, Lb) in enumerate(late)]
            s.step(1)
            save(name + "_info2", np.array([s.info()[k] - before[k] for k in ("prefill_passes", "tokens_prefilled")]))
            drain(s, name, slots)

    tiny = lambda L, s: prompt(L, s, 400, fcfg.TINY_TOKENS["semantic_start_id"], 64)
    fish = lambda L, s: prompt(L, s, 100000, fcfg.FISH_1_5_TOKENS["semantic_start_id"], 1024)
    fish_batch = lambda B: [fish(3 + (7 * i) % 11, 100 * B + i) for i in range(B)]
    MID = dict(fcfg.TINY, dim=256, n_head=4, n_local_heads=2, head_dim=64, intermediate_size=1024, max_seq_len=512)
    FISH3 = dict(fcfg.FISH_1_5, n_layer=3)
    fish_lm = lambda dt, B: fishrt.DualARTransformer(FISH3, fcfg.FISH_1_5_TOKENS, 0, dt, B).load_synthetic(SEED)

    mid_lm = lambda dt, B: fishrt.DualARTransformer(MID, fcfg.TINY_TOKENS, 0, dt, B).load_synthetic(SEED)
    mid_batch = lambda B: [tiny(3 + (5 * i) % 17, 20 * B + i) for i in range(B)]
    if args.nofold_child:
        for dt in ("bf16", "fp8"):
            if "fish_b32_nofold" in want:
                lm = fish_lm(dt, 32)
                batch(lm, f"fish_{dt}_b32_nofold", fish_batch(32), 3)
                lm.close()
            if "small_nofold" in want:
                lm = fish_lm(dt, 5)
                batch(lm, f"fish_{dt}_b5_nofold", fish_batch(5), 3)
                lm.close()
                lm = mid_lm(dt, 17)
                for B in (5, 17):
                    lm.clear_slow_layer_caches()
                    batch(lm, f"mid_{dt}_b{B}_nofold", mid_batch(B), 3)
                lm.close()
        return

    for name, cfg in (("tiny", fcfg.TINY), ("mid", MID)):
        if name + "_pf" in want:
            lm = fishrt.DualARTransformer(cfg, fcfg.TINY_TOKENS, 0, "bf16").load_synthetic(SEED)
            passes(lm, name + "_pf", tiny(180, 2), [0, 1, 18, 51, 180])
            lm.close()
    for dt in ("bf16", "fp8"):
        if "mid_b" in want:
            lm = mid_lm(dt, 17)
            for B in (5, 17):
                lm.clear_slow_layer_caches()
                batch(lm, f"mid_{dt}_b{B}", mid_batch(B), 3)
            lm.close()
        if "mid_pfx" in want:
            lm = mid_lm(dt, 6)
            prefixed(lm, f"mid_{dt}_pfx", tiny)
            lm.close()
    for dt in ("bf16", "fp8"):
        if {"fish_pf129", "fish_pf513", "fish_b5", "fish_b17", "fish_b32", "fish_b40"} & set(want):
            lm = fish_lm(dt, 40)
            if "fish_pf129" in want: passes(lm, f"fish_{dt}_pf129", fish(129, 3), [0, 129])
            if "fish_pf513" in want: passes(lm, f"fish_{dt}_pf513", fish(513, 4), [0, 513])
            for B in (5, 17, 32, 40):
                if f"fish_b{B}" in want:
                    lm.clear_slow_layer_caches()
                    batch(lm, f"fish_{dt}_b{B}", fish_batch(B), 3)
            lm.close()
        if "fish_sess" in want:
            lm = fish_lm(dt, 4)
            with lm.session(seed=42, **GREEDY) as s:
                drain(s, f"fish_{dt}_sess", [s.add(fish(L, 50 + L), L + 6) for L in (9, 1, 40, 17)])
            lm.close()
        if "fish_pfx" in want:
            lm = fish_lm(dt, 6)
            prefixed(lm, f"fish_{dt}_pfx", fish)
            lm.close()
    print("wrote", len(os.listdir(args.out)), "files to", args.out)


if __name__ == "__main__":
    main()
