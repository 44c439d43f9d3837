"""Outputs of a fixed list of small synthetic cases that between them launch every attention instantiation the engine reaches (csrc/lm_attn.hip),
as .npy files -- for a byte-for-byte comparison of two builds (a refactor of the attention kernels must not move one bit):
    python tools/attn_paths_dump.py --out DIR                      # the in-tree build
    python tools/attn_paths_dump.py --lib /path/libfishrt.so --out DIR2   # another build (a parent commit); then: cmp every file of DIR and DIR2
One process per library.  Cases and the kernels they are meant to reach: CASES below.  Observed on an MI355X: the 28 files of the build
that moved the launchers' if / else ladders into AttnKernels::decode_plan / rows_plan and of its parent are cmp-equal, file by file.  Which
instantiation a call reaches is no longer this file's to claim: every launcher reports the plan it dispatched through, and
tests/test_attn_paths_gpu.py asserts that name for each of its cases and that the names reached are the whole table (attn_refs.PLAN_TABLE);
the list below is still the intent only, it has not been confirmed by a kernel trace of this tool."""
import argparse, os, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fish-speech.rs_amd")]
SEED = 0xF15E5EED
GREEDY = dict(temp=0.0, top_p=1.0, top_k=0, ignore_eos=True)

CASES = """tiny_f32   TINY f32: 200-token prompt in chunks [0,70,200], then 6 greedy per-node frames   k_attn_decode<float,32,2>
tiny_rows  TINY bf16: one pass of 129 rows                                                 k_attn_decode<bf16,32,2> on rows, k_attn_combine<32>
tiny_b5    TINY bf16: static batch B = 5, 6 frames                                         k_attn_rows<bf16,32,2>, k_attn_small_rows<32>
mid_257    MID bf16: one pass of 257 rows                                                  k_attn_prefill_mfma
mid_sched  MID bf16: schedule [0,130,131,140]                                              k_attn_prefill_mfma (cached prefix), k_attn_decode<bf16,64,2> + k_attn_combine<64> (1-row pass)
mid_b5     MID bf16: ragged static batch B = 5 (group prefill), 6 frames                   k_attn_prefill_mfma (group), k_attn_rows<bf16,64,2>, k_attn_small_rows<64>
fish_b1    Fish x 3 layers bf16: 4 per-node frames behind 300 and 1100 cached tokens       k_attn_decode<bf16,64,2> hsplit 4; k_attn_rows<bf16,64,2,true> super-chunks
fish_bB    Fish x 3 layers bf16: static batch B in {2,3,4,33,40}, 4 frames                 k_attn_rows<bf16,64,2> plain / remapped, <bf16,64,4> plain / remapped, k_attn_small_rows_tbl<64>
fish_f32   Fish x 3 layers f32: 4 per-node frames behind 1200 cached tokens                k_attn_decode<float,64,8>, k_wo's general merge"""


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
    args = ap.parse_args()
    from fishrt import _ffi
    if args.lib:
        _ffi.LIB_PATH = os.path.abspath(args.lib)
    import fishrt
    from fishrt import config as fcfg
    os.makedirs(args.out, exist_ok=True)
    print("lib:", _ffi.LIB_PATH, fishrt.lib().fs_version().decode())

    def save(name, a):
        np.save(os.path.join(args.out, name + ".npy"), np.ascontiguousarray(a))

    def passes(lm, name, p, cuts):
        lm.clear_slow_layer_caches()
        for i in range(len(cuts) - 1):
            lg, hd = lm.forward_generate(p[:, cuts[i]:cuts[i + 1]], cuts[i])
            save(f"{name}_logits{i}", lg); save(f"{name}_hidden{i}", hd)

    def batch(lm, name, prompts, frames):
        got = lm.generate_static_batch(prompts, max(p.shape[1] for p in prompts) + frames - 2, seed=42, **GREEDY)
        save(name + "_codes", np.stack(got))

    tiny = lambda L, s: prompt(L, s, 400, fcfg.TINY_TOKENS["semantic_start_id"], 64)
    fish = lambda L, s: prompt(L, s, 100000, fcfg.FISH_1_5_TOKENS["semantic_start_id"], 1024)
    # tests/test_lm_gpu.MID with room for the 257-row pass
    MID = dict(fcfg.TINY, dim=256, n_head=4, n_local_heads=2, head_dim=64, intermediate_size=1024, max_seq_len=512)
    FISH3 = dict(fcfg.FISH_1_5, n_layer=3)

    lm = fishrt.DualARTransformer(fcfg.TINY, fcfg.TINY_TOKENS, 0, "f32").load_synthetic(SEED)
    p = tiny(200, 1)
    passes(lm, "tiny_f32", p, [0, 70, 200])
    lm.clear_slow_layer_caches()
    save("tiny_f32_codes", lm.generate_blocking(p, 200 + 6 - 2, persistent=False, **GREEDY))
    lm.close()

    lm = fishrt.DualARTransformer(fcfg.TINY, fcfg.TINY_TOKENS, 0, "bf16", 8).load_synthetic(SEED)
    passes(lm, "tiny_rows", tiny(129, 2), [0, 129])
    batch(lm, "tiny_b5", [tiny(L, 10 + L) for L in (5, 11, 8, 3, 7)], 6)
    lm.close()

    lm = fishrt.DualARTransformer(MID, fcfg.TINY_TOKENS, 0, "bf16", 8).load_synthetic(SEED)
    passes(lm, "mid_257", tiny(257, 3), [0, 257])
    passes(lm, "mid_sched", tiny(140, 4), [0, 130, 131, 140])
    batch(lm, "mid_b5", [tiny(L, 20 + L) for L in (17, 9, 12, 3, 15)], 6)
    lm.close()

    lm = fishrt.DualARTransformer(FISH3, fcfg.FISH_1_5_TOKENS, 0, "bf16").load_synthetic(SEED)
    for T in (300, 1100):
        lm.clear_slow_layer_caches()
        codes, hid = lm.generate_blocking_with_hidden(fish(T, T), T + 4 - 2, persistent=False, **GREEDY)
        save(f"fish_b1_T{T}_codes", codes); save(f"fish_b1_T{T}_hidden", hid)
    lm.close()
    lm = fishrt.DualARTransformer(FISH3, fcfg.FISH_1_5_TOKENS, 0, "bf16", 40).load_synthetic(SEED)
    for B in (2, 3, 4, 33, 40):
        batch(lm, f"fish_b{B}", [fish(3 + (7 * i) % 11, 100 * B + i) for i in range(B)], 4)
    lm.close()

    lm = fishrt.DualARTransformer(FISH3, fcfg.FISH_1_5_TOKENS, 0, "f32").load_synthetic(SEED)
    codes, hid = lm.generate_blocking_with_hidden(fish(1200, 5), 1200 + 4 - 2, persistent=False, **GREEDY)
    save("fish_f32_codes", codes); save("fish_f32_hidden", hid)
    lm.close()
    print("wrote", len(os.listdir(args.out)), "files to", args.out)


if __name__ == "__main__":
    main()
