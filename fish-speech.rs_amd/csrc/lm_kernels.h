// Launch interface of the dual-AR decode kernels (lm_kernels.hip), the MFMA row-path GEMMs (lm_gemm.hip), the attention kernels
// (lm_attn.hip) and the on-device samplers (lm_sample.hip).  gfx950 only.
//
// Data layout in HBM:
//  * weights: row-major [out, in] in WT (bf16, f32, or OCP e4m3fn bytes + one f32 scale per row), one 256-B aligned slab
//    per tensor; with fp8 weights the embedding tables and the KV cache stay bf16 (KVT<WT>); W1/W3 are stored
//    row-interleaved (row 2r = w1[r], row 2r+1 = w3[r]) so one wave streams a contiguous 2-row block and applies
//    SwiGLU in registers;
//  * KV cache: paged.  One pool per layer; page = 64 tokens; K element (t, g, d) lives at
//        pool_k + ((page_table[t >> 6] * Hk + g) * 64 + (t & 63)) * Dh + d
//    so that one wave-wide 16-B/lane load covers 8 (bf16) consecutive tokens of ONE kv head (1 KiB contiguous);
//  * activations: f32 vectors (residual stream x[dim], q[H*Dh], act[inter], logits) -- a few KB, L2-resident.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "fs_common.h"
#include "fs_slot_book.h"

struct fs_attn_case;
struct fs_gemm_case;
struct fs_gemm_out;
struct fs_gemv_case;
struct fs_gemv_out;
struct fs_sample_case;
struct fs_sample_out;

namespace fs {

// storage type of the KV cache and the embedding tables for a given weight type (fp8 weights keep bf16 KV / embeddings)
template <typename WT> struct KVOf { using type = WT; };
template <> struct KVOf<fp8_t> { using type = bf16_t; };
template <typename WT> using KVT = typename KVOf<WT>::type;

constexpr int KV_PAGE = 64;  // tokens per KV page

// Per-sequence device-resident generation state (read by the captured graph; never passed by value).
struct SeqState {
    int pos;        // current KV length T == index where the next token's K/V is written
    int rope_off;   // RoPE row = pos + rope_off (forward_generate's input_pos may differ from the KV length)
    int frame;      // decode iterations executed in this generate call
    int done;       // <|im_end|> sampled (audio_only termination, single_batch.rs:199-204)
    int n_out;      // frames recorded in out_codes
    int have_prev;  // previous_codes.is_some() (single_batch.rs:162-168)
    int step;       // prompt column consumed by the next prefill step
    int prompt_L;   // row stride of the staged prompt (tokens per row)
    uint32_t cur[16];   // [slow, c0..c7] of the frame being generated
    uint32_t prev[16];  // previous frame (rep-pen key)
};

struct KVView {
    void* k;                // pool base for this layer
    void* v;
    const int* page_table;  // [max_pages] for this sequence
};

struct LayerW {
    const void* wqkv;  // [(H+2Hk)*Dh, dim]
    const void* wo;    // [dim, dim]
    const void* w13;   // [2*inter, dim] row-interleaved
    const void* w2;    // [dim, inter]
    const float* attn_norm;
    const float* ffn_norm;
    // fp8 (e4m3fn) weights only: one f32 dequantisation scale per output row of each matrix (null otherwise)
    const float* s_qkv = nullptr;
    const float* s_o = nullptr;
    const float* s_13 = nullptr;  // interleaved like w13
    const float* s_2 = nullptr;
    // false: weights are streamed once per frame -> non-temporal loads (slow transformer, 717 MB / frame);
    // true: re-read 8x per frame and small enough for the 256 MB Infinity Cache (fast decoder, 122 MB) -> default policy
    bool cache_resident = false;
};

struct ModelDims {
    int dim, inter, H, Hk, Dh, n_rep;
    float eps;
};

struct SampleCfg;
size_t rows_xchg_bytes(int dim);

// Buffers + row mapping of the MFMA row path (prefill / batched decode).  All activation buffers hold Mcap rows (a multiple
// of 32: the GEMMs read whole 32-row panels, so rows >= M must exist and hold finite values).
struct RowsCtx {
    int Mcap;            // row capacity of every buffer below (except `part`)
    int part_rows;       // row capacity of `part` (chunked attention: static-batch steps, head_dim != 64 prefill passes)
    int down_split;      // K ranges (== slabs) of the down projection: inter / down_split must be 1024, 256 or 128
    float* X;            // [Mcap][dim]   residual stream (f32)
    float* Q;            // [Mcap][dim]   rope'd queries (f32)
    float* part;         // [part_rows][H][n_chunks_max][Dh + 2] attention partials
    float* P;            // [down_split][Mcap][dim] down-projection split-K slabs
    uint16_t* A;         // [Mcap][dim]   bf16 hi+lo GEMM input (normed x / attention output), fragment-major (lm_dev.h frag_off)
    uint16_t* C;         // [Mcap][inter] bf16 hi+lo SwiGLU activations, fragment-major
    uint16_t* A2 = nullptr;  // [Mcap][dim] second GEMM-input buffer: with `ss` set, the ffn RMSNorm is folded into the Wo / W13 GEMMs
    float* ss = nullptr;     // [Mcap][dim / 16] sum-of-squares partials of the Wo GEMM's blocks
    const float *cos_t, *sin_t;
    const SeqState* state;  // position source (row m sits at state->pos + m * pos_step)
    int n_chunks_max;    // stride of `part`
    int nc_launch;       // attention chunks launched (covers the longest row of this pass)
    int pos_step;        // 1: rows = consecutive tokens of one sequence (prefill); 0: rows = sequences (batched decode)
    int pt_stride;       // page-table stride between rows (0 for prefill) / between sequences (group prefill)
    int seq_rows = 0;    // > 0: group prefill -- rows = seq_rows consecutive tokens of each of M / seq_rows sequences, all starting at state->pos
    const SeqState* seq_states = nullptr;  // group prefill, device [M / seq_rows]: sequence s starts at seq_states[s].pos (null: all at state->pos)
    bool no_flash = false;       // micro-benchmark / test hook: keep the chunked row attention for prefill passes
    bool chunked_attn = false;   // micro-benchmark / test hook: keep k_attn_decode + k_attn_combine for rows-are-sequences passes
    bool small_attn = false;     // every row attends over <= 8 tokens of ONE page (fast decoder): fused attention node
    void* xchg = nullptr;        // fold: exchange units of the layer-closing down projection (rows_xchg_bytes(dim), zero-initialised, used by nothing else)
    uint32_t* epoch = nullptr;   // fold: [0] = step epoch (>= 1; bumped once per step by the slow-token sampler node), [1] = exchange timeouts
    uint32_t node_id = 0;        // fold: unique per rows_layer call of a step (< 4096)
    bool attn_t1 = false;        // fold + small_attn: every row sits at position 0 of an empty cache (first codebook pass): no attention node
    bool identity_pages = false; // small_attn: page_table[m * pt_stride] == m for every row (the batched fast decoder's one-page-per-row table)
    bool first_prepped = false;  // fold: the first layer's normalised input fragments are already in A (written by the sampler that produced the row)
    bool fold = false;           // decode step with the un-split down projection (see rows_layer's next_norm)
    const float* qkv0_tbl = nullptr;         // fold + small_attn, first layer of a codebook pass >= 1: [codebook_size][(H + 2 Hk) Dh] f32 qkv table (lm_persist.hip) -- no Wqkv node
    const SeqState* row_states = nullptr;    // ... the rows' generator states: row m's previous code = row_states[m].cur[code_slot]
    int code_slot = 0;
    unsigned stage_mask = 0xFFu;  // micro-benchmark hook: bit i enables stage i of rows_layer (prep, qkv, attn, combine, wo, prep, w13, w2)
};

// ---- launchers (all asynchronous on `st`) -------------------------------------------------------------------
template <typename WT>
struct LmKernels {
    // x -> rmsnorm -> Wqkv GEMV -> interleaved RoPE(q,k) -> q_out (f32), K/V appended at state->pos (or pos_static)
    // (state != null: KV index = state->pos, RoPE row = state->pos + state->rope_off; else the two static values)
    static void qkv(const ModelDims& d, const float* x, const LayerW& w, const float* cos_t, const float* sin_t,
                    const SeqState* state, int pos_static, int rope_static, float* q_out, KVView kv, hipStream_t st);
    // combine the chunks of state->pos + 1 tokens (or, fused_T > 0: attend over fused_T <= 8 cached tokens in the
    // prologue) -> Wo GEMV -> x += .
    // nc_launch = the chunk count AttnKernels::decode was launched with (ignored when fused_T > 0)
    static void wo(const ModelDims& d, const float* part, int n_chunks_max, int nc_launch, const SeqState* state, const float* q,
                   KVView kv, int fused_T, const LayerW& w, float* x, hipStream_t st);
    static void ffn_up(const ModelDims& d, const float* x, const LayerW& w, float* act, hipStream_t st);
    static void ffn_down(const ModelDims& d, const float* act, const LayerW& w, float* x, hipStream_t st);
    // x -> rmsnorm(norm_w) -> rows [0, n_rows) of W (x wscale[row] for fp8 weights) -> logits f32
    static void head(const ModelDims& d, const float* x, const float* norm_w, const void* W, const float* wscale, int n_rows,
                     float* logits, hipStream_t st);
    // x = tok_emb[t0] + sum_c mask * cb_emb[c*cbsize + t_{c+1}]   (dual_ar.rs:532-567); tokens from prompt column
    // state->step (prompt != null) or from state->cur
    static void embed(const ModelDims& d, const void* tok_emb, const void* cb_emb, int n_cb, int cb_size,
                      const SampleCfg* cfg, const uint32_t* prompt, SeqState* state, float* x, hipStream_t st);
    // fast_embeddings gather: out[i] = fast_emb[ids[i]]
    static void fast_embed(const ModelDims& d, const void* fast_emb, const uint32_t* ids, int n, float* out,
                           hipStream_t st);
};

// What a batch-1 GEMV launcher of LmKernels will launch for a given call: decided in ONE place (gemv_plan, lm_kernels.hip), the five launchers
// dispatch through it, and fs_selftest_gemv reports its name ("qkv/bf16/K1024/w2/nt", "wo/bf16/K1024/w4/dh64/nt", "up/f32/K256/w4/res",
// "down/fp8/K4096/ks4/res", "head/f32/K128/w4").  nt / res: non-temporal or default weight loads (LayerW::cache_resident); k_head has one policy.
struct GemvPlan {
    enum Op { QKV, WO, FFN_UP, FFN_DOWN, HEAD };
    Op op = QKV;
    int wt = 1;            // 0 f32, 1 bf16, 2 fp8 (FS_GEMV_WT_*)
    int K = 0;             // GEMV width of the instantiation (dim; FFN_DOWN: inter)
    int waves = 0;         // waves == weight rows (FFN_UP: row pairs) per block; FFN_DOWN: the KS waves that share one row
    bool nt = true;        // non-temporal weight loads (!cache_resident)
    bool fused = false;    // WO: the fused small attention prologue (fused_T > 0)
    int DH = 0;            // WO: head_dim of the instantiation
    unsigned gx = 1, block = 64;
    std::string name() const;
};
// host only; throws what the launcher would throw (unsupported width, unsupported wo geometry).  n_rows: output rows (FFN_UP: inter)
GemvPlan gemv_plan(int op, int wt, const ModelDims& d, int n_rows, bool cache_resident, int fused_T = 0);

// ---- MFMA row path (lm_gemm.hip; prefill passes, static-batch steps): bf16 weights, or fp8 weights widened to bf16 in registers
template <typename WT>
struct RowKernels {
    static bool has_mfma_prefill();
    // X[m] = embed(prompt column state->step + m), m < M
    static void prefill_embed(const ModelDims& d, const void* tok_emb, const void* cb_emb, int n_cb, int cb_size,
                              const SampleCfg* cfg, const uint32_t* prompt, const SeqState* state, int M, float* X,
                              hipStream_t st, int seq_rows = 0, size_t prompt_stride = 0);
    // one transformer block over M <= Mcap activation rows (X updated in place up to the down-projection, whose split-K
    // slabs are folded in by the NEXT rows_layer / rows_finish):
    //   x += slabs | rmsnorm+Wqkv+rope+KV append | attention over the paged cache | Wo + residual | rmsnorm+W13+SwiGLU | W2 slabs
    // c.fold (decode steps of <= 32 rows, rows_fold_ok): next_norm = the norm weight of whoever consumes this layer's output (the next
    // layer's attention_norm, or the final norm in front of the head) -- the down projection runs un-split and closes the layer itself
    // (no slabs, no k_prep node; rows_finish is then not called and rows_head takes rms = true)
    static void rows_layer(const ModelDims& d, int M, const RowsCtx& c, const LayerW& w, KVView kv, bool first, hipStream_t st,
                           const float* next_norm = nullptr);
    static bool rows_fold_ok(const ModelDims& d, int M, const RowsCtx& c);
    static void rows_finish(const ModelDims& d, int M, const RowsCtx& c, const float* norm_w, hipStream_t st);
    static void rows_head(const ModelDims& d, int M, const RowsCtx& c, const void* W, const float* wscale, int n_rows, float* logits, int ld,
                          hipStream_t st, bool rms = false);
};

// What a row-path GEMM launcher will launch for a given call: decided in ONE place (gemm_plan, lm_gemm.hip), launch_gemm3 and
// launch_gemm_down dispatch through it, and fs_selftest_gemm reports its name ("gemm3/QKV_RMS/nks8/rt1/bf16/half", "big/SWIGLU_RMS/fp8",
// "down/nks8/ks4/bf16").  The name is the kernel instantiation; ksplit of a GEMM3 / BIG launch is a grid dimension, not part of it.
struct GemmPlan {
    enum Kind { GEMM3, BIG, DOWN };
    Kind kind = GEMM3;
    int epi = 0;           // EPI_* of the instantiation (DOWN: its own epilogue, GEMM_EPI_DOWN)
    int nks = 0;           // 32-deep k-steps per wave (BIG: 16)
    int rt = 1;            // 16-row weight tiles per wave (GEMM3)
    bool fp8 = false;
    bool half = false;     // GEMM3, M <= 16: rows 16..31 of the only panel are skipped
    int ksplit = 1;        // K ranges == gridDim.y
    unsigned gx = 1, gy = 1, gz = 1;
    std::string name() const;
};
constexpr int GEMM_EPI_DOWN = 9;  // not a k_gemm3 epilogue: selects launch_gemm_down's plan (ksplit and nks follow from K)
// big_min_m: 0 = FISHRT_GEMM_BIG_MIN_M / the built-in row count from which the LDS-staged variant is taken
GemmPlan gemm_plan(int epi, int rt, int M, int N, int K, int ksplit, bool fp8, int big_min_m = 0);

// ---- attention launchers (lm_attn.hip; all asynchronous on `st`)
// What an attention launcher will launch for a given call: decided in ONE place (AttnKernels::decode_plan / rows_plan), the launchers
// dispatch through it, and fs_selftest_attn reports its name ("decode/bf16/64/2/hs4", "rows/bf16/64/4/hs2/remap", "small/64/ident", ...)
struct AttnPlan {
    enum Kind { DECODE, DECODE_PART, ROWS, ROWS_CHUNKED, SMALL, SMALL_TBL, PREFILL_MFMA };
    Kind kind = DECODE;
    bool f32_kv = false;   // KV type of the instantiation (f32 weights only)
    int DH = 0;            // head_dim of the instantiation
    int nrep = 0;          // query heads per block (template NREP; n_rep of the model for the kernels without it)
    int hsplit = 1;        // blocks the query heads of one kv group are spread over
    int tpb = 1;           // DECODE_PART: chunks per super-chunk block
    bool remap = false;    // ROWS, hsplit > 1: k_attn_rows' XCD placement condition per_xcd * 8 * hsplit == total holds for this grid
    bool group = false;    // PREFILL_MFMA: group pass (RowsCtx::seq_rows > 0)
    bool ident = false;    // SMALL / SMALL_TBL: identity page table
    unsigned gx = 1, gy = 1, gz = 1;  // grid
    std::string name() const;
};

template <typename WT>
struct AttnKernels {
    // the kernel AttnKernels::decode / rows launch for these arguments (host only; throws what the launcher would throw)
    static AttnPlan decode_plan(const ModelDims& d, int nc_launch);
    static AttnPlan rows_plan(const ModelDims& d, int M, const RowsCtx& c, bool tbl0);
    // tokens per attention chunk: chunk c covers tokens [c * chunk(), (c + 1) * chunk())
    static int chunk();
    // batch-1 decode over more than 8 chunks: attention blocks take this many consecutive chunks each so that k_wo merges 8 partials
    // (1: one chunk per block; FISHRT_ATTN_SUPERCHUNK=0 disables: tuning / test hook)
    static int tiles_per_block(const ModelDims& d, int nc_launch);
    // decode attention over the paged cache: un-normalised partial {o[Dh], m, l} per (q head, token chunk); part: [H][n_chunks_max][Dh + 2]
    // nc_launch: chunks actually launched (>= ceil(T / chunk()) for every T the launch will see; the host knows
    // the position of every frame, so graphs are captured per power-of-two bucket of nc_launch)
    static void decode(const ModelDims& d, const float* q, KVView kv, const SeqState* state, float* part, int n_chunks_max, int nc_launch,
                       hipStream_t st);
    // attention step of RowKernels::rows_layer over M activation rows: c.Q (or, tbl0, row code of c.qkv0_tbl) against each row's KV prefix ->
    // hi/lo fragments in c.A.  tbl0 is rows_layer's decision (it also drops the layer's k_prep and Wqkv nodes)
    static void rows(const ModelDims& d, int M, const RowsCtx& c, KVView kv, bool tbl0, hipStream_t st);
    // may the first layer of a pass with this context take q / k / v from a qkv table (RowsCtx::qkv0_tbl)?  The engine asks before it sets the
    // table and withholds the sampler's first_prepped fragments; rows_layer asks again before it drops the k_prep and Wqkv nodes
    static bool rows_qkv0_ok(const ModelDims& d, const RowsCtx& c);
};

struct SampleCfg {  // device-resident (the captured graphs read it through a pointer, so one graph serves every config)
    float temp, top_p;
    int top_k;
    float rep_pen;
    int ignore_eos;
    uint32_t im_end_id;
    uint32_t sem_lo, sem_hi;  // embed mask range (inclusive); Fish<=1.4: lo == hi == semantic id
    // slow-token candidates (constrain_probs_to_audio / rescale_semantic_tokens, generate/utils.rs:6-56): candidate 0 = <|im_end|>,
    // candidate i >= 1 = token audio_base + i, audio_base = semantic_start_id - 1.  Fish 1.5: audio_base == im_end_id (the adjacent
    // layout, one contiguous slice of the head); generic DualAR layout: the head image is [W[im_end]; W[semantic_start .. V)].
    uint32_t audio_base = 0;
    // Fish <= 1.4 slow token (single_batch.rs:104-124, sampling/mod.rs:8-26): 2-way softmax over {pad_id, im_end_id},
    // temperature ignored; logits[0] = pad logit, logits[1] = im_end logit
    int legacy;
    uint32_t pad_id;
    // batch_rows > 0: BatchedLogitsProcessor semantics on the single-sequence samplers (row batch_row of a static batch generated on its
    // own, lm_engine.hip generate_batch_sequential): temp <= 1e-7 -> FIRST-max argmax; temp > 0 -> child StdRng of (call, row)
    int batch_rows = 0, batch_row = 0, batch_calls = 0;  // batch_calls = sample() calls per frame (num_codebooks + 1)
    // continuous batching (fs_lm_session_*): the rows of the static-batch step are independent request slots -- a finished or empty slot
    // stops stepping (position, frame counter and outputs frozen) instead of following the live rows in lock-step
    int session = 0;
    // BatchedLogitsProcessor compares top_p (f64) with `sum_p as f64` (sampling/mod.rs:68); the single-sequence LogitsProcessor narrows
    // top_p to f32 first.  The batched samplers (k_sample_*_rows, batch_rows > 0) use this field for that one comparison.
    double top_p64 = 0.0;
};

__host__ __device__ inline uint32_t audio_tok(const SampleCfg& c, int idx) { return idx > 0 ? c.audio_base + (uint32_t)idx : c.im_end_id; }

struct RepPenState {   // rep_pen.rs:4-72, one per codebook
    float* mask;       // [n_cb][cb_size]
    uint8_t* seen;     // [n_cb][cb_size]
    int* ring;         // [n_cb][17]  (push_front / pop_back deque as a ring)
    int* ring_meta;    // [n_cb][2] head, len
};

struct RngState {      // rand 0.8.5 StdRng (ChaCha12) stream position
    uint32_t key[8];
    unsigned long long consumed;  // u32 words consumed so far
};
// rand_core SeedableRng::seed_from_u64 (PCG32 expansion) -> ChaCha key
__host__ __device__ inline void seed_from_u64(unsigned long long state, uint32_t* key8) {
    for (int i = 0; i < 8; ++i) {
        state = state * 6364136223846793005ull + 11634580027462260723ull;
        const uint32_t xorshifted = (uint32_t)(((state >> 18) ^ state) >> 27);
        const uint32_t rot = (uint32_t)(state >> 59);
        key8[i] = (xorshifted >> rot) | (xorshifted << ((32 - rot) & 31));
    }
}

struct SlotRng {       // per-slot sampler stream of a FS_SESSION_PER_SLOT session (k_sample_*_slots)
    RngState rng;
    // look-ahead cells, one per decision of a frame (0 slow, 1 + codebook): ahead_word[d] = the stream's word at position ahead_at[d],
    // derived by a spare wave of the previous decision's launch; ~0 = none (reset when the slot is activated)
    unsigned long long ahead_at[16];
    uint32_t ahead_word[16];
};

// ---- sampler setup on the host, shared by the engine (lm_engine.hip) and the sampler-node test hook (sample_frames_selftest): the
// SampleCfg of a token layout and of one request's settings, a request's StdRng stream, a freshly activated slot's stream
struct TokenLayout { uint32_t im_end_id, pad_id, semantic_start_id, semantic_end_id; bool has_semantic_end; };
inline SampleCfg sample_cfg_base(const TokenLayout& t) {
    const bool legacy = !t.has_semantic_end;  // Fish <= 1.4: slow token is a 2-way {pad, im_end} draw (single_batch.rs:104-124)
    SampleCfg c = {};
    c.temp = 0.f; c.top_p = 1.f; c.top_k = 0; c.rep_pen = 1.f; c.ignore_eos = 0;
    c.im_end_id = t.im_end_id;
    c.audio_base = legacy ? t.im_end_id : t.semantic_start_id - 1;
    c.sem_lo = t.semantic_start_id;
    c.sem_hi = t.has_semantic_end ? t.semantic_end_id : t.semantic_start_id;  // dual_ar.rs:554-559
    c.legacy = legacy ? 1 : 0;
    c.pad_id = t.pad_id;
    return c;
}
inline int clamp_top_k(uint64_t top_k) { return (int)(top_k < (1u << 30) ? top_k : (1u << 30)); }
// sample_cfg_base + one request's sampler settings; the callers set what differs (rep_pen = 1 in the batch paths, session, batch_*)
inline SampleCfg sample_cfg_make(const TokenLayout& t, double temp, double top_p, uint64_t top_k, float rep_pen, bool ignore_eos) {
    SampleCfg c = sample_cfg_base(t);
    c.temp = (float)temp; c.top_p = (float)top_p; c.top_p64 = top_p;
    c.top_k = clamp_top_k(top_k);
    c.rep_pen = rep_pen; c.ignore_eos = ignore_eos ? 1 : 0;
    return c;
}
inline RngState rng_fresh(uint64_t seed) {  // seed -> ChaCha key, stream position 0
    RngState r = {};
    seed_from_u64(seed, r.key);
    return r;
}
inline SlotRng slot_rng_fresh(uint64_t seed) {  // a slot's stream at its activation: word 0, no look-ahead word yet (every tag ~0)
    SlotRng sr;
    for (int i = 0; i < 16; ++i) { sr.ahead_at[i] = ~0ull; sr.ahead_word[i] = ~0u; }
    sr.rng = rng_fresh(seed);
    return sr;
}
// what a slot of a FS_SESSION_PER_SLOT session may sample with: the boundary of the in-launch samplers (fishrt.h: fs_lm_generate); in a
// wide session (FS_SESSION_WIDE_SAMPLER): greedy, or temp > 0 with any top_k and any finite top_p.  null = accepted, else the error text
inline const char* slot_sampling_error(double temp, double top_p, uint64_t top_k, bool wide) {
    if (wide) {
        if (!(temp >= 0.0) || temp > 1.7976931348623157e308) return "FS_SESSION_WIDE_SAMPLER: temp must be finite and >= 0 (0 = greedy)";
        if (!(top_p >= -1.7976931348623157e308 && top_p <= 1.7976931348623157e308)) return "FS_SESSION_WIDE_SAMPLER: top_p must be finite";
        return nullptr;
    }
    const bool ok = temp == 0.0 || (temp > 0.0 && top_k > 0 && top_k <= 256);
    return ok ? nullptr : "FS_SESSION_PER_SLOT: a slot samples greedy (temp == 0) or with temp > 0 and 0 < top_k <= 256 (the in-launch samplers' limit)";
}

template <typename WT>
struct SampleKernels {
    // slow token: logits over [im_end, V) (utils.rs:13-16) -> token = idx + im_end; sets done; copies x -> xf; *hid_slot (device
    // pointer cell, may hold null): hidden-state rows [iteration][dim] of generate_blocking_with_hidden
    static void sample_slow(const ModelDims& d, const float* logits, int n, const SampleCfg* c, RngState* rng,
                            SeqState* state, const float* x, float* xf, hipStream_t st, float* const* hid_slot = nullptr);
    // codebook cb: rep-pen (if have_prev), sample, cur[cb+1]; xf = fast_emb[code]; cb == last: finish the frame
    // (record codes, prev = cur, x = embed(cur), pos++, frame++)
    static void sample_fast(const ModelDims& d, const float* logits, int cb, int n_cb, int cb_size, const SampleCfg* c,
                            RngState* rng, RepPenState rp, SeqState* state, const void* fast_emb, float* xf,
                            const void* tok_emb, const void* cb_emb, float* x, uint32_t* out_codes, int out_cap,
                            hipStream_t st);
    // static-batch generator (static_batch.rs): one block per batch row, child StdRng per (call, row)
    // words != null: the block-parallel sampler (512 threads per row) with this step's pre-derived StdRng words (rows_rng_words);
    // requires temp > 1e-7, 0 < top_k <= 256 < candidates (rows_par_sampler_ok)
    static void sample_slow_rows(const ModelDims& d, const float* logits, int ld, int n, const SampleCfg* c, const RngState* master, int B,
                                 int calls_per_frame, SeqState* states, const float* X, float* XF, hipStream_t st, const uint32_t* words = nullptr,
                                 const float* prep_g = nullptr, uint16_t* prep_A = nullptr, uint32_t* epoch = nullptr);
    // prep_g != null (both samplers): the block also leaves RMSNorm(XF row; prep_g) as fragment-major hi/lo GEMM input in prep_A -- what the
    // k_prep node in front of the fast decoder's first layer would produce (RowsCtx::first_prepped)
    static void sample_fast_rows(const ModelDims& d, const float* logits, int cb, int n_cb, int cb_size, const SampleCfg* c,
                                 const RngState* master, int B, SeqState* states, const void* fast_emb, float* XF, const void* tok_emb,
                                 const void* cb_emb, float* X, uint32_t* out_codes, int out_cap, hipStream_t st, const uint32_t* words = nullptr,
                                 const float* prep_g = nullptr, uint16_t* prep_A = nullptr);
    // per-slot samplers of a FS_SESSION_PER_SLOT session: one block per slot, every decision that of the slot's own generate_blocking --
    // cfgs[B], rngs[B] and the repetition-penalty state (rp: mask / seen [B][n_cb][cb_size], ring [B][n_cb][17], ring_meta [B][n_cb][2])
    // are per slot.  Settings per slot: temp == 0, or temp > 0 with 0 < top_k <= 256; n <= 2048, cb_size <= 1024.
    // cfgs[b].legacy (Fish <= 1.4): logits row b = [pad, im_end], the slow token is the 2-way draw of k_sample_slow (one stream word per
    // live frame, greedy included); cap != null: its record [B][cap_frames][9][2048] gets {pad, im_end, u, .., pick at 2047} of decision 0
    // wide (FS_SESSION_WIDE_SAMPLER): the instantiation whose sampled decisions outside that limit (top_k == 0, top_k > 256, top_k >= the
    // candidates) run the block-wide general sampler (wide_sample in lm_sample.hip) instead of being excluded; inside it nothing changes
    static void sample_slow_slots(const ModelDims& d, const float* logits, int ld, int n, const SampleCfg* cfgs, SlotRng* rngs, int B,
                                  SeqState* states, const float* X, float* XF, hipStream_t st, const float* prep_g = nullptr,
                                  uint16_t* prep_A = nullptr, uint32_t* epoch = nullptr, float* cap = nullptr, int cap_frames = 0, bool wide = false);
    static void sample_fast_slots(const ModelDims& d, const float* logits, int cb, int n_cb, int cb_size, const SampleCfg* cfgs, SlotRng* rngs,
                                  RepPenState rp, int B, SeqState* states, const void* fast_emb, float* XF, const void* tok_emb,
                                  const void* cb_emb, float* X, uint32_t* out_codes, int out_cap, hipStream_t st,
                                  const float* prep_g = nullptr, uint16_t* prep_A = nullptr, bool wide = false);
    // words[b * 16 + call] = the StdRng word of sample() call `call` of this step for row b (child stream of master u64 number (frame * calls + call) * B + b)
    static void rows_rng_words(const RngState* master, int B, int calls_per_frame, const SeqState* states, uint32_t* words, hipStream_t st);
};
bool rows_par_sampler_ok(double temp, uint64_t top_k, int n_slow, int cb_size);

// dst[0] = src[r0], dst[1] = src[r1] (rows of `dim` elements): the 2-row head of the Fish <= 1.4 slow-token sampler
template <typename WT>
void launch_gather_rows(const void* src, int dim, uint32_t r0, uint32_t r1, void* dst, hipStream_t st);
void launch_advance(SeqState* state, hipStream_t st);  // pos++, step++ (sequential prefill step)
void launch_advance_n(SeqState* state, int n, hipStream_t st);
// decision capture on the row path (static batch / sessions): cap[row][cap_frames][9][2048]
void launch_cap_rows_logits(const float* logits, int ld, int n, const SeqState* states, const SampleCfg* cfg, int B, float* cap, int cap_frames, int decision,
                            hipStream_t st);
void launch_cap_rows_picks(const SeqState* states, const SampleCfg* cfg, int B, float* cap, int cap_frames, int n_cb, hipStream_t st);  // pos += n, step += n (chunked prefill)
void launch_reppen_reset(RepPenState rp, int n_cb, int cb_size, hipStream_t st);
// copy KV page pairs[2i] -> pairs[2i + 1] (device int array) in each of n_regions pool regions region_bytes apart: ONE launch
void launch_kv_page_copy(void* pool, int n_regions, size_t region_bytes, size_t page_bytes, const int* pairs, int n_pairs, hipStream_t st);
// Prefix KV blobs (fishrt.h: fs_lm_session_prefix_export / _import): the P rows of a prefix between its pages (`pages`: device int array
// of its ceil(P / 64) page ids, each page [Hk][64][Dh]) and the packed payload [n_regions][P][Hk][Dh] (`packed`, 16-byte aligned), in each
// of the n_regions pool regions region_bytes apart (k_kv_rows_gather: pages -> packed; k_kv_rows_scatter: packed -> pages; only the
// valid rows of the last page move).  16-byte loads and stores along Dh: head_dim % 8 != 0 is an error.  ONE launch each.
void launch_kv_rows_gather(const void* pool, int n_regions, size_t region_bytes, size_t page_bytes, const int* pages, int P, int Hk, int Dh,
                           size_t elem_bytes, void* packed, hipStream_t st);
void launch_kv_rows_scatter(void* pool, int n_regions, size_t region_bytes, size_t page_bytes, const int* pages, int P, int Hk, int Dh,
                            size_t elem_bytes, const void* packed, hipStream_t st);
// k_arena_fingerprint: *acc (device, zeroed by the caller) += sum_i w[i] * (2 i + 1) mod 2^64 over the bytes / 4 32-bit words of the arena
void launch_arena_fingerprint(const void* arena, size_t bytes, uint64_t* acc, hipStream_t st);
// Hidden-state collection of session slots (fishrt.h: fs_lm_session_add_hidden): the per-slot table is fs_slot_book.h's HidSlot.
// After the slow transformer of a step, before the slow-token decision: block b appends X[b] (the pre-norm residual row the head's
// RMSNorm reads) to tab[b].rows when the slot collects and runs this iteration (states[b].done == 0); everything else exits at once.
// dim % 4 == 0, X and the buffers 16-byte aligned.  ONE launch (a graph node of the session step: the table is read through pointers).
void launch_hidden_rows(HidSlot* tab, const SeqState* states, const float* X, int dim, int B, hipStream_t st);
// Scoring slots of a FS_SESSION_SCORE session (fishrt.h: fs_lm_session_add_scored): the per-slot table is fs_slot_book.h's ScoreSlot.
// In front of the per-slot sampler node of decision `decision` (0 = slow token over n candidates of rows ld apart; 1 + c = codebook c):
// block b records f32 log-softmax figures of logits row b for the slot's target (candidate 0 left out of a slow decision when
// cfgs[b].ignore_eos), then stores +INFINITY over the target's logit so that the greedy sampler behind it picks the target; at the last
// decision it bumps tab[b].count.  Null entries, done slots and full records exit at once.  2 <= n <= 2048, n_cb == 8.  ONE launch.
// trace_stash != null (FS_SESSION_TRACE sessions): an entry without targets is a TRACED slot (fishrt.h: fs_lm_session_add_traced) -- the
// node leaves top_logprob / top / eos_logprob in the record, m, log s and the raw row in the slot's stash, and the row as it is.
void launch_score_slots(ScoreSlot* tab, const SeqState* states, const SampleCfg* cfgs, float* logits, int ld, int n, int decision, int n_cb, int B,
                        hipStream_t st, float* trace_stash = nullptr, int n_alts = 0);
// n_alts > 0 (FS_SESSION_ALTS sessions, 1 .. 16): the second instantiation of the node -- every scoring and traced slot also leaves, behind
// its records [cap][32] and targets / token rows [cap][n_cb + 1], the n_alts most likely candidates of the decision by the node's own key
// (value descending, -0 == +0, the higher index first among equals; padding 0xFFFFFFFF / NaN where there are fewer) and its entropy:
// alt_index u32 [cap][n_cb + 1][n_alts], alt_logprob f32 [cap][n_cb + 1][n_alts], entropy f32 [cap][n_cb + 1] (fishrt.h:
// fs_lm_session_poll_alts).  n_alts == 0 launches the node as it always was.  The same holds for launch_trace_commit, which fills the
// skipped decisions of an <|im_end|> iteration.
// Traced slots: the per-handle stash f32 [B][TRACE_STASH_WORDS] (per slot a 32-word head + the step's 9 raw rows of <= 2048 candidates),
// and the ONE node behind the frame's last sampler node that closes the rows opened in this step: the picks out of SeqState::cur, their
// log-probs from the stash, the token row behind the records, count + 1.  Every other entry exits at once.  n_cb == 8.
constexpr int TRACE_STASH_WORDS = 32 + 9 * 2048;
void launch_trace_commit(ScoreSlot* tab, const SeqState* states, const SampleCfg* cfgs, float* trace_stash, int n_slow, int cb_size, int n_cb, int B,
                         hipStream_t st, int n_alts = 0);

// synthetic tensor fill (fs_synth.h): n_rows x n_cols, destination row = r * row_mul + row_off (W1/W3 interleave)
template <typename WT>
void launch_synth_fill(WT* dst, uint64_t key, int64_t n_rows, int64_t n_cols, int row_mul, int row_off, float mean,
                       float scale, int round_bf16, hipStream_t st);
// f32 -> WT conversion with the same row mapping (safetensors loader)
template <typename WT>
void launch_convert_rows(WT* dst, const float* src, int64_t n_rows, int64_t n_cols, int row_mul, int row_off,
                         hipStream_t st);
// fp8 quantisers: per-row absmax scale (amax / 448, 1 for an all-zero row), e4m3fn RNE bytes; same row mapping for the
// bytes and the scales.  synth: elements come from the generator (fs_synth.h); rows: from a staged f32 matrix.
void launch_synth_quant_fp8(uint8_t* dst, float* scales, uint64_t key, int64_t n_rows, int64_t n_cols, int row_mul, int row_off,
                            float mean, float scale, hipStream_t st);
void launch_quant_rows_fp8(uint8_t* dst, float* scales, const float* src, int64_t n_rows, int64_t n_cols, int row_mul,
                           int row_off, hipStream_t st);
// out[slot * 256 + b] = f32 value the fp8 GEMV unpack path gives byte b at lane-slot `slot` (16 x 256 floats)
void launch_fp8_decode_table(float* out, hipStream_t st);

// test hook behind fs_selftest_attn (include/fishrt.h; harness at the bottom of lm_attn.hip)
void attn_selftest(int device, const fs_attn_case& c, float* out, size_t out_cap, size_t* n_out, float* k_out, float* v_out, char* variant_out,
                   size_t variant_cap, int* guard_ok);
// test hook behind fs_selftest_gemm (include/fishrt.h; harness at the bottom of lm_gemm.hip)
void gemm_selftest(int device, const fs_gemm_case& c, fs_gemm_out& out);
// test hook behind fs_selftest_gemv (include/fishrt.h; harness at the bottom of lm_kernels.hip)
void gemv_selftest(int device, const fs_gemv_case& c, fs_gemv_out& out);
// test hook behind fs_selftest_sample_frames (include/fishrt.h; harness at the bottom of lm_sample.hip)
void sample_frames_selftest(int device, const fs_sample_case& c, fs_sample_out& out);
// test hook behind fs_selftest_sample_rows (include/fishrt.h)
void debug_sample_rows(int device, const float* logits, int B, int n, double temp, double top_p, uint64_t top_k, uint64_t seed,
                       int call_index, uint32_t* out);
void debug_sample_slots(int device, const float* logits, int S, int R, int n, const SampleCfg* cfgs, const uint64_t* seeds, uint32_t* out,
                        uint64_t* words_used);
// test hook behind fs_selftest_score_rows: the score node's device function on S caller rows of n candidates, one block per row
void debug_score_rows(int device, const float* logits, int S, int n, const uint32_t* targets, int exclude0, float* logprob_out,
                      float* top_logprob_out, uint32_t* top_out, float* row_out);
// test hook behind fs_selftest_alt_rows: the FS_SESSION_ALTS node's device functions on S caller rows of n candidates, one block per row
void debug_alt_rows(int device, const float* logits, int S, int n, int exclude0, int n_alts, uint32_t* alt_index_out, float* alt_logprob_out,
                    float* entropy_out);

}  // namespace fs
