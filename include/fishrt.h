/* fishrt.h -- C ABI of the MI355X-native Fish-Speech hot path (libfishrt.so).
 *
 * Drop-in boundary: the entry points below are what a Rust `fish_speech_core`-shaped shim
 * (or the PyO3 crate, or ctypes) binds INSTEAD of the candle-backed implementation.  Each entry cites the
 * reference interface it replaces (paths relative to the reference repo root).
 *
 * Conventions (mirror of the reference's library API):
 *  - every call returns int status, 0 = ok; on failure a thread-local message is available from
 *    fs_last_error()  (== the `Result<_, candle_core::Error>` / PyRuntimeError string, fish_speech_python/src/utils.rs:6-20);
 *  - all I/O buffers are caller-owned HOST memory, C-contiguous, same shapes as the numpy arrays of the PyO3 API
 *    (fish_speech_python/src/lm.rs:72-145, codec.rs:73-114); handles own all device memory;
 *  - a handle is single-threaded (one in-flight call): mirrors `&mut DualARTransformer`
 *    (server/lib/state.rs:13 serialises with a tokio::Mutex); distinct handles (one per GPU) are independent;
 *  - no CPU fallback exists: creating a handle without a usable gfx950 device fails.
 */
#ifndef FISHRT_H
#define FISHRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FS_OK 0
#define FS_ERR 1

/* weight / KV-cache storage type.  Activations and accumulation are always f32.
 * FS_BF16 == the reference's CUDA dtype choice (fish_speech_core/src/bin/llama_generate.rs:179-182),
 * FS_F32  == its CPU dtype (used here for token-exact parity runs against the f32 oracle),
 * FS_FP8  == no reference counterpart (SURVEY.md §8 configs[4]): the Linear weights (wqkv, wo, w1/w3, w2, output,
 *            fast_output) are quantised at load time to OCP e4m3fn bytes with one f32 absmax scale per output row
 *            (scale = amax/448); embeddings and the KV cache stay bf16, norm vectors f32, all accumulation f32. */
typedef enum { FS_F32 = 0, FS_BF16 = 1, FS_FP8 = 2 } fs_dtype;

/* fish_speech_core/lib/lm/dual_ar.rs:57-81  (BaseModelArgs; training-only fields dropped) */
typedef struct fs_model_args {
    int32_t dim, n_layer, n_fast_layer, n_head, n_local_heads, head_dim;
    int32_t intermediate_size, num_codebooks, codebook_size, vocab_size, max_seq_len;
    float norm_eps, rope_base;
    int32_t tie_word_embeddings;
} fs_model_args;

/* fish_speech_core/lib/lm/dual_ar.rs:17-23  (TokenConfig).  has_semantic_end = 1 for Fish 1.5 (Some(end)), 0 for <= 1.4 */
typedef struct fs_token_cfg {
    uint32_t im_end_id, pad_id, semantic_start_id, semantic_end_id;
    int32_t has_semantic_end;
} fs_token_cfg;

/* fish_speech_core/lib/lm/sampling/mod.rs:29-34  (SamplingArgs) */
typedef struct fs_sampling {
    double temp, top_p;
    uint64_t top_k;
    float repetition_penalty;
} fs_sampling;

typedef struct fs_lm fs_lm_t;
typedef struct fs_codec fs_codec_t;

/* optional per-frame streaming callback (invoked on the calling thread, in frame order):
 * codes[num_codebooks] of frame `frame_idx`.  Return non-zero to stop generation early. */
typedef int (*fs_frame_cb)(void* user, size_t frame_idx, const uint32_t* codes);

const char* fs_last_error(void);
/* library/ABI version and the gfx target the kernels were compiled for ("gfx950") */
const char* fs_version(void);
/* number of visible HIP devices (0 when none: every create call then fails loudly) */
int fs_device_count(void);

/* ---- DualARTransformer ---------------------------------------------------------------------------------- */

/* FS_FP8 storage format (no reference counterpart; SURVEY.md §8 configs[4]).  fs_fp8_quantize_rows runs the loader's device
 * quantiser on a host f32 matrix [rows, cols]: scales_out[r] = amax_r / 448 (1 for an all-zero row), q_out = e4m3fn bytes of
 * w / scale (round-to-nearest-even, saturating; never NaN) -- what fs_lm_load_* stores for every Linear weight of an FS_FP8
 * handle.  fs_fp8_decode_table returns, for each of the 16 byte positions of a lane's 16-byte weight load, the f32 value the
 * GEMV kernels give each of the 256 byte codes (out[slot * 256 + code]). */
int fs_fp8_quantize_rows(int device_id, const float* w, int64_t rows, int64_t cols, uint8_t* q_out, float* scales_out);
int fs_fp8_decode_table(int device_id, float* out);

/* Device self-test of an internal building block, by name (diagnostics; used by the parity tests): "pf_reduce" = the multi-value
 * wave reductions of the persistent fast-decoder kernel (csrc/lm_persist.hip) against host sums.  0 = passed. */
int fs_selftest(int device_id, const char* what);
/* The static-batch sampler (BatchedLogitsProcessor::sample, sampling/mod.rs:77-109) on caller-provided logits f32 [B, n]
 * (n <= 4096): out[b] = token of row b for sample() call number `call_index` of a request seeded with `seed` (row b draws from
 * the child StdRng seeded with master u64 number call_index * B + b; temp <= 1e-7 -> first-max argmax).  Diagnostics / parity tests. */
int fs_selftest_sample_rows(int device_id, const float* logits, int B, int n, const fs_sampling* s, uint64_t seed, int call_index,
                            uint32_t* out);

/* The per-slot sampler of a FS_SESSION_PER_SLOT | FS_SESSION_WIDE_SAMPLER session on caller-provided logits f32 [S][R][n] (n <= 2048).
 * Stream s is one slot: its StdRng is seeded seeds[s], its settings are samplings[s] (greedy, or temp > 0 with any top_k / top_p), and it
 * makes the decisions r = 0 .. R-1 in order on its rows -- no repetition penalty, no EOS masking.  out[s * R + r] = the picked index,
 * words_used[s] = stream words consumed after the R decisions.  One block per stream runs the device function the wide slot kernels
 * call; settings inside the narrow limit (0 < top_k <= 256 < n) take the block-parallel sampler, exactly as a slot's would.
 * Diagnostics / parity tests. */
int fs_selftest_sample_slots(int device_id, const float* logits, int S, int R, int n, const fs_sampling* samplings, const uint64_t* seeds,
                             uint32_t* out, uint64_t* words_used);
/* The score node of a FS_SESSION_SCORE session (k_score_slots' device function) on caller-provided logits f32 [S][n] (2 <= n <= 2048), one
 * block per row, target candidate targets[s] < n, exclude0 != 0: candidate 0 is left out (what FS_GEN_IGNORE_EOS does to <|im_end|> at
 * the slow decision).  logprob_out[s] = log-softmax of the row at its target, top_logprob_out[s] = at its maximum, top_out[s] = the LAST
 * maximal index (-0 == +0), all f32 arithmetic; row_out f32 [S][n] = the rows as the node leaves them (the input with +inf at the
 * target).  Output pointers nullable.  Diagnostics / parity tests. */
int fs_selftest_score_rows(int device_id, const float* logits, int S, int n, const uint32_t* targets, int exclude0, float* logprob_out,
                           float* top_logprob_out, uint32_t* top_out, float* row_out);
/* The score node of a FS_SESSION_ALTS session (its device functions) on caller-provided logits f32 [S][n] (2 <= n <= 2048), one block per
 * row, 1 <= n_alts <= 16, exclude0 as above (candidate 0 takes no part).  alt_index_out u32 / alt_logprob_out f32 [S][n_alts],
 * entropy_out f32 [S]: order, padding and arithmetic as stated at fs_lm_session_poll_alts.  Output pointers nullable.
 * Diagnostics / parity tests. */
int fs_selftest_alt_rows(int device_id, const float* logits, int S, int n, int exclude0, int n_alts, uint32_t* alt_index_out,
                         float* alt_logprob_out, float* entropy_out);

/* ONE convolution of the vocoder on caller-provided host data, through the load-time and launch functions the codec engine itself uses
 * (csrc/codec_kernels.h) and nothing else: the weights arrive in checkpoint layout -- Conv1d [Cout][Cin][K], ConvTranspose1d [Cin][Cout][K]
 * -- and go through codec_relayout / codec_relayout_tconv and, for the matrix modes, codec_pack_bf3; then one launcher call of kind `flow`:
 *   FS_CONV_CONV1D / FS_CONV_TCONV1D               codec_conv1d / codec_tconv1d: f32 in (input = FS_CONV_IN_F32), f32 out
 *   FS_CONV_CONV1D_PLANES / FS_CONV_TCONV1D_PLANES codec_conv1d_planes / codec_tconv1d_planes (precision 1 | 2): f32 or plane input, f32 and / or
 *                                                  plane output, post_silu, and with mean_a / mean_b the ParallelBlock mean folded into a
 *                                                  FS_CONV_EPI_RES epilogue: ((mean_a + mean_b) + (res + conv)) * (float)(1/3)
 *   FS_CONV_RESPAIR_F16                            codec_respair_f16 (precision 2, Cin == Cout in {16, 32}): res + conv2(silu(conv1(xp))) with
 *                                                  w / bias and w2 / bias2, the same K and dil on both
 * precision: 0 = f32, 1 = bf16x3, 2 = f16, the meaning fs_codec_set_precision gives them.  Causal, stride 1, left zero pad (K-1)*dil; a
 * transposed conv has `stride`, K % stride == 0, right trim K - stride, and T * stride output samples.  epi = FS_CONV_EPI_*; res [B][Cout][T],
 * gamma [Cout], bias [Cout].  No streaming contexts: every call is the start of a signal.
 * input: FS_CONV_IN_F32 = the launcher reads x [B][Cin][T] itself (pre_silu applies); the others first make the activation planes the launcher
 * reads: codec_act_split(x) without / with SiLU, or codec_mean3_planes(x, x_b, x_c) without / with SiLU (pre_silu is then not applied again).
 * outputs: bit FS_CONV_OUT_F32 -> y_out f32 [B][Cout][T (* stride)]; bit FS_CONV_OUT_PLANES -> planes_out f32 [B][Cout][64 + T]: the plane
 * tensor the launcher wrote, read back and returned as the values it encodes (bf16x3: hi + lo, f16: the f16 value), INCLUDING the 64 pad
 * slots in front of every row (zeros at the start of a signal).  Both output buffers are poisoned (NaN) before the launch.
 * variant_out receives the NUL-terminated name of the kernel instantiation the launcher chose ("f32/mfma/OT64/TT256",
 * "f16/bf3p/TT256/nibs4/RES", "f16/pair/K7/nib2/NW8/NH2", ...; "chk/" in front: the range-checked twin).
 * range_check != 0 (precision 1 | 2): pack, producers and launcher run as under fs_codec_set_range_check, and range_out[0] / [1] receive
 * the operands counted as saturated (|v| > 65504) / flushed (0 < |v| < 2^-24) by the f32 -> f16 conversions of this call (each weight once
 * at pack time; each activation once per conversion, i.e. once for a plane producer).  Diagnostics / parity tests. */
enum { FS_CONV_CONV1D = 0, FS_CONV_TCONV1D = 1, FS_CONV_CONV1D_PLANES = 2, FS_CONV_TCONV1D_PLANES = 3, FS_CONV_RESPAIR_F16 = 4 };
enum { FS_CONV_IN_F32 = 0, FS_CONV_IN_SPLIT = 1, FS_CONV_IN_SPLIT_SILU = 2, FS_CONV_IN_MEAN3 = 3, FS_CONV_IN_MEAN3_SILU = 4 };
enum { FS_CONV_EPI_NONE = 0, FS_CONV_EPI_GELU = 1, FS_CONV_EPI_GAMMA_RES = 2, FS_CONV_EPI_RES = 3, FS_CONV_EPI_TANH = 4 };
enum { FS_CONV_OUT_F32 = 1, FS_CONV_OUT_PLANES = 2 };
typedef struct fs_conv_case {
    int32_t flow, precision;
    int32_t B, Cin, Cout, T, K, dil, stride;
    int32_t pre_silu, epi, post_silu;
    int32_t input, outputs;
    int32_t range_check, reserved;
    const float *x, *x_b, *x_c;
    const float *w, *bias, *w2, *bias2;
    const float *res, *gamma, *mean_a, *mean_b;
} fs_conv_case;
int fs_selftest_conv1d(int device_id, const fs_conv_case* c, float* y_out, float* planes_out, char* variant_out, size_t variant_cap,
                       uint64_t* range_out);

/* ONE launcher of the codec's encoder-side / ConvNeXt / FSQ kernels (csrc/codec_kernels.h) on caller-provided host data, and nothing else:
 * the inputs go to the device as they are (no re-layout: these launchers read the checkpoint's own layouts), one launcher call of kind `op`
 * runs, the output comes back.  All tensors f32 row-major unless stated; T >= 1, every other dimension >= 1.
 *   FS_CODEC_OP_STFT_MAG        codec_stft_mag: x = PCM (n), n_fft (2048 only), hop, T = frames to compute -> lin [n_fft/2+1][T].  Frame f
 *                               = padded[f * hop, f * hop + n_fft) of the reflect pad that REPEATS the edge sample ((n_fft - hop) / 2 per
 *                               side, so n >= that), zero behind the padded signal, periodic Hann, f64 FFT, (f32)|.| + 1e-6f.  T is the
 *                               caller's: (T - 1) * hop < n + n_fft - hop is required (every frame starts inside the padded signal)
 *   FS_CODEC_OP_MEL_LOG         codec_mel_log: x = lin [nf][T], w0 = filterbank [nf][n_mels] -> [n_mels][T] = logf(clamp(sum_k lin[k][t] *
 *                               fb[k][m], 1e-5, 100)), the sum an ascending-k chain of separately rounded f32 products and sums
 *   FS_CODEC_OP_LAYERNORM_CF    codec_layernorm_cf: x [C][T], w0 = weight [C], w1 = bias [C] -> [C][T]; per time step over the channels,
 *                               biased variance, eps 1e-6
 *   FS_CODEC_OP_DWCONV_LN       codec_dwconv_ln: x [B][C][T], w0 = depthwise taps [C][7], w1 = their bias [C], w2 / w3 = LayerNorm weight /
 *                               bias [C] -> [B][C][T]; causal (tap k reads x[t + k - 6]).  ctx_mode 0: zeros in front of the signal; 1 (B ==
 *                               1): ctx [C][16] = the last 16 samples per channel of what came before; 2: ctx = a pool of ctx_elems floats
 *                               and ctx_off int64 [2B], item b reading its [C][16] context at ctx + ctx_off[2b] (the layout of the
 *                               multi-stream decoder's offset table; entry 2b + 1 is not read).  C > 1024 is the launcher's own error
 *   FS_CODEC_OP_SPACE_TO_DEPTH  codec_space_to_depth: x [C][T], s >= 1 -> [C * s][T / s], y[c * s + k][t] = x[c][t * s + k]; the last
 *                               T % s columns are dropped, T < s gives an empty output
 *   FS_CODEC_OP_FSQ_ENCODE      codec_fsq_encode: x [C][T], G groups (C % G == 0, dg = C / G), w0 = project_in weight [G][4][dg], w1 = its
 *                               bias [G][4] -> uint32 indices [G][T] (levels 8, 5, 5, 5; bases 1, 8, 40, 200)
 *   FS_CODEC_OP_FSQ_PROJECT     codec_fsq_project: codes uint32 [B * G][T] (each < 1000), dg, w0 = project_out weight [G][dg][4], w1 = its
 *                               bias [G][dg] -> [B][G * dg][T]; item (b, g) reads row g * B + b, or with item_rows != 0 row b * G + g
 * `out` receives n_out 4-byte elements (f32, or uint32 for FS_CODEC_OP_FSQ_ENCODE), out_cap >= that.  The device output buffer has 256
 * guard elements in front of and behind its logical extent and is filled with 0xFF bytes (f32 NaN, uint32 0xFFFFFFFF) before the launch:
 * an element the launcher did not write comes back as NaN, and guard_ok = 1 iff every guard byte is still 0xFF afterwards -- a write past
 * either end is reported instead of corrupting a neighbour.  Diagnostics / parity tests. */
enum { FS_CODEC_OP_STFT_MAG = 0, FS_CODEC_OP_MEL_LOG = 1, FS_CODEC_OP_LAYERNORM_CF = 2, FS_CODEC_OP_DWCONV_LN = 3,
       FS_CODEC_OP_SPACE_TO_DEPTH = 4, FS_CODEC_OP_FSQ_ENCODE = 5, FS_CODEC_OP_FSQ_PROJECT = 6 };
typedef struct fs_codec_op_case {
    int32_t op;
    int32_t B, C, T;
    int32_t n, n_fft, hop;   /* FS_CODEC_OP_STFT_MAG */
    int32_t nf, n_mels;      /* FS_CODEC_OP_MEL_LOG */
    int32_t s;               /* FS_CODEC_OP_SPACE_TO_DEPTH */
    int32_t G, dg;           /* FS_CODEC_OP_FSQ_* */
    int32_t ctx_mode;        /* FS_CODEC_OP_DWCONV_LN */
    int32_t item_rows;       /* FS_CODEC_OP_FSQ_PROJECT */
    int32_t reserved[2];
    int64_t ctx_elems;
    const float *x, *w0, *w1, *w2, *w3, *ctx;
    const int64_t* ctx_off;
    const uint32_t* codes;
} fs_codec_op_case;
int fs_selftest_codec_op(int device_id, const fs_codec_op_case* c, void* out, size_t out_cap, size_t* n_out, int* guard_ok);

/* ONE attention launcher call (csrc/lm_kernels.h: AttnKernels::decode / rows, LmKernels::wo) on caller-provided host data, and nothing else.
 *   FS_ATTN_DECODE     AttnKernels::decode (M == 1, position `pos`) -> out = the partials f32 [H][n_chunks_max][Dh + 2] ({o[Dh], m, l},
 *                      un-normalised), NaN-poisoned before the launch: slots of chunks the launch did not produce come back NaN
 *   FS_ATTN_DECODE_WO  decode, then LmKernels::wo with wo [dim][dim] and x [dim] -> out = x [dim] (x += Wo . merged attention); the
 *                      partials buffer is pre-filled with `stale_part` instead of NaN (the merge must mask every slot decode did not write)
 *   FS_ATTN_WO_FUSED   LmKernels::wo with fused_T in 1..8: attention of q over rows 0 .. fused_T - 1 of page 0, then Wo -> out = x [dim]
 *   FS_ATTN_ROWS       AttnKernels::rows with the RowsCtx flags below -> out = hi plane then lo plane, each f32 [Mcap][H * Dh], Mcap = M
 *                      rounded up to 32: the fragment-major bf16 GEMM input de-fragmented; rows >= M come back NaN (never written)
 *   FS_ATTN_EXPF       out[i] = __expf(expf_x[i]), i < n_expf, in a kernel of its own (the device function the softmaxes use)
 * wt: FS_ATTN_WT_F32 / _BF16 / _FP8 selects AttnKernels<WT> / LmKernels<WT>; the KV type is f32 for F32 and bf16 otherwise; with FP8 wo
 * is stored as e4m3fn bytes of its values with scale 1 per row.  dim == H * Dh.  Row positions: row m sits at pos + m * pos_step
 * (pos_step 1 / 0), at row_pos[m] (pos_step < 0), or -- seq_rows > 0, group prefill -- row m of sequence s at (seq_pos ? seq_pos[s] : pos) +
 * m; its length T is that + 1.  k / v: the pools in pool layout f32 [n_pages][Hk][64][Dh], converted to the KV type (RNE; exact for values
 * already in it); every row of every page is the caller's, stale ones included.  page_table int32 [pt_rows][pt_len] (row stride pt_stride
 * as the launcher sees it).  q f32 [M][H * Dh].  tbl0 != 0 (k_attn_small_rows_tbl): tbl f32 [tbl_rows][(H + 2 Hk) Dh], codes[m] < tbl_rows
 * the row's code (stored in cur[code_slot] of its state), cos_t / sin_t f32 [rope_rows][Dh / 2], RoPE row = position + rope_off.
 * Every device buffer the launch writes (outputs, partials, both pools) lies between 256-element guards of 0xFF bytes; guard_ok = 1 iff all
 * of them are intact afterwards.  k_out / v_out (nullable): the pools after the launch, f32 in pool layout.  variant_out: the name of the
 * launch plan (AttnPlan::name: "decode/bf16/64/2/hs4", "decode/part/tpb2", "rows/bf16/64/4/hs2/remap", "rows/chunked/32", "small/64/ident",
 * "small_tbl/64", "prefill_mfma/group", ...; DECODE_WO appends "+wo/reg" or "+wo/lds", the merge k_wo takes; "wo/fused/64").
 * The case is VALIDATED BEFORE ANY DEVICE CALL: geometry, capacities, every page id < n_pages, every page-table slot any launched block
 * reads inside the table, T <= pt_len * 64, small_attn => T <= 8; a bad case is an error and nothing is launched.  plan_only != 0: validate,
 * return the plan name, touch no device (works without a GPU).  Diagnostics / parity tests. */
enum { FS_ATTN_DECODE = 0, FS_ATTN_DECODE_WO = 1, FS_ATTN_WO_FUSED = 2, FS_ATTN_ROWS = 3, FS_ATTN_EXPF = 4 };
enum { FS_ATTN_WT_F32 = 0, FS_ATTN_WT_BF16 = 1, FS_ATTN_WT_FP8 = 2 };
typedef struct fs_attn_case {
    int32_t op, wt;
    int32_t H, Hk, Dh, dim;
    int32_t M, pos, pos_step, rope_off;
    int32_t pt_stride, pt_rows, pt_len, seq_rows;
    int32_t n_chunks_max, nc_launch, part_rows;
    int32_t no_flash, chunked_attn, small_attn, identity_pages;
    int32_t n_pages, fused_T;
    int32_t tbl0, code_slot, tbl_rows, rope_rows;
    int32_t n_expf, plan_only, reserved;
    float stale_part;
    int32_t reserved2;
    const int32_t *row_pos, *seq_pos, *page_table;
    const float *k, *v, *q, *wo, *x, *tbl, *cos_t, *sin_t, *expf_x;
    const uint32_t* codes;
} fs_attn_case;
int fs_selftest_attn(int device_id, const fs_attn_case* c, float* out, size_t out_cap, size_t* n_out, float* k_out, float* v_out,
                     char* variant_out, size_t variant_cap, int* guard_ok);

/* ONE launcher call of the row-path GEMM family (csrc/lm_gemm.hip: k_prep, launch_gemm3 -> k_gemm3 / k_gemm_big, launch_gemm_down ->
 * k_gemm_down) on caller-provided host data, and nothing else.  All tensors f32 row-major unless stated; Mcap = M rounded up to 32.
 *   FS_GEMM_PREP  k_prep as rows_layer / rows_finish launch it: x [M][D] (+= the S slabs p [S][M][D], S may be 0), norm_w [D] (nullable),
 *                 eps; want_frag = 0 launches it without a fragment output.  out.y = X [M][D]; out.planes = hi then lo, each [Mcap][D].
 *   FS_GEMM_ROWS  launch_gemm3<epi, rt> for the (epi, rt) pairs of rows_layer / rows_head (SWIGLU / SWIGLU_RMS with rt 2, every other
 *                 epilogue with rt 1; anything else is an error).  x [M][K]: the harness makes the hi / lo fragments with k_prep (no norm: a
 *                 plain split).  w [N][K]: fp8 == 0 -> every value exactly a bf16 value; fp8 != 0 -> every value exactly an e4m3fn value and
 *                 wscale [N] the row scales (anything else is an error).  Epilogue inputs: y [M][ldy] (the residual stream of RESIDUAL /
 *                 RESIDUAL_NORM), g [N] (RESIDUAL_NORM), ss [M][nblk] + eps (the *_RMS epilogues; the row's rms is sqrt(sum_b ss / K + eps)),
 *                 QKV*: cos_t / sin_t [rope_rows][Dh / 2], N == (H + 2 Hk) Dh, the pools k / v f32 [n_pages][Hk][64][Dh] (bf16 values),
 *                 page_table int32 [pt_rows][pt_len]; positions: row m at pos + m * pos_step (pos_step 1 / 0), at row_pos[m] with rope offset
 *                 row_rope_off[m] (pos_step < 0: per-row states), token m % seq_rows of sequence m / seq_rows at pos (QKV, QKV_RMS) or at
 *                 seq_pos[s] with seq_rope_off[s] (QKV_SEQ), page-table row of a sequence pt_stride apart; o1 != 0: the QKV launch also
 *                 leaves the attention output of a one-token cache.  ldy: row stride of Y; ldo: of the SwiGLU planes (0 = N / 2).
 *                 big_min_m (0 = the production value) replaces FISHRT_GEMM_BIG_MIN_M for this call.
 *                 out.y = Y: STORE / STORE_RMS [ksplit][Mcap][ldy] (every slab), else [Mcap][ldy]; out.planes = hi then lo of the fragment
 *                 output, each [Mcap][C]: SWIGLU* C = ldo, RESIDUAL_NORM C = N, QKV* with o1 C = H Dh; out.ss [Mcap][grid.x] (RESIDUAL_NORM);
 *                 out.k / out.v = both pools after the launch.
 *   FS_GEMM_DOWN  launch_gemm_down: x [M][K] (x2: the second launch's), w [N][K], y = X [M][N], g [N], n_launches 1 or 2 on the same
 *                 exchange buffer with node ids node_id, node_id + 1 and step epoch `epoch` (>= 1).  Every exchange unit starts as {NaN,
 *                 stale_tag, NaN, stale_tag}.  Refused unless gemm_down_ok AND the device holds the whole grid at once (the owner waves
 *                 wait for blocks of the same launch); with plan_only residency is not queried.  Per launch: out.y [32][N], out.planes
 *                 [2][32][N], out.ss [32][N / 16], out.epoch1 = the give-up counter.
 * Every device buffer a launch writes lies between 256-element guards of 0xFF bytes and is itself filled with 0xFF bytes (f32 / bf16 NaN)
 * where the caller provides nothing; out.guard_ok = 1 iff every guard is intact.  Fragment rows [M, Mcap) of every GEMM input hold bf16 NaN.
 * out.variant: GemmPlan::name ("gemm3/QKV_RMS/nks8/rt1/bf16/half", "big/SWIGLU_RMS/fp8", "down/nks8/ks4/bf16", "prep/one", "prep/reread");
 * out.grid: the launch grid.  Output pointers are nullable; a non-null one needs its capacity.  The case is VALIDATED BEFORE ANY DEVICE
 * CALL; a bad case is an error and nothing is launched.  plan_only != 0: validate, return name and grid, touch no device.
 * Diagnostics / parity tests. */
enum { FS_GEMM_PREP = 0, FS_GEMM_ROWS = 1, FS_GEMM_DOWN = 2 };
enum { FS_GEMM_EPI_STORE = 0, FS_GEMM_EPI_RESIDUAL = 1, FS_GEMM_EPI_SWIGLU = 2, FS_GEMM_EPI_QKV = 3, FS_GEMM_EPI_RESIDUAL_NORM = 4,
       FS_GEMM_EPI_SWIGLU_RMS = 5, FS_GEMM_EPI_QKV_RMS = 6, FS_GEMM_EPI_STORE_RMS = 7, FS_GEMM_EPI_QKV_SEQ = 8 };
typedef struct fs_gemm_case {
    int32_t op, fp8, epi, rt;
    int32_t M, N, K, ksplit;
    int32_t D, S, want_frag, ldy;
    int32_t ldo, H, Hk, Dh;
    int32_t pos, rope_off, pos_step, pt_stride;
    int32_t seq_rows, pt_rows, pt_len, n_pages;
    int32_t rope_rows, o1, nblk, big_min_m;
    int32_t n_launches, stale_tag, node_id, epoch;
    int32_t plan_only, reserved;
    float eps;
    int32_t reserved2;
    const float *x, *x2, *p, *norm_w, *w, *wscale, *y, *g, *ss, *cos_t, *sin_t, *k, *v;
    const int32_t *row_pos, *row_rope_off, *seq_pos, *seq_rope_off, *page_table;
} fs_gemm_case;
typedef struct fs_gemm_out {
    float *y, *planes, *ss, *k, *v;
    uint32_t* epoch1;
    char* variant;
    size_t y_cap, planes_cap, ss_cap, pool_cap, variant_cap;
    size_t n_y, n_planes, n_ss;
    int32_t grid[3];
    int32_t guard_ok;
} fs_gemm_out;
int fs_selftest_gemm(int device_id, const fs_gemm_case* c, fs_gemm_out* out);

/* ONE launcher call of the batch-1 node kernels (csrc/lm_kernels.hip: LmKernels::qkv / ffn_up / ffn_down / head / wo / embed / fast_embed) on
 * caller-provided host data, and nothing else.  All tensors f32 row-major unless stated.  wt: FS_GEMV_WT_F32 / _BF16 / _FP8 selects
 * LmKernels<WT>; the KV cache and the embedding tables are f32 for F32 and bf16 otherwise.  Weights `w` are f32 values that must already lie
 * on the weight type's grid (bf16 / e4m3fn; anything else is an error), fp8 also needs wscale, one f32 scale per weight row.
 *   FS_GEMV_QKV         x [dim], norm_w [dim], eps, w [(H + 2 Hk) Dh][dim], cos_t / sin_t [rope_rows][Dh / 2], the pools k / v
 *                       [n_pages][Hk][64][Dh] (values of the KV type), page_table int32 [pt_len].  use_state != 0: position and RoPE offset
 *                       come from a device SeqState {pos, rope_off} (the slow path); use_state == 0: a null state and pos_static = pos,
 *                       rope_static = pos + rope_off (the fast decoder).  out.y = q [H Dh]; out.k / out.v = both pools after the call.
 *   FS_GEMV_FFN_UP      x [dim], norm_w [dim], eps, w [2 inter][dim] row-interleaved (w1[r], w3[r]) -> out.y = act [inter]
 *   FS_GEMV_FFN_DOWN    x = act [inter], w [dim][inter], y = the residual stream [dim] -> out.y = y + s (W act) [dim]
 *   FS_GEMV_HEAD        x [dim], norm_w [dim], eps, w [n_rows][dim] -> out.y = logits [n_rows]
 *   FS_GEMV_WO_BODY     LmKernels::wo with fused_T = 0, nc_launch = 1 and host-written partials {o = x, m = 0, l = 1} of every head at
 *                       position 0: the merge weight is exactly 1 and the call computes y + s (W x).  x [dim], w [dim][dim], y [dim],
 *                       dim == H Dh -> out.y [dim]
 *   FS_GEMV_EMBED       tok_emb [tok_rows][dim], cb_emb [n_cb cb_size][dim] (values of the KV type), sem_lo / sem_hi.  use_prompt != 0:
 *                       tokens = the staged prompt, uint32 [n_tokens], token c of the column at tokens[step + c * prompt_L] (SeqState
 *                       {step, prompt_L}); use_prompt == 0: tokens = SeqState::cur, uint32 [n_cb + 1].  out.y = x [dim]
 *   FS_GEMV_FAST_EMBED  tok_emb = the fast embedding table [tok_rows][dim], ids uint32 [n_ids] -> out.y [n_ids][dim]
 * cache_resident selects the weight-load policy of the four launchers that have one (LayerW::cache_resident).  Every device buffer a
 * launch writes (outputs, both pools) lies between 256-element guards of 0xFF bytes and is itself 0xFF bytes (NaN) where the caller
 * provides nothing; out.guard_ok = 1 iff every guard is intact.  out.variant: GemvPlan::name ("qkv/bf16/K1024/w2/nt",
 * "down/fp8/K4096/ks4/res", "head/f32/K128/w4", "wo/bf16/K1024/w4/dh64/nt", "up/f32/K256/w4/res", "embed/bf16", "fast_embed/f32");
 * out.grid: the launch grid.  The case is VALIDATED BEFORE ANY DEVICE CALL (widths, geometry, every page id, the page-table slot of pos,
 * the RoPE row, every token id); a bad case is an error and nothing is launched.  plan_only != 0: validate, return name and grid, touch no
 * device.  Diagnostics / parity tests. */
enum { FS_GEMV_QKV = 0, FS_GEMV_FFN_UP = 1, FS_GEMV_FFN_DOWN = 2, FS_GEMV_HEAD = 3, FS_GEMV_WO_BODY = 4, FS_GEMV_EMBED = 5,
       FS_GEMV_FAST_EMBED = 6 };
enum { FS_GEMV_WT_F32 = 0, FS_GEMV_WT_BF16 = 1, FS_GEMV_WT_FP8 = 2 };
typedef struct fs_gemv_case {
    int32_t op, wt, plan_only, cache_resident;
    int32_t dim, inter, H, Hk;
    int32_t Dh, n_rows, pos, rope_off;
    int32_t use_state, n_pages, pt_len, rope_rows;
    int32_t n_cb, cb_size, tok_rows, prompt_L;
    int32_t step, use_prompt, n_tokens, n_ids;
    uint32_t sem_lo, sem_hi;
    float eps;
    int32_t reserved;
    const float *x, *norm_w, *w, *wscale, *y, *cos_t, *sin_t, *k, *v, *tok_emb, *cb_emb;
    const int32_t* page_table;
    const uint32_t *tokens, *ids;
} fs_gemv_case;
typedef struct fs_gemv_out {
    float *y, *k, *v;
    char* variant;
    size_t y_cap, pool_cap, variant_cap;
    size_t n_y, n_pool;
    int32_t grid[3];
    int32_t guard_ok;
} fs_gemv_out;
int fs_selftest_gemv(int device_id, const fs_gemv_case* c, fs_gemv_out* out);

/* F frames of the PRODUCTION sampler launches (csrc/lm_sample.hip) on caller-provided logits, and nothing else: per frame the launchers the
 * engine calls, in its order -- SampleKernels::rows_rng_words (ROWS_PAR only), the slow sampler, then the fast sampler for codebooks
 * 0 .. n_cb - 1 -- with the complete sampler state copied out after EVERY launch.  L = F * ((ROWS_PAR ? 1 : 0) + 1 + n_cb) launches.
 *   family                kernels
 *   FS_SAMPLE_SINGLE           k_sample_slow, k_sample_fast                     (B == 1)
 *   FS_SAMPLE_SINGLE_BATCHROW  the same two with batch_rows > 0: row batch_row of a static batch of batch_rows rows (B == 1)
 *   FS_SAMPLE_ROWS             k_sample_slow_rows, k_sample_fast_rows
 *   FS_SAMPLE_ROWS_PAR         k_rows_rng_words, k_sample_slow_rows_par, k_sample_fast_rows_par   (rows_par_sampler_ok settings only)
 *   FS_SAMPLE_SLOTS            k_sample_slow_slots<false>, k_sample_fast_slots<false>   (per slot: temp == 0, or temp > 0 with 0 < top_k <= 256)
 *   FS_SAMPLE_SLOTS_WIDE       k_sample_slow_slots<true>, k_sample_fast_slots<true>     (per slot: any finite temp >= 0, top_p)
 * wt: FS_GEMV_WT_F32 / _BF16 selects SampleKernels<float> / <bf16_t> (the two table types KVT<WT> has); the tables tok_emb [tok_rows][dim],
 * cb_emb [n_cb cb_size][dim], fast_emb [cb_size][dim] are f32 values that must lie on that type's grid.  tokens: the token layout, from which
 * the SampleCfg is made as the engine makes it (has_semantic_end == 0: the Fish <= 1.4 two-way slow decision; SINGLE, SLOTS, SLOTS_WIDE
 * only, n_slow == 2).  samplings / seeds / ignore_eos: n_cfg entries, n_cfg = B for the SLOTS families (one StdRng stream per slot, as a
 * freshly activated slot's) and 1 otherwise (the request's stream; the master stream of the row families, whose repetition_penalty is
 * ignored: the batch paths run with 1).  session: SampleCfg::session of the row families (0: dead rows step in lock-step, 1: they freeze).
 * state0: the initial SeqState of every row, int32 [B][40] = {pos, rope_off, frame, done, n_out, have_prev, step, prompt_L, cur[16],
 * prev[16]}.  x: the hidden row the slow sampler of frame f finds in X, f32 [F][B][dim] (uploaded in front of it).  logits: per frame the
 * slow rows [B][n_slow] (placed ld apart on the device, the gap poisoned), then per codebook [B][cb_size].  prep != 0: the RMSNorm + hi/lo
 * split epilogue with prep_g [dim], eps and the step epoch (row families, slots).  hid != 0 (SINGLE): the hidden-state rows of
 * generate_blocking_with_hidden.  cap_frames > 0 (SLOTS families): the decision capture record of the slow sampler.
 * Outputs, all nullable, cap[i] / need[i] in BYTES, [L] leading (the state after launch l):
 *   STATES int32 [L][B][40]; RING int32 [L][R][n_cb][17], META int32 [L][R][n_cb][2], MASK f32 [L][R][n_cb][cb_size] (R = B for the SLOTS
 *   families, 1 for SINGLE*, 0 for the row families, which take no penalty state); RNG: SINGLE* RngState as u32 [L][10], row families the
 *   master's [L][10], SLOTS the SlotRng cells u32 [L][B][58] ({key[8], consumed lo, hi, ahead_at[16] lo / hi pairs, ahead_word[16]});
 *   WORDS u32 [L][B][16] (ROWS_PAR); XF, X f32 [L][B][dim]; PREP uint16 [L][2 * 32 * dim] (the fragment-major hi / lo buffer of 32 rows),
 *   EPOCH u32 [L][2]; CODES u32 [L][B][n_cb][out_cap]; HID f32 [L][frame0 + F][dim]; CAP f32 [L][B][cap_frames][4] = entries 0, 1, 2 and
 *   2047 of decision 0's record.
 * Every device buffer lies between 256-element guards of 0xFF bytes and is 0xFF bytes where the case provides nothing; the penalty state
 * is reset with launch_reppen_reset as at a request's start.  guard_ok = 1 iff every guard is intact after the last launch.
 * The case is VALIDATED BEFORE ANY DEVICE CALL: the launchers' capacities, n_cb + 1 <= 16, rows_par_sampler_ok for ROWS_PAR, the
 * narrow-setting rule for SLOTS (greedy, or 0 < top_k <= 256 and below both
 * candidate counts), dim <= 1024 in whole 32-wide fragments for the prep epilogue, every token id the tables are indexed with; a bad case is an error and nothing
 * is launched.  plan_only != 0: validate, fill n_launches and need[], touch no device.  Diagnostics / parity tests.
 *
 * THE HOST ArgMax RULE (temp == 0 on the single-sequence and per-slot paths): candle's LogitsProcessor picks
 * `iter().enumerate().max_by(|a, b| a.total_cmp(b))`: the order is IEEE-754 totalOrder, under which -0.0 < +0.0, and among candidates of
 * IDENTICAL bit pattern the LAST index wins.  greedy_pick, slot_greedy_pick and the oracle's LogitsProcessor::sample follow it (a maximum
 * of +0 beats a -0 wherever either stands).  The batch rule (temp <= 1e-7 on the static-batch paths) is the tensor argmax: IEEE `>`, the
 * FIRST maximal index, -0 == +0.  NaN logits are outside both rules. */
enum { FS_SAMPLE_SINGLE = 0, FS_SAMPLE_SINGLE_BATCHROW = 1, FS_SAMPLE_ROWS = 2, FS_SAMPLE_ROWS_PAR = 3, FS_SAMPLE_SLOTS = 4,
       FS_SAMPLE_SLOTS_WIDE = 5 };
enum { FS_SAMPLE_OUT_STATES = 0, FS_SAMPLE_OUT_RING = 1, FS_SAMPLE_OUT_META = 2, FS_SAMPLE_OUT_MASK = 3, FS_SAMPLE_OUT_RNG = 4,
       FS_SAMPLE_OUT_WORDS = 5, FS_SAMPLE_OUT_XF = 6, FS_SAMPLE_OUT_X = 7, FS_SAMPLE_OUT_PREP = 8, FS_SAMPLE_OUT_EPOCH = 9,
       FS_SAMPLE_OUT_CODES = 10, FS_SAMPLE_OUT_HID = 11, FS_SAMPLE_OUT_CAP = 12, FS_SAMPLE_OUT_COUNT = 13 };
typedef struct fs_sample_case {
    int32_t family, wt, plan_only, B;
    int32_t F, n_cb, cb_size, n_slow;
    int32_t ld, dim, out_cap, tok_rows;
    int32_t prep, hid, session, cap_frames;
    int32_t batch_rows, batch_row, n_cfg, reserved;
    float eps;
    int32_t reserved2;
    fs_token_cfg tokens;
    int32_t reserved3;
    const fs_sampling* samplings;
    const uint64_t* seeds;
    const int32_t *ignore_eos, *state0;
    const float *tok_emb, *cb_emb, *fast_emb, *prep_g, *x, *logits;
} fs_sample_case;
typedef struct fs_sample_out {
    void* buf[FS_SAMPLE_OUT_COUNT];
    size_t cap[FS_SAMPLE_OUT_COUNT];
    size_t need[FS_SAMPLE_OUT_COUNT];
    int32_t n_launches, guard_ok;
} fs_sample_out;
int fs_selftest_sample_frames(int device_id, const fs_sample_case* c, fs_sample_out* out);

/* Stage tap of the encoder on a LOADED handle: runs fs_codec_encode's device path on the clip exactly as fs_codec_encode does (same buffers,
 * same launches, the codes are computed and dropped) and copies ONE intermediate tensor to the host:
 *   stage -1     the log-mel [160][F], F = mel frames of the clip
 *   stage 0..3   the activation after backbone stage i, [dims[i]][F]
 *   stage 4      after the backbone's final LayerNorm, [C][F]
 *   stage 5, 6   after the first / second downsample block of the quantizer, [C][F / 2] / [C][F / 4]
 *   stage -2     no encoder run (pcm may be null): the handle's regenerated slaney mel filterbank, [1025][160]
 * out receives *n_out floats (cap >= that).  The tap is one device-to-host copy on the handle's stream between two launches of the armed
 * call; an unarmed call (every other entry point) launches nothing more and writes no buffer it did not write before.
 * Diagnostics / parity tests. */
int fs_selftest_codec_encode_stage(fs_codec_t* c, const float* pcm, int n_samples, int stage, float* out, size_t cap, size_t* n_out);

/* Self-test of a LOADED handle, by name.  "persist": the persistent decode kernels of this binary (csrc/lm_persist.hip, lm_persist_slow.hip:
 * pinned weight registers, loads issued outside the compiler's wait-count bookkeeping) against the per-node kernels on the handle's own
 * weights -- 4 greedy frames on the persistent path with the decision capture armed for the first 2, then one teacher-forced per-node step
 * (fs_lm_forward_generate / _fast) compared with the captured logits of the first k_slow_persist step and the first k_fast_persist pass
 * (bound 2e-2 x max(1, max |logit|): loose for summation order, tight for a wrong weight register).  A deployment runs it once after a
 * toolchain change; 0 = passed, the message names the remedy otherwise.  Clears the handle's KV caches.  No reference counterpart. */
int fs_lm_selftest(fs_lm_t* lm, const char* what);
/* Decision capture of the persistent batch-1 decode path (diagnostics / parity tests; no reference counterpart).  After
 * fs_lm_debug_capture(lm, n) every fs_lm_generate call that takes the persistent fast decoder records, for its first n generator
 * iterations, what each of the 9 decisions of a frame saw and chose: fs_lm_debug_read copies f32 [n][9][2048]; row 0 = the slow
 * decision (entries [0, V - im_end): logits over the audio range after the <|im_end|> mask; entry 2047: the picked index), rows
 * 1 + c = codebook c (entries [0, 1024): logits after the repetition penalty; entry 1024: the picked code).  n = 0 switches it off.
 * The parity tests replay these rows through the CPU sampler: same logits, same StdRng stream => same picks, token for token. */
int fs_lm_debug_capture(fs_lm_t* lm, int n_frames);
int fs_lm_debug_read(fs_lm_t* lm, float* out, int n_frames);
/* test hook: the cached K / V rows [t0, t0 + n) of slow layer `layer` of KV slot `slot` (0 for batch-1 calls) as f32 [n][n_local_heads][head_dim]
 * -- the parity tests hand the GPU's own cache entries to the CPU oracle (tests/test_kv_forced_gpu.py) */
int fs_lm_debug_read_kv(fs_lm_t* lm, int slot, int layer, int t0, int n, float* k_out, float* v_out);
/* the same record of request `row` of the last fs_lm_generate_multi call (every request row is captured) */
int fs_lm_debug_read_row(fs_lm_t* lm, int row, float* out, int n_frames);

/* DualARTransformer::load (dual_ar.rs:460-529) is split in create + one of the load calls.
 * max_batch: number of independent sequences (KV caches) the handle can hold (1 for the single-batch generator). */
int fs_lm_create(const fs_model_args* args, const fs_token_cfg* tok, int device_id, fs_dtype dtype, int max_batch,
                 fs_lm_t** out);
void fs_lm_destroy(fs_lm_t* lm);
/* tensors by the reference's names (dual_ar.rs:125-156,219-223,415-419,466-511); bf16 or f32 safetensors */
int fs_lm_load_safetensors(fs_lm_t* lm, const char* path);
/* deterministic synthetic weights at the same names/shapes (spec: csrc/fs_synth.h; no checkpoint exists offline) */
int fs_lm_load_synthetic(fs_lm_t* lm, uint64_t seed);

/* DualARTransformer::forward_generate (dual_ar.rs:574-635).  toks: u32 [B, num_codebooks+1, L].
 * logits_out: f32 [B, vocab_size] or NULL; hidden_out: f32 [B, dim] (PRE-norm hidden of the last position) or NULL.
 * The pad mask argument of the reference is accepted nowhere because the reference ignores it (dual_ar.rs:589-615). */
int fs_lm_forward_generate(fs_lm_t* lm, const uint32_t* toks, int B, int L, int input_pos, float* logits_out,
                           float* hidden_out);
/* DualARTransformer::forward_generate_fast (dual_ar.rs:638-673).  x: f32 [B, dim]; logits_out: f32 [B, codebook_size] */
int fs_lm_forward_generate_fast(fs_lm_t* lm, const float* x, int B, int input_pos, float* logits_out);
/* fast_embeddings.forward (dual_ar.rs:447; used at generate/single_batch.rs:176-182): out f32 [n, dim] */
int fs_lm_fast_embed(fs_lm_t* lm, const uint32_t* ids, int n, float* out);
int fs_lm_clear_fast_layer_caches(fs_lm_t* lm);            /* dual_ar.rs:675-679 */
int fs_lm_clear_slow_layer_caches(fs_lm_t* lm);            /* dual_ar.rs:681-685 */
int fs_lm_clear_slow_caches_until(fs_lm_t* lm, int pos);   /* dual_ar.rs:687-693 (NOT inclusive) */
int fs_lm_curr_kv_size(fs_lm_t* lm);                       /* dual_ar.rs:695-700; < 0 on error */

/* generate_blocking (generate/single_batch.rs:217-324): batch-1 generator, audio_only = true.
 * prompt: u32 [num_codebooks+1, L].  codes_out: u32 [num_codebooks, cap] row-major with row stride `cap`;
 * *n_frames receives the number of frames written (<= cap).  The KV cache is NOT cleared first (the caller
 * owns cache lifetime exactly as with the reference: fish_speech_python/src/lm.rs:94,131-135).
 * seed: seeds the sampler RNG (the reference draws rand::random(), single_batch.rs:46).
 * Extensions / restrictions relative to the reference, stated here so that nobody takes them for parity:
 *   - sampling->top_k == 0 means "no top-k" when temp > 0.  The reference has no such setting: `select_nth_unstable_by(0, ..)` yields an
 *     empty candidate set (candle's single path then fails in WeightedIndex::new, the batch path falls to `unwrap_or(0)`,
 *     sampling/mod.rs:57-75).  With temp == 0 top_k is never looked at (argmax first), there as here.
 *   - both branches of constrain_probs_to_audio / rescale_semantic_tokens are implemented (generate/utils.rs:13-30,45-52): with
 *     im_end_id + 1 == semantic_start_id (Fish 1.5) the slow head reads the contiguous rows [im_end, V); otherwise (generic DualAR token
 *     layout) the candidates are [im_end] ++ [semantic_start, V) -- literally, so control tokens behind the range (<|im_end|> itself
 *     included) stay candidates -- gathered into one head image at load time.  All generation paths take either layout.
 * flags: FS_GEN_IGNORE_EOS masks <|im_end|> (bench-only, fixed-length runs: SURVEY.md §8d).
 *        FS_GEN_NO_PERSIST keeps the whole frame on the per-node graph path.  By default a call on a bf16 or fp8 handle with the Fish geometry
 *        runs a frame as TWO persistent launches (csrc/lm_persist_slow.hip: the 24 slow blocks + head; csrc/lm_persist.hip: the slow-token
 *        decision, the 8 codebook passes with weights resident in VGPRs / LDS and their 8 decisions -- greedy, or top-k / top-p sampled
 *        in-launch when 0 < top_k <= 256 -- with in-launch hand-offs); those launches need all 256 CUs of the device, so only one
 *        generate call per GPU uses them at a time (a concurrent call on another handle silently takes the per-node path). */
#define FS_GEN_IGNORE_EOS 1u
#define FS_GEN_NO_PERSIST 2u
/* measurement mode (bench.py `roofline.kernels`): the two persistent kernels of every decode frame are launched one by one with a HIP event
 * in front of, between and behind them instead of as one graph replay; same kernels, same arguments, same tokens -- only the host paces the
 * frames, so decode_ms of such a call is not a throughput figure.  Ignored when the call does not take both persistent kernels. */
#define FS_GEN_TIME_KERNELS 4u
int fs_lm_generate(fs_lm_t* lm, const uint32_t* prompt, int L, int max_new_tokens, const fs_sampling* sampling,
                   uint64_t seed, uint32_t flags, uint32_t* codes_out, size_t cap, size_t* n_frames, fs_frame_cb cb,
                   void* cb_user);
/* generate_blocking_with_hidden (generate/single_batch.rs:217-306; caller: server/lib/handlers/speech.rs:27-48).
 * hidden_out != NULL <=> collect_hidden_states = true: f32 [hidden_cap, dim] receives the slow transformer's pre-norm hidden state
 * (the `hidden_states` of forward_generate, dual_ar.rs:629-634) of EVERY generator iteration in order -- the first frame, every later
 * frame, and the terminating <|im_end|> iteration whose codes are not emitted (:264-266), so *n_hidden is *n_frames or
 * *n_frames + 1; hidden_cap >= max_new_tokens - L + 2 always suffices.  hidden_out == NULL is fs_lm_generate (the reference
 * returns None). */
int fs_lm_generate_with_hidden(fs_lm_t* lm, const uint32_t* prompt, int L, int max_new_tokens, const fs_sampling* sampling,
                               uint64_t seed, uint32_t flags, uint32_t* codes_out, size_t cap, size_t* n_frames, float* hidden_out,
                               size_t hidden_cap, size_t* n_hidden, fs_frame_cb cb, void* cb_user);

/* generate_static_batch (generate/static_batch.rs:282-390), audio_only = true: n prompts [num_codebooks+1, L_i]
 * (concatenated in `prompts`, lengths in `lens`), left-padded with <|im_end|>/0 as static_batch.rs:68-111,
 * lock-step decode, ragged outputs: codes_out u32 [n, num_codebooks, cap], n_frames[n].
 * bf16 / fp8 handles with n <= min(max_batch, 256): the n sequences are the rows of every GEMM (weights streamed once per step
 * for the whole batch) and the prompts are prefilled as group passes; otherwise (f32 handles, n > 256) the rows are generated
 * one after another on KV slot 0 -- with the BatchedLogitsProcessor semantics of the lock-step path (sampling/mod.rs:77-109: temp <= 1e-7
 * -> first-max argmax; else row b draws sample() call c from the child StdRng seeded with the master's u64 number c * n + b), so the
 * outputs are those of the lock-step batch. */
int fs_lm_generate_batch(fs_lm_t* lm, const uint32_t* prompts, const int* lens, int n, int max_new_tokens,
                         const fs_sampling* sampling, uint64_t seed, uint32_t flags, uint32_t* codes_out, size_t cap,
                         size_t* n_frames);

/* The same call with generate_static_batch's full signature (generate/static_batch.rs:282-390): `audio_only` as an argument and the second
 * return value, `Vec<Vec<bool>>` of BatchPosition::is_audio (:229: slow token >= semantic_start), as is_audio_out u8 [n, cap] (nullable;
 * is_audio_out[i * cap + f] for f < n_frames[i]).  With audio_only = 1 every returned position is audio except a row's FIRST position when its
 * slow token was <|im_end|> (the first position is returned unconditionally, :305-316, with zero codes, :230-233).  audio_only = 0 -- slow
 * token sampled over the full vocabulary, rows never terminate, outputs keep the slow-token row (:132-141,156-173,361-364) -- is NOT
 * implemented and returns an error; the reference's server always passes true (server/lib/handlers/speech.rs:80-86). */
int fs_lm_generate_static_batch(fs_lm_t* lm, const uint32_t* prompts, const int* lens, int n, int max_new_tokens, int audio_only,
                                const fs_sampling* sampling, uint64_t seed, uint32_t flags, uint32_t* codes_out, size_t cap,
                                size_t* n_frames, uint8_t* is_audio_out);

/* R concurrent batch-1 requests on ONE device (round 4; the reference's only multi-request generator is the lock-step static batch,
 * generate/static_batch.rs:117-274, which changes the sampler semantics; its server serialises requests behind one mutex,
 * server/lib/state.rs:12-29).  Request i IS generate_blocking(prompt_i, max_new_tokens[i], samplings[i]) with sampler seed seeds[i] on a
 * cleared cache (generate/single_batch.rs:76-214: its own KV, repetition-penalty window, RNG stream, <|im_end|> / budget rules) -- the
 * tokens of its own fs_lm_generate call (the kernels sum in another order, so greedy tokens may differ where two candidates are within
 * rounding of each other).  prompts: the n prompts u32 [C+1, L_i] concatenated; codes_out u32 [n, C, cap]; n_frames[n].
 * bf16 handles with the Fish 1.5 geometry and token layout, 2 <= n <= min(8, max_batch), and either every request greedy (temp == 0) or
 * every request inside the in-launch sampler (temp > 0, 0 < top_k <= 256: the server default): every decode frame is ONE persistent
 * launch of the slow transformer for all requests (csrc/lm_persist_rows.hip: the weights are streamed once per frame, the requests are
 * matrix-core columns) plus one fast-decoder launch per group of <= 4 requests, each request deciding on its own logits with its own
 * StdRng stream and repetition-penalty window.  Any other handle / sampler mix / n runs the requests one after the other through
 * fs_lm_generate.  The slow KV cache of every slot is cleared first. */
int fs_lm_generate_multi(fs_lm_t* lm, const uint32_t* prompts, const int* lens, int n, const int* max_new_tokens,
                         const fs_sampling* samplings, const uint64_t* seeds, uint32_t flags, uint32_t* codes_out, size_t cap,
                         size_t* n_frames);

/* Capability query for schedulers (fishrt/server.py): *supported = 1 when fs_lm_generate_multi would serve these n requests with these
 * sampler settings on the request-row kernels (one persistent launch group per frame), 0 when it would run them one after the other
 * through fs_lm_generate (handle dtype / token layout / n / sampler mix outside the row kernels) -- in which case a lock-step
 * fs_lm_generate_batch streams the weights once per step for all of them and is the better multi-request path.  Static property of the
 * handle and the settings: it does not look at whether another call currently holds the device's persistent kernels. */
int fs_lm_rows_supported(fs_lm_t* lm, int n, const fs_sampling* samplings, int* supported);

/* ---- replica start-up (no reference counterpart: the reference has no distributed layer).  The handle's device
 * weight arena -- every checkpoint tensor in the handle's storage type, laid out by its tensor plan -- is a pure function of (model args,
 * token config, dtype, checkpoint), so N replicas need ONE checkpoint read: rank 0 loads, fs_lm_weights_arena() gives every rank the
 * device pointer + size to hand to ncclBroadcast (torch.distributed.broadcast: fishrt/fanout.py broadcast_weights), and the receivers
 * call fs_lm_weights_adopt() (marks the handle loaded and builds the load-time derived data: persistent-kernel weight images etc.). */
int fs_lm_weights_arena(fs_lm_t* lm, void** dev_ptr, size_t* bytes);
int fs_lm_weights_adopt(fs_lm_t* lm);

/* ---- replica fan-out over RCCL / xGMI (BASELINE.json north_star: "batch-sharded across the 8 GPUs of one node with
 * RCCL over xGMI only for multi-request fan-out").  No reference counterpart: the reference serves one model behind one mutex
 * (server/lib/state.rs:12-29) and has no distributed layer.  One process per GPU; each holds its own fs_lm_t (full replica) and ONE
 * communicator.  Request i goes to rank i mod world; nothing on the per-token path crosses GPUs, so these are all the collectives there
 * are: (1) the weight arena from the rank that read the checkpoint (ncclBroadcast in 256 MB pieces, then fs_lm_weights_adopt on the
 * receivers), (2) the packed prompt batch, (3) the end-of-run fan-in of the code arrays (ncclAllGather), plus a barrier and small f64
 * reductions for the job's clock and frame counters (ncclAllReduce).  librccl is bound with dlopen at the first call: single-GPU hosts
 * never load it.  Host buffers are caller-owned, as everywhere in this header; calls block until the collective has completed.
 *   bring-up: rank 0 calls fs_comm_unique_id and ships the 128 bytes to the other ranks over the host's own channel (environment,
 *   file, TCP store); every rank then calls fs_comm_create(id, rank, world, device) -- collective, like ncclCommInitRank. */
#define FS_COMM_ID_BYTES 128
typedef struct fs_comm fs_comm_t;
int fs_comm_unique_id(uint8_t id_out[FS_COMM_ID_BYTES]);
int fs_comm_create(const uint8_t id[FS_COMM_ID_BYTES], int rank, int world, int device_id, fs_comm_t** out);
void fs_comm_destroy(fs_comm_t* comm);
int fs_comm_rank(fs_comm_t* comm);   /* -1 on a null handle */
int fs_comm_world(fs_comm_t* comm);
/* every rank enters; returns when all have (an all-reduce of a rank count + the stream sync behind it) */
int fs_comm_barrier(fs_comm_t* comm);
/* in place on a host array of n <= 4096 doubles; op: 0 sum, 1 max, 2 min (the job's wall time is the MAX over ranks, its frames the SUM) */
int fs_comm_all_reduce_f64(fs_comm_t* comm, double* vals, int n, int op);
/* (1) `lm` on rank `src` is loaded; on every other rank it was created with the same model args / token config / dtype and is NOT loaded:
 * after the call every rank's handle is ready (receivers ran fs_lm_weights_adopt).  Arena sizes are compared across ranks first; a
 * mismatch is an error on EVERY rank before a byte moves.  *bytes_moved (nullable) = the arena size. */
int fs_comm_broadcast_weights(fs_comm_t* comm, fs_lm_t* lm, int src, size_t* bytes_moved);
/* (2) the packed prompt batch: dims = {n_requests, num_codebooks + 1, Lmax}; packed u32 [n_requests][C+1][Lmax] (rows left-aligned,
 * zero-padded), lens i32 [n_requests].  Receivers first learn the shape (fs_comm_broadcast_prompt_dims fills dims from rank src), size
 * their buffers, then every rank calls fs_comm_broadcast_prompts with the same dims. */
int fs_comm_broadcast_prompt_dims(fs_comm_t* comm, int64_t dims[3], int src);
int fs_comm_broadcast_prompts(fs_comm_t* comm, uint32_t* packed, int32_t* lens, const int64_t dims[3], int src);
/* (3) fan-in: this rank's codes u32 [B][C][N] (its requests, padded to N frames) and n_frames i32 [B] -> on EVERY rank
 * codes_all u32 [world][B][C][N] and n_frames_all i32 [world][B].  B, C, N must be the same on every rank (pad the last shard). */
int fs_comm_all_gather_codes(fs_comm_t* comm, const uint32_t* codes, const int32_t* n_frames, int B, int C, int N, uint32_t* codes_all,
                             int32_t* n_frames_all);

/* ---- continuous batching (no reference counterpart: the reference server serialises requests behind one mutex, server/lib/state.rs:12-29,
 * or runs lock-step batches, generate/static_batch.rs:282-390; SURVEY.md section 8 f-4 asks for a scheduler that replaces the mutex).
 * A session turns the max_batch rows of the static-batch decode step into independent request SLOTS: a request's prompt is prefilled on
 * the matrix-core row path on a second stream while the other slots keep stepping, it joins between two steps once that has finished,
 * and leaves when done; every step streams the weights once for all live slots.  A slot behaves exactly like row 0 of a ONE-prompt fs_lm_generate_batch call: no left padding (own positions
 * and KV pages), first frame emitted unconditionally, BatchedLogitsProcessor sampling (sampling/mod.rs:77-109; repetition penalty is
 * ignored like static_batch.rs:204-206), 1 + max(0, max_new_tokens - L + 1) iterations (static_batch.rs:122), stopping early at
 * <|im_end|> or at max_seq_len.  With temp <= 1e-7 a slot's codes are independent of what the other slots do.
 * bf16 / fp8 handles; while a session is open the handle's other entry points fail.
 * Which session kind takes which token layout: plain sessions (no flag) and FS_SESSION_ROWS sessions need the Fish 1.5 / DualAR layout
 * (has_semantic_end != 0: the slow token is sampled over the audio range); a Fish <= 1.4 handle (has_semantic_end == 0: the slow token is
 * the 2-way {pad, im_end} draw) takes FS_SESSION_PER_SLOT sessions only -- the other two kinds fail with an error that says so. */
/* FS_SESSION_ROWS (round 4): the slots run on the request-row persistent kernels (csrc/lm_persist_rows.hip, see fs_lm_generate_multi) and keep
 * BATCH-1 semantics: a slot is its own generate_blocking call -- repetition penalty applied, LogitsProcessor sampling on its own StdRng stream
 * seeded `seed + the slot's admission number`, 1 + max(0, max_new_tokens - L + 1) iterations -- while requests join and leave between
 * frames; a decode frame costs one slow launch for all slots + one fast launch per 4 slots instead of the 373-node step.  bf16 Fish-1.5
 * handles with 2 <= max_batch <= 8, greedy or 0 < top_k <= 256; the device's persistent kernels are held for the session's lifetime. */
#define FS_SESSION_ROWS 8u
/* FS_SESSION_PER_SLOT: what a slot samples depends on the REQUEST, not on the session, at every max_batch and on every handle type
 * sessions take (bf16 / fp8, Fish 1.5 AND Fish <= 1.4 token layouts, max_batch <= 256).  The session runs on the static-batch step exactly as without the
 * flag -- same GEMM / attention nodes, prefill, paging, prefixes, poll / release / info, slot lifetime (1 + max(0, max_new_tokens - L + 1)
 * iterations, frame 0 emitted unconditionally, stop at <|im_end|> / budget / max_seq_len, FS_GEN_IGNORE_EOS) -- but each of a frame's 9
 * decisions is that of the slot's OWN fs_lm_generate call (generate/single_batch.rs:102-210, sampling/mod.rs:51-75, rep_pen.rs:4-72):
 *   - one StdRng stream per slot, seeded when the slot is activated, words consumed in decision order (slow, c0..c7 per frame);
 *   - repetition penalty per codebook: the 16-deep window and mask of the reference's RepPenState, applied from the slot's second frame
 *     on, logits divided by the mask whatever their sign, reset when a slot is (re)activated;
 *   - LogitsProcessor rules: greedy iff temp == 0 with the batch-1 tie rule (the last maximal index), top-p compared in f32, and when the
 *     slow token is <|im_end|> the codebook decisions are skipped (codes 0) and draw nothing;
 *   - the slot's own settings and seed (fs_lm_session_add_ex), else the session's settings and `seed + the slot's admission number`;
 *   - Fish <= 1.4 handles (has_semantic_end == 0): the slow decision is fs_lm_generate's legacy one (sampling/mod.rs:8-26,
 *     single_batch.rs:104-124): p_pad = softmax([pad logit, im_end logit])[0] in f32, u = (word >> 8) * 2^-24, token = pad_id when
 *     u < p_pad or under FS_GEN_IGNORE_EOS, else im_end_id.  It takes ONE stream word per live frame at every temperature, also when the
 *     slot is greedy (temp == 0); the codebook decisions and the next input's embedding (codebook embeddings only under the pad /
 *     <|semantic|> token) follow the rules above.  fs_lm_debug_capture records that decision as the batch-1 path does: entry 0 the pad
 *     logit, 1 the im_end logit, 2 the draw u, 2047 the picked index (0 pad, 1 im_end).
 * So a slot's codes do not depend on its slot index, on max_batch or on what the other slots do; against its own fs_lm_generate call
 * they can differ only where two candidates are within rounding of each other (the row path and the batch-1 kernels sum in different
 * orders).  Settings accepted per slot and for the session: greedy (temp == 0), or temp > 0 with 0 < top_k <= 256 -- the limit of the
 * in-launch samplers (see fs_lm_generate); anything else is an error from fs_lm_session_begin / fs_lm_session_add_ex, never another
 * sampler.  About 40 KB of device memory per slot; the step has as many graph nodes as the lock-step one (one fewer when sampling).
 * FS_SESSION_PER_SLOT | FS_SESSION_ROWS is an error.  fs_lm_debug_capture records the head's RAW logits (before the penalty; <|im_end|>
 * masked under FS_GEN_IGNORE_EOS) and the picks of every slot, readable with fs_lm_debug_read_row(slot). */
#define FS_SESSION_PER_SLOT 16u
/* FS_SESSION_WIDE_SAMPLER: valid only together with FS_SESSION_PER_SLOT (alone, or with FS_SESSION_ROWS, fs_lm_session_begin fails and
 * says so).  It lifts the sampling limit of a per-slot session: the session's own setting and every fs_lm_session_add_ex /
 * fs_lm_session_add_hidden setting may be greedy (temp == 0), or ANY temp > 0 with ANY top_k >= 0 and ANY finite top_p -- top_k == 0 (no
 * top-k: nucleus-only, what upstream Fish-Speech samples with) and top_k > 256 included; temp < 0 or a non-finite temp / top_p is an error
 * that names the field.  Per decision over n candidates (n = the audio range for the slow token, codebook_size for a codebook) the rule is
 * LogitsProcessor's (sampling/mod.rs:51-75): top_k == 0 or top_k >= n is nucleus-only (descending stable order, the lower index first on
 * ties; entries zeroed once the sequential f32 running sum has reached top_p; the WeightedIndex draw over all n weights in index order);
 * otherwise the top_k largest in ascending index order, their sequential f32 sum, the top-p cut only if 0 < top_p < sum, then the draw.  So
 * one slot can be top-k on the slow decision and nucleus-only on the codebooks (top_k = 1500 on Fish 1.5: n = 2037 and 1024).  Decisions
 * with 0 < top_k <= 256 < n and greedy ones run the same code as without the flag and give the same codes, bit for bit; the others run a
 * block-wide general sampler inside the same sampler nodes (no extra graph nodes, no device memory per slot; tens of microseconds more
 * per such decision).  Everything else FS_SESSION_PER_SLOT promises holds as written: one StdRng stream per slot with words consumed in
 * decision order, the repetition-penalty window, the last-max greedy rule, top-p compared in f32, no codebook decisions after <|im_end|>,
 * the legacy 2-way slow draw on Fish <= 1.4 handles, the capture record; the handle limits stay (<= 2048 slow candidates, codebooks of
 * <= 1024 entries).  Sessions begun without the flag are unchanged: same kernels, same errors, same codes. */
#define FS_SESSION_WIDE_SAMPLER 32u
/* FS_SESSION_SCORE: valid only together with FS_SESSION_PER_SLOT, with or without FS_SESSION_WIDE_SAMPLER (alone, with FS_SESSION_ROWS, or
 * on a Fish <= 1.4 handle -- has_semantic_end == 0 -- fs_lm_session_begin fails and says which; num_codebooks must be 8).  The session
 * additionally takes SCORING slots (fs_lm_session_add_scored): slots that are not sampled but forced along a given code sequence, and that
 * record how likely the model found every one of its tokens.  A scoring slot rides the same step as the generating slots next to it --
 * the weights are streamed once per step for all of them -- and uses the same prefill, paging, shared prefixes, prefix blobs and
 * hidden-state collection.  The step graphs of such a session carry one small node (k_score_slots, one block per slot) in front of each
 * of the 9 per-slot sampler nodes and behind fs_lm_debug_capture's record of the raw row; it reads a per-slot table, so admitting or
 * releasing a scoring slot never re-captures a graph, and for a generating slot it exits at once: every generating slot's codes are bit
 * for bit those of the same session without the flag.  Sessions begun without the flag replay exactly the graphs they did before. */
#define FS_SESSION_SCORE 64u
/* FS_SESSION_TRACE: valid only together with FS_SESSION_PER_SLOT | FS_SESSION_SCORE, with or without FS_SESSION_WIDE_SAMPLER (alone, with
 * FS_SESSION_ROWS, without FS_SESSION_SCORE, or on a Fish <= 1.4 handle fs_lm_session_begin fails and says which).  The session
 * additionally takes TRACED slots (fs_lm_session_add_traced): slots that generate like any other and leave the scoring slots' record for
 * the tokens they PICKED, so that the log-probs of a generated sequence need no second, teacher-forced pass.  The score nodes of the step
 * take a second path for such a slot (they keep the raw row and its normaliser, and leave the row as it is), and ONE more node per step
 * (k_trace_commit, one block per slot) behind the frame's last sampler node reads the picks and closes the record row.  Both read the
 * per-slot table, so one captured graph serves every mix of traced, scoring and plain slots and no add or release re-captures; plain,
 * scoring and collecting slots of such a session produce bit for bit what they produce without the flag.  The step graphs get one more
 * key bit: sessions begun without the flag -- FS_SESSION_SCORE sessions too -- replay exactly the graphs they did before.
 * Device memory: 4 (32 + 9 * 2048) bytes (72.1 KB) of stash per slot of the handle, allocated once at the first such session. */
#define FS_SESSION_TRACE 128u
int fs_lm_session_begin(fs_lm_t* lm, const fs_sampling* sampling, uint64_t seed, uint32_t flags /* FS_GEN_IGNORE_EOS | FS_SESSION_ROWS | FS_SESSION_PER_SLOT | FS_SESSION_WIDE_SAMPLER | FS_SESSION_SCORE | FS_SESSION_TRACE */);
/* prompt u32 [C+1, L] row-major (copied); *slot = the slot taken, or -1 when all max_batch slots are busy or the KV page pool cannot hold
 * the request right now (not an error: retry after a release).  Returns once the
 * prefill is enqueued (one prefill in flight: a second add first waits for the previous one); the slot starts generating in a later step */
int fs_lm_session_add(fs_lm_t* lm, const uint32_t* prompt, int L, int max_new_tokens, int* slot);
/* run up to n_frames decode steps for all live slots (stops early when none is live); *n_active = slots still generating afterwards */
int fs_lm_session_step(fs_lm_t* lm, int n_frames, int* n_active);
/* frames of `slot` so far: codes_out u32 [C, cap] row-major (may be NULL to query only), *n_frames, *done = 1 once the slot has finished */
int fs_lm_session_poll(fs_lm_t* lm, int slot, uint32_t* codes_out, size_t cap, size_t* n_frames, int* done);
/* give the slot (and its KV pages) back */
int fs_lm_session_release(fs_lm_t* lm, int slot);
int fs_lm_session_end(fs_lm_t* lm);
/* Shared conditioning prefixes: the KV of a prompt prefix (system text + voice prompt) is prefilled ONCE into pages owned by the session,
 * and any number of slots admitted with fs_lm_session_add_prefixed point their page tables at its full pages (reference counted; nothing
 * writes a page with more than one owner) and get a private copy of its partly filled last page; only their own body is prefilled.
 * A prefix lives until fs_lm_session_prefix_release or fs_lm_session_end, whichever comes first.
 * Prefill prompt u32 [C+1, P] (P >= 1; all P positions get K/V) into pages owned by the session; *prefix_id >= 0, or -1 when the KV page
 * pool cannot hold it right now (not an error, like fs_lm_session_add).  Queued on the prefill stream like an add. */
int fs_lm_session_prefix_create(fs_lm_t* lm, const uint32_t* prompt, int P, int* prefix_id);
/* drop the session's reference; the pages return to the pool when the last slot that uses them is released */
int fs_lm_session_prefix_release(fs_lm_t* lm, int prefix_id);
/* == fs_lm_session_add(lm, concat(prefix prompt, body), P + L_body, max_new_tokens, slot) in every respect (iteration count from
 * L = P + L_body, max_seq_len rule, admission number -> rows-mode sampler seed, frame-0 rule, EOS, budget), except that only the
 * L_body - 1 body positions are prefilled.  body u32 [C+1, L_body], L_body >= 1. */
int fs_lm_session_add_prefixed(fs_lm_t* lm, int prefix_id, const uint32_t* body, int L_body, int max_new_tokens, int* slot);
/* An add whose slot samples with its own settings and / or sampler seed.  prefix_id < 0: `prompt` u32 [C+1, L] is the whole prompt
 * (== fs_lm_session_add); prefix_id >= 0: it is the body on that prefix (== fs_lm_session_add_prefixed).  sampling NULL: the session's
 * settings; seed NULL: session seed + the slot's admission number.  With both NULL this is exactly the plain call, in every session.
 *   FS_SESSION_PER_SLOT sessions: any settings inside the limit stated there (else an error that names it); with
 *     FS_SESSION_WIDE_SAMPLER: greedy, or any temp > 0 with any top_k and any finite top_p.
 *   FS_SESSION_ROWS sessions: the row kernels read one setting and one stream per row already; the slot's settings must stay inside what
 *     fs_lm_rows_supported accepts together with the session's (all greedy or all sampled with 0 < top_k <= 256), else an error.
 *   plain sessions: a non-NULL sampling or seed is an error -- the lock-step sampler has no per-slot notion and keeps its outputs.
 * A slot admitted with a seed of its own is prefilled in a pass of its own (a group pass of several joining prompts rounds differently
 * from a single one), so its codes are a function of (prompt, budget, settings, seed) alone -- not of what was queued with it.
 * *slot = -1 when no slot / KV pages are free right now, as fs_lm_session_add. */
int fs_lm_session_add_ex(fs_lm_t* lm, int prefix_id, const uint32_t* prompt, int L, int max_new_tokens, const fs_sampling* sampling,
                         const uint64_t* seed, int* slot);
/* Hidden states of a session slot (the reference's server/lib/handlers/send_hidden_states.rs calls generate_blocking_with_hidden with
 * collect_hidden_states = true; fs_lm_generate_with_hidden is that call at batch 1).  fs_lm_session_add_hidden IS fs_lm_session_add_ex in
 * every respect -- prefix_id / sampling / seed rules per session kind, *slot = -1 when nothing is free, the slot's codes bit for bit --
 * and the slot additionally keeps the slow transformer's pre-norm hidden state (the `hidden_states` of forward_generate, dual_ar.rs:629-634:
 * the row the head's RMSNorm reads and the fast decoder starts from) of every generator iteration it runs.  Valid in plain,
 * FS_SESSION_PER_SLOT and FS_SESSION_ROWS sessions; collecting and non-collecting slots mix freely and run the same step (a small kernel
 * behind the slow head reads a per-slot pointer table, so admitting or releasing a collector never re-captures the step graph).
 * Device memory: one f32 [1 + max(0, max_new_tokens - L + 1)][dim] buffer per collecting slot (iterations clipped by max_seq_len as for
 * the add), taken from a per-handle pool when the slot is admitted and returned at fs_lm_session_release / fs_lm_session_end; nothing is
 * allocated for slots that do not collect.
 * fs_lm_session_poll_hidden: *n_rows (nullable) = rows the slot has so far; hidden_out (NULL: query only) f32 [cap_rows, dim] receives rows
 * [first_row, min(*n_rows, first_row + cap_rows)).  Row count rule == the *n_hidden rule of fs_lm_generate_with_hidden: one row per
 * iteration the slot ran, in order, row 0 being the iteration over the last prompt position (whose frame is emitted unconditionally) and
 * the terminating <|im_end|> iteration, whose frame is not emitted, included -- so *n_rows is the slot's n_frames or n_frames + 1.  A
 * slot still prefilling has 0 rows; a released and re-admitted slot starts again at row 0.  A slot that was not admitted with
 * fs_lm_session_add_hidden is an error that says so. */
int fs_lm_session_add_hidden(fs_lm_t* lm, int prefix_id, const uint32_t* prompt, int L, int max_new_tokens, const fs_sampling* sampling,
                             const uint64_t* seed, int* slot);
int fs_lm_session_poll_hidden(fs_lm_t* lm, int slot, size_t first_row, float* hidden_out, size_t cap_rows, size_t* n_rows);
/* Scoring slots (FS_SESSION_SCORE sessions; both calls fail with "needs FS_SESSION_SCORE" in any other).
 * A slot that is NOT sampled: iteration i (0-based) of the slot is forced to frames[:, i] -- frames u32 [C+1, N] row-major like a prompt
 * (row 0 the slow token, rows 1..C the codes), N >= 1 -- and records what the model thought of it.  Otherwise == fs_lm_session_add_ex
 * (prefix_id rules, *slot = -1 when no slot / pages are free, prefill in a pass of its own like a slot with its own seed) with
 * max_new_tokens = L + N - 2, i.e. exactly N iterations.  Validated before anything is queued, each an error naming the field and
 * leaving the session as it was: every frames[0][i] in [semantic_start_id, vocab_size), every code < codebook_size, and
 * L_total + N - 1 <= max_seq_len (L_total = L plus the prefix's length; a scored sequence is never clipped).  The slot emits
 * frames[1..C] as its codes (fs_lm_session_poll), draws no stream words, and never ends early.  collect_hidden != 0: also
 * fs_lm_session_add_hidden's rows (fs_lm_session_poll_hidden).
 * Per decision d of an iteration (0 = the slow token over the audio range, <|im_end|> at candidate 0 left out under FS_GEN_IGNORE_EOS;
 * 1 + c = codebook c over codebook_size entries) the record is taken from the RAW row the slot's sampler would have decided on -- no
 * temperature, no repetition penalty, no top-k / top-p -- in f32: m = max x_i, s = sum exp(x_i - m),
 *     logprob[d] = (x_target - m) - log(s)      top_logprob[d] = -log(s)      top[d] = the LAST index holding m (-0 == +0)
 * and eos_logprob = (x_0 - m) - log(s) of the slow decision (-inf when <|im_end|> is left out).  An f32 sum of <= 2048 non-negative terms:
 * within 2e-4 absolute of the exact log-softmax of the row.  Then the node stores +inf over the target's logit and the slot's own greedy
 * sampler node, unchanged, picks it and does the frame bookkeeping as for any slot.
 * Device memory: 128 + 4 (C + 1) bytes per iteration, one buffer per scoring slot from a per-handle pool (taken at the add, returned when
 * the add is refused, at fs_lm_session_release and at fs_lm_session_end). */
int fs_lm_session_add_scored(fs_lm_t* lm, int prefix_id, const uint32_t* prompt, int L, const uint32_t* frames, int N, int collect_hidden,
                             int* slot);
/* rows [first_row, ...) so far, one per iteration: logprob / top_logprob f32 [cap_rows][C+1], top u32 [cap_rows][C+1],
 * eos_logprob f32 [cap_rows]; every output pointer nullable; *n_rows = rows the slot has (0 while prefilling; a released and re-admitted
 * slot starts again at row 0).  A slot not admitted with fs_lm_session_add_scored is an error that says so. */
int fs_lm_session_poll_scores(fs_lm_t* lm, int slot, size_t first_row, float* logprob, float* top_logprob, uint32_t* top, float* eos_logprob,
                              size_t cap_rows, size_t* n_rows);
/* Traced slots (FS_SESSION_TRACE sessions; both calls fail with "needs FS_SESSION_TRACE" in any other).
 * fs_lm_session_add_traced IS fs_lm_session_add_ex in every respect -- prefix_id / sampling / seed rules, *slot = -1 when nothing is free,
 * the slot's codes bit for bit; any setting the session accepts: greedy, narrow, and wide in a FS_SESSION_WIDE_SAMPLER session -- and with
 * collect_hidden != 0 it is fs_lm_session_add_hidden.  Like a slot with a seed of its own it is prefilled in a pass of its own, so its
 * records are a function of the request alone.  Additionally the slot keeps one record row per generator iteration it runs, in order,
 * the terminating <|im_end|> iteration included (the *n_hidden rule: *n_rows is the slot's n_frames or n_frames + 1; 0 while it is
 * prefilling; a released and re-admitted slot starts again at row 0).
 * The record of decision d (0 = the slow token over the audio range, candidate 0 = <|im_end|> left out under FS_GEN_IGNORE_EOS; 1 + c =
 * codebook c) is the scoring slots' record (fs_lm_session_add_scored) taken AT THE PICK: f32, from the RAW row -- no temperature, no
 * repetition penalty, no top-k / top-p -- m = max x_i, s = sum exp(x_i - m),
 *     logprob[d] = (x_pick - m) - log(s)      top_logprob[d] = -log(s)      top[d] = the LAST index holding m
 * eos_logprob = the slow row's candidate 0 (-inf when left out); tokens[.][0] = the slow token id as it goes into the next input column
 * (<|im_end|>'s id on the terminating iteration), tokens[.][1 + c] = the code; n_decisions = C + 1, or 1 for an iteration whose slow pick
 * was <|im_end|> -- its codebook decisions are skipped: logprob = top_logprob = NaN, top = 0xFFFFFFFF, tokens = 0 there.  So a row equals,
 * field for field and bit for bit, what fs_lm_session_add_scored records when the same sequence is fed back.
 * Device memory: 128 + 4 (C + 1) bytes per iteration (the record and the token row: a scoring slot's buffer, from the same per-handle
 * pool -- taken at the add, returned when the add is refused, at fs_lm_session_release and at fs_lm_session_end), plus the slot's stash
 * (FS_SESSION_TRACE). */
int fs_lm_session_add_traced(fs_lm_t* lm, int prefix_id, const uint32_t* prompt, int L, int max_new_tokens, const fs_sampling* sampling,
                             const uint64_t* seed, int collect_hidden, int* slot);
/* rows [first_row, ...) so far: tokens u32 / logprob f32 / top_logprob f32 / top u32 [cap_rows][C+1], eos_logprob f32 [cap_rows],
 * n_decisions i32 [cap_rows]; every output pointer nullable; *n_rows = rows the slot has.  A slot not admitted with
 * fs_lm_session_add_traced is an error that says so (and fs_lm_session_poll_scores refuses a traced slot). */
int fs_lm_session_poll_trace(fs_lm_t* lm, int slot, size_t first_row, uint32_t* tokens, float* logprob, float* top_logprob, uint32_t* top,
                             float* eos_logprob, int* n_decisions, size_t cap_rows, size_t* n_rows);
/* FS_SESSION_ALTS (a flag of fs_lm_session_begin): valid only together with FS_SESSION_PER_SLOT | FS_SESSION_SCORE, with or without
 * FS_SESSION_WIDE_SAMPLER and FS_SESSION_TRACE (alone, with FS_SESSION_ROWS, without FS_SESSION_SCORE, or on a Fish <= 1.4 handle
 * fs_lm_session_begin fails and says which).  Every scoring and every traced slot of such a session additionally records, per iteration
 * and decision d (0 = the slow token, 1 + c = codebook c), the N most likely candidates with their log-probs and the entropy of the
 * decision -- OpenAI's top_logprobs, what a distillation consumes, and a confidence figure -- without the host copy of whole rows that
 * fs_lm_debug_capture makes.  N = FS_SESSION_ALTS_N(n), a 5-bit field of the flags: 1 .. FS_ALTS_MAX, 0 = the default of 8; a value
 * above 16, or a non-zero field without FS_SESSION_ALTS, is an error that names it.
 * The score nodes of the session are a second instantiation of k_score_slots (same launch shape, one more barrier, N a launch argument);
 * sessions begun without the flag replay exactly the graphs they did before, and plain, collecting, scoring and traced slots of an
 * FS_SESSION_ALTS session produce bit for bit the codes and records they produce without it.
 *   Candidates: those of the existing record -- under FS_GEN_IGNORE_EOS candidate 0 of the slow decision takes no part and never appears --
 *     from the RAW row: no temperature, no repetition penalty, no top-k / top-p.
 *   Order: the score node's own 64-bit key -- value descending, -0 == +0, among equal values the HIGHER index first -- so
 *     alt_index[d][0] == top[d] and alt_logprob[d][0] == top_logprob[d].  Slow-decision indices are candidate indices, as `top` is
 *     (0 = <|im_end|>).
 *   alt_logprob = (x - m) - log(s) in f32, the very expression of logprob[d]: bit-identical to it whenever the forced or picked token is
 *     among the alternatives (within 2e-4 of the exact log-softmax, as there).  Candidates holding -inf rank last, with log-prob -inf.
 *     With fewer than N candidates the tail is padded: index 0xFFFFFFFF, log-prob NaN.
 *   entropy[d] = log(s) - (sum_i exp(x_i - m) (x_i - m)) / s in f32 over the candidates with finite x_i (a -inf entry contributes exactly
 *     0): within 2.5e-3 absolute of the exact entropy of the row (two f32 sums of <= 2048 same-signed terms, a ratio of at most log 2048).
 *   On the <|im_end|> iteration of a traced slot the skipped codebook decisions hold index 0xFFFFFFFF, log-prob NaN and entropy NaN.
 *   A traced slot's alternatives and entropies are, field for field and bit for bit, those of fs_lm_session_add_scored fed the same tokens
 *     (a scoring slot's are taken before +inf goes over the target).
 * Device memory: 9 (8 N + 4) more bytes per iteration of a scoring or traced slot, behind its records in the same buffer (the per-handle
 * pool is emptied when a session's row size differs from the previous one's). */
#define FS_SESSION_ALTS 256u
#define FS_SESSION_ALTS_N(n) ((uint32_t)(n) << 16)
#define FS_ALTS_MAX 16u
/* rows [first_row, ...) so far of a scoring or a traced slot: alt_index u32 / alt_logprob f32 [cap_rows][C+1][N], entropy f32
 * [cap_rows][C+1]; every output pointer nullable; *n_rows = rows the slot has (the rule of fs_lm_session_poll_scores / _poll_trace),
 * *n_alts = the session's N.  A slot that is neither, or a session without the flag ("needs FS_SESSION_ALTS"), is an error. */
int fs_lm_session_poll_alts(fs_lm_t* lm, int slot, size_t first_row, uint32_t* alt_index, float* alt_logprob, float* entropy, size_t cap_rows,
                            size_t* n_rows, int* n_alts);
/* out[8] = {free pages, pages referenced by more than one owner, live prefixes, prefill passes, tokens prefilled,
 *           prefix tokens reused, tail pages copied, prefill-stream microseconds (HIP events around each pass)};
 * counters since fs_lm_session_begin */
int fs_lm_session_info(fs_lm_t* lm, int64_t out[8]);

/* ---- prefix KV blobs (no reference counterpart).  The K/V rows of a shared prefix are a pure function of (weights, KV storage type, prefix
 * tokens): fs_lm_session_prefix_export hands them out as bytes, fs_lm_session_prefix_import puts them back into pages of any later
 * session -- of this handle or of another one with the same weights -- without running the slow transformer.
 * A blob is one 64-byte header followed by the payload; everything little-endian.
 * Payload: the KV elements (kv_dtype) as [n_layer][2 (K, then V)][P][n_local_heads][head_dim], position-major: exactly the P rows, nothing
 * of the unused part of the last page, and nothing that depends on the page size, max_batch, the pool size or the session kind.  K is
 * stored as the cache holds it: AFTER RoPE, at the absolute positions 0 .. P-1; a prefix always starts at position 0, so the rows are
 * reusable as they are.  No payload checksum: callers that persist blobs wrap their own. */
typedef struct fs_kv_blob_header {
    char magic[8];                 /* "FSKVPFX1" */
    uint32_t version;              /* 1 */
    uint32_t kv_dtype;             /* fs_dtype of the KV storage: FS_BF16 on every handle that takes sessions */
    int32_t n_layer, n_local_heads, head_dim, P;
    uint32_t header_bytes;         /* 64 */
    uint32_t reserved;             /* 0 */
    uint64_t weights_fingerprint;  /* fs_lm_weights_fingerprint of the exporting handle */
    uint64_t payload_bytes;        /* n_layer * 2 * P * n_local_heads * head_dim * sizeof(element) */
    uint64_t reserved2;            /* 0 */
} fs_kv_blob_header;
/* 64-bit fingerprint of the handle's weight arena (fs_lm_weights_arena: n bytes = n / 4 little-endian 32-bit words w[0 .. n/4)), integer
 * arithmetic only, all of it mod 2^64:
 *     S = sum_i w[i] * (2 i + 1)
 *     z = S ^ ((n / 4) * 0x9E3779B97F4A7C15);  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
 *     fingerprint = z ^ (z >> 31)
 * S is a sum of integers, so it is bit-identical for any grid size and any order of the device's atomic adds; the weights 2 i + 1 are
 * odd and distinct, so S changes when two unequal words swap places ((w[a] - w[b]) * 2 (a - b) != 0 mod 2^64 for arenas below 2^32 words);
 * the last three lines are a bijection (the splitmix64 finaliser).  Computed on the device at the first call that needs it (this one, an
 * export or an import), cached per handle, invalidated by fs_lm_load_* and fs_lm_weights_adopt.  A bf16 and an fp8 handle of the same
 * checkpoint have different arenas, hence different fingerprints -- and different K/V. */
int fs_lm_weights_fingerprint(fs_lm_t* lm, uint64_t* out);
/* The blob of live prefix `prefix_id` of the open session: *bytes (nullable) = 64 + payload_bytes; blob_out NULL queries the size only,
 * cap < *bytes is an error.  If the prefix's own pass (creation or import) is still queued or in flight the call first lets it finish and
 * activates it, as fs_lm_session_step would.  The rows are gathered on the prefill stream into the handle's staging buffer and copied to
 * blob_out; the call returns once the bytes are there.  It does not touch the decode stream, any slot's codes, any page reference or any
 * counter of fs_lm_session_info.  Valid in every session kind, on bf16 and fp8 handles.
 * Staging: ONE grow-only device buffer per handle, freed with the handle; its size is the largest payload moved so far -- one export's
 * payload, or the summed payloads of the imports launched as one pass. */
int fs_lm_session_prefix_export(fs_lm_t* lm, int prefix_id, void* blob_out, size_t cap, size_t* bytes);
/* A prefix from a blob.  The whole header is validated before any page is taken and before any byte moves; each of these is an error
 * that names the field and leaves the pool as it was: magic, version, header_bytes, bytes == 64 + payload_bytes, kv_dtype, n_layer /
 * n_local_heads / head_dim against the handle, 1 <= P < max_seq_len, payload_bytes against the dimensions, weights_fingerprint against the
 * handle's.  Then the call behaves like fs_lm_session_prefix_create: the ceil(P / 64) pages are taken now, *prefix_id = -1 (not an
 * error) when the pool cannot hold them right now, and the prefix is the same object afterwards -- fs_lm_session_add_prefixed, the shared
 * full pages, the copied last page, release, fs_lm_session_end and fs_lm_session_info treat it as a created one.  The payload is copied
 * before the call returns (the caller may free the blob at once); the host-to-device copy and the scatter into the pages are queued on
 * the prefill stream as a pass of their own, ahead of every creation and every add queued with them, and activated through the same
 * event as a creating pass -- so an add with a one-column body on it, which prefills nothing, cannot go live before the rows are in
 * place.  No slow-transformer pass runs: the prefill passes / tokens prefilled counters of fs_lm_session_info do not move.
 * Blobs are portable between session kinds and between handles with equal fingerprints. */
int fs_lm_session_prefix_import(fs_lm_t* lm, const void* blob, size_t bytes, int* prefix_id);

/* ---- prefixes from a slot's history (no reference counterpart): multi-turn continuity, forks, "this voice, having said this".
 * fs_lm_session_prefix_from_slot makes a session prefix out of the first P cached positions of `slot` -- K/V rows the slot's prefill and
 * its DECODE steps wrote -- without running anything through the slow transformer.  The result is an ordinary prefix:
 * fs_lm_session_add_prefixed / _add_ex / _add_hidden / _add_scored / _add_traced on it, fs_lm_session_prefix_export, _prefix_release,
 * fs_lm_session_end and fs_lm_session_info treat it exactly as a created one.  The source slot is unchanged: it keeps generating if it
 * is live, keeps its frames and records, is released by its caller as before, and its later codes are bit for bit what they would have
 * been without the call.
 * How many positions are history: with L the slot's total prompt length (its prefix included) and n the frames it has emitted so far
 * (fs_lm_session_poll's *n_frames; 0 before its first step) the slot has T = L + n - 1 positions to give, in every state -- live,
 * finished on its budget, finished on <|im_end|>.  The column of the last emitted frame is never part of them: a live slot feeds it with
 * its next step, a slot finished on its budget never fed it, and a slot frozen by <|im_end|> (or dead at frame 0) keeps rewriting row T
 * with the <|im_end|> column while it rides the step.  Rows [0, T) are never written again by anyone.
 * n_positions == -1: P = T.  Otherwise 1 <= n_positions <= T and P = n_positions: a cut may lie inside the prompt or at any frame.
 * P < max_seq_len, as for every prefix (it must leave room for a body).  *P_out (nullable) = P.
 * Pages: the prefix takes one more reference on the slot's first P / 64 pages (also on pages the slot itself shares from another prefix:
 * chains of turns keep sharing) and, when P % 64 != 0, ONE new page from the pool, into which the slot's page P / 64 is copied
 * (k_kv_page_copy; rows [64 (P / 64), P) are the ones that count) on the decode stream, behind every step already enqueued; the call
 * returns when the copy is done, so it is ahead of any add on the prefix.  It counts in `tail pages copied`; no other counter of
 * fs_lm_session_info moves (no prefill pass, no tokens prefilled).  When that page is not free right now *prefix_id = -1 and nothing has
 * changed (not an error, as fs_lm_session_prefix_create); with P % 64 == 0 no page is taken and the call cannot be refused for room.
 * Everything from page T / 64 on stays the slot's alone, so the single-writer rule holds for a live and for a frozen source.
 * A slot still prefilling is first let finish and activated, as fs_lm_session_release does.
 * Valid in plain and FS_SESSION_PER_SLOT sessions with any of the WIDE / SCORE / TRACE / ALTS flags, on bf16 and fp8 handles, Fish 1.5 and
 * Fish <= 1.4 token layouts, for plain, collecting, scoring and traced source slots.  FS_SESSION_ROWS sessions refuse with an error that
 * says so.  Errors (each names its field and leaves the session as it was): no open session, not a live slot, n_positions outside
 * [1, T], T < 1 (a one-column prompt before its first step), P >= max_seq_len.
 * Semantics: let S be the slot's token history [C+1, L + n] -- its prompt columns, then one column per emitted frame.  A slot admitted on
 * the new prefix with body B is fs_lm_session_add_ex(concat(S[:, :P], B)) in every respect -- iteration count from P + L_body, max_seq_len
 * rule, admission number, own seed and settings, frame-0 rule, fresh repetition-penalty window, fresh StdRng stream -- except that rows
 * [0, P) are the ones the source slot computed (decode-step rows are not a prefill pass's rows) and only the body is prefilled.  To
 * continue a slot exactly where it stands: P = T and a body that starts with fs_lm_session_last_frame's column.  No kernel and no step
 * graph is specific to this call: sessions that never make it replay exactly the graphs they did before. */
int fs_lm_session_prefix_from_slot(fs_lm_t* lm, int slot, int n_positions, int* prefix_id, int* P_out);
/* column u32 [C+1] = the full input column [slow token, c0..c7] of the slot's last emitted frame, exactly as the engine would feed it
 * next (the host mirror of the slot's state after fs_lm_session_step).  The slow token of a Fish 1.5 frame is sampled, not derivable
 * from code 0, and fs_lm_session_poll does not return it: a continuation needs this call to be exact.  An error before the slot's first
 * frame.  For a cut at an EARLIER frame the caller needs that frame's slow token from elsewhere: a traced slot's token rows
 * (fs_lm_session_poll_trace) or the frames it forced a scoring slot along. */
int fs_lm_session_last_frame(fs_lm_t* lm, int slot, uint32_t* column);

/* timing of the last generate call, measured with HIP events on the handle's stream (the reference prints the
 * same quantities: single_batch.rs:233-246,291-304) */
typedef struct fs_gen_stats {
    double prefill_ms, decode_ms;     /* decode_ms covers frames 1..n-1 exactly like `start_decode` (:261) */
    uint64_t frames, prompt_tokens, graph_launches;
    uint64_t kernels_per_frame;       /* kernel launches per decode frame of this call: 266 on the per-node path (FS_GEN_NO_PERSIST), 146 with the
                                         persistent slow kernel only (sampler settings outside the in-launch sampler), 2 with both persistent
                                         kernels (greedy, and temp > 0 with 0 < top_k <= 256) */
    double slow_kernel_us, fast_kernel_us;  /* FS_GEN_TIME_KERNELS: average duration of k_slow_persist / k_fast_persist over the decode frames
                                               of this call (HIP events around every launch on the handle's stream); 0 otherwise */
} fs_gen_stats;
int fs_lm_last_stats(fs_lm_t* lm, fs_gen_stats* out);
/* the hipStream_t the handle launches on (for callers that bracket calls with their own HIP events) */
void* fs_lm_stream(fs_lm_t* lm);
/* Measurement hook (bench.py `roofline.dominant_kernel`): average duration in microseconds of ONE launch of a batch-1 decode kernel --
 * kind 0 qkv, 1 attention, 2 wo, 3 ffn_up (RMSNorm + W1||W3 GEMV + SwiGLU), 4 ffn_down -- run as a node of a captured hipGraph that cycles
 * over the slow layers' distinct weights (nothing cache-resident) at KV length kv_len, timed with HIP events on the engine stream;
 * kind 5 = average node of the fast decoder's layers over the 8 codebook positions, 6 = fast head GEMV, 7 = slow audio-range head GEMV.
 * Clears the slow KV caches. */
int fs_lm_bench_kernel(fs_lm_t* lm, int kind, int kv_len, int reps, float* us_per_launch);

/* ---- FireflyCodec ---------------------------------------------------------------------------------------- */

/* FireflyCodec::load (codec/firefly.rs:20-34) with FireflyConfig::get_config_for(1.4 | 1.5) (codec/config.rs:196-202).
 * channel_div = 1 for the real configuration; tests use 8 (channels / 8, same topology). */
int fs_codec_create(int device_id, int channel_div, fs_codec_t** out);
void fs_codec_destroy(fs_codec_t* c);
int fs_codec_load_safetensors(fs_codec_t* c, const char* path);
int fs_codec_load_synthetic(fs_codec_t* c, uint64_t seed);
/* FireflyCodec::decode (codec/firefly.rs:42-48): codes u32 [b, 8, T] (values 0..999) -> pcm f32 [b, 1, 2048*T] */
int fs_codec_decode(fs_codec_t* c, const uint32_t* codes, int b, int T, float* pcm_out);
/* FireflyCodec::encode (codec/firefly.rs:37-40) for one mono 44.1 kHz clip: LogMelSpectrogram::forward (audio/spectrogram.rs:
 * 153-158: streaming STFT n_fft 2048 / hop 512 with edge-repeating reflect padding, 160 slaney mel bins, clamp(1e-5,100).log())
 * -> FireflyEncoder::encode (codec/encoder.rs:38-42: ConvNeXt backbone, downsample x4, grouped FSQ).  codes_out: u32 [8, cap]
 * row-major, *n_frames = L = mel_frames / 4 codes per group.  (channel_div > 1 handles use a reduced backbone depth (1,1,2,1).) */
int fs_codec_encode(fs_codec_t* c, const float* pcm, int n_samples, uint32_t* codes_out, size_t cap, size_t* n_frames);
/* the (b, 1, samples) -> (b, 8, T) signature of FireflyCodec::encode (codec/firefly.rs:36-39, fish_speech_python/src/codec.rs:73-92) for
 * b clips: pcm f32 [b, stride] row-major (clip i = its first n_samples[i] samples), codes_out u32 [b, 8, cap], n_frames[b].  Every clip is
 * encoded ON ITS OWN (per-clip lengths, per-clip padding).  Deviation from the reference, on purpose: its front-end flattens whatever it is
 * given into ONE signal (audio/spectrogram.rs:33 `flatten_all`), so a batch comes back as (1, 8, L) codes of the clips glued together;
 * this entry point returns what the signature promises. */
int fs_codec_encode_batch(fs_codec_t* c, const float* pcm, int b, size_t stride, const int* n_samples, uint32_t* codes_out, size_t cap,
                          size_t* n_frames);
/* Stateful streaming decode (no reference counterpart: the reference vocodes an utterance in one piece, server/lib/handlers/speech.rs:98-129).
 * Every convolution of the 1.4+ / 1.5 codec is causal (codec/utils/mod.rs:53-62,110-122), so the chunks of ONE code sequence can be decoded
 * one after the other with the convolutions' left context carried on the device: fs_codec_stream_begin, then fs_codec_stream_decode per
 * chunk (codes u32 [8, T] row-major, T >= 16 frames; pcm_out f32 [2048 T]), then fs_codec_stream_end.  The concatenated PCM is bit-identical
 * to fs_codec_decode of the whole sequence and no frame is decoded twice.  Needs the plane data flow (precision mode 1 or 2, full-size codec);
 * the precision mode must not change inside a stream; one stream per handle. */
int fs_codec_stream_begin(fs_codec_t* c);
int fs_codec_stream_decode(fs_codec_t* c, const uint32_t* codes, int T, float* pcm_out);
int fs_codec_stream_end(fs_codec_t* c);
/* Many concurrent streams on ONE handle (one copy of the weights): every call advances n streams by T frames each in one launch sequence.
 * fs_codec_streams_open: *stream_id = a new stream (0 .. 63) starting from zero left context, like fs_codec_stream_begin; its precision mode
 * is the handle's mode at this moment, and a call that includes the stream after the mode changed is an error.  Ids of closed streams are
 * reused (a reopened id starts clean).  At most 64 streams are open per handle.  fs_codec_streams_close frees the id.
 * fs_codec_streams_decode: 1 <= n <= 64 DISTINCT open ids, in any order (the order does not change any stream's PCM); T >= 16 frames, the
 * same for every item.  codes u32 [n][8][T]: item i is the next (8, T) chunk of stream stream_ids[i] -- per item, NOT the raw reshape
 * (b, g, t) -> (g, b, t) that fs_codec_decode follows for b > 1 after the reference; pcm_out f32 [n][2048 T].  Per stream, the PCM of its
 * chunks concatenated is bit-identical to fs_codec_decode of its whole sequence at b = 1.  Everything (ids, T, codes < 1000, precision) is
 * validated before the first launch: a failed call leaves every stream's left context untouched.  Needs the plane data flow like the
 * single stream ("plane data flow" error for mode-0 and channel_div > 1 handles).  With the range check on, multi-stream chunks are
 * counted only.  Multi-streams and the single stream of fs_codec_stream_* are independent of each other.
 * Device memory per open stream: 2 x 96 x (C/4) x 1 KiB of plane contexts + 2 x 3 x C x 64 B of f32 contexts = 24.2 MiB at C = 512; the
 * pool keeps its high-water mark (grown in steps of doubling) until the handle is destroyed. */
int fs_codec_streams_open(fs_codec_t* c, int* stream_id);
int fs_codec_streams_close(fs_codec_t* c, int stream_id);
int fs_codec_streams_decode(fs_codec_t* c, int n, const int* stream_ids, const uint32_t* codes, int T, float* pcm_out);
/* Ragged form of fs_codec_streams_decode: item i = the next T[i] >= 1 frames of stream stream_ids[i]; the lengths differ per item and a
 * chunk may be as short as one frame (the 16-frame minimum of the calls above does not apply).  codes: the items' (8, T[i]) blocks
 * concatenated in item order; pcm_out: their 2048 * T[i] samples concatenated in item order.  Same rules otherwise (1 <= n <= 64 distinct open
 * ids, precision fixed per stream, everything -- n, every T[i], ids, precision, codes < 1000 -- validated before the first launch, a failed
 * call leaves every stream untouched).  Per stream, the PCM of all its chunks -- through this call and fs_codec_streams_decode in any
 * interleaving -- concatenated is bit-identical to fs_codec_decode of the whole sequence at b = 1; neither the order of the items nor the
 * lengths of the other items change a stream's PCM.  The left contexts follow the rule "last 64 slots of (old context ++ new data)", so they
 * are right for any chunk length.  The items run at the stride of the longest one: time and activation memory grow with n x max T[i], not
 * with the sum of the lengths; the per-stream device memory is that of fs_codec_streams_open, nothing is added per call. */
int fs_codec_streams_decode_ragged(fs_codec_t* c, int n, const int* stream_ids, const int* T, const uint32_t* codes, float* pcm_out);
/* FireflyCodec.sample_rate (codec/firefly.rs:13) */
int fs_codec_sample_rate(fs_codec_t* c);
/* Arithmetic of the decode path's convolutions (no reference counterpart: the reference runs the codec in f32,
 * server/lib/utils/load.rs:161-164; acceptance bound: PCM within 1e-4 RMS of it).
 * mode 2 (default) = "f16": every matrix operand rounded once to f16 (saturating at 65504), one f16 matrix product per term, f32
 *   accumulation, f32 residual stream and epilogues -- measured 1.6e-5 RMS at signal rms 0.031 (relative 5e-4, i.e. the size of the
 *   16-bit PCM quantisation step the server's WAV output applies anyway);
 * mode 1 = "bf16x3": each f32 operand split into bf16 hi + lo, three bf16 matrix products per term -- 3e-7 RMS, ~1.5x the time of mode 2;
 * mode 0 = exact f32 products on the f32 matrix cores (4e-8 of the oracle, ~4.5x the time of mode 2).  The encoder always uses mode 0. */
int fs_codec_set_precision(fs_codec_t* c, int mode);
int fs_codec_precision(fs_codec_t* c);
/* Range guard of mode 2 (validation tool, off by default; no reference counterpart).  f16 operands saturate beyond +-65504, vanish below
 * 2^-24, and carry a RELATIVE error (2^-11) against an absolute acceptance bound; synthetic N(0, 1 / fan_in) convs at the test signal's level
 * are far from all three, a weight-normed HiFi-GAN checkpoint or loud material has not been seen by this code.  With the check on,
 * fs_codec_decode in mode 2 (a) runs range-counting twins of the conversion kernels, (b) decodes the same codes in mode 1 (bf16x3: f32
 * exponent range, 2^-17 relative) too and takes the RMS difference of the two PCMs, and (c) returns the mode-1 PCM when an activation or
 * weight operand saturated or that difference exceeds 5e-5 (half the 1e-4 bound), else the mode-2 PCM.
 * fs_codec_range_stats: out5 = {activation operands saturated, flushed to zero (cumulative since the check was switched on), f16 weights
 * saturated, flushed (of the loaded checkpoint), decode calls answered from mode 1}; *last_pcm_rms_diff (nullable) = the RMS difference
 * of the last checked call.  Flushed operands are reported, not acted on (SiLU tails put a few hundred activations per decode below 2^-24
 * with any weights, < 6e-8 absolute each).  Streamed chunks (fs_codec_stream_decode) are counted only.  ~3x the cost of a plain call. */
int fs_codec_set_range_check(fs_codec_t* c, int on);
int fs_codec_range_stats(fs_codec_t* c, uint64_t* out5, double* last_pcm_rms_diff);

/* ---- Device sample-rate conversion (csrc/codec_resample.hip; counting rules and host evaluators in csrc/fs_resample_plan.h).  The reference
 * resamples on the CPU: server/lib/handlers/encode_speech.rs:50-54 (an uploaded clip, to the codec rate) and speech.rs:184-216 (every vocoded
 * chunk, 44.1 -> 24 kHz in front of the Opus encoder), both through audio/functional.rs::resample.  Two definitions:
 *
 * FS_RESAMPLE_LINEAR = fish_speech_core/lib/audio/functional.rs:3-37, bit for bit:
 *   ratio = (double)to / (double)from;  out_len = ceil((double)n * ratio);
 *   output i: idx = (double)i / ratio (an f64 division, not i * from / to);  f = floor(idx), c = min(ceil(idx), n - 1);
 *             t = (float)(idx - (double)f), u = 1.0f - t;  out = x[f] * u + x[c] * t, two f32 products rounded separately, then one f32 add.
 *   Where f64 rounding makes the last floor index n (n = 147 at 44.1 -> 24 kHz: out_len = 81, idx(80) = 147.0) the reference's gather is out
 *   of range and it returns an error; here f is clamped to n - 1 like c, and t = 0 there, so that sample repeats x[n - 1].
 *   from == to returns the input unchanged (finite samples).  Two taps and no low-pass: downsampling aliases at full level (a 19 845 Hz tone
 *   of amplitude 1 comes out of 44.1 -> 24 kHz at RMS 0.42).  It is there for parity with the reference on the encode path.
 *
 * FS_RESAMPLE_SINC = a Hann-windowed sinc polyphase filter, the construction of torchaudio's sinc_interp_hann with W = 6, rolloff = 0.99:
 *   g = gcd(from, to), o = from / g, p = to / g;  base = min(o, p) * rolloff, width = ceil(W * o / base), K = 2 * width + o taps;
 *   phase j < p, tap k < K: t = clamp((-j / p + (k - width) / o) * base, -W, W),
 *                           h[j][k] = (t == 0 ? 1 : sin(pi t) / (pi t)) * cos(pi t / (2 W))^2 * base / o, built in f64 once per pair, stored f32;
 *   out[m * p + j] = sum_{k = 0 .. K-1} h[j][k] * x[m * o + k - width], x = 0 outside [0, n), accumulated in f32 in ascending k (the fixed
 *   order is what makes chunked output equal one-shot output);  out_len = ceil(p * n / o) in integer arithmetic.
 *   44.1 -> 24 kHz: 80 x 171 taps, 44.1 -> 48: 160 x 161, 44.1 -> 16: 160 x 475, 22.05 -> 44.1: 2 x 15, 48 -> 44.1: 147 x 174, 8 -> 44.1: 441 x 94.
 *   A pair whose table would exceed 2^20 entries is refused with an error that names it.  The same tone comes out at RMS 5.6e-4.
 *
 * FS_PCM_F32: f32 samples.  FS_PCM_S16: fishrt/wav.py pcm_to_i16 (wav.rs:27-58) fused into the kernel's store: clip to [-1, 1], times
 * 32767.0f, truncate toward zero, NaN -> 0.  In the fs_codec_* calls a spec at the codec's own rate is a format conversion only, whatever
 * its mode; fs_resample follows the definitions to the letter, equal rates included. */
#define FS_RESAMPLE_LINEAR 0
#define FS_RESAMPLE_SINC 1
#define FS_PCM_F32 0
#define FS_PCM_S16 1
typedef struct fs_pcm_spec {
    int32_t rate, mode /* FS_RESAMPLE_* */, format /* FS_PCM_* */;
} fs_pcm_spec;
/* samples that n input samples become (either definition's out_len); no device */
int fs_resample_out_len(int from_rate, int to_rate, int mode, int64_t n, int64_t* out_len);
/* Stand-alone, no codec handle: b rows f32 at pcm + i * stride, row i n_samples[i] <= stride samples long (0 allowed), host -> device -> one
 * launch -> host.  out_buf: float or int16_t by out->format, row i at element i * out_stride, out_len[i] samples written; out_stride must hold
 * fs_resample_out_len of every row (checked before anything is launched). */
int fs_resample(int device_id, const float* pcm, int b, size_t stride, const int64_t* n_samples, int from_rate, const fs_pcm_spec* out,
                void* out_buf, size_t out_stride /* elements */, int64_t* out_len /* [b] */);
/* fs_codec_decode with every PCM row converted on the device, each on its own, before the copy to the host.  out: b rows of `cap` elements,
 * n_out[i] samples written in row i.  Equals fs_resample of fs_codec_decode's rows bit for bit. */
int fs_codec_decode_pcm(fs_codec_t* c, const uint32_t* codes, int b, int T, const fs_pcm_spec* spec, void* out, size_t cap /* elements per row */,
                        int64_t* n_out);
/* A multi-stream (fs_codec_streams_open) whose PCM leaves at spec->rate in spec->format.  On top of the stream's vocoder contexts it owns two
 * carry rows on the device -- the input samples that an output not yet emitted still reads: 2 x 2 floats in linear mode, 2 x (K + o) floats
 * in sinc mode (44.1 -> 24 kHz: 2.5 KB, 44.1 -> 16 kHz: 7.3 KB), none at the codec's own rate -- and three counters on the host.
 * fs_codec_streams_decode and fs_codec_streams_decode_ragged refuse such a stream (their PCM layout is fixed); use the call below. */
int fs_codec_streams_open_pcm(fs_codec_t* c, const fs_pcm_spec* spec, int* stream_id);
/* samples the next fs_codec_streams_decode_pcm item of T frames (final or not) would emit for this stream; changes nothing */
int fs_codec_streams_pending(fs_codec_t* c, int stream_id, int T, int final, int64_t* n_out);
/* fs_codec_streams_decode_ragged with a `final` flag per item (final == NULL: none) and every item's PCM converted by its stream's spec before
 * the copy to the host.  Streams opened any way are accepted: one from fs_codec_streams_open is codec rate, f32; one from
 * fs_codec_streams_open_speed (below) has a stretch stage in front of its conversion.  out: the items' outputs
 * concatenated in item order, each in its stream's format (so an f32 item may start at an odd 2-byte offset: copy it out before use);
 * n_out[i] = samples of item i.  A stream emits an output sample once all the input it reads exists -- linear: ceil(i / ratio) <= N - 1 after
 * N input samples, sinc: whole blocks of p outputs whose last tap lies inside the input -- and the rest, with the reference's clamp and the
 * right zero pad, when its item is final.  T[i] == 0 is allowed only with final[i] != 0: a pure flush.  After its final item a stream takes
 * no more items (close it).  Everything is validated before the first launch -- the rules of the ragged call, and cap_bytes against the
 * counted output, and final streams; a failed call leaves every stream untouched, vocoder contexts and resample counters alike.
 * Per stream, the outputs of all its calls concatenated equal fs_codec_decode_pcm of the whole sequence at b = 1, bit for bit, in both modes
 * and both formats, whatever the chunk lengths, the other items or their order. */
int fs_codec_streams_decode_pcm(fs_codec_t* c, int n, const int* stream_ids, const int* T, const uint8_t* final, const uint32_t* codes, void* out,
                                size_t cap_bytes, int64_t* n_out /* [n] samples */);
/* encode_speech.rs:50-54 on the device: pcm f32 interleaved [frames][channels] at `rate` Hz -> downmix (the channels summed in order in f32,
 * divided by (float)channels) -> resample to fs_codec_sample_rate in `mode` -> fs_codec_encode, with no trip to the host in between.  The
 * codes equal fs_codec_encode of the same resampled buffer bit for bit. */
int fs_codec_encode_pcm(fs_codec_t* c, const float* pcm, int channels, int64_t frames, int rate, int mode, uint32_t* codes_out, size_t cap,
                        size_t* n_frames);

/* ---- Device time-stretch: the `speed` of a request (csrc/codec_tsm.hip; lengths, checks and a host evaluator of this text in
 * csrc/fs_tsm_plan.h).  The reference has no speed control, and the LM cannot change its speaking rate, so speed is a time-scale modification
 * of the vocoder's PCM, done where the vocoder left it.  WSOLA with a squared-difference measure:
 *
 * Defaults: frame N = 1024, synthesis hop Hs = N / 2 = 512, search radius D = 512, at any rate.  fs_tsm_params may override them with N even,
 *   64 <= N <= 2048, 0 <= D <= 1024; the vocoder path (fs_codec_decode_speed) always uses the defaults.
 * Input x: f32, n samples, taken as zero outside [0, n).  speed: a double in [0.25, 4.0].
 *   out_len = floor(n / speed + 0.5), computed in f64;  K = ceil(out_len / Hs) frames;  nominal position q_k = floor(k * Hs * speed + 0.5), in f64.
 * Positions: p_0 = 0.  For k >= 1 the template is t[i] = x[p_{k-1} + Hs + i], i < N -- the natural continuation of the previous frame -- and
 *   for each lag d in [-D, D]:  e[d] = sum_{i < N} (t[i] - x[q_k + d + i])^2, accumulated in f32 in ONE order, the same for every lag:
 *     seg = ceil(N / 6); segment s = 0 .. 5 covers i in [s * seg, min(N, (s + 1) * seg)); within it, from a_s = 0 and in ascending i,
 *     df = t[i] - x[q_k + d + i] (one f32 subtraction), a_s = fma(df, df, a_s) (one rounding);
 *     e[d] = ((((a_0 + a_1) + a_2) + a_3) + a_4) + a_5, five f32 additions.
 *   p_k = q_k + d*, where d* minimises e; among equal e the smallest |d|, and of +-d the negative one.  A lag whose e is NaN never wins; when no
 *   lag's e is below +inf, d* = 0.
 * Window: w[i] = 0.5 - 0.5 cos(2 pi i / N), built in f64 and stored as f32.
 * Output sample m, with k = m / Hs and i = m - k * Hs:  k == 0: y[m] = x[m];  k >= 1: y[m] = w[i + Hs] * x[p_{k-1} + Hs + i] + w[i] * x[p_k + i],
 *   the two f32 products rounded separately, then one f32 add (no contraction into an FMA).
 * Consequences: at speed == 1 every e[0] is exactly 0 and p_k = k * Hs, so y is x up to the rounding of the two products.  Digital silence
 *   picks d = 0.  A signal that repeats bit for bit with an integer period P makes e[d] == e[d + P] bitwise -- every lag runs the same
 *   operations in the same order, which is why the order is fixed -- so there the tie rule decides.
 * In the fs_codec_* calls speed == 1.0 means "no stretch stage", as a spec at the codec's rate means no resample stage; fs_time_stretch follows
 * the definition to the letter, 1.0 included.
 *
 * Streams (fs_codec_streams_open_speed below).  The definition above stays the definition; a stream only adds WHEN a frame may be emitted, as
 * a function of n, the input samples it has seen so far.  With hi_k = lo_k = 0 for k == 0, else hi_k = q_k + D and lo_k = q_k - D, frame k --
 * output samples [k Hs, (k + 1) Hs) -- is emittable at n before the final item if and only if
 *     (k + 1) Hs <= out_len(n)                  it is a whole frame of whatever the final length turns out to be;
 *     k == 0:  Hs <= n;
 *     k >= 1:  q_k + D + N <= n                 the search region lies inside the input,
 *              hi_{k-1} + Hs + N <= n           and so does the template, wherever p_{k-1} was placed (the host does not know).
 *   A call emits the longest prefix of the frames not yet emitted that are emittable at its new n (emittability is monotone in k).  The final
 *   item emits every remaining frame up to K = ceil(out_len(n) / Hs), the last one cut at out_len(n), with x zero from n on as above; a final
 *   item of a stream that never saw a sample emits nothing.  At the defaults a frame waits for D + N = 1536 input samples beyond its nominal position.
 * Between calls a stream keeps p of its last frame (one int64 on the device) and the input the frames not yet emitted may still read: with k
 *   the next such frame, everything from max(0, min(lo_k, lo_{k-1} + Hs)) up to n.  That is fewer than
 *     ceil(max(g + 1, D + N, D + N + Hs - g + 1)) + ceil(max(D, g + 1 + D - Hs)),  g = Hs * speed
 *   samples whatever the chunk lengths (derived in csrc/fs_tsm_plan.h): at the defaults 4098 at speed 4.0, 2433 at speed 0.25. */
typedef struct fs_tsm_params {
    int32_t frame /* N */, radius /* D */;
} fs_tsm_params;
/* samples that n input samples become at `speed` (out_len above); no device */
int fs_time_stretch_out_len(int64_t n, double speed, int64_t* out_len);
/* Stand-alone, no codec handle: b rows f32 at pcm + i * stride, row i n_samples[i] <= stride samples long (0 allowed), host -> device -> the two
 * launches -> host.  params == NULL: the defaults.  out: f32, row i at element i * out_stride, out_len[i] samples written; out_stride must hold
 * fs_time_stretch_out_len of every row.  positions (nullable): int64, row i at element i * pos_stride, its K_i = ceil(out_len[i] / Hs) entries
 * p_0 .. p_{K_i - 1} written; pos_stride must hold every K_i.  Everything is checked before anything is launched. */
int fs_time_stretch(int device_id, const float* pcm, int b, size_t stride, const int64_t* n_samples, double speed, const fs_tsm_params* params,
                    float* out, size_t out_stride /* elements */, int64_t* out_len /* [b] */, int64_t* positions, size_t pos_stride);
/* fs_codec_decode -> time-stretch of every PCM row (the defaults) -> the resample / format stage of fs_codec_decode_pcm -> host, all on the
 * device.  out: b rows of `cap` elements, n_out[i] samples written in row i; cap must hold fs_resample_out_len of fs_time_stretch_out_len of a
 * row (checked, like speed and spec, before the first launch).  Equals fs_resample of fs_time_stretch of fs_codec_decode's rows bit for bit
 * (at the codec's own rate: the format conversion of fs_time_stretch's rows); with speed == 1.0 it is fs_codec_decode_pcm. */
int fs_codec_decode_speed(fs_codec_t* c, const uint32_t* codes, int b, int T, double speed, const fs_pcm_spec* spec, void* out,
                          size_t cap /* elements per row */, int64_t* n_out);
/* A multi-stream with a stretch stage (the defaults) between the vocoder and the stream's resample / format stage: the `speed` of a request
 * that streams.  spec == NULL: codec rate, f32.  speed == 1.0 means no stretch stage: the stream is then what fs_codec_streams_open_pcm (or,
 * with spec == NULL, fs_codec_streams_open) returns.  On top of what such a stream owns, a speed stream owns two stretch carry rows of the
 * bound above (2 x 16 KB at speed 4.0) and the position word on the device, and its frame and sample counters on the host.  It is decoded by
 * fs_codec_streams_decode_pcm, in any mix with plain and PCM streams; all speed streams of a call share one pair of stretch launches.  An
 * item's vocoder PCM goes through the stretch stage, which emits by the rule above; what that emits is fed, with the item's final flag, to the
 * stream's resample / format stage, which emits by its own rule.  fs_codec_streams_pending counts through both stages.  Per stream, the
 * outputs of all its calls concatenated equal fs_codec_decode_speed of the whole sequence at b = 1, bit for bit, whatever the chunk lengths,
 * the other items or their order.  speed and spec are checked here; fs_codec_streams_decode and fs_codec_streams_decode_ragged refuse a speed
 * stream.  A failed fs_codec_streams_decode_pcm call leaves the stretch counters, the carry rows' parity and the position word untouched too. */
int fs_codec_streams_open_speed(fs_codec_t* c, double speed, const fs_pcm_spec* spec /* nullable */, int* stream_id);
/* Test hook, no codec handle: the chunked stretch of ONE row.  pcm: n samples, cut into n_chunks consecutive chunks of chunk_len[i] >= 0
 * samples that add up to n; the last chunk is the final item (it may be empty: a pure flush).  Per chunk one plan step, one item and one
 * launch pair, with the two carry rows and the position word a speed stream owns; every chunk is uploaded on its own into poisoned storage,
 * so an earlier sample can only come from the carry.  out: the emitted samples concatenated, *out_len of them (out_cap must hold
 * fs_time_stretch_out_len); emitted[i]: samples chunk i emitted; positions (nullable): p_0 .. p_{K-1}, *n_positions = K (pos_cap must hold
 * K).  params == NULL: the defaults. */
int fs_selftest_tsm_chunks(int device_id, const float* pcm, int64_t n, const int64_t* chunk_len, int n_chunks, double speed,
                           const fs_tsm_params* params, float* out, size_t out_cap, int64_t* out_len, int64_t* emitted /* [n_chunks] */,
                           int64_t* positions, size_t pos_cap, int64_t* n_positions /* nullable */);

/* ---- Device loudness normalisation: the `loudness` of a request (csrc/codec_loud.hip; coefficients, counting, checks and a serial host
 * evaluator of this text in csrc/fs_loud_plan.h).  The vocoder's level depends on the voice's reference clip and on the text, and the
 * reference has no level control; a request that states a loudness in LUFS gets one gain for its whole PCM, measured and applied where the
 * vocoder left it.
 *
 * Measure: the integrated loudness of ITU-R BS.1770-4 for one channel, at any integer rate fs in 8000 .. 48000.
 * K-weighting: two biquads in cascade, their coefficients computed in f64 from the analogue prototypes (the libebur128 construction, which
 *   reproduces the standard's 48 kHz table).  For either stage K = tan(pi f0 / fs) and a0 = 1 + K/Q + K^2.
 *   Shelf: f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196, Vh = 10^(G/20), Vb = Vh^0.4996667741545416,
 *     b = [(Vh + Vb K/Q + K^2)/a0, 2 (K^2 - Vh)/a0, (Vh - Vb K/Q + K^2)/a0],  a = [1, 2 (K^2 - 1)/a0, (1 - K/Q + K^2)/a0].
 *   High-pass: f0 = 38.13547087602444, Q = 0.5003270373238773,  b = [1, -2, 1],  a = [1, 2 (K^2 - 1)/a0, (1 - K/Q + K^2)/a0].
 *   The input is f32, widened to f64, and zero before sample 0.  Both stages run in f64 from zero state, each in transposed direct form II:
 *     y = b0 x + s0;  s0 = b1 x - a1 y + s1;  s1 = b2 x - a2 y   (shelf)      z = y + s2;  s2 = -2 y - d1 z + s3;  s3 = y - d2 z   (high-pass,
 *     a = [1, d1, d2]).  An implementation may contract a product and a sum into an fma and may evaluate the recurrence in chunks (it is
 *     linear: the state after a chunk is A^len s_in + the state the chunk leaves from zero state); hop energies are held to a derived bound
 *     (tests/loud_refs.py), not to bits.
 * Hops and blocks: hop h = (fs + 5) / 10 in integer arithmetic (4410 at 44.1 kHz);  s_i = sum of z^2 over [i h, (i + 1) h) for the nb = n / h
 *   whole hops;  block j < nb - 3 has the mean square m_j = (s_j + s_{j+1} + s_{j+2} + s_{j+3}) / (4 h) and the loudness
 *   l_j = -0.691 + 10 log10(m_j).
 * Gates: absolute, keep the blocks with l_j > -70;  relative, Gamma = -0.691 + 10 log10(mean of the kept m_j) - 10, keep the blocks with
 *   l_j > -70 and l_j > Gamma;  L = -0.691 + 10 log10(mean of those m_j).  A comparison with a NaN is false, so such a block is never kept.
 *   With nb < 4, or when no block survives, the row has no loudness: L is reported as -inf and the gain is exactly 1.
 * Peak: the largest |x| of the row, in f32, NaN ignored (the sample peak, an exact quantity).
 * Gain: g_L = 10^((target_lufs - L) / 20) in f64;  g = min(g_L, 10^(max_gain_db / 20), 10^(peak_db / 20) / peak), the last term only when
 *   peak > 0;  rounded once to f32.  Output y[i] = x[i] * g, one f32 multiply.  No limiter, no look-ahead, no oversampling: the peak clause
 *   is what keeps the s16 pack from clipping.
 * Parameters: target_lufs in -40 .. -5;  peak_db <= 0 (FS_LOUD_PEAK_DB_DEFAULT = -1.0);  max_gain_db in 0 .. 60 (FS_LOUD_MAX_GAIN_DB_DEFAULT
 *   = 30).  A row takes at most 2^30 samples.
 * Out of scope, each a change of its own: loudness for multi-streams (fs_codec_streams_*: integrated loudness needs the whole signal, a stream
 *   needs a different, causal definition); normalising uploaded reference clips in fs_codec_encode_pcm; true-peak measurement (oversampled);
 *   multichannel weighting. */
#define FS_LOUD_PEAK_DB_DEFAULT (-1.0)
#define FS_LOUD_MAX_GAIN_DB_DEFAULT 30.0
typedef struct fs_loud_params {
    double target_lufs, peak_db, max_gain_db;
} fs_loud_params;
typedef struct fs_loud_result {
    double lufs;                       /* L, or -inf */
    float peak, gain;                  /* gain: 1 when the call only measures */
    int32_t blocks_total, blocks_kept; /* max(nb - 3, 0); the blocks that passed both gates */
} fs_loud_result;
/* Stand-alone, no codec handle: b rows f32 at pcm + i * stride, row i n_samples[i] <= stride samples long (0 allowed), host -> device -> host.
 * out == NULL measures only; then params may be NULL too and every gain is 1.  out: f32, row i at element i * out_stride, its n_samples[i]
 * samples written.  res: one record per row.  A row's record and output do not depend on the other rows of the call.  Everything (rate,
 * params, lengths, strides) is checked before anything is launched. */
int fs_loudness_normalize(int device_id, const float* pcm, int b, size_t stride, const int64_t* n_samples, int rate, const fs_loud_params* params,
                          float* out, size_t out_stride /* elements */, fs_loud_result* res /* [b] */);
/* fs_codec_decode -> loudness (measure, gain, multiply) of every PCM row at the codec's rate -> time-stretch (speed != 1.0 only) -> the
 * resample / format stage of fs_codec_decode_pcm -> host, all on the device.  res (nullable): one record per row.  Equals fs_resample of
 * fs_time_stretch of fs_loudness_normalize of fs_codec_decode's rows bit for bit.  loud == NULL: it is fs_codec_decode_speed (res untouched).
 * loud, speed, spec and cap are checked before the first launch; a refused call leaves the handle as it was. */
int fs_codec_decode_loud(fs_codec_t* c, const uint32_t* codes, int b, int T, const fs_loud_params* loud, double speed, const fs_pcm_spec* spec,
                         void* out, size_t cap /* elements per row */, int64_t* n_out, fs_loud_result* res);
/* Test hook, no codec handle: the hop energies s_0 .. s_{nb-1} of ONE row as the device summed them (cap must hold nb = n / h), and the row's
 * record of a measuring call. */
int fs_selftest_loud_hops(int device_id, const float* pcm, int64_t n, int rate, double* hops, size_t cap, int64_t* n_hops, fs_loud_result* res);

#ifdef __cplusplus
}
#endif
#endif /* FISHRT_H */
