"""ctypes binding of libfishrt.so (include/fishrt.h).  The library is REQUIRED: there is no CPU / PyTorch fallback --
importing works without a GPU (so the symbol table can be checked), but creating any handle without an MI355X fails."""
import ctypes as C
import os

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(_PKG, "libfishrt.so")


class ModelArgs(C.Structure):  # fs_model_args  <->  BaseModelArgs (dual_ar.rs:57-81)
    _fields_ = [(n, C.c_int32) for n in ("dim", "n_layer", "n_fast_layer", "n_head", "n_local_heads", "head_dim",
                                         "intermediate_size", "num_codebooks", "codebook_size", "vocab_size",
                                         "max_seq_len")] + [("norm_eps", C.c_float), ("rope_base", C.c_float),
                                                            ("tie_word_embeddings", C.c_int32)]


class TokenCfg(C.Structure):  # fs_token_cfg  <->  TokenConfig (dual_ar.rs:17-23)
    _fields_ = [("im_end_id", C.c_uint32), ("pad_id", C.c_uint32), ("semantic_start_id", C.c_uint32),
                ("semantic_end_id", C.c_uint32), ("has_semantic_end", C.c_int32)]


class Sampling(C.Structure):  # fs_sampling  <->  SamplingArgs (sampling/mod.rs:29-34)
    _fields_ = [("temp", C.c_double), ("top_p", C.c_double), ("top_k", C.c_uint64), ("repetition_penalty", C.c_float)]


class GenStats(C.Structure):
    _fields_ = [("prefill_ms", C.c_double), ("decode_ms", C.c_double), ("frames", C.c_uint64),
                ("prompt_tokens", C.c_uint64), ("graph_launches", C.c_uint64), ("kernels_per_frame", C.c_uint64),
                ("slow_kernel_us", C.c_double), ("fast_kernel_us", C.c_double)]


class KvBlobHeader(C.LittleEndianStructure):  # fs_kv_blob_header: the 64 bytes in front of a prefix KV blob's payload
    _fields_ = [("magic", C.c_char * 8), ("version", C.c_uint32), ("kv_dtype", C.c_uint32), ("n_layer", C.c_int32),
                ("n_local_heads", C.c_int32), ("head_dim", C.c_int32), ("P", C.c_int32), ("header_bytes", C.c_uint32),
                ("reserved", C.c_uint32), ("weights_fingerprint", C.c_uint64), ("payload_bytes", C.c_uint64),
                ("reserved2", C.c_uint64)]


class ConvCase(C.Structure):  # fs_conv_case: one convolution for fs_selftest_conv1d
    _fields_ = [(n, C.c_int32) for n in ("flow", "precision", "B", "Cin", "Cout", "T", "K", "dil", "stride", "pre_silu", "epi",
                                         "post_silu", "input", "outputs", "range_check", "reserved")] + \
               [(n, C.POINTER(C.c_float)) for n in ("x", "x_b", "x_c", "w", "bias", "w2", "bias2", "res", "gamma", "mean_a", "mean_b")]


class CodecOpCase(C.Structure):  # fs_codec_op_case: one encoder-side / ConvNeXt / FSQ launcher for fs_selftest_codec_op
    _fields_ = [(n, C.c_int32) for n in ("op", "B", "C", "T", "n", "n_fft", "hop", "nf", "n_mels", "s", "G", "dg", "ctx_mode", "item_rows",
                                         "reserved0", "reserved1")] + [("ctx_elems", C.c_int64)] + \
               [(n, C.POINTER(C.c_float)) for n in ("x", "w0", "w1", "w2", "w3", "ctx")] + \
               [("ctx_off", C.POINTER(C.c_int64)), ("codes", C.POINTER(C.c_uint32))]


class AttnCase(C.Structure):  # fs_attn_case: one attention launcher call for fs_selftest_attn
    _fields_ = [(n, C.c_int32) for n in ("op", "wt", "H", "Hk", "Dh", "dim", "M", "pos", "pos_step", "rope_off", "pt_stride", "pt_rows", "pt_len",
                                         "seq_rows", "n_chunks_max", "nc_launch", "part_rows", "no_flash", "chunked_attn", "small_attn",
                                         "identity_pages", "n_pages", "fused_T", "tbl0", "code_slot", "tbl_rows", "rope_rows", "n_expf",
                                         "plan_only", "reserved")] + [("stale_part", C.c_float), ("reserved2", C.c_int32)] + \
               [(n, C.POINTER(C.c_int32)) for n in ("row_pos", "seq_pos", "page_table")] + \
               [(n, C.POINTER(C.c_float)) for n in ("k", "v", "q", "wo", "x", "tbl", "cos_t", "sin_t", "expf_x")] + \
               [("codes", C.POINTER(C.c_uint32))]


class GemmCase(C.Structure):  # fs_gemm_case: one row-path GEMM launcher call for fs_selftest_gemm
    _fields_ = [(n, C.c_int32) for n in ("op", "fp8", "epi", "rt", "M", "N", "K", "ksplit", "D", "S", "want_frag", "ldy", "ldo", "H", "Hk", "Dh",
                                         "pos", "rope_off", "pos_step", "pt_stride", "seq_rows", "pt_rows", "pt_len", "n_pages", "rope_rows",
                                         "o1", "nblk", "big_min_m", "n_launches", "stale_tag", "node_id", "epoch", "plan_only",
                                         "reserved")] + [("eps", C.c_float), ("reserved2", C.c_int32)] + \
               [(n, C.POINTER(C.c_float)) for n in ("x", "x2", "p", "norm_w", "w", "wscale", "y", "g", "ss", "cos_t", "sin_t", "k", "v")] + \
               [(n, C.POINTER(C.c_int32)) for n in ("row_pos", "row_rope_off", "seq_pos", "seq_rope_off", "page_table")]


class GemmOut(C.Structure):  # fs_gemm_out: where fs_selftest_gemm leaves its results
    _fields_ = [(n, C.POINTER(C.c_float)) for n in ("y", "planes", "ss", "k", "v")] + [("epoch1", C.POINTER(C.c_uint32)), ("variant", C.c_char_p)] + \
               [(n, C.c_size_t) for n in ("y_cap", "planes_cap", "ss_cap", "pool_cap", "variant_cap", "n_y", "n_planes", "n_ss")] + \
               [("grid", C.c_int32 * 3), ("guard_ok", C.c_int32)]


class GemvCase(C.Structure):  # fs_gemv_case: one batch-1 node launcher call for fs_selftest_gemv
    _fields_ = [(n, C.c_int32) for n in ("op", "wt", "plan_only", "cache_resident", "dim", "inter", "H", "Hk", "Dh", "n_rows", "pos", "rope_off",
                                         "use_state", "n_pages", "pt_len", "rope_rows", "n_cb", "cb_size", "tok_rows", "prompt_L", "step",
                                         "use_prompt", "n_tokens", "n_ids")] + \
               [("sem_lo", C.c_uint32), ("sem_hi", C.c_uint32), ("eps", C.c_float), ("reserved", C.c_int32)] + \
               [(n, C.POINTER(C.c_float)) for n in ("x", "norm_w", "w", "wscale", "y", "cos_t", "sin_t", "k", "v", "tok_emb", "cb_emb")] + \
               [("page_table", C.POINTER(C.c_int32)), ("tokens", C.POINTER(C.c_uint32)), ("ids", C.POINTER(C.c_uint32))]


class GemvOut(C.Structure):  # fs_gemv_out: where fs_selftest_gemv leaves its results
    _fields_ = [(n, C.POINTER(C.c_float)) for n in ("y", "k", "v")] + [("variant", C.c_char_p)] + \
               [(n, C.c_size_t) for n in ("y_cap", "pool_cap", "variant_cap", "n_y", "n_pool")] + [("grid", C.c_int32 * 3), ("guard_ok", C.c_int32)]


class SampleCase(C.Structure):  # fs_sample_case: F frames of the production sampler launches for fs_selftest_sample_frames
    _fields_ = [(n, C.c_int32) for n in ("family", "wt", "plan_only", "B", "F", "n_cb", "cb_size", "n_slow", "ld", "dim", "out_cap", "tok_rows",
                                         "prep", "hid", "session", "cap_frames", "batch_rows", "batch_row", "n_cfg", "reserved")] + \
               [("eps", C.c_float), ("reserved2", C.c_int32), ("tokens", TokenCfg), ("reserved3", C.c_int32),
                ("samplings", C.POINTER(Sampling)), ("seeds", C.POINTER(C.c_uint64)), ("ignore_eos", C.POINTER(C.c_int32)),
                ("state0", C.POINTER(C.c_int32))] + \
               [(n, C.POINTER(C.c_float)) for n in ("tok_emb", "cb_emb", "fast_emb", "prep_g", "x", "logits")]


SAMPLE_OUTS = ("STATES", "RING", "META", "MASK", "RNG", "WORDS", "XF", "X", "PREP", "EPOCH", "CODES", "HID", "CAP")


class SampleOut(C.Structure):  # fs_sample_out: where fs_selftest_sample_frames leaves the state after every launch (sizes in bytes)
    _fields_ = [("buf", C.c_void_p * len(SAMPLE_OUTS)), ("cap", C.c_size_t * len(SAMPLE_OUTS)), ("need", C.c_size_t * len(SAMPLE_OUTS)),
                ("n_launches", C.c_int32), ("guard_ok", C.c_int32)]


FRAME_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32))

# every symbol include/fishrt.h declares (tests/test_abi.py checks the library exports all of them)
SYMBOLS = ["fs_last_error", "fs_version", "fs_device_count", "fs_lm_create", "fs_lm_destroy", "fs_lm_load_safetensors",
           "fs_lm_load_synthetic", "fs_lm_forward_generate", "fs_lm_forward_generate_fast", "fs_lm_fast_embed",
           "fs_lm_clear_fast_layer_caches", "fs_lm_clear_slow_layer_caches", "fs_lm_clear_slow_caches_until",
           "fs_lm_curr_kv_size", "fs_lm_generate", "fs_lm_generate_with_hidden", "fs_lm_generate_batch", "fs_lm_generate_static_batch", "fs_lm_generate_multi", "fs_lm_rows_supported", "fs_lm_debug_read_row", "fs_lm_debug_read_kv", "fs_lm_last_stats", "fs_lm_stream", "fs_lm_bench_kernel",
           "fs_lm_weights_arena", "fs_lm_weights_adopt", "fs_comm_unique_id", "fs_comm_create", "fs_comm_destroy", "fs_comm_rank", "fs_comm_world", "fs_comm_barrier",
           "fs_comm_all_reduce_f64", "fs_comm_broadcast_weights", "fs_comm_broadcast_prompt_dims", "fs_comm_broadcast_prompts", "fs_comm_all_gather_codes", "fs_lm_session_begin", "fs_lm_session_add", "fs_lm_session_step", "fs_lm_session_poll", "fs_lm_session_release", "fs_lm_session_end",
           "fs_lm_session_prefix_create", "fs_lm_session_prefix_release", "fs_lm_session_add_prefixed", "fs_lm_session_add_ex", "fs_lm_session_add_hidden", "fs_lm_session_poll_hidden", "fs_lm_session_info",
           "fs_lm_session_add_scored", "fs_lm_session_poll_scores", "fs_selftest_score_rows",
           "fs_lm_session_add_traced", "fs_lm_session_poll_trace",
           "fs_lm_session_poll_alts", "fs_selftest_alt_rows",
           "fs_selftest_conv1d", "fs_selftest_codec_op", "fs_selftest_codec_encode_stage", "fs_selftest_attn", "fs_selftest_gemm",
           "fs_selftest_gemv", "fs_selftest_sample_frames",
           "fs_lm_weights_fingerprint", "fs_lm_session_prefix_export", "fs_lm_session_prefix_import",
           "fs_lm_session_prefix_from_slot", "fs_lm_session_last_frame",
           "fs_codec_create", "fs_codec_destroy", "fs_codec_load_safetensors", "fs_codec_load_synthetic",
           "fs_codec_decode", "fs_codec_encode", "fs_codec_encode_batch", "fs_codec_sample_rate", "fs_codec_set_precision", "fs_codec_precision", "fs_codec_set_range_check", "fs_codec_range_stats", "fs_codec_stream_begin", "fs_codec_stream_decode", "fs_codec_stream_end", "fs_codec_streams_open", "fs_codec_streams_close", "fs_codec_streams_decode", "fs_codec_streams_decode_ragged",
           "fs_resample_out_len", "fs_resample", "fs_codec_decode_pcm", "fs_codec_streams_open_pcm", "fs_codec_streams_pending",
           "fs_codec_streams_decode_pcm", "fs_codec_encode_pcm",
           "fs_time_stretch_out_len", "fs_time_stretch", "fs_codec_decode_speed",
           "fs_codec_streams_open_speed", "fs_selftest_tsm_chunks",
           "fs_loudness_normalize", "fs_codec_decode_loud", "fs_selftest_loud_hops",
           "fs_fp8_quantize_rows", "fs_fp8_decode_table", "fs_selftest", "fs_lm_selftest", "fs_selftest_sample_rows", "fs_selftest_sample_slots", "fs_lm_debug_capture", "fs_lm_debug_read"]

# flags of fs_lm_generate* / fs_lm_session_begin (include/fishrt.h)
FS_GEN_IGNORE_EOS, FS_SESSION_ROWS, FS_SESSION_PER_SLOT, FS_SESSION_WIDE_SAMPLER = 1, 8, 16, 32
FS_SESSION_SCORE = 64
FS_SESSION_TRACE = 128
FS_SESSION_ALTS = 256
FS_ALTS_MAX = 16


def FS_SESSION_ALTS_N(n):  # the 5-bit N field of the flags (0 = the default of 8)
    return (int(n) & 0xFFFFFFFF) << 16


# argument types of the scoring entry points (the size_t / pointer arguments must not go through ctypes' int default)
_U32P, _F32P = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
SCORE_PROTOTYPES = {
    "fs_lm_session_add_scored": [C.c_void_p, C.c_int, _U32P, C.c_int, _U32P, C.c_int, C.c_int, C.POINTER(C.c_int)],
    "fs_lm_session_poll_scores": [C.c_void_p, C.c_int, C.c_size_t, _F32P, _F32P, _U32P, _F32P, C.c_size_t, C.POINTER(C.c_size_t)],
    "fs_selftest_score_rows": [C.c_int, _F32P, C.c_int, C.c_int, _U32P, C.c_int, _F32P, _F32P, _U32P, _F32P],
}
# ... and of the traced-slot entry points (sampling: const fs_sampling*, seed: const uint64_t*, both nullable)
TRACE_PROTOTYPES = {
    "fs_lm_session_add_traced": [C.c_void_p, C.c_int, _U32P, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.c_int, C.POINTER(C.c_int)],
    "fs_lm_session_poll_trace": [C.c_void_p, C.c_int, C.c_size_t, _U32P, _F32P, _F32P, _U32P, _F32P, C.POINTER(C.c_int), C.c_size_t,
                                 C.POINTER(C.c_size_t)],
}
# ... and of the alternatives' entry points (FS_SESSION_ALTS sessions)
ALTS_PROTOTYPES = {
    "fs_lm_session_poll_alts": [C.c_void_p, C.c_int, C.c_size_t, _U32P, _F32P, _F32P, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int)],
    "fs_selftest_alt_rows": [C.c_int, _F32P, C.c_int, C.c_int, C.c_int, C.c_int, _U32P, _F32P, _F32P],
}

# fs_selftest_conv1d (flows, input kinds, epilogues, outputs: include/fishrt.h)
FS_CONV_CONV1D, FS_CONV_TCONV1D, FS_CONV_CONV1D_PLANES, FS_CONV_TCONV1D_PLANES, FS_CONV_RESPAIR_F16 = range(5)
FS_CONV_IN_F32, FS_CONV_IN_SPLIT, FS_CONV_IN_SPLIT_SILU, FS_CONV_IN_MEAN3, FS_CONV_IN_MEAN3_SILU = range(5)
FS_CONV_EPI_NONE, FS_CONV_EPI_GELU, FS_CONV_EPI_GAMMA_RES, FS_CONV_EPI_RES, FS_CONV_EPI_TANH = range(5)
FS_CONV_OUT_F32, FS_CONV_OUT_PLANES = 1, 2
CONV_PROTOTYPES = {
    "fs_selftest_conv1d": [C.c_int, C.POINTER(ConvCase), _F32P, _F32P, C.c_char_p, C.c_size_t, C.POINTER(C.c_uint64)],
}

# fs_selftest_codec_op (ops: include/fishrt.h) and the encoder stage tap
(FS_CODEC_OP_STFT_MAG, FS_CODEC_OP_MEL_LOG, FS_CODEC_OP_LAYERNORM_CF, FS_CODEC_OP_DWCONV_LN, FS_CODEC_OP_SPACE_TO_DEPTH, FS_CODEC_OP_FSQ_ENCODE,
 FS_CODEC_OP_FSQ_PROJECT) = range(7)
CODEC_OP_PROTOTYPES = {
    "fs_selftest_codec_op": [C.c_int, C.POINTER(CodecOpCase), C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int)],
    "fs_selftest_codec_encode_stage": [C.c_void_p, _F32P, C.c_int, C.c_int, _F32P, C.c_size_t, C.POINTER(C.c_size_t)],
}

# fs_selftest_attn (ops, weight types: include/fishrt.h)
FS_ATTN_DECODE, FS_ATTN_DECODE_WO, FS_ATTN_WO_FUSED, FS_ATTN_ROWS, FS_ATTN_EXPF = range(5)
FS_ATTN_WT_F32, FS_ATTN_WT_BF16, FS_ATTN_WT_FP8 = range(3)
ATTN_PROTOTYPES = {
    "fs_selftest_attn": [C.c_int, C.POINTER(AttnCase), _F32P, C.c_size_t, C.POINTER(C.c_size_t), _F32P, _F32P, C.c_char_p, C.c_size_t,
                         C.POINTER(C.c_int)],
}

# fs_selftest_gemm (ops, epilogues: include/fishrt.h)
FS_GEMM_PREP, FS_GEMM_ROWS, FS_GEMM_DOWN = range(3)
GEMM_EPI = {n: i for i, n in enumerate(("STORE", "RESIDUAL", "SWIGLU", "QKV", "RESIDUAL_NORM", "SWIGLU_RMS", "QKV_RMS", "STORE_RMS", "QKV_SEQ"))}
GEMM_PROTOTYPES = {"fs_selftest_gemm": [C.c_int, C.POINTER(GemmCase), C.POINTER(GemmOut)]}

# fs_selftest_gemv (ops, weight types: include/fishrt.h)
GEMV_OPS = {n: i for i, n in enumerate(("QKV", "FFN_UP", "FFN_DOWN", "HEAD", "WO_BODY", "EMBED", "FAST_EMBED"))}
GEMV_WT = {"f32": 0, "bf16": 1, "fp8": 2}
GEMV_PROTOTYPES = {"fs_selftest_gemv": [C.c_int, C.POINTER(GemvCase), C.POINTER(GemvOut)]}

# fs_selftest_sample_frames (families: include/fishrt.h; wt: GEMV_WT's f32 / bf16)
SAMPLE_FAMILIES = {n: i for i, n in enumerate(("single", "single_batchrow", "rows", "rows_par", "slots", "slots_wide"))}
SAMPLE_PROTOTYPES = {"fs_selftest_sample_frames": [C.c_int, C.POINTER(SampleCase), C.POINTER(SampleOut)]}

# ... and of the calls that make a prefix out of a slot's history
HISTORY_PROTOTYPES = {
    "fs_lm_session_prefix_from_slot": [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)],
    "fs_lm_session_last_frame": [C.c_void_p, C.c_int, _U32P],
}

# device sample-rate conversion (include/fishrt.h: FS_RESAMPLE_*, FS_PCM_*, fs_pcm_spec)
RESAMPLE_MODES = {"linear": 0, "sinc": 1}
PCM_FORMATS = {"f32": 0, "s16": 1}
PCM_DTYPES = {"f32": "<f4", "s16": "<i2"}


class PcmSpec(C.Structure):  # fs_pcm_spec
    _fields_ = [("rate", C.c_int32), ("mode", C.c_int32), ("format", C.c_int32)]


def pcm_spec(rate, mode, dtype):
    if mode not in RESAMPLE_MODES:
        raise ValueError(f"resample mode must be one of {sorted(RESAMPLE_MODES)}")
    if dtype not in PCM_FORMATS:
        raise ValueError(f"PCM dtype must be one of {sorted(PCM_FORMATS)}")
    return PcmSpec(int(rate), RESAMPLE_MODES[mode], PCM_FORMATS[dtype])


_I64P = C.POINTER(C.c_int64)
RESAMPLE_PROTOTYPES = {
    "fs_resample_out_len": [C.c_int, C.c_int, C.c_int, C.c_int64, _I64P],
    "fs_resample": [C.c_int, _F32P, C.c_int, C.c_size_t, _I64P, C.c_int, C.POINTER(PcmSpec), C.c_void_p, C.c_size_t, _I64P],
    "fs_codec_decode_pcm": [C.c_void_p, _U32P, C.c_int, C.c_int, C.POINTER(PcmSpec), C.c_void_p, C.c_size_t, _I64P],
    "fs_codec_streams_open_pcm": [C.c_void_p, C.POINTER(PcmSpec), C.POINTER(C.c_int)],
    "fs_codec_streams_pending": [C.c_void_p, C.c_int, C.c_int, C.c_int, _I64P],
    "fs_codec_streams_decode_pcm": [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint8), _U32P, C.c_void_p,
                                    C.c_size_t, _I64P],
    "fs_codec_encode_pcm": [C.c_void_p, _F32P, C.c_int, C.c_int64, C.c_int, C.c_int, _U32P, C.c_size_t, C.POINTER(C.c_size_t)],
}



# device time-stretch (include/fishrt.h: fs_tsm_params; speed is a double)
class TsmParams(C.Structure):  # fs_tsm_params
    _fields_ = [("frame", C.c_int32), ("radius", C.c_int32)]


TSM_PROTOTYPES = {
    "fs_time_stretch_out_len": [C.c_int64, C.c_double, _I64P],
    "fs_time_stretch": [C.c_int, _F32P, C.c_int, C.c_size_t, _I64P, C.c_double, C.POINTER(TsmParams), _F32P, C.c_size_t, _I64P, _I64P, C.c_size_t],
    "fs_codec_decode_speed": [C.c_void_p, _U32P, C.c_int, C.c_int, C.c_double, C.POINTER(PcmSpec), C.c_void_p, C.c_size_t, _I64P],
    "fs_codec_streams_open_speed": [C.c_void_p, C.c_double, C.POINTER(PcmSpec), C.POINTER(C.c_int)],
    "fs_selftest_tsm_chunks": [C.c_int, _F32P, C.c_int64, _I64P, C.c_int, C.c_double, C.POINTER(TsmParams), _F32P, C.c_size_t, _I64P, _I64P, _I64P,
                               C.c_size_t, _I64P],
}



# device loudness normalisation (include/fishrt.h: fs_loud_params, fs_loud_result)
class LoudParams(C.Structure):  # fs_loud_params
    _fields_ = [("target_lufs", C.c_double), ("peak_db", C.c_double), ("max_gain_db", C.c_double)]


class LoudResult(C.Structure):  # fs_loud_result
    _fields_ = [("lufs", C.c_double), ("peak", C.c_float), ("gain", C.c_float), ("blocks_total", C.c_int32), ("blocks_kept", C.c_int32)]


LOUD_PROTOTYPES = {
    "fs_loudness_normalize": [C.c_int, _F32P, C.c_int, C.c_size_t, _I64P, C.c_int, C.POINTER(LoudParams), _F32P, C.c_size_t, C.POINTER(LoudResult)],
    "fs_codec_decode_loud": [C.c_void_p, _U32P, C.c_int, C.c_int, C.POINTER(LoudParams), C.c_double, C.POINTER(PcmSpec), C.c_void_p, C.c_size_t,
                             _I64P, C.POINTER(LoudResult)],
    "fs_selftest_loud_hops": [C.c_int, _F32P, C.c_int64, C.c_int, C.POINTER(C.c_double), C.c_size_t, _I64P, C.POINTER(LoudResult)],
}

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with fish-speech.rs_amd/build.sh (hipcc, gfx950). "
                               "fishrt has no fallback path.")
        L = C.CDLL(LIB_PATH)
        L.fs_last_error.restype = C.c_char_p
        L.fs_version.restype = C.c_char_p
        L.fs_lm_stream.restype = C.c_void_p
        L.fs_lm_destroy.restype = None
        L.fs_codec_destroy.restype = None
        L.fs_comm_destroy.restype = None
        L.fs_comm_destroy.argtypes = [C.c_void_p]
        L.fs_lm_destroy.argtypes = [C.c_void_p]
        L.fs_codec_destroy.argtypes = [C.c_void_p]
        for name, argtypes in {**SCORE_PROTOTYPES, **TRACE_PROTOTYPES, **ALTS_PROTOTYPES, **CONV_PROTOTYPES, **CODEC_OP_PROTOTYPES, **ATTN_PROTOTYPES, **GEMM_PROTOTYPES, **GEMV_PROTOTYPES, **SAMPLE_PROTOTYPES, **HISTORY_PROTOTYPES,
                               **RESAMPLE_PROTOTYPES, **TSM_PROTOTYPES, **LOUD_PROTOTYPES}.items():
            if hasattr(L, name):  # (an older build loaded through LIB_PATH -- tools/attn_paths_dump.py --lib -- may lack the newest entry points)
                getattr(L, name).argtypes = argtypes
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise RuntimeError(lib().fs_last_error().decode())
