// extern "C" surface of libfishrt.so (include/fishrt.h).  Thin: argument checks, exception -> status + message.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/fishrt.h"
#include "codec_engine.h"
#include "fs_comm.h"
#include "fs_common.h"
#include "fs_resample_plan.h"
#include "fs_loud_plan.h"
#include "fs_tsm_plan.h"
#include "lm_engine.h"
#include "lm_kernels.h"
#include "lm_persist.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

static thread_local std::string g_err;

struct fs_lm { fs::LMBase* impl; };
struct fs_codec { fs::CodecBase* impl; };
struct fs_comm { fs::Comm* impl; };

#define FS_TRY(body)                                                          \
    try { body; return FS_OK; }                                               \
    catch (const std::exception& e) { g_err = e.what(); return FS_ERR; }      \
    catch (...) { g_err = "unknown error"; return FS_ERR; }
#define FS_ARG(cond, msg) if (!(cond)) { g_err = msg; return FS_ERR; }

extern "C" {

const char* fs_last_error(void) { return g_err.c_str(); }
const char* fs_version(void) { return "fishrt 0.4.0 (gfx950)"; }
int fs_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int fs_fp8_quantize_rows(int device_id, const float* w, int64_t rows, int64_t cols, uint8_t* q_out, float* scales_out) {
    FS_ARG(w && q_out && scales_out, "null argument");
    FS_TRY(fs::fp8_quantize_rows(device_id, w, rows, cols, q_out, scales_out))
}
int fs_fp8_decode_table(int device_id, float* out) { FS_ARG(out, "null argument"); FS_TRY(fs::fp8_decode_table(device_id, out)) }

static void selftest_pf_reduce(int device) {
    FS_HIP(hipSetDevice(device));
    std::vector<float> in(64 * 32), out(96, 0.f);
    uint32_t st = 12345u;
    for (auto& v : in) { st = st * 1664525u + 1013904223u; v = (float)((st >> 8) & 0xFFFF) / 65536.f - 0.5f; }
    float *din = nullptr, *dout = nullptr;
    FS_HIP(hipMalloc(&din, in.size() * 4));
    FS_HIP(hipMalloc(&dout, out.size() * 4));
    FS_HIP(hipMemcpy(din, in.data(), in.size() * 4, hipMemcpyHostToDevice));
    FS_HIP(hipMemset(dout, 0, out.size() * 4));
    fs::launch_pf_reduce_selftest(din, dout, nullptr);
    FS_HIP(hipDeviceSynchronize());
    FS_HIP(hipMemcpy(out.data(), dout, out.size() * 4, hipMemcpyDeviceToHost));
    (void)hipFree(din); (void)hipFree(dout);
    auto host = [&](int i) { double s = 0; for (int l = 0; l < 64; ++l) s += in[l * 32 + i]; return (float)s; };
    for (int i = 0; i < 32; ++i) if (std::fabs(out[i] - host(i)) > 1e-4f) throw fs::Error("pf_reduce<32> value " + std::to_string(i) + " wrong");
    for (int i = 0; i < 16; ++i) if (std::fabs(out[32 + i] - host(i)) > 1e-4f) throw fs::Error("pf_reduce<16> value " + std::to_string(i) + " wrong");
    for (int i = 0; i < 8; ++i) if (std::fabs(out[48 + i] - host(i)) > 1e-4f) throw fs::Error("pf_reduce<8> value " + std::to_string(i) + " wrong");
    for (int i = 0; i < 4; ++i) if (std::fabs(out[64 + i] - host(i)) > 1e-4f) throw fs::Error("pf_reduce<4> value " + std::to_string(i) + " wrong");
    if (std::fabs(out[68] - host(0)) > 1e-4f) throw fs::Error("pf_wave_sum wrong");
}
int fs_selftest(int device_id, const char* what) {
    FS_ARG(what, "null argument");
    FS_TRY({
        if (std::strcmp(what, "pf_reduce") == 0) selftest_pf_reduce(device_id);
        else throw fs::Error(std::string("unknown self-test: ") + what);
    })
}

int fs_selftest_sample_rows(int device_id, const float* logits, int B, int n, const fs_sampling* s, uint64_t seed, int call_index, uint32_t* out) {
    FS_ARG(logits && s && out, "null argument");
    FS_TRY(fs::debug_sample_rows(device_id, logits, B, n, s->temp, s->top_p, s->top_k, seed, call_index, out))
}

int fs_selftest_sample_slots(int device_id, const float* logits, int S, int R, int n, const fs_sampling* samplings, const uint64_t* seeds,
                             uint32_t* out, uint64_t* words_used) {
    FS_ARG(logits && samplings && seeds && out && words_used, "null argument");
    FS_ARG(S >= 1 && R >= 1 && n >= 1 && n <= 2048, "bad sampler test shape (S, R >= 1; 1 <= n <= 2048)");
    FS_TRY({
        std::vector<fs::SampleCfg> cfgs((size_t)S);
        for (int i = 0; i < S; ++i) {
            const fs_sampling& sa = samplings[i];
            if (!std::isfinite(sa.temp) || sa.temp < 0.0) throw fs::Error("fs_selftest_sample_slots: temp must be finite and >= 0");
            if (!std::isfinite(sa.top_p)) throw fs::Error("fs_selftest_sample_slots: top_p must be finite");
            fs::SampleCfg c = {};
            c.temp = (float)sa.temp; c.top_p = (float)sa.top_p; c.top_p64 = sa.top_p;
            c.top_k = (int)std::min<uint64_t>(sa.top_k, 1u << 30);
            c.rep_pen = 1.f;
            cfgs[(size_t)i] = c;
        }
        fs::debug_sample_slots(device_id, logits, S, R, n, cfgs.data(), seeds, out, words_used);
    })
}
int fs_selftest_score_rows(int device_id, const float* logits, int S, int n, const uint32_t* targets, int exclude0, float* logprob_out,
                           float* top_logprob_out, uint32_t* top_out, float* row_out) {
    FS_ARG(logits && targets, "null argument");
    FS_ARG(S >= 1 && n >= 2 && n <= 2048, "bad score test shape (S >= 1; 2 <= n <= 2048)");
    FS_TRY(fs::debug_score_rows(device_id, logits, S, n, targets, exclude0, logprob_out, top_logprob_out, top_out, row_out))
}
int fs_selftest_alt_rows(int device_id, const float* logits, int S, int n, int exclude0, int n_alts, uint32_t* alt_index_out, float* alt_logprob_out,
                         float* entropy_out) {
    FS_ARG(logits, "null argument");
    FS_ARG(S >= 1 && n >= 2 && n <= 2048, "bad alternatives test shape (S >= 1; 2 <= n <= 2048)");
    FS_ARG(n_alts >= 1 && n_alts <= (int)FS_ALTS_MAX, "bad alternatives test shape (1 <= n_alts <= 16)");
    FS_TRY(fs::debug_alt_rows(device_id, logits, S, n, exclude0, n_alts, alt_index_out, alt_logprob_out, entropy_out))
}
static_assert(sizeof(fs_conv_case) == 16 * 4 + 11 * 8, "fs_conv_case is 16 x int32 and 11 pointers (fishrt/_ffi.py: ConvCase)");
int fs_selftest_conv1d(int device_id, const fs_conv_case* c, float* y_out, float* planes_out, char* variant_out, size_t variant_cap,
                       uint64_t* range_out) {
    FS_ARG(c && variant_out && variant_cap >= 1, "null argument");
    variant_out[0] = 0;
    FS_TRY(fs::codec_conv_selftest(device_id, *c, y_out, planes_out, variant_out, variant_cap, range_out))
}
static_assert(sizeof(fs_codec_op_case) == 16 * 4 + 8 + 8 * 8, "fs_codec_op_case is 16 x int32, one int64 and 8 pointers (fishrt/_ffi.py: CodecOpCase)");
int fs_selftest_codec_op(int device_id, const fs_codec_op_case* c, void* out, size_t out_cap, size_t* n_out, int* guard_ok) {
    FS_ARG(c && out && n_out && guard_ok, "null argument");
    *n_out = 0; *guard_ok = 0;
    FS_TRY(fs::codec_op_selftest(device_id, *c, out, out_cap, n_out, guard_ok))
}
static_assert(sizeof(fs_attn_case) == 32 * 4 + 13 * 8, "fs_attn_case is 30 x int32, one float, one int32 and 13 pointers (fishrt/_ffi.py: AttnCase)");
int fs_selftest_attn(int device_id, const fs_attn_case* c, float* out, size_t out_cap, size_t* n_out, float* k_out, float* v_out,
                     char* variant_out, size_t variant_cap, int* guard_ok) {
    FS_ARG(c && n_out && variant_out && variant_cap >= 1 && guard_ok, "null argument");
    *n_out = 0; *guard_ok = 0; variant_out[0] = 0;
    FS_TRY(fs::attn_selftest(device_id, *c, out, out_cap, n_out, k_out, v_out, variant_out, variant_cap, guard_ok))
}
static_assert(sizeof(fs_gemm_case) == 36 * 4 + 18 * 8, "fs_gemm_case is 34 x int32, one float, one int32 and 18 pointers (fishrt/_ffi.py: GemmCase)");
static_assert(sizeof(fs_gemm_out) == 7 * 8 + 8 * 8 + 4 * 4, "fs_gemm_out is 7 pointers, 8 x size_t and 4 x int32 (fishrt/_ffi.py: GemmOut)");
int fs_selftest_gemm(int device_id, const fs_gemm_case* c, fs_gemm_out* out) {
    FS_ARG(c && out && out->variant && out->variant_cap >= 1, "null argument");
    out->variant[0] = 0; out->guard_ok = 0; out->n_y = out->n_planes = out->n_ss = 0;
    out->grid[0] = out->grid[1] = out->grid[2] = 0;
    FS_TRY(fs::gemm_selftest(device_id, *c, *out))
}
static_assert(sizeof(fs_gemv_case) == 28 * 4 + 14 * 8, "fs_gemv_case is 24 x int32, two uint32, one float, one int32 and 14 pointers (fishrt/_ffi.py: GemvCase)");
static_assert(sizeof(fs_gemv_out) == 4 * 8 + 5 * 8 + 4 * 4, "fs_gemv_out is 4 pointers, 5 x size_t and 4 x int32 (fishrt/_ffi.py: GemvOut)");
int fs_selftest_gemv(int device_id, const fs_gemv_case* c, fs_gemv_out* out) {
    FS_ARG(c && out && out->variant && out->variant_cap >= 1, "null argument");
    out->variant[0] = 0; out->guard_ok = 0; out->n_y = out->n_pool = 0;
    out->grid[0] = out->grid[1] = out->grid[2] = 0;
    FS_TRY(fs::gemv_selftest(device_id, *c, *out))
}
static_assert(sizeof(fs_sample_case) == 28 * 4 + 10 * 8, "fs_sample_case is 20 x int32, one float, one int32, the 5-word token layout, one int32 and 10 pointers (fishrt/_ffi.py: SampleCase)");
static_assert(sizeof(fs_sample_out) == 3 * 13 * 8 + 2 * 4, "fs_sample_out is 13 pointers, 2 x 13 size_t and 2 x int32 (fishrt/_ffi.py: SampleOut)");
int fs_selftest_sample_frames(int device_id, const fs_sample_case* c, fs_sample_out* out) {
    FS_ARG(c && out, "null argument");
    out->n_launches = 0; out->guard_ok = 0;
    for (int i = 0; i < FS_SAMPLE_OUT_COUNT; ++i) out->need[i] = 0;
    FS_TRY(fs::sample_frames_selftest(device_id, *c, *out))
}

// ---- replica fan-out over RCCL (fs_comm.h)
int fs_comm_unique_id(uint8_t id_out[FS_COMM_ID_BYTES]) { FS_ARG(id_out, "null argument"); FS_TRY(fs::Comm::unique_id(id_out)) }
int fs_comm_create(const uint8_t id[FS_COMM_ID_BYTES], int rank, int world, int device_id, fs_comm_t** out) {
    FS_ARG(id && out, "null argument");
    FS_TRY({ *out = nullptr; fs::Comm* c = new fs::Comm(id, rank, world, device_id); *out = new fs_comm{c}; })
}
void fs_comm_destroy(fs_comm_t* c) {
    if (!c) return;
    delete c->impl;
    delete c;
}
int fs_comm_rank(fs_comm_t* c) { if (!c) { g_err = "null argument"; return -1; } return c->impl->rank(); }
int fs_comm_world(fs_comm_t* c) { if (!c) { g_err = "null argument"; return -1; } return c->impl->world(); }
int fs_comm_barrier(fs_comm_t* c) { FS_ARG(c, "null argument"); FS_TRY(c->impl->barrier()) }
int fs_comm_all_reduce_f64(fs_comm_t* c, double* vals, int n, int op) { FS_ARG(c && vals, "null argument"); FS_TRY(c->impl->all_reduce_f64(vals, n, op)) }
int fs_comm_broadcast_weights(fs_comm_t* c, fs_lm_t* lm, int src, size_t* bytes_moved) {
    FS_ARG(c && lm, "null argument");
    FS_TRY({ const size_t n = c->impl->broadcast_weights(lm->impl, src); if (bytes_moved) *bytes_moved = n; })
}
int fs_comm_broadcast_prompt_dims(fs_comm_t* c, int64_t dims[3], int src) {
    FS_ARG(c && dims, "null argument");
    FS_TRY(c->impl->broadcast_host(dims, 3 * sizeof(int64_t), src))
}
int fs_comm_broadcast_prompts(fs_comm_t* c, uint32_t* packed, int32_t* lens, const int64_t dims[3], int src) {
    FS_ARG(c && packed && lens && dims, "null argument");
    FS_ARG(dims[0] >= 0 && dims[1] >= 1 && dims[2] >= 0 && dims[0] <= (1 << 20) && dims[1] <= 64 && dims[2] <= (1 << 20), "bad prompt batch shape");
    FS_TRY({
        c->impl->broadcast_host(packed, (size_t)dims[0] * (size_t)dims[1] * (size_t)dims[2] * sizeof(uint32_t), src);
        c->impl->broadcast_host(lens, (size_t)dims[0] * sizeof(int32_t), src);
    })
}
int fs_comm_all_gather_codes(fs_comm_t* c, const uint32_t* codes, const int32_t* n_frames, int B, int C, int N, uint32_t* codes_all, int32_t* n_frames_all) {
    FS_ARG(c && codes && n_frames && codes_all && n_frames_all, "null argument");
    FS_ARG(B >= 1 && C >= 1 && N >= 0, "bad code array shape");
    FS_TRY({
        c->impl->all_gather_host(codes, codes_all, (size_t)B * (size_t)C * (size_t)N * sizeof(uint32_t));
        c->impl->all_gather_host(n_frames, n_frames_all, (size_t)B * sizeof(int32_t));
    })
}

int fs_lm_selftest(fs_lm_t* lm, const char* what) { FS_ARG(lm && what, "null argument"); FS_TRY(lm->impl->selftest(what)) }
int fs_lm_debug_capture(fs_lm_t* lm, int n_frames) { FS_ARG(lm, "null argument"); FS_TRY(lm->impl->debug_capture(n_frames)) }
int fs_lm_debug_read(fs_lm_t* lm, float* out, int n_frames) { FS_ARG(lm && out, "null argument"); FS_TRY(lm->impl->debug_read(out, n_frames)) }

int fs_lm_create(const fs_model_args* args, const fs_token_cfg* tok, int device_id, fs_dtype dtype, int max_batch, fs_lm_t** out) {
    FS_ARG(args && tok && out, "null argument");
    FS_TRY({ *out = nullptr; fs::LMBase* p = fs::make_lm(*args, *tok, device_id, dtype, max_batch); *out = new fs_lm{p}; })
}
void fs_lm_destroy(fs_lm_t* lm) {
    if (!lm) return;
    delete lm->impl;
    delete lm;
}
int fs_lm_load_safetensors(fs_lm_t* lm, const char* path) { FS_ARG(lm && path, "null argument"); FS_TRY(lm->impl->load_safetensors(path)) }
int fs_lm_load_synthetic(fs_lm_t* lm, uint64_t seed) { FS_ARG(lm, "null argument"); FS_TRY(lm->impl->load_synthetic(seed)) }
int fs_lm_forward_generate(fs_lm_t* lm, const uint32_t* toks, int B, int L, int input_pos, float* logits_out, float* hidden_out) {
    FS_ARG(lm && toks, "null argument");
    FS_ARG(input_pos >= 0, "negative input_pos");
    FS_TRY(lm->impl->forward_generate(toks, B, L, input_pos, logits_out, hidden_out))
}
int fs_lm_forward_generate_fast(fs_lm_t* lm, const float* x, int B, int input_pos, float* logits_out) {
    FS_ARG(lm && x && logits_out, "null argument");
    FS_ARG(input_pos >= 0, "negative input_pos");
    FS_TRY(lm->impl->forward_generate_fast(x, B, input_pos, logits_out))
}
int fs_lm_fast_embed(fs_lm_t* lm, const uint32_t* ids, int n, float* out) {
    FS_ARG(lm && ids && out && n > 0, "bad argument");
    FS_TRY(lm->impl->fast_embed(ids, n, out))
}
int fs_lm_clear_fast_layer_caches(fs_lm_t* lm) { FS_ARG(lm, "null argument"); FS_TRY(lm->impl->clear_fast()) }
int fs_lm_clear_slow_layer_caches(fs_lm_t* lm) { FS_ARG(lm, "null argument"); FS_TRY(lm->impl->clear_slow()) }
int fs_lm_clear_slow_caches_until(fs_lm_t* lm, int pos) { FS_ARG(lm, "null argument"); FS_TRY(lm->impl->clear_slow_until(pos)) }
int fs_lm_curr_kv_size(fs_lm_t* lm) {
    if (!lm) { g_err = "null argument"; return -1; }
    try { return lm->impl->kv_len(); } catch (const std::exception& e) { g_err = e.what(); return -1; }
}
int fs_lm_generate(fs_lm_t* lm, const uint32_t* prompt, int L, int max_new_tokens, const fs_sampling* sampling, uint64_t seed,
                   uint32_t flags, uint32_t* codes_out, size_t cap, size_t* n_frames, fs_frame_cb cb, void* cb_user) {
    FS_ARG(lm && prompt && sampling && n_frames, "null argument");
    FS_TRY(lm->impl->generate(prompt, L, max_new_tokens, *sampling, seed, flags, codes_out, cap, n_frames, cb, cb_user))
}
int fs_lm_generate_with_hidden(fs_lm_t* lm, const uint32_t* prompt, int L, int max_new_tokens, const fs_sampling* sampling, uint64_t seed,
                               uint32_t flags, uint32_t* codes_out, size_t cap, size_t* n_frames, float* hidden_out, size_t hidden_cap,
                               size_t* n_hidden, fs_frame_cb cb, void* cb_user) {
    FS_ARG(lm && prompt && sampling && n_frames, "null argument");
    FS_ARG(!hidden_out || n_hidden, "hidden_out without n_hidden");
    FS_TRY(lm->impl->generate(prompt, L, max_new_tokens, *sampling, seed, flags, codes_out, cap, n_frames, cb, cb_user, hidden_out,
                              hidden_cap, n_hidden))
}
int fs_lm_generate_batch(fs_lm_t* lm, const uint32_t* prompts, const int* lens, int n, int max_new_tokens, const fs_sampling* sampling,
                         uint64_t seed, uint32_t flags, uint32_t* codes_out, size_t cap, size_t* n_frames) {
    FS_ARG(lm && prompts && lens && sampling && codes_out && n_frames, "null argument");
    FS_TRY(lm->impl->generate_batch(prompts, lens, n, max_new_tokens, *sampling, seed, flags, codes_out, cap, n_frames))
}
int fs_lm_generate_static_batch(fs_lm_t* lm, const uint32_t* prompts, const int* lens, int n, int max_new_tokens, int audio_only,
                                const fs_sampling* sampling, uint64_t seed, uint32_t flags, uint32_t* codes_out, size_t cap, size_t* n_frames,
                                uint8_t* is_audio_out) {
    FS_ARG(lm && prompts && lens && sampling && codes_out && n_frames, "null argument");
    FS_ARG(audio_only != 0, "generate_static_batch(audio_only = false) is not implemented: the reference then samples the slow token over the FULL "
                            "vocabulary, never terminates a row and keeps the slow-token row in its outputs (static_batch.rs:132-141,156-173,361-364); "
                            "its server always passes true (server/lib/handlers/speech.rs:80-86)");
    FS_TRY(lm->impl->generate_batch(prompts, lens, n, max_new_tokens, *sampling, seed, flags, codes_out, cap, n_frames, is_audio_out))
}
int fs_lm_generate_multi(fs_lm_t* lm, const uint32_t* prompts, const int* lens, int n, const int* max_new_tokens, const fs_sampling* samplings,
                         const uint64_t* seeds, uint32_t flags, uint32_t* codes_out, size_t cap, size_t* n_frames) {
    FS_ARG(lm && prompts && lens && max_new_tokens && samplings && seeds && codes_out && n_frames, "null argument");
    FS_TRY(lm->impl->generate_multi(prompts, lens, n, max_new_tokens, samplings, seeds, flags, codes_out, cap, n_frames))
}
int fs_lm_rows_supported(fs_lm_t* lm, int n, const fs_sampling* samplings, int* supported) {
    FS_ARG(lm && samplings && supported && n >= 1, "bad argument");
    FS_TRY(*supported = lm->impl->rows_supported(n, samplings) ? 1 : 0)
}
int fs_lm_debug_read_row(fs_lm_t* lm, int row, float* out, int n_frames) { FS_ARG(lm && out, "null argument"); FS_TRY(lm->impl->debug_read_row(row, out, n_frames)) }
int fs_lm_debug_read_kv(fs_lm_t* lm, int slot, int layer, int t0, int n, float* k_out, float* v_out) {
    FS_ARG(lm && k_out && v_out, "null argument");
    FS_TRY(lm->impl->debug_read_kv(slot, layer, t0, n, k_out, v_out))
}
int fs_lm_weights_arena(fs_lm_t* lm, void** dev_ptr, size_t* bytes) {
    FS_ARG(lm && dev_ptr && bytes, "null argument");
    FS_TRY(lm->impl->weights_arena(dev_ptr, bytes))
}
int fs_lm_weights_adopt(fs_lm_t* lm) { FS_ARG(lm, "null argument"); FS_TRY(lm->impl->weights_adopt()) }
int fs_lm_session_begin(fs_lm_t* lm, const fs_sampling* sampling, uint64_t seed, uint32_t flags) {
    FS_ARG(lm && sampling, "null argument");
    FS_TRY(lm->impl->session_begin(*sampling, seed, flags))
}
// the six fs_lm_session_add* entry points fill one request (lm_engine.h: SlotRequest); what is not set here stays off
static fs::SlotRequest slot_request(int prefix_id, const uint32_t* prompt, int L, int max_new_tokens, const fs_sampling* sampling, const uint64_t* seed) {
    fs::SlotRequest r;
    r.prefix_id = prefix_id; r.prompt = prompt; r.L = L; r.max_new_tokens = max_new_tokens; r.sampling = sampling; r.seed = seed;
    return r;
}
int fs_lm_session_add(fs_lm_t* lm, const uint32_t* prompt, int L, int max_new_tokens, int* slot) {
    FS_ARG(lm && prompt && slot, "null argument");
    FS_TRY(*slot = lm->impl->session_admit(slot_request(-1, prompt, L, max_new_tokens, nullptr, nullptr)))
}
int fs_lm_session_step(fs_lm_t* lm, int n_frames, int* n_active) { FS_ARG(lm, "null argument"); FS_TRY(lm->impl->session_step(n_frames, n_active)) }
int fs_lm_session_poll(fs_lm_t* lm, int slot, uint32_t* codes_out, size_t cap, size_t* n_frames, int* done) {
    FS_ARG(lm, "null argument");
    FS_TRY(lm->impl->session_poll(slot, codes_out, cap, n_frames, done))
}
int fs_lm_session_release(fs_lm_t* lm, int slot) { FS_ARG(lm, "null argument"); FS_TRY(lm->impl->session_release(slot)) }
int fs_lm_session_end(fs_lm_t* lm) { FS_ARG(lm, "null argument"); FS_TRY(lm->impl->session_end()) }
int fs_lm_session_prefix_create(fs_lm_t* lm, const uint32_t* prompt, int P, int* prefix_id) {
    FS_ARG(lm && prompt && prefix_id, "null argument");
    FS_TRY(*prefix_id = lm->impl->session_prefix_create(prompt, P))
}
static_assert(sizeof(fs_kv_blob_header) == 64, "fs_kv_blob_header is the 64-byte blob header of fishrt.h");
int fs_lm_weights_fingerprint(fs_lm_t* lm, uint64_t* out) {
    FS_ARG(lm && out, "null argument");
    FS_TRY(*out = lm->impl->weights_fingerprint())
}
int fs_lm_session_prefix_export(fs_lm_t* lm, int prefix_id, void* blob_out, size_t cap, size_t* bytes) {
    FS_ARG(lm, "null argument");
    FS_TRY(lm->impl->session_prefix_export(prefix_id, blob_out, cap, bytes))
}
int fs_lm_session_prefix_import(fs_lm_t* lm, const void* blob, size_t bytes, int* prefix_id) {
    FS_ARG(lm && blob && prefix_id, "null argument");
    FS_TRY(*prefix_id = lm->impl->session_prefix_import(blob, bytes))
}
int fs_lm_session_prefix_release(fs_lm_t* lm, int prefix_id) { FS_ARG(lm, "null argument"); FS_TRY(lm->impl->session_prefix_release(prefix_id)) }
int fs_lm_session_prefix_from_slot(fs_lm_t* lm, int slot, int n_positions, int* prefix_id, int* P_out) {
    FS_ARG(lm && prefix_id, "null argument");
    FS_TRY(*prefix_id = lm->impl->session_prefix_from_slot(slot, n_positions, P_out))
}
int fs_lm_session_last_frame(fs_lm_t* lm, int slot, uint32_t* column) {
    FS_ARG(lm && column, "null argument");
    FS_TRY(lm->impl->session_last_frame(slot, column))
}
int fs_lm_session_add_prefixed(fs_lm_t* lm, int prefix_id, const uint32_t* body, int L_body, int max_new_tokens, int* slot) {
    FS_ARG(lm && body && slot, "null argument");
    FS_ARG(prefix_id >= 0, "unknown or released prefix id");  // (a negative id means a plain add only where the header says so: _add_ex and later)
    FS_TRY(*slot = lm->impl->session_admit(slot_request(prefix_id, body, L_body, max_new_tokens, nullptr, nullptr)))
}
int fs_lm_session_add_ex(fs_lm_t* lm, int prefix_id, const uint32_t* prompt, int L, int max_new_tokens, const fs_sampling* sampling,
                         const uint64_t* seed, int* slot) {
    FS_ARG(lm && prompt && slot, "null argument");
    FS_TRY(*slot = lm->impl->session_admit(slot_request(prefix_id, prompt, L, max_new_tokens, sampling, seed)))
}
int fs_lm_session_add_hidden(fs_lm_t* lm, int prefix_id, const uint32_t* prompt, int L, int max_new_tokens, const fs_sampling* sampling,
                             const uint64_t* seed, int* slot) {
    FS_ARG(lm && prompt && slot, "null argument");
    fs::SlotRequest r = slot_request(prefix_id, prompt, L, max_new_tokens, sampling, seed);
    r.collect_hidden = true;
    FS_TRY(*slot = lm->impl->session_admit(r))
}
int fs_lm_session_poll_hidden(fs_lm_t* lm, int slot, size_t first_row, float* hidden_out, size_t cap_rows, size_t* n_rows) {
    FS_ARG(lm, "null argument");
    FS_TRY(lm->impl->session_poll_hidden(slot, first_row, hidden_out, cap_rows, n_rows))
}
int fs_lm_session_add_scored(fs_lm_t* lm, int prefix_id, const uint32_t* prompt, int L, const uint32_t* frames, int N, int collect_hidden,
                             int* slot) {
    FS_ARG(lm && prompt && frames && slot, "null argument");
    fs::SlotRequest r = slot_request(prefix_id, prompt, L, 0, nullptr, nullptr);
    r.frames = frames; r.N = N; r.collect_hidden = collect_hidden != 0;
    FS_TRY(*slot = lm->impl->session_admit(r))
}
int fs_lm_session_poll_scores(fs_lm_t* lm, int slot, size_t first_row, float* logprob, float* top_logprob, uint32_t* top, float* eos_logprob,
                              size_t cap_rows, size_t* n_rows) {
    FS_ARG(lm, "null argument");
    FS_TRY(lm->impl->session_poll_scores(slot, first_row, logprob, top_logprob, top, eos_logprob, cap_rows, n_rows))
}
int fs_lm_session_add_traced(fs_lm_t* lm, int prefix_id, const uint32_t* prompt, int L, int max_new_tokens, const fs_sampling* sampling,
                             const uint64_t* seed, int collect_hidden, int* slot) {
    FS_ARG(lm && prompt && slot, "null argument");
    fs::SlotRequest r = slot_request(prefix_id, prompt, L, max_new_tokens, sampling, seed);
    r.traced = true; r.collect_hidden = collect_hidden != 0;
    FS_TRY(*slot = lm->impl->session_admit(r))
}
int fs_lm_session_poll_trace(fs_lm_t* lm, int slot, size_t first_row, uint32_t* tokens, float* logprob, float* top_logprob, uint32_t* top,
                             float* eos_logprob, int* n_decisions, size_t cap_rows, size_t* n_rows) {
    FS_ARG(lm, "null argument");
    FS_TRY(lm->impl->session_poll_trace(slot, first_row, tokens, logprob, top_logprob, top, eos_logprob, n_decisions, cap_rows, n_rows))
}
int fs_lm_session_poll_alts(fs_lm_t* lm, int slot, size_t first_row, uint32_t* alt_index, float* alt_logprob, float* entropy, size_t cap_rows,
                            size_t* n_rows, int* n_alts) {
    FS_ARG(lm, "null argument");
    FS_TRY(lm->impl->session_poll_alts(slot, first_row, alt_index, alt_logprob, entropy, cap_rows, n_rows, n_alts))
}
int fs_lm_session_info(fs_lm_t* lm, int64_t out[8]) { FS_ARG(lm && out, "null argument"); FS_TRY(lm->impl->session_info(out)) }
int fs_lm_last_stats(fs_lm_t* lm, fs_gen_stats* out) { FS_ARG(lm && out, "null argument"); FS_TRY(*out = lm->impl->last_stats()) }
void* fs_lm_stream(fs_lm_t* lm) { return lm ? lm->impl->stream() : nullptr; }
int fs_lm_bench_kernel(fs_lm_t* lm, int kind, int kv_len, int reps, float* us_per_launch) {
    FS_ARG(lm && us_per_launch, "null argument");
    FS_TRY(*us_per_launch = lm->impl->bench_kernel(kind, kv_len, reps))
}

int fs_codec_create(int device_id, int channel_div, fs_codec_t** out) {
    FS_ARG(out, "null argument");
    FS_TRY({ *out = nullptr; fs::CodecBase* p = fs::make_codec(device_id, channel_div); *out = new fs_codec{p}; })
}
void fs_codec_destroy(fs_codec_t* c) {
    if (!c) return;
    delete c->impl;
    delete c;
}
int fs_codec_load_safetensors(fs_codec_t* c, const char* path) { FS_ARG(c && path, "null argument"); FS_TRY(c->impl->load_safetensors(path)) }
int fs_codec_load_synthetic(fs_codec_t* c, uint64_t seed) { FS_ARG(c, "null argument"); FS_TRY(c->impl->load_synthetic(seed)) }
int fs_codec_decode(fs_codec_t* c, const uint32_t* codes, int b, int T, float* pcm_out) {
    FS_ARG(c && codes && pcm_out, "null argument");
    FS_TRY(c->impl->decode(codes, b, T, pcm_out))
}
int fs_codec_encode(fs_codec_t* c, const float* pcm, int n_samples, uint32_t* codes_out, size_t cap, size_t* n_frames) {
    FS_ARG(c && pcm && codes_out && n_frames, "null argument");
    FS_ARG(n_samples > 0, "empty input");
    FS_TRY(c->impl->encode(pcm, n_samples, codes_out, cap, n_frames))
}
int fs_selftest_codec_encode_stage(fs_codec_t* c, const float* pcm, int n_samples, int stage, float* out, size_t cap, size_t* n_out) {
    FS_ARG(c && out && n_out && (pcm || stage == -2), "null argument");
    FS_ARG(stage >= -2 && stage <= 6, "encoder stage tap: stage is -2 (mel table), -1 (log-mel) or 0 .. 6");
    FS_ARG(stage == -2 || n_samples > 0, "empty input");
    *n_out = 0;
    FS_TRY(c->impl->encode_stage(pcm, n_samples, stage, out, cap, n_out))
}
int fs_codec_encode_batch(fs_codec_t* c, const float* pcm, int b, size_t stride, const int* n_samples, uint32_t* codes_out, size_t cap, size_t* n_frames) {
    FS_ARG(c && pcm && n_samples && codes_out && n_frames, "null argument");
    FS_ARG(b >= 1, "empty batch");
    for (int i = 0; i < b; ++i) FS_ARG(n_samples[i] > 0 && (size_t)n_samples[i] <= stride, "clip length outside (0, stride]");
    FS_TRY({
        for (int i = 0; i < b; ++i) c->impl->encode(pcm + (size_t)i * stride, n_samples[i], codes_out + (size_t)i * 8 * cap, cap, &n_frames[i]);
    })
}
int fs_codec_sample_rate(fs_codec_t* c) { return c ? c->impl->sample_rate() : -1; }
int fs_codec_stream_begin(fs_codec_t* c) { FS_ARG(c, "null argument"); FS_TRY(c->impl->stream_begin()) }
int fs_codec_stream_decode(fs_codec_t* c, const uint32_t* codes, int T, float* pcm_out) {
    FS_ARG(c && codes && pcm_out, "null argument");
    FS_TRY(c->impl->stream_decode(codes, T, pcm_out))
}
int fs_codec_stream_end(fs_codec_t* c) { FS_ARG(c, "null argument"); FS_TRY(c->impl->stream_end()) }
int fs_codec_streams_open(fs_codec_t* c, int* stream_id) {
    FS_ARG(c && stream_id, "null argument");
    FS_TRY(*stream_id = c->impl->streams_open())
}
int fs_codec_streams_close(fs_codec_t* c, int stream_id) { FS_ARG(c, "null argument"); FS_TRY(c->impl->streams_close(stream_id)) }
int fs_codec_streams_decode(fs_codec_t* c, int n, const int* stream_ids, const uint32_t* codes, int T, float* pcm_out) {
    FS_ARG(c && stream_ids && codes && pcm_out, "null argument");
    FS_TRY(c->impl->streams_decode(n, stream_ids, codes, T, pcm_out))
}
int fs_codec_streams_decode_ragged(fs_codec_t* c, int n, const int* stream_ids, const int* T, const uint32_t* codes, float* pcm_out) {
    FS_ARG(c && stream_ids && T && codes && pcm_out, "null argument");
    FS_TRY(c->impl->streams_decode_ragged(n, stream_ids, T, codes, pcm_out))
}
static_assert(sizeof(fs_pcm_spec) == 3 * sizeof(int32_t), "fs_pcm_spec is passed to the engine as int[3]");
int fs_resample_out_len(int from_rate, int to_rate, int mode, int64_t n, int64_t* out_len) {
    FS_ARG(out_len, "null argument");
    FS_ARG(mode == FS_RESAMPLE_LINEAR || mode == FS_RESAMPLE_SINC, "mode is FS_RESAMPLE_LINEAR or FS_RESAMPLE_SINC");
    FS_ARG(n >= 0 && n < ((int64_t)1 << 40), "n out of range");
    FS_TRY(*out_len = fs::resample_out_len(fs::resample_rates(from_rate, to_rate), mode, n))
}
int fs_resample(int device_id, const float* pcm, int b, size_t stride, const int64_t* n_samples, int from_rate, const fs_pcm_spec* out,
                void* out_buf, size_t out_stride, int64_t* out_len) {
    FS_ARG(pcm && n_samples && out && out_buf && out_len, "null argument");
    FS_TRY(fs::resample_rows(device_id, pcm, b, stride, n_samples, from_rate, &out->rate, out_buf, out_stride, out_len))
}
int fs_codec_decode_pcm(fs_codec_t* c, const uint32_t* codes, int b, int T, const fs_pcm_spec* spec, void* out, size_t cap, int64_t* n_out) {
    FS_ARG(c && codes && spec && out && n_out, "null argument");
    FS_TRY(c->impl->decode_pcm(codes, b, T, &spec->rate, out, cap, n_out))
}
static_assert(sizeof(fs_tsm_params) == 2 * sizeof(int32_t), "fs_tsm_params is passed to the engine as int[2]");
int fs_time_stretch_out_len(int64_t n, double speed, int64_t* out_len) {
    FS_ARG(out_len, "null argument");
    FS_ARG(n >= 0 && n < ((int64_t)1 << 40), "n out of range");
    FS_TRY(fs::tsm_require_speed(speed); *out_len = fs::tsm_out_len(n, speed))
}
int fs_time_stretch(int device_id, const float* pcm, int b, size_t stride, const int64_t* n_samples, double speed, const fs_tsm_params* params,
                    float* out, size_t out_stride, int64_t* out_len, int64_t* positions, size_t pos_stride) {
    FS_ARG(pcm && n_samples && out && out_len, "null argument");
    FS_TRY(fs::time_stretch_rows(device_id, pcm, b, stride, n_samples, speed, params ? &params->frame : nullptr, out, out_stride, out_len, positions,
                                 pos_stride))
}
int fs_codec_decode_speed(fs_codec_t* c, const uint32_t* codes, int b, int T, double speed, const fs_pcm_spec* spec, void* out, size_t cap,
                          int64_t* n_out) {
    FS_ARG(c && codes && spec && out && n_out, "null argument");
    FS_TRY(c->impl->decode_speed(codes, b, T, speed, &spec->rate, out, cap, n_out))
}
int fs_codec_streams_open_speed(fs_codec_t* c, double speed, const fs_pcm_spec* spec, int* stream_id) {
    FS_ARG(c && stream_id, "null argument");
    FS_TRY(*stream_id = c->impl->streams_open_speed(speed, spec ? &spec->rate : nullptr))
}
int fs_selftest_tsm_chunks(int device_id, const float* pcm, int64_t n, const int64_t* chunk_len, int n_chunks, double speed,
                           const fs_tsm_params* params, float* out, size_t out_cap, int64_t* out_len, int64_t* emitted, int64_t* positions,
                           size_t pos_cap, int64_t* n_positions) {
    FS_ARG((pcm || n == 0) && chunk_len && out && out_len && emitted, "null argument");
    FS_TRY(fs::time_stretch_chunks(device_id, pcm, n, chunk_len, n_chunks, speed, params ? &params->frame : nullptr, out, out_cap, out_len, emitted,
                                   positions, pos_cap, n_positions))
}
static_assert(sizeof(fs_loud_params) == 3 * sizeof(double), "fs_loud_params is passed to the engine as double[3]");
static_assert(sizeof(fs_loud_result) == sizeof(fs::LoudResult) && offsetof(fs_loud_result, gain) == offsetof(fs::LoudResult, gain) &&
                  offsetof(fs_loud_result, blocks_kept) == offsetof(fs::LoudResult, blocks_kept),
              "fs_loud_result is the engine's record");
int fs_loudness_normalize(int device_id, const float* pcm, int b, size_t stride, const int64_t* n_samples, int rate, const fs_loud_params* params,
                          float* out, size_t out_stride, fs_loud_result* res) {
    FS_ARG(pcm && n_samples && res, "null argument");
    FS_TRY(fs::loudness_rows(device_id, pcm, b, stride, n_samples, rate, params ? &params->target_lufs : nullptr, out, out_stride, res, nullptr, 0,
                             nullptr))
}
int fs_codec_decode_loud(fs_codec_t* c, const uint32_t* codes, int b, int T, const fs_loud_params* loud, double speed, const fs_pcm_spec* spec,
                         void* out, size_t cap, int64_t* n_out, fs_loud_result* res) {
    FS_ARG(c && codes && spec && out && n_out, "null argument");
    FS_TRY(c->impl->decode_loud(codes, b, T, loud ? &loud->target_lufs : nullptr, speed, &spec->rate, out, cap, n_out, res))
}
int fs_selftest_loud_hops(int device_id, const float* pcm, int64_t n, int rate, double* hops, size_t cap, int64_t* n_hops, fs_loud_result* res) {
    FS_ARG(pcm && hops && n_hops && res, "null argument");
    FS_TRY(fs::loudness_rows(device_id, pcm, 1, (size_t)n, &n, rate, nullptr, nullptr, 0, res, hops, cap, n_hops))
}
int fs_codec_streams_open_pcm(fs_codec_t* c, const fs_pcm_spec* spec, int* stream_id) {
    FS_ARG(c && spec && stream_id, "null argument");
    FS_TRY(*stream_id = c->impl->streams_open_pcm(&spec->rate))
}
int fs_codec_streams_pending(fs_codec_t* c, int stream_id, int T, int final, int64_t* n_out) {
    FS_ARG(c && n_out, "null argument");
    FS_TRY(*n_out = c->impl->streams_pending(stream_id, T, final != 0))
}
int fs_codec_streams_decode_pcm(fs_codec_t* c, int n, const int* stream_ids, const int* T, const uint8_t* final, const uint32_t* codes, void* out,
                                size_t cap_bytes, int64_t* n_out) {
    FS_ARG(c && stream_ids && T && n_out && (out || cap_bytes == 0), "null argument");
    FS_TRY(c->impl->streams_decode_pcm(n, stream_ids, T, final, codes, out, cap_bytes, n_out))
}
int fs_codec_encode_pcm(fs_codec_t* c, const float* pcm, int channels, int64_t frames, int rate, int mode, uint32_t* codes_out, size_t cap,
                        size_t* n_frames) {
    FS_ARG(c && pcm && codes_out && n_frames, "null argument");
    FS_TRY(c->impl->encode_pcm(pcm, channels, frames, rate, mode, codes_out, cap, n_frames))
}
int fs_codec_set_precision(fs_codec_t* c, int mode) { FS_ARG(c, "null argument"); FS_TRY(c->impl->set_precision(mode)) }
int fs_codec_precision(fs_codec_t* c) { return c ? c->impl->precision() : -1; }
int fs_codec_set_range_check(fs_codec_t* c, int on) { FS_ARG(c, "null argument"); FS_TRY(c->impl->set_range_check(on != 0)) }
int fs_codec_range_stats(fs_codec_t* c, uint64_t* out5, double* last_pcm_rms_diff) {
    FS_ARG(c && out5, "null argument");
    FS_TRY(c->impl->range_stats(out5, last_pcm_rms_diff))
}

}  // extern "C"
