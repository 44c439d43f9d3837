// Host-side engine of the Firefly-GAN-VQ vocoder: FireflyCodec::decode (fish_speech_core/lib/codec/firefly.rs:42-48)
//   -> FireflyDecoder::decode (decoder.rs:37-68) -> quantizer.decode (quantizer.rs:135-146) -> upsample (:126-133)
//   -> HiFiGAN::forward (hifi_gan.rs:208-216).  Configuration = FireflyConfig::get_config_for(1.4 | 1.5)
//   (codec/config.rs:155-167,98-113,196-202); `channel_div` scales every channel count down for tests.
#include "codec_engine.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/fishrt.h"
#include "codec_kernels.h"
#include "codec_resample.h"
#include "codec_loud.h"
#include "codec_tsm.h"
#include "fs_common.h"
#include "fs_synth.h"
#include "safetensors.h"

namespace fs {

namespace {
struct DBuf {
    void* p = nullptr;
    size_t n = 0;
    void alloc(size_t bytes) { free(); n = bytes; if (bytes) FS_HIP(hipMalloc(&p, bytes)); }
    void ensure(size_t bytes) { if (bytes > n) alloc(bytes); }
    void free() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
    ~DBuf() { free(); }
    float* f() const { return (float*)p; }
    uint16_t* u16() const { return (uint16_t*)p; }
};
struct Tensor {  // one checkpoint tensor
    std::string name;
    std::vector<int64_t> shape;
    float mean;
    double stdv;
    size_t off;  // float offset in the raw arena
    size_t numel() const { size_t n = 1; for (auto s : shape) n *= (size_t)s; return n; }
};
struct ConvSpec { int raw, relaid, bias, cout, cin_g, k; bool transposed; int stride; };
}  // namespace

class Codec final : public CodecBase {
  public:
    Codec(int device, int channel_div) : device_(device) {
        FS_REQUIRE(channel_div >= 1 && 512 % channel_div == 0 && (512 / channel_div) % 64 == 0 || channel_div == 8,
                   "channel_div must keep the width a multiple of 64");
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
            throw Error("no HIP device visible: libfishrt has no CPU fallback (MI355X / gfx950 required)");
        FS_REQUIRE(device >= 0 && device < ndev, "device_id out of range");
        FS_HIP(hipSetDevice(device));
        hipDeviceProp_t prop;
        FS_HIP(hipGetDeviceProperties(&prop, device));
        if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
            throw Error(std::string("libfishrt kernels are built for gfx950 only; device reports ") + prop.gcnArchName);
        FS_HIP(hipStreamCreateWithFlags(&st_, hipStreamNonBlocking));
        C_ = 512 / channel_div;  // quantizer input_dim == HiFiGAN upsample_initial_channel (config.rs:98-113,155-167)
        plan();
        raw_.alloc(raw_floats_ * sizeof(float));
        relaid_.alloc(relaid_floats_ * sizeof(float));
    }
    ~Codec() override {
        (void)hipSetDevice(device_);
        if (st_) { (void)hipStreamSynchronize(st_); (void)hipStreamDestroy(st_); }
    }

    void load_synthetic(uint64_t seed) override {
        FS_HIP(hipSetDevice(device_));
        for (const auto& t : tensors_)
            codec_synth_fill(raw_.f() + t.off, synth_fnv1a64(t.name.c_str()) ^ seed, t.numel(), t.mean, synth_scale(t.stdv), st_);
        relayout();
        loaded_ = true;
    }
    void load_safetensors(const std::string& path) override {
        FS_HIP(hipSetDevice(device_));
        SafeTensors sf(path);
        std::vector<float> host;
        for (const auto& t : tensors_) {
            const StTensor* s = &sf.get(t.name, t.shape);  // exact shape, as candle's VarBuilder::get (a transposed tensor is an error)
            host.resize(t.numel());
            SafeTensors::to_f32(*s, host.data());
            FS_HIP(hipMemcpyAsync(raw_.f() + t.off, host.data(), host.size() * 4, hipMemcpyHostToDevice, st_));
            FS_HIP(hipStreamSynchronize(st_));
        }
        relayout();
        loaded_ = true;
    }
    int sample_rate() override { return 44100; }  // SpecTransformConfig (config.rs:13-22)
    void set_precision(int mode) override {
        FS_REQUIRE(mode >= 0 && mode <= 2, "codec precision: 0 = f32 (exact products), 1 = bf16x3 (split bf16 matrix products), 2 = f16");
        bf3_ = mode >= 1;
        f16_ = mode == 2;
    }
    int precision() override { return f16_ ? 2 : (bf3_ ? 1 : 0); }

    // ---- f16 range guard (no reference counterpart: the reference runs the codec in f32, server/lib/utils/load.rs:161-164).  The f16 mode
    // rounds every matrix operand to f16 once: |x| > 65504 saturates, 0 < |x| < 2^-24 becomes zero, and its error is RELATIVE (2^-11) while
    // the acceptance bound on the PCM is absolute.  None of this bites with the synthetic N(0, 1 / fan_in) convs at the test signal's level; a
    // weight-normed checkpoint, or loud material, is a different distribution.  With the check on, decode() in f16 mode
    //   * runs the range-counting kernel twins (csrc/codec_conv_bf3.hip, FS_C3_CHECK): operands saturated / flushed to zero, for the
    //     activations of the call and (once, when the check is switched on) the f16 weight images;
    //   * decodes the same codes in bf16x3 mode as well (f32 exponent range, 2^-17 relative) and measures the RMS difference of the two PCMs;
    //   * returns the bf16x3 PCM when an operand saturated or the difference exceeds kGuardRms (half the 1e-4 acceptance bound), else the
    //     f16 PCM.  Flushed operands alone are reported, not acted on: SiLU tails put a few hundred activations per decode below 2^-24 with
    //     any weights, at an absolute error below 6e-8 each.
    // Streamed chunks are counted, not compared (their left context lives in the f16 planes).  ~3x the cost of a plain call: a validation
    // tool for a new checkpoint, not a serving mode.
    static constexpr double kGuardRms = 5e-5;
    void set_range_check(bool on) override {
        FS_HIP(hipSetDevice(device_));
        range_check_ = on;
        if (!on || !loaded_) return;
        scan_weight_range();
    }
    void range_stats(uint64_t* out5, double* last_rms) override {
        out5[0] = range_act_[0]; out5[1] = range_act_[1]; out5[2] = range_w_[0]; out5[3] = range_w_[1]; out5[4] = range_fallbacks_;
        if (last_rms) *last_rms = range_last_rms_;
    }
    // PCM samples per code frame = the product of the two quantizer upsamplings (2 x 2, k = stride = 2 transposed convs) and the HiFi-GAN stages' strides
    // of the loaded topology (config.rs:196-202: 8 x 8 x 2 x 2 x 2), read from the conv specs instead of assumed
    size_t samples_per_frame() const {
        size_t h = 1;
        for (int i = 0; i < 2; ++i) h *= (size_t)convs_[up_conv_[i]].stride;
        for (int s2 = 0; s2 < 5; ++s2) h *= (size_t)convs_[ups_[s2]].stride;
        return h;
    }
    static std::mutex& range_guard_mutex() { static std::mutex m; return m; }  // one checked call at a time per process (one counter pair per device)
    void scan_weight_range() {  // pack the f16 weight images again through the counting twin (same bytes)
        if (!packed16_.p) return;
        std::lock_guard<std::mutex> g(range_guard_mutex());
        codec_range_check(true);
        codec_range_reset(st_);
        for (size_t i = 0; i < convs_.size(); ++i) {
            const ConvSpec& cs = convs_[i];
            const int K = cs.transposed ? cs.k / cs.stride : cs.k, Cout = cs.transposed ? cs.cout * cs.stride : cs.cout;
            codec_pack_bf3(relaid_.f() + relaid_off_[i], packed16_.u16() + packed16_off_[i], cs.cin_g, K, Cout, true, st_);
        }
        codec_range_check(false);
        unsigned long long r[2] = {0, 0};
        codec_range_read(r, st_);
        range_w_[0] = r[0]; range_w_[1] = r[1];
    }

    void decode(const uint32_t* codes, int B, int T, float* pcm_out) override {
        if (!(range_check_ && bf3_ && f16_)) { decode_impl(codes, B, T, pcm_out, kOneShot); return; }
        FS_HIP(hipSetDevice(device_));
        unsigned long long r[2] = {0, 0};
        {
            std::lock_guard<std::mutex> g(range_guard_mutex());
            codec_range_check(true);
            codec_range_reset(st_);
            try { decode_impl(codes, B, T, pcm_out, kOneShot); } catch (...) { codec_range_check(false); throw; }
            codec_range_check(false);
            codec_range_read(r, st_);
        }
        range_act_[0] += r[0]; range_act_[1] += r[1];
        std::vector<float> wide((size_t)B * T * samples_per_frame());  // (4 x 8 x 8 x 2 x 2 x 2 = 2048 for the Fish codec: config.rs:196-202)
        f16_ = false;
        try { decode_impl(codes, B, T, wide.data(), kOneShot); } catch (...) { f16_ = true; throw; }
        f16_ = true;
        double ss = 0.0;
        bool finite = true;
        for (size_t i = 0; i < wide.size(); ++i) {
            const double d = (double)pcm_out[i] - (double)wide[i];
            ss += d * d;
            finite &= std::isfinite(pcm_out[i]);
        }
        range_last_rms_ = std::sqrt(ss / (double)wide.size());
        if (r[0] || range_w_[0] || !finite || !(range_last_rms_ <= kGuardRms)) {  // this call's PCM comes from the bf16x3 mode
            ++range_fallbacks_;
            std::memcpy(pcm_out, wide.data(), wide.size() * sizeof(float));
        }
    }

    // ---- stateful streaming (no reference counterpart; the reference vocodes an utterance in one piece, server/lib/handlers/speech.rs:98-129).
    // Every conv of the 1.4+/1.5 codec is causal, so chunk i of a stream needs, per conv input, only the last `halo` samples of chunk i-1:
    // the producers keep the last CODEC_PLANE_PAD slots of every plane tensor (CODEC_CTX_F32 samples of the three f32 conv inputs) in a
    // per-tensor context and the next chunk starts from them instead of from zeros -- the PCM of the chunks, concatenated, is bit-identical
    // to decoding the whole sequence at once, with no frame decoded twice.
    void stream_begin() override {
        FS_HIP(hipSetDevice(device_));
        FS_REQUIRE(loaded_, "weights not loaded: call fs_codec_load_safetensors or fs_codec_load_synthetic first");
        FS_REQUIRE(bf3_ && C_ % 128 == 0 && (C_ >> 5) >= 16, "streaming state needs the plane data flow: f16 / bf16x3 precision, full-size codec");
        // one stream per handle: a second begin would silently zero the left context of the stream in progress
        FS_REQUIRE(stream_chunk_ < 0, "a stream is already open on this codec handle (fs_codec_stream_end first)");
        for (int i = 0; i < 2; ++i) {
            sctx_p_[i].ensure((size_t)kCtxSlots * ctx_slot_bytes());
            sctx_f_[i].ensure((size_t)3 * C_ * CODEC_CTX_F32 * sizeof(float));
            FS_HIP(hipMemsetAsync(sctx_p_[i].p, 0, (size_t)kCtxSlots * ctx_slot_bytes(), st_));
            FS_HIP(hipMemsetAsync(sctx_f_[i].p, 0, (size_t)3 * C_ * CODEC_CTX_F32 * sizeof(float), st_));
        }
        FS_HIP(hipStreamSynchronize(st_));
        stream_chunk_ = 0;
        stream_prec_ = precision();
    }
    void stream_decode(const uint32_t* codes, int T, float* pcm_out) override {
        FS_REQUIRE(stream_chunk_ >= 0, "fs_codec_stream_begin first");
        FS_REQUIRE(precision() == stream_prec_, "the precision mode changed inside a stream");
        FS_REQUIRE(T >= kStreamMinFrames, "a streamed chunk needs >= 16 frames (64 samples at the vocoder's lowest rate)");
        const bool chk = range_check_ && bf3_ && f16_;
        if (chk) {
            std::lock_guard<std::mutex> g(range_guard_mutex());
            codec_range_check(true); codec_range_reset(st_);
            try { decode_impl(codes, 1, T, pcm_out, kSingle); } catch (...) { codec_range_check(false); throw; }
            codec_range_check(false);
            unsigned long long r[2] = {0, 0};
            codec_range_read(r, st_);
            range_act_[0] += r[0]; range_act_[1] += r[1];
        } else {
            decode_impl(codes, 1, T, pcm_out, kSingle);
        }
        ++stream_chunk_;
    }
    void stream_end() override { stream_chunk_ = -1; }

    // ---- many concurrent streams on one handle (fs_codec_streams_*).  Every open stream owns two halves (ping-pong, like the single stream)
    // of the plane and the f32 contexts in one pool per kind, [stream][half][slot...]; a call decodes its n chunks as the n items of ONE
    // launch sequence, and every context-carrying kernel finds item b's "in" / "out" half through a per-call device table of offsets
    // (codec_kernels.h ctx_off) instead of a single pointer.  No copies: each item reads its context where the previous chunk left it.
    static constexpr int kMaxStreams = 64;
    int streams_open() override {
        FS_HIP(hipSetDevice(device_));
        FS_REQUIRE(loaded_, "weights not loaded: call fs_codec_load_safetensors or fs_codec_load_synthetic first");
        FS_REQUIRE(bf3_ && C_ % 128 == 0 && (C_ >> 5) >= 16, "streaming state needs the plane data flow: f16 / bf16x3 precision, full-size codec");
        int id = 0;
        while (id < (int)ms_.size() && ms_[id].chunk >= 0) ++id;
        FS_REQUIRE(id < kMaxStreams, "all 64 streams of this codec handle are open (fs_codec_streams_close one first)");
        if (id >= ms_cap_) {  // grow the pools (doubling), keeping the contexts of the open streams
            const int cap = std::min(kMaxStreams, std::max(4, 2 * ms_cap_));
            DBuf np, nf;
            np.alloc((size_t)cap * ms_stream_p_bytes());
            nf.alloc((size_t)cap * ms_stream_f_bytes());
            FS_HIP(hipStreamSynchronize(st_));
            if (ms_cap_) {
                FS_HIP(hipMemcpyAsync(np.p, mpool_p_.p, (size_t)ms_cap_ * ms_stream_p_bytes(), hipMemcpyDeviceToDevice, st_));
                FS_HIP(hipMemcpyAsync(nf.p, mpool_f_.p, (size_t)ms_cap_ * ms_stream_f_bytes(), hipMemcpyDeviceToDevice, st_));
                FS_HIP(hipStreamSynchronize(st_));
            }
            std::swap(mpool_p_.p, np.p); std::swap(mpool_p_.n, np.n);
            std::swap(mpool_f_.p, nf.p); std::swap(mpool_f_.n, nf.n);
            ms_cap_ = cap;
        }
        if (id == (int)ms_.size()) ms_.push_back(MStream{});
        FS_HIP(hipMemsetAsync((uint8_t*)mpool_p_.p + (size_t)id * ms_stream_p_bytes(), 0, ms_stream_p_bytes(), st_));
        FS_HIP(hipMemsetAsync((uint8_t*)mpool_f_.p + (size_t)id * ms_stream_f_bytes(), 0, ms_stream_f_bytes(), st_));
        FS_HIP(hipStreamSynchronize(st_));
        ms_[id] = MStream{};  // a reopened id starts clean: plain, nothing seen, not flushed
        ms_[id].chunk = 0;
        ms_[id].prec = precision();
        return id;
    }
    void streams_close(int id) override {
        FS_REQUIRE(id >= 0 && id < (int)ms_.size() && ms_[id].chunk >= 0, "not an open stream id of this codec handle");
        ms_[id].chunk = -1;
    }
    void streams_decode(int n, const int* ids, const uint32_t* codes, int T, float* pcm_out) override {
        // everything is validated before the first launch: a rejected call leaves every stream's contexts and parity as they were
        FS_REQUIRE(n >= 1 && n <= kMaxStreams, "fs_codec_streams_decode takes 1 .. 64 streams per call");
        FS_REQUIRE(T >= kStreamMinFrames, "a streamed chunk needs >= 16 frames (64 samples at the vocoder's lowest rate)");
        for (int b = 0; b < n; ++b) {
            FS_REQUIRE(ids[b] >= 0 && ids[b] < (int)ms_.size() && ms_[ids[b]].chunk >= 0, "not an open stream id of this codec handle");
            for (int a = 0; a < b; ++a) FS_REQUIRE(ids[a] != ids[b], "a stream id appears twice in one call");
            FS_REQUIRE(precision() == ms_[ids[b]].prec, "the precision mode changed since the stream was opened");
            FS_REQUIRE(!ms_[ids[b]].stretch, kSpeedStreamMsg);
            FS_REQUIRE(!ms_[ids[b]].spec, kSpecStreamMsg);
        }
        check_codes(codes, (size_t)n * 8 * T);
        fill_offset_table(n, ids, 4);
        run_streams(codes, n, T, pcm_out, kMulti);
        for (int b = 0; b < n; ++b) ++ms_[ids[b]].chunk;  // only after the whole call went through
    }
    // per-call table, `rows` x n entries: element offsets of item b's (in, out) halves -- plane table (u16), then f32 table; the ragged call
    // appends its lengths and PCM offsets (rows 4 and 5)
    void fill_offset_table(int n, const int* ids, int rows) {
        const size_t pb = ms_stream_p_bytes() / 2, fb = ms_stream_f_bytes() / 2;  // bytes per half
        ms_tab_.assign((size_t)rows * n, 0);
        for (int b = 0; b < n; ++b) {
            const int s = ids[b], par = ms_[s].chunk & 1;
            ms_tab_[2 * b] = (long long)(((size_t)2 * s + par) * pb / 2);
            ms_tab_[2 * b + 1] = (long long)(((size_t)2 * s + (par ^ 1)) * pb / 2);
            ms_tab_[2 * n + 2 * b] = (long long)(((size_t)2 * s + par) * fb / 4);
            ms_tab_[2 * n + 2 * b + 1] = (long long)(((size_t)2 * s + (par ^ 1)) * fb / 4);
        }
    }
    void run_streams(const uint32_t* codes, int n, int T, float* pcm_out, int kind, const float** dev_pcm = nullptr) {
        const bool chk = range_check_ && bf3_ && f16_;
        if (chk) {
            std::lock_guard<std::mutex> g(range_guard_mutex());
            codec_range_check(true); codec_range_reset(st_);
            try { decode_impl(codes, n, T, pcm_out, kind, dev_pcm); } catch (...) { codec_range_check(false); throw; }
            codec_range_check(false);
            unsigned long long r[2] = {0, 0};
            codec_range_read(r, st_);
            range_act_[0] += r[0]; range_act_[1] += r[1];
        } else {
            decode_impl(codes, n, T, pcm_out, kind, dev_pcm);
        }
    }

    // ---- ragged multi-stream call (fs_codec_streams_decode_ragged): item i = the next T[i] >= 1 frames of stream ids[i].  The items are laid
    // out at the stride of the longest one (codes padded with index 0 behind an item's end) and run through the launch sequence of the uniform
    // call; the length table travels with the offset table, and only the context saves and the final PCM gather read it (codec_kernels.h
    // CtxLen): a context becomes the last PAD slots of (old context ++ the item's own slots), which is what a chunk of any length needs.
    // Work grows with n x the longest item.
    void streams_decode_ragged(int n, const int* ids, const int* T, const uint32_t* codes, float* pcm_out) override {
        FS_REQUIRE(n >= 1 && n <= kMaxStreams, "fs_codec_streams_decode_ragged takes 1 .. 64 streams per call");
        int Tmax = 0;
        size_t total = 0;
        for (int b = 0; b < n; ++b) {
            FS_REQUIRE(T[b] >= 1, "a ragged chunk needs >= 1 frame");
            FS_REQUIRE(T[b] <= (1 << 20), "a ragged chunk of more than 2^20 frames");
            FS_REQUIRE(ids[b] >= 0 && ids[b] < (int)ms_.size() && ms_[ids[b]].chunk >= 0, "not an open stream id of this codec handle");
            for (int a = 0; a < b; ++a) FS_REQUIRE(ids[a] != ids[b], "a stream id appears twice in one call");
            FS_REQUIRE(precision() == ms_[ids[b]].prec, "the precision mode changed since the stream was opened");
            FS_REQUIRE(!ms_[ids[b]].stretch, kSpeedStreamMsg);
            FS_REQUIRE(!ms_[ids[b]].spec, kSpecStreamMsg);
            Tmax = std::max(Tmax, T[b]);
            total += (size_t)T[b];
        }
        check_codes(codes, total * 8);
        ragged_launch(n, ids, T, Tmax, codes, pcm_out, nullptr);
        for (int b = 0; b < n; ++b) ++ms_[ids[b]].chunk;  // only after the whole call went through
    }
    // the launch sequence of a validated ragged call; with dev_pcm the packed PCM stays on the device (decode_impl)
    void ragged_launch(int n, const int* ids, const int* T, int Tmax, const uint32_t* codes, float* pcm_out, const float** dev_pcm) {
        // codes [n][8][Tmax], item b's rows filled up to T[b] (index 0 behind it: a valid code whose output nothing reads)
        rag_codes_.assign((size_t)n * 8 * Tmax, 0u);
        {
            const uint32_t* src = codes;
            for (int b = 0; b < n; ++b)
                for (int g = 0; g < 8; ++g, src += T[b]) std::memcpy(rag_codes_.data() + ((size_t)b * 8 + g) * Tmax, src, sizeof(uint32_t) * T[b]);
        }
        fill_offset_table(n, ids, 6);
        const long long spf = (long long)samples_per_frame();
        long long at = 0;
        for (int b = 0; b < n; ++b) {  // lengths in frames, then the items' sample offsets in the packed PCM
            ms_tab_[(size_t)4 * n + b] = T[b];
            ms_tab_[(size_t)5 * n + b] = at;
            at += spf * T[b];
        }
        run_streams(rag_codes_.data(), n, Tmax, pcm_out, kRagged, dev_pcm);
    }

    // ---- device sample-rate conversion of the vocoder's PCM and the encoder's input (fs_codec_*_pcm; kernels in codec_resample.hip, counting
    // in fs_resample_plan.h).  The PCM is converted where the vocoder left it, before the copy to the host.  A spec at the codec's own rate is
    // a format conversion only (kResampleCopy), whatever its mode.
    static void parse_spec(const int* s3, int from, int to, int& mode, int& format, ResampleRates& r) {
        FS_REQUIRE(s3[0] > 0, "fs_pcm_spec: the rate must be positive");
        FS_REQUIRE(s3[1] == FS_RESAMPLE_LINEAR || s3[1] == FS_RESAMPLE_SINC, "fs_pcm_spec: mode is FS_RESAMPLE_LINEAR or FS_RESAMPLE_SINC");
        FS_REQUIRE(s3[2] == FS_PCM_F32 || s3[2] == FS_PCM_S16, "fs_pcm_spec: format is FS_PCM_F32 or FS_PCM_S16");
        r = resample_rates(from, to);
        mode = from == to ? (int)kResampleCopy : s3[1];
        format = s3[2];
        if (mode == kResampleSinc) resample_require_table(r);
    }
    static size_t pcm_bytes(int format) { return format == kPcmS16 ? 2 : 4; }

    void decode_pcm(const uint32_t* codes, int B, int T, const int* spec3, void* out, size_t cap, int64_t* n_out) override {
        decode_pcm_speed(codes, B, T, 1.0, spec3, out, cap, n_out, "fs_codec_decode_pcm: cap is smaller than fs_resample_out_len of a row");
    }
    // speed == 1.0: no stretch stage
    void decode_speed(const uint32_t* codes, int B, int T, double speed, const int* spec3, void* out, size_t cap, int64_t* n_out) override {
        tsm_require_speed(speed);
        decode_pcm_speed(codes, B, T, speed, spec3, out, cap, n_out,
                         "fs_codec_decode_speed: cap is smaller than fs_resample_out_len of fs_time_stretch_out_len of a row");
    }
    // loud3 null: fs_codec_decode_speed.  Everything is checked before the vocoder runs
    void decode_loud(const uint32_t* codes, int B, int T, const double* loud3, double speed, const int* spec3, void* out, size_t cap,
                     int64_t* n_out, void* res24) override {
        tsm_require_speed(speed);
        LoudParams lp;
        if (loud3) {
            lp.target_lufs = loud3[0]; lp.peak_db = loud3[1]; lp.max_gain_db = loud3[2];
            loud_require_params(lp);
            loud_require_rate(sample_rate());
        }
        decode_pcm_speed(codes, B, T, speed, spec3, out, cap, n_out,
                         "fs_codec_decode_loud: cap is smaller than fs_resample_out_len of fs_time_stretch_out_len of a row", loud3 ? &lp : nullptr,
                         loud3 ? res24 : nullptr);
    }
    void decode_pcm_speed(const uint32_t* codes, int B, int T, double speed, const int* spec3, void* out, size_t cap, int64_t* n_out,
                          const char* cap_msg, const LoudParams* lp = nullptr, void* res24 = nullptr) {
        FS_HIP(hipSetDevice(device_));
        FS_REQUIRE(B >= 1 && T >= 1, "empty input");
        int mode, format;
        ResampleRates r;
        parse_spec(spec3, sample_rate(), spec3[0], mode, format, r);
        const bool stretch = speed != 1.0;
        const TsmParams tp;
        const int64_t n_voc = (int64_t)samples_per_frame() * T, n_in = stretch ? tsm_out_len(n_voc, speed) : n_voc;
        const int64_t ol = resample_out_len(r, mode, n_in);
        FS_REQUIRE((int64_t)cap >= ol, cap_msg);
        const float* d = nullptr;
        decode_impl(codes, B, T, nullptr, kOneShot, &d);
        if (lp) {  // the vocoder's rows, scaled -> ld_out_, the rows the stages below read
            ld_out_.ensure((size_t)B * (size_t)n_voc * sizeof(float));
            std::vector<LoudItem> rows((size_t)B);
            for (int b = 0; b < B; ++b) {
                rows[(size_t)b].src = d + (size_t)b * n_voc; rows[(size_t)b].n = n_voc;
                rows[(size_t)b].out = ld_out_.f() + (size_t)b * n_voc;
            }
            loudness().run(rows, sample_rate(), lp);
            if (res24) FS_HIP(hipMemcpyAsync(res24, loudness().results(), (size_t)B * sizeof(LoudResult), hipMemcpyDeviceToHost, st_));
            d = ld_out_.f();
        }
        if (stretch) {  // those rows -> ts_out_, the rows the stage below reads
            const int64_t K = tsm_frames(n_in, tp);
            ts_out_.ensure((size_t)B * std::max<int64_t>(n_in, 1) * sizeof(float));
            ts_pos_.ensure((size_t)B * std::max<int64_t>(K, 1) * sizeof(long long));
            std::vector<TsmItem> rows((size_t)B);
            for (int b = 0; b < B; ++b) {
                rows[(size_t)b].src = d + (size_t)b * n_voc; rows[(size_t)b].n = n_voc;
                rows[(size_t)b].out = ts_out_.f() + (size_t)b * n_in;
                rows[(size_t)b].pos = (long long*)ts_pos_.p + (size_t)b * K;
            }
            stretcher().run(rows, speed, tp);
            d = ts_out_.f();
        }
        const size_t esz = pcm_bytes(format), row = ((size_t)ol * esz + 3) & ~(size_t)3;
        rs_out_.ensure((size_t)B * row);
        std::vector<ResampleItem> items((size_t)B);
        for (int b = 0; b < B; ++b) {
            ResampleItem& it = items[(size_t)b];
            resampler().set_rates(it, r, mode);
            it.format = format;
            it.src = d + (size_t)b * n_in; it.n_src = n_in;
            it.out = (uint8_t*)rs_out_.p + (size_t)b * row; it.n_out = ol;
        }
        resampler().run(items);
        for (int b = 0; b < B; ++b) {
            FS_HIP(hipMemcpyAsync((uint8_t*)out + (size_t)b * cap * esz, (const uint8_t*)rs_out_.p + (size_t)b * row, (size_t)ol * esz, hipMemcpyDeviceToHost, st_));
            n_out[b] = ol;
        }
        FS_HIP(hipStreamSynchronize(st_));
    }

    int streams_open_pcm(const int* spec3) override {
        int mode, format;
        ResampleRates r;
        parse_spec(spec3, sample_rate(), spec3[0], mode, format, r);
        const int id = streams_open();
        auto& s = ms_[id];
        s.spec = true; s.mode = mode; s.format = format; s.rates = r;
        if (mode != kResampleCopy) {
            s.carry_cap = resample_carry_cap(r, mode);
            s.carry = std::make_shared<DBuf>();
            try { s.carry->alloc((size_t)2 * s.carry_cap * sizeof(float)); } catch (...) { s.chunk = -1; throw; }
        }
        return id;
    }
    // spec3 null: codec rate, f32 (a plain stream's output).  speed == 1.0: no stretch stage, the stream is what the spec alone makes it
    int streams_open_speed(double speed, const int* spec3) override {
        tsm_require_speed(speed);
        const int id = spec3 ? streams_open_pcm(spec3) : streams_open();
        if (speed == 1.0) return id;
        auto& s = ms_[id];
        s.stretch = true; s.speed = speed;
        s.tcarry_cap = tsm_carry_bound(TsmParams{}, speed);
        s.tcarry = std::make_shared<DBuf>();
        try {
            s.tcarry->alloc(16 + (size_t)2 * s.tcarry_cap * sizeof(float));
            FS_HIP(hipMemsetAsync(s.tcarry->p, 0, 16, st_));
            FS_HIP(hipStreamSynchronize(st_));
        } catch (...) { s.chunk = -1; throw; }
        return id;
    }
    void require_open(int id) const {
        FS_REQUIRE(id >= 0 && id < (int)ms_.size() && ms_[id].chunk >= 0, "not an open stream id of this codec handle");
    }
    int64_t streams_pending(int id, int T, bool final) override {
        require_open(id);
        const auto& s = ms_[id];
        FS_REQUIRE(T >= 0 && T <= (1 << 20), "a chunk of 0 .. 2^20 frames");
        int64_t n_feed = (int64_t)samples_per_frame() * T;
        if (s.stretch && !s.tbook.final) n_feed = tsm_plan_step(TsmParams{}, s.speed, s.tbook, n_feed, final).n_emit;  // through both stages
        return resample_plan_step(s.rates, s.mode, s.book, n_feed, final).n_emit;
    }
    void streams_decode_pcm(int n, const int* ids, const int* T, const uint8_t* final, const uint32_t* codes, void* out, size_t cap_bytes,
                            int64_t* n_out) override {
        FS_HIP(hipSetDevice(device_));
        // everything is validated and counted before the first launch: a rejected call leaves the vocoder contexts and the books as they were
        FS_REQUIRE(n >= 1 && n <= kMaxStreams, "fs_codec_streams_decode_pcm takes 1 .. 64 streams per call");
        const int64_t spf = (int64_t)samples_per_frame();
        std::vector<ResampleStep> steps((size_t)n);
        std::vector<TsmStep> tsteps((size_t)n);  // the stretch stage of the speed streams among the items; its output feeds the stage above
        std::vector<size_t> doff((size_t)n);  // byte offset of the item's row in rs_out_ (4-byte aligned; the caller's buffer is packed)
        std::vector<size_t> toff((size_t)n), tpoff((size_t)n);  // the item's row in ts_out_ (samples) and in ts_pos_ (positions)
        std::vector<int> vid, vT;
        int Tmax = 0, n_stretch = 0;
        size_t total_codes = 0, packed = 0, dbytes = 0, tsamples = 0, tpositions = 0;
        const TsmParams tp;
        for (int b = 0; b < n; ++b) {
            require_open(ids[b]);
            const auto& s = ms_[ids[b]];
            for (int a = 0; a < b; ++a) FS_REQUIRE(ids[a] != ids[b], "a stream id appears twice in one call");
            FS_REQUIRE(precision() == s.prec, "the precision mode changed since the stream was opened");
            const bool fin = final && final[b];
            FS_REQUIRE(T[b] >= 0 && T[b] <= (1 << 20), "a chunk of 0 .. 2^20 frames");
            FS_REQUIRE(T[b] >= 1 || fin, "an item of 0 frames must be final (a pure flush)");
            FS_REQUIRE(!s.book.final, "the stream was already flushed by a final item (fs_codec_streams_close it)");
            int64_t n_feed = spf * T[b];
            if (s.stretch) {
                TsmStep& ts = tsteps[(size_t)b];
                ts = tsm_plan_step(tp, s.speed, s.tbook, n_feed, fin);
                FS_REQUIRE(ts.carry_len <= s.tcarry_cap, "time stretch carry exceeds the stream's carry rows");
                toff[(size_t)b] = tsamples; tsamples += (size_t)ts.n_emit;
                tpoff[(size_t)b] = tpositions; tpositions += (size_t)(ts.k1 - ts.k0 + 1);
                n_feed = ts.n_emit;
                ++n_stretch;
            }
            steps[(size_t)b] = resample_plan_step(s.rates, s.mode, s.book, n_feed, fin);
            FS_REQUIRE(steps[(size_t)b].carry_len <= s.carry_cap, "resample carry exceeds the stream's carry rows");
            doff[(size_t)b] = dbytes;
            packed += (size_t)steps[(size_t)b].n_emit * pcm_bytes(s.format);
            dbytes += ((size_t)steps[(size_t)b].n_emit * pcm_bytes(s.format) + 3) & ~(size_t)3;
            if (T[b] >= 1) { vid.push_back(ids[b]); vT.push_back(T[b]); Tmax = std::max(Tmax, T[b]); total_codes += (size_t)T[b] * 8; }
        }
        FS_REQUIRE(packed <= cap_bytes, "fs_codec_streams_decode_pcm: cap_bytes is smaller than the samples this call emits (fs_codec_streams_pending)");
        check_codes(codes, total_codes);
        const float* d = nullptr;
        if (!vid.empty()) ragged_launch((int)vid.size(), vid.data(), vT.data(), Tmax, codes, nullptr, &d);
        if (n_stretch) {  // one launch pair for all speed streams of the call: the vocoder's items -> ts_out_, the rows the stage below reads
            ts_out_.ensure(std::max<size_t>(tsamples, 1) * sizeof(float));
            ts_pos_.ensure(tpositions * sizeof(long long));
            std::vector<TsmItem> rows;
            int64_t vat = 0;
            for (int b = 0; b < n; ++b) {
                const auto& s = ms_[ids[b]];
                const int64_t n_voc = spf * T[b];
                if (s.stretch) {
                    const TsmStep& ts = tsteps[(size_t)b];
                    TsmItem it;
                    if (n_voc) it.src = d + vat;
                    it.in0 = ts.in0; it.n = ts.n_total;
                    it.carry = s.trow(s.tpar); it.carry_len = (int)s.tbook.carry_len;
                    it.carry_out = s.trow(s.tpar ^ 1); it.new_carry_len = (int)ts.carry_len;
                    it.state = s.tstate();
                    it.k0 = ts.k0; it.k1 = ts.k1; it.pos0 = std::max<int64_t>(ts.k0 - 1, 0); it.speed = s.speed;
                    it.out = ts_out_.f() + toff[(size_t)b]; it.out_len = ts.n_emit;
                    it.pos = (long long*)ts_pos_.p + tpoff[(size_t)b];
                    rows.push_back(it);
                }
                vat += n_voc;
            }
            stretcher().run_items(rows, tp);
        }
        rs_out_.ensure(dbytes);
        std::vector<ResampleItem> items((size_t)n);
        int64_t at = 0;
        for (int b = 0; b < n; ++b) {
            const auto& s = ms_[ids[b]];
            const ResampleStep& p = steps[(size_t)b];
            ResampleItem& it = items[(size_t)b];
            resampler().set_rates(it, s.rates, s.mode);
            it.format = s.format;
            it.in0 = p.in0; it.n_src = spf * T[b]; it.out0 = p.out0; it.n_out = p.n_emit;
            if (T[b] >= 1) { it.src = d + at; at += it.n_src; }
            if (s.stretch) { it.n_src = tsteps[(size_t)b].n_emit; it.src = it.n_src ? ts_out_.f() + toff[(size_t)b] : nullptr; }
            if (s.carry) {
                it.carry = s.carry->f() + (size_t)s.par * s.carry_cap; it.carry_len = (int)s.book.carry_len;
                it.carry_out = s.carry->f() + (size_t)(s.par ^ 1) * s.carry_cap; it.new_carry_len = (int)p.carry_len;
            }
            it.out = (uint8_t*)rs_out_.p + doff[(size_t)b];
        }
        resampler().run(items);
        rs_host_.resize(dbytes);
        if (dbytes) FS_HIP(hipMemcpyAsync(rs_host_.data(), rs_out_.p, dbytes, hipMemcpyDeviceToHost, st_));
        FS_HIP(hipStreamSynchronize(st_));
        uint8_t* dst = (uint8_t*)out;
        for (int b = 0; b < n; ++b) {  // only after the whole call went through
            auto& s = ms_[ids[b]];
            const size_t bytes = (size_t)steps[(size_t)b].n_emit * pcm_bytes(s.format);
            if (bytes) std::memcpy(dst, rs_host_.data() + doff[(size_t)b], bytes);
            dst += bytes;
            n_out[b] = steps[(size_t)b].n_emit;
            if (T[b] >= 1) ++s.chunk;
            if (s.carry) s.par ^= 1;
            resample_commit(s.book, steps[(size_t)b], final && final[b]);
            if (s.stretch) { s.tpar ^= 1; tsm_commit(s.tbook, tsteps[(size_t)b], final && final[b]); }
        }
    }

    // downmix, resample to the codec's rate, encode: the clip goes to the device once and only the codes come back
    void encode_pcm(const float* pcm, int channels, int64_t frames, int rate, int mode_in, uint32_t* codes_out, size_t cap, size_t* L_out) override {
        FS_HIP(hipSetDevice(device_));
        FS_REQUIRE(loaded_, "weights not loaded: call fs_codec_load_safetensors or fs_codec_load_synthetic first");
        FS_REQUIRE(channels >= 1 && channels <= 64 && frames >= 1 && frames < (1ll << 31), "fs_codec_encode_pcm: 1 .. 64 channels, 1 .. 2^31 - 1 frames");
        const int spec3[3] = {sample_rate(), mode_in, FS_PCM_F32};
        int mode, format;
        ResampleRates r;
        parse_spec(spec3, rate, sample_rate(), mode, format, r);
        const int64_t n = resample_out_len(r, mode, frames);
        (void)encode_frames(n);
        const size_t in_elems = (size_t)frames * channels;
        rs_mix_.ensure((in_elems + (channels > 1 ? (size_t)frames : 0)) * sizeof(float));
        FS_HIP(hipMemcpyAsync(rs_mix_.p, pcm, in_elems * sizeof(float), hipMemcpyHostToDevice, st_));
        const float* mono = rs_mix_.f();
        if (channels > 1) {
            codec_downmix(rs_mix_.f(), channels, frames, rs_mix_.f() + in_elems, st_);
            mono = rs_mix_.f() + in_elems;
        }
        dpcm_.ensure(sizeof(float) * (size_t)n);
        std::vector<ResampleItem> items(1);
        resampler().set_rates(items[0], r, mode);
        items[0].src = mono; items[0].n_src = frames;
        items[0].out = dpcm_.p; items[0].n_out = n;
        resampler().run(items);
        encode_device((int)n, codes_out, cap, L_out);
    }

    static constexpr int kCtxSlots = 96, kStreamMinFrames = 16;
    size_t ctx_slot_bytes() const { return (size_t)2 * (C_ / 8) * CODEC_PLANE_PAD * 16; }  // 2 parts x C/8 groups x PAD slots x 16 B (largest tensor)
    size_t ms_stream_p_bytes() const { return (size_t)2 * kCtxSlots * ctx_slot_bytes(); }             // both halves of one stream
    size_t ms_stream_f_bytes() const { return (size_t)2 * 3 * C_ * CODEC_CTX_F32 * sizeof(float); }

    static void check_codes(const uint32_t* codes, size_t n) {
        for (size_t i = 0; i < n; ++i)
            if (codes[i] >= 1000u) throw Error("FSQ index out of range (gather out of bounds)");
    }

    // decode_impl's `streaming`: none, fs_codec_stream_*, fs_codec_streams_decode, fs_codec_streams_decode_ragged (T = the longest item)
    enum { kOneShot = 0, kSingle = 1, kMulti = 2, kRagged = 3 };
    // dev_pcm: leave the PCM on the device (*dev_pcm, rows as pcm_out would get them) for the resampler: no copy to the host, no synchronisation
    void decode_impl(const uint32_t* codes, int B, int T, float* pcm_out, int streaming, const float** dev_pcm = nullptr) {
        FS_HIP(hipSetDevice(device_));
        FS_REQUIRE(loaded_, "weights not loaded: call fs_codec_load_safetensors or fs_codec_load_synthetic first");
        FS_REQUIRE(B >= 1 && T >= 1, "empty input");
        const bool multi = streaming >= kMulti, ragged = streaming == kRagged;
        FS_REQUIRE(!multi || ms_tab_.size() == (size_t)(ragged ? 6 : 4) * B, "multi-stream offset table");
        use_bf3_now_ = bf3_;
        const int G = 8;
        check_codes(codes, (size_t)B * G * T);
        // streaming: context slot k of this chunk is read from the buffer the previous chunk wrote and written to the other one.  Multi-stream:
        // ci = co = slot k of stream 0's first half in the pool; the per-item table adds each item's (in, out) half
        const long long *tab_p = nullptr, *tab_f = nullptr;
        CtxLen rl;  // ragged: the per-item lengths, next to the offsets in the same upload
        if (multi) {
            // stream-ordered upload; ms_tab_ stays untouched until the synchronisation at the end of this call
            dtab_.ensure(ms_tab_.size() * sizeof(long long));
            FS_HIP(hipMemcpyAsync(dtab_.p, ms_tab_.data(), ms_tab_.size() * sizeof(long long), hipMemcpyHostToDevice, st_));
            tab_p = (const long long*)dtab_.p;
            tab_f = tab_p + 2 * B;
            if (ragged) rl = CtxLen{tab_p + 4 * B, T};
        }
        int slot = 0, fslot = 0;
        struct PC { const uint16_t* ci; uint16_t* co; const long long* off; CtxLen rl; };
        auto pctx = [&]() -> PC {
            if (!streaming) return PC{nullptr, nullptr, nullptr, {}};
            FS_REQUIRE(slot < kCtxSlots, "streaming context slots exhausted");
            const size_t off = (size_t)slot++ * ctx_slot_bytes();
            if (multi) {
                uint16_t* p = reinterpret_cast<uint16_t*>((uint8_t*)mpool_p_.p + off);
                return PC{p, p, tab_p, rl};
            }
            return PC{reinterpret_cast<const uint16_t*>((const uint8_t*)sctx_p_[stream_chunk_ & 1].p + off), reinterpret_cast<uint16_t*>((uint8_t*)sctx_p_[(stream_chunk_ + 1) & 1].p + off), nullptr, {}};
        };
        struct FC { const float* ci; float* co; const long long* off; };
        auto fctx = [&]() -> FC {
            if (!streaming) return FC{nullptr, nullptr, nullptr};
            const size_t off = (size_t)fslot++ * C_ * CODEC_CTX_F32;
            if (multi) return FC{mpool_f_.f() + off, mpool_f_.f() + off, tab_f};
            return FC{sctx_f_[stream_chunk_ & 1].f() + off, sctx_f_[(stream_chunk_ + 1) & 1].f() + off, nullptr};
        };
        const size_t max_elems = (size_t)B * C_ * 4 * T * 8;  // largest activation: (C/2) x 32T .. (C/32) x 2048T = C*64*T
        (void)max_elems;
        const size_t act = (size_t)B * (size_t)C_ * 64 * T;   // every HiFiGAN stage holds C * 64 * T / 2^(i+1) * 2^... <= C*64*T... see stages
        for (auto& b : buf_) b.ensure(act * sizeof(float));
        dcodes_.ensure(sizeof(uint32_t) * B * G * T);
        FS_HIP(hipMemcpyAsync(dcodes_.p, codes, sizeof(uint32_t) * B * G * T, hipMemcpyHostToDevice, st_));
        float *x = buf_[0].f(), *t1 = buf_[1].f(), *t2 = buf_[2].f(), *r = buf_[3].f(), *acc0 = buf_[4].f(), *acc1 = buf_[5].f(),
              *acc2 = buf_[6].f();
        // quantizer.decode: FSQ lookup + project_out, concat groups -> (B, C, T)
        codec_fsq_project((const uint32_t*)dcodes_.p, B, G, T, R(proj_w_), R(proj_b_), C_ / G, x, st_, multi);
        int Tc = T;
        // upsample.0 then upsample.1 (quantizer.rs:126-133): transposed conv (k = s = 2) + ConvNeXt block
        // bf16x3 mode with 16-channel-block widths: the pointwise convs read and write activation planes as well (codec_conv_bf3.hip)
        const bool bb_planes = use_bf3_now_ && C_ % 128 == 0;
        uint16_t *bp0 = nullptr, *bp1 = nullptr;
        if (bb_planes) {
            for (auto& pb : pbuf_) pb.ensure(act * sizeof(float) + (size_t)B * C_ * CODEC_PLANE_PAD * 4 + (256 << 10));
            bp0 = pbuf_[0].u16(); bp1 = pbuf_[1].u16();
            codec_act_split(x, B, C_, Tc, false, bp0, f16_, st_);
        }
        for (int i = 0; i < 2; ++i) {
            const CnxSpec& c = cnx_[i];
            if (bb_planes) {
                codec_tconv1d_planes(bp0, B, C_, Tc, conv(up_conv_[i]), 2, t1, st_);
                Tc *= 2;
                const FC fd = fctx();  // the depthwise k = 7 conv reads 6 samples of left context
                codec_dwconv_ln(t1, B, C_, Tc, R(c.dw), R(c.db), R(c.lnw), R(c.lnb), t2, st_, fd.ci, fd.off);
                if (ragged) codec_save_tail_f32_ragged(t1, B, C_, Tc, fd.ci, fd.co, st_, fd.off, rl);
                else if (streaming) codec_save_tail_f32(t1, B, C_, Tc, fd.co, st_, fd.off);
                codec_act_split(t2, B, C_, Tc, false, bp0, f16_, st_);
                codec_conv1d_planes(nullptr, bp0, B, C_, Tc, conv(c.pw1), 1, false, CODEC_EPI_GELU, nullptr, nullptr, nullptr, bp1, false, st_);
                // pwconv2 + gamma + residual: the sum feeds the next transposed conv / conv_pre as planes (no SiLU in front of either);
                // only conv_pre (after the second block) reads left context from it
                const PC pb = i == 1 ? pctx() : PC{nullptr, nullptr, nullptr, {}};
                codec_conv1d_planes(nullptr, bp1, B, 4 * C_, Tc, conv(c.pw2), 1, false, CODEC_EPI_GAMMA_RES, t1, R(c.gamma), nullptr, bp0, false, st_,
                                    pb.ci, pb.co, nullptr, nullptr, pb.off, pb.rl);
                continue;
            }
            codec_tconv1d(x, B, C_, Tc, conv(up_conv_[i]), 2, false, t1, st_);
            Tc *= 2;
            codec_dwconv_ln(t1, B, C_, Tc, R(c.dw), R(c.db), R(c.lnw), R(c.lnb), t2, st_);
            codec_conv1d(t2, B, C_, Tc, conv(c.pw1), 1, false, CODEC_EPI_GELU, nullptr, nullptr, r, st_);
            codec_conv1d(r, B, 4 * C_, Tc, conv(c.pw2), 1, false, CODEC_EPI_GAMMA_RES, t1, R(c.gamma), x, st_);
        }
        // HiFiGAN (hifi_gan.rs:208-216)
        const int rates[5] = {8, 8, 2, 2, 2}, dils[3] = {1, 3, 5};
        // bf16x3 mode: stages whose convs all fit the split-bf16 kernel exchange "activation planes" (bf16 hi / lo of silu(x), written by
        // the producer's epilogue, codec_conv_bf3.hip) instead of f32: the consumer stages them by LDS-DMA and never re-activates
        auto stage_planes = [&](int s) { return use_bf3_now_ && s < 5 && (C_ >> (s + 1)) >= 16 && (C_ >> s) % 16 == 0; };
        uint16_t *xp = nullptr, *t1p = nullptr, *t2p = nullptr, *accp = nullptr;
        if (stage_planes(0)) {
            // 2 parts x 2 bytes = the f32 footprint, + the zero padding in front of every row + slack for window reads past T
            for (auto& b : pbuf_) b.ensure(act * sizeof(float) + (size_t)B * C_ * CODEC_PLANE_PAD * 4 + (256 << 10));
            xp = pbuf_[2].u16(); t1p = pbuf_[1].u16(); t2p = pbuf_[3].u16(); accp = pbuf_[4].u16();
            const PC px = pctx();
            if (bb_planes) codec_conv1d_planes(nullptr, bp0, B, C_, Tc, conv(conv_pre_), 1, false, CODEC_EPI_NONE, nullptr, nullptr, nullptr, xp, true, st_, px.ci, px.co, nullptr, nullptr, px.off, px.rl);
            else codec_conv1d_planes(x, nullptr, B, C_, Tc, conv(conv_pre_), 1, false, CODEC_EPI_NONE, nullptr, nullptr, nullptr, xp, true, st_, px.ci, px.co, nullptr, nullptr, px.off, px.rl);
        } else {
            codec_conv1d(x, B, C_, Tc, conv(conv_pre_), 1, false, CODEC_EPI_NONE, nullptr, nullptr, t1, st_);
            std::swap(x, t1);
        }
        int ch = C_;
        for (int s = 0; s < 5; ++s) {
            float* accs[3] = {acc0, acc1, acc2};
            if (stage_planes(s)) {
                codec_tconv1d_planes(xp, B, ch, Tc, conv(ups_[s]), rates[s], t1, st_);  // ups[i](silu(x)); xp holds split(silu(x))
                ch /= 2; Tc *= rates[s];
                const PC p1 = pctx();
                codec_act_split(t1, B, ch, Tc, true, t1p, f16_, st_, p1.ci, p1.co, p1.off, p1.rl);
                for (int j = 0; j < 3; ++j) {  // ResBlock1 (hifi_gan.rs:74-85): x += c2(silu(c1(silu(x)))), both convs dilated
                    const float* cur = t1;
                    const uint16_t* curp = t1p;
                    for (int m = 0; m < 3; ++m) {
                        const PC pa = pctx(), pb2 = m < 2 ? pctx() : PC{nullptr, nullptr, nullptr, {}};
                        const ConvW w1 = conv(res_[s][j][0][m]), w2 = conv(res_[s][j][1][m]);
                        if (w1.f16 && w2.f16 && w1.k == w2.k && codec_respair_ok(ch, w1.k, dils[m], true)) {
                            // thin stages, f16 mode: the pair in ONE kernel (the intermediate stays in LDS).  Its output planes go to the buffer the
                            // pair does not read (other waves still read the input planes' halo): t1p -> accp -> t2p
                            uint16_t* outp = curp == accp ? t2p : accp;
                            if (j == 2 && m == 2 && fold_mean_) {
                                if (stage_planes(s + 1)) {
                                    const PC pm = pctx();
                                    codec_respair_f16(curp, B, ch, Tc, w1.wp, w1.b, w2.wp, w2.b, w1.k, dils[m], cur, nullptr, xp, st_, pa.ci, pa.co, pm.ci, pm.co,
                                                      acc0, acc1, pa.off, pa.rl);
                                } else {
                                    codec_respair_f16(curp, B, ch, Tc, w1.wp, w1.b, w2.wp, w2.b, w1.k, dils[m], cur, x, nullptr, st_, pa.ci, pa.co, nullptr, nullptr,
                                                      acc0, acc1, pa.off, pa.rl);
                                }
                                break;
                            }
                            codec_respair_f16(curp, B, ch, Tc, w1.wp, w1.b, w2.wp, w2.b, w1.k, dils[m], cur, accs[j], m < 2 ? outp : nullptr, st_, pa.ci, pa.co,
                                              pb2.ci, pb2.co, nullptr, nullptr, pa.off, pa.rl);
                            cur = accs[j]; curp = outp;
                            continue;
                        }
                        codec_conv1d_planes(nullptr, curp, B, ch, Tc, conv(res_[s][j][0][m]), dils[m], true, CODEC_EPI_NONE, nullptr, nullptr,
                                            nullptr, t2p, true, st_, pa.ci, pa.co, nullptr, nullptr, pa.off, pa.rl);
                        if (j == 2 && m == 2 && fold_mean_) {
                            // the ParallelBlock mean (hifi_gan.rs:114-117) inside the epilogue of the last residual conv: ((acc0 + acc1) + this
                            // block's output) / 3 goes straight to the next stage's input planes (or, after the last stage, to conv_post's f32
                            // input) -- the third block's f32 output and the mean kernel's three plane-sized reads never touch memory
                            if (stage_planes(s + 1)) {
                                const PC pm = pctx();
                                codec_conv1d_planes(nullptr, t2p, B, ch, Tc, conv(res_[s][j][1][m]), dils[m], true, CODEC_EPI_RES, cur, nullptr, nullptr,
                                                    xp, true, st_, pm.ci, pm.co, acc0, acc1, pm.off, pm.rl);
                            } else {
                                codec_conv1d_planes(nullptr, t2p, B, ch, Tc, conv(res_[s][j][1][m]), dils[m], true, CODEC_EPI_RES, cur, nullptr, x,
                                                    nullptr, true, st_, nullptr, nullptr, acc0, acc1);
                            }
                            break;
                        }
                        codec_conv1d_planes(nullptr, t2p, B, ch, Tc, conv(res_[s][j][1][m]), dils[m], true, CODEC_EPI_RES, cur, nullptr, accs[j],
                                            m < 2 ? accp : nullptr, true, st_, pb2.ci, pb2.co, nullptr, nullptr, pb2.off, pb2.rl);
                        cur = accs[j]; curp = accp;
                    }
                }
                if (fold_mean_) continue;
                if (stage_planes(s + 1)) {
                    const PC pm = pctx();
                    codec_mean3_planes(acc0, acc1, acc2, B, ch, Tc, true, xp, f16_, st_, pm.ci, pm.co, pm.off, pm.rl);
                } else codec_mean3(acc0, acc1, acc2, x, (size_t)B * ch * Tc, st_);
                continue;
            }
            codec_tconv1d(x, B, ch, Tc, conv(ups_[s]), rates[s], true, t1, st_);  // ups[i](silu(x))
            ch /= 2; Tc *= rates[s];
            for (int j = 0; j < 3; ++j) {  // ResBlock1 (hifi_gan.rs:74-85): x += c2(silu(c1(silu(x)))), both convs dilated
                const float* cur = t1;
                for (int m = 0; m < 3; ++m) {
                    codec_conv1d(cur, B, ch, Tc, conv(res_[s][j][0][m]), dils[m], true, CODEC_EPI_NONE, nullptr, nullptr, t2, st_);
                    codec_conv1d(t2, B, ch, Tc, conv(res_[s][j][1][m]), dils[m], true, CODEC_EPI_RES, cur, nullptr, accs[j], st_);
                    cur = accs[j];
                }
            }
            codec_mean3(acc0, acc1, acc2, x, (size_t)B * ch * Tc, st_);
        }
        const FC fp = fctx();  // conv_post (k = 13 on the 16-channel f32 mean)
        codec_conv1d(x, B, ch, Tc, conv(conv_post_), 1, true, CODEC_EPI_TANH, nullptr, nullptr, t1, st_, fp.ci, fp.off);
        if (ragged) {
            codec_save_tail_f32_ragged(x, B, ch, Tc, fp.ci, fp.co, st_, fp.off, rl);
            // the items' own samples packed in item order (t2 is free by now), one copy to the host
            size_t total = 0;
            for (int b = 0; b < B; ++b) total += (size_t)ms_tab_[(size_t)4 * B + b] * (size_t)(Tc / T);
            codec_gather_ragged(t1, B, Tc, rl, tab_p + 5 * B, t2, st_);
            if (dev_pcm) { *dev_pcm = t2; return; }
            FS_HIP(hipMemcpyAsync(pcm_out, t2, sizeof(float) * total, hipMemcpyDeviceToHost, st_));
            FS_HIP(hipStreamSynchronize(st_));
            return;
        }
        if (streaming) codec_save_tail_f32(x, B, ch, Tc, fp.co, st_, fp.off);
        if (dev_pcm) { *dev_pcm = t1; return; }
        FS_HIP(hipMemcpyAsync(pcm_out, t1, sizeof(float) * (size_t)B * Tc, hipMemcpyDeviceToHost, st_));
        FS_HIP(hipStreamSynchronize(st_));
    }

    // FireflyCodec::encode (firefly.rs:37-40) for one mono clip: pcm (n) -> indices (8, L), L = frames / 4
    void encode(const float* pcm, int n, uint32_t* codes_out, size_t cap, size_t* L_out) override {
        FS_HIP(hipSetDevice(device_));
        FS_REQUIRE(loaded_, "weights not loaded: call fs_codec_load_safetensors or fs_codec_load_synthetic first");
        (void)encode_frames(n);
        dpcm_.ensure(sizeof(float) * n);
        FS_HIP(hipMemcpyAsync(dpcm_.p, pcm, sizeof(float) * n, hipMemcpyHostToDevice, st_));
        encode_device(n, codes_out, cap, L_out);
    }
    // fs_selftest_codec_encode_stage: encode() with the tap armed for one call; the codes are computed and dropped
    void encode_stage(const float* pcm, int n, int stage, float* out, size_t cap, size_t* n_out) override {
        FS_HIP(hipSetDevice(device_));
        if (stage == -2) {  // the table as the device holds it
            ensure_mel_table();
            const size_t ne = mel_fb_.n / sizeof(float);
            FS_REQUIRE(ne <= cap, "encoder stage tap: out capacity too small");
            FS_HIP(hipMemcpy(out, mel_fb_.p, mel_fb_.n, hipMemcpyDeviceToHost));
            *n_out = ne;
            return;
        }
        const int F = encode_frames(n);
        std::vector<uint32_t> codes((size_t)8 * (F / 4));
        size_t L = 0;
        struct Disarm { Codec* c; ~Disarm() { c->tap_stage_ = kTapOff; c->tap_out_ = nullptr; } } disarm{this};
        tap_stage_ = stage; tap_out_ = out; tap_cap_ = cap; tap_n_ = 0;
        encode(pcm, n, codes.data(), (size_t)(F / 4), &L);
        FS_REQUIRE(tap_n_ > 0, "encoder stage tap: the stage was not reached");
        *n_out = tap_n_;
    }
    // mel frames of an n-sample clip, or the reason it cannot be encoded
    static int encode_frames(long long n) {
        const int pad = (kFft - kHop) / 2;
        if (n < pad) throw Error("input shorter than the reflect padding (range end index out of range, spectrogram.rs:19)");
        FS_REQUIRE(n < (1ll << 31) - 2 * pad, "clip too long");
        const long long Lp = (long long)n + 2 * pad, full = Lp / kHop, rem = Lp % kHop;
        long long F = std::max(0LL, full - (kFft / kHop - 1));  // frames the streaming STFT emits (stft.rs:52-90)
        if (rem > 0 && Lp >= kFft) F += 1;
        FS_REQUIRE(F >= 4, "clip too short: the quantizer downsamples 4 mel frames into one code");
        return (int)F;
    }
    // the encoder on the n mono samples at the codec rate that dpcm_ holds on the device
    void encode_device(int n, uint32_t* codes_out, size_t cap, size_t* L_out) {
        use_bf3_now_ = false;  // the indices are a discontinuous function of the activations: exact-f32 products only
        const int T = encode_frames(n), G = 8, nf = kFft / 2 + 1;
        ensure_mel_table();
        const size_t act = (size_t)std::max(nf, 4 * C_) * T;  // largest activation: lin (1025 x T) or a ConvNeXt hidden (4C x T)
        for (int i = 0; i < 4; ++i) buf_[i].ensure(act * sizeof(float));
        float *x = buf_[0].f(), *t1 = buf_[1].f(), *t2 = buf_[2].f(), *r = buf_[3].f();
        codec_stft_mag((const float*)dpcm_.p, n, kFft, kHop, T, t1, st_);
        codec_mel_log(t1, mel_fb_.f(), nf, kMels, T, x, st_);
        // fs_selftest_codec_encode_stage: the armed call copies one tensor out (the copy is complete at the call's final synchronisation)
        auto tap = [&](int stage, const float* p, size_t ne) {
            if (tap_stage_ != stage) return;
            FS_REQUIRE(ne <= tap_cap_, "encoder stage tap: out capacity too small");
            FS_HIP(hipMemcpyAsync(tap_out_, p, ne * sizeof(float), hipMemcpyDeviceToHost, st_));
            tap_n_ = ne;
        };
        tap(-1, x, (size_t)kMels * T);
        auto block = [&](const CnxSpec& c, int Cb, int Tc) {  // x -> x (ConvNeXtBlock, convnext.rs:110-126)
            codec_dwconv_ln(x, 1, Cb, Tc, R(c.dw), R(c.db), R(c.lnw), R(c.lnb), t2, st_);
            codec_conv1d(t2, 1, Cb, Tc, conv(c.pw1), 1, false, CODEC_EPI_GELU, nullptr, nullptr, r, st_);
            codec_conv1d(r, 1, 4 * Cb, Tc, conv(c.pw2), 1, false, CODEC_EPI_GAMMA_RES, x, R(c.gamma), t1, st_);
            std::swap(x, t1);
        };
        // ConvNeXtEncoder (convnext.rs:319-331)
        codec_conv1d(x, 1, kMels, T, conv(stem_conv_), 1, false, CODEC_EPI_NONE, nullptr, nullptr, t1, st_);
        codec_layernorm_cf(t1, edims_[0], T, R(stem_lnw_), R(stem_lnb_), x, st_);
        for (const auto& c : stages_[0]) block(c, edims_[0], T);
        tap(0, x, (size_t)edims_[0] * T);
        for (int i = 1; i < 4; ++i) {
            codec_layernorm_cf(x, edims_[i - 1], T, R(mid_lnw_[i]), R(mid_lnb_[i]), t1, st_);
            codec_conv1d(t1, 1, edims_[i - 1], T, conv(mid_conv_[i]), 1, false, CODEC_EPI_NONE, nullptr, nullptr, x, st_);
            for (const auto& c : stages_[i]) block(c, edims_[i], T);
            tap(i, x, (size_t)edims_[i] * T);
        }
        codec_layernorm_cf(x, edims_[3], T, R(enc_lnw_), R(enc_lnb_), t1, st_);
        std::swap(x, t1);
        tap(4, x, (size_t)C_ * T);
        // quantizer.encode (quantizer.rs:104-124): (strided conv k = s = 2 as space-to-depth + 1x1 conv) + ConvNeXt block, twice
        int Tc = T;
        for (int i = 0; i < 2; ++i) {
            codec_space_to_depth(x, C_, Tc, 2, t1, st_);
            Tc /= 2;
            ConvW w = conv(down_conv_[i]);
            w.k = 1;  // re-laid [Cin][2][Cout] == [2 Cin][1][Cout] over the space-to-depth channels
            codec_conv1d(t1, 1, 2 * C_, Tc, w, 1, false, CODEC_EPI_NONE, nullptr, nullptr, x, st_);
            block(down_cnx_[i], C_, Tc);
            tap(5 + i, x, (size_t)C_ * Tc);
        }
        FS_REQUIRE((size_t)Tc <= cap, "codes_out capacity too small");
        dcodes_.ensure(sizeof(uint32_t) * G * Tc);
        codec_fsq_encode(x, C_, Tc, G, R(pin_w_), R(pin_b_), (uint32_t*)dcodes_.p, st_);
        std::vector<uint32_t> host((size_t)G * Tc);
        FS_HIP(hipMemcpyAsync(host.data(), dcodes_.p, sizeof(uint32_t) * G * Tc, hipMemcpyDeviceToHost, st_));
        FS_HIP(hipStreamSynchronize(st_));
        for (int g = 0; g < G; ++g) std::memcpy(codes_out + (size_t)g * cap, host.data() + (size_t)g * Tc, sizeof(uint32_t) * Tc);
        *L_out = (size_t)Tc;
    }

  private:
    struct CnxSpec { int dw, db, lnw, lnb, pw1, pw2, gamma; };
    static constexpr int kMels = 160, kFft = 2048, kHop = 512;  // LogMelSpectrogramConfig::default (spectrogram.rs:114-126)

    // slaney mel filterbank, [n_fft/2+1][n_mels] (the layout load_mel_buffer reads, spectrogram.rs:90-101), regenerated from
    // the published formula (librosa.filters.mel, norm = "slaney", htk = False, f_min 0, f_max sr/2) in f64 and rounded to f32;
    // the reference embeds the same table as melfilters160.bytes (max |diff| 1.8e-7, checked by the tests)
    void ensure_mel_table() {
        if (mel_fb_.p) return;
        const int nf = kFft / 2 + 1, sr = 44100;
        const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
        auto hz_to_mel = [&](double f) { return f >= min_log_hz ? min_log_mel + std::log(f / min_log_hz) / logstep : f / f_sp; };
        auto mel_to_hz = [&](double m) { return m >= min_log_mel ? min_log_hz * std::exp(logstep * (m - min_log_mel)) : f_sp * m; };
        std::vector<double> mel_f(kMels + 2);
        const double m0 = hz_to_mel(0.0), m1 = hz_to_mel(sr / 2.0);
        for (int i = 0; i < kMels + 2; ++i) mel_f[i] = mel_to_hz(m0 + (m1 - m0) * (double)i / (double)(kMels + 1));
        std::vector<float> fb((size_t)nf * kMels, 0.f);
        for (int m = 0; m < kMels; ++m) {
            const double enorm = 2.0 / (mel_f[m + 2] - mel_f[m]);
            for (int f = 0; f < nf; ++f) {
                const double freq = (sr / 2.0) * (double)f / (double)(nf - 1);
                const double lower = (freq - mel_f[m]) / (mel_f[m + 1] - mel_f[m]), upper = (mel_f[m + 2] - freq) / (mel_f[m + 2] - mel_f[m + 1]);
                fb[(size_t)f * kMels + m] = (float)(std::max(0.0, std::min(lower, upper)) * enorm);
            }
        }
        mel_fb_.alloc(fb.size() * sizeof(float));
        FS_HIP(hipMemcpy(mel_fb_.p, fb.data(), fb.size() * sizeof(float), hipMemcpyHostToDevice));
    }

    const float* R(int tensor_idx) const { return raw_.f() + tensors_[tensor_idx].off; }
    ConvW conv(int spec_idx) const {
        const ConvSpec& s = convs_[spec_idx];
        ConvW w;
        w.wt = relaid_.f() + relaid_off_[spec_idx];
        w.b = R(s.bias);
        w.cout = s.cout; w.k = s.k;
        w.f16 = use_bf3_now_ && f16_;
        w.wp = !use_bf3_now_ ? nullptr : (f16_ ? packed16_.u16() + packed16_off_[spec_idx] : packed_.u16() + packed_off_[spec_idx]);
        return w;
    }
    int add_tensor(const std::string& name, std::vector<int64_t> shape, float mean, double stdv) {
        Tensor t{name, std::move(shape), mean, stdv, raw_floats_};
        raw_floats_ += (t.numel() + 63) & ~(size_t)63;
        tensors_.push_back(t);
        return (int)tensors_.size() - 1;
    }
    // Conv1d `name.conv.weight [cout, cin_g, k]` / ConvTranspose1d `[cin, cout, k]` + `name.conv.bias [cout]`
    // (1.4+ names: codec/utils/mod.rs:28-40,84-96).  Synthetic init: N(0, 1/fan_in), bias N(0, 0.02^2).
    int add_conv(const std::string& name, int cout, int cin_g, int k, bool transposed, double fan_in, int stride = 1) {
        ConvSpec s;
        s.stride = stride;
        s.raw = transposed ? add_tensor(name + ".conv.weight", {cin_g, cout, k}, 0.f, 1.0 / std::sqrt(fan_in))
                           : add_tensor(name + ".conv.weight", {cout, cin_g, k}, 0.f, 1.0 / std::sqrt(fan_in));
        s.bias = add_tensor(name + ".conv.bias", {cout}, 0.f, 0.02);
        s.cout = cout; s.cin_g = cin_g; s.k = k; s.transposed = transposed;
        relaid_off_.push_back(relaid_floats_);
        relaid_floats_ += ((size_t)cout * cin_g * k + 63) & ~(size_t)63;
        convs_.push_back(s);
        return (int)convs_.size() - 1;
    }
    // pwconv{1,2}.{weight,bias} (nn.Linear: [cout, cin]); conv_k1: a kernel-1 Conv1d whose checkpoint tensor is [cout, cin, 1]
    int add_linear_as_conv(const std::string& name, int cout, int cin, double fan_in, bool conv_k1 = false) {
        ConvSpec s;
        s.stride = 1;
        s.raw = conv_k1 ? add_tensor(name + ".weight", {cout, cin, 1}, 0.f, 1.0 / std::sqrt(fan_in))
                        : add_tensor(name + ".weight", {cout, cin}, 0.f, 1.0 / std::sqrt(fan_in));
        s.bias = add_tensor(name + ".bias", {cout}, 0.f, 0.02);
        s.cout = cout; s.cin_g = cin; s.k = 1; s.transposed = false;
        relaid_off_.push_back(relaid_floats_);
        relaid_floats_ += ((size_t)cout * cin + 63) & ~(size_t)63;
        convs_.push_back(s);
        return (int)convs_.size() - 1;
    }
    void plan() {
        const int G = 8, dg = C_ / G;
        // project_out of every group packed as [G][dg][4] / [G][dg]: one tensor per group in the checkpoint
        proj_w_ = (int)tensors_.size();
        for (int g = 0; g < G; ++g)
            add_tensor("quantizer.residual_fsq.rvqs." + std::to_string(g) + ".project_out.weight", {dg, 4}, 0.f, 0.5);
        proj_b_ = (int)tensors_.size();
        for (int g = 0; g < G; ++g) add_tensor("quantizer.residual_fsq.rvqs." + std::to_string(g) + ".project_out.bias", {dg}, 0.f, 0.02);
        // the packed views require contiguity: [dg*4] and [dg] are multiples of 64 floats only when dg % 16 == 0 / dg % 64 == 0,
        // so the group tensors are packed without padding instead:
        repack_groups(proj_w_, G, (size_t)dg * 4);
        repack_groups(proj_b_, G, (size_t)dg);
        for (int i = 0; i < 2; ++i) {
            const std::string p = "quantizer.upsample." + std::to_string(i);
            up_conv_[i] = add_conv(p + ".0", C_, C_, 2, true, (double)C_, 2);
            CnxSpec c;
            const std::string q = p + ".1";
            c.dw = add_tensor(q + ".dwconv.conv.weight", {C_, 1, 7}, 0.f, 1.0 / std::sqrt(7.0));
            c.db = add_tensor(q + ".dwconv.conv.bias", {C_}, 0.f, 0.02);
            c.lnw = add_tensor(q + ".norm.weight", {C_}, 1.f, 0.1);
            c.lnb = add_tensor(q + ".norm.bias", {C_}, 0.f, 0.02);
            c.pw1 = add_linear_as_conv(q + ".pwconv1", 4 * C_, C_, (double)C_);
            c.pw2 = add_linear_as_conv(q + ".pwconv2", C_, 4 * C_, 4.0 * C_);
            c.gamma = add_tensor(q + ".gamma", {C_}, 0.1f, 0.02);
            cnx_[i] = c;
        }
        conv_pre_ = add_conv("head.conv_pre", C_, C_, 13, false, (double)C_ * 13);
        const int rates[5] = {8, 8, 2, 2, 2}, ks[5] = {16, 16, 4, 4, 4}, rk[3] = {3, 7, 11};
        for (int s = 0; s < 5; ++s) {
            const int cin = C_ >> s, cout = C_ >> (s + 1);
            ups_[s] = add_conv("head.ups." + std::to_string(s), cout, cin, ks[s], true, (double)cin * ks[s] / rates[s], rates[s]);
            for (int j = 0; j < 3; ++j)
                for (int m = 0; m < 3; ++m) {
                    const std::string q = "head.resblocks." + std::to_string(s) + ".blocks." + std::to_string(j);
                    res_[s][j][0][m] = add_conv(q + ".convs1." + std::to_string(m), cout, cout, rk[j], false, (double)cout * rk[j]);
                    res_[s][j][1][m] = add_conv(q + ".convs2." + std::to_string(m), cout, cout, rk[j], false, (double)cout * rk[j]);
                }
        }
        conv_post_ = add_conv("head.conv_post", 1, C_ >> 5, 13, false, (double)(C_ >> 5) * 13);
        plan_encoder();
    }
    CnxSpec plan_block(const std::string& q, int Cb) {  // ConvNeXtBlock tensors (convnext.rs:60-108)
        CnxSpec c;
        c.dw = add_tensor(q + ".dwconv.conv.weight", {Cb, 1, 7}, 0.f, 1.0 / std::sqrt(7.0));
        c.db = add_tensor(q + ".dwconv.conv.bias", {Cb}, 0.f, 0.02);
        c.lnw = add_tensor(q + ".norm.weight", {Cb}, 1.f, 0.1);
        c.lnb = add_tensor(q + ".norm.bias", {Cb}, 0.f, 0.02);
        c.pw1 = add_linear_as_conv(q + ".pwconv1", 4 * Cb, Cb, (double)Cb);
        c.pw2 = add_linear_as_conv(q + ".pwconv2", Cb, 4 * Cb, 4.0 * Cb);
        c.gamma = add_tensor(q + ".gamma", {Cb}, 0.1f, 0.02);
        return c;
    }
    // encoder side: backbone (ConvNeXtEncoder, convnext.rs:186-331; BackboneConfig::fish_1_4, config.rs:47-57), quantizer.downsample
    // (quantizer.rs:44-66) and the per-group project_in (grouped_residual_fsq.rs:52-56)
    void plan_encoder() {
        const int div = 512 / C_;
        const int full[4] = {128, 256, 384, 512};
        for (int i = 0; i < 4; ++i) edims_[i] = full[i] / div;
        if (div == 1) { edepths_[0] = 3; edepths_[1] = 3; edepths_[2] = 9; edepths_[3] = 3; }
        else { edepths_[0] = 1; edepths_[1] = 1; edepths_[2] = 2; edepths_[3] = 1; }  // reduced test topology (channel_div > 1)
        stem_conv_ = add_conv("backbone.downsample_layers.0.0", edims_[0], kMels, 7, false, (double)kMels * 7);
        stem_lnw_ = add_tensor("backbone.downsample_layers.0.1.weight", {edims_[0]}, 1.f, 0.1);
        stem_lnb_ = add_tensor("backbone.downsample_layers.0.1.bias", {edims_[0]}, 0.f, 0.02);
        for (int i = 0; i < 4; ++i) {
            if (i > 0) {
                const std::string q = "backbone.downsample_layers." + std::to_string(i);
                mid_lnw_[i] = add_tensor(q + ".0.weight", {edims_[i - 1]}, 1.f, 0.1);
                mid_lnb_[i] = add_tensor(q + ".0.bias", {edims_[i - 1]}, 0.f, 0.02);
                mid_conv_[i] = add_linear_as_conv(q + ".1", edims_[i], edims_[i - 1], (double)edims_[i - 1], /*conv_k1=*/true);
            }
            for (int j = 0; j < edepths_[i]; ++j)
                stages_[i].push_back(plan_block("backbone.stages." + std::to_string(i) + "." + std::to_string(j), edims_[i]));
        }
        enc_lnw_ = add_tensor("backbone.norm.weight", {edims_[3]}, 1.f, 0.1);
        enc_lnb_ = add_tensor("backbone.norm.bias", {edims_[3]}, 0.f, 0.02);
        for (int i = 0; i < 2; ++i) {
            const std::string q = "quantizer.downsample." + std::to_string(i);
            down_conv_[i] = add_conv(q + ".0", C_, C_, 2, false, (double)C_ * 2);
            down_cnx_[i] = plan_block(q + ".1", C_);
        }
        const int G = 8, dg = C_ / G;
        pin_w_ = (int)tensors_.size();
        for (int g = 0; g < G; ++g)
            add_tensor("quantizer.residual_fsq.rvqs." + std::to_string(g) + ".project_in.weight", {4, dg}, 0.f, 1.0 / std::sqrt((double)dg));
        pin_b_ = (int)tensors_.size();
        for (int g = 0; g < G; ++g) add_tensor("quantizer.residual_fsq.rvqs." + std::to_string(g) + ".project_in.bias", {4}, 0.f, 0.02);
        repack_groups(pin_w_, G, (size_t)4 * dg);
        repack_groups(pin_b_, G, 4);
    }
    void repack_groups(int first, int G, size_t each) {  // make G consecutive tensors contiguous (no padding between them)
        size_t off = tensors_[first].off;
        for (int g = 0; g < G; ++g) { tensors_[first + g].off = off; off += each; }
        raw_floats_ = std::max(raw_floats_, (off + 63) & ~(size_t)63);
    }
    void relayout() {
        for (size_t i = 0; i < convs_.size(); ++i) {
            const ConvSpec& s = convs_[i];
            if (s.transposed) codec_relayout_tconv(R(s.raw), relaid_.f() + relaid_off_[i], s.cout, s.cin_g, s.k, s.stride, st_);
            else codec_relayout(R(s.raw), relaid_.f() + relaid_off_[i], s.cout, s.cin_g, s.k, false, st_);
        }
        // bf16 hi/lo split copies in MFMA operand order (the decode path's "bf16x3" precision mode), GEMM shape of the polyphase form
        packed_off_.clear();
        packed16_off_.clear();
        size_t total = 0, total16 = 0;
        auto shape = [](const ConvSpec& s, int& K, int& Cout) {
            K = s.transposed ? s.k / s.stride : s.k;
            Cout = s.transposed ? s.cout * s.stride : s.cout;
        };
        for (const ConvSpec& s : convs_) {
            int K, Cout; shape(s, K, Cout);
            packed_off_.push_back(total);
            total += (codec_pack_bf3_elems(s.cin_g, K, Cout, false) + 63) & ~(size_t)63;
            packed16_off_.push_back(total16);
            total16 += (codec_pack_bf3_elems(s.cin_g, K, Cout, true) + 63) & ~(size_t)63;
        }
        packed_.ensure(total * sizeof(uint16_t));
        packed16_.ensure(total16 * sizeof(uint16_t));
        for (size_t i = 0; i < convs_.size(); ++i) {
            int K, Cout; shape(convs_[i], K, Cout);
            codec_pack_bf3(relaid_.f() + relaid_off_[i], packed_.u16() + packed_off_[i], convs_[i].cin_g, K, Cout, false, st_);
            codec_pack_bf3(relaid_.f() + relaid_off_[i], packed16_.u16() + packed16_off_[i], convs_[i].cin_g, K, Cout, true, st_);
        }
        FS_HIP(hipStreamSynchronize(st_));
        if (range_check_) scan_weight_range();  // (the check was switched on before the weights existed: ADVICE r5)
    }

    int device_, C_ = 512;
    hipStream_t st_ = nullptr;
    bool loaded_ = false;
    std::vector<Tensor> tensors_;
    std::vector<ConvSpec> convs_;
    std::vector<size_t> relaid_off_;
    size_t raw_floats_ = 0, relaid_floats_ = 0;
    DBuf raw_, relaid_, packed_, packed16_, dcodes_, buf_[7], pbuf_[5];
    DBuf sctx_p_[2], sctx_f_[2];            // streaming contexts (plane tensors / f32 conv inputs), ping-pong per chunk
    int stream_chunk_ = -1, stream_prec_ = 0;  // -1: no stream open
    // chunk: chunks decoded so far (its parity picks the "in" half), -1 = id free.  spec: opened by fs_codec_streams_open_pcm; mode / format /
    // rates: how its PCM leaves (a plain stream: copy, f32); book: samples in and out so far; carry: two rows of resample_carry_cap samples,
    // row `par` holds the carry_len samples in front of the next chunk
    struct MStream {
        int chunk = -1, prec = 0;
        bool spec = false;
        int mode = kResampleCopy, format = kPcmF32, par = 0;
        ResampleRates rates;
        ResampleBook book;
        std::shared_ptr<DBuf> carry;
        int64_t carry_cap = 0;
        // opened by fs_codec_streams_open_speed with speed != 1: a stretch stage in front of the stage above.  tbook: samples in, frames and
        // samples out so far; tcarry: the position word p_{k_next - 1} (8 bytes, padded to 16), then two rows of tcarry_cap =
        // tsm_carry_bound samples, row `tpar` holds the tbook.carry_len samples in front of the next chunk
        bool stretch = false;
        double speed = 1.0;
        TsmBook tbook;
        std::shared_ptr<DBuf> tcarry;
        int64_t tcarry_cap = 0;
        int tpar = 0;
        long long* tstate() const { return (long long*)tcarry->p; }
        float* trow(int half) const { return (float*)((uint8_t*)tcarry->p + 16) + (size_t)half * (size_t)tcarry_cap; }
    };
    static constexpr const char* kSpecStreamMsg =
        "the stream was opened with a PCM spec (fs_codec_streams_open_pcm): decode it with fs_codec_streams_decode_pcm";
    static constexpr const char* kSpeedStreamMsg =
        "the stream was opened with a speed (fs_codec_streams_open_speed): decode it with fs_codec_streams_decode_pcm";
    std::unique_ptr<Resampler> rs_;                // made on first use, on st_
    DBuf rs_out_, rs_mix_;                         // the resampled rows of a call; the downmixed clip of fs_codec_encode_pcm
    std::vector<uint8_t> rs_host_;                 // host side of rs_out_ (rows at 4-byte aligned offsets), unpacked into the caller's buffer
    Resampler& resampler() { if (!rs_) rs_.reset(new Resampler(st_)); return *rs_; }
    std::unique_ptr<TimeStretcher> ts_;            // made on first use, on st_ (fs_codec_decode_speed)
    DBuf ts_out_, ts_pos_;                         // the stretched rows of a call and their frame positions
    TimeStretcher& stretcher() { if (!ts_) ts_.reset(new TimeStretcher(st_)); return *ts_; }
    std::unique_ptr<Loudness> ld_;                 // made on first use, on st_ (fs_codec_decode_loud)
    DBuf ld_out_;                                  // the scaled rows of a call
    Loudness& loudness() { if (!ld_) ld_.reset(new Loudness(st_)); return *ld_; }
    std::vector<MStream> ms_;                      // fs_codec_streams_*, index = stream id
    int ms_cap_ = 0;                               // streams the pools hold
    DBuf mpool_p_, mpool_f_, dtab_;                // context pools [stream][half][...] and the per-call device offset table
    std::vector<long long> ms_tab_;                // host side of the table (alive until the call's final synchronisation)
    std::vector<uint32_t> rag_codes_;              // the ragged call's codes at the stride of its longest item
    std::vector<size_t> packed_off_, packed16_off_;
    bool fold_mean_ = getenv("FISHRT_VOC_NO_FOLD_MEAN") == nullptr;  // ParallelBlock mean inside the last residual conv's epilogue (A/B switch)
    bool range_check_ = false;              // fs_codec_set_range_check
    uint64_t range_act_[2] = {0, 0}, range_w_[2] = {0, 0}, range_fallbacks_ = 0;
    double range_last_rms_ = 0.0;            // RMS difference of the f16 and bf16x3 PCMs of the last checked decode call
    bool f16_ = true;   // with bf3_: the plane data flow carries single f16 operands (mode 2) instead of bf16 hi / lo pairs (mode 1)
    bool bf3_ = true, use_bf3_now_ = false;  // decode precision mode (fs_codec_set_precision); the encoder always runs exact f32
    int proj_w_ = 0, proj_b_ = 0, up_conv_[2] = {0, 0}, conv_pre_ = 0, conv_post_ = 0, ups_[5] = {0, 0, 0, 0, 0};
    int res_[5][3][2][3] = {};
    CnxSpec cnx_[2] = {};
    // encoder side
    int edims_[4] = {128, 256, 384, 512}, edepths_[4] = {3, 3, 9, 3};
    int stem_conv_ = 0, stem_lnw_ = 0, stem_lnb_ = 0, mid_lnw_[4] = {}, mid_lnb_[4] = {}, mid_conv_[4] = {}, enc_lnw_ = 0, enc_lnb_ = 0;
    int down_conv_[2] = {0, 0}, pin_w_ = 0, pin_b_ = 0;
    std::vector<CnxSpec> stages_[4];
    CnxSpec down_cnx_[2] = {};
    DBuf mel_fb_, dpcm_;
    // encoder stage tap (encode_stage): off except inside that call
    static constexpr int kTapOff = -1000;
    int tap_stage_ = kTapOff;
    float* tap_out_ = nullptr;
    size_t tap_cap_ = 0, tap_n_ = 0;
};

CodecBase* make_codec(int device, int channel_div) { return new Codec(device, channel_div); }

// fs_resample (include/fishrt.h): the rows go to the device, through ONE ragged launch of the resampler, and back.  Follows the two definitions
// to the letter, equal rates included (linear: the identity; sinc: the 1 x 15 filter)
void resample_rows(int device, const float* pcm, int b, size_t stride, const int64_t* n_samples, int from_rate, const int* spec3, void* out,
                   size_t out_stride, int64_t* out_len) {
    FS_REQUIRE(b >= 1 && b <= 4096, "fs_resample takes 1 .. 4096 rows");
    FS_REQUIRE(from_rate > 0 && spec3[0] > 0, "fs_resample: sample rates must be positive");
    FS_REQUIRE(spec3[1] == FS_RESAMPLE_LINEAR || spec3[1] == FS_RESAMPLE_SINC, "fs_pcm_spec: mode is FS_RESAMPLE_LINEAR or FS_RESAMPLE_SINC");
    FS_REQUIRE(spec3[2] == FS_PCM_F32 || spec3[2] == FS_PCM_S16, "fs_pcm_spec: format is FS_PCM_F32 or FS_PCM_S16");
    const ResampleRates r = resample_rates(from_rate, spec3[0]);
    const int mode = spec3[1], format = spec3[2];
    if (mode == kResampleSinc) resample_require_table(r);  // refused before anything touches the device
    const size_t esz = format == kPcmS16 ? 2 : 4;
    std::vector<int64_t> ol((size_t)b);
    std::vector<size_t> ioff((size_t)b), ooff((size_t)b);
    size_t in_elems = 0, out_bytes = 0;
    for (int i = 0; i < b; ++i) {
        FS_REQUIRE(n_samples[i] >= 0 && (size_t)n_samples[i] <= stride && n_samples[i] < (1ll << 40), "fs_resample: a row's length must be in 0 .. stride");
        ol[(size_t)i] = resample_out_len(r, mode, n_samples[i]);
        FS_REQUIRE((size_t)ol[(size_t)i] <= out_stride, "fs_resample: out_stride is smaller than fs_resample_out_len of a row");
        ioff[(size_t)i] = in_elems; in_elems += (size_t)n_samples[i];
        ooff[(size_t)i] = out_bytes; out_bytes += ((size_t)ol[(size_t)i] * esz + 3) & ~(size_t)3;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) throw Error("no HIP device visible: libfishrt has no CPU fallback (MI355X / gfx950 required)");
    FS_REQUIRE(device >= 0 && device < ndev, "device_id out of range");
    FS_HIP(hipSetDevice(device));
    struct Stream {
        hipStream_t s = nullptr;
        ~Stream() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } }
    } st;
    FS_HIP(hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
    DBuf din, dout;
    din.alloc(std::max<size_t>(in_elems, 1) * sizeof(float));
    dout.alloc(std::max<size_t>(out_bytes, 4));
    {
        Resampler rs(st.s);
        std::vector<ResampleItem> items((size_t)b);
        for (int i = 0; i < b; ++i) {
            ResampleItem& it = items[(size_t)i];
            if (n_samples[i])
                FS_HIP(hipMemcpyAsync(din.f() + ioff[(size_t)i], pcm + (size_t)i * stride, (size_t)n_samples[i] * sizeof(float), hipMemcpyHostToDevice, st.s));
            rs.set_rates(it, r, mode);
            it.format = format;
            it.src = din.f() + ioff[(size_t)i]; it.n_src = n_samples[i];
            it.out = (uint8_t*)dout.p + ooff[(size_t)i]; it.n_out = ol[(size_t)i];
        }
        rs.run(items);
        for (int i = 0; i < b; ++i) {
            if (ol[(size_t)i])
                FS_HIP(hipMemcpyAsync((uint8_t*)out + (size_t)i * out_stride * esz, (const uint8_t*)dout.p + ooff[(size_t)i], (size_t)ol[(size_t)i] * esz, hipMemcpyDeviceToHost, st.s));
            out_len[i] = ol[(size_t)i];
        }
        FS_HIP(hipStreamSynchronize(st.s));
    }
}

// fs_time_stretch (include/fishrt.h): the rows go to the device, through the two launches of the time stretcher, and back.  Follows the
// definition to the letter, speed 1.0 included
void time_stretch_rows(int device, const float* pcm, int b, size_t stride, const int64_t* n_samples, double speed, const int* params2, float* out,
                       size_t out_stride, int64_t* out_len, int64_t* positions, size_t pos_stride) {
    FS_REQUIRE(b >= 1 && b <= 4096, "fs_time_stretch takes 1 .. 4096 rows");
    tsm_require_speed(speed);
    TsmParams tp;
    if (params2) { tp.N = params2[0]; tp.D = params2[1]; }
    tsm_require_params(tp);
    std::vector<int64_t> ol((size_t)b), K((size_t)b);
    std::vector<size_t> ioff((size_t)b), ooff((size_t)b), poff((size_t)b);
    size_t in_elems = 0, out_elems = 0, pos_elems = 0;
    for (int i = 0; i < b; ++i) {
        FS_REQUIRE(n_samples[i] >= 0 && (size_t)n_samples[i] <= stride && n_samples[i] < (1ll << 40), "fs_time_stretch: a row's length must be in 0 .. stride");
        ol[(size_t)i] = tsm_out_len(n_samples[i], speed);
        K[(size_t)i] = tsm_frames(ol[(size_t)i], tp);
        FS_REQUIRE((size_t)ol[(size_t)i] <= out_stride, "fs_time_stretch: out_stride is smaller than fs_time_stretch_out_len of a row");
        FS_REQUIRE(!positions || (size_t)K[(size_t)i] <= pos_stride, "fs_time_stretch: pos_stride is smaller than the frame count of a row");
        ioff[(size_t)i] = in_elems; in_elems += (size_t)n_samples[i];
        ooff[(size_t)i] = out_elems; out_elems += (size_t)ol[(size_t)i];
        poff[(size_t)i] = pos_elems; pos_elems += (size_t)K[(size_t)i];
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) throw Error("no HIP device visible: libfishrt has no CPU fallback (MI355X / gfx950 required)");
    FS_REQUIRE(device >= 0 && device < ndev, "device_id out of range");
    FS_HIP(hipSetDevice(device));
    struct Stream {
        hipStream_t s = nullptr;
        ~Stream() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } }
    } st;
    FS_HIP(hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
    DBuf din, dout, dpos;
    din.alloc(std::max<size_t>(in_elems, 1) * sizeof(float));
    dout.alloc(std::max<size_t>(out_elems, 1) * sizeof(float));
    dpos.alloc(std::max<size_t>(pos_elems, 1) * sizeof(long long));
    {
        TimeStretcher ts(st.s);
        std::vector<TsmItem> items((size_t)b);
        for (int i = 0; i < b; ++i) {
            TsmItem& it = items[(size_t)i];
            if (n_samples[i])
                FS_HIP(hipMemcpyAsync(din.f() + ioff[(size_t)i], pcm + (size_t)i * stride, (size_t)n_samples[i] * sizeof(float), hipMemcpyHostToDevice, st.s));
            it.src = din.f() + ioff[(size_t)i]; it.n = n_samples[i];
            it.out = dout.f() + ooff[(size_t)i];
            it.pos = (long long*)dpos.p + poff[(size_t)i];
        }
        ts.run(items, speed, tp);
        static_assert(sizeof(long long) == sizeof(int64_t), "positions are copied out as they are");
        for (int i = 0; i < b; ++i) {
            if (ol[(size_t)i])
                FS_HIP(hipMemcpyAsync(out + (size_t)i * out_stride, dout.f() + ooff[(size_t)i], (size_t)ol[(size_t)i] * sizeof(float), hipMemcpyDeviceToHost, st.s));
            if (positions && K[(size_t)i])
                FS_HIP(hipMemcpyAsync(positions + (size_t)i * pos_stride, (const long long*)dpos.p + poff[(size_t)i], (size_t)K[(size_t)i] * sizeof(int64_t), hipMemcpyDeviceToHost, st.s));
            out_len[i] = ol[(size_t)i];
        }
        FS_HIP(hipStreamSynchronize(st.s));
    }
}

// fs_selftest_tsm_chunks (include/fishrt.h): what a speed stream does to its vocoder PCM, on a host row and without a codec: per chunk one
// plan step (fs_tsm_plan.h), one item, one launch pair, with the carry rows and the position word a stream owns.  Every chunk is uploaded into
// the same buffer, filled with 0xFF (NaN) first: a sample of an earlier chunk can only come from the carry.
void time_stretch_chunks(int device, const float* pcm, int64_t n, const int64_t* chunks, int n_chunks, double speed, const int* params2, float* out,
                         size_t out_cap, int64_t* out_len, int64_t* emitted, int64_t* positions, size_t pos_cap, int64_t* n_pos) {
    FS_REQUIRE(n_chunks >= 1 && n_chunks <= (1 << 20), "fs_selftest_tsm_chunks takes 1 .. 2^20 chunks");
    FS_REQUIRE(n >= 0 && n < (1ll << 31), "fs_selftest_tsm_chunks: the row's length");
    tsm_require_speed(speed);
    TsmParams tp;
    if (params2) { tp.N = params2[0]; tp.D = params2[1]; }
    tsm_require_params(tp);
    int64_t sum = 0, longest = 0;
    for (int c = 0; c < n_chunks; ++c) {
        FS_REQUIRE(chunks[c] >= 0 && chunks[c] <= n, "fs_selftest_tsm_chunks: a chunk's length");
        sum += chunks[c];
        longest = std::max(longest, chunks[c]);
    }
    FS_REQUIRE(sum == n, "fs_selftest_tsm_chunks: the chunk lengths must add up to the row's length");
    const int64_t ol = tsm_out_len(n, speed), K = tsm_frames(ol, tp), cap = tsm_carry_bound(tp, speed);
    FS_REQUIRE((size_t)ol <= out_cap, "fs_selftest_tsm_chunks: out_cap is smaller than fs_time_stretch_out_len of the row");
    FS_REQUIRE(!positions || (size_t)K <= pos_cap, "fs_selftest_tsm_chunks: pos_cap is smaller than the frame count of the row");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) throw Error("no HIP device visible: libfishrt has no CPU fallback (MI355X / gfx950 required)");
    FS_REQUIRE(device >= 0 && device < ndev, "device_id out of range");
    FS_HIP(hipSetDevice(device));
    struct Stream {
        hipStream_t s = nullptr;
        ~Stream() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } }
    } st;
    FS_HIP(hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
    DBuf dchunk, dcarry, dout, dpos;
    dchunk.alloc(std::max<int64_t>(longest, 1) * sizeof(float));
    dcarry.alloc(16 + (size_t)2 * cap * sizeof(float));
    dout.alloc(std::max<int64_t>(ol, 1) * sizeof(float));
    dpos.alloc((size_t)(K + 1) * sizeof(long long));
    FS_HIP(hipMemsetAsync(dcarry.p, 0, 16, st.s));
    float* rows = (float*)((uint8_t*)dcarry.p + 16);
    {
        TimeStretcher ts(st.s);
        TsmBook book;
        int par = 0;
        int64_t at = 0;
        for (int c = 0; c < n_chunks; ++c) {
            const bool fin = c + 1 == n_chunks;
            const TsmStep s = tsm_plan_step(tp, speed, book, chunks[c], fin);
            FS_REQUIRE(s.carry_len <= cap, "time stretch carry exceeds the carry rows");
            FS_HIP(hipMemsetAsync(dchunk.p, 0xFF, dchunk.n, st.s));
            if (chunks[c]) FS_HIP(hipMemcpyAsync(dchunk.p, pcm + at, (size_t)chunks[c] * sizeof(float), hipMemcpyHostToDevice, st.s));
            std::vector<TsmItem> items(1);
            TsmItem& it = items[0];
            if (chunks[c]) it.src = dchunk.f();
            it.in0 = s.in0; it.n = s.n_total;
            it.carry = rows + (size_t)par * cap; it.carry_len = (int)book.carry_len;
            it.carry_out = rows + (size_t)(par ^ 1) * cap; it.new_carry_len = (int)s.carry_len;
            it.state = (long long*)dcarry.p;
            it.k0 = s.k0; it.k1 = s.k1; it.pos0 = std::max<int64_t>(s.k0 - 1, 0); it.speed = speed;
            it.out = dout.f(); it.out_len = s.n_emit;
            it.pos = (long long*)dpos.p;
            ts.run_items(items, tp);
            if (s.n_emit) FS_HIP(hipMemcpyAsync(out + s.out0, dout.p, (size_t)s.n_emit * sizeof(float), hipMemcpyDeviceToHost, st.s));
            if (positions && s.k1 > s.k0)
                FS_HIP(hipMemcpyAsync(positions + s.k0, (const long long*)dpos.p + (s.k0 - it.pos0), (size_t)(s.k1 - s.k0) * sizeof(int64_t), hipMemcpyDeviceToHost, st.s));
            FS_HIP(hipStreamSynchronize(st.s));  // (the next chunk overwrites dchunk, dout and dpos)
            emitted[c] = s.n_emit;
            at += chunks[c];
            par ^= 1;
            tsm_commit(book, s, fin);
        }
        FS_REQUIRE(book.n_out == ol && book.k_next == K, "time stretch stream: the emitted totals");
    }
    *out_len = ol;
    if (n_pos) *n_pos = K;
}

// fs_loudness_normalize (include/fishrt.h): the rows go to the device, through the launches of codec_loud.hip, and back
void loudness_rows(int device, const float* pcm, int b, size_t stride, const int64_t* n_samples, int rate, const double* loud3, float* out,
                   size_t out_stride, void* res24, double* hops, size_t hops_cap, int64_t* n_hops) {
    FS_REQUIRE(b >= 1 && b <= 4096, "fs_loudness_normalize takes 1 .. 4096 rows");
    loud_require_rate(rate);
    LoudParams lp;
    if (loud3) {
        lp.target_lufs = loud3[0]; lp.peak_db = loud3[1]; lp.max_gain_db = loud3[2];
        loud_require_params(lp);
    }
    FS_REQUIRE(loud3 || !out, "fs_loudness_normalize: an output needs params");
    FS_REQUIRE(!hops || b == 1, "the hop energies are read one row at a time");
    std::vector<size_t> off((size_t)b);
    size_t elems = 0;
    for (int i = 0; i < b; ++i) {
        FS_REQUIRE(n_samples[i] >= 0 && (size_t)n_samples[i] <= stride && n_samples[i] <= kLoudMaxSamples,
                   "fs_loudness_normalize: a row's length must be in 0 .. stride and at most 2^30");
        FS_REQUIRE(!out || (size_t)n_samples[i] <= out_stride, "fs_loudness_normalize: out_stride is smaller than a row");
        off[(size_t)i] = elems; elems += (size_t)n_samples[i];
    }
    FS_REQUIRE(!hops || (size_t)loud_hops(n_samples[0], rate) <= hops_cap, "the hop energies do not fit");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) throw Error("no HIP device visible: libfishrt has no CPU fallback (MI355X / gfx950 required)");
    FS_REQUIRE(device >= 0 && device < ndev, "device_id out of range");
    FS_HIP(hipSetDevice(device));
    struct Stream {
        hipStream_t s = nullptr;
        ~Stream() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } }
    } st;
    FS_HIP(hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
    DBuf din, dout;
    din.alloc(std::max<size_t>(elems, 1) * sizeof(float));
    if (out) dout.alloc(std::max<size_t>(elems, 1) * sizeof(float));
    {
        Loudness ld(st.s);
        std::vector<LoudItem> items((size_t)b);
        for (int i = 0; i < b; ++i) {
            LoudItem& it = items[(size_t)i];
            if (n_samples[i])
                FS_HIP(hipMemcpyAsync(din.f() + off[(size_t)i], pcm + (size_t)i * stride, (size_t)n_samples[i] * sizeof(float), hipMemcpyHostToDevice, st.s));
            it.src = din.f() + off[(size_t)i]; it.n = n_samples[i];
            it.out = out ? dout.f() + off[(size_t)i] : nullptr;
        }
        ld.run(items, rate, loud3 ? &lp : nullptr);
        FS_HIP(hipMemcpyAsync(res24, ld.results(), (size_t)b * sizeof(LoudResult), hipMemcpyDeviceToHost, st.s));
        for (int i = 0; out && i < b; ++i)
            if (n_samples[i])
                FS_HIP(hipMemcpyAsync(out + (size_t)i * out_stride, dout.f() + off[(size_t)i], (size_t)n_samples[i] * sizeof(float), hipMemcpyDeviceToHost, st.s));
        if (hops) {
            if (ld.n_hops(0)) FS_HIP(hipMemcpyAsync(hops, ld.hops(0), (size_t)ld.n_hops(0) * sizeof(double), hipMemcpyDeviceToHost, st.s));
            if (n_hops) *n_hops = ld.n_hops(0);
        }
        FS_HIP(hipStreamSynchronize(st.s));
    }
}

// fs_selftest_conv1d (include/fishrt.h): one conv through the load-time functions (re-layout, pack), the plane producers and ONE launcher of
// codec_kernels.h, on host data.  Plane buffers are sized as decode_impl sizes them (256 KB of slack for window reads past T) and filled with
// 0xFF first, so a consumer that let a slot behind T -- or an unwritten pad slot -- reach a stored sample returns NaN.
void codec_conv_selftest(int device, const fs_conv_case& c, float* y_out, float* planes_out, char* variant_out, size_t variant_cap,
                         uint64_t* range_out) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) throw Error("no HIP device visible: libfishrt has no CPU fallback (MI355X / gfx950 required)");
    FS_REQUIRE(device >= 0 && device < ndev, "device_id out of range");
    FS_HIP(hipSetDevice(device));
    const int B = c.B, Cin = c.Cin, Cout = c.Cout, T = c.T, K = c.K, dil = c.dil;
    const bool tconv = c.flow == FS_CONV_TCONV1D || c.flow == FS_CONV_TCONV1D_PLANES, pair = c.flow == FS_CONV_RESPAIR_F16;
    const bool planes_flow = c.flow == FS_CONV_CONV1D_PLANES || c.flow == FS_CONV_TCONV1D_PLANES || pair;
    const int stride = tconv ? c.stride : 1;
    FS_REQUIRE(c.flow >= FS_CONV_CONV1D && c.flow <= FS_CONV_RESPAIR_F16, "conv self-test: unknown flow");
    FS_REQUIRE(c.precision >= 0 && c.precision <= 2, "conv self-test: precision 0 = f32, 1 = bf16x3, 2 = f16");
    FS_REQUIRE(B >= 1 && Cin >= 1 && Cout >= 1 && T >= 1 && K >= 1 && dil >= 1 && stride >= 1 && K % stride == 0, "conv self-test: bad shape");
    FS_REQUIRE(B <= 64 && Cin <= 4096 && Cout <= 4096 && K <= 64 && dil <= 256 && stride <= 64, "conv self-test: shape above the test range");
    FS_REQUIRE((long long)B * std::max(Cin, Cout * stride) * ((long long)T + CODEC_PLANE_PAD) < (1LL << 28), "conv self-test: activation above 2^28 elements");
    FS_REQUIRE(c.epi >= CODEC_EPI_NONE && c.epi <= CODEC_EPI_TANH, "conv self-test: unknown epilogue");
    FS_REQUIRE(c.input >= FS_CONV_IN_F32 && c.input <= FS_CONV_IN_MEAN3_SILU, "conv self-test: unknown input kind");
    FS_REQUIRE(c.x && c.w && c.bias, "conv self-test: x, w and bias are required");
    FS_REQUIRE(!planes_flow || c.precision >= 1, "conv self-test: the plane data flow needs precision 1 (bf16x3) or 2 (f16)");
    FS_REQUIRE(planes_flow || (c.input == FS_CONV_IN_F32 && c.outputs == FS_CONV_OUT_F32 && !c.mean_a && !c.mean_b && !c.post_silu),
               "conv self-test: codec_conv1d / codec_tconv1d read f32 and write f32");
    FS_REQUIRE(c.outputs >= 1 && c.outputs <= 3 && (!(c.outputs & FS_CONV_OUT_F32) || y_out) && (!(c.outputs & FS_CONV_OUT_PLANES) || planes_out),
               "conv self-test: outputs = FS_CONV_OUT_F32 | FS_CONV_OUT_PLANES, each with its buffer");
    FS_REQUIRE(!tconv || (c.epi == CODEC_EPI_NONE && dil == 1 && c.outputs == FS_CONV_OUT_F32), "conv self-test: a transposed conv has no epilogue, no dilation and an f32 output");
    FS_REQUIRE(c.flow != FS_CONV_TCONV1D_PLANES || c.input != FS_CONV_IN_F32, "conv self-test: codec_tconv1d_planes reads planes");
    FS_REQUIRE(!pair || (c.precision == 2 && Cin == Cout && c.input != FS_CONV_IN_F32 && c.w2 && c.bias2 && c.res && codec_respair_ok(Cin, K, dil, true)),
               "conv self-test: the fused pair needs f16 precision, Cin == Cout, a plane input, w2 / bias2 / res and a shape codec_respair_ok accepts");
    const bool need_res = c.epi == CODEC_EPI_RES || c.epi == CODEC_EPI_GAMMA_RES || pair;
    FS_REQUIRE(!need_res || c.res, "conv self-test: the residual epilogues need res");
    FS_REQUIRE(c.epi != CODEC_EPI_GAMMA_RES || c.gamma, "conv self-test: FS_CONV_EPI_GAMMA_RES needs gamma");
    FS_REQUIRE((c.mean_a != nullptr) == (c.mean_b != nullptr), "conv self-test: mean_a and mean_b come together");
    FS_REQUIRE(c.input < FS_CONV_IN_MEAN3 || (c.x_b && c.x_c), "conv self-test: the mean3 producer needs x_b and x_c");
    FS_REQUIRE(c.input == FS_CONV_IN_F32 || Cin % 16 == 0, "conv self-test: plane input needs Cin % 16 == 0");
    FS_REQUIRE(!(c.outputs & FS_CONV_OUT_PLANES) || Cout % 8 == 0, "conv self-test: plane output needs Cout % 8 == 0");
    FS_REQUIRE(!c.range_check || (c.precision >= 1 && range_out), "conv self-test: the range check needs precision 1 | 2 and range_out");
    FS_REQUIRE(variant_out && variant_cap >= 1, "conv self-test: variant_out");

    const bool f16 = c.precision == 2;
    const int NP = f16 ? 1 : 2;  // plane parts
    const size_t nx = (size_t)B * Cin * T, Tout = (size_t)T * stride, ny = (size_t)B * Cout * Tout, nw = (size_t)Cout * Cin * K;
    const size_t row = (size_t)CODEC_PLANE_PAD + T, slack = 256 << 10;
    auto plane_bytes = [&](int C) { return (size_t)B * NP * (C / 8) * row * 16 + slack; };
    hipStream_t st = nullptr;
    FS_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    struct StreamGuard { hipStream_t s; ~StreamGuard() { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } } sg{st};
    DBuf dx, dxb, dxc, dw, dw2, drel, drel2, dpk, dpk2, dbias, dbias2, dres, dgamma, dma, dmb, dy, dxp, dyp;
    auto up = [&](DBuf& d, const float* src, size_t n) {
        d.alloc(n * sizeof(float));
        FS_HIP(hipMemcpyAsync(d.p, src, n * sizeof(float), hipMemcpyHostToDevice, st));
    };
    up(dx, c.x, nx);
    if (c.input >= FS_CONV_IN_MEAN3) { up(dxb, c.x_b, nx); up(dxc, c.x_c, nx); }
    up(dw, c.w, nw); up(dbias, c.bias, Cout);
    if (pair) { up(dw2, c.w2, nw); up(dbias2, c.bias2, Cout); }
    if (need_res) up(dres, c.res, ny);
    if (c.epi == CODEC_EPI_GAMMA_RES) up(dgamma, c.gamma, Cout);
    if (c.mean_a) { up(dma, c.mean_a, ny); up(dmb, c.mean_b, ny); }

    std::unique_lock<std::mutex> range_lock;  // one checked call at a time per process (one counter pair per device)
    struct CheckGuard { bool on = false; ~CheckGuard() { if (on) codec_range_check(false); } } chk;
    if (c.range_check) {
        range_lock = std::unique_lock<std::mutex>(Codec::range_guard_mutex());
        codec_range_check(true);
        chk.on = true;
        codec_range_reset(st);
    }
    // load time: checkpoint layout -> [Cin][K][Cout] (polyphase form for a transposed conv) -> MFMA operand order of the precision mode
    const int Kg = K / stride, Cg = Cout * stride;  // GEMM shape
    auto load = [&](DBuf& raw, DBuf& rel, DBuf& pk, const DBuf& b) {
        rel.alloc(nw * sizeof(float));
        if (tconv) codec_relayout_tconv(raw.f(), rel.f(), Cout, Cin, K, stride, st);
        else codec_relayout(raw.f(), rel.f(), Cout, Cin, K, false, st);
        ConvW w;
        w.wt = rel.f(); w.b = b.f(); w.cout = Cout; w.k = K;
        if (c.precision >= 1) {
            pk.alloc(codec_pack_bf3_elems(Cin, Kg, Cg, f16) * sizeof(uint16_t));
            codec_pack_bf3(rel.f(), pk.u16(), Cin, Kg, Cg, f16, st);
            w.wp = pk.u16(); w.f16 = f16;
        }
        return w;
    };
    const ConvW w1 = load(dw, drel, dpk, dbias);
    ConvW w2;
    if (pair) w2 = load(dw2, drel2, dpk2, dbias2);
    // producers of the plane input
    if (c.input != FS_CONV_IN_F32) {
        dxp.alloc(plane_bytes(Cin));
        FS_HIP(hipMemsetAsync(dxp.p, 0xFF, dxp.n, st));
        const bool silu = c.input == FS_CONV_IN_SPLIT_SILU || c.input == FS_CONV_IN_MEAN3_SILU;
        if (c.input >= FS_CONV_IN_MEAN3) codec_mean3_planes(dx.f(), dxb.f(), dxc.f(), B, Cin, T, silu, dxp.u16(), f16, st);
        else codec_act_split(dx.f(), B, Cin, T, silu, dxp.u16(), f16, st);
    }
    if (c.outputs & FS_CONV_OUT_F32) { dy.alloc(ny * sizeof(float)); FS_HIP(hipMemsetAsync(dy.p, 0xFF, dy.n, st)); }
    if (c.outputs & FS_CONV_OUT_PLANES) { dyp.alloc(plane_bytes(Cout)); FS_HIP(hipMemsetAsync(dyp.p, 0xFF, dyp.n, st)); }
    const float* xin = c.input == FS_CONV_IN_F32 ? dx.f() : nullptr;
    codec_variant_note(nullptr);
    switch (c.flow) {
    case FS_CONV_CONV1D: codec_conv1d(dx.f(), B, Cin, T, w1, dil, c.pre_silu != 0, c.epi, dres.f(), dgamma.f(), dy.f(), st); break;
    case FS_CONV_TCONV1D: codec_tconv1d(dx.f(), B, Cin, T, w1, stride, c.pre_silu != 0, dy.f(), st); break;
    case FS_CONV_CONV1D_PLANES:
        codec_conv1d_planes(xin, dxp.u16(), B, Cin, T, w1, dil, c.pre_silu != 0, c.epi, dres.f(), dgamma.f(), dy.f(), dyp.u16(), c.post_silu != 0, st, nullptr,
                            nullptr, dma.f(), dmb.f());
        break;
    case FS_CONV_TCONV1D_PLANES: codec_tconv1d_planes(dxp.u16(), B, Cin, T, w1, stride, dy.f(), st); break;
    default:
        codec_respair_f16(dxp.u16(), B, Cin, T, w1.wp, w1.b, w2.wp, w2.b, K, dil, dres.f(), dy.f(), dyp.u16(), st, nullptr, nullptr, nullptr, nullptr, dma.f(),
                          dmb.f());
        break;
    }
    const char* name = codec_variant_last();
    if (c.range_check) {
        codec_range_check(false);
        chk.on = false;
        unsigned long long r[2] = {0, 0};
        codec_range_read(r, st);
        range_out[0] = r[0]; range_out[1] = r[1];
        range_lock.unlock();
    }
    if (c.outputs & FS_CONV_OUT_F32) FS_HIP(hipMemcpyAsync(y_out, dy.p, ny * sizeof(float), hipMemcpyDeviceToHost, st));
    std::vector<uint16_t> hp;
    if (c.outputs & FS_CONV_OUT_PLANES) {
        hp.resize((size_t)B * NP * (Cout / 8) * row * 8);
        FS_HIP(hipMemcpyAsync(hp.data(), dyp.p, hp.size() * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
    }
    FS_HIP(hipStreamSynchronize(st));
    if (c.outputs & FS_CONV_OUT_PLANES) {  // planes [B][part][Cout/8][64 + T][8] -> f32 [B][Cout][64 + T]
        const size_t CG = (size_t)Cout / 8;
        auto bf = [](uint16_t h) { const uint32_t u = (uint32_t)h << 16; float f; std::memcpy(&f, &u, 4); return f; };
        for (size_t b = 0; b < (size_t)B; ++b)
            for (size_t o = 0; o < (size_t)Cout; ++o)
                for (size_t s = 0; s < row; ++s) {
                    const size_t i0 = (((b * NP) * CG + o / 8) * row + s) * 8 + o % 8;
                    float v;
                    if (f16) { _Float16 h; std::memcpy(&h, &hp[i0], 2); v = (float)h; }
                    else v = bf(hp[i0]) + bf(hp[i0 + CG * row * 8]);
                    planes_out[(b * Cout + o) * row + s] = v;
                }
    }
    FS_REQUIRE(name, "conv self-test: the launcher recorded no variant name");
    std::snprintf(variant_out, variant_cap, "%s", name);
}

// fs_selftest_codec_op (include/fishrt.h): ONE launcher of the encoder-side / ConvNeXt / FSQ kernels on host data.  The output buffer is
// [256 guard][logical extent][256 guard] 4-byte elements, all 0xFF before the launch: an element the launcher skipped returns as NaN, a
// write outside the extent shows in the guards.  Every shape is checked against the launcher's own reads before anything is launched.
void codec_op_selftest(int device, const fs_codec_op_case& c, void* out, size_t out_cap, size_t* n_out, int* guard_ok) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) throw Error("no HIP device visible: libfishrt has no CPU fallback (MI355X / gfx950 required)");
    FS_REQUIRE(device >= 0 && device < ndev, "device_id out of range");
    FS_HIP(hipSetDevice(device));
    constexpr size_t kGuard = 256;
    const int B = c.B, C = c.C, T = c.T;
    FS_REQUIRE(c.op >= FS_CODEC_OP_STFT_MAG && c.op <= FS_CODEC_OP_FSQ_PROJECT, "codec op self-test: unknown op");
    FS_REQUIRE(T >= 1 && T <= (1 << 20), "codec op self-test: 1 <= T <= 2^20");
    size_t n_x = 0, n_w[4] = {0, 0, 0, 0}, n_y = 0, n_codes = 0, n_ctx = 0;
    switch (c.op) {
    case FS_CODEC_OP_STFT_MAG: {
        FS_REQUIRE(c.n_fft >= 2 && c.n_fft <= 8192 && c.hop >= 1 && c.hop <= c.n_fft && (c.n_fft - c.hop) % 2 == 0, "codec op self-test: bad STFT shape");
        const long long pad = (c.n_fft - c.hop) / 2;
        FS_REQUIRE(c.n >= 1 && c.n >= pad && c.n < (1 << 28), "codec op self-test: the clip is shorter than the reflect padding");
        FS_REQUIRE((long long)(T - 1) * c.hop < (long long)c.n + 2 * pad, "codec op self-test: a frame starts behind the padded signal");
        n_x = (size_t)c.n; n_y = (size_t)(c.n_fft / 2 + 1) * T;
        break;
    }
    case FS_CODEC_OP_MEL_LOG:
        FS_REQUIRE(c.nf >= 1 && c.nf <= 8192 && c.n_mels >= 1 && c.n_mels <= 4096, "codec op self-test: bad mel shape");
        n_x = (size_t)c.nf * T; n_w[0] = (size_t)c.nf * c.n_mels; n_y = (size_t)c.n_mels * T;
        break;
    case FS_CODEC_OP_LAYERNORM_CF:
        FS_REQUIRE(C >= 1 && C <= 4096, "codec op self-test: 1 <= C <= 4096");
        n_x = n_y = (size_t)C * T; n_w[0] = n_w[1] = (size_t)C;
        break;
    case FS_CODEC_OP_DWCONV_LN:
        FS_REQUIRE(C >= 1 && C <= 4096 && B >= 1 && B <= 64, "codec op self-test: 1 <= C <= 4096, 1 <= B <= 64");
        FS_REQUIRE(c.ctx_mode >= 0 && c.ctx_mode <= 2, "codec op self-test: ctx_mode 0 = none, 1 = one context, 2 = per-item offsets");
        n_x = n_y = (size_t)B * C * T; n_w[0] = (size_t)C * 7; n_w[1] = n_w[2] = n_w[3] = (size_t)C;
        if (c.ctx_mode == 1) {
            FS_REQUIRE(B == 1 && c.ctx, "codec op self-test: one context needs B == 1 and ctx");
            n_ctx = (size_t)C * CODEC_CTX_F32;
        } else if (c.ctx_mode == 2) {
            FS_REQUIRE(c.ctx && c.ctx_off && c.ctx_elems >= 1 && c.ctx_elems < (1ll << 28), "codec op self-test: per-item contexts need ctx, ctx_off and ctx_elems");
            for (int b = 0; b < B; ++b)
                FS_REQUIRE(c.ctx_off[2 * b] >= 0 && c.ctx_off[2 * b] + (long long)C * CODEC_CTX_F32 <= c.ctx_elems,
                           "codec op self-test: a context offset points outside the pool");
            n_ctx = (size_t)c.ctx_elems;
        }
        break;
    case FS_CODEC_OP_SPACE_TO_DEPTH:
        FS_REQUIRE(C >= 1 && C <= 4096 && c.s >= 1 && c.s <= 16, "codec op self-test: 1 <= C <= 4096, 1 <= s <= 16");
        n_x = (size_t)C * T; n_y = (size_t)C * c.s * (T / c.s);
        break;
    case FS_CODEC_OP_FSQ_ENCODE:
        FS_REQUIRE(c.G >= 1 && c.G <= 64 && C >= c.G && C <= 4096 && C % c.G == 0, "codec op self-test: C is a multiple of G, 1 <= G <= 64, C <= 4096");
        n_x = (size_t)C * T; n_w[0] = (size_t)4 * C; n_w[1] = (size_t)4 * c.G; n_y = (size_t)c.G * T;
        break;
    default:
        FS_REQUIRE(c.G >= 1 && c.G <= 64 && c.dg >= 1 && c.dg <= 512 && B >= 1 && B <= 64, "codec op self-test: 1 <= G, B <= 64, 1 <= dg <= 512");
        FS_REQUIRE(c.codes, "codec op self-test: codes are required");
        n_codes = (size_t)B * c.G * T; n_w[0] = (size_t)c.G * c.dg * 4; n_w[1] = (size_t)c.G * c.dg; n_y = (size_t)B * c.G * c.dg * T;
        for (size_t i = 0; i < n_codes; ++i) FS_REQUIRE(c.codes[i] < 1000u, "codec op self-test: an index is outside the codebook");
        break;
    }
    FS_REQUIRE(n_x < (1u << 28) && n_y < (1u << 28), "codec op self-test: tensor above 2^28 elements");
    FS_REQUIRE(n_y <= out_cap, "codec op self-test: out capacity too small");
    const float* wsrc[4] = {c.w0, c.w1, c.w2, c.w3};
    FS_REQUIRE(!n_x || c.x, "codec op self-test: x is required");
    for (int i = 0; i < 4; ++i) FS_REQUIRE(!n_w[i] || wsrc[i], "codec op self-test: a weight tensor of this op is missing");

    hipStream_t st = nullptr;
    FS_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    struct StreamGuard { hipStream_t s; ~StreamGuard() { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } } sg{st};
    DBuf dx, dw[4], dctx, doff, dcodes, dy;
    auto up = [&](DBuf& d, const void* src, size_t bytes) {
        d.alloc(bytes);
        FS_HIP(hipMemcpyAsync(d.p, src, bytes, hipMemcpyHostToDevice, st));
    };
    if (n_x) up(dx, c.x, n_x * sizeof(float));
    for (int i = 0; i < 4; ++i) if (n_w[i]) up(dw[i], wsrc[i], n_w[i] * sizeof(float));
    if (n_ctx) up(dctx, c.ctx, n_ctx * sizeof(float));
    if (c.op == FS_CODEC_OP_DWCONV_LN && c.ctx_mode == 2) up(doff, c.ctx_off, (size_t)2 * B * sizeof(long long));
    if (n_codes) up(dcodes, c.codes, n_codes * sizeof(uint32_t));
    dy.alloc((n_y + 2 * kGuard) * 4);
    FS_HIP(hipMemsetAsync(dy.p, 0xFF, dy.n, st));
    float* y = dy.f() + kGuard;
    static_assert(sizeof(long long) == sizeof(int64_t), "ctx_off is the launchers' long long table");
    switch (c.op) {
    case FS_CODEC_OP_STFT_MAG: codec_stft_mag(dx.f(), c.n, c.n_fft, c.hop, T, y, st); break;
    case FS_CODEC_OP_MEL_LOG: codec_mel_log(dx.f(), dw[0].f(), c.nf, c.n_mels, T, y, st); break;
    case FS_CODEC_OP_LAYERNORM_CF: codec_layernorm_cf(dx.f(), C, T, dw[0].f(), dw[1].f(), y, st); break;
    case FS_CODEC_OP_DWCONV_LN:
        codec_dwconv_ln(dx.f(), B, C, T, dw[0].f(), dw[1].f(), dw[2].f(), dw[3].f(), y, st, c.ctx_mode ? dctx.f() : nullptr,
                        c.ctx_mode == 2 ? (const long long*)doff.p : nullptr);
        break;
    case FS_CODEC_OP_SPACE_TO_DEPTH: codec_space_to_depth(dx.f(), C, T, c.s, y, st); break;
    case FS_CODEC_OP_FSQ_ENCODE: codec_fsq_encode(dx.f(), C, T, c.G, dw[0].f(), dw[1].f(), (uint32_t*)y, st); break;
    default: codec_fsq_project((const uint32_t*)dcodes.p, B, c.G, T, dw[0].f(), dw[1].f(), c.dg, y, st, c.item_rows != 0); break;
    }
    std::vector<uint32_t> host(n_y + 2 * kGuard);
    FS_HIP(hipMemcpyAsync(host.data(), dy.p, dy.n, hipMemcpyDeviceToHost, st));
    FS_HIP(hipStreamSynchronize(st));
    bool intact = true;
    for (size_t i = 0; i < kGuard; ++i) intact = intact && host[i] == 0xFFFFFFFFu && host[kGuard + n_y + i] == 0xFFFFFFFFu;
    if (n_y) std::memcpy(out, host.data() + kGuard, n_y * 4);
    *n_out = n_y;
    *guard_ok = intact ? 1 : 0;
}

}  // namespace fs
