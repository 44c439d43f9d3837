// Host-side engine of the Firefly-GAN-VQ vocoder (FireflyCodec::decode, codec/firefly.rs:42-48).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

namespace fs {

class CodecBase {
  public:
    virtual ~CodecBase() {}
    virtual void load_synthetic(uint64_t seed) = 0;
    virtual void load_safetensors(const std::string& path) = 0;
    virtual void decode(const uint32_t* codes, int b, int T, float* pcm_out) = 0;
    // stateful streaming: consecutive chunks of ONE code sequence; concatenated PCM == decode of the whole sequence, bit for bit
    virtual void stream_begin() = 0;
    virtual void stream_decode(const uint32_t* codes, int T, float* pcm_out) = 0;
    virtual void stream_end() = 0;
    // many concurrent streams on one handle (fs_codec_streams_*): one call advances n streams by T frames each; codes [n][8][T] per item
    virtual int streams_open() = 0;
    virtual void streams_close(int id) = 0;
    virtual void streams_decode(int n, const int* ids, const uint32_t* codes, int T, float* pcm_out) = 0;
    // ragged: item i advances stream ids[i] by T[i] >= 1 frames; codes = the items' (8, T[i]) blocks concatenated, pcm_out = their PCM concatenated
    virtual void streams_decode_ragged(int n, const int* ids, const int* T, const uint32_t* codes, float* pcm_out) = 0;
    virtual void encode(const float* pcm, int n, uint32_t* codes_out, size_t cap, size_t* L_out) = 0;
    // fs_selftest_codec_encode_stage: encode() with one intermediate tensor copied out (stage -1 .. 6), or the mel table (stage -2)
    virtual void encode_stage(const float* pcm, int n, int stage, float* out, size_t cap, size_t* n_out) = 0;
    // ---- device sample-rate conversion of the PCM (fs_codec_*_pcm, include/fishrt.h; codec_resample.hip).  spec = {rate, mode, format}
    virtual void decode_pcm(const uint32_t* codes, int b, int T, const int* spec3, void* out, size_t cap, int64_t* n_out) = 0;
    // fs_codec_decode_speed: the rows time-stretched (codec_tsm.hip, default parameters) between the vocoder and the stage above
    virtual void decode_speed(const uint32_t* codes, int b, int T, double speed, const int* spec3, void* out, size_t cap, int64_t* n_out) = 0;
    // fs_codec_decode_loud: the rows measured and scaled (codec_loud.hip) between the vocoder and the stretch stage.  loud3 = {target_lufs,
    // peak_db, max_gain_db} or null (then it is decode_speed); res24 = b fs_loud_result records or null
    virtual void decode_loud(const uint32_t* codes, int b, int T, const double* loud3, double speed, const int* spec3, void* out, size_t cap,
                             int64_t* n_out, void* res24) = 0;
    virtual int streams_open_pcm(const int* spec3) = 0;
    // fs_codec_streams_open_speed: a stream with a stretch stage between the vocoder and its resample / format stage; spec3 null = codec rate, f32
    virtual int streams_open_speed(double speed, const int* spec3) = 0;
    virtual int64_t streams_pending(int id, int T, bool final) = 0;
    virtual void streams_decode_pcm(int n, const int* ids, const int* T, const uint8_t* final, const uint32_t* codes, void* out,
                                    size_t cap_bytes, int64_t* n_out) = 0;
    virtual void encode_pcm(const float* pcm, int channels, int64_t frames, int rate, int mode, uint32_t* codes_out, size_t cap,
                            size_t* L_out) = 0;
    virtual int sample_rate() = 0;
    virtual void set_precision(int mode) = 0;  // 0 = f32 (exact f32 products), 1 = bf16x3, 2 = f16 (default); decode only
    virtual int precision() = 0;
    virtual void set_range_check(bool on) = 0;      // fs_codec_set_range_check
    virtual void range_stats(uint64_t* out5, double* last_rms) = 0;   // fs_codec_range_stats
};

CodecBase* make_codec(int device, int channel_div);

}  // namespace fs

struct fs_conv_case;  // include/fishrt.h
struct fs_codec_op_case;

namespace fs {

// fs_resample: b host rows of their own lengths, host -> device -> host, no codec handle
void resample_rows(int device, const float* pcm, int b, size_t stride, const int64_t* n_samples, int from_rate, const int* spec3, void* out,
                   size_t out_stride, int64_t* out_len);

// fs_time_stretch: b host rows of their own lengths, host -> device -> host, no codec handle; params2 = {frame, radius} or null
void time_stretch_rows(int device, const float* pcm, int b, size_t stride, const int64_t* n_samples, double speed, const int* params2, float* out,
                       size_t out_stride, int64_t* out_len, int64_t* positions, size_t pos_stride);

// fs_loudness_normalize: b host rows of their own lengths, host -> device -> host, no codec handle; loud3 as above or null (measure only, out
// null too), out null = measure only; res24 = b fs_loud_result records.  hops (nullable, b == 1): the row's hop energies s_i
void loudness_rows(int device, const float* pcm, int b, size_t stride, const int64_t* n_samples, int rate, const double* loud3, float* out,
                   size_t out_stride, void* res24, double* hops, size_t hops_cap, int64_t* n_hops);

// fs_selftest_tsm_chunks: one host row through the chunked stretch, one launch pair per chunk (the last chunk is final); params2 as above
void time_stretch_chunks(int device, const float* pcm, int64_t n, const int64_t* chunks, int n_chunks, double speed, const int* params2, float* out,
                         size_t out_cap, int64_t* out_len, int64_t* emitted, int64_t* positions, size_t pos_cap, int64_t* n_pos);

// fs_selftest_conv1d: one conv through re-layout, pack, plane producers and one launcher of codec_kernels.h (see include/fishrt.h)
void codec_conv_selftest(int device, const fs_conv_case& c, float* y_out, float* planes_out, char* variant_out, size_t variant_cap,
                         uint64_t* range_out);

// fs_selftest_codec_op: one encoder-side / ConvNeXt / FSQ launcher of codec_kernels.h on host data, output poisoned and guarded (see include/fishrt.h)
void codec_op_selftest(int device, const fs_codec_op_case& c, void* out, size_t out_cap, size_t* n_out, int* guard_ok);

}  // namespace fs
