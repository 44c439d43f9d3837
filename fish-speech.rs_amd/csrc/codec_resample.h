// Device sample-rate conversion (codec_resample.hip): one ragged launch converts the rows of a call, a second small one writes the carries
// of the streams among them, and a downmix kernel serves the encode path.  Counting is fs_resample_plan.h's; this is the arithmetic.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <utility>
#include <vector>

#include "fs_resample_plan.h"

namespace fs {

enum { kPcmF32 = 0, kPcmS16 = 1 };  // == FS_PCM_F32 / FS_PCM_S16 (include/fishrt.h)

// one row of a ragged call.  Absolute input index a lives at src[a - in0] for in0 <= a < in0 + n_src, at carry[a - (in0 - carry_len)] for the
// carry_len samples in front of in0, and is zero everywhere else.  Output q (absolute) goes to out[q - out0], q in [out0, out0 + n_out).
struct ResampleItem {
    const float* src = nullptr;
    const float* carry = nullptr;
    float* carry_out = nullptr;      // new carry = the last new_carry_len samples of (carry ++ src); never the row `carry` points at
    void* out = nullptr;             // float or int16_t, by `format`
    const float* taps_t = nullptr;   // sinc: the tap table transposed, [K][p]
    long long in0 = 0, n_src = 0, out0 = 0, n_out = 0;
    double ratio = 1.0;
    int o = 1, p = 1, width = 0, K = 0;
    int carry_len = 0, new_carry_len = 0, mode = kResampleLinear, format = kPcmF32;
    int wg0 = 0;                     // first workgroup of the row (filled by Resampler::run)
};

constexpr int kResampleWg = 256;  // outputs per workgroup, one per thread

// the tap tables of the rate pairs seen so far (device, transposed), the item upload, the two launches.  All work goes to `st`; run() does not
// synchronise, and the caller must before it changes `items` storage again (the upload reads the vector's copy kept inside).
class Resampler {
  public:
    explicit Resampler(hipStream_t st) : st_(st) {}
    ~Resampler();
    Resampler(const Resampler&) = delete;
    Resampler& operator=(const Resampler&) = delete;
    // fills the rate fields of an item (ratio, o, p, width, K, taps_t); sinc builds and uploads the pair's table on first use
    void set_rates(ResampleItem& it, const ResampleRates& r, int mode);
    void run(const std::vector<ResampleItem>& items);

  private:
    hipStream_t st_;
    std::map<std::pair<int, int>, float*> taps_;
    std::vector<ResampleItem> h_items_;
    void* d_items_ = nullptr;
    size_t d_items_cap_ = 0;
};

// interleaved [frames][channels] f32 -> mono: the channels summed in order in f32, divided by (float)channels
void codec_downmix(const float* x, int channels, long long frames, float* out, hipStream_t st);

}  // namespace fs
