// Device time-scale modification of PCM rows (codec_tsm.hip): one launch walks every row's frames in order and writes the frame positions,
// a second, fully parallel one overlap-adds the output.  The definition and the counting are fs_tsm_plan.h's; this is the arithmetic.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <vector>

#include "fs_tsm_plan.h"

namespace fs {

// one row of a ragged call: x = src[0 .. n), zero outside; out_len = tsm_out_len(n, speed) samples go to out, the K = tsm_frames(out_len)
// positions to pos (device, int64; never null when K > 0)
struct TsmItem {
    const float* src = nullptr;
    float* out = nullptr;
    long long* pos = nullptr;
    long long n = 0, out_len = 0, K = 0;
    int wg0 = 0;  // first workgroup of the row in the overlap-add launch (filled by TimeStretcher::run)
};

constexpr int kTsmWg = 256;       // threads of the overlap-add kernel, one output sample each
constexpr int kTsmChainWg = 512;  // threads of the chain kernel: two waves per SIMD, so that a SIMD issues a vector instruction every 2 cycles
constexpr int kTsmLags = 13;      // adjacent lags one thread accumulates: every template / candidate sample it reads from LDS feeds 13 sums

// the window tables of the frame lengths seen so far (device), the item upload, the two launches.  All work goes to `st`; run() does not
// synchronise (but for the first call with a frame length, which uploads that window), and the caller must before it calls run() again or
// frees what the items point at.
class TimeStretcher {
  public:
    explicit TimeStretcher(hipStream_t st) : st_(st) {}
    ~TimeStretcher();
    TimeStretcher(const TimeStretcher&) = delete;
    TimeStretcher& operator=(const TimeStretcher&) = delete;
    // the caller fills src / n / out / pos of every row; out_len, K and wg0 are counted here.  Rows with out_len == 0 cost nothing
    void run(const std::vector<TsmItem>& items, double speed, const TsmParams& p);

  private:
    hipStream_t st_;
    std::map<int, float*> windows_;
    std::vector<TsmItem> h_items_;
    void* d_items_ = nullptr;
    size_t d_items_cap_ = 0;
    const float* window(int N);
};

}  // namespace fs
