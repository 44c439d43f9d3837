// Device time-scale modification of PCM rows (codec_tsm.hip): one launch walks every row's frames in order and writes the frame positions,
// a second, fully parallel one overlap-adds the output.  The definition and the counting are fs_tsm_plan.h's; this is the arithmetic.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <vector>

#include "fs_tsm_plan.h"

namespace fs {

// one row of a ragged call, a window of a stream.  Absolute input index a lives at src[a - in0] for in0 <= a < n (n = the samples the stream has
// seen, this chunk's included), at carry[a - (in0 - carry_len)] for the carry_len samples in front of in0, and is zero below 0 and from n on (only a
// final item's frames read there: fs_tsm_plan.h).  The item places frames [k0, k1) and writes output samples [k0 Hs, k0 Hs + out_len) to
// out[m - k0 Hs].  pos (device, int64; never null when k1 > 0) holds p_k at pos[k - pos0]: a one-shot row has pos0 = 0, a stream's item
// pos0 = k0 - 1, so that its first entry is p_{k0 - 1}, which the chain kernel copies there from `state` -- the stream's device-resident
// position word, read at entry and written (p_{k1 - 1}) at exit.  carry_out (the stream's other carry row; never the row `carry` points at)
// receives the last new_carry_len samples of (carry ++ src).  A one-shot row is k0 = 0, k1 = K, no carry, no state.
struct TsmItem {
    const float* src = nullptr;
    float* out = nullptr;
    long long* pos = nullptr;
    long long n = 0, out_len = 0, K = 0;  // one-shot rows (TimeStretcher::run): the caller fills src / n / out / pos, run() the rest
    int wg0 = 0;  // first workgroup of the row in the overlap-add launch (filled by run / run_items)
    int carry_len = 0, new_carry_len = 0;
    const float* carry = nullptr;
    float* carry_out = nullptr;
    long long* state = nullptr;
    long long in0 = 0, k0 = 0, k1 = 0, pos0 = 0;
    double speed = 1.0;
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
    // windows of streams: the caller fills every field but wg0 (K is not read), from a TsmStep each; one launch pair for all of them
    void run_items(const std::vector<TsmItem>& items, const TsmParams& p);

  private:
    hipStream_t st_;
    std::map<int, float*> windows_;
    std::vector<TsmItem> h_items_;
    void* d_items_ = nullptr;
    size_t d_items_cap_ = 0;
    const float* window(int N);
    void launch(const TsmParams& p);  // h_items_, checked and with wg0 set -> the two launches
};

}  // namespace fs
