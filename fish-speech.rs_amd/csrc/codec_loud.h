// Device loudness measurement and normalisation of PCM rows (codec_loud.hip): BS.1770 integrated loudness with both gates, the sample peak,
// the gain and the gain multiply, ragged over the rows of a call.  The definition and the counting are fs_loud_plan.h's; this is the
// arithmetic.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <vector>

#include "fs_loud_plan.h"

namespace fs {

// one row of a ragged call: x = src[0 .. n); out (nullable: measure only) receives n samples.  The rest is counted by Loudness::run
struct LoudItem {
    const float* src = nullptr;
    float* out = nullptr;
    long long n = 0;
    long long chunk0 = 0;  // the row's first chunk record (kLoudWg records per workgroup)
    long long hop0 = 0;    // the row's first word in the hop workspace: s_i, then m_j, then l_j, nb words each
    int wg0 = 0, nwg = 0;  // the row's workgroups in the scan, energy and gain launches: kLoudSpan samples each
    int h = 0, nb = 0;     // hop length and whole hops
};

// the per-rate tables (device), the item upload, the workspaces and the launches.  All work goes to `st`; run() does not synchronise (but for
// the first call at a rate, which uploads that rate's tables), and the caller must before it calls run() again, reads results() or frees what
// the items point at.
class Loudness {
  public:
    explicit Loudness(hipStream_t st) : st_(st) {}
    ~Loudness();
    Loudness(const Loudness&) = delete;
    Loudness& operator=(const Loudness&) = delete;
    // the caller fills src / n / out of every row (n <= kLoudMaxSamples) and has validated rate and *p.  p null: measure only, gain 1.  Rows
    // whose out is null are not written.
    void run(const std::vector<LoudItem>& items, int rate, const LoudParams* p);
    const LoudResult* results() const { return (const LoudResult*)d_res_.p; }  // device, one per row of the last run
    const double* hops(size_t row) const { return (const double*)d_ws_.p + h_items_[row].hop0; }  // device, the row's s_i (nb of them)
    int64_t n_hops(size_t row) const { return h_items_[row].nb; }

  private:
    struct Buf {
        void* p = nullptr;
        size_t cap = 0;
        void ensure(size_t bytes);
        ~Buf();
    };
    hipStream_t st_;
    std::map<int, double*> tables_;
    std::vector<LoudItem> h_items_;
    Buf d_items_, d_pre_, d_agg_, d_pe_, d_pk_, d_ws_, d_res_;
    const double* tables(int rate);
};

}  // namespace fs
