// Device sample-rate conversion for the vocoder's output and the encoder's input (no reference kernel: the reference resamples on the
// CPU, fish_speech_core/lib/audio/functional.rs:3-37, called from server/lib/handlers/speech.rs:184-216 and encode_speech.rs:50-54).
// The definitions are in fs_resample_plan.h.  Two rules make a stream cut into chunks give the samples of the one-shot call, bit for bit:
//   * ABSOLUTE INDICES: an output sample is a function of its absolute output index and of the input samples at absolute input indices;
//     a row only says where those samples are to be found (carry row, source row, or nowhere = zero), never where a chunk began;
//   * FIXED ORDER: a sinc output is accumulated by ONE thread, acc = fma(h[j][k], x, acc) for k = 0 .. K-1 ascending, from acc = 0, zero
//     samples included -- the same instruction sequence whether the window sits in LDS, in global memory, in one chunk or across two.
// The linear mode keeps the reference's roundings: an f64 division per output, two f32 products rounded separately, one f32 add
// (__fmul_rn / __fadd_rn: the build contracts a * b + c into an FMA otherwise, which changes the last bit).
#include "codec_resample.h"

#include <algorithm>

#include "fs_common.h"

namespace fs {

#define FS_LAUNCH_CHECK() FS_HIP(hipGetLastError())

namespace {

constexpr int kLdsWindow = 4096;  // f32 samples of input window a workgroup stages (16 KiB); a wider window is read from global memory

__device__ __forceinline__ float rs_fetch(const ResampleItem& it, long long a) {
    if (a < 0 || a >= it.in0 + it.n_src) return 0.f;
    if (a >= it.in0) return it.src[a - it.in0];
    const long long c = a - (it.in0 - (long long)it.carry_len);
    return c >= 0 ? it.carry[c] : 0.f;
}

// fishrt/wav.py pcm_to_i16 (wav.rs:27-58): clip to [-1, 1], times 32767, truncate toward zero; NaN -> 0
__device__ __forceinline__ int16_t rs_to_i16(float v) {
    if (v != v) return 0;
    const float c = fminf(fmaxf(v, -1.0f), 1.0f);
    return (int16_t)(int)truncf(__fmul_rn(c, 32767.0f));
}

__global__ __launch_bounds__(kResampleWg) void k_resample(const ResampleItem* __restrict__ items, int n_items) {
    __shared__ float win[kLdsWindow];
    const int bid = (int)blockIdx.x, tid = (int)threadIdx.x;
    int ii = 0;
    while (ii + 1 < n_items && items[ii + 1].wg0 <= bid) ++ii;
    const ResampleItem it = items[ii];
    const long long l0 = (long long)(bid - it.wg0) * kResampleWg;  // first output of this workgroup, relative to the row's out0
    if (l0 >= it.n_out) return;                                     // (uniform)
    const long long l = l0 + tid, q = it.out0 + l;
    const bool live = l < it.n_out;
    float v = 0.f;
    if (it.mode == kResampleSinc) {
        const long long qa = it.out0 + l0, qb = it.out0 + min(l0 + (long long)kResampleWg, it.n_out) - 1;
        const long long ma = qa / it.p, mb = qb / it.p;
        const long long w0 = ma * it.o - it.width, wlen = (mb - ma) * it.o + it.K;
        const bool staged = wlen <= (long long)kLdsWindow;  // (uniform)
        if (staged) {
            for (int t = tid; t < (int)wlen; t += kResampleWg) win[t] = rs_fetch(it, w0 + t);
            __syncthreads();
        }
        if (live) {
            const long long m = q / it.p;
            const int j = (int)(q - m * it.p);
            const float* __restrict__ h = it.taps_t + j;
            float acc = 0.f;
            if (staged) {
                const float* x = win + (int)((m - ma) * it.o);
                for (int k = 0; k < it.K; ++k) acc = fmaf(h[(size_t)k * it.p], x[k], acc);
            } else {
                const long long a0 = m * it.o - it.width;
                for (int k = 0; k < it.K; ++k) acc = fmaf(h[(size_t)k * it.p], rs_fetch(it, a0 + k), acc);
            }
            v = acc;
        }
    } else if (live) {
        if (it.mode == kResampleLinear) {
            const long long N = it.in0 + it.n_src;
            const double idx = (double)q / it.ratio;
            const double fl = floor(idx);
            const long long f = min((long long)fl, N - 1), c = min((long long)ceil(idx), N - 1);
            const float t = (float)(idx - fl), u = __fsub_rn(1.0f, t);
            v = __fadd_rn(__fmul_rn(rs_fetch(it, f), u), __fmul_rn(rs_fetch(it, c), t));
        } else {
            v = rs_fetch(it, q);
        }
    }
    if (!live) return;
    if (it.format == kPcmS16) ((int16_t*)it.out)[l] = rs_to_i16(v);
    else ((float*)it.out)[l] = v;
}

// one workgroup per row: carry_out = the last new_carry_len samples the row has seen.  carry_out is the stream's other half, so the reads of
// the old carry and these writes never meet.
__global__ __launch_bounds__(256) void k_resample_carry(const ResampleItem* __restrict__ items) {
    const ResampleItem it = items[blockIdx.x];
    if (!it.carry_out) return;
    const long long a0 = it.in0 + it.n_src - (long long)it.new_carry_len;
    for (int t = (int)threadIdx.x; t < it.new_carry_len; t += 256) it.carry_out[t] = rs_fetch(it, a0 + t);
}

__global__ __launch_bounds__(256) void k_downmix(const float* __restrict__ x, int channels, long long frames, float* __restrict__ out) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= frames) return;
    const float* r = x + f * channels;
    float s = r[0];
    for (int c = 1; c < channels; ++c) s = __fadd_rn(s, r[c]);
    out[f] = __fdiv_rn(s, (float)channels);
}

}  // namespace

Resampler::~Resampler() {
    for (auto& t : taps_) (void)hipFree(t.second);
    if (d_items_) (void)hipFree(d_items_);
}

void Resampler::set_rates(ResampleItem& it, const ResampleRates& r, int mode) {
    it.mode = mode;
    it.ratio = r.ratio;
    if (mode != kResampleSinc) return;
    resample_require_table(r);
    it.o = (int)r.o; it.p = (int)r.p; it.width = (int)r.width; it.K = (int)r.K;
    auto key = std::make_pair(r.from, r.to);
    auto f = taps_.find(key);
    if (f == taps_.end()) {
        const std::vector<float> h = resample_taps(r);
        std::vector<float> ht(h.size());  // [K][p]: the threads of a wave walk the phases, so their loads of one tap are neighbours
        for (int64_t j = 0; j < r.p; ++j)
            for (int64_t k = 0; k < r.K; ++k) ht[(size_t)(k * r.p + j)] = h[(size_t)(j * r.K + k)];
        float* d = nullptr;
        FS_HIP(hipMalloc(&d, ht.size() * sizeof(float)));
        f = taps_.emplace(key, d).first;
        FS_HIP(hipMemcpyAsync(d, ht.data(), ht.size() * sizeof(float), hipMemcpyHostToDevice, st_));
        FS_HIP(hipStreamSynchronize(st_));  // ht goes out of scope
    }
    it.taps_t = f->second;
}

void Resampler::run(const std::vector<ResampleItem>& items) {
    if (items.empty()) return;
    h_items_ = items;
    long long wg = 0;
    bool carries = false;
    for (auto& it : h_items_) {
        FS_REQUIRE(it.n_out >= 0 && it.n_src >= 0 && it.carry_len >= 0 && it.new_carry_len >= 0, "resample item: negative count");
        FS_REQUIRE(it.n_out == 0 || it.out, "resample item: no output row");
        FS_REQUIRE(it.n_src == 0 || it.src, "resample item: no source row");
        FS_REQUIRE(it.carry_len == 0 || it.carry, "resample item: no carry row");
        FS_REQUIRE(it.mode != kResampleSinc || (it.taps_t && it.K >= 1 && it.p >= 1 && it.o >= 1), "resample item: no tap table");
        FS_REQUIRE(!it.carry_out || (it.carry_out != it.carry && (long long)it.new_carry_len <= (long long)it.carry_len + it.n_src),
                   "resample item: the new carry");
        FS_REQUIRE(wg < (1ll << 30), "resample: too many output samples in one call");
        it.wg0 = (int)wg;
        wg += (it.n_out + kResampleWg - 1) / kResampleWg;
        carries |= it.carry_out != nullptr;
    }
    FS_REQUIRE(wg < (1ll << 30), "resample: too many output samples in one call");
    const size_t bytes = h_items_.size() * sizeof(ResampleItem);
    if (bytes > d_items_cap_) {
        if (d_items_) (void)hipFree(d_items_);
        d_items_ = nullptr; d_items_cap_ = 0;
        FS_HIP(hipMalloc(&d_items_, bytes));
        d_items_cap_ = bytes;
    }
    FS_HIP(hipMemcpyAsync(d_items_, h_items_.data(), bytes, hipMemcpyHostToDevice, st_));
    const int n = (int)h_items_.size();
    if (wg > 0) {
        hipLaunchKernelGGL(k_resample, dim3((unsigned)wg), dim3(kResampleWg), 0, st_, (const ResampleItem*)d_items_, n);
        FS_LAUNCH_CHECK();
    }
    if (carries) {
        hipLaunchKernelGGL(k_resample_carry, dim3((unsigned)n), dim3(256), 0, st_, (const ResampleItem*)d_items_);
        FS_LAUNCH_CHECK();
    }
}

void codec_downmix(const float* x, int channels, long long frames, float* out, hipStream_t st) {
    FS_REQUIRE(channels >= 1 && frames >= 1 && frames < (1ll << 38), "downmix: channels and frames");
    hipLaunchKernelGGL(k_downmix, dim3((unsigned)((frames + 255) / 256)), dim3(256), 0, st, x, channels, frames, out);
    FS_LAUNCH_CHECK();
}

}  // namespace fs
