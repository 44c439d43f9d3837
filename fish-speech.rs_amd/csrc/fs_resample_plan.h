// Sample-rate conversion, the host side: the two definitions' lengths, the sinc tap table, and how many output samples a stream may emit
// after N input samples.  The kernels (codec_resample.hip) compute; this header counts and launches nothing.
//
// Linear = fish_speech_core/lib/audio/functional.rs:3-37, bit for bit:
//   ratio = (double)to / (double)from;  out_len = ceil((double)n * ratio)
//   output i: idx = (double)i / ratio (an f64 division);  f = floor(idx), c = min(ceil(idx), n - 1)
//             t = (float)(idx - (double)f), u = 1.0f - t;  out = x[f] * u + x[c] * t -- two f32 products, rounded separately, one f32 add
//             (f64 rounding can make the last f equal n, where the reference's gather fails: f is clamped to n - 1 as well, t is not)
// Sinc = a Hann-windowed sinc polyphase filter (the construction of torchaudio's sinc_interp_hann, W = 6 zero crossings, rolloff 0.99):
//   g = gcd(from, to), o = from / g, p = to / g;  base = min(o, p) * rolloff, width = ceil(W * o / base), K = 2 * width + o taps
//   h[j][k] = sinc(t) * cos(pi t / (2 W))^2 * base / o with t = clamp((-j / p + (k - width) / o) * base, -W, W), built in f64, stored f32
//   out[m * p + j] = sum_{k = 0 .. K-1} h[j][k] * x[m * o + k - width], x = 0 outside [0, n), f32 accumulation in ASCENDING k
//   out_len = ceil(p * n / o) in integers
// Every output sample is a function of its absolute index and the input samples alone, so a stream cut into chunks anywhere gives the
// samples of the one-shot call as long as no output is emitted before all its inputs exist:
//   linear, not final: every i with ceil(i / ratio) <= N - 1 -- the predicate evaluated with the kernel's own f64 expression
//   sinc, not final:   every whole block m (p outputs) with m * o + width + o - 1 <= N - 1
//   final:             everything up to out_len(N); only here the clamp to n - 1 and the right zero pad act
// The carry of a stream is the input samples an output not yet emitted still reads: at most 1 (linear), fewer than K + o (sinc).
// Plain C++ -- no HIP in here -- so that a host program can run it under a sanitizer (tools/resample_plan_check.cpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace fs {

// == FS_RESAMPLE_LINEAR / FS_RESAMPLE_SINC (include/fishrt.h); kResampleCopy is the engine's own: output i = input i (format conversion only)
enum { kResampleLinear = 0, kResampleSinc = 1, kResampleCopy = 2 };
constexpr int kSincZeros = 6;                     // W
constexpr double kSincRolloff = 0.99;
constexpr int64_t kSincMaxTable = (int64_t)1 << 20;  // p x K entries

struct ResampleRates {
    int from = 0, to = 0;
    double ratio = 1.0;        // linear
    int64_t o = 1, p = 1;      // sinc: from / g, to / g
    int64_t width = 0, K = 0;
    double base = 0.0;
};

inline ResampleRates resample_rates(int from, int to) {
    if (from <= 0 || to <= 0) throw std::invalid_argument("resample: sample rates must be positive");
    ResampleRates r;
    r.from = from; r.to = to;
    r.ratio = (double)to / (double)from;
    int64_t a = from, b = to;
    while (b) { const int64_t t = a % b; a = b; b = t; }
    r.o = from / a; r.p = to / a;
    r.base = (double)std::min(r.o, r.p) * kSincRolloff;
    r.width = (int64_t)std::ceil((double)kSincZeros * (double)r.o / r.base);
    r.K = 2 * r.width + r.o;
    return r;
}

inline bool resample_table_fits(const ResampleRates& r) { return r.p <= kSincMaxTable && r.K <= kSincMaxTable && r.p * r.K <= kSincMaxTable; }
inline void resample_require_table(const ResampleRates& r) {
    if (!resample_table_fits(r))
        throw std::invalid_argument("sinc resampling " + std::to_string(r.from) + " -> " + std::to_string(r.to) + " Hz needs a tap table of " +
                                    std::to_string(r.p) + " x " + std::to_string(r.K) + " entries (limit 2^20): refused");
}

inline int64_t resample_out_len(const ResampleRates& r, int mode, int64_t n) {
    if (n <= 0) return 0;
    if (mode == kResampleCopy) return n;
    if (mode == kResampleLinear) return (int64_t)std::ceil((double)n * r.ratio);
    return (r.p * n + r.o - 1) / r.o;
}

// one tap in f64, and the f32 table [p][K] the kernels read
inline double resample_tap_f64(const ResampleRates& r, int64_t j, int64_t k) {
    const double pi = 3.14159265358979323846, W = (double)kSincZeros;
    double t = (-(double)j / (double)r.p + (double)(k - r.width) / (double)r.o) * r.base;
    t = std::min(W, std::max(-W, t));
    const double win = std::cos(t * pi / W / 2.0), s = t == 0.0 ? 1.0 : std::sin(pi * t) / (pi * t);
    return s * win * win * (r.base / (double)r.o);
}
inline std::vector<float> resample_taps(const ResampleRates& r) {
    resample_require_table(r);
    std::vector<float> h((size_t)(r.p * r.K));
    for (int64_t j = 0; j < r.p; ++j)
        for (int64_t k = 0; k < r.K; ++k) h[(size_t)(j * r.K + k)] = (float)resample_tap_f64(r, j, k);
    return h;
}

// the two definitions evaluated on the host.  Linear: the reference's own dtype sequence, so exact.  Sinc: f64 taps, f64 sum.
inline float resample_linear_eval(const float* x, int64_t n, const ResampleRates& r, int64_t i) {
    const double idx = (double)i / r.ratio;
    const double fl = std::floor(idx);
    const int64_t f = std::min((int64_t)fl, n - 1), c = std::min((int64_t)std::ceil(idx), n - 1);
    const float t = (float)(idx - fl), u = 1.0f - t;
    volatile float a = x[f] * u, b = x[c] * t;  // (volatile: two roundings, no contraction into one FMA)
    return a + b;
}
inline double resample_sinc_eval(const float* x, int64_t n, const ResampleRates& r, int64_t i) {
    const int64_t m = i / r.p, j = i % r.p;
    double acc = 0.0;
    for (int64_t k = 0; k < r.K; ++k) {
        const int64_t a = m * r.o + k - r.width;
        if (a >= 0 && a < n) acc += resample_tap_f64(r, j, k) * (double)x[a];
    }
    return acc;
}

// ---- streams.  How many outputs exist after N inputs
inline bool resample_linear_ready(const ResampleRates& r, int64_t i, int64_t N) { return (int64_t)std::ceil((double)i / r.ratio) <= N - 1; }
inline int64_t resample_emittable(const ResampleRates& r, int mode, int64_t N, bool final) {
    if (final) return resample_out_len(r, mode, N);
    if (N <= 0) return 0;
    if (mode == kResampleCopy) return N;
    if (mode == kResampleLinear) {
        // a first guess, then the predicate decides (i / ratio is monotone in i, so the ready outputs are a prefix)
        int64_t i = std::max<int64_t>(0, (int64_t)std::floor((double)(N - 1) * r.ratio));
        while (i > 0 && !resample_linear_ready(r, i - 1, N)) --i;
        while (resample_linear_ready(r, i, N)) ++i;
        return std::min(i, resample_out_len(r, mode, N));
    }
    if (N < r.width + r.o) return 0;
    return ((N - r.width - r.o) / r.o + 1) * r.p;
}
// the first input sample an output from n_out on still reads (clamped to [0, N])
inline int64_t resample_carry_start(const ResampleRates& r, int mode, int64_t n_out, int64_t N) {
    if (mode == kResampleCopy) return N;
    const int64_t s = mode == kResampleLinear ? (int64_t)std::floor((double)n_out / r.ratio) : (n_out / r.p) * r.o - r.width;
    return std::min(N, std::max<int64_t>(0, s));
}
// samples of one carry row: the bound of carry_len in either mode
inline int64_t resample_carry_cap(const ResampleRates& r, int mode) { return mode == kResampleSinc ? r.K + r.o : 2; }

struct ResampleBook {  // one stream: input samples seen, output samples emitted, input samples kept for the outputs still to come
    int64_t n_in = 0, n_out = 0, carry_len = 0;
    bool final = false;
};
struct ResampleStep {  // what a call that feeds n_new samples does to a book; planning changes nothing
    int64_t in0 = 0, out0 = 0, n_emit = 0, n_total = 0, carry_len = 0;
};
inline ResampleStep resample_plan_step(const ResampleRates& r, int mode, const ResampleBook& b, int64_t n_new, bool final) {
    if (b.final) throw std::invalid_argument("resample: the stream was already flushed");
    ResampleStep s;
    s.in0 = b.n_in; s.out0 = b.n_out; s.n_total = b.n_in + n_new;
    s.n_emit = resample_emittable(r, mode, s.n_total, final) - b.n_out;
    s.carry_len = final ? 0 : s.n_total - resample_carry_start(r, mode, b.n_out + s.n_emit, s.n_total);
    return s;
}
inline void resample_commit(ResampleBook& b, const ResampleStep& s, bool final) {
    b.n_in = s.n_total; b.n_out = s.out0 + s.n_emit; b.carry_len = s.carry_len; b.final = final;
}

}  // namespace fs
