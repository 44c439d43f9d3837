// Time-scale modification of PCM (the `speed` of a request), the host side: lengths, frame positions, parameter checks, the window table and
// a plain C++ evaluator of the whole definition.  The kernels (codec_tsm.hip) compute; this header counts and launches nothing.
//
// WSOLA with a squared-difference measure (include/fishrt.h holds the same text):
//   frame N (even, 64 .. 2048; default 1024), synthesis hop Hs = N / 2, search radius D (0 .. 1024; default 512)
//   input x: f32, n samples, zero outside [0, n);  speed: a double in [0.25, 4.0]
//   out_len = floor(n / speed + 0.5) in f64;  K = ceil(out_len / Hs) frames;  q_k = floor(k * Hs * speed + 0.5) in f64
//   p_0 = 0.  For k >= 1: template t[i] = x[p_{k-1} + Hs + i], i < N;  e[d] = sum_{i < N} (t[i] - x[q_k + d + i])^2 for d in [-D, D];
//             p_k = q_k + d*, d* the lag of the smallest e; among equal e the smallest |d|, of +-d the negative one.
//   window w[i] = 0.5 - 0.5 cos(2 pi i / N), built in f64, stored f32
//   output m, k = m / Hs, i = m - k * Hs:  k == 0: y[m] = x[m];  k >= 1: y[m] = w[i + Hs] * x[p_{k-1} + Hs + i] + w[i] * x[p_k + i], the two
//             f32 products rounded separately, then one f32 add.
// THE ORDER OF e[d], the same for every lag (kTsmSegs = 6, seg = ceil(N / 6)):
//   segment s = 0 .. 5 covers i in [s * seg, min(N, (s + 1) * seg));  within it, from a = 0 and in ascending i:
//       df = t[i] - x[q_k + d + i] (one f32 subtraction);  a = fmaf(df, df, a) (one rounding)
//   e[d] = ((((a_0 + a_1) + a_2) + a_3) + a_4) + a_5, five f32 additions.
// A lag's e is a function of the values it reads alone, so a signal that repeats bit for bit with period P has e[d] == e[d + P] bitwise.
// A lag whose e is NaN never wins; when no lag's e is below +inf, d* = 0.
// Plain C++ -- no HIP in here -- so that a host program can run it under a sanitizer (tools/tsm_plan_check.cpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

namespace fs {

constexpr int kTsmFrame = 1024, kTsmRadius = 512;  // the defaults; the vocoder path always uses them
constexpr int kTsmSegs = 6;                        // partial sums of one lag's e
constexpr double kTsmSpeedMin = 0.25, kTsmSpeedMax = 4.0;

struct TsmParams {
    int N = kTsmFrame, D = kTsmRadius;
    int Hs() const { return N / 2; }
    int seg() const { return (N + kTsmSegs - 1) / kTsmSegs; }
};

inline void tsm_require_speed(double speed) {
    if (!(speed >= kTsmSpeedMin && speed <= kTsmSpeedMax))  // (NaN fails the comparison)
        throw std::invalid_argument("speed must be a finite number in 0.25 .. 4.0");
}
inline void tsm_require_params(const TsmParams& p) {
    if (p.N < 64 || p.N > 2048 || (p.N & 1)) throw std::invalid_argument("fs_tsm_params: frame must be even and in 64 .. 2048");
    if (p.D < 0 || p.D > 1024) throw std::invalid_argument("fs_tsm_params: radius must be in 0 .. 1024");
}

inline int64_t tsm_out_len(int64_t n, double speed) { return n <= 0 ? 0 : (int64_t)std::floor((double)n / speed + 0.5); }
inline int64_t tsm_frames(int64_t out_len, const TsmParams& p) { return (out_len + p.Hs() - 1) / p.Hs(); }
inline int64_t tsm_nominal(int64_t k, double speed, const TsmParams& p) { return (int64_t)std::floor((double)(k * p.Hs()) * speed + 0.5); }

inline std::vector<float> tsm_window(int N) {
    const double pi = 3.14159265358979323846;
    std::vector<float> w((size_t)N);
    for (int i = 0; i < N; ++i) w[(size_t)i] = (float)(0.5 - 0.5 * std::cos(2.0 * pi * (double)i / (double)N));
    return w;
}

inline float tsm_at(const float* x, int64_t n, int64_t a) { return a >= 0 && a < n ? x[a] : 0.f; }

// e[d] of one lag in the documented order; tpos = p_{k-1} + Hs, cpos = q_k + d
inline float tsm_error(const float* x, int64_t n, int64_t tpos, int64_t cpos, const TsmParams& p) {
    const int seg = p.seg();
    float e = 0.f;
    for (int s = 0; s < kTsmSegs; ++s) {
        float a = 0.f;
        const int i1 = std::min(p.N, (s + 1) * seg);
        for (int i = s * seg; i < i1; ++i) {
            volatile float df = tsm_at(x, n, tpos + i) - tsm_at(x, n, cpos + i);  // (volatile: the difference is rounded to f32 before it is squared)
            a = std::fmaf(df, df, a);
        }
        volatile float sum = e + a;  // (s == 0: 0 + a_0 is a_0)
        e = sum;
    }
    return e;
}

// is lag (e1, d1) better than (e0, d0)?  NaN is never better
inline bool tsm_better(float e1, int d1, float e0, int d0) {
    if (e1 < e0) return true;
    if (!(e1 == e0)) return false;
    const int a1 = d1 < 0 ? -d1 : d1, a0 = d0 < 0 ? -d0 : d0;
    return a1 < a0 || (a1 == a0 && d1 < d0);
}

// every p_k of a row, k < tsm_frames(out_len)
inline std::vector<int64_t> tsm_positions(const float* x, int64_t n, double speed, const TsmParams& p) {
    const int64_t K = tsm_frames(tsm_out_len(n, speed), p);
    std::vector<int64_t> pos((size_t)K);
    for (int64_t k = 1; k < K; ++k) {
        const int64_t q = tsm_nominal(k, speed, p), tpos = pos[(size_t)(k - 1)] + p.Hs();
        float be = std::numeric_limits<float>::infinity();
        int bd = 0;
        for (int d = -p.D; d <= p.D; ++d) {
            const float e = tsm_error(x, n, tpos, q + d, p);
            if (tsm_better(e, d, be, bd)) { be = e; bd = d; }
        }
        pos[(size_t)k] = q + bd;
    }
    return pos;
}

// one output sample, given the positions
inline float tsm_sample(const float* x, int64_t n, const int64_t* pos, const float* w, const TsmParams& p, int64_t m) {
    const int64_t k = m / p.Hs(), i = m - k * p.Hs();
    if (k == 0) return tsm_at(x, n, m);
    volatile float a = w[i + p.Hs()] * tsm_at(x, n, pos[k - 1] + p.Hs() + i), b = w[i] * tsm_at(x, n, pos[k] + i);  // (volatile: two roundings)
    return a + b;
}

// the whole definition: y (out_len samples) and, when asked for, the positions
inline std::vector<float> tsm_eval(const float* x, int64_t n, double speed, const TsmParams& p, std::vector<int64_t>* pos_out = nullptr) {
    tsm_require_speed(speed);
    tsm_require_params(p);
    const int64_t ol = tsm_out_len(n, speed);
    const std::vector<int64_t> pos = tsm_positions(x, n, speed, p);
    const std::vector<float> w = tsm_window(p.N);
    std::vector<float> y((size_t)ol);
    for (int64_t m = 0; m < ol; ++m) y[(size_t)m] = tsm_sample(x, n, pos.data(), w.data(), p, m);
    if (pos_out) *pos_out = pos;
    return y;
}

}  // namespace fs
