// Loudness normalisation of PCM (the `loudness` of a request), the host side: the K-weighting coefficients, hop and block counting, parameter
// checks, the transition-matrix tables the kernels combine chunk states with, and a plain serial f64 evaluator of the whole definition.  The
// kernels (codec_loud.hip) compute; this header counts and launches nothing.
//
// Integrated loudness of ITU-R BS.1770-4, one channel, any integer rate fs in 8000 .. 48000 (include/fishrt.h holds the same text):
//   K-weighting: two biquads in cascade, coefficients in f64 from the analogue prototypes (the libebur128 construction; it reproduces the
//   standard's 48 kHz table).  K = tan(pi f0 / fs), a0 = 1 + K/Q + K^2 for either stage.
//     shelf:     f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196, Vh = 10^(G/20), Vb = Vh^0.4996667741545416
//                b = [(Vh + Vb K/Q + K^2)/a0, 2 (K^2 - Vh)/a0, (Vh - Vb K/Q + K^2)/a0],  a = [1, 2 (K^2 - 1)/a0, (1 - K/Q + K^2)/a0]
//     high-pass: f0 = 38.13547087602444, Q = 0.5003270373238773;  b = [1, -2, 1],  a = [1, 2 (K^2 - 1)/a0, (1 - K/Q + K^2)/a0]
//   Filter: x is f32 widened to f64, zero before sample 0; both stages in f64 from zero state, each in transposed direct form II:
//       y = b0 x + s0;  s0 = b1 x - a1 y + s1;  s1 = b2 x - a2 y        (shelf, state s0 s1)
//       z = y + s2;     s2 = -2 y - d1 z + s3;  s3 = y - d2 z           (high-pass, a = [1, d1, d2], state s2 s3)
//     (an implementation may contract a product and a sum into one fma; the results are held to a derived bound, not to bits)
//   Hop h = (fs + 5) / 10 (integer);  s_i = sum of z^2 over [i h, (i + 1) h), i < nb = n / h whole hops
//   Block j < nb - 3:  m_j = (s_j + s_{j+1} + s_{j+2} + s_{j+3}) / (4 h),  l_j = -0.691 + 10 log10(m_j)
//   Absolute gate: keep l_j > -70.  Relative gate: G = -0.691 + 10 log10(mean of the kept m_j) - 10; keep l_j > -70 and l_j > G.
//   L = -0.691 + 10 log10(mean of those m_j).  A comparison with a NaN is false.  nb < 4 or no block kept: L = -inf, gain exactly 1.
//   Peak: the largest |x| of the row in f32, NaN ignored.
//   Gain: g_L = 10^((target - L) / 20) in f64;  g = min(g_L, 10^(max_gain_db / 20), 10^(peak_db / 20) / peak), the last only when peak > 0;
//         rounded once to f32.  Output y[i] = x[i] * g, one f32 multiply.
// The recurrence is linear: with A the 4 x 4 transition matrix of the cascade (state s0 .. s3, zero input), the state after c samples is
// A^c s_in + (the state the same samples leave from zero state).  The kernels filter chunks of kLoudChunk samples from zero state and combine
// the chunk states with powers of M = A^kLoudChunk (LoudTables below), then filter every chunk again from its true entry state.
// Plain C++ -- no HIP in here -- so that a host program can run it under a sanitizer (tools/loud_plan_check.cpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <vector>

namespace fs {

constexpr int kLoudRateMin = 8000, kLoudRateMax = 48000;
constexpr int kLoudChunk = 32;                      // samples one lane filters: the longest dependent chain of the filter
constexpr int kLoudWg = 256;                        // lanes of a workgroup
constexpr int kLoudSpan = kLoudChunk * kLoudWg;     // samples of a workgroup
constexpr int kLoudScanSteps = 8;                   // log2(kLoudWg)
constexpr int64_t kLoudMaxSamples = (int64_t)1 << 30;  // per row (a day at 8 kHz, six hours at 48 kHz); keeps a row's indices in 32 bits
constexpr double kLoudPeakDbDefault = -1.0, kLoudMaxGainDbDefault = 30.0;

struct LoudParams {  // fs_loud_params
    double target_lufs = -18.0, peak_db = kLoudPeakDbDefault, max_gain_db = kLoudMaxGainDbDefault;
};
struct LoudResult {  // fs_loud_result
    double lufs = -std::numeric_limits<double>::infinity();
    float peak = 0.f, gain = 1.f;
    int32_t blocks_total = 0, blocks_kept = 0;
};

inline void loud_require_rate(int rate) {
    if (rate < kLoudRateMin || rate > kLoudRateMax) throw std::invalid_argument("loudness: the rate must be in 8000 .. 48000");
}
inline void loud_require_params(const LoudParams& p) {  // (a NaN fails every comparison)
    if (!(p.target_lufs >= -40.0 && p.target_lufs <= -5.0)) throw std::invalid_argument("fs_loud_params: target_lufs must be in -40 .. -5");
    if (!(p.peak_db <= 0.0 && std::isfinite(p.peak_db))) throw std::invalid_argument("fs_loud_params: peak_db must be a finite number <= 0");
    if (!(p.max_gain_db >= 0.0 && p.max_gain_db <= 60.0)) throw std::invalid_argument("fs_loud_params: max_gain_db must be in 0 .. 60");
}

struct LoudCoefs {
    double b0, b1, b2, a1, a2;  // shelf
    double d1, d2;              // high-pass denominator (its numerator is 1, -2, 1)
};
inline LoudCoefs loud_coefs(int rate) {
    const double pi = 3.14159265358979323846, fs = (double)rate;
    LoudCoefs c;
    {
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = std::tan(pi * f0 / fs), Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        c.b0 = (Vh + Vb * K / Q + K * K) / a0;
        c.b1 = 2.0 * (K * K - Vh) / a0;
        c.b2 = (Vh - Vb * K / Q + K * K) / a0;
        c.a1 = 2.0 * (K * K - 1.0) / a0;
        c.a2 = (1.0 - K / Q + K * K) / a0;
    }
    {
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = std::tan(pi * f0 / fs), a0 = 1.0 + K / Q + K * K;
        c.d1 = 2.0 * (K * K - 1.0) / a0;
        c.d2 = (1.0 - K / Q + K * K) / a0;
    }
    return c;
}

inline int loud_hop(int rate) { return (rate + 5) / 10; }
inline int64_t loud_hops(int64_t n, int rate) { return n <= 0 ? 0 : n / loud_hop(rate); }
inline int64_t loud_blocks(int64_t n, int rate) { return std::max<int64_t>(loud_hops(n, rate) - 3, 0); }

// one sample through the cascade; s = {s0, s1, s2, s3}
inline double loud_step(const LoudCoefs& c, double x, double* s) {
    const double y = c.b0 * x + s[0];
    s[0] = c.b1 * x - c.a1 * y + s[1];
    s[1] = c.b2 * x - c.a2 * y;
    const double z = y + s[2];
    s[2] = -2.0 * y - c.d1 * z + s[3];
    s[3] = y - c.d2 * z;
    return z;
}

// ---- the chunk tables: 4 x 4 row-major matrices.  The powers are formed in long double (a 64-bit significand on x86-64) and rounded to f64
// once, when they are stored: up to 255 products in a row would otherwise leave an entry several hundred ulps off (tests/loud_refs.py (3))
struct LoudMat {
    long double m[16];
};
inline LoudMat loud_mat_identity() {
    LoudMat r{};
    for (int i = 0; i < 4; ++i) r.m[i * 4 + i] = 1.0L;
    return r;
}
inline LoudMat loud_mat_mul(const LoudMat& a, const LoudMat& b) {
    LoudMat r{};
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            long double t = 0.0L;
            for (int k = 0; k < 4; ++k) t += a.m[i * 4 + k] * b.m[k * 4 + j];
            r.m[i * 4 + j] = t;
        }
    return r;
}
// A: the state after one sample of zero input (loud_step with x = 0)
inline LoudMat loud_transition(const LoudCoefs& c) {
    LoudMat a{};
    a.m[0] = -(long double)c.a1;         a.m[1] = 1.0L;
    a.m[4] = -(long double)c.a2;
    a.m[8] = -2.0L - (long double)c.d1;  a.m[10] = -(long double)c.d1;  a.m[11] = 1.0L;
    a.m[12] = 1.0L - (long double)c.d2;  a.m[14] = -(long double)c.d2;
    return a;
}
// what the kernels read, as one array of doubles: the coefficients (8 slots), P[k] = M^(2^k) for k = 0 .. kLoudScanSteps (P[8] = M^256 carries
// a state across one workgroup), and Lane[l] = M^l for l < kLoudWg (a workgroup's entry state carried to lane l's chunk)
constexpr size_t kLoudTabCoef = 0, kLoudTabP = 8, kLoudTabLane = kLoudTabP + 16 * (kLoudScanSteps + 1),
                 kLoudTabDoubles = kLoudTabLane + 16 * (size_t)kLoudWg;
inline std::vector<double> loud_tables(int rate) {
    const LoudCoefs c = loud_coefs(rate);
    std::vector<double> t(kLoudTabDoubles, 0.0);
    const double cs[8] = {c.b0, c.b1, c.b2, c.a1, c.a2, c.d1, c.d2, 0.0};
    std::copy(cs, cs + 8, t.begin() + kLoudTabCoef);
    LoudMat M = loud_transition(c);
    for (int i = 0; i < 5; ++i) M = loud_mat_mul(M, M);  // A^32
    static_assert(kLoudChunk == 32, "M = A^(2^5)");
    LoudMat P = M;
    for (int k = 0; k <= kLoudScanSteps; ++k) {
        for (int e = 0; e < 16; ++e) t[kLoudTabP + 16 * (size_t)k + (size_t)e] = (double)P.m[e];
        P = loud_mat_mul(P, P);
    }
    LoudMat L = loud_mat_identity();
    for (int l = 0; l < kLoudWg; ++l) {
        for (int e = 0; e < 16; ++e) t[kLoudTabLane + 16 * (size_t)l + (size_t)e] = (double)L.m[e];
        L = loud_mat_mul(M, L);
    }
    return t;
}

// ---- the definition, walked serially in f64.  hops (nullable) receives s_0 .. s_{nb-1}
inline double loud_lufs_of(double mean_square) { return -0.691 + 10.0 * std::log10(mean_square); }

inline LoudResult loud_gate(const double* s, int64_t nb, int h) {
    LoudResult r;
    if (nb < 4) return r;
    const int64_t nblk = nb - 3;
    r.blocks_total = (int32_t)std::min<int64_t>(nblk, std::numeric_limits<int32_t>::max());
    std::vector<double> m((size_t)nblk), l((size_t)nblk);
    for (int64_t j = 0; j < nblk; ++j) {
        m[(size_t)j] = (s[j] + s[j + 1] + s[j + 2] + s[j + 3]) / (4.0 * (double)h);
        l[(size_t)j] = loud_lufs_of(m[(size_t)j]);
    }
    double sum = 0.0;
    int64_t kept = 0;
    for (int64_t j = 0; j < nblk; ++j)
        if (l[(size_t)j] > -70.0) { sum += m[(size_t)j]; ++kept; }
    if (!kept) return r;
    const double gamma = loud_lufs_of(sum / (double)kept) - 10.0;
    sum = 0.0; kept = 0;
    for (int64_t j = 0; j < nblk; ++j)
        if (l[(size_t)j] > -70.0 && l[(size_t)j] > gamma) { sum += m[(size_t)j]; ++kept; }
    if (!kept) return r;
    r.blocks_kept = (int32_t)std::min<int64_t>(kept, std::numeric_limits<int32_t>::max());
    r.lufs = loud_lufs_of(sum / (double)kept);
    return r;
}

inline float loud_gain(double lufs, float peak, const LoudParams& p) {
    if (!(lufs > -std::numeric_limits<double>::infinity())) return 1.f;  // no loudness (a NaN L cannot arise: a NaN block is never kept)
    double g = std::pow(10.0, (p.target_lufs - lufs) / 20.0);
    g = std::min(g, std::pow(10.0, p.max_gain_db / 20.0));
    if (peak > 0.f) g = std::min(g, std::pow(10.0, p.peak_db / 20.0) / (double)peak);
    return (float)g;
}

inline float loud_peak(const float* x, int64_t n) {
    float pk = 0.f;
    for (int64_t i = 0; i < n; ++i) {
        const float a = std::fabs(x[i]);
        if (a > pk) pk = a;  // (false for a NaN)
    }
    return pk;
}

// params null: measure only (gain stays 1)
inline LoudResult loud_measure(const float* x, int64_t n, int rate, const LoudParams* p, std::vector<double>* hops = nullptr) {
    loud_require_rate(rate);
    if (p) loud_require_params(*p);
    if (n < 0 || n > kLoudMaxSamples) throw std::invalid_argument("loudness: a row's length must be in 0 .. 2^30");
    const LoudCoefs c = loud_coefs(rate);
    const int h = loud_hop(rate);
    const int64_t nb = loud_hops(n, rate);
    std::vector<double> s((size_t)nb, 0.0);
    double st[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t i = 0; i < nb * h; ++i) {
        const double z = loud_step(c, (double)x[i], st);
        s[(size_t)(i / h)] += z * z;
    }
    LoudResult r = loud_gate(s.data(), nb, h);
    r.peak = loud_peak(x, n);
    if (p) r.gain = loud_gain(r.lufs, r.peak, *p);
    if (hops) *hops = std::move(s);
    return r;
}

}  // namespace fs
