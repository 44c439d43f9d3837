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
// Streams (fs_codec_streams_open_speed) cut x into chunks: when a frame may be emitted, what is carried from call to call and how much that
// can be is at "streams" below, with an evaluator that runs the definition chunk by chunk.
// Plain C++ -- no HIP in here -- so that a host program can run it under a sanitizer (tools/tsm_plan_check.cpp, tools/tsm_stream_plan_check.cpp).
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

// e[d] of one lag in the documented order; tpos = p_{k-1} + Hs, cpos = q_k + d.  at(a) is x[a]: a whole row (tsm_at) or a stream's window
template <class At>
inline float tsm_error_at(At at, int64_t tpos, int64_t cpos, const TsmParams& p) {
    const int seg = p.seg();
    float e = 0.f;
    for (int s = 0; s < kTsmSegs; ++s) {
        float a = 0.f;
        const int i1 = std::min(p.N, (s + 1) * seg);
        for (int i = s * seg; i < i1; ++i) {
            volatile float df = at(tpos + i) - at(cpos + i);  // (volatile: the difference is rounded to f32 before it is squared)
            a = std::fmaf(df, df, a);
        }
        volatile float sum = e + a;  // (s == 0: 0 + a_0 is a_0)
        e = sum;
    }
    return e;
}
inline float tsm_error(const float* x, int64_t n, int64_t tpos, int64_t cpos, const TsmParams& p) {
    return tsm_error_at([=](int64_t a) { return tsm_at(x, n, a); }, tpos, cpos, p);
}

// is lag (e1, d1) better than (e0, d0)?  NaN is never better
inline bool tsm_better(float e1, int d1, float e0, int d0) {
    if (e1 < e0) return true;
    if (!(e1 == e0)) return false;
    const int a1 = d1 < 0 ? -d1 : d1, a0 = d0 < 0 ? -d0 : d0;
    return a1 < a0 || (a1 == a0 && d1 < d0);
}

// p_k of one frame k >= 1, given p_{k-1} and q_k
template <class At>
inline int64_t tsm_place_at(At at, int64_t pprev, int64_t q, const TsmParams& p) {
    const int64_t tpos = pprev + p.Hs();
    float be = std::numeric_limits<float>::infinity();
    int bd = 0;
    for (int d = -p.D; d <= p.D; ++d) {
        const float e = tsm_error_at(at, tpos, q + d, p);
        if (tsm_better(e, d, be, bd)) { be = e; bd = d; }
    }
    return q + bd;
}

// every p_k of a row, k < tsm_frames(out_len)
inline std::vector<int64_t> tsm_positions(const float* x, int64_t n, double speed, const TsmParams& p) {
    const int64_t K = tsm_frames(tsm_out_len(n, speed), p);
    std::vector<int64_t> pos((size_t)K);
    for (int64_t k = 1; k < K; ++k)
        pos[(size_t)k] = tsm_place_at([=](int64_t a) { return tsm_at(x, n, a); }, pos[(size_t)(k - 1)], tsm_nominal(k, speed, p), p);
    return pos;
}

// output sample i < Hs of frame k, given p_{k-1} and p_k (frame 0: x[i])
template <class At>
inline float tsm_sample_at(At at, int64_t pprev, int64_t pk, const float* w, const TsmParams& p, int64_t k, int64_t i) {
    if (k == 0) return at(i);
    volatile float a = w[i + p.Hs()] * at(pprev + p.Hs() + i), b = w[i] * at(pk + i);  // (volatile: two roundings)
    return a + b;
}
// one output sample, given the positions
inline float tsm_sample(const float* x, int64_t n, const int64_t* pos, const float* w, const TsmParams& p, int64_t m) {
    const int64_t k = m / p.Hs(), i = m - k * p.Hs();
    return tsm_sample_at([=](int64_t a) { return tsm_at(x, n, a); }, k ? pos[k - 1] : 0, pos[k], w, p, k, i);
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

// ---- streams (include/fishrt.h holds the same rule).  The definition above stays the definition; a stream only adds WHEN a frame may be
// emitted, as a function of n, the input samples it has seen so far.  With hi_k = lo_k = 0 for k == 0, else hi_k = q_k + D, lo_k = q_k - D
// (p_k lies in [lo_k, hi_k], and the host does not know where), frame k -- output samples [k Hs, (k + 1) Hs) -- is emittable at n iff
//   (k + 1) Hs <= out_len(n)                       it is a whole frame of whatever the final length turns out to be (out_len grows with n)
//   k == 0:  Hs <= n                               it copies x[0, Hs)
//   k >= 1:  q_k + D + N <= n                      the search region x[q_k - D, q_k + D + N) lies inside the input
//            hi_{k-1} + Hs + N <= n                so does the template x[p_{k-1} + Hs, + N), wherever p_{k-1} was placed
// (the overlap-add reads inside the template and the region).  A call emits the longest prefix of the frames not yet emitted that are
// emittable at its new n.  A final item emits every remaining frame up to K = ceil(out_len(n) / Hs), the last one cut at out_len(n), with x
// zero from n on, as in the one-shot definition; a final item of a stream that never saw a sample emits nothing.
// THE CARRY is the input the frames not yet emitted may still read.  With k the next such frame it starts at
//   c_k = max(0, min(lo_k, lo_{k-1} + Hs))   (k == 0: 0)       the region's and the template's lowest possible index; c_k grows with k
// and ends at n.  ITS BOUND, for any n whatever the chunks were: k is not emittable, so n lies below one of its thresholds.  Write g = Hs *
// speed; q_k lies in (k g - 0.5, k g + 0.5], so q_k - q_{k-1} lies in (g - 1, g + 1).  Measured from q_k the thresholds are
//   out_len:   n < ((k + 1) Hs - 0.5) speed, and that minus q_k is below g + 0.5
//   region:    D + N
//   template:  hi_{k-1} + Hs + N - q_k < D + Hs + N - g + 1
// and q_k - c_k <= max(D, q_k - q_{k-1} + D - Hs) < max(D, g + 1 + D - Hs); frame 0 has c_0 = 0 and n < max(Hs, g).  Hence
//   carry = n - c_k < max(g + 0.5, D + N, D + N + Hs - g + 1) + max(D, g + 1 + D - Hs)
// and tsm_carry_bound rounds both terms up: 4098 samples at the defaults and speed 4.0 (the largest over 0.25 .. 4.0), 2433 at 0.25.  The
// length of a chunk does not enter: what a call leaves behind is a function of n alone, and the chunk itself is read where the caller holds it.
struct TsmBook {  // one stream: input samples seen, frames and output samples emitted, input samples kept for the frames still to come
    int64_t n_in = 0, k_next = 0, n_out = 0, carry_len = 0;
    bool final = false;
};
struct TsmStep {  // what a call that feeds n_new samples does to a book; planning changes nothing
    int64_t in0 = 0, n_total = 0, k0 = 0, k1 = 0, out0 = 0, n_emit = 0, carry_start = 0, carry_len = 0;
};

inline int64_t tsm_hi(int64_t k, double speed, const TsmParams& p) { return k <= 0 ? 0 : tsm_nominal(k, speed, p) + p.D; }
inline int64_t tsm_lo(int64_t k, double speed, const TsmParams& p) { return k <= 0 ? 0 : tsm_nominal(k, speed, p) - p.D; }
inline bool tsm_emittable(int64_t k, int64_t n, double speed, const TsmParams& p) {
    if ((k + 1) * p.Hs() > tsm_out_len(n, speed)) return false;
    if (k == 0) return p.Hs() <= n;
    return tsm_nominal(k, speed, p) + p.D + p.N <= n && tsm_hi(k - 1, speed, p) + p.Hs() + p.N <= n;
}
// first input sample that frame k or a later one may read
inline int64_t tsm_carry_start(int64_t k, double speed, const TsmParams& p) {
    if (k <= 0) return 0;
    return std::max<int64_t>(0, std::min(tsm_lo(k, speed, p), tsm_lo(k - 1, speed, p) + p.Hs()));
}
// samples of one carry row: the bound of carry_len derived above
inline int64_t tsm_carry_bound(const TsmParams& p, double speed) {
    const double g = (double)p.Hs() * speed, DN = (double)(p.D + p.N);
    return (int64_t)std::ceil(std::max({g + 1.0, DN, DN + (double)p.Hs() - g + 1.0})) +
           (int64_t)std::ceil(std::max((double)p.D, g + 1.0 + (double)(p.D - p.Hs())));
}

inline TsmStep tsm_plan_step(const TsmParams& p, double speed, const TsmBook& b, int64_t n_new, bool final) {
    if (b.final) throw std::invalid_argument("time stretch: the stream was already flushed");
    TsmStep s;
    s.in0 = b.n_in; s.n_total = b.n_in + n_new; s.k0 = b.k_next; s.out0 = b.n_out;
    if (final) {
        const int64_t ol = tsm_out_len(s.n_total, speed);  // (>= out0: every emitted frame was a whole frame of out_len(n) at a smaller n)
        s.k1 = std::max(s.k0, tsm_frames(ol, p));
        s.n_emit = std::max<int64_t>(0, ol - s.out0);
        s.carry_start = s.n_total;
    } else {
        s.k1 = s.k0;
        while (tsm_emittable(s.k1, s.n_total, speed, p)) ++s.k1;
        s.n_emit = (s.k1 - s.k0) * p.Hs();
        s.carry_start = std::min(s.n_total, tsm_carry_start(s.k1, speed, p));
    }
    s.carry_len = s.n_total - s.carry_start;
    return s;
}
inline void tsm_commit(TsmBook& b, const TsmStep& s, bool final) {
    b.n_in = s.n_total; b.k_next = s.k1; b.n_out = s.out0 + s.n_emit; b.carry_len = s.carry_len; b.final = final;
}

// The definition chunk by chunk, holding what a stream holds and no more: the book, the carry row and p_{k_next - 1}.  feed() returns the
// samples the call emits and appends the positions of its frames.  A read below the carry's start, or at or beyond n before the final item,
// would be a hole in the rule above: it throws std::logic_error.
class TsmStreamEval {
  public:
    TsmStreamEval(double speed, const TsmParams& p) : speed_(speed), p_(p) {
        tsm_require_speed(speed);
        tsm_require_params(p);
        w_ = tsm_window(p.N);
    }
    const TsmBook& book() const { return book_; }
    std::vector<float> feed(const float* chunk, int64_t n_new, bool final, std::vector<int64_t>* pos_out = nullptr) {
        const TsmStep s = tsm_plan_step(p_, speed_, book_, n_new, final);
        const int64_t c0 = s.in0 - (int64_t)carry_.size();
        const float* carry = carry_.data();
        auto at = [=](int64_t a) -> float {
            if (a < 0) return 0.f;
            if (a >= s.n_total) {
                if (!final) throw std::logic_error("time stretch stream: a frame reads at or beyond n");
                return 0.f;
            }
            if (a >= s.in0) return chunk[a - s.in0];
            if (a < c0) throw std::logic_error("time stretch stream: a frame reads below the carry");
            return carry[a - c0];
        };
        std::vector<float> y((size_t)s.n_emit);
        const int64_t Hs = p_.Hs(), end = s.out0 + s.n_emit;
        for (int64_t k = s.k0; k < s.k1; ++k) {
            const int64_t pk = k == 0 ? 0 : tsm_place_at(at, pprev_, tsm_nominal(k, speed_, p_), p_);
            for (int64_t m = k * Hs; m < std::min((k + 1) * Hs, end); ++m)
                y[(size_t)(m - s.out0)] = tsm_sample_at(at, pprev_, pk, w_.data(), p_, k, m - k * Hs);
            pprev_ = pk;
            if (pos_out) pos_out->push_back(pk);
        }
        std::vector<float> next((size_t)s.carry_len);
        for (int64_t t = 0; t < s.carry_len; ++t) next[(size_t)t] = at(s.carry_start + t);
        carry_.swap(next);
        tsm_commit(book_, s, final);
        return y;
    }

  private:
    double speed_;
    TsmParams p_;
    TsmBook book_;
    std::vector<float> carry_, w_;
    int64_t pprev_ = 0;
};

}  // namespace fs
