// Host check of the sample-rate conversion planner (csrc/fs_resample_plan.h): output lengths, the sinc tap table, the f64 evaluators of both
// definitions and the per-stream book that decides how many samples a chunked stream may emit.
// Small cases: every expected value below is worked out by hand from the definitions in the header's comment, never taken from the planner.
// Tap tables: K, width and the row sums of the six rate pairs the vocoder and the encoder meet.
// A seeded random walk over chunk lengths (empty chunks and the final flush included), in both modes: after every step the emitted count is
// monotone, never exceeds out_len(N) and equals it after the flush; carry_len stays within K + o (1 in linear mode); and the inputs that the
// first and the last output of the step read lie inside (old carry ++ new chunk) -- and, before the flush, below N.
// Meant to run under the sanitizers:
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/resample_plan_check.cpp -o resample_plan_check && ./resample_plan_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <stdexcept>
#include <vector>

#include "../fish-speech.rs_amd/csrc/fs_resample_plan.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "resample_plan_check: %s failed at line %d\n", #c, __LINE__); std::exit(1); } } while (0)

using namespace fs;

static void small_cases() {
    // linear 2 -> 1 Hz: ratio 0.5, n = 5 -> ceil(2.5) = 3 outputs at idx 0, 2, 4 (t = 0: the samples themselves)
    {
        const ResampleRates r = resample_rates(2, 1);
        const float x[5] = {1.f, 2.f, 3.f, 4.f, 5.f};
        CHECK(resample_out_len(r, kResampleLinear, 5) == 3);
        CHECK(resample_linear_eval(x, 5, r, 0) == 1.f && resample_linear_eval(x, 5, r, 1) == 3.f && resample_linear_eval(x, 5, r, 2) == 5.f);
    }
    // linear 1 -> 2 Hz: ratio 2, n = 3 -> 6 outputs; idx 0.5 is the mean of x0, x1; idx 2.5 has c clamped to n - 1 = 2: x2 / 2 + x2 / 2
    {
        const ResampleRates r = resample_rates(1, 2);
        const float x[3] = {1.f, 2.f, 4.f};
        CHECK(resample_out_len(r, kResampleLinear, 3) == 6);
        const float e[6] = {1.f, 1.5f, 2.f, 3.f, 4.f, 4.f};
        for (int i = 0; i < 6; ++i) CHECK(resample_linear_eval(x, 3, r, i) == e[i]);
        // streaming: output i is ready when ceil(i / 2) <= N - 1: N = 1 -> {0}; N = 2 -> {0, 1, 2}; flush of N = 3 -> 6
        CHECK(resample_emittable(r, kResampleLinear, 0, false) == 0 && resample_emittable(r, kResampleLinear, 1, false) == 1);
        CHECK(resample_emittable(r, kResampleLinear, 2, false) == 3 && resample_emittable(r, kResampleLinear, 3, false) == 5);
        CHECK(resample_emittable(r, kResampleLinear, 3, true) == 6);
    }
    // equal rates, linear: the identity
    {
        const ResampleRates r = resample_rates(44100, 44100);
        const float x[3] = {0.25f, -1.5f, 3.f};
        CHECK(resample_out_len(r, kResampleLinear, 3) == 3);
        for (int i = 0; i < 3; ++i) CHECK(resample_linear_eval(x, 3, r, i) == x[i]);
    }
    // sinc lengths: 44.1 -> 24 kHz is 147 -> 80: n = 147 -> 80, n = 148 -> ceil(80 * 148 / 147) = 81, n = 1 -> 1, n = 0 -> 0
    {
        const ResampleRates r = resample_rates(44100, 24000);
        CHECK(r.o == 147 && r.p == 80 && r.width == 12 && r.K == 171);
        CHECK(resample_out_len(r, kResampleSinc, 147) == 80 && resample_out_len(r, kResampleSinc, 148) == 81);
        CHECK(resample_out_len(r, kResampleSinc, 1) == 1 && resample_out_len(r, kResampleSinc, 0) == 0);
        // a whole block m needs inputs up to m * 147 + 12 + 147 - 1: N = 158 -> none, N = 159 -> block 0 (80), N = 306 -> blocks 0, 1 (160)
        CHECK(resample_emittable(r, kResampleSinc, 158, false) == 0 && resample_emittable(r, kResampleSinc, 159, false) == 80);
        CHECK(resample_emittable(r, kResampleSinc, 305, false) == 80 && resample_emittable(r, kResampleSinc, 306, false) == 160);
        CHECK(resample_emittable(r, kResampleSinc, 158, true) == 86);  // ceil(80 * 158 / 147) = ceil(85.98)
    }
    // sinc at equal rates: o = p = 1, base 0.99, width = ceil(6 / 0.99) = 7, K = 15.  A unit impulse at index 3 of 8 comes out as the taps
    // mirrored around it: out[3 + d] = h(t = -0.99 d) = sinc(0.99 d) cos^2(pi 0.99 d / 12) 0.99
    {
        const ResampleRates r = resample_rates(16000, 16000);
        CHECK(r.o == 1 && r.p == 1 && r.width == 7 && r.K == 15);
        float x[8] = {0, 0, 0, 1.f, 0, 0, 0, 0};
        const double pi = 3.14159265358979323846;
        for (int i = 0; i < 8; ++i) {
            const double t = 0.99 * (double)(i - 3);
            const double e = (t == 0.0 ? 1.0 : std::sin(pi * t) / (pi * t)) * std::pow(std::cos(pi * t / 12.0), 2) * 0.99;
            CHECK(std::fabs(resample_sinc_eval(x, 8, r, i) - e) < 1e-15);
        }
        CHECK(std::fabs(resample_sinc_eval(x, 8, r, 3) - 0.99) < 1e-15);
    }
    // the oversize pair is refused, and the message names it
    {
        const ResampleRates r = resample_rates(44100, 44101);
        CHECK(!resample_table_fits(r));
        bool threw = false;
        try { (void)resample_taps(r); } catch (const std::invalid_argument& e) {
            threw = std::string(e.what()).find("44100 -> 44101") != std::string::npos;
        }
        CHECK(threw);
    }
}

static void tables() {
    const int pairs[6][4] = {{44100, 24000, 80, 171}, {44100, 48000, 160, 161}, {44100, 16000, 160, 475},
                             {22050, 44100, 2, 15},   {48000, 44100, 147, 174}, {8000, 44100, 441, 94}};
    for (const auto& q : pairs) {
        const ResampleRates r = resample_rates(q[0], q[1]);
        CHECK(r.p == q[2] && r.K == q[3] && r.K == 2 * r.width + r.o);
        CHECK(r.width == (int64_t)std::ceil(6.0 * (double)r.o / ((double)std::min(r.o, r.p) * 0.99)));
        const std::vector<float> h = resample_taps(r);
        CHECK((int64_t)h.size() == r.p * r.K);
        // every phase passes DC at unit gain up to the ripple of a 6-crossing Hann window (a few 1e-3); a wrong scale or phase step is off by far more
        double worst = 0.0;
        for (int64_t j = 0; j < r.p; ++j) {
            double s = 0.0;
            for (int64_t k = 0; k < r.K; ++k) {
                s += (double)h[(size_t)(j * r.K + k)];
                CHECK((float)resample_tap_f64(r, j, k) == h[(size_t)(j * r.K + k)]);
            }
            worst = std::max(worst, std::fabs(s - 1.0));
        }
        std::printf("taps %d -> %d: %lld x %lld, width %lld, max |row sum - 1| %.3g\n", q[0], q[1], (long long)r.p, (long long)r.K,
                    (long long)r.width, worst);
        CHECK(worst < 1e-2);
    }
}

static void walk() {
    const int pairs[8][2] = {{44100, 24000}, {44100, 48000}, {44100, 16000}, {22050, 44100}, {48000, 44100}, {8000, 44100}, {44100, 44100}, {7, 3}};
    std::mt19937_64 rng(0x5EED5A3Bull);
    long long steps = 0;
    for (const auto& q : pairs)
        for (int mode = 0; mode < 2; ++mode)
            for (int rep = 0; rep < 40; ++rep) {
                const ResampleRates r = resample_rates(q[0], q[1]);
                ResampleBook b;
                const int n_chunks = 1 + (int)(rng() % 30);
                for (int c = 0; c < n_chunks; ++c) {
                    const bool final = c == n_chunks - 1;
                    const int kind = (int)(rng() % 4);
                    const int64_t n_new = kind == 0 ? (int64_t)(rng() % 3) : kind == 1 ? (int64_t)(rng() % 200) : (int64_t)(rng() % 5000);
                    const ResampleStep s = resample_plan_step(r, mode, b, n_new, final);
                    const int64_t N = s.n_total;
                    CHECK(s.in0 == b.n_in && s.out0 == b.n_out && N == b.n_in + n_new);
                    CHECK(s.n_emit >= 0);
                    CHECK(s.out0 + s.n_emit <= resample_out_len(r, mode, N));
                    if (final) CHECK(s.out0 + s.n_emit == resample_out_len(r, mode, N) && s.carry_len == 0);
                    CHECK(s.carry_len >= 0 && s.carry_len <= resample_carry_cap(r, mode) && s.carry_len <= N);
                    if (mode == kResampleLinear) CHECK(s.carry_len <= 1);
                    else CHECK(s.carry_len < r.K + r.o);
                    // the new carry is a suffix of (old carry ++ chunk)
                    if (!final) CHECK(N - s.carry_len >= b.n_in - b.carry_len);
                    // the inputs the step's outputs read
                    for (int e = 0; e < 2 && s.n_emit > 0; ++e) {
                        const int64_t i = e == 0 ? s.out0 : s.out0 + s.n_emit - 1;
                        int64_t lo, hi;
                        if (mode == kResampleLinear) {
                            const double idx = (double)i / r.ratio;
                            lo = (int64_t)std::floor(idx); hi = (int64_t)std::ceil(idx);
                        } else {
                            lo = (i / r.p) * r.o - r.width; hi = (i / r.p) * r.o + r.K - 1 - r.width;
                        }
                        CHECK(std::max<int64_t>(lo, 0) >= b.n_in - b.carry_len);
                        if (!final) CHECK(hi <= N - 1);
                    }
                    // and the first output NOT emitted is not ready yet (the count is the largest the rule allows)
                    if (!final) {
                        const int64_t i = s.out0 + s.n_emit;
                        if (mode == kResampleLinear) CHECK(!resample_linear_ready(r, i, N) || i >= resample_out_len(r, mode, N));
                        else CHECK((i / r.p) * r.o + r.width + r.o - 1 > N - 1 && i % r.p == 0);
                    }
                    resample_commit(b, s, final);
                    ++steps;
                }
                bool threw = false;
                try { (void)resample_plan_step(r, mode, b, 1, false); } catch (const std::invalid_argument&) { threw = true; }
                CHECK(threw);
            }
    std::printf("random walk: %lld steps\n", steps);
}

int main() {
    small_cases();
    tables();
    walk();
    std::printf("resample_plan_check ok\n");
    return 0;
}
