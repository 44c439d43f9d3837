// Host check of the time-stretch planner and evaluator (csrc/fs_tsm_plan.h): output lengths, frame counts and nominal positions, parameter and
// speed validation, the window table, the tie rule, the documented order of one lag's error sum, and whole chains whose positions can be
// worked out by hand: speed 1 (p_k = k Hs), digital silence (d = 0), and signals that repeat bit for bit, where the lags a period apart tie
// exactly and the rule (smallest |d|, of +-d the negative) decides.
// Every expected value below is worked out by hand from the definition in the header's comment, never taken from the evaluator.
// Meant to run under the sanitizers:
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/tsm_plan_check.cpp -o tsm_plan_check && ./tsm_plan_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <stdexcept>
#include <vector>

#include "../fish-speech.rs_amd/csrc/fs_tsm_plan.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "tsm_plan_check: %s failed at line %d\n", #c, __LINE__); std::exit(1); } } while (0)

using namespace fs;

template <class F>
static bool throws(F f) {
    try { f(); } catch (const std::invalid_argument&) { return true; }
    return false;
}

static void lengths() {
    const TsmParams p;  // N = 1024, Hs = 512, D = 512
    CHECK(p.Hs() == 512 && p.seg() == 171);
    // n = 0: nothing, at any speed
    CHECK(tsm_out_len(0, 1.25) == 0 && tsm_frames(0, p) == 0);
    // n < Hs: 100 / 0.5 = 200 samples, one frame; 300 / 2 = 150, one frame
    CHECK(tsm_out_len(100, 0.5) == 200 && tsm_frames(200, p) == 1);
    CHECK(tsm_out_len(300, 2.0) == 150 && tsm_frames(150, p) == 1);
    // out_len an exact multiple of Hs: 1280 / 1.25 = 1024 = 2 Hs -> 2 frames; one more input sample: 1024.8 + 0.5 -> 1025 -> 3 frames
    CHECK(tsm_out_len(1280, 1.25) == 1024 && tsm_frames(1024, p) == 2);
    CHECK(tsm_out_len(1281, 1.25) == 1025 && tsm_frames(1025, p) == 3);
    CHECK(tsm_nominal(1, 1.25, p) == 640 && tsm_nominal(2, 1.25, p) == 1280);
    // 1000 / 0.77 = 1298.70 -> 1299, 3 frames; q_1 = floor(394.24 + 0.5) = 394, q_2 = floor(788.48 + 0.5) = 788
    CHECK(tsm_out_len(1000, 0.77) == 1299 && tsm_frames(1299, p) == 3);
    CHECK(tsm_nominal(1, 0.77, p) == 394 && tsm_nominal(2, 0.77, p) == 788);
    // halves round up: 10 / 4 + 0.5 = 3.0 -> 3; 2 / 4 + 0.5 = 1.0 -> 1; 1 / 4 + 0.5 = 0.75 -> 0
    CHECK(tsm_out_len(10, 4.0) == 3 && tsm_out_len(2, 4.0) == 1 && tsm_out_len(1, 4.0) == 0);
    // speed 3: 4608 / 3 = 1536 = 3 Hs -> 3 frames, q_1 = 1536
    CHECK(tsm_out_len(4608, 3.0) == 1536 && tsm_frames(1536, p) == 3 && tsm_nominal(1, 3.0, p) == 1536);
    // other parameters: N = 256 (Hs 128): 1000 / 2 = 500 -> 4 frames, q_3 = 768
    TsmParams s;
    s.N = 256; s.D = 64;
    CHECK(tsm_frames(tsm_out_len(1000, 2.0), s) == 4 && tsm_nominal(3, 2.0, s) == 768 && s.seg() == 43);
}

static void validation() {
    for (double v : {0.25, 1.0, 4.0}) CHECK(!throws([&] { tsm_require_speed(v); }));
    for (double v : {0.0, 0.2499, 4.0001, -1.0, std::numeric_limits<double>::infinity(), std::nan("")}) CHECK(throws([&] { tsm_require_speed(v); }));
    const int good[4][2] = {{64, 0}, {2048, 1024}, {1024, 512}, {66, 1}}, bad[5][2] = {{62, 0}, {2050, 0}, {65, 0}, {1024, -1}, {1024, 1025}};
    for (const auto& g : good) { TsmParams p; p.N = g[0]; p.D = g[1]; CHECK(!throws([&] { tsm_require_params(p); })); }
    for (const auto& b : bad) { TsmParams p; p.N = b[0]; p.D = b[1]; CHECK(throws([&] { tsm_require_params(p); })); }
}

static void window() {
    for (int N : {64, 256, 1024, 2048}) {
        const std::vector<float> w = tsm_window(N);
        CHECK((int)w.size() == N && w[0] == 0.f && w[(size_t)N / 2] == 1.f && w[(size_t)N / 4] == 0.5f && w[(size_t)(3 * N / 4)] == 0.5f);
        for (int i = 1; i < N; ++i) CHECK(std::fabs(w[(size_t)i] - w[(size_t)(N - i)]) <= 6e-8f);
        for (int i = 0; i < N / 2; ++i) CHECK(std::fabs(w[(size_t)i] + w[(size_t)(i + N / 2)] - 1.f) <= 1.2e-7f);  // the two halves overlap-add to 1
    }
}

static void tie_rule() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::nanf("");
    CHECK(tsm_better(1.f, 5, 2.f, 0) && !tsm_better(2.f, 0, 1.f, 5));  // the smaller error, whatever the lags
    CHECK(tsm_better(1.f, -2, 1.f, 3) && !tsm_better(1.f, 3, 1.f, -2));  // equal errors: the smaller |d|
    CHECK(tsm_better(1.f, -3, 1.f, 3) && !tsm_better(1.f, 3, 1.f, -3));  // of +-d the negative
    CHECK(!tsm_better(1.f, 3, 1.f, 3));
    CHECK(!tsm_better(nan, 0, inf, 0) && !tsm_better(nan, 0, 1.f, 7) && !tsm_better(inf, 1, inf, 0) && tsm_better(3.f, 9, inf, 0));
}

// one lag's error, written again from the header's text: six segments of ceil(N / 6), each an ascending fmaf chain, five additions
static float error_by_the_text(const std::vector<float>& x, long long tpos, long long cpos, int N) {
    auto at = [&](long long a) { return a >= 0 && a < (long long)x.size() ? x[(size_t)a] : 0.f; };
    const int seg = (N + 5) / 6;
    float a[6];
    for (int s = 0; s < 6; ++s) {
        a[s] = 0.f;
        for (int i = s * seg; i < N && i < (s + 1) * seg; ++i) {
            volatile float df = at(tpos + i) - at(cpos + i);
            a[s] = std::fmaf(df, df, a[s]);
        }
    }
    volatile float e = a[0] + a[1];
    for (int s = 2; s < 6; ++s) e = e + a[s];
    return e;
}

static void error_order() {
    std::mt19937 rng(7);
    std::uniform_real_distribution<float> u(-1.f, 1.f);
    std::vector<float> x(600);
    for (auto& v : x) v = u(rng);
    int differs = 0;
    for (int N : {64, 66, 256, 1024}) {
        TsmParams p;
        p.N = N;
        for (long long c : {-40ll, 0ll, 3ll, 77ll, 500ll}) {
            const float e = tsm_error(x.data(), (long long)x.size(), 10, c, p);
            CHECK(e == error_by_the_text(x, 10, c, N));
            float plain = 0.f;  // one ascending chain: another order, another last bit somewhere
            for (int i = 0; i < N; ++i) {
                const float df = tsm_at(x.data(), 600, 10 + i) - tsm_at(x.data(), 600, c + i);
                plain = std::fmaf(df, df, plain);
            }
            differs += plain != e;
        }
    }
    CHECK(differs > 0);
}

static void chains() {
    std::mt19937 rng(11);
    std::uniform_real_distribution<float> u(-1.f, 1.f);
    // speed 1: e[0] is exactly 0 in every frame, so p_k = k Hs, and the output is the input up to the rounding of the two products
    {
        TsmParams p;
        p.N = 64; p.D = 8;
        std::vector<float> x(500);
        for (auto& v : x) v = u(rng);
        std::vector<int64_t> pos;
        const std::vector<float> y = tsm_eval(x.data(), 500, 1.0, p, &pos);
        CHECK(y.size() == 500 && pos.size() == 16);
        for (size_t k = 0; k < pos.size(); ++k) CHECK(pos[k] == (int64_t)k * 32);
        // w[0] = 0, w[32] = 1: y[32] = 1 * x[32] + 0 * x[32];  w[16] = w[48] = 0.5: y[48] = x[48] / 2 + x[48] / 2
        CHECK(y[0] == x[0] && y[31] == x[31] && y[32] == x[32] && y[48] == x[48] && y[64 + 16] == x[64 + 16]);
        for (size_t m = 0; m < 500; ++m) CHECK(std::fabs(y[m] - x[m]) <= 2.4e-7f * std::fabs(x[m]));
    }
    // digital silence: every error is 0, the tie rule picks d = 0, p_k = q_k
    {
        const TsmParams p;
        std::vector<float> x(3000, 0.f);
        const std::vector<int64_t> pos = tsm_positions(x.data(), 3000, 1.25, p);
        CHECK(pos.size() == 5);  // 2400 samples
        for (size_t k = 1; k < pos.size(); ++k) CHECK(pos[k] == tsm_nominal((int64_t)k, 1.25, p));
    }
    // period 7, N = 64 (Hs 32), D = 8, speed 1.25: the lags with q_k + d = p_{k-1} + 32 (mod 7) have e = 0 exactly.
    //   k = 1: q = 40, template at 32: d = -8 (mod 7) -> {-8, -1, 6} -> -1, p_1 = 39
    //   k = 2: q = 80, template at 71: d = -9 (mod 7) -> {-2, 5} -> -2, p_2 = 78
    //   k = 3: q = 120, template at 110: d = -10 (mod 7) -> {-3, 4} -> -3, p_3 = 117
    {
        TsmParams p;
        p.N = 64; p.D = 8;
        float pat[7];
        for (auto& v : pat) v = u(rng);
        std::vector<float> x(400);
        for (size_t a = 0; a < x.size(); ++a) x[a] = pat[a % 7];
        const std::vector<int64_t> pos = tsm_positions(x.data(), 400, 1.25, p);
        CHECK(pos.size() == 10 && pos[0] == 0 && pos[1] == 39 && pos[2] == 78 && pos[3] == 117);
    }
    // period 8, same frame, speed 1.125: q_1 = 36, template at 32: d = -4 (mod 8) -> {-4, 4}: the negative one, p_1 = 32
    {
        TsmParams p;
        p.N = 64; p.D = 8;
        float pat[8];
        for (auto& v : pat) v = u(rng);
        std::vector<float> x(400);
        for (size_t a = 0; a < x.size(); ++a) x[a] = pat[a % 8];
        const std::vector<int64_t> pos = tsm_positions(x.data(), 400, 1.125, p);
        CHECK(pos.size() >= 2 && pos[1] == 32);
    }
    // D = 0: no search, p_k = q_k on any signal;  n < Hs stretched: the row, then zeros
    {
        TsmParams p;
        p.N = 64; p.D = 0;
        std::vector<float> x(300);
        for (auto& v : x) v = u(rng);
        const std::vector<int64_t> pos = tsm_positions(x.data(), 300, 2.0, p);
        CHECK(pos.size() == 5);
        for (size_t k = 0; k < pos.size(); ++k) CHECK(pos[k] == (int64_t)k * 64);
        const TsmParams d;
        const std::vector<float> y = tsm_eval(x.data(), 100, 0.5, d);
        CHECK(y.size() == 200);
        for (size_t m = 0; m < 200; ++m) CHECK(y[m] == (m < 100 ? x[m] : 0.f));
        CHECK(tsm_eval(x.data(), 0, 0.5, d).empty());
    }
}

int main() {
    lengths();
    validation();
    window();
    tie_rule();
    error_order();
    chains();
    std::printf("tsm_plan_check ok\n");
    return 0;
}
