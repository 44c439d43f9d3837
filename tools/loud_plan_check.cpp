// Host check of the loudness planner and evaluator (csrc/fs_loud_plan.h): the K-weighting coefficients against the 48 kHz table of ITU-R
// BS.1770, hop and block counts at the edges of the rate range, rate and parameter validation, the rows without loudness (too short, digital
// silence, everything under the absolute gate, a NaN in every block), both gates on block energies chosen by hand, the three clauses of the
// gain, and the chunk tables: a row evaluated the way the kernels do it (chunks of 32 from zero state, the states combined with the stored
// powers, every chunk filtered again from its entry state) against the serial walk.
// Expected values are worked out from the definition in the header's comment, never taken from the evaluator.
// Meant to run under the sanitizers:
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/loud_plan_check.cpp -o loud_plan_check && ./loud_plan_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <stdexcept>
#include <vector>

#include "../fish-speech.rs_amd/csrc/fs_loud_plan.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "loud_plan_check: %s failed at line %d\n", #c, __LINE__); std::exit(1); } } while (0)

using namespace fs;

template <class F>
static bool throws(F f) {
    try { f(); } catch (const std::invalid_argument&) { return true; }
    return false;
}
static bool near(double a, double b, double tol) { return std::fabs(a - b) <= tol; }

static void coefficients() {
    const LoudCoefs c = loud_coefs(48000);  // the standard's table
    CHECK(near(c.b0, 1.53512485958697, 1e-12) && near(c.b1, -2.69169618940638, 1e-12) && near(c.b2, 1.19839281085285, 1e-12));
    CHECK(near(c.a1, -1.69065929318241, 1e-12) && near(c.a2, 0.73248077421585, 1e-12));
    CHECK(near(c.d1, -1.99004745483398, 1e-12) && near(c.d2, 0.99007225036621, 1e-12));
    // any rate: at DC the shelf passes 1 (b(1) / a(1) = 1) and the high-pass blocks (1 - 2 + 1 = 0)
    for (int rate : {8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000}) {
        const LoudCoefs k = loud_coefs(rate);
        CHECK(near((k.b0 + k.b1 + k.b2) / (1.0 + k.a1 + k.a2), 1.0, 1e-9));
        CHECK(k.d2 > 0.0 && k.d2 < 1.0 && 1.0 - std::sqrt(k.d2) < 0.03);  // the high-pass poles inside, and near, the unit circle
    }
}

static void counting() {
    CHECK(loud_hop(8000) == 800 && loud_hop(44100) == 4410 && loud_hop(48000) == 4800);
    CHECK(loud_hop(11025) == 1103 && loud_hop(22050) == 2205 && loud_hop(8004) == 800 && loud_hop(8005) == 801);  // (fs + 5) / 10
    CHECK(loud_hops(0, 8000) == 0 && loud_hops(799, 8000) == 0 && loud_hops(800, 8000) == 1 && loud_hops(3199, 8000) == 3);
    CHECK(loud_blocks(3199, 8000) == 0 && loud_blocks(3200, 8000) == 1 && loud_blocks(3999, 8000) == 1 && loud_blocks(4000, 8000) == 2);
    CHECK(loud_blocks(19199, 48000) == 0 && loud_blocks(19200, 48000) == 1 && loud_blocks(48000 * 30, 48000) == 297);
    CHECK(loud_blocks(44100 * 3, 44100) == 27);
    CHECK(throws([] { loud_require_rate(7999); }) && throws([] { loud_require_rate(48001); }) && throws([] { loud_require_rate(0); }));
    CHECK(!throws([] { loud_require_rate(8000); }) && !throws([] { loud_require_rate(48000); }));
    auto bad = [](double t, double p, double g) {
        LoudParams q;
        q.target_lufs = t; q.peak_db = p; q.max_gain_db = g;
        return throws([&] { loud_require_params(q); });
    };
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    CHECK(!bad(-40, -1, 30) && !bad(-5, 0, 0) && !bad(-18, -60, 60));
    CHECK(bad(-40.01, -1, 30) && bad(-4.99, -1, 30) && bad(nan, -1, 30) && bad(-18, 0.1, 30) && bad(-18, nan, 30) && bad(-18, -inf, 30));
    CHECK(bad(-18, -1, -0.1) && bad(-18, -1, 60.1) && bad(-18, -1, nan));
    std::vector<float> x(10, 0.f);
    CHECK(throws([&] { loud_measure(x.data(), -1, 44100, nullptr); }) && throws([&] { loud_measure(x.data(), 10, 4000, nullptr); }));
}

static void gates() {
    const int h = 1000;
    const double inf = std::numeric_limits<double>::infinity();
    auto hops_of_level = [&](double lufs) { return std::pow(10.0, (lufs + 0.691) / 10.0) * h; };  // s_i of a hop whose blocks measure `lufs`
    // fewer than four hops: nothing
    {
        const double s[3] = {1.0, 1.0, 1.0};
        const LoudResult r = loud_gate(s, 3, h);
        CHECK(r.lufs == -inf && r.blocks_total == 0 && r.blocks_kept == 0);
    }
    // one block at -23
    {
        const double v = hops_of_level(-23.0), s[4] = {v, v, v, v};
        const LoudResult r = loud_gate(s, 4, h);
        CHECK(near(r.lufs, -23.0, 1e-9) && r.blocks_total == 1 && r.blocks_kept == 1);
    }
    // digital silence, and a level under the absolute gate: blocks, none kept
    {
        const double z[6] = {0, 0, 0, 0, 0, 0};
        LoudResult r = loud_gate(z, 6, h);
        CHECK(r.lufs == -inf && r.blocks_total == 3 && r.blocks_kept == 0);
        const double v = hops_of_level(-70.5), q[6] = {v, v, v, v, v, v};
        r = loud_gate(q, 6, h);
        CHECK(r.lufs == -inf && r.blocks_total == 3 && r.blocks_kept == 0);
    }
    // 8 hops at -20, then 8 at -40: blocks 0..4 are at -20, 5..7 mixed (3/4, 1/2, 1/4 loud), 8..12 at -40.  All pass the absolute gate.
    // mean of all 13 = (5 + 1.5 + 0.0325 .. ) -> Gamma about -20 - 3 - 10 = -33: the -40 blocks go, the mixed ones (>= -26) stay: 8 kept,
    // L = 10 log10((5 + 0.75 + 0.5 + 0.25 + (0.25 + 0.5 + 0.75) * 0.01) / 8) - 20 = 10 log10(6.515 / 8) - 20
    {
        std::vector<double> s;
        for (int i = 0; i < 8; ++i) s.push_back(hops_of_level(-20.0));
        for (int i = 0; i < 8; ++i) s.push_back(hops_of_level(-40.0));
        const LoudResult r = loud_gate(s.data(), 16, h);
        CHECK(r.blocks_total == 13 && r.blocks_kept == 8 && near(r.lufs, -20.0 + 10.0 * std::log10(6.515 / 8.0), 1e-9));
    }
    // a NaN hop: the four blocks it touches are never kept
    {
        std::vector<double> s(10, hops_of_level(-23.0));
        s[9] = std::numeric_limits<double>::quiet_NaN();
        const LoudResult r = loud_gate(s.data(), 10, h);
        CHECK(r.blocks_total == 7 && r.blocks_kept == 6 && near(r.lufs, -23.0, 1e-9));
        s[3] = s[9];
        CHECK(loud_gate(s.data(), 10, h).blocks_kept == 2);  // blocks 4 and 5
        s[5] = s[9];
        CHECK(loud_gate(s.data(), 10, h).blocks_kept == 0 && loud_gate(s.data(), 10, h).lufs == -inf);
    }
}

static void gains() {
    LoudParams p;
    p.target_lufs = -18.0;
    const double inf = std::numeric_limits<double>::infinity();
    CHECK(loud_gain(-inf, 0.5f, p) == 1.f);                                               // no loudness: exactly 1
    CHECK(loud_gain(-24.0, 0.1f, p) == (float)std::pow(10.0, 6.0 / 20.0));                // the target decides: +6 dB
    CHECK(loud_gain(-68.0, 0.001f, p) == (float)std::pow(10.0, 30.0 / 20.0));             // 50 LU under: max_gain_db decides
    CHECK(loud_gain(-24.0, 0.5f, p) == (float)(std::pow(10.0, -1.0 / 20.0) / 0.5));       // +6 dB would lift 0.5 over -1 dBFS: the peak decides
    CHECK(loud_gain(-12.0, 1.0f, p) == (float)std::pow(10.0, -6.0 / 20.0));               // attenuation
    CHECK(loud_gain(-24.0, 0.f, p) == (float)std::pow(10.0, 6.0 / 20.0));                 // peak 0: no peak clause
    const float nan = std::numeric_limits<float>::quiet_NaN();
    const float x[5] = {0.25f, -0.75f, nan, 0.5f, -0.f};
    CHECK(loud_peak(x, 5) == 0.75f && loud_peak(x, 0) == 0.f && loud_peak(x + 2, 1) == 0.f);
}

// a known answer and the rows without loudness, through the whole evaluator
static void rows() {
    const int rate = 44100;
    const double pi = 3.14159265358979323846;
    std::vector<float> x((size_t)3 * rate);
    for (size_t i = 0; i < x.size(); ++i) x[i] = (float)std::sin(2.0 * pi * 997.0 * (double)i / rate);
    LoudParams p;
    p.target_lufs = -23.0;
    std::vector<double> hops;
    const LoudResult r = loud_measure(x.data(), (int64_t)x.size(), rate, &p, &hops);
    CHECK(near(r.lufs, -3.01, 0.01) && r.blocks_total == 27 && r.blocks_kept == 27 && hops.size() == 30);  // a full-scale 997 Hz sine: -3.01 LUFS
    CHECK(near(r.peak, 1.0, 1e-6) && near(r.gain, std::pow(10.0, (-23.0 - r.lufs) / 20.0), 1e-6));
    const double inf = std::numeric_limits<double>::infinity();
    LoudResult s = loud_measure(x.data(), 4 * 4410 - 1, rate, &p);
    CHECK(s.lufs == -inf && s.gain == 1.f && s.blocks_total == 0 && s.peak > 0.99f);
    s = loud_measure(x.data(), 4 * 4410, rate, &p);
    CHECK(s.blocks_total == 1 && s.blocks_kept == 1 && near(s.lufs, -3.0, 0.1));
    s = loud_measure(x.data(), 0, rate, &p);
    CHECK(s.lufs == -inf && s.gain == 1.f && s.peak == 0.f);
    std::vector<float> z((size_t)rate, 0.f);
    s = loud_measure(z.data(), rate, rate, &p);
    CHECK(s.lufs == -inf && s.gain == 1.f && s.blocks_total == 7 && s.blocks_kept == 0 && s.peak == 0.f);
    s = loud_measure(x.data(), rate, rate, nullptr);  // measuring only: gain 1
    CHECK(s.gain == 1.f && s.lufs > -4.0);
}

// the kernels' decomposition on the host, with the tables they read, against the serial walk
static void chunked(int rate, int64_t n, unsigned seed) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> u(-1.f, 1.f);
    std::vector<float> x((size_t)n);
    for (auto& v : x) v = u(rng);
    const LoudCoefs c = loud_coefs(rate);
    const std::vector<double> tab = loud_tables(rate);
    CHECK(tab.size() == kLoudTabDoubles);
    const int64_t nwg = (n + kLoudSpan - 1) / kLoudSpan, nchunk = nwg * kLoudWg;
    auto at = [&](int64_t a) { return a < n ? (double)x[(size_t)a] : 0.0; };
    auto mac = [](const double* m, const double* v, double* r) {
        for (int i = 0; i < 4; ++i) r[i] += m[i * 4] * v[0] + m[i * 4 + 1] * v[1] + m[i * 4 + 2] * v[2] + m[i * 4 + 3] * v[3];
    };
    // pass 1: zero-state chunk states, then per workgroup the inclusive scan with P[k]
    std::vector<double> st((size_t)nchunk * 4, 0.0);
    for (int64_t ch = 0; ch < nchunk; ++ch)
        for (int k = 0; k < kLoudChunk; ++k) (void)loud_step(c, at(ch * kLoudChunk + k), &st[(size_t)ch * 4]);
    for (int64_t w = 0; w < nwg; ++w)
        for (int k = 0; k < kLoudScanSteps; ++k) {
            const int off = 1 << k;
            std::vector<double> prev(st.begin() + (size_t)w * kLoudWg * 4, st.begin() + (size_t)(w + 1) * kLoudWg * 4);
            for (int l = off; l < kLoudWg; ++l) mac(&tab[kLoudTabP + 16 * (size_t)k], &prev[(size_t)(l - off) * 4], &st[((size_t)w * kLoudWg + (size_t)l) * 4]);
        }
    // pass 2: the row's state at every workgroup, every lane's entry state, the chunks again
    std::vector<double> z((size_t)n);
    double sw[4] = {0, 0, 0, 0};
    for (int64_t w = 0; w < nwg; ++w) {
        for (int l = 0; l < kLoudWg; ++l) {
            double s[4] = {0, 0, 0, 0};
            if (l) for (int i = 0; i < 4; ++i) s[i] = st[((size_t)w * kLoudWg + (size_t)l - 1) * 4 + (size_t)i];
            mac(&tab[kLoudTabLane + 16 * (size_t)l], sw, s);
            for (int k = 0; k < kLoudChunk; ++k) {
                const int64_t a = (w * kLoudWg + l) * kLoudChunk + k;
                const double v = loud_step(c, at(a), s);
                if (a < n) z[(size_t)a] = v;
            }
        }
        double r[4];
        for (int i = 0; i < 4; ++i) r[i] = st[((size_t)w * kLoudWg + kLoudWg - 1) * 4 + (size_t)i];
        mac(&tab[kLoudTabP + 16 * (size_t)kLoudScanSteps], sw, r);
        for (int i = 0; i < 4; ++i) sw[i] = r[i];
    }
    double s[4] = {0, 0, 0, 0}, worst = 0.0, scale = 0.0;
    for (int64_t a = 0; a < n; ++a) {
        const double v = loud_step(c, (double)x[(size_t)a], s);
        worst = std::max(worst, std::fabs(v - z[(size_t)a]));
        scale = std::max(scale, std::fabs(v));
    }
    CHECK(scale > 0.5 && worst <= 1e-9 * scale);  // (rounding alone: about 1e-13 in practice; a wrong table entry is off by its own size)
}

int main() {
    coefficients();
    counting();
    gates();
    gains();
    rows();
    chunked(44100, 2 * kLoudSpan + 4410 + 17, 1);
    chunked(48000, kLoudSpan, 2);
    chunked(8000, kLoudSpan + 1, 3);
    chunked(24000, 100, 4);
    std::printf("loud_plan_check ok\n");
    return 0;
}
