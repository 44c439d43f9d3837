// Host check of the chunked time stretch (csrc/fs_tsm_plan.h, "streams"): the emission rule, the carry start, the derived carry bound and the
// evaluator that runs the definition chunk by chunk.  Over speeds {0.25, 0.5, 0.77, 1.0, 1.25, 2.0, 3.0, 4.0}, (N, D) in {(1024, 512),
// (64, 0), (66, 3), (256, 64), (2048, 1024)} and seeded chunk sequences, one-sample chunks among them, it checks, from the index arithmetic
// written out again here and not from the header's helpers:
//   * emittability is monotone in k, so a call emits a prefix;
//   * no frame emitted before the final item reads at or beyond n, or below the start of the carry the call was given;
//   * the carry never exceeds tsm_carry_bound, and the bound is not slack by more than a few samples at its worst case;
//   * the emitted totals equal out_len(n);
//   * TsmStreamEval, fed the chunks, returns the samples and positions of tsm_eval bit for bit.
// Every step of every sequence is also printed ("case ..." lines), so that tests/test_tsm_stream_plan_cpu.py can hold its numpy restatement of
// the rule to this header.  The last line is "tsm_stream_plan_check ok".
// Meant to run under the sanitizers:
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/tsm_stream_plan_check.cpp -o tsm_stream_plan_check && ./tsm_stream_plan_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <stdexcept>
#include <vector>

#include "../fish-speech.rs_amd/csrc/fs_tsm_plan.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "tsm_stream_plan_check: %s failed at line %d\n", #c, __LINE__); std::exit(1); } } while (0)

using namespace fs;

static const double kSpeeds[] = {0.25, 0.5, 0.77, 1.0, 1.25, 2.0, 3.0, 4.0};
static const int kParams[][2] = {{1024, 512}, {64, 0}, {66, 3}, {256, 64}, {2048, 1024}};

// the rule's index arithmetic, from the text
static long long q_of(long long k, int Hs, double speed) { return (long long)std::floor((double)(k * Hs) * speed + 0.5); }
static long long out_len_of(long long n, double speed) { return n <= 0 ? 0 : (long long)std::floor((double)n / speed + 0.5); }

// chunk lengths summing to n: style 0 = one chunk, 1 = all ones, 2 = random up to 2 N, 3 = random with runs of one-sample chunks, 4 = all 300
static std::vector<int64_t> chunks_of(int64_t n, int style, int N, std::mt19937& rng) {
    std::vector<int64_t> c;
    int64_t left = n;
    while (left > 0) {
        int64_t t = left;
        if (style == 1) t = 1;
        else if (style == 2) t = 1 + (int64_t)(rng() % (unsigned)(2 * N));
        else if (style == 3) t = rng() % 3 == 0 ? 1 : 1 + (int64_t)(rng() % (unsigned)N);
        else if (style == 4) t = 300;
        t = std::min(t, left);
        c.push_back(t);
        left -= t;
    }
    if (c.empty() || style == 3) c.push_back(0);  // a pure flush
    return c;
}

static int64_t g_worst_default = 0;

// one sequence through the planner alone
static void rule_case(double speed, const TsmParams& p, const std::vector<int64_t>& chunks, bool print) {
    const int Hs = p.Hs(), N = p.N, D = p.D;
    const int64_t bound = tsm_carry_bound(p, speed);
    TsmBook book;
    int64_t emitted = 0;
    if (print) std::printf("case %.17g %d %d %lld :", speed, N, D, (long long)bound);
    for (size_t c = 0; c < chunks.size(); ++c) {
        const bool final = c + 1 == chunks.size();
        const int64_t carry_start_in = book.n_in - book.carry_len;
        const TsmStep s = tsm_plan_step(p, speed, book, chunks[c], final);
        const long long n = s.n_total;
        CHECK(s.in0 == book.n_in && s.k0 == book.k_next && s.out0 == book.n_out && s.k1 >= s.k0 && s.n_emit >= 0);
        if (!final) {
            // a prefix: every frame below k1 is emittable, none of the next ones is
            for (int64_t k = 0; k < s.k1 + 24; ++k) CHECK(tsm_emittable(k, n, speed, p) == (k < s.k1));
            CHECK(s.n_emit == (s.k1 - s.k0) * Hs && (s.k1 * Hs) <= out_len_of(n, speed));
            for (int64_t k = s.k0; k < s.k1; ++k) {
                // what frame k can read: [0, Hs) for k == 0, else the region [q_k - D, q_k + D + N) and the template anywhere in
                // [lo_{k-1} + Hs, hi_{k-1} + Hs + N)
                long long lo = 0, hi = Hs;
                if (k >= 1) {
                    const long long q = q_of(k, Hs, speed), qm = q_of(k - 1, Hs, speed);
                    const long long tlo = (k == 1 ? 0 : qm - D) + Hs, thi = (k == 1 ? 0 : qm + D) + Hs + N;
                    lo = std::max(0ll, std::min(q - D, tlo));
                    hi = std::max(q + D + N, thi);
                }
                CHECK(hi <= n);
                CHECK(lo >= carry_start_in);
            }
            CHECK(s.carry_len <= bound && s.carry_start >= carry_start_in && s.carry_start + s.carry_len == n);
            if (N == kTsmFrame && D == kTsmRadius) g_worst_default = std::max(g_worst_default, s.carry_len);
        } else {
            const long long ol = out_len_of(n, speed);
            CHECK(s.out0 + s.n_emit == ol && s.k1 == (ol + Hs - 1) / Hs && s.carry_len == 0);
            CHECK(n > 0 || s.n_emit == 0);
        }
        emitted += s.n_emit;
        if (print) std::printf(" %lld,%d,%lld,%lld,%lld,%lld", (long long)chunks[c], (int)final, (long long)s.k0, (long long)s.k1, (long long)s.n_emit, (long long)s.carry_start);
        tsm_commit(book, s, final);
    }
    if (print) std::printf("\n");
    CHECK(emitted == out_len_of(book.n_in, speed) && book.final);
    bool refused = false;
    try { (void)tsm_plan_step(p, speed, book, 1, false); } catch (const std::invalid_argument&) { refused = true; }
    CHECK(refused);
}

static void rule() {
    std::mt19937 rng(20240607);
    for (double speed : kSpeeds)
        for (const auto& pr : kParams) {
            TsmParams p;
            p.N = pr[0]; p.D = pr[1];
            const int64_t n = (int64_t)std::ceil(speed * p.Hs() * 11.3) + 2 * p.D + 17;
            for (int style = 0; style < 5; ++style) rule_case(speed, p, chunks_of(n, style, p.N, rng), style != 1);
            rule_case(speed, p, chunks_of(n / 3 + 1, 2, p.N, rng), true);
            for (int64_t e : {(int64_t)0, (int64_t)1, (int64_t)p.Hs() - 1, (int64_t)p.Hs(), (int64_t)p.Hs() + 1}) rule_case(speed, p, chunks_of(e, 0, p.N, rng), true);
        }
    // the bound at the defaults, over every n (one-sample chunks) and a fine grid of speeds: never exceeded, and reached to within 8 samples
    const TsmParams d;
    int64_t worst = 0, worst_bound = 0;
    for (int i = 0; i <= 60; ++i) {
        const double speed = 0.25 + (4.0 - 0.25) * i / 60.0;
        TsmBook book;
        for (int64_t n = 1; n <= 30000; ++n) {
            const TsmStep s = tsm_plan_step(d, speed, book, 1, false);
            CHECK(s.carry_len <= tsm_carry_bound(d, speed));
            if (s.carry_len > worst) { worst = s.carry_len; worst_bound = tsm_carry_bound(d, speed); }
            tsm_commit(book, s, false);
        }
    }
    CHECK(tsm_carry_bound(d, 4.0) == 4098 && tsm_carry_bound(d, 0.25) == 2433);
    CHECK(worst <= worst_bound && worst + 8 >= worst_bound);
    std::printf("default parameters: largest carry %lld (bound there %lld)\n", (long long)worst, (long long)worst_bound);
}

// the chunked evaluator against the one-shot one, bit for bit
static void evaluator() {
    std::mt19937 rng(99);
    std::uniform_real_distribution<float> u(-1.f, 1.f);
    for (double speed : kSpeeds)
        for (const auto& pr : kParams) {
            TsmParams p;
            p.N = pr[0]; p.D = pr[1];
            const int64_t n = (int64_t)std::ceil(speed * p.Hs() * (p.N >= 1024 ? 6.3 : 9.3)) + 17;
            std::vector<float> x((size_t)n);
            for (auto& v : x) v = u(rng);
            std::vector<int64_t> pos;
            const std::vector<float> y = tsm_eval(x.data(), n, speed, p, &pos);
            for (int style : {2, 3}) {
                const std::vector<int64_t> chunks = chunks_of(n, style, p.N, rng);
                TsmStreamEval ev(speed, p);
                std::vector<float> yc;
                std::vector<int64_t> posc;
                int64_t at = 0;
                for (size_t c = 0; c < chunks.size(); ++c) {
                    // the chunk alone, in storage of its own: nothing but the carry can supply earlier samples
                    const std::vector<float> chunk(x.begin() + at, x.begin() + at + chunks[c]);
                    const std::vector<float> part = ev.feed(chunk.data(), chunks[c], c + 1 == chunks.size(), &posc);
                    yc.insert(yc.end(), part.begin(), part.end());
                    at += chunks[c];
                }
                CHECK(posc == pos);
                CHECK(yc.size() == y.size() && (y.empty() || std::memcmp(yc.data(), y.data(), y.size() * sizeof(float)) == 0));
            }
        }
    // a stream that never saw a sample
    TsmStreamEval ev(1.25, TsmParams{});
    CHECK(ev.feed(nullptr, 0, true).empty());
}

int main() {
    rule();
    evaluator();
    std::printf("tsm_stream_plan_check ok\n");
    return 0;
}
