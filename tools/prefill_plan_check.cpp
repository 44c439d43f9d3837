// Host check of the prefill pass planner (csrc/fs_prefill_plan.h): which of a session's queued requests go into its next prefill pass, decided
// against a real page book (csrc/fs_kv_pages.h, pages of 64 positions) that is driven the way the engine drives it -- a request's own pages
// taken when it is queued (a slot shares its prefix's full pages, grows its private ones and holds the prefix's partly filled last page), a
// group's members grown to where their pad rows write when the pass is launched, a prefix trimmed to its length and a slot's hold dropped
// when it has run.
// Scripted queues: every expected plan below is written out by hand from the rules (the header's comment), never taken from the planner.
// The one exception is the burst of 32 requests, whose pass count was read off the engine on an MI355X.
// A seeded random walk: queues of imports, creations, plain, prefixed and seeded adds over a pool too small for all of them, 20 000
// planned passes and more; after every plan the invariants of a pass are asserted in words of their own (invariants()), the plan is
// carried out on the book, and every queued entry must be consumed exactly once.
// Meant to run under the sanitizers:
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/prefill_plan_check.cpp -o prefill_plan_check && ./prefill_plan_check
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <stdexcept>
#include <vector>

#include "../fish-speech.rs_amd/csrc/fs_prefill_plan.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "prefill_plan_check: %s failed at line %d\n", #c, __LINE__); std::exit(1); } } while (0)

using fs::KvPages;
using fs::PrefillLimits;
using fs::PrefillMember;
using fs::PrefillPass;
using fs::PrefillPlan;

constexpr int PAGE = 64;
static int pages_of(int n_tokens) { return (n_tokens + PAGE - 1) / PAGE; }

// a session's queue next to its page book; an entry is the planner's record plus what the check needs to carry the pass out
struct Entry {
    PrefillMember m;
    int id = -1, slot = -1, prefix = -1, tail = -1;
};
struct Prefix { int P = 0, owner = -1; bool live = true; };
struct Sess {
    KvPages book;
    std::vector<Entry> queue;
    std::vector<Prefix> prefixes;
    std::vector<char> slot_used;
    int next_id = 0;
    std::vector<char> consumed;  // per entry id
    Sess(int n_pages, int n_seq, int max_tokens) : slot_used((size_t)n_seq, 0) { book.init(n_pages, n_seq, PAGE, max_tokens); }
    Entry& push(Entry e) {
        e.id = next_id++;
        consumed.push_back(0);
        queue.push_back(e);
        return queue.back();
    }
    // fs_lm_session_prefix_create / _import: the prefix's pages taken now, its pass queued.  -1: the pool is short
    int add_prefix(int P, bool import_kv) {
        if (!book.room(KvPages::kNewOwner, P).fits) return -1;
        Prefix px;
        px.P = P; px.owner = book.add_prefix();
        book.grow(px.owner, P);
        prefixes.push_back(px);
        Entry e;
        e.m.L = P; e.m.create = true; e.m.import_kv = import_kv; e.m.owner = px.owner; e.prefix = (int)prefixes.size() - 1;
        push(e);
        return e.prefix;
    }
    // fs_lm_session_add*: slot b, `cols` columns of its own behind prefix `prefix` (-1: none), n_iter iterations.  False: the pool is short
    bool add(int b, int cols, int n_iter, int prefix = -1, bool has_seed = false) {
        const int P = prefix >= 0 ? prefixes[(size_t)prefix].P : 0, L = P + cols, end = L + n_iter - 1, nfull = P / PAGE;
        const KvPages::Share sh{prefix >= 0 ? prefixes[(size_t)prefix].owner : -1, nfull};
        if (!book.room(b, end, sh).fits) return false;
        book.share(b, sh);
        book.grow(b, end);
        Entry e;
        e.m.L = L; e.m.n_iter = n_iter; e.m.start = P; e.m.owner = b; e.m.has_seed = has_seed; e.slot = b; e.prefix = prefix;
        if (P % PAGE) e.tail = book.hold_page_of(sh.from, nfull);
        push(e);
        slot_used[(size_t)b] = 1;
        return true;
    }
    std::vector<PrefillMember> members() const {
        std::vector<PrefillMember> q;
        for (const Entry& e : queue) q.push_back(e.m);
        return q;
    }
    PrefillPlan plan(const PrefillLimits& lim) const { return fs::plan_prefill(members(), book, lim); }
    // what the engine does with a plan: the queue in the plan's order, a group's members grown to their pad_end, the pass's members off
    // the queue and activated (a prefix trimmed to its length, a slot's hold on its prefix's last page dropped).  Returns the members.
    std::vector<Entry> carry_out(const PrefillPlan& p) {
        CHECK(p.order.size() == queue.size());
        std::vector<Entry> ordered;
        for (int j : p.order) ordered.push_back(queue.at((size_t)j));
        queue = ordered;
        const PrefillPass& ps = p.pass;
        CHECK(ps.n >= 0 && (size_t)ps.n <= queue.size());
        if (ps.kind == PrefillPass::Group) {
            CHECK(ps.pad_end.size() == (size_t)ps.n);
            for (int s = 0; s < ps.n; ++s) book.grow(queue[(size_t)s].m.owner, ps.pad_end[(size_t)s]);  // (throws: the check fails)
        } else
            CHECK(ps.pad_end.empty());  // (no other kind grows anything)
        book.check();
        std::vector<Entry> done(queue.begin(), queue.begin() + ps.n);
        queue.erase(queue.begin(), queue.begin() + ps.n);
        for (const Entry& e : done) {
            CHECK(!consumed.at((size_t)e.id));
            consumed[(size_t)e.id] = 1;
            if (e.m.create) {
                const Prefix& px = prefixes[(size_t)e.prefix];
                book.truncate(px.owner, px.P);
                if (!px.live) book.drop(px.owner);
            } else if (e.tail >= 0)
                book.drop_hold(e.tail);
        }
        book.check();
        return done;
    }
    void release_slot(int b) { book.truncate(b, 0); slot_used[(size_t)b] = 0; }
};

static void expect(const PrefillPlan& p, std::vector<int> order, PrefillPass::Kind kind, int n, int Lp = 0, int max_start = 0,
                   std::vector<int> pad_end = {}) {
    CHECK(p.order == order);
    CHECK(p.pass.kind == kind && p.pass.n == n);
    if (kind == PrefillPass::Single || kind == PrefillPass::Group) CHECK(p.pass.Lp == Lp && p.pass.max_start == max_start);
    CHECK(p.pass.pad_end == pad_end);
}

static const PrefillLimits kLim{/*rows_cap=*/2048, /*max_batch=*/32, /*max_seq_len=*/4096, /*flash=*/true};

// 1. an import, a creation and adds queued together: three successive passes in that order; the adds wait even when they have nothing
// to prefill, and the one-column add is what is left at the end
static void kinds_in_order() {
    Sess t(64, 8, 4096);
    CHECK(t.add(0, /*cols=*/1, /*n_iter=*/10));   // rows 0
    CHECK(t.add(1, 50, 10));                      // rows 49, keeps 59 positions
    CHECK(t.add_prefix(70, false) == 0);          // rows 70
    CHECK(t.add_prefix(100, true) == 1);          // an import: rows 0
    CHECK(t.add(2, 30, 10));                      // rows 29, keeps 39 positions; padded to 49 rows it writes 49
    expect(t.plan(kLim), {3, 2, 1, 4, 0}, PrefillPass::Imports, 1);
    t.carry_out(t.plan(kLim));
    expect(t.plan(kLim), {0, 1, 2, 3}, PrefillPass::Single, 1, 70, 0);  // (the creation: no add joins a creation)
    t.carry_out(t.plan(kLim));
    expect(t.plan(kLim), {0, 1, 2}, PrefillPass::Group, 2, 49, 0, {59, 49});
    t.carry_out(t.plan(kLim));
    expect(t.plan(kLim), {0}, PrefillPass::NoRows, 1);
    t.carry_out(t.plan(kLim));
    CHECK(t.queue.empty());
}

// 2. only one-column bodies: no pass, all of them at once
static void no_rows() {
    Sess t(64, 8, 4096);
    CHECK(t.add_prefix(65, false) == 0);
    t.carry_out(t.plan(kLim));  // (the prefix is there)
    CHECK(t.add(0, 1, 5) && t.add(1, 1, 5, /*prefix=*/0) && t.add(2, 1, 5));
    expect(t.plan(kLim), {0, 1, 2}, PrefillPass::NoRows, 3);
    CHECK(t.carry_out(t.plan(kLim)).size() == 3 && t.queue.empty());
}

// 3. / 4. a member with a sampler seed of its own goes alone: sorted first, and behind an unseeded first, where it ends the group
static void seeded() {
    {
        Sess t(64, 8, 4096);
        CHECK(t.add(0, 60, 10) && t.add(1, 100, 10, -1, /*has_seed=*/true) && t.add(2, 40, 10));
        expect(t.plan(kLim), {1, 0, 2}, PrefillPass::Single, 1, 99, 0);
        t.carry_out(t.plan(kLim));
        expect(t.plan(kLim), {0, 1}, PrefillPass::Group, 2, 59, 0, {69, 59});  // (keeps 60 + 9 / 40 + 9 = 49 < 59 pad rows)
    }
    {
        Sess t(64, 8, 4096);
        CHECK(t.add(0, 100, 10) && t.add(1, 80, 10) && t.add(2, 60, 10, -1, true) && t.add(3, 40, 10));
        expect(t.plan(kLim), {0, 1, 2, 3}, PrefillPass::Group, 2, 99, 0, {109, 99});
        t.carry_out(t.plan(kLim));
        expect(t.plan(kLim), {0, 1}, PrefillPass::Single, 1, 59, 0);  // (the seeded one, now first)
        t.carry_out(t.plan(kLim));
        expect(t.plan(kLim), {0}, PrefillPass::Single, 1, 39, 0);
    }
}

// 5. / 6. the row buffers hold fit = rows_cap / Lp members, the staging rows max_batch
static void row_limits() {
    Sess t(64, 8, 4096);
    for (int b = 0; b < 5; ++b) CHECK(t.add(b, 501, 1));  // Lp = 500: fit = 2048 / 500 = 4 of the 5
    expect(t.plan(kLim), {0, 1, 2, 3, 4}, PrefillPass::Group, 4, 500, 0, {501, 501, 501, 501});
    PrefillLimits two = kLim;
    two.max_batch = 2;
    expect(t.plan(two), {0, 1, 2, 3, 4}, PrefillPass::Group, 2, 500, 0, {501, 501});
}

// 7. a prefixed member whose pad rows would pass max_seq_len ends the group; it leads the next one (the first member is not held to that)
static void max_seq_len() {
    PrefillLimits lim = kLim;
    lim.max_seq_len = 512;
    Sess t(64, 8, 512);
    CHECK(t.add_prefix(256, false) == 0);
    t.carry_out(t.plan(lim));
    CHECK(t.add(0, 5, 1));             // rows 4
    CHECK(t.add(1, 10, 1, 0));         // rows 9 from position 256: 256 + 300 > 512
    CHECK(t.add(2, 301, 1));           // rows 300
    CHECK(t.add(3, 250, 1));           // rows 249, keeps 250, writes 300
    expect(t.plan(lim), {2, 3, 1, 0}, PrefillPass::Group, 2, 300, 0, {301, 300});
    t.carry_out(t.plan(lim));
    expect(t.plan(lim), {0, 1}, PrefillPass::Group, 2, 9, 256, {266, 9});  // (keeps 256 + 10; the plain one keeps 5 and writes 9)
}

// 8. / 9. the pool in the middle of a group.  The first member's owner is one page short of what its own pass writes (the engine never
// leaves it so -- admission takes every page a slot keeps -- but the planner asks the book all the same)
static void short_pool() {
    for (int third : {0, 1}) {
        Sess t(/*n_pages=*/third ? 12 : 9, 8, 4096);
        CHECK(t.add(0, 301, 1) && t.add(1, 100, 1) && t.add(2, 90, 1));  // 5 + 2 + 2 pages
        t.book.truncate(0, 256);                                         // the first keeps 4 of its 5 pages: padding costs 1, the others 3 each
        CHECK(t.book.free_count() == (third ? 4 : 1));
        if (third) {  // 8. room for 1 + 3, not for 3 more: the group stops at two, and growing them succeeds
            const PrefillPlan p = t.plan(kLim);
            expect(p, {0, 1, 2}, PrefillPass::Group, 2, 300, 0, {301, 300});
            t.carry_out(p);
            CHECK(t.book.free_count() == 0 && t.book.of(0).size() == 5 && t.book.of(1).size() == 5 && t.book.of(2).size() == 2);
        } else {      // 9. room for the first one's page alone: nobody joins
            expect(t.plan(kLim), {0, 1, 2}, PrefillPass::Single, 1, 300, 0);
            CHECK(t.book.hold_new() >= 0);  // ... and not even that: the first goes alone, and a single pass grows nothing
            CHECK(t.book.free_count() == 0);
            const PrefillPlan p = t.plan(kLim);
            expect(p, {0, 1, 2}, PrefillPass::Single, 1, 300, 0);
            t.carry_out(p);
            CHECK(t.book.free_count() == 0 && t.book.of(0).size() == 4);
        }
    }
}

// 10. no group pass without the flash kernel (head_dim != 64), or when the longest member alone overflows the row buffers
static void single_only() {
    Sess t(128, 8, 4096);
    CHECK(t.add(0, 100, 1) && t.add(1, 80, 1));
    PrefillLimits chunked = kLim;
    chunked.flash = false;
    expect(t.plan(chunked), {0, 1}, PrefillPass::Single, 1, 99, 0);
    expect(t.plan(kLim), {0, 1}, PrefillPass::Group, 2, 99, 0, {100, 99});
    CHECK(t.add(2, 3000, 1));
    expect(t.plan(kLim), {2, 0, 1}, PrefillPass::Single, 1, 2999, 0);
}

// 11. a burst of 32 requests into an idle max_batch = 32 session of a Fish-1.5-sized handle (max_seq_len 8192): the prompt lengths are
// the first 32 of numpy.random.RandomState(77).randint(64, 385, 256) (bench.config2_prompts), 16 frames each.  The engine before this
// planner existed reports session_info()["prefill_passes"] == kBurstPasses for it (read on an MI355X).
static const int kBurstLens[32] = {279, 159, 148, 299, 357, 216, 288, 231, 181, 236, 339, 379, 292, 118, 270, 74,
                                   263, 355, 251, 321, 331, 190, 293, 248, 161, 360, 321, 246, 196, 221, 371, 348};
constexpr int kBurstPasses = 5;
static void burst() {
    PrefillLimits lim = kLim;
    lim.max_seq_len = 8192;
    Sess t(32 * pages_of(8192), 32, 8192);
    for (int b = 0; b < 32; ++b) CHECK(t.add(b, kBurstLens[b], 16));
    int passes = 0, members = 0;
    while (!t.queue.empty()) {
        const PrefillPlan p = t.plan(lim);
        CHECK(p.pass.kind == PrefillPass::Group);
        members += (int)t.carry_out(p).size();
        ++passes;
    }
    CHECK(members == 32 && passes == kBurstPasses);
}

// ---- the random walk
// What must hold of any plan, in words of its own: `q` is the queue the plan was made for, `book` the book before anything was grown.
struct Tally { long plans = 0, groups = 0, pool_stops = 0, kinds[4] = {0, 0, 0, 0}; };
static int cls(const PrefillMember& m) { return m.import_kv ? 0 : (m.create ? 1 : 2); }
static int written_to(const PrefillMember& m, int Lp) { return std::max(m.end(), m.start + Lp); }  // a pass of Lp rows, from its start
static int page_cost(const KvPages& book, const PrefillMember& m, int Lp) {
    return std::max(0, pages_of(written_to(m, Lp)) - (int)book.of(m.owner).size());
}
static void invariants(const std::vector<PrefillMember>& q, const KvPages& book, const PrefillLimits& lim, const PrefillPlan& p, Tally& tally) {
    const size_t N = q.size();
    // the order: a permutation; imports < creations < adds, then rows descending; equals in their order of arrival
    CHECK(p.order.size() == N);
    std::vector<char> seen(N, 0);
    for (int j : p.order) { CHECK(j >= 0 && (size_t)j < N && !seen[(size_t)j]); seen[(size_t)j] = 1; }
    std::vector<PrefillMember> o;
    for (int j : p.order) o.push_back(q[(size_t)j]);
    for (size_t i = 1; i < N; ++i) {
        const PrefillMember &a = o[i - 1], &b = o[i];
        CHECK(cls(a) <= cls(b));
        if (cls(a) == cls(b)) CHECK(a.rows() >= b.rows());
        if (cls(a) == cls(b) && a.rows() == b.rows()) CHECK(p.order[i - 1] < p.order[i]);
    }
    // the members: a prefix of the ordered queue, never empty
    const PrefillPass& ps = p.pass;
    const int n = ps.n;
    CHECK(n >= 1 && (size_t)n <= N);
    ++tally.plans;
    ++tally.kinds[ps.kind];
    size_t n_imports = 0;
    for (const PrefillMember& m : q) n_imports += m.import_kv;
    if (n_imports) {  // imports: all of them, nothing else
        CHECK(ps.kind == PrefillPass::Imports && (size_t)n == n_imports);
        for (int s = 0; s < n; ++s) CHECK(o[(size_t)s].import_kv);
        return;
    }
    int longest = 0;
    for (const PrefillMember& m : q) longest = std::max(longest, m.rows());
    if (longest < 1) {  // nothing to run anywhere (a creation always has rows): everything at once
        CHECK(ps.kind == PrefillPass::NoRows && (size_t)n == N);
        return;
    }
    CHECK(ps.kind == PrefillPass::Single || ps.kind == PrefillPass::Group);
    CHECK((ps.kind == PrefillPass::Single) == (n == 1));
    const int Lp = ps.Lp;
    CHECK(Lp == o[0].rows() && Lp >= 1);
    for (const PrefillMember& m : o) CHECK(m.create != o[0].create || m.rows() <= Lp);  // the first is the longest of its kind
    int max_start = 0, cost = 0;
    for (int s = 0; s < n; ++s) max_start = std::max(max_start, o[(size_t)s].start);
    CHECK(ps.max_start == max_start);
    if (ps.kind == PrefillPass::Single) {
        CHECK(ps.pad_end.empty());
    } else {
        ++tally.groups;
        CHECK(lim.flash && n * Lp <= lim.rows_cap && n <= lim.max_batch);
        CHECK(ps.pad_end.size() == (size_t)n);
        for (int s = 0; s < n; ++s) {
            const PrefillMember& m = o[(size_t)s];
            CHECK(m.create == o[0].create && !m.import_kv && !m.has_seed && m.rows() >= 1);
            if (s > 0) CHECK(m.start + Lp <= lim.max_seq_len);
            CHECK(ps.pad_end[(size_t)s] == written_to(m, Lp) && ps.pad_end[(size_t)s] <= lim.max_seq_len);
            cost += page_cost(book, m, Lp);
        }
        CHECK(cost <= book.free_count());
    }
    // ... and why it took no more: the next one in line breaks one of the rules, or the pool has no room for its pad pages as well
    if ((size_t)n < N && lim.flash && Lp <= lim.rows_cap) {
        const PrefillMember& m = o[(size_t)n];
        const bool rows_full = (n + 1) * Lp > lim.rows_cap || n + 1 > lim.max_batch;
        const bool barred = m.rows() < 1 || m.create != o[0].create || o[0].has_seed || m.has_seed || m.start + Lp > lim.max_seq_len;
        if (!rows_full && !barred) {
            if (n == 1) cost = page_cost(book, o[0], Lp);
            CHECK(cost + page_cost(book, m, Lp) > book.free_count());
            ++tally.pool_stops;
        }
    }
}

static void walk(unsigned seed, long n_plans, Tally& tally) {
    const int n_seq = 8, max_tokens = 6 * PAGE, n_pages = 26;
    std::mt19937 rng(seed);
    auto pick = [&](int n) { return (int)(rng() % (unsigned)n); };
    long refused = 0;
    const long target = tally.plans + n_plans;
    while (tally.plans < target) {
        Sess t(n_pages, n_seq, max_tokens);
        const PrefillLimits lim{/*rows_cap=*/128 << 2 * pick(3), /*max_batch=*/2 + pick(n_seq), max_tokens, /*flash=*/pick(8) != 0};
        auto one_pass = [&] {
            const std::vector<PrefillMember> q = t.members();
            const KvPages before = t.book;
            const PrefillPlan p = t.plan(lim);
            invariants(q, before, lim, p, tally);
            t.carry_out(p);
        };
        for (int it = 0, n_ops = 50 + pick(400); it < n_ops; ++it) {
            const int op = pick(100);
            if (op < 55) {  // an add: plain or on a live prefix (its pass may still be queued), now and then with a seed or a one-column body
                int b = -1;
                for (int i = 0; i < n_seq; ++i) if (!t.slot_used[(size_t)i]) { b = i; break; }
                if (b < 0) continue;
                int prefix = t.prefixes.empty() || pick(3) == 0 ? -1 : pick((int)t.prefixes.size());
                if (prefix >= 0 && !t.prefixes[(size_t)prefix].live) prefix = -1;
                const int P = prefix >= 0 ? t.prefixes[(size_t)prefix].P : 0;
                const int cols = pick(8) == 0 ? 1 : 1 + pick(std::min(200, max_tokens - P));
                const int n_iter = 1 + pick(std::min(20, max_tokens - P - cols + 1));
                refused += !t.add(b, cols, n_iter, prefix, pick(10) == 0);
            } else if (op < 66) {
                if (t.prefixes.size() < 6) refused += t.add_prefix(1 + pick(3 * PAGE), /*import_kv=*/pick(3) == 0) < 0;
            } else if (op < 76) {
                if (!t.queue.empty()) one_pass();
            } else if (op < 94) {  // a slot that has joined leaves
                const int b = pick(n_seq);
                bool queued = false;
                for (const Entry& e : t.queue) queued = queued || e.slot == b;
                if (t.slot_used[(size_t)b] && !queued) t.release_slot(b);
            } else if (op < 97) {  // a prefix is released (one whose pass is still queued goes after it)
                if (t.prefixes.empty()) continue;
                Prefix& px = t.prefixes[(size_t)pick((int)t.prefixes.size())];
                if (!px.live) continue;
                px.live = false;
                bool queued = false;
                for (const Entry& e : t.queue) queued = queued || (e.m.create && e.m.owner == px.owner);
                if (!queued) t.book.drop(px.owner);
            } else {  // the queue is drained by planning alone
                while (!t.queue.empty()) one_pass();
            }
            t.book.check();
        }
        while (!t.queue.empty()) one_pass();
        for (char c : t.consumed) CHECK(c);  // every entry ever queued went into exactly one pass (carry_out refuses a second)
        t.book.end_session();
        CHECK(t.book.free_count() == n_pages);
    }
    CHECK(refused > 100);
}

int main() {
    kinds_in_order();
    no_rows();
    seeded();
    row_limits();
    max_seq_len();
    short_pool();
    single_only();
    burst();
    Tally tally;
    walk(20241020u, 20000, tally);
    walk(7u, 5000, tally);
    std::printf("prefill_plan_check: %ld plans (%ld imports, %ld without rows, %ld single, %ld group; %ld passes ended by the pool)\n", tally.plans,
                tally.kinds[0], tally.kinds[1], tally.kinds[2], tally.kinds[3], tally.pool_stops);
    // (the pool is small on purpose: each of these happens all the time)
    CHECK(tally.plans >= 25000 && tally.groups > 1000 && tally.pool_stops > 300);
    for (long k : tally.kinds) CHECK(k > 300);
    std::puts("prefill_plan_check ok");
    return 0;
}
