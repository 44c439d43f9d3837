// Host check of the KV page book (csrc/fs_kv_pages.h) under the operations that make a prefix out of a slot's history
// (fs_lm_session_prefix_from_slot): the new prefix owner SHARES the leading P / 64 pages of a sequence-row owner -- pages that may
// themselves be shared from an earlier prefix -- and GROWS by one page of its own when P is not page-aligned; slots join the promoted prefix
// like any other (full pages shared, the partly filled last page held until copied); source, joiners and prefix are released in every
// order; and prefixes are promoted from slots that sit on prefixes promoted from slots, and so on.
// As in tools/kv_pages_check.cpp every operation is also carried out on a deliberately naive model (a vector for the free list, an array
// of counts, plain lists), and after every operation the book's check() runs and the book is compared with the model page ID by page ID:
// the free list in its order, every count, every list, every hold.  A refused promotion must leave the book exactly as it was.
// Meant to run under the sanitizers as a stand-alone host program:
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/kv_history_check.cpp -o kv_history_check && ./kv_history_check
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "../fish-speech.rs_amd/csrc/fs_kv_pages.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "kv_history_check: %s failed at line %d\n", #c, __LINE__); std::exit(1); } } while (0)

constexpr int PAGE = 64;
static int pages_of(int n_tokens) { return (n_tokens + PAGE - 1) / PAGE; }

// the naive model
struct Naive {
    std::vector<int> free_pages, page_refs;
    std::vector<std::vector<int>> seq_pages, prefix_pages;
    std::vector<int> tail;  // per slot: the held last page of the prefix it joins, -1 = none
    int scratch = -1;
    void init(int n_pages, int n_seq) {
        free_pages.clear();
        for (int p = n_pages - 1; p >= 0; --p) free_pages.push_back(p);
        page_refs.assign((size_t)n_pages, 0);
        seq_pages.assign((size_t)n_seq, {});
        prefix_pages.clear();
        tail.assign((size_t)n_seq, -1);
        scratch = -1;
    }
    int take_page() {  // (every caller has looked at the free list first)
        const int p = free_pages.back();
        free_pages.pop_back();
        page_refs[(size_t)p] = 1;
        return p;
    }
    void put_page(int p) {
        CHECK(page_refs[(size_t)p] > 0);
        if (--page_refs[(size_t)p] == 0) free_pages.push_back(p);
    }
    bool is_private(const std::vector<int>& pg, int pos0) const {
        for (size_t j = (size_t)(pos0 / PAGE); j < pg.size(); ++j)
            if (page_refs[(size_t)pg[j]] != 1) return false;
        return true;
    }
    int held(int p) const { return (int)std::count(tail.begin(), tail.end(), p) + (scratch == p ? 1 : 0); }
};

static bool equal(const fs::KvPages& a, const fs::KvPages& b, int n_pages) {
    if (a.free_list() != b.free_list() || a.owners() != b.owners()) return false;
    for (int o = 0; o < a.owners(); ++o) if (a.of(o) != b.of(o)) return false;
    for (int p = 0; p < n_pages; ++p) if (a.refs(p) != b.refs(p) || a.holds(p) != b.holds(p)) return false;
    return true;
}

// the book and the model, moved together
struct Pair {
    fs::KvPages book;
    Naive m;
    int n_pages, n_seq, max_tokens;
    std::vector<int> prefix_P;   // the session's prefixes: their lengths
    std::vector<int> slot_end;   // per slot: the positions its pages hold (0: free)
    std::vector<int> slot_T;     // per slot: the history it had at its last promotion (a slot's history only grows; a joiner starts at P)
    Pair(int n_pages_, int n_seq_, int max_tokens_) : n_pages(n_pages_), n_seq(n_seq_), max_tokens(max_tokens_) {
        book.init(n_pages, n_seq, PAGE, max_tokens);
        m.init(n_pages, n_seq);
        slot_end.assign((size_t)n_seq, 0);
        slot_T.assign((size_t)n_seq, 0);
        same();
    }
    void same() const {
        book.check();
        CHECK(book.free_list() == m.free_pages && book.free_count() == (int)m.free_pages.size());
        CHECK(book.owners() == n_seq + (int)m.prefix_pages.size());
        int shared = 0;
        for (int p = 0; p < n_pages; ++p) {
            CHECK(book.refs(p) == m.page_refs[(size_t)p] && book.holds(p) == m.held(p));
            shared += m.page_refs[(size_t)p] > 1;
        }
        CHECK(book.shared_count() == shared);
        for (int b = 0; b < n_seq; ++b) CHECK(book.of(b) == m.seq_pages[(size_t)b] && book.intact(b));
        for (int i = 0; i < (int)m.prefix_pages.size(); ++i)
            CHECK(book.of(book.prefix_owner(i)) == m.prefix_pages[(size_t)i] && book.intact(book.prefix_owner(i)));
    }
    void begin() {  // session_begin: the scratch page
        CHECK(!m.free_pages.empty());
        const int got = book.hold_new();
        m.scratch = m.take_page();
        CHECK(got == m.scratch);
        same();
    }
    // session_admit's page half: slot b (free) on prefix `id` (-1: a plain add) keeps positions < end.  False: refused, nothing changed
    bool admit(int b, int id, int end) {
        CHECK(m.seq_pages[(size_t)b].empty() && slot_end[(size_t)b] == 0);
        const int P = id >= 0 ? prefix_P[(size_t)id] : 0, nfull = P / PAGE;
        CHECK(end > P && end <= max_tokens);
        const fs::KvPages before = book;
        const fs::KvPages::Share sh{id >= 0 ? book.prefix_owner(id) : -1, nfull};
        const bool fits = book.room(b, end, sh).fits;
        CHECK(fits == ((int)m.free_pages.size() >= pages_of(end) - nfull));
        if (!fits) { CHECK(equal(book, before, n_pages)); same(); return false; }
        book.share(b, sh);
        book.grow(b, end);
        if (P % PAGE) CHECK(book.hold_page_of(sh.from, nfull) == book.of(sh.from)[(size_t)nfull]);
        std::vector<int>& pg = m.seq_pages[(size_t)b];
        if (id >= 0) {
            const std::vector<int>& px = m.prefix_pages[(size_t)id];
            for (int j = 0; j < nfull; ++j) { pg.push_back(px[(size_t)j]); ++m.page_refs[(size_t)px[(size_t)j]]; }
            if (P % PAGE) { m.tail[(size_t)b] = px[(size_t)nfull]; ++m.page_refs[(size_t)m.tail[(size_t)b]]; }
        }
        while ((int)pg.size() < pages_of(end)) pg.push_back(m.take_page());
        slot_end[(size_t)b] = end;
        slot_T[(size_t)b] = P;
        same();
        writable(b, P, true);  // (its body's prefill and its decode steps write from P on)
        return true;
    }
    // the single-writer rule: the book throws exactly when the model finds a shared page from pos0's on
    void writable(int b, int pos0, bool expect) {
        bool ok = true;
        try { book.writable_from(b, pos0); } catch (const std::exception& e) { ok = false; CHECK(std::string(e.what()) == "a session slot would write a shared KV page"); }
        CHECK(ok == m.is_private(m.seq_pages[(size_t)b], pos0) && ok == expect);
    }
    void joined(int b) {  // activation: the tail has been copied
        const int t = m.tail[(size_t)b];
        if (t < 0) return;
        book.drop_hold(t);
        m.put_page(t);
        m.tail[(size_t)b] = -1;
        same();
    }
    void release(int b) {  // session_release: a slot is activated first, then its pages go last-first
        joined(b);
        book.truncate(b, 0);
        std::vector<int>& pg = m.seq_pages[(size_t)b];
        while (!pg.empty()) { m.put_page(pg.back()); pg.pop_back(); }
        slot_end[(size_t)b] = 0;
        same();
    }
    // fs_lm_session_prefix_from_slot's page half: a prefix of the first P positions of slot b, whose history has T >= P positions.
    // -1: refused (the one page a cut inside a page needs is not free), the book bit for bit as it was
    int promote(int b, int P, int T) {
        CHECK(1 <= P && P <= T && slot_T[(size_t)b] <= T && T <= slot_end[(size_t)b] && P < max_tokens);
        slot_T[(size_t)b] = T;
        joined(b);  // (a slot still prefilling is activated first)
        const int nfull = P / PAGE;
        const fs::KvPages before = book;
        const fs::KvPages::Share sh{b, nfull};
        const fs::KvPages::Room r = book.room(fs::KvPages::kNewOwner, P, sh);
        CHECK(r.cost == (P % PAGE ? 1 : 0) && r.fits == (r.cost <= (int)m.free_pages.size()));
        if (!r.fits) { CHECK(equal(book, before, n_pages)); same(); return -1; }
        const int id = (int)prefix_P.size(), owner = book.add_prefix();
        CHECK(owner == book.prefix_owner(id));
        book.share(owner, sh);
        CHECK(book.grow(owner, P) == (P % PAGE != 0));
        m.prefix_pages.emplace_back();
        std::vector<int>& px = m.prefix_pages.back();
        const std::vector<int>& src = m.seq_pages[(size_t)b];
        for (int j = 0; j < nfull; ++j) { px.push_back(src[(size_t)j]); ++m.page_refs[(size_t)src[(size_t)j]]; }
        if (P % PAGE) {
            const int top = m.free_pages.back();  // (the documented order: the page at the back of the pool)
            px.push_back(m.take_page());
            CHECK(book.of(owner).back() == top && book.refs(top) == 1);
        }
        prefix_P.push_back(P);
        same();
        CHECK((int)book.of(owner).size() == pages_of(P));
        writable(b, T, true);  // everything from page T / 64 on is still the slot's alone: its next write, or its frozen one, goes there
        if (nfull > 0) writable(b, 0, false);  // (a write INTO the shared part is refused)
        return id;
    }
    void prefix_drop(int id) {
        book.drop(book.prefix_owner(id));
        std::vector<int>& pg = m.prefix_pages[(size_t)id];
        for (int p : pg) m.put_page(p);
        pg.clear();
        same();
    }
    void end() {  // session_end: the pending adds' holds first, then everything else in one call
        for (int b = 0; b < n_seq; ++b) joined(b);
        book.end_session();
        for (auto& pg : m.seq_pages) while (!pg.empty()) { m.put_page(pg.back()); pg.pop_back(); }
        for (auto& pg : m.prefix_pages) { for (int p : pg) m.put_page(p); pg.clear(); }
        m.prefix_pages.clear();
        if (m.scratch >= 0) m.put_page(m.scratch);
        m.scratch = -1;
        prefix_P.clear();
        std::fill(slot_end.begin(), slot_end.end(), 0);
        same();
        CHECK(book.free_count() == n_pages && book.shared_count() == 0 && book.owners() == n_seq);
    }
};

// tests/test_session_history_gpu.py's page accounting on the book alone: a cut inside a page, a page-aligned cut, a source that sits on
// another prefix, source / joiner / prefix released in all six orders, the refused promotion
static void accounting() {
    Pair t(/*n_pages=*/16, /*n_seq=*/4, /*max_tokens=*/256);
    t.begin();
    const int free0 = t.book.free_count();
    CHECK(free0 == 15 && t.m.scratch == 0);
    // P % 64 != 0: one page taken (the back of the pool), one page shared
    CHECK(t.admit(0, -1, 140));  // pages 1, 2, 3
    CHECK(t.book.of(0) == std::vector<int>({1, 2, 3}));
    int id = t.promote(0, 100, 100);
    CHECK(id == 0 && t.book.of(t.book.prefix_owner(id)) == std::vector<int>({1, 4}));
    CHECK(t.book.free_count() == free0 - 4 && t.book.shared_count() == 1);
    t.release(0);
    t.prefix_drop(id);
    CHECK(t.book.free_count() == free0 && t.book.shared_count() == 0);
    // P % 64 == 0: no page taken, also from a drained pool; the slot's write target (page T / 64) stays its own
    CHECK(t.admit(0, -1, 192) && t.admit(1, -1, 256) && t.admit(2, -1, 256) && t.admit(3, -1, 256));
    CHECK(t.book.free_count() == 0);
    id = t.promote(0, 128, 128);
    CHECK(id == 1 && t.book.free_count() == 0 && t.book.shared_count() == 2);
    CHECK(t.book.of(t.book.prefix_owner(id)) == std::vector<int>(t.book.of(0).begin(), t.book.of(0).begin() + 2));
    t.writable(0, 127, false);  // (a write below T would hit a shared page: refused)
    // the refused promotion: a cut inside a page needs the one page the pool does not have
    CHECK(t.promote(0, 130, 130) == -1 && t.promote(1, 1, 200) == -1);
    CHECK(t.promote(1, 64, 200) == 2);  // (aligned: never refused for room)
    t.end();
    // a source that sits on another prefix: the pages it shares simply gain a reference
    t.begin();
    CHECK(t.admit(0, -1, 200));
    const int base = t.promote(0, 150, 160);  // 2 shared + its own tail
    CHECK(base == 0);
    CHECK(t.admit(1, base, 256));  // joins: 2 shared, a hold on the tail, private pages 2 and 3
    t.joined(1);
    const int p0 = t.book.of(0)[0];
    CHECK(t.book.refs(p0) == 3);
    const int next = t.promote(1, 200, 210);  // 3 full pages: two of them the first source's, one slot 1's own
    CHECK(next == 1 && t.book.refs(p0) == 4 && t.book.refs(t.book.of(1)[2]) == 2);
    CHECK(t.book.of(t.book.prefix_owner(next))[0] == p0);
    t.release(0); t.prefix_drop(base);
    CHECK(t.book.refs(p0) == 2);
    t.release(1);
    CHECK(t.book.refs(p0) == 1 && t.book.shared_count() == 0);
    t.prefix_drop(next);
    CHECK(t.book.free_count() == free0);
    // source, joiner, prefix in all six release orders, for an aligned and an unaligned cut
    for (int P : {64, 100, 128}) {
        int order[3] = {0, 1, 2};
        do {
            const int n0 = (int)t.prefix_P.size();
            CHECK(t.admit(0, -1, 180));
            const int pid = t.promote(0, P, 128);
            CHECK(pid == n0);
            CHECK(t.admit(1, pid, 200));
            CHECK(t.book.free_count() == free0 - 3 - (P % PAGE ? 1 : 0) - (pages_of(200) - P / PAGE));
            CHECK(t.book.shared_count() == P / PAGE + (P % PAGE ? 1 : 0));  // (the held tail counts while the copy is pending)
            t.joined(1);
            CHECK(t.book.shared_count() == P / PAGE);
            for (int what : order) {
                if (what == 2) t.prefix_drop(pid);
                else t.release(what);
            }
            CHECK(t.book.free_count() == free0 && t.book.shared_count() == 0);
        } while (std::next_permutation(order, order + 3));
    }
    t.end();
}

// chains: turn k + 1 joins the prefix promoted from turn k's slot; the prefix reference is dropped once the add is queued
// (Session.continue_from), the old slot once the new one runs.  The conditioning pages are shared all the way down.
static void chains() {
    Pair t(/*n_pages=*/28, /*n_seq=*/3, /*max_tokens=*/1024);
    t.begin();
    const int free0 = t.book.free_count();
    CHECK(t.admit(0, -1, 90));
    const int first = t.book.of(0)[0];
    int cur = 0, T = 80;
    for (int turn = 1; turn <= 9; ++turn) {
        const int pid = t.promote(cur, T, T);
        CHECK(pid == turn - 1);
        const int nxt = (cur + 1) % 3, end = T + 30 + 60;
        CHECK(t.admit(nxt, pid, end));
        t.prefix_drop(pid);  // (the joiner's hold keeps the tail page alive until it has been copied)
        if (T % PAGE) CHECK(t.book.refs(t.m.tail[(size_t)nxt]) == 1);
        t.joined(nxt);
        t.release(cur);
        CHECK(t.book.of(nxt)[0] == first && t.book.refs(first) == 1);
        CHECK(t.book.free_count() == free0 - pages_of(end));  // nothing leaks from turn to turn
        cur = nxt;
        T = end - (turn % 3 == 0 ? (end % PAGE) : 7);  // (every third turn ends page-aligned)
    }
    // ... and a chain whose links are all kept: prefix from a slot on a prefix from a slot on a prefix
    std::vector<int> kept;
    for (int b = 0; b < 3; ++b) if (b != cur) CHECK(t.m.seq_pages[(size_t)b].empty());
    int src = cur, Tk = t.slot_end[(size_t)cur] - 5;
    for (int k = 0; k < 2; ++k) {
        const int pid = t.promote(src, Tk, Tk);
        CHECK(pid >= 0);
        kept.push_back(pid);
        const int nxt = (src + 1) % 3;
        CHECK(t.admit(nxt, pid, Tk + 70));
        t.joined(nxt);
        src = nxt; Tk += 65;
    }
    CHECK(t.book.refs(first) == 5);  // three slots and two prefixes
    t.end();
}

// the random walk: 6 slots, a pool of 12 pages of which a slot may want 5, prefixes promoted from whatever is live
static void walk(unsigned seed, int n_ops) {
    const int n_seq = 6, max_tokens = 5 * PAGE;
    Pair t(/*n_pages=*/12, n_seq, max_tokens);
    std::mt19937 rng(seed);
    auto pick = [&](int n) { return (int)(rng() % (unsigned)n); };
    std::vector<char> dropped;
    int promoted = 0, refused = 0, aligned = 0, chained = 0, admits_refused = 0, sessions = 0;
    std::vector<int> depth(n_seq, 0), prefix_depth;
    bool open = false;
    for (int it = 0; it < n_ops; ++it) {
        if (!open) { t.begin(); open = true; dropped.clear(); prefix_depth.clear(); std::fill(depth.begin(), depth.end(), 0); ++sessions; }
        const int b = pick(n_seq), op = pick(100);
        const bool live = t.slot_end[(size_t)b] > 0;
        if (op < 30) {  // admit to a free slot, on a live prefix when there is one
            if (live) continue;
            int id = t.prefix_P.empty() ? -1 : pick((int)t.prefix_P.size() + 1) - 1;
            if (id >= 0 && dropped[(size_t)id]) id = -1;
            const int P = id >= 0 ? t.prefix_P[(size_t)id] : 0;
            const int end = std::min(max_tokens, P + 1 + pick(max_tokens));
            if (!t.admit(b, id, end)) ++admits_refused;
            else depth[(size_t)b] = id >= 0 ? prefix_depth[(size_t)id] + 1 : 0;
        } else if (op < 60) {  // promote a live slot at a random history length and cut (every fourth cut page-aligned)
            if (!live || t.prefix_P.size() >= 24) continue;
            const int T = std::max(1, t.slot_T[(size_t)b] + pick(t.slot_end[(size_t)b] - t.slot_T[(size_t)b] + 1));
            int P = 1 + pick(T);
            if (pick(4) == 0 && T >= PAGE) P = PAGE * (1 + pick(T / PAGE));
            if (P >= max_tokens) continue;
            const int id = t.promote(b, P, T);
            if (id < 0) { ++refused; continue; }
            dropped.push_back(0);
            prefix_depth.push_back(depth[(size_t)b]);
            ++promoted; aligned += P % PAGE == 0; chained += depth[(size_t)b] > 0;
        } else if (op < 70) {
            t.joined(b);
        } else if (op < 85) {
            if (live) { t.release(b); depth[(size_t)b] = 0; }
        } else if (op < 99) {
            if (!t.prefix_P.empty()) {
                const int id = pick((int)t.prefix_P.size());
                if (!dropped[(size_t)id]) { t.prefix_drop(id); dropped[(size_t)id] = 1; }
            }
        } else {
            t.end();
            open = false;
        }
    }
    t.end();
    // (the pool is short on purpose: each of these happens all the time)
    std::printf("walk %u: promoted %d (aligned %d, chained %d), refused %d, admits refused %d, sessions %d\n", seed, promoted, aligned, chained, refused, admits_refused, sessions);
    CHECK(promoted > 500 && refused > 50 && aligned > 100 && chained > 100 && admits_refused > 100 && sessions > 50);
}

int main() {
    accounting();
    chains();
    walk(20240917u, 40000);
    walk(11u, 15000);
    std::puts("kv_history_check ok");
    return 0;
}
