// Host check of the KV page book (csrc/fs_kv_pages.h): the free list, the reference counts, the owners' page lists and the holds, driven the
// way the engine drives them (session begin: the scratch page; a prefix created, padded for its pass, trimmed, released; a slot admitted
// on a prefix -- full pages shared, private pages grown, the partly filled last page held until it has been copied --, grown, truncated,
// released; the end of a session with all of that still in place), in scripted scenarios and in a seeded random walk over a pool small
// enough that exhaustion, refusal and a full drain happen all the time.
// Every operation is also carried out on a deliberately naive model written out below -- a vector for the free list, an array of
// counts, plain lists, each rule spelled where it is used -- and after every operation the book's check() runs and the book is compared
// with the model page ID by page ID: the free list in its order, every count, every list, every hold.  Which page a request gets is part
// of the book's contract, not only how many.  An operation that throws must leave the book exactly as it was.
// Meant to run under the sanitizers:
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/kv_pages_check.cpp -o kv_pages_check && ./kv_pages_check
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "../fish-speech.rs_amd/csrc/fs_kv_pages.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "kv_pages_check: %s failed at line %d\n", #c, __LINE__); std::exit(1); } } while (0)

constexpr int PAGE = 64;
static int pages_of(int n_tokens) { return (n_tokens + PAGE - 1) / PAGE; }

// the naive model: loose members and hand-written rules
struct Naive {
    std::vector<int> free_pages, page_refs;
    std::vector<std::vector<int>> seq_pages, prefix_pages;
    std::vector<int> tail;  // per slot: the held last page of its prefix, -1 = none
    int scratch = -1, max_tokens = 0;
    void init(int n_pages, int n_seq, int max_tok) {
        max_tokens = max_tok;
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
        if (page_refs[(size_t)p] <= 0) throw std::runtime_error("KV page released twice");
        if (--page_refs[(size_t)p] == 0) free_pages.push_back(p);
    }
    void alloc_pages(std::vector<int>& pg, int n_tokens) {
        if (n_tokens > max_tokens) throw std::runtime_error("sequence longer than max_seq_len");
        const int need = pages_of(n_tokens);
        if ((int)free_pages.size() < need - (int)pg.size()) throw std::runtime_error("KV page pool exhausted");
        while ((int)pg.size() < need) pg.push_back(take_page());
    }
    void truncate(std::vector<int>& pg, int n_tokens) {
        const int keep = pages_of(n_tokens);
        while ((int)pg.size() > keep) { put_page(pg.back()); pg.pop_back(); }
    }
    void drop_pages(std::vector<int>& pg) {
        for (int p : pg) put_page(p);
        pg.clear();
    }
    void require_private(const std::vector<int>& pg, int pos0) const {
        for (size_t j = (size_t)(pos0 / PAGE); j < pg.size(); ++j)
            if (page_refs[(size_t)pg[j]] != 1) throw std::runtime_error("a session slot would write a shared KV page");
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
    std::vector<int> prefix_P;  // the session's prefixes: their lengths
    Pair(int n_pages_, int n_seq_, int max_tokens_) : n_pages(n_pages_), n_seq(n_seq_), max_tokens(max_tokens_) {
        book.init(n_pages, n_seq, PAGE, max_tokens);
        m.init(n_pages, n_seq, max_tokens);
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
        for (int i = 0; i < (int)m.prefix_pages.size(); ++i) CHECK(book.of(book.prefix_owner(i)) == m.prefix_pages[(size_t)i]);
    }
    // one operation on both sides: both succeed, or both throw the same text and the book stays bit for bit as it was
    template <typename F, typename G>
    std::string both(F on_book, G on_model) {
        const fs::KvPages before = book;
        std::string eb, em;
        try { on_book(); } catch (const std::exception& e) { eb = e.what(); CHECK(!eb.empty()); }
        try { on_model(); } catch (const std::exception& e) { em = e.what(); }
        CHECK(eb == em);
        if (!eb.empty()) CHECK(equal(book, before, n_pages));
        same();
        return eb;
    }
    std::vector<int>& model_list(int owner) { return owner < n_seq ? m.seq_pages[(size_t)owner] : m.prefix_pages[(size_t)(owner - n_seq)]; }

    std::string begin() {  // session_begin: the scratch page
        int got = -1;
        return both([&] { got = book.hold_new(); },
                    [&] {
                        if (m.free_pages.empty()) throw std::runtime_error("KV page pool exhausted");
                        m.scratch = m.take_page();
                        CHECK(got == m.scratch);
                    });
    }
    // growth, asked first: the query's cost is the model's arithmetic, and it fits exactly when the growth does not throw
    std::string grow(int owner, int n_tokens) {
        const int cost = std::max(0, pages_of(n_tokens) - (int)model_list(owner).size());
        fs::KvPages::Room r{false, cost};
        std::string asked;
        try { r = book.room(owner, n_tokens); } catch (const std::exception& x) { asked = x.what(); }
        CHECK(asked == (n_tokens > max_tokens ? "sequence longer than max_seq_len" : ""));
        if (asked.empty()) CHECK(r.cost == cost && r.fits == (cost <= (int)m.free_pages.size()));
        bool grew = false;
        const std::string e = both([&] { grew = book.grow(owner, n_tokens); }, [&] { m.alloc_pages(model_list(owner), n_tokens); });
        CHECK(e.empty() == r.fits);  // (a query that threw: the growth throws the same)
        if (!asked.empty()) CHECK(e == asked);
        if (e.empty()) CHECK(grew == (cost > 0));
        return e;
    }
    std::string truncate(int owner, int n_tokens) {
        return both([&] { book.truncate(owner, n_tokens); }, [&] { m.truncate(model_list(owner), n_tokens); });
    }
    // session_admit's page half: slot b on prefix `id` (-1: a plain add) keeps positions < end.  False: refused, the pool is short
    bool admit(int b, int id, int end, std::string* err = nullptr) {
        const int P = id >= 0 ? prefix_P[(size_t)id] : 0, nfull = P / PAGE;
        bool fits_book = false, fits_model = false;
        const fs::KvPages::Share sh{id >= 0 ? book.prefix_owner(id) : -1, nfull};
        const std::string e = both(
            [&] {
                fits_book = book.room(b, end, sh).fits;
                if (!fits_book) return;
                book.share(b, sh);  // (none of the three can fail after the query)
                book.grow(b, end);
                if (P % PAGE) CHECK(book.hold_page_of(sh.from, nfull) == book.of(sh.from)[(size_t)nfull]);
            },
            [&] {
                std::vector<int>& pg = m.seq_pages[(size_t)b];
                if (id >= 0 && !pg.empty()) throw std::runtime_error("a free slot still holds KV pages");
                fits_model = (int)m.free_pages.size() >= pages_of(end) - nfull - (int)pg.size();
                if (!fits_model) return;
                const std::vector<int>& px = id >= 0 ? m.prefix_pages[(size_t)id] : pg;
                for (int j = 0; j < nfull; ++j) { pg.push_back(px[(size_t)j]); ++m.page_refs[(size_t)px[(size_t)j]]; }
                m.alloc_pages(pg, end);
                if (P % PAGE) { m.tail[(size_t)b] = px[(size_t)nfull]; ++m.page_refs[(size_t)m.tail[(size_t)b]]; }
            });
        CHECK(fits_book == fits_model);
        if (err) *err = e; else CHECK(e.empty());
        return e.empty() && fits_book;
    }
    // the single-writer rule, asked like launch_tail_copies and activate_pending ask it
    void writable(int b, int pos0) {
        (void)both([&] { book.writable_from(b, pos0); }, [&] { m.require_private(m.seq_pages[(size_t)b], pos0); });
    }
    void joined(int b) {  // activation: the tail has been copied
        if (m.tail[(size_t)b] < 0) return;
        const int t = m.tail[(size_t)b];
        CHECK(both([&] { book.drop_hold(t); }, [&] { m.put_page(t); m.tail[(size_t)b] = -1; }).empty());
    }
    void release(int b) {
        joined(b);
        CHECK(truncate(b, 0).empty());
    }
    // a prefix of P positions whose pass pads it to pad_to; -1: refused
    int prefix_create(int P, int pad_to) {
        if (!book.room(fs::KvPages::kNewOwner, P).fits) {
            CHECK((int)m.free_pages.size() < pages_of(P));
            return -1;
        }
        CHECK((int)m.free_pages.size() >= pages_of(P));
        const int id = (int)prefix_P.size();
        CHECK(both([&] { CHECK(book.add_prefix() == book.prefix_owner(id)); book.grow(book.prefix_owner(id), P); },
                   [&] { m.prefix_pages.emplace_back(); for (int j = 0; j < pages_of(P); ++j) m.prefix_pages.back().push_back(m.take_page()); })
                  .empty());
        prefix_P.push_back(P);
        if (pad_to > P && book.room(book.prefix_owner(id), pad_to).fits) CHECK(grow(book.prefix_owner(id), pad_to).empty());  // (the pass's pad pages)
        return id;
    }
    void prefix_trim(int id) { CHECK(truncate(book.prefix_owner(id), prefix_P[(size_t)id]).empty()); }  // (activation: the pad pages go back)
    void prefix_drop(int id) {
        CHECK(both([&] { book.drop(book.prefix_owner(id)); }, [&] { m.drop_pages(m.prefix_pages[(size_t)id]); }).empty());
    }
    // session_end: the pending adds' holds first, then everything else in one call
    void end() {
        for (int b = 0; b < n_seq; ++b) joined(b);
        CHECK(both([&] { book.end_session(); },
                   [&] {
                       for (auto& pg : m.seq_pages) m.truncate(pg, 0);
                       for (auto& pg : m.prefix_pages) m.drop_pages(pg);
                       m.prefix_pages.clear();
                       if (m.scratch >= 0) m.put_page(m.scratch);
                       m.scratch = -1;
                   })
                  .empty());
        prefix_P.clear();
        CHECK(book.free_count() == n_pages && book.shared_count() == 0 && book.owners() == n_seq);
    }
};

// tests/test_session_prefix_gpu.py::test_page_accounting_is_exact on the book alone: k = 1, 2, 3 slots on a 100-token prefix, the six
// release orders of two slots and their prefix, the end of a session with a live prefix, a slot on it and a prefix still pending
static void accounting() {
    const int P = 100, Lb = 20, mnt = P + Lb + 40;
    const int n_iter = 1 + std::max(0, mnt - (P + Lb) + 1), end = P + Lb + n_iter - 1, priv = pages_of(end) - P / PAGE;
    Pair t(/*n_pages=*/32, /*n_seq=*/4, /*max_tokens=*/512);
    CHECK(t.begin().empty());
    const int free0 = t.book.free_count();
    CHECK(free0 == 31 && t.m.scratch == 0);  // (the pool starts as 31 .. 0 and is taken from the back)
    for (int k = 1; k <= 3; ++k) {
        const int id = t.prefix_create(P, 128);
        CHECK(id == k - 1);
        for (int b = 0; b < k; ++b) CHECK(t.admit(b, id, end));
        for (int b = 0; b < k; ++b) t.writable(b, P);
        t.prefix_trim(id);
        for (int b = 0; b < k; ++b) { t.joined(b); t.writable(b, P + Lb - 1); }
        CHECK(t.book.free_count() == free0 - pages_of(P) - k * priv && t.book.shared_count() == P / PAGE);
        for (int b = 0; b < k; ++b) t.release(b);
        t.prefix_drop(id);
        CHECK(t.book.free_count() == free0 && t.book.shared_count() == 0);
    }
    int order[3] = {0, 1, 2};  // slot a, slot b, the prefix
    do {
        const int id = t.prefix_create(P, P);
        CHECK(t.admit(0, id, end) && t.admit(1, id, end));
        t.prefix_trim(id);
        t.joined(0); t.joined(1);
        for (int what : order) {
            if (what == 2) t.prefix_drop(id);
            else t.release(what);
        }
        CHECK(t.book.free_count() == free0 && t.book.shared_count() == 0);
    } while (std::next_permutation(order, order + 3));
    const int id = t.prefix_create(P, P);
    CHECK(t.admit(0, id, end));
    t.prefix_trim(id);
    t.joined(0);
    CHECK(t.prefix_create(70, 192) >= 0);  // (still pending at the end: its pad pages are in its list)
    CHECK(t.admit(1, id, end));            // (and an add still queued: its hold on the prefix's last page is in place)
    t.end();
    CHECK(t.begin().empty() && t.book.free_count() == free0);
    t.end();
}

// refusals: each leaves the book bit for bit as it was (both() compares it with a copy taken before)
static void refusals() {
    Pair t(/*n_pages=*/6, /*n_seq=*/3, /*max_tokens=*/5 * PAGE);
    CHECK(t.begin().empty());
    CHECK(t.grow(0, 3 * PAGE).empty() && t.grow(0, 2 * PAGE).empty() && t.book.of(0).size() == 3);  // (the second one is no growth)
    CHECK(t.grow(1, 5 * PAGE + 1) == "sequence longer than max_seq_len");
    CHECK(t.grow(1, 3 * PAGE) == "KV page pool exhausted");  // needs 3, the pool has 2: none is taken
    CHECK(t.book.of(1).empty() && t.book.free_count() == 2);
    CHECK(t.grow(0, 5 * PAGE).empty() && t.book.free_count() == 0);
    CHECK(!t.book.room(1, 1).fits && t.book.room(1, 1).cost == 1 && t.book.room(1, 0).fits);
    CHECK(t.grow(1, 1) == "KV page pool exhausted");
    {  // taking from an empty pool is an error in every path: a hold, a new prefix, an admission
        const fs::KvPages before = t.book;
        std::string e;
        try { (void)t.book.hold_new(); } catch (const std::exception& x) { e = x.what(); }
        CHECK(e == "KV page pool exhausted" && equal(t.book, before, t.n_pages));
        CHECK(t.prefix_create(10, 10) == -1 && !t.admit(1, -1, 10));
    }
    {  // releasing twice: a hold that is not there (a page owned, a free page, no page at all), and a hold dropped a second time
        const int owned = t.book.of(0)[0];
        for (int p : {owned, -1, 6}) {
            const fs::KvPages before = t.book;
            std::string e;
            try { t.book.drop_hold(p); } catch (const std::exception& x) { e = x.what(); }
            CHECK(e == "KV page released twice" && equal(t.book, before, t.n_pages));
        }
        CHECK(t.truncate(0, 2 * PAGE).empty());
        const int h = t.book.hold_page_of(0, 1);
        t.book.drop_hold(h);
        std::string e;
        try { t.book.drop_hold(h); } catch (const std::exception& x) { e = x.what(); }
        CHECK(e == "KV page released twice");
        t.same();
    }
    // a slot that still holds pages is not shared into, and says so in the query already; a held page is not writable
    const int id = t.prefix_create(100, 100);
    CHECK(id == 0);
    std::string e;
    CHECK(!t.admit(0, id, 110, &e) && e == "a free slot still holds KV pages");
    CHECK(t.truncate(0, 0).empty() && t.admit(1, id, 110));
    const int tail = t.m.tail[1];
    t.m.tail[2] = t.book.hold_page_of(1, 1);  // (a second reference on slot 1's private page)
    ++t.m.page_refs[(size_t)t.m.tail[2]];
    t.same();
    t.writable(1, 100);  // both refuse
    t.writable(1, 0);
    t.joined(2);
    t.writable(1, 100);  // both agree again
    CHECK(tail == t.book.of(t.book.prefix_owner(id))[1]);
    t.end();
}

// the random walk: 8 slots, up to 3 prefixes per session, 24 pages of which a slot may want 6
static void walk(unsigned seed, int n_ops) {
    const int n_seq = 8, max_tokens = 6 * PAGE;
    Pair t(/*n_pages=*/24, n_seq, max_tokens);
    std::mt19937 rng(seed);
    auto pick = [&](int n) { return (int)(rng() % (unsigned)n); };
    std::vector<char> dropped;  // per prefix of the session
    int exhausted = 0, refused = 0, drained = 0, sessions = 0;
    bool open = false;
    for (int it = 0; it < n_ops; ++it) {
        if (!open) { CHECK(t.begin().empty()); open = true; dropped.clear(); ++sessions; }
        const int b = pick(n_seq), op = pick(100);
        if (op < 25) {  // grow a sequence (now and then beyond max_seq_len)
            const std::string e = t.grow(b, pick(max_tokens + 40));
            exhausted += e == "KV page pool exhausted";
        } else if (op < 40) {  // admit to a slot, on a prefix when there is one (a slot that is not empty: the error)
            int id = t.prefix_P.empty() ? -1 : pick((int)t.prefix_P.size() + 1) - 1;
            if (id >= 0 && dropped[(size_t)id]) id = -1;
            if (t.m.tail[(size_t)b] >= 0) { t.joined(b); continue; }
            const int P = id >= 0 ? t.prefix_P[(size_t)id] : 0;
            std::string e;
            if (!t.admit(b, id, std::min(max_tokens, P + 1 + pick(max_tokens)), &e)) refused += e.empty();
            else t.writable(b, P);
        } else if (op < 50) {
            t.joined(b);
            t.writable(b, pick(max_tokens));
        } else if (op < 65) {
            if (pick(2)) t.release(b);
            else CHECK(t.truncate(b, pick(max_tokens)).empty());
        } else if (op < 75) {  // a prefix, padded for its pass
            if (t.prefix_P.size() < 3) {
                const int P = 1 + pick(3 * PAGE);
                if (t.prefix_create(P, P + pick(2 * PAGE)) < 0) ++refused;
                else dropped.push_back(0);
            }
        } else if (op < 85) {
            if (!t.prefix_P.empty()) t.prefix_trim(pick((int)t.prefix_P.size()));
        } else if (op < 93) {
            if (!t.prefix_P.empty()) { const int id = pick((int)t.prefix_P.size()); t.prefix_drop(id); dropped[(size_t)id] = 1; }
        } else if (op < 96) {  // a group's cumulative query: what the first member was promised counts against the second
            const int c = pick(n_seq), n1 = pick(max_tokens), n2 = pick(max_tokens);
            const fs::KvPages::Room r1 = t.book.room(b, n1), r2 = t.book.room(c, n2, {}, r1.cost);
            CHECK(r2.fits == (r1.cost + r2.cost <= t.book.free_count()));
            if (b != c && r1.fits && r2.fits) CHECK(t.grow(b, n1).empty() && t.grow(c, n2).empty());
        } else if (op < 98) {  // a hold that is not there
            const int p = pick(24);
            if (t.book.holds(p) == 0) {
                const fs::KvPages before = t.book;
                std::string e;
                try { t.book.drop_hold(p); } catch (const std::exception& x) { e = x.what(); }
                CHECK(e == "KV page released twice" && equal(t.book, before, t.n_pages));
            }
        } else {
            t.end();
            open = false;
        }
        drained += t.book.free_count() == 0;
    }
    t.end();
    // (the pool is small on purpose: each of these happens hundreds of times)
    CHECK(exhausted > 100 && refused > 100 && drained > 100 && sessions > 100);
}

int main() {
    accounting();
    refusals();
    walk(20240601u, 30000);
    walk(7u, 10000);
    std::puts("kv_pages_check ok");
    return 0;
}
