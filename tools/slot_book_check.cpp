// Host check of the collector slots' bookkeeping (csrc/fs_slot_book.h): the buffer pool and the per-slot table of both kinds (scoring
// slots, hidden-state collectors), driven the way the engine drives them (take for an add that will be admitted, the first buffer put
// back when the second take fails, activate, refresh the counts, drop at release, end of session with adds still pending), with malloc /
// free standing in for the device allocator.
// Meant to run under the sanitizers:
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/slot_book_check.cpp -o slot_book_check && ./slot_book_check
// Every buffer is written end to end while it is live, so a pool that hands one out twice, frees one that is live, or computes the
// targets' offset wrongly shows up as a sanitizer report or a failed check; the process ends with every byte freed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>

#include "../fish-speech.rs_amd/csrc/fs_slot_book.h"

static int g_live_allocs = 0;
static void* book_alloc(size_t n) { ++g_live_allocs; return std::malloc(n); }
static void book_free(void* p) { --g_live_allocs; std::free(p); }
static void* null_alloc(size_t) { return nullptr; }

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "slot_book_check: %s failed at line %d\n", #c, __LINE__); std::exit(1); } } while (0)

// what the device does with a live entry.  Scoring (width = C + 1): targets read, records written; hidden rows (width = dim): rows written
static void touch(const fs::ScoreSlot& e, int C1, uint32_t tag) {
    uint32_t* t = const_cast<uint32_t*>(e.targets);
    for (int i = 0; i < e.cap * C1; ++i) t[i] = tag + (uint32_t)i;
    for (int i = 0; i < e.cap * fs::SCORE_REC_WORDS; ++i) e.rec[i] = (float)tag;
    for (int i = 0; i < e.cap * C1; ++i) CHECK(t[i] == tag + (uint32_t)i);  // (the records do not overlap the targets)
}
static void touch(const fs::HidSlot& e, int dim, uint32_t tag) {
    for (int i = 0; i < e.cap * dim; ++i) e.rows[i] = (float)tag;
}
static void check_layout(const fs::ScoreSlot& e, const fs::SlotBuf& b) { CHECK(e.rec == b.p && (const char*)e.targets == (const char*)b.p + (size_t)b.cap * 128); }
static void check_layout(const fs::HidSlot& e, const fs::SlotBuf& b) { CHECK(e.rows == b.p); }

template <typename E>
static void scenario(size_t row_bytes, int width) {
    using K = fs::SlotKind<E>;
    using Book = fs::SlotBook<E>;
    const int B = 4;
    {
        Book book(book_alloc, book_free);
        book.begin(B, row_bytes);
        CHECK(book.row_bytes() == row_bytes && book.live() == 0 && book.pooled() == 0 && book.in_hand() == 0);
        // a refused add: the buffer goes back and is the one the next add gets
        fs::SlotBuf a = book.take(12);
        CHECK(a.p && a.cap == 12 && book.in_hand() == 1);
        book.put(a);
        CHECK(book.pooled() == 1 && book.in_hand() == 0);
        book.put(a);  // (put back already: left alone)
        CHECK(book.pooled() == 1);
        fs::SlotBuf a2 = book.take(7);  // (the smallest that fits: the 12-row one)
        CHECK(a2.p == a.p && a2.cap == 12 && book.pooled() == 0);
        // admitted, polled while prefilling, activated, stepped, released
        book.admitted(1);
        CHECK(book.wanted(1) && !book.wanted(0) && K::buf(book.entry(1)) == nullptr);
        const E& e = book.activate(1, a2);
        CHECK(e.count == 0 && e.cap == 12 && book.live() == 1 && book.in_hand() == 0);
        check_layout(e, a2);
        touch(e, width, 1000u);
        bool threw = false;
        try { book.activate(1, a2); } catch (const std::exception&) { threw = true; }
        CHECK(threw && book.live() == 1);
        threw = false;
        try { book.activate(2, a2); } catch (const std::exception&) { threw = true; }  // (a live slot's buffer is not in hand)
        CHECK(threw && book.live() == 1 && K::buf(book.entry(2)) == nullptr);
        book.put(a2);  // (activated: left alone)
        CHECK(book.pooled() == 0 && book.live() == 1);
        std::vector<E> dev(B, E{});
        dev[1] = e; dev[1].count = 5;
        dev[2].count = 3;  // (an entry the host does not hold: ignored)
        book.refresh_counts(dev.data());
        CHECK(book.entry(1).count == 5 && book.entry(2).count == 0);
        dev[1].count = 13;  // (beyond the capacity: not taken)
        book.refresh_counts(dev.data());
        CHECK(book.entry(1).count == 5);
        std::vector<char> other(12 * row_bytes);
        dev[1] = K::entry(fs::SlotBuf{other.data(), 12}); dev[1].count = 7;  // (another buffer's pointer: not taken, and the host's own stays)
        book.refresh_counts(dev.data());
        CHECK(book.entry(1).count == 5 && K::buf(book.entry(1)) == a2.p);
        CHECK(book.drop(1) && !book.drop(1) && !book.wanted(1) && book.live() == 0 && book.pooled() == 1 && K::buf(book.entry(1)) == nullptr);
        // a re-admitted slot starts at row 0
        book.admitted(1);
        const E& e2 = book.activate(1, book.take(3));
        CHECK(e2.count == 0 && K::buf(e2) == a.p);
        // the pool never holds more than B buffers: the smallest goes first
        std::vector<fs::SlotBuf> held;
        for (int n : {1, 40, 2, 30, 5, 20}) held.push_back(book.take(n));
        CHECK(book.in_hand() == 6);
        for (const fs::SlotBuf& b : held) {
            touch(K::entry(b), width, 7u);
            book.put(b);
        }
        CHECK(book.pooled() == (size_t)B && book.in_hand() == 0);
        fs::SlotBuf smallest = book.take(1);  // (the 1- and 2-row buffers were freed: the 5-row one is the smallest left)
        CHECK(smallest.cap == 5);
        book.put(smallest);
        // session end with a live slot, a refused add, and two adds still queued or in flight: their buffers were never activated and
        // nobody hands them back -- end() reclaims them, once
        fs::SlotBuf refused = book.take(25);
        book.put(refused);
        const int allocs = g_live_allocs;
        fs::SlotBuf queued = book.take(50), flight = book.take(60);  // (larger than anything pooled: two new allocations)
        CHECK(g_live_allocs == allocs + 2 && book.in_hand() == 2 && queued.p != flight.p);
        touch(K::entry(queued), width, 8u);
        book.end();
        CHECK(book.live() == 0 && K::buf(book.entry(1)) == nullptr && !book.wanted(1) && book.in_hand() == 0 && book.pooled() == (size_t)B);
        CHECK(g_live_allocs == allocs - 1);  // (live + pool + in hand came to B + 3 buffers; the three smallest were freed, none twice)
        book.end();
        CHECK(book.pooled() == (size_t)B && g_live_allocs == allocs - 1);
        // a second session on the same handle reuses the pool: the two reclaimed buffers are the largest in it
        book.begin(B, row_bytes);
        const int before = g_live_allocs;
        fs::SlotBuf again = book.take(55);
        CHECK(g_live_allocs == before && again.p == flight.p && again.cap == 60);
        book.activate(0, again);
        // random traffic: no buffer is ever handed out twice
        std::mt19937 rng(12345);
        std::set<void*> out;
        std::vector<int> slot_live(B, 0);
        slot_live[0] = 1; out.insert(again.p);
        for (int it = 0; it < 2000; ++it) {
            const int b = (int)(rng() % B);
            if (slot_live[b]) {
                out.erase(K::buf(book.entry(b)));
                CHECK(book.drop(b));
                slot_live[b] = 0;
            } else {
                fs::SlotBuf nb = book.take(1 + (int)(rng() % 64));
                CHECK(out.insert(nb.p).second);
                if (rng() % 4 == 0) { out.erase(nb.p); book.put(nb); continue; }  // (refused add)
                book.admitted(b);
                touch(book.activate(b, nb), width, (uint32_t)it);
                slot_live[b] = 1;
            }
            int live = 0;
            for (int v : slot_live) live += v;
            CHECK(book.live() == live && book.pooled() <= (size_t)B && book.in_hand() == 0);
        }
        // the handle goes away with live slots, a filled pool, an add pending (its buffer in hand), and one buffer that was in hand and
        // has been put back: the destructor frees each of them once
        fs::SlotBuf pending = book.take(70), back = book.take(80);
        touch(K::entry(pending), width, 9u);
        book.put(back);
        CHECK(book.in_hand() == 1);
    }
    CHECK(g_live_allocs == 0);
    {
        Book book(null_alloc, book_free);
        book.begin(2, row_bytes);
        bool threw = false;
        try { (void)book.take(4); } catch (const std::exception&) { threw = true; }
        CHECK(threw && book.pooled() == 0 && book.live() == 0 && book.in_hand() == 0);
    }
}

// The engine's one admission path takes the buffers of a request that will be admitted, hidden rows first, records second; when the second
// take fails the first buffer goes back, and nothing is in hand in either book.  A request that needs both and gets both hands each to
// its book at activation.
static size_t g_alloc_budget = 0;  // allocations budget_alloc still grants
static void* budget_alloc(size_t n) { if (!g_alloc_budget) return nullptr; --g_alloc_budget; return book_alloc(n); }

static void admission(size_t hid_row_bytes, size_t sc_row_bytes, int dim, int C1) {
    {
        fs::SlotBook<fs::HidSlot> hid(budget_alloc, book_free);
        fs::SlotBook<fs::ScoreSlot> sc(budget_alloc, book_free);
        hid.begin(4, hid_row_bytes);
        sc.begin(4, sc_row_bytes);
        auto take_both = [&](int n_iter, fs::SlotBuf& h, fs::SlotBuf& s) {  // (step 4 of session_admit)
            h = hid.take(n_iter);
            try { s = sc.take(n_iter); } catch (...) { hid.put(h); throw; }
        };
        fs::SlotBuf h, s;
        g_alloc_budget = 1;  // the hidden-row buffer is granted, the record buffer is not
        bool threw = false;
        try { take_both(6, h, s); } catch (const std::exception&) { threw = true; }
        CHECK(threw && hid.in_hand() == 0 && sc.in_hand() == 0 && hid.pooled() == 1 && sc.pooled() == 0 && s.p == nullptr);
        hid.put(h);  // (put back already: left alone)
        CHECK(hid.pooled() == 1 && g_live_allocs == 1);
        g_alloc_budget = 0;  // the first take fails: nothing was taken, nothing to put back
        threw = false;
        try { take_both(9, h, s); } catch (const std::exception&) { threw = true; }
        CHECK(threw && hid.in_hand() == 0 && sc.in_hand() == 0 && hid.pooled() == 1);
        g_alloc_budget = 1;  // the same request again: the pooled row buffer serves it, the record buffer is new
        take_both(6, h, s);
        CHECK(hid.in_hand() == 1 && sc.in_hand() == 1 && hid.pooled() == 0 && g_live_allocs == 2 && g_alloc_budget == 0);
        hid.admitted(2); sc.admitted(2);
        touch(hid.activate(2, h), dim, 3u);
        touch(sc.activate(2, s), C1, 4u);
        CHECK(hid.in_hand() == 0 && sc.in_hand() == 0 && hid.live() == 1 && sc.live() == 1);
        // a request admitted but never activated (the session ends with it queued): both buffers are reclaimed by their books
        g_alloc_budget = 2;
        take_both(11, h, s);
        hid.admitted(3); sc.admitted(3);
        hid.end(); sc.end();
        CHECK(hid.in_hand() == 0 && sc.in_hand() == 0 && hid.live() == 0 && sc.live() == 0 && hid.pooled() == 2 && sc.pooled() == 2);
    }
    CHECK(g_live_allocs == 0);
}

// A handle's sessions need not agree on the row size: the score book's rows are longer in a FS_SESSION_ALTS session, by its N.  take()
// matches pooled buffers by their rows alone, so a buffer pooled under shorter rows must not serve a session with longer ones: begin()
// frees the pool when the row size changes (and keeps it when it does not).  The alternatives' blocks are written end to end behind the
// targets, so a buffer handed out too short is a sanitizer report.
static size_t g_last_alloc = 0;
static void* sized_alloc(size_t n) { g_last_alloc = n; return book_alloc(n); }
static void touch_alts(const fs::ScoreSlot& e, int C1, int n_alts) {
    touch(e, C1, 5u);
    uint32_t* idx = fs::score_alt_index(e, C1);
    float *lp = fs::score_alt_logprob(e, C1, n_alts), *ent = fs::score_alt_entropy(e, C1, n_alts);
    CHECK((const char*)idx == (const char*)e.rec + (size_t)e.cap * (128 + 4 * C1));
    for (int i = 0; i < e.cap * C1 * n_alts; ++i) { idx[i] = (uint32_t)i; lp[i] = -1.f; }
    for (int i = 0; i < e.cap * C1; ++i) ent[i] = 2.f;
    for (int i = 0; i < e.cap * C1 * n_alts; ++i) CHECK(idx[i] == (uint32_t)i);  // (the three blocks do not overlap)
    CHECK((const char*)(ent + (size_t)e.cap * C1) == (const char*)e.rec + (size_t)e.cap * (128 + 4 * C1 + fs::score_alts_bytes(C1, n_alts)));
}
static void row_size_change(int C1) {
    {
        fs::SlotBook<fs::ScoreSlot> book(sized_alloc, book_free);
        const size_t a = 128 + 4 * C1, b8 = a + fs::score_alts_bytes(C1, 8), b16 = a + fs::score_alts_bytes(C1, 16);
        CHECK(b8 == a + 9 * (8 * 8 + 4) && b16 > b8);
        book.begin(4, a);
        fs::SlotBuf s = book.take(12);
        CHECK(g_last_alloc == a * 12);
        book.put(s);
        CHECK(book.pooled() == 1 && g_live_allocs == 1);
        book.begin(4, a);  // (the same row size: the pool is kept, and serves the take)
        fs::SlotBuf s2 = book.take(12);
        CHECK(book.pooled() == 0 && s2.p == s.p && g_live_allocs == 1);
        book.put(s2);
        book.begin(4, b8);  // (longer rows: the pooled buffer is freed, the take is a fresh allocation of b8 * cap bytes)
        CHECK(book.pooled() == 0 && g_live_allocs == 0 && book.row_bytes() == b8);
        g_last_alloc = 0;
        fs::SlotBuf l = book.take(12);
        CHECK(l.p && l.cap == 12 && g_last_alloc == b8 * 12 && g_live_allocs == 1);
        book.admitted(0);
        touch_alts(book.activate(0, l), C1, 8);
        // the session ends with the slot live; another N, then a session without the flag: each starts with an empty pool
        book.begin(4, b16);
        CHECK(book.pooled() == 0 && g_live_allocs == 0);
        g_last_alloc = 0;
        fs::SlotBuf m = book.take(5);
        CHECK(g_last_alloc == b16 * 5);
        book.admitted(1);
        touch_alts(book.activate(1, m), C1, 16);
        book.begin(4, a);
        CHECK(book.pooled() == 0 && g_live_allocs == 0);
        touch(book.activate(2, book.take(5)), C1, 6u);
        CHECK(g_last_alloc == a * 5);
    }
    CHECK(g_live_allocs == 0);
}

int main() {
    const int C1 = 9, dim = 24;
    row_size_change(C1);
    scenario<fs::ScoreSlot>(128 + 4 * C1, C1);
    scenario<fs::HidSlot>(4 * dim, dim);
    admission(4 * dim, 128 + 4 * C1, dim, C1);
    std::puts("slot_book_check ok");
    return 0;
}
