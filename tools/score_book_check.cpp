// Host check of the scoring slots' bookkeeping (csrc/fs_score_book.h): the buffer pool and the per-slot table, driven the way the engine
// drives them (take before the add, put back on a refused add, activate, refresh the counts, drop at release, end of session), with
// malloc / free standing in for the device allocator.  Meant to run under the sanitizers:
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/score_book_check.cpp -o score_book_check && ./score_book_check
// Every buffer is written end to end while it is live, so a pool that hands one out twice, frees one that is live, or computes the
// targets' offset wrongly shows up as a sanitizer report or a failed check; the process ends with every byte freed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>

#include "../fish-speech.rs_amd/csrc/fs_score_book.h"

static int g_live_allocs = 0;
static void* book_alloc(size_t n) { ++g_live_allocs; return std::malloc(n); }
static void book_free(void* p) { --g_live_allocs; std::free(p); }
static void* null_alloc(size_t) { return nullptr; }

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "score_book_check: %s failed at line %d\n", #c, __LINE__); std::exit(1); } } while (0)

// what the device does with a live entry: targets read, records written, count bumped
static void touch(const fs::ScoreSlot& e, int C1, uint32_t tag) {
    uint32_t* t = const_cast<uint32_t*>(e.targets);
    for (int i = 0; i < e.cap * C1; ++i) t[i] = tag + (uint32_t)i;
    for (int i = 0; i < e.cap * fs::SCORE_REC_WORDS; ++i) e.rec[i] = (float)tag;
    for (int i = 0; i < e.cap * C1; ++i) CHECK(t[i] == tag + (uint32_t)i);  // (the records do not overlap the targets)
}

int main() {
    const int B = 4, C1 = 9;
    {
        fs::ScoreBook book(book_alloc, book_free);
        book.begin(B, C1);
        CHECK(book.row_bytes() == 128 + 4 * C1 && book.live() == 0 && book.pooled() == 0);
        // a refused add: the buffer goes back and is the one the next add gets
        fs::ScoreBuf a = book.take(12);
        CHECK(a.p && a.cap == 12);
        book.put(a);
        CHECK(book.pooled() == 1);
        fs::ScoreBuf a2 = book.take(7);  // (the smallest that fits: the 12-row one)
        CHECK(a2.p == a.p && a2.cap == 12 && book.pooled() == 0);
        // admitted, polled while prefilling, activated, stepped, released
        book.admitted(1);
        CHECK(book.wanted(1) && !book.wanted(0) && book.entry(1).rec == nullptr);
        const fs::ScoreSlot& e = book.activate(1, a2);
        CHECK(e.count == 0 && e.cap == 12 && e.rec == a2.p && book.live() == 1);
        CHECK((const char*)e.targets == (const char*)a2.p + (size_t)12 * 128);
        touch(e, C1, 1000u);
        bool threw = false;
        try { book.activate(1, a2); } catch (const std::exception&) { threw = true; }
        CHECK(threw && book.live() == 1);
        std::vector<fs::ScoreSlot> dev(B, fs::ScoreSlot{nullptr, nullptr, 0, 0});
        dev[1] = e; dev[1].count = 5;
        dev[2].count = 3;  // (an entry the host does not hold: ignored)
        book.refresh_counts(dev.data());
        CHECK(book.entry(1).count == 5 && book.entry(2).count == 0);
        dev[1].count = 13;  // (beyond the capacity: not taken)
        book.refresh_counts(dev.data());
        CHECK(book.entry(1).count == 5);
        CHECK(book.drop(1) && !book.drop(1) && !book.wanted(1) && book.live() == 0 && book.pooled() == 1 && book.entry(1).rec == nullptr);
        // a re-admitted slot starts at row 0
        book.admitted(1);
        const fs::ScoreSlot& e2 = book.activate(1, book.take(3));
        CHECK(e2.count == 0 && e2.rec == a.p);
        // the pool never holds more than B buffers: the smallest goes first
        std::vector<fs::ScoreBuf> held;
        for (int n : {1, 40, 2, 30, 5, 20}) held.push_back(book.take(n));
        for (const fs::ScoreBuf& b : held) {
            fs::ScoreSlot s{fs::ScoreBook::targets_of(b), fs::ScoreBook::rec_of(b), 0, b.cap};
            touch(s, C1, 7u);
            book.put(b);
        }
        CHECK(book.pooled() == (size_t)B);
        fs::ScoreBuf smallest = book.take(1);  // (the 1- and 2-row buffers were freed: the 5-row one is the smallest left)
        CHECK(smallest.cap == 5);
        book.put(smallest);
        // session end with a live slot and a queued add whose buffer was never activated
        fs::ScoreBuf queued = book.take(25);
        book.put(queued);
        book.end();
        CHECK(book.live() == 0 && book.entry(1).rec == nullptr && !book.wanted(1));
        // a second session on the same handle reuses the pool
        book.begin(B, C1);
        const int before = g_live_allocs;
        fs::ScoreBuf again = book.take(10);
        CHECK(g_live_allocs == before);
        book.activate(0, again);
        // random traffic: no buffer is ever handed out twice
        std::mt19937 rng(12345);
        std::set<void*> out;
        std::vector<int> slot_live(B, 0);
        slot_live[0] = 1; out.insert(again.p);
        for (int it = 0; it < 2000; ++it) {
            const int b = (int)(rng() % B);
            if (slot_live[b]) {
                out.erase(book.entry(b).rec);
                CHECK(book.drop(b));
                slot_live[b] = 0;
            } else {
                fs::ScoreBuf nb = book.take(1 + (int)(rng() % 64));
                CHECK(out.insert(nb.p).second);
                if (rng() % 4 == 0) { out.erase(nb.p); book.put(nb); continue; }  // (refused add)
                book.admitted(b);
                touch(book.activate(b, nb), C1, (uint32_t)it);
                slot_live[b] = 1;
            }
            int live = 0;
            for (int v : slot_live) live += v;
            CHECK(book.live() == live && book.pooled() <= (size_t)B);
        }
        // the handle goes away with live slots and a filled pool: the destructor frees both
    }
    CHECK(g_live_allocs == 0);
    {
        fs::ScoreBook book(null_alloc, book_free);
        book.begin(2, C1);
        bool threw = false;
        try { (void)book.take(4); } catch (const std::exception&) { threw = true; }
        CHECK(threw && book.pooled() == 0 && book.live() == 0);
    }
    std::puts("score_book_check ok");
    return 0;
}
