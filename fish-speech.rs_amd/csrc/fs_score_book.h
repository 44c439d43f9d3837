// Host-side bookkeeping of the scoring slots of a FS_SESSION_SCORE session (fishrt.h: fs_lm_session_add_scored): the per-slot table the
// step's k_score_slots nodes read (host mirror; the engine copies entries to the device), and the per-handle pool the slots' buffers come
// from.  Plain C++ -- no HIP in here, the allocator is handed in -- so that a host program can run it under a sanitizer
// (tools/score_book_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <vector>

namespace fs {

// One entry per slot: rec == null -> the slot is not scored; else iteration `count` of the slot is forced to targets[count][0 .. C]
// (slow token, c0..c7) and leaves the 32-word record rec[count]: [0..8] logprob of the target per decision, [9..17] logprob of the
// maximum, [18..26] the last maximal index (u32 bits), [27] logprob of <|im_end|> at the slow decision (-inf when masked), [28..31] zero.
struct ScoreSlot {
    const uint32_t* targets;  // [cap][C + 1]
    float* rec;               // [cap][32]
    int count, cap;
};
constexpr int SCORE_REC_WORDS = 32;

// one allocation per scoring slot: the records [cap][32] f32 first (128-byte rows), the targets [cap][C + 1] u32 behind them
struct ScoreBuf {
    void* p = nullptr;
    int cap = 0;
};

class ScoreBook {
public:
    using AllocFn = void* (*)(size_t);
    using FreeFn = void (*)(void*);
    ScoreBook(AllocFn a, FreeFn f) : alloc_(a), free_(f) {}
    ScoreBook(const ScoreBook&) = delete;
    ScoreBook& operator=(const ScoreBook&) = delete;
    ~ScoreBook() {
        for (ScoreSlot& e : tab_) if (e.rec) free_(e.rec);
        for (ScoreBuf& b : pool_) free_(b.p);
    }
    // session_begin: B slots of C + 1 decisions, nothing scored; buffers a previous session left live go back to the pool
    void begin(int B, int C1) {
        end();
        B_ = B; C1_ = C1;
        tab_.assign((size_t)B, ScoreSlot{nullptr, nullptr, 0, 0});
        want_.assign((size_t)B, 0);
    }
    size_t row_bytes() const { return sizeof(float) * SCORE_REC_WORDS + sizeof(uint32_t) * (size_t)C1_; }
    // a free buffer of >= n_rows rows (the smallest that fits), else a new one; throws when the allocator returns null
    ScoreBuf take(int n_rows) {
        if (n_rows < 1) throw std::runtime_error("score buffer: no rows");
        int best = -1;
        for (int i = 0; i < (int)pool_.size(); ++i)
            if (pool_[i].cap >= n_rows && (best < 0 || pool_[i].cap < pool_[best].cap)) best = i;
        if (best >= 0) {
            const ScoreBuf buf = pool_[best];
            pool_.erase(pool_.begin() + best);
            return buf;
        }
        void* p = alloc_(row_bytes() * (size_t)n_rows);
        if (!p) throw std::runtime_error("score buffer: out of device memory");
        return ScoreBuf{p, n_rows};
    }
    // a buffer goes back to the pool, which never holds more than B buffers (beyond that the smallest one is freed)
    void put(ScoreBuf buf) {
        if (!buf.p) return;
        pool_.push_back(buf);
        if ((int)pool_.size() <= B_) return;
        int small = 0;
        for (int i = 1; i < (int)pool_.size(); ++i) if (pool_[i].cap < pool_[small].cap) small = i;
        free_(pool_[small].p);
        pool_.erase(pool_.begin() + small);
    }
    static float* rec_of(const ScoreBuf& b) { return static_cast<float*>(b.p); }
    static uint32_t* targets_of(const ScoreBuf& b) { return reinterpret_cast<uint32_t*>(static_cast<float*>(b.p) + (size_t)b.cap * SCORE_REC_WORDS); }
    // the slot was admitted as a scoring slot (its prefill is queued): polls are answered from now on, with 0 rows until it is live
    void admitted(int b) { want_.at((size_t)b) = 1; }
    bool wanted(int b) const { return want_.at((size_t)b) != 0; }
    // activation: the slot's table entry, count 0 (the engine copies it to the device table)
    const ScoreSlot& activate(int b, ScoreBuf buf) {
        ScoreSlot& e = tab_.at((size_t)b);
        if (e.rec) throw std::runtime_error("score table: the slot already holds a buffer");
        e = ScoreSlot{targets_of(buf), rec_of(buf), 0, buf.cap};
        ++live_;
        return e;
    }
    // release: the entry is nulled and its buffer goes back; true when there was one (the engine then nulls the device entry)
    bool drop(int b) {
        want_.at((size_t)b) = 0;
        ScoreSlot& e = tab_.at((size_t)b);
        if (!e.rec) return false;
        put(ScoreBuf{e.rec, e.cap});
        e = ScoreSlot{nullptr, nullptr, 0, 0};
        --live_;
        return true;
    }
    // session_end: every live buffer back to the pool, every entry null
    void end() {
        for (ScoreSlot& e : tab_) { if (e.rec) put(ScoreBuf{e.rec, e.cap}); e = ScoreSlot{nullptr, nullptr, 0, 0}; }
        for (char& w : want_) w = 0;
        live_ = 0;
    }
    // the end-of-chunk copy of the device table lands here: only the counts are taken (the pointers are the host's own)
    void refresh_counts(const ScoreSlot* dev) {
        for (size_t b = 0; b < tab_.size(); ++b)
            if (tab_[b].rec && dev[b].rec == tab_[b].rec && dev[b].count >= 0 && dev[b].count <= tab_[b].cap) tab_[b].count = dev[b].count;
    }
    const ScoreSlot& entry(int b) const { return tab_.at((size_t)b); }
    int live() const { return live_; }
    size_t pooled() const { return pool_.size(); }

private:
    AllocFn alloc_;
    FreeFn free_;
    int B_ = 0, C1_ = 9, live_ = 0;
    std::vector<ScoreSlot> tab_;
    std::vector<char> want_;
    std::vector<ScoreBuf> pool_;
};

}  // namespace fs
