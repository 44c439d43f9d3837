// Host-side bookkeeping of the session slots that carry a collector buffer: scoring slots (fishrt.h: fs_lm_session_add_scored, entry
// ScoreSlot) and hidden-state collectors (fs_lm_session_add_hidden, entry HidSlot).  One SlotBook per kind: the per-slot table the step's
// graph node reads (host mirror; the engine copies entries to the device), and the per-handle pool the slots' buffers come from.
// Plain C++ -- no HIP in here, the allocator is handed in -- so that a host program can run it under a sanitizer
// (tools/slot_book_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace fs {

// One entry per slot: rec == null -> the slot is not scored; else iteration `count` of the slot is forced to targets[count][0 .. C]
// (slow token, c0..c7) and leaves the 32-word record rec[count]: [0..8] logprob of the target per decision, [9..17] logprob of the
// maximum, [18..26] the last maximal index (u32 bits), [27] logprob of <|im_end|> at the slow decision (-inf when masked), [28..31] zero.
// A TRACED slot (fs_lm_session_add_traced) is an entry of this table whose DEVICE copy has targets == null: it samples, its record rows
// hold the same figures for its own picks, and the rows behind the records ([cap][C + 1] u32, the host entry's `targets`) receive the picks.
// In a FS_SESSION_ALTS session the buffer goes on behind those rows: alt_index u32 [cap][C + 1][N], alt_logprob f32 [cap][C + 1][N],
// entropy f32 [cap][C + 1] (score_alts_bytes per row); the kernels derive the three from rec, cap and N, the entry stays as it is.
struct ScoreSlot {
    const uint32_t* targets;  // [cap][C + 1]
    float* rec;               // [cap][32]
    int count, cap;
};
constexpr int SCORE_REC_WORDS = 32;
// first word of each part of a record (the host's unpack; the device side writes the same layout)
constexpr int SCORE_REC_LOGPROB = 0, SCORE_REC_TOP_LOGPROB = 9, SCORE_REC_TOP = 18, SCORE_REC_EOS = 27;
// One entry per slot: rows == null -> the slot does not collect; else its buffer f32 [cap][dim], and count = rows stored so far == the
// slot's generator iterations so far.
struct HidSlot {
    float* rows;
    int count, cap;
};
// (the kernels read both tables: k_score_slots, k_hidden_rows)
static_assert(sizeof(ScoreSlot) == 24 && offsetof(ScoreSlot, targets) == 0 && offsetof(ScoreSlot, rec) == 8 && offsetof(ScoreSlot, count) == 16 &&
              offsetof(ScoreSlot, cap) == 20, "ScoreSlot layout");
static_assert(sizeof(HidSlot) == 16 && offsetof(HidSlot, rows) == 0 && offsetof(HidSlot, count) == 8 && offsetof(HidSlot, cap) == 12, "HidSlot layout");

// one allocation per slot, cap rows of the book's row_bytes.  Scoring: the records [cap][32] f32 first (128-byte rows), the targets
// [cap][C + 1] u32 behind them (row_bytes = 128 + 4 (C + 1)); hidden rows: [cap][dim] f32 (row_bytes = 4 dim)
struct SlotBuf {
    void* p = nullptr;
    int cap = 0;
};
inline float* score_rec(const SlotBuf& b) { return static_cast<float*>(b.p); }
inline uint32_t* score_targets(const SlotBuf& b) { return reinterpret_cast<uint32_t*>(static_cast<float*>(b.p) + (size_t)b.cap * SCORE_REC_WORDS); }
// the alternatives of a FS_SESSION_ALTS session (n_alts = N per decision, C1 = C + 1 decisions): bytes per row, and the three blocks of a buffer
inline size_t score_alts_bytes(int C1, int n_alts) { return (size_t)C1 * (8 * (size_t)n_alts + 4); }
inline uint32_t* score_alt_index(const ScoreSlot& e, int C1) { return const_cast<uint32_t*>(e.targets) + (size_t)e.cap * C1; }
inline float* score_alt_logprob(const ScoreSlot& e, int C1, int n_alts) { return reinterpret_cast<float*>(score_alt_index(e, C1) + (size_t)e.cap * C1 * n_alts); }
inline float* score_alt_entropy(const ScoreSlot& e, int C1, int n_alts) { return score_alt_logprob(e, C1, n_alts) + (size_t)e.cap * C1 * n_alts; }

// what the book needs of an entry type: the entry of a buffer (count 0) and the pointer that identifies the buffer; E{} is the null entry
template <typename E> struct SlotKind;
template <> struct SlotKind<ScoreSlot> {
    static constexpr const char* name = "score";
    static ScoreSlot entry(const SlotBuf& b) { return ScoreSlot{score_targets(b), score_rec(b), 0, b.cap}; }
    static void* buf(const ScoreSlot& e) { return e.rec; }
};
template <> struct SlotKind<HidSlot> {
    static constexpr const char* name = "hidden-row";
    static HidSlot entry(const SlotBuf& b) { return HidSlot{static_cast<float*>(b.p), 0, b.cap}; }
    static void* buf(const HidSlot& e) { return e.rows; }
};

template <typename E>
class SlotBook {
    using K = SlotKind<E>;

public:
    using AllocFn = void* (*)(size_t);
    using FreeFn = void (*)(void*);
    SlotBook(AllocFn a, FreeFn f) : alloc_(a), free_(f) {}
    SlotBook(const SlotBook&) = delete;
    SlotBook& operator=(const SlotBook&) = delete;
    ~SlotBook() {
        end();
        for (SlotBuf& b : pool_) free_(b.p);
    }
    // session_begin: B slots, buffers of row_bytes per row, no slot holds one; buffers a previous session left live go back to the pool.
    // take() matches pooled buffers by their rows alone, so a pool filled under another row size is freed here: a buffer allocated for
    // shorter rows would be handed out too short (the score book's rows grow in a FS_SESSION_ALTS session)
    void begin(int B, size_t row_bytes) {
        end();
        if (row_bytes != row_bytes_) {
            for (SlotBuf& b : pool_) free_(b.p);
            pool_.clear();
        }
        B_ = B; row_bytes_ = row_bytes;
        tab_.assign((size_t)B, E{});
        want_.assign((size_t)B, 0);
    }
    size_t row_bytes() const { return row_bytes_; }
    // a free buffer of >= n_rows rows (the smallest that fits), else a new one; throws when the allocator returns null.  The buffer is
    // IN HAND until it is activated or put back: end() and the destructor reclaim what is still in hand then (an add queued or in flight)
    SlotBuf take(int n_rows) {
        if (n_rows < 1) throw std::runtime_error(std::string(K::name) + " buffer: no rows");
        int best = -1;
        for (int i = 0; i < (int)pool_.size(); ++i)
            if (pool_[i].cap >= n_rows && (best < 0 || pool_[i].cap < pool_[best].cap)) best = i;
        SlotBuf buf{nullptr, n_rows};
        if (best >= 0) {
            buf = pool_[best];
            pool_.erase(pool_.begin() + best);
        } else if (!(buf.p = alloc_(row_bytes_ * (size_t)n_rows))) {
            throw std::runtime_error(std::string(K::name) + " buffer: out of device memory");
        }
        hand_.push_back(buf);
        return buf;
    }
    // a buffer in hand goes back to the pool (a refused add); one that is not in hand -- null, put back or activated already -- is left alone
    void put(const SlotBuf& buf) {
        if (unhand(buf)) pool_put(buf);
    }
    // the slot was admitted with a buffer (its prefill is queued): polls are answered from now on, with 0 rows until it is live
    void admitted(int b) { want_.at((size_t)b) = 1; }
    bool wanted(int b) const { return want_.at((size_t)b) != 0; }
    // activation: the slot's table entry, count 0 (the engine copies it to the device table)
    const E& activate(int b, const SlotBuf& buf) {
        E& e = tab_.at((size_t)b);
        if (K::buf(e)) throw std::runtime_error(std::string(K::name) + " table: the slot already holds a buffer");
        if (!unhand(buf)) throw std::runtime_error(std::string(K::name) + " table: the buffer is not in hand");
        e = K::entry(buf);
        ++live_;
        return e;
    }
    // release: the entry is nulled and its buffer goes back; true when there was one (the engine then nulls the device entry)
    bool drop(int b) {
        want_.at((size_t)b) = 0;
        E& e = tab_.at((size_t)b);
        if (!K::buf(e)) return false;
        pool_put(SlotBuf{K::buf(e), e.cap});
        e = E{};
        --live_;
        return true;
    }
    // session_end: every live buffer and every buffer still in hand back to the pool, every entry null
    void end() {
        for (E& e : tab_) { if (K::buf(e)) pool_put(SlotBuf{K::buf(e), e.cap}); e = E{}; }
        for (const SlotBuf& b : hand_) pool_put(b);
        hand_.clear();
        for (char& w : want_) w = 0;
        live_ = 0;
    }
    // the end-of-chunk copy of the device table lands here: only the counts are taken (the pointers are the host's own)
    void refresh_counts(const E* dev) {
        for (size_t b = 0; b < tab_.size(); ++b)
            if (K::buf(tab_[b]) && K::buf(dev[b]) == K::buf(tab_[b]) && dev[b].count >= 0 && dev[b].count <= tab_[b].cap) tab_[b].count = dev[b].count;
    }
    const E& entry(int b) const { return tab_.at((size_t)b); }
    int live() const { return live_; }
    size_t pooled() const { return pool_.size(); }
    size_t in_hand() const { return hand_.size(); }

private:
    bool unhand(const SlotBuf& buf) {
        for (size_t i = 0; buf.p && i < hand_.size(); ++i)
            if (hand_[i].p == buf.p) { hand_.erase(hand_.begin() + i); return true; }
        return false;
    }
    // the pool never holds more than B buffers (beyond that the smallest one is freed)
    void pool_put(const SlotBuf& buf) {
        pool_.push_back(buf);
        if ((int)pool_.size() <= B_) return;
        int small = 0;
        for (int i = 1; i < (int)pool_.size(); ++i) if (pool_[i].cap < pool_[small].cap) small = i;
        free_(pool_[small].p);
        pool_.erase(pool_.begin() + small);
    }
    AllocFn alloc_;
    FreeFn free_;
    int B_ = 0, live_ = 0;
    size_t row_bytes_ = 0;
    std::vector<E> tab_;
    std::vector<char> want_;
    std::vector<SlotBuf> pool_, hand_;
};

}  // namespace fs
