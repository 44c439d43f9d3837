// Host-side book of the slow transformer's paged KV cache: which page of the pool belongs to whom.  One book per handle.  It owns the free
// list, the reference count of every page, one page list per OWNER -- the n_seq sequence rows (owners 0 .. n_seq - 1) and a session's
// shared prefixes (prefix_owner(id)) -- and the loose HOLDS: a reference on one page that is in no list (a session's scratch page; a joining
// slot's hold on the partly filled last page of its prefix, until that page has been copied).  A page is free when nobody owns or holds it.
// The engine (lm_engine.hip) changes none of this except through the operations below, and sees a page list only as a const vector.
// The order in which pages are handed out is part of the contract (page ids show in exported prefixes and in KV dumps): the pool starts as
// n_pages - 1 .. 0, a page is taken from the back, and a page returns to the back when its last reference ends -- truncate() returns an
// owner's pages last-first, drop() first-first.
// Plain C++ -- no HIP in here -- so that a host program can run it under a sanitizer (tools/kv_pages_check.cpp).
#pragma once
#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

namespace fs {

// the leading k pages of owner `from` (a prefix) shared into a slot; from < 0: nothing shared
struct KvShare { int from = -1, k = 0; };
struct KvRoom { bool fits; int cost; };

class KvPages {
public:
    using Share = KvShare;
    using Room = KvRoom;
    static constexpr int kNewOwner = -1;  // room(): an owner that does not exist yet (a prefix about to be created)

    void init(int n_pages, int n_seq, int page_tokens, int max_tokens) {
        n_seq_ = n_seq; page_ = page_tokens; max_tokens_ = max_tokens;
        free_.clear();
        for (int p = n_pages - 1; p >= 0; --p) free_.push_back(p);
        refs_.assign((size_t)n_pages, 0);
        held_.assign((size_t)n_pages, 0);
        lists_.assign((size_t)n_seq, {});
    }
    int pages_for(int n_tokens) const { return (n_tokens + page_ - 1) / page_; }
    int prefix_owner(int id) const { return n_seq_ + id; }
    int add_prefix() { lists_.emplace_back(); return (int)lists_.size() - 1; }  // a new owner with no pages; prefix ids count up from 0 per session
    const std::vector<int>& of(int owner) const { return lists_.at((size_t)owner); }
    int owners() const { return (int)lists_.size(); }
    int free_count() const { return (int)free_.size(); }
    int shared_count() const { return (int)std::count_if(refs_.begin(), refs_.end(), [](int r) { return r > 1; }); }
    // (the host check compares these against its model; the engine has no use for them)
    const std::vector<int>& free_list() const { return free_; }
    int refs(int page) const { return refs_.at((size_t)page); }
    int holds(int page) const { return held_.at((size_t)page); }

    // Would growing `owner` to n_tokens -- its first s.k pages shared from s.from, not taken -- fit right now, and how many pages does it
    // take from the pool?  `reserved`: pages already promised to others that grow with it (the members of a group pass).  Reads only.
    // What makes share() or grow() throw for another reason than a short pool makes this throw, so a caller that was told `fits` may
    // share, grow and hold without a failure.
    Room room(int owner, int n_tokens, Share s = {}, int reserved = 0) const {
        need(n_tokens <= max_tokens_, "sequence longer than max_seq_len");
        const int have = owner == kNewOwner ? 0 : (int)of(owner).size();
        require_shareable(have, s);
        const int cost = std::max(0, pages_for(n_tokens) - s.k - have);
        return Room{reserved + cost <= free_count(), cost};
    }
    // the owner's list reaches n_tokens afterwards: every page it lacks is taken, or none is and this throws.  True when it grew.
    bool grow(int owner, int n_tokens) {
        need(n_tokens <= max_tokens_, "sequence longer than max_seq_len");
        std::vector<int>& pg = list(owner);
        const int want = pages_for(n_tokens);
        if ((int)pg.size() >= want) return false;
        need(free_count() >= want - (int)pg.size(), "KV page pool exhausted");
        while ((int)pg.size() < want) pg.push_back(take());
        return true;
    }
    // a slot without pages starts with the prefix's first k pages, one more reference on each
    void share(int owner, Share s) {
        std::vector<int>& pg = list(owner);
        require_shareable((int)pg.size(), s);
        for (int j = 0; j < s.k; ++j) { const int p = of(s.from)[(size_t)j]; pg.push_back(p); ++refs_[(size_t)p]; }
    }
    // holds: a page fresh from the pool, or page j of an owner's list; the page id is the handle drop_hold() takes
    int hold_new() {
        const int p = take();
        ++held_[(size_t)p];
        return p;
    }
    int hold_page_of(int owner, int j) {
        const int p = of(owner).at((size_t)j);
        ++refs_[(size_t)p]; ++held_[(size_t)p];
        return p;
    }
    void drop_hold(int page) {
        need(page >= 0 && page < (int)held_.size() && held_[(size_t)page] > 0, "KV page released twice");
        --held_[(size_t)page];
        put(page);
    }
    // keep the pages of the first n_tokens, the rest go back last-first (also: a prefix's pad pages after its pass, n_tokens = its length)
    void truncate(int owner, int n_tokens) {
        std::vector<int>& pg = list(owner);
        const int keep = pages_for(n_tokens);
        while ((int)pg.size() > keep) { put(pg.back()); pg.pop_back(); }
    }
    // the owner gives up all its pages, first-first
    void drop(int owner) {
        std::vector<int>& pg = list(owner);
        for (int p : pg) put(p);
        pg.clear();
    }
    // every reference of the session ends: the sequence rows (truncated to nothing, row by row), the prefixes (dropped in id order; the
    // prefix owners cease to exist), then whatever is still held (ascending page id)
    void end_session() {
        for (int b = 0; b < n_seq_; ++b) truncate(b, 0);
        for (int o = n_seq_; o < owners(); ++o) drop(o);
        lists_.resize((size_t)n_seq_);
        for (int p = 0; p < (int)held_.size(); ++p)
            while (held_[(size_t)p] > 0) drop_hold(p);
    }
    // the single-writer rule: nothing writes a page with more than one reference.  The owner writes positions >= pos0 (its prefill starts
    // there, its pad rows and decode steps lie beyond), so every page of its list from pos0's on must be its alone.
    void writable_from(int owner, int pos0) const {
        const std::vector<int>& pg = of(owner);
        for (size_t j = (size_t)(pos0 / page_); j < pg.size(); ++j) need(refs_[(size_t)pg[j]] == 1, "a session slot would write a shared KV page");
    }
    // every page of the owner's list is a page of the pool with a reference on it
    bool intact(int owner) const {
        for (int p : of(owner))
            if (p < 0 || p >= (int)refs_.size() || refs_[(size_t)p] < 1) return false;
        return true;
    }
    // The book's invariants, in O(pages + list entries): every page's count equals its appearances in the owners' lists plus its holds; the
    // free list is exactly the pages with count 0, each once; no list holds a page twice.  Throws on the first that does not hold.
    void check() const {
        const int n = (int)refs_.size();
        auto bad = [](int p, const char* what) { throw std::runtime_error("KV page book: page " + std::to_string(p) + " " + what); };
        std::vector<int> seen((size_t)n, 0), in_list((size_t)n, -1), on_free((size_t)n, 0);
        for (int o = 0; o < owners(); ++o)
            for (int p : lists_[(size_t)o]) {
                if (p < 0 || p >= n) bad(p, "is in an owner's list and not in the pool");
                if (in_list[(size_t)p] == o) bad(p, "is twice in one owner's list");
                in_list[(size_t)p] = o;
                ++seen[(size_t)p];
            }
        for (int p : free_) {
            if (p < 0 || p >= n) bad(p, "is on the free list and not in the pool");
            if (++on_free[(size_t)p] != 1) bad(p, "is on the free list twice");
        }
        for (int p = 0; p < n; ++p) {
            if (held_[(size_t)p] < 0 || refs_[(size_t)p] != seen[(size_t)p] + held_[(size_t)p]) bad(p, "has a count that is not its owners plus its holds");
            if ((refs_[(size_t)p] == 0) != (on_free[(size_t)p] == 1)) bad(p, on_free[(size_t)p] ? "is on the free list with references" : "has no reference and is not on the free list");
        }
    }

private:
    static void need(bool ok, const char* msg) {
        if (!ok) throw std::runtime_error(msg);
    }
    std::vector<int>& list(int owner) { return lists_.at((size_t)owner); }
    void require_shareable(int have, Share s) const {
        if (s.from < 0) { need(s.k == 0, "KV page book: shared pages without a prefix"); return; }
        need(have == 0, "a free slot still holds KV pages");
        need(s.k >= 0 && s.k <= (int)of(s.from).size(), "KV page book: more shared pages than the prefix holds");
    }
    // the two places a count changes by the pool's hand: a count goes to 1 from the free list only here, and down only in put()
    int take() {
        need(!free_.empty(), "KV page pool exhausted");
        const int p = free_.back();
        free_.pop_back();
        refs_[(size_t)p] = 1;
        return p;
    }
    void put(int p) {
        need(p >= 0 && p < (int)refs_.size() && refs_[(size_t)p] > 0, "KV page released twice");
        if (--refs_[(size_t)p] == 0) free_.push_back(p);
    }
    int n_seq_ = 0, page_ = 1, max_tokens_ = 0;
    std::vector<int> free_, refs_, held_;
    std::vector<std::vector<int>> lists_;  // [n_seq] the sequence rows, then the session's prefixes
};

}  // namespace fs
