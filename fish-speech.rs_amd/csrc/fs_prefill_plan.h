// Which of a session's queued requests go into its next prefill pass.  The engine (lm_engine.hip: flush_pending) queues joining requests --
// plain and prefixed adds, a prefix's own pass, a prefix's import -- and launches ONE pass at a time on its prefill stream; this header
// decides what that pass is and launches nothing.  It reads the queue (one PrefillMember per entry), the page book and four limits:
//   order   imports first, then creations, then by rows() descending; stable, so equals keep their order of arrival
//   Imports the queue's head is an import: all leading imports, and nothing else (copies and scatters, no transformer pass)
//   NoRows  the longest entry has no row to run (only adds with one-column bodies are left): the whole queue, no pass
//   Single  one sequence, its own Lp = rows() tokens in passes of the row buffers' capacity.  No pad rows, so nothing to grow.
//   Group   the first n entries side by side, each right-padded to the first one's Lp rows.  A member joins the first while there
//           are row buffers for it (n * Lp <= rows_cap, n <= max_batch), it has a row to run, it is of the first one's kind (creations
//           with creations), neither of the two names a sampler seed (a seeded member goes alone: a group pass rounds differently from
//           a single one, and whoever names a seed asks for codes that are a function of the request alone), its pad rows stay inside
//           max_seq_len (start + Lp; the first member is not held to that: Lp is its own row count) and the pool has the pages its pad
//           rows write -- counted CUMULATIVELY over the group: checked per member, several short members could each pass and the
//           growth would then throw in the middle of the flush.  A first member whose own pad pages do not fit goes alone.
// A group pass writes K/V up to pad_end[s] for member s; the engine grows each member's owner that far before it launches (the plan only
// asked the book whether it can).
// Plain C++ -- no HIP in here -- so that a host program can run it under a sanitizer (tools/prefill_plan_check.cpp).
#pragma once
#include <algorithm>
#include <numeric>
#include <vector>

#include "fs_kv_pages.h"

namespace fs {

// what the decision reads of a queued request (the engine's PendingAdd is one of these plus what the pass moves).  L: columns in all,
// the prefix's included; start: the prefix's length (0: none); owner: the page-book owner the pass writes -- the slot, or the prefix
// being created
struct PrefillMember {
    int L = 0, n_iter = 0, start = 0, owner = -1;
    bool create = false, import_kv = false, has_seed = false;
    int rows() const { return import_kv ? 0 : (create ? L : L - start - 1); }  // tokens this member runs through the slow transformer
    int cols() const { return create ? L : L - start; }                         // columns of its prompt
    int end() const { return create ? L : L + n_iter - 1; }                     // positions whose K/V the member keeps
};
struct PrefillLimits {
    int rows_cap;     // rows of the activation buffers
    int max_batch;    // sequences of a pass's staging page-table rows
    int max_seq_len;
    bool flash;       // head_dim == 64: the group pass exists
};
struct PrefillPass {
    enum Kind { Imports, NoRows, Single, Group } kind = NoRows;
    int n = 0;                 // members: the first n of the ordered queue
    int Lp = 0;                // Single / Group: rows of the longest member, the first
    int max_start = 0;         // Single / Group: the largest start among the members
    std::vector<int> pad_end;  // Group: per member, how far its pass writes K/V
};
struct PrefillPlan {
    std::vector<int> order;  // entry i of the ordered queue is entry order[i] of the queue given
    PrefillPass pass;
};

inline PrefillPlan plan_prefill(const std::vector<PrefillMember>& q, const KvPages& pages, const PrefillLimits& lim) {
    PrefillPlan plan;
    plan.order.resize(q.size());
    std::iota(plan.order.begin(), plan.order.end(), 0);
    std::stable_sort(plan.order.begin(), plan.order.end(), [&](int x, int y) {
        const PrefillMember &a = q[(size_t)x], &b = q[(size_t)y];
        if (a.import_kv != b.import_kv) return a.import_kv;
        return a.create != b.create ? a.create : a.rows() > b.rows();
    });
    PrefillPass& ps = plan.pass;
    if (q.empty()) return plan;
    auto at = [&](size_t i) -> const PrefillMember& { return q[(size_t)plan.order[i]]; };
    const PrefillMember& first = at(0);
    if (first.import_kv) {
        ps.kind = PrefillPass::Imports;
        while ((size_t)ps.n < q.size() && at((size_t)ps.n).import_kv) ++ps.n;
        return plan;
    }
    const int Lp = first.rows();
    if (Lp < 1) {
        ps.n = (int)q.size();
        return plan;
    }
    int S = 1;
    if (lim.flash && Lp <= lim.rows_cap) {
        const int fit = std::max(1, std::min(lim.rows_cap / Lp, lim.max_batch));
        auto pad_end = [&](const PrefillMember& m) { return std::max(m.end(), m.start + Lp); };
        int need_sum = 0;
        auto extra = [&](const PrefillMember& m) { return pages.room(m.owner, pad_end(m), {}, need_sum); };
        const KvRoom head = extra(first);
        need_sum = head.cost;
        while ((size_t)S < q.size() && S < fit && at((size_t)S).rows() >= 1 && at((size_t)S).create == first.create && !first.has_seed &&
               !at((size_t)S).has_seed && at((size_t)S).start + Lp <= lim.max_seq_len) {
            const KvRoom more = extra(at((size_t)S));
            if (!more.fits) break;
            need_sum += more.cost;
            ++S;
        }
        if (!head.fits) S = 1;  // (the first member's own pages were reserved when it was admitted: alone it needs none)
        if (S > 1)
            for (int s = 0; s < S; ++s) ps.pad_end.push_back(pad_end(at((size_t)s)));
    }
    ps.kind = S > 1 ? PrefillPass::Group : PrefillPass::Single;
    ps.n = S;
    ps.Lp = Lp;
    for (int s = 0; s < S; ++s) ps.max_start = std::max(ps.max_start, at((size_t)s).start);
    return plan;
}

}  // namespace fs
