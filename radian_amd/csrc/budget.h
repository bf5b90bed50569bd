// budget.h -- the device-memory budget contract of rd_align_batch, rd_fit_batch, rd_ctc_align_*, rd_map_batch, rd_polya_segment,
// rd_site_compare, rd_sim_lengths / rd_sim_signal and rd_eventalign, once.  Plain host C++ without a HIP type: tests/asan_budget.cpp compiles it with g++ and checks its properties.
//
// An entry point gives its items in its own launch order and gets back the launches that fit the caller's budget.  An item that alone
// exceeds the budget is counted, not launched; the entry point gives it its *_TOO_LARGE status and returns RD_ERR_NOMEM after the others
// have run.  Results never depend on the cut; peak memory and the number of launches do.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <utility>
#include <vector>

// budget_bytes == 0 of an entry point: a quarter of what is free, the blocks the context would regrow for the call counting as free
inline int64_t rd_default_budget(size_t free_bytes, size_t held_bytes) { return (int64_t)((free_bytes + held_bytes) / 4); }

struct BudgetPlan {
    std::vector<int32_t> run;                               // the launched items (original indices), in launch order
    std::vector<std::pair<int64_t, int64_t>> launches;      // [k0, k1) of run
    int64_t max_bytes = 0;                                  // the largest launch, overhead included (0: nothing is launched)
    int64_t too_large = 0, first_too_large = -1;            // items over the budget alone, and the lowest original index among them
};

// Cuts items order[0 .. n) (order == nullptr: 0 .. n - 1) greedily into launches of at most budget bytes, overhead per launch included.
//   bytes(p, prev)  what item p adds to a launch whose last item is prev; prev == -1: what p needs at the head of a launch, that is, alone.
//                   Negative with prev == -1: p takes no part (neither launched nor too large).
//   close_before(p, first, count, acc)  a further reason to end the open launch (first item `first`, count items, acc bytes) before p
//   too_large_closes  an item over the budget ends the open launch (for launches that must be ranges of consecutive items)
template <typename Bytes, typename CloseBefore>
inline BudgetPlan rd_plan_budget(int64_t n, const int32_t* order, int64_t budget, int64_t overhead, bool too_large_closes, Bytes bytes,
                                 CloseBefore close_before)
{
    BudgetPlan P;
    const int64_t room = budget - overhead;   // acc + add + overhead > budget, as acc + add > room: no sum that could overflow
    int64_t acc = 0;
    bool open = false;
    for (int64_t k = 0; k < n; k++) {
        const int32_t p = order ? order[k] : (int32_t)k;
        const int64_t alone = bytes(p, -1);
        if (alone < 0) continue;
        if (alone > room) {
            if (P.too_large++ == 0 || p < P.first_too_large) P.first_too_large = p;
            if (too_large_closes) open = false;
            continue;
        }
        const int64_t r = (int64_t)P.run.size(), r0 = open ? P.launches.back().first : r;
        int64_t add = open ? bytes(p, P.run[r - 1]) : alone;
        if (!open || add > room - acc || close_before(p, P.run[r0], r - r0, acc)) {
            P.launches.push_back({r, r});
            acc = 0;
            add = alone;
            open = true;
        }
        P.run.push_back(p);
        P.launches.back().second = r + 1;
        acc += add;
        P.max_bytes = std::max(P.max_bytes, acc + overhead);
    }
    return P;
}
inline bool rd_budget_never_closes(int32_t, int32_t, int64_t, int64_t) { return false; }
