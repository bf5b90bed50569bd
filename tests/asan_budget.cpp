// TEST INFRASTRUCTURE: AddressSanitizer + UBSan harness AND property check for radian_amd/csrc/budget.h -- the cutter that packs the items
// of rd_align_batch, rd_fit_batch, rd_ctc_align_*, rd_map_batch and rd_polya_segment into launches under the caller's budget.
// usage: asan_budget <instances per configuration>
// For seeded random instances of each of the five configurations (as the entry point calls the cutter: its order, overhead, state-dependent
// bytes, extra closing rule, closing flag, items that take no part):
//   * the launches tile the launched list in order, without gap or overlap, none empty; the launched list is, in order, every item that takes
//     part and fits alone;
//   * every launch's bytes plus the overhead are within the budget, and the reported largest launch is the true maximum;
//   * no launch ends early: its successor's first item would have broken the budget or the extra rule (or a too-large item lies between them
//     where those close a launch), and inside a launch the extra rule never asked for a cut;
//   * exactly the items with alone + overhead > budget are too large, and first_too_large is their lowest index;
//   * with the closing flag no launch spans a too-large item.
// The yardstick for "the cut did not change": the five loops as the entry points held them before budget.h existed, transcribed below
// (cut_*_loop).  The cutter must give the same launches, the same largest launch and the same too-large count and index on every instance.
#include "../radian_amd/csrc/budget.h"

#include <cstdio>
#include <cstdlib>
#include <functional>
#include <numeric>
#include <random>

#define CHECK(cond, ...)                                                          \
    do {                                                                          \
        if (!(cond)) {                                                            \
            printf("property violated: %s  (", #cond);                           \
            printf(__VA_ARGS__);                                                  \
            printf(")\n");                                                        \
            return 1;                                                             \
        }                                                                         \
    } while (0)

using BytesFn = std::function<int64_t(int32_t, int32_t)>;
using CloseFn = std::function<bool(int32_t, int32_t, int64_t, int64_t)>;

struct Config {
    const char* name;
    int64_t n;
    std::vector<int32_t> order;   // empty: the caller's order
    int64_t budget, overhead;
    bool closes;
    BytesFn bytes;
    CloseFn close_before;
};

// what a loop of the parent commit decided, in the cutter's terms
struct Cut {
    std::vector<std::vector<int32_t>> launches;   // the items of every launch
    int64_t max_bytes = 0, too_large = 0, first_too_large = -1;
};

static BudgetPlan run_cutter(const Config& c)
{
    return rd_plan_budget(c.n, c.order.empty() ? nullptr : c.order.data(), c.budget, c.overhead, c.closes, c.bytes, c.close_before);
}

static int check_properties(const Config& c, const BudgetPlan& P, int it)
{
    const auto item = [&](int64_t k) { return c.order.empty() ? (int32_t)k : c.order[k]; };
    const int64_t room = c.budget - c.overhead;
    // the launched list and the too-large items, from the definition
    std::vector<int32_t> fits;
    std::vector<int64_t> fits_at;   // position in the order
    std::vector<int64_t> big_at;
    int64_t n_big = 0, first_big = -1;
    for (int64_t k = 0; k < c.n; k++) {
        const int32_t p = item(k);
        const int64_t alone = c.bytes(p, -1);
        if (alone < 0) continue;
        if (alone > room) {
            if (n_big++ == 0 || p < first_big) first_big = p;
            big_at.push_back(k);
        } else {
            fits.push_back(p);
            fits_at.push_back(k);
        }
    }
    CHECK(P.too_large == n_big && P.first_too_large == first_big, "%s it %d: too large %lld first %lld, expected %lld first %lld", c.name, it,
          (long long)P.too_large, (long long)P.first_too_large, (long long)n_big, (long long)first_big);
    CHECK(P.run == fits, "%s it %d: the launched list is not the items that fit alone, in order", c.name, it);
    const auto big_between = [&](int64_t ka, int64_t kb) {   // a too-large item between launched items ka and kb of the list
        for (int64_t b : big_at)
            if (b > fits_at[ka] && b < fits_at[kb]) return true;
        return false;
    };
    int64_t next = 0, max_bytes = 0;
    for (size_t l = 0; l < P.launches.size(); l++) {
        const int64_t k0 = P.launches[l].first, k1 = P.launches[l].second;
        CHECK(k0 == next && k1 > k0 && k1 <= (int64_t)P.run.size(), "%s it %d: launch [%lld, %lld) after %lld of %zu", c.name, it, (long long)k0,
              (long long)k1, (long long)next, P.run.size());
        int64_t acc = c.bytes(P.run[k0], -1);
        for (int64_t k = k0 + 1; k < k1; k++) {
            CHECK(!c.close_before(P.run[k], P.run[k0], k - k0, acc), "%s it %d: launch [%lld, %lld) runs past the extra rule at %lld", c.name, it,
                  (long long)k0, (long long)k1, (long long)k);
            CHECK(!c.closes || !big_between(k - 1, k), "%s it %d: launch [%lld, %lld) spans a too-large item", c.name, it, (long long)k0, (long long)k1);
            acc += c.bytes(P.run[k], P.run[k - 1]);
        }
        CHECK(acc <= room, "%s it %d: launch [%lld, %lld) takes %lld + %lld bytes, budget %lld", c.name, it, (long long)k0, (long long)k1,
              (long long)acc, (long long)c.overhead, (long long)c.budget);
        max_bytes = std::max(max_bytes, acc + c.overhead);
        if (k1 < (int64_t)P.run.size()) {   // greedy: the next item would not have fitted
            const int32_t q = P.run[k1];
            const bool cut_needed = c.bytes(q, P.run[k1 - 1]) > room - acc || c.close_before(q, P.run[k0], k1 - k0, acc) || (c.closes && big_between(k1 - 1, k1));
            CHECK(cut_needed, "%s it %d: launch [%lld, %lld) ends early", c.name, it, (long long)k0, (long long)k1);
        }
        next = k1;
    }
    CHECK(next == (int64_t)P.run.size(), "%s it %d: launches end at %lld of %zu", c.name, it, (long long)next, P.run.size());
    CHECK(P.max_bytes == max_bytes, "%s it %d: largest launch %lld, expected %lld", c.name, it, (long long)P.max_bytes, (long long)max_bytes);
    return 0;
}

static int check_same(const Config& c, const BudgetPlan& P, const Cut& old, int it)
{
    CHECK(P.launches.size() == old.launches.size(), "%s it %d: %zu launches, the loop it replaces cut %zu", c.name, it, P.launches.size(), old.launches.size());
    for (size_t l = 0; l < P.launches.size(); l++) {
        const std::vector<int32_t> mine(P.run.begin() + P.launches[l].first, P.run.begin() + P.launches[l].second);
        CHECK(mine == old.launches[l], "%s it %d: launch %zu differs from the loop it replaces", c.name, it, l);
    }
    CHECK(P.max_bytes == old.max_bytes, "%s it %d: largest launch %lld, the loop it replaces had %lld", c.name, it, (long long)P.max_bytes, (long long)old.max_bytes);
    CHECK(P.too_large == old.too_large && P.first_too_large == old.first_too_large, "%s it %d: too large %lld first %lld, the loop it replaces had %lld first %lld",
          c.name, it, (long long)P.too_large, (long long)P.first_too_large, (long long)old.too_large, (long long)old.first_too_large);
    return 0;
}

// ---- the parent commit's loops ------------------------------------------------------------------------------------------------------------
// rd_align_batch: pairs largest first
static Cut cut_align_loop(int n_pairs, const std::vector<int64_t>& cells, const std::vector<int64_t>& bytes, int64_t budget_bytes, int64_t ALN_BATCH_BYTES)
{
    std::vector<int> order(n_pairs);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return cells[x] > cells[y]; });
    int too_large = 0, first_too_large = -1;
    std::vector<std::pair<int, int>> batches;   // [k0, k1) of the launched order
    std::vector<int> run;
    int64_t acc = 0, max_batch = 0;
    for (int p : order) {
        if (bytes[p] + (int64_t)ALN_BATCH_BYTES > budget_bytes) {
            if (too_large++ == 0 || p < first_too_large) first_too_large = p;
            continue;
        }
        const int k = (int)run.size();
        if (batches.empty() || acc + bytes[p] + (int64_t)ALN_BATCH_BYTES > budget_bytes) {
            batches.push_back({k, k});
            acc = 0;
        }
        run.push_back(p);
        batches.back().second = k + 1;
        acc += bytes[p];
        max_batch = std::max(max_batch, acc + (int64_t)ALN_BATCH_BYTES);
    }
    Cut c;
    for (auto [k0, k1] : batches) c.launches.push_back(std::vector<int32_t>(run.begin() + k0, run.begin() + k1));
    c.max_bytes = max_batch;
    c.too_large = too_large;
    c.first_too_large = first_too_large;
    return c;
}

// rd_fit_batch: queries by reference; a reference is paid for once per batch
static Cut cut_fit_loop(int64_t n_queries, const std::vector<int64_t>& m_of, const std::vector<int32_t>& query_ref, const std::vector<int64_t>& ref_bytes,
                        const std::function<int64_t(int64_t)>& fit_query_bytes, int64_t budget_bytes, int64_t FIT_BATCH_BYTES)
{
    std::vector<int32_t> order;
    int64_t too_large = 0, first_too_large = -1;
    for (int64_t p = 0; p < n_queries; p++) {
        const int64_t m = m_of[p];
        if (m == 0) {
        } else if ((int64_t)(ref_bytes[query_ref[p]] + fit_query_bytes(m) + FIT_BATCH_BYTES) > budget_bytes) {
            if (too_large++ == 0) first_too_large = p;
        } else {
            order.push_back((int32_t)p);
        }
    }
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return query_ref[x] < query_ref[y]; });
    std::vector<std::pair<size_t, size_t>> batches;   // [k0, k1) of order
    int64_t acc = 0, max_batch = 0;
    int32_t last_ref = -1;
    for (size_t k = 0; k < order.size(); k++) {
        const int32_t p = order[k], r = query_ref[p];
        const int64_t qb = (int64_t)fit_query_bytes(m_of[p]), rb = (int64_t)ref_bytes[r];
        int64_t add = qb + (r != last_ref ? rb : 0);
        if (batches.empty() || acc + add + (int64_t)FIT_BATCH_BYTES > budget_bytes) {
            batches.push_back({k, k});
            acc = 0;
            add = qb + rb;
        }
        batches.back().second = k + 1;
        acc += add;
        last_ref = r;
        max_batch = std::max(max_batch, acc + (int64_t)FIT_BATCH_BYTES);
    }
    Cut c;
    for (auto [k0, k1] : batches) c.launches.push_back(std::vector<int32_t>(order.begin() + k0, order.begin() + k1));
    c.max_bytes = max_batch;
    c.too_large = too_large;
    c.first_too_large = first_too_large;
    return c;
}

// rd_ctc_align_dev: the caller's order, at most CA_MAX_LAUNCH sequences per launch
static Cut cut_ctcalign_loop(int n_seq, const std::vector<int64_t>& seq_bytes, int64_t budget_bytes, int CA_MAX_LAUNCH)
{
    int too_large = 0, first_too_large = -1;
    std::vector<int> run;
    std::vector<std::pair<int, int>> launches;   // [k0, k1) of run
    int64_t acc = 0, max_launch = 0;
    for (int i = 0; i < n_seq; i++) {
        const int64_t bytes = seq_bytes[i];
        if (bytes > budget_bytes) {
            if (too_large++ == 0) first_too_large = i;
            continue;
        }
        const int k = (int)run.size();
        if (launches.empty() || acc + bytes > budget_bytes || k - launches.back().first >= CA_MAX_LAUNCH) {
            launches.push_back({k, k});
            acc = 0;
        }
        run.push_back(i);
        launches.back().second = k + 1;
        acc += bytes;
        max_launch = std::max(max_launch, acc);
    }
    Cut c;
    for (auto [k0, k1] : launches) c.launches.push_back(std::vector<int32_t>(run.begin() + k0, run.begin() + k1));
    c.max_bytes = max_launch;
    c.too_large = too_large;
    c.first_too_large = first_too_large;
    return c;
}

// rd_map_batch: launches are ranges of reads [r0, r1); reads without anchors lie inside them; the workspace was
// max_anchors * MAP_ANCHOR_BYTES + MAP_LAUNCH_BYTES (reserve_launch_ws) when there was a launch
static Cut cut_map_loop(int64_t n_reads, const std::vector<int64_t>& read_a, int64_t budget_bytes, int64_t MAP_ANCHOR_BYTES, int64_t MAP_LAUNCH_BYTES,
                        int MAP_MAX_LAUNCH_READS)
{
    struct Launch {
        int64_t r0, r1;
    };
    std::vector<Launch> launches;
    int64_t too_large = 0, first_too_large = -1, acc = 0, max_anchors = 0;
    bool open = false;   // a read over the budget closes the launch before it: a launch's anchors are one range of the scan
    for (int64_t r = 0; r < n_reads; r++) {
        const int64_t a = read_a[r + 1] - read_a[r];
        if (a == 0) continue;   // RD_MAP_NO_SEED already
        if (a * MAP_ANCHOR_BYTES + MAP_LAUNCH_BYTES > budget_bytes || a >= ((int64_t)1 << 31)) {
            if (too_large++ == 0) first_too_large = r;
            open = false;
            continue;
        }
        if (!open || (acc + a) * MAP_ANCHOR_BYTES + MAP_LAUNCH_BYTES > budget_bytes || r + 1 - launches.back().r0 > MAP_MAX_LAUNCH_READS ||
            acc + a >= ((int64_t)1 << 31)) {
            launches.push_back({r, r});
            acc = 0;
            open = true;
        }
        launches.back().r1 = r + 1;
        acc += a;
        max_anchors = std::max(max_anchors, acc);
    }
    Cut c;
    for (const Launch& L : launches) {
        c.launches.push_back({});
        for (int64_t r = L.r0; r < L.r1; r++)
            if (read_a[r + 1] - read_a[r]) c.launches.back().push_back((int32_t)r);   // (the cutter lists the reads that take part)
    }
    c.max_bytes = launches.empty() ? 0 : max_anchors * MAP_ANCHOR_BYTES + MAP_LAUNCH_BYTES;
    c.too_large = too_large;
    c.first_too_large = first_too_large;
    return c;
}

// rd_polya_segment: the caller's order; the loop launched as it cut (launch() here records the members)
static Cut cut_polya_loop(int n_reads, const std::vector<int64_t>& read_bytes, int64_t budget_bytes)
{
    Cut c;
    int first_too_large = -1, too_large = 0;
    std::vector<int> members;
    int64_t acc = 0, max_launch = 0;
    const auto launch = [&]() {
        const int n = (int)members.size();
        if (n == 0) return;
        c.launches.push_back(std::vector<int32_t>(members.begin(), members.end()));
        members.clear();
    };
    for (int r = 0; r < n_reads; r++) {
        const int64_t bytes = read_bytes[r];
        if (bytes > budget_bytes) {
            if (first_too_large < 0) first_too_large = r;
            too_large++;
            continue;
        }
        if (!members.empty() && acc + bytes > budget_bytes) {
            launch();
        }
        if (members.empty()) {
            acc = 0;
        }
        members.push_back(r);
        acc += bytes;
        max_launch = std::max(max_launch, acc);   // (the loop never knew its largest launch: what its launches summed to)
    }
    launch();
    c.max_bytes = max_launch;
    c.too_large = too_large;
    c.first_too_large = first_too_large;
    return c;
}

// ---- random instances ---------------------------------------------------------------------------------------------------------------------
// sizes of a few scales, and a budget that is tiny, exactly one item's need, a few items' worth or ample
static int64_t draw_size(std::mt19937_64& rng) { return 1 + (int64_t)(rng() % (rng() % 4 ? 4000 : 200000)); }
static int64_t draw_budget(std::mt19937_64& rng, int64_t overhead, const std::vector<int64_t>& alone)
{
    const int64_t one = alone.empty() ? 1000 : alone[rng() % alone.size()];
    switch (rng() % 6) {
    case 0: return (int64_t)(rng() % 64);                                 // (nearly) everything too large
    case 1: return one + overhead;                                        // exactly one item's need
    case 2: return one + overhead - 1;                                    // one byte short of it
    case 3: return overhead + one + (int64_t)(rng() % (8 * one + 1));     // a few items per launch
    case 4: return overhead + (int64_t)(rng() % 30000);
    default: return (int64_t)1 << 40;                                     // one launch
    }
}
static int draw_n(std::mt19937_64& rng, int it) { return it % 97 == 0 ? 0 : it % 97 == 1 ? 1 : (int)(rng() % 80); }

static int check_instance(const Config& c, const Cut& old, int it)
{
    const BudgetPlan P = run_cutter(c);
    return check_properties(c, P, it) || check_same(c, P, old, it);
}

static const CloseFn never = [](int32_t, int32_t, int64_t, int64_t) { return false; };

static int check_align(std::mt19937_64& rng, int it)
{
    const int n = draw_n(rng, it);
    std::vector<int64_t> cells(n), bytes(n);
    for (int p = 0; p < n; p++) {
        bytes[p] = draw_size(rng);
        cells[p] = rng() % 3 ? bytes[p] / 7 : (int64_t)(rng() % 5);   // (ties: the sort is stable)
    }
    const int64_t overhead = 1024, budget = draw_budget(rng, overhead, bytes);
    Config c{"align", n, std::vector<int32_t>(n), budget, overhead, false, [&](int32_t p, int32_t) { return bytes[p]; }, never};
    std::iota(c.order.begin(), c.order.end(), 0);
    std::stable_sort(c.order.begin(), c.order.end(), [&](int x, int y) { return cells[x] > cells[y]; });
    if (n == 0) c.order.clear();
    return check_instance(c, cut_align_loop(n, cells, bytes, budget, overhead), it);
}

static int check_fit(std::mt19937_64& rng, int it)
{
    const int n = draw_n(rng, it), n_refs = 1 + (int)(rng() % 6);
    std::vector<int64_t> ref_bytes(n_refs), m_of(n), alone(n);
    std::vector<int32_t> query_ref(n);
    for (int64_t& b : ref_bytes) b = (draw_size(rng) + 3) / 4 * 4;
    const auto query_bytes = [](int64_t m) { return 64 + m; };
    for (int p = 0; p < n; p++) {
        m_of[p] = rng() % 5 ? 1 + (int64_t)(rng() % 1024) : 0;   // empty queries take no part
        query_ref[p] = (int32_t)(rng() % n_refs);
        alone[p] = ref_bytes[query_ref[p]] + query_bytes(m_of[p]);
    }
    const int64_t overhead = 1024, budget = draw_budget(rng, overhead, alone);
    Config c{"fit", n, std::vector<int32_t>(n), budget, overhead, false,
             [&](int32_t p, int32_t prev) -> int64_t {
                 if (m_of[p] == 0) return -1;
                 return query_bytes(m_of[p]) + (prev >= 0 && query_ref[prev] == query_ref[p] ? 0 : ref_bytes[query_ref[p]]);
             },
             never};
    std::iota(c.order.begin(), c.order.end(), 0);
    std::stable_sort(c.order.begin(), c.order.end(), [&](int32_t x, int32_t y) { return query_ref[x] < query_ref[y]; });
    if (n == 0) c.order.clear();
    return check_instance(c, cut_fit_loop(n, m_of, query_ref, ref_bytes, query_bytes, budget, overhead), it);
}

static int check_ctcalign(std::mt19937_64& rng, int it)
{
    const int n = draw_n(rng, it), max_launch = rng() % 3 ? 1 + (int)(rng() % 6) : 32768;
    std::vector<int64_t> bytes(n);
    for (int64_t& b : bytes) b = (draw_size(rng) + 255) / 256 * 256;
    const int64_t budget = draw_budget(rng, 0, bytes);
    const Config c{"ctcalign", n, {}, budget, 0, false, [&](int32_t i, int32_t) { return bytes[i]; },
                   [&](int32_t, int32_t, int64_t count, int64_t) { return count >= max_launch; }};
    return check_instance(c, cut_ctcalign_loop(n, bytes, budget, max_launch), it);
}

static int check_map(std::mt19937_64& rng, int it)
{
    const int n = draw_n(rng, it), max_reads = rng() % 3 ? 1 + (int)(rng() % 8) : 65535;
    const int64_t AB = 64, LB = rng() % 2 ? (int64_t)1 << 20 : 4096, cap = (int64_t)1 << 31;
    const bool huge = rng() % 8 == 0;   // anchor counts around 2^31: the cap on a read and on a launch
    std::vector<int64_t> read_a(n + 1, 0), alone(n);
    for (int r = 0; r < n; r++) {
        const int64_t a = rng() % 3 == 0 ? 0 : huge ? (int64_t)(rng() % (3 * (uint64_t)cap / 2)) : draw_size(rng) / 16;   // reads without anchors take no part
        read_a[r + 1] = read_a[r] + a;
        alone[r] = a * AB;
    }
    const int64_t budget = huge ? (rng() % 2 ? INT64_MAX : (int64_t)1 << (36 + rng() % 6)) : draw_budget(rng, LB, alone);
    const auto anchors = [&](int64_t r) { return read_a[r + 1] - read_a[r]; };
    const Config c{"map", n, {}, budget, LB, true,
                   [&](int32_t r, int32_t) -> int64_t {
                       const int64_t a = anchors(r);
                       return a == 0 ? -1 : a >= cap ? INT64_MAX : a * AB;
                   },
                   [&](int32_t r, int32_t r0, int64_t, int64_t acc) { return r + 1 - r0 > max_reads || acc / AB + anchors(r) >= cap; }};
    return check_instance(c, cut_map_loop(n, read_a, budget, AB, LB, max_reads), it);
}

static int check_polya(std::mt19937_64& rng, int it)
{
    const int n = draw_n(rng, it);
    std::vector<int64_t> bytes(n);
    for (int64_t& b : bytes) b = 2048 + draw_size(rng);
    const int64_t budget = draw_budget(rng, 0, bytes);
    const Config c{"polya", n, {}, budget, 0, false, [&](int32_t r, int32_t) { return bytes[r]; }, never};
    return check_instance(c, cut_polya_loop(n, bytes, budget), it);
}

int main(int argc, char** argv)
{
    const int iters = argc > 1 ? atoi(argv[1]) : 20000;
    std::mt19937_64 rng(23);
    for (int it = 0; it < iters; it++)
        if (check_align(rng, it) || check_fit(rng, it) || check_ctcalign(rng, it) || check_map(rng, it) || check_polya(rng, it)) return 1;
    // the default-budget rule: a quarter of free + held
    if (rd_default_budget(0, 0) != 0 || rd_default_budget(4000, 96) != 1024 || rd_default_budget((size_t)200 << 30, (size_t)56 << 30) != (int64_t)64 << 30) {
        printf("rd_default_budget is not a quarter of free + held\n");
        return 1;
    }
    printf("%d instances of each of 5 configurations, every property holds, the launches equal the replaced loops', no sanitizer report\n", iters);
    return 0;
}
