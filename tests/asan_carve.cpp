// TEST INFRASTRUCTURE: AddressSanitizer + UBSan harness for radian_amd/csrc/carve.h -- the one workspace carver of the stage entry points and
// the run walker of their gathers (sanitizers run on the CPU build only; carve.h holds no HIP type).
// usage: asan_carve <iterations>   Every iteration draws a seeded random block list (element sizes 1, 2, 4, 8, 16 and 24; counts with 0 and
// 1; slacks 0, 1, 8, 16, 256; alignments 256, 4 and 1; a start offset) and a random gather (reads with lengths 0 among them, a subset of
// members in order), and checks the properties that a stage's layout function and its gather rest on.  The blocks are carved out of an
// EXACT-SIZE heap buffer and every block is written end to end: a block past the dry total is an ASan report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <utility>
#include <vector>

#include "../radian_amd/csrc/carve.h"

#define CHECK(cond, ...)                                                          \
    do {                                                                          \
        if (!(cond)) {                                                            \
            printf("property violated: %s  (", #cond);                           \
            printf(__VA_ARGS__);                                                  \
            printf(")\n");                                                        \
            return 1;                                                             \
        }                                                                         \
    } while (0)

struct E24 {
    char b[24];
};
struct Block {
    int esize;
    size_t count, slack, align;
};
struct Got {
    char* p;
    size_t mark;
};

static Got take_one(Carve& c, const Block& b)
{
    Got g;
    g.mark = c.mark();
    switch (b.esize) {
    case 1: g.p = (char*)c.take<uint8_t>(b.count, b.slack, b.align); break;
    case 2: g.p = (char*)c.take<int16_t>(b.count, b.slack, b.align); break;
    case 4: g.p = (char*)c.take<int32_t>(b.count, b.slack, b.align); break;
    case 8: g.p = (char*)c.take<int64_t>(b.count, b.slack, b.align); break;
    case 16: g.p = (char*)c.take<int64_t[2]>(b.count, b.slack, b.align); break;
    default: g.p = (char*)c.take<E24>(b.count, b.slack, b.align); break;
    }
    return g;
}

static int check_carve(std::mt19937_64& rng, int it)
{
    auto uni = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); };
    static const int esizes[] = {1, 2, 4, 8, 16, 24};
    static const size_t slacks[] = {0, 0, 1, 8, 16, 256}, aligns[] = {256, 256, 256, 4, 1};
    const int nblk = (int)uni(0, 16);
    const size_t at0 = it % 3 == 0 ? 256 * uni(0, 8) : 0;
    std::vector<Block> blocks(nblk);
    for (Block& b : blocks) {
        const int kind = (int)uni(0, 5);
        b = Block{esizes[uni(0, 5)], kind == 0 ? 0 : kind == 1 ? 1 : kind == 2 ? (size_t)uni(2, 70) : (size_t)uni(0, 5000), slacks[uni(0, 5)],
                  aligns[uni(0, 4)]};
    }
    // the dry pass: null pointers, the same marks
    Carve dry(nullptr, at0);
    CHECK(dry.base == nullptr && dry.mark() == at0, "it %d", it);
    std::vector<size_t> marks;
    for (const Block& b : blocks) {
        const Got g = take_one(dry, b);
        CHECK(g.p == nullptr, "it %d: a dry pass gave a pointer", it);
        marks.push_back(g.mark);
    }
    const size_t total = dry.at;
    CHECK(dry.fits(total) && (total == 0 || !dry.fits(total - 1)) && dry.fits(total + 1), "it %d: fits() around %zu", it, total);
    // the wet pass in a buffer of exactly the dry total (256-aligned, as hipMalloc's are)
    char* buf = (char*)aligned_alloc(256, total ? (total + 255) / 256 * 256 : 256);
    char* raw = (char*)malloc(total ? total : 1);   // exact size: the writes below must stay inside it
    Carve wet(buf, at0);
    size_t prev_end = at0;
    bool all256 = true;
    for (int i = 0; i < nblk; i++) {
        const Block& b = blocks[i];
        const Got g = take_one(wet, b);
        const size_t o = (size_t)(g.p - buf), need = b.count * (size_t)b.esize + b.slack, len = wet.mark() - o;
        CHECK(g.mark == marks[i] && o == marks[i], "it %d block %d: mark %zu, dry mark %zu, pointer offset %zu", it, i, g.mark, marks[i], o);
        CHECK(o == prev_end, "it %d block %d: starts at %zu, the block before ended at %zu (disjoint, in order, no hole)", it, i, o, prev_end);
        CHECK(len >= need && len < need + b.align && len % b.align == 0, "it %d block %d: %zu bytes for %zu at alignment %zu", it, i, len, need, b.align);
        if (all256) CHECK(o % 256 == 0 && ((uintptr_t)g.p) % 256 == 0, "it %d block %d: offset %zu is not 256-aligned", it, i, o);
        all256 = all256 && b.align == 256;   // (a block behind an unrounded one starts where that one ended, as align.hip's op slots do)
        memset(raw + o, i, len);             // inside the exact-size buffer, or ASan reports it
        prev_end = o + len;
    }
    CHECK(wet.at == total && wet.mark() == total, "it %d: the wet pass ends at %zu, the dry one at %zu", it, wet.at, total);
    Carve r(nullptr, total);
    r.round();
    CHECK(r.at >= total && r.at < total + 256 && r.at % 256 == 0, "it %d: round() of %zu gave %zu", it, total, r.at);
    free(raw);
    free(buf);
    return 0;
}

// the runs of members against src_off, with the properties checked
static int check_runs(const std::vector<int64_t>& src_off, const std::vector<int32_t>& members, int it, std::vector<std::pair<int64_t, int64_t>>* out)
{
    const int64_t n = (int64_t)members.size();
    std::vector<std::pair<int64_t, int64_t>> runs;
    rd_gather_runs(members.data(), n, src_off.data(), [&](int64_t i, int64_t k) { runs.push_back({i, k}); });
    std::vector<int64_t> off;
    rd_gather_offsets(src_off.data(), members.data(), n, off);
    CHECK((int64_t)off.size() == n + 1 && off[0] == 0, "it %d", it);
    for (int64_t i = 0; i < n; i++)
        CHECK(off[i + 1] - off[i] == src_off[members[i] + 1] - src_off[members[i]], "it %d: member %lld", it, (long long)i);
    int64_t at = 0;
    for (size_t r = 0; r < runs.size(); r++) {
        const auto [i, k] = runs[r];
        CHECK(i == at && k > i && k <= n, "it %d: run %zu is [%lld, %lld), the one before ended at %lld (the runs tile the members in order)", it, r,
              (long long)i, (long long)k, (long long)at);
        // contiguous in the source: one copy of off[k] - off[i] elements from src_off[members[i]] moves exactly the members' elements
        CHECK(src_off[members[k - 1] + 1] - src_off[members[i]] == off[k] - off[i], "it %d run %zu: the source span and the members' elements differ", it, r);
        for (int64_t j = i; j < k; j++)
            CHECK(src_off[members[j]] - src_off[members[i]] == off[j] - off[i], "it %d run %zu: member %lld is not where the copy puts it", it, r, (long long)j);
        if (r + 1 < runs.size())   // maximal: the next run does not start where this one ends
            CHECK(src_off[members[k]] != src_off[members[k - 1] + 1], "it %d: runs %zu and %zu could have been one", it, r, r + 1);
        at = k;
    }
    CHECK(at == n, "it %d: the runs end at %lld of %lld members", it, (long long)at, (long long)n);
    if (out) *out = runs;
    return 0;
}

static int check_gather(std::mt19937_64& rng, int it)
{
    auto uni = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); };
    const int n_reads = (int)uni(1, 24);
    std::vector<int64_t> src_off(1, (int64_t)uni(0, 5));
    for (int r = 0; r < n_reads; r++) src_off.push_back(src_off.back() + (uni(0, 2) == 0 ? 0 : (int64_t)uni(1, 40)));
    std::vector<int32_t> members;
    const int keep = (int)uni(0, 3);   // 0: every read; otherwise about keep in four are left out
    for (int r = 0; r < n_reads; r++)
        if (keep == 0 || uni(0, 3) >= (uint64_t)keep - 1 || uni(0, 1)) members.push_back(r);
    std::vector<std::pair<int64_t, int64_t>> runs;
    if (check_runs(src_off, members, it, &runs)) return 1;
    // a zero-length member never splits a run: without the empty reads the runs cover the same elements in as many copies at most
    std::vector<int32_t> full;
    for (int32_t m : members)
        if (src_off[m + 1] > src_off[m]) full.push_back(m);
    std::vector<std::pair<int64_t, int64_t>> runs_full;
    if (check_runs(src_off, full, it, &runs_full)) return 1;
    size_t with_elements = 0;
    for (auto [i, k] : runs) with_elements += src_off[members[k - 1] + 1] > src_off[members[i]] ? 1 : 0;
    CHECK(with_elements <= runs_full.size(), "it %d: %zu copies with the empty members, %zu without", it, with_elements, runs_full.size());
    // never more copies than the test by consecutive indices that poly(A) and the simulator used
    size_t by_index = 0;
    for (size_t i = 0; i < members.size(); i++) by_index += i == 0 || members[i] != members[i - 1] + 1 ? 1 : 0;
    CHECK(runs.size() <= by_index, "it %d: %zu runs, %zu by consecutive indices", it, runs.size(), by_index);
    return 0;
}

static int fixed_cases()
{
    typedef std::vector<std::pair<int64_t, int64_t>> Runs;
    Runs runs;
    // a skipped empty read between two members: one run
    if (check_runs({0, 10, 10, 25}, {0, 2}, -1, &runs)) return 1;
    CHECK(runs == Runs({{0, 2}}), "a skipped empty read split the run");
    // a skipped read with samples: two runs
    if (check_runs({0, 10, 14, 25}, {0, 2}, -2, &runs)) return 1;
    CHECK(runs == Runs({{0, 1}, {1, 2}}), "a skipped read with samples did not split the run");
    // a single member
    if (check_runs({3, 9}, {0}, -3, &runs)) return 1;
    CHECK(runs == Runs({{0, 1}}), "a single member");
    // every read empty: one run without elements (the gather issues no copy for it)
    if (check_runs({7, 7, 7, 7}, {0, 1, 2}, -4, &runs)) return 1;
    CHECK(runs == Runs({{0, 3}}), "reads without samples");
    // empty members inside and at the ends of a run
    if (check_runs({0, 0, 5, 5, 9, 9}, {0, 1, 2, 3, 4}, -5, &runs)) return 1;
    CHECK(runs == Runs({{0, 5}}), "empty members split a run");
    // no member at all
    if (check_runs({0, 4}, {}, -6, &runs)) return 1;
    CHECK(runs.empty(), "no members, but a run");
    return 0;
}

int main(int argc, char** argv)
{
    const int iters = argc > 1 ? atoi(argv[1]) : 4000;
    std::mt19937_64 rng(31);
    if (fixed_cases()) return 1;
    for (int it = 0; it < iters; it++)
        if (check_carve(rng, it) || check_gather(rng, it)) return 1;
    printf("%d block lists and gathers, every property holds, no sanitizer report\n", iters);
    return 0;
}
