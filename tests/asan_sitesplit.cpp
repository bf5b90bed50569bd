// TEST INFRASTRUCTURE: AddressSanitizer + UBSan harness for the host side of the two-cluster split in radian_amd/csrc/sitecmp.hip (the
// argument check, the rules of site_rules.h, the launch plan under rd_site_split_workspace_bytes, the bucketing and rd_site_split_host;
// sanitizers run on the CPU build only -- the kernels are not compiled here).
// usage: asan_sitesplit <iterations>   Every iteration draws events of the test cases' shapes (depths around 1, 64, the chunk of 256 and three
// chunks; one-sided sites; all values equal; the int16 extremes; site ids up to 2^32 - 2) into EXACT-SIZE heap buffers (a read or a write
// past either end is an ASan report), calls rd_site_split_host under a random min_frac_q16 and checks every entry against a quadratic search
// of its own over 128-bit cross products; cuts the sites into launches under a random budget and checks that the buckets hold each
// launch's events and nothing else; then the same buffers go through the refusals, which must answer RD_ERR_ARG and write nothing.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "../radian_amd/csrc/sitecmp.hip"   // the host half (this is no HIP build): the device blocks' layout functions live in its unnamed namespace

extern "C" int rd_site_split_host(const uint32_t* site, const uint8_t* cond, const int16_t* value, int64_t n_events, uint32_t n_sites,
                                  int64_t capacity, int min_frac_q16, uint32_t* out_site, int32_t* status, int64_t* n, int64_t* sum, int64_t* sumsq,
                                  int32_t* cut, int32_t* n_cuts, int64_t* n_lo, int64_t* sum_lo, int64_t* sumsq_lo, int64_t* n_out);
extern "C" int64_t rd_site_split_workspace_bytes(int64_t n_events);
void rd_set_error(const char* fmt, ...) { (void)fmt; }

static long g_accepted = 0, g_refused = 0;

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            printf("line %d: %s does not hold\n", __LINE__, #cond);     \
            exit(1);                                                     \
        }                                                                \
    } while (0)

template <typename T> static T* exact(const std::vector<T>& v)
{
    T* p = (T*)malloc(v.size() ? v.size() * sizeof(T) : 1);
    if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

struct Outs {
    uint32_t* site;
    int32_t *status, *cut, *n_cuts;
    int64_t *n, *sum, *sumsq, *n_lo, *sum_lo, *sumsq_lo, n_out;
    size_t cap;
    explicit Outs(size_t cap_) : cap(cap_)
    {
        const size_t m = cap ? cap : 1;
        site = (uint32_t*)malloc(m * 4), status = (int32_t*)malloc(m * 4), cut = (int32_t*)malloc(m * 4), n_cuts = (int32_t*)malloc(m * 4);
        n = (int64_t*)malloc(m * 16), sum = (int64_t*)malloc(m * 16), sumsq = (int64_t*)malloc(m * 16);
        n_lo = (int64_t*)malloc(m * 16), sum_lo = (int64_t*)malloc(m * 16), sumsq_lo = (int64_t*)malloc(m * 16);
        n_out = 77;
        for (size_t i = 0; i < cap; i++) {
            site[i] = 77, status[i] = cut[i] = n_cuts[i] = 77;
            for (int c = 0; c < 2; c++) n[2 * i + c] = sum[2 * i + c] = sumsq[2 * i + c] = n_lo[2 * i + c] = sum_lo[2 * i + c] = sumsq_lo[2 * i + c] = 77;
        }
    }
    ~Outs() { free(site), free(status), free(cut), free(n_cuts), free(n), free(sum), free(sumsq), free(n_lo), free(sum_lo), free(sumsq_lo); }
    bool untouched() const
    {
        if (n_out != 77) return false;
        for (size_t i = 0; i < cap; i++) {
            if (site[i] != 77 || status[i] != 77 || cut[i] != 77 || n_cuts[i] != 77) return false;
            for (int c = 0; c < 2; c++)
                if (n[2 * i + c] != 77 || sum[2 * i + c] != 77 || sumsq[2 * i + c] != 77 || n_lo[2 * i + c] != 77 || sum_lo[2 * i + c] != 77 ||
                    sumsq_lo[2 * i + c] != 77)
                    return false;
        }
        return true;
    }
    int call(const uint32_t* s, const uint8_t* c, const int16_t* v, int64_t ne, uint32_t ns, int64_t capacity, int mf)
    {
        return rd_site_split_host(s, c, v, ne, ns, capacity, mf, site, status, n, sum, sumsq, cut, n_cuts, n_lo, sum_lo, sumsq_lo, &n_out);
    }
};

// The yardstick of sc_layout for a split: the take lambda and the offset list that sc_run held, and the sizes and pointers of the split's
// own arrays behind them that rd_site_split held, before the layout function replaced them -- written out literally; on seeded random
// dimensions (0 and 1 of each among them) the total and every block's offset must be equal.
static void check_layout()
{
    std::mt19937_64 rng(7);
    const size_t dims[] = {0, 1, 2, 31, 32, 33, 255, 256, 257};
    auto dim = [&](size_t big) { return rng() % 3 ? dims[rng() % 9] : (size_t)(rng() % big); };
    char* const base = (char*)((uintptr_t)1 << 32);
    for (int it = 0; it < 4000; it++) {
        const int64_t n = (int64_t)dim(3000000), S = (int64_t)dim(100000), items = (int64_t)dim(200000), nl = n;
        const size_t tmp_bytes = dim(3000000);
        const size_t b_pre = align_up((size_t)nl * 8, 256), b_slot = align_up((size_t)items * sizeof(SsSlot), 256), b_cnt = align_up((size_t)S * 4, 256);
        const size_t extra_bytes = 2 * b_pre + b_slot + b_cnt + (size_t)S * sizeof(SsOut);
        size_t at = 0;
        const auto take = [&](size_t bytes) {
            const size_t o = at;
            at += align_up(bytes + 8, 256);
            return o;
        };
        const size_t o_site = take((size_t)n * 4), o_cond = take((size_t)n), o_value = take((size_t)n * 2), o_ka = take((size_t)n * 8),
                     o_kb = take((size_t)n * 8), o_flag = take((size_t)n * 4), o_pos = take((size_t)n * 4), o_start = take((size_t)(S + 1) * 4),
                     o_chunk = take((size_t)(S + 1) * 4), o_item = take((size_t)(S + 1) * 4), o_nseg = take(4), o_seg = take((size_t)S * sizeof(ScSeg)),
                     o_out = take((size_t)S * sizeof(ScOut)), o_tmp = take(tmp_bytes), o_extra = take(extra_bytes);
        ScWs W;
        Carve dry, wet(base);
        sc_layout(dry, n, S, tmp_bytes, items, &W);
        CHECK(!W.in_site && !W.tmp && !W.psum && !W.split_out);
        sc_layout(wet, n, S, tmp_bytes, items, &W);
        CHECK(wet.at == at && dry.at == at && W.tmp_bytes == tmp_bytes);
        CHECK((char*)W.in_site == base + o_site && (char*)W.in_cond == base + o_cond && (char*)W.in_value == base + o_value && (char*)W.ka == base + o_ka &&
              (char*)W.kb == base + o_kb && (char*)W.flag == base + o_flag && (char*)W.pos == base + o_pos && (char*)W.seg_start == base + o_start &&
              (char*)W.n_chunk == base + o_chunk && (char*)W.item_off == base + o_item && (char*)W.n_seg == base + o_nseg && (char*)W.seg == base + o_seg &&
              (char*)W.out == base + o_out && (char*)W.tmp == base + o_tmp && (char*)W.psum == base + o_extra);
        char* const extra = base + o_extra;
        CHECK((char*)W.psum == extra && (char*)W.psq == extra + b_pre && (char*)W.slot == extra + 2 * b_pre && (char*)W.cnt == extra + 2 * b_pre + b_slot &&
              (char*)W.split_out == extra + 2 * b_pre + b_slot + b_cnt);
    }
}

int main(int argc, char** argv)
{
    const int iters = argc > 1 ? atoi(argv[1]) : 50;
    check_layout();
    std::mt19937_64 rng(26);
    // the order of two candidates at the extremes: |D| = 2^46 at n_lo = n_hi = 2^15 against one unit less
    {
        const SsCand top{(uint64_t)1 << 46, 1u << 15, 1u << 15, 5}, less{((uint64_t)1 << 46) - 1, 1u << 15, 1u << 15, -5}, none{0, 0, 0, 0};
        CHECK(ss_better(top, less) && !ss_better(less, top) && ss_better(less, none) && !ss_better(none, less) && !ss_better(none, none));
        const SsCand same_lo{(uint64_t)1 << 46, 1u << 15, 1u << 15, 4};
        CHECK(ss_better(same_lo, top) && !ss_better(top, same_lo));                     // equal scores: the smaller cut
        const SsCand a{12, 2, 4, 0}, b{12, 4, 2, 1};                                    // the tie of the values 0 1 2
        CHECK(ss_better(a, b) && !ss_better(b, a));
        CHECK(ss_status(0, 5) == SC_ONE_SIDED && ss_status(1 << 15, 1 << 15) == SC_OK && ss_status((1 << 15) + 1, 1 << 15) == SC_DEEP);
        CHECK(ss_bytes(0) == 0 && ss_bytes(1) == 176 + 112 && ss_bytes(256) == 176 * 256 + 112 && ss_bytes(257) == 176 * 257 + 224);
        CHECK(rd_site_split_workspace_bytes(257) == ss_bytes(257) && rd_site_split_workspace_bytes(-1) == -1);
    }
    for (int it = 0; it < iters; it++) {
        const bool wide = it % 5 == 4;
        const uint32_t n_sites = wide ? 0xffffffffu : 1 + (uint32_t)(rng() % 40);
        const int mf = it % 3 == 0 ? 0 : it % 3 == 1 ? (int)(rng() % 32769) : 32768;
        const int depths[] = {1, 2, 3, 63, 64, 65, 255, 256, 257, 773};
        std::map<uint32_t, std::vector<int>> val[2];
        std::vector<uint32_t> site;
        std::vector<uint8_t> cond;
        std::vector<int16_t> value;
        const int ns = 1 + (int)(rng() % 6);
        for (int j = 0; j < ns; j++) {
            const uint32_t s = wide ? (j == 0 ? 0xfffffffeu : (uint32_t)(rng() % 0xfffffffeu)) : (uint32_t)(rng() % n_sites);
            const int d = depths[rng() % 10], mode = (int)(rng() % 5);   // mode 0: one-sided; 3: the extremes; 4: all equal
            for (int e = 0; e < d; e++) {
                const int c = mode == 0 ? j & 1 : (int)(rng() & 1);
                const int v = mode == 3 ? (rng() & 1 ? 32767 : -32768) : mode == 4 ? 9 : (int)(rng() % 21) - 10 + (rng() % 3 == 0 ? 40 : 0);
                site.push_back(s), cond.push_back((uint8_t)c), value.push_back((int16_t)v);
                val[c][s].push_back(v);
            }
        }
        for (size_t i = site.size(); i > 1; i--) {   // no site contiguous
            const size_t k = rng() % i;
            std::swap(site[i - 1], site[k]), std::swap(cond[i - 1], cond[k]), std::swap(value[i - 1], value[k]);
        }
        std::map<uint32_t, int> distinct;
        for (uint32_t s : site) distinct[s]++;
        const int64_t ne = (int64_t)site.size(), nd = (int64_t)distinct.size();
        uint32_t* ps = exact(site);
        uint8_t* pc = exact(cond);
        int16_t* pv = exact(value);
        {
            Outs o((size_t)nd);
            CHECK(o.call(ps, pc, pv, ne, n_sites, nd, mf) == 0 && o.n_out == nd);
            g_accepted++;
            int64_t j = 0;
            for (const auto& kv : distinct) {
                const std::vector<int>&a = val[0][kv.first], &b = val[1][kv.first];
                CHECK(o.site[j] == kv.first && o.n[2 * j] == (int64_t)a.size() && o.n[2 * j + 1] == (int64_t)b.size());
                int64_t s0 = 0, q0 = 0, s1 = 0, q1 = 0;
                for (int x : a) s0 += x, q0 += (int64_t)x * x;
                for (int x : b) s1 += x, q1 += (int64_t)x * x;
                CHECK(o.sum[2 * j] == s0 && o.sumsq[2 * j] == q0 && o.sum[2 * j + 1] == s1 && o.sumsq[2 * j + 1] == q1);
                // a search of its own: every value present as a cut, counts and sums by a pass over the site
                const int64_t N = (int64_t)(a.size() + b.size());
                std::set<int> xs(a.begin(), a.end());
                xs.insert(b.begin(), b.end());
                bool any = false;
                int best_cut = 0, n_adm = 0;
                unsigned __int128 best_d2 = 0;
                uint64_t best_m = 1;
                if (!a.empty() && !b.empty())
                    for (int x : xs) {
                        int64_t nl = 0, sl = 0;
                        for (int y : a) nl += y <= x, sl += y <= x ? y : 0;
                        for (int y : b) nl += y <= x, sl += y <= x ? y : 0;
                        const int64_t nh = N - nl;
                        if (nh < 1 || 65536 * nl < (int64_t)mf * N || 65536 * nh < (int64_t)mf * N) continue;
                        n_adm++;
                        const int64_t D = sl * nh - (s0 + s1 - sl) * nl;
                        const unsigned __int128 d2 = (unsigned __int128)(uint64_t)(D < 0 ? -D : D) * (uint64_t)(D < 0 ? -D : D);
                        const uint64_t m = (uint64_t)nl * (uint64_t)nh;
                        if (!any || d2 * best_m > best_d2 * m) any = true, best_cut = x, best_d2 = d2, best_m = m;   // ascending x, strict: the smallest
                    }
                const int want = a.empty() || b.empty() ? SC_ONE_SIDED : !any ? SS_NONE : SC_OK;
                CHECK(o.status[j] == want);
                if (want != SC_OK) {
                    CHECK(o.cut[j] == 0 && o.n_cuts[j] == 0 && o.n_lo[2 * j] == 0 && o.n_lo[2 * j + 1] == 0 && o.sum_lo[2 * j] == 0 && o.sum_lo[2 * j + 1] == 0 &&
                          o.sumsq_lo[2 * j] == 0 && o.sumsq_lo[2 * j + 1] == 0);
                } else {
                    int64_t nl[2] = {0, 0}, sl[2] = {0, 0}, ql[2] = {0, 0};
                    for (int y : a)
                        if (y <= best_cut) nl[0]++, sl[0] += y, ql[0] += (int64_t)y * y;
                    for (int y : b)
                        if (y <= best_cut) nl[1]++, sl[1] += y, ql[1] += (int64_t)y * y;
                    CHECK(o.cut[j] == best_cut && o.n_cuts[j] == n_adm);
                    for (int c = 0; c < 2; c++) CHECK(o.n_lo[2 * j + c] == nl[c] && o.sum_lo[2 * j + c] == sl[c] && o.sumsq_lo[2 * j + c] == ql[c]);
                }
                j++;
            }
        }
        {   // the plan and the buckets under a random budget: every launch holds its sites' events and nothing else
            std::vector<ScSite> sites;
            CHECK(sc_count_sites(ps, pc, ne, n_sites, sites) == -1 && (int64_t)sites.size() == nd);
            const int64_t budget = ss_bytes(1 + (int64_t)(rng() % 1100));
            const BudgetPlan plan = ss_plan(sites, budget);
            std::vector<int64_t> off;
            std::vector<uint32_t> gs;
            std::vector<uint8_t> gc;
            std::vector<int16_t> gv;
            sc_bucket(ps, pc, pv, ne, sites, plan, off, gs, gc, gv);
            int64_t launched = 0, left_out = 0;
            for (size_t l = 0; l < plan.launches.size(); l++) {
                int64_t want = 0, bytes = 0;
                std::map<uint32_t, int64_t> members;
                for (int64_t k = plan.launches[l].first; k < plan.launches[l].second; k++) {
                    const ScSite& s = sites[plan.run[k]];
                    CHECK(ss_site_bytes(s) <= budget && ss_site_bytes(s) == rd_site_split_workspace_bytes(s.n[0] + s.n[1]));
                    members[s.site] = s.n[0] + s.n[1];
                    want += s.n[0] + s.n[1];
                    bytes += ss_site_bytes(s);
                }
                CHECK(off[l + 1] - off[l] == want && bytes <= budget);
                for (int64_t i = off[l]; i < off[l + 1]; i++) CHECK(members.count(gs[i]) && members[gs[i]]-- > 0 && gc[i] <= 1);
                launched += want;
            }
            for (const ScSite& s : sites)
                if (ss_site_bytes(s) > budget) left_out += s.n[0] + s.n[1];
            CHECK(launched + left_out == ne && (int64_t)gs.size() == launched && (plan.too_large > 0) == (left_out > 0));
        }
        {   // the refusals
            Outs o((size_t)nd);
            CHECK(o.call(nullptr, pc, pv, ne, n_sites, nd, mf) == -1 && o.untouched());
            g_refused++;
            CHECK(o.call(ps, nullptr, pv, ne, n_sites, nd, mf) == -1 && o.untouched());
            g_refused++;
            CHECK(o.call(ps, pc, nullptr, ne, n_sites, nd, mf) == -1 && o.untouched());
            g_refused++;
            CHECK(o.call(ps, pc, pv, (int64_t)1 << 31, n_sites, nd, mf) == -1 && o.untouched());
            g_refused++;
            CHECK(o.call(ps, pc, pv, -1, n_sites, nd, mf) == -1 && o.untouched());
            g_refused++;
            CHECK(o.call(ps, pc, pv, ne, n_sites, nd - 1, mf) == -1 && o.untouched());
            g_refused++;
            CHECK(o.call(ps, pc, pv, ne, n_sites, nd, -1) == -1 && o.untouched());
            g_refused++;
            CHECK(o.call(ps, pc, pv, ne, n_sites, nd, 32769) == -1 && o.untouched());
            g_refused++;
            uint32_t top = 0;
            for (uint32_t s : site) top = s > top ? s : top;
            CHECK(o.call(ps, pc, pv, ne, top, nd, mf) == -1 && o.untouched());
            g_refused++;      // n_sites == the largest site
            pc[rng() % ne] = 2;
            CHECK(o.call(ps, pc, pv, ne, n_sites, nd, mf) == -1 && o.untouched());
            g_refused++;
        }
        {
            Outs o(0);
            CHECK(o.call(nullptr, nullptr, nullptr, 0, n_sites, 0, mf) == 0 && o.n_out == 0);
            g_accepted++;
        }
        free(ps), free(pc), free(pv);
    }
    printf("no sanitizer report\n%ld accepted %ld refused\n", g_accepted, g_refused);
    return 0;
}
