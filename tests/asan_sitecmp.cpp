// TEST INFRASTRUCTURE: AddressSanitizer + UBSan harness for the host side of radian_amd/csrc/sitecmp.hip (the argument check, the rules of
// site_rules.h, the counting pass, the launch plan, the bucketing and rd_site_compare_host; sanitizers run on the CPU build only -- the
// kernels are not compiled here).
// usage: asan_sitecmp <iterations>   Every iteration draws events of the test cases' shapes (depths around 1, 64, the chunk of 256 and three chunks;
// one-sided sites; the int16 extremes; site ids up to 2^32 - 2) into EXACT-SIZE heap buffers (a read or a write past either end is an ASan
// report), calls rd_site_compare_host and checks every entry against a quadratic count of its own; cuts the sites into launches under a
// random budget and checks that the buckets hold each launch's events and nothing else; then the same buffers go through the refusals,
// which must answer RD_ERR_ARG and write nothing.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <vector>

#include "../radian_amd/csrc/sitecmp.hip"   // the host half (this is no HIP build): the device blocks' layout functions live in its unnamed namespace

extern "C" int rd_site_compare_host(const uint32_t* site, const uint8_t* cond, const int16_t* value, int64_t n_events, uint32_t n_sites,
                                    int64_t capacity, uint32_t* out_site, int32_t* status, int64_t* n, int64_t* sum, int64_t* sumsq, int32_t* vmin,
                                    int32_t* vmax, int32_t* med2, int64_t* u2, int64_t* ks_num, int32_t* ks_x, int64_t* tie, int64_t* n_out);
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
    int32_t *status, *vmin, *vmax, *med2, *ks_x;
    int64_t *n, *sum, *sumsq, *u2, *ks_num, *tie, n_out;
    size_t cap;
    explicit Outs(size_t cap_) : cap(cap_)
    {
        const size_t m = cap ? cap : 1;
        site = (uint32_t*)malloc(m * 4), status = (int32_t*)malloc(m * 4), ks_x = (int32_t*)malloc(m * 4);
        vmin = (int32_t*)malloc(m * 8), vmax = (int32_t*)malloc(m * 8), med2 = (int32_t*)malloc(m * 8);
        n = (int64_t*)malloc(m * 16), sum = (int64_t*)malloc(m * 16), sumsq = (int64_t*)malloc(m * 16);
        u2 = (int64_t*)malloc(m * 8), ks_num = (int64_t*)malloc(m * 8), tie = (int64_t*)malloc(m * 8);
        n_out = 77;
        for (size_t i = 0; i < cap; i++) {
            site[i] = 77, status[i] = ks_x[i] = 77, u2[i] = ks_num[i] = tie[i] = 77;
            for (int c = 0; c < 2; c++) vmin[2 * i + c] = vmax[2 * i + c] = med2[2 * i + c] = 77, n[2 * i + c] = sum[2 * i + c] = sumsq[2 * i + c] = 77;
        }
    }
    ~Outs() { free(site), free(status), free(ks_x), free(vmin), free(vmax), free(med2), free(n), free(sum), free(sumsq), free(u2), free(ks_num), free(tie); }
    bool untouched() const
    {
        if (n_out != 77) return false;
        for (size_t i = 0; i < cap; i++) {
            if (site[i] != 77 || status[i] != 77 || ks_x[i] != 77 || u2[i] != 77 || ks_num[i] != 77 || tie[i] != 77) return false;
            for (int c = 0; c < 2; c++)
                if (vmin[2 * i + c] != 77 || vmax[2 * i + c] != 77 || med2[2 * i + c] != 77 || n[2 * i + c] != 77 || sum[2 * i + c] != 77 ||
                    sumsq[2 * i + c] != 77)
                    return false;
        }
        return true;
    }
    int call(const uint32_t* s, const uint8_t* c, const int16_t* v, int64_t ne, uint32_t ns, int64_t capacity)
    {
        return rd_site_compare_host(s, c, v, ne, ns, capacity, site, status, n, sum, sumsq, vmin, vmax, med2, u2, ks_num, ks_x, tie, &n_out);
    }
};

// The yardstick of sc_layout for a comparison: the take lambda and the offset list that sc_run held before the layout function replaced
// them, written out literally (extra_bytes = 0: a comparison asked for none); on seeded random dimensions (0 and 1 of each among them) the
// total and every block's offset must be equal.
static void check_layout()
{
    std::mt19937_64 rng(7);
    const size_t dims[] = {0, 1, 2, 31, 32, 33, 255, 256, 257};
    auto dim = [&](size_t big) { return rng() % 3 ? dims[rng() % 9] : (size_t)(rng() % big); };
    char* const base = (char*)((uintptr_t)1 << 32);
    for (int it = 0; it < 4000; it++) {
        const int64_t n = (int64_t)dim(3000000), S = (int64_t)dim(100000);
        const size_t tmp_bytes = dim(3000000), extra_bytes = 0;
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
        sc_layout(dry, n, S, tmp_bytes, -1, &W);
        CHECK(!W.in_site && !W.tmp && !W.psum);
        sc_layout(wet, n, S, tmp_bytes, -1, &W);
        CHECK(wet.at == at && dry.at == at && W.tmp_bytes == tmp_bytes);
        CHECK((char*)W.in_site == base + o_site && (char*)W.in_cond == base + o_cond && (char*)W.in_value == base + o_value && (char*)W.ka == base + o_ka &&
              (char*)W.kb == base + o_kb && (char*)W.flag == base + o_flag && (char*)W.pos == base + o_pos && (char*)W.seg_start == base + o_start &&
              (char*)W.n_chunk == base + o_chunk && (char*)W.item_off == base + o_item && (char*)W.n_seg == base + o_nseg && (char*)W.seg == base + o_seg &&
              (char*)W.out == base + o_out && (char*)W.tmp == base + o_tmp && (char*)W.psum == base + o_extra);
    }
}

int main(int argc, char** argv)
{
    const int iters = argc > 1 ? atoi(argv[1]) : 50;
    check_layout();
    std::mt19937_64 rng(20);
    // the key and the packed maximum at their extremes
    CHECK(sc_key(0xfffffffeu, 1, 32767) == (((uint64_t)0xfffffffeu << 17) | 0x1ffff) && sc_key_site(sc_key(0xfffffffeu, 1, -32768)) == 0xfffffffeu);
    CHECK(sc_key_value(sc_key(5, 0, -32768)) == -32768 && sc_key_value(sc_key(5, 1, 32767)) == 32767 && sc_key_cond(sc_key(5, 1, 0)) == 1);
    CHECK(sc_sort_bits(1) == 17 && sc_sort_bits(2) == 18 && sc_sort_bits(0xffffffffu) == 49 && sc_sort_bits(257) == 26);
    CHECK(sc_ks_pack((int64_t)1 << 38, -32768) < ((uint64_t)1 << 55) && sc_ks_x(sc_ks_pack(9, -32768)) == -32768 && sc_ks_x(sc_ks_pack(9, 32767)) == 32767);
    CHECK(sc_ks_pack(9, -5) > sc_ks_pack(9, -4) && sc_ks_pack(10, 100) > sc_ks_pack(9, -100) && sc_ks_num(sc_ks_pack(12345, 7)) == 12345);
    CHECK(sc_status(0, 5) == SC_ONE_SIDED && sc_status(5, 0) == SC_ONE_SIDED && sc_status(1 << 19, 1 << 19) == SC_OK && sc_status((1 << 19) + 1, 1 << 19) == SC_DEEP);
    for (int it = 0; it < iters; it++) {
        const bool wide = it % 5 == 4;
        const uint32_t n_sites = wide ? 0xffffffffu : 1 + (uint32_t)(rng() % 40);
        const int depths[] = {1, 2, 63, 64, 65, 255, 256, 257, 773, 30};
        std::map<uint32_t, std::vector<int>> val[2];
        std::vector<uint32_t> site;
        std::vector<uint8_t> cond;
        std::vector<int16_t> value;
        const int ns = 1 + (int)(rng() % 6);
        for (int j = 0; j < ns; j++) {
            const uint32_t s = wide ? (j == 0 ? 0xfffffffeu : (uint32_t)(rng() % 0xfffffffeu)) : (uint32_t)(rng() % n_sites);
            const int d = depths[rng() % 10], mode = (int)(rng() % 4);   // mode 0: one-sided; 3: the extremes
            for (int e = 0; e < d; e++) {
                const int c = mode == 0 ? j & 1 : (int)(rng() & 1);
                const int v = mode == 3 ? (rng() & 1 ? 32767 : -32768) : (int)(rng() % 21) - 10;
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
            CHECK(o.call(ps, pc, pv, ne, n_sites, nd) == 0 && o.n_out == nd);
            g_accepted++;
            int64_t j = 0;
            for (const auto& kv : distinct) {
                const std::vector<int>&a = val[0][kv.first], &b = val[1][kv.first];
                CHECK(o.site[j] == kv.first && o.n[2 * j] == (int64_t)a.size() && o.n[2 * j + 1] == (int64_t)b.size());
                CHECK(o.status[j] == (a.empty() || b.empty() ? SC_ONE_SIDED : SC_OK));
                int64_t s0 = 0, q0 = 0, u2 = 0;
                for (int x : a) {
                    s0 += x, q0 += (int64_t)x * x;
                    for (int y : b) u2 += y < x ? 2 : y == x ? 1 : 0;
                }
                CHECK(o.sum[2 * j] == s0 && o.sumsq[2 * j] == q0);
                if (o.status[j] != SC_OK) {
                    CHECK(o.u2[j] == 0 && o.ks_num[j] == 0 && o.ks_x[j] == 0 && o.tie[j] == 0);
                } else {
                    int64_t best = -1, tie = 0;
                    int best_x = 0;
                    for (int x = -32768; x <= 32767; x = x == -32768 ? -10 : x == 10 ? 32767 : x + 1) {   // the values drawn above
                        int64_t ca = 0, cb = 0, t = 0;
                        for (int y : a) ca += y <= x, t += y == x;
                        for (int y : b) cb += y <= x, t += y == x;
                        if (!t) continue;
                        tie += t * t * t - t;
                        const int64_t d = llabs(ca * (int64_t)b.size() - cb * (int64_t)a.size());
                        if (d > best) best = d, best_x = x;
                    }
                    CHECK(o.u2[j] == u2 && o.tie[j] == tie && o.ks_num[j] == best && o.ks_x[j] == best_x);
                }
                j++;
            }
        }
        {   // the plan and the buckets under a random budget: every launch holds its sites' events and nothing else
            std::vector<ScSite> sites;
            CHECK(sc_count_sites(ps, pc, ne, n_sites, sites) == -1 && (int64_t)sites.size() == nd);
            const int64_t budget = SC_EVENT_BYTES * (1 + (int64_t)(rng() % 1100));
            const BudgetPlan plan = sc_plan(sites, budget);
            std::vector<int64_t> off;
            std::vector<uint32_t> gs;
            std::vector<uint8_t> gc;
            std::vector<int16_t> gv;
            sc_bucket(ps, pc, pv, ne, sites, plan, off, gs, gc, gv);
            int64_t launched = 0, left_out = 0;
            for (size_t l = 0; l < plan.launches.size(); l++) {
                int64_t want = 0;
                std::map<uint32_t, int64_t> members;
                for (int64_t k = plan.launches[l].first; k < plan.launches[l].second; k++) {
                    const ScSite& s = sites[plan.run[k]];
                    CHECK(sc_site_bytes(s) <= budget);
                    members[s.site] = s.n[0] + s.n[1];
                    want += s.n[0] + s.n[1];
                }
                CHECK(off[l + 1] - off[l] == want && SC_EVENT_BYTES * want <= budget);
                for (int64_t i = off[l]; i < off[l + 1]; i++) CHECK(members.count(gs[i]) && members[gs[i]]-- > 0 && gc[i] <= 1);
                launched += want;
            }
            for (const ScSite& s : sites)
                if (sc_site_bytes(s) > budget) left_out += s.n[0] + s.n[1];
            CHECK(launched + left_out == ne && (int64_t)gs.size() == launched && (plan.too_large > 0) == (left_out > 0));
        }
        {   // the refusals
            Outs o((size_t)nd);
            CHECK(o.call(nullptr, pc, pv, ne, n_sites, nd) == -1 && o.untouched());
            g_refused++;
            CHECK(o.call(ps, nullptr, pv, ne, n_sites, nd) == -1 && o.untouched());
            g_refused++;
            CHECK(o.call(ps, pc, nullptr, ne, n_sites, nd) == -1 && o.untouched());
            g_refused++;
            CHECK(o.call(ps, pc, pv, (int64_t)1 << 31, n_sites, nd) == -1 && o.untouched());
            g_refused++;
            CHECK(o.call(ps, pc, pv, -1, n_sites, nd) == -1 && o.untouched());
            g_refused++;
            CHECK(o.call(ps, pc, pv, ne, n_sites, nd - 1) == -1 && o.untouched());
            g_refused++;
            uint32_t top = 0;
            for (uint32_t s : site) top = s > top ? s : top;
            CHECK(o.call(ps, pc, pv, ne, top, nd) == -1 && o.untouched());
            g_refused++;      // n_sites == the largest site
            pc[rng() % ne] = 2;
            CHECK(o.call(ps, pc, pv, ne, n_sites, nd) == -1 && o.untouched());
            g_refused++;
        }
        {
            Outs o(0);
            CHECK(o.call(nullptr, nullptr, nullptr, 0, n_sites, 0) == 0 && o.n_out == 0);
            g_accepted++;
        }
        free(ps), free(pc), free(pv);
    }
    printf("no sanitizer report\n%ld accepted %ld refused\n", g_accepted, g_refused);
    return 0;
}
