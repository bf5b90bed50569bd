// site_rules.h -- the rules of the two-sample site comparison (include/radian_hip.h, rd_site_compare), once: the
// argument check, the host twin (rd_site_compare_host), the host's counting pass and launch plan, and the kernels of sitecmp.hip all call
// these.  So do the rules of the exact two-cluster split (rd_site_split): its host twin, plan and kernels.
// Integer arithmetic only; plain C++ without a HIP type (tests/asan_sitecmp.cpp and tests/asan_sitesplit.cpp compile it with g++).
#pragma once
#include <stdint.h>
#include <algorithm>
#include <unordered_map>
#include <utility>
#include <vector>

#include "budget.h"

#if defined(__HIPCC__)
#define SC_HD __host__ __device__
#else
#define SC_HD
#endif

// per-site status (radian_hip.h RD_SITE_*)
constexpr int SC_OK = 0, SC_ONE_SIDED = 1, SC_DEEP = 2, SC_TOO_LARGE = 3;
constexpr int64_t SC_DEEP_LIMIT = (int64_t)1 << 20;   // n0 + n1 above this: no rank statistics
constexpr int SC_CHUNK = 256;                         // elements of a site one wave of the site kernel takes
constexpr int64_t SC_EVENT_BYTES = 160;               // rd_site_workspace_bytes per event

// the sort key: site << 17 | cond << 16 | (value + 32768).  Inside a site sample 1 follows sample 0, each in ascending value
SC_HD inline uint64_t sc_key(uint32_t site, uint32_t cond, int32_t value)
{
    return ((uint64_t)site << 17) | ((uint64_t)cond << 16) | (uint64_t)(uint32_t)(value + 32768);
}
SC_HD inline uint32_t sc_key_site(uint64_t key) { return (uint32_t)(key >> 17); }
SC_HD inline uint32_t sc_key_cond(uint64_t key) { return (uint32_t)(key >> 16) & 1u; }
SC_HD inline int32_t sc_key_value(uint64_t key) { return (int32_t)(key & 0xffffu) - 32768; }
// bits of the key in use: 17 + the bits of n_sites - 1
inline int sc_sort_bits(uint32_t n_sites)
{
    int b = 0;
    for (uint32_t m = n_sites ? n_sites - 1 : 0; m; m >>= 1) b++;
    return 17 + b;
}

SC_HD inline int sc_status(int64_t n0, int64_t n1) { return n0 == 0 || n1 == 0 ? SC_ONE_SIDED : n0 + n1 > SC_DEEP_LIMIT ? SC_DEEP : SC_OK; }

// ks_num and ks_x as one word whose maximum is the largest ks_num and, among equals, the smallest ks_x (below 2^55: ks_num <= 2^38)
SC_HD inline uint64_t sc_ks_pack(int64_t num, int32_t x) { return ((uint64_t)num << 16) | (uint64_t)(65535 - (x + 32768)); }
SC_HD inline int64_t sc_ks_num(uint64_t w) { return (int64_t)(w >> 16); }
SC_HD inline int32_t sc_ks_x(uint64_t w) { return 65535 - (int32_t)(w & 0xffffu) - 32768; }

// what a site comes to, as the kernels store it (96 bytes)
struct ScOut {
    int64_t sum[2], sumsq[2], u2, tie;
    uint64_t ks;   // sc_ks_pack
    uint32_t site;
    int32_t status;
    uint32_t n[2];
    int32_t vmin[2], vmax[2], med2[2];
};

// one element's (or one chunk's, or one site's) share of the sums and of the maximum
struct ScTerms {
    int64_t sum[2] = {0, 0}, sumsq[2] = {0, 0}, u2 = 0, tie = 0;
    uint64_t ks = 0;
};

// first index of [lo, hi) whose key is >= key (hi if none); k ascending
SC_HD inline int64_t sc_lower(const uint64_t* k, int64_t lo, int64_t hi, uint64_t key)
{
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (k[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// a site's sorted keys are k[start, end); its sample 1 begins at the first key with the cond bit
SC_HD inline int64_t sc_split(const uint64_t* k, int64_t start, int64_t end)
{
    return sc_lower(k, start, end, (k[start] & ~(uint64_t)0x1ffff) | 0x10000);
}

// counts, status, min, max and twice the median of both samples; the sums are zero
SC_HD inline ScOut sc_head(const uint64_t* k, int64_t start, int64_t split, int64_t end)
{
    ScOut o;
    o.sum[0] = o.sum[1] = o.sumsq[0] = o.sumsq[1] = o.u2 = o.tie = 0;
    o.ks = 0;
    o.site = sc_key_site(k[start]);
    const int64_t a[2] = {start, split}, b[2] = {split, end};
    o.status = sc_status(split - start, end - split);
    for (int c = 0; c < 2; c++) {
        const int64_t n = b[c] - a[c];
        o.n[c] = (uint32_t)n;
        o.vmin[c] = n ? sc_key_value(k[a[c]]) : 0;
        o.vmax[c] = n ? sc_key_value(k[b[c] - 1]) : 0;
        o.med2[c] = n ? sc_key_value(k[a[c] + (n - 1) / 2]) + sc_key_value(k[a[c] + n / 2]) : 0;
    }
    return o;
}

// Element i of a site adds to t.  Moments: its value.  Rank terms (rank: the site's status is OK) come from the LAST element of each run
// of equal values of a sample; a value present in both samples is weighed from sample 0's side.  With ta / tb the value's multiplicity in
// the two samples and lb / ub the elements of sample 1 below it / not above it:
//   u2 += ta (lb + ub);  tie += t^3 - t, t = ta + tb;  ks = max(ks, pack(|#{a <= x} n1 - #{b <= x} n0|, x))
SC_HD inline void sc_element(const uint64_t* k, int64_t start, int64_t split, int64_t end, int64_t i, bool rank, ScTerms& t)
{
    const uint64_t key = k[i];
    const int c = i >= split;
    const int64_t v = sc_key_value(key);
    t.sum[c] += v;
    t.sumsq[c] += v * v;
    if (!rank) return;
    if (i + 1 < (c ? end : split) && k[i + 1] == key) return;
    const int64_t n0 = split - start, n1 = end - split;
    int64_t ta, tb, cnt_a, cnt_b;
    if (c == 0) {
        const uint64_t other = key | 0x10000;
        const int64_t lb = sc_lower(k, split, end, other) - split, ub = sc_lower(k, split, end, other + 1) - split;
        ta = i + 1 - sc_lower(k, start, i, key);
        tb = ub - lb;
        t.u2 += ta * (lb + ub);
        cnt_a = i + 1 - start;
        cnt_b = ub;
    } else {
        const uint64_t other = key & ~(uint64_t)0x10000;
        const int64_t la = sc_lower(k, start, split, other), ua = sc_lower(k, start, split, other + 1);
        if (ua != la) return;
        ta = 0;
        tb = i + 1 - sc_lower(k, split, i, key);
        cnt_a = ua - start;
        cnt_b = i + 1 - split;
    }
    const int64_t tt = ta + tb, d = cnt_a * n1 - cnt_b * n0;
    t.tie += tt * tt * tt - tt;
    const uint64_t w = sc_ks_pack(d < 0 ? -d : d, (int32_t)v);
    if (w > t.ks) t.ks = w;
}

// ------------------------------------------------------------------------------------------------ the two-cluster split (section 26)
// rd_site_split: the threshold on a site's pooled values that maximises J(c) = D^2 / (n_lo n_hi), D = S_lo n_hi - S_hi n_lo, among the
// admissible cuts; ties to the smaller cut.  Everything is an integer; J is compared by cross-multiplication in 128 bits.
constexpr int SS_NONE = 4;                            // RD_SITE_NONE: no admissible cut (the other statuses are SC_*)
constexpr int64_t SS_DEEP_LIMIT = (int64_t)1 << 16;   // n0 + n1 above this: totals only (D^2 n_lo n_hi would pass 128 bits)
constexpr int SS_MIN_FRAC_MAX = 32768;                // min_frac_q16: 0 .. a half
constexpr int64_t SS_EVENT_BYTES = 16;                // what a split adds per event: the two prefix arrays
constexpr int64_t SS_ITEM_BYTES = 112;                // and per work item (chunk of SC_CHUNK): its slot, and 96 B that stand for the site's entry

SC_HD inline int ss_status(int64_t n0, int64_t n1) { return n0 == 0 || n1 == 0 ? SC_ONE_SIDED : n0 + n1 > SS_DEEP_LIMIT ? SC_DEEP : SC_OK; }

// a candidate cut: |D|, the pooled counts on both sides, the cut.  n_lo == 0: no candidate (an admissible cut has n_lo >= 1)
struct SsCand {
    uint64_t d;
    uint32_t n_lo, n_hi;
    int32_t cut;
};

// a beats b: the larger J = d^2 / (n_lo n_hi), then the smaller cut.  d <= 2^46 and n_lo n_hi <= 2^30: both products are below 2^122
SC_HD inline bool ss_better(const SsCand& a, const SsCand& b)
{
    if (!a.n_lo) return false;
    if (!b.n_lo) return true;
    const unsigned __int128 l = (unsigned __int128)a.d * a.d * ((uint64_t)b.n_lo * b.n_hi), r = (unsigned __int128)b.d * b.d * ((uint64_t)a.n_lo * a.n_hi);
    return l != r ? l > r : a.cut < b.cut;
}

// the sum of x[a, b), p the inclusive prefix sums of x
SC_HD inline int64_t ss_range(const int64_t* p, int64_t a, int64_t b) { return (b > 0 ? p[b - 1] : 0) - (a > 0 ? p[a - 1] : 0); }

// Element i of a site whose split status is OK, psum the inclusive prefix sums of the sorted values: true and the candidate when i is the
// LAST element of a run of equal values of its sample, the value is not the pooled maximum and the cut is admissible.  A value present in
// both samples is weighed from sample 0's side (the sc_element pattern)
SC_HD inline bool ss_candidate(const uint64_t* k, const int64_t* psum, int64_t start, int64_t split, int64_t end, int64_t i, int64_t min_frac_q16,
                               SsCand& out)
{
    const uint64_t key = k[i];
    const int c = i >= split;
    if (i + 1 < (c ? end : split) && k[i + 1] == key) return false;
    int64_t cnt_a, cnt_b;
    if (c == 0) {
        cnt_a = i + 1 - start;
        cnt_b = sc_lower(k, split, end, (key | 0x10000) + 1) - split;
    } else {
        const uint64_t other = key & ~(uint64_t)0x10000;
        const int64_t la = sc_lower(k, start, split, other), ua = sc_lower(k, start, split, other + 1);
        if (ua != la) return false;
        cnt_a = ua - start;
        cnt_b = i + 1 - split;
    }
    const int64_t N = end - start, n_lo = cnt_a + cnt_b, n_hi = N - n_lo;
    if (n_hi < 1 || 65536 * n_lo < min_frac_q16 * N || 65536 * n_hi < min_frac_q16 * N) return false;
    const int64_t s_lo = ss_range(psum, start, start + cnt_a) + ss_range(psum, split, split + cnt_b), s_all = ss_range(psum, start, end);
    const int64_t d = s_lo * n_hi - (s_all - s_lo) * n_lo;
    out.d = (uint64_t)(d < 0 ? -d : d);
    out.n_lo = (uint32_t)n_lo;
    out.n_hi = (uint32_t)n_hi;
    out.cut = sc_key_value(key);
    return true;
}

// what a site's split comes to, as the kernels store it (96 bytes)
struct SsOut {
    int64_t sum[2], sumsq[2], sum_lo[2], sumsq_lo[2];
    uint32_t site;
    int32_t status;
    uint32_t n[2];
    int32_t cut, n_cuts;
    uint32_t n_lo[2];
};

// The entry of the site k[start, end) from the best of its candidates (best.n_lo == 0: none) and their number: totals from the prefix
// arrays (psum of the values, psq of their squares), the low cluster per sample at the upper bounds of the cut in the two runs
SC_HD inline SsOut ss_entry(const uint64_t* k, const int64_t* psum, const int64_t* psq, int64_t start, int64_t split, int64_t end, const SsCand& best,
                            int32_t n_cuts)
{
    SsOut o;
    o.site = sc_key_site(k[start]);
    o.n[0] = (uint32_t)(split - start);
    o.n[1] = (uint32_t)(end - split);
    o.sum[0] = ss_range(psum, start, split), o.sum[1] = ss_range(psum, split, end);
    o.sumsq[0] = ss_range(psq, start, split), o.sumsq[1] = ss_range(psq, split, end);
    o.status = ss_status(split - start, end - split);
    if (o.status == SC_OK && !best.n_lo) o.status = SS_NONE;
    o.cut = o.n_cuts = 0;
    for (int c = 0; c < 2; c++) o.n_lo[c] = 0, o.sum_lo[c] = o.sumsq_lo[c] = 0;
    if (o.status != SC_OK) return o;
    o.cut = best.cut;
    o.n_cuts = n_cuts;
    const int64_t a[2] = {start, split}, b[2] = {split, end};
    for (int c = 0; c < 2; c++) {
        const int64_t u = sc_lower(k, a[c], b[c], sc_key(o.site, (uint32_t)c, best.cut) + 1);
        o.n_lo[c] = (uint32_t)(u - a[c]);
        o.sum_lo[c] = ss_range(psum, a[c], u);
        o.sumsq_lo[c] = ss_range(psq, a[c], u);
    }
    return o;
}

// ------------------------------------------------------------------------------------------------ the host's counting pass and plan
struct ScSite {
    uint32_t site;
    int64_t n[2];
};

// the distinct sites of the events in ascending order with their counts per sample.  Returns the index of the first event whose site is
// >= n_sites or whose cond is > 1, -1 if there is none.  One pass over the events: a dense table where the sites are few against the
// events, a hash table otherwise
inline int64_t sc_count_sites(const uint32_t* site, const uint8_t* cond, int64_t n_events, uint32_t n_sites, std::vector<ScSite>& out)
{
    out.clear();
    for (int64_t i = 0; i < n_events; i++)
        if (site[i] >= n_sites || cond[i] > 1) return i;
    if ((int64_t)n_sites <= std::max<int64_t>(65536, 4 * n_events)) {
        std::vector<int64_t> cnt(2 * (size_t)n_sites, 0);
        for (int64_t i = 0; i < n_events; i++) cnt[2 * (size_t)site[i] + cond[i]]++;
        for (uint32_t s = 0; s < n_sites; s++)
            if (cnt[2 * (size_t)s] || cnt[2 * (size_t)s + 1]) out.push_back(ScSite{s, {cnt[2 * (size_t)s], cnt[2 * (size_t)s + 1]}});
    } else {
        std::unordered_map<uint32_t, std::pair<int64_t, int64_t>> cnt;
        for (int64_t i = 0; i < n_events; i++) (cond[i] ? cnt[site[i]].second : cnt[site[i]].first)++;
        for (const auto& kv : cnt) out.push_back(ScSite{kv.first, {kv.second.first, kv.second.second}});
        std::sort(out.begin(), out.end(), [](const ScSite& a, const ScSite& b) { return a.site < b.site; });
    }
    return -1;
}

inline int64_t sc_site_bytes(const ScSite& s) { return SC_EVENT_BYTES * (s.n[0] + s.n[1]); }
inline int64_t sc_site_chunks(const ScSite& s) { return (s.n[0] + s.n[1] + SC_CHUNK - 1) / SC_CHUNK; }

// launches of consecutive sites under the budget; a site that alone exceeds it ends the open launch and is left out
inline BudgetPlan sc_plan(const std::vector<ScSite>& sites, int64_t budget)
{
    return rd_plan_budget((int64_t)sites.size(), nullptr, budget, 0, true, [&](int s, int) { return sc_site_bytes(sites[s]); },
                          rd_budget_never_closes);
}

// the same for rd_site_split: a site's need is rd_site_split_workspace_bytes of its events
inline int64_t ss_bytes(int64_t n_events) { return (SC_EVENT_BYTES + SS_EVENT_BYTES) * n_events + SS_ITEM_BYTES * ((n_events + SC_CHUNK - 1) / SC_CHUNK); }
inline int64_t ss_site_bytes(const ScSite& s) { return ss_bytes(s.n[0] + s.n[1]); }
inline BudgetPlan ss_plan(const std::vector<ScSite>& sites, int64_t budget)
{
    return rd_plan_budget((int64_t)sites.size(), nullptr, budget, 0, true, [&](int s, int) { return ss_site_bytes(sites[s]); },
                          rd_budget_never_closes);
}

// The events of every launch, gathered launch by launch (their order inside a launch is the caller's): launch l holds events
// off[l] .. off[l+1] of g_site / g_cond / g_value.  An event of a site that is in no launch is left out.  One counting pass
inline void sc_bucket(const uint32_t* site, const uint8_t* cond, const int16_t* value, int64_t n_events, const std::vector<ScSite>& sites,
                      const BudgetPlan& plan, std::vector<int64_t>& off, std::vector<uint32_t>& g_site, std::vector<uint8_t>& g_cond,
                      std::vector<int16_t>& g_value)
{
    const size_t nl = plan.launches.size();
    std::vector<uint32_t> first(nl), last(nl);
    for (size_t l = 0; l < nl; l++) {
        first[l] = sites[plan.run[plan.launches[l].first]].site;
        last[l] = sites[plan.run[plan.launches[l].second - 1]].site;
    }
    const auto launch_of = [&](uint32_t s) -> int64_t {
        const size_t l = (size_t)(std::upper_bound(first.begin(), first.end(), s) - first.begin());
        return l > 0 && s <= last[l - 1] ? (int64_t)l - 1 : -1;
    };
    off.assign(nl + 1, 0);
    for (int64_t i = 0; i < n_events; i++) {
        const int64_t l = launch_of(site[i]);
        if (l >= 0) off[l + 1]++;
    }
    for (size_t l = 0; l < nl; l++) off[l + 1] += off[l];
    g_site.resize((size_t)off[nl]);
    g_cond.resize((size_t)off[nl]);
    g_value.resize((size_t)off[nl]);
    std::vector<int64_t> at(off.begin(), off.end() - 1);
    for (int64_t i = 0; i < n_events; i++) {
        const int64_t l = launch_of(site[i]);
        if (l < 0) continue;
        const size_t o = (size_t)at[l]++;
        g_site[o] = site[i];
        g_cond[o] = cond[i];
        g_value[o] = value[i];
    }
}
