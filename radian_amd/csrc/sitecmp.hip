// sitecmp.hip -- two-sample comparison of event tables, site by site: moments, order statistics, Mann-Whitney U, the Kolmogorov-Smirnov
// numerator and the tie term of every transcript position, as integers.  DESIGN.md section 20.
//
// Contract (integer arithmetic only; include/radian_hip.h, rd_site_compare; the rules themselves are site_rules.h).  n_events events
// (site < n_sites, cond 0 / 1, value int16).  One entry per distinct site in ascending order; a / b the sorted values of sample 0 / 1:
//   n, sum, sumsq, vmin, vmax per sample; med2 = the sum of the two middle order statistics (ranks (n-1)/2 and n/2)
//   u2     = sum over x in a of 2 #{y in b : y < x} + #{y in b : y = x}
//   ks_num = max over the values x present of |#{a <= x} n1 - #{b <= x} n0|; ks_x = the smallest x that attains it
//   tie    = sum over the values x of t^3 - t, t the pooled multiplicity of x
//   status   n0 == 0 or n1 == 0 ONE_SIDED; else n0 + n1 > 2^20 DEEP; else OK.  Rank fields (u2, ks_num, ks_x, tie) are 0 unless OK.
//
// Kernels, on one stream, per launch of n events in S sites:
//   sc_pack_kernel     one thread per event: the 64-bit key site << 17 | cond << 16 | (value + 32768)
//   rocprim::radix_sort_keys over the bits in use
//   sc_flag_kernel     head flag where key >> 17 changes; rocprim::exclusive_scan of the flags; sc_compact_kernel writes the segment starts
//   sc_head_kernel     one thread per site: the split (a binary search for the cond bit), counts, status, min, max, med2 by direct indexing,
//                      zeroed sums, and the site's number of chunks of SC_CHUNK elements; rocprim::exclusive_scan of those -> work items
//   sc_site_kernel     one wave per (site, chunk).  A lane takes every 64th element of the chunk and calls sc_element: the moments, and at the
//                      last element of a run of equal values two or three binary searches into the other run and its own.  The wave's terms
//                      are combined by xor-shuffles (integer add and max) and lane 0 adds them to the site's entry with 64-bit atomics;
//                      ks_num and ks_x are one atomicMax on sc_ks_pack.  Every combination is an integer add or max: the result does not
//                      depend on how the elements are spread over lanes, waves and launches.
// No floating point, no LDS, no inline assembly.
//
// rd_site_split runs the same pack / sort / flag / scan / compact / head stages (sc_run) and then, per launch:
//   rocprim::inclusive_scan twice over the sorted keys' values and their squares (int64, read through a transform iterator)
//   ss_item_kernel     one wave per (site, chunk): a lane takes every 64th element and calls ss_candidate; the lane's best under ss_better,
//                      the wave's best by xor-shuffles under the same total order into the item's slot; the count of admissible cuts by
//                      one 32-bit atomic add per wave
//   ss_pick_kernel     one wave per site: the best over the site's slots under the same order, then lane 0 writes the entry (ss_entry:
//                      totals and the low cluster's n, sum and sumsq as differences of the two prefix arrays)
#include "common.h"
#include "carve.h"
#include "site_rules.h"
#include "../../include/radian_hip.h"

#include <cstring>
#include <vector>

namespace {

struct ScArrays {
    uint32_t* out_site;
    int32_t* status;
    int64_t *n, *sum, *sumsq;
    int32_t *vmin, *vmax, *med2;
    int64_t *u2, *ks_num;
    int32_t* ks_x;
    int64_t* tie;
};

int sc_check_args(const char* who, const uint32_t* site, const uint8_t* cond, const int16_t* value, int64_t n_events, const void* const* outs,
                  int n_outs)
{
    RD_REQUIRE(n_events >= 0 && n_events <= INT32_MAX, "%s: n_events must be 0 .. 2^31 - 1", who);
    for (int i = 0; i < n_outs; i++) RD_REQUIRE(outs[i], "%s: null output", who);
    if (n_events == 0) return RD_OK;
    RD_REQUIRE(site && cond && value, "%s: null argument", who);
    return RD_OK;
}

int sc_count_checked(const char* who, const uint32_t* site, const uint8_t* cond, int64_t n_events, uint32_t n_sites, int64_t capacity,
                     std::vector<ScSite>& sites)
{
    const int64_t bad = sc_count_sites(site, cond, n_events, n_sites, sites);
    if (bad >= 0) {
        if (site[bad] >= n_sites) rd_set_error("%s: event %lld has site %u, n_sites is %u", who, (long long)bad, site[bad], n_sites);
        else rd_set_error("%s: event %lld has cond %d (0 or 1)", who, (long long)bad, (int)cond[bad]);
        return RD_ERR_ARG;
    }
    RD_REQUIRE(capacity >= (int64_t)sites.size(), "%s: %lld distinct sites, the outputs hold %lld", who, (long long)sites.size(), (long long)capacity);
    return RD_OK;
}

// entry j of the caller's arrays from a site's result, by the field rules of its status: TOO_LARGE only the site and n, rank fields only for OK
void sc_scatter(const ScOut& o, int64_t j, const ScArrays& A)
{
    const bool rank = o.status == SC_OK, rest = o.status != SC_TOO_LARGE;
    A.out_site[j] = o.site;
    A.status[j] = o.status;
    for (int c = 0; c < 2; c++) {
        A.n[2 * j + c] = o.n[c];
        A.sum[2 * j + c] = rest ? o.sum[c] : 0;
        A.sumsq[2 * j + c] = rest ? o.sumsq[c] : 0;
        A.vmin[2 * j + c] = rest ? o.vmin[c] : 0;
        A.vmax[2 * j + c] = rest ? o.vmax[c] : 0;
        A.med2[2 * j + c] = rest ? o.med2[c] : 0;
    }
    A.u2[j] = rank ? o.u2 : 0;
    A.ks_num[j] = rank ? sc_ks_num(o.ks) : 0;
    A.ks_x[j] = rank ? sc_ks_x(o.ks) : 0;
    A.tie[j] = rank ? o.tie : 0;
}

}  // namespace

extern "C" int64_t rd_site_workspace_bytes(int64_t n_events)
{
    if (n_events < 0 || n_events > INT32_MAX) return -1;
    return SC_EVENT_BYTES * n_events;
}

extern "C" int rd_site_compare_host(const uint32_t* site, const uint8_t* cond, const int16_t* value, int64_t n_events, uint32_t n_sites,
                                    int64_t capacity, uint32_t* out_site, int32_t* status, int64_t* n, int64_t* sum, int64_t* sumsq, int32_t* vmin,
                                    int32_t* vmax, int32_t* med2, int64_t* u2, int64_t* ks_num, int32_t* ks_x, int64_t* tie, int64_t* n_out)
{
    const ScArrays A{out_site, status, n, sum, sumsq, vmin, vmax, med2, u2, ks_num, ks_x, tie};
    const void* const outs[13] = {out_site, status, n, sum, sumsq, vmin, vmax, med2, u2, ks_num, ks_x, tie, n_out};
    int rc = sc_check_args("rd_site_compare_host", site, cond, value, n_events, outs, 13);
    if (rc) return rc;
    RD_REQUIRE(capacity >= 0, "rd_site_compare_host: negative capacity");
    std::vector<ScSite> sites;
    if ((rc = sc_count_checked("rd_site_compare_host", site, cond, n_events, n_sites, capacity, sites))) return rc;
    *n_out = (int64_t)sites.size();
    if (n_events == 0) return RD_OK;
    std::vector<uint64_t> k((size_t)n_events);
    for (int64_t i = 0; i < n_events; i++) k[i] = sc_key(site[i], cond[i], value[i]);
    std::sort(k.begin(), k.end());
    int64_t start = 0;
    for (size_t j = 0; j < sites.size(); j++) {
        const int64_t end = start + sites[j].n[0] + sites[j].n[1], split = sc_split(k.data(), start, end);
        ScOut o = sc_head(k.data(), start, split, end);
        ScTerms t;
        for (int64_t i = start; i < end; i++) sc_element(k.data(), start, split, end, i, o.status == SC_OK, t);
        for (int c = 0; c < 2; c++) o.sum[c] = t.sum[c], o.sumsq[c] = t.sumsq[c];
        o.u2 = t.u2;
        o.tie = t.tie;
        o.ks = t.ks;
        sc_scatter(o, (int64_t)j, A);
        start = end;
    }
    return RD_OK;
}

// ------------------------------------------------------------------------------------------------------------------ the split, host half
namespace {

struct SsArrays {
    uint32_t* out_site;
    int32_t* status;
    int64_t *n, *sum, *sumsq;
    int32_t *cut, *n_cuts;
    int64_t *n_lo, *sum_lo, *sumsq_lo;
};

// entry j of the caller's arrays by the field rules of its status: TOO_LARGE only the site and n, cut fields only for OK (ss_entry zeroes them)
void ss_scatter(const SsOut& o, int64_t j, const SsArrays& A)
{
    const bool rest = o.status != SC_TOO_LARGE;
    A.out_site[j] = o.site;
    A.status[j] = o.status;
    A.cut[j] = rest ? o.cut : 0;
    A.n_cuts[j] = rest ? o.n_cuts : 0;
    for (int c = 0; c < 2; c++) {
        A.n[2 * j + c] = o.n[c];
        A.sum[2 * j + c] = rest ? o.sum[c] : 0;
        A.sumsq[2 * j + c] = rest ? o.sumsq[c] : 0;
        A.n_lo[2 * j + c] = rest ? o.n_lo[c] : 0;
        A.sum_lo[2 * j + c] = rest ? o.sum_lo[c] : 0;
        A.sumsq_lo[2 * j + c] = rest ? o.sumsq_lo[c] : 0;
    }
}

int ss_check_args(const char* who, const uint32_t* site, const uint8_t* cond, const int16_t* value, int64_t n_events, int min_frac_q16,
                  const SsArrays& A, const int64_t* n_out)
{
    const void* const outs[11] = {A.out_site, A.status, A.n, A.sum, A.sumsq, A.cut, A.n_cuts, A.n_lo, A.sum_lo, A.sumsq_lo, n_out};
    const int rc = sc_check_args(who, site, cond, value, n_events, outs, 11);
    if (rc) return rc;
    RD_REQUIRE(min_frac_q16 >= 0 && min_frac_q16 <= SS_MIN_FRAC_MAX, "%s: min_frac_q16 must be 0 .. 32768", who);
    return RD_OK;
}

}  // namespace

extern "C" int64_t rd_site_split_workspace_bytes(int64_t n_events)
{
    if (n_events < 0 || n_events > INT32_MAX) return -1;
    return ss_bytes(n_events);
}

extern "C" int rd_site_split_host(const uint32_t* site, const uint8_t* cond, const int16_t* value, int64_t n_events, uint32_t n_sites,
                                  int64_t capacity, int min_frac_q16, uint32_t* out_site, int32_t* status, int64_t* n, int64_t* sum, int64_t* sumsq,
                                  int32_t* cut, int32_t* n_cuts, int64_t* n_lo, int64_t* sum_lo, int64_t* sumsq_lo, int64_t* n_out)
{
    const SsArrays A{out_site, status, n, sum, sumsq, cut, n_cuts, n_lo, sum_lo, sumsq_lo};
    int rc = ss_check_args("rd_site_split_host", site, cond, value, n_events, min_frac_q16, A, n_out);
    if (rc) return rc;
    RD_REQUIRE(capacity >= 0, "rd_site_split_host: negative capacity");
    std::vector<ScSite> sites;
    if ((rc = sc_count_checked("rd_site_split_host", site, cond, n_events, n_sites, capacity, sites))) return rc;
    *n_out = (int64_t)sites.size();
    if (n_events == 0) return RD_OK;
    std::vector<uint64_t> k((size_t)n_events);
    for (int64_t i = 0; i < n_events; i++) k[i] = sc_key(site[i], cond[i], value[i]);
    std::sort(k.begin(), k.end());
    std::vector<int64_t> psum((size_t)n_events), psq((size_t)n_events);
    int64_t s = 0, q = 0;
    for (int64_t i = 0; i < n_events; i++) {
        const int64_t v = sc_key_value(k[i]);
        psum[i] = s += v;
        psq[i] = q += v * v;
    }
    int64_t start = 0;
    for (size_t j = 0; j < sites.size(); j++) {
        const int64_t end = start + sites[j].n[0] + sites[j].n[1], split = sc_split(k.data(), start, end);
        SsCand best{0, 0, 0, 0}, cand;
        int32_t n_cuts_j = 0;
        if (ss_status(split - start, end - split) == SC_OK)
            for (int64_t i = start; i < end; i++)
                if (ss_candidate(k.data(), psum.data(), start, split, end, i, min_frac_q16, cand)) {
                    n_cuts_j++;
                    if (ss_better(cand, best)) best = cand;
                }
        ss_scatter(ss_entry(k.data(), psum.data(), psq.data(), start, split, end, best, n_cuts_j), (int64_t)j, A);
        start = end;
    }
    return RD_OK;
}

// ------------------------------------------------------------------------------------------------------------------ a launch's device block
namespace {

struct ScSeg {
    uint32_t start, split, end, pad_;
};
// a work item's best candidate (n_lo == 0: none); n_hi is the site's count less n_lo
struct SsSlot {
    uint64_t d;
    uint32_t n_lo;
    int32_t cut;
};

struct ScWs {
    uint32_t* in_site;
    uint8_t* in_cond;
    int16_t* in_value;
    uint64_t *ka, *kb;
    uint32_t *flag, *pos, *seg_start, *n_chunk, *item_off, *n_seg;
    ScSeg* seg;
    ScOut* out;
    void* tmp;
    int64_t *psum, *psq;   // the split's: the two prefix arrays, the slots, the admissible-cut counts and the entries
    SsSlot* slot;
    int32_t* cnt;
    SsOut* split_out;
    size_t tmp_bytes;
    const uint64_t* sorted;
    size_t min_tmp = 0;         // set by the caller before sc_run: the least tmp_bytes
    int64_t split_items = -1;   // ... and, for a split, its work items (-1: a comparison, without the split's arrays)
};

// n events expected to fall into S sites, tmp_bytes of sort and scan storage
void sc_layout(Carve& c, int64_t n, int64_t S, size_t tmp_bytes, int64_t split_items, ScWs* W)
{
    W->in_site = c.take<uint32_t>((size_t)n, 8);
    W->in_cond = c.take<uint8_t>((size_t)n, 8);
    W->in_value = c.take<int16_t>((size_t)n, 8);
    W->ka = c.take<uint64_t>((size_t)n, 8);
    W->kb = c.take<uint64_t>((size_t)n, 8);
    W->flag = c.take<uint32_t>((size_t)n, 8);
    W->pos = c.take<uint32_t>((size_t)n, 8);
    W->seg_start = c.take<uint32_t>((size_t)S + 1, 8);
    W->n_chunk = c.take<uint32_t>((size_t)S + 1, 8);
    W->item_off = c.take<uint32_t>((size_t)S + 1, 8);
    W->n_seg = c.take<uint32_t>(1, 8);
    W->seg = c.take<ScSeg>((size_t)S, 8);
    W->out = c.take<ScOut>((size_t)S, 8);
    W->tmp = c.take<char>(tmp_bytes, 8);
    const bool split = split_items >= 0;   // (a comparison keeps the 8 bytes behind its last array)
    W->psum = c.take<int64_t>(split ? (size_t)n : 0);
    W->psq = c.take<int64_t>(split ? (size_t)n : 0);
    W->slot = c.take<SsSlot>(split ? (size_t)split_items : 0);
    W->cnt = c.take<int32_t>(split ? (size_t)S : 0);
    W->split_out = c.take<SsOut>(split ? (size_t)S : 0, 8);
    W->tmp_bytes = tmp_bytes;
}

}  // namespace

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------------------------------ device half
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

namespace {

constexpr int SC_WAVES = 4;   // waves (work items) per workgroup of the site kernel

__global__ __launch_bounds__(256) void sc_pack_kernel(const uint32_t* __restrict__ site, const uint8_t* __restrict__ cond,
                                                      const int16_t* __restrict__ value, uint32_t n, uint64_t* __restrict__ keys)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) keys[i] = sc_key(site[i], cond[i], value[i]);
}

__global__ __launch_bounds__(256) void sc_flag_kernel(const uint64_t* __restrict__ keys, uint32_t n, uint32_t* __restrict__ flag)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) flag[i] = i == 0 || (keys[i] >> 17) != (keys[i - 1] >> 17) ? 1u : 0u;
}

// seg_start[s] = the index of head s (pos: the exclusive scan of the flags); seg_start[n_seg] = n, n_seg <= cap_seg checked by the host's count
__global__ __launch_bounds__(256) void sc_compact_kernel(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos, uint32_t n,
                                                         uint32_t cap_seg, uint32_t* __restrict__ seg_start, uint32_t* __restrict__ n_seg)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    if (flag[i] && pos[i] < cap_seg) seg_start[pos[i]] = i;
    if (i == n - 1) {
        const uint32_t S = pos[i] + flag[i];
        *n_seg = S;
        if (S <= cap_seg) seg_start[S] = n;
    }
}

// (found: the number of heads the compaction saw.  It equals the host's count n_seg; if it ever did not, seg_start would not be filled as
// expected, so nothing is read through it and the host reports the mismatch)
__global__ __launch_bounds__(256) void sc_head_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ seg_start, uint32_t n_seg,
                                                      const uint32_t* __restrict__ found, ScSeg* __restrict__ seg, ScOut* __restrict__ out,
                                                      uint32_t* __restrict__ n_chunk)
{
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s > n_seg || *found != n_seg) return;
    if (s == n_seg) {   // (the scan runs over n_seg + 1 counts: its last output is the total)
        n_chunk[s] = 0;
        return;
    }
    const int64_t start = seg_start[s], end = seg_start[s + 1], split = sc_split(keys, start, end);
    seg[s] = ScSeg{(uint32_t)start, (uint32_t)split, (uint32_t)end, 0};
    out[s] = sc_head(keys, start, split, end);
    n_chunk[s] = (uint32_t)((end - start + SC_CHUNK - 1) / SC_CHUNK);
}

__device__ inline int64_t sc_wave_add(int64_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__global__ __launch_bounds__(64 * SC_WAVES) void sc_site_kernel(const uint64_t* __restrict__ keys, const ScSeg* __restrict__ seg,
                                                                const uint32_t* __restrict__ item_off, uint32_t n_seg, uint32_t n_items,
                                                                const uint32_t* __restrict__ found, ScOut* __restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const uint32_t item = blockIdx.x * (uint32_t)SC_WAVES + (threadIdx.x >> 6);   // (the same in every lane of the wave)
    if (item >= n_items || *found != n_seg || item_off[n_seg] != n_items) return;
    // the site of the item: the last s with item_off[s] <= item (sites have at least one chunk: item_off is strictly increasing)
    uint32_t lo = 0, hi = n_seg;
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (item_off[mid] <= item) lo = mid;
        else hi = mid;
    }
    const ScSeg sg = seg[lo];
    const bool rank = out[lo].status == SC_OK;   // (written by sc_head_kernel; the atomics below do not touch it)
    const int64_t i0 = (int64_t)sg.start + (int64_t)(item - item_off[lo]) * SC_CHUNK, i1 = i0 + SC_CHUNK < (int64_t)sg.end ? i0 + SC_CHUNK : (int64_t)sg.end;
    ScTerms t;
    for (int64_t i = i0 + lane; i < i1; i += 64) sc_element(keys, sg.start, sg.split, sg.end, i, rank, t);
    for (int c = 0; c < 2; c++) {
        t.sum[c] = sc_wave_add(t.sum[c]);
        t.sumsq[c] = sc_wave_add(t.sumsq[c]);
    }
    t.u2 = sc_wave_add(t.u2);
    t.tie = sc_wave_add(t.tie);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint64_t o = (uint64_t)__shfl_xor((long long)t.ks, d);
        t.ks = o > t.ks ? o : t.ks;
    }
    if (lane != 0) return;
    ScOut* o = out + lo;
    for (int c = 0; c < 2; c++) {
        if (t.sum[c]) atomicAdd((unsigned long long*)&o->sum[c], (unsigned long long)t.sum[c]);
        if (t.sumsq[c]) atomicAdd((unsigned long long*)&o->sumsq[c], (unsigned long long)t.sumsq[c]);
    }
    if (t.u2) atomicAdd((unsigned long long*)&o->u2, (unsigned long long)t.u2);
    if (t.tie) atomicAdd((unsigned long long*)&o->tie, (unsigned long long)t.tie);
    if (t.ks) atomicMax((unsigned long long*)&o->ks, (unsigned long long)t.ks);
}

// pack, sort and segment n events expected to fall into S sites; with n_items > 0 the head and site kernels too.  Leaves the stream running
int sc_run(rd_ctx* ctx, hipStream_t st, const uint32_t* site, const uint8_t* cond, const int16_t* value, int64_t n, int64_t S, int64_t n_items,
           int end_bit, ScWs& W)
{
    size_t sort_bytes = 0, scan_bytes = 0, scan2_bytes = 0;
    rocprim::double_buffer<uint64_t> probe((uint64_t*)nullptr, (uint64_t*)nullptr);
    RD_HIP(rocprim::radix_sort_keys(nullptr, sort_bytes, probe, (size_t)n, 0u, (unsigned)end_bit, st));
    RD_HIP(rocprim::exclusive_scan(nullptr, scan_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)n, rocprim::plus<uint32_t>(), st));
    RD_HIP(rocprim::exclusive_scan(nullptr, scan2_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)S + 1, rocprim::plus<uint32_t>(), st));
    const size_t tmp_bytes = std::max(std::max(sort_bytes, W.min_tmp), std::max(scan_bytes, scan2_bytes));
    if (rd_carve(ctx->ws_site, [&](Carve& c) { sc_layout(c, n, S, tmp_bytes, W.split_items, &W); })) return RD_ERR_NOMEM;
    RD_HIP(hipMemcpyAsync(W.in_site, site, (size_t)n * 4, hipMemcpyHostToDevice, st));
    RD_HIP(hipMemcpyAsync(W.in_cond, cond, (size_t)n, hipMemcpyHostToDevice, st));
    RD_HIP(hipMemcpyAsync(W.in_value, value, (size_t)n * 2, hipMemcpyHostToDevice, st));
    const unsigned nb = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(sc_pack_kernel, dim3(nb), dim3(256), 0, st, W.in_site, W.in_cond, W.in_value, (uint32_t)n, W.ka);
    RD_HIP(hipGetLastError());
    rocprim::double_buffer<uint64_t> dk(W.ka, W.kb);
    size_t tb = W.tmp_bytes;
    RD_HIP(rocprim::radix_sort_keys(W.tmp, tb, dk, (size_t)n, 0u, (unsigned)end_bit, st));
    W.sorted = dk.current();
    hipLaunchKernelGGL(sc_flag_kernel, dim3(nb), dim3(256), 0, st, W.sorted, (uint32_t)n, W.flag);
    RD_HIP(hipGetLastError());
    tb = W.tmp_bytes;
    RD_HIP(rocprim::exclusive_scan(W.tmp, tb, W.flag, W.pos, 0u, (size_t)n, rocprim::plus<uint32_t>(), st));
    hipLaunchKernelGGL(sc_compact_kernel, dim3(nb), dim3(256), 0, st, W.flag, W.pos, (uint32_t)n, (uint32_t)S, W.seg_start, W.n_seg);
    RD_HIP(hipGetLastError());
    hipLaunchKernelGGL(sc_head_kernel, dim3((unsigned)((S + 1 + 255) / 256)), dim3(256), 0, st, W.sorted, W.seg_start, (uint32_t)S, W.n_seg, W.seg, W.out,
                       W.n_chunk);
    RD_HIP(hipGetLastError());
    if (n_items > 0) {
        tb = W.tmp_bytes;
        RD_HIP(rocprim::exclusive_scan(W.tmp, tb, W.n_chunk, W.item_off, 0u, (size_t)S + 1, rocprim::plus<uint32_t>(), st));
        hipLaunchKernelGGL(sc_site_kernel, dim3((unsigned)((n_items + SC_WAVES - 1) / SC_WAVES)), dim3(64 * SC_WAVES), 0, st, W.sorted, W.seg,
                           W.item_off, (uint32_t)S, (uint32_t)n_items, W.n_seg, W.out);
        RD_HIP(hipGetLastError());
    }
    return RD_OK;
}

}  // namespace

extern "C" int rd_site_compare(rd_ctx* ctx, const uint32_t* site, const uint8_t* cond, const int16_t* value, int64_t n_events, uint32_t n_sites,
                               int64_t budget_bytes, int64_t capacity, uint32_t* out_site, int32_t* status, int64_t* n, int64_t* sum,
                               int64_t* sumsq, int32_t* vmin, int32_t* vmax, int32_t* med2, int64_t* u2, int64_t* ks_num, int32_t* ks_x,
                               int64_t* tie, int64_t* n_out)
{
    RD_REQUIRE(ctx, "rd_site_compare: null context");
    RD_REQUIRE(budget_bytes >= 0 && capacity >= 0, "rd_site_compare: negative budget or capacity");
    const ScArrays A{out_site, status, n, sum, sumsq, vmin, vmax, med2, u2, ks_num, ks_x, tie};
    const void* const outs[13] = {out_site, status, n, sum, sumsq, vmin, vmax, med2, u2, ks_num, ks_x, tie, n_out};
    int rc = sc_check_args("rd_site_compare", site, cond, value, n_events, outs, 13);
    if (rc) return rc;
    std::vector<ScSite> sites;
    if ((rc = sc_count_checked("rd_site_compare", site, cond, n_events, n_sites, capacity, sites))) return rc;
    *n_out = (int64_t)sites.size();
    if (n_events == 0) return RD_OK;
    RD_HIP(hipSetDevice(ctx->device));
    if ((rc = rd_resolve_budget(&budget_bytes, ctx->ws_site.cap))) return rc;   // (this context's block counts as free)
    const BudgetPlan plan = sc_plan(sites, budget_bytes);
    for (size_t j = 0; j < sites.size(); j++) {   // until its launch has run
        ScOut o;
        memset(&o, 0, sizeof o);
        o.site = sites[j].site;
        o.status = SC_TOO_LARGE;
        o.n[0] = (uint32_t)sites[j].n[0];
        o.n[1] = (uint32_t)sites[j].n[1];
        sc_scatter(o, (int64_t)j, A);
    }
    // one launch that holds every event takes the caller's arrays as they are; otherwise the events are gathered launch by launch
    std::vector<int64_t> off;
    std::vector<uint32_t> g_site;
    std::vector<uint8_t> g_cond;
    std::vector<int16_t> g_value;
    const bool whole = plan.launches.size() == 1 && plan.too_large == 0;
    if (!whole) sc_bucket(site, cond, value, n_events, sites, plan, off, g_site, g_cond, g_value);
    std::vector<ScOut> got;
    hipStream_t st = ctx->stream;
    const int end_bit = sc_sort_bits(n_sites);
    for (size_t l = 0; l < plan.launches.size(); l++) {
        const int64_t k0 = plan.launches[l].first, k1 = plan.launches[l].second, S = k1 - k0, j0 = plan.run[k0];
        int64_t nl = 0, items = 0;
        for (int64_t k = k0; k < k1; k++) {
            nl += sites[plan.run[k]].n[0] + sites[plan.run[k]].n[1];
            items += sc_site_chunks(sites[plan.run[k]]);
        }
        const int64_t e0 = whole ? 0 : off[l];
        ScWs W;
        if ((rc = sc_run(ctx, st, (whole ? site : g_site.data()) + e0, (whole ? cond : g_cond.data()) + e0, (whole ? value : g_value.data()) + e0, nl, S,
                         items, end_bit, W)))
            return rc;
        got.resize((size_t)S);
        uint32_t n_seg = 0;
        RD_HIP(hipMemcpyAsync(&n_seg, W.n_seg, 4, hipMemcpyDeviceToHost, st));
        RD_HIP(hipMemcpyAsync(got.data(), W.out, (size_t)S * sizeof(ScOut), hipMemcpyDeviceToHost, st));
        RD_HIP(hipStreamSynchronize(st));
        if ((int64_t)n_seg != S) {
            rd_set_error("rd_site_compare: internal: the device found %u sites in a launch of %lld", n_seg, (long long)S);
            return RD_ERR_STATE;
        }
        for (int64_t j = 0; j < S; j++) sc_scatter(got[(size_t)j], j0 + j, A);
    }
    if (plan.too_large) {
        const ScSite& s = sites[(size_t)plan.first_too_large];
        rd_set_error("rd_site_compare: site %u (%lld events) needs %lld bytes of workspace, over the budget of %lld; %lld site(s) not compared "
                     "(status RD_SITE_TOO_LARGE), the others were", s.site, (long long)(s.n[0] + s.n[1]), (long long)sc_site_bytes(s),
                     (long long)budget_bytes, (long long)plan.too_large);
        return RD_ERR_NOMEM;
    }
    return RD_OK;
}

extern "C" int rd_site_diag_segments(rd_ctx* ctx, const uint32_t* site, const uint8_t* cond, const int16_t* value, int64_t n_events, uint32_t n_sites,
                                     int64_t capacity, uint64_t* sorted_keys, int64_t* segments, int64_t* n_segments)
{
    RD_REQUIRE(ctx, "rd_site_diag_segments: null context");
    RD_REQUIRE(capacity >= 0, "rd_site_diag_segments: negative capacity");
    const void* const outs[3] = {sorted_keys, segments, n_segments};
    int rc = sc_check_args("rd_site_diag_segments", site, cond, value, n_events, outs, 3);
    if (rc) return rc;
    std::vector<ScSite> sites;
    if ((rc = sc_count_checked("rd_site_diag_segments", site, cond, n_events, n_sites, capacity, sites))) return rc;
    *n_segments = 0;
    if (n_events == 0) return RD_OK;
    RD_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int64_t S = (int64_t)sites.size();
    ScWs W;
    if ((rc = sc_run(ctx, st, site, cond, value, n_events, S, 0, sc_sort_bits(n_sites), W))) return rc;
    std::vector<ScSeg> seg((size_t)S);
    std::vector<ScOut> got((size_t)S);
    uint32_t n_seg = 0;
    RD_HIP(hipMemcpyAsync(&n_seg, W.n_seg, 4, hipMemcpyDeviceToHost, st));
    RD_HIP(hipMemcpyAsync(sorted_keys, W.sorted, (size_t)n_events * 8, hipMemcpyDeviceToHost, st));
    RD_HIP(hipMemcpyAsync(seg.data(), W.seg, (size_t)S * sizeof(ScSeg), hipMemcpyDeviceToHost, st));
    RD_HIP(hipMemcpyAsync(got.data(), W.out, (size_t)S * sizeof(ScOut), hipMemcpyDeviceToHost, st));
    RD_HIP(hipStreamSynchronize(st));
    if ((int64_t)n_seg != S) {
        rd_set_error("rd_site_diag_segments: internal: the device found %u sites, the host %lld", n_seg, (long long)S);
        return RD_ERR_STATE;
    }
    for (int64_t s = 0; s < S; s++) {
        segments[4 * s] = got[(size_t)s].site;
        segments[4 * s + 1] = seg[(size_t)s].start;
        segments[4 * s + 2] = seg[(size_t)s].split;
        segments[4 * s + 3] = seg[(size_t)s].end;
    }
    *n_segments = S;
    return RD_OK;
}

// ------------------------------------------------------------------------------------------------------------------ the split, device half
namespace {

struct SsValue {
    __host__ __device__ int64_t operator()(uint64_t key) const { return sc_key_value(key); }
};
struct SsSquare {
    __host__ __device__ int64_t operator()(uint64_t key) const { return (int64_t)sc_key_value(key) * sc_key_value(key); }
};

// the wave's best under ss_better (a total order over the candidates of a site: their cuts differ), in every lane
__device__ inline SsCand ss_wave_best(SsCand b)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        SsCand o;
        o.d = (uint64_t)__shfl_xor((long long)b.d, d);
        o.n_lo = (uint32_t)__shfl_xor((int)b.n_lo, d);
        o.n_hi = (uint32_t)__shfl_xor((int)b.n_hi, d);
        o.cut = __shfl_xor(b.cut, d);
        if (ss_better(o, b)) b = o;
    }
    return b;
}

__global__ __launch_bounds__(64 * SC_WAVES) void ss_item_kernel(const uint64_t* __restrict__ keys, const int64_t* __restrict__ psum,
                                                                const ScSeg* __restrict__ seg, const uint32_t* __restrict__ item_off, uint32_t n_seg,
                                                                uint32_t n_items, const uint32_t* __restrict__ found, int min_frac_q16,
                                                                SsSlot* __restrict__ slot, int32_t* __restrict__ n_cuts)
{
    const int lane = threadIdx.x & 63;
    const uint32_t item = blockIdx.x * (uint32_t)SC_WAVES + (threadIdx.x >> 6);   // (the same in every lane of the wave)
    if (item >= n_items || *found != n_seg || item_off[n_seg] != n_items) return;
    uint32_t lo = 0, hi = n_seg;
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (item_off[mid] <= item) lo = mid;
        else hi = mid;
    }
    const ScSeg sg = seg[lo];
    SsCand best{0, 0, 0, 0};
    int count = 0;
    if (ss_status((int64_t)sg.split - sg.start, (int64_t)sg.end - sg.split) == SC_OK) {
        const int64_t i0 = (int64_t)sg.start + (int64_t)(item - item_off[lo]) * SC_CHUNK, i1 = i0 + SC_CHUNK < (int64_t)sg.end ? i0 + SC_CHUNK : (int64_t)sg.end;
        for (int64_t i = i0 + lane; i < i1; i += 64) {
            SsCand cand;
            if (ss_candidate(keys, psum, sg.start, sg.split, sg.end, i, min_frac_q16, cand)) {
                count++;
                if (ss_better(cand, best)) best = cand;
            }
        }
        best = ss_wave_best(best);
        count = (int)sc_wave_add(count);
    }
    if (lane != 0) return;
    slot[item] = SsSlot{best.d, best.n_lo, best.cut};
    if (count) atomicAdd(n_cuts + lo, count);
}

__global__ __launch_bounds__(64 * SC_WAVES) void ss_pick_kernel(const uint64_t* __restrict__ keys, const int64_t* __restrict__ psum,
                                                                const int64_t* __restrict__ psq, const ScSeg* __restrict__ seg,
                                                                const uint32_t* __restrict__ item_off, uint32_t n_seg, uint32_t n_items,
                                                                const uint32_t* __restrict__ found, const SsSlot* __restrict__ slot,
                                                                const int32_t* __restrict__ n_cuts, SsOut* __restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const uint32_t s = blockIdx.x * (uint32_t)SC_WAVES + (threadIdx.x >> 6);
    if (s >= n_seg || *found != n_seg || item_off[n_seg] != n_items) return;
    const ScSeg sg = seg[s];
    const uint32_t N = sg.end - sg.start;
    SsCand best{0, 0, 0, 0};
    for (uint32_t it = item_off[s] + (uint32_t)lane; it < item_off[s + 1]; it += 64) {
        const SsSlot t = slot[it];
        const SsCand cand{t.d, t.n_lo, N - t.n_lo, t.cut};
        if (ss_better(cand, best)) best = cand;
    }
    best = ss_wave_best(best);
    if (lane == 0) out[s] = ss_entry(keys, psum, psq, sg.start, sg.split, sg.end, best, n_cuts[s]);
}

}  // namespace

extern "C" int rd_site_split(rd_ctx* ctx, const uint32_t* site, const uint8_t* cond, const int16_t* value, int64_t n_events, uint32_t n_sites,
                             int64_t budget_bytes, int64_t capacity, int min_frac_q16, uint32_t* out_site, int32_t* status, int64_t* n, int64_t* sum,
                             int64_t* sumsq, int32_t* cut, int32_t* n_cuts, int64_t* n_lo, int64_t* sum_lo, int64_t* sumsq_lo, int64_t* n_out)
{
    RD_REQUIRE(ctx, "rd_site_split: null context");
    RD_REQUIRE(budget_bytes >= 0 && capacity >= 0, "rd_site_split: negative budget or capacity");
    const SsArrays A{out_site, status, n, sum, sumsq, cut, n_cuts, n_lo, sum_lo, sumsq_lo};
    int rc = ss_check_args("rd_site_split", site, cond, value, n_events, min_frac_q16, A, n_out);
    if (rc) return rc;
    std::vector<ScSite> sites;
    if ((rc = sc_count_checked("rd_site_split", site, cond, n_events, n_sites, capacity, sites))) return rc;
    *n_out = (int64_t)sites.size();
    if (n_events == 0) return RD_OK;
    RD_HIP(hipSetDevice(ctx->device));
    if ((rc = rd_resolve_budget(&budget_bytes, ctx->ws_site.cap))) return rc;   // (this context's block counts as free)
    const BudgetPlan plan = ss_plan(sites, budget_bytes);
    for (size_t j = 0; j < sites.size(); j++) {   // until its launch has run
        SsOut o;
        memset(&o, 0, sizeof o);
        o.site = sites[j].site;
        o.status = SC_TOO_LARGE;
        o.n[0] = (uint32_t)sites[j].n[0];
        o.n[1] = (uint32_t)sites[j].n[1];
        ss_scatter(o, (int64_t)j, A);
    }
    std::vector<int64_t> off;
    std::vector<uint32_t> g_site;
    std::vector<uint8_t> g_cond;
    std::vector<int16_t> g_value;
    const bool whole = plan.launches.size() == 1 && plan.too_large == 0;
    if (!whole) sc_bucket(site, cond, value, n_events, sites, plan, off, g_site, g_cond, g_value);
    std::vector<SsOut> got;
    hipStream_t st = ctx->stream;
    const int end_bit = sc_sort_bits(n_sites);
    for (size_t l = 0; l < plan.launches.size(); l++) {
        const int64_t k0 = plan.launches[l].first, k1 = plan.launches[l].second, S = k1 - k0, j0 = plan.run[k0];
        int64_t nl = 0, items = 0;
        for (int64_t k = k0; k < k1; k++) {
            nl += sites[plan.run[k]].n[0] + sites[plan.run[k]].n[1];
            items += sc_site_chunks(sites[plan.run[k]]);
        }
        const int64_t e0 = whole ? 0 : off[l];
        size_t scan_bytes = 0;
        RD_HIP(rocprim::inclusive_scan(nullptr, scan_bytes, rocprim::make_transform_iterator((const uint64_t*)nullptr, SsValue()), (int64_t*)nullptr,
                                       (size_t)nl, rocprim::plus<int64_t>(), st));
        ScWs W;
        W.min_tmp = scan_bytes;
        W.split_items = items;
        if ((rc = sc_run(ctx, st, (whole ? site : g_site.data()) + e0, (whole ? cond : g_cond.data()) + e0, (whole ? value : g_value.data()) + e0, nl, S,
                         0, end_bit, W)))
            return rc;
        size_t tb = W.tmp_bytes;
        RD_HIP(rocprim::exclusive_scan(W.tmp, tb, W.n_chunk, W.item_off, 0u, (size_t)S + 1, rocprim::plus<uint32_t>(), st));
        tb = W.tmp_bytes;
        RD_HIP(rocprim::inclusive_scan(W.tmp, tb, rocprim::make_transform_iterator(W.sorted, SsValue()), W.psum, (size_t)nl, rocprim::plus<int64_t>(), st));
        tb = W.tmp_bytes;
        RD_HIP(rocprim::inclusive_scan(W.tmp, tb, rocprim::make_transform_iterator(W.sorted, SsSquare()), W.psq, (size_t)nl, rocprim::plus<int64_t>(), st));
        RD_HIP(hipMemsetAsync(W.cnt, 0, (size_t)S * 4, st));
        RD_HIP(hipMemsetAsync(W.split_out, 0, (size_t)S * sizeof(SsOut), st));
        hipLaunchKernelGGL(ss_item_kernel, dim3((unsigned)((items + SC_WAVES - 1) / SC_WAVES)), dim3(64 * SC_WAVES), 0, st, W.sorted, W.psum, W.seg, W.item_off,
                           (uint32_t)S, (uint32_t)items, W.n_seg, min_frac_q16, W.slot, W.cnt);
        RD_HIP(hipGetLastError());
        hipLaunchKernelGGL(ss_pick_kernel, dim3((unsigned)((S + SC_WAVES - 1) / SC_WAVES)), dim3(64 * SC_WAVES), 0, st, W.sorted, W.psum, W.psq, W.seg, W.item_off,
                           (uint32_t)S, (uint32_t)items, W.n_seg, W.slot, W.cnt, W.split_out);
        RD_HIP(hipGetLastError());
        got.resize((size_t)S);
        uint32_t n_seg = 0, n_it = 0;
        RD_HIP(hipMemcpyAsync(&n_seg, W.n_seg, 4, hipMemcpyDeviceToHost, st));
        RD_HIP(hipMemcpyAsync(&n_it, W.item_off + S, 4, hipMemcpyDeviceToHost, st));
        RD_HIP(hipMemcpyAsync(got.data(), W.split_out, (size_t)S * sizeof(SsOut), hipMemcpyDeviceToHost, st));
        RD_HIP(hipStreamSynchronize(st));
        if ((int64_t)n_seg != S || (int64_t)n_it != items) {
            rd_set_error("rd_site_split: internal: the device found %u sites and %u chunks in a launch of %lld and %lld", n_seg, n_it, (long long)S,
                         (long long)items);
            return RD_ERR_STATE;
        }
        for (int64_t j = 0; j < S; j++) ss_scatter(got[(size_t)j], j0 + j, A);
    }
    if (plan.too_large) {
        const ScSite& s = sites[(size_t)plan.first_too_large];
        rd_set_error("rd_site_split: site %u (%lld events) needs %lld bytes of workspace, over the budget of %lld; %lld site(s) not split "
                     "(status RD_SITE_TOO_LARGE), the others were", s.site, (long long)(s.n[0] + s.n[1]), (long long)ss_site_bytes(s),
                     (long long)budget_bytes, (long long)plan.too_large);
        return RD_ERR_NOMEM;
    }
    return RD_OK;
}
#endif  // __HIPCC__
