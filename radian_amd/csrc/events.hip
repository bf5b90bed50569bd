// events.hip -- the per-base event table of a forced alignment: which raw samples every aligned base sits on and what the current
// was there.  DESIGN.md section 17.
//
// Contract (integer arithmetic only; include/radian_hip.h, rd_event_stats).  A read of T samples, L >= 1 labels aligned with status
// RD_CTCALIGN_OK, steps first_step[k] <= last_step[k] (sample indices):
//   event k   = samples [start_k, end_k):  start_k = first_step[k];  end_k = first_step[k+1] for k < L-1, last_step[L-1] + 1 for the
//               last one (a base owns the blank rows after it, as a moves table does).  Events are non-empty and back to back; the
//               samples before first_step[0] and after last_step[L-1] belong to no event.
//   per event   sum and sum of squares (int64), min and max (int16) of the raw int16 samples
//   a read whose status is not OK (or with L = 0): start = end = -1, everything else 0, for each of its labels
// ev_bounds below is that boundary rule: the host loop (rd_event_stats_host), the argument check and the kernel all call it.
//
// Kernel: one wave per 64 consecutive events of a read ("group").  Lane j OWNS event k0 + j (its bounds, its accumulators, its
// six stores); the group's events cover one contiguous sample range, which the wave sweeps 64 samples at a time, lane l loading
// sample base + l (coalesced 2-byte loads, the next chunk's load issued before the current chunk's arithmetic).  Per chunk: every
// sample lane finds its event by a binary search over the owners' starts (6 shuffles), the chunk is combined by a SEGMENTED inclusive
// scan (6 steps; a lane takes its left neighbour at distance d only if that neighbour is not left of its event's first lane in the
// chunk), and every owner whose event meets the chunk pulls the scan value of its event's last lane there.  An event of 10^4 samples is
// therefore 157 chunks of the whole wave, never one lane's loop.  Integer adds and min / max are associative: the result does not
// depend on the chunking, on the other groups of the launch or on the order of the reads.  No atomics, no LDS, no barrier.
#include "common.h"
#include "../../include/radian_hip.h"

#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

namespace {

// event k of L: samples [*start, *end)
__host__ __device__ inline void ev_bounds(const int32_t* first, const int32_t* last, int k, int L, int32_t* start, int32_t* end)
{
    *start = first[k];
    *end = k + 1 < L ? first[k + 1] : last[L - 1] + 1;
}

constexpr int EV_OK = 0;   // RD_CTCALIGN_OK

int ev_check_args(const char* who, const int16_t* raw, const int64_t* read_off, int n_reads, const int32_t* first_step, const int32_t* last_step,
                  const int64_t* label_off, const int32_t* label_len, const int32_t* align_status, const void* const outs[6], int64_t* n_labels)
{
    RD_REQUIRE(n_reads >= 0, "%s: negative n_reads", who);
    *n_labels = 0;
    if (n_reads == 0) return RD_OK;
    RD_REQUIRE(raw && read_off && label_off && label_len && align_status, "%s: null argument", who);
    RD_REQUIRE(read_off[0] >= 0, "%s: negative read offset", who);
    int64_t labs_end = 0;
    for (int r = 0; r < n_reads; r++) {
        RD_REQUIRE(read_off[r + 1] >= read_off[r], "%s: read offsets must be non-decreasing (read %d)", who, r);
        RD_REQUIRE(read_off[r + 1] - read_off[r] <= INT32_MAX, "%s: read %d has more than 2^31 - 1 samples", who, r);
        RD_REQUIRE(label_len[r] >= 0, "%s: read %d has %d labels", who, r, label_len[r]);
        RD_REQUIRE(label_off[r] >= labs_end, "%s: label offsets must be non-decreasing and the reads' labels must not overlap (read %d)", who, r);
        labs_end = label_off[r] + label_len[r];
    }
    *n_labels = labs_end;
    if (labs_end) {
        RD_REQUIRE(first_step && last_step, "%s: null steps", who);
        for (int i = 0; i < 6; i++) RD_REQUIRE(outs[i], "%s: null output", who);
    }
    for (int r = 0; r < n_reads; r++) {
        if (align_status[r] != EV_OK) continue;
        const int64_t T = read_off[r + 1] - read_off[r];
        const int32_t *f = first_step + label_off[r], *l = last_step + label_off[r];
        const int L = label_len[r];
        for (int k = 0; k < L; k++) {
            RD_REQUIRE(0 <= f[k] && f[k] <= l[k] && l[k] < T, "%s: read %d, label %d: steps %d..%d outside 0 <= first <= last < %lld", who, r, k, f[k],
                       l[k], (long long)T);
            RD_REQUIRE(k + 1 == L || l[k] < f[k + 1], "%s: read %d, label %d: last step %d is not before the next label's first step %d", who, r, k,
                       l[k], f[k + 1]);
        }
    }
    return RD_OK;
}

}  // namespace

extern "C" int rd_event_stats_host(const int16_t* raw, const int64_t* read_off, int n_reads, const int32_t* first_step, const int32_t* last_step,
                                   const int64_t* label_off, const int32_t* label_len, const int32_t* align_status, int32_t* ev_start,
                                   int32_t* ev_end, int64_t* ev_sum, int64_t* ev_sumsq, int16_t* ev_min, int16_t* ev_max)
{
    const void* const outs[6] = {ev_start, ev_end, ev_sum, ev_sumsq, ev_min, ev_max};
    int64_t n_labels = 0;
    const int rc = ev_check_args("rd_event_stats_host", raw, read_off, n_reads, first_step, last_step, label_off, label_len, align_status, outs, &n_labels);
    if (rc) return rc;
    for (int r = 0; r < n_reads; r++) {
        const int64_t o = label_off[r];
        const int L = label_len[r];
        const int16_t* x = raw + read_off[r];
        for (int k = 0; k < L; k++) {
            if (align_status[r] != EV_OK) {
                ev_start[o + k] = ev_end[o + k] = -1;
                ev_sum[o + k] = ev_sumsq[o + k] = 0;
                ev_min[o + k] = ev_max[o + k] = 0;
                continue;
            }
            int32_t s, e;
            ev_bounds(first_step + o, last_step + o, k, L, &s, &e);
            int64_t sum = 0, sq = 0;
            int mn = 32767, mx = -32768;
            for (int32_t i = s; i < e; i++) {
                const int v = x[i];
                sum += v;
                sq += (int64_t)v * v;
                mn = v < mn ? v : mn;
                mx = v > mx ? v : mx;
            }
            ev_start[o + k] = s;
            ev_end[o + k] = e;
            ev_sum[o + k] = sum;
            ev_sumsq[o + k] = sq;
            ev_min[o + k] = (int16_t)mn;
            ev_max[o + k] = (int16_t)mx;
        }
    }
    return RD_OK;
}

namespace {

// the step and event arrays of n labels in one device block (ws_events_io)
struct EvIo {
    int32_t *first, *last, *start, *end;
    int64_t *sum, *sumsq;
    int16_t *mn, *mx;
};
void ev_io_layout(Carve& c, int64_t n_labels, EvIo* io)
{
    const size_t n = (size_t)n_labels;
    io->first = c.take<int32_t>(n, 16);
    io->last = c.take<int32_t>(n, 16);
    io->start = c.take<int32_t>(n, 16);
    io->end = c.take<int32_t>(n, 16);
    io->sum = c.take<int64_t>(n, 16);
    io->sumsq = c.take<int64_t>(n, 16);
    io->mn = c.take<int16_t>(n, 16);
    io->mx = c.take<int16_t>(n, 16);
}

}  // namespace

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------------------------------ device half
namespace {

struct EvGroup {
    int64_t raw0;   // the read's sample 0 in the raw buffer
    int64_t lab;    // the read's label 0 in the step and event arrays
    int32_t T, L;   // samples and labels of the read
    int32_t k0;     // first event of the group
    int32_t ok;     // 0: the read has no path -- its labels get -1, -1, 0 ...
};

__global__ __launch_bounds__(64) void ev_stats_kernel(const EvGroup* __restrict__ groups, const int16_t* __restrict__ raw,
                                                      const int32_t* __restrict__ first, const int32_t* __restrict__ last,
                                                      int32_t* __restrict__ ev_start, int32_t* __restrict__ ev_end, int64_t* __restrict__ ev_sum,
                                                      int64_t* __restrict__ ev_sumsq, int16_t* __restrict__ ev_min, int16_t* __restrict__ ev_max)
{
    const EvGroup g = groups[blockIdx.x];
    const int lane = threadIdx.x;
    const int k = g.k0 + lane;
    const bool own = k < g.L;
    const int64_t out = g.lab + k;
    if (!g.ok) {
        if (own) {
            ev_start[out] = ev_end[out] = -1;
            ev_sum[out] = ev_sumsq[out] = 0;
            ev_min[out] = ev_max[out] = 0;
        }
        return;
    }
    // lanes past the group's last event hold an empty event beyond every sample: the search never selects them
    int32_t st = INT32_MAX, en = INT32_MAX;
    if (own) ev_bounds(first + g.lab, last + g.lab, k, g.L, &st, &en);
    const int nev = g.L - g.k0 < 64 ? g.L - g.k0 : 64;
    // the samples the group covers, held inside the read whatever the steps say
    int64_t s0 = __shfl(st, 0), sE = __shfl(en, nev - 1);
    s0 = s0 < 0 ? 0 : s0;
    sE = sE > g.T ? g.T : sE;
    const int16_t* __restrict__ x = raw + g.raw0;
    int64_t a_sum = 0, a_sq = 0;
    int a_min = 32767, a_max = -32768;
    int nxt = s0 + lane < sE ? x[s0 + lane] : 0;
    for (int64_t base = s0; base < sE; base += 64) {
        const int64_t i = base + lane;
        const bool live = i < sE;
        const int v = nxt;
        nxt = i + 64 < sE ? x[i + 64] : 0;
        // the event of sample i: the last owner whose start is <= i
        int e = 0;
#pragma unroll
        for (int step = 32; step >= 1; step >>= 1) {
            const int cand = e + step;
            const int32_t s = __shfl(st, cand & 63);
            if (cand < 64 && s <= i) e = cand;
        }
        const int64_t se = __shfl(st, e);
        const int head = se > base ? (int)(se - base) : 0;   // the event's first lane in this chunk
        int sum = v;                                          // |sum over 64 samples| < 2^21
        int64_t sq = (int64_t)v * v;
        int mn = live ? v : 32767, mx = live ? v : -32768;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t_sum = __shfl_up(sum, d);
            const int64_t t_sq = __shfl_up(sq, d);
            const int t_mn = __shfl_up(mn, d), t_mx = __shfl_up(mx, d);
            if (lane - d >= head) {
                sum += t_sum;
                sq += t_sq;
                mn = t_mn < mn ? t_mn : mn;
                mx = t_mx > mx ? t_mx : mx;
            }
        }
        // owners: the scan value of the event's last lane in this chunk
        const int64_t cend = base + 64 < sE ? base + 64 : sE;
        const bool meets = own && st < cend && en > base;
        const int tail = meets ? (int)((en < cend ? en : cend) - 1 - base) : 0;
        const int p_sum = __shfl(sum, tail & 63);
        const int64_t p_sq = __shfl(sq, tail & 63);
        const int p_mn = __shfl(mn, tail & 63), p_mx = __shfl(mx, tail & 63);
        if (meets) {
            a_sum += p_sum;
            a_sq += p_sq;
            a_min = p_mn < a_min ? p_mn : a_min;
            a_max = p_mx > a_max ? p_mx : a_max;
        }
    }
    if (own) {
        ev_start[out] = st;
        ev_end[out] = en;
        ev_sum[out] = a_sum;
        ev_sumsq[out] = a_sq;
        ev_min[out] = (int16_t)a_min;
        ev_max[out] = (int16_t)a_max;
    }
}

}  // namespace

int rd_event_stats_dev(rd_ctx* ctx, hipStream_t st, const int16_t* d_raw, const int64_t* read_off, int n_reads, const int32_t* d_first,
                       const int32_t* d_last, const int64_t* label_off, const int32_t* label_len, const int32_t* align_status, int32_t* d_start,
                       int32_t* d_end, int64_t* d_sum, int64_t* d_sumsq, int16_t* d_min, int16_t* d_max)
{
    std::vector<EvGroup> groups;
    for (int r = 0; r < n_reads; r++)
        for (int k0 = 0; k0 < label_len[r]; k0 += 64)
            groups.push_back({read_off[r], label_off[r], (int32_t)(read_off[r + 1] - read_off[r]), label_len[r], k0, align_status[r] == EV_OK ? 1 : 0});
    if (groups.empty()) return RD_OK;
    const size_t bytes = groups.size() * sizeof(EvGroup);
    if (ctx->ws_events.reserve(bytes)) return RD_ERR_NOMEM;
    RD_HIP(hipMemcpyAsync(ctx->ws_events.p, groups.data(), bytes, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(ev_stats_kernel, dim3((unsigned)groups.size()), dim3(64), 0, st, ctx->ws_events.as<EvGroup>(), d_raw, d_first, d_last, d_start,
                       d_end, d_sum, d_sumsq, d_min, d_max);
    RD_HIP(hipGetLastError());
    RD_HIP(hipStreamSynchronize(st));   // (the descriptors' copy reads the vector)
    return RD_OK;
}

int rd_event_stats_steps(rd_ctx* ctx, hipStream_t st, const int16_t* d_raw, const int64_t* read_off, int n_reads, const int32_t* first_step,
                         const int32_t* last_step, const int64_t* label_off, const int32_t* label_len, const int32_t* align_status, int64_t n_labels,
                         int32_t* ev_start, int32_t* ev_end, int64_t* ev_sum, int64_t* ev_sumsq, int16_t* ev_min, int16_t* ev_max)
{
    if (n_labels == 0) return RD_OK;
    EvIo io;
    int rc;
    if (rd_carve(ctx->ws_events_io, [&](Carve& c) { ev_io_layout(c, n_labels, &io); })) return RD_ERR_NOMEM;
    const size_t n = (size_t)n_labels;
    RD_HIP(hipMemcpyAsync(io.first, first_step, n * 4, hipMemcpyHostToDevice, st));
    RD_HIP(hipMemcpyAsync(io.last, last_step, n * 4, hipMemcpyHostToDevice, st));
    if ((rc = rd_event_stats_dev(ctx, st, d_raw, read_off, n_reads, io.first, io.last, label_off, label_len, align_status, io.start, io.end, io.sum,
                                 io.sumsq, io.mn, io.mx)))
        return rc;
    for (int r = 0; r < n_reads; r++) {
        const size_t o = (size_t)label_off[r], L = (size_t)label_len[r];
        if (!L) continue;
        RD_HIP(hipMemcpyAsync(ev_start + o, io.start + o, L * 4, hipMemcpyDeviceToHost, st));
        RD_HIP(hipMemcpyAsync(ev_end + o, io.end + o, L * 4, hipMemcpyDeviceToHost, st));
        RD_HIP(hipMemcpyAsync(ev_sum + o, io.sum + o, L * 8, hipMemcpyDeviceToHost, st));
        RD_HIP(hipMemcpyAsync(ev_sumsq + o, io.sumsq + o, L * 8, hipMemcpyDeviceToHost, st));
        RD_HIP(hipMemcpyAsync(ev_min + o, io.mn + o, L * 2, hipMemcpyDeviceToHost, st));
        RD_HIP(hipMemcpyAsync(ev_max + o, io.mx + o, L * 2, hipMemcpyDeviceToHost, st));
    }
    RD_HIP(hipStreamSynchronize(st));
    return RD_OK;
}

extern "C" int rd_event_stats(rd_ctx* ctx, const int16_t* raw, const int64_t* read_off, int n_reads, const int32_t* first_step,
                              const int32_t* last_step, const int64_t* label_off, const int32_t* label_len, const int32_t* align_status,
                              int32_t* ev_start, int32_t* ev_end, int64_t* ev_sum, int64_t* ev_sumsq, int16_t* ev_min, int16_t* ev_max)
{
    RD_REQUIRE(ctx, "rd_event_stats: null context");
    const void* const outs[6] = {ev_start, ev_end, ev_sum, ev_sumsq, ev_min, ev_max};
    int64_t n_labels = 0;
    int rc = ev_check_args("rd_event_stats", raw, read_off, n_reads, first_step, last_step, label_off, label_len, align_status, outs, &n_labels);
    if (rc || n_reads == 0 || n_labels == 0) return rc;
    RD_HIP(hipSetDevice(ctx->device));
    // the samples the reads span, rebased to the first read's
    const int64_t lo = read_off[0], n = read_off[n_reads] - lo;
    if (ctx->ws_raw.reserve((size_t)n * 2 + 16)) return RD_ERR_NOMEM;
    if (n) RD_HIP(hipMemcpyAsync(ctx->ws_raw.p, raw + lo, (size_t)n * 2, hipMemcpyHostToDevice, ctx->stream));
    std::vector<int64_t> off(n_reads + 1);
    for (int r = 0; r <= n_reads; r++) off[r] = read_off[r] - lo;
    return rd_event_stats_steps(ctx, ctx->stream, ctx->ws_raw.as<int16_t>(), off.data(), n_reads, first_step, last_step, label_off, label_len,
                                align_status, n_labels, ev_start, ev_end, ev_sum, ev_sumsq, ev_min, ev_max);
}
#endif  // __HIPCC__
