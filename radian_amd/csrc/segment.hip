// segment.hip -- event detection: a read's raw samples cut into stretches of roughly constant level.  DESIGN.md section 27.
//
// Contract (integer arithmetic only; include/radian_hip.h, rd_segment; the rules themselves are segment_rules.h).  A read of T int16
// samples x, parameters w1, w2, th1, th2, v0.  For a detector with window w and a sample i in [w, T - w]:
//   S1, Q1 = the sum and the sum of squares of x[i - w .. i), S2, Q2 of x[i .. i + w)
//   N(i) = w (S1 - S2)^2, D(i) = w Q1 - S1^2 + w Q2 - S2^2 + 2 w^2 v0 (Welch's t^2 = N / D); outside that range N = 0, D = 1
//   candidate  N(i) > 0 and 16 N(i) >= th D(i)
//   peak       a candidate with t(j) < t(i) for every j in [i - w, i) and t(j) <= t(i) for every j in (i, i + w], j inside the read
//   boundary   a peak of detector 1, or a peak of detector 2 with no peak of detector 1 at |j - i| < w2
//   events     event 0 starts at sample 0, every boundary starts the next one; per event start, sum, sum of squares, min, max and the
//              detector that cut it
//
// Kernels, on one stream; a launch's reads lie back to back in the sample buffer, so its events tile that buffer:
//   sg_peak_kernel     one 256-thread workgroup per tile of 2048 samples of one read.  With W the longer window it stages the tile and
//                      2 W samples to either side in LDS, builds their prefix sums there (int32 sums, int64 sums of squares: a window
//                      sum is two LDS reads), then per detector writes N and D of the tile and W positions to either side to LDS (two
//                      arrays of 8-byte words: consecutive lanes read consecutive words, which a 32-lane half spreads over all 64 banks)
//                      and runs the suppression from there.  The halo is recomputed, nothing is exchanged between workgroups.  One flag
//                      byte per sample: bit 0 peak of detector 1, bit 1 of detector 2
//   sg_combine_kernel  the boundary rule: one byte per sample, 0 no boundary, 1 / 2 the detector, 3 a read's sample 0 (event 0)
//   rocprim::exclusive_scan of (byte != 0) over the launch: the dense index of the event a sample starts
//   sg_start_kernel    a sample that starts an event writes the event's start and detector
//   sg_event_kernel    one wave per run of 64 consecutive events: it walks the run's samples 64 at a time (coalesced), a segmented
//                      shuffle scan keyed by the event index reduces them, and the lane that owns an event picks its part of the chunk
//                      from the last lane of the event's segment.  No atomics: the sums are order-free integers
// No floating point, no scratch, no inline assembly.  A result does not depend on the launch's other reads.
#include "common.h"
#include "budget.h"
#include "segment_rules.h"
#include "eventalign_host.h"
#include "../../include/radian_hip.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace {

struct SgCall {
    const int16_t* raw;
    const int64_t* read_off;
    int n_reads;
    SgParams p;
    const int64_t *sc_lo, *sc_hi, *ev_off;
    int32_t *status, *n_events, *m2, *d4, *ev_start;
    int64_t *ev_sum, *ev_sumsq;
    int16_t *ev_min, *ev_max;
    uint8_t* ev_src;
};

int sg_check_reads(const char* who, const int16_t* raw, const int64_t* read_off, int n_reads, const SgParams& p)
{
    RD_REQUIRE(n_reads >= 0, "%s: negative n_reads", who);
    RD_REQUIRE(sg_params_ok(p), "%s: a parameter is outside its range (w1 2..32, w2 0 or w1 < w2 <= 64, v0 1..65536)", who);
    if (n_reads == 0) return RD_OK;
    RD_REQUIRE(raw && read_off, "%s: null argument", who);
    RD_REQUIRE(read_off[0] >= 0, "%s: negative read offset", who);
    for (int r = 0; r < n_reads; r++) RD_REQUIRE(read_off[r + 1] >= read_off[r], "%s: read offsets must be non-decreasing (read %d)", who, r);
    return RD_OK;
}

int sg_check_args(const char* who, const SgCall& c)
{
    const int rc = sg_check_reads(who, c.raw, c.read_off, c.n_reads, c.p);
    if (rc || c.n_reads == 0) return rc;
    RD_REQUIRE(c.ev_off && c.status && c.n_events && c.ev_start && c.ev_sum && c.ev_sumsq && c.ev_min && c.ev_max && c.ev_src, "%s: null argument", who);
    RD_REQUIRE((c.sc_lo != nullptr) == (c.sc_hi != nullptr), "%s: sc_lo and sc_hi go together", who);
    RD_REQUIRE(!c.sc_lo || (c.m2 && c.d4), "%s: scale windows without m2 / d4 outputs", who);
    RD_REQUIRE(c.ev_off[0] >= 0, "%s: negative event offset", who);
    for (int r = 0; r < c.n_reads; r++) {
        const int64_t T = c.read_off[r + 1] - c.read_off[r], room = c.ev_off[r + 1] - c.ev_off[r];
        RD_REQUIRE(room >= 0, "%s: event offsets must be non-decreasing (read %d)", who, r);
        RD_REQUIRE(sg_status(T) != SG_OK || room >= sg_max_events(T, c.p.w1), "%s: read %d (%lld samples) needs %lld event slots, has %lld", who, r,
                   (long long)T, (long long)sg_max_events(T, c.p.w1), (long long)room);
        RD_REQUIRE(!c.sc_lo || (c.read_off[r] <= c.sc_lo[r] && c.sc_lo[r] <= c.sc_hi[r] && c.sc_hi[r] <= c.read_off[r + 1]),
                   "%s: the scale window of read %d is out of order or outside the read", who, r);
    }
    return RD_OK;
}

void sg_blank(const SgCall& c, int r, int status)
{
    c.status[r] = status;
    c.n_events[r] = 0;
    if (c.m2) c.m2[r] = 0;
    if (c.d4) c.d4[r] = 0;
}

int64_t sg_read_bytes(int64_t T, int32_t w1)
{
    return 8 * T + T / 32 + 32 * sg_max_events(T, w1) + 8 * (T / 2048 + 1) + 8192;
}

// N and D of detector window w at every sample of the read, from its prefix sums
void sg_host_tstat(const std::vector<int64_t>& P, const std::vector<int64_t>& PQ, int64_t T, int32_t w, int32_t v0, std::vector<uint64_t>& N,
                   std::vector<uint64_t>& D)
{
    N.assign(T, 0);
    D.assign(T, 1);
    for (int64_t i = w; w > 0 && i <= T - w; i++) {
        const int32_t S1 = (int32_t)(P[i] - P[i - w]), S2 = (int32_t)(P[i + w] - P[i]);
        N[i] = sg_num(w, S1, S2);
        D[i] = sg_den(w, S1, PQ[i] - PQ[i - w], S2, PQ[i + w] - PQ[i], v0);
    }
}

void sg_host_peaks(const std::vector<uint64_t>& N, const std::vector<uint64_t>& D, int64_t T, int32_t w, uint32_t th, int bit, std::vector<uint8_t>& flags)
{
    for (int64_t i = w; w > 0 && i <= T - w; i++) {
        if (!sg_candidate(N[i], D[i], th)) continue;
        bool peak = true;
        for (int64_t j = std::max<int64_t>(i - w, 0); peak && j <= std::min<int64_t>(i + w, T - 1); j++)
            if (j != i) peak = sg_yields(j, i, N[j], D[j], N[i], D[i]);
        if (peak) flags[i] |= (uint8_t)(1 << bit);
    }
}

struct SgHostBufs {
    std::vector<int64_t> P, PQ;
    std::vector<uint64_t> N, D;
    std::vector<uint8_t> flags;
};

// the flag byte of every sample of a read (bit 0: peak of detector 1, bit 1: of detector 2); tN / tD / the flags to diag arrays when given
void sg_host_flags(const int16_t* x, int64_t T, const SgParams& p, SgHostBufs& b, uint64_t* const* tN, uint64_t* const* tD)
{
    b.P.assign(T + 1, 0);
    b.PQ.assign(T + 1, 0);
    for (int64_t i = 0; i < T; i++) {
        b.P[i + 1] = b.P[i] + x[i];
        b.PQ[i + 1] = b.PQ[i] + (int64_t)x[i] * x[i];
    }
    b.flags.assign(T, 0);
    for (int d = 0; d < 2; d++) {
        sg_host_tstat(b.P, b.PQ, T, sg_window(p, d), p.v0, b.N, b.D);
        sg_host_peaks(b.N, b.D, T, sg_window(p, d), sg_threshold(p, d), d, b.flags);
        if (tN && T) {
            memcpy(tN[d], b.N.data(), (size_t)T * 8);
            memcpy(tD[d], b.D.data(), (size_t)T * 8);
        }
    }
}

}  // namespace

extern "C" int64_t rd_segment_max_events(int64_t n_samples, int w1)
{
    if (n_samples < 0 || w1 < 2 || w1 > 32) return -1;
    return sg_max_events(n_samples, w1);
}

extern "C" int64_t rd_segment_workspace_bytes(int64_t n_samples, int w1)
{
    if (n_samples < 0 || w1 < 2 || w1 > 32) return -1;
    return sg_read_bytes(n_samples, w1);
}

extern "C" int rd_segment_host(const int16_t* raw, const int64_t* read_off, int n_reads, int w1, int w2, uint32_t th1, uint32_t th2, int v0,
                               const int64_t* sc_lo, const int64_t* sc_hi, const int64_t* ev_off, int32_t* status, int32_t* n_events, int32_t* m2,
                               int32_t* d4, int32_t* ev_start, int64_t* ev_sum, int64_t* ev_sumsq, int16_t* ev_min, int16_t* ev_max, uint8_t* ev_src)
{
    const SgCall c{raw, read_off, n_reads, SgParams{w1, w2, th1, th2, v0}, sc_lo, sc_hi, ev_off, status, n_events, m2, d4, ev_start, ev_sum, ev_sumsq,
                   ev_min, ev_max, ev_src};
    const int rc = sg_check_args("rd_segment_host", c);
    if (rc || n_reads == 0) return rc;
    SgHostBufs b;
    std::vector<int64_t> cnt;
    for (int r = 0; r < n_reads; r++) {
        const int64_t T = read_off[r + 1] - read_off[r];
        sg_blank(c, r, sg_status(T));
        if (status[r] != SG_OK) continue;
        const int16_t* x = raw + read_off[r];
        if (sc_lo && sc_hi[r] > sc_lo[r]) ea_host_scale(raw + sc_lo[r], sc_hi[r] - sc_lo[r], cnt, &m2[r], &d4[r]);
        sg_host_flags(x, T, c.p, b, nullptr, nullptr);
        int64_t e = ev_off[r] - 1;
        for (int64_t i = 0; i < T; i++) {
            int src = i == 0 ? 0 : (b.flags[i] & 1) ? 1 : (b.flags[i] & 2) ? 2 : -1;
            for (int64_t j = std::max<int64_t>(i - c.p.w2 + 1, 0); src == 2 && j <= std::min<int64_t>(i + c.p.w2 - 1, T - 1); j++)
                if ((b.flags[j] & 1) && sg_shadows(j, i, c.p.w2)) src = -1;
            if (src >= 0) {
                e++;
                ev_start[e] = (int32_t)i;
                ev_src[e] = (uint8_t)src;
                ev_sum[e] = ev_sumsq[e] = 0;
                ev_min[e] = ev_max[e] = x[i];
            }
            ev_sum[e] += x[i];
            ev_sumsq[e] += (int64_t)x[i] * x[i];
            ev_min[e] = std::min(ev_min[e], x[i]);
            ev_max[e] = std::max(ev_max[e], x[i]);
        }
        n_events[r] = (int32_t)(e + 1 - ev_off[r]);
    }
    return RD_OK;
}

// ------------------------------------------------------------------------------------------------------------------ a launch's device block
namespace {

struct SgRead {
    int64_t raw0;   // the read's sample 0 in the launch's sample buffer
    int32_t T, pad_;
};
struct SgTile {
    int32_t read, t0;   // samples [t0, t0 + SG_TILE) of the read
};
struct SgWs {
    SgRead* reads;
    SgTile* tiles;
    uint8_t *flags, *bnd, *ev_src;
    uint32_t* pos;
    int64_t *ev_g, *ev_sum, *ev_sumsq;
    int16_t *ev_min, *ev_max;
    uint64_t *tN, *tD;
    void* tmp;
    size_t tmp_bytes;
    int64_t n, cap;
    unsigned n_tiles;
};

// n samples, room for cap events, tmp_bytes of scan storage; diag: the two statistics of every sample and detector as well
void sg_layout(Carve& c, size_t n_reads, size_t n_tiles, int64_t n, int64_t cap, size_t tmp_bytes, bool diag, SgWs* ws)
{
    ws->reads = c.take<SgRead>(n_reads);
    ws->tiles = c.take<SgTile>(n_tiles, 8);
    ws->ev_g = c.take<int64_t>((size_t)cap);
    ws->ev_sum = c.take<int64_t>((size_t)cap);
    ws->ev_sumsq = c.take<int64_t>((size_t)cap);
    ws->tN = c.take<uint64_t>(diag ? (size_t)n * 2 : 0, diag ? 8 : 0);
    ws->tD = c.take<uint64_t>(diag ? (size_t)n * 2 : 0, diag ? 8 : 0);
    ws->tmp = c.take<char>(tmp_bytes, 8);
    ws->pos = c.take<uint32_t>((size_t)n + 1);
    ws->ev_min = c.take<int16_t>((size_t)cap);
    ws->ev_max = c.take<int16_t>((size_t)cap);
    ws->flags = c.take<uint8_t>((size_t)n + 1);
    ws->bnd = c.take<uint8_t>((size_t)n + 1);
    ws->ev_src = c.take<uint8_t>((size_t)cap);
    ws->tmp_bytes = tmp_bytes;
    ws->n = n;
    ws->cap = cap;
    ws->n_tiles = (unsigned)n_tiles;
}

}  // namespace

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------------------------------ device half
#include "signal_dev.h"

#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

namespace {

constexpr int SG_TILE = 2048;                                // samples per workgroup of the peak and combine kernels
constexpr int SG_NT = 256;
constexpr int SG_MAX_ST = SG_TILE + 4 * SG_MAX_W;            // staged samples: the tile and 2 W to either side
constexpr int SG_MAX_POS = SG_TILE + 2 * SG_MAX_W + 1;       // positions with N, D: the tile and W to either side
constexpr int64_t SG_MAX_LAUNCH_BYTES = (int64_t)1 << 35;    // a launch's workspace: its samples (under 2^35 / 8) give under 2^32 events

struct SgNonZero {
    __host__ __device__ uint32_t operator()(uint8_t v) const { return v != 0 ? 1u : 0u; }
};

// inclusive scan over the 64 lanes of a wave
template <typename T>
__device__ inline T sg_wave_sum_scan(T v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}

// tN / tD (rd_segment_diag_tstat; null otherwise): N and D of detector d at sample g of the launch go to [d * n_total + g]
__global__ __launch_bounds__(SG_NT) void sg_peak_kernel(const SgTile* __restrict__ tiles, const SgRead* __restrict__ reads,
                                                        const int16_t* __restrict__ raw, SgParams p, uint8_t* __restrict__ flags,
                                                        uint64_t* __restrict__ tN, uint64_t* __restrict__ tD, int64_t n_total)
{
    __shared__ int32_t P[SG_MAX_ST + 1];
    __shared__ int64_t PQ[SG_MAX_ST + 1];
    __shared__ uint64_t sN[SG_MAX_POS], sD[SG_MAX_POS];
    __shared__ int32_t wave_s[4];
    __shared__ int64_t wave_q[4];
    int16_t* xs = (int16_t*)sN;   // the staged samples: read for the last time before the first N is written
    const SgTile tile = tiles[blockIdx.x];
    const SgRead rd = reads[tile.read];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int W = p.w2 > p.w1 ? p.w2 : p.w1, n_st = SG_TILE + 4 * W, n_pos = SG_TILE + 2 * W + 1;
    const int64_t T = rd.T, base = (int64_t)tile.t0 - 2 * W;   // staged sample k is sample base + k of the read
    const int16_t* __restrict__ x = raw + rd.raw0;
    for (int k = tid; k < n_st; k += SG_NT) {
        const int64_t s = base + k;
        xs[k] = s >= 0 && s < T ? x[s] : (int16_t)0;
    }
    __syncthreads();
    // prefix sums: a thread owns `per` consecutive samples; P[k], PQ[k] = the sums of staged samples [0, k)
    const int per = (n_st + SG_NT - 1) / SG_NT, k0 = tid * per, k1 = k0 + per < n_st ? k0 + per : n_st;
    int32_t s = 0;
    int64_t q = 0;
    for (int k = k0; k < k1; k++) {
        const int v = xs[k];
        s += v;
        q += (int64_t)(v * v);
    }
    const int32_t s_in = sg_wave_sum_scan<int32_t>(s, lane);
    const int64_t q_in = sg_wave_sum_scan<int64_t>(q, lane);
    if (lane == 63) { wave_s[wave] = s_in; wave_q[wave] = q_in; }
    __syncthreads();
    int32_t s_run = s_in - s;
    int64_t q_run = q_in - q;
    for (int w = 0; w < wave; w++) { s_run += wave_s[w]; q_run += wave_q[w]; }
    if (tid == 0) { P[0] = 0; PQ[0] = 0; }
    for (int k = k0; k < k1; k++) {
        const int v = xs[k];
        s_run += v;
        q_run += (int64_t)(v * v);
        P[k + 1] = s_run;
        PQ[k + 1] = q_run;
    }
    __syncthreads();
    uint32_t bits = 0;   // two bits for each of the thread's SG_TILE / SG_NT samples
    for (int d = 0; d < 2; d++) {
        const int w = sg_window(p, d);
        const uint32_t th = sg_threshold(p, d);
        // position pp is sample t0 - W + pp of the read, staged sample pp + W
        for (int pp = tid; pp < n_pos; pp += SG_NT) {
            const int64_t i = (int64_t)tile.t0 - W + pp;
            uint64_t N = 0, D = 1;
            if (w > 0 && sg_in_range(i, T, w)) {
                const int k = pp + W;
                const int32_t S1 = P[k] - P[k - w], S2 = P[k + w] - P[k];
                N = sg_num(w, S1, S2);
                D = sg_den(w, S1, PQ[k] - PQ[k - w], S2, PQ[k + w] - PQ[k], p.v0);
            }
            sN[pp] = N;
            sD[pp] = D;
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < SG_TILE / SG_NT; m++) {
            const int qq = m * SG_NT + tid;
            const int64_t i = (int64_t)tile.t0 + qq;
            if (i >= T) continue;
            const int pp = qq + W;
            const uint64_t Ni = sN[pp], Di = sD[pp];
            bool peak = w > 0 && sg_candidate(Ni, Di, th);
            // a position outside the read holds N = 0, D = 1, which a candidate beats: no clamp of j to the read
            for (int dj = -w; peak && dj <= w; dj++)
                if (dj != 0) peak = sg_yields(dj, 0, sN[pp + dj], sD[pp + dj], Ni, Di);
            if (peak) bits |= 1u << (2 * m + d);
            if (tN) {
                tN[(int64_t)d * n_total + rd.raw0 + i] = Ni;
                tD[(int64_t)d * n_total + rd.raw0 + i] = Di;
            }
        }
        __syncthreads();   // the next detector rewrites sN, sD
    }
#pragma unroll
    for (int m = 0; m < SG_TILE / SG_NT; m++) {
        const int64_t i = (int64_t)tile.t0 + m * SG_NT + tid;
        if (i < T) flags[rd.raw0 + i] = (uint8_t)((bits >> (2 * m)) & 3u);
    }
}

__global__ __launch_bounds__(SG_NT) void sg_combine_kernel(const SgTile* __restrict__ tiles, const SgRead* __restrict__ reads, SgParams p,
                                                           const uint8_t* __restrict__ flags, uint8_t* __restrict__ bnd)
{
    const SgTile tile = tiles[blockIdx.x];
    const SgRead rd = reads[tile.read];
    const uint8_t* __restrict__ f = flags + rd.raw0;
    const int64_t T = rd.T;
    for (int m = 0; m < SG_TILE / SG_NT; m++) {
        const int64_t i = (int64_t)tile.t0 + m * SG_NT + threadIdx.x;
        if (i >= T) continue;
        const uint8_t fl = f[i];
        uint8_t b = i == 0 ? 3 : (fl & 1) ? 1 : (fl & 2) ? 2 : 0;
        if (b == 2) {
            const int64_t lo = i - p.w2 + 1 > 0 ? i - p.w2 + 1 : 0, hi = i + p.w2 - 1 < T - 1 ? i + p.w2 - 1 : T - 1;
            for (int64_t j = lo; j <= hi; j++)
                if ((f[j] & 1) && sg_shadows(j, i, p.w2)) b = 0;
        }
        bnd[rd.raw0 + i] = b;
    }
}

// cap: the entries the event arrays hold (the sum of the reads' rd_segment_max_events; an event index stays below it by the contract)
__global__ __launch_bounds__(SG_NT) void sg_start_kernel(const uint8_t* __restrict__ bnd, const uint32_t* __restrict__ pos, int64_t n, int64_t cap,
                                                         int64_t* __restrict__ ev_g, uint8_t* __restrict__ ev_src)
{
    const int64_t g = (int64_t)blockIdx.x * SG_NT + threadIdx.x;
    if (g >= n) return;
    const uint8_t b = bnd[g];
    const int64_t e = pos[g];
    if (b == 0 || e >= cap) return;
    ev_g[e] = g;
    ev_src[e] = b == 3 ? (uint8_t)0 : b;
}

__global__ __launch_bounds__(SG_NT) void sg_event_kernel(const int16_t* __restrict__ raw, const uint8_t* __restrict__ bnd,
                                                         const uint32_t* __restrict__ pos, const int64_t* __restrict__ ev_g, int64_t n,
                                                         int64_t n_ev, int64_t* __restrict__ ev_sum, int64_t* __restrict__ ev_sumsq,
                                                         int16_t* __restrict__ ev_min, int16_t* __restrict__ ev_max)
{
    const int lane = threadIdx.x & 63;
    const int64_t e0 = ((int64_t)blockIdx.x * (SG_NT / 64) + (threadIdx.x >> 6)) * 64, e = e0 + lane;   // (e0 is the same in every lane)
    if (e0 >= n_ev) return;
    const bool own = e < n_ev;
    // the lane's event is samples [lo, hi) of the launch; the events tile the sample buffer
    const int64_t lo = own ? ev_g[e] : n, hi = own && e + 1 < n_ev ? ev_g[e + 1] : n;
    const int64_t a = __shfl(lo, 0), b = e0 + 64 < n_ev ? __shfl(hi, 63) : n;
    if (a < 0 || b > n) return;   // (never: the starts are sample indices of the launch)
    int64_t sum = 0, sumsq = 0;
    int mn = 32767, mx = -32768;
    for (int64_t c = a; c < b; c += 64) {
        const int64_t g = c + lane;
        const bool live = g < b;
        const int v = live ? raw[g] : 0;
        // the event of the lane's sample, counted from e0; the lanes past the run's end share a key no event has
        int key = live ? (int)((int64_t)pos[g] + (bnd[g] != 0 ? 1 : 0) - 1 - e0) : 64;
        int32_t S = v;
        int64_t Q = (int64_t)(v * v);
        int lo_v = live ? v : 32767, hi_v = live ? v : -32768;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {   // the keys do not decrease along the wave: a lane d below with the same key is in the same segment
            const int k2 = __shfl_up(key, d);
            const int32_t S2 = __shfl_up(S, d);
            const int64_t Q2 = __shfl_up(Q, d);
            const int l2 = __shfl_up(lo_v, d), h2 = __shfl_up(hi_v, d);
            if (lane >= d && k2 == key) {
                S += S2;
                Q += Q2;
                lo_v = l2 < lo_v ? l2 : lo_v;
                hi_v = h2 > hi_v ? h2 : hi_v;
            }
        }
        // the event's samples inside this chunk end at lane `last`: that lane's values are the event's part of the chunk
        const bool meets = own && lo < c + 64 && hi > c;
        const int last = meets ? (int)((hi < c + 64 ? hi : c + 64) - 1 - c) : lane;
        const int32_t S3 = __shfl(S, last);
        const int64_t Q3 = __shfl(Q, last);
        const int l3 = __shfl(lo_v, last), h3 = __shfl(hi_v, last);
        if (meets) {
            sum += S3;
            sumsq += Q3;
            mn = l3 < mn ? l3 : mn;
            mx = h3 > mx ? h3 : mx;
        }
    }
    if (own) {
        ev_sum[e] = sum;
        ev_sumsq[e] = sumsq;
        ev_min[e] = (int16_t)mn;
        ev_max[e] = (int16_t)mx;
    }
}

// lays the launch out in ctx->ws_segment, uploads its descriptors and runs the peak kernel; off: the reads' offsets in the sample buffer
int sg_peaks(rd_ctx* ctx, hipStream_t st, const int16_t* d_raw, const int64_t* off, int nb, const SgParams& p, bool diag, SgWs* ws,
             std::vector<SgRead>& reads, std::vector<SgTile>& tiles)
{
    reads.resize(nb);
    tiles.clear();
    int64_t cap = 0;
    for (int i = 0; i < nb; i++) {
        const int64_t T = off[i + 1] - off[i];
        reads[i] = SgRead{off[i], (int32_t)T, 0};
        for (int64_t t0 = 0; t0 < T; t0 += SG_TILE) tiles.push_back(SgTile{i, (int32_t)t0});
        cap += sg_max_events(T, p.w1);
    }
    const int64_t n = off[nb];
    size_t tmp_bytes = 0;
    RD_HIP(rocprim::exclusive_scan(nullptr, tmp_bytes, rocprim::make_transform_iterator((const uint8_t*)nullptr, SgNonZero()), (uint32_t*)nullptr, 0u,
                                   (size_t)n + 1, rocprim::plus<uint32_t>(), st));
    if (rd_carve(ctx->ws_segment, [&](Carve& c) { sg_layout(c, reads.size(), tiles.size(), n, cap, tmp_bytes, diag, ws); })) return RD_ERR_NOMEM;
    RD_HIP(hipMemcpyAsync(ws->reads, reads.data(), reads.size() * sizeof(SgRead), hipMemcpyHostToDevice, st));
    RD_HIP(hipMemcpyAsync(ws->tiles, tiles.data(), tiles.size() * sizeof(SgTile), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(sg_peak_kernel, dim3(ws->n_tiles), dim3(SG_NT), 0, st, ws->tiles, ws->reads, d_raw, p, ws->flags, diag ? ws->tN : nullptr,
                       diag ? ws->tD : nullptr, n);
    RD_HIP(hipGetLastError());
    return RD_OK;
}

// one launch: members of the call (non-empty reads, in this order), their samples already at d_raw + off[i]
int sg_launch(rd_ctx* ctx, hipStream_t st, const SgCall& c, const int32_t* members, int nb, const int64_t* off, std::vector<SgRead>& reads,
              std::vector<SgTile>& tiles, std::vector<int64_t>& h_g, std::vector<int64_t>& h_sum, std::vector<int64_t>& h_sq,
              std::vector<int16_t>& h_min, std::vector<int16_t>& h_max, std::vector<uint8_t>& h_src)
{
    const int16_t* d_raw = ctx->ws_raw.as<int16_t>();
    SgWs ws;
    int rc = sg_peaks(ctx, st, d_raw, off, nb, c.p, false, &ws, reads, tiles);
    if (rc) return rc;
    const int64_t n = ws.n;
    RD_HIP(hipMemsetAsync(ws.bnd + n, 0, 1, st));
    hipLaunchKernelGGL(sg_combine_kernel, dim3(ws.n_tiles), dim3(SG_NT), 0, st, ws.tiles, ws.reads, c.p, ws.flags, ws.bnd);
    RD_HIP(hipGetLastError());
    size_t tb = ws.tmp_bytes;
    RD_HIP(rocprim::exclusive_scan(ws.tmp, tb, rocprim::make_transform_iterator((const uint8_t*)ws.bnd, SgNonZero()), ws.pos, 0u, (size_t)n + 1,
                                   rocprim::plus<uint32_t>(), st));
    uint32_t total = 0;
    RD_HIP(hipMemcpyAsync(&total, ws.pos + n, 4, hipMemcpyDeviceToHost, st));
    RD_HIP(hipStreamSynchronize(st));   // (the descriptors' copies read the vectors, too)
    const int64_t n_ev = total;
    if (n_ev < nb || n_ev > ws.cap) {
        rd_set_error("rd_segment: %lld events of %d reads against a bound of %lld", (long long)n_ev, nb, (long long)ws.cap);
        return RD_ERR_STATE;
    }
    hipLaunchKernelGGL(sg_start_kernel, dim3((unsigned)((n + SG_NT - 1) / SG_NT)), dim3(SG_NT), 0, st, ws.bnd, ws.pos, n, ws.cap, ws.ev_g, ws.ev_src);
    RD_HIP(hipGetLastError());
    hipLaunchKernelGGL(sg_event_kernel, dim3((unsigned)((n_ev + SG_NT - 1) / SG_NT)), dim3(SG_NT), 0, st, d_raw, ws.bnd, ws.pos, ws.ev_g, n, n_ev,
                       ws.ev_sum, ws.ev_sumsq, ws.ev_min, ws.ev_max);
    RD_HIP(hipGetLastError());
    h_g.resize(n_ev);
    h_sum.resize(n_ev);
    h_sq.resize(n_ev);
    h_min.resize(n_ev);
    h_max.resize(n_ev);
    h_src.resize(n_ev);
    RD_HIP(hipMemcpyAsync(h_g.data(), ws.ev_g, (size_t)n_ev * 8, hipMemcpyDeviceToHost, st));
    RD_HIP(hipMemcpyAsync(h_sum.data(), ws.ev_sum, (size_t)n_ev * 8, hipMemcpyDeviceToHost, st));
    RD_HIP(hipMemcpyAsync(h_sq.data(), ws.ev_sumsq, (size_t)n_ev * 8, hipMemcpyDeviceToHost, st));
    RD_HIP(hipMemcpyAsync(h_min.data(), ws.ev_min, (size_t)n_ev * 2, hipMemcpyDeviceToHost, st));
    RD_HIP(hipMemcpyAsync(h_max.data(), ws.ev_max, (size_t)n_ev * 2, hipMemcpyDeviceToHost, st));
    RD_HIP(hipMemcpyAsync(h_src.data(), ws.ev_src, (size_t)n_ev, hipMemcpyDeviceToHost, st));
    RD_HIP(hipStreamSynchronize(st));
    // the dense events back to their reads: read i holds those that start in [off[i], off[i + 1])
    int64_t e = 0;
    for (int i = 0; i < nb; i++) {
        const int r = members[i];
        const int64_t room = sg_max_events(off[i + 1] - off[i], c.p.w1);
        int64_t k = 0;
        for (; e < n_ev && h_g[e] < off[i + 1]; e++, k++) {
            if (k >= room || h_g[e] < off[i]) {
                rd_set_error("rd_segment: read %d came to more than %lld events", r, (long long)room);
                return RD_ERR_STATE;
            }
            const int64_t o = c.ev_off[r] + k;
            c.ev_start[o] = (int32_t)(h_g[e] - off[i]);
            c.ev_sum[o] = h_sum[e];
            c.ev_sumsq[o] = h_sq[e];
            c.ev_min[o] = h_min[e];
            c.ev_max[o] = h_max[e];
            c.ev_src[o] = h_src[e];
        }
        c.status[r] = SG_OK;
        c.n_events[r] = (int32_t)k;
    }
    if (c.sc_lo) {
        std::vector<SignalScaleIn> scin(nb);
        std::vector<int32_t> scale;
        for (int i = 0; i < nb; i++) {
            const int r = members[i];
            scin[i] = signal_scale_in(off[i] + c.sc_lo[r] - c.read_off[r], c.sc_hi[r] - c.sc_lo[r], 1, 1, 0, 0);
        }
        if ((rc = signal_scales(ctx, st, d_raw, scin, 1, scale))) return rc;
        for (int i = 0; i < nb; i++) {
            c.m2[members[i]] = scale[2 * (size_t)i];
            c.d4[members[i]] = scale[2 * (size_t)i + 1];
        }
    }
    return RD_OK;
}

}  // namespace

extern "C" int rd_segment(rd_ctx* ctx, const int16_t* raw, const int64_t* read_off, int n_reads, int w1, int w2, uint32_t th1, uint32_t th2, int v0,
                          const int64_t* sc_lo, const int64_t* sc_hi, const int64_t* ev_off, int64_t budget_bytes, int32_t* status,
                          int32_t* n_events, int32_t* m2, int32_t* d4, int32_t* ev_start, int64_t* ev_sum, int64_t* ev_sumsq, int16_t* ev_min,
                          int16_t* ev_max, uint8_t* ev_src)
{
    RD_REQUIRE(ctx, "rd_segment: null context");
    RD_REQUIRE(budget_bytes >= 0, "rd_segment: negative budget");
    const SgCall c{raw, read_off, n_reads, SgParams{w1, w2, th1, th2, v0}, sc_lo, sc_hi, ev_off, status, n_events, m2, d4, ev_start, ev_sum, ev_sumsq,
                   ev_min, ev_max, ev_src};
    int rc = sg_check_args("rd_segment", c);
    if (rc || n_reads == 0) return rc;
    RD_HIP(hipSetDevice(ctx->device));
    if ((rc = rd_resolve_budget(&budget_bytes, ctx->ws_raw.cap + ctx->ws_segment.cap))) return rc;   // (this context's blocks count as free)
    // launches: the reads with samples to look at, in the caller's order, as many as fit the budget; a read that alone exceeds it is
    // reported, not launched
    for (int r = 0; r < n_reads; r++) {
        const int stat = sg_status(read_off[r + 1] - read_off[r]);
        sg_blank(c, r, stat == SG_OK ? SG_TOO_LARGE : stat);   // OK: until its launch has run
    }
    const auto bytes = [&](int r, int) { return status[r] == SG_TOO_LARGE ? sg_read_bytes(read_off[r + 1] - read_off[r], w1) : (int64_t)-1; };
    const BudgetPlan plan = rd_plan_budget(n_reads, nullptr, budget_bytes, 0, false, bytes,
                                           [&](int r, int, int64_t, int64_t acc) { return acc + bytes(r, -1) > SG_MAX_LAUNCH_BYTES; });
    std::vector<int64_t> off, h_g, h_sum, h_sq;
    std::vector<int16_t> h_min, h_max;
    std::vector<uint8_t> h_src;
    std::vector<SgRead> reads;
    std::vector<SgTile> tiles;
    hipStream_t st = ctx->stream;
    for (auto [k0, k1] : plan.launches) {
        const int nb = (int)(k1 - k0);
        const int32_t* members = plan.run.data() + k0;
        rd_gather_offsets(read_off, members, nb, off);
        if (ctx->ws_raw.reserve((size_t)off[nb] * 2 + 16)) return RD_ERR_NOMEM;
        if ((rc = rd_gather_h2d(st, ctx->ws_raw.p, raw, 2, read_off, members, nb, off.data()))) return rc;
        if ((rc = sg_launch(ctx, st, c, members, nb, off.data(), reads, tiles, h_g, h_sum, h_sq, h_min, h_max, h_src))) return rc;
    }
    if (plan.too_large) {
        const int r = (int)plan.first_too_large;
        rd_set_error("rd_segment: read %d (%lld samples) needs %lld bytes of workspace, over the budget of %lld; %d read(s) not segmented "
                     "(status RD_SEGMENT_TOO_LARGE), the others were", r, (long long)(read_off[r + 1] - read_off[r]),
                     (long long)sg_read_bytes(read_off[r + 1] - read_off[r], w1), (long long)budget_bytes, (int)plan.too_large);
        return RD_ERR_NOMEM;
    }
    return RD_OK;
}

extern "C" int rd_segment_diag_tstat(rd_ctx* ctx, const int16_t* raw, const int64_t* read_off, int n_reads, int w1, int w2, uint32_t th1,
                                     uint32_t th2, int v0, uint64_t* t_num, uint64_t* t_den, uint8_t* peak)
{
    RD_REQUIRE(ctx, "rd_segment_diag_tstat: null context");
    const SgParams p{w1, w2, th1, th2, v0};
    const int rc = sg_check_reads("rd_segment_diag_tstat", raw, read_off, n_reads, p);
    if (rc || n_reads == 0) return rc;
    RD_REQUIRE(t_num && t_den && peak, "rd_segment_diag_tstat: null output");
    const int64_t lo = read_off[0], n = read_off[n_reads] - lo;
    for (int r = 0; r < n_reads; r++)
        RD_REQUIRE(read_off[r + 1] - read_off[r] <= SG_MAX_T, "rd_segment_diag_tstat: read %d has more than 2^30 samples", r);
    RD_REQUIRE(n < ((int64_t)1 << 31), "rd_segment_diag_tstat: more than 2^31 - 1 samples in one call");
    if (n == 0) return RD_OK;
    RD_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (ctx->ws_raw.reserve((size_t)n * 2 + 16)) return RD_ERR_NOMEM;
    RD_HIP(hipMemcpyAsync(ctx->ws_raw.p, raw + lo, (size_t)n * 2, hipMemcpyHostToDevice, st));
    // the reads with samples, rebased to the first
    std::vector<int64_t> off(1, 0);
    for (int r = 0; r < n_reads; r++)
        if (read_off[r + 1] > read_off[r]) off.push_back(read_off[r + 1] - lo);
    SgWs ws;
    std::vector<SgRead> reads;
    std::vector<SgTile> tiles;
    const int rc2 = sg_peaks(ctx, st, ctx->ws_raw.as<int16_t>(), off.data(), (int)off.size() - 1, p, true, &ws, reads, tiles);
    if (rc2) return rc2;
    for (int d = 0; d < 2; d++) {
        RD_HIP(hipMemcpyAsync(t_num + (size_t)d * n, ws.tN + (size_t)d * n, (size_t)n * 8, hipMemcpyDeviceToHost, st));
        RD_HIP(hipMemcpyAsync(t_den + (size_t)d * n, ws.tD + (size_t)d * n, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    }
    RD_HIP(hipMemcpyAsync(peak, ws.flags, (size_t)n, hipMemcpyDeviceToHost, st));
    RD_HIP(hipStreamSynchronize(st));
    return RD_OK;
}
#endif  // __HIPCC__
