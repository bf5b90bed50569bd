// polya.hip -- poly(A) tail estimation: the longest stretch of flat, low-variance current in a read's raw samples.  DESIGN.md section 18.
//
// Contract (integer arithmetic only; include/radian_hip.h, rd_polya_segment; the rules themselves are polya_rules.h).  A read of T int16
// samples x, parameters win, flat_q, use_level, lo_q, hi_q, max_gap, min_samples, search_limit:
//   scale     m2 = v1 + v2 (twice the median: the two middle order statistics of x, ranks (T-1)/2 and T/2), d4 = the sum of the two
//             middle order statistics of |2x - m2| (four times the MAD) -- mad_normalise_kernel's order statistics.
//             status: T == 0 EMPTY; else d4 == 0 MAD_ZERO; else T < win SHORT (in this order)
//   windows   nw = T / win; window j = samples [j win, (j+1) win); S_j = sum x, Q_j = sum x^2, V_j = win Q_j - S_j^2
//   flat      A = win flat_q d4, thr = floor(A^2 / 2^20) saturated to 2^64 - 1; window j is flat iff V_j <= thr and, with use_level,
//             lo_q d4 win <= 512 (2 S_j - win m2) <= hi_q d4 win
//   segments  flat windows i < j with no flat window between them are in one segment iff j - i <= max_gap + 1; a segment [a, b] (first and
//             last flat window) is a candidate iff (b - a + 1) win >= min_samples and (search_limit == 0 or a win < search_limit)
//   choice    the candidate with the largest b - a + 1, the smallest a on a tie; none: NONE
//   outputs   tail_start = a win, tail_end = (b + 1) win, n_flat = flat windows in [a, b], sum / sumsq over every sample of
//             [tail_start, tail_end), n_candidates; not OK: -1, -1 and zeros.  m2 and d4 whenever T > 0.
//
// Kernels, on one stream:
//   pa_scale_kernel    one 256-thread workgroup per read: radix_select2 (select.h) twice -> m2, d4, thr
//   pa_window_kernel   one workgroup per 64 windows of a read.  A wave is cut into 64 / g groups of g lanes (g = the power of two >= win,
//                      at most 64); a group owns one window at a time, lane l of it loads samples l, l + g, ... (2-byte loads, consecutive
//                      lanes on consecutive samples; nothing wider is assumed of the read's alignment) and the group's S and Q are
//                      reduced by log2 g xor-shuffles.  Stores the flag (1 B), S (int32) and Q (int64) of every window.
//   pa_segment_kernel  one 256-thread workgroup per read sweeps the flags 256 windows at a time, with a carry from chunk to chunk.  Window
//                      j takes from EXCLUSIVE scans the state left by the windows before it: the last flat window p (max-scan of the
//                      flat indices), the flat count (sum-scan), and -- once p says which flat windows start a segment -- the head of
//                      the segment p is in, (start << 32 | flat count before it), by a max-scan (a segmented scan whose segment value
//                      is its head: heads are monotone).  A flat window that starts a segment CLOSES the one before it, [head, p], and
//                      its thread weighs that candidate; the read's last segment is closed after the sweep.  The best key (length
//                      descending, start ascending) is a workgroup max-reduction; the chosen segment's sums come from S and Q.
// No floating point, no atomics but the select's LDS histogram, no inline assembly.  A result does not depend on the launch's other reads.
#include "common.h"
#include "budget.h"
#include "carve.h"
#include "polya_rules.h"
#include "../../include/radian_hip.h"

#include <cstring>
#include <vector>

namespace {

int pa_check_args(const char* who, const int16_t* raw, const int64_t* read_off, int n_reads, const PaParams& p, const void* const* outs, int n_outs)
{
    RD_REQUIRE(n_reads >= 0, "%s: negative n_reads", who);
    RD_REQUIRE(pa_params_ok(p), "%s: a parameter is outside its range (win 8..256, flat_q 1..32767, use_level 0/1, -2^20 <= lo_q <= hi_q <= 2^20, "
               "max_gap 0..1024, min_samples >= win, search_limit >= 0)", who);
    if (n_reads == 0) return RD_OK;
    RD_REQUIRE(raw && read_off, "%s: null argument", who);
    for (int i = 0; i < n_outs; i++) RD_REQUIRE(outs[i], "%s: null output", who);
    RD_REQUIRE(read_off[0] >= 0, "%s: negative read offset", who);
    for (int r = 0; r < n_reads; r++) {
        RD_REQUIRE(read_off[r + 1] >= read_off[r], "%s: read offsets must be non-decreasing (read %d)", who, r);
        RD_REQUIRE(read_off[r + 1] - read_off[r] <= INT32_MAX, "%s: read %d has more than 2^31 - 1 samples", who, r);
    }
    return RD_OK;
}

// the two middle order statistics of n keys counted in cnt[0 .. n_keys)
void pa_middle(const std::vector<int64_t>& cnt, int n_keys, int64_t n, int* v1, int* v2)
{
    const int64_t k1 = (n - 1) / 2, k2 = n / 2;
    int64_t c = 0;
    *v1 = *v2 = -1;
    for (int k = 0; k < n_keys; k++) {
        c += cnt[k];
        if (*v1 < 0 && k1 < c) *v1 = k;
        if (*v2 < 0 && k2 < c) { *v2 = k; break; }
    }
}

void pa_host_read(const int16_t* x, int64_t T, const PaParams& p, std::vector<int64_t>& cnt, PaOut* o)
{
    *o = PaOut{-1, -1, 0, 0, PA_EMPTY, 0, 0, 0, 0, 0};
    if (T <= 0) return;
    int v1, v2;
    cnt.assign(65536, 0);
    for (int64_t i = 0; i < T; i++) cnt[(int)x[i] + 32768]++;
    pa_middle(cnt, 65536, T, &v1, &v2);
    const int32_t m2 = (v1 - 32768) + (v2 - 32768);
    cnt.assign(131072, 0);
    for (int64_t i = 0; i < T; i++) {
        const int v = 2 * (int)x[i] - m2;
        cnt[v < 0 ? -v : v]++;
    }
    pa_middle(cnt, 131072, T, &v1, &v2);
    const int32_t d4 = v1 + v2;
    o->m2 = m2;
    o->d4 = d4;
    o->status = pa_scale_status(T, p.win, d4);
    if (o->status != PA_OK) return;
    const uint64_t thr = pa_threshold(p.win, p.flat_q, d4);
    const int64_t nw = T / p.win;
    // the open segment [a, b] and its flat count; the best candidate so far
    int64_t a = -1, b = -1;
    int32_t nflat = 0, best_nflat = 0, ncand = 0;
    uint64_t best = 0;
    auto close = [&]() {
        if (a < 0 || !pa_candidate(p, a, b)) return;
        ncand++;
        if (pa_key(a, b) > best) { best = pa_key(a, b); best_nflat = nflat; }
    };
    for (int64_t j = 0; j < nw; j++) {
        int32_t S = 0;
        int64_t Q = 0;
        for (int i = 0; i < p.win; i++) {
            const int v = x[j * p.win + i];
            S += v;
            Q += (int64_t)v * v;
        }
        if (!pa_flat(p, m2, d4, thr, S, Q)) continue;
        if (a >= 0 && pa_joined(p, b, j)) { b = j; nflat++; continue; }
        close();
        a = b = j;
        nflat = 1;
    }
    close();
    o->n_candidates = ncand;
    o->status = best ? PA_OK : PA_NONE;
    if (!best) return;
    const int64_t s = pa_key_start(best), e = s + pa_key_len(best);
    o->tail_start = s * p.win;
    o->tail_end = e * p.win;
    o->n_flat = best_nflat;
    for (int64_t i = o->tail_start; i < o->tail_end; i++) {
        o->sum += x[i];
        o->sumsq += (int64_t)x[i] * x[i];
    }
}

void pa_scatter(const PaOut& o, int r, int32_t* status, int64_t* tail_start, int64_t* tail_end, int32_t* n_flat, int64_t* sum, int64_t* sumsq,
                int32_t* m2, int32_t* d4, int32_t* n_candidates)
{
    status[r] = o.status;
    tail_start[r] = o.tail_start;
    tail_end[r] = o.tail_end;
    n_flat[r] = o.n_flat;
    sum[r] = o.sum;
    sumsq[r] = o.sumsq;
    m2[r] = o.m2;
    d4[r] = o.d4;
    n_candidates[r] = o.n_candidates;
}

}  // namespace

extern "C" int64_t rd_polya_workspace_bytes(int64_t n_samples, int win)
{
    if (n_samples < 0 || win < 8 || win > 256) return -1;
    return 2 * n_samples + 14 * (n_samples / win) + 2048;
}

extern "C" int rd_polya_segment_host(const int16_t* raw, const int64_t* read_off, int n_reads, int win, int flat_q, int use_level, int lo_q, int hi_q,
                                     int max_gap, int64_t min_samples, int64_t search_limit, int32_t* status, int64_t* tail_start,
                                     int64_t* tail_end, int32_t* n_flat, int64_t* sum, int64_t* sumsq, int32_t* m2, int32_t* d4, int32_t* n_candidates)
{
    const PaParams p{win, flat_q, use_level, lo_q, hi_q, max_gap, min_samples, search_limit};
    const void* const outs[9] = {status, tail_start, tail_end, n_flat, sum, sumsq, m2, d4, n_candidates};
    const int rc = pa_check_args("rd_polya_segment_host", raw, read_off, n_reads, p, outs, 9);
    if (rc) return rc;
    std::vector<int64_t> cnt;
    for (int r = 0; r < n_reads; r++) {
        PaOut o;
        pa_host_read(raw + read_off[r], read_off[r + 1] - read_off[r], p, cnt, &o);
        pa_scatter(o, r, status, tail_start, tail_end, n_flat, sum, sumsq, m2, d4, n_candidates);
    }
    return RD_OK;
}

// ------------------------------------------------------------------------------------------------------------------ a launch's device block
namespace {

struct PaRead {
    int64_t raw0;   // the read's sample 0 in the raw buffer
    int64_t w0;     // its window 0 in the window arrays
    int32_t T, nw;
};
struct PaScale {
    uint64_t thr;
    int32_t m2, d4;
};
struct PaBlock {
    int32_t read, j0;   // windows [j0, j0 + PA_WPB) of the read
};

// descriptors, scales and the window arrays
struct PaWs {
    PaRead* reads;
    PaScale* scale;
    PaBlock* blocks;
    uint8_t* flag;
    int32_t* S;
    int64_t* Q;
    int64_t n_windows;
};

void pa_layout(Carve& c, size_t n_reads, size_t n_blocks, int64_t nwin, PaWs* ws)
{
    ws->reads = c.take<PaRead>(n_reads);
    ws->scale = c.take<PaScale>(n_reads);
    ws->blocks = c.take<PaBlock>(n_blocks, 8);
    ws->Q = c.take<int64_t>((size_t)nwin, 8);
    ws->S = c.take<int32_t>((size_t)nwin, 8);
    ws->flag = c.take<uint8_t>((size_t)nwin, 8);
    ws->n_windows = nwin;
}

}  // namespace

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------------------------------ device half
#include "select.h"

namespace {

constexpr int PA_WPB = 64;   // windows per workgroup of the window kernel
constexpr int PA_SEG = 256;  // threads of the segment kernel = windows per chunk of its sweep

__global__ __launch_bounds__(256) void pa_scale_kernel(const PaRead* __restrict__ reads, const int16_t* __restrict__ raw, PaParams p,
                                                       PaScale* __restrict__ scale)
{
    __shared__ unsigned hist[512];
    __shared__ int sh[8];
    const PaRead rd = reads[blockIdx.x];
    const int64_t n = rd.T;
    if (n <= 0) {
        if (threadIdx.x == 0) scale[blockIdx.x] = PaScale{0, 0, 0};
        return;
    }
    const int16_t* x = raw + rd.raw0;
    const int64_t k1 = (n - 1) / 2, k2 = n / 2;
    // the order statistics of mad_normalise_kernel (preprocess.hip): keys x + 32768, then |2x - m2| in [0, 131071]
    const SelectResult m = radix_select2<8>(n, k1, k2, [&](int64_t i) { return (int)x[i] + 32768; }, hist, sh);
    const int m2 = (m.v1 - 32768) + (m.v2 - 32768);
    const SelectResult d = radix_select2<9>(n, k1, k2, [&](int64_t i) { const int v = 2 * (int)x[i] - m2; return v < 0 ? -v : v; }, hist, sh);
    const int d4 = d.v1 + d.v2;
    if (threadIdx.x == 0) scale[blockIdx.x] = PaScale{pa_threshold(p.win, p.flat_q, d4), m2, d4};
}

__global__ __launch_bounds__(256) void pa_window_kernel(const PaBlock* __restrict__ blocks, const PaRead* __restrict__ reads,
                                                        const PaScale* __restrict__ scale, const int16_t* __restrict__ raw, PaParams p, int g,
                                                        uint8_t* __restrict__ flag, int32_t* __restrict__ S_out, int64_t* __restrict__ Q_out)
{
    const PaBlock blk = blocks[blockIdx.x];
    const PaRead rd = reads[blk.read];
    const PaScale sc = scale[blk.read];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int gpw = 64 / g, grp = lane / g, li = lane - grp * g;
    const int jend = blk.j0 + PA_WPB < rd.nw ? blk.j0 + PA_WPB : rd.nw;
    const int16_t* __restrict__ x = raw + rd.raw0;
    for (int jb = blk.j0 + wave * gpw; jb < jend; jb += 4 * gpw) {   // (jb is the same in every lane of the wave)
        const int j = jb + grp;
        const bool live = j < jend;                                  // j < nw: the window's samples are inside the read
        int32_t S = 0;
        int64_t Q = 0;
        if (live) {
            const int16_t* __restrict__ w = x + (int64_t)j * p.win;
            for (int i = li; i < p.win; i += g) {
                const int v = w[i];
                S += v;
                Q += (int64_t)(v * v);
            }
        }
        for (int d = g >> 1; d >= 1; d >>= 1) {                      // groups are aligned to g lanes: the xor stays inside the group
            S += __shfl_xor(S, d);
            Q += __shfl_xor(Q, d);
        }
        if (live && li == 0) {
            const int64_t o = rd.w0 + j;
            flag[o] = pa_flat(p, sc.m2, sc.d4, sc.thr, S, Q) ? 1 : 0;
            S_out[o] = S;
            Q_out[o] = Q;
        }
    }
}

// inclusive scan over the 64 lanes of a wave
template <typename T, typename Op>
__device__ inline T pa_wave_scan(T v, Op op, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T t = __shfl_up(v, d);
        if (lane >= d) v = op(v, t);
    }
    return v;
}

__global__ __launch_bounds__(PA_SEG) void pa_segment_kernel(const PaRead* __restrict__ reads, const PaScale* __restrict__ scale, PaParams p,
                                                            const uint8_t* __restrict__ flag, const int32_t* __restrict__ S_in,
                                                            const int64_t* __restrict__ Q_in, PaOut* __restrict__ out)
{
    __shared__ int32_t sh_p[4], sh_c[4], sh_n[4], sh_pick;
    __shared__ int64_t sh_h[4], sh_s[4], sh_q[4];
    __shared__ unsigned long long sh_k[4];
    const PaRead rd = reads[blockIdx.x];
    const PaScale sc = scale[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    PaOut o{-1, -1, 0, 0, pa_scale_status(rd.T, p.win, sc.d4), 0, rd.T > 0 ? sc.m2 : 0, rd.T > 0 ? sc.d4 : 0, 0, 0};
    if (o.status != PA_OK) {   // (the same in every thread)
        if (tid == 0) out[blockIdx.x] = o;
        return;
    }
    const uint8_t* __restrict__ f = flag + rd.w0;
    const auto imax = [](int32_t a, int32_t b) { return a > b ? a : b; };
    const auto iadd = [](int32_t a, int32_t b) { return a + b; };
    const auto lmax = [](long long a, long long b) { return a > b ? a : b; };
    // the state the windows swept so far leave: the last flat window, the flat count, the head of the open segment
    int32_t carry_p = -1, carry_c = 0;
    long long carry_h = -1;
    unsigned long long best = 0;
    int32_t best_nflat = 0, ncand = 0;
    const auto weigh = [&](long long head, int32_t b, int32_t flats_to_b) {   // the closed segment [head's start, b]
        const int32_t a = (int32_t)(head >> 32), nflat = flats_to_b - (int32_t)(head & 0xffffffffll);
        if (!pa_candidate(p, a, b)) return;
        ncand++;
        const unsigned long long key = pa_key(a, b);
        if (key > best) { best = key; best_nflat = nflat; }
    };
    for (int32_t base = 0; base < rd.nw; base += PA_SEG) {
        const int32_t j = base + tid;
        const bool fl = j < rd.nw && f[j] != 0;
        // scans 1: the last flat index and the flat count
        const int32_t pw = pa_wave_scan<int32_t>(fl ? j : -1, imax, lane), cw = pa_wave_scan<int32_t>(fl ? 1 : 0, iadd, lane);
        if (lane == 63) { sh_p[wave] = pw; sh_c[wave] = cw; }
        __syncthreads();
        int32_t p_ex = carry_p, c_ex = carry_c, p_tot = carry_p, c_tot = carry_c;
        for (int w = 0; w < 4; w++) {
            if (w < wave) { p_ex = imax(p_ex, sh_p[w]); c_ex += sh_c[w]; }
            p_tot = imax(p_tot, sh_p[w]);
            c_tot += sh_c[w];
        }
        const int32_t pl = __shfl_up(pw, 1), cl = __shfl_up(cw, 1);
        if (lane > 0) { p_ex = imax(p_ex, pl); c_ex += cl; }
        const bool start = fl && (p_ex < 0 || !pa_joined(p, p_ex, j));
        // scan 2: the head of the segment the last flat window is in
        const long long hw = pa_wave_scan<long long>(start ? ((long long)j << 32) | (long long)c_ex : -1ll, lmax, lane);
        if (lane == 63) sh_h[wave] = hw;
        __syncthreads();
        long long h_ex = carry_h, h_tot = carry_h;
        for (int w = 0; w < 4; w++) {
            if (w < wave) h_ex = lmax(h_ex, sh_h[w]);
            h_tot = lmax(h_tot, sh_h[w]);
        }
        const long long hl = __shfl_up(hw, 1);
        if (lane > 0) h_ex = lmax(h_ex, hl);
        if (start && p_ex >= 0) weigh(h_ex, p_ex, c_ex);   // this window opens a segment: the one before it is complete
        carry_p = p_tot;
        carry_c = c_tot;
        carry_h = h_tot;
        __syncthreads();   // the four slots are rewritten by the next chunk
    }
    if (tid == 0 && carry_p >= 0) weigh(carry_h, carry_p, carry_c);   // the read's last segment
    // the best key and the number of candidates
    unsigned long long k = best;
    int32_t n = ncand;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long t = (unsigned long long)__shfl_xor((long long)k, d);
        k = t > k ? t : k;
        n += __shfl_xor(n, d);
    }
    if (lane == 0) { sh_k[wave] = k; sh_n[wave] = n; }
    __syncthreads();
    k = sh_k[0];
    n = sh_n[0];
    for (int w = 1; w < 4; w++) {
        k = sh_k[w] > k ? sh_k[w] : k;
        n += sh_n[w];
    }
    o.n_candidates = n;
    if (k == 0) {
        o.status = PA_NONE;
        if (tid == 0) out[blockIdx.x] = o;
        return;
    }
    if (best == k) sh_pick = best_nflat;   // a segment is weighed by one thread only: one writer
    // the chosen segment's sums, from its windows (the gap windows inside it count too)
    const int64_t a = pa_key_start(k), e = a + pa_key_len(k);
    int64_t s = 0, q = 0;
    for (int64_t j = a + tid; j < e; j += PA_SEG) {
        s += S_in[rd.w0 + j];
        q += Q_in[rd.w0 + j];
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        s += __shfl_xor(s, d);
        q += __shfl_xor(q, d);
    }
    if (lane == 0) { sh_s[wave] = s; sh_q[wave] = q; }
    __syncthreads();
    if (tid == 0) {
        o.tail_start = a * p.win;
        o.tail_end = e * p.win;
        o.n_flat = sh_pick;
        o.sum = sh_s[0] + sh_s[1] + sh_s[2] + sh_s[3];
        o.sumsq = sh_q[0] + sh_q[1] + sh_q[2] + sh_q[3];
        out[blockIdx.x] = o;
    }
}

// scale and window kernels (and, with d_out, the segment kernel) for reads whose samples are on the device; read_off is a host array
int pa_run(rd_ctx* ctx, hipStream_t st, const int16_t* d_raw, const int64_t* read_off, int n_reads, const PaParams& p, PaOut* d_out, PaWs* ws)
{
    std::vector<PaRead> reads(n_reads);
    std::vector<PaBlock> blocks;
    int64_t nwin = 0;
    for (int r = 0; r < n_reads; r++) {
        const int64_t T = read_off[r + 1] - read_off[r];
        reads[r] = PaRead{read_off[r], nwin, (int32_t)T, (int32_t)(T / p.win)};
        for (int32_t j0 = 0; j0 < reads[r].nw; j0 += PA_WPB) blocks.push_back(PaBlock{r, j0});
        nwin += reads[r].nw;
    }
    if (rd_carve(ctx->ws_polya, [&](Carve& c) { pa_layout(c, reads.size(), blocks.size(), nwin, ws); })) return RD_ERR_NOMEM;
    RD_HIP(hipMemcpyAsync(ws->reads, reads.data(), reads.size() * sizeof(PaRead), hipMemcpyHostToDevice, st));
    if (!blocks.empty()) RD_HIP(hipMemcpyAsync(ws->blocks, blocks.data(), blocks.size() * sizeof(PaBlock), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(pa_scale_kernel, dim3(n_reads), dim3(256), 0, st, ws->reads, d_raw, p, ws->scale);
    RD_HIP(hipGetLastError());
    if (!blocks.empty()) {
        int g = 8;
        while (g < p.win && g < 64) g <<= 1;
        hipLaunchKernelGGL(pa_window_kernel, dim3((unsigned)blocks.size()), dim3(256), 0, st, ws->blocks, ws->reads, ws->scale, d_raw, p, g, ws->flag,
                           ws->S, ws->Q);
        RD_HIP(hipGetLastError());
    }
    if (d_out) {
        hipLaunchKernelGGL(pa_segment_kernel, dim3(n_reads), dim3(PA_SEG), 0, st, ws->reads, ws->scale, p, ws->flag, ws->S, ws->Q, d_out);
        RD_HIP(hipGetLastError());
    }
    RD_HIP(hipStreamSynchronize(st));   // (the descriptors' copies read the vectors)
    return RD_OK;
}

}  // namespace

int rd_polya_segment_dev(rd_ctx* ctx, hipStream_t st, const int16_t* d_raw, const int64_t* read_off, int n_reads, const PaParams& p, PaOut* d_out)
{
    if (n_reads == 0) return RD_OK;
    PaWs ws;
    return pa_run(ctx, st, d_raw, read_off, n_reads, p, d_out, &ws);
}

extern "C" int rd_polya_segment(rd_ctx* ctx, const int16_t* raw, const int64_t* read_off, int n_reads, int win, int flat_q, int use_level, int lo_q,
                                int hi_q, int max_gap, int64_t min_samples, int64_t search_limit, int64_t budget_bytes, int32_t* status,
                                int64_t* tail_start, int64_t* tail_end, int32_t* n_flat, int64_t* sum, int64_t* sumsq, int32_t* m2, int32_t* d4,
                                int32_t* n_candidates)
{
    RD_REQUIRE(ctx, "rd_polya_segment: null context");
    RD_REQUIRE(budget_bytes >= 0, "rd_polya_segment: negative budget");
    const PaParams p{win, flat_q, use_level, lo_q, hi_q, max_gap, min_samples, search_limit};
    const void* const outs[9] = {status, tail_start, tail_end, n_flat, sum, sumsq, m2, d4, n_candidates};
    int rc = pa_check_args("rd_polya_segment", raw, read_off, n_reads, p, outs, 9);
    if (rc || n_reads == 0) return rc;
    RD_HIP(hipSetDevice(ctx->device));
    if ((rc = rd_resolve_budget(&budget_bytes, ctx->ws_raw.cap + ctx->ws_polya.cap))) return rc;   // (this context's blocks count as free)
    // launches: the reads in the caller's order, as many as fit the budget; a read that alone exceeds it is reported, not launched
    const BudgetPlan plan = rd_plan_budget(n_reads, nullptr, budget_bytes, 0, false,
                                           [&](int r, int) { return rd_polya_workspace_bytes(read_off[r + 1] - read_off[r], win); },
                                           rd_budget_never_closes);
    const int too_large = (int)plan.too_large, first_too_large = (int)plan.first_too_large;
    for (int r = 0; r < n_reads; r++)   // until its launch has run
        pa_scatter(PaOut{-1, -1, 0, 0, PA_TOO_LARGE, 0, 0, 0, 0, 0}, r, status, tail_start, tail_end, n_flat, sum, sumsq, m2, d4, n_candidates);
    std::vector<int64_t> off;
    std::vector<PaOut> got;
    hipStream_t st = ctx->stream;
    for (auto [k0, k1] : plan.launches) {
        const int n = (int)(k1 - k0);
        const int32_t* members = plan.run.data() + k0;
        rd_gather_offsets(read_off, members, n, off);
        if (ctx->ws_raw.reserve((size_t)off[n] * 2 + 16) || ctx->ws_polya_io.reserve((size_t)n * sizeof(PaOut))) return RD_ERR_NOMEM;
        if ((rc = rd_gather_h2d(st, ctx->ws_raw.p, raw, 2, read_off, members, n, off.data()))) return rc;
        if ((rc = rd_polya_segment_dev(ctx, st, ctx->ws_raw.as<int16_t>(), off.data(), n, p, ctx->ws_polya_io.as<PaOut>()))) return rc;
        got.resize(n);
        RD_HIP(hipMemcpyAsync(got.data(), ctx->ws_polya_io.p, (size_t)n * sizeof(PaOut), hipMemcpyDeviceToHost, st));
        RD_HIP(hipStreamSynchronize(st));
        for (int i = 0; i < n; i++) pa_scatter(got[i], members[i], status, tail_start, tail_end, n_flat, sum, sumsq, m2, d4, n_candidates);
    }
    if (too_large) {
        rd_set_error("rd_polya_segment: read %d (%lld samples) needs %lld bytes of workspace, over the budget of %lld; %d read(s) not segmented "
                     "(status RD_POLYA_TOO_LARGE), the others were", first_too_large, (long long)(read_off[first_too_large + 1] - read_off[first_too_large]),
                     (long long)rd_polya_workspace_bytes(read_off[first_too_large + 1] - read_off[first_too_large], win), (long long)budget_bytes, too_large);
        return RD_ERR_NOMEM;
    }
    return RD_OK;
}

extern "C" int rd_polya_diag_windows(rd_ctx* ctx, const int16_t* raw, const int64_t* read_off, int n_reads, int win, int flat_q, int use_level,
                                     int lo_q, int hi_q, int32_t* m2, int32_t* d4, uint64_t* thr, int32_t* win_sum, int64_t* win_sumsq,
                                     uint8_t* win_flat)
{
    RD_REQUIRE(ctx, "rd_polya_diag_windows: null context");
    const PaParams p{win, flat_q, use_level, lo_q, hi_q, 0, win, 0};
    const void* const outs[6] = {m2, d4, thr, win_sum, win_sumsq, win_flat};
    const int rc = pa_check_args("rd_polya_diag_windows", raw, read_off, n_reads, p, outs, 6);
    if (rc || n_reads == 0) return rc;
    RD_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int64_t lo = read_off[0], n = read_off[n_reads] - lo;
    if (ctx->ws_raw.reserve((size_t)n * 2 + 16)) return RD_ERR_NOMEM;
    if (n) RD_HIP(hipMemcpyAsync(ctx->ws_raw.p, raw + lo, (size_t)n * 2, hipMemcpyHostToDevice, st));
    std::vector<int64_t> off(n_reads + 1);
    for (int r = 0; r <= n_reads; r++) off[r] = read_off[r] - lo;
    PaWs ws;
    const int rc2 = pa_run(ctx, st, ctx->ws_raw.as<int16_t>(), off.data(), n_reads, p, nullptr, &ws);
    if (rc2) return rc2;
    std::vector<PaScale> sc(n_reads);
    RD_HIP(hipMemcpyAsync(sc.data(), ws.scale, (size_t)n_reads * sizeof(PaScale), hipMemcpyDeviceToHost, st));
    if (ws.n_windows) {
        RD_HIP(hipMemcpyAsync(win_sum, ws.S, (size_t)ws.n_windows * 4, hipMemcpyDeviceToHost, st));
        RD_HIP(hipMemcpyAsync(win_sumsq, ws.Q, (size_t)ws.n_windows * 8, hipMemcpyDeviceToHost, st));
        RD_HIP(hipMemcpyAsync(win_flat, ws.flag, (size_t)ws.n_windows, hipMemcpyDeviceToHost, st));
    }
    RD_HIP(hipStreamSynchronize(st));
    for (int r = 0; r < n_reads; r++) {
        m2[r] = sc[r].m2;
        d4[r] = sc[r].d4;
        thr[r] = sc[r].thr;
    }
    return RD_OK;
}
#endif  // __HIPCC__
