// ctcalign.hip -- forced (Viterbi) CTC alignment of a given label sequence against a probability matrix: the best path, the
// rows every base occupies, and the probability the model gave the base there (per-base quality).  DESIGN.md section 16.
//
// Contract (exact, not to a tolerance; include/radian_hip.h, rd_ctc_align_batch).  T rows, L labels c_0 .. c_{L-1}, states
// s = 0 .. 2L: even states are blank (class 4), odd state 2i+1 is label i.
//   lp[t][c]  = gm_log((double)P[t][c])                      glibc's log, operation for operation (glibc_math.h); log 0 = -inf
//   V[0][0]   = lp[0][4], V[0][1] = lp[0][c_0], every other V[0][s] = -inf
//   V[t][s]   = lp[t][cls(s)] + max(V[t-1][s], V[t-1][s-1], V[t-1][s-2])     the third only for odd s >= 3 with c_i != c_{i-1}
//               one fp64 max and one fp64 add per cell; a predecessor replaces the best so far only if STRICTLY greater, tried
//               in the order s, s-1, s-2
//   end       = state 2L, or 2L-1 if V[T-1][2L-1] is strictly greater; score = that value; -inf: RD_CTCALIGN_NO_PATH
//
// Kernels, per launch (a set of sequences whose workspace fits the budget):
//   ca_log_kernel   lp rows, 8 doubles each (A C G T blank, then -inf three times: the class of a label past L), once per row
//   ca_dp_kernel    one workgroup per sequence: band_sweep.h's sweep.  A thread's registers: the fp64 values of its 16 states, the
//                   classes of its 8 labels and their skip mask; a double crosses a thread boundary (the thread's first state is
//                   even, a blank: it has no s-2 predecessor, so the left neighbour's last state is all a row needs).  A tile is 32
//                   lp rows, the incoming column in slot 7.  Back-pointers: 2 bits per cell, a thread's 16 cells = one uint32, a row
//                   = ceil((2L+1)/16) consecutive words.  A band starts at row s_lo / 2: the cells above (s > 2t + 1) are -inf and
//                   never on a path.
//   ca_tb_kernel    one lane per sequence: end state, score, status, then the walk -- 8 rows' words (two per row: the path
//                   moves down by at most 2 states per row) fetched at once, walked from registers.
//   ca_qual_kernel  one lane per base: the maximum of P[t][c_i] over its rows, e = 1 - p, and the quality by comparison with
//                   the 50 thresholds 10^(-k/10).
// No atomics; a sequence's result does not depend on what else is in its launch.
#include "common.h"
#include "budget.h"
#include "glibc_math.h"
#include "glibc_tables.h"
#include "band_sweep.h"
#include "../../include/radian_hip.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace {

__device__ const uint64_t g_ca_log_tab[256] = RD_GLIBC_LOG_TAB;

// 10.0 ** (-k / 10) for k = 1 .. 50 as the C library's pow gives them
__device__ const double g_ca_thr[50] = {
    0x1.96b230bcdc434p-1,  0x1.430cd74f6d478p-1,  0x1.009b9cf334252p-1,  0x1.97a967f7524b2p-2,  0x1.43d136248490fp-2,
    0x1.0137987dd704cp-2,  0x1.98a13577c93c0p-3,  0x1.44960c576b375p-3,  0x1.01d3f2d9684d0p-3,  0x1.999999999999ap-4,
    0x1.455b5a30b035cp-4,  0x1.0270ac3f8a9fap-4,  0x1.9a9294b8536e9p-5,  0x1.46211ff90ea2ap-5,  0x1.030dc4ea03a72p-5,
    0x1.9b8c272fbe6dep-6,  0x1.46e75df96dc9ap-6,  0x1.03ab3d12bc2c4p-6,  0x1.9c86515bda14ep-7,  0x1.47ae147ae147bp-7,
    0x1.044914f3c02b0p-7,  0x1.9d811398ddcc0p-8,  0x1.487543c6a9257p-8,  0x1.04e74cc73ee88p-8,  0x1.9e7c6e43390b7p-9,
    0x1.493cec2631f18p-9,  0x1.0585e4c78b079p-9,  0x1.9f7861b7937a3p-10, 0x1.4a050de314dd8p-10, 0x1.0624dd2f1a9fcp-10,
    0x1.a074ee52cd119p-11, 0x1.4acda94717d66p-11, 0x1.06c4363887513p-11, 0x1.a1721471fe40dp-12, 0x1.4b96be9c2da2cp-12,
    0x1.0763f01e8e5adp-12, 0x1.a26fd472780c1p-13, 0x1.4c604e2c75fb6p-13, 0x1.08040b1c10b13p-13, 0x1.a36e2eb1c432dp-14,
    0x1.4d2a58423da81p-14, 0x1.08a4876c1311ep-14, 0x1.a46d238da54ebp-15, 0x1.4df4dd27fe99ep-15, 0x1.09456549be1bdp-15,
    0x1.a56cb36416f83p-16, 0x1.4ebfdd286009ap-16, 0x1.09e6a4f05e62bp-16, 0x1.a66cde934de7dp-17, 0x1.4f8b588e368f1p-17};

constexpr int CA_OK = 0, CA_NO_PATH = 1, CA_TOO_LARGE = 2;   // radian_hip.h RD_CTCALIGN_*
constexpr int CA_MAX_LAUNCH = 32768;       // sequences of one launch (grid.y of the row and base kernels)

struct CaSeq {
    int64_t row0;   // first row of the sequence in the probability buffer
    int64_t lab;    // offset of its labels in the label buffer, and of its per-base results in theirs
    int64_t lp;     // byte offsets into the workspace: log rows [T][8] doubles
    int64_t bp;     //   back-pointer words [T][ceil((2L+1)/16)] uint32
    int64_t col;    //   band columns [2][T] doubles
    int32_t T, L;
};

__device__ __forceinline__ double ca_prob(const void* P, int ptype, int64_t idx)
{
    if (ptype == 1) return ((const double*)P)[idx];
    if (ptype == 2) return (double)(float)((const _Float16*)P)[idx];
    return (double)((const float*)P)[idx];
}

// grid (ceil(max T / 32), sequences): 32 rows x 8 slots per workgroup
__global__ __launch_bounds__(256) void ca_log_kernel(const CaSeq* __restrict__ seqs, const void* __restrict__ P, int ptype, uint8_t* __restrict__ ws,
                                                     double* __restrict__ fin)
{
    const CaSeq q = seqs[blockIdx.y];
    if (blockIdx.x == 0 && threadIdx.x < 2) fin[2 * (int64_t)blockIdx.y + threadIdx.x] = -INFINITY;
    const int64_t t = (int64_t)blockIdx.x * 32 + (threadIdx.x >> 3);
    const int c = threadIdx.x & 7;
    if (t >= q.T) return;
    double v = -INFINITY;
    if (c < 5) v = gm_log(ca_prob(P, ptype, (q.row0 + t) * 5 + c), g_ca_log_tab);
    ((double*)(ws + q.lp))[t * 8 + c] = v;
}

// band_sweep.h's policy of the CTC alignment
struct CaSweep {
    using Cell = double;
    using Elem = double;
    static constexpr bool AHEAD_CLAMPED = false;
    static constexpr int TR = 32, SLOTS = 8;   // a tile: [row][lp of A C G T blank, -inf twice, the band's incoming column value V[t-1][s_lo-1] (band 0: -inf)]
    struct Row {
        double b, c, l[8];   // lp of the blank, the incoming column, lp of the thread's 8 labels
    };
    // the sequence
    const double* __restrict__ lp;
    uint32_t* __restrict__ bp;
    const uint8_t* lab;
    double* fin;   // the sequence's two end values
    int L, wpr;    // wpr: back-pointer words of a row
    // the thread's states of the band
    int s0, cl[8];   // its 8 labels: class (5 = past the sequence: lp -inf)
    uint32_t skip;   //   and whether s-2 is allowed
    double v[BS_K];

    static __device__ __forceinline__ int first_row(int b) { return b * (BS_BAND / 2); }   // rows above have s > 2t + 1 in the whole band
    static __device__ __forceinline__ Cell none() { return -INFINITY; }
    static __device__ __forceinline__ Cell incoming(const Row& in) { return in.c; }
    __device__ __forceinline__ Cell last() const { return v[BS_K - 1]; }

    __device__ __forceinline__ void begin_band(int b)
    {
        s0 = b * BS_BAND + (int)threadIdx.x * BS_K;
        skip = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int i = (s0 >> 1) + j;
            cl[j] = 5;
            if (i < L) {
                cl[j] = lab[i] & 3;
                if (i >= 1 && lab[i] != lab[i - 1]) skip |= 1u << j;
            }
        }
#pragma unroll
        for (int k = 0; k < BS_K; k++) v[k] = -INFINITY;
        // row -1 of band 0: V = 0 in state 0 and -inf elsewhere makes row 0 the contract's start
        if (s0 == 0) v[0] = 0.0;
    }
    __device__ __forceinline__ Elem tile_elem(int e, int tbase, int T, int b, const Cell* cin) const
    {
        const int c = e & 7, t = tbase + (e >> 3);
        Elem x = -INFINITY;
        if (t < T) x = c == 7 && b > 0 ? cin[t - 1] : lp[(size_t)t * 8 + c];
        return x;
    }
    __device__ __forceinline__ Row read_row(const Elem* tile, int r) const
    {
        Row in{tile[r * 8 + 4], tile[r * 8 + 7], {}};
#pragma unroll
        for (int j = 0; j < 8; j++) in.l[j] = tile[r * 8 + cl[j]];
        return in;
    }
    __device__ __forceinline__ void row(int t, const Row& in, Cell left)
    {
        uint32_t bits = 0;
#pragma unroll
        for (int k = BS_K - 1; k >= 0; k--) {
            double best = v[k];
            uint32_t d = 0;
            const double a1 = k >= 1 ? v[k - 1] : left;
            if (a1 > best) {
                best = a1;
                d = 1;
            }
            if (k & 1) {
                const double a2 = k >= 2 ? v[k - 2] : left;
                if (((skip >> (k >> 1)) & 1) && a2 > best) {
                    best = a2;
                    d = 2;
                }
                v[k] = in.l[k >> 1] + best;
            } else {
                v[k] = in.b + best;
            }
            bits |= d << (2 * k);
        }
        if ((s0 >> 4) < wpr) bp[(size_t)t * wpr + (s0 >> 4)] = bits;
    }
    // the two states the path may end in
    __device__ __forceinline__ void end_band() const
    {
#pragma unroll
        for (int k = 0; k < BS_K; k++) {
            if (s0 + k == 2 * L) fin[0] = v[k];
            if (s0 + k == 2 * L - 1) fin[1] = v[k];
        }
    }
};

__global__ __launch_bounds__(BS_NT) void ca_dp_kernel(const CaSeq* __restrict__ seqs, const uint8_t* __restrict__ labels, uint8_t* __restrict__ ws,
                                                      double* __restrict__ fin)
{
    const CaSeq q = seqs[blockIdx.x];
    const int S = 2 * q.L + 1;
    if (q.L > q.T) return;   // no path: the end values stay -inf
    CaSweep p{(const double*)(ws + q.lp), (uint32_t*)(ws + q.bp), labels + q.lab, fin + 2 * (int64_t)blockIdx.x, q.L, (S + 15) / 16};
    band_sweep(p, S, q.T, (double*)(ws + q.col));
}

__global__ __launch_bounds__(64) void ca_tb_kernel(const CaSeq* __restrict__ seqs, int n_seq, const uint8_t* __restrict__ ws,
                                                   const double* __restrict__ fin, double* __restrict__ score, int32_t* __restrict__ status,
                                                   int32_t* __restrict__ first, int32_t* __restrict__ last)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n_seq) return;
    const CaSeq q = seqs[p];
    const int L = q.L;
    int s = 2 * L;
    double sc = fin[2 * (int64_t)p];
    if (L > 0 && fin[2 * (int64_t)p + 1] > sc) {
        sc = fin[2 * (int64_t)p + 1];
        s = 2 * L - 1;
    }
    score[p] = sc;
    if (!(sc > -INFINITY)) {
        status[p] = CA_NO_PATH;
        return;
    }
    status[p] = CA_OK;
    const uint32_t* bp = (const uint32_t*)(ws + q.bp);
    const int64_t wpr = (2 * L + 1 + 15) / 16;
    int32_t* fs = first + q.lab;
    int32_t* ls = last + q.lab;
    int t = q.T - 1, cur = -1;
    while (t > 0) {
        const int n = t < 8 ? t : 8;   // rows t .. t - n + 1
        const int w0 = s >> 4;
        uint32_t a[8], b[8];
#pragma unroll
        for (int r = 0; r < 8; r++) {
            a[r] = b[r] = 0;
            if (r < n) {
                a[r] = bp[(int64_t)(t - r) * wpr + w0];
                if (w0 > 0) b[r] = bp[(int64_t)(t - r) * wpr + w0 - 1];
            }
        }
#pragma unroll
        for (int r = 0; r < 8; r++) {
            if (r < n) {
                const int tt = t - r;
                if ((s & 1) && cur != (s >> 1)) {
                    cur = s >> 1;
                    ls[cur] = tt;
                }
                const uint32_t word = (s >> 4) == w0 ? a[r] : b[r];
                int d = (int)((word >> (2 * (s & 15))) & 3u);
                d = d < s ? d : s;
                if (d && (s & 1)) fs[s >> 1] = tt;
                s -= d;
            }
        }
        t -= n;
    }
    if (s & 1) {
        if (cur != (s >> 1)) ls[s >> 1] = 0;
        fs[s >> 1] = 0;
    }
}

// grid (ceil(max L / 256), sequences)
__global__ __launch_bounds__(256) void ca_qual_kernel(const CaSeq* __restrict__ seqs, const void* __restrict__ P, int ptype,
                                                      const uint8_t* __restrict__ labels, const int32_t* __restrict__ status,
                                                      int32_t* __restrict__ first, int32_t* __restrict__ last, uint8_t* __restrict__ qual)
{
    const CaSeq q = seqs[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= q.L) return;
    if (status[blockIdx.y] != CA_OK) {
        first[q.lab + i] = -1;
        last[q.lab + i] = -1;
        qual[q.lab + i] = 0;
        return;
    }
    const int c = labels[q.lab + i] & 3;
    const int t0 = first[q.lab + i], t1 = last[q.lab + i];
    double p = ca_prob(P, ptype, (q.row0 + t0) * 5 + c);
    for (int t = t0 + 1; t <= t1; t++) {
        const double x = ca_prob(P, ptype, (q.row0 + t) * 5 + c);
        if (x > p) p = x;
    }
    const double e = 1.0 - p;
    int n = 0;
    for (int k = 0; k < 50; k++) n += e <= g_ca_thr[k] ? 1 : 0;
    qual[q.lab + i] = (uint8_t)n;
}

size_t ca_lp_bytes(int64_t T) { return align_up((size_t)T * 64, 256); }
size_t ca_bp_bytes(int64_t T, int64_t L) { return align_up((size_t)T * (size_t)((2 * L + 1 + 15) / 16) * 4, 256); }
size_t ca_col_bytes(int64_t T) { return align_up((size_t)T * 16, 256); }
size_t ca_seq_bytes(int64_t T, int64_t L) { return ca_lp_bytes(T) + ca_bp_bytes(T, L) + ca_col_bytes(T); }

}  // namespace

extern "C" int64_t rd_ctc_align_workspace_bytes(int64_t n_rows, int64_t n_labels)
{
    if (n_rows < 0 || n_labels < 0) return -1;
    return (int64_t)ca_seq_bytes(n_rows, n_labels);
}

namespace {

// a launch's io block (ws_calign) for nb sequences whose label offsets span nlab: descriptors | end values [2] | score | status | first |
// last | qual
struct CaIo {
    CaSeq* seqs;
    double *fin, *score;
    int32_t *status, *first, *last;
    uint8_t* qual;
};
void ca_io_layout(Carve& c, int nb, size_t nlab, CaIo* io)
{
    io->seqs = c.take<CaSeq>((size_t)nb);
    io->fin = c.take<double>((size_t)nb * 2);
    io->score = c.take<double>((size_t)nb);
    io->status = c.take<int32_t>((size_t)nb);
    io->first = c.take<int32_t>(nlab);
    io->last = c.take<int32_t>(nlab);
    io->qual = c.take<uint8_t>(nlab, 256, 1);
}

}  // namespace

int rd_ctc_align_dev(rd_ctx* ctx, hipStream_t st, const void* d_probs, int ptype, const int64_t* seq_off, const int32_t* seq_len, int n_seq,
                     const uint8_t* d_labels, const int64_t* dlab_off, const int32_t* label_len, int64_t budget_bytes, int32_t* first_step,
                     int32_t* last_step, uint8_t* qual, const int64_t* out_off, double* score, int32_t* status)
{
    RD_REQUIRE(ctx && seq_off && seq_len && dlab_off && label_len && out_off && score && status, "ctc_align: null argument");
    RD_REQUIRE(n_seq >= 0 && budget_bytes >= 0, "ctc_align: negative n_seq or budget");
    if (n_seq == 0) return RD_OK;
    int64_t labs_end = 0;
    for (int i = 0; i < n_seq; i++) {
        RD_REQUIRE(seq_len[i] >= 1, "ctc_align: sequence %d has %d rows (at least one is needed)", i, seq_len[i]);
        RD_REQUIRE(label_len[i] >= 0 && label_len[i] < (1 << 29), "ctc_align: sequence %d has %d labels", i, label_len[i]);
        RD_REQUIRE(seq_off[i] >= 0 && dlab_off[i] >= 0 && out_off[i] >= 0, "ctc_align: negative offset at sequence %d", i);
        labs_end = std::max(labs_end, dlab_off[i] + label_len[i]);
    }
    RD_REQUIRE(labs_end == 0 || (d_labels && first_step && last_step && qual), "ctc_align: null label or per-base buffer");
    RD_REQUIRE(d_probs, "ctc_align: null probs");
    if (int rc = rd_resolve_budget(&budget_bytes, ctx->ws_align.cap)) return rc;
    // launches: the sequences in the caller's order, as many as fit the budget; one that alone exceeds it is reported, not launched
    const BudgetPlan plan = rd_plan_budget(n_seq, nullptr, budget_bytes, 0, false,
                                           [&](int i, int) { return (int64_t)ca_seq_bytes(seq_len[i], label_len[i]); },
                                           [](int, int, int64_t count, int64_t) { return count >= CA_MAX_LAUNCH; });
    const std::vector<int32_t>& run = plan.run;
    const int too_large = (int)plan.too_large, first_too_large = (int)plan.first_too_large;
    for (int i = 0; i < n_seq; i++) {   // until its launch has run
        status[i] = CA_TOO_LARGE;
        score[i] = -INFINITY;
        for (int k = 0; k < label_len[i]; k++) {
            first_step[out_off[i] + k] = last_step[out_off[i] + k] = -1;
            qual[out_off[i] + k] = 0;
        }
    }
    if (ctx->ws_align.reserve_exact((size_t)plan.max_bytes, "ctc_align")) return RD_ERR_NOMEM;
    std::vector<CaSeq> desc;
    std::vector<double> h_score;
    std::vector<int32_t> h_status, h_first, h_last;
    std::vector<uint8_t> h_qual;
    for (auto [k0, k1] : plan.launches) {
        const int nb = (int)(k1 - k0);
        desc.resize(nb);
        Carve ws;   // (dry: the descriptors hold offsets into ws_align)
        int64_t lab_lo = INT64_MAX, lab_hi = 0, max_T = 0, max_L = 0;
        for (int k = 0; k < nb; k++) {
            const int i = run[k0 + k];
            CaSeq& d = desc[k];
            d.row0 = seq_off[i];
            d.lab = dlab_off[i];
            d.T = seq_len[i];
            d.L = label_len[i];
            d.lp = (int64_t)ws.mark();
            ws.take<char>(ca_lp_bytes(d.T), 0, 1);
            d.bp = (int64_t)ws.mark();
            ws.take<char>(ca_bp_bytes(d.T, d.L), 0, 1);
            d.col = (int64_t)ws.mark();
            ws.take<char>(ca_col_bytes(d.T), 0, 1);
            if (d.L) {
                lab_lo = std::min(lab_lo, d.lab);
                lab_hi = std::max(lab_hi, d.lab + d.L);
            }
            max_T = std::max<int64_t>(max_T, d.T);
            max_L = std::max<int64_t>(max_L, d.L);
        }
        if (int rc = rd_carve_check("ctc_align", ws, ctx->ws_align.cap)) return rc;
        if (lab_hi <= lab_lo) lab_lo = lab_hi = 0;
        const size_t nlab = (size_t)(lab_hi - lab_lo);   // the per-base results of the launch: the span of its label offsets
        CaIo io;
        if (rd_carve(ctx->ws_calign, [&](Carve& c) { ca_io_layout(c, nb, nlab, &io); })) return RD_ERR_NOMEM;
        uint8_t* dws = ctx->ws_align.as<uint8_t>();
        const CaSeq* d_seqs = io.seqs;
        double *d_fin = io.fin, *d_score = io.score;
        int32_t* d_status = io.status;
        // per-base buffers are indexed by the label offsets: shift them so that the launch's lowest offset is element 0
        int32_t *d_first = io.first - lab_lo, *d_last = io.last - lab_lo;
        uint8_t* d_qual = io.qual - lab_lo;
        RD_HIP(hipMemcpyAsync(io.seqs, desc.data(), (size_t)nb * sizeof(CaSeq), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(ca_log_kernel, dim3((unsigned)((max_T + 31) / 32), nb), dim3(256), 0, st, d_seqs, d_probs, ptype, dws, d_fin);
        RD_HIP(hipGetLastError());
        hipLaunchKernelGGL(ca_dp_kernel, dim3(nb), dim3(BS_NT), 0, st, d_seqs, d_labels, dws, d_fin);
        RD_HIP(hipGetLastError());
        hipLaunchKernelGGL(ca_tb_kernel, dim3((nb + 63) / 64), dim3(64), 0, st, d_seqs, nb, dws, d_fin, d_score, d_status, d_first, d_last);
        RD_HIP(hipGetLastError());
        if (max_L) {
            hipLaunchKernelGGL(ca_qual_kernel, dim3((unsigned)((max_L + 255) / 256), nb), dim3(256), 0, st, d_seqs, d_probs, ptype, d_labels, d_status,
                               d_first, d_last, d_qual);
            RD_HIP(hipGetLastError());
        }
        h_score.resize(nb);
        h_status.resize(nb);
        h_first.resize(nlab);
        h_last.resize(nlab);
        h_qual.resize(nlab);
        RD_HIP(hipMemcpyAsync(h_score.data(), d_score, (size_t)nb * 8, hipMemcpyDeviceToHost, st));
        RD_HIP(hipMemcpyAsync(h_status.data(), d_status, (size_t)nb * 4, hipMemcpyDeviceToHost, st));
        if (nlab) {
            RD_HIP(hipMemcpyAsync(h_first.data(), io.first, nlab * 4, hipMemcpyDeviceToHost, st));
            RD_HIP(hipMemcpyAsync(h_last.data(), io.last, nlab * 4, hipMemcpyDeviceToHost, st));
            RD_HIP(hipMemcpyAsync(h_qual.data(), io.qual, nlab, hipMemcpyDeviceToHost, st));
        }
        RD_HIP(hipStreamSynchronize(st));
        for (int k = 0; k < nb; k++) {
            const int i = run[k0 + k];
            const CaSeq& d = desc[k];
            score[i] = h_score[k];
            status[i] = h_status[k];
            if (d.L) {
                memcpy(first_step + out_off[i], h_first.data() + (d.lab - lab_lo), (size_t)d.L * 4);
                memcpy(last_step + out_off[i], h_last.data() + (d.lab - lab_lo), (size_t)d.L * 4);
                memcpy(qual + out_off[i], h_qual.data() + (d.lab - lab_lo), (size_t)d.L);
            }
        }
    }
    if (too_large) {
        rd_set_error("ctc_align: sequence %d (%d rows x %d labels) needs %lld bytes of workspace, over the budget of %lld; %d sequence(s) not "
                     "aligned (status RD_CTCALIGN_TOO_LARGE), the others were", first_too_large, seq_len[first_too_large], label_len[first_too_large],
                     (long long)ca_seq_bytes(seq_len[first_too_large], label_len[first_too_large]), (long long)budget_bytes, too_large);
        return RD_ERR_NOMEM;
    }
    return RD_OK;
}

extern "C" int rd_ctc_align_batch(rd_ctx* ctx, const void* probs, int prob_is_f64, const int64_t* seq_off, const int32_t* seq_len, int n_seq,
                                  const uint8_t* labels, const int64_t* label_off, const int32_t* label_len, int64_t budget_bytes,
                                  int32_t* first_step, int32_t* last_step, uint8_t* qual, double* score, int32_t* status)
{
    RD_REQUIRE(ctx, "rd_ctc_align_batch: null context");
    RD_REQUIRE(n_seq >= 0, "rd_ctc_align_batch: negative n_seq");
    if (n_seq == 0) return RD_OK;
    RD_REQUIRE(probs && seq_off && seq_len && label_off && label_len && score && status, "rd_ctc_align_batch: null argument");
    RD_REQUIRE(prob_is_f64 == 0 || prob_is_f64 == 1, "rd_ctc_align_batch: prob_is_f64 %d", prob_is_f64);
    RD_REQUIRE(budget_bytes >= 0, "rd_ctc_align_batch: negative budget");
    int64_t rows = 0, labs = 0;
    std::vector<int64_t> dlab(n_seq);
    for (int i = 0; i < n_seq; i++) {
        RD_REQUIRE(seq_off[i] >= 0 && seq_len[i] >= 1, "rd_ctc_align_batch: sequence %d has %d rows at offset %lld (at least one row is needed)", i,
                   seq_len[i], (long long)seq_off[i]);
        RD_REQUIRE(label_len[i] >= 0 && label_len[i] < (1 << 29) && label_off[i] >= 0, "rd_ctc_align_batch: bad labels of sequence %d", i);
        RD_REQUIRE(label_len[i] == 0 || (labels && first_step && last_step && qual), "rd_ctc_align_batch: null label or per-base buffer");
        for (int k = 0; k < label_len[i]; k++)
            RD_REQUIRE(labels[label_off[i] + k] < 4, "rd_ctc_align_batch: label %d of sequence %d is %d, not in 0..3", k, i, labels[label_off[i] + k]);
        rows = std::max(rows, seq_off[i] + seq_len[i]);
        dlab[i] = labs;
        labs += label_len[i];
    }
    RD_HIP(hipSetDevice(ctx->device));
    const size_t rb = prob_is_f64 ? 40 : 20;
    if (ctx->ws_mat.reserve((size_t)(rows + 1) * rb) || ctx->ws_labels.reserve((size_t)labs + 16)) return RD_ERR_NOMEM;
    std::vector<uint8_t> hl((size_t)labs + 16);
    for (int i = 0; i < n_seq; i++)
        if (label_len[i]) memcpy(hl.data() + dlab[i], labels + label_off[i], (size_t)label_len[i]);
    RD_HIP(hipMemcpyAsync(ctx->ws_mat.p, probs, (size_t)rows * rb, hipMemcpyHostToDevice, ctx->stream));
    if (labs) RD_HIP(hipMemcpyAsync(ctx->ws_labels.p, hl.data(), (size_t)labs, hipMemcpyHostToDevice, ctx->stream));
    const int rc = rd_ctc_align_dev(ctx, ctx->stream, ctx->ws_mat.p, prob_is_f64, seq_off, seq_len, n_seq, ctx->ws_labels.as<uint8_t>(), dlab.data(),
                                    label_len, budget_bytes, first_step, last_step, qual, label_off, score, status);
    if (rc == RD_OK || rc == RD_ERR_NOMEM) {
        const hipError_t e = hipStreamSynchronize(ctx->stream);   // (hl is read by the label upload when nothing was launched)
        if (e != hipSuccess && rc == RD_OK) RD_HIP(e);
    }
    return rc;
}
