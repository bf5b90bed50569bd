// ctc.hip -- model evaluation on labelled windows: the CTC loss of Keras's ctc_batch_cost (radian/model.py:77-98, the
// reference's val_loss) and a greedy decode scored by edit distance against the label, on the MI355X.  Evaluation only:
// no gradients.
//
// Contract, per window with softmax rows y[t][0..4] (A, C, G, T, blank), n = input_length rows counted and labels l[0..L-1]:
//   p[t][k] = (y[t][k] + 1e-7) / sum_j (y[t][j] + 1e-7)          (log(y + epsilon) then TF's log-softmax)
//   loss = -log sum over paths pi of length n that collapse to l (repeats merged, then blanks dropped) of prod_t p[t][pi_t]
// computed in fp64 (the per-row transform and every accumulator).  A window without such a path (L + adjacent equal labels > n)
// has loss +inf and status RD_CTC_INFEASIBLE.
//   greedy: argmax of each of the first n rows of y (lowest class on a tie), repeats collapsed, blanks dropped;
//   edit distance: Levenshtein (unit costs) between the greedy labels and l.
//
// ctc_alpha_kernel: one wave per window.  The S = 2L + 1 states of the extended label (blank, l0, blank, l1, ..., blank) are
// spread over the lanes, lane owning s = lane + 64k (k < ceil(S / 64) <= 8, registers).  One serial step per row: each state
// takes alpha(s - 1) and alpha(s - 2) of the previous row from lanes l - 1 / l - 2 by DPP wave_shr:1 (lane 0: from lanes 63 / 62
// of the block below, v_readlane), then alpha(s) = logaddexp of the two or three + log p[t][class of s].  The log p of 64 rows
// are computed one row per lane ahead of the steps and broadcast with v_readlane.  No LDS except two doubles at the end.
//
// ctc_greedy_ed_kernel: one wave per window.  Greedy labels: 64 rows per pass, one row per lane, kept flags compacted with a
// ballot into LDS.  Edit distance: rows = greedy labels, columns j = 0..L owned lane-wise (j = lane + 64c, c < 4, registers);
// a row is D[i][j] = j + prefix-min over k <= j of (T[k] - k), T[k] = min(D[i-1][k] + 1, D[i-1][k-1] + (g_i != l_k)), T[0] = i,
// a 64-lane min scan per block of columns.
#include "common.h"
#include "../../include/radian_hip.h"

#include <cmath>
#include <cstring>

namespace {

constexpr int CTC_T = RD_CTC_T;
constexpr int CTC_MAXL = RD_CTC_MAX_LABEL;
constexpr int CTC_KS = (2 * CTC_MAXL + 1 + 63) / 64;   // 8 state blocks per lane
constexpr int ED_KC = (CTC_MAXL + 1 + 63) / 64;        // 4 column blocks per lane
constexpr double CTC_EPS = 1e-7;                        // Keras backend epsilon()

struct CtcWin {
    int64_t lab;   // offset of the window's labels in the label array
    int32_t n;     // input_length
    int32_t L;     // label_length
};

// lane l receives v of lane l - 1, lane 0 receives edge (DPP wave_shr:1, bound_ctrl off: the invalid source keeps `old`)
__device__ __forceinline__ int ctc_shr1(int v, int edge) { return __builtin_amdgcn_update_dpp(edge, v, 0x138, 0xf, 0xf, false); }

__device__ __forceinline__ double ctc_shr1d(double v, double edge)
{
    const int2 a = __builtin_bit_cast(int2, v), e = __builtin_bit_cast(int2, edge);
    return __builtin_bit_cast(double, make_int2(ctc_shr1(a.x, e.x), ctc_shr1(a.y, e.y)));
}

__device__ __forceinline__ double ctc_readlane(double v, int l)
{
    const int2 a = __builtin_bit_cast(int2, v);
    return __builtin_bit_cast(double, make_int2(__builtin_amdgcn_readlane(a.x, l), __builtin_amdgcn_readlane(a.y, l)));
}

__device__ __forceinline__ double ctc_lse3(double a, double b, double c)
{
    const double m = fmax(fmax(a, b), c);
    if (m == -INFINITY) return -INFINITY;
    return m + log(exp(a - m) + exp(b - m) + exp(c - m));
}

__global__ __launch_bounds__(64) void ctc_alpha_kernel(const float* __restrict__ probs, const CtcWin* __restrict__ wins,
                                                       const uint8_t* __restrict__ labels, double* __restrict__ loss)
{
    __shared__ double fin[2];
    const int lane = threadIdx.x;
    const CtcWin W = wins[blockIdx.x];
    const int n = W.n, L = W.L, S = 2 * L + 1;
    const int nk = (S + 63) / 64;
    const float* __restrict__ y = probs + (int64_t)blockIdx.x * CTC_T * RD_NCLS;
    const uint8_t* __restrict__ lab = labels + W.lab;
    // per state: its class, and whether alpha(s - 2) feeds it (a label state whose label differs from the one before)
    int cls[CTC_KS];
    bool skip[CTC_KS];
    double a[CTC_KS];
#pragma unroll
    for (int k = 0; k < CTC_KS; k++) {
        const int s = lane + 64 * k;
        const bool lbl = (s & 1) && s < S;
        const int c = lbl ? lab[s >> 1] : 4;
        cls[k] = c;
        skip[k] = lbl && s >= 3 && lab[(s >> 1) - 1] != c;
        a[k] = s == 0 ? 0.0 : -INFINITY;   // alpha before row 0: the empty prefix
    }
    for (int t0 = 0; t0 < n; t0 += 64) {
        // log p of row t0 + lane, fp64
        double lp0 = 0.0, lp1 = 0.0, lp2 = 0.0, lp3 = 0.0, lp4 = 0.0;
        if (t0 + lane < n) {
            const float* r = y + (int64_t)(t0 + lane) * RD_NCLS;
            const double q0 = (double)r[0] + CTC_EPS, q1 = (double)r[1] + CTC_EPS, q2 = (double)r[2] + CTC_EPS, q3 = (double)r[3] + CTC_EPS,
                         q4 = (double)r[4] + CTC_EPS;
            const double ls = log(q0 + q1 + q2 + q3 + q4);
            lp0 = log(q0) - ls;
            lp1 = log(q1) - ls;
            lp2 = log(q2) - ls;
            lp3 = log(q3) - ls;
            lp4 = log(q4) - ls;
        }
        const int steps = min(64, n - t0);
        for (int u = 0; u < steps; u++) {
            const double b0 = ctc_readlane(lp0, u), b1 = ctc_readlane(lp1, u), b2 = ctc_readlane(lp2, u), b3 = ctc_readlane(lp3, u),
                         b4 = ctc_readlane(lp4, u);
            // blocks from the top down: block k's edges read block k - 1's values of the previous row
#pragma unroll
            for (int k = CTC_KS - 1; k >= 0; k--) {
                if (k >= nk) continue;
                const double e1 = k ? ctc_readlane(a[k - 1], 63) : -INFINITY;
                const double e2 = k ? ctc_readlane(a[k - 1], 62) : -INFINITY;
                const double p1 = ctc_shr1d(a[k], e1);
                const double p2 = ctc_shr1d(p1, e2);
                const int c = cls[k];
                const double lp = c == 0 ? b0 : c == 1 ? b1 : c == 2 ? b2 : c == 3 ? b3 : b4;
                a[k] = ctc_lse3(a[k], p1, skip[k] ? p2 : -INFINITY) + lp;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < CTC_KS; k++) {
        const int s = lane + 64 * k;
        if (s == S - 1) fin[0] = a[k];
        if (s == S - 2) fin[1] = a[k];
    }
    __syncthreads();
    if (lane == 0) {
        const double x = fin[0], z = L ? fin[1] : -INFINITY;
        const double m = fmax(x, z);
        loss[blockIdx.x] = m == -INFINITY ? INFINITY : -(m + log(exp(x - m) + exp(z - m)));
    }
}

__device__ __forceinline__ int ed_shfl_up(int v, int d) { return __shfl_up(v, (unsigned)d, 64); }

__global__ __launch_bounds__(64) void ctc_greedy_ed_kernel(const float* __restrict__ probs, const CtcWin* __restrict__ wins,
                                                           const uint8_t* __restrict__ labels, int32_t* __restrict__ out,
                                                           uint8_t* __restrict__ greedy_out)
{
    __shared__ uint8_t g[CTC_T];
    const int lane = threadIdx.x;
    const CtcWin W = wins[blockIdx.x];
    const int n = W.n, L = W.L;
    const float* __restrict__ y = probs + (int64_t)blockIdx.x * CTC_T * RD_NCLS;
    const uint8_t* __restrict__ lab = labels + W.lab;
    // greedy labels
    int G = 0, last = 4;   // last: the class of the row before this pass (row -1: blank, so row 0 is kept unless blank)
    for (int t0 = 0; t0 < n; t0 += 64) {
        const int t = t0 + lane;
        int c = 4;
        if (t < n) {
            const float* r = y + (int64_t)t * RD_NCLS;
            float best = r[0];
            c = 0;
#pragma unroll
            for (int k = 1; k < RD_NCLS; k++)
                if (r[k] > best) {
                    best = r[k];
                    c = k;
                }
        }
        const int prev = ctc_shr1(c, last);
        const bool keep = t < n && c != 4 && c != prev;
        const uint64_t mask = __ballot(keep);
        const int pos = G + __popcll(mask & ((1ull << lane) - 1));
        if (keep) g[pos] = (uint8_t)c;
        G += __popcll(mask);
        last = __builtin_amdgcn_readlane(c, 63);
    }
    __syncthreads();
    if (greedy_out)
        for (int i = lane; i < G; i += 64) greedy_out[(int64_t)blockIdx.x * CTC_T + i] = g[i];
    // Levenshtein distance between g[0..G) (rows) and lab[0..L) (columns 0..L)
    const int nc = (L + 1 + 63) / 64;
    int d[ED_KC], lj[ED_KC];
#pragma unroll
    for (int c = 0; c < ED_KC; c++) {
        const int j = lane + 64 * c;
        d[c] = j;   // row 0
        lj[c] = (j >= 1 && j <= L) ? lab[j - 1] : 0xff;
    }
    for (int i = 1; i <= G; i++) {
        const int gi = g[i - 1];
        int carry = i;   // min over the columns of the blocks before of (D[i][k] - k), seeded with T[0] - 0 = i
        int up_edge = i - 1;   // D[i-1][j-1] for lane 0 of block 0: D[i-1][-1] does not exist, column 0 takes T[0] = i below
#pragma unroll
        for (int c = 0; c < ED_KC; c++) {
            if (c >= nc) continue;
            const int j = lane + 64 * c;
            const int diag = ctc_shr1(d[c], up_edge);   // D[i-1][j-1]
            up_edge = __builtin_amdgcn_readlane(d[c], 63);
            int T = j == 0 ? i : min(d[c] + 1, diag + (gi != lj[c]));
            int u = T - j;
#pragma unroll
            for (int s = 1; s < 64; s <<= 1) {
                const int o = ed_shfl_up(u, s);
                if (lane >= s) u = min(u, o);
            }
            u = min(u, carry);
            d[c] = u + j;
            carry = __builtin_amdgcn_readlane(u, 63);
        }
    }
    int ed = 0;
#pragma unroll
    for (int c = 0; c < ED_KC; c++)
        if (c == L / 64) ed = __builtin_amdgcn_readlane(d[c], L & 63);
    if (lane == 0) {
        out[2 * (int64_t)blockIdx.x] = G;
        out[2 * (int64_t)blockIdx.x + 1] = ed;
    }
}

// L + adjacent equal labels > n: no path of n rows collapses to the label
bool ctc_infeasible(const uint8_t* l, int L, int n)
{
    int need = L;
    for (int k = 1; k < L; k++) need += l[k] == l[k - 1];
    return need > n;
}

// The windows' metadata, checked on the host before anything is uploaded or launched.
int ctc_check(const char* fn, int n, const int32_t* input_len, const uint8_t* labels, const int64_t* label_off, const int32_t* label_len)
{
    for (int i = 0; i < n; i++) {
        RD_REQUIRE(input_len[i] >= 1 && input_len[i] <= CTC_T, "%s: window %d has input_length %d, outside 1..%d", fn, i, input_len[i], CTC_T);
        RD_REQUIRE(label_len[i] >= 0 && label_len[i] <= CTC_MAXL, "%s: window %d has label_length %d, outside 0..%d", fn, i, label_len[i], CTC_MAXL);
        RD_REQUIRE(label_len[i] == 0 || label_off[i] >= 0, "%s: window %d has a negative label offset", fn, i);
        for (int k = 0; k < label_len[i]; k++)
            RD_REQUIRE(labels[label_off[i] + k] <= 3, "%s: window %d label %d is %d, not 0..3", fn, i, k, labels[label_off[i] + k]);
    }
    return RD_OK;
}

// ws_ctc: window descriptors | labels | loss [n] f64 | greedy_len + distance [n][2] i32 | greedy labels [n][1024] u8
struct CtcWs {
    CtcWin* win;
    uint8_t* lab;
    double* loss;
    int32_t* ed;
    uint8_t* greedy;
};
void ctc_layout(Carve& c, int n, int64_t nl, bool greedy, CtcWs* W)
{
    W->win = c.take<CtcWin>((size_t)n);
    W->lab = c.take<uint8_t>((size_t)nl + 1);
    W->loss = c.take<double>((size_t)n);
    W->ed = c.take<int32_t>((size_t)n * 2);
    W->greedy = c.take<uint8_t>(greedy ? (size_t)n * CTC_T : 0, 0, 1);
}

// Stages the (checked) metadata into the context's CTC workspace and runs both kernels on d_probs.
int ctc_run(rd_ctx* ctx, const float* d_probs, int n, const int32_t* input_len, const uint8_t* labels, const int64_t* label_off,
            const int32_t* label_len, double* loss, int32_t* status, int32_t* greedy_len, int32_t* edit_distance, uint8_t* greedy_out)
{
    int64_t nl = 0;
    for (int i = 0; i < n; i++) nl += label_len[i];
    if (n == 0) return RD_OK;
    CtcWs W;
    if (rd_carve(ctx->ws_ctc, [&](Carve& c) { ctc_layout(c, n, nl, greedy_out != nullptr, &W); })) return RD_ERR_NOMEM;
    const size_t a_win = (size_t)((uint8_t*)W.lab - (uint8_t*)W.win), a_g = greedy_out ? (size_t)n * CTC_T : 0;
    std::vector<uint8_t> stage((size_t)((uint8_t*)W.loss - (uint8_t*)W.win));   // descriptors and labels go up in one copy
    CtcWin* w = (CtcWin*)stage.data();
    int64_t at = 0;
    for (int i = 0; i < n; i++) {
        w[i] = CtcWin{at, input_len[i], label_len[i]};
        if (label_len[i]) memcpy(stage.data() + a_win + at, labels + label_off[i], (size_t)label_len[i]);
        at += label_len[i];
    }
    uint8_t* d_g = greedy_out ? W.greedy : nullptr;
    RD_HIP(hipMemcpyAsync(W.win, stage.data(), stage.size(), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(ctc_alpha_kernel, dim3(n), dim3(64), 0, ctx->stream, d_probs, W.win, W.lab, W.loss);
    RD_HIP(hipGetLastError());
    hipLaunchKernelGGL(ctc_greedy_ed_kernel, dim3(n), dim3(64), 0, ctx->stream, d_probs, W.win, W.lab, W.ed, d_g);
    RD_HIP(hipGetLastError());
    std::vector<int32_t> ed((size_t)n * 2);
    RD_HIP(hipMemcpyAsync(loss, W.loss, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
    RD_HIP(hipMemcpyAsync(ed.data(), W.ed, ed.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (greedy_out) RD_HIP(hipMemcpyAsync(greedy_out, d_g, a_g, hipMemcpyDeviceToHost, ctx->stream));
    RD_HIP(hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < n; i++) {
        status[i] = ctc_infeasible(labels + (label_len[i] ? label_off[i] : 0), label_len[i], input_len[i]) ? RD_CTC_INFEASIBLE : RD_CTC_OK;
        greedy_len[i] = ed[2 * (size_t)i];
        edit_distance[i] = ed[2 * (size_t)i + 1];
    }
    return RD_OK;
}

#define CTC_REQUIRE_ARGS(fn)                                                                                                      \
    RD_REQUIRE(ctx && n_windows >= 0, fn ": null context or negative window count");                                             \
    RD_REQUIRE(n_windows == 0 || (input_len && labels && label_off && label_len && loss && status && greedy_len && edit_distance), \
               fn ": null argument")

}  // namespace

extern "C" int rd_ctc_probs(rd_ctx* ctx, const float* probs, int n_windows, const int32_t* input_len, const uint8_t* labels,
                            const int64_t* label_off, const int32_t* label_len, double* loss, int32_t* status, int32_t* greedy_len,
                            int32_t* edit_distance, uint8_t* greedy_out)
{
    CTC_REQUIRE_ARGS("rd_ctc_probs");
    RD_REQUIRE(n_windows == 0 || probs, "rd_ctc_probs: null probs");
    RD_HIP(hipSetDevice(ctx->device));
    if (int rc = ctc_check("rd_ctc_probs", n_windows, input_len, labels, label_off, label_len)) return rc;
    const size_t bytes = (size_t)n_windows * CTC_T * RD_NCLS * 4;
    if (n_windows && ctx->ws_probs.reserve(bytes)) return RD_ERR_NOMEM;
    if (n_windows) RD_HIP(hipMemcpyAsync(ctx->ws_probs.p, probs, bytes, hipMemcpyHostToDevice, ctx->stream));
    return ctc_run(ctx, ctx->ws_probs.as<float>(), n_windows, input_len, labels, label_off, label_len, loss, status, greedy_len,
                   edit_distance, greedy_out);
}

extern "C" int rd_ctc_probs_resident(rd_ctx* ctx, const float* d_probs, int n_windows, const int32_t* input_len, const uint8_t* labels,
                                     const int64_t* label_off, const int32_t* label_len, double* loss, int32_t* status, int32_t* greedy_len,
                                     int32_t* edit_distance, uint8_t* greedy_out)
{
    CTC_REQUIRE_ARGS("rd_ctc_probs_resident");
    RD_REQUIRE(n_windows == 0 || d_probs, "rd_ctc_probs_resident: null d_probs");
    if (int rc = ctc_check("rd_ctc_probs_resident", n_windows, input_len, labels, label_off, label_len)) return rc;
    RD_HIP(hipSetDevice(ctx->device));
    return ctc_run(ctx, d_probs, n_windows, input_len, labels, label_off, label_len, loss, status, greedy_len, edit_distance, greedy_out);
}

extern "C" int rd_ctc_eval(rd_ctx* ctx, const float* windows, int n_windows, const int32_t* input_len, const uint8_t* labels,
                           const int64_t* label_off, const int32_t* label_len, double* loss, int32_t* status, int32_t* greedy_len,
                           int32_t* edit_distance, uint8_t* greedy_out)
{
    CTC_REQUIRE_ARGS("rd_ctc_eval");
    RD_REQUIRE(n_windows == 0 || windows, "rd_ctc_eval: null windows");
    RD_REQUIRE(ctx->model.loaded, "rd_ctc_eval: no weights loaded (rd_load_weights)");
    if (int rc = ctc_check("rd_ctc_eval", n_windows, input_len, labels, label_off, label_len)) return rc;
    if (n_windows == 0) return RD_OK;
    RD_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)n_windows * CTC_T;
    if (ctx->ws_in.reserve(n * 4) || ctx->ws_probs.reserve(n * 20)) return RD_ERR_NOMEM;
    RD_HIP(hipMemcpyAsync(ctx->ws_in.p, windows, n * 4, hipMemcpyHostToDevice, ctx->stream));
    // the forward sees the whole window (as Keras's does); the loss counts the first input_length rows
    int rc = rd_forward_dev(ctx, ctx->ws_in.as<float>(), n_windows, CTC_T, ctx->ws_probs.as<float>());
    if (rc) return rc;
    return ctc_run(ctx, ctx->ws_probs.as<float>(), n_windows, input_len, labels, label_off, label_len, loss, status, greedy_len,
                   edit_distance, greedy_out);
}
