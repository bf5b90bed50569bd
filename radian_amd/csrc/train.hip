// train.hip -- training of the signal model on labelled windows (radian/train.py + model.py:16-40,91-158) on the MI355X:
// a training forward that keeps what the backward needs, the gradient of Keras's ctc_batch_cost (mean over the batch), the
// gradients of every weight tensor, and TF 2.4's Adam.  Exact fp32 only (rd_set_precision 0).  DESIGN.md section 12.
//
// Rows: a batch of n windows is R = n * 1024 rows, window-major; every activation is [R][channels] fp32.
//   forward   h1 = relu(conv0(x)), h2 = relu(conv1(h1)), out = relu(h2 + res) per block (res = the 1x1 matching conv of the
//             signal in block 0, the block's input elsewhere); h3 = relu(dense(out)); y = softmax(dense_1(h3)).
//   CTC       log p = log((y + 1e-7) / sum(y + 1e-7)) in fp64; alpha and beta recursions in fp64 (one wave each per window, both
//             in one launch so that the two serial chains overlap); posterior gamma_k(t) = sum over states of class k of
//             exp(alpha + beta - log P); dL/dz through Keras's chain: dL/du = p - gamma, dL/dy = (p - gamma)/(y + eps),
//             dL/dz_j = y_j (dL/dy_j - sum_k y_k dL/dy_k); divided by n (the batch mean); zero beyond input_length and for
//             windows without a CTC path.
//   backward  one fp32 MFMA GEMM kernel (v_mfma_f32_32x32x2_f32, 128 x 128 tiles, K steps of 16) in three forms:
//               FWD  out[r][n] = sum_{j,c} act[r - (taps-1-j) d][c] W[j][c][n]       (causal conv / dense; epilogue: bias, ReLU, residual)
//               DX   out[r][n] = sum_{j,c} g[r + (taps-1-j) d][c] W[j][n][c]         (the transposed conv: anti-causal, weights transposed)
//               DW   part[s][(j,c)][n] = sum_{r in split s} act[r - (taps-1-j) d][c] g[r][n]   (split over rows)
//             shifted rows that leave their window read zeros.  Small reductions (biases, block 0's one-channel convs, the last
//             Dense) run on the vector ALU over fixed chunks of rows.  Every reduction writes fixed-order partials that one pass
//             sums in fp64: no float atomics, two identical steps give identical bits.
//   Adam      TF 2.4 ApplyAdam on the flat fp32 master weights (load_weights order), then the fp32 LDS images of the inference
//             kernels are rewritten on the device; the f16x3 / bf16x3 images are rebuilt on the host when next needed.
#include "common.h"
#include "model_params.h"
#include "../../include/radian_hip.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace {

constexpr int TT = RD_CTC_T;               // rows per window
constexpr int MAXL = RD_CTC_MAX_LABEL;
constexpr double EPS = 1e-7;               // Keras backend epsilon()

// ------------------------------------------------------------------------------------------------ fp32 image <-> flat weights
// kind 0: raw copy; 1: conv kernel [j][ci][co] <-> [chunk = (ci/16)*3 + j][co][swizzled ci%16]; 2: dense kernel [ci][h] <-> [ci/16][h][swz]
// (the index functions of model.hip's pack_conv / pack_dense, model_params.h: an image written here equals rd_load_weights' bit for bit)
struct PackSeg {
    int64_t src;
    float* dst;
    int32_t n, kind;
};
constexpr int MAX_SEGS = 6 * RD_MAX_BLOCKS + 8;
struct PackTable {
    PackSeg s[MAX_SEGS];
};

__global__ __launch_bounds__(256) void pack_kernel(float* __restrict__ flat, PackTable tb, int to_flat)
{
    const PackSeg sg = tb.s[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= sg.n) return;
    int64_t d = i;
    if (sg.kind == 1) {
        const int j = i / (RD_C * RD_C), ci = (i / RD_C) % RD_C, co = i % RD_C;
        d = (int64_t)rd_conv_image_row(j, ci, co) * 16 + rd_swz_f32(co, ci % 16);
    } else if (sg.kind == 2) {
        const int ci = i / RD_H, h = i % RD_H;
        d = (int64_t)rd_dense_image_row(ci, h) * 16 + rd_swz_f32(h, ci % 16);
    }
    if (to_flat) flat[sg.src + i] = sg.dst[d];
    else sg.dst[d] = flat[sg.src + i];
}

// ------------------------------------------------------------------------------------------------ forward pieces
// block 0's first conv (one input channel): h[r][co] = relu(b[co] + sum_j w[j][co] x[r - (2-j) d])
__global__ __launch_bounds__(256) void conv_in_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                      int d, float* __restrict__ h)
{
    const int64_t r = blockIdx.x;
    const int co = threadIdx.x, t = (int)(r % TT);
    float acc = b[co];
#pragma unroll
    for (int j = 0; j < RD_K; j++) {
        const int s = (RD_K - 1 - j) * d;
        if (t >= s) acc = fmaf(x[r - s], w[j * RD_C + co], acc);
    }
    h[r * RD_C + co] = fmaxf(acc, 0.f);
}

// y[r] = softmax(b2 + h3[r] W2), one thread per row
__global__ __launch_bounds__(256) void head_fwd_kernel(const float* __restrict__ h3, const float* __restrict__ w2, const float* __restrict__ b2,
                                                       float* __restrict__ y, int64_t R)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    float z[RD_NCLS];
#pragma unroll
    for (int k = 0; k < RD_NCLS; k++) z[k] = b2[k];
    const float4* hr = (const float4*)(h3 + r * RD_H);
    for (int q = 0; q < RD_H / 4; q++) {
        const float4 v = hr[q];
        const float hv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; e++)
#pragma unroll
            for (int k = 0; k < RD_NCLS; k++) z[k] = fmaf(hv[e], w2[(4 * q + e) * RD_NCLS + k], z[k]);
    }
    float m = z[0];
#pragma unroll
    for (int k = 1; k < RD_NCLS; k++) m = fmaxf(m, z[k]);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < RD_NCLS; k++) {
        z[k] = expf(z[k] - m);
        s += z[k];
    }
#pragma unroll
    for (int k = 0; k < RD_NCLS; k++) y[r * RD_NCLS + k] = z[k] / s;
}

// g_a3[r][h] = (sum_k g_z[r][k] W2[h][k]) [h3 > 0]
__global__ __launch_bounds__(256) void head_bwd_kernel(const float* __restrict__ gz, const float* __restrict__ w2, const float* __restrict__ h3,
                                                       float* __restrict__ ga3, int64_t R)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= R * RD_H) return;
    const int64_t r = i / RD_H;
    const int h = (int)(i % RD_H);
    float g = 0.f;
#pragma unroll
    for (int k = 0; k < RD_NCLS; k++) g = fmaf(gz[r * RD_NCLS + k], w2[h * RD_NCLS + k], g);
    ga3[i] = h3[i] > 0.f ? g : 0.f;
}

// ------------------------------------------------------------------------------------------------ the GEMM
enum { G_FWD = 0, G_DX = 1, G_DW = 2 };
enum { E_RELU = 0, E_RELU_ID = 1, E_RELU_MATCH = 2, E_MASK = 3, E_RES = 4, E_PART = 5 };

struct GemmP {
    const float* a;    // FWD / DX / DW: activations or gradients [rows][lda]
    const float* b;    // FWD: W [K][N]; DX: W [taps][N][cw]; DW: g [rows][ldb]
    int lda, ldb;
    int cin;           // channels per tap of the summed index (FWD, DX: K = taps * cin; DW: M = taps * cin)
    int taps, dil;
    int M, N, K;       // DW: K = rows per split (grid z = split)
    float* out;        // FWD / DX: [M][N]; DW: partial [split][M][N]
    float* out2;
    const float* bias;
    const float* aux;  // E_RELU_ID: block input; E_RELU_MATCH: signal; E_MASK: the mask tensor; E_RES: out of the block before
    const float* aux2; // E_RES: h2 of the block before
    const float* aux3; // E_RES: the residual gradient added (nullable)
    const float* res_w;
    const float* res_b;
};

constexpr int GB = 128, GK = 16, GLD = GB + 4;
using f32x16 = __attribute__((ext_vector_type(16))) float;

template <int KIND>
__device__ __forceinline__ void gemm_load(const GemmP& p, int m0, int n0, int64_t k0, float4 (&ra)[2], float4 (&rb)[2])
{
    const int tid = threadIdx.x;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (KIND == G_FWD || KIND == G_DX) {
        const int j = (int)(k0 / p.cin), c0 = (int)(k0 % p.cin);
        const int sh = (p.taps - 1 - j) * p.dil;
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int idx = tid + 256 * i, rr = idx >> 2, q = idx & 3;
            const int64_t m = m0 + rr;
            const int t = (int)(m % TT);
            bool ok;
            int64_t src;
            if (KIND == G_FWD) {
                ok = t >= sh;
                src = m - sh;
            } else {
                ok = t + sh < TT;
                src = m + sh;
            }
            ra[i] = ok ? *(const float4*)(p.a + src * p.lda + c0 + 4 * q) : z4;
            if (KIND == G_FWD) {
                const int kk = idx >> 5, c = (idx & 31) * 4;
                rb[i] = *(const float4*)(p.b + (k0 + kk) * p.N + n0 + c);
            } else {
                const int n = idx >> 2;
                rb[i] = *(const float4*)(p.b + (int64_t)j * p.N * p.cin + (int64_t)(n0 + n) * p.cin + c0 + 4 * q);
            }
        }
    } else {
        const int j = m0 / p.cin, c0 = m0 % p.cin;
        const int sh = (p.taps - 1 - j) * p.dil;
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int idx = tid + 256 * i, kk = idx >> 5, c = (idx & 31) * 4;
            const int64_t row = k0 + kk;
            const int t = (int)(row % TT);
            ra[i] = t >= sh ? *(const float4*)(p.a + (row - sh) * p.lda + c0 + c) : z4;
            rb[i] = *(const float4*)(p.b + row * p.ldb + n0 + c);
        }
    }
}

template <int KIND>
__device__ __forceinline__ void gemm_store(float (*As)[GLD], float (*Bs)[GLD], const float4 (&ra)[2], const float4 (&rb)[2])
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int idx = tid + 256 * i;
        if (KIND == G_DW) {
            const int kk = idx >> 5, c = (idx & 31) * 4;
            *(float4*)&As[kk][c] = ra[i];
            *(float4*)&Bs[kk][c] = rb[i];
        } else {
            const int rr = idx >> 2, q = idx & 3;
            As[4 * q + 0][rr] = ra[i].x;
            As[4 * q + 1][rr] = ra[i].y;
            As[4 * q + 2][rr] = ra[i].z;
            As[4 * q + 3][rr] = ra[i].w;
            if (KIND == G_FWD) {
                const int kk = idx >> 5, c = (idx & 31) * 4;
                *(float4*)&Bs[kk][c] = rb[i];
            } else {
                Bs[4 * q + 0][rr] = rb[i].x;
                Bs[4 * q + 1][rr] = rb[i].y;
                Bs[4 * q + 2][rr] = rb[i].z;
                Bs[4 * q + 3][rr] = rb[i].w;
            }
        }
    }
}

// 256 threads = 4 waves in 2 x 2, each wave 64 x 64 = 2 x 2 MFMA tiles of 32 x 32.  Every tile is full (the host checks
// M, N multiples of 128 and K multiples of 16), so nothing is guarded but the shifted rows.
template <int KIND, int EPI>
__global__ __launch_bounds__(256) void gemm_kernel(GemmP p)
{
    __shared__ float As[GK][GLD];
    __shared__ float Bs[GK][GLD];
    const int m0 = blockIdx.x * GB, n0 = blockIdx.y * GB;
    const int64_t kbase = KIND == G_DW ? (int64_t)blockIdx.z * p.K : 0;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int wm = (w >> 1) * 64, wn = (w & 1) * 64;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;
    float4 ra[2], rb[2];
    const int nk = p.K / GK;
    gemm_load<KIND>(p, m0, n0, kbase, ra, rb);
    gemm_store<KIND>(As, Bs, ra, rb);
    __syncthreads();
    for (int kt = 0; kt < nk; kt++) {
        if (kt + 1 < nk) gemm_load<KIND>(p, m0, n0, kbase + (int64_t)(kt + 1) * GK, ra, rb);
#pragma unroll
        for (int k2 = 0; k2 < GK / 2; k2++) {
            const int k = 2 * k2 + (lane >> 5);
            const float a0 = As[k][wm + (lane & 31)], a1 = As[k][wm + 32 + (lane & 31)];
            const float b0 = Bs[k][wn + (lane & 31)], b1 = Bs[k][wn + 32 + (lane & 31)];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
        if (kt + 1 < nk) {
            gemm_store<KIND>(As, Bs, ra, rb);
            __syncthreads();
        }
    }
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int64_t m = m0 + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                const int n = n0 + wn + 32 * j + (lane & 31);
                const int64_t o = m * p.N + n;
                const float v = acc[i][j][r];
                if (EPI == E_PART) {
                    p.out[(int64_t)blockIdx.z * p.M * p.N + o] = v;
                } else if (EPI == E_MASK) {
                    p.out[o] = p.aux[o] > 0.f ? v : 0.f;
                } else if (EPI == E_RES) {
                    const float g = p.aux3 ? v + p.aux3[o] : v;
                    const float gs = p.aux[o] > 0.f ? g : 0.f;
                    p.out[o] = gs;
                    p.out2[o] = p.aux2[o] > 0.f ? gs : 0.f;
                } else {
                    const float h = fmaxf(v + p.bias[n], 0.f);
                    p.out[o] = h;
                    if (EPI == E_RELU_ID) p.out2[o] = fmaxf(h + p.aux[o], 0.f);
                    if (EPI == E_RELU_MATCH) p.out2[o] = fmaxf(h + (p.aux[m] * p.res_w[n] + p.res_b[n]), 0.f);
                }
            }
}

// ------------------------------------------------------------------------------------------------ small reductions over rows
// part[chunk][m][n] = sum over the chunk's rows r of A(r, m) b[r][n]; A: mode 0 ones (M = 1), 1 columns of a [r][lda],
// 2 the signal shifted by tap m: a[r - (M-1-m) d] (zero before the window).  One thread per n (N <= 256), M <= 5.
constexpr int RS_ROWS = 256;
__global__ __launch_bounds__(256) void rowsum_kernel(const float* __restrict__ a, int lda, int amode, int M, int d, const float* __restrict__ b,
                                                     int ldb, int N, float* __restrict__ part)
{
    const int n = threadIdx.x;
    if (n >= N) return;
    const int64_t r0 = (int64_t)blockIdx.x * RS_ROWS;
    float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < RS_ROWS; k++) {
        const int64_t r = r0 + k;
        const float bv = b[r * ldb + n];
        const int t = (int)(r % TT);
#pragma unroll
        for (int m = 0; m < 5; m++) {
            if (m >= M) break;
            float av;
            if (amode == 0) av = 1.f;
            else if (amode == 1) av = a[r * lda + m];
            else {
                const int s = (M - 1 - m) * d;
                av = t >= s ? a[r - s] : 0.f;
            }
            acc[m] = fmaf(av, bv, acc[m]);
        }
    }
    for (int m = 0; m < M; m++) part[((int64_t)blockIdx.x * M + m) * N + n] = acc[m];
}

// out[m][n] (or out[n][m] when trans) = sum over splits, in split order, in fp64
__global__ __launch_bounds__(256) void reduce_kernel(const float* __restrict__ part, int nsplit, int M, int N, int trans, float* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t MN = (int64_t)M * N;
    if (i >= MN) return;
    double s = 0.0;
    for (int k = 0; k < nsplit; k++) s += (double)part[k * MN + i];
    const int m = (int)(i / N), n = (int)(i % N);
    out[trans ? (int64_t)n * M + m : i] = (float)s;
}

// ------------------------------------------------------------------------------------------------ CTC gradient
struct TWin {
    int64_t lab;    // offset of the labels
    int64_t ab;     // offset of the window's alpha / beta rows ([n][S] doubles each)
    int32_t n, L, infeasible, pad_;
};

// lp[r][k] = log((y + eps) / sum(y + eps)), fp64, rows t < input_length
__global__ __launch_bounds__(256) void ctc_logp_kernel(const float* __restrict__ y, const TWin* __restrict__ wins, double* __restrict__ lp, int64_t R)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    if ((int)(r % TT) >= wins[r / TT].n) return;
    double q[RD_NCLS], s = 0.0;
#pragma unroll
    for (int k = 0; k < RD_NCLS; k++) {
        q[k] = (double)y[r * RD_NCLS + k] + EPS;
        s += q[k];
    }
    const double ls = log(s);
#pragma unroll
    for (int k = 0; k < RD_NCLS; k++) lp[r * RD_NCLS + k] = log(q[k]) - ls;
}

__device__ __forceinline__ double lse3(double a, double b, double c)
{
    const double m = fmax(fmax(a, b), c);
    if (m == -INFINITY) return -INFINITY;
    return m + log(exp(a - m) + exp(b - m) + exp(c - m));
}

// Workgroups [0, n): alpha of window w; [n, 2n): beta of window w - n.  One wave each; states s = lane + 64 k in LDS, double
// buffered.  alpha_t(s) includes row t's emission; beta_t(s) covers rows t+1 .. n-1 (so alpha + beta - log P is the log
// posterior of state s at row t).  Workgroup w of the alpha half writes log P.
constexpr int CS = 2 * MAXL + 1;   // 511 states at most
__global__ __launch_bounds__(64) void ctc_ab_kernel(const TWin* __restrict__ wins, const uint8_t* __restrict__ labels, const double* __restrict__ lp,
                                                    double* __restrict__ alpha, double* __restrict__ beta, double* __restrict__ logp, int nwin)
{
    __shared__ double buf[2][CS + 4];
    __shared__ uint8_t cls[CS + 4];
    __shared__ uint8_t skp[CS + 4];
    const bool back = (int)blockIdx.x >= nwin;
    const int wi = back ? blockIdx.x - nwin : blockIdx.x;
    const TWin W = wins[wi];
    const int lane = threadIdx.x, n = W.n, L = W.L, S = 2 * L + 1;
    if (W.infeasible) {
        if (!back && lane == 0) logp[wi] = -INFINITY;
        return;
    }
    const uint8_t* lab = labels + W.lab;
    const double* lpw = lp + (int64_t)wi * TT * RD_NCLS;
    for (int s = lane; s < CS + 4; s += 64) {
        const bool lbl = (s & 1) && s < S;
        const int c = lbl ? lab[s >> 1] : 4;
        cls[s] = (uint8_t)c;
        skp[s] = lbl && s >= 3 && lab[(s >> 1) - 1] != c;   // alpha(s - 2) feeds s
        buf[0][s] = -INFINITY;
        buf[1][s] = -INFINITY;
    }
    __syncthreads();
    if (!back) {
        // buffer index s + 2: buf[.][0], buf[.][1] are the -inf states below 0
        double* A = alpha + W.ab;
        int cur = 0;
        for (int t = 0; t < n; t++) {
            const double* l = lpw + (int64_t)t * RD_NCLS;
            for (int s = lane; s < S; s += 64) {
                double v;
                if (t == 0) v = s <= 1 ? l[cls[s]] : -INFINITY;
                else v = lse3(buf[cur][s + 2], buf[cur][s + 1], skp[s] ? buf[cur][s] : -INFINITY) + l[cls[s]];
                buf[cur ^ 1][s + 2] = v;
                A[(int64_t)t * S + s] = v;
            }
            cur ^= 1;
            __syncthreads();
        }
        if (lane == 0) {
            const double x = buf[cur][S - 1 + 2], z = L ? buf[cur][S - 2 + 2] : -INFINITY;
            const double m = fmax(x, z);
            logp[wi] = m == -INFINITY ? -INFINITY : m + log(exp(x - m) + exp(z - m));
        }
    } else {
        // buffer index s; buf[.][S], buf[.][S + 1] stay -inf
        double* B = beta + W.ab;
        int cur = 0;
        for (int t = n - 1; t >= 0; t--) {
            const double* l = lpw + (int64_t)(t + 1) * RD_NCLS;
            for (int s = lane; s < S; s += 64) {
                double v;
                if (t == n - 1) v = (s == S - 1 || s == S - 2) ? 0.0 : -INFINITY;
                else
                    v = lse3(buf[cur][s] + l[cls[s]], buf[cur][s + 1] + (s + 1 < S ? l[cls[s + 1]] : 0.0),
                             (s + 2 < S && skp[s + 2]) ? buf[cur][s + 2] + l[cls[s + 2]] : -INFINITY);
                buf[cur ^ 1][s] = v;
                B[(int64_t)t * S + s] = v;
            }
            cur ^= 1;
            __syncthreads();
        }
    }
}

// g_z[r][j], one thread per row; scale = 1 / n (the batch mean)
__global__ __launch_bounds__(256) void ctc_grad_kernel(const float* __restrict__ y, const TWin* __restrict__ wins, const uint8_t* __restrict__ labels,
                                                       const double* __restrict__ lp, const double* __restrict__ alpha, const double* __restrict__ beta,
                                                       const double* __restrict__ logp, double scale, float* __restrict__ gz, int64_t R)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    const int wi = (int)(r / TT), t = (int)(r % TT);
    const TWin W = wins[wi];
    if (W.infeasible || t >= W.n) {
#pragma unroll
        for (int k = 0; k < RD_NCLS; k++) gz[r * RD_NCLS + k] = 0.f;
        return;
    }
    const int S = 2 * W.L + 1;
    const uint8_t* lab = labels + W.lab;
    const double lP = logp[wi];
    const double* A = alpha + W.ab + (int64_t)t * S;
    const double* B = beta + W.ab + (int64_t)t * S;
    double gam[RD_NCLS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int s = 0; s < S; s++) {
        const double e = exp(A[s] + B[s] - lP);
        if (s & 1) gam[lab[s >> 1]] += e;
        else gam[4] += e;
    }
    double yv[RD_NCLS], dy[RD_NCLS], sy = 0.0;
#pragma unroll
    for (int k = 0; k < RD_NCLS; k++) {
        yv[k] = (double)y[r * RD_NCLS + k];
        const double p = exp(lp[r * RD_NCLS + k]);
        dy[k] = (p - gam[k]) / (yv[k] + EPS);
        sy += yv[k] * dy[k];
    }
#pragma unroll
    for (int k = 0; k < RD_NCLS; k++) gz[r * RD_NCLS + k] = (float)(scale * yv[k] * (dy[k] - sy));
}

// ------------------------------------------------------------------------------------------------ Adam (TF 2.4 ApplyAdam, fp32)
//   m += (g - m) (1 - b1);  v += (g^2 - v) (1 - b2);  w -= m alpha / (sqrt(v) + eps),  alpha = lr sqrt(1 - b2^t) / (1 - b1^t)
// every operation rounded on its own (no contraction), as Eigen's CPU kernel does
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ w, float* __restrict__ m, float* __restrict__ v, const float* __restrict__ g,
                                                   int64_t n, float alpha, float omb1, float omb2, float eps)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float gi = g[i];
    const float mi = __fadd_rn(m[i], __fmul_rn(__fsub_rn(gi, m[i]), omb1));
    const float vi = __fadd_rn(v[i], __fmul_rn(__fsub_rn(__fmul_rn(gi, gi), v[i]), omb2));
    m[i] = mi;
    v[i] = vi;
    w[i] = __fsub_rn(w[i], __fdiv_rn(__fmul_rn(mi, alpha), __fadd_rn(__fsqrt_rn(vi), eps)));
}

// ------------------------------------------------------------------------------------------------ state
struct TrainState {
    int nblocks = 0;
    int dil[RD_MAX_BLOCKS] = {0};
    ParamMap pm = {};
    bool need_init = true;   // the master weights must be read back from the fp32 images (first use, rd_load_weights, a clone)
    int64_t t = 0;           // Adam steps since the moments were last zeroed
    DevBuf master, mom_m, mom_v, grad;
    DevBuf acts, gbuf, part, ctc;
};

TrainState* state_of(rd_ctx* ctx) { return (TrainState*)ctx->train; }

PackTable pack_table(const Model& m, const ParamMap& pm, int* nseg)
{
    PackTable tb = {};
    int k = 0;
    auto add = [&](size_t src, float* dst, int n, int kind) { tb.s[k++] = PackSeg{(int64_t)src, dst, n, kind}; };
    for (int b = 0; b < m.nblocks; b++) {
        if (b == 0) {
            add(pm.w0[0], m.w_in, RD_K * RD_C, 0);
            add(pm.b0[0], m.b_in, RD_C, 0);
        } else {
            add(pm.w0[b], m.w_conv[2 * b], (int)RD_CONV_N, 1);
            add(pm.b0[b], m.b_conv[2 * b], RD_C, 0);
        }
        add(pm.w1[b], m.w_conv[2 * b + 1], (int)RD_CONV_N, 1);
        add(pm.b1[b], m.b_conv[2 * b + 1], RD_C, 0);
    }
    add(pm.wm, m.w_match, RD_C, 0);
    add(pm.bm, m.b_match, RD_C, 0);
    add(pm.wd1, m.w_d1, RD_C * RD_H, 2);
    add(pm.bd1, m.b_d1, RD_H, 0);
    add(pm.wd2, m.w_d2, RD_H * RD_NCLS, 0);
    add(pm.bd2, m.b_d2, RD_NCLS, 0);
    *nseg = k;
    return tb;
}

int run_pack(rd_ctx* ctx, TrainState* st, int to_flat)
{
    int nseg = 0;
    PackTable tb = pack_table(ctx->model, st->pm, &nseg);
    hipLaunchKernelGGL(pack_kernel, dim3((unsigned)((RD_CONV_N + 255) / 256), nseg), dim3(256), 0, ctx->stream, st->master.as<float>(), tb, to_flat);
    RD_HIP(hipGetLastError());
    return RD_OK;
}

// the state exists, its master / moments / gradient are sized for the loaded model, and the master holds the model's weights
int state_ready(rd_ctx* ctx)
{
    Model& m = ctx->model;
    TrainState* st = state_of(ctx);
    if (!st) {
        st = new TrainState();
        ctx->train = st;
    }
    bool same = st->nblocks == m.nblocks;
    for (int b = 0; b < m.nblocks && same; b++) same = st->dil[b] == m.dil[b];
    if (!same) {
        st->nblocks = m.nblocks;
        for (int b = 0; b < RD_MAX_BLOCKS; b++) st->dil[b] = m.dil[b];
        st->pm = param_map(m.nblocks);
        st->need_init = true;
    }
    if (st->need_init) {
        const size_t bytes = st->pm.total * sizeof(float);
        if (st->master.reserve(bytes) || st->mom_m.reserve(bytes) || st->mom_v.reserve(bytes) || st->grad.reserve(bytes)) return RD_ERR_NOMEM;
        if (int rc = run_pack(ctx, st, 1)) return rc;
        RD_HIP(hipMemsetAsync(st->mom_m.p, 0, bytes, ctx->stream));
        RD_HIP(hipMemsetAsync(st->mom_v.p, 0, bytes, ctx->stream));
        st->t = 0;
        st->need_init = false;
    }
    return RD_OK;
}

int check_windows(const char* fn, int n, const int32_t* input_len, const uint8_t* labels, const int64_t* label_off, const int32_t* label_len)
{
    for (int i = 0; i < n; i++) {
        RD_REQUIRE(input_len[i] >= 1 && input_len[i] <= TT, "%s: window %d has input_length %d, outside 1..%d", fn, i, input_len[i], TT);
        RD_REQUIRE(label_len[i] >= 0 && label_len[i] <= MAXL, "%s: window %d has label_length %d, outside 0..%d", fn, i, label_len[i], MAXL);
        RD_REQUIRE(label_len[i] == 0 || label_off[i] >= 0, "%s: window %d has a negative label offset", fn, i);
        for (int k = 0; k < label_len[i]; k++)
            RD_REQUIRE(labels[label_off[i] + k] <= 3, "%s: window %d label %d is %d, not 0..3", fn, i, k, labels[label_off[i] + k]);
    }
    return RD_OK;
}

bool infeasible(const uint8_t* l, int L, int n)
{
    int need = L;
    for (int k = 1; k < L; k++) need += l[k] == l[k - 1];
    return need > n;
}

// The CTC part of a training call, on device rows y [n][1024][5]: window descriptors | labels | log p [R][5] | alpha | beta | log P [n]
// in `buf`; statuses computed on the host.
struct CtcDev {
    const TWin* win;
    const uint8_t* lab;
    double *lp, *alpha, *beta, *logP;
};

int ctc_stage(DevBuf& buf, hipStream_t s, int n, const int32_t* input_len, const uint8_t* labels, const int64_t* label_off,
              const int32_t* label_len, int32_t* status, CtcDev* cd)
{
    const int64_t R = (int64_t)n * TT;
    std::vector<TWin> tw(n);
    int64_t nl = 0, ab = 0;
    for (int i = 0; i < n; i++) {
        const uint8_t* li = labels + (label_len[i] ? label_off[i] : 0);
        status[i] = infeasible(li, label_len[i], input_len[i]) ? RD_CTC_INFEASIBLE : RD_CTC_OK;
        tw[i] = TWin{nl, ab, input_len[i], label_len[i], status[i], 0};
        nl += label_len[i];
        if (!status[i]) ab += (int64_t)input_len[i] * (2 * label_len[i] + 1);
    }
    const size_t c_win = align_up((size_t)n * sizeof(TWin), 256), c_lab = align_up((size_t)nl + 1, 256), c_lp = (size_t)R * RD_NCLS * 8,
                 c_ab = align_up((size_t)ab * 8, 256), c_lP = align_up((size_t)n * 8, 256);
    if (buf.reserve(c_win + c_lab + c_lp + 2 * c_ab + c_lP)) return RD_ERR_NOMEM;
    std::vector<uint8_t> stage(c_win + c_lab, 0);
    memcpy(stage.data(), tw.data(), n * sizeof(TWin));
    int64_t at = 0;
    for (int i = 0; i < n; i++) {
        if (label_len[i]) memcpy(stage.data() + c_win + at, labels + label_off[i], (size_t)label_len[i]);
        at += label_len[i];
    }
    RD_HIP(hipMemcpyAsync(buf.p, stage.data(), stage.size(), hipMemcpyHostToDevice, s));
    RD_HIP(hipStreamSynchronize(s));   // the staging vector leaves scope
    uint8_t* cw = buf.as<uint8_t>();
    cd->win = (const TWin*)cw;
    cd->lab = cw + c_win;
    cd->lp = (double*)(cw + c_win + c_lab);
    cd->alpha = (double*)(cw + c_win + c_lab + c_lp);
    cd->beta = (double*)(cw + c_win + c_lab + c_lp + c_ab);
    cd->logP = (double*)(cw + c_win + c_lab + c_lp + 2 * c_ab);
    return RD_OK;
}

// log p, alpha and beta side by side, posterior -> dL/dz of the batch mean (gz [R][5])
int ctc_launch(hipStream_t s, const CtcDev& cd, const float* y, int n, float* gz)
{
    const int64_t R = (int64_t)n * TT;
    const unsigned Rb = (unsigned)((R + 255) / 256);
    hipLaunchKernelGGL(ctc_logp_kernel, dim3(Rb), dim3(256), 0, s, y, cd.win, cd.lp, R);
    RD_HIP(hipGetLastError());
    hipLaunchKernelGGL(ctc_ab_kernel, dim3(2 * n), dim3(64), 0, s, cd.win, cd.lab, cd.lp, cd.alpha, cd.beta, cd.logP, n);
    RD_HIP(hipGetLastError());
    hipLaunchKernelGGL(ctc_grad_kernel, dim3(Rb), dim3(256), 0, s, y, cd.win, cd.lab, cd.lp, cd.alpha, cd.beta, cd.logP, 1.0 / n, gz, R);
    RD_HIP(hipGetLastError());
    return RD_OK;
}

// per-window losses (synchronises the stream: every copy queued before returns too)
int ctc_finish(hipStream_t s, const CtcDev& cd, int n, const int32_t* status, double* loss)
{
    std::vector<double> lP(n);
    RD_HIP(hipMemcpyAsync(lP.data(), cd.logP, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    RD_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < n; i++) loss[i] = status[i] ? INFINITY : -lP[i];
    return RD_OK;
}

// The kernel guards nothing but the shifted rows, so every shape is checked here: whole 128 x 128 tiles, whole K steps of 16 that
// stay inside one tap, and (weight gradient) 128-row tiles of M inside one tap.  The graph's shapes always fit (rows = n * 1024,
// 256 channels, 128 relu units, rows per split 256 or 16 n); a future shape that does not is refused instead of read out of bounds.
template <int KIND, int EPI>
int gemm(hipStream_t s, const GemmP& p, int splits = 1)
{
    RD_REQUIRE(p.M > 0 && p.N > 0 && p.K > 0 && splits >= 1 && p.M % GB == 0 && p.N % GB == 0 && p.K % GK == 0 && p.cin % GK == 0 &&
                   p.taps >= 1 && p.lda % 4 == 0 && (KIND == G_DW ? p.M == p.taps * p.cin && p.cin % GB == 0 && p.ldb % 4 == 0 : p.K == p.taps * p.cin),
               "train: GEMM shape M %d N %d K %d (%d taps of %d channels) does not fit the kernel's tiles", p.M, p.N, p.K, p.taps, p.cin);
    hipLaunchKernelGGL((gemm_kernel<KIND, EPI>), dim3(p.M / GB, p.N / GB, splits), dim3(256), 0, s, p);
    RD_HIP(hipGetLastError());
    return RD_OK;
}

// sum of partials [nsplit][M][N] into the gradient at `off`
int reduce(hipStream_t s, const float* part, int nsplit, int M, int N, int trans, float* out)
{
    const int64_t MN = (int64_t)M * N;
    hipLaunchKernelGGL(reduce_kernel, dim3((unsigned)((MN + 255) / 256)), dim3(256), 0, s, part, nsplit, M, N, trans, out);
    RD_HIP(hipGetLastError());
    return RD_OK;
}

int rowsum(hipStream_t s, const float* a, int lda, int amode, int M, int d, const float* b, int ldb, int N, int64_t R, float* part, int trans,
           float* out)
{
    const int nch = (int)(R / RS_ROWS);
    hipLaunchKernelGGL(rowsum_kernel, dim3(nch), dim3(256), 0, s, a, lda, amode, M, d, b, ldb, N, part);
    RD_HIP(hipGetLastError());
    return reduce(s, part, nch, M, N, trans, out);
}

// One training call: forward, CTC gradient, backward into st->grad; then (opt) one Adam update and the image refresh.
int train_run(rd_ctx* ctx, const char* fn, const float* windows, bool resident, int n, const int32_t* input_len, const uint8_t* labels,
              const int64_t* label_off, const int32_t* label_len, const rd_adam* opt, float* grad_out, double* loss, int32_t* status)
{
    RD_REQUIRE(ctx && n >= 1, "%s: null context or no windows", fn);
    RD_REQUIRE(windows && input_len && labels && label_off && label_len && loss && status, "%s: null argument", fn);
    RD_REQUIRE(ctx->model.loaded, "%s: no weights loaded (rd_load_weights)", fn);
    RD_REQUIRE(ctx->precision == 0, "%s: training is exact fp32 only (rd_set_precision 0), the context is set to mode %d", fn, ctx->precision);
    RD_REQUIRE(n <= (INT32_MAX / TT) / RD_C, "%s: %d windows in one call", fn, n);
    if (opt)
        RD_REQUIRE(opt->lr > 0.f && opt->beta1 >= 0.f && opt->beta1 < 1.f && opt->beta2 >= 0.f && opt->beta2 < 1.f && opt->epsilon >= 0.f,
                   "%s: Adam settings lr %g beta1 %g beta2 %g epsilon %g", fn, opt->lr, opt->beta1, opt->beta2, opt->epsilon);
    if (int rc = check_windows(fn, n, input_len, labels, label_off, label_len)) return rc;
    RD_HIP(hipSetDevice(ctx->device));
    if (int rc = rd_sync_lanes(ctx)) return rc;
    if (int rc = state_ready(ctx)) return rc;
    TrainState* st = state_of(ctx);
    const Model& md = ctx->model;
    const ParamMap& pm = st->pm;
    const int nb = md.nblocks;
    hipStream_t s = ctx->stream;
    const int64_t R = (int64_t)n * TT;
    const size_t A = (size_t)R * RD_C;   // floats of one [R][256] tensor

    // ---- workspaces (grow only)
    // acts: x [R] | h1, h2, out per block | h3 [R][128] | y [R][5]
    const size_t a_x = align_up((size_t)R, 64), a_blk = 3 * A, a_h3 = (size_t)R * RD_H, a_y = align_up((size_t)R * RD_NCLS, 64);
    // gbuf: gz [R][5] | ga3 [R][128] | gs x2 | ga2 x2 | ga1
    const size_t g_total = a_y + a_h3 + 5 * A;
    const int dw_split = (int)std::min<int64_t>(64, R / 256);
    const int64_t dw_rows = R / dw_split;
    const size_t p_total = std::max((size_t)dw_split * RD_K * RD_C * RD_C, (size_t)(R / RS_ROWS) * 5 * RD_C);
    if (st->acts.reserve((a_x + nb * a_blk + a_h3 + a_y) * 4) || st->gbuf.reserve(g_total * 4) || st->part.reserve(p_total * 4)) return RD_ERR_NOMEM;
    float* X = st->acts.as<float>();
    auto H1 = [&](int b) { return X + a_x + b * a_blk; };
    auto H2 = [&](int b) { return X + a_x + b * a_blk + A; };
    auto OUT = [&](int b) { return X + a_x + b * a_blk + 2 * A; };
    float* H3 = X + a_x + nb * a_blk;
    float* Y = H3 + a_h3;
    float* GZ = st->gbuf.as<float>();
    float* GA3 = GZ + a_y;
    float* GS[2] = {GA3 + a_h3, GA3 + a_h3 + A};
    float* GA2[2] = {GA3 + a_h3 + 2 * A, GA3 + a_h3 + 3 * A};
    float* GA1 = GA3 + a_h3 + 4 * A;
    float* P = st->part.as<float>();
    const float* Wm = st->master.as<float>();
    float* G = st->grad.as<float>();

    CtcDev cd;
    if (int rc = ctc_stage(st->ctc, s, n, input_len, labels, label_off, label_len, status, &cd)) return rc;

    // ---- forward
    if (resident) RD_HIP(hipMemcpyAsync(X, windows, (size_t)R * 4, hipMemcpyDeviceToDevice, s));
    else RD_HIP(hipMemcpyAsync(X, windows, (size_t)R * 4, hipMemcpyHostToDevice, s));
    const unsigned Rb = (unsigned)((R + 255) / 256);
    for (int b = 0; b < nb; b++) {
        const int d = md.dil[b];
        if (b == 0) {
            hipLaunchKernelGGL(conv_in_kernel, dim3((unsigned)R), dim3(RD_C), 0, s, X, Wm + pm.w0[0], Wm + pm.b0[0], d, H1(0));
            RD_HIP(hipGetLastError());
        } else {
            GemmP p = {};
            p.a = OUT(b - 1), p.lda = RD_C, p.b = Wm + pm.w0[b], p.cin = RD_C, p.taps = RD_K, p.dil = d;
            p.M = (int)R, p.N = RD_C, p.K = RD_K * RD_C, p.out = H1(b), p.bias = Wm + pm.b0[b];
            if (int rc = gemm<G_FWD, E_RELU>(s, p)) return rc;
        }
        GemmP p = {};
        p.a = H1(b), p.lda = RD_C, p.b = Wm + pm.w1[b], p.cin = RD_C, p.taps = RD_K, p.dil = d;
        p.M = (int)R, p.N = RD_C, p.K = RD_K * RD_C, p.out = H2(b), p.out2 = OUT(b), p.bias = Wm + pm.b1[b];
        if (b == 0) {
            p.aux = X, p.res_w = Wm + pm.wm, p.res_b = Wm + pm.bm;
            if (int rc = gemm<G_FWD, E_RELU_MATCH>(s, p)) return rc;
        } else {
            p.aux = OUT(b - 1);
            if (int rc = gemm<G_FWD, E_RELU_ID>(s, p)) return rc;
        }
    }
    {
        GemmP p = {};
        p.a = OUT(nb - 1), p.lda = RD_C, p.b = Wm + pm.wd1, p.cin = RD_C, p.taps = 1, p.dil = 0;
        p.M = (int)R, p.N = RD_H, p.K = RD_C, p.out = H3, p.bias = Wm + pm.bd1;
        if (int rc = gemm<G_FWD, E_RELU>(s, p)) return rc;
    }
    hipLaunchKernelGGL(head_fwd_kernel, dim3(Rb), dim3(256), 0, s, H3, Wm + pm.wd2, Wm + pm.bd2, Y, R);
    RD_HIP(hipGetLastError());

    // ---- CTC: log p, alpha and beta side by side, posterior -> dL/dz
    if (int rc = ctc_launch(s, cd, Y, n, GZ)) return rc;

    // ---- head
    hipLaunchKernelGGL(head_bwd_kernel, dim3((unsigned)((R * RD_H + 255) / 256)), dim3(256), 0, s, GZ, Wm + pm.wd2, H3, GA3, R);
    RD_HIP(hipGetLastError());
    if (int rc = rowsum(s, GZ, RD_NCLS, 1, RD_NCLS, 0, H3, RD_H, RD_H, R, P, 1, G + pm.wd2)) return rc;        // dW2 [h][k]
    if (int rc = rowsum(s, nullptr, 0, 0, 1, 0, GZ, RD_NCLS, RD_NCLS, R, P, 0, G + pm.bd2)) return rc;        // db2
    {
        GemmP p = {};
        p.a = OUT(nb - 1), p.lda = RD_C, p.b = GA3, p.ldb = RD_H, p.cin = RD_C, p.taps = 1, p.dil = 0;
        p.M = RD_C, p.N = RD_H, p.K = (int)dw_rows, p.out = P;
        if (int rc = gemm<G_DW, E_PART>(s, p, dw_split)) return rc;
        if (int rc = reduce(s, P, dw_split, RD_C, RD_H, 0, G + pm.wd1)) return rc;
    }
    if (int rc = rowsum(s, nullptr, 0, 0, 1, 0, GA3, RD_H, RD_H, R, P, 0, G + pm.bd1)) return rc;
    int cur = 0;
    {
        GemmP p = {};
        p.a = GA3, p.lda = RD_H, p.b = Wm + pm.wd1, p.cin = RD_H, p.taps = 1, p.dil = 0;
        p.M = (int)R, p.N = RD_C, p.K = RD_H, p.out = GS[cur], p.out2 = GA2[cur], p.aux = OUT(nb - 1), p.aux2 = H2(nb - 1), p.aux3 = nullptr;
        if (int rc = gemm<G_DX, E_RES>(s, p)) return rc;
    }
    // ---- blocks, last to first
    for (int b = nb - 1; b >= 0; b--) {
        const int d = md.dil[b];
        {   // conv1: dW1, db1, then g_a1 = conv1^T(g_a2) [h1 > 0]
            GemmP p = {};
            p.a = H1(b), p.lda = RD_C, p.b = GA2[cur], p.ldb = RD_C, p.cin = RD_C, p.taps = RD_K, p.dil = d;
            p.M = RD_K * RD_C, p.N = RD_C, p.K = (int)dw_rows, p.out = P;
            if (int rc = gemm<G_DW, E_PART>(s, p, dw_split)) return rc;
            if (int rc = reduce(s, P, dw_split, RD_K * RD_C, RD_C, 0, G + pm.w1[b])) return rc;
            if (int rc = rowsum(s, nullptr, 0, 0, 1, 0, GA2[cur], RD_C, RD_C, R, P, 0, G + pm.b1[b])) return rc;
            GemmP q = {};
            q.a = GA2[cur], q.lda = RD_C, q.b = Wm + pm.w1[b], q.cin = RD_C, q.taps = RD_K, q.dil = d;
            q.M = (int)R, q.N = RD_C, q.K = RD_K * RD_C, q.out = GA1, q.aux = H1(b);
            if (int rc = gemm<G_DX, E_MASK>(s, q)) return rc;
        }
        if (int rc = rowsum(s, nullptr, 0, 0, 1, 0, GA1, RD_C, RD_C, R, P, 0, G + pm.b0[b])) return rc;
        if (b == 0) {
            if (int rc = rowsum(s, X, 1, 2, RD_K, d, GA1, RD_C, RD_C, R, P, 0, G + pm.w0[0])) return rc;          // [3][1][256]
            if (int rc = rowsum(s, X, 1, 1, 1, 0, GS[cur], RD_C, RD_C, R, P, 0, G + pm.wm)) return rc;            // matching conv
            if (int rc = rowsum(s, nullptr, 0, 0, 1, 0, GS[cur], RD_C, RD_C, R, P, 0, G + pm.bm)) return rc;
            break;
        }
        {   // conv0: dW0, then the block input's gradient (+ the identity residual) -> the block before's g_s, g_a2
            GemmP p = {};
            p.a = OUT(b - 1), p.lda = RD_C, p.b = GA1, p.ldb = RD_C, p.cin = RD_C, p.taps = RD_K, p.dil = d;
            p.M = RD_K * RD_C, p.N = RD_C, p.K = (int)dw_rows, p.out = P;
            if (int rc = gemm<G_DW, E_PART>(s, p, dw_split)) return rc;
            if (int rc = reduce(s, P, dw_split, RD_K * RD_C, RD_C, 0, G + pm.w0[b])) return rc;
            GemmP q = {};
            q.a = GA1, q.lda = RD_C, q.b = Wm + pm.w0[b], q.cin = RD_C, q.taps = RD_K, q.dil = d;
            q.M = (int)R, q.N = RD_C, q.K = RD_K * RD_C, q.out = GS[cur ^ 1], q.out2 = GA2[cur ^ 1], q.aux = OUT(b - 1), q.aux2 = H2(b - 1),
            q.aux3 = GS[cur];
            if (int rc = gemm<G_DX, E_RES>(s, q)) return rc;
            cur ^= 1;
        }
    }

    // ---- update
    if (opt) {
        st->t++;
        const float b1p = std::pow(opt->beta1, (float)st->t), b2p = std::pow(opt->beta2, (float)st->t);
        const float alpha = opt->lr * std::sqrt(1.f - b2p) / (1.f - b1p);
        const int64_t np = (int64_t)pm.total;
        hipLaunchKernelGGL(adam_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, s, st->master.as<float>(), st->mom_m.as<float>(),
                           st->mom_v.as<float>(), (const float*)G, np, alpha, 1.f - opt->beta1, 1.f - opt->beta2, opt->epsilon);
        RD_HIP(hipGetLastError());
        if (int rc = run_pack(ctx, st, 0)) return rc;
        ctx->model.split_stale = true;
        ctx->model.pack_ok = false;   // (the host has not seen the updated weights: window heads run unpacked)
    }
    if (grad_out) RD_HIP(hipMemcpyAsync(grad_out, G, pm.total * 4, hipMemcpyDeviceToHost, s));
    return ctc_finish(s, cd, n, status, loss);
}

}  // namespace

// ------------------------------------------------------------------------------------------------ library-internal
void rd_train_invalidate(rd_ctx* ctx)
{
    if (TrainState* st = state_of(ctx)) st->need_init = true;
}

void rd_train_destroy(rd_ctx* ctx)
{
    TrainState* st = state_of(ctx);
    if (!st) return;
    DevBuf* bufs[] = {&st->master, &st->mom_m, &st->mom_v, &st->grad, &st->acts, &st->gbuf, &st->part, &st->ctc};
    for (DevBuf* b : bufs) b->release();
    delete st;
    ctx->train = nullptr;
}

// the current weights in load_weights order (host), from the trained master copy
int rd_train_weights_host(rd_ctx* ctx, std::vector<float>& flat)
{
    RD_HIP(hipSetDevice(ctx->device));
    if (int rc = state_ready(ctx)) return rc;
    TrainState* st = state_of(ctx);
    flat.resize(st->pm.total);
    RD_HIP(hipMemcpyAsync(flat.data(), st->master.p, st->pm.total * 4, hipMemcpyDeviceToHost, ctx->stream));
    RD_HIP(hipStreamSynchronize(ctx->stream));
    return RD_OK;
}

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" int rd_train_grad(rd_ctx* ctx, const float* windows, int n_windows, const int32_t* input_len, const uint8_t* labels,
                             const int64_t* label_off, const int32_t* label_len, float* grad, double* loss, int32_t* status)
{
    RD_REQUIRE(grad, "rd_train_grad: null grad");
    return train_run(ctx, "rd_train_grad", windows, false, n_windows, input_len, labels, label_off, label_len, nullptr, grad, loss, status);
}

extern "C" int rd_train_step(rd_ctx* ctx, const float* windows, int n_windows, const int32_t* input_len, const uint8_t* labels,
                             const int64_t* label_off, const int32_t* label_len, const rd_adam* opt, double* loss, int32_t* status)
{
    RD_REQUIRE(opt, "rd_train_step: null Adam settings");
    return train_run(ctx, "rd_train_step", windows, false, n_windows, input_len, labels, label_off, label_len, opt, nullptr, loss, status);
}

extern "C" int rd_train_step_resident(rd_ctx* ctx, const float* d_windows, int n_windows, const int32_t* input_len, const uint8_t* labels,
                                      const int64_t* label_off, const int32_t* label_len, const rd_adam* opt, double* loss, int32_t* status)
{
    RD_REQUIRE(opt, "rd_train_step_resident: null Adam settings");
    return train_run(ctx, "rd_train_step_resident", d_windows, true, n_windows, input_len, labels, label_off, label_len, opt, nullptr, loss,
                     status);
}

extern "C" int rd_train_reset(rd_ctx* ctx)
{
    RD_REQUIRE(ctx, "rd_train_reset: null context");
    TrainState* st = state_of(ctx);
    if (!st || st->need_init) return RD_OK;   // the next training call starts from zero moments anyway
    RD_HIP(hipSetDevice(ctx->device));
    const size_t bytes = st->pm.total * sizeof(float);
    RD_HIP(hipMemsetAsync(st->mom_m.p, 0, bytes, ctx->stream));
    RD_HIP(hipMemsetAsync(st->mom_v.p, 0, bytes, ctx->stream));
    RD_HIP(hipStreamSynchronize(ctx->stream));
    st->t = 0;
    return RD_OK;
}

extern "C" int rd_get_weights(rd_ctx* ctx, float* flat, size_t n)
{
    RD_REQUIRE(ctx && flat, "rd_get_weights: null argument");
    RD_REQUIRE(ctx->model.loaded, "rd_get_weights: no weights loaded (rd_load_weights)");
    const size_t expect = param_map(ctx->model.nblocks).total;
    RD_REQUIRE(n == expect, "rd_get_weights: the model has %zu parameters, the buffer holds %zu", expect, n);
    std::vector<float> h;
    if (int rc = rd_train_weights_host(ctx, h)) return rc;
    memcpy(flat, h.data(), expect * 4);
    return RD_OK;
}

extern "C" int rd_train_ctc_grad(rd_ctx* ctx, const float* probs, int n_windows, const int32_t* input_len, const uint8_t* labels,
                                 const int64_t* label_off, const int32_t* label_len, float* grad_z, double* loss, int32_t* status)
{
    const char* fn = "rd_train_ctc_grad";
    RD_REQUIRE(ctx && n_windows >= 1, "%s: null context or no windows", fn);
    RD_REQUIRE(probs && input_len && labels && label_off && label_len && grad_z && loss && status, "%s: null argument", fn);
    RD_REQUIRE(n_windows <= (INT32_MAX / TT) / RD_C, "%s: %d windows in one call", fn, n_windows);
    if (int rc = check_windows(fn, n_windows, input_len, labels, label_off, label_len)) return rc;
    RD_HIP(hipSetDevice(ctx->device));
    if (!state_of(ctx)) ctx->train = new TrainState();
    TrainState* st = state_of(ctx);
    hipStream_t s = ctx->stream;
    const size_t rows = (size_t)n_windows * TT * RD_NCLS;
    if (st->gbuf.reserve(2 * rows * 4)) return RD_ERR_NOMEM;
    float* Y = st->gbuf.as<float>();
    float* GZ = Y + rows;
    CtcDev cd;
    if (int rc = ctc_stage(st->ctc, s, n_windows, input_len, labels, label_off, label_len, status, &cd)) return rc;
    RD_HIP(hipMemcpyAsync(Y, probs, rows * 4, hipMemcpyHostToDevice, s));
    if (int rc = ctc_launch(s, cd, Y, n_windows, GZ)) return rc;
    RD_HIP(hipMemcpyAsync(grad_z, GZ, rows * 4, hipMemcpyDeviceToHost, s));
    return ctc_finish(s, cd, n_windows, status, loss);
}

extern "C" int rd_model_params(rd_ctx* ctx, int64_t* n)
{
    RD_REQUIRE(ctx && n, "rd_model_params: null argument");
    RD_REQUIRE(ctx->model.loaded, "rd_model_params: no weights loaded (rd_load_weights)");
    *n = (int64_t)param_map(ctx->model.nblocks).total;
    return RD_OK;
}
