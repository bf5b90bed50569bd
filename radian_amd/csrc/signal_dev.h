// signal_dev.h -- device builds only: what rd_eventalign and rd_sigmap do alike before their launches -- the k-mer tables' upload and the
// scale stage (one scale per window: as given, or the window's own by select.h's window_scale2).  The rule is eventalign_rules.h's.
#pragma once
#include "common.h"
#include "select.h"

#include <vector>

namespace {

struct SignalScaleIn {
    int64_t raw0, n;   // the scale window's sample 0 in the raw buffer, its samples
    int32_t T, m2, d4, pad_;   // the rows of the window to align (max_T + 1: more than that), the scale as given (d4 = 0: compute it)
};

// one 256-thread workgroup per window; out[2 i], out[2 i + 1] = m2, d4 as used ((0, 0): nothing to align; d4 = 0: no scale)
__global__ __launch_bounds__(256) void signal_scale_kernel(const SignalScaleIn* __restrict__ in, const int16_t* __restrict__ raw, int max_T,
                                                           int32_t* __restrict__ out)
{
    __shared__ unsigned hist[512];
    __shared__ int sh[8];
    const SignalScaleIn q = in[blockIdx.x];
    int m2 = q.m2, d4 = q.d4;
    if (q.T <= 0 || q.T > max_T) m2 = d4 = 0;   // (the same in every thread)
    else if (q.d4 == 0) {
        m2 = 0;
        if (q.n > 0) window_scale2(raw + q.raw0, q.n, hist, sh, &m2, &d4);
    }
    if (threadIdx.x == 0) {
        out[2 * (int64_t)blockIdx.x] = m2;
        out[2 * (int64_t)blockIdx.x + 1] = d4;
    }
}

inline SignalScaleIn signal_scale_in(int64_t raw0, int64_t n, int64_t T, int64_t max_T, int32_t m2, int32_t d4)
{
    return SignalScaleIn{raw0, n, (int32_t)(T > max_T ? max_T + 1 : T), m2, d4, 0};
}

// every window's scale into scale[2 i], scale[2 i + 1], through ctx->ws_eval; the stream is idle on return
inline int signal_scales(rd_ctx* ctx, hipStream_t st, const int16_t* d_raw, const std::vector<SignalScaleIn>& in, int64_t max_T,
                         std::vector<int32_t>& scale)
{
    const size_t n = in.size();
    scale.resize(2 * n);
    SignalScaleIn* d_in = nullptr;
    int32_t* d_scale = nullptr;
    const auto layout = [&](Carve& c) {
        d_in = c.take<SignalScaleIn>(n);
        d_scale = c.take<int32_t>(2 * n, 256, 1);
    };
    if (rd_carve(ctx->ws_eval, layout)) return RD_ERR_NOMEM;
    RD_HIP(hipMemcpyAsync(d_in, in.data(), n * sizeof(SignalScaleIn), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(signal_scale_kernel, dim3((unsigned)n), dim3(256), 0, st, d_in, d_raw, (int)max_T, d_scale);
    RD_HIP(hipGetLastError());
    RD_HIP(hipMemcpyAsync(scale.data(), d_scale, n * 8, hipMemcpyDeviceToHost, st));
    RD_HIP(hipStreamSynchronize(st));
    return RD_OK;
}

struct KmerTables {
    const int32_t* lvl;
    const uint32_t* w;
    const int32_t* bias;
    uint8_t* extra;   // the caller's bytes behind the tables (256-aligned)
};

// the three tables of 4^k entries into ctx->ws_eval_model, with extra_bytes behind them
inline int signal_upload_tables(rd_ctx* ctx, hipStream_t st, int k, const int32_t* lvl, const uint32_t* w, const int32_t* bias, size_t extra_bytes,
                                KmerTables* d)
{
    const size_t nk = (size_t)1 << (2 * k);
    const auto layout = [&](Carve& c) {
        d->lvl = c.take<int32_t>(nk);
        d->w = c.take<uint32_t>(nk);
        d->bias = c.take<int32_t>(nk);
        d->extra = c.take<uint8_t>(extra_bytes, 0, 1);
    };
    if (rd_carve(ctx->ws_eval_model, layout)) return RD_ERR_NOMEM;
    RD_HIP(hipMemcpyAsync((void*)d->lvl, lvl, nk * 4, hipMemcpyHostToDevice, st));
    RD_HIP(hipMemcpyAsync((void*)d->w, w, nk * 4, hipMemcpyHostToDevice, st));
    RD_HIP(hipMemcpyAsync((void*)d->bias, bias, nk * 4, hipMemcpyHostToDevice, st));
    return RD_OK;
}

}  // namespace
