// scoremath.hip -- a probe of the beam search's scalar score arithmetic: rd_diag_score_math evaluates ONE routine of decode_common.h
// (the "fast" mode: exp_nonpos, log1p_unit, lae, safe_log<false>, count4_gt) or of glibc_math.h (the "glibc" mode: gm_exp, gm_log,
// gm_log1p, gm_log1p_unit, lae_gx, safe_log<true>) on n arguments, one thread per element; rd_diag_score_math_host evaluates the glibc
// selections from the same header compiled for the host.  For tests (include/radian_hip_diag.h): the search kernels call these routines
// only on the arguments a search happens to produce.
//
// Why a separate kernel is a faithful probe: this file includes the two headers and calls their routines themselves -- it holds no copy
// of them.  Both headers switch contraction off and spell every fused operation out (gm_fma / __builtin_fma / v_fma_f64 in the inline
// assembly), so each result is a fixed sequence of IEEE binary64 operations plus ldexp, rint, fmax / fmin and, for safe_log<false>, the
// device library's log.  The value of such a sequence does not depend on the kernel around it: what the compiler may change from one
// kernel to the next is register allocation and scheduling, not an operation or its rounding.  As in the search kernels, gm_exp's table is
// read from LDS and gm_log's in place.
#include "decode_common.h"

#include "../../include/radian_hip_diag.h"

#include <float.h>

namespace {

constexpr int kSmTPB = 256;
constexpr int64_t kSmMaxN = (int64_t)1 << 24;

__global__ __launch_bounds__(kSmTPB) void score_math_kernel(int which, const double* __restrict__ x, const double* __restrict__ y, int64_t n,
                                                            double* __restrict__ out)
{
    __shared__ uint64_t gx_lds[256];
    gx_lds[threadIdx.x] = g_gm_exp_tab[threadIdx.x];   // (kSmTPB == 256 == the table's words)
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * kSmTPB + threadIdx.x;
    if (i >= n) return;
    double r = 0.0;
    switch (which) {   // (uniform: a scalar branch)
        case RD_SM_EXP_NONPOS: r = exp_nonpos(x[i]); break;
        case RD_SM_LOG1P_UNIT: r = log1p_unit(x[i]); break;
        case RD_SM_LAE: r = lae(x[i], y[i]); break;
        case RD_SM_SAFE_LOG: r = safe_log<false>(x[i]); break;
        case RD_SM_GM_EXP: r = gm_exp(x[i], gx_lds); break;
        case RD_SM_GM_LOG: r = gm_log(x[i], g_gm_log_tab); break;
        case RD_SM_GM_LOG1P: r = gm_log1p(x[i]); break;
        case RD_SM_GM_LOG1P_UNIT: r = gm_log1p_unit(x[i]); break;
        case RD_SM_LAE_GX: r = lae_gx(x[i], y[i], gx_lds); break;
        case RD_SM_SAFE_LOG_GX: r = safe_log<true>(x[i]); break;
        case RD_SM_COUNT4_GT: r = (double)count4_gt(0, x[4 * i], x[4 * i + 1], x[4 * i + 2], x[4 * i + 3], y[i]); break;
    }
    out[i] = r;
}

const uint64_t h_gm_exp_tab[256] = RD_GLIBC_EXP_TAB;
const uint64_t h_gm_log_tab[256] = RD_GLIBC_LOG_TAB;

bool sm_needs_y(int which) { return which == RD_SM_LAE || which == RD_SM_LAE_GX || which == RD_SM_COUNT4_GT; }

int sm_check(const char* who, int which, const double* x, const double* y, int64_t n, const double* out)
{
    RD_REQUIRE(which >= RD_SM_EXP_NONPOS && which <= RD_SM_COUNT4_GT, "%s: unknown routine %d", who, which);
    RD_REQUIRE(x && out && (y || !sm_needs_y(which)), "%s: null argument", who);
    RD_REQUIRE(n >= 0 && n <= kSmMaxN, "%s: n = %lld is outside 0 .. 2^24", who, (long long)n);
    return RD_OK;
}

}  // namespace

extern "C" int rd_diag_score_math(rd_ctx* ctx, int which, const double* x, const double* y, int64_t n, double* out)
{
    RD_REQUIRE(ctx, "rd_diag_score_math: null context");
    if (int rc = sm_check("rd_diag_score_math", which, x, y, n, out)) return rc;
    RD_HIP(hipSetDevice(ctx->device));
    if (n == 0) return RD_OK;
    const size_t nx = (size_t)n * (which == RD_SM_COUNT4_GT ? 4 : 1), ny = sm_needs_y(which) ? (size_t)n : 0;
    if (ctx->ws_in.reserve((nx + ny) * 8) || ctx->ws_misc.reserve((size_t)n * 8)) return RD_ERR_NOMEM;
    double* const d_x = ctx->ws_in.as<double>();
    double* const d_y = ny ? d_x + nx : nullptr;
    double* const d_out = ctx->ws_misc.as<double>();
    RD_HIP(hipMemcpyAsync(d_x, x, nx * 8, hipMemcpyHostToDevice, ctx->stream));
    if (ny) RD_HIP(hipMemcpyAsync(d_y, y, ny * 8, hipMemcpyHostToDevice, ctx->stream));
    const unsigned blocks = (unsigned)((n + kSmTPB - 1) / kSmTPB);
    hipLaunchKernelGGL(score_math_kernel, dim3(blocks), dim3(kSmTPB), 0, ctx->stream, which, (const double*)d_x, (const double*)d_y, n, d_out);
    RD_HIP(hipGetLastError());
    RD_HIP(hipMemcpyAsync(out, d_out, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
    RD_HIP(hipStreamSynchronize(ctx->stream));
    return RD_OK;
}

// The glibc selections on the host, from glibc_math.h as this translation unit's host pass compiles it.  lae_gx and safe_log<true> are
// device functions of decode_common.h; their two lines around the header's routines are restated here.
extern "C" int rd_diag_score_math_host(int which, const double* x, const double* y, int64_t n, double* out)
{
    if (int rc = sm_check("rd_diag_score_math_host", which, x, y, n, out)) return rc;
    RD_REQUIRE(which >= RD_SM_GM_EXP && which <= RD_SM_SAFE_LOG_GX, "rd_diag_score_math_host: routine %d exists on the device only", which);
    for (int64_t i = 0; i < n; i++) {
        const double a = x[i];
        double r = 0.0;
        switch (which) {
            case RD_SM_GM_EXP: r = gm_exp(a, h_gm_exp_tab); break;
            case RD_SM_GM_LOG: r = gm_log(a, h_gm_log_tab); break;
            case RD_SM_GM_LOG1P: r = gm_log1p(a); break;
            case RD_SM_GM_LOG1P_UNIT: r = gm_log1p_unit(a); break;
            case RD_SM_LAE_GX: {
                const double b = y[i], hi = fmax(a, b), lo = fmin(a, b);
                const double s = hi + gm_log1p_unit(gm_exp(lo - hi, h_gm_exp_tab));
                r = a == b ? a + kLogE2 : s;
                break;
            }
            case RD_SM_SAFE_LOG_GX: r = (a > 0.0 && a <= DBL_MAX) ? gm_log(a, h_gm_log_tab) : -INFINITY; break;
        }
        out[i] = r;
    }
    return RD_OK;
}
