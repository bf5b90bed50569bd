// select.h -- exact order statistics of a read on the device: the two-pass radix select that preprocess.hip (mad_normalise_kernel) and
// polya.hip (pa_scale_kernel) share.  One workgroup per read; LDS: hist[512] unsigned, sh[8] int.
#pragma once
#include <stdint.h>

namespace {

struct SelectResult {
    int v1, v2;  // the two middle order statistics (equal ranks when N is odd)
};

// k-th smallest (0-based ranks k1 <= k2) of key(i), keys in [0, 2^(HB+8)); two histogram passes.
template <int HB, typename KeyFn>
__device__ SelectResult radix_select2(int64_t n, int64_t k1, int64_t k2, KeyFn key, unsigned* hist /*[1<<HB] or [256]*/,
                                      int* sh /*[8]*/)
{
    constexpr int NH = 1 << HB;
    const int tid = threadIdx.x;
    // ---- pass 1: high bits
    for (int i = tid; i < NH; i += blockDim.x) hist[i] = 0;
    __syncthreads();
    for (int64_t i = tid; i < n; i += blockDim.x) atomicAdd(&hist[key(i) >> 8], 1u);
    __syncthreads();
    if (tid == 0) {
        int64_t c = 0;
        int b1 = -1, b2 = -1;
        int64_t r1 = 0, r2 = 0;
        for (int b = 0; b < NH; b++) {
            const int64_t h = hist[b];
            if (b1 < 0 && k1 < c + h) { b1 = b; r1 = k1 - c; }
            if (b2 < 0 && k2 < c + h) { b2 = b; r2 = k2 - c; }
            c += h;
        }
        sh[0] = b1; sh[1] = b2; sh[2] = (int)r1; sh[3] = (int)r2;
    }
    __syncthreads();
    const int b1 = sh[0], b2 = sh[1];
    const int r1 = sh[2], r2 = sh[3];
    // ---- pass 2: low 8 bits inside bin b1 (and b2 when it differs): hist[0..255] and hist[256..511]
    __syncthreads();
    for (int i = tid; i < 512; i += blockDim.x) hist[i] = 0;
    __syncthreads();
    for (int64_t i = tid; i < n; i += blockDim.x) {
        const int k = key(i);
        const int hb = k >> 8;
        if (hb == b1) atomicAdd(&hist[k & 255], 1u);
        if (hb == b2 && b2 != b1) atomicAdd(&hist[256 + (k & 255)], 1u);
    }
    __syncthreads();
    if (tid == 0) {
        int c = 0, v1 = -1, v2 = -1;
        for (int b = 0; b < 256; b++) {
            c += (int)hist[b];
            if (v1 < 0 && r1 < c) v1 = (b1 << 8) | b;
            if (b2 == b1 && v2 < 0 && r2 < c) v2 = (b1 << 8) | b;
        }
        if (b2 != b1) {
            c = 0;
            for (int b = 0; b < 256; b++) {
                c += (int)hist[256 + b];
                if (v2 < 0 && r2 < c) v2 = (b2 << 8) | b;
            }
        }
        sh[4] = v1; sh[5] = v2;
    }
    __syncthreads();
    SelectResult r;
    r.v1 = sh[4];
    r.v2 = sh[5];
    __syncthreads();
    return r;
}

// the scale of a window of n >= 1 int16 samples (rd_eventalign's rule; signal_dev.h's signal_scale_kernel): m2 = the sum of the
// two middle order statistics, d4 = the same of |2x - m2|.  One workgroup; hist[512], sh[8]; the result is the same in every thread
__device__ inline void window_scale2(const int16_t* __restrict__ x, int64_t n, unsigned* hist, int* sh, int* m2_out, int* d4_out)
{
    const int64_t k1 = (n - 1) / 2, k2 = n / 2;
    const SelectResult m = radix_select2<8>(n, k1, k2, [&](int64_t i) { return (int)x[i] + 32768; }, hist, sh);
    const int m2 = (m.v1 - 32768) + (m.v2 - 32768);
    const SelectResult d = radix_select2<9>(n, k1, k2, [&](int64_t i) { const int v = 2 * (int)x[i] - m2; return v < 0 ? -v : v; }, hist, sh);
    *m2_out = m2;
    *d4_out = d.v1 + d.v2;
}

}  // namespace
