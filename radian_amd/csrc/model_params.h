// model_params.h -- the flat weight order (weights.py's load_weights order: what rd_load_weights reads, training updates and
// rd_get_weights returns) and where an element of a conv / dense kernel lies in the packed images (internal; model.hip, train.hip).
#pragma once
#include "common.h"

constexpr size_t RD_CONV_N = (size_t)RD_K * RD_C * RD_C;   // floats of a conv kernel [j][ci][co]
constexpr size_t RD_D1_N = (size_t)RD_C * RD_H;            // floats of the first dense kernel [ci][h]

// offsets of every tensor in the flat weights; block 0's first conv is the [3][256] kernel of the one-channel signal
struct ParamMap {
    size_t w0[RD_MAX_BLOCKS], b0[RD_MAX_BLOCKS], w1[RD_MAX_BLOCKS], b1[RD_MAX_BLOCKS], wm, bm, wd1, bd1, wd2, bd2, total;
};

inline ParamMap param_map(int nb)
{
    ParamMap p = {};
    size_t o = 0;
    for (int b = 0; b < nb; b++) {
        p.w0[b] = o;
        o += b == 0 ? (size_t)RD_K * RD_C : RD_CONV_N;
        p.b0[b] = o;
        o += RD_C;
        p.w1[b] = o;
        o += RD_CONV_N;
        p.b1[b] = o;
        o += RD_C;
        if (b == 0) {
            p.wm = o;
            o += RD_C;
            p.bm = o;
            o += RD_C;
        }
    }
    p.wd1 = o;
    o += RD_D1_N;
    p.bd1 = o;
    o += RD_H;
    p.wd2 = o;
    o += (size_t)RD_H * RD_NCLS;
    p.bd2 = o;
    o += RD_NCLS;
    p.total = o;
    return p;
}

// A packed image is rows of 16 input channels: row of element [j][ci][co] of a Keras conv kernel (chunk = (ci/16)*3 + j, then
// co) and of element [ci][h] of a dense kernel (chunk = ci/16, then h); the element is channel ci % 16 of its row.
__host__ __device__ inline size_t rd_conv_image_row(int j, int ci, int co) { return ((size_t)(ci / 16) * RD_K + j) * RD_C + co; }
__host__ __device__ inline size_t rd_dense_image_row(int ci, int h) { return (size_t)(ci / 16) * RD_H + h; }
// fp32 image: 64-B rows (16 floats), 16-B slot XOR (row >> 2) & 3 -- the LDS image of forward.hip's half-stages
__host__ __device__ inline int rd_swz_f32(int row, int k) { return ((((k >> 2) ^ ((row >> 2) & 3)) << 2) | (k & 3)); }
