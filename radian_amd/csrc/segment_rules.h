// segment_rules.h -- the rules of the event-detection contract (include/radian_hip.h, rd_segment), once: the host
// loop (rd_segment_host), the argument check and the kernels of segment.hip all call these.  Integer arithmetic only.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SG_HD __host__ __device__
#else
#define SG_HD
#endif

// per-read status (radian_hip.h RD_SEGMENT_*)
constexpr int SG_OK = 0, SG_EMPTY = 1, SG_TOO_LONG = 2, SG_TOO_LARGE = 3;
constexpr int64_t SG_MAX_T = (int64_t)1 << 30;
constexpr int SG_MAX_W = 64;   // the longest window

struct SgParams {
    int32_t w1, w2;       // the short window 2..32; the long one, 0 (off) or w1 < w2 <= 64
    uint32_t th1, th2;    // t^2 thresholds in sixteenths
    int32_t v0;           // variance floor in DAQ^2, 1..2^16
};

SG_HD inline bool sg_params_ok(const SgParams& p)
{
    return p.w1 >= 2 && p.w1 <= 32 && (p.w2 == 0 || (p.w2 > p.w1 && p.w2 <= SG_MAX_W)) && p.v0 >= 1 && p.v0 <= (1 << 16);
}

// the status a read has before a sample is looked at (SG_OK: go on)
SG_HD inline int sg_status(int64_t T) { return T <= 0 ? SG_EMPTY : T > SG_MAX_T ? SG_TOO_LONG : SG_OK; }

// events a read of T samples can come to: boundaries lie in [w1, T - w1] and more than w1 apart
SG_HD inline int64_t sg_max_events(int64_t T, int32_t w1) { return T / (w1 + 1) + 1; }

// detector d (0, 1) of the parameters: its window (0: the detector is off) and its threshold
SG_HD inline int32_t sg_window(const SgParams& p, int d) { return d == 0 ? p.w1 : p.w2; }
SG_HD inline uint32_t sg_threshold(const SgParams& p, int d) { return d == 0 ? p.th1 : p.th2; }

// has sample i of a read of T samples both windows of length w inside the read?
SG_HD inline bool sg_in_range(int64_t i, int64_t T, int32_t w) { return i >= w && i <= T - w; }

// Welch's t^2 = N / D between x[i - w .. i) and x[i .. i + w) from the windows' sums and sums of squares.  |S| <= w 2^15 and Q <= w 2^30:
// N < 2^50, 2 w^2 <= D < 2^44
SG_HD inline uint64_t sg_num(int32_t w, int32_t S1, int32_t S2)
{
    const int64_t d = (int64_t)S1 - S2;
    return (uint64_t)w * (uint64_t)(d * d);
}
SG_HD inline uint64_t sg_den(int32_t w, int32_t S1, int64_t Q1, int32_t S2, int64_t Q2, int32_t v0)
{
    return (uint64_t)((int64_t)w * Q1 - (int64_t)S1 * S1 + (int64_t)w * Q2 - (int64_t)S2 * S2 + 2 * (int64_t)w * w * v0);
}

// high 64 bits of a 64 x 64 -> 128-bit product
SG_HD inline uint64_t sg_mulhi(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// a b < c d, the products in 128 bits
SG_HD inline bool sg_prod_less(uint64_t a, uint64_t b, uint64_t c, uint64_t d)
{
    const uint64_t lh = sg_mulhi(a, b), ll = a * b, rh = sg_mulhi(c, d), rl = c * d;
    return lh < rh || (lh == rh && ll < rl);
}

// t(j) < t(i): N(j) D(i) < N(i) D(j)
SG_HD inline bool sg_t_less(uint64_t Nj, uint64_t Dj, uint64_t Ni, uint64_t Di) { return sg_prod_less(Nj, Di, Ni, Dj); }

// N > 0 and 16 N >= th D (16 N < 2^54; th D < 2^76)
SG_HD inline bool sg_candidate(uint64_t N, uint64_t D, uint32_t th)
{
    return N > 0 && sg_mulhi((uint64_t)th, D) == 0 && 16 * N >= (uint64_t)th * D;
}

// does j, |j - i| <= w, j != i, leave the candidate i a peak: t(j) < t(i) before it, t(j) <= t(i) behind it
SG_HD inline bool sg_yields(int64_t j, int64_t i, uint64_t Nj, uint64_t Dj, uint64_t Ni, uint64_t Di)
{
    return j < i ? sg_t_less(Nj, Dj, Ni, Di) : !sg_t_less(Ni, Di, Nj, Dj);
}

// a peak of detector 2 at i is dropped by a peak of detector 1 at j
SG_HD inline bool sg_shadows(int64_t j, int64_t i, int32_t w2) { return (j > i ? j - i : i - j) < w2; }

// the row sigmap --events hands to rd_sigmap for an event of n >= 1 samples: its mean, rounded half up
SG_HD inline int16_t sg_event_row(int64_t sum, int64_t n)
{
    const int64_t a = 2 * sum + n, b = 2 * n;
    return (int16_t)(a >= 0 ? a / b : -((-a + b - 1) / b));
}
