// polya_rules.h -- the rules of the poly(A) flat-segment contract (include/radian_hip.h, rd_polya_segment), once:
// the host loop (rd_polya_segment_host), the argument check and the kernels of polya.hip all call these.  Integer arithmetic only.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PA_HD __host__ __device__
#else
#define PA_HD
#endif

// per-read status (radian_hip.h RD_POLYA_*)
constexpr int PA_OK = 0, PA_NONE = 1, PA_MAD_ZERO = 2, PA_SHORT = 3, PA_EMPTY = 4, PA_TOO_LARGE = 5;

struct PaParams {
    int32_t win, flat_q, use_level, lo_q, hi_q, max_gap;
    int64_t min_samples, search_limit;
};

// what a read comes to (rd_polya_segment's per-read outputs, as the segment kernel stores them)
struct PaOut {
    int64_t tail_start, tail_end, sum, sumsq;
    int32_t status, n_flat, m2, d4, n_candidates, pad_;
};

PA_HD inline bool pa_params_ok(const PaParams& p)
{
    return p.win >= 8 && p.win <= 256 && p.flat_q >= 1 && p.flat_q <= 32767 && (p.use_level == 0 || p.use_level == 1) &&
           p.lo_q >= -(1 << 20) && p.hi_q <= (1 << 20) && p.lo_q <= p.hi_q && p.max_gap >= 0 && p.max_gap <= 1024 && p.min_samples >= p.win &&
           p.search_limit >= 0;
}

// the status a read has before any window is looked at (PA_OK: go on); T samples, d4 = 4 MAD
PA_HD inline int pa_scale_status(int64_t T, int32_t win, int32_t d4)
{
    return T <= 0 ? PA_EMPTY : d4 == 0 ? PA_MAD_ZERO : T < win ? PA_SHORT : PA_OK;
}

// high 64 bits of a 64 x 64 -> 128-bit product
PA_HD inline uint64_t pa_mulhi(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// thr = floor(A^2 / 2^20) saturated to 2^64 - 1, A = win * flat_q * d4 (below 2^41: 2^8 * 2^15 * 2^18).  A^2 = hi * 2^64 + lo;
// the quotient is hi * 2^44 + (lo >> 20) and leaves 64 bits when hi >= 2^20
PA_HD inline uint64_t pa_threshold(int32_t win, int32_t flat_q, int32_t d4)
{
    const uint64_t A = (uint64_t)win * (uint64_t)flat_q * (uint64_t)d4;
    const uint64_t hi = pa_mulhi(A, A), lo = A * A;
    return hi >= ((uint64_t)1 << 20) ? ~(uint64_t)0 : (hi << 44) | (lo >> 20);
}

// V = win * Q - S^2 (win^2 times the window's variance; at most 2^8 * 2^38) from the window's sum and sum of squares
PA_HD inline uint64_t pa_spread(int32_t win, int32_t S, int64_t Q)
{
    return (uint64_t)((int64_t)win * Q - (int64_t)S * S);
}

// is the window flat: V <= thr, and with use_level  lo_q d4 win <= 512 (2 S - win m2) <= hi_q d4 win  (every term fits int64)
PA_HD inline bool pa_flat(const PaParams& p, int32_t m2, int32_t d4, uint64_t thr, int32_t S, int64_t Q)
{
    if (pa_spread(p.win, S, Q) > thr) return false;
    if (!p.use_level) return true;
    const int64_t lvl = 512 * (2 * (int64_t)S - (int64_t)p.win * m2), unit = (int64_t)d4 * p.win;
    return (int64_t)p.lo_q * unit <= lvl && lvl <= (int64_t)p.hi_q * unit;
}

// flat windows i < j with no flat window between them: the same segment?
PA_HD inline bool pa_joined(const PaParams& p, int64_t i, int64_t j) { return j - i <= (int64_t)p.max_gap + 1; }

// segment [a, b] (its first and last flat window): a candidate?
PA_HD inline bool pa_candidate(const PaParams& p, int64_t a, int64_t b)
{
    return (b - a + 1) * p.win >= p.min_samples && (p.search_limit == 0 || a * p.win < p.search_limit);
}

// the choice as one key, larger is better: length descending, then start ascending.  0 is below every segment's key (length >= 1)
PA_HD inline uint64_t pa_key(int64_t a, int64_t b) { return ((uint64_t)(b - a + 1) << 32) | (uint64_t)(0xffffffffu - (uint32_t)a); }
PA_HD inline int64_t pa_key_len(uint64_t key) { return (int64_t)(key >> 32); }
PA_HD inline int64_t pa_key_start(uint64_t key) { return (int64_t)(0xffffffffu - (uint32_t)key); }
