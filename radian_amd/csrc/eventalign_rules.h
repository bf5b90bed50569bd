// eventalign_rules.h -- the rules of the eventalign contract (include/radian_hip.h, rd_eventalign), once: the host
// loop (rd_eventalign_host), the argument check and the kernels of eventalign.hip all call these.  Integer arithmetic only.
#pragma once
#include <stdint.h>

#include "sim_rules.h"  // sim_kmer, sim_mulhi, sim_k_ok: the k-mer rule is the simulator's

#if defined(__HIPCC__)
#define EA_HD __host__ __device__
#else
#define EA_HD
#endif

// per-read status (radian_hip.h RD_EVAL_*)
constexpr int EA_OK = 0, EA_EMPTY = 1, EA_TOO_LONG = 2, EA_MAD_ZERO = 3, EA_NO_PATH = 4, EA_TOO_LARGE = 5;

constexpr int32_t EA_INF = 1 << 30;       // an unreachable cell
constexpr int64_t EA_MAX_T = 1 << 19;     // rows of one alignment: finite values stay below 2^19 * 1280 < 2^30
constexpr int32_t EA_ZMAX = 1 << 14;      // |zq| <= 2^14 and |lvl| < 2^14: |d| < 2^15, d^2 < 2^30
constexpr int32_t EA_COST_CAP = 1024;     // the squared-distance term of a cell, in 1/32 nat
constexpr int32_t EA_BIAS_MAX = 256;
constexpr int32_t EA_M2_MAX = 1 << 17, EA_D4_MAX = 1 << 20;   // ranges of a given scale

// one state's model: the level in MAD/256, the Q32 inverse variance, the log-sd term in 1/32 nat
struct EaState {
    int32_t lvl;
    uint32_t w;
    int32_t bias;
};

EA_HD inline bool ea_entry_ok(int32_t lvl, int32_t bias) { return lvl > -EA_ZMAX && lvl < EA_ZMAX && bias >= -EA_BIAS_MAX && bias <= EA_BIAS_MAX; }
EA_HD inline bool ea_scale_ok(int32_t m2, int32_t d4) { return m2 >= -EA_M2_MAX && m2 <= EA_M2_MAX && d4 >= 0 && d4 <= EA_D4_MAX; }

// the status a read has before anything is aligned (EA_OK: go on); T rows, L bases, d4 as used
EA_HD inline int ea_status(int64_t T, int64_t L, int32_t d4)
{
    return T <= 0 ? EA_EMPTY : T > EA_MAX_T ? EA_TOO_LONG : d4 == 0 ? EA_MAD_ZERO : T < L ? EA_NO_PATH : EA_OK;
}

// the sample in MAD/256, rounded half up: u = 512 (2x - m2), zq = clamp(floor((2u + d4) / (2 d4)), +-2^14); d4 >= 1
EA_HD inline int32_t ea_quant(int32_t x, int32_t m2, int32_t d4)
{
    const int64_t u = 512 * (2 * (int64_t)x - m2), num = 2 * u + d4, den = 2 * (int64_t)d4;
    int64_t q = num / den;
    if (num % den < 0) q--;   // floor: den > 0
    return (int32_t)(q < -EA_ZMAX ? -EA_ZMAX : q > EA_ZMAX ? EA_ZMAX : q);
}

// c(t, s) = min(floor(d^2 w / 2^32), 1024) + bias, d = zq - lvl
EA_HD inline int32_t ea_cost(int32_t zq, int32_t lvl, uint32_t w, int32_t bias)
{
    const int32_t d = zq - lvl;
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t d2 = (uint32_t)__mul24(d, d);   // |d| < 2^15: the 24-bit multiply is exact
#else
    const uint32_t d2 = (uint32_t)(d * d);
#endif
    const uint32_t q = sim_mulhi(d2, w);
    return (int32_t)(q < (uint32_t)EA_COST_CAP ? q : (uint32_t)EA_COST_CAP) + bias;
}

// the model of state s of 0 .. L + 1: 0 and L + 1 are the background, s in 1 .. L is base s - 1 by its k-mer (sim_rules.h)
EA_HD inline EaState ea_state(int32_t s, int32_t L, const uint8_t* codes, int k, const int32_t* lvl, const uint32_t* w, const int32_t* bias,
                              const EaState& bg)
{
    if (s <= 0 || s > L) return bg;
    const int32_t i = sim_kmer(codes, L, s - 1, k);
    return EaState{lvl[i], w[i], bias[i]};
}

// the advance from s - 1 is taken only if strictly smaller
EA_HD inline bool ea_advance(int32_t stay, int32_t adv) { return adv < stay; }

// the path ends in L + 1, or in L if V[T-1][L+1] is not strictly smaller
EA_HD inline bool ea_ends_in_trail(int32_t v_trail, int32_t v_last) { return v_trail < v_last; }

// ---- event rows (include/radian_hip.h, rd_eventalign_events): the rows are a detector's events, each weighted by
// its sample count, and a third predecessor skips one base
constexpr int32_t EA_SKIP_MAX = 256;      // the largest skip penalty, in 1/32 nat; -1: no skip edge
constexpr int EAR_STAY = 0, EAR_ADV = 1, EAR_SKIP = 2;   // the two-bit back-pointer codes

EA_HD inline bool ear_pen_ok(int32_t skip_pen) { return skip_pen >= -1 && skip_pen <= EA_SKIP_MAX; }

// the status of a window of T samples cut into E events against L bases, before anything is aligned.  Row e reaches the states up to
// e + 1 without skips and up to 2 e + 1 with them; the path must reach state L in row E - 1
EA_HD inline int ear_status(int64_t T, int64_t E, int64_t L, int32_t d4, int32_t skip_pen)
{
    if (T <= 0 || E <= 0) return EA_EMPTY;
    if (T > EA_MAX_T) return EA_TOO_LONG;
    if (d4 == 0) return EA_MAD_ZERO;
    return (skip_pen < 0 ? E : 2 * E - 1) < L ? EA_NO_PATH : EA_OK;
}

// the row of an event of n >= 1 samples that sum to `sum`: its mean, rounded half up
EA_HD inline int64_t ear_mean(int64_t sum, int64_t n)
{
    const int64_t num = 2 * sum + n, den = 2 * n;
    int64_t q = num / den;
    if (num % den < 0) q--;   // floor: den > 0
    return q;
}

// c(e, s) = n_e * ea_cost: n < 2^23 and |cost| <= 1280, the 24-bit multiply is exact; with n <= T <= 2^19 the product stays below 2^30
EA_HD inline int32_t ear_cost(int32_t zq, int32_t n, int32_t lvl, uint32_t w, int32_t bias)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __mul24(ea_cost(zq, lvl, w, bias), n);
#else
    return ea_cost(zq, lvl, w, bias) * n;
#endif
}

// the best of the three predecessors and its code: stay; the advance only if STRICTLY smaller; the skip (skp = V[e-1][s-2] + skip_pen)
// only if STRICTLY smaller than the best of the other two.  On ties: stay, advance, skip
EA_HD inline int32_t ear_best(int32_t stay, int32_t adv, int32_t skp, bool skips, int* code)
{
    const bool a = ea_advance(stay, adv);
    const int32_t b2 = a ? adv : stay;
    const bool k = skips && skp < b2;
    *code = k ? EAR_SKIP : a ? EAR_ADV : EAR_STAY;
    return k ? skp : b2;
}

// ---- sample rows in a band round a guide (include/radian_hip.h, rd_eventalign_banded): rd_eventalign's Viterbi over
// the states of a 64-state window that slides with a per-base guide (the sample each base is expected to start at)
constexpr int EA_OFF_BAND = 6;            // the chosen end value is not finite: the window lost the path
constexpr int EAB_W = 64;                 // states of the window: one wave, one back-pointer word of 64 bits a row
constexpr int32_t EAB_FINITE = 3 << 28;   // a value at or above this started at 2^30 (finite values stay below 0.625 * 2^30)

// the window's lowest state at a row where g bases have guide <= the row's sample; L bases.  Non-decreasing in g
EA_HD inline int32_t eab_lo(int64_t g, int64_t L)
{
    const int64_t a = g - (EAB_W / 2 - 1) > 0 ? g - (EAB_W / 2 - 1) : 0, top = L + 2 - EAB_W > 0 ? L + 2 - EAB_W : 0;
    return (int32_t)(a < top ? a : top);
}

// g(t): the bases of guide[0 .. L) (non-decreasing) that are <= x, the row's sample in read coordinates
EA_HD inline int32_t eab_count(const int32_t* guide, int32_t L, int64_t x)
{
    int32_t lo = 0, hi = L;   // guide[lo - 1] <= x < guide[hi]
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (guide[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the end of a banded pass: `in_win` tells whether states L + 1 and L lie in the last row's window (the other counts as 2^30)
EA_HD inline bool eab_finite(int32_t v) { return v < EAB_FINITE; }

// does base b (state s = b + 1) touch the window's rim?  lo_last / lo_first: the window's lowest state at the base's last and first row
EA_HD inline bool eab_on_rim(int32_t s, int32_t lo_last, int32_t lo_first) { return lo_last == s || lo_first + EAB_W - 1 == s; }
