// quant_rules.h -- the rules of the transcript-quantification contract (include/radian_hip.h, rd_quant_em), once:
// the argument check, the packer, the host twin (rd_quant_em_host) and the kernels of quant.hip all call these.  Integer arithmetic only.
//
// Bounds (R reads < 2^31, at most 64 candidates per read, weights 1..4096 = 2^12, ONE = 2^20):
//   c[t] <= R * ONE < 2^51           every read gives away at most ONE in all
//   a_j = c[t_j] * w_j < 2^63        2^51 * 2^12
//   S = sum_j a_j < 2^63             the t of a read are distinct and sum_t c[t] <= R * ONE, so S <= 2^12 * R * ONE
//   sh = max(0, bitlen(S) - 44)      a'_j = a_j >> sh < 2^44, so a'_j << 20 fits 64 bits; S' = sum_j a'_j < 64 * 2^44 = 2^50
//   S' > 0                           a read's own shares of the step before keep sum_{t in T_r} c[t] >= ONE - 64, so S >= ONE - 64; with
//                                    sh > 0, S >= 2^44 and every floor loses less than 1: S' > S / 2^sh - 64 >= 2^43 - 64.  (In the first
//                                    step c = 1 and S is the sum of the weights.)  The host twin treats S' == 0 as an internal error.
//   share_j = (a'_j << 20) / S' <= ONE; a read loses at most n_r units of 2^-20 to the floors
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define QUANT_HD __host__ __device__
#else
#define QUANT_HD
#endif

constexpr int QUANT_MAX_CAND = 64;          // candidates of one read: a read never straddles a wave
constexpr int QUANT_MAX_W = 4096;           // largest weight
constexpr int QUANT_FRAC_BITS = 20;
constexpr uint64_t QUANT_ONE = (uint64_t)1 << QUANT_FRAC_BITS;
constexpr int QUANT_TERM_BITS = 44;         // a term is shifted down to fewer than 2^44 before the division
constexpr int QUANT_MAX_ITER = 100000;
constexpr int QUANT_ROW = 64;               // slots of a packed row: one wave

static_assert(QUANT_TERM_BITS + QUANT_FRAC_BITS <= 64, "the shifted numerator a' << 20 must fit 64 bits");
static_assert(31 + QUANT_FRAC_BITS + 12 <= 63 && QUANT_MAX_W == (1 << 12), "c[t] * w and a read's sum S stay below 2^63");
static_assert(QUANT_MAX_CAND <= QUANT_ROW && QUANT_TERM_BITS + 6 < 64, "S' is the sum of at most 64 terms below 2^44");

QUANT_HD inline bool quant_weight_ok(uint32_t w) { return w >= 1 && w <= (uint32_t)QUANT_MAX_W; }

QUANT_HD inline int quant_bitlen(uint64_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return 64 - __clzll((long long)x);   // (__clzll(0) is 64)
#else
    return x ? 64 - __builtin_clzll(x) : 0;
#endif
}

// a_j: the count of the candidate's transcript times its weight
QUANT_HD inline uint64_t quant_term(uint64_t c, uint32_t w) { return c * (uint64_t)w; }

// sh: how far the terms of a read whose terms sum to S are shifted down
QUANT_HD inline int quant_shift(uint64_t S)
{
    const int b = quant_bitlen(S);
    return b > QUANT_TERM_BITS ? b - QUANT_TERM_BITS : 0;
}

// share_j = floor(a'_j * 2^20 / S').  The division is the language's own unsigned 64-bit one, on the host and on the device (there the
// compiler's expansion of it): exact for every operand, so nothing has to be proved about an estimate
QUANT_HD inline uint64_t quant_share(uint64_t a_shifted, uint64_t s_shifted) { return (a_shifted << QUANT_FRAC_BITS) / s_shifted; }

// ---- host only ---------------------------------------------------------------------------------------------------------------------
#include <vector>

// The packed form of a call's multi-candidate reads: in the caller's order, into rows of QUANT_ROW slots so that no read straddles a
// row; a read that does not fit the rest of a row starts the next one, and the slots left over are padding (t = -1, their own segment).
// head[i] / end[i]: the first and the last slot, within the row, of the read slot i belongs to.  src[i]: the slot of the caller's CSR
// arrays that packed slot i holds (-1: padding).  base[t]: ONE per single-candidate read that names t (the constant term of every step).
struct QuantPack {
    std::vector<int32_t> t;
    std::vector<uint16_t> w;
    std::vector<uint8_t> head, end;
    std::vector<int64_t> src;
    std::vector<uint64_t> base;
    int64_t n_empty = 0, n_single = 0, n_multi = 0;
};

// (the arguments have passed quant_check_args)
inline void quant_pack(const int64_t* cand_off, const int32_t* cand_t, const uint16_t* cand_w, int64_t n_reads, int64_t n_tx, QuantPack* P)
{
    P->t.clear(), P->w.clear(), P->head.clear(), P->end.clear(), P->src.clear();
    P->base.assign((size_t)n_tx, 0);
    P->n_empty = P->n_single = P->n_multi = 0;
    const auto pad_row = [&]() {
        while (P->t.size() % QUANT_ROW) {
            const uint8_t lane = (uint8_t)(P->t.size() % QUANT_ROW);
            P->t.push_back(-1), P->w.push_back(0), P->head.push_back(lane), P->end.push_back(lane), P->src.push_back(-1);
        }
    };
    for (int64_t r = 0; r < n_reads; r++) {
        const int64_t s0 = cand_off[r], n = cand_off[r + 1] - s0;
        if (n == 0) {
            P->n_empty++;
        } else if (n == 1) {
            P->n_single++;
            P->base[(size_t)cand_t[s0]] += QUANT_ONE;
        } else {
            P->n_multi++;
            if (P->t.size() % QUANT_ROW + (size_t)n > (size_t)QUANT_ROW) pad_row();
            const uint8_t h = (uint8_t)(P->t.size() % QUANT_ROW), e = (uint8_t)(h + n - 1);
            for (int64_t j = 0; j < n; j++)
                P->t.push_back(cand_t[s0 + j]), P->w.push_back(cand_w[s0 + j]), P->head.push_back(h), P->end.push_back(e), P->src.push_back(s0 + j);
        }
    }
    pad_row();
}
