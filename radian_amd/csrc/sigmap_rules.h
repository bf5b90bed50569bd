// sigmap_rules.h -- the rules of the sigmap contract (include/radian_hip.h, rd_sigmap), once: the host loop
// (rd_sigmap_host), the argument check and the kernels of sigmap.hip all call these.  The sample, the cost, the state model and the strict
// advance are eventalign's (eventalign_rules.h); what is added is the free start and end in a reference of many targets.  Integers only.
#pragma once
#include <stdint.h>

#include "eventalign_rules.h"   // ea_quant, ea_cost, EaState, ea_advance, ea_scale_ok, ea_entry_ok

// per-query status (radian_hip.h RD_SIGMAP_*)
constexpr int SM_OK = 0, SM_EMPTY = 1, SM_TOO_LONG = 2, SM_MAD_ZERO = 3, SM_NO_TARGET = 4, SM_TOO_LARGE = 5;

constexpr int64_t SM_MAX_T = 1 << 14;      // rows of one query: every value stays inside +-2^14 * 1280 < 2^25
constexpr int32_t SM_BIAS = 1 << 25;       // added to a score to make the key of the reduction unsigned
constexpr int SM_MAX_BEST = 8;
constexpr int SM_BAND = 4096;              // states of one workgroup pass: 256 threads x 16 states
constexpr int32_t SM_PAYLOAD = 6145;       // end states a stripe reports (mirrored in backend.py); it computes T - 1 more in front of them:
                                           // with T = 2048 a stripe is two whole bands and a quarter of its cells are the halo's
constexpr uint64_t SM_NO_KEY = ~(uint64_t)0;

// the status a query has before anything is aligned (SM_OK: go on); T rows, d4 as used, n_states in its range
EA_HD inline int sm_status(int64_t T, int32_t d4, int64_t n_states)
{
    return T <= 0 ? SM_EMPTY : T > SM_MAX_T ? SM_TOO_LONG : d4 == 0 ? SM_MAD_ZERO : n_states <= 0 ? SM_NO_TARGET : SM_OK;
}

// the target that holds state s: the last j with tgt_off[j] <= s (empty targets before it share the offset and hold nothing)
EA_HD inline int32_t sm_target_of(const int64_t* tgt_off, int32_t n_tgt, int64_t s)
{
    int32_t lo = 0, hi = n_tgt;   // tgt_off[lo] <= s < tgt_off[hi]
    while (hi - lo > 1) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (tgt_off[mid] <= s) lo = mid;
        else hi = mid;
    }
    return lo;
}

// a state no path enters from the left: the first of its target, or the first of the query's range
EA_HD inline bool sm_head(int64_t s, int64_t tgt_first, int64_t s_lo) { return s == tgt_first || s == s_lo; }

// the reduction's key: smaller score first, then the smaller state; |score| < 2^25
EA_HD inline uint64_t sm_key(int32_t score, uint32_t s) { return ((uint64_t)(uint32_t)(score + SM_BIAS) << 32) | s; }
EA_HD inline int32_t sm_key_score(uint64_t key) { return (int32_t)(uint32_t)(key >> 32) - SM_BIAS; }
EA_HD inline uint32_t sm_key_state(uint64_t key) { return (uint32_t)key; }

// the stripes of a range of n states: stripe i reports the ends [s_lo + i P, min(s_lo + (i + 1) P, s_hi)) and computes from
// max(s_lo, that start - (T - 1)): a path that ends in e started at or after e - (T - 1)
EA_HD inline int64_t sm_n_stripes(int64_t n_states) { return (n_states + SM_PAYLOAD - 1) / SM_PAYLOAD; }
EA_HD inline int64_t sm_stripe_left(int64_t a, int64_t T, int64_t s_lo) { return a - (T - 1) > s_lo ? a - (T - 1) : s_lo; }

// device workspace of one query (rd_sigmap_workspace_bytes), each term rounded up to 256
EA_HD inline int64_t sm_round256(int64_t x) { return (x + 255) / 256 * 256; }
EA_HD inline int64_t sm_query_bytes(int64_t T, int64_t n_states, int64_t n_tgt)
{
    const int64_t widest = n_states < SM_PAYLOAD + T - 1 ? n_states : SM_PAYLOAD + T - 1;
    return sm_round256(4 * T) + sm_round256(4 * n_states) + sm_round256(8 * n_tgt) + (widest > SM_BAND ? sm_n_stripes(n_states) * sm_round256(16 * T) : 0);
}
