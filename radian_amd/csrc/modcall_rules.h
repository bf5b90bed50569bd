// modcall_rules.h -- the rules of the modcall contract (include/radian_hip.h, rd_modcall), once: the host loop
// (rd_modcall_host), the argument check and the kernel of modcall.hip all call these.  Integer arithmetic only.
//
// A job re-aligns the rows between two anchors of an existing alignment to the S <= 63 states round a site, twice: under the canonical
// states (ref) and with the job's entries in place of n_alt of them (alt).  Per hypothesis the best path (vit) and the sum over all paths
// (fwd), both in the cell's own unit, 1/32 nat, as negative log likelihoods: fwd = c + softmin(stay, adv),
// softmin(a, b) = min(a, b) - LSE[min(|a - b|, 133)], LSE[d] = floor(32 ln(1 + e^(-d/32)) + 1/2).
//
// Bounds (R <= 2^15 rows, a cell's cost in [-256, 1280], LSE in [0, 22]):
//   finite       a value reached from V[0][0] has taken at most 2^15 cells and lost LSE at most 2^15 - 1 times: it lies in (-2^15 * (256 +
//                22), 2^15 * 1280] = (-2^15 * 278, 2^15 * 1280], and 2^15 * 1280 = 5 * 2^23 < 3 * 2^28
//   unreachable  state i is unreachable at rows t < i only, so for at most 62 rows, in which a value that started at 2^30 loses at most
//                278 and gains at most 1280 a row: it stays in [2^30 - 62 * 278, 2^30 + 62 * 1280], inside [2^30 - 22 * 2^15, 2^31).  (The
//                kernel's lanes past the last state hold cells that cost nothing and are never read out; what they take from lane S - 1 is
//                finite, what they keep from 2^30 loses at most 22 a row: the same interval.)
//   apart        an unreachable value exceeds every finite one by more than 2^30 - 22 * 2^15 - 5 * 2^23 > 133: the difference clamps to
//                133, LSE[133] = 0, and softmin(finite, unreachable) is exactly the finite value.  So nothing is masked: min and softmin of
//                a cell with one unreachable predecessor are those of the reachable one alone
// No sum above leaves int32.
#pragma once
#include <stdint.h>

#include "eventalign_rules.h"   // ea_quant, ea_cost, ea_entry_ok, ea_scale_ok, EA_INF: the sample and the cell are eventalign's

// per-job status (radian_hip.h RD_MC_*)
constexpr int MC_OK = 0, MC_NO_ANCHOR = 1, MC_NO_PATH = 2, MC_TOO_LONG = 3, MC_TOO_LARGE = 4;

constexpr int32_t MC_MAX_ALT = 9;          // replaced states of a job: the k-mers of k <= 9 that cover one base
constexpr int32_t MC_MAX_FLANK = 27;       // 9 + 2 * 27 = 63 states at the most
constexpr int32_t MC_MAX_S = 63;
constexpr int64_t MC_MAX_R = 1 << 15;      // rows of a job
constexpr int32_t MC_LSE_N = 134;          // LSE[d], d = 0 .. 133; 0 from 133 on

// floor(32 ln(1 + e^(-d/32)) + 1/2): how far below the smaller of two values 1/32 nat apart by d their log-sum lies
#define MC_LSE_LITERAL                                                                                                                  \
    22, 22, 21, 21, 20, 20, 19, 19, 18, 18, 18, 17, 17, 16, 16, 16, 15, 15, 14, 14, 14, 13, 13, 13, 12, 12, 12, 11, 11, 11, 11, 10,    \
    10, 10, 9, 9, 9, 9, 9, 8, 8, 8, 8, 7, 7, 7, 7, 7, 6, 6, 6, 6, 6, 6, 5, 5, 5, 5, 5, 5, 5, 4, 4, 4,                                    \
    4, 4, 4, 4, 4, 4, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2,                                      \
    2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,                                      \
    1, 1, 1, 1, 1, 0
constexpr uint8_t MC_LSE[MC_LSE_N] = {MC_LSE_LITERAL};

EA_HD inline bool mc_flank_ok(int32_t F) { return F >= 0 && F <= MC_MAX_FLANK; }
EA_HD inline bool mc_job_ok(int32_t alt_first, int64_t n_alt, int32_t L) { return n_alt >= 1 && n_alt <= MC_MAX_ALT && alt_first >= 0 && alt_first + n_alt <= L; }

// the window of a job: states a0 .. a0 + S - 1 (bases, pore order), rows r0 .. r0 + R - 1 (read sample coordinates)
struct McWindow {
    int32_t status, a0, S, r0, R;   // (status: MC_TOO_LARGE is the launch's, not the window's)
};

// first / last: the read's steps (L of them each, -1: a base without rows); n: the read's samples.  The job has passed mc_job_ok
EA_HD inline McWindow mc_window(const int32_t* first, const int32_t* last, int32_t L, int64_t n, int32_t alt_first, int32_t n_alt, int32_t F)
{
    const int32_t a0 = alt_first - F > 0 ? alt_first - F : 0, top = alt_first + n_alt - 1 + F, a1 = top < L - 1 ? top : L - 1;
    McWindow wd{MC_OK, a0, a1 - a0 + 1, 0, 0};
    const int64_t r0 = first[a0], r1 = last[a1], R = r1 - r0 + 1;
    if (r0 == -1 || r1 == -1) return wd.status = MC_NO_ANCHOR, wd;
    if (R < wd.S || r0 < 0 || r1 >= n) return wd.status = MC_NO_PATH, wd;
    if (R > MC_MAX_R) return wd.status = MC_TOO_LONG, wd;
    wd.r0 = (int32_t)r0;
    wd.R = (int32_t)R;
    return wd;
}

// the index into LSE of two values: min(|a - b|, 133); the difference of any two int32 is exact as an unsigned 32-bit number
EA_HD inline int32_t mc_lse_index(int32_t a, int32_t b)
{
    const uint32_t d = a < b ? (uint32_t)b - (uint32_t)a : (uint32_t)a - (uint32_t)b;
    return (int32_t)(d < (uint32_t)(MC_LSE_N - 1) ? d : (uint32_t)(MC_LSE_N - 1));
}

// one cell: the best and the summed value from the two predecessors' (lse: the table, wherever the caller keeps it)
EA_HD inline int32_t mc_vit(int32_t c, int32_t stay, int32_t adv) { return c + (adv < stay ? adv : stay); }
template <typename Table> EA_HD inline int32_t mc_fwd(int32_t c, int32_t stay, int32_t adv, const Table& lse)
{
    return c + (adv < stay ? adv : stay) - (int32_t)lse[mc_lse_index(stay, adv)];
}
