// pileup_rules.h -- the rules of the pileup contract (include/radian_hip.h, rd_pileup_*), once: the argument check,
// the host twin (rd_pileup_host) and pileup_kernel of pileup.hip all call these.  Integer arithmetic only.
//
// One pair = the column ops o[0..L) ('M' 'X' 'D' 'I') of a span A[0..n) against a read B[0..m), the span's first base being site site0.
//   covered interval   from the first M / X column to the last M / X column; none: PILEUP_NO_BASE, nothing accumulated
//   outside it         nothing accumulates: I columns are soft clip (clip_head, clip_tail), D columns shorten [ref_lo, ref_hi)
//   inside it          M / X at span offset i   site[site0 + i][code(read byte)] += 1, conf[code(span byte)][code(read byte)] += 1,
//                                               kmer[ctx(i)][M ? match : sub] += 1 (the column kind is the caller's, the channel the byte's)
//                      D at span offset i       site[site0 + i][del] += 1, conf[code(span byte)][del] += 1, kmer[ctx(i)][del] += 1
//                      I                        ins_base[code(read byte)] += 1
//                      a maximal run of D       del_len[bucket(length)] += 1
//                      a maximal run of I       ins_len[bucket(length)] += 1, and with i the span offset of the nearest ref-consuming column
//                                               before it: site[site0 + i][ins] += 1, kmer[ctx(i)][ins] += 1
//                      the first column         site[site0 + ref_lo][starts] += 1
// The interval begins and ends with an M / X column, so every run inside it is bounded by columns of the interval: a run is seen from
// the column that follows it.  Between two I runs lies a ref-consuming column, so every channel of a site grows by at most one per pair.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PILEUP_HD __host__ __device__
#else
#define PILEUP_HD
#endif

// channels of a site
constexpr int PILEUP_CH = 8;
constexpr int PILEUP_CH_OTHER = 4, PILEUP_CH_DEL = 5, PILEUP_CH_INS = 6, PILEUP_CH_STARTS = 7;
// the profile: conf[5][6] | ins_base[5] | kmer[1024][4] | ins_len[64] | del_len[64]   (include/radian_hip.h RD_PILEUP_*)
constexpr int PILEUP_CONF = 0, PILEUP_INS_BASE = 30, PILEUP_KMER = 35, PILEUP_INS_LEN = 35 + 4096, PILEUP_DEL_LEN = 35 + 4096 + 64;
constexpr int PILEUP_PROFILE_LEN = 35 + 4096 + 128;
constexpr int PILEUP_K_MATCH = 0, PILEUP_K_SUB = 1, PILEUP_K_DEL = 2, PILEUP_K_INS = 3;
// per-pair result ints: status, score, ref_lo, ref_hi, clip_head, clip_tail, n_match, n_sub, n_ins, n_del
constexpr int PILEUP_RES = 10;
constexpr int PILEUP_OK = 0, PILEUP_NO_BASE = 1, PILEUP_TOO_LARGE = 2;
// n + m of a pair stays below 2^28 (rd_align_batch's own bound on its int32 scores), so four pairs add less than 2^30 to a 32-bit counter
constexpr int64_t PILEUP_MAX_COLS = (int64_t)1 << 28;
constexpr int64_t PILEUP_MAX_PAIRS = ((int64_t)1 << 31) - 1;   // pairs between open and close: no 32-bit site counter can overflow
constexpr int64_t PILEUP_MAX_SITES = (int64_t)1 << 30;

static_assert(PILEUP_PROFILE_LEN == 4259 && PILEUP_DEL_LEN + 64 == PILEUP_PROFILE_LEN, "profile layout");

PILEUP_HD inline int pileup_code(uint8_t c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4; }

PILEUP_HD inline bool pileup_is_op(uint8_t o) { return o == 'M' || o == 'X' || o == 'D' || o == 'I'; }

// the 5-mer of the span centred on offset i, A = 0 .. T = 3, leftmost base most significant; -1 within 2 of a span end or with a non-ACGT byte
PILEUP_HD inline int pileup_kmer(const uint8_t* A, int64_t n, int64_t i)
{
    if (i < 2 || i + 2 >= n) return -1;
    int k = 0;
    for (int d = -2; d <= 2; d++) {
        const int c = pileup_code(A[i + d]);
        if (c > 3) return -1;
        k = k * 4 + c;
    }
    return k;
}

// run lengths 1..63 in buckets 0..62, 64 and longer in bucket 63
PILEUP_HD inline int pileup_len_bucket(int64_t len) { return len >= 64 ? 63 : (int)len - 1; }

// ---- host only: one pair over plain loops (the ops have passed the check: every op is M / X / D / I, they consume n and m characters) ----
inline void pileup_pair_host(const uint8_t* o, int64_t L, const uint8_t* A, int64_t n, const uint8_t* B, int64_t m, int64_t site0, uint32_t* site,
                             uint64_t* prof, int32_t* res)
{
    for (int c = 0; c < PILEUP_RES; c++) res[c] = 0;
    int64_t first = -1, last = -1;
    for (int64_t k = 0; k < L; k++)
        if (o[k] == 'M' || o[k] == 'X') {
            if (first < 0) first = k;
            last = k;
        }
    if (first < 0) {
        res[0] = PILEUP_NO_BASE;
        res[4] = (int32_t)m;
        return;
    }
    int64_t i = 0, j = 0, run_d = 0, run_i = 0, last_ref = -1;
    int64_t cnt[4] = {0, 0, 0, 0};
    for (int64_t k = 0; k <= last; k++) {
        const uint8_t op = o[k];
        if (k < first) {
            i += op != 'I';
            j += op != 'D';
            continue;
        }
        if (k == first) {
            res[2] = (int32_t)i;
            res[4] = (int32_t)j;
            site[(site0 + i) * PILEUP_CH + PILEUP_CH_STARTS]++;
        }
        if (op != 'D' && run_d) {
            prof[PILEUP_DEL_LEN + pileup_len_bucket(run_d)]++;
            run_d = 0;
        }
        if (op != 'I' && run_i) {
            prof[PILEUP_INS_LEN + pileup_len_bucket(run_i)]++;
            site[(site0 + last_ref) * PILEUP_CH + PILEUP_CH_INS]++;
            const int km = pileup_kmer(A, n, last_ref);
            if (km >= 0) prof[PILEUP_KMER + km * 4 + PILEUP_K_INS]++;
            run_i = 0;
        }
        if (op == 'I') {
            prof[PILEUP_INS_BASE + pileup_code(B[j])]++;
            run_i++;
            cnt[2]++;
            j++;
            continue;
        }
        const int ca = pileup_code(A[i]), km = pileup_kmer(A, n, i);
        if (op == 'D') {
            site[(site0 + i) * PILEUP_CH + PILEUP_CH_DEL]++;
            prof[PILEUP_CONF + ca * 6 + 5]++;
            if (km >= 0) prof[PILEUP_KMER + km * 4 + PILEUP_K_DEL]++;
            run_d++;
            cnt[3]++;
        } else {
            const int cb = pileup_code(B[j]);
            site[(site0 + i) * PILEUP_CH + cb]++;
            prof[PILEUP_CONF + ca * 6 + cb]++;
            if (km >= 0) prof[PILEUP_KMER + km * 4 + (op == 'M' ? PILEUP_K_MATCH : PILEUP_K_SUB)]++;
            cnt[op == 'M' ? 0 : 1]++;
            j++;
        }
        last_ref = i;
        i++;
    }
    res[3] = (int32_t)i;
    res[5] = (int32_t)(m - j);
    for (int c = 0; c < 4; c++) res[6 + c] = (int32_t)cnt[c];
}
