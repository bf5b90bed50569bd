// sim_rules.h -- the rules of the signal-simulation contract (include/radian_hip.h, rd_sim_signal), once: the host
// loop (rd_sim_*_host), the argument check and the kernels of sim.hip all call these.  Integer arithmetic only.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SIM_HD __host__ __device__
#else
#define SIM_HD
#endif

// per-read status (radian_hip.h RD_SIM_*)
constexpr int SIM_OK = 0, SIM_EMPTY = 1, SIM_TOO_LARGE = 2;

constexpr int SIM_TILE = 2048;          // output samples of one workgroup of the sample kernel: 256 threads x 8 samples
constexpr int SIM_MAX_K = 9;
constexpr int32_t SIM_Z_OFFSET = 6138;  // 12 x 1023 / 2: the mean of the sum of twelve 10-bit fields

// ranges of the contract
SIM_HD inline bool sim_k_ok(int k) { return k >= 1 && k <= SIM_MAX_K && (k & 1); }
SIM_HD inline bool sim_model_entry_ok(int32_t level_q10, int32_t sd_q10, int32_t dwell_q8)
{
    return level_q10 >= -(1 << 15) && level_q10 <= (1 << 15) && sd_q10 >= 0 && sd_q10 <= (1 << 15) && dwell_q8 >= 256 && dwell_q8 <= (1 << 23);
}
SIM_HD inline bool sim_read_ok(int32_t lead, int32_t lead_level_q10, int32_t lead_sd_q10, int32_t median, int32_t scale_q10)
{
    return lead >= 0 && lead_level_q10 >= -(1 << 15) && lead_level_q10 <= (1 << 15) && lead_sd_q10 >= 0 && lead_sd_q10 <= (1 << 15) &&
           median >= -32768 && median <= 32767 && scale_q10 >= 1 && scale_q10 <= (1 << 26);
}

SIM_HD inline uint32_t sim_mulhi(uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(a, b);
#else
    return (uint32_t)(((uint64_t)a * b) >> 32);
#endif
}

// Philox4x32-10: counter c, key k -> w
SIM_HD inline void sim_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t w[4])
{
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int r = 0; r < 10; r++) {
        const uint32_t hi0 = sim_mulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0, hi1 = sim_mulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    w[0] = c0, w[1] = c1, w[2] = c2, w[3] = c3;
}

// the k-mer of base b of a read of L >= 1 bases (codes 0..3 in pore order, first base most significant); a position outside the read
// takes the nearest end base
SIM_HD inline int32_t sim_kmer(const uint8_t* codes, int32_t L, int32_t b, int k)
{
    const int h = k >> 1;
    int32_t idx = 0;
    for (int j = -h; j <= h; j++) {
        int64_t p = (int64_t)b + j;
        p = p < 0 ? 0 : p > L - 1 ? L - 1 : p;
        idx = (idx << 2) | codes[p];
    }
    return idx;
}

// the dwell of a base: the k-mer's mean dwell (Q8 samples) times the base's scale (Q8) times the quantile w0 picks (Q16 multiples of the mean)
SIM_HD inline int32_t sim_dwell(int32_t dwell_q8, uint32_t scale_q8, const uint32_t* cdf, uint32_t w0)
{
    const int64_t m = ((int64_t)dwell_q8 * (int64_t)scale_q8) >> 8;   // at most 2^23 * 2^12 >> 8
    const int64_t t = cdf[w0 >> 22];                                 // at most 2^20
    const int64_t d = (m * t + ((int64_t)1 << 23)) >> 24;
    return (int32_t)(d < 1 ? 1 : d > 32767 ? 32767 : d);
}

// z = the sum of the twelve 10-bit fields (bits 0-9, 10-19, 20-29 of each word) - 6138.  The low and the high fields of four words are
// summed in place: four values below 2^10 stay below 2^12, and the next field starts ten bits further up
SIM_HD inline int32_t sim_noise_z(const uint32_t w[4])
{
    const uint32_t outer = (w[0] & 0x3FF003FFu) + (w[1] & 0x3FF003FFu) + (w[2] & 0x3FF003FFu) + (w[3] & 0x3FF003FFu);
    const uint32_t mid = ((w[0] >> 10) & 1023u) + ((w[1] >> 10) & 1023u) + ((w[2] >> 10) & 1023u) + ((w[3] >> 10) & 1023u);
    return (int32_t)((outer & 0xFFFFu) + (outer >> 20) + mid) - SIM_Z_OFFSET;
}

// one raw sample: level (the k-mer's level plus the base's shift, or the lead's level) and sd in Q10 z units, z in 1/1024 sigma
SIM_HD inline int16_t sim_raw(int32_t level_q10, int32_t sd_q10, int32_t z, int32_t median, int32_t scale_q10)
{
    const int32_t v = level_q10 + ((sd_q10 * z) >> 10);                                        // |sd z| < 2^15 * 6139: floor by the shift
    const int64_t r = (int64_t)median + (((int64_t)v * scale_q10 + ((int64_t)1 << 19)) >> 20);   // |v| < 2^18, scale <= 2^26
    return (int16_t)(r < -32768 ? -32768 : r > 32767 ? 32767 : r);
}
