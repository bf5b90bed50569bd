// sim.hip -- direct-RNA signal simulation: raw int16 samples of reads whose sequence is given, with every base's first sample known.
// DESIGN.md section 21.
//
// Contract (integer arithmetic only; include/radian_hip.h, rd_sim_signal; the rules themselves are sim_rules.h).  Read r has bases
// codes[seq_off[r] .. seq_off[r+1]) in pore order, lead[r] samples before its first base, a 64-bit key; the model has a level, an sd and
// a mean dwell per k-mer and 1024 dwell quantiles:
//   dwell     base b: Philox4x32-10 of counter (b, 0, 0, 0) under the read's key -> w0; m = dwell_q8[kmer] * scale_q8 >> 8,
//             t = dwell_cdf[w0 >> 22], d = clamp((m t + 2^23) >> 24, 1, 32767)
//   positions base_first[b] = lead + the dwells before b; n_samples = lead + all dwells
//   sample    s: Philox of counter (s, 1, 0, 0) -> twelve 10-bit fields, z = their sum - 6138; v = level + shift + floor(sd z / 1024) of
//             the base s falls in (the lead's level and sd before the first base); raw = clamp(median + floor((v scale + 2^19) / 2^20))
//
// Kernels, on one stream:
//   sim_dwell_kernel   one thread per base of the launch: the read by a binary search over the launch's base offsets, the k-mer index
//                      with the edge rule, one Philox call, the dwell; it also stores level + shift and sd of the base (8 B)
//   rocprim::exclusive_scan of the dwells, in int64 (a launch may hold more than 2^31 samples)
//   sim_finish_kernel  one thread per base: base_first = scan - the scan at the read's first base + lead; one thread per read: n_samples
//   sim_sample_kernel  one 256-thread workgroup per tile of SIM_TILE = 2048 consecutive samples of one read.  The read is found by a uniform
//                      binary search over the reads' first tiles, the tile's first base by a uniform binary search over the read's
//                      base_first; the base starts inside the tile are staged in LDS (at most SIM_TILE - 1, since every dwell is >= 1; the
//                      rest of the 8 KB holds a sentinel).  A thread finds the base of its first sample by a binary search in LDS, walks
//                      over its 8 samples (one Philox call each; at most one base start per sample) and stores them as one 16-byte vector.
//                      A read's samples start at a multiple of 8 in the launch's buffer, so the store is aligned and the samples past the
//                      read's end that the last vector holds fall into the read's own padding.
// No floating point, no atomics, no inline assembly; every output element has one writer.  A result does not depend on the launch's other reads.
#include "common.h"
#include "budget.h"
#include "sim_rules.h"
#include "../../include/radian_hip.h"

#include <cstring>
#include <vector>

namespace {

// the inputs every rd_sim_* entry point takes
struct SimIn {
    const uint8_t* codes;
    const int64_t* seq_off;
    int n_reads;
    const int16_t* shift;
    const uint16_t* dscale;
    const int32_t *lead, *lead_level, *lead_sd, *median, *scale;
    const uint32_t* key;
    int k;
    const int32_t *level, *sd, *dwell;
    const uint32_t* cdf;
};

int sim_check_args(const char* who, const SimIn& in)
{
    RD_REQUIRE(in.n_reads >= 0, "%s: negative n_reads", who);
    RD_REQUIRE(sim_k_ok(in.k), "%s: k = %d is not an odd number from 1 to 9", who, in.k);
    RD_REQUIRE(in.level && in.sd && in.dwell && in.cdf, "%s: null model table", who);
    const int64_t n_kmers = (int64_t)1 << (2 * in.k);
    for (int64_t i = 0; i < n_kmers; i++)
        RD_REQUIRE(sim_model_entry_ok(in.level[i], in.sd[i], in.dwell[i]),
                   "%s: k-mer %lld of the model is outside its range (|level_q10| <= 2^15, sd_q10 0..2^15, dwell_q8 256..2^23)", who, (long long)i);
    for (int i = 0; i < 1024; i++) {
        RD_REQUIRE(in.cdf[i] <= (1u << 20), "%s: dwell_cdf[%d] is above 2^20", who, i);
        RD_REQUIRE(i == 0 || in.cdf[i] >= in.cdf[i - 1], "%s: dwell_cdf decreases at %d", who, i);
    }
    if (in.n_reads == 0) return RD_OK;
    RD_REQUIRE(in.seq_off && in.lead && in.lead_level && in.lead_sd && in.median && in.scale && in.key, "%s: null argument", who);
    RD_REQUIRE(in.seq_off[0] >= 0, "%s: negative sequence offset", who);
    for (int r = 0; r < in.n_reads; r++) {
        RD_REQUIRE(in.seq_off[r + 1] >= in.seq_off[r], "%s: sequence offsets must be non-decreasing (read %d)", who, r);
        RD_REQUIRE(in.seq_off[r + 1] - in.seq_off[r] <= INT32_MAX, "%s: read %d has more than 2^31 - 1 bases", who, r);
        RD_REQUIRE(sim_read_ok(in.lead[r], in.lead_level[r], in.lead_sd[r], in.median[r], in.scale[r]),
                   "%s: a parameter of read %d is outside its range (lead >= 0, |lead_level_q10| <= 2^15, lead_sd_q10 0..2^15, median an int16, "
                   "scale_q10 1..2^26)", who, r);
    }
    const int64_t b0 = in.seq_off[0], b1 = in.seq_off[in.n_reads];
    RD_REQUIRE(b1 == b0 || in.codes, "%s: null codes", who);
    for (int64_t i = b0; i < b1; i++) RD_REQUIRE(in.codes[i] <= 3, "%s: base %lld has code %d", who, (long long)i, (int)in.codes[i]);
    if (in.dscale)
        for (int64_t i = b0; i < b1; i++)
            RD_REQUIRE(in.dscale[i] >= 1 && in.dscale[i] <= 4096, "%s: dwell_scale_q8 of base %lld is outside 1..4096", who, (long long)i);
    return RD_OK;
}

// raw_off against lengths that are known
int sim_check_raw_off(const char* who, const int64_t* raw_off, const int64_t* len, const int32_t* skip, int n_reads)
{
    for (int r = 0; r < n_reads; r++) {
        if (skip && skip[r]) continue;
        RD_REQUIRE(len[r] <= INT32_MAX, "%s: read %d comes to %lld samples, more than 2^31 - 1", who, r, (long long)len[r]);
        RD_REQUIRE(raw_off[r + 1] - raw_off[r] == len[r], "%s: raw_off gives read %d %lld samples, it has %lld (rd_sim_lengths)", who, r,
                   (long long)(raw_off[r + 1] - raw_off[r]), (long long)len[r]);
    }
    return RD_OK;
}

int sim_check_raw_off_shape(const char* who, const int64_t* raw_off, int n_reads)
{
    RD_REQUIRE(raw_off, "%s: null raw_off", who);
    RD_REQUIRE(raw_off[0] >= 0, "%s: negative raw offset", who);
    for (int r = 0; r < n_reads; r++) {
        RD_REQUIRE(raw_off[r + 1] >= raw_off[r], "%s: raw offsets must be non-decreasing (read %d)", who, r);
        RD_REQUIRE(raw_off[r + 1] - raw_off[r] <= INT32_MAX, "%s: raw_off gives read %d more than 2^31 - 1 samples", who, r);
    }
    return RD_OK;
}

// one read on the host: its dwells into d (L entries), -> n_samples
int64_t sim_host_dwells(const SimIn& in, int r, std::vector<int32_t>& d)
{
    const int64_t s0 = in.seq_off[r];
    const int32_t L = (int32_t)(in.seq_off[r + 1] - s0);
    d.resize(L);
    int64_t n = in.lead[r];
    for (int32_t b = 0; b < L; b++) {
        uint32_t w[4];
        sim_philox((uint32_t)b, 0, 0, 0, in.key[2 * r], in.key[2 * r + 1], w);
        d[b] = sim_dwell(in.dwell[sim_kmer(in.codes + s0, L, b, in.k)], in.dscale ? in.dscale[s0 + b] : 256u, in.cdf, w[0]);
        n += d[b];
    }
    return n;
}

SimIn sim_in(const uint8_t* codes, const int64_t* seq_off, int n_reads, const int16_t* level_shift_q10, const uint16_t* dwell_scale_q8,
             const int32_t* lead, const int32_t* lead_level_q10, const int32_t* lead_sd_q10, const int32_t* median, const int32_t* scale_q10,
             const uint32_t* key, int k, const int32_t* level_q10, const int32_t* sd_q10, const int32_t* dwell_q8, const uint32_t* dwell_cdf)
{
    return SimIn{codes, seq_off, n_reads, level_shift_q10, dwell_scale_q8, lead, lead_level_q10, lead_sd_q10, median, scale_q10, key, k,
                 level_q10, sd_q10, dwell_q8, dwell_cdf};
}

}  // namespace

extern "C" int64_t rd_sim_workspace_bytes(int64_t n_bases, int64_t n_samples)
{
    if (n_bases < 0 || n_samples < 0) return -1;
    return 32 * n_bases + 2 * n_samples + 128;
}

extern "C" int rd_sim_lengths_host(const uint8_t* codes, const int64_t* seq_off, int n_reads, const int16_t* level_shift_q10,
                                   const uint16_t* dwell_scale_q8, const int32_t* lead, const int32_t* lead_level_q10, const int32_t* lead_sd_q10,
                                   const int32_t* median, const int32_t* scale_q10, const uint32_t* key, int k, const int32_t* level_q10,
                                   const int32_t* sd_q10, const int32_t* dwell_q8, const uint32_t* dwell_cdf, int64_t* n_samples)
{
    const SimIn in = sim_in(codes, seq_off, n_reads, level_shift_q10, dwell_scale_q8, lead, lead_level_q10, lead_sd_q10, median, scale_q10, key, k,
                            level_q10, sd_q10, dwell_q8, dwell_cdf);
    const int rc = sim_check_args("rd_sim_lengths_host", in);
    if (rc || n_reads == 0) return rc;
    RD_REQUIRE(n_samples, "rd_sim_lengths_host: null output");
    std::vector<int32_t> d;
    for (int r = 0; r < n_reads; r++) n_samples[r] = sim_host_dwells(in, r, d);
    return RD_OK;
}

extern "C" int rd_sim_signal_host(const uint8_t* codes, const int64_t* seq_off, int n_reads, const int16_t* level_shift_q10,
                                  const uint16_t* dwell_scale_q8, const int32_t* lead, const int32_t* lead_level_q10, const int32_t* lead_sd_q10,
                                  const int32_t* median, const int32_t* scale_q10, const uint32_t* key, int k, const int32_t* level_q10,
                                  const int32_t* sd_q10, const int32_t* dwell_q8, const uint32_t* dwell_cdf, const int64_t* raw_off, int16_t* raw,
                                  int32_t* base_first, int32_t* status)
{
    const char* who = "rd_sim_signal_host";
    const SimIn in = sim_in(codes, seq_off, n_reads, level_shift_q10, dwell_scale_q8, lead, lead_level_q10, lead_sd_q10, median, scale_q10, key, k,
                            level_q10, sd_q10, dwell_q8, dwell_cdf);
    int rc = sim_check_args(who, in);
    if (rc || n_reads == 0) return rc;
    RD_REQUIRE(status, "%s: null status", who);
    if ((rc = sim_check_raw_off_shape(who, raw_off, n_reads))) return rc;
    RD_REQUIRE(raw || raw_off[n_reads] == raw_off[0], "%s: null raw", who);
    std::vector<std::vector<int32_t>> dw(n_reads);
    std::vector<int64_t> len(n_reads);
    for (int r = 0; r < n_reads; r++) len[r] = sim_host_dwells(in, r, dw[r]);
    if ((rc = sim_check_raw_off(who, raw_off, len.data(), nullptr, n_reads))) return rc;
    for (int r = 0; r < n_reads; r++) {
        const int64_t s0 = seq_off[r];
        const int32_t L = (int32_t)dw[r].size();
        int16_t* out = raw + raw_off[r];
        status[r] = len[r] ? SIM_OK : SIM_EMPTY;
        int32_t s = 0;
        for (int32_t b = -1; b < L; b++) {   // b == -1: the lead
            const int32_t n = b < 0 ? lead[r] : dw[r][b];
            int32_t lv = lead_level_q10[r], sdv = lead_sd_q10[r];
            if (b >= 0) {
                const int32_t idx = sim_kmer(codes + s0, L, b, k);
                lv = level_q10[idx] + (level_shift_q10 ? level_shift_q10[s0 + b] : 0);
                sdv = sd_q10[idx];
                if (base_first) base_first[s0 + b] = s;
            }
            for (int32_t i = 0; i < n; i++, s++) {
                uint32_t w[4];
                sim_philox((uint32_t)s, 1, 0, 0, key[2 * r], key[2 * r + 1], w);
                out[s] = sim_raw(lv, sdv, sim_noise_z(w), median[r], scale_q10[r]);
            }
        }
    }
    return RD_OK;
}

// ------------------------------------------------------------------------------------------------------------------ a launch's device block
namespace {

// a read of a launch
struct SimRead {
    int64_t seq0;    // its first base in the launch's base arrays
    int64_t raw0;    // its first sample in the launch's sample buffer, a multiple of 8 (stage B)
    int64_t tile0;   // its first tile among the launch's tiles (stage B)
    int32_t L, lead, lead_level, lead_sd, median, scale, n;   // n: its samples (stage B)
    uint32_t key0, key1;
    int32_t pad_;
};
static_assert(sizeof(SimRead) == 64, "SimRead is copied as 64 bytes");

// The model sits at the head of ws_sim for the whole call.
struct SimWs {
    SimRead* reads;
    uint8_t* codes;
    int16_t* shift;
    uint16_t* dscale;
    int32_t* dwell;
    int64_t* cum;
    int32_t* bfirst;
    int2* lvsd;
    int64_t* len;
    int16_t* raw;
    void* tmp;
    size_t tmp_bytes, total;
};

size_t sim_model_bytes(int k) { return align_up(((size_t)12 << (2 * k)) + 4096, 256); }

// a launch of n reads, B bases and R padded samples behind the model, with tmp_bytes of scan storage.  What stage A leaves for the sample
// kernel (reads, lvsd, bfirst) lies before the samples: its place does not depend on R, which is known only after stage A
void sim_layout(Carve& c, int k, int n, int64_t B, int64_t R, bool with_shift, bool with_dscale, size_t tmp_bytes, SimWs* W)
{
    c.take<char>(sim_model_bytes(k));
    W->reads = c.take<SimRead>((size_t)n, 8);
    W->cum = c.take<int64_t>((size_t)B + 1, 8);
    W->len = c.take<int64_t>((size_t)n, 8);
    W->lvsd = c.take<int2>((size_t)B, 8);
    W->dwell = c.take<int32_t>((size_t)B + 1, 8);
    W->bfirst = c.take<int32_t>((size_t)B, 8);
    W->raw = c.take<int16_t>((size_t)R, 8);
    W->shift = c.take<int16_t>(with_shift ? (size_t)B : 0, 8);
    W->dscale = c.take<uint16_t>(with_dscale ? (size_t)B : 0, 8);
    W->codes = c.take<uint8_t>((size_t)B, 8);
    W->tmp = c.take<char>(tmp_bytes, 8);
    W->tmp_bytes = tmp_bytes;
    W->total = c.at;
}

}  // namespace

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------------------------------ device half
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

namespace {

constexpr int64_t SIM_LAUNCH_OVERHEAD = 12288;   // alignment of a launch's arrays and the scan's temporary storage

struct SimModelDev {
    const int32_t *level, *sd, *dwell;
    const uint32_t* cdf;
    int k;
};

struct ToI64 {
    __host__ __device__ int64_t operator()(int32_t v) const { return (int64_t)v; }
};

// the last read whose first base is at or before g: the read base g belongs to (a read without bases shares its offset with the next one)
__device__ inline int sim_read_of_base(const SimRead* __restrict__ reads, int n_reads, int64_t g)
{
    int lo = 0, hi = n_reads - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (reads[mid].seq0 <= g) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(256) void sim_dwell_kernel(const SimRead* __restrict__ reads, int n_reads, int64_t n_bases, SimModelDev m,
                                                        const uint8_t* __restrict__ codes, const int16_t* __restrict__ shift,
                                                        const uint16_t* __restrict__ dscale, int32_t* __restrict__ dwell, int2* __restrict__ lvsd)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g > n_bases) return;
    if (g == n_bases) {   // the scan's last element: the total
        dwell[g] = 0;
        return;
    }
    const SimRead rd = reads[sim_read_of_base(reads, n_reads, g)];
    const int32_t b = (int32_t)(g - rd.seq0);
    const int32_t idx = sim_kmer(codes + rd.seq0, rd.L, b, m.k);
    uint32_t w[4];
    sim_philox((uint32_t)b, 0, 0, 0, rd.key0, rd.key1, w);
    dwell[g] = sim_dwell(m.dwell[idx], dscale ? dscale[g] : 256u, m.cdf, w[0]);
    lvsd[g] = make_int2(m.level[idx] + (shift ? (int32_t)shift[g] : 0), m.sd[idx]);
}

__global__ __launch_bounds__(256) void sim_finish_kernel(const SimRead* __restrict__ reads, int n_reads, int64_t n_bases,
                                                         const int64_t* __restrict__ cum, int32_t* __restrict__ bfirst, int64_t* __restrict__ len)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g < n_reads) {
        const SimRead rd = reads[g];
        len[g] = (int64_t)rd.lead + cum[rd.seq0 + rd.L] - cum[rd.seq0];
    }
    if (g < n_bases) {
        const SimRead rd = reads[sim_read_of_base(reads, n_reads, g)];
        bfirst[g] = (int32_t)(cum[g] - cum[rd.seq0] + (int64_t)rd.lead);   // (a read beyond 2^31 - 1 samples is refused before this is used)
    }
}

__global__ __launch_bounds__(256) void sim_sample_kernel(const SimRead* __restrict__ reads, int n_reads, const int32_t* __restrict__ bfirst,
                                                         const int2* __restrict__ lvsd, int16_t* __restrict__ raw)
{
    __shared__ int32_t sh_start[SIM_TILE];
    const int tid = threadIdx.x;
    // the read of this tile: the last one whose first tile is at or before it (a read without samples shares its tile with the next one)
    const int64_t t = blockIdx.x;
    int lo = 0, hi = n_reads - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (reads[mid].tile0 <= t) lo = mid;
        else hi = mid - 1;
    }
    const SimRead rd = reads[lo];
    const int32_t s_lo = (int32_t)(t - rd.tile0) * SIM_TILE, s_hi = rd.n - s_lo > SIM_TILE ? s_lo + SIM_TILE : rd.n;
    const int32_t* __restrict__ bf = bfirst + rd.seq0;
    // the tile's first base b0: the last one that starts at or before s_lo; -1: the lead
    int32_t a = 0, e = rd.L;
    while (a < e) {
        const int32_t mid = a + ((e - a) >> 1);
        if (bf[mid] <= s_lo) a = mid + 1;
        else e = mid;
    }
    const int32_t b0 = a - 1;
    // the starts of bases b0 + 1 .. inside the tile; they increase, so a thread stops loading at the first one past the tile
    bool live = true;
    for (int i = tid; i < SIM_TILE; i += 256) {
        const int64_t b = (int64_t)b0 + 1 + i;
        int32_t v = INT32_MAX;
        if (live && b < rd.L) {
            const int32_t f = bf[b];
            if (f < s_hi) v = f;
            else live = false;
        }
        sh_start[i] = v;
    }
    __syncthreads();
    const int32_t s0 = s_lo + tid * 8;
    if (s0 >= s_hi) return;
    // j: the staged starts at or before s0 (at most SIM_TILE - 1 of them are real, so sh_start[SIM_TILE - 1] is the sentinel and j stays below it)
    int j = 0;
#pragma unroll
    for (int step = SIM_TILE / 2; step >= 1; step >>= 1)
        if (sh_start[j + step - 1] <= s0) j += step;
    int32_t next = sh_start[j];
    int32_t lv = rd.lead_level, sdv = rd.lead_sd;
    if (b0 + j >= 0) {
        const int2 p = lvsd[rd.seq0 + b0 + j];
        lv = p.x, sdv = p.y;
    }
    uint32_t out[4];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int32_t s = s0 + i;
        if (next <= s) {   // a base starts here (dwells are >= 1: at most one per sample)
            j++;
            next = sh_start[j];
            const int2 p = lvsd[rd.seq0 + b0 + j];
            lv = p.x, sdv = p.y;
        }
        uint32_t w[4];
        sim_philox((uint32_t)s, 1, 0, 0, rd.key0, rd.key1, w);
        const uint32_t x = (uint16_t)sim_raw(lv, sdv, sim_noise_z(w), rd.median, rd.scale);
        if (i & 1) out[i >> 1] |= x << 16;
        else out[i >> 1] = x;
    }
    *(uint4*)(raw + rd.raw0 + s0) = make_uint4(out[0], out[1], out[2], out[3]);   // (raw0 and s0 are multiples of 8)
}

// the scan's storage asked of rocprim, then sim_layout: dry with base == nullptr (W->total: the bytes)
int sim_carve(int k, int n, int64_t B, int64_t R, bool with_shift, bool with_dscale, hipStream_t st, char* base, SimWs* W)
{
    size_t tb = 0;
    RD_HIP(rocprim::exclusive_scan(nullptr, tb, rocprim::make_transform_iterator((const int32_t*)nullptr, ToI64()), (int64_t*)nullptr, (int64_t)0,
                                   (size_t)B + 1, rocprim::plus<int64_t>(), st));
    Carve c(base);
    sim_layout(c, k, n, B, R, with_shift, with_dscale, tb, W);
    return RD_OK;
}

struct SimLaunch {
    const int32_t* members;
    int n;
    std::vector<SimRead> reads;
    std::vector<int64_t> off;   // the members' first bases in the launch's base arrays, and B
    int64_t B = 0, R = 0, tiles = 0;
};

void sim_describe(const SimIn& in, const int32_t* members, int n, const int64_t* len, SimLaunch* Lc)
{
    Lc->members = members;
    Lc->n = n;
    Lc->reads.resize(n);
    rd_gather_offsets(in.seq_off, members, n, Lc->off);
    Lc->B = Lc->R = Lc->tiles = 0;
    for (int i = 0; i < n; i++) {
        const int r = members[i];
        const int32_t L = (int32_t)(in.seq_off[r + 1] - in.seq_off[r]);
        const int64_t ns = len ? len[r] : 0;
        Lc->reads[i] = SimRead{Lc->B, Lc->R, Lc->tiles, L, in.lead[r], in.lead_level[r], in.lead_sd[r], in.median[r], in.scale[r], (int32_t)ns,
                               in.key[2 * r], in.key[2 * r + 1], 0};
        Lc->B += L;
        Lc->R += (ns + 7) / 8 * 8;
        Lc->tiles += (ns + SIM_TILE - 1) / SIM_TILE;
    }
}

// stage A: the launch's bases to the device, dwells, scan, base_first and the lengths (len_out: one per member)
int sim_stage_a(hipStream_t st, const SimIn& in, const SimModelDev& m, const SimLaunch& Lc, const SimWs& W, int64_t* len_out)
{
    const int n = Lc.n;
    RD_HIP(hipMemcpyAsync(W.reads, Lc.reads.data(), (size_t)n * sizeof(SimRead), hipMemcpyHostToDevice, st));
    int rc = rd_gather_h2d(st, W.codes, in.codes, 1, in.seq_off, Lc.members, n, Lc.off.data());   // (off[i] == reads[i].seq0)
    if (!rc && in.shift) rc = rd_gather_h2d(st, W.shift, in.shift, 2, in.seq_off, Lc.members, n, Lc.off.data());
    if (!rc && in.dscale) rc = rd_gather_h2d(st, W.dscale, in.dscale, 2, in.seq_off, Lc.members, n, Lc.off.data());
    if (rc) return rc;
    const unsigned gb = (unsigned)((Lc.B + 1 + 255) / 256);
    hipLaunchKernelGGL(sim_dwell_kernel, dim3(gb), dim3(256), 0, st, W.reads, n, Lc.B, m, W.codes, in.shift ? W.shift : nullptr,
                       in.dscale ? W.dscale : nullptr, W.dwell, W.lvsd);
    RD_HIP(hipGetLastError());
    size_t tb = W.tmp_bytes;
    RD_HIP(rocprim::exclusive_scan(W.tmp, tb, rocprim::make_transform_iterator((const int32_t*)W.dwell, ToI64()), W.cum, (int64_t)0, (size_t)Lc.B + 1,
                                   rocprim::plus<int64_t>(), st));
    const unsigned gf = (unsigned)((std::max<int64_t>(Lc.B, n) + 255) / 256);
    hipLaunchKernelGGL(sim_finish_kernel, dim3(gf), dim3(256), 0, st, W.reads, n, Lc.B, W.cum, W.bfirst, W.len);
    RD_HIP(hipGetLastError());
    RD_HIP(hipMemcpyAsync(len_out, W.len, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    RD_HIP(hipStreamSynchronize(st));
    return RD_OK;
}

struct SimCall {
    SimIn in;
    BudgetPlan plan;
    SimModelDev model;
    int64_t budget;
    std::vector<int32_t> skip;   // 1: over the budget alone
};

// budget cut, workspace and model upload of a device call; raw_off: the samples the caller expects of every read (null: lengths only)
int sim_begin(rd_ctx* ctx, int64_t budget_bytes, const int64_t* raw_off, SimCall* C)
{
    const SimIn& in = C->in;
    RD_HIP(hipSetDevice(ctx->device));
    int rc;
    if ((rc = rd_resolve_budget(&budget_bytes, ctx->ws_sim.cap))) return rc;   // (this context's block counts as free)
    C->budget = budget_bytes;
    const int64_t overhead = (int64_t)sim_model_bytes(in.k) + SIM_LAUNCH_OVERHEAD;
    const auto need = [&](int r, int) {
        return rd_sim_workspace_bytes(in.seq_off[r + 1] - in.seq_off[r], raw_off ? raw_off[r + 1] - raw_off[r] : 0);
    };
    C->plan = rd_plan_budget(in.n_reads, nullptr, budget_bytes, overhead, false, need, rd_budget_never_closes);
    C->skip.assign(in.n_reads, 1);
    for (int32_t r : C->plan.run) C->skip[r] = 0;
    // one block for the largest launch
    size_t most = sim_model_bytes(in.k);
    SimLaunch Lc;
    SimWs W;
    std::vector<int64_t> claimed(raw_off ? in.n_reads : 0);
    for (size_t r = 0; r < claimed.size(); r++) claimed[r] = raw_off[r + 1] - raw_off[r];
    for (auto [k0, k1] : C->plan.launches) {
        sim_describe(in, C->plan.run.data() + k0, (int)(k1 - k0), raw_off ? claimed.data() : nullptr, &Lc);
        if ((rc = sim_carve(in.k, Lc.n, Lc.B, Lc.R, in.shift != nullptr, in.dscale != nullptr, ctx->stream, nullptr, &W))) return rc;
        most = std::max(most, W.total);
    }
    if (ctx->ws_sim.reserve(most)) return RD_ERR_NOMEM;
    const size_t nk = (size_t)1 << (2 * in.k);
    int32_t* d = ctx->ws_sim.as<int32_t>();
    RD_HIP(hipMemcpyAsync(d, in.level, nk * 4, hipMemcpyHostToDevice, ctx->stream));
    RD_HIP(hipMemcpyAsync(d + nk, in.sd, nk * 4, hipMemcpyHostToDevice, ctx->stream));
    RD_HIP(hipMemcpyAsync(d + 2 * nk, in.dwell, nk * 4, hipMemcpyHostToDevice, ctx->stream));
    RD_HIP(hipMemcpyAsync(d + 3 * nk, in.cdf, 4096, hipMemcpyHostToDevice, ctx->stream));
    C->model = SimModelDev{d, d + nk, d + 2 * nk, (const uint32_t*)(d + 3 * nk), in.k};
    return RD_OK;
}

int sim_too_large_error(const char* who, const SimCall& C, const int64_t* raw_off, const char* what)
{
    const int r = (int)C.plan.first_too_large;
    const int64_t nb = C.in.seq_off[r + 1] - C.in.seq_off[r], ns = raw_off ? raw_off[r + 1] - raw_off[r] : 0;
    rd_set_error("%s: read %d (%lld bases, %lld samples) needs %lld bytes of workspace, over the budget of %lld less %lld per launch; %d read(s) not "
                 "%s (status RD_SIM_TOO_LARGE), the others were", who, r, (long long)nb, (long long)ns, (long long)rd_sim_workspace_bytes(nb, ns),
                 (long long)C.budget, (long long)((int64_t)sim_model_bytes(C.in.k) + SIM_LAUNCH_OVERHEAD), (int)C.plan.too_large, what);
    return RD_ERR_NOMEM;
}

}  // namespace

extern "C" int rd_sim_lengths(rd_ctx* ctx, const uint8_t* codes, const int64_t* seq_off, int n_reads, const int16_t* level_shift_q10,
                              const uint16_t* dwell_scale_q8, const int32_t* lead, const int32_t* lead_level_q10, const int32_t* lead_sd_q10,
                              const int32_t* median, const int32_t* scale_q10, const uint32_t* key, int k, const int32_t* level_q10,
                              const int32_t* sd_q10, const int32_t* dwell_q8, const uint32_t* dwell_cdf, int64_t budget_bytes, int64_t* n_samples)
{
    const char* who = "rd_sim_lengths";
    RD_REQUIRE(ctx, "%s: null context", who);
    RD_REQUIRE(budget_bytes >= 0, "%s: negative budget", who);
    SimCall C;
    C.in = sim_in(codes, seq_off, n_reads, level_shift_q10, dwell_scale_q8, lead, lead_level_q10, lead_sd_q10, median, scale_q10, key, k, level_q10,
                  sd_q10, dwell_q8, dwell_cdf);
    int rc = sim_check_args(who, C.in);
    if (rc || n_reads == 0) return rc;
    RD_REQUIRE(n_samples, "%s: null output", who);
    if ((rc = sim_begin(ctx, budget_bytes, nullptr, &C))) return rc;
    for (int r = 0; r < n_reads; r++) n_samples[r] = -1;   // until its launch has run
    SimLaunch Lc;
    SimWs W;
    std::vector<int64_t> got;
    for (auto [k0, k1] : C.plan.launches) {
        sim_describe(C.in, C.plan.run.data() + k0, (int)(k1 - k0), nullptr, &Lc);
        if ((rc = sim_carve(k, Lc.n, Lc.B, 0, C.in.shift != nullptr, C.in.dscale != nullptr, ctx->stream, (char*)ctx->ws_sim.p, &W))) return rc;
        got.resize(Lc.n);
        if ((rc = sim_stage_a(ctx->stream, C.in, C.model, Lc, W, got.data()))) return rc;
        for (int i = 0; i < Lc.n; i++) n_samples[Lc.members[i]] = got[i];
    }
    if (C.plan.too_large) return sim_too_large_error(who, C, nullptr, "measured (n_samples -1)");
    return RD_OK;
}

extern "C" int rd_sim_signal(rd_ctx* ctx, const uint8_t* codes, const int64_t* seq_off, int n_reads, const int16_t* level_shift_q10,
                             const uint16_t* dwell_scale_q8, const int32_t* lead, const int32_t* lead_level_q10, const int32_t* lead_sd_q10,
                             const int32_t* median, const int32_t* scale_q10, const uint32_t* key, int k, const int32_t* level_q10,
                             const int32_t* sd_q10, const int32_t* dwell_q8, const uint32_t* dwell_cdf, const int64_t* raw_off, int64_t budget_bytes,
                             int16_t* raw, int32_t* base_first, int32_t* status)
{
    const char* who = "rd_sim_signal";
    RD_REQUIRE(ctx, "%s: null context", who);
    RD_REQUIRE(budget_bytes >= 0, "%s: negative budget", who);
    SimCall C;
    C.in = sim_in(codes, seq_off, n_reads, level_shift_q10, dwell_scale_q8, lead, lead_level_q10, lead_sd_q10, median, scale_q10, key, k, level_q10,
                  sd_q10, dwell_q8, dwell_cdf);
    const SimIn& in = C.in;
    int rc = sim_check_args(who, in);
    if (rc || n_reads == 0) return rc;
    RD_REQUIRE(status, "%s: null status", who);
    if ((rc = sim_check_raw_off_shape(who, raw_off, n_reads))) return rc;
    RD_REQUIRE(raw || raw_off[n_reads] == raw_off[0], "%s: null raw", who);
    if ((rc = sim_begin(ctx, budget_bytes, raw_off, &C))) return rc;
    hipStream_t st = ctx->stream;
    const size_t n_launches = C.plan.launches.size();
    SimLaunch Lc;
    SimWs W;
    // the lengths first: raw_off is checked against them before anything is written.  A single launch keeps its stage A for the samples.
    std::vector<int64_t> len(n_reads, 0), got;
    for (auto [k0, k1] : C.plan.launches) {
        sim_describe(in, C.plan.run.data() + k0, (int)(k1 - k0), nullptr, &Lc);
        if ((rc = sim_carve(k, Lc.n, Lc.B, 0, in.shift != nullptr, in.dscale != nullptr, st, (char*)ctx->ws_sim.p, &W))) return rc;
        got.resize(Lc.n);
        if ((rc = sim_stage_a(st, in, C.model, Lc, W, got.data()))) return rc;
        for (int i = 0; i < Lc.n; i++) len[Lc.members[i]] = got[i];
    }
    if ((rc = sim_check_raw_off(who, raw_off, len.data(), C.skip.data(), n_reads))) return rc;
    for (int r = 0; r < n_reads; r++) status[r] = C.skip[r] ? SIM_TOO_LARGE : len[r] ? SIM_OK : SIM_EMPTY;
    std::vector<int16_t> h_raw;
    std::vector<int32_t> h_bf;
    for (auto [k0, k1] : C.plan.launches) {
        sim_describe(in, C.plan.run.data() + k0, (int)(k1 - k0), len.data(), &Lc);
        if ((rc = sim_carve(k, Lc.n, Lc.B, Lc.R, in.shift != nullptr, in.dscale != nullptr, st, (char*)ctx->ws_sim.p, &W))) return rc;
        if (W.total > ctx->ws_sim.cap) {
            rd_set_error("%s: internal: a launch of %lld bytes in a block of %lld", who, (long long)W.total, (long long)ctx->ws_sim.cap);
            return RD_ERR_STATE;
        }
        if (n_launches > 1) {   // (the block held another launch since)
            got.resize(Lc.n);
            if ((rc = sim_stage_a(st, in, C.model, Lc, W, got.data()))) return rc;
        } else {
            RD_HIP(hipMemcpyAsync(W.reads, Lc.reads.data(), (size_t)Lc.n * sizeof(SimRead), hipMemcpyHostToDevice, st));
        }
        if (Lc.tiles) {
            RD_REQUIRE(Lc.tiles <= INT32_MAX, "%s: a launch of %lld tiles; give a budget", who, (long long)Lc.tiles);
            hipLaunchKernelGGL(sim_sample_kernel, dim3((unsigned)Lc.tiles), dim3(256), 0, st, W.reads, Lc.n, W.bfirst, W.lvsd, W.raw);
            RD_HIP(hipGetLastError());
            h_raw.resize(Lc.R);
            RD_HIP(hipMemcpyAsync(h_raw.data(), W.raw, (size_t)Lc.R * 2, hipMemcpyDeviceToHost, st));
        }
        if (base_first && Lc.B) {
            h_bf.resize(Lc.B);
            RD_HIP(hipMemcpyAsync(h_bf.data(), W.bfirst, (size_t)Lc.B * 4, hipMemcpyDeviceToHost, st));
        }
        RD_HIP(hipStreamSynchronize(st));
        for (int i = 0; i < Lc.n; i++) {
            const int r = Lc.members[i];
            const SimRead& rd = Lc.reads[i];
            if (rd.n) memcpy(raw + raw_off[r], h_raw.data() + rd.raw0, (size_t)rd.n * 2);
            if (base_first && rd.L) memcpy(base_first + in.seq_off[r], h_bf.data() + rd.seq0, (size_t)rd.L * 4);
        }
    }
    if (C.plan.too_large) return sim_too_large_error(who, C, raw_off, "simulated");
    return RD_OK;
}
#endif  // __HIPCC__
