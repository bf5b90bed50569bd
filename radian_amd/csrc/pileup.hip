// pileup.hip -- per-site base counts and an error profile from the column-by-column alignment of reads against their spans, on the
// MI355X (rd_pileup_*; rd_pileup_host is the twin in plain loops).  DESIGN.md section 23; the rules are pileup_rules.h.
//
// The accumulator lives in the context from rd_pileup_open to rd_pileup_close: a site table [n_sites][8] uint32 (A C G T other del ins
// starts) and a profile of PILEUP_PROFILE_LEN uint64 (conf, ins_base, kmer, ins_len, del_len).  rd_pileup_add aligns as rd_align_batch
// does (align.hip's routine, align_batch.h) and consumes every launch's M / X / D / I columns where align_tb_kernel left them;
// rd_pileup_add_ops stages columns the caller already has and runs the same kernel on them.
//
// pileup_kernel: one wave per pair, four pairs per workgroup of 256 threads, a fixed grid whose workgroups take the pairs in rounds.  The
// ops go by in chunks of 64 columns, one column per lane:
//   pass 1   ballots of the M / X, ref-consuming and read-consuming columns: the first and last M / X column (the covered interval) and
//            the ref / read characters consumed before and up to them (ref_lo, ref_hi, clip_head, clip_tail), all wave-uniform
//   pass 2   a column's span offset i and read offset j are the chunk totals so far (uniform) plus mbcnt of the chunk's ballots.  The
//            length of the D (I) run that ends in the lane below comes from the D (I) ballot: the highest clear bit below the lane, or,
//            when there is none, the lane index plus the carry -- the length of the run the previous chunks ended with.  The column that
//            follows a run accounts for it.  n_match .. n_del are popcounts of ballots.
//   Site counters: 32-bit global atomic adds whose result nobody takes.  Profile counters: 32-bit LDS atomics into the workgroup's own
//   copy (4259 counters, 17 KB), added to the global profile with 64-bit atomics once per workgroup (nonzero ones only) -- the conf cells
//   would otherwise take one global atomic per aligned base of the run on 30 addresses.  The LDS copy is flushed early once the columns a
//   workgroup has seen since its last flush reach 2^30 (a round adds fewer than 4 * 2^28), so no 32-bit counter wraps.
// Integer adds only: the tables do not depend on the launch order, the budget, the batching or the run.
#include "common.h"
#include "align_batch.h"
#include "pileup_rules.h"
#include "../../include/radian_hip.h"

#include <algorithm>
#include <cstring>
#include <vector>

static_assert(RD_PILEUP_PROFILE_LEN == PILEUP_PROFILE_LEN && RD_PILEUP_CONF == PILEUP_CONF && RD_PILEUP_INS_BASE == PILEUP_INS_BASE &&
              RD_PILEUP_KMER == PILEUP_KMER && RD_PILEUP_INS_LEN == PILEUP_INS_LEN && RD_PILEUP_DEL_LEN == PILEUP_DEL_LEN &&
              RD_PILEUP_RES == PILEUP_RES && RD_PILEUP_OK == PILEUP_OK && RD_PILEUP_NO_BASE == PILEUP_NO_BASE &&
              RD_PILEUP_TOO_LARGE == PILEUP_TOO_LARGE, "include/radian_hip.h and pileup_rules.h agree");

namespace {

// the pairs of a call: lengths below the column bound, spans inside the site table
int pileup_check_pairs(const char* who, const int64_t* ref_off, const int64_t* read_off, int n_pairs, const int64_t* site0, int64_t n_sites)
{
    RD_REQUIRE(ref_off[0] == 0 && read_off[0] == 0, "%s: offsets must start at 0", who);
    for (int p = 0; p < n_pairs; p++) {
        const int64_t n = ref_off[p + 1] - ref_off[p], m = read_off[p + 1] - read_off[p];
        RD_REQUIRE(n >= 0 && m >= 0, "%s: pair %d has a negative length", who, p);
        RD_REQUIRE(n + m < PILEUP_MAX_COLS, "%s: pair %d (%lld x %lld) has 2^28 columns or more", who, p, (long long)n, (long long)m);
        RD_REQUIRE(site0[p] >= 0 && site0[p] + n <= n_sites, "%s: pair %d covers sites %lld .. %lld of %lld", who, p, (long long)site0[p],
                   (long long)(site0[p] + n), (long long)n_sites);
    }
    return RD_OK;
}

// every op is M / X / D / I and the ops of a pair consume exactly its n span and m read characters
int pileup_check_ops(const char* who, const uint8_t* ops, const int64_t* ops_off, const int64_t* ref_off, const int64_t* read_off, int n_pairs)
{
    RD_REQUIRE(ops_off[0] == 0, "%s: offsets must start at 0", who);
    for (int p = 0; p < n_pairs; p++) {
        const int64_t L = ops_off[p + 1] - ops_off[p];
        RD_REQUIRE(L >= 0, "%s: pair %d has a negative number of ops", who, p);
        RD_REQUIRE(L == 0 || ops, "%s: null ops", who);
        int64_t nr = 0, nq = 0;
        for (int64_t k = 0; k < L; k++) {
            const uint8_t o = ops[ops_off[p] + k];
            RD_REQUIRE(pileup_is_op(o), "%s: op %lld of pair %d is 0x%02x, not one of M X D I", who, (long long)k, p, o);
            nr += o != 'I';
            nq += o != 'D';
        }
        RD_REQUIRE(nr == ref_off[p + 1] - ref_off[p] && nq == read_off[p + 1] - read_off[p],
                   "%s: the ops of pair %d consume %lld span and %lld read characters, the pair has %lld and %lld", who, p, (long long)nr,
                   (long long)nq, (long long)(ref_off[p + 1] - ref_off[p]), (long long)(read_off[p + 1] - read_off[p]));
    }
    return RD_OK;
}

int pileup_check_count(const char* who, int64_t added, int n_pairs)
{
    RD_REQUIRE(n_pairs >= 0, "%s: n_pairs %d", who, n_pairs);
    RD_REQUIRE(added + (int64_t)n_pairs <= PILEUP_MAX_PAIRS, "%s: %lld pairs added since rd_pileup_open and %d more: at most 2^31 - 1 (a site's 32-bit counters)",
               who, (long long)added, n_pairs);
    return RD_OK;
}

}  // namespace

extern "C" int rd_pileup_host(const uint8_t* ops, const int64_t* ops_off, const uint8_t* refs, const int64_t* ref_off, const uint8_t* reads,
                              const int64_t* read_off, int n_pairs, const int64_t* site0, int64_t n_sites, uint32_t* sites, uint64_t* profile,
                              int32_t* out)
{
    const char* who = "rd_pileup_host";
    if (int rc = pileup_check_count(who, 0, n_pairs)) return rc;
    RD_REQUIRE(n_sites >= 0 && n_sites <= PILEUP_MAX_SITES, "%s: n_sites = %lld (0 .. 2^30)", who, (long long)n_sites);
    RD_REQUIRE(ops_off && ref_off && read_off && profile && (sites || n_sites == 0) && ((site0 && out) || n_pairs == 0), "%s: null argument", who);
    if (int rc = pileup_check_pairs(who, ref_off, read_off, n_pairs, site0, n_sites)) return rc;
    RD_REQUIRE((ref_off[n_pairs] == 0 || refs) && (read_off[n_pairs] == 0 || reads), "%s: null sequences", who);
    if (int rc = pileup_check_ops(who, ops, ops_off, ref_off, read_off, n_pairs)) return rc;
    for (int p = 0; p < n_pairs; p++)
        pileup_pair_host(ops ? ops + ops_off[p] : nullptr, ops_off[p + 1] - ops_off[p], refs ? refs + ref_off[p] : nullptr, ref_off[p + 1] - ref_off[p],
                         reads ? reads + read_off[p] : nullptr, read_off[p + 1] - read_off[p], site0[p], sites, profile, out + (int64_t)p * PILEUP_RES);
    return RD_OK;
}

// ------------------------------------------------------------------------------------------------------------------ the device blocks
namespace {

// A launch of rd_pileup_add_ops, nb pairs.  It is staged on the host and copied whole, so its blocks are offsets: descriptors | results as
// align_tb_kernel leaves them | site0 | this kernel's results | then every pair's sequences and ops, unrounded (pu_ops_pair)
struct PuOpsAt {
    size_t res, site, out;
};
void pu_ops_layout(Carve& c, int nb, PuOpsAt* o)
{
    c.take<AlnPair>((size_t)nb);
    o->res = c.mark();
    c.take<int32_t>((size_t)nb * ALN_RES);
    o->site = c.mark();
    c.take<int64_t>((size_t)nb);
    o->out = c.mark();
    c.take<int32_t>((size_t)nb * PILEUP_RES);
}
void pu_ops_pair(Carve& c, int64_t n, int64_t m, int64_t L, AlnPair* d)
{
    d->n = (int32_t)n;
    d->m = (int32_t)m;
    d->ref = (int64_t)c.mark();
    d->read = d->ref + n;
    d->ops = d->read + m;
    d->bnd = d->dir = 0;
    c.take<uint8_t>((size_t)(n + m + L), 0, 1);
}

// rd_pileup_read over S sites: flags | positions | the scan's own | then the rows, `need` of them once their number is known (0 before)
struct PuReadWs {
    uint32_t *flag, *pos, *site, *counts;
    void* tmp;
};
void pu_read_layout(Carve& c, int64_t S, size_t scan_bytes, int64_t need, PuReadWs* w)
{
    w->flag = c.take<uint32_t>((size_t)S);
    w->pos = c.take<uint32_t>((size_t)S);
    w->tmp = c.take<char>(scan_bytes);
    w->site = c.take<uint32_t>((size_t)need);
    w->counts = c.take<uint32_t>((size_t)need * PILEUP_CH, 0, 1);
}

}  // namespace

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------------------------------ device half

#include <rocprim/device/device_scan.hpp>

namespace {

constexpr int PU_WAVES = 4;                      // pairs of a workgroup's round
constexpr uint32_t PU_FLUSH_COLS = 1u << 30;     // columns seen since the last flush at which the LDS copy is flushed

__device__ __forceinline__ int pu_below(uint64_t b)   // set bits of b in lanes below this one
{
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
}

// length of the run of set bits of b that ends in lane - 1 (0: lane - 1 is clear); carry: the run the previous chunks ended with
__device__ __forceinline__ int pu_run_before(int lane, uint64_t b, int carry)
{
    if (lane == 0) return carry;
    const uint64_t clear = ~b & (((uint64_t)1 << lane) - 1);
    return clear ? lane - 1 - (63 - __clzll((long long)clear)) : lane + carry;
}

__device__ __forceinline__ int pu_carry(uint64_t b, int carry)   // the run of set bits the chunk ends with
{
    const uint64_t clear = ~b;
    return clear ? __clzll((long long)clear) : carry + 64;
}

__device__ __forceinline__ void pu_site(uint32_t* sites, int64_t s, int ch)
{
    (void)__hip_atomic_fetch_add(&sites[s * PILEUP_CH + ch], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void pu_prof(uint32_t* prof, int k) { (void)__hip_atomic_fetch_add(&prof[k], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// one pair, by one wave
__device__ void pu_pair(const uint8_t* __restrict__ O, int L, const uint8_t* __restrict__ A, int n, const uint8_t* __restrict__ B, int m, int64_t s0,
                        int score, uint32_t* __restrict__ sites, uint32_t* prof, int32_t* __restrict__ out, int lane)
{
    const int nch = (L + 63) >> 6;
    int first = -1, last = -1, ref_lo = 0, ref_hi = 0, rd_lo = 0, rd_hi = 0, racc = 0, qacc = 0;
    for (int c = 0; c < nch; c++) {
        const int k = c * 64 + lane;
        const uint8_t o = k < L ? O[k] : 0;
        const bool mx = o == 'M' || o == 'X';
        const uint64_t bm = __ballot(mx), br = __ballot(mx || o == 'D'), bq = __ballot(mx || o == 'I');
        if (bm) {
            if (first < 0) {
                const int f = __ffsll((long long)bm) - 1;
                const uint64_t lt = ((uint64_t)1 << f) - 1;
                first = c * 64 + f;
                ref_lo = racc + __popcll(br & lt);
                rd_lo = qacc + __popcll(bq & lt);
            }
            const int h = 63 - __clzll((long long)bm);
            const uint64_t le = h == 63 ? ~(uint64_t)0 : ((uint64_t)1 << (h + 1)) - 1;
            last = c * 64 + h;
            ref_hi = racc + __popcll(br & le);
            rd_hi = qacc + __popcll(bq & le);
        }
        racc += __popcll(br);
        qacc += __popcll(bq);
    }
    if (first < 0) {
        if (lane < PILEUP_RES) out[lane] = lane == 0 ? PILEUP_NO_BASE : lane == 1 ? score : lane == 4 ? m : 0;
        return;
    }
    int n_m = 0, n_x = 0, n_i = 0, n_d = 0, carry_d = 0, carry_i = 0;
    racc = qacc = 0;
    for (int c = 0; c <= (last >> 6); c++) {
        const int k = c * 64 + lane;
        const uint8_t o = k < L ? O[k] : 0;
        const bool is_m = o == 'M', is_x = o == 'X', is_d = o == 'D', is_i = o == 'I';
        const uint64_t br = __ballot(is_m || is_x || is_d), bq = __ballot(is_m || is_x || is_i), bd = __ballot(is_d), bi = __ballot(is_i);
        const int i = racc + pu_below(br), j = qacc + pu_below(bq);
        const bool in = k >= first && k <= last;
        const int dlen = pu_run_before(lane, bd, carry_d), ilen = pu_run_before(lane, bi, carry_i);
        if (in) {
            if ((is_m || is_x) && i < n && j < m) {
                const int ca = pileup_code(A[i]), cb = pileup_code(B[j]), km = pileup_kmer(A, n, i);
                pu_site(sites, s0 + i, cb);
                pu_prof(prof, PILEUP_CONF + ca * 6 + cb);
                if (km >= 0) pu_prof(prof, PILEUP_KMER + km * 4 + (is_m ? PILEUP_K_MATCH : PILEUP_K_SUB));
            } else if (is_d && i < n) {
                const int ca = pileup_code(A[i]), km = pileup_kmer(A, n, i);
                pu_site(sites, s0 + i, PILEUP_CH_DEL);
                pu_prof(prof, PILEUP_CONF + ca * 6 + 5);
                if (km >= 0) pu_prof(prof, PILEUP_KMER + km * 4 + PILEUP_K_DEL);
            } else if (is_i && j < m) {
                pu_prof(prof, PILEUP_INS_BASE + pileup_code(B[j]));
            }
            if (k > first && !is_d && dlen > 0) pu_prof(prof, PILEUP_DEL_LEN + pileup_len_bucket(dlen));
            if (k > first && !is_i && ilen > 0 && i >= 1 && i <= n) {   // the run lies between span offsets i - 1 and i
                const int km = pileup_kmer(A, n, i - 1);
                pu_prof(prof, PILEUP_INS_LEN + pileup_len_bucket(ilen));
                pu_site(sites, s0 + i - 1, PILEUP_CH_INS);
                if (km >= 0) pu_prof(prof, PILEUP_KMER + km * 4 + PILEUP_K_INS);
            }
            if (k == first && i < n) pu_site(sites, s0 + i, PILEUP_CH_STARTS);
        }
        n_m += __popcll(__ballot(in && is_m));
        n_x += __popcll(__ballot(in && is_x));
        n_i += __popcll(__ballot(in && is_i));
        n_d += __popcll(__ballot(in && is_d));
        racc += __popcll(br);
        qacc += __popcll(bq);
        carry_d = pu_carry(bd, carry_d);
        carry_i = pu_carry(bi, carry_i);
    }
    if (lane < PILEUP_RES) {
        const int v[PILEUP_RES] = {PILEUP_OK, score, ref_lo, ref_hi, rd_lo, m - rd_hi, n_m, n_x, n_i, n_d};
        int x = 0;
#pragma unroll
        for (int c = 0; c < PILEUP_RES; c++) x = lane == c ? v[c] : x;
        out[lane] = x;
    }
}

__device__ __forceinline__ void pu_flush(uint32_t* prof, unsigned long long* __restrict__ profile)
{
    for (int k = threadIdx.x; k < PILEUP_PROFILE_LEN; k += 64 * PU_WAVES) {
        const uint32_t v = prof[k];
        if (v) {
            (void)__hip_atomic_fetch_add(&profile[k], (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            prof[k] = 0;
        }
    }
}

// slot k: the ops at ws + pairs[k].ops, res[k * ALN_RES + 6] of them (res[.. + 0] the score), the span's first site site0[k]
__global__ __launch_bounds__(64 * PU_WAVES) void pileup_kernel(const AlnPair* __restrict__ pairs, int n_pairs, const uint8_t* __restrict__ ws,
                                                               const int32_t* __restrict__ res, const int64_t* __restrict__ site0,
                                                               uint32_t* __restrict__ sites, unsigned long long* __restrict__ profile,
                                                               int32_t* __restrict__ out)
{
    __shared__ uint32_t s_prof[PILEUP_PROFILE_LEN];
    __shared__ uint32_t s_cols;
    for (int k = threadIdx.x; k < PILEUP_PROFILE_LEN; k += 64 * PU_WAVES) s_prof[k] = 0;
    if (threadIdx.x == 0) s_cols = 0;
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t per_round = (int64_t)gridDim.x * PU_WAVES;
    const int rounds = (int)((n_pairs + per_round - 1) / per_round);
    for (int r = 0; r < rounds; r++) {   // (the same number of rounds for every wave: the barriers below are uniform)
        const int64_t p = (int64_t)r * per_round + (int64_t)blockIdx.x * PU_WAVES + wave;
        if (p < n_pairs) {
            const AlnPair P = pairs[p];
            const int L = res[p * ALN_RES + 6];
            pu_pair(ws + P.ops, L, ws + P.ref, P.n, ws + P.read, P.m, site0[p], res[p * ALN_RES], sites, s_prof, out + p * PILEUP_RES, lane);
            if (lane == 0) atomicAdd(&s_cols, (uint32_t)L);
        }
        __syncthreads();
        const uint32_t cols = s_cols;
        __syncthreads();
        if (cols >= PU_FLUSH_COLS) {
            pu_flush(s_prof, profile);
            if (threadIdx.x == 0) s_cols = 0;
            __syncthreads();
        }
    }
    pu_flush(s_prof, profile);
}

__global__ __launch_bounds__(256) void pileup_flag_kernel(const uint32_t* __restrict__ sites, int64_t n_sites, uint32_t min_depth, uint32_t* __restrict__ flag)
{
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= n_sites) return;
    const uint4 a = ((const uint4*)sites)[2 * s], b = ((const uint4*)sites)[2 * s + 1];
    const uint64_t depth = (uint64_t)a.x + a.y + a.z + a.w + b.x + b.y;
    flag[s] = depth >= min_depth ? 1u : 0u;
}

__global__ __launch_bounds__(256) void pileup_gather_kernel(const uint32_t* __restrict__ sites, int64_t n_sites, const uint32_t* __restrict__ flag,
                                                            const uint32_t* __restrict__ pos, uint32_t* __restrict__ out_site,
                                                            uint32_t* __restrict__ out_counts)
{
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= n_sites || !flag[s]) return;
    const uint32_t q = pos[s];
    out_site[q] = (uint32_t)s;
    ((uint4*)out_counts)[2 * (int64_t)q] = ((const uint4*)sites)[2 * s];
    ((uint4*)out_counts)[2 * (int64_t)q + 1] = ((const uint4*)sites)[2 * s + 1];
}

int pileup_launch(rd_ctx* ctx, hipStream_t st, const AlnPair* d_pairs, int nb, const uint8_t* d_ws, const int32_t* d_res, const int64_t* d_site0,
                  int32_t* d_out)
{
    if (nb == 0) return RD_OK;
    const int grid = std::max(1, std::min((nb + PU_WAVES - 1) / PU_WAVES, 2 * ctx->n_cu));
    hipLaunchKernelGGL(pileup_kernel, dim3(grid), dim3(64 * PU_WAVES), 0, st, d_pairs, nb, d_ws, d_res, d_site0, ctx->pileup_sites.as<uint32_t>(),
                       ctx->pileup_profile.as<unsigned long long>(), d_out);
    RD_HIP(hipGetLastError());
    return RD_OK;
}

constexpr size_t PU_EXTRA = 8 + PILEUP_RES * 4;   // per slot: site0, then the results

struct PileupHook : AlnHook {
    rd_ctx* ctx;
    const int64_t* site0;
    int32_t* out;
    std::vector<int64_t> h_site0;
    std::vector<int32_t> h_out;
    PileupHook(rd_ctx* c, const int64_t* s, int32_t* o) : ctx(c), site0(s), out(o) { extra_pair_bytes = PU_EXTRA; }
    void accepted(int n_pairs) override   // behind the routine's argument checks: a refused call leaves `out` as it was
    {
        for (int64_t k = 0; k < (int64_t)n_pairs * PILEUP_RES; k++) out[k] = k % PILEUP_RES == 0 ? PILEUP_TOO_LARGE : 0;   // until its batch has run
    }
    int launched(const AlnLaunch& l) override
    {
        h_site0.resize(l.n_slots);
        h_out.resize((size_t)l.n_slots * PILEUP_RES);
        for (int k = 0; k < l.n_slots; k++) h_site0[k] = site0[l.slot_pair[k]];
        int64_t* d_site0 = (int64_t*)l.d_extra;
        int32_t* d_out = (int32_t*)(l.d_extra + (size_t)l.n_slots * 8);
        RD_HIP(hipMemcpyAsync(d_site0, h_site0.data(), (size_t)l.n_slots * 8, hipMemcpyHostToDevice, l.stream));
        if (int rc = pileup_launch(ctx, l.stream, l.d_pairs, l.n_slots, l.d_ws, l.d_res, d_site0, d_out)) return rc;
        RD_HIP(hipMemcpyAsync(h_out.data(), d_out, h_out.size() * 4, hipMemcpyDeviceToHost, l.stream));
        return RD_OK;
    }
    int finished(const AlnLaunch& l) override
    {
        for (int k = 0; k < l.n_slots; k++) memcpy(out + (int64_t)l.slot_pair[k] * PILEUP_RES, &h_out[(size_t)k * PILEUP_RES], PILEUP_RES * 4);
        return RD_OK;
    }
};

}  // namespace

extern "C" int rd_pileup_open(rd_ctx* ctx, int64_t n_sites)
{
    RD_REQUIRE(ctx, "rd_pileup_open: null context");
    RD_REQUIRE(n_sites >= 0 && n_sites <= PILEUP_MAX_SITES, "rd_pileup_open: n_sites = %lld (0 .. 2^30)", (long long)n_sites);
    RD_HIP(hipSetDevice(ctx->device));
    ctx->pileup_n_sites = -1;
    if (ctx->pileup_sites.reserve((size_t)n_sites * PILEUP_CH * 4 + 256) || ctx->pileup_profile.reserve((size_t)PILEUP_PROFILE_LEN * 8)) return RD_ERR_NOMEM;
    RD_HIP(hipMemsetAsync(ctx->pileup_sites.p, 0, (size_t)n_sites * PILEUP_CH * 4 + 256, ctx->stream));
    RD_HIP(hipMemsetAsync(ctx->pileup_profile.p, 0, (size_t)PILEUP_PROFILE_LEN * 8, ctx->stream));
    RD_HIP(hipStreamSynchronize(ctx->stream));
    ctx->pileup_n_sites = n_sites;
    ctx->pileup_pairs = 0;
    return RD_OK;
}

extern "C" int rd_pileup_close(rd_ctx* ctx)
{
    RD_REQUIRE(ctx, "rd_pileup_close: null context");
    RD_HIP(hipSetDevice(ctx->device));
    RD_HIP(hipStreamSynchronize(ctx->stream));
    ctx->pileup_sites.release();
    ctx->pileup_profile.release();
    ctx->ws_pileup.release();
    ctx->pileup_n_sites = -1;
    ctx->pileup_pairs = 0;
    return RD_OK;
}

extern "C" int64_t rd_pileup_workspace_bytes(int64_t n, int64_t m)
{
    const int64_t a = rd_align_workspace_bytes(n, m);
    return a < 0 ? a : a + (int64_t)PU_EXTRA + 256;
}

extern "C" int rd_pileup_add(rd_ctx* ctx, const uint8_t* refs, const int64_t* ref_off, const uint8_t* reads, const int64_t* read_off, int n_pairs,
                             const int64_t* site0, int match, int mismatch, int gap_open, int gap_extend, int64_t budget_bytes, int32_t* out,
                             uint8_t* ops_out, const int64_t* ops_off, int32_t* ops_len)
{
    const char* who = "rd_pileup_add";
    RD_REQUIRE(ctx, "%s: null context", who);
    RD_REQUIRE(ctx->pileup_n_sites >= 0, "%s: no pileup is open (rd_pileup_open)", who);
    if (int rc = pileup_check_count(who, ctx->pileup_pairs, n_pairs)) return rc;
    RD_REQUIRE(ref_off && read_off && ((site0 && out) || n_pairs == 0), "%s: null argument", who);
    if (int rc = pileup_check_pairs(who, ref_off, read_off, n_pairs, site0, ctx->pileup_n_sites)) return rc;
    std::vector<int32_t> score((size_t)n_pairs + 1), counts(4 * (size_t)n_pairs + 1), status((size_t)n_pairs + 1);
    PileupHook hook(ctx, site0, out);
    const int rc = rd_align_batch_run(ctx, who, "RD_PILEUP_TOO_LARGE", refs, ref_off, reads, read_off, n_pairs, match, mismatch, gap_open, gap_extend,
                                      budget_bytes, score.data(), counts.data(), status.data(), ops_out, ops_off, ops_len, hook);
    if (rc == RD_OK || rc == RD_ERR_NOMEM) ctx->pileup_pairs += n_pairs;
    return rc;
}

extern "C" int rd_pileup_add_ops(rd_ctx* ctx, const uint8_t* ops, const int64_t* ops_off, const uint8_t* refs, const int64_t* ref_off,
                                 const uint8_t* reads, const int64_t* read_off, int n_pairs, const int64_t* site0, int32_t* out)
{
    const char* who = "rd_pileup_add_ops";
    RD_REQUIRE(ctx, "%s: null context", who);
    RD_REQUIRE(ctx->pileup_n_sites >= 0, "%s: no pileup is open (rd_pileup_open)", who);
    if (int rc = pileup_check_count(who, ctx->pileup_pairs, n_pairs)) return rc;
    RD_REQUIRE(ops_off && ref_off && read_off && ((site0 && out) || n_pairs == 0), "%s: null argument", who);
    if (int rc = pileup_check_pairs(who, ref_off, read_off, n_pairs, site0, ctx->pileup_n_sites)) return rc;
    RD_REQUIRE((ref_off[n_pairs] == 0 || refs) && (read_off[n_pairs] == 0 || reads), "%s: null sequences", who);
    if (int rc = pileup_check_ops(who, ops, ops_off, ref_off, read_off, n_pairs)) return rc;
    RD_HIP(hipSetDevice(ctx->device));
    // launches of consecutive pairs, each under 256 MB of staged bytes (a larger pair goes alone)
    const int64_t cap = (int64_t)256 << 20;
    std::vector<uint8_t> stage;
    for (int p0 = 0; p0 < n_pairs;) {
        int p1 = p0;
        int64_t bytes = 0;
        while (p1 < n_pairs) {
            const int64_t b = 2 * (ops_off[p1 + 1] - ops_off[p1]) + 128;   // n + m <= 2 L
            if (p1 > p0 && bytes + b > cap) break;
            bytes += b;
            p1++;
        }
        const int nb = p1 - p0;
        Carve c;   // (dry: the offsets go into the descriptors and the host's staging buffer)
        PuOpsAt o;
        pu_ops_layout(c, nb, &o);
        std::vector<AlnPair> desc(nb);
        for (int k = 0; k < nb; k++) {
            const int p = p0 + k;
            pu_ops_pair(c, ref_off[p + 1] - ref_off[p], read_off[p + 1] - read_off[p], ops_off[p + 1] - ops_off[p], &desc[k]);
        }
        const size_t at = c.at, res_at = o.res, site_at = o.site, out_at = o.out;
        stage.assign(at, 0);
        memcpy(stage.data(), desc.data(), (size_t)nb * sizeof(AlnPair));
        for (int k = 0; k < nb; k++) {
            const int p = p0 + k;
            const int64_t L = ops_off[p + 1] - ops_off[p];
            ((int32_t*)(stage.data() + res_at))[(size_t)k * ALN_RES + 6] = (int32_t)L;
            ((int64_t*)(stage.data() + site_at))[k] = site0[p];
            if (desc[k].n) memcpy(stage.data() + desc[k].ref, refs + ref_off[p], desc[k].n);
            if (desc[k].m) memcpy(stage.data() + desc[k].read, reads + read_off[p], desc[k].m);
            if (L) memcpy(stage.data() + desc[k].ops, ops + ops_off[p], (size_t)L);
        }
        if (ctx->ws_pileup.reserve(at)) return RD_ERR_NOMEM;
        uint8_t* dws = ctx->ws_pileup.as<uint8_t>();
        RD_HIP(hipMemcpyAsync(dws, stage.data(), at, hipMemcpyHostToDevice, ctx->stream));
        if (int rc = pileup_launch(ctx, ctx->stream, (const AlnPair*)dws, nb, dws, (const int32_t*)(dws + res_at), (const int64_t*)(dws + site_at),
                                   (int32_t*)(dws + out_at)))
            return rc;
        RD_HIP(hipMemcpyAsync(out + (int64_t)p0 * PILEUP_RES, dws + out_at, (size_t)nb * PILEUP_RES * 4, hipMemcpyDeviceToHost, ctx->stream));
        RD_HIP(hipStreamSynchronize(ctx->stream));
        p0 = p1;
    }
    ctx->pileup_pairs += n_pairs;
    return RD_OK;
}

extern "C" int rd_pileup_read(rd_ctx* ctx, uint32_t min_depth, int64_t capacity, uint32_t* site, uint32_t* counts, uint64_t* profile, int64_t* n_out)
{
    const char* who = "rd_pileup_read";
    RD_REQUIRE(ctx && n_out, "%s: null argument", who);
    RD_REQUIRE(ctx->pileup_n_sites >= 0, "%s: no pileup is open (rd_pileup_open)", who);
    RD_REQUIRE(min_depth >= 1, "%s: min_depth 0 (at least 1: a site nobody covers is never returned)", who);
    RD_REQUIRE(capacity >= 0 && ((site && counts) || capacity == 0), "%s: capacity %lld with null outputs", who, (long long)capacity);
    RD_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int64_t S = ctx->pileup_n_sites;
    *n_out = 0;
    if (profile) RD_HIP(hipMemcpyAsync(profile, ctx->pileup_profile.p, (size_t)PILEUP_PROFILE_LEN * 8, hipMemcpyDeviceToHost, st));
    RD_HIP(hipStreamSynchronize(st));
    if (S == 0) return RD_OK;
    size_t scan_bytes = 0;
    RD_HIP(rocprim::exclusive_scan(nullptr, scan_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)S, rocprim::plus<uint32_t>(), st));
    PuReadWs w;
    if (rd_carve(ctx->ws_pileup, [&](Carve& c) { pu_read_layout(c, S, scan_bytes, 0, &w); })) return RD_ERR_NOMEM;
    const unsigned grid = (unsigned)((S + 255) / 256);
    hipLaunchKernelGGL(pileup_flag_kernel, dim3(grid), dim3(256), 0, st, ctx->pileup_sites.as<uint32_t>(), S, min_depth, w.flag);
    RD_HIP(hipGetLastError());
    RD_HIP(rocprim::exclusive_scan(w.tmp, scan_bytes, w.flag, w.pos, 0u, (size_t)S, rocprim::plus<uint32_t>(), st));
    uint32_t tail[2] = {0, 0};
    RD_HIP(hipMemcpyAsync(&tail[0], w.flag + (S - 1), 4, hipMemcpyDeviceToHost, st));
    RD_HIP(hipMemcpyAsync(&tail[1], w.pos + (S - 1), 4, hipMemcpyDeviceToHost, st));
    RD_HIP(hipStreamSynchronize(st));
    const int64_t need = (int64_t)tail[0] + tail[1];
    *n_out = need;
    RD_REQUIRE(capacity >= need, "%s: %lld sites at depth %u or more, the outputs hold %lld", who, (long long)need, min_depth, (long long)capacity);
    if (need == 0) return RD_OK;
    // (growing the workspace would drop the flags: the rows get a block of their own size only when the first one is too small)
    const size_t cap0 = ctx->ws_pileup.cap;
    if (rd_carve(ctx->ws_pileup, [&](Carve& c) { pu_read_layout(c, S, scan_bytes, need, &w); })) return RD_ERR_NOMEM;
    if (ctx->ws_pileup.cap != cap0) {
        hipLaunchKernelGGL(pileup_flag_kernel, dim3(grid), dim3(256), 0, st, ctx->pileup_sites.as<uint32_t>(), S, min_depth, w.flag);
        RD_HIP(hipGetLastError());
        RD_HIP(rocprim::exclusive_scan(w.tmp, scan_bytes, w.flag, w.pos, 0u, (size_t)S, rocprim::plus<uint32_t>(), st));
    }
    hipLaunchKernelGGL(pileup_gather_kernel, dim3(grid), dim3(256), 0, st, ctx->pileup_sites.as<uint32_t>(), S, w.flag, w.pos, w.site, w.counts);
    RD_HIP(hipGetLastError());
    RD_HIP(hipMemcpyAsync(site, w.site, (size_t)need * 4, hipMemcpyDeviceToHost, st));
    RD_HIP(hipMemcpyAsync(counts, w.counts, (size_t)need * PILEUP_CH * 4, hipMemcpyDeviceToHost, st));
    RD_HIP(hipStreamSynchronize(st));
    return RD_OK;
}
#endif  // __HIPCC__
