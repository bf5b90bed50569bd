// modcall.hip -- per-read modification calls: the rows between two anchors of an existing alignment, re-aligned to the states round a site
// under the canonical model and under an alternative one, by the best path and by the sum over all paths.  DESIGN.md section 31.
//
// Contract (integer arithmetic only, met exactly; include/radian_hip.h, rd_modcall; the rules themselves are modcall_rules.h).  A job is a
// (read, site) pair: n_alt replaced states from base alt_first on, a flank F.  Its window is the states a0 .. a1 = the replaced ones and F
// bases either side, clipped to the read's bases (S <= 63 of them), and the rows first[a0] .. last[a1] of the read's steps (R of them):
//   zq[t]     = ea_quant(raw[r0 + t], m2, d4); c(t, i) = ea_cost(zq[t], state i), state i base a0 + i's k-mer (ref), or the job's entry (alt)
//   V[0][0]   = c(0, 0), every other state starts at 2^30; per hypothesis vit = c + min(stay, adv) and fwd = c + softmin(stay, adv)
//   results   the four values at (R - 1, S - 1)
//
// Kernel, on the context's stream, once per launch (a set of reads whose blocks fit the budget):
//   mc_kernel   one wave per job, four jobs of one read per workgroup.  Lane i holds state i: four values and six constants.  The left
//               neighbour's four values come by DPP (wave_shr:1, lane 0 keeps 2^30).  A tile is 64 rows: lane r loads and quantises row r
//               (the load predicated on the row lying in the window), and the row's zq reaches all lanes by v_readlane with the row counter
//               in a scalar register.  The LSE table sits in LDS, filled before the workgroup's only barrier; a wave with nothing to do
//               leaves after it.  No back-pointers, no per-row store, no workspace beyond the inputs; the results leave by plain vector
//               stores.  No floating point, no atomics, no inline assembly.
// A launch's block in ws_align is staged on the host as one image and goes up in one copy: the job descriptors, the result slots, then
// per read its samples, its steps and its alt entries.  A job's result depends on nothing but its own inputs.
#include "common.h"
#include "budget.h"
#include "modcall_rules.h"
#include "../../include/radian_hip.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace {

struct McCall {
    const int16_t* raw;
    const int64_t* read_off;
    int n_reads;
    const int32_t *m2, *d4;
    const uint8_t* codes;
    const int64_t* ref_off;
    const int32_t *ref_len, *first, *last;
    int k;
    const int32_t* lvl;
    const uint32_t* w;
    const int32_t* bias;
    int n_jobs;
    const int32_t *job_read, *alt_first;
    const int64_t* alt_off;
    const int32_t* alt_lvl;
    const uint32_t* alt_w;
    const int32_t* alt_bias;
    int flank;
    int32_t *status, *n_rows, *n_states, *vit_ref, *vit_alt, *fwd_ref, *fwd_alt;
};

int mc_check_args(const char* who, const McCall& c)
{
    RD_REQUIRE(c.n_reads >= 0 && c.n_jobs >= 0, "%s: negative n_reads or n_jobs", who);
    RD_REQUIRE(mc_flank_ok(c.flank), "%s: flank = %d, not in 0..%d", who, c.flank, MC_MAX_FLANK);
    RD_REQUIRE(sim_k_ok(c.k), "%s: k = %d, not odd and 1..9", who, c.k);
    RD_REQUIRE(c.lvl && c.w && c.bias, "%s: null model table", who);
    const int64_t n_kmers = (int64_t)1 << (2 * c.k);
    for (int64_t i = 0; i < n_kmers; i++)
        RD_REQUIRE(ea_entry_ok(c.lvl[i], c.bias[i]), "%s: model entry %lld (lvl %d, bias %d) is outside |lvl| < 2^14, |bias| <= 256", who, (long long)i,
                   c.lvl[i], c.bias[i]);
    if (c.n_reads) {
        RD_REQUIRE(c.raw && c.read_off && c.m2 && c.d4 && c.ref_off && c.ref_len, "%s: null argument", who);
        RD_REQUIRE(c.read_off[0] >= 0, "%s: negative read offset", who);
    }
    int64_t end = 0;
    for (int r = 0; r < c.n_reads; r++) {
        const int64_t n = c.read_off[r + 1] - c.read_off[r];
        RD_REQUIRE(n >= 0, "%s: read offsets must be non-decreasing (read %d)", who, r);
        RD_REQUIRE(n <= INT32_MAX, "%s: read %d has more than 2^31 - 1 samples", who, r);
        RD_REQUIRE(ea_scale_ok(c.m2[r], c.d4[r]) && c.d4[r] != 0, "%s: read %d: the scale (m2 %d, d4 %d) is outside |m2| <= 2^17, 1 <= d4 <= 2^20", who, r,
                   c.m2[r], c.d4[r]);
        RD_REQUIRE(c.ref_len[r] >= 0 && c.ref_len[r] < (1 << 29), "%s: read %d has %d bases", who, r, c.ref_len[r]);
        RD_REQUIRE(c.ref_off[r] >= end, "%s: base offsets must be non-decreasing and the reads' bases must not overlap (read %d)", who, r);
        end = c.ref_off[r] + c.ref_len[r];
    }
    if (end) {
        RD_REQUIRE(c.codes && c.first && c.last, "%s: null code or step buffer", who);
        for (int r = 0; r < c.n_reads; r++)
            for (int i = 0; i < c.ref_len[r]; i++)
                RD_REQUIRE(c.codes[c.ref_off[r] + i] < 4, "%s: base %d of read %d is %d, not in 0..3", who, i, r, c.codes[c.ref_off[r] + i]);
    }
    if (c.n_jobs == 0) return RD_OK;
    RD_REQUIRE(c.job_read && c.alt_first && c.alt_off && c.alt_lvl && c.alt_w && c.alt_bias, "%s: null job argument", who);
    RD_REQUIRE(c.status && c.n_rows && c.n_states && c.vit_ref && c.vit_alt && c.fwd_ref && c.fwd_alt, "%s: null output", who);
    RD_REQUIRE(c.alt_off[0] >= 0, "%s: negative alt offset", who);
    for (int j = 0; j < c.n_jobs; j++) {
        const int r = c.job_read[j];
        RD_REQUIRE(r >= 0 && r < c.n_reads, "%s: job %d names read %d of %d", who, j, r, c.n_reads);
        const int64_t n_alt = c.alt_off[j + 1] - c.alt_off[j];
        RD_REQUIRE(mc_job_ok(c.alt_first[j], n_alt, c.ref_len[r]), "%s: job %d replaces %lld states from base %d on, of %d bases (1..9 states inside the read)",
                   who, j, (long long)n_alt, c.alt_first[j], c.ref_len[r]);
        for (int64_t i = c.alt_off[j]; i < c.alt_off[j + 1]; i++)
            RD_REQUIRE(ea_entry_ok(c.alt_lvl[i], c.alt_bias[i]), "%s: alt entry %lld of job %d (lvl %d, bias %d) is outside |lvl| < 2^14, |bias| <= 256", who,
                       (long long)(i - c.alt_off[j]), j, c.alt_lvl[i], c.alt_bias[i]);
    }
    return RD_OK;
}

void mc_blank(const McCall& c, int j, int status)
{
    c.status[j] = status;
    c.n_rows[j] = c.n_states[j] = c.vit_ref[j] = c.vit_alt[j] = c.fwd_ref[j] = c.fwd_alt[j] = 0;
}

struct McJob {       // 64 bytes: four of them are the descriptors of a workgroup
    int64_t raw;     // byte offsets into the launch's block: the read's samples,
    int64_t steps;   //   its first[L] followed by last[L],
    int64_t alt;     //   the job's alt entries (EaState)
    int64_t codes;   // the read's base 0 in the code buffer
    int32_t n, L, m2, d4, alt_first, n_alt, out, pad_;   // n_alt == 0: a slot without a job; out: its slot of the results
};
struct McOut {       // 32 bytes
    int32_t status, n_rows, n_states, vit_ref, vit_alt, fwd_ref, fwd_alt, pad_;
};
static_assert(sizeof(McJob) == 64 && sizeof(McOut) == 32 && sizeof(EaState) == 12, "the workspace formula counts these");

size_t mc_read_bytes(int64_t n_samples, int64_t n_bases, int64_t n_jobs, int64_t n_alt)
{
    return align_up((size_t)n_samples * 2, 256) + align_up((size_t)n_bases * 8, 256) + align_up((size_t)n_jobs * sizeof(McJob), 256) +
           align_up((size_t)n_jobs * sizeof(McOut), 256) + align_up((size_t)n_alt * sizeof(EaState), 256);
}

}  // namespace

extern "C" int64_t rd_modcall_workspace_bytes(int64_t n_samples, int64_t n_bases, int64_t n_jobs, int64_t n_alt)
{
    if (n_samples < 0 || n_bases < 0 || n_jobs < 0 || n_alt < 0) return -1;
    return (int64_t)mc_read_bytes(n_samples, n_bases, n_jobs, n_alt);
}

extern "C" int rd_modcall_host(const int16_t* raw, const int64_t* read_off, int n_reads, const int32_t* m2, const int32_t* d4, const uint8_t* codes,
                               const int64_t* ref_off, const int32_t* ref_len, const int32_t* first, const int32_t* last, int k, const int32_t* lvl,
                               const uint32_t* w, const int32_t* bias, int n_jobs, const int32_t* job_read, const int32_t* alt_first,
                               const int64_t* alt_off, const int32_t* alt_lvl, const uint32_t* alt_w, const int32_t* alt_bias, int flank, int32_t* status,
                               int32_t* n_rows, int32_t* n_states, int32_t* vit_ref, int32_t* vit_alt, int32_t* fwd_ref, int32_t* fwd_alt)
{
    const McCall c{raw, read_off, n_reads, m2, d4, codes, ref_off, ref_len, first, last, k, lvl, w, bias, n_jobs, job_read, alt_first, alt_off,
                   alt_lvl, alt_w, alt_bias, flank, status, n_rows, n_states, vit_ref, vit_alt, fwd_ref, fwd_alt};
    if (int rc = mc_check_args("rd_modcall_host", c)) return rc;
    for (int j = 0; j < n_jobs; j++) {
        const int r = job_read[j];
        const int32_t L = ref_len[r], n_alt = (int32_t)(alt_off[j + 1] - alt_off[j]);
        const int64_t o = ref_off[r];
        const McWindow wd = mc_window(first + o, last + o, L, read_off[r + 1] - read_off[r], alt_first[j], n_alt, flank);
        mc_blank(c, j, wd.status);
        if (wd.status != MC_OK) continue;
        EaState ref[MC_MAX_S], alt[MC_MAX_S];
        int32_t V[4][MC_MAX_S];   // vit_ref, vit_alt, fwd_ref, fwd_alt
        for (int32_t i = 0; i < wd.S; i++) {
            const int32_t b = wd.a0 + i, idx = sim_kmer(codes + o, L, b, k), a = b - alt_first[j];
            ref[i] = alt[i] = EaState{lvl[idx], w[idx], bias[idx]};
            if (a >= 0 && a < n_alt) alt[i] = EaState{alt_lvl[alt_off[j] + a], alt_w[alt_off[j] + a], alt_bias[alt_off[j] + a]};
            for (auto& v : V) v[i] = EA_INF;
        }
        const int16_t* x = raw + read_off[r] + wd.r0;
        for (int32_t t = 0; t < wd.R; t++) {
            const int32_t zq = ea_quant(x[t], m2[r], d4[r]);
            for (int32_t i = wd.S - 1; i >= 0; i--) {
                const int32_t cr = ea_cost(zq, ref[i].lvl, ref[i].w, ref[i].bias), ca = ea_cost(zq, alt[i].lvl, alt[i].w, alt[i].bias);
                if (t == 0) {
                    if (i == 0) V[0][0] = V[2][0] = cr, V[1][0] = V[3][0] = ca;
                    continue;
                }
                V[0][i] = mc_vit(cr, V[0][i], i ? V[0][i - 1] : EA_INF);
                V[1][i] = mc_vit(ca, V[1][i], i ? V[1][i - 1] : EA_INF);
                V[2][i] = mc_fwd(cr, V[2][i], i ? V[2][i - 1] : EA_INF, MC_LSE);
                V[3][i] = mc_fwd(ca, V[3][i], i ? V[3][i - 1] : EA_INF, MC_LSE);
            }
        }
        n_rows[j] = wd.R, n_states[j] = wd.S;
        vit_ref[j] = V[0][wd.S - 1], vit_alt[j] = V[1][wd.S - 1], fwd_ref[j] = V[2][wd.S - 1], fwd_alt[j] = V[3][wd.S - 1];
    }
    return RD_OK;
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------------------------------ device half
#include "signal_dev.h"

namespace {

constexpr int MC_WAVES = 4;   // jobs of a workgroup, one wave each: the 256 bytes of descriptors a read's jobs are rounded up to

__device__ const uint8_t mc_lse_dev[MC_LSE_N] = {MC_LSE_LITERAL};

// lane l receives v of lane l - 1, lane 0 keeps `edge` (DPP wave_shr:1 without bound_ctrl: a lane without a source keeps the old value)
__device__ __forceinline__ int32_t lane_shr1(int32_t v, int32_t edge) { return __builtin_amdgcn_update_dpp(edge, v, 0x138, 0xf, 0xf, false); }

__global__ __launch_bounds__(64 * MC_WAVES) void mc_kernel(const McJob* __restrict__ jobs, const uint8_t* __restrict__ codes, const int32_t* __restrict__ lvl_t,
                                                          const uint32_t* __restrict__ w_t, const int32_t* __restrict__ bias_t, int k, int F,
                                                          const uint8_t* __restrict__ ws, McOut* __restrict__ out)
{
    __shared__ uint8_t lse[(MC_LSE_N + 3) & ~3];
    if (threadIdx.x < MC_LSE_N) lse[threadIdx.x] = mc_lse_dev[threadIdx.x];
    __syncthreads();   // the only barrier: before any wave leaves or its lanes part
    const int p = __builtin_amdgcn_readfirstlane(blockIdx.x * MC_WAVES + ((int)threadIdx.x >> 6)), lane = threadIdx.x & 63;   // (the wave's: a scalar)
    const McJob q = jobs[p];
    if (q.n_alt == 0) return;   // a slot of the read's last, partly filled workgroup
    const int32_t* __restrict__ first = (const int32_t*)(ws + q.steps);
    const McWindow wd = mc_window(first, first + q.L, q.L, q.n, q.alt_first, q.n_alt, F);
    if (wd.status != MC_OK) {
        if (lane == 0) out[q.out] = McOut{wd.status, 0, 0, 0, 0, 0, 0, 0};
        return;
    }
    const int S = wd.S, R = wd.R;
    // the lane's state under both hypotheses; a lane past the last state costs nothing and is never read out
    EaState ref{0, 0, 0}, alt{0, 0, 0};
    if (lane < S) {
        const int32_t b = wd.a0 + lane, idx = sim_kmer(codes + q.codes, q.L, b, k), a = b - q.alt_first;
        ref = alt = EaState{lvl_t[idx], w_t[idx], bias_t[idx]};
        if (a >= 0 && a < q.n_alt) alt = ((const EaState*)(ws + q.alt))[a];
    }
    const int16_t* __restrict__ x = (const int16_t*)(ws + q.raw) + wd.r0;
    // a tile: lane r holds row tbase + r.  The load is predicated: the last tile reaches past the window, and past the block for the last read
    int32_t tz = lane < R ? ea_quant(x[lane], q.m2, q.d4) : 0;
    const int z0 = __builtin_amdgcn_readlane(tz, 0);   // (by lane number, before the lanes part)
    int32_t vr = lane == 0 ? ea_cost(z0, ref.lvl, ref.w, ref.bias) : EA_INF, va = lane == 0 ? ea_cost(z0, alt.lvl, alt.w, alt.bias) : EA_INF;
    int32_t fr = vr, fa = va;
    for (int tbase = 0; tbase < R; tbase += 64) {
        const int32_t nz = tbase + 64 + lane < R ? ea_quant(x[tbase + 64 + lane], q.m2, q.d4) : 0;   // the next tile's rows
        const int rows = R - tbase < 64 ? R - tbase : 64;
        for (int r = __builtin_amdgcn_readfirstlane(tbase == 0 ? 1 : 0); r < rows; r++) {   // (row 0 is done)
            const int z = __builtin_amdgcn_readlane(tz, r);
            const int32_t cr = ea_cost(z, ref.lvl, ref.w, ref.bias), ca = ea_cost(z, alt.lvl, alt.w, alt.bias);
            const int32_t lvr = lane_shr1(vr, EA_INF), lva = lane_shr1(va, EA_INF), lfr = lane_shr1(fr, EA_INF), lfa = lane_shr1(fa, EA_INF);
            vr = mc_vit(cr, vr, lvr);
            va = mc_vit(ca, va, lva);
            fr = mc_fwd(cr, fr, lfr, lse);
            fa = mc_fwd(ca, fa, lfa, lse);
        }
        tz = nz;
    }
    if (lane == S - 1) out[q.out] = McOut{MC_OK, R, S, vr, va, fr, fa, 0};
}

}  // namespace

extern "C" int rd_modcall(rd_ctx* ctx, const int16_t* raw, const int64_t* read_off, int n_reads, const int32_t* m2, const int32_t* d4, const uint8_t* codes,
                          const int64_t* ref_off, const int32_t* ref_len, const int32_t* first, const int32_t* last, int k, const int32_t* lvl,
                          const uint32_t* w, const int32_t* bias, int n_jobs, const int32_t* job_read, const int32_t* alt_first, const int64_t* alt_off,
                          const int32_t* alt_lvl, const uint32_t* alt_w, const int32_t* alt_bias, int flank, int64_t budget_bytes, int32_t* status,
                          int32_t* n_rows, int32_t* n_states, int32_t* vit_ref, int32_t* vit_alt, int32_t* fwd_ref, int32_t* fwd_alt)
{
    RD_REQUIRE(ctx, "rd_modcall: null context");
    RD_REQUIRE(budget_bytes >= 0, "rd_modcall: negative budget");
    const McCall c{raw, read_off, n_reads, m2, d4, codes, ref_off, ref_len, first, last, k, lvl, w, bias, n_jobs, job_read, alt_first, alt_off,
                   alt_lvl, alt_w, alt_bias, flank, status, n_rows, n_states, vit_ref, vit_alt, fwd_ref, fwd_alt};
    int rc = mc_check_args("rd_modcall", c);
    if (rc || n_jobs == 0) return rc;
    // the jobs of every read, in the caller's order within a read
    std::vector<int64_t> job0(n_reads + 1, 0), n_alt_of(n_reads, 0);
    for (int j = 0; j < n_jobs; j++) {
        job0[job_read[j] + 1]++;
        n_alt_of[job_read[j]] += alt_off[j + 1] - alt_off[j];
        mc_blank(c, j, MC_TOO_LARGE);   // until its launch has run
    }
    for (int r = 0; r < n_reads; r++) job0[r + 1] += job0[r];
    std::vector<int32_t> by_read(n_jobs);
    {
        std::vector<int64_t> at(job0.begin(), job0.end() - 1);
        for (int j = 0; j < n_jobs; j++) by_read[at[job_read[j]]++] = j;
    }
    const auto read_bytes = [&](int r) { return mc_read_bytes(read_off[r + 1] - read_off[r], ref_len[r], job0[r + 1] - job0[r], n_alt_of[r]); };
    RD_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int64_t n_bases = ref_off[n_reads - 1] + ref_len[n_reads - 1];
    if (ctx->ws_labels.reserve((size_t)n_bases + 16)) return RD_ERR_NOMEM;
    const uint8_t* d_codes = ctx->ws_labels.as<uint8_t>();
    if (n_bases) RD_HIP(hipMemcpyAsync(ctx->ws_labels.p, codes, (size_t)n_bases, hipMemcpyHostToDevice, st));
    KmerTables tab;
    if ((rc = signal_upload_tables(ctx, st, k, lvl, w, bias, 0, &tab))) return rc;
    // the launches: the reads that have jobs, in the caller's order, as many as fit the budget; a read that alone exceeds it is reported
    if ((rc = rd_resolve_budget(&budget_bytes, ctx->ws_align.cap))) return rc;
    const BudgetPlan plan = rd_plan_budget(n_reads, nullptr, budget_bytes, 0, false,
                                           [&](int r, int) { return job0[r + 1] > job0[r] ? (int64_t)read_bytes(r) : (int64_t)-1; }, rd_budget_never_closes);
    if (plan.max_bytes && ctx->ws_align.reserve_exact((size_t)plan.max_bytes, "rd_modcall")) return RD_ERR_NOMEM;
    std::vector<uint8_t> img;
    std::vector<McOut> res;
    for (auto [k0, k1] : plan.launches) {
        const int nb = (int)(k1 - k0);
        const int32_t* members = plan.run.data() + k0;
        // the block: the descriptors of every member (four to a workgroup), the result slots, then per member its samples, steps and entries
        size_t total = 0;
        for (int i = 0; i < nb; i++) total += read_bytes(members[i]);
        img.assign(total, 0);   // (a descriptor slot without a job: n_alt == 0)
        Carve ws(img.data());
        std::vector<McJob*> jobs_of(nb);
        for (int i = 0; i < nb; i++) jobs_of[i] = ws.take<McJob>((size_t)(job0[members[i] + 1] - job0[members[i]]));
        const size_t n_slots = ws.mark() / sizeof(McJob), out_at = ws.mark();
        std::vector<int64_t> out_of(nb);
        for (int i = 0; i < nb; i++) out_of[i] = (ws.take<McOut>((size_t)(job0[members[i] + 1] - job0[members[i]])) - (McOut*)(img.data() + out_at));
        const size_t n_out = (ws.mark() - out_at) / sizeof(McOut);
        for (int i = 0; i < nb; i++) {
            const int r = members[i];
            const int64_t n = read_off[r + 1] - read_off[r], L = ref_len[r], nj = job0[r + 1] - job0[r];
            int16_t* p_raw = ws.take<int16_t>((size_t)n);
            int32_t* p_steps = ws.take<int32_t>(2 * (size_t)L);
            EaState* p_alt = ws.take<EaState>((size_t)n_alt_of[r]);
            if (n) memcpy(p_raw, raw + read_off[r], (size_t)n * 2);
            if (L) memcpy(p_steps, first + ref_off[r], (size_t)L * 4), memcpy(p_steps + L, last + ref_off[r], (size_t)L * 4);
            int64_t a_at = 0;
            for (int64_t jj = 0; jj < nj; jj++) {
                const int j = by_read[job0[r] + jj];
                const int32_t na = (int32_t)(alt_off[j + 1] - alt_off[j]);
                for (int32_t a = 0; a < na; a++) p_alt[a_at + a] = EaState{alt_lvl[alt_off[j] + a], alt_w[alt_off[j] + a], alt_bias[alt_off[j] + a]};
                jobs_of[i][jj] = McJob{(int64_t)((uint8_t*)p_raw - img.data()), (int64_t)((uint8_t*)p_steps - img.data()),
                                       (int64_t)((uint8_t*)(p_alt + a_at) - img.data()), ref_off[r], (int32_t)n, (int32_t)L, m2[r], d4[r], alt_first[j], na,
                                       (int32_t)(out_of[i] + jj), 0};
                a_at += na;
            }
        }
        if ((rc = rd_carve_check("rd_modcall", ws, ctx->ws_align.cap))) return rc;
        if (ws.mark() != total) return rd_carve_check("rd_modcall", Carve(nullptr, std::max(ws.mark(), total)), std::min(ws.mark(), total));
        uint8_t* dws = ctx->ws_align.as<uint8_t>();
        RD_HIP(hipMemcpyAsync(dws, img.data(), total, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(mc_kernel, dim3((unsigned)(n_slots / MC_WAVES)), dim3(64 * MC_WAVES), 0, st, (const McJob*)dws, d_codes, tab.lvl, tab.w, tab.bias, k,
                           flank, (const uint8_t*)dws, (McOut*)(dws + out_at));
        RD_HIP(hipGetLastError());
        res.resize(n_out);
        RD_HIP(hipMemcpyAsync(res.data(), dws + out_at, n_out * sizeof(McOut), hipMemcpyDeviceToHost, st));
        RD_HIP(hipStreamSynchronize(st));
        for (int i = 0; i < nb; i++) {
            const int r = members[i];
            for (int64_t jj = 0; jj < job0[r + 1] - job0[r]; jj++) {
                const int j = by_read[job0[r] + jj];
                const McOut& o = res[(size_t)(out_of[i] + jj)];
                status[j] = o.status, n_rows[j] = o.n_rows, n_states[j] = o.n_states;
                vit_ref[j] = o.vit_ref, vit_alt[j] = o.vit_alt, fwd_ref[j] = o.fwd_ref, fwd_alt[j] = o.fwd_alt;
            }
        }
    }
    if (plan.too_large) {
        const int r = (int)plan.first_too_large;
        rd_set_error("rd_modcall: read %d (%lld samples x %d bases, %lld jobs) needs %lld bytes of workspace, over the budget of %lld; the jobs of %d "
                     "read(s) not done (status RD_MC_TOO_LARGE), the others were", r, (long long)(read_off[r + 1] - read_off[r]), ref_len[r],
                     (long long)(job0[r + 1] - job0[r]), (long long)read_bytes(r), (long long)budget_bytes, (int)plan.too_large);
        return RD_ERR_NOMEM;
    }
    return RD_OK;
}
#endif  // __HIPCC__
