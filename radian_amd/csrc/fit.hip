// fit.hip -- label windows for training shards (radian_amd/label_build.py): fitting alignment of very many short queries (a window's
// basecall, 1..1024 labels) against long references (the read's reference sequence, 1-20 kb), on the MI355X.
//
// Fitting = query-global, reference-local: the whole query is aligned, the reference before and after the span it covers is free.
// Gotoh's three states, int32, reference = rows i (0..n), query = columns j (0..m), a gap of length L costs open + (L-1) * extend:
//   H[i][0] = 0                                  H[0][j] = F[0][j] = open + (j-1) * extend  (j >= 1)       E[i][0] = F[i][0] = E[0][j] = -inf
//   E[i][j] = max(H[i-1][j] + open, E[i-1][j] + extend)         deletion  (consumes a reference base)
//   F[i][j] = max(H[i][j-1] + open, F[i][j-1] + extend)         insertion (consumes a query base)
//   H[i][j] = max(H[i-1][j-1] + s(r_i, q_j), E[i][j], F[i][j])
//   score = max_i H[i][m], ref_end = the smallest such i; the traceback from (ref_end, m) has align.hip's fixed preference (diagonal,
//   then E, then F; inside a gap run extend before close) and ends at column 0 in row ref_start.
// Codes are bytes: queries 0..3, references 0..4; code 4 (any letter that is not A C G T) equals nothing, itself included.
//
// No direction bits and no traceback kernel: the preference makes the traceback's path from every (cell, state) unique, so what the
// traceback would find -- the row it ends in and its matches and substitutions -- is carried forward beside each of H, E and F as two
// ints (start row; n_match | n_sub << 16, both <= m <= 1024) and selected with the same comparisons that select the score.  Insertions and
// deletions follow from the path's shape: n_ins = m - n_match - n_sub, n_del = (ref_end - ref_start) - n_match - n_sub.  The kernel needs
// no per-cell memory at all, which is what lets a million windows go in one launch.
//
// Shape (fit_kernel<B>): the QUERY lies on the lanes, B columns per lane in registers, and the wave sweeps down the reference with a skew
// of one row per lane: at step t lane s of a query works on row t - s + 1, its B cells from left to right (the F chain is serial inside
// the lane; E and the diagonal come from the lane's own registers of the row above).  H and F of the column to the left of a lane's block,
// their carried ints and the reference byte come from lane s - 1's previous step with DPP wave_shr:1.  A query takes a GROUP of G lanes
// (8, 16, 32 or 64, G * B >= m), so a wave holds 64 / G queries, each against its own reference: the first lane of a group takes the
// boundary column (H = 0, start = the row) in place of the shifted values and reads its reference four bytes at a time, one word ahead.
// No LDS, no atomics.  A 30-label query takes 16 lanes of B = 2 (94 % of them useful) where one wave of 64 reference rows per pair would
// keep under a third of its steps; the sweep's n + G - 1 steps cost G - 1 rows of fill, under 2 % at n = 1.5 kb.
#include "common.h"
#include "budget.h"
#include "../../include/radian_hip.h"

#include <algorithm>
#include <cstring>
#include <numeric>

namespace {

constexpr int FIT_NEG = -(1 << 30);
constexpr int FIT_RES = 8;   // per-query result ints: score, ref_start, ref_end, n_match, n_sub, n_ins, n_del, (pad)
constexpr int FIT_MAX_M = 1024;

struct FitScores {
    int match, mismatch, open, extend;
};

struct FitQuery {
    int64_t ref;     // byte offset of the reference in the workspace (4-aligned, padded to a multiple of 4)
    int64_t query;   // byte offset of the query
    int32_t n, m;
    int32_t slot;    // result slot (the query's index in the batch)
    int32_t pad;
};

// lane l receives v of lane l - 1 (DPP wave_shr:1, bound_ctrl off: lane 0 keeps `v`, a group's first lane never uses the result)
__device__ __forceinline__ int fit_shr1(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xf, 0xf, false); }

template <int B>
__global__ __launch_bounds__(64) void fit_kernel(const FitQuery* __restrict__ qs, int n_q, int G, const uint8_t* __restrict__ ws,
                                                 int32_t* __restrict__ res, FitScores sc)
{
    const int lane = threadIdx.x;
    const int s = lane & (G - 1);                                   // lane of the group
    const int qi = blockIdx.x * (64 / G) + lane / G;                // the group's query; groups past the last one idle
    const bool have = qi < n_q;
    const FitQuery Q = qs[have ? qi : n_q - 1];
    const int n = have ? Q.n : 0, m = Q.m;
    const uint8_t* R = ws + Q.ref;
    const uint8_t* q = ws + Q.query;
    const bool lead = s == 0;

    // row 0 of the lane's columns j = s * B + k + 1; columns past m hold a byte no reference code equals and feed nobody
    int qb[B], Hc[B], HS[B], HC[B], Ec[B], ES[B], EC[B];
#pragma unroll
    for (int k = 0; k < B; k++) {
        const int j = s * B + k + 1;
        qb[k] = j <= m ? q[j - 1] : 0xff;
        Hc[k] = sc.open + (j - 1) * sc.extend;
        HS[k] = 0;
        HC[k] = 0;
        Ec[k] = FIT_NEG;
        ES[k] = 0;
        EC[k] = 0;
    }
    const int kl = s == (m - 1) / B ? (m - 1) % B : -1;             // the lane and register that hold column m
    int best = sc.open + (m - 1) * sc.extend, bestEnd = 0, bestS = 0, bestC = 0;   // H[0][m]: m insertions
    // what the lane handed to its right neighbour after its last step, and what it took from the left at that step (the next diagonal)
    int oH = 0, oHS = 0, oHC = 0, oF = FIT_NEG, oFS = 0, oFC = 0, orb = 0;
    int pH = lead ? 0 : sc.open + (s * B - 1) * sc.extend, pHS = 0, pHC = 0;       // H[0][s * B]
    uint32_t cur = 0, nxt = 0;
    if (lead && n > 0) nxt = *(const uint32_t*)R;

    // steps of the wave: its longest group's n + (lanes that hold columns) - 1
    int steps = n > 0 ? n + (m + B - 1) / B - 1 : 0;
    for (int g = 0; g < 64; g += G) steps = max(steps, __builtin_amdgcn_readlane(steps, g));
    steps = __builtin_amdgcn_readfirstlane(steps);

    for (int t = 0; t < steps; t++) {
        const int i = t - s + 1;
        if (lead && (t & 3) == 0) {
            cur = nxt;
            if (t + 4 < n) nxt = *(const uint32_t*)(R + t + 4);
        }
        int hl = fit_shr1(oH), hlS = fit_shr1(oHS), hlC = fit_shr1(oHC);
        int fl = fit_shr1(oF), flS = fit_shr1(oFS), flC = fit_shr1(oFC);
        int rb = fit_shr1(orb);
        if (lead) {
            hl = 0;
            hlS = i;
            hlC = 0;
            fl = FIT_NEG;
            rb = (cur >> (8 * (t & 3))) & 0xff;
        }
        orb = rb;
        if (i >= 1 && i <= n) {
            int dg = pH, dgS = pHS, dgC = pHC;
            pH = hl;
            pHS = hlS;
            pHC = hlC;
            int selH = FIT_NEG, selS = 0, selC = 0;
#pragma unroll
            for (int k = 0; k < B; k++) {
                const int up = Hc[k], upS = HS[k], upC = HC[k];
                const int eo = up + sc.open, ee = Ec[k] + sc.extend;
                const bool eext = ee >= eo;                         // inside a gap run extend before close
                const int en = max(eo, ee), enS = eext ? ES[k] : upS, enC = eext ? EC[k] : upC;
                const int fo = hl + sc.open, fe = fl + sc.extend;
                const bool fext = fe >= fo;
                const int fn = max(fo, fe), fnS = fext ? flS : hlS, fnC = fext ? flC : hlC;
                const bool eq = rb == qb[k];
                int hn = dg + (eq ? sc.match : sc.mismatch), hS = dgS, hC = dgC + (eq ? 1 : 0x10000);
                if (en > hn) {
                    hn = en;
                    hS = enS;
                    hC = enC;
                }
                if (fn > hn) {
                    hn = fn;
                    hS = fnS;
                    hC = fnC;
                }
                dg = up;
                dgS = upS;
                dgC = upC;
                Hc[k] = hn;
                HS[k] = hS;
                HC[k] = hC;
                Ec[k] = en;
                ES[k] = enS;
                EC[k] = enC;
                hl = hn;
                hlS = hS;
                hlC = hC;
                fl = fn;
                flS = fnS;
                flC = fnC;
                if (k == kl) {
                    selH = hn;
                    selS = hS;
                    selC = hC;
                }
            }
            oH = hl;
            oHS = hlS;
            oHC = hlC;
            oF = fl;
            oFS = flS;
            oFC = flC;
            if (kl >= 0 && selH > best) {   // rows ascend: the smallest row that attains the maximum stays
                best = selH;
                bestEnd = i;
                bestS = selS;
                bestC = selC;
            }
        }
    }
    if (have && kl >= 0) {
        const int nm = bestC & 0xffff, ns = bestC >> 16;
        int32_t* r = res + (int64_t)Q.slot * FIT_RES;
        r[0] = best;
        r[1] = bestS;
        r[2] = bestEnd;
        r[3] = nm;
        r[4] = ns;
        r[5] = m - nm - ns;
        r[6] = bestEnd - bestS - nm - ns;
        r[7] = 0;
    }
}

// launch class of a query: columns per lane B and lanes per group G, the smallest G * B >= m of this list
struct FitClass {
    int B, G;
};
constexpr FitClass kFitClasses[] = {{2, 8}, {2, 16}, {2, 32}, {2, 64}, {4, 64}, {8, 64}, {16, 64}};
constexpr int FIT_NCLASS = sizeof kFitClasses / sizeof kFitClasses[0];

int fit_class(int m)
{
    for (int c = 0; c < FIT_NCLASS; c++)
        if (m <= kFitClasses[c].B * kFitClasses[c].G) return c;
    return -1;
}

constexpr size_t FIT_QUERY_FIXED = sizeof(FitQuery) + FIT_RES * 4;   // descriptor + result of a query
constexpr size_t FIT_BATCH_BYTES = 1024;                             // alignment slack of a batch's regions
size_t fit_ref_bytes(int64_t n) { return align_up((size_t)std::max<int64_t>(n, 1), 4); }
size_t fit_query_bytes(int64_t m) { return FIT_QUERY_FIXED + (size_t)m; }

}  // namespace

extern "C" int rd_fit_batch(rd_ctx* ctx, const uint8_t* refs, const int64_t* ref_off, int64_t n_refs, const uint8_t* queries,
                            const int64_t* query_off, const int32_t* query_ref, int64_t n_queries, int match, int mismatch, int gap_open,
                            int gap_extend, int64_t budget_bytes, int32_t* score, int32_t* ref_start, int32_t* ref_end, int32_t* counts,
                            int32_t* status)
{
    RD_REQUIRE(ctx && ref_off && query_off && score && ref_start && ref_end && counts && status, "rd_fit_batch: null argument");
    RD_REQUIRE(n_refs >= 0 && n_queries >= 0 && n_queries < (1ll << 31) && n_refs < (1ll << 31), "rd_fit_batch: %lld references, %lld queries",
               (long long)n_refs, (long long)n_queries);
    RD_REQUIRE(query_ref || n_queries == 0, "rd_fit_batch: null query_ref");
    RD_REQUIRE(budget_bytes >= 0, "rd_fit_batch: negative budget");
    const int lim = 1 << 16;
    RD_REQUIRE(abs(match) < lim && abs(mismatch) < lim && abs(gap_open) < lim && abs(gap_extend) < lim, "rd_fit_batch: score out of range");
    // with open > extend the recurrence closes a gap and reopens it in the next column: its optimum is not the stated gap cost
    RD_REQUIRE(gap_open <= gap_extend, "rd_fit_batch: gap_open %d is above gap_extend %d (gap_open <= gap_extend is required: otherwise adjacent "
               "gaps reopen and the score is not open + (L-1) * extend per gap)", gap_open, gap_extend);
    RD_REQUIRE(ref_off[0] == 0 && query_off[0] == 0, "rd_fit_batch: offsets must start at 0");
    const int64_t smax = std::max(std::max(abs(match), abs(mismatch)), std::max(abs(gap_open), abs(gap_extend)));
    for (int64_t r = 0; r < n_refs; r++) {
        const int64_t n = ref_off[r + 1] - ref_off[r];
        // scores stay far from FIT_NEG: |H| <= smax * (n + m + 1)
        RD_REQUIRE(n >= 0 && n < (1 << 30) && smax * (n + FIT_MAX_M + 1) < (1 << 28), "rd_fit_batch: reference %lld (%lld codes) is negative or too long for int32 scores",
                   (long long)r, (long long)n);
    }
    RD_REQUIRE(ref_off[n_refs] == 0 || refs, "rd_fit_batch: null refs");
    RD_REQUIRE(query_off[n_queries] == 0 || queries, "rd_fit_batch: null queries");
    for (int64_t k = 0; k < ref_off[n_refs]; k++) RD_REQUIRE(refs[k] <= 4, "rd_fit_batch: reference code %d at byte %lld (codes are 0..4)", refs[k], (long long)k);
    for (int64_t k = 0; k < query_off[n_queries]; k++)
        RD_REQUIRE(queries[k] <= 3, "rd_fit_batch: query code %d at byte %lld (codes are 0..3)", queries[k], (long long)k);
    for (int64_t p = 0; p < n_queries; p++) {
        const int64_t m = query_off[p + 1] - query_off[p];
        RD_REQUIRE(m >= 0 && m <= FIT_MAX_M, "rd_fit_batch: query %lld has %lld labels (0..%d)", (long long)p, (long long)m, FIT_MAX_M);
        RD_REQUIRE(query_ref[p] >= 0 && query_ref[p] < n_refs, "rd_fit_batch: query %lld names reference %d of %lld", (long long)p, query_ref[p],
                   (long long)n_refs);
    }
    RD_HIP(hipSetDevice(ctx->device));
    if (int rc = rd_resolve_budget(&budget_bytes, ctx->ws_align.cap)) return rc;
    // queries in the order of their references (stable), so that a reference is uploaded once per batch and the groups of a wave sweep
    // references of one length; batches are cut where the references and queries gathered so far would pass the budget
    std::vector<int32_t> sorted((size_t)n_queries);
    std::iota(sorted.begin(), sorted.end(), 0);
    std::stable_sort(sorted.begin(), sorted.end(), [&](int32_t x, int32_t y) { return query_ref[x] < query_ref[y]; });
    // a query pays for its reference at the head of a batch and wherever the query before it names another one; empty queries take no part
    const BudgetPlan plan = rd_plan_budget(n_queries, sorted.data(), budget_bytes, (int64_t)FIT_BATCH_BYTES, false,
                                           [&](int32_t p, int32_t prev) -> int64_t {
                                               const int32_t r = query_ref[p];
                                               if (query_off[p + 1] == query_off[p]) return -1;
                                               const size_t rb = prev >= 0 && query_ref[prev] == r ? 0 : fit_ref_bytes(ref_off[r + 1] - ref_off[r]);
                                               return (int64_t)(fit_query_bytes(query_off[p + 1] - query_off[p]) + rb);
                                           },
                                           rd_budget_never_closes);
    const std::vector<int32_t>& order = plan.run;
    const int64_t too_large = plan.too_large, first_too_large = plan.first_too_large;
    for (int64_t p = 0; p < n_queries; p++) {
        score[p] = ref_start[p] = ref_end[p] = 0;
        for (int c = 0; c < 4; c++) counts[4 * p + c] = 0;
        status[p] = query_off[p + 1] == query_off[p] ? RD_FIT_EMPTY : RD_FIT_TOO_LARGE;   // until its batch has run
    }
    if (ctx->ws_align.reserve_exact((size_t)plan.max_bytes, "rd_fit_batch")) return RD_ERR_NOMEM;
    const FitScores sc{match, mismatch, gap_open, gap_extend};
    std::vector<uint8_t> stage;
    std::vector<FitQuery> desc;
    std::vector<int32_t> res;
    for (auto [k0, k1] : plan.launches) {
        const size_t nb = (size_t)(k1 - k0);
        // layout: descriptors (sorted by class) | results | references, 4-aligned each | queries
        Carve ws;   // (dry: the descriptors hold offsets into ws_align; the whole block is staged on the host and copied)
        ws.take<FitQuery>(nb);
        const size_t res_at = ws.mark();
        ws.take<int32_t>(nb * FIT_RES);
        desc.resize(nb);
        int32_t cur_ref = -1;
        int64_t cur_ref_at = 0;
        std::vector<std::pair<int32_t, int64_t>> ref_at;   // the batch's references and where they go
        for (size_t k = 0; k < nb; k++) {
            const int32_t p = order[k0 + k], r = query_ref[p];
            if (r != cur_ref) {
                cur_ref = r;
                cur_ref_at = (int64_t)ws.mark();
                ref_at.push_back({r, cur_ref_at});
                ws.take<uint8_t>(fit_ref_bytes(ref_off[r + 1] - ref_off[r]), 0, 1);
            }
            FitQuery& d = desc[k];
            d.ref = cur_ref_at;
            d.n = (int32_t)(ref_off[r + 1] - ref_off[r]);
            d.m = (int32_t)(query_off[p + 1] - query_off[p]);
            d.slot = (int32_t)k;
            d.pad = 0;
        }
        for (size_t k = 0; k < nb; k++) {
            desc[k].query = (int64_t)ws.mark();
            ws.take<uint8_t>((size_t)desc[k].m, 0, 1);
        }
        const size_t up_bytes = ws.mark();
        if (int rc = rd_carve_check("rd_fit_batch", ws, ctx->ws_align.cap)) return rc;
        stage.assign(up_bytes, 0);
        for (auto [r, where] : ref_at)
            if (ref_off[r + 1] > ref_off[r]) memcpy(stage.data() + where, refs + ref_off[r], (size_t)(ref_off[r + 1] - ref_off[r]));
        for (size_t k = 0; k < nb; k++) memcpy(stage.data() + desc[k].query, queries + query_off[order[k0 + k]], (size_t)desc[k].m);
        // one launch per class: the descriptors of a class lie together, in reference order
        std::stable_sort(desc.begin(), desc.end(), [](const FitQuery& a, const FitQuery& b) { return fit_class(a.m) < fit_class(b.m); });
        memcpy(stage.data(), desc.data(), nb * sizeof(FitQuery));
        uint8_t* dws = ctx->ws_align.as<uint8_t>();
        RD_HIP(hipMemcpyAsync(dws, stage.data(), up_bytes, hipMemcpyHostToDevice, ctx->stream));
        int32_t* dres = (int32_t*)(dws + res_at);
        size_t c0 = 0;
        while (c0 < nb) {
            const int c = fit_class(desc[c0].m);
            size_t c1 = c0;
            while (c1 < nb && fit_class(desc[c1].m) == c) c1++;
            const int B = kFitClasses[c].B, G = kFitClasses[c].G, nq = (int)(c1 - c0);
            const dim3 grid((unsigned)((nq + 64 / G - 1) / (64 / G))), block(64);
            const FitQuery* dq = (const FitQuery*)dws + c0;
            if (B == 2)
                hipLaunchKernelGGL(fit_kernel<2>, grid, block, 0, ctx->stream, dq, nq, G, dws, dres, sc);
            else if (B == 4)
                hipLaunchKernelGGL(fit_kernel<4>, grid, block, 0, ctx->stream, dq, nq, G, dws, dres, sc);
            else if (B == 8)
                hipLaunchKernelGGL(fit_kernel<8>, grid, block, 0, ctx->stream, dq, nq, G, dws, dres, sc);
            else
                hipLaunchKernelGGL(fit_kernel<16>, grid, block, 0, ctx->stream, dq, nq, G, dws, dres, sc);
            RD_HIP(hipGetLastError());
            c0 = c1;
        }
        res.resize(nb * FIT_RES);
        RD_HIP(hipMemcpyAsync(res.data(), dres, res.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
        RD_HIP(hipStreamSynchronize(ctx->stream));
        for (size_t k = 0; k < nb; k++) {
            const int32_t p = order[k0 + k];
            const int32_t* r = &res[k * FIT_RES];
            score[p] = r[0];
            ref_start[p] = r[1];
            ref_end[p] = r[2];
            for (int c = 0; c < 4; c++) counts[4 * (int64_t)p + c] = r[3 + c];
            status[p] = RD_FIT_OK;
        }
    }
    if (too_large) {
        const int64_t p = first_too_large;
        rd_set_error("rd_fit_batch: query %lld (%lld labels against reference %d of %lld codes) needs %lld bytes, over the budget of %lld; "
                     "%lld quer%s not aligned (status RD_FIT_TOO_LARGE), the others were", (long long)p, (long long)(query_off[p + 1] - query_off[p]),
                     query_ref[p], (long long)(ref_off[query_ref[p] + 1] - ref_off[query_ref[p]]),
                     (long long)(fit_ref_bytes(ref_off[query_ref[p] + 1] - ref_off[query_ref[p]]) + fit_query_bytes(query_off[p + 1] - query_off[p]) + FIT_BATCH_BYTES),
                     (long long)budget_bytes, (long long)too_large, too_large == 1 ? "y" : "ies");
        return RD_ERR_NOMEM;
    }
    return RD_OK;
}
