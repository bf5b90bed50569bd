// align.hip -- read-accuracy evaluation (radian/align.py): affine-gap global alignment of basecalls against their
// reference sequences, soft clip and the counts of analyse_alignment, on the MI355X.
//
// Scores (pairwise2.align.globalms(ref, seq, 2, -4, -4, -2), align.py:87): match / mismatch by byte equality, a gap of
// length L costs open + (L-1) * extend, end gaps are penalised.  Gotoh's three states, int32, ref = rows i (1..n),
// read = columns j (1..m):
//   E[i][j] = max(H[i-1][j] + open, E[i-1][j] + extend)         deletion  (ref base against a read gap)
//   F[i][j] = max(H[i][j-1] + open, F[i][j-1] + extend)         insertion (read base against a ref gap)
//   H[i][j] = max(H[i-1][j-1] + s(a_i, b_j), E[i][j], F[i][j])
//   H[0][0] = 0, H[i][0] = gap(i), H[0][j] = gap(j)
//
// Forward (align_fwd_kernel): one wave per pair.  The ref is cut into tiles of 64 rows, lane l owning row 64T + l + 1;
// the wave sweeps the read with a skew of one column per lane (step t: lane l computes column t - l + 1), so a lane
// takes H and E of the row above from lane l - 1's previous step with one DPP wave_shr:1 each, and the read byte rides
// along the same way.  Lane 0 takes them from the row above the tile: 64 columns at a time in registers (one per lane,
// a uniform v_readlane per step), loaded one chunk ahead from a per-pair boundary row in global memory that lane 63
// writes back 64 columns at a time for the next tile.  No LDS.  A step is one cell per lane.
//
// Direction bits, 4 per cell: bits 0-1 the source of H (0 diagonal, 1 E, 2 F), bit 2 "E opened here" (from H, not
// extended), bit 3 "F opened here".  Each lane packs 8 steps into a uint32, so a tile writes 256 contiguous bytes
// every 8 steps: word (T * S8 + t / 8) * 64 + l, nibble t % 8, S8 = 8 * ceil((m + 63) / 64).
//
// Tie-break (fixed; the reference draws one of the co-optimal alignments with random.choice, align.py:88-89):
// H prefers the diagonal, then E (deletion), then F (insertion); inside a gap run extending comes before closing
// (the open bit is set only when opening is strictly better).  The traceback walks these bits from (n, m).
//
// Traceback (align_tb_kernel): one lane per pair; writes the pair's column ops ('M' match, 'X' mismatch, 'D' deletion,
// 'I' insertion) to its slot of n + m bytes, then clips and counts them (align_clip_count, below).
#include "common.h"
#include "budget.h"
#include "align_batch.h"

#include <algorithm>
#include <cstring>
#include <numeric>

namespace {

constexpr int ALN_NEG = -(1 << 30);
constexpr int ALN_OK = 0, ALN_CLIP_INDEX_ERROR = 1, ALN_EMPTY_AFTER_CLIP = 2, ALN_TOO_LARGE = 3;   // radian_hip.h RD_ALIGN_*

struct AlnScores {
    int match, mismatch, open, extend;
};

__host__ __device__ inline int aln_gap(int len, const AlnScores& s) { return len == 0 ? 0 : s.open + (len - 1) * s.extend; }

__host__ __device__ inline bool aln_is_base(uint8_t c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }

// Soft clip + counts of analyse_alignment (radian/align.py:9-57) on the op string of an alignment.  The ref line has a
// '-' exactly at the 'I' columns.  clip_start: first column with three non-gap ref characters, short-circuit order,
// IndexError when it reads past the end; clip_end: the same scanning backwards, where Python's negative indices wrap
// (IndexError only below -len).  Columns of a read gap whose ref character is not in {A,C,G,T}, and of a ref gap whose
// read character is not, count as nothing.  cnt = {n_match, n_sub, n_ins, n_del} (analyse_alignment's return order).
__host__ __device__ inline int aln_clip_count(const uint8_t* ops, int64_t L, const uint8_t* A, const uint8_t* B, int32_t* cnt)
{
    cnt[0] = cnt[1] = cnt[2] = cnt[3] = 0;
    int64_t cs = 0;
    for (int64_t k = 0; k < L; k++) {
        cs = k;
        if (ops[k] == 'I') continue;
        if (k + 1 >= L) return ALN_CLIP_INDEX_ERROR;
        if (ops[k + 1] == 'I') continue;
        if (k + 2 >= L) return ALN_CLIP_INDEX_ERROR;
        if (ops[k + 2] == 'I') continue;
        break;
    }
    int64_t ce = L - 1;
    for (int64_t k = L - 1; k >= 0; k--) {
        ce = k;
        if (ops[k] == 'I') continue;
        int64_t q = k - 1 < 0 ? k - 1 + L : k - 1;
        if (q < 0) return ALN_CLIP_INDEX_ERROR;
        if (ops[q] == 'I') continue;
        q = k - 2 < 0 ? k - 2 + L : k - 2;
        if (q < 0) return ALN_CLIP_INDEX_ERROR;
        if (ops[q] == 'I') continue;
        break;
    }
    if (cs > ce) return ALN_EMPTY_AFTER_CLIP;
    int64_t i = 0, j = 0;   // ref / read characters consumed before column k
    for (int64_t k = 0; k <= ce; k++) {
        const uint8_t o = ops[k];
        const bool in = k >= cs;
        if (o == 'M' || o == 'X') {
            if (in) cnt[o == 'M' ? 0 : 1]++;
            i++;
            j++;
        } else if (o == 'D') {
            if (in && aln_is_base(A[i])) cnt[3]++;
            i++;
        } else {
            if (in && aln_is_base(B[j])) cnt[2]++;
            j++;
        }
    }
    return ALN_OK;
}

// lane l receives v of lane l - 1, lane 0 receives edge (DPP wave_shr:1, bound_ctrl off: the invalid source keeps `old`)
__device__ __forceinline__ int aln_shr1(int v, int edge) { return __builtin_amdgcn_update_dpp(edge, v, 0x138, 0xf, 0xf, false); }

__device__ __forceinline__ int aln_chunks(int m) { return (m + 63 + 63) / 64; }   // 64-step chunks of a tile sweep (m + 63 steps)

__global__ __launch_bounds__(64) void align_fwd_kernel(const AlnPair* __restrict__ pairs, uint8_t* __restrict__ ws, int32_t* __restrict__ res,
                                                       AlnScores sc)
{
    const AlnPair P = pairs[blockIdx.x];
    const int lane = threadIdx.x;
    const int n = P.n, m = P.m;
    if (n == 0 || m == 0) {
        if (lane == 0) res[(int64_t)blockIdx.x * ALN_RES] = aln_gap(n + m, sc);
        return;
    }
    const uint8_t* A = ws + P.ref;
    const uint8_t* B = ws + P.read;
    int32_t* bH = (int32_t*)ws + P.bnd;
    int32_t* bE = bH + (m + 1);
    uint32_t* dirs = (uint32_t*)ws + P.dir;
    for (int j = lane; j <= m; j += 64) {   // row 0
        bH[j] = aln_gap(j, sc);
        bE[j] = ALN_NEG;
    }
    const int nch = aln_chunks(m);
    const int tiles = (n + 63) / 64;
    for (int T = 0; T < tiles; T++) {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   // the boundary row written by the previous tile (this wave)
        const int i = T * 64 + lane + 1;
        const int a = i <= n ? A[i - 1] : 0x100;   // rows past n compute values nobody reads
        int h = aln_gap(i, sc), e = ALN_NEG, f = ALN_NEG, bc = 0x200;
        int diag = aln_gap(i - 1, sc);
        uint32_t acc = 0;
        uint32_t* D = dirs + (int64_t)T * nch * 8 * 64 + lane;
        // chunk c: lane k holds column 64c + 1 + k of the row above the tile and read byte 64c + k
        auto load = [&](int c, int& cH, int& cE, int& cB) {
            const int col = c * 64 + 1 + lane, rb = c * 64 + lane;
            cH = col <= m ? bH[col] : ALN_NEG;
            cE = col <= m ? bE[col] : ALN_NEG;
            cB = rb < m ? B[rb] : 0x200;
        };
        int cH, cE, cB, nH = ALN_NEG, nE = ALN_NEG, nB = 0x200;
        load(0, cH, cE, cB);
        int oH = 0, oE = 0;   // lane 63's cells, gathered one per lane until 64 columns are complete
        for (int c = 0; c < nch; c++) {
            if (c + 1 < nch) load(c + 1, nH, nE, nB);
            for (int k = 0; k < 64; k++) {
                const int t = c * 64 + k;
                const int j = t - lane + 1;
                const int up = aln_shr1(h, __builtin_amdgcn_readlane(cH, k));
                const int upE = aln_shr1(e, __builtin_amdgcn_readlane(cE, k));
                bc = aln_shr1(bc, __builtin_amdgcn_readlane(cB, k));
                const int eo_v = up + sc.open, ee_v = upE + sc.extend;
                const int fo_v = h + sc.open, fe_v = f + sc.extend;
                const int en = max(eo_v, ee_v), fn = max(fo_v, fe_v);
                int hn = diag + (a == bc ? sc.match : sc.mismatch), src = 0;
                if (en > hn) { hn = en; src = 1; }
                if (fn > hn) { hn = fn; src = 2; }
                diag = up;
                acc |= (uint32_t)(src | (eo_v > ee_v) << 2 | (fo_v > fe_v) << 3) << (4 * (k & 7));
                if ((k & 7) == 7) {
                    D[(int64_t)(t >> 3) * 64] = acc;
                    acc = 0;
                }
                const bool valid = j >= 1;   // j > m: columns past the read, nobody reads them
                h = valid ? hn : h;
                e = valid ? en : ALN_NEG;
                f = valid ? fn : ALN_NEG;
                if (i == n && j == m) res[(int64_t)blockIdx.x * ALN_RES] = hn;
                // lane 63's cell of this step is column t - 62 of the tile's last row
                const int jw = t - 62;
                const int h63 = __builtin_amdgcn_readlane(h, 63), e63 = __builtin_amdgcn_readlane(e, 63);
                if (jw >= 0 && jw <= m) {   // columns past m do not exist: the flush at jw == m is the last
                    if (lane == (jw & 63)) {
                        oH = h63;
                        oE = e63;
                    }
                    if ((jw & 63) == 63 || jw == m) {
                        const int col = (jw & ~63) + lane;
                        if (col <= jw) {
                            bH[col] = oH;
                            bE[col] = oE;
                        }
                    }
                }
            }
            cH = nH;
            cE = nE;
            cB = nB;
        }
    }
}

__global__ __launch_bounds__(64) void align_tb_kernel(const AlnPair* __restrict__ pairs, int n_pairs, uint8_t* __restrict__ ws,
                                                      int32_t* __restrict__ res)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n_pairs) return;
    const AlnPair P = pairs[p];
    const uint8_t* A = ws + P.ref;
    const uint8_t* B = ws + P.read;
    uint8_t* O = ws + P.ops;
    const uint32_t* dirs = (const uint32_t*)ws + P.dir;
    const int64_t S8 = (int64_t)aln_chunks(P.m) * 8;
    int i = P.n, j = P.m, st = 0;   // st: the state the walk is in, 0 H, 1 E, 2 F
    int64_t L = 0;
    while (i > 0 || j > 0) {
        if (i == 0) {
            O[L++] = 'I';
            j--;
            continue;
        }
        if (j == 0) {
            O[L++] = 'D';
            i--;
            continue;
        }
        const int l = (i - 1) & 63, t = j - 1 + l;
        const uint32_t w = dirs[((int64_t)((i - 1) >> 6) * S8 + (t >> 3)) * 64 + l];
        const int d = (w >> (4 * (t & 7))) & 15;
        if (st == 0) {
            st = d & 3;
            if (st == 0) {
                O[L++] = A[i - 1] == B[j - 1] ? 'M' : 'X';
                i--;
                j--;
            }
        } else if (st == 1) {
            O[L++] = 'D';
            if (d & 4) st = 0;
            i--;
        } else {
            O[L++] = 'I';
            if (d & 8) st = 0;
            j--;
        }
    }
    for (int64_t k = 0; k < L / 2; k++) {
        const uint8_t x = O[k];
        O[k] = O[L - 1 - k];
        O[L - 1 - k] = x;
    }
    int32_t* r = res + (int64_t)p * ALN_RES;
    r[5] = aln_clip_count(O, L, A, B, r + 1);
    r[6] = (int32_t)L;
}

// bytes of workspace a pair takes (its share of a batch): descriptor + results, sequences, op slot, boundary rows, direction words
size_t aln_pair_bytes(int64_t n, int64_t m)
{
    size_t b = 128 + align_up((size_t)(n + m), 256) + (size_t)(n + m);
    if (n > 0 && m > 0) {
        const size_t nch = (size_t)(m + 126) / 64;
        b += align_up((size_t)8 * (m + 1), 256) + align_up((size_t)((n + 63) / 64) * nch * 8 * 64 * 4, 256);
    }
    return b;
}
constexpr size_t ALN_BATCH_BYTES = 1024;   // alignment slack of a batch's descriptor, result and op arrays

}  // namespace

extern "C" int64_t rd_align_workspace_bytes(int64_t n, int64_t m)
{
    if (n < 0 || m < 0) return -1;
    return (int64_t)(aln_pair_bytes(n, m) + ALN_BATCH_BYTES);
}

extern "C" int rd_align_clip_count(const uint8_t* ops, int64_t n_ops, const uint8_t* ref, const uint8_t* read, int32_t* counts,
                                   int32_t* status)
{
    RD_REQUIRE(counts && status && (ops || n_ops == 0) && n_ops >= 0, "rd_align_clip_count: bad argument");
    int64_t nr = 0, nq = 0;
    for (int64_t k = 0; k < n_ops; k++) {
        const uint8_t o = ops[k];
        RD_REQUIRE(o == 'M' || o == 'X' || o == 'D' || o == 'I', "rd_align_clip_count: op %lld is 0x%02x, not one of M X D I", (long long)k, o);
        nr += o != 'I';
        nq += o != 'D';
    }
    RD_REQUIRE((ref || nr == 0) && (read || nq == 0), "rd_align_clip_count: null sequence");
    *status = aln_clip_count(ops, n_ops, ref, read, counts);
    return RD_OK;
}

// The argument checks, the budget plan, the staging and the two kernels of a batch alignment; after align_tb_kernel every launch goes
// through the hook (align_batch.h).  rd_align_batch is this with an empty hook.
int rd_align_batch_run(rd_ctx* ctx, const char* who, const char* too_large_name, const uint8_t* refs, const int64_t* ref_off, const uint8_t* reads,
                       const int64_t* read_off, int n_pairs, int match, int mismatch, int gap_open, int gap_extend, int64_t budget_bytes,
                       int32_t* score, int32_t* counts, int32_t* status, uint8_t* ops_out, const int64_t* ops_off, int32_t* ops_len, AlnHook& hook)
{
    RD_REQUIRE(ctx && ref_off && read_off && score && counts && status, "%s: null argument", who);
    RD_REQUIRE(n_pairs >= 0, "%s: n_pairs %d", who, n_pairs);
    RD_REQUIRE((ops_out == nullptr) == (ops_off == nullptr) && (ops_out == nullptr) == (ops_len == nullptr),
               "%s: ops_out, ops_off and ops_len are given together or not at all", who);
    RD_REQUIRE(budget_bytes >= 0, "%s: negative budget", who);
    const int lim = 1 << 16;
    RD_REQUIRE(abs(match) < lim && abs(mismatch) < lim && abs(gap_open) < lim && abs(gap_extend) < lim, "%s: score out of range", who);
    // with open > extend the recurrence closes a gap and reopens it in the next column: its optimum is not the stated gap cost
    RD_REQUIRE(gap_open <= gap_extend, "%s: gap_open %d is above gap_extend %d (gap_open <= gap_extend is required: otherwise adjacent gaps "
               "reopen and the score is not open + (L-1) * extend per gap)", who, gap_open, gap_extend);
    RD_REQUIRE(ref_off[0] == 0 && read_off[0] == 0, "%s: offsets must start at 0", who);
    std::vector<int64_t> cells(n_pairs), bytes(n_pairs);
    const size_t extra = hook.extra_pair_bytes, batch_bytes = ALN_BATCH_BYTES + (extra ? 256 : 0);
    const int64_t smax = std::max(std::max(abs(match), abs(mismatch)), std::max(abs(gap_open), abs(gap_extend)));
    for (int p = 0; p < n_pairs; p++) {
        const int64_t n = ref_off[p + 1] - ref_off[p], m = read_off[p + 1] - read_off[p];
        RD_REQUIRE(n >= 0 && m >= 0, "%s: pair %d has a negative length", who, p);
        // scores stay far from ALN_NEG: |H| <= smax * (n + m + 1)
        RD_REQUIRE(n < (1 << 30) && m < (1 << 30) && smax * (n + m + 1) < (1 << 28), "%s: pair %d (%lld x %lld) is too long for int32 scores", who,
                   p, (long long)n, (long long)m);
        cells[p] = n * m;
        bytes[p] = (int64_t)(aln_pair_bytes(n, m) + extra);
    }
    RD_REQUIRE(ref_off[n_pairs] == 0 || refs, "%s: null refs", who);
    RD_REQUIRE(read_off[n_pairs] == 0 || reads, "%s: null reads", who);
    RD_HIP(hipSetDevice(ctx->device));
    if (int rc = rd_resolve_budget(&budget_bytes, ctx->ws_align.cap)) return rc;
    // largest pairs first (load balance of a launch), packed into batches under the budget; a pair that alone exceeds it is
    // reported, not launched
    std::vector<int> order(n_pairs);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return cells[x] > cells[y]; });
    const BudgetPlan plan = rd_plan_budget(n_pairs, order.data(), budget_bytes, (int64_t)batch_bytes, false,
                                           [&](int p, int) { return bytes[p]; }, rd_budget_never_closes);
    const std::vector<int32_t>& run = plan.run;
    const int too_large = (int)plan.too_large, first_too_large = (int)plan.first_too_large;
    for (int p = 0; p < n_pairs; p++) {   // until its batch has run
        status[p] = ALN_TOO_LARGE;
        score[p] = 0;
        for (int c = 0; c < 4; c++) counts[4 * (int64_t)p + c] = 0;
        if (ops_len) ops_len[p] = 0;
    }
    hook.accepted(n_pairs);
    if (ctx->ws_align.reserve_exact((size_t)plan.max_bytes, who)) return RD_ERR_NOMEM;
    const AlnScores sc{match, mismatch, gap_open, gap_extend};
    std::vector<uint8_t> stage;
    std::vector<AlnPair> desc;
    std::vector<int32_t> res;
    std::vector<uint8_t> ops_h;
    for (auto [k0, k1] : plan.launches) {
        const int nb = (int)(k1 - k0);
        Carve c;   // (dry: the descriptors hold offsets into ws_align; the head of the block is staged on the host and copied whole)
        c.take<AlnPair>((size_t)nb);
        const size_t res_at = c.mark();
        c.take<int32_t>((size_t)nb * ALN_RES);
        desc.resize(nb);
        for (int k = 0; k < nb; k++) {   // sequences first (one upload with the descriptors), then the device-only regions
            const int p = run[k0 + k];
            AlnPair& d = desc[k];
            d.n = (int32_t)(ref_off[p + 1] - ref_off[p]);
            d.m = (int32_t)(read_off[p + 1] - read_off[p]);
            d.ref = (int64_t)c.mark();
            d.read = d.ref + d.n;
            c.take<uint8_t>((size_t)(d.n + d.m));
        }
        const size_t up_bytes = c.mark();
        for (int k = 0; k < nb; k++) {   // op slots side by side, unrounded (one copy back)
            desc[k].ops = (int64_t)c.mark();
            c.take<uint8_t>((size_t)(desc[k].n + desc[k].m), 0, 1);
        }
        const size_t ops_lo = up_bytes, ops_hi = c.mark();
        c.round();
        for (int k = 0; k < nb; k++) {
            AlnPair& d = desc[k];
            if (d.n > 0 && d.m > 0) {
                d.bnd = (int64_t)(c.mark() / 4);
                c.take<int32_t>(2 * ((size_t)d.m + 1));
                d.dir = (int64_t)(c.mark() / 4);
                c.take<uint32_t>((size_t)((d.n + 63) / 64) * ((d.m + 126) / 64) * 8 * 64);
            } else {
                d.bnd = d.dir = 0;
            }
        }
        const size_t extra_at = c.mark();
        c.take<uint8_t>((size_t)nb * extra, 0, 1);
        if (int rc = rd_carve_check(who, c, ctx->ws_align.cap)) return rc;
        stage.assign(up_bytes, 0);
        memcpy(stage.data(), desc.data(), (size_t)nb * sizeof(AlnPair));
        for (int k = 0; k < nb; k++) {
            const int p = run[k0 + k];
            if (desc[k].n) memcpy(stage.data() + desc[k].ref, refs + ref_off[p], desc[k].n);
            if (desc[k].m) memcpy(stage.data() + desc[k].read, reads + read_off[p], desc[k].m);
        }
        uint8_t* dws = ctx->ws_align.as<uint8_t>();
        RD_HIP(hipMemcpyAsync(dws, stage.data(), up_bytes, hipMemcpyHostToDevice, ctx->stream));
        const AlnPair* dpairs = (const AlnPair*)dws;
        int32_t* dres = (int32_t*)(dws + res_at);
        hipLaunchKernelGGL(align_fwd_kernel, dim3(nb), dim3(64), 0, ctx->stream, dpairs, dws, dres, sc);
        RD_HIP(hipGetLastError());
        hipLaunchKernelGGL(align_tb_kernel, dim3((nb + 63) / 64), dim3(64), 0, ctx->stream, dpairs, nb, dws, dres);
        RD_HIP(hipGetLastError());
        res.resize((size_t)nb * ALN_RES);
        RD_HIP(hipMemcpyAsync(res.data(), dres, res.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (ops_out && ops_hi > ops_lo) {
            ops_h.resize(ops_hi - ops_lo);
            RD_HIP(hipMemcpyAsync(ops_h.data(), dws + ops_lo, ops_hi - ops_lo, hipMemcpyDeviceToHost, ctx->stream));
        }
        const AlnLaunch launch{dpairs, dws, dres, extra ? dws + extra_at : nullptr, nb, &run[k0], desc.data(), ctx->stream};
        if (int rc = hook.launched(launch)) return rc;
        RD_HIP(hipStreamSynchronize(ctx->stream));
        if (int rc = hook.finished(launch)) return rc;
        for (int k = 0; k < nb; k++) {
            const int p = run[k0 + k];
            const int32_t* r = &res[(size_t)k * ALN_RES];
            score[p] = r[0];
            for (int c = 0; c < 4; c++) counts[4 * (int64_t)p + c] = r[1 + c];
            status[p] = r[5];
            if (ops_out) {
                ops_len[p] = r[6];
                memcpy(ops_out + ops_off[p], ops_h.data() + (desc[k].ops - ops_lo), (size_t)r[6]);
            }
        }
    }
    if (too_large) {
        rd_set_error("%s: pair %d (%lld x %lld) needs %lld bytes of workspace, over the budget of %lld; %d pair(s) not aligned "
                     "(status %s), the others were", who, first_too_large, (long long)(ref_off[first_too_large + 1] - ref_off[first_too_large]),
                     (long long)(read_off[first_too_large + 1] - read_off[first_too_large]), (long long)(bytes[first_too_large] + (int64_t)batch_bytes),
                     (long long)budget_bytes, too_large, too_large_name);
        return RD_ERR_NOMEM;
    }
    return RD_OK;
}

extern "C" int rd_align_batch(rd_ctx* ctx, const uint8_t* refs, const int64_t* ref_off, const uint8_t* reads, const int64_t* read_off,
                              int n_pairs, int match, int mismatch, int gap_open, int gap_extend, int64_t budget_bytes, int32_t* score,
                              int32_t* counts, int32_t* status, uint8_t* ops_out, const int64_t* ops_off, int32_t* ops_len)
{
    AlnHook none;
    return rd_align_batch_run(ctx, "rd_align_batch", "RD_ALIGN_TOO_LARGE", refs, ref_off, reads, read_off, n_pairs, match, mismatch, gap_open,
                              gap_extend, budget_bytes, score, counts, status, ops_out, ops_off, ops_len, none);
}
