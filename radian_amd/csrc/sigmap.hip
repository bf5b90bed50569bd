// sigmap.hip -- raw samples against a panel of transcripts under a k-mer pore model: the subsequence DP that finds, for a window of a
// read's samples, the targets it fits best, where in each the fit ends and where it began.  No basecall takes part.  DESIGN.md section 25.
//
// Contract (integer arithmetic only, met exactly; include/radian_hip.h, rd_sigmap; the rules themselves are sigmap_rules.h, the sample,
// the cost and the strict advance eventalign_rules.h's).  Targets j = 0 .. n_tgt - 1 hold the states tgt_off[j] .. tgt_off[j+1]; a query is
// T rows of samples, a scale and a range [s_lo, s_hi) of states:
//   head(s)   s is the first state of its target, or s == s_lo
//   V[0][s]   = c(0, s), O[0][s] = s
//   V[t][s]   = c(t, s) + (adv ? V[t-1][s-1] : V[t-1][s]), adv = !head(s) && V[t-1][s-1] < V[t-1][s] (STRICTLY); O follows
//   per target the smallest V[T-1][s] over its states in range, the smallest s on ties; per query the n_best targets by (score, j)
//
// Kernels, on one stream:
//   sm_state_kernel   once per call, one thread per state of the panel: its k-mer within its own target (bit 31: first state of the
//                     target) and its target
//   signal_scale_kernel   (signal_dev.h) once per call, one 256-thread workgroup per query: the scale as given, or the scale window's own
//   per launch (a set of queries whose workspace fits the budget):
//   sm_quant_kernel   zq rows, one int32 per sample; the (query, target) keys to "none"
//   sm_dp_kernel      one workgroup per STRIPE: band_sweep.h's sweep.  A stripe reports the ends [a, b) (SM_PAYLOAD of them) and computes
//                     the states [left, b), left = max(s_lo, a - (T - 1)), with a free start: cell (t, s) is exact for s >= left + t, so
//                     row T - 1 is exact on [a, b).  A thread's registers: value, origin, level, weight and bias of its 16 states and a
//                     16-bit head mask; value and origin (8 bytes) cross a thread boundary; a tile is 128 rows of zq and of the incoming
//                     column's value and origin.  A wave that holds no head runs the row without the mask.  Nothing is stored per row
//                     but the column.  At the end a thread stores the origins of its end states (4 bytes per state of the range) and
//                     merges its end values into the (query, target) keys, (score + 2^25) << 32 | state, with a 64-bit atomicMin per
//                     run of states of one target: the minimum does not depend on the order.
//   sm_select_kernel  one wave per query: n_best times the smallest (score, j) above the previous one
// No floating point, no scratch.  A query's result does not depend on its launch's other queries.
#include "common.h"
#include "budget.h"
#include "sigmap_rules.h"
#include "eventalign_host.h"
#include "../../include/radian_hip.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace {

struct SmCall {
    const int16_t* raw;
    int64_t n_raw;
    int n_q;
    const int64_t *q_lo, *q_hi, *sc_lo, *sc_hi;
    const int32_t *m2_in, *d4_in;
    const int64_t *s_lo, *s_hi;
    const uint8_t* codes;
    const int64_t* tgt_off;
    int n_tgt, k;
    const int32_t* lvl;
    const uint32_t* w;
    const int32_t* bias;
    int n_best;
    int32_t *status, *m2, *d4, *best_tgt, *best_score, *best_end, *best_org;
};

int sm_check_args(const char* who, const SmCall& c)
{
    RD_REQUIRE(c.n_q >= 0 && c.n_tgt >= 0 && c.n_raw >= 0, "%s: negative count", who);
    RD_REQUIRE(c.n_best >= 1 && c.n_best <= SM_MAX_BEST, "%s: n_best = %d, not in 1..%d", who, c.n_best, SM_MAX_BEST);
    RD_REQUIRE(sim_k_ok(c.k), "%s: k = %d, not odd and 1..9", who, c.k);
    RD_REQUIRE(c.lvl && c.w && c.bias, "%s: null model table", who);
    const int64_t n_kmers = (int64_t)1 << (2 * c.k);
    for (int64_t i = 0; i < n_kmers; i++)
        RD_REQUIRE(ea_entry_ok(c.lvl[i], c.bias[i]), "%s: model entry %lld (lvl %d, bias %d) is outside |lvl| < 2^14, |bias| <= 256", who, (long long)i,
                   c.lvl[i], c.bias[i]);
    RD_REQUIRE(c.tgt_off, "%s: null target offsets", who);
    RD_REQUIRE(c.tgt_off[0] == 0, "%s: target offsets must start at 0", who);
    for (int j = 0; j < c.n_tgt; j++)
        RD_REQUIRE(c.tgt_off[j + 1] >= c.tgt_off[j], "%s: target offsets must be non-decreasing (target %d)", who, j);
    const int64_t R = c.tgt_off[c.n_tgt];
    RD_REQUIRE(R <= INT32_MAX, "%s: %lld states, more than 2^31 - 1", who, (long long)R);
    RD_REQUIRE(R == 0 || c.codes, "%s: null codes", who);
    for (int64_t s = 0; s < R; s++) RD_REQUIRE(c.codes[s] < 4, "%s: code %lld is %d, not in 0..3", who, (long long)s, c.codes[s]);
    if (c.n_q == 0) return RD_OK;
    RD_REQUIRE(c.q_lo && c.q_hi && c.sc_lo && c.sc_hi && c.m2_in && c.d4_in && c.s_lo && c.s_hi, "%s: null argument", who);
    RD_REQUIRE(c.status && c.m2 && c.d4 && c.best_tgt && c.best_score && c.best_end && c.best_org, "%s: null output", who);
    RD_REQUIRE(c.n_raw == 0 || c.raw, "%s: null samples", who);
    for (int q = 0; q < c.n_q; q++) {
        RD_REQUIRE(0 <= c.q_lo[q] && c.q_lo[q] <= c.q_hi[q] && c.q_hi[q] <= c.n_raw, "%s: query %d: the window [%lld, %lld) is outside the %lld samples",
                   who, q, (long long)c.q_lo[q], (long long)c.q_hi[q], (long long)c.n_raw);
        RD_REQUIRE(0 <= c.sc_lo[q] && c.sc_lo[q] <= c.sc_hi[q] && c.sc_hi[q] <= c.n_raw && c.sc_hi[q] - c.sc_lo[q] <= INT32_MAX,
                   "%s: query %d: the scale window [%lld, %lld) is outside the %lld samples or longer than 2^31 - 1", who, q, (long long)c.sc_lo[q],
                   (long long)c.sc_hi[q], (long long)c.n_raw);
        RD_REQUIRE(ea_scale_ok(c.m2_in[q], c.d4_in[q]), "%s: query %d: the scale (m2 %d, d4 %d) is outside |m2| <= 2^17, 0 <= d4 <= 2^20", who, q,
                   c.m2_in[q], c.d4_in[q]);
        RD_REQUIRE(0 <= c.s_lo[q] && c.s_lo[q] <= c.s_hi[q] && c.s_hi[q] <= R, "%s: query %d: the state range [%lld, %lld) is outside the %lld states",
                   who, q, (long long)c.s_lo[q], (long long)c.s_hi[q], (long long)R);
    }
    return RD_OK;
}

// the outputs of query q with this status and scale, no target found
void sm_blank(const SmCall& c, int q, int status, int32_t m2, int32_t d4)
{
    c.status[q] = status;
    c.m2[q] = m2;
    c.d4[q] = d4;
    for (int i = 0; i < c.n_best; i++) {
        const int64_t o = (int64_t)q * c.n_best + i;
        c.best_tgt[o] = c.best_score[o] = c.best_end[o] = c.best_org[o] = -1;
    }
}

// the index span of the targets that meet [s_lo, s_hi), s_lo < s_hi: *j_lo and the count up to the target of s_hi - 1
int64_t sm_target_span(const SmCall& c, int q, int32_t* j_lo)
{
    *j_lo = sm_target_of(c.tgt_off, c.n_tgt, c.s_lo[q]);
    return sm_target_of(c.tgt_off, c.n_tgt, c.s_hi[q] - 1) - *j_lo + 1;
}

int64_t sm_bytes_of(const SmCall& c, int q)
{
    int32_t j_lo;
    return sm_query_bytes(c.q_hi[q] - c.q_lo[q], c.s_hi[q] - c.s_lo[q], sm_target_span(c, q, &j_lo));
}

}  // namespace

extern "C" int64_t rd_sigmap_workspace_bytes(int64_t n_rows, int64_t n_states, int64_t n_tgt_in_range)
{
    if (n_rows < 0 || n_states < 0 || n_tgt_in_range < 0) return -1;
    return sm_query_bytes(n_rows, n_states, n_tgt_in_range);
}

extern "C" int rd_sigmap_host(const int16_t* raw, int64_t n_raw, int n_q, const int64_t* q_lo, const int64_t* q_hi, const int64_t* sc_lo,
                              const int64_t* sc_hi, const int32_t* m2_in, const int32_t* d4_in, const int64_t* s_lo, const int64_t* s_hi,
                              const uint8_t* codes, const int64_t* tgt_off, int n_tgt, int k, const int32_t* lvl, const uint32_t* w,
                              const int32_t* bias, int n_best, int32_t* status, int32_t* m2, int32_t* d4, int32_t* best_tgt, int32_t* best_score,
                              int32_t* best_end, int32_t* best_org)
{
    const SmCall c{raw, n_raw, n_q, q_lo, q_hi, sc_lo, sc_hi, m2_in, d4_in, s_lo, s_hi, codes, tgt_off, n_tgt, k, lvl, w, bias, n_best,
                   status, m2, d4, best_tgt, best_score, best_end, best_org};
    int rc = sm_check_args("rd_sigmap_host", c);
    if (rc || n_q == 0) return rc;
    std::vector<int64_t> cnt;
    std::vector<int32_t> zq, V, O;
    std::vector<EaState> st;
    std::vector<uint8_t> head;
    std::vector<uint64_t> keys;
    std::vector<int32_t> orgs;
    for (int q = 0; q < n_q; q++) {
        const int64_t T = q_hi[q] - q_lo[q], n = s_hi[q] - s_lo[q], lo = s_lo[q];
        int32_t um2 = m2_in[q], ud4 = d4_in[q];
        if (T <= 0 || T > SM_MAX_T) {
            sm_blank(c, q, sm_status(T, 1, n), 0, 0);
            continue;
        }
        if (ud4 == 0) {
            um2 = 0;
            if (sc_hi[q] > sc_lo[q]) ea_host_scale(raw + sc_lo[q], sc_hi[q] - sc_lo[q], cnt, &um2, &ud4);
        }
        const int stat = sm_status(T, ud4, n);
        sm_blank(c, q, stat, um2, ud4);
        if (stat != SM_OK) continue;
        zq.resize(T);
        for (int64_t t = 0; t < T; t++) zq[t] = ea_quant(raw[q_lo[q] + t], um2, ud4);
        int32_t j_lo;
        const int64_t n_j = sm_target_span(c, q, &j_lo);
        st.resize(n);
        head.resize(n);
        V.resize(n);
        O.resize(n);
        for (int64_t j = j_lo; j < j_lo + n_j; j++) {
            const int64_t first = tgt_off[j], len = tgt_off[j + 1] - first;
            for (int64_t s = std::max(first, lo); s < std::min(first + len, s_hi[q]); s++) {
                const int32_t i = sim_kmer(codes + first, (int32_t)len, (int32_t)(s - first), k);
                st[s - lo] = EaState{lvl[i], w[i], bias[i]};
                head[s - lo] = sm_head(s, first, lo);
            }
        }
        for (int64_t i = 0; i < n; i++) {
            V[i] = ea_cost(zq[0], st[i].lvl, st[i].w, st[i].bias);
            O[i] = (int32_t)(lo + i);
        }
        for (int64_t t = 1; t < T; t++)
            for (int64_t i = n - 1; i >= 0; i--) {
                const bool adv = !head[i] && ea_advance(V[i], V[i - 1]);
                V[i] = ea_cost(zq[t], st[i].lvl, st[i].w, st[i].bias) + (adv ? V[i - 1] : V[i]);
                if (adv) O[i] = O[i - 1];
            }
        // per target its best end, then the n_best targets by (score, j)
        keys.clear();
        orgs.clear();
        for (int64_t j = j_lo; j < j_lo + n_j; j++) {
            uint64_t best = SM_NO_KEY;
            for (int64_t s = std::max(tgt_off[j], lo); s < std::min(tgt_off[j + 1], s_hi[q]); s++) best = std::min(best, sm_key(V[s - lo], (uint32_t)s));
            if (best == SM_NO_KEY) continue;
            keys.push_back((best & 0xffffffff00000000ull) | (uint64_t)(j - j_lo));
            orgs.push_back((int32_t)sm_key_state(best));
        }
        std::vector<size_t> order(keys.size());
        for (size_t i = 0; i < order.size(); i++) order[i] = i;
        std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return keys[a] < keys[b]; });
        for (size_t r = 0; r < order.size() && r < (size_t)n_best; r++) {
            const uint64_t key = keys[order[r]];
            const int64_t j = j_lo + (int64_t)(uint32_t)key, o = (int64_t)q * n_best + (int64_t)r, e = orgs[order[r]];
            best_tgt[o] = (int32_t)j;
            best_score[o] = sm_key_score(key);
            best_end[o] = (int32_t)(e - tgt_off[j]);
            best_org[o] = (int32_t)(O[e - lo] - tgt_off[j]);
        }
    }
    return RD_OK;
}

// ------------------------------------------------------------------------------------------------------------------ the device blocks
namespace {

struct SmQuery {
    int64_t raw0;            // the query window's sample 0 in the raw buffer
    int64_t zq, org, key;    // byte offsets into the workspace
    int32_t T, m2, d4, s_lo, j_lo, n_j, pad_[2];
};
struct SmStripe {
    int64_t col;             // byte offset of its two band columns in the workspace
    int32_t q, left, a, b;   // the query (of the launch); computes [left, b), reports [a, b)
};
struct SmOut {
    int32_t tgt[SM_MAX_BEST], score[SM_MAX_BEST], end[SM_MAX_BEST], org[SM_MAX_BEST];
};

// behind the k-mer tables in ws_eval_model: the panel's target offsets, and per state its k-mer (bit 31: a target's first) and its target
struct SmPanel {
    int64_t* off;
    uint32_t* kid;
    int32_t* tg;
};
void sm_panel_layout(Carve& c, int n_tgt, int64_t R, SmPanel* p)
{
    p->off = c.take<int64_t>((size_t)n_tgt + 1);
    p->kid = c.take<uint32_t>((size_t)R, 16);
    p->tg = c.take<int32_t>((size_t)R, 16);
}

// a launch's io block (ws_eval): descriptors | stripes | results
struct SmIo {
    SmQuery* qs;
    SmStripe* str;
    SmOut* out;
};
void sm_io_layout(Carve& c, int nb, size_t n_stripes, SmIo* io)
{
    io->qs = c.take<SmQuery>((size_t)nb);
    io->str = c.take<SmStripe>(n_stripes);
    io->out = c.take<SmOut>((size_t)nb, 0, 1);
}

}  // namespace

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------------------------------ device half
#include "band_sweep.h"
#include "signal_dev.h"

namespace {

constexpr int SM_MAX_LAUNCH = 4096;        // queries of one launch
static_assert(SM_BAND == BS_BAND, "a band is a workgroup pass");

__global__ __launch_bounds__(256) void sm_state_kernel(const int64_t* __restrict__ tgt_off, int n_tgt, const uint8_t* __restrict__ codes, int k,
                                                       int64_t R, uint32_t* __restrict__ kid, int32_t* __restrict__ tg)
{
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= R) return;
    const int32_t j = sm_target_of(tgt_off, n_tgt, s);
    const int64_t first = tgt_off[j];
    kid[s] = (uint32_t)sim_kmer(codes + first, (int32_t)(tgt_off[j + 1] - first), (int32_t)(s - first), k) | (s == first ? 0x80000000u : 0u);
    tg[s] = j;
}

// grid (ceil(max T / 256), queries)
__global__ __launch_bounds__(256) void sm_quant_kernel(const SmQuery* __restrict__ qs, const int16_t* __restrict__ raw, uint8_t* __restrict__ ws)
{
    const SmQuery q = qs[blockIdx.y];
    if (blockIdx.x == 0) {
        uint64_t* key = (uint64_t*)(ws + q.key);
        for (int i = threadIdx.x; i < q.n_j; i += 256) key[i] = SM_NO_KEY;
    }
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= q.T) return;
    ((int32_t*)(ws + q.zq))[t] = ea_quant(raw[q.raw0 + t], q.m2, q.d4);
}

// what crosses a thread boundary: a state's value and origin
struct alignas(8) SmCell {
    int32_t v, o;
};
__device__ __forceinline__ SmCell lane_shr1(SmCell c) { return SmCell{lane_shr1(c.v), lane_shr1(c.o)}; }

// one row of a thread's 16 states, from the last down: every cell still reads the row before
template <bool HEADS>
__device__ __forceinline__ void sm_row(int32_t z, int32_t left_v, int32_t left_o, uint32_t hm, const int32_t (&lv)[BS_K], const uint32_t (&wt)[BS_K],
                                       const int32_t (&bi)[BS_K], int32_t (&v)[BS_K], int32_t (&o)[BS_K])
{
#pragma unroll
    for (int j = BS_K - 1; j >= 0; j--) {
        const int32_t av = j >= 1 ? v[j - 1] : left_v, ao = j >= 1 ? o[j - 1] : left_o;
        bool take = ea_advance(v[j], av);
        if (HEADS) take = take && !((hm >> j) & 1u);
        v[j] = ea_cost(z, lv[j], wt[j], bi[j]) + (take ? av : v[j]);
        o[j] = take ? ao : o[j];
    }
}

// band_sweep.h's policy of sigmap
struct SmSweep {
    using Cell = SmCell;
    using Elem = int32_t;
    static constexpr bool AHEAD_CLAMPED = true;
    static constexpr int TR = 128, SLOTS = 3;   // a tile: [0: zq, 1 and 2: the band's incoming column, V and O of [t-1][first state - 1]][row]
    struct Row {
        int32_t z;
        SmCell c;
    };
    // the stripe and its query
    SmStripe sp;
    const int32_t* __restrict__ zq;
    const uint32_t* __restrict__ kid;
    const int32_t* __restrict__ tg;
    const int32_t* __restrict__ lvl_t;
    const uint32_t* __restrict__ w_t;
    const int32_t* __restrict__ bias_t;
    int32_t* __restrict__ org;
    unsigned long long* key;
    int32_t s_lo, j_lo;
    // the thread's states of the band
    int64_t s0;
    int32_t lv[BS_K], bi[BS_K], v[BS_K], o[BS_K];
    uint32_t wt[BS_K], hm;
    bool heads;   // (the same in every lane of a wave)

    static __device__ __forceinline__ int first_row(int) { return 0; }
    static __device__ __forceinline__ Cell none() { return SmCell{EA_INF, 0}; }
    static __device__ __forceinline__ Cell incoming(const Row& in) { return in.c; }
    __device__ __forceinline__ Cell last() const { return SmCell{v[BS_K - 1], o[BS_K - 1]}; }

    __device__ __forceinline__ void begin_band(int b)
    {
        s0 = (int64_t)sp.left + (int64_t)b * SM_BAND + (int)threadIdx.x * BS_K;
        hm = 0;
#pragma unroll
        for (int j = 0; j < BS_K; j++) {
            lv[j] = bi[j] = 0;   // a state past the stripe: cost 0, reported nowhere
            wt[j] = 0;
            v[j] = 0;            // row -1: all equal, so no advance is taken in row 0 and V[0][s] = c(0, s)
            o[j] = (int32_t)(s0 + j);
            if (s0 + j < sp.b) {
                const uint32_t kd = kid[s0 + j], i = kd & 0x7fffffffu;
                lv[j] = lvl_t[i];
                wt[j] = w_t[i];
                bi[j] = bias_t[i];
                if ((kd >> 31) || s0 + j == sp.left) hm |= 1u << j;
            }
        }
        heads = __ballot(hm != 0) != 0;
    }
    __device__ __forceinline__ Elem tile_elem(int e, int tbase, int T, int b, const Cell* cin) const
    {
        const int which = e / TR, t = tbase + (e % TR);
        Elem x = which == 1 ? EA_INF : 0;   // row 0, band 0: nothing comes from the left
        if (t < T) {
            if (which == 0) x = zq[t];
            else if (b > 0 && t >= 1) x = which == 1 ? cin[t - 1].v : cin[t - 1].o;
        }
        return x;
    }
    __device__ __forceinline__ Row read_row(const Elem* tile, int r) const { return Row{tile[r], SmCell{tile[TR + r], tile[2 * TR + r]}}; }
    __device__ __forceinline__ void row(int, const Row& in, Cell left)
    {
        if (heads) sm_row<true>(in.z, left.v, left.o, hm, lv, wt, bi, v, o);
        else sm_row<false>(in.z, left.v, left.o, hm, lv, wt, bi, v, o);
    }
    // the ends this stripe reports: the origin of every one, the best of every run of one target
    __device__ __forceinline__ void end_band() const
    {
        uint64_t best = SM_NO_KEY;
        int32_t cur = -1;
#pragma unroll
        for (int j = 0; j < BS_K; j++) {
            const int64_t s = s0 + j;
            if (s >= sp.a && s < sp.b) {
                org[s - s_lo] = o[j];
                const int32_t jt = tg[s];
                if (jt != cur) {
                    if (cur >= 0) atomicMin(key + (cur - j_lo), (unsigned long long)best);
                    cur = jt;
                    best = SM_NO_KEY;
                }
                const uint64_t ky = sm_key(v[j], (uint32_t)s);
                best = ky < best ? ky : best;
            }
        }
        if (cur >= 0) atomicMin(key + (cur - j_lo), (unsigned long long)best);
    }
};

__global__ __launch_bounds__(BS_NT) void sm_dp_kernel(const SmQuery* __restrict__ qs, const SmStripe* __restrict__ stripes,
                                                      const uint32_t* __restrict__ kid, const int32_t* __restrict__ tg,
                                                      const int32_t* __restrict__ lvl_t, const uint32_t* __restrict__ w_t,
                                                      const int32_t* __restrict__ bias_t, uint8_t* __restrict__ ws)
{
    const SmStripe sp = stripes[blockIdx.x];
    const SmQuery q = qs[sp.q];
    SmSweep p{sp, (const int32_t*)(ws + q.zq), kid, tg, lvl_t, w_t, bias_t, (int32_t*)(ws + q.org), (unsigned long long*)(ws + q.key), q.s_lo, q.j_lo};
    band_sweep(p, (int64_t)sp.b - sp.left, q.T, (SmCell*)(ws + sp.col));   // at most SM_PAYLOAD + T - 1 states
}

// one wave per query
__global__ __launch_bounds__(64) void sm_select_kernel(const SmQuery* __restrict__ qs, const int64_t* __restrict__ tgt_off, const uint8_t* __restrict__ ws,
                                                       int n_best, SmOut* __restrict__ out)
{
    const SmQuery q = qs[blockIdx.x];
    const int lane = threadIdx.x;
    const uint64_t* __restrict__ key = (const uint64_t*)(ws + q.key);
    const int32_t* __restrict__ org = (const int32_t*)(ws + q.org);
    uint64_t prev = 0;
    bool have = false, done = false;   // (the same in every lane)
    for (int r = 0; r < SM_MAX_BEST; r++) {
        uint64_t m = SM_NO_KEY;
        if (!done && r < n_best)
            for (int i = lane; i < q.n_j; i += 64) {
                const uint64_t ky = key[i];
                if (ky == SM_NO_KEY) continue;   // an empty target
                const uint64_t sk = (ky & 0xffffffff00000000ull) | (uint32_t)i;
                if ((!have || sk > prev) && sk < m) m = sk;
            }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const uint64_t x = __shfl_xor((unsigned long long)m, d);
            m = x < m ? x : m;
        }
        int32_t tgt = -1, score = -1, end = -1, og = -1;
        if (m != SM_NO_KEY) {
            const int32_t i = (int32_t)(uint32_t)m;
            const int64_t first = tgt_off[q.j_lo + i], e = sm_key_state(key[i]);
            tgt = q.j_lo + i;
            score = sm_key_score(m);
            end = (int32_t)(e - first);
            og = (int32_t)(org[e - q.s_lo] - first);
            prev = m;
            have = true;
        } else done = true;
        if (lane == 0) {
            out[blockIdx.x].tgt[r] = tgt;
            out[blockIdx.x].score[r] = score;
            out[blockIdx.x].end[r] = end;
            out[blockIdx.x].org[r] = og;
        }
    }
}

}  // namespace

extern "C" int rd_sigmap(rd_ctx* ctx, const int16_t* raw, int64_t n_raw, int n_q, const int64_t* q_lo, const int64_t* q_hi, const int64_t* sc_lo,
                         const int64_t* sc_hi, const int32_t* m2_in, const int32_t* d4_in, const int64_t* s_lo, const int64_t* s_hi,
                         const uint8_t* codes, const int64_t* tgt_off, int n_tgt, int k, const int32_t* lvl, const uint32_t* w, const int32_t* bias,
                         int n_best, int64_t budget_bytes, int32_t* status, int32_t* m2, int32_t* d4, int32_t* best_tgt, int32_t* best_score,
                         int32_t* best_end, int32_t* best_org)
{
    RD_REQUIRE(ctx, "rd_sigmap: null context");
    RD_REQUIRE(budget_bytes >= 0, "rd_sigmap: negative budget");
    const SmCall c{raw, n_raw, n_q, q_lo, q_hi, sc_lo, sc_hi, m2_in, d4_in, s_lo, s_hi, codes, tgt_off, n_tgt, k, lvl, w, bias, n_best,
                   status, m2, d4, best_tgt, best_score, best_end, best_org};
    int rc = sm_check_args("rd_sigmap", c);
    if (rc || n_q == 0) return rc;
    RD_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // the samples the queries and their scale windows span, rebased to the first of them; the panel; the model
    int64_t lo = n_raw, hi = 0;
    for (int q = 0; q < n_q; q++) {
        lo = std::min(lo, std::min(q_lo[q], sc_lo[q]));
        hi = std::max(hi, std::max(q_hi[q], sc_hi[q]));
    }
    const int64_t n_samples = hi > lo ? hi - lo : 0, R = tgt_off[n_tgt];
    if (ctx->ws_raw.reserve((size_t)n_samples * 2 + 16) || ctx->ws_labels.reserve((size_t)R + 16)) return RD_ERR_NOMEM;
    const int16_t* d_raw = ctx->ws_raw.as<int16_t>();
    const uint8_t* d_codes = ctx->ws_labels.as<uint8_t>();
    if (n_samples) RD_HIP(hipMemcpyAsync(ctx->ws_raw.p, raw + lo, (size_t)n_samples * 2, hipMemcpyHostToDevice, st));
    if (R) RD_HIP(hipMemcpyAsync(ctx->ws_labels.p, codes, (size_t)R, hipMemcpyHostToDevice, st));
    KmerTables tab;
    SmPanel panel;
    Carve panel_dry;
    sm_panel_layout(panel_dry, n_tgt, R, &panel);
    if ((rc = signal_upload_tables(ctx, st, k, lvl, w, bias, panel_dry.at, &tab))) return rc;
    Carve panel_wet(tab.extra);
    sm_panel_layout(panel_wet, n_tgt, R, &panel);
    const int32_t *d_lvl = tab.lvl, *d_bias = tab.bias;
    const uint32_t* d_w = tab.w;
    RD_HIP(hipMemcpyAsync(panel.off, tgt_off, (size_t)(n_tgt + 1) * 8, hipMemcpyHostToDevice, st));
    if (R) {
        hipLaunchKernelGGL(sm_state_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, st, panel.off, n_tgt, d_codes, k, R, panel.kid, panel.tg);
        RD_HIP(hipGetLastError());
    }
    // every query's scale: a property of the query alone, whatever the budget does with it afterwards
    std::vector<SignalScaleIn> scin(n_q);
    std::vector<int32_t> scale;
    for (int q = 0; q < n_q; q++) scin[q] = signal_scale_in(sc_lo[q] - lo, sc_hi[q] - sc_lo[q], q_hi[q] - q_lo[q], SM_MAX_T, m2_in[q], d4_in[q]);
    if ((rc = signal_scales(ctx, st, d_raw, scin, SM_MAX_T, scale))) return rc;
    // statuses that need no alignment, then the launches: the other queries in the caller's order, as many as fit the budget; a query that
    // alone exceeds it is reported, not launched
    for (int q = 0; q < n_q; q++) {
        const int stat = sm_status(q_hi[q] - q_lo[q], scale[2 * (size_t)q + 1], s_hi[q] - s_lo[q]);
        sm_blank(c, q, stat == SM_OK ? SM_TOO_LARGE : stat, scale[2 * (size_t)q], scale[2 * (size_t)q + 1]);   // OK: until its launch has run
    }
    if ((rc = rd_resolve_budget(&budget_bytes, ctx->ws_align.cap))) return rc;
    const BudgetPlan plan = rd_plan_budget(n_q, nullptr, budget_bytes, 0, false,
                                           [&](int q, int) { return status[q] == SM_TOO_LARGE ? sm_bytes_of(c, q) : (int64_t)-1; },
                                           [](int, int, int64_t count, int64_t) { return count >= SM_MAX_LAUNCH; });
    if (plan.max_bytes && ctx->ws_align.reserve_exact((size_t)plan.max_bytes, "rd_sigmap")) return RD_ERR_NOMEM;
    std::vector<SmQuery> desc;
    std::vector<SmStripe> stripes;
    std::vector<SmOut> h_out;
    for (auto [k0, k1] : plan.launches) {
        const int nb = (int)(k1 - k0);
        const int32_t* members = plan.run.data() + k0;
        desc.resize(nb);
        stripes.clear();
        Carve ws;   // (dry: the descriptors hold offsets into ws_align)
        int64_t max_T = 0;
        for (int i = 0; i < nb; i++) {
            const int q = members[i];
            SmQuery& d = desc[i];
            const int64_t T = q_hi[q] - q_lo[q], n = s_hi[q] - s_lo[q];
            int32_t j_lo;
            const int64_t n_j = sm_target_span(c, q, &j_lo);
            d = SmQuery{q_lo[q] - lo, 0, 0, 0, (int32_t)T, m2[q], d4[q], (int32_t)s_lo[q], j_lo, (int32_t)n_j, {0, 0}};
            d.zq = (int64_t)ws.mark();
            ws.take<int32_t>((size_t)T);
            d.org = (int64_t)ws.mark();
            ws.take<int32_t>((size_t)n);
            d.key = (int64_t)ws.mark();
            ws.take<int64_t>((size_t)n_j);
            const bool cols = std::min<int64_t>(n, SM_PAYLOAD + T - 1) > SM_BAND;
            for (int64_t a = s_lo[q]; a < s_hi[q]; a += SM_PAYLOAD) {
                stripes.push_back(SmStripe{(int64_t)ws.mark(), i, (int32_t)sm_stripe_left(a, T, s_lo[q]), (int32_t)a, (int32_t)std::min<int64_t>(a + SM_PAYLOAD, s_hi[q])});
                if (cols) ws.take<int64_t>(2 * (size_t)T);
            }
            max_T = std::max(max_T, T);
        }
        if ((rc = rd_carve_check("rd_sigmap", ws, ctx->ws_align.cap))) return rc;
        SmIo io;
        if (rd_carve(ctx->ws_eval, [&](Carve& c) { sm_io_layout(c, nb, stripes.size(), &io); })) return RD_ERR_NOMEM;
        uint8_t* dws = ctx->ws_align.as<uint8_t>();
        RD_HIP(hipMemcpyAsync(io.qs, desc.data(), (size_t)nb * sizeof(SmQuery), hipMemcpyHostToDevice, st));
        RD_HIP(hipMemcpyAsync(io.str, stripes.data(), stripes.size() * sizeof(SmStripe), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(sm_quant_kernel, dim3((unsigned)((max_T + 255) / 256), nb), dim3(256), 0, st, io.qs, d_raw, dws);
        RD_HIP(hipGetLastError());
        hipLaunchKernelGGL(sm_dp_kernel, dim3((unsigned)stripes.size()), dim3(BS_NT), 0, st, io.qs, io.str, panel.kid, panel.tg, d_lvl, d_w, d_bias, dws);
        RD_HIP(hipGetLastError());
        hipLaunchKernelGGL(sm_select_kernel, dim3(nb), dim3(64), 0, st, io.qs, panel.off, dws, n_best, io.out);
        RD_HIP(hipGetLastError());
        h_out.resize(nb);
        RD_HIP(hipMemcpyAsync(h_out.data(), io.out, (size_t)nb * sizeof(SmOut), hipMemcpyDeviceToHost, st));
        RD_HIP(hipStreamSynchronize(st));
        for (int i = 0; i < nb; i++) {
            const int q = members[i];
            status[q] = SM_OK;
            for (int r = 0; r < n_best; r++) {
                const int64_t o = (int64_t)q * n_best + r;
                best_tgt[o] = h_out[i].tgt[r];
                best_score[o] = h_out[i].score[r];
                best_end[o] = h_out[i].end[r];
                best_org[o] = h_out[i].org[r];
            }
        }
    }
    if (plan.too_large) {
        const int q = (int)plan.first_too_large;
        rd_set_error("rd_sigmap: query %d (%lld samples x %lld states) needs %lld bytes of workspace, over the budget of %lld; %d query(ies) not "
                     "mapped (status RD_SIGMAP_TOO_LARGE), the others were", q, (long long)(q_hi[q] - q_lo[q]), (long long)(s_hi[q] - s_lo[q]),
                     (long long)sm_bytes_of(c, q), (long long)budget_bytes, (int)plan.too_large);
        return RD_ERR_NOMEM;
    }
    return RD_OK;
}
#endif  // __HIPCC__
