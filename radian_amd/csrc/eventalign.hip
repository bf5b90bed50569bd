// eventalign.hip -- raw samples against a k-mer pore model: the Viterbi path of a reference span through a read's window of samples, the
// samples every base sits on, their event table and the sums a rescaling needs.  No neural network takes part.  DESIGN.md section 24.
//
// Contract (integer arithmetic only, met exactly; include/radian_hip.h, rd_eventalign; the rules themselves are eventalign_rules.h).  A
// window of T samples x, L bases, a scale (m2, d4), a model (lvl, w, bias per k-mer and for the background):
//   zq[t]     = clamp(floor((2 u + d4) / (2 d4)), +-2^14), u = 512 (2 x[t] - m2): the sample in MAD/256
//   states    s = 0 .. L + 1: 0 the lead and L + 1 the trail (background), s in 1 .. L base s - 1 by its k-mer
//   c(t, s)   = min(floor((zq[t] - lvl(s))^2 w(s) / 2^32), 1024) + bias(s)
//   V[0][0]   = c(0, 0), V[0][1] = c(0, 1); V[t][s] = c(t, s) + min(V[t-1][s], V[t-1][s-1]), the advance only if STRICTLY smaller (bit 1)
//   end       = state L + 1, or L if V[T-1][L+1] is not strictly smaller; score = that value
//
// Kernels, on one stream:
//   signal_scale_kernel   (signal_dev.h) once per call, one 256-thread workgroup per read: the scale as given, or the window's own by
//                     radix_select2 (select.h) twice, as pa_scale_kernel
//   per launch (a set of reads whose workspace fits the budget):
//   ea_quant_kernel   zq rows, one int32 per sample
//   ea_dp_kernel      one workgroup per read: band_sweep.h's sweep.  A thread's registers: value, level, weight and bias of its 16
//                     states; a 4-byte cell crosses a thread boundary; a tile is 128 rows of zq and of the incoming column.
//                     Back-pointers: 1 bit per cell, a thread's 16 cells = one uint16, a wave's 64 stores = 128 consecutive bytes, a
//                     row = 4 ceil((L + 2) / 32) bytes.  Band b > 0 starts at row 4096 b - 1: the cells above (s > t + 1) are
//                     unreachable.  Unreachable cells are computed unmasked from 2^30: they stay above 2^30 - 2^19 * 256, every finite
//                     value stays below 2^19 * 1280, so none ever wins.
//   ea_tb_kernel      one wave per read: end state, score, then the walk, 64 rows at a time -- lane r holds row t - r's two words (the one
//                     of the path's state and the one below), a ballot of the state's bit over the rows not yet walked finds the nearest
//                     row the state was entered at, and the state moves down; the path dwells tens of rows per state, so a step of the
//                     walk is a transition, not a row.  Steps are stored in read coordinates (t_lo added).
//   ev_stats_kernel   events.hip's, on the steps while the samples are on the device
//   ea_sums_kernel    one workgroup per read: N, sum l, sum l^2, sum x, sum x l over its events (int64 adds: any order gives the same)
// No floating point, no atomics but the select's LDS histogram, no scratch.  A read's result does not depend on its launch's other reads.
//
// rd_eventalign_events is the same Viterbi over event rows: a row is one of rd_segment's events, weighted by its
// sample count, and a third predecessor skips one base.  Per launch: ear_row_kernel (n, mean and zq per event), ear_dp_kernel (a fourth
// policy of band_sweep.h: the cell that crosses a thread boundary is the thread's last TWO states, Cell2; two bits per back-pointer, a
// thread's 16 cells = one uint32, a wave's 64 stores = 256 consecutive bytes; band b > 0 starts at row 2048 b), ear_tb_kernel (one wave
// per read, 64 rows of back-pointer words staged in LDS, a row a step), ear_reduce_kernel (one lane per base over its rows' records) and
// ea_sums_kernel as it is.
//
// rd_eventalign_banded is rd_eventalign over a window of 64 states that slides with a per-base guide: eab_rows_kernel
// (zq, the window's lowest state per row, the states' constants), eab_dp_kernel (one wave per read, state s in lane s & 63, no band_sweep.h),
// eab_tb_kernel (ea_tb_kernel's walk on one 64-bit word a row), eab_edge_kernel (the bases on the window's rim), then ev_stats_kernel and
// ea_sums_kernel as they are.
//
// The two row kinds differ in their DP (one predecessor or two, one back-pointer bit or two) and in their traceback (a ballot walk or an
// LDS walk); DESIGN.md section 28 says why.  What surrounds the DPs exists once (section 29): EaBases, the bases side of a call with its
// checks, blank outputs and host fit sums; EaBand, the read fields and thread registers of both sweep policies; EaIo, the launch's io
// block; and the helpers the two launch loops call to place a read's workspace, fetch the block, scatter a member and report a read
// over the budget.
#include "common.h"
#include "budget.h"
#include "eventalign_rules.h"
#include "eventalign_host.h"
#include "../../include/radian_hip.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace {

struct EaModel {
    int k;
    const int32_t* lvl;
    const uint32_t* w;
    const int32_t* bias;
    EaState bg;
};

// the bases side of a call, the same for sample rows and event rows: first / last are steps (samples) or rows (events)
struct EaBases {
    const uint8_t* codes;
    const int64_t* ref_off;
    const int32_t *ref_len, *m2_in, *d4_in;
    EaModel m;
    int32_t* status;
    int64_t* score;
    int32_t *first, *last, *ev_start, *ev_end;
    int64_t *ev_sum, *ev_sumsq;
    int16_t *ev_min, *ev_max;
    int64_t* fit_sums;
};

struct EaCall {
    const int16_t* raw;
    const int64_t *read_off, *t_lo, *t_hi;
    int n_reads;
    EaBases b;
    int32_t *m2, *d4;
};

int ea_check_model(const char* who, const EaModel& m)
{
    RD_REQUIRE(sim_k_ok(m.k), "%s: k = %d, not odd and 1..9", who, m.k);
    RD_REQUIRE(m.lvl && m.w && m.bias, "%s: null model table", who);
    const int64_t n_kmers = (int64_t)1 << (2 * m.k);
    for (int64_t i = 0; i < n_kmers; i++)
        RD_REQUIRE(ea_entry_ok(m.lvl[i], m.bias[i]), "%s: model entry %lld (lvl %d, bias %d) is outside |lvl| < 2^14, |bias| <= 256", who,
                   (long long)i, m.lvl[i], m.bias[i]);
    RD_REQUIRE(ea_entry_ok(m.bg.lvl, m.bg.bias), "%s: the background (lvl %d, bias %d) is outside |lvl| < 2^14, |bias| <= 256", who, m.bg.lvl, m.bg.bias);
    return RD_OK;
}

// read r's bases and scale; *end: where the bases of the reads before it end, then where its own do
int ea_check_read_bases(const char* who, const EaBases& b, int r, int64_t* end)
{
    RD_REQUIRE(b.ref_len[r] >= 0 && b.ref_len[r] < (1 << 29), "%s: read %d has %d bases", who, r, b.ref_len[r]);
    RD_REQUIRE(b.ref_off[r] >= *end, "%s: base offsets must be non-decreasing and the reads' bases must not overlap (read %d)", who, r);
    RD_REQUIRE(ea_scale_ok(b.m2_in[r], b.d4_in[r]), "%s: read %d: the scale (m2 %d, d4 %d) is outside |m2| <= 2^17, 0 <= d4 <= 2^20", who, r,
               b.m2_in[r], b.d4_in[r]);
    *end = b.ref_off[r] + b.ref_len[r];
    return RD_OK;
}

// the per-base buffers and the codes of a call with n_bases bases, after every read has passed
int ea_check_codes(const char* who, const EaBases& b, int n_reads, int64_t n_bases)
{
    if (!n_bases) return RD_OK;
    RD_REQUIRE(b.codes && b.first && b.last && b.ev_start && b.ev_end && b.ev_sum && b.ev_sumsq && b.ev_min && b.ev_max,
               "%s: null code or per-base buffer", who);
    for (int r = 0; r < n_reads; r++)
        for (int i = 0; i < b.ref_len[r]; i++)
            RD_REQUIRE(b.codes[b.ref_off[r] + i] < 4, "%s: base %d of read %d is %d, not in 0..3", who, i, r, b.codes[b.ref_off[r] + i]);
    return RD_OK;
}

int ea_check_args(const char* who, const EaCall& c, int64_t* n_bases)
{
    *n_bases = 0;
    RD_REQUIRE(c.n_reads >= 0, "%s: negative n_reads", who);
    if (int rc = ea_check_model(who, c.b.m)) return rc;
    if (c.n_reads == 0) return RD_OK;
    RD_REQUIRE(c.raw && c.read_off && c.t_lo && c.t_hi && c.b.ref_off && c.b.ref_len && c.b.m2_in && c.b.d4_in, "%s: null argument", who);
    RD_REQUIRE(c.b.status && c.b.score && c.m2 && c.d4 && c.b.fit_sums, "%s: null output", who);
    RD_REQUIRE(c.read_off[0] >= 0, "%s: negative read offset", who);
    for (int r = 0; r < c.n_reads; r++) {
        const int64_t n = c.read_off[r + 1] - c.read_off[r];
        RD_REQUIRE(n >= 0, "%s: read offsets must be non-decreasing (read %d)", who, r);
        RD_REQUIRE(n <= INT32_MAX, "%s: read %d has more than 2^31 - 1 samples", who, r);
        RD_REQUIRE(0 <= c.t_lo[r] && c.t_lo[r] <= c.t_hi[r] && c.t_hi[r] <= n, "%s: read %d: the window [%lld, %lld) is outside its %lld samples", who,
                   r, (long long)c.t_lo[r], (long long)c.t_hi[r], (long long)n);
        if (int rc = ea_check_read_bases(who, c.b, r, n_bases)) return rc;
    }
    return ea_check_codes(who, c.b, c.n_reads, *n_bases);
}

// the "no path" outputs of read r with this status; the caller adds its row kind's own fields
void ea_blank(const EaBases& b, int r, int status)
{
    b.status[r] = status;
    b.score[r] = 0;
    for (int i = 0; i < 5; i++) b.fit_sums[5 * (int64_t)r + i] = 0;
    const int64_t o = b.ref_off[r];
    for (int i = 0; i < b.ref_len[r]; i++) {
        b.first[o + i] = b.last[o + i] = b.ev_start[o + i] = b.ev_end[o + i] = -1;
        b.ev_sum[o + i] = b.ev_sumsq[o + i] = 0;
        b.ev_min[o + i] = b.ev_max[o + i] = 0;
    }
}
void ea_blank(const EaCall& c, int r, int status, int32_t m2, int32_t d4)
{
    ea_blank(c.b, r, status);
    c.m2[r] = m2;
    c.d4[r] = d4;
}

// the five fit sums of an OK read from its events (a skipped base has no samples and no sum: it adds nothing)
void ea_host_sums(const EaBases& c, int r)
{
    const int64_t o = c.ref_off[r];
    const int32_t L = c.ref_len[r];
    int64_t* s = c.fit_sums + 5 * (int64_t)r;
    for (int32_t b = 0; b < L; b++) {
        const int64_t l = c.m.lvl[sim_kmer(c.codes + o, L, b, c.m.k)], n = c.ev_end[o + b] - c.ev_start[o + b], x = c.ev_sum[o + b];
        s[0] += n;
        s[1] += n * l;
        s[2] += n * l * l;
        s[3] += x;
        s[4] += x * l;
    }
}

// the L + 2 states of read r
void ea_host_states(const EaBases& b, int r, std::vector<EaState>& st)
{
    const int32_t L = b.ref_len[r];
    st.resize((size_t)L + 2);
    for (int32_t s = 0; s < L + 2; s++) st[s] = ea_state(s, L, b.codes + b.ref_off[r], b.m.k, b.m.lvl, b.m.w, b.m.bias, b.m.bg);
}

size_t ea_zq_bytes(int64_t T) { return align_up((size_t)T * 4, 256); }
size_t ea_bp_bytes(int64_t T, int64_t L) { return align_up((size_t)T * (size_t)((L + 2 + 31) / 32) * 4, 256); }
size_t ea_col_bytes(int64_t T, int64_t L) { return L + 2 > 4096 ? align_up((size_t)T * 8, 256) : 0; }
size_t ea_read_bytes(int64_t T, int64_t L) { return ea_zq_bytes(T) + ea_bp_bytes(T, L) + ea_col_bytes(T, L); }

}  // namespace

extern "C" int64_t rd_eventalign_workspace_bytes(int64_t n_rows, int64_t n_bases)
{
    if (n_rows < 0 || n_bases < 0) return -1;
    return (int64_t)ea_read_bytes(n_rows, n_bases);
}

extern "C" int rd_eventalign_host(const int16_t* raw, const int64_t* read_off, int n_reads, const int64_t* t_lo, const int64_t* t_hi,
                                  const uint8_t* codes, const int64_t* ref_off, const int32_t* ref_len, const int32_t* m2_in, const int32_t* d4_in,
                                  int k, const int32_t* lvl, const uint32_t* w, const int32_t* bias, int32_t lvl_bg, uint32_t w_bg, int32_t bias_bg,
                                  int32_t* status, int64_t* score, int32_t* m2, int32_t* d4, int32_t* first_step, int32_t* last_step,
                                  int32_t* ev_start, int32_t* ev_end, int64_t* ev_sum, int64_t* ev_sumsq, int16_t* ev_min, int16_t* ev_max,
                                  int64_t* fit_sums)
{
    const EaCall c{raw, read_off, t_lo, t_hi, n_reads,
                   EaBases{codes, ref_off, ref_len, m2_in, d4_in, EaModel{k, lvl, w, bias, EaState{lvl_bg, w_bg, bias_bg}}, status, score, first_step,
                           last_step, ev_start, ev_end, ev_sum, ev_sumsq, ev_min, ev_max, fit_sums},
                   m2, d4};
    int64_t n_bases = 0;
    int rc = ea_check_args("rd_eventalign_host", c, &n_bases);
    if (rc || n_reads == 0) return rc;
    std::vector<int64_t> cnt;
    std::vector<int32_t> zq, V, ev_status(n_reads);
    std::vector<EaState> st;
    std::vector<uint8_t> bp;
    for (int r = 0; r < n_reads; r++) {
        const int64_t T = t_hi[r] - t_lo[r], L = ref_len[r], S = L + 2, o = ref_off[r];
        const int16_t* x = raw + read_off[r] + t_lo[r];
        int32_t um2 = m2_in[r], ud4 = d4_in[r];
        ev_status[r] = 1;
        if (T <= 0 || T > EA_MAX_T) {
            ea_blank(c, r, ea_status(T, L, 1), 0, 0);
            continue;
        }
        if (ud4 == 0) ea_host_scale(x, T, cnt, &um2, &ud4);
        const int stat = ea_status(T, L, ud4);
        ea_blank(c, r, stat, um2, ud4);
        if (stat != EA_OK) continue;
        ev_status[r] = 0;
        zq.resize(T);
        for (int64_t t = 0; t < T; t++) zq[t] = ea_quant(x[t], um2, ud4);
        ea_host_states(c.b, r, st);
        V.assign(S, EA_INF);
        bp.assign((size_t)((T * S + 7) / 8), 0);
        V[0] = ea_cost(zq[0], st[0].lvl, st[0].w, st[0].bias);
        V[1] = ea_cost(zq[0], st[1].lvl, st[1].w, st[1].bias);
        for (int64_t t = 1; t < T; t++) {
            const int64_t top = t + 1 < S - 1 ? t + 1 : S - 1;   // cells with s > t + 1 stay unreachable
            for (int64_t s = top; s >= 0; s--) {
                int32_t best = V[s];
                if (s > 0 && ea_advance(V[s], V[s - 1])) {
                    best = V[s - 1];
                    bp[(size_t)((t * S + s) >> 3)] |= (uint8_t)(1u << ((t * S + s) & 7));
                }
                V[s] = ea_cost(zq[t], st[s].lvl, st[s].w, st[s].bias) + best;
            }
        }
        int64_t s = ea_ends_in_trail(V[L + 1], V[L]) ? L + 1 : L;
        score[r] = V[s];
        const int32_t off = (int32_t)t_lo[r];
        if (s >= 1 && s <= L) last_step[o + s - 1] = (int32_t)(T - 1) + off;
        for (int64_t t = T - 1; t > 0; t--) {
            if (!((bp[(size_t)((t * S + s) >> 3)] >> ((t * S + s) & 7)) & 1)) continue;
            if (s <= L) first_step[o + s - 1] = (int32_t)t + off;
            if (s - 1 >= 1) last_step[o + s - 2] = (int32_t)t - 1 + off;
            s--;
        }
        if (s == 1 && L >= 1) first_step[o] = off;
    }
    if (n_bases &&
        (rc = rd_event_stats_host(raw, read_off, n_reads, first_step, last_step, ref_off, ref_len, ev_status.data(), ev_start, ev_end, ev_sum, ev_sumsq,
                                  ev_min, ev_max)))
        return rc;
    for (int r = 0; r < n_reads; r++)
        if (status[r] == EA_OK) ea_host_sums(c.b, r);
    return RD_OK;
}

// ------------------------------------------------------------------------------------------------------------------ event rows
// rd_eventalign_events (include/radian_hip.h): the same Viterbi, but a row is one of the detector's events (rd_segment's
// records as they are; no raw sample is read), weighted by its sample count, and a third predecessor skips one base:
//   n_e = start[e+1] - start[e] (the window's T closes the last), x_e = floor((2 sum_e + n_e) / (2 n_e)), zq_e = ea_quant(x_e, m2, d4)
//   c(e, s) = n_e * ea_cost(zq_e, s);  V[e][s] = c(e, s) + ear_best(V[e-1][s], V[e-1][s-1], V[e-1][s-2] + skip_pen): two bits per cell
// Only the events side of the call and its checks are here: the bases side, the blank outputs, the state table and the fit sums are EaBases'.
namespace {

struct EarCall {
    int n_reads;
    const int64_t *n_samples, *sample_off, *ev_off;
    const int32_t* n_events;
    const int32_t* in_start;
    const int64_t *in_sum, *in_sumsq;
    const int16_t *in_min, *in_max;
    int skip_pen;
    EaBases b;
    int32_t* n_skipped;
};

int ear_check_args(const char* who, const EarCall& c, int64_t* n_bases)
{
    *n_bases = 0;
    RD_REQUIRE(c.n_reads >= 0, "%s: negative n_reads", who);
    if (int rc = ea_check_model(who, c.b.m)) return rc;
    RD_REQUIRE(ear_pen_ok(c.skip_pen), "%s: skip_pen = %d, not -1 (no skips) or 0..256", who, c.skip_pen);
    if (c.n_reads == 0) return RD_OK;
    RD_REQUIRE(c.n_samples && c.sample_off && c.ev_off && c.n_events && c.b.ref_off && c.b.ref_len && c.b.m2_in && c.b.d4_in, "%s: null argument", who);
    RD_REQUIRE(c.b.status && c.b.score && c.n_skipped && c.b.fit_sums, "%s: null output", who);
    for (int r = 0; r < c.n_reads; r++) {
        const int64_t T = c.n_samples[r], E = c.n_events[r];
        RD_REQUIRE(T >= 0 && c.sample_off[r] >= 0 && T <= INT32_MAX && c.sample_off[r] <= INT32_MAX - T,
                   "%s: read %d: %lld samples from %lld on do not fit 0 .. 2^31 - 1", who, r, (long long)T, (long long)c.sample_off[r]);
        RD_REQUIRE(E >= 0 && c.ev_off[r] >= 0, "%s: read %d: negative event count or offset", who, r);
        if (int rc = ea_check_read_bases(who, c.b, r, n_bases)) return rc;
        if (E == 0) continue;
        RD_REQUIRE(c.in_start && c.in_sum && c.in_sumsq && c.in_min && c.in_max, "%s: null event array", who);
        const int32_t* s = c.in_start + c.ev_off[r];
        RD_REQUIRE(s[0] == 0, "%s: read %d: event 0 starts at sample %d, not 0", who, r, s[0]);
        for (int64_t e = 0; e < E; e++) {
            RD_REQUIRE(s[e] < T && (e == 0 || s[e] > s[e - 1]), "%s: read %d: event %lld starts at sample %d: not after the event before it, or not inside the %lld samples",
                       who, r, (long long)e, s[e], (long long)T);
            const int64_t n = (e + 1 < E ? (int64_t)s[e + 1] : T) - s[e], sum = c.in_sum[c.ev_off[r] + e];   // (n <= 0 is refused at e + 1)
            if (n <= 0) continue;
            RD_REQUIRE(sum >= -32768 * n && sum <= 32767 * n && ear_mean(sum, n) <= 32767, "%s: read %d: the mean of event %lld (sum %lld over %lld samples) does not fit int16",
                       who, r, (long long)e, (long long)sum, (long long)n);
        }
    }
    return ea_check_codes(who, c.b, c.n_reads, *n_bases);
}

void ear_blank(const EarCall& c, int r, int status)
{
    ea_blank(c.b, r, status);
    c.n_skipped[r] = 0;
}

size_t ear_row_bytes(int64_t E) { return align_up((size_t)E * 8, 256); }
size_t ear_bp_bytes(int64_t E, int64_t L) { return align_up((size_t)E * (size_t)((L + 2 + 15) / 16) * 4, 256); }
size_t ear_col_bytes(int64_t E, int64_t L) { return L + 2 > 4096 ? align_up((size_t)E * 16, 256) : 0; }
size_t ear_read_bytes(int64_t E, int64_t L) { return ear_row_bytes(E) + ear_bp_bytes(E, L) + ear_col_bytes(E, L); }

}  // namespace

extern "C" int64_t rd_eventalign_events_workspace_bytes(int64_t n_rows, int64_t n_bases)
{
    if (n_rows < 0 || n_bases < 0) return -1;
    return (int64_t)ear_read_bytes(n_rows, n_bases);
}

extern "C" int rd_eventalign_events_host(int n_reads, const int64_t* n_samples, const int64_t* sample_off, const int64_t* ev_off, const int32_t* n_events,
                                         const int32_t* in_start, const int64_t* in_sum, const int64_t* in_sumsq, const int16_t* in_min,
                                         const int16_t* in_max, const uint8_t* codes, const int64_t* ref_off, const int32_t* ref_len,
                                         const int32_t* m2_in, const int32_t* d4_in, int k, const int32_t* lvl, const uint32_t* w, const int32_t* bias,
                                         int32_t lvl_bg, uint32_t w_bg, int32_t bias_bg, int skip_pen, int32_t* status, int64_t* score,
                                         int32_t* n_skipped, int32_t* row_first, int32_t* row_last, int32_t* ev_start, int32_t* ev_end, int64_t* ev_sum,
                                         int64_t* ev_sumsq, int16_t* ev_min, int16_t* ev_max, int64_t* fit_sums)
{
    const EarCall c{n_reads, n_samples, sample_off, ev_off, n_events, in_start, in_sum, in_sumsq, in_min, in_max, skip_pen,
                    EaBases{codes, ref_off, ref_len, m2_in, d4_in, EaModel{k, lvl, w, bias, EaState{lvl_bg, w_bg, bias_bg}}, status, score, row_first,
                            row_last, ev_start, ev_end, ev_sum, ev_sumsq, ev_min, ev_max, fit_sums},
                    n_skipped};
    int64_t n_bases = 0;
    const int rc = ear_check_args("rd_eventalign_events_host", c, &n_bases);
    if (rc || n_reads == 0) return rc;
    const bool skips = skip_pen >= 0;
    std::vector<int32_t> zq, nn, V;
    std::vector<EaState> st;
    std::vector<uint32_t> bp;
    for (int r = 0; r < n_reads; r++) {
        const int64_t T = n_samples[r], E = n_events[r], L = ref_len[r], S = L + 2, o = ref_off[r], eo = ev_off[r], wpr = (S + 15) / 16;
        const int stat = ear_status(T, E, L, d4_in[r], skip_pen);
        ear_blank(c, r, stat);
        if (stat != EA_OK) continue;
        const int32_t off = (int32_t)sample_off[r];
        const auto row_end = [&](int64_t e) { return e + 1 < E ? in_start[eo + e + 1] : (int32_t)T; };   // the sample behind row e
        zq.resize(E);
        nn.resize(E);
        for (int64_t e = 0; e < E; e++) {
            nn[e] = row_end(e) - in_start[eo + e];
            zq[e] = ea_quant((int32_t)ear_mean(in_sum[eo + e], nn[e]), m2_in[r], d4_in[r]);
        }
        ea_host_states(c.b, r, st);
        V.assign(S, EA_INF);
        bp.assign((size_t)(E * wpr), 0);
        V[0] = ear_cost(zq[0], nn[0], st[0].lvl, st[0].w, st[0].bias);
        V[1] = ear_cost(zq[0], nn[0], st[1].lvl, st[1].w, st[1].bias);
        for (int64_t e = 1; e < E; e++) {
            const int64_t reach = skips ? 2 * e + 1 : e + 1, top = reach < S - 1 ? reach : S - 1;   // the cells above stay unreachable
            for (int64_t s = top; s >= 0; s--) {
                int code;
                const int32_t best = ear_best(V[s], s >= 1 ? V[s - 1] : EA_INF, (s >= 2 ? V[s - 2] : EA_INF) + (skips ? skip_pen : 0), skips, &code);
                bp[(size_t)(e * wpr + (s >> 4))] |= (uint32_t)code << (2 * (s & 15));
                V[s] = ear_cost(zq[e], nn[e], st[s].lvl, st[s].w, st[s].bias) + best;
            }
        }
        int64_t s = ea_ends_in_trail(V[L + 1], V[L]) ? L + 1 : L;
        score[r] = V[s];
        // the walk: row_first of a skipped base holds -2 - (the row at which the path jumped over it) until the reduce below
        if (s >= 1 && s <= L) row_last[o + s - 1] = (int32_t)(E - 1);
        for (int64_t e = E - 1; e > 0 && s > 0; e--) {
            const int code = (int)((bp[(size_t)(e * wpr + (s >> 4))] >> (2 * (s & 15))) & 3);
            if (code == EAR_STAY) continue;
            if (s <= L) row_first[o + s - 1] = (int32_t)e;
            if (code == EAR_SKIP) {
                row_first[o + s - 2] = (int32_t)(-2 - e);
                n_skipped[r]++;
            }
            if (s - code >= 1) row_last[o + s - code - 1] = (int32_t)(e - 1);
            s -= code;
        }
        if (s == 1 && L >= 1) row_first[o] = 0;
        for (int64_t b = 0; b < L; b++) {
            const int32_t f = row_first[o + b], l = row_last[o + b];
            if (f <= -2) {
                ev_start[o + b] = ev_end[o + b] = in_start[eo + (-2 - f)] + off;
                row_first[o + b] = row_last[o + b] = -1;
                continue;
            }
            int64_t sum = 0, sq = 0;
            int16_t mn = in_min[eo + f], mx = in_max[eo + f];
            for (int64_t e = f; e <= l; e++) {
                sum += in_sum[eo + e];
                sq += in_sumsq[eo + e];
                mn = std::min(mn, in_min[eo + e]);
                mx = std::max(mx, in_max[eo + e]);
            }
            ev_start[o + b] = in_start[eo + f] + off;
            ev_end[o + b] = row_end(l) + off;
            ev_sum[o + b] = sum;
            ev_sumsq[o + b] = sq;
            ev_min[o + b] = mn;
            ev_max[o + b] = mx;
        }
        ea_host_sums(c.b, r);
    }
    return RD_OK;
}

// ------------------------------------------------------------------------------------------------------------------ sample rows in a band
// rd_eventalign_banded (include/radian_hip.h): rd_eventalign's rows, cost and tie-break over the EAB_W states of a
// window that slides with a per-base guide (eventalign_rules.h: eab_count, eab_lo).  A state outside the row's window does not exist: the
// window's lowest state has no advance edge, a state that entered the window this row has no stay edge.  One 64-bit back-pointer word a
// row, bit s & 63.  Only the guide, the window and the rim count are here: everything else is EaCall's.
namespace {

int eab_check_guide(const char* who, const EaCall& c, const int32_t* guide, int32_t* n_edge, int64_t n_bases)
{
    if (c.n_reads == 0) return RD_OK;
    RD_REQUIRE(n_edge, "%s: null output", who);
    RD_REQUIRE(guide || !n_bases, "%s: null guide", who);
    for (int r = 0; r < c.n_reads; r++)
        for (int i = 1; i < c.b.ref_len[r]; i++)
            RD_REQUIRE(guide[c.b.ref_off[r] + i] >= guide[c.b.ref_off[r] + i - 1], "%s: the guide of read %d decreases at base %d", who, r, i);
    return RD_OK;
}

size_t eab_lo_bytes(int64_t T) { return align_up((size_t)T * 4, 256); }
size_t eab_bp_bytes(int64_t T) { return align_up((size_t)T * 8, 256); }
int64_t eab_tab_entries(int64_t L) { return L + 2 + 2 * EAB_W; }   // a lane prefetches the constants of its state + 64
size_t eab_tab_bytes(int64_t L) { return align_up((size_t)eab_tab_entries(L) * 12, 256); }
size_t eab_read_bytes(int64_t T, int64_t L) { return ea_zq_bytes(T) + eab_bp_bytes(T) + eab_lo_bytes(T) + eab_tab_bytes(L); }

}  // namespace

extern "C" int64_t rd_eventalign_banded_workspace_bytes(int64_t n_rows, int64_t n_bases)
{
    if (n_rows < 0 || n_bases < 0) return -1;
    return (int64_t)eab_read_bytes(n_rows, n_bases);
}

extern "C" int rd_eventalign_banded_host(const int16_t* raw, const int64_t* read_off, int n_reads, const int64_t* t_lo, const int64_t* t_hi,
                                         const uint8_t* codes, const int64_t* ref_off, const int32_t* ref_len, const int32_t* guide,
                                         const int32_t* m2_in, const int32_t* d4_in, int k, const int32_t* lvl, const uint32_t* w, const int32_t* bias,
                                         int32_t lvl_bg, uint32_t w_bg, int32_t bias_bg, int32_t* status, int64_t* score, int32_t* m2, int32_t* d4,
                                         int32_t* n_edge, int32_t* first_step, int32_t* last_step, int32_t* ev_start, int32_t* ev_end, int64_t* ev_sum,
                                         int64_t* ev_sumsq, int16_t* ev_min, int16_t* ev_max, int64_t* fit_sums)
{
    const EaCall c{raw, read_off, t_lo, t_hi, n_reads,
                   EaBases{codes, ref_off, ref_len, m2_in, d4_in, EaModel{k, lvl, w, bias, EaState{lvl_bg, w_bg, bias_bg}}, status, score, first_step,
                           last_step, ev_start, ev_end, ev_sum, ev_sumsq, ev_min, ev_max, fit_sums},
                   m2, d4};
    int64_t n_bases = 0;
    int rc = ea_check_args("rd_eventalign_banded_host", c, &n_bases);
    if (!rc) rc = eab_check_guide("rd_eventalign_banded_host", c, guide, n_edge, n_bases);
    if (rc || n_reads == 0) return rc;
    std::vector<int64_t> cnt;
    std::vector<int32_t> zq, V, lo_t, ev_status(n_reads);
    std::vector<EaState> st;
    std::vector<uint64_t> bp;
    for (int r = 0; r < n_reads; r++) {
        const int64_t T = t_hi[r] - t_lo[r], L = ref_len[r], S = L + 2, o = ref_off[r];
        const int16_t* x = raw + read_off[r] + t_lo[r];
        int32_t um2 = m2_in[r], ud4 = d4_in[r];
        ev_status[r] = 1;
        n_edge[r] = 0;
        if (T <= 0 || T > EA_MAX_T) {
            ea_blank(c, r, ea_status(T, L, 1), 0, 0);
            continue;
        }
        if (ud4 == 0) ea_host_scale(x, T, cnt, &um2, &ud4);
        const int stat = ea_status(T, L, ud4);
        ea_blank(c, r, stat, um2, ud4);
        if (stat != EA_OK) continue;
        zq.resize(T);
        lo_t.resize(T);
        int64_t g = 0;
        for (int64_t t = 0; t < T; t++) {
            zq[t] = ea_quant(x[t], um2, ud4);
            while (g < L && guide[o + g] <= t_lo[r] + t) g++;
            lo_t[t] = eab_lo(g, L);
        }
        ea_host_states(c.b, r, st);
        V.assign(S, EA_INF);   // a state above every window so far still holds this
        bp.assign((size_t)T, 0);
        for (int64_t s = 0; s < 2; s++)
            if (s >= lo_t[0]) V[s] = ea_cost(zq[0], st[s].lvl, st[s].w, st[s].bias);   // (s <= 1 is below the window's top)
        for (int64_t t = 1; t < T; t++) {
            const int64_t lo = lo_t[t], hi = std::min<int64_t>(lo + EAB_W - 1, S - 1);
            for (int64_t s = hi; s >= lo; s--) {
                int32_t best = V[s];
                if (s > lo && ea_advance(V[s], V[s - 1])) {
                    best = V[s - 1];
                    bp[(size_t)t] |= (uint64_t)1 << (s & (EAB_W - 1));
                }
                V[s] = ea_cost(zq[t], st[s].lvl, st[s].w, st[s].bias) + best;
            }
        }
        const int64_t hi = std::min<int64_t>((int64_t)lo_t[T - 1] + EAB_W - 1, S - 1);
        const int32_t v_trail = L + 1 <= hi ? V[L + 1] : EA_INF, v_last = L <= hi ? V[L] : EA_INF;   // (the window never starts above L)
        int64_t s = ea_ends_in_trail(v_trail, v_last) ? L + 1 : L;
        const int32_t end = s == L + 1 ? v_trail : v_last;
        if (!eab_finite(end)) {
            status[r] = EA_OFF_BAND;
            continue;
        }
        ev_status[r] = 0;
        score[r] = end;
        const int32_t off = (int32_t)t_lo[r];
        if (s >= 1 && s <= L) last_step[o + s - 1] = (int32_t)(T - 1) + off;
        for (int64_t t = T - 1; t > 0; t--) {
            if (!((bp[(size_t)t] >> (s & (EAB_W - 1))) & 1)) continue;
            if (s <= L) first_step[o + s - 1] = (int32_t)t + off;
            if (s - 1 >= 1) last_step[o + s - 2] = (int32_t)t - 1 + off;
            s--;
        }
        if (s == 1 && L >= 1) first_step[o] = off;
        for (int64_t b = 0; b < L; b++)
            n_edge[r] += eab_on_rim((int32_t)b + 1, lo_t[last_step[o + b] - off], lo_t[first_step[o + b] - off]);
    }
    if (n_bases &&
        (rc = rd_event_stats_host(raw, read_off, n_reads, first_step, last_step, ref_off, ref_len, ev_status.data(), ev_start, ev_end, ev_sum, ev_sumsq,
                                  ev_min, ev_max)))
        return rc;
    for (int r = 0; r < n_reads; r++)
        if (status[r] == EA_OK) ea_host_sums(c.b, r);
    return RD_OK;
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------------------------------ device half
#include "band_sweep.h"
#include "signal_dev.h"

namespace {

constexpr int EA_MAX_LAUNCH = 32768;       // reads of one launch (grid.y of the row kernel)

struct EaSeq {
    int64_t raw0;    // the window's sample 0 in the raw buffer
    int64_t codes;   // the read's base 0 in the code buffer
    int64_t lab;     // its base 0 in the launch's per-base arrays
    int64_t zq, bp, col;   // byte offsets into the workspace
    int32_t T, L, m2, d4, t_lo, n_win;   // (n_win: the samples of the window when the rows are events, T of them; 0 otherwise)
};
struct EaOut {
    int64_t score, sums[5];
};

// grid (ceil(max T / 256), reads)
__global__ __launch_bounds__(256) void ea_quant_kernel(const EaSeq* __restrict__ seqs, const int16_t* __restrict__ raw, uint8_t* __restrict__ ws,
                                                       int32_t* __restrict__ fin)
{
    const EaSeq q = seqs[blockIdx.y];
    if (blockIdx.x == 0 && threadIdx.x < 2) fin[2 * (int64_t)blockIdx.y + threadIdx.x] = EA_INF;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= q.T) return;
    ((int32_t*)(ws + q.zq))[t] = ea_quant(raw[q.raw0 + t], q.m2, q.d4);
}

// What both band_sweep.h policies of this file hold besides their rows and back-pointers: the read, the thread's 16 states of the band,
// how a band starts and what it leaves
struct EaBand {
    // the read
    const uint8_t* cod;
    const int32_t* __restrict__ lvl_t;
    const uint32_t* __restrict__ w_t;
    const int32_t* __restrict__ bias_t;
    EaState bg;
    int32_t* fin;   // the read's two end values
    int k, L, S;
    // the thread's states of the band
    int s0;
    int32_t lv[BS_K], bi[BS_K], v[BS_K];
    uint32_t wt[BS_K];

    __device__ __forceinline__ void begin_band(int b)
    {
        s0 = b * BS_BAND + (int)threadIdx.x * BS_K;
#pragma unroll
        for (int j = 0; j < BS_K; j++) {
            EaState st{0, 0, 0};   // a state past the read: it costs nothing, its value stays where it starts
            if (s0 + j < S) st = ea_state(s0 + j, L, cod, k, lvl_t, w_t, bias_t, bg);
            lv[j] = st.lvl;
            wt[j] = st.w;
            bi[j] = st.bias;
            v[j] = EA_INF;
        }
        // row -1 of band 0: V = 0 in state 0 and unreachable elsewhere makes row 0 the contract's start, state 1 by the advance
        if (s0 == 0) v[0] = 0;
    }
    // the two states the path may end in
    __device__ __forceinline__ void end_band() const
    {
#pragma unroll
        for (int j = 0; j < BS_K; j++) {
            if (s0 + j == L + 1) fin[0] = v[j];
            if (s0 + j == L) fin[1] = v[j];
        }
    }
};

// band_sweep.h's policy of eventalign
struct EaSweep : EaBand {
    using Cell = int32_t;
    using Elem = int32_t;
    static constexpr bool AHEAD_CLAMPED = true;
    static constexpr int TR = 128, SLOTS = 2;   // a tile: [0: zq, 1: the band's incoming column value V[t-1][s_lo-1]][row]
    struct Row {
        int32_t z, c;
    };
    const int32_t* __restrict__ zq;
    uint16_t* __restrict__ bp;
    int hpr;   // 16-bit words of a back-pointer row

    static __device__ __forceinline__ int first_row(int b) { return b ? b * BS_BAND - 1 : 0; }   // rows above have s > t + 1 in the whole band
    static __device__ __forceinline__ Cell none() { return EA_INF; }
    static __device__ __forceinline__ Cell incoming(const Row& in) { return in.c; }
    __device__ __forceinline__ Cell last() const { return v[BS_K - 1]; }

    __device__ __forceinline__ Elem tile_elem(int e, int tbase, int T, int b, const Cell* cin) const
    {
        const int which = e / TR, t = tbase + (e % TR);
        Elem x = EA_INF;
        if (t < T) {
            if (which == 0) x = zq[t];
            else if (b > 0) x = cin[t - 1];   // t >= first_row(b) >= 1
        }
        return x;
    }
    __device__ __forceinline__ Row read_row(const Elem* tile, int r) const { return Row{tile[r], tile[TR + r]}; }
    __device__ __forceinline__ void row(int t, const Row& in, Cell left)
    {
        uint32_t bits = 0;
#pragma unroll
        for (int j = BS_K - 1; j >= 0; j--) {
            const int32_t adv = j >= 1 ? v[j - 1] : left;
            const bool take = ea_advance(v[j], adv);
            v[j] = ea_cost(in.z, lv[j], wt[j], bi[j]) + (take ? adv : v[j]);
            bits |= (take ? 1u : 0u) << j;
        }
        if (s0 < S) bp[(size_t)t * hpr + (s0 >> 4)] = (uint16_t)bits;
    }
};

__global__ __launch_bounds__(BS_NT) void ea_dp_kernel(const EaSeq* __restrict__ seqs, const uint8_t* __restrict__ codes, const int32_t* __restrict__ lvl_t,
                                                      const uint32_t* __restrict__ w_t, const int32_t* __restrict__ bias_t, EaState bg, int k,
                                                      uint8_t* __restrict__ ws, int32_t* __restrict__ fin)
{
    const EaSeq q = seqs[blockIdx.x];
    const int S = q.L + 2;
    EaSweep p{{codes + q.codes, lvl_t, w_t, bias_t, bg, fin + 2 * (int64_t)blockIdx.x, k, q.L, S},
              (const int32_t*)(ws + q.zq), (uint16_t*)(ws + q.bp), 2 * ((S + 31) / 32)};
    band_sweep(p, S, q.T, (int32_t*)(ws + q.col));
}

// one wave per read
__global__ __launch_bounds__(64) void ea_tb_kernel(const EaSeq* __restrict__ seqs, const uint8_t* __restrict__ ws, const int32_t* __restrict__ fin,
                                                   EaOut* __restrict__ out, int32_t* __restrict__ first, int32_t* __restrict__ last)
{
    const int p = blockIdx.x, lane = threadIdx.x;
    const EaSeq q = seqs[p];
    const int L = q.L, off = q.t_lo;
    const int32_t v_trail = fin[2 * (int64_t)p], v_last = fin[2 * (int64_t)p + 1];
    int s = ea_ends_in_trail(v_trail, v_last) ? L + 1 : L;   // (s, t and r0 below are the same in every lane)
    const uint32_t* __restrict__ bp = (const uint32_t*)(ws + q.bp);
    const int64_t wpr = (L + 2 + 31) / 32;
    int32_t* fs = first + q.lab;
    int32_t* ls = last + q.lab;
    int t = q.T - 1;
    if (lane == 0) {
        out[p].score = s == L + 1 ? v_trail : v_last;
        if (s >= 1 && s <= L) ls[s - 1] = t + off;
    }
    while (t > 0) {
        // lane r holds the two words of row t - r that the path can be in while it stays within 32 states below s's word
        const int n = t < 64 ? t : 64, w0 = s >> 5;
        uint32_t a = 0, b = 0;
        if (lane < n) {
            a = bp[(int64_t)(t - lane) * wpr + w0];
            if (w0 > 0) b = bp[(int64_t)(t - lane) * wpr + w0 - 1];
        }
        int r0 = 0;   // rows t .. t - r0 + 1 are walked
        while (r0 < n && s > 0 && (s >> 5) >= w0 - 1) {
            const uint32_t word = (s >> 5) == w0 ? a : b;
            const unsigned long long m = __ballot(lane >= r0 && lane < n && ((word >> (s & 31)) & 1u));
            if (m == 0) {   // the path stays in s for the rest of these rows
                r0 = n;
                break;
            }
            const int r1 = __ffsll((long long)m) - 1, tt = t - r1;   // the nearest row that was entered from s - 1
            if (lane == 0) {
                if (s <= L) fs[s - 1] = tt + off;
                if (s - 1 >= 1) ls[s - 2] = tt - 1 + off;
            }
            s--;
            r0 = r1 + 1;
        }
        if (s == 0) break;   // the lead: nothing is left to record
        t -= r0;
    }
    if (lane == 0 && s == 1 && L >= 1) fs[0] = off;
}

__global__ __launch_bounds__(256) void ea_sums_kernel(const EaSeq* __restrict__ seqs, const uint8_t* __restrict__ codes, const int32_t* __restrict__ lvl_t,
                                                      int k, const int32_t* __restrict__ ev_start, const int32_t* __restrict__ ev_end,
                                                      const int64_t* __restrict__ ev_sum, EaOut* __restrict__ out)
{
    __shared__ int64_t sh[4][5];
    const EaSeq q = seqs[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t a[5] = {0, 0, 0, 0, 0};
    for (int b = tid; b < q.L; b += 256) {
        const int64_t l = lvl_t[sim_kmer(codes + q.codes, q.L, b, k)], n = ev_end[q.lab + b] - ev_start[q.lab + b], x = ev_sum[q.lab + b];
        a[0] += n;
        a[1] += n * l;
        a[2] += n * l * l;
        a[3] += x;
        a[4] += x * l;
    }
#pragma unroll
    for (int i = 0; i < 5; i++) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) a[i] += __shfl_xor(a[i], d);
        if (lane == 0) sh[wave][i] = a[i];
    }
    __syncthreads();
    if (tid < 5) out[blockIdx.x].sums[tid] = sh[0][tid] + sh[1][tid] + sh[2][tid] + sh[3][tid];
}

// a launch's io block (ws_eval) for nb reads of nlab bases: descriptors | end values [2] | skip counts (n_skip of them: nb for event rows,
// none for sample rows, which moves nothing) | score and sums | first, last, start, end | sum, sumsq | min, max.  Arrays of one type
// follow each other at one stride, so the host fetches each type in one copy.
struct EaIo {
    EaSeq* seqs;
    int32_t *fin, *nskip;
    EaOut* out;
    int32_t *first, *last, *start, *end;
    int64_t *sum, *sumsq;
    int16_t *mn, *mx;
};
void ea_io_layout(Carve& c, int nb, int64_t nlab, int n_skip, EaIo* io)
{
    const size_t n = (size_t)nlab;
    io->seqs = c.take<EaSeq>((size_t)nb);
    io->fin = c.take<int32_t>((size_t)nb * 2);
    io->nskip = c.take<int32_t>((size_t)n_skip);
    io->out = c.take<EaOut>((size_t)nb);
    io->first = c.take<int32_t>(n, 16);
    io->last = c.take<int32_t>(n, 16);
    io->start = c.take<int32_t>(n, 16);
    io->end = c.take<int32_t>(n, 16);
    io->sum = c.take<int64_t>(n, 16);
    io->sumsq = c.take<int64_t>(n, 16);
    io->mn = c.take<int16_t>(n, 16);
    io->mx = c.take<int16_t>(n, 16);
}

// ---- event rows (rd_eventalign_events).  An EaSeq of these kernels: raw0 = the read's event 0 in the launch's event arrays, T = its rows
// (events), n_win = its window's samples, t_lo = what is added to a sample index; zq = the rows' block, E zq then E sample counts.
// Only what differs from sample rows is here: the event arrays, the four kernels and the sweep's rows.  Band state and io block are above.
struct EarEvents {
    int32_t* start;
    int64_t *sum, *sumsq;
    int16_t *mn, *mx;
};
void ear_events_layout(Carve& c, int64_t n_ev, EarEvents* ev)
{
    const size_t n = (size_t)n_ev;
    ev->start = c.take<int32_t>(n);
    ev->sum = c.take<int64_t>(n);
    ev->sumsq = c.take<int64_t>(n);
    ev->mn = c.take<int16_t>(n);
    ev->mx = c.take<int16_t>(n);
}

// grid (ceil(max E / 256), reads): n_e, x_e and zq_e of every event
__global__ __launch_bounds__(256) void ear_row_kernel(const EaSeq* __restrict__ seqs, const int32_t* __restrict__ ev_start, const int64_t* __restrict__ ev_sum,
                                                      uint8_t* __restrict__ ws, int32_t* __restrict__ fin)
{
    const EaSeq q = seqs[blockIdx.y];
    if (blockIdx.x == 0 && threadIdx.x < 2) fin[2 * (int64_t)blockIdx.y + threadIdx.x] = EA_INF;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= q.T) return;
    const int32_t s = ev_start[q.raw0 + e], n = (e + 1 < q.T ? ev_start[q.raw0 + e + 1] : q.n_win) - s;
    int32_t* rows = (int32_t*)(ws + q.zq);
    rows[e] = ea_quant((int32_t)ear_mean(ev_sum[q.raw0 + e], n), q.m2, q.d4);
    rows[q.T + e] = n;
}

// band_sweep.h's policy of eventalign on event rows: the cell that crosses a thread boundary is the thread's last TWO states
template <bool SKIPS>
struct EarSweep : EaBand {
    using Cell = Cell2;
    using Elem = int32_t;
    static constexpr bool AHEAD_CLAMPED = true;
    static constexpr int TR = 128, SLOTS = 4;   // a tile: [0: zq, 1: n, 2 and 3: the band's incoming pair V[e-1][s_lo-2], V[e-1][s_lo-1]][row]
    struct Row {
        int32_t z, n;
        Cell2 c;
    };
    const int32_t* __restrict__ zq;
    const int32_t* __restrict__ nn;
    uint32_t* __restrict__ bp;
    int wpr, pen;   // wpr: 32-bit words of a back-pointer row

    // Row e reaches the states up to 2 e + 1 (two per row from state 1 at row 0), so the band's first state 4096 b is first reachable at
    // row 2048 b, from states 4096 b - 1 and 4096 b - 2 of row 2048 b - 1: that is the first row whose incoming column is read, and band
    // b - 1, which starts at 2048 (b - 1), has written it.  At row 2048 b - 1 every state of the band is still unreachable: begin_band's
    // 2^30.  Without skips the same row is early (state 4096 b is reached at row 4096 b - 1), which costs rows of unreachable cells, no more.
    static __device__ __forceinline__ int first_row(int b) { return b * (BS_BAND / 2); }
    static __device__ __forceinline__ Cell none() { return Cell2{EA_INF, EA_INF}; }
    static __device__ __forceinline__ Cell incoming(const Row& in) { return in.c; }
    __device__ __forceinline__ Cell last() const { return Cell2{v[BS_K - 2], v[BS_K - 1]}; }

    __device__ __forceinline__ Elem tile_elem(int e, int tbase, int T, int b, const Cell* cin) const
    {
        const int which = e / TR, t = tbase + (e % TR);
        Elem x = EA_INF;
        if (t < T) {
            if (which == 0) x = zq[t];
            else if (which == 1) x = nn[t];
            else if (b > 0) x = which == 2 ? cin[t - 1].a : cin[t - 1].b;   // t >= first_row(b) >= 1
        }
        return x;
    }
    __device__ __forceinline__ Row read_row(const Elem* tile, int r) const { return Row{tile[r], tile[TR + r], Cell2{tile[2 * TR + r], tile[3 * TR + r]}}; }
    __device__ __forceinline__ void row(int t, const Row& in, Cell left)
    {
        uint32_t bits = 0;
        // begin_band's row -1 holds V = 0 in state 0.  A skip from that 0 would reach state 2 and beat its 2^30, so row 0 takes no skip edge
        const bool skips = SKIPS && t > 0;   // (wave-uniform)
#pragma unroll
        for (int j = BS_K - 1; j >= 0; j--) {
            const int32_t adv = j >= 1 ? v[j - 1] : left.b;
            const int32_t two = j >= 2 ? v[j - 2] : j == 1 ? left.b : left.a;
            int code;
            const int32_t best = ear_best(v[j], adv, two + pen, skips, &code);
            v[j] = ear_cost(in.z, in.n, lv[j], wt[j], bi[j]) + best;
            bits |= (uint32_t)code << (2 * j);
        }
        if (s0 < S) bp[(size_t)t * wpr + (s0 >> 4)] = bits;
    }
};

template <bool SKIPS>
__global__ __launch_bounds__(BS_NT) void ear_dp_kernel(const EaSeq* __restrict__ seqs, const uint8_t* __restrict__ codes, const int32_t* __restrict__ lvl_t,
                                                       const uint32_t* __restrict__ w_t, const int32_t* __restrict__ bias_t, EaState bg, int k, int pen,
                                                       uint8_t* __restrict__ ws, int32_t* __restrict__ fin)
{
    const EaSeq q = seqs[blockIdx.x];
    const int S = q.L + 2;
    const int32_t* rows = (const int32_t*)(ws + q.zq);
    EarSweep<SKIPS> p{{codes + q.codes, lvl_t, w_t, bias_t, bg, fin + 2 * (int64_t)blockIdx.x, k, q.L, S},
                      rows, rows + q.T, (uint32_t*)(ws + q.bp), (S + 15) / 16, pen};
    band_sweep(p, S, q.T, (Cell2*)(ws + q.col));
}

// One wave per read: end state, score, then the walk.  With 1.7 rows per base nearly every row is a transition, so ea_tb_kernel's ballot
// (which jumps over the rows a state dwells in) has little to jump over; here the wave stages 64 rows of the words the path can be in --
// it moves down at most two states a row, 126 states over the block, 9 words of 16 -- into LDS with independent loads, and the walk reads
// LDS, a row a step, the same in every lane.  first[] of a skipped base holds -2 - (the row at which the path jumped over it) for
// ear_reduce_kernel.
constexpr int EAR_TB_ROWS = 64, EAR_TB_WORDS = 9;
__global__ __launch_bounds__(64) void ear_tb_kernel(const EaSeq* __restrict__ seqs, const uint8_t* __restrict__ ws, const int32_t* __restrict__ fin,
                                                    EaOut* __restrict__ out, int32_t* __restrict__ nskip, int32_t* __restrict__ first,
                                                    int32_t* __restrict__ last)
{
    __shared__ uint32_t blk[EAR_TB_ROWS][EAR_TB_WORDS];
    const int p = blockIdx.x, lane = threadIdx.x;
    const EaSeq q = seqs[p];
    const int L = q.L;
    const int32_t v_trail = fin[2 * (int64_t)p], v_last = fin[2 * (int64_t)p + 1];
    // s, e and the walk below are the same in every lane; read through the first lane they are the compiler's scalars, and the walk branches
    // on scalar compares instead of masking lanes
    int s = __builtin_amdgcn_readfirstlane(ea_ends_in_trail(v_trail, v_last) ? L + 1 : L);
    const uint32_t* __restrict__ bp = (const uint32_t*)(ws + q.bp);
    const int64_t wpr = (L + 2 + 15) / 16;
    int32_t* fs = first + q.lab;
    int32_t* ls = last + q.lab;
    int e = q.T - 1, skipped = 0;
    if (lane == 0) {
        out[p].score = s == L + 1 ? v_trail : v_last;
        if (s >= 1 && s <= L) ls[s - 1] = e;
    }
    while (e > 0 && s > 0) {
        const int n = e < EAR_TB_ROWS ? e : EAR_TB_ROWS;   // rows e .. e - n + 1
        const int w_hi = s >> 4, w_lo = w_hi >= EAR_TB_WORDS - 1 ? w_hi - (EAR_TB_WORDS - 1) : 0;
        // a lane's nine words of the block: every load is issued before the first is stored (a loop that loads and stores a word a turn
        // waits for each load in turn: nine latencies a block instead of one)
        uint32_t word[EAR_TB_WORDS];
#pragma unroll
        for (int j = 0; j < EAR_TB_WORDS; j++) {
            const int i = lane + 64 * j, r = i / EAR_TB_WORDS, w = w_lo + i % EAR_TB_WORDS;
            word[j] = r < n && w <= w_hi ? bp[(int64_t)(e - r) * wpr + w] : 0u;
        }
#pragma unroll
        for (int j = 0; j < EAR_TB_WORDS; j++) (&blk[0][0])[lane + 64 * j] = word[j];
        __syncthreads();
        int r = 0;
        for (; r < n && s > 0; r++) {
            int code = __builtin_amdgcn_readfirstlane((int)((blk[r][(s >> 4) - w_lo] >> (2 * (s & 15))) & 3u));
            if (code == EAR_STAY) continue;
            if (code > s) code = s;   // (no reachable cell has such a code: the state never leaves the read)
            const int row = e - r;
            if (lane == 0) {
                if (s <= L) fs[s - 1] = row;
                if (code == EAR_SKIP) fs[s - 2] = -2 - row;
                if (s - code >= 1) ls[s - code - 1] = row - 1;
            }
            skipped += code == EAR_SKIP;
            s -= code;
        }
        e -= r;
        __syncthreads();
    }
    if (lane == 0) {
        if (s == 1 && L >= 1) fs[0] = 0;
        nskip[p] = skipped;
    }
}

// grid (ceil(max L / 256), reads), one lane per base: the records of the base's rows (1.7 on average) summed.  A base the path stalls in for
// thousands of rows is one lane reading 28 bytes a row while its wave waits; at 2^19 rows that is tens of milliseconds, and a detector
// that cuts an event per 17 samples leaves no such base in practice.
__global__ __launch_bounds__(256) void ear_reduce_kernel(const EaSeq* __restrict__ seqs, const int32_t* __restrict__ in_start, const int64_t* __restrict__ in_sum,
                                                         const int64_t* __restrict__ in_sumsq, const int16_t* __restrict__ in_min,
                                                         const int16_t* __restrict__ in_max, int32_t* __restrict__ first, int32_t* __restrict__ last,
                                                         int32_t* __restrict__ start, int32_t* __restrict__ end, int64_t* __restrict__ sum,
                                                         int64_t* __restrict__ sumsq, int16_t* __restrict__ mn, int16_t* __restrict__ mx)
{
    const EaSeq q = seqs[blockIdx.y];
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= q.L) return;
    const int64_t o = q.lab + b;
    int32_t f = first[o], l = last[o];
    if (f <= -2) {
        start[o] = end[o] = in_start[q.raw0 + min(-2 - f, q.T - 1)] + q.t_lo;
        first[o] = last[o] = -1;
        sum[o] = sumsq[o] = 0;
        mn[o] = mx[o] = 0;
        return;
    }
    f = min(max(f, 0), q.T - 1);   // (a walked path leaves 0 <= f <= l < T; no index leaves the read's events whatever the words held)
    l = min(max(l, f), q.T - 1);
    int64_t a = 0, a2 = 0;
    int lo = 32767, hi = -32768;
    for (int e = f; e <= l; e++) {
        a += in_sum[q.raw0 + e];
        a2 += in_sumsq[q.raw0 + e];
        lo = min(lo, (int)in_min[q.raw0 + e]);
        hi = max(hi, (int)in_max[q.raw0 + e]);
    }
    start[o] = in_start[q.raw0 + f] + q.t_lo;
    end[o] = (l + 1 < q.T ? in_start[q.raw0 + l + 1] : q.n_win) + q.t_lo;
    sum[o] = a;
    sumsq[o] = a2;
    mn[o] = (int16_t)lo;
    mx[o] = (int16_t)hi;
}

// ---- what the two launch loops call
// a read's three blocks of the launch's workspace (ws is dry: the descriptor holds offsets into ws_align)
void ea_place(Carve& ws, EaSeq& d, size_t zq_bytes, size_t bp_bytes, size_t col_bytes)
{
    d.zq = (int64_t)ws.mark();
    ws.take<char>(zq_bytes, 0, 1);
    d.bp = (int64_t)ws.mark();
    ws.take<char>(bp_bytes, 0, 1);
    d.col = (int64_t)ws.mark();
    ws.take<char>(col_bytes, 0, 1);
}

// the host's copy of a launch's io block
struct EaFetched {
    std::vector<EaOut> out;
    std::vector<int32_t> i32, skip;
    std::vector<int64_t> i64;
    std::vector<int16_t> i16;
    size_t s4, s8, s2;   // the arrays' strides, in elements
};
// the device-to-host copies of the block (the skip counts where it holds them), and the wait for them
int ea_fetch(hipStream_t st, const EaIo& io, int nb, int64_t nlab, bool skips, EaFetched& h)
{
    h.s4 = io.last - io.first, h.s8 = io.sumsq - io.sum, h.s2 = io.mx - io.mn;
    h.out.resize(nb);
    h.skip.resize(nb);
    h.i32.resize(4 * h.s4);
    h.i64.resize(2 * h.s8);
    h.i16.resize(2 * h.s2);
    RD_HIP(hipMemcpyAsync(h.out.data(), io.out, (size_t)nb * sizeof(EaOut), hipMemcpyDeviceToHost, st));
    if (skips) RD_HIP(hipMemcpyAsync(h.skip.data(), io.nskip, (size_t)nb * 4, hipMemcpyDeviceToHost, st));
    if (nlab) {
        RD_HIP(hipMemcpyAsync(h.i32.data(), io.first, 4 * h.s4 * 4, hipMemcpyDeviceToHost, st));
        RD_HIP(hipMemcpyAsync(h.i64.data(), io.sum, 2 * h.s8 * 8, hipMemcpyDeviceToHost, st));
        RD_HIP(hipMemcpyAsync(h.i16.data(), io.mn, 2 * h.s2 * 2, hipMemcpyDeviceToHost, st));
    }
    RD_HIP(hipStreamSynchronize(st));
    return RD_OK;
}
// member i of the launch, read r of the call with descriptor d, into the caller's arrays
void ea_scatter(const EaBases& b, int r, const EaSeq& d, int i, const EaFetched& h)
{
    const size_t L = (size_t)d.L, o = (size_t)b.ref_off[r], s = (size_t)d.lab;
    b.status[r] = EA_OK;
    b.score[r] = h.out[i].score;
    memcpy(b.fit_sums + 5 * (int64_t)r, h.out[i].sums, 40);
    if (!L) return;
    memcpy(b.first + o, h.i32.data() + s, L * 4);
    memcpy(b.last + o, h.i32.data() + h.s4 + s, L * 4);
    memcpy(b.ev_start + o, h.i32.data() + 2 * h.s4 + s, L * 4);
    memcpy(b.ev_end + o, h.i32.data() + 3 * h.s4 + s, L * 4);
    memcpy(b.ev_sum + o, h.i64.data() + s, L * 8);
    memcpy(b.ev_sumsq + o, h.i64.data() + h.s8 + s, L * 8);
    memcpy(b.ev_min + o, h.i16.data() + s, L * 2);
    memcpy(b.ev_max + o, h.i16.data() + h.s2 + s, L * 2);
}

// the report of a call that left reads over the budget: the first of them, its rows ("samples" or "events"), what it needs
int ea_too_large(const char* who, const BudgetPlan& plan, long long rows, const char* noun, int L, size_t bytes, int64_t budget_bytes)
{
    rd_set_error("%s: read %d (%lld %s x %d bases) needs %lld bytes of workspace, over the budget of %lld; %d read(s) not "
                 "aligned (status RD_EVAL_TOO_LARGE), the others were", who, (int)plan.first_too_large, rows, noun, L, (long long)bytes,
                 (long long)budget_bytes, (int)plan.too_large);
    return RD_ERR_NOMEM;
}

}  // namespace

extern "C" int rd_eventalign(rd_ctx* ctx, const int16_t* raw, const int64_t* read_off, int n_reads, const int64_t* t_lo, const int64_t* t_hi,
                             const uint8_t* codes, const int64_t* ref_off, const int32_t* ref_len, const int32_t* m2_in, const int32_t* d4_in, int k,
                             const int32_t* lvl, const uint32_t* w, const int32_t* bias, int32_t lvl_bg, uint32_t w_bg, int32_t bias_bg,
                             int64_t budget_bytes, int32_t* status, int64_t* score, int32_t* m2, int32_t* d4, int32_t* first_step,
                             int32_t* last_step, int32_t* ev_start, int32_t* ev_end, int64_t* ev_sum, int64_t* ev_sumsq, int16_t* ev_min,
                             int16_t* ev_max, int64_t* fit_sums)
{
    RD_REQUIRE(ctx, "rd_eventalign: null context");
    RD_REQUIRE(budget_bytes >= 0, "rd_eventalign: negative budget");
    const EaCall c{raw, read_off, t_lo, t_hi, n_reads,
                   EaBases{codes, ref_off, ref_len, m2_in, d4_in, EaModel{k, lvl, w, bias, EaState{lvl_bg, w_bg, bias_bg}}, status, score, first_step,
                           last_step, ev_start, ev_end, ev_sum, ev_sumsq, ev_min, ev_max, fit_sums},
                   m2, d4};
    int64_t n_bases = 0;
    int rc = ea_check_args("rd_eventalign", c, &n_bases);
    if (rc || n_reads == 0) return rc;
    RD_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // the samples the reads span, rebased to the first read's; the bases; the model
    const int64_t lo = read_off[0], n_samples = read_off[n_reads] - lo;
    if (ctx->ws_raw.reserve((size_t)n_samples * 2 + 16) || ctx->ws_labels.reserve((size_t)n_bases + 16)) return RD_ERR_NOMEM;
    const int16_t* d_raw = ctx->ws_raw.as<int16_t>();
    const uint8_t* d_codes = ctx->ws_labels.as<uint8_t>();
    if (n_samples) RD_HIP(hipMemcpyAsync(ctx->ws_raw.p, raw + lo, (size_t)n_samples * 2, hipMemcpyHostToDevice, st));
    if (n_bases) RD_HIP(hipMemcpyAsync(ctx->ws_labels.p, codes, (size_t)n_bases, hipMemcpyHostToDevice, st));
    KmerTables tab;
    if ((rc = signal_upload_tables(ctx, st, k, lvl, w, bias, 0, &tab))) return rc;
    const int32_t *d_lvl = tab.lvl, *d_bias = tab.bias;
    const uint32_t* d_w = tab.w;
    std::vector<int64_t> off(n_reads + 1);
    for (int r = 0; r <= n_reads; r++) off[r] = read_off[r] - lo;
    // every read's scale: a property of the read alone, whatever the budget does with it afterwards
    std::vector<SignalScaleIn> scin(n_reads);
    std::vector<int32_t> scale;
    for (int r = 0; r < n_reads; r++) scin[r] = signal_scale_in(off[r] + t_lo[r], t_hi[r] - t_lo[r], t_hi[r] - t_lo[r], EA_MAX_T, m2_in[r], d4_in[r]);
    if ((rc = signal_scales(ctx, st, d_raw, scin, EA_MAX_T, scale))) return rc;
    // statuses that need no alignment, then the launches: the other reads in the caller's order, as many as fit the budget; a read that
    // alone exceeds it is reported, not launched
    for (int r = 0; r < n_reads; r++) {
        const int stat = ea_status(t_hi[r] - t_lo[r], ref_len[r], scale[2 * (size_t)r + 1]);   // (EMPTY and TOO_LONG come before the scale is looked at)
        ea_blank(c, r, stat == EA_OK ? EA_TOO_LARGE : stat, scale[2 * (size_t)r], scale[2 * (size_t)r + 1]);   // OK: until its launch has run
    }
    if ((rc = rd_resolve_budget(&budget_bytes, ctx->ws_align.cap))) return rc;
    const BudgetPlan plan = rd_plan_budget(n_reads, nullptr, budget_bytes, 0, false,
                                           [&](int r, int) { return status[r] == EA_TOO_LARGE ? (int64_t)ea_read_bytes(t_hi[r] - t_lo[r], ref_len[r]) : (int64_t)-1; },
                                           [](int, int, int64_t count, int64_t) { return count >= EA_MAX_LAUNCH; });
    if (plan.max_bytes && ctx->ws_align.reserve_exact((size_t)plan.max_bytes, "rd_eventalign")) return RD_ERR_NOMEM;
    std::vector<EaSeq> desc;
    EaFetched h;
    std::vector<int32_t> ev_len, ev_status;
    std::vector<int64_t> ev_lab;
    for (auto [k0, k1] : plan.launches) {
        const int nb = (int)(k1 - k0);
        const int32_t* members = plan.run.data() + k0;
        const int r_lo = members[0], r_hi = members[nb - 1] + 1;   // the launch's reads lie in [r_lo, r_hi) of the call's
        desc.resize(nb);
        ev_len.assign(r_hi - r_lo, 0);
        ev_lab.assign(r_hi - r_lo, 0);
        ev_status.assign(r_hi - r_lo, 0);
        Carve ws;   // (dry: the descriptors hold offsets into ws_align)
        int64_t nlab = 0, max_T = 0;
        for (int i = 0; i < nb; i++) {
            const int r = members[i];
            EaSeq& d = desc[i];
            d.raw0 = off[r] + t_lo[r];
            d.codes = ref_off[r];
            d.lab = nlab;
            d.T = (int32_t)(t_hi[r] - t_lo[r]);
            d.L = ref_len[r];
            d.m2 = m2[r];
            d.d4 = d4[r];
            d.t_lo = (int32_t)t_lo[r];
            d.n_win = 0;
            ea_place(ws, d, ea_zq_bytes(d.T), ea_bp_bytes(d.T, d.L), ea_col_bytes(d.T, d.L));
            ev_len[r - r_lo] = d.L;   // (a read between two members that is not one has no labels in this launch)
            ev_lab[r - r_lo] = d.lab;
            nlab += d.L;
            max_T = std::max<int64_t>(max_T, d.T);
        }
        if ((rc = rd_carve_check("rd_eventalign", ws, ctx->ws_align.cap))) return rc;
        EaIo io;
        if (rd_carve(ctx->ws_eval, [&](Carve& cv) { ea_io_layout(cv, nb, nlab, 0, &io); })) return RD_ERR_NOMEM;
        uint8_t* dws = ctx->ws_align.as<uint8_t>();
        RD_HIP(hipMemcpyAsync(io.seqs, desc.data(), (size_t)nb * sizeof(EaSeq), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(ea_quant_kernel, dim3((unsigned)((max_T + 255) / 256), nb), dim3(256), 0, st, io.seqs, d_raw, dws, io.fin);
        RD_HIP(hipGetLastError());
        hipLaunchKernelGGL(ea_dp_kernel, dim3(nb), dim3(BS_NT), 0, st, io.seqs, d_codes, d_lvl, d_w, d_bias, c.b.m.bg, k, dws, io.fin);
        RD_HIP(hipGetLastError());
        hipLaunchKernelGGL(ea_tb_kernel, dim3(nb), dim3(64), 0, st, io.seqs, dws, io.fin, io.out, io.first, io.last);
        RD_HIP(hipGetLastError());
        if ((rc = rd_event_stats_dev(ctx, st, d_raw, off.data() + r_lo, r_hi - r_lo, io.first, io.last, ev_lab.data(), ev_len.data(), ev_status.data(),
                                     io.start, io.end, io.sum, io.sumsq, io.mn, io.mx)))
            return rc;
        hipLaunchKernelGGL(ea_sums_kernel, dim3(nb), dim3(256), 0, st, io.seqs, d_codes, d_lvl, k, io.start, io.end, io.sum, io.out);
        RD_HIP(hipGetLastError());
        if ((rc = ea_fetch(st, io, nb, nlab, false, h))) return rc;
        for (int i = 0; i < nb; i++) ea_scatter(c.b, members[i], desc[i], i, h);
    }
    if (plan.too_large) {
        const int r = (int)plan.first_too_large;
        const int64_t T = t_hi[r] - t_lo[r];
        return ea_too_large("rd_eventalign", plan, (long long)T, "samples", ref_len[r], ea_read_bytes(T, ref_len[r]), budget_bytes);
    }
    return RD_OK;
}

extern "C" int rd_eventalign_events(rd_ctx* ctx, int n_reads, const int64_t* n_samples, const int64_t* sample_off, const int64_t* ev_off,
                                    const int32_t* n_events, const int32_t* in_start, const int64_t* in_sum, const int64_t* in_sumsq,
                                    const int16_t* in_min, const int16_t* in_max, const uint8_t* codes, const int64_t* ref_off, const int32_t* ref_len,
                                    const int32_t* m2_in, const int32_t* d4_in, int k, const int32_t* lvl, const uint32_t* w, const int32_t* bias,
                                    int32_t lvl_bg, uint32_t w_bg, int32_t bias_bg, int skip_pen, int64_t budget_bytes, int32_t* status, int64_t* score,
                                    int32_t* n_skipped, int32_t* row_first, int32_t* row_last, int32_t* ev_start, int32_t* ev_end, int64_t* ev_sum,
                                    int64_t* ev_sumsq, int16_t* ev_min, int16_t* ev_max, int64_t* fit_sums)
{
    RD_REQUIRE(ctx, "rd_eventalign_events: null context");
    RD_REQUIRE(budget_bytes >= 0, "rd_eventalign_events: negative budget");
    const EarCall c{n_reads, n_samples, sample_off, ev_off, n_events, in_start, in_sum, in_sumsq, in_min, in_max, skip_pen,
                    EaBases{codes, ref_off, ref_len, m2_in, d4_in, EaModel{k, lvl, w, bias, EaState{lvl_bg, w_bg, bias_bg}}, status, score, row_first,
                            row_last, ev_start, ev_end, ev_sum, ev_sumsq, ev_min, ev_max, fit_sums},
                    n_skipped};
    int64_t n_bases = 0;
    int rc = ear_check_args("rd_eventalign_events", c, &n_bases);
    if (rc || n_reads == 0) return rc;
    RD_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (ctx->ws_labels.reserve((size_t)n_bases + 16)) return RD_ERR_NOMEM;
    const uint8_t* d_codes = ctx->ws_labels.as<uint8_t>();
    if (n_bases) RD_HIP(hipMemcpyAsync(ctx->ws_labels.p, codes, (size_t)n_bases, hipMemcpyHostToDevice, st));
    KmerTables tab;
    if ((rc = signal_upload_tables(ctx, st, k, lvl, w, bias, 0, &tab))) return rc;
    // statuses that need no alignment, then the launches: the other reads in the caller's order, as many as fit the budget; a read that
    // alone exceeds it is reported, not launched
    for (int r = 0; r < n_reads; r++) {
        const int stat = ear_status(n_samples[r], n_events[r], ref_len[r], d4_in[r], skip_pen);
        ear_blank(c, r, stat == EA_OK ? EA_TOO_LARGE : stat);   // OK: until its launch has run
    }
    if ((rc = rd_resolve_budget(&budget_bytes, ctx->ws_align.cap))) return rc;
    const BudgetPlan plan = rd_plan_budget(n_reads, nullptr, budget_bytes, 0, false,
                                           [&](int r, int) { return status[r] == EA_TOO_LARGE ? (int64_t)ear_read_bytes(n_events[r], ref_len[r]) : (int64_t)-1; },
                                           [](int, int, int64_t count, int64_t) { return count >= EA_MAX_LAUNCH; });
    if (plan.max_bytes && ctx->ws_align.reserve_exact((size_t)plan.max_bytes, "rd_eventalign_events")) return RD_ERR_NOMEM;
    std::vector<EaSeq> desc;
    EaFetched h;
    std::vector<int32_t> p_start;
    std::vector<int64_t> p_sum, p_sumsq;
    std::vector<int16_t> p_min, p_max;
    for (auto [k0, k1] : plan.launches) {
        const int nb = (int)(k1 - k0);
        const int32_t* members = plan.run.data() + k0;
        desc.resize(nb);
        p_start.clear();
        p_sum.clear();
        p_sumsq.clear();
        p_min.clear();
        p_max.clear();
        Carve ws;   // (dry: the descriptors hold offsets into ws_align)
        int64_t nlab = 0, max_E = 0, max_L = 0;
        for (int i = 0; i < nb; i++) {
            const int r = members[i];
            const int64_t E = n_events[r], eo = ev_off[r];
            EaSeq& d = desc[i];
            d.raw0 = (int64_t)p_start.size();   // the launch's events, the members' back to back
            p_start.insert(p_start.end(), in_start + eo, in_start + eo + E);
            p_sum.insert(p_sum.end(), in_sum + eo, in_sum + eo + E);
            p_sumsq.insert(p_sumsq.end(), in_sumsq + eo, in_sumsq + eo + E);
            p_min.insert(p_min.end(), in_min + eo, in_min + eo + E);
            p_max.insert(p_max.end(), in_max + eo, in_max + eo + E);
            d.codes = ref_off[r];
            d.lab = nlab;
            d.T = (int32_t)E;
            d.L = ref_len[r];
            d.m2 = m2_in[r];
            d.d4 = d4_in[r];
            d.t_lo = (int32_t)sample_off[r];
            d.n_win = (int32_t)n_samples[r];
            ea_place(ws, d, ear_row_bytes(E), ear_bp_bytes(E, d.L), ear_col_bytes(E, d.L));
            nlab += d.L;
            max_E = std::max<int64_t>(max_E, E);
            max_L = std::max<int64_t>(max_L, d.L);
        }
        if ((rc = rd_carve_check("rd_eventalign_events", ws, ctx->ws_align.cap))) return rc;
        const int64_t n_ev = (int64_t)p_start.size();
        EarEvents ev;
        EaIo io;
        if (rd_carve(ctx->ws_raw, [&](Carve& cv) { ear_events_layout(cv, n_ev, &ev); })) return RD_ERR_NOMEM;
        if (rd_carve(ctx->ws_eval, [&](Carve& cv) { ea_io_layout(cv, nb, nlab, nb, &io); })) return RD_ERR_NOMEM;
        uint8_t* dws = ctx->ws_align.as<uint8_t>();
        RD_HIP(hipMemcpyAsync(io.seqs, desc.data(), (size_t)nb * sizeof(EaSeq), hipMemcpyHostToDevice, st));
        RD_HIP(hipMemcpyAsync(ev.start, p_start.data(), (size_t)n_ev * 4, hipMemcpyHostToDevice, st));
        RD_HIP(hipMemcpyAsync(ev.sum, p_sum.data(), (size_t)n_ev * 8, hipMemcpyHostToDevice, st));
        RD_HIP(hipMemcpyAsync(ev.sumsq, p_sumsq.data(), (size_t)n_ev * 8, hipMemcpyHostToDevice, st));
        RD_HIP(hipMemcpyAsync(ev.mn, p_min.data(), (size_t)n_ev * 2, hipMemcpyHostToDevice, st));
        RD_HIP(hipMemcpyAsync(ev.mx, p_max.data(), (size_t)n_ev * 2, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(ear_row_kernel, dim3((unsigned)((max_E + 255) / 256), nb), dim3(256), 0, st, io.seqs, ev.start, ev.sum, dws, io.fin);
        RD_HIP(hipGetLastError());
        if (skip_pen >= 0)
            hipLaunchKernelGGL(ear_dp_kernel<true>, dim3(nb), dim3(BS_NT), 0, st, io.seqs, d_codes, tab.lvl, tab.w, tab.bias, c.b.m.bg, k, skip_pen, dws, io.fin);
        else
            hipLaunchKernelGGL(ear_dp_kernel<false>, dim3(nb), dim3(BS_NT), 0, st, io.seqs, d_codes, tab.lvl, tab.w, tab.bias, c.b.m.bg, k, 0, dws, io.fin);
        RD_HIP(hipGetLastError());
        hipLaunchKernelGGL(ear_tb_kernel, dim3(nb), dim3(64), 0, st, io.seqs, dws, io.fin, io.out, io.nskip, io.first, io.last);
        RD_HIP(hipGetLastError());
        if (max_L) {
            hipLaunchKernelGGL(ear_reduce_kernel, dim3((unsigned)((max_L + 255) / 256), nb), dim3(256), 0, st, io.seqs, ev.start, ev.sum, ev.sumsq, ev.mn,
                               ev.mx, io.first, io.last, io.start, io.end, io.sum, io.sumsq, io.mn, io.mx);
            RD_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL(ea_sums_kernel, dim3(nb), dim3(256), 0, st, io.seqs, d_codes, tab.lvl, k, io.start, io.end, io.sum, io.out);
        RD_HIP(hipGetLastError());
        if ((rc = ea_fetch(st, io, nb, nlab, true, h))) return rc;
        for (int i = 0; i < nb; i++) {
            ea_scatter(c.b, members[i], desc[i], i, h);
            n_skipped[members[i]] = h.skip[i];
        }
    }
    if (plan.too_large) {
        const int r = (int)plan.first_too_large;
        return ea_too_large("rd_eventalign_events", plan, n_events[r], "events", ref_len[r], ear_read_bytes(n_events[r], ref_len[r]), budget_bytes);
    }
    return RD_OK;
}

// ---- sample rows in a band (rd_eventalign_banded).  An EaSeq of these kernels: zq the quantised samples, bp one
// 64-bit word a row, col the window's lowest state per row (int32) followed, at the next multiple of 256 bytes, by the state table: lvl,
// w and bias of n = L + 2 + 128 states, three arrays of n, zeros past the read (a state that costs nothing and is never read out).
namespace {

constexpr int EAB_WAVES = 4;   // reads of a DP workgroup, one wave each, no barrier

__device__ __forceinline__ const int32_t* eab_tab(const uint8_t* ws, const EaSeq& q) { return (const int32_t*)(ws + q.col + (((int64_t)q.T * 4 + 255) & ~(int64_t)255)); }

// grid (ceil(max(T, L + 130) / 256), reads): zq and the window's lowest state of every row, the constants of every state
__global__ __launch_bounds__(256) void eab_rows_kernel(const EaSeq* __restrict__ seqs, const int16_t* __restrict__ raw, const uint8_t* __restrict__ codes,
                                                       const int32_t* __restrict__ guide, const int32_t* __restrict__ lvl_t, const uint32_t* __restrict__ w_t,
                                                       const int32_t* __restrict__ bias_t, EaState bg, int k, uint8_t* __restrict__ ws,
                                                       int32_t* __restrict__ fin)
{
    const EaSeq q = seqs[blockIdx.y];
    if (blockIdx.x == 0 && threadIdx.x < 2) fin[2 * (int64_t)blockIdx.y + threadIdx.x] = EA_INF;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < q.T) {
        ((int32_t*)(ws + q.zq))[t] = ea_quant(raw[q.raw0 + t], q.m2, q.d4);
        ((int32_t*)(ws + q.col))[t] = eab_lo(eab_count(guide + q.lab, q.L, (int64_t)q.t_lo + t), q.L);
    }
    if (t < (int64_t)q.L + 2 + 2 * EAB_W) {
        EaState st{0, 0, 0};
        if (t < q.L + 2) st = ea_state((int32_t)t, q.L, codes + q.codes, k, lvl_t, w_t, bias_t, bg);
        int32_t* tab = (int32_t*)eab_tab(ws, q);
        const int64_t n = (int64_t)q.L + 2 + 2 * EAB_W;
        tab[t] = st.lvl;
        tab[n + t] = (int32_t)st.w;
        tab[2 * n + t] = st.bias;
    }
}

// lane l receives v of lane l - 1, lane 0 that of lane 63 (DPP wave_ror:1)
__device__ __forceinline__ int32_t lane_ror1(int32_t v) { return __builtin_amdgcn_update_dpp(v, v, 0x13C, 0xf, 0xf, false); }

// One wave per read.  Lane l holds the window's state s with s & 63 == l: its value and its constants, and, prefetched, the constants of
// s + 64, which the lane takes when the window's lowest state passes s (the load of the state after that is issued then and is not waited
// for until the lane recycles again, some thirty rows a state later).  zq and the window's lowest state of 64 rows sit in two registers
// across the wave, loaded a tile ahead, and reach the row as scalars by v_readlane; the row's back-pointer word is the ballot of "advance
// taken", kept by lane t & 63 and stored 512 consecutive bytes every 64 rows.
__global__ __launch_bounds__(64 * EAB_WAVES) void eab_dp_kernel(const EaSeq* __restrict__ seqs, int n_reads, uint8_t* __restrict__ ws, int32_t* __restrict__ fin)
{
    const int p = __builtin_amdgcn_readfirstlane(blockIdx.x * EAB_WAVES + ((int)threadIdx.x >> 6)), lane = threadIdx.x & 63;   // (the wave's: a scalar)
    if (p >= n_reads) return;
    const EaSeq q = seqs[p];
    const int T = q.T, L = q.L;
    const int32_t* __restrict__ zq = (const int32_t*)(ws + q.zq);
    const int32_t* __restrict__ lo_t = (const int32_t*)(ws + q.col);
    const int n_tab = L + 2 + 2 * EAB_W;
    const int32_t* __restrict__ t_lvl = eab_tab(ws, q);
    const int32_t* __restrict__ t_w = t_lvl + n_tab;
    const int32_t* __restrict__ t_bias = t_w + n_tab;
    unsigned long long* __restrict__ bp = (unsigned long long*)(ws + q.bp);
    int32_t tz = lane < T ? zq[lane] : 0, tl = lane < T ? lo_t[lane] : 0;
    int lo = __builtin_amdgcn_readfirstlane(tl);
    int s = lo + ((lane - lo) & (EAB_W - 1));
    int32_t lv = t_lvl[s], bi = t_bias[s], nlv = t_lvl[s + EAB_W], nbi = t_bias[s + EAB_W];   // the state's constants and, prefetched, those of the state 64 above
    uint32_t wt = (uint32_t)t_w[s], nwt = (uint32_t)t_w[s + EAB_W];
    // row 0: states 0 and 1 start the path, every other state of the window is unreachable.  (Lane 0's sample by its number, read before
    // the lanes part: the first ACTIVE lane of the branch is lane 1 when the window starts at state 1)
    const int z0 = __builtin_amdgcn_readlane(tz, 0);
    int32_t v = s <= 1 ? ea_cost(z0, lv, wt, bi) : EA_INF;
    unsigned long long mine = 0;
    // every load so far has landed before the first row: a row then waits for no load (the compiler would otherwise let the row wait until
    // few enough loads are in flight for these to be among the landed, and with them for a recycle's prefetch)
    __builtin_amdgcn_s_waitcnt(0);
    for (int tbase = 0; tbase < T; tbase += 64) {
        int32_t nz = 0, nl = 0;   // the next tile's rows
        if (tbase + 64 + lane < T) {
            nz = zq[tbase + 64 + lane];
            nl = lo_t[tbase + 64 + lane];
        }
        const int rows = T - tbase < 64 ? T - tbase : 64;
        for (int r = __builtin_amdgcn_readfirstlane(tbase == 0 ? 1 : 0); r < rows; r++) {   // (row 0 is done)
            const int z = __builtin_amdgcn_readlane(tz, r), l = __builtin_amdgcn_readlane(tl, r);
            if (l != lo) {   // (wave-uniform; about once in thirty rows)
                lo = l;
                // A lane whose state fell out takes its state + 64 and the constants it had prefetched.  Every lane loads its next constants
                // (those it holds already, or the new ones), so the load lands in the registers themselves and nothing here waits for it.
                // After a jump of more than 64 states in one row the same again, now waiting for each load in turn
                do {
                    const bool out = s < lo;
                    s = out ? s + EAB_W : s;
                    lv = out ? nlv : lv;
                    wt = out ? nwt : wt;
                    bi = out ? nbi : bi;
                    v = out ? EA_INF : v;
                    nlv = t_lvl[s + EAB_W];
                    nwt = (uint32_t)t_w[s + EAB_W];
                    nbi = t_bias[s + EAB_W];
                } while (__ballot(s < lo));
            }
            const int32_t left = lane_ror1(v), adv = s == lo ? EA_INF : left;
            const bool take = ea_advance(v, adv);
            v = ea_cost(z, lv, wt, bi) + (take ? adv : v);
            const unsigned long long word = __ballot(take);
            if (lane == r) mine = word;
        }
        if (tbase + lane < T) bp[tbase + lane] = mine;
        tz = nz;
        tl = nl;
    }
    // the two states the path may end in, where the last window holds them
    if (s == L + 1) fin[2 * (int64_t)p] = v;
    if (s == L) fin[2 * (int64_t)p + 1] = v;
}

// one wave per read: ea_tb_kernel's ballot walk on one 64-bit word a row.  A read whose end value is not finite is flagged, its steps blank
__global__ __launch_bounds__(64) void eab_tb_kernel(const EaSeq* __restrict__ seqs, const uint8_t* __restrict__ ws, const int32_t* __restrict__ fin,
                                                    EaOut* __restrict__ out, int32_t* __restrict__ lost, int32_t* __restrict__ first,
                                                    int32_t* __restrict__ last)
{
    const int p = blockIdx.x, lane = threadIdx.x;
    const EaSeq q = seqs[p];
    const int L = q.L, off = q.t_lo;
    const int32_t v_trail = fin[2 * (int64_t)p], v_last = fin[2 * (int64_t)p + 1];
    int s = ea_ends_in_trail(v_trail, v_last) ? L + 1 : L;   // (s, t and r0 below are the same in every lane)
    const int32_t end = s == L + 1 ? v_trail : v_last;
    int32_t* fs = first + q.lab;
    int32_t* ls = last + q.lab;
    if (!eab_finite(end)) {
        for (int b = lane; b < L; b += 64) fs[b] = ls[b] = -1;
        if (lane == 0) {
            lost[p] = 1;
            out[p].score = 0;
        }
        return;
    }
    const unsigned long long* __restrict__ bp = (const unsigned long long*)(ws + q.bp);
    int t = q.T - 1;
    if (lane == 0) {
        lost[p] = 0;
        out[p].score = end;
        if (s >= 1 && s <= L) ls[s - 1] = t + off;
    }
    while (t > 0) {
        const int n = t < 64 ? t : 64;
        const unsigned long long a = lane < n ? bp[t - lane] : 0ull;   // lane r holds the word of row t - r
        int r0 = 0;   // rows t .. t - r0 + 1 are walked
        while (r0 < n && s > 0) {
            const unsigned long long m = __ballot(lane >= r0 && lane < n && ((a >> (s & (EAB_W - 1))) & 1ull));
            if (m == 0) {   // the path stays in s for the rest of these rows
                r0 = n;
                break;
            }
            const int r1 = __ffsll((long long)m) - 1, tt = t - r1;   // the nearest row that was entered from s - 1
            if (lane == 0) {
                if (s <= L) fs[s - 1] = tt + off;
                if (s - 1 >= 1) ls[s - 2] = tt - 1 + off;
            }
            s--;
            r0 = r1 + 1;
        }
        if (s == 0) break;   // the lead: nothing is left to record
        t -= r0;
    }
    if (lane == 0 && s == 1 && L >= 1) fs[0] = off;
}

// one wave per read, a lane per base: the bases whose rows touch the window's rim
__global__ __launch_bounds__(64) void eab_edge_kernel(const EaSeq* __restrict__ seqs, const uint8_t* __restrict__ ws, const int32_t* __restrict__ lost,
                                                      const int32_t* __restrict__ first, const int32_t* __restrict__ last, int32_t* __restrict__ n_edge)
{
    const int p = blockIdx.x, lane = threadIdx.x;
    const EaSeq q = seqs[p];
    const int32_t* __restrict__ lo_t = (const int32_t*)(ws + q.col);
    int cnt = 0;
    if (!lost[p])
        for (int b = lane; b < q.L; b += 64) {
            const int f = min(max(first[q.lab + b] - q.t_lo, 0), q.T - 1), l = min(max(last[q.lab + b] - q.t_lo, 0), q.T - 1);   // (a walked path leaves them inside)
            cnt += eab_on_rim(b + 1, lo_t[l], lo_t[f]) ? 1 : 0;
        }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d);
    if (lane == 0) n_edge[p] = cnt;
}

}  // namespace

extern "C" int rd_eventalign_banded(rd_ctx* ctx, const int16_t* raw, const int64_t* read_off, int n_reads, const int64_t* t_lo, const int64_t* t_hi,
                                    const uint8_t* codes, const int64_t* ref_off, const int32_t* ref_len, const int32_t* guide, const int32_t* m2_in,
                                    const int32_t* d4_in, int k, const int32_t* lvl, const uint32_t* w, const int32_t* bias, int32_t lvl_bg, uint32_t w_bg,
                                    int32_t bias_bg, int64_t budget_bytes, int32_t* status, int64_t* score, int32_t* m2, int32_t* d4, int32_t* n_edge,
                                    int32_t* first_step, int32_t* last_step, int32_t* ev_start, int32_t* ev_end, int64_t* ev_sum, int64_t* ev_sumsq,
                                    int16_t* ev_min, int16_t* ev_max, int64_t* fit_sums)
{
    RD_REQUIRE(ctx, "rd_eventalign_banded: null context");
    RD_REQUIRE(budget_bytes >= 0, "rd_eventalign_banded: negative budget");
    const EaCall c{raw, read_off, t_lo, t_hi, n_reads,
                   EaBases{codes, ref_off, ref_len, m2_in, d4_in, EaModel{k, lvl, w, bias, EaState{lvl_bg, w_bg, bias_bg}}, status, score, first_step,
                           last_step, ev_start, ev_end, ev_sum, ev_sumsq, ev_min, ev_max, fit_sums},
                   m2, d4};
    int64_t n_bases = 0;
    int rc = ea_check_args("rd_eventalign_banded", c, &n_bases);
    if (!rc) rc = eab_check_guide("rd_eventalign_banded", c, guide, n_edge, n_bases);
    if (rc || n_reads == 0) return rc;
    RD_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int64_t lo = read_off[0], n_samples = read_off[n_reads] - lo;
    if (ctx->ws_raw.reserve((size_t)n_samples * 2 + 16) || ctx->ws_labels.reserve((size_t)n_bases + 16)) return RD_ERR_NOMEM;
    const int16_t* d_raw = ctx->ws_raw.as<int16_t>();
    const uint8_t* d_codes = ctx->ws_labels.as<uint8_t>();
    if (n_samples) RD_HIP(hipMemcpyAsync(ctx->ws_raw.p, raw + lo, (size_t)n_samples * 2, hipMemcpyHostToDevice, st));
    if (n_bases) RD_HIP(hipMemcpyAsync(ctx->ws_labels.p, codes, (size_t)n_bases, hipMemcpyHostToDevice, st));
    KmerTables tab;
    if ((rc = signal_upload_tables(ctx, st, k, lvl, w, bias, 0, &tab))) return rc;
    std::vector<int64_t> off(n_reads + 1);
    for (int r = 0; r <= n_reads; r++) off[r] = read_off[r] - lo;
    std::vector<SignalScaleIn> scin(n_reads);
    std::vector<int32_t> scale;
    for (int r = 0; r < n_reads; r++) scin[r] = signal_scale_in(off[r] + t_lo[r], t_hi[r] - t_lo[r], t_hi[r] - t_lo[r], EA_MAX_T, m2_in[r], d4_in[r]);
    if ((rc = signal_scales(ctx, st, d_raw, scin, EA_MAX_T, scale))) return rc;
    for (int r = 0; r < n_reads; r++) {
        const int stat = ea_status(t_hi[r] - t_lo[r], ref_len[r], scale[2 * (size_t)r + 1]);
        ea_blank(c, r, stat == EA_OK ? EA_TOO_LARGE : stat, scale[2 * (size_t)r], scale[2 * (size_t)r + 1]);   // OK: until its launch has run
        n_edge[r] = 0;
    }
    if ((rc = rd_resolve_budget(&budget_bytes, ctx->ws_align.cap))) return rc;
    const BudgetPlan plan = rd_plan_budget(n_reads, nullptr, budget_bytes, 0, false,
                                           [&](int r, int) { return status[r] == EA_TOO_LARGE ? (int64_t)eab_read_bytes(t_hi[r] - t_lo[r], ref_len[r]) : (int64_t)-1; },
                                           [](int, int, int64_t count, int64_t) { return count >= EA_MAX_LAUNCH; });
    if (plan.max_bytes && ctx->ws_align.reserve_exact((size_t)plan.max_bytes, "rd_eventalign_banded")) return RD_ERR_NOMEM;
    std::vector<EaSeq> desc;
    EaFetched h;
    std::vector<int32_t> ev_len, ev_status, p_guide, rim;
    std::vector<int64_t> ev_lab;
    for (auto [k0, k1] : plan.launches) {
        const int nb = (int)(k1 - k0);
        const int32_t* members = plan.run.data() + k0;
        const int r_lo = members[0], r_hi = members[nb - 1] + 1;   // the launch's reads lie in [r_lo, r_hi) of the call's
        desc.resize(nb);
        ev_len.assign(r_hi - r_lo, 0);
        ev_lab.assign(r_hi - r_lo, 0);
        ev_status.assign(r_hi - r_lo, 0);
        p_guide.clear();
        Carve ws;   // (dry: the descriptors hold offsets into ws_align)
        int64_t nlab = 0, max_n = 0;
        for (int i = 0; i < nb; i++) {
            const int r = members[i];
            EaSeq& d = desc[i];
            d.raw0 = off[r] + t_lo[r];
            d.codes = ref_off[r];
            d.lab = nlab;
            d.T = (int32_t)(t_hi[r] - t_lo[r]);
            d.L = ref_len[r];
            d.m2 = m2[r];
            d.d4 = d4[r];
            d.t_lo = (int32_t)t_lo[r];
            d.n_win = 0;
            ea_place(ws, d, ea_zq_bytes(d.T), eab_bp_bytes(d.T), eab_lo_bytes(d.T) + eab_tab_bytes(d.L));
            p_guide.insert(p_guide.end(), guide + ref_off[r], guide + ref_off[r] + d.L);   // the launch's guides, the members' back to back
            ev_len[r - r_lo] = d.L;
            ev_lab[r - r_lo] = d.lab;
            nlab += d.L;
            max_n = std::max<int64_t>(max_n, std::max<int64_t>(d.T, eab_tab_entries(d.L)));
        }
        if ((rc = rd_carve_check("rd_eventalign_banded", ws, ctx->ws_align.cap))) return rc;
        EaIo io;
        int32_t* d_guide = nullptr;
        // the io block with two int32 per read in the skip counts' place (rim count, lost flag), and the launch's guides behind it
        if (rd_carve(ctx->ws_eval, [&](Carve& cv) {
                ea_io_layout(cv, nb, nlab, 2 * nb, &io);
                d_guide = cv.take<int32_t>((size_t)nlab);
            }))
            return RD_ERR_NOMEM;
        int32_t *d_edge = io.nskip, *d_lost = io.nskip + nb;
        uint8_t* dws = ctx->ws_align.as<uint8_t>();
        RD_HIP(hipMemcpyAsync(io.seqs, desc.data(), (size_t)nb * sizeof(EaSeq), hipMemcpyHostToDevice, st));
        if (nlab) RD_HIP(hipMemcpyAsync(d_guide, p_guide.data(), (size_t)nlab * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(eab_rows_kernel, dim3((unsigned)((max_n + 255) / 256), nb), dim3(256), 0, st, io.seqs, d_raw, d_codes, d_guide, tab.lvl, tab.w,
                           tab.bias, c.b.m.bg, k, dws, io.fin);
        RD_HIP(hipGetLastError());
        hipLaunchKernelGGL(eab_dp_kernel, dim3((unsigned)((nb + EAB_WAVES - 1) / EAB_WAVES)), dim3(64 * EAB_WAVES), 0, st, io.seqs, nb, dws, io.fin);
        RD_HIP(hipGetLastError());
        hipLaunchKernelGGL(eab_tb_kernel, dim3(nb), dim3(64), 0, st, io.seqs, dws, io.fin, io.out, d_lost, io.first, io.last);
        RD_HIP(hipGetLastError());
        hipLaunchKernelGGL(eab_edge_kernel, dim3(nb), dim3(64), 0, st, io.seqs, dws, d_lost, io.first, io.last, d_edge);
        RD_HIP(hipGetLastError());
        if ((rc = rd_event_stats_dev(ctx, st, d_raw, off.data() + r_lo, r_hi - r_lo, io.first, io.last, ev_lab.data(), ev_len.data(), ev_status.data(),
                                     io.start, io.end, io.sum, io.sumsq, io.mn, io.mx)))
            return rc;
        hipLaunchKernelGGL(ea_sums_kernel, dim3(nb), dim3(256), 0, st, io.seqs, d_codes, tab.lvl, k, io.start, io.end, io.sum, io.out);
        RD_HIP(hipGetLastError());
        rim.resize(2 * (size_t)nb);
        RD_HIP(hipMemcpyAsync(rim.data(), io.nskip, 2 * (size_t)nb * 4, hipMemcpyDeviceToHost, st));
        if ((rc = ea_fetch(st, io, nb, nlab, false, h))) return rc;
        for (int i = 0; i < nb; i++) {
            const int r = members[i];
            if (rim[(size_t)nb + i]) {   // the window lost the path: the not-OK outputs, the scale as used
                ea_blank(c, r, EA_OFF_BAND, m2[r], d4[r]);
                continue;
            }
            ea_scatter(c.b, r, desc[i], i, h);
            n_edge[r] = rim[i];
        }
    }
    if (plan.too_large) {
        const int r = (int)plan.first_too_large;
        const int64_t T = t_hi[r] - t_lo[r];
        return ea_too_large("rd_eventalign_banded", plan, (long long)T, "samples", ref_len[r], eab_read_bytes(T, ref_len[r]), budget_bytes);
    }
    return RD_OK;
}
#endif  // __HIPCC__
