// TEST INFRASTRUCTURE: AddressSanitizer + UBSan harness for the host side of radian_amd/csrc/sigmap.hip (the argument checks, the rules of
// sigmap_rules.h, the plain loops of rd_sigmap_host; sanitizers run on the CPU build only -- the kernels are not compiled here).
// usage: asan_sigmap <iterations>   The rules at their limits first.  Every iteration draws a panel (empty and one-state targets among
// them), a model, samples and queries (empty windows, empty ranges, ranges that start inside a target, given and computed scales) into
// EXACT-SIZE heap buffers (a read or a write past either end is an ASan report), calls the host twin and checks every field against a
// whole-table loop of its own written from the contract's text; then the same buffers go through the refusals, which must answer
// RD_ERR_ARG and write nothing.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../radian_amd/csrc/sigmap.hip"   // the host half (this is no HIP build): the device blocks' layout functions live in its unnamed namespace

extern "C" int rd_sigmap_host(const int16_t* raw, int64_t n_raw, int n_q, const int64_t* q_lo, const int64_t* q_hi, const int64_t* sc_lo,
                              const int64_t* sc_hi, const int32_t* m2_in, const int32_t* d4_in, const int64_t* s_lo, const int64_t* s_hi,
                              const uint8_t* codes, const int64_t* tgt_off, int n_tgt, int k, const int32_t* lvl, const uint32_t* w,
                              const int32_t* bias, int n_best, int32_t* status, int32_t* m2, int32_t* d4, int32_t* best_tgt, int32_t* best_score,
                              int32_t* best_end, int32_t* best_org);
extern "C" int64_t rd_sigmap_workspace_bytes(int64_t n_rows, int64_t n_states, int64_t n_tgt_in_range);
void rd_set_error(const char* fmt, ...) { (void)fmt; }

static long g_accepted = 0, g_refused = 0;

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            printf("line %d: %s does not hold\n", __LINE__, #cond);     \
            exit(1);                                                     \
        }                                                                \
    } while (0)

template <typename T> static T* exact(const std::vector<T>& v)
{
    T* p = (T*)malloc(v.size() ? v.size() * sizeof(T) : 1);
    if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

struct Panel {
    std::vector<uint8_t> codes;
    std::vector<int64_t> off;
    int k;
    std::vector<int32_t> lvl, bias;
    std::vector<uint32_t> w;
};

// the contract over one query, the whole table kept: -> the rows of (score, target, end, origin), sorted
static void own_query(const Panel& P, const std::vector<int32_t>& zq, int64_t lo, int64_t hi, std::vector<std::vector<int64_t>>& best)
{
    const int64_t T = (int64_t)zq.size(), n = hi - lo, n_tgt = (int64_t)P.off.size() - 1;
    std::vector<int64_t> tgt(n), cost_lvl(n), cost_w(n), cost_b(n);
    std::vector<char> head(n);
    for (int64_t s = lo; s < hi; s++) {
        int64_t j = 0;
        while (!(P.off[j] <= s && s < P.off[j + 1])) j++;   // the one target that holds s
        CHECK(j < n_tgt);
        const int64_t L = P.off[j + 1] - P.off[j], b = s - P.off[j];
        int64_t idx = 0;
        for (int d = -(P.k / 2); d <= P.k / 2; d++) idx = idx * 4 + P.codes[P.off[j] + std::min(std::max(b + d, (int64_t)0), L - 1)];
        tgt[s - lo] = j;
        cost_lvl[s - lo] = P.lvl[idx], cost_w[s - lo] = P.w[idx], cost_b[s - lo] = P.bias[idx];
        head[s - lo] = b == 0 || s == lo;
    }
    auto c = [&](int64_t t, int64_t i) {
        const int64_t d = zq[t] - cost_lvl[i];
        return std::min((int64_t)(((unsigned __int128)(d * d) * (unsigned __int128)cost_w[i]) >> 32), (int64_t)1024) + cost_b[i];
    };
    std::vector<std::vector<int64_t>> V(T, std::vector<int64_t>(n)), O(T, std::vector<int64_t>(n));
    for (int64_t i = 0; i < n; i++) V[0][i] = c(0, i), O[0][i] = lo + i;
    for (int64_t t = 1; t < T; t++)
        for (int64_t i = 0; i < n; i++) {
            const bool adv = !head[i] && V[t - 1][i - 1] < V[t - 1][i];
            V[t][i] = c(t, i) + (adv ? V[t - 1][i - 1] : V[t - 1][i]);
            O[t][i] = adv ? O[t - 1][i - 1] : O[t - 1][i];
            CHECK(V[t][i] > -(1 << 25) && V[t][i] < (1 << 25));
        }
    best.clear();
    for (int64_t j = 0; j < n_tgt; j++) {
        int64_t at = -1;
        for (int64_t i = 0; i < n; i++)
            if (tgt[i] == j && (at < 0 || V[T - 1][i] < V[T - 1][at])) at = i;
        if (at >= 0) best.push_back({V[T - 1][at], j, lo + at - P.off[j], O[T - 1][at] - P.off[j]});
    }
    std::sort(best.begin(), best.end());
}

static void rules_at_their_limits()
{
    CHECK(sm_status(0, 5, 9) == SM_EMPTY && sm_status(SM_MAX_T + 1, 0, 0) == SM_TOO_LONG && sm_status(SM_MAX_T, 0, 0) == SM_MAD_ZERO);
    CHECK(sm_status(1, 1, 0) == SM_NO_TARGET && sm_status(1, 1, 1) == SM_OK);
    const int64_t off[6] = {0, 0, 3, 3, 3, 7};
    CHECK(sm_target_of(off, 5, 0) == 1 && sm_target_of(off, 5, 2) == 1 && sm_target_of(off, 5, 3) == 4 && sm_target_of(off, 5, 6) == 4);
    CHECK(sm_key(-(1 << 25) + 1, 0) < sm_key(0, 0) && sm_key(7, 5) < sm_key(7, 6) && sm_key(7, 0xffffffffu) < sm_key(8, 0));
    CHECK(sm_key_score(sm_key(-12345, 77)) == -12345 && sm_key_state(sm_key(-12345, 0x7fffffffu)) == 0x7fffffffu);
    CHECK(sm_key((1 << 25) - 1, 0xffffffffu) < SM_NO_KEY);
    CHECK(sm_n_stripes(0) == 0 && sm_n_stripes(SM_PAYLOAD) == 1 && sm_n_stripes(SM_PAYLOAD + 1) == 2);
    CHECK(sm_stripe_left(100, 30, 0) == 71 && sm_stripe_left(100, 30, 90) == 90 && sm_stripe_left(5, 1, 5) == 5);
    CHECK(rd_sigmap_workspace_bytes(1, 1, 1) == 768 && rd_sigmap_workspace_bytes(-1, 0, 0) == -1);
    CHECK(rd_sigmap_workspace_bytes(SM_MAX_T, INT32_MAX, INT32_MAX) > 0);   // no overflow at the contract's largest query
}

// The yardsticks of sm_panel_layout and sm_io_layout: the size and offset expressions that rd_sigmap held before the layout functions
// replaced them, written out literally; on seeded random dimensions (0 and 1 of each among them) the totals and every offset must be equal.
static void check_layout()
{
    std::mt19937_64 rng(7);
    const size_t dims[] = {0, 1, 2, 31, 32, 33, 255, 256, 257};
    auto dim = [&](size_t big) { return rng() % 3 ? dims[rng() % 9] : (size_t)(rng() % big); };
    char* const base = (char*)((uintptr_t)1 << 32);
    for (int it = 0; it < 4000; it++) {
        const int n_tgt = (int)dim(50000), nb = (int)dim(4096);
        const int64_t R = (int64_t)dim(5000000);
        const size_t n_stripes = dim(100000);
        const size_t b_off = align_up((size_t)(n_tgt + 1) * 8, 256), b_st = align_up((size_t)R * 4 + 16, 256);
        SmPanel p;
        Carve pd, pw(base);
        sm_panel_layout(pd, n_tgt, R, &p);
        CHECK(pd.at == b_off + 2 * b_st && !p.off && !p.kid && !p.tg);
        sm_panel_layout(pw, n_tgt, R, &p);
        CHECK(pw.at == b_off + 2 * b_st && (char*)p.off == base && (char*)p.kid == base + b_off && (char*)p.tg == base + b_off + b_st);
        const size_t o_str = align_up((size_t)nb * sizeof(SmQuery), 256), o_out = o_str + align_up(n_stripes * sizeof(SmStripe), 256);
        const size_t total = o_out + (size_t)nb * sizeof(SmOut);
        SmIo io;
        Carve dry, wet(base);
        sm_io_layout(dry, nb, n_stripes, &io);
        CHECK(dry.at == total && !io.qs && !io.str && !io.out);
        sm_io_layout(wet, nb, n_stripes, &io);
        CHECK(wet.at == total && (char*)io.qs == base && (char*)io.str == base + o_str && (char*)io.out == base + o_out);
    }
}

int main(int argc, char** argv)
{
    const int iters = argc > 1 ? atoi(argv[1]) : 20;
    check_layout();
    rules_at_their_limits();
    std::mt19937_64 rng(2525);
    auto U = [&](int64_t a, int64_t b) { return (int64_t)(a + (int64_t)(rng() % (uint64_t)(b - a + 1))); };
    for (int it = 0; it < iters; it++) {
        Panel P;
        P.k = U(0, 1) ? 3 : 1;
        const int n_tgt = (int)U(1, 7), n_kmers = 1 << (2 * P.k);
        P.off.push_back(0);
        for (int j = 0; j < n_tgt; j++) {
            const int64_t L = U(0, 3) == 0 ? U(0, 1) : U(2, 40);
            for (int64_t b = 0; b < L; b++) P.codes.push_back((uint8_t)U(0, 3));
            P.off.push_back(P.off.back() + L);
        }
        const int64_t R = P.off.back();
        for (int i = 0; i < n_kmers; i++) {
            P.lvl.push_back((int32_t)U(-(1 << 14) + 1, (1 << 14) - 1));
            P.w.push_back(U(0, 4) == 0 ? (U(0, 1) ? 0u : 0xffffffffu) : (uint32_t)U(1 << 20, 1 << 28));
            P.bias.push_back((int32_t)U(-256, 256));
        }
        const int64_t n_raw = U(1, 60);
        std::vector<int16_t> raw(n_raw);
        for (auto& x : raw) x = (int16_t)(U(0, 9) == 0 ? U(-32768, 32767) : U(300, 900));
        const int n_q = (int)U(1, 5), n_best = (int)U(1, 8);
        std::vector<int64_t> q_lo(n_q), q_hi(n_q), sc_lo(n_q), sc_hi(n_q), s_lo(n_q), s_hi(n_q);
        std::vector<int32_t> m2_in(n_q), d4_in(n_q);
        for (int q = 0; q < n_q; q++) {
            q_lo[q] = U(0, n_raw), q_hi[q] = U(q_lo[q], n_raw);
            sc_lo[q] = U(0, n_raw), sc_hi[q] = U(sc_lo[q], n_raw);
            s_lo[q] = U(0, R), s_hi[q] = U(0, 5) == 0 ? s_lo[q] : U(s_lo[q], R);
            const bool given = U(0, 1);
            m2_in[q] = given ? (int32_t)U(-2000, 2000) : 0, d4_in[q] = given ? (int32_t)U(1, 2000) : 0;
        }
        int16_t* d_raw = exact(raw);
        uint8_t* d_codes = exact(P.codes);
        int64_t *d_off = exact(P.off), *d_qlo = exact(q_lo), *d_qhi = exact(q_hi), *d_sclo = exact(sc_lo), *d_schi = exact(sc_hi), *d_slo = exact(s_lo),
                *d_shi = exact(s_hi);
        int32_t *d_m2in = exact(m2_in), *d_d4in = exact(d4_in), *d_lvl = exact(P.lvl), *d_bias = exact(P.bias);
        uint32_t* d_w = exact(P.w);
        const std::vector<int32_t> fill_q(n_q, 0x5a5a5a5a), fill_b((size_t)n_q * n_best, 0x5a5a5a5a);
        int32_t *status = exact(fill_q), *m2 = exact(fill_q), *d4 = exact(fill_q), *bt = exact(fill_b), *bs = exact(fill_b), *be = exact(fill_b),
                *bo = exact(fill_b);
        auto call = [&](int nq, int nt, int k, int nb, int64_t nraw) {
            return rd_sigmap_host(d_raw, nraw, nq, d_qlo, d_qhi, d_sclo, d_schi, d_m2in, d_d4in, d_slo, d_shi, d_codes, d_off, nt, k, d_lvl, d_w, d_bias, nb,
                                  status, m2, d4, bt, bs, be, bo);
        };
        CHECK(call(n_q, n_tgt, P.k, n_best, n_raw) == 0);
        g_accepted++;
        std::vector<std::vector<int64_t>> best;
        std::vector<int64_t> cnt;
        for (int q = 0; q < n_q; q++) {
            const int64_t T = q_hi[q] - q_lo[q];
            int32_t um2 = m2_in[q], ud4 = d4_in[q];
            int want = SM_OK;
            if (T == 0) want = SM_EMPTY, um2 = ud4 = 0;
            else {
                if (ud4 == 0) {   // the two middle order statistics, by sorting
                    um2 = 0;
                    std::vector<int64_t> v(raw.begin() + sc_lo[q], raw.begin() + sc_hi[q]);
                    if (!v.empty()) {
                        std::sort(v.begin(), v.end());
                        um2 = (int32_t)(v[(v.size() - 1) / 2] + v[v.size() / 2]);
                        for (auto& x : v) x = std::llabs(2 * x - um2);
                        std::sort(v.begin(), v.end());
                        ud4 = (int32_t)(v[(v.size() - 1) / 2] + v[v.size() / 2]);
                    }
                }
                if (ud4 == 0) want = SM_MAD_ZERO;
                else if (s_lo[q] == s_hi[q]) want = SM_NO_TARGET;
            }
            CHECK(status[q] == want && m2[q] == um2 && d4[q] == ud4);
            best.clear();
            if (want == SM_OK) {
                std::vector<int32_t> zq(T);
                for (int64_t t = 0; t < T; t++) zq[t] = ea_quant(raw[q_lo[q] + t], um2, ud4);
                own_query(P, zq, s_lo[q], s_hi[q], best);
            }
            for (int r = 0; r < n_best; r++) {
                const int64_t o = (int64_t)q * n_best + r;
                if (r < (int)best.size()) CHECK(bs[o] == best[r][0] && bt[o] == best[r][1] && be[o] == best[r][2] && bo[o] == best[r][3]);
                else CHECK(bt[o] == -1 && bs[o] == -1 && be[o] == -1 && bo[o] == -1);
            }
        }
        // the refusals: nothing may be written
        for (int q = 0; q < n_q; q++) status[q] = 0x5a5a5a5a;
        auto refused = [&](int rc) {
            CHECK(rc == -1);
            for (int q = 0; q < n_q; q++) CHECK(status[q] == 0x5a5a5a5a);
            g_refused++;
        };
        refused(call(n_q, n_tgt, P.k, 0, n_raw));
        refused(call(n_q, n_tgt, P.k, 9, n_raw));
        refused(call(n_q, n_tgt, 2, n_best, n_raw));
        refused(call(n_q, n_tgt, 11, n_best, n_raw));
        refused(call(-1, n_tgt, P.k, n_best, n_raw));
        refused(call(n_q, -1, P.k, n_best, n_raw));
        refused(call(n_q, n_tgt, P.k, n_best, -1));
        { const int64_t keep = d_qhi[0]; d_qhi[0] = n_raw + 1; refused(call(n_q, n_tgt, P.k, n_best, n_raw)); d_qhi[0] = keep; }
        { const int64_t keep = d_qlo[0]; d_qlo[0] = d_qhi[0] + 1; refused(call(n_q, n_tgt, P.k, n_best, n_raw)); d_qlo[0] = keep; }
        { const int64_t keep = d_schi[0]; d_schi[0] = n_raw + 1; refused(call(n_q, n_tgt, P.k, n_best, n_raw)); d_schi[0] = keep; }
        { const int64_t keep = d_shi[n_q - 1]; d_shi[n_q - 1] = R + 1; refused(call(n_q, n_tgt, P.k, n_best, n_raw)); d_shi[n_q - 1] = keep; }
        { const int64_t keep = d_slo[0]; d_slo[0] = -1; refused(call(n_q, n_tgt, P.k, n_best, n_raw)); d_slo[0] = keep; }
        { const int32_t keep = d_d4in[0]; d_d4in[0] = -1; refused(call(n_q, n_tgt, P.k, n_best, n_raw)); d_d4in[0] = (1 << 20) + 1; refused(call(n_q, n_tgt, P.k, n_best, n_raw)); d_d4in[0] = keep; }
        { const int32_t keep = d_lvl[n_kmers - 1]; d_lvl[n_kmers - 1] = 1 << 14; refused(call(n_q, n_tgt, P.k, n_best, n_raw)); d_lvl[n_kmers - 1] = keep; }
        { const int32_t keep = d_bias[0]; d_bias[0] = -257; refused(call(n_q, n_tgt, P.k, n_best, n_raw)); d_bias[0] = keep; }
        if (R > 0) { const uint8_t keep = d_codes[R - 1]; d_codes[R - 1] = 4; refused(call(n_q, n_tgt, P.k, n_best, n_raw)); d_codes[R - 1] = keep; }
        { const int64_t keep = d_off[0]; d_off[0] = 1; refused(call(n_q, n_tgt, P.k, n_best, n_raw)); d_off[0] = keep; }
        if (n_tgt >= 2 && P.off[1] > 0) { const int64_t keep = d_off[1]; d_off[1] = d_off[2] + 1; refused(call(n_q, n_tgt, P.k, n_best, n_raw)); d_off[1] = keep; }
        CHECK(call(n_q, n_tgt, P.k, n_best, n_raw) == 0);   // and the buffers are as they were
        g_accepted++;
        for (void* p : {(void*)d_raw, (void*)d_codes, (void*)d_off, (void*)d_qlo, (void*)d_qhi, (void*)d_sclo, (void*)d_schi, (void*)d_slo, (void*)d_shi,
                        (void*)d_m2in, (void*)d_d4in, (void*)d_lvl, (void*)d_bias, (void*)d_w, (void*)status, (void*)m2, (void*)d4, (void*)bt, (void*)bs,
                        (void*)be, (void*)bo})
            free(p);
    }
    printf("no sanitizer report\n%ld accepted %ld refused\n", g_accepted, g_refused);
    return 0;
}
