// TEST INFRASTRUCTURE: AddressSanitizer + UBSan harness for the host side of rd_eventalign_events (radian_amd/csrc/eventalign.hip: the
// argument checks, the event-row rules of eventalign_rules.h, the plain loop of rd_eventalign_events_host; sanitizers run on the CPU build
// only -- the kernels are not compiled here).
// usage: asan_eventalign_events <iterations>   The rules at their limits first.  Every iteration draws a few reads (empty windows, reads
// without events, reads one row short of a path and all-skip reads among them), a model, a penalty and event records into EXACT-SIZE heap
// buffers (a read or a write past either end is an ASan report), calls the host twin and checks every field against a whole-table loop of
// its own written from the contract's text; then the same buffers go through the refusals, which must answer RD_ERR_ARG and write nothing.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../radian_amd/csrc/eventalign.hip"   // the host half (this is no HIP build)

extern "C" int rd_event_stats_host(const int16_t*, const int64_t*, int, const int32_t*, const int32_t*, const int64_t*, const int32_t*, const int32_t*,
                                   int32_t*, int32_t*, int64_t*, int64_t*, int16_t*, int16_t*)
{
    return RD_ERR_STATE;   // (rd_eventalign_host's; not under test here)
}
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

static void rules_at_their_limits()
{
    CHECK(ear_pen_ok(-1) && ear_pen_ok(0) && ear_pen_ok(256) && !ear_pen_ok(-2) && !ear_pen_ok(257));
    CHECK(ear_mean(7, 2) == 4 && ear_mean(-7, 2) == -3 && ear_mean(6, 4) == 2 && ear_mean(-6, 4) == -1 && ear_mean(-32768, 1) == -32768);
    CHECK(ear_mean((int64_t)32767 << 19, 1 << 19) == 32767 && ear_mean(-((int64_t)32768 << 19), 1 << 19) == -32768);
    CHECK(ear_status(0, 3, 1, 5, 0) == EA_EMPTY && ear_status(9, 0, 1, 5, 0) == EA_EMPTY && ear_status(EA_MAX_T + 1, 3, 1, 5, 0) == EA_TOO_LONG);
    CHECK(ear_status(EA_MAX_T + 1, 0, 1, 5, 0) == EA_EMPTY && ear_status(9, 3, 1, 0, 0) == EA_MAD_ZERO && ear_status(EA_MAX_T, 3, 9, 0, 0) == EA_MAD_ZERO);
    CHECK(ear_status(9, 3, 5, 1, 0) == EA_OK && ear_status(9, 3, 6, 1, 0) == EA_NO_PATH && ear_status(9, 3, 3, 1, -1) == EA_OK &&
          ear_status(9, 3, 4, 1, -1) == EA_NO_PATH);
    // the largest cell: 2^19 samples at the cap with bias 256, and the smallest
    CHECK(ear_cost(EA_ZMAX, 1 << 19, -EA_ZMAX + 1, 0xffffffffu, 256) == (1 << 19) * 1280 && ear_cost(0, 1 << 19, 0, 0, -256) == -(1 << 19) * 256);
    int code;
    CHECK(ear_best(5, 5, 5, true, &code) == 5 && code == EAR_STAY);
    CHECK(ear_best(5, 4, 4, true, &code) == 4 && code == EAR_ADV);
    CHECK(ear_best(5, 4, 3, true, &code) == 3 && code == EAR_SKIP);
    CHECK(ear_best(5, 6, 4, true, &code) == 4 && code == EAR_SKIP);
    CHECK(ear_best(5, 6, 4, false, &code) == 5 && code == EAR_STAY);
    CHECK(ear_best(EA_INF, EA_INF, EA_INF + 256, true, &code) == EA_INF && code == EAR_STAY);
}

struct Read {
    int64_t T, off;
    std::vector<int32_t> start;
    std::vector<int64_t> sum, sumsq;
    std::vector<int16_t> mn, mx;
    std::vector<uint8_t> codes;
    int32_t m2, d4;
};

struct Want {
    int32_t status = 0, n_skipped = 0;
    int64_t score = 0, sums[5] = {0, 0, 0, 0, 0};
    std::vector<int32_t> first, last, start, end;
    std::vector<int64_t> sum, sumsq;
    std::vector<int16_t> mn, mx;
};

// the contract over one read, the whole table kept, in 64 bits
static Want own_align(const Read& rd, int k, const std::vector<int32_t>& lvl, const std::vector<uint32_t>& w, const std::vector<int32_t>& bias,
                      const EaState& bg, int pen)
{
    const int64_t T = rd.T, E = (int64_t)rd.start.size(), L = (int64_t)rd.codes.size(), S = L + 2;
    Want o;
    o.first.assign(L, -1), o.last.assign(L, -1), o.start.assign(L, -1), o.end.assign(L, -1);
    o.sum.assign(L, 0), o.sumsq.assign(L, 0), o.mn.assign(L, 0), o.mx.assign(L, 0);
    o.status = (T == 0 || E == 0) ? 1 : T > (1 << 19) ? 2 : rd.d4 == 0 ? 3 : (pen < 0 ? E : 2 * E - 1) < L ? 4 : 0;
    if (o.status) return o;
    const int64_t INF = (int64_t)1 << 30;
    std::vector<int64_t> n(E), z(E), sl(S), sw(S), sb(S);
    for (int64_t e = 0; e < E; e++) {
        n[e] = (e + 1 < E ? rd.start[e + 1] : T) - rd.start[e];
        int64_t num = 2 * rd.sum[e] + n[e], den = 2 * n[e], x = num / den;
        if (num % den < 0) x--;
        const int64_t u = 512 * (2 * x - rd.m2), num2 = 2 * u + rd.d4, den2 = 2 * (int64_t)rd.d4;
        int64_t q = num2 / den2;
        if (num2 % den2 < 0) q--;
        z[e] = std::max<int64_t>(-(1 << 14), std::min<int64_t>(1 << 14, q));
    }
    for (int64_t s = 0; s < S; s++) {
        if (s == 0 || s == L + 1) {
            sl[s] = bg.lvl, sw[s] = bg.w, sb[s] = bg.bias;
            continue;
        }
        int64_t idx = 0;
        for (int j = -(k / 2); j <= k / 2; j++) idx = idx * 4 + rd.codes[std::min<int64_t>(std::max<int64_t>(s - 1 + j, 0), L - 1)];
        sl[s] = lvl[idx], sw[s] = w[idx], sb[s] = bias[idx];
    }
    const auto cell = [&](int64_t e, int64_t s) {
        const int64_t d = z[e] - sl[s];
        return n[e] * (std::min<int64_t>((int64_t)(((unsigned __int128)(d * d) * (uint64_t)sw[s]) >> 32), 1024) + sb[s]);
    };
    std::vector<int64_t> V((size_t)(E * S), INF);
    std::vector<uint8_t> code((size_t)(E * S), 0);
    V[0] = cell(0, 0);
    V[1] = cell(0, 1);
    for (int64_t e = 1; e < E; e++)
        for (int64_t s = 0; s <= std::min(S - 1, pen < 0 ? e + 1 : 2 * e + 1); s++) {
            int64_t best = V[(e - 1) * S + s];
            uint8_t c = 0;
            if (s >= 1 && V[(e - 1) * S + s - 1] < best) best = V[(e - 1) * S + s - 1], c = 1;
            if (pen >= 0 && s >= 2 && V[(e - 1) * S + s - 2] + pen < best) best = V[(e - 1) * S + s - 2] + pen, c = 2;
            CHECK(best < 3 * (INF >> 2));
            V[e * S + s] = cell(e, s) + best;
            code[e * S + s] = c;
        }
    int64_t s = V[(E - 1) * S + L + 1] < V[(E - 1) * S + L] ? L + 1 : L;
    o.score = V[(E - 1) * S + s];
    std::vector<int64_t> jump(L, -1);
    if (s >= 1 && s <= L) o.last[s - 1] = (int32_t)(E - 1);
    for (int64_t e = E - 1; e > 0; e--) {
        const int c = code[e * S + s];
        if (!c) continue;
        if (s <= L) o.first[s - 1] = (int32_t)e;
        if (c == 2) jump[s - 2] = e, o.n_skipped++;
        if (s - c >= 1) o.last[s - c - 1] = (int32_t)(e - 1);
        s -= c;
    }
    CHECK(s == 0 || s == 1);
    if (s == 1 && L >= 1) o.first[0] = 0;
    for (int64_t b = 0; b < L; b++) {
        if (jump[b] >= 0) {
            CHECK(o.first[b] == -1 && o.last[b] == -1);
            o.start[b] = o.end[b] = (int32_t)(rd.start[jump[b]] + rd.off);
            continue;
        }
        const int64_t f = o.first[b], l = o.last[b];
        CHECK(0 <= f && f <= l && l < E);
        o.start[b] = (int32_t)(rd.start[f] + rd.off);
        o.end[b] = (int32_t)((l + 1 < E ? rd.start[l + 1] : T) + rd.off);
        o.mn[b] = rd.mn[f], o.mx[b] = rd.mx[f];
        for (int64_t e = f; e <= l; e++) {
            o.sum[b] += rd.sum[e], o.sumsq[b] += rd.sumsq[e];
            o.mn[b] = std::min(o.mn[b], rd.mn[e]), o.mx[b] = std::max(o.mx[b], rd.mx[e]);
        }
        const int64_t lv = sl[b + 1], cnt = o.end[b] - o.start[b];
        o.sums[0] += cnt, o.sums[1] += cnt * lv, o.sums[2] += cnt * lv * lv, o.sums[3] += o.sum[b], o.sums[4] += o.sum[b] * lv;
    }
    return o;
}

int main(int argc, char** argv)
{
    const int iters = argc > 1 ? atoi(argv[1]) : 50;
    rules_at_their_limits();
    std::mt19937_64 rng(28);
    const auto rnd = [&](int64_t lo, int64_t hi) { return lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1)); };
    for (int it = 0; it < iters; it++) {
        const int k = (int)(2 * rnd(0, 2) + 1), n_kmers = 1 << (2 * k), n_reads = (int)rnd(1, 5), pen = (int)std::vector<int>{-1, 0, 32, 96, 256}[rnd(0, 4)];
        std::vector<int32_t> lvl(n_kmers), bias(n_kmers);
        std::vector<uint32_t> w(n_kmers);
        for (int i = 0; i < n_kmers; i++) {
            lvl[i] = (int32_t)rnd(-1600, 1600), bias[i] = (int32_t)rnd(-256, 256);
            w[i] = rnd(0, 9) == 0 ? (rnd(0, 1) ? 0u : 0xffffffffu) : (uint32_t)rnd(1 << 18, 1 << 30);
        }
        lvl[0] = -(1 << 14) + 1, lvl[n_kmers - 1] = (1 << 14) - 1;
        const EaState bg{(int32_t)rnd(-50, 50), (uint32_t)rnd(1 << 17, 1 << 20), (int32_t)rnd(-20, 20)};
        std::vector<Read> reads(n_reads);
        std::vector<int64_t> n_samples, sample_off, ev_off, ref_off;
        std::vector<int32_t> n_events, ref_len, m2, d4, in_start;
        std::vector<int64_t> in_sum, in_sumsq;
        std::vector<int16_t> in_min, in_max;
        std::vector<uint8_t> codes;
        for (Read& rd : reads) {
            const int kind = (int)rnd(0, 9);
            int64_t E = kind == 0 ? 0 : rnd(1, 40);
            const int64_t L = kind == 1 ? (pen < 0 ? E + 1 : 2 * E) : kind == 2 ? (pen < 0 ? E : 2 * E - 1) : rnd(0, 30);   // one short; the last that fits
            rd.off = rnd(0, 1) ? rnd(0, 100000) : 0;
            rd.m2 = (int32_t)rnd(1100, 1300), rd.d4 = kind == 3 ? 0 : (int32_t)rnd(kind == 4 ? 8 : 200, kind == 4 ? 20 : 300);
            std::vector<int16_t> x;
            for (int64_t e = 0; e < E; e++) {
                const int64_t n = rnd(0, 5) ? rnd(1, 12) : 1;
                const int v = kind == 4 && rnd(0, 3) == 0 ? (rnd(0, 1) ? 32767 : -32768) : (int)rnd(200, 1000);
                rd.start.push_back((int32_t)x.size());
                int64_t s = 0, q = 0;
                int16_t lo = 32767, hi = -32768;
                for (int64_t i = 0; i < n; i++) {
                    const int16_t y = (int16_t)std::max<int64_t>(-32768, std::min<int64_t>(32767, v + rnd(-4, 4)));
                    x.push_back(y), s += y, q += (int64_t)y * y, lo = std::min(lo, y), hi = std::max(hi, y);
                }
                rd.sum.push_back(s), rd.sumsq.push_back(q), rd.mn.push_back(lo), rd.mx.push_back(hi);
            }
            rd.T = kind == 0 && rnd(0, 1) ? rnd(1, 50) : (int64_t)x.size();
            for (int64_t b = 0; b < L; b++) rd.codes.push_back((uint8_t)rnd(0, 3));
            n_samples.push_back(rd.T), sample_off.push_back(rd.off), n_events.push_back((int32_t)E), m2.push_back(rd.m2), d4.push_back(rd.d4);
            ev_off.push_back((int64_t)in_start.size()), ref_off.push_back((int64_t)codes.size()), ref_len.push_back((int32_t)L);
            in_start.insert(in_start.end(), rd.start.begin(), rd.start.end());
            in_sum.insert(in_sum.end(), rd.sum.begin(), rd.sum.end());
            in_sumsq.insert(in_sumsq.end(), rd.sumsq.begin(), rd.sumsq.end());
            in_min.insert(in_min.end(), rd.mn.begin(), rd.mn.end());
            in_max.insert(in_max.end(), rd.mx.begin(), rd.mx.end());
            codes.insert(codes.end(), rd.codes.begin(), rd.codes.end());
        }
        const size_t nb = codes.size();
        int64_t *p_ns = exact(n_samples), *p_so = exact(sample_off), *p_eo = exact(ev_off), *p_ro = exact(ref_off), *p_sum = exact(in_sum), *p_sq = exact(in_sumsq);
        int32_t *p_ne = exact(n_events), *p_rl = exact(ref_len), *p_m2 = exact(m2), *p_d4 = exact(d4), *p_st = exact(in_start), *p_lvl = exact(lvl), *p_bias = exact(bias);
        int16_t *p_mn = exact(in_min), *p_mx = exact(in_max);
        uint32_t* p_w = exact(w);
        uint8_t* p_codes = exact(codes);
        const std::vector<int32_t> fill4(nb, 77), fillr(n_reads, 77);
        const std::vector<int64_t> fill8(nb, 77), fillr8(n_reads, 77), fills(5 * (size_t)n_reads, 77);
        const std::vector<int16_t> fill2(nb, 77);
        int32_t *status = exact(fillr), *nskip = exact(fillr), *first = exact(fill4), *last = exact(fill4), *start = exact(fill4), *end = exact(fill4);
        int64_t *score = exact(fillr8), *sum = exact(fill8), *sumsq = exact(fill8), *sums = exact(fills);
        int16_t *mn = exact(fill2), *mx = exact(fill2);
        const auto call = [&](int n, int kk, int pp) {
            return rd_eventalign_events_host(n, p_ns, p_so, p_eo, p_ne, p_st, p_sum, p_sq, p_mn, p_mx, p_codes, p_ro, p_rl, p_m2, p_d4, kk, p_lvl, p_w, p_bias,
                                             bg.lvl, bg.w, bg.bias, pp, status, score, nskip, first, last, start, end, sum, sumsq, mn, mx, sums);
        };
        CHECK(call(n_reads, k, pen) == RD_OK);
        g_accepted++;
        for (int r = 0; r < n_reads; r++) {
            const Want o = own_align(reads[r], k, lvl, w, bias, bg, pen);
            const size_t at = (size_t)ref_off[r], L = reads[r].codes.size();
            CHECK(status[r] == o.status && score[r] == o.score && nskip[r] == o.n_skipped && !memcmp(sums + 5 * r, o.sums, 40));
            for (size_t b = 0; b < L; b++)
                CHECK(first[at + b] == o.first[b] && last[at + b] == o.last[b] && start[at + b] == o.start[b] && end[at + b] == o.end[b] &&
                      sum[at + b] == o.sum[b] && sumsq[at + b] == o.sumsq[b] && mn[at + b] == o.mn[b] && mx[at + b] == o.mx[b]);
        }
        // the refusals: RD_ERR_ARG, and nothing is written
        for (int r = 0; r < n_reads; r++) status[r] = nskip[r] = 77, score[r] = 77;
        const auto refused = [&](int rc) {
            CHECK(rc == RD_ERR_ARG);
            for (int r = 0; r < n_reads; r++) CHECK(status[r] == 77 && nskip[r] == 77 && score[r] == 77);
            g_refused++;
        };
        refused(call(-1, k, pen));
        refused(call(n_reads, 2, pen));
        refused(call(n_reads, 11, pen));
        refused(call(n_reads, k, -2));
        refused(call(n_reads, k, 257));
        const int r = (int)rnd(0, n_reads - 1);
        const auto with = [&](auto* p, auto v) {
            const auto keep = *p;
            *p = v;
            refused(call(n_reads, k, pen));
            *p = keep;
        };
        with(p_ns + r, (int64_t)-1);
        with(p_so + r, (int64_t)-1);
        with(p_so + r, (int64_t)INT32_MAX - p_ns[r] + 1);
        with(p_eo + r, (int64_t)-1);
        with(p_ne + r, (int32_t)-1);
        with(p_rl + r, (int32_t)-1);
        with(p_d4 + r, (int32_t)-1);
        with(p_d4 + r, (int32_t)(1 << 20) + 1);
        with(p_m2 + r, (int32_t)(1 << 17) + 1);
        with(p_lvl + rnd(0, n_kmers - 1), (int32_t)(1 << 14));
        with(p_bias + rnd(0, n_kmers - 1), (int32_t)257);
        if (nb) with(p_codes + rnd(0, (int64_t)nb - 1), (uint8_t)4);
        if (n_events[r]) {
            const int64_t E = n_events[r], e = rnd(0, E - 1), at = ev_off[r];
            with(p_st + at, (int32_t)1);                                        // event 0 does not start at 0
            if (e > 0) with(p_st + at + e, p_st[at + e - 1]);                   // not strictly increasing
            with(p_st + at + E - 1, (int32_t)p_ns[r]);                          // a start at T
            const int64_t n = (e + 1 < E ? p_st[at + e + 1] : p_ns[r]) - p_st[at + e];
            if (p_ns[r] > p_st[at + E - 1]) {
                with(p_sum + at + e, 32767 * n + 1);                            // a mean above int16
                with(p_sum + at + e, -32768 * n - 1);
            }
        }
        for (void* p : {(void*)p_ns, (void*)p_so, (void*)p_eo, (void*)p_ro, (void*)p_sum, (void*)p_sq, (void*)p_ne, (void*)p_rl, (void*)p_m2, (void*)p_d4,
                        (void*)p_st, (void*)p_lvl, (void*)p_bias, (void*)p_mn, (void*)p_mx, (void*)p_w, (void*)p_codes, (void*)status, (void*)nskip,
                        (void*)first, (void*)last, (void*)start, (void*)end, (void*)score, (void*)sum, (void*)sumsq, (void*)sums, (void*)mn, (void*)mx})
            free(p);
    }
    CHECK(rd_eventalign_events_workspace_bytes(-1, 0) == -1 && rd_eventalign_events_workspace_bytes(1, 0) == 512);
    CHECK(rd_eventalign_events_workspace_bytes(1000, 4095) == 8192 + 1028096 + 16128);   // 8000, 4 * 1000 * 257 and 16000, each rounded up to 256
    printf("no sanitizer report\n%ld accepted %ld refused\n", g_accepted, g_refused);
    return 0;
}
