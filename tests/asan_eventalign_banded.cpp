// TEST INFRASTRUCTURE: AddressSanitizer + UBSan harness for the host side of rd_eventalign_banded (radian_amd/csrc/eventalign.hip: the
// argument checks, the window rules of eventalign_rules.h, the plain loop of rd_eventalign_banded_host; sanitizers run on the CPU build
// only -- the kernels are not compiled here).
// usage: asan_eventalign_banded <iterations>   The rules at their limits first.  Every iteration draws a few reads (empty windows, reads a
// sample short of a path, reads on both sides of 64 states, guides on the path, off it, all before and all after the window among them)
// and a model into EXACT-SIZE heap buffers (a read or a write past either end is an ASan report), calls the host twin and checks every
// field against a whole-table loop of its own written from the contract's text; then the same buffers go through the refusals, which must
// answer RD_ERR_ARG and write nothing.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../radian_amd/csrc/eventalign.hip"   // the host half (this is no HIP build)

// rd_event_stats_host's rule (events.hip), restated: event b is samples first[b] .. first[b + 1] - 1, the last ends at last[L - 1]
extern "C" int rd_event_stats_host(const int16_t* raw, const int64_t* read_off, int n_reads, const int32_t* first, const int32_t* last, const int64_t* lab_off,
                                   const int32_t* lab_len, const int32_t* skip, int32_t* start, int32_t* end, int64_t* sum, int64_t* sumsq, int16_t* mn,
                                   int16_t* mx)
{
    for (int r = 0; r < n_reads; r++)
        for (int b = 0; b < lab_len[r]; b++) {
            const int64_t o = lab_off[r] + b;
            start[o] = end[o] = -1, sum[o] = sumsq[o] = 0, mn[o] = mx[o] = 0;
            if (skip[r]) continue;
            const int32_t s = first[o], e = b + 1 < lab_len[r] ? first[o + 1] : last[lab_off[r] + lab_len[r] - 1] + 1;
            int16_t lo = 32767, hi = -32768;
            for (int32_t t = s; t < e; t++) {
                const int16_t x = raw[read_off[r] + t];
                sum[o] += x, sumsq[o] += (int64_t)x * x, lo = std::min(lo, x), hi = std::max(hi, x);
            }
            start[o] = s, end[o] = e, mn[o] = lo, mx[o] = hi;
        }
    return RD_OK;
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
    CHECK(EAB_W == 64 && EA_OFF_BAND == 6 && EAB_FINITE == 3 * (1 << 28));
    CHECK(eab_lo(0, 64) == 0 && eab_lo(31, 64) == 0 && eab_lo(32, 64) == 1 && eab_lo(33, 64) == 2 && eab_lo(64, 64) == 2);
    CHECK(eab_lo(62, 62) == 0 && eab_lo(0, 0) == 0 && eab_lo((1 << 29) - 1, (1 << 29) - 1) == (1 << 29) - 1 + 2 - 64);
    const int32_t g[5] = {INT32_MIN, -3, 7, 7, INT32_MAX};
    CHECK(eab_count(g, 5, (int64_t)INT32_MIN - 1) == 0 && eab_count(g, 5, INT32_MIN) == 1 && eab_count(g, 5, 6) == 2 && eab_count(g, 5, 7) == 4);
    CHECK(eab_count(g, 5, (int64_t)INT32_MAX - 1) == 4 && eab_count(g, 5, (int64_t)INT32_MAX + (1 << 19)) == 5 && eab_count(g, 0, 0) == 0);
    CHECK(eab_finite((1 << 19) * 1280) && !eab_finite(EA_INF - (1 << 19) * 256) && !eab_finite(EAB_FINITE) && eab_finite(EAB_FINITE - 1));
    CHECK(eab_on_rim(5, 5, 0) && eab_on_rim(63, 0, 0) && !eab_on_rim(62, 0, 0) && !eab_on_rim(5, 4, 0) && eab_on_rim(100, 3, 37));
}

struct Read {
    std::vector<int16_t> x;   // the whole read
    int64_t t_lo, t_hi;
    std::vector<uint8_t> codes;
    std::vector<int32_t> guide;
    int32_t m2, d4;
};

struct Want {
    int32_t status = 0, n_edge = 0, m2 = 0, d4 = 0;
    int64_t score = 0, sums[5] = {0, 0, 0, 0, 0};
    std::vector<int32_t> first, last;
};

// the contract over one read, the whole T x (L + 2) table kept with 2^30 outside the windows, in 64 bits
static Want own_align(const Read& rd, int k, const std::vector<int32_t>& lvl, const std::vector<uint32_t>& w, const std::vector<int32_t>& bias,
                      const EaState& bg)
{
    const int64_t T = rd.t_hi - rd.t_lo, L = (int64_t)rd.codes.size(), S = L + 2, INF = (int64_t)1 << 30;
    Want o;
    o.first.assign(L, -1), o.last.assign(L, -1);
    if (T == 0) return o.status = 1, o;
    int64_t m2 = rd.m2, d4 = rd.d4;
    if (d4 == 0) {
        std::vector<int64_t> v(rd.x.begin() + rd.t_lo, rd.x.begin() + rd.t_hi);
        std::sort(v.begin(), v.end());
        m2 = v[(T - 1) / 2] + v[T / 2];
        for (auto& y : v) y = std::llabs(2 * y - m2);
        std::sort(v.begin(), v.end());
        d4 = v[(T - 1) / 2] + v[T / 2];
    }
    o.m2 = (int32_t)m2, o.d4 = (int32_t)d4;
    if (d4 == 0) return o.status = 3, o;
    if (T < L) return o.status = 4, o;
    std::vector<int64_t> z(T), lo(T), sl(S), sw(S), sb(S);
    for (int64_t t = 0; t < T; t++) {
        const int64_t u = 512 * (2 * (int64_t)rd.x[rd.t_lo + t] - m2), num = 2 * u + d4, den = 2 * d4;
        int64_t q = num / den;
        if (num % den < 0) q--;
        z[t] = std::max<int64_t>(-(1 << 14), std::min<int64_t>(1 << 14, q));
        int64_t g = 0;
        for (int64_t b = 0; b < L; b++) g += rd.guide[b] <= rd.t_lo + t;
        lo[t] = std::min(std::max<int64_t>(g - 31, 0), std::max<int64_t>(S - 64, 0));
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
    const auto cell = [&](int64_t t, int64_t s) {
        const int64_t d = z[t] - sl[s];
        return std::min<int64_t>((int64_t)(((unsigned __int128)(d * d) * (uint64_t)sw[s]) >> 32), 1024) + sb[s];
    };
    const auto in_win = [&](int64_t t, int64_t s) { return s >= lo[t] && s <= std::min(lo[t] + 63, S - 1); };
    std::vector<int64_t> V((size_t)(T * S), INF);
    std::vector<uint8_t> adv((size_t)(T * S), 0);
    for (int64_t s = 0; s < 2; s++)
        if (in_win(0, s)) V[s] = cell(0, s);
    for (int64_t t = 1; t < T; t++)
        for (int64_t s = 0; s < S; s++) {
            if (!in_win(t, s)) continue;
            const int64_t stay = in_win(t - 1, s) ? V[(t - 1) * S + s] : INF;
            const int64_t a = s - 1 >= lo[t] && in_win(t - 1, s - 1) ? V[(t - 1) * S + s - 1] : INF;
            adv[t * S + s] = a < stay;
            V[t * S + s] = cell(t, s) + std::min(a, stay);
        }
    const int64_t v_trail = in_win(T - 1, L + 1) ? V[(T - 1) * S + L + 1] : INF, v_last = in_win(T - 1, L) ? V[(T - 1) * S + L] : INF;
    int64_t s = v_trail < v_last ? L + 1 : L;
    const int64_t end = std::min(v_trail, v_last);
    if (end >= 3 * ((int64_t)1 << 28)) return o.status = 6, o;
    o.score = end;
    const int32_t off = (int32_t)rd.t_lo;
    if (s >= 1 && s <= L) o.last[s - 1] = (int32_t)(T - 1) + off;
    for (int64_t t = T - 1; t > 0; t--) {
        if (!adv[t * S + s]) continue;
        if (s <= L) o.first[s - 1] = (int32_t)t + off;
        if (s >= 2) o.last[s - 2] = (int32_t)t - 1 + off;
        s--;
    }
    if (s == 1 && L >= 1) o.first[0] = off;
    for (int64_t b = 0; b < L; b++) {
        o.n_edge += lo[o.last[b] - off] == b + 1 || lo[o.first[b] - off] + 63 == b + 1;
        int64_t idx = 0;
        for (int j = -(k / 2); j <= k / 2; j++) idx = idx * 4 + rd.codes[std::min<int64_t>(std::max<int64_t>(b + j, 0), L - 1)];
        const int64_t e = b + 1 < L ? o.first[b + 1] : o.last[L - 1] + 1, n = e - o.first[b], l = lvl[idx];
        int64_t x = 0;
        for (int64_t t = o.first[b]; t < e; t++) x += rd.x[t];
        o.sums[0] += n, o.sums[1] += n * l, o.sums[2] += n * l * l, o.sums[3] += x, o.sums[4] += x * l;
    }
    return o;
}

int main(int argc, char** argv)
{
    const long iters = argc > 1 ? atol(argv[1]) : 100;
    rules_at_their_limits();
    std::mt19937_64 gen(20261);
    const auto rnd = [&](int64_t lo, int64_t hi) { return (int64_t)(gen() % (uint64_t)(hi - lo + 1)) + lo; };
    static const int64_t sizes[6] = {61, 62, 63, 64, 90, 140};   // bases: on both sides of 64 states
    for (long it = 0; it < iters; it++) {
        const int k = (int)(2 * rnd(0, 2) + 1), n_kmers = 1 << (2 * k), n_reads = (int)rnd(1, 4);
        std::vector<int32_t> lvl(n_kmers), bias(n_kmers);
        std::vector<uint32_t> w(n_kmers);
        for (int i = 0; i < n_kmers; i++) {
            lvl[i] = (int32_t)rnd(-1600, 1600), bias[i] = (int32_t)rnd(-256, 256);
            w[i] = rnd(0, 9) == 0 ? (rnd(0, 1) ? 0u : 0xffffffffu) : (uint32_t)rnd(1 << 18, 1 << 30);
        }
        lvl[0] = -(1 << 14) + 1, lvl[n_kmers - 1] = (1 << 14) - 1;
        const EaState bg{(int32_t)rnd(-50, 50), (uint32_t)rnd(1 << 17, 1 << 20), (int32_t)rnd(-20, 20)};
        std::vector<Read> reads(n_reads);
        std::vector<int16_t> raw;
        std::vector<int64_t> read_off{0}, t_lo, t_hi, ref_off;
        std::vector<int32_t> ref_len, m2, d4, guide;
        std::vector<uint8_t> codes;
        for (Read& rd : reads) {
            const int kind = (int)rnd(0, 11);
            const int64_t L = kind == 5 ? rnd(0, 5) : sizes[rnd(0, 5)] * (rnd(0, 3) ? 1 : 0) + rnd(0, 3);
            const int64_t T = kind == 0 ? 0 : kind == 1 ? std::max<int64_t>(L - 1, 0) : kind == 2 ? std::max<int64_t>(L, 1) : L + rnd(1, 3 * L + 20);
            const int64_t before = rnd(0, 1) ? rnd(0, 30) : 0, after = rnd(0, 1) ? rnd(0, 30) : 0;
            rd.t_lo = before, rd.t_hi = before + T;
            for (int64_t t = 0; t < before + T + after; t++)
                rd.x.push_back((int16_t)(kind == 3 ? 700 : kind == 4 && rnd(0, 3) == 0 ? (rnd(0, 1) ? 32767 : -32768) : rnd(200, 1000)));
            rd.m2 = (int32_t)rnd(1100, 1300), rd.d4 = kind == 3 || kind == 6 ? 0 : (int32_t)rnd(kind == 4 ? 8 : 200, kind == 4 ? 20 : 300);
            for (int64_t b = 0; b < L; b++) rd.codes.push_back((uint8_t)rnd(0, 3));
            // guides: a diagonal (runs where T < 2 L), a diagonal moved by up to 40 states, all before, all after, one value, random sorted
            const int gk = (int)rnd(0, 6);
            const int64_t mv = rnd(-40, 40);
            for (int64_t b = 0; b < L; b++) {
                const int64_t diag = before + (L ? (b + (gk == 1 ? mv : 0)) * T / L : 0);
                rd.guide.push_back((int32_t)(gk <= 1 ? diag : gk == 2 ? -7 : gk == 3 ? before + T + 9 : gk == 4 ? before + T / 2 : rnd(before - 5, before + T + 5)));
            }
            std::sort(rd.guide.begin(), rd.guide.end());
            raw.insert(raw.end(), rd.x.begin(), rd.x.end());
            read_off.push_back((int64_t)raw.size()), t_lo.push_back(rd.t_lo), t_hi.push_back(rd.t_hi), m2.push_back(rd.m2), d4.push_back(rd.d4);
            ref_off.push_back((int64_t)codes.size()), ref_len.push_back((int32_t)L);
            codes.insert(codes.end(), rd.codes.begin(), rd.codes.end());
            guide.insert(guide.end(), rd.guide.begin(), rd.guide.end());
        }
        const size_t nb = codes.size();
        int16_t* p_raw = exact(raw);
        int64_t *p_off = exact(read_off), *p_lo = exact(t_lo), *p_hi = exact(t_hi), *p_ro = exact(ref_off);
        int32_t *p_rl = exact(ref_len), *p_m2 = exact(m2), *p_d4 = exact(d4), *p_g = exact(guide), *p_lvl = exact(lvl), *p_bias = exact(bias);
        uint32_t* p_w = exact(w);
        uint8_t* p_codes = exact(codes);
        const std::vector<int32_t> fill4(nb, 77), fillr(n_reads, 77);
        const std::vector<int64_t> fill8(nb, 77), fillr8(n_reads, 77), fills(5 * (size_t)n_reads, 77);
        const std::vector<int16_t> fill2(nb, 77);
        int32_t *status = exact(fillr), *o_m2 = exact(fillr), *o_d4 = exact(fillr), *nedge = exact(fillr), *first = exact(fill4), *last = exact(fill4),
                *start = exact(fill4), *end = exact(fill4);
        int64_t *score = exact(fillr8), *sum = exact(fill8), *sumsq = exact(fill8), *sums = exact(fills);
        int16_t *mn = exact(fill2), *mx = exact(fill2);
        const auto call = [&](int n, int kk) {
            return rd_eventalign_banded_host(p_raw, p_off, n, p_lo, p_hi, p_codes, p_ro, p_rl, p_g, p_m2, p_d4, kk, p_lvl, p_w, p_bias, bg.lvl, bg.w, bg.bias,
                                             status, score, o_m2, o_d4, nedge, first, last, start, end, sum, sumsq, mn, mx, sums);
        };
        CHECK(call(n_reads, k) == RD_OK);
        g_accepted++;
        for (int r = 0; r < n_reads; r++) {
            Read rd = reads[r];
            const int64_t base = read_off[r];
            const Want o = own_align(rd, k, lvl, w, bias, bg);
            const size_t at = (size_t)ref_off[r], L = rd.codes.size();
            CHECK(status[r] == o.status && score[r] == o.score && nedge[r] == o.n_edge && o_m2[r] == o.m2 && o_d4[r] == o.d4 && !memcmp(sums + 5 * r, o.sums, 40));
            for (size_t b = 0; b < L; b++) {
                CHECK(first[at + b] == o.first[b] && last[at + b] == o.last[b] && start[at + b] == o.first[b]);
                if (o.status == 0) {
                    const int32_t e = b + 1 < L ? o.first[b + 1] : o.last[L - 1] + 1;
                    int64_t s = 0;
                    for (int32_t t = o.first[b]; t < e; t++) s += p_raw[base + t];
                    CHECK(end[at + b] == e && sum[at + b] == s);
                } else
                    CHECK(end[at + b] == -1 && sum[at + b] == 0 && sumsq[at + b] == 0 && mn[at + b] == 0 && mx[at + b] == 0);
            }
        }
        // the refusals: RD_ERR_ARG, and nothing is written
        for (int r = 0; r < n_reads; r++) status[r] = nedge[r] = 77, score[r] = 77;
        const auto refused = [&](int rc) {
            CHECK(rc == RD_ERR_ARG);
            for (int r = 0; r < n_reads; r++) CHECK(status[r] == 77 && nedge[r] == 77 && score[r] == 77);
            g_refused++;
        };
        refused(call(-1, k));
        refused(call(n_reads, 2));
        refused(call(n_reads, 11));
        const int r = (int)rnd(0, n_reads - 1);
        const auto with = [&](auto* p, auto v) {
            const auto keep = *p;
            *p = v;
            refused(call(n_reads, k));
            *p = keep;
        };
        with(p_lo + r, (int64_t)-1);
        with(p_hi + r, read_off[r + 1] - read_off[r] + 1);
        with(p_rl + r, (int32_t)-1);
        with(p_d4 + r, (int32_t)-1);
        with(p_d4 + r, (int32_t)(1 << 20) + 1);
        with(p_m2 + r, (int32_t)(1 << 17) + 1);
        with(p_lvl + rnd(0, n_kmers - 1), (int32_t)(1 << 14));
        with(p_bias + rnd(0, n_kmers - 1), (int32_t)257);
        if (nb) with(p_codes + rnd(0, (int64_t)nb - 1), (uint8_t)4);
        if (ref_len[r] >= 2) {                                                   // a guide that decreases inside a read
            const int64_t b = ref_off[r] + rnd(1, ref_len[r] - 1);
            with(p_g + b, (int32_t)(p_g[b - 1] - 1));
        }
        for (void* p : {(void*)p_raw, (void*)p_off, (void*)p_lo, (void*)p_hi, (void*)p_ro, (void*)p_rl, (void*)p_m2, (void*)p_d4, (void*)p_g, (void*)p_lvl,
                        (void*)p_bias, (void*)p_w, (void*)p_codes, (void*)status, (void*)o_m2, (void*)o_d4, (void*)nedge, (void*)first, (void*)last,
                        (void*)start, (void*)end, (void*)score, (void*)sum, (void*)sumsq, (void*)sums, (void*)mn, (void*)mx})
            free(p);
    }
    CHECK(rd_eventalign_banded_workspace_bytes(-1, 0) == -1 && rd_eventalign_banded_workspace_bytes(1, 0) == 256 + 256 + 256 + 1792);
    CHECK(rd_eventalign_banded_workspace_bytes(120000, 4000) == 480000 + 960000 + 480000 + 49664);   // each a multiple of 256 but the last: 12 * 4130 = 49560
    printf("no sanitizer report\n%ld accepted %ld refused\n", g_accepted, g_refused);
    return 0;
}
