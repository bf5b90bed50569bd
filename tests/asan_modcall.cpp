// TEST INFRASTRUCTURE: AddressSanitizer + UBSan harness for the host side of rd_modcall (radian_amd/csrc/modcall.hip: the argument checks,
// the rules of modcall_rules.h, the plain loop of rd_modcall_host; sanitizers run on the CPU build only -- the kernel is not compiled here).
// usage: asan_modcall <iterations>   The rules at their limits first.  Every iteration draws a few reads with steps (bases without rows,
// steps that leave too few rows, steps past the read's end among them), a model and jobs in any order into EXACT-SIZE heap buffers (a read
// or a write past either end is an ASan report), calls the host twin and checks every field against a whole-table loop of its own written
// from the contract's text in 64 bits, its table from libm; then the same buffers go through the refusals, which must answer RD_ERR_ARG
// and write nothing.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../radian_amd/csrc/modcall.hip"   // the host half (this is no HIP build)

void rd_set_error(const char* fmt, ...) { (void)fmt; }

static long g_accepted = 0, g_refused = 0, g_jobs = 0;

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

static int64_t own_lse(int64_t d) { return (int64_t)std::floor(32.0 * std::log1p(std::exp(-(double)d / 32.0)) + 0.5); }

static void rules_at_their_limits()
{
    CHECK(MC_LSE_N == 134 && sizeof(MC_LSE) == 134 && MC_LSE[0] == 22 && MC_LSE[132] == 1 && MC_LSE[133] == 0);
    for (int d = 0; d < MC_LSE_N; d++) CHECK(MC_LSE[d] == own_lse(d));
    CHECK(mc_lse_index(0, 0) == 0 && mc_lse_index(5, -127) == 132 && mc_lse_index(-127, 6) == 133 && mc_lse_index(EA_INF, -(1 << 23)) == 133);
    CHECK(mc_lse_index(INT32_MAX, -(1 << 15) * 278) == 133 && mc_lse_index(-(1 << 15) * 278, INT32_MAX) == 133);
    CHECK(mc_vit(7, 3, 2) == 9 && mc_vit(7, 2, 2) == 9 && mc_fwd(7, 2, 2, MC_LSE) == 9 - 22 && mc_fwd(-256, 100, 100 + 133, MC_LSE) == -156);
    CHECK(mc_fwd(1280, EA_INF, 5, MC_LSE) == 1285 && mc_fwd(0, 40, 8, MC_LSE) == 8 - 10);
    CHECK(mc_flank_ok(0) && mc_flank_ok(27) && !mc_flank_ok(28) && !mc_flank_ok(-1));
    CHECK(mc_job_ok(0, 1, 1) && mc_job_ok(3, 9, 12) && !mc_job_ok(3, 10, 20) && !mc_job_ok(3, 0, 20) && !mc_job_ok(-1, 1, 20) && !mc_job_ok(4, 9, 12));
    const int32_t first[4] = {10, -1, 30, 40}, last[4] = {19, -1, 39, 40 + (1 << 15) - 1};
    McWindow w = mc_window(first, last, 4, 100000, 0, 1, 0);
    CHECK(w.status == MC_OK && w.a0 == 0 && w.S == 1 && w.r0 == 10 && w.R == 10);
    CHECK(mc_window(first, last, 4, 100000, 1, 1, 0).status == MC_NO_ANCHOR && mc_window(first, last, 4, 100000, 0, 1, 1).status == MC_NO_ANCHOR);
    w = mc_window(first, last, 4, 100000, 2, 1, 27);
    CHECK(w.status == MC_TOO_LONG && w.a0 == 0 && w.S == 4);
    w = mc_window(first, last, 4, 100000, 3, 1, 0);
    CHECK(w.status == MC_OK && w.R == 1 << 15);
    CHECK(mc_window(first, last, 4, 40 + (1 << 15) - 1, 3, 1, 0).status == MC_NO_PATH);   // the last row is the read's n-th sample
    CHECK(mc_window(first, last, 4, 100000, 3, 1, 1).status == MC_TOO_LONG);
}

struct Read {
    std::vector<int16_t> x;
    std::vector<uint8_t> codes;
    std::vector<int32_t> first, last;
    int32_t m2, d4;
};
struct Job {
    int read, alt_first;
    std::vector<int32_t> lvl, bias;
    std::vector<uint32_t> w;
};
struct Want {
    int32_t status = 0, R = 0, S = 0;
    int64_t v[4] = {0, 0, 0, 0};   // vit_ref, vit_alt, fwd_ref, fwd_alt
};

// the contract over one job, the whole R x S table of each of the four values kept, in 64 bits
static Want own_job(const Read& rd, const Job& jb, int F, int k, const std::vector<int32_t>& lvl, const std::vector<uint32_t>& w, const std::vector<int32_t>& bias)
{
    const int64_t L = (int64_t)rd.codes.size(), n_alt = (int64_t)jb.lvl.size(), INF = (int64_t)1 << 30;
    const int64_t a0 = std::max<int64_t>(0, jb.alt_first - F), a1 = std::min<int64_t>(L - 1, jb.alt_first + n_alt - 1 + F), S = a1 - a0 + 1;
    Want o;
    const int64_t r0 = rd.first[a0], r1 = rd.last[a1], R = r1 - r0 + 1;
    if (r0 == -1 || r1 == -1) return o.status = 1, o;
    if (R < S || r0 < 0 || r1 >= (int64_t)rd.x.size()) return o.status = 2, o;
    if (R > (1 << 15)) return o.status = 3, o;
    std::vector<int64_t> sl[2], sw[2], sb[2];
    for (int h = 0; h < 2; h++) sl[h].resize(S), sw[h].resize(S), sb[h].resize(S);
    for (int64_t i = 0; i < S; i++) {
        int64_t idx = 0;
        for (int j = -(k / 2); j <= k / 2; j++) idx = idx * 4 + rd.codes[std::min<int64_t>(std::max<int64_t>(a0 + i + j, 0), L - 1)];
        const int64_t a = a0 + i - jb.alt_first;
        const bool rep = a >= 0 && a < n_alt;
        sl[0][i] = lvl[idx], sw[0][i] = w[idx], sb[0][i] = bias[idx];
        sl[1][i] = rep ? jb.lvl[a] : lvl[idx], sw[1][i] = rep ? jb.w[a] : w[idx], sb[1][i] = rep ? jb.bias[a] : bias[idx];
    }
    std::vector<int64_t> V[4];
    for (auto& t : V) t.assign((size_t)(R * S), INF);
    for (int64_t t = 0; t < R; t++) {
        const int64_t u = 512 * (2 * (int64_t)rd.x[r0 + t] - rd.m2), num = 2 * u + rd.d4, den = 2 * (int64_t)rd.d4;
        int64_t q = num / den;
        if (num % den < 0) q--;
        const int64_t z = std::max<int64_t>(-(1 << 14), std::min<int64_t>(1 << 14, q));
        for (int64_t i = 0; i < S; i++)
            for (int h = 0; h < 2; h++) {
                const int64_t d = z - sl[h][i], c = std::min<int64_t>((int64_t)(((unsigned __int128)(d * d) * (uint64_t)sw[h][i]) >> 32), 1024) + sb[h][i];
                if (t == 0) {
                    if (i == 0) V[h][0] = V[2 + h][0] = c;
                    continue;
                }
                for (int f = 0; f < 2; f++) {
                    const std::vector<int64_t>& T = V[2 * f + h];
                    const int64_t stay = T[(t - 1) * S + i], adv = i ? T[(t - 1) * S + i - 1] : INF;
                    V[2 * f + h][t * S + i] = c + std::min(stay, adv) - (f ? own_lse(std::min<int64_t>(std::llabs(stay - adv), 133)) : 0);
                }
            }
    }
    o.R = (int32_t)R, o.S = (int32_t)S;
    for (int f = 0; f < 4; f++) o.v[f] = V[f][R * S - 1];
    return o;
}

int main(int argc, char** argv)
{
    const long iters = argc > 1 ? atol(argv[1]) : 100;
    rules_at_their_limits();
    std::mt19937_64 gen(20311);
    const auto rnd = [&](int64_t lo, int64_t hi) { return (int64_t)(gen() % (uint64_t)(hi - lo + 1)) + lo; };
    for (long it = 0; it < iters; it++) {
        const int k = (int)(2 * rnd(0, 2) + 1), n_kmers = 1 << (2 * k), n_reads = (int)rnd(1, 4), F = (int)(rnd(0, 3) ? rnd(0, 8) : rnd(20, 27));
        std::vector<int32_t> lvl(n_kmers), bias(n_kmers);
        std::vector<uint32_t> w(n_kmers);
        for (int i = 0; i < n_kmers; i++) {
            lvl[i] = (int32_t)rnd(-1600, 1600), bias[i] = (int32_t)rnd(-256, 256);
            w[i] = rnd(0, 9) == 0 ? (rnd(0, 1) ? 0u : 0xffffffffu) : (uint32_t)rnd(1 << 18, 1 << 30);
        }
        lvl[0] = -(1 << 14) + 1, lvl[n_kmers - 1] = (1 << 14) - 1;
        std::vector<Read> reads(n_reads);
        std::vector<int16_t> raw;
        std::vector<int64_t> read_off{0}, ref_off;
        std::vector<int32_t> ref_len, m2, d4, first, last;
        std::vector<uint8_t> codes;
        for (Read& rd : reads) {
            const int64_t L = rnd(0, 5) ? rnd(1, 70) : 0, lead = rnd(0, 20);
            int64_t t = lead;
            for (int64_t b = 0; b < L; b++) {
                rd.codes.push_back((uint8_t)rnd(0, 3));
                const int64_t n = rnd(0, 9) == 0 ? 0 : rnd(0, 5) == 0 ? 1 : rnd(1, 12);   // (0: a base without rows)
                rd.first.push_back(n ? (int32_t)t : -1), rd.last.push_back(n ? (int32_t)(t + n - 1) : -1);
                t += n;
            }
            const int kind = (int)rnd(0, 9);
            const int64_t T = kind == 0 && t > 3 ? t - 3 : t + rnd(0, 20);   // (kind 0: the last steps lie past the read's end)
            if (kind == 1 && L) rd.last[rnd(0, L - 1)] = (int32_t)rnd(-1, 30);   // a step that leaves too few rows, or none
            if (kind == 2 && L) rd.first[rnd(0, L - 1)] = (int32_t)rnd(-9, -2);
            for (int64_t i = 0; i < T; i++) rd.x.push_back((int16_t)(rnd(0, 30) == 0 ? (rnd(0, 1) ? 32767 : -32768) : rnd(200, 1000)));
            rd.m2 = (int32_t)rnd(1100, 1300), rd.d4 = (int32_t)(rnd(0, 9) == 0 ? rnd(1, 20) : rnd(200, 300));
            raw.insert(raw.end(), rd.x.begin(), rd.x.end());
            read_off.push_back((int64_t)raw.size()), m2.push_back(rd.m2), d4.push_back(rd.d4);
            ref_off.push_back((int64_t)codes.size()), ref_len.push_back((int32_t)L);
            codes.insert(codes.end(), rd.codes.begin(), rd.codes.end());
            first.insert(first.end(), rd.first.begin(), rd.first.end()), last.insert(last.end(), rd.last.begin(), rd.last.end());
        }
        std::vector<Job> jobs;
        for (int r = 0; r < n_reads; r++) {
            const int64_t L = ref_len[r];
            for (int64_t j = L ? rnd(0, 6) : 0; j > 0; j--) {
                Job jb;
                const int64_t n_alt = std::min<int64_t>(L, rnd(0, 2) ? 1 : rnd(1, 9));
                jb.read = r, jb.alt_first = (int)rnd(0, L - n_alt);
                for (int64_t a = 0; a < n_alt; a++)
                    jb.lvl.push_back((int32_t)rnd(-1700, 1700)), jb.bias.push_back((int32_t)rnd(-256, 256)), jb.w.push_back((uint32_t)rnd(0, 1 << 30));
                jobs.push_back(jb);
            }
        }
        std::shuffle(jobs.begin(), jobs.end(), gen);
        const int n_jobs = (int)jobs.size();
        std::vector<int32_t> job_read, alt_first, a_lvl, a_bias;
        std::vector<uint32_t> a_w;
        std::vector<int64_t> alt_off{0};
        for (const Job& jb : jobs) {
            job_read.push_back(jb.read), alt_first.push_back(jb.alt_first);
            a_lvl.insert(a_lvl.end(), jb.lvl.begin(), jb.lvl.end()), a_bias.insert(a_bias.end(), jb.bias.begin(), jb.bias.end());
            a_w.insert(a_w.end(), jb.w.begin(), jb.w.end());
            alt_off.push_back((int64_t)a_lvl.size());
        }
        int16_t* p_raw = exact(raw);
        int64_t *p_off = exact(read_off), *p_ro = exact(ref_off), *p_ao = exact(alt_off);
        int32_t *p_rl = exact(ref_len), *p_m2 = exact(m2), *p_d4 = exact(d4), *p_first = exact(first), *p_last = exact(last), *p_lvl = exact(lvl),
                *p_bias = exact(bias), *p_jr = exact(job_read), *p_af = exact(alt_first), *p_al = exact(a_lvl), *p_ab = exact(a_bias);
        uint32_t *p_w = exact(w), *p_aw = exact(a_w);
        uint8_t* p_codes = exact(codes);
        const std::vector<int32_t> fill(n_jobs, 77);
        int32_t* out[7];
        for (auto& p : out) p = exact(fill);
        const auto call = [&](int n, int nj, int kk, int flank) {
            return rd_modcall_host(p_raw, p_off, n, p_m2, p_d4, p_codes, p_ro, p_rl, p_first, p_last, kk, p_lvl, p_w, p_bias, nj, p_jr, p_af, p_ao, p_al, p_aw,
                                   p_ab, flank, out[0], out[1], out[2], out[3], out[4], out[5], out[6]);
        };
        CHECK(call(n_reads, n_jobs, k, F) == RD_OK);
        g_accepted++;
        for (int j = 0; j < n_jobs; j++) {
            const Want o = own_job(reads[jobs[j].read], jobs[j], F, k, lvl, w, bias);
            CHECK(out[0][j] == o.status && out[1][j] == o.R && out[2][j] == o.S);
            for (int f = 0; f < 4; f++) CHECK(out[3 + f][j] == o.v[f]);
            g_jobs++;
        }
        // the refusals: RD_ERR_ARG, and nothing is written
        for (auto& p : out)
            for (int j = 0; j < n_jobs; j++) p[j] = 77;
        const auto refused = [&](int rc) {
            CHECK(rc == RD_ERR_ARG);
            for (auto& p : out)
                for (int j = 0; j < n_jobs; j++) CHECK(p[j] == 77);
            g_refused++;
        };
        refused(call(-1, n_jobs, k, F));
        refused(call(n_reads, -1, k, F));
        refused(call(n_reads, n_jobs, 2, F));
        refused(call(n_reads, n_jobs, 11, F));
        refused(call(n_reads, n_jobs, k, -1));
        refused(call(n_reads, n_jobs, k, 28));
        const int r = (int)rnd(0, n_reads - 1);
        const auto with = [&](auto* p, auto v) {
            const auto keep = *p;
            *p = v;
            refused(call(n_reads, n_jobs, k, F));
            *p = keep;
        };
        with(p_rl + r, (int32_t)-1);
        with(p_d4 + r, (int32_t)0);
        with(p_d4 + r, (int32_t)(1 << 20) + 1);
        with(p_m2 + r, (int32_t)-(1 << 17) - 1);
        with(p_off + r + 1, p_off[r] - 1);
        with(p_lvl + rnd(0, n_kmers - 1), (int32_t)(1 << 14));
        with(p_bias + rnd(0, n_kmers - 1), (int32_t)-257);
        if (!codes.empty()) with(p_codes + rnd(0, (int64_t)codes.size() - 1), (uint8_t)4);
        if (n_jobs) {
            const int j = (int)rnd(0, n_jobs - 1);
            with(p_jr + j, (int32_t)n_reads);
            with(p_jr + j, (int32_t)-1);
            with(p_af + j, (int32_t)-1);
            with(p_af + j, (int32_t)(ref_len[job_read[j]] - (alt_off[j + 1] - alt_off[j]) + 1));
            with(p_al + alt_off[j], (int32_t)-(1 << 14));
            with(p_ab + alt_off[j], (int32_t)257);
            if (j + 1 < n_jobs) with(p_ao + j + 1, alt_off[j]);           // a job without entries
            if (j + 1 < n_jobs && alt_off[j + 2] - alt_off[j] >= 10) with(p_ao + j + 1, alt_off[j] + 10);   // a job of ten
        }
        for (void* p : {(void*)p_raw, (void*)p_off, (void*)p_ro, (void*)p_ao, (void*)p_rl, (void*)p_m2, (void*)p_d4, (void*)p_first, (void*)p_last, (void*)p_lvl,
                        (void*)p_bias, (void*)p_jr, (void*)p_af, (void*)p_al, (void*)p_ab, (void*)p_w, (void*)p_aw, (void*)p_codes})
            free(p);
        for (auto& p : out) free(p);
    }
    CHECK(rd_modcall_workspace_bytes(-1, 0, 0, 0) == -1 && rd_modcall_workspace_bytes(1, 1, 1, 1) == 5 * 256);
    CHECK(rd_modcall_workspace_bytes(1000, 30, 5, 45) == 2048 + 256 + 512 + 256 + 768);
    printf("no sanitizer report\n%ld accepted %ld refused %ld jobs\n", g_accepted, g_refused, g_jobs);
    return 0;
}
