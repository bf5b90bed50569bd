// TEST INFRASTRUCTURE: AddressSanitizer + UBSan harness for the host side of radian_amd/csrc/sim.hip (the argument check, the rules of
// sim_rules.h, the plain loops of rd_sim_lengths_host / rd_sim_signal_host) and the budget cut rd_sim_signal uses (budget.h; sanitizers run
// on the CPU build only -- the kernels are not compiled here).
// usage: asan_sim <iterations>   Philox's three known answers first.  Every iteration draws a model (k 1, 3 or 5) and a batch of reads (0, 1,
// k / 2 and more bases; leads from 0; the parameters' extremes) into EXACT-SIZE heap buffers (a read or a write past either end is an ASan
// report), calls the two host entry points and checks every output against its invariants and a loop of its own over the rules; cuts the
// batch under a random budget and checks the plan; then the same buffers go through the refusals, which must answer RD_ERR_ARG and write nothing.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../radian_amd/csrc/budget.h"
#include "../radian_amd/csrc/sim.hip"   // the host half (this is no HIP build): the device blocks' layout functions live in its unnamed namespace

extern "C" int rd_sim_lengths_host(const uint8_t* codes, const int64_t* seq_off, int n_reads, const int16_t* level_shift_q10,
                                   const uint16_t* dwell_scale_q8, const int32_t* lead, const int32_t* lead_level_q10, const int32_t* lead_sd_q10,
                                   const int32_t* median, const int32_t* scale_q10, const uint32_t* key, int k, const int32_t* level_q10,
                                   const int32_t* sd_q10, const int32_t* dwell_q8, const uint32_t* dwell_cdf, int64_t* n_samples);
extern "C" int rd_sim_signal_host(const uint8_t* codes, const int64_t* seq_off, int n_reads, const int16_t* level_shift_q10,
                                  const uint16_t* dwell_scale_q8, const int32_t* lead, const int32_t* lead_level_q10, const int32_t* lead_sd_q10,
                                  const int32_t* median, const int32_t* scale_q10, const uint32_t* key, int k, const int32_t* level_q10,
                                  const int32_t* sd_q10, const int32_t* dwell_q8, const uint32_t* dwell_cdf, const int64_t* raw_off, int16_t* raw,
                                  int32_t* base_first, int32_t* status);
extern "C" int64_t rd_sim_workspace_bytes(int64_t n_bases, int64_t n_samples);
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

// a call's inputs, each in a heap block of its exact size
struct In {
    uint8_t* codes;
    int64_t *seq_off, *raw_off;
    int n;
    int16_t* shift;
    uint16_t* dscale;
    int32_t *lead, *lead_level, *lead_sd, *median, *scale;
    uint32_t* key;
    int k;
    int32_t *level, *sd, *dwell;
    uint32_t* cdf;
};

static int lengths(const In& a, int64_t* ns)
{
    return rd_sim_lengths_host(a.codes, a.seq_off, a.n, a.shift, a.dscale, a.lead, a.lead_level, a.lead_sd, a.median, a.scale, a.key, a.k, a.level,
                               a.sd, a.dwell, a.cdf, ns);
}
static int signal(const In& a, int16_t* raw, int32_t* bf, int32_t* st)
{
    return rd_sim_signal_host(a.codes, a.seq_off, a.n, a.shift, a.dscale, a.lead, a.lead_level, a.lead_sd, a.median, a.scale, a.key, a.k, a.level,
                              a.sd, a.dwell, a.cdf, a.raw_off, raw, bf, st);
}

// The yardstick of sim_layout: the take lambda and the block list that sim_carve held before the layout function replaced them, written
// out literally; on seeded random dimensions (0 and 1 of each among them) the total and every block's offset must be equal, dry and wet.
static void check_layout()
{
    std::mt19937_64 rng(7);
    const size_t dims[] = {0, 1, 2, 31, 32, 33, 255, 256, 257};
    auto dim = [&](size_t big) { return rng() % 3 ? dims[rng() % 9] : (size_t)(rng() % big); };
    char* const base = (char*)((uintptr_t)1 << 32);
    for (int it = 0; it < 4000; it++) {
        const int k = 1 + (int)(rng() % 9), n = (int)dim(4000);
        const int64_t B = (int64_t)dim(2000000), R = (int64_t)dim(20000000);
        const bool with_shift = rng() % 2, with_dscale = rng() % 2;
        const size_t tb = dim(200000);
        for (int wet = 0; wet < 2; wet++) {
            char* const b = wet ? base : nullptr;
            SimWs old;
            size_t at = sim_model_bytes(k);
            const auto take = [&](size_t bytes) {
                char* p = b ? b + at : nullptr;
                at += align_up(bytes + 8, 256);
                return p;
            };
            old.reads = (SimRead*)take((size_t)n * sizeof(SimRead));
            old.cum = (int64_t*)take((size_t)(B + 1) * 8);
            old.len = (int64_t*)take((size_t)n * 8);
            old.lvsd = (int2*)take((size_t)B * 8);
            old.dwell = (int32_t*)take((size_t)(B + 1) * 4);
            old.bfirst = (int32_t*)take((size_t)B * 4);
            old.raw = (int16_t*)take((size_t)R * 2);
            old.shift = (int16_t*)take(with_shift ? (size_t)B * 2 : 0);
            old.dscale = (uint16_t*)take(with_dscale ? (size_t)B * 2 : 0);
            old.codes = (uint8_t*)take((size_t)B);
            old.tmp = take(tb);
            old.total = at;
            SimWs W;
            Carve c(b);
            sim_layout(c, k, n, B, R, with_shift, with_dscale, tb, &W);
            CHECK(W.total == old.total && c.at == old.total && W.tmp_bytes == tb);
            CHECK(W.reads == old.reads && W.cum == old.cum && W.len == old.len && W.lvsd == old.lvsd && W.dwell == old.dwell && W.bfirst == old.bfirst &&
                  W.raw == old.raw && W.shift == old.shift && W.dscale == old.dscale && W.codes == old.codes && W.tmp == old.tmp);
            CHECK(wet ? (char*)W.reads == base + sim_model_bytes(k) : W.reads == nullptr);
        }
    }
}

int main(int argc, char** argv)
{
    const long iters = argc > 1 ? atol(argv[1]) : 20;
    check_layout();
    // Philox4x32-10: the known answers
    {
        uint32_t w[4];
        sim_philox(0, 0, 0, 0, 0, 0, w);
        CHECK(w[0] == 0x6627e8d5u && w[1] == 0xe169c58du && w[2] == 0xbc57ac4cu && w[3] == 0x9b00dbd8u);
        sim_philox(~0u, ~0u, ~0u, ~0u, ~0u, ~0u, w);
        CHECK(w[0] == 0x408f276du && w[1] == 0x41c83b0eu && w[2] == 0xa20bc7c6u && w[3] == 0x6d5451fdu);
        sim_philox(0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u, w);
        CHECK(w[0] == 0xd16cfe09u && w[1] == 0x94fdccebu && w[2] == 0x5001e420u && w[3] == 0x24126ea1u);
        // the rules at their limits
        const uint32_t all[4] = {~0u, ~0u, ~0u, ~0u}, none[4] = {0, 0, 0, 0};
        CHECK(sim_noise_z(all) == 6138 && sim_noise_z(none) == -6138);
        CHECK(sim_raw(1 << 16, 1 << 15, 6138, 32767, 1 << 26) == 32767 && sim_raw(-(1 << 16), 1 << 15, -6138, -32768, 1 << 26) == -32768);
        CHECK(sim_raw(-1, 0, 0, 0, 1 << 20) == -1 && sim_raw(0, 1, -1, 0, 1 << 20) == -1 && sim_raw(1, 0, 0, 5, 1 << 19) == 6);
        std::vector<uint32_t> top(1024, 1u << 20), one(1024, 65536);
        CHECK(sim_dwell(1 << 23, 4096, top.data(), ~0u) == 32767 && sim_dwell(256, 1, top.data(), 0) == 1 && sim_dwell(256, 256, one.data(), 7) == 1);
        CHECK(sim_dwell(30 * 256, 256, one.data(), 0) == 30 && sim_dwell(30 * 256, 512, one.data(), 0) == 60);
        const uint8_t c[5] = {1, 2, 3, 0, 2};
        CHECK(sim_kmer(c, 5, 0, 3) == (1 * 16 + 1 * 4 + 2) && sim_kmer(c, 5, 4, 3) == (0 * 16 + 2 * 4 + 2) && sim_kmer(c, 5, 2, 5) == 0x1B2 >> 0);
        CHECK(sim_kmer(c, 1, 0, 9) == 0x15555 && sim_kmer(c, 5, 1, 1) == 2);
        CHECK(!sim_k_ok(0) && !sim_k_ok(2) && sim_k_ok(9) && !sim_k_ok(11));
    }
    std::mt19937_64 rng(12345);
    auto uni = [&](int64_t lo, int64_t hi) { return (int64_t)(lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1))); };
    for (long it = 0; it < iters; it++) {
        const int k = 1 + 2 * (int)uni(0, 2), nk = 1 << (2 * k), n = (int)uni(1, 6);
        std::vector<int32_t> level(nk), sd(nk), dwell(nk);
        for (int i = 0; i < nk; i++) level[i] = (int32_t)uni(-(1 << 15), 1 << 15), sd[i] = (int32_t)uni(0, 1 << 15), dwell[i] = (int32_t)uni(256, 40 * 256);
        level[0] = 1 << 15, sd[0] = 1 << 15, dwell[nk - 1] = 1 << 23;
        std::vector<uint32_t> cdf(1024);
        for (int i = 0; i < 1024; i++) cdf[i] = (uint32_t)(13000 + 300 * i);
        if (it % 3 == 0) cdf[1023] = 1u << 20;
        std::vector<int64_t> seq_off(1, 0);
        std::vector<int32_t> lead, lead_level, lead_sd, median, scale;
        std::vector<uint32_t> key;
        for (int r = 0; r < n; r++) {
            const int64_t choices[6] = {0, 1, k / 2, k / 2 + 1, uni(2, 40), uni(40, 300)};
            seq_off.push_back(seq_off.back() + choices[uni(0, 5)]);
            lead.push_back((int32_t)(uni(0, 3) ? uni(0, 500) : 0));
            lead_level.push_back((int32_t)uni(-(1 << 15), 1 << 15));
            lead_sd.push_back((int32_t)uni(0, 1 << 15));
            median.push_back((int32_t)uni(-32768, 32767));
            scale.push_back((int32_t)(uni(0, 4) ? uni(1, 200000) : (1 << 26)));
            key.push_back((uint32_t)rng()), key.push_back((uint32_t)rng());
        }
        const int64_t B = seq_off.back();
        std::vector<uint8_t> codes(B);
        std::vector<int16_t> shift(B);
        std::vector<uint16_t> dscale(B);
        for (int64_t i = 0; i < B; i++) codes[i] = (uint8_t)uni(0, 3), shift[i] = (int16_t)uni(-32768, 32767), dscale[i] = (uint16_t)(uni(0, 9) ? uni(1, 600) : 4096);
        const bool with_opt = it % 2 == 0;
        In a{exact(codes), exact(seq_off), nullptr, n, with_opt ? exact(shift) : nullptr, with_opt ? exact(dscale) : nullptr, exact(lead),
             exact(lead_level), exact(lead_sd), exact(median), exact(scale), exact(key), k, exact(level), exact(sd), exact(dwell), exact(cdf)};
        std::vector<int64_t> ns_v(n);
        int64_t* ns = exact(ns_v);
        CHECK(lengths(a, ns) == 0);
        std::vector<int64_t> raw_off(1, 0);
        for (int r = 0; r < n; r++) {
            CHECK(ns[r] >= lead[r] + (seq_off[r + 1] - seq_off[r]) && ns[r] <= lead[r] + 32767 * (seq_off[r + 1] - seq_off[r]));
            raw_off.push_back(raw_off.back() + ns[r]);
        }
        a.raw_off = exact(raw_off);
        const int64_t R = raw_off.back();
        int16_t* raw = (int16_t*)malloc(R ? R * 2 : 1);
        int32_t* bf = (int32_t*)malloc(B ? B * 4 : 1);
        int32_t* st = (int32_t*)malloc(n * 4);
        CHECK(signal(a, raw, bf, st) == 0);
        g_accepted++;
        for (int r = 0; r < n; r++) {   // a loop of its own over the rules
            const int64_t s0 = seq_off[r];
            const int32_t L = (int32_t)(seq_off[r + 1] - s0);
            CHECK(st[r] == (ns[r] ? SIM_OK : SIM_EMPTY));
            int64_t at = lead[r];
            for (int32_t b = 0; b < L; b++) {
                CHECK(bf[s0 + b] == at);
                uint32_t w[4];
                sim_philox((uint32_t)b, 0, 0, 0, key[2 * r], key[2 * r + 1], w);
                at += sim_dwell(dwell[sim_kmer(codes.data() + s0, L, b, k)], with_opt ? dscale[s0 + b] : 256u, cdf.data(), w[0]);
            }
            CHECK(at == ns[r]);
            for (int64_t s = 0; s < ns[r]; s += 1 + (s % 7)) {   // spot checks of the samples
                int32_t b = -1;
                while (b + 1 < L && bf[s0 + b + 1] <= s) b++;
                int32_t lv = lead_level[r], sv = lead_sd[r];
                if (b >= 0) {
                    const int32_t idx = sim_kmer(codes.data() + s0, L, b, k);
                    lv = level[idx] + (with_opt ? shift[s0 + b] : 0), sv = sd[idx];
                }
                uint32_t w[4];
                sim_philox((uint32_t)s, 1, 0, 0, key[2 * r], key[2 * r + 1], w);
                CHECK(raw[raw_off[r] + s] == sim_raw(lv, sv, sim_noise_z(w), median[r], scale[r]));
            }
        }
        // null base_first is allowed
        CHECK(signal(a, raw, nullptr, st) == 0);
        // the budget cut rd_sim_signal makes: every read in one launch or too large, launches within the budget, order kept
        {
            const int64_t overhead = 4096, budget = overhead + uni(0, 3) * 20000 + uni(0, 50000);
            const BudgetPlan P = rd_plan_budget(n, nullptr, budget, overhead, false,
                                                [&](int r, int) { return rd_sim_workspace_bytes(seq_off[r + 1] - seq_off[r], ns[r]); },
                                                rd_budget_never_closes);
            CHECK((int64_t)P.run.size() + P.too_large == n);
            for (auto [k0, k1] : P.launches) {
                int64_t sum = overhead;
                for (int64_t i = k0; i < k1; i++) {
                    sum += rd_sim_workspace_bytes(seq_off[P.run[i] + 1] - seq_off[P.run[i]], ns[P.run[i]]);
                    CHECK(i == k0 || P.run[i] > P.run[i - 1]);
                }
                CHECK(k1 > k0 && sum <= budget);
            }
            CHECK(P.max_bytes <= budget);
        }
        // the refusals: RD_ERR_ARG, nothing written
        auto refused = [&](const In& bad) {
            memset(raw, 0x4d, R * 2);
            memset(bf, 0x4d, B * 4);
            memset(st, 0x4d, n * 4);
            CHECK(signal(bad, raw, bf, st) == -1);
            for (int64_t i = 0; i < R * 2; i++) CHECK(((unsigned char*)raw)[i] == 0x4d);
            for (int64_t i = 0; i < B * 4; i++) CHECK(((unsigned char*)bf)[i] == 0x4d);
            for (int64_t i = 0; i < n * 4; i++) CHECK(((unsigned char*)st)[i] == 0x4d);
            g_refused++;
        };
        {
            In b = a; b.k = 2; refused(b);
            b = a; b.k = 11; refused(b);
            b = a; b.n = -1; refused(b);
            b = a; b.cdf = nullptr; refused(b);
            b = a; b.level = nullptr; refused(b);
            b = a; b.key = nullptr; refused(b);
            b = a; b.raw_off = nullptr; refused(b);
            b = a; b.seq_off = nullptr; refused(b);
            const auto with = [&](auto* In::*field, auto& vec, size_t i, auto v) {   // one entry of one array changed, in an exact-size copy
                auto copy = vec;
                copy[i] = v;
                In c = a;
                auto* p = exact(copy);
                c.*field = p;
                refused(c);
                free(p);
            };
            with(&In::cdf, cdf, 512, 0u);
            with(&In::cdf, cdf, 0, (1u << 20) + 1);
            with(&In::level, level, nk - 1, (int32_t)((1 << 15) + 1));
            with(&In::sd, sd, 0, (int32_t)-1);
            with(&In::dwell, dwell, 0, (int32_t)255);
            with(&In::dwell, dwell, nk - 1, (int32_t)((1 << 23) + 1));
            with(&In::lead, lead, 0, (int32_t)-1);
            with(&In::lead_level, lead_level, n - 1, (int32_t)(-(1 << 15) - 1));
            with(&In::lead_sd, lead_sd, 0, (int32_t)((1 << 15) + 1));
            with(&In::median, median, 0, (int32_t)-32769);
            with(&In::scale, scale, n - 1, (int32_t)0);
            with(&In::scale, scale, 0, (int32_t)((1 << 26) + 1));
            with(&In::seq_off, seq_off, 0, (int64_t)-1);
            with(&In::raw_off, raw_off, n, raw_off[n] + 1);
            with(&In::raw_off, raw_off, 0, (int64_t)-1);
            if (B) {
                with(&In::codes, codes, (size_t)(B - 1), (uint8_t)4);
                if (with_opt) with(&In::dscale, dscale, 0, (uint16_t)0);
                if (with_opt) with(&In::dscale, dscale, (size_t)(B - 1), (uint16_t)4097);
            }
            if (n > 1 && B) with(&In::seq_off, seq_off, (size_t)n, (int64_t)0);
        }
        free(raw), free(bf), free(st), free(ns);
        free(a.codes), free(a.seq_off), free(a.raw_off), free(a.shift), free(a.dscale), free(a.lead), free(a.lead_level), free(a.lead_sd),
            free(a.median), free(a.scale), free(a.key), free(a.level), free(a.sd), free(a.dwell), free(a.cdf);
    }
    printf("no sanitizer report\n%ld accepted %ld refused\n", g_accepted, g_refused);
    return 0;
}
