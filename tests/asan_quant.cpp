// TEST INFRASTRUCTURE: AddressSanitizer + UBSan harness for the host side of radian_amd/csrc/quant.hip (the argument check, the rules of
// quant_rules.h, the packer, the plain loops of rd_quant_em_host; sanitizers run on the CPU build only -- the kernels are not compiled here).
// usage: asan_quant <iterations>   The rules at their limits first.  Every iteration draws reads (0, 1, 2 .. 64 candidates, weights 1 and
// 4096 among them, runs of single reads large enough for the shift) into EXACT-SIZE heap buffers (a read or a write past either end is an
// ASan report), packs them and checks the packed form, calls the host twin and checks every output against a loop of its own over the
// rules on the unpacked reads; then the same buffers go through the refusals, which must answer RD_ERR_ARG and write nothing.
#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../radian_amd/csrc/quant_rules.h"

extern "C" int rd_quant_em_host(const int64_t* cand_off, const int32_t* cand_t, const uint16_t* cand_w, int64_t n_reads, int64_t n_tx, int max_iter,
                                uint64_t tol_q20, uint64_t* count_q20, uint32_t* share_q20, int64_t* stats);
extern "C" int64_t rd_quant_workspace_bytes(int64_t slots, int64_t n_reads, int64_t n_tx);
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

// one step of the contract over the unpacked reads
static void own_step(const std::vector<int64_t>& off, const std::vector<int32_t>& t, const std::vector<uint16_t>& w, const std::vector<uint64_t>& c,
                     std::vector<uint64_t>& cn, std::vector<uint32_t>& share)
{
    std::fill(cn.begin(), cn.end(), 0);
    for (size_t r = 0; r + 1 < off.size(); r++) {
        if (off[r + 1] == off[r]) continue;
        uint64_t S = 0, Sp = 0;
        for (int64_t i = off[r]; i < off[r + 1]; i++) S += c[t[i]] * w[i];
        const int sh = quant_shift(S);
        for (int64_t i = off[r]; i < off[r + 1]; i++) Sp += (c[t[i]] * w[i]) >> sh;
        CHECK(Sp > 0);
        for (int64_t i = off[r]; i < off[r + 1]; i++) {
            share[i] = (uint32_t)quant_share((c[t[i]] * w[i]) >> sh, Sp);
            cn[t[i]] += share[i];
        }
    }
}

int main(int argc, char** argv)
{
    const long iters = argc > 1 ? atol(argv[1]) : 20;
    // the rules at their limits
    CHECK(quant_bitlen(0) == 0 && quant_bitlen(1) == 1 && quant_bitlen(~(uint64_t)0) == 64 && quant_bitlen((uint64_t)1 << 43) == 44);
    CHECK(quant_shift(0) == 0 && quant_shift(((uint64_t)1 << 44) - 1) == 0 && quant_shift((uint64_t)1 << 44) == 1 && quant_shift(((uint64_t)1 << 63) - 1) == 19);
    CHECK(quant_share(((uint64_t)1 << 44) - 1, ((uint64_t)1 << 44) - 1) == QUANT_ONE && quant_share(0, 5) == 0 && quant_share(1, 3) == QUANT_ONE / 3);
    CHECK(quant_share(((uint64_t)1 << 44) - 1, ((uint64_t)1 << 50) - 64) == 16384);
    CHECK(quant_term(((uint64_t)1 << 51) - 1, 4096) < ((uint64_t)1 << 63) && quant_weight_ok(1) && quant_weight_ok(4096) && !quant_weight_ok(0) && !quant_weight_ok(4097));
    CHECK(rd_quant_workspace_bytes(0, 0, 0) == 12 * 64 + 4096 && rd_quant_workspace_bytes(-1, 0, 0) == -1);
    std::mt19937_64 rng(4242);
    auto uni = [&](int64_t lo, int64_t hi) { return (int64_t)(lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1))); };
    for (long it = 0; it < iters; it++) {
        const int64_t M = uni(64, 90);
        const int n_multi = (int)uni(0, 12);
        const int64_t n_single = it % 10 == 0 ? uni(5000, 9000) : uni(0, 30);   // (a long run of single reads of transcript 0: the shift)
        std::vector<int64_t> off(1, 0);
        std::vector<int32_t> t;
        std::vector<uint16_t> w;
        auto add_read = [&](int n, int first_t) {
            std::vector<int32_t> all((size_t)M);
            for (int64_t i = 0; i < M; i++) all[(size_t)i] = (int32_t)i;
            for (int j = 0; j < n; j++) std::swap(all[(size_t)j], all[(size_t)uni(j, M - 1)]);
            if (first_t >= 0 && n > 0) {
                for (int j = 1; j < n; j++)
                    if (all[(size_t)j] == first_t) all[(size_t)j] = all[0];
                all[0] = first_t;
            }
            for (int j = 0; j < n; j++) {
                t.push_back(all[(size_t)j]);
                const int64_t pick = uni(0, 3);
                w.push_back((uint16_t)(pick == 0 ? 1 : pick == 1 ? 4096 : uni(1, 4096)));
            }
            off.push_back(off.back() + n);
        };
        for (int64_t i = 0; i < n_single; i++) add_read(1, 0);
        for (int i = 0; i < n_multi; i++) {
            const int64_t choices[8] = {0, 1, 2, 3, 63, 64, uni(2, 64), uni(20, 45)};
            add_read((int)choices[uni(0, 7)], it % 10 == 0 ? 0 : -1);
        }
        const int64_t R = (int64_t)off.size() - 1, slots = off.back();
        int64_t* p_off = exact(off);
        int32_t* p_t = exact(t);
        uint16_t* p_w = exact(w);
        // the packer
        QuantPack P;
        quant_pack(p_off, p_t, p_w, R, M, &P);
        CHECK(P.t.size() % QUANT_ROW == 0 && P.t.size() == P.w.size() && P.t.size() == P.head.size() && P.t.size() == P.end.size() && P.t.size() == P.src.size());
        CHECK((int64_t)P.t.size() <= 2 * slots + QUANT_ROW && P.n_empty + P.n_single + P.n_multi == R);
        {
            int64_t next = -1, multi_slots = 0;
            for (size_t i = 0; i < P.t.size(); i++) {
                const size_t lane = i % QUANT_ROW, row = i - lane;
                CHECK(P.head[i] <= lane && lane <= P.end[i] && P.end[i] < QUANT_ROW);
                CHECK(P.head[row + P.head[i]] == P.head[i] && P.end[row + P.end[i]] == P.end[i]);
                if (P.src[i] < 0) {
                    CHECK(P.t[i] == -1 && P.head[i] == lane && P.end[i] == lane);
                    continue;
                }
                CHECK(P.src[i] > next && P.t[i] == t[(size_t)P.src[i]] && P.w[i] == w[(size_t)P.src[i]]);
                next = P.src[i];
                multi_slots++;
            }
            int64_t expect = 0;
            uint64_t base_sum = 0;
            for (int64_t r = 0; r < R; r++) expect += off[r + 1] - off[r] > 1 ? off[r + 1] - off[r] : 0;
            for (uint64_t b : P.base) base_sum += b;
            CHECK(multi_slots == expect && base_sum == (uint64_t)P.n_single * QUANT_ONE);
        }
        // the host twin against a loop of its own
        const int max_iter = (int)uni(0, 6);
        const uint64_t tol = (uint64_t)(uni(0, 2) ? 0 : 50000);
        uint64_t* count = (uint64_t*)malloc((size_t)M * 8);
        uint32_t* share = (uint32_t*)malloc(slots ? (size_t)slots * 4 : 1);
        int64_t* stats = (int64_t*)malloc(16 * 8);
        CHECK(rd_quant_em_host(p_off, p_t, p_w, R, M, max_iter, tol, count, share, stats) == 0);
        g_accepted++;
        {
            std::vector<uint64_t> c((size_t)M, 1), cn((size_t)M);
            std::vector<uint32_t> sh((size_t)slots);
            own_step(off, t, w, c, cn, sh);
            c.swap(cn);
            int done = 0;
            uint64_t last = 0;
            while (done < max_iter) {
                own_step(off, t, w, c, cn, sh);
                uint64_t d = 0;
                for (int64_t i = 0; i < M; i++) d = std::max(d, c[(size_t)i] > cn[(size_t)i] ? c[(size_t)i] - cn[(size_t)i] : cn[(size_t)i] - c[(size_t)i]);
                c.swap(cn);
                done++;
                last = d;
                if (d <= tol) break;
            }
            uint64_t total = 0;
            for (int64_t i = 0; i < M; i++) {
                CHECK(count[i] == c[(size_t)i]);
                total += count[i];
            }
            for (int64_t i = 0; i < slots; i++) CHECK(share[i] == sh[(size_t)i]);
            CHECK(stats[0] == done && stats[1] == (int64_t)last && stats[3] == P.n_empty && stats[4] == P.n_single && stats[5] == slots);
            CHECK(stats[2] == (int64_t)((uint64_t)(R - P.n_empty) * QUANT_ONE - total) && stats[2] >= 0 && stats[2] <= slots);
        }
        CHECK(rd_quant_em_host(p_off, p_t, p_w, R, M, max_iter, tol, count, nullptr, nullptr) == 0);   // null share and stats are allowed
        // the refusals: RD_ERR_ARG, nothing written
        auto refused = [&](const int64_t* o, const int32_t* tt, const uint16_t* ww, int64_t n_reads, int64_t n_tx, int mi, uint64_t* cnt) {
            memset(count, 0x4d, (size_t)M * 8);
            memset(share, 0x4d, (size_t)slots * 4);
            memset(stats, 0x4d, 16 * 8);
            CHECK(rd_quant_em_host(o, tt, ww, n_reads, n_tx, mi, 0, cnt, share, stats) == -1);
            for (int64_t i = 0; i < M * 8; i++) CHECK(((unsigned char*)count)[i] == 0x4d);
            for (int64_t i = 0; i < slots * 4; i++) CHECK(((unsigned char*)share)[i] == 0x4d);
            for (int64_t i = 0; i < 16 * 8; i++) CHECK(((unsigned char*)stats)[i] == 0x4d);
            g_refused++;
        };
        refused(nullptr, p_t, p_w, R, M, 3, count);
        refused(p_off, p_t, p_w, -1, M, 3, count);
        refused(p_off, p_t, p_w, R, M, -1, count);
        refused(p_off, p_t, p_w, R, M, QUANT_MAX_ITER + 1, count);
        refused(p_off, p_t, p_w, R, (int64_t)1 << 24, 3, count);
        refused(p_off, p_t, p_w, R, M, 3, nullptr);
        if (slots) {
            refused(p_off, nullptr, p_w, R, M, 3, count);
            refused(p_off, p_t, nullptr, R, M, 3, count);
            const auto with_t = [&](size_t i, int32_t v) {
                auto copy = t;
                copy[i] = v;
                int32_t* p = exact(copy);
                refused(p_off, p, p_w, R, M, 3, count);
                free(p);
            };
            const auto with_w = [&](size_t i, uint16_t v) {
                auto copy = w;
                copy[i] = v;
                uint16_t* p = exact(copy);
                refused(p_off, p_t, p, R, M, 3, count);
                free(p);
            };
            with_t((size_t)uni(0, slots - 1), (int32_t)M);
            with_t((size_t)(slots - 1), -1);
            with_w(0, 0);
            with_w((size_t)uni(0, slots - 1), 4097);
            for (int64_t r = 0; r < R; r++)
                if (off[r + 1] - off[r] >= 2) {   // a duplicate within a read: its last candidate takes the name of its first
                    with_t((size_t)(off[r + 1] - 1), t[(size_t)off[r]]);
                    break;
                }
        }
        if (R) {
            const auto with_off = [&](size_t i, int64_t v) {
                auto copy = off;
                copy[i] = v;
                int64_t* p = exact(copy);
                refused(p, p_t, p_w, R, M, 3, count);
                free(p);
            };
            with_off(0, 1);
            with_off(0, -1);
            if (R >= 2 && off[2] > 0) with_off(1, off[2] + 1);   // decreasing at read 1
            {   // a read of 65 candidates (the arrays grow so that the offsets stay inside them)
                auto o2 = off;
                auto t2 = t;
                auto w2 = w;
                for (int j = 0; j < 65; j++) t2.push_back(j), w2.push_back(1);
                o2.push_back(o2.back() + 65);
                int64_t* po = exact(o2);
                int32_t* pt = exact(t2);
                uint16_t* pw = exact(w2);
                refused(po, pt, pw, R + 1, M, 3, count);
                free(po), free(pt), free(pw);
            }
        }
        free(count), free(share), free(stats), free(p_off), free(p_t), free(p_w);
    }
    printf("no sanitizer report\n%ld accepted %ld refused\n", g_accepted, g_refused);
    return 0;
}
