// TEST INFRASTRUCTURE: AddressSanitizer + UBSan harness for the host side of radian_amd/csrc/segment.hip (the argument checks, the rules of
// segment_rules.h, the plain loops of rd_segment_host; sanitizers run on the CPU build only -- the kernels are not compiled here).
// usage: asan_segment <iterations>   The rules at their limits first.  Every iteration draws reads (empty ones and ones shorter than two
// windows among them) and parameters into EXACT-SIZE heap buffers (a read or a write past either end is an ASan report; the event arrays
// hold exactly rd_segment_max_events per read), calls the host twin and checks every field against loops of its own written from the
// contract's text (window sums by direct summation, comparisons in unsigned __int128); then the refusals, which must answer RD_ERR_ARG
// and write nothing.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../radian_amd/csrc/segment.hip"   // the host half (this is no HIP build): the device blocks' layout functions live in its unnamed namespace

extern "C" int rd_segment_host(const int16_t* raw, const int64_t* read_off, int n_reads, int w1, int w2, uint32_t th1, uint32_t th2, int v0,
                               const int64_t* sc_lo, const int64_t* sc_hi, const int64_t* ev_off, int32_t* status, int32_t* n_events, int32_t* m2,
                               int32_t* d4, int32_t* ev_start, int64_t* ev_sum, int64_t* ev_sumsq, int16_t* ev_min, int16_t* ev_max, uint8_t* ev_src);
extern "C" int64_t rd_segment_workspace_bytes(int64_t n_samples, int w1);
extern "C" int64_t rd_segment_max_events(int64_t n_samples, int w1);
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

typedef unsigned __int128 u128;

// the contract over one read: the peak bit of every sample for one detector
static std::vector<char> own_peaks(const std::vector<int16_t>& x, int w, uint32_t th, int v0)
{
    const int64_t T = (int64_t)x.size();
    std::vector<u128> N(T, 0), D(T, 1);
    std::vector<char> peak(T, 0);
    if (w == 0) return peak;
    for (int64_t i = w; i <= T - w; i++) {
        int64_t S1 = 0, Q1 = 0, S2 = 0, Q2 = 0;
        for (int64_t j = i - w; j < i; j++) S1 += x[j], Q1 += (int64_t)x[j] * x[j];
        for (int64_t j = i; j < i + w; j++) S2 += x[j], Q2 += (int64_t)x[j] * x[j];
        N[i] = (u128)((int64_t)w * (S1 - S2) * (S1 - S2));
        D[i] = (u128)(w * Q1 - S1 * S1 + w * Q2 - S2 * S2 + 2 * (int64_t)w * w * v0);
        CHECK(N[i] < ((u128)1 << 50) && D[i] >= (u128)(2 * w * w) && D[i] < ((u128)1 << 44));
    }
    for (int64_t i = 0; i < T; i++) {
        if (!(N[i] > 0 && 16 * N[i] >= (u128)th * D[i])) continue;
        bool ok = true;
        for (int64_t j = std::max<int64_t>(i - w, 0); j < i; j++) ok = ok && N[j] * D[i] < N[i] * D[j];
        for (int64_t j = i + 1; j <= std::min<int64_t>(i + w, T - 1); j++) ok = ok && N[j] * D[i] <= N[i] * D[j];
        peak[i] = ok;
    }
    return peak;
}

static void rules_at_their_limits()
{
    CHECK(sg_status(0) == SG_EMPTY && sg_status(1) == SG_OK && sg_status(SG_MAX_T) == SG_OK && sg_status(SG_MAX_T + 1) == SG_TOO_LONG);
    CHECK(sg_params_ok(SgParams{2, 0, 0, 0, 1}) && sg_params_ok(SgParams{32, 64, 0xffffffffu, 0xffffffffu, 1 << 16}));
    CHECK(!sg_params_ok(SgParams{1, 0, 0, 0, 1}) && !sg_params_ok(SgParams{33, 0, 0, 0, 1}) && !sg_params_ok(SgParams{4, 4, 0, 0, 1}));
    CHECK(!sg_params_ok(SgParams{4, 65, 0, 0, 1}) && !sg_params_ok(SgParams{4, 3, 0, 0, 1}) && !sg_params_ok(SgParams{4, 0, 0, 0, 0}));
    CHECK(!sg_params_ok(SgParams{4, 0, 0, 0, (1 << 16) + 1}));
    // the largest N and D: 64 samples of -32768 against 64 of 32767; alternating +-32767 under the largest floor
    const uint64_t N = sg_num(64, -64 * 32768, 64 * 32767), D = sg_den(64, 0, 64 * (int64_t)32767 * 32767, 0, 64 * (int64_t)32767 * 32767, 1 << 16);
    CHECK(N == (uint64_t)64 * 4194240 * 4194240 && N < ((uint64_t)1 << 50) && D > ((uint64_t)1 << 43) && D < ((uint64_t)1 << 44));
    CHECK(sg_prod_less(N, D - 1, N, D) && !sg_prod_less(N, D, N, D) && !sg_prod_less(N, D, N, D - 1) && sg_prod_less(N - 1, D, N, D));   // beyond 2^64
    CHECK(sg_prod_less(0, D, 1, 1) && !sg_prod_less(1, 1, 0, D));
    CHECK(sg_candidate(1, 1, 16) && !sg_candidate(1, 1, 17) && !sg_candidate(0, 1, 0) && sg_candidate(1, D, 0) && !sg_candidate(N, D, 0xffffffffu));
    CHECK(sg_candidate((uint64_t)1 << 49, 32, 0xffffffffu));   // th D passes 2^36, 16 N = 2^53
    CHECK(sg_yields(3, 5, 1, 2, 1, 2) == false && sg_yields(7, 5, 1, 2, 1, 2) == true);   // a tie: the smaller index wins
    CHECK(sg_shadows(5, 7, 3) && !sg_shadows(4, 7, 3) && sg_shadows(7, 7, 1));
    CHECK(sg_event_row(7, 2) == 4 && sg_event_row(-7, 2) == -3 && sg_event_row(-9, 3) == -3 && sg_event_row(5, 3) == 2 && sg_event_row(-32768 * 5, 5) == -32768);
    CHECK(rd_segment_max_events(0, 4) == 1 && rd_segment_max_events(SG_MAX_T, 2) == SG_MAX_T / 3 + 1 && rd_segment_max_events(-1, 4) == -1 && rd_segment_max_events(9, 1) == -1);
    CHECK(rd_segment_workspace_bytes(0, 4) == 32 + 8 + 8192 && rd_segment_workspace_bytes(4096, 3) == 8 * 4096 + 128 + 32 * 1025 + 24 + 8192);
    CHECK(rd_segment_workspace_bytes(SG_MAX_T, 2) > 0 && rd_segment_workspace_bytes(-1, 4) == -1 && rd_segment_workspace_bytes(1, 33) == -1);
}

// The yardstick of sg_layout: the size expressions and the pointer chain that sg_peaks held before the layout function replaced them,
// written out literally; on seeded random dimensions (0 and 1 of each among them) the total and every block's offset must be equal.
static void check_layout()
{
    std::mt19937_64 rng(7);
    const size_t dims[] = {0, 1, 2, 31, 32, 33, 255, 256, 257};
    auto dim = [&](size_t big) { return rng() % 3 ? dims[rng() % 9] : (size_t)(rng() % big); };
    char* const base = (char*)((uintptr_t)1 << 32);
    for (int it = 0; it < 4000; it++) {
        const size_t n_reads = dim(3000), n_tiles = dim(30000), tmp_bytes = dim(100000);
        const int64_t n = (int64_t)dim(3000000), cap = (int64_t)dim(1500000);
        const bool diag = it % 2;
        const size_t b_reads = align_up(n_reads * sizeof(SgRead), 256), b_tiles = align_up(n_tiles * sizeof(SgTile) + 8, 256),
                     b_byte = align_up((size_t)n + 1, 256), b_pos = align_up(((size_t)n + 1) * 4, 256), b_e8 = align_up((size_t)cap * 8, 256),
                     b_e2 = align_up((size_t)cap * 2, 256), b_e1 = align_up((size_t)cap, 256), b_tmp = align_up(tmp_bytes + 8, 256),
                     b_t = diag ? align_up((size_t)n * 16 + 8, 256) : 0;
        const size_t total = b_reads + b_tiles + 2 * b_byte + b_pos + 3 * b_e8 + 2 * b_e2 + b_e1 + b_tmp + 2 * b_t;
        char* c = base;
        SgWs old;
        old.reads = (SgRead*)c; c += b_reads;
        old.tiles = (SgTile*)c; c += b_tiles;
        old.ev_g = (int64_t*)c; c += b_e8;
        old.ev_sum = (int64_t*)c; c += b_e8;
        old.ev_sumsq = (int64_t*)c; c += b_e8;
        old.tN = (uint64_t*)c; c += b_t;
        old.tD = (uint64_t*)c; c += b_t;
        old.tmp = c; c += b_tmp;
        old.pos = (uint32_t*)c; c += b_pos;
        old.ev_min = (int16_t*)c; c += b_e2;
        old.ev_max = (int16_t*)c; c += b_e2;
        old.flags = (uint8_t*)c; c += b_byte;
        old.bnd = (uint8_t*)c; c += b_byte;
        old.ev_src = (uint8_t*)c;
        SgWs ws;
        Carve dry, wet(base);
        sg_layout(dry, n_reads, n_tiles, n, cap, tmp_bytes, diag, &ws);
        CHECK(dry.at == total && !ws.reads && !ws.ev_src && !ws.tmp);
        sg_layout(wet, n_reads, n_tiles, n, cap, tmp_bytes, diag, &ws);
        CHECK(wet.at == total && ws.reads == old.reads && ws.tiles == old.tiles && ws.ev_g == old.ev_g && ws.ev_sum == old.ev_sum &&
              ws.ev_sumsq == old.ev_sumsq && ws.tN == old.tN && ws.tD == old.tD && ws.tmp == old.tmp && ws.pos == old.pos &&
              ws.ev_min == old.ev_min && ws.ev_max == old.ev_max && ws.flags == old.flags && ws.bnd == old.bnd && ws.ev_src == old.ev_src);
        CHECK(ws.tmp_bytes == tmp_bytes && ws.n == n && ws.cap == cap && ws.n_tiles == (unsigned)n_tiles);
        CHECK((size_t)((char*)ws.ev_src - base) + b_e1 == total);   // (the last block's size stood in the sum only)
    }
}

int main(int argc, char** argv)
{
    const int iters = argc > 1 ? atoi(argv[1]) : 20;
    check_layout();
    rules_at_their_limits();
    std::mt19937_64 rng(2727);
    auto U = [&](int64_t a, int64_t b) { return (int64_t)(a + (int64_t)(rng() % (uint64_t)(b - a + 1))); };
    for (int it = 0; it < iters; it++) {
        const int w1 = (int)U(2, 6), w2 = U(0, 2) == 0 ? 0 : (int)U(w1 + 1, 14), v0 = U(0, 3) == 0 ? 1 << 16 : (int)U(1, 40);
        const uint32_t th1 = (uint32_t)U(0, 400), th2 = U(0, 9) == 0 ? 0xffffffffu : (uint32_t)U(0, 900);
        const int n_reads = (int)U(1, 5);
        std::vector<std::vector<int16_t>> reads(n_reads);
        std::vector<int16_t> raw;
        std::vector<int64_t> off(1, 0), ev_off(1, 0), sc_lo, sc_hi;
        for (auto& x : reads) {
            const int64_t T = U(0, 4) == 0 ? U(0, 2 * w1 + 1) : U(20, 300);
            const bool wild = U(0, 5) == 0;
            int16_t level = 0;
            for (int64_t i = 0; i < T; i++) {
                if (i == 0 || U(0, 11) == 0) level = (int16_t)U(-500, 500);
                x.push_back(wild ? (int16_t)U(-32768, 32767) : (int16_t)(level + U(-8, 8)));
            }
            raw.insert(raw.end(), x.begin(), x.end());
            sc_lo.push_back(off.back() + U(0, T));
            sc_hi.push_back(U(sc_lo.back(), off.back() + T));
            off.push_back(off.back() + T);
            ev_off.push_back(ev_off.back() + rd_segment_max_events(T, w1));
        }
        const int64_t cap = ev_off.back();
        int16_t* d_raw = exact(raw);
        int64_t *d_off = exact(off), *d_ev = exact(ev_off), *d_lo = exact(sc_lo), *d_hi = exact(sc_hi);
        const std::vector<int32_t> f4r(n_reads, 0x5a5a5a5a), f4e(cap, 0x5a5a5a5a);
        const std::vector<int64_t> f8e(cap, 0x5a5a5a5a5a5a5a5all);
        const std::vector<int16_t> f2e(cap, 0x5a5a);
        const std::vector<uint8_t> f1e(cap, 0x5a);
        int32_t *status = exact(f4r), *n_ev = exact(f4r), *m2 = exact(f4r), *d4 = exact(f4r), *e_start = exact(f4e);
        int64_t *e_sum = exact(f8e), *e_sq = exact(f8e);
        int16_t *e_min = exact(f2e), *e_max = exact(f2e);
        uint8_t* e_src = exact(f1e);
        auto call = [&](int nr, int a, int b, int v, bool scale) {
            return rd_segment_host(d_raw, d_off, nr, a, b, th1, th2, v, scale ? d_lo : nullptr, scale ? d_hi : nullptr, d_ev, status, n_ev, m2, d4, e_start,
                                   e_sum, e_sq, e_min, e_max, e_src);
        };
        CHECK(call(n_reads, w1, w2, v0, true) == 0);
        g_accepted++;
        for (int r = 0; r < n_reads; r++) {
            const std::vector<int16_t>& x = reads[r];
            const int64_t T = (int64_t)x.size();
            if (T == 0) {
                CHECK(status[r] == SG_EMPTY && n_ev[r] == 0 && m2[r] == 0 && d4[r] == 0);
                continue;
            }
            // the scale, by sorting
            int32_t um2 = 0, ud4 = 0;
            std::vector<int64_t> v(raw.begin() + sc_lo[r], raw.begin() + sc_hi[r]);
            if (!v.empty()) {
                std::sort(v.begin(), v.end());
                um2 = (int32_t)(v[(v.size() - 1) / 2] + v[v.size() / 2]);
                for (auto& s : v) s = std::llabs(2 * s - um2);
                std::sort(v.begin(), v.end());
                ud4 = (int32_t)(v[(v.size() - 1) / 2] + v[v.size() / 2]);
            }
            CHECK(status[r] == SG_OK && m2[r] == um2 && d4[r] == ud4);
            const std::vector<char> k1 = own_peaks(x, w1, th1, v0), k2 = own_peaks(x, w2, th2, v0);
            int64_t e = -1, last1 = -1000, last = -1000;
            for (int64_t i = 0; i < T; i++) {
                int src = i == 0 ? 0 : k1[i] ? 1 : -1;
                if (src < 0 && k2[i]) {
                    src = 2;
                    for (int64_t j = 0; j < T; j++)
                        if (k1[j] && std::llabs(j - i) < w2) src = -1;
                }
                if (src < 0) continue;
                e++;
                const int64_t o = ev_off[r] + e;
                CHECK(e < n_ev[r] && e_start[o] == i && e_src[o] == src);
                if (src == 1) { CHECK(i - last1 > w1); last1 = i; }
                if (i > 0) { CHECK(i >= w1 && i <= T - w1 && (last < 0 || i - last > w1)); last = i; }
            }
            CHECK(e + 1 == n_ev[r] && n_ev[r] <= rd_segment_max_events(T, w1));
            for (int64_t k = 0; k < n_ev[r]; k++) {
                const int64_t o = ev_off[r] + k, a = e_start[o], b = k + 1 < n_ev[r] ? e_start[o + 1] : T;
                CHECK(a < b);
                int64_t s = 0, q = 0;
                int16_t lo = 32767, hi = -32768;
                for (int64_t i = a; i < b; i++) s += x[i], q += (int64_t)x[i] * x[i], lo = std::min(lo, x[i]), hi = std::max(hi, x[i]);
                CHECK(e_sum[o] == s && e_sq[o] == q && e_min[o] == lo && e_max[o] == hi);
            }
            for (int64_t o = ev_off[r] + n_ev[r]; o < ev_off[r + 1]; o++) CHECK(e_start[o] == 0x5a5a5a5a && e_src[o] == 0x5a);   // the unused slots
        }
        // the refusals: nothing may be written
        for (int r = 0; r < n_reads; r++) status[r] = 0x5a5a5a5a;
        auto refused = [&](int rc) {
            CHECK(rc == -1);
            for (int r = 0; r < n_reads; r++) CHECK(status[r] == 0x5a5a5a5a);
            g_refused++;
        };
        refused(call(-1, w1, w2, v0, true));
        refused(call(n_reads, 1, w2, v0, true));
        refused(call(n_reads, 33, 0, v0, true));
        refused(call(n_reads, w1, w1, v0, true));
        refused(call(n_reads, w1, 65, v0, true));
        refused(call(n_reads, w1, w2, 0, true));
        refused(call(n_reads, w1, w2, (1 << 16) + 1, true));
        { const int64_t keep = d_off[0]; d_off[0] = -1; refused(call(n_reads, w1, w2, v0, true)); d_off[0] = keep; }
        { const int64_t keep = d_off[n_reads]; d_off[n_reads] = d_off[n_reads - 1] - 1; refused(call(n_reads, w1, w2, v0, true)); d_off[n_reads] = keep; }
        if (!reads[n_reads - 1].empty()) { const int64_t keep = d_ev[n_reads]; d_ev[n_reads] = keep - 1; refused(call(n_reads, w1, w2, v0, true)); d_ev[n_reads] = keep; }
        { const int64_t keep = d_hi[0]; d_hi[0] = d_off[1] + 1; refused(call(n_reads, w1, w2, v0, true)); d_hi[0] = keep; }
        { const int64_t keep = d_lo[0]; d_lo[0] = d_hi[0] + 1; refused(call(n_reads, w1, w2, v0, true)); d_lo[0] = keep; }
        CHECK(rd_segment_host(d_raw, d_off, n_reads, w1, w2, th1, th2, v0, d_lo, nullptr, d_ev, status, n_ev, m2, d4, e_start, e_sum, e_sq, e_min, e_max, e_src) == -1);
        CHECK(rd_segment_host(d_raw, d_off, n_reads, w1, w2, th1, th2, v0, d_lo, d_hi, d_ev, status, n_ev, nullptr, d4, e_start, e_sum, e_sq, e_min, e_max, e_src) == -1);
        CHECK(rd_segment_host(d_raw, d_off, n_reads, w1, w2, th1, th2, v0, nullptr, nullptr, d_ev, status, n_ev, m2, d4, e_start, e_sum, e_sq, e_min, e_max, nullptr) == -1);
        g_refused += 3;
        for (int r = 0; r < n_reads; r++) CHECK(status[r] == 0x5a5a5a5a);
        CHECK(call(n_reads, w1, w2, v0, false) == 0);   // without scale windows: m2 = d4 = 0; and the buffers are as they were
        g_accepted++;
        for (int r = 0; r < n_reads; r++) CHECK(m2[r] == 0 && d4[r] == 0);
        for (void* p : {(void*)d_raw, (void*)d_off, (void*)d_ev, (void*)d_lo, (void*)d_hi, (void*)status, (void*)n_ev, (void*)m2, (void*)d4, (void*)e_start,
                        (void*)e_sum, (void*)e_sq, (void*)e_min, (void*)e_max, (void*)e_src})
            free(p);
    }
    printf("no sanitizer report\n%ld accepted %ld refused\n", g_accepted, g_refused);
    return 0;
}
