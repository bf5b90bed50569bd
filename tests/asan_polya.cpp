// TEST INFRASTRUCTURE: AddressSanitizer + UBSan harness for the host side of radian_amd/csrc/polya.hip (the argument check, the rules of
// polya_rules.h and the plain loop of rd_polya_segment_host; sanitizers run on the CPU build only -- the kernels are not compiled here).
// usage: asan_polya <iterations>   Every iteration draws a batch of reads of the test cases' shapes (0, win - 1, win, 2 win - 1 samples;
// 63 .. 257 windows; constant reads; the int16 extremes) into EXACT-SIZE heap buffers (a read or a write past either end is an ASan
// report), calls rd_polya_segment_host and checks every output against its invariants and a window loop of its own; then the same buffers
// go through the refusals, which must answer RD_ERR_ARG and write nothing.  The threshold rule is also called directly where no read can
// take it: beyond A = 2^41, up to its saturation.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../radian_amd/csrc/polya.hip"   // the host half (this is no HIP build): the launch's layout function lives in its unnamed namespace

extern "C" int rd_polya_segment_host(const int16_t* raw, const int64_t* read_off, int n_reads, int win, int flat_q, int use_level, int lo_q, int hi_q,
                                     int max_gap, int64_t min_samples, int64_t search_limit, int32_t* status, int64_t* tail_start,
                                     int64_t* tail_end, int32_t* n_flat, int64_t* sum, int64_t* sumsq, int32_t* m2, int32_t* d4, int32_t* n_candidates);
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

struct Outs {
    int32_t *status, *n_flat, *m2, *d4, *ncand;
    int64_t *start, *end, *sum, *sumsq;
    size_t n;
    explicit Outs(size_t n_) : n(n_)
    {
        const size_t m = n ? n : 1;
        status = (int32_t*)malloc(m * 4), n_flat = (int32_t*)malloc(m * 4), m2 = (int32_t*)malloc(m * 4), d4 = (int32_t*)malloc(m * 4);
        ncand = (int32_t*)malloc(m * 4);
        start = (int64_t*)malloc(m * 8), end = (int64_t*)malloc(m * 8), sum = (int64_t*)malloc(m * 8), sumsq = (int64_t*)malloc(m * 8);
        for (size_t i = 0; i < n; i++) status[i] = n_flat[i] = m2[i] = d4[i] = ncand[i] = 77, start[i] = end[i] = sum[i] = sumsq[i] = 77;
    }
    ~Outs() { free(status), free(n_flat), free(m2), free(d4), free(ncand), free(start), free(end), free(sum), free(sumsq); }
    bool untouched() const
    {
        for (size_t i = 0; i < n; i++)
            if (status[i] != 77 || n_flat[i] != 77 || m2[i] != 77 || d4[i] != 77 || ncand[i] != 77 || start[i] != 77 || end[i] != 77 || sum[i] != 77 ||
                sumsq[i] != 77)
                return false;
        return true;
    }
};

static int call(const int16_t* raw, const int64_t* off, int n, const PaParams& p, Outs& o)
{
    return rd_polya_segment_host(raw, off, n, p.win, p.flat_q, p.use_level, p.lo_q, p.hi_q, p.max_gap, p.min_samples, p.search_limit, o.status, o.start,
                                 o.end, o.n_flat, o.sum, o.sumsq, o.m2, o.d4, o.ncand);
}

// The yardstick of pa_layout: the size expressions and the pointer chain that pa_run held before the layout function replaced them, written
// out literally; on seeded random dimensions (0 and 1 of each among them) the total and every block's offset must be equal.
static void check_layout()
{
    std::mt19937_64 rng(7);
    const size_t dims[] = {0, 1, 2, 31, 32, 33, 255, 256, 257};
    auto dim = [&](size_t big) { return rng() % 3 ? dims[rng() % 9] : (size_t)(rng() % big); };
    for (int it = 0; it < 4000; it++) {
        const size_t n_reads = dim(5000), n_blocks = dim(20000);
        const int64_t nwin = (int64_t)dim(2000000);
        const size_t b_reads = align_up(n_reads * sizeof(PaRead), 256), b_scale = align_up((size_t)n_reads * sizeof(PaScale), 256),
                     b_blocks = align_up(n_blocks * sizeof(PaBlock) + 8, 256), b_flag = align_up((size_t)nwin + 8, 256),
                     b_S = align_up((size_t)nwin * 4 + 8, 256), b_Q = align_up((size_t)nwin * 8 + 8, 256);
        const size_t total = b_reads + b_scale + b_blocks + b_flag + b_S + b_Q;
        char* const base = (char*)((uintptr_t)1 << 32);
        char* c = base;
        PaWs old;
        old.reads = (PaRead*)c; c += b_reads;
        old.scale = (PaScale*)c; c += b_scale;
        old.blocks = (PaBlock*)c; c += b_blocks;
        old.Q = (int64_t*)c; c += b_Q;
        old.S = (int32_t*)c; c += b_S;
        old.flag = (uint8_t*)c;
        PaWs ws;
        Carve dry, wet(base);
        pa_layout(dry, n_reads, n_blocks, nwin, &ws);
        CHECK(dry.at == total && !ws.reads && !ws.scale && !ws.blocks && !ws.Q && !ws.S && !ws.flag);
        pa_layout(wet, n_reads, n_blocks, nwin, &ws);
        CHECK(wet.at == total && ws.reads == old.reads && ws.scale == old.scale && ws.blocks == old.blocks && ws.Q == old.Q && ws.S == old.S &&
              ws.flag == old.flag && ws.n_windows == nwin);
        CHECK((size_t)((char*)ws.flag - base) + b_flag == total);   // (the last block's size stood in the sum only)
    }
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const int iters = atoi(argv[1]);
    check_layout();
    std::mt19937_64 rng(2025);
    auto uni = [&](int64_t lo, int64_t hi) { return (int64_t)(lo + rng() % (uint64_t)(hi - lo + 1)); };

    // the threshold rule beyond what a read can give: A = win flat_q d4 with d4 up to 2^31 - 1
    auto thr128 = [](uint64_t win, uint64_t fq, uint64_t d4) {
        const unsigned __int128 A = (unsigned __int128)(win * fq * d4), q = A * A >> 20;
        return q >> 64 ? ~(uint64_t)0 : (uint64_t)q;
    };
    CHECK(pa_threshold(8, 1, 0) == 0);
    CHECK(pa_threshold(256, 32767, 262142) == thr128(256, 32767, 262142) && pa_threshold(256, 32767, 262142) < ~(uint64_t)0);   // the largest A of the contract: below 2^41
    CHECK(pa_threshold(256, 16384, 1 << 19) == ((uint64_t)1 << 62));                                                           // A = 2^41: A^2 / 2^20 = 2^62
    CHECK(pa_threshold(256, 32767, 1 << 19) == thr128(256, 32767, 1 << 19) && pa_threshold(256, 32767, 1 << 19) < ~(uint64_t)0);   // A = 2^42 - 2^27: just below
    CHECK(pa_threshold(256, 32768, 1 << 19) == ~(uint64_t)0);                                                                  // A = 2^42: A^2 = 2^84 saturates
    CHECK(pa_threshold(256, 32767, INT32_MAX) == ~(uint64_t)0);
    CHECK(pa_threshold(1, 1, 1 << 16) == ((uint64_t)1 << 12) && pa_threshold(1, 1, 1023) == 0 && pa_threshold(1, 1, 1024) == 1);
    for (int k = 0; k < 2000; k++) {
        const uint64_t win = (uint64_t)uni(8, 256), fq = (uint64_t)uni(1, 32767), d4 = (uint64_t)uni(0, k % 2 ? 262142 : INT32_MAX);
        CHECK(pa_threshold((int32_t)win, (int32_t)fq, (int32_t)d4) == thr128(win, fq, d4));
    }

    for (int it = 0; it < iters; it++) {
        PaParams p;
        p.win = (int32_t)(it % 5 == 0 ? 256 : it % 5 == 1 ? 8 : uni(8, 256));
        p.flat_q = (int32_t)(it % 3 == 0 ? 32767 : uni(1, 400));
        p.use_level = (int32_t)uni(0, 1);
        p.lo_q = (int32_t)uni(-(1 << 20), 0);
        p.hi_q = (int32_t)uni(0, 1 << 20);
        p.max_gap = (int32_t)(it % 7 == 0 ? 1024 : uni(0, 4));
        p.min_samples = p.win * uni(1, 4);
        p.search_limit = it % 2 ? 0 : p.win * uni(0, 40) + uni(0, 1);
        const int n = (int)uni(1, 6);
        std::vector<int16_t> raw;
        std::vector<int64_t> off(1, 0);
        const int64_t nws[] = {63, 64, 65, 255, 256, 257};
        for (int r = 0; r < n; r++) {
            const int shape = (int)uni(0, 7);
            int64_t T = shape == 0 ? 0 : shape == 1 ? p.win - 1 : shape == 2 ? p.win : shape == 3 ? 2 * p.win - 1
                                                                                                : p.win * (p.win > 64 ? uni(1, 9) : nws[uni(0, 5)]) + uni(0, p.win - 1);
            const int kind = (int)uni(0, 3);   // 0 constant, 1 the int16 extremes alternating, 2 / 3 quiet and loud stretches
            const int16_t level = (int16_t)uni(-3000, 3000);
            for (int64_t i = 0; i < T; i++) {
                int v;
                if (kind == 0) v = level;
                else if (kind == 1) v = i % 2 ? 32767 : -32768;
                else v = level + (((i / (3 * p.win)) % 2) ? (int)uni(-2, 2) : (int)uni(-3000, 3000));
                raw.push_back((int16_t)v);
            }
            off.push_back((int64_t)raw.size());
        }
        int16_t* x = exact(raw);
        int64_t* o = exact(off);
        {
            Outs out(n);
            CHECK(call(x, o, n, p, out) == 0);
            for (int r = 0; r < n; r++) {
                const int64_t T = o[r + 1] - o[r];
                const int st = out.status[r];
                CHECK(st >= PA_OK && st <= PA_EMPTY);
                CHECK((st == PA_EMPTY) == (T == 0));
                if (T == 0) CHECK(out.m2[r] == 0 && out.d4[r] == 0);
                if (T > 0) CHECK((st == PA_MAD_ZERO) == (out.d4[r] == 0));
                if (T > 0 && out.d4[r] != 0) CHECK((st == PA_SHORT) == (T < p.win));
                if (st != PA_OK) {
                    CHECK(out.start[r] == -1 && out.end[r] == -1 && out.n_flat[r] == 0 && out.sum[r] == 0 && out.sumsq[r] == 0);
                    CHECK(out.ncand[r] == 0);
                    continue;
                }
                const int64_t a = out.start[r], e = out.end[r];
                CHECK(a >= 0 && a < e && e <= T - T % p.win && a % p.win == 0 && e % p.win == 0);
                CHECK(e - a >= p.min_samples && (p.search_limit == 0 || a < p.search_limit) && out.ncand[r] >= 1);
                // the segment's own windows: its ends are flat, no run of more than max_gap non-flat windows inside, the counts and sums agree
                const uint64_t thr = pa_threshold(p.win, p.flat_q, out.d4[r]);
                int64_t sum = 0, sq = 0;
                int flats = 0, gap = 0;
                for (int64_t j = a / p.win; j < e / p.win; j++) {
                    int32_t S = 0;
                    int64_t Q = 0;
                    for (int i = 0; i < p.win; i++) {
                        const int v = x[o[r] + j * p.win + i];
                        S += v;
                        Q += (int64_t)v * v;
                    }
                    sum += S;
                    sq += Q;
                    const bool f = pa_flat(p, out.m2[r], out.d4[r], thr, S, Q);
                    if (j == a / p.win || j == e / p.win - 1) CHECK(f);
                    gap = f ? 0 : gap + 1;
                    CHECK(gap <= p.max_gap);
                    flats += f;
                }
                CHECK(flats == out.n_flat[r] && sum == out.sum[r] && sq == out.sumsq[r]);
            }
            g_accepted++;
        }
        // refusals: nothing is written
        auto refuse = [&](const int16_t* xr, const int64_t* orr, int nn, const PaParams& q, int null_out) {
            Outs out(n);
            int32_t* keep = out.n_flat;
            if (null_out) out.n_flat = nullptr;
            const int rc = call(xr, orr, nn, q, out);
            out.n_flat = keep;
            CHECK(rc == -1 && out.untouched());
            g_refused++;
        };
        refuse(nullptr, o, n, p, 0);
        refuse(x, nullptr, n, p, 0);
        refuse(x, o, n, p, 1);
        refuse(x, o, -1, p, 0);
        {
            std::vector<int64_t> bad(off);
            bad[n] = bad[n - 1] - 1;
            int64_t* b = exact(bad);
            refuse(x, b, n, p, 0);
            free(b);
        }
        PaParams q = p;
        q.win = 7; refuse(x, o, n, q, 0); q = p;
        q.win = 257; q.min_samples = 257; refuse(x, o, n, q, 0); q = p;
        q.flat_q = 0; refuse(x, o, n, q, 0); q = p;
        q.flat_q = 32768; refuse(x, o, n, q, 0); q = p;
        q.use_level = 2; refuse(x, o, n, q, 0); q = p;
        q.lo_q = -(1 << 20) - 1; refuse(x, o, n, q, 0); q = p;
        q.hi_q = (1 << 20) + 1; refuse(x, o, n, q, 0); q = p;
        q.lo_q = 5; q.hi_q = 4; refuse(x, o, n, q, 0); q = p;
        q.max_gap = -1; refuse(x, o, n, q, 0); q = p;
        q.max_gap = 1025; refuse(x, o, n, q, 0); q = p;
        q.min_samples = p.win - 1; refuse(x, o, n, q, 0); q = p;
        q.search_limit = -1; refuse(x, o, n, q, 0);
        {
            Outs none(0);
            CHECK(call(nullptr, nullptr, 0, p, none) == 0);   // n_reads == 0 is RD_OK
        }
        free(x);
        free(o);
    }
    printf("no sanitizer report\n%ld accepted %ld refused\n", g_accepted, g_refused);
    return 0;
}
