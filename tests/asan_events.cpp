// TEST INFRASTRUCTURE: AddressSanitizer + UBSan harness for the host side of radian_amd/csrc/events.hip (the argument check, the boundary
// rule and the plain loop of rd_event_stats_host; sanitizers run on the CPU build only -- the kernel is not compiled here).
// usage: asan_events <iterations>   Every iteration draws a batch of reads with random valid steps into EXACT-SIZE heap buffers (a read or a
// write past either end is an ASan report), calls rd_event_stats_host and compares every value with a loop of its own; then the same
// buffers go through the refusals -- one broken step, offset or pointer at a time -- which must answer RD_ERR_ARG and write nothing.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
extern "C" int rd_event_stats_host(const int16_t* raw, const int64_t* read_off, int n_reads, const int32_t* first_step, const int32_t* last_step,
                                   const int64_t* label_off, const int32_t* label_len, const int32_t* align_status, int32_t* ev_start,
                                   int32_t* ev_end, int64_t* ev_sum, int64_t* ev_sumsq, int16_t* ev_min, int16_t* ev_max);
#include "../radian_amd/csrc/events.hip"   // the host half (this is no HIP build): the device blocks' layout functions live in its unnamed namespace

void rd_set_error(const char* fmt, ...) { (void)fmt; }

static long g_accepted = 0, g_refused = 0;

template <typename T> static T* exact(const std::vector<T>& v)
{
    T* p = (T*)malloc(v.size() ? v.size() * sizeof(T) : 1);
    if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            printf("line %d: %s does not hold\n", __LINE__, #cond);     \
            exit(1);                                                     \
        }                                                                \
    } while (0)

struct Outs {
    int32_t *start, *end;
    int64_t *sum, *sumsq;
    int16_t *mn, *mx;
    explicit Outs(size_t n)
    {
        const size_t m = n ? n : 1;
        start = (int32_t*)malloc(m * 4), end = (int32_t*)malloc(m * 4);
        sum = (int64_t*)malloc(m * 8), sumsq = (int64_t*)malloc(m * 8);
        mn = (int16_t*)malloc(m * 2), mx = (int16_t*)malloc(m * 2);
        for (size_t i = 0; i < n; i++) start[i] = end[i] = 77, sum[i] = sumsq[i] = 77, mn[i] = mx[i] = 77;
    }
    ~Outs() { free(start), free(end), free(sum), free(sumsq), free(mn), free(mx); }
    bool untouched(size_t n) const
    {
        for (size_t i = 0; i < n; i++)
            if (start[i] != 77 || end[i] != 77 || sum[i] != 77 || sumsq[i] != 77 || mn[i] != 77 || mx[i] != 77) return false;
        return true;
    }
};

// The yardstick of ev_io_layout: the size expressions and the pointer chain it held before it took a Carve, written out literally; on
// seeded random label counts (0 and 1 among them) the total and every array's offset must be equal.
static void check_layout()
{
    std::mt19937_64 rng(7);
    const size_t dims[] = {0, 1, 2, 31, 32, 33, 255, 256, 257};
    auto dim = [&](size_t big) { return rng() % 3 ? dims[rng() % 9] : (size_t)(rng() % big); };
    char* const base = (char*)((uintptr_t)1 << 32);
    for (int it = 0; it < 4000; it++) {
        const size_t n = dim(3000000), a4 = align_up(n * 4 + 16, 256), a8 = align_up(n * 8 + 16, 256), a2 = align_up(n * 2 + 16, 256);
        const size_t total = 4 * a4 + 2 * a8 + 2 * a2;
        char* p = base;
        EvIo old;
        old.first = (int32_t*)p; p += a4;
        old.last = (int32_t*)p; p += a4;
        old.start = (int32_t*)p; p += a4;
        old.end = (int32_t*)p; p += a4;
        old.sum = (int64_t*)p; p += a8;
        old.sumsq = (int64_t*)p; p += a8;
        old.mn = (int16_t*)p; p += a2;
        old.mx = (int16_t*)p;
        EvIo io;
        Carve dry, wet(base);
        ev_io_layout(dry, (int64_t)n, &io);
        CHECK(dry.at == total && !io.first && !io.mx);
        ev_io_layout(wet, (int64_t)n, &io);
        CHECK(wet.at == total && io.first == old.first && io.last == old.last && io.start == old.start && io.end == old.end && io.sum == old.sum &&
              io.sumsq == old.sumsq && io.mn == old.mn && io.mx == old.mx);
    }
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const int iters = atoi(argv[1]);
    check_layout();
    std::mt19937_64 rng(2024);
    auto below = [&](uint64_t n) { return (int64_t)(rng() % n); };
    for (int it = 0; it < iters; it++) {
        const int n_reads = 1 + (int)below(5);
        std::vector<int16_t> raw;
        std::vector<int64_t> read_off{0}, label_off;
        std::vector<int32_t> first, last, label_len, status;
        for (int r = 0; r < n_reads; r++) {
            const int L = below(4) == 0 ? 0 : 1 + (int)below(90);
            const bool ok = below(5) != 0;
            int32_t t = (int32_t)below(4);   // samples of no event before the first label
            label_off.push_back((int64_t)first.size());
            label_len.push_back(L);
            status.push_back(ok ? 0 : 1 + (int32_t)below(2));
            for (int k = 0; k < L; k++) {
                const int32_t n = below(20) == 0 ? 64 + (int32_t)below(200) : 1 + (int32_t)below(12);
                const int32_t own = 1 + (int32_t)below(n);
                first.push_back(ok ? t : -1);
                last.push_back(ok ? t + own - 1 : -1);
                t += n;
            }
            const int64_t T = ok ? t + below(4) : 1 + below(50);
            for (int64_t i = 0; i < T; i++) raw.push_back((int16_t)(below(65536) - 32768));
            read_off.push_back((int64_t)raw.size());
        }
        const size_t nl = first.size();
        int16_t* x = exact(raw);
        int64_t *ro = exact(read_off), *lo = exact(label_off);
        int32_t *f = exact(first), *l = exact(last), *ll = exact(label_len), *st = exact(status);
        {
            Outs o(nl);
            CHECK(rd_event_stats_host(x, ro, n_reads, f, l, lo, ll, st, o.start, o.end, o.sum, o.sumsq, o.mn, o.mx) == 0);
            g_accepted++;
            for (int r = 0; r < n_reads; r++)
                for (int k = 0; k < label_len[r]; k++) {
                    const size_t at = (size_t)label_off[r] + k;
                    if (status[r] != 0) {
                        CHECK(o.start[at] == -1 && o.end[at] == -1 && o.sum[at] == 0 && o.sumsq[at] == 0 && o.mn[at] == 0 && o.mx[at] == 0);
                        continue;
                    }
                    const int32_t s = first[at], e = k + 1 < label_len[r] ? first[at + 1] : last[at] + 1;
                    int64_t sum = 0, sq = 0;
                    int mn = 32767, mx = -32768;
                    for (int32_t i = s; i < e; i++) {
                        const int v = raw[(size_t)read_off[r] + i];
                        sum += v, sq += (int64_t)v * v;
                        mn = v < mn ? v : mn, mx = v > mx ? v : mx;
                    }
                    CHECK(o.start[at] == s && o.end[at] == e && o.sum[at] == sum && o.sumsq[at] == sq && o.mn[at] == mn && o.mx[at] == mx);
                }
        }
        // refusals: the first OK read with at least two labels gets one broken step at a time
        auto refused = [&](const int16_t* x_, const int64_t* ro_, const int32_t* f_, const int32_t* l_, const int64_t* lo_, const int32_t* ll_,
                           const int32_t* st_, int null_out) {
            Outs o(nl);
            const int rc = rd_event_stats_host(x_, ro_, n_reads, f_, l_, lo_, ll_, st_, null_out == 0 ? nullptr : o.start, null_out == 1 ? nullptr : o.end,
                                               null_out == 2 ? nullptr : o.sum, null_out == 3 ? nullptr : o.sumsq, null_out == 4 ? nullptr : o.mn,
                                               null_out == 5 ? nullptr : o.mx);
            CHECK(rc == -1);
            CHECK(o.untouched(nl));
            g_refused++;
        };
        int victim = -1;
        for (int r = 0; r < n_reads && victim < 0; r++)
            if (status[r] == 0 && label_len[r] >= 2) victim = r;
        if (victim >= 0) {
            const size_t at = (size_t)label_off[victim];
            const int32_t T = (int32_t)(read_off[victim + 1] - read_off[victim]);
            const size_t end = at + label_len[victim] - 1;
            struct Edit { int which; size_t at; int32_t v; };
            const Edit edits[] = {{0, at, -1}, {0, at + 1, last[at + 1] + 1}, {1, end, T}, {1, at, first[at + 1]}, {1, at, first[at + 1] + 3}};
            for (const Edit& e : edits) {
                std::vector<int32_t> ff = first, lv = last;
                (e.which == 0 ? ff : lv)[e.at] = e.v;
                int32_t *f2 = exact(ff), *l2 = exact(lv);
                refused(x, ro, f2, l2, lo, ll, st, -1);
                free(f2), free(l2);
            }
        }
        if (nl) {
            for (int which = 0; which < 6; which++) refused(x, ro, f, l, lo, ll, st, which);
            refused(x, ro, nullptr, l, lo, ll, st, -1);
            refused(x, ro, f, nullptr, lo, ll, st, -1);
        }
        refused(nullptr, ro, f, l, lo, ll, st, -1);
        refused(x, nullptr, f, l, lo, ll, st, -1);
        refused(x, ro, f, l, nullptr, ll, st, -1);
        refused(x, ro, f, l, lo, nullptr, st, -1);
        refused(x, ro, f, l, lo, ll, nullptr, -1);
        {
            std::vector<int64_t> bad = read_off;   // offsets that are not monotone
            bad[1 + (size_t)below(n_reads)] = -1;
            int64_t* b = exact(bad);
            refused(x, b, f, l, lo, ll, st, -1);
            free(b);
            std::vector<int32_t> neg = label_len;
            neg[(size_t)below(n_reads)] = -1;
            int32_t* n2 = exact(neg);
            refused(x, ro, f, l, lo, n2, st, -1);
            free(n2);
            if (n_reads >= 2 && label_len[0] > 0) {
                std::vector<int64_t> ov = label_off;   // the second read's labels start inside the first's
                ov[1] = label_off[0] + label_len[0] - 1;
                int64_t* o2 = exact(ov);
                refused(x, ro, f, l, o2, ll, st, -1);
                free(o2);
            }
        }
        free(x), free(ro), free(lo), free(f), free(l), free(ll), free(st);
    }
    printf("no sanitizer report\n%ld accepted %ld refused\n", g_accepted, g_refused);
    return 0;
}
