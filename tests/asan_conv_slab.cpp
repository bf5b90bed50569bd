// TEST INFRASTRUCTURE: AddressSanitizer + UBSan harness AND property check for the slab-tile classification (rd_slab_tile, common.h; DESIGN.md
// 4.1) on the tile lists of radian_amd/csrc/plan.hip.  Random models, read sets, chunk and step, drawn as tests/asan_headpack.cpp draws
// them; chunk-mode and global-mode plans.  For every layer's list and every workgroup tile of it:
//   * the tile qualifies exactly when, by the row-by-row statement of the rule, its 128 rows are rows t0 .. t0 + 127 of ONE segment, all of
//     them computed (t < seg_len) and present as input (t < in_len), and no conv-input or residual row of them is redirected to the read's
//     stream (t < alt_in, t < alt_res) -- a segment's last partial tile, a tile that mixes segments, head rows behind the switch and padding
//     descriptors never qualify;
//   * every row a qualifying tile's region holds for any dilation 1 .. RD_SLAB_DMAX -- time steps t0 - 2 d .. t0 + 127 that are >= 0 -- is a
//     row of the same segment inside the activation tensors (what the kernel DMAs without looking at alt_row);
//   * TileLists::slab is the number of qualifying tiles of the list, TileLists::slab_stream that of the stream prefix a packed launch
//     runs, and the mixed tile's own descriptors (head sub-tiles emptied) do not qualify.
#include "../radian_amd/csrc/plan.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>

void rd_set_error(const char* fmt, ...) { (void)fmt; }
extern "C" hipError_t hipHostMalloc(void** p, size_t n, unsigned int) { *p = malloc(n); return hipSuccess; }
extern "C" hipError_t hipHostFree(void* p) { free(p); return hipSuccess; }
extern "C" const char* hipGetErrorString(hipError_t) { return "stub"; }

#define CHECK(cond, ...)                                                          \
    do {                                                                          \
        if (!(cond)) {                                                            \
            printf("property violated: %s  (", #cond);                           \
            printf(__VA_ARGS__);                                                  \
            printf(")\n");                                                        \
            return 1;                                                             \
        }                                                                         \
    } while (0)

// the rule row by row: tile row R (0 .. 127) belongs to sub-tile R / 32 and is time step d[R / 32].t0 + R % 32 of its segment
static bool slab_by_rows(const TileDesc* d)
{
    for (int R = 0; R < 128; R++) {
        const TileDesc& s = d[R / 32];
        const int64_t t = (int64_t)s.t0 + R % 32;
        if (s.seg_row != d[0].seg_row || s.seg_len != d[0].seg_len || s.in_len != d[0].in_len) return false;   // one segment
        if (t != (int64_t)d[0].t0 + R) return false;                                                          // consecutive rows
        if (t >= s.seg_len || t >= s.in_len) return false;                                                    // interior
        if (t >= s.alt_in || t >= s.alt_res) return false;                                                    // the segment's own rows
    }
    return d[0].t0 >= 0;
}

static int check_lists(const rdi::ReadsPlan& P, const TileLists& tl, const std::vector<TileDesc>& host, const TileDesc* dev, bool packed, int it,
                       const char* mode, long* n_slab, long* n_tiles)
{
    for (int li = 0; li < P.n_layers; li++) {
        const TileDesc* list = &host[tl.d[li] - dev];
        int count = 0, count_stream = 0;
        const int n_run = tl.pack[li].n_tiles > 0 ? tl.pack[li].n_stream_tiles - tl.pack[li].mixed : 0;
        for (int i = 0; i < tl.n[li]; i++) {
            const TileDesc* d = list + 4 * (size_t)i;
            const bool q = rd_slab_tile(d);
            CHECK(q == slab_by_rows(d), "it %d %s layer %d tile %d: rd_slab_tile says %d", it, mode, li, i, (int)q);
            (*n_tiles)++;
            if (!q) continue;
            count++;
            if (i < n_run) count_stream++;
            for (int dil = 1; dil <= RD_SLAB_DMAX; dil++)
                for (int64_t t = std::max<int64_t>(0, (int64_t)d[0].t0 - 2 * dil); t < (int64_t)d[0].t0 + 128; t++) {
                    CHECK(t < d[0].alt_in && t < d[0].in_len, "it %d %s layer %d tile %d: region row t = %lld is not the segment's own", it, mode, li, i, (long long)t);
                    CHECK(d[0].seg_row + t >= 0 && d[0].seg_row + t < P.total_rows, "it %d %s layer %d tile %d: region row %lld of %lld", it, mode, li, i,
                          (long long)(d[0].seg_row + t), (long long)P.total_rows);
                }
        }
        *n_slab += count;
        CHECK(tl.slab[li] == count, "it %d %s layer %d: TileLists::slab %d, %d tiles qualify", it, mode, li, tl.slab[li], count);
        CHECK(tl.slab_stream[li] == (packed ? count_stream : 0), "it %d %s layer %d: TileLists::slab_stream %d, %d stream-prefix tiles qualify", it, mode, li,
              tl.slab_stream[li], count_stream);
        if (tl.pack[li].n_tiles > 0 && tl.pack[li].mixed) {
            const TileDesc* mixed = &host[tl.head_segs[li] - dev] + tl.pack[li].n_heads;
            CHECK(!rd_slab_tile(mixed), "it %d %s layer %d: the mixed tile qualifies", it, mode, li);
        }
    }
    for (int li = P.n_layers; li < RD_MAX_LAYERS; li++) CHECK(tl.slab[li] == 0 && tl.slab_stream[li] == 0, "it %d %s layer %d: counts of a layer that does not exist", it, mode, li);
    return 0;
}

static int check_plan(rdi::ReadsPlan& P, bool pack, int it, const char* mode, long* n_slab, long* n_tiles)
{
    using namespace rdi;
    const size_t n_list = plan_pad_tiles(P), n_pack = pack ? plan_packed_descs(P) : 0;
    std::vector<TileDesc> dev(n_list + n_pack + 1), host(n_list + n_pack + 1);
    TileLists tl;
    memset((void*)&tl, 0x77, sizeof tl);
    CHECK(plan_fill_lists(P, dev.data(), host.data(), tl) == n_list, "it %d %s: list descriptors", it, mode);
    if (pack) CHECK(plan_fill_packed(P, dev.data() + n_list, host.data() + n_list, tl) == n_pack, "it %d %s: packed descriptors", it, mode);
    return check_lists(P, tl, host, dev.data(), pack, it, mode, n_slab, n_tiles);
}

int main(int argc, char** argv)
{
    using namespace rdi;
    const int iters = argc > 1 ? atoi(argv[1]) : 5000;
    std::mt19937_64 rng(31);
    long n_slab = 0, n_tiles = 0;
    for (int it = 0; it < iters; it++) {
        Model m;
        m.nblocks = 1 + (int)(rng() % 7);
        int halo = 0;
        for (int b = 0; b < m.nblocks; b++) {
            m.dil[b] = 1 << (rng() % 7);
            if (rng() % 5 == 0) m.dil[b] = 1 + (int)(rng() % 70);
            halo += 4 * m.dil[b];
        }
        const int chunk = (it % 3 == 0) ? 1024 : 8 + (int)(rng() % 1500);
        const int step = (rng() % 6 == 0) ? chunk : 1 + (int)(rng() % chunk);
        const int n_reads = 1 + (int)(rng() % 7);
        std::vector<int64_t> off(n_reads + 1, 0);
        for (int r = 0; r < n_reads; r++) {
            int64_t N = 1 + (int64_t)(rng() % (rng() % 4 ? 3 * chunk : 12 * chunk));
            if (rng() % 9 == 0) N = chunk + (int64_t)(rng() % 3) * step;
            if (rng() % 7 == 0) N = 128 * (1 + (int64_t)(rng() % 4)) + (int64_t)(rng() % 3) - 1;   // around the tile edge
            off[r + 1] = off[r] + N;
        }
        for (int pack = 0; pack < 2; pack++) {
            ReadsPlan P;
            CHECK(plan_reads_chunk(m, off.data(), n_reads, chunk, step, halo, P) == 0, "it %d: plan_reads_chunk failed", it);
            if (check_plan(P, pack == 1, it, pack ? "chunk, packed" : "chunk", &n_slab, &n_tiles)) return 1;
        }
        ReadsPlan G;
        bool streamed = false;
        CHECK(plan_reads_global(m, off.data(), n_reads, chunk, step, halo, G, &streamed) == 0, "it %d: plan_reads_global failed", it);
        if (check_plan(G, false, it, "global", &n_slab, &n_tiles)) return 1;
    }
    CHECK(n_slab > 0 && n_slab < n_tiles, "%ld of %ld tiles qualify: the check saw only one kind", n_slab, n_tiles);
    printf("%d geometries, %ld tiles, %ld slab tiles, every property holds, no sanitizer report\n", iters, n_tiles, n_slab);
    return 0;
}
