// TEST INFRASTRUCTURE: AddressSanitizer + UBSan harness AND property check for the packed window heads of radian_amd/csrc/plan.hip (PackLayer,
// common.h): the second, compact description of a chunk-mode plan's heads that the exact-fp32 conv kernel indexes HBM with.
// Random models (1..7 blocks, any dilations), read sets, chunk and step, drawn as tests/asan_plan.cpp draws them.  For every conv layer behind
// block 0:
//   * every (head, t < seg_len) appears in exactly one packed row, and every packed row maps back into its head (or is inert);
//   * every row a packed row reads (conv input per live tap, residual) or writes lies inside the activation tensors;
//   * for every class, each tap below tap_lo lies before the window (t - shift < 0) for all of the class's rows: what the kernel leaves out is
//     a product with the zero padding;
//   * the classes tile the launch's packed range behind the stream tiles without overlap, longest K loop first;
//   * the mixed tile (a stream prefix that ends inside a workgroup tile) holds the prefix's last sub-tiles and empty descriptors;
//   * plan_fill_packed writes plan_packed_descs descriptors, no more, and points the lists into the block;
//   * the tile lists (ReadsPlan::tiles / rows) are byte for byte what the planner without packing builds: rebuilt here from the layout rules.
// Block 0's pair, the dense head, and global-mode plans carry no packed form.
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

// the tile lists of a chunk-mode plan by the layout rules, without plan.hip: per layer the streams of all reads in
// 32-row sub-tiles, then the heads of the windows i >= 1 with the layer's head length
static void reference_lists(const Model& m, const std::vector<int64_t>& off, int n_reads, int chunk, int step, int halo, std::vector<TileDesc>* lists,
                            int64_t* rows)
{
    const int nl = 2 * m.nblocks + 1;
    std::vector<int> h_in(nl), h_res(nl), h_out(nl);
    int H = 0;
    for (int b = 0; b < m.nblocks; b++) {
        const int d = m.dil[b];
        h_in[2 * b] = H, h_res[2 * b] = H, h_out[2 * b] = H + 2 * d;
        h_in[2 * b + 1] = H + 2 * d, h_res[2 * b + 1] = H, h_out[2 * b + 1] = H + 4 * d;
        H += 4 * d;
    }
    h_in[nl - 1] = h_res[nl - 1] = h_out[nl - 1] = H;
    auto add = [&](std::vector<TileDesc>& v, int64_t& r, int64_t seg, int64_t src, int len, int in_len, int64_t alt, int alt_in, int alt_res) {
        for (int t0 = 0; t0 < len; t0 += 32) {
            TileDesc td;
            memset(&td, 0, sizeof td);
            td.seg_row = seg, td.src_row = src, td.alt_row = alt, td.t0 = t0, td.seg_len = len, td.in_len = in_len, td.alt_in = alt_in, td.alt_res = alt_res;
            v.push_back(td);
        }
        r += len;
    };
    std::vector<std::vector<TileDesc>> heads(nl);
    int64_t row = 0;
    for (int li = 0; li < nl; li++) lists[li].clear(), rows[li] = 0;
    for (int r = 0; r < n_reads; r++) {
        const int64_t N = off[r + 1] - off[r], stream = row;
        const int nW = rdi::count_windows(N, chunk, step);
        const int pad = (int)(chunk - (N - (int64_t)(nW - 1) * step));
        for (int li = 0; li < nl; li++) add(lists[li], rows[li], stream, off[r], (int)N, (int)N, 0, INT32_MAX, INT32_MAX);
        row += N;
        for (int i = 1; i < nW; i++) {
            const int valid = i < nW - 1 ? chunk : chunk - pad, h = std::min(halo, valid);
            if (h <= 0) continue;
            for (int li = 0; li < nl; li++) {
                const int len = std::min(h_out[li], valid);
                if (len > 0) add(heads[li], rows[li], row, off[r] + (int64_t)i * step, len, valid, stream + (int64_t)i * step, h_in[li], h_res[li]);
            }
            row += h;
        }
    }
    for (int li = 0; li < nl; li++) lists[li].insert(lists[li].end(), heads[li].begin(), heads[li].end());
}

static bool same_desc(const TileDesc& a, const TileDesc& b)
{
    return a.seg_row == b.seg_row && a.src_row == b.src_row && a.alt_row == b.alt_row && a.t0 == b.t0 && a.seg_len == b.seg_len && a.in_len == b.in_len &&
           a.alt_in == b.alt_in && a.alt_res == b.alt_res && a.pad_ == b.pad_;
}

static int check_packed(const Model& m, const std::vector<int64_t>& off, int n_reads, int chunk, int step, int halo, int it, long* packed_rows)
{
    using namespace rdi;
    ReadsPlan P;
    CHECK(plan_reads_chunk(m, off.data(), n_reads, chunk, step, halo, P) == 0, "it %d: plan_reads_chunk failed", it);
    // ---- the old lists are what they were
    std::vector<TileDesc> ref[RD_MAX_LAYERS];
    int64_t ref_rows[RD_MAX_LAYERS];
    reference_lists(m, off, n_reads, chunk, step, halo, ref, ref_rows);
    for (int li = 0; li < P.n_layers; li++) {
        CHECK(P.tiles[li].size() == ref[li].size() && P.rows[li] == ref_rows[li], "it %d layer %d: %zu descriptors / %lld rows, expected %zu / %lld", it, li,
              P.tiles[li].size(), (long long)P.rows[li], ref[li].size(), (long long)ref_rows[li]);
        for (size_t k = 0; k < ref[li].size(); k++) CHECK(same_desc(P.tiles[li][k], ref[li][k]), "it %d layer %d: descriptor %zu differs", it, li, k);
    }
    const size_t n_list = plan_pad_tiles(P);
    for (int li = 0; li < P.n_layers; li++) {
        CHECK(P.tiles[li].size() % 8 == 0 && P.tiles[li].size() >= ref[li].size() && P.tiles[li].size() < ref[li].size() + 8, "it %d layer %d: padding", it, li);
        for (size_t k = 0; k < ref[li].size(); k++) CHECK(same_desc(P.tiles[li][k], ref[li][k]), "it %d layer %d: descriptor %zu differs after padding", it, li, k);
    }
    // ---- the packed block
    const size_t n_pack = plan_packed_descs(P);
    std::vector<TileDesc> dev(n_list + n_pack + 1), host(n_list + n_pack + 1);
    memset((void*)&host[n_list + n_pack], 0x5a, sizeof(TileDesc));
    const TileDesc guard = host[n_list + n_pack];
    TileLists tl;
    memset((void*)&tl, 0x77, sizeof tl);
    CHECK(plan_fill_lists(P, dev.data(), host.data(), tl) == n_list, "it %d: list descriptors", it);
    for (int li = 0; li < RD_MAX_LAYERS; li++) CHECK(tl.head_segs[li] == nullptr && tl.pack[li].n_tiles == 0, "it %d layer %d: plan_fill_lists leaves a layer packed", it, li);
    CHECK(plan_fill_packed(P, dev.data() + n_list, host.data() + n_list, tl) == n_pack, "it %d: packed descriptors written != %zu", it, n_pack);
    CHECK(memcmp(&host[n_list + n_pack], &guard, sizeof(TileDesc)) == 0, "it %d: written beyond the packed block", it);
    for (int li = 0; li < P.n_layers; li++)
        CHECK(P.tiles[li].empty() || memcmp(&host[tl.d[li] - dev.data()], P.tiles[li].data(), P.tiles[li].size() * sizeof(TileDesc)) == 0, "it %d layer %d: list bytes", it, li);
    size_t next = n_list;
    for (int li = 0; li < RD_MAX_LAYERS; li++) {
        const PackLayer& pk = tl.pack[li];
        const bool handled = li >= 2 && li < P.n_layers - 1;
        // the heads of the layer, from the list
        std::vector<TileDesc> heads;
        size_t nS = 0;
        if (li < P.n_layers) {
            for (const TileDesc& d : ref[li]) {
                if (d.alt_in == INT32_MAX && d.alt_res == INT32_MAX) nS++;
                else if (d.t0 == 0) heads.push_back(d);
            }
        }
        if (!handled || heads.empty()) {
            CHECK(pk.n_tiles == 0 && tl.head_segs[li] == nullptr, "it %d layer %d: packed without heads to pack", it, li);
            continue;
        }
        CHECK(pk.n_tiles > 0 && tl.head_segs[li] != nullptr, "it %d layer %d: %zu heads not packed", it, li, heads.size());
        const size_t o = (size_t)(tl.head_segs[li] - dev.data());
        const size_t n_own = heads.size() + (pk.mixed ? 4 : 0);
        CHECK(o == next && o + n_own <= n_list + n_pack, "it %d layer %d: head_segs at %zu, expected %zu", it, li, o, next);
        next = o + n_own;
        const TileDesc* hs = &host[o];
        CHECK(pk.n_heads == (int)heads.size(), "it %d layer %d: %d heads, expected %zu", it, li, pk.n_heads, heads.size());
        for (size_t w = 0; w < heads.size(); w++) CHECK(same_desc(hs[w], heads[w]), "it %d layer %d: head %zu differs from its t0 == 0 descriptor", it, li, w);
        // stream prefix and mixed tile
        CHECK(pk.n_stream_tiles == (int)((nS + 3) / 4) && pk.mixed == (nS % 4 ? 1 : 0), "it %d layer %d: %zu stream sub-tiles, %d tiles, mixed %d", it, li, nS, pk.n_stream_tiles, pk.mixed);
        if (pk.mixed)
            for (size_t j = 0; j < 4; j++) {
                const size_t k = nS / 4 * 4 + j;
                const TileDesc& d = hs[heads.size() + j];
                if (k < nS) CHECK(same_desc(d, ref[li][k]), "it %d layer %d: mixed tile sub-tile %zu", it, li, j);
                else CHECK(d.seg_len == 0 && d.t0 == 0 && d.in_len == 0, "it %d layer %d: mixed tile sub-tile %zu not empty", it, li, j);
            }
        // classes: C, B, A behind the stream tiles
        const int d = m.dil[li / 2];
        int tile = pk.n_stream_tiles;
        int hmax = 1;
        for (const TileDesc& h : heads) hmax = std::max(hmax, h.seg_len);
        std::vector<uint8_t> seen(heads.size() * (size_t)hmax, 0);   // [head][t] -> times packed
        int64_t n_seen = 0;
        int t_next = -1;
        for (int c = 0; c < 3; c++) {
            const PackClass& pc = pk.cls[c];
            CHECK(pc.tap_lo == c && pc.first_tile == tile && pc.n_tiles >= 0 && pc.L >= 0 && pc.t_lo >= 0, "it %d layer %d class %d: header", it, li, c);
            CHECK((int64_t)pc.n_tiles * 128 >= (int64_t)pk.n_heads * pc.L && (int64_t)pc.n_tiles * 128 < (int64_t)pk.n_heads * pc.L + 128, "it %d layer %d class %d: %d tiles for %d x %d rows", it, li, c, pc.n_tiles, pk.n_heads, pc.L);
            CHECK(pc.n_tiles == 0 || pc.L > 0, "it %d layer %d class %d: tiles of an empty class", it, li, c);
            tile += pc.n_tiles;
            if (c > 0) CHECK(pc.t_lo + pc.L == t_next, "it %d layer %d class %d: time steps [%d, %d) do not meet the class before at %d", it, li, c, pc.t_lo, pc.t_lo + pc.L, t_next);
            t_next = pc.t_lo;
            // taps below tap_lo lie before the window for every row of the class
            for (int tap = 0; tap < pc.tap_lo; tap++)
                CHECK(pc.L == 0 || pc.t_lo + pc.L - 1 - (2 - tap) * d < 0, "it %d layer %d class %d: tap %d is live at t = %d", it, li, c, tap, pc.t_lo + pc.L - 1);
            for (int64_t p = 0; p < (int64_t)pc.n_tiles * 128; p++) {
                const int64_t w = p / pc.L;
                const int t = pc.t_lo + (int)(p % pc.L);
                if (w >= pk.n_heads) continue;   // inert: past the last head
                const TileDesc& h = hs[w];
                if (t >= h.seg_len) continue;    // inert: a last window shorter than the class's time step
                CHECK(seen[(size_t)w * hmax + t] == 0, "it %d layer %d class %d: head %lld step %d packed twice", it, li, c, (long long)w, t);
                seen[(size_t)w * hmax + t] = 1;
                n_seen++;
                (*packed_rows)++;
                // writes
                CHECK(h.seg_row >= 0 && h.seg_row + t < P.total_rows, "it %d layer %d class %d: row %lld written of %lld", it, li, c, (long long)(h.seg_row + t), (long long)P.total_rows);
                // conv input, per live tap
                for (int tap = pc.tap_lo; tap < 3; tap++) {
                    const int u = t - (2 - tap) * d;
                    if (u < 0 || u >= h.in_len) continue;   // zero row
                    const int64_t src = (u < h.alt_in ? h.seg_row : h.alt_row) + u;
                    CHECK(src >= 0 && src < P.total_rows, "it %d layer %d class %d: input row %lld of %lld", it, li, c, (long long)src, (long long)P.total_rows);
                }
                const int64_t res = (t < h.alt_res ? h.seg_row : h.alt_row) + t;
                CHECK(res >= 0 && res < P.total_rows, "it %d layer %d class %d: residual row %lld of %lld", it, li, c, (long long)res, (long long)P.total_rows);
            }
        }
        CHECK(t_next == 0, "it %d layer %d: the classes start at time step %d", it, li, t_next);
        CHECK(tile == pk.n_tiles, "it %d layer %d: %d tiles in the launch, classes end at %d", it, li, pk.n_tiles, tile);
        for (size_t w = 0; w < heads.size(); w++)
            for (int t = 0; t < heads[w].seg_len; t++) CHECK(seen[w * hmax + t] == 1, "it %d layer %d: head %zu step %d not packed", it, li, w, t);
        int64_t total = 0;
        for (const TileDesc& h : heads) total += h.seg_len;
        CHECK(n_seen == total, "it %d layer %d: %lld packed rows for %lld head rows", it, li, (long long)n_seen, (long long)total);
    }
    CHECK(next == n_list + n_pack, "it %d: head_segs cover %zu of %zu descriptors", it, next - n_list, n_pack);
    // ---- global mode: nothing packed
    ReadsPlan G;
    bool streamed = false;
    CHECK(plan_reads_global(m, off.data(), n_reads, chunk, step, halo, G, &streamed) == 0, "it %d: plan_reads_global failed", it);
    CHECK(plan_packed_descs(G) == 0, "it %d: a global-mode plan with a packed block", it);
    for (int li = 0; li < RD_MAX_LAYERS; li++) CHECK(G.pack[li].n_tiles == 0, "it %d layer %d: global mode packed", it, li);
    return 0;
}

int main(int argc, char** argv)
{
    const int iters = argc > 1 ? atoi(argv[1]) : 5000;
    std::mt19937_64 rng(29);
    long packed_rows = 0;
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
            off[r + 1] = off[r] + N;
        }
        if (check_packed(m, off, n_reads, chunk, step, halo, it, &packed_rows)) return 1;
    }
    printf("%d geometries, %ld packed rows, every property holds, no sanitizer report\n", iters, packed_rows);
    return 0;
}
