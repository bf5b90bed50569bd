// plan.hip -- host-side geometry of the reads-level paths: see plan.h.
#include "plan.h"

#include <string.h>

namespace rdi {

int64_t assembled_rows(int nW, int T, int pad, int step)
{
    int64_t N = 0;
    for (int i = 0; i < nW; i++) {
        int rows = (i == nW - 1) ? T - pad : T;
        int64_t end = (int64_t)i * step + rows;
        if (rows > 0 && end > N) N = end;
    }
    return N;
}

int assembled_is_f64(int nW, int T, int pad, int step)
{
    // some time step is covered twice <=> a window i >= 1 with rows starts inside window i-1
    if (step >= T) return 0;
    if (nW >= 3) return 1;
    if (nW == 2 && T - pad > 0) return 1;
    return 0;
}

int64_t classify_reads(const int32_t* win_off, const int32_t* pad, int n_reads, int T, int step, int64_t rows64, std::vector<ReadRows>& out)
{
    out.resize(n_reads);
    for (int r = 0; r < n_reads; r++) {
        const int nW = win_off[r + 1] - win_off[r];
        out[r].N = assembled_rows(nW, T, pad[r], step);
        out[r].is64 = assembled_is_f64(nW, T, pad[r], step);
        out[r].row64 = rows64;
        if (out[r].is64) rows64 += out[r].N;
    }
    return rows64;
}

void add_segment(std::vector<TileDesc>& list, int64_t& rows, int64_t seg_row, int64_t src_row, int len, int in_len,
                 int64_t alt_row = 0, int alt_in = INT32_MAX, int alt_res = INT32_MAX)
{
    for (int t0 = 0; t0 < len; t0 += 32) {   // 32-row sub-tiles; four of them (of any segments) make a workgroup tile
        TileDesc td;
        td.seg_row = seg_row;
        td.src_row = src_row;
        td.alt_row = alt_row;
        td.t0 = t0;
        td.seg_len = len;
        td.in_len = in_len;
        td.alt_in = alt_in;
        td.alt_res = alt_res;
        td.pad_ = 0;
        list.push_back(td);
    }
    rows += len;
}

// Rows of a head that differ from the stream, per tensor: the signal has none; a k=3 conv of dilation d adds 2d.
struct LayerHalo {
    int h_in, h_res, h_out;
};
void layer_halos(const Model& m, LayerHalo* lh)
{
    int H = 0;  // halo of the block input
    for (int b = 0; b < m.nblocks; b++) {
        const int d = m.dil[b];
        lh[2 * b] = {H, H, H + 2 * d};               // first conv (block 0: from the raw signal)
        lh[2 * b + 1] = {H + 2 * d, H, H + 4 * d};   // second conv, residual = block input
        H += 4 * d;
    }
    lh[2 * m.nblocks] = {H, H, H};                   // dense head
}

// The packed form of a layer's heads (PackLayer, common.h): n_stream sub-tiles of streams are in `list` so far, `heads` are the head
// sub-tiles that will follow them.  d = the layer's dilation, h = its head length (capped at the chunk length: no head is longer).
void pack_layer_heads(const std::vector<TileDesc>& list, const std::vector<TileDesc>& heads, int d, int h, std::vector<TileDesc>& segs, PackLayer& pk)
{
    pk = PackLayer();
    segs.clear();
    for (const TileDesc& td : heads)
        if (td.t0 == 0) segs.push_back(td);
    const int64_t nH = (int64_t)segs.size();
    if (nH == 0 || nH * h >= ((int64_t)1 << 30)) {   // (packed rows are indexed with 32 bits; such a batch does not fit the row space anyway)
        segs.clear();
        return;
    }
    const size_t nS = list.size();
    pk.n_heads = (int32_t)nH;
    pk.n_stream_tiles = (int32_t)((nS + 3) / 4);
    pk.mixed = nS % 4 ? 1 : 0;
    if (pk.mixed) {
        for (size_t j = nS / 4 * 4; j < nS / 4 * 4 + 4; j++) {
            TileDesc e = {};
            e.alt_in = e.alt_res = INT32_MAX;
            segs.push_back(j < nS ? list[j] : e);
        }
    }
    const int t1 = d < h ? d : h, t2 = 2 * d < h ? 2 * d : h;
    const int lo[3] = {t2, t1, 0}, hi[3] = {h, t2, t1};   // C, B, A: longest K loop first
    int32_t tile = pk.n_stream_tiles;
    for (int c = 0; c < 3; c++) {
        PackClass& pc = pk.cls[c];
        pc.t_lo = lo[c];
        pc.L = hi[c] - lo[c];
        pc.tap_lo = c;
        pc.first_tile = tile;
        pc.n_tiles = (int32_t)((nH * pc.L + 127) / 128);
        tile += pc.n_tiles;
    }
    pk.n_tiles = tile;
}

// chunk mode: one stream per read + one head per window i >= 1; per-layer head lengths
int plan_reads_chunk(const Model& m, const int64_t* read_off, int n_reads, int chunk, int step, int halo, ReadsPlan& P)
{
    LayerHalo lh[RD_MAX_LAYERS];
    layer_halos(m, lh);
    P.n_layers = 2 * m.nblocks + 1;
    P.per_layer = true;
    int64_t row = 0;
    P.read_win_off.assign(1, 0);
    // A layer's tile list holds the streams of ALL reads first, then the heads: workgroups are dispatched in list order as
    // slots free up, so the full 128-row stream tiles fill the rounds and the short head tiles (few rows, waves without rows
    // skip their MFMAs) make up the last, partial round -- longest-processing-time-first.  (Tiles of one launch are
    // independent: a head reads its later rows from the layer's INPUT tensor.)
    std::vector<TileDesc> heads[RD_MAX_LAYERS];
    for (int r = 0; r < n_reads; r++) {
        const int64_t N = read_off[r + 1] - read_off[r];
        RD_REQUIRE(N >= 1, "read %d is empty", r);
        RD_REQUIRE(N < INT32_MAX, "read %d too long", r);
        const WindowGeom g = window_geom(N, chunk, step);
        const int64_t stream_row = row;
        P.read_row.push_back(stream_row);
        for (int li = 0; li < P.n_layers; li++) add_segment(P.tiles[li], P.rows[li], stream_row, read_off[r], (int)N, (int)N);
        row += N;
        for (int i = 0; i < g.nW; i++) {
            const int valid = (i < g.nW - 1) ? chunk : chunk - g.pad;
            const int h = (i == 0) ? 0 : (halo < valid ? halo : valid);
            int64_t o1 = stream_row + (int64_t)i * step;
            if (h > 0) {
                o1 = row;
                const int64_t alt = stream_row + (int64_t)i * step;
                for (int li = 0; li < P.n_layers; li++) {
                    const int len = lh[li].h_out < valid ? lh[li].h_out : valid;   // rows of this head the layer must produce
                    if (len > 0)
                        add_segment(heads[li], P.rows[li], row, read_off[r] + (int64_t)i * step, len, valid, alt, lh[li].h_in, lh[li].h_res);
                }
                row += h;
            }
            P.off1.push_back(o1);
            P.off2.push_back(stream_row + (int64_t)i * step);
            P.split.push_back(h);
            P.valid.push_back(valid);
        }
        P.n_windows += g.nW;
        P.read_win_off.push_back(P.n_windows);
    }
    for (int li = 2; li < P.n_layers - 1; li++)   // (block 0's pair -- the fused first-conv launch -- and the dense head keep their head tiles)
        pack_layer_heads(P.tiles[li], heads[li], m.dil[li / 2], lh[li].h_out < chunk ? lh[li].h_out : chunk, P.head_segs[li], P.pack[li]);
    for (int li = 0; li < P.n_layers; li++) P.tiles[li].insert(P.tiles[li].end(), heads[li].begin(), heads[li].end());
    P.total_rows = row;
    return RD_OK;
}

// global mode: one stream per read when the geometry allows it, else per-window segments in a uniform row layout
int plan_reads_global(const Model& m, const int64_t* read_off, int n_reads, int chunk, int step, int halo, ReadsPlan& P, bool* streamed)
{
    const bool st = step <= chunk - halo;
    *streamed = st;
    P.n_layers = 2 * m.nblocks + 1;
    P.per_layer = false;
    int64_t row = 0;
    P.read_win_off.assign(1, 0);
    for (int r = 0; r < n_reads; r++) {
        const int64_t N = read_off[r + 1] - read_off[r];
        RD_REQUIRE(N >= 1, "read %d is empty", r);
        RD_REQUIRE(N < INT32_MAX, "read %d too long", r);
        const WindowGeom g = window_geom(N, chunk, step);
        P.read_row.push_back(row);
        if (st) {
            add_segment(P.tiles[0], P.rows[0], row, read_off[r], (int)N, (int)N);
            row += N;
        } else {
            for (int i = 0; i < g.nW; i++) {
                const int valid = (i < g.nW - 1) ? chunk : chunk - g.pad;
                if (valid > 0) add_segment(P.tiles[0], P.rows[0], row + (int64_t)i * chunk, read_off[r] + (int64_t)i * step, valid, valid);
            }
            row += (int64_t)g.nW * chunk;
        }
        P.valid.push_back(g.pad);   // per read: the pad of its last window
        P.n_windows += g.nW;
        P.read_win_off.push_back(P.n_windows);
    }
    P.total_rows = row;
    return RD_OK;
}

size_t plan_pad_tiles(ReadsPlan& P)
{
    size_t total = 0;
    for (int li = 0; li < P.n_layers; li++)
        if (P.per_layer || li == 0) {
            std::vector<TileDesc>& v = P.tiles[li];
            while (v.size() % 8) {
                TileDesc e = {};
                e.alt_in = e.alt_res = INT32_MAX;
                v.push_back(e);
            }
            total += v.size();
        }
    return total;
}

bool PlanKey::matches(const Model& m, const int64_t* read_off, int n_reads, int chunk_, int step_, int mode_, int halo_) const
{
    if (!valid || chunk != chunk_ || step != step_ || mode != mode_ || halo != halo_ || nblocks != m.nblocks || read_off[0] != 0 ||
        lens.size() != (size_t)n_reads)
        return false;
    for (int b = 0; b < m.nblocks; b++)
        if (dil[b] != m.dil[b]) return false;
    for (int r = 0; r < n_reads; r++)
        if (lens[r] != read_off[r + 1] - read_off[r]) return false;
    return true;
}

int PlanKey::rebuild(const Model& m, const int64_t* read_off, int n_reads, int chunk_, int step_, int mode_, int halo_, ReadsPlan& P, bool* streamed,
                     size_t* n_desc)
{
    invalidate();
    P = ReadsPlan();
    int rc = mode_ == 0 ? plan_reads_chunk(m, read_off, n_reads, chunk_, step_, halo_, P) : plan_reads_global(m, read_off, n_reads, chunk_, step_, halo_, P, streamed);
    if (rc) return rc;
    *n_desc = plan_pad_tiles(P);
    chunk = chunk_;
    step = step_;
    mode = mode_;
    halo = halo_;
    nblocks = m.nblocks;
    for (int b = 0; b < RD_MAX_BLOCKS; b++) dil[b] = b < m.nblocks ? m.dil[b] : 0;
    lens.resize(n_reads);
    for (int r = 0; r < n_reads; r++) lens[r] = read_off[r + 1] - read_off[r];
    return RD_OK;
}

size_t plan_fill_lists(const ReadsPlan& P, const TileDesc* d_base, TileDesc* h_dst, TileLists& lists)
{
    size_t off = 0;
    for (int li = 0; li < RD_MAX_LAYERS; li++) {
        lists.d[li] = nullptr;
        lists.n[li] = 0;
        lists.rows[li] = 0;
        lists.head_segs[li] = nullptr;
        lists.pack[li] = PackLayer();
        lists.slab[li] = lists.slab_stream[li] = 0;
    }
    for (int li = 0; li < P.n_layers; li++) {
        if (P.per_layer || li == 0) {
            const std::vector<TileDesc>& v = P.tiles[li];
            if (!v.empty()) memcpy(h_dst + off, v.data(), v.size() * sizeof(TileDesc));
            lists.d[li] = d_base + off;
            lists.n[li] = (int)(v.size() / 4);
            lists.rows[li] = P.rows[li];
            lists.slab[li] = rd_count_slab_tiles(v.data(), v.size() / 4);
            off += v.size();
        } else {
            lists.d[li] = lists.d[0];
            lists.n[li] = lists.n[0];
            lists.rows[li] = lists.rows[0];
            lists.slab[li] = lists.slab[0];
        }
    }
    return off;
}

size_t plan_packed_descs(const ReadsPlan& P)
{
    size_t n = 0;
    for (int li = 0; li < RD_MAX_LAYERS; li++) n += P.head_segs[li].size();
    return n;
}

size_t plan_fill_packed(const ReadsPlan& P, const TileDesc* d_base, TileDesc* h_dst, TileLists& lists)
{
    size_t off = 0;
    for (int li = 0; li < RD_MAX_LAYERS; li++) {
        const std::vector<TileDesc>& v = P.head_segs[li];
        lists.head_segs[li] = nullptr;
        lists.pack[li] = PackLayer();
        lists.slab_stream[li] = 0;
        if (v.empty() || P.pack[li].n_tiles == 0) continue;
        memcpy(h_dst + off, v.data(), v.size() * sizeof(TileDesc));
        lists.head_segs[li] = d_base + off;
        lists.pack[li] = P.pack[li];
        lists.slab_stream[li] = rd_count_slab_tiles(P.tiles[li].data(), (size_t)(P.pack[li].n_stream_tiles - P.pack[li].mixed));
        off += v.size();
    }
    return off;
}

int pinned_reserve(void** p, size_t* cap, size_t bytes)
{
    if (bytes <= *cap) return RD_OK;
    if (*p) (void)hipHostFree(*p);
    *p = nullptr;
    *cap = 0;
    size_t want = align_up(bytes + bytes / 8, 1 << 16);
    RD_HIP(hipHostMalloc(p, want, hipHostMallocDefault));
    *cap = want;
    return RD_OK;
}

}  // namespace rdi
