// plan.h -- host-side geometry of the reads-level paths (internal; shared by api.hip and pipe_reads.hip; plain host C++):
// windows of a read (preprocess.py:4-22), assembled length / dtype of a read (matrix_assembly.py:6-53), and the
// segment / tile-descriptor plans of the streamed forward.
#pragma once
#include "common.h"

namespace rdi {

int64_t assembled_rows(int nW, int T, int pad, int step);
int assembled_is_f64(int nW, int T, int pad, int step);

// One read of a global-mode batch as the decoder sees it: N assembled rows -- float64 rows, from row row64 of the batch's float64
// matrix, when some time step is covered twice; the float32 rows of the forward themselves otherwise.
struct ReadRows {
    int64_t N, row64;
    int is64;
};
// The reads of a batch (read r: windows win_off[r] .. win_off[r+1], pad[r] = the pad of its last window), their float64 rows
// behind the rows64 rows the matrix holds already; -> the rows of the matrix with this batch
int64_t classify_reads(const int32_t* win_off, const int32_t* pad, int n_reads, int T, int step, int64_t rows64, std::vector<ReadRows>& out);

inline int count_windows(int64_t N, int chunk, int step) { return (N < chunk ? 0 : (int)((N - chunk) / step) + 1) + 1; }

struct WindowGeom {
    int nW, pad;
};
inline WindowGeom window_geom(int64_t N, int chunk, int step)
{
    WindowGeom g;
    g.nW = count_windows(N, chunk, step);
    const int64_t last_start = (int64_t)(g.nW - 1) * step;
    g.pad = (int)(chunk - (N - last_start));   // >= 1 always (preprocess.py:17-19)
    return g;
}

struct ReadsPlan {
    int n_layers = 0;                       // 2 * nblocks + 1
    bool per_layer = false;                 // false: tiles[0] serves every layer
    std::vector<TileDesc> tiles[RD_MAX_LAYERS];
    int64_t rows[RD_MAX_LAYERS] = {0};      // time steps evaluated per layer
    // per decoded sequence (chunk mode: window; global mode: read)
    std::vector<int64_t> off1, off2;
    std::vector<int32_t> split, valid;
    std::vector<int32_t> read_win_off;   // n_reads + 1
    std::vector<int64_t> read_row;       // first stream row of each read
    int64_t total_rows = 0;
    int n_windows = 0;
    // Packed window heads (chunk mode; PackLayer, common.h) of every conv layer behind block 0, beside the head sub-tiles of `tiles`
    // (which stay complete: the f16x3 / bf16x3 kernels and rd_set_head_pack 0 run them).  head_segs[li]: one descriptor per head of the
    // layer -- its t0 == 0 sub-tile's -- then, where pack[li].mixed, the four descriptors of the workgroup tile the stream prefix ends in.
    std::vector<TileDesc> head_segs[RD_MAX_LAYERS];
    PackLayer pack[RD_MAX_LAYERS] = {};
};

// chunk mode: one stream per read + one head per window i >= 1; per-layer head lengths
int plan_reads_chunk(const Model& m, const int64_t* read_off, int n_reads, int chunk, int step, int halo, ReadsPlan& P);
// global mode: one stream per read when the geometry allows it (*streamed), else per-window segments
int plan_reads_global(const Model& m, const int64_t* read_off, int n_reads, int chunk, int step, int halo, ReadsPlan& P, bool* streamed);
// pads every tile list the plan uses to whole workgroup tiles (eight sub-tiles: the bf16x3 kernel's tile); -> descriptors in total
size_t plan_pad_tiles(ReadsPlan& P);

// What a cached plan was built for: a batch with the same key has the same plan and the same descriptors.  (Per-layer head
// lengths depend on every block's dilation, not only on their sum.)
struct PlanKey {
    bool valid = false;   // set by the owner once the descriptors of the rebuilt plan are on the device
    int chunk = -1, step = -1, mode = -1, halo = -1, nblocks = -1;
    int dil[RD_MAX_BLOCKS] = {0};
    std::vector<int64_t> lens;
    bool matches(const Model& m, const int64_t* read_off, int n_reads, int chunk_, int step_, int mode_, int halo_) const;
    void invalidate() { valid = false; }   // a failure between rebuild and upload must not leave a half-built plan reachable
    // voids the key, plans the batch into P (mode 0: chunk, 1: global -> *streamed) and pads its tile lists to *n_desc descriptors; the
    // key then describes the batch but stays invalid
    int rebuild(const Model& m, const int64_t* read_off, int n_reads, int chunk_, int step_, int mode_, int halo_, ReadsPlan& P, bool* streamed,
                size_t* n_desc);
};
// The descriptors of a padded plan, list after list, to h_dst, and `lists` pointing at the same places from d_base (layers
// without a list of their own share list 0); -> descriptors written
size_t plan_fill_lists(const ReadsPlan& P, const TileDesc* d_base, TileDesc* h_dst, TileLists& lists);

// The packed block of a plan: plan_packed_descs(P) descriptors, which plan_fill_packed writes to h_dst and points `lists` at from d_base
// (the device address of h_dst[0]: the owners put the block behind the descriptor block plan_fill_lists filled, in the same upload);
// -> descriptors written.  Call it after plan_fill_lists, which marks every layer of `lists` unpacked.
size_t plan_packed_descs(const ReadsPlan& P);
size_t plan_fill_packed(const ReadsPlan& P, const TileDesc* d_base, TileDesc* h_dst, TileLists& lists);

// api.hip: what every reads-level entry point requires of its arguments (RD_ERR_ARG), then loaded weights (RD_ERR_STATE)
int rd_check_reads_args(rd_ctx* ctx, const void* signal, const int64_t* read_off, int n_reads, int chunk_len, int step, int W);

// grow-only pinned host buffer
int pinned_reserve(void** p, size_t* cap, size_t bytes);

}  // namespace rdi
