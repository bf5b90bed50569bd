// common.h -- shared declarations for the radian_hip library (gfx950 / MI355X only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <string>
#include <vector>

#include "carve.h"
#include "polya_rules.h"

#define RD_OK 0
#define RD_ERR_ARG (-1)
#define RD_ERR_HIP (-2)
#define RD_ERR_STATE (-3)
#define RD_ERR_NOMEM (-4)
#define RD_ERR_RCCL (-5)

void rd_set_error(const char* fmt, ...);

#define RD_HIP(expr)                                                                                   \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess) {                                                                        \
            rd_set_error("%s:%d: %s failed: %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e));   \
            return RD_ERR_HIP;                                                                         \
        }                                                                                              \
    } while (0)

#define RD_REQUIRE(cond, ...)                                                                          \
    do {                                                                                               \
        if (!(cond)) {                                                                                 \
            rd_set_error(__VA_ARGS__);                                                                 \
            return RD_ERR_ARG;                                                                         \
        }                                                                                              \
    } while (0)

// A grow-only device buffer (workspace); never shrinks, freed with the context.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    int reserve(size_t bytes);
    int reserve_exact(size_t bytes, const char* who);   // exactly `bytes` when it has to grow (a budgeted workspace); the error names `who`
    void release();
    template <typename T> T* as() const { return (T*)p; }
};
// A launch's members gathered from the host array src (elements of elem_bytes; member i: src_off[members[i]] .. src_off[members[i] + 1]) into
// the dense device array dst, member i at element off[i] (rd_gather_offsets, carve.h): one copy per run of members that are contiguous in
// the source (rd_gather_runs), none for a run without elements.  Queues on st; the caller keeps src alive until the stream has run.
int rd_gather_h2d(hipStream_t st, void* dst, const void* src, size_t elem_bytes, const int64_t* src_off, const int32_t* members, int n,
                  const int64_t* off);
// a stage's block (carve.h): a dry pass of the stage's layout sizes buf, a second pass carves it
template <typename Layout> inline int rd_carve(DevBuf& buf, Layout layout)
{
    Carve dry;
    layout(dry);
    if (buf.reserve(dry.at)) return RD_ERR_NOMEM;
    Carve c(buf.p);
    layout(c);
    return RD_OK;
}
// a launch carved into ws_align (whose size comes from the entry point's byte formulas, not from the layout) must have stayed inside it
inline int rd_carve_check(const char* who, const Carve& c, size_t cap)
{
    if (c.fits(cap)) return RD_OK;
    rd_set_error("%s: internal workspace accounting (%zu > %zu)", who, c.at, cap);
    return RD_ERR_STATE;
}

// Model geometry: radian/models/sig2seq.yaml:34-49
constexpr int RD_C = 256;      // tcn.nb_filters
constexpr int RD_K = 3;        // tcn.kernel_size
constexpr int RD_H = 128;      // relu_units
constexpr int RD_NCLS = 5;     // softmax_units (A,C,G,T,blank)
constexpr int RD_MAX_BLOCKS = 16;

struct Model {
    bool loaded = false;
    int nblocks = 0;
    int dil[RD_MAX_BLOCKS] = {0};
    // device tensors (packed layouts, see forward.hip)
    float* sink = nullptr;      // 1024 floats, write-only scratch
    float* w_in = nullptr;      // block0.conv0 kernel [3][256]
    float* b_in = nullptr;      // [256]
    float* w_match = nullptr;   // [256]
    float* b_match = nullptr;   // [256]
    float* w_conv[2 * RD_MAX_BLOCKS] = {nullptr};  // packed [48 chunks][256 co][16 k]; index 2*blk+which (blk0.conv0 unused)
    float* b_conv[2 * RD_MAX_BLOCKS] = {nullptr};  // [256]
    float* w_d1 = nullptr;      // packed like conv, K=256: [8 chunks][128 co][32 k]
    float* b_d1 = nullptr;      // [128]
    // split-f16 images of the same tensors (forward.hip, f16x3 section): [chunk][co][hi 32 | lo 32] halves, scaled by 1/inv_scale
    void* ws_conv[2 * RD_MAX_BLOCKS] = {nullptr};
    float inv_scale[2 * RD_MAX_BLOCKS] = {0};
    void* ws_d1 = nullptr;
    float inv_scale_d1 = 0.f;
    // three-term bf16 images (forward.hip, bf16x3 section): [chunk][co][6 slots x 8 bf16], slots swizzled, unscaled
    void* w3_conv[2 * RD_MAX_BLOCKS] = {nullptr};
    void* w3_d1 = nullptr;
    float* w_d2 = nullptr;      // [128][5] (Keras layout)
    float* b_d2 = nullptr;      // [5]
    DevBuf storage;
    // rd_load_weights: every conv kernel weight is finite and no conv bias is -0.0, so leaving out a product with a zero-padding row gives results
    // equal under IEEE comparison (an accumulator that reaches -0.0 by underflow may keep its sign)
    // and the packed window heads (forward.hip) may skip it.  False for weights the host has not seen (after training, on a broadcast's receiver).
    bool pack_ok = false;
    bool split_stale = false;   // training rewrote the fp32 images (train.hip): the f16x3 / bf16x3 images are rebuilt before their next use
};

struct LM {
    bool loaded = false;
    int k = 0;                      // context length (labels)
    int table_order = 0;            // the table has 4^table_order rows (= k unless hashed)
    int hashed = 0;                 // 1: long-context mode, row = hash(context) (decode.hip)
    double* table = nullptr;        // [4^table_order][4] device
    double* d_entropy = nullptr;    // [4^k] device: entropy of each context's distribution (glibc log, computed at load)
    int sparse = 0;                 // 1: some contexts are absent (rows of NaN at rd_load_lm): d_missing has their bits
    uint32_t* d_missing = nullptr;  // bit ctx: the model does not hold this context (decode.py:83 raises KeyError on it)
    uint32_t* gate_bits = nullptr;  // bit ctx: d_entropy[ctx] < gate_r_thr
    double gate_r_thr = 0.0;
    bool gate_valid = false;
    DevBuf storage, gate_storage;   // storage = table, d_entropy, d_missing (one RCCL broadcast)
};

// One 32-row SUB-TILE of the forward: rows [t0, t0+32) of a segment whose time step 0 is global row seg_row; a
// workgroup tile is four consecutive descriptors of a layer's list (any mix of segments; lists are padded with empty ones).
// A segment is a window, a whole read (the "stream"), or the first rows of a window (a "head").  Heads only hold the
// rows that see their window's own zero left-padding; every later row equals the read's stream row, so a head's
// reads of rows t >= alt_in (conv input) / alt_res (residual) are redirected to global row alt_row + t.
struct TileDesc {
    int64_t seg_row;   // global row (activations / probabilities) of the segment's time step 0
    int64_t src_row;   // index of the segment's sample 0 in the signal buffer
    int64_t alt_row;   // global row of the stream row that equals this segment's time step 0
    int32_t t0;        // first time step of this sub-tile
    int32_t seg_len;   // time steps this layer computes and stores for the segment
    int32_t in_len;    // time steps that exist as input (zero beyond)
    int32_t alt_in;    // conv-input rows t >= alt_in come from alt_row + t   (INT32_MAX: never)
    int32_t alt_res;   // residual rows  t >= alt_res come from alt_row + t
    int32_t pad_;
};

// Slab tiles (the exact-fp32 conv kernel of the product shape, layers behind block 0 of dilation <= RD_SLAB_DMAX): a
// workgroup tile d[0..3] whose four sub-tiles are consecutive interior pieces of ONE segment and whose every conv-input and residual row
// is the segment's own (nothing redirected to alt_row).  The three taps of such a tile read one run of 128 + 2 dil rows of the segment (or
// the zero padding in front of it), which the kernel stages once per input-channel slice.  Everything else -- a segment's last partial
// tile, head tiles, the mixed tile, padding -- runs the per-tap staging.  The kernel decides per tile with this test; the planner counts
// with it (TileLists::slab).
constexpr int RD_SLAB_DMAX = 32;
// (sub-tile j, descriptor dj, of a tile whose sub-tile 0 is d0; without branches: the kernel evaluates it once per lane)
__host__ __device__ inline bool rd_slab_sub(const TileDesc& d0, const TileDesc& dj, int j)
{
    const int64_t end = (int64_t)d0.t0 + 128;
    return (d0.t0 >= 0) & (end <= d0.seg_len) & (end <= d0.in_len) & (dj.seg_row == d0.seg_row) & (dj.t0 == d0.t0 + 32 * j) &
           (dj.seg_len == d0.seg_len) & (dj.in_len == d0.in_len) & (dj.alt_in >= end) & (dj.alt_res >= end);
}
inline bool rd_slab_tile(const TileDesc* d)
{
    return rd_slab_sub(d[0], d[0], 0) && rd_slab_sub(d[0], d[1], 1) && rd_slab_sub(d[0], d[2], 2) && rd_slab_sub(d[0], d[3], 3);
}
// workgroup tiles [0, n_tiles) of a host copy of a tile list that are slab tiles
inline int rd_count_slab_tiles(const TileDesc* list, size_t n_tiles)
{
    int n = 0;
    for (size_t i = 0; i < n_tiles; i++) n += rd_slab_tile(list + 4 * i) ? 1 : 0;
    return n;
}

// per-layer tile lists: index 0 = block-0 first conv (C_in = 1); 2b = first conv of block b >= 1; 2b+1 = second conv of
// block b; 2*nblocks = dense head.  Uniform windows and streams use one list for every layer.
constexpr int RD_MAX_LAYERS = 2 * 16 + 1;

// Packed window heads (chunk-mode plans, exact-fp32 conv kernel only).  The head rows of a layer of dilation d and head
// length h, sorted by what they read of their window's zero left-padding: class A = time steps [0, d) (only tap 2, shift 0, is live),
// B = [d, 2d) (taps 1 and 2), C = [2d, h) (all taps).  Packed row p of a class is time step t_lo + p % L of head p / L (a TileDesc of
// the layer's head_segs: the head's t0 == 0 descriptor); a class is padded to whole 128-row workgroup tiles, rows past the last head or
// past a head's seg_len are inert.  A launch runs the list's stream prefix, then C, B, A.
struct PackClass {
    int32_t t_lo, L, tap_lo;
    int32_t first_tile, n_tiles;   // workgroup tiles of the launch (first_tile counts from the launch's first workgroup)
};
struct PackLayer {
    PackClass cls[3];          // C, B, A
    int32_t n_heads;
    int32_t n_stream_tiles;    // workgroup tiles of the list's stream prefix
    int32_t n_tiles;           // workgroup tiles of the packed launch: stream prefix + classes (0: the layer is not packed)
    int32_t mixed;             // 1: the stream prefix ends inside a workgroup tile; that tile's four descriptors, its head sub-tiles
                               //    emptied, follow the layer's head_segs
};
struct TileLists {
    const TileDesc* d[RD_MAX_LAYERS];
    int n[RD_MAX_LAYERS];          // workgroup tiles = descriptors / 4
    int64_t rows[RD_MAX_LAYERS];   // time steps the layer evaluates (for the FLOP / byte accounting of the timers)
    // packed heads (plan_fill_packed; plan_fill_lists leaves them off)
    const TileDesc* head_segs[RD_MAX_LAYERS];
    PackLayer pack[RD_MAX_LAYERS];
    // slab tiles (rd_slab_tile) of the whole list, and of the stream prefix a packed launch runs (without its mixed tile)
    int slab[RD_MAX_LAYERS];
    int slab_stream[RD_MAX_LAYERS];
};

struct KernelTimer {
    // HIP-event timing of one kernel family on the launch stream (bench.py roofline leg)
    bool enabled = false;
    std::vector<hipEvent_t> starts, stops;
    size_t used = 0;
    double flops = 0.0;  // algorithmic flops accumulated over recorded launches
    double bytes = 0.0;
    std::vector<double> each_flops;   // per recorded launch (rd_timer_read_launches: the roofline by kernel variant)
    std::vector<int> each_tag;        // conv: 0 relu (a block's first conv), 1 res_ident, 2 res_match (block 0's second conv); others 0
};

// One forward "lane": a stream with its own three activation tensors.  Lane 0 is the context's main stream; the
// pipelined entry points spread consecutive batches over several lanes so that independent kernel chains overlap (the
// partially filled last round of one chain's launch is filled by the other chain's workgroups).
constexpr int RD_MAX_LANES = 4;
struct FwdLane {
    hipStream_t st = nullptr;
    DevBuf act[3];
    hipEvent_t done = nullptr;   // recorded after the lane's latest forward
};

struct rd_ctx {
    int device = 0;
    int n_cu = 256;      // compute units of the device (launch-shape decisions)
    int precision = 0;   // 0: exact fp32 MFMA (default); 1: split-f16 (f16x3); 2: three-term bf16 split (bf16x3) matrix products
    int decode_form = 0; // rd_set_decode_form
    int decode_math = 1; // rd_set_decode_math (default: glibc's operation sequence -- scores bit-identical to the reference's)
    int conv_fuse = 1;   // rd_set_conv_fuse: 1 = block 0's first conv is computed inside its second (forward.hip, FIN), 0 = its own kernel
    int64_t packed_tiles = 0;   // packed window-head workgroup tiles the latest forward launched (rd_head_pack_tiles)
    int head_pack = 1;   // rd_set_head_pack: 1 = chunk-mode window heads run as packed classes that skip the zero-padding taps (exact fp32 only), 0 = as head tiles
    int conv_slab = 1;   // rd_set_conv_slab: 1 = slab tiles (rd_slab_tile) stage their input rows once per channel slice (exact fp32, product shape), 0 = per tap
    int64_t slab_tiles = 0;     // slab workgroup tiles the latest forward launched (rd_conv_slab_tiles)
    int conv_shape = 0;  // rd_set_conv_shape: 0 = 128-row tiles, two 256-thread workgroups per CU; 1 = 256-row tiles, one 512-thread workgroup
    int logits_f16 = 0;  // 1: the reads-level paths keep the softmax rows as f16 in HBM (10 B per time step), the decoder widens them
    hipStream_t stream = nullptr;
    hipStream_t stream_hi = nullptr;   // high priority: the beam search of the unpipelined entry points (a few long-running waves
                                       // that must not queue behind another context's forward workgroups)
    hipEvent_t ev_chain = nullptr;
    Model model;
    LM lm;
    // workspaces
    DevBuf ws_tiles, ws_raw;
    int tiles_nW = -1, tiles_T = -1;   // shape the cached uniform tile descriptors were built for
    int tiles_slab = 0;                // slab tiles among them
    // lanes[0].st == stream; lanes >= 1 are created on first use.  Lanes [RD_MAX_LANES, 2 RD_MAX_LANES) are the PARTITIONED
    // twins of lanes [0, RD_MAX_LANES): their streams are CU-masked to everything but the decode partition (below)
    FwdLane lanes[2 * RD_MAX_LANES];
    // Decode partition (global-mode reads pipeline): part_cus CUs of every XCD are kept free of forward workgroups and run
    // the beam search.  A beam-search wave that shares a SIMD with conv waves issuing MFMAs back to back gets about one
    // instruction issue per MFMA (measured: 17 us per time step instead of 2), and a read's search is one serial chain.
    int part_mode = -1;   // rd_set_decode_partition: -1 = chosen by beam width, 0 = off, k = k CUs per XCD
    int part_cus = 0;     // CUs per XCD the existing masked streams were created for (0: none exist)
    DevBuf ws_in, ws_probs, ws_mat, ws_seq, ws_nodes_child, ws_nodes_back, ws_labels, ws_misc;
    DevBuf ws_queue;                // the work-queue counter of beam_search_queue_kernel (decode.hip)
    DevBuf ws_wide, ws_wide_slot;   // beam widths above 51 (decode_wide.hip): per-sequence scratch block, per-trie-node slot map
    // The stages' device blocks.  Each is described once, by its stage's layout function (carve.h), which sizes it dry and then carves it.
    DevBuf ws_align;                // the budgeted entry points (align, fit, ctc_align, map, eventalign, sigmap): one launch at a time, sized exactly to the
                                    // largest launch under the caller's budget (budget.h, reserve_exact); carved per launch, checked by rd_carve_check
    DevBuf ws_ctc;                  // rd_ctc_* (ctc.hip): ctc_layout
    DevBuf ws_calign;               // rd_ctc_align_* (ctcalign.hip): ca_io_layout
    DevBuf ws_events, ws_events_io; // rd_event_stats* (events.hip): a launch's group descriptors; ev_io_layout
    DevBuf ws_polya, ws_polya_io;   // rd_polya_* (polya.hip): pa_layout; the per-read results of a host-pointer call
    DevBuf ws_segment;              // rd_segment* (segment.hip): sg_layout
    DevBuf ws_sim;                  // rd_sim_* (sim.hip): sim_layout
    DevBuf ws_eval, ws_eval_model;  // rd_eventalign, rd_sigmap and signal_dev.h: ea_io_layout, sm_io_layout, signal_scales; signal_upload_tables, sm_panel_layout
    DevBuf ws_site;                 // rd_site_* (sitecmp.hip): sc_layout
    DevBuf ws_quant;                // rd_quant_em (quant.hip): the packed candidates, the counts and the shares of one call, resident over its iterations
    // rd_pileup_* (pileup.hip): the accumulator lives from rd_pileup_open to rd_pileup_close, across calls (as the seed index of rd_map_index does)
    DevBuf pileup_sites;            // [pileup_n_sites][8] uint32: A C G T other del ins starts
    DevBuf pileup_profile;          // [RD_PILEUP_PROFILE_LEN] uint64
    DevBuf ws_pileup;               // rd_pileup_add_ops and rd_pileup_read (pileup.hip): pu_ops_layout, pu_read_layout
    int64_t pileup_n_sites = -1;    // -1: not open
    int64_t pileup_pairs = 0;       // pairs added since rd_pileup_open (at most 2^31 - 1: no 32-bit site counter can overflow)
    int64_t trie_budget = (int64_t)24 << 30;   // bytes of beam-search workspace one launch may ask for (rd_plan_trie_runs; rd_set_trie_budget)
    // pinned host staging
    void* h_stage = nullptr;
    size_t h_stage_cap = 0;
    bool h_stage_busy = false;   // an async copy out of h_stage was queued and the stream has not been synchronised since
    KernelTimer timer_conv, timer_decode, timer_head, timer_in;
    void* rccl = nullptr;  // RcclState*
    void* rpipe = nullptr; // ReadsPipe* (the forward / decode software pipeline over submitted batches, pipe_reads.hip)
    int pipe_group = 4;    // batches per beam-search launch (rd_pipe_config)
    int pipe_lanes = 2;    // forward streams the submitted batches rotate over (rd_pipe_set_lanes)
    void* plan_cache[2] = {nullptr, nullptr};  // PlanCache* for chunk / global reads-level plans
    void* train = nullptr; // TrainState* (train.hip): created by the first training call, never by inference
    void* map = nullptr;   // MapState* (map.hip): the seed index of rd_map_index and the buffers of rd_map_batch
};

// model.hip
size_t rd_model_image_floats(int nblocks);   // floats of a model's device storage: every packed image of every precision
void rd_model_bind(Model& m);                // the pointers of m into m.storage, by m.nblocks
int rd_model_refresh_split(rd_ctx* ctx);     // rebuilds every packed image from the trained weights when split_stale is set
int rd_model_halo(const rd_ctx* ctx);        // receptive field - 1 = (K-1) * 2 * sum(dilations)
// the LM image: table [n][4], entropies [n], then one bit per context ("absent from a sparse model"), padded to doubles
size_t rd_lm_image_doubles(int table_order);
void rd_lm_bind(LM& lm);   // the pointers of lm into lm.storage, by lm.table_order
// lmbuild.hip: entropies and absent mask of the table in lm.table (rows of NaN = absent contexts), on the device; marks the model loaded
int rd_lm_finish_device(rd_ctx* ctx, int table_order, int context_len, int hashed);
// forward.hip
bool rd_pack_heads(const rd_ctx* ctx);   // the context runs chunk-mode window heads as packed classes (rd_set_head_pack, exact fp32, product shape, Model::pack_ok)
bool rd_conv_slab(const rd_ctx* ctx);    // the context's exact-fp32 conv launches behind block 0 take the slab path for their slab tiles (rd_set_conv_slab, exact fp32, product shape)
int rd_forward_dev(rd_ctx* ctx, const float* d_windows, int nW, int T, float* d_probs, int lane = 0);
int rd_forward_tiles_dev(rd_ctx* ctx, const float* d_signal, const TileLists& tiles, int64_t total_rows, void* d_probs, int lane = 0,
                         int probs_f16 = 0 /* 1: d_probs is _Float16 [rows][5] */);
int rd_lane_get(rd_ctx* ctx, int lane, FwdLane** out);   // creates the lane's stream on first use
constexpr int RD_XCDS = 8;                               // MI355X: 8 XCDs x 32 CUs; CU-mask bit i = CU i / 8 of XCD i % 8
int rd_part_set(rd_ctx* ctx, int cus_per_xcd);           // (re)size the decode partition: drops the masked lane streams of another size
// pooled CU-masked streams: on the first k CUs of every XCD (complement = false) or on all the others
int rd_masked_stream_acquire(int device, int cus_per_xcd, bool complement, hipStream_t* out);
void rd_masked_stream_release(hipStream_t st);   // waits for the stream, then hands it back (never destroyed)
int rd_sync_lanes(rd_ctx* ctx);                          // every forward stream idle
int rd_split3_dev(rd_ctx* ctx, const float* d_in, size_t n, uint16_t* d_out);   // fp32 -> [3][n] bf16 bit patterns (hi, mid, lo)
// decode.hip
int rd_decode_dev(rd_ctx* ctx, const void* d_probs, int ptype /* 0 f32, 1 f64, 2 f16 rows */, const int64_t* d_seq_off, const int32_t* d_seq_len,
                  const int64_t* d_node_off, const int64_t* d_label_off, int n_seq, int64_t total_nodes, int W, int use_lm,
                  double s_thr, double r_thr, uint8_t* d_labels, int32_t* d_label_len, double* d_best_score,
                  hipStream_t stream = nullptr /* default: ctx->stream */, const int64_t* d_seq_off2 = nullptr,
                  const int32_t* d_seq_split = nullptr, int n_cu_avail = 0 /* CUs the stream may use (0: all) */,
                  int queue_wave_slots = 0 /* > 0: n_seq exceeds what those CUs keep resident: that many waves' worth of workgroups take the sequences from a queue */);
// preprocess.hip
int rd_normalise_dev(rd_ctx* ctx, const int16_t* d_raw, const int64_t* d_read_off, int n_reads, int clip, float* d_out,
                     int32_t* d_status, hipStream_t stream = nullptr /* default: ctx->stream */);
// assemble.hip
// one read of a batched assembly: its forward rows start at row src_row of the probability buffer (streamed: row t of the
// read; windowed: window i at src_row + i*T), its N assembled float64 rows go to row out_row of the output
struct AsmRead {
    int64_t src_row, out_row;
    int32_t N, nW, pad, pad_;
};
int rd_assemble_batch_dev(hipStream_t st, const void* d_probs, const AsmRead* d_reads, int n_reads, int64_t max_n, int T, int step,
                          double* d_out, int streamed, int in_f16);
int rd_gather_windows_dev(hipStream_t st, const float* d_rows, const int64_t* d_off1, const int64_t* d_off2, const int32_t* d_split,
                          const int32_t* d_valid, int n_windows, int T, float* d_out);
int rd_assemble_dev(rd_ctx* ctx, const void* d_probs, int nW, int T, int pad, int step, double* d_out, int64_t N,
                    int streamed = 0 /* 1: d_probs is the streamed forward [N][5]; row t is taken from row t */,
                    int in_f16 = 0 /* 1: d_probs rows are _Float16 */);

// ctcalign.hip: forced CTC alignment of sequences whose rows (ptype 0 f32, 1 f64, 2 f16) and labels are on the device already; every
// array argument but d_probs / d_labels is a host array.  Sequence i: rows seq_off[i] .. + seq_len[i] of d_probs, label_len[i] labels at
// d_labels + dlab_off[i]; its per-base results go to first_step / last_step / qual + out_off[i].  Launches on st and waits for it.
// Contract, budget and return value as rd_ctc_align_batch (include/radian_hip.h).
int rd_ctc_align_dev(rd_ctx* ctx, hipStream_t st, const void* d_probs, int ptype, const int64_t* seq_off, const int32_t* seq_len, int n_seq,
                     const uint8_t* d_labels, const int64_t* dlab_off, const int32_t* label_len, int64_t budget_bytes, int32_t* first_step,
                     int32_t* last_step, uint8_t* qual, const int64_t* out_off, double* score, int32_t* status);
// events.hip: the event table of reads whose raw samples and steps are on the device already; read_off, label_off,
// label_len and align_status are host arrays, every other array is a device pointer indexed as in rd_event_stats.  No argument check: the
// kernel stays inside the read and inside its own labels whatever the steps say.  Launches on st and waits for it.
int rd_event_stats_dev(rd_ctx* ctx, hipStream_t st, const int16_t* d_raw, const int64_t* read_off, int n_reads, const int32_t* d_first,
                       const int32_t* d_last, const int64_t* label_off, const int32_t* label_len, const int32_t* align_status, int32_t* d_start,
                       int32_t* d_end, int64_t* d_sum, int64_t* d_sumsq, int16_t* d_min, int16_t* d_max);
// ... with the steps and the event arrays on the host (n_labels: the extent of the label offsets): uploads the steps, runs
// rd_event_stats_dev and fetches every read's events
int rd_event_stats_steps(rd_ctx* ctx, hipStream_t st, const int16_t* d_raw, const int64_t* read_off, int n_reads, const int32_t* first_step,
                         const int32_t* last_step, const int64_t* label_off, const int32_t* label_len, const int32_t* align_status, int64_t n_labels,
                         int32_t* ev_start, int32_t* ev_end, int64_t* ev_sum, int64_t* ev_sumsq, int16_t* ev_min, int16_t* ev_max);
// polya.hip: the flat-segment search of reads whose raw samples are on the device already: read r is samples
// d_raw + read_off[r] .. read_off[r+1] (read_off is a host array), its result goes to d_out[r] on the device.  No argument check and no
// budget: one launch of each kernel, on a workspace sized to the reads (ws_polya).  Launches on st and waits for it.
int rd_polya_segment_dev(rd_ctx* ctx, hipStream_t st, const int16_t* d_raw, const int64_t* read_off, int n_reads, const PaParams& p, PaOut* d_out);
// context.hip: budget_bytes == 0 of a budgeted entry point becomes rd_default_budget (budget.h) of the device's free memory and `held`
int rd_resolve_budget(int64_t* budget_bytes, size_t held);
// train.hip
void rd_train_invalidate(rd_ctx* ctx);   // new weights arrived: the next training call re-reads them and zeroes the Adam moments
void rd_train_destroy(rd_ctx* ctx);
int rd_train_weights_host(rd_ctx* ctx, std::vector<float>& flat);
// map.hip
void rd_map_destroy(rd_ctx* ctx);
// api.hip
void rd_plan_cache_destroy_internal(rd_ctx* ctx);   // the cached reads-level plans of the synchronous entry points

// pipe_reads.hip
bool rd_rpipe_idle(const rd_ctx* ctx);
int rd_rpipe_drain_decode(rd_ctx* ctx);   // wait for the pipeline's beam searches in flight (they share the trie workspace)
void rd_rpipe_destroy(rd_ctx* ctx);

// The beam search packs (parent node id << 2) | label into a 32-bit back-pointer and gives a sequence at most 1 + W * rows
// trie nodes: a sequence must satisfy 1 + W * rows < 2^29 (W = 10: 53 M rows; W = 51: 10.5 M rows).  Host-side check of
// every entry point that knows its sequence lengths (RD_ERR_ARG beyond, instead of a silently wrong traceback).
inline bool rd_decode_len_ok(int W, int64_t rows) { return 1 + (int64_t)W * rows < ((int64_t)1 << 29); }

extern "C" int rd_decode_max_width(void);
constexpr int RD_LANE_MAX_W = 256;     // decode.hip: the wave-per-sequence kernels' widest beam (rd_decode_lane_width)
constexpr int RD_HASHED_MAX_W = 64;    // ... and the widest one with hashed long contexts (rd_load_lm_hashed)
// decode_wide.hip: beam widths above RD_LANE_MAX_W, up to RD_WIDE_MAX_W (40 W bytes of LDS for the ranking keys)
constexpr int RD_WIDE_MAX_W = 1024;
int rd_decode_wide_launch(rd_ctx* ctx, hipStream_t st, const void* decode_args, int ptype, int n_seq, int64_t total_nodes, bool lm);

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// decode_wide.hip's per-sequence scratch block: beams [2][W] of 48 B | c_ptot, c_pb, c_pnb [5W] doubles | c_pj, c_src [5W] ints | mq [W] ints
inline size_t rd_wide_scratch_bytes(int W)
{
    const size_t b = (size_t)2 * W * 48 + (size_t)3 * 5 * W * 8 + (size_t)2 * 5 * W * 4 + (size_t)W * 4;
    return (b + 255) & ~(size_t)255;
}

// One beam-search launch needs (1 + W * rows) trie nodes per sequence -- 20 B each (child table + back pointer), 24 B above the lane
// kernels' width (the slot map of decode_wide.hip) plus that kernel's scratch block per sequence -- for ALL its sequences at once: W x the
// rows of the launch.  A pipeline group of 96 M rows at W = 100, or a few thousand windows at W = 1024, would ask for hundreds of GB and die
// with RD_ERR_NOMEM in the middle of a job.  So every caller that builds a launch's node offsets cuts its sequences -- in launch
// order -- into RUNS whose workspace fits the context's budget (at least one sequence per run); the runs go to rd_decode_dev one after the
// other on the same stream and share the workspace.  Node offsets restart at 0 in every run.  Results do not depend on the cut.
struct TrieRun {
    int k0, k1;          // sequences [k0, k1) of the launch order
    int64_t nodes;       // their trie nodes
};
template <typename LenOf>
inline void rd_plan_trie_runs(const rd_ctx* ctx, int W, int k_begin, int k_end, LenOf len_of, int64_t* node_off, std::vector<TrieRun>& runs)
{
    const int64_t per_node = W > RD_LANE_MAX_W ? 24 : 20;
    const int64_t per_seq = W > RD_LANE_MAX_W ? (int64_t)rd_wide_scratch_bytes(W) : 0;
    int64_t nodes = 0, bytes = 0;
    int k0 = k_begin;
    for (int k = k_begin; k < k_end; k++) {
        const int64_t nk = 1 + (int64_t)W * len_of(k), bk = nk * per_node + per_seq;
        if (k > k0 && bytes + bk > ctx->trie_budget) {
            runs.push_back({k0, k, nodes});
            k0 = k;
            nodes = bytes = 0;
        }
        node_off[k] = nodes;
        nodes += nk;
        bytes += bk;
    }
    if (k_end > k0) runs.push_back({k0, k_end, nodes});
}

// Hashed long contexts (rd_load_lm_hashed) exist in the lane kernels only: refused where the arguments are checked, not when a group
// of batches is launched after earlier reads were written
#define RD_REQUIRE_WIDTH_LM(ctx, W, use_lm)                                                                                     \
    RD_REQUIRE(!((use_lm) && (ctx)->lm.loaded && (ctx)->lm.hashed && (W) > RD_HASHED_MAX_W),                                     \
               "beam width %d with a hashed long-context RNA model (rd_load_lm_hashed): hashed contexts exist for widths up to 64", (W))
