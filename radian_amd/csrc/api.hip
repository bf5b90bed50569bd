// api.hip -- the host-pointer entry points of libradian_hip.so (declared in include/radian_hip.h): the seams around the device
// paths, the fused chunk / global paths, and the reads-level and raw-signal paths.
#include "common.h"
#include "plan.h"
#include "../../include/radian_hip.h"

#include <math.h>
#include <string.h>

using namespace rdi;

// --------------------------------------------------------------------------------------------- helpers
namespace {

struct SeqMeta {
    // device pointers inside ctx->ws_seq
    int64_t *d_seq_off, *d_seq_off2, *d_node_off, *d_label_off;
    int32_t *d_seq_len, *d_split, *d_label_len;
    double* d_score;
    int64_t total_labels;
    std::vector<TrieRun> runs;   // launches that share the trie workspace, one after the other (rd_plan_trie_runs)
};

// uploads per-sequence metadata; seq_off2/split may be null (single source region per sequence)
int prepare_seq_meta(rd_ctx* ctx, const int64_t* seq_off, const int64_t* seq_off2, const int32_t* split, const int32_t* seq_len,
                     int n_seq, int W, SeqMeta& sm, std::vector<int64_t>& label_off_used)
{
    std::vector<int64_t> node_off(n_seq), lab_off(n_seq);
    int64_t labs = 0;
    for (int i = 0; i < n_seq; i++) {
        RD_REQUIRE(seq_len[i] >= 0, "decode: negative sequence length at %d", i);
        RD_REQUIRE(rd_decode_len_ok(W, seq_len[i]), "decode: sequence %d has %d rows; beam width %d supports at most %lld (1 + W * rows < 2^29)", i,
                   seq_len[i], W, (long long)((((int64_t)1 << 29) - 2) / W));
        lab_off[i] = labs;
        labs += seq_len[i];
    }
    sm.runs.clear();
    rd_plan_trie_runs(ctx, W, 0, n_seq, [&](int k) { return (int64_t)seq_len[k]; }, node_off.data(), sm.runs);
    label_off_used = lab_off;
    const size_t n = (size_t)n_seq;
    const size_t a8 = align_up(n * 8, 256), a4 = align_up(n * 4, 256);
    if (ctx->ws_seq.reserve(5 * a8 + 3 * a4)) return RD_ERR_NOMEM;
    char* p = (char*)ctx->ws_seq.p;
    sm.d_seq_off = (int64_t*)p; p += a8;
    sm.d_seq_off2 = (int64_t*)p; p += a8;
    sm.d_node_off = (int64_t*)p; p += a8;
    sm.d_label_off = (int64_t*)p; p += a8;
    sm.d_score = (double*)p; p += a8;
    sm.d_seq_len = (int32_t*)p; p += a4;
    sm.d_split = (int32_t*)p; p += a4;
    sm.d_label_len = (int32_t*)p;
    sm.total_labels = labs;
    // The metadata goes through the context's pinned staging block in ONE copy that needs no host-side wait: the block
    // is only rewritten by the next call on this context, and a caller that runs to completion ends with a stream
    // synchronisation (decode_and_fetch) before that can happen.  A caller that left early on an error did not: then the
    // copy may still be reading the block -- wait for it here before the block is rewritten (or freed).
    if (ctx->h_stage_busy) {
        RD_HIP(hipStreamSynchronize(ctx->stream));
        ctx->h_stage_busy = false;
    }
    const size_t stage_bytes = 4 * a8 + 2 * a4;   // seq_off | seq_off2 | node_off | label_off | seq_len | split
    if (ctx->h_stage_cap < stage_bytes) {
        RD_HIP(hipStreamSynchronize(ctx->stream));
        if (ctx->h_stage) (void)hipHostFree(ctx->h_stage);
        ctx->h_stage = nullptr;
        ctx->h_stage_cap = 0;
        const size_t want = align_up(stage_bytes + stage_bytes / 4, 1 << 16);
        RD_HIP(hipHostMalloc(&ctx->h_stage, want, hipHostMallocDefault));
        ctx->h_stage_cap = want;
    }
    char* hs = (char*)ctx->h_stage;
    memcpy(hs, seq_off, n * 8);
    if (seq_off2) memcpy(hs + a8, seq_off2, n * 8);
    memcpy(hs + 2 * a8, node_off.data(), n * 8);
    memcpy(hs + 3 * a8, lab_off.data(), n * 8);
    memcpy(hs + 4 * a8, seq_len, n * 4);
    if (split) memcpy(hs + 4 * a8 + a4, split, n * 4);
    // device layout: 5 x a8 (seq_off, seq_off2, node_off, label_off, score) then 3 x a4 (seq_len, split, label_len)
    ctx->h_stage_busy = true;
    RD_HIP(hipMemcpyAsync(sm.d_seq_off, hs, 4 * a8, hipMemcpyHostToDevice, ctx->stream));
    RD_HIP(hipMemcpyAsync(sm.d_seq_len, hs + 4 * a8, 2 * a4, hipMemcpyHostToDevice, ctx->stream));
    if (!seq_off2) {
        sm.d_seq_off2 = nullptr;
        sm.d_split = nullptr;
    }
    return RD_OK;
}

// the forced alignment of every decoded sequence against the rows its beam search read (ctcalign.hip): per-base outputs indexed as
// labels_out (label_off), score and status per sequence
struct AlignOut {
    int64_t budget;
    int32_t *first, *last;
    uint8_t* qual;
    double* score;
    int32_t* status;
    bool too_large = false;   // some sequence came back RD_CTCALIGN_TOO_LARGE (the call goes on and returns RD_ERR_NOMEM at its end)
};

// decode sequences over device rows and deliver labels to host buffers
int decode_and_fetch(rd_ctx* ctx, const void* d_probs, int is_f64, const int64_t* seq_off, const int32_t* seq_len, int n_seq,
                     int W, int use_lm, double s_thr, double r_thr, uint8_t* labels_out, const int64_t* label_off,
                     int32_t* label_len, double* best_score, const int64_t* seq_off2 = nullptr, const int32_t* split = nullptr,
                     AlignOut* ao = nullptr)
{
    if (n_seq == 0) return RD_OK;
    SeqMeta sm;
    std::vector<int64_t> lab_off;
    // beam searches still in flight on the pipeline's decode streams use the context's trie workspace: let them finish
    int rc = rd_rpipe_drain_decode(ctx);
    if (rc) return rc;
    rc = prepare_seq_meta(ctx, seq_off, seq_off2, split, seq_len, n_seq, W, sm, lab_off);
    if (rc) return rc;
    if (ctx->ws_labels.reserve((size_t)sm.total_labels + 16)) return RD_ERR_NOMEM;
    uint8_t* d_labels = ctx->ws_labels.as<uint8_t>();
    // everything queued on the context's stream so far (forward, assembly, metadata) precedes the beam search, which runs on
    // the high-priority stream: with another context's forward filling the chip, its few waves are dispatched first
    hipStream_t ds = ctx->stream_hi;
    RD_HIP(hipEventRecord(ctx->ev_chain, ctx->stream));
    RD_HIP(hipStreamWaitEvent(ds, ctx->ev_chain, 0));
    for (const TrieRun& r : sm.runs) {
        rc = rd_decode_dev(ctx, d_probs, is_f64, sm.d_seq_off + r.k0, sm.d_seq_len + r.k0, sm.d_node_off + r.k0, sm.d_label_off + r.k0, r.k1 - r.k0,
                           r.nodes, W, use_lm, s_thr, r_thr, d_labels, sm.d_label_len + r.k0, best_score ? sm.d_score + r.k0 : nullptr, ds,
                           sm.d_seq_off2 ? sm.d_seq_off2 + r.k0 : nullptr, sm.d_split ? sm.d_split + r.k0 : nullptr);
        if (rc) return rc;
    }
    std::vector<uint8_t> hl((size_t)sm.total_labels + 16);
    RD_HIP(hipMemcpyAsync(hl.data(), d_labels, (size_t)sm.total_labels, hipMemcpyDeviceToHost, ds));
    RD_HIP(hipMemcpyAsync(label_len, sm.d_label_len, (size_t)n_seq * 4, hipMemcpyDeviceToHost, ds));
    if (best_score) RD_HIP(hipMemcpyAsync(best_score, sm.d_score, (size_t)n_seq * 8, hipMemcpyDeviceToHost, ds));
    RD_HIP(hipStreamSynchronize(ds));
    ctx->h_stage_busy = false;   // (ds waited for ctx->stream's event: the metadata copy is done)
    for (int i = 0; i < n_seq; i++) {
        if (label_len[i] == RD_LEN_MISSING_CONTEXT && use_lm) continue;   // sparse LM: the search reached an absent context (the caller raises KeyError)
        if (label_len[i] < 0 || label_len[i] > seq_len[i]) {
            rd_set_error("decode: sequence %d produced an impossible label length %d (rows %d)", i, label_len[i], seq_len[i]);
            return RD_ERR_STATE;
        }
        if (label_len[i]) memcpy(labels_out + label_off[i], hl.data() + lab_off[i], (size_t)label_len[i]);
    }
    if (ao) {
        // the rows and the labels are still where the search left them
        RD_REQUIRE(!seq_off2, "internal: no forced alignment of sequences with two source regions");
        std::vector<int32_t> al(n_seq);
        for (int i = 0; i < n_seq; i++) al[i] = label_len[i] < 0 ? 0 : label_len[i];
        rc = rd_ctc_align_dev(ctx, ds, d_probs, is_f64, seq_off, seq_len, n_seq, d_labels, lab_off.data(), al.data(), ao->budget, ao->first, ao->last,
                              ao->qual, label_off, ao->score, ao->status);
        bool tl = false;
        for (int i = 0; i < n_seq; i++) {
            tl |= ao->status[i] == RD_CTCALIGN_TOO_LARGE;
            if (label_len[i] < 0) {   // no labels (RD_LEN_MISSING_CONTEXT): nothing was aligned
                ao->status[i] = RD_CTCALIGN_NO_PATH;
                ao->score[i] = -INFINITY;
            }
        }
        if (rc == RD_ERR_NOMEM && tl) ao->too_large = true;
        else if (rc) return rc;
    }
    return RD_OK;
}

}  // namespace

// --------------------------------------------------------------------------------------------- seams
extern "C" int rd_forward(rd_ctx* ctx, const float* windows, int n_windows, int chunk_len, float* probs)
{
    RD_REQUIRE(ctx && (n_windows == 0 || (windows && probs)), "rd_forward: null argument");
    RD_REQUIRE(n_windows >= 0 && chunk_len >= 1, "rd_forward: bad shape n_windows=%d chunk_len=%d", n_windows, chunk_len);
    if (n_windows == 0) return RD_OK;
    RD_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)n_windows * chunk_len;
    if (ctx->ws_in.reserve(n * 4) || ctx->ws_probs.reserve(n * 20)) return RD_ERR_NOMEM;
    RD_HIP(hipMemcpyAsync(ctx->ws_in.p, windows, n * 4, hipMemcpyHostToDevice, ctx->stream));
    int rc = rd_forward_dev(ctx, ctx->ws_in.as<float>(), n_windows, chunk_len, ctx->ws_probs.as<float>());
    if (rc) return rc;
    RD_HIP(hipMemcpyAsync(probs, ctx->ws_probs.p, n * 20, hipMemcpyDeviceToHost, ctx->stream));
    RD_HIP(hipStreamSynchronize(ctx->stream));
    return RD_OK;
}

extern "C" int rd_assemble(rd_ctx* ctx, const float* probs, int n_windows, int chunk_len, int pad, int step, double* out,
                           int64_t out_cap, int64_t* n_rows, int* is_f64)
{
    RD_REQUIRE(ctx && probs && out && n_rows, "rd_assemble: null argument");
    RD_REQUIRE(n_windows >= 1 && chunk_len >= 1, "rd_assemble: bad shape");
    RD_REQUIRE(step >= 1 && step <= chunk_len, "rd_assemble: step %d must be in [1, chunk_len]", step);
    RD_REQUIRE(pad >= 0 && pad <= chunk_len, "rd_assemble: pad %d out of range", pad);
    RD_HIP(hipSetDevice(ctx->device));
    const int64_t N = assembled_rows(n_windows, chunk_len, pad, step);
    RD_REQUIRE(N <= out_cap, "rd_assemble: output needs %lld rows, capacity %lld", (long long)N, (long long)out_cap);
    const size_t nin = (size_t)n_windows * chunk_len * 5;
    if (ctx->ws_probs.reserve(nin * 4) || ctx->ws_mat.reserve((size_t)(N + 1) * 40)) return RD_ERR_NOMEM;
    RD_HIP(hipMemcpyAsync(ctx->ws_probs.p, probs, nin * 4, hipMemcpyHostToDevice, ctx->stream));
    int rc = rd_assemble_dev(ctx, ctx->ws_probs.as<float>(), n_windows, chunk_len, pad, step, ctx->ws_mat.as<double>(), N);
    if (rc) return rc;
    if (N) RD_HIP(hipMemcpyAsync(out, ctx->ws_mat.p, (size_t)N * 40, hipMemcpyDeviceToHost, ctx->stream));
    RD_HIP(hipStreamSynchronize(ctx->stream));
    *n_rows = N;
    if (is_f64) *is_f64 = assembled_is_f64(n_windows, chunk_len, pad, step);
    return RD_OK;
}

extern "C" int rd_decode_batch(rd_ctx* ctx, const void* probs, int prob_is_f64, const int64_t* seq_off, const int32_t* seq_len,
                               int n_seq, int beam_width, int use_lm, double s_thr, double r_thr, uint8_t* labels_out,
                               const int64_t* label_off, int32_t* label_len, double* best_score)
{
    RD_REQUIRE(ctx, "rd_decode_batch: null context");
    RD_REQUIRE(n_seq >= 0, "rd_decode_batch: negative n_seq");
    if (n_seq == 0) return RD_OK;
    RD_REQUIRE(seq_off && seq_len && labels_out && label_off && label_len, "rd_decode_batch: null argument");
    RD_REQUIRE(beam_width >= 1 && beam_width <= rd_decode_max_width(), "rd_decode_batch: beam_width %d out of range [1,%d]",
               beam_width, rd_decode_max_width());
    RD_REQUIRE_WIDTH_LM(ctx, beam_width, use_lm);
    RD_HIP(hipSetDevice(ctx->device));
    int64_t rows = 0;
    for (int i = 0; i < n_seq; i++) {
        RD_REQUIRE(seq_len[i] >= 0 && seq_off[i] >= 0, "rd_decode_batch: bad sequence %d", i);
        RD_REQUIRE(rd_decode_len_ok(beam_width, seq_len[i]), "rd_decode_batch: sequence %d has %d rows; beam width %d supports at most %lld (1 + W * rows < 2^29)",
                   i, seq_len[i], beam_width, (long long)((((int64_t)1 << 29) - 2) / beam_width));
        if (seq_off[i] + seq_len[i] > rows) rows = seq_off[i] + seq_len[i];
    }
    RD_REQUIRE(rows == 0 || probs, "rd_decode_batch: null probs");
    const size_t rb = prob_is_f64 ? 40 : 20;
    if (ctx->ws_mat.reserve((size_t)(rows + 1) * rb)) return RD_ERR_NOMEM;
    if (rows) RD_HIP(hipMemcpyAsync(ctx->ws_mat.p, probs, (size_t)rows * rb, hipMemcpyHostToDevice, ctx->stream));
    return decode_and_fetch(ctx, ctx->ws_mat.p, prob_is_f64, seq_off, seq_len, n_seq, beam_width, use_lm, s_thr, r_thr, labels_out,
                            label_off, label_len, best_score);
}

// --------------------------------------------------------------------------------------------- fused
static int chunk_decode_from_probs(rd_ctx* ctx, const float* d_probs, int n_windows, int chunk_len, const int32_t* valid_len,
                                   int beam_width, uint8_t* labels_out, int32_t* label_len)
{
    std::vector<int64_t> seq_off(n_windows), lab_off(n_windows);
    for (int i = 0; i < n_windows; i++) {
        RD_REQUIRE(valid_len[i] >= 0 && valid_len[i] <= chunk_len, "valid_len[%d]=%d out of range [0,%d]", i, valid_len[i], chunk_len);
        seq_off[i] = (int64_t)i * chunk_len;
        lab_off[i] = (int64_t)i * chunk_len;
    }
    return decode_and_fetch(ctx, d_probs, 0, seq_off.data(), valid_len, n_windows, beam_width, 0, 0.0, 0.0, labels_out, lab_off.data(),
                            label_len, nullptr);
}

extern "C" int rd_basecall_chunk_resident(rd_ctx* ctx, const float* d_windows, int n_windows, int chunk_len,
                                          const int32_t* valid_len, int beam_width, uint8_t* labels_out, int32_t* label_len)
{
    RD_REQUIRE(ctx && d_windows && valid_len && labels_out && label_len, "rd_basecall_chunk_resident: null argument");
    RD_REQUIRE(n_windows >= 1 && chunk_len >= 1, "rd_basecall_chunk_resident: bad shape");
    RD_REQUIRE(beam_width >= 1 && beam_width <= rd_decode_max_width(), "beam_width %d out of range", beam_width);
    RD_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)n_windows * chunk_len;
    if (ctx->ws_probs.reserve(n * 20)) return RD_ERR_NOMEM;
    int rc = rd_forward_dev(ctx, d_windows, n_windows, chunk_len, ctx->ws_probs.as<float>());
    if (rc) return rc;
    return chunk_decode_from_probs(ctx, ctx->ws_probs.as<float>(), n_windows, chunk_len, valid_len, beam_width, labels_out, label_len);
}

extern "C" int rd_basecall_chunk(rd_ctx* ctx, const float* windows, int n_windows, int chunk_len, const int32_t* valid_len,
                                 int beam_width, uint8_t* labels_out, int32_t* label_len)
{
    RD_REQUIRE(ctx && windows, "rd_basecall_chunk: null argument");
    RD_REQUIRE(n_windows >= 1 && chunk_len >= 1, "rd_basecall_chunk: bad shape");
    RD_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)n_windows * chunk_len;
    if (ctx->ws_in.reserve(n * 4)) return RD_ERR_NOMEM;
    RD_HIP(hipMemcpyAsync(ctx->ws_in.p, windows, n * 4, hipMemcpyHostToDevice, ctx->stream));
    return rd_basecall_chunk_resident(ctx, ctx->ws_in.as<float>(), n_windows, chunk_len, valid_len, beam_width, labels_out, label_len);
}

extern "C" int rd_decode_resident(rd_ctx* ctx, const float* d_probs, int n_windows, int chunk_len, const int32_t* valid_len,
                                  int beam_width, uint8_t* labels_out, int32_t* label_len)
{
    RD_REQUIRE(ctx && d_probs && valid_len && labels_out && label_len, "rd_decode_resident: null argument");
    RD_REQUIRE(beam_width >= 1 && beam_width <= rd_decode_max_width(), "beam_width %d out of range", beam_width);
    RD_HIP(hipSetDevice(ctx->device));
    return chunk_decode_from_probs(ctx, d_probs, n_windows, chunk_len, valid_len, beam_width, labels_out, label_len);
}

extern "C" int rd_forward_resident(rd_ctx* ctx, const float* d_windows, int n_windows, int chunk_len, float* d_probs)
{
    RD_REQUIRE(ctx && d_windows, "rd_forward_resident: null argument");
    RD_HIP(hipSetDevice(ctx->device));
    if (!d_probs) {
        if (ctx->ws_probs.reserve((size_t)n_windows * chunk_len * 20)) return RD_ERR_NOMEM;
        d_probs = ctx->ws_probs.as<float>();
    }
    return rd_forward_dev(ctx, d_windows, n_windows, chunk_len, d_probs);
}

// Assembly + decode of a batch of reads given the forward's probabilities d_probs (f16: _Float16 rows; streamed or windowed row
// layout): read r has the windows win_off[r] .. win_off[r+1] (pad[r]: the pad of its last one) and its forward rows start at row
// src_row[r].  Reads some time step of which is covered twice are assembled into one concatenated float64 matrix; the others
// (single coverage: the forward's rows are consecutive time steps) are decoded straight from their float32 / f16 rows.
// read_off (nullable): the reads' samples, which the assembled lengths must equal.
// the rows of every read of the batch: classification, and the float64 matrix of the assembled ones in ctx->ws_mat
static int global_rows(rd_ctx* ctx, const void* d_probs, int f16, bool streamed, const int32_t* win_off, const int32_t* pad, const int64_t* src_row,
                       const int64_t* read_off, int n_reads, int chunk_len, int step, std::vector<ReadRows>& rr)
{
    const int64_t rows64 = classify_reads(win_off, pad, n_reads, chunk_len, step, 0, rr);
    for (int r = 0; read_off && r < n_reads; r++)
        RD_REQUIRE(rr[r].N == read_off[r + 1] - read_off[r], "internal: assembled length mismatch for read %d", r);
    if (ctx->ws_mat.reserve((size_t)(rows64 + 1) * 40)) return RD_ERR_NOMEM;
    int rc;
    for (int r = 0; r < n_reads; r++) {
        if (!rr[r].is64) continue;
        rc = rd_assemble_dev(ctx, (const char*)d_probs + (size_t)src_row[r] * 5 * (f16 ? 2 : 4), win_off[r + 1] - win_off[r], chunk_len, pad[r], step,
                             ctx->ws_mat.as<double>() + rr[r].row64 * 5, rr[r].N, streamed ? 1 : 0, f16);
        if (rc) return rc;
    }
    return RD_OK;
}

static int global_finish(rd_ctx* ctx, const void* d_probs, int f16, bool streamed, const int32_t* win_off, const int32_t* pad, const int64_t* src_row,
                         const int64_t* read_off, int n_reads, int chunk_len, int step, int beam_width, int use_lm, double s_thr, double r_thr,
                         uint8_t* labels_out, const int64_t* label_off, int32_t* label_len, AlignOut* ao = nullptr /* per read, as label_len */)
{
    std::vector<ReadRows> rr;
    int rc = global_rows(ctx, d_probs, f16, streamed, win_off, pad, src_row, read_off, n_reads, chunk_len, step, rr);
    if (rc) return rc;
    // two decode launches: float64 (assembled) reads and float32 (single-coverage) reads
    for (int pass = 0; pass < 2; pass++) {
        std::vector<int64_t> so, lo;
        std::vector<int32_t> sl;
        std::vector<int> idx;
        for (int r = 0; r < n_reads; r++)
            if (rr[r].is64 == (pass == 0)) {
                so.push_back(pass == 0 ? rr[r].row64 : src_row[r]);
                sl.push_back((int32_t)rr[r].N);
                lo.push_back(label_off[r]);
                idx.push_back(r);
            }
        if (idx.empty()) continue;
        std::vector<int32_t> ll(idx.size()), ast(idx.size());
        std::vector<double> asc(idx.size());
        AlignOut pa;
        if (ao) {
            pa = *ao;
            pa.score = asc.data();
            pa.status = ast.data();
        }
        rc = decode_and_fetch(ctx, pass == 0 ? (const void*)ctx->ws_mat.p : d_probs, pass == 0 ? 1 : (f16 ? 2 : 0), so.data(), sl.data(),
                              (int)idx.size(), beam_width, use_lm, s_thr, r_thr, labels_out, lo.data(), ll.data(), nullptr, nullptr, nullptr,
                              ao ? &pa : nullptr);
        if (rc) return rc;
        for (size_t i = 0; i < idx.size(); i++) {
            label_len[idx[i]] = ll[i];
            if (ao) {
                ao->score[idx[i]] = asc[i];
                ao->status[idx[i]] = ast[i];
                ao->too_large |= pa.too_large;
            }
        }
    }
    return RD_OK;
}

extern "C" int rd_basecall_global(rd_ctx* ctx, const float* windows, int chunk_len, int step, const int32_t* read_win_off,
                                  const int32_t* pad, int n_reads, int beam_width, int use_lm, double s_thr, double r_thr,
                                  uint8_t* labels_out, const int64_t* label_off, int32_t* label_len)
{
    RD_REQUIRE(ctx && windows && read_win_off && pad && labels_out && label_off && label_len, "rd_basecall_global: null argument");
    RD_REQUIRE(n_reads >= 1 && chunk_len >= 1, "rd_basecall_global: bad shape");
    RD_REQUIRE(step >= 1 && step <= chunk_len, "rd_basecall_global: step %d must be in [1, chunk_len]", step);
    RD_REQUIRE(beam_width >= 1 && beam_width <= rd_decode_max_width(), "beam_width %d out of range", beam_width);
    RD_REQUIRE_WIDTH_LM(ctx, beam_width, use_lm);
    RD_HIP(hipSetDevice(ctx->device));
    const int nW = read_win_off[n_reads];
    RD_REQUIRE(nW >= n_reads, "rd_basecall_global: every read needs at least one window");
    const size_t n = (size_t)nW * chunk_len;
    if (ctx->ws_in.reserve(n * 4) || ctx->ws_probs.reserve(n * 20)) return RD_ERR_NOMEM;
    RD_HIP(hipMemcpyAsync(ctx->ws_in.p, windows, n * 4, hipMemcpyHostToDevice, ctx->stream));
    int rc = rd_forward_dev(ctx, ctx->ws_in.as<float>(), nW, chunk_len, ctx->ws_probs.as<float>());
    if (rc) return rc;
    std::vector<int64_t> src_row(n_reads);
    for (int r = 0; r < n_reads; r++) {
        RD_REQUIRE(read_win_off[r + 1] > read_win_off[r], "rd_basecall_global: read %d has no windows", r);
        RD_REQUIRE(pad[r] >= 0 && pad[r] <= chunk_len, "rd_basecall_global: pad[%d] out of range", r);
        src_row[r] = (int64_t)read_win_off[r] * chunk_len;
    }
    return global_finish(ctx, ctx->ws_probs.p, 0, false, read_win_off, pad, src_row.data(), nullptr, n_reads, chunk_len, step, beam_width, use_lm,
                         s_thr, r_thr, labels_out, label_off, label_len);
}

extern "C" int rd_count_windows(int64_t n_samples, int chunk_len, int step)
{
    if (n_samples < 0 || chunk_len < 1 || step < 1 || step > chunk_len) return -1;
    return count_windows(n_samples, chunk_len, step);
}

// --------------------------------------------------------------------------------------------- reads-level paths
// The reference windows every read (chunk_len rows every step samples, preprocess.py:4-22) and runs the model on every
// window, although the TCN is causal with a finite receptive field RF = 1 + (K-1)*2*sum(dilations) (253 samples):
// row r >= RF-1 of a window does not depend on where the window starts.  So the forward is run ONCE over the whole read
// (the "stream"); a window's rows >= halo = RF-1 are the stream's rows, and only its first `halo` rows -- the ones that
// see the window's own zero left-padding -- are computed separately ("heads").  Results are bit-identical to the
// windowed computation (each output row is the same fp32 fma chain over the same values; tests/test_gpu_reads.py), at
// N + (nW-1)*halo rows per read instead of nW*chunk_len (chunk mode), or N rows (global mode, where only the earliest
// covering window's row of each time step is ever used, matrix_assembly.py:46-53; valid when step <= chunk_len - halo).
namespace {
// plan + device tile descriptors for a batch of reads, cached while consecutive batches have the same read lengths
struct PlanCache {
    PlanKey key;
    ReadsPlan plan;
    bool streamed = false;
    DevBuf d_tiles;
    TileLists lists;
    bool has_pack = false;   // the packed heads' block was uploaded with the descriptors (only for a context that packs: rd_pack_heads)
};

int get_plan(rd_ctx* ctx, const int64_t* read_off, int n_reads, int chunk, int step, int mode, const ReadsPlan** out,
             const TileLists** lists, bool* streamed)
{
    PlanCache* pc = (PlanCache*)ctx->plan_cache[mode];
    if (!pc) {
        pc = new PlanCache();
        ctx->plan_cache[mode] = pc;
    }
    const int halo = rd_model_halo(ctx);
    const bool pack = mode == 0 && rd_pack_heads(ctx);
    if (!(pc->d_tiles.p && pc->key.matches(ctx->model, read_off, n_reads, chunk, step, mode, halo)) || (pack && !pc->has_pack)) {
        RD_REQUIRE(read_off[0] == 0, "read_off[0] must be 0");
        size_t total = 0;
        int rc = pc->key.rebuild(ctx->model, read_off, n_reads, chunk, step, mode, halo, pc->plan, &pc->streamed, &total);
        if (rc) return rc;
        const size_t n_desc = total;
        if (pack) total += plan_packed_descs(pc->plan);   // the packed heads' block, behind the descriptors
        if (pc->d_tiles.reserve(total * sizeof(TileDesc) + 16)) return RD_ERR_NOMEM;
        // make sure no forward still reads the previous descriptors
        if ((rc = rd_sync_lanes(ctx))) return rc;
        std::vector<TileDesc> host(total);
        plan_fill_lists(pc->plan, pc->d_tiles.as<TileDesc>(), host.data(), pc->lists);
        if (pack) plan_fill_packed(pc->plan, pc->d_tiles.as<TileDesc>() + n_desc, host.data() + n_desc, pc->lists);
        pc->has_pack = pack;
        if (total) RD_HIP(hipMemcpy(pc->d_tiles.p, host.data(), total * sizeof(TileDesc), hipMemcpyHostToDevice));
        pc->key.valid = true;
    }
    *out = &pc->plan;
    *lists = &pc->lists;
    if (streamed) *streamed = pc->streamed;
    return RD_OK;
}

}  // namespace

int rdi::rd_check_reads_args(rd_ctx* ctx, const void* signal, const int64_t* read_off, int n_reads, int chunk_len, int step, int W)
{
    RD_REQUIRE(ctx && signal && read_off, "null argument");
    RD_REQUIRE(n_reads >= 1 && chunk_len >= 1, "bad shape");
    RD_REQUIRE(step >= 1 && step <= chunk_len, "step %d must be in [1, chunk_len]", step);
    RD_REQUIRE(W >= 1 && W <= rd_decode_max_width(), "beam_width %d out of range", W);
    if (!ctx->model.loaded) {
        rd_set_error("no weights loaded (rd_load_weights)");
        return RD_ERR_STATE;
    }
    return RD_OK;
}

void rd_plan_cache_destroy_internal(rd_ctx* ctx)
{
    for (int m = 0; m < 2; m++) {
        PlanCache* pc = (PlanCache*)ctx->plan_cache[m];
        if (pc) {
            pc->d_tiles.release();
            delete pc;
        }
        ctx->plan_cache[m] = nullptr;
    }
}

extern "C" int rd_basecall_reads_chunk_resident(rd_ctx* ctx, const float* d_signal, const int64_t* read_off, int n_reads,
                                                int chunk_len, int step, int beam_width, uint8_t* labels_out,
                                                int32_t* label_len)
{
    int rc = rd_check_reads_args(ctx, d_signal, read_off, n_reads, chunk_len, step, beam_width);
    if (rc) return rc;
    RD_REQUIRE(labels_out && label_len, "rd_basecall_reads_chunk: null output");
    RD_HIP(hipSetDevice(ctx->device));
    const ReadsPlan* P = nullptr;
    const TileLists* tl = nullptr;
    if ((rc = get_plan(ctx, read_off, n_reads, chunk_len, step, 0, &P, &tl, nullptr))) return rc;
    if (ctx->ws_probs.reserve((size_t)P->total_rows * 20)) return RD_ERR_NOMEM;
    const int f16 = ctx->logits_f16;
    rc = rd_forward_tiles_dev(ctx, d_signal, *tl, P->total_rows, ctx->ws_probs.p, 0, f16);
    if (rc) return rc;
    std::vector<int64_t> lab_off(P->n_windows);
    for (int w = 0; w < P->n_windows; w++) lab_off[w] = (int64_t)w * chunk_len;
    return decode_and_fetch(ctx, ctx->ws_probs.p, f16 ? 2 : 0, P->off1.data(), P->valid.data(), P->n_windows, beam_width, 0, 0.0, 0.0,
                            labels_out, lab_off.data(), label_len, nullptr, P->off2.data(), P->split.data());
}

// forward only, at the reads level: the streamed evaluation (every time step once + the window heads in chunk mode) of a batch of
// normalised reads resident in HBM, on forward lane `lane`, asynchronous.  The probability rows land in the context's workspace
// (row layout of the plan: DESIGN.md 4.6); *total_rows (nullable) receives their number.
extern "C" int rd_forward_reads_resident(rd_ctx* ctx, const float* d_signal, const int64_t* read_off, int n_reads, int chunk_len,
                                         int step, int decode_type, int lane, int64_t* total_rows)
{
    int rc = rd_check_reads_args(ctx, d_signal, read_off, n_reads, chunk_len, step, 1);
    if (rc) return rc;
    RD_REQUIRE(decode_type == 0 || decode_type == 1, "rd_forward_reads_resident: decode_type %d (0 = chunk plan, 1 = global plan)", decode_type);
    RD_REQUIRE(lane >= 0 && lane < RD_MAX_LANES, "rd_forward_reads_resident: lane %d out of range [0,%d)", lane, RD_MAX_LANES);
    RD_HIP(hipSetDevice(ctx->device));
    const ReadsPlan* P = nullptr;
    const TileLists* tl = nullptr;
    if ((rc = get_plan(ctx, read_off, n_reads, chunk_len, step, decode_type, &P, &tl, nullptr))) return rc;
    if (ctx->ws_probs.reserve((size_t)P->total_rows * 20)) return RD_ERR_NOMEM;
    if (total_rows) *total_rows = P->total_rows;
    return rd_forward_tiles_dev(ctx, d_signal, *tl, P->total_rows, ctx->ws_probs.p, lane, ctx->logits_f16);
}

// sig_model.predict for the windows of whole reads (basecall.py:83-93) through the streamed evaluation: host signal in, window-shaped
// probabilities out -- bit-identical to rd_forward on the same reads' windows for the rows basecall.py:96 keeps.
extern "C" int rd_forward_reads(rd_ctx* ctx, const float* signal, const int64_t* read_off, int n_reads, int chunk_len, int step,
                                float* probs_out, int64_t windows_cap, int64_t* n_windows)
{
    int rc = rd_check_reads_args(ctx, signal, read_off, n_reads, chunk_len, step, 1);
    if (rc) return rc;
    RD_REQUIRE(probs_out && n_windows, "rd_forward_reads: null output");
    RD_REQUIRE(!ctx->logits_f16, "rd_forward_reads: float32 rows only (rd_set_logits 0)");
    RD_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)read_off[n_reads];
    if (ctx->ws_in.reserve(n * 4 + 16)) return RD_ERR_NOMEM;
    RD_HIP(hipMemcpyAsync(ctx->ws_in.p, signal, n * 4, hipMemcpyHostToDevice, ctx->stream));
    const ReadsPlan* P = nullptr;
    const TileLists* tl = nullptr;
    if ((rc = get_plan(ctx, read_off, n_reads, chunk_len, step, 0, &P, &tl, nullptr))) return rc;
    *n_windows = P->n_windows;
    RD_REQUIRE(P->n_windows <= windows_cap, "rd_forward_reads: %d windows, room for %lld", P->n_windows, (long long)windows_cap);
    if (ctx->ws_probs.reserve((size_t)P->total_rows * 20)) return RD_ERR_NOMEM;
    if ((rc = rd_forward_tiles_dev(ctx, ctx->ws_in.as<float>(), *tl, P->total_rows, ctx->ws_probs.p, 0, 0))) return rc;
    const size_t nw = (size_t)P->n_windows, a8 = align_up(nw * 8, 256), a4 = align_up(nw * 4, 256);
    const size_t out_bytes = nw * chunk_len * 20;
    if (ctx->ws_misc.reserve(2 * a8 + 2 * a4) || ctx->ws_mat.reserve(out_bytes + 16)) return RD_ERR_NOMEM;
    char* dm = (char*)ctx->ws_misc.p;
    RD_HIP(hipMemcpyAsync(dm, P->off1.data(), nw * 8, hipMemcpyHostToDevice, ctx->stream));
    RD_HIP(hipMemcpyAsync(dm + a8, P->off2.data(), nw * 8, hipMemcpyHostToDevice, ctx->stream));
    RD_HIP(hipMemcpyAsync(dm + 2 * a8, P->split.data(), nw * 4, hipMemcpyHostToDevice, ctx->stream));
    RD_HIP(hipMemcpyAsync(dm + 2 * a8 + a4, P->valid.data(), nw * 4, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = rd_gather_windows_dev(ctx->stream, ctx->ws_probs.as<float>(), (const int64_t*)dm, (const int64_t*)(dm + a8), (const int32_t*)(dm + 2 * a8),
                                    (const int32_t*)(dm + 2 * a8 + a4), P->n_windows, chunk_len, (float*)ctx->ws_mat.p)))
        return rc;
    RD_HIP(hipMemcpyAsync(probs_out, ctx->ws_mat.p, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    RD_HIP(hipStreamSynchronize(ctx->stream));
    return RD_OK;
}

extern "C" int rd_basecall_reads_chunk(rd_ctx* ctx, const float* signal, const int64_t* read_off, int n_reads, int chunk_len,
                                       int step, int beam_width, uint8_t* labels_out, int32_t* label_len)
{
    int rc = rd_check_reads_args(ctx, signal, read_off, n_reads, chunk_len, step, beam_width);
    if (rc) return rc;
    RD_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)read_off[n_reads];
    if (ctx->ws_in.reserve(n * 4 + 16)) return RD_ERR_NOMEM;
    RD_HIP(hipMemcpyAsync(ctx->ws_in.p, signal, n * 4, hipMemcpyHostToDevice, ctx->stream));
    return rd_basecall_reads_chunk_resident(ctx, ctx->ws_in.as<float>(), read_off, n_reads, chunk_len, step, beam_width, labels_out,
                                            label_len);
}

static int reads_global_resident(rd_ctx* ctx, const float* d_signal, const int64_t* read_off, int n_reads, int chunk_len, int step, int beam_width,
                                 int use_lm, double s_thr, double r_thr, uint8_t* labels_out, const int64_t* label_off, int32_t* label_len,
                                 AlignOut* ao)
{
    int rc = rd_check_reads_args(ctx, d_signal, read_off, n_reads, chunk_len, step, beam_width);
    if (rc) return rc;
    RD_REQUIRE(labels_out && label_off && label_len, "rd_basecall_reads_global: null output");
    RD_REQUIRE_WIDTH_LM(ctx, beam_width, use_lm);
    RD_HIP(hipSetDevice(ctx->device));
    const ReadsPlan* P = nullptr;
    const TileLists* tl = nullptr;
    bool streamed = false;
    if ((rc = get_plan(ctx, read_off, n_reads, chunk_len, step, 1, &P, &tl, &streamed))) return rc;
    if (ctx->ws_probs.reserve((size_t)P->total_rows * 20)) return RD_ERR_NOMEM;
    const int f16 = ctx->logits_f16;
    rc = rd_forward_tiles_dev(ctx, d_signal, *tl, P->total_rows, ctx->ws_probs.p, 0, f16);
    if (rc) return rc;
    return global_finish(ctx, ctx->ws_probs.p, f16, streamed, P->read_win_off.data(), P->valid.data(), P->read_row.data(), read_off, n_reads, chunk_len,
                         step, beam_width, use_lm, s_thr, r_thr, labels_out, label_off, label_len, ao);
}

extern "C" int rd_basecall_reads_global_resident(rd_ctx* ctx, const float* d_signal, const int64_t* read_off, int n_reads,
                                                 int chunk_len, int step, int beam_width, int use_lm, double s_thr, double r_thr,
                                                 uint8_t* labels_out, const int64_t* label_off, int32_t* label_len)
{
    return reads_global_resident(ctx, d_signal, read_off, n_reads, chunk_len, step, beam_width, use_lm, s_thr, r_thr, labels_out, label_off, label_len,
                                 nullptr);
}

extern "C" int rd_basecall_reads_global(rd_ctx* ctx, const float* signal, const int64_t* read_off, int n_reads, int chunk_len,
                                        int step, int beam_width, int use_lm, double s_thr, double r_thr, uint8_t* labels_out,
                                        const int64_t* label_off, int32_t* label_len)
{
    int rc = rd_check_reads_args(ctx, signal, read_off, n_reads, chunk_len, step, beam_width);
    if (rc) return rc;
    RD_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)read_off[n_reads];
    if (ctx->ws_in.reserve(n * 4 + 16)) return RD_ERR_NOMEM;
    RD_HIP(hipMemcpyAsync(ctx->ws_in.p, signal, n * 4, hipMemcpyHostToDevice, ctx->stream));
    return rd_basecall_reads_global_resident(ctx, ctx->ws_in.as<float>(), read_off, n_reads, chunk_len, step, beam_width, use_lm,
                                             s_thr, r_thr, labels_out, label_off, label_len);
}

// ---- raw int16 reads in: normalisation on the device, then the reads-level paths --------------------------------
namespace {

// uploads raw samples + offsets, runs mad_normalise_kernel into ctx->ws_in, returns per-read status on the host
int normalise_upload(rd_ctx* ctx, const int16_t* raw, const int64_t* read_off, int n_reads, int clip, int32_t* status)
{
    RD_REQUIRE(ctx && raw && read_off && status, "null argument");
    RD_REQUIRE(n_reads >= 1 && read_off[0] == 0, "bad read offsets");
    for (int r = 0; r < n_reads; r++) RD_REQUIRE(read_off[r + 1] >= read_off[r], "read offsets must be non-decreasing");
    RD_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)read_off[n_reads];
    const size_t o_off = align_up(n * 2 + 16, 256), o_st = o_off + align_up((size_t)(n_reads + 1) * 8, 256);
    if (ctx->ws_raw.reserve(o_st + (size_t)n_reads * 4 + 16) || ctx->ws_in.reserve(n * 4 + 16)) return RD_ERR_NOMEM;
    char* base = (char*)ctx->ws_raw.p;
    if (n) RD_HIP(hipMemcpyAsync(base, raw, n * 2, hipMemcpyHostToDevice, ctx->stream));
    RD_HIP(hipMemcpyAsync(base + o_off, read_off, (size_t)(n_reads + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    int rc = rd_normalise_dev(ctx, (const int16_t*)base, (const int64_t*)(base + o_off), n_reads, clip, ctx->ws_in.as<float>(),
                              (int32_t*)(base + o_st));
    if (rc) return rc;
    RD_HIP(hipMemcpyAsync(status, base + o_st, (size_t)n_reads * 4, hipMemcpyDeviceToHost, ctx->stream));
    RD_HIP(hipStreamSynchronize(ctx->stream));
    return RD_OK;
}

}  // namespace

extern "C" int rd_normalise_reads(rd_ctx* ctx, const int16_t* raw, const int64_t* read_off, int n_reads, int outlier_clip,
                                  float* norm_out, int32_t* status)
{
    int rc = normalise_upload(ctx, raw, read_off, n_reads, outlier_clip, status);
    if (rc) return rc;
    const size_t n = (size_t)read_off[n_reads];
    if (norm_out && n) {
        RD_HIP(hipMemcpyAsync(norm_out, ctx->ws_in.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
        RD_HIP(hipStreamSynchronize(ctx->stream));
    }
    return RD_OK;
}

extern "C" int rd_basecall_raw_chunk(rd_ctx* ctx, const int16_t* raw, const int64_t* read_off, int n_reads, int outlier_clip,
                                     int chunk_len, int step, int beam_width, uint8_t* labels_out, int32_t* label_len,
                                     int32_t* status)
{
    int rc = normalise_upload(ctx, raw, read_off, n_reads, outlier_clip, status);
    if (rc) return rc;
    for (int r = 0; r < n_reads; r++)
        RD_REQUIRE(status[r] != 2, "rd_basecall_raw_chunk: read %d is empty (the caller skips empty reads, basecall.py:77-82)", r);
    return rd_basecall_reads_chunk_resident(ctx, ctx->ws_in.as<float>(), read_off, n_reads, chunk_len, step, beam_width, labels_out,
                                            label_len);
}

extern "C" int rd_basecall_raw_global(rd_ctx* ctx, const int16_t* raw, const int64_t* read_off, int n_reads, int outlier_clip,
                                      int chunk_len, int step, int beam_width, int use_lm, double s_thr, double r_thr,
                                      uint8_t* labels_out, const int64_t* label_off, int32_t* label_len, int32_t* status)
{
    int rc = normalise_upload(ctx, raw, read_off, n_reads, outlier_clip, status);
    if (rc) return rc;
    for (int r = 0; r < n_reads; r++)
        RD_REQUIRE(status[r] != 2, "rd_basecall_raw_global: read %d is empty (the caller skips empty reads, basecall.py:77-82)", r);
    return rd_basecall_reads_global_resident(ctx, ctx->ws_in.as<float>(), read_off, n_reads, chunk_len, step, beam_width, use_lm,
                                             s_thr, r_thr, labels_out, label_off, label_len);
}

// rd_basecall_raw_global plus, per read, the forced alignment of its labels against the rows its beam search read (ctcalign.hip)
extern "C" int rd_basecall_raw_global_q(rd_ctx* ctx, const int16_t* raw, const int64_t* read_off, int n_reads, int outlier_clip,
                                        int chunk_len, int step, int beam_width, int use_lm, double s_thr, double r_thr,
                                        uint8_t* labels_out, const int64_t* label_off, int32_t* label_len, int32_t* status, int64_t budget_bytes,
                                        uint8_t* qual_out, int32_t* first_step_out, int32_t* last_step_out, double* score_out, int32_t* align_status)
{
    RD_REQUIRE(qual_out && first_step_out && last_step_out && score_out && align_status, "rd_basecall_raw_global_q: null output");
    RD_REQUIRE(budget_bytes >= 0, "rd_basecall_raw_global_q: negative budget");
    int rc = normalise_upload(ctx, raw, read_off, n_reads, outlier_clip, status);
    if (rc) return rc;
    for (int r = 0; r < n_reads; r++)
        RD_REQUIRE(status[r] != 2, "rd_basecall_raw_global_q: read %d is empty (the caller skips empty reads, basecall.py:77-82)", r);
    AlignOut ao{budget_bytes, first_step_out, last_step_out, qual_out, score_out, align_status};
    rc = reads_global_resident(ctx, ctx->ws_in.as<float>(), read_off, n_reads, chunk_len, step, beam_width, use_lm, s_thr, r_thr, labels_out, label_off,
                               label_len, &ao);
    if (rc) return rc;
    return ao.too_large ? RD_ERR_NOMEM : RD_OK;   // (rd_last_error names the first read over the budget)
}

// "Resquiggle": rd_basecall_raw_global_q's rows, GIVEN labels instead of a beam search, and the event table of the alignment
// (events.hip) from the raw samples normalise_upload left on the device
extern "C" int rd_resquiggle_raw(rd_ctx* ctx, const int16_t* raw, const int64_t* read_off, int n_reads, int outlier_clip, int chunk_len, int step,
                                 const uint8_t* ref_labels, const int64_t* ref_off, const int32_t* ref_len, int64_t budget_bytes,
                                 int32_t* first_step, int32_t* last_step, uint8_t* qual, double* score, int32_t* align_status, int32_t* read_status,
                                 int32_t* ev_start, int32_t* ev_end, int64_t* ev_sum, int64_t* ev_sumsq, int16_t* ev_min, int16_t* ev_max)
{
    RD_REQUIRE(ctx && ref_off && ref_len && score && align_status && read_status, "rd_resquiggle_raw: null argument");
    RD_REQUIRE(n_reads >= 1, "rd_resquiggle_raw: bad shape");
    RD_REQUIRE(budget_bytes >= 0, "rd_resquiggle_raw: negative budget");
    int64_t labs = 0, labs_end = 0;
    std::vector<int64_t> dlab(n_reads);
    for (int r = 0; r < n_reads; r++) {
        RD_REQUIRE(ref_len[r] >= 0 && ref_len[r] < (1 << 29), "rd_resquiggle_raw: read %d has %d labels", r, ref_len[r]);
        RD_REQUIRE(ref_off[r] >= labs_end, "rd_resquiggle_raw: label offsets must be non-decreasing and the reads' labels must not overlap (read %d)", r);
        labs_end = ref_off[r] + ref_len[r];
        dlab[r] = labs;
        labs += ref_len[r];
    }
    RD_REQUIRE(labs == 0 || (ref_labels && first_step && last_step && qual && ev_start && ev_end && ev_sum && ev_sumsq && ev_min && ev_max),
               "rd_resquiggle_raw: null label or per-base buffer");
    for (int r = 0; r < n_reads; r++)
        for (int k = 0; k < ref_len[r]; k++)
            RD_REQUIRE(ref_labels[ref_off[r] + k] < 4, "rd_resquiggle_raw: label %d of read %d is %d, not in 0..3", k, r, ref_labels[ref_off[r] + k]);
    int rc = normalise_upload(ctx, raw, read_off, n_reads, outlier_clip, read_status);
    if (rc) return rc;
    for (int r = 0; r < n_reads; r++)
        RD_REQUIRE(read_status[r] != 2, "rd_resquiggle_raw: read %d is empty (the caller skips empty reads, basecall.py:77-82)", r);
    if ((rc = rd_check_reads_args(ctx, ctx->ws_in.p, read_off, n_reads, chunk_len, step, 1))) return rc;
    const ReadsPlan* P = nullptr;
    const TileLists* tl = nullptr;
    bool streamed = false;
    if ((rc = get_plan(ctx, read_off, n_reads, chunk_len, step, 1, &P, &tl, &streamed))) return rc;
    if (ctx->ws_probs.reserve((size_t)P->total_rows * 20)) return RD_ERR_NOMEM;
    const int f16 = ctx->logits_f16;
    if ((rc = rd_forward_tiles_dev(ctx, ctx->ws_in.as<float>(), *tl, P->total_rows, ctx->ws_probs.p, 0, f16))) return rc;
    std::vector<ReadRows> rr;
    if ((rc = global_rows(ctx, ctx->ws_probs.p, f16, streamed, P->read_win_off.data(), P->valid.data(), P->read_row.data(), read_off, n_reads, chunk_len,
                          step, rr)))
        return rc;
    // the labels, packed
    if (ctx->ws_labels.reserve((size_t)labs + 16)) return RD_ERR_NOMEM;
    std::vector<uint8_t> hl((size_t)labs + 16);
    for (int r = 0; r < n_reads; r++)
        if (ref_len[r]) memcpy(hl.data() + dlab[r], ref_labels + ref_off[r], (size_t)ref_len[r]);
    if (labs) RD_HIP(hipMemcpyAsync(ctx->ws_labels.p, hl.data(), (size_t)labs, hipMemcpyHostToDevice, ctx->stream));
    // two alignment calls: float64 (assembled) reads and float32 / f16 (single-coverage) reads
    bool too_large = false;
    for (int r = 0; r < n_reads; r++) {
        if (read_status[r] == 0) continue;
        align_status[r] = RD_CTCALIGN_NO_PATH;   // normalisation refused the read: nothing is aligned
        score[r] = -INFINITY;
        for (int k = 0; k < ref_len[r]; k++) {
            first_step[ref_off[r] + k] = last_step[ref_off[r] + k] = -1;
            qual[ref_off[r] + k] = 0;
        }
    }
    for (int pass = 0; pass < 2; pass++) {
        std::vector<int64_t> so, lo, oo;
        std::vector<int32_t> sl, ll;
        std::vector<int> idx;
        for (int r = 0; r < n_reads; r++)
            if (rr[r].is64 == (pass == 0) && read_status[r] == 0) {
                so.push_back(pass == 0 ? rr[r].row64 : P->read_row[r]);
                sl.push_back((int32_t)rr[r].N);
                lo.push_back(dlab[r]);
                ll.push_back(ref_len[r]);
                oo.push_back(ref_off[r]);
                idx.push_back(r);
            }
        if (idx.empty()) continue;
        std::vector<int32_t> ast(idx.size());
        std::vector<double> asc(idx.size());
        rc = rd_ctc_align_dev(ctx, ctx->stream, pass == 0 ? (const void*)ctx->ws_mat.p : ctx->ws_probs.p, pass == 0 ? 1 : (f16 ? 2 : 0), so.data(),
                              sl.data(), (int)idx.size(), ctx->ws_labels.as<uint8_t>(), lo.data(), ll.data(), budget_bytes, first_step, last_step, qual,
                              oo.data(), asc.data(), ast.data());
        bool tl_here = false;
        for (size_t i = 0; i < idx.size(); i++) tl_here |= ast[i] == RD_CTCALIGN_TOO_LARGE;
        if (rc == RD_ERR_NOMEM && tl_here) too_large = true;
        else if (rc) return rc;
        for (size_t i = 0; i < idx.size(); i++) {
            score[idx[i]] = asc[i];
            align_status[idx[i]] = ast[i];
        }
    }
    RD_HIP(hipStreamSynchronize(ctx->stream));   // (hl is read by the label upload when nothing was launched)
    rc = rd_event_stats_steps(ctx, ctx->stream, (const int16_t*)ctx->ws_raw.p, read_off, n_reads, first_step, last_step, ref_off, ref_len, align_status,
                              labs_end, ev_start, ev_end, ev_sum, ev_sumsq, ev_min, ev_max);
    if (rc) return rc;
    return too_large ? RD_ERR_NOMEM : RD_OK;   // (rd_last_error names the first read over the budget)
}
