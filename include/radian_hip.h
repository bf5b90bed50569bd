/*
 * radian_hip.h -- C ABI of libradian_hip.so: the MI355X (gfx950) backend for RADIAN's
 * inference + decode hot path.
 *
 * The reference (comprna/radian) has no FFI; the seam is five in-process Python calls made by
 * radian/basecall.py.  Each entry point below names the reference call it replaces (file:line under
 * the reference tree).  INTEGRATION.md shows the ctypes binding a maintainer adds to basecall.py.
 * This header lists what a RADIAN maintainer binds and nothing else: the measurement switches, kernel timers and pipeline
 * read-outs that bench.py, tools/ and tests/ use live in radian_hip_diag.h (same library; none of them changes a result).
 *
 * Conventions
 *   - every function returns 0 on success or a negative RD_ERR_* code; rd_last_error() then returns
 *     a thread-local human-readable message.  Nothing is thrown, nothing calls back into the host.
 *   - all pointers are caller-owned HOST memory unless the parameter name starts with d_ (device
 *     memory obtained from rd_dev_alloc).  Plain pointers and sizes only; no framework types.
 *   - one rd_ctx per process and per GPU rank; calls on one context are not thread-safe.
 *   - class order of probability rows is A, C, G, T, blank (radian/models/sig2seq.yaml:2;
 *     radian/decode.py:124); labels are 0..3 = A,C,G,T and are NOT reversed (basecall.py:129
 *     reverses the string on the host).
 *   - there is no CPU fallback: without a GPU rd_create fails.
 */
#ifndef RADIAN_HIP_H
#define RADIAN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RD_OK 0
#define RD_ERR_ARG (-1)   /* bad argument */
#define RD_ERR_HIP (-2)   /* HIP runtime error */
#define RD_ERR_STATE (-3) /* call order (e.g. forward before weights) */
#define RD_ERR_NOMEM (-4) /* device allocation failed */
#define RD_ERR_RCCL (-5)  /* RCCL error / librccl not loadable */
#define RD_ERR_FORMAT (-6) /* rd_lm_json_* / rd_fast5_*: the input is not of the one shape the fast reader handles (no verdict: use the full parser / libhdf5); rd_tfrecord_*: the shard is malformed */
#define RD_ERR_IO (-7)     /* rd_fast5_open / rd_tfrecord_open: the file cannot be opened or mapped */
/* Not an error code: the value of label_len[i] for a sequence whose beam search looked up a context that a SPARSE RNA model
 * does not hold (rd_load_lm, rows of NaN).  The reference raises KeyError at radian/decode.py:83 on such a read; the caller
 * does the same when it reaches that read (radian_amd/basecall.py).  The sequence's labels are not written. */
#define RD_LEN_MISSING_CONTEXT (-1)

typedef struct rd_ctx rd_ctx;

/* ---- library ------------------------------------------------------------------------------- */
const char* rd_last_error(void);
int rd_version(void);                 /* ABI version, currently 1 */
int rd_device_count(int* n);          /* number of visible HIP devices */
int rd_decode_max_width(void);        /* largest supported --beam-width (1024; radian/decode.py:145 slices with any width) */
int rd_decode_lane_width(void);       /* widths up to this (256) run on the wave-per-sequence kernels, wider ones on the general kernel */

/* ---- context ------------------------------------------------------------------------------- */
int rd_create(int device_id, rd_ctx** out);
int rd_destroy(rd_ctx* ctx);
int rd_sync(rd_ctx* ctx);             /* wait for the context's stream */
/* Matrix-product arithmetic of the forward (sig_model.predict, radian/basecall.py:88-93; the reference computes in fp32):
 *   0 (default) exact fp32 MFMA;
 *   1 split-f16 "f16x3": every fp32 operand carried as an f16 hi+lo pair (22 significant bits), products
 *     hi*hi + hi*lo + lo*hi accumulated in fp32 on the f16 matrix pipe;
 *   2 three-term bf16 split "bf16x3": every fp32 operand carried EXACTLY as hi+mid+lo bf16 (3 x 8 significant bits,
 *     fp32's exponent range), the six cross products down to 2^-16 relative accumulated in fp32 on the bf16 matrix pipe;
 *     the dropped terms are below one fp32 rounding of the product. */
int rd_set_precision(rd_ctx* ctx, int mode);

/* ---- model artefacts ----------------------------------------------------------------------- */
/* Replaces model.load_weights(checkpoint) -- radian/model.py:42-45.
 * blob = rd_weights_header followed by float32 tensors in Keras load_weights order and layouts:
 *   block0: conv0.kernel[K][1][C], conv0.bias[C], conv1.kernel[K][C][C], conv1.bias[C],
 *           matching.kernel[1][1][C], matching.bias[C];
 *   block i>0: conv0.kernel[K][C][C], bias[C], conv1.kernel[K][C][C], bias[C];
 *   dense.kernel[C][H], dense.bias[H]; dense_1.kernel[H][5], dense_1.bias[5].
 * Geometry is fixed to radian/models/sig2seq.yaml:34-49 (C=256, K=3, H=128, 5 classes); the number
 * of blocks and their dilations come from the header. */
typedef struct rd_weights_header {
    uint32_t magic;      /* 'RDNW' = 0x574e4452 */
    uint32_t version;    /* 1 */
    uint32_t nb_filters; /* 256 */
    uint32_t kernel_size;/* 3 */
    uint32_t relu_units; /* 128 */
    uint32_t n_classes;  /* 5 */
    uint32_t n_blocks;   /* len(dilations) * nb_stacks, <= 16 */
    uint32_t dilations[16];
    uint32_t n_floats;   /* number of float32 values that follow */
} rd_weights_header;
int rd_load_weights(rd_ctx* ctx, const void* blob, size_t nbytes);

/* Replaces the RNA-model dict built at radian/basecall.py:48-57 and read at decode.py:83.
 * table[ctx][4] doubles, ctx = base-4 number of the k context labels, oldest label most
 * significant (the JSON key string read left to right).  k = --context-len, 1..13.
 * A row of NaNs marks a context the model does NOT hold (a sparse JSON): the reference's dict lookup raises KeyError
 * when -- and only when -- the search of a read keeps a labeling that ends in such a context (decode.py:83, looked up
 * for every kept labeling of >= k labels at every time step, whatever the gate says); here that read's label_len comes
 * back as RD_LEN_MISSING_CONTEXT and every other read is unaffected.
 * Passing table == NULL unloads the LM. */
int rd_load_lm(rd_ctx* ctx, const double* table, int k);
/* --context-len k (1..13) with an RNA model whose keys have another length: the reference's `model[context]` (decode.py:83) then
 * raises KeyError for EVERY context, i.e. on the first read whose search keeps a labeling of >= k labels before its last time step,
 * after having basecalled the shorter reads before it (basecall.py:70-141).  Loads that model: every read that reaches such a
 * labeling comes back as RD_LEN_MISSING_CONTEXT, every other read decodes as without an LM (no lookup ever succeeds). */
int rd_load_lm_absent(rd_ctx* ctx, int k);
/* Long contexts (--context-len up to 256; BASELINE configs[4]).  NO reference behaviour: the reference needs one dict
 * entry per context (decode.py:83), impossible beyond a dozen labels.  A synthetic LM for such contexts is a dense
 * table[4^table_order][4] addressed by a hash of the context: row = H(l_0..l_{k-1}) & (4^table_order - 1),
 * H = sum l_i * B^(k-1-i) mod 2^32, B = 0x9E3779B1; gate and mixing as decode.py:79-96.  The decoder keeps the hash
 * incrementally per beam with a 256-label ring (the label leaving the window).  Parity: the oracle's same definition. */
int rd_load_lm_hashed(rd_ctx* ctx, const double* table, int table_order, int context_len);
/* Storage type of the softmax rows between the head kernel and the decoder on the reads-level paths
 * (rd_basecall_reads_*, rd_basecall_raw_*, rd_pipe_submit_reads): 0 float32 (the reference's, default), 1 float16
 * (10 B per time step; rounded to nearest by the head kernel, widened exactly by the decoder / assembly).  Not a
 * reference option (BASELINE configs[4] "fp16 logits"): labels equal the oracle's on the same f16-rounded rows. */
int rd_set_logits(rd_ctx* ctx, int mode);
/* Decode partition of the global-mode reads pipeline (rd_pipe_submit_reads_global / rd_pipe_submit_raw_global; no effect on
 * results, no reference counterpart): cus_per_xcd CUs of each of the 8 XCDs are kept free of forward workgroups (the
 * pipeline's forward streams are CU-masked to the others) and run the beam search.  A read's search is one serial chain of
 * a time step per sample; a beam-search wave that shares its SIMD with conv waves issuing MFMAs back to back gets about one
 * instruction issue per MFMA (17 us per step measured instead of 2).  -1 (default) = by beam width (4 CUs per XCD, 8 above
 * W = 25, 12 above W = 64, 16 above W = 128: 12.5 ... 50 % of the chip; a masked queue's CUs are dealt over the four shader engines of an XCD and the forward
 * runs at the pace of the engine left with the fewest, so only multiples of four are worth setting), 0 = off (groups then
 * grow until their forward rows cover the slow chain). */
int rd_set_decode_partition(rd_ctx* ctx, int cus_per_xcd);
/* Arithmetic of the beam search's log / logaddexp (decode.py:16-17,172-201 call math.log and np.logaddexp, i.e. the host's
 * libm): 1 (default) = the operation sequence of glibc 2.35's x86-64 FMA build (exp, log, log1p restated in
 * csrc/glibc_math.h): scores and labelings bit-identical to the reference's on such a host, including labelings that are
 * equiprobable in exact arithmetic; 0 = this library's faster routines (<= 1 ulp from glibc's, so scores agree to a few ulp
 * and labelings are identical unless two labelings tie within that distance; the beam search runs 10 % (peaked rows,
 * thousands of sequences) to 35 % (flat rows, few sequences) faster). */
int rd_set_decode_math(rd_ctx* ctx, int mode);
/* Window heads of the chunk-mode reads paths (the rows of windows i >= 1 that see their window's zero left-padding): 1 (default) =
 * evaluated as packed classes of rows that leave out the conv taps lying wholly in the padding, 0 = as tiles of their own that
 * multiply the padding's zeros.  No effect on results (equal under IEEE comparison: a left-out product is fma(0, w, acc); the sign
 * of a zero may differ).  Packing applies to the exact-fp32 mode with weights whose conv kernels are finite and whose conv biases
 * are not -0.0, as rd_load_weights saw them: after a training step (rd_train_*) the context runs head tiles until weights are
 * loaded again.  rd_head_pack_active says whether the context's next chunk-mode forward will pack (1 / 0); rd_head_pack_tiles how
 * many packed workgroup tiles the context's latest forward launched (0: it ran head tiles, or had no heads). */
int rd_set_head_pack(rd_ctx* ctx, int on);
int rd_head_pack_active(rd_ctx* ctx);
int64_t rd_head_pack_tiles(rd_ctx* ctx);
/* Input staging of the exact-fp32 conv launches behind block 0 (128-row workgroup shape, dilation <= 32): 1 = a workgroup tile that
 * lies wholly inside one segment (a "slab tile": 128 consecutive interior rows of a window or read, nothing redirected to the read's
 * stream) copies the 128 + 2 dilation input rows its three taps share into LDS once per 16-channel slice (default), 0 = every tap
 * copies its own 128 shifted rows.  Same bits: the products and their order are unchanged.  Every other tile runs the per-tap staging
 * under either setting.  rd_conv_slab_active says whether the context's next forward will take the slab path (1 / 0: the setting, exact
 * fp32, 128-row shape); rd_conv_slab_tiles how many slab tiles the context's latest forward launched, over all its conv launches. */
int rd_set_conv_slab(rd_ctx* ctx, int on);
int rd_conv_slab_active(rd_ctx* ctx);
int64_t rd_conv_slab_tiles(rd_ctx* ctx);

/* ---- the five seams, host-pointer form ----------------------------------------------------- */
/* sig_model.predict(windows) -- radian/basecall.py:91,93.
 * windows [n_windows][chunk_len] float32 (MAD-normalised) -> probs [n_windows][chunk_len][5] float32. */
int rd_forward(rd_ctx* ctx, const float* windows, int n_windows, int chunk_len, float* probs);

/* assemble_matrices(matrices, step_size) after matrices[-1] = matrices[-1][:-pad]
 * -- radian/basecall.py:96,100; radian/matrix_assembly.py:6-53.
 * probs [n_windows][chunk_len][5] float32 of ONE read; out receives [*n_rows][5] float64
 * (capacity out_cap rows); *is_f64 reports the reference's result dtype (float64 when any time step
 * is covered by more than one window, else float32 -- the values are exact either way). */
int rd_assemble(rd_ctx* ctx, const float* probs, int n_windows, int chunk_len, int pad, int step, double* out,
                int64_t out_cap, int64_t* n_rows, int* is_f64);

/* beam_search(mat, 'ACGT', beam_width, lm, s_threshold, r_threshold, len_context, cache)
 * -- radian/basecall.py:102-109 (global) and :113-120 (chunk); radian/decode.py:100-212.
 * A batch of independent sequences over concatenated probability rows:
 *   probs      rows [*][5], float32 (prob_is_f64=0) or float64 (1)
 *   seq_off[i] first row of sequence i, seq_len[i] its number of rows (0 allowed)
 *   use_lm     0: lm=None (chunk mode); 1: use the table from rd_load_lm with thresholds s_thr/r_thr
 *   labels_out receives sequence i's labels at labels_out + label_off[i] (capacity >= seq_len[i]),
 *   label_len[i] its length; best_score (nullable) the winner's log pr_total. */
int rd_decode_batch(rd_ctx* ctx, const void* probs, int prob_is_f64, const int64_t* seq_off, const int32_t* seq_len,
                    int n_seq, int beam_width, int use_lm, double s_thr, double r_thr, uint8_t* labels_out,
                    const int64_t* label_off, int32_t* label_len, double* best_score);

/* ---- fused paths (probabilities never leave HBM) ------------------------------------------- */
/* chunk mode, radian/basecall.py:86-96,110-121 for a batch of windows that may span many reads:
 * forward, then an LM-free beam search of each window over its first valid_len[i] rows
 * (chunk_len, or chunk_len - pad for the last window of a read).  Labels of window i are written
 * at labels_out + i*chunk_len.  simple_assembly (basecall.py:122-123) stays on the host. */
int rd_basecall_chunk(rd_ctx* ctx, const float* windows, int n_windows, int chunk_len, const int32_t* valid_len,
                      int beam_width, uint8_t* labels_out, int32_t* label_len);

/* global mode, radian/basecall.py:86-109 for a batch of reads: forward over all windows, per-read
 * assembly, one LM-gated beam search per read.
 *   read_win_off[r] first window of read r (n_reads+1 entries), pad[r] the zero padding of its last
 *   window, step the window step; labels of read r at labels_out + label_off[r]
 *   (capacity >= assembled length = (nW_r-1)*step + chunk_len - pad[r]). */
int rd_basecall_global(rd_ctx* ctx, const float* windows, int chunk_len, int step, const int32_t* read_win_off,
                       const int32_t* pad, int n_reads, int beam_width, int use_lm, double s_thr, double r_thr,
                       uint8_t* labels_out, const int64_t* label_off, int32_t* label_len);

/* ---- reads-level fused paths: windowing happens on the device and each time step is computed once ------------
 * The loop body of radian/basecall.py:83-121 for a batch of whole reads.  signal = the reads' MAD-normalised samples
 * (basecall.py:78) packed back to back, read r at [read_off[r], read_off[r+1]) (n_reads+1 offsets, read_off[0] = 0).
 * Windows are those of get_windows(signal, chunk_len, step) (preprocess.py:4-22).  The causal TCN is evaluated once
 * over each read ("stream"); a window's rows past the receptive field are the stream's rows and only its first
 * RF-1 rows are computed separately, so the probabilities -- and the labels -- are bit-identical to the windowed
 * computation at a fraction of the work.
 *   chunk : labels of window w (counted across the batch, rd_count_windows per read) at labels_out + w*chunk_len,
 *           label_len[w]; simple_assembly stays on the host.
 *   global: labels of read r at labels_out + label_off[r] (capacity >= its number of samples), label_len[r]. */
int rd_count_windows(int64_t n_samples, int chunk_len, int step);   /* windows get_windows makes of one read */
int rd_basecall_reads_chunk(rd_ctx* ctx, const float* signal, const int64_t* read_off, int n_reads, int chunk_len,
                            int step, int beam_width, uint8_t* labels_out, int32_t* label_len);
int rd_basecall_reads_global(rd_ctx* ctx, const float* signal, const int64_t* read_off, int n_reads, int chunk_len,
                             int step, int beam_width, int use_lm, double s_thr, double r_thr, uint8_t* labels_out,
                             const int64_t* label_off, int32_t* label_len);

/* ---- the step before the hot path on the device: mad_normalise -- radian/preprocess.py:24-49, basecall.py:78 ----
 * raw = unscaled int16 DAQ samples of the reads packed back to back (read r at [read_off[r], read_off[r+1])).
 * status[r]: 0 ok; 1 "MAD is zero, issue with signal." (output zeros); 2 "Signal must not be empty to normalise" --
 * the two ValueErrors after which basecall.py:77-82 skips the read.  Output = float32(mad_normalise(raw, clip)),
 * bit-identical to NumPy (exact order statistics, IEEE float64 arithmetic, np.vectorize's int64 quirk included). */
int rd_normalise_reads(rd_ctx* ctx, const int16_t* raw, const int64_t* read_off, int n_reads, int outlier_clip,
                       float* norm_out /* nullable */, int32_t* status);
/* normalise + reads-level chunk / global basecall in one call; reads with status 1 are computed on zeros and must be
 * dropped by the caller, empty reads are rejected (filter them first). */
int rd_basecall_raw_chunk(rd_ctx* ctx, const int16_t* raw, const int64_t* read_off, int n_reads, int outlier_clip,
                          int chunk_len, int step, int beam_width, uint8_t* labels_out, int32_t* label_len, int32_t* status);
int rd_basecall_raw_global(rd_ctx* ctx, const int16_t* raw, const int64_t* read_off, int n_reads, int outlier_clip,
                           int chunk_len, int step, int beam_width, int use_lm, double s_thr, double r_thr,
                           uint8_t* labels_out, const int64_t* label_off, int32_t* label_len, int32_t* status);

/* ---- device-resident form (inputs already in HBM; used by bench.py and by pipelined hosts) -- */
int rd_dev_alloc(rd_ctx* ctx, size_t bytes, void** d_ptr);
int rd_dev_free(rd_ctx* ctx, void* d_ptr);
int rd_mem_info(rd_ctx* ctx, size_t* free_bytes, size_t* total_bytes);   /* hipMemGetInfo of the context's device (batch sizing) */
int rd_memcpy_h2d(rd_ctx* ctx, void* d_dst, const void* src, size_t bytes);
int rd_memcpy_d2h(rd_ctx* ctx, void* dst, const void* d_src, size_t bytes);
/* same contract as rd_forward / rd_basecall_chunk with d_windows resident; d_probs may be NULL
 * (internal workspace).  Asynchronous on the context stream except for the label copy-out. */
int rd_forward_resident(rd_ctx* ctx, const float* d_windows, int n_windows, int chunk_len, float* d_probs);
/* sig_model.predict alone (radian/basecall.py:88-93; BASELINE configs[1] "forward only") for a batch of whole normalised
 * reads resident in HBM: the streamed evaluation of rd_basecall_reads_chunk (decode_type 0: one row per time step + the
 * rows of every window's zero-padded head) or rd_basecall_reads_global (1) without the decode, asynchronous on forward
 * lane `lane` (0..3; lanes are independent streams with their own activations).  Rows go to the context's probability
 * workspace -- ONE workspace per context: calls on several lanes overwrite each other's rows (the entry point exists for the
 * forward's timing, BASELINE configs[1]; rd_forward_reads returns rows); *total_rows (nullable) = their number.  rd_sync
 * waits for every lane. */
int rd_forward_reads_resident(rd_ctx* ctx, const float* d_signal, const int64_t* read_off, int n_reads, int chunk_len,
                              int step, int decode_type, int lane, int64_t* total_rows);
/* The same forward with the reference's shapes: `signal` holds the normalised reads back to back (host), probs_out receives
 * [*n_windows][chunk_len][5] float32 -- what `sig_model.predict(windows)` returns for get_windows() of every read in turn
 * (radian/basecall.py:83-93), window rows the pad trim at basecall.py:96 drops are zero.  Every time step is evaluated once
 * (plus each later window's first 252 rows, which see that window's own zero padding) and the rows are gathered into
 * windows on the device: bit-identical to rd_forward on the same windows.  Blocking. */
int rd_forward_reads(rd_ctx* ctx, const float* signal, const int64_t* read_off, int n_reads, int chunk_len, int step,
                     float* probs_out, int64_t windows_cap, int64_t* n_windows);
int rd_basecall_chunk_resident(rd_ctx* ctx, const float* d_windows, int n_windows, int chunk_len,
                               const int32_t* valid_len, int beam_width, uint8_t* labels_out, int32_t* label_len);
int rd_decode_resident(rd_ctx* ctx, const float* d_probs, int n_windows, int chunk_len, const int32_t* valid_len,
                       int beam_width, uint8_t* labels_out, int32_t* label_len);

/* reads-level forms with the signal resident in HBM */
int rd_basecall_reads_chunk_resident(rd_ctx* ctx, const float* d_signal, const int64_t* read_off, int n_reads,
                                     int chunk_len, int step, int beam_width, uint8_t* labels_out, int32_t* label_len);
int rd_basecall_reads_global_resident(rd_ctx* ctx, const float* d_signal, const int64_t* read_off, int n_reads,
                                      int chunk_len, int step, int beam_width, int use_lm, double s_thr, double r_thr,
                                      uint8_t* labels_out, const int64_t* label_off, int32_t* label_len);

/* Software pipeline over submitted batches inside ONE context -- for a stream of read batches, the loop body of
 * radian/basecall.py:77-121 (mad_normalise, get_windows, predict, assemble_matrices, beam_search).  A submit only queues its
 * batch on the next forward lane (a stream with its own activation tensors; default 2, rd_pipe_set_lanes): [raw form: H2D of
 * the samples out of the lane's pinned staging block, MAD normalisation] -> forward (streamed over whole reads; the windows form:
 * every window's rows) -> [global: per-read assembly].  Consecutive batches' kernel chains on different lanes fill each other's
 * last partial round of workgroups.  Batches gather in a GROUP; a closed group's beam search of every read (global; LM-gated
 * with use_lm) or window (chunk) + labels to the host runs on a high-priority decode stream under the next groups' forwards.
 * A group closes after rd_pipe_config batches (default 4), or -- global mode -- as soon as its forward rows cover the beam
 * search of its longest read (a read's search is one serial chain of a time step per sample, which only the next group's
 * forwards can hide).  rd_pipe_config / rd_pipe_set_lanes only while the pipeline is empty (after rd_pipe_flush).
 * Contracts as the blocking entry points -- rd_basecall_chunk_resident (rd_pipe_submit), rd_basecall_reads_chunk_resident
 * (rd_pipe_submit_reads), rd_basecall_reads_global / rd_basecall_raw_global / rd_basecall_raw_chunk -- except:
 *   - labels_out / label_len / status of a submitted batch are valid once rd_pipe_progress reports it delivered (or after
 *     rd_pipe_flush); the caller keeps them alive until then (chunk mode: labels of window i at labels_out + i*chunk_len).
 *     raw / read_off / label_off / valid_len may be reused when the call returns; d_signal / d_windows must stay untouched until
 *     delivery;
 *   - empty reads are rejected (RD_ERR_ARG): basecall.py:77-82 skips them before this point.
 * Batches whose read lengths equal the previous batch's on the same lane reuse its tile descriptors; otherwise the plan
 * is rebuilt on the host and uploaded behind the lane's previous forward -- no stream is drained for it. */
int rd_pipe_config(rd_ctx* ctx, int group_batches);
int rd_pipe_set_lanes(rd_ctx* ctx, int lanes); /* 1..4; only while the pipeline is empty */
int rd_pipe_submit(rd_ctx* ctx, const float* d_windows, int n_windows, int chunk_len, const int32_t* valid_len,
                   int beam_width, uint8_t* labels_out, int32_t* label_len);
int rd_pipe_submit_reads(rd_ctx* ctx, const float* d_signal, const int64_t* read_off, int n_reads, int chunk_len,
                         int step, int beam_width, uint8_t* labels_out, int32_t* label_len);
int rd_pipe_submit_reads_global(rd_ctx* ctx, const float* d_signal, const int64_t* read_off, int n_reads, int chunk_len,
                                int step, int beam_width, int use_lm, double s_thr, double r_thr, uint8_t* labels_out,
                                const int64_t* label_off, int32_t* label_len);
int rd_pipe_submit_raw_global(rd_ctx* ctx, const int16_t* raw, const int64_t* read_off, int n_reads, int outlier_clip,
                              int chunk_len, int step, int beam_width, int use_lm, double s_thr, double r_thr,
                              uint8_t* labels_out, const int64_t* label_off, int32_t* label_len, int32_t* status);
int rd_pipe_submit_raw_chunk(rd_ctx* ctx, const int16_t* raw, const int64_t* read_off, int n_reads, int outlier_clip,
                             int chunk_len, int step, int beam_width, uint8_t* labels_out, int32_t* label_len, int32_t* status);
/* Deliver finished groups of the pipeline to their callers, in submission order.  Without blocking when
 * wait_for <= 0; otherwise returns once at least wait_for of the batches submitted so far (counted since the context was
 * created) have been delivered, closing the open group if what is awaited sits in it.  *delivered = that count. */
int rd_pipe_progress(rd_ctx* ctx, int64_t wait_for, int64_t* delivered);
int rd_pipe_flush(rd_ctx* ctx);   /* launches the open group and delivers every batch submitted so far */
/* Batches submitted to the pipeline so far: right after a submit, the number rd_pipe_progress must reach for
 * that batch to have been delivered. */
int rd_pipe_submitted(rd_ctx* ctx, int64_t* submitted);

/* RNA model file -> dense table, without a JSON object tree.  radian/basecall.py:48-57 (json.load, then every "ACGT..." key re-keyed as a
 * tuple of label indices).  The reference's default model has 4^11 keys in ~420 MB of text; these two calls scan the one shape such a
 * file has -- an object of k-character keys over ACGT, each with an array of four JSON numbers -- straight into the [4^k][4] float64 table
 * rd_load_lm takes (row = base-4 number of the context, first character most significant):
 *   rd_lm_json_probe: k = length of the first key (1..13);
 *   rd_lm_json_fill:  the caller has filled table with NaN; every key's row is written (a repeated key keeps its last value, like a Python
 *                     dict), rows of contexts the file does not hold stay NaN (sparse model: see rd_load_lm); *n_entries = pairs read,
 *                     *n_contexts = distinct contexts.
 * Anything else in the text (escapes, another alphabet, a key of another length, NaN / Infinity, nested values, trailing text) returns
 * RD_ERR_FORMAT and decides nothing: the caller falls back to a full JSON parser, whose errors are the reference's.  Numbers are
 * converted correctly rounded and locale-independently (the double Python's float() gives).  No GPU is touched, no context is needed. */
int rd_lm_json_probe(const char* buf, size_t n, int* k_out);
int rd_lm_json_fill(const char* buf, size_t n, int k, double* table, int64_t* n_entries, int64_t* n_contexts);
/* The way back: table [4^k][4] -> that text, in one pass, keys in row order, every number with the shortest digits that convert back to
 * the same double -- rd_lm_json_fill and json.load (the reference) both return the table bit for bit.  Rows of NaN (absent contexts) are
 * left out.  RD_ERR_ARG: a row mixes NaN with numbers, or holds an infinity or a negative value; RD_ERR_IO: the file cannot be written. */
int rd_lm_json_write(const char* path, const double* table, int k, int64_t* n_rows, int64_t* n_bytes);

/* ---- making the RNA model.  The reference ships one model (human protein-coding mRNA) and nothing that builds one.
 * What a row means is fixed by the reference's lookup (radian/decode.py:42-49,77-96,152-158): labelings are in decode order, 3'->5'
 * (basecall.py:130 writes the FASTA line reversed), the row of a context is the distribution of the label after it.
 *
 * rd_fasta_scan: host only.  One pass over a FASTA text: `>` lines are headers; in sequence lines ACGT, U = T and their lower case are
 *   codes 0..3, any other letter, `*` and `-` are code 255 (a break: no counted window spans it), white space is skipped and any other
 *   byte is RD_ERR_FORMAT with record and line in rd_last_error().  field >= 0 keeps only the records whose header (the text after `>`),
 *   split on `|`, has `value` as field `field` (0-based).  counts = {records read, records kept, codes of the kept records}.  Call once with
 *   codes = offsets = NULL for the sizes, then with codes[counts[2]] and offsets[counts[1] + 1].
 *
 * rd_lm_build: counts every window of k + 1 labels over ACGT of every record -- in decode order, i.e. of the record reversed, unless
 *   as_written -- then the lower orders as exact marginals, and fills row c from the largest order j <= k whose row of c's last j labels
 *   has a positive sum s: p[b] = (count[b] + alpha) / (s + 4 alpha), float64, each operation rounded once.  unseen: 0 = that back-off;
 *   1 = a context without a count at order k gets 0.25 four times; 2 = it gets a row of NaN (a sparse model).  k in 1..13.  The table becomes
 *   the context's RNA model exactly as if rd_load_lm had been called with it, and is copied to table_out [4^k][4] when that is not NULL
 *   (counts_out [4^k][4], the order-k counts, likewise).  cut: bytes of input per launch (0: the default); no effect on the result.
 *   Counters are 32-bit: an input of more than 2^32 - 1 codes is refused (RD_ERR_ARG), as is one without any window to count.
 *   stats[32]: [0] windows counted, [1] contexts with a count at order k, [2] contexts whose gate opens at r_thr (entropy < r_thr,
 *   decode.py:90), [3] counted windows whose context is one of those, [4] absent rows, [5] uniform rows, [6] launches of the count,
 *   [8 + j] rows filled from order j, [24..28] microseconds of the call's stages: host staging, upload, count, marginals + table +
 *   entropies, download.
 *
 * rd_lm_score: the records' windows against the context's RNA model (built or loaded; not a hashed one).  stats[8]: [0] windows,
 *   [1] those with p(next | context) > 0, [2] with p = 0, [3] whose context the model does not hold, [4] whose context's gate opens at
 *   r_thr; *nll_sum = sum of -ln p over [1], glibc's ln, added in a fixed order. */
int rd_fasta_scan(const char* buf, size_t n, int field, const char* value, uint8_t* codes, int64_t* offsets, int64_t* counts);
int rd_lm_build(rd_ctx* ctx, const uint8_t* codes, const int64_t* offsets, int64_t n_records, int k, int as_written, int unseen, double alpha,
                double r_thr, int64_t cut, double* table_out, uint32_t* counts_out, int64_t* stats);
int rd_lm_score(rd_ctx* ctx, const uint8_t* codes, const int64_t* offsets, int64_t n_records, int as_written, double r_thr, int64_t cut,
                int64_t* stats, double* nll_sum);

/* ---- the step before the hot path, on the HOST's cores: raw signals out of fast5 files, in batches --
 * radian/basecall.py:7,70-76: `get_fast5_file(path).get_reads()`, `read.read_id`, `read.get_raw_data()` (int16 DAQ values, unscaled).
 * A handle indexes one file's reads in ont_fast5_api's order -- multi-read: the root's `read_<id>` groups by name, signal at Raw/Signal;
 * single-read: the groups of /Raw/Reads, id = the group's `read_id` attribute (else its name) -- over a read-only mapping of the file, walking
 * the CLASSIC HDF5 layout (superblock 0/1, version-1 object headers, symbol-table or compact-link groups, contiguous / compact / chunked
 * int16 datasets, chunks raw or through HDF5's built-in deflate / shuffle / Fletcher-32 filters: what libhdf5's defaults write, what
 * radian/data/reads.fast5 is, and the gzip-compressed signals of pre-VBZ MinKNOW files) with every access bounds-checked.
 *   rd_fast5_open / rd_fast5_open_mem (the caller keeps buf alive and unchanged) / rd_fast5_close
 *   rd_fast5_count       reads of the file
 *   rd_fast5_lengths     samples of reads [lo, hi): sizes the block for ...
 *   rd_fast5_read_batch  reads [lo, hi) copied back to back into samples (capacity cap), offsets[hi - lo + 1] = where each starts (the
 *                        last entry = the total); ids (nullable): the read ids, NUL-terminated, id_stride bytes apart.
 * Anything else in the file (newer superblock / object headers, fractal-heap groups, any other filter such as VBZ, a chunk that fails to
 * inflate or fails its checksum, another sample type, an address outside the file) returns RD_ERR_FORMAT and decides nothing: the caller reads the file
 * through libhdf5, whose errors are then the verdict.  ~2 us per 4096-sample read on one core (libhdf5: ~63; deflated signals 60 M samples/s against 18 M); no GPU is touched, no
 * context is needed, a handle is used by one thread at a time. */
typedef struct rd_fast5 rd_fast5;
int rd_fast5_open(const char* path, rd_fast5** out);
int rd_fast5_open_mem(const void* buf, size_t n, rd_fast5** out);
void rd_fast5_close(rd_fast5* f);
int rd_fast5_count(const rd_fast5* f, int64_t* n_reads);
int rd_fast5_lengths(rd_fast5* f, int64_t lo, int64_t hi, int64_t* n_samples);
int rd_fast5_read_batch(rd_fast5* f, int64_t lo, int64_t hi, int16_t* samples, int64_t cap, int64_t* offsets, char* ids, int id_stride);

/* ---- the step after the hot path in chunk mode, on the HOST's cores: simple_assembly + argmax --
 * radian/sequence_assembly.py:19-48, radian/basecall.py:122-123.  labels / label_len as the chunk-mode entry points return
 * them (window w at labels + w * chunk_len); read r owns windows [read_win_off[r], read_win_off[r + 1]).  The consensus of
 * read r (labels 0..3, not reversed) goes to seq_out + seq_off[r] (capacity >= the sum of its windows' label_len),
 * seq_len[r] its length -- or -1 where the reference raises IndexError (its vote matrix grows at most once per fragment).
 * Fragment placement restates difflib.SequenceMatcher (autojunk included) exactly; n_threads host threads share the
 * reads.  No GPU is touched and no context is needed. */
int rd_stitch_chunk(const uint8_t* labels, const int32_t* label_len, int chunk_len, const int32_t* read_win_off, int n_reads,
                    uint8_t* seq_out, const int64_t* seq_off, int32_t* seq_len, int n_threads);

/* ---- read-accuracy evaluation: radian/align.py ------------------------------------------------------------------------ */
/* pairwise2.align.globalms(ref, seq, match, mismatch, gap_open, gap_extend) + analyse_alignment (radian/align.py:9-57,87-92;
 * the reference passes 2, -4, -4, -2) for a batch of pairs, on the GPU (align.hip).
 *   refs / reads   concatenated bytes; pair p is refs[ref_off[p] .. ref_off[p+1]) against reads[read_off[p] .. read_off[p+1])
 *                  (offsets have n_pairs + 1 entries and start at 0).  Characters are compared as bytes (no U -> T here).
 *   Affine-gap global alignment (Gotoh), int32 scores: a gap of length L costs gap_open + (L-1) * gap_extend, end gaps are
 *   penalised.  Every |score| < 2^16, and gap_open <= gap_extend (equal: linear gaps), else RD_ERR_ARG before anything is staged
 *   or launched: with open > extend the recurrence reopens adjacent gaps, so the score is not the stated gap cost.  A pair with
 *   max|score| * (n + m + 1) >= 2^28 is RD_ERR_ARG too (int32 scores).  Of the co-optimal alignments the traceback takes
 *   the one of a FIXED tie-break (the reference draws one at random, align.py:89): diagonal before deletion (ref base
 *   against a read gap) before insertion, and inside a gap run extending before closing.
 *   score[p]       the optimal score
 *   counts[4p..]   n_match, n_sub, n_ins, n_del after analyse_alignment's soft clip (its return order)
 *   status[p]      RD_ALIGN_OK, RD_ALIGN_CLIP_INDEX_ERROR (analyse_alignment raises IndexError), RD_ALIGN_EMPTY_AFTER_CLIP
 *                  (clip_start > clip_end: all counts 0), RD_ALIGN_TOO_LARGE (not aligned, see below)
 *   ops_out / ops_off / ops_len (all NULL, or all given): pair p's alignment columns go to ops_out + ops_off[p] (capacity
 *                  n + m), ops_len[p] of them, 'M' match, 'X' mismatch, 'D' deletion, 'I' insertion.
 *   budget_bytes   device workspace one batch of pairs may take (rd_align_workspace_bytes each); 0 = a quarter of the free
 *                  device memory.  Pairs are sorted by cells and packed into batches under it.  A pair that alone exceeds it is
 *                  not aligned: status RD_ALIGN_TOO_LARGE, and the call returns RD_ERR_NOMEM naming it after aligning the others
 *                  (the check is made before any launch).
 * Synchronous; uses the context's stream. */
#define RD_ALIGN_OK 0
#define RD_ALIGN_CLIP_INDEX_ERROR 1
#define RD_ALIGN_EMPTY_AFTER_CLIP 2
#define RD_ALIGN_TOO_LARGE 3
int rd_align_batch(rd_ctx* ctx, const uint8_t* refs, const int64_t* ref_off, const uint8_t* reads, const int64_t* read_off, int n_pairs,
                   int match, int mismatch, int gap_open, int gap_extend, int64_t budget_bytes, int32_t* score, int32_t* counts,
                   int32_t* status, uint8_t* ops_out, const int64_t* ops_off, int32_t* ops_len);
/* Workspace bytes rd_align_batch needs for one pair of lengths n x m alone (about n * m / 2: four direction bits per cell). */
int64_t rd_align_workspace_bytes(int64_t n, int64_t m);
/* Host, no GPU: the soft clip and counts rd_align_batch applies to an alignment -- the same code the device runs.  ops: n_ops
 * columns of M / X / D / I; ref / read: the characters the D / I columns consume (their order in the alignment). */
int rd_align_clip_count(const uint8_t* ops, int64_t n_ops, const uint8_t* ref, const uint8_t* read, int32_t* counts, int32_t* status);

/* ---- forced CTC alignment: per-base qualities and signal positions (ctcalign.hip) -------------------------
 * NO reference behaviour: the reference writes bare FASTA.  The Viterbi alignment of a GIVEN label sequence (labels 0..3 as the
 * decode returns them; blank is class 4) against the [T,5] probability rows of a sequence; rows and sequences as rd_decode_batch
 * (seq_off / seq_len in rows, n_seq sequences, float32 or float64 rows), labels of sequence i at labels + label_off[i],
 * label_len[i] of them.  Per sequence with T rows and L labels c_0 .. c_{L-1}, met EXACTLY (bit for bit), not to a tolerance:
 *   states    s = 0 .. 2L; even states are blank, odd state 2i+1 is label i
 *   lp[t][c]  = log((double)P[t][c]) as glibc's log evaluates it (csrc/glibc_math.h, whatever rd_set_decode_math says); log 0 = -inf
 *   start     V[0][0] = lp[0][4], V[0][1] = lp[0][c_0], every other state -inf
 *   step      V[t][s] = lp[t][cls(s)] + max(V[t-1][s], V[t-1][s-1], V[t-1][s-2]); the third term only for odd s >= 3 with
 *             c_i != c_{i-1}.  fp64, one max and one add per cell.  Tie-break: a predecessor replaces the best so far only if
 *             it is STRICTLY greater, tried in the order s, s-1, s-2
 *   end       state 2L, or 2L-1 if V[T-1][2L-1] is strictly greater; score[i] = that value
 *   status[i] RD_CTCALIGN_OK; RD_CTCALIGN_NO_PATH when the score is -inf (L > T, repeats without room for the blank between them,
 *             zero-probability rows): the per-base outputs are then -1, -1, 0; RD_CTCALIGN_TOO_LARGE (see budget_bytes; same outputs)
 *   L = 0 is valid (the score of the all-blank path); T = 0 is RD_ERR_ARG
 *   first_step / last_step [label_off[i] + k]   the first and the last row the traced path spends in state 2k+1 (every row between
 *             them is in that state)
 *   qual [label_off[i] + k]   p = max over those rows of (double)P[t][c_k], e = 1 - p; the number of q in 1..50 with
 *             e <= 10^(-q/10), i.e. min(50, floor(-10 log10 e)) by comparison with a table of 50 doubles (e = 0 gives 50).
 *             This is the model's own confidence in the base where it was emitted -- NOT calibrated against observed error rates
 *   budget_bytes   device workspace one launch may take (rd_ctc_align_workspace_bytes per sequence; the 2-bit back-pointers are
 *             nearly all of it); 0 = a quarter of the free device memory.  Sequences are packed into launches under it in the
 *             caller's order.  A sequence that alone exceeds it is not aligned: status RD_CTCALIGN_TOO_LARGE, and the call returns
 *             RD_ERR_NOMEM naming it after aligning the others.  Results do not depend on the launches.
 * Synchronous; uses the context's stream. */
#define RD_CTCALIGN_OK 0
#define RD_CTCALIGN_NO_PATH 1
#define RD_CTCALIGN_TOO_LARGE 2
int rd_ctc_align_batch(rd_ctx* ctx, const void* probs, int prob_is_f64, const int64_t* seq_off, const int32_t* seq_len, int n_seq,
                       const uint8_t* labels, const int64_t* label_off, const int32_t* label_len, int64_t budget_bytes,
                       int32_t* first_step, int32_t* last_step, uint8_t* qual, double* score, int32_t* status);
/* Workspace bytes of one sequence of n_rows rows and n_labels labels, each term rounded up to 256:
 *   64 n_rows (log rows) + 4 n_rows ceil((2 n_labels + 1) / 16) (back-pointers) + 16 n_rows (band columns) */
int64_t rd_ctc_align_workspace_bytes(int64_t n_rows, int64_t n_labels);
/* rd_basecall_raw_global plus the forced alignment of every read's labels against the very rows its beam search read (the
 * assembled float64 rows, or the forward's float32 / f16 rows of a single-coverage read), while they are on the device.  Labels,
 * label_len and status exactly as rd_basecall_raw_global.  qual_out / first_step_out / last_step_out are indexed as labels_out
 * (label_off); one row is one raw sample, so the steps are sample indices into the read.  score_out / align_status per read
 * (a read that came back RD_LEN_MISSING_CONTEXT: RD_CTCALIGN_NO_PATH).  budget_bytes and RD_ERR_NOMEM as rd_ctc_align_batch:
 * every read is basecalled and every read under the budget aligned before the call returns it. */
int rd_basecall_raw_global_q(rd_ctx* ctx, const int16_t* raw, const int64_t* read_off, int n_reads, int outlier_clip, int chunk_len,
                             int step, int beam_width, int use_lm, double s_thr, double r_thr, uint8_t* labels_out,
                             const int64_t* label_off, int32_t* label_len, int32_t* status, int64_t budget_bytes, uint8_t* qual_out,
                             int32_t* first_step_out, int32_t* last_step_out, double* score_out, int32_t* align_status);

/* ---- signal-to-reference alignment: the per-base event table (events.hip) -------------------------------
 * NO reference behaviour.  Given a forced alignment (rd_ctc_align_batch, or the fused route below) of label_len[r] labels against
 * read r -- samples raw + read_off[r] .. read_off[r+1], steps at first_step / last_step + label_off[r], one row = one raw sample --
 * the samples every label sits on and what the current was there.  Integer arithmetic only; met exactly.  Per read with T samples,
 * L >= 1 labels and align_status[r] == RD_CTCALIGN_OK:
 *   event k   covers samples [start_k, end_k): start_k = first_step[k]; end_k = first_step[k+1] for k < L-1 and last_step[L-1] + 1
 *             for the last one (a base owns the blank rows after it, as a moves table does).  Events are non-empty and back to back;
 *             the samples before first_step[0] and after last_step[L-1] belong to no event
 *   ev_start / ev_end [label_off[r] + k]   start_k, end_k
 *   ev_sum / ev_sumsq   the sum and the sum of squares of the raw int16 samples of the event (int64: 2^30 * 2^31 < 2^63)
 *   ev_min / ev_max     their minimum and maximum
 * A read whose align_status is not OK gets start = end = -1 and 0 everywhere else for each of its labels; its neighbours are
 * unaffected.  RD_ERR_ARG before anything is launched: a null pointer, offsets that are not monotone (read_off non-decreasing;
 * label_off[r+1] >= label_off[r] + label_len[r]), and for an OK read any step outside 0 <= first_step[k] <= last_step[k] < T or
 * last_step[k] >= first_step[k+1].  A result does not depend on what else is in the call or on the order of the reads.
 *   rd_event_stats        on the GPU; synchronous, uses the context's stream
 *   rd_event_stats_host   host, no GPU: the same boundary code and a plain loop */
int rd_event_stats(rd_ctx* ctx, const int16_t* raw, const int64_t* read_off, int n_reads, const int32_t* first_step,
                   const int32_t* last_step, const int64_t* label_off, const int32_t* label_len, const int32_t* align_status,
                   int32_t* ev_start, int32_t* ev_end, int64_t* ev_sum, int64_t* ev_sumsq, int16_t* ev_min, int16_t* ev_max);
int rd_event_stats_host(const int16_t* raw, const int64_t* read_off, int n_reads, const int32_t* first_step, const int32_t* last_step,
                        const int64_t* label_off, const int32_t* label_len, const int32_t* align_status, int32_t* ev_start,
                        int32_t* ev_end, int64_t* ev_sum, int64_t* ev_sumsq, int16_t* ev_min, int16_t* ev_max);
/* "Resquiggle": the sibling of rd_basecall_raw_global_q that aligns GIVEN labels -- a reference span in decode order, codes 0..3,
 * ref_len[r] of them at ref_labels + ref_off[r] (0 is valid, a code above 3 is RD_ERR_ARG) -- instead of the read's own call.
 * Normalisation, forward and assembly as rd_basecall_raw_global (the rows are the ones its beam search would read: the assembled
 * float64 rows, or a single-coverage read's float32 / f16 rows); NO beam search; then rd_ctc_align_batch's alignment of the labels
 * against those rows and rd_event_stats on the raw samples, while both are on the device.  Per-base outputs are indexed by ref_off,
 * score / align_status / read_status per read.  read_status as rd_basecall_raw_global (an empty read is RD_ERR_ARG); a read that
 * normalisation refuses (read_status 1) is not aligned: RD_CTCALIGN_NO_PATH, score -inf, "no path" outputs.  budget_bytes,
 * RD_CTCALIGN_TOO_LARGE and RD_ERR_NOMEM as rd_ctc_align_batch. */
int rd_resquiggle_raw(rd_ctx* ctx, const int16_t* raw, const int64_t* read_off, int n_reads, int outlier_clip, int chunk_len, int step,
                      const uint8_t* ref_labels, const int64_t* ref_off, const int32_t* ref_len, int64_t budget_bytes,
                      int32_t* first_step, int32_t* last_step, uint8_t* qual, double* score, int32_t* align_status, int32_t* read_status,
                      int32_t* ev_start, int32_t* ev_end, int64_t* ev_sum, int64_t* ev_sumsq, int16_t* ev_min, int16_t* ev_max);

/* ---- poly(A) tail estimation: the longest flat stretch of a read's raw samples (polya.hip) ----------------
 * NO reference behaviour.  A homopolymer of 30..250 A collapses in any CTC decode, so the tail is measured on the raw samples: the
 * longest run of windows whose spread is small against the read's own MAD.  Integer arithmetic only; met exactly.  Read r is samples
 * raw + read_off[r] .. read_off[r+1] (T of them).  Parameters (anything outside its range is RD_ERR_ARG):
 *   win 8..256 (window length); flat_q 1..32767 (spread threshold); use_level 0/1; -2^20 <= lo_q <= hi_q <= 2^20 (level band);
 *   max_gap 0..1024 (non-flat windows tolerated inside a segment); min_samples >= win; search_limit >= 0 (0: the whole read).
 *   The _q values are in units of MAD / 256: a threshold of z in mad_normalise's units is q = round(z * 1.4826 * 256).
 * Per read:
 *   scale     m2 = the sum of the two middle order statistics of the samples (ranks (T-1)/2 and T/2: twice the median); d4 = the sum
 *             of the two middle order statistics of |2x - m2| (four times the MAD) -- the order statistics of rd_normalise_reads.
 *             status, in this order: T == 0 RD_POLYA_EMPTY; d4 == 0 RD_POLYA_MAD_ZERO; T < win RD_POLYA_SHORT
 *   windows   nw = T / win; window j covers samples [j win, (j+1) win); the last T mod win samples belong to no window.
 *             S_j = sum x, Q_j = sum x^2, V_j = win Q_j - S_j^2 (>= 0: win^2 times the variance)
 *   flat      A = win flat_q d4 (below 2^41), thr = floor(A^2 / 2^20) saturated to 2^64 - 1.  Window j is flat iff V_j <= thr -- that is
 *             sd <= (flat_q / 256) MAD with no rounding anywhere -- and, with use_level, lo_q d4 win <= 512 (2 S_j - win m2) <= hi_q d4 win
 *   segments  two flat windows i < j with no flat window between them belong to the same segment iff j - i <= max_gap + 1.  A segment
 *             [a, b] (its first and last flat window) is a CANDIDATE iff (b - a + 1) win >= min_samples and (search_limit == 0 or
 *             a win < search_limit)
 *   choice    the candidate with the largest b - a + 1; on a tie the smallest a.  No candidate: RD_POLYA_NONE
 *   outputs   status; tail_start = a win, tail_end = (b + 1) win; n_flat = the flat windows inside the chosen segment; sum / sumsq over
 *             all samples of [tail_start, tail_end) (gap windows included); m2, d4; n_candidates.  For any status other than OK the two
 *             ends are -1 and everything else is 0, except m2 and d4, which are reported whenever T > 0 (not for RD_POLYA_TOO_LARGE)
 * A read never affects its neighbours; a result does not depend on what else is in the call, on the order of the reads or on the
 * launches.  RD_ERR_ARG before anything is launched: a null pointer, read offsets that are not monotone, a parameter outside its range.
 * n_reads == 0 is RD_OK.
 *   rd_polya_segment        on the GPU; synchronous, uses the context's stream.  budget_bytes: device workspace one launch may take
 *                           (rd_polya_workspace_bytes per read); 0 = a quarter of the free device memory.  Reads are packed into
 *                           launches under it in the caller's order; a read that alone exceeds it is not looked at: status
 *                           RD_POLYA_TOO_LARGE, and the call returns RD_ERR_NOMEM naming it after doing the others
 *   rd_polya_segment_host   host, no GPU: the same rules (csrc/polya_rules.h) in a plain loop, counting over the keys for the order statistics
 *   rd_polya_workspace_bytes   2 n_samples + 14 (n_samples / win) + 2048: the samples, 13 B per window (flag, S, Q) and the descriptors
 *   rd_polya_diag_windows   the first two stages alone, through their own kernels, for stage tests (it changes no result and has no
 *                           budget): per read m2, d4 and thr; per window S_j, Q_j and the flag, the reads' windows back to back
 *                           (read r's window 0 at the sum of T / win over the reads before it).  Computed whatever the read's status */
#define RD_POLYA_OK 0
#define RD_POLYA_NONE 1
#define RD_POLYA_MAD_ZERO 2
#define RD_POLYA_SHORT 3
#define RD_POLYA_EMPTY 4
#define RD_POLYA_TOO_LARGE 5
int rd_polya_segment(rd_ctx* ctx, const int16_t* raw, const int64_t* read_off, int n_reads, int win, int flat_q, int use_level, int lo_q,
                     int hi_q, int max_gap, int64_t min_samples, int64_t search_limit, int64_t budget_bytes, int32_t* status,
                     int64_t* tail_start, int64_t* tail_end, int32_t* n_flat, int64_t* sum, int64_t* sumsq, int32_t* m2, int32_t* d4,
                     int32_t* n_candidates);
int rd_polya_segment_host(const int16_t* raw, const int64_t* read_off, int n_reads, int win, int flat_q, int use_level, int lo_q, int hi_q,
                          int max_gap, int64_t min_samples, int64_t search_limit, int32_t* status, int64_t* tail_start, int64_t* tail_end,
                          int32_t* n_flat, int64_t* sum, int64_t* sumsq, int32_t* m2, int32_t* d4, int32_t* n_candidates);
int64_t rd_polya_workspace_bytes(int64_t n_samples, int win);
int rd_polya_diag_windows(rd_ctx* ctx, const int16_t* raw, const int64_t* read_off, int n_reads, int win, int flat_q, int use_level, int lo_q,
                          int hi_q, int32_t* m2, int32_t* d4, uint64_t* thr, int32_t* win_sum, int64_t* win_sumsq, uint8_t* win_flat);

/* ---- two-sample site comparison of event tables (sitecmp.hip) --------------------------------------------
 * NO reference behaviour.  The events of two samples (cond 0: e.g. native, cond 1: e.g. in-vitro transcribed) are put side by side
 * transcript position by transcript position, one channel (level or dwell) per call.  Integer arithmetic only; met exactly.
 * Event i: site[i] (< n_sites), cond[i] (0 or 1), value[i] (int16).  One output entry per DISTINCT site with at least one event, in
 * ascending site order (*n_out of them, at most `capacity`: the entries the output arrays hold; n, sum, sumsq, vmin, vmax and med2 hold
 * two values per entry, [entry][cond]).  With a / b the sorted values of sample 0 / 1 of the site and n0, n1 their counts:
 *   out_site  the site
 *   n         n0, n1
 *   sum, sumsq   over the values of each sample
 *   vmin, vmax   of each sample
 *   med2      the sum of the two middle order statistics of each sample (ranks (n-1)/2 and n/2): twice the median
 *   u2        sum over x in a of ( 2 #{y in b : y < x} + #{y in b : y = x} ): twice the Mann-Whitney U of sample 0
 *   ks_num    max over the values x present in either sample of | #{a <= x} n1 - #{b <= x} n0 |: n0 n1 times the Kolmogorov-Smirnov D
 *   ks_x      the SMALLEST x that attains that maximum
 *   tie       sum over the values x of t^3 - t, t the multiplicity of x in both samples together
 *   status    RD_SITE_ONE_SIDED  n0 == 0 or n1 == 0; otherwise
 *             RD_SITE_DEEP       n0 + n1 > 2^20 (moments, vmin, vmax and med2 are still filled); otherwise RD_SITE_OK
 *             RD_SITE_TOO_LARGE  the site alone exceeds the budget: only out_site and n are filled
 * Fields of an absent sample are 0; the rank fields u2, ks_num, ks_x and tie are 0 unless the status is RD_SITE_OK.
 * Bounds: with |value| <= 2^15 and n0 + n1 <= 2^20 (the rank fields), sumsq < 2^61 (for any n below 2^31), tie <= 2^60, u2 <= 2^39,
 * ks_num <= 2^38; ks_num << 16 | (65535 - (ks_x + 32768)), the word the kernels take the maximum of, is below 2^55.  No field overflows.
 * A site never affects another; a result does not depend on the order of the events, on what else is in the call or on the launches.
 * RD_ERR_ARG before anything is launched: a null pointer, n_events > 2^31 - 1, a site >= n_sites, a cond > 1, a capacity below the
 * number of distinct sites.  n_events == 0 is RD_OK with *n_out = 0.
 *   rd_site_compare         on the GPU; synchronous, uses the context's stream.  budget_bytes: device workspace one launch may take
 *                           (rd_site_workspace_bytes of a site's events); 0 = a quarter of the free device memory.  Sites are packed
 *                           into launches under it in ascending order; a site that alone exceeds it is not looked at: status
 *                           RD_SITE_TOO_LARGE, and the call returns RD_ERR_NOMEM naming it after doing the others
 *   rd_site_compare_host    host, no GPU: the same rules (csrc/site_rules.h) over std::sort and plain loops
 *   rd_site_workspace_bytes   160 n_events: 31 B per event (its three inputs, two key buffers, head flag and scan) and up to 124 B per
 *                           site (a site has at least one event); the remainder stands for the sort's temporary storage, which is
 *                           sized by the sort's own query
 *   rd_site_diag_segments   the pack, sort and segment stages alone, through the same kernels, for stage tests (it changes no result
 *                           and has no budget): the sorted keys site << 17 | cond << 16 | (value + 32768) [n_events] and per segment
 *                           (site, start, split, end) as int64 [capacity][4]: the site's keys are [start, end) of the sorted keys,
 *                           sample 1 begins at split */
#define RD_SITE_OK 0
#define RD_SITE_ONE_SIDED 1
#define RD_SITE_DEEP 2
#define RD_SITE_TOO_LARGE 3
int rd_site_compare(rd_ctx* ctx, const uint32_t* site, const uint8_t* cond, const int16_t* value, int64_t n_events, uint32_t n_sites,
                    int64_t budget_bytes, int64_t capacity, uint32_t* out_site, int32_t* status, int64_t* n, int64_t* sum, int64_t* sumsq,
                    int32_t* vmin, int32_t* vmax, int32_t* med2, int64_t* u2, int64_t* ks_num, int32_t* ks_x, int64_t* tie, int64_t* n_out);
int rd_site_compare_host(const uint32_t* site, const uint8_t* cond, const int16_t* value, int64_t n_events, uint32_t n_sites, int64_t capacity,
                         uint32_t* out_site, int32_t* status, int64_t* n, int64_t* sum, int64_t* sumsq, int32_t* vmin, int32_t* vmax,
                         int32_t* med2, int64_t* u2, int64_t* ks_num, int32_t* ks_x, int64_t* tie, int64_t* n_out);
int64_t rd_site_workspace_bytes(int64_t n_events);
int rd_site_diag_segments(rd_ctx* ctx, const uint32_t* site, const uint8_t* cond, const int16_t* value, int64_t n_events, uint32_t n_sites,
                          int64_t capacity, uint64_t* sorted_keys, int64_t* segments, int64_t* n_segments);

/* ---- exact two-cluster split of a site's pooled values (sitecmp.hip, csrc/site_rules.h) ----------------------
 * NO reference behaviour.  The hard-assignment limit of a two-component mixture in one dimension: the threshold on the pooled values of a
 * site that splits them into the two clusters of least within-cluster variance.  Integer arithmetic only; met exactly.  Inputs, output
 * order and capacity as rd_site_compare; one channel per call; n, sum, sumsq, n_lo, sum_lo and sumsq_lo hold two values per entry,
 * [entry][cond].  With a / b the values of sample 0 / 1 of the site, n0, n1 their counts and N = n0 + n1:
 *   a CUT c is a value present in either sample other than the pooled maximum; its low cluster is the events with value <= c (pooled
 *   count n_lo, sum S_lo), its high cluster the rest (n_hi, S_hi).  It is ADMISSIBLE iff n_lo >= 1, n_hi >= 1, 65536 n_lo >= min_frac_q16 N
 *   and 65536 n_hi >= min_frac_q16 N (min_frac_q16 in 0 .. 32768: the least share of either cluster, in 1/65536).
 *   D(c) = S_lo n_hi - S_hi n_lo;  J(c) = D^2 / (n_lo n_hi).  The cut chosen is the admissible cut of the largest J, the SMALLEST c among
 *   equals; J1 against J2 is D1^2 (n_lo2 n_hi2) against D2^2 (n_lo1 n_hi1), compared exactly.
 *   out_site, n, sum, sumsq   as rd_site_compare's
 *   cut       the cut chosen (int32);  n_cuts  the number of admissible cuts (int32)
 *   n_lo, sum_lo, sumsq_lo    per sample, over its values <= cut (the high cluster follows by subtraction)
 *   status    RD_SITE_ONE_SIDED  n0 == 0 or n1 == 0; otherwise
 *             RD_SITE_DEEP       N > 2^16 (totals only); otherwise
 *             RD_SITE_NONE       no admissible cut: every value equal, or min_frac_q16 cannot be met; otherwise RD_SITE_OK
 *             RD_SITE_TOO_LARGE  the site alone exceeds the budget: only out_site and n are filled
 * cut, n_cuts, n_lo, sum_lo and sumsq_lo are 0 unless the status is RD_SITE_OK.
 * Bounds: with |value| <= 2^15 and N <= 2^16, |D| <= 2^16 n_lo n_hi <= 2^46, D^2 <= 2^92 and n_lo n_hi <= 2^30: a cross product is
 * below 2^122, one unsigned 128-bit product.  No field overflows.
 * A site never affects another; a result does not depend on the order of the events, on what else is in the call, on the budget or on
 * the launches.  RD_ERR_ARG before anything is launched: the cases of rd_site_compare, and min_frac_q16 outside 0 .. 32768.
 * n_events == 0 is RD_OK with *n_out = 0.
 *   rd_site_split           on the GPU; synchronous, uses the context's stream.  budget_bytes as rd_site_compare's, in units of
 *                           rd_site_split_workspace_bytes; a site that alone exceeds it: RD_SITE_TOO_LARGE, RD_ERR_NOMEM naming it
 *                           after doing the others
 *   rd_site_split_host      host, no GPU: the same rules over std::sort and plain loops
 *   rd_site_split_workspace_bytes   rd_site_workspace_bytes(n_events) + 16 n_events + 112 ceil(n_events / 256): the two int64 prefix
 *                           arrays (values and squares) per event; per work item (a chunk of 256 sorted elements of a site) its
 *                           16 B slot and 96 B that stand for the site's entry (a site has at least one work item) */
#define RD_SITE_NONE 4
int rd_site_split(rd_ctx* ctx, const uint32_t* site, const uint8_t* cond, const int16_t* value, int64_t n_events, uint32_t n_sites,
                  int64_t budget_bytes, int64_t capacity, int min_frac_q16, uint32_t* out_site, int32_t* status, int64_t* n, int64_t* sum,
                  int64_t* sumsq, int32_t* cut, int32_t* n_cuts, int64_t* n_lo, int64_t* sum_lo, int64_t* sumsq_lo, int64_t* n_out);
int rd_site_split_host(const uint32_t* site, const uint8_t* cond, const int16_t* value, int64_t n_events, uint32_t n_sites, int64_t capacity,
                       int min_frac_q16, uint32_t* out_site, int32_t* status, int64_t* n, int64_t* sum, int64_t* sumsq, int32_t* cut,
                       int32_t* n_cuts, int64_t* n_lo, int64_t* sum_lo, int64_t* sumsq_lo, int64_t* n_out);
int64_t rd_site_split_workspace_bytes(int64_t n_events);

/* ---- signal simulation: raw samples of reads whose sequence, base boundaries and noise are known (sim.hip) ----
 * NO reference behaviour.  Sequences plus a pore-model table become raw int16 samples with every base's first sample known.  Integer
 * arithmetic only; met exactly.
 *   read      read r has bases codes[seq_off[r] .. seq_off[r+1]), each 0..3, in the order the pore sees them (3'->5': the decode order);
 *             L = 0 is allowed.  Per read: lead[r] >= 0 samples before the first base, drawn at lead_level_q10[r] (|.| <= 2^15) with
 *             lead_sd_q10[r] (0..2^15); median[r] in DAQ units (an int16 value); scale_q10[r] = DAQ units per z unit times 1024
 *             (1..2^26); a 64-bit key, key[2r] and key[2r+1]
 *   model     k odd, 1 <= k <= 9; level_q10 (int32, |.| <= 2^15), sd_q10 (0..2^15) and dwell_q8 (256..2^23) of 4^k entries each, indexed
 *             by the k-mer in pore order, first base most significant; dwell_cdf uint32[1024], non-decreasing, each <= 2^20: quantiles
 *             of the dwell in Q16 multiples of its mean.  Levels and sds are Q10 in mad_normalise's z units, dwells Q8 samples
 *   k-mer     base b's k-mer is centred on b, h = k / 2 bases to either side; a position outside the read takes the read's nearest end base
 *   per base  optional, indexed like codes, either may be null: level_shift_q10 (int16), dwell_scale_q8 (uint16, 1..4096; 256 is 1.0)
 *   random    Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85), counter (i, stream, 0, 0),
 *             key key[r]; output words w0..w3
 *   dwell     base b: stream 0, i = b.  m = dwell_q8[kmer] * scale_q8 >> 8; t = dwell_cdf[w0 >> 22];
 *             d = clamp((m t + 2^23) >> 24, 1, 32767), the product in 64 bits
 *   positions base_first[b] = lead + the sum of d over the bases before b; n_samples = lead + the sum of every d
 *   sample    s: stream 1, i = s.  Z = the sum of the twelve 10-bit fields (bits 0-9, 10-19, 20-29 of each word), z = Z - 6138 (mean 0,
 *             sd sqrt(2^20 - 1): z is in 1/1024 sigma, |z| <= 6138).  The base of s is the b with base_first[b] <= s < base_first[b+1];
 *             s < lead is the lead.  v = level + shift + floor(sd z / 1024);
 *             raw = clamp(median + floor((v scale_q10 + 2^19) / 2^20), -32768, 32767)
 * A read's output depends on its own inputs and key only: not on the batch, the order, the budget or the launches.  RD_ERR_ARG before
 * anything is launched or written: a null pointer, offsets that are not monotone, a code above 3, a parameter or a table entry outside
 * its range, a cdf that decreases.  n_reads == 0 is RD_OK.
 *   rd_sim_lengths          n_samples[r] (int64) on the GPU; synchronous, uses the context's stream.  budget_bytes as below (a read over
 *                           it: n_samples -1 and RD_ERR_NOMEM)
 *   rd_sim_signal           the same inputs and the caller's raw_off[n_reads + 1]: read r's samples go to raw[raw_off[r] .. raw_off[r+1]).
 *                           A difference of raw_off that is not the read's n_samples, or above 2^31 - 1, is RD_ERR_ARG before anything
 *                           is written.  Outputs: raw; base_first (int32, indexed like codes; may be null); status per read: RD_SIM_OK,
 *                           RD_SIM_EMPTY (no samples), RD_SIM_TOO_LARGE.  budget_bytes: device workspace one launch may take, DESIGN.md
 *                           section 19: the sum of rd_sim_workspace_bytes over its reads plus 12 * 4^k + 4096 (rounded up to 256) + 12288
 *                           for the model and the launch; 0 = a quarter of the free device memory.  Reads are packed into launches under
 *                           it in the caller's order; a read that alone exceeds it is not looked at (its raw_off neither): status
 *                           RD_SIM_TOO_LARGE, and the call returns RD_ERR_NOMEM naming it after doing the others
 *   rd_sim_lengths_host, rd_sim_signal_host   host, no GPU: the same rules (csrc/sim_rules.h) in a plain loop
 *   rd_sim_workspace_bytes  32 n_bases + 2 n_samples + 128 */
#define RD_SIM_OK 0
#define RD_SIM_EMPTY 1
#define RD_SIM_TOO_LARGE 2
int rd_sim_lengths(rd_ctx* ctx, const uint8_t* codes, const int64_t* seq_off, int n_reads, const int16_t* level_shift_q10,
                   const uint16_t* dwell_scale_q8, const int32_t* lead, const int32_t* lead_level_q10, const int32_t* lead_sd_q10,
                   const int32_t* median, const int32_t* scale_q10, const uint32_t* key, int k, const int32_t* level_q10, const int32_t* sd_q10,
                   const int32_t* dwell_q8, const uint32_t* dwell_cdf, int64_t budget_bytes, int64_t* n_samples);
int rd_sim_lengths_host(const uint8_t* codes, const int64_t* seq_off, int n_reads, const int16_t* level_shift_q10, const uint16_t* dwell_scale_q8,
                        const int32_t* lead, const int32_t* lead_level_q10, const int32_t* lead_sd_q10, const int32_t* median,
                        const int32_t* scale_q10, const uint32_t* key, int k, const int32_t* level_q10, const int32_t* sd_q10,
                        const int32_t* dwell_q8, const uint32_t* dwell_cdf, int64_t* n_samples);
int rd_sim_signal(rd_ctx* ctx, const uint8_t* codes, const int64_t* seq_off, int n_reads, const int16_t* level_shift_q10,
                  const uint16_t* dwell_scale_q8, const int32_t* lead, const int32_t* lead_level_q10, const int32_t* lead_sd_q10,
                  const int32_t* median, const int32_t* scale_q10, const uint32_t* key, int k, const int32_t* level_q10, const int32_t* sd_q10,
                  const int32_t* dwell_q8, const uint32_t* dwell_cdf, const int64_t* raw_off, int64_t budget_bytes, int16_t* raw,
                  int32_t* base_first, int32_t* status);
int rd_sim_signal_host(const uint8_t* codes, const int64_t* seq_off, int n_reads, const int16_t* level_shift_q10, const uint16_t* dwell_scale_q8,
                       const int32_t* lead, const int32_t* lead_level_q10, const int32_t* lead_sd_q10, const int32_t* median,
                       const int32_t* scale_q10, const uint32_t* key, int k, const int32_t* level_q10, const int32_t* sd_q10,
                       const int32_t* dwell_q8, const uint32_t* dwell_cdf, const int64_t* raw_off, int16_t* raw, int32_t* base_first,
                       int32_t* status);
int64_t rd_sim_workspace_bytes(int64_t n_bases, int64_t n_samples);

/* ---- eventalign: raw samples against a k-mer pore model, Viterbi (eventalign.hip) -------------------------
 * NO reference behaviour.  The inverse of rd_sim_signal: given samples, a sequence and a pore-model table, which samples belong to which
 * base.  No neural network takes part.  Integer arithmetic only; met exactly.
 *   read      read r is samples raw + read_off[r] .. read_off[r+1] (n of them); only the window [t_lo[r], t_hi[r]) takes part,
 *             0 <= t_lo <= t_hi <= n, T = t_hi - t_lo rows.  L = ref_len[r] bases codes[ref_off[r] ..], each 0..3, in the order the pore
 *             sees them (3'->5': the decode order); L = 0 is valid.  Per-base outputs are indexed by ref_off[r] + b (ref_off[r+1] >=
 *             ref_off[r] + ref_len[r])
 *   scale     d4_in[r] > 0: (m2_in[r], d4_in[r]) as given (|m2_in| <= 2^17, d4_in <= 2^20).  d4_in[r] == 0: the window's own, as
 *             rd_polya_segment: m2 = the sum of the two middle order statistics of the window's samples, d4 = the sum of the two middle
 *             order statistics of |2x - m2|
 *   model     k odd, 1 <= k <= 9; per k-mer (4^k entries, pore order, first base most significant) lvl (int32, |.| < 2^14: the level in
 *             MAD/256), w (uint32: the inverse variance in Q32) and bias (int32, |.| <= 256: the log-sd term in 1/32 nat); the same three
 *             numbers for the background, lvl_bg, w_bg, bias_bg.  Base b's k-mer by rd_sim_signal's rule: centred on b, a position outside
 *             the span takes the nearest end base
 *   sample    u = 512 (2x - m2); zq = clamp(floor((2u + d4) / (2 d4)), -2^14, 2^14), the division in 64 bits: the sample in MAD/256,
 *             rounded half up
 *   states    s = 0 .. L + 1: 0 is the lead and L + 1 the trail (both the background), s in 1 .. L is base s - 1
 *   cell      d = zq[t] - lvl(s) (d^2 < 2^30); c(t, s) = min(floor(d^2 w(s) / 2^32), 1024) + bias(s)
 *   path      int32.  V[0][0] = c(0, 0), V[0][1] = c(0, 1); a cell with s > t + 1 is unreachable (2^30);
 *             V[t][s] = c(t, s) + min(V[t-1][s], V[t-1][s-1]), the advance from s - 1 taken only if STRICTLY smaller.  Every cell with
 *             s <= t + 1 is reachable, so 2^30 is never added to a result.  With T <= 2^19 every finite value stays below 2^19 * 1280 <
 *             2^30 and an unreachable cell computed unmasked from 2^30 stays above 2^30 - 2^19 * 256: it never wins.  There are no skips
 *             and no dwell prior.  The path ends in state L + 1 at row T - 1, or in L if V[T-1][L+1] is not strictly smaller
 *   status    in this order: T == 0 RD_EVAL_EMPTY; T > 2^19 RD_EVAL_TOO_LONG; a computed d4 == 0 RD_EVAL_MAD_ZERO; T < L
 *             RD_EVAL_NO_PATH; over the budget alone RD_EVAL_TOO_LARGE; otherwise RD_EVAL_OK
 *   outputs   status; score (int64: the end value); m2, d4 as used (0, 0 for EMPTY and TOO_LONG; whatever the status otherwise);
 *             first_step / last_step per base in READ sample coordinates (t_lo added): last_step[b] = first_step[b+1] - 1, last_step[L-1]
 *             is the last row in state L -- exactly what rd_event_stats accepts; ev_start .. ev_max: rd_event_stats of those steps;
 *             fit_sums[5 r ..]: N, sum l, sum l^2, sum x, sum x l over the samples that sit in base states, l the base's lvl and x the
 *             raw sample (all below 2^49): the normal equations of x = alpha + beta l.  A read that is not OK has score 0, zero sums and
 *             the "no path" outputs of rd_event_stats (-1, -1 and zeros; steps -1); it never affects its neighbours
 * A result does not depend on the batch, the order, the budget or the launches.  RD_ERR_ARG before anything is launched: a null pointer,
 * offsets that are not monotone, a code above 3, a window outside its read, a scale or a table entry outside its range.  n_reads == 0 is
 * RD_OK.
 *   rd_eventalign        on the GPU; synchronous, uses the context's stream.  budget_bytes and RD_ERR_NOMEM as rd_ctc_align_batch
 *                        (DESIGN.md section 19): the DP workspace one launch may take, rd_eventalign_workspace_bytes per read, 0 = a
 *                        quarter of the free device memory; a read that alone exceeds it is not aligned: RD_EVAL_TOO_LARGE, and the
 *                        call returns RD_ERR_NOMEM naming it after doing the others
 *   rd_eventalign_host   host, no GPU: the same rules (csrc/eventalign_rules.h) in a plain loop
 *   rd_eventalign_workspace_bytes   of a window of n_rows rows and n_bases bases, each term rounded up to 256:
 *                        4 n_rows (quantised samples) + 4 n_rows ceil((n_bases + 2) / 32) (back-pointers, one bit per cell)
 *                        + 8 n_rows (two band columns) when n_bases + 2 > 4096 */
#define RD_EVAL_OK 0
#define RD_EVAL_EMPTY 1
#define RD_EVAL_TOO_LONG 2
#define RD_EVAL_MAD_ZERO 3
#define RD_EVAL_NO_PATH 4
#define RD_EVAL_TOO_LARGE 5
int rd_eventalign(rd_ctx* ctx, const int16_t* raw, const int64_t* read_off, int n_reads, const int64_t* t_lo, const int64_t* t_hi,
                  const uint8_t* codes, const int64_t* ref_off, const int32_t* ref_len, const int32_t* m2_in, const int32_t* d4_in, int k,
                  const int32_t* lvl, const uint32_t* w, const int32_t* bias, int32_t lvl_bg, uint32_t w_bg, int32_t bias_bg,
                  int64_t budget_bytes, int32_t* status, int64_t* score, int32_t* m2, int32_t* d4, int32_t* first_step, int32_t* last_step,
                  int32_t* ev_start, int32_t* ev_end, int64_t* ev_sum, int64_t* ev_sumsq, int16_t* ev_min, int16_t* ev_max, int64_t* fit_sums);
int rd_eventalign_host(const int16_t* raw, const int64_t* read_off, int n_reads, const int64_t* t_lo, const int64_t* t_hi, const uint8_t* codes,
                       const int64_t* ref_off, const int32_t* ref_len, const int32_t* m2_in, const int32_t* d4_in, int k, const int32_t* lvl,
                       const uint32_t* w, const int32_t* bias, int32_t lvl_bg, uint32_t w_bg, int32_t bias_bg, int32_t* status, int64_t* score,
                       int32_t* m2, int32_t* d4, int32_t* first_step, int32_t* last_step, int32_t* ev_start, int32_t* ev_end, int64_t* ev_sum,
                       int64_t* ev_sumsq, int16_t* ev_min, int16_t* ev_max, int64_t* fit_sums);
int64_t rd_eventalign_workspace_bytes(int64_t n_rows, int64_t n_bases);

/* ---- eventalign on sample rows in a band round a guide (eventalign.hip) ---------------------------------
 * NO reference behaviour.  rd_eventalign over the states of a window of W = 64 (RD_EVAL_BAND_W) states that slides with a per-base guide:
 * the accuracy of sample rows at a workspace of O(T + L) bytes a read.  Integer arithmetic only; met exactly.  Inputs, window [t_lo,
 * t_hi), scale rule, model, zq, states 0 .. L + 1, the cell's cost, the strict tie-break, the end rule, the bounds and the outputs status,
 * score, m2, d4, first_step, last_step, ev_*, fit_sums are rd_eventalign's.  What is new:
 *   guide     guide[ref_off[r] + b], int32 in READ sample coordinates, one per base: the sample base b is expected to start at;
 *             non-decreasing within a read (equal values and jumps are normal: it is what rd_eventalign_events returns as ev_start, where
 *             a skipped base repeats a value)
 *   window    g(t) = #{b : guide[b] <= t_lo + t};  lo(t) = min(max(g(t) - 31, 0), max(L + 2 - 64, 0)), non-decreasing;
 *             win(t) = [lo(t), lo(t) + 63] within [0, L + 1]
 *   path      V[0][s] = c(0, s) for s in {0, 1} and in win(0); every other state of the window starts at 2^30.  Row t >= 1, s in win(t):
 *             stay = V[t-1][s] if s is in win(t-1), else 2^30; advance = V[t-1][s-1] if s - 1 >= lo(t) and s - 1 is in win(t-1), else
 *             2^30 -- a state that has left the window is gone at once, the window's lowest state has no advance edge;
 *             V = c + min(stay, advance), the advance only if STRICTLY smaller; one back-pointer bit.  Unreachable values may be computed
 *             unmasked: one that started at 2^30 stays in (0.875 * 2^30, 2^31), a finite one below 0.625 * 2^30
 *   end       rd_eventalign's rule over the states of {L, L + 1} that lie in win(T - 1), the other counting as 2^30.  If the chosen end
 *             value is not finite (>= 3 * 2^28) the window lost the path: RD_EVAL_OFF_BAND, with the not-OK outputs of rd_eventalign
 *   status    in this order: EMPTY, TOO_LONG, MAD_ZERO, NO_PATH (T < L), TOO_LARGE, OFF_BAND, OK
 *   n_edge    per read: the bases b (state s = b + 1) whose rows touch the window's rim -- lo(last_step[b] - t_lo) == s (the lower rim)
 *             or lo(first_step[b] - t_lo) + 63 == s (the upper rim); lo being monotone, that is "some row of the base sits on the rim".
 *             0 for a read that is not OK
 * IDENTITY.  If the path rd_eventalign finds on the same scale satisfies at every row t (lo(t) == 0 or s(t) > lo(t)) and s(t) <= lo(t) + 63,
 * every output of this call equals rd_eventalign's: banded values are minima over a subset of the full DP's paths, they are equal along
 * that path, and at every compare on it the edge that loses does not get better.  In particular L + 2 <= 64 gives rd_eventalign for
 * any guide.  A result does not depend on the batch, the order, the budget or the launches.  RD_ERR_ARG before anything is launched:
 * whatever rd_eventalign refuses; a null guide; a guide that decreases within a read.  n_reads == 0 is RD_OK.
 *   rd_eventalign_banded        on the GPU; synchronous, uses the context's stream; budget_bytes and RD_ERR_NOMEM as rd_eventalign
 *   rd_eventalign_banded_host   host, no GPU: the same rules (csrc/eventalign_rules.h) in a plain loop
 *   rd_eventalign_banded_workspace_bytes   of a window of n_rows rows and n_bases bases, each term rounded up to 256: 4 n_rows (quantised
 *                        samples) + 8 n_rows (back-pointers, one 64-bit word a row) + 4 n_rows (the window's lowest state per row)
 *                        + 12 (n_bases + 2 + 128) (the states' constants) */
#define RD_EVAL_OFF_BAND 6
#define RD_EVAL_BAND_W 64
int rd_eventalign_banded(rd_ctx* ctx, const int16_t* raw, const int64_t* read_off, int n_reads, const int64_t* t_lo, const int64_t* t_hi,
                         const uint8_t* codes, const int64_t* ref_off, const int32_t* ref_len, const int32_t* guide, const int32_t* m2_in,
                         const int32_t* d4_in, int k, const int32_t* lvl, const uint32_t* w, const int32_t* bias, int32_t lvl_bg, uint32_t w_bg,
                         int32_t bias_bg, int64_t budget_bytes, int32_t* status, int64_t* score, int32_t* m2, int32_t* d4, int32_t* n_edge,
                         int32_t* first_step, int32_t* last_step, int32_t* ev_start, int32_t* ev_end, int64_t* ev_sum, int64_t* ev_sumsq,
                         int16_t* ev_min, int16_t* ev_max, int64_t* fit_sums);
int rd_eventalign_banded_host(const int16_t* raw, const int64_t* read_off, int n_reads, const int64_t* t_lo, const int64_t* t_hi,
                              const uint8_t* codes, const int64_t* ref_off, const int32_t* ref_len, const int32_t* guide, const int32_t* m2_in,
                              const int32_t* d4_in, int k, const int32_t* lvl, const uint32_t* w, const int32_t* bias, int32_t lvl_bg, uint32_t w_bg,
                              int32_t bias_bg, int32_t* status, int64_t* score, int32_t* m2, int32_t* d4, int32_t* n_edge, int32_t* first_step,
                              int32_t* last_step, int32_t* ev_start, int32_t* ev_end, int64_t* ev_sum, int64_t* ev_sumsq, int16_t* ev_min,
                              int16_t* ev_max, int64_t* fit_sums);
int64_t rd_eventalign_banded_workspace_bytes(int64_t n_rows, int64_t n_bases);

/* ---- eventalign on event rows: weighted rows and base skips (eventalign.hip) ------------------------------
 * NO reference behaviour.  rd_eventalign's Viterbi over lead, base 1 .. base L, trail, with rows that are a detector's EVENTS, each
 * weighted by its sample count, and a third predecessor that skips one base.  Integer arithmetic only; met exactly.  With one event per
 * sample and skips off it is rd_eventalign on a given scale.  Model, states, ea_quant and the cell's cost are rd_eventalign's.
 *   read      n_samples[r] = T, the window's length, which closes the last event; sample_off[r] (>= 0, sample_off + T <= 2^31 - 1) is
 *             added to every reported sample index.  E = n_events[r] events at ev_off[r] + e of in_start, in_sum, in_sumsq, in_min, in_max,
 *             exactly as rd_segment returns them (in_start relative to the window); no raw sample is read.  codes / ref_off / ref_len and
 *             the model as rd_eventalign.  The scale (m2_in, d4_in) is always given (rd_segment's, or a refit); d4_in == 0 is
 *             RD_EVAL_MAD_ZERO.  skip_pen: -1 no skip edge, otherwise 0..256 in 1/32 nat
 *   rows      n_e = in_start[e+1] - in_start[e], T - in_start[E-1] for the last; x_e = floor((2 in_sum[e] + n_e) / (2 n_e)), the mean rounded
 *             half up; zq_e = rd_eventalign's sample rule on x_e
 *   cell      c(e, s) = n_e * cost(zq_e, s).  V[0][0] = c(0, 0), V[0][1] = c(0, 1); V[e][s] = c(e, s) + the best of three: stay
 *             V[e-1][s]; advance V[e-1][s-1], taken only if STRICTLY smaller than stay; skip V[e-1][s-2] + skip_pen (2 <= s <= L + 1), taken
 *             only if STRICTLY smaller than the best of the other two.  On ties: stay, advance, skip.  Lead to base 2 skips base 1; base
 *             L - 1 to the trail skips base L.  The path ends in L + 1, or in L if the trail is not strictly smaller
 *   bounds    T <= 2^19 and sum n_e = T: the weighted costs of a path sum to less than 2^19 * 1280; at most one skip per row, E <= T and
 *             skip_pen <= 256: finite values stay below 2^19 * 1536 = 0.75 * 2^30.  An unreachable cell (s > 2 e + 1; s > e + 1 without
 *             skips) starts at 2^30, stays above 2^30 - 2^19 * 256 = 0.875 * 2^30 and below 2^31, so computed unmasked it never wins.
 *             n_e < 2^23 and |cost| <= 1280: n_e * cost is exact as a 24-bit multiply
 *   status    in this order: T == 0 or E == 0 RD_EVAL_EMPTY; T > 2^19 RD_EVAL_TOO_LONG; d4_in == 0 RD_EVAL_MAD_ZERO; E < L without
 *             skips, 2 E - 1 < L with them RD_EVAL_NO_PATH; over the budget alone RD_EVAL_TOO_LARGE; otherwise RD_EVAL_OK
 *   outputs   per read status, score, n_skipped, fit_sums (rd_eventalign's, a skipped base adding nothing).  Per base at ref_off[r] + b:
 *             row_first / row_last, indices into the read's events (-1, -1 for a skipped base); ev_start / ev_end in read coordinates
 *             (sample_off added), for a skipped base both the start of the row at which the path jumped over it; ev_sum, ev_sumsq,
 *             ev_min, ev_max accumulated from the records of the base's rows, zeros for a skipped base.  A read that is not OK has score
 *             0, n_skipped 0, zero sums, -1 in row_first, row_last, ev_start, ev_end and zeros elsewhere; it never affects its neighbours
 * A result does not depend on the batch, the order, the budget or the launches.  RD_ERR_ARG before anything is launched: whatever
 * rd_eventalign refuses; E > 0 with in_start[0] != 0, starts that do not strictly increase or a start >= T; an event whose mean does not fit
 * int16; skip_pen outside -1..256.  n_reads == 0 is RD_OK.
 *   rd_eventalign_events        on the GPU; synchronous, uses the context's stream; budget_bytes and RD_ERR_NOMEM as rd_eventalign
 *   rd_eventalign_events_host   host, no GPU: the same rules (csrc/eventalign_rules.h) in a plain loop
 *   rd_eventalign_events_workspace_bytes   of n_rows events and n_bases bases, each term rounded up to 256: 8 n_rows (zq and n per row)
 *                        + 4 n_rows ceil((n_bases + 2) / 16) (back-pointers, two bits per cell) + 16 n_rows (two band columns of two
 *                        cells per row) when n_bases + 2 > 4096 */
int rd_eventalign_events(rd_ctx* ctx, int n_reads, const int64_t* n_samples, const int64_t* sample_off, const int64_t* ev_off,
                         const int32_t* n_events, const int32_t* in_start, const int64_t* in_sum, const int64_t* in_sumsq, const int16_t* in_min,
                         const int16_t* in_max, const uint8_t* codes, const int64_t* ref_off, const int32_t* ref_len, const int32_t* m2_in,
                         const int32_t* d4_in, int k, const int32_t* lvl, const uint32_t* w, const int32_t* bias, int32_t lvl_bg, uint32_t w_bg,
                         int32_t bias_bg, int skip_pen, int64_t budget_bytes, int32_t* status, int64_t* score, int32_t* n_skipped,
                         int32_t* row_first, int32_t* row_last, int32_t* ev_start, int32_t* ev_end, int64_t* ev_sum, int64_t* ev_sumsq,
                         int16_t* ev_min, int16_t* ev_max, int64_t* fit_sums);
int rd_eventalign_events_host(int n_reads, const int64_t* n_samples, const int64_t* sample_off, const int64_t* ev_off, const int32_t* n_events,
                              const int32_t* in_start, const int64_t* in_sum, const int64_t* in_sumsq, const int16_t* in_min, const int16_t* in_max,
                              const uint8_t* codes, const int64_t* ref_off, const int32_t* ref_len, const int32_t* m2_in, const int32_t* d4_in,
                              int k, const int32_t* lvl, const uint32_t* w, const int32_t* bias, int32_t lvl_bg, uint32_t w_bg, int32_t bias_bg,
                              int skip_pen, int32_t* status, int64_t* score, int32_t* n_skipped, int32_t* row_first, int32_t* row_last,
                              int32_t* ev_start, int32_t* ev_end, int64_t* ev_sum, int64_t* ev_sumsq, int16_t* ev_min, int16_t* ev_max,
                              int64_t* fit_sums);
int64_t rd_eventalign_events_workspace_bytes(int64_t n_rows, int64_t n_bases);

/* ---- modcall: per-read modification calls by local re-alignment under two models (modcall.hip) --------------
 * NO reference behaviour.  A job is a (read, site) pair.  The rows between two anchors of an alignment the caller already has are
 * re-aligned to the at most 63 states round the site, under the canonical model (ref) and with the job's entries in place of some states
 * (alt); per hypothesis the best path (vit) and the sum over all paths (fwd, the forward algorithm) are returned as negative log
 * likelihoods in 1/32 nat.  Integer arithmetic only; met exactly.  The rules are csrc/modcall_rules.h.
 *   reads     raw, read_off, n_reads as rd_eventalign (the whole read, no window).  Per read a GIVEN scale (m2[r], d4[r]): d4 == 0 or a value
 *             outside rd_eventalign's ranges is RD_ERR_ARG.  codes / ref_off / ref_len in pore order, as rd_eventalign.  first / last per
 *             base at ref_off[r] + b, int32 in READ sample coordinates: what rd_eventalign and rd_eventalign_banded return as first_step
 *             and last_step, or ev_start and ev_end - 1 of event rows; -1 marks a base without rows
 *   model     k, lvl, w, bias as rd_eventalign.  No background takes part
 *   jobs      n_jobs of them: job_read[j]; alt_first[j], the pore-order index of the first base whose state is replaced; the replacing
 *             entries alt_lvl / alt_w / alt_bias at alt_off[j] .. alt_off[j+1] (alt_off holds n_jobs + 1 offsets).  1 <= n_alt <= 9,
 *             alt_first >= 0, alt_first + n_alt <= L, every entry within the model's ranges; a flank F for all jobs, 0 <= F <= 27
 *   window    a0 = max(0, alt_first - F), a1 = min(L - 1, alt_first + n_alt - 1 + F), S = a1 - a0 + 1 <= 63 states; rows r0 = first[a0] ..
 *             r1 = last[a1], R = r1 - r0 + 1
 *   status    in this order: either anchor -1 RD_MC_NO_ANCHOR; R < S or rows outside the read RD_MC_NO_PATH; R > 2^15 RD_MC_TOO_LONG;
 *             the read alone over the budget RD_MC_TOO_LARGE; otherwise RD_MC_OK
 *   cell      zq = rd_eventalign's sample rule on raw[r0 + t]; c(t, i) = rd_eventalign's cell cost of zq against state i.  ref: state i is
 *             base a0 + i's k-mer.  alt: the same, the job's entries in place of bases alt_first .. alt_first + n_alt - 1
 *   path      anchored at both ends: V[0][0] = c(0, 0), every other state starts at 2^30.  Per hypothesis vit = c + min(stay, adv) and
 *             fwd = c + softmin(stay, adv), softmin(a, b) = min(a, b) - LSE[min(|a - b|, 133)], LSE[d] = floor(32 ln(1 + e^(-d/32)) + 1/2),
 *             a literal of 134 integers (LSE[0] = 22, LSE[133] = 0); state 0 has no advance (2^30).  No libm on either side
 *   bounds    finite values lie in (-2^15 * 278, 2^15 * 1280], below 3 * 2^28; a value that started at 2^30 stays in [2^30 - 22 * 2^15, 2^31); the
 *             two differ by more than 133, so LSE contributes 0 between them and nothing is masked
 *   outputs   per job status, n_rows = R, n_states = S and the four values at (R - 1, S - 1): vit_ref, vit_alt, fwd_ref, fwd_alt (int32).  A
 *             job that is not OK returns zeros in all six
 * fwd <= vit <= fwd + 22 (R - 1).  Alt entries equal to the canonical ones give *_alt == *_ref.  With first / last from rd_eventalign on the
 * same scale vit_ref is the summed cell cost of that path over rows r0 .. r1 (a sub-path of an optimal path is optimal between its ends);
 * from any other steps it is at most that sum.  A result does not depend on the batch, the order of reads or jobs, the budget or the
 * launches.  RD_ERR_ARG before anything is launched: a null pointer, offsets that are not monotone, a code above 3, a scale, a table or alt
 * entry, a flank or a job outside its range.  n_jobs == 0 is RD_OK.
 *   rd_modcall        on the GPU; synchronous, uses the context's stream.  budget_bytes and RD_ERR_NOMEM as rd_eventalign (DESIGN.md section
 *                     19): the reads that have jobs are packed into launches in the caller's order, rd_modcall_workspace_bytes per read,
 *                     0 = a quarter of the free device memory; a read that alone exceeds it has all its jobs RD_MC_TOO_LARGE, and the call
 *                     returns RD_ERR_NOMEM naming it after doing the others
 *   rd_modcall_host   host, no GPU: the same rules in a plain loop (no budget: never RD_MC_TOO_LARGE)
 *   rd_modcall_workspace_bytes   of a read of n_samples samples and n_bases bases with n_jobs jobs of n_alt entries in all, each term
 *                     rounded up to 256: 2 n_samples (samples) + 8 n_bases (steps) + 64 n_jobs (descriptors) + 32 n_jobs (results)
 *                     + 12 n_alt (entries) */
#define RD_MC_OK 0
#define RD_MC_NO_ANCHOR 1
#define RD_MC_NO_PATH 2
#define RD_MC_TOO_LONG 3
#define RD_MC_TOO_LARGE 4
int rd_modcall(rd_ctx* ctx, const int16_t* raw, const int64_t* read_off, int n_reads, const int32_t* m2, const int32_t* d4, const uint8_t* codes,
               const int64_t* ref_off, const int32_t* ref_len, const int32_t* first, const int32_t* last, int k, const int32_t* lvl,
               const uint32_t* w, const int32_t* bias, int n_jobs, const int32_t* job_read, const int32_t* alt_first, const int64_t* alt_off,
               const int32_t* alt_lvl, const uint32_t* alt_w, const int32_t* alt_bias, int flank, int64_t budget_bytes, int32_t* status,
               int32_t* n_rows, int32_t* n_states, int32_t* vit_ref, int32_t* vit_alt, int32_t* fwd_ref, int32_t* fwd_alt);
int rd_modcall_host(const int16_t* raw, const int64_t* read_off, int n_reads, const int32_t* m2, const int32_t* d4, const uint8_t* codes,
                    const int64_t* ref_off, const int32_t* ref_len, const int32_t* first, const int32_t* last, int k, const int32_t* lvl,
                    const uint32_t* w, const int32_t* bias, int n_jobs, const int32_t* job_read, const int32_t* alt_first, const int64_t* alt_off,
                    const int32_t* alt_lvl, const uint32_t* alt_w, const int32_t* alt_bias, int flank, int32_t* status, int32_t* n_rows,
                    int32_t* n_states, int32_t* vit_ref, int32_t* vit_alt, int32_t* fwd_ref, int32_t* fwd_alt);
int64_t rd_modcall_workspace_bytes(int64_t n_samples, int64_t n_bases, int64_t n_jobs, int64_t n_alt);

/* ---- sigmap: raw samples against a panel of targets, subsequence Viterbi with a free start and end (sigmap.hip)
 * NO reference behaviour.  Which targets of a panel a window of samples fits best, where the fit ends in each and where it began.  No
 * basecall and no neural network take part.  Integer arithmetic only; met exactly.  Sample, cell and the three model tables are
 * rd_eventalign's (no background).
 *   panel     n_tgt targets, base codes 0..3 in pore order: codes[tgt_off[j] .. tgt_off[j+1]); tgt_off[0] = 0, non-decreasing; an empty
 *             target holds no state.  State s is a global index 0 .. R - 1, R = tgt_off[n_tgt] <= 2^31 - 1; its model is the k-mer centred
 *             on it WITHIN ITS OWN TARGET (rd_sim_signal's rule: a position outside the target takes the nearest end base)
 *   query     q of n_q: rows are the samples raw[q_lo[q] .. q_hi[q]), T = q_hi - q_lo <= 2^14; all indices are absolute into raw
 *             (n_raw samples), and several queries may name the same samples.  Scale: d4_in[q] > 0: (m2_in[q], d4_in[q]) as given;
 *             d4_in[q] == 0: that of the scale window raw[sc_lo[q] .. sc_hi[q]) (at most 2^31 - 1 samples) by rd_eventalign's rule, an
 *             empty scale window giving (0, 0).  States: the range [s_lo[q], s_hi[q])
 *   path      int32.  head(s): s is the first state of its target, or s == s_lo.  V[0][s] = c(0, s), O[0][s] = s;
 *             V[t][s] = c(t, s) + (adv ? V[t-1][s-1] : V[t-1][s]), adv = !head(s) and V[t-1][s-1] STRICTLY smaller than V[t-1][s];
 *             O[t][s] is the O of the predecessor taken.  No cell is unreachable, no path crosses from a target into the next, every
 *             value stays inside +-2^14 * 1280 < 2^25
 *   result    per target with a state in range: the smallest V[T-1][s] over them, the smallest s on ties.  Per query the n_best (1..8)
 *             such targets ordered by (score, j): best_tgt / best_score / best_end / best_org, int32 [n_q][n_best], end and origin state
 *             local to the target (tgt_off[j] subtracted); slots past the number of targets hold -1 in all four
 *   status    in this order: T == 0 RD_SIGMAP_EMPTY; T > 2^14 RD_SIGMAP_TOO_LONG; a computed d4 == 0 RD_SIGMAP_MAD_ZERO; s_lo == s_hi
 *             RD_SIGMAP_NO_TARGET; over the budget alone RD_SIGMAP_TOO_LARGE; otherwise RD_SIGMAP_OK.  m2, d4 as used (0, 0 for EMPTY
 *             and TOO_LONG; whatever the status otherwise).  A query that is not OK has -1 in every slot
 * A result does not depend on the batch, the order, the budget or the launches.  RD_ERR_ARG before anything is launched: a null pointer,
 * offsets that are not monotone, a code above 3, a window or a range out of order or outside its array, a scale or a table entry outside
 * rd_eventalign's ranges, n_best outside 1..8.  n_q == 0 is RD_OK.
 *   rd_sigmap        on the GPU; synchronous, uses the context's stream.  Every query's scale is settled first.  budget_bytes and
 *                    RD_ERR_NOMEM as rd_eventalign: the DP workspace one launch may take, rd_sigmap_workspace_bytes per query, 0 = a
 *                    quarter of the free device memory; a query that alone exceeds it is not mapped: RD_SIGMAP_TOO_LARGE, and the call
 *                    returns RD_ERR_NOMEM naming the first such query after doing the others
 *   rd_sigmap_host   host, no GPU: the same rules (csrc/sigmap_rules.h) in a plain loop
 *   rd_sigmap_workspace_bytes   of a query of n_rows rows over n_states states whose first and last state lie in targets j_lo and j_hi,
 *                    n_tgt_in_range = j_hi - j_lo + 1; each term rounded up to 256; P = 6145, the end states one stripe reports:
 *                    4 n_rows (quantised samples) + 4 n_states (the origin of every end state) + 8 n_tgt_in_range (one key per target)
 *                    + ceil(n_states / P) * round256(16 n_rows) (two band columns per stripe) when min(n_states, P + n_rows - 1) > 4096 */
#define RD_SIGMAP_OK 0
#define RD_SIGMAP_EMPTY 1
#define RD_SIGMAP_TOO_LONG 2
#define RD_SIGMAP_MAD_ZERO 3
#define RD_SIGMAP_NO_TARGET 4
#define RD_SIGMAP_TOO_LARGE 5
int rd_sigmap(rd_ctx* ctx, const int16_t* raw, int64_t n_raw, int n_q, const int64_t* q_lo, const int64_t* q_hi, const int64_t* sc_lo,
              const int64_t* sc_hi, const int32_t* m2_in, const int32_t* d4_in, const int64_t* s_lo, const int64_t* s_hi, const uint8_t* codes,
              const int64_t* tgt_off, int n_tgt, int k, const int32_t* lvl, const uint32_t* w, const int32_t* bias, int n_best,
              int64_t budget_bytes, int32_t* status, int32_t* m2, int32_t* d4, int32_t* best_tgt, int32_t* best_score, int32_t* best_end,
              int32_t* best_org);
int rd_sigmap_host(const int16_t* raw, int64_t n_raw, int n_q, const int64_t* q_lo, const int64_t* q_hi, const int64_t* sc_lo,
                   const int64_t* sc_hi, const int32_t* m2_in, const int32_t* d4_in, const int64_t* s_lo, const int64_t* s_hi,
                   const uint8_t* codes, const int64_t* tgt_off, int n_tgt, int k, const int32_t* lvl, const uint32_t* w, const int32_t* bias,
                   int n_best, int32_t* status, int32_t* m2, int32_t* d4, int32_t* best_tgt, int32_t* best_score, int32_t* best_end,
                   int32_t* best_org);
int64_t rd_sigmap_workspace_bytes(int64_t n_rows, int64_t n_states, int64_t n_tgt_in_range);

/* ---- event detection: a read's raw samples cut into stretches of roughly constant level (segment.hip) -------
 * NO reference behaviour.  Two sliding Welch t-tests, a short and a long window, and non-maximum suppression of their t^2; no sequential
 * peak state as in scrappie's detector.  Integer arithmetic only; met exactly.  Read r is samples raw + read_off[r] .. read_off[r+1]
 * (T of them).  Parameters (anything outside its range is RD_ERR_ARG): w1 2..32 (short window); w2 0 (detector 2 off) or
 * w1 < w2 <= 64 (long window); th1, th2 (uint32: the t^2 thresholds in sixteenths); v0 1..65536 (variance floor in DAQ^2).
 * For a detector with window w and a sample i in [w, T - w]:
 *   S1, Q1 = the sum and the sum of squares of x[i - w .. i), S2, Q2 of x[i .. i + w)
 *   N(i) = w (S1 - S2)^2; D(i) = w Q1 - S1^2 + w Q2 - S2^2 + 2 w^2 v0; t^2(i) = N / D.  Outside that range N = 0, D = 1.
 *   N < 2^50 and 2 w^2 <= D < 2^44; t(j) < t(i) means N(j) D(i) < N(i) D(j), the products in 128 bits
 *   candidate  N(i) > 0 and 16 N(i) >= th D(i)
 *   peak       a candidate with t(j) < t(i) for every j in [i - w, i) and t(j) <= t(i) for every j in (i, i + w], j inside the read:
 *              non-maximum suppression of radius w, ties to the smaller index
 *   boundary   a peak of detector 1, or a peak of detector 2 with no peak of detector 1 at |j - i| < w2
 *   events     event 0 starts at sample 0, every boundary starts the next event; an event ends where the next starts, or at T.
 *              Boundaries lie more than w1 apart: every event is non-empty and n_events <= T / (w1 + 1) + 1 = rd_segment_max_events
 *   status     in this order: T == 0 RD_SEGMENT_EMPTY; T > 2^30 RD_SEGMENT_TOO_LONG (its samples are never read); over the budget alone
 *              RD_SEGMENT_TOO_LARGE; otherwise RD_SEGMENT_OK
 *   outputs    per read status and n_events (0 unless OK).  Per event, at ev_off[r] + e (ev_off [n_reads + 1], non-decreasing; an OK
 *              read's room ev_off[r+1] - ev_off[r] is at least rd_segment_max_events(T, w1)): ev_start (sample of the read), ev_sum,
 *              ev_sumsq, ev_min, ev_max over its samples, ev_src (0 for event 0, otherwise 1 or 2: the detector that cut it).  With
 *              sc_lo / sc_hi (both or neither; absolute indices into raw, read_off[r] <= sc_lo[r] <= sc_hi[r] <= read_off[r+1]) m2 and
 *              d4 of an OK read are the scale of raw[sc_lo[r] .. sc_hi[r]) by rd_eventalign's rule, (0, 0) for an empty window and for
 *              every other status; without them m2 and d4 may be null
 * A read never affects its neighbours; a result does not depend on the batch, the order, the budget or the launches.  RD_ERR_ARG before
 * anything is launched: a null pointer, offsets that are not monotone, too little room for a read's events, a scale window outside its
 * read, a parameter outside its range.  n_reads == 0 is RD_OK.
 *   rd_segment        on the GPU; synchronous, uses the context's stream.  budget_bytes and RD_ERR_NOMEM as rd_polya_segment:
 *                     rd_segment_workspace_bytes per read, 0 = a quarter of the free device memory; a read that alone exceeds it is not
 *                     looked at: RD_SEGMENT_TOO_LARGE, and the call returns RD_ERR_NOMEM naming it after doing the others
 *   rd_segment_host   host, no GPU: the same rules (csrc/segment_rules.h) in plain loops
 *   rd_segment_workspace_bytes   8 T + T / 32 + 32 (T / (w1 + 1) + 1) + 8 (T / 2048 + 1) + 8192: the samples, two flag bytes and a scan
 *                     entry per sample, the scan's own block, 29 B per possible event, the tile descriptors
 *   rd_segment_max_events        T / (w1 + 1) + 1 (-1 for a negative T or a w1 outside its range, as rd_segment_workspace_bytes)
 *   rd_segment_diag_tstat  the first stage alone, through the same kernel, for stage tests (it changes no result and has no budget; at
 *                     most 2^31 - 1 samples, no read above 2^30): with n = read_off[n_reads] - read_off[0] and g = the sample's index
 *                     minus read_off[0], t_num / t_den [2][n] hold N and D of detector d at [d n + g] (N = 0, D = 1 throughout for
 *                     w2 == 0) and peak [n] bit 0 for a peak of detector 1, bit 1 of detector 2 */
#define RD_SEGMENT_OK 0
#define RD_SEGMENT_EMPTY 1
#define RD_SEGMENT_TOO_LONG 2
#define RD_SEGMENT_TOO_LARGE 3
int rd_segment(rd_ctx* ctx, const int16_t* raw, const int64_t* read_off, int n_reads, int w1, int w2, uint32_t th1, uint32_t th2, int v0,
               const int64_t* sc_lo, const int64_t* sc_hi, const int64_t* ev_off, int64_t budget_bytes, int32_t* status, int32_t* n_events,
               int32_t* m2, int32_t* d4, int32_t* ev_start, int64_t* ev_sum, int64_t* ev_sumsq, int16_t* ev_min, int16_t* ev_max,
               uint8_t* ev_src);
int rd_segment_host(const int16_t* raw, const int64_t* read_off, int n_reads, int w1, int w2, uint32_t th1, uint32_t th2, int v0,
                    const int64_t* sc_lo, const int64_t* sc_hi, const int64_t* ev_off, int32_t* status, int32_t* n_events, int32_t* m2,
                    int32_t* d4, int32_t* ev_start, int64_t* ev_sum, int64_t* ev_sumsq, int16_t* ev_min, int16_t* ev_max, uint8_t* ev_src);
int64_t rd_segment_workspace_bytes(int64_t n_samples, int w1);
int64_t rd_segment_max_events(int64_t n_samples, int w1);
int rd_segment_diag_tstat(rd_ctx* ctx, const int16_t* raw, const int64_t* read_off, int n_reads, int w1, int w2, uint32_t th1, uint32_t th2,
                          int v0, uint64_t* t_num, uint64_t* t_den, uint8_t* peak);

/* ---- model evaluation on labelled windows: the reference's val_loss (radian/model.py:77-98, radian/train.py:48-79) ------------
 * Labelled windows as the reference stores them: TFRecord shards of tf.train.Example records (radian/data.py:9-31), read on the
 * HOST without TensorFlow (tfrecord.hip).  Framing: u64 length, u32 masked crc32c of it, the data, u32 masked crc32c of the data;
 * both checksums are verified.  Features: `signal` 1024 floats, `label` a float list (the first label_length values are the labels,
 * each exactly 0..3), `signal_length` (1..1024) and `label_length` (0..len(label)) one int64 each; repeated fields packed or not.
 *   rd_tfrecord_open / rd_tfrecord_open_mem (the buffer is parsed at once and may be released after the call) / rd_tfrecord_close
 *   rd_tfrecord_count   records of the shard and the total of their labels
 *   rd_tfrecord_read    records [lo, hi): signals [hi - lo][1024] float32, input_len (= signal_length), label_off [hi - lo + 1] into
 *                       labels (capacity labels_cap, 0..3 each), label_len
 * Anything else -- a bad checksum, a truncated frame, a missing or malformed feature, a value outside the ranges above -- returns
 * RD_ERR_FORMAT with a message naming the record's index; rd_tfrecord_open returns RD_ERR_IO when the file cannot be read.
 * rd_crc32c: the Castagnoli CRC of a buffer (unmasked; crc32c("123456789") = 0xE3069283).
 *   rd_tfrecord_write   the writer of the same shards: n records to path (created or truncated; append != 0: added at its end), record i
 *                       with signals[i][1024], signal_length input_len[i] (1..1024) and the label_len[i] labels (0..3 each) at
 *                       labels + label_off[i].  `signal` and `label` are packed float lists, the lengths one int64 each, map entries
 *                       in key order, both checksums per frame: the bytes depend on the arguments only, and rd_tfrecord_read returns
 *                       exactly what was written.  RD_ERR_ARG for a value outside those ranges (nothing is written), RD_ERR_IO when
 *                       the file cannot be written. */
typedef struct rd_tfrecord rd_tfrecord;
int rd_tfrecord_open(const char* path, rd_tfrecord** out);
int rd_tfrecord_open_mem(const void* buf, size_t n, rd_tfrecord** out);
void rd_tfrecord_close(rd_tfrecord* f);
int rd_tfrecord_count(const rd_tfrecord* f, int64_t* n_records, int64_t* n_labels);
int rd_tfrecord_read(const rd_tfrecord* f, int64_t lo, int64_t hi, float* signals, int32_t* input_len, int64_t* label_off,
                     int32_t* label_len, uint8_t* labels, int64_t labels_cap);
uint32_t rd_crc32c(const void* buf, size_t n);
int rd_tfrecord_write(const char* path, const float* signals, const int32_t* input_len, const uint8_t* labels, const int64_t* label_off,
                      const int32_t* label_len, int64_t n, int append);

/* ---- label windows for training shards: fitting alignment of window calls against reference sequences (fit.hip, DESIGN.md
 * section 14; radian_amd/label_build.py) ------------------------------------------------------------------------------------
 * Query p = queries[query_off[p] .. query_off[p+1]) (codes 0..3, m <= 1024 of them) is fitted into reference query_ref[p] =
 * refs[ref_off[r] .. ref_off[r+1]) (codes 0..4; code 4, any letter that is not A C G T, matches nothing, itself included): the
 * whole query is aligned, the reference before and after the span it covers is free.  Offsets have count + 1 entries and start
 * at 0.  Many queries may name one reference; it is uploaded once per batch, not once per query.
 *   Gotoh's three states, int32, reference = rows i, query = columns j, a gap of length L costs gap_open + (L-1) * gap_extend:
 *     H(i,0) = 0;  H(0,j) = F(0,j) = gap_open + (j-1) * gap_extend (j >= 1);  E(i,0) = F(i,0) = E(0,j) = -inf
 *     E(i,j) = max(H(i-1,j) + open, E(i-1,j) + extend)      deletion: consumes a reference base
 *     F(i,j) = max(H(i,j-1) + open, F(i,j-1) + extend)      insertion: consumes a query base
 *     H(i,j) = max(H(i-1,j-1) + s(r[i-1], q[j-1]), E(i,j), F(i,j))
 *   score[p]       max over i of H(i,m)
 *   ref_end[p]     the smallest i that attains it
 *   ref_start[p]   the row in which the traceback from (ref_end, m) reaches column 0; the traceback has rd_align_batch's fixed
 *                  preference: diagonal, then E, then F, and inside a gap run extending before closing.  The query's label is
 *                  the reference's [ref_start, ref_end)
 *   counts[4p..]   n_match, n_sub, n_ins, n_del of the traced columns (no soft clip)
 *   status[p]      RD_FIT_OK; RD_FIT_EMPTY (m = 0: nothing to fit, outputs 0); RD_FIT_TOO_LARGE (see budget_bytes)
 *   budget_bytes   the kernel keeps no per-cell state (what the traceback would find is carried through the recurrence), so the
 *                  budget caps the call's own device buffer: the references, queries, descriptors and results of one batch.
 *                  0 = a quarter of the free device memory.  Queries are packed into batches under it in reference order; one
 *                  whose reference and query alone exceed it is not aligned: status RD_FIT_TOO_LARGE, and the call returns
 *                  RD_ERR_NOMEM naming it after aligning the others.  Results do not depend on the batches.
 * A code outside its range, a query longer than 1024 or a reference index outside 0..n_refs-1 is RD_ERR_ARG before anything is
 * launched.  So are a |score| >= 2^16, a reference with max|score| * (n + 1025) >= 2^28 (int32 scores), and gap_open > gap_extend
 * (equal, linear gaps, is legal): with open > extend the recurrence reopens adjacent gaps, so the score is not the stated gap cost.
 * Synchronous; uses the context's stream. */
#define RD_FIT_OK 0
#define RD_FIT_EMPTY 1
#define RD_FIT_TOO_LARGE 2
int rd_fit_batch(rd_ctx* ctx, const uint8_t* refs, const int64_t* ref_off, int64_t n_refs, const uint8_t* queries, const int64_t* query_off,
                 const int32_t* query_ref, int64_t n_queries, int match, int mismatch, int gap_open, int gap_extend, int64_t budget_bytes,
                 int32_t* score, int32_t* ref_start, int32_t* ref_end, int32_t* counts, int32_t* status);

/* ---- reads onto transcripts: minimizer seeds, chains, the best transcript of every read (map.hip, DESIGN.md section 15;
 * radian_amd/map.py writes align's and label_build's read_ref.tsv with it).  The reference makes that file outside its own tree with
 * minimap2 (radian/align.py:62,87; radian/accuracy.py parses its SAM).  Forward strand only.  Everything below is integer arithmetic:
 * results are exact and depend on neither the budget nor the way reads are grouped into calls.
 * Records (transcripts, reads) are codes back to back with count + 1 offsets that start at 0; codes 0..3 are A C G T, any other value
 * (rd_fasta_scan's 255, an N) is a break.
 *   Seeds      a k-mer (RD_MAP_MIN_K <= k <= RD_MAP_MAX_K) exists where k consecutive codes are 0..3; packed 2 bits per base, first base
 *              highest, into x < 2^2k.  Its hash: x = x * RD_MAP_HASH_C1 mod 2^2k; x ^= x >> k; x = x * RD_MAP_HASH_C2 mod 2^2k; x ^= x >> k
 *              (both constants odd: the map is invertible on 2k bits).  A segment is a maximal run of codes 0..3 within one record.  In
 *              every window of w (1..64) consecutive k-mers of one segment the k-mer with the smallest (hash, position) is a minimizer; a
 *              segment with fewer than w k-mers gives its single minimum.  The minimizers of a record are the distinct positions chosen.
 *   Index      rd_map_index: for every minimizer of every transcript, hash -> (transcript t, position r); the entries of one hash are in
 *              ascending (t, r).  Built on the device, kept in the context (a second call replaces it).  A hash with more than max_occ
 *              entries is not used for seeding.  Fewer than 2^24 transcripts of fewer than 2^24 codes each, fewer than 2^31 codes and
 *              records together: RD_ERR_ARG otherwise.  stats[8] (nullable): [0] entries, [1] distinct hashes, [2] hashes over max_occ,
 *              [3] [4] microseconds of the seeding and of the sort.
 *   Anchors    for every minimizer of a read at q whose hash is usable, one anchor (t, r, q) per index entry; a read's anchors are
 *              ordered by (t, r, q), and those of one t are a segment.
 *   Chains     over a segment's anchors in that order, with dq = q_i - q_j, dr = r_i - r_j:
 *                f(i) = max(k, max_j f(j) + min(dq, dr, k) - gap(|dr - dq|)),   gap(0) = 0, gap(d) = (d * k >> 6) + (floor(log2 d) >> 1)
 *              j over the RD_MAP_LOOKBACK anchors before i in the segment with 0 < dq <= max_gap, 0 < dr <= max_gap and
 *              |dr - dq| <= bandwidth.  Anchor i extends the best j when that candidate is greater than k, and of equal candidates the
 *              nearest j; otherwise it starts a chain of its own.  The chain's first anchor and anchor count travel with f (no
 *              back-pointer pass).  The segment's chain ends at the smallest i with the largest f; it qualifies with at least
 *              min_anchors anchors and a score of at least min_score.
 *   rd_map_batch  per read: status[p] and hits[8p..] = t, score, score2, n_anchors, q0, r0, q1, r1: the transcript of the qualifying
 *              chain with the largest score (of equal scores the smallest t), the best qualifying score on any other transcript or 0,
 *              the chain's anchor count, and its first (q0, r0) and last (q1, r1) anchors.  status: RD_MAP_OK; RD_MAP_NO_SEED (no
 *              anchor: hits 0); RD_MAP_NO_CHAIN (anchors, but no qualifying chain: hits 0); RD_MAP_TOO_LARGE (see budget_bytes).
 *              RD_MAP_EMPTY_SPAN is never returned here: radian_amd/map.py gives it to a read whose fitted span is empty.
 *   budget_bytes  bounds the anchor workspace (64 bytes per anchor of a launch + 1 MiB); 0 = a quarter of the free device memory.  A
 *              count pass and a scan give every read's anchors before anything is allocated; consecutive reads are packed into
 *              launches under the budget (at most 65535 reads each), a fill pass writes the anchors.  A read that alone exceeds the
 *              budget is not mapped: status RD_MAP_TOO_LARGE, and the call returns RD_ERR_NOMEM naming it after mapping the others.
 *              stats[16] (nullable): [0] launches, [1] read minimizers, [2] anchors, [3] segments, [8..13] microseconds of seeds,
 *              count + scan, fill, sort, segments + chains, best-of-read (asking for them synchronises between the stages).
 *   rd_map_minimizers  host, no context: the minimizer positions (ascending) and hashes of one record, from the same code the
 *              device runs.  *n_out is their number; at most cap are written (pos, hash nullable).
 * RD_ERR_STATE for rd_map_batch without an index.  Synchronous; the context's stream. */
#define RD_MAP_HASH_C1 0x9E3779B1u
#define RD_MAP_HASH_C2 0x85EBCA6Bu
#define RD_MAP_MIN_K 8
#define RD_MAP_MAX_K 15
#define RD_MAP_LOOKBACK 64
#define RD_MAP_OK 0
#define RD_MAP_NO_SEED 1
#define RD_MAP_NO_CHAIN 2
#define RD_MAP_TOO_LARGE 3
#define RD_MAP_EMPTY_SPAN 4
int rd_map_minimizers(const uint8_t* codes, int64_t n, int k, int w, int32_t* pos, uint32_t* hash, int64_t cap, int64_t* n_out);
int rd_map_index(rd_ctx* ctx, const uint8_t* codes, const int64_t* offsets, int64_t n_records, int k, int w, int max_occ, int64_t* stats);
int rd_map_batch(rd_ctx* ctx, const uint8_t* reads, const int64_t* read_off, int64_t n_reads, int min_anchors, int min_score, int max_gap,
                 int bandwidth, int64_t budget_bytes, int32_t* status, int32_t* hits, int64_t* stats);

/* ---- transcript quantification: the candidate transcripts of every read, then an expectation-maximisation over them in fixed-point
 * integers (map.hip, quant.hip; radian_amd/quant.py).  No length normalisation: in direct RNA one read is one
 * molecule.  Everything is integer arithmetic: results are exact against the text below and depend on neither budget, batches nor order.
 *   rd_map_candidates  the arguments, index, seeds, chains, budget contract and launches of rd_map_batch; per read p the K = max_cand
 *              (1..RD_MAP_MAX_CAND) best qualifying chains instead of the best one.
 *              Qualify    a segment (read, t) qualifies as in rd_map_batch: n_anchors >= min_anchors and score >= min_score.
 *              d3         with transcript length n_t and read length L, d3 = (n_t - r1) - (L - q1): the transcript's bases after the
 *                         chain's last anchor less the read's bases after it; negative when the read runs past the transcript's end.
 *                         With max_3p >= 0 (-1: off) a qualifying segment also needs d3 <= max_3p.
 *              Candidates best = the largest score of the segments that pass; a passing segment is a candidate when
 *                         score * 1024 >= best * min_frac_q10 (0..1024).  n_qual[p] counts them.
 *              Order      (score descending, t ascending); the first n_cand[p] = min(n_qual, K) are written, the other rows are 0:
 *                         cands[(p K + j) 8 ..] = t, score, n_anchors, q0, r0, q1, r1, d3.  With max_3p = -1 row 0 is rd_map_batch's
 *                         hit of the read (t, score, n_anchors, q0, r0, q1, r1).
 *              status     RD_MAP_OK; RD_MAP_NO_SEED; RD_MAP_NO_CHAIN (also when the 3' filter leaves nothing); RD_MAP_TOO_LARGE, with
 *                         RD_ERR_NOMEM naming the read, as rd_map_batch.  stats[16] as rd_map_batch; [13] is 0 and [14] holds the
 *                         microseconds of the candidate stage.
 *   rd_quant_em  Read r has the candidates cand_t (int32) / cand_w (uint16) [cand_off[r] .. cand_off[r+1]), cand_off int64 [n_reads + 1]
 *              from 0; n_reads < 2^31, n_tx < 2^24, max_iter 0..100000.  RD_ERR_ARG before anything is written unless every read has
 *              0..64 candidates, every t is in 0..n_tx-1, the t of one read are distinct and every w is in 1..4096.  ONE = 2^20:
 *                step(c)  for every read with candidates: a_j = c[t_j] w_j; S = sum_j a_j; sh = max(0, bitlen(S) - 44); a'_j = a_j >> sh;
 *                         S' = sum_j a'_j; share_j = floor(a'_j 2^20 / S'); c'[t] = the sum of the shares that name t
 *                c_0 = step(1, ..., 1); for i = 1 .. max_iter: c_i = step(c_{i-1}), d_i = max_t |c_i[t] - c_{i-1}[t]|; stop after
 *                iteration i when d_i <= tol_q20
 *              count_q20 [n_tx] (uint64) = the last c; share_q20 [cand_off[n_reads]] (uint32, nullable) = the shares of the last step
 *              executed, so count[t] is always the sum of the shares that name t.
 *              Bounds     c[t] <= n_reads 2^20 < 2^51, so a_j < 2^63; the t of a read are distinct and sum_t c[t] <= n_reads 2^20, so
 *                         S < 2^63; a'_j < 2^44, so a'_j 2^20 fits 64 bits; S' > 0 always (a read's own shares keep the counts of its
 *                         transcripts at ONE - 64 together or more; with sh > 0, S' > 2^43 - 64).  A transcript's count can reach 0
 *                         and then stays 0.  A read loses at most one unit of 2^-20 per candidate to the floors.
 *              stats[16] (nullable): [0] iterations run, [1] the last d_i, [2] lost units = (reads with candidates) 2^20 - sum count,
 *                         [3] reads without candidates, [4] single-candidate reads, [5] slots, [8..11] microseconds of upload, first
 *                         step, iterations, download.
 *              The candidates stay on the device over the iterations: rd_quant_workspace_bytes(slots, n_reads, n_tx) =
 *              12 (2 slots + 64) + 24 n_tx + 4096 bounds the workspace (reads are packed into rows of 64 slots that no read
 *              straddles: at most 2 slots + 64 packed slots of 12 bytes; 24 bytes per transcript).  RD_ERR_NOMEM naming the figure when
 *              it cannot be reserved: an EM is not cut into launches.  Synchronous; the context's stream.
 *   rd_quant_em_host  host, no GPU: the same rules (csrc/quant_rules.h) and the same packed form in plain loops */
#define RD_MAP_MAX_CAND 64
int rd_map_candidates(rd_ctx* ctx, const uint8_t* reads, const int64_t* read_off, int64_t n_reads, int min_anchors, int min_score, int max_gap,
                      int bandwidth, int64_t budget_bytes, int max_cand, int min_frac_q10, int max_3p, int32_t* status, int32_t* n_qual,
                      int32_t* n_cand, int32_t* cands, int64_t* stats);
int rd_quant_em(rd_ctx* ctx, const int64_t* cand_off, const int32_t* cand_t, const uint16_t* cand_w, int64_t n_reads, int64_t n_tx, int max_iter,
                uint64_t tol_q20, uint64_t* count_q20, uint32_t* share_q20, int64_t* stats);
int rd_quant_em_host(const int64_t* cand_off, const int32_t* cand_t, const uint16_t* cand_w, int64_t n_reads, int64_t n_tx, int max_iter,
                     uint64_t tol_q20, uint64_t* count_q20, uint32_t* share_q20, int64_t* stats);
int64_t rd_quant_workspace_bytes(int64_t slots, int64_t n_reads, int64_t n_tx);

/* ---- pileup: per-site base counts and an error profile (pileup.hip, csrc/pileup_rules.h) ---------------------
 * NO reference behaviour.  Pair p is a span refs[ref_off[p] .. ref_off[p+1]) of n characters whose first character is site site0[p] of a
 * table of n_sites sites, against a read of m characters, and the column ops of their alignment ('M' 'X' 'D' 'I' as rd_align_batch
 * writes them).  Bytes are taken as they are (no U -> T here); code(byte): A 0, C 1, G 2, T 3, anything else 4.
 *   The covered interval of a pair runs from its first M / X column to its last; a pair without one has status RD_PILEUP_NO_BASE and
 *   adds nothing.  Columns outside the interval add nothing: I columns there are soft clip, D columns shorten the covered range.
 *   Site channels (uint32 [8] per site): A C G T other (the read byte of an M / X column at this site), del (a D column), ins (a maximal
 *   run of I columns, at the site of the nearest ref-consuming column before it), starts (the interval's first column).  A channel
 *   grows by at most one per pair and site; at most 2^31 - 1 pairs are accepted between open and close (RD_ERR_ARG beyond).
 *   Profile (uint64 [RD_PILEUP_PROFILE_LEN], the covered interval only):
 *     [RD_PILEUP_CONF + 6 a + b]      span code a (0..4) x outcome b (read code 0..4 of an M / X column, 5 = a D column)
 *     [RD_PILEUP_INS_BASE + c]        inserted read bytes by code
 *     [RD_PILEUP_KMER + 4 k + e]      k: the 5-mer span[i-2 .. i+2], A = 0 .. T = 3, leftmost base most significant; e: 0 an M column at
 *                                     i, 1 an X column, 2 a D column, 3 an insertion run attributed to i.  Offsets within 2 of a span end
 *                                     and 5-mers with a non-ACGT byte count in conf only.
 *     [RD_PILEUP_INS_LEN + b], [RD_PILEUP_DEL_LEN + b]   maximal run lengths 1..63 in b = 0..62, 64 and longer in b = 63
 *   The column kind is the caller's (M against X), the channel comes from the read byte: rd_pileup_add_ops does not require them to agree.
 *   out [n_pairs][RD_PILEUP_RES] int32: status, alignment score (0 from rd_pileup_add_ops and rd_pileup_host), ref_lo, ref_hi (the covered
 *     span offsets, half-open), clip_head, clip_tail (read characters before / after the interval), n_match, n_sub, n_ins, n_del: the
 *     M, X, I and D columns INSIDE THE COVERED INTERVAL.  These are not rd_align_batch's counts, which follow analyse_alignment's clip
 *     (three non-gap ref characters, gap columns against a non-ACGT character dropped).  RD_PILEUP_NO_BASE: clip_head = m, the rest 0.
 *   rd_pileup_open      allocates and zeroes the tables of n_sites (0 .. 2^30) sites in the context; a second open starts again from zero
 *   rd_pileup_close     frees them
 *   rd_pileup_add       aligns exactly as rd_align_batch does (scores, tie-break, optional ops, budget) and accumulates.  Requires
 *                       site0[p] + n <= n_sites, and gap_open <= gap_extend as rd_align_batch does (RD_ERR_ARG, nothing added and
 *                       `out` not written: with open > extend the recurrence reopens adjacent gaps, so the score is not the
 *                       stated gap cost).  A pair that alone exceeds the budget is not aligned and adds nothing: status
 *                       RD_PILEUP_TOO_LARGE, and the call returns RD_ERR_NOMEM naming it after the others ran.  A pair takes
 *                       rd_pileup_workspace_bytes(n, m) = rd_align_workspace_bytes(n, m) + 48 + 256.
 *   rd_pileup_add_ops   the same accumulation from columns the caller has (ops + ops_off[p] .. ops_off[p+1]); no alignment runs.
 *                       RD_ERR_ARG before anything is added unless every op is M / X / D / I and the ops of a pair consume exactly its n
 *                       and m characters; n + m < 2^28.
 *   rd_pileup_read      the sites whose depth (channels A .. del summed) is >= min_depth >= 1, in site order: site [n_out] and counts
 *                       [8 n_out]; profile (nullable) is always written.  *n_out is the number of such sites; when capacity is smaller
 *                       the call returns RD_ERR_ARG with *n_out set and no site written.
 *   rd_pileup_host      host, no GPU, no context: the same rules in plain loops ADDED into the caller's sites [8 n_sites] and profile.
 * Integer adds only: the tables do not depend on launch order, budget or batching.  Synchronous; the context's stream. */
#define RD_PILEUP_OK 0
#define RD_PILEUP_NO_BASE 1
#define RD_PILEUP_TOO_LARGE 2
#define RD_PILEUP_RES 10
#define RD_PILEUP_CONF 0
#define RD_PILEUP_INS_BASE 30
#define RD_PILEUP_KMER 35
#define RD_PILEUP_INS_LEN 4131
#define RD_PILEUP_DEL_LEN 4195
#define RD_PILEUP_PROFILE_LEN 4259
int rd_pileup_open(rd_ctx* ctx, int64_t n_sites);
int rd_pileup_close(rd_ctx* ctx);
int rd_pileup_add(rd_ctx* ctx, const uint8_t* refs, const int64_t* ref_off, const uint8_t* reads, const int64_t* read_off, int n_pairs,
                  const int64_t* site0, int match, int mismatch, int gap_open, int gap_extend, int64_t budget_bytes, int32_t* out,
                  uint8_t* ops_out, const int64_t* ops_off, int32_t* ops_len);
int rd_pileup_add_ops(rd_ctx* ctx, const uint8_t* ops, const int64_t* ops_off, const uint8_t* refs, const int64_t* ref_off,
                      const uint8_t* reads, const int64_t* read_off, int n_pairs, const int64_t* site0, int32_t* out);
int rd_pileup_read(rd_ctx* ctx, uint32_t min_depth, int64_t capacity, uint32_t* site, uint32_t* counts, uint64_t* profile, int64_t* n_out);
int64_t rd_pileup_workspace_bytes(int64_t n, int64_t m);
int rd_pileup_host(const uint8_t* ops, const int64_t* ops_off, const uint8_t* refs, const int64_t* ref_off, const uint8_t* reads,
                   const int64_t* read_off, int n_pairs, const int64_t* site0, int64_t n_sites, uint32_t* sites, uint64_t* profile, int32_t* out);

/* The CTC loss of Keras's ctc_batch_cost and a greedy edit distance, per window, on the GPU (ctc.hip).
 * Window i has RD_CTC_T = 1024 softmax rows y[t][0..4] (A, C, G, T, blank), input_len[i] (1..1024) rows counted, and
 * label_len[i] (0..RD_CTC_MAX_LABEL) labels 0..3 at labels + label_off[i].
 *   loss[i]          -log of the summed probability of every path of input_len[i] rows that collapses to the labels, with
 *                    p[t][k] = (y[t][k] + 1e-7) / sum_j (y[t][j] + 1e-7) (Keras log(y + epsilon), then TF's log-softmax), in fp64;
 *                    +inf when no path exists
 *   status[i]        RD_CTC_OK, or RD_CTC_INFEASIBLE: label_len + (adjacent equal labels) > input_len, loss +inf
 *   greedy_len[i]    labels of the greedy decode: argmax of each counted row (lowest class on a tie), repeats collapsed, blanks dropped
 *   edit_distance[i] Levenshtein distance (unit costs) between the greedy labels and the window's labels
 *   greedy_out       nullable: window i's greedy labels at greedy_out + i * 1024
 * A label_len above RD_CTC_MAX_LABEL, an input_len outside 1..1024 or a label outside 0..3 is RD_ERR_ARG before anything is launched.
 * One launch per call, over the caller's windows; the context's workspaces are reused.  Synchronous; the context's stream.
 *   rd_ctc_eval           windows [n][1024] float32 (MAD-normalised) -> the forward (rd_forward, the loaded weights) -> the above
 *   rd_ctc_probs          caller-supplied rows probs [n][1024][5] float32 (host)
 *   rd_ctc_probs_resident the same with d_probs in device memory (rd_dev_alloc; e.g. rd_forward_resident's output) */
#define RD_CTC_T 1024
#define RD_CTC_MAX_LABEL 255
#define RD_CTC_OK 0
#define RD_CTC_INFEASIBLE 1
int rd_ctc_eval(rd_ctx* ctx, const float* windows, int n_windows, const int32_t* input_len, const uint8_t* labels, const int64_t* label_off,
                const int32_t* label_len, double* loss, int32_t* status, int32_t* greedy_len, int32_t* edit_distance, uint8_t* greedy_out);
int rd_ctc_probs(rd_ctx* ctx, const float* probs, int n_windows, const int32_t* input_len, const uint8_t* labels, const int64_t* label_off,
                 const int32_t* label_len, double* loss, int32_t* status, int32_t* greedy_len, int32_t* edit_distance, uint8_t* greedy_out);
int rd_ctc_probs_resident(rd_ctx* ctx, const float* d_probs, int n_windows, const int32_t* input_len, const uint8_t* labels,
                          const int64_t* label_off, const int32_t* label_len, double* loss, int32_t* status, int32_t* greedy_len,
                          int32_t* edit_distance, uint8_t* greedy_out);

/* Training of the signal model on labelled windows (train.hip): radian/train.py's model.fit with
 * Keras's ctc_batch_cost (the batch mean of the per-window losses above) and TF 2.4's Adam.  Exact fp32 only: a context set to
 * another precision is refused (RD_ERR_ARG).  The windows, input_len, labels and their checks are those of rd_ctc_eval
 * (all RD_ERR_ARG before anything is launched).  A window without a CTC path (RD_CTC_INFEASIBLE) contributes zero loss and
 * zero gradient; the mean still divides by n_windows (Keras would turn the whole step into inf / NaN).
 *   loss[i], status[i]   per window, from the weights before the update (loss +inf when infeasible)
 *   rd_train_grad        the gradient of the batch's mean loss, in load_weights order (rd_get_weights' layout); no update
 *   rd_train_step        the same gradient, then one Adam update of the context's weights, in place:
 *                          t += 1;  m += (g - m)(1 - beta1);  v += (g^2 - v)(1 - beta2);
 *                          w -= m alpha / (sqrt(v) + epsilon),  alpha = lr sqrt(1 - beta2^t) / (1 - beta1^t)   (fp32)
 *                        every later forward, rd_clone_artifacts and rd_rccl_bcast_model sees the new weights, in every packing
 *   rd_train_step_resident  d_windows [n][1024] in device memory (rd_dev_alloc)
 *   rd_train_reset       Adam's moments and t to zero (rd_load_weights does this too: Keras restores weights, not the optimiser)
 *   rd_get_weights       the context's current weights, n = the model's parameter count (2 200 581 for sig2seq.yaml)
 * Training workspaces (saved activations: about 19 x 1 KiB x 1024 per window) are allocated by the first training call and
 * only grow; a context that never trains allocates none.  Synchronous; the context's stream. */
typedef struct rd_adam {
    float lr;        /* 1e-4 in sig2seq.yaml */
    float beta1;     /* 0.9 */
    float beta2;     /* 0.999 */
    float epsilon;   /* 1e-7 */
} rd_adam;
int rd_train_grad(rd_ctx* ctx, const float* windows, int n_windows, const int32_t* input_len, const uint8_t* labels, const int64_t* label_off,
                  const int32_t* label_len, float* grad, double* loss, int32_t* status);
int rd_train_step(rd_ctx* ctx, const float* windows, int n_windows, const int32_t* input_len, const uint8_t* labels, const int64_t* label_off,
                  const int32_t* label_len, const rd_adam* opt, double* loss, int32_t* status);
int rd_train_step_resident(rd_ctx* ctx, const float* d_windows, int n_windows, const int32_t* input_len, const uint8_t* labels,
                           const int64_t* label_off, const int32_t* label_len, const rd_adam* opt, double* loss, int32_t* status);
int rd_train_reset(rd_ctx* ctx);
int rd_get_weights(rd_ctx* ctx, float* flat, size_t n);
/* The loaded model's parameter count (the size of rd_get_weights' and rd_train_grad's arrays). */
int rd_model_params(rd_ctx* ctx, int64_t* n);
/* The CTC part of rd_train_grad alone, on caller-supplied softmax rows probs [n][1024][5] float32 (host): grad_z [n][1024][5] is
 * dL/dz of the batch's mean loss with respect to the last Dense's output z (y = softmax(z)), through Keras's chain
 * dL/du = p - gamma (u = log(y + eps)), dL/dy = (p - gamma)/(y + eps), dL/dz_j = y_j (dL/dy_j - sum_k y_k dL/dy_k); zero on rows
 * t >= input_len and on infeasible windows.  Accumulated in fp64, written as fp32.  Any precision setting. */
int rd_train_ctc_grad(rd_ctx* ctx, const float* probs, int n_windows, const int32_t* input_len, const uint8_t* labels,
                      const int64_t* label_off, const int32_t* label_len, float* grad_z, double* loss, int32_t* status);

/* ---- multi-GPU start-up: one RCCL broadcast of weights + LM table over xGMI ------------------- */
/* librccl can be loaded in this process (dlopen + symbol lookup; creates nothing).  Ranks other than the one that draws the
 * unique id call this before the collective ncclCommInitRank, so that a rank without a usable librccl is known to everyone first. */
int rd_rccl_probe(void);
int rd_rccl_unique_id(uint8_t id_out[128]);                       /* rank 0, then shared out of band */
int rd_rccl_init(rd_ctx* ctx, int rank, int nranks, const uint8_t id[128]);
int rd_rccl_bcast_model(rd_ctx* ctx, int root);                   /* weights (+ LM when loaded on root) */
/* Hand the loaded artefacts of `src` (weights in every packing, LM table) to `dst`, another context of this process: what
 * rd_rccl_bcast_model does for another rank, with a device copy as the transport.  No reference counterpart. */
int rd_clone_artifacts(rd_ctx* dst, rd_ctx* src);
int rd_rccl_allreduce_max(rd_ctx* ctx, double* inout, int n);     /* host values, max over ranks */
int rd_rccl_barrier(rd_ctx* ctx);
/* Size of the communicator as RCCL itself reports it (ncclCommCount): the evidence that N ranks really joined. */
int rd_rccl_comm_count(rd_ctx* ctx, int* nranks);
int rd_rccl_finalize(rd_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* RADIAN_HIP_H */
