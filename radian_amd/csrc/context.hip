// context.hip -- the context of libradian_hip.so: error string, device workspaces, rd_create / rd_destroy, the rd_set_* switches,
// device-memory helpers and the kernel timers (declared in include/radian_hip.h and radian_hip_diag.h).
#include "common.h"
#include "budget.h"
#include "../../include/radian_hip.h"
#include "../../include/radian_hip_diag.h"

#include <algorithm>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

// --------------------------------------------------------------------------------------------- errors
static thread_local char g_err[1024] = "";

void rd_set_error(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* rd_last_error(void) { return g_err; }
extern "C" int rd_version(void) { return 1; }

int DevBuf::reserve(size_t bytes)
{
    if (bytes <= cap) return 0;
    // allocate, then swap: a failed growth leaves the old (smaller, still valid) buffer in place.  Only if the new block
    // does not fit BESIDE the old one is the old one given up first (workspaces carry no state between calls).
    size_t want = align_up(bytes + bytes / 8, 1 << 20);
    void* np = nullptr;
    hipError_t e = hipMalloc(&np, want);
    if (e != hipSuccess && p) {
        (void)hipGetLastError();
        (void)hipDeviceSynchronize();   // (see below)
        (void)hipFree(p);
        p = nullptr;
        cap = 0;
        e = hipMalloc(&np, want);
        if (e != hipSuccess) e = hipMalloc(&np, want = align_up(bytes, 1 << 20));
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        rd_set_error("hipMalloc(%zu bytes) failed: %s", want, hipGetErrorString(e));
        return -1;
    }
    if (p) {
        // A workspace can be regrown while kernels launched earlier on another stream still use the old block (the pipeline's shared
        // trie workspace while the previous group's search runs): wait for the device explicitly rather than lean on hipFree's own
        // synchronisation.  Growth is geometric (+ 1/8), so this happens a handful of times in a context's life.
        (void)hipDeviceSynchronize();
        (void)hipFree(p);
    }
    p = np;
    cap = want;
    return 0;
}

// A workspace that lives under a caller's budget: DevBuf::reserve would add headroom beyond it, so this one takes exactly what the largest
// launch needs.  It grows on a context's first budgeted call or for a larger batch only; the device is idle before the old block goes
// (release() itself does not wait, and the block is shared by entry points that run on different streams).
int DevBuf::reserve_exact(size_t bytes, const char* who)
{
    if (cap >= bytes) return 0;
    (void)hipDeviceSynchronize();
    release();
    const hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        p = nullptr;
        rd_set_error("%s: hipMalloc(%zu bytes) of the workspace failed: %s", who, bytes, hipGetErrorString(e));
        return -1;
    }
    cap = bytes;
    return 0;
}

int rd_resolve_budget(int64_t* budget_bytes, size_t held)
{
    if (*budget_bytes != 0) return RD_OK;
    size_t fr = 0, tot = 0;
    RD_HIP(hipMemGetInfo(&fr, &tot));
    *budget_bytes = rd_default_budget(fr, held);
    return RD_OK;
}

void DevBuf::release()
{
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
}

int rd_gather_h2d(hipStream_t st, void* dst, const void* src, size_t elem_bytes, const int64_t* src_off, const int32_t* members, int n,
                  const int64_t* off)
{
    hipError_t e = hipSuccess;
    rd_gather_runs(members, n, src_off, [&](int64_t i, int64_t k) {
        if (off[k] > off[i] && e == hipSuccess)
            e = hipMemcpyAsync((char*)dst + (size_t)off[i] * elem_bytes, (const char*)src + (size_t)src_off[members[i]] * elem_bytes,
                               (size_t)(off[k] - off[i]) * elem_bytes, hipMemcpyHostToDevice, st);
    });
    RD_HIP(e);
    return RD_OK;
}

extern "C" int rd_device_count(int* n)
{
    RD_REQUIRE(n != nullptr, "rd_device_count: null argument");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) {
        *n = 0;
        rd_set_error("hipGetDeviceCount failed: %s", hipGetErrorString(e));
        return RD_ERR_HIP;
    }
    *n = c;
    return RD_OK;
}


// --------------------------------------------------------------------------------------------- context
extern "C" int rd_create(int device_id, rd_ctx** out)
{
    RD_REQUIRE(out != nullptr, "rd_create: null out pointer");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        rd_set_error("rd_create: no HIP device available (%s); this backend has no CPU fallback",
                     e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
        return RD_ERR_HIP;
    }
    RD_REQUIRE(device_id >= 0 && device_id < n, "rd_create: device_id %d out of range [0,%d)", device_id, n);
    RD_HIP(hipSetDevice(device_id));
    hipDeviceProp_t prop;
    RD_HIP(hipGetDeviceProperties(&prop, device_id));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        rd_set_error("rd_create: device %d is %s; libradian_hip is built for gfx950 (MI355X) only", device_id, prop.gcnArchName);
        return RD_ERR_HIP;
    }
    rd_ctx* ctx = new rd_ctx();
    ctx->device = device_id;
    ctx->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if (e == hipSuccess) {
        int lo = 0, hi = 0;
        e = hipDeviceGetStreamPriorityRange(&lo, &hi);
        if (e == hipSuccess) e = hipStreamCreateWithPriority(&ctx->stream_hi, hipStreamNonBlocking, hi);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->ev_chain, hipEventDisableTiming);
    }
    if (e != hipSuccess) {
        rd_set_error("hipStreamCreate failed: %s", hipGetErrorString(e));
        if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
        if (ctx->stream_hi) (void)hipStreamDestroy(ctx->stream_hi);
        delete ctx;
        return RD_ERR_HIP;
    }
    *out = ctx;
    return RD_OK;
}

static void timer_free(KernelTimer& t)
{
    for (auto ev : t.starts) (void)hipEventDestroy(ev);
    for (auto ev : t.stops) (void)hipEventDestroy(ev);
    t.starts.clear();
    t.stops.clear();
    t.each_flops.clear();
    t.each_tag.clear();
    t.used = 0;
    t.enabled = false;
}

extern "C" int rd_destroy(rd_ctx* ctx)
{
    if (!ctx) return RD_OK;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    rd_rccl_finalize(ctx);
    rd_rpipe_destroy(ctx);
    rd_plan_cache_destroy_internal(ctx);
    rd_train_destroy(ctx);
    rd_map_destroy(ctx);
    timer_free(ctx->timer_conv);
    timer_free(ctx->timer_decode);
    timer_free(ctx->timer_head);
    timer_free(ctx->timer_in);
    for (int i = 0; i < 2 * RD_MAX_LANES; i++) {
        FwdLane& L = ctx->lanes[i];
        if (i > 0 && L.st) {
            (void)hipStreamSynchronize(L.st);
            if (i >= RD_MAX_LANES) rd_masked_stream_release(L.st);   // CU-masked streams are pooled, never destroyed (forward.hip)
            else (void)hipStreamDestroy(L.st);
        }
        if (L.done) (void)hipEventDestroy(L.done);
        for (DevBuf& b : L.act) b.release();
    }
    DevBuf* bufs[] = {&ctx->ws_tiles, &ctx->ws_raw, &ctx->ws_in, &ctx->ws_probs, &ctx->ws_mat, &ctx->ws_seq,
                      &ctx->ws_nodes_child, &ctx->ws_nodes_back, &ctx->ws_wide, &ctx->ws_wide_slot, &ctx->ws_align, &ctx->ws_ctc, &ctx->ws_calign, &ctx->ws_events, &ctx->ws_events_io, &ctx->ws_polya, &ctx->ws_polya_io, &ctx->ws_segment, &ctx->ws_eval, &ctx->ws_eval_model, &ctx->ws_site, &ctx->ws_quant, &ctx->pileup_sites, &ctx->pileup_profile, &ctx->ws_pileup, &ctx->ws_sim, &ctx->ws_queue, &ctx->ws_labels, &ctx->ws_misc, &ctx->model.storage,
                      &ctx->lm.storage, &ctx->lm.gate_storage};
    for (DevBuf* b : bufs) b->release();
    if (ctx->h_stage) (void)hipHostFree(ctx->h_stage);   // (ctx->stream was synchronised at the top)
    if (ctx->stream_hi) {
        (void)hipStreamSynchronize(ctx->stream_hi);
        (void)hipStreamDestroy(ctx->stream_hi);
    }
    if (ctx->ev_chain) (void)hipEventDestroy(ctx->ev_chain);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return RD_OK;
}

extern "C" int rd_set_precision(rd_ctx* ctx, int mode)
{
    RD_REQUIRE(ctx, "rd_set_precision: null context");
    RD_REQUIRE(mode >= 0 && mode <= 2, "rd_set_precision: mode %d (0 = fp32 MFMA, 1 = split-f16 f16x3, 2 = three-term bf16x3)", mode);
    ctx->precision = mode;
    return RD_OK;
}

extern "C" int rd_sync(rd_ctx* ctx)
{
    RD_REQUIRE(ctx, "rd_sync: null context");
    return rd_sync_lanes(ctx);
}

extern "C" int rd_set_logits(rd_ctx* ctx, int mode)
{
    RD_REQUIRE(ctx, "rd_set_logits: null context");
    RD_REQUIRE(mode == 0 || mode == 1, "rd_set_logits: mode %d (0 = float32 rows, 1 = float16 rows)", mode);
    ctx->logits_f16 = mode;
    return RD_OK;
}

extern "C" int rd_set_decode_form(rd_ctx* ctx, int form)
{
    RD_REQUIRE(ctx, "rd_set_decode_form: null context");
    RD_REQUIRE(form >= 0 && form <= 5, "rd_set_decode_form: form %d (0 = per launch, 1 = waves per sequence, 2 = candidates per lane, 3 = W <= 12: two sequences per "
               "wave, 4 = one, 5 = work queue)", form);
    ctx->decode_form = form;
    return RD_OK;
}

extern "C" int rd_set_trie_budget(rd_ctx* ctx, int64_t bytes)
{
    RD_REQUIRE(ctx, "rd_set_trie_budget: null context");
    RD_REQUIRE(bytes >= 0, "rd_set_trie_budget: negative budget");
    ctx->trie_budget = bytes ? bytes : (int64_t)24 << 30;
    return RD_OK;
}

extern "C" int rd_set_conv_shape(rd_ctx* ctx, int shape)
{
    RD_REQUIRE(ctx, "rd_set_conv_shape: null context");
    RD_REQUIRE(shape == 0 || shape == 1, "rd_set_conv_shape: shape %d (0 = 128-row tiles, two workgroups per CU; 1 = 256-row tiles, one workgroup per CU)", shape);
    ctx->conv_shape = shape;
    return RD_OK;
}

extern "C" int rd_set_conv_fuse(rd_ctx* ctx, int on)
{
    RD_REQUIRE(ctx, "rd_set_conv_fuse: null context");
    RD_REQUIRE(on == 0 || on == 1, "rd_set_conv_fuse: %d (1 = block 0's first conv inside its second, 0 = its own kernel)", on);
    ctx->conv_fuse = on;
    return RD_OK;
}

extern "C" int rd_set_head_pack(rd_ctx* ctx, int on)
{
    RD_REQUIRE(ctx, "rd_set_head_pack: null context");
    RD_REQUIRE(on == 0 || on == 1, "rd_set_head_pack: %d (1 = window heads as packed classes without their zero-padding taps, 0 = as head tiles)", on);
    ctx->head_pack = on;
    return RD_OK;
}

extern "C" int rd_head_pack_active(rd_ctx* ctx)
{
    if (!ctx) return 0;
    return rd_pack_heads(ctx) ? 1 : 0;
}

extern "C" int64_t rd_head_pack_tiles(rd_ctx* ctx) { return ctx ? ctx->packed_tiles : 0; }

extern "C" int rd_set_conv_slab(rd_ctx* ctx, int on)
{
    RD_REQUIRE(ctx, "rd_set_conv_slab: null context");
    RD_REQUIRE(on == 0 || on == 1, "rd_set_conv_slab: %d (1 = slab tiles stage their input rows once per channel slice, 0 = once per tap)", on);
    ctx->conv_slab = on;
    return RD_OK;
}

extern "C" int rd_conv_slab_active(rd_ctx* ctx)
{
    if (!ctx) return 0;
    return rd_conv_slab(ctx) ? 1 : 0;
}

extern "C" int64_t rd_conv_slab_tiles(rd_ctx* ctx) { return ctx ? ctx->slab_tiles : 0; }

extern "C" int rd_set_decode_partition(rd_ctx* ctx, int cus_per_xcd)
{
    RD_REQUIRE(ctx, "rd_set_decode_partition: null context");
    RD_REQUIRE(cus_per_xcd >= -1 && cus_per_xcd <= 16, "rd_set_decode_partition: %d CUs per XCD (-1 = by beam width, 0 = off, 1..16)", cus_per_xcd);
    RD_REQUIRE(rd_rpipe_idle(ctx), "rd_set_decode_partition: pipeline not empty (call rd_pipe_flush first)");
    ctx->part_mode = cus_per_xcd;
    return RD_OK;
}

extern "C" int rd_set_decode_math(rd_ctx* ctx, int mode)
{
    RD_REQUIRE(ctx, "rd_set_decode_math: null context");
    RD_REQUIRE(mode == 0 || mode == 1, "rd_set_decode_math: mode %d (0 = library routines, 1 = glibc's operation sequence)", mode);
    ctx->decode_math = mode;
    return RD_OK;
}

// --------------------------------------------------------------------------------------------- device memory
extern "C" int rd_dev_alloc(rd_ctx* ctx, size_t bytes, void** d_ptr)
{
    RD_REQUIRE(ctx && d_ptr, "rd_dev_alloc: null argument");
    RD_HIP(hipSetDevice(ctx->device));
    RD_HIP(hipMalloc(d_ptr, bytes ? bytes : 1));
    return RD_OK;
}
extern "C" int rd_mem_info(rd_ctx* ctx, size_t* free_bytes, size_t* total_bytes)
{
    RD_REQUIRE(ctx && free_bytes && total_bytes, "rd_mem_info: null argument");
    RD_HIP(hipSetDevice(ctx->device));
    RD_HIP(hipMemGetInfo(free_bytes, total_bytes));
    return RD_OK;
}
extern "C" int rd_dev_free(rd_ctx* ctx, void* d_ptr)
{
    RD_REQUIRE(ctx, "rd_dev_free: null context");
    if (d_ptr) RD_HIP(hipFree(d_ptr));
    return RD_OK;
}
extern "C" int rd_memcpy_h2d(rd_ctx* ctx, void* d_dst, const void* src, size_t bytes)
{
    RD_REQUIRE(ctx && d_dst && src, "rd_memcpy_h2d: null argument");
    RD_HIP(hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    RD_HIP(hipStreamSynchronize(ctx->stream));
    return RD_OK;
}
extern "C" int rd_memcpy_d2h(rd_ctx* ctx, void* dst, const void* d_src, size_t bytes)
{
    RD_REQUIRE(ctx && dst && d_src, "rd_memcpy_d2h: null argument");
    RD_HIP(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    RD_HIP(hipStreamSynchronize(ctx->stream));
    return RD_OK;
}

extern "C" int rd_split3(rd_ctx* ctx, const float* values, size_t n, uint16_t* terms_out)
{
    RD_REQUIRE(ctx && values && terms_out, "rd_split3: null argument");
    RD_HIP(hipSetDevice(ctx->device));
    if (n == 0) return RD_OK;
    if (ctx->ws_in.reserve(n * 4) || ctx->ws_misc.reserve(n * 6)) return RD_ERR_NOMEM;
    RD_HIP(hipMemcpyAsync(ctx->ws_in.p, values, n * 4, hipMemcpyHostToDevice, ctx->stream));
    int rc = rd_split3_dev(ctx, ctx->ws_in.as<float>(), n, ctx->ws_misc.as<uint16_t>());
    if (rc) return rc;
    RD_HIP(hipMemcpyAsync(terms_out, ctx->ws_misc.p, n * 6, hipMemcpyDeviceToHost, ctx->stream));
    RD_HIP(hipStreamSynchronize(ctx->stream));
    return RD_OK;
}

// --------------------------------------------------------------------------------------------- timers
static KernelTimer* timer_of(rd_ctx* ctx, int which)
{
    switch (which) {
        case RD_TIMER_CONV: return &ctx->timer_conv;
        case RD_TIMER_DECODE: return &ctx->timer_decode;
        case RD_TIMER_HEAD: return &ctx->timer_head;
        case RD_TIMER_IN: return &ctx->timer_in;
    }
    return nullptr;
}

extern "C" int rd_timer_enable(rd_ctx* ctx, int which, int max_launches)
{
    RD_REQUIRE(ctx, "rd_timer_enable: null context");
    KernelTimer* t = timer_of(ctx, which);
    RD_REQUIRE(t, "rd_timer_enable: unknown timer %d", which);
    RD_HIP(hipSetDevice(ctx->device));
    RD_HIP(hipStreamSynchronize(ctx->stream));
    timer_free(*t);
    t->flops = t->bytes = 0.0;
    if (max_launches <= 0) return RD_OK;
    t->starts.resize(max_launches);
    t->stops.resize(max_launches);
    for (int i = 0; i < max_launches; i++) {
        RD_HIP(hipEventCreate(&t->starts[i]));
        RD_HIP(hipEventCreate(&t->stops[i]));
    }
    t->enabled = true;
    return RD_OK;
}

extern "C" int rd_timer_read(rd_ctx* ctx, int which, double* total_ms, int* launches, double* flops, double* bytes)
{
    RD_REQUIRE(ctx, "rd_timer_read: null context");
    KernelTimer* t = timer_of(ctx, which);
    RD_REQUIRE(t, "rd_timer_read: unknown timer %d", which);
    RD_HIP(hipStreamSynchronize(ctx->stream));
    double ms = 0.0;
    for (size_t i = 0; i < t->used; i++) {
        float f = 0.f;
        RD_HIP(hipEventElapsedTime(&f, t->starts[i], t->stops[i]));
        ms += f;
    }
    if (total_ms) *total_ms = ms;
    if (launches) *launches = (int)t->used;
    if (flops) *flops = t->flops;
    if (bytes) *bytes = t->bytes;
    return RD_OK;
}

extern "C" int rd_timer_read_launches(rd_ctx* ctx, int which, int cap, float* ms_out, double* flops_out, int32_t* tag_out, int* n_out)
{
    RD_REQUIRE(ctx && n_out, "rd_timer_read_launches: null argument");
    KernelTimer* t = timer_of(ctx, which);
    RD_REQUIRE(t, "rd_timer_read_launches: unknown timer %d", which);
    RD_HIP(hipStreamSynchronize(ctx->stream));
    const size_t n = std::min(t->used, (size_t)std::max(0, cap));
    for (size_t i = 0; i < n; i++) {
        float f = 0.f;
        RD_HIP(hipEventElapsedTime(&f, t->starts[i], t->stops[i]));
        if (ms_out) ms_out[i] = f;
        if (flops_out) flops_out[i] = i < t->each_flops.size() ? t->each_flops[i] : 0.0;
        if (tag_out) tag_out[i] = i < t->each_tag.size() ? t->each_tag[i] : 0;
    }
    *n_out = (int)n;
    return RD_OK;
}
