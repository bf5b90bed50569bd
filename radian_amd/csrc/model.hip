// model.hip -- the artefacts of a context: the packed weight images of the signal model (all three precisions) and the RNA
// model's device image (declared in include/radian_hip.h).
#include "common.h"
#include "model_params.h"
#include "../../include/radian_hip.h"

#include <cmath>
#include <math.h>
#include <string.h>

// --------------------------------------------------------------------------------------------- weights
namespace {

struct ModelLayout {
    size_t sink, w_in, b_in, w_match, b_match, w_conv[2 * RD_MAX_BLOCKS], b_conv[2 * RD_MAX_BLOCKS], w_d1, b_d1, w_d2, b_d2;
    size_t ws_conv[2 * RD_MAX_BLOCKS], ws_d1, w3_conv[2 * RD_MAX_BLOCKS], w3_d1, total;
};

ModelLayout model_layout(int nblocks)
{
    ModelLayout L = {};
    size_t off = 0;
    auto take = [&](size_t n) {
        size_t o = off;
        off += align_up(n, 64);
        return o;
    };
    L.sink = take(1024);
    L.w_in = take(RD_K * RD_C);
    L.b_in = take(RD_C);
    L.w_match = take(RD_C);
    L.b_match = take(RD_C);
    for (int b = 0; b < nblocks; b++)
        for (int w = 0; w < 2; w++) {
            if (b == 0 && w == 0) continue;
            L.w_conv[2 * b + w] = take(RD_CONV_N);
            L.b_conv[2 * b + w] = take(RD_C);
        }
    for (int b = 0; b < nblocks; b++)
        for (int w = 0; w < 2; w++) {
            if (b == 0 && w == 0) continue;
            L.ws_conv[2 * b + w] = take(RD_CONV_N);   // split-f16 image: same byte size as the fp32 one
        }
    L.ws_d1 = take(RD_D1_N);
    for (int b = 0; b < nblocks; b++)
        for (int w = 0; w < 2; w++) {
            if (b == 0 && w == 0) continue;
            L.w3_conv[2 * b + w] = take(RD_CONV_N * 3 / 2);   // three bf16 per weight = 6 B
        }
    L.w3_d1 = take(RD_D1_N * 3 / 2);
    L.w_d1 = take(RD_D1_N);
    L.b_d1 = take(RD_H);
    L.w_d2 = take(RD_H * RD_NCLS);
    L.b_d2 = take(RD_NCLS);
    L.total = off;
    return L;
}

void model_bind(Model& m, const ModelLayout& L)
{
    float* base = m.storage.as<float>();
    m.sink = base + L.sink;
    m.w_in = base + L.w_in;
    m.b_in = base + L.b_in;
    m.w_match = base + L.w_match;
    m.b_match = base + L.b_match;
    for (int b = 0; b < m.nblocks; b++)
        for (int w = 0; w < 2; w++) {
            if (b == 0 && w == 0) continue;
            m.w_conv[2 * b + w] = base + L.w_conv[2 * b + w];
            m.b_conv[2 * b + w] = base + L.b_conv[2 * b + w];
            m.ws_conv[2 * b + w] = base + L.ws_conv[2 * b + w];
            m.w3_conv[2 * b + w] = base + L.w3_conv[2 * b + w];
        }
    m.ws_d1 = base + L.ws_d1;
    m.w3_d1 = base + L.w3_d1;
    m.w_d1 = base + L.w_d1;
    m.b_d1 = base + L.b_d1;
    m.w_d2 = base + L.w_d2;
    m.b_d2 = base + L.b_d2;
}

// power-of-two scale that brings max|w| into [512, 1024): the lo halves of the split stay normal f16 numbers
float split_scale(const float* w, size_t n)
{
    float mx = 0.f;
    for (size_t i = 0; i < n; i++) mx = fabsf(w[i]) > mx ? fabsf(w[i]) : mx;
    if (!(mx > 0.f) || !std::isfinite(mx)) return 1.f;
    int e = 0;
    frexpf(mx, &e);              // mx = f * 2^e, f in [0.5, 1)
    return ldexpf(1.f, 10 - e);  // mx * scale in [512, 1024)
}

// one 64-B row of a 16-channel chunk: [16 hi | 16 lo] halves, 16-B slots (hi 0-7, hi 8-15, lo 0-7, lo 8-15) XOR (row >> 2) & 3
inline void split_store(_Float16* row, int k, int rowidx, float v)
{
    const _Float16 hi = (_Float16)v;
    const _Float16 lo = (_Float16)(v - (float)hi);
    const int sw = (rowidx >> 2) & 3;
    row[((k >> 3) ^ sw) * 8 + (k & 7)] = hi;
    row[((2 + (k >> 3)) ^ sw) * 8 + (k & 7)] = lo;
}

// fp32 -> bf16, round to nearest even (what v_cvt_pk_bf16_f32 does); finite inputs
inline uint16_t f2bf(float v)
{
    uint32_t u;
    memcpy(&u, &v, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
inline float bf2f(uint16_t h)
{
    const uint32_t u = (uint32_t)h << 16;
    float v;
    memcpy(&v, &u, 4);
    return v;
}
// one 96-B row of a 16-channel chunk: six 16-B slots (term * 2 + k / 8), physical slot = slot ^ ((row >> 3) & 1)
inline void bf3_store(uint16_t* row, int k, int rowidx, float v)
{
    uint16_t hi = f2bf(v);
    if ((hi & 0x7fffu) == 0x7f80u && std::isfinite(v)) {   // rounded up to infinity: truncate (as split3 on the device)
        uint32_t u;
        memcpy(&u, &v, 4);
        hi = (uint16_t)(u >> 16);
    }
    const float r1 = v - bf2f(hi);
    const uint16_t mid = f2bf(r1);
    const uint16_t lo = f2bf(r1 - bf2f(mid));
    const int sw = (rowidx >> 3) & 1, kh = k >> 3, kl = k & 7;
    row[((0 + kh) ^ sw) * 8 + kl] = hi;
    row[((2 + kh) ^ sw) * 8 + kl] = mid;
    row[((4 + kh) ^ sw) * 8 + kl] = lo;
}

// What a packed image stores for input channel k of row rowidx (= the output channel): its element type, the elements of a row, the store.
struct StoreF32 {   // fp32 image: 16 floats, slots swizzled
    typedef float T;
    static constexpr int ROW = 16;
    void put(float* row, int k, int rowidx, float v) const { row[rd_swz_f32(rowidx, k)] = v; }
};
struct StoreSplit {   // split-f16 image of the weights scaled by sc: [hi 16 | lo 16] halves
    typedef _Float16 T;
    static constexpr int ROW = 32;
    float sc;
    void put(_Float16* row, int k, int rowidx, float v) const { split_store(row, k, rowidx, v * sc); }
};
struct StoreBf3 {   // bf16x3 image: 6 slots x 8 bf16, unscaled
    typedef uint16_t T;
    static constexpr int ROW = 48;
    void put(uint16_t* row, int k, int rowidx, float v) const { bf3_store(row, k, rowidx, v); }
};

// Keras conv kernel [j][ci][co] -> [chunk = (ci/16)*3 + j][co][ci%16 as the store lays it out]
template <class S> void pack_conv(const float* k, void* dst, const S& st)
{
    for (int j = 0; j < RD_K; j++)
        for (int ci = 0; ci < RD_C; ci++) {
            const float* src = k + ((size_t)j * RD_C + ci) * RD_C;
            for (int co = 0; co < RD_C; co++) st.put((typename S::T*)dst + rd_conv_image_row(j, ci, co) * S::ROW, ci % 16, co, src[co]);
        }
}

// Keras dense kernel [ci][h] -> [chunk = ci/16][h][ci%16 as the store lays it out]
template <class S> void pack_dense(const float* k, void* dst, const S& st)
{
    for (int ci = 0; ci < RD_C; ci++) {
        const float* src = k + (size_t)ci * RD_H;
        for (int h = 0; h < RD_H; h++) st.put((typename S::T*)dst + rd_dense_image_row(ci, h) * S::ROW, ci % 16, h, src[h]);
    }
}

// every packed image of the flat weights w (load_weights order) into host (model_layout(nb).total floats); sets the split scales of m
void model_image(const float* w, int nb, const ModelLayout& L, Model& m, std::vector<float>& host)
{
    host.assign(L.total, 0.f);
    const ParamMap pm = param_map(nb);
    auto copy = [&](size_t dst, size_t src, size_t n) { memcpy(&host[dst], w + src, sizeof(float) * n); };
    auto conv = [&](int i, size_t kernel, size_t bias) {
        const StoreSplit split = {split_scale(w + kernel, RD_CONV_N)};
        pack_conv(w + kernel, &host[L.w_conv[i]], StoreF32());
        pack_conv(w + kernel, &host[L.ws_conv[i]], split);
        pack_conv(w + kernel, &host[L.w3_conv[i]], StoreBf3());
        m.inv_scale[i] = 1.f / split.sc;
        copy(L.b_conv[i], bias, RD_C);
    };
    copy(L.w_in, pm.w0[0], RD_K * RD_C);
    copy(L.b_in, pm.b0[0], RD_C);
    copy(L.w_match, pm.wm, RD_C);
    copy(L.b_match, pm.bm, RD_C);
    for (int b = 0; b < nb; b++) {
        if (b > 0) conv(2 * b, pm.w0[b], pm.b0[b]);
        conv(2 * b + 1, pm.w1[b], pm.b1[b]);
    }
    const StoreSplit split = {split_scale(w + pm.wd1, RD_D1_N)};
    pack_dense(w + pm.wd1, &host[L.w_d1], StoreF32());
    pack_dense(w + pm.wd1, &host[L.ws_d1], split);
    pack_dense(w + pm.wd1, &host[L.w3_d1], StoreBf3());
    m.inv_scale_d1 = 1.f / split.sc;
    copy(L.b_d1, pm.bd1, RD_H);
    copy(L.w_d2, pm.wd2, RD_H * RD_NCLS);
    copy(L.b_d2, pm.bd2, RD_NCLS);
}

// Model::pack_ok of the flat weights w: every weight of the conv kernels the packed heads run (blocks >= 1) is finite, none of their
// biases is -0.0.  Then leaving out a product with a zero-padding row gives results equal under IEEE comparison: fma(0, w, acc) == acc
// unless w is non-finite (NaN); an accumulator of -0.0 becomes +0.0, which compares equal -- the bias check keeps the common way to one out.
bool weights_allow_packing(const float* w, int nb)
{
    const ParamMap pm = param_map(nb);
    auto finite = [&](size_t at, size_t n) {
        for (size_t i = 0; i < n; i++)
            if (!std::isfinite(w[at + i])) return false;
        return true;
    };
    auto no_neg_zero = [&](size_t at, size_t n) {
        for (size_t i = 0; i < n; i++)
            if (w[at + i] == 0.f && std::signbit(w[at + i])) return false;
        return true;
    };
    for (int b = 1; b < nb; b++)
        if (!finite(pm.w0[b], RD_CONV_N) || !finite(pm.w1[b], RD_CONV_N) || !no_neg_zero(pm.b0[b], RD_C) || !no_neg_zero(pm.b1[b], RD_C)) return false;
    return true;
}

}  // namespace

size_t rd_model_image_floats(int nblocks) { return model_layout(nblocks).total; }
void rd_model_bind(Model& m) { model_bind(m, model_layout(m.nblocks)); }

extern "C" int rd_load_weights(rd_ctx* ctx, const void* blob, size_t nbytes)
{
    RD_REQUIRE(ctx && blob, "rd_load_weights: null argument");
    RD_REQUIRE(nbytes >= sizeof(rd_weights_header), "rd_load_weights: blob too small (%zu bytes)", nbytes);
    rd_weights_header h;
    memcpy(&h, blob, sizeof(h));
    RD_REQUIRE(h.magic == 0x574e4452u, "rd_load_weights: bad magic 0x%08x", h.magic);
    RD_REQUIRE(h.version == 1, "rd_load_weights: unsupported version %u", h.version);
    RD_REQUIRE(h.nb_filters == RD_C && h.kernel_size == RD_K && h.relu_units == RD_H && h.n_classes == RD_NCLS,
               "rd_load_weights: geometry (%u filters, k=%u, %u relu units, %u classes) is not sig2seq.yaml's (256,3,128,5)",
               h.nb_filters, h.kernel_size, h.relu_units, h.n_classes);
    RD_REQUIRE(h.n_blocks >= 1 && h.n_blocks <= RD_MAX_BLOCKS, "rd_load_weights: n_blocks %u out of range", h.n_blocks);
    const int nb = (int)h.n_blocks;
    const size_t expect = param_map(nb).total;
    RD_REQUIRE(h.n_floats == expect, "rd_load_weights: header says %u floats, geometry needs %zu", h.n_floats, expect);
    RD_REQUIRE(nbytes == sizeof(h) + expect * sizeof(float), "rd_load_weights: blob is %zu bytes, expected %zu", nbytes,
               sizeof(h) + expect * sizeof(float));
    for (int b = 0; b < nb; b++) RD_REQUIRE(h.dilations[b] >= 1 && h.dilations[b] <= 4096, "rd_load_weights: bad dilation");
    const float* w = (const float*)((const char*)blob + sizeof(h));

    RD_HIP(hipSetDevice(ctx->device));
    Model& m = ctx->model;
    m.loaded = false;
    m.nblocks = nb;
    for (int b = 0; b < nb; b++) m.dil[b] = (int)h.dilations[b];
    ModelLayout L = model_layout(nb);
    std::vector<float> host;
    model_image(w, nb, L, m, host);
    if (m.storage.reserve(L.total * sizeof(float))) return RD_ERR_NOMEM;
    RD_HIP(hipMemcpy(m.storage.p, host.data(), L.total * sizeof(float), hipMemcpyHostToDevice));
    model_bind(m, L);
    m.split_stale = false;
    m.pack_ok = weights_allow_packing(w, nb);
    rd_train_invalidate(ctx);   // Keras restores weights into a fresh optimiser
    m.loaded = true;
    return RD_OK;
}

// After training steps (train.hip) only the fp32 images are current: rebuild every image from the trained weights on the host,
// with rd_load_weights' packers, so that each packing equals a fresh load of the same weights.
int rd_model_refresh_split(rd_ctx* ctx)
{
    Model& m = ctx->model;
    if (!m.split_stale) return RD_OK;
    std::vector<float> flat;
    if (int rc = rd_train_weights_host(ctx, flat)) return rc;
    const ModelLayout L = model_layout(m.nblocks);
    std::vector<float> host;
    model_image(flat.data(), m.nblocks, L, m, host);
    if (int rc = rd_sync_lanes(ctx)) return rc;
    RD_HIP(hipMemcpy(m.storage.p, host.data(), L.total * sizeof(float), hipMemcpyHostToDevice));
    m.split_stale = false;
    m.pack_ok = weights_allow_packing(flat.data(), m.nblocks);
    return RD_OK;
}

int rd_model_halo(const rd_ctx* ctx)
{
    int s = 0;
    for (int b = 0; b < ctx->model.nblocks; b++) s += ctx->model.dil[b];
    return (RD_K - 1) * 2 * s;
}

// --------------------------------------------------------------------------------------------- LM
// doubles of the LM image: table [n][4], entropies [n], then one bit per context ("absent from a sparse model"), padded to doubles
size_t rd_lm_image_doubles(int table_order)
{
    const size_t n = (size_t)1 << (2 * table_order);
    return n * 5 + (n + 63) / 64;
}

void rd_lm_bind(LM& lm)
{
    const size_t n = (size_t)1 << (2 * lm.table_order);
    lm.table = lm.storage.as<double>();
    lm.d_entropy = lm.table + n * 4;
    lm.d_missing = (uint32_t*)(lm.table + n * 5);
}

// The table goes up as it is; what the search needs beside it -- per-context entropy (decode.py:73-76,85-90), and for a row of NaNs (a
// context that the sparse model does not hold: the reference's dict lookup raises KeyError when the search reaches it, decode.py:83) a
// zeroed row, a closed gate (entropy +inf) and its bit in the "absent" mask, which the beam search checks for every labeling that enters
// the beam -- is derived on the device by the pass a model built there goes through as well (rd_lm_finish_device, lmbuild.hip).
static int load_lm_table(rd_ctx* ctx, const double* table, int table_order, int context_len, int hashed)
{
    LM& lm = ctx->lm;
    lm.loaded = false;
    lm.gate_valid = false;
    if (!table) return RD_OK;
    RD_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)1 << (2 * table_order);
    if (lm.storage.reserve(rd_lm_image_doubles(table_order) * sizeof(double))) return RD_ERR_NOMEM;
    lm.table_order = table_order;
    rd_lm_bind(lm);
    RD_HIP(hipMemcpyAsync(lm.table, table, n * 4 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    return rd_lm_finish_device(ctx, table_order, context_len, hashed);
}

extern "C" int rd_load_lm(rd_ctx* ctx, const double* table, int k)
{
    RD_REQUIRE(ctx, "rd_load_lm: null context");
    if (!table) return load_lm_table(ctx, nullptr, 0, 0, 0);
    RD_REQUIRE(k >= 1 && k <= 13, "rd_load_lm: context length %d out of range [1,13] (longer contexts: rd_load_lm_hashed)", k);
    return load_lm_table(ctx, table, k, k, 0);
}

// An RNA model none of whose keys has k characters: `model[context]` (decode.py:83) raises KeyError for every context of k labels.  The
// image is an ordinary sparse one -- every row absent, every gate bit closed (entropy NaN compares false) -- filled on the device.
extern "C" int rd_load_lm_absent(rd_ctx* ctx, int k)
{
    RD_REQUIRE(ctx, "rd_load_lm_absent: null context");
    RD_REQUIRE(k >= 1 && k <= 13, "rd_load_lm_absent: context length %d out of range [1,13]", k);
    LM& lm = ctx->lm;
    lm.loaded = false;
    lm.gate_valid = false;
    RD_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)1 << (2 * k);
    lm.k = k;
    lm.table_order = k;
    lm.hashed = 0;
    lm.sparse = 1;
    if (lm.storage.reserve(rd_lm_image_doubles(k) * sizeof(double))) return RD_ERR_NOMEM;
    rd_lm_bind(lm);
    RD_HIP(hipMemset(lm.table, 0, n * 4 * sizeof(double)));
    RD_HIP(hipMemset(lm.d_entropy, 0xff, n * sizeof(double)));                  // NaN: `entropy < r_threshold` is false
    RD_HIP(hipMemset(lm.d_missing, 0xff, ((n + 63) / 64) * sizeof(double)));
    RD_HIP(hipDeviceSynchronize());
    lm.loaded = true;
    return RD_OK;
}

extern "C" int rd_load_lm_hashed(rd_ctx* ctx, const double* table, int table_order, int context_len)
{
    RD_REQUIRE(ctx && table, "rd_load_lm_hashed: null argument");
    RD_REQUIRE(table_order >= 1 && table_order <= 13, "rd_load_lm_hashed: table order %d out of range [1,13]", table_order);
    RD_REQUIRE(context_len >= 1 && context_len <= 256, "rd_load_lm_hashed: context length %d out of range [1,256]", context_len);
    return load_lm_table(ctx, table, table_order, context_len, 1);
}
