// rccl.hip -- the RCCL client (librccl by dlopen): communicator, the start-up broadcast of the artefacts, and their copy between
// two contexts of one process (declared in include/radian_hip.h).
#include "common.h"
#include "../../include/radian_hip.h"

#include <dlfcn.h>
#include <rccl/rccl.h>
#include <string.h>

namespace {

struct RcclApi {
    void* h = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;
    ncclResult_t (*Broadcast)(const void*, void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
};

RcclApi g_rccl;

int rccl_load()
{
    if (g_rccl.h) return RD_OK;
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    void* h = nullptr;
    for (const char* n : names) {
        h = dlopen(n, RTLD_NOW | RTLD_LOCAL);
        if (h) break;
    }
    if (!h) {
        rd_set_error("cannot dlopen librccl: %s", dlerror());
        return RD_ERR_RCCL;
    }
    g_rccl.h = h;
#define RD_SYM(field, name)                                                        \
    *(void**)(&g_rccl.field) = dlsym(h, name);                                     \
    if (!g_rccl.field) {                                                           \
        rd_set_error("librccl lacks symbol %s", name);                             \
        g_rccl.h = nullptr;                                                        \
        return RD_ERR_RCCL;                                                        \
    }
    RD_SYM(GetUniqueId, "ncclGetUniqueId");
    RD_SYM(CommInitRank, "ncclCommInitRank");
    RD_SYM(CommDestroy, "ncclCommDestroy");
    RD_SYM(CommCount, "ncclCommCount");
    RD_SYM(Broadcast, "ncclBroadcast");
    RD_SYM(AllReduce, "ncclAllReduce");
    RD_SYM(GetErrorString, "ncclGetErrorString");
#undef RD_SYM
    return RD_OK;
}

struct RcclState {
    ncclComm_t comm = nullptr;
    int rank = 0, nranks = 1;
    DevBuf scratch;
};

#define RD_NCCL(expr)                                                                              \
    do {                                                                                           \
        ncclResult_t _r = (expr);                                                                  \
        if (_r != ncclSuccess) {                                                                   \
            rd_set_error("%s:%d: %s failed: %s", __FILE__, __LINE__, #expr, g_rccl.GetErrorString(_r)); \
            return RD_ERR_RCCL;                                                                    \
        }                                                                                          \
    } while (0)

struct BcastHeader {
    int32_t model_loaded, nblocks, dil[RD_MAX_BLOCKS];
    int32_t lm_loaded, lm_k, lm_order, lm_hashed, lm_sparse;
    int64_t model_floats, lm_doubles;
    float inv_scale[2 * RD_MAX_BLOCKS], inv_scale_d1;
    int32_t pack_ok;   // Model::pack_ok of the sender: the images are its images
};

}  // namespace

extern "C" int rd_rccl_probe(void) { return rccl_load(); }

extern "C" int rd_rccl_unique_id(uint8_t id_out[128])
{
    RD_REQUIRE(id_out, "rd_rccl_unique_id: null argument");
    int rc = rccl_load();
    if (rc) return rc;
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
    ncclUniqueId id;
    RD_NCCL(g_rccl.GetUniqueId(&id));
    memcpy(id_out, &id, 128);
    return RD_OK;
}

extern "C" int rd_rccl_init(rd_ctx* ctx, int rank, int nranks, const uint8_t id[128])
{
    RD_REQUIRE(ctx && id, "rd_rccl_init: null argument");
    RD_REQUIRE(nranks >= 1 && rank >= 0 && rank < nranks, "rd_rccl_init: bad rank %d of %d", rank, nranks);
    int rc = rccl_load();
    if (rc) return rc;
    RD_HIP(hipSetDevice(ctx->device));
    if (ctx->rccl) rd_rccl_finalize(ctx);
    RcclState* st = new RcclState();
    st->rank = rank;
    st->nranks = nranks;
    ncclUniqueId uid;
    memcpy(&uid, id, 128);
    ncclResult_t r = g_rccl.CommInitRank(&st->comm, nranks, uid, rank);
    if (r != ncclSuccess) {
        rd_set_error("ncclCommInitRank(rank %d of %d) failed: %s", rank, nranks, g_rccl.GetErrorString(r));
        delete st;
        return RD_ERR_RCCL;
    }
    ctx->rccl = st;
    return RD_OK;
}

extern "C" int rd_rccl_finalize(rd_ctx* ctx)
{
    if (!ctx || !ctx->rccl) return RD_OK;
    RcclState* st = (RcclState*)ctx->rccl;
    if (st->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(st->comm);
    st->scratch.release();
    delete st;
    ctx->rccl = nullptr;
    return RD_OK;
}

// What a receiver must know before the device images arrive (the sender's side of rd_rccl_bcast_model / rd_clone_artifacts)
static void artifacts_header(const rd_ctx* ctx, BcastHeader& hd)
{
    hd = BcastHeader{};
    hd.model_loaded = 1;
    hd.nblocks = ctx->model.nblocks;
    for (int i = 0; i < RD_MAX_BLOCKS; i++) hd.dil[i] = ctx->model.dil[i];
    hd.model_floats = (int64_t)rd_model_image_floats(ctx->model.nblocks);
    for (int i = 0; i < 2 * RD_MAX_BLOCKS; i++) hd.inv_scale[i] = ctx->model.inv_scale[i];
    hd.inv_scale_d1 = ctx->model.inv_scale_d1;
    hd.pack_ok = ctx->model.pack_ok ? 1 : 0;
    hd.lm_loaded = ctx->lm.loaded ? 1 : 0;
    hd.lm_k = ctx->lm.k;
    hd.lm_order = ctx->lm.table_order;
    hd.lm_hashed = ctx->lm.hashed;
    hd.lm_sparse = ctx->lm.sparse;
    hd.lm_doubles = ctx->lm.loaded ? (int64_t)rd_lm_image_doubles(ctx->lm.table_order) : 0;
}

// The receiver's side: geometry and scales from the header, storage reserved and bound; the images are not there yet
// (artifacts_arrived marks them loaded).
static int artifacts_prepare(rd_ctx* ctx, const BcastHeader& hd)
{
    RD_REQUIRE(hd.model_loaded == 1 && hd.nblocks >= 1 && hd.nblocks <= RD_MAX_BLOCKS && hd.model_floats == (int64_t)rd_model_image_floats(hd.nblocks),
               "artefact header: %d blocks, %lld floats do not describe a model of this library", hd.nblocks, (long long)hd.model_floats);
    Model& m = ctx->model;
    m.loaded = false;
    m.nblocks = hd.nblocks;
    for (int i = 0; i < RD_MAX_BLOCKS; i++) m.dil[i] = hd.dil[i];
    for (int i = 0; i < 2 * RD_MAX_BLOCKS; i++) m.inv_scale[i] = hd.inv_scale[i];
    m.inv_scale_d1 = hd.inv_scale_d1;
    m.pack_ok = hd.pack_ok == 1;
    if (m.storage.reserve((size_t)hd.model_floats * 4)) return RD_ERR_NOMEM;
    rd_model_bind(m);
    ctx->lm.loaded = false;
    ctx->lm.gate_valid = false;
    if (hd.lm_loaded) {
        RD_REQUIRE(hd.lm_order >= 1 && hd.lm_order <= 13 && hd.lm_doubles == (int64_t)rd_lm_image_doubles(hd.lm_order),
                   "artefact header: LM table of order %d with %lld doubles", hd.lm_order, (long long)hd.lm_doubles);
        ctx->lm.k = hd.lm_k;
        ctx->lm.table_order = hd.lm_order;
        ctx->lm.hashed = hd.lm_hashed;
        ctx->lm.sparse = hd.lm_sparse;
        if (ctx->lm.storage.reserve((size_t)hd.lm_doubles * 8)) return RD_ERR_NOMEM;
        rd_lm_bind(ctx->lm);
    }
    return RD_OK;
}

static void artifacts_arrived(rd_ctx* ctx, const BcastHeader& hd)
{
    ctx->model.split_stale = false;
    rd_train_invalidate(ctx);
    ctx->model.loaded = true;
    if (hd.lm_loaded) ctx->lm.loaded = true;
}

extern "C" int rd_rccl_bcast_model(rd_ctx* ctx, int root)
{
    RD_REQUIRE(ctx && ctx->rccl, "rd_rccl_bcast_model: rd_rccl_init not called");
    RcclState* st = (RcclState*)ctx->rccl;
    RD_REQUIRE(root >= 0 && root < st->nranks, "rd_rccl_bcast_model: bad root");
    RD_HIP(hipSetDevice(ctx->device));
    BcastHeader hd = {};
    if (st->rank == root) {
        RD_REQUIRE(ctx->model.loaded, "rd_rccl_bcast_model: root has no weights loaded");
        if (int rc = rd_model_refresh_split(ctx)) return rc;
        artifacts_header(ctx, hd);
    }
    if (st->scratch.reserve(sizeof(BcastHeader))) return RD_ERR_NOMEM;
    RD_HIP(hipMemcpyAsync(st->scratch.p, &hd, sizeof(hd), hipMemcpyHostToDevice, ctx->stream));
    RD_NCCL(g_rccl.Broadcast(st->scratch.p, st->scratch.p, sizeof(hd), ncclUint8, root, st->comm, ctx->stream));
    RD_HIP(hipMemcpyAsync(&hd, st->scratch.p, sizeof(hd), hipMemcpyDeviceToHost, ctx->stream));
    RD_HIP(hipStreamSynchronize(ctx->stream));
    if (st->rank != root) {
        int rc = artifacts_prepare(ctx, hd);
        if (rc) return rc;
    }
    // one broadcast of the packed weights (8.8 MB) and, when present, one of the LM table + entropies
    RD_NCCL(g_rccl.Broadcast(ctx->model.storage.p, ctx->model.storage.p, (size_t)hd.model_floats, ncclFloat32, root, st->comm,
                             ctx->stream));
    if (hd.lm_loaded)
        RD_NCCL(g_rccl.Broadcast(ctx->lm.storage.p, ctx->lm.storage.p, (size_t)hd.lm_doubles, ncclFloat64, root, st->comm,
                                 ctx->stream));
    RD_HIP(hipStreamSynchronize(ctx->stream));
    artifacts_arrived(ctx, hd);
    return RD_OK;
}

// A second context of the same process takes the device images of a loaded one (weights in all three packings, LM table,
// entropies): the receiver's code of rd_rccl_bcast_model with a device-to-device copy as the transport.  The driver's
// extra contexts of a GPU use it instead of parsing and repacking the artefacts again; peer copies make it work across the
// GPUs of one process too.
extern "C" int rd_clone_artifacts(rd_ctx* dst, rd_ctx* src)
{
    RD_REQUIRE(dst && src && dst != src, "rd_clone_artifacts: two distinct contexts are needed");
    RD_REQUIRE(src->model.loaded, "rd_clone_artifacts: the source context has no weights loaded");
    BcastHeader hd;
    RD_HIP(hipSetDevice(src->device));
    if (int rc = rd_model_refresh_split(src)) return rc;
    artifacts_header(src, hd);
    RD_HIP(hipStreamSynchronize(src->stream));
    RD_HIP(hipSetDevice(dst->device));
    int rc = artifacts_prepare(dst, hd);
    if (rc) return rc;
    RD_HIP(hipMemcpyAsync(dst->model.storage.p, src->model.storage.p, (size_t)hd.model_floats * 4, hipMemcpyDefault, dst->stream));
    if (hd.lm_loaded)
        RD_HIP(hipMemcpyAsync(dst->lm.storage.p, src->lm.storage.p, (size_t)hd.lm_doubles * 8, hipMemcpyDefault, dst->stream));
    RD_HIP(hipStreamSynchronize(dst->stream));
    artifacts_arrived(dst, hd);
    return RD_OK;
}

extern "C" int rd_rccl_allreduce_max(rd_ctx* ctx, double* inout, int n)
{
    RD_REQUIRE(ctx && ctx->rccl && inout && n >= 1, "rd_rccl_allreduce_max: bad argument / rd_rccl_init not called");
    RcclState* st = (RcclState*)ctx->rccl;
    RD_HIP(hipSetDevice(ctx->device));
    if (st->scratch.reserve((size_t)n * 8 + 256)) return RD_ERR_NOMEM;
    RD_HIP(hipMemcpyAsync(st->scratch.p, inout, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
    RD_NCCL(g_rccl.AllReduce(st->scratch.p, st->scratch.p, (size_t)n, ncclFloat64, ncclMax, st->comm, ctx->stream));
    RD_HIP(hipMemcpyAsync(inout, st->scratch.p, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
    RD_HIP(hipStreamSynchronize(ctx->stream));
    return RD_OK;
}

extern "C" int rd_rccl_comm_count(rd_ctx* ctx, int* nranks)
{
    RD_REQUIRE(ctx && ctx->rccl && nranks, "rd_rccl_comm_count: bad argument / rd_rccl_init not called");
    RcclState* st = (RcclState*)ctx->rccl;
    int n = 0;
    RD_NCCL(g_rccl.CommCount(st->comm, &n));
    *nranks = n;
    return RD_OK;
}

extern "C" int rd_rccl_barrier(rd_ctx* ctx)
{
    double v = 0.0;
    return rd_rccl_allreduce_max(ctx, &v, 1);
}
