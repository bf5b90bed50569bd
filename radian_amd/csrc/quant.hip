// quant.hip -- transcript quantification: an expectation-maximisation over the candidate transcripts of every read, in fixed-point
// integer arithmetic (rd_quant_em on the GPU, rd_quant_em_host its twin in plain loops).  DESIGN.md section 22.
//
// Contract (include/radian_hip.h; the rules themselves and their bounds are quant_rules.h).  Read r has the candidates
// cand_t / cand_w [cand_off[r] .. cand_off[r+1]): 0..64 distinct transcripts with weights 1..4096.  ONE = 2^20.
//   step(c)   for every read with candidates: a_j = c[t_j] w_j, S = sum a_j, sh = max(0, bitlen(S) - 44), a'_j = a_j >> sh,
//             S' = sum a'_j, share_j = (a'_j << 20) / S'; c'[t] = the sum of the shares that name t
//   c0 = step(1, ..., 1); for i = 1 .. max_iter: c_i = step(c_{i-1}), d_i = max_t |c_i[t] - c_{i-1}[t]|, stop after i when d_i <= tol_q20
//   count = the last c, share = the shares of the last step executed
// A single-candidate read gives ONE to its transcript in every step (its share is (a' << 20) / a'), so those reads are summed once into
// base[t] and every step starts from a copy of base and runs over the multi-candidate reads only.
//
// Kernels, on the context's stream:
//   quant_fill_kernel    c = 1 for every transcript (the first step's input)
//   quant_step_kernel    one lane per packed slot (quant_pack: rows of 64 slots, no read straddles a row, so a read lives in one wave).
//                        Coalesced loads of t, w and the slot's segment bounds, a gather of c[t], an inclusive prefix sum of the terms over
//                        the wave by six shuffle steps (64-bit, modulo 2^64: the difference of two prefixes is exact since S < 2^63), the
//                        read's S as prefix[end] - prefix[head - 1], the shift, a second prefix sum for S', one unsigned 64-bit division,
//                        the share stored, and a 64-bit integer atomicAdd into c'[t] (vector atomics; integer adds commute, so the result
//                        does not depend on the order)
//   quant_delta_kernel   one thread per transcript: |c' - c|, a wave maximum by xor-shuffles, one 64-bit atomicMax per wave
// The host reads the 8 bytes of the maximum after every iteration.  No floating point, no inline assembly.
#include "common.h"
#include "quant_rules.h"
#include "../../include/radian_hip.h"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

namespace {

struct QuantIn {
    const int64_t* off;
    const int32_t* t;
    const uint16_t* w;
    int64_t n_reads, n_tx;
    int max_iter;
    uint64_t tol;
};

int quant_check_args(const char* who, const QuantIn& in, const uint64_t* count, const int64_t* stats)
{
    (void)stats;   // nullable
    RD_REQUIRE(in.n_reads >= 0 && in.n_reads < ((int64_t)1 << 31), "%s: n_reads = %lld (0 .. 2^31 - 1)", who, (long long)in.n_reads);
    RD_REQUIRE(in.n_tx >= 0 && in.n_tx < ((int64_t)1 << 24), "%s: n_tx = %lld (0 .. 2^24 - 1)", who, (long long)in.n_tx);
    RD_REQUIRE(in.max_iter >= 0 && in.max_iter <= QUANT_MAX_ITER, "%s: max_iter = %d (0 .. %d)", who, in.max_iter, QUANT_MAX_ITER);
    RD_REQUIRE(in.off != nullptr, "%s: null cand_off", who);
    RD_REQUIRE(count != nullptr || in.n_tx == 0, "%s: null count_q20", who);
    RD_REQUIRE(in.off[0] == 0, "%s: cand_off starts at %lld, not 0", who, (long long)in.off[0]);
    for (int64_t r = 0; r < in.n_reads; r++) {
        const int64_t n = in.off[r + 1] - in.off[r];
        RD_REQUIRE(n >= 0, "%s: cand_off decreases at read %lld", who, (long long)r);
        RD_REQUIRE(n <= QUANT_MAX_CAND, "%s: read %lld has %lld candidates (at most %d)", who, (long long)r, (long long)n, QUANT_MAX_CAND);
    }
    const int64_t slots = in.off[in.n_reads];
    RD_REQUIRE(slots == 0 || (in.t != nullptr && in.w != nullptr), "%s: null cand_t or cand_w", who);
    for (int64_t r = 0; r < in.n_reads; r++) {
        const int64_t s0 = in.off[r], s1 = in.off[r + 1];
        for (int64_t i = s0; i < s1; i++) {
            RD_REQUIRE(in.t[i] >= 0 && in.t[i] < in.n_tx, "%s: candidate %lld of read %lld names transcript %d of %lld", who, (long long)(i - s0),
                       (long long)r, in.t[i], (long long)in.n_tx);
            RD_REQUIRE(quant_weight_ok(in.w[i]), "%s: candidate %lld of read %lld has weight %d (1 .. %d)", who, (long long)(i - s0), (long long)r,
                       (int)in.w[i], QUANT_MAX_W);
            for (int64_t j = s0; j < i; j++)
                RD_REQUIRE(in.t[j] != in.t[i], "%s: read %lld names transcript %d twice: the candidates of a read are distinct", who, (long long)r,
                           in.t[i]);
        }
    }
    return RD_OK;
}

double quant_now_us()
{
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// one step over the packed reads on the host: cn = base + the shares; share (packed, nullable).  false: a read's S' came to 0
bool quant_host_step(const QuantPack& P, const uint64_t* c, uint64_t* cn, uint32_t* share)
{
    const size_t n = P.t.size();
    if (!P.base.empty()) memcpy(cn, P.base.data(), P.base.size() * 8);
    for (size_t i = 0; i < n;) {
        if (P.t[i] < 0) {
            i++;
            continue;
        }
        const size_t len = (size_t)(P.end[i] - P.head[i]) + 1;
        uint64_t S = 0, Sp = 0;
        for (size_t j = i; j < i + len; j++) S += quant_term(c[P.t[j]], P.w[j]);
        const int sh = quant_shift(S);
        for (size_t j = i; j < i + len; j++) Sp += quant_term(c[P.t[j]], P.w[j]) >> sh;
        if (Sp == 0) return false;
        for (size_t j = i; j < i + len; j++) {
            const uint64_t s = quant_share(quant_term(c[P.t[j]], P.w[j]) >> sh, Sp);
            if (share) share[j] = (uint32_t)s;
            cn[P.t[j]] += s;
        }
        i += len;
    }
    return true;
}

// the caller's outputs from the final counts and the packed shares of the last step
void quant_finish(const QuantIn& in, const QuantPack& P, const uint64_t* c, const uint32_t* share_packed, int iters, uint64_t last_d, uint64_t* count,
                  uint32_t* share, int64_t* stats)
{
    uint64_t total = 0;
    for (int64_t t = 0; t < in.n_tx; t++) {
        count[t] = c[t];
        total += c[t];
    }
    if (share) {
        for (int64_t r = 0; r < in.n_reads; r++)
            if (in.off[r + 1] - in.off[r] == 1) share[in.off[r]] = (uint32_t)QUANT_ONE;
        for (size_t i = 0; i < P.src.size(); i++)
            if (P.src[i] >= 0) share[P.src[i]] = share_packed[i];
    }
    if (stats) {
        for (int c16 = 0; c16 < 16; c16++) stats[c16] = 0;
        stats[0] = iters;
        stats[1] = (int64_t)last_d;
        stats[2] = (int64_t)((uint64_t)(in.n_reads - P.n_empty) * QUANT_ONE - total);
        stats[3] = P.n_empty;
        stats[4] = P.n_single;
        stats[5] = in.off[in.n_reads];
    }
}

int64_t quant_ws_bytes(int64_t n_packed, int64_t n_tx) { return 12 * n_packed + 24 * n_tx + 4096; }

}  // namespace

extern "C" int64_t rd_quant_workspace_bytes(int64_t slots, int64_t n_reads, int64_t n_tx)
{
    if (slots < 0 || n_reads < 0 || n_tx < 0) return -1;
    // a row and the first read of the next one together exceed 64 slots, so the packed rows hold fewer than 2 * slots + 64 slots
    return quant_ws_bytes(2 * slots + QUANT_ROW, n_tx);
}

extern "C" int rd_quant_em_host(const int64_t* cand_off, const int32_t* cand_t, const uint16_t* cand_w, int64_t n_reads, int64_t n_tx, int max_iter,
                                uint64_t tol_q20, uint64_t* count_q20, uint32_t* share_q20, int64_t* stats)
{
    const char* who = "rd_quant_em_host";
    const QuantIn in{cand_off, cand_t, cand_w, n_reads, n_tx, max_iter, tol_q20};
    if (int rc = quant_check_args(who, in, count_q20, stats)) return rc;
    QuantPack P;
    quant_pack(cand_off, cand_t, cand_w, n_reads, n_tx, &P);
    std::vector<uint64_t> a((size_t)n_tx, 1), b((size_t)n_tx, 0);
    std::vector<uint32_t> sp(share_q20 ? P.t.size() : 0);
    uint32_t* spp = share_q20 ? sp.data() : nullptr;
    uint64_t *c = a.data(), *cn = b.data();
    const auto fail = [&]() {
        rd_set_error("%s: internal: a read's shifted terms sum to 0", who);
        return RD_ERR_STATE;
    };
    if (!quant_host_step(P, c, cn, spp)) return fail();
    std::swap(c, cn);
    int iters = 0;
    uint64_t last_d = 0;
    while (iters < max_iter) {
        if (!quant_host_step(P, c, cn, spp)) return fail();
        uint64_t d = 0;
        for (int64_t t = 0; t < n_tx; t++) d = std::max(d, c[t] > cn[t] ? c[t] - cn[t] : cn[t] - c[t]);
        std::swap(c, cn);
        iters++;
        last_d = d;
        if (d <= tol_q20) break;
    }
    quant_finish(in, P, c, spp, iters, last_d, count_q20, share_q20, stats);
    return RD_OK;
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------------------------------ device half
namespace {

__global__ __launch_bounds__(256) void quant_fill_kernel(uint64_t* __restrict__ c, int64_t n, uint64_t v)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) c[i] = v;
}

// the sum of v over lanes head .. end of the wave, in every lane of that range (modulo 2^64)
__device__ __forceinline__ uint64_t quant_segment_sum(uint64_t v, int head, int end, int lane)
{
    uint64_t p = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t o = (uint64_t)__shfl_up((unsigned long long)p, d, 64);
        if (lane >= d) p += o;
    }
    const uint64_t pe = (uint64_t)__shfl((unsigned long long)p, end, 64);
    const uint64_t pb = (uint64_t)__shfl((unsigned long long)p, (head + 63) & 63, 64);   // lane head - 1
    return head ? pe - pb : pe;
}

// n_packed is a multiple of 64: a wave is inside the packed slots or outside them as a whole
__global__ __launch_bounds__(256) void quant_step_kernel(const int32_t* __restrict__ pt, const uint16_t* __restrict__ pw, const uint8_t* __restrict__ phead,
                                                         const uint8_t* __restrict__ pend, int64_t n_packed, const uint64_t* __restrict__ c,
                                                         unsigned long long* __restrict__ cn, uint32_t* __restrict__ share)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= n_packed) return;
    const int lane = threadIdx.x & 63;
    const int32_t t = pt[g];
    const uint64_t a = t >= 0 ? quant_term(c[t], pw[g]) : 0;
    const int head = phead[g], end = pend[g];
    const uint64_t S = quant_segment_sum(a, head, end, lane);
    const uint64_t as = a >> quant_shift(S);
    const uint64_t Sp = quant_segment_sum(as, head, end, lane);
    if (t < 0) return;
    const uint64_t s = quant_share(as, Sp);   // Sp > 0: quant_rules.h
    if (share) share[g] = (uint32_t)s;
    if (s) atomicAdd(&cn[t], (unsigned long long)s);
}

__global__ __launch_bounds__(256) void quant_delta_kernel(const uint64_t* __restrict__ c, const uint64_t* __restrict__ cn, int64_t n,
                                                          unsigned long long* __restrict__ dmax)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    uint64_t d = 0;
    if (i < n) {
        const uint64_t a = c[i], b = cn[i];
        d = a > b ? a - b : b - a;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint64_t v = (uint64_t)__shfl_xor((unsigned long long)d, o, 64);
        d = v > d ? v : d;
    }
    if ((threadIdx.x & 63) == 0 && d) atomicMax(dmax, (unsigned long long)d);
}

}  // namespace

extern "C" int rd_quant_em(rd_ctx* ctx, const int64_t* cand_off, const int32_t* cand_t, const uint16_t* cand_w, int64_t n_reads, int64_t n_tx,
                           int max_iter, uint64_t tol_q20, uint64_t* count_q20, uint32_t* share_q20, int64_t* stats)
{
    const char* who = "rd_quant_em";
    RD_REQUIRE(ctx != nullptr, "%s: null context", who);
    const QuantIn in{cand_off, cand_t, cand_w, n_reads, n_tx, max_iter, tol_q20};
    if (int rc = quant_check_args(who, in, count_q20, stats)) return rc;
    RD_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    double t0 = quant_now_us();
    QuantPack P;
    quant_pack(cand_off, cand_t, cand_w, n_reads, n_tx, &P);
    const int64_t np = (int64_t)P.t.size(), M = n_tx;
    const int64_t need = quant_ws_bytes(np, M);
    if (ctx->ws_quant.reserve((size_t)need)) {
        rd_set_error("%s: the workspace of %lld bytes (%lld packed slots of %lld candidates, %lld transcripts; rd_quant_workspace_bytes) could not be "
                     "reserved: an EM is not cut into launches", who, (long long)need, (long long)np, (long long)cand_off[n_reads], (long long)M);
        return RD_ERR_NOMEM;
    }
    // layout: dmax | base | c a | c b | share | t | w | head | end  (every part a multiple of 8 bytes up to the shares: np is a multiple of 64)
    char* p = (char*)ctx->ws_quant.p;
    unsigned long long* d_dmax = (unsigned long long*)p;
    uint64_t* d_base = (uint64_t*)(p + 256);
    uint64_t* d_c = d_base + M;
    uint64_t* d_cn = d_c + M;
    uint32_t* d_share = (uint32_t*)(d_cn + M);
    int32_t* d_t = (int32_t*)(d_share + np);
    uint16_t* d_w = (uint16_t*)(d_t + np);
    uint8_t* d_head = (uint8_t*)(d_w + np);
    uint8_t* d_end = d_head + np;
    if (np) {
        RD_HIP(hipMemcpyAsync(d_t, P.t.data(), (size_t)np * 4, hipMemcpyHostToDevice, st));
        RD_HIP(hipMemcpyAsync(d_w, P.w.data(), (size_t)np * 2, hipMemcpyHostToDevice, st));
        RD_HIP(hipMemcpyAsync(d_head, P.head.data(), (size_t)np, hipMemcpyHostToDevice, st));
        RD_HIP(hipMemcpyAsync(d_end, P.end.data(), (size_t)np, hipMemcpyHostToDevice, st));
    }
    if (M) RD_HIP(hipMemcpyAsync(d_base, P.base.data(), (size_t)M * 8, hipMemcpyHostToDevice, st));
    RD_HIP(hipStreamSynchronize(st));
    const double t_upload = quant_now_us() - t0;
    t0 = quant_now_us();
    const unsigned gm = (unsigned)((M + 255) / 256), gs = (unsigned)((np + 255) / 256);
    uint32_t* d_share_arg = share_q20 ? d_share : nullptr;
    // one step: cn = base, then the multi-candidate reads on top
    const auto step = [&]() -> int {
        if (M) RD_HIP(hipMemcpyAsync(d_cn, d_base, (size_t)M * 8, hipMemcpyDeviceToDevice, st));
        if (np) hipLaunchKernelGGL(quant_step_kernel, dim3(gs), dim3(256), 0, st, d_t, d_w, d_head, d_end, np, d_c, (unsigned long long*)d_cn, d_share_arg);
        RD_HIP(hipGetLastError());
        return RD_OK;
    };
    if (M) hipLaunchKernelGGL(quant_fill_kernel, dim3(gm), dim3(256), 0, st, d_c, M, (uint64_t)1);
    if (int rc = step()) return rc;
    std::swap(d_c, d_cn);
    RD_HIP(hipStreamSynchronize(st));
    const double t_init = quant_now_us() - t0;
    t0 = quant_now_us();
    int iters = 0;
    uint64_t last_d = 0;
    while (iters < max_iter) {
        RD_HIP(hipMemsetAsync(d_dmax, 0, 8, st));
        if (int rc = step()) return rc;
        if (M) hipLaunchKernelGGL(quant_delta_kernel, dim3(gm), dim3(256), 0, st, d_c, d_cn, M, d_dmax);
        RD_HIP(hipGetLastError());
        unsigned long long d = 0;
        RD_HIP(hipMemcpyAsync(&d, d_dmax, 8, hipMemcpyDeviceToHost, st));
        RD_HIP(hipStreamSynchronize(st));
        std::swap(d_c, d_cn);
        iters++;
        last_d = d;
        if (d <= tol_q20) break;
    }
    const double t_iter = quant_now_us() - t0;
    t0 = quant_now_us();
    std::vector<uint64_t> c((size_t)M);
    std::vector<uint32_t> sp(share_q20 ? (size_t)np : 0);
    if (M) RD_HIP(hipMemcpyAsync(c.data(), d_c, (size_t)M * 8, hipMemcpyDeviceToHost, st));
    if (!sp.empty()) RD_HIP(hipMemcpyAsync(sp.data(), d_share, (size_t)np * 4, hipMemcpyDeviceToHost, st));
    RD_HIP(hipStreamSynchronize(st));
    quant_finish(in, P, c.data(), sp.data(), iters, last_d, count_q20, share_q20, stats);
    if (stats) {
        stats[8] = (int64_t)t_upload;
        stats[9] = (int64_t)t_init;
        stats[10] = (int64_t)t_iter;
        stats[11] = (int64_t)(quant_now_us() - t0);
    }
    return RD_OK;
}
#endif  // __HIPCC__
