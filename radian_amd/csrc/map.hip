// map.hip -- reads onto transcripts: (w,k)-minimizer seeds, a sorted seed index kept in the context, anchors by count / scan / fill,
// a radix sort by (read, transcript, r, q), one wave per (read, transcript) segment for the chain recurrence and a reduction per read
// (rd_map_index, rd_map_batch; rd_map_minimizers is the host twin of the seed definition), or the K best qualifying chains of every read
// in place of that reduction (rd_map_candidates).  The contract is in include/radian_hip.h, the shapes and figures
// in DESIGN.md section 15.  Everything is integer arithmetic: no output depends on how reads are packed.
#include "common.h"
#include "budget.h"
#include "../../include/radian_hip.h"
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <algorithm>
#include <chrono>
#include <cstring>

namespace {

constexpr uint32_t MZ_NONE = 0xFFFFFFFFu;   // "no k-mer here": hashes have at most 30 bits
constexpr int MZ_TILE = 1024;               // positions a workgroup of 256 threads decides
constexpr int MAP_MAX_W = 64;
constexpr int CP_PER = 2048;                // flags a workgroup of 256 threads compacts (8 per thread)
constexpr int64_t MAP_ANCHOR_BYTES = 64;    // workspace per anchor: two key and two q buffers (24), head flag (1), segment start (4) and
                                            // segment result (16) at one segment per anchor, block counts and the sort's temporary (< 19)
constexpr int64_t MAP_LAUNCH_BYTES = 1 << 20;   // alignment of the parts and the sort's histograms
constexpr int MAP_MAX_LAUNCH_READS = 65535;     // the read's index within a launch is the key's top 16 bits

// ---- the seed definition, host and device ------------------------------------------------------------------------------------
__host__ __device__ inline uint32_t map_hash(uint32_t x, int k)
{
    const uint32_t mask = (1u << (2 * k)) - 1u;
    x = (x * RD_MAP_HASH_C1) & mask;
    x ^= x >> k;
    x = (x * RD_MAP_HASH_C2) & mask;
    x ^= x >> k;
    return x;
}

// hash of the k-mer c[0..k), or MZ_NONE when one of its codes is not 0..3
__host__ __device__ inline uint32_t map_kmer_hash(const uint8_t* c, int k)
{
    uint32_t x = 0;
    for (int j = 0; j < k; j++) {
        if (c[j] > 3) return MZ_NONE;
        x = (x << 2) | c[j];
    }
    return map_hash(x, k);
}

// hs[0..w): the hashes of the k-mers at s, s+1, ...  Which of them the window that starts at s selects (offset from s), or -1 when no
// window starts at s.  k-mers of one segment are consecutive, so the run of existing k-mers from s is the window (w of them) or, at a
// segment's first k-mer, the whole of a segment shorter than w.
__host__ __device__ inline int map_pick(const uint32_t* hs, int w, bool segment_start)
{
    if (hs[0] == MZ_NONE) return -1;
    int best = 0, run = 1;
    uint32_t bh = hs[0];
    for (; run < w; run++) {
        const uint32_t h = hs[run];
        if (h == MZ_NONE) break;
        if (h < bh) {   // strict: of equal hashes the smallest position
            bh = h;
            best = run;
        }
    }
    return (run == w || segment_start) ? best : -1;
}

template <typename T>
__host__ __device__ inline int64_t lower_bound_dev(const T* a, int64_t n, T x)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
template <typename T>
__host__ __device__ inline int64_t upper_bound_dev(const T* a, int64_t n, T x)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// ---- minimizers of a flat buffer (records back to back, one break code after each) ------------------------------------------------
// A workgroup stages MZ_TILE positions plus the halo of w + k - 2 codes (and the code before the tile) in LDS, hashes every k-mer once,
// and each thread marks the choice of the windows that start in its positions.  Marks are byte stores of 1: the order does not matter.
__global__ __launch_bounds__(256) void mz_flag_kernel(const uint8_t* __restrict__ codes, int64_t N, int k, int w, uint8_t* __restrict__ flags)
{
    __shared__ uint8_t sc[1 + MZ_TILE + MAP_MAX_W + 16];
    __shared__ uint32_t sh[MZ_TILE + MAP_MAX_W];
    const int64_t t0 = (int64_t)blockIdx.x * MZ_TILE;
    const int nc = 1 + MZ_TILE + w + k - 2;   // sc[j] = the code at t0 - 1 + j
    for (int j = threadIdx.x; j < nc; j += 256) {
        const int64_t g = t0 - 1 + j;
        sc[j] = (g >= 0 && g < N) ? codes[g] : (uint8_t)255;
    }
    __syncthreads();
    const int nh = MZ_TILE + w - 1;           // sh[j] = the hash of the k-mer at t0 + j (reads sc[1 + j .. 1 + j + k), below nc)
    for (int j = threadIdx.x; j < nh; j += 256) sh[j] = map_kmer_hash(sc + 1 + j, k);
    __syncthreads();
    for (int s = threadIdx.x; s < MZ_TILE; s += 256) {
        if (t0 + s >= N) break;
        const int pick = map_pick(sh + s, w, sc[s] > 3);
        if (pick >= 0) flags[t0 + s + pick] = 1;   // a k-mer exists there, so the position is below N
    }
}

// ---- positions of the set flags, ascending: count per block, scan of the block counts, write ---------------------------------------
__global__ __launch_bounds__(256) void compact_count_kernel(const uint8_t* __restrict__ flags, int64_t N, uint32_t* __restrict__ block_cnt, uint32_t n_blocks)
{
    __shared__ uint32_t part[256];
    const int64_t base = (int64_t)blockIdx.x * CP_PER + (int64_t)threadIdx.x * 8;
    uint32_t c = 0;
    for (int j = 0; j < 8; j++)
        if (base + j < N) c += flags[base + j] != 0;
    part[threadIdx.x] = c;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        block_cnt[blockIdx.x] = part[0];
        if (blockIdx.x == 0) block_cnt[n_blocks] = 0;   // the scan's last output is the total
    }
}

__global__ __launch_bounds__(256) void compact_write_kernel(const uint8_t* __restrict__ flags, int64_t N, const uint32_t* __restrict__ block_off,
                                                            uint32_t* __restrict__ out)
{
    __shared__ uint32_t part[2][256];
    const int64_t base = (int64_t)blockIdx.x * CP_PER + (int64_t)threadIdx.x * 8;
    uint32_t c = 0;
    for (int j = 0; j < 8; j++)
        if (base + j < N) c += flags[base + j] != 0;
    int cur = 0;
    part[0][threadIdx.x] = c;
    __syncthreads();
    for (int s = 1; s < 256; s <<= 1) {   // inclusive scan over the threads
        uint32_t v = part[cur][threadIdx.x];
        if ((int)threadIdx.x >= s) v += part[cur][threadIdx.x - s];
        part[cur ^ 1][threadIdx.x] = v;
        cur ^= 1;
        __syncthreads();
    }
    uint32_t at = block_off[blockIdx.x] + part[cur][threadIdx.x] - c;
    for (int j = 0; j < 8; j++)
        if (base + j < N && flags[base + j]) out[at++] = (uint32_t)(base + j);
}

// ---- index entries: key = the minimizer's hash, value = transcript << 24 | position ----------------------------------------------------
__global__ void index_entries_kernel(const uint8_t* __restrict__ codes, const uint32_t* __restrict__ pos, int64_t n, const int64_t* __restrict__ flat_off,
                                     int64_t n_records, int k, uint32_t* __restrict__ keys, uint64_t* __restrict__ vals)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t g = pos[i];
    const int64_t t = upper_bound_dev(flat_off, n_records + 1, g) - 1;
    keys[i] = map_kmer_hash(codes + g, k);
    vals[i] = ((uint64_t)t << 24) | (uint64_t)(g - flat_off[t]);
}

// distinct keys and those with more than max_occ entries (two integer sums: the order of the additions does not matter)
__global__ void index_key_stats_kernel(const uint32_t* __restrict__ keys, int64_t n, int max_occ, unsigned long long* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || (i > 0 && keys[i] == keys[i - 1])) return;
    atomicAdd(&out[0], 1ull);
    if (upper_bound_dev(keys, n, keys[i]) - i > max_occ) atomicAdd(&out[1], 1ull);
}

// ---- lookup: count, (scan,) fill ----------------------------------------------------------------------------------------------------
struct MzHit {
    uint32_t lb;     // first index entry of the key
    uint32_t read;   // the read of the minimizer
    uint32_t q;      // its position in the read
    uint32_t pad;
};

__global__ void lookup_count_kernel(const uint8_t* __restrict__ codes, const uint32_t* __restrict__ pos, int64_t M, const int64_t* __restrict__ flat_off,
                                    int64_t n_reads, int k, const uint32_t* __restrict__ idx_keys, int64_t n_idx, int max_occ, MzHit* __restrict__ hit,
                                    uint64_t* __restrict__ cnt)
{
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m > M) return;
    if (m == M) {
        cnt[M] = 0;   // the scan's last output is the total
        return;
    }
    const int64_t g = pos[m];
    const int64_t r = upper_bound_dev(flat_off, n_reads + 1, g) - 1;
    const uint32_t key = map_kmer_hash(codes + g, k);
    const int64_t lb = lower_bound_dev(idx_keys, n_idx, key), ub = upper_bound_dev(idx_keys, n_idx, key);
    hit[m] = MzHit{(uint32_t)lb, (uint32_t)r, (uint32_t)(g - flat_off[r]), 0u};
    cnt[m] = (ub - lb > max_occ) ? 0 : (uint64_t)(ub - lb);
}

// per read (and one past the last): its first minimizer and the anchors before it
__global__ void read_ranges_kernel(const uint32_t* __restrict__ pos, int64_t M, const int64_t* __restrict__ flat_off, int64_t n_reads,
                                   const uint64_t* __restrict__ scan, int64_t* __restrict__ read_m, int64_t* __restrict__ read_a)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n_reads) return;
    const int64_t mb = lower_bound_dev(pos, M, (uint32_t)flat_off[r]);
    read_m[r] = mb;
    read_a[r] = (int64_t)scan[mb];
}

// anchors of minimizers [m0, m1): key = read in launch << 48 | transcript << 24 | r, value = q.  A read's minimizers are in ascending q and
// a key's entries in ascending (transcript, r), so the layout before the sort is fixed and a stable sort by the key orders equal
// (read, transcript, r) by q.
__global__ void anchor_fill_kernel(const MzHit* __restrict__ hit, const uint64_t* __restrict__ cnt, const uint64_t* __restrict__ scan, int64_t m0, int64_t m1,
                                   uint64_t a0, uint32_t r0, const uint64_t* __restrict__ idx_vals, uint64_t* __restrict__ keys, uint32_t* __restrict__ qs)
{
    const int64_t m = m0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= m1) return;
    const uint32_t c = (uint32_t)cnt[m];
    const MzHit h = hit[m];
    const uint64_t at = scan[m] - a0, top = (uint64_t)(h.read - r0) << 48;
    for (uint32_t j = 0; j < c; j++) {
        keys[at + j] = top | idx_vals[h.lb + j];
        qs[at + j] = h.q;
    }
}

__global__ void segment_flag_kernel(const uint64_t* __restrict__ keys, uint32_t A, uint8_t* __restrict__ flags)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A) return;
    flags[i] = (i == 0 || (keys[i] >> 24) != (keys[i - 1] >> 24)) ? 1 : 0;
}

// maximum over the wave, the same value in every lane: four DPP row shifts leave a row's maximum in its lane 15, two row broadcasts carry
// it on to lane 63 (bound_ctrl off: a lane without a source keeps its own value), one readlane hands it out
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_max(int v)
{
    return max(v, __builtin_amdgcn_update_dpp(v, v, CTRL, ROW_MASK, 0xf, false));
}
__device__ __forceinline__ int wave_max(int v)
{
    v = dpp_max<0x111, 0xf>(v);   // row_shr:1
    v = dpp_max<0x112, 0xf>(v);   // row_shr:2
    v = dpp_max<0x114, 0xf>(v);   // row_shr:4
    v = dpp_max<0x118, 0xf>(v);   // row_shr:8
    v = dpp_max<0x142, 0xa>(v);   // row_bcast:15 into rows 1 and 3
    v = dpp_max<0x143, 0xc>(v);   // row_bcast:31 into rows 2 and 3
    return __builtin_amdgcn_readlane(v, 63);
}

// ---- chains: one wave per (read, transcript) segment ---------------------------------------------------------------------------------
// Lane L holds anchor j with j % 64 == L of the last 64: its q, r, f, the chain's first anchor and its anchor count.  At anchor i every
// lane scores its anchor as predecessor, a wave maximum and a ballot pick the nearest of the best, and lane i % 64 takes the new anchor.
// Anchors are read 64 at a time, one per lane; the loop itself reads no memory.
__global__ __launch_bounds__(256) void map_chain_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ qs, const uint32_t* __restrict__ seg_start,
                                                        uint32_t n_seg, uint32_t A, int k, int min_anchors, int max_gap, int bandwidth, int4* __restrict__ seg_res)
{
    const uint32_t s = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= n_seg) return;
    const int lane = threadIdx.x & 63;
    const uint32_t a0 = seg_start[s], a1 = s + 1 < n_seg ? seg_start[s + 1] : A;
    const int len = (int)(a1 - a0);
    if (len < min_anchors) {   // no chain of min_anchors anchors fits
        if (lane == 0) seg_res[s] = make_int4(0, (int)a0, 0, (int)a0);
        return;
    }
    int qw = 0, rw = 0, fw = 0, firstw = 0, cntw = 0, qn = 0, rn = 0;
    int best_f = 0, best_i = 0, best_first = 0, best_cnt = 0;
    for (int i = 0; i < len; i++) {
        const int li = i & 63;
        if (li == 0 && i + lane < len) {
            rn = (int)(keys[a0 + i + lane] & 0xFFFFFFu);
            qn = (int)qs[a0 + i + lane];
        }
        const int qi = __builtin_amdgcn_readlane(qn, li), ri = __builtin_amdgcn_readlane(rn, li);
        const int d = (li - 1 - lane) & 63;   // this lane's anchor is j = i - 1 - d
        int cand = -1;
        if (i - 1 - d >= 0) {
            const int dq = qi - qw, dr = ri - rw;
            if (dq > 0 && dr > 0 && dq <= max_gap && dr <= max_gap) {
                const int dd = dr > dq ? dr - dq : dq - dr;
                if (dd <= bandwidth) {
                    const int gap = dd ? ((dd * k) >> 6) + ((31 - __clz(dd)) >> 1) : 0;
                    cand = fw + min(min(dq, dr), k) - gap;
                }
            }
        }
        const int m = wave_max(cand);
        int fi = k, firsti = i, cnti = 1;
        if (m > k) {
            const uint64_t mask = __ballot(cand == m);
            const int p = (li - 1) & 63, sh = 63 - p;                              // lane p is the nearest anchor; lane L goes to bit 63 - d(L)
            const uint64_t rot = sh ? (mask << sh) | (mask >> (64 - sh)) : mask;
            const int win = (p - __clzll((long long)rot)) & 63;
            fi = m;
            firsti = __builtin_amdgcn_readlane(firstw, win);
            cnti = __builtin_amdgcn_readlane(cntw, win) + 1;
        }
        if (lane == li) {
            qw = qi;
            rw = ri;
            fw = fi;
            firstw = firsti;
            cntw = cnti;
        }
        if (fi > best_f) {   // strict: the smallest i of the largest f
            best_f = fi;
            best_i = i;
            best_first = firsti;
            best_cnt = cnti;
        }
    }
    if (lane == 0) seg_res[s] = make_int4(best_f, (int)a0 + best_first, best_cnt, (int)a0 + best_i);
}

// ---- best and second-best segment of every read of the launch --------------------------------------------------------------------------
__global__ void map_best_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ qs, const uint32_t* __restrict__ seg_start, uint32_t n_seg,
                                const int4* __restrict__ seg_res, int n_local, int min_anchors, int min_score, int32_t* __restrict__ out)
{
    const int rl = blockIdx.x * blockDim.x + threadIdx.x;
    if (rl >= n_local) return;
    int64_t lo = 0, hi = n_seg;   // first segment of a read >= rl
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int)(keys[seg_start[mid]] >> 48) < rl) lo = mid + 1;
        else hi = mid;
    }
    int32_t* o = out + (int64_t)rl * 9;
    for (int c = 0; c < 9; c++) o[c] = 0;
    int best = -1, best_score = 0, second = 0;
    int64_t s = lo;
    for (; s < n_seg && (int)(keys[seg_start[s]] >> 48) == rl; s++) {
        const int4 r = seg_res[s];
        if (r.z < min_anchors || r.x < min_score) continue;
        if (r.x > best_score) {   // strict: of equal scores the smallest transcript
            second = best_score;
            best_score = r.x;
            best = (int)s;
        } else if (r.x > second) {
            second = r.x;
        }
    }
    if (s == lo) {
        o[0] = RD_MAP_NO_SEED;
    } else if (best < 0) {
        o[0] = RD_MAP_NO_CHAIN;
    } else {
        const int4 r = seg_res[best];
        const uint64_t kf = keys[r.y], kl = keys[r.w];
        o[0] = RD_MAP_OK;
        o[1] = (int32_t)((kf >> 24) & 0xFFFFFFu);
        o[2] = r.x;
        o[3] = second;
        o[4] = r.z;
        o[5] = (int32_t)qs[r.y];
        o[6] = (int32_t)(kf & 0xFFFFFFu);
        o[7] = (int32_t)qs[r.w];
        o[8] = (int32_t)(kl & 0xFFFFFFu);
    }
}

// ---- the K best candidate segments of every read of the launch (rd_map_candidates) ---------------------------------------------------------
// One wave per read.  The read's segments [lo, hi) by two binary searches, lanes striding over them.  A segment passes with min_anchors
// anchors, a score of min_score and, when max_3p >= 0, d3 <= max_3p; pass 1 is the wave maximum of the passing scores, a candidate is a
// passing segment with score * 1024 >= best * min_frac_q10.  Pass 2: a candidate's row is its rank, the number of the read's candidates
// that come before it in (score descending, t ascending) -- segments are in ascending t, so of equal scores the smaller segment index --
// counted against 64 segments at a time, one per lane, handed round by readlane.  A candidate of rank < K writes its row: one writer per
// row, no atomics.  The host has zeroed the rows.  out: MAP_CAND_HEAD + 8 K ints per read: status, n_qual, n_cand, then the rows.
constexpr int MAP_CAND_HEAD = 3;

struct CandSeg {
    int score, t, n_anchors, q0, r0, q1, r1, d3;
    bool pass;
};

__device__ __forceinline__ CandSeg map_cand_eval(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ qs, const int4* __restrict__ seg_res,
                                                 int64_t s, int min_anchors, int min_score, int L, const int32_t* __restrict__ tlen, int max_3p)
{
    const int4 r = seg_res[s];
    const uint64_t kf = keys[r.y], kl = keys[r.w];
    CandSeg c;
    c.score = r.x;
    c.t = (int)((kf >> 24) & 0xFFFFFFu);
    c.n_anchors = r.z;
    c.q0 = (int)qs[r.y];
    c.r0 = (int)(kf & 0xFFFFFFu);
    c.q1 = (int)qs[r.w];
    c.r1 = (int)(kl & 0xFFFFFFu);
    c.d3 = (tlen[c.t] - c.r1) - (L - c.q1);
    c.pass = r.z >= min_anchors && r.x >= min_score && (max_3p < 0 || c.d3 <= max_3p);
    return c;
}

__global__ __launch_bounds__(256) void map_cand_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ qs, const uint32_t* __restrict__ seg_start,
                                                       uint32_t n_seg, const int4* __restrict__ seg_res, int n_local, int min_anchors, int min_score,
                                                       const int64_t* __restrict__ read_flat_off, const int32_t* __restrict__ tlen, int K, int min_frac_q10,
                                                       int max_3p, int32_t* __restrict__ out)
{
    const int rl = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (rl >= n_local) return;
    const int lane = threadIdx.x & 63;
    int64_t lo = 0, hi = n_seg;   // first segment of a read >= rl
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int)(keys[seg_start[mid]] >> 48) < rl) lo = mid + 1;
        else hi = mid;
    }
    int64_t end = lo;
    hi = n_seg;                   // first segment of a read > rl
    while (end < hi) {
        const int64_t mid = (end + hi) >> 1;
        if ((int)(keys[seg_start[mid]] >> 48) <= rl) end = mid + 1;
        else hi = mid;
    }
    const int64_t n = end - lo;
    const int L = (int)(read_flat_off[rl + 1] - read_flat_off[rl] - 1);   // (the flat image has one break after every read)
    int32_t* o = out + (int64_t)rl * (MAP_CAND_HEAD + 8 * K);
    // pass 1: the best passing score (scores are >= min_score >= 0)
    int best = -1;
    for (int64_t i = lane; i < n; i += 64) {
        const CandSeg c = map_cand_eval(keys, qs, seg_res, lo + i, min_anchors, min_score, L, tlen, max_3p);
        if (c.pass) best = max(best, c.score);
    }
    best = wave_max(best);
    if (best < 0) {
        if (lane == 0) {
            o[0] = n == 0 ? RD_MAP_NO_SEED : RD_MAP_NO_CHAIN;
            o[1] = o[2] = 0;
        }
        return;
    }
    const int64_t need = (int64_t)best * min_frac_q10;
    // pass 2
    int n_qual = 0;
    for (int64_t b = 0; b < n; b += 64) {
        const int64_t i = b + lane;
        CandSeg mine;
        mine.pass = false;
        mine.score = -1;
        if (i < n) mine = map_cand_eval(keys, qs, seg_res, lo + i, min_anchors, min_score, L, tlen, max_3p);
        const bool cand = mine.pass && (int64_t)mine.score * 1024 >= need;
        n_qual += __popcll(__ballot(cand));
        int rank = 0;
        for (int64_t b2 = 0; b2 < n; b2 += 64) {
            const int64_t j = b2 + lane;
            int other = -1;   // the score of segment j when it is a candidate
            if (b2 == b) {
                other = cand ? mine.score : -1;
            } else if (j < n) {
                const CandSeg c = map_cand_eval(keys, qs, seg_res, lo + j, min_anchors, min_score, L, tlen, max_3p);
                if (c.pass && (int64_t)c.score * 1024 >= need) other = c.score;
            }
            for (int l = 0; l < 64; l++) {
                const int sj = __builtin_amdgcn_readlane(other, l);
                if (sj > mine.score || (sj == mine.score && b2 + l < i)) rank++;
            }
        }
        if (cand && rank < K) {
            int32_t* row = o + MAP_CAND_HEAD + 8 * rank;
            row[0] = mine.t;
            row[1] = mine.score;
            row[2] = mine.n_anchors;
            row[3] = mine.q0;
            row[4] = mine.r0;
            row[5] = mine.q1;
            row[6] = mine.r1;
            row[7] = mine.d3;
        }
    }
    if (lane == 0) {
        o[0] = RD_MAP_OK;
        o[1] = n_qual;
        o[2] = min(n_qual, K);
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
struct MapState {
    int k = 0, w = 0, max_occ = 0;
    int64_t n_idx = 0, n_records = 0;
    DevBuf keys, vals;                                           // the index: uint32 keys ascending, uint64 values in (transcript, position) order
    DevBuf tlen;                                                 // int32 per transcript: its length in codes (rd_map_candidates' 3' distance)
    DevBuf codes, off, flags, bcnt, boff, pos, tmp, hit, cnt, scan, rm, ra, out;   // per call
};

double now_us()
{
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

#define RD_RESERVE(buf, bytes)                                     \
    do {                                                           \
        if ((buf).reserve((size_t)(bytes)) != 0) return RD_ERR_NOMEM; \
    } while (0)

// records back to back with one break after each: host image and the records' starts in it
void flatten(const uint8_t* codes, const int64_t* off, int64_t n, std::vector<uint8_t>& flat, std::vector<int64_t>& flat_off)
{
    flat.resize((size_t)(off[n] + n));
    flat_off.resize((size_t)n + 1);
    for (int64_t r = 0; r < n; r++) {
        flat_off[r] = off[r] + r;
        if (off[r + 1] > off[r]) memcpy(flat.data() + flat_off[r], codes + off[r], (size_t)(off[r + 1] - off[r]));
        flat[(size_t)(off[r + 1] + r)] = 255;
    }
    flat_off[n] = off[n] + n;
}

// positions (ascending) of the set flags of d_flags[0..N) into d_out (capacity: every position); *count on the host
int compact(rd_ctx* ctx, MapState* st, const uint8_t* d_flags, int64_t N, uint32_t* d_out, DevBuf& bcnt, DevBuf& boff, int64_t* count)
{
    const uint32_t nb = (uint32_t)((N + CP_PER - 1) / CP_PER);
    RD_RESERVE(bcnt, (size_t)(nb + 1) * 4);
    RD_RESERVE(boff, (size_t)(nb + 1) * 4);
    hipLaunchKernelGGL(compact_count_kernel, dim3(nb), dim3(256), 0, ctx->stream, d_flags, N, bcnt.as<uint32_t>(), nb);
    size_t tb = 0;
    RD_HIP(rocprim::exclusive_scan(nullptr, tb, bcnt.as<uint32_t>(), boff.as<uint32_t>(), 0u, (size_t)nb + 1, rocprim::plus<uint32_t>(), ctx->stream));
    RD_RESERVE(st->tmp, std::max<size_t>(tb, 256));
    RD_HIP(rocprim::exclusive_scan(st->tmp.p, tb, bcnt.as<uint32_t>(), boff.as<uint32_t>(), 0u, (size_t)nb + 1, rocprim::plus<uint32_t>(), ctx->stream));
    hipLaunchKernelGGL(compact_write_kernel, dim3(nb), dim3(256), 0, ctx->stream, d_flags, N, boff.as<uint32_t>(), d_out);
    RD_HIP(hipGetLastError());
    uint32_t total = 0;
    RD_HIP(hipMemcpyAsync(&total, boff.as<uint32_t>() + nb, 4, hipMemcpyDeviceToHost, ctx->stream));
    RD_HIP(hipStreamSynchronize(ctx->stream));
    *count = total;
    return RD_OK;
}

// uploads the flat image and its offsets and leaves the minimizer positions in st->pos; *M of them
int minimizers_dev(rd_ctx* ctx, MapState* st, const std::vector<uint8_t>& flat, const std::vector<int64_t>& flat_off, int k, int w, int64_t* M)
{
    const int64_t N = (int64_t)flat.size();
    RD_RESERVE(st->codes, N);
    RD_RESERVE(st->off, flat_off.size() * 8);
    RD_RESERVE(st->flags, N);
    RD_RESERVE(st->pos, (size_t)N * 4);
    RD_HIP(hipMemcpyAsync(st->codes.p, flat.data(), (size_t)N, hipMemcpyHostToDevice, ctx->stream));
    RD_HIP(hipMemcpyAsync(st->off.p, flat_off.data(), flat_off.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    RD_HIP(hipMemsetAsync(st->flags.p, 0, (size_t)N, ctx->stream));
    hipLaunchKernelGGL(mz_flag_kernel, dim3((unsigned)((N + MZ_TILE - 1) / MZ_TILE)), dim3(256), 0, ctx->stream, st->codes.as<uint8_t>(), N, k, w,
                       st->flags.as<uint8_t>());
    RD_HIP(hipGetLastError());
    return compact(ctx, st, st->flags.as<uint8_t>(), N, st->pos.as<uint32_t>(), st->bcnt, st->boff, M);
}

int check_records(const char* who, const uint8_t* codes, const int64_t* off, int64_t n)
{
    RD_REQUIRE(off != nullptr && n >= 0, "%s: null offsets", who);
    RD_REQUIRE(off[0] == 0, "%s: offsets start at %lld, not 0", who, (long long)off[0]);
    for (int64_t r = 0; r < n; r++) RD_REQUIRE(off[r + 1] >= off[r], "%s: offsets decrease at record %lld", who, (long long)r);
    RD_REQUIRE(off[n] == 0 || codes != nullptr, "%s: null codes", who);
    RD_REQUIRE(off[n] + n < ((int64_t)1 << 31), "%s: %lld codes in %lld records: one call takes fewer than 2^31 together", who, (long long)off[n], (long long)n);
    return RD_OK;
}

// ---- the anchor workspace of one launch, and the part of a launch that follows the sort (rd_map_batch; rd_map_diag_chain) ---------------
// layout: keys a | keys b | q a | q b | segment starts | segment results | head flags | block counts | block offsets | the sort's temporary
struct LaunchWs {
    uint64_t *ka, *kb;
    uint32_t *qa, *qb, *seg_start;
    int4* seg_res;
    uint8_t* head;
    uint32_t nb, *bcnt, *boff;
    void* tmp;
    size_t sort_bytes, scan_bytes;
};

int carve_launch_ws(rd_ctx* ctx, const char* who, int64_t A, int end_bit, LaunchWs& W)
{
    Carve c(ctx->ws_align.p);
    W.ka = c.take<uint64_t>((size_t)A);
    W.kb = c.take<uint64_t>((size_t)A);
    W.qa = c.take<uint32_t>((size_t)A);
    W.qb = c.take<uint32_t>((size_t)A);
    W.seg_start = c.take<uint32_t>((size_t)A);
    W.seg_res = c.take<int4>((size_t)A);
    W.head = c.take<uint8_t>((size_t)A);
    W.nb = (uint32_t)((A + CP_PER - 1) / CP_PER);
    W.bcnt = c.take<uint32_t>((size_t)W.nb + 1);
    W.boff = c.take<uint32_t>((size_t)W.nb + 1);
    rocprim::double_buffer<uint64_t> dk(W.ka, W.kb);
    rocprim::double_buffer<uint32_t> dq(W.qa, W.qb);
    W.sort_bytes = W.scan_bytes = 0;
    RD_HIP(rocprim::radix_sort_pairs(nullptr, W.sort_bytes, dk, dq, (size_t)A, 0u, (unsigned)end_bit, ctx->stream));
    RD_HIP(rocprim::exclusive_scan(nullptr, W.scan_bytes, W.bcnt, W.boff, 0u, (size_t)W.nb + 1, rocprim::plus<uint32_t>(), ctx->stream));
    W.tmp = c.take<char>(std::max(W.sort_bytes, W.scan_bytes));
    return rd_carve_check(who, c, ctx->ws_align.cap);   // (A anchors: the size came from MAP_ANCHOR_BYTES and MAP_LAUNCH_BYTES)
}

// sorted anchors (keys, qs) -> segment starts and one chain result per segment in W; *n_seg on the host
int chain_launch(rd_ctx* ctx, const LaunchWs& W, const uint64_t* keys, const uint32_t* qs, int64_t A, int k, int min_anchors, int max_gap, int bandwidth,
                 uint32_t* n_seg)
{
    hipLaunchKernelGGL(segment_flag_kernel, dim3((unsigned)((A + 255) / 256)), dim3(256), 0, ctx->stream, keys, (uint32_t)A, W.head);
    hipLaunchKernelGGL(compact_count_kernel, dim3(W.nb), dim3(256), 0, ctx->stream, W.head, A, W.bcnt, W.nb);
    size_t scan_bytes = W.scan_bytes;
    RD_HIP(rocprim::exclusive_scan(W.tmp, scan_bytes, W.bcnt, W.boff, 0u, (size_t)W.nb + 1, rocprim::plus<uint32_t>(), ctx->stream));
    hipLaunchKernelGGL(compact_write_kernel, dim3(W.nb), dim3(256), 0, ctx->stream, W.head, A, W.boff, W.seg_start);
    RD_HIP(hipGetLastError());
    *n_seg = 0;
    RD_HIP(hipMemcpyAsync(n_seg, W.boff + W.nb, 4, hipMemcpyDeviceToHost, ctx->stream));
    RD_HIP(hipStreamSynchronize(ctx->stream));
    hipLaunchKernelGGL(map_chain_kernel, dim3((*n_seg + 3) / 4), dim3(256), 0, ctx->stream, keys, qs, W.seg_start, *n_seg, (uint32_t)A, k, min_anchors, max_gap,
                       bandwidth, W.seg_res);
    RD_HIP(hipGetLastError());
    return RD_OK;
}

}   // namespace

void rd_map_destroy(rd_ctx* ctx)
{
    MapState* st = (MapState*)ctx->map;
    if (!st) return;
    DevBuf* bufs[] = {&st->keys, &st->vals, &st->tlen, &st->codes, &st->off, &st->flags, &st->bcnt, &st->boff, &st->pos, &st->tmp, &st->hit, &st->cnt, &st->scan, &st->rm, &st->ra, &st->out};
    for (DevBuf* b : bufs) b->release();
    delete st;
    ctx->map = nullptr;
}

extern "C" int rd_map_minimizers(const uint8_t* codes, int64_t n, int k, int w, int32_t* pos, uint32_t* hash, int64_t cap, int64_t* n_out)
{
    RD_REQUIRE(n_out != nullptr && n >= 0 && (n == 0 || codes != nullptr), "rd_map_minimizers: null argument");
    RD_REQUIRE(k >= RD_MAP_MIN_K && k <= RD_MAP_MAX_K, "rd_map_minimizers: k = %d (%d..%d)", k, RD_MAP_MIN_K, RD_MAP_MAX_K);
    RD_REQUIRE(w >= 1 && w <= MAP_MAX_W, "rd_map_minimizers: w = %d (1..%d)", w, MAP_MAX_W);
    RD_REQUIRE(n < ((int64_t)1 << 31), "rd_map_minimizers: %lld codes (fewer than 2^31)", (long long)n);
    std::vector<uint32_t> hs((size_t)n + (size_t)w, MZ_NONE);
    for (int64_t i = 0; i + k <= n; i++) hs[(size_t)i] = map_kmer_hash(codes + i, k);
    std::vector<uint8_t> flag((size_t)n + 1, 0);
    for (int64_t s = 0; s < n; s++) {
        const int pick = map_pick(hs.data() + s, w, s == 0 || codes[s - 1] > 3);
        if (pick >= 0) flag[(size_t)(s + pick)] = 1;
    }
    int64_t c = 0;
    for (int64_t i = 0; i < n; i++)
        if (flag[(size_t)i]) {
            if (c < cap) {
                if (pos) pos[c] = (int32_t)i;
                if (hash) hash[c] = hs[(size_t)i];
            }
            c++;
        }
    *n_out = c;
    return RD_OK;
}

extern "C" int rd_map_index(rd_ctx* ctx, const uint8_t* codes, const int64_t* offsets, int64_t n_records, int k, int w, int max_occ, int64_t* stats)
{
    RD_REQUIRE(ctx != nullptr, "rd_map_index: null context");
    RD_REQUIRE(k >= RD_MAP_MIN_K && k <= RD_MAP_MAX_K, "rd_map_index: k = %d (%d..%d)", k, RD_MAP_MIN_K, RD_MAP_MAX_K);
    RD_REQUIRE(w >= 1 && w <= MAP_MAX_W, "rd_map_index: w = %d (1..%d)", w, MAP_MAX_W);
    RD_REQUIRE(max_occ >= 1, "rd_map_index: max_occ = %d (at least 1)", max_occ);
    if (int rc = check_records("rd_map_index", codes, offsets, n_records)) return rc;
    RD_REQUIRE(n_records >= 1 && n_records < (1 << 24), "rd_map_index: %lld transcripts (1 .. 2^24 - 1)", (long long)n_records);
    for (int64_t r = 0; r < n_records; r++)
        RD_REQUIRE(offsets[r + 1] - offsets[r] < (1 << 24), "rd_map_index: transcript %lld has %lld codes (fewer than 2^24)", (long long)r,
                   (long long)(offsets[r + 1] - offsets[r]));
    RD_HIP(hipSetDevice(ctx->device));
    if (!ctx->map) ctx->map = new MapState();
    MapState* st = (MapState*)ctx->map;
    st->n_idx = 0;
    st->k = 0;   // no index until this call has built one
    const double t0 = now_us();
    std::vector<uint8_t> flat;
    std::vector<int64_t> flat_off;
    flatten(codes, offsets, n_records, flat, flat_off);
    int64_t n = 0;
    if (int rc = minimizers_dev(ctx, st, flat, flat_off, k, w, &n)) return rc;
    const double t1 = now_us();
    unsigned long long key_stats[2] = {0, 0};
    if (n > 0) {
        // entries in position order, then a stable sort by the key: a key's entries stay in (transcript, position) order
        DevBuf k2, v2;
        RD_RESERVE(st->keys, (size_t)n * 4);
        RD_RESERVE(st->vals, (size_t)n * 8);
        int rc = RD_OK;
        if (k2.reserve((size_t)n * 4) != 0 || v2.reserve((size_t)n * 8) != 0) rc = RD_ERR_NOMEM;
        if (rc == RD_OK) {
            hipLaunchKernelGGL(index_entries_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, st->codes.as<uint8_t>(),
                               st->pos.as<uint32_t>(), n, st->off.as<int64_t>(), n_records, k, st->keys.as<uint32_t>(), st->vals.as<uint64_t>());
            rocprim::double_buffer<uint32_t> dk(st->keys.as<uint32_t>(), k2.as<uint32_t>());
            rocprim::double_buffer<uint64_t> dv(st->vals.as<uint64_t>(), v2.as<uint64_t>());
            size_t tb = 0;
            hipError_t e = rocprim::radix_sort_pairs(nullptr, tb, dk, dv, (size_t)n, 0u, (unsigned)(2 * k), ctx->stream);
            if (e == hipSuccess && st->tmp.reserve(std::max<size_t>(tb, 256)) != 0) rc = RD_ERR_NOMEM;
            if (e == hipSuccess && rc == RD_OK) e = rocprim::radix_sort_pairs(st->tmp.p, tb, dk, dv, (size_t)n, 0u, (unsigned)(2 * k), ctx->stream);
            if (e == hipSuccess && rc == RD_OK && dk.current() != st->keys.as<uint32_t>())
                e = hipMemcpyAsync(st->keys.p, dk.current(), (size_t)n * 4, hipMemcpyDeviceToDevice, ctx->stream);
            if (e == hipSuccess && rc == RD_OK && dv.current() != st->vals.as<uint64_t>())
                e = hipMemcpyAsync(st->vals.p, dv.current(), (size_t)n * 8, hipMemcpyDeviceToDevice, ctx->stream);
            if (e == hipSuccess && rc == RD_OK) {
                // (st->cnt is free between calls: two counters)
                if (st->cnt.reserve(16) != 0) rc = RD_ERR_NOMEM;
                else {
                    e = hipMemsetAsync(st->cnt.p, 0, 16, ctx->stream);
                    hipLaunchKernelGGL(index_key_stats_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, st->keys.as<uint32_t>(), n,
                                       max_occ, st->cnt.as<unsigned long long>());
                    if (e == hipSuccess) e = hipMemcpyAsync(key_stats, st->cnt.p, 16, hipMemcpyDeviceToHost, ctx->stream);
                }
            }
            if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
            else (void)hipStreamSynchronize(ctx->stream);
            if (e != hipSuccess && rc == RD_OK) {
                rd_set_error("rd_map_index: sorting the index failed: %s", hipGetErrorString(e));
                rc = RD_ERR_HIP;
            }
        }
        k2.release();
        v2.release();
        if (rc != RD_OK) return rc;
    }
    {
        std::vector<int32_t> tlen((size_t)n_records);
        for (int64_t r = 0; r < n_records; r++) tlen[(size_t)r] = (int32_t)(offsets[r + 1] - offsets[r]);
        RD_RESERVE(st->tlen, (size_t)n_records * 4);
        RD_HIP(hipMemcpyAsync(st->tlen.p, tlen.data(), (size_t)n_records * 4, hipMemcpyHostToDevice, ctx->stream));
        RD_HIP(hipStreamSynchronize(ctx->stream));
    }
    const double t2 = now_us();
    st->k = k;
    st->w = w;
    st->max_occ = max_occ;
    st->n_idx = n;
    st->n_records = n_records;
    if (stats) {
        stats[0] = n;
        stats[1] = (int64_t)key_stats[0];
        stats[2] = (int64_t)key_stats[1];
        stats[3] = (int64_t)(t1 - t0);
        stats[4] = (int64_t)(t2 - t1);
        stats[5] = stats[6] = stats[7] = 0;
    }
    return RD_OK;
}

// what rd_map_candidates asks of a call in place of rd_map_batch's hits
struct MapCand {
    int K, min_frac_q10, max_3p;
    int32_t *n_qual, *n_cand, *cands;
};

// rd_map_batch (cd == nullptr: hits) and rd_map_candidates (cd: hits unused): seeds, count + scan, the launches under the budget, fill, sort
// and chains are one code; the calls differ in the kernel that reduces a read's segments and in what it leaves per read
static int map_run(rd_ctx* ctx, const char* who, const uint8_t* reads, const int64_t* read_off, int64_t n_reads, int min_anchors, int min_score, int max_gap,
                   int bandwidth, int64_t budget_bytes, int32_t* status, int32_t* hits, const MapCand* cd, int64_t* stats)
{
    RD_REQUIRE(ctx != nullptr && status != nullptr && (cd ? cd->n_qual != nullptr && cd->n_cand != nullptr && cd->cands != nullptr : hits != nullptr),
               "%s: null argument", who);
    MapState* st = (MapState*)ctx->map;
    if (!st || st->k == 0) {
        rd_set_error("%s: no index in this context (rd_map_index first)", who);
        return RD_ERR_STATE;
    }
    RD_REQUIRE(min_anchors >= 1, "%s: min_anchors = %d (at least 1)", who, min_anchors);
    RD_REQUIRE(min_score >= 0, "%s: min_score = %d (at least 0)", who, min_score);
    RD_REQUIRE(max_gap >= 1 && max_gap < (1 << 24), "%s: max_gap = %d (1 .. 2^24 - 1)", who, max_gap);
    RD_REQUIRE(bandwidth >= 0 && bandwidth < (1 << 24), "%s: bandwidth = %d (0 .. 2^24 - 1)", who, bandwidth);
    RD_REQUIRE(budget_bytes >= 0, "%s: negative budget", who);
    if (cd) {
        RD_REQUIRE(cd->K >= 1 && cd->K <= RD_MAP_MAX_CAND, "%s: max_cand = %d (1 .. %d)", who, cd->K, RD_MAP_MAX_CAND);
        RD_REQUIRE(cd->min_frac_q10 >= 0 && cd->min_frac_q10 <= 1024, "%s: min_frac_q10 = %d (0 .. 1024)", who, cd->min_frac_q10);
        RD_REQUIRE(cd->max_3p >= -1, "%s: max_3p = %d (-1: off, or at least 0)", who, cd->max_3p);
    }
    if (int rc = check_records(who, reads, read_off, n_reads)) return rc;
    const int per_read = cd ? MAP_CAND_HEAD + 8 * cd->K : 9;   // ints a read has in st->out
    if (stats)
        for (int c = 0; c < 16; c++) stats[c] = 0;
    for (int64_t r = 0; r < n_reads; r++) {
        status[r] = RD_MAP_NO_SEED;
        if (cd) {
            cd->n_qual[r] = cd->n_cand[r] = 0;
            for (int c = 0; c < 8 * cd->K; c++) cd->cands[(int64_t)8 * cd->K * r + c] = 0;
        } else {
            for (int c = 0; c < 8; c++) hits[8 * r + c] = 0;
        }
    }
    if (n_reads == 0) return RD_OK;
    RD_HIP(hipSetDevice(ctx->device));
    if (int rc = rd_resolve_budget(&budget_bytes, ctx->ws_align.cap)) return rc;
    const int k = st->k;
    double t_stage[7] = {0, 0, 0, 0, 0, 0, 0};   // seeds, lookup, fill, sort, chain, best, candidates
    double t0 = now_us();
    std::vector<uint8_t> flat;
    std::vector<int64_t> flat_off;
    flatten(reads, read_off, n_reads, flat, flat_off);
    int64_t M = 0;
    if (int rc = minimizers_dev(ctx, st, flat, flat_off, k, st->w, &M)) return rc;
    t_stage[0] = now_us() - t0;
    if (M == 0 || st->n_idx == 0) return RD_OK;
    // count pass and scan over every minimizer of the call; per read its minimizers and the anchors before it
    t0 = now_us();
    RD_RESERVE(st->hit, (size_t)M * sizeof(MzHit));
    RD_RESERVE(st->cnt, (size_t)(M + 1) * 8);
    RD_RESERVE(st->scan, (size_t)(M + 1) * 8);
    RD_RESERVE(st->rm, (size_t)(n_reads + 1) * 8);
    RD_RESERVE(st->ra, (size_t)(n_reads + 1) * 8);
    RD_RESERVE(st->out, (size_t)n_reads * per_read * 4);
    hipLaunchKernelGGL(lookup_count_kernel, dim3((unsigned)((M + 1 + 255) / 256)), dim3(256), 0, ctx->stream, st->codes.as<uint8_t>(), st->pos.as<uint32_t>(), M,
                       st->off.as<int64_t>(), n_reads, k, st->keys.as<uint32_t>(), st->n_idx, st->max_occ, st->hit.as<MzHit>(), st->cnt.as<uint64_t>());
    RD_HIP(hipGetLastError());
    {
        size_t tb = 0;
        RD_HIP(rocprim::exclusive_scan(nullptr, tb, st->cnt.as<uint64_t>(), st->scan.as<uint64_t>(), (uint64_t)0, (size_t)M + 1, rocprim::plus<uint64_t>(), ctx->stream));
        RD_RESERVE(st->tmp, std::max<size_t>(tb, 256));
        RD_HIP(rocprim::exclusive_scan(st->tmp.p, tb, st->cnt.as<uint64_t>(), st->scan.as<uint64_t>(), (uint64_t)0, (size_t)M + 1, rocprim::plus<uint64_t>(), ctx->stream));
    }
    hipLaunchKernelGGL(read_ranges_kernel, dim3((unsigned)((n_reads + 1 + 255) / 256)), dim3(256), 0, ctx->stream, st->pos.as<uint32_t>(), M, st->off.as<int64_t>(),
                       n_reads, st->scan.as<uint64_t>(), st->rm.as<int64_t>(), st->ra.as<int64_t>());
    RD_HIP(hipGetLastError());
    std::vector<int64_t> read_m((size_t)n_reads + 1), read_a((size_t)n_reads + 1);
    RD_HIP(hipMemcpyAsync(read_m.data(), st->rm.p, read_m.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    RD_HIP(hipMemcpyAsync(read_a.data(), st->ra.p, read_a.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    RD_HIP(hipStreamSynchronize(ctx->stream));
    t_stage[1] = now_us() - t0;
    // launches: consecutive reads whose anchors fit the budget together.  A read over the budget closes the launch before it: a launch's
    // anchors are one range of the scan.  Reads without anchors take no part (RD_MAP_NO_SEED already) and lie inside the launch around them.
    const auto anchors = [&](int64_t r) { return read_a[r + 1] - read_a[r]; };
    const BudgetPlan plan = rd_plan_budget(n_reads, nullptr, budget_bytes, MAP_LAUNCH_BYTES, true,
                                           [&](int r, int) -> int64_t {
                                               const int64_t a = anchors(r);
                                               return a == 0 ? -1 : a >= ((int64_t)1 << 31) ? INT64_MAX : a * MAP_ANCHOR_BYTES;
                                           },
                                           [&](int r, int r0, int64_t, int64_t acc) {
                                               return r + 1 - r0 > MAP_MAX_LAUNCH_READS || acc / MAP_ANCHOR_BYTES + anchors(r) >= ((int64_t)1 << 31);
                                           });
    const int64_t too_large = plan.too_large, first_too_large = plan.first_too_large;
    for (int64_t r = 0; r < n_reads; r++)
        if (anchors(r)) status[r] = RD_MAP_TOO_LARGE;   // until its launch has run
    struct Launch {
        int64_t r0, r1;
    };
    std::vector<Launch> launches;
    for (auto [k0, k1] : plan.launches) launches.push_back({plan.run[k0], plan.run[k1 - 1] + 1});
    if (ctx->ws_align.reserve_exact((size_t)plan.max_bytes, who)) return RD_ERR_NOMEM;
    RD_HIP(hipMemsetAsync(st->out.p, 0, (size_t)n_reads * per_read * 4, ctx->stream));
    int64_t total_anchors = 0, total_segments = 0;
    for (const Launch& L : launches) {
        const int64_t m0 = read_m[L.r0], m1 = read_m[L.r1], a0 = read_a[L.r0], A = read_a[L.r1] - a0;
        const int n_local = (int)(L.r1 - L.r0);
        int end_bit = 48;
        while (end_bit < 64 && (n_local - 1) >> (end_bit - 48)) end_bit++;
        LaunchWs W;
        if (int rc = carve_launch_ws(ctx, who, A, end_bit, W)) return rc;
        rocprim::double_buffer<uint64_t> dk(W.ka, W.kb);
        rocprim::double_buffer<uint32_t> dq(W.qa, W.qb);
        t0 = now_us();
        hipLaunchKernelGGL(anchor_fill_kernel, dim3((unsigned)((m1 - m0 + 255) / 256)), dim3(256), 0, ctx->stream, st->hit.as<MzHit>(), st->cnt.as<uint64_t>(),
                           st->scan.as<uint64_t>(), m0, m1, (uint64_t)a0, (uint32_t)L.r0, st->vals.as<uint64_t>(), W.ka, W.qa);
        RD_HIP(hipGetLastError());
        if (stats) {
            RD_HIP(hipStreamSynchronize(ctx->stream));
            t_stage[2] += now_us() - t0;
            t0 = now_us();
        }
        RD_HIP(rocprim::radix_sort_pairs(W.tmp, W.sort_bytes, dk, dq, (size_t)A, 0u, (unsigned)end_bit, ctx->stream));
        const uint64_t* keys = dk.current();
        const uint32_t* qs = dq.current();
        if (stats) {
            RD_HIP(hipStreamSynchronize(ctx->stream));
            t_stage[3] += now_us() - t0;
            t0 = now_us();
        }
        uint32_t n_seg = 0;
        if (int rc = chain_launch(ctx, W, keys, qs, A, k, min_anchors, max_gap, bandwidth, &n_seg)) return rc;
        if (stats) {
            RD_HIP(hipStreamSynchronize(ctx->stream));
            t_stage[4] += now_us() - t0;
            t0 = now_us();
        }
        if (cd)
            hipLaunchKernelGGL(map_cand_kernel, dim3((unsigned)((n_local + 3) / 4)), dim3(256), 0, ctx->stream, keys, qs, W.seg_start, n_seg, W.seg_res, n_local,
                               min_anchors, min_score, st->off.as<int64_t>() + L.r0, st->tlen.as<int32_t>(), cd->K, cd->min_frac_q10, cd->max_3p,
                               st->out.as<int32_t>() + L.r0 * per_read);
        else
            hipLaunchKernelGGL(map_best_kernel, dim3((unsigned)((n_local + 255) / 256)), dim3(256), 0, ctx->stream, keys, qs, W.seg_start, n_seg, W.seg_res,
                               n_local, min_anchors, min_score, st->out.as<int32_t>() + L.r0 * 9);
        RD_HIP(hipGetLastError());
        RD_HIP(hipStreamSynchronize(ctx->stream));   // the next launch reuses the workspace
        if (stats) t_stage[cd ? 6 : 5] += now_us() - t0;
        total_anchors += A;
        total_segments += n_seg;
    }
    std::vector<int32_t> out((size_t)n_reads * per_read);
    RD_HIP(hipMemcpyAsync(out.data(), st->out.p, out.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    RD_HIP(hipStreamSynchronize(ctx->stream));
    for (const Launch& L : launches)
        for (int64_t r = L.r0; r < L.r1; r++) {
            const int32_t* o = out.data() + (size_t)r * per_read;
            status[r] = o[0];
            if (cd) {
                cd->n_qual[r] = o[1];
                cd->n_cand[r] = o[2];
                memcpy(cd->cands + (int64_t)8 * cd->K * r, o + MAP_CAND_HEAD, (size_t)8 * cd->K * 4);
            } else {
                for (int c = 0; c < 8; c++) hits[8 * r + c] = o[1 + c];
            }
        }
    if (stats) {
        stats[0] = (int64_t)launches.size();
        stats[1] = M;
        stats[2] = total_anchors;
        stats[3] = total_segments;
        for (int c = 0; c < 7; c++) stats[8 + c] = (int64_t)t_stage[c];
    }
    if (too_large) {
        const int64_t r = first_too_large;
        rd_set_error("%s: read %lld has %lld anchors and needs %lld bytes of workspace, over the budget of %lld; %lld read%s not mapped "
                     "(status RD_MAP_TOO_LARGE), the others were", who, (long long)r, (long long)(read_a[r + 1] - read_a[r]),
                     (long long)((read_a[r + 1] - read_a[r]) * MAP_ANCHOR_BYTES + MAP_LAUNCH_BYTES), (long long)budget_bytes, (long long)too_large,
                     too_large == 1 ? "" : "s");
        return RD_ERR_NOMEM;
    }
    return RD_OK;
}

extern "C" int rd_map_batch(rd_ctx* ctx, const uint8_t* reads, const int64_t* read_off, int64_t n_reads, int min_anchors, int min_score, int max_gap,
                            int bandwidth, int64_t budget_bytes, int32_t* status, int32_t* hits, int64_t* stats)
{
    return map_run(ctx, "rd_map_batch", reads, read_off, n_reads, min_anchors, min_score, max_gap, bandwidth, budget_bytes, status, hits, nullptr, stats);
}

extern "C" int rd_map_candidates(rd_ctx* ctx, const uint8_t* reads, const int64_t* read_off, int64_t n_reads, int min_anchors, int min_score, int max_gap,
                                 int bandwidth, int64_t budget_bytes, int max_cand, int min_frac_q10, int max_3p, int32_t* status, int32_t* n_qual,
                                 int32_t* n_cand, int32_t* cands, int64_t* stats)
{
    const MapCand cd{max_cand, min_frac_q10, max_3p, n_qual, n_cand, cands};
    return map_run(ctx, "rd_map_candidates", reads, read_off, n_reads, min_anchors, min_score, max_gap, bandwidth, budget_bytes, status, nullptr, &cd, stats);
}

// ---- diagnostic seams (include/radian_hip_diag.h): the stages above, one at a time, through the same kernels ----------------------------
extern "C" int rd_map_diag_minimizers(rd_ctx* ctx, const uint8_t* codes, const int64_t* offsets, int64_t n_records, int k, int w, uint32_t* pos_out,
                                      int64_t cap, int64_t* n_out)
{
    RD_REQUIRE(ctx != nullptr && n_out != nullptr && cap >= 0 && (cap == 0 || pos_out != nullptr), "rd_map_diag_minimizers: null argument");
    RD_REQUIRE(k >= RD_MAP_MIN_K && k <= RD_MAP_MAX_K, "rd_map_diag_minimizers: k = %d (%d..%d)", k, RD_MAP_MIN_K, RD_MAP_MAX_K);
    RD_REQUIRE(w >= 1 && w <= MAP_MAX_W, "rd_map_diag_minimizers: w = %d (1..%d)", w, MAP_MAX_W);
    if (int rc = check_records("rd_map_diag_minimizers", codes, offsets, n_records)) return rc;
    *n_out = 0;
    if (n_records == 0) return RD_OK;
    RD_HIP(hipSetDevice(ctx->device));
    if (!ctx->map) ctx->map = new MapState();   // k = 0: no index; an index that exists keeps its keys and values
    MapState* st = (MapState*)ctx->map;
    std::vector<uint8_t> flat;
    std::vector<int64_t> flat_off;
    flatten(codes, offsets, n_records, flat, flat_off);
    int64_t M = 0;
    if (int rc = minimizers_dev(ctx, st, flat, flat_off, k, w, &M)) return rc;
    *n_out = M;
    const int64_t n = std::min(M, cap);
    if (n > 0) {
        RD_HIP(hipMemcpyAsync(pos_out, st->pos.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
        RD_HIP(hipStreamSynchronize(ctx->stream));
    }
    return RD_OK;
}

extern "C" int rd_map_diag_chain(rd_ctx* ctx, const uint32_t* t, const uint32_t* r, const uint32_t* q, int64_t n, int k, int min_anchors, int max_gap,
                                 int bandwidth, int32_t* seg_out, int64_t cap_seg, int64_t* n_seg_out)
{
    RD_REQUIRE(ctx != nullptr && n_seg_out != nullptr && n >= 0 && cap_seg >= 0 && (cap_seg == 0 || seg_out != nullptr), "rd_map_diag_chain: null argument");
    RD_REQUIRE(n == 0 || (t != nullptr && r != nullptr && q != nullptr), "rd_map_diag_chain: null anchors");
    RD_REQUIRE(k >= RD_MAP_MIN_K && k <= RD_MAP_MAX_K, "rd_map_diag_chain: k = %d (%d..%d)", k, RD_MAP_MIN_K, RD_MAP_MAX_K);
    RD_REQUIRE(min_anchors >= 1, "rd_map_diag_chain: min_anchors = %d (at least 1)", min_anchors);
    RD_REQUIRE(max_gap >= 1 && max_gap < (1 << 24), "rd_map_diag_chain: max_gap = %d (1 .. 2^24 - 1)", max_gap);
    RD_REQUIRE(bandwidth >= 0 && bandwidth < (1 << 24), "rd_map_diag_chain: bandwidth = %d (0 .. 2^24 - 1)", bandwidth);
    RD_REQUIRE(n < ((int64_t)1 << 31), "rd_map_diag_chain: %lld anchors (fewer than 2^31)", (long long)n);
    for (int64_t i = 0; i < n; i++) {
        RD_REQUIRE(t[i] < (1u << 24) && r[i] < (1u << 24) && q[i] < (1u << 24), "rd_map_diag_chain: anchor %lld is (%u, %u, %u): every value is below 2^24",
                   (long long)i, t[i], r[i], q[i]);
        if (i == 0) continue;
        const bool up = t[i] != t[i - 1] ? t[i] > t[i - 1] : r[i] != r[i - 1] ? r[i] > r[i - 1] : q[i] > q[i - 1];
        RD_REQUIRE(up, "rd_map_diag_chain: anchor %lld is not above anchor %lld in (t, r, q) order: the anchors come strictly ascending", (long long)i,
                   (long long)(i - 1));
    }
    *n_seg_out = 0;
    if (n == 0) return RD_OK;
    RD_HIP(hipSetDevice(ctx->device));
    if (ctx->ws_align.reserve_exact((size_t)(n * MAP_ANCHOR_BYTES + MAP_LAUNCH_BYTES), "rd_map_diag_chain")) return RD_ERR_NOMEM;
    LaunchWs W;
    if (int rc = carve_launch_ws(ctx, "rd_map_diag_chain", n, 48, W)) return rc;   // read 0 of one launch: no bit above 48 in use
    std::vector<uint64_t> keys((size_t)n);
    for (int64_t i = 0; i < n; i++) keys[(size_t)i] = ((uint64_t)t[i] << 24) | (uint64_t)r[i];
    RD_HIP(hipMemcpyAsync(W.ka, keys.data(), (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
    RD_HIP(hipMemcpyAsync(W.qa, q, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    uint32_t n_seg = 0;
    if (int rc = chain_launch(ctx, W, W.ka, W.qa, n, k, min_anchors, max_gap, bandwidth, &n_seg)) return rc;
    std::vector<uint32_t> start(n_seg);
    std::vector<int32_t> res((size_t)n_seg * 4);
    RD_HIP(hipMemcpyAsync(start.data(), W.seg_start, (size_t)n_seg * 4, hipMemcpyDeviceToHost, ctx->stream));
    RD_HIP(hipMemcpyAsync(res.data(), W.seg_res, (size_t)n_seg * 16, hipMemcpyDeviceToHost, ctx->stream));
    RD_HIP(hipStreamSynchronize(ctx->stream));
    *n_seg_out = n_seg;
    for (int64_t s = 0; s < std::min<int64_t>(n_seg, cap_seg); s++) {
        const int32_t a0 = (int32_t)start[(size_t)s], *v = res.data() + 4 * s;
        int32_t* o = seg_out + 5 * s;
        o[0] = a0;
        o[1] = v[0];
        o[2] = v[1] - a0;
        o[3] = v[2];
        o[4] = v[3] - a0;
    }
    return RD_OK;
}
