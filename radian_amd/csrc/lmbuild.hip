// lmbuild.hip -- building the RNA k-mer model the beam search decodes with (radian/decode.py:42-49,77-96,152-158 fix what a row means;
// the reference ships one model and no tool that makes one).  DESIGN.md 13.
//
//   host   rd_fasta_scan   one pass over a FASTA text: header filter, one code byte per base (0..3 = ACGT, 255 = break), record offsets
//   device rd_lm_build     count every window of k + 1 labels (decode order: the transcript reversed), marginals for the lower orders,
//                          back-off selection and normalisation into the context's LM image, then the same finishing pass rd_load_lm
//                          runs (entropies, absent mask) -- the built table IS the loaded model, without a host round trip
//          rd_lm_score     mean -ln p(next | context) of another set of transcripts under the context's model
//
// Counts are integers (32-bit, the input refused when it could hold more windows than that), the table is one correctly rounded float64
// division per entry, sums of float64 terms are reduced in a fixed order: the result depends neither on record order nor on how the
// input is cut into launches, and two builds are bit-identical.
//
// The scanner is plain C++ (tests/asan_fasta.cpp compiles this file for the CPU under the sanitizers); the device half needs hipcc.
#include "common.h"
#include "../../include/radian_hip.h"

#include <algorithm>
#include <chrono>
#include <string.h>

// ------------------------------------------------------------------------------------------------------------------ FASTA scanner
namespace {

// one code per byte of a sequence line: 0..3 ACGT (U = T, either case), 255 a break (any other letter, '*', '-'), 254 white space,
// 253 an error
struct FastaCodes {
    uint8_t t[256];
    FastaCodes()
    {
        for (int c = 0; c < 256; c++) t[c] = 253;
        for (int c = 'A'; c <= 'Z'; c++) t[c] = t[c + 32] = 255;
        t['*'] = t['-'] = 255;
        t[' '] = t['\t'] = t['\r'] = t['\n'] = t['\v'] = t['\f'] = 254;
        const char* b = "ACGT";
        for (int i = 0; i < 4; i++) t[(int)b[i]] = t[(int)b[i] + 32] = (uint8_t)i;
        t['U'] = t['u'] = 3;
    }
};

// does field `field` of the header [h, he), split on '|', equal value?
bool header_matches(const char* h, const char* he, int field, const char* value, size_t vlen)
{
    for (int f = 0; f < field; f++) {
        const char* bar = (const char*)memchr(h, '|', (size_t)(he - h));
        if (!bar) return false;
        h = bar + 1;
    }
    const char* bar = (const char*)memchr(h, '|', (size_t)(he - h));
    const char* fe = bar ? bar : he;
    return (size_t)(fe - h) == vlen && memcmp(h, value, vlen) == 0;
}

}  // namespace

// counts[0] = records read, [1] = records kept, [2] = codes of the kept records.  codes == nullptr: count only (the first pass);
// otherwise codes[counts[2]] and offsets[counts[1] + 1] are filled (the second pass, sized by the first).
extern "C" int rd_fasta_scan(const char* buf, size_t n, int field, const char* value, uint8_t* codes, int64_t* offsets, int64_t* counts)
{
    RD_REQUIRE(counts && (buf || n == 0), "rd_fasta_scan: null argument");
    RD_REQUIRE((codes == nullptr) == (offsets == nullptr), "rd_fasta_scan: codes and offsets go together");
    RD_REQUIRE(field < 0 || value, "rd_fasta_scan: a header field to match needs a value");
    static const FastaCodes T;
    const size_t vlen = field >= 0 ? strlen(value) : 0;
    const char* p = buf;
    const char* e = buf + n;
    int64_t line = 0, rec = 0, kept = 0, bases = 0;
    bool keep = false;
    while (p < e) {
        line++;
        const char* eol = (const char*)memchr(p, '\n', (size_t)(e - p));
        if (!eol) eol = e;
        if (*p == '>') {
            const char* he = eol;
            if (he > p + 1 && he[-1] == '\r') he--;
            rec++;
            keep = field < 0 || header_matches(p + 1, he, field, value, vlen);
            if (keep) {
                if (offsets) offsets[kept] = bases;
                kept++;
            }
        } else {
            for (const char* q = p; q < eol; q++) {
                const uint8_t c = T.t[(uint8_t)*q];
                if (c == 254) continue;
                if (c == 253) {
                    rd_set_error("rd_fasta_scan: record %lld, line %lld: byte 0x%02x is not a sequence character", (long long)rec, (long long)line,
                                 (unsigned)(uint8_t)*q);
                    return RD_ERR_FORMAT;
                }
                if (rec == 0) {
                    rd_set_error("rd_fasta_scan: record 0, line %lld: sequence before the first '>' header", (long long)line);
                    return RD_ERR_FORMAT;
                }
                if (keep) {
                    if (codes) codes[bases] = c;
                    bases++;
                }
            }
        }
        p = eol < e ? eol + 1 : e;
    }
    if (offsets) offsets[kept] = bases;
    counts[0] = rec;
    counts[1] = kept;
    counts[2] = bases;
    return RD_OK;
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------------------------------ device half
#include "glibc_math.h"
#include "glibc_tables.h"

namespace {

__device__ const uint64_t g_lb_log_tab[256] = RD_GLIBC_LOG_TAB;

#pragma clang fp contract(off)

constexpr int kThreads = 256;
constexpr int kScoreItems = 16;                       // windows per thread of the scorer: one partial sum per kThreads * kScoreItems windows
constexpr uint8_t kBreak = 255;
constexpr int64_t kDefaultCut = (int64_t)256 << 20;   // stream bytes per launch

// first counter of order j in the counts buffer: orders k, k - 1, ..., 0 follow each other, order j holding 4^(j+1) counters
__host__ __device__ inline size_t order_off(int k, int j) { return (((size_t)1 << (2 * (k + 2))) - ((size_t)1 << (2 * (j + 2)))) / 3; }

// the window starting at s[0]: k + 1 labels.  Decode order is the transcript reversed (basecall.py:130 writes the FASTA line reversed):
// next label = s[0], context = s[k] (oldest) ... s[1]; as_written: context = s[0] (oldest) ... s[k-1], next = s[k].
// -> (context << 2) | next, or 0xffffffff when a label is a break
__device__ inline uint32_t window_code(const uint8_t* s, int k, int as_written)
{
    uint32_t code = 0, bad = 0;
    if (as_written)
        for (int q = 0; q <= k; q++) {
            const uint32_t b = s[q];
            bad |= b;
            code = (code << 2) | (b & 3u);
        }
    else
        for (int q = k; q >= 0; q--) {
            const uint32_t b = s[q];
            bad |= b;
            code = (code << 2) | (b & 3u);
        }
    return bad > 3u ? 0xffffffffu : code;
}

// The count: partition, then histogram in LDS.  (One global integer atomic per window, the obvious form, was measured beside this one and
// left: 28.3 ms against 8.0 ms for 2.5e8 windows at k = 11)  A window's code is split into a bucket (its high bits) and `low`
// bits such that a bucket's sub-table of 2^low counters fits one workgroup's LDS.  lm_part_hist_kernel sizes the buckets, lm_part_scan_kernel places them,
// lm_part_scatter_kernel writes every window's low bits into its bucket (one global atomic per bucket and tile of 8192 windows, not per
// window), lm_bucket_hist_kernel -- one workgroup per bucket -- counts in LDS and adds its sub-table to the table with plain stores.
constexpr int kTileItems = 32;                      // windows per thread of the partition kernels
constexpr int kMaxBuckets = 8192;
constexpr int kMaxLow = 15;

__global__ void __launch_bounds__(kThreads) lm_part_hist_kernel(const uint8_t* __restrict__ s, int64_t m, int k, int as_written, int low, int n_buckets,
                                                                uint32_t* __restrict__ bucket_count)
{
    __shared__ uint32_t h[kMaxBuckets];
    for (int b = threadIdx.x; b < n_buckets; b += kThreads) h[b] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * kThreads * kTileItems;
    for (int q = 0; q < kTileItems; q++) {
        const int64_t i = base + (int64_t)q * kThreads + threadIdx.x;
        if (i >= m) break;
        const uint32_t code = window_code(s + i, k, as_written);
        if (code != 0xffffffffu) atomicAdd(&h[code >> low], 1u);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < n_buckets; b += kThreads)
        if (h[b]) atomicAdd(&bucket_count[b], h[b]);
}

// start[b] = cursor[b] = windows in the buckets before b; start[n_buckets] = all
__global__ void __launch_bounds__(kThreads) lm_part_scan_kernel(const uint32_t* __restrict__ bucket_count, int n_buckets, uint32_t* __restrict__ start,
                                                                uint32_t* __restrict__ cursor)
{
    __shared__ uint32_t h[kMaxBuckets + 1];
    for (int b = threadIdx.x; b < n_buckets; b += kThreads) h[b] = bucket_count[b];
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (int b = 0; b < n_buckets; b++) {
            const uint32_t c = h[b];
            h[b] = run;
            run += c;
        }
        h[n_buckets] = run;
    }
    __syncthreads();
    for (int b = threadIdx.x; b <= n_buckets; b += kThreads) {
        start[b] = h[b];
        if (b < n_buckets) cursor[b] = h[b];
    }
}

__global__ void __launch_bounds__(kThreads) lm_part_scatter_kernel(const uint8_t* __restrict__ s, int64_t m, int k, int as_written, int low, int n_buckets,
                                                                   uint32_t* __restrict__ cursor, uint16_t* __restrict__ out)
{
    __shared__ uint32_t h[kMaxBuckets], at[kMaxBuckets];
    for (int b = threadIdx.x; b < n_buckets; b += kThreads) h[b] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * kThreads * kTileItems;
    uint32_t code[kTileItems];
#pragma unroll
    for (int q = 0; q < kTileItems; q++) {
        const int64_t i = base + (int64_t)q * kThreads + threadIdx.x;
        code[q] = i < m ? window_code(s + i, k, as_written) : 0xffffffffu;
        if (code[q] != 0xffffffffu) atomicAdd(&h[code[q] >> low], 1u);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < n_buckets; b += kThreads) {
        at[b] = h[b] ? atomicAdd(&cursor[b], h[b]) : 0u;
        h[b] = 0;
    }
    __syncthreads();
    const uint32_t mask = (1u << low) - 1u;
#pragma unroll
    for (int q = 0; q < kTileItems; q++)
        if (code[q] != 0xffffffffu) {
            const uint32_t b = code[q] >> low;
            out[at[b] + atomicAdd(&h[b], 1u)] = (uint16_t)(code[q] & mask);
        }
}

__global__ void __launch_bounds__(1024) lm_bucket_hist_kernel(const uint16_t* __restrict__ in, const uint32_t* __restrict__ start, int low, uint32_t* __restrict__ counts)
{
    __shared__ uint32_t sub[1 << kMaxLow];
    const uint32_t n_sub = 1u << low;
    const uint32_t lo = start[blockIdx.x], hi = start[blockIdx.x + 1];
    if (lo == hi) return;
    for (uint32_t i = threadIdx.x; i < n_sub; i += 1024) sub[i] = 0;
    __syncthreads();
    for (uint32_t i = lo + threadIdx.x; i < hi; i += 1024) atomicAdd(&sub[in[i]], 1u);
    __syncthreads();
    uint32_t* dst = counts + ((size_t)blockIdx.x << low);
    for (uint32_t i = threadIdx.x; i < n_sub; i += 1024)
        if (sub[i]) dst[i] += sub[i];
}

// C_j[s][b] = sum over the oldest label a of C_{j+1}[a s][b]: flat, out[i] = sum_a in[a * n_out + i]
__global__ void __launch_bounds__(kThreads) lm_marginal_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, size_t n_out)
{
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n_out) out[i] = in[i] + in[n_out + i] + in[2 * n_out + i] + in[3 * n_out + i];
}

// Row of context c: the largest order j <= k whose row of the context's last j labels has a positive sum; p = (C + alpha) / (sum + 4 alpha).
// unseen: 0 = back off as above, 1 = uniform row when order k has no count, 2 = NaN row (absent).  hist[j] = rows filled from order j,
// hist[14] = uniform rows, hist[15] = absent rows.
__global__ void __launch_bounds__(kThreads) lm_normalise_kernel(const uint32_t* __restrict__ counts, int k, int unseen, double alpha,
                                                                double* __restrict__ table, unsigned long long* __restrict__ hist)
{
    __shared__ uint32_t h[16];
    if (threadIdx.x < 16) h[threadIdx.x] = 0;
    __syncthreads();
    const size_t n = (size_t)1 << (2 * k);
    const size_t c = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (c < n) {
        double p[4];
        int slot = -1;
        for (int j = k; j >= 0; j--) {
            const size_t suffix = c & (((size_t)1 << (2 * j)) - 1);
            const uint32_t* row = counts + order_off(k, j) + suffix * 4;
            const uint32_t r0 = row[0], r1 = row[1], r2 = row[2], r3 = row[3];
            const unsigned long long sum = (unsigned long long)r0 + r1 + r2 + r3;
            if (sum > 0) {
                const double den = __dadd_rn((double)sum, 4.0 * alpha);      // (4 alpha is exact)
                p[0] = __ddiv_rn(__dadd_rn((double)r0, alpha), den);
                p[1] = __ddiv_rn(__dadd_rn((double)r1, alpha), den);
                p[2] = __ddiv_rn(__dadd_rn((double)r2, alpha), den);
                p[3] = __ddiv_rn(__dadd_rn((double)r3, alpha), den);
                slot = j;
                break;
            }
            if (unseen != 0) break;
        }
        if (slot < 0) {
            const double v = unseen == 1 ? 0.25 : __builtin_nan("");
            p[0] = p[1] = p[2] = p[3] = v;
            slot = unseen == 1 ? 14 : 15;
        }
        double* t = table + c * 4;
        t[0] = p[0];
        t[1] = p[1];
        t[2] = p[2];
        t[3] = p[3];
        atomicAdd(&h[slot], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 16 && h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], (unsigned long long)h[threadIdx.x]);
}

// What rd_load_lm derives from a table: per-context entropy (decode.py:73-76,85-90: math.log == glibc's log, Python's sum is left to right),
// and for a row of NaN -- a context a sparse model does not hold -- a zeroed row, entropy +inf (the gate stays closed) and its bit in the
// absent mask.  One context per lane; a wave writes its 64 mask bits as two words.
__global__ void __launch_bounds__(kThreads) lm_finish_kernel(double* __restrict__ table, size_t n, int hashed, double* __restrict__ entropy,
                                                             uint32_t* __restrict__ missing, unsigned long long* __restrict__ n_missing)
{
    const size_t c = (size_t)blockIdx.x * kThreads + threadIdx.x;
    bool absent = false;
    if (c < n) {
        double* d = table + c * 4;
        double v[4] = {d[0], d[1], d[2], d[3]};
        absent = !hashed && v[0] != v[0];
        double ent;
        if (absent) {
            d[0] = d[1] = d[2] = d[3] = 0.0;
            ent = __builtin_inf();
        } else {
            double s = 0.0;
            bool any = false;
            for (int i = 0; i < 4; i++)
                if (v[i] > 0) {
                    const double t = __dmul_rn(v[i], gm_log(v[i], g_lb_log_tab));
                    s = any ? __dadd_rn(s, t) : t;
                    any = true;
                }
            ent = any ? -s : 0.0;
        }
        entropy[c] = ent;
    }
    const unsigned long long bits = __ballot(absent);
    if ((threadIdx.x & 63) == 0 && c < n) {
        missing[c >> 5] = (uint32_t)bits;
        missing[(c >> 5) + 1] = (uint32_t)(bits >> 32);
        if (bits) atomicAdd(n_missing, (unsigned long long)__popcll(bits));
    }
}

// out[0] += contexts whose gate would open (entropy < r, decode.py:90), out[1] += windows counted at order k in such contexts,
// out[2] += contexts seen at order k
__global__ void __launch_bounds__(kThreads) lm_gate_stats_kernel(const double* __restrict__ entropy, const uint32_t* __restrict__ counts, size_t n, double r_thr,
                                                                 unsigned long long* __restrict__ out)
{
    __shared__ unsigned long long s[3];
    if (threadIdx.x < 3) s[threadIdx.x] = 0;
    __syncthreads();
    const size_t c = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (c < n) {
        const uint32_t* row = counts + c * 4;
        const unsigned long long sum = (unsigned long long)row[0] + row[1] + row[2] + row[3];
        if (sum) atomicAdd(&s[2], 1ull);
        if (entropy[c] < r_thr) {
            atomicAdd(&s[0], 1ull);
            if (sum) atomicAdd(&s[1], sum);
        }
    }
    __syncthreads();
    if (threadIdx.x < 3 && s[threadIdx.x]) atomicAdd(&out[threadIdx.x], s[threadIdx.x]);
}

// Held-out score.  Block b takes windows [b * kThreads * kScoreItems, ...): a thread adds its terms in order, the block's 256 sums are
// folded pairwise in a fixed order into partial[b].  tallies: [0] windows, [1] p > 0 (a term each), [2] p = 0, [3] context absent,
// [4] gate open.
__global__ void __launch_bounds__(kThreads) lm_score_kernel(const uint8_t* __restrict__ s, int64_t m, int k, int as_written, const double* __restrict__ table,
                                                            const double* __restrict__ entropy, const uint32_t* __restrict__ missing, int sparse, double r_thr,
                                                            double* __restrict__ partial, unsigned long long* __restrict__ tallies)
{
    __shared__ double acc[kThreads];
    __shared__ unsigned long long t[5];
    if (threadIdx.x < 5) t[threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * kThreads * kScoreItems;
    double sum = 0.0;
    uint32_t n_win = 0, n_pos = 0, n_zero = 0, n_abs = 0, n_open = 0;
    for (int q = 0; q < kScoreItems; q++) {
        const int64_t i = base + (int64_t)q * kThreads + threadIdx.x;
        if (i >= m) break;
        const uint32_t code = window_code(s + i, k, as_written);
        if (code == 0xffffffffu) continue;
        const uint32_t ctx = code >> 2;
        n_win++;
        if (entropy[ctx] < r_thr) n_open++;
        if (sparse && ((missing[ctx >> 5] >> (ctx & 31)) & 1u)) {
            n_abs++;
            continue;
        }
        const double p = table[code];
        if (p > 0) {
            sum = __dadd_rn(sum, -gm_log(p, g_lb_log_tab));
            n_pos++;
        } else
            n_zero++;
    }
    acc[threadIdx.x] = sum;
    if (n_win) atomicAdd(&t[0], (unsigned long long)n_win);
    if (n_pos) atomicAdd(&t[1], (unsigned long long)n_pos);
    if (n_zero) atomicAdd(&t[2], (unsigned long long)n_zero);
    if (n_abs) atomicAdd(&t[3], (unsigned long long)n_abs);
    if (n_open) atomicAdd(&t[4], (unsigned long long)n_open);
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) acc[threadIdx.x] = __dadd_rn(acc[threadIdx.x], acc[threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = acc[0];
    if (threadIdx.x < 5 && t[threadIdx.x]) atomicAdd(&tallies[threadIdx.x], t[threadIdx.x]);
}

// the partial sums of every launch, in one pass and one fixed order: thread t adds partial[t], partial[t + 256], ..., then the pairwise fold
__global__ void __launch_bounds__(kThreads) lm_score_fold_kernel(const double* __restrict__ partial, int64_t n, double* __restrict__ out)
{
    __shared__ double acc[kThreads];
    double sum = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += kThreads) sum = __dadd_rn(sum, partial[i]);
    acc[threadIdx.x] = sum;
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) acc[threadIdx.x] = __dadd_rn(acc[threadIdx.x], acc[threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = acc[0];
}

// The records as one stream: record r's codes, then one break, so that no window spans two records.  Record r starts at stream
// position offsets[r] + r.  fill() copies stream bytes [at, at + len) into out, breaks beyond the end.
struct Stream {
    const uint8_t* codes;
    const int64_t* offsets;
    int64_t n_records;
    int64_t size() const { return offsets[n_records] + n_records; }
    void fill(int64_t at, int64_t len, uint8_t* out) const
    {
        const int64_t total = size();
        int64_t done = 0;
        // first record whose end (its break included) lies beyond `at`: binary search on offsets[r + 1] + r + 1 > at
        int64_t lo = 0, hi = n_records;
        while (lo < hi) {
            const int64_t mid = (lo + hi) / 2;
            if (offsets[mid + 1] + mid + 1 > at) hi = mid;
            else lo = mid + 1;
        }
        int64_t r = lo;
        while (done < len && at + done < total) {
            const int64_t pos = at + done;
            const int64_t start = offsets[r] + r, end = offsets[r + 1] + r;   // [start, end) codes, `end` the break
            if (pos < end) {
                const int64_t take = std::min(end - pos, len - done);
                memcpy(out + done, codes + offsets[r] + (pos - start), (size_t)take);
                done += take;
            } else {
                out[done++] = kBreak;
                r++;
            }
        }
        if (done < len) memset(out + done, kBreak, (size_t)(len - done));
    }
};

using Clock = std::chrono::steady_clock;
// microseconds since t; t becomes now
int64_t since(Clock::time_point& t)
{
    const Clock::time_point now = Clock::now();
    const int64_t us = std::chrono::duration_cast<std::chrono::microseconds>(now - t).count();
    t = now;
    return us;
}

struct Scratch {   // device buffers of one call
    DevBuf b[4];
    ~Scratch()
    {
        for (DevBuf& x : b) x.release();
    }
};

int check_records(const char* who, const uint8_t* codes, const int64_t* offsets, int64_t n_records)
{
    RD_REQUIRE(offsets && n_records >= 0 && offsets[0] == 0, "%s: record offsets must start at 0", who);
    for (int64_t r = 0; r < n_records; r++) RD_REQUIRE(offsets[r + 1] >= offsets[r], "%s: record offsets must not decrease (record %lld)", who, (long long)r);
    RD_REQUIRE(codes || offsets[n_records] == 0, "%s: null codes", who);
    return RD_OK;
}

}  // namespace

int rd_lm_finish_device(rd_ctx* ctx, int table_order, int context_len, int hashed)
{
    LM& lm = ctx->lm;
    const size_t n = (size_t)1 << (2 * table_order);
    unsigned long long* d_n = nullptr;
    RD_HIP(hipMalloc((void**)&d_n, sizeof(unsigned long long)));
    hipError_t e = hipMemsetAsync(d_n, 0, sizeof(unsigned long long), ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(lm.d_missing, 0, ((n + 63) / 64) * sizeof(double), ctx->stream);
    unsigned long long n_missing = 0;
    if (e == hipSuccess) {
        hipLaunchKernelGGL(lm_finish_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, ctx->stream, lm.table, n, hashed, lm.d_entropy,
                           lm.d_missing, d_n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&n_missing, d_n, sizeof n_missing, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    (void)hipFree(d_n);
    RD_HIP(e);
    lm.k = context_len;
    lm.table_order = table_order;
    lm.hashed = hashed;
    lm.sparse = n_missing ? 1 : 0;
    lm.gate_valid = false;
    lm.loaded = true;
    return RD_OK;
}

extern "C" int rd_lm_build(rd_ctx* ctx, const uint8_t* codes, const int64_t* offsets, int64_t n_records, int k, int as_written, int unseen, double alpha,
                           double r_thr, int64_t cut, double* table_out, uint32_t* counts_out, int64_t* stats)
{
    RD_REQUIRE(ctx && stats, "rd_lm_build: null argument");
    RD_REQUIRE(k >= 1 && k <= 13, "rd_lm_build: context length %d out of range [1,13]", k);
    RD_REQUIRE(unseen >= 0 && unseen <= 2, "rd_lm_build: unseen mode %d (0 = back off, 1 = uniform, 2 = absent)", unseen);
    RD_REQUIRE(alpha >= 0 && alpha < 1e300, "rd_lm_build: pseudocount %g must be finite and not negative", alpha);
    RD_REQUIRE(cut >= 0, "rd_lm_build: negative launch cut");
    as_written = as_written ? 1 : 0;
    if (int rc = check_records("rd_lm_build", codes, offsets, n_records)) return rc;
    // 32-bit counters: every window ends at a code of its own, so the codes bound the windows -- and every counter
    RD_REQUIRE(offsets[n_records] <= (int64_t)0xffffffffll, "rd_lm_build: %lld bases could hold more than 2^32 - 1 counted windows (32-bit counters)",
               (long long)offsets[n_records]);
    RD_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const Stream S{codes, offsets, n_records};
    const int64_t total = S.size();
    if (cut == 0) cut = kDefaultCut;
    cut = std::min<int64_t>(cut, std::max<int64_t>(total, 1));
    const size_t n = (size_t)1 << (2 * k);
    const size_t n_counters = order_off(k, -1);      // orders k .. 0
    Scratch sc;
    DevBuf &d_counts = sc.b[0], &d_codes = sc.b[1], &d_small = sc.b[2];
    if (d_counts.reserve(n_counters * sizeof(uint32_t)) || d_codes.reserve((size_t)(cut + k)) || d_small.reserve(32 * sizeof(unsigned long long))) return RD_ERR_NOMEM;
    uint32_t* counts = d_counts.as<uint32_t>();
    unsigned long long* small = d_small.as<unsigned long long>();   // [0..15] rows per order, [16..18] gate statistics
    RD_HIP(hipMemsetAsync(counts, 0, n * 4 * sizeof(uint32_t), st));
    RD_HIP(hipMemsetAsync(small, 0, 32 * sizeof(unsigned long long), st));
    // bucket = code >> low; at least 256 buckets where the code has the bits for it, sub-tables of at most 2^15 counters
    const int low = std::max(0, std::min(kMaxLow, 2 * (k + 1) - 8));
    const int n_buckets = 1 << (2 * (k + 1) - low);
    DevBuf &d_part = sc.b[3];
    if (d_part.reserve((size_t)(cut + 2) * sizeof(uint16_t) + (size_t)(3 * n_buckets + 4) * sizeof(uint32_t))) return RD_ERR_NOMEM;
    uint32_t* bucket_count = (uint32_t*)(d_part.as<uint16_t>() + ((cut + 1) & ~(int64_t)1));   // behind the partitioned windows, 4-byte aligned
    uint32_t* bucket_start = bucket_count + n_buckets;
    uint32_t* bucket_cursor = bucket_start + n_buckets + 1;
    std::vector<uint8_t> stage((size_t)(cut + k));
    int64_t us[5] = {0, 0, 0, 0, 0};   // host staging, upload, count, marginals + table + finishing, download
    for (int64_t at = 0; at < total; at += cut) {
        const int64_t m = std::min(cut, total - at);
        Clock::time_point t = Clock::now();
        S.fill(at, m + k, stage.data());
        us[0] += since(t);
        RD_HIP(hipMemcpyAsync(d_codes.p, stage.data(), (size_t)(m + k), hipMemcpyHostToDevice, st));
        RD_HIP(hipStreamSynchronize(st));
        us[1] += since(t);
        {
            const int tiles = (int)((m + kThreads * kTileItems - 1) / (kThreads * kTileItems));
            RD_HIP(hipMemsetAsync(bucket_count, 0, (size_t)n_buckets * sizeof(uint32_t), st));
            hipLaunchKernelGGL(lm_part_hist_kernel, dim3(tiles), dim3(kThreads), 0, st, d_codes.as<uint8_t>(), m, k, as_written, low, n_buckets, bucket_count);
            hipLaunchKernelGGL(lm_part_scan_kernel, dim3(1), dim3(kThreads), 0, st, bucket_count, n_buckets, bucket_start, bucket_cursor);
            hipLaunchKernelGGL(lm_part_scatter_kernel, dim3(tiles), dim3(kThreads), 0, st, d_codes.as<uint8_t>(), m, k, as_written, low, n_buckets, bucket_cursor,
                               d_part.as<uint16_t>());
            hipLaunchKernelGGL(lm_bucket_hist_kernel, dim3(n_buckets), dim3(1024), 0, st, d_part.as<uint16_t>(), bucket_start, low, counts);
        }
        RD_HIP(hipGetLastError());
        RD_HIP(hipStreamSynchronize(st));            // (the staging buffer is reused)
        us[2] += since(t);
    }
    Clock::time_point t = Clock::now();
    for (int j = k - 1; j >= 0; j--) {
        const size_t n_out = (size_t)1 << (2 * (j + 1));
        hipLaunchKernelGGL(lm_marginal_kernel, dim3((unsigned)((n_out + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, counts + order_off(k, j + 1),
                           counts + order_off(k, j), n_out);
        RD_HIP(hipGetLastError());
    }
    uint32_t c0[4];
    RD_HIP(hipMemcpyAsync(c0, counts + order_off(k, 0), sizeof c0, hipMemcpyDeviceToHost, st));
    RD_HIP(hipStreamSynchronize(st));
    const int64_t windows = (int64_t)c0[0] + c0[1] + c0[2] + c0[3];
    RD_REQUIRE(windows > 0, "rd_lm_build: the input holds no window of %d labels over ACGT: nothing to count", k + 1);

    LM& lm = ctx->lm;
    lm.loaded = false;
    lm.gate_valid = false;
    if (lm.storage.reserve(rd_lm_image_doubles(k) * sizeof(double))) return RD_ERR_NOMEM;
    lm.table_order = k;
    rd_lm_bind(lm);
    const unsigned blocks = (unsigned)((n + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(lm_normalise_kernel, dim3(blocks), dim3(kThreads), 0, st, counts, k, unseen, alpha, lm.table, small);
    RD_HIP(hipGetLastError());
    RD_HIP(hipStreamSynchronize(st));
    us[3] += since(t);
    if (counts_out) RD_HIP(hipMemcpyAsync(counts_out, counts, n * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (table_out) RD_HIP(hipMemcpyAsync(table_out, lm.table, n * 4 * sizeof(double), hipMemcpyDeviceToHost, st));   // (before the absent rows are zeroed)
    RD_HIP(hipStreamSynchronize(st));
    us[4] += since(t);
    if (int rc = rd_lm_finish_device(ctx, k, k, 0)) return rc;
    hipLaunchKernelGGL(lm_gate_stats_kernel, dim3(blocks), dim3(kThreads), 0, st, lm.d_entropy, counts, n, r_thr, small + 16);
    RD_HIP(hipGetLastError());
    unsigned long long h[32];
    RD_HIP(hipMemcpyAsync(h, small, sizeof h, hipMemcpyDeviceToHost, st));
    RD_HIP(hipStreamSynchronize(st));
    stats[0] = windows;
    stats[1] = (int64_t)h[18];      // contexts seen at order k
    stats[2] = (int64_t)h[16];      // contexts whose gate opens
    stats[3] = (int64_t)h[17];      // counted windows in such contexts
    stats[4] = (int64_t)h[15];      // absent rows
    stats[5] = (int64_t)h[14];      // uniform rows
    stats[6] = total ? (total + cut - 1) / cut : 0;   // launches of the count
    stats[7] = 0;
    for (int j = 0; j < 14; j++) stats[8 + j] = (int64_t)h[j];
    us[3] += since(t);
    for (int i = 0; i < 5; i++) stats[24 + i] = us[i];
    return RD_OK;
}

extern "C" int rd_lm_score(rd_ctx* ctx, const uint8_t* codes, const int64_t* offsets, int64_t n_records, int as_written, double r_thr, int64_t cut,
                           int64_t* stats, double* nll_sum)
{
    RD_REQUIRE(ctx && stats && nll_sum, "rd_lm_score: null argument");
    const LM& lm = ctx->lm;
    if (!lm.loaded) {
        rd_set_error("rd_lm_score: no RNA model in the context (rd_lm_build / rd_load_lm)");
        return RD_ERR_STATE;
    }
    RD_REQUIRE(!lm.hashed, "rd_lm_score: a hashed long-context model (rd_load_lm_hashed) has no rows to score against");
    RD_REQUIRE(cut >= 0, "rd_lm_score: negative launch cut");
    if (int rc = check_records("rd_lm_score", codes, offsets, n_records)) return rc;
    RD_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int k = lm.k;
    const Stream S{codes, offsets, n_records};
    const int64_t total = S.size();
    if (cut == 0) cut = kDefaultCut;
    cut = std::min<int64_t>(cut, std::max<int64_t>(total, 1));
    const int64_t per_block = (int64_t)kThreads * kScoreItems;
    const int64_t blocks_per_cut = (cut + per_block - 1) / per_block;
    const int64_t n_launch = (total + cut - 1) / cut;
    const int64_t n_partial = std::max<int64_t>(1, n_launch * blocks_per_cut);
    Scratch sc;
    DevBuf &d_codes = sc.b[0], &d_partial = sc.b[1], &d_small = sc.b[2];
    if (d_codes.reserve((size_t)(cut + k)) || d_partial.reserve((size_t)n_partial * sizeof(double)) || d_small.reserve(8 * sizeof(unsigned long long))) return RD_ERR_NOMEM;
    unsigned long long* small = d_small.as<unsigned long long>();   // [0..4] tallies, [5] the folded sum (a double)
    RD_HIP(hipMemsetAsync(small, 0, 8 * sizeof(unsigned long long), st));
    RD_HIP(hipMemsetAsync(d_partial.p, 0, (size_t)n_partial * sizeof(double), st));
    std::vector<uint8_t> stage((size_t)(cut + k));
    int64_t used = 0;
    for (int64_t at = 0; at < total; at += cut) {
        const int64_t m = std::min(cut, total - at);
        const int64_t blocks = (m + per_block - 1) / per_block;
        S.fill(at, m + k, stage.data());
        RD_HIP(hipMemcpyAsync(d_codes.p, stage.data(), (size_t)(m + k), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(lm_score_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, st, d_codes.as<uint8_t>(), m, k, as_written, lm.table, lm.d_entropy,
                           lm.d_missing, lm.sparse, r_thr, d_partial.as<double>() + used, small);
        RD_HIP(hipGetLastError());
        RD_HIP(hipStreamSynchronize(st));
        used += blocks;
    }
    hipLaunchKernelGGL(lm_score_fold_kernel, dim3(1), dim3(kThreads), 0, st, d_partial.as<double>(), used, (double*)(small + 5));
    RD_HIP(hipGetLastError());
    unsigned long long h[8];
    RD_HIP(hipMemcpyAsync(h, small, sizeof h, hipMemcpyDeviceToHost, st));
    RD_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < 5; i++) stats[i] = (int64_t)h[i];
    memcpy(nll_sum, &h[5], sizeof(double));
    return RD_OK;
}
#endif  // __HIPCC__
