// align_batch.h -- the batch alignment routine of align.hip as other sources call it: rd_align_batch is this routine with an empty
// hook, rd_pileup_add (pileup.hip) the same with a hook that consumes a launch's alignment columns where they lie.
#pragma once
#include "common.h"

struct AlnPair {
    int64_t ref, read;   // byte offsets of the sequences in the workspace
    int64_t ops;         // byte offset of the op slot (n + m bytes)
    int64_t bnd;         // int32 offset of the boundary rows: H [m + 1], then E [m + 1]
    int64_t dir;         // uint32 offset of the direction words
    int32_t n, m;
};
constexpr int ALN_RES = 7;   // per-pair result ints: score, n_match, n_sub, n_ins, n_del, status, n_ops

// One launch of the routine, after align_tb_kernel was queued on `stream`: slot k of the launch is the caller's pair slot_pair[k]
struct AlnLaunch {
    const AlnPair* d_pairs;      // device: the slots' descriptors
    uint8_t* d_ws;               // device: the workspace the descriptors' offsets refer to
    const int32_t* d_res;        // device: ALN_RES ints per slot (score and n_ops are final once the stream reaches the hook's work)
    uint8_t* d_extra;            // device: n_slots * extra_pair_bytes of the hook's own, 256-aligned (nullptr without extra bytes)
    int n_slots;
    const int32_t* slot_pair;    // host
    const AlnPair* h_pairs;      // host: the descriptors
    hipStream_t stream;
};
struct AlnHook {
    size_t extra_pair_bytes = 0;   // workspace the hook wants per slot, inside the budget (a batch then takes 256 bytes more)
    virtual void accepted(int n_pairs) {}                      // every argument check passed: set the hook's own outputs to "not aligned yet"
    virtual int launched(const AlnLaunch&) { return RD_OK; }   // queue work behind the traceback; must not wait
    virtual int finished(const AlnLaunch&) { return RD_OK; }   // the stream has been synchronised
    virtual ~AlnHook() {}
};

// who: the entry point the error texts name; too_large: the name of its status for a pair over the budget
int rd_align_batch_run(rd_ctx* ctx, const char* who, const char* too_large, const uint8_t* refs, const int64_t* ref_off, const uint8_t* reads,
                       const int64_t* read_off, int n_pairs, int match, int mismatch, int gap_open, int gap_extend, int64_t budget_bytes,
                       int32_t* score, int32_t* counts, int32_t* status, uint8_t* ops_out, const int64_t* ops_off, int32_t* ops_len, AlnHook& hook);
