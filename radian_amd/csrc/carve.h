// carve.h -- how a stage lays out its device block, once.  Plain host C++ without a HIP type: tests/asan_carve.cpp
// compiles it with g++ and checks its properties.
//
// A stage describes its block in ONE function, xx_layout(Carve&, dims..., XxWs*), a list of take() calls in the block's order.  The entry
// point runs it twice: dry (no base), which gives the bytes to reserve, and then on the buffer, which gives the pointers.  Sizes and
// pointers come from the same lines, so no block can be sized by one expression and carved by another.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

struct Carve {
    char* base;   // nullptr: a dry pass that only sizes
    size_t at;    // the offset the next block gets
    explicit Carve(void* base_ = nullptr, size_t at0 = 0) : base((char*)base_), at(at0) {}
    // a block of count * sizeof(T) + slack_bytes, rounded up to a multiple of align (1: as it is); nullptr when dry
    template <typename T> T* take(size_t count, size_t slack_bytes = 0, size_t align = 256)
    {
        const size_t o = at;
        at += (count * sizeof(T) + slack_bytes + align - 1) / align * align;
        return base ? (T*)(base + o) : nullptr;
    }
    void round(size_t align = 256) { at = (at + align - 1) / align * align; }   // (behind blocks taken unrounded)
    size_t mark() const { return at; }                                          // for the sites that store offsets in descriptors
    bool fits(size_t cap) const { return at <= cap; }
};

// The maximal runs of members[0 .. n) (indices into src_off, in launch order) that are contiguous in the source: run(i, k) for members
// [i, k) with src_off[members[j]] == src_off[members[j - 1] + 1] for every j in (i, k).  One copy of src_off[members[k - 1] + 1] -
// src_off[members[i]] elements moves such a run.  Members without elements never split a run, and skipped ones without elements neither.
// (the launch's side of it: off[i] = the elements of members [0, i), n + 1 of them -- where member i lands in the launch's dense array)
inline void rd_gather_offsets(const int64_t* src_off, const int32_t* members, int64_t n, std::vector<int64_t>& off)
{
    off.assign(1, 0);
    for (int64_t i = 0; i < n; i++) off.push_back(off.back() + src_off[members[i] + 1] - src_off[members[i]]);
}
template <typename Run>
inline void rd_gather_runs(const int32_t* members, int64_t n, const int64_t* src_off, Run run)
{
    for (int64_t i = 0, k; i < n; i = k) {
        for (k = i + 1; k < n && src_off[members[k]] == src_off[members[k - 1] + 1]; k++) {}
        run(i, k);
    }
}
