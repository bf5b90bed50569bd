// band_sweep.h -- device only: the row-by-row sweep of a left-to-right dynamic programme that ea_dp_kernel (eventalign.hip), sm_dp_kernel
// (sigmap.hip), ca_dp_kernel (ctcalign.hip) and ear_dp_kernel (eventalign.hip, event rows) share, and its primitives.  DESIGN.md section 16.
//
// One workgroup of 256 threads sweeps one sequence of n states over the rows t < T.  A thread owns 16 consecutive states in registers, a
// workgroup pass a BAND of 4096 states; a sequence of more states is swept band after band, the last state of a band at every row going
// through a one-cell-per-row column in global memory (two columns of T cells, written and read in turn).  Row t of a thread needs, from
// outside the thread, its left neighbour's last state of row t - 1 only: one DPP wave_shr:1 inside a wave, one LDS cell (xch, two
// parities) and the row's single barrier between waves, the band's incoming column for the first thread.  A sequence of at most 1024
// states runs on its first wave alone and has no barrier.  The per-row inputs and the incoming column come through LDS in tiles of
// P::TR rows, fetched from global memory a tile ahead and read from LDS a row ahead.
//
// On the single-wave path the tile is written by some lanes and read by others with no s_barrier between: LDS operations of one wave
// execute in order, so what is needed is that the compiler keeps them in order.  wave_barrier() alone restrains only the scheduler;
// wave_lds_sync() adds the wavefront-scope fence that makes the order a guarantee.  Every single-wave hand-off here goes through it.
//
// band_sweep<P> owns the protocol -- bands, barriers, parities, tiles, the neighbour, the column -- and a policy P the arithmetic:
//   P::Cell                  what crosses a thread boundary (the last state of a thread at a row); lane_shr1(Cell) must exist
//   P::Elem, P::TR, P::SLOTS a tile is TR * SLOTS elements, a multiple of 64; element e of the tile is tile[e] in LDS
//   P::first_row(b)          the first row of band b (the cells above are unreachable)
//   P::none()                the cell that means "nothing comes from the left"
//   p.begin_band(b)          the thread's states of band b: their constants and their values at row first_row(b) - 1
//   p.tile_elem(e, tbase, T, b, cin)   element e of the tile whose first row is tbase; cin[t - 1] is the incoming column at row t (b > 0)
//   P::Row, p.read_row(tile, r)        what a row reads from row r of a tile;  P::incoming(row): the incoming column's cell in it
//   P::AHEAD_CLAMPED         how the row-ahead read ends at a tile's last row: true, it reads that row again (no branch in the row: a lone
//                            wave of eventalign loses 0.75 % to the branch); false, it is skipped (ctcalign's ten doubles per row lose
//                            2.4 % to the clamped address); profiles/r26_band_sweep_ab.json
//   p.row(t, in, left)       row t of the thread's 16 states, with whatever it stores per row
//   p.last()                 the thread's last state
//   p.end_band()             after the last row
// The policy is a plain struct whose members are the thread's registers; everything is inlined.
#pragma once
#include <stdint.h>

namespace {

constexpr int BS_NT = 256;                 // threads of a DP workgroup
constexpr int BS_K = 16;                   // states a thread owns
constexpr int BS_BAND = BS_NT * BS_K;      // states of one workgroup pass
constexpr int BS_WAVE_STATES = 64 * BS_K;  // at most this many states: the first wave alone, no barrier

// lane l receives v of lane l - 1; lane 0 keeps its own (DPP wave_shr:1, bound_ctrl off)
__device__ __forceinline__ int32_t lane_shr1(int32_t v) { return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ double lane_shr1(double v) { return __hiloint2double(lane_shr1(__double2hiint(v)), lane_shr1(__double2loint(v))); }
// a thread's last TWO states, for a DP whose cell also reads two states to the left (ear_dp_kernel, eventalign.hip): b is the last state and
// a the one before it.  Two DPP moves; xch and the band column then carry 8 bytes a cell
struct Cell2 {
    int32_t a, b;
};
__device__ __forceinline__ Cell2 lane_shr1(Cell2 v) { return Cell2{lane_shr1(v.a), lane_shr1(v.b)}; }

// the single-wave path's ordering of LDS writes before other lanes' reads: a wavefront-scope fence, then the scheduling barrier
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

template <class P>
__device__ __forceinline__ void band_sweep(P& p, int64_t n, int T, typename P::Cell* col)
{
    using Cell = typename P::Cell;
    using Elem = typename P::Elem;
    constexpr int TR = P::TR, TILE = P::TR * P::SLOTS, PRE = TILE / 64;
    static_assert(TILE % 64 == 0, "a tile: whole elements per lane of a lone wave");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool single = n <= BS_WAVE_STATES;
    if (single && wave) return;   // (the first wave never waits at a barrier then)
    const int bands = (int)((n + BS_BAND - 1) / BS_BAND);
    __shared__ Cell xch[2][BS_NT / 64];   // [row parity][wave]
    __shared__ Elem tile[2][TILE];
    const int nact = single ? 64 : BS_NT, per = (TILE + nact - 1) / nact;   // threads at work, tile elements each
    auto mine = [&](int i, int e) { return i < per && (TILE % BS_NT == 0 || e < TILE); };   // (i < per: the same in every thread)

    for (int b = 0; b < bands; b++) {
        const int t_lo = P::first_row(b);
        if (t_lo >= T) break;   // (then the states of this band and the later ones are unreachable in the last row too)
        p.begin_band(b);
        const Cell* cin = col + (size_t)((b + 1) & 1) * T;   // written by band b - 1
        Cell* cout = col + (size_t)(b & 1) * T;
        const bool write_col = tid == BS_NT - 1 && b + 1 < bands;
        if (!single) {
            __syncthreads();   // the previous band's last exchange reads and column writes
            if (lane == 63) xch[(t_lo + 1) & 1][wave] = P::none();
            __syncthreads();
        }
        auto tile_load = [&](int tbase, Elem* pre) {
#pragma unroll
            for (int i = 0; i < PRE; i++) {
                const int e = tid + i * nact;
                if (mine(i, e)) pre[i] = p.tile_elem(e, tbase, T, b, cin);
            }
        };
        auto tile_store = [&](int buf, const Elem* pre) {
#pragma unroll
            for (int i = 0; i < PRE; i++) {
                const int e = tid + i * nact;
                if (mine(i, e)) tile[buf][e] = pre[i];
            }
            if (single) wave_lds_sync();
            else __syncthreads();
        };
        Elem pre[PRE];
        tile_load(t_lo, pre);
        tile_store(0, pre);
        // Everything the set-up loaded has arrived, on every path.  The compiler places a wait where a loaded register is first used; if
        // that is inside the row loop, the wait also covers the next tile's fetch and every row's store (one counter for all of them).
        __builtin_amdgcn_s_waitcnt(0);
        int buf = 0;
        for (int tb = t_lo; tb < T; tb += TR, buf ^= 1) {
            const bool more = tb + TR < T;
            if (more) tile_load(tb + TR, pre);
            const int nr = T - tb < TR ? T - tb : TR;
            typename P::Row next = p.read_row(tile[buf], 0);
            for (int r = 0; r < nr; r++) {
                const int t = tb + r;
                const typename P::Row in = next;
                if constexpr (P::AHEAD_CLAMPED) next = p.read_row(tile[buf], r + 1 < nr ? r + 1 : r);
                else if (r + 1 < nr) next = p.read_row(tile[buf], r + 1);
                Cell left = lane_shr1(p.last());
                if (lane == 0) left = wave > 0 ? xch[(t + 1) & 1][wave - 1] : P::incoming(in);
                p.row(t, in, left);
                if (write_col) cout[t] = p.last();
                if (!single) {
                    if (lane == 63) xch[t & 1][wave] = p.last();
                    __syncthreads();
                }
            }
            if (more) tile_store(buf ^ 1, pre);
        }
        p.end_band();
        if (!single) __threadfence_block();
    }
}

}  // namespace
