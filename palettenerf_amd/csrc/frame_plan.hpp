// frame_plan.hpp -- the integer rules of the frame call's host driver (frame.hip): how many iterations go out between two looks at the
// control block, and how large each iteration's launches are.  Host only, no HIP dependencies, so that tests/native/ can compile it with
// g++ and compare it with the expressions it replaced (frame_plan_check.cpp).
#pragma once
#include <stdint.h>

namespace pnr {

constexpr uint32_t kRayBlock = 256;
#ifndef PNR_MAX_MARCH_BLOCKS
#define PNR_MAX_MARCH_BLOCKS 4096   // (2048: a frame of 2 500 chunks gave 452 workgroups a second chunk behind their block barriers; first launch 88.1 -> 86.4 us on average)
#endif
constexpr uint32_t kMaxMarchBlocks = PNR_MAX_MARCH_BLOCKS;
constexpr uint32_t kResidentMarchBlocks = 1280;   // MODE 2 runs five workgroups per CU

inline uint64_t align256(uint64_t v) { return (v + 255) & ~uint64_t(255); }
inline uint32_t plan_cdiv(uint32_t a, uint32_t b) { return (a + b - 1) / b; }
inline uint32_t plan_min(uint32_t a, uint32_t b) { return a < b ? a : b; }

// Iterations enqueued between two looks at the control block.  Consecutive frames of a camera path need nearly the same
// number of iterations, so the first chunk is the previous frame's count (one look per frame when the guess holds; launches
// past the end are no-ops that cost a few microseconds each); after that, short chunks that grow for long, translucent marches.
// (+1: the launch that finds no ray left is the one that reports it; + `margin` spare iterations (pnr_set_option "iteration_margin").  Along a
// camera path the count drifts by one or two from frame to frame; a spare iteration is four early-exit launches (~19 us), a wrong guess one host
// round trip.  Measured on the moving-camera benchmark the round trip is the cheaper of the two: the margin defaults to 0)
inline uint32_t first_chunk(uint32_t predicted, uint32_t margin) {
    return predicted ? plan_min(predicted + 1u + margin, 1024u) : 8u;
}
// The chunk behind a look that found the frame unfinished (`looks` counts them, this one included afterwards).
inline uint32_t next_chunk(uint32_t chunk, uint32_t& looks, uint32_t predicted) {
    if (looks == 0) chunk = predicted ? 4u : 8u;
    if (++looks >= 4 && chunk < 64) chunk *= 2;
    return chunk;
}
// Upper bound of an iteration's sample rows: at most 8 samples per alive ray, and never more than N (the schedule's n_step = min(N / n_alive, 8))
inline uint32_t rows_upper_bound(uint32_t alive_ub, uint32_t N) { return (uint64_t)alive_ub * 8 < N ? alive_ub * 8 : N; }
// Workgroups along x of the lookup launch (256 rows each; the kernels stride over the rest) and of the NeRF field launch
inline uint32_t lookup_blocks(uint32_t rows_ub) { return plan_cdiv(rows_ub, 256); }
inline uint32_t lookup_blocks_capped(uint32_t rows_ub) { return plan_min(lookup_blocks(rows_ub), 1024u); }
inline uint32_t field_blocks(uint32_t rows_ub) { return plan_min(lookup_blocks(rows_ub), 512u); }
// The NeRF field launch deals 32-row wave tiles to its waves statically, SIMD-major: of a round's grid * waves tiles, four consecutive ones go to
// waves 0..3 of a workgroup (one per SIMD: wave w sits on SIMD w % 4), workgroup after workgroup, then four each to waves 4..7.  A launch's last,
// partial round so gives the first workgroups one tile per SIMD before any SIMD gets a second one (dealt by the workgroup, eight waves of the first
// few workgroups took it; dealt wave-major as the PaletteNeRF field does it, (it * waves + wave) * grid + block, the same waves of ALL workgroups,
// the last ones to start included: profiles/EXPERIMENTS.md).  A wave's tiles ascend with `it`: it stops at its first tile beyond the launch's
// count; a workgroup's first tile is its wave 0's.  `waves` is a multiple of four.  constexpr: the kernel calls it too.
constexpr uint32_t field_wave_tile(uint32_t it, uint32_t wave, uint32_t block, uint32_t grid, uint32_t waves) {
    return it * grid * waves + (wave / 4u) * (grid * 4u) + block * 4u + (wave % 4u);
}
// hosted tail (MODE 2): the march gives every ray `budget` sample-less probes and queues the rest for the lookup launch's first workgroups
inline uint32_t march_budget(bool hosted, int iter, int budget_first, int budget_later) { return hosted ? (uint32_t)(iter == 0 ? budget_first : budget_later) : 0u; }
inline int march_mode(uint32_t budget) { return budget ? 2 : 1; }
// Workgroups of a march launch (one 256-ray chunk of the alive list each, or several).
// MODE 2 runs five workgroups per CU (1 280 resident).  A typical later lego launch has 1 352 chunks: its last 72 workgroups start ~8 us late
// (launch 16.9 us), and capping the launch at 1 280 is no way out -- a workgroup's second chunk waits at the block barriers for the slowest
// wave of its first one (18.4 us).  With three chunks and more per resident workgroup (garden: 4 256) the cap does pay: the chunks of a
// workgroup share its prologue (mip staging, chunk sums): 38.7 -> 33.1 us per launch.  "march_blocks" overrides (0 / 65536 = this rule).
inline uint32_t march_blocks(uint32_t alive_ub, int mode, int march_blocks_option) {
    const uint32_t ray_blocks = plan_cdiv(alive_ub, kRayBlock);
    uint32_t cap = kMaxMarchBlocks;
    if (mode == 2) {
        if (march_blocks_option > 0 && march_blocks_option < 65536) cap = plan_min((uint32_t)march_blocks_option, kMaxMarchBlocks);
        else if (ray_blocks >= 2 * kResidentMarchBlocks) cap = kResidentMarchBlocks;
    }
    return plan_min(ray_blocks, cap);
}

}  // namespace pnr
