// field_tiles_check.cpp -- csrc/frame_plan.hpp: field_wave_tile, the static deal of 32-row wave tiles to the waves of the NeRF field launch.
// Every wave of every workgroup walks it = 0, 1, ... and stops at its first tile beyond the launch's count, as the kernel does.  Over all of them
// every wave tile of the launch must come up exactly once, a wave's tiles must ascend (so nothing in range lies behind the tile it stopped at),
// and no two waves' loads may differ by more than one tile.  Stand-alone: exit status 0 when every case holds, 1 (and the first failure on
// stderr) otherwise.
#include "../../palettenerf_amd/csrc/frame_plan.hpp"
#include <stdio.h>
#include <vector>

static int check(uint32_t grid, uint32_t waves, uint32_t nwt) {
    std::vector<uint32_t> seen(nwt, 0u);
    uint32_t lo = UINT32_MAX, hi = 0;
    for (uint32_t block = 0; block < grid; block++)
        for (uint32_t wave = 0; wave < waves; wave++) {
            uint32_t count = 0, last = 0;
            for (uint32_t it = 0;; it++) {
                const uint32_t wt = pnr::field_wave_tile(it, wave, block, grid, waves);
                if (wt >= nwt) {
                    // the kernel breaks here: whatever the deal holds for this wave afterwards must be out of range too
                    for (uint32_t more = 1; more <= 4; more++)
                        if (pnr::field_wave_tile(it + more, wave, block, grid, waves) < nwt) {
                            fprintf(stderr, "grid %u nwt %u: block %u wave %u has a tile in range behind round %u\n", grid, nwt, block, wave, it);
                            return 1;
                        }
                    break;
                }
                if (count && wt <= last) {
                    fprintf(stderr, "grid %u nwt %u: block %u wave %u round %u: tile %u after %u\n", grid, nwt, block, wave, it, wt, last);
                    return 1;
                }
                last = wt;
                count++;
                if (seen[wt]++) {
                    fprintf(stderr, "grid %u nwt %u: wave tile %u dealt twice (block %u wave %u round %u)\n", grid, nwt, wt, block, wave, it);
                    return 1;
                }
            }
            if (count < lo) lo = count;
            if (count > hi) hi = count;
        }
    for (uint32_t wt = 0; wt < nwt; wt++)
        if (seen[wt] != 1) {
            fprintf(stderr, "grid %u nwt %u: wave tile %u dealt %u times\n", grid, nwt, wt, seen[wt]);
            return 1;
        }
    if (hi - lo > 1) {
        fprintf(stderr, "grid %u nwt %u: wave loads from %u to %u tiles\n", grid, nwt, lo, hi);
        return 1;
    }
    return 0;
}

int main() {
    const uint32_t waves = 8;
    const uint32_t grids[] = {1, 2, 511, 512};
    unsigned long cases = 0;
    for (uint32_t grid : grids) {
        const uint32_t full = grid * waves;
        const uint32_t counts[] = {0, 1, 7, 8, 9, full - 1, full, full + 1, 3 * full - 5};
        for (uint32_t nwt : counts) {
            if (check(grid, waves, nwt)) return 1;
            cases++;
        }
    }
    // the kernel's early exit: a workgroup whose wave 0 has no tile in round 0 has none at all
    for (uint32_t grid : grids)
        for (uint32_t block = 0; block < grid; block++) {
            const uint32_t first = pnr::field_wave_tile(0, 0, block, grid, waves);
            for (uint32_t wave = 1; wave < waves; wave++)
                if (pnr::field_wave_tile(0, wave, block, grid, waves) < first) {
                    fprintf(stderr, "grid %u: workgroup %u wave %u starts below wave 0's tile %u\n", grid, block, wave, first);
                    return 1;
                }
        }
    printf("field_tiles_check: %lu cases hold\n", cases);
    return 0;
}
