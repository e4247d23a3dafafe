// grid_xside.hpp -- row indices of one x side of a D = 3 grid cell (host + device; no HIP dependencies so that tests/native/ can compile it with g++).
//
// The frame loop's lane-pair lookup (frame.hip: grid_pair_level) splits a cell's eight corners by their x bit: one lane of a pair loads the four
// corners (x, y + j, z + k), its neighbour the four (x + 1, y + j, z + k), so that the two rows of an x pair -- neighbours in the table on a dense
// level, and on a hashed level too, where x enters the hash as itself -- are requested by adjacent lanes of ONE load instruction.  x_side_rows()
// gives those four rows for each of the three index forms of grid_core.hpp (level_kind); every one equals the reference's
// get_grid_index (gridencoder.cu:49-72) of that corner: tests/native/grid_xside_check.cpp.
#pragma once
#include <stdint.h>

#ifndef PNR_HD
#if defined(__HIPCC__)
#define PNR_HD __host__ __device__ __forceinline__
#else
#define PNR_HD inline
#endif
#endif

namespace pnr {

// how a row index is formed on one level (grid_core.hpp describes the three forms)
PNR_HD uint32_t level_kind(uint32_t gridtype, uint32_t hashmap_size, uint32_t resolution) {
    const uint32_t side = resolution + 1u;
    if ((uint64_t)side * side * side <= (uint64_t)hashmap_size) return 1u;
    uint32_t stride = 1u;
    for (uint32_t d = 0; d < 3; d++)
        if (stride <= hashmap_size) stride *= side;
    return (gridtype == 0u && stride > hashmap_size && (hashmap_size & (hashmap_size - 1u)) == 0u) ? 2u : 0u;
}

// the reference's row index of lattice point pl (D = 3, align_corners = false), x CMUL: stride test per dimension, hash or tiled, `%`
template <uint32_t CMUL>
PNR_HD uint32_t grid_index3(uint32_t gridtype, uint32_t hashmap_size, uint32_t resolution, const uint32_t* pl /* [3] */) {
    uint32_t stride = 1, index = 0;
    for (uint32_t d = 0; d < 3; d++) {
        if (stride <= hashmap_size) {
            index += pl[d] * stride;
            stride *= resolution + 1u;
        }
    }
    if (gridtype == 0 && stride > hashmap_size) index = pl[0] ^ (pl[1] * 2654435761u) ^ (pl[2] * 805459861u);
    return (index % hashmap_size) * CMUL;
}

// rows[j + 2 k] = the row (x CMUL) of corner (pg[0] + xside, pg[1] + j, pg[2] + k), j, k in {0, 1}: corner idx = xside + 2 (j + 2 k) of the
// reference's loop.  kind: grid_core.hpp's level_kind (0 general, 1 dense, 2 hashed with a power-of-two size).
template <uint32_t CMUL>
PNR_HD void x_side_rows(uint32_t kind, uint32_t gridtype, uint32_t hashmap_size, uint32_t resolution, const uint32_t* pg /* [3] */, uint32_t xside,
                        uint32_t* rows /* [4] */) {
    const uint32_t x = pg[0] + xside;
    if (kind == 1u) {
        const uint32_t side = resolution + 1u;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (uint32_t jk = 0; jk < 4; jk++) rows[jk] = (x + (pg[1] + (jk & 1u)) * side + (pg[2] + (jk >> 1)) * side * side) * CMUL;
    } else if (kind == 2u) {
        const uint32_t mask = hashmap_size - 1u;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (uint32_t jk = 0; jk < 4; jk++) rows[jk] = ((x ^ ((pg[1] + (jk & 1u)) * 2654435761u) ^ ((pg[2] + (jk >> 1)) * 805459861u)) & mask) * CMUL;
    } else {
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (uint32_t jk = 0; jk < 4; jk++) {
            const uint32_t pl[3] = {x, pg[1] + (jk & 1u), pg[2] + (jk >> 1)};
            rows[jk] = grid_index3<CMUL>(gridtype, hashmap_size, resolution, pl);
        }
    }
}

}  // namespace pnr
