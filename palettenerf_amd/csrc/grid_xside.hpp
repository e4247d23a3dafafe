// grid_xside.hpp -- the arithmetic that turns a point into a hash-grid cell: unit cube, cell and fraction, row indices, trilinear weights.  One copy for
// every lookup (the users: grid_core.hpp).  Host + device with no HIP dependencies, so that tests/native/grid_xside_check.cpp can compile it with g++.
// The gathers and the interpolation chain, which need HIP, are in grid_core.hpp.
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef PNR_HD
#if defined(__HIPCC__)
#define PNR_HD __host__ __device__ __forceinline__
#else
#define PNR_HD inline
#endif
#endif
#if defined(__HIPCC__)
#define PNR_UNROLL _Pragma("unroll")
#else
#define PNR_UNROLL
#endif

namespace pnr {

// GridEncoder.forward's (x + bound) / (2 bound) (gridencoder/grid.py:142) for the three coordinates of a point; false = the point is outside [0, 1]^3
// (the lookup's output is then zero).  With 2 * bound a power of two -- every shipped scene -- the division is an exact scaling and so is the
// multiplication by the exact reciprocal (inv_two_bound: exact_reciprocal_or_zero(two_bound), 0 = divide): same bits, one v_mul instead of the
// ~10-instruction IEEE division (three per (sample, level): an eighth of the frame lookup's vector instructions).  Any other bound divides.
PNR_HD bool unit_cube_of(const float* xyz /* [3] */, float bound, float two_bound, float inv_two_bound, float* in /* [3] */) {
    bool oob = false;
    PNR_UNROLL
    for (int d = 0; d < 3; d++) {
        const float sft = xyz[d] + bound;
        in[d] = inv_two_bound != 0.0f ? sft * inv_two_bound : sft / two_bound;
        oob |= (in[d] < 0.0f) | (in[d] > 1.0f);
    }
    return !oob;
}

// the cell of a point of [0, 1]^D on a level -- its lower corner pg -- and the point's position inside it (gridencoder.cu:128-137)
template <uint32_t D>
PNR_HD void grid_cell(const float* in /* [D] */, float scale, bool align_corners, uint32_t* pg /* [D] */, float* frac /* [D] */) {
    PNR_UNROLL
    for (uint32_t d = 0; d < D; d++) {
        frac[d] = fmaf(in[d], scale, align_corners ? 0.0f : 0.5f);
        const float fl = floorf(frac[d]);
        pg[d] = (uint32_t)fl;
        frac[d] -= (float)pg[d];
    }
}

// the 2^D interpolation weights in the reference's order of multiplications (gridencoder.cu:150-163); corner idx's bit d = the upper side along d
template <uint32_t D>
PNR_HD float corner_weight(const float* frac /* [D] */, uint32_t idx) {
    float w = 1.0f;
    PNR_UNROLL
    for (uint32_t d = 0; d < D; d++) w *= (idx & (1u << d)) ? frac[d] : 1.0f - frac[d];
    return w;
}
template <uint32_t D>
PNR_HD void corner_weights(const float* frac /* [D] */, float* ws /* [1 << D] */) {
    PNR_UNROLL
    for (uint32_t idx = 0; idx < (1u << D); idx++) ws[idx] = corner_weight<D>(frac, idx);
}

// corner idx of the cell at pg in the reference's own loop (gridencoder.cu:150-163), for the kernels that walk the corners one by one: the corner's
// lattice point pl and, returned, its weight
template <uint32_t D>
PNR_HD float corner_point(const uint32_t* pg /* [D] */, const float* frac /* [D] */, uint32_t idx, uint32_t* pl /* [D] */) {
    float w = 1.0f;
    PNR_UNROLL
    for (uint32_t d = 0; d < D; d++) {
        if ((idx & (1u << d)) == 0) { w *= 1.0f - frac[d]; pl[d] = pg[d]; }
        else { w *= frac[d]; pl[d] = pg[d] + 1; }
    }
    return w;
}

// reference gridencoder.cu:35-72 (fast_hash + get_grid_index with ch = 0): the row of lattice point pl, x CMUL
template <uint32_t D, uint32_t CMUL>
PNR_HD uint32_t grid_index(uint32_t gridtype, bool align_corners, uint32_t hashmap_size, uint32_t resolution, const uint32_t* pl /* [D] */) {
    constexpr uint32_t primes[7] = {1u, 2654435761u, 805459861u, 3674653429u, 2097192037u, 1434869437u, 2165219737u};
    uint32_t stride = 1, index = 0;
    PNR_UNROLL
    for (uint32_t d = 0; d < D; d++) {
        if (stride <= hashmap_size) {
            index += pl[d] * stride;
            stride *= align_corners ? resolution : (resolution + 1);
        }
    }
    if (gridtype == 0 && stride > hashmap_size) {
        index = 0;
        PNR_UNROLL
        for (uint32_t d = 0; d < D; d++) index ^= pl[d] * primes[d];
    }
    return (index % hashmap_size) * CMUL;
}

// How a row index is formed on one level (gridencoder.cu:49-72 evaluated once per level instead of once per corner):
//   0 the reference's general form, grid_index (stride test per dimension, hash or tiled, `%`: ~25 instructions per corner);
//   1 dense: side^D <= size -- every stride test passes, nothing wraps, the index is below the size and the `%` is the identity;
//   2 hashed with a power-of-two size: a mask.
// All three give grid_index's value (tests/native/grid_xside_check.cpp; on the device tests/test_gpu_ops.py: the D3C2 kernel and the frame loops
// against the generic kernel and the oracle, incl. sizes that are neither).  Never dense under align_corners: there side == resolution and an
// input of exactly 1.0 gives pg + 1 == side, an index that may reach side^D >= size -- the reference wraps it with `%`, so those levels take the
// general form (or the mask, which wraps as well).
template <uint32_t D>
PNR_HD uint32_t level_kind(uint32_t gridtype, uint32_t hashmap_size, uint32_t resolution, bool align_corners = false) {
    static_assert(D == 2u || D == 3u, "forms 1 and 2 are written out for D = 2 and D = 3 (corner_row)");
    const uint32_t side = align_corners ? resolution : resolution + 1u;
    // (64-bit: side^D <= size implies every per-dimension stride test of the reference and no uint32 wrap)
    if (!align_corners && (D == 2u ? (uint64_t)side * side : (uint64_t)side * side * side) <= (uint64_t)hashmap_size) return 1u;
    // the reference multiplies a uint32 stride up dimension by dimension while it is <= size and hashes iff it ends up larger
    uint32_t stride = 1u;
    PNR_UNROLL
    for (uint32_t d = 0; d < D; d++)
        if (stride <= hashmap_size) stride *= side;
    return (gridtype == 0u && stride > hashmap_size && (hashmap_size & (hashmap_size - 1u)) == 0u) ? 2u : 0u;
}

// the row (x CMUL) of corner idx of the cell at pg, formed as `kind` says (kinds 1 and 2: D = 2 and D = 3 only)
template <uint32_t D, uint32_t CMUL>
PNR_HD uint32_t corner_row(uint32_t kind, uint32_t gridtype, bool align_corners, uint32_t hashmap_size, uint32_t resolution, const uint32_t* pg /* [D] */,
                           uint32_t idx) {
    uint32_t pl[D];
    PNR_UNROLL
    for (uint32_t d = 0; d < D; d++) pl[d] = pg[d] + ((idx >> d) & 1u);
    if constexpr (D == 2u || D == 3u) {
        if (kind == 1u) {
            const uint32_t side = resolution + 1u;
            if constexpr (D == 2u) return (pl[0] + pl[1] * side) * CMUL;
            else return (pl[0] + pl[1] * side + pl[2] * side * side) * CMUL;
        }
        if (kind == 2u) {
            const uint32_t mask = hashmap_size - 1u;
            if constexpr (D == 2u) return ((pl[0] ^ (pl[1] * 2654435761u)) & mask) * CMUL;
            else return ((pl[0] ^ (pl[1] * 2654435761u) ^ (pl[2] * 805459861u)) & mask) * CMUL;
        }
    }
    return grid_index<D, CMUL>(gridtype, align_corners, hashmap_size, resolution, pl);
}

// rows[i] = the row of corner idx = STEP i of the cell at pg, i < 2^D / STEP: all corners in the reference's order (STEP = 1), or the 2^(D-1) of
// the cell's lower x side (STEP = 2).  kind: level_kind<D> of the level, or 0.  (The kind is tested once, not once per corner.)
template <uint32_t D, uint32_t CMUL, uint32_t STEP = 1u>
PNR_HD void corner_rows(uint32_t kind, uint32_t gridtype, bool align_corners, uint32_t hashmap_size, uint32_t resolution, const uint32_t* pg /* [D] */,
                        uint32_t* rows /* [(1 << D) / STEP] */) {
    constexpr uint32_t N = (1u << D) / STEP;
    if (kind == 1u) {
        PNR_UNROLL
        for (uint32_t i = 0; i < N; i++) rows[i] = corner_row<D, CMUL>(1u, gridtype, align_corners, hashmap_size, resolution, pg, STEP * i);
    } else if (kind == 2u) {
        PNR_UNROLL
        for (uint32_t i = 0; i < N; i++) rows[i] = corner_row<D, CMUL>(2u, gridtype, align_corners, hashmap_size, resolution, pg, STEP * i);
    } else {
        PNR_UNROLL
        for (uint32_t i = 0; i < N; i++) rows[i] = corner_row<D, CMUL>(0u, gridtype, align_corners, hashmap_size, resolution, pg, STEP * i);
    }
}

// The frame loop's lane-pair lookup (frame.hip: grid_pair_level) splits a cell's eight corners by their x bit: one lane of a pair loads the four
// corners (x, y + j, z + k), its neighbour the four (x + 1, y + j, z + k), so that the two rows of an x pair -- neighbours in the table on a dense
// level, and on a hashed level too, where x enters the hash as itself -- are requested by adjacent lanes of ONE load instruction.
// rows[j + 2 k] = the row (x CMUL) of corner (pg[0] + xside, pg[1] + j, pg[2] + k), j, k in {0, 1}: corner idx = xside + 2 (j + 2 k) of the
// reference's loop, which is corner 2 (j + 2 k) of the cell one step along x.  D = 3, align_corners = false.
template <uint32_t CMUL>
PNR_HD void x_side_rows(uint32_t kind, uint32_t gridtype, uint32_t hashmap_size, uint32_t resolution, const uint32_t* pg /* [3] */, uint32_t xside,
                        uint32_t* rows /* [4] */) {
    const uint32_t qg[3] = {pg[0] + xside, pg[1], pg[2]};
    corner_rows<3, CMUL, 2u>(kind, gridtype, false, hashmap_size, resolution, qg, rows);
}

}  // namespace pnr
