// grid_xside_check.cpp -- csrc/grid_xside.hpp, the one copy of the hash-grid cell arithmetic, against plain restatements that share nothing with
// the header (the reference's get_grid_index, gridencoder.cu:49-72, and its weight loop, gridencoder.cu:150-163, written out below):
//   * every corner's row through corner_rows / corner_row, for D = 2 and D = 3, align_corners both ways, and the D = 3 x-side rows of the lane-pair
//     lookup, over random cells, resolutions and table sizes: powers of two and not, dense levels, hashed levels and sizes right at the dense / hashed
//     switch, tiled grids; the far-face cells (pg + 1 == side under align_corners) among them.  Every level is checked through the form
//     level_kind() picks for it AND through the general form (kind 0);
//   * grid_cell at 0, 1, the largest float below 1 and inputs that land exactly on a cell border;
//   * corner_weights and corner_point against the reference's order of multiplications, bit for bit.
// Stand-alone: exit status 0 when every case agrees, 1 (and the first mismatch on stderr) otherwise.
#include "../../palettenerf_amd/csrc/grid_xside.hpp"
#include <initializer_list>
#include <stdio.h>
#include <string.h>

namespace plain {
// one corner at a time, exactly as the reference's loop over idx = 0 .. 2^D - 1 forms it
uint32_t corner_row(uint32_t D, uint32_t gridtype, bool align_corners, uint32_t hashmap_size, uint32_t resolution, const uint32_t* pg, uint32_t idx) {
    const uint32_t primes[3] = {1u, 2654435761u, 805459861u};
    uint32_t pl[3] = {0, 0, 0};
    for (uint32_t d = 0; d < D; d++) pl[d] = (idx & (1u << d)) ? pg[d] + 1u : pg[d];
    uint32_t stride = 1, index = 0;
    for (uint32_t d = 0; d < D && stride <= hashmap_size; d++) {
        index += pl[d] * stride;
        stride *= align_corners ? resolution : resolution + 1u;
    }
    if (gridtype == 0 && stride > hashmap_size) {
        uint32_t h = 0;
        for (uint32_t d = 0; d < D; d++) h ^= pl[d] * primes[d];
        index = h;
    }
    return index % hashmap_size;
}
// the reference's weight of corner idx: one multiplication per dimension, in the order of the dimensions
float corner_weight(uint32_t D, const float* frac, uint32_t idx) {
    float w = 1;
    for (uint32_t d = 0; d < D; d++) {
        if ((idx & (1u << d)) == 0) w *= 1 - frac[d];
        else w *= frac[d];
    }
    return w;
}
}  // namespace plain

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {   // xorshift64*
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545f4914f6cdd1dull) >> 32);
}

// kinds_seen[D - 2][align_corners][kind]
typedef uint32_t KindsSeen[2][2][3];

template <uint32_t D>
static int check_level_d(uint32_t gridtype, bool ac, uint32_t size, uint32_t resolution, uint32_t cells, KindsSeen& kinds_seen) {
    const uint32_t kind = pnr::level_kind<D>(gridtype, size, resolution, ac);
    if (kind > 2u || (ac && kind == 1u)) { fprintf(stderr, "grid_xside_check: level_kind<%u> = %u with align_corners = %d (size %u resolution %u)\n", D, kind, (int)ac, size, resolution); return 1; }
    kinds_seen[D - 2][ac][kind]++;
    for (uint32_t c = 0; c < cells; c++) {
        uint32_t pg[3] = {0, 0, 0};
        // cells of the level (0 .. resolution - 1; the last one's upper corners sit on the grid's far faces: pg + 1 == side under align_corners), its corner cells among them
        for (uint32_t d = 0; d < D; d++) pg[d] = c < 8 ? (((c >> d) & 1u) ? resolution - 1u : 0u) : rnd() % resolution;
        for (uint32_t k : {kind, 0u}) {
            uint32_t rows[1u << D], rows3[1u << D];
            pnr::corner_rows<D, 1>(k, gridtype, ac, size, resolution, pg, rows);
            pnr::corner_rows<D, 3>(k, gridtype, ac, size, resolution, pg, rows3);
            for (uint32_t idx = 0; idx < (1u << D); idx++) {
                const uint32_t want = plain::corner_row(D, gridtype, ac, size, resolution, pg, idx);
                const uint32_t one = pnr::corner_row<D, 1>(k, gridtype, ac, size, resolution, pg, idx);
                if (rows[idx] != want || rows3[idx] != want * 3u || one != want || want >= size) {
                    fprintf(stderr, "grid_xside_check: D %u gridtype %u align_corners %d size %u resolution %u kind %u cell (%u, %u, %u) corner %u: %u (x3: %u, alone: %u), expected %u\n",
                            D, gridtype, (int)ac, size, resolution, k, pg[0], pg[1], pg[2], idx, rows[idx], rows3[idx], one, want);
                    return 1;
                }
            }
            if (D != 3u || ac) continue;
            for (uint32_t xside = 0; xside < 2; xside++) {   // the lane-pair lookup's split of the eight corners by their x bit
                uint32_t xs[4], xs3[4];
                pnr::x_side_rows<1>(k, gridtype, size, resolution, pg, xside, xs);
                pnr::x_side_rows<3>(k, gridtype, size, resolution, pg, xside, xs3);
                for (uint32_t jk = 0; jk < 4; jk++) {
                    const uint32_t want = plain::corner_row(3, gridtype, false, size, resolution, pg, xside + 2u * jk);
                    if (xs[jk] != want || xs3[jk] != want * 3u) {
                        fprintf(stderr, "grid_xside_check: gridtype %u size %u resolution %u kind %u cell (%u, %u, %u) xside %u jk %u: %u (x3: %u), expected %u\n", gridtype,
                                size, resolution, k, pg[0], pg[1], pg[2], xside, jk, xs[jk], xs3[jk], want);
                        return 1;
                    }
                }
            }
        }
    }
    return 0;
}
static int check_level(uint32_t gridtype, uint32_t size, uint32_t resolution, uint32_t cells, KindsSeen& kinds_seen) {
    for (int ac = 0; ac < 2; ac++)
        if (check_level_d<3>(gridtype, ac != 0, size, resolution, cells, kinds_seen) || check_level_d<2>(gridtype, ac != 0, size, resolution, cells, kinds_seen)) return 1;
    return 0;
}

static bool same_bits(float a, float b) { return memcmp(&a, &b, 4) == 0; }

// grid_cell: hand-worked cases (every product and sum below is exact in fp32 unless the comment says how it rounds)
static int check_cells() {
    const float below1 = 1.0f - 5.9604644775390625e-08f;   // 1 - 2^-24, the largest float below 1
    struct Case { float in, scale; bool ac; uint32_t pg; float frac; };
    const Case cases[] = {
        {0.0f, 15.0f, false, 0u, 0.5f},               // level 0 of the shipped encoder: scale 15, resolution 16
        {1.0f, 15.0f, false, 15u, 0.5f},              // 15.5: the last cell, pg + 1 = 16 = resolution < side
        {below1, 15.0f, false, 15u, 0.5f - 9.5367431640625e-07f},   // 15.5 - 15 * 2^-24 rounds to 15.5 - 2^-20 (0.94 of the spacing below 15.5)
        {0.0f, 15.0f, true, 0u, 0.0f},
        {1.0f, 15.0f, true, 15u, 0.0f},               // exactly on the far face: pg + 1 == side == resolution
        {below1, 15.0f, true, 14u, 1.0f - 9.5367431640625e-07f},    // 15 - 15 * 2^-24 rounds to 15 - 2^-20
        {0.3125f, 8.0f, false, 3u, 0.0f},             // 2.5 + 0.5: exactly on the border between cells 2 and 3 -> the upper cell, fraction 0
        {0.4375f, 8.0f, false, 4u, 0.0f},
        {0.375f, 8.0f, true, 3u, 0.0f},               // 3.0 on the border
        {0.5f, 4095.0f, false, 2048u, 0.0f},          // the finest shipped level: 2047.5 + 0.5
        {1.0f, 4095.0f, false, 4095u, 0.5f},
        {1.0f, 4095.0f, true, 4095u, 0.0f},
        {0.0f, 4095.0f, true, 0u, 0.0f},
    };
    for (const Case& c : cases) {
        for (uint32_t D = 2; D <= 3; D++) {
            const float in[3] = {c.in, c.in, c.in};
            uint32_t pg[3] = {~0u, ~0u, ~0u};
            float frac[3] = {-1.0f, -1.0f, -1.0f};
            if (D == 2) pnr::grid_cell<2>(in, c.scale, c.ac, pg, frac); else pnr::grid_cell<3>(in, c.scale, c.ac, pg, frac);
            for (uint32_t d = 0; d < 3; d++) {
                const bool set = d < D;
                if (set ? (pg[d] != c.pg || !same_bits(frac[d], c.frac)) : (pg[d] != ~0u || frac[d] != -1.0f)) {
                    fprintf(stderr, "grid_xside_check: grid_cell<%u>(%.9g, scale %g, align_corners %d)[%u] = cell %u fraction %.9g, expected %u and %.9g\n", D, c.in, c.scale,
                            (int)c.ac, d, pg[d], frac[d], c.pg, c.frac);
                    return 1;
                }
            }
        }
    }
    // the unit cube in front of it: the exact reciprocal and the division give the same bits for a power-of-two 2 * bound; outside is outside
    for (uint32_t t = 0; t < 20000; t++) {
        const float bound = (float)(1u << (t % 4u));
        float xyz[3], a[3], b[3];
        for (int d = 0; d < 3; d++) xyz[d] = ((float)(rnd() >> 8) / 8388608.0f - 1.0f) * bound * (t % 7u == 0 ? 1.25f : 1.0f);
        const bool ia = pnr::unit_cube_of(xyz, bound, 2 * bound, 1.0f / (2 * bound), a), ib = pnr::unit_cube_of(xyz, bound, 2 * bound, 0.0f, b);
        bool inside = true;
        for (int d = 0; d < 3; d++) {   // (the shifted coordinate as fp32 forms it: a point a rounding beyond the face still lands on it)
            const float sft = xyz[d] + bound;
            inside = inside && sft >= 0.0f && sft <= 2 * bound;
        }
        if (ia != ib || ia != inside || memcmp(a, b, sizeof(a)) != 0) {
            fprintf(stderr, "grid_xside_check: unit_cube_of(%.9g, %.9g, %.9g; bound %g): reciprocal %d (%.9g, %.9g, %.9g), division %d (%.9g, %.9g, %.9g), expected inside = %d\n",
                    xyz[0], xyz[1], xyz[2], bound, (int)ia, a[0], a[1], a[2], (int)ib, b[0], b[1], b[2], (int)inside);
            return 1;
        }
    }
    return 0;
}

template <uint32_t D>
static int check_weights_d() {
    for (uint32_t t = 0; t < 20000; t++) {
        float frac[D], ws[1u << D];
        for (uint32_t d = 0; d < D; d++) frac[d] = t < 8 ? (float)((t >> d) & 1u) * 0.99999994f : (float)(rnd() >> 8) / 16777216.0f;   // [0, 1), 0 and the largest fraction among them
        pnr::corner_weights<D>(frac, ws);
        const uint32_t pg[3] = {5, 6, 7};
        for (uint32_t idx = 0; idx < (1u << D); idx++) {
            const float want = plain::corner_weight(D, frac, idx);
            uint32_t pl[D];
            const float wp = pnr::corner_point<D>(pg, frac, idx, pl);
            bool point_ok = true;
            for (uint32_t d = 0; d < D; d++) point_ok = point_ok && pl[d] == pg[d] + ((idx >> d) & 1u);
            if (!same_bits(ws[idx], want) || !same_bits(pnr::corner_weight<D>(frac, idx), want) || !same_bits(wp, want) || !point_ok) {
                fprintf(stderr, "grid_xside_check: D %u corner %u: weight %.9g (alone %.9g, corner_point %.9g, its lattice point %s), expected %.9g\n", D, idx, ws[idx],
                        pnr::corner_weight<D>(frac, idx), wp, point_ok ? "right" : "wrong", want);
                return 1;
            }
        }
    }
    return 0;
}

int main() {
    if (check_cells() || check_weights_d<2>() || check_weights_d<3>()) return 1;
    KindsSeen kinds_seen = {};
    // the shipped configuration: 16 levels from 16 to 4096 (the encoder's resolutions), tables capped at 2^19 rows and aligned to 8 as the encoder sizes them
    const uint32_t res16[] = {16, 24, 34, 49, 71, 102, 147, 213, 308, 445, 643, 929, 1342, 1939, 2802, 4049, 4097};
    for (uint32_t r : res16) {
        uint64_t dense = (uint64_t)(r + 1) * (r + 1) * (r + 1);
        uint32_t size = (uint32_t)(dense < (1u << 19) ? (dense + 7) / 8 * 8 : (1u << 19));
        for (uint32_t gridtype = 0; gridtype < 2; gridtype++)
            if (check_level(gridtype, size, r, 2000, kinds_seen)) return 1;
    }
    // right at the dense / hashed switch: side^3 - 1, side^3, side^3 + 1 rows, and one and two strides short (the stride test stops after x, after y)
    for (uint32_t r : {1u, 2u, 3u, 7u, 15u, 16u, 31u, 63u, 79u}) {
        const uint32_t side = r + 1, cube = side * side * side;
        for (uint32_t size : {cube - 1, cube, cube + 1, side * side - 1, side * side, side * side + 1, side - 1, side, side + 1, 1u, 2u})
            for (uint32_t gridtype = 0; gridtype < 2; gridtype++)
                if (size && check_level(gridtype, size, r, 300, kinds_seen)) return 1;
    }
    // random resolutions against random sizes: powers of two (the mask form), their neighbours and arbitrary sizes
    for (uint32_t t = 0; t < 3000; t++) {
        const uint32_t r = 1u + rnd() % (t & 1u ? 5000u : 120u);
        const uint32_t p2 = 1u << (rnd() % 25u);
        const uint32_t size = (t % 3u == 0) ? p2 : ((t % 3u == 1) ? p2 + (rnd() % 3u) - 1u : 1u + rnd() % (1u << 24));
        if (size && check_level(t >> 1 & 1u, size, r, 64, kinds_seen)) return 1;
    }
    for (uint32_t D = 2; D <= 3; D++) {
        const uint32_t* plain_ = kinds_seen[D - 2][0];
        const uint32_t* ac = kinds_seen[D - 2][1];
        // every form was exercised (align_corners: never the dense form, by design)
        if (!plain_[0] || !plain_[1] || !plain_[2] || !ac[0] || ac[1] || !ac[2]) {
            fprintf(stderr, "grid_xside_check: D %u: a form was never exercised (%u general, %u dense, %u mask; align_corners: %u general, %u dense, %u mask)\n", D, plain_[0], plain_[1],
                    plain_[2], ac[0], ac[1], ac[2]);
            return 1;
        }
        printf("grid_xside_check: D %u ok (%u general, %u dense, %u mask levels; align_corners: %u general, %u mask)\n", D, plain_[0], plain_[1], plain_[2], ac[0], ac[2]);
    }
    return 0;
}
