// grid_xside_check.cpp -- csrc/grid_xside.hpp's x-side rows against a plain restatement of the eight-corner form (the reference's get_grid_index,
// gridencoder.cu:49-72 with D = 3 and align_corners = false, written out below without sharing anything with the header), over random cells,
// resolutions and table sizes: powers of two and not, dense levels, hashed levels and sizes right at the dense / hashed switch, tiled grids.
// Every level is checked through the form level_kind() picks for it AND through the general form (kind 0).  Stand-alone: exit status 0 when every
// case agrees, 1 (and the first mismatch on stderr) otherwise.
#include "../../palettenerf_amd/csrc/grid_xside.hpp"
#include <initializer_list>
#include <stdio.h>

namespace plain {
// one corner at a time, exactly as the reference's loop over idx = 0 .. 7 forms it
uint32_t corner_row(uint32_t gridtype, uint32_t hashmap_size, uint32_t resolution, const uint32_t pg[3], uint32_t idx) {
    const uint32_t primes[3] = {1u, 2654435761u, 805459861u};
    uint32_t pl[3];
    for (uint32_t d = 0; d < 3; d++) pl[d] = (idx & (1u << d)) ? pg[d] + 1u : pg[d];
    uint32_t stride = 1, index = 0;
    for (uint32_t d = 0; d < 3 && stride <= hashmap_size; d++) {
        index += pl[d] * stride;
        stride *= resolution + 1u;
    }
    if (gridtype == 0 && stride > hashmap_size) {
        uint32_t h = 0;
        for (uint32_t d = 0; d < 3; d++) h ^= pl[d] * primes[d];
        index = h;
    }
    return index % hashmap_size;
}
}  // namespace plain

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {   // xorshift64*
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545f4914f6cdd1dull) >> 32);
}

static int check_level(uint32_t gridtype, uint32_t size, uint32_t resolution, uint32_t cells, uint32_t kinds_seen[3]) {
    const uint32_t kind = pnr::level_kind(gridtype, size, resolution);
    kinds_seen[kind]++;
    for (uint32_t c = 0; c < cells; c++) {
        uint32_t pg[3];
        // cells of the level (0 .. resolution - 1; the last one's upper corners sit on the grid's far faces), its corner cells among them
        for (uint32_t d = 0; d < 3; d++) pg[d] = c < 8 ? (((c >> d) & 1u) ? resolution - 1u : 0u) : rnd() % resolution;
        for (uint32_t k : {kind, 0u})
            for (uint32_t xside = 0; xside < 2; xside++) {
                uint32_t rows[4], rows3[4];
                pnr::x_side_rows<1>(k, gridtype, size, resolution, pg, xside, rows);
                pnr::x_side_rows<3>(k, gridtype, size, resolution, pg, xside, rows3);
                for (uint32_t jk = 0; jk < 4; jk++) {
                    const uint32_t want = plain::corner_row(gridtype, size, resolution, pg, xside + 2u * jk);
                    if (rows[jk] != want || rows3[jk] != want * 3u || want >= size) {
                        fprintf(stderr, "grid_xside_check: gridtype %u size %u resolution %u kind %u cell (%u, %u, %u) xside %u jk %u: %u (x3: %u), expected %u\n", gridtype,
                                size, resolution, k, pg[0], pg[1], pg[2], xside, jk, rows[jk], rows3[jk], want);
                        return 1;
                    }
                }
            }
    }
    return 0;
}

int main() {
    uint32_t kinds_seen[3] = {0, 0, 0};
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
    if (!kinds_seen[0] || !kinds_seen[1] || !kinds_seen[2]) { fprintf(stderr, "grid_xside_check: a form was never exercised (%u general, %u dense, %u mask)\n", kinds_seen[0], kinds_seen[1], kinds_seen[2]); return 1; }
    printf("grid_xside_check: ok (%u general, %u dense, %u mask levels)\n", kinds_seen[0], kinds_seen[1], kinds_seen[2]);
    return 0;
}
