// frame_plan_check.cpp -- csrc/frame_plan.hpp against the expressions the frame call's host driver held inline before they moved there
// (transcribed below as they stood in render_frame_impl), exhaustively over the ranges the driver can meet.  Stand-alone: exit status 0
// when every case agrees, 1 (and the first mismatch on stderr) otherwise.
#include "../../palettenerf_amd/csrc/frame_plan.hpp"
#include <initializer_list>
#include <stdio.h>

namespace old {
constexpr uint32_t kRayBlock = 256, kMaxMarchBlocks = 4096;
inline uint32_t cdiv(uint32_t a, uint32_t b) { return (a + b - 1) / b; }

uint32_t first_chunk(uint32_t predicted_iterations, int iteration_margin) {
    const uint32_t want = predicted_iterations + 1u + (uint32_t)iteration_margin;
    uint32_t chunk = predicted_iterations ? (want < 1024u ? want : 1024u) : 8u;
    return chunk;
}
void after_look(uint32_t& chunk, uint32_t& looks, uint32_t predicted_iterations) {
    if (looks == 0) chunk = predicted_iterations ? 4u : 8u;
    if (++looks >= 4 && chunk < 64) chunk *= 2;
}
struct Launches { uint32_t rows_ub, gx, gxc, field, march; };
Launches launches(uint32_t alive_ub, uint32_t N, int mode, int opt_march_blocks) {
    Launches l;
    const uint32_t ray_blocks = cdiv(alive_ub, kRayBlock);
    const uint32_t rows_ub = (uint64_t)alive_ub * 8 < N ? alive_ub * 8 : N;
    const uint32_t kResident = 1280;
    uint32_t march_cap = kMaxMarchBlocks;
    if (mode == 2) {
        if (opt_march_blocks > 0 && opt_march_blocks < 65536) march_cap = (uint32_t)opt_march_blocks < kMaxMarchBlocks ? (uint32_t)opt_march_blocks : kMaxMarchBlocks;
        else if (ray_blocks >= 2 * kResident) march_cap = kResident;
    }
    l.march = ray_blocks < march_cap ? ray_blocks : march_cap;
    const uint32_t gx = cdiv(rows_ub, 256);
    const uint32_t gxc = gx < 1024u ? gx : 1024u;
    l.rows_ub = rows_ub; l.gx = gx; l.gxc = gxc; l.field = gx < 512u ? gx : 512u;
    return l;
}
uint32_t budget(bool hosted, int iter, int march_budget0, int march_budget) { return hosted ? (uint32_t)(iter == 0 ? march_budget0 : march_budget) : 0u; }
int mode(uint32_t budget) { return budget ? 2 : 1; }
uint64_t align256(uint64_t v) { return (v + 255) & ~uint64_t(255); }
}  // namespace old

#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "frame_plan_check: " __VA_ARGS__); fprintf(stderr, "\n"); return 1; } } while (0)

int main() {
    static_assert(pnr::kRayBlock == old::kRayBlock && pnr::kMaxMarchBlocks == old::kMaxMarchBlocks, "the constants the transcription was written for");
    for (uint32_t predicted = 0; predicted <= 1100; predicted++)
        for (int margin = 0; margin <= 3; margin++)
            CHECK(pnr::first_chunk(predicted, (uint32_t)margin) == old::first_chunk(predicted, margin), "first_chunk(%u, %d)", predicted, margin);

    const uint32_t chunks[] = {1, 4, 8, 16, 32, 64, 1024};
    for (uint32_t looks = 0; looks <= 12; looks++)
        for (uint32_t chunk : chunks)
            for (uint32_t predicted : {0u, 5u}) {
                uint32_t c0 = chunk, l0 = looks, l1 = looks;
                old::after_look(c0, l0, predicted);
                const uint32_t c1 = pnr::next_chunk(chunk, l1, predicted);
                CHECK(c0 == c1 && l0 == l1, "next_chunk(%u, looks %u, %u): %u / %u looks, expected %u / %u", chunk, looks, predicted, c1, l1, c0, l0);
            }

    const uint32_t alive[] = {0, 1, 255, 256, 257, 2 * 1280 * 256 - 1, 2 * 1280 * 256, 4096 * 256 + 1};
    const uint32_t sizes[] = {1, 256, 640000};
    const int blocks[] = {0, 1, 4095, 4096, 65535, 65536};
    for (uint32_t alive_ub : alive)
        for (uint32_t N : sizes)
            for (int mode : {1, 2})
                for (int mb : blocks) {
                    const old::Launches l = old::launches(alive_ub, N, mode, mb);
                    const uint32_t rows_ub = pnr::rows_upper_bound(alive_ub, N);
                    CHECK(rows_ub == l.rows_ub, "rows_upper_bound(%u, %u)", alive_ub, N);
                    CHECK(pnr::lookup_blocks(rows_ub) == l.gx && pnr::lookup_blocks_capped(rows_ub) == l.gxc, "lookup_blocks(%u)", rows_ub);
                    CHECK(pnr::field_blocks(rows_ub) == l.field, "field_blocks(%u)", rows_ub);
                    CHECK(pnr::march_blocks(alive_ub, mode, mb) == l.march, "march_blocks(%u, %d, %d)", alive_ub, mode, mb);
                }

    for (int hosted = 0; hosted <= 1; hosted++)
        for (int iter = 0; iter <= 3; iter++)
            for (int b0 = 0; b0 <= 3; b0++)
                for (int b = 0; b <= 3; b++) {
                    const uint32_t got = pnr::march_budget(hosted != 0, iter, b0, b);
                    CHECK(got == old::budget(hosted != 0, iter, b0, b) && pnr::march_mode(got) == old::mode(got), "march_budget(%d, %d, %d, %d)", hosted, iter, b0, b);
                }

    for (uint64_t v = 0; v <= 1024; v++) CHECK(pnr::align256(v) == old::align256(v), "align256(%llu)", (unsigned long long)v);
    for (uint64_t v : {(uint64_t)1 << 32, ((uint64_t)1 << 32) + 1, ((uint64_t)1 << 40) - 1})
        CHECK(pnr::align256(v) == old::align256(v), "align256(%llu)", (unsigned long long)v);
    return 0;
}
