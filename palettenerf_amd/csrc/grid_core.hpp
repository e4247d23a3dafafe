// grid_core.hpp -- the hash-grid lookup's shared pieces: level constants, the corner accumulators of the generic kernels, the eight gathers and the
// interpolation chain of the D = 3 lookups.  The arithmetic in front of them (unit cube, cell and fraction, row indices, weights) is grid_xside.hpp's.
// Users: gridencoder.hip (the generic kernels, k_grid_fwd_d3c2 and its pair form), grid_binned.hip (corners_of), frame.hip (grid_row, the lane-pair
// lookup), occupancy.hip (k_occ_lookup), background.hip (the D = 2 lookup and its gradient).
#pragma once
#include "pnr_common.hpp"
#include "grid_xside.hpp"
#include <math.h>

namespace pnr {

constexpr uint32_t kMaxLevels = 32;
struct LevelParams {
    float scale[kMaxLevels];
    uint32_t resolution[kMaxLevels];
};

__device__ __forceinline__ float to_f32(float v) { return v; }
__device__ __forceinline__ float to_f32(__half v) { return __half2float(v); }

// accumulate one corner: fp32 table -> fmaf chain; fp16 table -> half accumulator with the
// reference's two roundings (gridencoder.cu:142,165 with scalar_t = at::Half)
template <uint32_t C>
__device__ __forceinline__ void corner_accumulate(float acc[C], float w, const float* __restrict__ g) {
    if constexpr (C == 2) {
        const float2 v = *reinterpret_cast<const float2*>(g);
        acc[0] = fmaf(w, v.x, acc[0]); acc[1] = fmaf(w, v.y, acc[1]);
    } else if constexpr (C == 4) {
        const float4 v = *reinterpret_cast<const float4*>(g);
        acc[0] = fmaf(w, v.x, acc[0]); acc[1] = fmaf(w, v.y, acc[1]); acc[2] = fmaf(w, v.z, acc[2]); acc[3] = fmaf(w, v.w, acc[3]);
    } else {
#pragma unroll
        for (uint32_t ch = 0; ch < C; ch++) acc[ch] = fmaf(w, g[ch], acc[ch]);
    }
}
// half(w * v) with the reference's TWO roundings: the product to fp32, that to fp16.  Left as one expression the compiler may select v_fma_mixlo_f16
// for it (an fp32 fma with ONE rounding to f16) -- it did in k_grid_fwd<__half, D, 1> for every D and in <__half, 4, 4> and <__half, 5, 4> -- and where the
// fp32 product lands on the midpoint of two halves (~6e-5 of the products) the result is the other neighbour than the reference's and the oracle's
// (tests/test_gpu_grid_variants.py).  The empty statement makes the fp32 product a value of its own, whichever instructions are selected around it.
__device__ __forceinline__ __half half_of_product(float w, __half v) {
    float p = w * __half2float(v);
    asm("" : "+v"(p));
    return __float2half(p);
}
template <uint32_t C>
__device__ __forceinline__ void corner_accumulate(__half acc[C], float w, const __half* __restrict__ g) {
    __half v[C];
    if constexpr (C == 2) {
        *reinterpret_cast<__half2*>(v) = *reinterpret_cast<const __half2*>(g);
    } else if constexpr (C == 4) {
        *reinterpret_cast<uint2*>(v) = *reinterpret_cast<const uint2*>(g);
    } else if constexpr (C == 8) {
        *reinterpret_cast<uint4*>(v) = *reinterpret_cast<const uint4*>(g);
    } else {
#pragma unroll
        for (uint32_t ch = 0; ch < C; ch++) v[ch] = g[ch];
    }
#pragma unroll
    for (uint32_t ch = 0; ch < C; ch++)
        acc[ch] = __float2half(__half2float(acc[ch]) + __half2float(half_of_product(w, v[ch])));
}

// The interpolation of one D = 3 cell from its eight rows v, corners in the reference's order 0 .. 7.  A row (RowT) is NW 32-bit words.
//   !HALF: every word is a float; out[NW] gets the reference's fmaf chains (gridencoder.cu:142,165 with scalar_t = float).
//   HALF:  every word is a half2; out[2 NW] gets the reference's half accumulator per channel -- every addend and every partial sum rounded to fp16
//          (scalar_t = at::Half).  The chain is the plain expression, not half_of_product(): here the compiler turns it into v_cvt_pk_f16_f32 +
//          v_pk_add_f16, which keeps the product's rounding to fp16 a step of its own -- the reference's two roundings -- while the empty statement
//          of half_of_product() would cost the packed forms (k_grid_fwd_d3c2<__half>: 584 -> 602 instructions).
//   OutT:  float (a half accumulator is upcast once, exact); a HALF caller that stores or merges halves may take the accumulator as it is (__half).
template <typename RowT, bool HALF, typename OutT>
__device__ __forceinline__ void cell_chain(const RowT (&v)[8], const float (&ws)[8], OutT* out /* [HALF ? 2 * NW : NW] */) {
    constexpr uint32_t NW = sizeof(RowT) / 4;
    if constexpr (!HALF) {
#pragma unroll
        for (uint32_t w = 0; w < NW; w++) out[w] = 0.0f;
#pragma unroll
        for (uint32_t idx = 0; idx < 8; idx++) {
            float fv[NW];
            __builtin_memcpy(fv, &v[idx], sizeof(fv));
#pragma unroll
            for (uint32_t w = 0; w < NW; w++) out[w] = fmaf(ws[idx], fv[w], out[w]);
        }
    } else {
        __half acc[2 * NW];
#pragma unroll
        for (uint32_t ch = 0; ch < 2 * NW; ch++) acc[ch] = __float2half(0.0f);
#pragma unroll
        for (uint32_t idx = 0; idx < 8; idx++) {
            __half hv[2 * NW];
            __builtin_memcpy(hv, &v[idx], sizeof(hv));
#pragma unroll
            for (uint32_t ch = 0; ch < 2 * NW; ch++)
                acc[ch] = __float2half(__half2float(acc[ch]) + __half2float(__float2half(ws[idx] * __half2float(hv[ch]))));
        }
#pragma unroll
        for (uint32_t ch = 0; ch < 2 * NW; ch++) {
            if constexpr (sizeof(OutT) == 2) out[ch] = acc[ch]; else out[ch] = __half2float(acc[ch]);
        }
    }
}

// One D = 3 cell: the eight gathers, the weights, the chain.  RowT = one table row (NW words: f32x2, f32x4 or NW x uint32 of half2), tab = the
// level's first row, idxs = corner_rows' indices, frac = grid_cell's fraction.
// The eight gathers go out first, back to back, and the weights are formed while they are in flight: every address exists before the first load
// and every load returns into registers of its own (load8_fresh, pnr_common.hpp), and nothing is scheduled across the end of the group.  Left to
// itself the compiler does this too -- until it is asked to keep the kernel within a register budget (amdgpu_waves_per_eu, which the frame loop's
// hosted tail needs): then it forms the weights first and threads the loads between the address arithmetic, and the frame loop's lego lookup
// launch takes 76 instead of 66 us with the very same instructions.  ORDERED = false (the hosted tail's own few rows): the compiler's order.
template <typename RowT, bool HALF, bool ORDERED, typename OutT>
__device__ __forceinline__ void cell_interp(const RowT* tab, const uint32_t (&idxs)[8], const float (&frac)[3], OutT* out /* [HALF ? 2 * NW : NW] */) {
    const RowT* p[8];
#pragma unroll
    for (int i = 0; i < 8; i++) p[i] = tab + idxs[i];
    RowT v[8];
    if constexpr (ORDERED) {
        load8_fresh(p, v);
    } else {
#pragma unroll
        for (int i = 0; i < 8; i++) v[i] = *p[i];
    }
    float ws[8];
    corner_weights<3>(frac, ws);
    cell_chain<RowT, HALF>(v, ws, out);
}

// 1 / v when v is a power of two (then x / v == x * (1 / v) bit for bit for every finite x that does not end subnormal), else 0: "divide"
static inline float exact_reciprocal_or_zero(float v) {
    int e2 = 0;
    const float mant = frexpf(v, &e2);
    return (mant == 0.5f && e2 > -100 && e2 < 100) ? 1.0f / v : 0.0f;
}

static inline LevelParams make_level_params(uint32_t L, float S, uint32_t H) {
    LevelParams lp;
    for (uint32_t l = 0; l < kMaxLevels; l++) { lp.scale[l] = 0; lp.resolution[l] = 0; }
    for (uint32_t l = 0; l < L; l++) {
        lp.scale[l] = exp2f((float)l * S) * (float)H - 1.0f;               // gridencoder.cu:125
        lp.resolution[l] = (uint32_t)ceil((double)lp.scale[l]) + 1;        // gridencoder.cu:126
    }
    return lp;
}

}  // namespace pnr
