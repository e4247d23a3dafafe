// image_core.hpp -- reading a pixel of a ground-truth stack (fp32 / fp16 / uint8, 3 or 4 channels) and the sRGB -> linear curve: one statement for
// train_batch.hip (the training batch) and extract.hip (the palette extraction's histograms), so that the two agree bit for bit.
#pragma once
#include "pnr_common.hpp"

namespace pnr {

// one pixel of C channels as fp32: fp32 as stored, fp16 converted exactly, uint8 as the loader's astype(float32) / 255.
// vec: the stack's base allows one request per RGBA pixel (16 / 8 / 4 bytes).
template <int FMT, int C>
__device__ __forceinline__ void load_pixel(const void* __restrict__ images, uint64_t pix, bool vec, float (&px)[4]) {
    if (FMT == PNR_IMAGE_FP32) {
        const float* s = reinterpret_cast<const float*>(images) + pix * C;
        if (C == 4 && vec) {
            const float4 q = *reinterpret_cast<const float4*>(s);
            px[0] = q.x; px[1] = q.y; px[2] = q.z; px[3] = q.w;
        } else {
#pragma unroll
            for (int c = 0; c < C; c++) px[c] = s[c];
        }
    } else if (FMT == PNR_IMAGE_FP16) {
        const __half* s = reinterpret_cast<const __half*>(images) + pix * C;
        if (C == 4 && vec) {
            const uint2 q = *reinterpret_cast<const uint2*>(s);
#pragma unroll
            for (int c = 0; c < 4; c++) px[c] = __half2float(__ushort_as_half((unsigned short)(((c < 2 ? q.x : q.y) >> (16 * (c & 1))) & 0xffffu)));
        } else {
#pragma unroll
            for (int c = 0; c < C; c++) px[c] = __half2float(s[c]);
        }
    } else {
        const uint8_t* s = reinterpret_cast<const uint8_t*>(images) + pix * C;
        if (C == 4 && vec) {
            const uint32_t q = *reinterpret_cast<const uint32_t*>(s);
#pragma unroll
            for (int c = 0; c < 4; c++) px[c] = (float)((q >> (8 * c)) & 0xffu) / 255.0f;
        } else {
#pragma unroll
            for (int c = 0; c < C; c++) px[c] = (float)s[c] / 255.0f;
        }
    }
}

// srgb_to_linear (nerf/utils.py:48-49)
__device__ __forceinline__ float srgb_to_linear(float x) { return x < 0.04045f ? x / 12.92f : powf((x + 0.055f) / 1.055f, 2.4f); }

}  // namespace pnr
