// present.hip -- the viewer's step behind a frame (palette/utils.py:1106-1119 test_gui, palette/gui.py:225-231; nerf/utils.py has the same
// without the pick maps) as ONE launch: the rendered maps at rH x rW -> the display maps at H x W
//   image      F.interpolate(preds.clamp(0, 1), size=(H, W), mode='nearest') [, linear_to_srgb]
//   depth      F.interpolate(preds_depth, ...)
//   xyz        F.interpolate(rays_o + rays_d * depth_origin[..., None], ...)         (palette/utils.py:952; PaletteNeRF's point picking)
//   clip_feat  F.interpolate(clip_feat, ...)
//   accum      need_update ? image : (accum * spp + image) / (spp + 1)                 (gui.py:225-231, the still camera's running mean)
//              (a true fp32 division, as numpy's on the reference's host buffers -- torch on the device would multiply by the reciprocal of a scalar)
// The reference does this with a dozen torch launches and four permutes per frame, then moves every map to the host.  Every value is produced by
// the fp32 operations of those expressions in their order (the translation unit is built without contraction), so the maps are the bits torch
// gives -- the sRGB branch apart, whose powf is the device library's (as in pnr_image_to_uint8).
// Source pixel of a destination pixel: ATen's nearest_neighbor_compute_source_index, min((int)floorf(dst * scale), in - 1) per axis with
// scale = (float)in / out formed in fp32 (what F.interpolate(size=...) uses); in == out gives the identity.
#include "pnr_common.hpp"

namespace pnr {

constexpr uint32_t kPresentBlock = 256;

// LANES lanes per destination pixel: lanes 0..2 a colour / xyz channel each, lane 3 the depth, and every lane four floats of the clip_feat row per
// round (one 16-byte store).  RV = floats per load of the clip_feat row: 4 (16-byte aligned rows), 2 (8-byte: the row inside a PaletteNeRF aux map
// starts at column 6 + 7 nb) or 1 (anything else, any clip_dim)
template <uint32_t LANES, int RV>
__global__ void __launch_bounds__(kPresentBlock) k_present_frame(pnr_present_args a, float scale_y, float scale_x, int wide_store) {
    const uint32_t pix = (blockIdx.x * kPresentBlock + threadIdx.x) / LANES, q = threadIdx.x % LANES;
    if (pix >= a.dst_h * a.dst_w) return;
    const uint32_t y = pix / a.dst_w, x = pix - y * a.dst_w;
    const uint32_t sy = min((uint32_t)(int)floorf((float)y * scale_y), a.src_h - 1u);
    const uint32_t sx = min((uint32_t)(int)floorf((float)x * scale_x), a.src_w - 1u);
    const size_t s = (size_t)sy * a.src_w + sx;
    if (q < 3) {
        float v = a.image[s * 3 + q];
        v = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);   // torch.clamp(0, 1): a NaN stays a NaN
        if (a.linear_to_srgb) v = v < 0.0031308f ? 12.92f * v : 1.055f * powf(v, 0.41666f) - 0.055f;   // nerf/utils.py:43-44
        a.out_image[(size_t)pix * 3 + q] = v;
        if (a.accum) {
            float* acc = a.accum + (size_t)pix * 3 + q;
            *acc = a.spp == 0 ? v : (*acc * (float)a.spp + v) / (float)(a.spp + 1u);
        }
        if (a.out_xyz) a.out_xyz[(size_t)pix * 3 + q] = a.rays_o[s * 3 + q] + a.rays_d[s * 3 + q] * a.depth_origin[s];
    } else if (q == 3) {
        a.out_depth[pix] = a.depth[s];
    }
    if (a.out_clip) {
        const float* src = a.clip_feat + s * a.clip_stride;
        float* dst = a.out_clip + (size_t)pix * a.clip_dim;
        for (uint32_t c = q * 4; c < a.clip_dim; c += LANES * 4) {
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if constexpr (RV == 4) {
                v = *reinterpret_cast<const float4*>(src + c);
            } else if constexpr (RV == 2) {
                const float2 lo = *reinterpret_cast<const float2*>(src + c), hi = *reinterpret_cast<const float2*>(src + c + 2);
                v = make_float4(lo.x, lo.y, hi.x, hi.y);
            } else {
                v.x = src[c];
                if (c + 1 < a.clip_dim) v.y = src[c + 1];
                if (c + 2 < a.clip_dim) v.z = src[c + 2];
                if (c + 3 < a.clip_dim) v.w = src[c + 3];
            }
            if (wide_store) {
                *reinterpret_cast<float4*>(dst + c) = v;
            } else {
                dst[c] = v.x;
                if (c + 1 < a.clip_dim) dst[c + 1] = v.y;
                if (c + 2 < a.clip_dim) dst[c + 2] = v.z;
                if (c + 3 < a.clip_dim) dst[c + 3] = v.w;
            }
        }
    }
}

}  // namespace pnr

using namespace pnr;

extern "C" int pnr_present_frame(const pnr_present_args* args, pnr_stream_t stream) {
    if (!args) return PNR_ERR_INVALID;
    const pnr_present_args& a = *args;
    const uint64_t n_dst = (uint64_t)a.dst_h * a.dst_w;
    if (n_dst == 0) return PNR_OK;
    if (a.src_h == 0 || a.src_w == 0) return PNR_ERR_INVALID;
    if (!a.image || !a.depth || !a.out_image || !a.out_depth) return PNR_ERR_INVALID;
    if (a.out_xyz && (!a.rays_o || !a.rays_d || !a.depth_origin)) return PNR_ERR_INVALID;
    if (a.out_clip && (!a.clip_feat || a.clip_dim == 0 || a.clip_stride < a.clip_dim)) return PNR_ERR_INVALID;
    if (n_dst * 8 > 0xffffffffull || (uint64_t)a.src_h * a.src_w > 0xffffffffull) return PNR_ERR_UNSUPPORTED;
    const float scale_y = (float)a.src_h / (float)a.dst_h, scale_x = (float)a.src_w / (float)a.dst_w;
    hipStream_t s = as_stream(stream);
    if (!a.out_clip) {
        hipLaunchKernelGGL((k_present_frame<4, 1>), dim3(cdiv((uint32_t)n_dst * 4, kPresentBlock)), dim3(kPresentBlock), 0, s, a, scale_y, scale_x, 0);
        return check_launch();
    }
    const uintptr_t src = reinterpret_cast<uintptr_t>(a.clip_feat);
    const bool quads = (a.clip_dim & 3u) == 0;
    const int rv = (quads && (src & 15u) == 0 && (a.clip_stride & 3u) == 0) ? 4 : ((quads && (src & 7u) == 0 && (a.clip_stride & 1u) == 0) ? 2 : 1);
    const int wide_store = (quads && (reinterpret_cast<uintptr_t>(a.out_clip) & 15u) == 0) ? 1 : 0;
    const dim3 grid(cdiv((uint32_t)n_dst * 8, kPresentBlock)), block(kPresentBlock);
    const auto kernel = rv == 4 ? k_present_frame<8, 4> : (rv == 2 ? k_present_frame<8, 2> : k_present_frame<8, 1>);   // floats per read of a feature row
    hipLaunchKernelGGL(kernel, grid, block, 0, s, a, scale_y, scale_x, wide_store);
    return check_launch();
}
