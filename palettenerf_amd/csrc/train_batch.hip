// train_batch.hip -- what a training step does in front of model.render, on the device (include/pnr.h, "training batches"):
//   pnr_train_batch       collate (palette/provider.py:356-410) + train_step's head (palette/utils.py:450-478): rays, pixel gather,
//                         srgb_to_linear, alpha blend over the background, palette-weight guide, feature gather -- one launch, one lane per ray
//   pnr_error_map_update  the error map's EMA scatter (palette/utils.py:578-599) -- one launch
// At 4 096 rays both are latency, not bandwidth: one lane per ray, no LDS, the 0.5-1 MB guide table is read through L2.
// Built with -ffp-contract=off like every unit: a * b + c below is two roundings, which is what torch's separate kernels give.
#include "pnr_common.hpp"
#include "ray_core.hpp"
#include "image_core.hpp"

namespace pnr {
namespace {

constexpr uint32_t kBatchBlock = 256;

__device__ __forceinline__ long long clamp_index(long long i, long long n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

template <int FMT, int C>
__global__ void __launch_bounds__(kBatchBlock) k_train_batch(const pnr_train_batch_args a, const int vec) {
    const uint64_t r = (uint64_t)blockIdx.x * kBatchBlock + threadIdx.x;
    if (r >= (uint64_t)a.B * a.N) return;
    const uint64_t HW = (uint64_t)a.H * a.W;
    const uint64_t v = (uint64_t)clamp_index(a.view_index[r / a.N], (long long)a.V);      // a bad index is the caller's error: read inside the stack anyway
    const uint64_t p = (uint64_t)clamp_index(a.inds[r], (long long)HW);
    const uint64_t pix = v * HW + p;

    if (a.rays_o) pinhole_ray(a.poses, v, (uint32_t)p, a.W, a.fx, a.fy, a.cx, a.cy, a.rays_o, a.rays_d, r);

    if (a.gt_clip) {
        float* dst = a.gt_clip + r * a.D;
        if (a.feat_format == PNR_IMAGE_FP32) {
            const float* s = reinterpret_cast<const float*>(a.feat_images) + pix * a.D;
            for (uint32_t c = 0; c < a.D; c++) dst[c] = s[c];
        } else {
            const __half* s = reinterpret_cast<const __half*>(a.feat_images) + pix * a.D;
            for (uint32_t c = 0; c < a.D; c++) dst[c] = __half2float(s[c]);
        }
    }

    if (!a.pixels && !a.gt_rgb && !a.gt_weights) return;
    float px[4];
    load_pixel<FMT, C>(a.images, pix, vec != 0, px);
    if (a.pixels) {
#pragma unroll
        for (int c = 0; c < C; c++) a.pixels[r * C + c] = px[c];
    }
    if (!a.gt_rgb && !a.gt_weights) return;

    float g[3];
#pragma unroll 1
    for (int c = 0; c < 3; c++) {      // (rolled: one copy of powf)
        float x = px[c];
        if (a.srgb_to_linear) x = srgb_to_linear(x);
        if (C == 4) {
            const float bg = a.bg_mode == 0 ? a.bg_const : (a.bg_mode == 1 ? a.bg_color[c] : a.bg_color[r * 3 + c]);
            x = x * px[3] + bg * (1.0f - px[3]);                                                    // palette/utils.py:471
        }
        g[c] = x;
    }
    if (a.gt_rgb) { a.gt_rgb[r * 3 + 0] = g[0]; a.gt_rgb[r * 3 + 1] = g[1]; a.gt_rgb[r * 3 + 2] = g[2]; }
    if (!a.gt_weights) return;

    // get_palette_weight_with_hist (palette/utils.py:117-124): hist[k, r, g, b] trilinear at c (S - 1), a corner outside [0, S) counts as zero
    const uint32_t S[3] = {a.Sr, a.Sg, a.Sb};
    int i0[3];
    float w0[3], w1[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float x = g[c] * (float)(S[c] - 1);
        x = fminf(fmaxf(x, -2.0f), (float)S[c] + 1.0f);        // keeps the int conversion defined; every such corner is outside the table (NaN -> -2)
        const float fl = floorf(x);
        i0[c] = (int)fl;
        w1[c] = x - fl;
        w0[c] = (fl + 1.0f) - x;
    }
    uint64_t off[8];
    float wt[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {      // grid_sample's corner order: b fastest, then g, then r
        const int db = j & 1, dg = (j >> 1) & 1, dr = j >> 2;
        const int ir = i0[0] + dr, ig = i0[1] + dg, ib = i0[2] + db;
        const bool in = ir >= 0 && ir < (int)S[0] && ig >= 0 && ig < (int)S[1] && ib >= 0 && ib < (int)S[2];
        off[j] = in ? (uint64_t)ir * a.hist_stride[1] + (uint64_t)ig * a.hist_stride[2] + (uint64_t)ib * a.hist_stride[3] : 0;
        wt[j] = in ? ((db ? w1[2] : w0[2]) * (dg ? w1[1] : w0[1])) * (dr ? w1[0] : w0[0]) : 0.0f;
    }
    for (uint32_t k = 0; k < a.num_basis; k++) {
        const float* h = a.hist_weights + k * a.hist_stride[0];
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; j++) acc = acc + h[off[j]] * wt[j];
        a.gt_weights[r * a.num_basis + k] = acc;
    }
}

__global__ void __launch_bounds__(kBatchBlock) k_error_map_update(float* __restrict__ error_map, uint32_t cells, const long long* __restrict__ view_index,
                                                                   const long long* __restrict__ inds_coarse, const float* __restrict__ loss_ray,
                                                                   uint32_t B, uint32_t N) {
    const uint64_t r = (uint64_t)blockIdx.x * kBatchBlock + threadIdx.x;
    if (r >= (uint64_t)B * N) return;
    const long long v = view_index[r / N];
    const uint64_t c = (uint64_t)clamp_index(inds_coarse[r], (long long)cells);
    float* m = error_map + (uint64_t)(v < 0 ? 0 : v) * cells + c;
    *m = 0.1f * *m + 0.9f * loss_ray[r];                                                            // palette/utils.py:595-596
}

typedef decltype(&k_train_batch<PNR_IMAGE_FP32, 3>) TrainBatchKernel;
TrainBatchKernel train_batch_kernel(int image_format, uint32_t C) {   // [image format][C == 4]; both validated (or defaulted) by the caller
#define ROW(FMT) {k_train_batch<FMT, 3>, k_train_batch<FMT, 4>}
    static const TrainBatchKernel table[3][2] = {ROW(PNR_IMAGE_FP32), ROW(PNR_IMAGE_FP16), ROW(PNR_IMAGE_UINT8)};
#undef ROW
    return table[image_format == PNR_IMAGE_FP32 ? 0 : image_format == PNR_IMAGE_FP16 ? 1 : 2][C == 4];
}

}  // namespace
}  // namespace pnr

using namespace pnr;

extern "C" {

int pnr_train_batch(const pnr_train_batch_args* args, pnr_stream_t stream) {
    if (!args) return PNR_ERR_INVALID;
    pnr_train_batch_args a = *args;
    const uint64_t rays = (uint64_t)a.B * a.N;
    if (rays == 0) return PNR_OK;
    if (!a.view_index || !a.inds || a.V == 0 || a.H == 0 || a.W == 0) return PNR_ERR_INVALID;
    if ((uint64_t)a.H * a.W > 0xffffffffull) return PNR_ERR_UNSUPPORTED;
    const uint64_t blocks = (rays + kBatchBlock - 1) / kBatchBlock;
    if (blocks > 0x7fffffffull) return PNR_ERR_UNSUPPORTED;
    if ((a.rays_o == nullptr) != (a.rays_d == nullptr)) return PNR_ERR_INVALID;
    if (a.rays_o && (!a.poses || a.fx == 0.0f || a.fy == 0.0f)) return PNR_ERR_INVALID;
    const bool colour = a.gt_rgb || a.gt_weights;
    if (a.pixels || colour) {
        if (!a.images || (a.C != 3 && a.C != 4)) return PNR_ERR_INVALID;
        if (a.image_format != PNR_IMAGE_FP32 && a.image_format != PNR_IMAGE_FP16 && a.image_format != PNR_IMAGE_UINT8) return PNR_ERR_UNSUPPORTED;
    } else {
        a.C = 3;
        a.image_format = PNR_IMAGE_FP32;
    }
    if (colour && a.C == 4) {
        if (a.bg_mode < 0 || a.bg_mode > 2 || (a.bg_mode != 0 && !a.bg_color)) return PNR_ERR_INVALID;
    }
    if (a.gt_weights) {
        if (!a.hist_weights || a.Sr == 0 || a.Sg == 0 || a.Sb == 0 || a.Sr > 1024 || a.Sg > 1024 || a.Sb > 1024) return PNR_ERR_INVALID;
        if (a.num_basis == 0 || a.num_basis > PNR_MAX_BASIS) return PNR_ERR_UNSUPPORTED;
        if (!(a.hist_stride[0] | a.hist_stride[1] | a.hist_stride[2] | a.hist_stride[3])) {
            a.hist_stride[3] = 1;
            a.hist_stride[2] = a.Sb;
            a.hist_stride[1] = (uint64_t)a.Sg * a.Sb;
            a.hist_stride[0] = (uint64_t)a.Sr * a.Sg * a.Sb;
        }
    }
    if (a.gt_clip) {
        if (!a.feat_images || a.D == 0) return PNR_ERR_INVALID;
        if (a.feat_format != PNR_IMAGE_FP32 && a.feat_format != PNR_IMAGE_FP16) return PNR_ERR_UNSUPPORTED;
    }
    if (!a.rays_o && !a.gt_clip && !a.pixels && !colour) return PNR_OK;
    const uintptr_t base = reinterpret_cast<uintptr_t>(a.images);
    const int vec = a.image_format == PNR_IMAGE_FP32 ? (base & 15u) == 0 : (a.image_format == PNR_IMAGE_FP16 ? (base & 7u) == 0 : (base & 3u) == 0);
    hipLaunchKernelGGL(train_batch_kernel(a.image_format, a.C), dim3((uint32_t)blocks), dim3(kBatchBlock), 0, as_stream(stream), a, vec);
    return check_launch();
}

int pnr_error_map_update(float* error_map, uint32_t cells, const int64_t* view_index, const int64_t* inds_coarse, const float* loss_ray, uint32_t B,
                         uint32_t N, pnr_stream_t stream) {
    const uint64_t rays = (uint64_t)B * N;
    if (rays == 0) return PNR_OK;
    if (!error_map || !view_index || !inds_coarse || !loss_ray || cells == 0) return PNR_ERR_INVALID;
    const uint64_t blocks = (rays + kBatchBlock - 1) / kBatchBlock;
    if (blocks > 0x7fffffffull) return PNR_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_error_map_update, dim3((uint32_t)blocks), dim3(kBatchBlock), 0, as_stream(stream), error_map, cells,
                       reinterpret_cast<const long long*>(view_index), reinterpret_cast<const long long*>(inds_coarse), loss_ray, B, N);
    return check_launch();
}

}  // extern "C"
