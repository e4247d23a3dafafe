// evaluate.hip -- what a user does with a trained model, on the device: the uint8 images of PaletteTrainer.test / evaluate_one_epoch
// (palette/utils.py:993-1038, :852-909) and the meters of evaluate_one_epoch (nerf/utils.py:220-330, palette/utils.py:52-114, eval_step :610-638).
// The reference moves ~23 fp32 values per pixel to the host for this (every map through .cpu().numpy()) and needs kornia for SSIM; here a frame
// leaves the device as bytes plus eight doubles of totals read once per epoch, with two launches behind the frame call:
//   k_palette_sheets   all nine images of a frame in one launch, ray-major: a workgroup takes 256 consecutive rays, reads their rows of every map ONCE
//                      (the aux columns are strided views of one row per ray: an image-major pass would fetch every row once per image), keeps one
//                      byte per value in LDS and writes each image's bytes of the chunk as dwords where the address allows, single bytes at ragged
//                      run ends.  ~74 MB of traffic at 800 x 800, nb = 4.
//   k_frame_metrics    MSE / PSNR / SSIM / Sparsity / TV of one view in one launch: a workgroup stages a 32 x 32 tile with SSIM's 5-pixel halo
//                      (prediction as fp32, ground truth as double) in LDS -- the interior pixels give the MSE, Sparsity and TV terms on the way --
//                      then filters separably per channel (rows into LDS, then columns) and forms the SSIM ratio last.  Everything after the fp32
//                      inputs is double: the E[p^2] - mu^2 form loses most of its fp32 bits on flat regions (results log).
//                      Sums: lane -> wave butterfly -> workgroup -> one row of partials per workgroup; the last workgroup (agent-scope ticket, as
//                      in train_loss.hip) adds the rows by index and updates the totals.  A fixed order: two runs give the same bits.
#include <math.h>
#include "pnr_common.hpp"

namespace pnr {

// ------------------------------------------------------------------------------------------------ sheets
constexpr uint32_t kSheetBlock = 256, kSheetRays = 256, kSheetMaps = 8;
enum : uint32_t { kSheetPix3 = 0, kSheetDepth = 1, kSheetBasis3 = 2, kSheetBasis1 = 3 };
constexpr uint32_t kSwatch = 100;   // palette/utils.py:1019: basis_color[i, None, None, :].repeat(100, 100, 1)
constexpr uint32_t kSheetLds = kSheetRays * (10 + 8 * PNR_SHEET_MAX_BASIS);   // one byte per input value of a chunk: 18 944

struct SheetMap {
    const float* src;
    uint8_t* dst;
    uint32_t stride, cols, kind, lds_base;   // lds_base: where the chunk's [rays][cols] bytes of this map start
    int srgb;
};
struct SheetPlan {
    SheetMap m[kSheetMaps];
    uint32_t count, n_rays, W, nb, chunks;
    const float* palette;   // [nb,3] or NULL
    uint8_t* swatch;        // [100, 100 nb, 3]
};

__device__ __forceinline__ uint8_t sheet_byte(float v, bool clip, int srgb) {
    if (srgb) v = v < 0.0031308f ? 12.92f * v : 1.055f * powf(v, 0.41666f) - 0.055f;   // nerf/utils.py:43-44, as k_image_to_uint8
    if (clip) v = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);                              // np.clip(0, 1); the depth has none (palette/utils.py:1002)
    return (uint8_t)(int)(v * 255.0f);
}

// `len` consecutive output bytes at dst, byte k = byte_at(k), by the whole workgroup: dwords where dst + k is on a dword boundary, single bytes at the
// ragged head and tail (W 3 and nb W are in general no multiples of four, so a run of a per-basis image starts anywhere)
template <typename F>
__device__ __forceinline__ void sheet_run(uint8_t* dst, uint32_t len, F byte_at) {
    const uint32_t head = min(len, (uint32_t)(-(intptr_t)reinterpret_cast<uintptr_t>(dst)) & 3u);
    const uint32_t nd = (len - head) >> 2, tail = len - head - 4u * nd;
    for (uint32_t u = threadIdx.x; u < nd; u += kSheetBlock) {
        const uint32_t k = head + 4u * u;
        *reinterpret_cast<uint32_t*>(dst + k) = (uint32_t)byte_at(k) | ((uint32_t)byte_at(k + 1) << 8) | ((uint32_t)byte_at(k + 2) << 16) | ((uint32_t)byte_at(k + 3) << 24);
    }
    if (threadIdx.x < head) dst[threadIdx.x] = byte_at(threadIdx.x);
    if (threadIdx.x < tail) { const uint32_t k = head + 4u * nd + threadIdx.x; dst[k] = byte_at(k); }
}

__global__ void __launch_bounds__(kSheetBlock) k_palette_sheets(SheetPlan p) {
    __shared__ uint8_t stage[kSheetLds];
    if (blockIdx.x >= p.chunks) {   // the swatch strip: no rays behind it
        const uint32_t n = kSwatch * kSwatch * 3u * p.nb, rowb = p.nb * kSwatch * 3u;
        const uint32_t head = (uint32_t)(-(intptr_t)reinterpret_cast<uintptr_t>(p.swatch)) & 3u;
        const int64_t start = (head ? (int64_t)head - 4 : 0) + 4 * (int64_t)((blockIdx.x - p.chunks) * kSheetBlock + threadIdx.x);
        auto at = [&](uint32_t j) { const uint32_t r = j % rowb; return sheet_byte(p.palette[(r / (kSwatch * 3u)) * 3u + r % 3u], true, 0); };
        if (start >= 0 && start + 4 <= (int64_t)n) {
            const uint32_t j = (uint32_t)start;
            *reinterpret_cast<uint32_t*>(p.swatch + j) = (uint32_t)at(j) | ((uint32_t)at(j + 1) << 8) | ((uint32_t)at(j + 2) << 16) | ((uint32_t)at(j + 3) << 24);
        } else {
            for (int k = 0; k < 4; k++)
                if (start + k >= 0 && start + k < (int64_t)n) p.swatch[start + k] = at((uint32_t)(start + k));
        }
        return;
    }
    // ---- the chunk's rows of every map, read once (a row's columns by adjacent lanes), one byte per value into LDS
    const uint32_t ray0 = blockIdx.x * kSheetRays, rc = min(kSheetRays, p.n_rays - ray0);
    for (uint32_t mi = 0; mi < p.count; mi++) {
        const SheetMap& m = p.m[mi];
        const uint32_t total = rc * m.cols;
        const bool clip = m.kind != kSheetDepth;
        for (uint32_t e = threadIdx.x; e < total; e += kSheetBlock) {
            const uint32_t r = e / m.cols, c = e - r * m.cols;
            stage[m.lds_base + e] = sheet_byte(m.src[(size_t)(ray0 + r) * m.stride + c], clip, m.srgb);
        }
    }
    __syncthreads();
    // ---- the chunk's bytes of every image: [H,W,3] / [H,W] images are one run; a per-basis image has one run per basis and image row
    for (uint32_t mi = 0; mi < p.count; mi++) {
        const SheetMap& m = p.m[mi];
        const uint8_t* lds = stage + m.lds_base;
        if (m.kind == kSheetPix3) {
            sheet_run(m.dst + (size_t)ray0 * 3u, rc * 3u, [&](uint32_t k) { return lds[k]; });
        } else if (m.kind == kSheetDepth) {
            sheet_run(m.dst + ray0, rc, [&](uint32_t k) { return lds[k]; });
        } else {
            const uint32_t px = m.kind == kSheetBasis3 ? 3u : 1u, W = p.W, nb = p.nb;
            for (uint32_t y = ray0 / W; y <= (ray0 + rc - 1u) / W; y++) {
                const uint32_t ra = max(ray0, y * W), rb = min(ray0 + rc, (y + 1u) * W), xa = ra - y * W, first = ra - ray0;
                for (uint32_t i = 0; i < nb; i++) {
                    uint8_t* dst = m.dst + ((size_t)y * nb * W + (size_t)i * W + xa) * px;
                    if (px == 3u)
                        sheet_run(dst, (rb - ra) * 3u, [&](uint32_t k) { const uint32_t q = k / 3u; return lds[(first + q) * m.cols + 3u * i + (k - 3u * q)]; });
                    else
                        sheet_run(dst, rb - ra, [&](uint32_t k) { return lds[(first + k) * m.cols + i]; });
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ meters
constexpr int kMetTile = 32, kMetHalo = 5, kMetSpan = kMetTile + 2 * kMetHalo, kMetTaps = 2 * kMetHalo + 1;
constexpr uint32_t kMetBlock = 256, kMetHdr = 64, kMetSums = 5, kMetRow = 8;   // sums: squared error, SSIM term, sparsity, TV along x, TV along y
constexpr uint32_t kMetLdsT = 3 * kMetSpan * kMetSpan * sizeof(double);         // ground truth tile
constexpr uint32_t kMetLdsR = 5 * kMetSpan * kMetTile * sizeof(double);         // row-filtered sums of one channel
constexpr uint32_t kMetLdsP = 3 * kMetSpan * kMetSpan * sizeof(float);          // prediction tile
constexpr uint32_t kMetLds = kMetLdsT + kMetLdsR + kMetLdsP;                    // 117 264 bytes of the 160 KB

// exp(-(k - 5)^2 / (2 * 1.5^2)) / their sum, k = 0 .. 10, rounded to double: the normalised 11-tap Gaussian of sigma 1.5
__device__ constexpr double kMetGauss[kMetTaps] = {0.00102838008447911, 0.007598758135239185, 0.03600077212843083, 0.10936068950970002,
                                                   0.2130055377112537,  0.26601172486179436,  0.2130055377112537,  0.10936068950970002,
                                                   0.03600077212843083, 0.007598758135239185, 0.00102838008447911};

struct MetricsLaunch {
    pnr_metrics_args a;
    uint32_t tiles_x;
};

// nerf/utils.py:48-49 in double; kept out of line: pow's constants would otherwise crowd the scalar registers of the tile loop
__device__ __attribute__((noinline)) double srgb_to_linear_d(double x) { return x < 0.04045 ? x / 12.92 : pow((x + 0.055) / 1.055, 2.4); }

// thread 0 of the workgroup returns with the sums of all 256 lanes in v (waves by butterfly, then the four waves in order)
__device__ __forceinline__ void block_sum(double (&v)[kMetSums], double (*red)[kMetSums]) {
#pragma unroll
    for (uint32_t q = 0; q < kMetSums; q++)
#pragma unroll
        for (int off = PNR_WAVE / 2; off > 0; off >>= 1) v[q] += __shfl_xor(v[q], off, PNR_WAVE);
    __syncthreads();   // red may still be read from an earlier call
    if ((threadIdx.x & (PNR_WAVE - 1)) == 0)
        for (uint32_t q = 0; q < kMetSums; q++) red[threadIdx.x / PNR_WAVE][q] = v[q];
    __syncthreads();
    if (threadIdx.x == 0)
        for (uint32_t q = 0; q < kMetSums; q++) v[q] = ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q];
}

__global__ void __launch_bounds__(kMetBlock) k_frame_metrics(MetricsLaunch L) {
    extern __shared__ double met_lds[];
    __shared__ double red[kMetBlock / PNR_WAVE][kMetSums];
    __shared__ uint32_t is_last;
    const pnr_metrics_args& a = L.a;
    double* T = met_lds;                                               // [3][span][span]
    double* R = met_lds + 3 * kMetSpan * kMetSpan;                     // [5][span][tile]
    float* P = reinterpret_cast<float*>(R + 5 * kMetSpan * kMetTile);  // [3][span][span]
    const int H = (int)a.H, W = (int)a.W;
    const int x0 = (int)(blockIdx.x % L.tiles_x) * kMetTile, y0 = (int)(blockIdx.x / L.tiles_x) * kMetTile;
    const bool ssim = (a.want & PNR_METRIC_SSIM) != 0;
    const bool mse = (a.want & (PNR_METRIC_MSE | PNR_METRIC_PSNR)) != 0;
    const bool sparsity = a.basis_acc && (a.want & PNR_METRIC_SPARSITY), tv = a.basis_acc && (a.want & PNR_METRIC_TV);
    const uint32_t C = a.truth_channels, nb = a.num_basis;
    double sum[kMetSums] = {0.0, 0.0, 0.0, 0.0, 0.0};

    // ---- the tile with its halo; the interior pixels also give the per-pixel terms of the other meters
    for (int idx = (int)threadIdx.x; idx < kMetSpan * kMetSpan; idx += (int)kMetBlock) {
        const int ty = idx / kMetSpan, tx = idx - ty * kMetSpan;
        const int y = y0 + ty - kMetHalo, x = x0 + tx - kMetHalo;
        const bool interior = ty >= kMetHalo && ty < kMetHalo + kMetTile && tx >= kMetHalo && tx < kMetHalo + kMetTile && y < H && x < W;
        if (!ssim && !interior) continue;
        const int yr = y < 0 ? -y : (y >= H ? 2 * H - 2 - y : y), xr = x < 0 ? -x : (x >= W ? 2 * W - 2 - x : x);   // torch 'reflect'
        float p[3] = {0.0f, 0.0f, 0.0f};
        double t[3] = {0.0, 0.0, 0.0};
        if (yr >= 0 && yr < H && xr >= 0 && xr < W) {   // (positions further than the halo past the image are never used)
            const size_t ray = (size_t)yr * (size_t)W + (size_t)xr;
            const float* ps = a.pred + ray * a.pred_stride;
            const float* ts = a.truth + ray * C;
            p[0] = ps[0]; p[1] = ps[1]; p[2] = ps[2];
            t[0] = (double)ts[0]; t[1] = (double)ts[1]; t[2] = (double)ts[2];
            if (a.srgb_to_linear_truth)
#pragma unroll 1
                for (int c = 0; c < 3; c++) t[c] = srgb_to_linear_d(t[c]);
            if (C == 4) {
                const double al = (double)ts[3];
#pragma unroll
                for (int c = 0; c < 3; c++) t[c] = t[c] * al + (1.0 - al);   // palette/utils.py:623 with bg_color = 1
            }
            if (interior) {
                if (a.truth_rgb_out) {
                    float* o = a.truth_rgb_out + ray * 3;
                    o[0] = (float)t[0]; o[1] = (float)t[1]; o[2] = (float)t[2];
                }
                if (mse)
#pragma unroll
                    for (int c = 0; c < 3; c++) { const double d = (double)p[c] - t[c]; sum[0] = fma(d, d, sum[0]); }
                if (sparsity || tv) {
                    const float* w = a.basis_acc + ray * a.basis_acc_stride;
                    const float* wx = x + 1 < W ? w + a.basis_acc_stride : nullptr;
                    const float* wy = y + 1 < H ? w + (size_t)W * a.basis_acc_stride : nullptr;
                    double s1 = 0.0, s2 = 0.0;
                    for (uint32_t i = 0; i < nb; i++) {
                        const double wi = (double)w[i];
                        s1 += wi;
                        s2 = fma(wi, wi, s2);
                        if (tv && wx) { const double d = wi - (double)wx[i]; sum[3] = fma(d, d, sum[3]); }
                        if (tv && wy) { const double d = wi - (double)wy[i]; sum[4] = fma(d, d, sum[4]); }
                    }
                    if (sparsity) sum[2] += s1 / (s2 + 1e-6) - 1.0;   // palette/utils.py:69
                }
            }
        }
        if (ssim) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                P[(c * kMetSpan + ty) * kMetSpan + tx] = p[c];
                T[(c * kMetSpan + ty) * kMetSpan + tx] = t[c];
            }
        }
    }

    if (ssim) {
        const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
        double gv[kMetHalo + 1];   // the taps in vector registers (there are plenty: LDS allows one workgroup per CU), as literals they crowd the scalar file
#pragma unroll
        for (int k = 0; k <= kMetHalo; k++) { gv[k] = kMetGauss[k]; asm volatile("" : "+v"(gv[k])); }
        for (int c = 0; c < 3; c++) {
            __syncthreads();   // the tile is complete / the previous channel's columns are done with R
            for (int idx = (int)threadIdx.x; idx < kMetSpan * kMetTile; idx += (int)kMetBlock) {
                const int r = idx / kMetTile, x = idx - r * kMetTile;
                const float* pr = P + (c * kMetSpan + r) * kMetSpan + x;
                const double* tr = T + (c * kMetSpan + r) * kMetSpan + x;
                double m1 = 0.0, m2 = 0.0, e11 = 0.0, e22 = 0.0, e12 = 0.0;
#pragma unroll
                for (int k = 0; k < kMetTaps; k++) {
                    const double g = gv[k <= kMetHalo ? k : 2 * kMetHalo - k], pv = (double)pr[k], tv_ = tr[k];
                    const double gp = g * pv, gt = g * tv_;
                    m1 += gp; m2 += gt;
                    e11 = fma(gp, pv, e11); e22 = fma(gt, tv_, e22); e12 = fma(gp, tv_, e12);
                }
                R[(0 * kMetSpan + r) * kMetTile + x] = m1;
                R[(1 * kMetSpan + r) * kMetTile + x] = m2;
                R[(2 * kMetSpan + r) * kMetTile + x] = e11;
                R[(3 * kMetSpan + r) * kMetTile + x] = e22;
                R[(4 * kMetSpan + r) * kMetTile + x] = e12;
            }
            __syncthreads();
            for (int idx = (int)threadIdx.x; idx < kMetTile * kMetTile; idx += (int)kMetBlock) {
                const int y = idx / kMetTile, x = idx - y * kMetTile;
                if (y0 + y >= H || x0 + x >= W) continue;
                double q[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int k = 0; k < kMetTaps; k++) {
                    const double g = gv[k <= kMetHalo ? k : 2 * kMetHalo - k];
#pragma unroll
                    for (int v = 0; v < 5; v++) q[v] = fma(g, R[(v * kMetSpan + y + k) * kMetTile + x], q[v]);
                }
                const double m1 = q[0], m2 = q[1];
                const double s1 = q[2] - m1 * m1, s2 = q[3] - m2 * m2, s12 = q[4] - m1 * m2;
                const double S = ((2.0 * m1 * m2 + C1) * (2.0 * s12 + C2)) / ((m1 * m1 + m2 * m2 + C1) * (s1 + s2 + C2) + 1e-12);
                const double term = (1.0 - S) / 2.0;
                sum[1] += term < 0.0 ? 0.0 : (term > 1.0 ? 1.0 : term);
            }
        }
    }

    // ---- workgroup -> partial row -> the last workgroup adds the rows by index
    uint32_t* ticket = reinterpret_cast<uint32_t*>(a.workspace);
    double* partials = reinterpret_cast<double*>(reinterpret_cast<char*>(a.workspace) + kMetHdr);
    block_sum(sum, red);
    if (threadIdx.x == 0) {
        for (uint32_t q = 0; q < kMetSums; q++) partials[(size_t)blockIdx.x * kMetRow + q] = sum[q];
        __threadfence();   // the row is out at agent scope before this workgroup takes its ticket
        is_last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1 ? 1u : 0u;
    }
    __syncthreads();
    if (!is_last) return;
    __threadfence();       // every lane of the last workgroup reads the other workgroups' rows behind the ticket
    for (uint32_t q = 0; q < kMetSums; q++) sum[q] = 0.0;
    for (uint32_t b = threadIdx.x; b < gridDim.x; b += kMetBlock)
        for (uint32_t q = 0; q < kMetSums; q++) sum[q] += partials[(size_t)b * kMetRow + q];
    block_sum(sum, red);
    if (threadIdx.x == 0) {
        const double n1 = (double)a.H * (double)a.W, n3 = 3.0 * n1;
        double f[8] = {1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        const double m = sum[0] / n3;
        if (mse) f[1] = m;
        if (a.want & PNR_METRIC_PSNR) f[2] = -10.0 * log10(m);                       // nerf/utils.py:242
        if (ssim) f[3] = 1.0 - 2.0 * (sum[1] / n3);                                 // nerf/utils.py:317-318
        if (sparsity) f[4] = sum[2] / n1;
        if (tv) f[5] = 100.0 * (sum[3] / ((double)a.H * (double)(a.W - 1u) * (double)nb) + sum[4] / ((double)(a.H - 1u) * (double)a.W * (double)nb));
        for (int k = 0; k < 8; k++) {
            a.totals[k] += f[k];
            if (a.frame_out) a.frame_out[k] = f[k];
        }
        *ticket = 0u;      // ready for the next launch on this workspace (kernel boundaries order it)
    }
}

}  // namespace pnr

using namespace pnr;

extern "C" {

int pnr_palette_sheets(const pnr_sheet_args* args, pnr_stream_t stream) {
    if (!args) return PNR_ERR_INVALID;
    const pnr_sheet_args& a = *args;
    const uint64_t n = (uint64_t)a.H * a.W;
    if (n == 0) return PNR_OK;
    if (!a.image || !a.depth || a.image_stride < 3 || a.depth_stride < 1) return PNR_ERR_INVALID;
    const uint32_t nb = a.num_basis;
    const bool per_basis = a.basis_rgb || a.unscaled_basis_rgb || a.basis_acc || a.gt_weights || a.basis_color || a.out_basis_img ||
                           a.out_unscaled_basis_img || a.out_basis_acc || a.out_weights_guide || a.out_basis_color;
    if (nb > PNR_SHEET_MAX_BASIS || (nb == 0 && per_basis)) return PNR_ERR_INVALID;
    if ((a.out_view_dep && !a.view_dep_rgb) || (a.out_direct && !a.direct_rgb) || (a.out_basis_img && !a.basis_rgb) ||
        (a.out_unscaled_basis_img && !a.unscaled_basis_rgb) || (a.out_basis_acc && !a.basis_acc) || (a.out_weights_guide && !a.gt_weights) ||
        (a.out_basis_color && !a.basis_color))
        return PNR_ERR_INVALID;
    if ((a.view_dep_rgb && a.view_dep_stride < 3) || (a.direct_rgb && a.direct_stride < 3) || (a.basis_rgb && a.basis_rgb_stride < 3 * nb) ||
        (a.unscaled_basis_rgb && a.unscaled_stride < 3 * nb) || (a.basis_acc && a.basis_acc_stride < nb) || (a.gt_weights && a.gt_weights_stride < nb))
        return PNR_ERR_INVALID;
    if (n * 3 * (nb ? nb : 1u) > 0xffffffffull) return PNR_ERR_UNSUPPORTED;
    SheetPlan p{};
    p.W = a.W;
    p.nb = nb;
    p.n_rays = (uint32_t)n;
    uint32_t lds = 0;
    auto add = [&](const float* src, uint32_t stride, uint8_t* dst, uint32_t kind, uint32_t cols, int srgb) {
        if (!src || !dst) return;
        SheetMap& m = p.m[p.count++];
        m.src = src; m.dst = dst; m.stride = stride; m.cols = cols; m.kind = kind; m.lds_base = lds; m.srgb = srgb;
        lds += kSheetRays * cols;
    };
    add(a.image, a.image_stride, a.out_rgb, kSheetPix3, 3, a.linear_to_srgb ? 1 : 0);
    add(a.depth, a.depth_stride, a.out_depth, kSheetDepth, 1, 0);
    add(a.view_dep_rgb, a.view_dep_stride, a.out_view_dep, kSheetPix3, 3, 0);
    add(a.direct_rgb, a.direct_stride, a.out_direct, kSheetPix3, 3, 0);
    add(a.basis_rgb, a.basis_rgb_stride, a.out_basis_img, kSheetBasis3, 3 * nb, 0);
    add(a.unscaled_basis_rgb, a.unscaled_stride, a.out_unscaled_basis_img, kSheetBasis3, 3 * nb, 0);
    add(a.basis_acc, a.basis_acc_stride, a.out_basis_acc, kSheetBasis1, nb, 0);
    add(a.gt_weights, a.gt_weights_stride, a.out_weights_guide, kSheetBasis1, nb, 0);
    if (lds > kSheetLds) return PNR_ERR_INVALID;   // (cannot happen: nb <= PNR_SHEET_MAX_BASIS)
    p.chunks = p.count ? (uint32_t)((n + kSheetRays - 1) / kSheetRays) : 0u;
    uint32_t swatch_blocks = 0;
    if (a.basis_color && a.out_basis_color) {
        p.palette = a.basis_color;
        p.swatch = a.out_basis_color;
        swatch_blocks = cdiv(kSwatch * kSwatch * 3u * nb + 3u, 4u * kSheetBlock);   // + 3: a ragged head shifts the dword units by up to three bytes
    }
    if (p.chunks + swatch_blocks == 0) return PNR_OK;
    hipLaunchKernelGGL(k_palette_sheets, dim3(p.chunks + swatch_blocks), dim3(kSheetBlock), 0, as_stream(stream), p);
    return check_launch();
}

uint64_t pnr_frame_metrics_workspace_bytes(uint32_t H, uint32_t W) {
    const uint64_t tiles = (uint64_t)cdiv(H ? H : 1u, kMetTile) * cdiv(W ? W : 1u, kMetTile);
    return kMetHdr + tiles * kMetRow * sizeof(double);
}

int pnr_frame_metrics(const pnr_metrics_args* args, pnr_stream_t stream) {
    if (!args) return PNR_ERR_INVALID;
    const pnr_metrics_args& a = *args;
    if ((uint64_t)a.H * a.W == 0) return PNR_OK;
    if (!a.pred || !a.truth || !a.totals || !a.workspace || a.pred_stride < 3) return PNR_ERR_INVALID;
    if (a.truth_channels != 3 && a.truth_channels != 4) return PNR_ERR_INVALID;
    if (a.basis_acc && (a.num_basis < 1 || a.num_basis > PNR_MAX_BASIS || a.basis_acc_stride < a.num_basis)) return PNR_ERR_INVALID;
    if ((a.want & PNR_METRIC_SSIM) && (a.H <= (uint32_t)kMetHalo || a.W <= (uint32_t)kMetHalo)) return PNR_ERR_INVALID;
    if (a.basis_acc && (a.want & PNR_METRIC_TV) && (a.H < 2 || a.W < 2)) return PNR_ERR_INVALID;
    if (a.workspace_bytes < pnr_frame_metrics_workspace_bytes(a.H, a.W) || (reinterpret_cast<uintptr_t>(a.workspace) & 7u)) return PNR_ERR_INVALID;
    const uint64_t tiles = (uint64_t)cdiv(a.H, kMetTile) * cdiv(a.W, kMetTile);
    if (tiles > 0x7fffffffull || (uint64_t)a.H * a.W > 0x7fffffffull) return PNR_ERR_UNSUPPORTED;
    if (!raise_lds<k_frame_metrics>(kMetLds)) return PNR_ERR_LAUNCH;
    MetricsLaunch L;
    L.a = a;
    L.tiles_x = cdiv(a.W, kMetTile);
    hipLaunchKernelGGL(k_frame_metrics, dim3((uint32_t)tiles), dim3(kMetBlock), kMetLds, as_stream(stream), L);
    return check_launch();
}

}  // extern "C"
