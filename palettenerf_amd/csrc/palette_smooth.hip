// palette_smooth.hip -- the smooth-loss block of a PaletteNeRF training step for gfx950 (palette/renderer.py:360-378).
//
// From smooth_loss_start_epoch on, every training step perturbs its M ~ 6e5 sample points, evaluates the field a second time there and
// weighs the squared change of the palette weights (and of the clip feature) by a bilateral weight over position, diffuse colour and clip
// feature.  In torch that is ~25-30 elementwise / reduction launches each way; here it is one launch for the points, one for the weight and
// the norm, one for the gradient:
//   xyzs_diff   = clamp(xyzs + noise * bound * 0.03, -bound, bound)                                       (torch's order, bit for bit)
//   w           = exp(-|xyzs - xyzs_diff|^2 / bound^2 / sigma_xyz - |diffuse - diffuse_diff|^2 / sigma_color - |clip - clip_diff| / sigma_clip)
//   smooth_norm = w * (sum_b (omega_diff_b - omega_b)^2 + sum_c (clip_diff_c - clip_c)^2)                 (w detached)
// The rows are 3, nb and clip_dim floats wide.  Forward: a workgroup owns 256 consecutive rows, reads each array's 256 x width block as one
// contiguous span (consecutive lanes, consecutive addresses), keeps the differences in an LDS tile of odd stride, and lane r then sums row r.
// Backward: purely elementwise over the same spans, the row's 2 g w taken from LDS.  HBM-bound: (12 + 2 nb + 2 clip) * 4 B read and 8 B
// written per sample forward, (2 + 2 nb + 2 clip) * 4 B read and (2 nb + 2 clip) * 4 B written backward.
#include "pnr_common.hpp"
#include <string.h>

namespace pnr {

constexpr uint32_t kSmoothMaxBasis = 16;    // as the shade kernels (palette_train.hip)
constexpr uint32_t kSmoothMaxClip = 128;    // CHECK_CHANNEL of the flex composite the row ends up in
constexpr uint32_t kSmoothRows = 256;       // rows of a tile = lanes of a workgroup
constexpr uint32_t kSmoothCols = 32;        // columns of the LDS tile: 3 + 3 + nb of the narrow arrays, or one chunk of the clip feature
constexpr uint32_t kSmoothStride = kSmoothCols | 1u;
constexpr uint32_t kSmoothMaxBlocks = 2048;

// f / w for f < 2^15 and 2 <= w <= 128 through one v_mul_hi_u32: magic = floor(2^32 / w) + 1 overshoots f / w by less than f / 2^32 < 1 / w
static_assert(kSmoothRows * kSmoothMaxClip <= (1u << 15) && kSmoothMaxClip <= 128 && 6 + kSmoothMaxBasis <= kSmoothCols, "row_of is exact for f < 2^15, w <= 128; the narrow arrays share one tile");
inline uint32_t row_magic(uint32_t w) { return w < 2 ? 0u : (uint32_t)(0x100000000ull / w) + 1u; }
__device__ __forceinline__ uint32_t row_of(uint32_t f, uint32_t w, uint32_t magic) { return w < 2 ? f : __umulhi(f, magic); }

// tile[r][col0 + c] = b[row0 + r][c0 + c] - a[row0 + r][c0 + c] for the nrows x cw block of two [M, width] arrays; with cw == width the block
// is one contiguous span, with a chunk of a wide row it is contiguous 4 cw bytes at a time
__device__ __forceinline__ void stage_diff(float* tile, const float* __restrict__ a, const float* __restrict__ b, uint32_t row0, uint32_t nrows,
                                           uint32_t width, uint32_t c0, uint32_t cw, uint32_t magic, uint32_t col0) {
    for (uint32_t f = threadIdx.x; f < nrows * cw; f += kSmoothRows) {
        const uint32_t r = row_of(f, cw, magic), c = f - r * cw;
        const size_t at = (size_t)(row0 + r) * width + c0 + c;
        tile[r * kSmoothStride + col0 + c] = b[at] - a[at];
    }
}

__device__ __forceinline__ float clamp_t(float v, float lo, float hi) { v = v < lo ? lo : v; return v > hi ? hi : v; }   // torch.clamp: a NaN stays
__device__ __forceinline__ float smooth_point(float x, float u, float bound) { return clamp_t(x + (u * bound) * 0.03f, -bound, bound); }

// n4 float4 groups, then the n - 4 n4 elements behind them one by one (n4 = 0 when an array does not start on a 16-byte boundary)
__global__ void __launch_bounds__(256) k_palette_smooth_points(uint64_t n4, uint64_t n, const float* __restrict__ xyzs, const float* __restrict__ noise,
                                                               float bound, float* __restrict__ out) {
    const uint64_t tid = (uint64_t)blockIdx.x * 256 + threadIdx.x, stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = tid; i < n4; i += stride) {
        const f32x4 x = reinterpret_cast<const f32x4*>(xyzs)[i], u = reinterpret_cast<const f32x4*>(noise)[i];
        f32x4 y;
#pragma unroll
        for (int k = 0; k < 4; k++) y[k] = smooth_point(x[k], u[k], bound);
        reinterpret_cast<f32x4*>(out)[i] = y;
    }
    for (uint64_t i = n4 * 4 + tid; i < n; i += stride) out[i] = smooth_point(xyzs[i], noise[i], bound);
}

__global__ void __launch_bounds__(256) k_palette_smooth_fwd(uint32_t M, uint32_t nb, uint32_t clip, const float* __restrict__ xyzs,
                                                            const float* __restrict__ xyzs_diff, const float* __restrict__ diffuse,
                                                            const float* __restrict__ diffuse_diff, const float* __restrict__ omega,
                                                            const float* __restrict__ omega_diff, const float* __restrict__ clip_feat,
                                                            const float* __restrict__ clip_feat_diff, float bound2, float sigma_xyz, float sigma_color,
                                                            float sigma_clip, uint32_t magic_nb, uint32_t magic_chunk, uint32_t magic_last,
                                                            float* __restrict__ smooth_weight, float* __restrict__ smooth_norm) {
    __shared__ float tile[kSmoothRows * kSmoothStride];
    const uint32_t magic3 = 0x55555556u;   // row_magic(3)
    const uint32_t ntiles = (M + kSmoothRows - 1) / kSmoothRows;
    const float* row = tile + threadIdx.x * kSmoothStride;
    for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint32_t row0 = t * kSmoothRows, i = row0 + threadIdx.x, nrows = M - row0 < kSmoothRows ? M - row0 : kSmoothRows;
        stage_diff(tile, xyzs, xyzs_diff, row0, nrows, 3, 0, 3, magic3, 0);
        stage_diff(tile, diffuse, diffuse_diff, row0, nrows, 3, 0, 3, magic3, 3);
        stage_diff(tile, omega, omega_diff, row0, nrows, nb, 0, nb, magic_nb, 6);
        __syncthreads();
        float sx = 0.0f, sr = 0.0f, so = 0.0f, sc = 0.0f;
        if (i < M) {
#pragma unroll
            for (int c = 0; c < 3; c++) { sx += row[c] * row[c]; sr += row[3 + c] * row[3 + c]; }
            for (uint32_t b = 0; b < nb; b++) so += row[6 + b] * row[6 + b];
        }
        __syncthreads();
        if (clip_feat)
            for (uint32_t c0 = 0; c0 < clip; c0 += kSmoothCols) {
                const bool last = clip - c0 <= kSmoothCols;
                const uint32_t cw = last ? clip - c0 : kSmoothCols;
                stage_diff(tile, clip_feat, clip_feat_diff, row0, nrows, clip, c0, cw, last ? magic_last : magic_chunk, 0);
                __syncthreads();
                if (i < M)
                    for (uint32_t c = 0; c < cw; c++) sc += row[c] * row[c];
                __syncthreads();
            }
        if (i < M) {
            const float xw = sx / bound2 / sigma_xyz, rw = sr / sigma_color;
            const float cwgt = (clip_feat && sigma_clip > 0.0f) ? sqrtf(sc) / sigma_clip : 0.0f;   // the norm, not its square (palette/renderer.py:371)
            const float w = expf(-xw - rw - cwgt);
            smooth_weight[i] = w;
            smooth_norm[i] = w * (so + sc);        // sc = 0 without a clip head; with one it counts whether or not sigma_clip > 0 (:377)
        }
    }
}

// one [M, width] pair: g_b = s_r (b - a), g_a = -g_b over the tile's contiguous span; either output may be null
__device__ __forceinline__ void smooth_pair_grad(const float* s, const float* __restrict__ a, const float* __restrict__ b, uint32_t row0, uint32_t nrows,
                                                 uint32_t width, uint32_t magic, float* __restrict__ g_a, float* __restrict__ g_b) {
    const size_t base = (size_t)row0 * width;
    for (uint32_t f = threadIdx.x; f < nrows * width; f += kSmoothRows) {
        const float v = s[row_of(f, width, magic)] * (b[base + f] - a[base + f]);
        if (g_b) g_b[base + f] = v;
        if (g_a) g_a[base + f] = -v;
    }
}

__global__ void __launch_bounds__(256) k_palette_smooth_bwd(uint32_t M, uint32_t nb, uint32_t clip, const float* __restrict__ g_norm,
                                                            const float* __restrict__ smooth_weight, const float* __restrict__ omega,
                                                            const float* __restrict__ omega_diff, const float* __restrict__ clip_feat,
                                                            const float* __restrict__ clip_feat_diff, uint32_t magic_nb, uint32_t magic_clip,
                                                            float* __restrict__ g_omega, float* __restrict__ g_omega_diff, float* __restrict__ g_clip,
                                                            float* __restrict__ g_clip_diff) {
    __shared__ float s[kSmoothRows];       // 2 g w of the tile's rows
    const uint32_t ntiles = (M + kSmoothRows - 1) / kSmoothRows;
    for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint32_t row0 = t * kSmoothRows, i = row0 + threadIdx.x, nrows = M - row0 < kSmoothRows ? M - row0 : kSmoothRows;
        if (i < M) s[threadIdx.x] = 2.0f * (g_norm[i] * smooth_weight[i]);
        __syncthreads();
        smooth_pair_grad(s, omega, omega_diff, row0, nrows, nb, magic_nb, g_omega, g_omega_diff);
        if (g_clip || g_clip_diff) smooth_pair_grad(s, clip_feat, clip_feat_diff, row0, nrows, clip, magic_clip, g_clip, g_clip_diff);
        __syncthreads();
    }
}

inline uint32_t smooth_blocks(uint32_t M) { const uint32_t want = cdiv(M, kSmoothRows); return want < kSmoothMaxBlocks ? want : kSmoothMaxBlocks; }
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
// k_palette_smooth_points: `items` = float4 groups when every array starts on a 16-byte boundary, single elements otherwise; one per lane and trip
// (the up to three elements behind the groups are picked up by the grid stride)
inline uint32_t smooth_points_blocks(uint64_t items) { const uint64_t want = (items + kSmoothRows - 1) / kSmoothRows; return (uint32_t)(want < kSmoothMaxBlocks ? want : kSmoothMaxBlocks); }

int smooth_launch_geometry(const char* entry, uint64_t rows, uint32_t* workgroups, uint32_t* rows_per_trip) {
    if (!strcmp(entry, "pnr_palette_smooth_points")) {
        if (rows > 3ull * UINT32_MAX) return PNR_ERR_INVALID;
        *workgroups = smooth_points_blocks(rows);
    } else if (!strcmp(entry, "pnr_palette_smooth_forward") || !strcmp(entry, "pnr_palette_smooth_backward")) {
        if (rows > UINT32_MAX) return PNR_ERR_INVALID;
        *workgroups = smooth_blocks((uint32_t)rows);
    } else
        return PNR_ERR_INVALID;
    *rows_per_trip = kSmoothRows;
    return PNR_OK;
}

}  // namespace pnr

using namespace pnr;

extern "C" {

int pnr_palette_smooth_points(const float* xyzs, const float* noise, float bound, uint32_t M, float* xyzs_diff, pnr_stream_t stream) {
    if (M == 0) return PNR_OK;
    if (!xyzs || !noise || !xyzs_diff) return PNR_ERR_INVALID;
    const uint64_t n = (uint64_t)M * 3, n4 = aligned16(xyzs) && aligned16(noise) && aligned16(xyzs_diff) ? n / 4 : 0;
    hipLaunchKernelGGL(k_palette_smooth_points, dim3(smooth_points_blocks(n4 ? n4 : n)), dim3(256), 0, as_stream(stream), n4, n,
                       xyzs, noise, bound, xyzs_diff);
    return check_launch();
}

int pnr_palette_smooth_forward(uint32_t M, uint32_t num_basis, uint32_t clip_dim, const float* xyzs, const float* xyzs_diff, const float* diffuse,
                               const float* diffuse_diff, const float* omega, const float* omega_diff, const float* clip_feat,
                               const float* clip_feat_diff, float bound, float sigma_xyz, float sigma_color, float sigma_clip, float* smooth_weight,
                               float* smooth_norm, pnr_stream_t stream) {
    if (num_basis == 0 || num_basis > kSmoothMaxBasis || clip_dim > kSmoothMaxClip) return PNR_ERR_UNSUPPORTED;
    if (M == 0) return PNR_OK;
    if (!xyzs || !xyzs_diff || !diffuse || !diffuse_diff || !omega || !omega_diff || !smooth_weight || !smooth_norm) return PNR_ERR_INVALID;
    if ((clip_feat == nullptr) != (clip_feat_diff == nullptr)) return PNR_ERR_INVALID;
    const uint32_t tail = clip_dim % kSmoothCols ? clip_dim % kSmoothCols : (clip_dim ? kSmoothCols : 0);
    hipLaunchKernelGGL(k_palette_smooth_fwd, dim3(smooth_blocks(M)), dim3(256), 0, as_stream(stream), M, num_basis, clip_dim, xyzs, xyzs_diff, diffuse,
                       diffuse_diff, omega, omega_diff, clip_feat, clip_feat_diff, bound * bound, sigma_xyz, sigma_color, sigma_clip, row_magic(num_basis),
                       row_magic(kSmoothCols), row_magic(tail), smooth_weight, smooth_norm);
    return check_launch();
}

int pnr_palette_smooth_backward(uint32_t M, uint32_t num_basis, uint32_t clip_dim, const float* grad_smooth_norm, const float* smooth_weight,
                                const float* omega, const float* omega_diff, const float* clip_feat, const float* clip_feat_diff, float* grad_omega,
                                float* grad_omega_diff, float* grad_clip_feat, float* grad_clip_feat_diff, pnr_stream_t stream) {
    if (num_basis == 0 || num_basis > kSmoothMaxBasis || clip_dim > kSmoothMaxClip) return PNR_ERR_UNSUPPORTED;
    if (M == 0) return PNR_OK;
    if (!grad_smooth_norm || !smooth_weight || !omega || !omega_diff || !grad_omega || !grad_omega_diff) return PNR_ERR_INVALID;
    if ((clip_feat == nullptr) != (clip_feat_diff == nullptr)) return PNR_ERR_INVALID;
    if ((grad_clip_feat || grad_clip_feat_diff) && !clip_feat) return PNR_ERR_INVALID;
    if (clip_dim == 0) grad_clip_feat = grad_clip_feat_diff = nullptr;
    hipLaunchKernelGGL(k_palette_smooth_bwd, dim3(smooth_blocks(M)), dim3(256), 0, as_stream(stream), M, num_basis, clip_dim, grad_smooth_norm,
                       smooth_weight, omega, omega_diff, clip_feat, clip_feat_diff, row_magic(num_basis), row_magic(clip_dim), grad_omega,
                       grad_omega_diff, grad_clip_feat, grad_clip_feat_diff);
    return check_launch();
}

}  // extern "C"
