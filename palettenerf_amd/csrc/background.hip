// background.hip -- the background model of an unbounded capture (bg_radius > 0) as ONE launch for gfx950 (MI355X).
//
// What it computes is nerf/network.py:145-160 behind raymarching.cu:166-201 (sph_from_ray): per ray the sphere coordinates, the 2-D hash-grid
// lookup of `encoder_bg` (4 levels x 2 features), SH degree 4 of the direction and bg_net 24 -> 64 -> 3 with ReLU and sigmoid.  Written per
// operator that is ten launches for all N rays of every frame; the work is one coordinate transform, 16 gathers and 1 728 multiply-adds per ray.
//
// One ray per lane, 256 lanes per workgroup.  The 7 KiB of weights sit in LDS; every lane of a wave reads the SAME weight at the same time (a
// broadcast read: no bank conflict), 16 bytes per instruction.  The products are fp32 fmaf chains in input order: accuracy is worth more here than
// matrix rate (no split-fp16 path).  Measured, the launch moves its bytes at 0.24 of 8 TB/s: it is not bound by its 16 gathers per ray
// (profiles/background/README.md); what remains is this network.
//
// Training (pnr_background_train_forward / pnr_background_backward): the forward is the same arithmetic from the raw weights (staged into LDS in
// the packed layout by the kernel: no pack launch behind every optimiser step) and always writes the sphere coordinates.  The backward takes one
// ray per lane in ONE-wave workgroups: it recomputes the hidden layer, takes the gradient through sigmoid and ReLU, scatters the table gradient
// with float atomics and leaves the wave's 64 x 24 and 3 x 64 weight-gradient sums as one slab of the workspace (summed over its 64 rays in ray
// order out of LDS: lane j owns row j).  k_background_wgrad_sum adds the slabs in slab order: two launches, no hand-off between workgroups, and
// weight gradients that are the same bits on every run.
#include "pnr_common.hpp"
#include "grid_core.hpp"
#include "sh_eval.hpp"
#include "sph_core.hpp"

namespace pnr {

constexpr uint32_t kBgLevels = 4, kBgIn = 24, kBgHidden = 64;
constexpr uint32_t kBgW1Off = kBgHidden * kBgIn;               // W0 [64][24] as nn.Linear stores it, then W1 as [64][4] = (W1[0][j], W1[1][j], W1[2][j], 0)
constexpr uint32_t kBgBlobFloats = kBgW1Off + kBgHidden * 4;   // 1 792 floats = 7 168 bytes

struct BgParams {
    uint32_t N;
    const float* rays_o;
    const float* rays_d;
    float radius;
    const float* coords_in;
    const void* embeddings;
    const int32_t* offsets;
    uint32_t table_rows, gridtype;
    bool align_corners;
    float scale[kBgLevels];
    uint32_t resolution[kBgLevels];
    const float* packed;
    float* out;
    float* coords_out;
};

__global__ void __launch_bounds__(256) k_background_pack(const float* __restrict__ w0, const float* __restrict__ w1, float* __restrict__ packed) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < kBgW1Off) packed[i] = w0[i];
    else if (i < kBgBlobFloats) {
        const uint32_t j = (i - kBgW1Off) >> 2, c = (i - kBgW1Off) & 3u;
        packed[i] = c < 3u ? w1[c * kBgHidden + j] : 0.0f;
    }
}

// the cell of one level of the D = 2 lookup: the cell, corner order and index of k_grid_fwd<T, 2, 2> (gridencoder.hip), bit for bit.  Shared by
// the lookup (bg_level) and the table gradient (k_background_bwd).  false: the level contributes nothing (out of range, or it would reach beyond
// the table the caller described -- the offsets are device data the host never sees); true: rows off0 + idxs[c] < table_rows with weights ws[c]
__device__ __forceinline__ bool bg_level_corners(const BgParams& p, uint32_t level, const float in[2], bool oob, uint32_t& off0, uint32_t idxs[4], float ws[4]) {
    off0 = (uint32_t)p.offsets[level];
    const uint32_t hashmap_size = (uint32_t)p.offsets[level + 1] - off0;
    if (oob || hashmap_size == 0u || (uint64_t)off0 + hashmap_size > (uint64_t)p.table_rows) return false;
    const float scale = p.scale[level];
    const uint32_t resolution = p.resolution[level];
    float pos[2];
    uint32_t pg[2];
    grid_cell<2>(in, scale, p.align_corners, pg, pos);
#pragma unroll
    for (uint32_t d = 0; d < 2; d++) pg[d] = pg[d] < resolution ? pg[d] : resolution - 1u;   // the identity for inputs in [0, 1] (pg <= scale + 0.5 < resolution); keeps any other cell inside the level
    corner_weights<2>(pos, ws);
    corner_rows<2, 1>(level_kind<2>(p.gridtype, hashmap_size, resolution, p.align_corners), p.gridtype, p.align_corners, hashmap_size, resolution, pg, idxs);   // (wave-uniform kind)
    return true;
}

// one level of the D = 2, C = 2 lookup: the accumulation of k_grid_fwd<T, 2, 2> over bg_level_corners' cell
template <typename T>
__device__ __forceinline__ void bg_level(const BgParams& p, uint32_t level, const float in[2], bool oob, float& f0, float& f1) {
    f0 = f1 = 0.0f;
    uint32_t off0, idxs[4];
    float ws[4];
    if (!bg_level_corners(p, level, in, oob, off0, idxs, ws)) return;
    const T* grid = static_cast<const T*>(p.embeddings) + (size_t)off0 * 2;
    T acc[2];
    if constexpr (sizeof(T) == 4) { acc[0] = 0.0f; acc[1] = 0.0f; } else { acc[0] = __float2half(0.0f); acc[1] = __float2half(0.0f); }
#pragma unroll
    for (uint32_t idx = 0; idx < 4; idx++) corner_accumulate<2>(acc, ws[idx], grid + (size_t)idxs[idx] * 2);
    f0 = to_f32(acc[0]);      // fp16 table: the half accumulator of the reference's autocast lookup, upcast once
    f1 = to_f32(acc[1]);
}

template <typename T>
__global__ void __launch_bounds__(256) k_background(const BgParams p) {
    __shared__ __attribute__((aligned(16))) float w[kBgBlobFloats];
    for (uint32_t i = threadIdx.x; i < kBgBlobFloats / 4; i += 256u)
        reinterpret_cast<float4*>(w)[i] = reinterpret_cast<const float4*>(p.packed)[i];
    __syncthreads();
    const uint32_t n = blockIdx.x * 256u + threadIdx.x;
    if (n >= p.N) return;

    const float dx = p.rays_d[(size_t)n * 3], dy = p.rays_d[(size_t)n * 3 + 1], dz = p.rays_d[(size_t)n * 3 + 2];
    float u, v;
    if (p.coords_in) {
        const float2 c = reinterpret_cast<const float2*>(p.coords_in)[n];
        u = c.x; v = c.y;
    } else {
        sph_coords_of(p.rays_o[(size_t)n * 3], p.rays_o[(size_t)n * 3 + 1], p.rays_o[(size_t)n * 3 + 2], dx, dy, dz, p.radius, u, v);
    }
    if (p.coords_out) reinterpret_cast<float2*>(p.coords_out)[n] = make_float2(u, v);

    // h = cat([encoder_dir(d), encoder_bg(x)]): the direction features come first (nerf/network.py:151)
    float x[kBgIn];
    sh_eval<4>(dx, dy, dz, x);
    // GridEncoder.forward with its default bound = 1: (x + 1) / 2, the same two roundings (gridencoder/grid.py:142)
    const float in[2] = {(u + 1.0f) / 2.0f, (v + 1.0f) / 2.0f};
    const bool oob = (in[0] < 0.0f) | (in[0] > 1.0f) | (in[1] < 0.0f) | (in[1] > 1.0f);     // outside the grid: zero features (gridencoder.cu:97-113)
#pragma unroll
    for (uint32_t l = 0; l < kBgLevels; l++) bg_level<T>(p, l, in, oob, x[16 + 2 * l], x[17 + 2 * l]);

    // bg_net: 24 -> 64 (ReLU) -> 3, then torch.sigmoid
    float o0 = 0.0f, o1 = 0.0f, o2 = 0.0f;
#pragma unroll 2
    for (uint32_t j = 0; j < kBgHidden; j++) {
        const float4* row = reinterpret_cast<const float4*>(w + j * kBgIn);
        float acc = 0.0f;
#pragma unroll
        for (uint32_t q = 0; q < kBgIn / 4; q++) {
            const float4 c = row[q];
            acc = fmaf(x[4 * q], c.x, acc);
            acc = fmaf(x[4 * q + 1], c.y, acc);
            acc = fmaf(x[4 * q + 2], c.z, acc);
            acc = fmaf(x[4 * q + 3], c.w, acc);
        }
        const float h = acc < 0.0f ? 0.0f : acc;       // F.relu (a NaN stays a NaN)
        const float4 c = reinterpret_cast<const float4*>(w + kBgW1Off)[j];
        o0 = fmaf(h, c.x, o0);
        o1 = fmaf(h, c.y, o1);
        o2 = fmaf(h, c.z, o2);
    }
    float* out = p.out + (size_t)n * 3;
    out[0] = 1.0f / (1.0f + expf(-o0));     // as the NeRF field kernel's colour head (field.hip)
    out[1] = 1.0f / (1.0f + expf(-o1));
    out[2] = 1.0f / (1.0f + expf(-o2));
}

// ---------------------------------------------------------------- training
// The pieces of k_background's body, for the training kernels (k_background itself keeps its text: its instructions are the inference path's and do
// not move with this section).  The arithmetic is therefore written twice; what keeps the two copies together is
// tests/test_gpu_background_train.py::test_forward_is_the_inference_launch_bit_for_bit (train forward == k_background<float>, every bit).  Per ray: the sphere coordinates (computed or read; written to coords_out when that is given) and the network's 24 inputs
template <typename T>
__device__ __forceinline__ void bg_inputs(const BgParams& p, uint32_t n, float x[kBgIn], float in[2], bool& oob) {
    const float dx = p.rays_d[(size_t)n * 3], dy = p.rays_d[(size_t)n * 3 + 1], dz = p.rays_d[(size_t)n * 3 + 2];
    float u, v;
    if (p.coords_in) {
        const float2 c = reinterpret_cast<const float2*>(p.coords_in)[n];
        u = c.x; v = c.y;
    } else {
        sph_coords_of(p.rays_o[(size_t)n * 3], p.rays_o[(size_t)n * 3 + 1], p.rays_o[(size_t)n * 3 + 2], dx, dy, dz, p.radius, u, v);
    }
    if (p.coords_out) reinterpret_cast<float2*>(p.coords_out)[n] = make_float2(u, v);

    // h = cat([encoder_dir(d), encoder_bg(x)]): the direction features come first (nerf/network.py:151)
    sh_eval<4>(dx, dy, dz, x);
    // GridEncoder.forward with its default bound = 1: (x + 1) / 2, the same two roundings (gridencoder/grid.py:142)
    in[0] = (u + 1.0f) / 2.0f;
    in[1] = (v + 1.0f) / 2.0f;
    oob = (in[0] < 0.0f) | (in[0] > 1.0f) | (in[1] < 0.0f) | (in[1] > 1.0f);     // outside the grid: zero features (gridencoder.cu:97-113)
#pragma unroll
    for (uint32_t l = 0; l < kBgLevels; l++) bg_level<T>(p, l, in, oob, x[16 + 2 * l], x[17 + 2 * l]);
}

// hidden unit j before its ReLU: an fmaf chain in input order over row j of W0 in LDS
__device__ __forceinline__ float bg_hidden(const float* w, uint32_t j, const float x[kBgIn]) {
    const float4* row = reinterpret_cast<const float4*>(w + j * kBgIn);
    float acc = 0.0f;
#pragma unroll
    for (uint32_t q = 0; q < kBgIn / 4; q++) {
        const float4 c = row[q];
        acc = fmaf(x[4 * q], c.x, acc);
        acc = fmaf(x[4 * q + 1], c.y, acc);
        acc = fmaf(x[4 * q + 2], c.z, acc);
        acc = fmaf(x[4 * q + 3], c.w, acc);
    }
    return acc;
}

// bg_net: 24 -> 64 (ReLU) -> 3, then torch.sigmoid; `w` is the packed blob in LDS
__device__ __forceinline__ void bg_net(const float* w, const float x[kBgIn], float* out) {
    float o0 = 0.0f, o1 = 0.0f, o2 = 0.0f;
#pragma unroll 2
    for (uint32_t j = 0; j < kBgHidden; j++) {
        const float acc = bg_hidden(w, j, x);
        const float h = acc < 0.0f ? 0.0f : acc;       // F.relu (a NaN stays a NaN)
        const float4 c = reinterpret_cast<const float4*>(w + kBgW1Off)[j];
        o0 = fmaf(h, c.x, o0);
        o1 = fmaf(h, c.y, o1);
        o2 = fmaf(h, c.z, o2);
    }
    out[0] = 1.0f / (1.0f + expf(-o0));     // as the NeRF field kernel's colour head (field.hip)
    out[1] = 1.0f / (1.0f + expf(-o1));
    out[2] = 1.0f / (1.0f + expf(-o2));
}

struct BgTrainParams {
    BgParams p;                  // p.packed is not read: the kernels stage the raw weights themselves
    const float* w0;             // bg_net.0.weight [64][24]
    const float* w1;             // bg_net.1.weight [3][64]
    const float* grad_rgb;       // [N][3]
    float* grad_table;           // [table_rows][2], zeroed by the caller; may be null (no table gradient wanted)
    float* slabs;                // [cdiv(N, 64)][kBgSlabFloats]
};

constexpr uint32_t kBgSlabFloats = kBgHidden * kBgIn + 3 * kBgHidden;      // grad W0 [64][24], then grad W1 [3][64]
constexpr uint32_t kBgRowPad = PNR_WAVE + 1;                               // [unit][ray] LDS rows: lane j reads row j, an odd stride keeps the 64 rows on distinct banks

// the packed layout of k_background_pack, written into LDS from the raw weights: W0 is a straight copy, W1 [3][64] becomes [64][4].  Branch-free
// loops with independent loads (a lane's loads are all in flight together)
template <uint32_t THREADS>
__device__ __forceinline__ void bg_stage_weights(const float* __restrict__ w0, const float* __restrict__ w1, float* w) {
#pragma unroll
    for (uint32_t i = 0; i < kBgW1Off / THREADS; i++) w[i * THREADS + threadIdx.x] = w0[i * THREADS + threadIdx.x];
    if (threadIdx.x < kBgHidden)
        reinterpret_cast<float4*>(w + kBgW1Off)[threadIdx.x] = make_float4(w1[threadIdx.x], w1[kBgHidden + threadIdx.x], w1[2 * kBgHidden + threadIdx.x], 0.0f);
}
static_assert(kBgW1Off % 256 == 0 && kBgW1Off % PNR_WAVE == 0, "bg_stage_weights copies W0 in whole rounds of the workgroup");

__global__ void __launch_bounds__(256) k_background_train_fwd(const BgTrainParams t) {
    __shared__ __attribute__((aligned(16))) float w[kBgBlobFloats];
    bg_stage_weights<256>(t.w0, t.w1, w);
    __syncthreads();
    const uint32_t n = blockIdx.x * 256u + threadIdx.x;
    if (n >= t.p.N) return;
    float x[kBgIn], in[2];
    bool oob;
    bg_inputs<float>(t.p, n, x, in, oob);
    bg_net(w, x, t.p.out + (size_t)n * 3);
}

// One wave per workgroup, one ray per lane.  LDS: the packed weights; then per ray the inputs X [ray][24], d loss / d output GO [ray][4], and
// per hidden unit the activations HT [unit][ray] and their gradients GT [unit][ray].
__global__ void __launch_bounds__(PNR_WAVE) k_background_bwd(const BgTrainParams t) {
    __shared__ __attribute__((aligned(16))) float w[kBgBlobFloats];
    __shared__ __attribute__((aligned(16))) float X[PNR_WAVE * kBgIn];
    __shared__ __attribute__((aligned(16))) float GO[PNR_WAVE * 4];
    __shared__ float HT[kBgHidden * kBgRowPad];
    __shared__ float GT[kBgHidden * kBgRowPad];
    const BgParams& p = t.p;
    bg_stage_weights<PNR_WAVE>(t.w0, t.w1, w);
    __syncthreads();
    const uint32_t lane = threadIdx.x, n = blockIdx.x * PNR_WAVE + lane;
    const bool live = n < p.N;

    // a lane without a ray holds zeros: it adds nothing to the sums below
    float x[kBgIn], in[2] = {0.0f, 0.0f}, g[3] = {0.0f, 0.0f, 0.0f};
    bool oob = true;
#pragma unroll
    for (uint32_t i = 0; i < kBgIn; i++) x[i] = 0.0f;
    if (live) bg_inputs<float>(p, n, x, in, oob);      // p.coords_in: the coordinates the forward saved; p.coords_out is null
#pragma unroll
    for (uint32_t q = 0; q < kBgIn / 4; q++) reinterpret_cast<float4*>(X + lane * kBgIn)[q] = make_float4(x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]);

    // the forward again: the hidden layer is 1 536 fmaf per ray, cheaper than an [N, 64] tensor kept since the forward
    float o[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll 2
    for (uint32_t j = 0; j < kBgHidden; j++) {
        const float acc = bg_hidden(w, j, x);
        const float h = acc < 0.0f ? 0.0f : acc;
        HT[j * kBgRowPad + lane] = h;
        const float4 c = reinterpret_cast<const float4*>(w + kBgW1Off)[j];
        o[0] = fmaf(h, c.x, o[0]);
        o[1] = fmaf(h, c.y, o[1]);
        o[2] = fmaf(h, c.z, o[2]);
    }
    if (live) {
#pragma unroll
        for (uint32_t k = 0; k < 3; k++) {
            const float s = 1.0f / (1.0f + expf(-o[k]));
            g[k] = t.grad_rgb[(size_t)n * 3 + k] * ((1.0f - s) * s);      // sigmoid'
        }
    }
    reinterpret_cast<float4*>(GO)[lane] = make_float4(g[0], g[1], g[2], 0.0f);

    // through W1 and the ReLU (a NaN activation keeps its gradient, which is a NaN already: threshold_backward's rule), on to the eight table features
    float gx[2 * kBgLevels];
#pragma unroll
    for (uint32_t i = 0; i < 2 * kBgLevels; i++) gx[i] = 0.0f;
#pragma unroll 2
    for (uint32_t j = 0; j < kBgHidden; j++) {
        const float h = HT[j * kBgRowPad + lane];
        const float4 c = reinterpret_cast<const float4*>(w + kBgW1Off)[j];
        const float gh = h <= 0.0f ? 0.0f : fmaf(g[2], c.z, fmaf(g[1], c.y, g[0] * c.x));
        GT[j * kBgRowPad + lane] = gh;
        const float4* row = reinterpret_cast<const float4*>(w + j * kBgIn + 16);
        const float4 r0 = row[0], r1 = row[1];
        gx[0] = fmaf(gh, r0.x, gx[0]); gx[1] = fmaf(gh, r0.y, gx[1]); gx[2] = fmaf(gh, r0.z, gx[2]); gx[3] = fmaf(gh, r0.w, gx[3]);
        gx[4] = fmaf(gh, r1.x, gx[4]); gx[5] = fmaf(gh, r1.y, gx[5]); gx[6] = fmaf(gh, r1.z, gx[6]); gx[7] = fmaf(gh, r1.w, gx[7]);
    }

    // table gradient: the forward's own cells, one float atomic per corner and feature (k_grid_bwd's form)
    if (live && t.grad_table) {
#pragma unroll
        for (uint32_t l = 0; l < kBgLevels; l++) {
            uint32_t off0, idxs[4];
            float ws[4];
            if (!bg_level_corners(p, l, in, oob, off0, idxs, ws)) continue;
            float* dst = t.grad_table + (size_t)off0 * 2;
#pragma unroll
            for (uint32_t idx = 0; idx < 4; idx++) {
                unsafeAtomicAdd(dst + (size_t)idxs[idx] * 2, ws[idx] * gx[2 * l]);
                unsafeAtomicAdd(dst + (size_t)idxs[idx] * 2 + 1, ws[idx] * gx[2 * l + 1]);
            }
        }
    }
    __syncthreads();

    // weight gradients of this wave's 64 rays, summed in ray order: lane j owns hidden unit j
    float* slab = t.slabs + (size_t)blockIdx.x * kBgSlabFloats;
    float a0[kBgIn], a1[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (uint32_t i = 0; i < kBgIn; i++) a0[i] = 0.0f;
    for (uint32_t r = 0; r < PNR_WAVE; r++) {
        const float gh = GT[lane * kBgRowPad + r], h = HT[lane * kBgRowPad + r];
        const float4 go = reinterpret_cast<const float4*>(GO)[r];
        a1[0] = fmaf(go.x, h, a1[0]);
        a1[1] = fmaf(go.y, h, a1[1]);
        a1[2] = fmaf(go.z, h, a1[2]);
#pragma unroll
        for (uint32_t q = 0; q < kBgIn / 4; q++) {
            const float4 xr = reinterpret_cast<const float4*>(X + r * kBgIn)[q];
            a0[4 * q] = fmaf(gh, xr.x, a0[4 * q]);
            a0[4 * q + 1] = fmaf(gh, xr.y, a0[4 * q + 1]);
            a0[4 * q + 2] = fmaf(gh, xr.z, a0[4 * q + 2]);
            a0[4 * q + 3] = fmaf(gh, xr.w, a0[4 * q + 3]);
        }
    }
#pragma unroll
    for (uint32_t q = 0; q < kBgIn / 4; q++)
        reinterpret_cast<float4*>(slab + lane * kBgIn)[q] = make_float4(a0[4 * q], a0[4 * q + 1], a0[4 * q + 2], a0[4 * q + 3]);
#pragma unroll
    for (uint32_t k = 0; k < 3; k++) slab[kBgHidden * kBgIn + k * kBgHidden + lane] = a1[k];
}

// the slabs added in slab order (four interleaved running sums, then ((s0 + s1) + s2) + s3): every element of both gradients is written
__global__ void __launch_bounds__(256) k_background_wgrad_sum(const float* __restrict__ slabs, uint32_t n_slabs, float* __restrict__ grad_w0, float* __restrict__ grad_w1) {
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e >= kBgSlabFloats) return;
    float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    uint32_t b = 0;
    for (; b + 4 <= n_slabs; b += 4) {
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) s[k] += slabs[(size_t)(b + k) * kBgSlabFloats + e];
    }
    for (uint32_t k = 0; b < n_slabs; b++, k++) s[k] += slabs[(size_t)b * kBgSlabFloats + e];
    const float v = ((s[0] + s[1]) + s[2]) + s[3];
    if (e < kBgHidden * kBgIn) grad_w0[e] = v;
    else grad_w1[e - kBgHidden * kBgIn] = v;
}

}  // namespace pnr

using namespace pnr;

extern "C" {

uint64_t pnr_background_packed_bytes(void) { return (uint64_t)kBgBlobFloats * sizeof(float); }

int pnr_background_pack(const float* w0, const float* w1, float* packed, pnr_stream_t stream) {
    if (!w0 || !w1 || !packed) return PNR_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(packed) & 15u) != 0) return PNR_ERR_ALIGNMENT;
    hipLaunchKernelGGL(k_background_pack, dim3(cdiv(kBgBlobFloats, 256)), dim3(256), 0, as_stream(stream), w0, w1, packed);
    return check_launch();
}

int pnr_background_forward(const pnr_background_args* a, pnr_stream_t stream) {
    if (!a) return PNR_ERR_INVALID;
    if (a->num_levels != kBgLevels || a->level_dim != 2u || a->sh_degree != 4u || a->num_layers != 2u || a->hidden_dim != kBgHidden) return PNR_ERR_UNSUPPORTED;
    if (a->table_dtype != PNR_DTYPE_F32 && a->table_dtype != PNR_DTYPE_F16) return PNR_ERR_UNSUPPORTED;
    if (a->gridtype > 1u) return PNR_ERR_UNSUPPORTED;
    if (a->N == 0) return PNR_OK;
    if (!a->rays_d || !a->embeddings || !a->offsets || !a->packed || !a->out || a->table_rows == 0u) return PNR_ERR_INVALID;
    if (!a->coords_in && !a->rays_o) return PNR_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(a->packed) & 15u) != 0) return PNR_ERR_ALIGNMENT;
    // float2 accesses of the coordinate arrays, 4- / 8-byte rows of the table
    if ((reinterpret_cast<uintptr_t>(a->coords_in) & 7u) != 0 || (reinterpret_cast<uintptr_t>(a->coords_out) & 7u) != 0) return PNR_ERR_ALIGNMENT;
    if ((reinterpret_cast<uintptr_t>(a->embeddings) & (a->table_dtype == PNR_DTYPE_F32 ? 7u : 3u)) != 0) return PNR_ERR_ALIGNMENT;
    const LevelParams lp = make_level_params(kBgLevels, a->S, a->H);      // the op's own per-level scale / resolution (gridencoder.cu:125-126)
    BgParams p;
    p.N = a->N; p.rays_o = a->rays_o; p.rays_d = a->rays_d; p.radius = a->radius; p.coords_in = a->coords_in;
    p.embeddings = a->embeddings; p.offsets = a->offsets; p.table_rows = a->table_rows; p.gridtype = a->gridtype; p.align_corners = a->align_corners != 0;
    for (uint32_t l = 0; l < kBgLevels; l++) { p.scale[l] = lp.scale[l]; p.resolution[l] = lp.resolution[l]; }
    p.packed = a->packed; p.out = a->out; p.coords_out = a->coords_out;
    const dim3 grid(cdiv(a->N, 256)), block(256);
    hipLaunchKernelGGL(a->table_dtype == PNR_DTYPE_F32 ? k_background<float> : k_background<__half>, grid, block, 0, as_stream(stream), p);
    return check_launch();
}

static int background_train_check(const pnr_background_train_args* a) {
    if (!a) return PNR_ERR_INVALID;
    if (a->num_levels != kBgLevels || a->level_dim != 2u || a->sh_degree != 4u || a->num_layers != 2u || a->hidden_dim != kBgHidden) return PNR_ERR_UNSUPPORTED;
    if (a->table_dtype != PNR_DTYPE_F32) return PNR_ERR_UNSUPPORTED;        // training reads and differentiates the fp32 table
    if (a->gridtype > 1u) return PNR_ERR_UNSUPPORTED;
    return PNR_OK;
}

static BgTrainParams background_train_params(const pnr_background_train_args* a) {
    const LevelParams lp = make_level_params(kBgLevels, a->S, a->H);
    BgTrainParams t;
    BgParams& p = t.p;
    p.N = a->N; p.rays_o = a->rays_o; p.rays_d = a->rays_d; p.radius = a->radius; p.coords_in = a->coords_in;
    p.embeddings = a->embeddings; p.offsets = a->offsets; p.table_rows = a->table_rows; p.gridtype = a->gridtype; p.align_corners = a->align_corners != 0;
    for (uint32_t l = 0; l < kBgLevels; l++) { p.scale[l] = lp.scale[l]; p.resolution[l] = lp.resolution[l]; }
    p.packed = nullptr; p.out = a->out; p.coords_out = a->coords_out;
    t.w0 = a->w0; t.w1 = a->w1; t.grad_rgb = a->grad_rgb; t.grad_table = a->grad_table; t.slabs = static_cast<float*>(a->workspace);
    return t;
}

int pnr_background_train_forward(const pnr_background_train_args* a, pnr_stream_t stream) {
    if (const int rc = background_train_check(a)) return rc;
    if (a->N == 0) return PNR_OK;
    if (!a->rays_d || !a->embeddings || !a->offsets || !a->w0 || !a->w1 || !a->out || !a->coords_out || a->table_rows == 0u) return PNR_ERR_INVALID;
    if (!a->coords_in && !a->rays_o) return PNR_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(a->coords_in) & 7u) != 0 || (reinterpret_cast<uintptr_t>(a->coords_out) & 7u) != 0) return PNR_ERR_ALIGNMENT;
    if ((reinterpret_cast<uintptr_t>(a->embeddings) & 7u) != 0) return PNR_ERR_ALIGNMENT;
    const BgTrainParams t = background_train_params(a);
    hipLaunchKernelGGL(k_background_train_fwd, dim3(cdiv(a->N, 256)), dim3(256), 0, as_stream(stream), t);
    return check_launch();
}

uint64_t pnr_background_backward_workspace_bytes(uint32_t N) { return (uint64_t)cdiv(N ? N : 1u, PNR_WAVE) * kBgSlabFloats * sizeof(float); }

int pnr_background_backward(const pnr_background_train_args* a, pnr_stream_t stream) {
    if (const int rc = background_train_check(a)) return rc;
    if (a->N == 0) return PNR_OK;
    if (!a->rays_d || !a->coords_in || !a->embeddings || !a->offsets || !a->w0 || !a->w1 || !a->grad_rgb || !a->grad_w0 || !a->grad_w1 || !a->workspace
        || a->table_rows == 0u)
        return PNR_ERR_INVALID;
    if (a->workspace_bytes < pnr_background_backward_workspace_bytes(a->N)) return PNR_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(a->workspace) & 15u) != 0) return PNR_ERR_ALIGNMENT;                    // the slabs are written 16 bytes at a time
    if ((reinterpret_cast<uintptr_t>(a->coords_in) & 7u) != 0 || (reinterpret_cast<uintptr_t>(a->embeddings) & 7u) != 0) return PNR_ERR_ALIGNMENT;
    if ((reinterpret_cast<uintptr_t>(a->grad_table) & 3u) != 0) return PNR_ERR_ALIGNMENT;
    BgTrainParams t = background_train_params(a);
    t.p.out = nullptr; t.p.coords_out = nullptr;
    const uint32_t n_slabs = cdiv(a->N, PNR_WAVE);
    hipLaunchKernelGGL(k_background_bwd, dim3(n_slabs), dim3(PNR_WAVE), 0, as_stream(stream), t);
    if (const int rc = check_launch()) return rc;
    hipLaunchKernelGGL(k_background_wgrad_sum, dim3(cdiv(kBgSlabFloats, 256)), dim3(256), 0, as_stream(stream), t.slabs, n_slabs, a->grad_w0, a->grad_w1);
    return check_launch();
}

}  // extern "C"
