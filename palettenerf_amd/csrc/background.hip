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

// one level of the D = 2, C = 2 lookup: the cell, corner order and accumulation of k_grid_fwd<T, 2, 2> (gridencoder.hip), bit for bit
template <typename T>
__device__ __forceinline__ void bg_level(const BgParams& p, uint32_t level, const float in[2], bool oob, float& f0, float& f1) {
    const uint32_t off0 = (uint32_t)p.offsets[level];
    const uint32_t hashmap_size = (uint32_t)p.offsets[level + 1] - off0;
    f0 = f1 = 0.0f;
    // a level that would reach beyond the table the caller described reads nothing (the offsets are device data the host never sees)
    if (oob || hashmap_size == 0u || (uint64_t)off0 + hashmap_size > (uint64_t)p.table_rows) return;
    const T* grid = static_cast<const T*>(p.embeddings) + (size_t)off0 * 2;
    const float scale = p.scale[level];
    const uint32_t resolution = p.resolution[level];
    float pos[2];
    uint32_t pg[2];
#pragma unroll
    for (uint32_t d = 0; d < 2; d++) {
        pos[d] = fmaf(in[d], scale, p.align_corners ? 0.0f : 0.5f);
        const float fl = floorf(pos[d]);
        pg[d] = (uint32_t)fl;
        pos[d] -= (float)pg[d];
        pg[d] = pg[d] < resolution ? pg[d] : resolution - 1u;   // the identity for inputs in [0, 1] (pg <= scale + 0.5 < resolution); keeps any other cell inside the level
    }
    // get_grid_index (gridencoder.cu:49-72) by kind of level, decided by the running stride as grid_index does; wave-uniform
    const uint32_t side = p.align_corners ? resolution : resolution + 1u;
    const bool dense = !p.align_corners && (uint64_t)side * side <= (uint64_t)hashmap_size;      // index < side^2 <= size: the `%` is the identity
    uint32_t stride = 1u;
#pragma unroll
    for (uint32_t d = 0; d < 2; d++)
        if (stride <= hashmap_size) stride *= side;
    const bool hashed_pow2 = !dense && p.gridtype == 0u && stride > hashmap_size && (hashmap_size & (hashmap_size - 1u)) == 0u;
    uint32_t idxs[4];
    float ws[4];
#pragma unroll
    for (uint32_t idx = 0; idx < 4; idx++) {
        const uint32_t pl[2] = {pg[0] + (idx & 1u), pg[1] + ((idx >> 1) & 1u)};
        float w = 1.0f;
        w *= (idx & 1u) ? pos[0] : 1.0f - pos[0];
        w *= (idx & 2u) ? pos[1] : 1.0f - pos[1];
        ws[idx] = w;
        if (dense) idxs[idx] = pl[0] + pl[1] * side;
        else if (hashed_pow2) idxs[idx] = (pl[0] ^ (pl[1] * 2654435761u)) & (hashmap_size - 1u);
        else idxs[idx] = grid_index<2, 1>(p.gridtype, p.align_corners, hashmap_size, resolution, pl);
    }
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
    if (a->table_dtype == PNR_DTYPE_F32) hipLaunchKernelGGL(k_background<float>, grid, block, 0, as_stream(stream), p);
    else hipLaunchKernelGGL(k_background<__half>, grid, block, 0, as_stream(stream), p);
    return check_launch();
}

}  // extern "C"
