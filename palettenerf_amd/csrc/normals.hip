// normals.hip -- the coloured mesh export's two device stages (include/pnr.h, "coloured mesh export"), as HIP for gfx950:
//   pnr_density_gradient     logit, d logit / d p and the unit normal of the shipped density field at n points, ONE launch
//   pnr_mesh_vertex_records  the vertex block of a binary PLY (world position | normal | rgba | float properties), ONE launch
//
// The gradient's layout: one lane per point, 256 points per workgroup, no grid cap and no tile loop.  sigma_net's first layer sits in LDS,
// transposed to [input j][hidden k] (8 KiB) so that the 64 weights of one input are sixteen ds_read_b128 at one address for the whole wave (a
// broadcast: no bank conflict), the 64 weights of the read row of the second layer beside it.  A lane walks the sixteen levels TWICE:
//   pass 1  cell, eight gathers, the forward chain (cell_interp: the library's own) -> the level's two features e; z_k += W0[k][2l] e0 + W0[k][2l+1] e1
//           for the 64 hidden units, held in registers.  Then logit = sum_k w1[k] max(z_k, 0) and a_k = z_k > 0 ? w1[k] : 0 in z's place.
//   pass 2  the same cell and gathers again (the rows are in the caches from pass 1), c_j = sum_k a_k W0[k][j] for the level's two inputs, the
//           level's 3 x 2 derivatives from the eight rows, grad_d += c_2l d e0 / d x_d + c_2l+1 d e1 / d x_d.
// Why twice: which hidden units are live is known only after ALL levels, and the alternatives keep either the [16, 3, 2] Jacobian (96 registers on
// top of z's 64: two waves per SIMD for a kernel whose time is gather latency) or 64 x 3 hidden derivatives alive.  Two walks keep a lane at
// z[64] + one level's rows; the Jacobian exists one level at a time, in registers.  Nothing is written but the outputs: no workspace, no scratch.
// Every sum is an fmaf chain in a fixed order inside one lane: a row's bits depend on the row alone.
#include "grid_core.hpp"

namespace pnr {

constexpr uint32_t kDgBlock = 256;      // points per workgroup = threads
constexpr uint32_t kDgLevels = 16, kDgHidden = 64, kDgIn = 32;

struct DgArgs {
    const float* points;
    uint32_t n;
    float bound, two_bound, inv_two_bound;
    const float* table;
    const int32_t* offsets;
    uint32_t gridtype;
    const float* sigma0;
    const float* sigma1;
    float* logit;
    float* grad;
    float* normal;
};

struct DgLevel {
    const f32x2* tab;
    uint32_t idxs[8];
    float frac[3];
    float scale;
};

// the cell of `in` on `level` through grid_core.hpp's path: the rows of its eight corners and the position inside it
__device__ __forceinline__ void dg_level(const DgArgs& a, const LevelParams& lp, uint32_t level, const float (&in)[3], DgLevel& c) {
    const uint32_t off0 = (uint32_t)a.offsets[level];
    const uint32_t hashmap_size = (uint32_t)a.offsets[level + 1] - off0;
    const uint32_t resolution = lp.resolution[level];
    const uint32_t kind = level_kind<3>(a.gridtype, hashmap_size, resolution);
    c.tab = reinterpret_cast<const f32x2*>(a.table) + off0;
    c.scale = lp.scale[level];
    uint32_t pg[3];
    grid_cell<3>(in, c.scale, false, pg, c.frac);
    corner_rows<3, 1>(kind, a.gridtype, false, hashmap_size, resolution, pg, c.idxs);
}

// d e / d x_axis of one cell (the dy_dx of gridencoder.cu:177-219): scale * sum over the four corner pairs of w(other two axes) * (right - left)
__device__ __forceinline__ void dg_axis(const f32x2 (&v)[8], const float (&frac)[3], float scale, uint32_t axis, float (&d)[2]) {
    const uint32_t o0 = axis == 0 ? 1u : 0u, o1 = axis == 2 ? 1u : 2u;      // the other two axes, lower first
    d[0] = 0.0f; d[1] = 0.0f;
#pragma unroll
    for (uint32_t pair = 0; pair < 4; pair++) {
        const uint32_t b0 = pair & 1u, b1 = pair >> 1;
        float w = scale;
        w *= b0 ? frac[o0] : 1.0f - frac[o0];
        w *= b1 ? frac[o1] : 1.0f - frac[o1];
        const uint32_t left = (b0 << o0) | (b1 << o1), right = left | (1u << axis);
        d[0] = fmaf(w, v[right].x - v[left].x, d[0]);
        d[1] = fmaf(w, v[right].y - v[left].y, d[1]);
    }
}

__global__ void __launch_bounds__(kDgBlock) k_density_gradient(DgArgs a, LevelParams lp) {
    __shared__ __attribute__((aligned(16))) float w0t[kDgIn * kDgHidden];      // [j][k] = sigma0[k][j]
    __shared__ __attribute__((aligned(16))) float w1[kDgHidden];               // sigma1[0][k]
    for (uint32_t i = threadIdx.x; i < kDgIn * kDgHidden; i += kDgBlock) w0t[(i & (kDgIn - 1)) * kDgHidden + (i >> 5)] = a.sigma0[i];
    if (threadIdx.x < kDgHidden) w1[threadIdx.x] = a.sigma1[threadIdx.x];
    __syncthreads();
    const uint32_t i = blockIdx.x * kDgBlock + threadIdx.x;
    if (i >= a.n) return;
    const float p[3] = {a.points[(size_t)i * 3], a.points[(size_t)i * 3 + 1], a.points[(size_t)i * 3 + 2]};
    float in[3];
    float logit = 0.0f, g[3] = {0.0f, 0.0f, 0.0f};
    if (unit_cube_of(p, a.bound, a.two_bound, a.inv_two_bound, in)) {
        float z[kDgHidden];
#pragma unroll
        for (uint32_t k = 0; k < kDgHidden; k++) z[k] = 0.0f;
#pragma unroll 1
        for (uint32_t level = 0; level < kDgLevels; level++) {
            DgLevel c;
            dg_level(a, lp, level, in, c);
            float e[2];
            cell_interp<f32x2, false, true>(c.tab, c.idxs, c.frac, e);
            const float4* r0 = reinterpret_cast<const float4*>(&w0t[(2 * level) * kDgHidden]);
            const float4* r1 = r0 + kDgHidden / 4;
#pragma unroll
            for (uint32_t q = 0; q < kDgHidden / 4; q++) {
                const float4 u0 = r0[q], u1 = r1[q];
                z[4 * q + 0] = fmaf(u1.x, e[1], fmaf(u0.x, e[0], z[4 * q + 0]));
                z[4 * q + 1] = fmaf(u1.y, e[1], fmaf(u0.y, e[0], z[4 * q + 1]));
                z[4 * q + 2] = fmaf(u1.z, e[1], fmaf(u0.z, e[0], z[4 * q + 2]));
                z[4 * q + 3] = fmaf(u1.w, e[1], fmaf(u0.w, e[0], z[4 * q + 3]));
            }
        }
        // logit, and in z's place a_k = d logit / d z_k: the ReLU's derivative is z > 0, strict
#pragma unroll
        for (uint32_t k = 0; k < kDgHidden; k++) {
            const float wk = w1[k];
            logit = fmaf(wk, fmaxf(z[k], 0.0f), logit);
            z[k] = z[k] > 0.0f ? wk : 0.0f;
        }
        if (a.grad || a.normal) {
#pragma unroll 1
            for (uint32_t level = 0; level < kDgLevels; level++) {
                DgLevel c;
                dg_level(a, lp, level, in, c);
                const f32x2* ptrs[8];
#pragma unroll
                for (int k = 0; k < 8; k++) ptrs[k] = c.tab + c.idxs[k];
                f32x2 v[8];
                load8_fresh(ptrs, v);
                const float4* r0 = reinterpret_cast<const float4*>(&w0t[(2 * level) * kDgHidden]);
                const float4* r1 = r0 + kDgHidden / 4;
                float c0 = 0.0f, c1 = 0.0f;
#pragma unroll
                for (uint32_t q = 0; q < kDgHidden / 4; q++) {
                    const float4 u0 = r0[q], u1 = r1[q];
                    c0 = fmaf(z[4 * q + 0], u0.x, c0); c1 = fmaf(z[4 * q + 0], u1.x, c1);
                    c0 = fmaf(z[4 * q + 1], u0.y, c0); c1 = fmaf(z[4 * q + 1], u1.y, c1);
                    c0 = fmaf(z[4 * q + 2], u0.z, c0); c1 = fmaf(z[4 * q + 2], u1.z, c1);
                    c0 = fmaf(z[4 * q + 3], u0.w, c0); c1 = fmaf(z[4 * q + 3], u1.w, c1);
                }
#pragma unroll
                for (uint32_t axis = 0; axis < 3; axis++) {
                    float d[2];
                    dg_axis(v, c.frac, c.scale, axis, d);
                    g[axis] = fmaf(c1, d[1], fmaf(c0, d[0], g[axis]));
                }
            }
            // x = (p + bound) / (2 bound): d / d p = d / d x / (2 bound)
#pragma unroll
            for (uint32_t d = 0; d < 3; d++) g[d] = a.inv_two_bound != 0.0f ? g[d] * a.inv_two_bound : g[d] / a.two_bound;
        }
    }
    if (a.logit) a.logit[i] = logit;
    if (a.grad) { float* o = a.grad + (size_t)i * 3; o[0] = g[0]; o[1] = g[1]; o[2] = g[2]; }
    if (a.normal) {
        // scaled by a power of two first (exact), so that neither the squares nor their sum leave fp32's range
        const float m = fmaxf(fabsf(g[0]), fmaxf(fabsf(g[1]), fabsf(g[2])));
        float nrm[3] = {0.0f, 0.0f, 0.0f};
        if (m > 0.0f && isfinite(g[0]) && isfinite(g[1]) && isfinite(g[2])) {
            int ex;
            frexpf(m, &ex);
            const float s[3] = {ldexpf(g[0], -ex), ldexpf(g[1], -ex), ldexpf(g[2], -ex)};
            const float len = sqrtf(fmaf(s[2], s[2], fmaf(s[1], s[1], s[0] * s[0])));
#pragma unroll
            for (uint32_t d = 0; d < 3; d++) nrm[d] = -s[d] / len;
        }
        float* o = a.normal + (size_t)i * 3;
        o[0] = nrm[0]; o[1] = nrm[1]; o[2] = nrm[2];
    }
}

// ------------------------------------------------------------------------------------------ vertex records
struct VrArgs {
    const float* vertices;
    const float* normal;
    const float* rgb;
    const float* extra;
    float* world;
    uint32_t* records;
    float lo[3], span[3];       // span = box_max - box_min, subtracted in fp32
    uint32_t nm1[3];
    uint32_t extra_channels, extra_stride;
    int srgb;
};

__device__ __forceinline__ uint32_t vr_byte(float c, int srgb) {
    float x = fminf(1.0f, fmaxf(0.0f, c));
    if (srgb) x = x < 0.0031308f ? 12.92f * x : 1.055f * powf(x, 0.41666f) - 0.055f;      // nerf/utils.py:43-44, as k_image_to_uint8
    return (uint32_t)(uint8_t)(int)(x * 255.0f);
}

// one lane per 32-bit word of the output: word w of vertex v
__global__ void __launch_bounds__(256) k_vertex_records(VrArgs a, uint32_t words, uint32_t total) {
    const uint32_t idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const uint32_t v = idx / words;
    uint32_t w = idx - v * words;
    uint32_t bits;
    if (w < 3) {
        // extract_geometry's float64 expression, rounded once
        const double x = (double)a.vertices[(size_t)v * 3 + w] / (double)a.nm1[w] * (double)a.span[w] + (double)a.lo[w];
        const float xf = (float)x;
        if (a.world) a.world[(size_t)v * 3 + w] = xf;
        bits = __float_as_uint(xf);
    } else {
        w -= 3;
        bool done = false;
        bits = 0;
        if (a.normal) {
            if (w < 3) { bits = __float_as_uint(a.normal[(size_t)v * 3 + w]); done = true; }
            else w -= 3;
        }
        if (!done && a.rgb) {
            if (w == 0) {
                const float* c = a.rgb + (size_t)v * 3;
                bits = vr_byte(c[0], a.srgb) | (vr_byte(c[1], a.srgb) << 8) | (vr_byte(c[2], a.srgb) << 16) | 0xff000000u;
                done = true;
            } else w -= 1;
        }
        if (!done) bits = __float_as_uint(a.extra[(size_t)v * a.extra_stride + w]);
    }
    if (a.records) a.records[idx] = bits;
}

static uint32_t vr_record_words(bool has_normal, bool has_rgb, uint32_t extra_channels) {
    return 3u + (has_normal ? 3u : 0u) + (has_rgb ? 1u : 0u) + extra_channels;
}

}  // namespace pnr

using namespace pnr;

extern "C" {

int pnr_density_gradient(const pnr_density_gradient_args* a, pnr_stream_t stream) {
    if (!a) return PNR_ERR_INVALID;
    if (a->num_levels != kDgLevels || a->gridtype > 1 || !(a->bound > 0.0f)) return PNR_ERR_UNSUPPORTED;      // the shipped 16 x 2 -> 64 -> 16 stack
    if (!a->embeddings || !a->offsets || !a->sigma0 || !a->sigma1) return PNR_ERR_INVALID;
    if (!a->logit && !a->grad && !a->normal) return PNR_ERR_INVALID;
    if (a->n == 0) return PNR_OK;
    if (!a->points) return PNR_ERR_INVALID;
    DgArgs k;
    k.points = a->points; k.n = a->n;
    k.bound = a->bound; k.two_bound = 2.0f * a->bound; k.inv_two_bound = exact_reciprocal_or_zero(2.0f * a->bound);
    k.table = a->embeddings; k.offsets = a->offsets; k.gridtype = a->gridtype;
    k.sigma0 = a->sigma0; k.sigma1 = a->sigma1;
    k.logit = a->logit; k.grad = a->grad; k.normal = a->normal;
    const LevelParams lp = make_level_params(a->num_levels, a->S, a->base_resolution);
    hipLaunchKernelGGL(k_density_gradient, dim3(cdiv(a->n, kDgBlock)), dim3(kDgBlock), 0, as_stream(stream), k, lp);
    return check_launch();
}

uint32_t pnr_mesh_vertex_record_bytes(int has_normal, int has_rgb, uint32_t extra_channels) {
    return extra_channels > (1u << 20) ? 0u : 4u * vr_record_words(has_normal != 0, has_rgb != 0, extra_channels);
}

int pnr_mesh_vertex_records(const pnr_vertex_records_args* a, pnr_stream_t stream) {
    if (!a || (!a->world && !a->records)) return PNR_ERR_INVALID;
    if (a->n[0] < 2 || a->n[1] < 2 || a->n[2] < 2) return PNR_ERR_INVALID;
    if (a->extra_channels && (!a->extra || a->extra_stride < a->extra_channels)) return PNR_ERR_INVALID;
    if (a->extra_channels > (1u << 20)) return PNR_ERR_UNSUPPORTED;
    if (reinterpret_cast<uintptr_t>(a->records) & 3) return PNR_ERR_INVALID;
    if (a->nv == 0) return PNR_OK;
    if (!a->vertices) return PNR_ERR_INVALID;
    const uint32_t words = a->records ? vr_record_words(a->normal != nullptr, a->rgb != nullptr, a->extra_channels) : 3u;
    const uint64_t total = (uint64_t)a->nv * words;
    if (total >= (1ull << 32)) return PNR_ERR_UNSUPPORTED;
    VrArgs k;
    k.vertices = a->vertices; k.normal = a->normal; k.rgb = a->rgb; k.extra = a->extra_channels ? a->extra : nullptr;
    k.world = a->world; k.records = reinterpret_cast<uint32_t*>(a->records);
    for (int d = 0; d < 3; d++) { k.lo[d] = a->box_min[d]; k.span[d] = a->box_max[d] - a->box_min[d]; k.nm1[d] = a->n[d] - 1u; }
    k.extra_channels = a->extra_channels; k.extra_stride = a->extra_stride; k.srgb = a->linear_to_srgb;
    hipLaunchKernelGGL(k_vertex_records, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, as_stream(stream), k, words, (uint32_t)total);
    return check_launch();
}

}  // extern "C"
