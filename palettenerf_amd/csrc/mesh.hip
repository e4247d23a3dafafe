// mesh.hip -- marching cubes over a device-resident density volume, and the lattice the volume is sampled on, as HIP for gfx950.
//
// What it replaces is the tail of the reference's Trainer.save_mesh (nerf/utils.py:187-217, :633-653): extract_fields builds blocks of lattice
// points on the host side with linspace / meshgrid / cat, reads every block's densities back, and PyMCubes walks the volume on the CPU.  Here the
// volume stays on the device (pnr_lattice_points below hands the field its points in chunks; the field's own kernels fill the volume) and
// the surface is a stream compaction of the kind frame.hip and occupancy.hip already do: count, one scan launch, write.  The host reads two counts.
//
// Order is the contract (include/pnr.h): one vertex per straddling lattice edge, ascending by (point index * 3 + axis); triangles by cell in C
// order, then in table order.  Both follow from the work layout: a workgroup owns 256 CONSECUTIVE lattice points (thread t the t-th), a cell is
// owned by its low corner, and ranks are block offset (the scan launch) + rank within the block (wave64 prefix sums).  No device-wide atomics:
// two runs give the same bits.
//
//   count :  k_mc_classify  u -> per point: three straddle flags (into the workspace) ; per block: vertices, triangles
//            k_mc_scan      one workgroup: exclusive scan of both block arrays in place, totals -> counts[2]
//            k_mc_rank      per point: vertex rank of its first edge into the upper 29 bits of its workspace word (3 * 512^3 < 2^29)
//   emit  :  k_mc_emit      per point: its <= 3 vertices; per cell: case (eight reads of u; neighbours of a block's points are its own rows and
//                           the two next rows / planes, which the caches hold), <= 5 triangles, vertex ids from the eight neighbours' words
// The case table is generated (gen_mc_tables.py -> mc_tables.inc); pnr_mesh_case_triangles lets host code and tests read the very table the kernel uses.
#include "mesh_core.hpp"

namespace pnr {

#define PNR_MC_TABLE static const
namespace mc_host {
#include "mc_tables.inc"
}
#undef PNR_MC_TABLE
#define PNR_MC_TABLE __device__ static const
namespace mc_dev {
#include "mc_tables.inc"
}
#undef PNR_MC_TABLE

constexpr uint32_t kMcBlock = 256;        // lattice points per workgroup = threads

struct McGeom {
    uint32_t nx, ny, nz, total, nblk;
};
struct McWorkspace {
    uint32_t* code;      // [total]  bits 0..2: straddle flags of the point's +x, +y, +z edges; bits 3..31: rank of its first vertex
    int32_t* blk_v;      // [nblk]   vertices per block, then exclusive offsets
    int32_t* blk_t;      // [nblk]   triangles per block, then exclusive offsets
};

static inline uint64_t mc_align256(uint64_t v) { return (v + 255) & ~(uint64_t)255; }
static bool mc_geom(uint32_t nx, uint32_t ny, uint32_t nz, McGeom* g) {
    if (nx < 2 || ny < 2 || nz < 2 || nx > kLatticeMaxAxis || ny > kLatticeMaxAxis || nz > kLatticeMaxAxis) return false;
    g->nx = nx; g->ny = ny; g->nz = nz; g->total = nx * ny * nz; g->nblk = cdiv(g->total, kMcBlock);
    return true;
}
static uint64_t mc_bytes(const McGeom& g) { return mc_align256((uint64_t)g.total * 4) + 2 * mc_align256((uint64_t)g.nblk * 4); }
static bool mc_carve(const McGeom& g, const void* workspace, uint64_t bytes, McWorkspace* w) {
    if (!workspace || bytes < mc_bytes(g) || (reinterpret_cast<uintptr_t>(workspace) & 255)) return false;
    unsigned char* p = static_cast<unsigned char*>(const_cast<void*>(workspace));
    w->code = reinterpret_cast<uint32_t*>(p); p += mc_align256((uint64_t)g.total * 4);
    w->blk_v = reinterpret_cast<int32_t*>(p); p += mc_align256((uint64_t)g.nblk * 4);
    w->blk_t = reinterpret_cast<int32_t*>(p);
    return true;
}

// ------------------------------------------------------------------------------------------ lattice points
__global__ void __launch_bounds__(256) k_lattice_points(LatticeGeom g, uint32_t first, uint32_t count, float* __restrict__ pts) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    float p[3];
    lattice_point(g, first + i, p);
    float* o = pts + (size_t)i * 3;
    o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
}

// ------------------------------------------------------------------------------------------ marching cubes
struct McPoint {
    uint32_t x, y, z;
    uint32_t flags;      // straddle flags of the +x, +y, +z edges
    uint32_t ntri;       // triangles of the cell this point is the low corner of
    uint32_t mc_case;
};

// Everything a thread knows about its lattice point from u alone.  Reads stay inside the volume: a neighbour is read only where the point's
// coordinate on that axis is below n - 1.
__device__ __forceinline__ McPoint mc_point(const float* __restrict__ u, const McGeom& g, uint32_t i, float thr) {
    McPoint p;
    p.z = i % g.nz;
    const uint32_t xy = i / g.nz;
    p.y = xy % g.ny; p.x = xy / g.ny;
    const bool hx = p.x + 1 < g.nx, hy = p.y + 1 < g.ny, hz = p.z + 1 < g.nz;
    const uint32_t sy = g.nz, sx = g.ny * g.nz;
    const bool in0 = u[i] > thr;
    p.flags = 0; p.ntri = 0; p.mc_case = 0;
    if (hx && hy && hz) {
        // corner c = x + 2 y + 4 z
        uint32_t c = in0 ? 1u : 0u;
        c |= (u[i + sx] > thr) ? 2u : 0u;
        c |= (u[i + sy] > thr) ? 4u : 0u;
        c |= (u[i + sx + sy] > thr) ? 8u : 0u;
        c |= (u[i + 1] > thr) ? 16u : 0u;
        c |= (u[i + sx + 1] > thr) ? 32u : 0u;
        c |= (u[i + sy + 1] > thr) ? 64u : 0u;
        c |= (u[i + sx + sy + 1] > thr) ? 128u : 0u;
        p.mc_case = c;
        p.ntri = mc_dev::MC_NTRI[c];
        p.flags = (((c >> 1) ^ c) & 1u) | ((((c >> 2) ^ c) & 1u) << 1) | ((((c >> 4) ^ c) & 1u) << 2);
    } else {
        if (hx && (u[i + sx] > thr) != in0) p.flags |= 1u;
        if (hy && (u[i + sy] > thr) != in0) p.flags |= 2u;
        if (hz && (u[i + 1] > thr) != in0) p.flags |= 4u;
    }
    return p;
}

// exclusive rank of v within the 256-thread workgroup, in thread order
__device__ __forceinline__ int block_exclusive(int v, int* wsum /* [4] */) {
    const int incl = wave_inclusive_scan(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = incl;
    __syncthreads();
    int off = incl - v;
    for (int w = 0; w < (int)(threadIdx.x >> 6); w++) off += wsum[w];
    return off;
}

__global__ void __launch_bounds__(256) k_mc_classify(const float* __restrict__ u, McGeom g, float thr, McWorkspace w) {
    __shared__ int wv[4], wt[4];
    const uint32_t i = blockIdx.x * kMcBlock + threadIdx.x;
    int nv = 0, nt = 0;
    if (i < g.total) {
        const McPoint p = mc_point(u, g, i, thr);
        w.code[i] = p.flags;
        nv = __popc(p.flags); nt = (int)p.ntri;
    }
    for (int off = PNR_WAVE / 2; off > 0; off >>= 1) { nv += __shfl_xor(nv, off, PNR_WAVE); nt += __shfl_xor(nt, off, PNR_WAVE); }
    if ((threadIdx.x & 63) == 0) { wv[threadIdx.x >> 6] = nv; wt[threadIdx.x >> 6] = nt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        w.blk_v[blockIdx.x] = wv[0] + wv[1] + wv[2] + wv[3];
        w.blk_t[blockIdx.x] = wt[0] + wt[1] + wt[2] + wt[3];
    }
}

// one workgroup: exclusive scans of the two block arrays in place (blockIdx.x = 0: vertices, 1: triangles), totals to counts
__global__ void __launch_bounds__(1024) k_mc_scan(McWorkspace w, uint32_t nblk, int32_t* __restrict__ counts) {
    __shared__ int wsum[16];
    __shared__ int carry;
    int32_t* b = blockIdx.x == 0 ? w.blk_v : w.blk_t;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t base = 0; base < nblk; base += 1024) {
        const uint32_t i = base + threadIdx.x;
        const int v = i < nblk ? b[i] : 0;
        const int incl = wave_inclusive_scan(v);
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int off = carry;
        for (int k = 0; k < wave; k++) off += wsum[k];
        if (i < nblk) b[i] = off + incl - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry = off + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) counts[blockIdx.x] = carry;
}

__global__ void __launch_bounds__(256) k_mc_rank(McGeom g, McWorkspace w) {
    __shared__ int wsum[4];
    const uint32_t i = blockIdx.x * kMcBlock + threadIdx.x;
    const uint32_t flags = i < g.total ? w.code[i] : 0u;
    const int rank = w.blk_v[blockIdx.x] + block_exclusive(__popc(flags), wsum);
    if (i < g.total) w.code[i] = ((uint32_t)rank << 3) | flags;
}

// vertex id of the lattice edge (point q, axis) from q's workspace word
__device__ __forceinline__ int32_t mc_vertex_id(uint32_t code, uint32_t axis) {
    return (int32_t)((code >> 3) + __popc(code & ((1u << axis) - 1u)));
}

__global__ void __launch_bounds__(256) k_mc_emit(const float* __restrict__ u, McGeom g, float thr, McWorkspace w, float* __restrict__ vertices,
                                                 uint32_t cap_v, int32_t* __restrict__ triangles, uint32_t cap_t) {
    __shared__ int wsum[4];
    const uint32_t i = blockIdx.x * kMcBlock + threadIdx.x;
    const bool live = i < g.total;
    McPoint p = {};
    if (live) p = mc_point(u, g, i, thr);
    const uint32_t stride[3] = {g.ny * g.nz, g.nz, 1u};
    if (p.flags) {
        uint32_t id = w.code[i] >> 3;
        const float u0 = u[i];
        const float base[3] = {(float)p.x, (float)p.y, (float)p.z};
#pragma unroll
        for (uint32_t axis = 0; axis < 3; axis++) {
            if (!(p.flags & (1u << axis))) continue;
            const float u1 = u[i + stride[axis]];
            float t = (thr - u0) / (u1 - u0);
            if (!isfinite(t)) t = 0.5f;
            t = fminf(1.0f, fmaxf(0.0f, t));
            if (id < cap_v) {
                float* o = vertices + (size_t)id * 3;
#pragma unroll
                for (uint32_t d = 0; d < 3; d++) o[d] = d == axis ? base[d] + t : base[d];
            }
            id++;
        }
    }
    uint32_t tri = (uint32_t)(w.blk_t[blockIdx.x] + block_exclusive((int)p.ntri, wsum));
    for (uint32_t k = 0; k < p.ntri; k++, tri++) {
        if (tri >= cap_t) break;
        int32_t* o = triangles + (size_t)tri * 3;
#pragma unroll
        for (uint32_t c = 0; c < 3; c++) {
            // edge e = axis * 4 + (offsets of the other two axes, lower axis in bit 0): a lattice edge of the point q = p + offsets
            const uint32_t e = mc_dev::MC_TRI[p.mc_case][k * 3 + c], axis = e >> 2, o0 = e & 1u, o1 = (e >> 1) & 1u;
            const uint32_t q = i + o0 * (axis == 0 ? stride[1] : stride[0]) + o1 * (axis == 2 ? stride[1] : stride[2]);
            o[c] = mc_vertex_id(w.code[q], axis);
        }
    }
}

}  // namespace pnr

using namespace pnr;

extern "C" {

int pnr_lattice_points(const float* box_min, const float* box_max, const uint32_t* n, uint64_t first, uint32_t count, float* points, pnr_stream_t stream) {
    LatticeGeom g;
    if (!make_lattice(box_min, box_max, n, &g) || !points || first + (uint64_t)count > lattice_total(g)) return PNR_ERR_INVALID;
    if (count == 0) return PNR_OK;
    hipLaunchKernelGGL(k_lattice_points, dim3(cdiv(count, 256)), dim3(256), 0, as_stream(stream), g, (uint32_t)first, count, points);
    return check_launch();
}

int pnr_mesh_case_triangles(uint32_t mc_case, uint8_t* edges) {
    if (mc_case > 255) return PNR_ERR_INVALID;
    if (edges) for (int k = 0; k < 15; k++) edges[k] = mc_host::MC_TRI[mc_case][k];
    return mc_host::MC_NTRI[mc_case];
}

uint64_t pnr_mesh_workspace_bytes(uint32_t nx, uint32_t ny, uint32_t nz) {
    McGeom g;
    return mc_geom(nx, ny, nz, &g) ? mc_bytes(g) : 0;
}

int pnr_mesh_count(const float* u, uint32_t nx, uint32_t ny, uint32_t nz, float threshold, void* workspace, uint64_t workspace_bytes, int32_t* counts,
                   pnr_stream_t stream) {
    McGeom g; McWorkspace w;
    if (!u || !counts || !mc_geom(nx, ny, nz, &g) || !mc_carve(g, workspace, workspace_bytes, &w)) return PNR_ERR_INVALID;
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(k_mc_classify, dim3(g.nblk), dim3(256), 0, s, u, g, threshold, w);
    hipLaunchKernelGGL(k_mc_scan, dim3(2), dim3(1024), 0, s, w, g.nblk, counts);
    hipLaunchKernelGGL(k_mc_rank, dim3(g.nblk), dim3(256), 0, s, g, w);
    return check_launch();
}

int pnr_mesh_emit(const float* u, uint32_t nx, uint32_t ny, uint32_t nz, float threshold, const void* workspace, uint64_t workspace_bytes,
                  float* vertices, uint32_t cap_vertices, int32_t* triangles, uint32_t cap_triangles, pnr_stream_t stream) {
    McGeom g; McWorkspace w;
    if (!u || !mc_geom(nx, ny, nz, &g) || !mc_carve(g, workspace, workspace_bytes, &w)) return PNR_ERR_INVALID;
    if ((cap_vertices && !vertices) || (cap_triangles && !triangles)) return PNR_ERR_INVALID;
    if (cap_vertices == 0 && cap_triangles == 0) return PNR_OK;
    hipLaunchKernelGGL(k_mc_emit, dim3(g.nblk), dim3(256), 0, as_stream(stream), u, g, threshold, w, vertices, cap_vertices, triangles, cap_triangles);
    return check_launch();
}

}  // extern "C"
