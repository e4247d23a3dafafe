// lut.hip -- the back end of the palette extraction that has a closed statement, for gfx950 (include/pnr.h, "palette extraction, weight LUT"):
//   pnr_lut_weights   the Tan-2016/2018 "ASAP" palette weights of N colours against a palette of 4..16 colours -- ONE launch, float64
// (rgbsg/fastLayerDecomposition/Additive_mixing_layers_extraction.py:397-547 as palette/utils.py:235-245 calls it: the hist_weights table).
//
// One thread per point; a workgroup takes contiguous runs of 128 points, so the fp32 stores of one palette column of the LUT layout are coalesced.
// Every workgroup first rebuilds the whole hull in LDS (the prologue below: no second launch, no host pre-pass), and the per-point loop then reads
// nothing but LDS at addresses that are the same in every lane (broadcast reads, no bank conflicts):
//   order   the palette rows by L1 distance to black, a tie to the lower row: V[0] is the darkest row and a hull vertex
//   faces   every triple i < j < k of V whose plane has all other rows strictly (by more than 1e-9) on one side, in ascending (i, j, k);
//           its unit normal turned outwards.  At most 2M - 4 = 28 faces out of at most C(16,3) = 560 triples.
//   star    for every face without V[0] the inverse of the edge matrix [Vi-V0 Vj-V0 Vk-V0] (adjugate over determinant)
// A point is outside when its signed distance to some face plane exceeds 1e-8; it is then replaced by the closest point of the hull surface
// (the nearest of the closest points on the triangles: Voronoi regions of the triangle, strict <, so a tie goes to the lower face).  Its four
// weights are the barycentric coordinates in the star tetrahedron whose smallest coordinate is largest (strict >: the lower face on a tie).
// Two refusals, found by every workgroup alike and reported in info[0]: PNR_LUT_FLAT (no triple has a row off its plane) and PNR_LUT_COPLANAR
// (a supporting plane carries a fourth row within 1e-9).  float64 throughout, no atomics, every sum and minimum in a fixed order: two runs give
// the same bits.  Built with -ffp-contract=off like every unit: nothing below is fused.
#include <string.h>
#include "pnr_common.hpp"

namespace pnr {
namespace {

constexpr uint32_t kLutBlock = 128;        // points of one trip of a workgroup
constexpr uint32_t kLutMaxGrid = 1024;     // workgroups; a larger batch is walked in trips
constexpr uint32_t kLutMaxM = PNR_LUT_MAX_M, kLutMaxFaces = PNR_LUT_MAX_FACES;
constexpr uint32_t kLutTriples = kLutMaxM * kLutMaxM * kLutMaxM;      // (i, j, k) as a 12-bit code; the ascending ones are the candidates
constexpr double kPlaneEps = 1e-9, kOutsideEps = 1e-8;
static_assert(kLutMaxM == 16 && kLutMaxFaces == 2 * kLutMaxM - 4, "the triple code is three hex digits");

inline uint32_t lut_blocks(uint64_t n) { const uint64_t t = (n + kLutBlock - 1) / kLutBlock; return t < kLutMaxGrid ? (t ? (uint32_t)t : 1u) : kLutMaxGrid; }

struct LutLds {
    double V[kLutMaxM][3];             // the palette in hull order
    double key[kLutMaxM];
    double fa[kLutMaxFaces][3];        // a face: its first vertex, its two edges, its unit outward normal
    double fab[kLutMaxFaces][3];
    double fac[kLutMaxFaces][3];
    double fn[kLutMaxFaces][3];
    double finv[kLutMaxFaces][9];      // star tetrahedron of the face: the inverse edge matrix, row-major
    uint32_t fcol[kLutMaxFaces];       // the caller's columns of V0, Vi, Vj, Vk, one byte each
    uint16_t ftri[kLutMaxFaces];       // the face's triple code
    uint8_t fflip[kLutMaxFaces];
    uint8_t fstar[kLutMaxFaces];
    uint8_t order[kLutMaxM];           // hull order -> the caller's row
    uint8_t cand[kLutTriples];         // 0 no face, 1 face, 2 face with the normal turned
    int nfaces, nonflat, coplanar;
};

__device__ __forceinline__ double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// the unit normal (Vj - Vi) x (Vk - Vi); false for three collinear rows
__device__ __forceinline__ bool triple_normal(const LutLds& s, uint32_t i, uint32_t j, uint32_t k, double (&e1)[3], double (&e2)[3], double (&n)[3]) {
#pragma unroll
    for (int d = 0; d < 3; d++) {
        e1[d] = s.V[j][d] - s.V[i][d];
        e2[d] = s.V[k][d] - s.V[i][d];
    }
    n[0] = e1[1] * e2[2] - e1[2] * e2[1];
    n[1] = e1[2] * e2[0] - e1[0] * e2[2];
    n[2] = e1[0] * e2[1] - e1[1] * e2[0];
    const double len2 = dot3(n, n);
    if (!(len2 > 0.0)) return false;
    const double len = sqrt(len2);
#pragma unroll
    for (int d = 0; d < 3; d++) n[d] = n[d] / len;
    return true;
}

// The hull of the palette into LDS; returns the status (the same in every lane of every workgroup).
__device__ __forceinline__ int lut_prologue(LutLds& s, const double* __restrict__ palette, uint32_t M) {
    const uint32_t tid = threadIdx.x;
    if (tid == 0) s.nfaces = s.nonflat = s.coplanar = 0;
    if (tid < M) s.key[tid] = (fabs(palette[3 * tid]) + fabs(palette[3 * tid + 1])) + fabs(palette[3 * tid + 2]);
    __syncthreads();
    if (tid < M) {
        uint32_t rank = 0;
        for (uint32_t j = 0; j < M; j++) rank += s.key[j] < s.key[tid] || (s.key[j] == s.key[tid] && j < tid);
        for (int d = 0; d < 3; d++) s.V[rank][d] = palette[3 * tid + d];
        s.order[rank] = (uint8_t)tid;
    }
    __syncthreads();

    // ---- every ascending triple against every other row (codes from M << 8 on have i >= M: none of them is looked at) ----
    const uint32_t codes = M << 8;
    for (uint32_t t = tid; t < codes; t += kLutBlock) {
        const uint32_t i = t >> 8, j = (t >> 4) & 15u, k = t & 15u;
        uint8_t flag = 0;
        double e1[3], e2[3], n[3];
        if (i < j && j < k && k < M && triple_normal(s, i, j, k, e1, e2, n)) {
            uint32_t pos = 0, neg = 0, near = 0;
            for (uint32_t l = 0; l < M; l++) {
                if (l == i || l == j || l == k) continue;
                double r[3];
#pragma unroll
                for (int d = 0; d < 3; d++) r[d] = s.V[l][d] - s.V[i][d];
                const double dist = dot3(n, r);
                if (dist > kPlaneEps) pos++;
                else if (dist < -kPlaneEps) neg++;
                else near++;
            }
            if (pos + neg) {
                s.nonflat = 1;
                if (pos == 0 || neg == 0) {
                    if (near) s.coplanar = 1;
                    else flag = pos ? 2 : 1;           // the others in front: the normal points inwards and is turned
                }
            }
        }
        s.cand[t] = flag;
    }
    __syncthreads();

    // ---- the faces in ascending triple order: the first wave compacts 64 codes a step ----
    if (tid < PNR_WAVE) {
        uint32_t nf = 0;
        for (uint32_t base = 0; base < codes; base += PNR_WAVE) {
            const uint8_t flag = s.cand[base + tid];
            const unsigned long long mask = __ballot(flag != 0);
            const uint32_t slot = nf + (uint32_t)__popcll(mask & ((1ull << tid) - 1ull));
            if (flag && slot < kLutMaxFaces) {
                s.ftri[slot] = (uint16_t)(base + tid);
                s.fflip[slot] = flag == 2;
            }
            nf += (uint32_t)__popcll(mask);
        }
        if (tid == 0) s.nfaces = (int)nf;
    }
    __syncthreads();
    const uint32_t F = (uint32_t)s.nfaces;
    if (!s.nonflat) return PNR_LUT_FLAT;
    if (s.coplanar || F > kLutMaxFaces) return PNR_LUT_COPLANAR;       // (more than 2M - 4 faces cannot be a simplicial hull)
    if (F < 4) return PNR_LUT_FLAT;                                    // (nor can fewer than four)

    if (tid < F) {
        const uint32_t t = s.ftri[tid], i = t >> 8, j = (t >> 4) & 15u, k = t & 15u;
        double e1[3], e2[3], n[3];
        triple_normal(s, i, j, k, e1, e2, n);
        const bool flip = s.fflip[tid] != 0;
#pragma unroll
        for (int d = 0; d < 3; d++) {
            s.fa[tid][d] = s.V[i][d];
            s.fab[tid][d] = e1[d];
            s.fac[tid][d] = e2[d];
            s.fn[tid][d] = flip ? -n[d] : n[d];
        }
        s.fstar[tid] = i != 0;
        s.fcol[tid] = (uint32_t)s.order[0] | ((uint32_t)s.order[i] << 8) | ((uint32_t)s.order[j] << 16) | ((uint32_t)s.order[k] << 24);
        if (i != 0) {
            double c[3][3];                    // c[m] = column m of the edge matrix
#pragma unroll
            for (int d = 0; d < 3; d++) {
                c[0][d] = s.V[i][d] - s.V[0][d];
                c[1][d] = s.V[j][d] - s.V[0][d];
                c[2][d] = s.V[k][d] - s.V[0][d];
            }
            double r[3][3];                    // r[m] = c[m+1] x c[m+2]: row m of the adjugate
#pragma unroll
            for (int m = 0; m < 3; m++) {
                const double* u = c[(m + 1) % 3];
                const double* v = c[(m + 2) % 3];
                r[m][0] = u[1] * v[2] - u[2] * v[1];
                r[m][1] = u[2] * v[0] - u[0] * v[2];
                r[m][2] = u[0] * v[1] - u[1] * v[0];
            }
            const double det = dot3(c[0], r[0]);
#pragma unroll
            for (int m = 0; m < 3; m++)
#pragma unroll
                for (int d = 0; d < 3; d++) s.finv[tid][3 * m + d] = r[m][d] / det;
        }
    }
    __syncthreads();
    return PNR_LUT_OK;
}

// the closest point of triangle (a, a + ab, a + ac) to p as a + v ab + w ac: the Voronoi regions of the triangle in a fixed order
__device__ __forceinline__ void closest_vw(const double* a, const double* ab, const double* ac, const double (&p)[3], double& v, double& w) {
    double ap[3], bp[3], cp[3];
#pragma unroll
    for (int d = 0; d < 3; d++) {
        ap[d] = p[d] - a[d];
        bp[d] = p[d] - (a[d] + ab[d]);
        cp[d] = p[d] - (a[d] + ac[d]);
    }
    const double d1 = dot3(ab, ap), d2 = dot3(ac, ap), d3 = dot3(ab, bp), d4 = dot3(ac, bp), d5 = dot3(ab, cp), d6 = dot3(ac, cp);
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    if (d1 <= 0.0 && d2 <= 0.0) { v = 0.0; w = 0.0; }                                         // vertex a
    else if (d3 >= 0.0 && d4 <= d3) { v = 1.0; w = 0.0; }                                     // vertex b
    else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) { v = d1 / (d1 - d3); w = 0.0; }            // edge ab
    else if (d6 >= 0.0 && d5 <= d6) { v = 0.0; w = 1.0; }                                     // vertex c
    else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) { v = 0.0; w = d2 / (d2 - d6); }            // edge ac
    else if (va <= 0.0 && d4 - d3 >= 0.0 && d5 - d6 >= 0.0) { w = (d4 - d3) / ((d4 - d3) + (d5 - d6)); v = 1.0 - w; }     // edge bc
    else { const double sum = (va + vb) + vc; v = vb / sum; w = vc / sum; }                   // the inside
}

template <int SRC>
__global__ void __launch_bounds__(kLutBlock) k_lut_weights(const pnr_lut_weights_args a) {
    __shared__ LutLds s;
    const uint32_t M = a.M;
    const int status = lut_prologue(s, a.palette, M);
    const uint32_t F = (uint32_t)s.nfaces;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        uint32_t stars = 0;
        if (status == PNR_LUT_OK)
            for (uint32_t f = 0; f < F; f++) stars += s.fstar[f];
        a.info[0] = status;
        a.info[1] = status == PNR_LUT_OK ? (int32_t)F : 0;
        a.info[2] = (int32_t)stars;
        a.info[3] = 0;
    }
    if (status != PNR_LUT_OK) return;

    const uint64_t N = a.N;
    for (uint64_t n = (uint64_t)blockIdx.x * kLutBlock + threadIdx.x; n < N; n += (uint64_t)gridDim.x * kLutBlock) {
        double x[3];
        if (SRC == PNR_LUT_POINTS_BINS) {            // (code + 0.5) / 32 per channel, r most significant: exact in fp32 and in fp64
            const uint32_t code = (uint32_t)n;
            x[0] = (double)(2 * ((code >> 10) & 31u) + 1) * 0.015625;
            x[1] = (double)(2 * ((code >> 5) & 31u) + 1) * 0.015625;
            x[2] = (double)(2 * (code & 31u) + 1) * 0.015625;
        } else if (SRC == PNR_LUT_POINTS_FP32) {
            const float* p = reinterpret_cast<const float*>(a.points) + n * a.point_stride;
            x[0] = (double)p[0]; x[1] = (double)p[1]; x[2] = (double)p[2];
        } else {
            const double* p = reinterpret_cast<const double*>(a.points) + n * a.point_stride;
            x[0] = p[0]; x[1] = p[1]; x[2] = p[2];
        }
        if (a.normalize_input) {                     // palette/utils.py:237-240
#pragma unroll
            for (int d = 0; d < 3; d++) x[d] = x[d] + 0.05;
            const double norm = sqrt(dot3(x, x));
#pragma unroll
            for (int d = 0; d < 3; d++) x[d] = x[d] / norm;
        }

        // ---- outside?  then the closest point of the hull surface ----
        bool outside = false;
        for (uint32_t f = 0; f < F; f++) {
            double r[3];
#pragma unroll
            for (int d = 0; d < 3; d++) r[d] = x[d] - s.fa[f][d];
            outside |= dot3(s.fn[f], r) > kOutsideEps;
        }
        if (outside) {
            double best = 0.0, q[3] = {x[0], x[1], x[2]};
            for (uint32_t f = 0; f < F; f++) {
                double v, w, c[3], e[3];
                closest_vw(s.fa[f], s.fab[f], s.fac[f], x, v, w);
#pragma unroll
                for (int d = 0; d < 3; d++) {
                    c[d] = s.fa[f][d] + (v * s.fab[f][d] + w * s.fac[f][d]);
                    e[d] = x[d] - c[d];
                }
                const double sq = dot3(e, e);
                if (f == 0 || sq < best) { best = sq; q[0] = c[0]; q[1] = c[1]; q[2] = c[2]; }
            }
            x[0] = q[0]; x[1] = q[1]; x[2] = q[2];
        }

        // ---- the star tetrahedron whose smallest coordinate is largest ----
        double y[3], b0 = 0.0, b1 = 0.0, b2 = 0.0, b3 = 0.0, bestm = 0.0;
        uint32_t bf = 0;
        bool any = false;
#pragma unroll
        for (int d = 0; d < 3; d++) y[d] = x[d] - s.V[0][d];
        for (uint32_t f = 0; f < F; f++) {
            if (!s.fstar[f]) continue;
            const double c1 = dot3(&s.finv[f][0], y), c2 = dot3(&s.finv[f][3], y), c3 = dot3(&s.finv[f][6], y);
            const double c0 = 1.0 - ((c1 + c2) + c3);
            const double m = fmin(fmin(c0, c1), fmin(c2, c3));
            if (!any || m > bestm) { any = true; bestm = m; bf = f; b0 = c0; b1 = c1; b2 = c2; b3 = c3; }
        }
        const uint32_t cols = s.fcol[bf];
        const uint32_t k0 = cols & 255u, k1 = (cols >> 8) & 255u, k2 = (cols >> 16) & 255u, k3 = cols >> 24;
        for (uint32_t k = 0; k < M; k++) {
            const double wk = k == k0 ? b0 : k == k1 ? b1 : k == k2 ? b2 : k == k3 ? b3 : 0.0;
            if (a.weights64) a.weights64[n * M + k] = wk;
            if (a.lut32) a.lut32[SRC == PNR_LUT_POINTS_BINS ? (uint64_t)k * N + n : n * M + k] = (float)wk;
        }
    }
}

typedef decltype(&k_lut_weights<PNR_LUT_POINTS_BINS>) LutKernel;
LutKernel lut_weights_kernel(int points_format) {
    static const LutKernel table[3] = {k_lut_weights<PNR_LUT_POINTS_BINS>, k_lut_weights<PNR_LUT_POINTS_FP32>, k_lut_weights<PNR_LUT_POINTS_FP64>};
    if (points_format != PNR_LUT_POINTS_BINS && points_format != PNR_LUT_POINTS_FP32 && points_format != PNR_LUT_POINTS_FP64) return nullptr;
    return table[points_format];
}

}  // namespace

int lut_launch_geometry(const char* entry, uint64_t rows, uint32_t* workgroups, uint32_t* rows_per_trip) {
    if (strcmp(entry, "pnr_lut_weights") || rows > 0xffffffffull) return PNR_ERR_INVALID;
    *workgroups = lut_blocks(rows);
    *rows_per_trip = kLutBlock;
    return PNR_OK;
}

}  // namespace pnr

using namespace pnr;

extern "C" {

int pnr_lut_weights(const pnr_lut_weights_args* args, pnr_stream_t stream) {
    if (!args) return PNR_ERR_INVALID;
    const pnr_lut_weights_args& a = *args;
    if (!a.palette || !a.info || (!a.weights64 && !a.lut32)) return PNR_ERR_INVALID;
    if (a.M < PNR_LUT_MIN_M || a.M > PNR_LUT_MAX_M) return PNR_ERR_INVALID;
    LutKernel kernel = lut_weights_kernel(a.points_format);
    if (!kernel) return PNR_ERR_UNSUPPORTED;
    if (a.points_format == PNR_LUT_POINTS_BINS) {
        if (a.points || a.N != PNR_EXTRACT_FINE_BINS) return PNR_ERR_INVALID;
    } else {
        const uintptr_t elem = a.points_format == PNR_LUT_POINTS_FP32 ? 4u : 8u;
        if (!a.points || reinterpret_cast<uintptr_t>(a.points) % elem || a.point_stride < 3) return PNR_ERR_INVALID;
    }
    if (reinterpret_cast<uintptr_t>(a.palette) % 8 || reinterpret_cast<uintptr_t>(a.weights64) % 8 || reinterpret_cast<uintptr_t>(a.lut32) % 4 ||
        reinterpret_cast<uintptr_t>(a.info) % 4)
        return PNR_ERR_INVALID;
    // N = 0 still launches: the status of the palette is part of the answer
    hipLaunchKernelGGL(kernel, dim3(lut_blocks(a.N)), dim3(kLutBlock), 0, as_stream(stream), a);
    return check_launch();
}

}  // extern "C"
