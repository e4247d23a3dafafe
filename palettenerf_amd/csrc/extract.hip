// extract.hip -- the front end of the palette extraction for gfx950 (PaletteTrainer.extract_palette, palette/utils.py:1135-1200, into
// palette_extraction as far as run_kmeans' return, :167-226; include/pnr.h, "palette extraction, front end"):
//   pnr_extract_accumulate   one rendered view folded into the 3-bit and the 5-bit colour histogram -- one launch per view
//   pnr_extract_kmeans       the non-empty fine bins clustered from the heavy coarse bins, scikit-learn's Lloyd loop -- one launch, one workgroup
//
// Accumulate.  The extraction's sample weights are all 1, so a histogram is a table of integer counts: exact, independent of the order the
// pixels arrive in, reproducible bit for bit with no ordering protocol.  A workgroup keeps both tables privately in LDS as uint32 (fine 128 KB +
// coarse 2 KB: one workgroup of 1024 lanes per CU), counts its pixels there with LDS integer atomics, and at the end adds every non-zero bin to
// the 64-bit global table with one integer atomic.  The grid is persistent -- at most one workgroup per CU of the MI355X (256), each striding
// over the view -- so the flush costs at most 256 x 33 280 bins whatever the view's size, and a small view launches only the workgroups it fills.
//
// k-means.  P <= 32 768 points (bin codes, uint16) and their labels (uint8) live in LDS next to the K <= 128 centres (float64); the weights
// count / total are formed once into the workspace.  An iteration is (1) every lane labels its points (p = lane, lane + 1024, ...: argmin of
// ((x0-c0)^2 + (x1-c1)^2) + (x2-c2)^2 over the centres in index order, strict <, so a tie goes to the lowest index), (2) cluster k is summed by
// a GROUP of L = min(64, 1024 / pow2(K)) neighbouring lanes of one wave: lane j of the group walks its own contiguous slice of the points in
// order and adds those labelled k, then the L partials are combined by an xor butterfly (a fixed tree), (3) the group's first lane forms the new
// centre and its squared shift.  Everything float64, no atomics, every sum in a fixed order: two runs give the same bits.
// Built with -ffp-contract=off like every unit: nothing below is fused.
#include <string.h>
#include "pnr_common.hpp"
#include "image_core.hpp"

namespace pnr {
namespace {

constexpr uint32_t kFineBins = PNR_EXTRACT_FINE_BINS, kCoarseBins = PNR_EXTRACT_COARSE_BINS;
constexpr uint32_t kAccBlock = 1024;       // pixels of one trip of a workgroup
constexpr uint32_t kAccMaxGrid = 256;      // one workgroup per CU: the 130 KB of LDS allow no second one
constexpr uint32_t kAccLdsBytes = (kFineBins + kCoarseBins + 4) * 4;

inline uint32_t acc_blocks(uint64_t n) { const uint64_t t = (n + kAccBlock - 1) / kAccBlock; return t < kAccMaxGrid ? (uint32_t)t : kAccMaxGrid; }

// the reference's RGB_to_bin_index for one channel (palette/src/bindings.cpp:44-47)
__device__ __forceinline__ uint32_t bin_of(float c, float scale) { return (uint32_t)(fmaxf(0.0f, fminf(0.999f, c)) * scale); }

template <int FMT, int C>
__global__ void __launch_bounds__(kAccBlock) k_extract_accumulate(const pnr_extract_accumulate_args a, const uint64_t row_bytes, const int vec) {
    extern __shared__ __align__(16) uint32_t acc_lds[];
    uint32_t* fine = acc_lds;
    uint32_t* coarse = acc_lds + kFineBins;
    uint32_t* nvalid = coarse + kCoarseBins;
    for (uint32_t b = threadIdx.x; b < kFineBins + kCoarseBins + 1; b += kAccBlock) acc_lds[b] = 0u;
    __syncthreads();

    const uint64_t n = (uint64_t)a.H * a.W;
    uint32_t mine = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kAccBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kAccBlock) {
        if (!(a.weights_sum[i] > a.thresh)) continue;                 // strict; a NaN is not valid (palette/utils.py:1185)
        const uint32_t y = (uint32_t)(i / a.W), x = (uint32_t)(i - (uint64_t)y * a.W);
        float px[4];
        load_pixel<FMT, C>(reinterpret_cast<const uint8_t*>(a.pixels) + (uint64_t)y * row_bytes, x, vec != 0, px);
        float c[3];
#pragma unroll 1
        for (int k = 0; k < 3; k++) c[k] = (a.linear ? srgb_to_linear(px[k]) : px[k]) + 0.05f;      // (rolled: one copy of powf)  :1169-1172
        const float norm = sqrtf((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);                          // :1173
        uint32_t i5 = 0, i3 = 0;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float v = c[k] / norm;
            i5 = (i5 << 5) + bin_of(v, 32.0f);
            i3 = (i3 << 3) + bin_of(v, 8.0f);
        }
        atomicAdd(&fine[i5], 1u);
        atomicAdd(&coarse[i3], 1u);
        mine++;
    }
    if (mine) atomicAdd(nvalid, mine);
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < kFineBins + kCoarseBins; b += kAccBlock) {
        const uint32_t v = acc_lds[b];
        if (v) atomicAdd(reinterpret_cast<unsigned long long*>(b < kFineBins ? a.counts_fine + b : a.counts_coarse + (b - kFineBins)), (unsigned long long)v);
    }
    if (threadIdx.x == 0 && *nvalid) atomicAdd(reinterpret_cast<unsigned long long*>(a.total), (unsigned long long)*nvalid);
}

typedef decltype(&k_extract_accumulate<PNR_IMAGE_FP32, 3>) AccKernel;
LdsKernel<AccKernel>* extract_accumulate_kernel(int image_format, uint32_t C) {
#define ROW(F) {{k_extract_accumulate<F, 3>, {}}, {k_extract_accumulate<F, 4>, {}}}
    static LdsKernel<AccKernel> table[3][2] = {ROW(PNR_IMAGE_FP32), ROW(PNR_IMAGE_FP16), ROW(PNR_IMAGE_UINT8)};
#undef ROW
    if ((image_format != PNR_IMAGE_FP32 && image_format != PNR_IMAGE_FP16 && image_format != PNR_IMAGE_UINT8) || (C != 3 && C != 4)) return nullptr;
    return &table[image_format == PNR_IMAGE_FP32 ? 0 : image_format == PNR_IMAGE_FP16 ? 1 : 2][C == 4];
}

// ---------------------------------------------------------------- k-means ----------------------------------------------------------------
constexpr uint32_t kKmBlock = 1024, kKmWaves = kKmBlock / PNR_WAVE;
constexpr uint32_t kKmMaxK = PNR_EXTRACT_MAX_K;
constexpr uint32_t kKmPerLane = kFineBins / kKmBlock;      // fine bins a lane compacts: 32 neighbouring codes

struct KmLds {
    uint16_t code[kFineBins];          // the points: fine-bin codes in ascending order
    uint8_t label[kFineBins];
    double cen[2][kKmMaxK * 3];
    double wk[kKmMaxK];                // weight in cluster, from the last summation
    double red[kKmBlock];              // block sums; per-cluster squared shifts
    uint32_t heavy[kCoarseBins];
    uint32_t wave_n[kKmWaves];
    int K, changed, empty;
};
static_assert(sizeof(KmLds) <= kLdsCeiling, "the k-means state has to fit the LDS of one CU");
static_assert(kKmMaxK <= 255, "labels are bytes, 255 = none yet");

// the sum of v over the workgroup by a fixed tree, returned to every lane
__device__ __forceinline__ double block_sum(double v, double* red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t s = kKmBlock / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

__device__ __forceinline__ void point_of(uint32_t code, double (&x)[3]) {      // (code + 0.5) / 32 per channel, r most significant: exact
    x[0] = (double)(2 * ((code >> 10) & 31u) + 1) * 0.015625;
    x[1] = (double)(2 * ((code >> 5) & 31u) + 1) * 0.015625;
    x[2] = (double)(2 * (code & 31u) + 1) * 0.015625;
}

// every lane labels its points against `cen`; sets s.changed when a label differs from the one it replaces
__device__ __forceinline__ void km_label(KmLds& s, const double* cen, uint32_t P, uint32_t K) {
    bool changed = false;
    for (uint32_t p = threadIdx.x; p < P; p += kKmBlock) {
        double x[3];
        point_of(s.code[p], x);
        double best = 0.0;
        uint32_t arg = 0;
        for (uint32_t k = 0; k < K; k++) {
            const double d0 = x[0] - cen[3 * k], d1 = x[1] - cen[3 * k + 1], d2 = x[2] - cen[3 * k + 2];
            const double d = (d0 * d0 + d1 * d1) + d2 * d2;
            if (k == 0 || d < best) { best = d; arg = k; }
        }
        changed |= s.label[p] != (uint8_t)arg;
        s.label[p] = (uint8_t)arg;
    }
    if (changed) s.changed = 1;
}

// cluster sums by lane groups (see the head of the file).  The group's first lane returns true with sum = (sum w x0, sum w x1, sum w x2, sum w).
__device__ __forceinline__ bool km_sums(const KmLds& s, const double* __restrict__ wgt, uint32_t P, uint32_t K, uint32_t L, double (&sum)[4]) {
    const uint32_t k = threadIdx.x / L, j = threadIdx.x % L;
    const uint32_t slice = ((P + L - 1) / L + 3u) & ~3u;          // whole label words
    uint32_t p0 = j * slice, p1 = p0 + slice;
    if (p1 > P) p1 = P;
    if (k >= K || p0 > P) p0 = p1 = 0;
    sum[0] = sum[1] = sum[2] = sum[3] = 0.0;
    const uint32_t* words = reinterpret_cast<const uint32_t*>(s.label);
    for (uint32_t p = p0; p < p1; p += 4) {
        const uint32_t q = words[p >> 2];
#pragma unroll
        for (uint32_t b = 0; b < 4; b++) {
            if (p + b < p1 && ((q >> (8 * b)) & 0xffu) == k) {
                double x[3];
                point_of(s.code[p + b], x);
                const double w = wgt[p + b];
                sum[0] += w * x[0];
                sum[1] += w * x[1];
                sum[2] += w * x[2];
                sum[3] += w;
            }
        }
    }
    for (uint32_t off = 1; off < L; off <<= 1) {
#pragma unroll
        for (int c = 0; c < 4; c++) sum[c] += __shfl_xor(sum[c], (int)off, PNR_WAVE);
    }
    return j == 0 && k < K;
}

__global__ void __launch_bounds__(kKmBlock) k_extract_kmeans(const pnr_extract_kmeans_args a) {
    extern __shared__ __align__(16) unsigned char km_raw[];
    KmLds& s = *reinterpret_cast<KmLds*>(km_raw);
    const uint32_t tid = threadIdx.x, lane = tid & (PNR_WAVE - 1), wave = tid / PNR_WAVE;
    double* wgt = reinterpret_cast<double*>(a.workspace);
    const double total = (double)*a.total;

    // ---- the K initial centres: the coarse bins heavier than tau, in ascending bin order (palette/utils.py:209-215) ----
    if (tid < kCoarseBins) s.heavy[tid] = total > 0.0 && (double)a.counts_coarse[tid] / total > a.tau;
    __syncthreads();
    if (tid == 0) {
        uint32_t K = 0;
        for (uint32_t b = 0; b < kCoarseBins; b++) {
            if (!s.heavy[b]) continue;
            if (K < kKmMaxK)
                for (int d = 0; d < 3; d++) s.cen[0][3 * K + d] = (double)(2 * ((b >> (6 - 3 * d)) & 7u) + 1) * 0.0625;     // (c + 0.5) / 8
            K++;
        }
        s.K = (int)K;
    }
    // ---- the P points: the non-empty fine bins in ascending code order, weight count / total (:217-222) ----
    uint32_t n_mine = 0;
    for (uint32_t i = 0; i < kKmPerLane; i++) n_mine += a.counts_fine[tid * kKmPerLane + i] != 0;
    const uint32_t incl = (uint32_t)wave_inclusive_scan((int)n_mine);
    if (lane == PNR_WAVE - 1) s.wave_n[wave] = incl;
    __syncthreads();
    uint32_t first = incl - n_mine, P = 0;
    for (uint32_t w = 0; w < kKmWaves; w++) {
        if (w < wave) first += s.wave_n[w];
        P += s.wave_n[w];
    }
    for (uint32_t i = 0; i < kKmPerLane; i++) {
        const uint32_t code = tid * kKmPerLane + i;
        const uint64_t c = a.counts_fine[code];
        if (c) {
            s.code[first] = (uint16_t)code;
            wgt[first] = (double)c / total;
            first++;
        }
    }
    for (uint32_t p = tid; p < kFineBins; p += kKmBlock) s.label[p] = 0xffu;
    const uint32_t K = (uint32_t)s.K;
    int status = PNR_EXTRACT_OK, stop = PNR_EXTRACT_STOP_CAP;
    uint32_t iters = 0, cur = 0;
    if (K == 0) status = PNR_EXTRACT_NO_CENTER;
    else if (K > kKmMaxK) status = PNR_EXTRACT_TOO_MANY;
    else if (P < K) status = PNR_EXTRACT_FEW_POINTS;
    __syncthreads();       // the points and their weights are in place

    if (status == PNR_EXTRACT_OK) {
        // ---- tol * mean(var(X, axis=0)), unweighted over the points (sklearn _tolerance) ----
        double m[3] = {0.0, 0.0, 0.0}, v[3] = {0.0, 0.0, 0.0};
        for (uint32_t p = tid; p < P; p += kKmBlock) {
            double x[3];
            point_of(s.code[p], x);
            for (int d = 0; d < 3; d++) m[d] += x[d];
        }
        for (int d = 0; d < 3; d++) m[d] = block_sum(m[d], s.red) / (double)P;
        for (uint32_t p = tid; p < P; p += kKmBlock) {
            double x[3];
            point_of(s.code[p], x);
            for (int d = 0; d < 3; d++) v[d] += (x[d] - m[d]) * (x[d] - m[d]);
        }
        for (int d = 0; d < 3; d++) v[d] = block_sum(v[d], s.red) / (double)P;
        const double tol = ((v[0] + v[1]) + v[2]) / 3.0 * a.tol;

        uint32_t Kp = 1;
        while (Kp < K) Kp <<= 1;
        const uint32_t L = kKmBlock / Kp < PNR_WAVE ? kKmBlock / Kp : PNR_WAVE;

        for (uint32_t it = 0; it < a.max_iter; it++) {
            if (tid == 0) s.changed = s.empty = 0;
            __syncthreads();
            km_label(s, s.cen[cur], P, K);
            __syncthreads();
            double sum[4];
            if (km_sums(s, wgt, P, K, L, sum)) {
                const uint32_t k = tid / L;
                s.wk[k] = sum[3];
                double shift = 0.0;
                if (sum[3] > 0.0) {
                    const double alpha = 1.0 / sum[3];                         // sklearn _average_centers: the sums times 1 / weight
                    for (int d = 0; d < 3; d++) {
                        const double c = sum[d] * alpha, e = c - s.cen[cur][3 * k + d];
                        s.cen[cur ^ 1][3 * k + d] = c;
                        shift += e * e;
                    }
                } else {
                    s.empty = 1;
                }
                s.red[k] = shift;
            }
            __syncthreads();
            const bool empty = s.empty != 0, changed = s.changed != 0;
            double shift = 0.0;
            for (uint32_t k = 0; k < K; k++) shift += s.red[k];
            __syncthreads();       // the flags and the shifts are read: the next iteration may write them
            if (empty) { status = PNR_EXTRACT_EMPTIED; break; }         // the centres this iteration started from stay; the host goes on
            cur ^= 1;
            iters = it + 1;
            if (!changed) { stop = PNR_EXTRACT_STOP_LABELS; break; }
            if (shift <= tol) { stop = PNR_EXTRACT_STOP_SHIFT; break; }
        }
        if (status == PNR_EXTRACT_OK && stop != PNR_EXTRACT_STOP_LABELS) {     // labels of the final centres (sklearn: "rerun E-step")
            km_label(s, s.cen[cur], P, K);
            __syncthreads();
            double sum[4];
            if (km_sums(s, wgt, P, K, L, sum)) s.wk[tid / L] = sum[3];
            __syncthreads();
        }
    }

    // ---- out: centres and weights by descending weight, ties to the lower cluster index (:159-165); after an emptied cluster in cluster order ----
    if (status == PNR_EXTRACT_OK || status == PNR_EXTRACT_EMPTIED) {
        if (tid < K) {
            uint32_t rank = tid;
            if (status == PNR_EXTRACT_OK) {
                rank = 0;
                for (uint32_t j = 0; j < K; j++) rank += s.wk[j] > s.wk[tid] || (s.wk[j] == s.wk[tid] && j < tid);
            }
            for (int d = 0; d < 3; d++) a.centers[3 * rank + d] = s.cen[cur][3 * tid + d];
            a.center_weights[rank] = status == PNR_EXTRACT_OK ? s.wk[tid] : 0.0;
        }
        if (a.labels)
            for (uint32_t p = tid; p < P; p += kKmBlock) a.labels[p] = status == PNR_EXTRACT_OK ? (int32_t)s.label[p] : -1;
    }
    if (tid == 0) {
        a.info[0] = (int32_t)K;
        a.info[1] = (int32_t)P;
        a.info[2] = (int32_t)iters;
        a.info[3] = stop;
        a.info[4] = status;
        a.info[5] = a.info[6] = a.info[7] = 0;
    }
}

}  // namespace

int extract_launch_geometry(const char* entry, uint64_t rows, uint32_t* workgroups, uint32_t* rows_per_trip) {
    if (strcmp(entry, "pnr_extract_accumulate")) return PNR_ERR_INVALID;
    *workgroups = acc_blocks(rows);
    *rows_per_trip = kAccBlock;
    return PNR_OK;
}

}  // namespace pnr

using namespace pnr;

extern "C" {

int pnr_extract_accumulate(const pnr_extract_accumulate_args* args, pnr_stream_t stream) {
    if (!args) return PNR_ERR_INVALID;
    const pnr_extract_accumulate_args& a = *args;
    LdsKernel<AccKernel>* kernel = extract_accumulate_kernel(a.image_format, a.channels);
    if (!kernel) return PNR_ERR_UNSUPPORTED;
    if (a.H == 0 || a.W == 0) return PNR_OK;
    if (!a.weights_sum || !a.pixels || !a.counts_coarse || !a.counts_fine || !a.total) return PNR_ERR_INVALID;
    const uint32_t elem = a.image_format == PNR_IMAGE_FP32 ? 4u : a.image_format == PNR_IMAGE_FP16 ? 2u : 1u;
    const uint64_t row_bytes = a.row_stride_bytes ? a.row_stride_bytes : (uint64_t)a.W * a.channels * elem;
    const uintptr_t base = reinterpret_cast<uintptr_t>(a.pixels);
    if (row_bytes < (uint64_t)a.W * a.channels * elem || row_bytes % elem || base % elem) return PNR_ERR_INVALID;
    const uint32_t pixel = 4 * elem;      // one request per RGBA pixel where base and rows allow it
    const int vec = a.channels == 4 && base % pixel == 0 && row_bytes % pixel == 0;
    if (!kernel->raise_lds()) return PNR_ERR_LAUNCH;
    hipLaunchKernelGGL(kernel->fn, dim3(acc_blocks((uint64_t)a.H * a.W)), dim3(kAccBlock), kAccLdsBytes, as_stream(stream), a, row_bytes, vec);
    return check_launch();
}

uint64_t pnr_extract_kmeans_workspace_bytes(void) { return (uint64_t)kFineBins * sizeof(double); }

int pnr_extract_kmeans(const pnr_extract_kmeans_args* args, pnr_stream_t stream) {
    if (!args) return PNR_ERR_INVALID;
    const pnr_extract_kmeans_args& a = *args;
    if (!a.counts_coarse || !a.counts_fine || !a.total || !a.centers || !a.center_weights || !a.info || !a.workspace) return PNR_ERR_INVALID;
    if (a.workspace_bytes < pnr_extract_kmeans_workspace_bytes() || reinterpret_cast<uintptr_t>(a.workspace) % 8) return PNR_ERR_INVALID;
    if (a.max_iter == 0 || !(a.tau >= 0.0) || !(a.tol >= 0.0)) return PNR_ERR_INVALID;
    if (!raise_lds<k_extract_kmeans>()) return PNR_ERR_LAUNCH;
    hipLaunchKernelGGL(k_extract_kmeans, dim3(1), dim3(kKmBlock), sizeof(KmLds), as_stream(stream), a);
    return check_launch();
}

}  // extern "C"
