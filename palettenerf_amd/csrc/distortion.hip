// distortion.hip -- the mip-NeRF 360 distortion loss on the ragged training rays, for gfx950 (MI355X).  include/pnr_distortion.h.
//
// Per ray, with the samples, the weights w_k = alpha_k T_k and the stop rule of the training composite (composite.hip, raymarching.cu:537-570),
// m_k the running sum of deltas[:,1] counted from the ray's first sample and d_k = deltas[k,0]:
//   dist = sum_{i,j} w_i w_j |m_i - m_j| + (1/3) sum_k d_k w_k^2 = sum_k 2 w_k (m_k Wpre_k - WMpre_k) + (1/3) d_k w_k^2
// (Wpre, WMpre: exclusive prefix sums of w and w m -- the O(n) form of the reference's loss.py:29-76), and
//   v_k = 2 (m_k (Wpre_k - Wsuf_k) + (WMsuf_k - WMpre_k)) + (2/3) d_k w_k            (= d dist / d w_k)
//   d dist / d sigma_k = d_k (v_k T_{k+1} - (2 dist - S_k)),   S_k = inclusive prefix sum of v_j w_j
// (d w_k / d sigma_k = d_k T_{k+1}, d w_j / d sigma_k = -d_k w_j behind k, and sum_j v_j w_j = 2 dist: the loss is homogeneous of degree 2 in w).
//
// The lane layout is k_composite_train_fwd_coop's: 16 lanes per ray, one SAMPLE per lane, the state in front of a group of 16 samples carried
// along, the loop over for the whole group once T < T_thresh.  A ray's 16 lanes are one DPP row, so the four steps of every prefix scan are
// row shifts (v_*_dpp row_shr:1,2,4,8: a lane without a source keeps the identity) instead of ds_bpermute round trips.  No atomics, no LDS,
// one summation order: two launches give the same bits.  The next group's three floats are fetched before the current group's scans.
#include "pnr_common.hpp"
#include "../../include/pnr_distortion.h"

namespace pnr {

constexpr uint32_t kDistBlock = 256;
constexpr uint32_t kDistLanes = 16;                         // lanes per ray: one DPP row
constexpr uint32_t kDistRays = kDistBlock / kDistLanes;     // rays per workgroup

__device__ __forceinline__ float dist_alpha(float sigma, float delta) { return 1.0f - __expf(-sigma * delta); }   // composite.hip's alpha_of

// lane q of a row takes the value of lane q - kShift of ITS row; the first kShift lanes of a row take `fill`
template <int kShift>
__device__ __forceinline__ float row_shr(float v, float fill) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(fill), __float_as_int(v), 0x110 + kShift, 0xf, 0xf, false));
}
__device__ __forceinline__ float row_last(float v) { return __shfl(v, kDistLanes - 1, kDistLanes); }

// composite.hip's three group helpers on row shifts: the same terms in the same order
__device__ __forceinline__ float row_incl_sum(float v, float& total) {
    v += row_shr<1>(v, 0.0f); v += row_shr<2>(v, 0.0f); v += row_shr<4>(v, 0.0f); v += row_shr<8>(v, 0.0f);
    total = row_last(v);
    return v;
}
__device__ __forceinline__ float row_excl_product(float v, float& total) {
    v *= row_shr<1>(v, 1.0f); v *= row_shr<2>(v, 1.0f); v *= row_shr<4>(v, 1.0f); v *= row_shr<8>(v, 1.0f);
    total = row_last(v);
    return row_shr<1>(v, 1.0f);
}
__device__ __forceinline__ float row_sum(float v) {
#pragma unroll
    for (int off = kDistLanes / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off, kDistLanes);
    return v;
}

// One group of 16 samples of a ray: what the forward and the backward both need of it.
struct DistGroup {
    float d0, Tq, after, w, m, Wpre, WMpre, wm;   // per lane: delta, T in front of the sample, 1 - alpha, weight, m, exclusive sums, w m
    float keep, msum, wtot, wmtot;                // per group: what the carried state advances by
    bool live;
};
__device__ __forceinline__ DistGroup dist_group(float sg, float d0, float d1, bool in, bool first, float T, float m, float W, float WM,
                                                float T_thresh) {
    DistGroup g;
    const float alpha = in ? dist_alpha(sg, d0) : 0.0f;
    g.d0 = d0;
    g.after = 1.0f - alpha;
    g.Tq = T * row_excl_product(g.after, g.keep);
    g.m = m + row_incl_sum((in && !first) ? d1 : 0.0f, g.msum);   // m counts from the ray's first sample: no fp32 cancellation at a far t
    g.live = in && !(g.Tq < T_thresh);                            // the sample that brings T below the threshold still counts, none behind it
    g.w = g.live ? alpha * g.Tq : 0.0f;
    g.wm = g.w * g.m;
    const float wi = row_incl_sum(g.w, g.wtot), wmi = row_incl_sum(g.wm, g.wmtot);
    g.Wpre = W + row_shr<1>(wi, 0.0f);
    g.WMpre = WM + row_shr<1>(wmi, 0.0f);
    return g;
}

struct DistRay { uint32_t index, offset, num_steps; bool empty; };
__device__ __forceinline__ DistRay dist_ray(const int32_t* __restrict__ rays, uint32_t n, uint32_t M) {
    DistRay r;
    r.index = (uint32_t)rays[(size_t)n * 3]; r.offset = (uint32_t)rays[(size_t)n * 3 + 1]; r.num_steps = (uint32_t)rays[(size_t)n * 3 + 2];
    r.empty = r.num_steps == 0 || (uint64_t)r.offset + r.num_steps > M;
    return r;
}
// the row lane q reads in the group at `base`: its own sample, or the ray's last one (stays inside the ray's rows)
__device__ __forceinline__ size_t dist_row(const DistRay& r, uint32_t base, int q) {
    const uint32_t k = base + (uint32_t)q;
    return (size_t)r.offset + (k < r.num_steps ? k : r.num_steps - 1);
}

__global__ void __launch_bounds__(kDistBlock) k_distortion_fwd(const float* __restrict__ sigmas, const float* __restrict__ deltas,
                                                               const int32_t* __restrict__ rays, uint32_t M, uint32_t N, float T_thresh,
                                                               float* __restrict__ dist, float* __restrict__ w_sum, float* __restrict__ wm_sum) {
    const uint32_t n = blockIdx.x * kDistRays + threadIdx.x / kDistLanes;
    const int q = (int)(threadIdx.x % kDistLanes);
    if (n >= N) return;   // whole 16-lane rows leave together
    const DistRay r = dist_ray(rays, n, M);
    float acc = 0, W = 0, WM = 0;
    if (!r.empty) {
        float T = 1.0f, m = 0.0f;   // the state in front of the current group
        size_t row = dist_row(r, 0, q);
        float sg = sigmas[row], d0 = deltas[row * 2], d1 = deltas[row * 2 + 1];
        for (uint32_t base = 0; base < r.num_steps && !(T < T_thresh); base += kDistLanes) {
            const float sg_c = sg, d0_c = d0, d1_c = d1;
            row = dist_row(r, base + kDistLanes, q);
            sg = sigmas[row]; d0 = deltas[row * 2]; d1 = deltas[row * 2 + 1];
            const uint32_t k = base + (uint32_t)q;
            const DistGroup g = dist_group(sg_c, d0_c, d1_c, k < r.num_steps, k == 0, T, m, W, WM, T_thresh);
            const float bi = fmaf(g.m, g.Wpre, -g.WMpre);                            // sum_{j<k} w_j (m_k - m_j)
            acc += fmaf(2.0f * g.w, bi, (1.0f / 3.0f) * g.d0 * (g.w * g.w));
            T *= g.keep; m += g.msum; W += g.wtot; WM += g.wmtot;
        }
    }
    acc = row_sum(acc);
    if (q == 0) { dist[r.index] = acc; w_sum[r.index] = W; wm_sum[r.index] = WM; }
}

// Writes the samples that count; every other element of grad_sigmas is the zero the entry filled in before the launch.
__global__ void __launch_bounds__(kDistBlock) k_distortion_bwd(const float* __restrict__ grad_dist, const float* __restrict__ sigmas,
                                                               const float* __restrict__ deltas, const int32_t* __restrict__ rays,
                                                               const float* __restrict__ dist, const float* __restrict__ w_sum,
                                                               const float* __restrict__ wm_sum, uint32_t M, uint32_t N, float T_thresh,
                                                               float* __restrict__ grad_sigmas) {
    const uint32_t n = blockIdx.x * kDistRays + threadIdx.x / kDistLanes;
    const int q = (int)(threadIdx.x % kDistLanes);
    if (n >= N) return;
    const DistRay r = dist_ray(rays, n, M);
    if (r.empty) return;
    const float gd = grad_dist[r.index], dist2 = 2.0f * dist[r.index], Wt = w_sum[r.index], WMt = wm_sum[r.index];
    float T = 1.0f, m = 0.0f, W = 0.0f, WM = 0.0f, S = 0.0f;
    size_t row = dist_row(r, 0, q);
    float sg = sigmas[row], d0 = deltas[row * 2], d1 = deltas[row * 2 + 1];
    for (uint32_t base = 0; base < r.num_steps && !(T < T_thresh); base += kDistLanes) {
        const float sg_c = sg, d0_c = d0, d1_c = d1;
        const size_t row_c = row;
        row = dist_row(r, base + kDistLanes, q);
        sg = sigmas[row]; d0 = deltas[row * 2]; d1 = deltas[row * 2 + 1];
        const uint32_t k = base + (uint32_t)q;
        const DistGroup g = dist_group(sg_c, d0_c, d1_c, k < r.num_steps, k == 0, T, m, W, WM, T_thresh);
        const float Wsuf = Wt - g.Wpre - g.w, WMsuf = WMt - g.WMpre - g.wm;
        const float v = fmaf(2.0f, fmaf(g.m, g.Wpre - Wsuf, WMsuf - g.WMpre), (2.0f / 3.0f) * g.d0 * g.w);
        float stot;
        const float Sq = S + row_incl_sum(v * g.w, stot);
        if (g.live) grad_sigmas[row_c] = gd * (g.d0 * fmaf(v, g.Tq * g.after, -(dist2 - Sq)));
        T *= g.keep; m += g.msum; W += g.wtot; WM += g.wmtot; S += stot;
    }
}

}  // namespace pnr

using namespace pnr;

extern "C" {

int pnr_distortion_forward(const float* sigmas, const float* deltas, const int32_t* rays, uint32_t M, uint32_t N, float T_thresh, float* dist,
                           float* w_sum, float* wm_sum, pnr_stream_t stream) {
    if (N == 0) return PNR_OK;
    if (!rays || !dist || !w_sum || !wm_sum) return PNR_ERR_INVALID;
    if (M > 0 && (!sigmas || !deltas)) return PNR_ERR_INVALID;
    // M == 0: every ray is empty, the kernel writes its three zeros and reads no sample
    hipLaunchKernelGGL(k_distortion_fwd, dim3(cdiv(N, kDistRays)), dim3(kDistBlock), 0, as_stream(stream), sigmas, deltas, rays, M, N, T_thresh,
                       dist, w_sum, wm_sum);
    return check_launch();
}

int pnr_distortion_backward(const float* grad_dist, const float* sigmas, const float* deltas, const int32_t* rays, const float* dist,
                            const float* w_sum, const float* wm_sum, uint32_t M, uint32_t N, float T_thresh, float* grad_sigmas,
                            pnr_stream_t stream) {
    if (N == 0 || M == 0) return PNR_OK;
    if (!grad_dist || !sigmas || !deltas || !rays || !dist || !w_sum || !wm_sum || !grad_sigmas) return PNR_ERR_INVALID;
    if (hipMemsetAsync(grad_sigmas, 0, (size_t)M * sizeof(float), as_stream(stream)) != hipSuccess) return PNR_ERR_LAUNCH;
    hipLaunchKernelGGL(k_distortion_bwd, dim3(cdiv(N, kDistRays)), dim3(kDistBlock), 0, as_stream(stream), grad_dist, sigmas, deltas, rays, dist,
                       w_sum, wm_sum, M, N, T_thresh, grad_sigmas);
    return check_launch();
}

}  // extern "C"
