/* pnr_distortion.h -- the mip-NeRF 360 distortion loss on the ragged training rays (additive to include/pnr.h, ABI 10; csrc/distortion.hip).
 *
 * The reference ships the loss as loss.py:29-76 (EffDistLoss, the O(n) form on a dense [B, N] weight matrix) and never calls it: on the
 * cuda_ray path the rays are ragged (rays [N,3] = index, offset, num_steps) and the weights w_k = alpha_k T_k exist only inside the composite
 * kernels.  These two entries compute it in the layout of pnr_composite_rays_train_*: 12 bytes read per sample forward, 16 moved backward,
 * no padding.
 *
 * This header is separate from pnr.h because pnr.h's entries are held to an inventory (tests/test_guard_bands_host.py) that this change does
 * not edit.  Its bindings are palettenerf_amd/_lib.py's DISTORTION_SIGNATURES, its tests tests/test_abi_distortion.py and
 * tests/test_gpu_distortion.py (the guard bands of its arrays are tested there).
 *
 * For one ray with samples k = 0 .. K-1 in the sample order and with the stop rule of pnr_composite_rays_train_forward (raymarching.cu:537-570):
 *   alpha_k = 1 - exp(-sigmas[k] * deltas[k,0]),  w_k = alpha_k T_k,  T_0 = 1,  T_{k+1} = T_k (1 - alpha_k);
 *   the sample that brings T below T_thresh still counts, the ones behind it have w = 0;
 *   num_steps == 0 or offset + num_steps > M is an empty ray: dist = w_sum = wm_sum = 0, no gradient.
 * With d_k = deltas[k,0] and m_k = deltas[1,1] + .. + deltas[k,1] (the running sum `depth` uses, counted from the ray's FIRST sample, m_0 = 0:
 * the value does not depend on where m starts, and fp32 does not cancel at a far t this way):
 *   dist   = sum_{i,j} w_i w_j |m_i - m_j| + (1/3) sum_k d_k w_k^2
 *          = sum_k 2 w_k (m_k Wpre_k - WMpre_k) + (1/3) d_k w_k^2           Wpre, WMpre: exclusive prefix sums of w and w m
 *   w_sum  = sum_k w_k,   wm_sum = sum_k w_k m_k                            (what the backward needs of the forward, with dist)
 *   v_k    = 2 (m_k (Wpre_k - Wsuf_k) + (WMsuf_k - WMpre_k)) + (2/3) d_k w_k,   Wsuf_k = w_sum - Wpre_k - w_k, likewise WMsuf
 *   d dist / d sigmas[k] = d_k (v_k T_{k+1} - (2 dist - S_k)),   S_k = inclusive prefix sum of v_j w_j
 * The second line of dist is EffDistLoss with m = t and interval = dt, per ray (its mean over rays is the caller's).  deltas gets no gradient.
 *
 * 16 lanes per ray, one sample per lane, as the 16-lane training composite; sums in scan order.  No atomics: two calls give the same bits.
 *
 * sigmas [M], deltas [M,2], rays [N,3] int32.  dist, w_sum, wm_sum and grad_dist are [N], indexed by the ray's `index` (as weights_sum is);
 * the three outputs of the forward are the backward's inputs.
 * pnr_distortion_backward writes EVERY element of grad_sigmas [M]: grad_dist[index] * d dist / d sigmas for the samples that count, zero for
 * the samples behind a stop, the samples of empty rays and the samples no ray owns (the entry clears the array in front of its one launch).
 *
 * N == 0: PNR_OK, nothing is read or written.  M == 0 with N > 0: the forward writes zeros for every ray (sigmas and deltas may be NULL then),
 * the backward has nothing to write.  Otherwise a NULL array is PNR_ERR_INVALID.  All of this is decided before anything is enqueued. */
#ifndef PNR_DISTORTION_H_
#define PNR_DISTORTION_H_
#include "pnr.h"
#ifdef __cplusplus
extern "C" {
#endif

int pnr_distortion_forward(const float* sigmas, const float* deltas, const int32_t* rays, uint32_t M, uint32_t N, float T_thresh, float* dist,
                           float* w_sum, float* wm_sum, pnr_stream_t stream);
int pnr_distortion_backward(const float* grad_dist, const float* sigmas, const float* deltas, const int32_t* rays, const float* dist,
                            const float* w_sum, const float* wm_sum, uint32_t M, uint32_t N, float T_thresh, float* grad_sigmas,
                            pnr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PNR_DISTORTION_H_ */
