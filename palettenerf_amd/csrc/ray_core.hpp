// ray_core.hpp -- the pinhole ray of one pixel, shared by pnr_get_rays (raymarch.hip) and pnr_train_batch (train_batch.hip).
//
// Scalar spec (include/pnr.h, "ray generation"; the oracle's is the same): xs = ((x + 0.5) - cx) / fx, ys likewise,
// n = sqrt(fma(xs,xs, fma(ys,ys, 1))), d = (xs/n, ys/n, 1/n), rays_d[k] = fma(d2,R[k][2], fma(d1,R[k][1], d0*R[k][0])), rays_o[k] = pose[k][3].
#pragma once
#include "pnr_common.hpp"

namespace pnr {

// p: flat pixel id y*W + x; poses [.,4,4] row-major cam2world, `view` the pose to use; rays_o, rays_d [.,3], `ray` the row to write
__device__ __forceinline__ void pinhole_ray(const float* poses, size_t view, uint32_t p, uint32_t W, float fx, float fy, float cx, float cy,
                                            float* rays_o, float* rays_d, size_t ray) {
    const float xs = (((float)(p % W) + 0.5f) - cx) / fx;
    const float ys = (((float)(p / W) + 0.5f) - cy) / fy;
    const float nrm = sqrtf(fmaf(xs, xs, fmaf(ys, ys, 1.0f)));
    const float d0 = xs / nrm, d1 = ys / nrm, d2 = 1.0f / nrm;
    const float* P = poses + view * 16;
    float* o = rays_o + ray * 3;
    float* d = rays_d + ray * 3;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        d[k] = fmaf(d2, P[k * 4 + 2], fmaf(d1, P[k * 4 + 1], d0 * P[k * 4 + 0]));
        o[k] = P[k * 4 + 3];
    }
}

}  // namespace pnr
