// sph_core.hpp -- where a ray leaves the background sphere, as the two angles the background hash grid is indexed by.
// Shared by k_sph_from_ray (raymarch.hip) and k_background (background.hip): one body, built with -ffp-contract=off in both units, so the two
// kernels give the same bits for the same ray.
#pragma once
#include <hip/hip_runtime.h>

namespace pnr {

// reference raymarching.cu:166-201: the far root of |o + t d| = radius, then (theta, phi) of that point scaled to [-1, 1]
__device__ __forceinline__ void sph_coords_of(float ox, float oy, float oz, float dx, float dy, float dz, float radius, float& u, float& v) {
    const float RPI = 0.3183098861837907f;
    const float A = dx * dx + dy * dy + dz * dz;
    const float B = ox * dx + oy * dy + oz * dz;
    const float Cq = ox * ox + oy * oy + oz * oz - radius * radius;
    const float t = (-B + sqrtf(B * B - A * Cq)) / A;
    const float x = ox + t * dx, y = oy + t * dy, z = oz + t * dz;
    u = 2 * atan2f(sqrtf(x * x + z * z), y) * RPI - 1;
    v = atan2f(z, x) * RPI;
}

}  // namespace pnr
