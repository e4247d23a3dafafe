// pnr_common.hpp -- device-side scalar helpers and launch plumbing shared by the gfx950 kernels.
//
// Canonical scalar spec (DESIGN.md "Scalar semantics"): IEEE fp32, translation units are built
// with -ffp-contract=off, and every contraction the reference's nvcc build performs is written
// as an explicit fmaf().  Wavefront width is 64 everywhere.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include "../../include/pnr.h"

#define PNR_WAVE 64

namespace pnr {

inline int check_launch() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? PNR_OK : PNR_ERR_LAUNCH;
}
inline hipStream_t as_stream(pnr_stream_t s) { return reinterpret_cast<hipStream_t>(s); }
inline uint32_t cdiv(uint32_t a, uint32_t b) { return (a + b - 1) / b; }

// pnr_launch_geometry (launch_geometry.hip): every translation unit whose entries launch a capped grid answers for them here, through the very
// helper its launcher calls.  PNR_OK and both outputs written for one of the unit's entries, PNR_ERR_INVALID otherwise (not its name, or more
// rows than the entry's 32-bit row count can express).
int heads_launch_geometry(const char* entry, uint64_t rows, uint32_t* workgroups, uint32_t* rows_per_trip);    // palette_heads.hip
int smooth_launch_geometry(const char* entry, uint64_t rows, uint32_t* workgroups, uint32_t* rows_per_trip);   // palette_smooth.hip
int shade_launch_geometry(const char* entry, uint64_t rows, uint32_t* workgroups, uint32_t* rows_per_trip);    // palette_train.hip
int field_launch_geometry(const char* entry, uint64_t rows, uint32_t* workgroups, uint32_t* rows_per_trip);    // field.hip
int mlp_launch_geometry(const char* entry, uint64_t rows, uint32_t* workgroups, uint32_t* rows_per_trip);      // mlp.hip
int occupancy_launch_geometry(const char* entry, uint64_t rows, uint32_t* workgroups, uint32_t* rows_per_trip);   // occupancy.hip
int extract_launch_geometry(const char* entry, uint64_t rows, uint32_t* workgroups, uint32_t* rows_per_trip);     // extract.hip
int lut_launch_geometry(const char* entry, uint64_t rows, uint32_t* workgroups, uint32_t* rows_per_trip);         // lut.hip

// One process may drive several GPUs: function attributes and events belong to a device, so one-time set-up is tracked per device id.
constexpr int kMaxDevices = 64;
inline int current_device() { int d = 0; if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= kMaxDevices) d = 0; return d; }
// Host launch path.  An entry point with several instantiations of its kernel has one selector, `<entry>_kernel(run-time arguments)`: a pure function
// that reads the kernel out of a static table (or a short chain of returns) -- the table IS the set of compiled instantiations, nullptr = there is none
// (PNR_ERR_UNSUPPORTED) -- and after it one launch statement.  A kernel that takes more dynamic LDS than the 64 KiB default is held as an LdsKernel:
// the once-per-device "limit raised" flags live beside the pointer, and the limit goes to a fixed ceiling per kernel (all of a gfx950 workgroup's
// LDS, or the kernel's own constant), never to the size one call happened to ask for.
constexpr uint32_t kLdsCeiling = 160 * 1024;
template <typename F>
struct LdsKernel {
    F fn;
    bool raised[kMaxDevices];
    bool raise_lds(uint32_t ceiling = kLdsCeiling) {   // false = the runtime refused
        const int d = current_device();
        if (raised[d]) return true;
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ceiling) != hipSuccess) return false;
        return raised[d] = true;
    }
};
// ... and for a kernel named in the source, the same keyed on the kernel itself: raise_lds<k_foo<1>>(ceiling)
template <auto K>
inline bool raise_lds(uint32_t ceiling = kLdsCeiling) {
    static LdsKernel<decltype(K)> kernel = {K, {}};
    return kernel.raise_lds(ceiling);
}

__device__ __forceinline__ float clampf(float x, float lo, float hi) { return fminf(hi, fmaxf(lo, x)); }
__device__ __forceinline__ float signf(float x) { return copysignf(1.0f, x); }

// 10-bit-per-axis bit interleave (reference raymarching.cu:59-84)
__host__ __device__ __forceinline__ uint32_t spread3(uint32_t v) {
    v = (v * 0x00010001u) & 0xFF0000FFu;
    v = (v * 0x00000101u) & 0x0F00F00Fu;
    v = (v * 0x00000011u) & 0xC30C30C3u;
    v = (v * 0x00000005u) & 0x49249249u;
    return v;
}
__host__ __device__ __forceinline__ uint32_t morton3(uint32_t x, uint32_t y, uint32_t z) {
    return spread3(x) | (spread3(y) << 1) | (spread3(z) << 2);
}
__host__ __device__ __forceinline__ uint32_t gather3(uint32_t x) {
    x &= 0x49249249u;
    x = (x | (x >> 2)) & 0xc30c30c3u;
    x = (x | (x >> 4)) & 0x0f00f00fu;
    x = (x | (x >> 8)) & 0xff0000ffu;
    x = (x | (x >> 16)) & 0x0000ffffu;
    return x;
}

// cascade level selectors (reference raymarching.cu:45-57)
__device__ __forceinline__ int mip_from_pos(float x, float y, float z, float max_cascade) {
    const float mx = fmaxf(fabsf(x), fmaxf(fabsf(y), fabsf(z)));
    int e;
    frexpf(mx, &e);
    return (int)fminf(max_cascade - 1.0f, fmaxf(0.0f, (float)e));
}
__device__ __forceinline__ int mip_from_dt(float dt, float H, float max_cascade) {
    const float mx = (dt * H) * 0.5f;  // the reference multiplies by a double 0.5: exact either way
    int e;
    frexpf(mx, &e);
    return (int)fminf(max_cascade - 1.0f, fmaxf(0.0f, (float)e));
}

// Eight independent global loads issued back to back, each returning into registers of its own.  On gfx950 a load whose destination
// overlaps its own address registers (`global_load_dwordx2 v[6:7], v[6:7], off` -- what the compiler writes once registers are scarce) is
// slow: the lookup launch of the frame loop took 75.6 instead of 65.6 us with otherwise identical code ("March: the hosted
// tail").  All eight addresses are formed first (one empty asm statement with all of them as operands pins that point; it also hides where
// a pointer came from, hence the address-space cast: without it the loads become flat_load), nothing is scheduled into the group, and the
// addresses stay alive past the loads.
typedef float f32x2 __attribute__((ext_vector_type(2)));   // (built-in vector types: a load through an address-space pointer needs no operator=)
typedef float f32x4 __attribute__((ext_vector_type(4)));
template <typename T>
struct GlobalPtr { typedef const T __attribute__((address_space(1))) * type; };
template <typename T>
__device__ __forceinline__ void load8_fresh(const T* (&p)[8], T (&v)[8]) {
    asm volatile("" : "+v"(p[0]), "+v"(p[1]), "+v"(p[2]), "+v"(p[3]), "+v"(p[4]), "+v"(p[5]), "+v"(p[6]), "+v"(p[7]));
#pragma unroll
    for (int i = 0; i < 8; i++) v[i] = *(typename GlobalPtr<T>::type)(uintptr_t)p[i];
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" :: "v"(p[0]), "v"(p[1]), "v"(p[2]), "v"(p[3]), "v"(p[4]), "v"(p[5]), "v"(p[6]), "v"(p[7]));
}

// 16 bytes per lane from global memory straight into LDS (global_load_lds_dwordx4: no staging registers, no ds_write pass).  The LDS
// destination of a wave is its first lane's address + lane x 16, so `lds` must be lane-linear -- a plain copy loop over float4 indices is.
// Completion: s_waitcnt vmcnt(0) (lds_copy_wait) and then the workgroup barrier; a wave must not end before its copies have landed.
__device__ __forceinline__ void lds_copy16(const void* gsrc, void* lds) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc, (__attribute__((address_space(3))) void*)lds, 16, 0, 0);
}
__device__ __forceinline__ void lds_copy_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
__device__ __forceinline__ uint32_t lds_address(const void* p) { return (uint32_t)reinterpret_cast<uintptr_t>(p); }   // LDS aperture: the low 32 bits are the LDS offset

// wave64 inclusive prefix sum of an int (DPP-free, shuffle based)
__device__ __forceinline__ int wave_inclusive_scan(int v) {
    const int lane = threadIdx.x & (PNR_WAVE - 1);
#pragma unroll
    for (int off = 1; off < PNR_WAVE; off <<= 1) {
        int n = __shfl_up(v, off, PNR_WAVE);
        if (lane >= off) v += n;
    }
    return v;
}

}  // namespace pnr

// Run-time switches for A/B measurements and tests (pnr_set_option): `extern int g_opt_<name>` for every line of options.def.  None changes any result.
#include "options.hpp"
