// Stand-in for ONE library overload the HIP headers lack: atomicAdd(__half2*, __half2), as CUDA's cuda_fp16.h declares it.  Forced in front of the
// reference's gridencoder.cu (-include, oracle/ref_build.py: build_hip) only when its unmodified build fails; this repository's code, nothing else in it.
// Reached only by the table gradient of an fp16 table with an even feature count: what that path accumulates with is this primitive, not the reference's.
#pragma once
#include <hip/hip_fp16.h>

static inline __device__ __half2 atomicAdd(__half2* address, __half2 val) { return unsafeAtomicAdd(address, val); }
