"""include/pnr_distortion.h held the way tests/test_abi_hull.py holds include/pnr_hull.h: both entries are declared, bound
(palettenerf_amd._lib.DISTORTION_SIGNATURES, beside SIGNATURES and HULL_SIGNATURES, which stay as they are) and exported, the ABI version is
unchanged, and every refusal returns its code before a launch.  No GPU: the pointers are dummies that nothing may follow."""
import ctypes
import os
import re

from palettenerf_amd import _lib

INVALID, OK = -1, 0
P = 64      # a non-null, 16-byte aligned address that is never read
INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
HEADER = os.path.join(INCLUDE, "pnr_distortion.h")
ENTRIES = ["pnr_distortion_backward", "pnr_distortion_forward"]
_ptr, _u32, _f32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_float


def header_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(pnr_[a-z0-9_]+)\s*\(", src)))


def forward(sigmas=P, deltas=P, rays=P, M=100, N=4, dist=P, w_sum=P, wm_sum=P):
    return _lib.load().pnr_distortion_forward(sigmas, deltas, rays, M, N, 1e-4, dist, w_sum, wm_sum, None)


def backward(grad_dist=P, sigmas=P, deltas=P, rays=P, dist=P, w_sum=P, wm_sum=P, M=100, N=4, grad_sigmas=P):
    return _lib.load().pnr_distortion_backward(grad_dist, sigmas, deltas, rays, dist, w_sum, wm_sum, M, N, 1e-4, grad_sigmas, None)


def test_the_entries_are_declared_bound_and_exported_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.pnr_abi_version() == 10
    assert header_symbols() == sorted(_lib.DISTORTION_SIGNATURES) == ENTRIES
    assert not set(_lib.DISTORTION_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.HULL_SIGNATURES))
    header = re.sub(r"\s+", " ", open(HEADER).read())
    assert '#include "pnr.h"' in header
    assert ("int pnr_distortion_forward(const float* sigmas, const float* deltas, const int32_t* rays, uint32_t M, uint32_t N, float T_thresh, "
            "float* dist, float* w_sum, float* wm_sum, pnr_stream_t stream);") in header
    assert ("int pnr_distortion_backward(const float* grad_dist, const float* sigmas, const float* deltas, const int32_t* rays, "
            "const float* dist, const float* w_sum, const float* wm_sum, uint32_t M, uint32_t N, float T_thresh, float* grad_sigmas, "
            "pnr_stream_t stream);") in header
    assert lib.pnr_distortion_forward.argtypes == [_ptr, _ptr, _ptr, _u32, _u32, _f32, _ptr, _ptr, _ptr, _ptr]
    assert lib.pnr_distortion_backward.argtypes == [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _u32, _u32, _f32, _ptr, _ptr]
    assert all(getattr(lib, n).restype is ctypes.c_int for n in ENTRIES)
    assert "pnr_distortion" not in open(os.path.join(INCLUDE, "pnr.h")).read()        # pnr.h and its inventory stay as they are


def test_a_null_array_is_refused_before_a_launch():
    for name in ("sigmas", "deltas", "rays", "dist", "w_sum", "wm_sum"):
        assert forward(**{name: None}) == INVALID, name
    for name in ("grad_dist", "sigmas", "deltas", "rays", "dist", "w_sum", "wm_sum", "grad_sigmas"):
        assert backward(**{name: None}) == INVALID, name
    # without samples the forward reads neither sigmas nor deltas, but still writes its three arrays
    for name in ("rays", "dist", "w_sum", "wm_sum"):
        assert forward(M=0, sigmas=None, deltas=None, **{name: None}) == INVALID, name


def test_nothing_to_do_is_ok_without_a_launch():
    assert forward(N=0) == OK and backward(N=0) == OK
    assert forward(N=0, M=0, sigmas=None, deltas=None, rays=None, dist=None, w_sum=None, wm_sum=None) == OK      # empty tensors have no address
    assert backward(N=0, grad_dist=None, rays=None, dist=None, w_sum=None, wm_sum=None) == OK
    assert backward(M=0) == OK and backward(M=0, sigmas=None, deltas=None, grad_sigmas=None) == OK              # no sample: nothing to write
