"""The training composite with the rgb_norm regulariser on the host: pnr_composite_rays_train_norm_forward / _backward (nerf/renderer.py:301-332,
raymarching.cu:848-882) are declared, bound and validate before any launch; the operator and train_loss's lambda_sparse exist (no GPU needed).
Additive entries: the ABI version stays 10."""
import ctypes
import inspect
import os
import re

from palettenerf_amd import _lib, raymarching
from palettenerf_amd.train_loss import TERM_NAMES, train_loss

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = ("pnr_composite_rays_train_norm_forward", "pnr_composite_rays_train_norm_backward")
INVALID = -1
P = 256     # any non-null address: nothing below reaches a launch


def test_both_entries_are_declared_bound_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pnr.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    vp, f32, u32 = ctypes.c_void_p, ctypes.c_float, ctypes.c_uint32
    # the plain entries' arguments plus rays_gt and rgb_norm (backward: and grad_rgb_norm)
    assert _lib.SIGNATURES[NAMES[0]] == [vp] * 5 + [u32, u32, f32] + [vp] * 5
    assert _lib.SIGNATURES[NAMES[1]] == [vp] * 11 + [u32, u32, f32] + [vp] * 3
    assert len(_lib.SIGNATURES[NAMES[0]]) == len(_lib.SIGNATURES["pnr_composite_rays_train_forward"]) + 2
    assert len(_lib.SIGNATURES[NAMES[1]]) == len(_lib.SIGNATURES["pnr_composite_rays_train_backward"]) + 3
    assert lib.pnr_abi_version() == 10


def test_the_header_cites_the_reference_lines():
    hdr = open(os.path.join(ROOT, "include", "pnr.h")).read()
    block = hdr[:hdr.index("int pnr_composite_rays_train_norm_forward")]
    comment = block[block.rindex("/*"):]
    assert "nerf/renderer.py:301-332" in comment and "raymarching.cu:848-882" in comment


def fwd(lib, M, N, ins, outs):
    return lib.pnr_composite_rays_train_norm_forward(*ins, M, N, 1e-4, *outs, None)


def bwd(lib, M, N, ins, outs):
    return lib.pnr_composite_rays_train_norm_backward(*ins, M, N, 1e-4, *outs, None)


def test_forward_validates_before_any_launch():
    lib = _lib.load()
    assert fwd(lib, 8, 0, [None] * 5, [None] * 4) == 0                # N = 0: nothing is read
    assert fwd(lib, 8, 4, [None] * 5, [None] * 4) == INVALID
    for k in range(5):                                                  # sigmas, rgbs, deltas, rays, rays_gt
        ins = [P] * 5
        ins[k] = None
        assert fwd(lib, 8, 4, ins, [P] * 4) == INVALID, k
    for k in range(4):                                                  # weights_sum, depth, image, rgb_norm
        outs = [P] * 4
        outs[k] = None
        assert fwd(lib, 8, 4, [P] * 5, outs) == INVALID, k


def test_backward_validates_before_any_launch():
    lib = _lib.load()
    assert bwd(lib, 8, 0, [None] * 11, [None] * 2) == 0               # N = 0
    assert bwd(lib, 0, 4, [None] * 11, [None] * 2) == 0               # M = 0: no sample to write, as in the plain backward
    assert bwd(lib, 8, 4, [None] * 11, [None] * 2) == INVALID
    for k in range(11):     # grad_weights_sum, grad_image, grad_rgb_norm, sigmas, rgbs, deltas, rays, rays_gt, weights_sum, image, rgb_norm
        ins = [P] * 11
        ins[k] = None
        assert bwd(lib, 8, 4, ins, [P] * 2) == INVALID, k
    for k in range(2):
        outs = [P] * 2
        outs[k] = None
        assert bwd(lib, 8, 4, [P] * 11, outs) == INVALID, k


def test_the_operator_and_the_loss_weight_exist():
    sig = inspect.signature(raymarching.composite_rays_train_norm)
    assert list(sig.parameters) == ["sigmas", "rgbs", "deltas", "rays", "rays_gt", "T_thresh"]
    assert sig.parameters["T_thresh"].default == 1e-4
    p = inspect.signature(train_loss).parameters
    assert p["lambda_sparse"].default == 0.0
    assert len(TERM_NAMES) == 10
    assert _lib.SIGNATURES["pnr_train_loss_forward"] == _lib.SIGNATURES["pnr_train_loss_backward"]      # (one struct pointer and a stream, as before)
