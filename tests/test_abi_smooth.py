"""The smooth-loss entries on the host: pnr_palette_smooth_points / _forward / _backward (palette/renderer.py:360-378) are declared, bound and
validate before any launch (no GPU needed).  Additive entries: the ABI version stays 10."""
import ctypes
import os
import re

from palettenerf_amd import _lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = ("pnr_palette_smooth_points", "pnr_palette_smooth_forward", "pnr_palette_smooth_backward")
INVALID, UNSUPPORTED = -1, -2
P = 256     # any non-null address: nothing below reaches a launch


def test_the_three_entries_are_declared_bound_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pnr.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    vp, f32, u32 = ctypes.c_void_p, ctypes.c_float, ctypes.c_uint32
    assert _lib.SIGNATURES["pnr_palette_smooth_points"] == [vp, vp, f32, u32, vp, vp]
    assert _lib.SIGNATURES["pnr_palette_smooth_forward"] == [u32] * 3 + [vp] * 8 + [f32] * 4 + [vp] * 3
    assert _lib.SIGNATURES["pnr_palette_smooth_backward"] == [u32] * 3 + [vp] * 11
    assert lib.pnr_abi_version() == 10


def test_the_header_cites_the_reference_block():
    hdr = open(os.path.join(ROOT, "include", "pnr.h")).read()
    block = hdr[:hdr.index("int pnr_palette_smooth_points")]
    assert "palette/renderer.py:360-378" in block[block.rindex("/*"):]


def fwd(lib, M, nb, clip, ptrs, scalars=(1.0, 0.005, 0.2, 0.0), outs=(P, P)):
    return lib.pnr_palette_smooth_forward(M, nb, clip, *ptrs, *scalars, *outs, None)


def test_points_validates_before_any_launch():
    lib = _lib.load()
    assert lib.pnr_palette_smooth_points(None, None, 1.0, 0, None, None) == 0         # M = 0: nothing is read
    for k in range(3):
        args = [P, P, P]
        args[k] = None
        assert lib.pnr_palette_smooth_points(args[0], args[1], 1.0, 8, args[2], None) == INVALID, k


def test_forward_validates_before_any_launch():
    lib = _lib.load()
    none8, full8, noclip = [None] * 8, [P] * 8, [P] * 6 + [None, None]
    for nb, clip in ((0, 0), (17, 0), (4, 129)):
        assert fwd(lib, 8, nb, clip, none8, outs=(None, None)) == UNSUPPORTED, (nb, clip)
        assert fwd(lib, 0, nb, clip, none8, outs=(None, None)) == UNSUPPORTED, (nb, clip)     # the shape is checked first, as in the shade entries
    for nb, clip in ((1, 0), (16, 128), (4, 16)):
        assert fwd(lib, 0, nb, clip, none8, outs=(None, None)) == 0, (nb, clip)          # M = 0
    assert fwd(lib, 8, 4, 16, none8, outs=(None, None)) == INVALID
    for k in range(6):                                                                      # every required input
        ptrs = list(full8)
        ptrs[k] = None
        assert fwd(lib, 8, 4, 16, ptrs) == INVALID, k
    assert fwd(lib, 8, 4, 16, full8, outs=(None, P)) == INVALID and fwd(lib, 8, 4, 16, full8, outs=(P, None)) == INVALID
    assert fwd(lib, 8, 4, 16, [P] * 6 + [P, None]) == INVALID                            # one clip pointer of the pair without the other
    assert fwd(lib, 8, 4, 16, [P] * 6 + [None, P]) == INVALID
    assert fwd(lib, 8, 4, 16, noclip, outs=(None, P)) == INVALID                         # (no clip head is fine; the outputs still must exist)


def bwd(lib, M, nb, clip, ins, outs):
    return lib.pnr_palette_smooth_backward(M, nb, clip, *ins, *outs, None)


def test_backward_validates_before_any_launch():
    lib = _lib.load()
    none6, full6, none4, full4 = [None] * 6, [P] * 6, [None] * 4, [P] * 4
    for nb, clip in ((0, 0), (17, 0), (4, 129)):
        assert bwd(lib, 8, nb, clip, none6, none4) == UNSUPPORTED, (nb, clip)
    assert bwd(lib, 0, 4, 16, none6, none4) == 0                                          # M = 0
    assert bwd(lib, 8, 4, 16, none6, none4) == INVALID
    for k in range(4):                                                                      # grad_smooth_norm, smooth_weight, omega, omega_diff
        ins = list(full6)
        ins[k] = None
        assert bwd(lib, 8, 4, 16, ins, full4) == INVALID, k
    for k in range(2):                                                                      # grad_omega, grad_omega_diff
        outs = list(full4)
        outs[k] = None
        assert bwd(lib, 8, 4, 16, full6, outs) == INVALID, k
    assert bwd(lib, 8, 4, 16, [P] * 4 + [P, None], full4) == INVALID                     # one clip pointer of the pair without the other
    assert bwd(lib, 8, 4, 16, [P] * 4 + [None, P], full4) == INVALID
    assert bwd(lib, 8, 4, 16, [P] * 4 + [None, None], [P, P, P, None]) == INVALID        # a clip gradient asked for without the clip pair
    assert bwd(lib, 8, 4, 16, [P] * 4 + [None, None], [P, P, None, P]) == INVALID
