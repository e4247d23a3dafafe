"""Holes of the host's kernel tables (csrc/*.hip: the `<entry>_kernel` selectors) refuse cleanly: PNR_ERR_UNSUPPORTED through the C ABI, before
anything is launched.  No GPU: every call here has to return ahead of its first launch, so the pointers are dummies that nothing may follow.

What cannot be asked on the host is a hole that falls back instead of refusing: a half table with one channel has no run-combining table gradient
and takes the plain kernel on every level (tests/test_gpu_grid_variants.py runs fp16 with C = 1 against float64), a stack without a split-fp16
backward takes the fp32 one (tests/test_gpu_ops.py runs every stack with mlp_f16x3 on and off)."""
import ctypes

import pytest

from palettenerf_amd import _lib

u32, f32, i32, u64 = ctypes.c_uint32, ctypes.c_float, ctypes.c_int, ctypes.c_uint64
UNSUPPORTED = -2
P = ctypes.c_void_p(64)      # a non-null, 16-byte aligned address that is never read


def grid_forward(D, C, dtype, layout=0):
    return _lib.load().pnr_grid_encode_forward_layout(P, P, P, P, u32(8), u32(D), u32(C), u32(4), f32(1.0), u32(16), None, u32(0), i32(0), i32(dtype), i32(layout), None)


@pytest.mark.parametrize("dtype", [0, 1], ids=["fp32", "fp16"])
def test_grid_lookup_has_kernels_for_one_to_five_dimensions_and_power_of_two_channels_only(dtype):
    for D, C in ((3, 3), (3, 0), (3, 5), (3, 6), (3, 7), (3, 16), (1, 3), (5, 3), (0, 2), (6, 2), (6, 3), (0, 0)):
        assert grid_forward(D, C, dtype) == UNSUPPORTED, (D, C)
    # the row layout exists for D = 3, C = 2 alone
    for D, C in ((2, 2), (3, 4), (3, 3)):
        assert grid_forward(D, C, dtype, layout=1) == UNSUPPORTED, (D, C)


def test_grid_lookup_through_the_plain_entry_refuses_three_channels():
    lib = _lib.load()
    assert lib.pnr_grid_encode_forward(P, P, P, P, u32(8), u32(3), u32(3), u32(4), f32(1.0), u32(16), None, u32(0), i32(0), i32(0), None) == UNSUPPORTED


@pytest.mark.parametrize("dtype", [0, 1], ids=["fp32", "fp16"])
def test_grid_table_gradient_refuses_what_has_no_kernel(dtype):
    lib = _lib.load()
    for D, C in ((3, 3), (3, 16), (0, 2), (6, 2)):
        assert lib.pnr_grid_encode_backward(P, P, P, P, P, u32(8), u32(D), u32(C), u32(4), f32(1.0), u32(16), None, None, u32(0), i32(0), i32(dtype), None) == UNSUPPORTED, (D, C)


def mlp_desc(dims, act=0):
    d = _lib.MlpDesc()
    d.n_layers = len(dims) - 1
    for i, v in enumerate(dims):
        d.dims[i] = v
    d.activation = act
    return d


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("dims", [[64, 64, 64, 64], [33, 64, 64, 40]], ids=str)
def test_three_layer_backward_with_two_tiles_at_both_ends_has_no_kernel(dims, act):
    """both orientations of three 64 x 64 layers and the stages are 166 944 bytes of LDS: k_mlp_bwd<3, 2, 2> is the hole of the backward table"""
    lib = _lib.load()
    desc = mlp_desc(dims, act)
    assert lib.pnr_mlp_packed_bytes(ctypes.byref(desc)) > 0                   # the stack itself is a valid one (the forward has its kernel)
    assert lib.pnr_mlp_backward(ctypes.byref(desc), P, P, None, P, u32(8), P, P, P, P, P, u64(1 << 30), None) == UNSUPPORTED
    for opt in (0, 1):                                                        # with and without the split-fp16 kernels
        assert lib.pnr_set_option(b"mlp_f16x3", opt) == 0
        try:
            assert lib.pnr_mlp_backward(ctypes.byref(desc), P, P, None, P, u32(8), P, P, P, P, P, u64(1 << 30), None) == UNSUPPORTED
        finally:
            lib.pnr_set_option(b"mlp_f16x3", 1)


def test_palette_field_has_no_watched_network_heads_kernel():
    """edit mode 3 (the network-heads row) with an overflow flag: the hole of the watched row of the field's table"""
    lib = _lib.load()
    edit = _lib.PaletteEdit()
    edit.mode = 3
    a = _lib.PaletteFieldArgs()
    a.B, a.num_basis, a.clip_dim, a.precision, a.aux_stride = 8, 4, 0, 1, lib.pnr_palette_aux_channels(u32(4), u32(0))
    for name in ("enc", "enc_palette", "dirs", "packed", "sigmas", "rgbs", "aux", "overflow_flag"):
        setattr(a, name, P)
    a.edit = ctypes.cast(ctypes.pointer(edit), ctypes.c_void_p)
    assert lib.pnr_palette_field_forward(ctypes.byref(a), None) == UNSUPPORTED
