"""pnr_palette_sheets / pnr_frame_metrics on the host (no GPU: every check below returns before a launch), the PNG writer, and the float64 SSIM
statement the device meter is held to."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from palettenerf_amd import _lib
from palettenerf_amd import evaluate as ev
from tests import evaluate_reference as ref

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
OK, INVALID = 0, -1
P = 256   # a non-NULL "pointer": nothing is dereferenced before the checks fail


@pytest.mark.parametrize("cname,mirror,nfields", [("pnr_sheet_args", _lib.SheetArgs, 30), ("pnr_metrics_args", _lib.MetricsArgs, 16)])
def test_struct_layout_is_the_headers(tmp_path, cname, mirror, nfields):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pnr.h"', 'int main(void) {', f'  printf("{cname} %zu\\n", sizeof({cname}));']
    for fname, *_ in mirror._fields_:
        lines.append(f'  printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['  printf("bits %d %d %d %d %d %d\\n", PNR_METRIC_MSE, PNR_METRIC_PSNR, PNR_METRIC_SSIM, PNR_METRIC_SPARSITY, PNR_METRIC_TV, PNR_SHEET_MAX_BASIS);',
              '  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    rows = [line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()]
    got = {r[0]: r[1] for r in rows if r[0] != "bits"}
    assert int(got[cname]) == ctypes.sizeof(mirror)
    for fname, *_ in mirror._fields_:
        assert int(got[f"{cname}.{fname}"]) == getattr(mirror, fname).offset, fname
    assert len(mirror._fields_) == nfields
    bits = [int(v) for v in next(r for r in rows if r[0] == "bits")[1:]]
    assert bits == [_lib.METRIC_MSE, _lib.METRIC_PSNR, _lib.METRIC_SSIM, _lib.METRIC_SPARSITY, _lib.METRIC_TV, _lib.SHEET_MAX_BASIS]


def test_the_abi_stays_10_and_the_entries_exist():
    lib = _lib.load()
    assert lib.pnr_abi_version() == 10
    assert _lib.SIGNATURES["pnr_palette_sheets"] == [ctypes.c_void_p] * 2
    assert _lib.SIGNATURES["pnr_frame_metrics"] == [ctypes.c_void_p] * 2
    assert lib.pnr_frame_metrics_workspace_bytes(32, 32) == 64 + 8 * 8
    assert lib.pnr_frame_metrics_workspace_bytes(45, 70) == 64 + 2 * 3 * 8 * 8
    assert lib.pnr_frame_metrics_workspace_bytes(800, 800) == 64 + 625 * 8 * 8


def sheet_args(nb=4):
    a = _lib.SheetArgs()
    a.H, a.W, a.num_basis = 6, 6, nb
    a.image, a.depth, a.image_stride, a.depth_stride = P, P, 3, 1
    return a


def test_sheet_argument_errors():
    call = lambda a: _lib.load().pnr_palette_sheets(ctypes.byref(a), None)
    assert _lib.load().pnr_palette_sheets(None, None) == INVALID
    assert call(_lib.SheetArgs()) == OK                                  # an empty frame: nothing to do, nothing is read
    a = sheet_args()
    a.H = 0
    a.image = None
    assert call(a) == OK
    for missing in ("image", "depth"):
        a = sheet_args()
        setattr(a, missing, None)
        assert call(a) == INVALID, missing
    for nb in (0, 9, 100):                                               # nb outside 1 .. 8
        a = sheet_args(nb)
        a.basis_acc, a.basis_acc_stride, a.out_basis_acc = P, max(nb, 1), P
        assert call(a) == INVALID, nb
    assert call(sheet_args(9)) == INVALID
    for out, inp in (("out_view_dep", "view_dep_rgb"), ("out_direct", "direct_rgb"), ("out_basis_img", "basis_rgb"),
                     ("out_unscaled_basis_img", "unscaled_basis_rgb"), ("out_basis_acc", "basis_acc"), ("out_weights_guide", "gt_weights"),
                     ("out_basis_color", "basis_color")):
        a = sheet_args()
        setattr(a, out, P)                                               # an output without its input
        assert call(a) == INVALID, out
    for inp, stride, short in (("view_dep_rgb", "view_dep_stride", 2), ("direct_rgb", "direct_stride", 2), ("basis_rgb", "basis_rgb_stride", 11),
                               ("unscaled_basis_rgb", "unscaled_stride", 11), ("basis_acc", "basis_acc_stride", 3), ("gt_weights", "gt_weights_stride", 3)):
        a = sheet_args()
        setattr(a, inp, P)
        setattr(a, stride, short)                                        # rows shorter than their columns
        assert call(a) == INVALID, inp
    a = sheet_args()
    a.image_stride = 2
    assert call(a) == INVALID
    a = sheet_args()                                                     # inputs only, no output asked for: nothing to launch
    assert call(a) == OK


def metric_args(H=6, W=6, want=31):
    a = _lib.MetricsArgs()
    a.H, a.W, a.pred, a.pred_stride, a.truth, a.truth_channels, a.want = H, W, P, 3, P, 3, want
    a.totals, a.workspace, a.workspace_bytes = P, P, _lib.load().pnr_frame_metrics_workspace_bytes(H, W)
    return a


def test_metric_argument_errors():
    call = lambda a: _lib.load().pnr_frame_metrics(ctypes.byref(a), None)
    assert _lib.load().pnr_frame_metrics(None, None) == INVALID
    assert call(_lib.MetricsArgs()) == OK                                # an empty view touches nothing
    for missing in ("pred", "truth", "totals", "workspace"):
        a = metric_args()
        setattr(a, missing, None)
        assert call(a) == INVALID, missing
    for C in (0, 1, 2, 5):
        a = metric_args()
        a.truth_channels = C
        assert call(a) == INVALID, C
    for H, W in ((5, 6), (6, 5), (1, 40), (40, 3)):                      # SSIM's reflected border needs more than 5 pixels each way
        assert call(metric_args(H, W, _lib.METRIC_SSIM)) == INVALID, (H, W)
    for H, W in ((1, 8), (8, 1)):                                        # TV needs a neighbour each way
        a = metric_args(H, W, _lib.METRIC_TV)
        a.basis_acc, a.basis_acc_stride, a.num_basis = P, 4, 4
        assert call(a) == INVALID, (H, W)
    for nb, stride in ((0, 4), (11, 11), (4, 3)):
        a = metric_args()
        a.basis_acc, a.basis_acc_stride, a.num_basis = P, stride, nb
        assert call(a) == INVALID, (nb, stride)
    a = metric_args(45, 70)
    a.workspace_bytes -= 1                                               # too small a workspace
    assert call(a) == INVALID
    a = metric_args()
    a.workspace = P + 4                                                  # doubles live in it
    assert call(a) == INVALID
    a = metric_args()
    a.pred_stride = 2
    assert call(a) == INVALID


@pytest.mark.parametrize("shape", [(1, 1), (7, 13), (13, 7, 3), (1, 5, 3), (45, 281), (45, 70, 3)])
def test_png_files_decode_to_the_same_bytes(tmp_path, shape):
    img = np.random.default_rng(sum(shape)).integers(0, 256, size=shape, dtype=np.uint8)
    path = str(tmp_path / "a.png")
    ev.write_png(path, img)
    back = ref.decode_png(path)
    assert back.dtype == np.uint8 and back.shape == img.shape and np.array_equal(back, img)
    ev.write_png(path, img[:, ::-1])                                     # a view with negative strides is written as it looks
    assert np.array_equal(ref.decode_png(path), img[:, ::-1])


def test_png_writer_refuses_what_it_cannot_write(tmp_path):
    for bad in (np.zeros((4, 4), np.float32), np.zeros((4, 4, 4), np.uint8), np.zeros((0, 4), np.uint8), np.zeros(4, np.uint8)):
        with pytest.raises(ValueError):
            ev.write_png(str(tmp_path / "b.png"), bad)


def images(H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(H, W, 3, generator=g, dtype=torch.float64), torch.rand(H, W, 3, generator=g, dtype=torch.float64)


@pytest.mark.parametrize("H,W", [(6, 6), (13, 37), (45, 70)])
def test_float64_ssim_of_identical_images_and_symmetry(H, W):
    a, b = images(H, W, H * W)
    # Identical images: numerator and denominator of S are the same double per pixel (2 m m = m m + m m and 2 s = s + s exactly), so without the
    # 1e-12 in the denominator S = 1 and the meter is exactly 1 ...
    assert float(ref.ssim(a, a, eps=0.0)) == 1.0
    # ... and with it S = n / (n + 1e-12) with n >= C1 C2 (both variances are 0 at least up to rounding: allow 1 %), so 0 <= 1 - SSIM <= 1e-12 / (C1 C2)
    d = 1.0 - float(ref.ssim(a, a))
    assert 0.0 <= d <= 1.01 * ref.EPS / (ref.C1 * ref.C2), d
    # symmetric in its arguments, bit for bit: every product and sum in S is commutative
    assert float(ref.ssim(a, b)) == float(ref.ssim(b, a))
    assert float(ref.ssim(a, b)) < 0.5                                   # (unrelated noise is far from similar)
    # fp32 evaluation of the same text stays close on a textured image (the E of the device test)
    assert abs(float(ref.ssim(a.float(), b.float())) - float(ref.ssim(a, b))) < 1e-5


def test_the_reference_statements_on_a_case_done_by_hand():
    # 2 x 2 x nb = 2 weights: sparsity and TV written out
    w = torch.tensor([[[1.0, 0.0], [0.5, 0.5]], [[0.0, 0.0], [0.25, 0.75]]], dtype=torch.float64)
    sp = [1 / (1 + 1e-6) - 1, 1 / (0.5 + 1e-6) - 1, 0 / 1e-6 - 1, 1 / (0.625 + 1e-6) - 1]
    assert abs(float(ref.sparsity(w)) - sum(sp) / 4) < 1e-15
    wv = (0.25 + 0.25 + 0.0625 + 0.5625) / 4
    hv = (1.0 + 0.0 + 0.0625 + 0.0625) / 4
    assert abs(float(ref.tv(w)) - 100 * (wv + hv)) < 1e-13
    t = torch.tensor([[[0.2, 0.4, 0.04, 0.5]]], dtype=torch.float32)
    gt = ref.ground_truth(t)
    assert torch.allclose(gt, torch.tensor([[[0.6, 0.7, 0.52]]], dtype=torch.float64), atol=1e-7)
    lin = ref.ground_truth(t[..., :3], srgb=True)
    want = [((0.2 + 0.055) / 1.055) ** 2.4, ((0.4 + 0.055) / 1.055) ** 2.4, 0.04 / 12.92]
    assert torch.allclose(lin, torch.tensor([[want]], dtype=torch.float64), atol=1e-7)
    # the byte expression: clip, times 255, truncate
    assert ref.to_u8([-0.5, 0.0, 0.999, 1.0, 7.0, 128 / 255]).tolist() == [0, 0, 254, 255, 255, 128]
    assert ref.to_u8([0.5, 1.5], clip=False).tolist() == [127, 382 - 256]
