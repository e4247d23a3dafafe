"""pnr_palette_sheets and pnr_frame_metrics on the device, and the loops over them (palettenerf_amd.evaluate).

Sheets are compared byte for byte with the numpy expressions of the reference (tests/evaluate_reference.py: palette/utils.py:993-1038, :852-909).
Meters are compared with the float64 statements of the same module.  The bound of a meter value is 4 E, E being the error of the SAME statement
evaluated in fp32 by torch on the device -- the project's convention (tests/test_gpu_background_train.py, tests/test_gpu_grid_caps.py); E and the
kernel's error are printed per case (profiles/evaluate/README.md records them).

Shapes: 6 x 6 is the smallest view SSIM accepts (the reflected border needs 6 pixels), 13 x 37 is odd with rows shorter than a tile plus its
halo, 45 x 70 has two ragged 32 x 32 tiles each way; nb 4, 5 and 8; maps contiguous and as columns of one buffer whose row is the frame call's aux
row for that nb (pnr_palette_aux_channels)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from palettenerf_amd import _lib, palette_utils, pipeline, scene
from palettenerf_amd import evaluate as ev
from palettenerf_amd import rays as prays
from palettenerf_amd._torch_glue import stream_ptr
from tests import evaluate_reference as ref
from tests.test_gpu_jitter import make_model

pytestmark = pytest.mark.gpu

SHAPES = [(6, 6), (13, 37), (45, 70)]
SENTINEL = 0xAB
KW = dict(max_steps=1024, T_thresh=1e-4)
IN_KEYS = ("image", "depth", "view_dep_rgb", "direct_rgb", "basis_rgb", "unscaled_basis_rgb", "basis_acc", "gt_weights", "basis_color")
OUT_OF = {"rgb": "image", "depth": "depth", "view_dep": "view_dep_rgb", "direct": "direct_rgb", "basis_img": "basis_rgb",
          "unscaled_basis_img": "unscaled_basis_rgb", "basis_acc": "basis_acc", "weights_guide": "gt_weights", "basis_color": "basis_color"}
FIELDS = {"rgb": "out_rgb", "depth": "out_depth", "view_dep": "out_view_dep", "direct": "out_direct", "basis_img": "out_basis_img",
          "unscaled_basis_img": "out_unscaled_basis_img", "basis_acc": "out_basis_acc", "weights_guide": "out_weights_guide", "basis_color": "out_basis_color"}
STRIDES = {"image": "image_stride", "depth": "depth_stride", "view_dep_rgb": "view_dep_stride", "direct_rgb": "direct_stride",
           "basis_rgb": "basis_rgb_stride", "unscaled_basis_rgb": "unscaled_stride", "basis_acc": "basis_acc_stride", "gt_weights": "gt_weights_stride"}


def cols_of(key, nb):
    return {"image": 3, "depth": 1, "view_dep_rgb": 3, "direct_rgb": 3, "basis_rgb": 3 * nb, "unscaled_basis_rgb": 3 * nb, "basis_acc": nb,
            "gt_weights": nb}[key]


def out_shape(name, H, W, nb):
    return {"rgb": (H, W, 3), "depth": (H, W), "view_dep": (H, W, 3), "direct": (H, W, 3), "basis_img": (H, nb * W, 3),
            "unscaled_basis_img": (H, nb * W, 3), "basis_acc": (H, nb * W), "weights_guide": (H, nb * W), "basis_color": (100, nb * 100, 3)}[name]


def special_values():
    """below 0, above 1, exactly 0 and 1, every k / 255 as fp32 with its two neighbours: the values at which a byte changes"""
    k = (np.arange(256, dtype=np.float64) / 255).astype(np.float32)
    return np.concatenate([k, np.nextafter(k, np.float32(-1)), np.nextafter(k, np.float32(2)),
                           np.array([-0.5, -1e-8, 0.0, 1.0, 1.0 + 1e-6, 1.5, 3.0, 0.999999], np.float32)])


def make_maps(cuda, H, W, nb, layout, seed, in_range=False):
    """The maps of one frame as device tensors [HW, cols] (depth [HW]): random in [-0.3, 1.3] with the special values scattered in (in_range:
    everything in [0, 1], as a rendered colour is).  layout "aux": the five aux maps are columns of one [HW, aux channels] buffer."""
    rng = np.random.default_rng(seed)
    n = H * W
    sp = special_values()
    host = {}
    for key in IN_KEYS[:-1]:
        v = rng.uniform(-0.3, 1.3, size=(n, cols_of(key, nb))).astype(np.float32)
        flat = v.reshape(-1)
        where = rng.choice(flat.size, size=min(flat.size // 2, sp.size), replace=False)
        flat[where] = rng.permutation(sp)[:where.size]
        host[key] = v.clip(0, 1) if in_range else v
    host["depth"] = host["depth"].reshape(n)
    host["basis_color"] = rng.uniform(-0.2, 1.2, size=(nb, 3)).astype(np.float32)
    dev = {k: torch.from_numpy(v).to(cuda) for k, v in host.items()}
    if layout == "aux":
        ch = int(_lib.load().pnr_palette_aux_channels(nb, 0))
        aux = torch.full((n, ch), 7.0, dtype=torch.float32, device=cuda)
        for key, c0 in (("direct_rgb", 0), ("view_dep_rgb", 3), ("basis_acc", 6), ("basis_rgb", 6 + nb), ("unscaled_basis_rgb", 6 + 4 * nb)):
            aux[:, c0:c0 + cols_of(key, nb)] = dev[key]
            dev[key] = aux[:, c0:c0 + cols_of(key, nb)]
            assert not dev[key].is_contiguous() or n == 1
    return host, dev


def run_sheets(dev, H, W, nb, names, srgb=False, offset=0):
    """pnr_palette_sheets with exactly the outputs in `names`, every output a view `offset` bytes into a sentinel-filled buffer with 8 guard bytes
    behind it.  Inputs are passed for the requested outputs only (a NULL input: that sheet is not written).  Returns {name: (buffer, view)}."""
    a = _lib.SheetArgs()
    a.H, a.W, a.num_basis, a.linear_to_srgb = H, W, nb, int(srgb)
    outs = {}
    for key in ("image", "depth"):
        a.__setattr__(key, dev[key].data_ptr())
        a.__setattr__(STRIDES[key], dev[key].stride(0))
    for name in names:
        key = OUT_OF[name]
        t = dev[key]
        setattr(a, key, t.data_ptr())
        if key in STRIDES:
            setattr(a, STRIDES[key], t.stride(0))
        size = int(np.prod(out_shape(name, H, W, nb)))
        buf = torch.full((offset + size + 8,), SENTINEL, dtype=torch.uint8, device=t.device)
        outs[name] = (buf, buf[offset:offset + size].view(out_shape(name, H, W, nb)))
        setattr(a, FIELDS[name], outs[name][1].data_ptr())
        assert outs[name][1].data_ptr() % 4 == offset % 4
    _lib.check(_lib.load().pnr_palette_sheets(ctypes.byref(a), stream_ptr()), "pnr_palette_sheets")
    return outs


def check_guards(outs, offset):
    for name, (buf, view) in outs.items():
        n = view.numel()
        assert bool((buf[:offset] == SENTINEL).all()) and bool((buf[offset + n:] == SENTINEL).all()), f"{name}: bytes outside the image were written"


# ---------------------------------------------------------------- 1. sheets, bit for bit
@pytest.mark.parametrize("layout", ["contiguous", "aux"])
@pytest.mark.parametrize("nb", [4, 5, 8])
@pytest.mark.parametrize("H,W", SHAPES)
def test_every_sheet_equals_the_reference_expression(cuda, H, W, nb, layout):
    host, dev = make_maps(cuda, H, W, nb, layout, seed=H * 1000 + W * 10 + nb)
    want = ref.sheets(host, H, W, nb)
    names = list(OUT_OF)
    aligned = run_sheets(dev, H, W, nb, names)
    check_guards(aligned, 0)
    for name in names:
        got = aligned[name][1].cpu().numpy()
        assert got.shape == want[name].shape, name
        np.testing.assert_array_equal(got, want[name], err_msg=f"{name} {H}x{W} nb={nb} {layout}")
    # an output that starts at byte 1, 2, 3 of a dword: the same bytes, nothing outside them
    for offset in (1, 2, 3):
        shifted = run_sheets(dev, H, W, nb, names, offset=offset)
        check_guards(shifted, offset)
        for name in names:
            assert torch.equal(shifted[name][1], aligned[name][1]), (name, offset)
    # the public call on a result dict gives the same tensors
    r = {k: dev[k] for k in ("image", "depth", "view_dep_rgb", "direct_rgb", "basis_rgb", "unscaled_basis_rgb", "basis_acc")}
    sh = ev.frame_sheets(r, H, W, nb, basis_color=dev["basis_color"], gt_weights=dev["gt_weights"])
    assert sorted(sh) == sorted(names)
    for name in names:
        assert sh[name].dtype == torch.uint8 and torch.equal(sh[name], aligned[name][1]), name


@pytest.mark.parametrize("H,W", SHAPES)
def test_rgb_and_depth_sheets_are_render_paths_bytes(cuda, H, W):
    """On a frame's own maps (colour in [0, 1], where the clip of palette/utils.py:999 changes nothing) the rgb and depth sheets are the bytes
    rays.image_to_uint8 gives render_path -- with and without linear_to_srgb.  The sRGB branch's powf is not correctly rounded on either side:
    against numpy's it may differ by one level at a byte boundary (the allowance of the pnr_image_to_uint8 test); against the project's own
    expression it may not differ at all."""
    host, dev = make_maps(cuda, H, W, 4, "contiguous", seed=H + W, in_range=True)
    for srgb in (False, True):
        outs = run_sheets(dev, H, W, 4, ["rgb", "depth"], srgb=srgb)
        assert torch.equal(outs["rgb"][1], prays.image_to_uint8(dev["image"].reshape(H, W, 3), srgb))
        assert torch.equal(outs["depth"][1], prays.image_to_uint8(dev["depth"].reshape(H, W), False))
        want = ref.sheets(host, H, W, 4, linear_to_srgb=srgb)
        got = outs["rgb"][1].cpu().numpy()
        diff = np.abs(got.astype(np.int32) - want["rgb"].astype(np.int32))
        print(f"{H}x{W} srgb={srgb}: {int((diff != 0).sum())} of {diff.size} rgb bytes differ from numpy")
        assert diff.max() <= (1 if srgb else 0)
        np.testing.assert_array_equal(outs["depth"][1].cpu().numpy(), want["depth"])


def test_a_null_input_leaves_its_output_untouched_and_a_nerf_result_gives_two_sheets(cuda):
    H, W, nb = 13, 37, 5
    host, dev = make_maps(cuda, H, W, nb, "aux", seed=5)
    want = ref.sheets(host, H, W, nb)
    # one sentinel buffer for all nine images back to back; only four inputs are given
    sizes = {name: int(np.prod(out_shape(name, H, W, nb))) for name in OUT_OF}
    start, pos = {}, 0
    for name in OUT_OF:
        start[name], pos = pos, pos + sizes[name]
    buf = torch.full((pos,), SENTINEL, dtype=torch.uint8, device=cuda)
    given = ["rgb", "direct", "basis_acc", "basis_color"]
    a = _lib.SheetArgs()
    a.H, a.W, a.num_basis = H, W, nb
    a.image, a.image_stride, a.depth, a.depth_stride = dev["image"].data_ptr(), 3, dev["depth"].data_ptr(), 1
    for name in given:
        key = OUT_OF[name]
        setattr(a, key, dev[key].data_ptr())
        if key in STRIDES:
            setattr(a, STRIDES[key], dev[key].stride(0))
        setattr(a, FIELDS[name], buf.data_ptr() + start[name])
    _lib.check(_lib.load().pnr_palette_sheets(ctypes.byref(a), stream_ptr()), "pnr_palette_sheets")
    got = buf.cpu().numpy()
    for name in OUT_OF:
        part = got[start[name]:start[name] + sizes[name]]
        if name in given:
            np.testing.assert_array_equal(part.reshape(want[name].shape), want[name], err_msg=name)
        else:
            assert (part == SENTINEL).all(), name
    # a NeRF result, and a gui_mode result (no per-basis maps): rgb and depth only
    sh = ev.frame_sheets({"image": dev["image"], "depth": dev["depth"]}, H, W)
    assert sorted(sh) == ["depth", "rgb"]
    np.testing.assert_array_equal(sh["rgb"].cpu().numpy(), want["rgb"])
    np.testing.assert_array_equal(sh["depth"].cpu().numpy(), want["depth"])


# ---------------------------------------------------------------- 2. meters against float64
def image_pair(kind, H, W, C, seed):
    """pred [H,W,3] and truth [H,W,C] fp32 (host): textured noise, a smooth ramp with slight noise, flat 0.7 +- 0.002; alpha in {0, 0.3, 1}."""
    g = torch.Generator().manual_seed(seed)
    if kind == "textured":
        pred, rgb = torch.rand(H, W, 3, generator=g), torch.rand(H, W, 3, generator=g)
    elif kind == "ramp":
        yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
        base = torch.stack([0.1 + 0.8 * xx, 0.1 + 0.8 * yy, 0.5 + 0.4 * (xx - yy)], dim=-1)
        pred = (base + 0.01 * torch.randn(H, W, 3, generator=g)).clamp(0, 1)
        rgb = (base + 0.01 * torch.randn(H, W, 3, generator=g)).clamp(0, 1)
    else:
        pred = 0.7 + 0.002 * (2 * torch.rand(H, W, 3, generator=g) - 1)
        rgb = 0.7 + 0.002 * (2 * torch.rand(H, W, 3, generator=g) - 1)
    if C == 4:
        alpha = torch.tensor([0.0, 0.3, 1.0])[torch.randint(0, 3, (H, W, 1), generator=g)]
        return pred.float(), torch.cat([rgb, alpha], dim=-1).float()
    return pred.float(), rgb.float()


def weights_map(H, W, nb, seed):
    g = torch.Generator().manual_seed(seed + 77)
    w = torch.rand(H, W, nb, generator=g) ** 3
    w[0, 0] = 0.0            # a pixel without any weight: the 1e-6 of the sparsity term decides
    w[-1, -1] = 1.0
    return w.float()


def device_frame(cuda, pred, truth, omega, strided):
    """The maps on the device; strided: pred and omega are columns of wider buffers (the aux row of that nb)."""
    nb = omega.shape[-1]
    H, W = pred.shape[:2]
    if not strided:
        return pred.to(cuda), truth.to(cuda), omega.to(cuda)
    ch = int(_lib.load().pnr_palette_aux_channels(nb, 0))
    aux = torch.full((H * W, ch), 9.0, dtype=torch.float32, device=cuda)
    aux[:, 6:6 + nb] = omega.reshape(-1, nb).to(cuda)
    wide = torch.full((H * W, 5), 9.0, dtype=torch.float32, device=cuda)
    wide[:, 1:4] = pred.reshape(-1, 3).to(cuda)
    return wide[:, 1:4].reshape(H, W, 3), truth.to(cuda), aux[:, 6:6 + nb].reshape(H, W, nb)


def kernel_values(pred, truth, omega, srgb, want=("psnr", "ssim", "sparsity", "tv", "mse")):
    ms = ev.MeterSet(omega.shape[-1] if omega is not None else None, want=want)
    out = torch.zeros(8, dtype=torch.float64, device=pred.device)
    ms.update(pred, truth, omega, srgb_to_linear_truth=srgb, frame_out=out)
    f = out.cpu().tolist()
    assert f[0] == 1.0 and f[6] == 0.0 and f[7] == 0.0
    return dict(zip(("mse", "psnr", "ssim", "sparsity", "tv"), f[1:6])), ms


@pytest.mark.parametrize("kind", ["textured", "ramp", "flat"])
@pytest.mark.parametrize("H,W,nb", [(6, 6, 4), (13, 37, 5), (45, 70, 8)])
def test_meters_are_within_four_times_the_fp32_error_of_float64(cuda, H, W, nb, kind):
    for C in (3, 4):
        for srgb in (False, True):
            seed = H * W + 10 * C + int(srgb)
            pred, truth = image_pair(kind, H, W, C, seed)
            omega = weights_map(H, W, nb, seed)
            exact = ref.metrics(pred, truth, omega, srgb, torch.float64, "cpu")
            fp32 = ref.metrics(pred, truth, omega, srgb, torch.float32, cuda)
            got, _ = kernel_values(*device_frame(cuda, pred, truth, omega, strided=(C == 4)), srgb)
            for k in ("mse", "psnr", "ssim", "sparsity", "tv"):
                E, err = abs(fp32[k] - exact[k]), abs(got[k] - exact[k])
                print(f"{kind} {H}x{W} nb={nb} C={C} srgb={int(srgb)} {k}: float64 {exact[k]:.12g}  E(fp32 torch) {E:.3g}  kernel {err:.3g}")
                assert err <= 4 * E, f"{kind} {H}x{W} C={C} srgb={srgb} {k}: kernel error {err} against 4 x {E}"


def test_the_ground_truth_colour_and_the_want_mask(cuda):
    H, W, nb = 13, 37, 5
    pred, truth = image_pair("textured", H, W, 4, 3)
    omega = weights_map(H, W, nb, 3)
    p, t, w = device_frame(cuda, pred, truth, omega, strided=True)
    for srgb in (False, True):
        gt = torch.full((H, W, 3), -1.0, dtype=torch.float32, device=cuda)
        ms = ev.MeterSet(nb)
        ms.update(p, t, w, srgb_to_linear_truth=srgb, truth_rgb_out=gt)
        want = ref.ground_truth(truth, srgb)                      # float64; the kernel rounds its double once to fp32
        assert float((gt.cpu().double() - want).abs().max()) <= 2.0 ** -24
    full, _ = kernel_values(p, t, w, False)
    only, _ = kernel_values(p, t, w, False, want=("ssim",))
    assert only["ssim"] == full["ssim"] and only["mse"] == 0.0 and only["psnr"] == 0.0 and only["sparsity"] == 0.0 and only["tv"] == 0.0
    nopal, _ = kernel_values(p, t, None, False)
    assert nopal["psnr"] == full["psnr"] and nopal["ssim"] == full["ssim"] and nopal["sparsity"] == 0.0 and nopal["tv"] == 0.0
    small, _ = kernel_values(p[:4, :3], t[:4, :3].contiguous(), w[:4, :3], False, want=("psnr", "sparsity", "tv"))   # below SSIM's size: legal without it
    mse = float(((pred[:4, :3].double() - ref.ground_truth(truth[:4, :3])) ** 2).mean())
    assert abs(small["tv"] - float(ref.tv(omega[:4, :3].double()))) < 1e-12 and abs(small["sparsity"] - float(ref.sparsity(omega[:4, :3].double()))) < 1e-12
    assert abs(small["mse"] - mse) < 1e-15 and abs(small["psnr"] + 10 * np.log10(mse)) < 1e-12 and small["ssim"] == 0.0


# ---------------------------------------------------------------- 3. totals
def test_totals_are_the_sum_of_the_frames_and_reproducible(cuda):
    H, W, nb = 45, 70, 5
    frames = []
    for s in range(3):
        pred, truth = image_pair(("textured", "ramp", "flat")[s], H, W, 3 + (s % 2), 100 + s)
        frames.append(device_frame(cuda, pred, truth, weights_map(H, W, nb, s), strided=bool(s % 2)))

    def run():
        ms = ev.MeterSet(nb, want=("psnr", "ssim", "sparsity", "tv", "mse"))
        rows = torch.zeros(3, 8, dtype=torch.float64, device=cuda)
        for s, (p, t, w) in enumerate(frames):
            ms.update(p, t, w, frame_out=rows[s])
        return ms, rows.cpu(), ms._totals.cpu().clone()

    ms, rows, totals = run()
    acc = torch.zeros(8, dtype=torch.float64)
    for s in range(3):
        acc = acc + rows[s]                                          # the order the launches added them in
    assert torch.equal(totals, acc) and float(totals[0]) == 3.0
    assert all(float(rows[s, k]) != 0.0 for s in range(3) for k in range(1, 6))
    ms2, rows2, totals2 = run()
    assert torch.equal(rows2, rows) and torch.equal(totals2, totals)  # the same bits
    psnr, ssim, sparsity, tv = ms.meters()
    assert (psnr.basis_metric if hasattr(psnr, "basis_metric") else False) is False and sparsity.basis_metric and tv.basis_metric
    for meter, k in ((psnr, 2), (ssim, 3), (sparsity, 4), (tv, 5)):
        assert meter.measure() == float(totals[k]) / float(totals[0])
        assert meter.report().startswith(meter.label + " = ")
    ms.clear()
    assert ms.totals()[0] == 0.0
    # the meters used alone, in the reference's shapes ([B,H,W,*]): the same per-frame values
    alone = [ev.PSNRMeter(), ev.SSIMMeter(), ev.SparsityMeter(nb), ev.TVMeter(nb)]
    for p, t, w in frames:
        alone[0].update(p[None], t[None][..., :3] if t.shape[-1] == 3 else t[None])
        alone[1].update(p[None], t[None])
        alone[2].update(w[None])
        alone[3].update(w[None])
    for meter, k in zip(alone, (2, 3, 4, 5)):
        assert meter.measure() == float(totals[k]) / 3.0
        meter.clear()


# ---------------------------------------------------------------- 4. end to end
def path_setup(cuda, kind):
    m = make_model(kind, cuda, 0, 100.0 if kind == "palette" else 1.0)
    H, W = 45, 70
    intr = scene.intrinsics_from_fov(H, W)
    poses = np.stack([scene.lookat_pose(azimuth_deg=30.0 + 40.0 * i) for i in range(3)])
    g = torch.Generator().manual_seed(11)
    images = torch.rand(3, H, W, 4, generator=g)
    return m, H, W, intr, poses, images


@pytest.mark.parametrize("kind", ["palette", "nerf"])
def test_evaluate_path_equals_the_meters_on_plain_renders(cuda, kind):
    m, H, W, intr, poses, images = path_setup(cuda, kind)
    palette = kind == "palette"
    nb = m.num_basis if palette else None
    if palette:
        g = torch.Generator().manual_seed(12)
        m.hist_weights = torch.rand(1, nb, 8, 8, 8, generator=g).to(cuda)
    seen = []
    out = ev.evaluate_path(m, poses, intr, H, W, images, sheets=True, consume=lambda i, r, sh: seen.append((i, {k: v.clone() for k, v in sh.items()})), **KW)
    ms = ev.MeterSet(nb, want=("psnr", "ssim", "sparsity", "tv", "mse"))
    extra = {"gui_mode": False} if palette else {}
    with torch.no_grad():
        for i in range(3):
            ro, rd = prays.rays_from_indices(torch.from_numpy(poses[i:i + 1]).to(cuda), intr, H, W, None)
            r = m.render(ro, rd, bg_color=1, perturb=False, **extra, **KW)
            gt = torch.empty(H, W, 3, dtype=torch.float32, device=cuda)
            ms.update(r["image"].reshape(H, W, 3), images[i].to(cuda), r["basis_acc"].reshape(H, W, nb) if palette else None, truth_rgb_out=gt)
            gw = palette_utils.get_palette_weight_with_hist(gt, m.hist_weights) if palette else None
            sh = ev.frame_sheets(r, H, W, nb, m.basis_color if palette else None, gw)
            assert seen[i][0] == i and sorted(seen[i][1]) == sorted(sh)
            assert sorted(sh) == (sorted(OUT_OF) if palette else ["depth", "rgb"])
            for k in sh:
                assert torch.equal(seen[i][1][k], sh[k]), (i, k)
    t = ms.totals()
    assert out["frames"] == 3 and t[0] == 3.0
    want = {"loss": t[1] / 3, "PSNR": t[2] / 3, "SSIM": t[3] / 3}
    if palette:
        want.update({"Sparsity": t[4] / 3, "TV": t[5] / 3})
    assert sorted(out) == sorted(list(want) + ["frames"])            # no palette meters for a NeRF model
    for k, v in want.items():
        assert out[k] == v and np.isfinite(v), (k, out[k], v)


@pytest.mark.parametrize("kind", ["palette", "nerf"])
def test_test_path_writes_its_files_and_agrees_with_render_path(cuda, tmp_path, kind):
    m, H, W, intr, poses, _ = path_setup(cuda, kind)
    kw = dict(perturb=False, bg_color=1, **KW)
    sh = ev.test_path(m, poses, intr, H, W, save_path=str(tmp_path), name="run", **kw)
    suffix = {"rgb": "rgb", "depth": "depth", "basis_img": "basis_img", "basis_acc": "basis_acc", "basis_color": "basis_color", "view_dep_color": "view_dep"}
    if kind == "nerf":
        suffix = {"rgb": "rgb", "depth": "depth"}
        assert sorted(sh) == ["depth", "rgb"]
    else:
        assert sorted(sh) == sorted(suffix.values())
        assert sh["basis_img"].shape == (3, H, m.num_basis * W, 3) and sh["basis_color"].shape == (3, 100, m.num_basis * 100, 3)
    assert sorted(os.listdir(tmp_path)) == sorted(f"run_{t:04d}_{s}.png" for t in range(3) for s in suffix)
    for t in range(3):
        for s, key in suffix.items():
            img = ref.decode_png(str(tmp_path / f"run_{t:04d}_{s}.png"))
            assert img.dtype == np.uint8 and np.array_equal(img, sh[key][t]), (t, s)
    assert sh["rgb"].std() > 0
    # the untouched path: render_path's bytes over the same poses are the rgb and depth sheets
    rgb, dep = pipeline.render_path(m, poses, intr, H, W, frames_in_flight=1, **kw)
    assert np.array_equal(rgb, sh["rgb"]) and np.array_equal(dep, sh["depth"])
    dev = ev.test_path(m, poses[:1], intr, H, W, to_host=False, **kw)
    assert dev["rgb"].is_cuda and np.array_equal(dev["rgb"].cpu().numpy()[0], sh["rgb"][0])
